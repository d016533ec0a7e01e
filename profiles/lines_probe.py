"""Cost of the line filter on the config-2 text (100 MB of English) resident in HBM, 20 lines of the text to a document:
wp_filter_lines_device five ways (the C4 rules alone; plus the nine C4 phrases; plus dup_scope 2; plus the cut; plus the
compact form; and min_words with dup_scope 2 and the cut, which keeps most lines), beside quality_rows_tensor without and with duplicate lines and encode_rows_tensor of the same documents;
in one process, the calls alternated; medians of host wall time around calls that end in a device synchronise.  The
stages come from one more call per form under WP_OPT_STAGE_TIMING.  The arrays of the first 200 documents are held
against tests/lines_model.py before anything is timed.  One JSON line, appended to --out (default
profiles/lines_probe.jsonl).

    python profiles/lines_probe.py [--mb 100] [--reps 7] [--lines 20] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library: torch's HIP runtime serves the process)

import lines_model as M  # noqa: E402
import wordpiece_amd as W  # noqa: E402
from wordpiece_amd import lines as L  # noqa: E402
from wordpiece_amd import synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=float, default=100.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--lines", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lines_probe.jsonl"))
    args = ap.parse_args()
    text, vocab = synth.parallel_corpus("english", int(args.mb * 1e6), 2, 29000, 0)
    text, line_off = W.line_rows(text)
    off = np.ascontiguousarray(np.concatenate((line_off[:-1:args.lines], line_off[-1:])))
    n, n_rows = int(text.size), int(off.size - 1)
    c4 = L.lines_rules("c4")
    rules, phrases = c4["rules"], dict(phrases=c4["phrases"], doc_phrases=c4["doc_phrases"])
    q_rules = W.quality_rules("gopher")
    stop = [w.encode() for w in q_rules.pop("stop_words")]
    q_no_dup = {k: v for k, v in q_rules.items() if not k.startswith("max_dup")}
    t = torch.zeros((n + 19) // 16 * 16, dtype=torch.uint8, device="cuda:0")
    t[:n] = torch.from_numpy(text).to("cuda:0")
    d_off = torch.from_numpy(off).to("cuda:0")
    torch.cuda.synchronize()
    gv = W.Vocab(vocab, device=0)
    # the first documents, once, against the model (their own batch: dup_scope 2 looks across the whole of it)
    head = min(200, n_rows)
    h_off = torch.from_numpy(np.ascontiguousarray(off[:head + 1])).to("cuda:0")
    got = L.filter_lines_tensor(gv, t[:int(off[head])], h_off, rules=rules, dup_scope=2, lines=True, cut=True, compact=True, **phrases)
    exp = M.filter_lines(text[:off[head]].tobytes(), off[:head + 1].tolist(), rules=rules, dup_scope=2, **phrases)
    for key in ("signals", "reasons", "line_row", "line_start", "line_len", "line_reasons", "cut_off", "kept", "row_off"):
        assert got[key].cpu().numpy().tolist() == exp[key], "%s differs from the model's" % key
    assert got["cut_data"].cpu().numpy().tobytes() == exp["cut_data"] and got["data"].cpu().numpy().tobytes() == exp["data"], "the cut differs from the model's"
    f = lambda **kw: (lambda: L.filter_lines_tensor(gv, t[:n], d_off, rules=rules, copy=False, **kw))  # noqa: E731
    calls = {
        "lines_rules": f(),
        "lines_phrases": f(**phrases),
        "lines_phrases_dup": f(dup_scope=2, **phrases),
        "lines_phrases_dup_cut": f(dup_scope=2, cut=True, **phrases),
        "lines_phrases_dup_compact": f(dup_scope=2, compact=True, **phrases),
        # (the synthetic text ends no line in punctuation, so the C4 rules drop every line: this form keeps most and moves bytes)
        "lines_min_words_dup_cut": lambda: L.filter_lines_tensor(gv, t[:n], d_off, rules={"min_words": 3}, dup_scope=2, cut=True, copy=False),
        "quality": lambda: gv.quality_rows_tensor(t[:n], d_off, rules=q_no_dup, stop_words=stop, copy=False),
        "quality_dup_lines": lambda: gv.quality_rows_tensor(t[:n], d_off, rules=q_rules, stop_words=stop, copy=False),
        "encode_rows": lambda: gv.encode_rows_tensor(t[:n], d_off, copy=False),
    }
    times, stats = {k: [] for k in calls}, {}
    for k, call in calls.items():  # warm-up (code objects, the buffers), and what each form drops
        call()
        call()
        if k.startswith("lines"):
            stats[k] = L.lines_stats(gv)
    for _ in range(args.reps):
        for k, call in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            times[k].append((time.perf_counter() - t0) * 1e3)
    med = {k: statistics.median(v) for k, v in times.items()}
    stages = {}
    gv.set_option(W.WP_OPT_STAGE_TIMING, 1)
    for name in calls:
        if name != "encode_rows":
            calls[name]()
            s = gv.stats()
            stages[name] = {k: round(s[k], 3) for k in ("ms_decode", "ms_sa", "ms_scan", "ms_walk", "ms_total")}
    gv.set_option(W.WP_OPT_STAGE_TIMING, 0)
    out = {"config": 2, "mb": args.mb, "n_bytes": n, "n_rows": n_rows, "lines_per_doc": args.lines, "reps": args.reps, "lines_stats": stats,
           "ms_median": {k: round(v, 3) for k, v in med.items()}, "ms_min": {k: round(min(v), 3) for k, v in times.items()},
           "ms_max": {k: round(max(v), 3) for k, v in times.items()}, "stages": stages, "per_kernel_split": "not measured",
           "lines_phrases_over_quality": round(med["lines_phrases"] / med["quality"], 3),
           "phrase_scan_ms": round(med["lines_phrases"] - med["lines_rules"], 3)}
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
