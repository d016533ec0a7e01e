"""Cost of the scrub on the config-2 text (100 MB of English) resident in HBM, 20 lines of the text to a document, with an
address planted on --share of the lines (an e-mail and an IPv4 address by turns): wp_scrub_rows_device four ways (the
signals alone; with the match table; with the text; with the compact form), beside filter_lines_tensor with the C4 phrases,
quality_rows_tensor and a device copy of the same bytes; in one process, the calls alternated, each between two device
events after two warm-up calls; medians with the spread.  The stages come from one more call per form under
WP_OPT_STAGE_TIMING.  The host baseline is Python re with the two patterns of tests/test_scrub_model.py over a sample of
the same text, scaled by bytes and marked as such.  The arrays of the first 200 documents are held against
tests/scrub_model.py before anything is timed.  One JSON line, appended to --out (default profiles/scrub_probe.jsonl).

    python profiles/scrub_probe.py [--mb 100] [--reps 7] [--lines 20] [--share 0.02] [--out FILE]
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

import scrub_model as M  # noqa: E402
import test_scrub_model as R  # noqa: E402  (the regular expressions of the host baseline)
import wordpiece_amd as W  # noqa: E402
from wordpiece_amd import lines as L  # noqa: E402
from wordpiece_amd import scrub as S  # noqa: E402
from wordpiece_amd import synth  # noqa: E402

PLANTS = (b" write to Jane.Doe+list@mail.example.org today ", b" the host 93.184.216.34 answered ")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=float, default=100.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--lines", type=int, default=20)
    ap.add_argument("--share", type=float, default=0.02)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scrub_probe.jsonl"))
    args = ap.parse_args()
    text, vocab = synth.parallel_corpus("english", int(args.mb * 1e6), 2, 29000, 0)
    text, line_off = W.line_rows(text)
    text = text.copy()
    rng = np.random.default_rng(28)
    starts, lens = line_off[:-1], np.diff(line_off)
    planted = 0
    for k, plant in enumerate(PLANTS):  # over the first bytes of the chosen lines that have room for it
        sel = starts[(rng.random(starts.size) < args.share / len(PLANTS)) & (lens > len(plant) + 1)]
        text[sel[:, None] + np.arange(len(plant))] = np.frombuffer(plant, dtype=np.uint8)
        planted += int(sel.size)
    off = np.ascontiguousarray(np.concatenate((line_off[:-1:args.lines], line_off[-1:])))
    n, n_rows = int(text.size), int(off.size - 1)
    c4 = L.lines_rules("c4")
    q_rules = W.quality_rules("gopher")
    stop = [w.encode() for w in q_rules.pop("stop_words")]
    q_rules = {k: v for k, v in q_rules.items() if not k.startswith("max_dup")}
    t = torch.zeros((n + 19) // 16 * 16, dtype=torch.uint8, device="cuda:0")
    t[:n] = torch.from_numpy(text).to("cuda:0")
    t2 = torch.empty_like(t)
    d_off = torch.from_numpy(off).to("cuda:0")
    torch.cuda.synchronize()
    gv = W.Vocab(vocab, device=0)
    head = min(200, n_rows)
    h_off = torch.from_numpy(np.ascontiguousarray(off[:head + 1])).to("cuda:0")
    got = S.scrub_rows_tensor(gv, t[:int(off[head])], h_off, matches=True, text=True, compact=True)
    default = S.scrub_replacements("default")
    exp = M.scrub_rows(text[:off[head]].tobytes(), off[:head + 1].tolist(), 3, [x.encode() for x in default["email"]], [x.encode() for x in default["ip"]])
    for key in ("signals", "reasons", "match_row", "match_start", "match_len", "match_kind", "match_repl", "out_off", "kept", "row_off"):
        assert got[key].cpu().numpy().tolist() == exp[key], "%s differs from the model's" % key
    assert got["out_data"].cpu().numpy().tobytes() == exp["out_data"] and got["data"].cpu().numpy().tobytes() == exp["data"], "the text differs from the model's"
    f = lambda **kw: (lambda: S.scrub_rows_tensor(gv, t[:n], d_off, copy=False, **kw))  # noqa: E731
    calls = {
        "scrub_signals": f(),
        "scrub_matches": f(matches=True),
        "scrub_text": f(text=True),
        "scrub_compact": f(compact=True),
        "lines_phrases": lambda: L.filter_lines_tensor(gv, t[:n], d_off, rules=c4["rules"], phrases=c4["phrases"], doc_phrases=c4["doc_phrases"], copy=False),
        "quality": lambda: gv.quality_rows_tensor(t[:n], d_off, rules=q_rules, stop_words=stop, copy=False),
        "device_copy": lambda: t2.copy_(t),
    }
    times, stats = {k: [] for k in calls}, {}
    for k, call in calls.items():  # warm-up (code objects, the buffers), and what the scrub finds
        call()
        call()
        if k.startswith("scrub"):
            stats[k] = S.scrub_stats(gv)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for _ in range(args.reps):
        for k, call in calls.items():
            torch.cuda.synchronize()
            ev[0].record()
            call()
            ev[1].record()
            torch.cuda.synchronize()
            times[k].append(ev[0].elapsed_time(ev[1]))
    med = {k: statistics.median(v) for k, v in times.items()}
    stages = {}
    gv.set_option(W.WP_OPT_STAGE_TIMING, 1)
    for name in calls:
        if name != "device_copy":
            calls[name]()
            s = gv.stats()
            stages[name] = {k: round(s[k], 3) for k in ("ms_decode", "ms_sa", "ms_scan", "ms_walk", "ms_total")}
    gv.set_option(W.WP_OPT_STAGE_TIMING, 0)
    # the host baseline: both patterns over the documents of a sample, in one thread, scaled to the whole text by bytes
    docs = [text[off[r]:off[r + 1]].tobytes() for r in range(min(n_rows, 2000))]
    t0 = time.perf_counter()
    hits = sum(len(R.EMAIL_RE.findall(d)) + len(R.IPV4_RE.findall(d)) for d in docs)
    sample_ms = (time.perf_counter() - t0) * 1e3
    sample_bytes = sum(map(len, docs))
    out = {"config": 2, "mb": args.mb, "n_bytes": n, "n_rows": n_rows, "lines_per_doc": args.lines, "share": args.share, "planted": planted, "reps": args.reps,
           "scrub_stats": stats, "ms_median": {k: round(v, 3) for k, v in med.items()}, "ms_min": {k: round(min(v), 3) for k, v in times.items()},
           "ms_max": {k: round(max(v), 3) for k, v in times.items()}, "stages": stages,
           "per_kernel_split": "profiles/scrub_kernel_stats.csv, from a rocprofv3 --kernel-trace --stats run of this probe, of its own",
           "scrub_signals_over_lines_phrases": round(med["scrub_signals"] / med["lines_phrases"], 3),
           "host_re": {"sample_bytes": sample_bytes, "sample_ms": round(sample_ms, 1), "sample_hits": hits, "ms_scaled_by_bytes": round(sample_ms * n / sample_bytes, 1)}}
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
