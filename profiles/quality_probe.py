"""Cost of the quality call on the config-2 text (100 MB of English) resident in HBM, 20 lines of the text to a
document: wp_quality_rows_device with the Gopher rules without and with the duplicate-line stage, and with the compact
form; in one process, the calls alternated; medians of host wall time around calls that end in a device synchronise.  Its
stages come from one more call per form under WP_OPT_STAGE_TIMING (HIP events inside the library, handed out through
wp_stats as the header's section "quality signals" says).  Yardsticks beside them:

  encode_rows      the handle's encode of the same documents
  dedup_rows       the handle's exact dedup of the same documents
  host_model       tests/quality_model.py over the first --sample documents, SCALED by bytes to the whole text
  short_rows       the first --short-mb of the text as rows of 8 bytes, beside the same bytes as documents

The signals and reasons of the first 200 documents are held against the model before anything is timed.  One JSON line,
appended to --out (default profiles/quality_probe.jsonl).

    python profiles/quality_probe.py [--mb 100] [--reps 7] [--lines 20] [--sample 400] [--short-mb 8] [--out FILE]
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

import quality_model as M  # noqa: E402
import wordpiece_amd as W  # noqa: E402
from wordpiece_amd import synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=float, default=100.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--lines", type=int, default=20)
    ap.add_argument("--sample", type=int, default=400)
    ap.add_argument("--short-mb", type=float, default=8.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quality_probe.jsonl"))
    args = ap.parse_args()
    text, vocab = synth.parallel_corpus("english", int(args.mb * 1e6), 2, 29000, 0)
    text, line_off = W.line_rows(text)
    off = np.ascontiguousarray(np.concatenate((line_off[:-1:args.lines], line_off[-1:])))
    n, n_rows = int(text.size), int(off.size - 1)
    rules = W.quality_rules("gopher")
    stop = [w.encode() for w in rules.pop("stop_words")]
    no_dup = {k: v for k, v in rules.items() if not k.startswith("max_dup")}
    t = torch.zeros((n + 19) // 16 * 16, dtype=torch.uint8, device="cuda:0")
    t[:n] = torch.from_numpy(text).to("cuda:0")
    d_off = torch.from_numpy(off).to("cuda:0")
    torch.cuda.synchronize()
    gv = W.Vocab(vocab, device=0)
    # the first documents, once, against the model; the model's time on a sample, scaled by bytes
    head = min(200, n_rows)
    got = gv.quality_rows_tensor(t[:n], d_off, rules=rules, stop_words=stop, copy=False)
    exp = M.quality(text[:off[head]].tobytes(), off[:head + 1].tolist(), limit=M.limits(**rules), stop_words=stop)
    assert got["signals"][:, :head].cpu().numpy().tolist() == exp["signals"], "the signals differ from the model's"
    assert got["reasons"][:head].cpu().numpy().view(np.uint32).tolist() == exp["reasons"], "the reasons differ from the model's"
    q_stats = gv.quality_stats()
    sample = min(args.sample, n_rows)
    t0 = time.perf_counter()
    M.quality(text[:off[sample]].tobytes(), off[:sample + 1].tolist(), limit=M.limits(**rules), stop_words=stop)
    ms_model_sample = (time.perf_counter() - t0) * 1e3
    calls = {
        "quality": lambda: gv.quality_rows_tensor(t[:n], d_off, rules=no_dup, stop_words=stop, copy=False),
        "quality_dup_lines": lambda: gv.quality_rows_tensor(t[:n], d_off, rules=rules, stop_words=stop, copy=False),
        "quality_dup_lines_compact": lambda: gv.quality_rows_tensor(t[:n], d_off, rules=rules, stop_words=stop, compact=True, copy=False),
        "encode_rows": lambda: gv.encode_rows_tensor(t[:n], d_off, copy=False),
        "dedup_rows": lambda: gv.dedup_rows_tensor(t[:n], d_off, copy=False),
    }
    # the same bytes cut into rows far below a tile: the first --short-mb of the text as rows of 8 bytes, beside those bytes
    # as documents (flat over bytes, not rows, is the claim this pair measures)
    m = min(n, int(args.short_mb * 1e6)) // 8 * 8
    d_off8 = torch.arange(0, m + 1, 8, dtype=torch.int64, device="cuda:0")
    k_docs = int(np.searchsorted(off, m, side="right")) - 1
    d_off_docs = torch.from_numpy(np.ascontiguousarray(off[:k_docs + 1])).to("cuda:0")
    m_docs = int(off[k_docs])
    calls["short_rows_of_8_bytes"] = lambda: gv.quality_rows_tensor(t[:m], d_off8, rules=no_dup, stop_words=stop, copy=False)
    calls["short_same_bytes_as_docs"] = lambda: gv.quality_rows_tensor(t[:m_docs], d_off_docs, rules=no_dup, stop_words=stop, copy=False)
    times = {k: [] for k in calls}
    for f in calls.values():  # warm-up (code objects, the buffers)
        f()
        f()
    for _ in range(args.reps):
        for k, f in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            times[k].append((time.perf_counter() - t0) * 1e3)
    med = {k: statistics.median(v) for k, v in times.items()}
    # the stages, by HIP events inside the library
    stages = {}
    gv.set_option(W.WP_OPT_STAGE_TIMING, 1)
    for name in ("quality", "quality_dup_lines_compact"):
        calls[name]()
        s = gv.stats()
        stages[name] = {"ms_offsets": round(s["ms_decode"], 3), "ms_signals": round(s["ms_sa"], 3), "ms_dup_lines": round(s["ms_scan"], 3),
                        "ms_rules_compact": round(s["ms_walk"], 3), "ms_total": round(s["ms_total"], 3)}
    gv.set_option(W.WP_OPT_STAGE_TIMING, 0)
    scaled = ms_model_sample * n / max(1, int(off[sample]))
    out = {"config": 2, "mb": args.mb, "n_bytes": n, "n_rows": n_rows, "lines_per_doc": args.lines, "reps": args.reps, "quality_stats": q_stats,
           "ms_median": {k: round(v, 3) for k, v in med.items()},
           "ms_min": {k: round(min(v), 3) for k, v in times.items()},
           "ms_max": {k: round(max(v), 3) for k, v in times.items()},
           "stages": stages, "per_kernel_split": "not measured",
           "short_rows": {"n_rows": m // 8, "n_bytes": m, "docs_n_rows": k_docs, "docs_n_bytes": m_docs,
                          "rows_of_8_over_docs": round(med["short_rows_of_8_bytes"] / med["short_same_bytes_as_docs"], 2)},
           "host_model": {"sample_rows": sample, "sample_bytes": int(off[sample]), "ms_sample": round(ms_model_sample, 1),
                          "ms_scaled_by_bytes": round(scaled, 1), "scaled": True},
           "gb_per_s": {k: round(n / med[k] / 1e6, 2) for k in ("quality", "quality_dup_lines", "quality_dup_lines_compact")},
           "quality_over_encode": round(med["quality"] / med["encode_rows"], 3),
           "quality_dup_over_dedup": round(med["quality_dup_lines"] / med["dedup_rows"], 3),
           "host_model_scaled_over_quality_dup": round(scaled / med["quality_dup_lines"], 1)}
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
