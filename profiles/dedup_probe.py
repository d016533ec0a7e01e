"""Cost of the dedup call on the config-2 text (100 MB of English) resident in HBM, its rows the lines of the text:
wp_dedup_rows_device over the text bytes, and over the ids of encode_rows_tensor with and without the compact form; in one
process, the calls alternated; medians of host wall time around calls that end in a device synchronise.  Its stages come
from one more call per form under WP_OPT_STAGE_TIMING (HIP events inside the library, handed out through wp_stats as the
header's section "duplicate rows" says).  Yardsticks beside them:

  count_words      the handle's word count of the same text
  encode_tensor    the handle's plain encode of the same text
  host_dict        a dict over the lines of the text on the host (split and dict timed apart)

The kept lines of the device are compared with the host's before anything is timed.  One JSON line, appended to --out
(default profiles/dedup_probe.jsonl).

    python profiles/dedup_probe.py [--mb 100] [--reps 7] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (before the library: torch's HIP runtime serves the process)

import wordpiece_amd as W  # noqa: E402
from wordpiece_amd import synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=float, default=100.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dedup_probe.jsonl"))
    args = ap.parse_args()
    text, vocab = synth.parallel_corpus("english", int(args.mb * 1e6), 2, 29000, 0)
    text, off = W.line_rows(text)
    n, n_rows = int(text.size), int(off.size - 1)
    raw = text.tobytes()
    t0 = time.perf_counter()
    lines = raw.split(b"\n")[:-1]
    ms_split = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    seen = {}
    for i, line in enumerate(lines):
        seen.setdefault(line, i)
    ms_dict = (time.perf_counter() - t0) * 1e3
    assert len(lines) == n_rows
    t = torch.zeros((n + 19) // 16 * 16, dtype=torch.uint8, device="cuda:0")
    t[:n] = torch.from_numpy(text).to("cuda:0")
    d_off = torch.from_numpy(off).to("cuda:0")
    torch.cuda.synchronize()
    gv = W.Vocab(vocab, device=0)
    # the kept lines, once, against the host's
    got = gv.dedup_rows_tensor(t[:n], d_off, copy=False)
    assert got["kept"].tolist() == list(seen.values()), "the kept lines differ from the host's"
    text_stats = gv.dedup_stats()
    ids, splits = gv.encode_rows_tensor(t[:n], d_off)
    gv.dedup_rows_tensor(ids, splits, copy=False)
    ids_stats = gv.dedup_stats()
    calls = {
        "dedup_text": lambda: gv.dedup_rows_tensor(t[:n], d_off, copy=False),
        "dedup_text_compact": lambda: gv.dedup_rows_tensor(t[:n], d_off, compact=True, copy=False),
        "dedup_ids": lambda: gv.dedup_rows_tensor(ids, splits, copy=False),
        "dedup_ids_compact": lambda: gv.dedup_rows_tensor(ids, splits, inverse=True, compact=True, copy=False),
        "count_words": lambda: gv.count_words_tensor(t[:n], order="first", copy=False),
        "encode_tensor": lambda: gv.encode_tensor(t[:n], copy=False),
    }
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
    for name in ("dedup_text_compact", "dedup_ids_compact"):
        calls[name]()
        s = gv.stats()
        stages[name] = {"ms_list": round(s["ms_decode"], 3), "ms_rounds": round(s["ms_sa"], 3), "ms_table": round(s["ms_walk"], 3),
                        "ms_total": round(s["ms_total"], 3), "ms_radix_scatter": round(s["ms_radix_scatter"], 3),
                        "radix_passes": s["radix_passes"], "radix_pass_bytes": s["radix_pass_bytes"]}
    gv.set_option(W.WP_OPT_STAGE_TIMING, 0)
    out = {"config": 2, "mb": args.mb, "n_bytes": n, "n_rows": n_rows, "n_ids": int(ids.numel()), "reps": args.reps,
           "dedup_stats_text": text_stats, "dedup_stats_ids": ids_stats,
           "ms_median": {k: round(v, 3) for k, v in med.items()},
           "ms_min": {k: round(min(v), 3) for k, v in times.items()},
           "ms_max": {k: round(max(v), 3) for k, v in times.items()},
           "stages": stages,
           "host_ms": {"split": round(ms_split, 1), "dict": round(ms_dict, 1)},
           "dedup_text_over_encode": round(med["dedup_text"] / med["encode_tensor"], 3),
           "dedup_text_over_count": round(med["dedup_text"] / med["count_words"], 3),
           "host_over_dedup_text": round((ms_split + ms_dict) / med["dedup_text"], 1)}
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
