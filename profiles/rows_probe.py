"""Cost of the documents calls on the config-2 text (100 MB of English, the rows are its lines), device entry points,
in one process, the calls alternated; medians of host wall time around calls that end in a device synchronise:

  ids           wp_linear_encode_device
  offsets_byte  wp_linear_encode_offsets_device, bytes                    (the yardstick of the rows calls)
  rows_none     wp_linear_encode_rows_device, lines mode, unit -1
  rows_byte     the same with byte offsets
  padded_128    wp_linear_encode_padded_device, lines mode, max_len 128 with [CLS] / [SEP], into caller-owned tensors
  batch         wp_linear_encode_batch over the first 10,000 lines, scaled to one line: today's per-document price

One JSON line, appended to --out (default profiles/rows_probe.jsonl).  The device time of the new kernels comes from a
run of its own:  rocprofv3 --kernel-trace --stats -d <dir> -- python profiles/rows_probe.py --reps 3 --no-batch

    python profiles/rows_probe.py [--mb 100] [--reps 9] [--no-batch] [--out FILE]
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
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--no-batch", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rows_probe.jsonl"))
    args = ap.parse_args()
    text, vocab = synth.parallel_corpus("english", int(args.mb * 1e6), 2, 29000, 0)
    n = len(text)
    t = torch.zeros((n + 19) // 16 * 16, dtype=torch.uint8, device="cuda:0")
    t[:n] = torch.frombuffer(bytearray(text), dtype=torch.uint8).to("cuda:0")
    torch.cuda.synchronize()
    gv = W.Vocab(vocab, device=0)
    n_rows = gv.encode_rows_tensor(t[:n], copy=False)[1].numel() - 1
    own = (torch.empty((n_rows, 128), dtype=torch.int32, device="cuda:0"), torch.empty(n_rows, dtype=torch.int32, device="cuda:0"))
    calls = {
        "ids": lambda: gv.encode_device(t.data_ptr(), n),
        "offsets_byte": lambda: gv.encode_device_with_offsets(t.data_ptr(), n, "byte"),
        "rows_none": lambda: gv.encode_rows_tensor(t[:n], copy=False),
        "rows_byte": lambda: gv.encode_rows_tensor(t[:n], offsets="byte", copy=False),
        "padded_128": lambda: gv.encode_padded_tensor(t[:n], max_len=128, cls_id=101, sep_id=102, out=own),
    }
    times, stats = {k: [] for k in calls}, {}
    for f in calls.values():  # warm-up (arena growth, code objects)
        f()
        f()
    for _ in range(args.reps):
        for k, f in calls.items():
            t0 = time.perf_counter()
            f()
            times[k].append((time.perf_counter() - t0) * 1e3)
            stats[k] = gv.stats()
    med = {k: statistics.median(v) for k, v in times.items()}
    out = {"config": 2, "mb": args.mb, "n_bytes": n, "n_rows": n_rows, "n_ids": stats["ids"]["n_ids"], "reps": args.reps,
           "rows_route": stats["rows_byte"]["rows_route"], "rows_truncated_128": stats["padded_128"]["rows_truncated"],
           "ms_median": {k: round(v, 3) for k, v in med.items()},
           "ms_min": {k: round(min(v), 3) for k, v in times.items()},
           "ms_max": {k: round(max(v), 3) for k, v in times.items()},
           "rows_byte_minus_offsets_byte_ms": round(med["rows_byte"] - med["offsets_byte"], 3),
           "rows_byte_over_offsets_byte": round(med["rows_byte"] / med["offsets_byte"], 3)}
    if not args.no_batch:
        lines = text.split(b"\n")[:10000]
        gv.encode_batch(lines[:200])
        t0 = time.perf_counter()
        gv.encode_batch(lines)
        ms = (time.perf_counter() - t0) * 1e3
        out["batch_lines"] = len(lines)
        out["batch_ms_per_line"] = round(ms / len(lines), 4)
        out["batch_ms_scaled_to_all_rows"] = round(ms / len(lines) * n_rows, 1)
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
