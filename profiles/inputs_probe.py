"""Cost of the model-inputs call on the config-2 text (100 MB of English, the rows are its lines), device entry points
with caller-owned buffers, in one process, the calls alternated; medians of host wall time around calls that end in a
device synchronise:

  padded_128    wp_linear_encode_padded_device, max_len 128 with [CLS] / [SEP]        (the yardstick: unchanged code)
  inputs_single wp_linear_encode_inputs_device, pairs 0, stride -1, longest_first: the same rows plus token_type_ids, sample
  inputs_pairs  pairs 1, longest_first (neighbouring lines are A and B; an odd last line is left out of the text)
  inputs_windows pairs 0, only_first, stride 32: the windows path (plan, scan, one more scalar fetch, pack)

One JSON line, appended to --out (default profiles/inputs_probe.jsonl).  The device time of plan / scan / pack comes
from a run of its own:  rocprofv3 --kernel-trace --stats -d <dir> -- python profiles/inputs_probe.py --reps 3

    python profiles/inputs_probe.py [--mb 100] [--reps 9] [--max-len 128] [--out FILE]
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
    ap.add_argument("--max-len", type=int, default=128)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inputs_probe.jsonl"))
    args = ap.parse_args()
    L = args.max_len
    text, vocab = synth.parallel_corpus("english", int(args.mb * 1e6), 2, 29000, 0)
    if text.count(b"\n") % 2:  # (pairs need an even number of lines: the last one goes)
        text = text[:text.rstrip(b"\n").rfind(b"\n") + 1]
    n = len(text)
    t = torch.zeros((n + 19) // 16 * 16, dtype=torch.uint8, device="cuda:0")
    t[:n] = torch.frombuffer(bytearray(text), dtype=torch.uint8).to("cuda:0")
    torch.cuda.synchronize()
    gv = W.Vocab(vocab, device=0)
    n_rows = gv.encode_rows_tensor(t[:n], copy=False)[1].numel() - 1
    kw = dict(max_len=L, cls_id=101, sep_id=102)
    n_win = gv.encode_inputs_tensor(t[:n], truncation="only_first", stride=32, **kw)["lengths"].numel()
    cap = max(n_rows, n_win)
    own = {"input_ids": torch.empty((cap, L), dtype=torch.int32, device="cuda:0"),
           "token_type_ids": torch.empty((cap, L), dtype=torch.int32, device="cuda:0"),
           "lengths": torch.empty(cap, dtype=torch.int32, device="cuda:0"), "sample": torch.empty(cap, dtype=torch.int32, device="cuda:0")}
    calls = {
        "padded_128": lambda: gv.encode_padded_tensor(t[:n], out=(own["input_ids"], own["lengths"]), **kw),
        "inputs_single": lambda: gv.encode_inputs_tensor(t[:n], out=own, **kw),
        "inputs_pairs": lambda: gv.encode_inputs_tensor(t[:n], pairs=True, out=own, **kw),
        "inputs_windows": lambda: gv.encode_inputs_tensor(t[:n], truncation="only_first", stride=32, out=own, **kw),
    }
    times, stats, istats = {k: [] for k in calls}, {}, {}
    for f in calls.values():  # warm-up (arena growth, code objects)
        f()
        f()
    for _ in range(args.reps):
        for k, f in calls.items():
            t0 = time.perf_counter()
            f()
            times[k].append((time.perf_counter() - t0) * 1e3)
            stats[k], istats[k] = gv.stats(), gv.inputs_stats()
    med = {k: statistics.median(v) for k, v in times.items()}
    cell = 4 * L
    out = {"config": 2, "mb": args.mb, "n_bytes": n, "n_rows": n_rows, "n_ids": stats["padded_128"]["n_ids"], "reps": args.reps,
           "max_len": L, "rows_truncated_128": stats["padded_128"]["rows_truncated"],
           "inputs": {k: istats[k] for k in calls if k != "padded_128"},
           "bytes_written": {"padded_128": n_rows * (cell + 4), "inputs_single": n_rows * (2 * cell + 8),
                             "inputs_pairs": n_rows // 2 * (2 * cell + 8), "inputs_windows": n_win * (2 * cell + 8)},
           "ms_median": {k: round(v, 3) for k, v in med.items()},
           "ms_min": {k: round(min(v), 3) for k, v in times.items()},
           "ms_max": {k: round(max(v), 3) for k, v in times.items()},
           "inputs_single_minus_padded_ms": round(med["inputs_single"] - med["padded_128"], 3),
           "inputs_single_over_padded": round(med["inputs_single"] / med["padded_128"], 3)}
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
