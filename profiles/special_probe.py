"""Cost of the special-tokens documents call on the config-2 text (100 MB of English, the rows are its lines), device
entry points, byte offsets, against wp_linear_encode_rows_device with byte offsets on the same text in the same process;
the calls alternated; medians of host wall time around calls that end in a device synchronise.  Three texts:

  none     the text as it is: no literal (the extra cost is the match pass)
  sep      " [SEP]" in front of every line end: one literal per line
  mask20   "[MASK] " put in behind every 20th blank: one word in twenty a literal

  special_<text>  wp_linear_encode_special_rows_device, "[SEP]" and "[MASK]" listed
  rows_<text>     wp_linear_encode_rows_device on the same bytes (what the literals cost the plain call: more punctuation)

One JSON line, appended to --out (default profiles/special_probe.jsonl).  --trace: every call three times and nothing
written, for a `rocprofv3 --kernel-trace --stats` run of its own.

    python profiles/special_probe.py [--mb 100] [--reps 9] [--out FILE] [--trace]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (before the library: torch's HIP runtime serves the process)

import wordpiece_amd as W  # noqa: E402
from wordpiece_amd import synth  # noqa: E402


def insert_behind(a, where, piece):
    """the bytes of `a` with `piece` put in behind every position of `where` (ascending)"""
    piece = np.frombuffer(piece, dtype=np.uint8)
    mark = np.zeros(len(a) + 1, dtype=np.int64)
    mark[where + 1] = len(piece)
    dest = np.arange(len(a), dtype=np.int64) + np.cumsum(mark)[:-1]
    out = np.empty(len(a) + len(piece) * len(where), dtype=np.uint8)
    out[dest] = a
    gaps = dest[where] + 1
    for k in range(len(piece)):
        out[gaps + k] = piece[k]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=float, default=100.0)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "special_probe.jsonl"))
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    text, vocab = synth.parallel_corpus("english", int(args.mb * 1e6), 2, 29000, 0)
    a = np.frombuffer(text, dtype=np.uint8)
    blanks = np.flatnonzero(a == 0x20)
    texts = {"none": a,
             "sep": np.frombuffer(bytes(text).replace(b"\n", b" [SEP]\n"), dtype=np.uint8),
             "mask20": insert_behind(a, blanks[19::20], b"[MASK] ")}
    dev = torch.device("cuda:0")
    gv = W.Vocab(vocab, device=0)
    listed = gv.special_ids(["[SEP]", "[MASK]"])
    calls, info, keep = {}, {}, []
    for name, arr in texts.items():
        n = len(arr)
        t = torch.zeros((n + 19) // 16 * 16, dtype=torch.uint8, device=dev)
        t[:n] = torch.from_numpy(arr.copy()).to(dev)
        keep.append(t)
        calls["special_" + name] = lambda t=t, n=n: gv.encode_special_rows_tensor(t[:n], None, special_ids=listed, offsets="byte", copy=False)
        calls["rows_" + name] = lambda t=t, n=n: gv.encode_rows_tensor(t[:n], offsets="byte", copy=False)
    torch.cuda.synchronize()
    for k, f in calls.items():  # warm-up (buffer growth, code objects), and what each call returns
        f()
        ids, splits, offs = f()
        info[k] = {"n_ids": ids.numel(), "n_rows": splits.numel() - 1}
        if k.startswith("special_"):
            info[k].update(gv.special_stats())
            info[k]["n_bytes"] = len(texts[k[len("special_"):]])
    if args.trace:
        for _ in range(3):
            for f in calls.values():
                f()
        return
    times = {k: [] for k in calls}
    for _ in range(args.reps):
        for k, f in calls.items():
            t0 = time.perf_counter()
            f()
            times[k].append((time.perf_counter() - t0) * 1e3)
    med = {k: statistics.median(v) for k, v in times.items()}
    out = {"config": 2, "mb": args.mb, "reps": args.reps, "listed": listed, "calls": info,
           "ms_median": {k: round(v, 3) for k, v in med.items()},
           "ms_min": {k: round(min(v), 3) for k, v in times.items()},
           "ms_max": {k: round(max(v), 3) for k, v in times.items()},
           "extra_ms": {k: round(med["special_" + k] - med["rows_" + k], 3) for k in texts},
           "special_over_rows": {k: round(med["special_" + k] / med["rows_" + k], 3) for k in texts}}
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
