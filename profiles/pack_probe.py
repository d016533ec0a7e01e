"""Cost of the pack call on the config-2 text (100 MB of English, the rows are its lines): the text goes through
encode_rows_tensor once (the ids and row_splits are cloned: every pack call reads the same tensors), then
wp_pack_sequences_device runs on them into caller-owned buffers; [CLS] / [SEP] around every document; in one process,
the calls alternated; medians of host wall time around calls that end in a device synchronise:

  next_fit_L_wW  WP_PACK_NEXT_FIT + WP_PACK_LONG_TRUNCATE at max_len L, want W (0: input_ids and lengths; 7: all five)
  stream_L_wW    WP_PACK_STREAM
  copy_<call>    the yardstick of that call: one device-to-device memcpy of the bytes the call must move — 4 B per id
                 read plus 4 B per cell and output written (and the lengths): half of them read, half written (torch's
                 copy_ between contiguous uint8 tensors, a hipMemcpyDtoD, and one synchronise)

One JSON line, appended to --out (default profiles/pack_probe.jsonl).  --trace: every call three times and nothing
written, for a `rocprofv3 --kernel-trace --stats` run of its own.

    python profiles/pack_probe.py [--mb 100] [--reps 9] [--out FILE] [--trace] [--only CALL]
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

CLS, SEP = 101, 102


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=float, default=100.0)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pack_probe.jsonl"))
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--only", default=None, help="one call by name (with its copy), e.g. next_fit_128_w7")
    args = ap.parse_args()
    text, vocab = synth.parallel_corpus("english", int(args.mb * 1e6), 2, 29000, 0)
    n = len(text)
    dev = torch.device("cuda:0")
    t = torch.zeros((n + 19) // 16 * 16, dtype=torch.uint8, device=dev)
    t[:n] = torch.frombuffer(bytearray(text), dtype=torch.uint8).to(dev)
    torch.cuda.synchronize()
    gv = W.Vocab(vocab, device=0)
    ids, splits = gv.encode_rows_tensor(t[:n])  # (copies)
    n_ids, n_docs = ids.numel(), splits.numel() - 1
    configs = [(mode, L, want) for L in (128, 512) for mode in ("next_fit", "stream") for want in (0, 7)
               if args.only in (None, "%s_%d_w%d" % (mode, L, want))]
    calls, moved, stats, keep = {}, {}, {}, []
    for mode, L, want in configs:
        name = "%s_%d_w%d" % (mode, L, want)
        names = [k for k, bit in W._PACK_WANT.items() if want & bit]
        first = gv.pack_sequences_tensor(ids, splits, max_len=L, mode=mode, bos_id=CLS, eos_id=SEP, want=names)
        stats[name] = gv.pack_stats()
        rows = first["lengths"].numel()
        kw = dict(max_len=L, mode=mode, bos_id=CLS, eos_id=SEP, want=names, out=first)
        calls[name] = lambda kw=kw: gv.pack_sequences_tensor(ids, splits, **kw)  # (ends in the library's synchronise)
        moved[name] = 4 * n_ids + 4 * rows * L * (1 + len(names)) + 4 * rows
        half = moved[name] // 2
        a, b = torch.empty(half, dtype=torch.uint8, device=dev), torch.empty(half, dtype=torch.uint8, device=dev)
        keep.append((first, a, b))

        def copy(a=a, b=b):
            b.copy_(a)
            torch.cuda.synchronize()
        calls["copy_" + name] = copy
        moved["copy_" + name] = 2 * half
    torch.cuda.synchronize()
    for f in calls.values():  # warm-up (buffer growth, code objects)
        f()
        f()
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
    out = {"config": 2, "mb": args.mb, "n_bytes": n, "n_docs": n_docs, "n_ids": n_ids, "reps": args.reps,
           "pack_stats": stats,
           "ms_median": {k: round(v, 3) for k, v in med.items()},
           "ms_min": {k: round(min(v), 3) for k, v in times.items()},
           "ms_max": {k: round(max(v), 3) for k, v in times.items()},
           "bytes_moved": moved,
           "gb_per_s": {k: round(moved[k] / med[k] / 1e6, 1) for k in moved},
           "call_over_copy": {k: round(med[k] / med["copy_" + k], 2) for k in med if not k.startswith("copy_")}}
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
