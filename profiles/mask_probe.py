"""Cost of the masking call on the config-2 text (100 MB of English, the rows are its lines): the text goes through
encode_inputs_tensor at max_len 128 into caller-owned buffers, then the mask call runs on that batch; in one process,
the calls alternated; medians of host wall time around calls that end in a device synchronise:

  inputs_128     wp_linear_encode_inputs_device, pairs 0, longest_first, [CLS] / [SEP]   (the call the mask call follows)
  mask           wp_mlm_mask_device, whole words, 15 % / 80 / 10 / 10, into buffers of its own: 4 B in, 8 B out per cell
  mask_word_ids  the same with word_ids: 12 B out per cell
  mask_in_place  the same as `mask`, masked ids over the batch
  word_ids       wp_word_ids_device alone: 4 B in, 4 B out per cell
  copy_12b       the yardstick: one device-to-device memcpy that moves the bytes the mask call moves — 6 B per cell read
                 and 6 B per cell written (torch's copy_ between contiguous uint8 tensors, a hipMemcpyDtoD, and one
                 synchronise)

One JSON line, appended to --out (default profiles/mask_probe.jsonl).

    python profiles/mask_probe.py [--mb 100] [--reps 9] [--max-len 128] [--out FILE]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mask_probe.jsonl"))
    args = ap.parse_args()
    L = args.max_len
    text, vocab = synth.parallel_corpus("english", int(args.mb * 1e6), 2, 29000, 0)
    vocab = list(vocab) + ["[MASK]"]
    mask_id = len(vocab) - 1
    n = len(text)
    t = torch.zeros((n + 19) // 16 * 16, dtype=torch.uint8, device="cuda:0")
    t[:n] = torch.frombuffer(bytearray(text), dtype=torch.uint8).to("cuda:0")
    torch.cuda.synchronize()
    gv = W.Vocab(vocab, device=0)
    n_rows = gv.encode_rows_tensor(t[:n], copy=False)[1].numel() - 1
    kw = dict(max_len=L, cls_id=101, sep_id=102)
    new = lambda: torch.empty((n_rows, L), dtype=torch.int32, device="cuda:0")
    own = {"input_ids": new(), "token_type_ids": new(), "lengths": torch.empty(n_rows, dtype=torch.int32, device="cuda:0"),
           "sample": torch.empty(n_rows, dtype=torch.int32, device="cuda:0")}
    masked, labels, wids, work = new(), new(), new(), new()
    batch = gv.encode_inputs_tensor(t[:n], out=own, **kw)
    ids, lens = batch["input_ids"], batch["lengths"]
    work.copy_(ids)
    spec = W._mask_spec(L, mask_id, 0.15, 0.8, 0.1, True, 0, 0, -100, 101, 102, 0)
    ptr = lambda x: None if x is None else W.C.c_void_p(x.data_ptr())
    seed = [0]

    def mask(src, dst, wid):
        seed[0] += 1  # (a new seed every call: dynamic masking)
        spec.seed = seed[0]
        W._check(W.lib().wp_mlm_mask_device(gv._h, ptr(src), ptr(lens), n_rows, W.C.byref(spec), ptr(dst), ptr(labels), ptr(wid)))

    cells = n_rows * L
    src6 = torch.empty(6 * cells, dtype=torch.uint8, device="cuda:0")
    dst6 = torch.empty(6 * cells, dtype=torch.uint8, device="cuda:0")

    def copy_12b():
        dst6.copy_(src6)
        torch.cuda.synchronize()

    calls = {
        "inputs_128": lambda: gv.encode_inputs_tensor(t[:n], out=own, **kw),
        "mask": lambda: mask(ids, masked, None),
        "mask_word_ids": lambda: mask(ids, masked, wids),
        "mask_in_place": lambda: mask(work, work, None),
        "word_ids": lambda: W._check(W.lib().wp_word_ids_device(gv._h, ptr(ids), ptr(lens), n_rows, W.C.byref(spec), ptr(wids))),
        "copy_12b": copy_12b,
    }
    times, mstats = {k: [] for k in calls}, {}
    torch.cuda.synchronize()
    for f in calls.values():  # warm-up (arena growth, code objects, the class table)
        f()
        f()
    for _ in range(args.reps):
        for k, f in calls.items():
            t0 = time.perf_counter()
            f()
            times[k].append((time.perf_counter() - t0) * 1e3)
            if k == "mask":
                mstats = gv.mask_stats()
    med = {k: statistics.median(v) for k, v in times.items()}
    moved = {"mask": 12 * cells, "mask_word_ids": 16 * cells, "mask_in_place": 12 * cells, "word_ids": 8 * cells, "copy_12b": 12 * cells}
    out = {"config": 2, "mb": args.mb, "n_bytes": n, "n_rows": n_rows, "max_len": L, "cells": cells, "reps": args.reps,
           "mask_stats": mstats,
           "ms_median": {k: round(v, 3) for k, v in med.items()},
           "ms_min": {k: round(min(v), 3) for k, v in times.items()},
           "ms_max": {k: round(max(v), 3) for k, v in times.items()},
           "bytes_moved": moved,
           "gb_per_s": {k: round(moved[k] / med[k] / 1e6, 1) for k in moved},
           "mask_over_copy_12b": round(med["mask"] / med["copy_12b"], 3),
           "mask_over_inputs": round(med["mask"] / med["inputs_128"], 4)}
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
