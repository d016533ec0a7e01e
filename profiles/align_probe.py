"""Cost of the span-alignment call on the config-2 text (100 MB of English, the rows are its lines): the text goes through
encode_inputs_tensor at max_len 128 with byte offsets into caller-owned buffers, then the align call runs on that batch
with one labelled span per sample; in one process, the calls alternated; medians of host wall time around calls that
end in a device synchronise:

  align_labels     wp_align_device, labels only: 8 B offsets + 4 B type in, 4 B out per cell
  align_positions  the same, start / end positions only: 12 B in per cell, 8 B out per row
  align_both       labels and positions: 12 B in, 4 B out per cell
  align_all        labels, span_index and positions: 12 B in, 8 B out per cell
  word_ids         the yardstick, a call of the same geometry on the same batch: wp_word_ids_device, 4 B in, 4 B out per cell

One JSON line, appended to --out (default profiles/align_probe.jsonl).

    python profiles/align_probe.py [--mb 100] [--reps 9] [--max-len 128] [--out FILE]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_probe.jsonl"))
    args = ap.parse_args()
    L = args.max_len
    text, vocab = synth.parallel_corpus("english", int(args.mb * 1e6), 2, 29000, 0)
    n = len(text)
    t = torch.zeros((n + 19) // 16 * 16, dtype=torch.uint8, device="cuda:0")
    t[:n] = torch.frombuffer(bytearray(text), dtype=torch.uint8).to("cuda:0")
    torch.cuda.synchronize()
    gv = W.Vocab(vocab, device=0)
    n_rows = gv.encode_rows_tensor(t[:n], copy=False)[1].numel() - 1
    new = lambda *shape: torch.empty(shape, dtype=torch.int32, device="cuda:0")
    own = {"input_ids": new(n_rows, L), "token_type_ids": new(n_rows, L), "lengths": new(n_rows), "sample": new(n_rows),
           "offsets": new(n_rows, L, 2)}
    batch = gv.encode_inputs_tensor(t[:n], out=own, max_len=L, cls_id=101, sep_id=102, offsets="byte")
    assert batch["input_ids"].shape[0] == n_rows
    # one span per sample, its place and length a function of the sample's number: bytes [b, b + 1 + s % 13), b = 7 s % 40
    s = torch.arange(n_rows, dtype=torch.int64, device="cuda:0")
    begin = (7 * s) % 40
    spans = torch.stack((begin, begin + 1 + s % 13), dim=1).to(torch.int32).contiguous()
    splits = torch.arange(n_rows + 1, dtype=torch.int64, device="cuda:0")
    span_labels = (1 + s % 9).to(torch.int32)
    labels, index, start, end, wids = new(n_rows, L), new(n_rows, L), new(n_rows), new(n_rows), new(n_rows, L)
    spec = W.AlignSpec(max_len=L, side=0, outside_label=0, inside_add=1, ignore_id=-100, no_answer=0)
    mspec = W.MaskSpec(max_len=L, cls_id=101, sep_id=102, pad_id=0)
    ptr = lambda x: None if x is None else W.C.c_void_p(x.data_ptr())

    def align(lab, idx, pos):
        W._check(W.lib().wp_align_device(gv._h, ptr(own["offsets"]), ptr(own["token_type_ids"]), ptr(own["lengths"]), ptr(own["sample"]), n_rows,
                                         ptr(splits), n_rows, ptr(spans), ptr(span_labels), n_rows, W.C.byref(spec), ptr(lab), ptr(idx),
                                         ptr(start) if pos else None, ptr(end) if pos else None))

    calls = {
        "align_labels": lambda: align(labels, None, False),
        "align_positions": lambda: align(None, None, True),
        "align_both": lambda: align(labels, None, True),
        "align_all": lambda: align(labels, index, True),
        "word_ids": lambda: W._check(W.lib().wp_word_ids_device(gv._h, ptr(own["input_ids"]), ptr(own["lengths"]), n_rows, W.C.byref(mspec), ptr(wids))),
    }
    times, astats = {k: [] for k in calls}, {}
    torch.cuda.synchronize()
    for f in calls.values():  # warm-up (code objects, the class table)
        f()
        f()
    for _ in range(args.reps):
        for k, f in calls.items():
            t0 = time.perf_counter()
            f()
            times[k].append((time.perf_counter() - t0) * 1e3)
            if k == "align_all":
                astats = gv.align_stats()
    med = {k: statistics.median(v) for k, v in times.items()}
    cells = n_rows * L
    moved = {"align_labels": 16 * cells, "align_positions": 12 * cells + 8 * n_rows, "align_both": 16 * cells + 8 * n_rows,
             "align_all": 20 * cells + 8 * n_rows, "word_ids": 8 * cells}
    out = {"config": 2, "mb": args.mb, "n_bytes": n, "n_rows": n_rows, "max_len": L, "cells": cells, "reps": args.reps,
           "align_stats": astats,
           "ms_median": {k: round(v, 3) for k, v in med.items()},
           "ms_min": {k: round(min(v), 3) for k, v in times.items()},
           "ms_max": {k: round(max(v), 3) for k, v in times.items()},
           "bytes_moved": moved,
           "gb_per_s": {k: round(moved[k] / med[k] / 1e6, 1) for k in moved},
           "align_labels_over_word_ids": round(med["align_labels"] / med["word_ids"], 3),
           "align_both_over_word_ids": round(med["align_both"] / med["word_ids"], 3)}
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
