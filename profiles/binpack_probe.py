"""Cost and fill of best-fit packing beside next fit on the config-2 text (100 MB of English): the text goes through
encode_rows_tensor once, then the same ids are packed as its lines (one document each) and as documents of 20 lines
(75,425 of them), at max_len 128, 512 and 2048, [CLS] / [SEP] around every unit, all five outputs, into caller-owned
buffers; in one process, the calls alternated; medians of host wall time around calls that end in a device synchronise:

  best_fit_<rows>_<L>   wordpiece_amd.binpack.pack_best_fit_tensor, long_docs "split"
  next_fit_<rows>_<L>   Vocab.pack_sequences_tensor, mode "next_fit", long_docs "split"

Per call also n_out, the fill n_cells / (n_out * max_len), for best fit the runs and row ranges of its plan, and the host
time of the planner alone on that call's length histogram (plan_best_fit, median of the same number of runs).

One JSON line, appended to --out (default profiles/binpack_probe.jsonl).

    python profiles/binpack_probe.py [--mb 100] [--reps 9] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library: torch's HIP runtime serves the process)

import wordpiece_amd as W  # noqa: E402
from wordpiece_amd import binpack, synth  # noqa: E402

CLS, SEP = 101, 102


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=float, default=100.0)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "binpack_probe.jsonl"))
    args = ap.parse_args()
    text, vocab = synth.parallel_corpus("english", int(args.mb * 1e6), 2, 29000, 0)
    n = len(text)
    dev = torch.device("cuda:0")
    t = torch.zeros((n + 19) // 16 * 16, dtype=torch.uint8, device=dev)
    t[:n] = torch.frombuffer(bytearray(text), dtype=torch.uint8).to(dev)
    torch.cuda.synchronize()
    gv = W.Vocab(vocab, device=0)
    ids, line_splits = gv.encode_rows_tensor(t[:n])  # (copies)
    n_lines = line_splits.numel() - 1
    at = torch.arange(0, n_lines + 20, 20, device=dev).clamp(max=n_lines)
    rows = {"lines": line_splits, "docs": line_splits[at].contiguous()}
    calls, info, hists = {}, {}, {}
    for shape, splits in rows.items():
        lens = np.diff(splits.cpu().numpy())
        for L in (128, 512, 2048):
            kw = dict(max_len=L, bos_id=CLS, eos_id=SEP, long_docs="split")
            B_ = L - 2
            u = np.concatenate([np.full(int((lens // B_).sum()), L), lens[lens % B_ > 0] % B_ + 2])  # the unit lengths under split
            hists[(shape, L)] = np.bincount(u, minlength=L + 1).astype(np.int64)
            best = binpack.pack_best_fit_tensor(gv, ids, splits, **kw)
            bs = binpack.binpack_stats(gv)
            nxt = gv.pack_sequences_tensor(ids, splits, mode="next_fit", **kw)
            ps = gv.pack_stats()
            for name, st in (("best_fit", bs), ("next_fit", ps)):
                info["%s_%s_%d" % (name, shape, L)] = dict(n_docs=st["n_docs"], n_pieces=st["n_pieces"], n_out=st["n_out"], n_cells=st["n_cells"],
                                                           fill=round(st["n_cells"] / (st["n_out"] * L), 4))
            info["best_fit_%s_%d" % (shape, L)].update(n_runs=bs["n_runs"], n_row_ranges=bs["n_row_ranges"])
            calls["best_fit_%s_%d" % (shape, L)] = lambda s=splits, kw=kw, o=best: binpack.pack_best_fit_tensor(gv, ids, s, out=o, **kw)
            calls["next_fit_%s_%d" % (shape, L)] = lambda s=splits, kw=kw, o=nxt: gv.pack_sequences_tensor(ids, s, mode="next_fit", out=o, **kw)
    torch.cuda.synchronize()
    for f in calls.values():  # warm-up (buffer growth, code objects)
        f()
        f()
    times = {k: [] for k in calls}
    for _ in range(args.reps):
        for k, f in calls.items():
            t0 = time.perf_counter()
            f()
            times[k].append((time.perf_counter() - t0) * 1e3)
    plan_ms = {}
    for (shape, L), h in hists.items():
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            p = binpack.plan_best_fit(h, L)
            ts.append((time.perf_counter() - t0) * 1e3)
        assert p["n_out"] == info["best_fit_%s_%d" % (shape, L)]["n_out"], "the planner and the call disagree"
        plan_ms["%s_%d" % (shape, L)] = round(statistics.median(ts), 3)
    out = {"config": 2, "mb": args.mb, "n_bytes": n, "n_ids": ids.numel(), "n_lines": n_lines, "reps": args.reps, "calls": info,
           "ms_median": {k: round(statistics.median(v), 3) for k, v in times.items()},
           "ms_min": {k: round(min(v), 3) for k, v in times.items()},
           "ms_max": {k: round(max(v), 3) for k, v in times.items()},
           "plan_host_ms_median": plan_ms}
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
