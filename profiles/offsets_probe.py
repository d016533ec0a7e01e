"""Cost of offsets mode: wp_linear_encode_device against wp_linear_encode_offsets_device (byte and code-point units)
on configs 2, 3 and 5, in one process, the calls alternated; medians.  Also the host entry points on config 2 and the
arena bytes per symbol of each mode.  One JSON line per config.

    python profiles/offsets_probe.py [--configs 2,3,5] [--mb 2=100,3=1000,5=1000] [--reps 7]
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

KINDS = {2: ("english", 100.0, 29000), 3: ("multilingual", 1000.0, 120000), 5: ("deep", 1000.0, 0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="2,3,5")
    ap.add_argument("--mb", default="", help="per-config sizes in MB, e.g. 2=100,3=300")
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    sizes = {int(k): float(v) for k, v in (kv.split("=") for kv in args.mb.split(",") if kv)}
    for cfg in (int(c) for c in args.configs.split(",")):
        kind, mb, vs = KINDS[cfg]
        mb = sizes.get(cfg, mb)
        text, vocab = synth.parallel_corpus(kind, int(mb * 1e6), 2, vs, 0)
        n = len(text)
        t = torch.zeros((n + 19) // 16 * 16, dtype=torch.uint8, device="cuda:0")
        t[:n] = torch.frombuffer(bytearray(text), dtype=torch.uint8).to("cuda:0")
        torch.cuda.synchronize()
        gv = W.Vocab(vocab, device=0)
        calls = {
            "ids": lambda: gv.encode_device(t.data_ptr(), n),
            "offsets_byte": lambda: gv.encode_device_with_offsets(t.data_ptr(), n, "byte"),
            "offsets_char": lambda: gv.encode_device_with_offsets(t.data_ptr(), n, "char"),
        }
        times, arena, stats = {k: [] for k in calls}, {}, {}
        for k, f in calls.items():  # warm-up (arena growth)
            f()
            f()
        for _ in range(args.reps):
            for k, f in calls.items():
                t0 = time.perf_counter()
                f()
                times[k].append((time.perf_counter() - t0) * 1e3)
                st = gv.stats()
                arena[k] = st["arena_bytes"] / max(st["n_total"], 1)
                stats[k] = (st["anchor_mode"], st["staged_emit"], st["n_ids"])
        med = {k: statistics.median(v) for k, v in times.items()}
        out = {"config": cfg, "mb": mb, "n_bytes": n, "n_ids": stats["ids"][2], "anchor_mode": stats["ids"][0],
               "staged_emit": stats["ids"][1], "ms_median": {k: round(v, 3) for k, v in med.items()},
               "ratio_byte": round(med["offsets_byte"] / med["ids"], 3), "ratio_char": round(med["offsets_char"] / med["ids"], 3),
               "arena_bytes_per_symbol": {k: round(v, 1) for k, v in arena.items()}}
        if cfg == 2:  # host entry points: upload, device path, download (8 more bytes per id)
            h = {"ids": [], "offsets_byte": []}
            gv.encode(text)
            gv.encode_with_offsets(text)
            for _ in range(args.reps):
                t0 = time.perf_counter()
                gv.encode(text)
                h["ids"].append((time.perf_counter() - t0) * 1e3)
                t0 = time.perf_counter()
                gv.encode_with_offsets(text)
                h["offsets_byte"].append((time.perf_counter() - t0) * 1e3)
            hm = {k: statistics.median(v) for k, v in h.items()}
            out["host_ms_median"] = {k: round(v, 3) for k, v in hm.items()}
            out["host_ratio_byte"] = round(hm["offsets_byte"] / hm["ids"], 3)
        print(json.dumps(out), flush=True)
        del gv, t
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
