"""Cost of the neardup call on the config-2 text (100 MB of English) resident in HBM, its rows the lines of the text:
wp_neardup_rows_device over the text bytes and over the ids of encode_rows_tensor, at (k = 5, n_perm = 128, bands = 16)
and (k = 5, n_perm = 256, bands = 32), min_agree = ceil(0.5 n_perm); in one process, the calls alternated; medians of host
wall time around calls that end in a device synchronise.  The stages come from one more call per form under
WP_OPT_STAGE_TIMING (HIP events inside the library, handed out through wp_stats as the header's section "near-duplicate
rows" says).  Yardsticks beside them: the dedup calls and the plain encode of the same text.

Before anything is timed, the signatures of the first rows are compared with tests/neardup_model.py, and rows that are
byte-equal (dedup's `first`) must share a cluster.  One JSON line, appended to --out (default
profiles/neardup_probe.jsonl).

    python profiles/neardup_probe.py [--mb 100] [--reps 7] [--out FILE]
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

import neardup_model as M  # noqa: E402
import wordpiece_amd as W  # noqa: E402
from wordpiece_amd import synth  # noqa: E402

SHAPES = {"128x16": dict(shingle=5, n_perm=128, bands=16), "256x32": dict(shingle=5, n_perm=256, bands=32)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=float, default=100.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "neardup_probe.jsonl"))
    args = ap.parse_args()
    text, vocab = synth.parallel_corpus("english", int(args.mb * 1e6), 2, 29000, 0)
    text, off = W.line_rows(text)
    n, n_rows = int(text.size), int(off.size - 1)
    t = torch.zeros((n + 19) // 16 * 16, dtype=torch.uint8, device="cuda:0")
    t[:n] = torch.from_numpy(text).to("cuda:0")
    d_off = torch.from_numpy(off).to("cuda:0")
    torch.cuda.synchronize()
    gv = W.Vocab(vocab, device=0)
    ids, splits = gv.encode_rows_tensor(t[:n], d_off)
    # the first rows against the model, entry by entry; byte-equal rows share a cluster
    head = 200
    for name, data, offs, eb in (("text", t[:n], d_off, 1), ("ids", ids, splits, 4)):
        got = gv.neardup_rows_tensor(data, offs, signatures=True, **SHAPES["128x16"])
        end = int(offs[head])
        exp = M.neardup_rows(data[:end].cpu().numpy().tobytes(), offs[:head + 1].tolist(), eb, want=4, **SHAPES["128x16"])
        assert np.array_equal(got["signatures"][:head].cpu().numpy().view(np.uint32), exp["signatures"]), name + ": signatures differ from the model"
        first = gv.dedup_rows_tensor(data, offs)["first"].long()
        assert bool((got["cluster"][first.to(got["cluster"].device)] == got["cluster"]).all()), name + ": equal rows in two clusters"
    stats = {}
    calls = {}
    for shape, spec in SHAPES.items():
        kw = dict(spec, min_agree=W.lsh_min_agree(0.5, spec["n_perm"]), copy=False)
        calls["neardup_text_" + shape] = lambda kw=kw: gv.neardup_rows_tensor(t[:n], d_off, **kw)
        calls["neardup_ids_" + shape] = lambda kw=kw: gv.neardup_rows_tensor(ids, splits, **kw)
        calls["neardup_ids_compact_" + shape] = lambda kw=kw: gv.neardup_rows_tensor(ids, splits, inverse=True, compact=True, **kw)
    for k, f in calls.items():
        f()
        stats[k] = gv.neardup_stats()
    calls["dedup_text"] = lambda: gv.dedup_rows_tensor(t[:n], d_off, copy=False)
    calls["dedup_ids"] = lambda: gv.dedup_rows_tensor(ids, splits, copy=False)
    calls["encode_tensor"] = lambda: gv.encode_tensor(t[:n], copy=False)
    times = {k: [] for k in calls}
    for f in calls.values():  # warm-up (code objects, the buffers)
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
    for name in calls:
        if name.startswith("neardup"):
            calls[name]()
            s = gv.stats()
            stages[name] = {"ms_list": round(s["ms_decode"], 3), "ms_signatures": round(s["ms_scan"], 3), "ms_grouping": round(s["ms_sa"], 3),
                            "ms_components_table": round(s["ms_walk"], 3), "ms_total": round(s["ms_total"], 3),
                            "radix_passes": s["radix_passes"], "radix_pass_bytes": s["radix_pass_bytes"]}
    gv.set_option(W.WP_OPT_STAGE_TIMING, 0)
    out = {"config": 2, "mb": args.mb, "n_bytes": n, "n_rows": n_rows, "n_ids": int(ids.numel()), "reps": args.reps,
           "neardup_stats": stats,
           "ms_median": {k: round(v, 3) for k, v in med.items()},
           "ms_min": {k: round(min(v), 3) for k, v in times.items()},
           "ms_max": {k: round(max(v), 3) for k, v in times.items()},
           "stages": stages}
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
