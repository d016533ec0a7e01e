"""Cost of the overlap call on the config-2 text (100 MB of English) resident in HBM, its rows the lines of the text,
against a reference set of every 150th line of the same text (so the rows that truly hit are known) and as many lines
of a text that does not occur in it: wp_overlap_rows_device over the ids of encode_rows_tensor at k = 13 and k = 64 and
over the text bytes at k = 50, with and without mask + ref + compact; in one process, the calls alternated; medians of
host wall time around calls that end in a device synchronise.  The stages come from one more call per form under
WP_OPT_STAGE_TIMING (HIP events inside the library, handed out through wp_stats as the header's section "n-gram
overlap" says): the reference table on its own.  Yardsticks beside them: the dedup call over the same ids, the plain
encode of the same text, and the host baseline — a Python set of the reference windows (tuples of ids) and a loop over
the windows of the first --host-rows corpus rows.

Before anything is timed, the results of the first 200 rows are held to tests/overlap_model.py, and every 150th row must
hit.  One JSON line, appended to --out (default profiles/overlap_probe.jsonl).

    python profiles/overlap_probe.py [--mb 100] [--reps 7] [--host-rows 20000] [--out FILE]
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

import overlap_model as M  # noqa: E402
import wordpiece_amd as W  # noqa: E402
from wordpiece_amd import synth  # noqa: E402

EVERY = 150


def resident(text):
    n = int(text.size)
    t = torch.zeros((n + 19) // 16 * 16, dtype=torch.uint8, device="cuda:0")
    t[:n] = torch.from_numpy(text).to("cuda:0")
    return t[:n]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=float, default=100.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-rows", type=int, default=20000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "overlap_probe.jsonl"))
    args = ap.parse_args()
    text, vocab = synth.parallel_corpus("english", int(args.mb * 1e6), 2, 29000, 0)
    text, off = W.line_rows(text)
    n, n_rows = int(text.size), int(off.size - 1)
    leaked = np.arange(0, n_rows, EVERY)
    other, _ = synth.parallel_corpus("english", int(args.mb * 1e6 * len(leaked) / n_rows) + 1000, 2, 29000, 3)  # (another word sequence over the same lexicon)
    other, other_off = W.line_rows(other)
    n_other = min(len(leaked), int(other_off.size - 1))
    ref_text = np.concatenate([text[off[i]:off[i + 1]] for i in leaked] + [other[:other_off[n_other]]])
    ref_text, ref_off = W.line_rows(ref_text)
    t, d_off, rt, d_roff = resident(text), torch.from_numpy(off).to("cuda:0"), resident(ref_text), torch.from_numpy(ref_off).to("cuda:0")
    torch.cuda.synchronize()
    gv = W.Vocab(vocab, device=0)
    ids, splits = gv.encode_rows_tensor(t, d_off)
    ids, splits = ids.clone(), splits.clone()
    rids, rsplits = gv.encode_rows_tensor(rt, d_roff)
    rids, rsplits = rids.clone(), rsplits.clone()
    forms = {"ids_k13": (ids, splits, rids, rsplits, 13, 4), "ids_k64": (ids, splits, rids, rsplits, 64, 4), "text_k50": (t, d_off, rt, d_roff, 50, 1)}
    # the first rows against the model, array by array; the leaked rows hit
    head = 200
    for name, (data, offs, rdata, roffs, k, eb) in forms.items():
        got = gv.overlap_rows_tensor(data, offs, rdata, roffs, ngram=k, mask=True)
        end = int(offs[head])
        exp = M.overlap_rows(data[:end].cpu().numpy().tobytes(), offs[:head + 1].tolist(), rdata.cpu().numpy().tobytes(), roffs.tolist(), eb, k, want=1)
        for key in ("hits", "first_hit", "first_ref", "covered"):
            assert got[key][:head].tolist() == exp[key], name + ": " + key + " differs from the model"
        assert got["mask"][:end].tolist() == exp["mask"], name + ": mask differs from the model"
        at = torch.from_numpy(leaked).to(offs.device)
        long_enough = (offs[1:] - offs[:-1])[at] >= k
        assert bool((got["hits"][at][long_enough] > 0).all()), name + ": a leaked row does not hit"
    stats = {}
    calls = {}
    for name, (data, offs, rdata, roffs, k, eb) in forms.items():
        calls["overlap_" + name] = lambda a=(data, offs, rdata, roffs), k=k: gv.overlap_rows_tensor(*a, ngram=k, copy=False)
        calls["overlap_" + name + "_all"] = lambda a=(data, offs, rdata, roffs), k=k: gv.overlap_rows_tensor(*a, ngram=k, mask=True, ref=True, compact=True,
                                                                                                      copy=False)
    for k, f in calls.items():
        f()
        stats[k] = gv.overlap_stats()
    calls["dedup_ids"] = lambda: gv.dedup_rows_tensor(ids, splits, copy=False)
    calls["encode_tensor"] = lambda: gv.encode_tensor(t, copy=False)
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
        if name.startswith("overlap"):
            calls[name]()
            s = gv.stats()
            stages[name] = {"ms_offsets": round(s["ms_decode"], 3), "ms_table": round(s["ms_sa"], 3), "ms_lookup": round(s["ms_scan"], 3),
                            "ms_rows_compact": round(s["ms_walk"], 3), "ms_total": round(s["ms_total"], 3)}
    gv.set_option(W.WP_OPT_STAGE_TIMING, 0)
    # the host baseline, over the first rows: a set of the reference windows, a loop over the corpus windows
    h_rows = min(args.host_rows, n_rows)
    h_ids, h_off = ids[:int(splits[h_rows])].cpu().numpy().tolist(), splits[:h_rows + 1].tolist()
    r_ids, r_off = rids.cpu().numpy().tolist(), rsplits.tolist()
    t0 = time.perf_counter()
    table = set()
    for j in range(len(r_off) - 1):
        for p in range(r_off[j], r_off[j + 1] - 12):
            table.add(tuple(r_ids[p:p + 13]))
    ms_set = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    host_hits = [sum(1 for p in range(h_off[i], h_off[i + 1] - 12) if tuple(h_ids[p:p + 13]) in table) for i in range(h_rows)]
    ms_loop = (time.perf_counter() - t0) * 1e3
    assert host_hits == gv.overlap_rows_tensor(ids, splits, rids, rsplits, ngram=13)["hits"][:h_rows].tolist(), "the host baseline differs"
    out = {"config": 2, "mb": args.mb, "n_bytes": n, "n_rows": n_rows, "n_ids": int(ids.numel()), "n_ref_rows": int(ref_off.size - 1),
           "n_ref_ids": int(rids.numel()), "reps": args.reps, "overlap_stats": stats,
           "ms_median": {k: round(v, 3) for k, v in med.items()},
           "ms_min": {k: round(min(v), 3) for k, v in times.items()},
           "ms_max": {k: round(max(v), 3) for k, v in times.items()},
           "stages": stages,
           "host_baseline_ids_k13": {"rows": h_rows, "ids": len(h_ids), "ms_reference_set": round(ms_set, 1), "ms_corpus_loop": round(ms_loop, 1),
                                     "ms_corpus_loop_scaled_to_all_ids": round(ms_loop * int(ids.numel()) / max(len(h_ids), 1), 1)}}
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
