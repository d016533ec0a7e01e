"""Cost of the repeat call on the config-2 text (100 MB of English) resident in HBM, its rows the lines of the text, with
something to find: every 150th line stands a second time half the corpus later, and every 10th line ends in the same
templated sentence.  wp_repeat_rows_device over the ids of encode_rows_tensor at k = 13 and at the largest k <= 64 that
still has windows in these short lines, and over the text bytes at k = 50 — each plain and with mask + src + cut +
compact; in one process, the calls alternated; medians of host wall time around calls that end in a device synchronise.
The stages come from one more call per form under WP_OPT_STAGE_TIMING (HIP events inside the library, handed out through
wp_stats as the header's section "repeated spans" says).  Yardsticks beside them in the same process: the overlap call
of the same ids against every 150th line, the dedup call over the same ids, the plain encode of the same text, and the
host baseline — the Python dict loop of tests/repeat_model.py's kind over the ids of the first --host-rows rows, scaled
to all ids by their number (a dict grows with the corpus, so the scaled figure flatters the host).

Before anything is timed, the results of the first 200 rows are held to tests/repeat_model.py, and n_repeats must equal
n_windows - n_distinct.  One JSON line, appended to --out (default profiles/repeat_probe.jsonl).

    python profiles/repeat_probe.py [--mb 100] [--reps 7] [--host-rows 20000] [--out FILE]
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

import repeat_model as M  # noqa: E402
import wordpiece_amd as W  # noqa: E402
from wordpiece_amd import synth  # noqa: E402

EVERY, TEMPLATED = 150, 10
TEMPLATE = b" this page uses cookies to improve your experience , accept all or manage your settings"


def resident(text):
    n = int(text.size)
    t = torch.zeros((n + 19) // 16 * 16, dtype=torch.uint8, device="cuda:0")
    t[:n] = torch.from_numpy(text).to("cuda:0")
    return t[:n]


def corpus(mb):
    """the lines of the config-2 text, every TEMPLATED-th with the template behind it, every EVERY-th a second time half
    the corpus later -> (uint8 text, int64 row_off, the vocabulary)"""
    text, vocab = synth.parallel_corpus("english", int(mb * 1e6), 2, 29000, 0)
    text, off = W.line_rows(text)
    n_rows = int(off.size - 1)
    tmpl = np.frombuffer(TEMPLATE + b"\n", dtype=np.uint8)
    parts = []
    again = {}
    for i in range(n_rows):
        row = text[off[i]:off[i + 1]]
        if i % TEMPLATED == 0:
            row = np.concatenate((row[:-1], tmpl))
        parts.append(row)
        if i % EVERY == 0:
            again[min(i + n_rows // 2, n_rows - 1)] = row
        if i in again:
            parts.append(again.pop(i))
    text, off = W.line_rows(np.concatenate(parts))
    return text, off, vocab


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=float, default=100.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-rows", type=int, default=20000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "repeat_probe.jsonl"))
    args = ap.parse_args()
    text, off, vocab = corpus(args.mb)
    n, n_rows = int(text.size), int(off.size - 1)
    t, d_off = resident(text), torch.from_numpy(off).to("cuda:0")
    torch.cuda.synchronize()
    gv = W.Vocab(vocab, device=0)
    ids, splits = gv.encode_rows_tensor(t, d_off)
    ids, splits = ids.clone(), splits.clone()
    k_top = int(min(64, int((splits[1:] - splits[:-1]).max())))
    ref_rows = torch.arange(0, n_rows, EVERY, device="cuda:0")
    forms = {"ids_k13": (ids, splits, 13, 4), "ids_k%d" % k_top: (ids, splits, k_top, 4), "text_k50": (t, d_off, 50, 1)}
    # the first rows against the model, array by array (a prefix of the batch: its first occurrences are the batch's)
    head = 200
    for name, (data, offs, k, eb) in forms.items():
        got = gv.repeat_rows_tensor(data, offs, ngram=k, mask=True, src=True, utf8=False)
        end = int(offs[head])
        exp = M.repeat_rows(data[:end].cpu().numpy().tobytes(), offs[:head + 1].tolist(), eb, k, want=3)
        for key in ("repeats", "first_repeat", "first_src_row", "first_src_pos", "covered"):
            assert got[key][:head].tolist() == exp[key], name + ": " + key + " differs from the model"
        assert got["mask"][:end].tolist() == exp["mask"] and got["src"][:end].tolist() == exp["src"], name + ": mask or src differs from the model"
        st = gv.repeat_stats()
        assert st["n_repeats"] == st["n_windows"] - st["n_distinct"] and st["n_repeats"] > 0, name + ": the invariant of scope 0 fails"
    stats = {}
    calls = {}
    for name, (data, offs, k, eb) in forms.items():
        calls["repeat_" + name] = lambda a=(data, offs), k=k: gv.repeat_rows_tensor(*a, ngram=k, utf8=False, copy=False)
        calls["repeat_" + name + "_all"] = lambda a=(data, offs), k=k: gv.repeat_rows_tensor(*a, ngram=k, mask=True, src=True, cut=True, compact=True,
                                                                                            utf8=False, copy=False)
    calls["repeat_text_k50_utf8_all"] = lambda: gv.repeat_rows_tensor(t, d_off, ngram=50, mask=True, src=True, cut=True, compact=True, copy=False)
    for k, f in calls.items():
        f()
        stats[k] = gv.repeat_stats()
    # the overlap call's reference set: every EVERY-th row of the ids, gathered on the host once
    h_splits = splits.cpu().numpy()
    h_ids = ids.cpu().numpy()
    rrows = [h_ids[h_splits[i]:h_splits[i + 1]] for i in ref_rows.tolist()]
    rids = torch.from_numpy(np.concatenate(rrows)).to("cuda:0")
    rsplits = torch.from_numpy(np.concatenate(([0], np.cumsum([len(r) for r in rrows]))).astype(np.int64)).to("cuda:0")
    calls["overlap_ids_k13"] = lambda: gv.overlap_rows_tensor(ids, splits, rids, rsplits, ngram=13, copy=False)
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
        if name.startswith("repeat"):
            calls[name]()
            s = gv.stats()
            stages[name] = {"ms_offsets": round(s["ms_decode"], 3), "ms_keys_sort_first": round(s["ms_sa"], 3), "ms_flags_cover": round(s["ms_scan"], 3),
                            "ms_rows_cut_compact": round(s["ms_walk"], 3), "ms_total": round(s["ms_total"], 3), "radix_passes": s["radix_passes"]}
    gv.set_option(W.WP_OPT_STAGE_TIMING, 0)
    # the host baseline, over the first rows: the dict loop
    h_rows = min(args.host_rows, n_rows)
    l_ids, l_off = h_ids[:h_splits[h_rows]].tolist(), h_splits[:h_rows + 1].tolist()
    t0 = time.perf_counter()
    first = {}
    host_repeats = []
    for i in range(h_rows):
        r = 0
        for p in range(l_off[i], l_off[i + 1] - 12):
            if first.setdefault(tuple(l_ids[p:p + 13]), p) != p:
                r += 1
        host_repeats.append(r)
    ms_loop = (time.perf_counter() - t0) * 1e3
    assert host_repeats == gv.repeat_rows_tensor(ids, splits, ngram=13)["repeats"][:h_rows].tolist(), "the host baseline differs"
    out = {"config": 2, "mb": args.mb, "n_bytes": n, "n_rows": n_rows, "n_ids": int(ids.numel()), "k_top": k_top, "reps": args.reps,
           "repeat_stats": stats,
           "ms_median": {k: round(v, 3) for k, v in med.items()},
           "ms_min": {k: round(min(v), 3) for k, v in times.items()},
           "ms_max": {k: round(max(v), 3) for k, v in times.items()},
           "stages": stages,
           "host_baseline_ids_k13": {"rows": h_rows, "ids": len(l_ids), "ms_dict_loop": round(ms_loop, 1),
                                     "ms_dict_loop_scaled_to_all_ids": round(ms_loop * int(ids.numel()) / max(len(l_ids), 1), 1)}}
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
