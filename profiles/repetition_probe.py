"""Cost of the repetition call on the config-2 text (100 MB of English) resident in HBM, 20 lines of the text to a
document: wp_repetition_rows_device with the Gopher limits without and with the compact form, beside quality_rows_tensor
and encode_rows_tensor of the same batch; in one process, the calls alternated; medians of host wall time around calls
that end in a device synchronise.  The stages come from one more call under WP_OPT_STAGE_TIMING (HIP events inside the
library, handed out through wp_stats as include/wordpiece_amd_repetition.h says): word identity (with the intake, the
class passes and the word list), the five sorts, the LCP with the run passes, the cover with the rules.

  host_model       tests/repetition_model.py over the first --sample documents, SCALED by bytes to the whole text

The signals and reasons of the first 200 documents are held against the model before anything is timed.  One JSON line,
appended to --out (default profiles/repetition_probe.jsonl).

    python profiles/repetition_probe.py [--mb 100] [--reps 7] [--lines 20] [--sample 400] [--out FILE]
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

import repetition_model as M  # noqa: E402
import wordpiece_amd as W  # noqa: E402
from wordpiece_amd import repetition as R  # noqa: E402
from wordpiece_amd import synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=float, default=100.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--lines", type=int, default=20)
    ap.add_argument("--sample", type=int, default=400)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "repetition_probe.jsonl"))
    args = ap.parse_args()
    text, vocab = synth.parallel_corpus("english", int(args.mb * 1e6), 2, 29000, 0)
    text, line_off = W.line_rows(text)
    off = np.ascontiguousarray(np.concatenate((line_off[:-1:args.lines], line_off[-1:])))
    n, n_rows = int(text.size), int(off.size - 1)
    t = torch.zeros((n + 19) // 16 * 16, dtype=torch.uint8, device="cuda:0")
    t[:n] = torch.from_numpy(text).to("cuda:0")
    d_off = torch.from_numpy(off).to("cuda:0")
    torch.cuda.synchronize()
    gv = W.Vocab(vocab, device=0)
    q_rules = W.quality_rules("gopher")
    stop = [w.encode() for w in q_rules.pop("stop_words")]
    # the first documents, once, against the model; the model's time on a sample, scaled by bytes
    head = min(200, n_rows)
    got = R.repetition_rows_tensor(gv, t[:n], d_off, rules="gopher", copy=False)
    exp = M.repetition(text[:off[head]].tobytes(), off[:head + 1].tolist(), limit=M.limits(**M.GOPHER))
    assert got["signals"][:, :head].cpu().numpy().tolist() == exp["signals"], "the signals differ from the model's"
    assert got["reasons"][:head].cpu().numpy().view(np.uint32).tolist() == exp["reasons"], "the reasons differ from the model's"
    r_stats = R.repetition_stats(gv)
    sample = min(args.sample, n_rows)
    t0 = time.perf_counter()
    M.repetition(text[:off[sample]].tobytes(), off[:sample + 1].tolist(), limit=M.limits(**M.GOPHER))
    ms_model_sample = (time.perf_counter() - t0) * 1e3
    calls = {
        "repetition": lambda: R.repetition_rows_tensor(gv, t[:n], d_off, rules="gopher", copy=False),
        "repetition_compact": lambda: R.repetition_rows_tensor(gv, t[:n], d_off, rules="gopher", compact=True, copy=False),
        "quality": lambda: gv.quality_rows_tensor(t[:n], d_off, rules=q_rules, stop_words=stop, copy=False),
        "encode_rows": lambda: gv.encode_rows_tensor(t[:n], d_off, copy=False),
    }
    times = {k: [] for k in calls}
    for f in calls.values():  # warm-up (code objects, the buffers)
        f()
        f()
    for _ in range(args.reps):
        for k, f in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            times[k].append((time.perf_counter() - t0) * 1e3)
    med = {k: statistics.median(v) for k, v in times.items()}
    gv.set_option(W.WP_OPT_STAGE_TIMING, 1)
    calls["repetition_compact"]()
    s = gv.stats()
    stages = {"ms_word_identity": round(s["ms_decode"], 3), "ms_five_sorts": round(s["ms_sa"], 3), "ms_lcp_runs": round(s["ms_scan"], 3),
              "ms_cover_rules_compact": round(s["ms_walk"], 3), "ms_total": round(s["ms_total"], 3)}
    gv.set_option(W.WP_OPT_STAGE_TIMING, 0)
    scaled = ms_model_sample * n / max(1, int(off[sample]))
    out = {"config": 2, "mb": args.mb, "n_bytes": n, "n_rows": n_rows, "lines_per_doc": args.lines, "reps": args.reps, "repetition_stats": r_stats,
           "ms_median": {k: round(v, 3) for k, v in med.items()},
           "ms_min": {k: round(min(v), 3) for k, v in times.items()},
           "ms_max": {k: round(max(v), 3) for k, v in times.items()},
           "stages": stages, "per_kernel_counters": "not measured", "long_repeated_runs": "not measured",
           "host_model": {"sample_rows": sample, "sample_bytes": int(off[sample]), "ms_sample": round(ms_model_sample, 1),
                          "ms_scaled_by_bytes": round(scaled, 1), "scaled": True},
           "gb_per_s": {k: round(n / med[k] / 1e6, 2) for k in ("repetition", "repetition_compact")},
           "repetition_over_quality": round(med["repetition"] / med["quality"], 3),
           "repetition_over_encode": round(med["repetition"] / med["encode_rows"], 3),
           "host_model_scaled_over_repetition": round(scaled / med["repetition"], 1)}
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
