"""Cost of the word-count call on the config-2 text (100 MB of English) resident in HBM: wp_count_words_device for both
orders, with and without word_index; in one process, the calls alternated; medians of host wall time around calls that end
in a device synchronise.  Its stages come from one more call per order under WP_OPT_STAGE_TIMING (HIP events inside the
library, handed out through wp_stats as the header's section "word counts" says).  Two yardsticks beside them:

  encode_tensor    the handle's plain encode of the same text
  host_counter     collections.Counter over the split of the text on the host (the regular expression below gives the split
                   of tests/count_model.py on this ASCII text; the first 200 kB are held against the model itself)

The table of the device is compared with the host's before anything is timed.  One JSON line, appended to --out (default
profiles/count_probe.jsonl).

    python profiles/count_probe.py [--mb 100] [--reps 7] [--out FILE]
"""
import argparse
import json
import os
import re
import statistics
import sys
import time
from collections import Counter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402  (before the library: torch's HIP runtime serves the process)

import wordpiece_amd as W  # noqa: E402
from wordpiece_amd import synth  # noqa: E402

SPLIT = re.compile(rb"[A-Za-z0-9]+|[^\sA-Za-z0-9]")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=float, default=100.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "count_probe.jsonl"))
    args = ap.parse_args()
    text, vocab = synth.parallel_corpus("english", int(args.mb * 1e6), 2, 29000, 0)
    n = len(text)
    import count_model as CM
    head = text[:200_000]
    assert SPLIT.findall(head) == CM.split(head), "the host split is not the model's on this text"
    t0 = time.perf_counter()
    words = SPLIT.findall(text)
    ms_split = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    host = Counter(words)
    ms_counter = (time.perf_counter() - t0) * 1e3
    t = torch.zeros((n + 19) // 16 * 16, dtype=torch.uint8, device="cuda:0")
    t[:n] = torch.frombuffer(bytearray(text), dtype=torch.uint8).to("cuda:0")
    torch.cuda.synchronize()
    gv = W.Vocab(vocab, device=0)
    # the table itself, once, against the host's
    got = gv.count_words_tensor(t[:n], order="count", index=True, copy=False)
    pairs = host.most_common()
    assert got["words"].cpu().numpy().tobytes() == b"".join(w for w, _ in pairs), "the table differs from the host's"
    assert got["counts"].tolist() == [c for _, c in pairs] and got["word_index"].numel() == len(words)
    stats = gv.count_stats()
    calls = {
        "count_first": lambda: gv.count_words_tensor(t[:n], order="first", copy=False),
        "count_first_index": lambda: gv.count_words_tensor(t[:n], order="first", index=True, copy=False),
        "count_count": lambda: gv.count_words_tensor(t[:n], order="count", copy=False),
        "count_count_index": lambda: gv.count_words_tensor(t[:n], order="count", index=True, copy=False),
        "encode_tensor": lambda: gv.encode_tensor(t[:n], copy=False),
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
    # the stages, by HIP events inside the library
    stages = {}
    gv.set_option(W.WP_OPT_STAGE_TIMING, 1)
    for order in ("first", "count"):
        gv.count_words_tensor(t[:n], order=order, index=True, copy=False)
        s = gv.stats()
        stages[order] = {"ms_normalize": round(s["ms_normalize"], 3), "ms_words": round(s["ms_decode"], 3), "ms_rounds": round(s["ms_sa"], 3),
                         "ms_table": round(s["ms_walk"], 3), "ms_total": round(s["ms_total"], 3),
                         "ms_radix_scatter": round(s["ms_radix_scatter"], 3), "radix_passes": s["radix_passes"],
                         "radix_pass_bytes": s["radix_pass_bytes"],
                         "radix_scatter_share": round(s["ms_radix_scatter"] / s["ms_total"], 3),
                         "radix_bytes_per_input_byte": round(s["radix_pass_bytes"] / n, 2)}
    gv.set_option(W.WP_OPT_STAGE_TIMING, 0)
    out = {"config": 2, "mb": args.mb, "n_bytes": n, "reps": args.reps, "count_stats": stats,
           "ms_median": {k: round(v, 3) for k, v in med.items()},
           "ms_min": {k: round(min(v), 3) for k, v in times.items()},
           "ms_max": {k: round(max(v), 3) for k, v in times.items()},
           "stages": stages,
           "host_ms": {"split": round(ms_split, 1), "counter": round(ms_counter, 1)},
           "count_first_over_encode": round(med["count_first"] / med["encode_tensor"], 3),
           "host_over_count_first": round((ms_split + ms_counter) / med["count_first"], 1)}
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
