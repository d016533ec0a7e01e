"""Cost of the vocabulary learner on the word table of the config-2 text (100 MB of English) resident in HBM:
wp_count_words_device (count order) and then wp_learn_vocab_device on its table, vocab_size 30,000 and the defaults
otherwise; in one process, the calls alternated; medians of host wall time around calls that end in a device synchronise.
The stages come from one more learn call under WP_OPT_STAGE_TIMING (HIP events inside the library, handed out through
wp_stats as the header's section "vocabulary learner" says).  Beside them:

  count            the count call that makes the table
  encode_tensor    the handle's plain encode of the same text
  model            tests/learn_model.py on the host, on the first --prefix words of the count-ordered table (the whole
                   table takes the model minutes per search step), against the device on the same prefix; the two lists
                   are compared before either time is reported

Commands per search step: per iteration one clear of the sums, one sum launch, one clear of the kept counter and one
level launch per token length that has tokens (the lengths up to the longest remaining word), and a split launch in every
iteration but the first.  One JSON line, appended to --out (default profiles/learn_probe.jsonl).

    python profiles/learn_probe.py [--mb 100] [--reps 7] [--vocab-size 30000] [--prefix 10000] [--out FILE]
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
import torch  # noqa: E402  (before the library: torch's HIP runtime serves the process)

import wordpiece_amd as W  # noqa: E402
from wordpiece_amd import synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=float, default=100.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--vocab-size", type=int, default=30000)
    ap.add_argument("--prefix", type=int, default=10000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "learn_probe.jsonl"))
    args = ap.parse_args()
    text, vocab = synth.parallel_corpus("english", int(args.mb * 1e6), 2, 29000, 0)
    n = len(text)
    t = torch.zeros((n + 19) // 16 * 16, dtype=torch.uint8, device="cuda:0")
    t[:n] = torch.frombuffer(bytearray(text), dtype=torch.uint8).to("cuda:0")
    torch.cuda.synchronize()
    gv = W.Vocab(vocab, device=0)
    table = gv.count_words_tensor(t[:n], order="count")  # (copies: the table outlives the count calls below)
    n_words = table["counts"].numel()

    def learn(tab=table, size=args.vocab_size):
        return gv.learn_vocab_tensor(tab["words"], tab["word_off"], tab["counts"], size, copy=False)
    learn()
    stats = gv.learn_stats()
    print("table of %d words learned: %s" % (n_words, stats), file=sys.stderr, flush=True)
    off = table["word_off"].tolist()
    pool = table["words"].cpu().numpy().tobytes()
    longest = max(len(pool[a:b].decode("utf8")) for a, b in zip(off, off[1:]))
    levels = min(50, longest)
    commands = 4 * (levels + 3) + 3

    # the model on a prefix of the table, against the device on the same prefix
    import learn_model as M
    k = min(args.prefix, n_words)
    words = [pool[a:b] for a, b in zip(off[:k], off[1:k + 1])]
    counts = table["counts"][:k].tolist()
    size_k = max(1000, args.vocab_size * k // n_words)
    t0 = time.perf_counter()
    exp = M.learn(words, counts, size_k)
    ms_model = (time.perf_counter() - t0) * 1e3
    print("model on %d words: %.0f ms" % (k, ms_model), file=sys.stderr, flush=True)
    sub = {"words": table["words"][:off[k]].contiguous(), "word_off": table["word_off"][:k + 1].contiguous(),
           "counts": table["counts"][:k].contiguous()}
    got = learn(sub, size_k)
    assert bytes(got["tokens"].cpu().numpy()).decode("utf8").split("\n")[:-1] == exp["tokens"], "the list differs from the model's"
    assert got["scores"].tolist() == exp["scores"] and got["thresh"] == exp["thresh"]
    prefix_stats = gv.learn_stats()

    calls = {
        "count": lambda: gv.count_words_tensor(t[:n], order="count", copy=False),
        "learn": learn,
        "learn_prefix": lambda: learn(sub, size_k),
        "encode_tensor": lambda: gv.encode_tensor(t[:n], copy=False),
    }
    times = {name: [] for name in calls}
    for f in calls.values():  # warm-up (code objects, the buffers)
        f()
    for _ in range(args.reps):
        for name, f in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            times[name].append((time.perf_counter() - t0) * 1e3)
    med = {name: statistics.median(v) for name, v in times.items()}
    gv.set_option(W.WP_OPT_STAGE_TIMING, 1)
    learn()
    s = gv.stats()
    stages = {"ms_table": round(s["ms_decode"], 3), "ms_grouping": round(s["ms_sa"], 3), "ms_search": round(s["ms_scan"], 3),
              "ms_list": round(s["ms_walk"], 3), "ms_total": round(s["ms_total"], 3),
              "ms_per_search_step": round(s["ms_scan"] / max(1, stats["n_steps"]), 3),
              "search_share": round(s["ms_scan"] / s["ms_total"], 3)}
    gv.set_option(W.WP_OPT_STAGE_TIMING, 0)
    out = {"config": 2, "mb": args.mb, "n_bytes": n, "reps": args.reps, "vocab_size": args.vocab_size, "n_table_words": n_words,
           "learn_stats": stats, "longest_word": longest, "commands_per_search_step": commands,
           "ms_median": {name: round(v, 3) for name, v in med.items()},
           "ms_min": {name: round(min(v), 3) for name, v in times.items()},
           "ms_max": {name: round(max(v), 3) for name, v in times.items()},
           "stages": stages,
           "prefix": {"words": k, "vocab_size": size_k, "learn_stats": prefix_stats, "model_ms": round(ms_model, 1),
                      "model_over_learn": round(ms_model / med["learn_prefix"], 1)},
           "learn_over_count": round(med["learn"] / med["count"], 2), "learn_over_encode": round(med["learn"] / med["encode_tensor"], 2)}
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
