"""Soak run on the GPU box (not collected by pytest): thousands of adversarial random cases through the
default path (text-only layout, pruned, depth capped), the reference layout, the multi-context entry point
and the fast path, each against the CPU oracle.  usage: python tests/soak_gpu.py [cases] [seed]"""
import os
import random
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: F401,E402
import oracle_lib as O  # noqa: E402
import wordpiece_amd as W  # noqa: E402
from round0_cases import make_case  # noqa: E402  (shared with tests/test_gpu_round0_edges.py)


def main():
    cases = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
    rng = random.Random(int(sys.argv[2]) if len(sys.argv) > 2 else 12345)
    done = bad = 0
    k = 0
    while done < cases:
        text, vocab = make_case(rng, k)
        k += 1
        try:
            ov = O.Vocab(vocab)
        except O.OracleError:
            continue
        exp = ov.encode(text, threads=8 if len(text) > 1_000_000 else 1)
        gv = W.Vocab(vocab)
        got = gv.encode(text)
        st = gv.stats()
        checks = [("default", got)]
        if done % 3 == 0:
            g2 = W.Vocab(vocab)
            g2.set_option(W.WP_OPT_VOCAB_IN_S, 1)
            checks.append(("vocab_in_s", g2.encode(text)))
        if done % 5 == 0:
            checks.append(("multi", gv.encode_multi(text, [0, 0])))
        for name, ids in checks:
            if not np.array_equal(ids, exp):
                bad += 1
                print("MISMATCH", name, "case", k - 1, "kind", (k - 1) % 8, repr(text[:120]), vocab[:12], st, flush=True)
        fexp = ov.fast_encode(text, threads=8 if len(text) > 1_000_000 else 1)
        if not np.array_equal(gv.fast_encode(text), fexp):
            bad += 1
            print("MISMATCH fast case", k - 1, repr(text[:120]), vocab[:12], flush=True)
        done += 1
        if done % 200 == 0:
            print("soak: %d cases, %d mismatches (last: kind %d, n=%d, rounds=%d, needed=%d)"
                  % (done, bad, (k - 1) % 8, st.get("n_total", 0), st.get("rounds", 0), st.get("needed_after_round0", 0)), flush=True)
    print("SOAK DONE: %d cases, %d mismatches" % (done, bad), flush=True)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
