"""Cost of the seen-rows call on the config-2 text (100 MB of English) resident in HBM, its rows the lines of the text, over
the text bytes and over the ids of encode_rows_tensor; in one process, medians of host wall time around calls that end in a
device synchronise, each beside dedup_rows_tensor of the same batch in the same run:

  first        the batch on an empty set (every key new; the set is cleared and given its room in front of the timed call)
  again        the same batch a second time (every key seen; nothing is inserted)
  behind_10 / behind_100   "again", once the set also holds 10 / 100 batches' worth of other keys (loaded through
               seen_add_keys_tensor), so that the table is out of the caches
  growth       a call that has to double a table of one batch's keys (the rehash) beside one on a table with room
  export       seen_keys_tensor of one batch's keys, and behind_100's

The stages of "first" and "again" come from one more call each under WP_OPT_STAGE_TIMING.  The states of the device are
compared with a dict over the lines on the host before anything is timed.  One JSON line, appended to --out.

    python profiles/seen_probe.py [--mb 100] [--reps 7] [--out FILE]
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
from wordpiece_amd import seen as S, synth  # noqa: E402


def timed(f, reps, before=None):
    ms = []
    for _ in range(reps + 2):  # (two warm-up rounds: code objects, the buffers)
        if before:
            before()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        ms.append((time.perf_counter() - t0) * 1e3)
    ms = ms[2:]
    return {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=float, default=100.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seen_probe.jsonl"))
    args = ap.parse_args()
    text, vocab = synth.parallel_corpus("english", int(args.mb * 1e6), 2, 29000, 0)
    text, off = W.line_rows(text)
    n, n_rows = int(text.size), int(off.size - 1)
    first_of = {}
    lines = text.tobytes().split(b"\n")[:-1]
    for i, line in enumerate(lines):
        first_of.setdefault(line, i)
    t = torch.zeros((n + 19) // 16 * 16, dtype=torch.uint8, device="cuda:0")
    t[:n] = torch.from_numpy(text).to("cuda:0")
    d_off = torch.from_numpy(off).to("cuda:0")
    gv = W.Vocab(vocab, device=0)
    ids, splits = gv.encode_rows_tensor(t[:n], d_off)
    # the states and firsts, once, against the host's
    got = S.seen_rows_tensor(gv, t[:n], d_off)
    assert got["first"].tolist() == [first_of[line] for line in lines], "first differs from the host's"
    assert got["state"].tolist() == [0 if first_of[line] == i else 1 for i, line in enumerate(lines)], "state differs from the host's"
    n_distinct = S.seen_stats(gv)["n_keys"]
    assert n_distinct == len(first_of) and int((S.seen_rows_tensor(gv, t[:n], d_off)["state"] != 2).sum()) == 0
    out = {"config": 2, "mb": args.mb, "n_bytes": n, "n_rows": n_rows, "n_ids": int(ids.numel()), "n_distinct": n_distinct, "reps": args.reps}
    gen = torch.Generator(device="cuda:0").manual_seed(1)
    other = lambda k: torch.randint(-2 ** 62, 2 ** 62, (k * n_distinct,), dtype=torch.int64, device="cuda:0", generator=gen)  # noqa: E731
    for name, data, rows in (("text", t[:n], d_off), ("ids", ids, splits)):
        call = lambda insert=True: S.seen_rows_tensor(gv, data, rows, insert=insert, copy=False)  # noqa: E731
        fresh = lambda room: (S.seen_clear(gv), S.seen_reserve(gv, room))  # noqa: E731
        r = {"dedup": timed(lambda: gv.dedup_rows_tensor(data, rows, copy=False), args.reps)}
        r["first"] = timed(call, args.reps, lambda: fresh(2 * n_rows))
        r["again"] = timed(call, args.reps)
        r["probes_again"] = S.seen_stats(gv)["n_probes"]
        gv.set_option(W.WP_OPT_STAGE_TIMING, 1)
        for stage, before in (("first", lambda: fresh(2 * n_rows)), ("again", None)):
            if before:
                before()
            call()
            s = gv.stats()
            r["stages_" + stage] = {k: round(s[k], 3) for k in ("ms_decode", "ms_sa", "ms_walk", "ms_total")}
        gv.set_option(W.WP_OPT_STAGE_TIMING, 0)
        r["export_1"] = timed(lambda: S.seen_keys_tensor(gv), args.reps)
        held = 0
        for k in (10, 100):
            while held < k:  # (ten batches' worth a call: each within the 2^31 keys of a call)
                S.seen_add_keys_tensor(gv, other(10))
                held += 10
            st = S.seen_stats(gv)
            r["behind_%d" % k] = dict(timed(call, args.reps), n_keys=st["n_keys"], capacity=st["capacity"], probes=S.seen_stats(gv)["n_probes"])
        r["export_100"] = timed(lambda: S.seen_keys_tensor(gv), args.reps)
        # a growth: a table that one batch fills to the brim has to double for the next call; beside it the same call with room
        half = other(1)

        def brim():
            S.seen_clear(gv)
            S.seen_add_keys_tensor(gv, half[:n_distinct // 2])
        r["call_with_growth"] = timed(call, args.reps, brim)
        r["n_grown_in_it"] = S.seen_stats(gv)["n_grown"]
        r["call_with_room"] = timed(call, args.reps, lambda: (brim(), S.seen_reserve(gv, 4 * n_rows)))
        r["all_seen_over_dedup"] = round(r["again"]["median"] / r["dedup"]["median"], 3)
        out[name] = r
        S.seen_clear(gv)
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
