#!/usr/bin/env python3
"""Measurements of WP_OPT_NORMALIZE on the config-2 shard (100 MB English-shaped text, upper case at word starts).

    python profiles/normalize_probe.py encode [--mb 100] [--steps 7] [--out FILE.jsonl]
        device-resident encodes with WP_OPT_STAGE_TIMING: option on (flags 7) on the mixed-case text, option off on the
        host-pre-normalised text (what a caller had to do before), alternated; one JSON line per step and a summary
        line with the medians, the spread, and the bytes of one radix scatter launch of the same encode.
    python profiles/normalize_probe.py trace [--mb 100]
        three option-on encodes and nothing else: the program to run under `rocprofv3 --kernel-trace --stats` (a run of
        its own) for the device time of norm_count_kernel / norm_write_kernel beside the radix scatter kernel.
    python profiles/normalize_probe.py host [--mb 100] [--out FILE.jsonl]
        the host alternative the option replaces: text.decode().lower() + NFD + drop Mn in Python, one thread.
A digest of the MI355X runs is kept beside this file as normalize_probe.jsonl (profiles/README.md says what it holds).
"""
import argparse
import json
import os
import statistics
import sys
import time
import unicodedata

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def shard(mb, seed=2, accents=0.0):
    """the bench's config-2 text with a third of its word starts in upper case -> (mixed-case bytes, vocab);
    accents: the share of words whose second letter, a vowel, gets an acute (a 2-byte code point)"""
    from wordpiece_amd import synth
    text, vocab = synth.english_corpus(int(mb * 1e6), seed=seed)
    tb = np.frombuffer(text, dtype=np.uint8).copy()
    rng = np.random.default_rng(seed)
    start = np.nonzero((tb >= 0x61) & (tb <= 0x7A) & (np.concatenate([[0x20], tb[:-1]]) == 0x20))[0]
    tb[start[rng.random(len(start)) < 0.33]] -= 0x20
    if accents > 0.0:
        at = start[rng.random(len(start)) < accents] + 1
        at = at[at < len(tb)]
        at = at[np.isin(tb[at], np.frombuffer(b"aeiou", dtype=np.uint8))]
        second = {0x61: 0xA1, 0x65: 0xA9, 0x69: 0xAD, 0x6F: 0xB3, 0x75: 0xBA}  # C3 xx: a e i o u with an acute
        ins = np.array([second[int(x)] for x in tb[at]], dtype=np.uint8)
        tb[at] = 0xC3
        tb = np.insert(tb, at + 1, ins)
    return tb.tobytes(), vocab


def host_normalize(text):
    s = text.decode("utf8").lower()
    return "".join(c for c in unicodedata.normalize("NFD", s) if unicodedata.category(c) != "Mn").encode("utf8")


def emit(out, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("encode", "trace", "host"))
    ap.add_argument("--mb", type=float, default=100.0)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--accents", type=float, default=0.0, help="share of the words that get an accented letter (default: none)")
    args = ap.parse_args()
    text, vocab = shard(args.mb, accents=args.accents)
    if args.mode == "host":
        t0 = time.perf_counter()
        norm = host_normalize(text)
        emit(args.out, {"what": "host str.lower() + NFD + drop Mn, one thread", "mb": args.mb, "accents": args.accents, "seconds": time.perf_counter() - t0,
                        "norm_bytes": len(norm), "python": sys.version.split()[0], "unicode": unicodedata.unidata_version})
        return
    import torch
    import wordpiece_amd as W
    on = W.Vocab(vocab, device=0, normalize=W.WP_NORM_BERT_UNCASED)
    t_mixed = torch.frombuffer(bytearray(text), dtype=torch.uint8).to("cuda:0")
    if args.mode == "trace":
        for _ in range(3):
            on.encode_tensor(t_mixed, copy=False)
        st = on.stats()
        print(json.dumps({"what": "trace run", "n_ids": st["n_ids"], "norm_bytes": st["norm_bytes"],
                          "radix_passes": st["radix_passes"], "radix_pass_bytes": st["radix_pass_bytes"]}))
        return
    off = W.Vocab(vocab, device=0)
    norm = host_normalize(text)
    t_norm = torch.frombuffer(bytearray(norm), dtype=torch.uint8).to("cuda:0")
    for v in (on, off):
        v.set_option(W.WP_OPT_STAGE_TIMING, 1)
    ids_on = on.encode_tensor(t_mixed).cpu().numpy()
    ids_off = off.encode_tensor(t_norm).cpu().numpy()
    assert np.array_equal(ids_on, ids_off), "option on differs from the encode of the host-normalised text"
    assert on.normalize_tensor(t_mixed).cpu().numpy().tobytes() == norm, "device and host normalisation differ"
    rows = {"on": [], "off": [], "normalize": []}
    for step in range(args.warmup + args.steps):
        on.encode_tensor(t_mixed, copy=False)
        s_on = on.stats()
        off.encode_tensor(t_norm, copy=False)
        s_off = off.stats()
        if step < args.warmup:
            continue
        rows["on"].append(s_on["ms_total"])
        rows["off"].append(s_off["ms_total"])
        rows["normalize"].append(s_on["ms_normalize"])
        emit(args.out, {"what": "step", "ms_total_on": s_on["ms_total"], "ms_normalize": s_on["ms_normalize"],
                        "ms_total_off_prenormalised": s_off["ms_total"], "ms_radix_scatter_on": s_on["ms_radix_scatter"],
                        "radix_passes": s_on["radix_passes"]})
    med = {k: statistics.median(v) for k, v in rows.items()}
    st = on.stats()
    scatter_launch_bytes = st["radix_pass_bytes"] / max(st["radix_passes"], 1)
    emit(args.out, {"what": "summary", "mb": args.mb, "accents": args.accents, "steps": args.steps, "n_bytes": st["n_bytes"], "norm_bytes": st["norm_bytes"],
                    "ms_total_on_median": med["on"], "ms_total_on_min_max": [min(rows["on"]), max(rows["on"])],
                    "ms_total_off_median": med["off"], "ms_total_off_min_max": [min(rows["off"]), max(rows["off"])],
                    "ms_normalize_median": med["normalize"], "ms_normalize_min_max": [min(rows["normalize"]), max(rows["normalize"])],
                    "end_to_end_cost_ms": med["on"] - med["off"],
                    "prepass_algorithmic_bytes": 2 * st["n_bytes"] + st["norm_bytes"],
                    "prepass_GBps_over_event_time": (2 * st["n_bytes"] + st["norm_bytes"]) / med["normalize"] / 1e6,
                    "one_scatter_launch_bytes": scatter_launch_bytes,
                    "one_scatter_launch_ms_from_events": st["ms_radix_scatter"] / max(st["radix_passes"], 1)})


if __name__ == "__main__":
    main()
