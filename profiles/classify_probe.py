"""Cost of the classifier on the config-2 text (100 MB of English) resident in HBM, as documents of 20 lines and as its
lines, with two synthetic models: the shape of lid.176 (dim 16, 2 M buckets, minn 2, maxn 4, 176 labels) and that of a
quality classifier (dim 256, word_ngrams 2, 2 labels, 2 M buckets), their words the first --words whole words of the
vocabulary, their weights standard normal.  wp_classify_rows_device plain and with the compact form, beside
quality_rows_tensor and scrub_rows_tensor of the same bytes; in one process, the calls alternated, each between two device
events after two warm-up calls; medians with the spread.  The stages come from one more call per form under
WP_OPT_STAGE_TIMING (ms_decode: intake and tokens, ms_sa: feature list, ms_scan: row gathers, ms_walk: output stage and
compact form).  The host baseline is tests/classify_model.py over the first documents, scaled by bytes and marked as
such; the same documents are held against it before anything is timed.  One JSON line, appended to --out (default
profiles/classify_probe.jsonl).

    python profiles/classify_probe.py [--mb 100] [--reps 7] [--lines 20] [--words 20000] [--sample 40] [--out FILE]
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

import classify_model as M  # noqa: E402
import wordpiece_amd as W  # noqa: E402
from wordpiece_amd import classify as K  # noqa: E402
from wordpiece_amd import scrub as S  # noqa: E402
from wordpiece_amd import synth  # noqa: E402

SHAPES = {"lid": dict(dim=16, n_labels=176, minn=2, maxn=4, word_ngrams=1, bucket=2000000),
          "quality": dict(dim=256, n_labels=2, minn=0, maxn=0, word_ngrams=2, bucket=2000000)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=float, default=100.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--lines", type=int, default=20)
    ap.add_argument("--words", type=int, default=20000)
    ap.add_argument("--sample", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "classify_probe.jsonl"))
    args = ap.parse_args()
    text, vocab = synth.parallel_corpus("english", int(args.mb * 1e6), 2, 29000, 0)
    text, line_off = W.line_rows(text)
    offs = {"docs": np.ascontiguousarray(np.concatenate((line_off[:-1:args.lines], line_off[-1:]))), "lines": np.ascontiguousarray(line_off)}
    n = int(text.size)
    words = [W._bytes(w) for w in vocab if not W._bytes(w).startswith((b"##", b"["))][:args.words]
    t = torch.zeros((n + 19) // 16 * 16, dtype=torch.uint8, device="cuda:0")
    t[:n] = torch.from_numpy(text).to("cuda:0")
    d_offs = {k: torch.from_numpy(o).to("cuda:0") for k, o in offs.items()}
    torch.cuda.synchronize()
    gv = W.Vocab(vocab, device=0)
    q_rules = W.quality_rules("gopher")
    stop = [w.encode() for w in q_rules.pop("stop_words")]
    q_rules = {k: v for k, v in q_rules.items() if not k.startswith("max_dup")}
    rng = np.random.default_rng(30)
    host, sample_bytes = {}, int(offs["docs"][min(args.sample, offs["docs"].size - 1)])
    for slot, (name, shape) in enumerate(SHAPES.items()):  # the models, and the first documents against the reference
        inp = rng.standard_normal((len(words) + shape["bucket"], shape["dim"]), dtype=np.float32)
        outp = rng.standard_normal((shape["n_labels"], shape["dim"]), dtype=np.float32)
        how = {k: shape[k] for k in ("minn", "maxn", "word_ngrams", "bucket")}
        K.classify_load(gv, words, inp, outp, slot=slot, **how)
        head = min(args.sample, offs["docs"].size - 1)
        got = K.classify_rows_tensor(gv, t[:sample_bytes], d_offs["docs"][:head + 1].clone(), slot=slot, logits=True)
        ref = M.Model(words, inp, outp, **how)
        t0 = time.perf_counter()
        exp = [ref.score(text[offs["docs"][r]:offs["docs"][r + 1]].tobytes()) for r in range(head)]
        host[name] = (time.perf_counter() - t0) * 1e3
        assert got["n_features"].cpu().tolist() == [p["F"] for p in exp], "%s: n_features differs from the model's" % name
        assert np.allclose(got["logits"].cpu().numpy(), np.array([p["logits"] for p in exp]), rtol=1e-3, atol=1e-4), "%s: the logits differ from the model's" % name
        del inp, outp, ref
    calls = {}
    for batch, d_off in d_offs.items():
        for slot, name in enumerate(SHAPES):
            calls["cls_%s_%s" % (name, batch)] = lambda d_off=d_off, slot=slot: K.classify_rows_tensor(gv, t[:n], d_off, slot=slot, copy=False)
            calls["cls_%s_%s_compact" % (name, batch)] = lambda d_off=d_off, slot=slot: K.classify_rows_tensor(gv, t[:n], d_off, slot=slot, compact=True, copy=False)  # (every document kept)
        calls["quality_rows_%s" % batch] = lambda d_off=d_off: gv.quality_rows_tensor(t[:n], d_off, rules=q_rules, stop_words=stop, copy=False)
        calls["scrub_rows_%s" % batch] = lambda d_off=d_off: S.scrub_rows_tensor(gv, t[:n], d_off, copy=False)
    times, stats = {k: [] for k in calls}, {}
    for k, call in calls.items():  # warm-up (code objects, the buffers), and what the classifier counts
        call()
        call()
        if k.startswith("cls_"):
            stats[k] = K.classify_stats(gv, list(SHAPES).index(k.split("_")[1]))
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for _ in range(args.reps):
        for k, call in calls.items():
            torch.cuda.synchronize()
            ev[0].record()
            call()
            ev[1].record()
            torch.cuda.synchronize()
            times[k].append(ev[0].elapsed_time(ev[1]))
    stages = {}
    gv.set_option(W.WP_OPT_STAGE_TIMING, 1)
    for name, call in calls.items():
        call()
        s = gv.stats()
        stages[name] = {k: round(s[k], 3) for k in ("ms_decode", "ms_sa", "ms_scan", "ms_walk", "ms_total")}
    gv.set_option(W.WP_OPT_STAGE_TIMING, 0)
    out = {"config": 2, "mb": args.mb, "n_bytes": n, "n_rows": {k: int(o.size - 1) for k, o in offs.items()}, "lines_per_doc": args.lines, "n_words": len(words),
           "shapes": SHAPES, "reps": args.reps, "classify_stats": stats, "ms_median": {k: round(statistics.median(v), 3) for k, v in times.items()},
           "ms_min": {k: round(min(v), 3) for k, v in times.items()}, "ms_max": {k: round(max(v), 3) for k, v in times.items()}, "stages": stages,
           "host_model": {k: {"sample_bytes": sample_bytes, "sample_ms": round(ms, 1), "ms_scaled_by_bytes": round(ms * n / sample_bytes, 1)} for k, ms in host.items()}}
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
