"""Cost of the byte-level BPE encoder on the config-2 text (100 MB of English) resident in HBM, as documents of 20 lines and
as its lines.  The model is learnt by the trainer of tests/bpe_model.py from the first --sample-kb of the text, --merges
merges (the trainer rescans its word table per merge, so the default stays far below a production list; the pair table's
residency in L2 at 30 K merges and more is NOT measured by this).  wp_bpe_encode_rows_device beside encode_rows_tensor (the
WordPiece encode) and a device copy of the same bytes; in one process, the calls alternated, each between two device events
after two warm-up calls; medians with the spread.  The stages come from one more call per form under WP_OPT_STAGE_TIMING
(ms_decode: intake, class and start pass, piece list; ms_sa: merge pass; ms_scan: compaction).  The first documents are held
against the model before anything is timed.  Where `tokenizers` can be imported, its host time over the same sample is given,
scaled by bytes and marked as such.  One JSON line, appended to --out (default profiles/bpe_probe.jsonl).

    python profiles/bpe_probe.py [--mb 100] [--reps 7] [--lines 20] [--merges 2000] [--sample-kb 150] [--out FILE]
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

import bpe_model as M  # noqa: E402
import wordpiece_amd as W  # noqa: E402
from wordpiece_amd import bpe as B  # noqa: E402
from wordpiece_amd import synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=float, default=100.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--lines", type=int, default=20)
    ap.add_argument("--merges", type=int, default=2000)
    ap.add_argument("--sample-kb", type=int, default=150)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bpe_probe.jsonl"))
    args = ap.parse_args()
    text, vocab = synth.parallel_corpus("english", int(args.mb * 1e6), 2, 29000, 0)
    text, line_off = W.line_rows(text)
    offs = {"docs": np.ascontiguousarray(np.concatenate((line_off[:-1:args.lines], line_off[-1:]))), "lines": np.ascontiguousarray(line_off)}
    n = int(text.size)
    head = int(np.searchsorted(offs["docs"], args.sample_kb * 1000))
    sample = [text[offs["docs"][r]:offs["docs"][r + 1]].tobytes() for r in range(head)]
    sample_bytes = int(offs["docs"][head])
    t0 = time.perf_counter()
    model = M.train(sample, args.merges, seed=31)
    train_s = time.perf_counter() - t0
    tokens, pairs = model.vocab()
    t = torch.zeros((n + 19) // 16 * 16, dtype=torch.uint8, device="cuda:0")
    t[:n] = torch.from_numpy(text).to("cuda:0")
    d_offs = {k: torch.from_numpy(o).to("cuda:0") for k, o in offs.items()}
    torch.cuda.synchronize()
    gv = W.Vocab(vocab, device=0)
    B.bpe_load(gv, tokens, pairs)
    check = min(head, 40)  # the first documents against the model
    got = B.bpe_encode_rows_tensor(gv, t[:int(offs["docs"][check])], d_offs["docs"][:check + 1].clone())
    exp = model.encode(sample[:check])
    assert got["ids"].cpu().tolist() == exp["ids"].tolist() and got["row_splits"].cpu().tolist() == exp["row_splits"].tolist(), "the ids differ from the model's"
    calls = {}
    for batch, d_off in d_offs.items():
        calls["bpe_%s" % batch] = lambda d_off=d_off: B.bpe_encode_rows_tensor(gv, t[:n], d_off, copy=False)
        calls["wordpiece_%s" % batch] = lambda d_off=d_off: gv.encode_rows_tensor(t[:n], d_off)
    calls["device_copy"] = lambda: t.clone()
    times, stats = {k: [] for k in calls}, {}
    for k, call in calls.items():  # warm-up (code objects, the buffers), and what the encoder counts
        call()
        call()
        if k.startswith("bpe_"):
            stats[k] = B.bpe_stats(gv)
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
        if name != "device_copy":
            call()
            s = gv.stats()
            stages[name] = {k: round(s[k], 3) for k in ("ms_decode", "ms_sa", "ms_scan", "ms_walk", "ms_total")}
    gv.set_option(W.WP_OPT_STAGE_TIMING, 0)
    host = None
    try:
        import tokenizers as tk
        hf = tk.Tokenizer(tk.models.BPE(vocab=tokens, merges=pairs))
        hf.pre_tokenizer = tk.pre_tokenizers.ByteLevel(add_prefix_space=False, use_regex=True)
        docs = [d.decode("utf-8", "replace") for d in sample]
        t0 = time.perf_counter()
        hf.encode_batch(docs)
        ms = (time.perf_counter() - t0) * 1e3
        host = {"sample_bytes": sample_bytes, "sample_ms": round(ms, 1), "ms_scaled_by_bytes": round(ms * n / sample_bytes, 1), "version": tk.__version__}
    except ImportError:
        pass  # (not measured)
    med = {k: round(statistics.median(v), 3) for k, v in times.items()}
    out = {"config": 2, "mb": args.mb, "n_bytes": n, "n_rows": {k: int(o.size - 1) for k, o in offs.items()}, "lines_per_doc": args.lines, "n_merges": len(model.merges),
           "sample_bytes": sample_bytes, "train_s": round(train_s, 1), "reps": args.reps, "bpe_stats": stats, "ms_median": med,
           "ms_min": {k: round(min(v), 3) for k, v in times.items()}, "ms_max": {k: round(max(v), 3) for k, v in times.items()}, "stages": stages,
           "bpe_over_wordpiece": {b: round(med["bpe_%s" % b] / med["wordpiece_%s" % b], 2) for b in offs}, "tokenizers_host": host}
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
