"""Cost of wp_detokenize_device on the ids of the config-2 text (100 MB of English): the text is encoded once, then its
ids go back to text in two layouts, in one process, the calls alternated; medians of host wall time around calls that
end in a device synchronise:

  ragged_one_row   the flat ids as one ragged row (row_splits [0, n]), cleanup on, no terminator
  padded_128       the same ids as [n / 128, 128] padded rows, full lengths, terminator '\\n'
  copy_same_bytes  the yardstick: one device-to-device hipMemcpyAsync (torch's copy_ between contiguous uint8 tensors)
                   that moves the algorithmic bytes of the ragged call, half read and half written, and one synchronise

Algorithmic bytes of a detokenize call: 4 B per cell read twice (count and write pass), one 8-byte record gather per
cell and pass, and the text written once.  The host baseline decodes a sample of the padded rows with tokenizers'
decode_batch where that package is importable and the vocabulary has no duplicate lines, else with the Python model
of tests/detok_model.py; `host_baseline` says which.

One JSON line, appended to --out (default profiles/detok_probe.jsonl).

    python profiles/detok_probe.py [--mb 100] [--reps 9] [--sample-rows 4000] [--out FILE]
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


def host_baseline(gv, vocab, rows):
    """(name, seconds, bytes) of decoding `rows` (a list of id lists) on the host"""
    try:
        from tokenizers import Tokenizer, decoders, models
        if len(set(vocab)) != len(vocab):
            raise ValueError("duplicate vocabulary lines")
        tok = Tokenizer(models.WordPiece(vocab={t: i for i, t in enumerate(vocab)}, unk_token="[UNK]"))
        tok.decoder = decoders.WordPiece(prefix="##", cleanup=True)
        t0 = time.perf_counter()
        out = tok.decode_batch(rows, skip_special_tokens=False)
        dt = time.perf_counter() - t0
        return "tokenizers.decode_batch", dt, sum(len(s.encode("utf-8")) for s in out)
    except Exception as e:  # noqa: BLE001  (not importable, or a vocabulary the package does not take)
        import detok_model as M
        m = M.Model.from_vocab(gv)
        t0 = time.perf_counter()
        text, _, _ = m.detokenize(rows, clean=True)
        dt = time.perf_counter() - t0
        return "python model (tests/detok_model.py); tokenizers: %s" % type(e).__name__, dt, len(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=float, default=100.0)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--sample-rows", type=int, default=4000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "detok_probe.jsonl"))
    args = ap.parse_args()
    text, vocab = synth.parallel_corpus("english", int(args.mb * 1e6), 2, 29000, 0)
    vocab = list(vocab)
    n = len(text)
    t = torch.zeros((n + 19) // 16 * 16, dtype=torch.uint8, device="cuda:0")
    t[:n] = torch.frombuffer(bytearray(text), dtype=torch.uint8).to("cuda:0")
    torch.cuda.synchronize()
    gv = W.Vocab(vocab, device=0)
    ids = gv.encode_tensor(t[:n])  # (a copy: the library's buffers are its own again)
    n_ids = ids.numel()
    L = 128
    n_rows = n_ids // L
    batch = ids[:n_rows * L].reshape(n_rows, L).contiguous()
    splits = torch.tensor([0, n_ids], dtype=torch.int64, device="cuda:0")
    stats = {}

    def ragged():
        gv.detokenize_tensor(ids, row_splits=splits, copy=False)
        stats["ragged_one_row"] = gv.detok_stats()

    def padded():
        gv.detokenize_tensor(batch, terminator="\n", copy=False)
        stats["padded_128"] = gv.detok_stats()

    ragged()
    padded()
    moved = {k: 2 * 4 * s["n_cells"] + 2 * 8 * s["n_cells"] + s["n_bytes"] for k, s in stats.items()}
    half = moved["ragged_one_row"] // 2
    src = torch.empty(half, dtype=torch.uint8, device="cuda:0")
    dst = torch.empty(half, dtype=torch.uint8, device="cuda:0")

    def copy_same_bytes():
        dst.copy_(src)
        torch.cuda.synchronize()

    moved["copy_same_bytes"] = 2 * half
    calls = {"ragged_one_row": ragged, "padded_128": padded, "copy_same_bytes": copy_same_bytes}
    times = {k: [] for k in calls}
    for f in calls.values():  # warm-up (buffer growth, code objects, the piece table)
        f()
        f()
    for _ in range(args.reps):
        for k, f in calls.items():
            t0 = time.perf_counter()
            f()
            times[k].append((time.perf_counter() - t0) * 1e3)
    med = {k: statistics.median(v) for k, v in times.items()}
    sample = batch[:args.sample_rows].cpu().tolist()
    name, dt, nbytes = host_baseline(gv, vocab, sample)
    out = {"config": 2, "mb": args.mb, "n_bytes_text": n, "n_ids": n_ids, "rows_128": n_rows, "reps": args.reps,
           "detok_stats": stats,
           "ms_median": {k: round(v, 3) for k, v in med.items()},
           "ms_min": {k: round(min(v), 3) for k, v in times.items()},
           "ms_max": {k: round(max(v), 3) for k, v in times.items()},
           "bytes_moved": moved,
           "gb_per_s": {k: round(moved[k] / med[k] / 1e6, 1) for k in moved},
           "ragged_over_copy": round(med["ragged_one_row"] / med["copy_same_bytes"], 3),
           "host_baseline": name, "host_sample_rows": len(sample), "host_ms": round(dt * 1e3, 3),
           "host_mb_per_s": round(nbytes / dt / 1e6, 2),
           "device_mb_per_s_text": round(stats["padded_128"]["n_bytes"] / med["padded_128"] / 1e3, 1)}
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
