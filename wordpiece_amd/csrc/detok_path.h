// detok_path.h — detokenize on a context (include/wordpiece_amd.h, section "detokenize"; kernels: detok.h): the
// argument rules, the table of pieces, and the three passes over device buffers.
#pragma once
#include "context.h"
#include "detok.h"
#include "rows.h"  // check_splits_kernel

namespace wp {

// every argument rule that needs neither the ids nor a device; n_cells of a padded call, -1 of a ragged one
static DetokGeom check_detok_spec(const wp_vocab *v, const wp_detok_spec *spec, size_t n_rows) {
  if (!spec) throw std::invalid_argument("detokenize: spec is NULL");
  if (spec->cleanup != 0 && spec->cleanup != 1) throw std::invalid_argument("detokenize: cleanup must be 0 or 1");
  if (spec->terminator < -1 || spec->terminator > 255) throw std::invalid_argument("detokenize: terminator must lie in [-1, 255]");
  if (spec->n_skip < 0 || spec->n_skip > 8) throw std::invalid_argument("detokenize: n_skip must lie in [0, 8]");
  if (spec->max_len < 0) throw std::invalid_argument("detokenize: max_len must be at least 0");
  if (n_rows > static_cast<size_t>(INT32_MAX)) throw std::length_error("detokenize: more rows than INT32_MAX");
  DetokGeom g{};
  g.n_rows = static_cast<long long>(n_rows);
  g.max_len = spec->max_len;
  g.term = spec->terminator;
  g.n_skip = spec->n_skip;
  for (int k = 0; k < 8; k++) g.skip_ids[k] = k < spec->n_skip ? spec->skip_ids[k] : -1;
  g.vocab_size = static_cast<long long>(v->hv.tokens.size());
  g.n_cells = -1;
  if (spec->max_len > 0) {  // (n_rows <= 2^31 - 1 and max_len <= 2^31 - 1: the product fits 64 bits)
    g.n_cells = static_cast<long long>(n_rows) * spec->max_len;
    if (g.n_cells > INT32_MAX) throw std::length_error("detokenize: more cells than INT32_MAX");
  }
  return g;
}

static wp_detok_stats &begin_detok_stats(wp_vocab *v, size_t n_rows) {
  v->stats.detok_call = 1;
  v->stats.detok = wp_detok_stats{};
  v->stats.detok.n_rows = static_cast<int64_t>(n_rows);
  return v->stats.detok;
}

// the pieces of every id, both forms, both cleanup values: records [cleanup][form][id] and the pool of their bytes
static void ensure_detok_table(const wp_vocab *v, Context *c) {
  if (c->d_detok_rec) return;
  const size_t V = v->hv.tokens.size();
  std::vector<DetokRec> rec(4 * V);
  std::vector<uint8_t> pool;
  for (int cleanup = 0; cleanup < 2; cleanup++) {
    for (int form = 0; form < 2; form++) {
      for (size_t i = 0; i < V; i++) {
        const HostToken &t = v->hv.tokens[i];
        DetokRec &r = rec[(static_cast<size_t>(cleanup) * 2 + static_cast<size_t>(form)) * V + i];
        if (t.is_malformed) {
          r = DetokRec{kDetokNoPiece, 0};
          continue;
        }
        const std::string piece = detok_piece_bytes(t, form, cleanup);
        if (cleanup == 1 && piece == detok_piece_bytes(t, form, 0)) {  // the clean-up changes few pieces: the bytes are shared
          r = rec[static_cast<size_t>(form) * V + i];
          continue;
        }
        if (pool.size() + piece.size() >= static_cast<size_t>(kDetokNoPiece)) throw std::length_error("detokenize: the pieces of the vocabulary exceed 4 GB");
        r = DetokRec{static_cast<uint32_t>(pool.size()), static_cast<uint32_t>(piece.size())};
        pool.insert(pool.end(), piece.begin(), piece.end());
      }
    }
  }
  c->d_detok_rec = upload(rec, c->stream);
  c->d_detok_pool = upload(pool, c->stream);
  c->detok_pool_bytes = pool.size();
  WP_HIP(hipStreamSynchronize(c->stream));  // rec and pool are locals
}

// The three passes over device buffers on c's stream.  g.n_cells < 0: a ragged call whose row_splits have not been
// checked (the device entry point).  The result lies in c->detok_out until the handle's next call.
static void detok_on_device(wp_vocab *v, Context *c, const int32_t *d_ids, const long long *d_splits, const int32_t *d_lengths,
                            DetokGeom g, int cleanup, const void **d_text, const long long **d_text_off, size_t *n_bytes) {
  wp_detok_stats &ds = begin_detok_stats(v, static_cast<size_t>(g.n_rows));
  hipStream_t st = c->stream;
  const size_t n_rows = static_cast<size_t>(g.n_rows);
  if (g.n_cells < 0) {
    clear_scalars(c, kScalarDetokLast, kScalarDetokBad, st);
    hipLaunchKernelGGL(check_splits_kernel, dim3(std::min<unsigned>(cdiv(n_rows + 1, kBlock), 1024u)), dim3(kBlock), 0, st, d_splits, n_rows,
                       c->d_scalars + kScalarDetokBad, reinterpret_cast<long long *>(c->d_scalars + kScalarDetokLast));
    WP_LAUNCH_CHECK();
    queue_scalar_slots(c, kScalarDetokLast, kScalarDetokBad, st);
    WP_HIP(hipStreamSynchronize(st));
    if (c->h_scalars[kScalarDetokBad] != 0) throw std::invalid_argument("detokenize: row_splits must start at 0 and never descend");
    long long last;
    std::memcpy(&last, c->h_scalars + kScalarDetokLast, sizeof(last));
    if (last > INT32_MAX) throw std::length_error("detokenize: more cells than INT32_MAX");
    g.n_cells = last;
  }
  if (g.n_cells > 0 && !d_ids) throw std::invalid_argument("detokenize: ids is NULL");
  ensure_detok_table(v, c);
  g.pool_bytes = c->detok_pool_bytes;
  const size_t n_tiles = static_cast<size_t>(g.n_cells) / kDetokTile + 1;
  Arena aux(&c->detok_aux);
  DetokTile *d_tiles = nullptr;
  unsigned long long *d_tile_off = nullptr;
  uint32_t *d_tile_carry = nullptr;
  for (int pass = 0; pass < 2; pass++) {
    d_tiles = aux.take<DetokTile>(n_tiles);
    d_tile_off = aux.take<unsigned long long>(n_tiles);
    d_tile_carry = aux.take<uint32_t>(n_tiles);
    if (pass == 0) aux.commit();
  }
  const DetokRec *d_rec = c->d_detok_rec + static_cast<size_t>(cleanup) * 2 * static_cast<size_t>(g.vocab_size);
  static_assert(scalar_end(kScalarDetok) - kScalarDetok == 2 * kDetokCounters, "the slot kScalarDetok holds the totals of a detokenize call");
  unsigned long long *d_tot = reinterpret_cast<unsigned long long *>(c->d_scalars + kScalarDetok);
  const dim3 grid(static_cast<unsigned>(n_tiles)), block(kBlock);
  hipLaunchKernelGGL((detok_tile_kernel<false>), grid, block, 0, st, d_ids, d_splits, d_lengths, g, d_rec, c->d_detok_pool, d_tiles,
                     static_cast<const unsigned long long *>(nullptr), static_cast<const uint32_t *>(nullptr),
                     static_cast<uint8_t *>(nullptr), static_cast<long long *>(nullptr));
  hipLaunchKernelGGL(detok_spine_kernel, dim3(1), block, 0, st, d_tiles, n_tiles, d_tile_off, d_tile_carry, d_tot);
  WP_LAUNCH_CHECK();
  queue_scalar_slots(c, kScalarDetok, kScalarDetok, st);
  WP_HIP(hipStreamSynchronize(st));
  const unsigned long long *h_tot = reinterpret_cast<const unsigned long long *>(c->h_scalars + kScalarDetok);
  const unsigned long long total = h_tot[kDetokBytes] + (g.term >= 0 ? static_cast<unsigned long long>(n_rows) : 0ull);
  if (total >= (1ull << 32)) throw std::length_error("detokenize: the text has 2^32 bytes or more");
  g.n_bytes = total;
  Arena res(&c->detok_out);  // its own arena: the size of the text is known only behind the wait above
  long long *d_off = nullptr;
  uint8_t *d_txt = nullptr;
  for (int pass = 0; pass < 2; pass++) {
    d_off = res.take<long long>(n_rows + 1);
    d_txt = res.take<uint8_t>(static_cast<size_t>(total) + 4);  // + 4: detok_tile_kernel stores the text in whole 4-byte words
    if (pass == 0) res.commit();
  }
  hipLaunchKernelGGL((detok_tile_kernel<true>), grid, block, 0, st, d_ids, d_splits, d_lengths, g, d_rec, c->d_detok_pool,
                     static_cast<DetokTile *>(nullptr), d_tile_off, d_tile_carry, d_txt, d_off);
  WP_LAUNCH_CHECK();
  WP_HIP(hipStreamSynchronize(st));
  throw_if_oob(kSiteDetok, "detokenize", "gathers or stores outside their buffers skipped");
  ds.n_kept = static_cast<int64_t>(h_tot[kDetokKept]);
  ds.n_skipped = static_cast<int64_t>(h_tot[kDetokSkipped]);
  ds.n_dropped = static_cast<int64_t>(h_tot[kDetokDropped]);
  ds.n_cells = ds.n_kept + ds.n_skipped + ds.n_dropped;
  ds.n_bytes = static_cast<int64_t>(total);
  *d_text = total ? d_txt : nullptr;
  *d_text_off = d_off;
  *n_bytes = static_cast<size_t>(total);
}

}  // namespace wp
