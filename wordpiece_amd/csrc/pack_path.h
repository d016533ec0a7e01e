// pack_path.h — sequence packing on a context (include/wordpiece_amd.h, section "pack"; kernels: packing.h): the
// argument rules, the passes over device buffers, and the buffers of a host call's batch.
#pragma once
#include "context.h"
#include "packing.h"
#include "rows.h"  // check_splits_kernel

namespace wp {

// every argument rule that needs neither the rows nor a device
static PackGeom check_pack_spec(const wp_pack_spec *spec, size_t n_docs) {
  if (!spec) throw std::invalid_argument("pack: spec is NULL");
  if (spec->mode != WP_PACK_NEXT_FIT && spec->mode != WP_PACK_STREAM) throw std::invalid_argument("pack: unknown mode");
  if (spec->mode == WP_PACK_NEXT_FIT && spec->long_docs != WP_PACK_LONG_TRUNCATE && spec->long_docs != WP_PACK_LONG_SPLIT) {
    throw std::invalid_argument("pack: unknown long_docs");
  }
  if ((spec->want & ~7) != 0) throw std::invalid_argument("pack: want has bits outside 7");
  if (spec->max_len < 1) throw std::invalid_argument("pack: max_len must be at least 1");
  const int specials = (spec->bos_id >= 0 ? 1 : 0) + (spec->eos_id >= 0 ? 1 : 0);
  if (spec->max_len - specials < 1) throw std::invalid_argument("pack: max_len leaves no room for an id beside the specials");
  if (n_docs > static_cast<size_t>(INT32_MAX)) throw std::length_error("pack: more documents than INT32_MAX");
  PackGeom g{};
  g.max_len = spec->max_len;
  g.budget = spec->max_len - specials;
  g.stream = spec->mode == WP_PACK_STREAM;
  g.split = !g.stream && spec->long_docs == WP_PACK_LONG_SPLIT;
  g.bos_id = spec->bos_id;
  g.eos_id = spec->eos_id;
  g.pad_id = spec->pad_id;
  g.want = spec->want;
  return g;
}

static wp_pack_stats &begin_pack_stats(wp_vocab *v, size_t n_docs) {
  v->stats.pack_call = 1;
  v->stats.pack = wp_pack_stats{};
  v->stats.pack.n_docs = static_cast<int64_t>(n_docs);
  return v->stats.pack;
}

static void check_pack_totals(unsigned long long n_ids, unsigned long long n_cells) {
  if (n_ids > static_cast<unsigned long long>(INT32_MAX)) throw std::length_error("pack: more ids than INT32_MAX");
  if (n_cells > static_cast<unsigned long long>(INT32_MAX)) throw std::length_error("pack: more cells in the units than INT32_MAX");
}
static void check_pack_rows(unsigned long long n_out, int max_len) {
  if (n_out * static_cast<unsigned long long>(max_len) > static_cast<unsigned long long>(INT32_MAX)) {
    throw std::length_error("pack: n_out * max_len exceeds INT32_MAX");
  }
}

// The passes over device buffers on c's stream; the row_splits are checked here in a kernel.  place(n_out): the
// buffers of the batch once the number of rows is known (throws where there is no room); not called for n_out == 0.
// Returns n_out.  Nothing is written through the caller's pointers before every check has passed.
template <typename Place>
static size_t pack_on_device(wp_vocab *v, Context *c, const int32_t *d_ids, const long long *d_splits, size_t n_docs, PackGeom g,
                             Place &&place) {
  wp_pack_stats &ps = begin_pack_stats(v, n_docs);
  if (n_docs == 0) return 0;
  hipStream_t st = c->stream;
  const dim3 block(kBlock);
  Arena plan(&c->pack_plan);
  uint32_t *d_piece_base = nullptr, *d_cell_base = nullptr, *d_scan_tmp = nullptr;
  for (int pass = 0; pass < 2; pass++) {
    d_piece_base = plan.take<uint32_t>(n_docs);                        // pieces per document, scanned in place
    d_cell_base = plan.take<uint32_t>(n_docs);                         // cells per document, scanned in place
    d_scan_tmp = plan.take<uint32_t>(cdiv(n_docs, kScanTile) + 1);     // the scans' tile sums (device_exclusive_scan: + 1)
    if (pass == 0) plan.commit();
  }
  unsigned long long *d_tot = reinterpret_cast<unsigned long long *>(c->d_scalars + kScalarPack);
  const unsigned long long *h_tot = reinterpret_cast<const unsigned long long *>(c->h_scalars + kScalarPack);
  clear_scalars(c, kScalarPackLast, kScalarPack, st);
  hipLaunchKernelGGL(check_splits_kernel, dim3(std::min<unsigned>(cdiv(n_docs + 1, kBlock), 1024u)), block, 0, st, d_splits, n_docs,
                     c->d_scalars + kScalarPackBad, reinterpret_cast<long long *>(c->d_scalars + kScalarPackLast));
  hipLaunchKernelGGL(seqpack_plan_kernel, dim3(std::min<unsigned>(cdiv(n_docs, kBlock), kPackMaxGrid)), block, 0, st, d_splits, n_docs, g,
                     d_piece_base, d_cell_base, d_tot);
  WP_LAUNCH_CHECK();
  queue_scalar_slots(c, kScalarPackLast, kScalarPack, st);
  WP_HIP(hipStreamSynchronize(st));
  if (c->h_scalars[kScalarPackBad] != 0) throw std::invalid_argument("pack: row_splits must start at 0 and never descend");
  long long last;
  std::memcpy(&last, c->h_scalars + kScalarPackLast, sizeof(last));
  check_pack_totals(static_cast<unsigned long long>(last), h_tot[kPackStream]);
  if (last > 0 && !d_ids) throw std::invalid_argument("pack: ids is NULL");
  ps.n_empty = static_cast<int64_t>(h_tot[kPackEmpty]);
  ps.n_cut = static_cast<int64_t>(h_tot[kPackCut]);
  ps.n_ids_cut = static_cast<int64_t>(h_tot[kPackIdsCut]);
  ps.n_pieces = static_cast<int64_t>(h_tot[kPackPieces]);
  g.n_ids = static_cast<uint32_t>(last);
  g.n_cells = static_cast<uint32_t>(h_tot[kPackStream]);
  g.n_pieces = static_cast<uint32_t>(h_tot[kPackPieces]);  // (every unit holds a cell: n_pieces <= n_cells)
  if (g.n_pieces == 0) return 0;
  const size_t n_p = g.n_pieces, n_tiles = cdiv(n_p, kPackPieceTile);
  Arena tab(&c->pack_tab);  // its own arena: the number of pieces is known only behind the wait above
  uint32_t *d_P = nullptr, *d_nx = nullptr, *d_row_first = nullptr, *d_tile_entry = nullptr, *d_tile_row = nullptr;
  int32_t *d_src0 = nullptr;
  unsigned long long *d_rec = nullptr;
  for (int pass = 0; pass < 2; pass++) {
    // + 1: P[n_p] = N (seqpack_pieces_kernel) and row_first[n_out] = n_p (seqpack_spine_kernel); src0 and nx are sized alike
    d_P = tab.take<uint32_t>(n_p + 1);
    d_src0 = tab.take<int32_t>(n_p + 1);
    d_nx = tab.take<uint32_t>(n_p + 1);
    d_row_first = tab.take<uint32_t>(n_p + 1);
    d_tile_entry = tab.take<uint32_t>(n_tiles);
    d_tile_row = tab.take<uint32_t>(n_tiles);
    d_rec = tab.take<unsigned long long>(n_p);
    if (pass == 0) tab.commit();
  }
  device_exclusive_scan(d_piece_base, d_piece_base, n_docs, d_scan_tmp, nullptr, st);
  device_exclusive_scan(d_cell_base, d_cell_base, n_docs, d_scan_tmp, nullptr, st);
  hipLaunchKernelGGL(seqpack_pieces_kernel, dim3(cdiv(n_p, kBlock)), block, 0, st, d_splits, static_cast<uint32_t>(n_docs), d_piece_base,
                     d_cell_base, g, d_P, d_src0);
  WP_LAUNCH_CHECK();
  unsigned long long n_out = (static_cast<unsigned long long>(g.n_cells) + g.max_len - 1) / static_cast<unsigned long long>(g.max_len);
  if (!g.stream) {
    WP_HIP(hipMemsetAsync(d_tile_entry, 0xFF, n_tiles * sizeof(uint32_t), st));
    hipLaunchKernelGGL(seqpack_tile_kernel, dim3(static_cast<unsigned>(n_tiles)), block, 0, st, d_P, g.n_pieces, static_cast<uint32_t>(g.max_len),
                       d_nx, d_rec);
    hipLaunchKernelGGL(seqpack_spine_kernel, dim3(1), dim3(kWave), 0, st, d_rec, g.n_pieces, d_tile_entry, d_tile_row, d_row_first, d_tot);
    WP_LAUNCH_CHECK();
    queue_scalar_slots(c, kScalarPack, kScalarPack, st);
    WP_HIP(hipStreamSynchronize(st));
    n_out = h_tot[kPackRows];
  }
  ps.n_out = static_cast<int64_t>(n_out);
  check_pack_rows(n_out, g.max_len);
  g.n_out = static_cast<uint32_t>(n_out);
  const PackOut o = place(static_cast<size_t>(n_out));
  if (!g.stream) {
    hipLaunchKernelGGL(seqpack_apply_kernel, dim3(static_cast<unsigned>(n_tiles)), block, 0, st, d_nx, g.n_pieces, static_cast<uint32_t>(g.max_len),
                       d_tile_entry, d_tile_row, d_row_first);
  }
  const size_t cell_tiles = cdiv(static_cast<size_t>(n_out) * static_cast<size_t>(g.max_len), kPackCellTile);
  hipLaunchKernelGGL(seqpack_write_kernel, dim3(static_cast<unsigned>(std::min<size_t>(cell_tiles, kPackMaxGrid))), block, 0, st, d_ids, d_P,
                     d_src0, d_row_first, g, o, d_tot);
  WP_LAUNCH_CHECK();
  queue_scalar_slots(c, kScalarPack, kScalarPack, st);
  WP_HIP(hipStreamSynchronize(st));
  throw_if_oob(kSitePack, "pack", "gathers or stores outside their buffers skipped");
  ps.n_cells = static_cast<int64_t>(h_tot[kPackCells]);
  ps.n_segments = static_cast<int64_t>(h_tot[kPackSegments]);
  return static_cast<size_t>(n_out);
}

// the buffers of a host call's batch of n_out rows, in c->pack_out until the handle's next call:
// input_ids | segment_ids | position_ids | source | lengths
static PackOut pack_batch(Context *c, size_t n_out, int max_len) {
  const size_t cells = n_out * static_cast<size_t>(max_len);
  Arena a(&c->pack_out);
  PackOut o{};
  for (int pass = 0; pass < 2; pass++) {
    o.input_ids = a.take<int32_t>(cells);
    o.segment_ids = a.take<int32_t>(cells);
    o.position_ids = a.take<int32_t>(cells);
    o.source = a.take<int32_t>(cells);
    o.lengths = a.take<int32_t>(n_out);
    if (pass == 0) a.commit();
  }
  return o;
}

}  // namespace wp
