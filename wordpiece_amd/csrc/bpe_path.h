// bpe_path.h — the byte-level BPE encoder on a context (include/wordpiece_amd_bpe.h; kernels: bpe.h): the argument rules of
// a model and of a call, the model a slot of the handle owns (its upload, its pair table, its release), the launches over
// one device batch and the buffers of a call.  The intake and the per-row arrays are text_path.h's.
#pragma once
#include <algorithm>
#include <vector>

#include "bpe.h"
#include "context.h"
#include "text_path.h"

namespace wp {

static int check_bpe_slot(int slot) {
  if (slot < 0 || slot >= WP_BPE_SLOTS) throw std::invalid_argument("bpe: slot must be in [0, 3]");
  return slot;
}

// ---- the model of a slot ------------------------------------------------------------------------------------------------------
// frees the model s holds on its device (the streams that used it have been waited for: every call ends with a wait) and
// empties s
static void bpe_free(wp_vocab *v, BpeSlot &s) {
  if (s.loaded) {
    DeviceGuard keep;
    (void)hipSetDevice(s.device);
    if (v->ctx) (void)hipStreamSynchronize(v->ctx->stream);
    for (const void *p : {static_cast<const void *>(s.m.byte_id), static_cast<const void *>(s.m.merges), static_cast<const void *>(s.m.table),
                          static_cast<const void *>(s.m.cls_index), static_cast<const void *>(s.m.cls_pages)}) {
      if (p) (void)hipFree(const_cast<void *>(p));
    }
  }
  s = BpeSlot{};
}
static void bpe_release(wp_vocab *v, int slot) { bpe_free(v, v->bpe[slot]); }

// Every rule of a model, each with the field it is about, and its pair table: `cap` entries (left, right, rank, result), a
// power of two >= 2 n_merges and 16, left = kBpeEmpty where the slot is empty; a pair's home is bpe_pair_hash & (cap - 1),
// linear probing forward with wrap.  Nothing here needs a device.
static std::vector<uint4> check_bpe_model(const wp_bpe_model *m) {
  if (!m) throw std::invalid_argument("bpe: m is NULL");
  if (m->pattern != WP_BPE_PATTERN_GPT2) throw std::invalid_argument("bpe: pattern must be WP_BPE_PATTERN_GPT2 (0)");
  if (m->reserved != 0) throw std::invalid_argument("bpe: reserved must be 0");
  if (m->n_ids < 256 || m->n_ids >= (int64_t(1) << 31)) throw std::invalid_argument("bpe: n_ids must be in [256, 2^31)");
  if (m->n_merges < 0) throw std::invalid_argument("bpe: n_merges must not be negative");
  if (m->n_merges >= (int64_t(1) << 30)) throw std::length_error("bpe: n_merges must stay below 2^30");
  if (!m->byte_id) throw std::invalid_argument("bpe: byte_id is NULL");
  if (m->n_merges != 0 && !m->merges) throw std::invalid_argument("bpe: merges is NULL");
  std::vector<bool> known(static_cast<size_t>(m->n_ids), false);
  for (int b = 0; b < 256; b++) {
    const int32_t id = m->byte_id[b];
    if (id < 0 || id >= m->n_ids) throw std::invalid_argument("bpe: byte_id[" + std::to_string(b) + "] is outside [0, n_ids)");
    if (known[static_cast<size_t>(id)]) throw std::invalid_argument("bpe: byte_id[" + std::to_string(b) + "] is the id of an earlier byte");
    known[static_cast<size_t>(id)] = true;
  }
  size_t cap = 16;
  while (cap < 2 * static_cast<size_t>(m->n_merges)) cap <<= 1;
  std::vector<uint4> table(cap, uint4{kBpeEmpty, 0u, 0u, 0u});
  for (int64_t k = 0; k < m->n_merges; k++) {
    const int32_t *t = m->merges + 3 * k;
    const std::string name = "bpe: merges[" + std::to_string(k) + "]";
    for (int f = 0; f < 3; f++) {
      if (t[f] < 0 || t[f] >= m->n_ids) throw std::invalid_argument(name + " has an id outside [0, n_ids)");
    }
    for (int f = 0; f < 2; f++) {
      if (!known[static_cast<size_t>(t[f])]) throw std::invalid_argument(name + " has an operand that is neither a byte id nor the result of an earlier merge");
    }
    const uint32_t l = static_cast<uint32_t>(t[0]), r = static_cast<uint32_t>(t[1]);
    size_t slot = bpe_pair_hash(l, r) & (cap - 1);
    for (; table[slot].x != kBpeEmpty; slot = (slot + 1) & (cap - 1)) {
      if (table[slot].x == l && table[slot].y == r) throw std::invalid_argument(name + " repeats the pair of merges[" + std::to_string(table[slot].z) + "]");
    }
    table[slot] = uint4{l, r, static_cast<uint32_t>(k), static_cast<uint32_t>(t[2])};
    known[static_cast<size_t>(t[2])] = true;
  }
  return table;
}

template <typename T>
static const T *bpe_upload(const T *src, size_t count, hipStream_t st) {
  T *d = nullptr;
  WP_HIP(hipMalloc(&d, std::max<size_t>(count, 1) * sizeof(T)));
  if (count != 0 && hipMemcpyAsync(d, src, count * sizeof(T), hipMemcpyHostToDevice, st) != hipSuccess) {
    (void)hipFree(d);
    throw HipError("bpe: a table of the model could not be copied to the device");
  }
  return d;
}

// the checked model m with its table into the slot, on c's device; the slot's earlier model goes once the new one is there,
// and stays where the load fails
static void bpe_load_on_device(wp_vocab *v, Context *c, int slot, const wp_bpe_model *m, const std::vector<uint4> &table) {
  BpeSlot s;
  s.loaded = true;  // (from here on bpe_free frees what is there)
  s.device = c->device;
  hipStream_t st = c->stream;
  try {
    s.m.byte_id = bpe_upload(m->byte_id, 256, st);
    s.m.merges = bpe_upload(m->merges, 3 * static_cast<size_t>(m->n_merges), st);
    s.m.table = bpe_upload(table.data(), table.size(), st);
    s.m.cls_index = bpe_upload(kBpeIndex, kBpeIndexSize, st);
    s.m.cls_pages = bpe_upload(kBpePageData, sizeof(kBpePageData), st);
    WP_HIP(hipStreamSynchronize(st));
  } catch (...) {
    bpe_free(v, s);
    throw;
  }
  s.m.table_mask = static_cast<uint32_t>(table.size() - 1);
  s.m.n_merges = static_cast<uint32_t>(m->n_merges);
  s.m.n_ids = static_cast<uint32_t>(m->n_ids);
  bpe_release(v, slot);  // (the statistics of the slot start again with the new model)
  v->bpe[slot] = s;
}

// ---- a call ---------------------------------------------------------------------------------------------------------------------
struct BpePlan {
  int slot = 0;
  bool want_offsets = false, want_pieces = false;
};

// every rule of the spec that reads no model, each with the field it is about; nothing here needs a device
static BpePlan check_bpe_spec(const wp_bpe_spec *spec, const wp_bpe_result *out) {
  if (!spec) throw std::invalid_argument("bpe: spec is NULL");
  if (!out) throw std::invalid_argument("bpe: out is NULL");
  BpePlan p;
  p.slot = check_bpe_slot(spec->slot);
  check_want("bpe", spec->want, WP_BPE_WANT_OFFSETS | WP_BPE_WANT_PIECES);
  p.want_offsets = (spec->want & WP_BPE_WANT_OFFSETS) != 0;
  p.want_pieces = (spec->want & WP_BPE_WANT_PIECES) != 0;
  if (spec->pad != 0) throw std::invalid_argument("bpe: pad must be 0");
  if (spec->pad2 != 0) throw std::invalid_argument("bpe: pad2 must be 0");
  if (spec->reserved != 0) throw std::invalid_argument("bpe: reserved must be 0");
  return p;
}

// ... and, behind the rules of the batch, the one that reads the slot: it holds a model
static void check_bpe_loaded(const wp_vocab *v, const BpePlan &p) {
  if (!v->bpe[p.slot].loaded) throw std::invalid_argument("bpe: slot " + std::to_string(p.slot) + " holds no model");
}

// (kept: the medium pieces; words: the pieces; lines: the long pieces; out_bytes: their bytes; counters: the longest piece)
constexpr TextLayer kBpeLayer{"bpe", "bpe", "gathers or stores outside the tile, piece, cell or row arrays skipped",
                              kScalarBpeBad, kScalarBpeMedium, kScalarBpeElems, kScalarBpeWindows, kScalarBpePieces, kScalarBpeLong, kScalarBpeLongBytes,
                              kScalarBpe, 1};

static wp_bpe_stats &begin_bpe_stats(wp_vocab *v, int slot, size_t n_rows) {
  BpeSlot &s = v->bpe[slot];
  s.called = true;
  s.last = wp_bpe_stats{};
  s.last.n_rows = static_cast<int64_t>(n_rows);
  return s.last;
}

// The batch `in` (n_rows >= 1), on c's stream.  The results are device pointers into c->bpe_out, valid until the handle's
// next call.  Waits: the sizes; the pieces; the medium and the long ones; the ids; the one that ends the call.
static void bpe_on_device(wp_vocab *v, Context *c, const RaggedIn &in, const BpePlan &plan, wp_bpe_result *R) {
  const TextLayer &L = kBpeLayer;
  const BpeModel m = v->bpe[plan.slot].m;
  const size_t n = in.n_rows, n1 = n + 1;
  wp_bpe_stats &ps = begin_bpe_stats(v, plan.slot, n);
  *R = wp_bpe_result{};
  R->n_rows = static_cast<int64_t>(n);
  hipStream_t st = c->stream;
  const bool guard = v->arena_guard || EnvOptions::get().arena_guard;
  // WP_OPT_STAGE_TIMING: kMarkStart, kMarkCounted (intake, class and start pass, piece list), kMarkSorted (merge pass),
  // kMarkScanned (compaction, row_splits, offsets), kMarkWalked (the end)
  const bool timing = v->stage_timing;
  begin_stage_timing(c, timing, st);

  // ---- the per-row arrays, the offset check ----------------------------------------------------------------------------------
  Arena ra(&c->bpe_rows, guard);
  TextRows rows;  // (the byte offsets and the scan scratch are what this layer takes; its one signal per row stays 0)
  for (int pass = 0; pass < 2; pass++) {
    rows.take(ra, n, 1);
    if (pass == 0) ra.commit();
  }
  ra.arm(st);
  rows.queue(c, L, in, st);
  const size_t nb = rows.read(c, L, in, st);
  const uint32_t *d32 = static_cast<const uint32_t *>(in.d_data);
  const uint8_t *d8 = static_cast<const uint8_t *>(in.d_data);

  // ---- the class and start pass: the document bits, the start bitmap, the tiles' scan, the piece list -----------------------
  const size_t n_tiles = cdiv(nb, kBpeTile), nt1 = n_tiles + 1, n_groups = n_tiles * kBpeGroups;
  Arena ta(&c->bpe_tiles, guard);
  uint32_t *d_docbits = nullptr, *d_tiles = nullptr, *d_ttmp = nullptr;
  unsigned long long *d_startbits = nullptr;
  for (int pass = 0; pass < 2; pass++) {
    d_docbits = ta.take<uint32_t>(nb / 32 + 2);
    d_startbits = ta.take<unsigned long long>(n_groups + 1);
    d_tiles = ta.take<uint32_t>(nt1);
    d_ttmp = ta.take<uint32_t>(cdiv(nt1, kScanTile) + 8);
    if (pass == 0) ta.commit();
  }
  ta.arm(st);
  WP_HIP(hipMemsetAsync(d_docbits, 0, (nb / 32 + 2) * sizeof(uint32_t), st));
  WP_HIP(hipMemsetAsync(d_tiles, 0, nt1 * sizeof(uint32_t), st));
  size_t np = 0;
  if (nb != 0) {
    hipLaunchKernelGGL(cls_docbits_kernel, count_grid(n), dim3(kBlock), 0, st, static_cast<const uint32_t *>(rows.d_boff), n, nb, d_docbits);
    hipLaunchKernelGGL(bpe_start_kernel, dim3(n_tiles), dim3(kBlock), 0, st, d32, nb, static_cast<const uint32_t *>(d_docbits), m, d_startbits, d_tiles);
    device_exclusive_scan(d_tiles, d_tiles, nt1, d_ttmp, c->d_scalars + L.words, st);
    WP_LAUNCH_CHECK();
    queue_scalar_slots(c, L.words, L.words, st);
    WP_HIP(hipStreamSynchronize(st));
    np = c->h_scalars[L.words];
    if (np == 0 || np > nb) throw HipError("bpe: the pieces of the text do not fit its bytes");
  }
  const size_t np1 = np + 1;
  Arena pa(&c->bpe_pieces, guard);
  uint32_t *d_pstart = nullptr, *d_cnt = nullptr, *d_idpos = nullptr, *d_med = nullptr, *d_lng = nullptr, *d_med_pos = nullptr, *d_lng_pos = nullptr, *d_ptmp = nullptr, *d_ends = nullptr;
  int32_t *d_cells = nullptr;
  for (int pass = 0; pass < 2; pass++) {
    d_pstart = pa.take<uint32_t>(np1);
    d_cnt = pa.take<uint32_t>(np1);
    d_idpos = pa.take<uint32_t>(np1);
    d_med = pa.take<uint32_t>(np1);
    d_lng = pa.take<uint32_t>(np1);
    d_med_pos = pa.take<uint32_t>(np1);
    d_lng_pos = pa.take<uint32_t>(np1);
    d_ptmp = pa.take<uint32_t>(cdiv(np1, kScanTile) + 8);
    d_cells = pa.take<int32_t>(nb);
    if (plan.want_offsets) d_ends = pa.take<uint32_t>(nb);
    if (pass == 0) pa.commit();
  }
  pa.arm(st);
  WP_HIP(hipMemsetAsync(d_cnt, 0, np1 * sizeof(uint32_t), st));
  size_t n_med = 0, n_lng = 0, long_bytes = 0;
  if (np != 0) {
    hipLaunchKernelGGL(bpe_list_kernel, dim3(n_tiles), dim3(kBlock), 0, st, static_cast<const unsigned long long *>(d_startbits), static_cast<const uint32_t *>(d_tiles),
                       nb, np, d_pstart);
    hipLaunchKernelGGL(bpe_deal_kernel, count_grid(np1), dim3(kBlock), 0, st, static_cast<const uint32_t *>(d_pstart), np, d_med, d_lng,
                       reinterpret_cast<unsigned long long *>(c->d_scalars + L.counters), c->d_scalars + L.out_bytes);
  }
  if (timing) WP_HIP(hipEventRecord(c->ev[kMarkCounted], st));

  // ---- the merge pass ----------------------------------------------------------------------------------------------------------
  const BpeCells cells{d_cells, d_ends, d_cnt};
  Arena sa(&c->bpe_scratch, guard);
  if (np != 0) {
    hipLaunchKernelGGL(bpe_short_kernel, count_grid(np), dim3(kBlock), 0, st, d8, nb, static_cast<const uint32_t *>(d_pstart), np, m, cells);
    device_exclusive_scan(d_med, d_med_pos, np1, d_ptmp, c->d_scalars + L.kept, st);
    device_exclusive_scan(d_lng, d_lng_pos, np1, d_ptmp, c->d_scalars + L.lines, st);
    WP_LAUNCH_CHECK();
    queue_scalar_slots(c, L.kept, L.counters, st);
    WP_HIP(hipStreamSynchronize(st));
    n_med = c->h_scalars[L.kept];
    n_lng = c->h_scalars[L.lines];
    long_bytes = c->h_scalars[L.out_bytes];
    if (n_med + n_lng > np || long_bytes > nb || (n_lng == 0) != (long_bytes == 0)) throw HipError("bpe: the medium and long pieces do not fit the piece list");
  }
  if (n_med + n_lng != 0) {
    uint32_t *d_mlist = nullptr, *d_llist = nullptr, *d_llen = nullptr, *d_loff = nullptr, *d_ltmp = nullptr, *s_rk = nullptr, *s_len = nullptr;
    int32_t *s_sym = nullptr;
    uint8_t *s_fresh = nullptr;
    for (int pass = 0; pass < 2; pass++) {
      d_mlist = sa.take<uint32_t>(n_med);
      d_llist = sa.take<uint32_t>(n_lng);
      d_llen = sa.take<uint32_t>(n_lng + 1);
      d_loff = sa.take<uint32_t>(n_lng + 1);
      d_ltmp = sa.take<uint32_t>(cdiv(n_lng + 1, kScanTile) + 8);
      s_sym = sa.take<int32_t>(2 * long_bytes);
      s_rk = sa.take<uint32_t>(2 * long_bytes);
      s_len = sa.take<uint32_t>(2 * long_bytes);
      s_fresh = sa.take<uint8_t>(long_bytes);
      if (pass == 0) sa.commit();
    }
    sa.arm(st);
    hipLaunchKernelGGL(bpe_lists_kernel, count_grid(np), dim3(kBlock), 0, st, static_cast<const uint32_t *>(d_pstart), np, static_cast<const uint32_t *>(d_med),
                       static_cast<const uint32_t *>(d_med_pos), n_med, static_cast<const uint32_t *>(d_lng), static_cast<const uint32_t *>(d_lng_pos), n_lng, d_mlist,
                       d_llist, d_llen);
    if (n_med != 0) {
      hipLaunchKernelGGL(bpe_medium_kernel, dim3(cdiv(n_med, kBlock / kWave)), dim3(kBlock), 0, st, d8, nb, static_cast<const uint32_t *>(d_pstart), np,
                         static_cast<const uint32_t *>(d_mlist), n_med, m, cells);
    }
    if (n_lng != 0) {
      device_exclusive_scan(d_llen, d_loff, n_lng + 1, d_ltmp, nullptr, st);
      hipLaunchKernelGGL(bpe_long_kernel, dim3(n_lng), dim3(kBlock), 0, st, d8, nb, static_cast<const uint32_t *>(d_pstart), np, static_cast<const uint32_t *>(d_llist),
                         static_cast<const uint32_t *>(d_loff), n_lng, long_bytes, m, s_sym, s_rk, s_len, s_fresh, cells);
    }
    WP_LAUNCH_CHECK();
  }
  if (timing) WP_HIP(hipEventRecord(c->ev[kMarkSorted], st));

  // ---- the compaction: the scan of the counts, the flat copy, the splits ----------------------------------------------------------
  device_exclusive_scan(d_cnt, d_idpos, np1, d_ptmp, c->d_scalars + kScalarBpeIds, st);
  queue_scalar_slots(c, kScalarBpeIds, kScalarBpeIds, st);
  WP_HIP(hipStreamSynchronize(st));
  const size_t n_out = c->h_scalars[kScalarBpeIds];
  if (n_out > nb || (n_out == 0) != (nb == 0)) throw HipError("bpe: the ids of the pieces do not fit the bytes of the text");
  Arena oa(&c->bpe_out, guard);
  BpeOut o{};
  for (int pass = 0; pass < 2; pass++) {
    o.ids = oa.take<int32_t>(n_out);
    o.row_splits = oa.take<long long>(n1);
    if (plan.want_offsets) {
      o.begin = oa.take<int32_t>(n_out);
      o.end = oa.take<int32_t>(n_out);
    }
    if (plan.want_pieces) o.piece_splits = oa.take<long long>(np1);
    if (pass == 0) oa.commit();
  }
  oa.arm(st);
  if (nb != 0) {
    hipLaunchKernelGGL(bpe_copy_kernel, dim3(n_tiles), dim3(kBlock), 0, st, static_cast<const unsigned long long *>(d_startbits), static_cast<const uint32_t *>(d_tiles), nb,
                       static_cast<const uint32_t *>(d_pstart), static_cast<const uint32_t *>(d_idpos), np, cells, static_cast<const uint32_t *>(rows.d_boff), n, n_out, o);
  }
  hipLaunchKernelGGL(bpe_splits_kernel, count_grid(std::max(n1, np1)), dim3(kBlock), 0, st, static_cast<const unsigned long long *>(d_startbits),
                     static_cast<const uint32_t *>(d_tiles), nb, static_cast<const uint32_t *>(d_idpos), np, static_cast<const uint32_t *>(rows.d_boff), n, o);
  WP_LAUNCH_CHECK();
  if (timing) {
    WP_HIP(hipEventRecord(c->ev[kMarkScanned], st));
    WP_HIP(hipEventRecord(c->ev[kMarkWalked], st));
  }
  WP_HIP(hipStreamSynchronize(st));
  unsigned long long longest;
  std::memcpy(&longest, c->h_scalars + L.counters, sizeof(longest));
  ps.n_pieces = static_cast<int64_t>(np);
  ps.n_ids = static_cast<int64_t>(n_out);
  ps.max_piece = static_cast<int64_t>(longest);
  ps.n_short = static_cast<int64_t>(np - n_med - n_lng);
  ps.n_medium = static_cast<int64_t>(n_med);
  ps.n_long = static_cast<int64_t>(n_lng);
  if (timing) end_four_stage_timing(v, c);
  throw_if_group_oob(kSiteQuality, L.oob_name, L.oob_skipped, kSiteOverlap, "gathers or stores outside the row arrays skipped");
  for (const Arena *a : {&ra, &ta, &pa, &sa, &oa}) check_arena_guard(c, *a, st, L.name);
  R->ids = o.ids;
  R->row_splits = reinterpret_cast<int64_t *>(o.row_splits);
  R->begin = o.begin;
  R->end = o.end;
  R->piece_splits = reinterpret_cast<int64_t *>(o.piece_splits);
  R->n_ids = static_cast<int64_t>(n_out);
  R->n_pieces = static_cast<int64_t>(np);
}

}  // namespace wp
