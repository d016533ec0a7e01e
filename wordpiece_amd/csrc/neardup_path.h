// neardup_path.h — near-duplicate rows on a context (include/wordpiece_amd.h, section "near-duplicate rows"; kernels:
// neardup.h): the argument rules, the launches over a device batch, the component rounds and the buffers of a call.
#pragma once
#include "context.h"
#include "group_path.h"
#include "neardup.h"

namespace wp {

// the component rounds did not end within what the scheme guarantees: WP_ERR_INTERNAL
struct InternalError : std::logic_error {
  using std::logic_error::logic_error;
};

// the spec of a call, checked
struct NearDupPlan {
  uint32_t elem_bytes = 1, shingle = 5, n_perm = 128, bands = 16, min_agree = 0;
  uint64_t seed = 0;
  bool want_inverse = false, want_compact = false, want_signatures = false;
};

// every rule of the spec, each with the field it is about; nothing here needs a device
static NearDupPlan check_neardup_spec(const wp_neardup_spec *spec, const wp_neardup_result *out) {
  if (!spec) throw std::invalid_argument("neardup: spec is NULL");
  if (!out) throw std::invalid_argument("neardup: out is NULL");
  check_elem_bytes("neardup", spec->elem_bytes);
  check_want("neardup", spec->want, WP_NEARDUP_WANT_INVERSE | WP_NEARDUP_WANT_COMPACT | WP_NEARDUP_WANT_SIGNATURES);
  if (spec->shingle < 1 || spec->shingle > kNearMaxShingle) throw std::invalid_argument("neardup: shingle must be in [1, 64]");
  if (spec->n_perm < 1 || spec->n_perm > kNearMaxPerm) throw std::invalid_argument("neardup: n_perm must be in [1, 256]");
  if (spec->bands < 1 || spec->n_perm % spec->bands != 0) throw std::invalid_argument("neardup: bands must be at least 1 and divide n_perm");
  if (spec->min_agree < 0 || spec->min_agree > spec->n_perm) throw std::invalid_argument("neardup: min_agree must be in [0, n_perm]");
  if (spec->reserved[0] != 0 || spec->reserved[1] != 0) throw std::invalid_argument("neardup: reserved must be 0");
  NearDupPlan p;
  p.elem_bytes = static_cast<uint32_t>(spec->elem_bytes);
  p.shingle = static_cast<uint32_t>(spec->shingle);
  p.n_perm = static_cast<uint32_t>(spec->n_perm);
  p.bands = static_cast<uint32_t>(spec->bands);
  p.min_agree = static_cast<uint32_t>(spec->min_agree);
  p.seed = spec->seed;
  p.want_inverse = (spec->want & WP_NEARDUP_WANT_INVERSE) != 0;
  p.want_compact = (spec->want & WP_NEARDUP_WANT_COMPACT) != 0;
  p.want_signatures = (spec->want & WP_NEARDUP_WANT_SIGNATURES) != 0;
  return p;
}

static void check_neardup_rows(size_t n_rows, const NearDupPlan &plan) {
  check_row_count("neardup", n_rows);
  if (static_cast<unsigned long long>(n_rows) * plan.n_perm >= (1ull << 32)) throw std::length_error("neardup: n_rows * n_perm reaches 2^32");
  if (static_cast<unsigned long long>(n_rows) * plan.bands >= (1ull << 32)) throw std::length_error("neardup: n_rows * bands reaches 2^32");
}

// the statistics of a neardup call before anything is known of its rows
static wp_neardup_stats &begin_neardup_stats(wp_vocab *v, size_t n_rows) {
  v->stats.neardup_call = 1;
  v->stats.neardup = wp_neardup_stats{};
  v->stats.neardup.n_rows = static_cast<int64_t>(n_rows);
  return v->stats.neardup;
}

// no row, or rows that are all empty and so each a cluster of its own: no device needed
static wp_neardup_result neardup_all_empty(wp_vocab *v, size_t n_rows, const NearDupPlan &plan) {
  wp_neardup_stats &ns = begin_neardup_stats(v, n_rows);
  wp_neardup_result h{};
  h.n_rows = static_cast<int64_t>(n_rows);
  h.n_perm = static_cast<int64_t>(plan.n_perm);
  if (plan.want_compact) h.row_off = static_cast<int64_t *>(zeroed((n_rows + 1) * sizeof(int64_t)));
  if (n_rows == 0) return h;
  ns.n_unique = ns.n_empty = static_cast<int64_t>(n_rows);
  h.n_unique = static_cast<int64_t>(n_rows);
  h.cluster = static_cast<int32_t *>(zeroed(n_rows * sizeof(int32_t)));
  h.kept = static_cast<int32_t *>(zeroed(n_rows * sizeof(int32_t)));
  h.counts = static_cast<int64_t *>(zeroed(n_rows * sizeof(int64_t)));
  if (plan.want_inverse) h.inverse = static_cast<int32_t *>(zeroed(n_rows * sizeof(int32_t)));
  for (size_t r = 0; r < n_rows; r++) {
    h.cluster[r] = h.kept[r] = static_cast<int32_t>(r);
    h.counts[r] = 1;
    if (h.inverse) h.inverse[r] = static_cast<int32_t>(r);
  }
  if (plan.want_signatures) {
    const size_t bytes = n_rows * plan.n_perm * sizeof(uint32_t);
    h.signatures = static_cast<uint32_t *>(zeroed(bytes));
    std::memset(h.signatures, 0xff, bytes);
  }
  return h;
}

template <int SLOTS>
static void launch_near_sig(unsigned tiles, hipStream_t st, const uint32_t *d32, size_t n_bytes, const uint32_t *d_boff, const uint32_t *d_pos_off,
                            size_t n, size_t n_positions, const NearDupPlan &plan, uint32_t *d_sig) {
  hipLaunchKernelGGL(near_sig_kernel<SLOTS>, dim3(tiles), dim3(kBlock), 0, st, d32, n_bytes, d_boff, d_pos_off, n, n_positions, plan.elem_bytes,
                     plan.shingle, plan.n_perm, plan.seed, d_sig);
}

// The rows of the batch `in` (n_rows >= 1), on c's stream.  The results are device pointers into
// c->neardup_rows (cluster, signatures) and c->neardup_out (everything else), valid until the handle's next call.
// Waits: the sizes (the offset check, the elements, the positions, the empty rows), one behind the grouping (it brings
// the candidate count), with min_agree > 0 one behind the comparison (the edge count), one per component round (its
// "changed" word), the kept count, and the one that ends the call (the size of the compact form and the counters).
// The component rounds.  At the start of a round every label is a root (label[label[i]] == label[i]: the jump kernel
// of the round before, or the first labels).  A round that lowers any label lowers a root's first, and that row is no
// root afterwards, so every round that reports a change leaves at least one root fewer; there are at most n_rows roots.
// The loop therefore ends within n_rows + 1 rounds, and throws where it does not.
static void neardup_on_device(wp_vocab *v, Context *c, const RaggedIn &in, const NearDupPlan &plan, wp_neardup_result *R) {
  const size_t n = in.n_rows;
  wp_neardup_stats &ns = begin_neardup_stats(v, n);
  *R = wp_neardup_result{};
  R->n_rows = static_cast<int64_t>(n);
  R->n_perm = static_cast<int64_t>(plan.n_perm);
  hipStream_t st = c->stream;
  const bool guard = v->arena_guard || EnvOptions::get().arena_guard;
  const uint32_t eb = in.elem_bytes;
  // WP_OPT_STAGE_TIMING: kMarkStart, kMarkCounted (offsets checked, positions listed), kMarkSymbols (signatures),
  // kMarkSorted (band keys, sort, heads, edges), kMarkWalked (components, table, compact form)
  const bool timing = v->stage_timing;
  RadixStats *rs = begin_stage_timing(c, timing, st);

  // ---- the per-row arrays, the offset check, the position list ---------------------------------------------------------
  const size_t n1 = n + 1;
  const size_t sig_words = n * plan.n_perm;  // (< 2^32: check_neardup_rows)
  Arena ra(&c->neardup_rows, guard);
  uint32_t *d_boff = nullptr, *d_npos = nullptr, *d_pos_off = nullptr, *d_has = nullptr, *d_has_pos = nullptr, *d_rows = nullptr, *d_sig = nullptr,
           *d_rcount = nullptr, *d_keep = nullptr, *d_keep_pos = nullptr, *d_out_len = nullptr, *d_out_pos = nullptr, *d_stmp = nullptr;
  int32_t *d_cluster = nullptr;
  for (int pass = 0; pass < 2; pass++) {
    d_boff = ra.take<uint32_t>(n1);
    d_npos = ra.take<uint32_t>(n1);
    d_pos_off = ra.take<uint32_t>(n1);
    d_has = ra.take<uint32_t>(n1);
    d_has_pos = ra.take<uint32_t>(n1);
    d_rows = ra.take<uint32_t>(n);
    d_cluster = ra.take<int32_t>(n);
    d_sig = ra.take<uint32_t>(sig_words);
    d_rcount = ra.take<uint32_t>(n);
    d_keep = ra.take<uint32_t>(n1);
    d_keep_pos = ra.take<uint32_t>(n1);
    d_out_len = ra.take<uint32_t>(n1);
    d_out_pos = ra.take<uint32_t>(n1);
    d_stmp = ra.take<uint32_t>(cdiv(n1, kScanTile) + 8);
    if (pass == 0) ra.commit();
  }
  ra.arm(st);
  unsigned long long *d_counters = reinterpret_cast<unsigned long long *>(c->d_scalars + kScalarNear);
  unsigned long long *d_elems = reinterpret_cast<unsigned long long *>(c->d_scalars + kScalarNearElems);
  unsigned long long *d_positions = reinterpret_cast<unsigned long long *>(c->d_scalars + kScalarNearPositions);
  clear_scalars(c, kScalarNearBad, kScalarNear, st);
  WP_HIP(hipMemsetAsync(c->d_scalars + kScalarNearBad, 0xff, sizeof(uint32_t), st));
  hipLaunchKernelGGL(near_rows_kernel, count_grid(n1), dim3(kBlock), 0, st, in.d_row_off, n, eb, plan.shingle, d_boff, d_npos, d_has, d_cluster,
                     c->d_scalars + kScalarNearBad, d_elems, d_counters);
  device_exclusive_scan(d_npos, d_pos_off, n1, d_stmp, nullptr, st, nullptr, d_positions);
  device_exclusive_scan(d_has, d_has_pos, n1, d_stmp, nullptr, st);
  compact_flagged(d_has, d_has_pos, n, nullptr, d_rows, st);
  WP_HIP(hipMemsetAsync(d_sig, 0xff, sig_words * sizeof(uint32_t), st));  // (a row without shingles keeps this; atomicMin starts from it)
  WP_HIP(hipMemsetAsync(d_rcount, 0, n * sizeof(uint32_t), st));
  WP_LAUNCH_CHECK();
  if (timing) WP_HIP(hipEventRecord(c->ev[kMarkCounted], st));
  queue_scalar_slots(c, kScalarNearBad, kScalarNear, st);
  WP_HIP(hipStreamSynchronize(st));
  unsigned long long elems64, positions64, counters[kNearCounters];
  std::memcpy(&elems64, c->h_scalars + kScalarNearElems, sizeof(elems64));
  std::memcpy(&positions64, c->h_scalars + kScalarNearPositions, sizeof(positions64));
  std::memcpy(counters, c->h_scalars + kScalarNear, sizeof(counters));
  const size_t n_bytes = check_ragged_device("neardup", in, c->h_scalars[kScalarNearBad], elems64);
  if (positions64 > elems64 || counters[kNearEmpty] > n) throw HipError("neardup: the position list does not fit the rows");
  const size_t n_positions = static_cast<size_t>(positions64), n_live = n - static_cast<size_t>(counters[kNearEmpty]);
  ns.n_elems = static_cast<int64_t>(elems64);
  ns.n_empty = static_cast<int64_t>(counters[kNearEmpty]);
  ns.n_shingles = static_cast<int64_t>(positions64);
  const uint32_t *d32 = static_cast<const uint32_t *>(in.d_data);

  // ---- signatures: flat over the positions ------------------------------------------------------------------------------
  if (n_positions != 0) {
    const unsigned tiles = cdiv(n_positions, kNearTile);
    switch ((plan.n_perm + kWave - 1) / kWave) {
      case 1: launch_near_sig<1>(tiles, st, d32, n_bytes, d_boff, d_pos_off, n, n_positions, plan, d_sig); break;
      case 2: launch_near_sig<2>(tiles, st, d32, n_bytes, d_boff, d_pos_off, n, n_positions, plan, d_sig); break;
      case 3: launch_near_sig<3>(tiles, st, d32, n_bytes, d_boff, d_pos_off, n, n_positions, plan, d_sig); break;
      default: launch_near_sig<4>(tiles, st, d32, n_bytes, d_boff, d_pos_off, n, n_positions, plan, d_sig); break;
    }
    WP_LAUNCH_CHECK();
  }
  if (timing) WP_HIP(hipEventRecord(c->ev[kMarkSymbols], st));

  // ---- band keys, one sort, heads, edges ----------------------------------------------------------------------------------
  const size_t m = n_live * plan.bands;  // (< 2^32: check_neardup_rows)
  const size_t tmp_words = radix_tmp_words<uint64_t>(m);
  Arena ia(&c->neardup_items, guard);
  uint64_t *d_k0 = nullptr, *d_k1 = nullptr;
  uint32_t *d_v0 = nullptr, *d_v1 = nullptr, *d_head = nullptr, *d_run = nullptr, *d_head_pos = nullptr, *d_edge = nullptr, *d_edge_pos = nullptr,
           *d_mrow = nullptr, *d_hrow = nullptr, *d_eu = nullptr, *d_ev = nullptr, *d_rtmp = nullptr, *d_itmp = nullptr;
  for (int pass = 0; pass < 2; pass++) {
    d_k0 = ia.take<uint64_t>(m);
    d_k1 = ia.take<uint64_t>(m);
    d_v0 = ia.take<uint32_t>(m);
    d_v1 = ia.take<uint32_t>(m);
    d_head = ia.take<uint32_t>(m + 1);
    d_run = ia.take<uint32_t>(m + 1);
    d_head_pos = ia.take<uint32_t>(m + 1);
    d_edge = ia.take<uint32_t>(m + 1);
    d_edge_pos = ia.take<uint32_t>(m + 1);
    d_mrow = ia.take<uint32_t>(m);
    d_hrow = ia.take<uint32_t>(m);
    d_eu = ia.take<uint32_t>(m);
    d_ev = ia.take<uint32_t>(m);
    d_rtmp = ia.take<uint32_t>(tmp_words);
    d_itmp = ia.take<uint32_t>(cdiv(m + 1, kScanTile) + 8);
    if (pass == 0) ia.commit();
  }
  ia.arm(st);
  size_t n_edges = 0;
  if (m != 0) {
    hipLaunchKernelGGL(near_band_keys_kernel, count_grid(m), dim3(kBlock), 0, st, static_cast<const uint32_t *>(d_sig),
                       static_cast<const uint32_t *>(d_rows), m, n, plan.n_perm, plan.bands, plan.seed, d_k0);
    const int cur = radix_sort_pairs<uint64_t>(d_k0, d_v0, d_k1, d_v1, m, 0, 64, d_rtmp, tmp_words, st, rs, true);
    const uint64_t *keys = cur ? d_k1 : d_k0;
    const uint32_t *vals = cur ? d_v1 : d_v0;
    uint32_t *d_runs = c->d_scalars + kScalarNearRuns;
    group_runs(keys, m, d_head, d_run, d_head_pos, d_itmp, d_runs, st);
    hipLaunchKernelGGL(near_match_kernel, count_grid(m), dim3(kBlock), 0, st, static_cast<const uint32_t *>(d_rows), vals,
                       static_cast<const uint32_t *>(d_head), static_cast<const uint32_t *>(d_run), static_cast<const uint32_t *>(d_head_pos), m, n,
                       plan.bands, d_edge, d_mrow, d_hrow, d_counters);
    // the candidates, compacted in sorted order: (d_eu, d_ev)
    device_exclusive_scan(d_edge, d_edge_pos, m, d_itmp, c->d_scalars + kScalarNearEdges, st);
    compact_flagged(d_edge, d_edge_pos, m, d_mrow, d_eu, st);
    compact_flagged(d_edge, d_edge_pos, m, d_hrow, d_ev, st);
    WP_LAUNCH_CHECK();
    queue_scalar_slots(c, kScalarNearRuns, kScalarNearEdges, st);
    WP_HIP(hipStreamSynchronize(st));
    const size_t n_cand = c->h_scalars[kScalarNearEdges];
    if (n_cand > m) throw HipError("neardup: more candidates than bucket members");
    ns.n_candidates = static_cast<int64_t>(n_cand);
    n_edges = n_cand;
    if (plan.min_agree != 0 && n_cand != 0) {  // the candidates that pass, compacted again: (d_mrow, d_hrow), free since the first compaction
      hipLaunchKernelGGL(near_agree_kernel, count_grid(n_cand * kNearEdgeLanes), dim3(kBlock), 0, st, static_cast<const uint32_t *>(d_sig),
                         static_cast<const uint32_t *>(d_eu), static_cast<const uint32_t *>(d_ev), n_cand, n, plan.n_perm, plan.min_agree, d_edge);
      device_exclusive_scan(d_edge, d_edge_pos, n_cand, d_itmp, c->d_scalars + kScalarNearEdges, st);
      compact_flagged(d_edge, d_edge_pos, n_cand, d_eu, d_mrow, st);
      compact_flagged(d_edge, d_edge_pos, n_cand, d_ev, d_hrow, st);
      WP_LAUNCH_CHECK();
      if (timing) WP_HIP(hipEventRecord(c->ev[kMarkSorted], st));
      queue_scalar_slots(c, kScalarNearEdges, kScalarNearEdges, st);
      WP_HIP(hipStreamSynchronize(st));
      n_edges = c->h_scalars[kScalarNearEdges];
      if (n_edges > n_cand) throw HipError("neardup: more edges than candidates");
      std::swap(d_eu, d_mrow);
      std::swap(d_ev, d_hrow);
    } else if (timing) {
      WP_HIP(hipEventRecord(c->ev[kMarkSorted], st));
    }
  } else if (timing) {
    WP_HIP(hipEventRecord(c->ev[kMarkSorted], st));
  }
  ns.n_edges = static_cast<int64_t>(n_edges);

  // ---- components: hook rounds over the edge list, pointer jumping behind each ------------------------------------------
  if (n_edges != 0) {
    const size_t cap = n + 1;  // (see above: at most n_rows rounds change a label, and one more sees none)
    for (;;) {
      if (static_cast<size_t>(ns.n_rounds) >= cap) throw InternalError("neardup: the component rounds did not end within n_rows + 1 rounds");
      clear_scalars(c, kScalarNearChanged, kScalarNearChanged, st);
      hipLaunchKernelGGL(near_hook_kernel, count_grid(n_edges), dim3(kBlock), 0, st, static_cast<const uint32_t *>(d_eu),
                         static_cast<const uint32_t *>(d_ev), n_edges, n, d_cluster, c->d_scalars + kScalarNearChanged);
      hipLaunchKernelGGL(near_jump_kernel, count_grid(n), dim3(kBlock), 0, st, d_cluster, n);
      WP_LAUNCH_CHECK();
      queue_scalar_slots(c, kScalarNearChanged, kScalarNearChanged, st);
      WP_HIP(hipStreamSynchronize(st));
      ns.n_rounds++;
      if (c->h_scalars[kScalarNearChanged] == 0) break;
    }
  }

  // ---- the kept rows and their sizes ----------------------------------------------------------------------------------------
  hipLaunchKernelGGL(near_sizes_kernel, count_grid(n), dim3(kBlock), 0, st, static_cast<const int32_t *>(d_cluster), n, d_rcount);
  hipLaunchKernelGGL(group_keep_kernel, count_grid(n1), dim3(kBlock), 0, st, static_cast<const int32_t *>(d_cluster), n, d_keep);
  device_exclusive_scan(d_keep, d_keep_pos, n1, d_stmp, c->d_scalars + kScalarNearUnique, st);
  WP_LAUNCH_CHECK();
  queue_scalar_slots(c, kScalarNearUnique, kScalarNearUnique, st);
  WP_HIP(hipStreamSynchronize(st));
  const size_t n_unique = c->h_scalars[kScalarNearUnique];
  if (n_unique == 0 || n_unique > n) throw HipError("neardup: the kept rows do not fit the rows");
  ns.n_unique = static_cast<int64_t>(n_unique);

  // ---- the table and the compact form: dedup's kernels over `cluster` ------------------------------------------------------
  const GroupTable t = group_table(c, in, d_cluster, d_keep_pos, d_rcount, d_boff, n_unique, n_bytes, plan.want_inverse, plan.want_compact, &c->neardup_out,
                                   guard, d_out_len, d_out_pos, d_stmp, kScalarNearOutBytes, st);
  WP_LAUNCH_CHECK();
  if (timing) WP_HIP(hipEventRecord(c->ev[kMarkWalked], st));
  queue_scalar_slots(c, kScalarNearOutBytes, kScalarNear, st);
  WP_HIP(hipStreamSynchronize(st));
  std::memcpy(counters, c->h_scalars + kScalarNear, sizeof(counters));
  ns.n_buckets = static_cast<int64_t>(counters[kNearBuckets]);
  if (timing) {  // wp_stats, as the header's section says: the stage times of this call in the fields an encode times itself in
    const float list = mark_ms(c, kMarkStart, kMarkCounted), sigs = mark_ms(c, kMarkCounted, kMarkSymbols), group = mark_ms(c, kMarkSymbols, kMarkSorted),
                table = mark_ms(c, kMarkSorted, kMarkWalked);
    v->stats.ms_normalize = 0;
    v->stats.ms_decode = list;
    v->stats.ms_scan = sigs;
    v->stats.ms_sa = group;
    v->stats.ms_walk = table;
    v->stats.ms_total = list + sigs + group + table;
    end_stage_timing(v, c);
  }
  throw_if_group_oob(kSiteNearDup, "near-duplicate rows", "gathers or stores outside the row, item or edge arrays skipped");
  check_arena_guard(c, ra, st, "neardup");
  check_arena_guard(c, ia, st, "neardup");
  check_arena_guard(c, t.oa, st, "neardup");
  R->cluster = d_cluster;
  if (plan.want_signatures) R->signatures = d_sig;
  t.hand_out(R, n_unique, plan.want_compact, c->h_scalars[kScalarNearOutBytes], eb);
}

}  // namespace wp
