// overlap_path.h — the n-gram overlap search on a context (include/wordpiece_amd.h, section "n-gram overlap"; kernels:
// overlap.h): the argument rules, the answer of a call without windows, the launches over two device batches and the
// buffers of a call.  Shared with repeat_path.h, in window_path.h: the intake, the window table, the kept rows.
#pragma once
#include <algorithm>

#include "context.h"
#include "overlap.h"
#include "window_path.h"

namespace wp {

// the spec of a call with its defaults filled in
struct OverlapPlan {
  uint32_t elem_bytes = 1, ngram = 13, max_hits = 0;
  int hash_bits = 64;
  bool want_mask = false, want_ref = false, want_compact = false;
};

// every rule of the spec, each with the field it is about; nothing here needs a device
static OverlapPlan check_overlap_spec(const wp_overlap_spec *spec, const wp_overlap_result *out) {
  if (!spec) throw std::invalid_argument("overlap: spec is NULL");
  if (!out) throw std::invalid_argument("overlap: out is NULL");
  check_elem_bytes("overlap", spec->elem_bytes);
  check_want("overlap", spec->want, WP_OVERLAP_WANT_MASK | WP_OVERLAP_WANT_REF | WP_OVERLAP_WANT_COMPACT);
  check_ngram("overlap", spec->ngram);
  if (spec->max_hits < 0) throw std::invalid_argument("overlap: max_hits must not be negative");
  const int hash_bits = checked_hash_bits("overlap", spec->hash_bits);
  for (int32_t r : spec->reserved) {
    if (r != 0) throw std::invalid_argument("overlap: reserved must be 0");
  }
  OverlapPlan p;
  p.elem_bytes = static_cast<uint32_t>(spec->elem_bytes);
  p.ngram = static_cast<uint32_t>(spec->ngram);
  p.max_hits = static_cast<uint32_t>(spec->max_hits);
  p.hash_bits = hash_bits;
  p.want_mask = (spec->want & WP_OVERLAP_WANT_MASK) != 0;
  p.want_ref = (spec->want & WP_OVERLAP_WANT_REF) != 0;
  p.want_compact = (spec->want & WP_OVERLAP_WANT_COMPACT) != 0;
  return p;
}

// the pointers and the row counts of both batches
static void check_overlap_rows(const void *row_off, size_t n_rows, const void *ref_off, size_t n_ref) {
  if (n_rows != 0 && !row_off) throw std::invalid_argument("overlap: row_off is NULL");
  if (n_ref != 0 && !ref_off) throw std::invalid_argument("overlap: ref_off is NULL");
  check_row_count("overlap", n_rows, " in row_off");
  check_row_count("overlap", n_ref, " in ref_off");
}

// the statistics of an overlap call before anything is known of its rows
static wp_overlap_stats &begin_overlap_stats(wp_vocab *v, size_t n_rows, size_t n_ref) {
  v->stats.overlap_call = 1;
  v->stats.overlap = wp_overlap_stats{};
  v->stats.overlap.n_rows = static_cast<int64_t>(n_rows);
  v->stats.overlap.n_ref = static_cast<int64_t>(n_ref);
  return v->stats.overlap;
}

// A host call whose corpus or whose reference set has no window (n_rows >= 1): no device needed.  Nothing hits; every
// row is kept.  The distinct reference windows, which the statistics state, are counted here by a sort.
static wp_overlap_result overlap_no_window(wp_vocab *v, const OverlapPlan &plan, const void *data, const int64_t *row_off, size_t n_rows,
                                           const void *ref_data, const int64_t *ref_off, size_t n_ref, unsigned long long n_windows,
                                           unsigned long long n_ref_windows) {
  wp_overlap_stats &os = begin_overlap_stats(v, n_rows, n_ref);
  const size_t n_elems = static_cast<size_t>(row_off[n_rows]), n_ref_elems = n_ref ? static_cast<size_t>(ref_off[n_ref]) : 0;
  os.n_elems = static_cast<int64_t>(n_elems);
  os.n_ref_elems = static_cast<int64_t>(n_ref_elems);
  os.n_windows = static_cast<int64_t>(n_windows);
  os.n_ref_windows = static_cast<int64_t>(n_ref_windows);
  if (n_ref_windows != 0) {
    const size_t wb = static_cast<size_t>(plan.ngram) * plan.elem_bytes;
    const uint8_t *rb = static_cast<const uint8_t *>(ref_data);
    std::vector<const uint8_t *> win;
    win.reserve(static_cast<size_t>(n_ref_windows));
    for (size_t r = 0; r < n_ref; r++) {
      for (int64_t p = ref_off[r]; p + static_cast<int64_t>(plan.ngram) <= ref_off[r + 1]; p++) win.push_back(rb + static_cast<size_t>(p) * plan.elem_bytes);
    }
    std::sort(win.begin(), win.end(), [wb](const uint8_t *a, const uint8_t *b) { return std::memcmp(a, b, wb) < 0; });
    os.n_ref_distinct = 1;
    for (size_t i = 1; i < win.size(); i++) os.n_ref_distinct += std::memcmp(win[i - 1], win[i], wb) != 0 ? 1 : 0;
  }
  wp_overlap_result h{};
  h.n_rows = static_cast<int64_t>(n_rows);
  h.n_ref = static_cast<int64_t>(n_ref);
  h.hits = static_cast<int64_t *>(zeroed(n_rows * sizeof(int64_t)));
  h.covered = static_cast<int64_t *>(zeroed(n_rows * sizeof(int64_t)));
  h.first_hit = static_cast<int64_t *>(zeroed(n_rows * sizeof(int64_t)));
  h.first_ref = static_cast<int32_t *>(zeroed(n_rows * sizeof(int32_t)));
  for (size_t r = 0; r < n_rows; r++) {
    h.first_hit[r] = -1;
    h.first_ref[r] = -1;
  }
  if (plan.want_mask && n_elems != 0) h.mask = static_cast<uint8_t *>(zeroed(n_elems));
  if (plan.want_ref && n_ref != 0) h.ref_hits = static_cast<int64_t *>(zeroed(n_ref * sizeof(int64_t)));
  if (plan.want_compact) {
    h.n_kept = static_cast<int64_t>(n_rows);
    h.n_elems = static_cast<int64_t>(n_elems);
    h.kept = static_cast<int32_t *>(zeroed(n_rows * sizeof(int32_t)));
    for (size_t r = 0; r < n_rows; r++) h.kept[r] = static_cast<int32_t>(r);
    h.row_off = static_cast<int64_t *>(zeroed((n_rows + 1) * sizeof(int64_t)));
    std::memcpy(h.row_off, row_off, (n_rows + 1) * sizeof(int64_t));
    if (n_elems != 0) {
      h.data = zeroed(n_elems * plan.elem_bytes);
      std::memcpy(h.data, data, n_elems * plan.elem_bytes);
    }
  }
  return h;
}

// The corpus `in` (n_rows >= 1) against the reference set `ref` (any number of rows), on c's stream.  The results are
// device pointers into c->overlap_rows (the per-row arrays), c->overlap_items (mask) and c->overlap_out (the compact
// form), valid until the handle's next call.  Waits: the sizes of both batches (the offset checks, the elements, the
// windows), the candidate count (with it the table size), with WP_OVERLAP_WANT_COMPACT the kept count, and the one that
// ends the call: three or four by the spec, whatever the data holds and however the keys collide.  The table needs no
// wait of its own: its arrays and its bucket index are sized by the reference windows, which the first wait brought.
static void overlap_on_device(wp_vocab *v, Context *c, const RaggedIn &in, const RaggedIn &ref, const OverlapPlan &plan, wp_overlap_result *R) {
  const size_t n = in.n_rows, nr = ref.n_rows;
  wp_overlap_stats &os = begin_overlap_stats(v, n, nr);
  *R = wp_overlap_result{};
  R->n_rows = static_cast<int64_t>(n);
  R->n_ref = static_cast<int64_t>(nr);
  hipStream_t st = c->stream;
  const bool guard = v->arena_guard || EnvOptions::get().arena_guard;
  const uint32_t eb = in.elem_bytes, k = plan.ngram;
  // WP_OPT_STAGE_TIMING: kMarkStart, kMarkCounted (offsets checked), kMarkSorted (the reference table is built),
  // kMarkScanned (corpus windows, lookup, comparison), kMarkWalked (per-row results, compact form)
  const bool timing = v->stage_timing;
  RadixStats *rs = begin_stage_timing(c, timing, st);

  // ---- the per-row arrays of both batches, the offset checks ---------------------------------------------------------------
  const size_t n1 = n + 1, nr1 = nr + 1;
  Arena ra(&c->overlap_rows, guard);
  uint32_t *d_boff = nullptr, *d_rboff = nullptr, *d_keep = nullptr, *d_keep_pos = nullptr, *d_out_len = nullptr, *d_out_pos = nullptr, *d_stmp = nullptr;
  long long *d_hits = nullptr, *d_first_hit = nullptr, *d_covered = nullptr, *d_ref_hits = nullptr;
  int32_t *d_first_ref = nullptr;
  for (int pass = 0; pass < 2; pass++) {
    d_boff = ra.take<uint32_t>(n1);
    d_rboff = ra.take<uint32_t>(nr1);
    d_hits = ra.take<long long>(n);
    d_first_hit = ra.take<long long>(n);
    d_covered = ra.take<long long>(n);
    d_first_ref = ra.take<int32_t>(n);
    if (plan.want_ref) d_ref_hits = ra.take<long long>(nr);
    d_keep = ra.take<uint32_t>(n1);
    d_keep_pos = ra.take<uint32_t>(n1);
    d_out_len = ra.take<uint32_t>(n1);
    d_out_pos = ra.take<uint32_t>(n1);
    d_stmp = ra.take<uint32_t>(cdiv(std::max(n1, nr1), kScanTile) + 8);
    if (pass == 0) ra.commit();
  }
  ra.arm(st);
  unsigned long long *d_counters = reinterpret_cast<unsigned long long *>(c->d_scalars + kScalarOvl);
  clear_scalars(c, kScalarOvlBad, kScalarOvl, st);
  WP_HIP(hipMemsetAsync(c->d_scalars + kScalarOvlBad, 0xff, 2 * sizeof(uint32_t), st));  // (both bad-row words)
  queue_window_rows(c, in, k, d_boff, kScalarOvlBad, kScalarOvlElems, kScalarOvlWindows, st);
  if (nr != 0) queue_window_rows(c, ref, k, d_rboff, kScalarOvlRefBad, kScalarOvlRefElems, kScalarOvlRefWindows, st);
  WP_LAUNCH_CHECK();
  if (timing) WP_HIP(hipEventRecord(c->ev[kMarkCounted], st));
  queue_scalar_slots(c, kScalarOvlBad, kScalarOvlRefWindows, st);
  WP_HIP(hipStreamSynchronize(st));
  const WindowSizes cs = read_window_rows(c, "overlap", in, kScalarOvlBad, kScalarOvlElems, kScalarOvlWindows);
  const WindowSizes fs = read_window_rows(c, "overlap", ref, kScalarOvlRefBad, kScalarOvlRefElems, kScalarOvlRefWindows, "ref_off", "ref_data");
  const size_t n_bytes = cs.n_bytes, n_ref_bytes = fs.n_bytes, ne = cs.n_elems, nre = fs.n_elems, nw = cs.n_windows, m = fs.n_windows;
  os.n_elems = static_cast<int64_t>(ne);
  os.n_ref_elems = static_cast<int64_t>(nre);
  os.n_windows = static_cast<int64_t>(nw);
  os.n_ref_windows = static_cast<int64_t>(m);
  const uint32_t *c32 = static_cast<const uint32_t *>(in.d_data), *r32 = static_cast<const uint32_t *>(ref.d_data);

  // ---- the per-element and per-window arrays -------------------------------------------------------------------------------
  // (without reference windows there is no table, and without windows on either side no lookup: the results then follow
  // from hit flags that are all zero)
  const bool table = m != 0, search = table && nw != 0;
  const int hb = plan.hash_bits;
  int bb = 1;  // the bits of a bucket number: about one reference window per bucket, within the narrowed key
  while (bb < kOvlMaxBucketBits && bb < hb && (size_t(1) << bb) < m) bb++;
  const size_t n_buckets = size_t(1) << bb;
  const uint32_t shift = static_cast<uint32_t>(hb - bb);
  const uint64_t mask = hb >= 64 ? ~0ull : (1ull << hb) - 1ull;
  const size_t ne1 = ne + 1, nre1 = nre + 1, m1 = m + 1;
  Arena ia(&c->overlap_items, guard);
  WindowTable t;  // of the reference set
  uint32_t *d_flag = nullptr, *d_scan = nullptr, *d_ent = nullptr, *d_ce = nullptr, *d_ct = nullptr, *d_hit = nullptr, *d_H = nullptr, *d_ent_of = nullptr,
           *d_ent_pos = nullptr, *d_ent_hit = nullptr, *d_bucket = nullptr, *d_itmp = nullptr;
  uint64_t *d_ent_key = nullptr;
  uint8_t *d_mask = nullptr;
  for (int pass = 0; pass < 2; pass++) {
    d_flag = ia.take<uint32_t>(ne1);   // the candidate flags, then the cover flags
    d_scan = ia.take<uint32_t>(ne1);   // their scans
    d_ent = ia.take<uint32_t>(ne);     // the entry of a candidate, then of a hit
    d_ce = ia.take<uint32_t>(ne);      // the candidates, compacted: position and entry
    d_ct = ia.take<uint32_t>(ne);
    d_hit = ia.take<uint32_t>(ne1);
    d_H = ia.take<uint32_t>(ne1);
    if (plan.want_mask) d_mask = ia.take<uint8_t>(ne);
    t.take(ia, nre, m);
    d_ent_of = ia.take<uint32_t>(m);
    d_ent_key = ia.take<uint64_t>(m);
    d_ent_pos = ia.take<uint32_t>(m);
    d_ent_hit = ia.take<uint32_t>(m);
    d_bucket = ia.take<uint32_t>(2 * n_buckets);
    d_itmp = ia.take<uint32_t>(cdiv(std::max(std::max(ne1, nre1), m1), kScanTile) + 8);
    if (pass == 0) ia.commit();
  }
  ia.arm(st);
  WP_HIP(hipMemsetAsync(d_hit, 0, ne1 * sizeof(uint32_t), st));
  uint32_t *d_n_ent = c->d_scalars + kScalarOvlEntries;

  // ---- the reference table: the window table of the reference set, its entries, the bucket index ----------------------------
  if (table) {
    t.list(ref, nre, d_rboff, k, mask, false, d_itmp, nullptr, st);
    t.group(ref, nre, n_ref_bytes, m, k, hb, d_itmp, c->d_scalars + kScalarOvlRuns, d_counters, d_n_ent, rs, st);
    hipLaunchKernelGGL(ovl_table_kernel, count_grid(m), dim3(kBlock), 0, st, t.keys, t.vals, t.d_rep, t.entry_pos(), m, d_ent_of, d_ent_key, d_ent_pos,
                       d_ent_hit);
    WP_HIP(hipMemsetAsync(d_bucket, 0, 2 * n_buckets * sizeof(uint32_t), st));
    hipLaunchKernelGGL(ovl_bucket_kernel, count_grid(m), dim3(kBlock), 0, st, d_ent_key, d_n_ent, m, shift, n_buckets, d_bucket);
    WP_LAUNCH_CHECK();
  }
  if (timing) WP_HIP(hipEventRecord(c->ev[kMarkSorted], st));

  // ---- the corpus windows: keys and lookup in one kernel, the candidates compacted and compared ----------------------------
  if (search) {
    hipLaunchKernelGGL(ovl_keys_kernel, dim3(cdiv(ne, kOvlTile)), dim3(kBlock), 0, st, c32, ne, d_boff, n, eb, k, overlap_powers(k), mask,
                       nullptr, d_flag, d_ent_key, d_n_ent, d_bucket, shift, n_buckets, d_ent, 0u);
    device_exclusive_scan(d_flag, d_scan, ne, d_itmp, c->d_scalars + kScalarOvlCands, st);
    compact_flagged(d_flag, d_scan, ne, nullptr, d_ce, st);
    compact_flagged(d_flag, d_scan, ne, d_ent, d_ct, st);
    WP_LAUNCH_CHECK();
  }
  queue_scalar_slots(c, kScalarOvlRuns, kScalarOvlCands, st);
  WP_HIP(hipStreamSynchronize(st));
  const size_t n_entries = c->h_scalars[kScalarOvlEntries], n_cand = c->h_scalars[kScalarOvlCands];
  if (n_entries > m || n_cand > nw || (table && n_entries == 0)) throw HipError("overlap: the table or the candidates do not fit the windows");
  os.n_ref_distinct = static_cast<int64_t>(n_entries);
  os.n_candidates = static_cast<int64_t>(n_cand);
  if (n_cand != 0) {
    hipLaunchKernelGGL(ovl_verify_kernel, count_grid(n_cand * kOvlLanes), dim3(kBlock), 0, st, c32, n_bytes, r32, n_ref_bytes, d_ce, d_ct,
                       n_cand, d_ent_key, d_ent_pos, d_n_ent, m, eb, k, d_hit, d_ent, d_ent_hit);
    WP_LAUNCH_CHECK();
  }
  if (timing) WP_HIP(hipEventRecord(c->ev[kMarkScanned], st));

  // ---- the per-row results: scans of the hit and cover flags, differences at the row ends ----------------------------------
  device_exclusive_scan(d_hit, d_H, ne1, d_itmp, c->d_scalars + kScalarOvlHits, st);
  WP_HIP(hipMemsetAsync(d_first_hit, 0xff, n * sizeof(long long), st));  // (-1)
  WP_HIP(hipMemsetAsync(d_first_ref, 0xff, n * sizeof(int32_t), st));
  WP_HIP(hipMemsetAsync(d_flag + ne, 0, sizeof(uint32_t), st));  // (a batch without elements: the cover kernel does not run)
  if (ne != 0) {
    hipLaunchKernelGGL(ovl_cover_kernel, count_grid(ne), dim3(kBlock), 0, st, d_hit, d_H, d_ent, d_ent_pos, m, d_boff, n, d_rboff, nr, ne, eb, k, d_flag,
                       d_mask, d_first_hit, d_first_ref);
  }
  device_exclusive_scan(d_flag, d_scan, ne1, d_itmp, c->d_scalars + kScalarOvlCovered, st);
  hipLaunchKernelGGL(ovl_row_results_kernel, count_grid(n1), dim3(kBlock), 0, st, d_H, d_scan, d_boff, n, eb, plan.max_hits, d_hits, d_covered, d_keep,
                     d_counters);
  if (plan.want_ref && nr != 0) {
    uint32_t *d_rhit = t.d_valid, *d_R = t.d_vpos;  // (the window flags are listed: their arrays are free)
    WP_HIP(hipMemsetAsync(d_rhit, 0, nre1 * sizeof(uint32_t), st));
    if (table) hipLaunchKernelGGL(ovl_ref_mark_kernel, count_grid(m), dim3(kBlock), 0, st, t.vals, d_ent_of, d_ent_hit, m, nre, d_rhit);
    device_exclusive_scan(d_rhit, d_R, nre1, d_itmp, nullptr, st);
    hipLaunchKernelGGL(ovl_ref_rows_kernel, count_grid(nr), dim3(kBlock), 0, st, d_R, d_rboff, nr, eb, d_ref_hits);
  }
  WP_LAUNCH_CHECK();

  // ---- the compact form of the kept rows -------------------------------------------------------------------------------------
  Arena oa(&c->overlap_out, guard);
  KeptRows kept;
  if (plan.want_compact) {
    kept.count(c, "overlap", d_keep, d_keep_pos, n, d_stmp, kScalarOvlKept, st);
    for (int pass = 0; pass < 2; pass++) {
      kept.take(oa, n_bytes);
      if (pass == 0) oa.commit();
    }
    oa.arm(st);
    kept.queue(c, in, d_keep, d_keep_pos, d_boff, n_bytes, d_out_len, d_out_pos, d_stmp, kScalarOvlOutBytes, st);
    WP_LAUNCH_CHECK();
  }
  if (timing) WP_HIP(hipEventRecord(c->ev[kMarkWalked], st));
  queue_scalar_slots(c, kScalarOvlHits, kScalarOvl, st);
  WP_HIP(hipStreamSynchronize(st));
  unsigned long long counters[kOvlCounters];
  std::memcpy(counters, c->h_scalars + kScalarOvl, sizeof(counters));
  os.n_hits = static_cast<int64_t>(c->h_scalars[kScalarOvlHits]);
  os.n_covered = static_cast<int64_t>(c->h_scalars[kScalarOvlCovered]);
  os.n_hit_rows = static_cast<int64_t>(counters[kOvlHitRows]);
  os.n_collided = static_cast<int64_t>(counters[kOvlCollided]);
  if (timing) end_four_stage_timing(v, c);  // (check, table, lookup, rows: the header's section)
  throw_if_group_oob(kSiteOverlap, "n-gram overlap", "gathers or stores outside the window, table, candidate or result arrays skipped");
  check_arena_guard(c, ra, st, "overlap");
  check_arena_guard(c, ia, st, "overlap");
  check_arena_guard(c, oa, st, "overlap");
  R->hits = reinterpret_cast<int64_t *>(d_hits);
  R->first_hit = reinterpret_cast<int64_t *>(d_first_hit);
  R->covered = reinterpret_cast<int64_t *>(d_covered);
  R->first_ref = d_first_ref;
  if (plan.want_mask && ne != 0) R->mask = d_mask;
  if (plan.want_ref && nr != 0) R->ref_hits = reinterpret_cast<int64_t *>(d_ref_hits);
  if (plan.want_compact) kept.hand_out(R, c->h_scalars[kScalarOvlOutBytes], eb);
}

}  // namespace wp
