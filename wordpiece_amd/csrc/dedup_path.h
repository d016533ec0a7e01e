// dedup_path.h — duplicate rows on a context (include/wordpiece_amd.h, section "duplicate rows"; kernels: dedup.h): the
// argument rules, the launches over a device batch, the rounds of the grouping and the buffers of a call.
#pragma once
#include "context.h"
#include "dedup.h"
#include "group_path.h"

namespace wp {

// the spec of a call with its defaults filled in
struct DedupPlan {
  uint32_t elem_bytes = 1;
  int hash_bits = 64;
  bool want_inverse = false, want_compact = false;
};

// every rule of the spec, each with the field it is about; nothing here needs a device
static DedupPlan check_dedup_spec(const wp_dedup_spec *spec, const wp_dedup_result *out) {
  if (!spec) throw std::invalid_argument("dedup: spec is NULL");
  if (!out) throw std::invalid_argument("dedup: out is NULL");
  check_elem_bytes("dedup", spec->elem_bytes);
  check_want("dedup", spec->want, WP_DEDUP_WANT_INVERSE | WP_DEDUP_WANT_COMPACT);
  const int hash_bits = checked_hash_bits("dedup", spec->hash_bits);
  if (spec->reserved != 0) throw std::invalid_argument("dedup: reserved must be 0");
  DedupPlan p;
  p.elem_bytes = static_cast<uint32_t>(spec->elem_bytes);
  p.hash_bits = hash_bits;
  p.want_inverse = (spec->want & WP_DEDUP_WANT_INVERSE) != 0;
  p.want_compact = (spec->want & WP_DEDUP_WANT_COMPACT) != 0;
  return p;
}

// the statistics of a dedup call before anything is known of its rows
static wp_dedup_stats &begin_dedup_stats(wp_vocab *v, size_t n_rows) {
  v->stats.dedup_call = 1;
  v->stats.dedup = wp_dedup_stats{};
  v->stats.dedup.n_rows = static_cast<int64_t>(n_rows);
  return v->stats.dedup;
}

// no row, or rows that are all empty and so all equal to row 0: no device needed
static wp_dedup_result dedup_all_empty(wp_vocab *v, size_t n_rows, const DedupPlan &plan) {
  wp_dedup_stats &ds = begin_dedup_stats(v, n_rows);
  wp_dedup_result h{};
  h.n_rows = static_cast<int64_t>(n_rows);
  if (plan.want_compact) h.row_off = static_cast<int64_t *>(zeroed((n_rows ? 2 : 1) * sizeof(int64_t)));
  if (n_rows == 0) return h;
  ds.n_unique = 1;
  ds.n_empty = static_cast<int64_t>(n_rows);
  h.n_unique = 1;
  h.first = static_cast<int32_t *>(zeroed(n_rows * sizeof(int32_t)));
  h.kept = static_cast<int32_t *>(zeroed(sizeof(int32_t)));
  h.counts = static_cast<int64_t *>(zeroed(sizeof(int64_t)));
  h.counts[0] = static_cast<int64_t>(n_rows);
  if (plan.want_inverse) h.inverse = static_cast<int32_t *>(zeroed(n_rows * sizeof(int32_t)));
  return h;
}

// The rows of the batch `in` (n_rows >= 1), on c's stream.  The results are device pointers into
// c->dedup_rows (first) and c->dedup_out (everything else), valid until the handle's next call.  Waits: the sizes (the
// offset check, the elements, the chunks), one per round, and the one that ends the call (it brings the size of the
// compact form, whose room was the size of the input).
static void dedup_on_device(wp_vocab *v, Context *c, const RaggedIn &in, const DedupPlan &plan, wp_dedup_result *R) {
  const size_t n = in.n_rows;
  wp_dedup_stats &ds = begin_dedup_stats(v, n);
  *R = wp_dedup_result{};
  R->n_rows = static_cast<int64_t>(n);
  hipStream_t st = c->stream;
  const bool guard = v->arena_guard || EnvOptions::get().arena_guard;
  const uint32_t eb = in.elem_bytes;
  // WP_OPT_STAGE_TIMING: the marks of a dedup call are kMarkStart, kMarkCounted (offsets checked, chunks listed),
  // kMarkSorted (the rounds are over) and kMarkWalked (the table and the compact form are written)
  const bool timing = v->stage_timing;
  RadixStats *rs = begin_stage_timing(c, timing, st);

  // ---- the per-row arrays, the offset check, the chunk list -------------------------------------------------------
  const size_t n1 = n + 1;
  const size_t tmp_words = radix_tmp_words<uint64_t>(n);
  Arena ra(&c->dedup_rows, guard);
  uint32_t *d_boff = nullptr, *d_nch = nullptr, *d_choff0 = nullptr, *d_choff1 = nullptr, *d_icnt = nullptr, *d_items0 = nullptr, *d_items1 = nullptr,
           *d_head_row = nullptr, *d_rcount = nullptr, *d_head = nullptr, *d_run = nullptr, *d_head_pos = nullptr, *d_agree = nullptr,
           *d_agree_pos = nullptr, *d_left = nullptr, *d_left_pos = nullptr, *d_v0 = nullptr, *d_v1 = nullptr, *d_rtmp = nullptr, *d_stmp = nullptr;
  int32_t *d_first = nullptr;
  uint64_t *d_k0 = nullptr, *d_k1 = nullptr;
  for (int pass = 0; pass < 2; pass++) {
    d_boff = ra.take<uint32_t>(n1);
    d_nch = ra.take<uint32_t>(n1);
    d_choff0 = ra.take<uint32_t>(n1);
    d_choff1 = ra.take<uint32_t>(n1);
    d_icnt = ra.take<uint32_t>(n1);
    d_items0 = ra.take<uint32_t>(n);
    d_items1 = ra.take<uint32_t>(n);
    d_first = ra.take<int32_t>(n);
    d_head_row = ra.take<uint32_t>(n);
    d_rcount = ra.take<uint32_t>(n);
    d_head = ra.take<uint32_t>(n1);
    d_run = ra.take<uint32_t>(n1);
    d_head_pos = ra.take<uint32_t>(n1);
    d_agree = ra.take<uint32_t>(n1);
    d_agree_pos = ra.take<uint32_t>(n1);
    d_left = ra.take<uint32_t>(n1);
    d_left_pos = ra.take<uint32_t>(n1);
    d_k0 = ra.take<uint64_t>(n);
    d_k1 = ra.take<uint64_t>(n);
    d_v0 = ra.take<uint32_t>(n);
    d_v1 = ra.take<uint32_t>(n);
    d_rtmp = ra.take<uint32_t>(tmp_words);
    d_stmp = ra.take<uint32_t>(cdiv(n1, kScanTile) + 8);
    if (pass == 0) ra.commit();
  }
  ra.arm(st);
  unsigned long long *d_counters = reinterpret_cast<unsigned long long *>(c->d_scalars + kScalarDedup);
  unsigned long long *d_elems = reinterpret_cast<unsigned long long *>(c->d_scalars + kScalarDedupElems);
  unsigned long long *d_chunks = reinterpret_cast<unsigned long long *>(c->d_scalars + kScalarDedupChunks);
  clear_scalars(c, kScalarDedupBad, kScalarDedup, st);
  WP_HIP(hipMemsetAsync(c->d_scalars + kScalarDedupBad, 0xff, sizeof(uint32_t), st));
  hipLaunchKernelGGL(dedup_rows_kernel, count_grid(n1), dim3(kBlock), 0, st, in.d_row_off, n, eb, d_boff, d_nch, d_items0, d_first,
                     c->d_scalars + kScalarDedupBad, d_elems, d_counters);
  device_exclusive_scan(d_nch, d_choff0, n1, d_stmp, nullptr, st, nullptr, d_chunks);
  WP_LAUNCH_CHECK();
  if (timing) WP_HIP(hipEventRecord(c->ev[kMarkCounted], st));
  queue_scalar_slots(c, kScalarDedupBad, kScalarDedup, st);
  WP_HIP(hipStreamSynchronize(st));
  unsigned long long elems64, chunks64, counters[kDedupCounters];
  std::memcpy(&elems64, c->h_scalars + kScalarDedupElems, sizeof(elems64));
  std::memcpy(&chunks64, c->h_scalars + kScalarDedupChunks, sizeof(chunks64));
  std::memcpy(counters, c->h_scalars + kScalarDedup, sizeof(counters));
  const size_t n_bytes = check_ragged_device("dedup", in, c->h_scalars[kScalarDedupBad], elems64);
  ds.n_elems = static_cast<int64_t>(elems64);
  ds.n_empty = static_cast<int64_t>(counters[kDedupEmpty]);
  ds.n_chunks = static_cast<int64_t>(chunks64);
  const uint32_t *d32 = static_cast<const uint32_t *>(in.d_data);

  // ---- the rounds: chunk hashes summed per row, sort, compare with the head of the run, leftovers on ------------------
  const uint64_t mask = plan.hash_bits >= 64 ? ~0ull : (1ull << plan.hash_bits) - 1ull;
  size_t m = n, mc = static_cast<size_t>(chunks64), n_unique = 0;  // (mc < 2^32: dedup.h, dedup_keys_kernel)
  uint32_t *items = d_items0, *next = d_items1, *choff = d_choff0, *choff_next = d_choff1;
  while (m != 0) {
    const uint64_t seed = static_cast<uint64_t>(ds.n_rounds);
    hipLaunchKernelGGL(dedup_key_init_kernel, count_grid(m), dim3(kBlock), 0, st, items, m, d_boff, n, seed, d_k0);
    if (mc != 0) {
      hipLaunchKernelGGL(dedup_keys_kernel, count_grid(mc), dim3(kBlock), 0, st, d32, n_bytes, d_boff, items, choff, m, mc, n, seed,
                         reinterpret_cast<unsigned long long *>(d_k0));
    }
    if (mask != ~0ull) hipLaunchKernelGGL(dedup_mask_kernel, count_grid(m), dim3(kBlock), 0, st, d_k0, m, mask);
    const int cur = radix_sort_pairs<uint64_t>(d_k0, d_v0, d_k1, d_v1, m, 0, plan.hash_bits, d_rtmp, tmp_words, st, rs, true);
    const uint64_t *keys = cur ? d_k1 : d_k0;
    const uint32_t *vals = cur ? d_v1 : d_v0;
    uint32_t *d_runs = c->d_scalars + kScalarDedupRuns, *d_nleft = c->d_scalars + kScalarDedupLeft;
    group_runs(keys, m, d_head, d_run, d_head_pos, d_stmp, d_runs, st);
    hipLaunchKernelGGL(dedup_match_kernel, count_grid(m), dim3(kBlock), 0, st, items, vals, d_head, d_run, d_head_pos, m, n, d_boff, d_head_row, d_left);
    if (mc != 0) {
      hipLaunchKernelGGL(dedup_compare_kernel, count_grid(mc), dim3(kBlock), 0, st, d32, n_bytes, d_boff, items, choff, d_head_row, m, mc, n, d_left,
                         d_counters + kDedupCompared);
    }
    hipLaunchKernelGGL(dedup_settle_kernel, count_grid(m), dim3(kBlock), 0, st, items, vals, d_head_row, d_left, m, n, d_agree, d_first);
    device_exclusive_scan(d_agree, d_agree_pos, m + 1, d_stmp, nullptr, st);
    hipLaunchKernelGGL(dedup_run_counts_kernel, count_grid(m), dim3(kBlock), 0, st, items, vals, d_head_pos, d_agree_pos, d_runs, m, n, d_rcount);
    carry_leftovers(d_left, d_left_pos, m, items, next, d_stmp, d_nleft, st);
    // the chunk list of the next round: the chunks of its items, scanned
    hipLaunchKernelGGL(dedup_item_chunks_kernel, count_grid(m + 1), dim3(kBlock), 0, st, next, d_nleft, m, d_nch, n, d_icnt);
    device_exclusive_scan(d_icnt, choff_next, m + 1, d_stmp, nullptr, st, nullptr, d_chunks);
    // (the slots from the runs through the leftovers hold the chunks as well: one wait)
    n_unique += end_round(c, kScalarDedupRuns, kScalarDedupLeft, "dedup", "row", &m, &ds, st);
    std::memcpy(&chunks64, c->h_scalars + kScalarDedupChunks, sizeof(chunks64));
    mc = static_cast<size_t>(chunks64);
    std::swap(items, next);
    std::swap(choff, choff_next);
  }
  if (timing) WP_HIP(hipEventRecord(c->ev[kMarkSorted], st));
  ds.n_unique = static_cast<int64_t>(n_unique);

  // ---- the table and the compact form ----------------------------------------------------------------------------------
  uint32_t *d_keep = d_head, *d_keep_pos = d_run, *d_out_len = d_agree, *d_out_pos = d_agree_pos;  // (the rounds are over)
  hipLaunchKernelGGL(group_keep_kernel, count_grid(n1), dim3(kBlock), 0, st, d_first, n, d_keep);
  device_exclusive_scan(d_keep, d_keep_pos, n1, d_stmp, c->d_scalars + kScalarDedupUnique, st);
  // (the size of the compact form comes through the word the round totals came in)
  const GroupTable t = group_table(c, in, d_first, d_keep_pos, d_rcount, d_boff, n_unique, n_bytes, plan.want_inverse, plan.want_compact, &c->dedup_out, guard,
                                   d_out_len, d_out_pos, d_stmp, kScalarDedupLeft, st);
  WP_LAUNCH_CHECK();
  if (timing) WP_HIP(hipEventRecord(c->ev[kMarkWalked], st));
  queue_scalar_slots(c, kScalarDedupLeft, kScalarDedup, st);
  WP_HIP(hipStreamSynchronize(st));
  std::memcpy(counters, c->h_scalars + kScalarDedup, sizeof(counters));
  ds.n_compared = static_cast<int64_t>(counters[kDedupCompared] / eb);
  if (c->h_scalars[kScalarDedupUnique] != n_unique) throw HipError("dedup: the kept rows are not the heads of the rounds");
  if (timing) {  // wp_stats, as the header's section says: the stage times of this call in the fields a count call uses
    const float list = mark_ms(c, kMarkStart, kMarkCounted), rounds = mark_ms(c, kMarkCounted, kMarkSorted), table = mark_ms(c, kMarkSorted, kMarkWalked);
    v->stats.ms_normalize = 0;
    v->stats.ms_decode = list;
    v->stats.ms_sa = rounds;
    v->stats.ms_walk = table;
    v->stats.ms_total = list + rounds + table;
    end_stage_timing(v, c);
  }
  throw_if_group_oob(kSiteDedup, "duplicate rows", "stores or gathers outside the row, chunk or table arrays skipped");
  check_arena_guard(c, ra, st, "dedup");
  check_arena_guard(c, t.oa, st, "dedup");
  R->first = d_first;
  t.hand_out(R, n_unique, plan.want_compact, c->h_scalars[kScalarDedupLeft], eb);
}

}  // namespace wp
