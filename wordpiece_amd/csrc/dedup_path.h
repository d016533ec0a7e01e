// dedup_path.h — duplicate rows on a context (include/wordpiece_amd.h, section "duplicate rows"; kernels: dedup.h): the
// argument rules, the launches over a device batch, the rounds of the grouping and the buffers of a call.
#pragma once
#include "context.h"
#include "count_path.h"  // count_grid, check_count_guard
#include "dedup.h"

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
  if (spec->elem_bytes != 1 && spec->elem_bytes != 4) throw std::invalid_argument("dedup: elem_bytes must be 1 or 4");
  if ((spec->want & ~(WP_DEDUP_WANT_INVERSE | WP_DEDUP_WANT_COMPACT)) != 0) throw std::invalid_argument("dedup: want has bits outside 3");
  if (spec->hash_bits != 0 && (spec->hash_bits < 8 || spec->hash_bits > 64)) throw std::invalid_argument("dedup: hash_bits must be 0 (64) or in [8, 64]");
  if (spec->reserved != 0) throw std::invalid_argument("dedup: reserved must be 0");
  DedupPlan p;
  p.elem_bytes = static_cast<uint32_t>(spec->elem_bytes);
  p.hash_bits = spec->hash_bits == 0 ? 64 : spec->hash_bits;
  p.want_inverse = (spec->want & WP_DEDUP_WANT_INVERSE) != 0;
  p.want_compact = (spec->want & WP_DEDUP_WANT_COMPACT) != 0;
  return p;
}

static void check_dedup_rows(size_t n_rows) {
  if (n_rows >= (size_t(1) << 31)) throw std::length_error("dedup: 2^31 rows or more");
}
static void check_dedup_bytes(unsigned long long n_elems, uint32_t elem_bytes) {
  if (n_elems > static_cast<unsigned long long>(UINT32_MAX) / elem_bytes) throw std::length_error("dedup: the data has more than UINT32_MAX bytes");
}

// the statistics of a dedup call before anything is known of its rows
static wp_dedup_stats &begin_dedup_stats(wp_vocab *v, size_t n_rows) {
  v->stats.dedup_call = 1;
  v->stats.dedup = wp_dedup_stats{};
  v->stats.dedup.n_rows = static_cast<int64_t>(n_rows);
  return v->stats.dedup;
}

// The rows of the batch at d_data / d_row_off (n_rows >= 1), on c's stream.  The results are device pointers into
// c->dedup_rows (first) and c->dedup_out (everything else), valid until the handle's next call.  Waits: the sizes (the
// offset check, the elements, the chunks), one per round, and the one that ends the call (it brings the size of the
// compact form, whose room was the size of the input).
static void dedup_on_device(wp_vocab *v, Context *c, const void *d_data, const long long *d_row_off, size_t n, const DedupPlan &plan,
                            wp_dedup_result *R) {
  wp_dedup_stats &ds = begin_dedup_stats(v, n);
  *R = wp_dedup_result{};
  R->n_rows = static_cast<int64_t>(n);
  hipStream_t st = c->stream;
  const bool guard = v->arena_guard || EnvOptions::get().arena_guard;
  const uint32_t eb = plan.elem_bytes;
  // WP_OPT_STAGE_TIMING: the marks of a dedup call are kMarkStart, kMarkCounted (offsets checked, chunks listed),
  // kMarkSorted (the rounds are over) and kMarkWalked (the table and the compact form are written)
  const bool timing = v->stage_timing;
  RadixStats *rs = timing ? &c->rstats : nullptr;
  if (timing) {
    c->rstats.passes = 0;
    c->rstats.elems = 0;
    c->rstats.digit_bytes = 0;
    c->rstats.bytes = 0;
    c->rstats.spans.used = 0;
    c->rstats.spans.on = true;
    WP_HIP(hipEventRecord(c->ev[kMarkStart], st));
  }

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
  hipLaunchKernelGGL(dedup_rows_kernel, count_grid(n1), dim3(kBlock), 0, st, d_row_off, n, eb, d_boff, d_nch, d_items0, d_first,
                     c->d_scalars + kScalarDedupBad, d_elems, d_counters);
  device_exclusive_scan(d_nch, d_choff0, n1, d_stmp, nullptr, st, nullptr, d_chunks);
  WP_LAUNCH_CHECK();
  if (timing) WP_HIP(hipEventRecord(c->ev[kMarkCounted], st));
  queue_scalar_slots(c, kScalarDedupBad, kScalarDedup, st);
  WP_HIP(hipStreamSynchronize(st));
  const uint32_t bad = c->h_scalars[kScalarDedupBad];
  if (bad != kDedupNoBad) {
    throw std::invalid_argument(bad == 0 ? "dedup: row_off must start at 0 and never descend: row 0"
                                         : "dedup: row_off must never descend: row " + std::to_string(bad));
  }
  unsigned long long elems64, chunks64, counters[kDedupCounters];
  std::memcpy(&elems64, c->h_scalars + kScalarDedupElems, sizeof(elems64));
  std::memcpy(&chunks64, c->h_scalars + kScalarDedupChunks, sizeof(chunks64));
  std::memcpy(counters, c->h_scalars + kScalarDedup, sizeof(counters));
  check_dedup_bytes(elems64, eb);
  const size_t n_bytes = static_cast<size_t>(elems64) * eb;
  if (n_bytes != 0 && !d_data) throw std::invalid_argument("dedup: data is NULL");
  ds.n_elems = static_cast<int64_t>(elems64);
  ds.n_empty = static_cast<int64_t>(counters[kDedupEmpty]);
  ds.n_chunks = static_cast<int64_t>(chunks64);
  const uint32_t *d32 = static_cast<const uint32_t *>(d_data);

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
    hipLaunchKernelGGL(count_heads_kernel, count_grid(m), dim3(kBlock), 0, st, keys, m, d_head);
    device_exclusive_scan(d_head, d_run, m, d_stmp, d_runs, st);
    hipLaunchKernelGGL(count_head_pos_kernel, count_grid(m), dim3(kBlock), 0, st, d_head, d_run, m, d_runs, d_head_pos);
    hipLaunchKernelGGL(dedup_match_kernel, count_grid(m), dim3(kBlock), 0, st, items, vals, d_head, d_run, d_head_pos, m, n, d_boff, d_head_row, d_left);
    if (mc != 0) {
      hipLaunchKernelGGL(dedup_compare_kernel, count_grid(mc), dim3(kBlock), 0, st, d32, n_bytes, d_boff, items, choff, d_head_row, m, mc, n, d_left,
                         d_counters + kDedupCompared);
    }
    hipLaunchKernelGGL(dedup_settle_kernel, count_grid(m), dim3(kBlock), 0, st, items, vals, d_head_row, d_left, m, n, d_agree, d_first);
    device_exclusive_scan(d_agree, d_agree_pos, m + 1, d_stmp, nullptr, st);
    hipLaunchKernelGGL(dedup_run_counts_kernel, count_grid(m), dim3(kBlock), 0, st, items, vals, d_head_pos, d_agree_pos, d_runs, m, n, d_rcount);
    device_exclusive_scan(d_left, d_left_pos, m, d_stmp, d_nleft, st);
    hipLaunchKernelGGL(count_compact_kernel, count_grid(m), dim3(kBlock), 0, st, d_left, d_left_pos, m, static_cast<const uint32_t *>(items), next, m);
    // the chunk list of the next round: the chunks of its items, scanned
    hipLaunchKernelGGL(dedup_item_chunks_kernel, count_grid(m + 1), dim3(kBlock), 0, st, next, d_nleft, m, d_nch, n, d_icnt);
    device_exclusive_scan(d_icnt, choff_next, m + 1, d_stmp, nullptr, st, nullptr, d_chunks);
    WP_LAUNCH_CHECK();
    queue_scalar_slots(c, kScalarDedupRuns, kScalarDedupLeft, st);
    WP_HIP(hipStreamSynchronize(st));
    const size_t runs = c->h_scalars[kScalarDedupRuns], left = c->h_scalars[kScalarDedupLeft];
    if (runs == 0 || left >= m) throw HipError("dedup: a round settled no row");  // (every run settles its head)
    std::memcpy(&chunks64, c->h_scalars + kScalarDedupChunks, sizeof(chunks64));
    n_unique += runs;
    if (ds.n_rounds == 0) ds.n_collided = static_cast<int64_t>(left);
    ds.n_rounds++;
    m = left;
    mc = static_cast<size_t>(chunks64);
    std::swap(items, next);
    std::swap(choff, choff_next);
  }
  if (timing) WP_HIP(hipEventRecord(c->ev[kMarkSorted], st));
  ds.n_unique = static_cast<int64_t>(n_unique);

  // ---- the table and the compact form ----------------------------------------------------------------------------------
  Arena oa(&c->dedup_out, guard);
  int32_t *d_kept = nullptr, *d_inverse = nullptr;
  long long *d_counts = nullptr, *d_out_off = nullptr;
  uint32_t *d_out = nullptr;
  for (int pass = 0; pass < 2; pass++) {
    d_kept = oa.take<int32_t>(n_unique);
    d_counts = oa.take<long long>(n_unique);
    if (plan.want_inverse) d_inverse = oa.take<int32_t>(n);
    if (plan.want_compact) {
      d_out_off = oa.take<long long>(n_unique + 1);
      d_out = oa.take<uint32_t>(n_bytes / 4 + 1);
    }
    if (pass == 0) oa.commit();
  }
  oa.arm(st);
  uint32_t *d_keep = d_head, *d_keep_pos = d_run, *d_out_len = d_agree, *d_out_pos = d_agree_pos;  // (the rounds are over)
  hipLaunchKernelGGL(dedup_keep_kernel, count_grid(n1), dim3(kBlock), 0, st, d_first, n, d_keep);
  device_exclusive_scan(d_keep, d_keep_pos, n1, d_stmp, c->d_scalars + kScalarDedupUnique, st);
  hipLaunchKernelGGL(dedup_table_kernel, count_grid(n), dim3(kBlock), 0, st, d_first, d_keep_pos, d_rcount, d_boff, n, n_unique, d_kept, d_counts,
                     d_inverse, plan.want_compact ? d_out_len : static_cast<uint32_t *>(nullptr));
  if (plan.want_compact) {
    device_exclusive_scan(d_out_len, d_out_pos, n_unique + 1, d_stmp, nullptr, st);
    hipLaunchKernelGGL(dedup_out_off_kernel, count_grid(n_unique + 1), dim3(kBlock), 0, st, d_out_pos, n_unique, eb, d_out_off);
    if (n_bytes != 0) {
      hipLaunchKernelGGL(dedup_gather_kernel, count_grid((n_bytes + 3) / 4), dim3(kBlock), 0, st, static_cast<const uint8_t *>(d_data), n_bytes, d_boff,
                         d_kept, d_out_pos, n_unique, n, n_bytes, d_out);
    }
    // (the size of the compact form: the last entry of its offsets, through the word the round totals came in)
    WP_HIP(hipMemcpyAsync(c->d_scalars + kScalarDedupLeft, d_out_pos + n_unique, sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
  }
  WP_LAUNCH_CHECK();
  if (timing) WP_HIP(hipEventRecord(c->ev[kMarkWalked], st));
  queue_scalar_slots(c, kScalarDedupLeft, kScalarDedup, st);
  WP_HIP(hipStreamSynchronize(st));
  std::memcpy(counters, c->h_scalars + kScalarDedup, sizeof(counters));
  ds.n_compared = static_cast<int64_t>(counters[kDedupCompared] / eb);
  if (c->h_scalars[kScalarDedupUnique] != n_unique) throw HipError("dedup: the kept rows are not the heads of the rounds");
  if (timing) {  // wp_stats, as the header's section says: the stage times of this call in the fields a count call uses
    float list = 0, rounds = 0, table = 0;
    WP_HIP(hipEventElapsedTime(&list, c->ev[kMarkStart], c->ev[kMarkCounted]));
    WP_HIP(hipEventElapsedTime(&rounds, c->ev[kMarkCounted], c->ev[kMarkSorted]));
    WP_HIP(hipEventElapsedTime(&table, c->ev[kMarkSorted], c->ev[kMarkWalked]));
    v->stats.ms_normalize = 0;
    v->stats.ms_decode = list;
    v->stats.ms_sa = rounds;
    v->stats.ms_walk = table;
    v->stats.ms_total = list + rounds + table;
    v->stats.ms_radix_scatter = c->rstats.spans.resolve();
    v->stats.radix_passes = c->rstats.passes;
    v->stats.radix_pass_elems = c->rstats.elems;
    v->stats.radix_pass_bytes = c->rstats.bytes;
    c->rstats.spans.on = false;
  }
  throw_if_oob(kSiteDedup, "duplicate rows", "stores or gathers outside the row, chunk or table arrays skipped");
  check_count_guard(c, ra, st, "dedup");
  check_count_guard(c, oa, st, "dedup");
  R->first = d_first;
  R->kept = d_kept;
  R->counts = reinterpret_cast<int64_t *>(d_counts);
  R->inverse = d_inverse;
  R->n_unique = static_cast<int64_t>(n_unique);
  if (plan.want_compact) {
    const size_t out_bytes = c->h_scalars[kScalarDedupLeft];
    R->row_off = reinterpret_cast<int64_t *>(d_out_off);
    R->data = out_bytes ? d_out : nullptr;
    R->n_elems = static_cast<int64_t>(out_bytes / eb);
  }
}

}  // namespace wp
