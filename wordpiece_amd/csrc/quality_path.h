// quality_path.h — the quality signals on a context (include/wordpiece_amd.h, section "quality signals"; kernels:
// quality.h): the argument rules, the answer of a call without bytes, the launches over one device batch and the buffers
// of a call.  The intake and the kept rows are window_path.h's, the duplicate-line stage runs dedup_path.h's search over
// the lines.
#pragma once
#include <algorithm>
#include <vector>

#include "context.h"
#include "dedup_path.h"
#include "quality.h"
#include "window_path.h"

namespace wp {

// the spec of a call with its defaults filled in
struct QualityPlan {
  bool want_dup = false, want_compact = false;
  uint32_t short_chars = 30, n_stop = 0;
  QualLimits lim{};
  std::vector<uint32_t> stop;  // the stop table as the word pass reads it (quality.h)
};

// every rule of the spec, each with the field it is about; nothing here needs a device
static QualityPlan check_quality_spec(const wp_quality_spec *spec, const wp_quality_result *out) {
  if (!spec) throw std::invalid_argument("quality: spec is NULL");
  if (!out) throw std::invalid_argument("quality: out is NULL");
  if (spec->elem_bytes != 1) throw std::invalid_argument("quality: elem_bytes must be 1");
  check_want("quality", spec->want, WP_QUALITY_WANT_DUP_LINES | WP_QUALITY_WANT_COMPACT);
  if (spec->short_line_chars < 0) throw std::invalid_argument("quality: short_line_chars must not be negative");
  QualityPlan p;
  p.want_dup = (spec->want & WP_QUALITY_WANT_DUP_LINES) != 0;
  p.want_compact = (spec->want & WP_QUALITY_WANT_COMPACT) != 0;
  p.short_chars = spec->short_line_chars == 0 ? 30u : static_cast<uint32_t>(spec->short_line_chars);
  for (int r = 0; r < WP_QUALITY_RULES; r++) {
    const int64_t L = spec->limit[r];
    const std::string name = "quality: limit[" + std::to_string(r) + "]";
    if (L != -1 && (L < 0 || L > 1000000000)) throw std::invalid_argument(name + " must be -1 or in [0, 10^9]");
    if (r == WP_QR_RESERVED && L != -1) throw std::invalid_argument(name + " is reserved and must be -1");
    if ((r == WP_QR_MAX_DUP_LINES || r == WP_QR_MAX_DUP_LINE_CHARS) && L != -1 && !p.want_dup) {
      throw std::invalid_argument(name + " needs WP_QUALITY_WANT_DUP_LINES");
    }
    p.lim.v[r] = L;
  }
  if (spec->n_stop_words < 0 || spec->n_stop_words > kQualMaxStop) throw std::invalid_argument("quality: n_stop_words must be in [0, 64]");
  p.n_stop = static_cast<uint32_t>(spec->n_stop_words);
  if (p.n_stop != 0) {
    if (!spec->stop_pool) throw std::invalid_argument("quality: stop_pool is NULL");
    if (!spec->stop_off) throw std::invalid_argument("quality: stop_off is NULL");
    if (spec->stop_off[0] != 0) throw std::invalid_argument("quality: stop_off must start at 0");
    const uint8_t *pool = static_cast<const uint8_t *>(spec->stop_pool);
    p.stop.assign(static_cast<size_t>(p.n_stop) * kQualStopWords, 0u);
    for (uint32_t t = 0; t < p.n_stop; t++) {
      const int64_t a = spec->stop_off[t], len = spec->stop_off[t + 1] - a;
      if (len < 1 || len > kQualMaxStopBytes) throw std::invalid_argument("quality: stop_off: word " + std::to_string(t) + " must have 1 to 32 bytes");
      uint32_t *q = p.stop.data() + static_cast<size_t>(t) * kQualStopWords;
      q[0] = static_cast<uint32_t>(len);
      for (int64_t i = 0; i < len; i++) {
        const uint32_t b = pool[a + i];
        if (b >= 'A' && b <= 'Z') throw std::invalid_argument("quality: stop_pool: word " + std::to_string(t) + " holds ASCII upper case");
        q[1 + i / 4] |= b << (8u * static_cast<uint32_t>(i % 4));
      }
    }
  }
  if (spec->reserved != 0) throw std::invalid_argument("quality: reserved must be 0");
  return p;
}

// the pointer and the row count of the batch
static void check_quality_rows(const void *row_off, size_t n_rows) {
  if (n_rows != 0 && !row_off) throw std::invalid_argument("quality: row_off is NULL");
  check_row_count("quality", n_rows, " in row_off");
}

// the statistics of a quality call before anything is known of its rows
static wp_quality_stats &begin_quality_stats(wp_vocab *v, size_t n_rows) {
  v->stats.quality_call = 1;
  v->stats.quality = wp_quality_stats{};
  v->stats.quality.n_rows = static_cast<int64_t>(n_rows);
  return v->stats.quality;
}

// A host call whose batch has no byte (n_rows >= 1): no device needed.  Every signal is 0 and the reasons are the rules
// over zeros, the same for every row.
static wp_quality_result quality_no_bytes(wp_vocab *v, const QualityPlan &plan, size_t n_rows) {
  wp_quality_stats &qs = begin_quality_stats(v, n_rows);
  const long long zeros[WP_QUALITY_SIGNALS] = {};
  const uint32_t reasons = quality_reasons(zeros, plan.lim);
  wp_quality_result h{};
  h.n_rows = static_cast<int64_t>(n_rows);
  h.signals = static_cast<int64_t *>(zeroed(n_rows * WP_QUALITY_SIGNALS * sizeof(int64_t)));
  h.reasons = static_cast<uint32_t *>(zeroed(n_rows * sizeof(uint32_t)));
  std::fill(h.reasons, h.reasons + n_rows, reasons);
  const size_t n_kept = reasons == 0 ? n_rows : 0;
  qs.n_kept = static_cast<int64_t>(n_kept);
  for (int r = 0; r < WP_QUALITY_RULES; r++) qs.rule_failed[r] = (reasons >> r) & 1u ? static_cast<int64_t>(n_rows) : 0;
  if (plan.want_compact) {
    h.n_kept = static_cast<int64_t>(n_kept);
    if (n_kept != 0) {
      h.kept = static_cast<int32_t *>(zeroed(n_kept * sizeof(int32_t)));
      for (size_t r = 0; r < n_kept; r++) h.kept[r] = static_cast<int32_t>(r);
    }
    h.row_off = static_cast<int64_t *>(zeroed((n_kept + 1) * sizeof(int64_t)));
  }
  return h;
}

// the class table of quality.h on the device of c, uploaded once per context
static void ensure_class_table(Context *c, hipStream_t st) {
  if (c->d_class_index) return;
  uint8_t *pages = nullptr;
  uint16_t *index = nullptr;
  WP_HIP(hipMalloc(&pages, sizeof(kClassPageData)));
  if (hipMalloc(&index, sizeof(kClassIndex)) != hipSuccess) {  // (neither is kept: the next call starts over)
    (void)hipFree(pages);
    throw HipError("quality: no device memory for the class table");
  }
  c->d_class_pages = pages;
  c->d_class_index = index;
  WP_HIP(hipMemcpyAsync(c->d_class_pages, kClassPageData, sizeof(kClassPageData), hipMemcpyHostToDevice, st));
  WP_HIP(hipMemcpyAsync(c->d_class_index, kClassIndex, sizeof(kClassIndex), hipMemcpyHostToDevice, st));
}

// what a quality call borrows from the handle while the duplicate-row search runs inside it, put back when the scope
// ends: the statistics of the dedup layer and the handle's stage timing (the quality call times itself)
struct BorrowedDedup {
  wp_vocab *v;
  wp_dedup_stats stats;
  int32_t call;
  bool timing;
  explicit BorrowedDedup(wp_vocab *v_) : v(v_), stats(v_->stats.dedup), call(v_->stats.dedup_call), timing(v_->stage_timing) { v->stage_timing = false; }
  ~BorrowedDedup() {
    v->stats.dedup = stats;
    v->stats.dedup_call = call;
    v->stage_timing = timing;
  }
  BorrowedDedup(const BorrowedDedup &) = delete;
  BorrowedDedup &operator=(const BorrowedDedup &) = delete;
};

// The batch `in` (n_rows >= 1), on c's stream.  The results are device pointers into c->quality_rows (signals, reasons)
// and c->quality_out (the compact form), valid until the handle's next call.  Waits: the header's section lists them.
// Per-row totals: per-tile partial sums combined by 64-bit integer atomics (quality.h).
static void quality_on_device(wp_vocab *v, Context *c, const RaggedIn &in, const QualityPlan &plan, wp_quality_result *R) {
  const size_t n = in.n_rows;
  wp_quality_stats &qs = begin_quality_stats(v, n);
  *R = wp_quality_result{};
  R->n_rows = static_cast<int64_t>(n);
  hipStream_t st = c->stream;
  const bool guard = v->arena_guard || EnvOptions::get().arena_guard;
  // WP_OPT_STAGE_TIMING: kMarkStart, kMarkCounted (offsets checked), kMarkSorted (class passes, word pass, line pass),
  // kMarkScanned (duplicate lines), kMarkWalked (rules, compact form)
  const bool timing = v->stage_timing;
  RadixStats *rs = begin_stage_timing(c, timing, st);

  // ---- the per-row arrays, the offset check --------------------------------------------------------------------------------
  const size_t n1 = n + 1;
  Arena ra(&c->quality_rows, guard);
  uint32_t *d_boff = nullptr, *d_reasons = nullptr, *d_keep = nullptr, *d_keep_pos = nullptr, *d_out_len = nullptr, *d_out_pos = nullptr, *d_stmp = nullptr;
  long long *d_sig = nullptr;
  for (int pass = 0; pass < 2; pass++) {
    d_boff = ra.take<uint32_t>(n1);
    d_sig = ra.take<long long>(n * WP_QUALITY_SIGNALS);
    d_reasons = ra.take<uint32_t>(n);
    d_keep = ra.take<uint32_t>(n1);
    d_keep_pos = ra.take<uint32_t>(n1);
    d_out_len = ra.take<uint32_t>(n1);
    d_out_pos = ra.take<uint32_t>(n1);
    d_stmp = ra.take<uint32_t>(cdiv(n1, kScanTile) + 8);
    if (pass == 0) ra.commit();
  }
  ra.arm(st);
  unsigned long long *d_counters = reinterpret_cast<unsigned long long *>(c->d_scalars + kScalarQual);
  unsigned long long *d_usig = reinterpret_cast<unsigned long long *>(d_sig);
  clear_scalars(c, kScalarQualBad, kScalarQual, st);
  WP_HIP(hipMemsetAsync(c->d_scalars + kScalarQualBad, 0xff, sizeof(uint32_t), st));
  WP_HIP(hipMemsetAsync(d_sig, 0, n * WP_QUALITY_SIGNALS * sizeof(long long), st));
  queue_window_rows(c, in, 1, d_boff, kScalarQualBad, kScalarQualElems, kScalarQualWindows, st);
  WP_LAUNCH_CHECK();
  if (timing) WP_HIP(hipEventRecord(c->ev[kMarkCounted], st));
  queue_scalar_slots(c, kScalarQualBad, kScalarQualWindows, st);
  WP_HIP(hipStreamSynchronize(st));
  const size_t nb = read_window_rows(c, "quality", in, kScalarQualBad, kScalarQualElems, kScalarQualWindows).n_bytes;
  qs.n_bytes = static_cast<int64_t>(nb);
  const uint8_t *d_text = static_cast<const uint8_t *>(in.d_data);

  // ---- the class pass: counts and per-character signals, the scan of the tile counts, the lists ------------------------------
  const size_t n_tiles = cdiv(nb, kQualTile), nt1 = n_tiles + 1, n_counts = kQualKinds * nt1;
  Arena ia(&c->quality_items, guard);
  uint32_t *d_tiles = nullptr, *d_ttmp = nullptr, *d_stop = nullptr;
  for (int pass = 0; pass < 2; pass++) {
    d_tiles = ia.take<uint32_t>(n_counts);
    d_ttmp = ia.take<uint32_t>(cdiv(n_counts, kScanTile) + 8);
    d_stop = ia.take<uint32_t>(static_cast<size_t>(kQualMaxStop) * kQualStopWords);
    if (pass == 0) ia.commit();
  }
  ia.arm(st);
  size_t nw = 0, nl = 0;
  QualLists lists{};
  if (nb != 0) {
    ensure_class_table(c, st);
    if (plan.n_stop != 0) WP_HIP(hipMemcpyAsync(d_stop, plan.stop.data(), plan.stop.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    WP_HIP(hipMemsetAsync(d_tiles, 0, n_counts * sizeof(uint32_t), st));
    hipLaunchKernelGGL(qual_class_kernel<false>, dim3(n_tiles), dim3(kBlock), 0, st, d_text, nb, d_boff, n, c->d_class_index, c->d_class_pages, d_tiles, nt1, d_usig,
                       lists);
    device_exclusive_scan(d_tiles, d_tiles, n_counts, d_ttmp, nullptr, st);
    hipLaunchKernelGGL(qual_totals_kernel, dim3(1), dim3(kWave), 0, st, d_tiles, nt1, c->d_scalars + kScalarQualWords, c->d_scalars + kScalarQualLines);
    WP_LAUNCH_CHECK();
    queue_scalar_slots(c, kScalarQualWords, kScalarQualLines, st);
    WP_HIP(hipStreamSynchronize(st));
    nw = c->h_scalars[kScalarQualWords];
    nl = c->h_scalars[kScalarQualLines];
    if (nw > nb || nl > nb) throw HipError("quality: the starts and the ends of the words or lines do not pair up");
  }
  if (plan.want_dup && nl >= (size_t(1) << 30)) throw std::length_error("quality: 2^30 lines or more with WP_QUALITY_WANT_DUP_LINES");
  const bool dup = plan.want_dup && nl != 0;
  const size_t dup_rows = 2 * nl + 1, tmp_words = radix_tmp_words<uint64_t>(nl);
  Arena la(&c->quality_lists, guard);
  uint32_t *d_lchars = nullptr, *d_v0 = nullptr, *d_v1 = nullptr, *d_head = nullptr, *d_rtmp = nullptr;
  uint64_t *d_k0 = nullptr, *d_k1 = nullptr;
  long long *d_dup_off = nullptr;
  for (int pass = 0; pass < 2; pass++) {
    lists.wstart = la.take<uint32_t>(nw);
    lists.wrow = la.take<uint32_t>(nw);
    lists.wa0 = la.take<uint32_t>(nw);
    lists.wend = la.take<uint32_t>(nw);
    lists.wa1 = la.take<uint32_t>(nw);
    lists.lstart = la.take<uint32_t>(nl);
    lists.lrow = la.take<uint32_t>(nl);
    lists.lc0 = la.take<uint32_t>(nl);
    lists.lend = la.take<uint32_t>(nl);
    lists.lc1 = la.take<uint32_t>(nl);
    d_lchars = la.take<uint32_t>(nl);
    if (dup) {
      d_dup_off = la.take<long long>(dup_rows + 1);
      d_k0 = la.take<uint64_t>(nl);
      d_k1 = la.take<uint64_t>(nl);
      d_v0 = la.take<uint32_t>(nl);
      d_v1 = la.take<uint32_t>(nl);
      d_head = la.take<uint32_t>(nl + 1);
      d_rtmp = la.take<uint32_t>(tmp_words);
    }
    if (pass == 0) la.commit();
  }
  la.arm(st);
  lists.n_words = nw;
  lists.n_lines = nl;
  if (nb != 0) {
    hipLaunchKernelGGL(qual_class_kernel<true>, dim3(n_tiles), dim3(kBlock), 0, st, d_text, nb, d_boff, n, c->d_class_index, c->d_class_pages, d_tiles, nt1, d_usig,
                       lists);
    if (nw != 0) hipLaunchKernelGGL(qual_words_kernel, count_grid(nw), dim3(kBlock), 0, st, d_text, nb, lists, n, d_stop, plan.n_stop, d_usig);
    if (nl != 0) hipLaunchKernelGGL(qual_lines_kernel, count_grid(nl), dim3(kBlock), 0, st, d_text, nb, lists, n, plan.short_chars, d_usig, d_lchars, d_dup_off);
    WP_LAUNCH_CHECK();
  }
  if (timing) WP_HIP(hipEventRecord(c->ev[kMarkSorted], st));

  // ---- duplicate lines: the duplicate-row search over the lines, one sort of (row, first row with the same bytes) -------------
  if (dup) {
    wp_dedup_result first{};
    {
      BorrowedDedup borrowed(v);
      dedup_on_device(v, c, RaggedIn{in.d_data, d_dup_off, dup_rows, 1}, DedupPlan{}, &first);
    }
    const int id_bits = bit_length(dup_rows), row_bits = std::max(1, bit_length(n - 1));
    hipLaunchKernelGGL(qual_dup_keys_kernel, count_grid(nl), dim3(kBlock), 0, st, lists.lrow, first.first, nl, id_bits, d_k0);
    const int cur = radix_sort_pairs<uint64_t>(d_k0, d_v0, d_k1, d_v1, nl, 0, id_bits + row_bits, d_rtmp, tmp_words, st, rs, true);
    hipLaunchKernelGGL(group_heads_kernel, count_grid(nl), dim3(kBlock), 0, st, static_cast<const uint64_t *>(cur ? d_k1 : d_k0), nl, d_head);
    hipLaunchKernelGGL(qual_dup_kernel, count_grid(nl), dim3(kBlock), 0, st, static_cast<const uint32_t *>(cur ? d_v1 : d_v0), static_cast<const uint32_t *>(d_head),
                       nl, lists.lrow, d_lchars, n, d_usig);
    WP_LAUNCH_CHECK();
  }
  if (timing) WP_HIP(hipEventRecord(c->ev[kMarkScanned], st));

  // ---- the rules, the kept rows, the compact form -----------------------------------------------------------------------------
  hipLaunchKernelGGL(qual_rules_kernel, count_grid(n1), dim3(kBlock), 0, st, d_boff, n, plan.lim, d_sig, d_reasons, d_keep, d_counters);
  WP_LAUNCH_CHECK();
  KeptRows kept;
  Arena oa(&c->quality_out, guard);
  if (plan.want_compact) {
    kept.count(c, "quality", d_keep, d_keep_pos, n, d_stmp, kScalarQualKept, st);
    for (int pass = 0; pass < 2; pass++) {
      kept.take(oa, nb);
      if (pass == 0) oa.commit();
    }
    oa.arm(st);
    kept.queue(c, in, d_keep, d_keep_pos, d_boff, nb, d_out_len, d_out_pos, d_stmp, kScalarQualOutBytes, st);
    WP_LAUNCH_CHECK();
  } else {
    device_exclusive_scan(d_keep, d_keep_pos, n1, d_stmp, c->d_scalars + kScalarQualKept, st);
  }
  if (timing) WP_HIP(hipEventRecord(c->ev[kMarkWalked], st));
  queue_scalar_slots(c, kScalarQualKept, kScalarQual, st);
  WP_HIP(hipStreamSynchronize(st));
  unsigned long long counters[kQualCounters];
  std::memcpy(counters, c->h_scalars + kScalarQual, sizeof(counters));
  qs.n_chars = static_cast<int64_t>(counters[kQualChars]);
  qs.n_invalid = static_cast<int64_t>(counters[kQualInvalid]);
  qs.n_words = static_cast<int64_t>(counters[kQualWordsTotal]);
  qs.n_lines = static_cast<int64_t>(counters[kQualLinesTotal]);
  qs.n_dup_lines = static_cast<int64_t>(counters[kQualDupLines]);
  qs.n_kept = static_cast<int64_t>(c->h_scalars[kScalarQualKept]);
  for (int r = 0; r < WP_QUALITY_RULES; r++) qs.rule_failed[r] = static_cast<int64_t>(counters[kQualRuleFailed + r]);
  if (static_cast<size_t>(qs.n_words) != nw || static_cast<size_t>(qs.n_lines) != nl) throw HipError("quality: the rows do not sum to the words and lines of the text");
  if (timing) end_four_stage_timing(v, c);  // (check, signals, duplicate lines, rules: the header's section)
  // (kSiteOverlap: the row kernel and the kept rows of overlap.h run here too)
  throw_if_group_oob(kSiteQuality, "quality signals", "gathers or stores outside the tile, word, line or signal arrays skipped", kSiteOverlap,
                     "gathers or stores outside the row arrays skipped");
  check_arena_guard(c, ra, st, "quality");
  check_arena_guard(c, ia, st, "quality");
  check_arena_guard(c, la, st, "quality");
  check_arena_guard(c, oa, st, "quality");
  R->signals = reinterpret_cast<int64_t *>(d_sig);
  R->reasons = d_reasons;
  if (plan.want_compact) kept.hand_out(R, c->h_scalars[kScalarQualOutBytes], 1);
}

}  // namespace wp
