// repetition_path.h — the repetition signals on a context (include/wordpiece_amd_repetition.h; kernels: repetition.h):
// the argument rules, the answer of a call without bytes, the launches over one device batch and the buffers of a call.
// The intake and the kept rows are window_path.h's, the class passes and the word list quality.h's, and the word
// identities come from dedup_path.h's search over the words.
#pragma once
#include <algorithm>
#include <vector>

#include "context.h"
#include "dedup_path.h"
#include "quality_path.h"
#include "repetition.h"
#include "window_path.h"

namespace wp {

struct RepetitionPlan {
  bool want_compact = false;
  RptLimits lim{};
};

// every rule of the spec, each with the field it is about; nothing here needs a device
static RepetitionPlan check_repetition_spec(const wp_repetition_spec *spec, const wp_repetition_result *out) {
  if (!spec) throw std::invalid_argument("repetition: spec is NULL");
  if (!out) throw std::invalid_argument("repetition: out is NULL");
  if (spec->elem_bytes != 1) throw std::invalid_argument("repetition: elem_bytes must be 1");
  check_want("repetition", spec->want, WP_RPT_WANT_COMPACT);
  RepetitionPlan p;
  p.want_compact = (spec->want & WP_RPT_WANT_COMPACT) != 0;
  for (int k = 0; k < WP_RPT_RULES; k++) {
    const int64_t L = spec->limit[k];
    if (L < -1 || L > 1000) throw std::invalid_argument("repetition: limit[" + std::to_string(k) + "] must be -1 or in [0, 1000]");
    p.lim.v[k] = L;
  }
  if (spec->reserved != 0) throw std::invalid_argument("repetition: reserved must be 0");
  return p;
}

static void check_repetition_rows(const void *row_off, size_t n_rows) {
  if (n_rows != 0 && !row_off) throw std::invalid_argument("repetition: row_off is NULL");
  check_row_count("repetition", n_rows, " in row_off");
}

static wp_repetition_stats &begin_repetition_stats(wp_vocab *v, size_t n_rows) {
  v->stats.repetition_call = 1;
  v->stats.repetition = wp_repetition_stats{};
  v->stats.repetition.n_rows = static_cast<int64_t>(n_rows);
  return v->stats.repetition;
}

// A host call whose batch has no byte (n_rows >= 1): no device needed.  Every signal is 0 and the reasons are the rules
// over zeros, the same for every row.
static wp_repetition_result repetition_no_bytes(wp_vocab *v, const RepetitionPlan &plan, size_t n_rows) {
  wp_repetition_stats &ps = begin_repetition_stats(v, n_rows);
  const long long zeros[WP_RPT_SIGNALS] = {};
  const uint32_t reasons = repetition_reasons(zeros, plan.lim);
  wp_repetition_result h{};
  h.n_rows = static_cast<int64_t>(n_rows);
  h.signals = static_cast<int64_t *>(zeroed(n_rows * WP_RPT_SIGNALS * sizeof(int64_t)));
  h.reasons = static_cast<uint32_t *>(zeroed(n_rows * sizeof(uint32_t)));
  std::fill(h.reasons, h.reasons + n_rows, reasons);
  const size_t n_kept = reasons == 0 ? n_rows : 0;
  ps.n_kept = static_cast<int64_t>(n_kept);
  for (int k = 0; k < WP_RPT_RULES; k++) ps.rule_failed[k] = (reasons >> k) & 1u ? static_cast<int64_t>(n_rows) : 0;
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

// The batch `in` (n_rows >= 1), on c's stream.  The results are device pointers into c->repetition_rows (signals,
// reasons) and c->repetition_out (the compact form), valid until the handle's next call.  Waits: the sizes, the numbers
// of words and lines, those of the duplicate-row search over the words, with the compact form the kept count, and the
// one that ends the call.
static void repetition_on_device(wp_vocab *v, Context *c, const RaggedIn &in, const RepetitionPlan &plan, wp_repetition_result *R) {
  const size_t n = in.n_rows;
  wp_repetition_stats &ps = begin_repetition_stats(v, n);
  *R = wp_repetition_result{};
  R->n_rows = static_cast<int64_t>(n);
  hipStream_t st = c->stream;
  const bool guard = v->arena_guard || EnvOptions::get().arena_guard;
  // WP_OPT_STAGE_TIMING: kMarkStart, kMarkCounted (intake, class passes, word list, word identity), kMarkSorted (the
  // five sorts), kMarkScanned (the LCP and the run passes), kMarkWalked (cover, rules, compact form)
  const bool timing = v->stage_timing;
  RadixStats *rs = begin_stage_timing(c, timing, st);

  // ---- the per-row arrays, the offset check --------------------------------------------------------------------------------
  const size_t n1 = n + 1;
  Arena ra(&c->repetition_rows, guard);
  uint32_t *d_boff = nullptr, *d_reasons = nullptr, *d_keep = nullptr, *d_keep_pos = nullptr, *d_out_len = nullptr, *d_out_pos = nullptr, *d_stmp = nullptr;
  long long *d_sig = nullptr;
  unsigned long long *d_top = nullptr, *d_qsig = nullptr;
  for (int pass = 0; pass < 2; pass++) {
    d_boff = ra.take<uint32_t>(n1);
    d_sig = ra.take<long long>(n * WP_RPT_SIGNALS);
    d_top = ra.take<unsigned long long>(n * kRptGroup);
    d_qsig = ra.take<unsigned long long>(n * WP_QUALITY_SIGNALS);  // what the class pass sums beside its counts: not read
    d_reasons = ra.take<uint32_t>(n);
    d_keep = ra.take<uint32_t>(n1);
    d_keep_pos = ra.take<uint32_t>(n1);
    d_out_len = ra.take<uint32_t>(n1);
    d_out_pos = ra.take<uint32_t>(n1);
    d_stmp = ra.take<uint32_t>(cdiv(n1, kScanTile) + 8);
    if (pass == 0) ra.commit();
  }
  ra.arm(st);
  unsigned long long *d_counters = reinterpret_cast<unsigned long long *>(c->d_scalars + kScalarRpt);
  unsigned long long *d_usig = reinterpret_cast<unsigned long long *>(d_sig);
  clear_scalars(c, kScalarRptBad, kScalarRpt, st);
  WP_HIP(hipMemsetAsync(c->d_scalars + kScalarRptBad, 0xff, sizeof(uint32_t), st));
  WP_HIP(hipMemsetAsync(d_sig, 0, n * WP_RPT_SIGNALS * sizeof(long long), st));
  WP_HIP(hipMemsetAsync(d_top, 0, n * kRptGroup * sizeof(unsigned long long), st));
  WP_HIP(hipMemsetAsync(d_qsig, 0, n * WP_QUALITY_SIGNALS * sizeof(unsigned long long), st));
  queue_window_rows(c, in, 1, d_boff, kScalarRptBad, kScalarRptElems, kScalarRptWindows, st);
  WP_LAUNCH_CHECK();
  queue_scalar_slots(c, kScalarRptBad, kScalarRptWindows, st);
  WP_HIP(hipStreamSynchronize(st));
  const size_t nb = read_window_rows(c, "repetition", in, kScalarRptBad, kScalarRptElems, kScalarRptWindows).n_bytes;
  ps.n_bytes = static_cast<int64_t>(nb);
  const uint8_t *d_text = static_cast<const uint8_t *>(in.d_data);

  // ---- the class pass of quality.h: counts, the scan of the tile counts, the numbers of words and lines ----------------------
  const size_t n_tiles = cdiv(nb, kQualTile), nt1 = n_tiles + 1, n_counts = kQualKinds * nt1;
  Arena ia(&c->repetition_items, guard);
  uint32_t *d_tiles = nullptr, *d_ttmp = nullptr;
  for (int pass = 0; pass < 2; pass++) {
    d_tiles = ia.take<uint32_t>(n_counts);
    d_ttmp = ia.take<uint32_t>(cdiv(n_counts, kScanTile) + 8);
    if (pass == 0) ia.commit();
  }
  ia.arm(st);
  size_t nw = 0, nl = 0;
  QualLists lists{};
  if (nb != 0) {
    ensure_class_table(c, st);
    WP_HIP(hipMemsetAsync(d_tiles, 0, n_counts * sizeof(uint32_t), st));
    hipLaunchKernelGGL(qual_class_kernel<false>, dim3(n_tiles), dim3(kBlock), 0, st, d_text, nb, d_boff, n, c->d_class_index, c->d_class_pages, d_tiles, nt1, d_qsig,
                       lists);
    device_exclusive_scan(d_tiles, d_tiles, n_counts, d_ttmp, nullptr, st);
    hipLaunchKernelGGL(qual_totals_kernel, dim3(1), dim3(kWave), 0, st, d_tiles, nt1, c->d_scalars + kScalarRptWords, c->d_scalars + kScalarRptLines);
    WP_LAUNCH_CHECK();
    queue_scalar_slots(c, kScalarRptWords, kScalarRptLines, st);
    WP_HIP(hipStreamSynchronize(st));
    nw = c->h_scalars[kScalarRptWords];
    nl = c->h_scalars[kScalarRptLines];
    if (nw > nb || nl > nb) throw HipError("repetition: the starts and the ends of the words or lines do not pair up");
  }
  if (nw >= (size_t(1) << 30)) throw std::length_error("repetition: 2^30 words or more");

  // ---- the per-word arrays ---------------------------------------------------------------------------------------------------
  const size_t nw1 = nw + 1, dup_rows = 2 * nw + 1, tmp_words = radix_tmp_words<uint64_t>(nw);
  Arena la(&c->repetition_lists, guard);
  uint32_t *d_wchars = nullptr, *d_v0 = nullptr, *d_v1 = nullptr, *d_r1 = nullptr, *d_r2 = nullptr, *d_r4 = nullptr, *d_r8 = nullptr, *d_rtmp = nullptr,
           *d_wtmp = nullptr;
  uint64_t *d_k0 = nullptr, *d_k1 = nullptr;
  uint8_t *d_lcp = nullptr, *d_flags = nullptr;
  long long *d_dup_off = nullptr;
  RptRuns runs{};
  for (int pass = 0; pass < 2; pass++) {
    lists.wstart = la.take<uint32_t>(nw);
    lists.wrow = la.take<uint32_t>(nw);
    lists.wa0 = la.take<uint32_t>(nw);
    lists.wend = la.take<uint32_t>(nw);
    lists.wa1 = la.take<uint32_t>(nw);
    lists.wc0 = la.take<uint32_t>(nw);
    lists.wc1 = la.take<uint32_t>(nw);
    lists.lstart = la.take<uint32_t>(nl);
    lists.lrow = la.take<uint32_t>(nl);
    lists.lc0 = la.take<uint32_t>(nl);
    lists.lend = la.take<uint32_t>(nl);
    lists.lc1 = la.take<uint32_t>(nl);
    d_wchars = la.take<uint32_t>(nw);
    d_dup_off = la.take<long long>(dup_rows + 1);
    d_k0 = la.take<uint64_t>(nw);
    d_k1 = la.take<uint64_t>(nw);
    d_v0 = la.take<uint32_t>(nw);
    d_v1 = la.take<uint32_t>(nw);
    d_r1 = la.take<uint32_t>(nw);
    d_r2 = la.take<uint32_t>(nw);
    d_r4 = la.take<uint32_t>(nw);
    d_r8 = la.take<uint32_t>(nw);
    d_lcp = la.take<uint8_t>(nw);
    d_flags = la.take<uint8_t>(2 * nw);  // (one byte per word and run pass of n >= 5)
    for (int j = 0; j < kRptGroup; j++) {
      runs.head[j] = la.take<uint32_t>(nw1);
      runs.run[j] = la.take<uint32_t>(nw1);
      runs.aux[j] = la.take<uint32_t>(nw1);
    }
    d_rtmp = la.take<uint32_t>(tmp_words);
    d_wtmp = la.take<uint32_t>(cdiv(nw1, kScanTile) + 8);
    if (pass == 0) la.commit();
  }
  la.arm(st);
  lists.n_words = nw;
  lists.n_lines = nl;
  if (nw != 0) {
    // ---- the word list, every word's characters, the word batch; the word identities ------------------------------------------
    hipLaunchKernelGGL(qual_class_kernel<true>, dim3(n_tiles), dim3(kBlock), 0, st, d_text, nb, d_boff, n, c->d_class_index, c->d_class_pages, d_tiles, nt1, d_qsig,
                       lists);
    hipLaunchKernelGGL(rpt_word_rows_kernel, count_grid(nw), dim3(kBlock), 0, st, lists, nb, d_wchars, d_dup_off);
    WP_LAUNCH_CHECK();
    wp_dedup_result first{};
    {
      BorrowedDedup borrowed(v);
      dedup_on_device(v, c, RaggedIn{in.d_data, d_dup_off, dup_rows, 1}, DedupPlan{}, &first);
    }
    if (timing) WP_HIP(hipEventRecord(c->ev[kMarkCounted], st));

    // ---- r1, then the rounds: one order of the positions by their 10-word windows -------------------------------------------
    const int id_bits = bit_length(dup_rows), row_bits = std::max(1, bit_length(n - 1)), bits = bit_length(nw);
    const uint32_t *vals = nullptr;
    auto sort_and_rank = [&](int key_bits, uint32_t *rank) {
      const int cur = radix_sort_pairs<uint64_t>(d_k0, d_v0, d_k1, d_v1, nw, 0, key_bits, d_rtmp, tmp_words, st, rs, true);
      vals = cur ? d_v1 : d_v0;
      if (!rank) return;
      hipLaunchKernelGGL(group_heads_kernel, count_grid(nw), dim3(kBlock), 0, st, static_cast<const uint64_t *>(cur ? d_k1 : d_k0), nw, runs.head[0]);
      device_exclusive_scan(runs.head[0], runs.run[0], nw, d_wtmp, nullptr, st);
      hipLaunchKernelGGL(rpt_rank_kernel, count_grid(nw), dim3(kBlock), 0, st, vals, static_cast<const uint32_t *>(runs.head[0]),
                         static_cast<const uint32_t *>(runs.run[0]), nw, rank);
    };
    auto pair_keys = [&](const uint32_t *a, const uint32_t *b, uint32_t h) {
      hipLaunchKernelGGL(rpt_pair_keys_kernel, count_grid(nw), dim3(kBlock), 0, st, a, b, static_cast<const uint32_t *>(lists.wrow), nw, h, bits, d_k0);
    };
    hipLaunchKernelGGL(rpt_word_keys_kernel, count_grid(nw), dim3(kBlock), 0, st, static_cast<const uint32_t *>(lists.wrow), static_cast<const int32_t *>(first.first),
                       nw, id_bits, d_k0);
    sort_and_rank(id_bits + row_bits, d_r1);
    pair_keys(d_r1, d_r1, 1);
    sort_and_rank(2 * bits, d_r2);
    pair_keys(d_r2, d_r2, 2);
    sort_and_rank(2 * bits, d_r4);
    pair_keys(d_r4, d_r4, 4);
    sort_and_rank(2 * bits, d_r8);
    pair_keys(d_r8, d_r2, 8);
    sort_and_rank(2 * bits, nullptr);
    WP_LAUNCH_CHECK();
    if (timing) WP_HIP(hipEventRecord(c->ev[kMarkSorted], st));

    // ---- the LCP of neighbours, the runs of every length three lengths at a time ----------------------------------------------
    hipLaunchKernelGGL(rpt_lcp_kernel, count_grid(nw), dim3(kBlock), 0, st, vals, static_cast<const uint32_t *>(d_r1), static_cast<const uint32_t *>(lists.wrow), nw,
                       d_lcp);
    for (uint32_t n0 = 2; n0 <= 8; n0 += kRptGroup) {
      hipLaunchKernelGGL(rpt_heads_kernel, count_grid(nw1), dim3(kBlock), 0, st, static_cast<const uint8_t *>(d_lcp), nw, n0, runs);
      for (int j = 0; j < kRptGroup; j++) device_exclusive_scan(runs.head[j], runs.run[j], nw1, d_wtmp, nullptr, st);
      if (n0 == 2) {
        hipLaunchKernelGGL(rpt_head_pos_kernel, count_grid(nw1), dim3(kBlock), 0, st, nw, runs);
        hipLaunchKernelGGL(rpt_top_kernel, count_grid(nw), dim3(kBlock), 0, st, vals, nw, runs, static_cast<const uint32_t *>(lists.wrow),
                           static_cast<const uint32_t *>(d_wchars), n, d_top);
      } else {
        for (int j = 0; j < kRptGroup; j++) WP_HIP(hipMemsetAsync(runs.aux[j], 0xff, nw1 * sizeof(uint32_t), st));
        hipLaunchKernelGGL(rpt_first_kernel, count_grid(nw), dim3(kBlock), 0, st, vals, nw, runs);
        hipLaunchKernelGGL(rpt_mark_kernel, count_grid(nw), dim3(kBlock), 0, st, vals, nw, runs, d_flags + (n0 == 5 ? 0 : nw));
      }
    }
    WP_LAUNCH_CHECK();
    if (timing) WP_HIP(hipEventRecord(c->ev[kMarkScanned], st));
    hipLaunchKernelGGL(rpt_cover_kernel, count_grid(nw), dim3(kBlock), 0, st, static_cast<const uint8_t *>(d_flags), static_cast<const uint32_t *>(lists.wrow),
                       static_cast<const uint32_t *>(d_wchars), nw, n, d_usig);
  } else if (timing) {  // (no word: the three stages in front of the rules are empty)
    WP_HIP(hipEventRecord(c->ev[kMarkCounted], st));
    WP_HIP(hipEventRecord(c->ev[kMarkSorted], st));
    WP_HIP(hipEventRecord(c->ev[kMarkScanned], st));
  }

  // ---- the rules, the kept rows, the compact form -----------------------------------------------------------------------------
  hipLaunchKernelGGL(rpt_rules_kernel, count_grid(n1), dim3(kBlock), 0, st, n, plan.lim, static_cast<const unsigned long long *>(d_top), d_sig, d_reasons, d_keep,
                     d_counters);
  WP_LAUNCH_CHECK();
  KeptRows kept;
  Arena oa(&c->repetition_out, guard);
  if (plan.want_compact) {
    kept.count(c, "repetition", d_keep, d_keep_pos, n, d_stmp, kScalarRptKept, st);
    for (int pass = 0; pass < 2; pass++) {
      kept.take(oa, nb);
      if (pass == 0) oa.commit();
    }
    oa.arm(st);
    kept.queue(c, in, d_keep, d_keep_pos, d_boff, nb, d_out_len, d_out_pos, d_stmp, kScalarRptOutBytes, st);
    WP_LAUNCH_CHECK();
  } else {
    device_exclusive_scan(d_keep, d_keep_pos, n1, d_stmp, c->d_scalars + kScalarRptKept, st);
  }
  if (timing) WP_HIP(hipEventRecord(c->ev[kMarkWalked], st));
  queue_scalar_slots(c, kScalarRptKept, kScalarRpt, st);
  WP_HIP(hipStreamSynchronize(st));
  unsigned long long counters[kRptCounters];
  std::memcpy(counters, c->h_scalars + kScalarRpt, sizeof(counters));
  ps.n_words = static_cast<int64_t>(counters[kRptWordsTotal]);
  ps.n_word_chars = static_cast<int64_t>(counters[kRptWordChars]);
  ps.n_kept = static_cast<int64_t>(c->h_scalars[kScalarRptKept]);
  for (int k = 0; k < WP_RPT_RULES; k++) ps.rule_failed[k] = static_cast<int64_t>(counters[kRptRuleFailed + k]);
  if (static_cast<size_t>(ps.n_words) != nw) throw HipError("repetition: the rows do not sum to the words of the text");
  if (timing) end_four_stage_timing(v, c);  // (words, sorts, runs, cover and rules: the header's section)
  // (kSiteOverlap: the row kernel and the kept rows of overlap.h run here too)
  throw_if_group_oob(kSiteQuality, "repetition signals", "gathers or stores outside the tile, word, slot or signal arrays skipped", kSiteOverlap,
                     "gathers or stores outside the row arrays skipped");
  check_arena_guard(c, ra, st, "repetition");
  check_arena_guard(c, ia, st, "repetition");
  check_arena_guard(c, la, st, "repetition");
  check_arena_guard(c, oa, st, "repetition");
  R->signals = reinterpret_cast<int64_t *>(d_sig);
  R->reasons = d_reasons;
  if (plan.want_compact) kept.hand_out(R, c->h_scalars[kScalarRptOutBytes], 1);
}

}  // namespace wp
