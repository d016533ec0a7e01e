// quality_path.h — the quality signals on a context (include/wordpiece_amd.h, section "quality signals"; kernels:
// quality.h): the argument rules, the answer of a call without bytes, the launches over one device batch and the buffers
// of a call.  The intake, the class pass, the order of the lines by (row, first equal line) and the end of a call are
// text_path.h's.
#pragma once
#include <vector>

#include "context.h"
#include "quality.h"
#include "text_path.h"

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

static_assert(kQualCounters <= kTextMaxCounters, "the counters of a text-signal layer");
constexpr TextLayer kQualLayer{"quality", "quality signals", "gathers or stores outside the tile, word, line or signal arrays skipped",
                               kScalarQualBad, kScalarQualKept, kScalarQualElems, kScalarQualWindows, kScalarQualWords, kScalarQualLines, kScalarQualOutBytes,
                               kScalarQual, kQualCounters};

// the statistics of a quality call before anything is known of its rows
static wp_quality_stats &begin_quality_stats(wp_vocab *v, size_t n_rows) {
  v->stats.quality_call = 1;
  v->stats.quality = wp_quality_stats{};
  v->stats.quality.n_rows = static_cast<int64_t>(n_rows);
  return v->stats.quality;
}

// a host call whose batch has no byte (n_rows >= 1): the rules over zeros (text_path.h)
static wp_quality_result quality_no_bytes(wp_vocab *v, const QualityPlan &plan, size_t n_rows) {
  const long long zeros[WP_QUALITY_SIGNALS] = {};
  return text_no_bytes<wp_quality_result>(begin_quality_stats(v, n_rows), n_rows, WP_QUALITY_SIGNALS, WP_QUALITY_RULES, quality_reasons(zeros, plan.lim),
                                          plan.want_compact);
}

// The batch `in` (n_rows >= 1), on c's stream.  The results are device pointers into c->quality_rows (signals, reasons)
// and c->quality_out (the compact form), valid until the handle's next call.  Waits: the header's section lists them.
// Per-row totals: per-tile partial sums combined by 64-bit integer atomics (quality.h).
static void quality_on_device(wp_vocab *v, Context *c, const RaggedIn &in, const QualityPlan &plan, wp_quality_result *R) {
  const TextLayer &L = kQualLayer;
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
  Arena ra(&c->quality_rows, guard);
  TextRows rows;
  for (int pass = 0; pass < 2; pass++) {
    rows.take(ra, n, WP_QUALITY_SIGNALS);
    if (pass == 0) ra.commit();
  }
  ra.arm(st);
  unsigned long long *d_counters = reinterpret_cast<unsigned long long *>(c->d_scalars + kScalarQual);
  unsigned long long *d_usig = rows.usig();
  rows.queue(c, L, in, st);
  if (timing) WP_HIP(hipEventRecord(c->ev[kMarkCounted], st));
  const size_t nb = rows.read(c, L, in, st);
  qs.n_bytes = static_cast<int64_t>(nb);
  const uint8_t *d_text = static_cast<const uint8_t *>(in.d_data);

  // ---- the class pass: counts and per-character signals, the lists; the word pass, the line pass -----------------------------
  Arena ia(&c->quality_items, guard);
  ClassPass cls;
  uint32_t *d_stop = nullptr;
  for (int pass = 0; pass < 2; pass++) {
    cls.take(ia, nb);
    d_stop = ia.take<uint32_t>(static_cast<size_t>(kQualMaxStop) * kQualStopWords);
    if (pass == 0) ia.commit();
  }
  ia.arm(st);
  if (nb != 0 && plan.n_stop != 0) WP_HIP(hipMemcpyAsync(d_stop, plan.stop.data(), plan.stop.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  const ClassPass::Counts counts = cls.count(c, L, in, rows, d_usig, st);
  const size_t nw = counts.n_words, nl = counts.n_lines;
  if (plan.want_dup && nl >= (size_t(1) << 30)) throw std::length_error("quality: 2^30 lines or more with WP_QUALITY_WANT_DUP_LINES");
  const bool dup = plan.want_dup && nl != 0;
  Arena la(&c->quality_lists, guard);
  QualLists lists{};
  ItemOrder order;
  uint32_t *d_lchars = nullptr;
  long long *d_dup_off = nullptr;
  for (int pass = 0; pass < 2; pass++) {
    lists = ClassPass::take_lists(la, nw, nl, false);
    d_lchars = la.take<uint32_t>(nl);
    if (dup) {
      d_dup_off = la.take<long long>(2 * nl + 2);
      order.take(la, nl);
    }
    if (pass == 0) la.commit();
  }
  la.arm(st);
  cls.write(c, in, rows, d_usig, lists, st);
  if (nw != 0) hipLaunchKernelGGL(qual_words_kernel, count_grid(nw), dim3(kBlock), 0, st, d_text, nb, lists, n, d_stop, plan.n_stop, d_usig);
  if (nl != 0) hipLaunchKernelGGL(qual_lines_kernel, count_grid(nl), dim3(kBlock), 0, st, d_text, nb, lists, n, plan.short_chars, d_usig, d_lchars, d_dup_off);
  WP_LAUNCH_CHECK();
  if (timing) WP_HIP(hipEventRecord(c->ev[kMarkSorted], st));

  // ---- duplicate lines: the lines ordered by (row, first line with the same bytes) ------------------------------------------
  if (dup) {
    order.sort(lists.lrow, first_equal_items(v, c, in, d_dup_off, nl), nl, n, rs, st);
    hipLaunchKernelGGL(qual_dup_kernel, count_grid(nl), dim3(kBlock), 0, st, order.vals, static_cast<const uint32_t *>(order.d_head), nl, lists.lrow, d_lchars, n, d_usig);
    WP_LAUNCH_CHECK();
  }
  if (timing) WP_HIP(hipEventRecord(c->ev[kMarkScanned], st));

  // ---- the rules, the kept rows, the compact form -----------------------------------------------------------------------------
  hipLaunchKernelGGL(qual_rules_kernel, count_grid(n + 1), dim3(kBlock), 0, st, rows.d_boff, n, plan.lim, rows.d_sig, rows.d_reasons, rows.d_keep, d_counters);
  WP_LAUNCH_CHECK();
  Arena oa(&c->quality_out, guard);
  TextTail tail;
  tail.begin(c, L, rows, nb, plan.want_compact, oa, st);
  // (stage timing: check, signals, duplicate lines, rules: the header's section)
  tail.end(v, c, L, rows, in, rows.d_boff, nb, plan.want_compact, {&ra, &ia, &la, &oa}, R, [&](const unsigned long long *counters, int64_t n_kept) {
    qs.n_chars = static_cast<int64_t>(counters[kQualChars]);
    qs.n_invalid = static_cast<int64_t>(counters[kQualInvalid]);
    qs.n_words = static_cast<int64_t>(counters[kQualWordsTotal]);
    qs.n_lines = static_cast<int64_t>(counters[kQualLinesTotal]);
    qs.n_dup_lines = static_cast<int64_t>(counters[kQualDupLines]);
    qs.n_kept = n_kept;
    for (int r = 0; r < WP_QUALITY_RULES; r++) qs.rule_failed[r] = static_cast<int64_t>(counters[kQualRuleFailed + r]);
    if (static_cast<size_t>(qs.n_words) != nw || static_cast<size_t>(qs.n_lines) != nl) throw HipError("quality: the rows do not sum to the words and lines of the text");
  });
}

}  // namespace wp
