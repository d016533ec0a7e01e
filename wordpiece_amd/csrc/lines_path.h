// lines_path.h — the line filter on a context (include/wordpiece_amd_lines.h; kernels: lines.h): the argument rules and
// the phrase table, the answer of a call without bytes, the launches over one device batch and the buffers of a call.
// The intake, the class pass with the lists, the order of the lines by (row, first equal line) and the end of a call are
// text_path.h's.
#pragma once
#include <algorithm>
#include <numeric>
#include <vector>

#include "context.h"
#include "lines.h"
#include "text_path.h"

namespace wp {

struct LinesPlan {
  bool want_lines = false, want_cut = false, want_compact = false;
  int dup_scope = 0;
  uint32_t dup_min_chars = 0, n_phrases = 0, n_one = 0, pool_words = 0;
  LfLimits lim{};
  std::vector<uint32_t> table;  // the phrase table as lf_phrase_kernel reads it (lines.h: kLfTab*), cut behind the pool's last word
};

// The phrases sorted by (one byte or more, prefix, index) into the table of lines.h: the two maps, per phrase its pool
// offset in words, length and flags, its key, and the pool with every phrase zero-padded to whole words.
static void lf_phrase_table(LinesPlan &p, const uint8_t *pool, const int64_t *off, const int32_t *flags) {
  const uint32_t n = p.n_phrases;
  std::vector<uint32_t> order(n), key(n);
  std::iota(order.begin(), order.end(), 0u);
  for (uint32_t t = 0; t < n; t++) {
    const int64_t a = off[t], len = off[t + 1] - a;
    key[t] = len == 1 ? pool[a] : 0x10000u | pool[a] | (static_cast<uint32_t>(pool[a + 1]) << 8);
    if (len == 1) p.n_one++;
  }
  std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return key[x] < key[y]; });
  p.table.assign(kLfTabWords, 0u);
  uint32_t words = 0;
  for (uint32_t s = 0; s < n; s++) {
    const uint32_t t = order[s], k = key[t] & 0xffffu;
    const int64_t a = off[t], len = off[t + 1] - a;
    if (len == 1) p.table[kLfTabOne + (k >> 5)] |= 1u << (k & 31u); else p.table[k >> 5] |= 1u << (k & 31u);
    p.table[kLfTabMeta + s] = words | (static_cast<uint32_t>(len) << 16) | (static_cast<uint32_t>(flags[t]) << 24);
    p.table[kLfTabKeys + (s >> 1)] |= k << (16u * (s & 1u));
    for (int64_t i = 0; i < len; i++) p.table[kLfTabPool + words + i / 4] |= static_cast<uint32_t>(pool[a + i]) << (8u * static_cast<uint32_t>(i % 4));
    words += static_cast<uint32_t>((len + 3) / 4);
  }
  p.pool_words = words;
  p.table.resize(kLfTabPool + words);
}

// every rule of the spec, each with the field it is about; nothing here needs a device
static LinesPlan check_lines_spec(const wp_lines_spec *spec, const wp_lines_result *out) {
  if (!spec) throw std::invalid_argument("lines: spec is NULL");
  if (!out) throw std::invalid_argument("lines: out is NULL");
  if (spec->elem_bytes != 1) throw std::invalid_argument("lines: elem_bytes must be 1");
  check_want("lines", spec->want, WP_LF_WANT_LINES | WP_LF_WANT_CUT | WP_LF_WANT_COMPACT);
  LinesPlan p;
  p.want_lines = (spec->want & WP_LF_WANT_LINES) != 0;
  p.want_cut = (spec->want & WP_LF_WANT_CUT) != 0;
  p.want_compact = (spec->want & WP_LF_WANT_COMPACT) != 0;
  auto limit = [](const char *what, int k, int64_t L, bool flag) {
    const std::string name = std::string("lines: ") + what + "[" + std::to_string(k) + "]";
    if (flag && L != -1 && L != 0) throw std::invalid_argument(name + " must be 0 or -1");
    if (L != -1 && (L < 0 || L > 1000000000)) throw std::invalid_argument(name + " must be -1 or in [0, 10^9]");
    return static_cast<long long>(L);
  };
  for (int k = 0; k < 4; k++) p.lim.line[k] = limit("line_limit", k, spec->line_limit[k], k == WP_LR_NOT_TERMINAL || k == WP_LR_ELLIPSIS_END);
  for (int k = 0; k < WP_LF_DOC_RULES; k++) p.lim.doc[k] = limit("doc_limit", k, spec->doc_limit[k], false);
  if (spec->dup_scope < 0 || spec->dup_scope > 2) throw std::invalid_argument("lines: dup_scope must be 0, 1 or 2");
  if (spec->dup_min_chars < 0) throw std::invalid_argument("lines: dup_min_chars must not be negative");
  p.dup_scope = spec->dup_scope;
  p.dup_min_chars = static_cast<uint32_t>(spec->dup_min_chars);
  if (spec->n_phrases < 0 || spec->n_phrases > WP_LF_MAX_PHRASES) throw std::invalid_argument("lines: n_phrases must be in [0, 512]");
  if (spec->pad != 0) throw std::invalid_argument("lines: pad must be 0");
  p.n_phrases = static_cast<uint32_t>(spec->n_phrases);
  if (p.n_phrases != 0) {
    if (!spec->phrase_pool) throw std::invalid_argument("lines: phrase_pool is NULL");
    if (!spec->phrase_off) throw std::invalid_argument("lines: phrase_off is NULL");
    if (!spec->phrase_flags) throw std::invalid_argument("lines: phrase_flags is NULL");
    if (spec->phrase_off[0] != 0) throw std::invalid_argument("lines: phrase_off must start at 0");
    const uint8_t *pool = static_cast<const uint8_t *>(spec->phrase_pool);
    for (uint32_t t = 0; t < p.n_phrases; t++) {
      const int64_t a = spec->phrase_off[t], len = spec->phrase_off[t + 1] - a;
      const std::string at = "phrase " + std::to_string(t);
      if (len < 1 || len > WP_LF_MAX_PHRASE_BYTES) throw std::invalid_argument("lines: phrase_off: " + at + " must have 1 to 32 bytes");
      if (a + len > WP_LF_MAX_POOL_BYTES) throw std::invalid_argument("lines: phrase_off: " + at + " ends behind the 8192 bytes of a pool");
      for (int64_t i = 0; i < len; i++) {
        const uint32_t b = pool[a + i];
        if (b >= 'A' && b <= 'Z') throw std::invalid_argument("lines: phrase_pool: " + at + " holds ASCII upper case");
        if (b == 0x0a) throw std::invalid_argument("lines: phrase_pool: " + at + " holds a line feed");
      }
      if ((spec->phrase_flags[t] & ~(WP_LF_PHRASE_BOUNDED | WP_LF_PHRASE_DOC)) != 0) throw std::invalid_argument("lines: phrase_flags: " + at + " has bits outside 3");
    }
    lf_phrase_table(p, pool, spec->phrase_off, spec->phrase_flags);
  }
  if (spec->reserved != 0) throw std::invalid_argument("lines: reserved must be 0");
  return p;
}

static_assert(kLfCounters <= kTextMaxCounters, "the counters of a text-signal layer");
constexpr TextLayer kLfLayer{"lines", "line filter", "gathers or stores outside the tile, word, line, signal or cut arrays skipped",
                             kScalarLfBad, kScalarLfKept, kScalarLfElems, kScalarLfWindows, kScalarLfWords, kScalarLfLines, kScalarLfOutBytes,
                             kScalarLf, kLfCounters};

static wp_lines_stats &begin_lines_stats(wp_vocab *v, size_t n_rows) {
  v->stats.lines_call = 1;
  v->stats.lines = wp_lines_stats{};
  v->stats.lines.n_rows = static_cast<int64_t>(n_rows);
  return v->stats.lines;
}

// A host call whose batch has no byte (n_rows >= 1): the document rules over zeros (text_path.h); no row has a line, and
// the cut rows are the empty rows themselves.
static wp_lines_result lines_no_bytes(wp_vocab *v, const LinesPlan &plan, size_t n_rows) {
  const long long zeros[WP_LF_SIGNALS] = {};
  wp_lines_result h = text_no_bytes<wp_lines_result>(begin_lines_stats(v, n_rows), n_rows, WP_LF_SIGNALS, WP_LF_DOC_RULES, lines_reasons(zeros, plan.lim),
                                                     plan.want_compact);
  if (plan.want_cut) h.cut_off = static_cast<int64_t *>(zeroed((n_rows + 1) * sizeof(int64_t)));
  return h;
}

// The batch `in` (n_rows >= 1), on c's stream.  The results are device pointers into c->lines_rows (signals, reasons),
// c->lines_lists (the arrays per line) and c->lines_out (the cut and the compact form), valid until the handle's next
// call.  Waits, from the spec alone: the sizes; the numbers of words and lines; with dup_scope != 0 those of the
// duplicate-row search over the lines; with the compact form the kept count; the one that ends the call.
// Per-document sums: 64-bit integer atomics per line (lf_sums_kernel).  The lines of a row are neighbours in the list,
// so a segmented sum would also do, but it would need the row boundaries in the line list and a pass per signal; the
// atomics are one pass, order-free because they are integer adds, and a line adds only what is not zero.
static void lines_on_device(wp_vocab *v, Context *c, const RaggedIn &in, const LinesPlan &plan, wp_lines_result *R) {
  const TextLayer &L = kLfLayer;
  const size_t n = in.n_rows;
  wp_lines_stats &ps = begin_lines_stats(v, n);
  *R = wp_lines_result{};
  R->n_rows = static_cast<int64_t>(n);
  hipStream_t st = c->stream;
  const bool guard = v->arena_guard || EnvOptions::get().arena_guard;
  // WP_OPT_STAGE_TIMING: kMarkStart, kMarkCounted (intake, class passes, lists), kMarkSorted (phrase scan, line pass),
  // kMarkScanned (duplicates), kMarkWalked (sums, document rules, cut, compact form)
  const bool timing = v->stage_timing;
  RadixStats *rs = begin_stage_timing(c, timing, st);

  // ---- the per-row arrays, the offset check --------------------------------------------------------------------------------
  const size_t n1 = n + 1;
  Arena ra(&c->lines_rows, guard);
  TextRows rows;
  uint32_t *d_cut_boff = nullptr;
  unsigned long long *d_qsig = nullptr;
  for (int pass = 0; pass < 2; pass++) {
    rows.take(ra, n, WP_LF_SIGNALS);
    d_cut_boff = ra.take<uint32_t>(n1);
    d_qsig = ra.take<unsigned long long>(n * WP_QUALITY_SIGNALS);  // what the class pass sums beside its counts: not read
    if (pass == 0) ra.commit();
  }
  ra.arm(st);
  unsigned long long *d_counters = reinterpret_cast<unsigned long long *>(c->d_scalars + kScalarLf);
  unsigned long long *d_usig = rows.usig();
  const uint32_t *d_boff = rows.d_boff;
  WP_HIP(hipMemsetAsync(d_qsig, 0, n * WP_QUALITY_SIGNALS * sizeof(unsigned long long), st));
  rows.queue(c, L, in, st);
  const size_t nb = rows.read(c, L, in, st);
  ps.n_bytes = static_cast<int64_t>(nb);
  const uint8_t *d_text = static_cast<const uint8_t *>(in.d_data);
  const uint32_t *d32 = static_cast<const uint32_t *>(in.d_data);

  // ---- the class pass of quality.h: the numbers of words and lines -------------------------------------------------------------
  Arena ia(&c->lines_items, guard);
  ClassPass cls;
  uint32_t *d_table = nullptr;
  for (int pass = 0; pass < 2; pass++) {
    cls.take(ia, nb);
    d_table = ia.take<uint32_t>(kLfTabWords);
    if (pass == 0) ia.commit();
  }
  ia.arm(st);
  if (nb != 0 && plan.n_phrases != 0) WP_HIP(hipMemcpyAsync(d_table, plan.table.data(), plan.table.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  const ClassPass::Counts counts = cls.count(c, L, in, rows, d_qsig, st);
  const size_t nw = counts.n_words, nl = counts.n_lines;
  if (plan.dup_scope != 0 && nl >= (size_t(1) << 30)) throw std::length_error("lines: 2^30 lines or more with dup_scope != 0");

  // ---- the lists and the per-line arrays --------------------------------------------------------------------------------------
  const bool dup = plan.dup_scope != 0 && nl != 0, sorted = dup && plan.dup_scope == 1;
  const size_t nl1 = nl + 1;
  Arena la(&c->lines_lists, guard);
  QualLists lists{};
  LfLines ln{};
  ItemOrder order;
  uint32_t *d_drop = nullptr, *d_D = nullptr, *d_ltmp = nullptr;
  long long *d_dup_off = nullptr, *d_line_start = nullptr;
  int32_t *d_line_row = nullptr, *d_line_len = nullptr;
  for (int pass = 0; pass < 2; pass++) {
    lists = ClassPass::take_lists(la, nw, nl, false);
    ln.words = la.take<uint32_t>(nl);
    ln.chars = la.take<uint32_t>(nl);
    ln.own_end = la.take<uint32_t>(nl);
    ln.reasons = la.take<uint32_t>(nl);
    d_drop = la.take<uint32_t>(nl1);
    d_D = la.take<uint32_t>(nl1);
    d_ltmp = la.take<uint32_t>(cdiv(nl1, kScanTile) + 8);
    if (plan.want_lines) {
      d_line_start = la.take<long long>(nl);
      d_line_row = la.take<int32_t>(nl);
      d_line_len = la.take<int32_t>(nl);
    }
    if (dup) d_dup_off = la.take<long long>(2 * nl + 2);
    if (sorted) order.take(la, nl);
    if (pass == 0) la.commit();
  }
  la.arm(st);
  cls.write(c, in, rows, d_qsig, lists, st);
  if (nl != 0) WP_HIP(hipMemsetAsync(ln.reasons, 0, nl * sizeof(uint32_t), st));
  WP_LAUNCH_CHECK();
  if (timing) WP_HIP(hipEventRecord(c->ev[kMarkCounted], st));

  // ---- the phrase scan, the line pass ------------------------------------------------------------------------------------------
  if (nb != 0 && plan.n_phrases != 0) {
    hipLaunchKernelGGL(lf_phrase_kernel, dim3(std::min<size_t>(cls.n_tiles, 1024)), dim3(kBlock), 0, st, d32, nb, d_boff, n, static_cast<const uint32_t *>(d_table),
                       plan.n_one, plan.n_phrases, plan.pool_words, lists, ln.reasons, d_usig, d_counters + kLfMatches);
  }
  if (nl != 0) hipLaunchKernelGGL(lf_lines_kernel, count_grid(nl), dim3(kBlock), 0, st, d_text, nb, d_boff, lists, n, plan.lim, ln, d_dup_off);
  WP_LAUNCH_CHECK();
  if (timing) WP_HIP(hipEventRecord(c->ev[kMarkSorted], st));

  // ---- duplicate lines: the first line with the same bytes; scope 1: the lines ordered by (row, that line) --------------------
  if (dup) {
    const int32_t *first = first_equal_items(v, c, in, d_dup_off, nl);
    if (sorted) order.sort(lists.lrow, first, nl, n, rs, st);
    hipLaunchKernelGGL(lf_dup_kernel, count_grid(nl), dim3(kBlock), 0, st, first, order.vals, static_cast<const uint32_t *>(order.d_head), nl,
                       static_cast<const uint32_t *>(ln.chars), plan.dup_min_chars, ln.reasons);
    WP_LAUNCH_CHECK();
  }
  if (timing) WP_HIP(hipEventRecord(c->ev[kMarkScanned], st));

  // ---- the sums, D, the document rules, the kept rows; the cut, and the compact form over it -----------------------------------
  hipLaunchKernelGGL(lf_sums_kernel, count_grid(nl1), dim3(kBlock), 0, st, lists, ln, n, d_usig, d_drop, d_line_row, d_line_start, d_line_len);
  device_exclusive_scan(d_drop, d_D, nl1, d_ltmp, c->d_scalars + kScalarLfDropped, st);
  hipLaunchKernelGGL(lf_docs_kernel, count_grid(n1), dim3(kBlock), 0, st, d_boff, n, plan.lim, rows.d_sig, rows.d_reasons, rows.d_keep, d_counters);
  WP_LAUNCH_CHECK();
  const bool cut = plan.want_cut || plan.want_compact;
  Arena oa(&c->lines_out, guard);
  TextTail tail;
  long long *d_cut_off = nullptr;
  uint32_t *d_cut = nullptr;
  tail.begin(c, L, rows, nb, plan.want_compact, cut, oa, st, [&](Arena &a) {
    d_cut_off = a.take<long long>(n1);
    d_cut = a.take<uint32_t>(nb / 4 + 1);
  });
  if (cut) {
    hipLaunchKernelGGL(lf_cut_off_kernel, count_grid(n1), dim3(kBlock), 0, st, static_cast<const uint32_t *>(d_D), static_cast<const uint32_t *>(lists.lstart), nl,
                       d_boff, n, d_cut_off, d_cut_boff);
    if (nb != 0) {
      hipLaunchKernelGGL(lf_cut_kernel, dim3(cdiv(nb, kLfCutTile)), dim3(kBlock), 0, st, d32, nb, static_cast<const uint32_t *>(lists.lstart),
                         static_cast<const uint32_t *>(ln.own_end), static_cast<const uint32_t *>(d_D), nl, d_cut);
    }
    WP_LAUNCH_CHECK();
  }
  // (the compact form is taken from the cut: nb bounds its bytes, which the last wait brings; stage timing: lists,
  // phrases and lines, duplicates, rules and cut: the header's section)
  size_t dropped = 0;
  tail.end(v, c, L, rows, RaggedIn{d_cut, d_cut_off, n, 1}, d_cut_boff, nb, plan.want_compact, {&ra, &ia, &la, &oa}, R,
           [&](const unsigned long long *counters, int64_t n_kept) {
             dropped = c->h_scalars[kScalarLfDropped];
             if (counters[kLfLinesTotal] != nl || dropped > nb) throw HipError("lines: the rows do not sum to the lines of the text");
             ps.n_lines = static_cast<int64_t>(nl);
             ps.n_kept_lines = static_cast<int64_t>(counters[kLfKeptLines]);
             ps.n_kept_bytes = static_cast<int64_t>(counters[kLfKeptBytes]);
             ps.n_kept = n_kept;
             ps.n_phrase_matches = static_cast<int64_t>(counters[kLfMatches]);
             for (int k = 0; k < WP_LF_LINE_RULES; k++) ps.line_failed[k] = static_cast<int64_t>(counters[kLfLineFailed + k]);
             for (int k = 0; k < WP_LF_DOC_RULES; k++) ps.rule_failed[k] = static_cast<int64_t>(counters[kLfRuleFailed + k]);
           });
  if (plan.want_lines) {
    R->n_lines = static_cast<int64_t>(nl);
    if (nl != 0) {
      R->line_row = d_line_row;
      R->line_start = reinterpret_cast<int64_t *>(d_line_start);
      R->line_len = d_line_len;
      R->line_reasons = ln.reasons;
    }
  }
  if (plan.want_cut) {
    R->n_cut_elems = static_cast<int64_t>(nb - dropped);
    R->cut_off = reinterpret_cast<int64_t *>(d_cut_off);
    R->cut_data = R->n_cut_elems ? d_cut : nullptr;
  }
}

}  // namespace wp
