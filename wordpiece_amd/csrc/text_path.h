// text_path.h — what the text-signal layers share on a context (quality signals: quality_path.h, repetition signals:
// repetition_path.h, line filter: lines_path.h; kernels: quality.h): the names and the scalar slots of a
// layer, the rows rule and the answer of a call without bytes, the per-row arrays with the intake, the class pass with
// its lists, the items of a batch ordered by (row, first equal item), and the end of a call from the kept flags on.
// The intake and the kept rows are window_path.h's, the search for equal items dedup_path.h's.
#pragma once
#include <algorithm>
#include <initializer_list>

#include "context.h"
#include "dedup_path.h"
#include "quality.h"
#include "window_path.h"

namespace wp {

// ---- one layer: the prefix of its messages, its texts in the bounds-checking build, its block of scalar slots ----------
// bad to out_bytes: one word each, elems and windows 64 bits; counters: n_counters 64-bit counters.  The word between
// out_bytes and counters is the layer's own.
constexpr int kTextMaxCounters = 24;
struct TextLayer {
  const char *name, *oob_name, *oob_skipped;
  int bad, kept, elems, windows, words, lines, out_bytes, counters, n_counters;
};

// ---- the rules of the rows, the answer of a call without bytes ---------------------------------------------------------
static void check_text_rows(const char *layer, const void *row_off, size_t n_rows) {
  if (n_rows != 0 && !row_off) throw std::invalid_argument(std::string(layer) + ": row_off is NULL");
  check_row_count(layer, n_rows, " in row_off");
}

// A host call whose batch has no byte (n_rows >= 1): no device needed.  Every signal is 0 and `reasons`, the layer's
// rules over zeros, is the answer of every row.  s: the statistics of the call, begun; n_kept and rule_failed are filled.
template <typename Result, typename Stats>
static Result text_no_bytes(Stats &s, size_t n_rows, int n_signals, int n_rules, uint32_t reasons, bool want_compact) {
  Result h{};
  h.n_rows = static_cast<int64_t>(n_rows);
  h.signals = static_cast<int64_t *>(zeroed(n_rows * n_signals * sizeof(int64_t)));
  h.reasons = static_cast<uint32_t *>(zeroed(n_rows * sizeof(uint32_t)));
  std::fill(h.reasons, h.reasons + n_rows, reasons);
  const size_t n_kept = reasons == 0 ? n_rows : 0;
  s.n_kept = static_cast<int64_t>(n_kept);
  for (int r = 0; r < n_rules; r++) s.rule_failed[r] = (reasons >> r) & 1u ? static_cast<int64_t>(n_rows) : 0;
  if (want_compact) {
    h.n_kept = static_cast<int64_t>(n_kept);
    if (n_kept != 0) {
      h.kept = static_cast<int32_t *>(zeroed(n_kept * sizeof(int32_t)));
      for (size_t r = 0; r < n_kept; r++) h.kept[r] = static_cast<int32_t>(r);
    }
    h.row_off = static_cast<int64_t *>(zeroed((n_kept + 1) * sizeof(int64_t)));
  }
  return h;
}

// ---- the per-row arrays and the intake -----------------------------------------------------------------------------------
// The layer calls take() in both passes of the loop over its row arena, beside what it takes there alone, then queue()
// and read(); a stage mark of its own may stand between the two.
struct TextRows {
  size_t n = 0;
  int n_signals = 0;
  uint32_t *d_boff = nullptr, *d_reasons = nullptr, *d_keep = nullptr, *d_keep_pos = nullptr, *d_out_len = nullptr, *d_out_pos = nullptr, *d_stmp = nullptr;
  long long *d_sig = nullptr;
  unsigned long long *usig() const { return reinterpret_cast<unsigned long long *>(d_sig); }

  void take(Arena &a, size_t n_rows, int signals) {
    n = n_rows;
    n_signals = signals;
    d_boff = a.take<uint32_t>(n + 1);
    d_sig = a.take<long long>(n * n_signals);
    d_reasons = a.take<uint32_t>(n);
    d_keep = a.take<uint32_t>(n + 1);
    d_keep_pos = a.take<uint32_t>(n + 1);
    d_out_len = a.take<uint32_t>(n + 1);
    d_out_pos = a.take<uint32_t>(n + 1);
    d_stmp = a.take<uint32_t>(cdiv(n + 1, kScanTile) + 8);
  }
  // the layer's slots and the signals cleared, the offsets of the rows checked (window_path.h, windows of one element)
  void queue(Context *c, const TextLayer &L, const RaggedIn &in, hipStream_t st) {
    clear_scalars(c, L.bad, L.counters, st);
    WP_HIP(hipMemsetAsync(c->d_scalars + L.bad, 0xff, sizeof(uint32_t), st));
    WP_HIP(hipMemsetAsync(d_sig, 0, n * n_signals * sizeof(long long), st));
    queue_window_rows(c, in, 1, d_boff, L.bad, L.elems, L.windows, st);
    WP_LAUNCH_CHECK();
  }
  // the wait for the sizes -> the bytes of the batch
  size_t read(Context *c, const TextLayer &L, const RaggedIn &in, hipStream_t st) {
    queue_scalar_slots(c, L.bad, L.windows, st);
    WP_HIP(hipStreamSynchronize(st));
    return read_window_rows(c, L.name, in, L.bad, L.elems, L.windows).n_bytes;
  }
};

// ---- the class pass of quality.h -------------------------------------------------------------------------------------------
// the class table on the device of c, uploaded once per context
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

// The tile counts of a batch of n_bytes bytes and their scan scratch.  take() in both passes of the loop over the layer's
// item arena; count() (one wait) brings the numbers of words and lines; take_lists() in both passes of the loop over the
// list arena; write() fills the lists.  d_sums: n_rows * WP_QUALITY_SIGNALS sums, cleared, that both kernel passes add the
// per-character signals of quality.h to.  A batch without bytes has no word and no line and launches nothing.
struct ClassPass {
  size_t nb = 0, n_tiles = 0, nt1 = 0, n_counts = 0;
  uint32_t *d_tiles = nullptr, *d_ttmp = nullptr;
  struct Counts {
    size_t n_words, n_lines;
  };

  void take(Arena &a, size_t n_bytes) {
    nb = n_bytes;
    n_tiles = cdiv(nb, kQualTile);
    nt1 = n_tiles + 1;
    n_counts = kQualKinds * nt1;
    d_tiles = a.take<uint32_t>(n_counts);
    d_ttmp = a.take<uint32_t>(cdiv(n_counts, kScanTile) + 8);
  }
  Counts count(Context *c, const TextLayer &L, const RaggedIn &in, const TextRows &rows, unsigned long long *d_sums, hipStream_t st) {
    if (nb == 0) return Counts{0, 0};
    ensure_class_table(c, st);
    WP_HIP(hipMemsetAsync(d_tiles, 0, n_counts * sizeof(uint32_t), st));
    launch<false>(c, in, rows, d_sums, QualLists{}, st);
    device_exclusive_scan(d_tiles, d_tiles, n_counts, d_ttmp, nullptr, st);
    hipLaunchKernelGGL(qual_totals_kernel, dim3(1), dim3(kWave), 0, st, d_tiles, nt1, c->d_scalars + L.words, c->d_scalars + L.lines);
    WP_LAUNCH_CHECK();
    queue_scalar_slots(c, L.words, L.lines, st);
    WP_HIP(hipStreamSynchronize(st));
    const size_t nw = c->h_scalars[L.words], nl = c->h_scalars[L.lines];
    if (nw > nb || nl > nb) throw HipError(std::string(L.name) + ": the starts and the ends of the words or lines do not pair up");
    return Counts{nw, nl};
  }
  // with_word_chars: the character positions of the word ends too (wc0, wc1)
  static QualLists take_lists(Arena &a, size_t nw, size_t nl, bool with_word_chars) {
    QualLists q{};
    q.wstart = a.take<uint32_t>(nw);
    q.wrow = a.take<uint32_t>(nw);
    q.wa0 = a.take<uint32_t>(nw);
    q.wend = a.take<uint32_t>(nw);
    q.wa1 = a.take<uint32_t>(nw);
    if (with_word_chars) {
      q.wc0 = a.take<uint32_t>(nw);
      q.wc1 = a.take<uint32_t>(nw);
    }
    q.lstart = a.take<uint32_t>(nl);
    q.lrow = a.take<uint32_t>(nl);
    q.lc0 = a.take<uint32_t>(nl);
    q.lend = a.take<uint32_t>(nl);
    q.lc1 = a.take<uint32_t>(nl);
    q.n_words = nw;
    q.n_lines = nl;
    return q;
  }
  void write(Context *c, const RaggedIn &in, const TextRows &rows, unsigned long long *d_sums, const QualLists &lists, hipStream_t st) {
    if (nb != 0) launch<true>(c, in, rows, d_sums, lists, st);
  }

 private:
  template <bool kWrite>
  void launch(Context *c, const RaggedIn &in, const TextRows &rows, unsigned long long *d_sums, const QualLists &lists, hipStream_t st) {
    hipLaunchKernelGGL(qual_class_kernel<kWrite>, dim3(n_tiles), dim3(kBlock), 0, st, static_cast<const uint8_t *>(in.d_data), nb, rows.d_boff, rows.n, c->d_class_index,
                       c->d_class_pages, d_tiles, nt1, d_sums, lists);
  }
};

// ---- the items of a batch (its words, its lines) ordered by (row, first equal item) ---------------------------------------
// what a layer borrows from the handle while the duplicate-row search runs inside its call, put back when the scope
// ends: the statistics of the dedup layer and the handle's stage timing (the layer's call times itself)
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

// The duplicate-row search of dedup_path.h (with its waits) over 2 m + 1 pseudo-rows of the batch's bytes, item i of m
// being pseudo-row 2 i + 1 and the bytes between the items the rows around them: d_dup_off, 2 m + 2 offsets that a
// kernel of the layer wrote.  -> per pseudo-row the first one with the same bytes, in the buffers of the dedup layer.
static const int32_t *first_equal_items(wp_vocab *v, Context *c, const RaggedIn &in, const long long *d_dup_off, size_t m) {
  wp_dedup_result first{};
  BorrowedDedup borrowed(v);
  dedup_on_device(v, c, RaggedIn{in.d_data, d_dup_off, 2 * m + 1, 1}, DedupPlan{}, &first);
  return first.first;
}

// One stable sort of the m items by (row, first equal item): behind sort() vals lists the items in that order and
// d_head[s] is set where position s starts a run, so every later member of a run repeats an earlier item of its row.
struct ItemOrder {
  uint64_t *d_k0 = nullptr, *d_k1 = nullptr;
  uint32_t *d_v0 = nullptr, *d_v1 = nullptr, *d_head = nullptr, *d_rtmp = nullptr;
  size_t tmp_words = 0;
  const uint32_t *vals = nullptr;

  void take(Arena &a, size_t m) {
    tmp_words = radix_tmp_words<uint64_t>(m);
    d_k0 = a.take<uint64_t>(m);
    d_k1 = a.take<uint64_t>(m);
    d_v0 = a.take<uint32_t>(m);
    d_v1 = a.take<uint32_t>(m);
    d_head = a.take<uint32_t>(m + 1);
    d_rtmp = a.take<uint32_t>(tmp_words);
  }
  // d_row[i]: the row of item i; first: what first_equal_items() returned
  void sort(const uint32_t *d_row, const int32_t *first, size_t m, size_t n_rows, RadixStats *rs, hipStream_t st) {
    const int id_bits = bit_length(2 * m + 1), row_bits = std::max(1, bit_length(n_rows - 1));
    hipLaunchKernelGGL(qual_dup_keys_kernel, count_grid(m), dim3(kBlock), 0, st, d_row, first, m, id_bits, d_k0);
    const int cur = radix_sort_pairs<uint64_t>(d_k0, d_v0, d_k1, d_v1, m, 0, id_bits + row_bits, d_rtmp, tmp_words, st, rs, true);
    hipLaunchKernelGGL(group_heads_kernel, count_grid(m), dim3(kBlock), 0, st, static_cast<const uint64_t *>(cur ? d_k1 : d_k0), m, d_head);
    vals = cur ? d_v1 : d_v0;
  }
};

// ---- the end of a call, from d_keep on --------------------------------------------------------------------------------------
// begin(): the kept rows counted (with the compact form: one wait) or d_keep scanned, then the output arena: what the
// layer takes in front (`extra`, called in both passes), the compact form behind it.  Kernels of the layer that fill its
// extras go between the two calls.  end(): the compact form of `src`, whose rows start at the byte offsets d_src_boff
// and hold n_bytes bytes at most; the layer's last wait; the counters handed to `stats` with the kept count, for the
// layer's statistics and the checks of its own; the end of the stage timing, the checks of the bounds-checking build and
// of the arena guards; signals, reasons and the compact form into R.
struct TextTail {
  KeptRows kept;

  template <typename Extra>
  void begin(Context *c, const TextLayer &L, const TextRows &rows, size_t n_bytes, bool want_compact, bool want_extra, Arena &oa, hipStream_t st, Extra extra) {
    if (want_compact) {
      kept.count(c, L.name, rows.d_keep, rows.d_keep_pos, rows.n, rows.d_stmp, L.kept, st);
    } else {
      device_exclusive_scan(rows.d_keep, rows.d_keep_pos, rows.n + 1, rows.d_stmp, c->d_scalars + L.kept, st);
    }
    if (!want_compact && !want_extra) return;
    for (int pass = 0; pass < 2; pass++) {
      extra(oa);
      if (want_compact) kept.take(oa, n_bytes);
      if (pass == 0) oa.commit();
    }
    oa.arm(st);
  }
  void begin(Context *c, const TextLayer &L, const TextRows &rows, size_t n_bytes, bool want_compact, Arena &oa, hipStream_t st) {
    begin(c, L, rows, n_bytes, want_compact, false, oa, st, [](Arena &) {});
  }

  template <typename Result, typename Stats>
  void end(wp_vocab *v, Context *c, const TextLayer &L, const TextRows &rows, const RaggedIn &src, const uint32_t *d_src_boff, size_t n_bytes, bool want_compact,
           std::initializer_list<const Arena *> arenas, Result *R, Stats stats) {
    hipStream_t st = c->stream;
    if (want_compact) {
      kept.queue(c, src, rows.d_keep, rows.d_keep_pos, d_src_boff, n_bytes, rows.d_out_len, rows.d_out_pos, rows.d_stmp, L.out_bytes, st);
      WP_LAUNCH_CHECK();
    }
    if (v->stage_timing) WP_HIP(hipEventRecord(c->ev[kMarkWalked], st));
    queue_scalar_slots(c, L.kept, L.counters, st);
    WP_HIP(hipStreamSynchronize(st));
    unsigned long long counters[kTextMaxCounters];
    std::memcpy(counters, c->h_scalars + L.counters, L.n_counters * sizeof(unsigned long long));
    stats(counters, static_cast<int64_t>(c->h_scalars[L.kept]));
    if (v->stage_timing) end_four_stage_timing(v, c);
    // (kSiteOverlap: the row kernel and the kept rows of overlap.h run here too)
    throw_if_group_oob(kSiteQuality, L.oob_name, L.oob_skipped, kSiteOverlap, "gathers or stores outside the row arrays skipped");
    for (const Arena *a : arenas) check_arena_guard(c, *a, st, L.name);
    R->signals = reinterpret_cast<int64_t *>(rows.d_sig);
    R->reasons = rows.d_reasons;
    if (want_compact) kept.hand_out(R, c->h_scalars[L.out_bytes], 1);
  }
};

}  // namespace wp
