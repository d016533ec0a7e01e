// align_path.h — span alignment on a context (include/wordpiece_amd.h, section "span alignment"; kernels: align.h): the
// argument rules, the launches over device buffers, and the buffers of a host call.
#pragma once
#include "align.h"
#include "context.h"
#include "rows.h"  // lanes_for

namespace wp {

// the arrays of a call, wherever they lie; the padded form has types / lengths / sample, the ragged form row_splits
struct AlignIn {
  const uint32_t *offsets = nullptr;
  const int32_t *types = nullptr, *lengths = nullptr, *sample = nullptr;
  const int64_t *row_splits = nullptr;
  const int64_t *span_splits = nullptr;
  const uint32_t *spans = nullptr;
  const int32_t *span_labels = nullptr;
  size_t n_rows = 0, n_samples = 0, n_spans = 0, n_ids = 0;
};
struct AlignOut {
  int32_t *labels = nullptr, *span_index = nullptr, *start = nullptr, *end = nullptr;
};

// every rule of the spec and the sizes that needs no array; want: the WP_ALIGN_* bits of the outputs of this call; host:
// a host entry point (labels need span_labels whatever n_spans is; a device array of no spans may be NULL)
static AlignGeom check_align_spec(const wp_align_spec *spec, const AlignIn &in, bool ragged, int want, bool host) {
  if (!spec) throw std::invalid_argument("align: spec is NULL");
  if (!ragged && spec->max_len < 1) throw std::invalid_argument("align: max_len must be at least 1");
  if (!ragged && spec->side != 0 && spec->side != 1) throw std::invalid_argument("align: side must be 0 or 1");
  if (!ragged && spec->side == 1 && !in.types) throw std::invalid_argument("align: side 1 needs token_type_ids");
  if ((want & ~7) != 0) throw std::invalid_argument("align: want has bits outside 7");
  if (ragged && (want & WP_ALIGN_POSITIONS)) throw std::invalid_argument("align: the ragged form has no positions");
  if (want == 0) throw std::invalid_argument("align: no output is wanted");
  if ((want & WP_ALIGN_LABELS) && (host || in.n_spans != 0) && !in.span_labels) throw std::invalid_argument("align: labels wanted without span_labels");
  if (in.n_rows > static_cast<size_t>(INT32_MAX)) throw std::length_error("align: more rows than INT32_MAX");
  if (in.n_samples > static_cast<size_t>(INT32_MAX)) throw std::length_error("align: more samples than INT32_MAX");
  if (in.n_spans > static_cast<size_t>(INT32_MAX)) throw std::length_error("align: more spans than INT32_MAX");
  if (in.n_ids > static_cast<size_t>(INT32_MAX)) throw std::length_error("align: more ids than INT32_MAX");
  if (!ragged && in.n_rows > SIZE_MAX / (2 * sizeof(uint32_t)) / static_cast<size_t>(spec->max_len)) {
    throw std::length_error("align: n_rows * max_len is too large");
  }
  if (!in.span_splits) throw std::invalid_argument("align: span_splits is NULL");
  if (in.n_spans != 0 && !in.spans) throw std::invalid_argument("align: spans is NULL");
  AlignGeom g{};
  g.max_len = ragged ? 0 : spec->max_len;
  g.side = ragged ? 0 : spec->side;
  g.outside_label = spec->outside_label;
  g.inside_add = spec->inside_add;
  g.ignore_id = spec->ignore_id;
  g.no_answer = spec->no_answer;
  g.n_samples = static_cast<long long>(in.n_samples);
  g.n_spans = static_cast<long long>(in.n_spans);
  return g;
}

// what the array check found (host loop or align_check_kernel), in the words of the header
[[noreturn]] static void throw_align_bad(unsigned long long key) {
  const int rule = static_cast<int>(key >> 32);
  const unsigned long long detail = 0xFFFFFFFFull - (key & 0xFFFFFFFFull);
  switch (rule) {
    case kAlignBadRowSplits:
      throw std::invalid_argument("align: row_splits must start at 0, never descend and end at n_ids (entry " + std::to_string(detail) + ")");
    case kAlignBadSpanSplits:
      throw std::invalid_argument("align: span_splits must start at 0, never descend and end at n_spans (entry " + std::to_string(detail) + ")");
    case kAlignBadSpan:
      if (detail % 2 == 0) throw std::invalid_argument("align: span " + std::to_string(detail / 2) + " is empty (begin >= end)");
      throw std::invalid_argument("align: span " + std::to_string(detail / 2) + " begins before span " + std::to_string(detail / 2 - 1) +
                                  " of its sample ends (spans must be sorted and disjoint)");
    default:
      throw std::invalid_argument("align: the sample of row " + std::to_string(detail) + " is outside [0, n_samples)");
  }
}

// the array rules on host arrays, in the order the kernel's key ranks them; throws at the first offender
static void check_align_arrays(const AlignIn &in, bool ragged) {
  if (ragged) {
    for (size_t i = 0; i <= in.n_rows; i++) {
      const int64_t s = in.row_splits[i];
      if ((i == 0 && s != 0) || (i < in.n_rows && in.row_splits[i + 1] < s) || (i == in.n_rows && s != static_cast<int64_t>(in.n_ids))) {
        throw_align_bad(align_bad_key(kAlignBadRowSplits, i));
      }
    }
  }
  for (size_t i = 0; i <= in.n_samples; i++) {
    const int64_t s = in.span_splits[i];
    if ((i == 0 && s != 0) || (i < in.n_samples && in.span_splits[i + 1] < s) || (i == in.n_samples && s != static_cast<int64_t>(in.n_spans))) {
      throw_align_bad(align_bad_key(kAlignBadSpanSplits, i));
    }
  }
  for (size_t s = 0; s < in.n_samples; s++) {
    for (int64_t j = in.span_splits[s]; j < in.span_splits[s + 1]; j++) {
      if (in.spans[2 * j] >= in.spans[2 * j + 1]) throw_align_bad(align_bad_key(kAlignBadSpan, 2 * static_cast<unsigned long long>(j)));
      if (j > in.span_splits[s] && in.spans[2 * j - 1] > in.spans[2 * j]) {
        throw_align_bad(align_bad_key(kAlignBadSpan, 2 * static_cast<unsigned long long>(j) + 1));
      }
    }
  }
  if (!ragged) {
    for (size_t r = 0; r < in.n_rows; r++) {
      const long long s = in.sample ? static_cast<long long>(in.sample[r]) : static_cast<long long>(r);
      if (s < 0 || s >= static_cast<long long>(in.n_samples)) throw_align_bad(align_bad_key(kAlignBadSample, r));
    }
  }
}

// the statistics of an align call before its counters are known (all there is to say of a call without rows)
static wp_align_stats &begin_align_stats(wp_vocab *v, size_t n_rows, size_t n_spans) {
  v->stats.align_call = 1;
  v->stats.align = wp_align_stats{};
  v->stats.align.n_rows = static_cast<int64_t>(n_rows);
  v->stats.align.n_spans = static_cast<int64_t>(n_spans);
  return v->stats.align;
}

template <bool LABELS, bool INDEX, bool POS, typename... Args>
static void launch_align(dim3 grid, hipStream_t st, Args... args) {
  hipLaunchKernelGGL((align_kernel<LABELS, INDEX, POS>), grid, dim3(kBlock), 0, st, args...);
}

// The launches of a call over device arrays on c's stream (`in` and `out` hold device pointers), one wait (for the
// counters and the word of the check), the statistics of the call.  check: the array rules are checked here, in a
// kernel (the device entry points); the kernel behind it writes nothing where they fail, and the call throws.
static void align_on_device(wp_vocab *v, Context *c, const AlignIn &in, const AlignGeom &g, bool ragged, const AlignOut &out, bool check) {
  wp_align_stats &as = begin_align_stats(v, in.n_rows, in.n_spans);
  const size_t n_cells = ragged ? in.n_ids : in.n_rows;  // (what the grid is sized by)
  if (n_cells == 0 && !check) return;
  hipStream_t st = c->stream;
  static_assert(scalar_end(kScalarAlign) - kScalarAlign == 2 * kAlignCounters, "the slot kScalarAlign holds the counters of an align call");
  static_assert(scalar_end(kScalarAlignBad) == kScalarAlign, "the word of the check lies in front of the counters");
  unsigned long long *d_bad = reinterpret_cast<unsigned long long *>(c->d_scalars + kScalarAlignBad);
  unsigned long long *d_cnt = reinterpret_cast<unsigned long long *>(c->d_scalars + kScalarAlign);
  clear_scalars(c, kScalarAlignBad, kScalarAlign, st);
  const uint2 *d_offsets = reinterpret_cast<const uint2 *>(in.offsets), *d_spans = reinterpret_cast<const uint2 *>(in.spans);
  const long long *d_splits = reinterpret_cast<const long long *>(in.span_splits);
  if (check) {
    const size_t n_items = std::max(std::max(in.n_rows, in.n_samples) + 1, in.n_spans);
    hipLaunchKernelGGL(align_check_kernel, dim3(static_cast<unsigned>(std::min<size_t>(cdiv(n_items, kBlock), 1024))), dim3(kBlock), 0, st,
                       ragged ? reinterpret_cast<const long long *>(in.row_splits) : nullptr, in.n_rows, static_cast<long long>(in.n_ids),
                       in.sample, d_splits, in.n_samples, d_spans, in.n_spans, d_bad);
  }
  if (n_cells != 0 && ragged) {
    const size_t n_tiles = cdiv(in.n_ids, kBlock);
    const dim3 grid(static_cast<unsigned>(std::min<size_t>(n_tiles, kAlignMaxGrid)));
    const long long *d_rows = reinterpret_cast<const long long *>(in.row_splits);
    const long long n_rows = static_cast<long long>(in.n_rows), n_ids = static_cast<long long>(in.n_ids);
    if (out.labels && out.span_index) {
      hipLaunchKernelGGL((align_rows_kernel<true, true>), grid, dim3(kBlock), 0, st, d_offsets, d_rows, n_rows, n_ids, n_tiles, g, d_splits,
                         d_spans, in.span_labels, out.labels, out.span_index, d_bad, d_cnt);
    } else if (out.labels) {
      hipLaunchKernelGGL((align_rows_kernel<true, false>), grid, dim3(kBlock), 0, st, d_offsets, d_rows, n_rows, n_ids, n_tiles, g, d_splits,
                         d_spans, in.span_labels, out.labels, out.span_index, d_bad, d_cnt);
    } else {
      hipLaunchKernelGGL((align_rows_kernel<false, true>), grid, dim3(kBlock), 0, st, d_offsets, d_rows, n_rows, n_ids, n_tiles, g, d_splits,
                         d_spans, in.span_labels, out.labels, out.span_index, d_bad, d_cnt);
    }
  } else if (n_cells != 0) {
    const int lanes = lanes_for(g.max_len);
    const size_t n_blocks = cdiv(in.n_rows, static_cast<size_t>(kBlock / lanes));
    const dim3 grid(static_cast<unsigned>(std::min<size_t>(n_blocks, kAlignMaxGrid)));
    const int which = (out.labels ? 1 : 0) | (out.span_index ? 2 : 0) | (out.start ? 4 : 0);
    auto go = [&](auto labels, auto index, auto pos) {
      launch_align<decltype(labels)::value, decltype(index)::value, decltype(pos)::value>(
          grid, st, d_offsets, in.types, in.lengths, in.sample, in.n_rows, n_blocks, g, lanes, d_splits, d_spans, in.span_labels, out.labels,
          out.span_index, out.start, out.end, static_cast<const unsigned long long *>(d_bad), d_cnt);
    };
    constexpr std::true_type T{};
    constexpr std::false_type F{};
    switch (which) {
      case 1: go(T, F, F); break;
      case 2: go(F, T, F); break;
      case 3: go(T, T, F); break;
      case 4: go(F, F, T); break;
      case 5: go(T, F, T); break;
      case 6: go(F, T, T); break;
      default: go(T, T, T); break;
    }
  }
  WP_LAUNCH_CHECK();
  queue_scalar_slots(c, kScalarAlignBad, kScalarAlign, st);
  WP_HIP(hipStreamSynchronize(st));
  unsigned long long bad;
  std::memcpy(&bad, c->h_scalars + kScalarAlignBad, sizeof(bad));
  if (bad != 0) throw_align_bad(bad);
  throw_if_oob(kSiteAlign, "span alignment", "samples outside the splits or gathers outside the span list skipped");
  const unsigned long long *h_cnt = reinterpret_cast<const unsigned long long *>(c->h_scalars + kScalarAlign);
  as.n_tokens = static_cast<int64_t>(h_cnt[kAlignTokens]);
  as.n_covered = static_cast<int64_t>(h_cnt[kAlignCovered]);
  as.n_begin = static_cast<int64_t>(h_cnt[kAlignBegin]);
  as.n_answer_rows = static_cast<int64_t>(h_cnt[kAlignAnswer]);
  as.n_no_answer_rows = static_cast<int64_t>(h_cnt[kAlignNoAnswer]);
}

// The host form as far as the device: the arrays go up into c->pad_buf, the launches, and the blocks the caller asked for
// lie there until the handle's next call: offsets | types | lengths | sample | row_splits | span_splits | spans |
// span_labels | labels | span_index | start | end.  The array rules were checked on the host.
static AlignOut align_from_host(wp_vocab *v, Context *c, const AlignIn &in, const AlignGeom &g, bool ragged, int want) {
  const size_t cells = ragged ? in.n_ids : in.n_rows * static_cast<size_t>(g.max_len);
  Arena a(&c->pad_buf, v->arena_guard || EnvOptions::get().arena_guard);
  AlignIn d = in;
  AlignOut o;
  uint32_t *d_offsets = nullptr, *d_spans = nullptr;
  int32_t *d_types = nullptr, *d_lengths = nullptr, *d_sample = nullptr, *d_span_labels = nullptr;
  int64_t *d_row_splits = nullptr, *d_span_splits = nullptr;
  for (int pass = 0; pass < 2; pass++) {
    d_offsets = a.take<uint32_t>(2 * cells);
    if (in.types) d_types = a.take<int32_t>(cells);
    if (in.lengths) d_lengths = a.take<int32_t>(in.n_rows);
    if (in.sample) d_sample = a.take<int32_t>(in.n_rows);
    if (ragged) d_row_splits = a.take<int64_t>(in.n_rows + 1);
    d_span_splits = a.take<int64_t>(in.n_samples + 1);
    d_spans = a.take<uint32_t>(2 * in.n_spans);
    if (in.span_labels) d_span_labels = a.take<int32_t>(in.n_spans);
    if (want & WP_ALIGN_LABELS) o.labels = a.take<int32_t>(cells);
    if (want & WP_ALIGN_SPAN_INDEX) o.span_index = a.take<int32_t>(cells);
    if (want & WP_ALIGN_POSITIONS) {
      o.start = a.take<int32_t>(in.n_rows);
      o.end = a.take<int32_t>(in.n_rows);
    }
    if (pass == 0) a.commit();
  }
  hipStream_t st = c->stream;
  a.arm(st);
  auto up = [&](void *dst, const void *src, size_t bytes) {
    if (bytes) WP_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st));
  };
  up(d_offsets, in.offsets, 2 * cells * sizeof(uint32_t));
  if (in.types) up(d_types, in.types, cells * sizeof(int32_t));
  if (in.lengths) up(d_lengths, in.lengths, in.n_rows * sizeof(int32_t));
  if (in.sample) up(d_sample, in.sample, in.n_rows * sizeof(int32_t));
  if (ragged) up(d_row_splits, in.row_splits, (in.n_rows + 1) * sizeof(int64_t));
  up(d_span_splits, in.span_splits, (in.n_samples + 1) * sizeof(int64_t));
  up(d_spans, in.spans, 2 * in.n_spans * sizeof(uint32_t));
  if (in.span_labels) up(d_span_labels, in.span_labels, in.n_spans * sizeof(int32_t));
  d.offsets = d_offsets;
  d.types = in.types ? d_types : nullptr;
  d.lengths = in.lengths ? d_lengths : nullptr;
  d.sample = in.sample ? d_sample : nullptr;
  d.row_splits = d_row_splits;
  d.span_splits = d_span_splits;
  d.spans = d_spans;
  d.span_labels = in.span_labels ? d_span_labels : nullptr;
  align_on_device(v, c, d, g, ragged, o, false);
  if (a.guard && !a.zones.empty()) {
    const uint32_t init[2] = {0u, 0xffffffffu};
    WP_HIP(hipMemcpyAsync(c->d_scalars + kScalarGuard, init, sizeof(init), hipMemcpyHostToDevice, st));
    a.check(st, c->d_scalars + kScalarGuard);
    queue_scalar_slots(c, kScalarGuardBad, kScalarGuardFirst, st);
    WP_HIP(hipStreamSynchronize(st));
    if (c->h_scalars[kScalarGuardBad] != 0) {
      throw HipError("arena guard: align: " + std::to_string(c->h_scalars[kScalarGuardBad]) + " guard zone(s) overwritten, first behind allocation #" +
                     std::to_string(c->h_scalars[kScalarGuardFirst] - 1));
    }
  }
  return o;
}

}  // namespace wp
