// repeat_path.h — the repeated-span search on a context (include/wordpiece_amd.h, section "repeated spans"; kernels:
// repeat.h, and overlap.h for the windows and their grouping): the argument rules, the answer of a call without windows,
// the launches over one device batch and the buffers of a call.  Shared with overlap_path.h, in window_path.h: the intake,
// the window table, the kept rows.
#pragma once
#include <algorithm>

#include "context.h"
#include "repeat.h"
#include "window_path.h"

namespace wp {

// the spec of a call with its defaults filled in
struct RepeatPlan {
  uint32_t elem_bytes = 1, ngram = 50, scope = 0, max_repeats = 0;
  int hash_bits = 64;
  bool want_mask = false, want_src = false, want_compact = false, want_cut = false, utf8 = false;
};

// every rule of the spec, each with the field it is about; nothing here needs a device
static RepeatPlan check_repeat_spec(const wp_repeat_spec *spec, const wp_repeat_result *out) {
  if (!spec) throw std::invalid_argument("repeat: spec is NULL");
  if (!out) throw std::invalid_argument("repeat: out is NULL");
  check_elem_bytes("repeat", spec->elem_bytes);
  check_want("repeat", spec->want, WP_REPEAT_WANT_MASK | WP_REPEAT_WANT_SRC | WP_REPEAT_WANT_COMPACT | WP_REPEAT_WANT_CUT);
  check_ngram("repeat", spec->ngram);
  if (spec->scope != 0 && spec->scope != 1) throw std::invalid_argument("repeat: scope must be 0 (anywhere) or 1 (earlier rows)");
  if (spec->max_repeats < 0) throw std::invalid_argument("repeat: max_repeats must not be negative");
  const int hash_bits = checked_hash_bits("repeat", spec->hash_bits);
  if ((spec->flags & ~WP_REPEAT_UTF8) != 0) throw std::invalid_argument("repeat: flags has bits outside WP_REPEAT_UTF8");
  if ((spec->flags & WP_REPEAT_UTF8) != 0 && spec->elem_bytes != 1) throw std::invalid_argument("repeat: flags: WP_REPEAT_UTF8 needs elem_bytes 1");
  if (spec->reserved != 0) throw std::invalid_argument("repeat: reserved must be 0");
  RepeatPlan p;
  p.elem_bytes = static_cast<uint32_t>(spec->elem_bytes);
  p.ngram = static_cast<uint32_t>(spec->ngram);
  p.scope = static_cast<uint32_t>(spec->scope);
  p.max_repeats = static_cast<uint32_t>(spec->max_repeats);
  p.hash_bits = hash_bits;
  p.want_mask = (spec->want & WP_REPEAT_WANT_MASK) != 0;
  p.want_src = (spec->want & WP_REPEAT_WANT_SRC) != 0;
  p.want_compact = (spec->want & WP_REPEAT_WANT_COMPACT) != 0;
  p.want_cut = (spec->want & WP_REPEAT_WANT_CUT) != 0;
  p.utf8 = (spec->flags & WP_REPEAT_UTF8) != 0;
  return p;
}

// the pointer and the row count of the batch
static void check_repeat_rows(const void *row_off, size_t n_rows) {
  if (n_rows != 0 && !row_off) throw std::invalid_argument("repeat: row_off is NULL");
  check_row_count("repeat", n_rows, " in row_off");
}

// the statistics of a repeat call before anything is known of its rows
static wp_repeat_stats &begin_repeat_stats(wp_vocab *v, size_t n_rows) {
  v->stats.repeat_call = 1;
  v->stats.repeat = wp_repeat_stats{};
  v->stats.repeat.n_rows = static_cast<int64_t>(n_rows);
  return v->stats.repeat;
}

// A host call whose batch has no window (n_rows >= 1): no device needed.  Nothing repeats: every row is kept and the cut
// is the input.
static wp_repeat_result repeat_no_window(wp_vocab *v, const RepeatPlan &plan, const void *data, const int64_t *row_off, size_t n_rows) {
  wp_repeat_stats &rs = begin_repeat_stats(v, n_rows);
  const size_t n_elems = static_cast<size_t>(row_off[n_rows]);
  rs.n_elems = static_cast<int64_t>(n_elems);
  wp_repeat_result h{};
  h.n_rows = static_cast<int64_t>(n_rows);
  h.repeats = static_cast<int64_t *>(zeroed(n_rows * sizeof(int64_t)));
  h.covered = static_cast<int64_t *>(zeroed(n_rows * sizeof(int64_t)));
  h.first_repeat = static_cast<int64_t *>(zeroed(n_rows * sizeof(int64_t)));
  h.first_src_pos = static_cast<int64_t *>(zeroed(n_rows * sizeof(int64_t)));
  h.first_src_row = static_cast<int32_t *>(zeroed(n_rows * sizeof(int32_t)));
  for (size_t r = 0; r < n_rows; r++) {
    h.first_repeat[r] = h.first_src_pos[r] = -1;
    h.first_src_row[r] = -1;
  }
  if (plan.want_mask && n_elems != 0) h.mask = static_cast<uint8_t *>(zeroed(n_elems));
  if (plan.want_src && n_elems != 0) {
    h.src = static_cast<int64_t *>(zeroed(n_elems * sizeof(int64_t)));
    std::fill(h.src, h.src + n_elems, int64_t(-1));
  }
  auto whole = [&](int64_t **off, void **out) {
    *off = static_cast<int64_t *>(zeroed((n_rows + 1) * sizeof(int64_t)));
    std::memcpy(*off, row_off, (n_rows + 1) * sizeof(int64_t));
    if (n_elems != 0) {
      *out = zeroed(n_elems * plan.elem_bytes);
      std::memcpy(*out, data, n_elems * plan.elem_bytes);
    }
  };
  if (plan.want_compact) {
    h.n_kept = static_cast<int64_t>(n_rows);
    h.n_elems = static_cast<int64_t>(n_elems);
    h.kept = static_cast<int32_t *>(zeroed(n_rows * sizeof(int32_t)));
    for (size_t r = 0; r < n_rows; r++) h.kept[r] = static_cast<int32_t>(r);
    whole(&h.row_off, &h.data);
  }
  if (plan.want_cut) {
    h.n_cut_elems = static_cast<int64_t>(n_elems);
    rs.n_cut_elems = h.n_cut_elems;
    whole(&h.cut_off, &h.cut_data);
  }
  return h;
}

// The batch `in` (n_rows >= 1) against itself, on c's stream.  The results are device pointers into c->repeat_rows (the
// per-row arrays), c->repeat_items (mask, src) and c->repeat_out (the cut and the compact form), valid until the
// handle's next call.  Waits: the sizes (the offset check, the elements, the windows), with WP_REPEAT_UTF8 the eligible
// windows, with WP_REPEAT_WANT_COMPACT the kept count, and the one that ends the call: by the spec, whatever the data
// holds and however the keys collide.  Every array is sized by the elements or by the windows the first wait brought.
static void repeat_on_device(wp_vocab *v, Context *c, const RaggedIn &in, const RepeatPlan &plan, wp_repeat_result *R) {
  const size_t n = in.n_rows;
  wp_repeat_stats &ps = begin_repeat_stats(v, n);
  *R = wp_repeat_result{};
  R->n_rows = static_cast<int64_t>(n);
  hipStream_t st = c->stream;
  const bool guard = v->arena_guard || EnvOptions::get().arena_guard;
  const uint32_t eb = in.elem_bytes, k = plan.ngram;
  // WP_OPT_STAGE_TIMING: kMarkStart, kMarkCounted (offsets checked), kMarkSorted (keys, sort, runs, first occurrences),
  // kMarkScanned (repeat flags, cover), kMarkWalked (per-row results, cut, compact form)
  const bool timing = v->stage_timing;
  RadixStats *rs = begin_stage_timing(c, timing, st);

  // ---- the per-row arrays, the offset check --------------------------------------------------------------------------------
  const size_t n1 = n + 1;
  Arena ra(&c->repeat_rows, guard);
  uint32_t *d_boff = nullptr, *d_keep = nullptr, *d_keep_pos = nullptr, *d_out_len = nullptr, *d_out_pos = nullptr, *d_stmp = nullptr;
  long long *d_repeats = nullptr, *d_first_repeat = nullptr, *d_first_src_pos = nullptr, *d_covered = nullptr;
  int32_t *d_first_src_row = nullptr;
  for (int pass = 0; pass < 2; pass++) {
    d_boff = ra.take<uint32_t>(n1);
    d_repeats = ra.take<long long>(n);
    d_first_repeat = ra.take<long long>(n);
    d_first_src_pos = ra.take<long long>(n);
    d_covered = ra.take<long long>(n);
    d_first_src_row = ra.take<int32_t>(n);
    d_keep = ra.take<uint32_t>(n1);
    d_keep_pos = ra.take<uint32_t>(n1);
    d_out_len = ra.take<uint32_t>(n1);
    d_out_pos = ra.take<uint32_t>(n1);
    d_stmp = ra.take<uint32_t>(cdiv(n1, kScanTile) + 8);
    if (pass == 0) ra.commit();
  }
  ra.arm(st);
  unsigned long long *d_counters = reinterpret_cast<unsigned long long *>(c->d_scalars + kScalarRep);
  clear_scalars(c, kScalarRepBad, kScalarRep, st);
  WP_HIP(hipMemsetAsync(c->d_scalars + kScalarRepBad, 0xff, sizeof(uint32_t), st));
  queue_window_rows(c, in, k, d_boff, kScalarRepBad, kScalarRepElems, kScalarRepWindows, st);
  WP_LAUNCH_CHECK();
  if (timing) WP_HIP(hipEventRecord(c->ev[kMarkCounted], st));
  queue_scalar_slots(c, kScalarRepBad, kScalarRepWindows, st);
  WP_HIP(hipStreamSynchronize(st));
  const WindowSizes sizes = read_window_rows(c, "repeat", in, kScalarRepBad, kScalarRepElems, kScalarRepWindows);
  const size_t n_bytes = sizes.n_bytes, ne = sizes.n_elems, nw = sizes.n_windows;
  ps.n_elems = static_cast<int64_t>(ne);
  const uint32_t *d32 = static_cast<const uint32_t *>(in.d_data);

  // ---- the per-element and per-window arrays -------------------------------------------------------------------------------
  const int hb = plan.hash_bits;
  const uint64_t mask = hb >= 64 ? ~0ull : (1ull << hb) - 1ull;
  const size_t ne1 = ne + 1, nw1 = nw + 1;
  Arena ia(&c->repeat_items, guard);
  WindowTable t;  // of the batch itself
  uint32_t *d_first = nullptr, *d_hit = nullptr, *d_H = nullptr, *d_cover = nullptr, *d_C = nullptr, *d_itmp = nullptr;
  uint8_t *d_mask = nullptr;
  long long *d_src = nullptr;
  for (int pass = 0; pass < 2; pass++) {
    d_first = ia.take<uint32_t>(ne);  // the first occurrence of the window at an element
    d_hit = ia.take<uint32_t>(ne1);
    d_H = ia.take<uint32_t>(ne1);
    d_cover = ia.take<uint32_t>(ne1);
    d_C = ia.take<uint32_t>(ne1);
    if (plan.want_mask) d_mask = ia.take<uint8_t>(ne);
    if (plan.want_src) d_src = ia.take<long long>(ne);
    t.take(ia, ne, nw);
    d_itmp = ia.take<uint32_t>(cdiv(std::max(ne1, nw1), kScanTile) + 8);
    if (pass == 0) ia.commit();
  }
  ia.arm(st);

  // ---- the window table of the batch; the first member of a run with the same bytes is the first occurrence -----------------
  size_t m = 0;  // the listed windows
  if (ne != 0) WP_HIP(hipMemsetAsync(d_first, 0xff, ne * sizeof(uint32_t), st));  // (kRepNone)
  if (nw != 0) {
    t.list(in, ne, d_boff, k, mask, plan.utf8, d_itmp, c->d_scalars + kScalarRepListed, st);
    m = nw;
    if (plan.utf8) {  // (the eligible windows are known to the device alone)
      queue_scalar_slots(c, kScalarRepListed, kScalarRepListed, st);
      WP_HIP(hipStreamSynchronize(st));
      m = c->h_scalars[kScalarRepListed];
      if (m > nw) throw HipError("repeat: more eligible windows than windows");
    }
  }
  if (m != 0) {
    t.group(in, ne, n_bytes, m, k, hb, d_itmp, c->d_scalars + kScalarRepRuns, d_counters, c->d_scalars + kScalarRepDistinct, rs, st);
    hipLaunchKernelGGL(rep_back_kernel, count_grid(m), dim3(kBlock), 0, st, t.vals, t.d_rep, m, ne, d_first);
    WP_LAUNCH_CHECK();
  }
  if (timing) WP_HIP(hipEventRecord(c->ev[kMarkSorted], st));

  // ---- the repeat flags, their scan, the cover pass ------------------------------------------------------------------------
  WP_HIP(hipMemsetAsync(d_hit + ne, 0, sizeof(uint32_t), st));
  WP_HIP(hipMemsetAsync(d_cover + ne, 0, sizeof(uint32_t), st));
  WP_HIP(hipMemsetAsync(d_first_repeat, 0xff, n * sizeof(long long), st));  // (-1)
  WP_HIP(hipMemsetAsync(d_first_src_pos, 0xff, n * sizeof(long long), st));
  WP_HIP(hipMemsetAsync(d_first_src_row, 0xff, n * sizeof(int32_t), st));
  if (ne != 0) hipLaunchKernelGGL(rep_flag_kernel, dim3(cdiv(ne, kRepTile)), dim3(kBlock), 0, st, d_first, d_boff, n, ne, eb, plan.scope, d_hit, d_src);
  device_exclusive_scan(d_hit, d_H, ne1, d_itmp, c->d_scalars + kScalarRepRepeats, st);
  if (ne != 0) {
    hipLaunchKernelGGL(rep_cover_kernel, dim3(cdiv(ne, kRepTile)), dim3(kBlock), 0, st, d_hit, d_H, d_first, d_boff, n, ne, eb, k, d_cover, d_mask,
                       d_first_repeat, d_first_src_row, d_first_src_pos);
  }
  device_exclusive_scan(d_cover, d_C, ne1, d_itmp, c->d_scalars + kScalarRepCovered, st);
  WP_LAUNCH_CHECK();
  if (timing) WP_HIP(hipEventRecord(c->ev[kMarkScanned], st));

  // ---- the per-row results, the cut, the compact form ----------------------------------------------------------------------
  hipLaunchKernelGGL(ovl_row_results_kernel, count_grid(n1), dim3(kBlock), 0, st, d_H, d_C, d_boff, n, eb, plan.max_repeats, d_repeats, d_covered, d_keep,
                     d_counters);
  WP_LAUNCH_CHECK();
  KeptRows kept;
  if (plan.want_compact) kept.count(c, "repeat", d_keep, d_keep_pos, n, d_stmp, kScalarRepKept, st);
  Arena oa(&c->repeat_out, guard);
  long long *d_cut_off = nullptr;
  uint32_t *d_cut = nullptr;
  for (int pass = 0; pass < 2 && (plan.want_compact || plan.want_cut); pass++) {
    if (plan.want_compact) kept.take(oa, n_bytes);
    if (plan.want_cut) {
      d_cut_off = oa.take<long long>(n1);
      d_cut = oa.take<uint32_t>(n_bytes / 4 + 1);
    }
    if (pass == 0) oa.commit();
  }
  if (plan.want_compact || plan.want_cut) oa.arm(st);
  if (plan.want_cut) {
    hipLaunchKernelGGL(rep_cut_off_kernel, count_grid(n1), dim3(kBlock), 0, st, d_C, d_boff, n, ne, eb, d_cut_off);
    if (ne != 0 && eb == 4) {
      hipLaunchKernelGGL(rep_cut_ids_kernel, count_grid(ne), dim3(kBlock), 0, st, d32, d_cover, d_C, ne, d_cut);
    } else if (ne != 0) {
      hipLaunchKernelGGL(rep_cut_bytes_kernel, dim3(cdiv(ne, kRepCutTile)), dim3(kBlock), 0, st, d32, d_cover, d_C, ne, n_bytes, d_cut);
    }
    WP_LAUNCH_CHECK();
  }
  if (plan.want_compact) {
    kept.queue(c, in, d_keep, d_keep_pos, d_boff, n_bytes, d_out_len, d_out_pos, d_stmp, kScalarRepOutBytes, st);
    WP_LAUNCH_CHECK();
  }
  if (timing) WP_HIP(hipEventRecord(c->ev[kMarkWalked], st));
  queue_scalar_slots(c, kScalarRepListed, kScalarRep, st);
  WP_HIP(hipStreamSynchronize(st));
  unsigned long long counters[kRepCounters];
  std::memcpy(counters, c->h_scalars + kScalarRep, sizeof(counters));
  const size_t n_covered = c->h_scalars[kScalarRepCovered];
  if (n_covered > ne) throw HipError("repeat: more covered elements than elements");
  ps.n_windows = static_cast<int64_t>(m);
  ps.n_distinct = static_cast<int64_t>(m != 0 ? c->h_scalars[kScalarRepDistinct] : 0);
  ps.n_repeats = static_cast<int64_t>(c->h_scalars[kScalarRepRepeats]);
  ps.n_covered = static_cast<int64_t>(n_covered);
  ps.n_repeat_rows = static_cast<int64_t>(counters[kRepRepeatRows]);
  ps.n_collided = static_cast<int64_t>(counters[kRepCollided]);
  ps.n_cut_elems = plan.want_cut ? static_cast<int64_t>(ne - n_covered) : 0;
  if (timing) end_four_stage_timing(v, c);  // (check, grouping, cover, rows: the header's section)
  // (kSiteOverlap: overlap.h's kernels run here too)
  throw_if_group_oob(kSiteRepeat, "repeated spans", "gathers or stores outside the element, window or cut arrays skipped", kSiteOverlap,
                     "gathers or stores outside the window or result arrays skipped");
  check_arena_guard(c, ra, st, "repeat");
  check_arena_guard(c, ia, st, "repeat");
  check_arena_guard(c, oa, st, "repeat");
  R->repeats = reinterpret_cast<int64_t *>(d_repeats);
  R->first_repeat = reinterpret_cast<int64_t *>(d_first_repeat);
  R->first_src_pos = reinterpret_cast<int64_t *>(d_first_src_pos);
  R->covered = reinterpret_cast<int64_t *>(d_covered);
  R->first_src_row = d_first_src_row;
  if (plan.want_mask && ne != 0) R->mask = d_mask;
  if (plan.want_src && ne != 0) R->src = reinterpret_cast<int64_t *>(d_src);
  if (plan.want_compact) kept.hand_out(R, c->h_scalars[kScalarRepOutBytes], eb);
  if (plan.want_cut) {
    R->n_cut_elems = ps.n_cut_elems;
    R->cut_off = reinterpret_cast<int64_t *>(d_cut_off);
    R->cut_data = ps.n_cut_elems ? d_cut : nullptr;
  }
}

}  // namespace wp
