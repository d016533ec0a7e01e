// seen_path.h — the persistent key set on a handle (include/wordpiece_amd_seen.h; kernels: seen.h): the argument rules,
// the table the handle owns and its growth, the launches of a call over rows or over given keys, the export, and the
// buffers of a call.  The intake, the run heads and the compact form are group_path.h's, the row keys dedup.h's.
#pragma once
#include "context.h"
#include "group_path.h"
#include "seen.h"

namespace wp {

struct SeenPlan {
  uint32_t elem_bytes = 1;
  bool want_keys = false, want_compact = false, query_only = false;
};

// every rule of the spec, each with the field it is about; nothing here needs a device (rows: a call over rows, else over keys)
static SeenPlan check_seen_spec(const wp_seen_spec *spec, const wp_seen_result *out, bool rows) {
  if (!spec) throw std::invalid_argument("seen: spec is NULL");
  if (!out) throw std::invalid_argument("seen: out is NULL");
  SeenPlan p;
  if (rows) {
    check_elem_bytes("seen", spec->elem_bytes);
    check_want("seen", spec->want, WP_SEEN_WANT_KEYS | WP_SEEN_WANT_COMPACT);
    p.elem_bytes = static_cast<uint32_t>(spec->elem_bytes);
  } else if (spec->want != 0) {
    throw std::invalid_argument("seen: want must be 0 in a call over keys");
  }
  if ((spec->flags & ~WP_SEEN_QUERY_ONLY) != 0) throw std::invalid_argument("seen: flags has bits outside 1");
  if (spec->pad != 0) throw std::invalid_argument("seen: pad must be 0");
  if (spec->reserved != 0) throw std::invalid_argument("seen: reserved must be 0");
  p.want_keys = rows && (spec->want & WP_SEEN_WANT_KEYS) != 0;
  p.want_compact = rows && (spec->want & WP_SEEN_WANT_COMPACT) != 0;
  p.query_only = (spec->flags & WP_SEEN_QUERY_ONLY) != 0;
  return p;
}

static wp_seen_stats &begin_seen_stats(wp_vocab *v, size_t n_rows) {
  v->seen.called = true;
  v->seen.last = wp_seen_stats{};
  v->seen.last.n_rows = static_cast<int64_t>(n_rows);
  return v->seen.last;
}

// ---- the table ----------------------------------------------------------------------------------------------------------
// frees the table on its device (the streams that used it have been waited for: every call ends with a wait)
static void seen_release(wp_vocab *v) {
  SeenSet &s = v->seen;
  if (s.d_slots || s.d_old) {
    DeviceGuard keep;
    (void)hipSetDevice(s.device);
    if (v->ctx) (void)hipStreamSynchronize(v->ctx->stream);
    free_dev(s.d_slots, s.d_old);
  }
  s.capacity = 0;
  s.n_keys = 0;
  s.n_grown = 0;
}

static uint32_t seen_log2(size_t capacity) { return static_cast<uint32_t>(bit_length(capacity) - 1); }

// the smallest table that keeps `keys` keys at a load of 1/2 or below
static size_t seen_slots_for(size_t keys) {
  if (keys > (size_t(1) << 30)) throw std::length_error("seen: the set would need more than 2^31 slots");
  size_t cap = WP_SEEN_MIN_SLOTS;
  while (cap < 2 * keys) cap <<= 1;
  return cap;
}

static uint64_t *seen_new_table(size_t capacity, hipStream_t st) {
  uint64_t *d = nullptr;
  WP_HIP(hipMalloc(&d, capacity * sizeof(uint64_t)));
  if (hipMemsetAsync(d, 0, capacity * sizeof(uint64_t), st) != hipSuccess) {
    (void)hipFree(d);
    throw HipError("seen: the new table could not be cleared");
  }
  return d;
}

static void seen_drop_old(wp_vocab *v) { free_dev(v->seen.d_old); }

// Room for `keys` keys, queued on c's stream with no wait: a table not yet made is made (at `first` slots at least), one
// that is too small is replaced by one that fits and its keys rehashed into it.  The old table stays in d_old until
// seen_drop_old, behind the caller's next wait.
static void seen_ensure(wp_vocab *v, Context *c, size_t keys, size_t first = WP_SEEN_MIN_SLOTS) {
  SeenSet &s = v->seen;
  hipStream_t st = c->stream;
  if (s.d_old) {  // (a call that failed behind its growth left it: nothing queued may still read it)
    WP_HIP(hipStreamSynchronize(st));
    seen_drop_old(v);
  }
  if (!s.d_slots) {
    s.d_slots = seen_new_table(first, st);
    s.capacity = first;
    s.device = c->device;
  }
  const size_t want = seen_slots_for(keys);
  if (want <= s.capacity) return;
  uint64_t *d_new = seen_new_table(want, st);
  hipLaunchKernelGGL(seen_rehash_kernel, count_grid(s.capacity), dim3(kBlock), 0, st, static_cast<const uint64_t *>(s.d_slots), s.capacity / kSeenGroup, d_new,
                     seen_log2(want), c->d_scalars + kScalarSeen);
  s.d_old = s.d_slots;
  s.d_slots = d_new;
  s.capacity = want;
  s.n_grown++;
}

// ---- a call --------------------------------------------------------------------------------------------------------------
// the per-item arrays of the sort, the runs and the table stage, for m items
struct SeenArrays {
  uint64_t *d_k0 = nullptr, *d_k1 = nullptr, *d_keys_out = nullptr;
  uint32_t *d_v0 = nullptr, *d_v1 = nullptr, *d_head = nullptr, *d_run = nullptr, *d_head_pos = nullptr, *d_found = nullptr, *d_rtmp = nullptr, *d_stmp = nullptr;
  int32_t *d_state = nullptr, *d_first = nullptr;
  size_t tmp_words = 0;
  void take(Arena &a, size_t m, bool want_keys) {
    tmp_words = radix_tmp_words<uint64_t>(m);
    d_k0 = a.take<uint64_t>(m);
    d_k1 = a.take<uint64_t>(m);
    if (want_keys) d_keys_out = a.take<uint64_t>(m);
    d_v0 = a.take<uint32_t>(m);
    d_v1 = a.take<uint32_t>(m);
    d_head = a.take<uint32_t>(m + 1);
    d_run = a.take<uint32_t>(m + 1);
    d_head_pos = a.take<uint32_t>(m + 1);
    d_found = a.take<uint32_t>(m + 1);
    d_state = a.take<int32_t>(m);
    d_first = a.take<int32_t>(m);
    d_rtmp = a.take<uint32_t>(tmp_words);
    d_stmp = a.take<uint32_t>(cdiv(m + 1, kScanTile) + 8);
  }
};

// The m >= 1 keys in A.d_k0 (none of them 0) against the set, on c's stream, no wait: the stable sort of (key, item), the
// runs, the growth where the table is too small, the lookup of the run heads, their insert unless the call only asks,
// and the state and first of every item.
static void seen_probe(wp_vocab *v, Context *c, const SeenArrays &A, size_t m, const SeenPlan &plan, bool timing, RadixStats *rs) {
  hipStream_t st = c->stream;
  uint32_t *d_counters = c->d_scalars + kScalarSeen, *d_runs = c->d_scalars + kScalarSeenRuns;
  const int cur = radix_sort_pairs<uint64_t>(A.d_k0, A.d_v0, A.d_k1, A.d_v1, m, 0, 64, A.d_rtmp, A.tmp_words, st, rs, true);
  const uint64_t *keys = cur ? A.d_k1 : A.d_k0;
  const uint32_t *vals = cur ? A.d_v1 : A.d_v0;
  group_runs(keys, m, A.d_head, A.d_run, A.d_head_pos, A.d_stmp, d_runs, st);
  if (timing) WP_HIP(hipEventRecord(c->ev[kMarkSorted], st));
  seen_ensure(v, c, v->seen.n_keys + (plan.query_only ? 0 : m));
  const uint32_t log2cap = seen_log2(v->seen.capacity);
  const dim3 probes(std::max(1u, cdiv(m, kSeenPerBlock)));
  // (the kernels that count stride a grid of kSeenGrid workgroups at the most: seen.h, seen_block_sum)
  const dim3 lookups(std::min(probes.x, kSeenGrid)), settles(std::min(count_grid(m).x, kSeenGrid));
  hipLaunchKernelGGL(seen_lookup_kernel, lookups, dim3(kBlock), 0, st, keys, static_cast<const uint32_t *>(A.d_head_pos), static_cast<const uint32_t *>(d_runs), m,
                     static_cast<const uint64_t *>(v->seen.d_slots), log2cap, A.d_found, d_counters);
  if (!plan.query_only) {
    hipLaunchKernelGGL(seen_insert_kernel, probes, dim3(kBlock), 0, st, keys, static_cast<const uint32_t *>(A.d_head_pos), static_cast<const uint32_t *>(d_runs), m,
                       static_cast<const uint32_t *>(A.d_found), v->seen.d_slots, log2cap, d_counters);
  }
  hipLaunchKernelGGL(seen_settle_kernel, settles, dim3(kBlock), 0, st, keys, vals, static_cast<const uint32_t *>(A.d_head),
                     static_cast<const uint32_t *>(A.d_run), static_cast<const uint32_t *>(A.d_head_pos), static_cast<const uint32_t *>(A.d_found), m, A.d_state,
                     A.d_first, A.d_keys_out, d_counters);
}

// behind the last wait of a call: the counters into the statistics and the host's count of the keys, the old table freed,
// and the checks that fail the call
static void seen_finish(wp_vocab *v, Context *c, size_t m, const SeenPlan &plan, wp_seen_stats &ss) {
  const uint32_t *k = c->h_scalars + kScalarSeen;
  seen_drop_old(v);
  ss.n_new = k[kSeenNew];
  ss.n_repeat_batch = k[kSeenRepeat];
  ss.n_seen_before = k[kSeenBefore];
  unsigned long long probes;
  std::memcpy(&probes, k + kSeenProbes, sizeof(probes));
  ss.n_probes = static_cast<int64_t>(probes);
  if (!plan.query_only) v->seen.n_keys += k[kSeenNew];
  if (k[kSeenRanOut] != 0) throw HipError("seen: " + std::to_string(k[kSeenRanOut]) + " probe(s) ran through the whole table");
  if (static_cast<size_t>(ss.n_new + ss.n_repeat_batch + ss.n_seen_before) != m) throw HipError("seen: the states do not add up to the rows");
  throw_if_group_oob(kSiteDedup, "seen rows", "stores or gathers outside the row, chunk, run or kept arrays skipped");
}

static void seen_stage_times(wp_vocab *v, Context *c) {
  const float keys = mark_ms(c, kMarkStart, kMarkCounted), sort = mark_ms(c, kMarkCounted, kMarkSorted), table = mark_ms(c, kMarkSorted, kMarkWalked);
  v->stats.ms_normalize = 0;
  v->stats.ms_decode = keys;
  v->stats.ms_sa = sort;
  v->stats.ms_walk = table;
  v->stats.ms_total = keys + sort + table;
  end_stage_timing(v, c);
}

// The rows of the batch `in` (n_rows >= 1), on c's stream.  The results are device pointers into c->seen_rows (state,
// first, keys) and c->seen_out (the compact form), valid until the handle's next call.  Waits: the sizes (the offset check,
// the elements, the chunks) and the one that ends the call (it brings the counters and the size of the compact form, whose
// room was the size of the input).  A growth adds none.
static void seen_rows_on_device(wp_vocab *v, Context *c, const RaggedIn &in, const SeenPlan &plan, wp_seen_result *R) {
  const size_t n = in.n_rows, n1 = n + 1;
  wp_seen_stats &ss = begin_seen_stats(v, n);
  *R = wp_seen_result{};
  R->n_rows = static_cast<int64_t>(n);
  hipStream_t st = c->stream;
  const bool guard = v->arena_guard || EnvOptions::get().arena_guard;
  const uint32_t eb = in.elem_bytes;
  // WP_OPT_STAGE_TIMING: kMarkStart, kMarkCounted (the keys are written), kMarkSorted (the runs are known), kMarkWalked
  const bool timing = v->stage_timing;
  RadixStats *rs = begin_stage_timing(c, timing, st);

  Arena ra(&c->seen_rows, guard);
  SeenArrays A;
  uint32_t *d_boff = nullptr, *d_nch = nullptr, *d_choff = nullptr, *d_items = nullptr, *d_keep = nullptr, *d_keep_pos = nullptr, *d_out_len = nullptr,
           *d_out_pos = nullptr;
  for (int pass = 0; pass < 2; pass++) {
    A.take(ra, n, plan.want_keys);
    d_boff = ra.take<uint32_t>(n1);
    d_nch = ra.take<uint32_t>(n1);
    d_choff = ra.take<uint32_t>(n1);
    d_items = ra.take<uint32_t>(n);
    if (plan.want_compact) {
      d_keep = ra.take<uint32_t>(n1);
      d_keep_pos = ra.take<uint32_t>(n1);
      d_out_len = ra.take<uint32_t>(n1);
      d_out_pos = ra.take<uint32_t>(n1);
    }
    if (pass == 0) ra.commit();
  }
  ra.arm(st);
  unsigned long long *d_elems = reinterpret_cast<unsigned long long *>(c->d_scalars + kScalarSeenElems);
  unsigned long long *d_chunks = reinterpret_cast<unsigned long long *>(c->d_scalars + kScalarSeenChunks);
  clear_scalars(c, kScalarSeenBad, kScalarSeen, st);
  WP_HIP(hipMemsetAsync(c->d_scalars + kScalarSeenBad, 0xff, sizeof(uint32_t), st));
  // (the row kernel of the dedup: byte offsets, chunks, the rows as the items of a round 0; its `first` is rewritten below)
  hipLaunchKernelGGL(dedup_rows_kernel, count_grid(n1), dim3(kBlock), 0, st, in.d_row_off, n, eb, d_boff, d_nch, d_items, A.d_first,
                     c->d_scalars + kScalarSeenBad, d_elems, reinterpret_cast<unsigned long long *>(c->d_scalars + kScalarSeenDedup));
  device_exclusive_scan(d_nch, d_choff, n1, A.d_stmp, nullptr, st, nullptr, d_chunks);
  WP_LAUNCH_CHECK();
  queue_scalar_slots(c, kScalarSeenBad, kScalarSeenChunks, st);
  WP_HIP(hipStreamSynchronize(st));
  unsigned long long elems64, chunks64;
  std::memcpy(&elems64, c->h_scalars + kScalarSeenElems, sizeof(elems64));
  std::memcpy(&chunks64, c->h_scalars + kScalarSeenChunks, sizeof(chunks64));
  const size_t n_bytes = check_ragged_device("seen", in, c->h_scalars[kScalarSeenBad], elems64);
  const size_t mc = static_cast<size_t>(chunks64);

  // ---- the keys: the dedup's round 0 at seed 0, then 0 -> 1 ----------------------------------------------------------------
  hipLaunchKernelGGL(dedup_key_init_kernel, count_grid(n), dim3(kBlock), 0, st, static_cast<const uint32_t *>(d_items), n, static_cast<const uint32_t *>(d_boff), n,
                     uint64_t(0), A.d_k0);
  if (mc != 0) {
    hipLaunchKernelGGL(dedup_keys_kernel, count_grid(mc), dim3(kBlock), 0, st, static_cast<const uint32_t *>(in.d_data), n_bytes,
                       static_cast<const uint32_t *>(d_boff), static_cast<const uint32_t *>(d_items), static_cast<const uint32_t *>(d_choff), n, mc, n, uint64_t(0),
                       reinterpret_cast<unsigned long long *>(A.d_k0));
  }
  hipLaunchKernelGGL(seen_keys_kernel, count_grid(n), dim3(kBlock), 0, st, static_cast<const uint64_t *>(A.d_k0), A.d_k0, n);
  if (timing) WP_HIP(hipEventRecord(c->ev[kMarkCounted], st));
  seen_probe(v, c, A, n, plan, timing, rs);

  // ---- the compact form: the new rows, counted on the device alone --------------------------------------------------------
  Arena oa(&c->seen_out, guard);
  int32_t *d_kept = nullptr;
  long long *d_out_off = nullptr;
  uint32_t *d_out = nullptr;
  if (plan.want_compact) {
    for (int pass = 0; pass < 2; pass++) {
      d_kept = oa.take<int32_t>(n);
      d_out_off = oa.take<long long>(n1);
      d_out = oa.take<uint32_t>(n_bytes / 4 + 1);
      if (pass == 0) oa.commit();
    }
    oa.arm(st);
    uint32_t *d_n_kept = c->d_scalars + kScalarSeenKept;
    hipLaunchKernelGGL(seen_keep_kernel, count_grid(n1), dim3(kBlock), 0, st, static_cast<const int32_t *>(A.d_state), n, d_keep);
    device_exclusive_scan(d_keep, d_keep_pos, n1, A.d_stmp, d_n_kept, st);
    hipLaunchKernelGGL(seen_kept_kernel, count_grid(n1), dim3(kBlock), 0, st, static_cast<const int32_t *>(A.d_state), static_cast<const uint32_t *>(d_keep_pos),
                       static_cast<const uint32_t *>(d_n_kept), static_cast<const uint32_t *>(d_boff), n, d_kept, d_out_len);
    // (over n entries: those behind the kept rows are empty and end where the data ends; seen.h, seen_kept_kernel)
    compact_rows(c, in, d_boff, d_kept, n, n_bytes, d_out_len, d_out_pos, A.d_stmp, d_out_off, d_out, kScalarSeenOutBytes, st);
  }
  WP_LAUNCH_CHECK();
  if (timing) WP_HIP(hipEventRecord(c->ev[kMarkWalked], st));
  queue_scalar_slots(c, kScalarSeenRuns, kScalarSeen, st);
  WP_HIP(hipStreamSynchronize(st));
  seen_finish(v, c, n, plan, ss);
  if (timing) seen_stage_times(v, c);
  if (plan.want_compact && c->h_scalars[kScalarSeenKept] != static_cast<uint32_t>(ss.n_new)) throw HipError("seen: the kept rows are not the new ones");
  check_arena_guard(c, ra, st, "seen");
  check_arena_guard(c, oa, st, "seen");
  ss.n_keys = static_cast<int64_t>(v->seen.n_keys);
  R->state = A.d_state;
  R->first = A.d_first;
  R->keys = A.d_keys_out;
  if (plan.want_compact) {
    const size_t out_bytes = c->h_scalars[kScalarSeenOutBytes];
    R->kept = d_kept;
    R->n_kept = ss.n_new;
    R->row_off = reinterpret_cast<int64_t *>(d_out_off);
    R->data = out_bytes ? d_out : nullptr;
    R->n_elems = static_cast<int64_t>(out_bytes / eb);
  }
}

// The n >= 1 keys at d_keys, on c's stream: state and first per key, in c->seen_rows.  One wait, the one that ends the call.
static void seen_keys_on_device(wp_vocab *v, Context *c, const uint64_t *d_keys, size_t n, const SeenPlan &plan, wp_seen_result *R) {
  wp_seen_stats &ss = begin_seen_stats(v, n);
  *R = wp_seen_result{};
  R->n_rows = static_cast<int64_t>(n);
  hipStream_t st = c->stream;
  const bool guard = v->arena_guard || EnvOptions::get().arena_guard;
  const bool timing = v->stage_timing;
  RadixStats *rs = begin_stage_timing(c, timing, st);
  Arena ra(&c->seen_rows, guard);
  SeenArrays A;
  for (int pass = 0; pass < 2; pass++) {
    A.take(ra, n, false);
    if (pass == 0) ra.commit();
  }
  ra.arm(st);
  clear_scalars(c, kScalarSeenBad, kScalarSeen, st);
  hipLaunchKernelGGL(seen_keys_kernel, count_grid(n), dim3(kBlock), 0, st, d_keys, A.d_k0, n);
  if (timing) WP_HIP(hipEventRecord(c->ev[kMarkCounted], st));
  seen_probe(v, c, A, n, plan, timing, rs);
  WP_LAUNCH_CHECK();
  if (timing) WP_HIP(hipEventRecord(c->ev[kMarkWalked], st));
  queue_scalar_slots(c, kScalarSeenRuns, kScalarSeen, st);
  WP_HIP(hipStreamSynchronize(st));
  seen_finish(v, c, n, plan, ss);
  if (timing) seen_stage_times(v, c);
  check_arena_guard(c, ra, st, "seen");
  ss.n_keys = static_cast<int64_t>(v->seen.n_keys);
  R->state = A.d_state;
  R->first = A.d_first;
}

// The keys of the set, ascending, into c->seen_rows: the slots that hold one compacted in slot order, then sorted.  Returns
// the device pointer to the n_keys >= 1 keys; the caller copies them out and waits.
static const uint64_t *seen_export_on_device(wp_vocab *v, Context *c) {
  const SeenSet &s = v->seen;
  const size_t cap = s.capacity, nk = s.n_keys;
  hipStream_t st = c->stream;
  const bool guard = v->arena_guard || EnvOptions::get().arena_guard;
  Arena ra(&c->seen_rows, guard);
  const size_t tmp_words = radix_tmp_words<uint64_t>(nk);
  uint64_t *d_k0 = nullptr, *d_k1 = nullptr;
  uint32_t *d_v0 = nullptr, *d_v1 = nullptr, *d_flag = nullptr, *d_pos = nullptr, *d_rtmp = nullptr, *d_stmp = nullptr;
  for (int pass = 0; pass < 2; pass++) {
    d_k0 = ra.take<uint64_t>(nk);
    d_k1 = ra.take<uint64_t>(nk);
    d_v0 = ra.take<uint32_t>(nk);
    d_v1 = ra.take<uint32_t>(nk);
    d_flag = ra.take<uint32_t>(cap + 1);
    d_pos = ra.take<uint32_t>(cap + 1);
    d_rtmp = ra.take<uint32_t>(tmp_words);
    d_stmp = ra.take<uint32_t>(cdiv(cap + 1, kScanTile) + 8);
    if (pass == 0) ra.commit();
  }
  ra.arm(st);
  hipLaunchKernelGGL(seen_flag_kernel, count_grid(cap + 1), dim3(kBlock), 0, st, static_cast<const uint64_t *>(s.d_slots), cap, d_flag);
  device_exclusive_scan(d_flag, d_pos, cap + 1, d_stmp, c->d_scalars + kScalarSeenKept, st);
  hipLaunchKernelGGL(seen_scatter_kernel, count_grid(cap), dim3(kBlock), 0, st, static_cast<const uint64_t *>(s.d_slots), cap, static_cast<const uint32_t *>(d_flag),
                     static_cast<const uint32_t *>(d_pos), d_k0, nk);
  const int cur = radix_sort_pairs<uint64_t>(d_k0, d_v0, d_k1, d_v1, nk, 0, 64, d_rtmp, tmp_words, st, nullptr, true);
  WP_LAUNCH_CHECK();
  queue_scalar_slots(c, kScalarSeenKept, kScalarSeenKept, st);
  WP_HIP(hipStreamSynchronize(st));
  if (c->h_scalars[kScalarSeenKept] != nk) throw HipError("seen: the table does not hold the keys the host counted");
  throw_if_group_oob(kSiteDedup, "seen export", "stores outside the key array skipped");
  check_arena_guard(c, ra, st, "seen");
  return cur ? d_k1 : d_k0;
}

}  // namespace wp
