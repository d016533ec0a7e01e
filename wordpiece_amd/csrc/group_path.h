// group_path.h — what the layers that group items by a 64-bit key share on a context (word counts: count_path.h, the
// vocabulary learner: learn_path.h, duplicate rows: dedup_path.h, near-duplicate rows: neardup_path.h, and through
// window_path.h n-gram overlap: overlap_path.h and repeated spans: repeat_path.h; device side: group.h): the spec rules
// with one wording, the launch grid, the arena-guard check, the end check of the bounds-checking build, the stage timing
// of a call, the run heads of a sorted key list, the end of a collision round, a ragged batch on the device, the compact
// form and the table in front of it.
#pragma once
#include "context.h"
#include "group.h"

namespace wp {

static dim3 count_grid(size_t n) { return dim3(std::max(1u, cdiv(n, kBlock))); }

// ---- the rules of a spec that read the same in every layer, under the layer's prefix -----------------------------------
// known: the WANT bits of the layer, 2^b - 1; checked_hash_bits returns the bits of a key, 64 for 0; where: what follows
// "2^31 rows or more" in the layer's message ("", or " in " and the name of the offsets)
static void check_elem_bytes(const char *layer, int elem_bytes) {
  if (elem_bytes != 1 && elem_bytes != 4) throw std::invalid_argument(std::string(layer) + ": elem_bytes must be 1 or 4");
}
static void check_want(const char *layer, int want, int known) {
  if ((want & ~known) != 0) throw std::invalid_argument(std::string(layer) + ": want has bits outside " + std::to_string(known));
}
static int checked_hash_bits(const char *layer, int hash_bits) {
  if (hash_bits != 0 && (hash_bits < 8 || hash_bits > 64)) throw std::invalid_argument(std::string(layer) + ": hash_bits must be 0 (64) or in [8, 64]");
  return hash_bits == 0 ? 64 : hash_bits;
}
static void check_row_count(const char *layer, size_t n_rows, const char *where = "") {
  if (n_rows >= (size_t(1) << 31)) throw std::length_error(std::string(layer) + ": 2^31 rows or more" + where);
}

// the guard zones of one arena of the call, checked behind the kernels that wrote into it
static void check_arena_guard(Context *c, const Arena &a, hipStream_t st, const char *layer) {
  if (!a.guard || a.zones.empty()) return;
  const uint32_t init[2] = {0u, 0xffffffffu};
  WP_HIP(hipMemcpyAsync(c->d_scalars + kScalarGuard, init, sizeof(init), hipMemcpyHostToDevice, st));
  a.check(st, c->d_scalars + kScalarGuard);
  queue_scalar_slots(c, kScalarGuardBad, kScalarGuardFirst, st);
  WP_HIP(hipStreamSynchronize(st));
  if (c->h_scalars[kScalarGuardBad] != 0) {
    throw HipError(std::string("arena guard: ") + layer + ": " + std::to_string(c->h_scalars[kScalarGuardBad]) + " guard zone(s) overwritten, first behind allocation #" +
                   std::to_string(c->h_scalars[kScalarGuardFirst] - 1));
  }
}

// Behind the last kernel of a grouping layer's call, in the bounds-checking build: the layer's own site, the site the
// kernels of group.h count at whichever layer ran them, and where a layer runs another layer's kernels, that layer's
// site (`also`, with its text; -1: none).  All are taken before any of them fails the call, so nothing is left behind
// for the next one.
static void throw_if_group_oob(int site, const char *layer, const char *skipped, int also = -1, const char *also_skipped = "") {
#ifdef WP_DEBUG_BOUNDS
  unsigned int own = 0, shared = 0, other = 0;
  take_oob(site, 1, &own);
  take_oob(kSiteGroup, 1, &shared);
  if (also >= 0) take_oob(also, 1, &other);
  const std::string head = std::string("debug bounds: ") + layer + ": ";
  if (own != 0) throw HipError(head + std::to_string(own) + " " + skipped);
  if (other != 0) throw HipError(head + std::to_string(other) + " " + also_skipped);
  if (shared != 0) {
    throw HipError(head + std::to_string(shared) +
                   " stores or gathers outside the run, list, table or compact-form arrays of the shared grouping kernels skipped");
  }
#endif
}

// ---- WP_OPT_STAGE_TIMING ----------------------------------------------------------------------------------------------
// A timed call starts here: the radix statistics from zero, their spans on, kMarkStart recorded.  Returns what the sorts
// of the call report into (nullptr: the call is not timed).
static RadixStats *begin_stage_timing(Context *c, bool timing, hipStream_t st) {
  if (!timing) return nullptr;
  c->rstats.passes = 0;
  c->rstats.elems = 0;
  c->rstats.digit_bytes = 0;
  c->rstats.bytes = 0;
  c->rstats.spans.used = 0;
  c->rstats.spans.on = true;
  WP_HIP(hipEventRecord(c->ev[kMarkStart], st));
  return &c->rstats;
}
// ... and ends here, behind the last wait: the radix fields of wp_stats, the spans off
static void end_stage_timing(wp_vocab *v, Context *c) {
  v->stats.ms_radix_scatter = c->rstats.spans.resolve();
  v->stats.radix_passes = c->rstats.passes;
  v->stats.radix_pass_elems = c->rstats.elems;
  v->stats.radix_pass_bytes = c->rstats.bytes;
  c->rstats.spans.on = false;
}
static float mark_ms(Context *c, int from, int to) {
  float ms = 0;
  WP_HIP(hipEventElapsedTime(&ms, c->ev[from], c->ev[to]));
  return ms;
}
// the end of a call with all five marks: four stage times in the fields an encode times itself in (what each holds: the layer's section of the header)
static void end_four_stage_timing(wp_vocab *v, Context *c) {
  v->stats.ms_normalize = 0;
  v->stats.ms_decode = mark_ms(c, kMarkStart, kMarkCounted);
  v->stats.ms_sa = mark_ms(c, kMarkCounted, kMarkSorted);
  v->stats.ms_scan = mark_ms(c, kMarkSorted, kMarkScanned);
  v->stats.ms_walk = mark_ms(c, kMarkScanned, kMarkWalked);
  v->stats.ms_total = v->stats.ms_decode + v->stats.ms_sa + v->stats.ms_scan + v->stats.ms_walk;
  end_stage_timing(v, c);
}

// ---- the round protocol ----------------------------------------------------------------------------------
// The runs of m sorted keys: d_head[s] marks the first item of a run, d_run is the exclusive scan of the marks,
// d_head_pos[r] the position of the head of run r (and m behind the last), *d_runs the number of runs.
static void group_runs(const uint64_t *keys, size_t m, uint32_t *d_head, uint32_t *d_run, uint32_t *d_head_pos, uint32_t *d_stmp, uint32_t *d_runs,
                       hipStream_t st) {
  hipLaunchKernelGGL(group_heads_kernel, count_grid(m), dim3(kBlock), 0, st, keys, m, d_head);
  device_exclusive_scan(d_head, d_run, m, d_stmp, d_runs, st);
  hipLaunchKernelGGL(group_head_pos_kernel, count_grid(m), dim3(kBlock), 0, st, static_cast<const uint32_t *>(d_head), static_cast<const uint32_t *>(d_run),
                     m, static_cast<const uint32_t *>(d_runs), d_head_pos);
}

// out[pos[i]] = src ? src[i] : i for the flagged i < n, in order (out has room for n)
static void compact_flagged(const uint32_t *flag, const uint32_t *pos, size_t n, const uint32_t *src, uint32_t *out, hipStream_t st) {
  hipLaunchKernelGGL(group_compact_kernel, count_grid(n), dim3(kBlock), 0, st, flag, pos, n, src, out, n);
}

// The end of a collision round, in two steps so that a layer can queue work on `next` in front of the round's one wait.
// First the items the round's head comparison flagged in d_left go to `next`, in order, and their number to *d_nleft.
static void carry_leftovers(const uint32_t *d_left, uint32_t *d_left_pos, size_t m, const uint32_t *items, uint32_t *next, uint32_t *d_stmp,
                            uint32_t *d_nleft, hipStream_t st) {
  device_exclusive_scan(d_left, d_left_pos, m, d_stmp, d_nleft, st);
  compact_flagged(d_left, d_left_pos, m, items, next, st);
}
// Then the wait: it brings the scalar slots from slot_runs through slot_left.  Every run settles at least its head, so
// a round with no run or with nothing settled is an error.  Counts the round in the layer's statistics, leaves the
// leftovers in *m and returns the number of runs, each a new group.
template <typename Stats>
static size_t end_round(Context *c, int slot_runs, int slot_left, const char *layer, const char *noun, size_t *m, Stats *stats, hipStream_t st) {
  WP_LAUNCH_CHECK();
  queue_scalar_slots(c, slot_runs, slot_left, st);
  WP_HIP(hipStreamSynchronize(st));
  const size_t runs = c->h_scalars[slot_runs], left = c->h_scalars[slot_left];
  if (runs == 0 || left >= *m) throw HipError(std::string(layer) + ": a round settled no " + noun);
  if (stats->n_rounds == 0) stats->n_collided = static_cast<int64_t>(left);
  stats->n_rounds++;
  *m = left;
  return runs;
}

// ---- a ragged batch ---------------------------------------------------------------------------------------------------
// rows of elem_bytes-wide elements back to back at d_data, row r from d_row_off[r] to d_row_off[r + 1] (in elements)
struct RaggedIn {
  const void *d_data = nullptr;
  const long long *d_row_off = nullptr;
  size_t n_rows = 0;
  uint32_t elem_bytes = 1;
};

static void check_ragged_bytes(const char *layer, unsigned long long n_elems, uint32_t elem_bytes) {
  if (n_elems > static_cast<unsigned long long>(UINT32_MAX) / elem_bytes) throw std::length_error(std::string(layer) + ": the data has more than UINT32_MAX bytes");
}
static void throw_bad_row(const char *layer, size_t row, const char *off_name = "row_off") {
  throw std::invalid_argument(std::string(layer) + ": " + off_name + (row == 0 ? " must start at 0 and never descend: row 0" : " must never descend: row " + std::to_string(row)));
}

// the offsets of a batch in host memory, walked: returns the number of elements (off_name, data_name: what a message
// calls the two arrays of the batch)
static unsigned long long check_ragged_host(const char *layer, const void *data, const int64_t *row_off, size_t n_rows, uint32_t elem_bytes,
                                            const char *off_name = "row_off", const char *data_name = "data") {
  if (n_rows != 0 && row_off[0] != 0) throw_bad_row(layer, 0, off_name);
  for (size_t r = 0; r < n_rows; r++) {
    if (row_off[r + 1] < row_off[r]) throw_bad_row(layer, r, off_name);
  }
  const unsigned long long n_elems = n_rows ? static_cast<unsigned long long>(row_off[n_rows]) : 0ull;
  check_ragged_bytes(layer, n_elems, elem_bytes);
  if (n_elems != 0 && !data) throw std::invalid_argument(std::string(layer) + ": " + data_name + " is NULL");
  return n_elems;
}

// the batch of a host call into `buf`, data | row_off, on st (the data with the room of a text: the kernels read whole aligned words)
static RaggedIn upload_ragged(DeviceBuffer &buf, hipStream_t st, const void *data, const int64_t *row_off, size_t n_rows, size_t n_bytes, uint32_t elem_bytes) {
  Arena in(&buf);
  uint8_t *d_data = nullptr;
  long long *d_off = nullptr;
  for (int pass = 0; pass < 2; pass++) {
    d_data = in.take<uint8_t>(text_room(n_bytes));
    d_off = in.take<long long>(n_rows + 1);
    if (pass == 0) in.commit();
  }
  WP_HIP(hipMemcpyAsync(d_data, data, n_bytes, hipMemcpyHostToDevice, st));
  WP_HIP(hipMemcpyAsync(d_off, row_off, (n_rows + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
  return RaggedIn{d_data, d_off, n_rows, elem_bytes};
}

// what the layer's row kernel found, behind the wait that brought it: `bad` the first row whose offsets fail the check
// (kNoBadRow: none), n_elems the last offset.  Returns the bytes of the data.
static size_t check_ragged_device(const char *layer, const RaggedIn &in, uint32_t bad, unsigned long long n_elems, const char *off_name = "row_off",
                                  const char *data_name = "data") {
  if (bad != kNoBadRow) throw_bad_row(layer, bad, off_name);
  check_ragged_bytes(layer, n_elems, in.elem_bytes);
  if (n_elems != 0 && !in.d_data) throw std::invalid_argument(std::string(layer) + ": " + data_name + " is NULL");
  return static_cast<size_t>(n_elems) * in.elem_bytes;
}

// ---- the compact form ------------------------------------------------------------------------------------
// The n_kept rows d_kept of `in`, ascending, back to back.  d_out_len: their lengths in bytes and a 0 behind them;
// d_out_pos: room for the scan of the lengths; d_boff: the byte offsets of the rows of `in`.  Queues the offsets of the
// compact form (d_out_off, in elements), its rows (d_out, room: the n_bytes of the input) and the copy of its size in
// bytes into slot_out_bytes.  No wait: the caller's last one brings that slot.
static void compact_rows(Context *c, const RaggedIn &in, const uint32_t *d_boff, const int32_t *d_kept, size_t n_kept, size_t n_bytes, uint32_t *d_out_len,
                         uint32_t *d_out_pos, uint32_t *d_stmp, long long *d_out_off, uint32_t *d_out, int slot_out_bytes, hipStream_t st) {
  device_exclusive_scan(d_out_len, d_out_pos, n_kept + 1, d_stmp, nullptr, st);
  hipLaunchKernelGGL(group_out_off_kernel, count_grid(n_kept + 1), dim3(kBlock), 0, st, static_cast<const uint32_t *>(d_out_pos), n_kept, in.elem_bytes, d_out_off);
  if (n_bytes != 0 && n_kept != 0) {
    hipLaunchKernelGGL(group_gather_kernel, count_grid((n_bytes + 3) / 4), dim3(kBlock), 0, st, static_cast<const uint8_t *>(in.d_data), n_bytes, d_boff, d_kept,
                       static_cast<const uint32_t *>(d_out_pos), n_kept, in.n_rows, n_bytes, d_out);
  }
  // (the size of the compact form: the last entry of its offsets)
  WP_HIP(hipMemcpyAsync(c->d_scalars + slot_out_bytes, d_out_pos + n_kept, sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
}

// ---- the table in front of it ------------------------------------------------------------------------------------------
// device pointers into the output buffer of the call, with the arena that laid them out (for the caller's guard check)
struct GroupTable {
  Arena oa;
  int32_t *d_kept = nullptr, *d_inverse = nullptr;
  long long *d_counts = nullptr, *d_out_off = nullptr;
  uint32_t *d_out = nullptr;
  // into a layer's result, behind the caller's last wait (out_bytes: the word that wait brought from the out-bytes slot)
  template <typename Result>
  void hand_out(Result *R, size_t n_unique, bool want_compact, size_t out_bytes, uint32_t elem_bytes) const {
    R->kept = d_kept;
    R->counts = reinterpret_cast<int64_t *>(d_counts);
    R->inverse = d_inverse;
    R->n_unique = static_cast<int64_t>(n_unique);
    if (!want_compact) return;
    R->row_off = reinterpret_cast<int64_t *>(d_out_off);
    R->data = out_bytes ? d_out : nullptr;
    R->n_elems = static_cast<int64_t>(out_bytes / elem_bytes);
  }
};

// d_rep[i]: the representative of row i (itself where the row is kept); d_keep_pos: the scan of the kept flags;
// d_rcount: the rows each kept row stands for; d_boff: the byte offsets of the rows of `in`.  Lays `out` out, queues the
// table and with want_compact compact_rows over the n_unique >= 1 kept rows.  No wait.  d_out_len, d_out_pos: n_rows + 1
// words of scratch.
static GroupTable group_table(Context *c, const RaggedIn &in, const int32_t *d_rep, const uint32_t *d_keep_pos, const uint32_t *d_rcount, const uint32_t *d_boff,
                              size_t n_unique, size_t n_bytes, bool want_inverse, bool want_compact, DeviceBuffer *out, bool guard, uint32_t *d_out_len,
                              uint32_t *d_out_pos, uint32_t *d_stmp, int slot_out_bytes, hipStream_t st) {
  const size_t n = in.n_rows;
  GroupTable t{Arena(out, guard)};
  for (int pass = 0; pass < 2; pass++) {
    t.d_kept = t.oa.take<int32_t>(n_unique);
    t.d_counts = t.oa.take<long long>(n_unique);
    if (want_inverse) t.d_inverse = t.oa.take<int32_t>(n);
    if (want_compact) {
      t.d_out_off = t.oa.take<long long>(n_unique + 1);
      t.d_out = t.oa.take<uint32_t>(n_bytes / 4 + 1);
    }
    if (pass == 0) t.oa.commit();
  }
  t.oa.arm(st);
  hipLaunchKernelGGL(group_table_kernel, count_grid(n), dim3(kBlock), 0, st, d_rep, d_keep_pos, d_rcount, d_boff, n, n_unique, t.d_kept, t.d_counts,
                     t.d_inverse, want_compact ? d_out_len : static_cast<uint32_t *>(nullptr));
  if (want_compact) compact_rows(c, in, d_boff, t.d_kept, n_unique, n_bytes, d_out_len, d_out_pos, d_stmp, t.d_out_off, t.d_out, slot_out_bytes, st);
  return t;
}

}  // namespace wp
