// window_path.h — what the layers that work on the windows of a ragged batch share on a context (n-gram overlap:
// overlap_path.h, repeated spans: repeat_path.h; kernels: overlap.h): the window rule of the spec, the windows
// of a host batch, the per-row intake of a device batch, the window table and the kept rows with their compact form.
#pragma once
#include "context.h"
#include "group_path.h"
#include "overlap.h"

namespace wp {

static void check_ngram(const char *layer, int ngram) {
  if (ngram < 1 || ngram > kOvlMaxNgram) throw std::invalid_argument(std::string(layer) + ": ngram must be in [1, 64]");
}

// the windows of a batch in host memory (its offsets are checked)
static unsigned long long host_windows(const int64_t *row_off, size_t n_rows, uint32_t k) {
  unsigned long long w = 0;
  for (size_t r = 0; r < n_rows; r++) {
    const unsigned long long len = static_cast<unsigned long long>(row_off[r + 1] - row_off[r]);
    if (len >= k) w += len - k + 1;
  }
  return w;
}

static OvlPowers overlap_powers(uint32_t k) {
  OvlPowers pw{};
  uint64_t p = 1;
  for (int i = 0; i < kOvlItems; i++) p *= kOvlB;
  for (int i = 0; i < 6; i++) {
    pw.step[i] = p;
    p *= p;
  }
  pw.wave = p;  // (B^(kOvlItems * 64))
  pw.bk = 1;
  for (uint32_t i = 0; i < k; i++) pw.bk *= kOvlB;
  return pw;
}

// ---- the per-row intake of one batch ------------------------------------------------------------------------------------
// d_boff: the byte offsets of the rows; slot_bad: the first bad row (set to kNoBadRow by the caller); the 64-bit slots
// slot_elems and slot_windows (cleared by the caller): the elements and the windows of k elements
static void queue_window_rows(Context *c, const RaggedIn &in, uint32_t k, uint32_t *d_boff, int slot_bad, int slot_elems, int slot_windows, hipStream_t st) {
  hipLaunchKernelGGL(ovl_rows_kernel, count_grid(in.n_rows + 1), dim3(kBlock), 0, st, in.d_row_off, in.n_rows, in.elem_bytes, k, d_boff, c->d_scalars + slot_bad,
                     reinterpret_cast<unsigned long long *>(c->d_scalars + slot_elems), reinterpret_cast<unsigned long long *>(c->d_scalars + slot_windows));
}

struct WindowSizes {
  size_t n_bytes, n_elems, n_windows;
};
// ... and what it found, behind the layer's wait that brought the three slots
static WindowSizes read_window_rows(Context *c, const char *layer, const RaggedIn &in, int slot_bad, int slot_elems, int slot_windows,
                                    const char *off_name = "row_off", const char *data_name = "data") {
  unsigned long long elems, windows;
  std::memcpy(&elems, c->h_scalars + slot_elems, sizeof(elems));
  std::memcpy(&windows, c->h_scalars + slot_windows, sizeof(windows));
  const size_t n_bytes = check_ragged_device(layer, in, c->h_scalars[slot_bad], elems, off_name, data_name);
  if (windows > elems) throw HipError(std::string(layer) + ": more windows than elements");
  return WindowSizes{n_bytes, static_cast<size_t>(elems), static_cast<size_t>(windows)};
}

// ---- the window table --------------------------------------------------------------------------------------
// The arrays of the table of one batch and the two steps that fill them.  Between the steps the layer knows how many
// windows are listed: all of them, or what a wait of its own brought from the scan.
struct WindowTable {
  uint64_t *d_key = nullptr, *d_k0 = nullptr, *d_k1 = nullptr;
  uint32_t *d_valid = nullptr, *d_vpos = nullptr;  // per element: the flag of a listed window, the scan of the flags
  uint32_t *d_v0 = nullptr, *d_v1 = nullptr, *d_head = nullptr, *d_run = nullptr, *d_head_pos = nullptr, *d_differ = nullptr, *d_rep = nullptr,
           *d_entry = nullptr, *d_rtmp = nullptr;
  size_t tmp_words = 0;
  const uint64_t *keys = nullptr;  // behind group(): the listed windows sorted by key, stably: a run ascends by position
  const uint32_t *vals = nullptr;

  // both passes of the layer's arena loop call this: n_elems elements, at most n_windows listed windows
  void take(Arena &a, size_t n_elems, size_t n_windows) {
    tmp_words = radix_tmp_words<uint64_t>(n_windows);
    d_key = a.take<uint64_t>(n_elems);
    d_valid = a.take<uint32_t>(n_elems + 1);
    d_vpos = a.take<uint32_t>(n_elems + 1);
    d_k0 = a.take<uint64_t>(n_windows);
    d_k1 = a.take<uint64_t>(n_windows);
    d_v0 = a.take<uint32_t>(n_windows);
    d_v1 = a.take<uint32_t>(n_windows);
    d_head = a.take<uint32_t>(n_windows + 1);  // the run heads, then the scan of the entry flags
    d_run = a.take<uint32_t>(n_windows + 1);
    d_head_pos = a.take<uint32_t>(n_windows + 1);
    d_differ = a.take<uint32_t>(n_windows);
    d_rep = a.take<uint32_t>(n_windows);
    d_entry = a.take<uint32_t>(n_windows + 1);
    d_rtmp = a.take<uint32_t>(tmp_words);
  }  const uint32_t *entry_pos() const { return d_head; }

  // Step (a): the key of the window at every element (d_key) and the flag of those that are listed (d_valid; utf8: only
  // windows between code point boundaries), the scan of the flags (d_vpos), their number into *d_listed (may be nullptr).
  void list(const RaggedIn &in, size_t n_elems, const uint32_t *d_boff, uint32_t k, uint64_t mask, bool utf8, uint32_t *d_stmp, uint32_t *d_listed,
            hipStream_t st) {
    hipLaunchKernelGGL(ovl_keys_kernel, dim3(cdiv(n_elems, kOvlTile)), dim3(kBlock), 0, st, static_cast<const uint32_t *>(in.d_data), n_elems, d_boff, in.n_rows,
                       in.elem_bytes, k, overlap_powers(k), mask, d_key, d_valid, nullptr, nullptr, nullptr, 0u, size_t(0), nullptr, utf8 ? 1u : 0u);
    device_exclusive_scan(d_valid, d_vpos, n_elems + 1, d_stmp, d_listed, st);
  }

  // Step (b), for m >= 1 listed windows: the list, one stable sort by the low hash_bits of the key, the runs of equal
  // keys (their number into *d_runs), every member compared with the head of its run (d_differ; the counters of the
  // layer count the collisions), d_rep[s] the first member of the run with the bytes of member s, d_entry[s] set where s is
  // that member, and the scan of d_entry (entry_pos(), the distinct windows into *d_entries).
  void group(const RaggedIn &in, size_t n_elems, size_t n_bytes, size_t m, uint32_t k, int hash_bits, uint32_t *d_stmp, uint32_t *d_runs,
             unsigned long long *d_counters, uint32_t *d_entries, RadixStats *rs, hipStream_t st) {
    const uint32_t *d32 = static_cast<const uint32_t *>(in.d_data);
    const uint32_t eb = in.elem_bytes;
    hipLaunchKernelGGL(ovl_list_kernel, count_grid(n_elems), dim3(kBlock), 0, st, d_key, d_valid, d_vpos, n_elems, m, d_k0, d_v0);
    const int cur = radix_sort_pairs<uint64_t>(d_k0, d_v0, d_k1, d_v1, m, 0, hash_bits, d_rtmp, tmp_words, st, rs, false);
    keys = cur ? d_k1 : d_k0;
    vals = cur ? d_v1 : d_v0;
    group_runs(keys, m, d_head, d_run, d_head_pos, d_stmp, d_runs, st);
    hipLaunchKernelGGL(ovl_ref_head_kernel, count_grid(m), dim3(kBlock), 0, st, d32, n_bytes, vals, d_head, d_run, d_head_pos, m, eb, k, d_differ, d_counters);
    hipLaunchKernelGGL(ovl_ref_rep_kernel, count_grid(m), dim3(kBlock), 0, st, d32, n_bytes, vals, d_head, d_run, d_head_pos, d_differ, m, eb, k, d_rep, d_entry);
    device_exclusive_scan(d_entry, d_head, m + 1, d_stmp, d_entries, st);
  }
};

// ---- the kept rows and their compact form ---------------------------------------------------------------------------------
// d_keep[r]: row r stays (n_rows + 1 words, the last one 0).  The layer calls count() (one wait), take() in both passes of
// the loop over its output arena (room for the rows: the n_bytes of the input), queue() and, behind its last wait,
// hand_out() with the word that wait brought from slot_out_bytes.
struct KeptRows {
  size_t n_kept = 0;
  int32_t *d_kept = nullptr;
  long long *d_out_off = nullptr;
  uint32_t *d_out = nullptr;

  void count(Context *c, const char *layer, const uint32_t *d_keep, uint32_t *d_keep_pos, size_t n_rows, uint32_t *d_stmp, int slot_kept, hipStream_t st) {
    device_exclusive_scan(d_keep, d_keep_pos, n_rows + 1, d_stmp, c->d_scalars + slot_kept, st);
    queue_scalar_slots(c, slot_kept, slot_kept, st);
    WP_HIP(hipStreamSynchronize(st));
    n_kept = c->h_scalars[slot_kept];
    if (n_kept > n_rows) throw HipError(std::string(layer) + ": more kept rows than rows");
  }
  void take(Arena &oa, size_t n_bytes) {
    d_kept = oa.take<int32_t>(n_kept);
    d_out_off = oa.take<long long>(n_kept + 1);
    d_out = oa.take<uint32_t>(n_bytes / 4 + 1);
  }
  // the list of the kept rows, then compact_rows (group_path.h); d_out_len, d_out_pos: n_rows + 1 words of scratch
  void queue(Context *c, const RaggedIn &in, const uint32_t *d_keep, const uint32_t *d_keep_pos, const uint32_t *d_boff, size_t n_bytes, uint32_t *d_out_len,
             uint32_t *d_out_pos, uint32_t *d_stmp, int slot_out_bytes, hipStream_t st) {
    hipLaunchKernelGGL(ovl_kept_kernel, count_grid(in.n_rows), dim3(kBlock), 0, st, d_keep, d_keep_pos, d_boff, in.n_rows, n_kept, d_kept, d_out_len);
    compact_rows(c, in, d_boff, d_kept, n_kept, n_bytes, d_out_len, d_out_pos, d_stmp, d_out_off, d_out, slot_out_bytes, st);
  }
  template <typename Result>
  void hand_out(Result *R, size_t out_bytes, uint32_t elem_bytes) const {
    R->n_kept = static_cast<int64_t>(n_kept);
    R->kept = n_kept ? d_kept : nullptr;
    R->row_off = reinterpret_cast<int64_t *>(d_out_off);
    R->data = out_bytes ? d_out : nullptr;
    R->n_elems = static_cast<int64_t>(out_bytes / elem_bytes);
  }
};

}  // namespace wp
