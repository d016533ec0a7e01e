// rows_path.h — the documents layer on a context (include/wordpiece_amd.h, section "documents"; kernels: rows.h): the
// rows of a text through the joined route (linear_path.h, RowsCall) or document by document, and the padded batch of a
// rows result.
#pragma once
#include "context.h"
#include "linear_path.h"
#include "rows.h"

namespace wp {

struct RowsResult {  // device pointers, valid until the handle's next call
  const int32_t *d_ids = nullptr;
  const long long *d_row_splits = nullptr;
  const uint32_t *d_offs = nullptr;
  size_t n_ids = 0, n_rows = 0;
};

// A vocabulary that can match differently inside a joined text than in a document of its own: an eligible token with
// U+000A matches across the separator; a token with U+0000 / U+0001 can match into the 1 . vocab tail of S, which only
// the end of a text has; with duplicate eligible lines the copy a match at the end of a text names depends on what
// follows it.  Such batches are encoded document by document.
static bool rows_per_document(const wp_vocab *v) { return v->hv.newline_in_token || v->hv.low_cp || v->hv.n_dup_eligible > 0; }

static void check_rows_call(int unit, size_t nbytes) {
  if (unit != -1 && unit != WP_OFFSETS_BYTES && unit != WP_OFFSETS_CODE_POINTS) {
    throw std::invalid_argument("offsets unit must be -1 (none), 0 (bytes) or 1 (code points)");
  }
  // (row membership goes through the 32-bit first-byte table of the code points in every unit)
  if (nbytes > static_cast<size_t>(UINT32_MAX)) throw std::length_error("a documents call needs nbytes <= UINT32_MAX");
}

static int padded_specials(int max_len, int32_t cls_id, int32_t sep_id) {
  const int specials = (cls_id >= 0 ? 1 : 0) + (sep_id >= 0 ? 1 : 0);
  if (max_len < 1 || max_len < specials) throw std::invalid_argument("max_len must be at least 1 and at least the number of specials");
  return specials;
}

static void check_doc_off_host(const char *utf8, size_t nbytes, const int64_t *doc_off, size_t n_docs) {
  bool ok = doc_off[0] == 0 && static_cast<uint64_t>(doc_off[n_docs]) == nbytes && doc_off[n_docs] >= 0;
  for (size_t i = 1; ok && i <= n_docs; i++) {
    ok = doc_off[i] > doc_off[i - 1] && static_cast<uint64_t>(doc_off[i]) <= nbytes && utf8[doc_off[i] - 1] == '\n';
  }
  if (!ok) throw std::invalid_argument("document offsets must increase from 0 to nbytes with a '\\n' in front of each");
}

// The per-document route: the rows' starts come to the host (explicit: checked and copied; lines: found by the kernels
// of the joined route), every document is copied into the context's second text buffer (a document starts at any byte,
// the decoder wants 4-byte alignment) and encoded through the existing ids-only / offsets path, and the assembled result
// goes back into c->rows_out.  A correctness route: it syncs per document.
static void rows_by_document(wp_vocab *v, Context *c, const uint8_t *d_text, size_t nbytes, const long long *d_doc_off, size_t n_docs,
                             int unit, size_t capacity, RowsResult &out) {
  hipStream_t st = c->stream;
  clear_scalars(c, kScalarRows, kScalarRowsCut, st);
  size_t n_rows = n_docs;
  const void *d_starts = d_doc_off;
  auto check_capacity = [&] {
    out.n_rows = n_rows;
    if (n_rows > capacity) throw std::invalid_argument("capacity_rows is smaller than the number of rows");
  };
  if (d_doc_off) {
    hipLaunchKernelGGL(rows_check_kernel, dim3(cdiv(n_docs + 1, kBlock)), dim3(kBlock), 0, st, d_text, nbytes, d_doc_off, n_docs,
                       c->d_scalars + kScalarRowsBad);
    WP_LAUNCH_CHECK();
    fetch_scalars(c, kScalarRowsCut);
    if (c->h_scalars[kScalarRowsBad] != 0) {
      throw std::invalid_argument("document offsets must increase from 0 to nbytes with a '\\n' in front of each");
    }
    check_capacity();
  } else {
    const unsigned tiles = cdiv(nbytes, kLineTile);
    Arena in(&c->rows_in);
    uint32_t *d_cnt = nullptr, *d_tmp = nullptr;
    for (int pass = 0; pass < 2; pass++) {  // (sized as the joined route sizes its line counts: linear_path.h)
      d_cnt = in.take<uint32_t>(tiles + 1);
      d_tmp = in.take<uint32_t>(cdiv(tiles, kScanTile) + 8);  // the scan's tile sums
      if (pass == 0) in.commit();
    }
    hipLaunchKernelGGL(line_count_kernel, dim3(tiles), dim3(kBlock), 0, st, d_text, nbytes, d_cnt);
    device_exclusive_scan(d_cnt, d_cnt, tiles, d_tmp, c->d_scalars + kScalarRows, st);
    fetch_scalars(c, kScalarRowsCut);
    n_rows = c->h_scalars[kScalarRows];
    check_capacity();
    c->rows_out.ensure((n_rows + 1) * sizeof(long long));
    hipLaunchKernelGGL(line_write_kernel, dim3(tiles), dim3(kBlock), 0, st, d_text, nbytes, static_cast<const uint32_t *>(d_cnt), n_rows,
                       static_cast<long long *>(c->rows_out.p));
    WP_LAUNCH_CHECK();
    d_starts = c->rows_out.p;
  }
  std::vector<long long> starts(n_rows + 1);
  WP_HIP(hipMemcpyAsync(starts.data(), d_starts, (n_rows + 1) * sizeof(long long), hipMemcpyDeviceToHost, st));
  WP_HIP(hipStreamSynchronize(st));
  uint8_t last = '\n';
  WP_HIP(hipMemcpyAsync(&last, d_text + nbytes - 1, 1, hipMemcpyDeviceToHost, st));
  WP_HIP(hipStreamSynchronize(st));
  auto doc_end = [&](size_t i) {  // (a last line without a separator runs to the end of the text)
    return static_cast<size_t>(starts[i + 1]) - ((i + 1 == n_rows && last != '\n') ? 0 : 1);
  };
  size_t longest = 0;
  for (size_t i = 0; i < n_rows; i++) longest = std::max(longest, doc_end(i) - static_cast<size_t>(starts[i]));
  c->text_buf2.ensure(text_room(longest));
  std::vector<int32_t> h_ids;
  std::vector<uint32_t> h_offs;
  std::vector<long long> splits(n_rows + 1, 0);
  EncodeStats last_stats;
  std::memset(&last_stats, 0, sizeof(last_stats));
  int32_t guard_zones = 0;
  int64_t norm_bytes = 0;  // (WP_OPT_NORMALIZE: every document is normalised by its own encode)
  for (size_t i = 0; i < n_rows; i++) {
    splits[i] = static_cast<long long>(h_ids.size());
    const size_t a = static_cast<size_t>(starts[i]), len = doc_end(i) - a;
    if (len == 0) continue;
    char *dst = static_cast<char *>(c->text_buf2.p);
    zero_text_tail(dst, len, st);
    WP_HIP(hipMemcpyAsync(dst, d_text + a, len, hipMemcpyDeviceToDevice, st));
    size_t n = 0;
    encode_on_device(v, c, reinterpret_cast<const uint8_t *>(dst), len, &n, last_stats, unit);
    guard_zones = std::max(guard_zones, last_stats.guard_zones);
    norm_bytes += last_stats.norm_bytes;
    if (n == 0) continue;
    const size_t at = h_ids.size();
    h_ids.resize(at + n);
    WP_HIP(hipMemcpyAsync(h_ids.data() + at, c->d_ids, n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (unit >= 0) {
      h_offs.resize(2 * (at + n));
      WP_HIP(hipMemcpyAsync(h_offs.data() + 2 * at, c->d_offs, 2 * n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    }
    WP_HIP(hipStreamSynchronize(st));
  }
  const size_t n_ids = h_ids.size(), n_offs = unit >= 0 ? 2 * n_ids : 0;
  splits[n_rows] = static_cast<long long>(n_ids);
  Arena res(&c->rows_out);  // (the row starts in it have been read)
  long long *d_splits = nullptr;
  uint32_t *d_offs = nullptr;
  int32_t *d_ids = nullptr;
  for (int pass = 0; pass < 2; pass++) {
    d_splits = res.take<long long>(n_rows + 1);
    d_offs = res.take<uint32_t>(n_offs);
    d_ids = res.take<int32_t>(n_ids + 4);  // + 4: the 16 bytes this block always ended with; no kernel reads behind the ids
    if (pass == 0) res.commit();
  }
  WP_HIP(hipMemcpyAsync(d_splits, splits.data(), (n_rows + 1) * sizeof(long long), hipMemcpyHostToDevice, st));
  if (n_offs) WP_HIP(hipMemcpyAsync(d_offs, h_offs.data(), n_offs * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  if (n_ids) WP_HIP(hipMemcpyAsync(d_ids, h_ids.data(), n_ids * sizeof(int32_t), hipMemcpyHostToDevice, st));
  WP_HIP(hipStreamSynchronize(st));
  c->d_ids = nullptr;  // (the arenas hold the last document only)
  c->d_offs = nullptr;
  out.d_row_splits = d_splits;
  out.d_offs = n_offs ? d_offs : nullptr;
  out.d_ids = n_ids ? d_ids : nullptr;
  out.n_ids = n_ids;
  v->stats = last_stats;  // (of the last non-empty document; the sums of the call below)
  v->stats.guard_zones = guard_zones;
  v->stats.normalize = v->normalize;
  v->stats.norm_bytes = norm_bytes;
  v->stats.n_bytes = static_cast<int64_t>(nbytes);
  v->stats.n_ids = static_cast<int64_t>(n_ids);
  v->stats.n_rows = static_cast<int64_t>(n_rows);
  v->stats.rows_route = 0;
}

// both routes: d_text as wp_linear_encode_device wants it, nbytes > 0; d_doc_off in device memory or nullptr (lines)
static void rows_on_device(wp_vocab *v, Context *c, const uint8_t *d_text, size_t nbytes, const long long *d_doc_off, size_t n_docs,
                           int unit, size_t capacity, RowsResult &out) {
  if (rows_per_document(v)) {
    rows_by_document(v, c, d_text, nbytes, d_doc_off, n_docs, unit, capacity, out);
  } else {
    RowsCall rc{d_doc_off, n_docs, unit, capacity};
    size_t n = 0;
    try {  // (row membership comes from the spans: without a unit they stay in code points, which need no second pass)
      encode_on_device(v, c, d_text, nbytes, &n, v->stats, unit >= 0 ? unit : WP_OFFSETS_CODE_POINTS, &rc);
    } catch (...) {
      out.n_rows = rc.n_rows;
      throw;
    }
    out.d_ids = n ? c->d_ids : nullptr;
    out.d_row_splits = rc.d_row_splits;
    out.d_offs = (n && unit >= 0) ? c->d_offs : nullptr;
    out.n_ids = n;
    out.n_rows = rc.n_rows;
  }
  v->stats.offsets_unit = unit;
  v->stats.n_devices = 1;
}

// the padded batch of a rows result, into device buffers of n_rows * max_len and n_rows int32; waits for it
static void pad_rows_on_device(wp_vocab *v, Context *c, const RowsResult &r, int max_len, int32_t cls_id, int32_t sep_id, int32_t pad_id,
                               int32_t *d_input_ids, int32_t *d_lengths) {
  v->stats.rows_truncated = 0;
  if (r.n_rows == 0) return;
  const int lanes = lanes_for(max_len);
  clear_scalars(c, kScalarRowsCut, kScalarRowsCut, c->stream);
  hipLaunchKernelGGL(pack_rows_kernel, dim3(cdiv(r.n_rows, static_cast<size_t>(kBlock / lanes))), dim3(kBlock), 0, c->stream, r.d_ids,
                     r.d_row_splits, r.n_rows, max_len, cls_id, sep_id, pad_id, lanes, d_input_ids, d_lengths,
                     c->d_scalars + kScalarRowsCut);
  WP_LAUNCH_CHECK();
  fetch_scalars(c, kScalarRowsCut);
  v->stats.rows_truncated = c->h_scalars[kScalarRowsCut];
}

// the buffers of a host call's padded batch, in c->pad_buf until the handle's next call: input_ids | lengths
struct PaddedBatch {
  int32_t *d_input_ids = nullptr, *d_lengths = nullptr;
};
static PaddedBatch padded_batch(Context *c, size_t n_rows, int max_len) {
  Arena a(&c->pad_buf);
  PaddedBatch b;
  for (int pass = 0; pass < 2; pass++) {
    b.d_input_ids = a.take<int32_t>(n_rows * static_cast<size_t>(max_len));
    b.d_lengths = a.take<int32_t>(n_rows);
    if (pass == 0) a.commit();
  }
  return b;
}

// the host form of a documents call as far as its rows: the text and the explicit row starts go up, then rows_on_device
static Context *rows_from_host(wp_vocab *v, const char *utf8, size_t nbytes, const int64_t *doc_off, size_t n_docs, int unit,
                               RowsResult &r) {
  Context *c = get_context(v);
  upload_text(c, utf8, nbytes);
  if (doc_off) {
    c->rows_in.ensure((n_docs + 1) * sizeof(int64_t));
    WP_HIP(hipMemcpyAsync(c->rows_in.p, doc_off, (n_docs + 1) * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
  }
  rows_on_device(v, c, static_cast<const uint8_t *>(c->text_buf.p), nbytes, doc_off ? static_cast<const long long *>(c->rows_in.p) : nullptr,
                 n_docs, unit, SIZE_MAX, r);
  return c;
}

}  // namespace wp
