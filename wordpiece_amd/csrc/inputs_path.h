// inputs_path.h — model inputs on a context (include/wordpiece_amd.h, section "model inputs"; kernels: inputs.h): the
// argument rules, the plan / scan / pack passes over a rows result, and the buffers of a host call's batch.
#pragma once
#include "context.h"
#include "inputs.h"
#include "rows_path.h"

namespace wp {

// every argument rule that needs neither the text nor a device
static InputsGeom check_inputs_spec(const wp_inputs_spec *spec, size_t nbytes) {
  if (!spec) throw std::invalid_argument("inputs: spec is NULL");
  check_rows_call(spec->unit, nbytes);
  if (spec->truncation != WP_TRUNC_LONGEST_FIRST && spec->truncation != WP_TRUNC_ONLY_FIRST && spec->truncation != WP_TRUNC_ONLY_SECOND) {
    throw std::invalid_argument("inputs: unknown truncation strategy");
  }
  if (spec->stride < -1) throw std::invalid_argument("inputs: stride must be -1 (no windows) or at least 0");
  if (spec->pairs != 0 && spec->pairs != 1) throw std::invalid_argument("inputs: pairs must be 0 or 1");
  InputsGeom g;
  g.max_len = spec->max_len;
  g.head = spec->cls_id >= 0 ? 1 : 0;
  g.nsep = spec->sep_id >= 0 ? 1 : 0;
  const int specials = g.head + g.nsep * (spec->pairs ? 2 : 1);
  if (spec->max_len < 1 || spec->max_len < specials) {
    throw std::invalid_argument("max_len must be at least 1 and at least the number of specials");
  }
  g.budget = spec->max_len - specials;
  g.pairs = spec->pairs;
  g.truncation = spec->truncation;
  g.stride = spec->stride;
  g.cls_id = spec->cls_id;
  g.sep_id = spec->sep_id;
  g.pad_id = spec->pad_id;
  if (spec->truncation == WP_TRUNC_LONGEST_FIRST) {
    if (spec->stride >= 0) throw std::invalid_argument("inputs: windows (stride >= 0) need the truncation only_first or only_second");
  } else {
    if (spec->truncation == WP_TRUNC_ONLY_SECOND && !spec->pairs) throw std::invalid_argument("inputs: only_second needs pairs");
    if (static_cast<long long>(g.budget) < static_cast<long long>(std::max(spec->stride, 0)) + 1) {
      throw std::invalid_argument("inputs: max_len leaves no room for a window");
    }
  }
  return g;
}

static void check_inputs_rows(const InputsGeom &g, size_t n_rows) {
  if (g.pairs && (n_rows & 1) != 0) throw std::invalid_argument("inputs: pairs need an even number of rows");
}

// n_out * max_len cells of 8 bytes must be addressable
static void check_inputs_size(size_t n_out, int max_len) {
  if (n_out > static_cast<size_t>(UINT32_MAX) || n_out > SIZE_MAX / 8 / static_cast<size_t>(max_len)) {
    throw std::length_error("inputs: too many output rows");
  }
}

// The model inputs of a rows result.  place(n_out) names the buffers of the batch once the number of output rows is
// known (and throws where they do not fit); returns n_out.  Waits for the batch.  Without windows the host waits once,
// behind the packer (as pad_rows_on_device does); with windows once more, for the row count.
template <typename Place>
static size_t inputs_on_device(wp_vocab *v, Context *c, const RowsResult &r, const InputsGeom &g, int unit, Place &&place) {
  hipStream_t st = c->stream;
  const size_t n_samples = r.n_rows / (g.pairs ? 2 : 1);
  v->stats.rows_truncated = 0;
  v->stats.inputs_call = 1;
  wp_inputs_stats &is = v->stats.inputs;
  is = wp_inputs_stats{};
  is.n_samples = static_cast<int64_t>(n_samples);
  is.pairs = g.pairs;
  is.truncation = g.truncation;
  is.stride = g.stride;
  if (n_samples > static_cast<size_t>(INT32_MAX)) throw std::length_error("inputs: too many samples");
  if (n_samples == 0) {
    (void)place(0);
    return 0;
  }
  const bool windows = g.stride >= 0;
  Arena scratch(&c->inputs_buf);
  InputsRec *d_rec = nullptr;
  uint32_t *d_win = nullptr, *d_tmp = nullptr;
  for (int pass = 0; pass < 2; pass++) {
    d_rec = scratch.take<InputsRec>(n_samples);                       // a record per sample
    d_win = scratch.take<uint32_t>(n_samples);                        // window counts, scanned in place
    d_tmp = scratch.take<uint32_t>(cdiv(n_samples, kScanTile) + 8);   // the scan's tile sums (+ 8 as the encoder's scans)
    if (pass == 0) scratch.commit();
  }
  clear_scalars(c, kScalarInCut, kScalarInWindowed, st);
  hipLaunchKernelGGL(inputs_plan_kernel, dim3(cdiv(n_samples, kBlock)), dim3(kBlock), 0, st, r.d_row_splits, n_samples, g, d_win, d_rec,
                     c->d_scalars + kScalarInCut, c->d_scalars + kScalarInWindowed);
  WP_LAUNCH_CHECK();
  size_t n_out = n_samples;
  if (windows) {
    device_exclusive_scan(d_win, d_win, n_samples, d_tmp, nullptr, st, nullptr,
                          reinterpret_cast<unsigned long long *>(c->d_scalars + kScalarInRows));
    fetch_scalars(c, kScalarInWindowed);
    unsigned long long total;
    std::memcpy(&total, c->h_scalars + kScalarInRows, sizeof(total));
    if (total > static_cast<unsigned long long>(UINT32_MAX)) throw std::length_error("inputs: too many output rows");
    n_out = static_cast<size_t>(total);
  }
  check_inputs_size(n_out, g.max_len);
  is.n_out = static_cast<int64_t>(n_out);
  const wp_inputs o = place(n_out);
  const int lanes = lanes_for(g.max_len);
  hipLaunchKernelGGL(inputs_pack_kernel, dim3(cdiv(n_out, static_cast<size_t>(kBlock / lanes))), dim3(kBlock), 0, st, r.d_ids,
                     reinterpret_cast<const uint2 *>(r.d_offs), r.n_ids, r.d_row_splits, static_cast<const InputsRec *>(d_rec),
                     windows ? static_cast<const uint32_t *>(d_win) : nullptr, n_samples, n_out, g, lanes, o.input_ids, o.token_type_ids,
                     unit >= 0 ? reinterpret_cast<uint2 *>(o.offsets) : nullptr, o.lengths, o.sample);
  WP_LAUNCH_CHECK();
  if (windows) {
    WP_HIP(hipStreamSynchronize(st));
  } else {
    fetch_scalars(c, kScalarInWindowed);
  }
  throw_if_oob(kSiteInputs, "model inputs", "gathers outside the id list skipped");
  is.n_cut = c->h_scalars[kScalarInCut];
  is.n_windowed = c->h_scalars[kScalarInWindowed];
  return n_out;
}

// the buffers of a host call's batch of n_out rows, in c->pad_buf until the handle's next call:
// offsets (unit >= 0) | input_ids | token_type_ids | lengths | sample
static wp_inputs inputs_batch(Context *c, int unit, size_t n_out, int max_len) {
  const size_t cells = n_out * static_cast<size_t>(max_len);
  Arena a(&c->pad_buf);
  wp_inputs o{};
  for (int pass = 0; pass < 2; pass++) {
    if (unit >= 0) o.offsets = a.take<uint32_t>(2 * cells);
    o.input_ids = a.take<int32_t>(cells);
    o.token_type_ids = a.take<int32_t>(cells);
    o.lengths = a.take<int32_t>(n_out);
    o.sample = a.take<int32_t>(n_out + 4);  // + 4: the 16 bytes this block always ended with; inputs_pack_kernel writes nothing behind row n_out
    if (pass == 0) a.commit();
  }
  return o;
}

static size_t count_lines_host(const char *utf8, size_t nbytes) {
  if (nbytes == 0) return 0;
  size_t n = utf8[nbytes - 1] != '\n' ? 1 : 0;
  for (const char *p = utf8, *end = utf8 + nbytes; (p = static_cast<const char *>(std::memchr(p, '\n', end - p))) != nullptr; p++) n++;
  return n;
}

}  // namespace wp
