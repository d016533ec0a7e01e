// special_path.h — special tokens on a context (include/wordpiece_amd.h, section "special tokens"; kernels: special.h):
// the rules of a list, and the passes around the encode of the blanked text — flat (encode_on_device) or by documents
// (rows_on_device), both as they stand.
#pragma once
#include <algorithm>

#include "context.h"
#include "linear_path.h"
#include "rows_path.h"
#include "special.h"

namespace wp {

// a checked wp_special_spec: the distinct lines in ascending byte order, as the kernels' table wants them
struct SpecialList {
  std::vector<uint8_t> lines;  // n rows of kSpecialMaxLine bytes, zero behind the line
  std::vector<int32_t> ids;    // the id of every row
  size_t n_listed = 0;         // entries of the spec (repeats included)
  size_t size() const { return ids.size(); }
};

// every argument rule of a list: needs the vocabulary, no device
static SpecialList check_special_spec(const wp_vocab *v, const wp_special_spec *spec) {
  if (!spec) throw std::invalid_argument("special: spec is NULL");
  if (spec->n_ids < 0 || spec->n_ids > kSpecialMaxListed) throw std::invalid_argument("special: n_ids must be in [0, 4096]");
  if (spec->n_ids > 0 && !spec->ids) throw std::invalid_argument("special: ids is NULL");
  struct Row {
    std::array<uint8_t, kSpecialMaxLine> line;
    int32_t id;
  };
  std::vector<Row> rows;
  for (int32_t k = 0; k < spec->n_ids; k++) {
    const int32_t id = spec->ids[k];
    const std::string name = "special: id " + std::to_string(id);
    if (id < 0 || static_cast<size_t>(id) >= v->hv.tokens.size()) throw std::invalid_argument(name + " is out of range");
    const HostToken &t = v->hv.tokens[static_cast<size_t>(id)];
    if (!t.is_special || t.is_malformed) throw std::invalid_argument(name + " is no special token of the vocabulary (wp_vocab_token_flags)");
    if (t.word.size() > static_cast<size_t>(kSpecialMaxLine)) throw std::invalid_argument(name + " has a line of more than 64 bytes");
    Row r{};
    r.id = id;
    for (size_t i = 0; i < t.word.size(); i++) {
      const uint32_t cp = t.word[i];
      if (cp < 0x21u || cp > 0x7eu) throw std::invalid_argument(name + " has a byte outside 0x21..0x7E in its line");
      if ((cp == 0x5bu && i != 0) || (cp == 0x5du && i + 1 != t.word.size())) {
        throw std::invalid_argument(name + " has a '[' behind the first or a ']' before the last byte of its line");
      }
      r.line[i] = static_cast<uint8_t>(cp);
    }
    rows.push_back(r);
  }
  std::stable_sort(rows.begin(), rows.end(), [](const Row &a, const Row &b) { return a.line < b.line; });
  SpecialList list;
  list.n_listed = static_cast<size_t>(spec->n_ids);
  for (size_t k = 0; k < rows.size(); k++) {
    if (k > 0 && rows[k].line == rows[k - 1].line) {
      if (rows[k].id == rows[k - 1].id) continue;  // (the same id twice is one entry)
      throw std::invalid_argument("special: id " + std::to_string(std::max(rows[k].id, rows[k - 1].id)) + " has the same line as id " +
                                  std::to_string(std::min(rows[k].id, rows[k - 1].id)));
    }
    list.lines.insert(list.lines.end(), rows[k].line.begin(), rows[k].line.end());
    list.ids.push_back(rows[k].id);
  }
  return list;
}

static void check_special_call(int unit, size_t nbytes) {
  if (unit != -1 && unit != WP_OFFSETS_BYTES && unit != WP_OFFSETS_CODE_POINTS) {
    throw std::invalid_argument("offsets unit must be -1 (none), 0 (bytes) or 1 (code points)");
  }
  // (a literal's byte start is a 32-bit value in every unit)
  if (nbytes > static_cast<size_t>(UINT32_MAX)) throw std::length_error("a special-tokens call needs nbytes <= UINT32_MAX");
}

static void set_special_stats(wp_vocab *v, const SpecialList &list, size_t n_literals, size_t n_ids, bool by_rows, size_t n_rows) {
  v->stats.special_call = 1;
  v->stats.special.n_literals = static_cast<int64_t>(n_literals);
  v->stats.special.n_ids = static_cast<int64_t>(n_ids);
  v->stats.special.n_rows = by_rows ? static_cast<int64_t>(n_rows) : -1;
  v->stats.special.n_listed = static_cast<int64_t>(list.n_listed);
}

// Both forms.  d_text as wp_linear_encode_device wants it, nbytes > 0.  by_rows: the documents form — d_doc_off, n_docs
// and capacity as rows_on_device takes them; else the flat form, whose result is one row without row_splits.  The
// result lies in the context's buffers until the handle's next call.  A text without literals, and an empty list, is
// the plain call on the caller's buffer.
static void special_on_device(wp_vocab *v, Context *c, const uint8_t *d_text, size_t nbytes, bool by_rows, const long long *d_doc_off,
                              size_t n_docs, int unit, size_t capacity, const SpecialList &list, RowsResult &out) {
  hipStream_t st = c->stream;
  const dim3 block(kBlock);
  auto plain = [&](const uint8_t *text, int inner_unit) {
    if (by_rows) {
      rows_on_device(v, c, text, nbytes, d_doc_off, n_docs, inner_unit, capacity, out);
    } else {
      size_t n = 0;
      encode_on_device(v, c, text, nbytes, &n, v->stats, inner_unit);
      v->stats.n_devices = 1;
      out.d_ids = n ? c->d_ids : nullptr;
      out.d_offs = (n && inner_unit >= 0) ? c->d_offs : nullptr;
      out.n_ids = n;
    }
  };
  uint32_t n_lits = 0;
  const unsigned tiles = cdiv(nbytes, kSpecialTile);
  uint32_t *d_tile_cnt = nullptr;
  SpecialTable tab{};
  if (list.size() > 0) {
    // ---- match, pass 1: the table goes up, the literals are counted, the count comes down ----
    Arena in(&c->special_in);
    uint8_t *d_lines = nullptr;
    int32_t *d_tab_ids = nullptr;
    uint32_t *d_scan_tmp = nullptr;
    for (int pass = 0; pass < 2; pass++) {
      d_lines = in.take<uint8_t>(list.lines.size());
      d_tab_ids = in.take<int32_t>(list.size());
      d_tile_cnt = in.take<uint32_t>(tiles + 1);
      d_scan_tmp = in.take<uint32_t>(cdiv(tiles, kScanTile) + 1);
      if (pass == 0) in.commit();
    }
    WP_HIP(hipMemcpyAsync(d_lines, list.lines.data(), list.lines.size(), hipMemcpyHostToDevice, st));
    WP_HIP(hipMemcpyAsync(d_tab_ids, list.ids.data(), list.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    tab = SpecialTable{d_lines, d_tab_ids, static_cast<int>(list.size())};
    hipLaunchKernelGGL(special_count_kernel, dim3(tiles), block, 0, st, d_text, nbytes, tab, d_tile_cnt);
    device_exclusive_scan(d_tile_cnt, d_tile_cnt, tiles, d_scan_tmp, c->d_scalars + kScalarSpecial, st);
    queue_scalar_slots(c, kScalarSpecial, kScalarSpecial, st);
    WP_HIP(hipStreamSynchronize(st));  // (also: the list's vectors have been read)
    n_lits = c->h_scalars[kScalarSpecial];
  }
  if (n_lits == 0) {
    plain(d_text, unit);
    set_special_stats(v, list, 0, out.n_ids, by_rows, out.n_rows);
    return;
  }
  const bool guard = v->arena_guard || EnvOptions::get().arena_guard;
  // ---- match, pass 2, and the blanked copy ----
  Arena la(&c->special_lit, guard);
  uint32_t *d_lit_start = nullptr, *d_lit_len = nullptr;
  int32_t *d_lit_id = nullptr;
  for (int pass = 0; pass < 2; pass++) {
    d_lit_start = la.take<uint32_t>(n_lits);
    d_lit_len = la.take<uint32_t>(n_lits);
    d_lit_id = la.take<int32_t>(n_lits);
    if (pass == 0) la.commit();
  }
  la.arm(st);
  hipLaunchKernelGGL(special_write_kernel, dim3(tiles), block, 0, st, d_text, nbytes, tab, static_cast<const uint32_t *>(d_tile_cnt), n_lits,
                     d_lit_start, d_lit_len, d_lit_id);
  c->special_text.ensure(text_room(nbytes));
  uint8_t *d_copy = static_cast<uint8_t *>(c->special_text.p);
  zero_text_tail(d_copy, nbytes, st);
  WP_HIP(hipMemcpyAsync(d_copy, d_text, nbytes, hipMemcpyDeviceToDevice, st));
  hipLaunchKernelGGL(special_blank_kernel, dim3(cdiv(n_lits, kBlock)), block, 0, st, d_copy, nbytes, static_cast<const uint32_t *>(d_lit_start),
                     static_cast<const uint32_t *>(d_lit_len), n_lits);
  WP_LAUNCH_CHECK();
#ifdef WP_DEBUG_BOUNDS
  WP_HIP(hipStreamSynchronize(st));  // (the encode below takes every site's counter)
  throw_if_oob(kSiteSpecial, "special", "stores of the literal list or of the blanks skipped");
#endif
  // ---- the encode of the blanked text; the placement needs spans, so a call without a unit runs with bytes ----
  const int inner_unit = unit >= 0 ? unit : WP_OFFSETS_BYTES;
  plain(d_copy, inner_unit);  // (a capacity error leaves the count in out.n_rows)
  const RowsResult r = out;
  const size_t n_ids = r.n_ids, n_out = n_ids + n_lits, n_rows = by_rows ? r.n_rows : 0;
  // ---- place and merge ----
  const bool lines = by_rows && !d_doc_off;
  const bool cps = inner_unit == WP_OFFSETS_CODE_POINTS;
  const unsigned line_tiles = cdiv(nbytes, kLineTile);
  const size_t cp_rows = nbytes / static_cast<size_t>(kDecRowBytes) + 1;
  Arena oa(&c->special_out, guard);
  long long *d_out_splits = nullptr, *d_starts = nullptr;
  uint2 *d_out_spans = nullptr;
  int32_t *d_out_ids = nullptr;
  uint32_t *d_lit_at = nullptr, *d_lit_pos = nullptr, *d_line_cnt = nullptr, *d_line_tmp = nullptr, *d_cp_rows = nullptr, *d_cp_tmp = nullptr;
  for (int pass = 0; pass < 2; pass++) {
    d_out_splits = oa.take<long long>(by_rows ? n_rows + 1 : 0);
    d_out_spans = oa.take<uint2>(unit >= 0 ? n_out : 0);
    d_out_ids = oa.take<int32_t>(n_out);
    d_lit_at = oa.take<uint32_t>(n_lits);
    d_lit_pos = oa.take<uint32_t>(n_lits);
    d_starts = oa.take<long long>(lines ? n_rows + 1 : 0);
    d_line_cnt = oa.take<uint32_t>(lines ? line_tiles + 1 : 0);
    d_line_tmp = oa.take<uint32_t>(lines ? cdiv(line_tiles, kScanTile) + 1 : 0);
    d_cp_rows = oa.take<uint32_t>(cps ? cp_rows : 0);
    d_cp_tmp = oa.take<uint32_t>(cps ? cdiv(cp_rows, kScanTile) + 1 : 0);
    if (pass == 0) oa.commit();
  }
  oa.arm(st);
  SpecialRows rows{nullptr, nullptr, 0};
  if (by_rows) {
    if (lines) {  // the row starts of the caller's text (the blanked copy has the same lines)
      hipLaunchKernelGGL(line_count_kernel, dim3(line_tiles), block, 0, st, d_copy, nbytes, d_line_cnt);
      device_exclusive_scan(d_line_cnt, d_line_cnt, line_tiles, d_line_tmp, nullptr, st);
      hipLaunchKernelGGL(line_write_kernel, dim3(line_tiles), block, 0, st, d_copy, nbytes, static_cast<const uint32_t *>(d_line_cnt), n_rows,
                         d_starts);
    }
    rows = SpecialRows{lines ? d_starts : d_doc_off, r.d_row_splits, n_rows};
  }
  if (cps) {
    hipLaunchKernelGGL(special_cp_rows_kernel, dim3(cdiv(cp_rows, kDecTile / kDecRowBytes)), block, 0, st, d_copy, nbytes, cp_rows, d_cp_rows);
    device_exclusive_scan(d_cp_rows, d_cp_rows, cp_rows, d_cp_tmp, nullptr, st);
  }
  hipLaunchKernelGGL(special_place_kernel, dim3(cdiv(n_lits, kBlock)), block, 0, st, d_copy, nbytes, static_cast<const uint32_t *>(d_lit_start),
                     n_lits, rows, reinterpret_cast<const uint2 *>(r.d_offs), n_ids, inner_unit, static_cast<const uint32_t *>(d_cp_rows),
                     d_lit_at, d_lit_pos);
  hipLaunchKernelGGL(special_merge_kernel, dim3(cdiv(n_out, kSpecialMergeTile)), block, 0, st, r.d_ids, reinterpret_cast<const uint2 *>(r.d_offs),
                     n_ids, static_cast<const uint32_t *>(d_lit_at), static_cast<const uint32_t *>(d_lit_pos),
                     static_cast<const uint32_t *>(d_lit_len), static_cast<const int32_t *>(d_lit_id), n_lits, d_out_ids,
                     unit >= 0 ? d_out_spans : nullptr);
  if (by_rows) {
    hipLaunchKernelGGL(special_splits_kernel, dim3(cdiv(n_rows + 1, kBlock)), block, 0, st, rows, static_cast<const uint32_t *>(d_lit_start), n_lits,
                       d_out_splits);
  }
  WP_LAUNCH_CHECK();
  if (guard) {  // debugging aid: no kernel of this layer may have written outside the buffer it was given
    static const uint32_t init[2] = {0u, 0xffffffffu};
    WP_HIP(hipMemcpyAsync(c->d_scalars + kScalarGuard, init, sizeof(init), hipMemcpyHostToDevice, st));
    la.check(st, c->d_scalars + kScalarGuard);
    oa.check(st, c->d_scalars + kScalarGuard);
    queue_scalar_slots(c, kScalarGuardBad, kScalarGuardFirst, st);
  }
  WP_HIP(hipStreamSynchronize(st));
  if (guard) {
    if (c->h_scalars[kScalarGuardBad] != 0) {
      throw HipError("arena guard: special: " + std::to_string(c->h_scalars[kScalarGuardBad]) + " guard zone(s) overwritten, first behind allocation #" +
                     std::to_string(c->h_scalars[kScalarGuardFirst] - 1));
    }
    v->stats.guard_zones += static_cast<int32_t>(la.zones.size() + oa.zones.size());
  }
  throw_if_oob(kSiteSpecial, "special", "rows outside the ids or gathers of the merge skipped");
  c->d_ids = nullptr;  // (the encoder's arenas hold the blanked text's result)
  c->d_offs = nullptr;
  out.d_ids = d_out_ids;
  out.d_offs = unit >= 0 ? reinterpret_cast<const uint32_t *>(d_out_spans) : nullptr;
  out.d_row_splits = by_rows ? d_out_splits : nullptr;
  out.n_ids = n_out;
  out.n_rows = n_rows;
  v->stats.n_ids = static_cast<int64_t>(n_out);
  v->stats.offsets_unit = unit;
  set_special_stats(v, list, n_lits, n_out, by_rows, n_rows);
}

// the documents form: the signature of rows_on_device plus the list
static void special_rows_on_device(wp_vocab *v, Context *c, const uint8_t *d_text, size_t nbytes, const long long *d_doc_off, size_t n_docs,
                                   int unit, size_t capacity, const SpecialList &list, RowsResult &out) {
  special_on_device(v, c, d_text, nbytes, true, d_doc_off, n_docs, unit, capacity, list, out);
}

}  // namespace wp
