// scrub_path.h — the scrub on a context (include/wordpiece_amd_scrub.h; kernels: scrub.h): the argument rules and the
// replacement table, the answer of a call without bytes, the launches over one device batch and the buffers of a call.
// The intake, the per-row arrays and the end of a call are text_path.h's; the class pass of quality.h is not needed.
#pragma once
#include <algorithm>
#include <vector>

#include "context.h"
#include "scrub.h"
#include "text_path.h"

namespace wp {

struct ScrubPlan {
  bool want_matches = false, want_text = false, want_compact = false;
  int kinds = 0;
  ScLimits lim{};
  ScRepl repl{};
  std::vector<uint32_t> pool;  // kScPoolWords words: the strings at their offsets, zeros behind them
};

// every rule of the spec, each with the field it is about; nothing here needs a device
static ScrubPlan check_scrub_spec(const wp_scrub_spec *spec, const wp_scrub_result *out) {
  if (!spec) throw std::invalid_argument("scrub: spec is NULL");
  if (!out) throw std::invalid_argument("scrub: out is NULL");
  if (spec->elem_bytes != 1) throw std::invalid_argument("scrub: elem_bytes must be 1");
  check_want("scrub", spec->want, WP_SCRUB_WANT_MATCHES | WP_SCRUB_WANT_TEXT | WP_SCRUB_WANT_COMPACT);
  ScrubPlan p;
  p.want_matches = (spec->want & WP_SCRUB_WANT_MATCHES) != 0;
  p.want_text = (spec->want & WP_SCRUB_WANT_TEXT) != 0;
  p.want_compact = (spec->want & WP_SCRUB_WANT_COMPACT) != 0;
  if ((spec->kinds & ~(WP_SCRUB_EMAIL | WP_SCRUB_IPV4 | WP_SCRUB_IP_KEEP_PRIVATE)) != 0) throw std::invalid_argument("scrub: kinds has bits outside 7");
  if (spec->pad != 0) throw std::invalid_argument("scrub: pad must be 0");
  p.kinds = spec->kinds;
  for (int k = 0; k < WP_SCRUB_RULES; k++) {
    const int64_t L = spec->doc_limit[k];
    if (L != -1 && (L < 0 || L > 1000000000)) throw std::invalid_argument("scrub: doc_limit[" + std::to_string(k) + "] must be -1 or in [0, 10^9]");
    p.lim.doc[k] = static_cast<long long>(L);
  }
  auto count = [](const char *what, int32_t n, bool searched) {
    if (n < 0 || n > WP_SCRUB_MAX_REPL) throw std::invalid_argument(std::string("scrub: ") + what + " must be in [0, 16]");
    if (searched && n == 0) throw std::invalid_argument(std::string("scrub: ") + what + " must be 1 at least where kinds searches for the kind");
    return static_cast<uint16_t>(n);
  };
  p.repl.n_email = count("n_email_repl", spec->n_email_repl, (spec->kinds & WP_SCRUB_EMAIL) != 0);
  p.repl.n_ip = count("n_ip_repl", spec->n_ip_repl, (spec->kinds & WP_SCRUB_IPV4) != 0);
  const int n = p.repl.n_email + p.repl.n_ip;
  p.pool.assign(kScPoolWords, 0u);
  if (n != 0) {
    if (!spec->repl_pool) throw std::invalid_argument("scrub: repl_pool is NULL");
    if (!spec->repl_off) throw std::invalid_argument("scrub: repl_off is NULL");
    if (spec->repl_off[0] != 0) throw std::invalid_argument("scrub: repl_off must start at 0");
    const uint8_t *pool = static_cast<const uint8_t *>(spec->repl_pool);
    for (int t = 0; t < n; t++) {
      const int64_t a = spec->repl_off[t], len = spec->repl_off[t + 1] - a;
      const std::string at = "string " + std::to_string(t);
      if (len < 0 || len > WP_SCRUB_MAX_REPL_BYTES) throw std::invalid_argument("scrub: repl_off: " + at + " must have 0 to 64 bytes");
      if (a + len > WP_SCRUB_MAX_POOL_BYTES) throw std::invalid_argument("scrub: repl_off: " + at + " ends behind the 2048 bytes of a pool");
      for (int64_t i = 0; i < len; i++) {
        if (pool[a + i] == 0x0a) throw std::invalid_argument("scrub: repl_pool: " + at + " holds a line feed");
        p.pool[(a + i) / 4] |= static_cast<uint32_t>(pool[a + i]) << (8u * static_cast<uint32_t>((a + i) % 4));
      }
      p.repl.off[t + 1] = static_cast<uint16_t>(a + len);
    }
  }
  if (spec->reserved != 0) throw std::invalid_argument("scrub: reserved must be 0");
  return p;
}

static_assert(kScCounters <= kTextMaxCounters, "the counters of a text-signal layer");
constexpr TextLayer kScrubLayer{"scrub", "scrub", "gathers or stores outside the tile, match, signal or text arrays skipped",
                                kScalarScrubBad, kScalarScrubKept, kScalarScrubElems, kScalarScrubWindows, kScalarScrubMatches, kScalarScrubFree, kScalarScrubOutBytes,
                                kScalarScrub, kScCounters};

static wp_scrub_stats &begin_scrub_stats(wp_vocab *v, size_t n_rows) {
  v->stats.scrub_call = 1;
  v->stats.scrub = wp_scrub_stats{};
  v->stats.scrub.n_rows = static_cast<int64_t>(n_rows);
  return v->stats.scrub;
}

// A host call whose batch has no byte (n_rows >= 1): the document rules over zeros (text_path.h); no row has a match, and
// the scrubbed rows are the empty rows themselves.
static wp_scrub_result scrub_no_bytes(wp_vocab *v, const ScrubPlan &plan, size_t n_rows) {
  const long long zeros[WP_SCRUB_SIGNALS] = {};
  wp_scrub_result h = text_no_bytes<wp_scrub_result>(begin_scrub_stats(v, n_rows), n_rows, WP_SCRUB_SIGNALS, WP_SCRUB_RULES, scrub_reasons(zeros, plan.lim),
                                                     plan.want_compact);
  if (plan.want_text) h.out_off = static_cast<int64_t *>(zeroed((n_rows + 1) * sizeof(int64_t)));
  return h;
}

// The batch `in` (n_rows >= 1), on c's stream.  The results are device pointers into c->scrub_rows (signals, reasons,
// out_off), c->scrub_items (the arrays per match) and c->scrub_out (the text and the compact form), valid until the
// handle's next call.  Waits, from the spec alone: the sizes; the number of matches; the 64-bit totals of the bytes the
// replacements add and remove; with the compact form the kept count; the one that ends the call.
static void scrub_on_device(wp_vocab *v, Context *c, const RaggedIn &in, const ScrubPlan &plan, wp_scrub_result *R) {
  const TextLayer &L = kScrubLayer;
  const size_t n = in.n_rows, n1 = n + 1;
  wp_scrub_stats &ps = begin_scrub_stats(v, n);
  *R = wp_scrub_result{};
  R->n_rows = static_cast<int64_t>(n);
  hipStream_t st = c->stream;
  const bool guard = v->arena_guard || EnvOptions::get().arena_guard;
  // WP_OPT_STAGE_TIMING: kMarkStart, kMarkCounted (intake), kMarkSorted (both find passes), kMarkScanned (offsets),
  // kMarkWalked (document rules, text, compact form)
  const bool timing = v->stage_timing;
  begin_stage_timing(c, timing, st);

  // ---- the per-row arrays, the offset check --------------------------------------------------------------------------------
  Arena ra(&c->scrub_rows, guard);
  TextRows rows;
  uint32_t *d_out_boff = nullptr;
  long long *d_out_off = nullptr;
  for (int pass = 0; pass < 2; pass++) {
    rows.take(ra, n, WP_SCRUB_SIGNALS);
    d_out_boff = ra.take<uint32_t>(n1);
    d_out_off = ra.take<long long>(n1);
    if (pass == 0) ra.commit();
  }
  ra.arm(st);
  unsigned long long *d_counters = reinterpret_cast<unsigned long long *>(c->d_scalars + kScalarScrub);
  rows.queue(c, L, in, st);
  const size_t nb = rows.read(c, L, in, st);
  ps.n_bytes = static_cast<int64_t>(nb);
  const uint32_t *d32 = static_cast<const uint32_t *>(in.d_data);
  if (timing) WP_HIP(hipEventRecord(c->ev[kMarkCounted], st));

  // ---- the count pass: the matches of every tile, their scan, their number -------------------------------------------------
  const size_t n_tiles = cdiv(nb, kQualTile), nt1 = n_tiles + 1;
  Arena ta(&c->scrub_tiles, guard);
  uint32_t *d_tiles = nullptr, *d_ttmp = nullptr, *d_pool = nullptr;
  for (int pass = 0; pass < 2; pass++) {
    d_tiles = ta.take<uint32_t>(nt1);
    d_ttmp = ta.take<uint32_t>(cdiv(nt1, kScanTile) + 8);
    d_pool = ta.take<uint32_t>(kScPoolWords);
    if (pass == 0) ta.commit();
  }
  ta.arm(st);
  WP_HIP(hipMemcpyAsync(d_pool, plan.pool.data(), kScPoolWords * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  WP_HIP(hipMemsetAsync(d_tiles, 0, nt1 * sizeof(uint32_t), st));
  if (nb != 0) {
    hipLaunchKernelGGL(scrub_find_kernel<false>, dim3(n_tiles), dim3(kBlock), 0, st, d32, nb, rows.d_boff, n, plan.kinds, plan.repl, d_tiles, ScMatches{}, rows.usig(),
                       d_counters);
  }
  device_exclusive_scan(d_tiles, d_tiles, nt1, d_ttmp, c->d_scalars + L.words, st);
  WP_LAUNCH_CHECK();
  queue_scalar_slots(c, L.words, L.words, st);
  WP_HIP(hipStreamSynchronize(st));
  const size_t nm = c->h_scalars[L.words];
  if (nm > nb / 6 + 1) throw HipError("scrub: more matches than the bytes have room for");

  // ---- the write pass: the matches in text order, the signals, the totals; E --------------------------------------------------
  Arena ia(&c->scrub_items, guard);
  ScMatches ms{};
  uint32_t *d_E = nullptr, *d_etmp = nullptr;
  for (int pass = 0; pass < 2; pass++) {
    ms.start = ia.take<uint32_t>(nm);
    ms.delta = ia.take<uint32_t>(nm + 1);
    ms.row = ia.take<int32_t>(nm);
    ms.len = ia.take<int32_t>(nm);
    ms.kind = ia.take<int32_t>(nm);
    ms.repl = ia.take<int32_t>(nm);
    ms.start64 = plan.want_matches ? ia.take<long long>(nm) : nullptr;
    d_E = ia.take<uint32_t>(nm + 1);
    d_etmp = ia.take<uint32_t>(cdiv(nm + 1, kScanTile) + 8);
    if (pass == 0) ia.commit();
  }
  ia.arm(st);
  ms.n = nm;
  WP_HIP(hipMemsetAsync(ms.delta + nm, 0, sizeof(uint32_t), st));
  if (nb != 0) {  // (without a match too: the '@' bytes are counted here)
    hipLaunchKernelGGL(scrub_find_kernel<true>, dim3(n_tiles), dim3(kBlock), 0, st, d32, nb, rows.d_boff, n, plan.kinds, plan.repl, d_tiles, ms, rows.usig(), d_counters);
  }
  WP_LAUNCH_CHECK();
  if (timing) WP_HIP(hipEventRecord(c->ev[kMarkSorted], st));
  device_exclusive_scan(ms.delta, d_E, nm + 1, d_etmp, nullptr, st);
  if (timing) WP_HIP(hipEventRecord(c->ev[kMarkScanned], st));

  // ---- the document rules, the kept rows; the size of the text from the 64-bit totals ---------------------------------------
  hipLaunchKernelGGL(scrub_docs_kernel, count_grid(n1), dim3(kBlock), 0, st, static_cast<const uint32_t *>(rows.d_boff), n, static_cast<const uint32_t *>(ms.start),
                     static_cast<const uint32_t *>(d_E), nm, plan.lim, rows.d_sig, rows.d_reasons, rows.d_keep, d_out_off, d_out_boff, d_counters);
  WP_LAUNCH_CHECK();
  queue_scalar_slots(c, kScalarScrub, kScalarScrub, st);
  const bool text = plan.want_text || plan.want_compact;
  size_t out_bytes = 0;
  auto read_totals = [&] {
    unsigned long long tot[kScCounters];
    std::memcpy(tot, c->h_scalars + kScalarScrub, sizeof(tot));
    if (tot[kScRemoved] > nb) throw HipError("scrub: the matches hold more bytes than the text");
    const unsigned long long ob = nb - tot[kScRemoved] + tot[kScAdded];
    if (ob > UINT32_MAX) throw std::length_error("scrub: more than UINT32_MAX bytes behind the scrub");
    out_bytes = static_cast<size_t>(ob);
  };
  WP_HIP(hipStreamSynchronize(st));
  read_totals();
  Arena oa(&c->scrub_out, guard);
  TextTail tail;
  uint32_t *d_out = nullptr;
  tail.begin(c, L, rows, out_bytes, plan.want_compact, text, oa, st, [&](Arena &a) { d_out = a.take<uint32_t>(out_bytes / 4 + 1); });
  if (text && nb != 0) {
    hipLaunchKernelGGL(scrub_write_kernel, dim3(n_tiles), dim3(kBlock), 0, st, d32, nb, ms, static_cast<const uint32_t *>(d_E), static_cast<const uint32_t *>(d_pool),
                       plan.repl, d_out, out_bytes);
    WP_LAUNCH_CHECK();
  }
  tail.end(v, c, L, rows, RaggedIn{d_out, d_out_off, n, 1}, d_out_boff, out_bytes, plan.want_compact, {&ra, &ta, &ia, &oa}, R,
           [&](const unsigned long long *counters, int64_t n_kept) {
             if (counters[kScKinds] + counters[kScKinds + 1] + counters[kScKinds + 2] != nm) throw HipError("scrub: the rows do not sum to the matches of the text");
             ps.n_out_bytes = static_cast<int64_t>(out_bytes);
             ps.n_kept = n_kept;
             for (int k = 0; k < 3; k++) ps.n_matches[k] = static_cast<int64_t>(counters[kScKinds + k]);
             for (int k = 0; k < WP_SCRUB_RULES; k++) ps.rule_failed[k] = static_cast<int64_t>(counters[kScRuleFailed + k]);
           });
  if (plan.want_matches) {
    R->n_matches = static_cast<int64_t>(nm);
    if (nm != 0) {
      R->match_row = ms.row;
      R->match_start = reinterpret_cast<int64_t *>(ms.start64);
      R->match_len = ms.len;
      R->match_kind = ms.kind;
      R->match_repl = ms.repl;
    }
  }
  if (plan.want_text) {
    R->n_out_elems = static_cast<int64_t>(out_bytes);
    R->out_off = reinterpret_cast<int64_t *>(d_out_off);
    R->out_data = out_bytes ? d_out : nullptr;
  }
}

}  // namespace wp
