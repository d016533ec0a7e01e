// classify_path.h — the linear classifier on a context (include/wordpiece_amd_classify.h; kernels: classify.h): the
// argument rules of a model and of a call, the model a slot of the handle owns (its upload, its dictionary table, its
// release), the launches over one device batch and the buffers of a call.  The intake and the per-row arrays are
// text_path.h's, the kept rows window_path.h's.
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

#include "classify.h"
#include "context.h"
#include "text_path.h"

namespace wp {

static uint32_t cls_host_hash(const uint8_t *p, size_t n) {
  uint32_t h = kClsFnvInit;
  for (size_t i = 0; i < n; i++) h = (h ^ static_cast<uint32_t>(static_cast<int32_t>(static_cast<int8_t>(p[i])))) * kClsFnvPrime;
  return h;
}

static int check_classify_slot(int slot) {
  if (slot < 0 || slot >= WP_CLASSIFY_SLOTS) throw std::invalid_argument("classify: slot must be in [0, 3]");
  return slot;
}

// ---- the model of a slot ------------------------------------------------------------------------------------------------------
// frees the model s holds on its device (the streams that used it have been waited for: every call ends with a wait) and
// empties s
static void classify_free(wp_vocab *v, ClassifySlot &s) {
  if (s.loaded) {
    DeviceGuard keep;
    (void)hipSetDevice(s.device);
    if (v->ctx) (void)hipStreamSynchronize(v->ctx->stream);
    for (const void *p : {static_cast<const void *>(s.m.input), static_cast<const void *>(s.m.output), static_cast<const void *>(s.m.table),
                          static_cast<const void *>(s.m.pool), static_cast<const void *>(s.m.word_off)}) {
      if (p) (void)hipFree(const_cast<void *>(p));
    }
  }
  s = ClassifySlot{};
}
static void classify_release(wp_vocab *v, int slot) { classify_free(v, v->classify[slot]); }

// every rule of a model, each with the field it is about; nothing here needs a device
static void check_classify_model(const wp_classify_model *m) {
  if (!m) throw std::invalid_argument("classify: m is NULL");
  if (m->dim < 1 || m->dim > WP_CLASSIFY_MAX_DIM) throw std::invalid_argument("classify: dim must be in [1, 512]");
  if (m->n_labels < 1 || m->n_labels > WP_CLASSIFY_MAX_LABELS) throw std::invalid_argument("classify: n_labels must be in [1, 65535]");
  if (m->maxn < 0 || m->maxn > WP_CLASSIFY_MAX_MAXN) throw std::invalid_argument("classify: maxn must be in [0, 6]");
  if (m->minn < 0 || m->minn > m->maxn) throw std::invalid_argument("classify: minn must be in [0, maxn]");
  if (m->minn == 0 && m->maxn > 0) throw std::invalid_argument("classify: minn must be 1 at least where maxn > 0");
  if (m->word_ngrams < 1 || m->word_ngrams > WP_CLASSIFY_MAX_WORD_NGRAMS) throw std::invalid_argument("classify: word_ngrams must be in [1, 5]");
  if (m->bucket < 0) throw std::invalid_argument("classify: bucket must not be negative");
  if (m->bucket == 0 && (m->maxn > 0 || m->word_ngrams > 1)) throw std::invalid_argument("classify: bucket must be 1 at least where maxn > 0 or word_ngrams > 1");
  if (m->n_words < 0) throw std::invalid_argument("classify: n_words must not be negative");
  if (m->reserved != 0) throw std::invalid_argument("classify: reserved must be 0");
  if (m->n_words >= (int64_t(1) << 31) || m->bucket >= (int64_t(1) << 31) || m->n_words + m->bucket >= (int64_t(1) << 31)) {
    throw std::length_error("classify: n_words + bucket must stay below 2^31");
  }
  if (m->n_words + m->bucket == 0) throw std::invalid_argument("classify: n_words + bucket must be 1 at least");
  if (!m->input) throw std::invalid_argument("classify: input is NULL");
  if (!m->output) throw std::invalid_argument("classify: output is NULL");
  if (m->n_words != 0) {
    if (!m->word_off) throw std::invalid_argument("classify: word_off is NULL");
    if (m->word_off[0] != 0) throw std::invalid_argument("classify: word_off must start at 0 and never descend: word 0");
    for (int64_t w = 0; w < m->n_words; w++) {
      if (m->word_off[w + 1] < m->word_off[w]) throw std::invalid_argument("classify: word_off must never descend: word " + std::to_string(w));
    }
    if (m->word_off[m->n_words] >= (int64_t(1) << 32)) throw std::length_error("classify: words holds 2^32 bytes or more");
    if (m->word_off[m->n_words] != 0 && !m->words) throw std::invalid_argument("classify: words is NULL");
  }
}

// The dictionary of a checked model: `cap` pairs (H, wid), a power of two >= 2 n_words and 16, wid 0xffffffff where the
// slot is empty; a word's home is H & (cap - 1), linear probing forward with wrap.  A word whose bytes an earlier word has
// is left out (first wins).  Returns the longest word's length through max_len and the word "</s>" through wid_eos.
static std::vector<uint2> classify_table(const wp_classify_model *m, uint32_t *max_len, int32_t *wid_eos) {
  size_t cap = 16;
  while (cap < 2 * static_cast<size_t>(m->n_words)) cap <<= 1;
  std::vector<uint2> table(cap, uint2{0u, 0xffffffffu});
  const uint8_t *pool = static_cast<const uint8_t *>(m->words);
  *max_len = 0;
  *wid_eos = -1;
  for (int64_t w = 0; w < m->n_words; w++) {
    const size_t a = static_cast<size_t>(m->word_off[w]), len = static_cast<size_t>(m->word_off[w + 1]) - a;
    const uint32_t h = cls_host_hash(pool + a, len);
    size_t slot = h & (cap - 1);
    bool dup = false;
    for (; table[slot].y != 0xffffffffu; slot = (slot + 1) & (cap - 1)) {
      const size_t b = static_cast<size_t>(m->word_off[table[slot].y]), blen = static_cast<size_t>(m->word_off[table[slot].y + 1]) - b;
      if (table[slot].x == h && blen == len && std::memcmp(pool + a, pool + b, len) == 0) {
        dup = true;
        break;
      }
    }
    if (dup) continue;
    table[slot] = uint2{h, static_cast<uint32_t>(w)};
    *max_len = std::max(*max_len, static_cast<uint32_t>(std::min<size_t>(len, UINT32_MAX)));
    if (len == 4 && std::memcmp(pool + a, "</s>", 4) == 0) *wid_eos = static_cast<int32_t>(w);
  }
  return table;
}

template <typename T>
static const T *classify_upload(const T *src, size_t count, hipStream_t st) {
  T *d = nullptr;
  WP_HIP(hipMalloc(&d, std::max<size_t>(count, 1) * sizeof(T)));
  if (count != 0 && hipMemcpyAsync(d, src, count * sizeof(T), hipMemcpyHostToDevice, st) != hipSuccess) {
    (void)hipFree(d);
    throw HipError("classify: a table of the model could not be copied to the device");
  }
  return d;
}

// the checked model m into the slot, on c's device; the slot's earlier model goes once the new one is there, and stays
// where the load fails
static void classify_load_on_device(wp_vocab *v, Context *c, int slot, const wp_classify_model *m) {
  uint32_t max_len = 0;
  int32_t wid_eos = -1;
  const std::vector<uint2> table = classify_table(m, &max_len, &wid_eos);
  std::vector<uint32_t> woff(static_cast<size_t>(m->n_words) + 1, 0u);
  for (int64_t w = 0; w <= m->n_words && m->n_words != 0; w++) woff[static_cast<size_t>(w)] = static_cast<uint32_t>(m->word_off[w]);
  ClassifySlot s;
  s.loaded = true;  // (from here on classify_free frees what is there)
  s.device = c->device;
  hipStream_t st = c->stream;
  const size_t rows_in = static_cast<size_t>(m->n_words + m->bucket);
  try {
    s.m.input = classify_upload(m->input, rows_in * m->dim, st);
    s.m.output = classify_upload(m->output, static_cast<size_t>(m->n_labels) * m->dim, st);
    s.m.table = classify_upload(table.data(), table.size(), st);
    s.m.pool = classify_upload(static_cast<const uint8_t *>(m->words), woff.back(), st);
    s.m.word_off = classify_upload(woff.data(), woff.size(), st);
    WP_HIP(hipStreamSynchronize(st));
  } catch (...) {
    classify_free(v, s);
    throw;
  }
  s.m.n_words = static_cast<uint32_t>(m->n_words);
  s.m.bucket = static_cast<uint32_t>(m->bucket);
  s.m.table_mask = static_cast<uint32_t>(table.size() - 1);
  s.m.max_word_len = max_len;
  s.m.dim = m->dim;
  s.m.n_labels = m->n_labels;
  s.m.minn = m->minn;
  s.m.maxn = m->maxn;
  s.m.word_ngrams = m->word_ngrams;
  s.m.wid_eos = wid_eos;
  s.n_words = m->n_words;
  s.bucket = m->bucket;
  classify_release(v, slot);  // (the statistics of the slot start again with the new model)
  v->classify[slot] = s;
}

// ---- a call ---------------------------------------------------------------------------------------------------------------------
struct ClassifyPlan {
  int slot = 0;
  bool want_logits = false, want_compact = false, keep_some = false;
  float min_prob = 0.0f;
  std::vector<uint32_t> keep_bits;  // a bit per label, where keep_labels names some
};

// every rule of the spec that reads no model, each with the field it is about; nothing here needs a device
static ClassifyPlan check_classify_spec(const wp_classify_spec *spec, const wp_classify_result *out) {
  if (!spec) throw std::invalid_argument("classify: spec is NULL");
  if (!out) throw std::invalid_argument("classify: out is NULL");
  ClassifyPlan p;
  p.slot = check_classify_slot(spec->slot);
  check_want("classify", spec->want, WP_CLASSIFY_WANT_LOGITS | WP_CLASSIFY_WANT_COMPACT);
  p.want_logits = (spec->want & WP_CLASSIFY_WANT_LOGITS) != 0;
  p.want_compact = (spec->want & WP_CLASSIFY_WANT_COMPACT) != 0;
  if (spec->pad != 0) throw std::invalid_argument("classify: pad must be 0");
  if (spec->pad2 != 0) throw std::invalid_argument("classify: pad2 must be 0");
  if (spec->reserved != 0) throw std::invalid_argument("classify: reserved must be 0");
  if (spec->n_keep < 0) throw std::invalid_argument("classify: n_keep must not be negative");
  if (spec->n_keep > 0 && !spec->keep_labels) throw std::invalid_argument("classify: keep_labels is NULL");
  if (!(spec->min_prob >= 0.0f && spec->min_prob <= 1.0f)) throw std::invalid_argument("classify: min_prob must be in [0, 1]");
  p.min_prob = spec->min_prob;
  return p;
}

// ... and, behind the rules of the batch, the two that read the model of the slot: it is there, and it has the kept labels
static void check_classify_labels(const wp_vocab *v, const wp_classify_spec *spec, ClassifyPlan *p) {
  const ClassifySlot &s = v->classify[p->slot];
  if (!s.loaded) throw std::invalid_argument("classify: slot " + std::to_string(p->slot) + " holds no model");
  if (!spec->keep_labels) return;
  p->keep_some = true;
  p->keep_bits.assign(static_cast<size_t>(s.m.n_labels) / 32 + 1, 0u);
  for (int32_t k = 0; k < spec->n_keep; k++) {
    const int32_t l = spec->keep_labels[k];
    if (l < 0 || l >= s.m.n_labels) throw std::invalid_argument("classify: keep_labels[" + std::to_string(k) + "] is no label of the model");
    p->keep_bits[static_cast<size_t>(l) / 32] |= 1u << (l % 32);
  }
}

constexpr TextLayer kClsLayer{"classify", "classify", "gathers or stores outside the tile, token, feature, partial or row arrays skipped",
                              kScalarClsBad, kScalarClsKept, kScalarClsElems, kScalarClsWindows, kScalarClsTokens, kScalarClsFound, kScalarClsOutBytes,
                              kScalarCls, 1};

static wp_classify_stats &begin_classify_stats(wp_vocab *v, int slot, size_t n_rows) {
  ClassifySlot &s = v->classify[slot];
  s.called = true;
  s.last = wp_classify_stats{};
  s.last.n_rows = static_cast<int64_t>(n_rows);
  return s.last;
}

// the lanes that read one row of `input`: the power of two that covers dim, 64 at the most
static int classify_lanes_per_row(int dim) {
  int lpr = 1;
  while (lpr < dim && lpr < kWave) lpr <<= 1;
  return lpr;
}

// The batch `in` (n_rows >= 1), on c's stream.  The results are device pointers into c->classify_rows (label, prob,
// n_features, reasons, logits) and c->classify_out (the compact form), valid until the handle's next call.  Waits: the
// sizes; the tokens; the features; with the compact form the kept count; the one that ends the call.
static void classify_on_device(wp_vocab *v, Context *c, const RaggedIn &in, const ClassifyPlan &plan, wp_classify_result *R) {
  const TextLayer &L = kClsLayer;
  const ClsModel m = v->classify[plan.slot].m;
  const size_t n = in.n_rows, n1 = n + 1, n_labels = static_cast<size_t>(m.n_labels), dim = static_cast<size_t>(m.dim);
  wp_classify_stats &ps = begin_classify_stats(v, plan.slot, n);
  *R = wp_classify_result{};
  R->n_rows = static_cast<int64_t>(n);
  R->n_labels = m.n_labels;
  hipStream_t st = c->stream;
  const bool guard = v->arena_guard || EnvOptions::get().arena_guard;
  // WP_OPT_STAGE_TIMING: kMarkStart, kMarkCounted (intake, token list), kMarkSorted (feature list), kMarkScanned (row
  // gathers, partial sums), kMarkWalked (output stage, compact form)
  const bool timing = v->stage_timing;
  begin_stage_timing(c, timing, st);

  // ---- the per-row arrays, the offset check ----------------------------------------------------------------------------------
  Arena ra(&c->classify_rows, guard);
  TextRows rows;  // (its one signal per row is n_features)
  uint32_t *d_foff = nullptr, *d_keep_bits = nullptr;
  int32_t *d_label = nullptr;
  float *d_prob = nullptr, *d_logits = nullptr;
  for (int pass = 0; pass < 2; pass++) {
    rows.take(ra, n, 1);
    d_foff = ra.take<uint32_t>(n1);
    d_label = ra.take<int32_t>(n);
    d_prob = ra.take<float>(n);
    d_keep_bits = ra.take<uint32_t>(n_labels / 32 + 1);
    if (plan.want_logits) d_logits = ra.take<float>(n * n_labels);
    if (pass == 0) ra.commit();
  }
  ra.arm(st);
  rows.queue(c, L, in, st);
  const size_t nb = rows.read(c, L, in, st);
  const uint32_t *d32 = static_cast<const uint32_t *>(in.d_data);
  if (plan.keep_some) WP_HIP(hipMemcpyAsync(d_keep_bits, plan.keep_bits.data(), plan.keep_bits.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));

  // ---- the token pass: the document bits, the starts of every tile, their scan, the list -----------------------------------
  const size_t n_tiles = cdiv(nb, kClsTile), nt1 = n_tiles + 1;
  Arena ta(&c->classify_tiles, guard);
  uint32_t *d_docbits = nullptr, *d_tiles = nullptr, *d_ftiles = nullptr, *d_ttmp = nullptr, *d_gpre = nullptr;
  uint8_t *d_cnt = nullptr;
  for (int pass = 0; pass < 2; pass++) {
    d_docbits = ta.take<uint32_t>(nb / 32 + 2);
    d_tiles = ta.take<uint32_t>(nt1);
    d_ftiles = ta.take<uint32_t>(nt1);
    d_ttmp = ta.take<uint32_t>(cdiv(nt1, kScanTile) + 8);
    d_gpre = ta.take<uint32_t>(nb / kClsGroup + 2);
    d_cnt = ta.take<uint8_t>(nb + 1);
    if (pass == 0) ta.commit();
  }
  ta.arm(st);
  WP_HIP(hipMemsetAsync(d_docbits, 0, (nb / 32 + 2) * sizeof(uint32_t), st));
  WP_HIP(hipMemsetAsync(d_tiles, 0, nt1 * sizeof(uint32_t), st));
  WP_HIP(hipMemsetAsync(d_ftiles, 0, nt1 * sizeof(uint32_t), st));
  size_t nt = 0;
  if (nb != 0) {
    hipLaunchKernelGGL(cls_docbits_kernel, count_grid(n), dim3(kBlock), 0, st, static_cast<const uint32_t *>(rows.d_boff), n, nb, d_docbits);
    hipLaunchKernelGGL(cls_token_kernel<false>, dim3(n_tiles), dim3(kBlock), 0, st, d32, nb, static_cast<const uint32_t *>(d_docbits),
                       static_cast<const uint32_t *>(rows.d_boff), n, m, d_tiles, ClsTokens{}, static_cast<uint32_t *>(nullptr));
    device_exclusive_scan(d_tiles, d_tiles, nt1, d_ttmp, c->d_scalars + L.words, st);
    WP_LAUNCH_CHECK();
    queue_scalar_slots(c, L.words, L.words, st);
    WP_HIP(hipStreamSynchronize(st));
    nt = c->h_scalars[L.words];
    if (nt > nb / 2 + 1) throw HipError("classify: more tokens than the bytes have room for");
  }
  Arena ka(&c->classify_toks, guard);
  ClsTokens toks{};
  for (int pass = 0; pass < 2; pass++) {
    toks.hash = ka.take<uint32_t>(nt);
    toks.doc = ka.take<uint32_t>(nt);
    toks.wid = ka.take<int32_t>(nt);
    if (pass == 0) ka.commit();
  }
  ka.arm(st);
  toks.n = nt;
  if (nb != 0) {
    hipLaunchKernelGGL(cls_token_kernel<true>, dim3(n_tiles), dim3(kBlock), 0, st, d32, nb, static_cast<const uint32_t *>(d_docbits),
                       static_cast<const uint32_t *>(rows.d_boff), n, m, d_tiles, toks, c->d_scalars + L.lines);
    WP_LAUNCH_CHECK();
  }
  if (timing) WP_HIP(hipEventRecord(c->ev[kMarkCounted], st));

  // ---- the feature list: the features of every byte and tile, their scan, the ids in text order, the offsets of the rows ------
  size_t nf = 0;
  if (nb != 0) {
    hipLaunchKernelGGL(cls_feature_kernel<false>, dim3(n_tiles), dim3(kBlock), 0, st, d32, nb, static_cast<const uint32_t *>(d_docbits), m,
                       static_cast<const uint32_t *>(d_tiles), toks, d_cnt, d_ftiles, d_gpre, static_cast<uint32_t *>(nullptr), size_t(0));
    device_exclusive_scan(d_ftiles, d_ftiles, nt1, d_ttmp, c->d_scalars + kScalarClsFeatures, st, nullptr,
                          reinterpret_cast<unsigned long long *>(c->d_scalars + kScalarClsFeatures64));
    WP_LAUNCH_CHECK();
    queue_scalar_slots(c, kScalarClsFeatures, kScalarClsFeatures64, st);
    WP_HIP(hipStreamSynchronize(st));
    unsigned long long nf64;
    std::memcpy(&nf64, c->h_scalars + kScalarClsFeatures64, sizeof(nf64));
    if (nf64 > UINT32_MAX) throw std::length_error("classify: the batch lists more than UINT32_MAX features");
    if (nf64 > static_cast<unsigned long long>(nb) * kClsMaxPerByte) throw HipError("classify: more features than the bytes can list");
    nf = static_cast<size_t>(nf64);
  }
  const int lpr = classify_lanes_per_row(m.dim);
  const size_t unit_len = static_cast<size_t>(kClsUnitSteps) * lpr, n_units = cdiv(nf, unit_len), n_slots = n_units + n;
  Arena fa(&c->classify_feats, guard);
  uint32_t *d_feats = nullptr;
  float *d_partial = nullptr;
  for (int pass = 0; pass < 2; pass++) {
    d_feats = fa.take<uint32_t>(nf);
    d_partial = fa.take<float>(n_slots * dim);
    if (pass == 0) fa.commit();
  }
  fa.arm(st);
  if (nb != 0) {
    hipLaunchKernelGGL(cls_feature_kernel<true>, dim3(n_tiles), dim3(kBlock), 0, st, d32, nb, static_cast<const uint32_t *>(d_docbits), m,
                       static_cast<const uint32_t *>(d_tiles), toks, d_cnt, d_ftiles, d_gpre, d_feats, nf);
  }
  hipLaunchKernelGGL(cls_row_features_kernel, count_grid(n1), dim3(kBlock), 0, st, static_cast<const uint32_t *>(rows.d_boff), n, nb,
                     static_cast<const uint8_t *>(d_cnt), static_cast<const uint32_t *>(d_gpre), static_cast<const uint32_t *>(c->d_scalars + kScalarClsFeatures), d_foff);
  WP_LAUNCH_CHECK();
  if (timing) WP_HIP(hipEventRecord(c->ev[kMarkSorted], st));

  // ---- the row gathers: one partial per (unit, document) ----------------------------------------------------------------------
  if (nf != 0) {
    hipLaunchKernelGGL(cls_accumulate_kernel, count_grid(n_units * lpr), dim3(kBlock), 0, st, static_cast<const uint32_t *>(d_feats), nf,
                       static_cast<const uint32_t *>(d_foff), n, m, lpr, d_partial, n_slots);
    WP_LAUNCH_CHECK();
  }
  if (timing) WP_HIP(hipEventRecord(c->ev[kMarkScanned], st));

  // ---- the output stage, the kept rows ---------------------------------------------------------------------------------------------
  const ClsOut o{d_label, d_prob, d_logits, rows.d_sig, rows.d_reasons, rows.d_keep};
  hipLaunchKernelGGL(cls_output_kernel, dim3(cdiv(n1, kBlock / kWave)), dim3(kBlock), 0, st, static_cast<const uint32_t *>(d_foff), n, m, lpr,
                     static_cast<const float *>(d_partial), n_slots, plan.keep_some ? static_cast<const uint32_t *>(d_keep_bits) : nullptr, plan.min_prob, o,
                     reinterpret_cast<unsigned long long *>(c->d_scalars + L.counters));
  WP_LAUNCH_CHECK();
  Arena oa(&c->classify_out, guard);
  KeptRows kept;
  if (plan.want_compact) {
    kept.count(c, L.name, rows.d_keep, rows.d_keep_pos, n, rows.d_stmp, L.kept, st);
    for (int pass = 0; pass < 2; pass++) {
      kept.take(oa, nb);
      if (pass == 0) oa.commit();
    }
    oa.arm(st);
    kept.queue(c, in, rows.d_keep, rows.d_keep_pos, rows.d_boff, nb, rows.d_out_len, rows.d_out_pos, rows.d_stmp, L.out_bytes, st);
    WP_LAUNCH_CHECK();
  } else {
    device_exclusive_scan(rows.d_keep, rows.d_keep_pos, n1, rows.d_stmp, c->d_scalars + L.kept, st);
  }
  if (timing) WP_HIP(hipEventRecord(c->ev[kMarkWalked], st));
  queue_scalar_slots(c, L.kept, L.counters, st);
  WP_HIP(hipStreamSynchronize(st));
  unsigned long long features;
  std::memcpy(&features, c->h_scalars + L.counters, sizeof(features));
  ps.n_kept = c->h_scalars[L.kept];
  ps.n_features = static_cast<int64_t>(features);
  ps.n_tokens = static_cast<int64_t>(nt + n);
  ps.n_found = static_cast<int64_t>(c->h_scalars[L.lines]) + (m.wid_eos >= 0 ? static_cast<int64_t>(n) : 0);
  if (features != nf + (m.wid_eos >= 0 ? n : 0)) throw HipError("classify: the rows do not sum to the features of the list");
  if (timing) end_four_stage_timing(v, c);
  throw_if_group_oob(kSiteQuality, L.oob_name, L.oob_skipped, kSiteOverlap, "gathers or stores outside the row arrays skipped");
  for (const Arena *a : {&ra, &ta, &ka, &fa, &oa}) check_arena_guard(c, *a, st, L.name);
  R->label = d_label;
  R->prob = d_prob;
  R->logits = d_logits;
  R->n_features = reinterpret_cast<int64_t *>(rows.d_sig);
  R->reasons = rows.d_reasons;
  if (plan.want_compact) kept.hand_out(R, c->h_scalars[L.out_bytes], 1);
}

}  // namespace wp
