// classify.h — kernels of the linear classifier (include/wordpiece_amd_classify.h; host path: classify_path.h).
// Four stages, every one flat over bytes, tokens or features:
//   1. token pass (cls_token_kernel, count then write): a tile of kClsTile bytes with its halo goes into LDS once, as
//      bytes and as a flag plane (white space / outside the text, first byte of a document).  Token starts are counted per
//      tile, scanned, and the token list is written: H, wid, document.  The lane of a token start hashes the token, a
//      sequential walk that ends one byte past the longest model word unless word n-grams need the whole hash, and probes
//      the dictionary, an open-addressing table of (H, wid) pairs read a pair a step, whose hits are confirmed byte by byte
//      against the word pool.
//   2. feature list (cls_feature_kernel, count then write): one lane per byte.  The lane of a token start lists the token's
//      word id and word n-grams, then the grams that start at '<'; every lane whose byte starts a character lists the grams
//      from there, FNV running on from gram n to gram n + 1.  The ids go to one flat list in text order, 4 bytes each;
//      cls_row_features_kernel turns the per-byte counts into the feature offsets of the documents.
//   3. accumulation (cls_accumulate_kernel): the list is cut into units of kClsUnitSteps * lanes-per-row features.  A row of
//      `input` is read by lpr = min(64, 2^ceil(log2 dim)) consecutive lanes, dim consecutive floats: at dim 16 one wave load
//      brings four rows of 64 bytes.  A unit sums its rows per document in registers, in list order, and writes one partial
//      per (unit, document) to slot unit + document: the pairs that occur form a staircase, so the slots are distinct, each
//      written once, and a document's partials are consecutive.
//   4. output stage (cls_output_kernel): one wave per document adds the partials in unit order into LDS (the second
//      sequential walk: a document's partials, one per unit of its features, are added by one wave), then the row of
//      "</s>", and runs the [dim] x [dim, n_labels] product with a fixed k order, a label per lane, fused with the division
//      by F, the max / argmax, the sum of exp (logits recomputed, the same bits, so none is stored unless asked for), and the
//      three rule bits.
// No floating-point atomic anywhere: lanes meet through integer adds, ballots and fixed shuffle trees alone.
#pragma once
#include "../../include/wordpiece_amd_classify.h"
#include "common.h"
#include "primitives.h"

namespace wp {

constexpr int kClsItems = 4;                      // bytes per lane of a tile, one per trip
constexpr int kClsTile = kBlock * kClsItems;      // T: bytes per workgroup of the token and feature passes
constexpr int kClsHaloL = 4;                      // bytes in front of a tile: the start of a 4-byte token ("</s>")
constexpr int kClsHaloR = 28;                     // bytes behind it: 4 * maxn + 1 = 25 of a gram in valid UTF-8, rounded to words
constexpr int kClsSpan = kClsHaloL + kClsTile + kClsHaloR;
constexpr int kClsUnitSteps = 4;                  // features a lane group of the accumulation takes per wave of a unit: unit = 4 * lpr
constexpr int kClsMaxCols = 8;                    // columns of a row one lane holds: 512 / 64
constexpr int kClsMaxPerByte = 17;                // features one byte can list: wid, 4 word n-grams, 6 + 6 grams
constexpr uint32_t kClsFnvInit = 2166136261u, kClsFnvPrime = 16777619u, kClsHashEos = 3617362777u;
constexpr unsigned long long kClsWordMul = 116049371ull;
constexpr uint32_t kClsFlagBreak = 1, kClsFlagDoc = 2;
constexpr int kClsGroup = 64;                     // bytes per entry of the feature prefix (one wave of one trip)

// what a kernel knows of the model (device pointers; table: cap pairs of (H, wid), wid -1 = empty)
struct ClsModel {
  const float *input, *output;
  const uint2 *table;
  const uint8_t *pool;
  const uint32_t *word_off;
  uint32_t n_words, bucket, table_mask, max_word_len;
  int32_t dim, n_labels, minn, maxn, word_ngrams, wid_eos;
};

struct ClsTokens {
  uint32_t *hash, *doc;
  int32_t *wid;
  size_t n;
};

__device__ __forceinline__ uint32_t cls_fnv(uint32_t h, uint32_t byte) {
  return (h ^ static_cast<uint32_t>(static_cast<int32_t>(static_cast<int8_t>(byte)))) * kClsFnvPrime;
}
__device__ __forceinline__ bool cls_is_space(uint32_t b) { return b == 0x20 || (b >= 0x09 && b <= 0x0d) || b == 0; }
__device__ __forceinline__ bool cls_is_cont(uint32_t b) { return (b & 0xc0u) == 0x80u; }

// The text around a tile: bytes and flags from LDS inside [lo, lo + kClsSpan), from memory outside it (a character of
// stray continuation bytes or a long token can reach past any halo).  Positions are signed: lo is -4 in tile 0.
struct ClsView {
  const uint8_t *sb, *fl;  // LDS
  long long lo;
  const uint8_t *text;
  const uint32_t *docbits;
  long long nb;
  __device__ __forceinline__ uint32_t flag(long long p) const {
    if (p >= lo && p < lo + kClsSpan) return fl[p - lo];
    if (p < 0 || p >= nb) return kClsFlagBreak;
    return (cls_is_space(text[p]) ? kClsFlagBreak : 0u) | (((docbits[p >> 5] >> (p & 31)) & 1u) ? kClsFlagDoc : 0u);
  }
  __device__ __forceinline__ uint32_t byte(long long p) const {
    if (p >= lo && p < lo + kClsSpan) return sb[p - lo];
    return (p < 0 || p >= nb) ? 0u : text[p];
  }
  // p ends a token in front of it / starts one: the byte is white space, outside the text, or the first of a document
  __device__ __forceinline__ bool breaks(long long p) const { return flag(p) != 0; }
  __device__ __forceinline__ bool token_start(long long p) const {
    const uint32_t f = flag(p);
    return (f & kClsFlagBreak) == 0 && ((f & kClsFlagDoc) != 0 || (flag(p - 1) & kClsFlagBreak) != 0);
  }
};

// the tile of workgroup blockIdx.x into LDS: whole words of the text (the buffer is readable in whole words), the flags
__device__ __forceinline__ ClsView cls_load_tile(const uint32_t *__restrict__ text32, const uint32_t *__restrict__ docbits, size_t nb, uint32_t *sw, uint8_t *fl) {
  const long long base = static_cast<long long>(blockIdx.x) * kClsTile, lo = base - kClsHaloL, n = static_cast<long long>(nb);
  for (int i = threadIdx.x; i < kClsSpan / 4; i += kBlock) {
    const long long p = lo + 4ll * i;
    sw[i] = (p >= 0 && p < n) ? text32[p >> 2] : 0u;
  }
  __syncthreads();
  const uint8_t *sb = reinterpret_cast<const uint8_t *>(sw);
  for (int i = threadIdx.x; i < kClsSpan; i += kBlock) {
    const long long p = lo + i;
    uint32_t f = kClsFlagBreak;
    if (p >= 0 && p < n) f = (cls_is_space(sb[i]) ? kClsFlagBreak : 0u) | (((docbits[p >> 5] >> (p & 31)) & 1u) ? kClsFlagDoc : 0u);
    fl[i] = static_cast<uint8_t>(f);
  }
  __syncthreads();
  return ClsView{sb, fl, lo, reinterpret_cast<const uint8_t *>(text32), docbits, n};
}

// ---- the documents: a bit per first byte ----------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void cls_docbits_kernel(const uint32_t *__restrict__ boff, size_t n_rows, size_t nb, uint32_t *__restrict__ docbits) {
  const size_t r = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (r >= n_rows) return;
  const uint32_t b = boff[r];
  if (b < nb) atomicOr(&docbits[b >> 5], 1u << (b & 31));  // (empty documents behind the last byte start at nb)
}

// the document of byte p < nb: the last row that starts at or in front of it
__device__ __forceinline__ uint32_t cls_row_of(const uint32_t *__restrict__ boff, size_t n_rows, uint32_t p) {
  size_t lo = 0, hi = n_rows;  // boff[lo] <= p < boff[hi]
  while (hi - lo > 1) {
    const size_t mid = lo + (hi - lo) / 2;
    if (boff[mid] <= p) lo = mid; else hi = mid;
  }
  return static_cast<uint32_t>(lo);
}

// ---- the dictionary ---------------------------------------------------------------------------------------------------------
// the word of the token [start, start + len) with hash h, or -1
__device__ __forceinline__ int32_t cls_probe(const ClsModel &m, const ClsView &v, long long start, uint32_t len, uint32_t h) {
  uint32_t slot = h & m.table_mask;
  for (uint32_t tries = 0; tries <= m.table_mask; tries++, slot = (slot + 1) & m.table_mask) {
    const uint2 e = m.table[slot];
    if (e.y == 0xffffffffu) return -1;
    if (e.x != h || !wp_checked(e.y < m.n_words, kSiteQuality)) continue;
    const uint32_t a = m.word_off[e.y];
    if (m.word_off[e.y + 1] - a != len) continue;
    bool same = true;
    for (uint32_t i = 0; i < len && same; i++) same = m.pool[a + i] == v.byte(start + i);
    if (same) return static_cast<int32_t>(e.y);
  }
  return -1;
}

// ---- 1. the token pass --------------------------------------------------------------------------------------------------------
// kWrite false: tiles[t] = the token starts of tile t.  kWrite true: tiles holds the scan; the list is written.
template <bool kWrite>
__global__ __launch_bounds__(kBlock) void cls_token_kernel(const uint32_t *__restrict__ text32, size_t nb, const uint32_t *__restrict__ docbits,
                                                           const uint32_t *__restrict__ boff, size_t n_rows, ClsModel m, uint32_t *__restrict__ tiles, ClsTokens toks,
                                                           uint32_t *__restrict__ n_found) {
  __shared__ uint32_t sw[kClsSpan / 4];
  __shared__ uint8_t fl[kClsSpan];
  __shared__ uint32_t sm[8];
  const ClsView v = cls_load_tile(text32, docbits, nb, sw, fl);
  const long long base = static_cast<long long>(blockIdx.x) * kClsTile;
  uint32_t running = kWrite ? tiles[blockIdx.x] : 0u, found = 0;
  for (int it = 0; it < kClsItems; it++) {
    const long long p = base + it * kBlock + threadIdx.x;
    const bool is_start = v.token_start(p);
    uint32_t total;
    const uint32_t ex = block_excl_sum(is_start ? 1u : 0u, sm, total);
    if (kWrite && is_start) {
      const size_t g = static_cast<size_t>(running) + ex;
      const bool hash_all = m.word_ngrams > 1;
      uint32_t h = kClsFnvInit;
      // (the walk ends one byte past the longest model word where only the word id is wanted: such a token has none, and
      // nothing else reads its length or its hash)
      const long long cap = hash_all ? v.nb : static_cast<long long>(m.max_word_len) + 1;
      long long e = p;
      for (; (!v.breaks(e) || e == p) && e - p < cap; e++) h = cls_fnv(h, v.byte(e));
      const uint32_t len = static_cast<uint32_t>(e - p);
      const int32_t wid = len <= m.max_word_len ? cls_probe(m, v, p, len, h) : -1;
      found += wid >= 0 ? 1u : 0u;
      if (wp_checked(g < toks.n, kSiteQuality)) {
        toks.hash[g] = h;
        toks.wid[g] = wid;
        toks.doc[g] = cls_row_of(boff, n_rows, static_cast<uint32_t>(p));
      }
    }
    running += total;
  }
  if (!kWrite) {
    if (threadIdx.x == 0) tiles[blockIdx.x] = running;
  } else {
    found = wave_reduce_sum(found);
    if (lane_id() == 0 && found != 0) atomicAdd(n_found, found);
  }
}

// ---- 2. the feature list --------------------------------------------------------------------------------------------------------
// The grams that start at byte p of a token (bow: p is its first byte and the grams start at the '<' in front of it) -> their
// number; out (nullptr: count only) gets their features in order of n.  Byte p itself belongs to the token even where it
// carries the document flag; every later byte with a flag ends the token.
__device__ __forceinline__ int cls_grams(const ClsView &v, long long p, bool bow, const ClsModel &m, uint32_t *out) {
  uint32_t h = kClsFnvInit;
  long long j = p;
  int cnt = 0;
  bool at_end = false;  // the gram holds the '>' behind the token
  for (int n = 1; n <= m.maxn && !at_end; n++) {
    if (n == 1 && bow) {
      h = cls_fnv(h, '<');
    } else if (j != p && v.breaks(j)) {
      h = cls_fnv(h, '>');
      at_end = true;
    } else {
      h = cls_fnv(h, v.byte(j));
      j++;
    }
    while (!at_end && (j == p || !v.breaks(j)) && cls_is_cont(v.byte(j))) {
      h = cls_fnv(h, v.byte(j));
      j++;
    }
    if (n >= m.minn && !(n == 1 && (bow || at_end))) {
      if (out) out[cnt] = m.n_words + h % m.bucket;
      cnt++;
    }
  }
  return cnt;
}

// whether the token that holds the non-break byte p is the four bytes "</s>"
__device__ __forceinline__ bool cls_in_eos_literal(const ClsView &v, long long p) {
  long long s = p;
  for (int k = 0; k < 3 && !v.token_start(s); k++) s--;
  if (!v.token_start(s)) return false;
  return v.byte(s) == '<' && v.byte(s + 1) == '/' && v.byte(s + 2) == 's' && v.byte(s + 3) == '>' && !v.breaks(s + 1) && !v.breaks(s + 2) && !v.breaks(s + 3) &&
         v.breaks(s + 4);
}

// The features of byte p, in the order of the list: at a token start (token g) the word id, the word n-grams and the
// grams from '<'; at every character start the grams from there.  -> their number; out: nullptr, or room for them.
__device__ __forceinline__ int cls_byte_features(const ClsView &v, long long p, bool is_start, size_t g, const ClsModel &m, const ClsTokens &toks, uint32_t *out) {
  if ((v.flag(p) & kClsFlagBreak) != 0) return 0;
  int cnt = 0;
  if (is_start && wp_checked(g < toks.n, kSiteQuality)) {
    const int32_t wid = toks.wid[g];
    if (wid >= 0) {
      if (out) out[cnt] = static_cast<uint32_t>(wid);
      cnt++;
    }
    if (m.word_ngrams > 1) {
      const uint32_t r = toks.doc[g];
      unsigned long long h = static_cast<unsigned long long>(static_cast<long long>(static_cast<int32_t>(toks.hash[g])));
      for (int k = 1; k < m.word_ngrams; k++) {
        const size_t j = g + k;
        const bool eos = j >= toks.n || toks.doc[j] != r;
        const int32_t s = static_cast<int32_t>(eos ? kClsHashEos : toks.hash[j]);
        h = h * kClsWordMul + static_cast<unsigned long long>(static_cast<long long>(s));
        if (out) out[cnt] = m.n_words + static_cast<uint32_t>(h % m.bucket);
        cnt++;
        if (eos) break;
      }
    }
  }
  if (m.maxn > 0 && !cls_in_eos_literal(v, p)) {
    if (is_start) cnt += cls_grams(v, p, true, m, out ? out + cnt : nullptr);
    if (!cls_is_cont(v.byte(p))) cnt += cls_grams(v, p, false, m, out ? out + cnt : nullptr);
  }
  return cnt;
}

// kWrite false: cnt[p] = the features of byte p, ftiles[t] = those of tile t.  kWrite true: ftiles holds the scan; the ids
// are written at their places and gpre[p / 64] = the features in front of byte p for every p that starts a group.
template <bool kWrite>
__global__ __launch_bounds__(kBlock) void cls_feature_kernel(const uint32_t *__restrict__ text32, size_t nb, const uint32_t *__restrict__ docbits, ClsModel m,
                                                             const uint32_t *__restrict__ tiles, ClsTokens toks, uint8_t *__restrict__ cnt,
                                                             uint32_t *__restrict__ ftiles, uint32_t *__restrict__ gpre, uint32_t *__restrict__ feats, size_t n_feats) {
  __shared__ uint32_t sw[kClsSpan / 4];
  __shared__ uint8_t fl[kClsSpan];
  __shared__ uint32_t sm[8], sm2[8];
  const ClsView v = cls_load_tile(text32, docbits, nb, sw, fl);
  const long long base = static_cast<long long>(blockIdx.x) * kClsTile;
  uint32_t tok_running = tiles[blockIdx.x], running = kWrite ? ftiles[blockIdx.x] : 0u;
  for (int it = 0; it < kClsItems; it++) {
    const long long p = base + it * kBlock + threadIdx.x;
    const bool inside = p < static_cast<long long>(nb), is_start = inside && v.token_start(p);
    uint32_t tok_total, total;
    const uint32_t tok_ex = block_excl_sum(is_start ? 1u : 0u, sm, tok_total);
    const size_t g = static_cast<size_t>(tok_running) + tok_ex;
    uint32_t c = 0;
    if (!kWrite) {
      if (inside) {
        c = static_cast<uint32_t>(cls_byte_features(v, p, is_start, g, m, toks, nullptr));
        cnt[p] = static_cast<uint8_t>(c);
      }
    } else if (inside) {
      c = cnt[p];
    }
    const uint32_t ex = block_excl_sum(c, sm2, total);
    if (kWrite && inside) {
      const size_t at = static_cast<size_t>(running) + ex;
      if (lane_id() == 0) gpre[p / kClsGroup] = static_cast<uint32_t>(at);
      if (c != 0 && wp_checked(c <= kClsMaxPerByte && at + c <= n_feats, kSiteQuality)) {
        uint32_t mine[kClsMaxPerByte];
        const int wrote = cls_byte_features(v, p, is_start, g, m, toks, mine);
        for (int k = 0; k < kClsMaxPerByte; k++) {
          if (k < wrote && k < static_cast<int>(c)) feats[at + k] = mine[k];
        }
      }
    }
    tok_running += tok_total;
    running += total;
  }
  if (!kWrite && threadIdx.x == 0) ftiles[blockIdx.x] = running;
}

// foff[r], r <= n_rows: the features in front of the first byte of document r (n_feats behind the text)
__global__ __launch_bounds__(kBlock) void cls_row_features_kernel(const uint32_t *__restrict__ boff, size_t n_rows, size_t nb, const uint8_t *__restrict__ cnt,
                                                                  const uint32_t *__restrict__ gpre, const uint32_t *__restrict__ n_feats, uint32_t *__restrict__ foff) {
  const size_t r = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (r > n_rows) return;
  const size_t b = boff[r];
  uint32_t f = *n_feats;
  if (b < nb) {
    f = gpre[b / kClsGroup];
    for (size_t q = b - b % kClsGroup; q < b; q++) f += cnt[q];
  }
  foff[r] = f;
}

// ---- 3. the accumulation ----------------------------------------------------------------------------------------------------------
// lpr lanes read a row (a power of two, 64 at most); a lane group takes kClsUnitSteps * lpr consecutive features, its unit.
// partial[(unit + document) * dim + k]: the sum of column k over the features of the document inside the unit.
__global__ __launch_bounds__(kBlock) void cls_accumulate_kernel(const uint32_t *__restrict__ feats, size_t n_feats, const uint32_t *__restrict__ foff, size_t n_rows,
                                                                ClsModel m, int lpr, float *__restrict__ partial, size_t n_slots) {
  const size_t unit_len = static_cast<size_t>(kClsUnitSteps) * lpr;
  const size_t unit = (static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x) / lpr;
  const int sub = threadIdx.x % lpr;
  const size_t first = unit * unit_len, last = min(n_feats, first + unit_len);
  if (first >= n_feats) return;
  const size_t rows_in = static_cast<size_t>(m.n_words) + m.bucket;
  // the document of the unit's first feature: the last r with foff[r] <= first (documents without a feature share an offset)
  size_t lo = 0, hi = n_rows;
  while (hi - lo > 1) {
    const size_t mid = lo + (hi - lo) / 2;
    if (foff[mid] <= first) lo = mid; else hi = mid;
  }
  size_t r = lo;
  uint32_t next = foff[r + 1];
  float acc[kClsMaxCols];
#pragma unroll
  for (int k = 0; k < kClsMaxCols; k++) acc[k] = 0.0f;
  auto flush = [&] {
    const size_t slot = unit + r;
    if (wp_checked(slot < n_slots, kSiteQuality)) {
#pragma unroll
      for (int k = 0; k < kClsMaxCols; k++) {
        const int col = sub + k * lpr;
        if (col < m.dim) partial[slot * m.dim + col] = acc[k];
        acc[k] = 0.0f;
      }
    }
  };
  for (size_t i = first; i < last; i++) {
    if (i >= next) {
      flush();
      while (r + 1 < n_rows && foff[r + 1] <= i) r++;
      next = foff[r + 1];
    }
    const uint32_t f = feats[i];
    if (!wp_checked(f < rows_in, kSiteQuality)) continue;
    const float *row = m.input + static_cast<size_t>(f) * m.dim;
#pragma unroll
    for (int k = 0; k < kClsMaxCols; k++) {
      const int col = sub + k * lpr;
      if (col < m.dim) acc[k] += row[col];
    }
  }
  flush();
}

// ---- 4. the output stage --------------------------------------------------------------------------------------------------------
struct ClsOut {
  int32_t *label;
  float *prob, *logits;  // logits: nullptr unless asked for
  long long *n_features;
  uint32_t *reasons, *keep;
};

// the (value, index) pair with the larger value, the smaller index on ties, over the wave
__device__ __forceinline__ void cls_wave_argmax(float &best, int32_t &at) {
#pragma unroll
  for (int d = kWave / 2; d > 0; d >>= 1) {
    const float ob = __shfl_xor(best, d, kWave);
    const int32_t oa = __shfl_xor(at, d, kWave);
    if (oa >= 0 && (at < 0 || ob > best || (ob == best && oa < at))) {
      best = ob;
      at = oa;
    }
  }
}
__device__ __forceinline__ float cls_wave_sum(float v) {
#pragma unroll
  for (int d = kWave / 2; d > 0; d >>= 1) v += __shfl_xor(v, d, kWave);
  return v;
}

// one wave per document; keep_bits: a bit per label (nullptr: every label); keep[r] = reasons == 0 (keep[n_rows] = 0)
__global__ __launch_bounds__(kBlock) void cls_output_kernel(const uint32_t *__restrict__ foff, size_t n_rows, ClsModel m, int lpr, const float *__restrict__ partial,
                                                            size_t n_slots, const uint32_t *__restrict__ keep_bits, float min_prob, ClsOut out,
                                                            unsigned long long *__restrict__ counters) {
  __shared__ float s_all[kBlock / kWave][WP_CLASSIFY_MAX_DIM];
  const int lane = lane_id(), w = wave_id();
  const size_t r = static_cast<size_t>(blockIdx.x) * (kBlock / kWave) + w;
  if (r == n_rows && lane == 0) out.keep[r] = 0;
  if (r >= n_rows) return;
  float *S = s_all[w];
  const uint32_t f0 = foff[r], f1 = foff[r + 1];
  const unsigned long long F = static_cast<unsigned long long>(f1 - f0) + (m.wid_eos >= 0 ? 1ull : 0ull);
  const size_t unit_len = static_cast<size_t>(kClsUnitSteps) * lpr;
  for (int col = lane; col < m.dim; col += kWave) {
    float s = 0.0f;
    if (f1 > f0) {
      for (size_t u = f0 / unit_len; u <= (f1 - 1) / unit_len; u++) {
        if (wp_checked(u + r < n_slots, kSiteQuality)) s += partial[(u + r) * m.dim + col];
      }
    }
    if (m.wid_eos >= 0) s += m.input[static_cast<size_t>(m.wid_eos) * m.dim + col];
    S[col] = s;
  }
  __builtin_amdgcn_wave_barrier();
  __threadfence_block();
  const float fF = static_cast<float>(F);
  auto logit = [&](int j) {
    const float *o = m.output + static_cast<size_t>(j) * m.dim;
    float d = 0.0f;
    for (int k = 0; k < m.dim; k++) d = fmaf(o[k], S[k], d);
    return F == 0 ? 0.0f : d / fF;
  };
  float best = 0.0f;
  int32_t at = -1;
  for (int j = lane; j < m.n_labels; j += kWave) {
    const float x = logit(j);
    if (out.logits) out.logits[r * static_cast<size_t>(m.n_labels) + j] = x;
    if (at < 0 || x > best) {
      best = x;
      at = j;
    }
  }
  cls_wave_argmax(best, at);
  float sum = 0.0f;
  for (int j = lane; j < m.n_labels; j += kWave) sum += expf(logit(j) - best);
  sum = cls_wave_sum(sum);
  if (lane != 0) return;
  const bool none = F == 0;
  const float prob = none ? 0.0f : 1.0f / sum;
  const int32_t label = none ? -1 : at;
  uint32_t reasons = none ? 1u : 0u;
  if (!none) {
    if (keep_bits && ((keep_bits[label >> 5] >> (label & 31)) & 1u) == 0) reasons |= 2u;
    if (prob < min_prob) reasons |= 4u;
  }
  out.label[r] = label;
  out.prob[r] = prob;
  out.n_features[r] = static_cast<long long>(F);
  out.reasons[r] = reasons;
  out.keep[r] = reasons == 0 ? 1u : 0u;
  atomicAdd(&counters[0], F);
}

}  // namespace wp
