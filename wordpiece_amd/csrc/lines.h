// lines.h — the kernels of the line filter (include/wordpiece_amd_lines.h; host path: lines_path.h).  The characters, the
// words and the lines are quality.h's: its class pass leaves the word and line lists, and the duplicate-row search of
// dedup.h gives every line the first line with its bytes.  New here:
//   Phrase scan.  A workgroup takes tiles of kQualTile bytes in a grid-stride loop and keeps the filter in LDS for all of
// them: a 65,536-bit map of the two-byte prefixes of the phrases of two bytes or more, a 256-bit map of the one-byte
// phrases, the phrases sorted by (one byte or more, prefix) with their keys, lengths, flags and pool offsets, and the pool
// with every phrase on a word boundary.  A tile is staged folded (A-Z to a-z) with kLfFront bytes in front of it and
// kLfBehind behind it.  A lane tests its kQualItems positions with one bit load each (two where one-byte phrases exist);
// the positions that pass are handed out across the wave through an LDS queue by ballot and prefix count, so a lane with
// five candidates does not hold 63 idle.  A candidate bisects its key to the phrases with that prefix, compares each four
// bytes at a time against the pool's words, finds its row inside the tile's row range, applies the bound rule from the
// two neighbour bytes, finds its line by bisection over the line starts, and ORs the PHRASE bit into the line's reasons
// or adds one to the row's DOC_PHRASE_HITS.  No loop runs over all phrases, over a line or over a row.
//   Line pass, one lane per line: its words from two bisections over the word starts, its characters from the two
// counts, rules 0 to 3 as qual_lines_kernel decides them, the end of what it owns, the offsets of the line batch.
//   Duplicate pass: rule 5 from the first line with the same bytes (scope 2), or from the heads of the sorted (row,
// first) runs (scope 1).  Sum pass: the per-document sums by 64-bit integer atomics per line, and the bytes a dropped
// line owns for the scan D.  Document pass, one lane per row: KEPT_*, the reasons, the keep flag, the statistics.
//   Cut.  No per-byte flag and no per-byte scan: D is the exclusive scan over the LINES of the bytes the dropped ones
// own.  A tile of bytes loads the lines that intersect it into LDS (start, owned end, D), every lane finds the line of
// its first byte there and steps on from it; a kept byte at p goes to p - D.  The bytes are compacted through LDS and
// stored as whole aligned words, the at most two words a tile shares with its neighbours byte by byte.
#pragma once
#include "../../include/wordpiece_amd_lines.h"
#include "quality.h"

namespace wp {

constexpr int kLfFront = 4;                                  // staged bytes in front of a tile: the byte in front of a match, on a word boundary
constexpr int kLfBehind = WP_LF_MAX_PHRASE_BYTES;            // behind it: the 31 bytes of a match that starts on the last position, and the byte behind it
constexpr int kLfSpanWords = (kLfFront + kQualTile + kLfBehind) / 4 + 2;  // (a compare reads one word past its last byte)
constexpr int kLfBitmapWords = 65536 / 32, kLfOneWords = 256 / 32;
constexpr int kLfPoolWords = (WP_LF_MAX_POOL_BYTES + 3 * WP_LF_MAX_PHRASES) / 4;  // every phrase padded to whole words
constexpr int kLfQueue = kWave * kQualItems * 2;             // candidates of a wave and tile: every position, both kinds
// the phrase table as the host lays it out in 32-bit words (lf_phrase_table): the two maps, the entries, the keys, the pool
constexpr int kLfTabOne = kLfBitmapWords, kLfTabMeta = kLfTabOne + kLfOneWords, kLfTabKeys = kLfTabMeta + WP_LF_MAX_PHRASES;
constexpr int kLfTabPool = kLfTabKeys + WP_LF_MAX_PHRASES / 2, kLfTabWords = kLfTabPool + kLfPoolWords;
constexpr int kLfCutTile = kQualTile;                        // bytes per workgroup of the cut
constexpr int kLfCutLines = kLfCutTile + 2;                  // the lines that can intersect a tile (starts are distinct), and the entry in front of them
static_assert((kLfFront + kQualTile + kLfBehind) % 4 == 0 && kLfFront % 4 == 0, "the staged span is whole words and the tile begins on one");

// the counters of a call, 64 bits each, in d_scalars from kScalarLf on
enum LfCounter { kLfRuleFailed = 0, kLfLineFailed = 4, kLfLinesTotal = 10, kLfKeptLines = 11, kLfKeptBytes = 12, kLfMatches = 13, kLfCounters = 16 };

struct LfLimits {
  long long line[4], doc[WP_LF_DOC_RULES];
};

// The document rules over the signals of one row; the host-answered batch and lf_docs_kernel share this function.
__host__ __device__ inline uint32_t lines_reasons(const long long *s, const LfLimits &lim) {
  const long long *L = lim.doc;
  uint32_t r = 0;
  if (L[WP_LD_MIN_KEPT_LINES] >= 0 && s[WP_LF_KEPT_LINES] < L[WP_LD_MIN_KEPT_LINES]) r |= 1u << WP_LD_MIN_KEPT_LINES;
  if (L[WP_LD_MIN_KEPT_WORDS] >= 0 && s[WP_LF_KEPT_WORDS] < L[WP_LD_MIN_KEPT_WORDS]) r |= 1u << WP_LD_MIN_KEPT_WORDS;
  if (L[WP_LD_MAX_DROPPED_X1000] >= 0 && (s[WP_LF_LINE_CHARS] - s[WP_LF_KEPT_CHARS]) * 1000 > L[WP_LD_MAX_DROPPED_X1000] * s[WP_LF_LINE_CHARS]) {
    r |= 1u << WP_LD_MAX_DROPPED_X1000;
  }
  if (L[WP_LD_MAX_DOC_PHRASE_HITS] >= 0 && s[WP_LF_DOC_PHRASE_HITS] > L[WP_LD_MAX_DOC_PHRASE_HITS]) r |= 1u << WP_LD_MAX_DOC_PHRASE_HITS;
  return r;
}

// the four bytes of a word, A-Z folded to a-z
__device__ __forceinline__ uint32_t lf_fold4(uint32_t x) {
  uint32_t y = 0;
#pragma unroll
  for (int b = 0; b < 4; b++) {
    uint32_t c = (x >> (8 * b)) & 0xffu;
    if (c - 'A' < 26u) c += 32u;
    y |= c << (8 * b);
  }
  return y;
}
// whether a (folded) byte next to a match leaves it bounded: ASCII and neither a digit nor a letter
__device__ __forceinline__ bool lf_boundary(uint32_t b) { return b < 0x80u && !(b - '0' < 10u) && !(b - 'a' < 26u) && !(b - 'A' < 26u); }

// table: kLfTabWords words as lf_phrase_table lays them out, of which the first n_one entries are the one-byte phrases;
// pool_words: the words of the padded pool.  lines: the line list (lstart, lend) with n_lines >= 0; line_reasons cleared;
// sig: [WP_LF_SIGNALS][n_rows], cleared.  matches: the counter of the (position, phrase) matches.
__global__ __launch_bounds__(kBlock) void lf_phrase_kernel(const uint32_t *__restrict__ d32, size_t n_bytes, const uint32_t *__restrict__ byte_off, size_t n_rows,
                                                           const uint32_t *__restrict__ table, uint32_t n_one, uint32_t n_phrases, uint32_t pool_words,
                                                           QualLists lines, uint32_t *__restrict__ line_reasons, unsigned long long *__restrict__ sig,
                                                           unsigned long long *__restrict__ matches) {
  __shared__ uint32_t s_bm[kLfBitmapWords];
  __shared__ uint32_t s_one[kLfOneWords];
  __shared__ uint32_t s_meta[WP_LF_MAX_PHRASES];  // pool offset in words | length << 16 | flags << 24
  __shared__ uint16_t s_key[WP_LF_MAX_PHRASES];   // the first byte (one-byte phrases), the first two (the others), ascending in each part
  __shared__ uint32_t s_pool[kLfPoolWords];
  __shared__ uint32_t s_txt[kLfSpanWords];        // the folded bytes of [base - kLfFront, ...)
  __shared__ uint16_t s_q[kBlock / kWave][kLfQueue];
  __shared__ uint32_t s_rows[2];
  const int tid = threadIdx.x, lane = lane_id(), w = wave_id();
  for (int i = tid; i < kLfBitmapWords; i += kBlock) s_bm[i] = table[i];
  if (tid < kLfOneWords) s_one[tid] = table[kLfTabOne + tid];
  for (uint32_t i = tid; i < n_phrases; i += kBlock) {
    s_meta[i] = table[kLfTabMeta + i];
    s_key[i] = static_cast<uint16_t>(table[kLfTabKeys + (i >> 1)] >> (16u * (i & 1u)));
  }
  for (uint32_t i = tid; i < pool_words && i < static_cast<uint32_t>(kLfPoolWords); i += kBlock) s_pool[i] = table[kLfTabPool + i];
  const uint8_t *sb = reinterpret_cast<const uint8_t *>(s_txt);
  const size_t n_tiles = (n_bytes + kQualTile - 1) / kQualTile;
  unsigned long long found = 0;
  for (size_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const size_t base = t * kQualTile, end = min(base + kQualTile, n_bytes);
    __syncthreads();  // (the tables are loaded; the last tile's candidates are done with s_txt and s_rows)
    for (int i = tid; i < kLfSpanWords; i += kBlock) {
      const long long p = static_cast<long long>(base) - kLfFront + 4ll * i;  // (whole aligned words that begin inside the data)
      s_txt[i] = (p >= 0 && static_cast<size_t>(p) < n_bytes) ? lf_fold4(d32[p >> 2]) : 0u;
    }
    if (tid == 0 || tid == kWave) s_rows[tid != 0] = ovl_row_of(byte_off, 0, static_cast<uint32_t>(n_rows - 1), tid == 0 ? base : end - 1);
    __syncthreads();
    const uint32_t r_lo = s_rows[0], r_hi = s_rows[1];
    // ---- a lane's positions: bit j of m2 / m1 where a phrase of two bytes or more / of one byte may begin ---------------
    const int k0 = kLfFront + tid * kQualItems;
    const size_t p0 = base + static_cast<size_t>(tid) * kQualItems;
    const uint32_t x0 = s_txt[k0 >> 2], x1 = s_txt[(k0 >> 2) + 1], x2 = s_txt[(k0 >> 2) + 2];
    uint32_t m2 = 0, m1 = 0;
#pragma unroll
    for (int j = 0; j < kQualItems; j++) {
      const uint32_t lo = j < 4 ? x0 : x1, hi = j < 3 ? x0 : j < 7 ? x1 : x2;
      const uint32_t b0 = (lo >> (8 * (j & 3))) & 0xffu, b1 = (hi >> (8 * ((j + 1) & 3))) & 0xffu;
      if (p0 + j >= end) continue;
      const uint32_t key = b0 | (b1 << 8);
      m2 |= ((s_bm[key >> 5] >> (key & 31u)) & 1u) << j;
      if (n_one != 0) m1 |= ((s_one[b0 >> 5] >> (b0 & 31u)) & 1u) << j;
    }
    // ---- the candidates of the wave into its queue, in any order: bit 15 set for the one-byte kind ------------------------
    uint32_t n_q = 0;
    if (__ballot(m2 | m1) != 0ull) {
#pragma unroll
      for (int j = 0; j < 2 * kQualItems; j++) {
        const bool c = ((j < kQualItems ? m2 : m1) >> (j & (kQualItems - 1))) & 1u;
        const unsigned long long b = __ballot(c);
        if (c) s_q[w][n_q + __popcll(b & ((1ull << lane) - 1ull))] = static_cast<uint16_t>((k0 + (j & (kQualItems - 1))) | (j < kQualItems ? 0 : 0x8000));
        n_q += __popcll(b);
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();  // (a wave reads only what it wrote itself: no workgroup barrier; n_q <= kLfQueue by construction)
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    for (uint32_t q = lane; q < n_q; q += kWave) {
      const uint32_t e = s_q[w][q];
      const int k = e & 0x7fff;
      const bool one = (e & 0x8000u) != 0;
      const size_t p = base + static_cast<size_t>(k - kLfFront);
      const uint32_t key = one ? sb[k] : sb[k] | (static_cast<uint32_t>(sb[k + 1]) << 8);
      // the first phrase of its part with that key
      uint32_t lo = one ? 0u : n_one, hi = one ? n_one : n_phrases;
      const uint32_t part_end = hi;
      while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (s_key[mid] < key) lo = mid + 1; else hi = mid;
      }
      if (lo >= part_end || s_key[lo] != key) continue;
      const uint32_t r = ovl_row_of(byte_off, r_lo, r_hi, p);
      const size_t rs = byte_off[r], re = byte_off[r + 1];
      if (!wp_checked(rs <= p && p < re && re <= n_bytes, kSiteQuality)) continue;
      const uint32_t sh = static_cast<uint32_t>(k & 3) * 8u;
      uint32_t line_hits = 0, doc_hits = 0;
      for (uint32_t t2 = lo; t2 < part_end && s_key[t2] == key; t2++) {
        const uint32_t meta = s_meta[t2], off = meta & 0xffffu, len = (meta >> 16) & 0xffu, flags = meta >> 24;
        if (p + len > re || !wp_checked(off + ((len + 3u) >> 2) <= static_cast<uint32_t>(kLfPoolWords) && len <= kLfBehind, kSiteQuality)) continue;
        bool same = true;
        for (uint32_t i = 0; 4u * i < len && same; i++) {
          const uint32_t a = s_txt[(k >> 2) + i], b = s_txt[(k >> 2) + i + 1];
          uint32_t x = sh ? (a >> sh) | (b << (32u - sh)) : a;
          const uint32_t rem = len - 4u * i;
          if (rem < 4u) x &= (1u << (8u * rem)) - 1u;
          same = x == s_pool[off + i];
        }
        if (!same) continue;
        if (flags & WP_LF_PHRASE_BOUNDED) {
          if (p > rs && !lf_boundary(sb[k - 1])) continue;
          if (p + len < re && !lf_boundary(sb[k + len])) continue;
        }
        if (flags & WP_LF_PHRASE_DOC) doc_hits++; else line_hits++;
      }
      if (doc_hits) atomicAdd(&sig[static_cast<size_t>(WP_LF_DOC_PHRASE_HITS) * n_rows + r], static_cast<unsigned long long>(doc_hits));
      if (line_hits && wp_checked(lines.n_lines != 0 && lines.lstart[0] <= p, kSiteQuality)) {
        const size_t l = last_le(lines.lstart, size_t(0), lines.n_lines, p);
        if (wp_checked(p < lines.lend[l], kSiteQuality)) atomicOr(&line_reasons[l], 1u << WP_LR_PHRASE);
      }
      found += doc_hits + line_hits;
    }
  }
  found = wave_reduce_sum64(found);
  if (lane == 0 && found != 0) atomicAdd(matches, found);
}

// what the line pass leaves per line for the passes behind it
struct LfLines {
  uint32_t *words, *chars, *own_end;  // its words, its characters, the end of what it owns
  uint32_t *reasons;                  // line_reasons: the PHRASE bit is in; rules 0 to 3 are ORed in here
};

// Line l: rules 0 to 3, its words and characters, the end of the bytes it owns; dup_off (optional): the offsets of the
// batch of 2 * n_lines + 1 rows in which row 2 l + 1 is line l (quality.h, qual_lines_kernel).
__global__ __launch_bounds__(kBlock) void lf_lines_kernel(const uint8_t *__restrict__ text, size_t n_bytes, const uint32_t *__restrict__ byte_off, QualLists in,
                                                          size_t n_rows, LfLimits lim, LfLines out, long long *__restrict__ dup_off) {
  const size_t l = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (l == 0 && dup_off) {
    dup_off[0] = 0;
    dup_off[2 * in.n_lines + 1] = static_cast<long long>(n_bytes);
  }
  if (l >= in.n_lines) return;
  const uint32_t ls = in.lstart[l], le = in.lend[l], r = in.lrow[l];
  const bool sane = wp_checked(ls < le && le <= n_bytes && r < n_rows, kSiteQuality);
  if (dup_off) {  // (a line that fails the check fails the call of the bounds-checking build; its entries stay defined)
    dup_off[2 * l + 1] = sane ? ls : 0;
    dup_off[2 * l + 2] = sane ? le : 0;
  }
  out.words[l] = 0;
  out.chars[l] = 0;
  out.own_end[l] = sane ? le : ls;
  if (!sane) return;
  const uint32_t row_end = byte_off[r + 1];
  const bool next_here = l + 1 < in.n_lines && in.lrow[l + 1] == r;
  const uint32_t own = next_here ? in.lstart[l + 1] : row_end;
  out.own_end[l] = wp_checked(own >= le && own <= n_bytes, kSiteQuality) ? own : le;
  const uint32_t nch = in.lc1[l] - in.lc0[l];
  out.chars[l] = nch;
  // the words that start in [ls, le): two bisections over the word starts
  const size_t nw = in.n_words;
  auto first_at = [&](uint32_t x) {
    size_t lo = 0, hi = nw;
    while (lo < hi) {
      const size_t mid = (lo + hi) >> 1;
      if (in.wstart[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
  };
  const size_t wa = first_at(ls), wb = first_at(le);
  const uint32_t words = static_cast<uint32_t>(wb - wa);
  out.words[l] = words;
  uint32_t bits = 0;
  if (lim.line[WP_LR_MIN_WORDS] >= 0 && static_cast<long long>(words) < lim.line[WP_LR_MIN_WORDS]) bits |= 1u << WP_LR_MIN_WORDS;
  if (lim.line[WP_LR_MIN_CHARS] >= 0 && static_cast<long long>(nch) < lim.line[WP_LR_MIN_CHARS]) bits |= 1u << WP_LR_MIN_CHARS;
  bool terminal = false, ellipsis = false;
  if (words != 0) {
    // the last word that ends at or in front of le: the last non-space character of the line ends it
    const size_t wl = last_le(in.wend, wa, nw, static_cast<size_t>(le));  // (wend[wa] <= le: the word at wa lies inside the line)
    const uint32_t e = in.wend[wl];
    if (wp_checked(e > ls && e <= le, kSiteQuality)) {
      const uint32_t b = text[e - 1];
      terminal = b == '.' || b == '!' || b == '?' || b == '"' || b == '\'';
      if (e >= ls + 3) {
        const uint32_t b1 = text[e - 2], b2 = text[e - 3];
        ellipsis = (b == 0xa6u && b1 == 0x80u && b2 == 0xe2u) || (b == '.' && b1 == '.' && b2 == '.');
      }
    }
  }
  if (lim.line[WP_LR_NOT_TERMINAL] >= 0 && !terminal) bits |= 1u << WP_LR_NOT_TERMINAL;
  if (lim.line[WP_LR_ELLIPSIS_END] >= 0 && ellipsis) bits |= 1u << WP_LR_ELLIPSIS_END;
  if (bits) out.reasons[l] |= bits;  // (the phrase scan is done: this lane alone touches the word)
}

// Rule 5.  scope 2, lane l: the line fails where the first row of the line batch with its bytes is not its own.  scope 1,
// lane s of the lines sorted by (row, first): a member of a run that is not its head fails (val: the line at s).
__global__ __launch_bounds__(kBlock) void lf_dup_kernel(const int32_t *__restrict__ first, const uint32_t *__restrict__ val, const uint32_t *__restrict__ head,
                                                        size_t n_lines, const uint32_t *__restrict__ chars, uint32_t min_chars, uint32_t *__restrict__ reasons) {
  const size_t s = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (s >= n_lines) return;
  size_t l = s;
  bool dup;
  if (val) {
    l = val[s];
    if (!wp_checked(l < n_lines, kSiteQuality)) return;
    dup = !head[s];
  } else {
    dup = first[2 * l + 1] != static_cast<int32_t>(2 * l + 1);
  }
  if (dup && chars[l] >= min_chars) reasons[l] |= 1u << WP_LR_DUPLICATE;  // (one lane per line)
}

// Line l, its reasons final: the sums of its row by 64-bit integer atomics (KEPT_BYTES holds the dropped bytes until
// lf_docs_kernel turns it), drop[l] = the bytes it owns where it is dropped (drop[n_lines] = 0 closes the array), and
// with WP_LF_WANT_LINES its row, start and length.
__global__ __launch_bounds__(kBlock) void lf_sums_kernel(QualLists in, LfLines ln, size_t n_rows, unsigned long long *__restrict__ sig, uint32_t *__restrict__ drop,
                                                         int32_t *__restrict__ line_row, long long *__restrict__ line_start, int32_t *__restrict__ line_len) {
  const size_t l = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (l == in.n_lines) drop[l] = 0;
  if (l >= in.n_lines) return;
  const uint32_t ls = in.lstart[l], r = in.lrow[l], bits = ln.reasons[l];
  const uint32_t own = ln.own_end[l] - ls;
  drop[l] = bits ? own : 0u;
  if (line_row) {
    line_row[l] = static_cast<int32_t>(r);
    line_start[l] = ls;
    line_len[l] = static_cast<int32_t>(in.lend[l] - ls);
  }
  if (!wp_checked(r < n_rows, kSiteQuality)) return;
  auto add = [&](int signal, unsigned long long x) {
    if (x) atomicAdd(&sig[static_cast<size_t>(signal) * n_rows + r], x);
  };
  add(WP_LF_LINES, 1);
  add(WP_LF_LINE_CHARS, ln.chars[l]);
  add(WP_LF_WORDS, ln.words[l]);
  if (bits == 0) {
    add(WP_LF_KEPT_LINES, 1);
    add(WP_LF_KEPT_CHARS, ln.chars[l]);
    add(WP_LF_KEPT_WORDS, ln.words[l]);
  } else {
    add(WP_LF_KEPT_BYTES, own);
#pragma unroll
    for (int k = 0; k < WP_LF_LINE_RULES; k++) add(WP_LF_FAILED_0 + k, (bits >> k) & 1u);
  }
}

// Row i: BYTES, KEPT_BYTES, the document rules, keep[i] = 1 where none failed (keep[n_rows] = 0 closes the flags); the rows
// each rule failed and the totals of the call into the counters.
__global__ __launch_bounds__(kBlock) void lf_docs_kernel(const uint32_t *__restrict__ byte_off, size_t n_rows, LfLimits lim, long long *__restrict__ sig,
                                                         uint32_t *__restrict__ reasons, uint32_t *__restrict__ keep, unsigned long long *__restrict__ counters) {
  const size_t i = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  uint32_t r = 0;
  unsigned long long tot[3 + WP_LF_LINE_RULES] = {};
  if (i < n_rows) {
    long long s[WP_LF_SIGNALS];
#pragma unroll
    for (int k = 0; k < WP_LF_SIGNALS; k++) s[k] = sig[static_cast<size_t>(k) * n_rows + i];
    s[WP_LF_BYTES] = static_cast<long long>(byte_off[i + 1]) - static_cast<long long>(byte_off[i]);
    s[WP_LF_KEPT_BYTES] = s[WP_LF_BYTES] - s[WP_LF_KEPT_BYTES];
    sig[static_cast<size_t>(WP_LF_BYTES) * n_rows + i] = s[WP_LF_BYTES];
    sig[static_cast<size_t>(WP_LF_KEPT_BYTES) * n_rows + i] = s[WP_LF_KEPT_BYTES];
    r = lines_reasons(s, lim);
    reasons[i] = r;
    keep[i] = r == 0 ? 1u : 0u;
    tot[0] = s[WP_LF_LINES];
    tot[1] = s[WP_LF_KEPT_LINES];
    tot[2] = s[WP_LF_KEPT_BYTES];
#pragma unroll
    for (int k = 0; k < WP_LF_LINE_RULES; k++) tot[3 + k] = s[WP_LF_FAILED_0 + k];
  } else if (i == n_rows) {
    keep[i] = 0;
  }
#pragma unroll
  for (int k = 0; k < 3 + WP_LF_LINE_RULES; k++) {
    const unsigned long long t = wave_reduce_sum64(tot[k]);
    if (lane_id() == 0 && t != 0) atomicAdd(&counters[k < 3 ? kLfLinesTotal + k : kLfLineFailed + k - 3], t);
  }
  for (int k = 0; k < WP_LF_DOC_RULES; k++) {
    const unsigned long long f = __popcll(__ballot((r >> k) & 1u));
    if (lane_id() == 0 && f != 0) atomicAdd(&counters[kLfRuleFailed + k], f);
  }
}

// Row i of the cut (D: the exclusive scan of drop over n_lines + 1 entries): cut_off[i] and cut_boff[i] = the row's start
// minus the D of its first line, which is the first line at or behind its start; entry n_rows closes both.
__global__ __launch_bounds__(kBlock) void lf_cut_off_kernel(const uint32_t *__restrict__ Dv, const uint32_t *__restrict__ lstart, size_t n_lines,
                                                            const uint32_t *__restrict__ byte_off, size_t n_rows, long long *__restrict__ cut_off,
                                                            uint32_t *__restrict__ cut_boff) {
  const size_t i = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (i > n_rows) return;
  const uint32_t a = byte_off[i];
  size_t lo = 0, hi = n_lines;
  while (lo < hi) {
    const size_t mid = (lo + hi) >> 1;
    if (lstart[mid] < a) lo = mid + 1; else hi = mid;
  }
  const uint32_t d = Dv[lo];
  const uint32_t at = wp_checked(d <= a, kSiteQuality) ? a - d : 0u;
  cut_off[i] = at;
  cut_boff[i] = at;
}

// The cut, tile blockIdx.x of kLfCutTile bytes.  LDS entry 0 stands in front of the lines (it owns nothing), entries 1 ..
// m are the lines that begin below the tile's end from the last one that begins at or below its start on; s_D[j] is the
// D of entry j and s_D[m + 1] closes it.  The bytes dropped in front of x: inside a dropped line's own bytes its D plus
// x's distance from its start, else the D of the next line.  The kept bytes of the tile are [o0, o1) of the output; they
// meet in LDS at (output position - the word boundary at or below o0) and leave as rep_cut_bytes_kernel stores them.
__global__ __launch_bounds__(kBlock) void lf_cut_kernel(const uint32_t *__restrict__ d32, size_t n_bytes, const uint32_t *__restrict__ lstart,
                                                        const uint32_t *__restrict__ own_end, const uint32_t *__restrict__ Dv, size_t n_lines,
                                                        uint32_t *__restrict__ out) {
  __shared__ uint32_t s_start[kLfCutLines], s_own[kLfCutLines], s_D[kLfCutLines + 1];
  __shared__ uint32_t s_out[kLfCutTile / 4 + 2];
  __shared__ uint32_t s_range[2];
  uint8_t *sb = reinterpret_cast<uint8_t *>(s_out);
  const int tid = threadIdx.x;
  const size_t base = static_cast<size_t>(blockIdx.x) * kLfCutTile;
  const size_t end = min(base + kLfCutTile, n_bytes);
  if (tid == 0) {
    size_t la = 0, lo = 0, hi = n_lines;
    if (n_lines != 0 && lstart[0] <= base) la = last_le(lstart, size_t(0), n_lines, base);
    while (lo < hi) {  // the lines that begin below end
      const size_t mid = (lo + hi) >> 1;
      if (lstart[mid] < end) lo = mid + 1; else hi = mid;
    }
    s_range[0] = static_cast<uint32_t>(la);
    s_range[1] = static_cast<uint32_t>(lo > la ? lo - la : 0);
  }
  __syncthreads();
  const size_t la = s_range[0];
  const uint32_t m = s_range[1];
  if (!wp_checked(m + 1 < static_cast<uint32_t>(kLfCutLines) && la + m <= n_lines, kSiteQuality)) return;  // (the whole workgroup leaves together)
  for (uint32_t j = tid; j <= m + 1; j += kBlock) {
    s_D[j] = Dv[la + (j ? j - 1 : 0)];
    if (j <= m) {
      s_start[j] = j ? lstart[la + j - 1] : 0u;
      s_own[j] = j ? own_end[la + j - 1] : 0u;
    }
  }
  __syncthreads();
  auto entry_of = [&](size_t x) { return last_le(s_start, 0u, m + 1u, x); };
  auto dropped_before = [&](uint32_t j, size_t x) {
    return x < s_own[j] && s_D[j + 1] != s_D[j] ? static_cast<size_t>(s_D[j]) + (x - s_start[j]) : static_cast<size_t>(s_D[j + 1]);
  };
  const size_t c0 = dropped_before(entry_of(base), base), c1 = dropped_before(entry_of(end), end);
  const bool sane = c0 <= base && c1 <= end && c0 <= c1 && c1 - c0 <= end - base;
  if (!wp_checked(sane, kSiteQuality)) return;
  const size_t o0 = base - c0, o1 = end - c1, w0 = o0 & ~static_cast<size_t>(3);
  const size_t q0 = base + static_cast<size_t>(tid) * kQualItems;
  if (q0 < end) {
    uint32_t j = entry_of(q0);
    size_t o = q0 - dropped_before(j, q0);
    const uint32_t x0 = d32[q0 >> 2], x1 = q0 + 4 < end ? d32[(q0 >> 2) + 1] : 0u;
#pragma unroll
    for (int b = 0; b < kQualItems; b++) {
      const size_t p = q0 + b;
      if (p >= end) break;
      if (j < m && s_start[j + 1] <= p) j++;  // (lines hold a byte each: one step a byte is enough)
      if (p < s_own[j] && s_D[j + 1] != s_D[j]) continue;
      const size_t at = o - w0;
      if (wp_checked(o >= o0 && at < kLfCutTile + 4, kSiteQuality)) sb[at] = static_cast<uint8_t>((b < 4 ? x0 : x1) >> (8u * (b & 3)));
      o++;
    }
  }
  __syncthreads();
  uint8_t *out8 = reinterpret_cast<uint8_t *>(out);
  const size_t words = (o1 - w0 + 3) >> 2;
  for (size_t jw = tid; jw < words; jw += kBlock) {
    const size_t at = w0 + 4 * jw;
    if (at >= o0 && at + 4 <= o1) {
      out[at >> 2] = s_out[jw];
    } else {
      for (uint32_t b = 0; b < 4; b++) {
        if (at + b >= o0 && at + b < o1) out8[at + b] = sb[4 * jw + b];
      }
    }
  }
}

}  // namespace wp
