// quality.h — the kernels of the quality signals (include/wordpiece_amd.h, section "quality signals"; host path:
// quality_path.h).  All work is flat over bytes, words or lines, never over rows.
//   Class pass.  A tile of kQualTile bytes per workgroup, with kQualHalo bytes in front of it and kQualTail positions
// behind it in LDS.  The rows of the first and the last position come from two bisections over all rows; every position
// then finds its row within that range, so the start and the end of its row are the boundaries of its text.  Per
// position: the length of the valid sequence that starts there (inside its row), the class of its code point, and
// whether it starts a character — a valid sequence, or a byte that no valid sequence of the three positions in front of
// it covers.  Then a lane takes kQualItems consecutive positions: the character in front of each lies at most four
// positions back, the one behind it at most four ahead, so word starts, the last characters of words, line starts and
// line ends are decided without looking further.
//   The pass runs twice, as count_starts_kernel does.  First it counts, per tile, the word starts, word ends, line
// starts, line ends, characters and alpha characters, and it sums the per-character signals: a lane sums while its row
// stays the same and adds to LDS slots of the tile's first kQualSlots rows (to memory beyond them); the slots go to the
// signals by 64-bit integer atomics, one per tile, row and signal.  Every combination is an integer sum, so no result
// depends on an order of execution.  After one scan over the six tile counts the second run stores, in text order, the
// start, row and alpha count in front of every word, the end and the alpha count behind it, and the same with the
// character count for every line: the k-th end closes the k-th start.
//   Word pass, one lane per word: a word holds an alpha character iff the two alpha counts differ; a word of at most 32
// bytes is folded (ASCII A-Z) into eight registers and compared with the stop list in LDS.  Line pass, one lane per
// line: its characters are the difference of the two counts; its first non-space character begins the first word that
// starts inside it and its last one ends the last word that ends inside it (two bisections over the word lists).
//   Duplicate lines.  The lines and what lies between them form a ragged batch over the same bytes (qual_lines_kernel
// writes its offsets); the duplicate-row search gives every line the first row with its bytes; (row, that id) is sorted
// once, and every member of a run that is not its head is a duplicate.
#pragma once
#include "class_tables.h"
#include "common.h"
#include "group.h"
#include "overlap.h"  // ovl_row_of
#include "primitives.h"

namespace wp {

constexpr int kQualItems = 8;                    // positions per lane
constexpr int kQualTile = kBlock * kQualItems;   // T: bytes per workgroup of the class pass
constexpr int kQualHalo = 8;                     // positions in front of a tile: the character in front (4) and what may cover it (3)
constexpr int kQualTail = 4;                     // positions behind a tile: the character behind its last one
constexpr int kQualSpan = kQualHalo + kQualTile + kQualTail;
constexpr int kQualSlots = 32;                   // rows of a tile whose sums meet in LDS
constexpr int kQualKinds = 6;                    // the tile counts: word starts, word ends, line starts, line ends, characters, alpha characters
constexpr int kQualStopWords = 9;                // words per entry of the stop table: the length, then 32 bytes
constexpr int kQualMaxStop = 64, kQualMaxStopBytes = 32;
static_assert(kQualHalo >= 7 && kQualTail >= 4, "the neighbours of a character and what may cover them lie inside the span");

// class bits of a position
constexpr uint8_t kQcSpace = 1, kQcSpacing = 2, kQcPunct = 4, kQcAlpha = 8, kQcDigit = 16, kQcUpper = 32, kQcChar = 64, kQcInside = 128;

// the per-character signals a lane sums, and where they go
constexpr int kQualAcc = 14;
enum QualAcc { kQaChars, kQaInvalid, kQaSpace, kQaAlpha, kQaDigit, kQaUpper, kQaPunct, kQaWords, kQaTextWords, kQaTextWordChars, kQaHashes, kQaEllipses,
               kQaNewlines, kQaLines };
__device__ __forceinline__ int qual_acc_signal(int a) { return a < kQaHashes ? a + 1 : a + 3; }
static_assert(WP_QS_CHARS == 1 && WP_QS_TEXT_WORD_CHARS == 10 && WP_QS_HASHES == 13 && WP_QS_LINES == 16, "qual_acc_signal");

// the counters of a call, 64 bits each, in d_scalars from kScalarQual on: rule_failed[16], then the totals
enum QualCounter { kQualRuleFailed = 0, kQualChars = 16, kQualInvalid = 17, kQualWordsTotal = 18, kQualLinesTotal = 19, kQualDupLines = 20, kQualCounters = 24 };

struct QualLimits {
  long long v[WP_QUALITY_RULES];
};

// The rules over the signals of one row: bit r set where rule r is on and the row fails it.  Integer inequalities and
// nothing else: with a zero denominator both sides are 0 and the rule passes.  The host-answered cases and the kernel
// share this function.
__host__ __device__ inline uint32_t quality_reasons(const long long *s, const QualLimits &lim) {
  const long long *L = lim.v;
  uint32_t r = 0;
  auto over = [&](int rule, int num, int den) {
    if (L[rule] >= 0 && s[num] * 1000 > L[rule] * s[den]) r |= 1u << rule;
  };
  auto under = [&](int rule, int num, int den) {
    if (L[rule] >= 0 && s[num] * 1000 < L[rule] * s[den]) r |= 1u << rule;
  };
  if (L[WP_QR_MIN_TEXT_WORDS] >= 0 && s[WP_QS_TEXT_WORDS] < L[WP_QR_MIN_TEXT_WORDS]) r |= 1u << WP_QR_MIN_TEXT_WORDS;
  if (L[WP_QR_MAX_TEXT_WORDS] >= 0 && s[WP_QS_TEXT_WORDS] > L[WP_QR_MAX_TEXT_WORDS]) r |= 1u << WP_QR_MAX_TEXT_WORDS;
  under(WP_QR_MIN_MEAN_WORD_X1000, WP_QS_TEXT_WORD_CHARS, WP_QS_TEXT_WORDS);
  over(WP_QR_MAX_MEAN_WORD_X1000, WP_QS_TEXT_WORD_CHARS, WP_QS_TEXT_WORDS);
  over(WP_QR_MAX_HASH_PER_WORD, WP_QS_HASHES, WP_QS_WORDS);
  over(WP_QR_MAX_ELLIPSIS_PER_WORD, WP_QS_ELLIPSES, WP_QS_WORDS);
  over(WP_QR_MAX_BULLET_LINES, WP_QS_BULLET_LINES, WP_QS_LINES);
  over(WP_QR_MAX_ELLIPSIS_LINES, WP_QS_ELLIPSIS_LINES, WP_QS_LINES);
  under(WP_QR_MIN_ALPHA_WORDS, WP_QS_ALPHA_WORDS, WP_QS_WORDS);
  if (L[WP_QR_MIN_STOP_WORDS] >= 0 && s[WP_QS_STOP_WORDS] < L[WP_QR_MIN_STOP_WORDS]) r |= 1u << WP_QR_MIN_STOP_WORDS;
  over(WP_QR_MAX_DUP_LINES, WP_QS_DUP_LINES, WP_QS_LINES);
  over(WP_QR_MAX_DUP_LINE_CHARS, WP_QS_DUP_LINE_CHARS, WP_QS_CHARS);
  under(WP_QR_MIN_TERMINAL_LINES, WP_QS_TERMINAL_LINES, WP_QS_LINES);
  over(WP_QR_MAX_SHORT_LINES, WP_QS_SHORT_LINES, WP_QS_LINES);
  over(WP_QR_MAX_NEWLINES_PER_WORD, WP_QS_NEWLINES, WP_QS_WORDS);
  return r;
}

// the alpha / digit / upper bits of a code point (class_tables.h), as class bits of a position
__host__ __device__ inline uint8_t quality_class_bits(uint32_t cp, const uint16_t *index, const uint8_t *pages) {
  if (cp >= 0x110000u) return 0;
  return static_cast<uint8_t>(pages[static_cast<size_t>(index[cp >> 8]) * 256 + (cp & 255u)] << 3);
}

struct QualLists {
  // per word: its start, its row, the alpha characters in front of it; its end, the alpha characters in front of its end
  uint32_t *wstart, *wrow, *wa0, *wend, *wa1;
  // per line: the same with the characters
  uint32_t *lstart, *lrow, *lc0, *lend, *lc1;
  size_t n_words, n_lines;
};

// Tile blockIdx.x of the bytes (n_bytes >= 1, n_rows >= 1).  tiles: kQualKinds arrays of nt1 entries.  WRITE false: the
// tile counts and the per-character signals (sig: [WP_QUALITY_SIGNALS][n_rows], cleared).  WRITE true: tiles holds the
// exclusive scan over all kQualKinds * nt1 counts; the lists are stored.
template <bool WRITE>
__global__ __launch_bounds__(kBlock) void qual_class_kernel(const uint8_t *__restrict__ text, size_t n_bytes, const uint32_t *__restrict__ byte_off,
                                                            size_t n_rows, const uint16_t *__restrict__ cls_index, const uint8_t *__restrict__ cls_pages,
                                                            uint32_t *__restrict__ tiles, size_t nt1, unsigned long long *__restrict__ sig, QualLists out) {
  __shared__ uint8_t s_b[kQualSpan + 4];  // the bytes of [origin, origin + kQualSpan + 4)
  __shared__ uint8_t s_cls[kQualSpan];    // class bits of the position
  __shared__ uint8_t s_len[kQualSpan];    // bytes of the valid sequence that starts there, 0: none
  __shared__ uint16_t s_rs[kQualSpan], s_re[kQualSpan];  // start and end of the position's row, relative to origin and clipped to the span
  __shared__ uint32_t s_rows[2];
  __shared__ uint32_t s_scan[8];
  __shared__ uint32_t s_acc[WRITE ? 1 : kQualSlots * kQualAcc];
  const int tid = threadIdx.x;
  const size_t base = static_cast<size_t>(blockIdx.x) * kQualTile;
  const long long origin = static_cast<long long>(base) - kQualHalo;
  for (int k = tid; k < kQualSpan + 4; k += kBlock) {
    const long long p = origin + k;
    s_b[k] = (p >= 0 && static_cast<size_t>(p) < n_bytes) ? text[p] : 0;
  }
  if constexpr (!WRITE) {
    for (int k = tid; k < kQualSlots * kQualAcc; k += kBlock) s_acc[k] = 0;
  }
  if (tid == 0 || tid == kWave) {  // the rows of the first and the last position of the span inside the data
    const size_t e = tid == 0 ? static_cast<size_t>(origin > 0 ? origin : 0) : min(base + kQualTile + kQualTail, n_bytes) - 1;
    s_rows[tid != 0] = ovl_row_of(byte_off, 0, static_cast<uint32_t>(n_rows - 1), e);
  }
  __syncthreads();
  const uint32_t r_lo = s_rows[0], r_hi = s_rows[1];
  // ---- per position: its row, the sequence that starts there, its class ------------------------------------------------
  for (int k = tid; k < kQualSpan; k += kBlock) {
    const long long p = origin + k;
    uint8_t cls = 0, len = 0;
    uint16_t rs_rel = 0, re_rel = 0;
    if (p >= 0 && static_cast<size_t>(p) < n_bytes) {
      const uint32_t r = ovl_row_of(byte_off, r_lo, r_hi, static_cast<size_t>(p));
      const long long rs = byte_off[r], re = byte_off[r + 1];
      if (wp_checked(rs <= p && p < re, kSiteQuality)) {
        rs_rel = static_cast<uint16_t>(max(rs - origin, 0ll));
        re_rel = static_cast<uint16_t>(min(re - origin, static_cast<long long>(kQualSpan + 4)));
        const uint32_t cp = decode_one(s_b + k, re - p);
        cls = kQcInside;
        if (cp != kInvalidUnicode) {
          const uint32_t b0 = s_b[k];
          len = b0 < 0x80u ? 1 : b0 < 0xe0u ? 2 : b0 < 0xf0u ? 3 : 4;
          if (is_space(cp)) cls |= kQcSpace;
          if (is_punctuation(cp)) cls |= kQcPunct;
          if (is_spacing_char(cp)) cls |= kQcSpacing;
          cls |= quality_class_bits(cp, cls_index, cls_pages);
        }
      }
    }
    s_cls[k] = cls;
    s_len[k] = len;
    s_rs[k] = rs_rel;
    s_re[k] = re_rel;
  }
  __syncthreads();
  // ---- a position starts a character unless a valid sequence of its row that starts in front of it covers it ----------
  for (int k = tid; k < kQualSpan; k += kBlock) {
    if (!(s_cls[k] & kQcInside)) continue;
    bool covered = false;
#pragma unroll
    for (int d = 1; d <= 3; d++) covered = covered || (k - d >= static_cast<int>(s_rs[k]) && s_len[k - d] > d);
    if (!covered) s_cls[k] |= kQcChar;
  }
  __syncthreads();
  // ---- a lane's positions --------------------------------------------------------------------------------------------------
  const int k0 = kQualHalo + tid * kQualItems;
  const size_t p0 = base + static_cast<size_t>(tid) * kQualItems;
  uint32_t acc[kQualAcc];
#pragma unroll
  for (int a = 0; a < kQualAcc; a++) acc[a] = 0;
  auto flush = [&](uint32_t row) {
    if constexpr (!WRITE) {
#pragma unroll
      for (int a = 0; a < kQualAcc; a++) {
        if (acc[a] == 0) continue;
        if (row - r_lo < static_cast<uint32_t>(kQualSlots)) {
          atomicAdd(&s_acc[(row - r_lo) * kQualAcc + a], acc[a]);
        } else if (wp_checked(row < n_rows, kSiteQuality)) {
          atomicAdd(&sig[static_cast<size_t>(qual_acc_signal(a)) * n_rows + row], static_cast<unsigned long long>(acc[a]));
        }
        acc[a] = 0;
      }
    }
  };
  uint32_t m_ws = 0, m_we = 0, m_ls = 0, m_le = 0, m_ch = 0, m_al = 0;  // bit j: position k0 + j
  uint32_t rj[kQualItems];
  uint32_t row = 0;
  int re_rel = 0;
  bool have_row = false;
#pragma unroll
  for (int j = 0; j < kQualItems; j++) {
    const int k = k0 + j;
    rj[j] = row;
    const uint8_t c = s_cls[k];
    if (p0 + j >= n_bytes || !(c & kQcInside)) continue;
    if (!have_row || k >= re_rel) {  // another row begins
      if (have_row) flush(row);
      row = ovl_row_of(byte_off, have_row ? min(row + 1, r_hi) : r_lo, r_hi, p0 + j);
      have_row = true;
      re_rel = s_re[k];
    }
    rj[j] = row;
    const uint32_t b = s_b[k];
    const int rs_rel = s_rs[k];
    // lines: maximal runs of bytes other than 0x0A inside the row
    if (b != 0x0a) {
      if (k == rs_rel || s_b[k - 1] == 0x0a) {
        m_ls |= 1u << j;
        acc[kQaLines]++;
      }
      if (k + 1 == re_rel || s_b[k + 1] == 0x0a) m_le |= 1u << j;
    } else {
      acc[kQaNewlines]++;
    }
    if (!(c & kQcChar)) continue;
    m_ch |= 1u << j;
    acc[kQaChars]++;
    const int len = s_len[k];
    if (len == 0) acc[kQaInvalid]++;
    if (c & kQcSpace) acc[kQaSpace]++;
    if (c & kQcAlpha) {
      acc[kQaAlpha]++;
      m_al |= 1u << j;
    }
    if (c & kQcDigit) acc[kQaDigit]++;
    if (c & kQcUpper) acc[kQaUpper]++;
    if (c & kQcPunct) acc[kQaPunct]++;
    if (b == '#') acc[kQaHashes]++;
    if (len == 3 && b == 0xe2u && s_b[k + 1] == 0x80u && s_b[k + 2] == 0xa6u) acc[kQaEllipses]++;  // U+2026
    // the third '.' of a maximal run inside the row counts the run
    if (b == '.' && k - 2 >= rs_rel && s_b[k - 1] == '.' && s_b[k - 2] == '.' && !(k - 3 >= rs_rel && s_b[k - 3] == '.')) acc[kQaEllipses]++;
    if (c & kQcSpace) continue;
    // the character in front, inside the row: at most four positions back
    int pv = -1;
#pragma unroll
    for (int d = 4; d >= 1; d--) {
      if (k - d >= rs_rel && (s_cls[k - d] & kQcChar)) pv = s_cls[k - d];
    }
    const bool start = pv < 0 || (c & kQcSpacing) || (pv & kQcSpacing);
    if (start) {
      m_ws |= 1u << j;
      acc[kQaWords]++;
      if (!(c & kQcPunct)) acc[kQaTextWords]++;
    }
    // (a punctuation character is a word of its own, so the characters of the other words are the non-space ones without it)
    if (!(c & kQcPunct)) acc[kQaTextWordChars]++;
    // the character behind, inside the row: the word ends here where there is none, or a space, or a word start
    const int kn = k + (len ? len : 1);
    bool last = kn >= re_rel;
    if (!last) {
      const uint8_t nc = s_cls[kn];
      last = (nc & kQcSpace) || (nc & kQcSpacing) || (c & kQcSpacing);
    }
    if (last) m_we |= 1u << j;
  }
  if (have_row) flush(row);
  uint32_t tot_w, tot_l, tot_c;
  const uint32_t ex_w = block_excl_sum(__popc(m_ws) | (__popc(m_we) << 16), s_scan, tot_w);
  const uint32_t ex_l = block_excl_sum(__popc(m_ls) | (__popc(m_le) << 16), s_scan, tot_l);
  const uint32_t ex_c = block_excl_sum(__popc(m_ch) | (__popc(m_al) << 16), s_scan, tot_c);
  if constexpr (!WRITE) {
    if (tid == 0) {
      const size_t t = blockIdx.x;
      tiles[0 * nt1 + t] = tot_w & 0xffffu;
      tiles[1 * nt1 + t] = tot_w >> 16;
      tiles[2 * nt1 + t] = tot_l & 0xffffu;
      tiles[3 * nt1 + t] = tot_l >> 16;
      tiles[4 * nt1 + t] = tot_c & 0xffffu;
      tiles[5 * nt1 + t] = tot_c >> 16;
    }
    __syncthreads();  // (the LDS slots are complete)
    for (int i = tid; i < kQualSlots * kQualAcc; i += kBlock) {
      const uint32_t v = s_acc[i];
      const size_t r = static_cast<size_t>(r_lo) + i / kQualAcc;
      if (v != 0 && wp_checked(r < n_rows, kSiteQuality)) {
        atomicAdd(&sig[static_cast<size_t>(qual_acc_signal(i % kQualAcc)) * n_rows + r], static_cast<unsigned long long>(v));
      }
    }
  } else {
    const size_t t = blockIdx.x;
    auto tile_base = [&](int kind) { return tiles[kind * nt1 + t] - tiles[kind * nt1]; };  // (modulo 2^32, as the counts are)
    size_t iw = static_cast<size_t>(tile_base(0)) + (ex_w & 0xffffu), ie = static_cast<size_t>(tile_base(1)) + (ex_w >> 16);
    size_t il = static_cast<size_t>(tile_base(2)) + (ex_l & 0xffffu), ile = static_cast<size_t>(tile_base(3)) + (ex_l >> 16);
    uint32_t ch = tile_base(4) + (ex_c & 0xffffu), al = tile_base(5) + (ex_c >> 16);
#pragma unroll
    for (int j = 0; j < kQualItems; j++) {
      const uint32_t bit = 1u << j, p = static_cast<uint32_t>(p0 + j);
      if (m_ls & bit) {
        if (wp_checked(il < out.n_lines, kSiteQuality)) {
          out.lstart[il] = p;
          out.lrow[il] = rj[j];
          out.lc0[il] = ch;
        }
        il++;
      }
      if (m_ws & bit) {
        if (wp_checked(iw < out.n_words, kSiteQuality)) {
          out.wstart[iw] = p;
          out.wrow[iw] = rj[j];
          out.wa0[iw] = al;
        }
        iw++;
      }
      if (m_ch & bit) ch++;
      if (m_al & bit) al++;
      if (m_we & bit) {
        const int len = s_len[k0 + j];
        if (wp_checked(ie < out.n_words, kSiteQuality)) {
          out.wend[ie] = p + (len ? len : 1);
          out.wa1[ie] = al;
        }
        ie++;
      }
      if (m_le & bit) {
        if (wp_checked(ile < out.n_lines, kSiteQuality)) {
          out.lend[ile] = p + 1;
          out.lc1[ile] = ch;
        }
        ile++;
      }
    }
  }
}

// tiles: the exclusive scan over kQualKinds arrays of nt1 counts, the last of each 0.  *words / *lines = the word and
// line starts of the text; ~0 where the ends are not as many.
__global__ void qual_totals_kernel(const uint32_t *__restrict__ tiles, size_t nt1, uint32_t *__restrict__ words, uint32_t *__restrict__ lines) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  auto total = [&](int kind) { return tiles[kind * nt1 + nt1 - 1] - tiles[kind * nt1]; };
  *words = total(0) == total(1) ? total(0) : 0xffffffffu;
  *lines = total(2) == total(3) ? total(2) : 0xffffffffu;
}

// Word w: ALPHA_WORDS where the alpha counts at its ends differ; STOP_WORDS where its bytes, ASCII A-Z folded, equal an
// entry of the stop table (n_stop entries of kQualStopWords words: the length, then the bytes, zero-padded).
__global__ __launch_bounds__(kBlock) void qual_words_kernel(const uint8_t *__restrict__ text, size_t n_bytes, QualLists in, size_t n_rows,
                                                            const uint32_t *__restrict__ stop, uint32_t n_stop, unsigned long long *__restrict__ sig) {
  __shared__ uint32_t s_stop[kQualMaxStop * kQualStopWords];
  for (uint32_t i = threadIdx.x; i < n_stop * kQualStopWords; i += kBlock) s_stop[i] = stop[i];
  __syncthreads();
  const size_t w = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (w >= in.n_words) return;
  const uint32_t s = in.wstart[w], e = in.wend[w], r = in.wrow[w];
  if (!wp_checked(s < e && e <= n_bytes && r < n_rows, kSiteQuality)) return;
  if (in.wa1[w] != in.wa0[w]) atomicAdd(&sig[static_cast<size_t>(WP_QS_ALPHA_WORDS) * n_rows + r], 1ull);
  const uint32_t len = e - s;
  if (n_stop == 0 || len > kQualMaxStopBytes) return;
  uint32_t x[kQualMaxStopBytes / 4];
#pragma unroll
  for (int i = 0; i < kQualMaxStopBytes / 4; i++) x[i] = 0;
#pragma unroll
  for (uint32_t i = 0; i < kQualMaxStopBytes; i++) {
    if (i < len) {
      uint32_t b = text[s + i];
      if (b >= 'A' && b <= 'Z') b += 32;
      x[i / 4] |= b << (8u * (i % 4));
    }
  }
  bool hit = false;
  for (uint32_t t = 0; t < n_stop && !hit; t++) {
    const uint32_t *q = s_stop + t * kQualStopWords;
    if (q[0] != len || q[1] != x[0]) continue;
    bool same = true;
#pragma unroll
    for (int i = 1; i < kQualMaxStopBytes / 4; i++) same = same && q[1 + i] == x[i];
    hit = same;
  }
  if (hit) atomicAdd(&sig[static_cast<size_t>(WP_QS_STOP_WORDS) * n_rows + r], 1ull);
}

// Line l: SHORT_LINES, BULLET_LINES, ELLIPSIS_LINES, TERMINAL_LINES; lchars[l] = its characters; dup_off (optional): the
// offsets of the batch of 2 * n_lines + 1 rows in which row 2 l + 1 is line l and the rows between hold the line feeds.
__global__ __launch_bounds__(kBlock) void qual_lines_kernel(const uint8_t *__restrict__ text, size_t n_bytes, QualLists in, size_t n_rows,
                                                            uint32_t short_chars, unsigned long long *__restrict__ sig, uint32_t *__restrict__ lchars,
                                                            long long *__restrict__ dup_off) {
  const size_t l = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (l == 0 && dup_off) {
    dup_off[0] = 0;
    dup_off[2 * in.n_lines + 1] = static_cast<long long>(n_bytes);
  }
  if (l >= in.n_lines) return;
  const uint32_t ls = in.lstart[l], le = in.lend[l], r = in.lrow[l];
  const bool sane = wp_checked(ls < le && le <= n_bytes && r < n_rows, kSiteQuality);
  if (dup_off) {  // (a line that fails the check is counted above and fails the call of the bounds-checking build; its entries stay defined)
    dup_off[2 * l + 1] = sane ? ls : 0;
    dup_off[2 * l + 2] = sane ? le : 0;
  }
  if (!sane) {
    lchars[l] = 0;
    return;
  }
  const uint32_t nch = in.lc1[l] - in.lc0[l];
  lchars[l] = nch;
  auto add = [&](int signal) { atomicAdd(&sig[static_cast<size_t>(signal) * n_rows + r], 1ull); };
  if (nch <= short_chars) add(WP_QS_SHORT_LINES);
  const size_t nw = in.n_words;
  if (nw == 0) return;
  // the first word that starts at or behind ls: the first non-space character of the line begins it
  size_t lo = 0, hi = nw;
  while (lo < hi) {
    const size_t mid = (lo + hi) >> 1;
    if (in.wstart[mid] < ls) lo = mid + 1; else hi = mid;
  }
  if (lo >= nw || in.wstart[lo] >= le) return;  // a line of spaces only
  const uint32_t f = in.wstart[lo];
  if (text[f] == '-' || (f + 3 <= le && text[f] == 0xe2u && text[f + 1] == 0x80u && text[f + 2] == 0xa2u)) add(WP_QS_BULLET_LINES);
  // the last word that ends at or in front of le: the last non-space character of the line ends it
  const size_t wl = last_le(in.wend, lo, nw, static_cast<size_t>(le));  // (wend[lo] <= le: the word at lo lies inside the line)
  const uint32_t e = in.wend[wl];
  if (!wp_checked(e > ls && e <= le, kSiteQuality)) return;
  const uint32_t b = text[e - 1];
  if (b == '.' || b == '!' || b == '?' || b == '"' || b == '\'') add(WP_QS_TERMINAL_LINES);
  if (e >= ls + 3) {
    const uint32_t b1 = text[e - 2], b2 = text[e - 3];
    if ((b == 0xa6u && b1 == 0x80u && b2 == 0xe2u) || (b == '.' && b1 == '.' && b2 == '.')) add(WP_QS_ELLIPSIS_LINES);
  }
}

// key[l] = (row of line l, the first row of the line batch with its bytes)
__global__ __launch_bounds__(kBlock) void qual_dup_keys_kernel(const uint32_t *__restrict__ lrow, const int32_t *__restrict__ first, size_t n_lines,
                                                               int id_bits, uint64_t *__restrict__ key) {
  const size_t l = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (l >= n_lines) return;
  key[l] = (static_cast<uint64_t>(lrow[l]) << id_bits) | static_cast<uint32_t>(first[2 * l + 1]);
}

// sorted position s: a member of a run that is not its head is a line whose bytes an earlier line of its row holds
__global__ __launch_bounds__(kBlock) void qual_dup_kernel(const uint32_t *__restrict__ val, const uint32_t *__restrict__ head, size_t n_lines,
                                                          const uint32_t *__restrict__ lrow, const uint32_t *__restrict__ lchars, size_t n_rows,
                                                          unsigned long long *__restrict__ sig) {
  const size_t s = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (s >= n_lines || head[s]) return;
  const uint32_t l = val[s];
  if (!wp_checked(l < n_lines, kSiteQuality)) return;
  const uint32_t r = lrow[l];
  if (!wp_checked(r < n_rows, kSiteQuality)) return;
  atomicAdd(&sig[static_cast<size_t>(WP_QS_DUP_LINES) * n_rows + r], 1ull);
  atomicAdd(&sig[static_cast<size_t>(WP_QS_DUP_LINE_CHARS) * n_rows + r], static_cast<unsigned long long>(lchars[l]));
}

// Row i: BYTES, the rules over its signals, keep[i] = 1 where none failed (keep[n_rows] = 0 closes the flags); the rows
// each rule failed and the totals of the call into the counters.
__global__ __launch_bounds__(kBlock) void qual_rules_kernel(const uint32_t *__restrict__ byte_off, size_t n_rows, QualLimits lim, long long *__restrict__ sig,
                                                            uint32_t *__restrict__ reasons, uint32_t *__restrict__ keep,
                                                            unsigned long long *__restrict__ counters) {
  const size_t i = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  uint32_t r = 0;
  unsigned long long tot[5] = {0, 0, 0, 0, 0};
  if (i < n_rows) {
    long long s[WP_QUALITY_SIGNALS];
    sig[i] = static_cast<long long>(byte_off[i + 1]) - static_cast<long long>(byte_off[i]);
#pragma unroll
    for (int k = 0; k < WP_QUALITY_SIGNALS; k++) s[k] = sig[static_cast<size_t>(k) * n_rows + i];
    r = quality_reasons(s, lim);
    reasons[i] = r;
    keep[i] = r == 0 ? 1u : 0u;
    tot[0] = s[WP_QS_CHARS];
    tot[1] = s[WP_QS_INVALID];
    tot[2] = s[WP_QS_WORDS];
    tot[3] = s[WP_QS_LINES];
    tot[4] = s[WP_QS_DUP_LINES];
  } else if (i == n_rows) {
    keep[i] = 0;
  }
#pragma unroll
  for (int k = 0; k < 5; k++) {
    const unsigned long long t = wave_reduce_sum64(tot[k]);
    if (lane_id() == 0 && t != 0) atomicAdd(&counters[kQualChars + k], t);
  }
  for (int k = 0; k < WP_QUALITY_RULES; k++) {
    const unsigned long long f = __popcll(__ballot((r >> k) & 1u));
    if (lane_id() == 0 && f != 0) atomicAdd(&counters[kQualRuleFailed + k], f);
  }
}

}  // namespace wp
