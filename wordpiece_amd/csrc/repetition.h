// repetition.h — the kernels of the repetition signals (include/wordpiece_amd_repetition.h; host path: repetition_path.h).
// One lexicographic order of the word positions of every row answers all nine window lengths; nothing here hashes.
//   Words.  The word list is quality.h's, with the characters in front of every word's start and end beside it.  Every
// word gets the index of the first word of the batch with its bytes from the duplicate-row search over the words as a
// ragged batch (rpt_word_rows_kernel writes its offsets: row 2 w + 1 is word w, the rows between hold what separates them).
//   Ranks.  r1[p] is the rank of (row, word id) among all positions: equal iff the same word in the same row.  A round
// with step h sorts the key (r[p], r[p + h] + 1, or 0 where p + h lies behind the row) stably and gives every position
// the run of its key as the rank of its 2h words.  h = 1, 2, 4 give r2, r4, r8; the last sort pairs r8[p] with r2[p + 8].
// Behind it the positions stand in the lexicographic order of their 10-word windows, a window that the row end cuts
// sorting in front of its extensions.  Every key is two exact ranks, so the order needs no verification.
//   LCP.  Slot s compares its window with its predecessor's word by word through r1, at most 10 words and only while the
// later of the two stays inside its row (the earlier one then does too, and r1 tells rows apart).
//   Runs.  For a length n a run is a maximal stretch of slots with LCP >= n: the occurrences of one n-gram.  Three
// lengths go through one set of kernels at a time.  n = 2..4: a run's occurrences are the distance between two heads;
// its head folds (occurrences, characters) into one 64-bit word per (row, n) by atomicMax.  n = 5..10: every member of a
// run of two or more folds its position into the run's slot by atomicMin, and whoever is not that minimum sets the bit of
// n in its word's flag byte of the pass (one byte array per pass, stored whole): an equal n-gram begins in front of it.
//   Cover.  A tile of kBlock words with the kRptHalo words in front of it in LDS, flag bytes and rows: word j is covered
// for n iff bit n - 5 is set at some word of its row in [j - n + 1, j].  The per-row sums (words, characters, covered
// characters per n) meet in LDS slots of the tile's first kRptSlots rows and go to the signals by 64-bit atomics.
// Integer sums, maxima and minima only: no result depends on an order of execution.
#pragma once
#include "../../include/wordpiece_amd_repetition.h"
#include "common.h"
#include "group.h"
#include "primitives.h"
#include "quality.h"

namespace wp {

constexpr int kRptMaxN = 10;             // the longest window
constexpr int kRptHalo = kRptMaxN - 1;   // words in front of a tile of the cover kernel
constexpr int kRptSlots = 32;            // rows of a tile whose sums meet in LDS
constexpr int kRptAcc = 8;               // WORDS, WORD_CHARS, DUP_5_CHARS .. DUP_10_CHARS
constexpr int kRptGroup = 3;             // window lengths a run pass works at a time
static_assert(WP_RPT_DUP_5_CHARS + 5 == WP_RPT_DUP_10_CHARS && WP_RPT_SIGNALS == WP_RPT_DUP_10_CHARS + 1, "the covered characters close the signals");
static_assert(WP_RPT_TOP_2_COUNT == 2 && WP_RPT_TOP_4_CHARS == 7, "rpt_rules_kernel");

// the counters of a call, 64 bits each, in d_scalars from kScalarRpt on
enum RptCounter { kRptRuleFailed = 0, kRptWordsTotal = WP_RPT_RULES, kRptWordChars, kRptCounters = 12 };

struct RptLimits {
  long long v[WP_RPT_RULES];
};

// the arrays of the kRptGroup window lengths of a run pass: the head flags, their exclusive scan, and per run either the
// slot of its head (n = 2..4) or its smallest position (n = 5..10)
struct RptRuns {
  uint32_t *head[kRptGroup], *run[kRptGroup], *aux[kRptGroup];
};

// The rules over the signals of one row: bit k set where rule k is on and the row fails it; with a zero denominator both
// sides are 0 and the rule passes.  The host-answered cases and the kernel share this function.
__host__ __device__ inline uint32_t repetition_reasons(const long long *s, const RptLimits &lim) {
  uint32_t r = 0;
  for (int k = 0; k < WP_RPT_RULES; k++) {
    const int x = k < 3 ? WP_RPT_TOP_2_CHARS + 2 * k : WP_RPT_DUP_5_CHARS + (k - 3);
    if (lim.v[k] >= 0 && s[x] * 1000 > lim.v[k] * s[WP_RPT_WORD_CHARS]) r |= 1u << k;
  }
  return r;
}

// Word w: its characters, and rows 2 w + 1 (the word) and 2 w + 2 (what follows it) of the batch the duplicate-row
// search runs over.  A word that fails the check is counted and stays defined (an empty row).
__global__ __launch_bounds__(kBlock) void rpt_word_rows_kernel(QualLists in, size_t n_bytes, uint32_t *__restrict__ wchars, long long *__restrict__ dup_off) {
  const size_t w = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (w == 0) {
    dup_off[0] = 0;
    dup_off[2 * in.n_words + 1] = static_cast<long long>(n_bytes);
  }
  if (w >= in.n_words) return;
  const uint32_t s = in.wstart[w], e = in.wend[w];
  const bool sane = wp_checked(s < e && e <= n_bytes, kSiteQuality);
  dup_off[2 * w + 1] = sane ? s : 0;
  dup_off[2 * w + 2] = sane ? e : 0;
  wchars[w] = sane ? in.wc1[w] - in.wc0[w] : 0u;
}

// key[w] = (row of word w, the first row of the word batch with its bytes)
__global__ __launch_bounds__(kBlock) void rpt_word_keys_kernel(const uint32_t *__restrict__ wrow, const int32_t *__restrict__ first, size_t n_words, int id_bits,
                                                               uint64_t *__restrict__ key) {
  const size_t w = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (w >= n_words) return;
  key[w] = (static_cast<uint64_t>(wrow[w]) << id_bits) | static_cast<uint32_t>(first[2 * w + 1]);
}

// key[p] = (ra[p], rb[p + h] + 1 where p + h lies in the row of p, else 0); every rank is below 2^bits - 1
__global__ __launch_bounds__(kBlock) void rpt_pair_keys_kernel(const uint32_t *__restrict__ ra, const uint32_t *__restrict__ rb, const uint32_t *__restrict__ wrow,
                                                               size_t n_words, uint32_t h, int bits, uint64_t *__restrict__ key) {
  const size_t p = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (p >= n_words) return;
  const size_t q = p + h;
  const uint32_t second = q < n_words && wrow[q] == wrow[p] ? rb[q] + 1u : 0u;
  key[p] = (static_cast<uint64_t>(ra[p]) << bits) | second;
}

// rank[val[s]] = the run of sorted slot s (run: the exclusive scan of head): equal keys, equal ranks, in key order
__global__ __launch_bounds__(kBlock) void rpt_rank_kernel(const uint32_t *__restrict__ val, const uint32_t *__restrict__ head, const uint32_t *__restrict__ run,
                                                          size_t n_words, uint32_t *__restrict__ rank) {
  const size_t s = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (s >= n_words) return;
  const uint32_t p = val[s];
  if (wp_checked(p < n_words, kSiteQuality)) rank[p] = run_of(head, run, s);
}

// lcp[s] = the equal leading words of the windows at slots s - 1 and s, at most kRptMaxN and only inside the row
__global__ __launch_bounds__(kBlock) void rpt_lcp_kernel(const uint32_t *__restrict__ val, const uint32_t *__restrict__ r1, const uint32_t *__restrict__ wrow,
                                                         size_t n_words, uint8_t *__restrict__ lcp) {
  const size_t s = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (s >= n_words) return;
  uint32_t l = 0;
  if (s != 0) {
    const uint32_t a = val[s - 1], b = val[s];
    if (wp_checked(a < n_words && b < n_words, kSiteQuality)) {
      const size_t lo = min(a, b), hi = max(a, b);
      const uint32_t row = wrow[hi];
      for (; l < static_cast<uint32_t>(kRptMaxN); l++) {
        if (hi + l >= n_words || wrow[hi + l] != row || r1[lo + l] != r1[hi + l]) break;
      }
    }
  }
  lcp[s] = static_cast<uint8_t>(l);
}

// head[j][s] = 1 where slot s opens a run of the length n0 + j; entry n_words closes the flags for their scan
__global__ __launch_bounds__(kBlock) void rpt_heads_kernel(const uint8_t *__restrict__ lcp, size_t n_words, uint32_t n0, RptRuns runs) {
  const size_t s = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (s > n_words) return;
  const uint32_t l = s < n_words && s != 0 ? lcp[s] : 0u;
#pragma unroll
  for (int j = 0; j < kRptGroup; j++) runs.head[j][s] = s < n_words && l < n0 + j ? 1u : 0u;
}

// aux[j][r] = the slot of the head of run r of the length n0 + j, and n_words behind the last run
__global__ __launch_bounds__(kBlock) void rpt_head_pos_kernel(size_t n_words, RptRuns runs) {
  const size_t s = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (s > n_words) return;
#pragma unroll
  for (int j = 0; j < kRptGroup; j++) {
    const uint32_t r = runs.run[j][s];  // (s == n_words: the number of runs)
    if ((s == n_words || runs.head[j][s]) && wp_checked(r <= n_words, kSiteQuality)) runs.aux[j][r] = static_cast<uint32_t>(s);
  }
}

// n = 2..4.  The head of a run of two or more slots: (occurrences, characters of the n-gram) into top[n - 2][row] by atomicMax
__global__ __launch_bounds__(kBlock) void rpt_top_kernel(const uint32_t *__restrict__ val, size_t n_words, RptRuns runs, const uint32_t *__restrict__ wrow,
                                                         const uint32_t *__restrict__ wchars, size_t n_rows, unsigned long long *__restrict__ top) {
  const size_t s = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (s >= n_words) return;
#pragma unroll
  for (int j = 0; j < kRptGroup; j++) {
    if (!runs.head[j][s]) continue;
    const uint32_t r = runs.run[j][s];
    if (!wp_checked(r < n_words, kSiteQuality)) continue;
    const uint32_t next = runs.aux[j][r + 1];
    if (next <= s + 1) continue;  // (one occurrence)
    const uint32_t p = val[s], n = 2u + j;
    if (!wp_checked(static_cast<size_t>(p) + n <= n_words, kSiteQuality)) continue;
    const uint32_t row = wrow[p];
    if (!wp_checked(row < n_rows, kSiteQuality)) continue;
    uint32_t chars = 0;
    for (uint32_t i = 0; i < n; i++) chars += wchars[p + i];
    atomicMax(&top[static_cast<size_t>(j) * n_rows + row], (static_cast<unsigned long long>(next - s) << 32) | chars);
  }
}

// whether slot s is a run of its own
__device__ __forceinline__ bool rpt_alone(const uint32_t *__restrict__ head, size_t s, size_t n_words) { return head[s] && (s + 1 == n_words || head[s + 1]); }

// n = 5..10, first pass: aux[j][run of s] = the smallest position of the run (cleared to ~0); runs of one slot stay out
__global__ __launch_bounds__(kBlock) void rpt_first_kernel(const uint32_t *__restrict__ val, size_t n_words, RptRuns runs) {
  const size_t s = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (s >= n_words) return;
  const uint32_t p = val[s];
#pragma unroll
  for (int j = 0; j < kRptGroup; j++) {
    if (rpt_alone(runs.head[j], s, n_words)) continue;
    const uint32_t r = run_of(runs.head[j], runs.run[j], s);
    if (wp_checked(r < n_words, kSiteQuality)) atomicMin(&runs.aux[j][r], p);
  }
}

// ... second pass: flags[p] = bit j where the window of n0 + j words at p is not the first occurrence of its run.  Every
// position has one slot and the pass has the array to itself: a plain store of the whole byte, whatever ran before.
__global__ __launch_bounds__(kBlock) void rpt_mark_kernel(const uint32_t *__restrict__ val, size_t n_words, RptRuns runs, uint8_t *__restrict__ flags) {
  const size_t s = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (s >= n_words) return;
  const uint32_t p = val[s];
  uint32_t bits = 0;
#pragma unroll
  for (int j = 0; j < kRptGroup; j++) {
    if (rpt_alone(runs.head[j], s, n_words)) continue;
    const uint32_t r = run_of(runs.head[j], runs.run[j], s);
    if (wp_checked(r < n_words, kSiteQuality) && runs.aux[j][r] != p) bits |= 1u << j;
  }
  if (wp_checked(p < n_words, kSiteQuality)) flags[p] = static_cast<uint8_t>(bits);
}

// Tile blockIdx.x of the words: WORDS, WORD_CHARS and the covered characters of every length into sig ([WP_RPT_SIGNALS][n_rows]).
// flags: the bytes of the pass n = 5..7, then from n_words on those of n = 8..10.
__global__ __launch_bounds__(kBlock) void rpt_cover_kernel(const uint8_t *__restrict__ flags, const uint32_t *__restrict__ wrow, const uint32_t *__restrict__ wchars,
                                                           size_t n_words, size_t n_rows, unsigned long long *__restrict__ sig) {
  __shared__ uint8_t s_flag[kRptHalo + kBlock];
  __shared__ uint32_t s_row[kRptHalo + kBlock];
  __shared__ uint32_t s_acc[kRptSlots * kRptAcc];
  const int tid = threadIdx.x;
  const size_t base = static_cast<size_t>(blockIdx.x) * kBlock;
  for (int k = tid; k < kRptHalo + kBlock; k += kBlock) {
    const long long j = static_cast<long long>(base) - kRptHalo + k;
    const bool in = j >= 0 && static_cast<size_t>(j) < n_words;
    s_flag[k] = in ? static_cast<uint8_t>(flags[j] | (flags[n_words + j] << kRptGroup)) : 0;
    s_row[k] = in ? wrow[j] : 0xffffffffu;
  }
  for (int k = tid; k < kRptSlots * kRptAcc; k += kBlock) s_acc[k] = 0;
  __syncthreads();
  const uint32_t r_lo = s_row[kRptHalo];  // (base < n_words: the row of the tile's first word)
  const size_t j = base + tid;
  if (j < n_words) {
    const int k = kRptHalo + tid;
    const uint32_t row = s_row[k], ch = wchars[j];
    uint32_t cov = 0;
#pragma unroll
    for (int d = 0; d < kRptMaxN; d++) {  // a duplicate window of n words that begins d words back holds word j iff n > d
      const uint32_t lengths = (0x3fu << (d > 4 ? d - 4 : 0)) & 0x3fu;
      if (s_row[k - d] == row) cov |= s_flag[k - d] & lengths;
    }
    if (wp_checked(row < n_rows, kSiteQuality)) {
      auto add = [&](int a, uint32_t x) {
        if (x == 0) return;
        if (row - r_lo < static_cast<uint32_t>(kRptSlots)) {
          atomicAdd(&s_acc[(row - r_lo) * kRptAcc + a], x);
        } else {
          atomicAdd(&sig[static_cast<size_t>(a < 2 ? a : a + WP_RPT_DUP_5_CHARS - 2) * n_rows + row], static_cast<unsigned long long>(x));
        }
      };
      add(0, 1u);
      add(1, ch);
#pragma unroll
      for (int b = 0; b < 6; b++) {
        if ((cov >> b) & 1u) add(2 + b, ch);
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < kRptSlots * kRptAcc; i += kBlock) {
    const uint32_t x = s_acc[i];
    const size_t r = static_cast<size_t>(r_lo) + i / kRptAcc;
    const int a = i % kRptAcc;
    if (x != 0 && wp_checked(r < n_rows, kSiteQuality)) {
      atomicAdd(&sig[static_cast<size_t>(a < 2 ? a : a + WP_RPT_DUP_5_CHARS - 2) * n_rows + r], static_cast<unsigned long long>(x));
    }
  }
}

// Row i: TOP_n_COUNT and TOP_n_CHARS from top, the rules over its signals, keep[i] = 1 where none failed (keep[n_rows] = 0
// closes the flags); the rows each rule failed and the totals of the call into the counters.
__global__ __launch_bounds__(kBlock) void rpt_rules_kernel(size_t n_rows, RptLimits lim, const unsigned long long *__restrict__ top, long long *__restrict__ sig,
                                                           uint32_t *__restrict__ reasons, uint32_t *__restrict__ keep, unsigned long long *__restrict__ counters) {
  const size_t i = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  uint32_t r = 0;
  unsigned long long words = 0, chars = 0;
  if (i < n_rows) {
    long long s[WP_RPT_SIGNALS];
#pragma unroll
    for (int j = 0; j < kRptGroup; j++) {
      const unsigned long long t = top[static_cast<size_t>(j) * n_rows + i];
      const long long count = static_cast<long long>(t >> 32);
      sig[static_cast<size_t>(WP_RPT_TOP_2_COUNT + 2 * j) * n_rows + i] = count;
      sig[static_cast<size_t>(WP_RPT_TOP_2_CHARS + 2 * j) * n_rows + i] = count * static_cast<long long>(t & 0xffffffffull);
    }
#pragma unroll
    for (int k = 0; k < WP_RPT_SIGNALS; k++) s[k] = sig[static_cast<size_t>(k) * n_rows + i];
    r = repetition_reasons(s, lim);
    reasons[i] = r;
    keep[i] = r == 0 ? 1u : 0u;
    words = s[WP_RPT_WORDS];
    chars = s[WP_RPT_WORD_CHARS];
  } else if (i == n_rows) {
    keep[i] = 0;
  }
  words = wave_reduce_sum64(words);
  chars = wave_reduce_sum64(chars);
  if (lane_id() == 0 && words != 0) atomicAdd(&counters[kRptWordsTotal], words);
  if (lane_id() == 0 && chars != 0) atomicAdd(&counters[kRptWordChars], chars);
  for (int k = 0; k < WP_RPT_RULES; k++) {
    const unsigned long long f = __popcll(__ballot((r >> k) & 1u));
    if (lane_id() == 0 && f != 0) atomicAdd(&counters[kRptRuleFailed + k], f);
  }
}

}  // namespace wp
