// scrub.h — the kernels of the scrub (include/wordpiece_amd_scrub.h; host path: scrub_path.h): e-mail and IPv4 addresses
// found by character class and bounded run, and the text rewritten with placeholders of other lengths.
//   Find.  A tile of kQualTile bytes per workgroup, staged in LDS as words with kScFront bytes in front of it and
// kScBehind behind it.  Every lane classifies groups of eight bytes once and leaves one BYTE per class in a bit plane:
// LOC, DOM, NUM, AN, AL, '.', '@', WORDISH, one bit per position of the span; the row starts that fall into the span are
// ORed into a ninth plane, which is all a run needs to stay inside its row.  From there on nothing looks at single bytes
// to measure a run: 64 positions of a plane are one unaligned 64-bit read, the local run in front of an '@' is a count of
// leading ones, the domain run behind it a count of trailing ones over at most four such reads, the next label edge a
// count of trailing zeros in the '.' plane, an AL-only label one masked compare.  A lane owns the '@' bytes and the
// starts of NUM runs among its kQualItems positions, so matches come out in text order (the surviving matches are
// disjoint, and an e-mail holds its '@').  An IPv4 match lies inside an e-mail iff the '@' behind its LOC run or the
// nearest '@' within 256 bytes in front of it matches and covers it: the lane evaluates that e-mail itself from the
// planes, which is why the halo is wider than one match (and why no pass over the matches is needed to drop them).
//   The kernel runs twice, as qual_class_kernel does: first the matches of every tile are counted and the counts scanned;
// the second run stores each match with its row, kind, the FNV-1a hash's pick among the replacements and the change of
// length, adds the per-row signals by 64-bit integer atomics and the two 64-bit totals the output size comes from.
//   Offsets.  One exclusive scan over the MATCHES of (replacement length - match length), modulo 2^32: E.  A byte at p
// that no match holds goes to p + E[matches that start at or in front of p]; no per-byte flag, no per-byte scan.
//   Write.  A tile of input bytes per workgroup finds by bisection the matches that meet it (at most kScTileMatches: an
// e-mail has six bytes at least, an address seven) and stages them with their E.  The stretches between matches are
// copied one after the other by the whole workgroup: every output word that lies inside a stretch is gathered from the
// staged input with a funnel shift and stored aligned, the at most three bytes at either edge byte by byte.  The
// replacement of a match is written, from the pool in LDS, by the tile that holds the match's first byte.
//   Rules, one lane per row: BYTES, OUT_BYTES and out_off from two bisections over the match starts, the reasons, the
// keep flag, the statistics.
#pragma once
#include "../../include/wordpiece_amd_scrub.h"
#include "quality.h"

namespace wp {

constexpr int kScFront = 328;   // staged bytes in front of a tile: an '@' 256 in front of an address, its local run (65), whole groups
constexpr int kScBehind = 328;  // behind it: an address (16), the rest of a local run (64), the '@', a domain run (256) from there
constexpr int kScSpan = kScFront + kQualTile + kScBehind;
constexpr int kScGroups = kScSpan / 8;
constexpr int kScPlaneWords = kScSpan / 64 + 4;  // 64-bit words of a plane: a read may begin 64 + 255 positions behind the last '@' looked at
constexpr int kScTxtWords = kScSpan / 4 + 24;    // (the label edges of such an e-mail are read as bytes: zeros behind the span)
constexpr int kScTileMatches = kQualTile / 6 + 2;
constexpr int kScPoolWords = WP_SCRUB_MAX_POOL_BYTES / 4;  // the replacement pool on the device, zero-padded
static_assert(kScFront % 8 == 0 && kScSpan % 8 == 0, "whole groups of eight positions");
enum ScPlane { kScLoc, kScDom, kScNum, kScAn, kScAl, kScDot, kScAt, kScWord, kScBnd, kScPlanes };

// the counters of a call, 64 bits each, in d_scalars from kScalarScrub on
enum ScrubCounter { kScRuleFailed = 0, kScKinds = 2, kScAdded = 5, kScRemoved = 6, kScCounters = 8 };

struct ScLimits {
  long long doc[WP_SCRUB_RULES];
};
// the replacement strings: off[t] .. off[t + 1] of the pool, the e-mail strings first
struct ScRepl {
  uint16_t off[2 * WP_SCRUB_MAX_REPL + 1];
  uint16_t n_email, n_ip;
};
// the matches of a call in text order
struct ScMatches {
  uint32_t *start, *delta;             // the first byte; replacement length - length modulo 2^32 (the host clears delta[n], which closes it)
  int32_t *row, *len, *kind, *repl;
  long long *start64;                  // optional: match_start of the result
  size_t n;
};

// The document rules over the signals of one row; the host-answered batch and scrub_docs_kernel share this function.
__host__ __device__ inline uint32_t scrub_reasons(const long long *s, const ScLimits &lim) {
  uint32_t r = 0;
  if (lim.doc[WP_SR_MAX_EMAILS] >= 0 && s[WP_SS_EMAILS] > lim.doc[WP_SR_MAX_EMAILS]) r |= 1u << WP_SR_MAX_EMAILS;
  if (lim.doc[WP_SR_MAX_IPS] >= 0 && s[WP_SS_IPS] + s[WP_SS_IPS_LEFT] > lim.doc[WP_SR_MAX_IPS]) r |= 1u << WP_SR_MAX_IPS;
  return r;
}

// the private ranges of the header
__host__ __device__ inline bool scrub_private(uint32_t a) {
  const uint32_t a8 = a >> 24;
  return a8 == 0 || a8 == 10 || a8 == 127 || (a >> 16) == ((169u << 8) | 254u) || (a >> 20) == ((172u << 4) | 1u) || (a >> 16) == ((192u << 8) | 168u) || a8 >= 224;
}

// 64 positions of a plane from position q on (bit i: position q + i), and one position
__device__ __forceinline__ uint64_t sc_bits(const uint64_t *pl, int q) {
  const uint64_t w0 = pl[q >> 6], w1 = pl[(q >> 6) + 1];
  const int sh = q & 63;
  return sh ? (w0 >> sh) | (w1 << (64 - sh)) : w0;
}
__device__ __forceinline__ bool sc_bit(const uint64_t *pl, int q) { return (pl[q >> 6] >> (q & 63)) & 1ull; }
__device__ __forceinline__ int sc_ones_low(uint64_t x) { return x == ~0ull ? 64 : __builtin_ctzll(~x); }   // trailing ones
__device__ __forceinline__ int sc_ones_high(uint64_t x) { return x == ~0ull ? 64 : __builtin_clzll(~x); }  // leading ones

// The e-mail at the '@' at span position k (65 <= k, k + 320 inside the planes): -> whether it matches, [s, e).
__device__ __noinline__ bool sc_email_at(const uint64_t (*pl)[kScPlaneWords], const uint8_t *txt, int k, int &s, int &e) {
  const uint64_t *bnd = pl[kScBnd];
  // position k - 64 + i may join the run iff it is LOC and no row begins behind it
  const uint64_t G = sc_bits(pl[kScLoc], k - 64) & ~sc_bits(bnd, k - 63);
  const int L = sc_ones_high(G);
  if (L == 0) return false;
  const int f = k - 1 - L;  // the byte in front of R, inside the row iff no row begins at R's first byte
  const bool f_in = !sc_bit(bnd, f + 1);
  if (f_in && (txt[f] == '@' || (L == 64 && sc_bit(pl[kScLoc], f)))) return false;
  const uint64_t A = sc_bits(pl[kScAn], k - 64) & (L == 64 ? ~0ull : ~0ull << (64 - L));
  if (A == 0) return false;
  s = k - 64 + __builtin_ctzll(A);
  int n = 0;  // the bytes of D
  for (int i = 0; i < 4; i++) {
    const int t = sc_ones_low(sc_bits(pl[kScDom], k + 1 + 64 * i) & ~sc_bits(bnd, k + 1 + 64 * i));
    n += t;
    if (t < 64) break;
  }
  if (n >= 256) return false;
  int pos = 0, labels = 0, end = -1;
  while (pos < n) {
    const uint64_t dots = sc_bits(pl[kScDot], k + 1 + pos);
    const int len = min(dots ? __builtin_ctzll(dots) : 64, n - pos);
    if (len < 1 || len > 63 || txt[k + 1 + pos] == '-' || txt[k + pos + len] == '-') break;
    labels++;
    const uint64_t m = (1ull << len) - 1ull;
    if (labels >= 2 && len >= 2 && (sc_bits(pl[kScAl], k + 1 + pos) & m) == m) end = pos + len;
    pos += len + 1;
  }
  e = k + 1 + end;
  return end >= 0;
}

// The IPv4 address of the NUM run that starts at span position k of the tile: -> whether it matches, its length and value.
__device__ __noinline__ bool sc_ipv4_at(const uint64_t (*pl)[kScPlaneWords], const uint8_t *txt, int k, int &len, uint32_t &addr) {
  const uint64_t *bnd = pl[kScBnd];
  int n = sc_ones_low(sc_bits(pl[kScNum], k) & ~(sc_bits(bnd, k) & ~1ull));
  if (n > 16) return false;
  if (!sc_bit(bnd, k) && sc_bit(pl[kScWord], k - 1)) return false;
  if (!sc_bit(bnd, k + n) && sc_bit(pl[kScWord], k + n)) return false;
  if (txt[k + n - 1] == '.') n--;
  uint32_t a = 0, val = 0;
  int parts = 0, digits = 0;
  for (int i = 0; i < n; i++) {
    const uint32_t c = txt[k + i];
    if (c == '.') {
      if (digits == 0) return false;
      a = (a << 8) | val;
      parts++;
      digits = 0;
      val = 0;
    } else {
      if (digits == 1 && val == 0) return false;
      val = val * 10 + (c - '0');
      if (++digits > 3 || val > 255) return false;
    }
  }
  if (digits == 0 || parts != 3) return false;
  len = n;
  addr = (a << 8) | val;
  return true;
}

// whether an e-mail holds the IPv4 match [k, k + len): the '@' that ends its LOC run, or the nearest '@' in front
__device__ __forceinline__ bool sc_inside_email(const uint64_t (*pl)[kScPlaneWords], const uint8_t *txt, int k, int len) {
  const uint64_t *bnd = pl[kScBnd];
  const int b = k + len;
  int s, e;
  const uint64_t G = sc_bits(pl[kScLoc], b) & ~sc_bits(bnd, b);
  if (G != ~0ull) {
    const int q = b + __builtin_ctzll(~G);
    if (!sc_bit(bnd, q) && txt[q] == '@' && sc_email_at(pl, txt, q, s, e) && s <= k) return true;
  }
  for (int i = 1; i <= 4; i++) {
    const uint64_t w = sc_bits(pl[kScAt], k - 64 * i);
    if (w == 0) continue;
    const int p = k - 64 * i + 63 - __builtin_clzll(w);
    return sc_email_at(pl, txt, p, s, e) && e >= b;
  }
  return false;
}

// Tile blockIdx.x of the bytes (n_bytes >= 1, n_rows >= 1).  kWrite false: tiles[t] = the matches the tile owns.  kWrite
// true: tiles holds the exclusive scan of the counts; the matches are stored, sig ([WP_SCRUB_SIGNALS][n_rows], cleared)
// and the counters get their sums.
template <bool kWrite>
__global__ __launch_bounds__(kBlock) void scrub_find_kernel(const uint32_t *__restrict__ d32, size_t n_bytes, const uint32_t *__restrict__ byte_off, size_t n_rows,
                                                            int kinds, ScRepl rp, uint32_t *__restrict__ tiles, ScMatches out, unsigned long long *__restrict__ sig,
                                                            unsigned long long *__restrict__ counters) {
  __shared__ uint32_t s_txt[kScTxtWords];
  __shared__ uint64_t s_pl[kScPlanes][kScPlaneWords];
  __shared__ uint32_t s_rows[2];
  __shared__ uint32_t s_scan[8];
  const int tid = threadIdx.x;
  const size_t base = static_cast<size_t>(blockIdx.x) * kQualTile;
  const long long origin = static_cast<long long>(base) - kScFront;
  const uint8_t *txt = reinterpret_cast<const uint8_t *>(s_txt);
  for (int i = tid; i < kScTxtWords; i += kBlock) {
    const long long p = origin + 4ll * i;  // (whole aligned words that begin inside the data; what lies behind its last byte is cleared)
    uint32_t x = 0;
    if (i < kScSpan / 4 && p >= 0 && static_cast<size_t>(p) < n_bytes) {
      x = d32[p >> 2];
      if (static_cast<size_t>(p) + 4 > n_bytes) x &= (1u << (8u * static_cast<uint32_t>(n_bytes - static_cast<size_t>(p)))) - 1u;
    }
    s_txt[i] = x;
  }
  for (int i = tid; i < kScPlanes * kScPlaneWords; i += kBlock) (&s_pl[0][0])[i] = 0;
  if (tid == 0 || tid == kWave) {  // the rows of the first and the last position of the span inside the data
    const size_t e = tid == 0 ? static_cast<size_t>(origin > 0 ? origin : 0) : min(base + kQualTile + kScBehind, n_bytes) - 1;
    s_rows[tid != 0] = ovl_row_of(byte_off, 0, static_cast<uint32_t>(n_rows - 1), e);
  }
  __syncthreads();
  const uint32_t r_lo = s_rows[0], r_hi = s_rows[1];
  // ---- the planes: a byte per class and group of eight positions; the row starts (and the end of the last row) ---------
  for (int g = tid; g < kScGroups; g += kBlock) {
    const uint32_t x0 = s_txt[2 * g], x1 = s_txt[2 * g + 1];
    uint32_t bits[kScBnd] = {};
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const uint32_t b = ((j < 4 ? x0 : x1) >> (8 * (j & 3))) & 0xffu;
      const bool al = ((b | 32u) - 'a') < 26u, dg = (b - '0') < 10u, an = al || dg, dot = b == '.', hy = b == '-';
      bits[kScAl] |= static_cast<uint32_t>(al) << j;
      bits[kScAn] |= static_cast<uint32_t>(an) << j;
      bits[kScDot] |= static_cast<uint32_t>(dot) << j;
      bits[kScNum] |= static_cast<uint32_t>(dg || dot) << j;
      bits[kScDom] |= static_cast<uint32_t>(an || dot || hy) << j;
      bits[kScLoc] |= static_cast<uint32_t>(an || dot || hy || b == '_' || b == '%' || b == '+') << j;
      bits[kScAt] |= static_cast<uint32_t>(b == '@') << j;
      bits[kScWord] |= static_cast<uint32_t>(an || b == '_' || b >= 0x80u) << j;
    }
#pragma unroll
    for (int c = 0; c < kScBnd; c++) reinterpret_cast<uint8_t *>(s_pl[c])[g] = static_cast<uint8_t>(bits[c]);
  }
  for (size_t r = static_cast<size_t>(r_lo) + tid; r <= static_cast<size_t>(r_hi) + 1; r += kBlock) {
    const long long q = static_cast<long long>(byte_off[r]) - origin;
    if (q >= 0 && q < kScSpan) atomicOr(reinterpret_cast<uint32_t *>(s_pl[kScBnd]) + (q >> 5), 1u << (q & 31));
  }
  __syncthreads();
  // ---- a lane's positions: the '@' bytes and the starts of the NUM runs among them ---------------------------------------
  const int k0 = kScFront + tid * kQualItems, g0 = k0 >> 3;
  const size_t p0 = base + static_cast<size_t>(tid) * kQualItems;
  const uint32_t at8 = reinterpret_cast<const uint8_t *>(s_pl[kScAt])[g0], num8 = reinterpret_cast<const uint8_t *>(s_pl[kScNum])[g0];
  const uint32_t bnd8 = reinterpret_cast<const uint8_t *>(s_pl[kScBnd])[g0];
  const uint32_t prev = (num8 << 1) | (sc_bit(s_pl[kScNum], k0 - 1) ? 1u : 0u);
  uint32_t cand_at = at8, cand_ip = (kinds & WP_SCRUB_IPV4) ? num8 & (bnd8 | ~prev) & 0xffu : 0u;
  uint32_t found = 0;
  uint32_t mv[kQualItems] = {};  // write pass, per key position (registers: only constant indices below): the match's start in front of it | length << 8 | kind << 20 | pick << 24
  unsigned long long added = 0, removed = 0;
  while (cand_at | cand_ip) {
    const int j = __builtin_ctz(cand_at | cand_ip), k = k0 + j;
    const bool is_at = (cand_at >> j) & 1u;
    cand_at &= ~(1u << j);
    cand_ip &= ~(1u << j);
    int s = 0, len = 0, kind = 0;
    bool hit = false;
    uint32_t row = 0;
    if (kWrite && is_at) {
      row = ovl_row_of(byte_off, r_lo, r_hi, p0 + j);
      if (wp_checked(row < n_rows, kSiteQuality)) atomicAdd(&sig[static_cast<size_t>(WP_SS_AT_SIGNS) * n_rows + row], 1ull);
    }
    if (is_at) {
      int e = 0;
      hit = (kinds & WP_SCRUB_EMAIL) && sc_email_at(s_pl, txt, k, s, e);
      len = e - s;
    } else {
      uint32_t addr = 0;
      hit = sc_ipv4_at(s_pl, txt, k, len, addr) && !((kinds & WP_SCRUB_EMAIL) && sc_inside_email(s_pl, txt, k, len));
      s = k;
      kind = (kinds & WP_SCRUB_IP_KEEP_PRIVATE) && scrub_private(addr) ? 2 : 1;
    }
    if (!hit) continue;
    found |= 1u << j;
    if constexpr (kWrite) {
      uint32_t pick = 0;
      if (kind != 2) {
        uint32_t h = 2166136261u;
        for (int i = 0; i < len; i++) {
          uint32_t b = txt[s + i];
          if (b - 'A' < 26u) b += 32u;
          h = (h ^ b) * 16777619u;
        }
        pick = h % (kind == 0 ? rp.n_email : rp.n_ip);
      }
      const uint32_t packed = static_cast<uint32_t>(k - s) | (static_cast<uint32_t>(len) << 8) | (static_cast<uint32_t>(kind) << 20) | (pick << 24);
#pragma unroll
      for (int i = 0; i < kQualItems; i++) mv[i] = i == j ? packed : mv[i];
      if (!is_at) row = ovl_row_of(byte_off, r_lo, r_hi, p0 + j);
      if (wp_checked(row < n_rows, kSiteQuality)) {
        atomicAdd(&sig[static_cast<size_t>(kind == 0 ? WP_SS_EMAILS : kind == 1 ? WP_SS_IPS : WP_SS_IPS_LEFT) * n_rows + row], 1ull);
        if (kind != 2) atomicAdd(&sig[static_cast<size_t>(kind == 0 ? WP_SS_EMAIL_BYTES : WP_SS_IP_BYTES) * n_rows + row], static_cast<unsigned long long>(len));
      }
    }
  }
  uint32_t total;
  const uint32_t ex = block_excl_sum(__popc(found), s_scan, total);
  if constexpr (!kWrite) {
    if (tid == 0) tiles[blockIdx.x] = total;
  } else {
    size_t at = static_cast<size_t>(tiles[blockIdx.x]) + ex;
#pragma unroll
    for (int j = 0; j < kQualItems; j++) {
      if (!((found >> j) & 1u)) continue;
      const uint32_t m = mv[j];
      const uint32_t back = m & 0xffu, len = (m >> 8) & 0xfffu, kind = (m >> 20) & 3u, pick = m >> 24;
      const size_t start = p0 + j - back;
      const uint32_t t = pick + (kind == 1 ? rp.n_email : 0u);
      const uint32_t rlen = kind == 2 ? len : static_cast<uint32_t>(rp.off[t + 1] - rp.off[t]);
      if (wp_checked(at < out.n, kSiteQuality)) {
        out.start[at] = static_cast<uint32_t>(start);
        out.delta[at] = rlen - len;
        out.row[at] = static_cast<int32_t>(ovl_row_of(byte_off, r_lo, r_hi, start));
        out.len[at] = static_cast<int32_t>(len);
        out.kind[at] = static_cast<int32_t>(kind);
        out.repl[at] = kind == 2 ? -1 : static_cast<int32_t>(pick);
        if (out.start64) out.start64[at] = static_cast<long long>(start);
      }
      if (kind != 2) {
        added += rlen;
        removed += len;
      }
      at++;
    }
    added = wave_reduce_sum64(added);
    removed = wave_reduce_sum64(removed);
    if (lane_id() == 0 && added != 0) atomicAdd(&counters[kScAdded], added);
    if (lane_id() == 0 && removed != 0) atomicAdd(&counters[kScRemoved], removed);
  }
}

// Row i (E: the exclusive scan of delta over n + 1 entries): out_off[i] and out_boff[i] = the row's start plus the E of the
// first match at or behind it, entry n_rows closes both; BYTES, OUT_BYTES, the rules, keep[i] = 1 where none failed
// (keep[n_rows] = 0 closes the flags); the rows each rule failed and the matches of each kind into the counters.
__global__ __launch_bounds__(kBlock) void scrub_docs_kernel(const uint32_t *__restrict__ byte_off, size_t n_rows, const uint32_t *__restrict__ mstart,
                                                            const uint32_t *__restrict__ E, size_t n_matches, ScLimits lim, long long *__restrict__ sig,
                                                            uint32_t *__restrict__ reasons, uint32_t *__restrict__ keep, long long *__restrict__ out_off,
                                                            uint32_t *__restrict__ out_boff, unsigned long long *__restrict__ counters) {
  const size_t i = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  auto out_at = [&](uint32_t a) {
    size_t lo = 0, hi = n_matches;
    while (lo < hi) {
      const size_t mid = (lo + hi) >> 1;
      if (mstart[mid] < a) lo = mid + 1; else hi = mid;
    }
    return a + E[lo];  // (modulo 2^32: the true value fits, the host checked the total)
  };
  uint32_t r = 0;
  unsigned long long tot[3] = {};
  if (i <= n_rows) {
    const uint32_t o0 = out_at(byte_off[i]);
    out_off[i] = o0;
    out_boff[i] = o0;
    if (i == n_rows) keep[i] = 0;
    if (i < n_rows) {
      long long s[WP_SCRUB_SIGNALS];
#pragma unroll
      for (int k = 0; k < WP_SCRUB_SIGNALS; k++) s[k] = sig[static_cast<size_t>(k) * n_rows + i];
      s[WP_SS_BYTES] = static_cast<long long>(byte_off[i + 1]) - static_cast<long long>(byte_off[i]);
      s[WP_SS_OUT_BYTES] = static_cast<long long>(out_at(byte_off[i + 1]) - o0);
      sig[static_cast<size_t>(WP_SS_BYTES) * n_rows + i] = s[WP_SS_BYTES];
      sig[static_cast<size_t>(WP_SS_OUT_BYTES) * n_rows + i] = s[WP_SS_OUT_BYTES];
      r = scrub_reasons(s, lim);
      reasons[i] = r;
      keep[i] = r == 0 ? 1u : 0u;
      tot[0] = s[WP_SS_EMAILS];
      tot[1] = s[WP_SS_IPS];
      tot[2] = s[WP_SS_IPS_LEFT];
    }
  }
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const unsigned long long t = wave_reduce_sum64(tot[k]);
    if (lane_id() == 0 && t != 0) atomicAdd(&counters[kScKinds + k], t);
  }
  for (int k = 0; k < WP_SCRUB_RULES; k++) {
    const unsigned long long f = __popcll(__ballot((r >> k) & 1u));
    if (lane_id() == 0 && f != 0) atomicAdd(&counters[kScRuleFailed + k], f);
  }
}

// The text behind the scrub, tile blockIdx.x of kQualTile input bytes.  LDS entry j of m is a match that meets the tile
// ([s_ms, s_me); a match that is left alone counts as empty, so its bytes are copied), s_E[j] the E in front of it and
// s_E[m] the E behind the last.  Stretch j lies between entry j - 1 (or the tile's start) and entry j (or its end).
// pool: kScPoolWords words, the replacement strings at the offsets of rp; out: out_bytes / 4 + 1 words.
__global__ __launch_bounds__(kBlock) void scrub_write_kernel(const uint32_t *__restrict__ d32, size_t n_bytes, ScMatches in, const uint32_t *__restrict__ E,
                                                             const uint32_t *__restrict__ pool, ScRepl rp, uint32_t *__restrict__ out, size_t out_bytes) {
  __shared__ uint32_t s_in[kQualTile / 4 + 2];
  __shared__ uint32_t s_pool[kScPoolWords];
  __shared__ uint32_t s_ms[kScTileMatches], s_me[kScTileMatches], s_E[kScTileMatches + 1], s_rp[kScTileMatches];
  __shared__ uint32_t s_range[2];
  const int tid = threadIdx.x;
  const size_t base = static_cast<size_t>(blockIdx.x) * kQualTile, end = min(base + kQualTile, n_bytes);
  for (int i = tid; i < kQualTile / 4 + 2; i += kBlock) {
    const size_t p = base + 4 * static_cast<size_t>(i);
    s_in[i] = p < n_bytes ? d32[p >> 2] : 0u;
  }
  if (tid == 0 || tid == kWave) {  // two lanes of two waves, side by side: the matches that end at or below base / that begin below end
    size_t lo = 0, hi = in.n;
    while (lo < hi) {
      const size_t mid = (lo + hi) >> 1;
      const bool below = tid == 0 ? static_cast<size_t>(in.start[mid]) + static_cast<size_t>(in.len[mid]) <= base : in.start[mid] < end;
      if (below) lo = mid + 1; else hi = mid;
    }
    s_range[tid != 0] = static_cast<uint32_t>(lo);
  }
  __syncthreads();
  const size_t first = s_range[0];
  const uint32_t m = s_range[1] >= s_range[0] ? s_range[1] - s_range[0] : 0u;
  if (!wp_checked(m <= static_cast<uint32_t>(kScTileMatches) && first + m <= in.n, kSiteQuality)) return;  // (the whole workgroup leaves together)
  if (m != 0) {  // (most tiles meet no match and need no replacement)
    for (int i = tid; i < kScPoolWords; i += kBlock) s_pool[i] = pool[i];
  }
  for (uint32_t j = tid; j <= m; j += kBlock) {
    s_E[j] = E[first + j];
    if (j == m) break;
    const uint32_t kind = static_cast<uint32_t>(in.kind[first + j]), len = static_cast<uint32_t>(in.len[first + j]), st = in.start[first + j];
    const uint32_t t = static_cast<uint32_t>(in.repl[first + j]) + (kind == 1 ? rp.n_email : 0u);
    const bool ok = kind == 2 || wp_checked(kind < 2 && t < 2u * WP_SCRUB_MAX_REPL && rp.off[t + 1] <= WP_SCRUB_MAX_POOL_BYTES && rp.off[t] <= rp.off[t + 1], kSiteQuality);
    s_ms[j] = st;
    s_me[j] = kind == 2 || !ok ? st : st + len;
    s_rp[j] = kind == 2 || !ok ? 0u : rp.off[t] | (static_cast<uint32_t>(rp.off[t + 1] - rp.off[t]) << 16);
  }
  __syncthreads();
  uint8_t *out8 = reinterpret_cast<uint8_t *>(out);
  const uint8_t *in8 = reinterpret_cast<const uint8_t *>(s_in), *pool8 = reinterpret_cast<const uint8_t *>(s_pool);
  // ---- the stretches between the matches, shifted by their E ------------------------------------------------------------------
  for (uint32_t j = 0; j <= m; j++) {
    const size_t a = j ? max(base, static_cast<size_t>(s_me[j - 1])) : base, b = j < m ? min(end, static_cast<size_t>(s_ms[j])) : end;
    if (a >= b) continue;
    const uint32_t Ed = s_E[j];
    const size_t oa = static_cast<uint32_t>(static_cast<uint32_t>(a) + Ed), ob = oa + (b - a);
    if (!wp_checked(ob <= out_bytes, kSiteQuality)) continue;
    const size_t w0 = (oa + 3) & ~static_cast<size_t>(3), w1 = ob & ~static_cast<size_t>(3);
    for (size_t x = w0 + 4 * static_cast<size_t>(tid); x < w1; x += 4 * kBlock) {
      const uint32_t k = static_cast<uint32_t>(a - base + (x - oa)), sh = (k & 3u) * 8u;
      const uint32_t lo = s_in[k >> 2], hi = s_in[(k >> 2) + 1];
      out[x >> 2] = sh ? (lo >> sh) | (hi << (32u - sh)) : lo;
    }
    if (tid < 8) {  // the bytes in front of the first whole word (lanes 0..3) and behind the last (lanes 4..7)
      const size_t head_end = min(w0, ob);
      const size_t x = tid < 4 ? oa + tid : max(w1, head_end) + (tid - 4);
      if (x < (tid < 4 ? head_end : ob)) out8[x] = in8[a - base + (x - oa)];
    }
  }
  // ---- the replacements of the matches whose first byte lies in the tile ------------------------------------------------------
  for (uint32_t j = tid; j < m; j += kBlock) {
    if (s_me[j] == s_ms[j] || s_ms[j] < base) continue;
    const uint32_t off = s_rp[j] & 0xffffu, rlen = s_rp[j] >> 16;
    const size_t o = static_cast<uint32_t>(s_ms[j] + s_E[j]);
    if (!wp_checked(o + rlen <= out_bytes, kSiteQuality)) continue;
    for (uint32_t t = 0; t < rlen; t++) out8[o + t] = pool8[off + t];
  }
}

}  // namespace wp
