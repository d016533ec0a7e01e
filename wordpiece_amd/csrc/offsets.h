// offsets.h — offsets mode of the Linear path (wp_linear_encode_offsets): code-point spans to byte spans.
//
// The walk leaves every id's span [begin, end) in code points (walk.h, StagedSpanOut / SparseSpanOut).  The byte unit
// needs the byte of every code point: byte_of[p], written from the decoder's own row loads and valid-lead masks
// (decode.h, utf8_swar.h), so that an invalid sequence is dropped by the same verdicts the decoder gave it.  A span
// [b, e) then covers bytes [byte_of[b], byte_of[e - 1] + length of the sequence that starts there): dropped bytes
// inside it belong to it, dropped bytes between two spans to neither.
#pragma once
#include "decode.h"
#include "walk.h"

namespace wp {

// byte_of[p] = first byte of code point p (same tiles and order as decode_write_kernel: tile_prefix = its output
// position of the tile)
__global__ __launch_bounds__(kBlock) void cp_byte_kernel(const uint8_t *__restrict__ text, size_t nbytes,
                                                         const uint32_t *__restrict__ tile_prefix, size_t n_text,
                                                         uint32_t *__restrict__ byte_of) {
  __shared__ uint32_t s_rows[kBlock / kWave][kDecRows];
  const int lane = lane_id(), wv = wave_id();
  const size_t tile_base = static_cast<size_t>(blockIdx.x) * kDecTile;
  const size_t wave_base = tile_base + static_cast<size_t>(wv) * kDecWaveBytes;
  uint32_t w[kDecRows][5];
  dec_load_rows(text, nbytes, wave_base, lane, w);
  uint32_t starts[kDecRows], row_cnt[kDecRows];
#pragma unroll
  for (int r = 0; r < kDecRows; r++) {
    const size_t off = wave_base + static_cast<size_t>(r) * kDecRowBytes + static_cast<size_t>(lane) * kDecChunk;
    const uint32_t inside = dec_inside16(off, nbytes);
    uint32_t m = 0;
    if (((w[r][0] | w[r][1] | w[r][2] | w[r][3]) & kHi) == 0u) {
      m = inside;
    } else {
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const Utf8Starts u = utf8_starts(w[r][k], w[r][k + 1]);
        m |= byte_mask4(u.v1 | u.v2 | u.v3 | u.v4) << (4 * k);
      }
      m &= inside;
    }
    starts[r] = m;
    row_cnt[r] = wave_reduce_sum(__popc(m));
  }
  if (lane == 0) {
#pragma unroll
    for (int r = 0; r < kDecRows; r++) s_rows[wv][r] = row_cnt[r];
  }
  __syncthreads();
  size_t out = tile_prefix[blockIdx.x];
  for (int i = 0; i < wv; i++) {
#pragma unroll
    for (int r = 0; r < kDecRows; r++) out += s_rows[i][r];
  }
#pragma unroll
  for (int r = 0; r < kDecRows; r++) {
    const uint32_t off = static_cast<uint32_t>(wave_base + static_cast<size_t>(r) * kDecRowBytes + static_cast<size_t>(lane) * kDecChunk);
    uint32_t m = starts[r];
    const uint32_t c = __popc(m);
    size_t o = out + (wave_incl_sum(c) - c);
    if (m == 0xffffu && wp_in_bounds(o + kDecChunk <= n_text, kSiteSpan) && o + kDecChunk <= n_text) {  // 16 one-byte code points
      typedef uint32_t u32x4 __attribute__((ext_vector_type(4), aligned(4)));
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const uint32_t b = off + 4u * static_cast<uint32_t>(k);
        *reinterpret_cast<u32x4 *>(byte_of + o + 4 * k) = u32x4{b, b + 1u, b + 2u, b + 3u};
      }
    } else {
      while (m) {
        const int j = __ffs(static_cast<int>(m)) - 1;
        m &= m - 1u;
        if (wp_in_bounds(o < n_text, kSiteSpan) && o < n_text) byte_of[o] = off + static_cast<uint32_t>(j);
        o++;
      }
    }
    out += row_cnt[r];
  }
}

// offs[k] = [begin, end) of id k in code points -> in bytes (in place)
__global__ __launch_bounds__(kBlock) void span_bytes_kernel(uint2 *__restrict__ offs, size_t n_ids, const uint32_t *__restrict__ byte_of,
                                                            const uint8_t *__restrict__ text, size_t n_text) {
  const size_t k = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (k >= n_ids) return;
  const uint2 s = offs[k];
  const bool ok = s.x < s.y && s.y <= n_text;
  if (!wp_in_bounds(ok, kSiteSpan) || !ok) {
    offs[k] = make_uint2(0u, 0u);
    return;
  }
  const uint32_t b = byte_of[s.x], l = byte_of[s.y - 1u];
  const uint32_t lead = text[l];
  const uint32_t len = lead < 0x80u ? 1u : lead < 0xe0u ? 2u : lead < 0xf0u ? 3u : 4u;  // (a valid lead)
  offs[k] = make_uint2(b, l + len);
}

}  // namespace wp
