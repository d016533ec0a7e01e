// fast_path.h — word_piece::fast on the device (fast.cpp:19-150; kernels in fast.h): decode -> code points + class
// bytes -> anchors -> trie walk per word -> id stream.
#pragma once
#include "context.h"
#include "fast.h"
#include "long_word_path.h"
#include "normalize.h"
#include "walk.h"

namespace wp {

static void encode_fast_on_device(const wp_vocab *v, Context *c, const uint8_t *d_text, size_t nbytes, size_t *n_ids_out,
                                  EncodeStats &S) {
  hipStream_t st = c->stream;
  const HostVocab &hv = v->hv;
  std::memset(&S, 0, sizeof(S));
  S.n_bytes = static_cast<int64_t>(nbytes);
  S.longest_token = hv.fast_max_len;
  S.n_devices = 1;
  c->d_ids = nullptr;
  c->dbg = {};
  *n_ids_out = 0;
  if (nbytes == 0) return;  // fast.cpp:154-156
  NormResult norm;
  if (v->normalize != 0) {  // WP_OPT_NORMALIZE: the words are those of the normalised text
    normalize_on_device(c, d_text, nbytes, v->normalize, false, v->stage_timing, norm);
    S.normalize = v->normalize;
    S.norm_bytes = static_cast<int64_t>(norm.nbytes);
    S.ms_normalize = norm.ms;
    if (norm.nbytes == 0) return;
    d_text = norm.text;
    nbytes = norm.nbytes;
  }
  Arena aa(&c->a_buf, v->arena_guard || EnvOptions::get().arena_guard);
  if (v->stage_timing) WP_HIP(hipEventRecord(c->ev[kMarkStart], st));
  const unsigned dec_tiles = cdiv(nbytes, kDecTile);
  uint32_t *d_tile_cnt = nullptr, *d_cnt_tmp = nullptr, *d_cps = nullptr;
  uint8_t *d_cls = nullptr;
  for (int pass = 0; pass < 2; pass++) {
    d_tile_cnt = aa.take<uint32_t>(dec_tiles + 1);
    d_cnt_tmp = aa.take<uint32_t>(cdiv(dec_tiles, kScanTile) + 8);
    d_cps = aa.take<uint32_t>(nbytes + 1);
    d_cls = aa.take<uint8_t>(nbytes + 16);
    if (pass == 0) aa.commit();
  }
  aa.arm(st);
  WP_HIP(hipMemsetAsync(c->d_scalars, 0, sizeof(uint32_t) * kScalars, st));
  hipLaunchKernelGGL(decode_count_kernel<false>, dim3(dec_tiles), dim3(kBlock), 0, st, d_text, nbytes, d_tile_cnt,
                     reinterpret_cast<unsigned long long *>(c->d_scalars + kScalarInvalid), static_cast<uint32_t *>(nullptr));
  device_exclusive_scan(d_tile_cnt, d_tile_cnt, dec_tiles, d_cnt_tmp, c->d_scalars + kScalarCps, st, nullptr,
                        reinterpret_cast<unsigned long long *>(c->d_scalars + kScalarCps64));
  WP_LAUNCH_CHECK();
  fetch_scalars(c, kScalarCps64);
  unsigned long long n_text64;
  std::memcpy(&n_text64, c->h_scalars + kScalarCps64, sizeof(n_text64));
  // positions are 32-bit and bit 31 of an anchor entry is the skip flag of the sparse / long-word walk (walk.h,
  // kAnchorSkip): the same kind of limit as linear.cpp:104-106, never silent truncation
  if (n_text64 >= (1ull << 31)) throw std::length_error("64bit not implemented (fast path: text of 2^31 or more code points)");
  const size_t n_text = c->h_scalars[kScalarCps];
  unsigned long long dropped;
  std::memcpy(&dropped, c->h_scalars + kScalarInvalid, sizeof(dropped));
  if (dropped != 0) std::cerr << "WARNING Input contains invalid unicode characters." << std::endl;
  S.n_text = static_cast<int64_t>(n_text);
  S.n_total = static_cast<int64_t>(n_text);
  if (v->stage_timing) WP_HIP(hipEventRecord(c->ev[kMarkCounted], st));
  if (n_text == 0) return;

  Arena ar(&c->b_buf, aa.guard);
  const size_t tiles = cdiv(n_text, kScanTile), atiles = cdiv(n_text, kAnchorTile), walk_blocks = cdiv(n_text, kBlock);
  const bool staged_possible = !EnvOptions::get().sparse_emit && !v->sparse_emit;
  const uint32_t lw_cap = static_cast<uint32_t>(n_text / kMaxAnchorGap + 2);
  int32_t *d_emit = nullptr, *d_ids = nullptr, *d_lid = nullptr;
  uint32_t *d_anchors = nullptr, *d_anchor_cnt = nullptr, *d_anchor_tmp = nullptr, *d_emit_cnt = nullptr, *d_emit_tmp = nullptr,
           *d_blk_cnt = nullptr, *d_blk_off = nullptr, *jump_a = nullptr, *jump_b = nullptr, *d_lw_off = nullptr, *d_lw_fail = nullptr;
  uint8_t *d_mark = nullptr;
  LongWord *d_lw = nullptr;
  for (int pass = 0; pass < 2; pass++) {
    d_emit = ar.take<int32_t>(n_text + 1);
    d_ids = ar.take<int32_t>(n_text + 1);
    d_anchors = ar.take<uint32_t>(n_text + 1);
    d_anchor_cnt = ar.take<uint32_t>(atiles + 1);
    d_anchor_tmp = ar.take<uint32_t>(cdiv(atiles, kScanTile) + 8);
    d_emit_cnt = ar.take<uint32_t>(tiles + 1);
    d_emit_tmp = ar.take<uint32_t>(cdiv(walk_blocks, kScanTile) + 8);
    d_blk_cnt = ar.take<uint32_t>(walk_blocks + 2);
    d_blk_off = ar.take<uint32_t>(walk_blocks + 2);
    d_lid = ar.take<int32_t>(n_text + 1);
    jump_a = ar.take<uint32_t>(n_text + 1);
    jump_b = ar.take<uint32_t>(n_text + 1);
    d_mark = ar.take<uint8_t>(n_text + 1);
    d_lw = ar.take<LongWord>(lw_cap);
    d_lw_off = ar.take<uint32_t>(lw_cap + 1);
    d_lw_fail = ar.take<uint32_t>(lw_cap + 1);
    if (pass == 0) ar.commit();
  }
  ar.arm(st);
  hipLaunchKernelGGL(HIP_KERNEL_NAME(decode_write_kernel<uint32_t>), dim3(dec_tiles), dim3(kBlock), 0, st, d_text, nbytes,
                     d_tile_cnt, static_cast<const uint32_t *>(nullptr), static_cast<uint32_t *>(nullptr), d_cls, d_cps,
                     c->d_cls_bmp, static_cast<const uint32_t *>(nullptr), 0, static_cast<uint32_t *>(nullptr), 0);
  hipLaunchKernelGGL(fast_anchor_count_kernel, dim3(atiles), dim3(kBlock), 0, st, d_cls, n_text, d_anchor_cnt);
  device_exclusive_scan(d_anchor_cnt, d_anchor_cnt, atiles, d_anchor_tmp, c->d_scalars + kScalarAnchors, st);
  hipLaunchKernelGGL(fast_anchor_write_kernel, dim3(atiles), dim3(kBlock), 0, st, d_cls, n_text, d_anchor_cnt, d_anchors);
  hipLaunchKernelGGL(fast_anchor_gap_kernel, dim3(std::min<size_t>(atiles, 1024)), dim3(kBlock), 0, st, d_anchors,
                     c->d_scalars + kScalarAnchors, n_text, d_cls, c->d_scalars + kScalarAnchorGap);
  WP_LAUNCH_CHECK();
  fetch_scalars(c, kScalarAnchorGap);
  const size_t n_anchors = c->h_scalars[kScalarAnchors], max_gap = c->h_scalars[kScalarAnchorGap];
  S.n_anchors = static_cast<int64_t>(n_anchors);
  S.walk.max_anchor_gap = static_cast<int32_t>(max_gap);  // (wp_walk_stats: no wide walk here, and no lean kernel)
  if (v->stage_timing) WP_HIP(hipEventRecord(c->ev[kMarkSymbols], st));
  FastArgs fa{d_cps, d_cls, n_text,
              TrieView{c->d_trie_key, c->d_trie_child, c->d_trie_id, static_cast<uint32_t>(hv.trie_key.size() - 1)},
              c->d_tok_len, hv.unk_id, static_cast<uint32_t>(std::min<uint64_t>(static_cast<uint64_t>(hv.fast_max_len), n_text)),
              d_emit};
  // ids as per-workgroup lists (walk.h, StagedOut) unless the long-word kernels contribute ids of their own
  const bool staged = staged_possible && max_gap <= kMaxAnchorGap;
  if (!staged) WP_HIP(hipMemsetAsync(d_emit, 0x80, n_text * sizeof(int32_t), st));
  if (max_gap > kMaxAnchorGap) {  // long words: pointer doubling instead of one lane per word (walk.h)
    hipLaunchKernelGGL(fast_long_word_collect_kernel, dim3(std::min<size_t>(cdiv(std::max<size_t>(n_anchors, 1), kBlock), 2048)),
                       dim3(kBlock), 0, st, d_anchors, c->d_scalars + kScalarAnchors, n_text, d_cls, d_lw, lw_cap, c->d_scalars + kScalarLongWords);
    WP_LAUNCH_CHECK();
    const LongWordList lw = long_word_offsets(c, d_lw, lw_cap, d_lw_off, d_lw_fail, st);
    if (lw.nw > 0) {
      S.walk.n_long_words = static_cast<int64_t>(lw.nw);
      hipLaunchKernelGGL(fast_long_word_next_kernel, lw.grid(), dim3(kBlock), 0, st, fa, d_lw, d_lw_off, lw.nw, lw.total, d_lid, jump_a,
                         d_mark);
      WP_HIP(hipStreamSynchronize(st));  // lw.h_off is an upload source
      long_word_chains(lw, jump_a, jump_b, d_lid, d_mark, d_lw_off, d_lw_fail, st);
      hipLaunchKernelGGL(fast_long_word_emit_kernel, lw.grid(), dim3(kBlock), 0, st, fa, d_lw, d_lw_off, lw.nw, lw.total, d_lid, d_mark,
                         d_lw_fail);
      WP_LAUNCH_CHECK();
      S.anchor_mode = 2;
    }
  }
  const size_t acap = std::max<size_t>(n_anchors, 1);
  const unsigned wblocks = cdiv(acap, kBlock);
  if (staged) {
    const int words = kWbWords;
    const unsigned sblocks = cdiv(acap, static_cast<size_t>(words));
    hipLaunchKernelGGL(HIP_KERNEL_NAME(walk_balanced_kernel<FastArgs, FastStep, false>), dim3(sblocks), dim3(kBlock), 0, st, fa,
                       d_anchors, c->d_scalars + kScalarAnchors, acap, d_lid, d_blk_cnt,  // (d_lid: the long-word id buffer, idle here)
                       static_cast<const uint32_t *>(nullptr));
    device_exclusive_scan(d_blk_cnt, d_blk_off, sblocks, d_emit_tmp, c->d_scalars + kScalarIds, st);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(emit_gather_kernel<false>), dim3(sblocks), dim3(kBlock), 0, st, d_anchors,
                       c->d_scalars + kScalarAnchors, acap, d_lid, d_blk_cnt, d_blk_off, d_ids, words,
                       static_cast<const uint2 *>(nullptr), static_cast<uint2 *>(nullptr));
  } else {
    hipLaunchKernelGGL(fast_walk_kernel, dim3(wblocks), dim3(kBlock), 0, st, fa, d_anchors, c->d_scalars + kScalarAnchors, acap);
    hipLaunchKernelGGL(emit_count_kernel, dim3(tiles), dim3(kBlock), 0, st, d_emit, n_text, d_emit_cnt);
    device_exclusive_scan(d_emit_cnt, d_emit_cnt, tiles, d_emit_tmp, c->d_scalars + kScalarIds, st);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(emit_write_kernel<false>), dim3(tiles), dim3(kBlock), 0, st, d_emit, n_text, d_emit_cnt, d_ids,
                       static_cast<const uint2 *>(nullptr), static_cast<uint2 *>(nullptr));
  }
  S.staged_emit = staged ? 1 : 0;
  WP_LAUNCH_CHECK();
  if (v->stage_timing) WP_HIP(hipEventRecord(c->ev[kMarkWalked], st));
  if (ar.guard) {
    static const uint32_t init[2] = {0u, 0xffffffffu};
    WP_HIP(hipMemcpyAsync(c->d_scalars + kScalarGuard, init, sizeof(init), hipMemcpyHostToDevice, st));
    ar.check(st, c->d_scalars + kScalarGuard);
    aa.check(st, c->d_scalars + kScalarGuard);
    fetch_scalars(c, kScalarGuardFirst);
    if (c->h_scalars[kScalarGuardBad] != 0) throw HipError("arena guard: guard zone overwritten in the fast path");
    S.guard_zones = static_cast<int32_t>(ar.zones.size() + aa.zones.size());
  }
  fetch_scalars(c, kScalarIds);
  const size_t n_ids = c->h_scalars[kScalarIds];
  S.n_ids = static_cast<int64_t>(n_ids);
  if (v->stage_timing) {
    auto span = [&](int a, int b) {
      float ms = 0;
      WP_HIP(hipEventElapsedTime(&ms, c->ev[a], c->ev[b]));
      return static_cast<double>(ms);
    };
    S.ms_decode = span(kMarkStart, kMarkSymbols);
    S.ms_walk = span(kMarkSymbols, kMarkWalked);
    S.ms_total = span(kMarkStart, kMarkWalked) + S.ms_normalize;
  }
  c->d_ids = d_ids;
  *n_ids_out = n_ids;
}


}  // namespace wp
