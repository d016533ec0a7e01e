// linear_path.h — one encode of the Linear WordPiece path on one device context, stage by stage.
//
// Stages (reference file:line in parentheses):
//   decode + classes + alphabet   utils.cpp:37-79, utf8.cpp:54-90, linear.cpp:83-103        decode.h      encode_on_device
//   dense symbols, code, keys     linear.cpp:77-103                                          decode.h      symbols_and_keys
//   round 0 of the suffix sort    linear.cpp:118-141 (libsais_int)                           radix_sort.h  sort_round0
//   ranks, needed groups          linear.cpp:144-147 (inverse SA), prune.h                   suffix_array.h ranks_round0
//   refinement                    trie.h (default layout) / doubling rounds + LCP            local_sort.h  refine
//   who marks + 4 scanlines       linear.cpp:153-213                                         scanline.h    scanlines
//   greedy walk + id stream       linear.cpp:215-316                                         walk.h        walk
#pragma once
#include "context.h"
#include "local_sort.h"
#include "long_word_path.h"
#include "prune.h"
#include "trie.h"
#include "offsets.h"
#include "normalize.h"
#include "rows.h"
#include "walk.h"

namespace wp {

// The needed list of round 0 (prune.h) is sized from a guess (the handle remembers what the last encode needed); when
// a text needs more, the device keeps the list empty, reports the length it wanted, and the encode runs again with room.
struct ListOverflow {
  size_t wanted;
};

// The one kernel of this file, which is host code otherwise: it fuses kernels of scanline.h, trie.h and prune.h, and only
// here are all three in view.
// The per-token and per-group kernels between the late searches and the sort of the step starts in one launch (early
// refinement, key lookup): thread i does what group_starts_kernel does for group i, and what trie_token_range_kernel
// (in list space: trie_token_range_in_list), virtual_marks_kernel and piece_starts_kernel do for token i, one after the
// other in registers — four launches of one thread per token each were four links of a chain that is bound by launch
// latency.  No thread reads what another writes: a group's starts come from gfirst / ghead, a token's from its own range.
__global__ __launch_bounds__(kBlock) void token_marks_kernel(const uint32_t *__restrict__ node_of_entry, const uint32_t *__restrict__ tok_node,
                                                             const uint32_t *__restrict__ tok_subtree, int M, uint32_t *__restrict__ rng_lo,
                                                             uint32_t *__restrict__ rng_hi, const uint8_t *__restrict__ rng_long,
                                                             const uint32_t *__restrict__ tok_group, const uint32_t *__restrict__ ghead,
                                                             const uint32_t *__restrict__ gfirst, const uint32_t *__restrict__ totals, size_t n,
                                                             const int32_t *__restrict__ tok_id, const uint32_t *__restrict__ tok_info,
                                                             uint32_t *__restrict__ mslot, int32_t *__restrict__ mid, uint32_t *__restrict__ minfo,
                                                             int32_t *__restrict__ reach_fwd, int32_t *__restrict__ reach_bwd,
                                                             uint32_t *__restrict__ pstart, uint32_t *__restrict__ gend) {
  const int m = blockIdx.x * kBlock + threadIdx.x;
  const uint32_t last = static_cast<uint32_t>(n - 1);
  if (static_cast<uint32_t>(m) < totals[1]) {  // group m (at most one group per token): group_starts_kernel
    const uint32_t f = gfirst[m], e = f + (ghead[m + 1] - ghead[m]);
    uint32_t *tail = pstart + kStepsPerMark * static_cast<size_t>(M) + 1;
    tail[2 * static_cast<size_t>(m)] = f;
    tail[2 * static_cast<size_t>(m) + 1] = min(e, last);
    gend[m] = e;
  }
  if (m == 0) pstart[kStepsPerMark * static_cast<size_t>(M)] = 0;
  if (m >= M) return;
  uint32_t lo = rng_lo[m], hi = rng_hi[m];
  const uint32_t g = rng_long[m] ? tok_group[m] : kClaimNoGroup;
  if (g != kClaimNoGroup) {  // a long token with a group on the list: trie_token_range_kernel, in list space
    trie_token_range_in_list(node_of_entry, tok_node[m], tok_subtree[m], ghead[g], lo, hi);
    rng_lo[m] = lo;
    rng_hi[m] = hi;
  }
  const uint32_t reach = max(hi, lo);  // virtual_marks_kernel
  mslot[m] = lo;
  mid[m] = tok_id[m];
  minfo[m] = tok_info[m];
  reach_fwd[m] = static_cast<int32_t>(reach);
  reach_bwd[m] = static_cast<int32_t>(lo);
  uint32_t *o = pstart + kStepsPerMark * static_cast<size_t>(m);  // piece_starts_kernel
  o[0] = min(lo + 1u, last);
  o[1] = min(lo, last);
  o[2] = min(lo + 1u, last);
  o[3] = min(reach, last);
}

// The keys-only round 0 leaves the blank-start suffixes out only where the code's symbol histogram shows at least this
// share of blanks: the test of every key (builder and first pass) costs about as much as sorting a few percent fewer
// keys saves (config 2, 14.9 % blanks: 0.15 ms per step gained; config 5, 0.2 %: 1.5 % slower with the drop on).
constexpr double kBlankDropMinShare = 1.0 / 16;

// What the decode phase of encode_on_device hands to LinearPath.
struct DecodedText {
  const uint8_t *d_text;
  size_t nbytes;
  const uint32_t *d_tile_prefix;
  size_t n_text, n;  // code points of the text | symbols of S (the separator and, in the reference layout, the vocabulary behind them)
  uint32_t *d_cps;
  uint8_t *d_cls;
  int bits;
  bool text_only;
};

// One bucket index of a step table (scanline.h: StepTable bidx / bfast / shift).  A table has up to four, in this order:
// slot space and key space (key lookup), and for each an "_all" twin with fewer buckets where that makes another shift.
enum { kIxSlot = 0, kIxKey = 1, kIxSlotAll = 2, kIxKeyAll = 3, kStepIndexes = 4 };
struct BucketIndex {
  uint32_t *idx = nullptr;
  int2 *fast = nullptr;
  int shift = 0;         // (set for an absent index too: wp_step_stats reports all four)
  unsigned used = 0;     // buckets in use: slot space holds n_sorted <= n slots (scanlines())
  unsigned planned = 0;  // buckets the arena was planned for, from n; 0: absent (no key lookup, or a twin with the same shift)
  bool keyed = false;    // key space: a step inside a needed group answers kStepNeeded
  const uint32_t *starts = nullptr;  // the sorted step starts it indexes: slots, or their keys (scanlines())
};

template <typename SymT>
struct LinearPath : DecodedText {
  // ---- what the decode phase hands over (and DecodedText)
  const wp_vocab *v;
  Context *c;
  EncodeStats &S;
  Arena &ar, &aa;
  int offs_unit;  // offsets mode (wp_linear_encode_offsets): WP_OFFSETS_BYTES / WP_OFFSETS_CODE_POINTS; -1: ids only
  RowsCall *rows;  // a documents call (rows.h; offsets mode is on): the row structure is built behind the spans; else nullptr
  const NormMap *nmap;  // offsets mode on normalised text (normalize.h): d_text is the normalised copy, spans go back through this

  // ---- derived
  hipStream_t st, st2;
  const HostVocab &hv;
  bool full, prune, use_trie, key_lookup, keys_only, window_store, use_digit_bytes, staged_possible, sparse_emit;
  // keys_only: the needed groups are built from the candidate runs and refined beside the round-0 passes (ranks_round0,
  // "the early refinement"; WP_OPT_LATE_REFINE: behind the sort as before)
  bool early_refine;
  // key_lookup: the trie round's rank store writes a needed position's slot over its round-0 key (rank_out())
  bool rank_in_key;
  bool wide_ran = false;  // the walk took the wide branch: scalar 13 holds its count of words (wp_walk_stats)
  uint32_t need_depth;
  int M, P, P_cap, hb_n, win_mid;
  unsigned sl_tiles, sl_groups;
  BucketIndex bix[kStepIndexes];
  size_t radix_words, emit_tiles, walk_blocks, claim_size, list_cap;

  // ---- device buffers.  n-sized "slabs" of 4 bytes per symbol change roles from stage to stage (see plan()).
  SymT *d_sym = nullptr, *d_vsym = nullptr;
  Key0 *KA = nullptr, *KB = nullptr;           // round-0 keys, ping-pong (key_lookup: KA keeps them for the walk, X0 / KB ping-pong)
  uint32_t *VA = nullptr, *VB = nullptr;       // round-0 values (suffix starts), ping-pong (keys_only: the candidate list)
  uint32_t *X0 = nullptr, *X1 = nullptr;       // scratch pair of the rank store; walk stage: see walk()
  uint8_t *DG0 = nullptr, *DG1 = nullptr;      // digit bytes
  RankEntry *d_rank = nullptr;
  uint32_t *d_node_of_slot = nullptr;          // trie refinement: end node of the suffix in a slot of a needed group
  int32_t *d_lcp = nullptr;                    // reference layout / debug
  uint32_t *d_sa = nullptr, *d_gdepth = nullptr;
  RankEntry *d_hd_n = nullptr;                 // reference layout: round 0's rank entries in suffix order
  int32_t *d_emit = nullptr, *d_dbg_best = nullptr;
  int32_t *d_step_views = nullptr;  // WP_OPT_KEEP_DEBUG = 2: ids and lengths of the two classes by text position (walk.h, step_views_kernel)
  uint32_t *d_anchors = nullptr, *d_anchor_cnt = nullptr, *d_anchor_tmp = nullptr, *d_emit_cnt = nullptr, *d_emit_tmp = nullptr,
           *d_blk_cnt = nullptr, *d_blk_off = nullptr, *d_tile_scratch = nullptr;
  // list-sized (list_cap entries): the active list of the rounds and the large-group path
  uint32_t *AS0 = nullptr, *AS1 = nullptr, *AG = nullptr, *AD0 = nullptr, *AD1 = nullptr, *LA = nullptr, *LB = nullptr, *d_tdep = nullptr;
  uint64_t *LK0 = nullptr, *LK1 = nullptr, *LK2 = nullptr;  // sorted list keys | rank entries + scratch, large-list keys (and the widened round-0 keys), ping-pong
  uint32_t *LV0 = nullptr, *LV1 = nullptr, *LPOS = nullptr;
  uint32_t *d_ghead = nullptr, *d_gneed0 = nullptr, *d_gneed1 = nullptr, *d_lg_head = nullptr, *d_lg_off = nullptr;
  RerankAgg *d_agg = nullptr, *d_chunk_agg = nullptr;
  // vocabulary-sized
  uint32_t *d_claim = nullptr, *d_claim_need = nullptr, *d_gclaim = nullptr, *d_gfirst = nullptr, *d_gdep = nullptr, *d_gnode = nullptr,
           *d_gdone = nullptr, *d_rng_lo = nullptr, *d_rng_hi = nullptr, *d_child_sym = nullptr, *d_radix_tmp = nullptr,
           *d_radix_tmp2 = nullptr;  // (second: the large-group sort of the trie round runs on the side stream beside the rank store)
  uint8_t *d_rng_long = nullptr;
  uint32_t *d_mslot0 = nullptr, *d_mslot1 = nullptr, *d_midx0 = nullptr, *d_midx1 = nullptr, *d_minfo = nullptr, *d_tile_mlo = nullptr;
  int32_t *d_mid = nullptr, *d_rf = nullptr, *d_rb = nullptr, *d_cover_f = nullptr, *d_cover_b = nullptr;
  int32_t *d_tmin_f = nullptr, *d_tmin_b = nullptr, *d_gmin_f = nullptr, *d_gmin_b = nullptr, *d_pval_p = nullptr, *d_pval_s = nullptr;
  uint32_t *d_ps0 = nullptr, *d_ps1 = nullptr;
  // the step table in key space (scanline.h): starts, values (indices: bix); the ends of the needed groups
  uint32_t *d_gend = nullptr, *d_kstart = nullptr;
  int32_t *d_kval_p = nullptr, *d_kval_s = nullptr, *d_cover_tot = nullptr;
  uint8_t *d_kneed = nullptr;  // per step: its start lies inside a needed group (scanline.h, step_tables_kernel)
  // keys-only round 0 (decode.h, CandSet): the long-token key set, the runs of its slots in the sorted candidate list,
  // and per needed group the start of its run
  unsigned long long *d_cand_table = nullptr;
  uint32_t *d_cand_filter = nullptr, *d_cand_lo = nullptr, *d_cand_hi = nullptr, *d_gcand = nullptr;
  uint32_t *d_tok_group = nullptr;  // early refinement: per eligible token, the needed group that carries its key (prune.h)
  uint32_t *d_cand_bcnt = nullptr, *d_cand_boff = nullptr, *d_cand_scan = nullptr;  // per key-builder workgroup
  int cand_bits = 0;
  uint32_t *d_blank_bits = nullptr;  // keys-only round 0: which keys start with a blank (radix_sort.h, key_is_blank)
  // offsets mode: the spans of the walk (per stretch, walk.h), their compact list beside the id lists, the result,
  // and the first byte of every code point (byte unit)
  uint2 *d_ospill = nullptr, *d_cspan = nullptr, *d_offs = nullptr;
  uint32_t *d_byte_of = nullptr;
  // documents call: the starts of the lines (lines mode), the row splits, the start of every row in the offsets' unit
  long long *d_line_starts = nullptr, *d_row_splits = nullptr;
  uint32_t *d_row_base = nullptr;

  // ---- state handed from stage to stage
  SymbolCode code;
  DevCode dcode{};
  DigitBytes db;
  RadixPlan sort_plan;        // round-0 sort: set up ahead of it when the key builder takes its first histogram
  bool hist_in_keys = false;
  // keys-only round 0 drops the suffixes that start at a blank (the walk never looks them up): the sorted array and
  // slot space then hold n_sorted <= n suffixes; text-position arrays stay sized by n
  bool drop_blanks = false;
  size_t n_sorted = 0;
  int cur = 0, rounds = 1;
  Key0 *keys = nullptr, *other_keys = nullptr;
  uint32_t *vals = nullptr, *other_vals = nullptr, *slots = nullptr, *other_slots = nullptr, *adep = nullptr, *other_dep = nullptr;
  uint32_t *avals = nullptr, *spare_vals = nullptr;
  bool classified = false, anchors_queued = false;
  bool anchor_scalars_queued = false;  // the anchor scalars reach the host from the side stream, behind kEvAnchorScalars
  size_t n_act = 0, n_large = 0, n_large_groups = 0, n_groups = 0;
  // one per bucket index (an absent twin: its table again; no key lookup: empty).  The "_all" ones are for the kernels
  // that look up EVERY position of a stretch (scanlines())
  StepTable tables[kStepIndexes] = {};
  CandSet cand{};                    // keys_only: the set and the list the key builder appends to
  CandRuns cand_runs{};              // keys_only: the sorted list as the needed-group kernels read it
  size_t n_cand = 0;

  LinearPath(const wp_vocab *v_, Context *c_, EncodeStats &S_, Arena &ar_, Arena &aa_, const DecodedText &text, int offs_unit_,
             RowsCall *rows_ = nullptr, const NormMap *nmap_ = nullptr)
      : DecodedText(text), v(v_), c(c_), S(S_), ar(ar_), aa(aa_), offs_unit(offs_unit_), rows(rows_), nmap(nmap_), st(c_->stream),
        st2(c_->stream2), hv(v_->hv) {
    full = v->full_depth || hv.n_dup_eligible > 0 || v->lcp_kasai;
    need_depth = static_cast<uint32_t>(std::min<int64_t>(hv.longest + 1, 0x7fffffff));
    M = static_cast<int>(hv.elig_id.size());
    // round 0 only keeps the tied groups that carry the key of a long eligible token (prune.h)
    prune = !full && (M > 0 || text_only);
    // default layout: the needed groups are resolved along the token trie (trie.h) instead of by doubling rounds
    use_trie = text_only && !full && M > 0;
    // ... and the walk finds its steps by the round-0 key of a position, through rank[] only for the keys of needed
    // groups: no inverse suffix array for the whole text (scanline.h, "the step table in key space").  The debug views
    // (which keep LCPs) keep the full rank table.
    key_lookup = use_trie && !v->keep_debug && kKeyBits <= 32;
    // ... and then round 0 sorts the keys alone: the only suffixes whose position is read after it (the members of the
    // needed groups) come from the key builder's candidate list (decode.h, CandSet; WP_OPT_INDEXED_ROUND0: the
    // (key, index) sort as before)
    // 8-bit symbols only: with 32-bit symbols (config 3: 1 GB of mixed scripts, 120 k tokens) the list holds a third of
    // the suffixes and its test, packing and sort cost more than the value column (33.1 against 31.1 ms per step)
    keys_only = key_lookup && !v->indexed_round0 && sizeof(SymT) == 1;
    early_refine = keys_only && !v->late_refine;
    rank_in_key = key_lookup;
    sl_tiles = cdiv(n, kSlTile);
    sl_groups = cdiv(sl_tiles, kSlGroup);
    P = kStepsPerMark * M + 1;  // steps of the scanline result (scanline.h)
    P_cap = P + 2 * M + 2;      // ... and two per needed group (at most one group per eligible token) with key_lookup
    // buckets of the step table's index: about four per step (most lookups then end at the bucket entry, scanline.h)
    const int bucket_bits = std::min(kStepBucketBitsMax, std::max(kStepBucketBits, bit_length(4 * static_cast<size_t>(P))));
    const int bucket_shift = std::max(0, bit_length(n) - bucket_bits);
    // ... and a second index of 2^18 buckets (2 MB: stays in the L2) for the kernels that look up every position of a
    // long word, on the chain or not — their ranks spread over all slots, and 16 MB of entries miss the L2 (config 5:
    // 13.0 against 11.0 ms; the coverage rule's reach kernel, whose positions nearly all ARE visited, is faster on the
    // fine index: config 3, 9.3 against 9.8 ms)
    const int bucket_shift_all = std::max(0, bit_length(n) - kStepBucketBits);
    // the key-space indices: as many buckets, on the top bits of the key (entropy-coded: near-uniform)
    for (int i = 0; i < kStepIndexes; i++) {
      BucketIndex &b = bix[i];
      const int slot_shift = i >= kIxSlotAll ? bucket_shift_all : bucket_shift;
      const int kb = std::min(kKeyBits, std::max(1, bit_length(n - 1) - slot_shift));
      b.keyed = i == kIxKey || i == kIxKeyAll;
      b.shift = b.keyed ? kKeyBits - kb : slot_shift;
      const bool present = (!b.keyed || key_lookup) && (i < kIxSlotAll || b.shift != bix[i - 2].shift);
      if (present) b.planned = b.used = b.keyed ? 1u << kb : static_cast<unsigned>(((n - 1) >> slot_shift) + 1);
    }
    radix_words = std::max(radix_tmp_words<uint64_t>(n), radix_tmp_words<uint32_t>(std::max<size_t>(n, static_cast<size_t>(P_cap))));
    emit_tiles = cdiv(std::max<size_t>(n_text, 1), kScanTile);
    walk_blocks = cdiv(std::max<size_t>(n_text, 1), kBlock);  // (at most one anchor per position)
    sparse_emit = v->sparse_emit || EnvOptions::get().sparse_emit;
    // ids as per-workgroup lists (walk.h, StagedOut) unless several kernels contribute ids: decided here, except
    // for long words, which only the anchor gaps reveal
    staged_possible = !sparse_emit && !v->cover_anchors && hv.soft.empty();
    // digit bytes (radix_sort.h): the round-0 sort's histograms read 1 byte per key instead of the key
    use_digit_bytes = n > kRadixSmallN;
    claim_size = 1024;  // hash table of claimed key ranges (prune.h): a power of two >= 2 M
    while (claim_size < 2 * static_cast<size_t>(std::max(M, 1))) claim_size *= 2;
    cand_bits = bit_length(claim_size - 1);  // the long-token key set: as many slots (at most half of them taken)
    // Round 0 stores a rank for every position: a permutation.  From 2^22 symbols on the list is partitioned by ALL
    // destination bits above kWinBits (one or two radix passes over 8-byte records) and every 2^kWinBits-slot window of
    // the rank table is assembled in LDS and written with full-width stores (window_store_kernel).
    hb_n = bit_length(n - 1);
    window_store = n >= (1u << 22);
    // (more than 8 bits above the window: two passes of about half the bits each — with uniform digits the runs a
    // tile appends to its bins are 4096 / bins entries, and 16-entry runs leave the workgroup as half lines)
    win_mid = hb_n - kWinBits <= kRadixBits ? hb_n : kWinBits + (hb_n - kWinBits + 1) / 2;
    // room for the active list: every suffix where every tied group goes on (full depth, no pruning), else the handle's
    // memory of the last encode or an eighth of the text
    if (!prune) {
      list_cap = n;
    } else {
      const size_t guess = c->list_hint ? c->list_hint : n / 8;
      list_cap = std::min(n, guess + guess / 4 + 65536);
    }
    S.symbol_bits = bits;
    S.full_depth = full;
    S.trie_refine = use_trie ? 1 : 0;
    S.key_bits = kKeyBits;
    S.round0_keys_only = keys_only ? 1 : 0;
    S.round0_candidates = keys_only ? 0 : -1;
    n_sorted = n;
    S.round0_sorted = static_cast<int64_t>(n);
  }

  // st2 starts after everything queued on st so far / st continues after everything queued on st2
  void fork() {
    WP_HIP(hipEventRecord(c->evs[kEvFork], st));
    WP_HIP(hipStreamWaitEvent(st2, c->evs[kEvFork], 0));
  }
  void join() {
    WP_HIP(hipEventRecord(c->evs[kEvJoin], st2));
    WP_HIP(hipStreamWaitEvent(st, c->evs[kEvJoin], 0));
  }

  // ---- HBM layout (arena B) -------------------------------------------------------------------------------------
  // Per symbol, default layout with 8-bit symbols: sym 1, keys 4 + 4, values 4 + 4, digit bytes 1 + 1, rank-store
  // scratch 4 + 4, trie nodes by slot 4, id scratch 4, anchors 4 = 39 B, + ~80 B per entry of the active list
  // (an eighth of the text unless the last encode needed more) + vocabulary-sized tables.  The reference layout, the
  // debug views and the bounds-checking build add their own arrays, the rank table (4 B) among them: with the key
  // lookup the ranks of the needed list stand in KA, over their keys (rank_out()).  Roles of the n-sized slabs by stage:
  //   sort        KA/KB keys, VA/VB values
  //   rank store  X0/X1 first partition pass, (other values, keys) second, d_rank <- windows (no key lookup)
  //   walk        see walk(): ids, id lists, wide / long-word / coverage scratch in KA KB VA VB X0 X1
  void plan() {
    const bool ref = !text_only;                       // S = text . 1 . vocab: LCP-driven scanlines, doubling rounds
    const bool want_lcp = ref || v->keep_debug;        // (decided by flags, never by a pointer: the planning pass hands out nullptr)
    const size_t lc = list_cap, lg = lc / 2 + static_cast<size_t>(M) + 8;  // list entries, groups
    const size_t rr_tiles_l = cdiv(lc, kRrTile);
    const size_t rtiles = cdiv(std::max<size_t>(n_text, 1), kReachTile);
    for (int pass = 0; pass < 2; pass++) {
      d_sym = ar.take<SymT>(n + 16);
      KA = ar.take<Key0>(n + 16);
      KB = ar.take<Key0>(n + 16);
      VA = ar.take<uint32_t>(n + 16);
      VB = ar.take<uint32_t>(n + 16);
      X0 = ar.take<uint32_t>(n + 16);
      X1 = ar.take<uint32_t>(n + 16);
      DG0 = use_digit_bytes ? ar.take<uint8_t>(n + 64) : nullptr;
      DG1 = use_digit_bytes ? ar.take<uint8_t>(n + 64) : nullptr;
      // (key lookup: the ranks of the needed list go over their keys in KA, rank_out(); no kernel of the trie path
      // dereferences the table it is handed — its second keys are trie nodes)
      d_rank = (rank_in_key && kRankOverKey) ? nullptr : ar.take<RankEntry>(n);
      d_node_of_slot = use_trie ? ar.take<uint32_t>(n) : nullptr;
      d_lcp = want_lcp ? ar.take<int32_t>(n) : nullptr;  // (default layout: nothing reads LCPs)
      d_sa = (v->keep_debug || v->lcp_kasai) ? ar.take<uint32_t>(n) : nullptr;
      d_gdepth = (use_trie && !want_lcp) ? nullptr : ar.take<uint32_t>(n);  // group depths: the doubling rounds' (and the debug LCPs')
      d_hd_n = (want_lcp || !prune) ? ar.take<RankEntry>(n + 16) : nullptr;
      d_dbg_best = v->keep_debug ? ar.take<int32_t>(2 * n) : nullptr;
      d_emit = ar.take<int32_t>(n_text + 1);
      d_anchors = ar.take<uint32_t>(n_text + 1);
      d_anchor_cnt = ar.take<uint32_t>(emit_tiles + 1);
      d_anchor_tmp = ar.take<uint32_t>(cdiv(emit_tiles, kScanTile) + 8);
      d_emit_cnt = ar.take<uint32_t>(emit_tiles + 1);
      d_emit_tmp = ar.take<uint32_t>(cdiv(walk_blocks, kScanTile) + 8);  // (walk_blocks >= emit_tiles)
      d_blk_cnt = ar.take<uint32_t>(walk_blocks + 2);
      d_blk_off = ar.take<uint32_t>(walk_blocks + 2);
      d_tile_scratch = ar.take<uint32_t>(5 * (rtiles + 2) + 4 * (n_text / kMaxAnchorGap + 4));  // coverage tiles / long-word table
      // the active list
      AS0 = ar.take<uint32_t>(lc);
      AS1 = ar.take<uint32_t>(lc);
      AG = ar.take<uint32_t>(lc);
      AD0 = ar.take<uint32_t>(lc);
      AD1 = ar.take<uint32_t>(lc);
      LA = ar.take<uint32_t>(lc);
      LB = ar.take<uint32_t>(lc);
      d_tdep = ar.take<uint32_t>(lc + 2);
      LK0 = ar.take<uint64_t>(lc + 2);
      LK1 = ar.take<uint64_t>(lc + 2);
      LK2 = ar.take<uint64_t>(lc + 2);
      LV0 = ar.take<uint32_t>(lc);
      LV1 = ar.take<uint32_t>(lc);
      LPOS = ar.take<uint32_t>(lc + 16);
      d_ghead = ar.take<uint32_t>(lg);
      d_gneed0 = use_trie ? nullptr : ar.take<uint32_t>(lg);
      d_gneed1 = use_trie ? nullptr : ar.take<uint32_t>(lg);
      d_lg_head = ar.take<uint32_t>(lc / kLsMaxGroup + 4);
      d_lg_off = ar.take<uint32_t>(lc / kLsMaxGroup + 4);
      d_agg = ar.take<RerankAgg>(rr_tiles_l + 1);
      d_chunk_agg = ar.take<RerankAgg>(cdiv(rr_tiles_l, kRrChunk) + 1);
      d_radix_tmp = ar.take<uint32_t>(radix_words);
      // (keys_only: first the candidate sort — any length up to n — on the side stream beside round 0)
      d_radix_tmp2 = use_trie ? ar.take<uint32_t>(std::max(radix_tmp_words<uint64_t>(lc), keys_only ? radix_tmp_words<uint32_t>(n) : 0))
                              : nullptr;
      // vocabulary-sized
      d_claim = ar.take<uint32_t>(claim_size);
      if (keys_only) {  // the three tables that sort_candidates clears to 0, in one block: one memset
        uint32_t *zeroed = ar.take<uint32_t>(3 * claim_size);
        d_cand_lo = zeroed;
        d_cand_hi = zeroed ? zeroed + claim_size : nullptr;
        d_claim_need = zeroed ? zeroed + 2 * claim_size : nullptr;
      } else {
        d_claim_need = ar.take<uint32_t>(claim_size);
      }
      d_gclaim = ar.take<uint32_t>(M + 4);
      d_gfirst = ar.take<uint32_t>(M + 4);  // per needed group (at most one per long token): first slot,
      d_gdep = ar.take<uint32_t>(M + 4);    // depth (whole codewords of the key),
      d_gnode = ar.take<uint32_t>(M + 4);   // trie node its members share and the symbols behind it (trie.h)
      d_gdone = ar.take<uint32_t>(M + 4);
      d_rng_lo = ar.take<uint32_t>(M + 1);
      d_rng_hi = ar.take<uint32_t>(M + 1);
      d_rng_long = ar.take<uint8_t>(M + 1);
      d_vsym = use_trie ? ar.take<SymT>(hv.stream.size() + 16) : nullptr;
      d_child_sym = use_trie ? ar.take<uint32_t>(hv.lt_child_cp.size() + 1) : nullptr;
      d_mslot0 = ar.take<uint32_t>(M + 1);
      d_mslot1 = ar.take<uint32_t>(M + 1);
      d_midx0 = ar.take<uint32_t>(M + 1);
      d_midx1 = ar.take<uint32_t>(M + 1);
      d_mid = ar.take<int32_t>(M + 1);
      d_minfo = ar.take<uint32_t>(M + 1);
      d_rf = ar.take<int32_t>(M + 1);
      d_cover_f = ar.take<int32_t>(2 * static_cast<size_t>(M) + 2);
      d_cover_b = ar.take<int32_t>(2 * static_cast<size_t>(M) + 2);
      d_rb = ar.take<int32_t>(M + 1);
      d_cover_tot = ar.take<int32_t>(4 * cdiv(static_cast<size_t>(std::max(M, 1)), kCoverChunk));
      d_tile_mlo = ref ? ar.take<uint32_t>(sl_tiles + 2) : nullptr;
      d_tmin_f = ref ? ar.take<int32_t>(sl_tiles + 1) : nullptr;
      d_tmin_b = ref ? ar.take<int32_t>(sl_tiles + 1) : nullptr;
      d_gmin_f = ref ? ar.take<int32_t>(sl_groups + 1) : nullptr;
      d_gmin_b = ref ? ar.take<int32_t>(sl_groups + 1) : nullptr;
      d_ps0 = ar.take<uint32_t>(P_cap + 1);
      d_ps1 = ar.take<uint32_t>(P_cap + 1);
      d_pval_p = ar.take<int32_t>(P_cap + 1);
      d_pval_s = ar.take<int32_t>(P_cap + 1);
      for (BucketIndex &b : bix) {
        b.idx = b.planned ? ar.take<uint32_t>(static_cast<size_t>(b.planned) + 2) : nullptr;
        b.fast = b.planned ? ar.take<int2>(static_cast<size_t>(b.planned) + 1) : nullptr;
      }
      d_gend = key_lookup ? ar.take<uint32_t>(M + 4) : nullptr;
      d_kstart = key_lookup ? ar.take<uint32_t>(P_cap + 1) : nullptr;
      d_kval_p = key_lookup ? ar.take<int32_t>(P_cap + 1) : nullptr;
      d_kval_s = key_lookup ? ar.take<int32_t>(P_cap + 1) : nullptr;
      d_kneed = key_lookup ? ar.take<uint8_t>(P_cap + 1) : nullptr;
      d_cand_table = keys_only ? ar.take<unsigned long long>(claim_size) : nullptr;
      d_cand_filter = keys_only ? ar.take<uint32_t>(kCandFilterWords) : nullptr;
      d_gcand = keys_only ? ar.take<uint32_t>(M + 4) : nullptr;
      d_tok_group = keys_only ? ar.take<uint32_t>(M + 1) : nullptr;
      d_cand_bcnt = keys_only ? ar.take<uint32_t>(cdiv(n, kKeyTile) + 2) : nullptr;  // (the generic builder's tiles: the smaller)
      d_cand_boff = keys_only ? ar.take<uint32_t>(cdiv(n, kKeyTile) + 2) : nullptr;
      d_cand_scan = keys_only ? ar.take<uint32_t>(cdiv(cdiv(n, kKeyTile), kScanTile) + 8) : nullptr;
      d_blank_bits = keys_only ? ar.take<uint32_t>(kBlankWords) : nullptr;
      // offsets mode only (the ids-only layout is unchanged): 8 + 8 + 8 (+ 4 in bytes) B per text position
      const bool offs = offs_unit >= 0;
      d_ospill = offs ? ar.take<uint2>(n_text + 16) : nullptr;
      d_cspan = offs ? ar.take<uint2>(n_text + 16) : nullptr;
      d_offs = offs ? ar.take<uint2>(n_text + 1) : nullptr;
      // (normalised text: the spans go back to the source through nmap, byte_of[] is only needed for the rows)
      d_byte_of = ((offs_unit == WP_OFFSETS_BYTES && !nmap) || rows) ? ar.take<uint32_t>(n_text + 1) : nullptr;
      // documents call: 8 (+ 8 in lines mode, + 4 with offsets) B per row
      // (normalised text: explicit rows are carried from source bytes to normalised bytes into the same array)
      d_line_starts = (rows && (!rows->d_doc_off || nmap)) ? ar.take<long long>(rows->n_rows + 1) : nullptr;
      d_row_splits = rows ? ar.take<long long>(rows->n_rows + 1) : nullptr;
      d_row_base = (rows && rows->unit >= 0) ? ar.take<uint32_t>(rows->n_rows + 1) : nullptr;
      d_step_views = v->keep_step_views ? ar.take<int32_t>(4 * n_text + 4) : nullptr;
      if (pass == 0) ar.commit();
    }
    ar.arm(st);
  }

  // side stream: the anchor list (and the cleared emit array of the sparse id path) only need the class bytes; they
  // run next to the small latency-bound kernels of the scanline stage, not next to the radix passes (key_lookup: on
  // the main stream, next to the needed-group searches and the trie round of the side stream, ranks_round0)
  // behind_store: the rank store runs on another stream and sets kClsRanked in the class bytes (rank_flags()), which
  // anchor_write_kernel rewrites — that kernel waits for kEvRankStored; the count and the scan touch no class byte
  void launch_anchors(hipStream_t as, bool behind_store = false) {
    anchors_queued = true;
    const unsigned atiles = cdiv(n_text, kAnchorTile);
    if (!staged_possible) WP_HIP(hipMemsetAsync(d_emit, 0x80, n_text * sizeof(int32_t), as));
    hipLaunchKernelGGL(anchor_count_kernel, dim3(atiles), dim3(kBlock), 0, as, d_cls, static_cast<const uint8_t *>(nullptr),
                       n_text, d_anchor_cnt);
    device_exclusive_scan(d_anchor_cnt, d_anchor_cnt, atiles, d_anchor_tmp, c->d_scalars + kScalarAnchors, as);
    if (behind_store) WP_HIP(hipStreamWaitEvent(as, c->evs[kEvRankStored], 0));
    hipLaunchKernelGGL(anchor_write_kernel, dim3(atiles), dim3(kBlock), 0, as, d_cls, static_cast<const uint8_t *>(nullptr),
                       n_text, d_anchor_cnt, d_anchors);
    hipLaunchKernelGGL(anchor_gap_kernel, dim3(std::min<size_t>(atiles, 1024)), dim3(kBlock), 0, as, d_anchors,
                       c->d_scalars + kScalarAnchors, n_text, d_cls, hv.soft.empty() ? 1 : 0, c->d_scalars + kScalarAnchorGap);
    // The two scalars the host needs to queue the walk are final here.  On the side stream they travel at once, two words
    // alone (every earlier copy into the mirror has been waited for; the main stream queues none before the walk), so
    // that the walk is queued while the scanline kernels still wait in the main stream.  (On the main stream — the late
    // refinement of the key lookup — the side stream's copy of the list sizes may still be under way: walk() fetches.)
    if (as == st2) {
      static_assert(kScalarAnchorGap == kScalarAnchors + 1, "one copy takes both anchor scalars");
      queue_scalar_slots(c, kScalarAnchors, kScalarAnchorGap, as);
      WP_HIP(hipEventRecord(c->evs[kEvAnchorScalars], as));
      anchor_scalars_queued = true;
    }
  }

  // ---- S build: dense symbols, symbol code, round-0 keys (linear.cpp:77-103) -----------------------------------------
  void symbols_and_keys() {
    // alphabets > 255: the code covers symbol >> lo_bits (<= 256 values), the low bits follow verbatim
    const int lo_bits = sizeof(SymT) == 1 ? 0 : std::max(0, bits - 8);
    constexpr int kCodeReuse = 64;
    const bool reuse_code = c->code_cached && c->code_alphabet == static_cast<uint32_t>(S.alphabet) && c->code_bits == bits &&
                            c->code_lo == lo_bits && c->code_uses < kCodeReuse;
    if (!reuse_code) WP_HIP(hipMemsetAsync(c->d_symhist, 0, sizeof(uint32_t) * 256, st));
    // (8-bit symbols: lut[] of the blank code points, to find their share in the histogram below)
    constexpr uint32_t kBlankCpRuns[3][2] = {{0x09, 7}, {0x20, 2}, {kSpaceToken, 2}};  // first, words: lut[c .. c + words)
    uint32_t h_blank_lut[3][7] = {};
    hipLaunchKernelGGL(HIP_KERNEL_NAME(decode_write_kernel<SymT>), dim3(cdiv(nbytes, kDecTile)), dim3(kBlock), 0, st, d_text,
                       nbytes, d_tile_prefix, c->d_lut, d_sym, d_cls, d_cps, c->d_cls_bmp, c->d_soft,
                       static_cast<int>(hv.soft.size()), reuse_code ? nullptr : c->d_symhist, lo_bits);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(map_vocab_symbols_kernel<SymT>), dim3(cdiv(n - n_text, kBlock)), dim3(kBlock), 0, st,
                       c->d_stream, n_text, n, c->d_lut, d_sym);
    if (reuse_code) {
      code = c->code_cache;  // (the device tables still hold it)
      c->code_uses++;
    } else {
      // frequencies of symbol >> lo_bits -> optimal order-preserving code (host, <= 256 items) -> device tables
      std::vector<uint32_t> h32(256);
      WP_HIP(hipMemcpyAsync(h32.data(), c->d_symhist, sizeof(uint32_t) * 256, hipMemcpyDeviceToHost, st));
      if (sizeof(SymT) == 1) {
        for (int r = 0; r < 3; r++) {
          WP_HIP(hipMemcpyAsync(h_blank_lut[r], c->d_lut + kBlankCpRuns[r][0], sizeof(uint32_t) * kBlankCpRuns[r][1],
                                hipMemcpyDeviceToHost, st));
        }
      }
      WP_HIP(hipStreamSynchronize(st));
      const size_t nitems = (static_cast<size_t>(S.alphabet) >> lo_bits) + 1;  // dense symbols 0..sigma
      std::vector<uint64_t> freq(nitems);
      for (size_t i = 0; i < nitems; i++) freq[i] = h32[i];
      code = build_symbol_code(freq, bits, true);  // (falls back to a fixed width where no code of <= 12 bits exists)
      if (!code.uniform_bits) {
        code.lo_bits = lo_bits;
        code.avg_bits += lo_bits;
      }
      c->code_cache = code;
      c->code_cached = true;
      c->code_alphabet = static_cast<uint32_t>(S.alphabet);
      c->code_bits = bits;
      c->code_lo = lo_bits;
      c->code_uses = 0;
      // the blanks' share of the histogram: symbol s of a used code point c is lut[c] + 1 (lut[c + 1] != lut[c])
      uint64_t all = 0, blank = 0;
      for (size_t i = 0; i < nitems; i++) all += freq[i];
      if (sizeof(SymT) == 1) {
        for (int r = 0; r < 3; r++) {
          for (uint32_t k = 0; k + 1 < kBlankCpRuns[r][1]; k++) {
            const uint32_t cp = kBlankCpRuns[r][0] + k, s = h_blank_lut[r][k] + 1u;
            if (is_space(cp) && h_blank_lut[r][k + 1] != h_blank_lut[r][k] && s < nitems) blank += freq[s];
          }
        }
      }
      c->code_blank_share = all ? static_cast<double>(blank) / static_cast<double>(all) : 0.0;
      if (!code.uniform_bits) {
        const size_t blob_bytes = 512 + 256 + kDecodeTableBytes;
        std::memset(c->h_code, 0, blob_bytes);
        std::memcpy(c->h_code, code.cw.data(), code.cw.size() * sizeof(uint16_t));
        std::memcpy(c->h_code + 512, code.len.data(), code.len.size());
        std::memcpy(c->h_code + 768, code.bmask.data(), kDecodeTableBytes);
        WP_HIP(hipMemcpyAsync(c->d_code, c->h_code, blob_bytes, hipMemcpyHostToDevice, st));
      }
    }
    dcode = DevCode{reinterpret_cast<const uint16_t *>(c->d_code), c->d_code + 512, c->d_code + 768,
                    code.uniform_bits ? code.uniform_bits : -code.lo_bits};
    S.symbols_per_key = static_cast<int32_t>(kKeyBits / std::max(1.0, code.avg_bits));
    // 8-bit symbols with no codeword shorter than kKeys8MinLen bits (every ordinary text): the register form
    if (keys_only) {  // the long-token key set of this encode (prune.h); the builder's candidates go to VA / VB
      WP_HIP(hipMemsetAsync(d_cand_table, 0, claim_size * sizeof(unsigned long long), st));
      WP_HIP(hipMemsetAsync(d_cand_filter, 0, kCandFilterWords * sizeof(uint32_t), st));
      hipLaunchKernelGGL(long_key_set_kernel, dim3(cdiv(static_cast<size_t>(M) * kWave, kBlock)), dim3(kBlock), 0, st, c->d_stream,
                         c->d_elig_start, c->d_elig_info, M, c->d_lut, dcode, d_cand_table, cand_bits, d_cand_filter);
      cand.filter = d_cand_filter;
      cand.table = d_cand_table;
      cand.table_bits = cand_bits;
      cand.slot = VA;
      cand.pos = VB;
      cand.bcount = d_cand_bcnt;
    }
    size_t cand_blocks = 0;
    int min_len = code.uniform_bits ? code.uniform_bits : 99;
    for (uint8_t l : code.len) min_len = std::min<int>(min_len, l);
    if (sizeof(SymT) == 1 && min_len >= kKeys8MinLen) {
      cand.tile = kKeys8Tile;
      cand_blocks = cdiv(n, kKeys8Tile);
      if (n > kRadixSmallN) {  // its tiles are the tiles of the round-0 sort: the first digit's histogram comes along
        sort_plan = radix_plan<Key0>(n, d_radix_tmp, radix_words, st);
        hist_in_keys = true;
      }
      // keys alone and a histogram the builder takes: the sort may drop the blank-start suffixes (sort_round0) — where
      // they are common enough to pay for the blank test of every key in the builder and the first pass
      drop_blanks = keys_only && hist_in_keys && !v->sort_blanks && c->code_blank_share >= kBlankDropMinShare;
      if (drop_blanks) {
        hipLaunchKernelGGL(blank_bits_kernel, dim3(1), dim3(kBlankWords), 0, st, c->d_lut, dcode, d_blank_bits);
      }
      hipLaunchKernelGGL(build_keys0_u8_kernel, dim3(cdiv(n, kKeys8Tile)), dim3(kKeys8Threads), 0, st,
                         reinterpret_cast<const uint8_t *>(d_sym), n, dcode, KA, hist_in_keys ? nullptr : DG0,
                         hist_in_keys ? sort_plan.table : nullptr, hist_in_keys ? sort_plan.chunk_sums0 : nullptr, cand,
                         drop_blanks ? d_blank_bits : nullptr);
    } else {
      cand.tile = kKeyTile;
      cand_blocks = cdiv(n, kKeyTile);
      if (keys_only) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(build_keys0_kernel<SymT, true>), dim3(cdiv(n, kKeyTile)), dim3(kBlock), 0, st, d_sym, n,
                           dcode, KA, DG0, cand);
      } else {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(build_keys0_kernel<SymT, false>), dim3(cdiv(n, kKeyTile)), dim3(kBlock), 0, st, d_sym, n,
                           dcode, KA, DG0, cand);
      }
    }
    if (keys_only) {  // the list packed into X1 / trie nodes by slot on the side stream; the host learns its length while the sort runs
      WP_HIP(hipEventRecord(c->evs[kEvKeysBuilt], st));
      WP_HIP(hipStreamWaitEvent(st2, c->evs[kEvKeysBuilt], 0));
      device_exclusive_scan(d_cand_bcnt, d_cand_boff, cand_blocks, d_cand_scan, c->d_scalars + kScalarCand, st2);
      hipLaunchKernelGGL(cand_compact_kernel, dim3(cand_blocks), dim3(kBlock), 0, st2, VA, VB, d_cand_bcnt, d_cand_boff, cand.tile, n,
                         X1, d_node_of_slot);
      WP_HIP(hipMemcpyAsync(c->h_scalars + kScalarCand, c->d_scalars + kScalarCand, sizeof(uint32_t), hipMemcpyDeviceToHost, st2));
      WP_HIP(hipEventRecord(c->evs[kEvCandCount], st2));
    }
    WP_LAUNCH_CHECK();
  }

  // ---- round 0: 4 LSD passes over (key, suffix start) records (linear.cpp:121-141) ----------------------------------
  void sort_round0() {
    // (the low bits of a round-0 key are the tail of a compressed codeword stream: near-uniform digits)
    db.dg0 = DG0;
    db.dg1 = DG1;
    db.dg0_ready = DG0 != nullptr && !hist_in_keys;
    if (key_lookup) {  // (no rank store: the last pass leaves no digits; the keys go X0 <-> KB so that KA survives)
      Key0 *sk = reinterpret_cast<Key0 *>(X0);
      // drop_blanks: the first pass leaves the non-blank keys alone; the host learns their number (n_sorted) from its
      // spine, on the side stream while its scatter runs, and queues the later passes over them
      RadixDrop drop;
      drop.blank_bits = d_blank_bits;
      drop.d_kept = c->d_scalars + kScalarKept;
      drop.h_kept = c->h_scalars + kScalarKept;
      drop.side = st2;
      drop.spine_done = c->evs[kEvSpine];
      drop.copied = c->evs[kEvKept];
      cur = radix_sort_pairs<Key0>(sk, keys_only ? nullptr : VA, KB, keys_only ? nullptr : VB, n, 0, kKeyBits, d_radix_tmp, radix_words,
                                   st, &c->rstats, true, code.uniform_bits ? 0 : 8, db, true, hist_in_keys ? &sort_plan : nullptr, KA,
                                   drop_blanks ? &drop : nullptr);
      if (drop_blanks) n_sorted = drop.kept;
      S.round0_sorted = static_cast<int64_t>(n_sorted);
      S.hist_in_keys = hist_in_keys ? 1 : 0;
      keys = cur ? KB : sk;
      other_keys = cur ? sk : KB;
#ifdef WP_DEBUG_BOUNDS
      if constexpr (sizeof(Key0) == 4) {
        hipLaunchKernelGGL(sorted_check_kernel, dim3(std::min<size_t>(cdiv(n, kBlock), 1024)), dim3(kBlock), 0, st,
                           reinterpret_cast<const uint32_t *>(keys), n_sorted, reinterpret_cast<const uint32_t *>(KA), n, d_cls, n_text,
                           drop_blanks ? d_blank_bits : static_cast<const uint32_t *>(nullptr));
        hipLaunchKernelGGL(sorted_check_close_kernel, dim3(1), dim3(1), 0, st);
        WP_LAUNCH_CHECK();
      }
#endif
      vals = keys_only ? nullptr : (cur ? VB : VA);
      other_vals = keys_only ? nullptr : (cur ? VA : VB);
      if (keys_only) sort_candidates();
    } else {
      if (window_store) {  // the last pass leaves the first digit of the rank store's destination partition
        db.tail_bit = kWinBits;
        db.tail_mask = (1u << (win_mid - kWinBits)) - 1u;
        db.tail_from_val = true;
      }
      // histogram: one per-wave LDS counter per digit for the lowest digit (near-uniform), interleaved copies above it
      cur = radix_sort_pairs<Key0>(KA, VA, KB, VB, n, 0, kKeyBits, d_radix_tmp, radix_words, st, &c->rstats, true,
                                   code.uniform_bits ? 0 : 8, db, true, hist_in_keys ? &sort_plan : nullptr);
      S.hist_in_keys = hist_in_keys ? 1 : 0;
      keys = cur ? KB : KA;
      other_keys = cur ? KA : KB;
      vals = cur ? VB : VA;
      other_vals = cur ? VA : VB;
    }
    slots = AS0;
    other_slots = AS1;
    adep = AD0;
    other_dep = AD1;
    avals = LA;
    spare_vals = LB;
  }

  // The candidate list (X1 slots, trie nodes by slot: positions; both unused until the trie round) sorted by slot on the
  // side stream, beside the keys-only passes (a few percent of their bytes), and the run of every slot.  The host reads
  // the list length, known long before the queued passes end.  Ping-pong through VA / VB.
  void sort_candidates() {
    WP_HIP(hipEventSynchronize(c->evs[kEvCandCount]));
    n_cand = c->h_scalars[kScalarCand];
    S.round0_candidates = static_cast<int64_t>(n_cand);
    WP_HIP(hipMemsetAsync(d_cand_lo, 0, 3 * claim_size * sizeof(uint32_t), st2));  // (and d_cand_hi, d_claim_need: plan())
    const uint32_t *sorted_slot = X1, *sorted_pos = d_node_of_slot;
    if (n_cand > 1) {
      const int cc = radix_sort_pairs<uint32_t>(X1, d_node_of_slot, VA, VB, n_cand, 0, cand_bits, d_radix_tmp2,
                                                std::max(radix_tmp_words<uint64_t>(list_cap), radix_tmp_words<uint32_t>(n)), st2, nullptr,
                                                false, cand_bits, DigitBytes(), true);
      sorted_slot = cc ? VA : X1;
      sorted_pos = cc ? VB : d_node_of_slot;
    }
    if (n_cand > 0) {
      hipLaunchKernelGGL(cand_runs_kernel, dim3(cdiv(n_cand, kBlock)), dim3(kBlock), 0, st2, sorted_slot, n_cand, d_cand_lo, d_cand_hi);
    }
    WP_LAUNCH_CHECK();
    cand_runs.table = d_cand_table;
    cand_runs.bits = cand_bits;
    cand_runs.lo = d_cand_lo;
    cand_runs.hi = d_cand_hi;
    cand_runs.pos = sorted_pos;
  }

  // after every rerank: classify the new groups (large ones take the global path next round)
  // (runs on the side stream, next to the rank scatter)
  bool classify_groups(size_t list_len) {
    if (list_len <= static_cast<size_t>(kLsMaxGroup)) return false;  // no group can be large
    const size_t cap = list_len / 2 + 1;                              // a group has >= 2 entries
    clear_scalars(c, kScalarListLargeGroups, kScalarListLargeEntries, st2);
    hipLaunchKernelGGL(large_groups_kernel, dim3(std::min<size_t>(cdiv(cap, kBlock), 2048)), dim3(kBlock), 0, st2, d_ghead,
                       c->d_scalars + kScalarListGroups, reinterpret_cast<unsigned long long *>(c->d_scalars + kScalarListLargeGroups),
                       d_lg_head, d_lg_off);
    hipLaunchKernelGGL(large_groups_close_kernel, dim3(1), dim3(1), 0, st2, c->d_scalars + kScalarListLargeGroups, d_lg_off);
    return true;
  }

  // rank[dst[k]] = val[k] (val == nullptr: k) for a list of m entries.  Random 4-byte stores leave the L2s as partial
  // lines; from 4 M entries on, one radix pass over the top 8 bits of the destination first, and an XCD-aware scatter
  // after it, lets the stores of a workgroup fall into one ~1/256 window of the rank table.  t_dst / t_val: scratch.
  void store_ranks(uint32_t *dst, uint32_t *val, uint32_t *t_dst, uint32_t *t_val, size_t m) {
    if (val && m >= (1u << 22)) {
      const int hb = bit_length(n - 1);
      // (the top bits of a text position are uniformly distributed: histogram by LDS atomics)
      const int bc = radix_sort_pairs<uint32_t>(dst, val, t_dst, t_val, m, std::max(0, hb - 8), hb, d_radix_tmp, radix_words, st,
                                                nullptr, false, hb + 1, DigitBytes(), true);
      hipLaunchKernelGGL(scatter_pairs_kernel, dim3(cdiv(m, kSpTile)), dim3(kBlock), 0, st, bc ? t_dst : dst, bc ? t_val : val, m,
                         rank_out(), n, 1, rank_flags(), n_text);
    } else {
      hipLaunchKernelGGL(scatter_pairs_kernel, dim3(cdiv(m, kSpTile)), dim3(kBlock), 0, st, dst, val, m, rank_out(), n, 0, rank_flags(),
                         n_text);
    }
  }
  // Where the rank store writes.  Key lookup ("rank in the key's place", walk.h, step_at): over the round-0 key of the
  // position in KA — the only ranks anything reads are those of the needed list, whose keys answer kStepNeeded and are
  // never looked at again — with kClsRanked set in the position's class byte; there is no rank table.  The
  // bounds-checking build keeps the table and the keys and sets the flag alone (kRankOverKey).
  RankEntry *rank_out() const { return (rank_in_key && kRankOverKey) ? reinterpret_cast<RankEntry *>(KA) : d_rank; }
  uint8_t *rank_flags() const { return rank_in_key ? d_cls : nullptr; }

  // The rank store of round 0 at full size.  val == nullptr: the values are the slots themselves, made up by the first
  // pass.  The passes go through the scratch pairs a = (X0, X1) and b = (the value buffer the sort did not end in, the
  // sorted keys — free once the side stream's searches in them are over: keys_free).
  // dig: digit bytes of dst bits [kWinBits, ...), left by the last pass of the sort; other: the second byte buffer.
  void store_ranks_round0(uint32_t *dst, uint32_t *val, uint8_t *dig, uint8_t *other) {
    // (a per-device attribute: set on every call, the context may live on any device)
    WP_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(window_store_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               static_cast<int>(kWinLdsBytes)));
    uint32_t *a_dst = X0, *a_val = X1, *b_dst = other_vals, *b_val = reinterpret_cast<uint32_t *>(keys);
    DigitBytes d1;
    d1.dg0 = dig;
    d1.dg1 = other;
    d1.dg0_ready = dig != nullptr;
    if (win_mid < hb_n) {  // (the first pass leaves the second pass's digits)
      d1.tail_bit = win_mid;
      d1.tail_mask = (1u << (hb_n - win_mid)) - 1u;
    }
    // (the digits of both passes are position bits, uniform over 64..128 values: LDS atomics into interleaved copies)
    radix_sort_pairs<uint32_t>(dst, val, a_dst, a_val, n, kWinBits, win_mid, d_radix_tmp, radix_words, st, &c->rstats,
                               val == nullptr, 0, d1, true);
    keys_free();
    const uint32_t *f_dst = a_dst, *f_val = a_val;
    if (win_mid < hb_n) {
      DigitBytes d2;
      d2.dg0 = dig ? d1.tail_out(1) : nullptr;
      d2.dg1 = dig ? dig : nullptr;
      d2.dg0_ready = dig != nullptr;
      radix_sort_pairs<uint32_t>(a_dst, a_val, b_dst, b_val, n, win_mid, hb_n, d_radix_tmp, radix_words, st, &c->rstats, false, 0,
                                 d2);
      f_dst = b_dst;
      f_val = b_val;
    }
    start_trie_round();
    hipLaunchKernelGGL(window_store_kernel, dim3(cdiv(n, size_t(1) << kWinBits)), dim3(kWinThreads), kWinLdsBytes, st, f_dst, f_val,
                       n, d_rank);
  }

  // ---- the needed groups of a pruned round 0 (prune.h, trie.h): what the late and the early path share ----------------
  TokenTrie token_trie() const {
    return TokenTrie{c->d_lt_chain_len, c->d_lt_chain_off, c->d_lt_child_begin, c->d_lt_child_node, d_child_sym};
  }
  // early: the list is built before the sort ends, the groups' first slots are not known yet (refine_early)
  NeededList needed_list(bool early) const {
    return NeededList{slots, avals, AG, adep, d_ghead, early ? nullptr : d_gfirst, d_gdep,
                      reinterpret_cast<unsigned long long *>(c->d_scalars + kScalarList), static_cast<uint32_t *>(nullptr), need_depth,
                      d_claim_need, d_gclaim, d_gneed0, keys_only ? d_gcand : nullptr, keys_only ? cand_runs.pos : nullptr,
                      keys_only ? n_cand : 0};
  }
  void clear_claims() {
    WP_HIP(hipMemsetAsync(d_claim, 0xff, claim_size * sizeof(uint32_t), st2));
    if (!keys_only) WP_HIP(hipMemsetAsync(d_claim_need, 0, claim_size * sizeof(uint32_t), st2));  // (else: sort_candidates)
  }
  // the vocabulary stream and the trie's child labels as dense symbols of this encode's alphabet
  void map_trie_symbols() {
    const size_t ns = hv.stream.size(), nc = hv.lt_child_cp.size();
    hipLaunchKernelGGL(HIP_KERNEL_NAME(trie_map_symbols_kernel<SymT>), dim3(cdiv(std::max<size_t>(std::max(ns, nc), 1), kBlock)),
                       dim3(kBlock), 0, st2, c->d_stream, ns, c->d_lt_child_cp, nc, c->d_lut, d_vsym, d_child_sym);
  }
  // a list longer than its room is emptied and reported (ListOverflow); the closing entry of the group heads
  void close_needed_list() {
    hipLaunchKernelGGL(needed_list_clamp_kernel, dim3(1), dim3(1), 0, st2, c->d_scalars + kScalarList, static_cast<uint32_t>(list_cap),
                       c->d_scalars + kScalarListWanted);
    hipLaunchKernelGGL(needed_list_close_kernel, dim3(1), dim3(1), 0, st2, c->d_scalars + kScalarList, d_ghead);
  }

  // Depth-capped mode, behind the sort: the groups that have to go on are found from the vocabulary (prune.h) and
  // appended to the active list by the kernel that finds them — on the side stream (a few thousand waves of searches).
  void enqueue_needed_groups() {
    clear_claims();
    const NeededList nl = needed_list(false);
    if (use_trie) map_trie_symbols();
    if (M > 0) {  // (no eligible token at all: every tied group retires)
      hipLaunchKernelGGL(HIP_KERNEL_NAME(need_groups_kernel<SymT>), dim3(cdiv(static_cast<size_t>(M) * kWave, kBlock)),
                         dim3(kBlock), 0, st2, keys, vals, n_sorted, n, d_sym, c->d_stream, c->d_elig_start, c->d_elig_info, M, c->d_lut, dcode,
                         d_claim, static_cast<uint32_t>(claim_size - 1), nl, text_only ? d_rng_lo : nullptr, d_rng_hi, d_rng_long,
                         cand_runs);
    }
    close_needed_list();
    if (key_lookup) {  // (the group heads are overwritten by the trie round: the group ends are taken now)
      hipLaunchKernelGGL(group_starts_kernel, dim3(cdiv(M, kBlock)), dim3(kBlock), 0, st2, d_gfirst, d_ghead, c->d_scalars + kScalarList,
                         n_sorted, d_ps0 + P, d_gend);
    }
    if (M > 0) {
      if (!use_trie) hipLaunchKernelGGL(needed_need_kernel, dim3(cdiv(M, kBlock)), dim3(kBlock), 0, st2, nl);
      hipLaunchKernelGGL(needed_fill_kernel, dim3(1024), dim3(kBlock), 0, st2, nl, vals, n_sorted);
      if (use_trie) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(trie_group_start_kernel<SymT>), dim3(cdiv(M, kBlock)), dim3(kBlock), 0, st2, vals,
                           keys_only ? cand_runs.pos : nullptr, d_gcand, d_gfirst,
                           d_gdep, c->d_scalars + kScalarList, d_sym, n, d_vsym, token_trie(), d_gnode, d_gdone);
      }
    }
    // (from here on the side stream no longer reads the sorted keys and suffixes: the rank store may reuse them)
    WP_HIP(hipEventRecord(c->evs[kEvKeysFree], st2));
    if (use_trie) trie_round_sizes();
  }
  // pair b of the rank store holds the sorted keys: the side stream's searches in them must be over
  void keys_free() {
    if (prune) WP_HIP(hipStreamWaitEvent(st, c->evs[kEvKeysFree], 0));
  }
  // The trie round (side stream) starts when the partition passes are through: its small latency-bound kernels run
  // beside the window store — beside the radix passes they took a quarter of the passes' bandwidth for the same gain.
  void start_trie_round() {
    if (!use_trie) return;
    WP_HIP(hipEventRecord(c->evs[kEvPartition], st));
    WP_HIP(hipStreamWaitEvent(st2, c->evs[kEvPartition], 0));
    trie_round_sort();
  }

  // ---- behind the sort: which tied groups go on (side stream), and the inverse suffix array (linear.cpp:144-147) ----
  void ranks_round0() {
    if (early_refine) {
      refine_early();
    } else if (key_lookup) {
      refine_late_by_key();
    } else {
      rank_all_round0();
    }
  }

  // No rank store: the needed-group searches and the trie round (side stream) are the critical path now, and the
  // anchor list (main stream: class bytes only) runs beside them.  The trie round stores a rank for every entry
  // of the needed list — the only ranks anything reads (walk.h, step_value).
  void refine_late_by_key() {
    fork();
    enqueue_needed_groups();
    trie_round_sort();
    if (n_text > 0) launch_anchors(st);
    WP_LAUNCH_CHECK();
    trie_round_finish();
  }

  // The rank store: a rank for every suffix, beside the needed groups of a pruned round 0 or with every tied group on the list.
  void rank_all_round0() {
    // Default layout: nobody asks for a group's head or depth — the step functions change at boundaries between
    // distinct keys only (short tokens) or inside needed groups (long tokens, resolved by the trie round, which stores
    // every rank it touches) — so a suffix's own slot serves as its rank and no kernel derives group heads.
    const bool slot_ranks = text_only && !d_lcp;
    uint8_t *dig = DG0 ? db.tail_out(cur) : nullptr, *dig_other = DG0 ? db.tail_out(cur ^ 1) : nullptr;
    if (prune) {
      // (the searches start when the sort ends, beside the first partition pass's histogram: started beside its scatter
      // instead, which is bandwidth-bound, they cost the scatter more than they cost the histogram now — measured)
      fork();
      enqueue_needed_groups();
      if (!slot_ranks) {  // reference layout: rank entries, LCPs and group depths from the sorted keys
        hipLaunchKernelGGL(round0_rank_kernel<true>, dim3(cdiv(n, kR0Tile)), dim3(kBlock), 0, st, keys, vals, n, dcode.first_len,
                           dcode.uniform_bits, d_sa, d_hd_n, d_lcp, d_gdepth);
      }
    } else {
      // every tied group goes on (true suffix array, or no pruning possible): the count / prefix / apply kernels take
      // 64-bit keys, the 32-bit round-0 keys are widened into the large-list key buffer (free during round 0)
      const DepthRule rule{need_depth, full ? 1 : 0, nullptr, nullptr, 0, nullptr};
      const unsigned tiles = cdiv(n, kRrTile);
      hipLaunchKernelGGL(widen_keys_kernel, dim3(std::min<size_t>(cdiv(n, kBlock), 8192)), dim3(kBlock), 0, st, keys, LK2, n);
      hipLaunchKernelGGL(HIP_KERNEL_NAME(rerank_agg_kernel<true>), dim3(tiles), dim3(kBlock), 0, st, LK2, vals, n,
                         static_cast<const uint32_t *>(nullptr), static_cast<const RankEntry *>(nullptr),
                         static_cast<const uint32_t *>(nullptr), n, dcode.first_len, dcode.uniform_bits, rule, d_tdep, d_agg);
      hipLaunchKernelGGL(rerank_chunk_kernel, dim3(cdiv(tiles, kRrChunk)), dim3(kBlock), 0, st, d_agg, tiles, d_chunk_agg);
      hipLaunchKernelGGL(rerank_prefix_kernel, dim3(cdiv(tiles, kRrChunk)), dim3(kBlock), 0, st, d_agg, d_chunk_agg, tiles);
      hipLaunchKernelGGL(HIP_KERNEL_NAME(rerank_apply_kernel<SymT, true>), dim3(tiles), dim3(kBlock), 0, st, LK2, vals,
                         static_cast<const uint32_t *>(nullptr), static_cast<const uint32_t *>(nullptr), d_tdep, n, d_agg, d_sym, n,
                         dcode.first_len, dcode.uniform_bits, rule, d_sa, d_hd_n, d_lcp, slots, avals, AG, adep, d_ghead, d_gdepth,
                         c->d_scalars + kScalarList);
    }
    uint32_t *rank_vals = slot_ranks ? nullptr : reinterpret_cast<uint32_t *>(d_hd_n);
    if (window_store) {
      store_ranks_round0(vals, rank_vals, dig, dig_other);
    } else {
      keys_free();
      start_trie_round();
      store_ranks(vals, rank_vals, X0, X1, n);
    }
    WP_LAUNCH_CHECK();
    if (use_trie) {
      trie_round_finish();
    } else {
      if (prune) join();
      fork();
      classified = classify_groups(std::min(n, list_cap));
      join();
    }
  }

  // ---- keys-only round 0: the refinement beside the sort ("early refinement") -------------------------------------------
  // The members of every needed group are known when the candidate list is sorted by slot (sort_candidates), while the
  // second of the four passes over the keys still runs: a group is the run of its key's slot, its size the run length,
  // its members' positions cand_pos.  The sorted keys add one number per group, its first slot — an additive base.  So
  // the side stream builds the list, sends its sizes to the host and runs the whole trie round (which reads neither a
  // rank nor a sorted key) in LIST SPACE beside the remaining passes: an entry's provisional slot is its list position,
  // and whatever the round indexes by slot (slots, the trie nodes by slot, the rank entries) is indexed by list position.
  // Behind the last pass only the slot-dependent tail is left, on the main stream: the searches in the sorted keys
  // (every token's range, every group's first slot), the group starts of the step table, and the rank scatter, which
  // adds gfirst[g] - ghead[g] to every entry while it reads (token_marks_kernel does the same for the ranges).
  // The streams are ordered by events alone.  The anchor list goes to the side stream behind the round and behind the
  // sort (kEvSorted): beside the tail and the scanline stage, not beside the passes.
  void refine_early() {
    clear_claims();
    const NeededList nl = needed_list(true);
    const unsigned tok_blocks = cdiv(static_cast<size_t>(M) * kWave, kBlock);
    map_trie_symbols();
    // (a long token's table slot, run length and state wait in its cells of rng_lo / rng_hi / rng_long for the late half)
    hipLaunchKernelGGL(HIP_KERNEL_NAME(need_groups_early_kernel<SymT>), dim3(tok_blocks), dim3(kBlock), 0, st2, n, d_sym, c->d_stream,
                       c->d_elig_start, c->d_elig_info, M, c->d_lut, dcode, d_claim, nl, d_rng_lo, d_rng_hi, d_rng_long, cand_runs);
    close_needed_list();
    hipLaunchKernelGGL(needed_fill_kernel, dim3(1024), dim3(kBlock), 0, st2, nl, static_cast<const uint32_t *>(nullptr), n_sorted);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(trie_group_start_kernel<SymT>), dim3(cdiv(M, kBlock)), dim3(kBlock), 0, st2,
                       static_cast<const uint32_t *>(nullptr), cand_runs.pos, d_gcand, static_cast<const uint32_t *>(nullptr), d_gdep,
                       c->d_scalars + kScalarList, d_sym, n, d_vsym, token_trie(), d_gnode, d_gdone);
    WP_HIP(hipEventRecord(c->evs[kEvListBuilt], st2));  // (the late half may overwrite the tokens' cells from here on)
    trie_round_sizes();
    trie_round_sort();
    S.sched.early = 1;
    // main stream, behind the last pass: the late half of the searches (the group starts follow in token_marks_kernel,
    // scanlines(): they read the group table and its sizes, which nothing writes after the list is built — the round's
    // own totals go elsewhere, trie_round_finish)
    WP_HIP(hipEventRecord(c->evs[kEvSorted], st));
    WP_HIP(hipStreamWaitEvent(st, c->evs[kEvListBuilt], 0));
    hipLaunchKernelGGL(need_ranges_kernel, dim3(tok_blocks), dim3(kBlock), 0, st, keys, n_sorted, c->d_stream, c->d_elig_start,
                       c->d_elig_info, M, c->d_lut, dcode, d_claim, d_gfirst, d_rng_lo, d_rng_hi, d_rng_long, d_tok_group);
    WP_LAUNCH_CHECK();
    trie_round_finish();
  }

  // ---- trie refinement of the needed groups (trie.h), on the side stream BESIDE the window store of the rank store ----
  // Nothing in it reads a rank: every entry of the needed list walks the token trie (its end node is its sort key),
  // the groups are sorted by node (LDS windows; large groups through a radix sort with its own temporary), one split
  // assigns the new slots.  Only the last step — the ranks of the entries that moved — has to wait for the rank table.
  // The list sizes travel to the host as soon as the list is built, so every launch is queued long before it can run.
  int trie_rb() const { return bit_length(hv.lt_chain_len.size() + 1); }  // second keys: 1 + trie node
  void trie_round_sizes() {
    classified = classify_groups(list_cap);  // (side stream: the table of large groups)
    queue_scalars(c, kScalarAnchorGap, st2);
    WP_HIP(hipEventRecord(c->evs[kEvScalars], st2));
  }
  void trie_round_sort() {
    // (sizes are read on the device: the launches do not wait for the host to learn them)
    hipLaunchKernelGGL(HIP_KERNEL_NAME(trie_walk_kernel<SymT>), dim3(std::min<size_t>(cdiv(list_cap, kBlock), 16384)), dim3(kBlock), 0,
                       st2, avals, AG, d_gnode, d_gdone, c->d_scalars + kScalarList, d_sym, n, d_vsym, token_trie(), adep);
    WP_HIP(hipEventRecord(c->evs[kEvTrieNodes], st2));  // (the large-group path starts from here, beside the LDS sort: trie_round_finish)
    hipLaunchKernelGGL(local_sort_kernel, dim3(cdiv(list_cap, kLsT)), dim3(kBlock), 0, st2, avals, AG, adep, c->d_scalars + kScalarList,
                       d_ghead, d_rank, n, trie_rb(), LK0, spare_vals, adep);
  }
  // wp_refine_stats: the list of the first refinement round as the host has just learnt it, and what it is sorted with
  void refine_stats(size_t groups, int rbits) {
    S.refine.n_groups = static_cast<int64_t>(groups);
    S.refine.n_entries = static_cast<int64_t>(n_act);
    S.refine.n_large_groups = static_cast<int64_t>(n_large_groups);
    S.refine.n_large_entries = static_cast<int64_t>(n_large);
    S.refine.trie_nodes = static_cast<int64_t>(hv.lt_chain_len.size());
    S.refine.sort_bits = rbits;
    S.refine.key_lookup = key_lookup ? 1 : 0;
    S.refine.symbol_bytes = static_cast<int32_t>(sizeof(SymT));
  }
  void trie_round_finish() {
    WP_HIP(hipEventSynchronize(c->evs[kEvScalars]));
    n_act = c->h_scalars[kScalarListEntries];
    n_groups = c->h_scalars[kScalarListGroups];
    n_large_groups = classified ? c->h_scalars[kScalarListLargeGroups] : 0;
    n_large = classified ? c->h_scalars[kScalarListLargeEntries] : 0;
    // (an overflowing list was kept empty: nothing ran on it)
    if (c->h_scalars[kScalarListWanted] > list_cap) throw ListOverflow{c->h_scalars[kScalarListWanted]};
    S.active_per_round[0] = static_cast<int64_t>(n);
    refine_stats(n_groups, trie_rb());
    uint64_t *skeys = LK0;
    RankEntry *hd = reinterpret_cast<RankEntry *>(LK1);
    if (n_act > 0) {
      S.active_per_round[1] = static_cast<int64_t>(n_act);
      const int rb = trie_rb();
      if (n_large > 0) {  // (second side stream: other list positions than the LDS sort's, scratch of its own)
        hipStream_t st3 = c->stream3;
        WP_HIP(hipStreamWaitEvent(st3, c->evs[kEvTrieNodes], 0));
        const int lgb = bit_length(n_large_groups > 0 ? n_large_groups - 1 : 0);
        hipLaunchKernelGGL(large_extract_kernel, dim3(cdiv(cdiv(n_large, kLxSpan), kBlock / kWave)), dim3(kBlock), 0, st3, avals, adep,
                           d_lg_head, d_lg_off, static_cast<uint32_t>(n_large_groups), n_large, d_rank, n, rb, LK1, LV0, LPOS, adep);
        const int lc = radix_sort_pairs<uint64_t>(LK1, LV0, LK2, LV1, n_large, 0, rb + lgb, d_radix_tmp2,
                                                  radix_tmp_words<uint64_t>(list_cap), st3, nullptr);
        hipLaunchKernelGGL(large_writeback_kernel, dim3(std::min<size_t>(cdiv(n_large, kBlock), 8192)), dim3(kBlock), 0, st3,
                           lc ? LK2 : LK1, lc ? LV1 : LV0, LPOS, n_large, AG, rb, skeys, spare_vals);
        WP_HIP(hipEventRecord(c->evs[kEvLargeSorted], st3));
        WP_HIP(hipStreamWaitEvent(st2, c->evs[kEvLargeSorted], 0));
      }
      DepthRule rrule{need_depth, 0, nullptr, nullptr, 1, d_node_of_slot};  // final round: every group retires
      const unsigned tiles = cdiv(n_act, kRrTile);
      hipLaunchKernelGGL(HIP_KERNEL_NAME(rerank_agg_kernel<false>), dim3(tiles), dim3(kBlock), 0, st2, skeys, spare_vals, n_act, adep,
                         d_rank, d_gdepth, n, dcode.first_len, dcode.uniform_bits, rrule, d_tdep, d_agg);
      hipLaunchKernelGGL(rerank_chunk_kernel, dim3(cdiv(tiles, kRrChunk)), dim3(kBlock), 0, st2, d_agg, tiles, d_chunk_agg);
      hipLaunchKernelGGL(rerank_prefix_kernel, dim3(cdiv(tiles, kRrChunk)), dim3(kBlock), 0, st2, d_agg, d_chunk_agg, tiles);
      hipLaunchKernelGGL(HIP_KERNEL_NAME(rerank_apply_kernel<SymT, false>), dim3(tiles), dim3(kBlock), 0, st2, skeys, spare_vals, slots,
                         adep, d_tdep, n_act, d_agg, d_sym, n, dcode.first_len, dcode.uniform_bits, rrule, d_sa, hd, d_lcp,
                         other_slots, avals, AG, other_dep, d_ghead, d_gdepth,
                         c->d_scalars + (early_refine ? kScalarSplitTotals : kScalarList));  // (early: token_marks_kernel still reads the sizes)
    }
    if (early_refine) {  // the main stream goes on behind the round; the anchor list follows it on the side stream, behind the sort
      WP_HIP(hipEventRecord(c->evs[kEvRoundDone], st2));
      WP_HIP(hipStreamWaitEvent(st, c->evs[kEvRoundDone], 0));
      // (the store is queued first: the side stream's anchor_write_kernel waits for the event behind it)
      if (n_act > 0) {  // hd: list positions of the subgroup heads; the scatter moves them to the group's slots
        if (n_act >= (1u << 22)) {
          hipLaunchKernelGGL(list_rank_base_kernel, dim3(cdiv(n_act, kBlock)), dim3(kBlock), 0, st, hd, AG, d_gfirst, d_ghead, n_act);
          store_ranks(spare_vals, hd, reinterpret_cast<uint32_t *>(hd) + list_cap + 2, reinterpret_cast<uint32_t *>(skeys), n_act);
        } else {
          hipLaunchKernelGGL(scatter_list_ranks_kernel, dim3(cdiv(n_act, kBlock)), dim3(kBlock), 0, st, spare_vals, hd, AG, d_gfirst,
                             d_ghead, n_act, rank_out(), n, rank_flags(), n_text);
        }
        rounds = 2;
      }
      if (n_text > 0) {
        const bool flags_stored = n_act > 0 && rank_flags() != nullptr;
        if (flags_stored) WP_HIP(hipEventRecord(c->evs[kEvRankStored], st));
        WP_HIP(hipStreamWaitEvent(st2, c->evs[kEvSorted], 0));
        launch_anchors(st2, flags_stored);
      }
      WP_LAUNCH_CHECK();
      return;
    }
    join();  // the rank table is complete (main stream) and the new ranks are known (side stream)
    if (n_act > 0) {
      store_ranks(spare_vals, hd, reinterpret_cast<uint32_t *>(hd) + list_cap + 2, reinterpret_cast<uint32_t *>(skeys), n_act);
      rounds = 2;
    }
    WP_LAUNCH_CHECK();
  }

  // Between two rounds the host needs the new list sizes (grids, large-group path).  The copy of the scalars and the
  // LDS segmented sort of the next round are queued first — the sort reads its sizes on the device and gets a grid for
  // the largest possible list — and only then does the host wait for the copy: the round trip hides behind the sort.
  void next_round_begin(size_t upper, int rb) {
    queue_scalars(c, kScalarAnchorGap, st);
    WP_HIP(hipEventRecord(c->evs[kEvScalars], st));
    fork();  // the large-group path of the next round (side stream) may start from here
    if (upper > 0) {
      hipLaunchKernelGGL(local_sort_kernel, dim3(cdiv(upper, kLsT)), dim3(kBlock), 0, st, avals, AG, adep, c->d_scalars + kScalarList, d_ghead,
                         d_rank, n, rb, LK0, spare_vals, static_cast<const uint32_t *>(nullptr));
    }
    WP_HIP(hipEventSynchronize(c->evs[kEvScalars]));
    n_act = c->h_scalars[kScalarListEntries];
    n_large_groups = classified ? c->h_scalars[kScalarListLargeGroups] : 0;
    n_large = classified ? c->h_scalars[kScalarListLargeEntries] : 0;
    // (an overflowing list was kept empty: nothing ran on it)
    if (c->h_scalars[kScalarListWanted] > list_cap) throw ListOverflow{c->h_scalars[kScalarListWanted]};
  }

  // ---- rounds >= 1 over the active list --------------------------------------------------------------------------
  // Default layout: ONE split — every entry's second key is the trie node its suffix ends in (trie.h), all groups
  // retire — run beside the rank store (trie_round_begin / _finish).  Reference layout / full depth: prefix
  // doubling, a group sorted by rank[i + depth(group)] per round (doubling_rounds).
  void refine() {
    if (!use_trie) doubling_rounds();  // (trie refinement has run beside the rank store: trie_round_begin / _finish)
    S.rounds = rounds;
    // every tie that is left shares at least this many symbols: need_depth for the groups that went through the
    // rounds, the shortest possible key (whole codewords in kKeyBits bits) for the groups round 0 let go
    const int max_len = code.uniform_bits ? code.uniform_bits : kMaxCodeLen + code.lo_bits;
    const int32_t key_syms = std::max(1, kKeyBits / max_len);
    S.sorted_depth = full ? 0x7fffffff
                          : (prune ? std::min<int32_t>(static_cast<int32_t>(need_depth), key_syms) : static_cast<int32_t>(need_depth));
    S.needed_after_round0 = prune ? (rounds > 1 ? S.active_per_round[1] : 0) : -1;
    if (prune && rounds > 1) c->list_hint = static_cast<size_t>(S.active_per_round[1]);
  }

  void doubling_rounds() {
    const int rb = bit_length(n);  // second keys of a round: 1 + rank (<= n)
    const DepthRule rule{need_depth, full ? 1 : 0, nullptr, nullptr, 0, nullptr};
    next_round_begin(std::min(n, list_cap), rb);
    S.active_per_round[0] = static_cast<int64_t>(n);
    refine_stats(c->h_scalars[kScalarListGroups], rb);  // (the list behind round 0: what the first doubling round runs on)
    // behind a pruned round 0 every group carries the depth its own tokens need (DepthRule, prune.h)
    uint32_t *gneed_cur = d_gneed0, *gneed_nxt = d_gneed1;
    const bool group_need = prune && M > 0;
    while (n_act > 0) {
      DepthRule rrule = rule;
      if (group_need) {
        rrule.gneed_in = gneed_cur;
        rrule.gneed_out = gneed_nxt;
        std::swap(gneed_cur, gneed_nxt);
      }
      // A doubling round adds to a group's depth the depth of the group its second keys point into: that doubles the
      // depth while those groups are refined too (full depth: 31 rounds for 2^31 symbols), and adds at least the depth
      // of a round-0 group — one symbol or more — when they retired in round 0.  More rounds than that can only mean
      // corrupted ranks: stop instead of spinning.
      if (static_cast<uint64_t>(rounds) > 80 + (full ? 0ull : static_cast<uint64_t>(need_depth))) {
        throw HipError("prefix doubling did not converge (internal error)");
      }
      if (rounds < 40) S.active_per_round[rounds] = static_cast<int64_t>(n_act);
      // small groups: one LDS-resident segmented sort per window of the list (already queued by next_round_begin:
      // avals -> (LK0, spare_vals))
      uint64_t *skeys = LK0, *kfree = LK1;
      uint32_t *svals = spare_vals, *nvals = avals;  // avals is free again once the sorts have consumed it
      if (n_large > 0) {  // large groups (side stream, disjoint list positions): extract, global radix sort on
                          // (dense large id, second key), write back
        const int lgb = bit_length(n_large_groups > 0 ? n_large_groups - 1 : 0);
        hipLaunchKernelGGL(large_extract_kernel, dim3(cdiv(cdiv(n_large, kLxSpan), kBlock / kWave)), dim3(kBlock), 0, st2, avals, adep,
                           d_lg_head, d_lg_off, static_cast<uint32_t>(n_large_groups), n_large, d_rank, n, rb, LK1, LV0, LPOS,
                           static_cast<const uint32_t *>(nullptr));
        const int lc = radix_sort_pairs<uint64_t>(LK1, LV0, LK2, LV1, n_large, 0, rb + lgb, d_radix_tmp, radix_words, st2, nullptr);
        hipLaunchKernelGGL(large_writeback_kernel, dim3(std::min<size_t>(cdiv(n_large, kBlock), 8192)), dim3(kBlock), 0, st2,
                           lc ? LK2 : LK1, lc ? LV1 : LV0, LPOS, n_large, AG, rb, skeys, svals);
        join();
      }
      const unsigned tiles = cdiv(n_act, kRrTile);
      RankEntry *hd = reinterpret_cast<RankEntry *>(kfree);
      hipLaunchKernelGGL(HIP_KERNEL_NAME(rerank_agg_kernel<false>), dim3(tiles), dim3(kBlock), 0, st, skeys, svals, n_act, adep,
                         d_rank, d_gdepth, n, dcode.first_len, dcode.uniform_bits, rrule, d_tdep, d_agg);
      hipLaunchKernelGGL(rerank_chunk_kernel, dim3(cdiv(tiles, kRrChunk)), dim3(kBlock), 0, st, d_agg, tiles, d_chunk_agg);
      hipLaunchKernelGGL(rerank_prefix_kernel, dim3(cdiv(tiles, kRrChunk)), dim3(kBlock), 0, st, d_agg, d_chunk_agg, tiles);
      hipLaunchKernelGGL(HIP_KERNEL_NAME(rerank_apply_kernel<SymT, false>), dim3(tiles), dim3(kBlock), 0, st, skeys, svals, slots,
                         adep, d_tdep, n_act, d_agg, d_sym, n, dcode.first_len, dcode.uniform_bits, rrule, d_sa, hd, d_lcp,
                         other_slots, nvals, AG, other_dep, d_ghead, d_gdepth, c->d_scalars + kScalarList);
      fork();
      // (scratch of the partitioned store: behind the rank entries in their buffer, and the sorted keys)
      store_ranks(svals, hd, reinterpret_cast<uint32_t *>(hd) + list_cap + 2, reinterpret_cast<uint32_t *>(skeys), n_act);
      WP_LAUNCH_CHECK();
      rounds++;
      classified = classify_groups(n_act);
      join();
      std::swap(slots, other_slots);
      std::swap(adep, other_dep);
      avals = nvals;
      spare_vals = svals;
      next_round_begin(n_act, rb);  // (the next list is at most as long as this one)
    }
  }

  // ---- who marks + the four scanlines as step functions (linear.cpp:153-213) -----------------------------------------
  void scanlines() {
    // (the side stream may start now, but its launches are issued behind the first scanline kernels so that the host
    // does not keep the main stream waiting)
    if (n_text > 0) fork();
    MarkView mv{};
    // (step values carry the token length above the id where both fit: scanline.h)
    const int pack_steps = (hv.longest < kStepMaxLen && hv.tokens.size() < (size_t(1) << kStepIdBits)) ? 1 : 0;
    const size_t vocab_base = n_text + 1;
    uint32_t *mslot = d_mslot0, *midx = d_midx0;
    if (text_only) {
      // S = text . 1: the reach of every token is its range in the sorted keys (prune.h); a long token's is the run of
      // the trie nodes below its own inside its group (trie.h).  The marks arrive sorted (tokens in lexicographic order).
      if (M > 0) {
        if (early_refine) {  // the group starts, the token ranges, the marks and their step starts in one launch
          hipLaunchKernelGGL(token_marks_kernel, dim3(cdiv(M, kBlock)), dim3(kBlock), 0, st, d_node_of_slot, c->d_elig_node,
                             c->d_elig_subtree, M, d_rng_lo, d_rng_hi, d_rng_long, d_tok_group, d_ghead, d_gfirst,
                             c->d_scalars + kScalarList, n_sorted, c->d_elig_id, c->d_elig_info, d_mslot0, d_mid, d_minfo, d_rf, d_rb,
                             d_ps0, d_gend);
        } else {
          hipLaunchKernelGGL(trie_token_range_kernel, dim3(cdiv(M, kBlock)), dim3(kBlock), 0, st, d_node_of_slot, c->d_elig_node,
                             c->d_elig_subtree, M, d_rng_lo, d_rng_hi, d_rng_long);
          hipLaunchKernelGGL(virtual_marks_kernel, dim3(cdiv(M, kBlock)), dim3(kBlock), 0, st, d_rng_lo, d_rng_hi, M, c->d_elig_id,
                             c->d_elig_info, d_mslot0, d_mid, d_minfo, d_rf, d_rb);
        }
      }
      mv = MarkView{mslot, d_mid, d_minfo, d_rf, d_rb, M, d_cover_f, d_cover_b};
    } else {
      if (M > 0) {
        hipLaunchKernelGGL(mark_slots_kernel, dim3(cdiv(M, kBlock)), dim3(kBlock), 0, st, c->d_elig_start, M, vocab_base, d_rank,
                           d_mslot0, d_midx0);
        int mc = radix_sort_pairs<uint32_t>(d_mslot0, d_midx0, d_mslot1, d_midx1, M, 0, bit_length(n), d_radix_tmp, radix_words, st,
                                            nullptr);
        mslot = mc ? d_mslot1 : d_mslot0;
        midx = mc ? d_midx1 : d_midx0;
        hipLaunchKernelGGL(mark_gather_kernel, dim3(cdiv(M, kBlock)), dim3(kBlock), 0, st, midx, M, c->d_elig_id, c->d_elig_info,
                           d_mid, d_minfo);
      }
      hipLaunchKernelGGL(tile_mlo_kernel, dim3(cdiv(sl_tiles + 1, kBlock)), dim3(kBlock), 0, st, mslot, M, n, sl_tiles, d_tile_mlo);
      hipLaunchKernelGGL(sl_summary_kernel, dim3(sl_tiles), dim3(kBlock), 0, st, d_lcp, n, mslot, d_minfo, d_tile_mlo, d_tmin_f,
                         d_tmin_b, d_rf, d_rb);
      hipLaunchKernelGGL(sl_group_min_kernel, dim3(cdiv(static_cast<size_t>(sl_groups) * kWave, kBlock)), dim3(kBlock), 0, st,
                         d_tmin_f, d_tmin_b, sl_tiles, sl_groups, d_gmin_f, d_gmin_b);
      mv = MarkView{mslot, d_mid, d_minfo, d_rf, d_rb, M, d_cover_f, d_cover_b};
      if (M > 0) {
        hipLaunchKernelGGL(sl_reach_global_kernel, dim3(cdiv(static_cast<size_t>(M) * kWave, kBlock)), dim3(kBlock), 0, st, d_lcp, n,
                           sl_tiles, sl_groups, mslot, d_minfo, M, d_tmin_f, d_tmin_b, d_gmin_f, d_gmin_b, d_rf, d_rb);
      }
    }
    // The tail of the stage on two streams (key lookup): the cover scan runs on the second side stream beside the step
    // starts and their sort, and so does, beside the step values, everything behind the sort that reads no value
    // (side_tables).  The main stream waits for the scan in front of piece_values_kernel and for the tables behind it.
    hipStream_t st3 = key_lookup ? c->stream3 : st;
    if (M > 0) {
      if (key_lookup) {
        WP_HIP(hipEventRecord(c->evs[kEvMarks], st));
        WP_HIP(hipStreamWaitEvent(st3, c->evs[kEvMarks], 0));
      }
      const unsigned chunks = cdiv(M, kCoverChunk);
      if (chunks > 1) {
        hipLaunchKernelGGL(mark_cover_totals_kernel, dim3(chunks, 4), dim3(kCoverThreads), 0, st3, d_minfo, d_rf, d_rb, M, d_cover_tot);
      }
      hipLaunchKernelGGL(mark_cover_kernel, dim3(chunks, 4), dim3(kCoverThreads), 0, st3, d_minfo, d_rf, d_rb, M,
                         chunks > 1 ? d_cover_tot : static_cast<const int32_t *>(nullptr), d_cover_f, d_cover_b);
      if (key_lookup) WP_HIP(hipEventRecord(c->evs[kEvCovered], st3));
    }
    if (n_text > 0 && !anchors_queued) launch_anchors(st2);
    if (!early_refine) {  // (else: token_marks_kernel)
      hipLaunchKernelGGL(piece_starts_kernel, dim3(cdiv(std::max(M, 1), kBlock)), dim3(kBlock), 0, st, mv, n_sorted, d_ps0);
    }
    // (key_lookup: the starts of the needed groups wait behind the marks' starts, group_starts_kernel; extra starts
    // leave the slot-space step function as it is — every value is evaluated at its own start)
    const int P = this->P + (key_lookup ? 2 * static_cast<int>(n_groups) : 0);
    // (keys alone: only the sorted starts go on)
    const int pc = radix_sort_pairs<uint32_t>(d_ps0, nullptr, d_ps1, nullptr, P, 0, bit_length(n), d_radix_tmp, radix_words, st, nullptr);
    uint32_t *pstart = pc ? d_ps1 : d_ps0;
    for (BucketIndex &b : bix) {  // (slot space holds n_sorted slots: the indices need no bucket behind them)
      if (b.planned && !b.keyed) b.used = static_cast<unsigned>(((n_sorted - 1) >> b.shift) + 1);
      b.starts = b.keyed ? d_kstart : pstart;
    }
    if (key_lookup) {
      WP_HIP(hipEventRecord(c->evs[kEvStartsSorted], st));
      if (M > 0) WP_HIP(hipStreamWaitEvent(st, c->evs[kEvCovered], 0));
    }
    hipLaunchKernelGGL(piece_values_kernel, dim3(cdiv(static_cast<size_t>(P) * kWave, kBlock)), dim3(kBlock), 0, st, mv, pstart, P,
                       d_pval_p, d_pval_s, pack_steps);
    if (key_lookup) {  // (queued behind the values, which take longer than these six launches: the host keeps neither stream waiting)
      WP_HIP(hipStreamWaitEvent(st3, c->evs[kEvStartsSorted], 0));
      side_tables(pstart, P, st3);
      WP_HIP(hipEventRecord(c->evs[kEvTablesIndexed], st3));
      WP_HIP(hipStreamWaitEvent(st, c->evs[kEvTablesIndexed], 0));
      fill_tables(pstart, P);
    } else {
      for (const BucketIndex &b : bix) {
        if (!b.planned) continue;
        bucket_index(b, P, st);
        hipLaunchKernelGGL(piece_bucket_fast_kernel, dim3(cdiv(b.used, kBlock)), dim3(kBlock), 0, st, b.idx, d_pval_p, d_pval_s, b.used,
                           b.fast);
      }
    }
    WP_LAUNCH_CHECK();
    for (int i = 0; i < kStepIndexes; i++) {  // (an absent twin: the table of the index it would repeat)
      const BucketIndex &b = bix[i].planned || i < kIxSlotAll ? bix[i] : bix[i - 2];
      if (!b.planned) continue;
      tables[i] = StepTable{b.starts, b.keyed ? d_kval_p : d_pval_p, b.keyed ? d_kval_s : d_pval_s, b.idx, b.shift, pack_steps, b.fast};
    }
    // wp_step_stats: the tables as the walk gets them
    S.step.n_marks = M;
    S.step.n_steps = P;
    S.step.n_tiles = sl_tiles;
    S.step.n_groups_of_tiles = sl_groups;
    S.step.bucket_shift = bix[kIxSlot].shift;
    S.step.bucket_shift_all = bix[kIxSlotAll].shift;
    S.step.key_shift = bix[kIxKey].shift;
    S.step.key_shift_all = bix[kIxKeyAll].shift;
    S.step.packed = pack_steps;
    S.step.key_lookup = key_lookup ? 1 : 0;
  }

  // bidx of one index: the first step of every bucket
  void bucket_index(const BucketIndex &b, int P, hipStream_t s) {
    hipLaunchKernelGGL(piece_bucket_kernel, dim3(cdiv(b.used + 1, kBlock)), dim3(kBlock), 0, s, b.starts, P, b.shift, b.used, b.idx);
  }

  // The tables of the key lookup in two halves (scanlines()): the step table in key space (scanline.h) has its starts by
  // the sorted keys, and its entries inside needed groups answer kStepNeeded.  side_tables: what needs the sorted starts,
  // the sorted keys and the group table only — the bucket indices of both spaces, kstart and the steps inside needed
  // groups — on stream s, beside piece_values_kernel.  fill_tables: behind the values, one launch for kval and every fast
  // entry.
  void side_tables(const uint32_t *pstart, int P, hipStream_t s) {
    const uint32_t *skeys = reinterpret_cast<const uint32_t *>(keys);
    hipLaunchKernelGGL(key_starts_kernel, dim3(cdiv(P, kBlock)), dim3(kBlock), 0, s, pstart, P, skeys, d_kstart, d_kneed);
    if (n_groups > 0) {
      hipLaunchKernelGGL(key_steps_flag_kernel, dim3(cdiv(n_groups, kBlock)), dim3(kBlock), 0, s, d_gfirst, d_gend,
                         static_cast<uint32_t>(n_groups), pstart, P, d_kneed);
    }
    for (const BucketIndex &b : bix) {
      if (b.planned) bucket_index(b, P, s);
    }
    WP_LAUNCH_CHECK();
  }
  void fill_tables(const uint32_t *pstart, int P) {
    StepFill fill{};
    unsigned most = static_cast<unsigned>(P);
    for (const BucketIndex &b : bix) {
      if (!b.planned) continue;
      fill.t[fill.count++] = StepFillTable{b.idx, b.fast, b.used, b.keyed ? 1 : 0};
      most = std::max(most, b.used);
    }
    hipLaunchKernelGGL(step_tables_kernel, dim3(cdiv(most, kBlock)), dim3(kBlock), 0, st, d_pval_p, d_pval_s, P, d_kneed, d_kval_p, d_kval_s,
                       fill);
#ifdef WP_DEBUG_BOUNDS
    hipLaunchKernelGGL(key_steps_check_kernel, dim3(cdiv(P, kBlock)), dim3(kBlock), 0, st, pstart, P,
                       reinterpret_cast<const uint32_t *>(keys), d_kval_p, d_kval_s);
#endif
    WP_LAUNCH_CHECK();
  }

  // words longer than a lane should walk (walk.h, "long words"): pointer doubling instead.  Scratch: the slabs of the sort.
  // (KA holds the round-0 keys of the key-space lookup: the walk's scratch stays out of it in every layout)
  void walk_long_words(const WalkArgs &wa, size_t n_anchors) {
    const uint32_t lw_cap = static_cast<uint32_t>(n_text / kMaxAnchorGap + 2);
    LongWord *d_lw = reinterpret_cast<LongWord *>(d_tile_scratch);
    uint32_t *d_lw_off = d_tile_scratch + 2 * static_cast<size_t>(lw_cap);
    uint32_t *d_lw_fail = d_lw_off + lw_cap + 1;
    hipLaunchKernelGGL(long_word_collect_kernel, dim3(std::min<size_t>(cdiv(std::max<size_t>(n_anchors, 1), kBlock), 2048)),
                       dim3(kBlock), 0, st, d_anchors, c->d_scalars + kScalarAnchors, n_text, d_cls, d_lw, lw_cap, c->d_scalars + kScalarLongWords);
    WP_LAUNCH_CHECK();
    const LongWordList lw = long_word_offsets(c, d_lw, lw_cap, d_lw_off, d_lw_fail, st);
    if (lw.nw == 0) return;
    S.walk.n_long_words = static_cast<int64_t>(lw.nw);
    int32_t *d_lid = reinterpret_cast<int32_t *>(VA);
    uint32_t *jump_a = X1, *jump_b = X0;
    uint8_t *d_mark = reinterpret_cast<uint8_t *>(KB);
    // (every position of the long words is looked up: the small index)
    hipLaunchKernelGGL(long_word_next_kernel, lw.grid(), dim3(kBlock), 0, st, walk_args(true), d_lw, d_lw_off, lw.nw, lw.total, d_lid,
                       jump_a, d_mark);
    WP_HIP(hipStreamSynchronize(st));  // lw.h_off is an upload source
    long_word_chains(lw, jump_a, jump_b, d_lid, d_mark, d_lw_off, d_lw_fail, st);
    const bool offs = offs_unit >= 0;
    uint32_t *d_lw_end = offs ? d_lw_fail + lw_cap : nullptr;
    if (offs) {  // (the [UNK] of a failed word spans the word: up to its first blank)
      WP_HIP(hipMemsetAsync(d_lw_end, 0xff, sizeof(uint32_t) * lw.nw, st));
      hipLaunchKernelGGL(long_word_end_kernel, lw.grid(), dim3(kBlock), 0, st, d_lw, d_lw_off, lw.nw, lw.total, d_lid, d_lw_end);
    }
    hipLaunchKernelGGL(offs ? long_word_emit_kernel<true> : long_word_emit_kernel<false>, lw.grid(), dim3(kBlock), 0, st, wa, d_lw,
                       d_lw_off, lw.nw, lw.total, d_lid, d_mark, d_lw_fail, d_ospill, static_cast<const uint32_t *>(d_lw_end));
    WP_LAUNCH_CHECK();
    S.anchor_mode = 2;
  }

  // long stretches without class-rule anchors ("soft" spacing chars): anchors from the matches themselves, inside the
  // long gaps of the class rule only (walk.h).  Returns the number of anchors.
  size_t cover_anchors(WalkArgs &wa) {
    uint32_t *d_reach = VA, *d_reach_tiles = d_tile_scratch;
    uint8_t *d_aflags = reinterpret_cast<uint8_t *>(X1);
    const unsigned rtiles = cdiv(n_text, kReachTile), atiles = cdiv(n_text, kAnchorTile);
    uint32_t *d_wp_tiles = d_reach_tiles + rtiles + 1;  // first word-prefix position at or behind each tile
    uint32_t *d_ns_tiles = d_wp_tiles + rtiles + 1;     // same for non-space positions
    uint32_t *d_gap_a = d_ns_tiles + rtiles + 1, *d_gap_b = d_gap_a + rtiles + 1;  // where the coverage rule applies
    // (the class-rule anchor list is still in d_anchors: the coverage rule is only needed inside its long gaps)
    hipLaunchKernelGGL(gap_tiles_kernel, dim3(cdiv(rtiles, kBlock)), dim3(kBlock), 0, st, d_anchors, c->d_scalars + kScalarAnchors, n_text, rtiles,
                       v->cover_anchors ? 1 : 0, d_gap_a, d_gap_b);
    hipLaunchKernelGGL(reach_kernel, dim3(rtiles), dim3(kBlock), 0, st, wa, d_reach, d_reach_tiles, d_gap_a, d_gap_b);
    hipLaunchKernelGGL(reach_spine_kernel, dim3(1), dim3(1024), 0, st, d_reach_tiles, static_cast<size_t>(rtiles));
    WP_HIP(hipMemsetAsync(d_anchor_cnt, 0, sizeof(uint32_t) * atiles, st));
    hipLaunchKernelGGL(cover_flags_kernel, dim3(rtiles), dim3(kBlock), 0, st, d_cls, d_reach, d_reach_tiles, n_text, d_aflags,
                       d_wp_tiles, d_ns_tiles, d_gap_a, d_gap_b, d_anchor_cnt);
    hipLaunchKernelGGL(suffix_min_kernel, dim3(2), dim3(1024), 0, st, d_wp_tiles, d_ns_tiles, static_cast<size_t>(rtiles));
    device_exclusive_scan(d_anchor_cnt, d_anchor_cnt, atiles, d_anchor_tmp, c->d_scalars + kScalarAnchors, st);  // (counted by cover_flags_kernel)
    hipLaunchKernelGGL(anchor_write_kernel, dim3(atiles), dim3(kBlock), 0, st, d_cls, d_aflags, n_text, d_anchor_cnt, d_anchors);
    WP_LAUNCH_CHECK();
    fetch_scalars(c, kScalarAnchors);
    wa.aflags = d_aflags;
    wa.wp_from_tile = d_wp_tiles;
    wa.ns_from_tile = d_ns_tiles;
    S.anchor_mode = 1;
    return c->h_scalars[kScalarAnchors];
  }

  // ---- greedy walk + id stream (linear.cpp:215-316).  Slabs: round-0 keys KA (key_lookup), ids VB, id lists X0, wide
  // list / counts KB VA (VA / X1 hold the coverage rule's reach / flags; VA X1 X0 KB the long words' scratch) ----------
  // all: with the "_all" indexes, for a kernel that looks up every position of a stretch
  WalkArgs walk_args(bool all = false) const {
    return WalkArgs{d_cls, n_text, d_rank, tables[all ? kIxSlotAll : kIxSlot], c->d_tok_len, hv.unk_id, d_emit, nullptr, nullptr, nullptr,
                    hv.soft.empty() ? 1 : 0, static_cast<int32_t>(hv.tokens.size()),
                    key_lookup ? reinterpret_cast<const uint32_t *>(KA) : nullptr, tables[all ? kIxKeyAll : kIxKey], drop_blanks ? 1 : 0};
  }

  // WP_OPT_KEEP_DEBUG = 2: what the walk's own lookup answers at every text position, behind the scanline stage and the
  // rank scatter (both on the main stream) and in front of the walk, which reuses the slabs of the sort but none the
  // lookup reads
  void step_views() {
    if (!d_step_views || n_text == 0) return;
    hipLaunchKernelGGL(step_views_kernel, dim3(cdiv(n_text, kBlock)), dim3(kBlock), 0, st, walk_args(), d_step_views);
    WP_LAUNCH_CHECK();
  }

  int32_t *walk(size_t *n_ids_out) {
    int32_t *d_ids = reinterpret_cast<int32_t *>(VB);
    *n_ids_out = 0;
    if (n_text == 0) return d_ids;
    WalkArgs wa = walk_args();
    S.anchor_mode = 0;
    join();  // (the anchor list of the side stream)
    if (anchor_scalars_queued) {  // (their own copy, queued behind the anchor list: no wait for the main stream)
      WP_HIP(hipEventSynchronize(c->evs[kEvAnchorScalars]));
    } else {
      fetch_scalars(c, kScalarAnchorGap);
    }
    size_t n_anchors = c->h_scalars[kScalarAnchors];
    const size_t max_anchor_gap = c->h_scalars[kScalarAnchorGap];
    S.walk.max_anchor_gap = static_cast<int32_t>(max_anchor_gap);
    const bool all_hard = hv.soft.empty();
    bool staged = staged_possible && max_anchor_gap <= kMaxAnchorGap;
    if (staged_possible && !staged) WP_HIP(hipMemsetAsync(d_emit, 0x80, n_text * sizeof(int32_t), st));  // long words after all
    if (!v->cover_anchors && all_hard && max_anchor_gap > kMaxAnchorGap) {
      walk_long_words(wa, n_anchors);
    } else if (v->cover_anchors || max_anchor_gap > kMaxAnchorGap) {
      n_anchors = cover_anchors(wa);
      // coverage anchors: every id still comes from the lanes of the walk kernel, each inside its own stretch
      // [anchor, next anchor) — the id lists work as they do for the class rule (the cleared emit array is not used)
      staged = !sparse_emit;
    }
    S.n_anchors = static_cast<int64_t>(n_anchors);
    // one lane per anchor (a grid sized for the worst case, every position an anchor, costs 0.35 ms of empty workgroups)
    const size_t acap = std::max<size_t>(n_anchors, 1);
    const bool offs = offs_unit >= 0;
    if (staged) {
      int32_t *d_ctmp = reinterpret_cast<int32_t *>(X0);
      const unsigned sblocks = cdiv(acap, static_cast<size_t>(kWbWords));
      // stretches of more than kWideMin positions (class rule, hard spacing chars only: one word each) go to a whole
      // wave each first (walk.h, wide walk)
      if (S.anchor_mode == 0 && all_hard && max_anchor_gap > kWideMin) {
        uint32_t *d_wide_list = reinterpret_cast<uint32_t *>(KB), *d_wide_cnt = VA;
        wide_ran = true;
        clear_scalars(c, kScalarWideWords, kScalarWideWords, st);
        hipLaunchKernelGGL(wide_collect_kernel, dim3(std::min<size_t>(cdiv(acap, kBlock), 2048)), dim3(kBlock), 0, st, d_anchors,
                           c->d_scalars + kScalarAnchors, n_text, d_wide_list, c->d_scalars + kScalarWideWords);
        // (every position of the wide words is looked up: the small index)
        hipLaunchKernelGGL(offs ? walk_wide_kernel<true> : walk_wide_kernel<false>, dim3(std::min<size_t>(cdiv(acap, kBlock / kWave), 8192)),
                           dim3(kBlock), 0, st, walk_args(true), d_anchors, c->d_scalars + kScalarAnchors, d_wide_list,
                           c->d_scalars + kScalarWideWords, d_wide_cnt, d_ospill);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(offs ? walk_lean_kernel<true, true> : walk_lean_kernel<true, false>), dim3(sblocks), dim3(kBlock),
                           0, st, wa, d_anchors, c->d_scalars + kScalarAnchors, acap, d_ctmp, d_blk_cnt, d_wide_cnt, d_ospill, d_cspan);
      } else {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(offs ? walk_lean_kernel<false, true> : walk_lean_kernel<false, false>), dim3(sblocks),
                           dim3(kBlock), 0, st, wa, d_anchors, c->d_scalars + kScalarAnchors, acap, d_ctmp, d_blk_cnt,
                           static_cast<const uint32_t *>(nullptr), d_ospill, d_cspan);
      }
      device_exclusive_scan(d_blk_cnt, d_blk_off, sblocks, d_emit_tmp, c->d_scalars + kScalarIds, st);
      hipLaunchKernelGGL(offs ? emit_gather_kernel<true> : emit_gather_kernel<false>, dim3(sblocks), dim3(kBlock), 0, st, d_anchors,
                         c->d_scalars + kScalarAnchors, acap, d_ctmp, d_blk_cnt, d_blk_off, d_ids, kWbWords,
                         static_cast<const uint2 *>(d_cspan), d_offs);
    } else {
      hipLaunchKernelGGL(offs ? walk_kernel<true> : walk_kernel<false>, dim3(cdiv(acap, kBlock)), dim3(kBlock), 0, st, wa, d_anchors,
                         c->d_scalars + kScalarAnchors, acap, d_ospill);
      const unsigned tiles = cdiv(n_text, kScanTile);
      hipLaunchKernelGGL(emit_count_kernel, dim3(tiles), dim3(kBlock), 0, st, d_emit, n_text, d_emit_cnt);
      device_exclusive_scan(d_emit_cnt, d_emit_cnt, tiles, d_emit_tmp, c->d_scalars + kScalarIds, st);
      hipLaunchKernelGGL(offs ? emit_write_kernel<true> : emit_write_kernel<false>, dim3(tiles), dim3(kBlock), 0, st, d_emit, n_text,
                         d_emit_cnt, d_ids, static_cast<const uint2 *>(d_ospill), d_offs);
    }
    S.staged_emit = staged ? 1 : 0;
    S.walk.lean = staged ? 1 : 0;  // (every list-building walk of this path is walk_lean_kernel)
    WP_LAUNCH_CHECK();
    return d_ids;
  }

  // documents call (rows.h): the starts of the rows, then row_splits[] (and the rows' starts in the offsets' unit) from
  // the spans, which are still in code points here
  void row_structure(size_t n_ids) {
    const size_t n_rows = rows->n_rows;
    const long long *d_starts = rows->d_doc_off;
    if (!d_starts) {
      // (normalised text: a last line of dropped code points only is a row of the source that the normalised text has
      // no line for — it starts, empty, at the end)
      if (nmap) hipLaunchKernelGGL(norm_fill_starts_kernel, dim3(cdiv(n_rows + 1, kBlock)), dim3(kBlock), 0, st, d_line_starts, n_rows + 1, static_cast<long long>(nbytes));
      hipLaunchKernelGGL(line_write_kernel, dim3(cdiv(nbytes, kLineTile)), dim3(kBlock), 0, st, d_text, nbytes,
                         static_cast<const uint32_t *>(rows->d_line_cnt), n_rows, d_line_starts);
      d_starts = d_line_starts;
    }
    if (n_ids > 0) {
      hipLaunchKernelGGL(cp_byte_kernel, dim3(cdiv(nbytes, kDecTile)), dim3(kBlock), 0, st, d_text, nbytes, d_tile_prefix, n_text,
                         d_byte_of);
      if (nmap && rows->d_doc_off) {  // explicit rows are bytes of the source
        hipLaunchKernelGGL(norm_doc_starts_kernel, dim3(cdiv(n_rows + 1, kBlock)), dim3(kBlock), 0, st, rows->d_doc_off, n_rows, *nmap,
                           static_cast<const uint32_t *>(d_byte_of), nbytes, d_line_starts);
        d_starts = d_line_starts;
      }
      hipLaunchKernelGGL(row_splits_kernel, dim3(cdiv(n_rows + 1, kBlock)), dim3(kBlock), 0, st, d_starts, n_rows,
                         static_cast<const uint32_t *>(d_byte_of), n_text, static_cast<const uint2 *>(d_offs), n_ids, rows->unit,
                         d_row_splits, d_row_base);
      if (nmap && d_row_base) {  // the rows' starts in the caller's text
        hipLaunchKernelGGL(norm_row_base_kernel, dim3(cdiv(n_rows + 1, kBlock)), dim3(kBlock), 0, st, d_starts, n_rows,
                           static_cast<const uint32_t *>(d_byte_of), n_text, *nmap, rows->unit, d_row_base);
      }
    } else {
      WP_HIP(hipMemsetAsync(d_row_splits, 0, (n_rows + 1) * sizeof(long long), st));
    }
    WP_LAUNCH_CHECK();
    rows->d_starts = d_starts;
    rows->d_row_splits = d_row_splits;
  }

  // guard zones, bounds counters, the id count, statistics, debug views
  void finish(int32_t *d_ids, size_t *n_ids_out) {
    c->d_offs = nullptr;
    if (offs_unit >= 0 && n_text > 0) {
      fetch_scalars(c, kScalarIds);
      const size_t n_ids = c->h_scalars[kScalarIds];
      if (rows) row_structure(n_ids);
      if (nmap) {  // normalised code points -> the caller's text, in either unit (a documents call without offsets: not needed)
        if (n_ids > 0 && (!rows || rows->unit >= 0)) {
          hipLaunchKernelGGL(span_source_kernel, dim3(cdiv(n_ids, kBlock)), dim3(kBlock), 0, st, d_offs, n_ids, *nmap, offs_unit);
          WP_LAUNCH_CHECK();
        }
      } else if (offs_unit == WP_OFFSETS_BYTES && n_ids > 0) {  // code points -> bytes
        if (!rows) {  // (a documents call has built byte_of[] for its row splits)
          hipLaunchKernelGGL(cp_byte_kernel, dim3(cdiv(nbytes, kDecTile)), dim3(kBlock), 0, st, d_text, nbytes, d_tile_prefix, n_text,
                             d_byte_of);
        }
        hipLaunchKernelGGL(span_bytes_kernel, dim3(cdiv(n_ids, kBlock)), dim3(kBlock), 0, st, d_offs, n_ids,
                           static_cast<const uint32_t *>(d_byte_of), d_text, n_text);
        WP_LAUNCH_CHECK();
      }
      if (rows && rows->unit >= 0 && n_ids > 0) {  // offsets relative to the id's own document: one pass over the spans
        hipLaunchKernelGGL(rebase_kernel, dim3(cdiv(n_ids, kRebaseTile)), dim3(kBlock), 0, st, d_offs, n_ids,
                           static_cast<const long long *>(d_row_splits), rows->n_rows, static_cast<const uint32_t *>(d_row_base));
        WP_LAUNCH_CHECK();
      }
      c->d_offs = reinterpret_cast<const uint32_t *>(d_offs);
    } else if (rows) {  // (a text without one code point: every row is empty)
      row_structure(0);
    }
    if (ar.guard) {  // debugging aid: no kernel may have written outside the buffer it was given
      static const uint32_t init[2] = {0u, 0xffffffffu};
      WP_HIP(hipMemcpyAsync(c->d_scalars + kScalarGuard, init, sizeof(init), hipMemcpyHostToDevice, st));
      ar.check(st, c->d_scalars + kScalarGuard);
      aa.check(st, c->d_scalars + kScalarGuard);
      fetch_scalars(c, kScalarGuardFirst);
      if (c->h_scalars[kScalarGuardBad] != 0) {
        throw HipError("arena guard: " + std::to_string(c->h_scalars[kScalarGuardBad]) + " guard zone(s) overwritten, first behind allocation #" +
                       std::to_string(c->h_scalars[kScalarGuardFirst] - 1));
      }
      S.guard_zones = static_cast<int32_t>(ar.zones.size() + aa.zones.size());
    }
#ifdef WP_DEBUG_BOUNDS
    {
      unsigned int oob[kCountedSites] = {};
      WP_HIP(hipStreamSynchronize(st));
      take_oob(0, kCountedSites, oob);
      if (oob[0] | oob[1] | oob[2] | oob[3] | oob[4] | oob[5] | oob[6] | oob[7] | oob[8] | oob[kSiteRankFlag]) {
        throw HipError("debug bounds: out-of-range addresses skipped: radix scatter " + std::to_string(oob[0]) + ", rank store " +
                       std::to_string(oob[1]) + ", token id " + std::to_string(oob[2]) + ", list slot " + std::to_string(oob[3]) +
                       "; key-space step starts inside a run of equal keys " + std::to_string(oob[4]) +
                       "; candidate runs unlike their group " + std::to_string(oob[5]) + "; offsets " + std::to_string(oob[6]) +
                       "; step values used at blanks " + std::to_string(oob[7]) +
                       "; round-0 sorted array: descents, blank keys left, multiset unlike the kept keys " + std::to_string(oob[8]) +
                       "; lookups whose ranked flag and key-space answer disagree " + std::to_string(oob[kSiteRankFlag]));
      }
      S.reserved0 = 1;  // this is the bounds-checking build
    }
#endif
    fetch_scalars(c, kScalarSplitTotals);
    const size_t n_ids = n_text > 0 ? c->h_scalars[kScalarIds] : 0;
    S.n_ids = static_cast<int64_t>(n_ids);
    S.walk.n_wide_words = wide_ran ? static_cast<int64_t>(c->h_scalars[kScalarWideWords]) : 0;  // (cleared only when that branch runs)
    S.radix_passes = c->rstats.passes;
    S.radix_pass_elems = c->rstats.elems;
    S.radix_digit_bytes = c->rstats.digit_bytes;
    S.radix_pass_bytes = c->rstats.bytes;
    S.arena_bytes = static_cast<int64_t>(c->a_buf.cap + c->b_buf.cap);
    if (v->stage_timing) {
      auto span = [&](int a, int b) {
        float ms = 0;
        WP_HIP(hipEventElapsedTime(&ms, c->ev[a], c->ev[b]));
        return static_cast<double>(ms);
      };
      S.ms_decode = span(kMarkStart, kMarkSymbols);
      S.ms_sa = span(kMarkSymbols, kMarkSorted);
      S.ms_lcp = span(kMarkSorted, kMarkLcp);
      S.ms_scan = span(kMarkLcp, kMarkScanned);
      S.ms_walk = span(kMarkScanned, kMarkWalked);
      S.ms_total = span(kMarkStart, kMarkWalked) + S.ms_normalize;
      S.ms_radix_scatter = c->rstats.spans.resolve();
      S.sched.ms_sort_to_scan = span(kMarkRound0, kMarkLcp);
    }
    c->d_ids = d_ids;
    c->dbg.sym = d_sym;
    c->dbg.sym_bytes = sizeof(SymT);
    c->dbg.sa = d_sa;
    c->dbg.rank = d_rank;
    c->dbg.lcp = d_lcp;
    c->dbg.steps = tables[kIxSlot];
    c->dbg.best_scratch = d_dbg_best;
    c->dbg.step_views = n_text > 0 ? d_step_views : nullptr;
    c->dbg.cps = d_cps;
    c->dbg.cls = v->keep_debug ? d_cls : nullptr;
    c->dbg.n = n;
    c->dbg.n_text = n_text;
    *n_ids_out = n_ids;
  }

  void run(size_t *n_ids_out) {
    plan();
    symbols_and_keys();
    if (v->stage_timing) WP_HIP(hipEventRecord(c->ev[kMarkSymbols], st));
    sort_round0();
    if (v->stage_timing) WP_HIP(hipEventRecord(c->ev[kMarkRound0], st));
    ranks_round0();
    refine();
    if (v->stage_timing) WP_HIP(hipEventRecord(c->ev[kMarkSorted], st));
    if (v->lcp_kasai) {  // alternative LCP builder: chunked Kasai exactly as linear.cpp:18-70
      const size_t chunk = 64;
      hipLaunchKernelGGL(HIP_KERNEL_NAME(kasai_kernel<SymT>), dim3(cdiv(cdiv(n, chunk), kBlock)), dim3(kBlock), 0, st, d_sym, d_sa,
                         d_rank, n, chunk, d_lcp);
      WP_LAUNCH_CHECK();
    }
    if (v->stage_timing) WP_HIP(hipEventRecord(c->ev[kMarkLcp], st));
    scanlines();
    if (v->stage_timing) WP_HIP(hipEventRecord(c->ev[kMarkScanned], st));
    if (v->keep_step_views) step_views();  // (behind the mark: ms_scan stays the stage's own time, ms_walk carries the debug kernel)
    size_t n_ids = 0;
    int32_t *d_ids = walk(&n_ids);
    if (v->stage_timing) WP_HIP(hipEventRecord(c->ev[kMarkWalked], st));
    finish(d_ids, n_ids_out);
  }
};

// the radix statistics of an encode start from zero, and again when the encode starts over (ListOverflow)
static void reset_radix_stats(Context *c) {
  c->rstats.passes = 0;
  c->rstats.elems = 0;
  c->rstats.digit_bytes = 0;
  c->rstats.bytes = 0;
  c->rstats.spans.used = 0;
}

// The whole device path on context c (the calling thread has c's device current).  d_text must be
// 4-byte aligned and readable up to the next multiple of 16.  S: statistics of this call.
// offs_unit >= 0 (offsets mode, WP_OFFSETS_*): c->d_offs also holds the span of every id, [begin, end) as two uint32
static void encode_on_device(const wp_vocab *v, Context *c, const uint8_t *d_text, size_t nbytes, size_t *n_ids_out,
                             EncodeStats &S, int offs_unit = -1, RowsCall *rows = nullptr) {
  hipStream_t st = c->stream;
  const HostVocab &hv = v->hv;
  std::memset(&S, 0, sizeof(S));
  S.offsets_unit = -1;
  S.n_rows = -1;
  S.rows_route = -1;
  S.n_bytes = static_cast<int64_t>(nbytes);
  S.longest_token = hv.longest;
  c->d_ids = nullptr;
  c->d_offs = nullptr;
  c->dbg = {};
  *n_ids_out = 0;
  if (nbytes == 0) return;  // linear.cpp:323-325
  // (no limit on the byte length: the reference limits total_length = code points + vocab symbols,
  // linear.cpp:104-106, checked below once the code points are counted — in 64 bits, since the tile
  // prefix itself is 32-bit and wraps for inputs beyond 4 G code points)
  const bool guard = v->arena_guard || EnvOptions::get().arena_guard;
  S.offsets_unit = offs_unit;
  c->d_offs = nullptr;

  // ---------------- WP_OPT_NORMALIZE: the text is rewritten first, everything below runs on the copy ----------------
  const uint8_t *src_text = d_text;  // what the caller passed: explicit rows are checked, lines counted, against it
  const size_t src_bytes = nbytes;
  NormResult norm;
  const NormMap *nmap = nullptr;
  if (v->normalize != 0) {
    normalize_on_device(c, d_text, nbytes, v->normalize, offs_unit >= 0, v->stage_timing, norm);
    S.normalize = v->normalize;
    S.norm_bytes = static_cast<int64_t>(norm.nbytes);
    S.ms_normalize = norm.ms;
    if (norm.nbytes == 0) {
      if (!rows) return;  // nothing is left: no ids
      // (a documents call still has its one empty row to report: the lines of a single blank)
      WP_HIP(hipMemsetAsync(c->norm_buf.p, 0x20, 1, st));
      norm.nbytes = 1;
    }
    d_text = norm.text;
    nbytes = norm.nbytes;
    if (offs_unit >= 0) nmap = &norm.map;
  }

  reset_radix_stats(c);
  c->rstats.spans.on = v->stage_timing;
  if (v->stage_timing) WP_HIP(hipEventRecord(c->ev[kMarkStart], st));

  // ---------------- phase A: decode ----------------
  const unsigned dec_tiles = cdiv(nbytes, kDecTile);
  Arena aa(&c->a_buf, guard);
  uint32_t *d_tile_cnt = nullptr, *d_cnt_tmp = nullptr, *d_cps = nullptr;
  uint8_t *d_cls = nullptr;
  const unsigned line_tiles = cdiv(nbytes, kLineTile), src_line_tiles = cdiv(src_bytes, kLineTile);
  uint32_t *d_line_tmp = nullptr, *d_src_line_cnt = nullptr;
  for (int pass = 0; pass < 2; pass++) {
    d_tile_cnt = aa.take<uint32_t>(dec_tiles + 1);
    d_cnt_tmp = aa.take<uint32_t>(cdiv(dec_tiles, kScanTile) + 8);
    d_cps = v->keep_debug ? aa.take<uint32_t>(nbytes + 1) : nullptr;  // raw code points: debug copy only
    d_cls = aa.take<uint8_t>(nbytes + 32);  // (the walk reads 16 class bytes from any position on)
    if (rows && !rows->d_doc_off) {  // lines mode of a documents call: line ends per tile and the scan's scratch
      rows->d_line_cnt = aa.take<uint32_t>(line_tiles + 1);
      d_line_tmp = aa.take<uint32_t>(cdiv(line_tiles, kScanTile) + 8);
      if (v->normalize != 0) d_src_line_cnt = aa.take<uint32_t>(src_line_tiles + 1 + cdiv(src_line_tiles, kScanTile) + 8);
    }
    if (pass == 0) aa.commit();
  }
  aa.arm(st);
  WP_HIP(hipMemsetAsync(c->d_scalars, 0, sizeof(uint32_t) * kScalars, st));
  WP_HIP(hipMemsetAsync(c->d_used, 0, sizeof(uint32_t) * kCpWords, st));
  hipLaunchKernelGGL(decode_count_kernel<true>, dim3(dec_tiles), dim3(kBlock), 0, st, d_text, nbytes, d_tile_cnt,
                     reinterpret_cast<unsigned long long *>(c->d_scalars + kScalarInvalid), c->d_used);
  device_exclusive_scan(d_tile_cnt, d_tile_cnt, dec_tiles, d_cnt_tmp, c->d_scalars + kScalarCps, st, nullptr,
                        reinterpret_cast<unsigned long long *>(c->d_scalars + kScalarCps64));
  // does the text itself hold code point 0 or 1 (the separator)?  (read before the vocab marks its symbols)
  // (bits 0 and 1 of the first bitmap word)
  WP_HIP(hipMemcpyAsync(c->d_scalars + kScalarAlphaWord0, c->d_used, sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
  hipLaunchKernelGGL(vocab_alphabet_kernel, dim3(cdiv(hv.used_word_idx.size(), kBlock)), dim3(kBlock), 0, st,
                     c->d_vocab_word_idx, c->d_vocab_word_bits, static_cast<uint32_t>(hv.used_word_idx.size()), c->d_used);
  // alphabet: bitmap -> per-word prefixes + sigma -> lut (dense symbol of a used code point c = lut[c] + 1)
  hipLaunchKernelGGL(alphabet_prefix_kernel, dim3(1), dim3(kAlphaThreads), 0, st, c->d_used, c->d_scan_tmp, c->d_scalars + kScalarAlphabet);
  hipLaunchKernelGGL(alphabet_lut_kernel, dim3(kCpTableSize / kBlock), dim3(kBlock), 0, st, c->d_used, c->d_scan_tmp, c->d_lut);
  if (rows) {  // the rows of a documents call: counted (lines) or checked (explicit) beside the decode, fetched with its scalars
    if (rows->d_doc_off) {
      hipLaunchKernelGGL(rows_check_kernel, dim3(cdiv(rows->n_docs + 1, kBlock)), dim3(kBlock), 0, st, src_text, src_bytes, rows->d_doc_off,
                         rows->n_docs, c->d_scalars + kScalarRowsBad);
    } else {
      if (v->normalize != 0) {  // the rows are the lines of the caller's text (a last line may normalise to nothing)
        hipLaunchKernelGGL(line_count_kernel, dim3(src_line_tiles), dim3(kBlock), 0, st, src_text, src_bytes, d_src_line_cnt);
        device_exclusive_scan(d_src_line_cnt, d_src_line_cnt, src_line_tiles, d_src_line_cnt + src_line_tiles + 1,
                              c->d_scalars + kScalarSrcRows, st);
      }
      hipLaunchKernelGGL(line_count_kernel, dim3(line_tiles), dim3(kBlock), 0, st, d_text, nbytes, rows->d_line_cnt);
      device_exclusive_scan(rows->d_line_cnt, rows->d_line_cnt, line_tiles, d_line_tmp, c->d_scalars + kScalarRows, st);
    }
  }
  WP_LAUNCH_CHECK();
  fetch_scalars(c, rows ? (v->normalize != 0 ? kScalarSrcRows : kScalarRowsCut) : kScalarRows);
  if (rows) {
    if (rows->d_doc_off && c->h_scalars[kScalarRowsBad] != 0) {
      throw std::invalid_argument("document offsets: " + std::to_string(c->h_scalars[kScalarRowsBad]) +
                                  " boundaries are not increasing from 0 to nbytes with a '\\n' in front of each");
    }
    rows->n_rows = rows->d_doc_off ? rows->n_docs : c->h_scalars[v->normalize != 0 ? kScalarSrcRows : kScalarRows];
    if (rows->n_rows > rows->capacity) throw std::invalid_argument("capacity_rows is smaller than the number of rows");
    S.n_rows = static_cast<int64_t>(rows->n_rows);
    S.rows_route = 1;
  }
  unsigned long long n_text64;
  std::memcpy(&n_text64, c->h_scalars + kScalarCps64, sizeof(n_text64));
  if (n_text64 + 1 + hv.stream.size() > 2000000000ull) throw std::length_error("64bit not implemented");  // linear.cpp:104-106
  const size_t n_text = c->h_scalars[kScalarCps];
  // Layout of S.  The reference concatenates the whole vocabulary behind the text in every call and batch
  // (linear.cpp:77-101, 333, 347, 367).  Here the vocabulary normally stays out of the suffix sort: S = text . 1,
  // and the tokens come in through their code streams (prune.h).  The reference's layout is kept for the true
  // suffix array (full depth, duplicate vocab lines), for texts or tokens that hold the code points 0 / 1
  // (they sort around the separator), and on request (WP_OPT_VOCAB_IN_S).
  const bool full_sa = v->full_depth || hv.n_dup_eligible > 0 || v->lcp_kasai;
  const bool text_only = !full_sa && !v->vocab_in_s && !EnvOptions::get().vocab_in_s && !hv.low_cp && (c->h_scalars[kScalarAlphaWord0] & 3u) == 0;
  S.vocab_in_s = text_only ? 0 : 1;
  const uint32_t sigma = c->h_scalars[kScalarAlphabet];
  unsigned long long dropped;
  std::memcpy(&dropped, c->h_scalars + kScalarInvalid, sizeof(dropped));
  if (dropped != 0) std::cerr << "WARNING Input contains invalid unicode characters." << std::endl;

  const size_t n = n_text + 1 + (text_only ? 0 : hv.stream.size());  // total_length, linear.cpp:77-82
  S.n_text = static_cast<int64_t>(n_text);
  S.n_total = static_cast<int64_t>(n);
  S.alphabet = sigma;
  if (n > 2000000000ull) throw std::length_error("64bit not implemented");  // linear.cpp:104-106
  if (v->stage_timing) WP_HIP(hipEventRecord(c->ev[kMarkCounted], st));

  const int bits = std::max(1, bit_length(sigma));  // symbols are 1..sigma, 0 = past the end
  const DecodedText decoded{d_text, nbytes, d_tile_cnt, n_text, n, d_cps, d_cls, bits, text_only};
  for (int attempt = 0;; attempt++) {
    Arena ab(&c->b_buf, guard);
    try {
      if (sigma <= 255) {
        LinearPath<uint8_t>(v, c, S, ab, aa, decoded, offs_unit, rows, nmap).run(n_ids_out);
      } else {
        LinearPath<uint32_t>(v, c, S, ab, aa, decoded, offs_unit, rows, nmap).run(n_ids_out);
      }
      S.list_retries = attempt;
      return;
    } catch (const ListOverflow &o) {
      // the needed list of round 0 did not fit the room it was given (an eighth of the text, or what the last encode on
      // this context needed): nothing ran on the list — once more from the symbols on, with room for what it asked for
      if (attempt >= 2) throw HipError("needed list overflow after a retry (internal error)");
      WP_HIP(hipStreamSynchronize(c->stream));
      WP_HIP(hipStreamSynchronize(c->stream2));
      c->list_hint = o.wanted;
      reset_radix_stats(c);
      clear_scalars(c, kScalarListEntries, kScalarWideWords, st);  // (list sizes, overflow flag, walk counters)
    }
  }
}

}  // namespace wp
