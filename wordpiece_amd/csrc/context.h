// context.h — what a vocabulary handle owns on a device: streams, vocabulary tables, bump arenas, the pool of parked
// contexts (the C ABI itself is in encoder.hip; the device path in linear_path.h and fast_path.h, the layers on top of
// it in rows_path.h, inputs_path.h, mask_path.h, detok_path.h, pack_path.h, special_path.h, align_path.h, count_path.h, learn_path.h, dedup_path.h, neardup_path.h, overlap_path.h, repeat_path.h and quality_path.h).
#pragma once
#include <array>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/wordpiece_amd.h"
#include "code.h"
#include "decode.h"
#include "detok.h"
#include "packing.h"
#include "radix_sort.h"
#include "special.h"
#include "scanline.h"
#include "suffix_array.h"
#include "vocab.h"

namespace wp {

static thread_local std::string g_last_error;

// The environment switches of the library, read once per process (every other choice is an option of the handle,
// include/wordpiece_amd.h): debugging aids and process-wide defaults of tested behaviours, nothing that tunes.
struct EnvOptions {
  bool arena_guard;   // WP_ARENA_GUARD=1: guard zones behind every arena allocation, for every handle
  bool vocab_in_s;    // WP_VOCAB_IN_S=1: the reference's S = text . 1 . vocab layout, for every handle
  bool sparse_emit;   // WP_SPARSE_EMIT=1: ids through the per-position array, for every handle
  bool no_pool;       // WP_NO_CONTEXT_POOL=1: destroyed handles do not park their contexts
  static bool flag(const char *name) {
    const char *e = getenv(name);
    return e && atoi(e) != 0;
  }
  static const EnvOptions &get() {
    static const EnvOptions o{flag("WP_ARENA_GUARD"), flag("WP_VOCAB_IN_S"), flag("WP_SPARSE_EMIT"), flag("WP_NO_CONTEXT_POOL")};
    return o;
  }
};

struct DeviceBuffer {
  void *p = nullptr;
  size_t cap = 0;
  // slack: room for a somewhat larger next text without another hipFree / hipMalloc
  void ensure(size_t bytes, bool slack = true) {
    if (bytes <= cap) return;
    if (p) WP_HIP(hipFree(p));
    p = nullptr;
    cap = 0;
    size_t want = slack ? bytes + bytes / 16 + (1 << 20) : bytes;
    WP_HIP(hipMalloc(&p, want));
    cap = want;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
};

// A text in device memory.  The decoder reads 16 bytes at a time and ahead of the end of the text: the buffer of a text of
// `len` bytes has room for text_room(len), and holds 32 zero bytes from len & ~15 on (queued in front of the copy of the
// text, which overwrites the first len & 15 of them).
static size_t text_room(size_t len) { return len + 64; }
static void zero_text_tail(void *d_text, size_t len, hipStream_t st) {
  WP_HIP(hipMemsetAsync(static_cast<char *>(d_text) + (len & ~static_cast<size_t>(15)), 0, 32, st));
}

// Guard zones (WP_OPT_ARENA_GUARD / env WP_ARENA_GUARD=1, a debugging aid): every arena allocation is
// followed by kGuardBytes of a fixed pattern; after the encode a kernel checks that every zone is
// intact, i.e. that no kernel wrote past the end (or before the start) of the buffer it was given.
constexpr size_t kGuardBytes = 256;
constexpr uint32_t kGuardWord = 0xA5C3F00Du;

__global__ __launch_bounds__(kBlock) void guard_fill_kernel(char *base, const unsigned long long *offs, int count) {
  const int z = blockIdx.x;
  if (z >= count) return;
  uint32_t *g = reinterpret_cast<uint32_t *>(base + offs[z]);
  if (threadIdx.x < kGuardBytes / 4) g[threadIdx.x] = kGuardWord;
}
// bad[0] = number of damaged zones, bad[1] = 1 + index of the first one
__global__ __launch_bounds__(kBlock) void guard_check_kernel(const char *base, const unsigned long long *offs, int count,
                                                             uint32_t *bad) {
  const int z = blockIdx.x;
  if (z >= count) return;
  const uint32_t *g = reinterpret_cast<const uint32_t *>(base + offs[z]);
  const bool broken = threadIdx.x < kGuardBytes / 4 && g[threadIdx.x] != kGuardWord;
  if (__syncthreads_or(broken) && threadIdx.x == 0) {
    atomicAdd(&bad[0], 1u);
    atomicMin(&bad[1], static_cast<uint32_t>(z) + 1u);
  }
}

// bump allocator over a DeviceBuffer: plan() first with the same sequence of take() calls
struct Arena {
  DeviceBuffer *buf;
  size_t off = 0, planned = 0;
  bool planning = true, guard = false;
  std::vector<unsigned long long> zones;  // byte offsets of the guard zones (guard mode)
  explicit Arena(DeviceBuffer *b, bool g = false) : buf(b), guard(g) {}
  template <typename T>
  T *take(size_t count) {
    size_t bytes = (count * sizeof(T) + 255) & ~static_cast<size_t>(255);
    size_t o = off;
    off += bytes;
    if (guard) {
      if (!planning) zones.push_back(off);
      off += kGuardBytes;
    }
    if (planning) return nullptr;
    // (the two rounds of take() must ask for the same sizes: a layout decided by a pointer that is null while planning
    // would hand out memory behind the buffer)
    if (off > planned) throw std::logic_error("arena: the allocation sequence differs from the planned one");
    return reinterpret_cast<T *>(static_cast<char *>(buf->p) + o);
  }
  void commit() {
    buf->ensure(off + (guard ? 8 * 512 : 0));  // (guard mode: room for the zone table behind the arena)
    planned = off;
    off = 0;
    planning = false;
  }
  // the zone table lives behind the last allocation; call after the second (real) round of take()s
  unsigned long long *zone_table() const {
    return reinterpret_cast<unsigned long long *>(static_cast<char *>(buf->p) + ((off + 255) & ~static_cast<size_t>(255)));
  }
  void arm(hipStream_t st) {
    if (!guard || zones.empty()) return;
    if (zones.size() > 500) throw std::logic_error("arena guard: too many allocations");
    WP_HIP(hipMemcpyAsync(zone_table(), zones.data(), zones.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, st));
    WP_HIP(hipStreamSynchronize(st));
    hipLaunchKernelGGL(guard_fill_kernel, dim3(zones.size()), dim3(kBlock), 0, st, static_cast<char *>(buf->p), zone_table(),
                       static_cast<int>(zones.size()));
  }
  // bad: 2 device words, cleared by the caller to {0, 0xffffffff}
  void check(hipStream_t st, uint32_t *bad) const {
    if (!guard || zones.empty()) return;
    hipLaunchKernelGGL(guard_check_kernel, dim3(zones.size()), dim3(kBlock), 0, st, static_cast<const char *>(buf->p),
                       zone_table(), static_cast<int>(zones.size()), bad);
  }
};

static int bit_length(uint64_t v) {
  int b = 0;
  while (v) {
    b++;
    v >>= 1;
  }
  return b;
}

// ---- the device scalar block ----------------------------------------------------------------------------------------
// c->d_scalars: kScalars 32-bit words that kernels and scans leave their totals in; c->h_scalars: the pinned mirror the
// host reads them from.  Every word has a name here and nowhere else; no call site names a number.  An encode clears
// the whole block when it starts (and the pre-pass of WP_OPT_NORMALIZE in front of it does the same, see below).
constexpr int kScalars = 252;
constexpr int kScalarCps = 0;       // code points of the text, 32 bits: the decode scan (linear, fast) -> host
constexpr int kScalarAlphabet = 1;  // alphabet size: alphabet_prefix_kernel -> host
constexpr int kScalarInvalid = 2;   // invalid sequences, 64 bits (words 2, 3): decode_count_kernel / norm_count_kernel -> host
// The active list of the refinement (linear_path.h).  The kernels are given d_scalars + kScalarList (needed_list_*,
// group_starts, trie and sort kernels), + kScalarListGroups or + kScalarListLargeGroups (large_groups_*) and index from
// there; NeededList takes words 0, 1 of the block as one 64-bit word, large_groups_kernel words 2, 3.
constexpr int kScalarList = 4;
constexpr int kScalarListEntries = kScalarList + 0;       // entries of the list -> host after every round
constexpr int kScalarListGroups = kScalarList + 1;        // its groups -> host (trie round)
constexpr int kScalarListLargeGroups = kScalarList + 2;   // groups too large for the LDS sort: classify_groups -> host
constexpr int kScalarListLargeEntries = kScalarList + 3;  // their entries
constexpr int kScalarListWanted = 8;  // the length the needed list asked for: needed_list_clamp_kernel -> host (ListOverflow)
constexpr int kScalarIds = 9;         // number of ids: the emit scan (linear, fast) -> host
constexpr int kScalarAnchors = 10;    // number of anchors: the anchor scan -> the walk kernels and the host
constexpr int kScalarAnchorGap = 11;  // largest anchor gap: anchor_gap kernels -> host
constexpr int kScalarLongWords = 12;  // long words: long_word_collect kernels -> host
constexpr int kScalarWideWords = 13;  // wide words: wide_collect / walk_wide kernels -> host (cleared only when that branch runs)
constexpr int kScalarCps64 = 14;      // code points of the text, 64 bits (words 14, 15): the decode scan -> host (size limit)
constexpr int kScalarGuard = 16;      // arena guard (guard_check_kernel gets + kScalarGuard, host writes {0, ~0} first):
constexpr int kScalarGuardBad = kScalarGuard + 0;    //   damaged zones -> host
constexpr int kScalarGuardFirst = kScalarGuard + 1;  //   1 + index of the first one -> host
constexpr int kScalarSplitTotals = 18; // words 18, 19: the totals of the trie round's split where it runs early (refine_early: the
                                       // list sizes in kScalarList are still read then); not read by the host, inside the download behind the walk
constexpr int kScalarAlphaWord0 = 20;  // first word of the text's alphabet bitmap before the vocabulary marks it: copy -> host
// documents calls (rows.h): lines of the text / boundaries of explicit rows that fail the check / rows a padded call cut
constexpr int kScalarRows = 21, kScalarRowsBad = 22, kScalarRowsCut = 23;
constexpr int kScalarCand = 24;  // d_scalars word: entries of the keys-only round 0's candidate list (linear_path.h)
constexpr int kScalarKept = 25;  // d_scalars word: suffixes the keys-only round 0 kept (not blank-start; radix_sort.h, RadixDrop)
constexpr int kScalarSrcRows = 26;  // lines of the caller's text in a documents call on normalised text (normalize.h)
// model inputs (inputs.h): samples that lost ids / the number of output rows, 64 bits (words 28, 29) / samples with windows
constexpr int kScalarInCut = 27, kScalarInRows = 28, kScalarInWindowed = 30;
constexpr int kScalarSpecial = 31;  // special tokens (special.h): the literals of the text, the total of their scan -> host
constexpr int kScalarMask = 32;    // d_scalars words 32..43: the six 64-bit counters of a mask call (mask.h, MaskCounter)
// detokenize (detok.h): the last entry of row_splits given in device memory, 64 bits (words 44, 45) / its violations
constexpr int kScalarDetokLast = 44, kScalarDetokBad = 46;
constexpr int kScalarFree47 = 47;  // free
constexpr int kScalarDetok = 48;   // d_scalars words 48..55: the four 64-bit totals of a detokenize call (detok.h, DetokCounter)
// packing (packing.h): the last entry of row_splits as the check kernel read it, 64 bits (words 56, 57) / its violations
constexpr int kScalarPackLast = 56, kScalarPackBad = 58;
constexpr int kScalarFree59 = 59;  // free
constexpr int kScalarPack = 60;    // d_scalars words 60..75: the eight 64-bit totals of a pack call (packing.h, PackCounter)
// span alignment (align.h): what the argument check found, one 64-bit word (words 76, 77; align_bad_key) / the five 64-bit
// counters of a call (words 78..87, AlignCounter)
constexpr int kScalarAlignBad = 76, kScalarAlign = 78;
// word counts (count.h): the words of the text, 64 bits (words 88, 89) / the listed ones / the runs and the leftovers of
// a round / the kept groups / the 64-bit counters of a call (words 94, 95, CountCounter)
constexpr int kScalarCountWords = 88, kScalarCountListed = 90, kScalarCountRuns = 91, kScalarCountLeft = 92, kScalarCountKept = 93;
constexpr int kScalarCount = 94;
// vocabulary learner (learn.h): what the table check found, 64 bits (words 96, 97; ~0: nothing) / the substring occurrences,
// 64 bits (words 98, 99) / the character cells / the characters / the runs and the leftovers of a grouping round / the
// kept tokens of an iteration / the bytes of the list / the 64-bit counters of a call (words 106..113, LearnCounter)
constexpr int kScalarLearnBad = 96, kScalarLearnItems = 98, kScalarLearnCells = 100, kScalarLearnChars = 101, kScalarLearnRuns = 102;
constexpr int kScalarLearnLeft = 103, kScalarLearnKept = 104, kScalarLearnOutBytes = 105, kScalarLearn = 106;
// duplicate rows (dedup.h): the first row whose offsets fail the check (~0: none) / the runs of a round / row_off[n_rows],
// 64 bits (words 116, 117) / the chunks of the call, then of the next round, 64 bits (words 118, 119) / the leftovers of a
// round, and the bytes of the compact form when the call ends / the kept rows / the 64-bit counters of a call (words
// 122..129, DedupCounter)
constexpr int kScalarDedupBad = 114, kScalarDedupRuns = 115, kScalarDedupElems = 116, kScalarDedupChunks = 118, kScalarDedupLeft = 120;
constexpr int kScalarDedupUnique = 121, kScalarDedup = 122;
// near-duplicate rows (neardup.h): the first row whose offsets fail the check (~0: none) / the runs of the grouping /
// row_off[n_rows], 64 bits (words 132, 133) / the shingle positions, 64 bits (words 134, 135) / the edges / whether a
// component round lowered a label / the kept rows / the bytes of the compact form / the 64-bit counters of a call (words
// 140..147, NearCounter)
constexpr int kScalarNearBad = 130, kScalarNearRuns = 131, kScalarNearElems = 132, kScalarNearPositions = 134, kScalarNearEdges = 136;
constexpr int kScalarNearChanged = 137, kScalarNearUnique = 138, kScalarNearOutBytes = 139, kScalarNear = 140;
// n-gram overlap (overlap.h): the first bad row of the corpus and of the reference set (~0: none) / row_off[n_rows] and
// ref_off[n_ref], 64 bits each (words 150..153) / the windows of both, 64 bits each (words 154..157) / the runs of the
// reference sort / the table entries / the candidates / the hits / the covered elements / the kept rows / the bytes of
// the compact form / a free word / the 64-bit counters of a call (words 166..173, OvlCounter)
constexpr int kScalarOvlBad = 148, kScalarOvlRefBad = 149, kScalarOvlElems = 150, kScalarOvlRefElems = 152, kScalarOvlWindows = 154;
constexpr int kScalarOvlRefWindows = 156, kScalarOvlRuns = 158, kScalarOvlEntries = 159, kScalarOvlCands = 160, kScalarOvlHits = 161;
constexpr int kScalarOvlCovered = 162, kScalarOvlKept = 163, kScalarOvlOutBytes = 164, kScalarFree165 = 165, kScalarOvl = 166;
// repeated spans (repeat.h): the first bad row (~0: none) / the runs of the window sort / row_off[n_rows], 64 bits (words
// 176, 177) / the windows, 64 bits (words 178, 179) / the listed (eligible) windows / the distinct windows / the repeats /
// the covered elements / the kept rows / the bytes of the compact form / the 64-bit counters of a call (words 186..193,
// RepCounter)
constexpr int kScalarRepBad = 174, kScalarRepRuns = 175, kScalarRepElems = 176, kScalarRepWindows = 178, kScalarRepListed = 180;
constexpr int kScalarRepDistinct = 181, kScalarRepRepeats = 182, kScalarRepCovered = 183, kScalarRepKept = 184, kScalarRepOutBytes = 185;
constexpr int kScalarRep = 186;
// quality signals (quality.h): the first bad row (~0: none) / the kept rows / row_off[n_rows], 64 bits (words 196, 197) /
// what the shared row kernel counts as windows, 64 bits (words 198, 199: the bytes again, not read) / the words / the
// lines / the bytes of the compact form / a free word / the 64-bit counters of a call (words 204..251, QualCounter)
constexpr int kScalarQualBad = 194, kScalarQualKept = 195, kScalarQualElems = 196, kScalarQualWindows = 198, kScalarQualWords = 200;
constexpr int kScalarQualLines = 201, kScalarQualOutBytes = 202, kScalarFree203 = 203, kScalarQual = 204;
// normalize_on_device runs in front of the encode, which clears the block again: while it runs, four slots mean
constexpr int kScalarNormBytes = kScalarCps;           // bytes of the normalised text, 32 bits: its scan
constexpr int kScalarNormCps = kScalarAlphabet;        // code points of the normalised text (offsets mode) -> host
constexpr int kScalarNormSrcCps = kScalarListEntries;  // code points of the source text (offsets mode)
constexpr int kScalarNormBytes64 = kScalarCps64;       // bytes of the normalised text, 64 bits -> host
// (kScalarInvalid keeps its meaning there)

// the table in order: {first word, words}; a range of an even number of words holds 64-bit values
struct ScalarRange {
  int first, words;
};
constexpr ScalarRange kScalarLayout[] = {
    {kScalarCps, 1},         {kScalarAlphabet, 1},   {kScalarInvalid, 2},         {kScalarListEntries, 1},
    {kScalarListGroups, 1},  {kScalarListLargeGroups, 1}, {kScalarListLargeEntries, 1}, {kScalarListWanted, 1},
    {kScalarIds, 1},         {kScalarAnchors, 1},    {kScalarAnchorGap, 1},       {kScalarLongWords, 1},
    {kScalarWideWords, 1},   {kScalarCps64, 2},      {kScalarGuardBad, 1},        {kScalarGuardFirst, 1},
    {kScalarSplitTotals, 2},      {kScalarAlphaWord0, 1}, {kScalarRows, 1},            {kScalarRowsBad, 1},
    {kScalarRowsCut, 1},     {kScalarCand, 1},       {kScalarKept, 1},            {kScalarSrcRows, 1},
    {kScalarInCut, 1},       {kScalarInRows, 2},     {kScalarInWindowed, 1},      {kScalarSpecial, 1},
    {kScalarMask, 12},       {kScalarDetokLast, 2},  {kScalarDetokBad, 1},        {kScalarFree47, 1},
    {kScalarDetok, 8},       {kScalarPackLast, 2},   {kScalarPackBad, 1},         {kScalarFree59, 1},
    {kScalarPack, 16},       {kScalarAlignBad, 2},   {kScalarAlign, 10},
    {kScalarCountWords, 2},  {kScalarCountListed, 1}, {kScalarCountRuns, 1},      {kScalarCountLeft, 1},
    {kScalarCountKept, 1},   {kScalarCount, 2},
    {kScalarLearnBad, 2},    {kScalarLearnItems, 2},  {kScalarLearnCells, 1},     {kScalarLearnChars, 1},
    {kScalarLearnRuns, 1},   {kScalarLearnLeft, 1},   {kScalarLearnKept, 1},      {kScalarLearnOutBytes, 1},
    {kScalarLearn, 8},
    {kScalarDedupBad, 1},    {kScalarDedupRuns, 1},   {kScalarDedupElems, 2},     {kScalarDedupChunks, 2},
    {kScalarDedupLeft, 1},   {kScalarDedupUnique, 1}, {kScalarDedup, 8},
    {kScalarNearBad, 1},     {kScalarNearRuns, 1},    {kScalarNearElems, 2},      {kScalarNearPositions, 2},
    {kScalarNearEdges, 1},   {kScalarNearChanged, 1}, {kScalarNearUnique, 1},     {kScalarNearOutBytes, 1},
    {kScalarNear, 8},
    {kScalarOvlBad, 1},      {kScalarOvlRefBad, 1},   {kScalarOvlElems, 2},       {kScalarOvlRefElems, 2},
    {kScalarOvlWindows, 2},  {kScalarOvlRefWindows, 2}, {kScalarOvlRuns, 1},      {kScalarOvlEntries, 1},
    {kScalarOvlCands, 1},    {kScalarOvlHits, 1},     {kScalarOvlCovered, 1},     {kScalarOvlKept, 1},
    {kScalarOvlOutBytes, 1}, {kScalarFree165, 1},     {kScalarOvl, 8},
    {kScalarRepBad, 1},      {kScalarRepRuns, 1},     {kScalarRepElems, 2},       {kScalarRepWindows, 2},
    {kScalarRepListed, 1},   {kScalarRepDistinct, 1}, {kScalarRepRepeats, 1},     {kScalarRepCovered, 1},
    {kScalarRepKept, 1},     {kScalarRepOutBytes, 1}, {kScalarRep, 8},
    {kScalarQualBad, 1},     {kScalarQualKept, 1},    {kScalarQualElems, 2},      {kScalarQualWindows, 2},
    {kScalarQualWords, 1},   {kScalarQualLines, 1},   {kScalarQualOutBytes, 1},   {kScalarFree203, 1},
    {kScalarQual, 48}};
// one past the last word of the range `slot` lies in: where a download or a clear "through" that slot ends
constexpr int scalar_end(int slot) {
  for (const ScalarRange &r : kScalarLayout) {
    if (slot < r.first + r.words) return r.first + r.words;
  }
  return kScalars;
}
// every word belongs to exactly one range (no gap, no overlap, nothing past kScalars); 64-bit values are 8-byte aligned
constexpr bool scalar_layout_ok() {
  int at = 0;
  for (const ScalarRange &r : kScalarLayout) {
    if (r.first != at || r.words < 1 || (r.words % 2 == 0 && r.first % 2 != 0)) return false;
    at += r.words;
  }
  return at == kScalars;
}
static_assert(scalar_layout_ok(), "the scalar table must cover d_scalars word by word, 64-bit slots on even words");
static_assert(kScalarList % 2 == 0 && kScalarListLargeGroups % 2 == 0, "both halves of the list block are also read as 64-bit words");

// A documents call (wp_linear_encode_rows / _padded) as encode_on_device sees it: how the rows are given, and where it
// left the row structure (device pointers into the arenas, valid like c->d_ids until the handle's next call).
struct RowsCall {
  const long long *d_doc_off = nullptr;  // explicit rows: n_docs + 1 starts in device memory; nullptr: the lines of the text
  size_t n_docs = 0;
  int unit = -1;                   // unit of the offsets the caller asked for (-1: none; the spans are then left in code points)
  size_t capacity = SIZE_MAX;      // rows the caller has room for: more is std::invalid_argument once the count is known
  size_t n_rows = 0;               // out: the number of rows (set before the capacity check)
  const long long *d_starts = nullptr;      // out: n_rows + 1 document starts in bytes
  const long long *d_row_splits = nullptr;  // out: n_rows + 1
  uint32_t *d_line_cnt = nullptr;  // lines mode: line ends per tile, scanned (phase A arena)
};

// c->evs: the events that order the streams of an encode (no timing)
//   kEvFork / kEvJoin          the side stream may start / is done
//   kEvScalars                 the scalars of a refinement round are in the pinned mirror
//   kEvKeysFree                the side stream is done with the sorted keys
//   kEvPartition               the partition passes are queued
//   kEvTrieNodes               the trie nodes of the groups are known
//   kEvLargeSorted             the large groups are sorted
//   kEvKeysBuilt               the key builder is done
//   kEvCandCount               the candidate count is in the pinned mirror
//   kEvSpine / kEvKept         the spine of round 0's first pass is done / its kept count is in the pinned mirror
//   kEvSorted                  the last pass of round 0 is done (early refinement: the side stream's anchor list waits for it)
//   kEvListBuilt               early refinement: the needed list is built (the late half may overwrite the tokens' cells)
//   kEvRoundDone               early refinement: the trie round's split is done (the rank scatter may start; the side
//                              stream goes on with the anchor list, which kEvJoin covers at the walk)
//   kEvAnchorScalars           the anchor count and the largest anchor gap are in the pinned mirror (side stream, directly
//                              behind the anchor list: the host waits for it alone before it queues the walk)
//   kEvMarks / kEvCovered      scanline stage, key lookup: the marks are written (main stream) / their cover scan is done
//                              (second side stream, beside the step starts and their sort)
//   kEvStartsSorted / kEvTablesIndexed  the step starts are sorted (main stream) / the bucket indices, kstart and the flags
//                              of the needed groups are built (second side stream, beside the step values)
//   kEvRankStored              early refinement, key lookup: the rank scatter (main stream) has set kClsRanked in the class
//                              bytes of the needed list; the side stream's anchor_write_kernel, which rewrites them, waits
enum SideEvent { kEvFork, kEvJoin, kEvScalars, kEvKeysFree, kEvPartition, kEvTrieNodes, kEvLargeSorted, kEvKeysBuilt, kEvCandCount,
                 kEvSpine, kEvKept, kEvSorted, kEvListBuilt, kEvRoundDone, kEvAnchorScalars,
                 kEvMarks, kEvCovered, kEvStartsSorted, kEvTablesIndexed, kEvRankStored, kSideEvents };
// c->ev: the marks of WP_OPT_STAGE_TIMING in the order an encode passes them: its start / code points counted / symbols,
// classes and keys written / suffix array refined / LCP / scanlines / walk (the fast path: start, counted, symbols,
// walked).  normalize_on_device: its start, and its end in the mark the encode behind it records next.
// kMarkRound0: behind the last pass of the round-0 sort (wp_refine_sched.ms_sort_to_scan runs from there to kMarkLcp).
enum TimingMark { kMarkStart, kMarkCounted, kMarkSymbols, kMarkSorted, kMarkLcp, kMarkScanned, kMarkWalked, kMarkNormStart,
                  kMarkRound0, kTimingMarks, kMarkNormEnd = kMarkStart };

struct Context {
  int device = 0;
  hipStream_t stream = nullptr;
  hipStream_t stream2 = nullptr;  // side stream: latency-bound helpers overlap the bandwidth-bound kernels
  hipStream_t stream3 = nullptr;  // second side stream: the large-group path of the trie round beside its LDS sort
  hipEvent_t evs[kSideEvents] = {};  // order between the streams of an encode (SideEvent)
  // vocab tables on the device
  uint32_t *d_stream = nullptr, *d_elig_start = nullptr, *d_elig_info = nullptr, *d_soft = nullptr;
  uint32_t *d_vocab_word_idx = nullptr, *d_vocab_word_bits = nullptr;  // the vocabulary's words of the alphabet bitmap
  uint8_t *d_cls_bmp = nullptr;                                         // class byte of every BMP code point
  uint32_t *d_lt_chain_len = nullptr, *d_lt_chain_off = nullptr, *d_lt_child_begin = nullptr, *d_lt_child_cp = nullptr,
           *d_lt_child_node = nullptr, *d_elig_node = nullptr, *d_elig_subtree = nullptr;  // the token trie (vocab.h, trie.h)
  int32_t *d_elig_id = nullptr, *d_tok_len = nullptr;
  uint8_t *d_tok_class = nullptr;  // wp_vocab_token_flags of every id, one byte each: uploaded by the first mask call (mask.h)
  // the pieces of every id, uploaded by the first detokenize call (detok.h): records [cleanup][form][id] and their bytes
  DetokRec *d_detok_rec = nullptr;
  uint8_t *d_detok_pool = nullptr;
  size_t detok_pool_bytes = 0;
  unsigned long long *d_trie_key = nullptr;  // the fast path's token trie (vocab.h)
  uint32_t *d_trie_child = nullptr;
  int32_t *d_trie_id = nullptr;
  DeviceBuffer text_buf, a_buf, b_buf, fmt_buf;  // fmt_buf: id text of encodeExternal
  // wp_linear_encode_batch: second text buffer, two id staging buffers and the copy streams of the shard pipeline
  DeviceBuffer text_buf2, ids_stage[2];
  // documents calls: explicit row starts of a host call, results of the per-document route, padded batch of a host call
  DeviceBuffer rows_in, rows_out, pad_buf;
  DeviceBuffer inputs_buf;  // model inputs: window counts and records per sample (inputs.h)
  // detokenize (detok.h): ids and rows of a host call, tile records and offsets, the text and text_off of the last call
  DeviceBuffer detok_in, detok_aux, detok_out;
  // packing (packing.h): ids and row_splits of a host call, the per-document plan, the per-piece tables and row starts,
  // the batch of a host call
  DeviceBuffer pack_in, pack_plan, pack_tab, pack_out;
  // special tokens (special.h): the blanked copy of the text, the listed lines and the tile counts of the match, the
  // literal list, and the merged result with the tables its placement needs
  DeviceBuffer special_text, special_in, special_lit, special_out;
  // word counts (count.h): the tile counts of the word-start pass, the per-word and per-group arrays of the rounds, and
  // the table of the last call (the counted text itself is in norm_buf)
  DeviceBuffer count_aux, count_words, count_out;
  // vocabulary learner (learn.h): the table and the reserved tokens of a host call, the per-word and per-character
  // arrays, the per-occurrence arrays of the grouping, the per-token arrays of the search, and the list of the last call
  DeviceBuffer learn_in, learn_aux, learn_items, learn_groups, learn_out;
  // duplicate rows (dedup.h): the data and the offsets of a host call, the per-row arrays of the rounds (with `first`
  // of the last call), and the table and the compact form of the last call
  DeviceBuffer dedup_in, dedup_rows, dedup_out;
  // near-duplicate rows (neardup.h): the data and the offsets of a host call, the per-row arrays (with the signatures
  // and `cluster` of the last call), the per-item arrays of the grouping and the edge list, and the table and the
  // compact form of the last call
  DeviceBuffer neardup_in, neardup_rows, neardup_items, neardup_out;
  // n-gram overlap (overlap.h): the data and the offsets of both batches of a host call, the per-row arrays of both (with
  // hits, first_hit, first_ref, covered and ref_hits of the last call), the per-element and per-window arrays of the
  // table and the lookup (with mask), and the compact form of the last call
  DeviceBuffer overlap_in, overlap_ref_in, overlap_rows, overlap_items, overlap_out;
  // repeated spans (repeat.h): the data and the offsets of a host call, the per-row arrays (with repeats, first_repeat,
  // first_src_row, first_src_pos and covered of the last call), the per-element and per-window arrays (with mask and
  // src), and the cut and the compact form of the last call
  DeviceBuffer repeat_in, repeat_rows, repeat_items, repeat_out;
  // quality signals (quality.h): the data and the offsets of a host call, the per-row arrays (with signals and reasons
  // of the last call), the tile counts and the stop table, the per-word and per-line lists with the arrays of the
  // duplicate-line stage, and the compact form of the last call; the class table (uploaded with the first quality call)
  DeviceBuffer quality_in, quality_rows, quality_items, quality_lists, quality_out;
  uint16_t *d_class_index = nullptr;
  uint8_t *d_class_pages = nullptr;
  // WP_OPT_NORMALIZE (normalize.h): the tables (uploaded with the first normalising call), the normalised text, the
  // tile counts of the pre-pass, and the source of every normalised code point (offsets mode)
  uint16_t *d_norm_index = nullptr;
  uint32_t *d_norm_pages = nullptr, *d_norm_pool = nullptr;
  DeviceBuffer norm_buf, norm_aux, norm_map;
  hipStream_t up_stream = nullptr, down_stream = nullptr;
  hipEvent_t pipe_ev[4] = {};  // ids staged [2], ids downloaded [2]
  uint32_t *d_used = nullptr, *d_lut = nullptr, *d_scan_tmp = nullptr;  // bitmap of the code points in use (kCpWords), lut (kCpTableSize), per-word prefixes (kCpWords)
  uint32_t *d_scalars = nullptr;                                         // kScalars words of device scalars
  uint8_t *d_code = nullptr;     // symbol code tables: cw u16[256] | len u8[256] | bmask u16[4096]
  // The symbol code of the last encode, kept while the alphabet size stays the same: ANY order-preserving code over
  // the dense symbol ids 0..sigma is correct (the histogram only steers the codeword lengths), so consecutive
  // shards / batches of one corpus reuse it and skip the histogram download, the host-side construction and the
  // table upload — one host round trip less per encode.  Rebuilt every kCodeReuse encodes to follow the text.
  size_t list_hint = 0;  // entries the needed list of the last encode held (sizes the list arenas of the next one)
  SymbolCode code_cache;
  bool code_cached = false;
  uint32_t code_alphabet = 0;
  int code_bits = 0, code_lo = 0, code_uses = 0;
  // share of blanks in the histogram the cached code was built from (8-bit symbols): whether the keys-only round 0
  // leaves the blank-start suffixes out (linear_path.h, kBlankDropMinShare) — a speed decision only, never a result
  double code_blank_share = 0.0;
  uint8_t *h_code = nullptr;     // pinned staging of the same (the upload needs no host wait: every encode ends with one)
  uint32_t *d_symhist = nullptr;  // 256 counters
  uint32_t *h_scalars = nullptr;                                         // pinned mirror
  RadixStats rstats;
  hipEvent_t ev[kTimingMarks] = {};  // WP_OPT_STAGE_TIMING (TimingMark)
  // results / debug views of the last call (device pointers into the arenas)
  const int32_t *d_ids = nullptr;
  const uint32_t *d_offs = nullptr;  // offsets mode: [begin, end) per id (linear_path.h, offsets.h)
  struct {
    const void *sym = nullptr;
    int sym_bytes = 0;
    const uint32_t *sa = nullptr, *cps = nullptr;
    const RankEntry *rank = nullptr;
    const int32_t *lcp = nullptr;
    const uint8_t *cls = nullptr;  // class byte per text position (n_text; kept only with WP_OPT_KEEP_DEBUG)
    StepTable steps{};
    int32_t *best_scratch = nullptr;  // room for 2n int32 (debug expansion of the step functions)
    const int32_t *step_views = nullptr;  // WP_OPT_KEEP_DEBUG = 2: 4 x n_text (ids prefix / ##, lengths prefix / ##) by text position
    size_t n = 0, n_text = 0;
  } dbg;
  // every DeviceBuffer above, for destroy_context, release_arenas and park_context: a new buffer is one more name here
  std::array<DeviceBuffer *, 54> buffers() {
    return {&text_buf, &a_buf,    &b_buf,   &fmt_buf,    &text_buf2, &ids_stage[0], &ids_stage[1], &rows_in,   &rows_out,
            &pad_buf,  &inputs_buf, &norm_buf, &norm_aux, &norm_map, &detok_in,     &detok_aux,    &detok_out,
            &pack_in,  &pack_plan,  &pack_tab, &pack_out, &special_text, &special_in, &special_lit, &special_out,
            &count_aux, &count_words, &count_out, &learn_in, &learn_aux, &learn_items, &learn_groups, &learn_out,
            &dedup_in, &dedup_rows, &dedup_out, &neardup_in, &neardup_rows, &neardup_items, &neardup_out,
            &overlap_in, &overlap_ref_in, &overlap_rows, &overlap_items, &overlap_out,
            &repeat_in, &repeat_rows, &repeat_items, &repeat_out,
            &quality_in, &quality_rows, &quality_items, &quality_lists, &quality_out};
  }
  Context() = default;
  Context(const Context &) = delete;
  Context &operator=(const Context &) = delete;
  ~Context();  // releases whatever was built (a half-built context of a failed make_context included)
};

// The calling thread's current HIP device, put back when the scope ends: no entry point of the C ABI leaves the
// caller on another device than it came in with (a host process — PyTorch, say — keeps allocating on "its" GPU).
struct DeviceGuard {
  int prev = -1;
  DeviceGuard() {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
  DeviceGuard(const DeviceGuard &) = delete;
  DeviceGuard &operator=(const DeviceGuard &) = delete;
};

#ifdef WP_DEBUG_BOUNDS
// the bounds-checking build: reads the counters of `count` sites from `first` on into oob (the kernels that count there
// are over) and, where any counted, clears them for the next call
static void take_oob(int first, int count, unsigned int *oob) {
  WP_HIP(hipMemcpyFromSymbol(oob, HIP_SYMBOL(g_wp_oob), count * sizeof(unsigned int), first * sizeof(unsigned int)));
  bool any = false;
  for (int i = 0; i < count; i++) any = any || oob[i] != 0;
  if (!any) return;
  const unsigned int zero[kCountedSites] = {};
  WP_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_wp_oob), zero, count * sizeof(unsigned int), first * sizeof(unsigned int)));
}
#endif
// behind the last kernel of a layer's call: the bounds-checking build fails the call where the kernels skipped an access
// at `site` (the release build counts nothing)
static void throw_if_oob(int site, const char *layer, const char *skipped) {
#ifdef WP_DEBUG_BOUNDS
  unsigned int oob = 0;
  take_oob(site, 1, &oob);
  if (oob != 0) throw HipError(std::string("debug bounds: ") + layer + ": " + std::to_string(oob) + " " + skipped);
#endif
}

}  // namespace wp

using namespace wp;

// the statistics of an encode as the device path fills them: wp_stats and, behind it, what wp_get_norm_stats and
// wp_get_walk_stats / wp_get_refine_stats hand out
struct EncodeStats : wp_stats {
  int32_t normalize;
  int64_t norm_bytes;
  double ms_normalize;
  wp_walk_stats walk;
  wp_refine_stats refine;  // which refinement ran (linear_path.h: trie_round_finish / doubling_rounds)
  wp_refine_sched sched;   // ... and where it was queued (linear_path.h: ranks_round0)
  wp_step_stats step;      // the step tables the walk read (linear_path.h: scanlines)
  wp_inputs_stats inputs;  // wp_get_inputs_stats: filled by an inputs call (inputs_call 1), zero otherwise
  int32_t inputs_call;
  wp_mask_stats mask;  // wp_get_mask_stats: filled by a mask or word-ids call (mask_call 1), zero otherwise
  int32_t mask_call;
  wp_detok_stats detok;  // wp_get_detok_stats: filled by a detokenize call (detok_call 1), zero otherwise
  int32_t detok_call;
  wp_pack_stats pack;  // wp_get_pack_stats: filled by a pack call (pack_call 1), zero otherwise
  int32_t pack_call;
  wp_special_stats special;  // wp_get_special_stats: filled by a special-tokens call (special_call 1), zero otherwise
  int32_t special_call;
  wp_align_stats align;  // wp_get_align_stats: filled by an align call (align_call 1), zero otherwise
  int32_t align_call;
  wp_count_stats count;  // wp_get_count_stats: filled by a count call (count_call 1), zero otherwise
  int32_t count_call;
  wp_learn_stats learn;  // wp_get_learn_stats: filled by a learn call (learn_call 1), zero otherwise
  int32_t learn_call;
  wp_dedup_stats dedup;  // wp_get_dedup_stats: filled by a dedup call (dedup_call 1), zero otherwise
  int32_t dedup_call;
  wp_neardup_stats neardup;  // wp_get_neardup_stats: filled by a neardup call (neardup_call 1), zero otherwise
  int32_t neardup_call;
  wp_overlap_stats overlap;  // wp_get_overlap_stats: filled by an overlap call (overlap_call 1), zero otherwise
  int32_t overlap_call;
  wp_repeat_stats repeat;  // wp_get_repeat_stats: filled by a repeat call (repeat_call 1), zero otherwise
  int32_t repeat_call;
  wp_quality_stats quality;  // wp_get_quality_stats: filled by a quality call (quality_call 1), zero otherwise
  int32_t quality_call;
};

#ifndef WP_LATE_REFINE_DEFAULT
#define WP_LATE_REFINE_DEFAULT 0
#endif

struct wp_vocab {
  HostVocab hv;
  std::unique_ptr<Context> ctx;                  // the handle's own device context
  std::vector<std::unique_ptr<Context>> multi;  // one per entry of the device list of wp_linear_encode_multi
  int device = -1;
  bool full_depth = false, keep_debug = false, stage_timing = false, lcp_kasai = false, cover_anchors = false;
  bool keep_step_views = false;  // WP_OPT_KEEP_DEBUG = 2: the step views by position, nothing else changes
  bool arena_guard = false;
  bool sparse_emit = false;  // WP_OPT_SPARSE_EMIT: ids through the per-position emit array even where per-workgroup lists would do
  bool vocab_in_s = false;  // WP_OPT_VOCAB_IN_S: always the reference's S = text . 1 . vocab layout
  bool indexed_round0 = false;  // WP_OPT_INDEXED_ROUND0: the (key, index) round-0 sort also where keys alone would do
  bool sort_blanks = false;     // WP_OPT_SORT_BLANKS: the keys-only round 0 sorts the blank-start suffixes too
  // WP_OPT_LATE_REFINE: the keys-only round 0 starts the refinement behind the sort, not beside it
  // (-DWP_LATE_REFINE_DEFAULT=1: a build whose handles start with it, for A/B runs of programs that set no options)
  bool late_refine = WP_LATE_REFINE_DEFAULT != 0;
  int normalize = 0;  // WP_OPT_NORMALIZE: WP_NORM_* flags of the pre-pass in front of every encode (normalize.h); 0: none
  int n_devices = 1;  // WP_OPT_DEVICES: GPUs wp_linear_encode shards a host buffer over (-1: all visible)
  EncodeStats stats{};
  ~wp_vocab();
};

namespace wp {

// hipFree of raw device pointers, each cleared as it is released
template <typename... T>
static void free_dev(T *&...p) {
  (((p ? (void)hipFree(p) : (void)0), p = nullptr), ...);
}

// the tables of a vocabulary: they go when the handle is destroyed (a parked context gets the next handle's); a new
// table is one more name here
static void free_vocab_tables(Context *c) {
  free_dev(c->d_stream, c->d_elig_start, c->d_elig_info, c->d_soft, c->d_elig_id, c->d_tok_len, c->d_tok_class, c->d_detok_rec, c->d_detok_pool, c->d_trie_key,
           c->d_trie_child, c->d_trie_id, c->d_vocab_word_idx, c->d_vocab_word_bits, c->d_cls_bmp, c->d_lt_chain_len,
           c->d_lt_chain_off, c->d_lt_child_begin, c->d_lt_child_cp, c->d_lt_child_node, c->d_elig_node, c->d_elig_subtree);
}

template <size_t N>
static void destroy_events(hipEvent_t (&events)[N]) {
  for (auto &e : events) {
    if (e) (void)hipEventDestroy(e);
    e = nullptr;
  }
}

// idempotent: every resource is cleared as it is released (runs from ~Context too)
static void destroy_context(Context *c) {
  if (!c) return;
  bool owns = c->stream || c->stream2 || c->stream3 || c->d_used || c->d_lut || c->d_scan_tmp || c->d_scalars || c->d_code ||
              c->d_symhist || c->h_scalars || c->h_code || c->d_stream;
  for (DeviceBuffer *b : c->buffers()) owns = owns || b->p;
  if (!owns) return;
  DeviceGuard keep;
  (void)hipSetDevice(c->device);
  free_vocab_tables(c);
  // the tables of the context itself: they stay while it is parked
  free_dev(c->d_used, c->d_lut, c->d_scan_tmp, c->d_scalars, c->d_code, c->d_symhist, c->d_norm_index, c->d_norm_pages, c->d_norm_pool, c->d_class_index,
           c->d_class_pages);
  if (c->h_scalars) (void)hipHostFree(c->h_scalars);
  if (c->h_code) (void)hipHostFree(c->h_code);
  c->h_scalars = nullptr;
  c->h_code = nullptr;
  for (DeviceBuffer *b : c->buffers()) b->release();
  destroy_events(c->pipe_ev);
  destroy_events(c->ev);
  destroy_events(c->evs);
  for (hipStream_t *s : {&c->up_stream, &c->down_stream, &c->stream3, &c->stream2, &c->stream}) {
    if (*s) (void)hipStreamDestroy(*s);
    *s = nullptr;
  }
}
Context::~Context() { destroy_context(this); }

template <typename T>
static T *upload(const std::vector<T> &v, hipStream_t st) {
  T *d = nullptr;
  WP_HIP(hipMalloc(&d, std::max<size_t>(v.size(), 1) * sizeof(T)));
  if (!v.empty()) WP_HIP(hipMemcpyAsync(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, st));
  return d;
}

// The reference's API has no handles: every word_piece::linear::encode(text, vocab) parses the vocabulary and
// sets everything up again (linear.cpp:332-341), and its test-suite does that tens of thousands of times.
// Here a context (two streams, events, code point tables, scalars, the arenas) costs ~1.5 ms to make, so
// the contexts of destroyed handles are parked in a small process-wide pool and the next handle on the
// same device takes one over, replacing only the vocabulary tables.  What a parked context keeps is SMALL
// state: arenas of more than kPoolArenaBytes in total go back to the driver when the handle is destroyed (a
// destroyed handle must not sit on the gigabytes its last encode needed — the pool exists for the sub-millisecond
// one-shot calls on tiny inputs); wp_trim() releases the rest.
static constexpr size_t kPoolArenaBytes = size_t(256) << 20;
static constexpr size_t kPoolContexts = 4;
static std::mutex g_pool_mu;
static std::vector<std::unique_ptr<Context>> &context_pool() {
  static auto *pool = new std::vector<std::unique_ptr<Context>>();  // never destroyed: the HIP runtime may be gone by then
  return *pool;
}

static void release_arenas(Context *c) {
  for (DeviceBuffer *b : c->buffers()) b->release();
  c->d_ids = nullptr;
  c->d_offs = nullptr;
  c->dbg = {};
}

static void park_context(std::unique_ptr<Context> c) {
  if (!c) return;
  const bool no_pool = EnvOptions::get().no_pool;
  DeviceGuard keep;
  (void)hipSetDevice(c->device);
  if (!no_pool && hipStreamSynchronize(c->stream) == hipSuccess && hipStreamSynchronize(c->stream2) == hipSuccess &&
      hipStreamSynchronize(c->stream3) == hipSuccess) {
    free_vocab_tables(c.get());
    size_t held = 0;
    for (DeviceBuffer *b : c->buffers()) held += b->cap;
    if (held > kPoolArenaBytes) release_arenas(c.get());
    c->d_ids = nullptr;
    c->d_offs = nullptr;
    c->dbg = {};
    std::lock_guard<std::mutex> g(g_pool_mu);
    if (context_pool().size() < kPoolContexts) {
      context_pool().push_back(std::move(c));
      return;
    }
  }
  destroy_context(c.get());
}

static void upload_vocab_tables(Context *c, const HostVocab &hv) {
  c->d_stream = upload(hv.stream, c->stream);
  c->d_elig_start = upload(hv.elig_start, c->stream);
  c->d_elig_info = upload(hv.elig_info, c->stream);
  c->d_elig_id = upload(hv.elig_id, c->stream);
  c->d_tok_len = upload(hv.tok_len, c->stream);
  c->d_soft = upload(hv.soft, c->stream);
  c->d_vocab_word_idx = upload(hv.used_word_idx, c->stream);
  c->d_vocab_word_bits = upload(hv.used_word_bits, c->stream);
  c->d_cls_bmp = upload(hv.cls_bmp, c->stream);
  c->d_lt_chain_len = upload(hv.lt_chain_len, c->stream);
  c->d_lt_chain_off = upload(hv.lt_chain_off, c->stream);
  c->d_lt_child_begin = upload(hv.lt_child_begin, c->stream);
  c->d_lt_child_cp = upload(hv.lt_child_cp, c->stream);
  c->d_lt_child_node = upload(hv.lt_child_node, c->stream);
  c->d_elig_node = upload(hv.elig_node, c->stream);
  c->d_elig_subtree = upload(hv.elig_subtree, c->stream);
  {
    std::vector<unsigned long long> tk(hv.trie_key.begin(), hv.trie_key.end());
    c->d_trie_key = upload(tk, c->stream);
    WP_HIP(hipStreamSynchronize(c->stream));  // tk is a local
  }
  c->d_trie_child = upload(hv.trie_child, c->stream);
  c->d_trie_id = upload(hv.trie_id, c->stream);
  WP_HIP(hipStreamSynchronize(c->stream));
}

static int device_count_or_throw() {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count == 0) {
    throw HipError("no HIP device available: the Linear WordPiece path has no CPU fallback");
  }
  return count;
}

// a context (streams, vocab tables, scratch) on `device` (< 0: the calling thread's current device): a parked
// one if there is any, else a fresh one
static std::unique_ptr<Context> make_context(const wp_vocab *v, int device) {
  const int count = device_count_or_throw();
  if (device >= 0) {
    if (device >= count) throw std::invalid_argument("no such HIP device: " + std::to_string(device));
  } else {
    WP_HIP(hipGetDevice(&device));
  }
  WP_HIP(hipSetDevice(device));
  std::unique_ptr<Context> c;
  {
    std::lock_guard<std::mutex> g(g_pool_mu);
    auto &pool = context_pool();
    for (size_t i = 0; i < pool.size(); i++) {
      if (pool[i]->device == device) {
        c = std::move(pool[i]);
        pool.erase(pool.begin() + static_cast<long>(i));
        break;
      }
    }
  }
  if (c) {
    upload_vocab_tables(c.get(), v->hv);  // (a throw destroys the context: ~Context)
    return c;
  }
  c.reset(new Context());  // (a throwing WP_HIP below releases what was built so far: ~Context)
  c->device = device;
  WP_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  WP_HIP(hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking));
  WP_HIP(hipStreamCreateWithFlags(&c->stream3, hipStreamNonBlocking));
  for (auto &e : c->evs) WP_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  WP_HIP(hipMalloc(&c->d_used, sizeof(uint32_t) * kCpWords));
  WP_HIP(hipMalloc(&c->d_lut, sizeof(uint32_t) * kCpTableSize));
  WP_HIP(hipMalloc(&c->d_scan_tmp, sizeof(uint32_t) * kCpWords));
  WP_HIP(hipMalloc(&c->d_scalars, sizeof(uint32_t) * kScalars));
  WP_HIP(hipMalloc(&c->d_code, 512 + 256 + kDecodeTableBytes));
  WP_HIP(hipHostMalloc(&c->h_code, 512 + 256 + kDecodeTableBytes));
  WP_HIP(hipMalloc(&c->d_symhist, sizeof(uint32_t) * 256));
  WP_HIP(hipHostMalloc(&c->h_scalars, sizeof(uint32_t) * kScalars));
  for (auto &e : c->ev) WP_HIP(hipEventCreate(&e));
  upload_vocab_tables(c.get(), v->hv);
  return c;
}

static Context *get_context(wp_vocab *v) {
  if (!v->ctx) v->ctx = make_context(v, v->device);
  WP_HIP(hipSetDevice(v->ctx->device));
  return v->ctx.get();
}

// `bytes` zero bytes for the caller to wp_free(): the arrays of a result that no device call made
static void *zeroed(size_t bytes) {
  void *p = std::calloc(std::max<size_t>(bytes, 1), 1);
  if (!p) throw std::bad_alloc();
  return p;
}

// uploads [utf8, utf8 + nbytes) into a text buffer (grown and padded as the decoder expects: text_room) on stream st
static void upload_text(DeviceBuffer &buf, hipStream_t st, const char *utf8, size_t nbytes) {
  buf.ensure(text_room(nbytes));
  zero_text_tail(buf.p, nbytes, st);
  WP_HIP(hipMemcpyAsync(buf.p, utf8, nbytes, hipMemcpyHostToDevice, st));
}
static void upload_text(Context *c, const char *utf8, size_t nbytes) { upload_text(c->text_buf, c->stream, utf8, nbytes); }

// The ids and the rows of a host call (detokenize, pack) in `buf`, ids | rows: n_ids int32 go up on st, and row_bytes of
// `rows` (nullptr: none) into room for the n_rows + 1 entries of row_splits.
struct StagedRows {
  int32_t *d_ids = nullptr;
  long long *d_rows = nullptr;
};
static StagedRows stage_ids_and_rows(DeviceBuffer &buf, hipStream_t st, const int32_t *ids, size_t n_ids, const void *rows, size_t row_bytes,
                                     size_t n_rows) {
  Arena in(&buf);
  StagedRows s;
  for (int pass = 0; pass < 2; pass++) {
    s.d_ids = in.take<int32_t>(n_ids);
    s.d_rows = in.take<long long>(n_rows + 1);
    if (pass == 0) in.commit();
  }
  if (n_ids) WP_HIP(hipMemcpyAsync(s.d_ids, ids, n_ids * sizeof(int32_t), hipMemcpyHostToDevice, st));
  if (rows) WP_HIP(hipMemcpyAsync(s.d_rows, rows, row_bytes, hipMemcpyHostToDevice, st));
  return s;
}

// queues the copy of the device scalars from word 0 through slot `last` to the pinned mirror
static void queue_scalars(Context *c, int last, hipStream_t st) {
  WP_HIP(hipMemcpyAsync(c->h_scalars, c->d_scalars, sizeof(uint32_t) * scalar_end(last), hipMemcpyDeviceToHost, st));
}
// the same on the context's stream, and waits
static void fetch_scalars(Context *c, int last) {
  queue_scalars(c, last, c->stream);
  WP_HIP(hipStreamSynchronize(c->stream));
}
// queues the copy of the slots `first` through `last` alone (other streams may be copying the words around them)
static void queue_scalar_slots(Context *c, int first, int last, hipStream_t st) {
  WP_HIP(hipMemcpyAsync(c->h_scalars + first, c->d_scalars + first, sizeof(uint32_t) * (scalar_end(last) - first), hipMemcpyDeviceToHost, st));
}
// queues the clearing of the device scalars from slot `first` through slot `last`
static void clear_scalars(Context *c, int first, int last, hipStream_t st) {
  WP_HIP(hipMemsetAsync(c->d_scalars + first, 0, sizeof(uint32_t) * (scalar_end(last) - first), st));
}

}  // namespace wp
