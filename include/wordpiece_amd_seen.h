/* wordpiece_amd_seen.h — rows seen in earlier batches: a set of 64-bit row keys that lives on the handle, in device
 * memory, across calls (the exact dedup of a corpus that comes in shards: what CCNet's paragraph hashes and DataTrove's
 * exact dedup do between the filters and the tokeniser).  An addition beside wordpiece_amd_scrub.h; the entry points live
 * in the same library.  This section is the contract; tests/seen_model.py is its executable form.
 *
 * The key.  K(row) is a 64-bit function of the row's bytes alone: the round-0 key of wp_dedup_rows at hash_bits 64.  All
 * arithmetic is mod 2^64.  mix64(h): h ^= h >> 33; h *= 0xff51afd7ed558ccd; h ^= h >> 33; h *= 0xc4ceb9fe1a85ec53;
 * h ^= h >> 33.  G = 0x9e3779b97f4a7c15; s0 = mix64(G).  The length term is mix64(s0 ^ (len_bytes | 1 << 40)).  The row is
 * cut into chunks of 256 bytes (the last one shorter); chunk k (from 0) of b bytes is read as ceil(b / 4) little-endian
 * 32-bit words, the last one zero-padded:  h = mix64((s0 ^ (k + 1)) + 0x632be59bd9b4e019); for every full pair of words
 * (w0, w1) in order h = mix64(h ^ (w0 | w1 << 32)) + G; x = (the odd last word, or 0) | b << 32; v = mix64(h ^ x).
 * K = the length term + the sum of v over the chunks.  The value 0 marks an empty slot of the set: a key that comes out 0
 * is stored, compared and returned as 1.  Membership is by key: two rows with one key are one row (2^-64 per pair of
 * different rows; no byte is compared, as wp_neardup_rows states of its hashes).
 *
 * The set holds keys only.  The handle owns it, on the handle's device; it is empty until first used, survives every
 * other call on the handle (encodes and wp_trim included) and ends with wp_seen_clear or with the handle.  One set belongs
 * to one handle on one device: sets of other handles, ranks or processes meet through wp_seen_export and wp_seen_keys.
 *
 * wp_seen_rows[_device](v, data, row_off, n_rows, spec, out).  The batch as wp_dedup_rows takes it: elem_bytes 1 or 4,
 * row_off int64 [n_rows + 1] ascending from 0 (the first bad row is named), at most UINT32_MAX bytes, fewer than 2^31 rows.
 * Per row: state int32 — 0 new (the key is not in the set and this is the key's smallest row of the batch), 1 (the key is
 * not in the set, but a smaller row of this batch has it), 2 (the key was in the set before the call) — and first int32,
 * the smallest row of the batch with the same key (the row itself where there is none smaller, whatever its state).
 * WP_SEEN_WANT_KEYS: keys uint64 [n_rows].  WP_SEEN_WANT_COMPACT: kept int32 [n_kept] (the rows of state 0, ascending),
 * data (n_elems elements) and row_off int64 [n_kept + 1]: those rows back to back, what wp_dedup_rows_device and the
 * encode of rows take.  Unless flags has WP_SEEN_QUERY_ONLY the keys of the state-0 rows are in the set when the call
 * returns; with the bit the set is unchanged (block lists, decontamination by exact row).
 * wp_seen_keys[_device](v, keys, n, spec, out): the same call over n given uint64 keys in place of rows (0 is taken as 1),
 * with the same state, first and flags; elem_bytes is not read and want must be 0.  It loads a saved set and merges sets.
 * wp_seen_export[_device](v, keys_out, room, n): *n = the keys of the set; where room >= *n they are written to keys_out
 * ascending, otherwise nothing is written.  Ascending order makes the result independent of the slot layout.
 * wp_seen_reserve(v, n_keys): room for n_keys keys in advance (a table not yet made is made at that size).
 * wp_seen_clear(v): empties the set and frees its memory; the statistics of the set start again.
 * The table: uint64 slots, a power of two of them and 1,024 at least, made at 1,024 by the first call that needs it; a key's
 * home is the slot its top log2(capacity) bits name, linear probing forward with wrap.  Before it probes, a call makes
 * capacity >= 2 (n_keys + n): the table is then replaced by one of the power of two that fits and its keys are rehashed
 * (one growth, counted in n_grown whether or not the table held a key yet).  Slot layout can depend on the order of
 * execution; no output does.
 * WP_ERR_ARG, before a device is touched and with the field named: spec or out NULL, elem_bytes not 1 or 4 (rows), want
 * with a bit outside 3 (rows) or not 0 (keys), flags with a bit outside 1, pad or reserved not 0, row_off NULL with rows,
 * keys NULL with n > 0, data NULL with elements, bad offsets with the first bad row (host form; the device form finds
 * them on the device), n or keys_out NULL in an export with room.  WP_ERR_TOO_LARGE: n_rows or n >= 2^31, more than
 * UINT32_MAX bytes, a table of more than 2^31 slots.  A call with no rows or keys needs no device and hands out NULLs.
 * Host form: the blocks of *out are malloc'd, each freed with wp_free.  Device form: data 4-byte aligned, row_off and
 * keys 8-byte aligned; the arrays of *d_out are device memory owned by the handle until its next call.
 * With WP_OPT_STAGE_TIMING a call leaves its device times in wp_stats: ms_decode (intake and keys), ms_sa (sort and runs),
 * ms_walk (growth, lookup, insert, states, compact form), ms_total (their sum). */
#ifndef WORDPIECE_AMD_SEEN_H
#define WORDPIECE_AMD_SEEN_H
#include "wordpiece_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WP_SEEN_WANT_KEYS    1
#define WP_SEEN_WANT_COMPACT 2
#define WP_SEEN_QUERY_ONLY   1
#define WP_SEEN_MIN_SLOTS    1024
enum { WP_SEEN_NEW = 0, WP_SEEN_REPEAT_BATCH = 1, WP_SEEN_BEFORE = 2 };
typedef struct {
  int32_t elem_bytes, want, flags, pad;
  int64_t reserved;
} wp_seen_spec;
typedef struct {
  int32_t *state, *first, *kept;
  uint64_t *keys;
  int64_t *row_off;
  void *data;
  int64_t n_rows, n_kept, n_elems;
} wp_seen_result;
int wp_seen_rows(wp_vocab *v, const void *data, const int64_t *row_off, size_t n_rows, const wp_seen_spec *spec, wp_seen_result *out);
int wp_seen_rows_device(wp_vocab *v, const void *d_data, const int64_t *d_row_off, size_t n_rows, const wp_seen_spec *spec, wp_seen_result *d_out);
int wp_seen_keys(wp_vocab *v, const uint64_t *keys, size_t n, const wp_seen_spec *spec, wp_seen_result *out);
int wp_seen_keys_device(wp_vocab *v, const uint64_t *d_keys, size_t n, const wp_seen_spec *spec, wp_seen_result *d_out);
int wp_seen_export(wp_vocab *v, uint64_t *keys_out, size_t room, size_t *n);
int wp_seen_export_device(wp_vocab *v, uint64_t *d_keys_out, size_t room, size_t *n);
int wp_seen_reserve(wp_vocab *v, size_t n_keys);
int wp_seen_clear(wp_vocab *v);
/* Of the last wp_seen_rows / wp_seen_keys call: its rows (or keys), and those of state 0, 1 and 2.  Of the set: its keys,
 * its slots and the growths so far.  n_probes is NOT part of the contract: the 64-byte lines the lookup of the last call
 * read, for profiles/seen_probe.py. */
typedef struct { int64_t n_rows, n_new, n_repeat_batch, n_seen_before, n_keys, capacity, n_grown, n_probes; } wp_seen_stats;
int wp_get_seen_stats(const wp_vocab *v, wp_seen_stats *out);   /* n_rows == -1: no such call yet */

#ifdef __cplusplus
}
#endif
#endif
