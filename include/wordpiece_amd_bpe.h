/* wordpiece_amd_bpe.h — byte-level BPE on the device: the GPT-2 pre-tokenizer pattern, a vocabulary of byte ids and a ranked
 * merge list, ids in the shape wp_linear_encode_rows gives (ids int32, row_splits int64), so that the pack calls behind the
 * encoder take them unchanged.  An addition beside wordpiece_amd_classify.h; the entry points live in the same library.
 * This section is the contract; tests/bpe_model.py is its executable form.
 * Out of scope: other patterns (cl100k / Llama-3), ignore_merges, special tokens inside text (<|endoftext|>; the pack calls
 * add eos_id), dropout, add_prefix_space, decoding ids back to bytes, learning merges.
 *
 * The model.  wp_bpe_load(v, slot, m) copies a model into slot 0..WP_BPE_SLOTS-1 of the handle, on the handle's device, and
 * builds the pair table; a model already in the slot is replaced.  m holds host pointers and sizes: byte_id int32 [256], the
 * id of each single byte; merges int32 [n_merges][3], (left id, right id, result id), the row index being the rank; n_ids,
 * the size of the vocabulary, every id in [0, n_ids); pattern = WP_BPE_PATTERN_GPT2 (the only value today: a later pattern
 * is a new value, not a new name); reserved = 0.  The model stays across every other call on the handle (encodes and
 * wp_trim included) until wp_bpe_clear(v, slot) or the end of the handle.  wp_bpe_load keeps the slot's earlier model where
 * it fails.  Load rules: the 256 byte ids are distinct; a pair (left, right) occurs once; each operand of merge k is a byte
 * id or the result of a merge j < k (a "proper" list: every trained merges file is one).
 *
 * Characters and classes.  A well-formed UTF-8 sequence (Unicode Table 3-7) that lies inside one document is one character;
 * any other byte is one character of class O.  S: the 25 White_Space code points U+0009..000D, 0020, 0085, 00A0, 1680,
 * 2000..200A, 2028, 2029, 202F, 205F, 3000 (U+001C..001F are not among them).  L: general category L*.  N: Nd, Nl, No.
 * O: everything else.  L and N come from a table generated with the Unicode version WP_BPE_UNICODE_VERSION names.
 *
 * Pieces.  The GPT-2 pattern  's|'t|'re|'ve|'m|'ll|'d| ?\p{L}+| ?\p{N}+| ?[^\s\p{L}\p{N}]+|\s+(?!\S)|\s+  applied to each
 * document alone, stated as a local rule.  Character i starts a piece iff
 *   1. it is S and its predecessor is not S (or there is none), or its predecessor is S and its successor exists and is not S;
 *   2. it is not S and there is no predecessor, or the predecessor is S and is not U+0020, or the predecessor is not S and
 *      has another class;
 *   3. contractions: where an apostrophe is a start by rule 2 and is followed by one of s t m d, the next character is not a
 *      start and the one behind it is; where it is followed by re, ve or ll, the next two are not starts and the one behind
 *      them is.  Lower case only.  A contraction ends in a letter, so an apostrophe behind it is a start by rule 2 already.
 * A piece runs from its start to the next start or to the end of the document.
 *
 * Merge.  A piece starts as the ids of its bytes.  While any adjacent pair is in the merge list: take the lowest rank
 * present, replace its occurrences left to right, without overlap, by the result, repeat.  A merger that applies one pair
 * at a time, lowest rank first and leftmost first (the `tokenizers` package), gives the same ids whenever no merge creates
 * a pair of a lower rank than its own; with a proper list that can only fail where two merges share a result and a merge
 * ranked between them reads it.  This loop is the contract there too.
 *
 * wp_bpe_encode_rows[_device](v, data, row_off, n_rows, spec, out): the batch as wp_scrub_rows takes it (text bytes, row_off
 * int64 [n_rows + 1] ascending from 0, at most UINT32_MAX bytes, fewer than 2^31 rows).  spec: slot; want; pad, pad2 and
 * reserved 0.  out: ids int32 [n_ids], the ids of every document back to back; row_splits int64 [n_rows + 1], document r
 * owning ids [row_splits[r], row_splits[r + 1]); n_rows, n_ids, n_pieces.  WP_BPE_WANT_OFFSETS: begin and end int32 [n_ids],
 * the bytes of every id as offsets into its document.  WP_BPE_WANT_PIECES: piece_splits int64 [n_pieces + 1], the index of
 * every piece's first id and n_ids behind the last.  The same batch gives the same bits in every run.
 * WP_ERR_ARG, before a device is touched, with the prefix "bpe: " and the field named: m, spec or out NULL; slot outside
 * 0..3, or (rows, behind the rules of the batch) a slot without a model; pattern not 0; reserved, pad or pad2 not 0; n_ids
 * outside [256, 2^31); n_merges negative; byte_id NULL, merges NULL with n_merges > 0; a byte id or an id of a merge
 * outside [0, n_ids) (the byte or the merge named); two bytes with one id; a pair that occurs twice; an operand that is
 * neither a byte id nor an earlier result; want with a bit outside 3; row_off NULL with rows, data NULL with bytes, bad
 * offsets with the first bad row.  WP_ERR_TOO_LARGE: n_merges >= 2^30, n_rows >= 2^31, more than UINT32_MAX bytes.
 * Host form: the blocks of *out are malloc'd, each freed with wp_free; n_rows == 0 needs no device and returns all NULL.
 * Device form: data 4-byte aligned and readable in whole words, row_off 8-byte aligned; the arrays of *d_out are device
 * memory owned by the handle until its next call.
 * With WP_OPT_STAGE_TIMING a call leaves its device times in wp_stats: ms_decode (intake, class and start pass, piece
 * list), ms_sa (merge pass), ms_scan (compaction, row_splits, offsets), ms_walk (the end of the call), ms_total (their sum).
 * A call leaves the statistics of every other layer as they were. */
#ifndef WORDPIECE_AMD_BPE_H
#define WORDPIECE_AMD_BPE_H
#include "wordpiece_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WP_BPE_SLOTS 4
#define WP_BPE_PATTERN_GPT2 0
#define WP_BPE_WANT_OFFSETS 1
#define WP_BPE_WANT_PIECES  2
typedef struct {
  const int32_t *byte_id, *merges;
  int64_t n_merges, n_ids;
  int32_t pattern, reserved;
} wp_bpe_model;
typedef struct {
  int32_t slot, want, pad, pad2;
  int64_t reserved;
} wp_bpe_spec;
typedef struct {
  int32_t *ids;
  int64_t *row_splits;
  int32_t *begin, *end;
  int64_t *piece_splits;
  int64_t n_rows, n_ids, n_pieces;
} wp_bpe_result;
int wp_bpe_load(wp_vocab *v, int slot, const wp_bpe_model *m);
int wp_bpe_clear(wp_vocab *v, int slot);
int wp_bpe_encode_rows(wp_vocab *v, const void *data, const int64_t *row_off, size_t n_rows, const wp_bpe_spec *spec, wp_bpe_result *out);
int wp_bpe_encode_rows_device(wp_vocab *v, const void *d_data, const int64_t *d_row_off, size_t n_rows, const wp_bpe_spec *spec, wp_bpe_result *d_out);
/* Of the last wp_bpe_encode_rows call on the slot: its rows, pieces and ids, the bytes of the longest piece, and the pieces
 * that went one lane each (n_short), one wave each (n_medium) and one workgroup each (n_long).  Of the model: its merges,
 * its ids and the slots of its pair table. */
typedef struct { int64_t n_rows, n_pieces, n_ids, max_piece, n_short, n_medium, n_long, n_merges, model_ids, table_slots; } wp_bpe_stats;
int wp_get_bpe_stats(const wp_vocab *v, int slot, wp_bpe_stats *out);   /* n_rows == -1: no such call yet */

#ifdef __cplusplus
}
#endif
#endif
