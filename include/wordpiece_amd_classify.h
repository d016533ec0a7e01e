/* wordpiece_amd_classify.h — documents scored by a fastText-style linear classifier on the device: hashed word,
 * character-n-gram and word-n-gram features, one embedding row per feature, their average, one small matrix product and a
 * softmax (language identification, a learned quality filter).  An addition beside wordpiece_amd_seen.h; the entry points
 * live in the same library.  This section is the contract; tests/classify_model.py is its executable form.  It is
 * fastText's supervised inference with a softmax loss on an unpruned, unquantised model as dictionary.cc / fasttext.cc of
 * 0.9.2 read; parity with the fasttext package is NOT claimed (it could not be checked where this was written).
 * Out of scope: hierarchical softmax and one-vs-all losses, pruned or quantised (.ftz) models, parsing a .bin file,
 * half-precision matrices, top-k beyond the argmax, and fastText's special case for tokens that begin with __label__ (here
 * they are ordinary tokens).
 *
 * The model.  wp_classify_load(v, slot, m) copies a model into slot 0..WP_CLASSIFY_SLOTS-1 of the handle, on the handle's
 * device, and builds the dictionary table; a model already in the slot is replaced.  m holds host pointers: words (a byte
 * pool) with word_off int64 [n_words + 1] ascending from 0, input float32 [n_words + bucket][dim] row-major, output
 * float32 [n_labels][dim]; n_words, bucket, dim, n_labels, minn, maxn, word_ngrams; reserved = 0.  The model stays across
 * every other call on the handle (encodes and wp_trim included) until wp_classify_clear(v, slot) or the end of the handle.
 *
 * Tokens.  A token is a maximal run of bytes other than 0x20 0x0A 0x0D 0x09 0x0B 0x0C 0x00 inside one document.  One
 * extra token "</s>" is appended to every document (an empty one too).
 * Hash.  H(bytes): h = 2166136261; per byte h ^= (uint32)(int8)byte (the byte sign-extended), h *= 16777619, mod 2^32.
 * H("a") = 3826002220, H("</s>") = 3617362777, H(C3 A9) = 1023043777.
 * Dictionary.  wid(token): the index of the first model word whose bytes equal the token's, or none.  The device table is
 * keyed by H, and every hit is confirmed by comparing the bytes: no result depends on a hash collision.
 * Features of a token.  wid, if it has one.  If maxn > 0 and the token's bytes are not "</s>" (the appended token and a
 * literal one alike): its character n-grams over w = "<" + token + ">".  For every byte index i of w whose byte is not a
 * continuation byte ((b & 0xC0) != 0x80), a gram grows from i one character at a time, a character being one byte plus the
 * continuation bytes that follow it, for n = 1..maxn while w lasts; gram n is kept iff n >= minn and not (n == 1 and
 * (i == 0 or the gram ends at the end of w)), and gives feature n_words + H(gram) % bucket.  The rule is per byte:
 * invalid UTF-8 needs none of its own.
 * Word n-grams (word_ngrams = N > 1).  s_t: H(token t) read as int32 and sign-extended to 64 bits, over all tokens of the
 * document, "</s>" and those without a wid included.  For every t: h = s_t in uint64 arithmetic; for j = t + 1 ..
 * min(t + N - 1, last): h = h * 116049371 + s_j, and feature n_words + h % bucket after each step.
 * Score.  F: the features of the document, repeats counted.  S[k]: the sum of input[f][k] over them.  logits[j] =
 * (sum over k of output[j][k] * S[k]) / (float)F; prob: the softmax of the logits; label: the argmax, the smallest index
 * on ties.  All in float32.  The order of the sums is the implementation's, but fixed: the same batch gives the same bits
 * in every run (no floating-point atomic anywhere).  The division comes last on purpose: with exactly representable
 * weights the sums are exact.  F = 0: label -1, prob 0, logits 0.
 *
 * wp_classify_rows[_device](v, data, row_off, n_rows, spec, out): the batch as wp_scrub_rows takes it (text bytes, row_off
 * int64 [n_rows + 1] ascending from 0, at most UINT32_MAX bytes, fewer than 2^31 rows).  spec: slot; want; keep_labels, an
 * int32 array of n_keep labels in host memory (both forms; NULL with n_keep 0: every label); min_prob in [0, 1]; pad, pad2
 * and reserved 0.  Per document: label int32, prob float32, n_features int64 (F) and reasons uint32: bit 0 no feature; and
 * only where bit 0 is clear: bit 1 label not in keep_labels, bit 2 prob < min_prob.  WP_CLASSIFY_WANT_LOGITS: logits float32
 * [n_rows][n_labels].  WP_CLASSIFY_WANT_COMPACT: kept int32 [n_kept] ascending, data (n_elems bytes) and row_off int64
 * [n_kept + 1]: the documents with reasons == 0 back to back, what wp_dedup_rows_device and the encode of rows take.
 * Two walks are sequential.  A lane hashes one token alone, which FNV demands; the walk ends one byte past the longest
 * model word (such a token has no wid) unless word_ngrams > 1 needs the whole hash.  And one wave adds the partial sums of
 * one document, one per 4 * min(64, 2^ceil(log2 dim)) of its features.  Everything else is flat over bytes, tokens or
 * features.  A call must not list more than UINT32_MAX features.  wp_classify_load keeps the slot's earlier model where it
 * fails.
 * WP_ERR_ARG, before a device is touched, with the prefix "classify: " and the field named: m, spec or out NULL; slot
 * outside 0..3, or (rows, behind the rules of the batch) a slot without a model; dim outside 1..512; n_labels outside 1..65535; maxn > 6 or
 * negative, minn > maxn or negative, minn == 0 with maxn > 0; word_ngrams outside 1..5; bucket negative, or 0 while
 * maxn > 0 or word_ngrams > 1; n_words negative; words, word_off, input or output NULL where they have entries; word_off
 * not ascending from 0 (the first bad word named); reserved, pad or pad2 not 0; want with a bit outside 3; n_keep negative,
 * keep_labels NULL with n_keep > 0, a keep label outside the model (its index named); min_prob outside [0, 1]; row_off
 * NULL with rows, data NULL with bytes, bad offsets with the first bad row.  WP_ERR_TOO_LARGE: n_words + bucket >= 2^31,
 * a word pool of 2^32 bytes or more, n_rows >= 2^31, more than UINT32_MAX bytes or features.
 * Host form: the blocks of *out are malloc'd, each freed with wp_free; n_rows == 0 needs no device and returns all NULL.
 * Device form: data 4-byte aligned and readable in whole words, row_off 8-byte aligned; the arrays of *d_out are device
 * memory owned by the handle until its next call.
 * With WP_OPT_STAGE_TIMING a call leaves its device times in wp_stats: ms_decode (intake and token list), ms_sa (feature
 * list), ms_scan (row gathers and partial sums), ms_walk (output stage and compact form), ms_total (their sum).
 * A call leaves the statistics of every other layer as they were. */
#ifndef WORDPIECE_AMD_CLASSIFY_H
#define WORDPIECE_AMD_CLASSIFY_H
#include "wordpiece_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WP_CLASSIFY_SLOTS 4
#define WP_CLASSIFY_MAX_DIM 512
#define WP_CLASSIFY_MAX_LABELS 65535
#define WP_CLASSIFY_MAX_MAXN 6
#define WP_CLASSIFY_MAX_WORD_NGRAMS 5
#define WP_CLASSIFY_WANT_LOGITS  1
#define WP_CLASSIFY_WANT_COMPACT 2
enum { WP_CR_NO_FEATURE = 0, WP_CR_LABEL, WP_CR_MIN_PROB };
typedef struct {
  const void *words;
  const int64_t *word_off;
  const float *input, *output;
  int64_t n_words, bucket;
  int32_t dim, n_labels, minn, maxn, word_ngrams, reserved;
} wp_classify_model;
typedef struct {
  int32_t slot, want, n_keep, pad;
  const int32_t *keep_labels;
  float min_prob;
  int32_t pad2;
  int64_t reserved;
} wp_classify_spec;
typedef struct {
  int32_t *label;
  float *prob, *logits;
  int64_t *n_features, *row_off;
  uint32_t *reasons;
  int32_t *kept;
  void *data;
  int64_t n_rows, n_labels, n_kept, n_elems;
} wp_classify_result;
int wp_classify_load(wp_vocab *v, int slot, const wp_classify_model *m);
int wp_classify_clear(wp_vocab *v, int slot);
int wp_classify_rows(wp_vocab *v, const void *data, const int64_t *row_off, size_t n_rows, const wp_classify_spec *spec, wp_classify_result *out);
int wp_classify_rows_device(wp_vocab *v, const void *d_data, const int64_t *d_row_off, size_t n_rows, const wp_classify_spec *spec, wp_classify_result *d_out);
/* Of the last wp_classify_rows call on the slot: its rows, those with reasons 0, the features (the sum of F), the tokens
 * ("</s>" included) and those with a wid.  Of the model: its sizes. */
typedef struct { int64_t n_rows, n_kept, n_features, n_tokens, n_found, n_words, bucket, dim, n_labels, minn, maxn, word_ngrams; } wp_classify_stats;
int wp_get_classify_stats(const wp_vocab *v, int slot, wp_classify_stats *out);   /* n_rows == -1: no such call yet */

#ifdef __cplusplus
}
#endif
#endif
