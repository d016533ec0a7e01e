/*
 * wordpiece_amd.h — C ABI of the MI355X-native Linear WordPiece encoder.
 *
 * This is the drop-in boundary for the reference's Linear path
 * (gleb-kov/wordpiece, src/word_piece.hpp:12-19 → src/linear.cpp:321-374).  The
 * reference has no FFI of its own: its boundary is the C++ header
 * word_piece.hpp, re-implemented on top of this ABI in include/word_piece.hpp.
 * Every entry point below cites the reference interface it replaces.
 *
 * Conventions: plain pointers and sizes, no C++/torch types; every function
 * returns WP_OK (0) or a WP_ERR_* code and wp_last_error() then holds the
 * message for the calling thread.  A vocab handle is single-caller (the
 * reference is effectively single-caller too: its global thread pool barrier
 * waits on all tasks, utils.cpp:25-28).  The library needs a HIP device: there
 * is NO CPU fallback — without a GPU every compute entry point fails loudly
 * with WP_ERR_NO_DEVICE.  No exception crosses the ABI, and every entry point leaves
 * the calling thread's current HIP device as it found it (hipGetDevice on entry,
 * hipSetDevice back on exit), whatever device the handle or its shards live on.
 */
#ifndef WORDPIECE_AMD_H
#define WORDPIECE_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WP_OK 0
#define WP_ERR_EMPTY_WORD 1 /* "Vocab word is empty"   utils.cpp:99-101  */
#define WP_ERR_TOO_LARGE 2  /* "64bit not implemented" linear.cpp:104-106 */
#define WP_ERR_HIP 3        /* HIP runtime error (replaces "SACA return code: N", linear.cpp:139-141) */
#define WP_ERR_NO_DEVICE 4
#define WP_ERR_IO 5  /* file could not be opened / mapped (Boost throws there) */
#define WP_ERR_ARG 6

typedef struct wp_vocab wp_vocab;

/* ---- vocabulary: utils.cpp:81-137 (WordPieceToken, parseVocab, readVocabFromFile) ----
 * Lines are raw UTF-8 without terminators; `##` prefix, [special] and malformed
 * classification exactly as the reference.  The handle also caches the device
 * copy of the vocab symbol stream (a pure function of the vocab). */
int wp_vocab_create(const char *const *lines, const size_t *line_bytes, size_t n_lines,
                    wp_vocab **out);
/* same, lines given as one buffer + n_lines+1 offsets (ctypes/JNI friendly) */
int wp_vocab_create_packed(const char *buf, const int64_t *offsets, int64_t n_lines,
                           wp_vocab **out);
/* utils.cpp:123-137: std::getline semantics (LF only; a CR stays in the token) */
int wp_vocab_from_file(const char *vocab_file, wp_vocab **out);
void wp_vocab_destroy(wp_vocab *v);
int64_t wp_vocab_size(const wp_vocab *v);
int32_t wp_vocab_unk_id(const wp_vocab *v);              /* utils.hpp:30-33, -1 if absent */
int32_t wp_vocab_token_flags(const wp_vocab *v, int64_t i); /* bit0 prefix, bit1 special, bit2 malformed */
int64_t wp_vocab_token_len(const wp_vocab *v, int64_t i);

/* ---- the hot path: linear.cpp:321-328 encodeLinearWordPiece ----
 * replaces word_piece::linear::encode(text, vocab)        word_piece.hpp:12, linear.cpp:332-335
 * host UTF-8 in, malloc'd int32 ids out (free with wp_free). */
int wp_linear_encode(wp_vocab *v, const char *utf8, size_t nbytes, int32_t **ids, size_t *n_ids);

/* Same path with the text already resident in device memory and the ids left
 * there (what bench.py times; what a training input pipeline would consume).
 * `d_ids` is owned by the handle and valid until the next call on it.
 * `d_utf8` must be 4-byte aligned and readable up to the next multiple of 16 bytes behind
 * `nbytes` (the decoder loads whole words; the padding bytes are ignored). */
int wp_linear_encode_device(wp_vocab *v, const void *d_utf8, size_t nbytes,
                            const int32_t **d_ids, size_t *n_ids);

/* ---- token offsets (an addition: TF Text tokenize_with_offsets, HF Encoding.offsets) ----
 * The ids of wp_linear_encode plus the span of the input each id came from: offsets[2k], offsets[2k + 1] =
 * [begin, end) of id k, in `unit`.  A token matched at code point p spans [p, p + its length in code points,
 * without "##"); an [UNK] (or id -1 when the vocab has none) spans the word it replaces: from the first token its
 * rollback drops (or the failing position) to where the walk resumes (the next word-prefix position, or the end
 * of the text; the blanks behind it excluded).  Spans are increasing and disjoint; every non-blank code point lies
 * in exactly one.
 *   WP_OFFSETS_BYTES: byte offsets into `utf8` — a span runs from the first byte of its first code point to one past
 *     the last byte of its last one; a dropped invalid byte inside a span belongs to it, one between spans to none.
 *     nbytes > UINT32_MAX fails with WP_ERR_TOO_LARGE.
 *   WP_OFFSETS_CODE_POINTS: positions in the decoded text (for valid UTF-8: Python str indices).
 *   With WP_OPT_NORMALIZE the meaning is unchanged: offsets refer to the text the caller passed, not to the normalised
 *     copy.  A span the walk reports as normalised code points [b, e) runs from the start of the source code point of b
 *     to the end of the source code point of e - 1; all code points one source code point expands into share its span.
 *     A source code point the rule drops (a combining mark, a cleaned control) inside a span belongs to it, one behind
 *     the last kept code point of a span or between spans to none — the rule for dropped invalid bytes.
 * Any other unit fails with WP_ERR_ARG.  Empty text gives 0 ids without a device.  Both entry points encode on the
 * handle's own device: WP_OPT_DEVICES does not shard them. */
#define WP_OFFSETS_BYTES 0
#define WP_OFFSETS_CODE_POINTS 1
/* host text in; ids and offsets out as two blocks (free each with wp_free) */
int wp_linear_encode_offsets(wp_vocab *v, const char *utf8, size_t nbytes, int unit, int32_t **ids,
                             uint32_t **offsets, size_t *n_ids);
/* device text (same buffer contract as wp_linear_encode_device); `d_ids` and `d_offsets` (2 * n_ids uint32) are
 * owned by the handle and valid until its next call */
int wp_linear_encode_offsets_device(wp_vocab *v, const void *d_utf8, size_t nbytes, int unit,
                                    const int32_t **d_ids, const uint32_t **d_offsets, size_t *n_ids);

/* ---- documents (an addition: TF Text RaggedTensor.row_splits, HF BatchEncoding / tokenizer(padding=, truncation=)) ----
 * Many documents in one call.  Input is the joined form: the documents back to back, each followed by one '\n' (a
 * corpus file with one document per line).  The rows are given
 *   explicitly: doc_off[0..n_docs] (increasing, doc_off[0] == 0, doc_off[n_docs] == nbytes); document i is bytes
 *     [doc_off[i], doc_off[i + 1] - 1) and byte doc_off[i + 1] - 1 must be '\n' (a document may itself hold '\n': a blank
 *     like any other).  Anything else fails with WP_ERR_ARG before ids are produced (host entry points check on the
 *     host, device entry points by a kernel);
 *   or as the lines of the text (doc_off == NULL; n_docs is ignored): a text that does not end in '\n' has a last
 *     line that runs to the end, one that does has no extra empty row.
 * Result for n_rows documents: ids (n_ids) and row_splits (n_rows + 1, row_splits[0] == 0, row_splits[n_rows] == n_ids)
 * — row i is ids[row_splits[i] .. row_splits[i + 1]) — and, with unit WP_OFFSETS_* (-1: none, offsets NULL), offsets
 * as wp_linear_encode_offsets gives them but relative to the start of the id's own document.  Row i and its offsets
 * are exactly what wp_linear_encode_offsets(document i) returns (an empty document, or one of blanks or invalid bytes
 * only, is an empty row); the rows concatenated are wp_linear_encode of the joined text.  The span of a word that
 * fails ([UNK]) begins at the word's first code point, so a failing first word belongs to its own document, with
 * offset 0 or the number of blanks in front of it.  With WP_OPT_NORMALIZE the rows are those of the text the caller
 * passed: a line of code points that the rule drops is still a row, an empty one — also the last line of a text that
 * does not end in '\n', and the only line of a text that normalises to nothing.
 * Normally that is one encode of the joined text plus a few kernels over the spans (wp_stats.rows_route == 1).  Three
 * kinds of vocabulary could match differently in the joined text than in a document of its own and are encoded
 * document by document instead (rows_route == 0, same results, one encode per document): an eligible token that holds
 * U+000A, a token that holds U+0000 / U+0001, duplicate eligible lines.
 * Limits: those of the joined text as one encode, and nbytes <= UINT32_MAX in every unit (WP_ERR_TOO_LARGE).  Like the
 * offsets calls these run on the handle's own device (WP_OPT_DEVICES does not shard them).  Empty input (nbytes == 0,
 * or explicit rows that are all empty) needs no device in the host entry points. */
/* tf_text tokenize_with_offsets on a batch -> RaggedTensor (values, row_splits); HF BatchEncoding.input_ids /
 * .offset_mapping.  Host text in; ids, row_splits and offsets out as blocks of their own (free each with wp_free; ids
 * and offsets NULL when n_ids == 0, offsets NULL when unit == -1). */
int wp_linear_encode_rows(wp_vocab *v, const char *utf8, size_t nbytes, const int64_t *doc_off, size_t n_docs, int unit,
                          int32_t **ids, int64_t **row_splits, uint32_t **offsets, size_t *n_ids, size_t *n_rows);
/* the same with the text (buffer contract of wp_linear_encode_device) and doc_off (8-byte aligned, or NULL) in device
 * memory; the results stay there, owned by the handle and valid until its next call */
int wp_linear_encode_rows_device(wp_vocab *v, const void *d_utf8, size_t nbytes, const int64_t *d_doc_off, size_t n_docs,
                                 int unit, const int32_t **d_ids, const int64_t **d_row_splits, const uint32_t **d_offsets,
                                 size_t *n_ids, size_t *n_rows);
/* HF tokenizer(batch, padding="max_length", truncation=True, max_length=) / tf_text pad_model_inputs: row r of
 * input_ids[n_rows, max_len] is [cls] + T[:keep] + [sep] + pad..., T the ids of document r, keep = min(len(T),
 * max_len - number of specials); lengths[r] = keep + number of specials (the attention mask is arange(max_len) <
 * lengths[:, None]).  cls_id / sep_id -1: none; the ids are not range-checked against the vocabulary.  max_len < 1 or
 * smaller than the number of specials fails with WP_ERR_ARG.  wp_stats.rows_truncated counts the rows that lost ids.
 * Host text in, two blocks out (free each with wp_free). */
int wp_linear_encode_padded(wp_vocab *v, const char *utf8, size_t nbytes, const int64_t *doc_off, size_t n_docs,
                            int max_len, int32_t cls_id, int32_t sep_id, int32_t pad_id, int32_t **input_ids,
                            int32_t **lengths, size_t *n_rows);
/* the same from device memory into caller-owned device buffers (a training loop's batch tensor: no copy): d_input_ids
 * holds capacity_rows * max_len int32, d_lengths capacity_rows; nothing beyond n_rows rows is touched.  More rows than
 * capacity_rows fails with WP_ERR_ARG, the needed count in *n_rows and nothing written.  The call returns when the
 * batch is complete. */
int wp_linear_encode_padded_device(wp_vocab *v, const void *d_utf8, size_t nbytes, const int64_t *d_doc_off, size_t n_docs,
                                   int max_len, int32_t cls_id, int32_t sep_id, int32_t pad_id, int32_t *d_input_ids,
                                   int32_t *d_lengths, size_t capacity_rows, size_t *n_rows);

/* ---- model inputs (an addition: HF tokenizer(a, b, truncation=, stride=, return_overflowing_tokens=, padding="max_length")) ----
 * The rows of a documents call (same joined input, explicit rows or lines, both routes, WP_OPT_NORMALIZE as there) become
 * SAMPLES: with pairs == 0 row s is sample s (sequence A only); with pairs == 1 rows 2s, 2s + 1 are A and B of sample s
 * (an odd number of rows fails with WP_ERR_ARG before anything is written).  T_A, T_B: the ids of those rows exactly as
 * wp_linear_encode_rows gives them, la, lb their lengths; specials = (cls_id >= 0) + (sep_id >= 0) * (pairs ? 2 : 1);
 * B = max_len - specials is the id budget of an output row.
 * An output row is [cls] A' [sep], or [cls] A' [sep] B' [sep] for pairs (an empty B' keeps its [sep]), then pad_id up
 * to max_len.  token_type_ids: 0 for [cls], A' and the first [sep], 1 for B' and the second [sep], 0 for the padding.
 * lengths[r] counts everything but the padding; sample[r] is the sample of output row r (HF
 * overflow_to_sample_mapping).  With unit WP_OFFSETS_* offsets[r][col] = [begin, end) of that id relative to its own
 * document, as wp_linear_encode_rows gives it; specials and padding get (0, 0).
 * stride == -1: one output row per sample, sample[r] == r.
 *   WP_TRUNC_LONGEST_FIRST: what HF's fast (Rust) tokenizer does, not the loop of the slow one: if la + lb <= B all is
 *     kept; else the shorter side (A on a tie) keeps min(short, max(B - long, B / 2)) and the longer one the rest of B:
 *       la <= lb: ka = min(la, max(B - lb, B / 2)), kb = min(lb, B - ka);  else kb = min(lb, max(B - la, B / 2)), ka = min(la, B - kb)
 *     e.g. (la, lb, B) = (5, 5, 7) -> (3, 4), (6, 5, 7) -> (4, 3), (4, 10, 7) -> (3, 4).  pairs == 0: ka = min(la, B).
 *   WP_TRUNC_ONLY_FIRST / WP_TRUNC_ONLY_SECOND: window 0 of the windows below, taken with stride 0.
 * stride >= 0 (WP_TRUNC_ONLY_FIRST / _SECOND only): one side is cut into windows (A / B; A when pairs == 0), the other
 *   is fixed and repeated in every window.  st = max(stride, 0).  The fixed side keeps kF = min(lF, B - st - 1) ids (0
 *   without pairs); W = B - kF >= st + 1 is the window size and step = W - st >= 1.  A windowed side of l ids gives 1
 *   window if l <= W, else 1 + ceil((l - W) / step); window j holds its ids [j * step, min(l, j * step + W)).  The
 *   windows of sample s are consecutive output rows, in order, in front of those of sample s + 1.  Where the fixed side
 *   fits this is HF's [encoding] + encoding.overflowing; where it does not, HF raises and this call cuts it to
 *   B - st - 1 ids, so that it is a total function.
 * WP_ERR_ARG, in the host entry point before a device is touched: spec NULL, an unknown truncation, stride < -1, pairs
 * not 0 / 1, max_len < 1 or B < 0, WP_TRUNC_LONGEST_FIRST with stride >= 0, WP_TRUNC_ONLY_SECOND with pairs == 0,
 * WP_TRUNC_ONLY_FIRST / _SECOND with B < st + 1 (no room for a window), an odd number of rows for pairs (device entry
 * point, lines mode: once the lines are counted, before any output is written), a unit other than -1, 0, 1.
 * WP_ERR_TOO_LARGE: more output rows than UINT32_MAX, more samples than INT32_MAX, or a batch whose size overflows size_t.
 * Empty input (nbytes == 0, or explicit rows that are all empty) needs no device in the host entry point. */
#define WP_TRUNC_LONGEST_FIRST 0
#define WP_TRUNC_ONLY_FIRST 1
#define WP_TRUNC_ONLY_SECOND 2
typedef struct { int32_t max_len, cls_id, sep_id, pad_id, pairs, truncation, stride, unit; } wp_inputs_spec;
typedef struct { int32_t *input_ids, *token_type_ids, *lengths, *sample; uint32_t *offsets; } wp_inputs;
/* host text in; five blocks out: input_ids, token_type_ids [n_out, max_len], lengths, sample [n_out], offsets
 * [n_out, max_len, 2] (free each with wp_free; offsets NULL when spec->unit == -1, all NULL when n_out == 0) */
int wp_linear_encode_inputs(wp_vocab *v, const char *utf8, size_t nbytes, const int64_t *doc_off, size_t n_docs,
                            const wp_inputs_spec *spec, wp_inputs *out, size_t *n_out, size_t *n_samples);
/* device text and doc_off (contracts of wp_linear_encode_rows_device) into caller-owned device buffers of
 * capacity_rows rows (offsets: 8-byte aligned; may be NULL when unit == -1); nothing behind n_out rows is touched; too
 * little room: WP_ERR_ARG, the needed count in *n_out, nothing written.  The call returns when the batch is complete:
 * without windows it waits as often as wp_linear_encode_padded_device, with windows once more (for the row count). */
int wp_linear_encode_inputs_device(wp_vocab *v, const void *d_utf8, size_t nbytes, const int64_t *d_doc_off, size_t n_docs,
                                   const wp_inputs_spec *spec, const wp_inputs *d_out, size_t capacity_rows,
                                   size_t *n_out, size_t *n_samples);

/* ---- masking (an addition: tf_text mask_language_model, HF DataCollatorForLanguageModeling / ForWholeWordMask, Encoding.word_ids()) ----
 * The masked-language-model transform of a batch in[n_rows][max_len] of int32 ids with an optional lengths[n_rows]: what
 * the padded / inputs calls produce, or any id batch the caller made.  lengths == NULL: every column is inside; a given
 * length is clamped to [0, max_len].  V = wp_vocab_size, f(x) = wp_vocab_token_flags(x).  For row r, column c, x = in[r][c]:
 *   outside(c): c >= len_r, or x < 0, or x >= V, or x equals one of cls_id, sep_id, pad_id that is >= 0
 *   solo(c):    !outside && (f(x) & 6)                — a special or malformed token ([UNK] and its kin) is a word of its own
 *   cont(c):    !outside && !solo && !(f(x) & 1)      — a "##" token
 *   start(c):   !outside(c) && (!cont(c) || c == 0 || outside(c - 1) || solo(c - 1))   — a window that begins inside a word begins a word
 *   word_ids[r][c]: -1 if outside, else (the number of start(c') for o < c' <= c) - 1, o the last outside column before c
 *     (-1 if none): the count restarts behind every special, so sequence B of a pair starts at 0 again (HF word_ids())
 *   w(c): the last c' <= c with start(c');  the selection unit u(c) is w(c) with whole_word == 1, c with whole_word == 0;
 *     a unit is selectable when !solo(u(c))
 *   selected(c): !outside(c) && selectable && draw(seed, row_base + r, u(c), 0) < select_q32
 *   a selected c: labels = x;  t = draw(seed, row_base + r, c, 1);  t < mask_q32: out = mask_id;  else
 *     t < mask_q32 + random_q32: out = (draw(seed, row_base + r, c, 2) * V) >> 32;  else out = x
 *   any other c: out = x, labels = ignore_id
 * Every cell of the n_rows rows is written, padding included; nothing behind row n_rows is.  `out` may be the buffer
 * `in` is (a cell is read before it is written, and no other cell is read for it).
 * select_q32, mask_q32, random_q32: probabilities times 2^32, in [0, 2^32] (2^32: always; a draw is a 32-bit value and
 * the comparison is made in 64 bits); mask_q32 + random_q32 <= 2^32.  The draw is part of the contract — the same
 * seed gives the same batch on every device and in every release.  All arithmetic mod 2^64, G = 0x9E3779B97F4A7C15:
 *   mix(x): x ^= x >> 30; x *= 0xBF58476D1CE4E5B9; x ^= x >> 27; x *= 0x94D049BB133111EB; x ^= x >> 31
 *   draw(seed, row, col, stream) = mix(mix(seed + G * (row + 1)) + G * (4 * col + stream + 1)) >> 32
 * row_base: the row number of row 0, so that a batch masked in slices gives the rows the whole batch would give.
 * The word-ids calls read max_len, cls_id, sep_id and pad_id of the spec only.
 * WP_ERR_ARG (host entry points: before a device is touched): spec NULL, a required pointer NULL, max_len < 1,
 * whole_word not 0 / 1, a q32 above 2^32, mask_q32 + random_q32 > 2^32, mask_id < 0 (mask calls).  WP_ERR_TOO_LARGE:
 * n_rows > INT32_MAX, or n_rows * max_len overflows.  n_rows == 0 needs no device and gives NULL blocks.  The device
 * calls run on the handle's device and stream, wait once (for the counters) and return when the batch is complete. */
typedef struct { int32_t max_len, cls_id, sep_id, pad_id, mask_id, ignore_id, whole_word, reserved;
                 uint64_t select_q32, mask_q32, random_q32, seed, row_base; } wp_mask_spec;
/* host ids in; word_ids [n_rows, max_len] out as a block (free with wp_free) */
int wp_word_ids(wp_vocab *v, const int32_t *input_ids, const int32_t *lengths, size_t n_rows, const wp_mask_spec *spec,
                int32_t **word_ids);
/* device ids in, a caller-owned device buffer of n_rows * max_len int32 out */
int wp_word_ids_device(wp_vocab *v, const int32_t *d_input_ids, const int32_t *d_lengths, size_t n_rows,
                       const wp_mask_spec *spec, int32_t *d_word_ids);
/* host ids in; masked, labels and (word_ids != NULL) word_ids [n_rows, max_len] out as blocks (free each with wp_free) */
int wp_mlm_mask(wp_vocab *v, const int32_t *input_ids, const int32_t *lengths, size_t n_rows, const wp_mask_spec *spec,
                int32_t **masked, int32_t **labels, int32_t **word_ids);
/* device ids in, caller-owned device buffers out (d_masked may be d_input_ids; d_word_ids may be NULL: not wanted) */
int wp_mlm_mask_device(wp_vocab *v, const int32_t *d_input_ids, const int32_t *d_lengths, size_t n_rows,
                       const wp_mask_spec *spec, int32_t *d_masked, int32_t *d_labels, int32_t *d_word_ids);
/* The statistics of the last mask or word-ids call, in a struct of its own (wp_stats keeps its size).  n_random and
 * n_kept count the branch taken, not whether the id changed.  A word-ids call fills n_rows and n_words only.  The other
 * statistics (wp_stats, wp_inputs_stats, ...) keep what the last encode left: a mask call runs no encode. */
typedef struct {
  int64_t n_rows;            /* rows of the call; -1: the last call was no mask call                                      */
  int64_t n_words;           /* cells with start(c)                                                                       */
  int64_t n_selected;        /* selected cells                                                                            */
  int64_t n_selected_units;  /* selected units: words with whole_word == 1, cells with 0                                  */
  int64_t n_masked, n_random, n_kept; /* selected cells by the branch they took                                            */
  int32_t whole_word, reserved; /* of the call's wp_mask_spec                                                             */
} wp_mask_stats;
int wp_get_mask_stats(const wp_vocab *v, wp_mask_stats *out);

/* ---- detokenize (an addition: ids back to text; tokenizers.decoders.WordPiece(prefix="##", cleanup=...), which is what HF
 * Tokenizer.decode runs; "decode" names the UTF-8 stage in this library, hence the other word) ----
 * That decoder works token by token: the first token stands as it is, a later one loses a leading "##" or else gets one
 * space in front, and with cleanup each such per-token string goes through the chain
 *   " ." -> ".", " ?" -> "?", " !" -> "!", " ," -> ",", " ' " -> "'", " n't" -> "n't", " 'm" -> "'m",
 *   " do not" -> " don't", " 's" -> "'s", " 've" -> "'ve", " 're" -> "'re"          (in this order, over bytes)
 * so the text of a row is a plain concatenation of per-id byte strings.  line(i) = wp_vocab_token_utf8(i) with "##" put
 * back in front when bit 0 of wp_vocab_token_flags(i) is clear; C = the chain with cleanup == 1, the identity with 0:
 *   form0(i) = C(line(i))                                  — the first kept cell of a row
 *   form1(i) = C(line(i) without its leading "##")         — a later cell, continuation token
 *   form1(i) = C(" " + line(i))                            — a later cell, any other token
 * (The whole-string clean-up that `transformers` may apply on top of Tokenizer.decode works across tokens and is out of
 * scope.)  V = wp_vocab_size.  For a cell x of row r:
 *   dropped: x < 0, x >= V, or wp_vocab_token_flags(x) & 4 (malformed) — the ids word_piece::fast::decode skips
 *   skipped: not dropped, and x is one of skip_ids[0 .. n_skip) (n_skip <= 8): [CLS], [SEP], [PAD] ... (skip_special_tokens)
 *   kept:    neither.  The row's text: form0 of its first kept cell, form1 of every later kept cell, then, with
 *   terminator in 0..255, that one byte (empty rows included; -1: nothing).  With '\n' the text is the joined documents
 *   form wp_linear_encode_rows takes, and text_off its doc_off.
 * Result: text, n_bytes bytes, the rows back to back; text_off, int64[n_rows + 1], text_off[0] == 0, text_off[n_rows] ==
 * n_bytes.  Two layouts of the rows, one set of kernels (csrc/detok.h):
 *   ragged (max_len == 0): ids[row_splits[n_rows]] with row_splits[0 .. n_rows] as wp_linear_encode_rows returns them:
 *     row_splits[0] == 0, no descent — checked on the host by the host entry point, in a kernel by the device entry
 *     point, which fails with WP_ERR_ARG before text is produced; lengths is not read
 *   padded (max_len >= 1): ids[n_rows][max_len] with lengths[n_rows] (NULL: full rows), each clamped to [0, max_len];
 *     the cells behind a row's length are no cells: not in the text, not in the statistics; row_splits is not read
 * WP_ERR_ARG (host entry point: before a device is touched): spec NULL, cleanup not 0 / 1, terminator outside [-1, 255],
 * n_skip outside [0, 8], max_len < 0, a required pointer NULL (a ragged call without row_splits, ids NULL where there
 * are cells, an out-pointer), bad row_splits, a device pointer that is not aligned to its element.  WP_ERR_TOO_LARGE:
 * n_rows > INT32_MAX, more than INT32_MAX cells (n_rows * max_len is computed without overflow), or a text of 2^32
 * bytes or more, found from a 64-bit total before the write pass runs.  The size rules are checked before the pointers.
 * n_rows == 0: the host entry point needs no device and gives text == NULL, n_bytes == 0 and a one-entry text_off (0).
 * text == NULL also for n_bytes == 0 with rows.  The device call runs on the handle's device and stream and returns when
 * the text is complete (it waits for the total to size the text, and a ragged call for the check of row_splits).
 * The pieces are a per-context table built by a handle's first detokenize call, for both cleanup values at once. */
typedef struct { int32_t max_len, cleanup, terminator, n_skip; int32_t skip_ids[8]; } wp_detok_spec;
/* host ids in; text and text_off out as blocks (free each with wp_free) */
int wp_detokenize(wp_vocab *v, const int32_t *ids, const int64_t *row_splits, const int32_t *lengths, size_t n_rows,
                  const wp_detok_spec *spec, char **text, int64_t **text_off, size_t *n_bytes);
/* device ids in; text and text_off in device memory, owned by the handle until its next call */
int wp_detokenize_device(wp_vocab *v, const int32_t *d_ids, const int64_t *d_row_splits, const int32_t *d_lengths,
                         size_t n_rows, const wp_detok_spec *spec, const void **d_text, const int64_t **d_text_off,
                         size_t *n_bytes);
/* form `form` (0 / 1) of id with cleanup 0 / 1: the host statement of the table the kernels read, without a device.
 * Returns the byte length and copies at most cap bytes; -1: id out of range or malformed, another form or cleanup. */
int64_t wp_detok_piece(const wp_vocab *v, int64_t id, int form, int cleanup, char *buf, size_t cap);
/* The statistics of the last detokenize call, in a struct of its own (wp_stats keeps its size); every other statistic
 * keeps what the last encode left.  n_cells = n_kept + n_skipped + n_dropped (padded: the cells below the lengths). */
typedef struct { int64_t n_rows, n_cells, n_kept, n_skipped, n_dropped, n_bytes; } wp_detok_stats;
int wp_get_detok_stats(const wp_vocab *v, wp_detok_stats *out); /* n_rows == -1: no such call yet */

/* ---- pack (an addition: several encoded documents per fixed-length row; seqio / T5 trim_and_pack_dataset with its
 * segment ids and positions, HF run_mlm.py group_texts) ----
 * Ragged ids in — ids[n_ids] with row_splits[0 .. n_docs], the layout the rows call returns and the detokenize call
 * takes — a packed batch of n_out rows of max_len cells out.  No encode runs and no vocabulary is read; the ids are not
 * range-checked.  Document i is T_i of l_i ids.  L = max_len, s = (bos_id >= 0) + (eos_id >= 0), B = L - s.
 * Pieces, in document order, numbered k = 0 .. n_p - 1: a document with l_i == 0 gives none;
 *   WP_PACK_STREAM:                            one piece (i, 0, l_i); long_docs is not read
 *   WP_PACK_NEXT_FIT + WP_PACK_LONG_TRUNCATE:  one piece (i, 0, min(l_i, B)); a document that loses ids counts in n_cut,
 *                                              its lost ids in n_ids_cut
 *   WP_PACK_NEXT_FIT + WP_PACK_LONG_SPLIT:     ceil(l_i / B) pieces (i, j B, min(B, l_i - j B))
 * The unit of a piece (i, f, n) is [bos] T_i[f : f + n] [eos], each special only where its id is >= 0: u = n + s cells.
 * P[k]: the sum of the unit lengths in front of piece k;  N = P[n_p].
 * Rows.  WP_PACK_STREAM: the units back to back are one stream of N cells, row r is its cells [r L, min(N, (r + 1) L)),
 *   n_out = ceil(N / L); a unit may straddle rows (group_texts with the remainder kept and padded).
 *   WP_PACK_NEXT_FIT: no unit is longer than L and none is split; row j holds the units [k_j, k_{j+1}), k_0 = 0, k_{j+1}
 *   the first k > k_j with P[k + 1] - P[k_j] > L, or n_p: order is kept, and a unit opens a new row exactly when it does
 *   not fit behind the ones before it (with WP_PACK_LONG_TRUNCATE: trim_and_pack_dataset for one feature).
 * Cells.  Every cell of the n_out rows is written, padding included; nothing behind row n_out is.
 *   input_ids:    the unit's cell; pad_id in a padding cell
 *   lengths[r]:   the cells of row r that are no padding, in [1, L]
 *   segment_ids:  1 + the number of columns c' in (0, c] at which a unit begins; 0 in a padding cell (the unit that goes on
 *                 from the row before in stream mode is segment 1: the T5 *_segment_ids convention)
 *   position_ids: c minus the column of the last such beginning at or before c (column 0 if there is none); 0 in a padding
 *                 cell.  Positions stay below L whatever a document's length
 *   source:       the index into ids of an id cell; -1 for specials and padding.  One gather x[source] carries per-token
 *                 data (the offsets of the rows call) into the batch.  Outside NEXT_FIT + LONG_TRUNCATE the entries >= 0
 *                 are 0 .. n_ids - 1 in row-major order
 * want (WP_PACK_WANT_*) names the optional outputs that are produced: the host entry point returns NULL for the others,
 * the device entry point reads only the pointers of the wanted ones.  input_ids and lengths are always produced.
 * WP_ERR_ARG (host entry point: before a device is touched): spec NULL, an unknown mode, an unknown long_docs under
 * NEXT_FIT, want with bits outside 7, max_len < 1 or B < 1, a required pointer NULL (row_splits, ids where there are
 * ids, an out-pointer, a wanted output of the device call), bad row_splits (row_splits[0] != 0 or a descent: checked on
 * the host by the host entry point, in a kernel by the device entry point, before anything is written), a device pointer
 * that is not aligned to its element; in the device call capacity_rows < n_out, with the needed count in *n_out and
 * nothing written.  WP_ERR_TOO_LARGE, from 64-bit totals before the write pass runs: n_docs, n_ids, N or n_out *
 * max_len above INT32_MAX.  The size rules are checked before the pointers.  n_docs == 0 or only empty documents:
 * n_out == 0, every block NULL, and the host entry point needs no device.  The device call runs on the handle's device
 * and stream, uses buffers of its own (a rows result of the same handle may be fed straight in) and returns when the
 * batch is complete. */
#define WP_PACK_NEXT_FIT 0
#define WP_PACK_STREAM   1
#define WP_PACK_LONG_TRUNCATE 0
#define WP_PACK_LONG_SPLIT    1
#define WP_PACK_WANT_SEGMENTS  1
#define WP_PACK_WANT_POSITIONS 2
#define WP_PACK_WANT_SOURCE    4
typedef struct { int32_t max_len, mode, bos_id, eos_id, pad_id, long_docs, want, reserved; } wp_pack_spec;
/* the blocks of a packed batch: input_ids, segment_ids, position_ids, source int32 [n_out, max_len], lengths int32 [n_out] */
typedef struct { int32_t *input_ids, *segment_ids, *position_ids, *source, *lengths; } wp_packed;
/* host ids in; the blocks out (free each with wp_free) */
int wp_pack_sequences(wp_vocab *v, const int32_t *ids, const int64_t *row_splits, size_t n_docs,
                      const wp_pack_spec *spec, wp_packed *out, size_t *n_out);
/* device ids in, caller-owned device buffers of capacity_rows rows out */
int wp_pack_sequences_device(wp_vocab *v, const int32_t *d_ids, const int64_t *d_row_splits, size_t n_docs,
                             const wp_pack_spec *spec, const wp_packed *d_out, size_t capacity_rows, size_t *n_out);
/* The statistics of the last pack call, in a struct of its own (wp_stats keeps its size); every other statistic keeps
 * what the last encode left.  n_cells: the sum of lengths (N); n_segments: the sum over the rows of the row's largest
 * segment id. */
typedef struct { int64_t n_docs, n_empty, n_cut, n_ids_cut, n_pieces, n_out, n_cells, n_segments; } wp_pack_stats;
int wp_get_pack_stats(const wp_vocab *v, wp_pack_stats *out); /* n_docs == -1: no such call yet */

/* ---- special tokens (an addition: HF tokenizer.add_special_tokens / all_special_ids — BertTokenizer with
 * split_special_tokens=False keeps "[MASK]", "[SEP]" ... in a text whole) ----
 * The encoder itself never matches a vocabulary line of the form "[...]" (utils.cpp:143-146): "[CLS] a" gives "[", "CLS",
 * "]", "a".  These calls take a list of such lines' ids and keep every listed line that stands in the text as its id, the
 * way that tokenizer does: the text is cut at them before anything else (before WP_OPT_NORMALIZE too: "[mask]" is
 * ordinary text), so "foo[MASK]bar" gives foo, [MASK], bar.
 * Eligible ids.  An id may be listed when it is in range, bit 1 of wp_vocab_token_flags is set (special) and bit 2 is
 * clear (malformed), its line has at most 64 bytes, every byte of it is in 0x21..0x7E, and '[' is its first byte only
 * and ']' its last byte only.  Any other id, and two listed ids with the same line, fail with WP_ERR_ARG and a message
 * that names the id; the same id twice is fine.  n_ids is in [0, 4096]; ids is host memory in every entry point.
 * Literals.  At a byte '[' of the caller's text take the bytes up to and including the next ']'.  They are a literal when
 * they lie inside nbytes, number at most 64, hold only bytes 0x21..0x7E with no further '[', and equal a listed line.  So
 * the candidate at a '[' is decided by the text alone, and two literals never overlap ("[[MASK]]" holds one, at byte 1).
 * Result.  That of wp_linear_encode_offsets on the text with every literal's bytes set to 0x20, with (id, [start, end))
 * of every literal merged in by position; start and end in `unit` — bytes, or code points, of the caller's text.  unit
 * -1: only the ids come back (offsets may be NULL).  No span of the inner encode covers a blanked byte, so positions are
 * distinct and offsets keep referring to the caller's text.  WP_OPT_NORMALIZE applies to the blanked text only.
 * Documents form.  Rows as wp_linear_encode_rows takes them (explicit rows or lines; both routes; empty rows; the row
 * rules under WP_OPT_NORMALIZE).  Row i and its document-relative offsets are the flat call on document i.
 * A text without a literal gives exactly the plain call's result (wp_linear_encode_offsets / wp_linear_encode_rows), and
 * so does n_ids == 0 in the spec.  Buffers, ownership and the order of errors are those of the offsets and rows calls:
 * the host forms report every argument error before a device is touched, and need no device for an empty text; without
 * a device the result is WP_ERR_NO_DEVICE.  nbytes > UINT32_MAX fails with WP_ERR_TOO_LARGE in every unit.
 * On the device (csrc/special.h): one pass over the text finds the literals (one table lookup per '[', a bisection over
 * the sorted lines), the count comes to the host, and with none the plain path runs on the caller's buffer.  Else the
 * text is copied and blanked, encoded through the offsets or rows path as it stands, and one pass per literal and one
 * over the ids put the literals in. */
typedef struct { const int32_t *ids; int32_t n_ids; } wp_special_spec;   /* host memory, n_ids in [0, 4096] */
/* host text in; ids and offsets out as blocks (free each with wp_free; NULL when n_ids == 0, offsets NULL when unit == -1) */
int wp_linear_encode_special(wp_vocab *v, const char *utf8, size_t nbytes, const wp_special_spec *spec, int unit,
                             int32_t **ids, uint32_t **offsets, size_t *n_ids);
/* device text (buffer contract of wp_linear_encode_device); the results stay there, owned by the handle until its next call */
int wp_linear_encode_special_device(wp_vocab *v, const void *d_utf8, size_t nbytes, const wp_special_spec *spec, int unit,
                                    const int32_t **d_ids, const uint32_t **d_offsets, size_t *n_ids);
/* the documents form: arguments and blocks of wp_linear_encode_rows, plus the spec */
int wp_linear_encode_special_rows(wp_vocab *v, const char *utf8, size_t nbytes, const int64_t *doc_off, size_t n_docs,
                                  const wp_special_spec *spec, int unit, int32_t **ids, int64_t **row_splits,
                                  uint32_t **offsets, size_t *n_ids, size_t *n_rows);
/* ... of wp_linear_encode_rows_device, plus the spec */
int wp_linear_encode_special_rows_device(wp_vocab *v, const void *d_utf8, size_t nbytes, const int64_t *d_doc_off,
                                         size_t n_docs, const wp_special_spec *spec, int unit, const int32_t **d_ids,
                                         const int64_t **d_row_splits, const uint32_t **d_offsets, size_t *n_ids,
                                         size_t *n_rows);
/* The statistics of the last special-tokens call, in a struct of its own (wp_stats keeps its size): the literals found,
 * the ids of the result (literals included), its rows (-1: the flat form) and the entries of the spec.  wp_stats and its
 * kin hold what the inner encode left, with n_ids and offsets_unit those of the call.  Any other encode on the handle
 * starts these statistics over. */
typedef struct { int64_t n_literals, n_ids, n_rows, n_listed; } wp_special_stats;
int wp_get_special_stats(const wp_vocab *v, wp_special_stats *out); /* n_literals == -1: no such call yet, or another encode since */

/* ---- span alignment (an addition: the label side of a fine-tuning batch — HF course preprocess_training_examples for
 * extractive QA, align_labels_with_tokens / Encoding.char_to_token for token classification) ----
 * Labelled character spans in, per-cell labels and per-row answer positions out, for a batch whose offsets are already
 * there: no encode runs and no vocabulary is read.
 * Spans, ragged per sample: span_splits[0 .. n_samples] (int64; [0] == 0, never descends, [n_samples] == n_spans),
 * spans[n_spans][2] (uint32, [begin, end)) and span_labels[n_spans] (int32).  Spans are in the unit and frame of the
 * batch's offsets (relative to the document they label; bytes or code points: the call does not know which).  Within a
 * sample they are non-empty, sorted and disjoint: begin < end, and end[j] <= begin[j + 1].
 * Padded form.  offsets[n_rows][max_len][2], token_type_ids[n_rows][max_len] (NULL: all 0), lengths[n_rows] (NULL:
 * max_len; a given length is clamped to [0, max_len]) and sample[n_rows] (NULL: sample[r] = r) as the inputs call hands
 * them out.  side: the sequence the spans label, 0 (A) or 1 (B, the context of a question-first pair).
 * For row r and column c, (b, e) the cell's offsets, s the row's sample and J = [span_splits[s], span_splits[s + 1]):
 *   token(c):   c < len_r, e > b and type(r, c) == side   (specials and padding carry (0, 0): never tokens)
 *   j(c):       the smallest j in J with end[j] > b
 *   covered(c): token(c), j(c) exists, and begin[j] < e   (overlap; a token over two spans takes the first)
 *   span_index[r][c] = j(c), an index into the flat span list, if covered, else -1
 *   labels[r][c] = ignore_id if !token(c);  outside_label if token(c) and not covered;
 *                  else span_labels[j] + (b > begin[j] ? inside_add : 0)
 * The begin cell of a span is the one that starts at or before the span's begin: the cell alone decides, so a token has
 * the same label in every window that holds it, and a window that opens inside an entity opens with an inside label.  A
 * span that begins in a gap in front of a token has no begin cell.
 *   start_positions[r], end_positions[r]: a = the first span of s.  no_answer in both when s has no span, when the row
 *   has no token cell, or when begin[a] < lo or end[a] > hi, lo / hi the smallest b / the largest e of the row's token
 *   cells (the window does not hold the whole answer).  Else start = the largest token column with b <= begin[a], end =
 *   the smallest token column with e >= end[a].  This is the loop of preprocess_training_examples on the context cells
 *   alone; it never walks into [SEP] or the padding.  Where several cells share one source span (WP_OPT_NORMALIZE),
 *   start may lie behind end: the rule is literal.
 * Ragged form.  offsets[n_ids][2] with row_splits[0 .. n_rows] as the rows call returns them: row i is sample i
 * (n_samples == n_rows), every cell is a token, the same cell rule; labels[n_ids] and span_index[n_ids], no positions,
 * and max_len and side of the spec are not read.  One gather through `source` of a packed batch carries them into it.
 * Outputs.  want (WP_ALIGN_*) names the blocks a host entry point produces (NULL for the others; each freed with
 * wp_free; all NULL without rows); a device entry point takes caller-owned buffers, NULL for an output that is not
 * wanted (start and end positions: both or neither), writes every cell of the n_rows rows and nothing behind them, and
 * does not read want.  At least one output must be wanted.
 * WP_ERR_ARG: spec NULL, max_len < 1 (padded form), side not 0 / 1, side 1 without token_type_ids, want without a
 * known bit or with an unknown one (WP_ALIGN_POSITIONS in the ragged form), labels wanted without span_labels, a
 * required pointer NULL, a device pointer that is not aligned (offsets, spans and splits to 8 bytes, everything else to
 * 4); and, with the first offender named: row_splits or span_splits that do not start at 0, descend or end elsewhere
 * than at n_ids / n_spans, a span that is empty or begins before the one in front of it in its sample ends, a row whose
 * sample is outside [0, n_samples).  The host entry points check all of this before a device is touched; the device entry
 * points check the arrays in a kernel with one word of result, and the kernels behind it write nothing where it
 * failed.  WP_ERR_TOO_LARGE: n_rows, n_samples, n_spans or n_ids above INT32_MAX, n_rows * max_len too large.
 * The device calls run on the handle's device and stream and return after one wait, for the counters. */
#define WP_ALIGN_LABELS     1
#define WP_ALIGN_SPAN_INDEX 2
#define WP_ALIGN_POSITIONS  4
typedef struct { int32_t max_len, side, outside_label, inside_add, ignore_id, no_answer, want, reserved; } wp_align_spec;
/* host arrays in; labels, span_index int32 [n_rows, max_len] and start_positions, end_positions int32 [n_rows] out as blocks */
int wp_align(wp_vocab *v, const uint32_t *offsets, const int32_t *token_type_ids, const int32_t *lengths,
             const int32_t *sample, size_t n_rows, const int64_t *span_splits, size_t n_samples, const uint32_t *spans,
             const int32_t *span_labels, size_t n_spans, const wp_align_spec *spec, int32_t **labels,
             int32_t **span_index, int32_t **start_positions, int32_t **end_positions);
/* device arrays in, caller-owned device buffers out */
int wp_align_device(wp_vocab *v, const uint32_t *d_offsets, const int32_t *d_token_type_ids, const int32_t *d_lengths,
                    const int32_t *d_sample, size_t n_rows, const int64_t *d_span_splits, size_t n_samples,
                    const uint32_t *d_spans, const int32_t *d_span_labels, size_t n_spans, const wp_align_spec *spec,
                    int32_t *d_labels, int32_t *d_span_index, int32_t *d_start_positions, int32_t *d_end_positions);
/* the ragged form: host arrays in; labels, span_index int32 [n_ids] out as blocks (n_ids = row_splits[n_rows]) */
int wp_align_rows(wp_vocab *v, const uint32_t *offsets, const int64_t *row_splits, size_t n_rows,
                  const int64_t *span_splits, const uint32_t *spans, const int32_t *span_labels, size_t n_spans,
                  const wp_align_spec *spec, int32_t **labels, int32_t **span_index);
/* ... device arrays in (n_ids given: it must be the last entry of d_row_splits), caller-owned device buffers out */
int wp_align_rows_device(wp_vocab *v, const uint32_t *d_offsets, const int64_t *d_row_splits, size_t n_rows, size_t n_ids,
                         const int64_t *d_span_splits, const uint32_t *d_spans, const int32_t *d_span_labels,
                         size_t n_spans, const wp_align_spec *spec, int32_t *d_labels, int32_t *d_span_index);
/* The statistics of the last align call, in a struct of its own (the other statistics structs keep their sizes); every
 * other statistic keeps what the last encode left.  n_tokens: token cells; n_covered, n_begin: covered cells and, of
 * those, begin cells (0 when neither labels nor span_index were wanted: no span is looked up then); n_spans: of the
 * call; n_answer_rows + n_no_answer_rows == n_rows when positions were wanted, both 0 otherwise. */
typedef struct { int64_t n_rows, n_tokens, n_covered, n_begin, n_spans, n_answer_rows, n_no_answer_rows; } wp_align_stats;
int wp_get_align_stats(const wp_vocab *v, wp_align_stats *out); /* n_rows == -1: the last call was no align call */

/* ---- word counts (an addition: the "word -> count" table a vocabulary learner starts from — HF WordPieceTrainer, TF
 * Text wordpiece_vocab —, collections.Counter over the split text) ----
 * The distinct words of a text with their counts, and per occurrence the word's index in that table, computed on the
 * device.  No vocabulary is read: two handles with different vocabularies give the same table.
 * Text.  What is counted is the text wp_normalize[_device] gives for the handle's WP_OPT_NORMALIZE flags (flags 0: the
 * valid UTF-8 of the input, invalid sequences dropped).
 * Words.  c[p] the code points of that text: p starts a word iff !is_space(c[p]) and (p == 0 or spacing(c[p]) or
 * spacing(c[p - 1])), and the word runs to the next word start or the next space (the classes of utf8.cpp:10-29:
 * spacing = space, punctuation or is_chinese).  So a maximal run of non-spacing characters is a word, every punctuation
 * character and every is_chinese character is a word of its own, and blanks belong to no word: the units the walk of the
 * encoder tokenises.  Only the vocabulary-independent classes count; the handle's soft list and the special-token list
 * play no part, so a literal "[MASK]" in the text counts as "[", "MASK", "]".
 * Long words.  A word of more than max_word_bytes UTF-8 bytes (0: 256; else 1..1024) is not listed: it counts in
 * wp_count_stats.n_long and in n_words, and takes a slot of word_index with value -1.
 * Result.  The distinct listed words whose count is at least min_count (0: 1), n_distinct of them:
 *   words       their UTF-8 bytes back to back, each followed by the byte `terminator` when that is in 0..255 (-1: nothing
 *               is added); n_bytes bytes.  With terminator '\n' this is the joined-documents text of
 *               wp_linear_encode_rows, one word per row, and word_off is its doc_off.
 *   word_off    int64 [n_distinct + 1]: word k lies at [word_off[k], word_off[k + 1]), its terminator, if any, last
 *   counts      int64 [n_distinct]
 *   word_index  int32 [n_words], with WP_COUNT_WANT_INDEX: for every word occurrence in text order the index of its
 *               word in the table, -1 where the word is long or was dropped by min_count
 * Order.  WP_COUNT_ORDER_FIRST: by first occurrence in the text (iterating collections.Counter(words));
 * WP_COUNT_ORDER_COUNT: count descending, ties by first occurrence (Counter(words).most_common()).  Neither depends on a
 * hash.
 * Exactness.  Two words are the same iff their bytes are equal.  Words are grouped by a 64-bit hash of their bytes, and
 * every member of a group is then compared byte by byte with the group's first occurrence; what differs is grouped again
 * under another seed (wp_count_stats.n_rounds, n_collided).  hash_bits (0: 64; else 8..64) narrows the hash so that a
 * test reaches those rounds with few words; it never changes a result.  reserved must be 0.
 * Host form: the blocks of *out are malloc'd, each freed with wp_free; a block is NULL where it is empty or was not asked
 * for (word_off always holds at least {0}).  The empty text is answered without a device.  Device form: d_utf8 under the
 * buffer contract of wp_linear_encode_device; the arrays of *d_out are device memory owned by the handle until its next
 * call.  Both return when the table is complete (one wait per size the host needs, one per round).
 * WP_ERR_ARG, before a device is touched and with the field named: spec or out NULL, order not 0 / 1, max_word_bytes
 * outside [0, 1024], terminator outside [-1, 255], want with an unknown bit, hash_bits not 0 and outside [8, 64],
 * reserved not 0, min_count negative.  WP_ERR_TOO_LARGE: a normalised text of more than UINT32_MAX bytes, 2^31 words or
 * more. */
#define WP_COUNT_ORDER_FIRST 0
#define WP_COUNT_ORDER_COUNT 1
#define WP_COUNT_WANT_INDEX  1
typedef struct { int32_t order, max_word_bytes, terminator, want, hash_bits, reserved; int64_t min_count; } wp_count_spec;
typedef struct { uint8_t *words; int64_t *word_off, *counts; int32_t *word_index; int64_t n_distinct, n_words, n_bytes; } wp_word_counts;
int wp_count_words(wp_vocab *v, const char *utf8, size_t nbytes, const wp_count_spec *spec, wp_word_counts *out);
int wp_count_words_device(wp_vocab *v, const void *d_utf8, size_t nbytes, const wp_count_spec *spec, wp_word_counts *d_out);
/* The statistics of the last count call, in a struct of its own (the other statistics structs keep their sizes); every
 * other statistic keeps what the last encode left, and an encode clears these as it clears every layer's.
 * n_words: every word, long ones included; n_distinct: the entries of the table; n_long: occurrences of long words;
 * n_below_min: distinct listed words that min_count dropped; n_text_bytes: bytes of the counted (normalised) text;
 * n_rounds: grouping rounds (0 without listed words, 1 unless hashes collided); n_collided: the word occurrences that
 * round 0 left for later rounds.  With WP_OPT_STAGE_TIMING a count call also leaves its device times (HIP events) in the
 * fields of wp_stats an encode times itself in: ms_normalize (the pre-pass), ms_decode (word starts, ends and the list),
 * ms_sa (the grouping rounds: keys, sort, comparison), ms_walk (filter, order, gather, index), ms_total (their sum),
 * and ms_radix_scatter, radix_passes, radix_pass_elems, radix_pass_bytes of its full-size sorts. */
typedef struct { int64_t n_words, n_distinct, n_long, n_below_min, n_text_bytes, n_rounds, n_collided; } wp_count_stats;
int wp_get_count_stats(const wp_vocab *v, wp_count_stats *out);   /* n_words == -1: no such call yet, or an encode since */

/* ---- vocabulary learner (an addition: a WordPiece vocabulary from the word table above, computed on the device; the
 * top-down scheme of TF Text's wordpiece_vocab learner — no bit parity with that package is claimed: the contract is the
 * one stated here, and tests/learn_model.py is its executable form) ----
 * Input.  A word table as wp_count_words[_device] gives it: words (a byte pool of n_bytes bytes), word_off int64
 * [n_words + 1], counts int64 [n_words], and spec->terminator, the byte behind every word in the pool (-1: none).  Any
 * table is taken: duplicate words add their counts up, a word of 0 bytes is skipped.  A check on the device answers
 * WP_ERR_ARG, naming the first word it concerns, where word_off descends or leaves the pool, a count is negative, or a
 * word is not valid UTF-8.  Lengths below are in code points.
 * Filters, in this order: (1) a word equal to a reserved token, and a word whose bytes begin with "##", is dropped;
 * (2) a word of more than max_token_chars is dropped; (3) with max_unique_chars = K > 0 the characters of the remaining
 * words are ranked by their occurrences weighted by the word counts, descending, ties by code point ascending: the first
 * K are allowed, and a word that holds any other character is dropped.  The characters of the call are those of the words
 * that remain.
 * Tokens.  A token is a pair (joined, text): the substring [s, e) of a word is the token (s > 0, those characters), and
 * two tokens are the same iff flag and bytes are equal.  The universe is every substring of every remaining word in the
 * order (word, s, e); a token's first occurrence is its first place in that order.
 * One threshold t runs num_iterations iterations.  In iteration 0 every start of every word is active; in iteration
 * k > 0 the active starts of a word are the piece starts of its greedy longest-match split over the tokens iteration
 * k - 1 ended with.  count[T] is the sum of the word counts over the occurrences of T whose start is active (int64).
 * Then for L = max_token_chars down to 1 every token of length L with count >= t is kept with that count as its score,
 * and its count is taken from each of its proper prefixes with the same flag (counts may go negative).  Behind the level
 * pass every character is added bare and joined, with score 1 where it was not kept.
 * The list: the reserved tokens in the order given (score 0), then for every character in code point order c, then ##c,
 * then the other kept tokens of the last iteration by score descending, ties by first occurrence; joined tokens are
 * written with "##".  Its length is the size.
 * Search.  lower = lower_thresh, upper = upper_thresh; a step takes t = (lower + upper) / 2 and is accepted if
 * size <= vocab_size and vocab_size - size <= slack (a number of entries), or lower >= upper, or t <= 1; otherwise
 * lower = t + 1 where size > vocab_size, else upper = t - 1.
 * Result.  tokens: the list as text, each token followed by '\n' (the content of a vocab.txt), n_bytes bytes; token_off
 * int64 [n_tokens + 1]; scores int64 [n_tokens]; thresh: the accepted threshold (0: no word remained, the list is the
 * reserved tokens alone).
 * Exactness.  Occurrences are grouped into tokens by a 64-bit hash of flag and bytes, and every member of a group is
 * compared with the group's first occurrence; what differs is grouped again under another seed (wp_learn_stats.n_rounds,
 * n_collided).  hash_bits (0: 64; else 8..64) narrows the hash for tests and never changes a result.  The sums are
 * integer sums: no result depends on an order of execution.
 * The handle lends its device context only: its vocabulary and its options are not read (WP_OPT_STAGE_TIMING and
 * WP_OPT_ARENA_GUARD excepted).  Host form: the table in host memory, the blocks of *out malloc'd, each freed with
 * wp_free; the empty table is answered without a device.  Device form: device arrays in (word_off, counts 8-byte
 * aligned), the arrays of *d_out device memory owned by the handle until its next learn call.
 * WP_ERR_ARG, before a device is touched and with the field named: spec or out NULL, words, word_off or counts NULL with
 * n_words > 0, vocab_size < 1, max_token_chars outside [1, 64], num_iterations < 1, lower_thresh or upper_thresh below
 * 1 or lower_thresh > upper_thresh, slack negative, max_unique_chars negative, terminator outside [-1, 255], hash_bits
 * not 0 and outside [8, 64], n_reserved negative or reserved_tokens / reserved_off NULL with n_reserved > 0, a reserved
 * token that is empty or holds '\n', reserved not 0.  WP_ERR_TOO_LARGE: a pool of more than UINT32_MAX bytes, 2^31
 * words, or 2^31 substring occurrences or more. */
typedef struct { const uint8_t *reserved_tokens; const int64_t *reserved_off; int64_t n_reserved, vocab_size, lower_thresh, upper_thresh, slack; int32_t num_iterations, max_token_chars, max_unique_chars, terminator, hash_bits, reserved; } wp_learn_spec;
typedef struct { uint8_t *tokens; int64_t *token_off, *scores; int64_t n_tokens, n_bytes, thresh; } wp_learned_vocab;
int wp_learn_vocab(wp_vocab *v, const uint8_t *words, const int64_t *word_off, const int64_t *counts, size_t n_words,
                   const wp_learn_spec *spec, wp_learned_vocab *out);
int wp_learn_vocab_device(wp_vocab *v, const void *d_words, size_t n_bytes, const int64_t *d_word_off, const int64_t *d_counts,
                          size_t n_words, const wp_learn_spec *spec, wp_learned_vocab *d_out);
/* The statistics of the last learn call, in a struct of its own.  n_words: the entries of the table; n_reserved, n_long,
 * n_char_dropped: the words filters 1, 2 and 3 dropped; n_chars: the characters; n_occurrences: the substring
 * occurrences; n_tokens: the distinct tokens among them; n_steps: the steps of the search; thresh: the accepted
 * threshold; n_rounds, n_collided: the grouping rounds and the occurrences round 0 left for later ones.  With
 * WP_OPT_STAGE_TIMING a learn call leaves its device times (HIP events) in the fields of wp_stats an encode times itself
 * in: ms_decode (table check, filters, characters, enumeration), ms_sa (the grouping: keys, sorts, comparison, parents,
 * the order by group), ms_scan (the search: every step's splits, sums and levels), ms_walk (order, list, gather),
 * ms_total (their sum). */
typedef struct { int64_t n_words, n_reserved, n_long, n_char_dropped, n_chars, n_occurrences, n_tokens, n_steps, thresh, n_rounds, n_collided; } wp_learn_stats;
int wp_get_learn_stats(const wp_vocab *v, wp_learn_stats *out);   /* n_words == -1: no such call yet, or an encode since */

/* ---- duplicate rows (an addition: the duplicate rows of a ragged batch dropped on the device, exactly; the contract is
 * the one stated here, and tests/dedup_model.py is its executable form) ----
 * Input.  data: a flat stream of elements of spec->elem_bytes bytes (1: text, 4: ids); row_off int64 [n_rows + 1],
 * ascending from row_off[0] == 0, in elements: row i is the elements [row_off[i], row_off[i + 1]), and n_elems =
 * row_off[n_rows].  These are the doc_off of the joined-documents form (the '\n' belongs to the row), the row_splits of
 * the rows calls, or the word_off of the count call.  A row may start at any byte.  No vocabulary is read: the handle
 * lends its device context, as it does to the learner (WP_OPT_STAGE_TIMING and WP_OPT_ARENA_GUARD are its only options
 * that matter).
 * Equality.  Two rows are the same iff they have the same number of elements and the same bytes; empty rows equal each
 * other.
 * Result, always: first int32 [n_rows], the smallest index of a row equal to row i (first[i] == i iff row i is kept);
 * kept int32 [n_unique], the kept rows ascending, i.e. in order of first occurrence; counts int64 [n_unique], how many
 * rows equal kept[k].  With WP_DEDUP_WANT_INVERSE: inverse int32 [n_rows] with first[i] == kept[inverse[i]] (numpy's
 * return_inverse).  With WP_DEDUP_WANT_COMPACT: data and row_off int64 [n_unique + 1], the kept rows back to back in
 * that order, n_elems elements — for text again a joined-documents text with its doc_off, for ids again ids and
 * row_splits.  (n_elems of the result is 0 without WP_DEDUP_WANT_COMPACT; wp_dedup_stats.n_elems is the input's.)
 * Exactness.  Rows are cut into chunks of 256 bytes; a row's key is the sum mod 2^64 of the seeded 64-bit hashes of its
 * chunks, each mixed with its index in the row, plus a mix of the length.  Rows are grouped by key (a stable sort, so a
 * group's head is its first row), every member is compared with the head chunk by chunk, and what differs is grouped
 * again under another seed (wp_dedup_stats.n_rounds, n_collided).  No part of the result depends on a hash, on a seed
 * or on an order of execution; hash_bits (0: 64; else 8..64) narrows the key for tests and never changes a result.  All
 * work on bytes is flat over the chunks: its cost follows n_elems, never the longest row.
 * WP_ERR_ARG, before a device is touched and with the field named: spec or out NULL, elem_bytes not 1 or 4, want with a
 * bit outside 3, hash_bits not 0 and outside [8, 64], reserved not 0, row_off NULL with n_rows > 0; data NULL with
 * n_elems > 0.  Offsets that do not start at 0 or descend give WP_ERR_ARG and name the first row i with
 * row_off[i + 1] < row_off[i] (row 0 also where row_off[0] != 0): the host form checks on the host, the device form by
 * a kernel.  (The host form has no length of data to check row_off[n_rows] against: that is the caller's.)
 * WP_ERR_TOO_LARGE: n_rows >= 2^31, or n_elems * elem_bytes > UINT32_MAX.
 * Host form: the blocks of *out are malloc'd, each freed with wp_free; a block is NULL where it is empty or was not asked
 * for.  n_rows == 0, and a batch whose rows are all empty, are answered without a device.  Device form: d_data under
 * the buffer contract of wp_linear_encode_device for text (4-byte aligned, readable to the next multiple of 16), 4-byte
 * aligned for ids; d_row_off 8-byte aligned; the arrays of *d_out are device memory owned by the handle until its next
 * call (n_rows == 0: all NULL).  Nothing behind n_elems * elem_bytes influences the result.
 * Waits of a call: one for the sizes (the offset check, n_elems, the chunks), one per round, one that ends the call and
 * brings the size of the compact form.  With WP_OPT_STAGE_TIMING a dedup call leaves its device times (HIP events) in
 * the fields of wp_stats a count call uses: ms_decode (offset check and chunk list), ms_sa (the rounds: keys, sort,
 * comparison), ms_walk (table, compact form), ms_total (their sum); ms_normalize is 0. */
#define WP_DEDUP_WANT_INVERSE 1
#define WP_DEDUP_WANT_COMPACT 2
typedef struct { int32_t elem_bytes, want, hash_bits, reserved; } wp_dedup_spec;
typedef struct { int32_t *first, *kept, *inverse; int64_t *counts, *row_off; void *data; int64_t n_rows, n_unique, n_elems; } wp_dedup_result;
int wp_dedup_rows(wp_vocab *v, const void *data, const int64_t *row_off, size_t n_rows, const wp_dedup_spec *spec, wp_dedup_result *out);
int wp_dedup_rows_device(wp_vocab *v, const void *d_data, const int64_t *d_row_off, size_t n_rows, const wp_dedup_spec *spec, wp_dedup_result *d_out);
/* The statistics of the last dedup call, in a struct of its own.  n_rows, n_unique, n_empty (rows of no element), n_elems
 * (of the input): these depend on no hash.  n_chunks: the chunks of the batch; n_compared: the elements of the chunks
 * that were compared with their head's; n_rounds, n_collided: the grouping rounds and the rows round 0 left for later
 * ones. */
typedef struct { int64_t n_rows, n_unique, n_empty, n_elems, n_chunks, n_compared, n_rounds, n_collided; } wp_dedup_stats;
int wp_get_dedup_stats(const wp_vocab *v, wp_dedup_stats *out);   /* n_rows == -1: no such call yet, or an encode since */

/* ---- near-duplicate rows (an addition: the rows of a ragged batch clustered by MinHash signatures over shingles and LSH
 * bands, on the device; every hash is a fixed integer function stated here, so the result is bit-exact against
 * tests/neardup_model.py, the contract's executable form) ----
 * Input.  As wp_dedup_rows: data, a flat stream of elements of spec->elem_bytes bytes (1: text, 4: ids), and row_off int64
 * [n_rows + 1], ascending from 0, in elements.  No vocabulary is read: the handle lends its device context
 * (WP_OPT_STAGE_TIMING and WP_OPT_ARENA_GUARD are its only options that matter).  Ids are the better view of text: the
 * shingles of the tokens of an uncased handle ignore case, accents and spacing.
 * Spec.  shingle = k in [1, 64] elements; n_perm in [1, 256]; bands >= 1 and a divisor of n_perm, r = n_perm / bands;
 * min_agree in [0, n_perm]; want: a bit set of WP_NEARDUP_WANT_*; seed: any; reserved: 0.
 * Functions.  M = the 64-bit finaliser (h ^= h >> 33; h *= 0xff51afd7ed558ccd; h ^= h >> 33; h *= 0xc4ceb9fe1a85ec53;
 * h ^= h >> 33), G = 0x9e3779b97f4a7c15, all arithmetic mod 2^64.
 *   Shingles of a row of L elements: none for L = 0; the whole row for 0 < L < k; else the L - k + 1 windows of k elements.
 *   Shingle hash over the B bytes of the shingle: h = M(M(seed ^ G) ^ (B | 1 << 41)); for every full little-endian 64-bit
 *   word x: h = M(h ^ x) + G; then with the rest zero-extended, or 0: h = M(h ^ x); x32 = (h ^ h >> 32) & 0xffffffff.
 *   Permutation j: a_j = M(seed + (2j + 1) G), b_j = M(seed + (2j + 2) G), P_j(x32) = (a_j x32 + b_j) >> 32
 *   (multiply-add-shift: strongly universal for a 32-bit x with 64-bit a and b).
 *   Signature: sig[i][j] = the minimum over row i's shingles of P_j, as uint32; 0xffffffff for a row without shingles.
 *   Band key of row i, band b: h = M(M(seed ^ G) ^ (b + (1 << 42))); for t < r: h = M(h ^ sig[i][b r + t]) + G.  The band
 *   index is in the key, so the keys of all bands share one sort.
 * Buckets.  A bucket is the set of (row, band) pairs with equal 64-bit band key; rows without shingles are in no
 * bucket; a bucket's head is its smallest row.  The contract defines buckets by the 64-bit key: a key collision joins
 * rows in the model exactly as on the device, and min_agree is what filters it.
 * Edges.  Every member of a bucket whose row is not the head is compared with the head only: agree = the number of j
 * with sig[m][j] == sig[head][j], and (m, head) is an edge iff agree >= min_agree (min_agree == 0: no signature is read).
 * Clusters.  cluster[i] = the smallest row index in the connected component of i in the edge graph.  Equal rows with
 * elements always share a cluster (equal signatures, equal keys).  Empty rows are each their own cluster — unlike
 * wp_dedup_rows, which joins them: there is no shingle to compare.
 * Result, always: cluster int32 [n_rows]; kept int32 [n_unique], the rows with cluster[i] == i, ascending; counts int64
 * [n_unique], the component sizes.  With WP_NEARDUP_WANT_INVERSE: inverse int32 [n_rows], cluster[i] ==
 * kept[inverse[i]].  With WP_NEARDUP_WANT_COMPACT: data and row_off int64 [n_unique + 1], the kept rows back to back,
 * n_elems elements, as in wp_dedup_rows.  With WP_NEARDUP_WANT_SIGNATURES: signatures uint32 [n_rows, n_perm],
 * row-major (n_perm of the result repeats the spec's).  Nothing depends on an order of execution: every combination
 * across lanes is an integer minimum or an integer sum.
 * WP_ERR_ARG, before a device is touched and with the field named: spec or out NULL, elem_bytes not 1 or 4, want with a
 * bit outside 7, shingle outside [1, 64], n_perm outside [1, 256], bands below 1 or no divisor of n_perm, min_agree
 * outside [0, n_perm], reserved not 0, row_off NULL with n_rows > 0; data NULL with n_elems > 0.  Offsets are checked as
 * wp_dedup_rows checks them, with the first bad row named: on the host in the host form, by a kernel in the device form.
 * WP_ERR_TOO_LARGE: n_rows >= 2^31, n_elems * elem_bytes > UINT32_MAX, n_rows * n_perm or n_rows * bands >= 2^32.
 * WP_ERR_INTERNAL: the component rounds did not end within n_rows + 1 rounds (every round that changes a label leaves at
 * least one root label fewer, so this cannot happen; the loop is capped all the same).
 * Host form: the blocks of *out are malloc'd, each freed with wp_free; a block is NULL where it is empty or was not asked
 * for.  n_rows == 0, and a batch whose rows are all empty, are answered without a device.  Device form: the buffer
 * contract of wp_dedup_rows_device; the arrays of *d_out are device memory owned by the handle until its next call
 * (n_rows == 0: all NULL).  Nothing behind n_elems * elem_bytes influences the result.
 * Cost.  All work on the data is flat over the shingle positions of the batch, n_shingles * n_perm multiply-add-min
 * steps: it follows n_elems, never the longest row.
 * Waits of a call: one for the sizes (the offset check, n_elems, the positions), one behind the grouping (the candidate
 * count), with min_agree > 0 one behind the comparison (the edge count), one per component round, one for the kept
 * count, one that ends the call.  With WP_OPT_STAGE_TIMING a call
 * leaves its device times (HIP events) in wp_stats: ms_decode (offset check and position list), ms_scan (signatures),
 * ms_sa (band keys, sort, heads, edges), ms_walk (components, table, compact form), ms_total (their sum). */
#define WP_ERR_INTERNAL 7
#define WP_NEARDUP_WANT_INVERSE    1
#define WP_NEARDUP_WANT_COMPACT    2
#define WP_NEARDUP_WANT_SIGNATURES 4
typedef struct { int32_t elem_bytes, want, shingle, n_perm, bands, min_agree; uint64_t seed; int32_t reserved[2]; } wp_neardup_spec;
typedef struct { int32_t *cluster, *kept, *inverse; int64_t *counts, *row_off; void *data; uint32_t *signatures; int64_t n_rows, n_unique, n_elems, n_perm; } wp_neardup_result;
int wp_neardup_rows(wp_vocab *v, const void *data, const int64_t *row_off, size_t n_rows, const wp_neardup_spec *spec, wp_neardup_result *out);
int wp_neardup_rows_device(wp_vocab *v, const void *d_data, const int64_t *d_row_off, size_t n_rows, const wp_neardup_spec *spec, wp_neardup_result *d_out);
/* The statistics of the last neardup call, in a struct of its own.  n_rows, n_unique, n_empty, n_elems (of the input),
 * n_shingles (the shingle positions), n_buckets (buckets of more than one member), n_candidates (members compared with
 * their head, one per (row, band) pair whose row is not the head), n_edges (the candidates that passed min_agree):
 * functions of the contract.  n_rounds: the component rounds, which depends on the scheme and is only reported. */
typedef struct { int64_t n_rows, n_unique, n_empty, n_elems, n_shingles, n_buckets, n_candidates, n_edges, n_rounds; } wp_neardup_stats;
int wp_get_neardup_stats(const wp_vocab *v, wp_neardup_stats *out);   /* n_rows == -1: no such call yet, or an encode since */

/* ---- n-gram overlap (an addition: the rows of a ragged batch that share an n-gram with a reference set, found on the
 * device, exactly — decontamination against evaluation data, a block list, licensed text; the contract is the one stated
 * here, and tests/overlap_model.py is its executable form) ----
 * Input.  Two batches as wp_dedup_rows takes one: the corpus, data and row_off int64 [n_rows + 1], and the reference
 * set, ref_data and ref_off int64 [n_ref + 1]; offsets ascending from 0, in elements of spec->elem_bytes bytes (1: text,
 * 4: ids), the same for both batches; a row may start at any byte.  No vocabulary is read: the handle lends its device
 * context (WP_OPT_STAGE_TIMING and WP_OPT_ARENA_GUARD are its only options that matter).  Ids are the better view of
 * text: the windows of the tokens of an uncased handle ignore case, accents and spacing.
 * Windows.  k = spec->ngram in [1, 64].  A row of L >= k elements has the L - k + 1 windows at the positions p = 0 ..
 * L - k; a row of L < k elements has none (unlike the shingles of wp_neardup_rows: a short row neither hits nor is hit).
 * A window never crosses a row boundary.
 * Hit.  Window p of corpus row i hits iff its k * elem_bytes bytes equal those of some window of some reference row.
 * Result, always: hits int64 [n_rows], the hitting windows of row i; first_hit int64 [n_rows], the smallest hitting p or
 * -1; first_ref int32 [n_rows], the smallest reference row that holds a window equal to the one at first_hit, or -1;
 * covered int64 [n_rows], the elements of row i that lie in at least one hitting window (the size of the union of the
 * [p, p + k)).  With WP_OVERLAP_WANT_MASK: mask uint8 [n_elems of the corpus], 1 where the element is covered — covered[i]
 * is its sum over row i, data[mask == 0] the corpus with the leaked spans cut out.  With WP_OVERLAP_WANT_REF: ref_hits
 * int64 [n_ref], the windows of reference row j that equal some corpus window (each window once, however often it is
 * met).  With WP_OVERLAP_WANT_COMPACT: kept int32 [n_kept], the rows with hits[i] <= spec->max_hits ascending (max_hits
 * >= 0; 0 keeps the clean rows), and those rows back to back as data and row_off int64 [n_kept + 1], n_elems elements,
 * as the compact forms of wp_dedup_rows and wp_neardup_rows; without the bit kept, data and row_off are NULL and n_kept,
 * n_elems are 0.
 * Exactness.  No part of any result array depends on a hash, a seed or an order of execution: every window that a key
 * lets through is compared byte by byte, and every combination across lanes is an integer sum, minimum or OR.
 * hash_bits (0: 64; else 8..64) narrows the window key to its low bits, for tests, and never changes a result; the
 * bucket index reads the top bits of the narrowed key.
 * WP_ERR_ARG, before a device is touched and with the field named: spec or out NULL, elem_bytes not 1 or 4, want with a
 * bit outside 7, ngram outside [1, 64], max_hits < 0, hash_bits not 0 and outside [8, 64], reserved not 0, row_off NULL
 * with n_rows > 0, ref_off NULL with n_ref > 0; data or ref_data NULL with elements.  Offsets that do not start at 0 or
 * descend give WP_ERR_ARG, naming the array (row_off or ref_off) and its first bad row: the host form checks on the
 * host, the device form by a kernel.
 * WP_ERR_TOO_LARGE: n_rows or n_ref >= 2^31, or either batch over UINT32_MAX bytes.
 * Host form: the blocks of *out are malloc'd, each freed with wp_free; a block is NULL where it is empty or was not asked
 * for.  n_rows == 0 returns all NULL; a corpus or a reference set without any window is answered without a device
 * (hits and covered 0, first_hit and first_ref -1, every row kept).  Device form: both batches under the buffer contract
 * of wp_dedup_rows_device; the arrays of *d_out are device memory owned by the handle until its next call (n_rows == 0:
 * all NULL).  Nothing behind n_elems * elem_bytes of either batch influences a result.
 * Cost.  All work is flat over the elements of the two batches, never over rows; a window key costs the same for every
 * k (a polynomial hash from two prefix values of a tile in LDS).
 * Waits of a call: one for the sizes of both batches (the offset checks, the elements, the windows), one for the
 * candidate count (it brings the table size too), with WP_OVERLAP_WANT_COMPACT one for the kept count, one that ends the
 * call: three or four by the spec, never by the data or by collisions.  With WP_OPT_STAGE_TIMING a call leaves its
 * device times (HIP events) in wp_stats: ms_decode (the offset checks), ms_sa (the reference table: keys, sort,
 * distinct windows, bucket index), ms_scan (the corpus windows, lookup and comparison), ms_walk (the per-row results and
 * the compact form), ms_total (their sum); ms_normalize is 0. */
#define WP_OVERLAP_WANT_MASK    1
#define WP_OVERLAP_WANT_REF     2
#define WP_OVERLAP_WANT_COMPACT 4
typedef struct { int32_t elem_bytes, want, ngram, max_hits, hash_bits, reserved[3]; } wp_overlap_spec;
typedef struct { int64_t *hits, *first_hit, *covered, *ref_hits, *row_off; int32_t *first_ref, *kept; uint8_t *mask; void *data; int64_t n_rows, n_ref, n_kept, n_elems; } wp_overlap_result;
int wp_overlap_rows(wp_vocab *v, const void *data, const int64_t *row_off, size_t n_rows, const void *ref_data, const int64_t *ref_off, size_t n_ref, const wp_overlap_spec *spec, wp_overlap_result *out);
int wp_overlap_rows_device(wp_vocab *v, const void *d_data, const int64_t *d_row_off, size_t n_rows, const void *d_ref_data, const int64_t *d_ref_off, size_t n_ref, const wp_overlap_spec *spec, wp_overlap_result *d_out);
/* The statistics of the last overlap call, in a struct of its own.  n_rows, n_ref, n_elems, n_ref_elems, n_windows,
 * n_ref_windows, n_ref_distinct (the distinct reference windows), n_hits (the sum of hits), n_hit_rows (the rows with a
 * hit), n_covered (the sum of covered): functions of the contract.  n_candidates (the corpus windows whose key was in the
 * table) and n_collided (the reference windows that differ from the first window of their key) depend on the hash and
 * are only reported. */
typedef struct { int64_t n_rows, n_ref, n_elems, n_ref_elems, n_windows, n_ref_windows, n_ref_distinct, n_hits, n_hit_rows, n_covered, n_candidates, n_collided; } wp_overlap_stats;
int wp_get_overlap_stats(const wp_vocab *v, wp_overlap_stats *out);   /* n_rows == -1: no such call yet, or an encode since */

/* ---- repeated spans (an addition: the windows of a ragged batch that already occurred earlier in the same batch, found
 * on the device, exactly, and cut out there — the exact-substring step of a corpus pipeline: licence headers, navigation
 * bars, templated paragraphs inside rows that are otherwise different; the contract is the one stated here, and
 * tests/repeat_model.py is its executable form) ----
 * Input.  One batch as wp_dedup_rows takes it: data, a flat stream of elements of spec->elem_bytes bytes (1: text, 4:
 * ids), and row_off int64 [n_rows + 1], ascending from 0, in elements; a row may start at any byte.  No vocabulary is
 * read: the handle lends its device context (WP_OPT_STAGE_TIMING and WP_OPT_ARENA_GUARD are its only options that matter).
 * Windows.  As in wp_overlap_rows: k = spec->ngram in [1, 64]; a row of L >= k elements has the windows at p = 0 .. L - k,
 * a shorter row has none; no window crosses a row boundary.  The flat position of (row i, p) is row_off[i] + p.
 * Repeat.  The first occurrence of a window is the smallest flat position that holds an equal window (the same
 * k * elem_bytes bytes); it may lie in the same row and it may overlap the window itself.  spec->scope 0 (anywhere): a
 * window is a repeat iff its first occurrence is not itself.  scope 1 (earlier rows only): iff its first occurrence lies
 * in a row of smaller index — what a row repeats of itself stays; the smallest occurrence lies in the smallest row, so
 * the same grouping answers both.
 * Covered.  An element is covered iff it lies in [p, p + k) of some repeat window of its row: the union, so a stretch may
 * be covered piecewise from several sources.  A first occurrence is never a repeat, but its elements may be covered by
 * other repeat windows: with k = 2, "aaaa" keeps "a".
 * spec->flags: WP_REPEAT_UTF8 (elem_bytes 1 only, WP_ERR_ARG otherwise): position p is a window only if byte p is no
 * continuation byte (10xxxxxx) and byte p + k is past the row end or no continuation byte.  The other positions are
 * windows neither as repeats nor as sources, so a cut never splits a sequence: valid UTF-8 stays valid.  The rule reads
 * bytes only and is defined for invalid text too.
 * Result, always, per row: repeats int64 [n_rows], the repeat windows of row i; first_repeat int64, the smallest
 * repeating p or -1; first_src_row int32, the row of the first occurrence of the window at first_repeat, or -1;
 * first_src_pos int64, the position of that first occurrence in its row, or -1; covered int64.  With
 * WP_REPEAT_WANT_MASK: mask uint8 [n_elems], 1 where the element is covered.  With WP_REPEAT_WANT_SRC: src int64
 * [n_elems], the flat position of the first occurrence where the window at that element is a repeat, else -1.  With
 * WP_REPEAT_WANT_COMPACT: kept int32 [n_kept], the rows with repeats[i] <= spec->max_repeats ascending, and those rows
 * whole and back to back as data and row_off int64 [n_kept + 1], n_elems elements, as the compact form of
 * wp_overlap_rows.  With WP_REPEAT_WANT_CUT: cut_data and cut_off int64 [n_rows + 1], every row with its covered
 * elements removed (data[mask == 0]) and its index unchanged — a row may become empty — and n_cut_elems, their number.
 * Both forms may be asked for in one call.  Without a bit its arrays are NULL and its counts 0.
 * Exactness.  No result array depends on a hash, a seed or an order of execution: every window a key groups is compared
 * byte by byte, every position is written by one lane, and every combination across lanes is an integer sum.
 * hash_bits (0: 64; else 8..64) narrows the window key to its low bits, for tests, and never changes a result.  The
 * default is the full 64 bits whatever the window count: no narrower default was measured, so none is claimed.
 * WP_ERR_ARG, before a device is touched and with the field named: spec or out NULL, elem_bytes not 1 or 4, want with a
 * bit outside 15, ngram outside [1, 64], scope outside {0, 1}, max_repeats < 0, hash_bits not 0 and outside [8, 64],
 * flags other than WP_REPEAT_UTF8 (and that one with elem_bytes 4), reserved not 0, row_off NULL with n_rows > 0; data
 * NULL with elements.  Offsets that do not start at 0 or descend give WP_ERR_ARG with the first bad row: the host form
 * checks on the host, the device form by a kernel, before anything reads through them.
 * WP_ERR_TOO_LARGE: n_rows >= 2^31, or the batch over UINT32_MAX bytes.
 * Host form: the blocks of *out are malloc'd, each freed with wp_free; a block is NULL where it is empty or was not asked
 * for.  n_rows == 0 returns all NULL; a batch without any window is answered without a device (repeats and covered 0,
 * the firsts -1, every row kept, the cut equal to the input).  Device form: the buffer contract of wp_dedup_rows_device;
 * the arrays of *d_out are device memory owned by the handle until its next call (n_rows == 0: all NULL).  Nothing
 * behind n_elems * elem_bytes influences a result.
 * Cost.  All work is flat over the elements or the windows of the batch, never over rows: one row of 10^8 elements costs
 * what 10^6 rows of 100 do.
 * Waits of a call, set by the spec alone: one for the sizes (the offset check, the elements, the windows), with
 * WP_REPEAT_UTF8 one for the number of eligible windows (without the flag every window is listed and the first wait
 * brought their number), with WP_REPEAT_WANT_COMPACT one for the kept count, one that ends the call.  The cut is bounded
 * by the input and needs none.  With WP_OPT_STAGE_TIMING a call leaves its device times (HIP events) in wp_stats:
 * ms_decode (the offset check), ms_sa (keys, sort, distinct windows, first occurrences), ms_scan (the repeat flags, their
 * scan, the cover pass), ms_walk (the per-row results, the cut, the compact form), ms_total (their sum); ms_normalize is 0. */
#define WP_REPEAT_WANT_MASK    1
#define WP_REPEAT_WANT_SRC     2
#define WP_REPEAT_WANT_COMPACT 4
#define WP_REPEAT_WANT_CUT     8
#define WP_REPEAT_UTF8         1
typedef struct { int32_t elem_bytes, want, ngram, scope, max_repeats, hash_bits, flags, reserved; } wp_repeat_spec;
typedef struct { int64_t *repeats, *first_repeat, *first_src_pos, *covered, *src, *row_off, *cut_off; int32_t *first_src_row, *kept; uint8_t *mask; void *data, *cut_data; int64_t n_rows, n_kept, n_elems, n_cut_elems; } wp_repeat_result;
int wp_repeat_rows(wp_vocab *v, const void *data, const int64_t *row_off, size_t n_rows, const wp_repeat_spec *spec, wp_repeat_result *out);
int wp_repeat_rows_device(wp_vocab *v, const void *d_data, const int64_t *d_row_off, size_t n_rows, const wp_repeat_spec *spec, wp_repeat_result *d_out);
/* The statistics of the last repeat call, in a struct of its own.  n_rows, n_elems, n_windows (with WP_REPEAT_UTF8: the
 * eligible ones), n_distinct (the distinct windows), n_repeats (the sum of repeats; at scope 0 n_windows - n_distinct),
 * n_repeat_rows (the rows with a repeat), n_covered (the sum of covered), n_cut_elems (with WP_REPEAT_WANT_CUT n_elems -
 * n_covered, else 0): functions of the contract.  n_collided (the windows that differ from the first window of their
 * key) depends on the hash and is only reported. */
typedef struct { int64_t n_rows, n_elems, n_windows, n_distinct, n_repeats, n_repeat_rows, n_covered, n_cut_elems, n_collided; } wp_repeat_stats;
int wp_get_repeat_stats(const wp_vocab *v, wp_repeat_stats *out);   /* n_rows == -1: no such call yet, or an encode since */

/* ---- quality signals (an addition: per document of a ragged batch of text a fixed set of exact integer signals, a list
 * of threshold rules over them, and the passing documents in compact form: the heuristic filters that Gopher, C4 and
 * FineWeb put in front of deduplication.  This section is the contract; tests/quality_model.py is its executable form) ----
 * wp_quality_rows[_device](v, data, row_off, n_rows, spec, out).  data: text bytes (elem_bytes 1 only); row_off int64
 * [n_rows + 1], ascending from 0, as wp_dedup_rows takes it; a row may start at any byte.  No vocabulary is read and no
 * normalisation applied (case is a signal); the handle lends its context.  Every signal of row i is a function of that
 * row's bytes alone.
 * Characters.  A row is decoded on its own by the decoder's rule: a lead byte starts a character iff the bytes its length
 * calls for lie inside the row and form a valid sequence; every byte no such sequence covers is an invalid byte, a
 * character of its own without a class (no space, no spacing character, not alphabetic).  The rule is local: within 3
 * bytes either way.
 * Classes.  Space, punctuation and CJK as everywhere in this library (the spacing characters are their union).  alpha is
 * general category L*, digit Nd, upper Lu, from a table generated by tools/gen_class_tables.py from Python's unicodedata
 * (csrc/class_tables.h, WP_CLASS_UNICODE_VERSION).
 * Words.  The rule of the word counts, per row: character p starts a word iff it is no space and (it is the row's first
 * character, or it or the character in front of it is a spacing character); a word ends in front of the next space or
 * word start, or with the row.  A punctuation character is therefore a word of its own.
 * Lines.  A line is a maximal run of bytes other than 0x0A inside a row, so none is empty.  Its first and last character
 * are its first and last non-space characters; a line of spaces only has neither.
 * Signals.  signals int64 [WP_QUALITY_SIGNALS][n_rows], signal-major, indices WP_QS_*: BYTES; CHARS (an invalid byte is
 * one); INVALID; SPACE_CHARS, ALPHA_CHARS, DIGIT_CHARS, UPPER_CHARS, PUNCT_CHARS; WORDS; TEXT_WORDS (words whose first
 * character is no punctuation) and TEXT_WORD_CHARS (their characters); ALPHA_WORDS (words that hold an alpha character);
 * STOP_WORDS (words equal to a listed stop word, ASCII A-Z of the text folded to lower case, nothing else folded, compared
 * byte for byte); HASHES ('#' bytes); ELLIPSES (U+2026 characters, plus maximal runs of three or more '.' inside the row,
 * each run once); NEWLINES (0x0A bytes); LINES; BULLET_LINES (first character '-' or U+2022); ELLIPSIS_LINES (last
 * character U+2026, or '.' with ".." directly in front of it inside the line); TERMINAL_LINES (last character one of
 * . ! ? " '); SHORT_LINES (at most short_line_chars characters, 0: 30; the line feed does not count); DUP_LINES (lines whose
 * bytes equal an earlier line of the same row; the line feed is no part of the comparison, so a last line without one
 * can duplicate an earlier line that has one) and DUP_LINE_CHARS (their characters).  The last two are 0 without
 * WP_QUALITY_WANT_DUP_LINES.
 * Stop words: n_stop_words words, word t the bytes stop_pool[stop_off[t] .. stop_off[t + 1]) in host memory; at most 64,
 * each 1 to 32 bytes without ASCII upper case; none is allowed.
 * Rules.  limit int64 [WP_QUALITY_RULES], each -1 (off) or in [0, 10^9], indices WP_QR_*.  A row fails rule r by its
 * integer inequality and nothing else (zero denominators need no case: both sides are 0 and the rule passes; every
 * product fits 64 bits): MIN_TEXT_WORDS: TEXT_WORDS < L; MAX_TEXT_WORDS: TEXT_WORDS > L; MIN_MEAN_WORD_X1000:
 * TEXT_WORD_CHARS * 1000 < L * TEXT_WORDS; MAX_MEAN_WORD_X1000: the same with >; MAX_HASH_PER_WORD: HASHES * 1000 > L *
 * WORDS; MAX_ELLIPSIS_PER_WORD: ELLIPSES * 1000 > L * WORDS; MAX_BULLET_LINES: BULLET_LINES * 1000 > L * LINES;
 * MAX_ELLIPSIS_LINES: ELLIPSIS_LINES * 1000 > L * LINES; MIN_ALPHA_WORDS: ALPHA_WORDS * 1000 < L * WORDS; MIN_STOP_WORDS:
 * STOP_WORDS < L; MAX_DUP_LINES: DUP_LINES * 1000 > L * LINES; MAX_DUP_LINE_CHARS: DUP_LINE_CHARS * 1000 > L * CHARS;
 * MIN_TERMINAL_LINES: TERMINAL_LINES * 1000 < L * LINES; MAX_SHORT_LINES: SHORT_LINES * 1000 > L * LINES;
 * MAX_NEWLINES_PER_WORD: NEWLINES * 1000 > L * WORDS; rule 15 is reserved and must be -1.  The two duplicate-line rules
 * need WP_QUALITY_WANT_DUP_LINES.  The published thresholds of Gopher and FineWeb can be stated in these rules (the Python
 * wrapper has them as presets), over THIS contract's words and lines: parity with another tokeniser's word count, such
 * as DataTrove's, is not claimed.
 * Results.  reasons uint32 [n_rows], bit r set where rule r failed; a row is kept iff its reasons are 0.  With
 * WP_QUALITY_WANT_COMPACT: kept int32 [n_kept] ascending, and the kept rows whole and back to back as data and row_off
 * int64 [n_kept + 1], n_elems bytes, as the compact form of wp_overlap_rows.
 * Exactness.  No result depends on a hash, a seed or an order of execution: every combination across lanes is an integer
 * sum (per-tile partial sums met by integer atomics), and the duplicate lines come from the exact duplicate-row search.
 * WP_ERR_ARG, before a device is touched and with the field named: spec or out NULL, elem_bytes not 1, want with a bit
 * outside 3, short_line_chars negative, a limit outside {-1} and [0, 10^9], limit[15] not -1, limit[10] or limit[11] on
 * without WP_QUALITY_WANT_DUP_LINES, a bad stop list (n_stop_words outside [0, 64], stop_pool or stop_off NULL with words,
 * stop_off not ascending from 0, a word of 0 or more than 32 bytes or with ASCII upper case), reserved not 0, row_off NULL
 * with n_rows > 0; data NULL with bytes.  Offsets that do not start at 0 or descend give WP_ERR_ARG with the first bad
 * row: the host form checks on the host, the device form by a kernel, before anything reads through them.
 * WP_ERR_TOO_LARGE: n_rows >= 2^31, the batch over UINT32_MAX bytes, or 2^30 lines or more with
 * WP_QUALITY_WANT_DUP_LINES.
 * Host form: the blocks of *out are malloc'd, each freed with wp_free.  n_rows == 0 returns all NULL; a batch of 0 bytes
 * is answered on the host (signals 0, reasons the rules over zeros).  Device form: the buffer contract of
 * wp_dedup_rows_device; the arrays of *d_out are device memory owned by the handle until its next call (the next dedup
 * call included: the duplicate-line stage uses its buffers); nothing behind the data influences a result.
 * Cost.  All work is flat over bytes, words or lines, never over rows.
 * Waits of a call, set by the spec alone: one for the sizes (the offset check, the bytes), one for the numbers of words
 * and lines; with WP_QUALITY_WANT_DUP_LINES, where there is a line, those of the duplicate-row search over the lines (its
 * sizes, one per round — one unless 64-bit keys collide — and its end); with WP_QUALITY_WANT_COMPACT one for the kept
 * count; one that ends the call.  With WP_OPT_STAGE_TIMING a call leaves its device times in wp_stats: ms_decode (the
 * offset check), ms_sa (both class passes, the word pass, the line pass), ms_scan (the duplicate-line stage), ms_walk (the
 * rules, the compact form), ms_total (their sum); ms_normalize is 0.  A quality call leaves the statistics of every
 * other layer as they were, those of wp_get_dedup_stats included. */
#define WP_QUALITY_SIGNALS 23
#define WP_QUALITY_RULES   16
#define WP_QUALITY_WANT_DUP_LINES 1
#define WP_QUALITY_WANT_COMPACT   2
enum { WP_QS_BYTES = 0, WP_QS_CHARS, WP_QS_INVALID, WP_QS_SPACE_CHARS, WP_QS_ALPHA_CHARS, WP_QS_DIGIT_CHARS, WP_QS_UPPER_CHARS, WP_QS_PUNCT_CHARS,
       WP_QS_WORDS, WP_QS_TEXT_WORDS, WP_QS_TEXT_WORD_CHARS, WP_QS_ALPHA_WORDS, WP_QS_STOP_WORDS, WP_QS_HASHES, WP_QS_ELLIPSES, WP_QS_NEWLINES,
       WP_QS_LINES, WP_QS_BULLET_LINES, WP_QS_ELLIPSIS_LINES, WP_QS_TERMINAL_LINES, WP_QS_SHORT_LINES, WP_QS_DUP_LINES, WP_QS_DUP_LINE_CHARS };
enum { WP_QR_MIN_TEXT_WORDS = 0, WP_QR_MAX_TEXT_WORDS, WP_QR_MIN_MEAN_WORD_X1000, WP_QR_MAX_MEAN_WORD_X1000, WP_QR_MAX_HASH_PER_WORD,
       WP_QR_MAX_ELLIPSIS_PER_WORD, WP_QR_MAX_BULLET_LINES, WP_QR_MAX_ELLIPSIS_LINES, WP_QR_MIN_ALPHA_WORDS, WP_QR_MIN_STOP_WORDS,
       WP_QR_MAX_DUP_LINES, WP_QR_MAX_DUP_LINE_CHARS, WP_QR_MIN_TERMINAL_LINES, WP_QR_MAX_SHORT_LINES, WP_QR_MAX_NEWLINES_PER_WORD, WP_QR_RESERVED };
typedef struct { int32_t elem_bytes, want, short_line_chars, n_stop_words; const void *stop_pool; const int64_t *stop_off; int64_t limit[WP_QUALITY_RULES]; int64_t reserved; } wp_quality_spec;
typedef struct { int64_t *signals, *row_off; uint32_t *reasons; int32_t *kept; void *data; int64_t n_rows, n_kept, n_elems; } wp_quality_result;
int wp_quality_rows(wp_vocab *v, const void *data, const int64_t *row_off, size_t n_rows, const wp_quality_spec *spec, wp_quality_result *out);
int wp_quality_rows_device(wp_vocab *v, const void *d_data, const int64_t *d_row_off, size_t n_rows, const wp_quality_spec *spec, wp_quality_result *d_out);
/* The statistics of the last quality call, in a struct of its own: the rows, the sums of BYTES, CHARS, INVALID, WORDS,
 * LINES and DUP_LINES over them, the kept rows, and rule_failed[r], the rows rule r failed: what a pipeline report prints. */
typedef struct { int64_t n_rows, n_bytes, n_chars, n_invalid, n_words, n_lines, n_dup_lines, n_kept, rule_failed[WP_QUALITY_RULES]; } wp_quality_stats;
int wp_get_quality_stats(const wp_vocab *v, wp_quality_stats *out);   /* n_rows == -1: no such call yet, or an encode since */
/* the class bits of tools/gen_class_tables.py for a code point (1 alpha, 2 digit, 4 upper; -1: no code point): the table the
 * kernels read, for its test */
int32_t wp_quality_class(uint32_t cp);

/* The same call sharded over several GPUs of the node, behind the boundary: the reference's own
 * precedent is the in-library chunking at whitespace of linear.cpp:283-299 (thread chunks) and
 * linear.cpp:355-367 (encodeExternal batches).  The text is cut at ASCII whitespace into one shard
 * per entry of `devices` (HIP ordinals; an ordinal may repeat), balanced by code points; every
 * shard is encoded on its device by its own host thread against the replicated vocabulary, and the
 * ids are downloaded in shard order into one host buffer (free with wp_free).
 * devices == NULL: the first n_devices visible GPUs (n_devices <= 0: all of them).
 * A vocabulary that holds whitespace inside a token can match across a cut (the reference's chunking
 * shares the caveat): such inputs are encoded in one piece on the first device of the list. */
int wp_linear_encode_multi(wp_vocab *v, const char *utf8, size_t nbytes, const int *devices,
                           int n_devices, int32_t **ids, size_t *n_ids);

/* A sequence of texts (shards / batches of one corpus) through one handle, pipelined: the upload of text i + 1 and
 * the download of the ids of text i - 1 run on copy streams beside the kernels of text i (second text buffer, id
 * staging buffers), so that host to host costs what the device path costs.  Same ids per text as n_texts calls of
 * wp_linear_encode — the reference's precedent for feeding a corpus piecewise is encodeExternal's batch loop,
 * linear.cpp:355-371.  ids[i] (free each with wp_free; NULL for a text without ids) and n_ids[i] per text. */
int wp_linear_encode_batch(wp_vocab *v, const char *const *texts, const size_t *nbytes, size_t n_texts,
                           int32_t **ids, size_t *n_ids);

/* The same pipeline for a corpus of any length, with constant memory: `next` supplies text i (return 0: no more; the
 * pointer must stay valid until the following call of `next`), `out` receives the ids of text i — in order, one text
 * behind the encodes, valid during the call only (two pinned blocks take turns).  This is the sustained form of the
 * host-to-host metric: uploads, kernels and downloads of neighbouring texts overlap. */
typedef int (*wp_text_source)(void *user, size_t index, const char **utf8, size_t *nbytes);
typedef void (*wp_ids_sink)(void *user, size_t index, const int32_t *ids, size_t n_ids);
int wp_linear_encode_stream(wp_vocab *v, wp_text_source next, wp_ids_sink out, void *user);

/* Sizes the handle's device arenas and host staging for inputs of up to `nbytes`, so that the
 * first encode does not pay for the allocations (about 100 bytes of HBM per input symbol). */
int wp_reserve(wp_vocab *v, size_t nbytes);

/* Memory the library keeps between calls, and how to get it back.  A handle keeps its device arenas (about
 * 100 bytes of HBM per input symbol of its largest encode) until it is destroyed.  A destroyed handle's
 * context (streams, events, code tables) is parked in a process-wide pool of at most 4 for the next handle on
 * the same device — the reference's API is one-shot, linear.cpp:332-335, and sets everything up per call —
 * but only with arenas of up to 256 MB in total: larger ones are released at wp_vocab_destroy.  Returned id
 * blocks are page-locked host memory; wp_free keeps up to 4 of them (6 GB) for reuse.
 * wp_trim releases all of that: the arenas of `v`'s contexts (v may be NULL), the parked contexts' arenas and
 * the pooled id blocks.  (Env WP_NO_CONTEXT_POOL=1 switches the context pool off.) */
int wp_trim(wp_vocab *v);

/* replaces word_piece::linear::encode(text_file, vocab_file)   word_piece.hpp:14, linear.cpp:337-341 */
int wp_linear_encode_file(const char *text_file, const char *vocab_file, int32_t **ids,
                          size_t *n_ids);
/* replaces word_piece::linear::encodeExternal(...)              word_piece.hpp:16-19, linear.cpp:343-374
 * batches of memory_limit/20 bytes extended to the next space; ids appended to
 * out_file as decimal text, each followed by one ' ' (utils.cpp:30-35). */
int wp_linear_encode_external(const char *text_file, const char *vocab_file, const char *out_file,
                              size_t memory_limit);

/* ---- the sibling algorithm: word_piece::fast (src/word_piece.hpp:23-36, src/fast.cpp) ----
 * Per word, longest-match-first against the vocabulary (fast.cpp:19-150) — on the GPU a trie walk per
 * word (csrc/fast.h).  Same ids as the Linear path on vocabularies whose tokens do not span spacing
 * chars (tests/tests.cpp:80-97 asserts linear == fast); an independent on-device cross-check.
 * replaces word_piece::fast::encode(text, vocab)              word_piece.hpp:25, fast.cpp:161-164 */
int wp_fast_encode(wp_vocab *v, const char *utf8, size_t nbytes, int32_t **ids, size_t *n_ids);
/* text and ids in device memory, same buffer contract as wp_linear_encode_device */
int wp_fast_encode_device(wp_vocab *v, const void *d_utf8, size_t nbytes, const int32_t **d_ids,
                          size_t *n_ids);
/* replaces word_piece::fast::encode(text_file, vocab_file)   word_piece.hpp:27, fast.cpp:166-170 */
int wp_fast_encode_file(const char *text_file, const char *vocab_file, int32_t **ids, size_t *n_ids);
/* replaces word_piece::fast::encodeExternal(...)              word_piece.hpp:31-34, fast.cpp:189-220
 * batches of memory_limit/2 bytes extended to the next space; same id text format. */
int wp_fast_encode_external(const char *text_file, const char *vocab_file, const char *out_file,
                            size_t memory_limit);
/* UTF-8 of the stored word of vocab line i (the "##" of continuation tokens stripped, utils.cpp:83-85):
 * what word_piece::fast::decode (fast.cpp:172-187) assembles its strings from.  Returns the length in
 * bytes (-1: no such line) and copies at most `cap` bytes into buf. */
int64_t wp_vocab_token_utf8(const wp_vocab *v, int64_t i, char *buf, size_t cap);

/* ---- options ---- */
#define WP_OPT_FULL_DEPTH 1   /* 1: sort suffixes to full depth (true suffix array).  0 (default):
                                 stop prefix doubling once the sorted depth exceeds the longest
                                 vocab token — token ids are identical for duplicate-free vocabs;
                                 vocabs with duplicate lines force full depth automatically. */
#define WP_OPT_DEVICE 2       /* HIP device ordinal used by this handle (default: current) */
#define WP_OPT_KEEP_DEBUG 3   /* 1: keep SA/rank/LCP/best arrays for wp_linear_debug_fetch (full rank table: the
                                 key-space step lookup is off).  2: keep the step views by text position only
                                 (wp_linear_debug_fetch 8..11): layout, key-space lookup, keys-only round 0 and the
                                 early refinement stay as without the option; one more kernel in front of the walk. */
#define WP_OPT_STAGE_TIMING 4 /* 1: record per-stage device times with HIP events */
#define WP_OPT_LCP_KASAI 5    /* 1: build LCP with the chunked Kasai kernel (linear.cpp:18-70)
                                 instead of deriving it inside the doubling rounds */
/* (option 6, a single-pass form of the group split, was measured slower and removed) */
#define WP_OPT_COVER_ANCHORS 7 /* 1: always derive the walk's start positions from the matches
                                 (default: only when the class rule leaves gaps > 2048 positions
                                 and some spacing char occurs inside a multi-char token, e.g. CJK
                                 text with multi-char CJK tokens; long words of ordinary
                                 vocabularies are walked by pointer doubling instead) */
#define WP_OPT_ARENA_GUARD 8  /* 1: debugging aid — every device arena allocation is followed by a
                                 guard zone that is checked after the encode; a kernel that wrote
                                 outside its buffer makes the call fail with WP_ERR_HIP
                                 (env WP_ARENA_GUARD=1 switches it on for every handle) */
#define WP_OPT_DEVICES 9      /* number of GPUs wp_linear_encode (and with it word_piece::linear::encode)
                                 shards a host buffer over, as wp_linear_encode_multi does:
                                 1 (default) = the handle's device only, -1 = all visible GPUs.
                                 Env WP_DEVICES=<count>|all sets the default for new handles. */
#define WP_OPT_VOCAB_IN_S 10  /* 1: always build S = text . 1 . vocab as linear.cpp:77-101 does.  Default 0:
                                 the vocabulary stays out of the suffix sort (S = text . 1) and enters
                                 through the handle's sorted token list and the tokens' code streams;
                                 the reference's layout is still used for the true suffix array (full
                                 depth, duplicate lines) and when text or tokens hold U+0000 / U+0001.
                                 Same token ids either way. */
#define WP_OPT_SPARSE_EMIT 11 /* 1: the walk writes each id into a per-position array that is compacted
                                 afterwards, always.  Default 0: that path is taken only when several
                                 kernels contribute ids (words longer than a lane walks);
                                 otherwise every workgroup of the walk leaves one compact id list.
                                 Same token ids either way (also env WP_SPARSE_EMIT=1). */
#define WP_OPT_INDEXED_ROUND0 12 /* 1: round 0 of the suffix sort moves (key, index) records in the default
                                 layout too.  Default 0: there it sorts the keys alone and takes the
                                 positions it needs from a candidate list the key builder leaves (the
                                 suffixes whose key is the key of a long token).  Same token ids. */
#define WP_OPT_SORT_BLANKS 13 /* 1: that keys-only round 0 sorts every suffix.  Default 0: in texts where
                                 blanks (is_space) are common it leaves out the suffixes that start at one,
                                 which the walk never looks up (wp_stats.round0_sorted).  Same token ids. */
#define WP_OPT_NORMALIZE 14   /* WP_NORM_* flags (default 0: none): every encode of the handle first normalises its
                                 text on the device — what BERT's BasicTokenizer does in front of WordPiece, apart from
                                 the punctuation and CJK splitting that the walk's character classes already do.  The
                                 rule is defined per code point, in the order clean, lower, strip:
                                   WP_NORM_CLEAN          drop U+0000, U+FFFD and every Cc / Cf code point except U+0009,
                                                          U+000A, U+000D (kept as they are); every Zs becomes U+0020
                                   WP_NORM_LOWER          Python's chr(c).lower() of the single code point
                                   WP_NORM_STRIP_ACCENTS  canonical decomposition (NFD) of what is left, then drop Mn;
                                                          Hangul syllables become their 2-3 jamo, as in BERT
                                 WP_NORM_BERT_UNCASED is do_lower_case=True; WP_NORM_CLEAN alone is what cased BERT does.
                                 A code point gives at most 3 code points and at most 3x its UTF-8 bytes.  Two known
                                 differences from a whole-string implementation: U+03A3 always becomes U+03C3 (no final
                                 sigma), and neighbouring combining marks are not reordered by class (visible only
                                 between the 23 combining marks that are not Mn).  The vocabulary is NOT normalised: its
                                 lines are matched as given (an uncased vocabulary is lower case already).  Ids are those
                                 of the normalised text; offsets refer to the text the caller passed (see "token
                                 offsets"); documents calls keep their contract.  A value with unknown bits fails with
                                 WP_ERR_ARG.  The pre-pass sizes its buffer from a count it waits for: one more host
                                 wait per encode, in front of the decoder's own (the pipelined calls overlap a little less
                                 with the option on).  The tables follow the Unicode version of the generator's Python
                                 (csrc/normalize_tables.h). */
#define WP_NORM_CLEAN 1
#define WP_NORM_LOWER 2
#define WP_NORM_STRIP_ACCENTS 4
#define WP_NORM_BERT_UNCASED 7
#define WP_OPT_LATE_REFINE 15 /* 1: the keys-only round 0 starts the refinement of the needed groups behind its last
                                 pass, as it did before the early start.  Default 0: the groups are taken from the runs
                                 of the sorted candidate list and refined on a side stream beside the remaining passes;
                                 only the searches in the sorted keys and the rank scatter wait for the sort
                                 (wp_refine_sched).  Same token ids, same wp_refine_stats; for same-build A/B runs. */
int wp_set_option(wp_vocab *v, int option, int64_t value);

/* ---- the normalisation stage on its own (WP_OPT_NORMALIZE's pre-pass; `flags` as there, 0 copies the valid UTF-8) ----
 * The rule for one code point, on the host, from the tables the kernels read: the number of code points (0..3) it
 * gives, in out[].  Surrogates, values >= 0x110000 and unknown flag bits: -1.  Needs no device. */
int wp_normalize_cp(int flags, uint32_t cp, uint32_t out[3]);
/* The normalised text of a device buffer (buffer contract of wp_linear_encode_device), on the handle's device: *d_out
 * is owned by the handle and valid until its next call; invalid sequences are dropped.  nbytes == 0 gives 0 bytes. */
int wp_normalize_device(wp_vocab *v, const void *d_utf8, size_t nbytes, int flags, const void **d_out, size_t *out_bytes);
/* host text in, a malloc'd block out (free with wp_free; NULL when it is empty); empty text needs no device */
int wp_normalize(wp_vocab *v, const char *utf8, size_t nbytes, int flags, char **out, size_t *out_bytes);

/* ---- statistics of the last encode on this handle (for bench.py / roofline) ---- */
typedef struct {
  int64_t n_bytes, n_text, n_total, alphabet, longest_token, n_ids;
  int32_t symbol_bits, symbols_per_key, rounds, sorted_depth, full_depth;
  int64_t radix_pass_elems;   /* sum over all radix passes of the elements moved      */
  int32_t radix_passes;       /* number of radix scatter launches                      */
  int64_t active_per_round[40];
  double ms_total, ms_decode, ms_sa, ms_lcp, ms_scan, ms_walk; /* WP_OPT_STAGE_TIMING */
  double ms_radix_scatter;    /* device time inside radix scatter kernels (HIP events) */
  int64_t n_anchors;          /* start positions of the parallel walk                  */
  int32_t anchor_mode;        /* 0: class rule, 1: coverage rule (WP_OPT_COVER_ANCHORS),
                                 2: class rule + long words by pointer doubling          */
  double ms_h2d, ms_d2h;      /* wp_linear_encode only: host time of the text upload (with
                                 WP_OPT_STAGE_TIMING) and of the id download                */
  int64_t radix_digit_bytes;  /* digit bytes written next to the records by the radix scatter
                                 launches (1 per element and launch, read back by the next
                                 histogram instead of the 8-byte key)                       */
  double ms_host_total;       /* host entry points: wall time of the whole call (upload, device
                                 path, download)                                            */
  int32_t guard_zones;        /* WP_OPT_ARENA_GUARD: guard zones checked (all intact, or the call
                                 fails)                                                     */
  int32_t n_devices;          /* devices that took part (wp_linear_encode_multi), else 1    */
  int32_t vocab_in_s;         /* 1: S = text . 1 . vocab as in linear.cpp:77-101; 0: S = text . 1 and
                                 the vocab comes in through the per-handle vocab structure  */
  int32_t reserved0;          /* 1: this is the bounds-checking build (libwordpiece_amd_dbg.so)     */
  int64_t needed_after_round0; /* depth-capped mode: suffixes in tied groups that carry the key of an
                                 eligible token longer than the key — the only ones that go on to
                                 round 1 (-1: every tied group does, e.g. full depth)          */
  int32_t key_bits;           /* bits of the codeword stream in a round-0 key; keys of up to 32 bits
                                 are sorted as 4-byte keys alone (default layout, see round0_keys_only)
                                 or as 8-byte (key, index) records, longer ones as 12-byte records */
  int32_t staged_emit;        /* 1: ids left the walk as per-workgroup lists (see WP_OPT_SPARSE_EMIT) */
  int32_t rank_in_pass;       /* 1: the ranks of round 0 were computed inside the first partition pass of the rank
                                 store (one more full-size launch of the radix scatter, not in radix_passes) */
  int32_t trie_refine;        /* 1: the needed groups of round 0 were resolved along the token trie (one walk + one segmented
                                 sort) instead of by prefix-doubling rounds (default in the text-only layout) */
  int64_t arena_bytes;        /* device memory of the handle's two bump arenas after this encode                     */
  int32_t list_retries;       /* 1: the needed list outgrew the room it was given and the encode ran a second time   */
  int32_t hist_in_keys;       /* 1: the key builder took the histogram of the sort's first pass (no digit bytes for it) */
  int64_t radix_pass_bytes;   /* algorithmic bytes of the counted radix scatter launches: record read (without the index
                                 column where the pass makes it up) + record written + digit byte written */
  int64_t round0_candidates;  /* keys-only round 0: suffixes whose key is the key of a long token (the candidate list the
                                 needed groups take their positions from); -1 when round 0 sorted (key, index) records */
  int32_t round0_keys_only;   /* 1: round 0 sorted the keys alone (no index column; WP_OPT_INDEXED_ROUND0 turns it off) */
  int32_t offsets_unit;       /* the unit of the last encode's offsets (WP_OFFSETS_*), -1: an ids-only encode        */
  int64_t round0_sorted;      /* suffixes in round 0's sorted array: n_total, or fewer when the keys-only round 0 left out
                                 the blank-start suffixes (see WP_OPT_SORT_BLANKS)                                     */
  int64_t n_rows, rows_truncated; /* documents calls (wp_linear_encode_rows / _padded): the number of rows, and the rows that
                                 lost ids to max_len in a padded call; n_rows -1: the last call was no documents call      */
  int32_t rows_route;         /* documents calls: 1 = one pass over the joined text, 0 = one encode per document (see the
                                 section "documents"); -1: the last call was no documents call                          */
} wp_stats;
int wp_get_stats(const wp_vocab *v, wp_stats *out);
/* WP_OPT_NORMALIZE's part of the statistics of the last encode, in a struct of its own: wp_stats keeps its size and its
 * last field for callers built against it */
typedef struct {
  int32_t normalize;          /* WP_OPT_NORMALIZE flags the last encode ran with (0: none)                              */
  int64_t norm_bytes;         /* bytes of the normalised text the encode ran on (0 without the option); wp_stats.n_bytes
                                 stays the caller's byte count                                                          */
  double ms_normalize;        /* WP_OPT_STAGE_TIMING: device time of the normalisation pre-pass (part of
                                 wp_stats.ms_total)                                                                     */
} wp_norm_stats;
int wp_get_norm_stats(const wp_vocab *v, wp_norm_stats *out);
/* The walk's part of the statistics of the last encode (Linear or fast), in a struct of its own for the same reason:
 * which of the walk's variants produced the ids.  Taken from values the host holds or fetches anyway (no extra wait).
 * Sharded and pipelined calls report the sums of the two counts, the largest gap and the first text's `lean`. */
typedef struct {
  int64_t n_wide_words;   /* stretches [anchor, next anchor) of more than 48 positions that a whole wave walked (Linear,
                             class rule with hard spacing chars only; 0: the wide walk did not run)                     */
  int64_t n_long_words;   /* words of more than 2048 positions walked by pointer doubling (wp_stats.anchor_mode == 2)    */
  int32_t lean;           /* 1: the Linear path's list-building walk kernel; 0: the per-position walk kernel of
                             WP_OPT_SPARSE_EMIT / long words, or the fast path's kernels                                 */
  int32_t max_anchor_gap; /* the largest distance between neighbouring class-rule anchors (text start and end included),
                             as the gap kernel reports it: when no spacing char occurs inside a token (and always in
                             the fast path) a distance above 2048 is measured up to the first blank and stops at 2049 */
} wp_walk_stats;
int wp_get_walk_stats(const wp_vocab *v, wp_walk_stats *out);
/* The refinement's part of the statistics of the last encode, in a struct of its own for the same reason: what the
 * stage between round 0 and the walk ran on (the needed groups along the token trie by default, the first doubling
 * round otherwise).  Taken from values the host holds at that point (no extra wait, no extra kernel).  All zero when
 * the stage was not reached (an empty text, the fast path); the four counts are zero when nothing was on the list.  Sharded and pipelined calls report the sums
 * of the four counts and the first text's other fields. */
typedef struct {
  int64_t n_groups;         /* groups on the list of the first refinement round (trie round: the needed groups)         */
  int64_t n_entries;        /* its entries; wp_stats.needed_after_round0 when round 0 was pruned                         */
  int64_t n_large_groups;   /* groups of more than 2048 entries, sorted by the global radix path instead of in LDS;
                               0 when the list was too short for one (no classification ran)                             */
  int64_t n_large_entries;  /* their entries                                                                             */
  int64_t trie_nodes;       /* nodes of the trie of the long tokens (a property of the vocabulary)                       */
  int32_t sort_bits;        /* bits of the second key the segmented sort ran with: bit_length(trie_nodes + 1) in the trie
                               round, bit_length(n_total) in a doubling round                                            */
  int32_t key_lookup;       /* 1: the walk looked its steps up by round-0 key and no full rank table was built           */
  int32_t symbol_bytes;     /* width of a dense symbol: 1 (alphabets up to 255), else 4                                  */
  int32_t reserved;
} wp_refine_stats;
int wp_get_refine_stats(const wp_vocab *v, wp_refine_stats *out);
/* Where the refinement of the last encode was queued, in a struct of its own for the same reason. */
typedef struct {
  int32_t early;            /* 1: the needed groups were built and refined beside the round-0 passes (keys-only round 0
                               without WP_OPT_LATE_REFINE); 0: behind the sort, or no refinement ran                      */
  int32_t reserved;
  double ms_sort_to_scan;   /* WP_OPT_STAGE_TIMING: device time from the end of the last round-0 pass to the first kernel
                               of the scanline stage (HIP events), else 0                                                */
} wp_refine_sched;
int wp_get_refine_sched(const wp_vocab *v, wp_refine_sched *out);
/* The step tables of the last Linear encode (csrc/scanline.h: what the walk looks its longest matches up in), in a
 * struct of its own for the same reason; from values the host holds anyway.  All zero when the stage was not reached.
 * Sharded and pipelined calls report the first text's. */
typedef struct {
  int64_t n_marks;          /* eligible tokens M: the marks of the scanlines                                             */
  int64_t n_steps;          /* steps of the table: 4 M + 1, and with key_lookup two more per needed group                */
  int64_t n_tiles;          /* tiles of 4096 slots of the total length (the scanlines of the reference layout)           */
  int64_t n_groups_of_tiles; /* groups of 64 tiles                                                                       */
  int32_t bucket_shift;     /* slot >> bucket_shift indexes the slot-space table                                         */
  int32_t bucket_shift_all; /* ... its small index, for the kernels that look up every position of a long word           */
  int32_t key_shift;        /* round-0 key >> key_shift indexes the key-space table (key_lookup; else as computed)       */
  int32_t key_shift_all;    /* ... its small index                                                                       */
  int32_t packed;           /* 1: a step value carries the token's length above its id (ids < 2^20, lengths < 2^11)      */
  int32_t key_lookup;       /* 1: the walk looked its steps up by round-0 key (wp_refine_stats.key_lookup)               */
} wp_step_stats;
int wp_get_step_stats(const wp_vocab *v, wp_step_stats *out);
/* The model-inputs part of the statistics of the last call, in a struct of its own for the same reason.  After an
 * inputs call wp_stats.n_rows, rows_route, offsets_unit and n_ids mean what they mean after a rows call and
 * rows_truncated is 0. */
typedef struct {
  int64_t n_samples, n_out;  /* samples and output rows; n_out -1: the last call was no inputs call                     */
  int64_t n_cut;             /* samples that lost ids for good (truncation, or a fixed side cut to leave a window room)  */
  int64_t n_windowed;        /* samples with more than one window                                                        */
  int32_t pairs, truncation, stride, reserved; /* of the call's wp_inputs_spec                                          */
} wp_inputs_stats;
int wp_get_inputs_stats(const wp_vocab *v, wp_inputs_stats *out);

/* ---- debug fetch (WP_OPT_KEEP_DEBUG): copies device intermediates to host ----
 * which: 0 S (dense symbols as int32, n), 1 SA (n), 2 rank (n; the inverse SA is kept only with this option, full
 * depth or the reference layout — the default layout otherwise has no rank table: the slots of the suffixes of needed
 * groups stand in the place of their round-0 keys, and the call fails), 3 lcp (n-1; -1 = "at least
 * sorted_depth"), 4 best_prefix (n), 5 best_suffix (n), 6 code points (n_text), 7 class bytes (n_text, as int32:
 * 1 is_space, 2 is_spacing_char, 4 soft spacing char, 8 is_punctuation; the Linear path's anchor kernels add 16 at a
 * word-prefix position and 32 at an anchor of the walk; 64, "the key's word holds the slot", is set only where the
 * key lookup is on, which this option turns off).
 * WP_OPT_KEEP_DEBUG = 2 keeps four views by text position instead (n_text each; the others fail), written by one kernel
 * in front of the walk through the walk's own lookup (key-space table, then rank and slot-space table for the key of a
 * needed group): 8 / 9 the id of the longest prefix-class / ##-class token that matches at the position, -1 for none
 * and at blank positions (the walk never looks them up); 10 / 11 that token's length in code points, 0 where the id
 * is -1. */
int wp_linear_debug_fetch(const wp_vocab *v, int which, int32_t *out, size_t capacity,
                          size_t *n_out);

void wp_free(void *p);
const char *wp_last_error(void);
int wp_device_count(void);

#ifdef __cplusplus
}
#endif
#endif
