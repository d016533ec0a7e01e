/* wordpiece_amd_repetition.h — the repetition signals of a document: its most frequent word n-grams and its duplicated
 * word n-grams, with the rules over them (the repetition half of the MassiveText (Gopher) filters, as FineWeb and
 * DataTrove run them in front of deduplication).  An addition beside the quality signals of wordpiece_amd.h; the entry
 * points live in the same library.  This section is the contract; tests/repetition_model.py is its executable form.
 *
 * wp_repetition_rows[_device](v, data, row_off, n_rows, spec, out).  data: text bytes (elem_bytes 1 only); row_off int64
 * [n_rows + 1], ascending from 0, as wp_quality_rows takes it, with the same intake rules.  No vocabulary is read and no
 * normalisation applied; the handle lends its context.  Every signal of row i is a function of that row's bytes alone.
 * Words.  The words of wp_quality_rows per row (wordpiece_amd.h, "quality signals"): a punctuation or CJK character is a
 * word of its own, and an invalid byte is a character without a class, so it is part of a word.  A word's characters are
 * its code points as that call counts them.  Two words are equal iff their bytes are equal: no normalisation, no case
 * folding.
 * N-grams.  The n-gram at word position p of a row is its words p .. p + n - 1; it exists only where all n words lie in
 * the row, so no window crosses a row end.  What stands between the words is no part of it ("a  b" and "a\tb" are the
 * same 2-gram; "ab c" and "a bc" are different ones).  Its characters are the sum of its words' characters.
 * Signals.  signals int64 [WP_RPT_SIGNALS][n_rows], signal-major, indices WP_RPT_*:
 *   WORDS, WORD_CHARS          the words of the row and the sum of their characters (the denominator of every rule);
 *   TOP_n_COUNT, TOP_n_CHARS   n = 2, 3, 4: among the distinct n-grams of the row the pairs (occurrences, characters)
 *                              are ordered by occurrences, then by characters; the largest pair gives TOP_n_COUNT = its
 *                              occurrences and TOP_n_CHARS = occurrences * characters.  Both are 0 where no n-gram
 *                              occurs twice.  The largest pair is a pure function of the row: where two n-grams tie in
 *                              both, they give the same two numbers;
 *   DUP_n_CHARS                n = 5 .. 10: an occurrence is a duplicate where an equal n-gram begins at a smaller word
 *                              position of the same row (the first occurrence stays); a word is covered where some
 *                              duplicate n-gram holds it; the signal is the sum of the characters of the covered words,
 *                              each once however many windows overlap it.
 * Rules.  limit int64 [WP_RPT_RULES], rule k for n = k + 2, each -1 (off) or in [0, 1000]: the row fails where
 * X * 1000 > limit * WORD_CHARS, X = TOP_n_CHARS (n <= 4) or DUP_n_CHARS.  A zero denominator passes (both sides are 0).
 * The published thresholds can be stated in these rules (the Python wrapper has Gopher's as a preset) over THIS
 * contract's words and denominator: parity with DataTrove's tokeniser, its greedy non-overlapping scan of the duplicated
 * n-grams and its len(text) denominator is not claimed.
 * Results.  reasons uint32 [n_rows], bit k set where rule k failed; a row is kept iff its reasons are 0.  With
 * WP_RPT_WANT_COMPACT: kept int32 [n_kept] ascending and the kept rows whole and back to back as data and row_off int64
 * [n_kept + 1], n_elems bytes: the compact form of wp_quality_rows, what wp_dedup_rows_device takes.
 * Exactness.  No result depends on a hash or on an order of execution.  Words get the index of the first word with
 * their bytes from the exact duplicate-row search; the order of the windows comes from sorts of pairs of exact ranks;
 * what lanes combine is an integer sum, maximum or minimum.
 * WP_ERR_ARG, before a device is touched and with the field named: spec or out NULL, elem_bytes not 1, want with a bit
 * outside 1, a limit outside {-1} and [0, 1000], reserved not 0, row_off NULL with n_rows > 0, data NULL with bytes; bad
 * offsets with the first bad row, as wp_quality_rows.  WP_ERR_TOO_LARGE: n_rows >= 2^31, more than UINT32_MAX bytes, or
 * 2^30 words or more.
 * Host form: the blocks of *out are malloc'd, each freed with wp_free; n_rows == 0 returns all NULL; a batch of 0 bytes is
 * answered on the host (signals 0, reasons the rules over zeros).  Device form: the buffer contract of
 * wp_quality_rows_device; the arrays of *d_out are device memory owned by the handle until its next call (the next dedup
 * call included: the word identities come through its buffers).
 * With WP_OPT_STAGE_TIMING a call leaves its device times in wp_stats: ms_decode (intake, class passes, word list, word
 * identity), ms_sa (the five sorts with their rank passes), ms_scan (the LCP and the run passes), ms_walk (cover, rules,
 * compact form), ms_total (their sum).  A repetition call leaves the statistics of every other layer as they were. */
#ifndef WORDPIECE_AMD_REPETITION_H
#define WORDPIECE_AMD_REPETITION_H
#include "wordpiece_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WP_RPT_SIGNALS 14
#define WP_RPT_RULES   9
#define WP_RPT_WANT_COMPACT 1
enum { WP_RPT_WORDS = 0, WP_RPT_WORD_CHARS, WP_RPT_TOP_2_COUNT, WP_RPT_TOP_2_CHARS, WP_RPT_TOP_3_COUNT, WP_RPT_TOP_3_CHARS, WP_RPT_TOP_4_COUNT,
       WP_RPT_TOP_4_CHARS, WP_RPT_DUP_5_CHARS, WP_RPT_DUP_6_CHARS, WP_RPT_DUP_7_CHARS, WP_RPT_DUP_8_CHARS, WP_RPT_DUP_9_CHARS, WP_RPT_DUP_10_CHARS };
typedef struct { int32_t elem_bytes, want; int64_t limit[WP_RPT_RULES]; int64_t reserved; } wp_repetition_spec;
typedef struct { int64_t *signals, *row_off; uint32_t *reasons; int32_t *kept; void *data; int64_t n_rows, n_kept, n_elems; } wp_repetition_result;
int wp_repetition_rows(wp_vocab *v, const void *data, const int64_t *row_off, size_t n_rows, const wp_repetition_spec *spec, wp_repetition_result *out);
int wp_repetition_rows_device(wp_vocab *v, const void *d_data, const int64_t *d_row_off, size_t n_rows, const wp_repetition_spec *spec, wp_repetition_result *d_out);
/* The statistics of the last repetition call: the rows, their bytes, the sums of WORDS and WORD_CHARS over them, the kept
 * rows, and rule_failed[k], the rows rule k failed. */
typedef struct { int64_t n_rows, n_bytes, n_words, n_word_chars, n_kept, rule_failed[WP_RPT_RULES]; } wp_repetition_stats;
int wp_get_repetition_stats(const wp_vocab *v, wp_repetition_stats *out);   /* n_rows == -1: no such call yet, or an encode since */

#ifdef __cplusplus
}
#endif
#endif
