/* wordpiece_amd_lines.h — the line filter: drop single lines of a document by rule, by phrase and by repetition, and hand
 * the documents back without them (the line-level step of C4, with CCNet's duplicate-line removal).  An addition beside
 * the quality signals of wordpiece_amd.h; the entry points live in the same library.  This section is the contract;
 * tests/lines_model.py is its executable form.
 *
 * wp_filter_lines[_device](v, data, row_off, n_rows, spec, out).  data: text bytes (elem_bytes 1 only); row_off int64
 * [n_rows + 1], ascending from 0, as wp_quality_rows takes it, with the same intake rules.  No vocabulary is read and no
 * normalisation applied; the handle lends its context.
 * Characters, words and lines are those of wp_quality_rows (wordpiece_amd.h, "quality signals").  A line is a maximal run
 * of bytes other than 0x0A in a row.  Its words are the words that start inside it; its characters are the characters
 * that start inside it; its last character is the last byte of the last word that ends in it.  A line OWNS the bytes
 * from its start up to the start of the next line of its row, or up to the row end: itself and the line feeds behind it.
 * Line feeds in front of a row's first line belong to no line and are never removed.
 * Phrases.  n_phrases in [0, 512], given in host memory (both forms) as phrase_pool + phrase_off int64 [n_phrases + 1]
 * from 0, and phrase_flags int32 per phrase (WP_LF_PHRASE_*).  A phrase has 1 to 32 bytes, the pool at most 8,192; it
 * holds no ASCII upper case and no 0x0A, any other byte is allowed.  Phrase t MATCHES at byte p of a row iff
 * [p, p + len) lies inside the row; the bytes are equal, with 0x41..0x5A of the text folded to lower case and nothing
 * else; and, with WP_LF_PHRASE_BOUNDED, the byte in front of the match and the byte behind it each lie outside the row
 * or are an ASCII byte other than [0-9A-Za-z] (a byte >= 0x80 counts as a letter).  A match lies in one line.  A phrase
 * with WP_LF_PHRASE_DOC is a document phrase, any other a line phrase.  Equal phrases may be listed twice; each counts.
 * Line rules.  line_reasons uint32 per line, bit k set where the line fails rule k; a line is dropped iff it is not 0.
 * line_limit int64 [4], each -1 (off) or in [0, 10^9]:
 *   0 MIN_WORDS     words < L                      1 MIN_CHARS     characters < L
 *   2 NOT_TERMINAL  (L 0 or -1) it has no last character, or that is none of . ! ? " '
 *   3 ELLIPSIS_END  (L 0 or -1) the ELLIPSIS_LINES rule of the quality signals holds for it
 *   4 PHRASE        a line phrase matches inside it
 *   5 DUPLICATE     it has at least dup_min_chars characters and its bytes (the line feed is no part of them) equal
 *                   those of a line at a smaller byte position: of the same row with dup_scope 1, of the whole batch
 *                   with dup_scope 2; dup_scope 0: off.
 * Signals.  signals int64 [WP_LF_SIGNALS][n_rows], signal-major: BYTES and KEPT_BYTES (the row's bytes, and those minus
 * what its dropped lines own), LINES and KEPT_LINES, LINE_CHARS and KEPT_CHARS (the characters of the lines: no line
 * feed), WORDS and KEPT_WORDS, FAILED_0 .. FAILED_5 (the lines that fail each rule; a line may fail several),
 * DOC_PHRASE_HITS (the (position, phrase) matches of document phrases, in any line, kept or not).
 * Document rules.  doc_limit int64 [4], each -1 or in [0, 10^9]; reasons uint32 per row, bit k set where rule k fails;
 * integer inequalities, a zero denominator passes:
 *   0 MIN_KEPT_LINES  KEPT_LINES < L        2 MAX_DROPPED_X1000    (LINE_CHARS - KEPT_CHARS) * 1000 > L * LINE_CHARS
 *   1 MIN_KEPT_WORDS  KEPT_WORDS < L        3 MAX_DOC_PHRASE_HITS  DOC_PHRASE_HITS > L
 * Results.  signals and reasons always.  WP_LF_WANT_LINES: n_lines and, per line in text order, line_row int32,
 * line_start int64 (its first byte, counted from the start of data), line_len int32 (bytes) and line_reasons.
 * WP_LF_WANT_CUT: cut_data (n_cut_elems bytes) and cut_off int64 [n_rows + 1]: every row without what its dropped lines
 * own; the row index is unchanged and reasons are not consulted (the cut form of wp_repeat_rows).  WP_LF_WANT_COMPACT:
 * kept int32 [n_kept] ascending, data (n_elems bytes) and row_off int64 [n_kept + 1]: the rows with reasons == 0, AFTER
 * the cut, back to back: what wp_dedup_rows_device and the encode of rows take.
 * Exactness.  No result depends on a hash or on an order of execution: lanes combine values by integer add and bitwise
 * or alone, and the duplicate lines come from the exact duplicate-row search.
 * WP_ERR_ARG, before a device is touched and with the field named: spec or out NULL, elem_bytes not 1, want with a bit
 * outside 7, line_limit[k] / doc_limit[k] outside {-1} and [0, 10^9], line_limit[2] or [3] other than 0 or -1, dup_scope
 * outside 0..2, dup_min_chars negative, n_phrases outside [0, 512], pad not 0, phrase_pool / phrase_off / phrase_flags NULL with
 * phrases, phrase_off[0] not 0, and with the index of the first bad phrase: a length outside 1..32, ASCII upper case or
 * 0x0A in it, flags with a bit outside 3; a pool of more than 8,192 bytes; reserved not 0; row_off NULL with n_rows > 0,
 * data NULL with bytes; bad offsets with the first bad row.  WP_ERR_TOO_LARGE: n_rows >= 2^31, more than UINT32_MAX
 * bytes, 2^30 lines or more with dup_scope != 0.
 * Host form: the blocks of *out are malloc'd, each freed with wp_free; n_rows == 0 returns all NULL; a batch of 0 bytes
 * is answered on the host (signals 0, reasons the document rules over zeros, no line, every row empty).  Device form: the
 * buffer contract of wp_quality_rows_device; the arrays of *d_out are device memory owned by the handle until its next
 * call (the next dedup call included: the duplicate lines come through its buffers).
 * With WP_OPT_STAGE_TIMING a call leaves its device times in wp_stats: ms_decode (intake, class passes, lists), ms_sa
 * (phrase scan and line pass), ms_scan (duplicates), ms_walk (document rules, cut, compact form), ms_total (their sum).
 * A call leaves the statistics of every other layer as they were. */
#ifndef WORDPIECE_AMD_LINES_H
#define WORDPIECE_AMD_LINES_H
#include "wordpiece_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WP_LF_SIGNALS    15
#define WP_LF_LINE_RULES 6
#define WP_LF_DOC_RULES  4
#define WP_LF_MAX_PHRASES      512
#define WP_LF_MAX_PHRASE_BYTES 32
#define WP_LF_MAX_POOL_BYTES   8192
#define WP_LF_WANT_LINES   1
#define WP_LF_WANT_CUT     2
#define WP_LF_WANT_COMPACT 4
#define WP_LF_PHRASE_BOUNDED 1
#define WP_LF_PHRASE_DOC     2
enum { WP_LF_BYTES = 0, WP_LF_KEPT_BYTES, WP_LF_LINES, WP_LF_KEPT_LINES, WP_LF_LINE_CHARS, WP_LF_KEPT_CHARS, WP_LF_WORDS, WP_LF_KEPT_WORDS, WP_LF_FAILED_0,
       WP_LF_FAILED_1, WP_LF_FAILED_2, WP_LF_FAILED_3, WP_LF_FAILED_4, WP_LF_FAILED_5, WP_LF_DOC_PHRASE_HITS };
enum { WP_LR_MIN_WORDS = 0, WP_LR_MIN_CHARS, WP_LR_NOT_TERMINAL, WP_LR_ELLIPSIS_END, WP_LR_PHRASE, WP_LR_DUPLICATE };
enum { WP_LD_MIN_KEPT_LINES = 0, WP_LD_MIN_KEPT_WORDS, WP_LD_MAX_DROPPED_X1000, WP_LD_MAX_DOC_PHRASE_HITS };
typedef struct {
  int32_t elem_bytes, want;
  int64_t line_limit[4], doc_limit[WP_LF_DOC_RULES];
  int32_t dup_scope, dup_min_chars, n_phrases, pad;
  const void *phrase_pool;
  const int64_t *phrase_off;
  const int32_t *phrase_flags;
  int64_t reserved;
} wp_lines_spec;
typedef struct {
  int64_t *signals, *line_start, *cut_off, *row_off;
  uint32_t *reasons, *line_reasons;
  int32_t *line_row, *line_len, *kept;
  void *cut_data, *data;
  int64_t n_rows, n_lines, n_cut_elems, n_kept, n_elems;
} wp_lines_result;
int wp_filter_lines(wp_vocab *v, const void *data, const int64_t *row_off, size_t n_rows, const wp_lines_spec *spec, wp_lines_result *out);
int wp_filter_lines_device(wp_vocab *v, const void *d_data, const int64_t *d_row_off, size_t n_rows, const wp_lines_spec *spec, wp_lines_result *d_out);
/* The statistics of the last line-filter call: the rows, their bytes, the lines, the kept lines, the bytes the cut
 * leaves, the rows with reasons 0, line_failed[k] the lines that failed line rule k, rule_failed[k] the rows that failed
 * document rule k, and the phrase matches ((position, phrase) pairs, line and document phrases together). */
typedef struct { int64_t n_rows, n_bytes, n_lines, n_kept_lines, n_kept_bytes, n_kept, line_failed[WP_LF_LINE_RULES], rule_failed[WP_LF_DOC_RULES],
                 n_phrase_matches; } wp_lines_stats;
int wp_get_lines_stats(const wp_vocab *v, wp_lines_stats *out);   /* n_rows == -1: no such call yet, or an encode since */

#ifdef __cplusplus
}
#endif
#endif
