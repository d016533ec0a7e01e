/* wordpiece_amd_scrub.h — the scrub: e-mail addresses and IPv4 addresses of a document replaced by placeholders, on the
 * device (the PII formatter that stands between the filters and the tokeniser of a corpus pipeline).  An addition beside
 * the line filter of wordpiece_amd_lines.h; the entry points live in the same library.  This section is the contract;
 * tests/scrub_model.py is its executable form.  The patterns are this header's own: parity with DataTrove's regular
 * expressions is NOT claimed, nor parity of the private ranges with ipaddress.is_global of any Python version.
 *
 * wp_scrub_rows[_device](v, data, row_off, n_rows, spec, out).  data: text bytes (elem_bytes 1 only); row_off int64
 * [n_rows + 1], ascending from 0, as wp_filter_lines takes it, with the same intake rules.  No vocabulary is read and no
 * normalisation applied; the handle lends its context.  A match never crosses a row's end: every "run" below is maximal
 * inside its row.
 * Byte classes, all ASCII.  AL [A-Za-z]; AN [A-Za-z0-9]; LOC: AN and . _ % + -; DOM: AN and . -; NUM [0-9.]; WORDISH: AN,
 * _ and every byte >= 0x80 (the convention of the line filter's bounded phrases).
 * E-mail (kinds & WP_SCRUB_EMAIL).  At every '@' at byte p: R is the maximal run of LOC bytes that ends at p - 1; no match
 * if R has more than 64 bytes, or if the byte in front of R is '@'.  The local part is R without its leading bytes that
 * are not AN; no match if it is empty.  D is the maximal run of DOM bytes from p + 1; no match if D has more than 255
 * bytes.  D split at '.' gives the labels L1, L2, ...; a label is valid iff it has 1 to 63 bytes and neither begins nor
 * ends with '-'.  The domain is L1. ... .Lk for the largest k >= 2 such that L1 .. Lk are all valid and Lk has at least
 * two bytes, all AL; no match if there is no such k.  The match is [start of the local part, end of Lk).  Two e-mail
 * matches are disjoint (DOM is part of LOC, so a local run that reaches back into a domain reaches its '@').
 * IPv4 (kinds & WP_SCRUB_IPV4).  For every maximal run T of NUM bytes: no match if the byte in front of T or the byte
 * behind it lies inside the row and is WORDISH, or if T has more than 16 bytes.  T' is T without one trailing '.', if it
 * has one; T' must be d.d.d.d, each d 1 to 3 digits, at most 255, with no leading zero other than "0" itself.  The match
 * is T'.  An IPv4 match that lies inside an e-mail match is dropped ("1.2.3.4@example.com" is one e-mail); no other
 * intersection occurs.  With WP_SCRUB_IP_KEEP_PRIVATE a match whose address lies in 0.0.0.0/8, 10.0.0.0/8, 127.0.0.0/8,
 * 169.254.0.0/16, 172.16.0.0/12, 192.168.0.0/16 or 224.0.0.0/3 stays in the text; it is listed with kind 2 and counted as
 * IPS_LEFT.
 * Replacement.  n_email_repl and n_ip_repl strings, 0 to 16 each and at least one where the kind is searched, in host
 * memory (both forms): repl_pool and repl_off int64 [n_email_repl + n_ip_repl + 1] from 0, the e-mail strings first.  A
 * string has 0 to 64 bytes (0 deletes the match) and no 0x0A; the pool has at most 2,048 bytes.  A match is replaced by
 * string h mod n of its kind, h the 32-bit FNV-1a hash of its bytes with A-Z folded to lower case:
 * h = 2166136261, then h = (h ^ b) * 16777619 per byte.  The hash is part of the contract: the same address gets the
 * same placeholder in every row and in every call.  Nothing else depends on a hash or on an order of execution: lanes
 * combine values by integer add alone.
 * Signals.  signals int64 [WP_SCRUB_SIGNALS][n_rows], signal-major: BYTES and OUT_BYTES (the row's bytes before and after
 * the scrub), AT_SIGNS (its '@' bytes, whatever kinds says), EMAILS and EMAIL_BYTES (the e-mail matches and their bytes
 * in data), IPS and IP_BYTES (the replaced IPv4 matches and their bytes in data), IPS_LEFT.
 * Document rules.  doc_limit int64 [2], each -1 (off) or in [0, 10^9]; reasons uint32 per row, bit k set where rule k
 * fails:   0 MAX_EMAILS  EMAILS > L        1 MAX_IPS  IPS + IPS_LEFT > L
 * Results.  signals and reasons always.  WP_SCRUB_WANT_MATCHES: n_matches and, per match in text order, match_row int32,
 * match_start int64 (counted from the start of data), match_len int32, match_kind int32 (0 e-mail, 1 IPv4 replaced, 2
 * IPv4 left) and match_repl int32 (the index inside its kind's list, -1 for kind 2).  WP_SCRUB_WANT_TEXT: out_data
 * (n_out_elems bytes) and out_off int64 [n_rows + 1]: every row with its matches replaced; the row index is unchanged and
 * reasons are not consulted.  WP_SCRUB_WANT_COMPACT: kept int32 [n_kept] ascending, data (n_elems bytes) and row_off int64
 * [n_kept + 1]: the rows with reasons == 0, AFTER the scrub, back to back: what wp_dedup_rows_device and the encode of
 * rows take.
 * WP_ERR_ARG, before a device is touched and with the field named: spec or out NULL, elem_bytes not 1, want with a bit
 * outside 7, kinds with a bit outside 7, pad not 0, doc_limit[k] outside {-1} and [0, 10^9], n_email_repl / n_ip_repl
 * outside [0, 16] or 0 where the kind is searched, repl_pool / repl_off NULL with strings, repl_off[0] not 0, and with the
 * index of the first bad string: a length outside 0..64, an end behind the 2,048 bytes of a pool, 0x0A in it; reserved
 * not 0; row_off NULL with n_rows > 0, data NULL with bytes; bad offsets with the first bad row.  WP_ERR_TOO_LARGE:
 * n_rows >= 2^31, more than UINT32_MAX bytes, more than UINT32_MAX bytes behind the scrub (from 64-bit totals, before
 * the text is written).
 * Host form: the blocks of *out are malloc'd, each freed with wp_free; n_rows == 0 returns all NULL; a batch of 0 bytes
 * is answered on the host (signals 0, reasons 0, no match, every row empty).  Device form: the buffer contract of
 * wp_filter_lines_device; the arrays of *d_out are device memory owned by the handle until its next call.
 * With WP_OPT_STAGE_TIMING a call leaves its device times in wp_stats: ms_decode (intake), ms_sa (both find passes),
 * ms_scan (offsets), ms_walk (document rules, text, compact form), ms_total (their sum).
 * A call leaves the statistics of every other layer as they were. */
#ifndef WORDPIECE_AMD_SCRUB_H
#define WORDPIECE_AMD_SCRUB_H
#include "wordpiece_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WP_SCRUB_SIGNALS 8
#define WP_SCRUB_RULES   2
#define WP_SCRUB_MAX_REPL       16
#define WP_SCRUB_MAX_REPL_BYTES 64
#define WP_SCRUB_MAX_POOL_BYTES 2048
#define WP_SCRUB_EMAIL           1
#define WP_SCRUB_IPV4            2
#define WP_SCRUB_IP_KEEP_PRIVATE 4
#define WP_SCRUB_WANT_MATCHES 1
#define WP_SCRUB_WANT_TEXT    2
#define WP_SCRUB_WANT_COMPACT 4
enum { WP_SS_BYTES = 0, WP_SS_OUT_BYTES, WP_SS_AT_SIGNS, WP_SS_EMAILS, WP_SS_EMAIL_BYTES, WP_SS_IPS, WP_SS_IP_BYTES, WP_SS_IPS_LEFT };
enum { WP_SR_MAX_EMAILS = 0, WP_SR_MAX_IPS };
typedef struct {
  int32_t elem_bytes, want, kinds, pad;
  int64_t doc_limit[WP_SCRUB_RULES];
  int32_t n_email_repl, n_ip_repl;
  const void *repl_pool;
  const int64_t *repl_off;
  int64_t reserved;
} wp_scrub_spec;
typedef struct {
  int64_t *signals, *match_start, *out_off, *row_off;
  uint32_t *reasons;
  int32_t *match_row, *match_len, *match_kind, *match_repl, *kept;
  void *out_data, *data;
  int64_t n_rows, n_matches, n_out_elems, n_kept, n_elems;
} wp_scrub_result;
int wp_scrub_rows(wp_vocab *v, const void *data, const int64_t *row_off, size_t n_rows, const wp_scrub_spec *spec, wp_scrub_result *out);
int wp_scrub_rows_device(wp_vocab *v, const void *d_data, const int64_t *d_row_off, size_t n_rows, const wp_scrub_spec *spec, wp_scrub_result *d_out);
/* The statistics of the last scrub call: the rows, their bytes, the bytes behind the scrub, n_matches[k] the matches of
 * kind k (0 e-mail, 1 IPv4 replaced, 2 IPv4 left), rule_failed[k] the rows that failed document rule k, and the rows with
 * reasons 0. */
typedef struct { int64_t n_rows, n_bytes, n_out_bytes, n_matches[3], rule_failed[WP_SCRUB_RULES], n_kept; } wp_scrub_stats;
int wp_get_scrub_stats(const wp_vocab *v, wp_scrub_stats *out);   /* n_rows == -1: no such call yet */

#ifdef __cplusplus
}
#endif
#endif
