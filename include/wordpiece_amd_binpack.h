/* wordpiece_amd_binpack.h — encoded documents packed into fixed-length rows by best-fit decreasing: long documents are cut
 * into chunks of at most one row, the chunks go into rows longest first, each into the fullest row that still has room
 * (Ding et al., "Fewer Truncations Improve Language Modeling", ICML 2024; what the histogram packers for BERT
 * approximate).  An addition beside the pack section of wordpiece_amd.h; the entry points live in the same library.  This
 * section is the contract; tests/binpack_model.py is its executable form.
 *
 * wp_pack_best_fit(v, ids, row_splits, n_docs, spec, out, n_out) and wp_pack_best_fit_device(v, d_ids, d_row_splits,
 * n_docs, spec, d_out, capacity_rows, n_out) follow wp_pack_sequences and wp_pack_sequences_device in arguments,
 * ownership and error order: host blocks are freed with wp_free, device buffers are the caller's; with capacity_rows <
 * n_out the needed count is in *n_out and nothing is written; n_docs == 0 or only empty documents gives n_out == 0 and
 * every block NULL, and the host entry point then needs no device; the 32-bit limits are checked from 64-bit totals
 * before the write pass.  out / d_out is the wp_packed of the pack section.
 * Spec.  long_docs and want take the WP_PACK_LONG_* and WP_PACK_WANT_* values; both reserved fields must be 0; max_len
 * lies in [1, WP_BINPACK_MAX_LEN] (the cap keeps the length histogram of a workgroup in 32 KB of static LDS).
 * Pieces and units are exactly those of the pack section under WP_PACK_NEXT_FIT with the given long_docs: truncate gives
 * one piece of at most B ids per document, split gives ceil(l / B), an empty document none; the unit of a piece is [bos]
 * ids [eos] of u = n + s cells, 1 <= u <= L; pieces are numbered k = 0 .. n_p - 1 in document order.
 * Rows.  (1) sigma: the pieces ordered by u descending, ties by k ascending.  (2) Every remaining capacity r in 1 .. L
 * has a FIFO queue of rows; rows are numbered in the order they are opened.  (3) For each unit in sigma order take the
 * smallest r >= u whose queue is not empty: if there is one, the unit goes to the row at that queue's head and the row
 * leaves the queue; if there is none, the unit goes to a newly opened row with r = L.  (4) The unit stands at column
 * L - r, behind the units already in the row.  (5) If r - u > 0 the row joins the tail of queue r - u.
 * n_out is the number of rows opened.  Inside a row the units stand in the order placed: longest first.  The multiset of
 * remaining capacities does not depend on which of several rows with equal r is taken, so n_out equals that of textbook
 * best-fit decreasing under any tie rule; the FIFO rule only fixes WHICH batch of that size comes out.
 * Cells.  With the units of the rows read row by row in that order, every output is as the pack section defines it for
 * next fit: input_ids, lengths, segment_ids (1 + the unit's index in its row), position_ids and source, whose entries
 * >= 0 are no longer ascending.  Padding is written; nothing behind row n_out is touched.
 * Planner.  wp_binpack_plan(hist, max_len, out) is a host function and needs no device: hist[u], u in 0 .. max_len, is
 * the number of units of u cells (hist[0] is ignored); out gets n_out, n_units, n_cells and two malloc'd tables (each
 * freed with wp_free; NULL where empty), the run-length form of the procedure above.
 *   A run {first_rank, row0, n_rows, unit, per_row, slot0, col0}: the units at sigma-ranks first_rank + j * per_row + t,
 *   j < n_rows, t < per_row, all have `unit` cells, and each stands in row row0 + j at slot slot0 + t and column col0 +
 *   t * unit.  Runs tile the sigma-ranks 0 .. n_units - 1 in order.
 *   A row range {row0, n_rows, first_unit, first_cell, units_per_row, cells_per_row}: a maximal stretch of consecutive
 *   rows that ended with the same pattern; ranges ascend in row0 and tile 0 .. n_out - 1; first_unit and first_cell are
 *   the units and cells of all rows in front.
 * The rows of a queue entry share one history, so the planner keeps groups of rows (row0, count), never single rows; a
 * group that takes units of length u takes floor(r / u) per row at once; a partly used group splits into a used
 * prefix, at most one partly filled row, and the rest, which stays at the head.  The work depends on max_len alone,
 * never on the number of documents: at most about 3 L sqrt(2 L) group moves.  A caller of the device form sizes
 * capacity_rows with it.  WP_ERR_ARG: hist or out NULL, max_len outside [1, WP_BINPACK_MAX_LEN], a negative count.
 * Errors.  WP_ERR_ARG comes before a device is touched, the texts prefixed "binpack:": spec NULL, an unknown long_docs,
 * want with bits outside 7, max_len outside [1, 8192], no room for an id beside the specials, a reserved field that is
 * not 0, the pointer and alignment rules of the pack calls, bad row_splits (the host form checks them on the host, the
 * device form in a kernel before anything is written).  WP_ERR_TOO_LARGE follows the pack calls.
 * A call leaves the statistics of every other layer as they were, wp_get_pack_stats and wp_stats included. */
#ifndef WORDPIECE_AMD_BINPACK_H
#define WORDPIECE_AMD_BINPACK_H
#include "wordpiece_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WP_BINPACK_MAX_LEN 8192
typedef struct { int32_t max_len, bos_id, eos_id, pad_id, long_docs, want, reserved0, reserved1; } wp_binpack_spec;
typedef struct { int64_t first_rank, row0, n_rows; int32_t unit, per_row, slot0, col0; } wp_binpack_run;
typedef struct { int64_t row0, n_rows, first_unit, first_cell; int32_t units_per_row, cells_per_row; } wp_binpack_row_range;
typedef struct {
  int64_t n_out, n_units, n_cells, n_runs, n_row_ranges;
  wp_binpack_run *runs;
  wp_binpack_row_range *row_ranges;
} wp_binpack_plan_result;
/* host ids in; the blocks out (free each with wp_free) */
int wp_pack_best_fit(wp_vocab *v, const int32_t *ids, const int64_t *row_splits, size_t n_docs, const wp_binpack_spec *spec,
                     wp_packed *out, size_t *n_out);
/* device ids in, caller-owned device buffers of capacity_rows rows out */
int wp_pack_best_fit_device(wp_vocab *v, const int32_t *d_ids, const int64_t *d_row_splits, size_t n_docs,
                            const wp_binpack_spec *spec, const wp_packed *d_out, size_t capacity_rows, size_t *n_out);
int wp_binpack_plan(const int64_t *hist, int32_t max_len, wp_binpack_plan_result *out);
/* The statistics of the last best-fit call, kept beside wp_pack_stats: the first eight as there (n_segments: the units
 * placed), then the runs and row ranges of its plan. */
typedef struct { int64_t n_docs, n_empty, n_cut, n_ids_cut, n_pieces, n_out, n_cells, n_segments, n_runs, n_row_ranges; } wp_binpack_stats;
int wp_get_binpack_stats(const wp_vocab *v, wp_binpack_stats *out); /* n_docs == -1: no such call yet */

#ifdef __cplusplus
}
#endif
#endif
