"""wordpiece_amd — MI355X-native Linear WordPiece (the src/linear.cpp path of gleb-kov/wordpiece).

Host-side mirror of the reference's `word_piece::linear` API on top of the C ABI in
include/wordpiece_amd.h (libwordpiece_amd.so, hand-written HIP for gfx950):

    from wordpiece_amd import linear
    ids = linear.encode("self-made", ["self", "made", "-", "##made"])     # word_piece.hpp:12
    ids = linear.encode("text.txt", "vocab.txt")                           # word_piece.hpp:14
    linear.encodeExternal("text.txt", "vocab.txt", "ids.txt", 500_000_000)  # word_piece.hpp:16

There is no CPU fallback: without the built extension or without a GPU every call raises.
"""
import ctypes as C
import math
import os
import weakref

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# WP_LIB: alternative build of the same library (tuning experiments: profiles/ab.sh)
LIB_PATH = os.environ.get("WP_LIB") or os.path.join(_HERE, "libwordpiece_amd.so")

WP_OPT_FULL_DEPTH, WP_OPT_DEVICE, WP_OPT_KEEP_DEBUG, WP_OPT_STAGE_TIMING, WP_OPT_LCP_KASAI = 1, 2, 3, 4, 5
WP_OPT_COVER_ANCHORS, WP_OPT_ARENA_GUARD, WP_OPT_DEVICES, WP_OPT_VOCAB_IN_S = 7, 8, 9, 10
WP_OPT_SPARSE_EMIT = 11
WP_OPT_INDEXED_ROUND0 = 12
WP_OPT_SORT_BLANKS = 13
WP_OPT_NORMALIZE = 14
WP_OPT_LATE_REFINE = 15
WP_NORM_CLEAN, WP_NORM_LOWER, WP_NORM_STRIP_ACCENTS, WP_NORM_BERT_UNCASED = 1, 2, 4, 7
WP_OFFSETS_BYTES, WP_OFFSETS_CODE_POINTS = 0, 1
_OFFSET_UNITS = {"byte": WP_OFFSETS_BYTES, "char": WP_OFFSETS_CODE_POINTS}
WP_TRUNC_LONGEST_FIRST, WP_TRUNC_ONLY_FIRST, WP_TRUNC_ONLY_SECOND = 0, 1, 2
WP_PACK_NEXT_FIT, WP_PACK_STREAM = 0, 1
WP_PACK_LONG_TRUNCATE, WP_PACK_LONG_SPLIT = 0, 1
WP_PACK_WANT_SEGMENTS, WP_PACK_WANT_POSITIONS, WP_PACK_WANT_SOURCE = 1, 2, 4
WP_ALIGN_LABELS, WP_ALIGN_SPAN_INDEX, WP_ALIGN_POSITIONS = 1, 2, 4
_PACK_MODES = {"next_fit": WP_PACK_NEXT_FIT, "stream": WP_PACK_STREAM}
_PACK_LONG_DOCS = {"truncate": WP_PACK_LONG_TRUNCATE, "split": WP_PACK_LONG_SPLIT}
_PACK_WANT = {"segment_ids": WP_PACK_WANT_SEGMENTS, "position_ids": WP_PACK_WANT_POSITIONS, "source": WP_PACK_WANT_SOURCE}
_TRUNCATIONS = {"longest_first": WP_TRUNC_LONGEST_FIRST, "only_first": WP_TRUNC_ONLY_FIRST,
                "only_second": WP_TRUNC_ONLY_SECOND}

# every symbol include/wordpiece_amd.h declares (checked by the CPU test-suite)
ABI_SYMBOLS = [
    "wp_vocab_create", "wp_vocab_create_packed", "wp_vocab_from_file", "wp_vocab_destroy", "wp_vocab_size",
    "wp_vocab_unk_id", "wp_vocab_token_flags", "wp_vocab_token_len", "wp_linear_encode",
    "wp_linear_encode_device", "wp_linear_encode_file", "wp_linear_encode_external", "wp_set_option",
    "wp_get_stats", "wp_linear_debug_fetch", "wp_free", "wp_last_error", "wp_device_count",
    "wp_linear_encode_multi", "wp_reserve", "wp_fast_encode", "wp_fast_encode_device", "wp_fast_encode_file",
    "wp_fast_encode_external", "wp_vocab_token_utf8", "wp_trim", "wp_linear_encode_batch", "wp_linear_encode_stream",
    "wp_linear_encode_offsets", "wp_linear_encode_offsets_device",
    "wp_linear_encode_rows", "wp_linear_encode_rows_device", "wp_linear_encode_padded", "wp_linear_encode_padded_device",
    "wp_normalize_cp", "wp_normalize_device", "wp_normalize", "wp_get_norm_stats", "wp_get_walk_stats",
    "wp_get_refine_stats", "wp_get_refine_sched", "wp_get_step_stats",
    "wp_linear_encode_inputs", "wp_linear_encode_inputs_device", "wp_get_inputs_stats",
    "wp_word_ids", "wp_word_ids_device", "wp_mlm_mask", "wp_mlm_mask_device", "wp_get_mask_stats",
    "wp_detokenize", "wp_detokenize_device", "wp_detok_piece", "wp_get_detok_stats",
    "wp_pack_sequences", "wp_pack_sequences_device", "wp_get_pack_stats",
    "wp_linear_encode_special", "wp_linear_encode_special_device", "wp_linear_encode_special_rows",
    "wp_linear_encode_special_rows_device", "wp_get_special_stats",
    "wp_align", "wp_align_device", "wp_align_rows", "wp_align_rows_device", "wp_get_align_stats",
    "wp_count_words", "wp_count_words_device", "wp_get_count_stats",
    "wp_learn_vocab", "wp_learn_vocab_device", "wp_get_learn_stats",
    "wp_dedup_rows", "wp_dedup_rows_device", "wp_get_dedup_stats",
    "wp_neardup_rows", "wp_neardup_rows_device", "wp_get_neardup_stats",
    "wp_overlap_rows", "wp_overlap_rows_device", "wp_get_overlap_stats",
    "wp_repeat_rows", "wp_repeat_rows_device", "wp_get_repeat_stats",
    "wp_quality_rows", "wp_quality_rows_device", "wp_get_quality_stats", "wp_quality_class",
]


class WordPieceError(RuntimeError):
    """Mirrors the std::runtime_error the reference throws (message = wp_last_error())."""


class Stats(C.Structure):
    _fields_ = [("n_bytes", C.c_int64), ("n_text", C.c_int64), ("n_total", C.c_int64), ("alphabet", C.c_int64),
                ("longest_token", C.c_int64), ("n_ids", C.c_int64),
                ("symbol_bits", C.c_int32), ("symbols_per_key", C.c_int32), ("rounds", C.c_int32),
                ("sorted_depth", C.c_int32), ("full_depth", C.c_int32),
                ("radix_pass_elems", C.c_int64), ("radix_passes", C.c_int32),
                ("active_per_round", C.c_int64 * 40),
                ("ms_total", C.c_double), ("ms_decode", C.c_double), ("ms_sa", C.c_double), ("ms_lcp", C.c_double),
                ("ms_scan", C.c_double), ("ms_walk", C.c_double), ("ms_radix_scatter", C.c_double),
                ("n_anchors", C.c_int64), ("anchor_mode", C.c_int32), ("ms_h2d", C.c_double), ("ms_d2h", C.c_double),
                ("radix_digit_bytes", C.c_int64), ("ms_host_total", C.c_double), ("guard_zones", C.c_int32),
                ("n_devices", C.c_int32), ("vocab_in_s", C.c_int32), ("reserved0", C.c_int32),
                ("needed_after_round0", C.c_int64), ("key_bits", C.c_int32), ("staged_emit", C.c_int32),
                ("rank_in_pass", C.c_int32), ("trie_refine", C.c_int32), ("arena_bytes", C.c_int64),
                ("list_retries", C.c_int32), ("hist_in_keys", C.c_int32), ("radix_pass_bytes", C.c_int64),
                ("round0_candidates", C.c_int64), ("round0_keys_only", C.c_int32), ("offsets_unit", C.c_int32),
                ("round0_sorted", C.c_int64), ("n_rows", C.c_int64), ("rows_truncated", C.c_int64),
                ("rows_route", C.c_int32)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if k != "active_per_round"}
        d["active_per_round"] = [int(x) for x in self.active_per_round[:max(self.rounds, 0)]]
        return d


class NormStats(C.Structure):
    """wp_norm_stats: WP_OPT_NORMALIZE's part of the statistics (Vocab.stats() merges it into its dict)."""
    _fields_ = [("normalize", C.c_int32), ("norm_bytes", C.c_int64), ("ms_normalize", C.c_double)]


class WalkStats(C.Structure):
    """wp_walk_stats: which variant of the walk produced the ids of the last encode (Vocab.walk_stats())."""
    _fields_ = [("n_wide_words", C.c_int64), ("n_long_words", C.c_int64), ("lean", C.c_int32),
                ("max_anchor_gap", C.c_int32)]


class RefineStats(C.Structure):
    """wp_refine_stats: what the refinement between round 0 and the walk ran on in the last encode (Vocab.refine_stats())."""
    _fields_ = [("n_groups", C.c_int64), ("n_entries", C.c_int64), ("n_large_groups", C.c_int64),
                ("n_large_entries", C.c_int64), ("trie_nodes", C.c_int64), ("sort_bits", C.c_int32),
                ("key_lookup", C.c_int32), ("symbol_bytes", C.c_int32), ("reserved", C.c_int32)]


class RefineSched(C.Structure):
    """wp_refine_sched: where the refinement of the last encode was queued (Vocab.refine_sched())."""
    _fields_ = [("early", C.c_int32), ("reserved", C.c_int32), ("ms_sort_to_scan", C.c_double)]


class StepStats(C.Structure):
    """wp_step_stats: the step tables the walk of the last encode read (Vocab.step_stats())."""
    _fields_ = [("n_marks", C.c_int64), ("n_steps", C.c_int64), ("n_tiles", C.c_int64), ("n_groups_of_tiles", C.c_int64),
                ("bucket_shift", C.c_int32), ("bucket_shift_all", C.c_int32), ("key_shift", C.c_int32),
                ("key_shift_all", C.c_int32), ("packed", C.c_int32), ("key_lookup", C.c_int32)]


class InputsSpec(C.Structure):
    """wp_inputs_spec: the arguments of an inputs call."""
    _fields_ = [("max_len", C.c_int32), ("cls_id", C.c_int32), ("sep_id", C.c_int32), ("pad_id", C.c_int32),
                ("pairs", C.c_int32), ("truncation", C.c_int32), ("stride", C.c_int32), ("unit", C.c_int32)]


class Inputs(C.Structure):
    """wp_inputs: the five blocks of a batch of model inputs (host blocks out, or caller-owned device buffers in)."""
    _fields_ = [("input_ids", C.c_void_p), ("token_type_ids", C.c_void_p), ("lengths", C.c_void_p), ("sample", C.c_void_p),
                ("offsets", C.c_void_p)]


class InputsStats(C.Structure):
    """wp_inputs_stats: the model-inputs part of the statistics of the last call (Vocab.inputs_stats())."""
    _fields_ = [("n_samples", C.c_int64), ("n_out", C.c_int64), ("n_cut", C.c_int64), ("n_windowed", C.c_int64),
                ("pairs", C.c_int32), ("truncation", C.c_int32), ("stride", C.c_int32), ("reserved", C.c_int32)]


class MaskSpec(C.Structure):
    """wp_mask_spec: the arguments of a mask or word-ids call (probabilities as q32: p * 2^32, see q32())."""
    _fields_ = [("max_len", C.c_int32), ("cls_id", C.c_int32), ("sep_id", C.c_int32), ("pad_id", C.c_int32),
                ("mask_id", C.c_int32), ("ignore_id", C.c_int32), ("whole_word", C.c_int32), ("reserved", C.c_int32),
                ("select_q32", C.c_uint64), ("mask_q32", C.c_uint64), ("random_q32", C.c_uint64), ("seed", C.c_uint64),
                ("row_base", C.c_uint64)]


class MaskStats(C.Structure):
    """wp_mask_stats: the statistics of the last mask or word-ids call (Vocab.mask_stats())."""
    _fields_ = [("n_rows", C.c_int64), ("n_words", C.c_int64), ("n_selected", C.c_int64), ("n_selected_units", C.c_int64),
                ("n_masked", C.c_int64), ("n_random", C.c_int64), ("n_kept", C.c_int64), ("whole_word", C.c_int32),
                ("reserved", C.c_int32)]


class DetokSpec(C.Structure):
    """wp_detok_spec: the arguments of a detokenize call (max_len 0: ragged rows; terminator -1: none)."""
    _fields_ = [("max_len", C.c_int32), ("cleanup", C.c_int32), ("terminator", C.c_int32), ("n_skip", C.c_int32),
                ("skip_ids", C.c_int32 * 8)]


class DetokStats(C.Structure):
    """wp_detok_stats: the statistics of the last detokenize call (Vocab.detok_stats())."""
    _fields_ = [("n_rows", C.c_int64), ("n_cells", C.c_int64), ("n_kept", C.c_int64), ("n_skipped", C.c_int64),
                ("n_dropped", C.c_int64), ("n_bytes", C.c_int64)]


class PackSpec(C.Structure):
    """wp_pack_spec: the arguments of a pack call (bos_id / eos_id -1: none)."""
    _fields_ = [("max_len", C.c_int32), ("mode", C.c_int32), ("bos_id", C.c_int32), ("eos_id", C.c_int32),
                ("pad_id", C.c_int32), ("long_docs", C.c_int32), ("want", C.c_int32), ("reserved", C.c_int32)]


class Packed(C.Structure):
    """wp_packed: the five blocks of a packed batch (host blocks out, or caller-owned device buffers in)."""
    _fields_ = [("input_ids", C.c_void_p), ("segment_ids", C.c_void_p), ("position_ids", C.c_void_p), ("source", C.c_void_p),
                ("lengths", C.c_void_p)]


class PackStats(C.Structure):
    """wp_pack_stats: the statistics of the last pack call (Vocab.pack_stats())."""
    _fields_ = [("n_docs", C.c_int64), ("n_empty", C.c_int64), ("n_cut", C.c_int64), ("n_ids_cut", C.c_int64),
                ("n_pieces", C.c_int64), ("n_out", C.c_int64), ("n_cells", C.c_int64), ("n_segments", C.c_int64)]


class SpecialSpec(C.Structure):
    """wp_special_spec: the listed ids of a special-tokens call (host memory)."""
    _fields_ = [("ids", C.POINTER(C.c_int32)), ("n_ids", C.c_int32)]


class SpecialStats(C.Structure):
    """wp_special_stats: the statistics of the last special-tokens call (Vocab.special_stats())."""
    _fields_ = [("n_literals", C.c_int64), ("n_ids", C.c_int64), ("n_rows", C.c_int64), ("n_listed", C.c_int64)]


class AlignSpec(C.Structure):
    """wp_align_spec: the arguments of an align call (want: WP_ALIGN_* bits, read by the host entry points)."""
    _fields_ = [("max_len", C.c_int32), ("side", C.c_int32), ("outside_label", C.c_int32), ("inside_add", C.c_int32),
                ("ignore_id", C.c_int32), ("no_answer", C.c_int32), ("want", C.c_int32), ("reserved", C.c_int32)]


class AlignStats(C.Structure):
    """wp_align_stats: the statistics of the last align call (Vocab.align_stats())."""
    _fields_ = [("n_rows", C.c_int64), ("n_tokens", C.c_int64), ("n_covered", C.c_int64), ("n_begin", C.c_int64),
                ("n_spans", C.c_int64), ("n_answer_rows", C.c_int64), ("n_no_answer_rows", C.c_int64)]


WP_COUNT_ORDER_FIRST, WP_COUNT_ORDER_COUNT = 0, 1
WP_COUNT_WANT_INDEX = 1
_COUNT_ORDERS = {"first": WP_COUNT_ORDER_FIRST, "count": WP_COUNT_ORDER_COUNT}


class CountSpec(C.Structure):
    """wp_count_spec: the arguments of a count call (want: WP_COUNT_WANT_* bits; hash_bits 0: 64)."""
    _fields_ = [("order", C.c_int32), ("max_word_bytes", C.c_int32), ("terminator", C.c_int32), ("want", C.c_int32),
                ("hash_bits", C.c_int32), ("reserved", C.c_int32), ("min_count", C.c_int64)]


class WordCounts(C.Structure):
    """wp_word_counts: the table of a count call (host blocks, or device memory owned by the handle)."""
    _fields_ = [("words", C.c_void_p), ("word_off", C.c_void_p), ("counts", C.c_void_p), ("word_index", C.c_void_p),
                ("n_distinct", C.c_int64), ("n_words", C.c_int64), ("n_bytes", C.c_int64)]


class CountStats(C.Structure):
    """wp_count_stats: the statistics of the last count call (Vocab.count_stats())."""
    _fields_ = [("n_words", C.c_int64), ("n_distinct", C.c_int64), ("n_long", C.c_int64), ("n_below_min", C.c_int64),
                ("n_text_bytes", C.c_int64), ("n_rounds", C.c_int64), ("n_collided", C.c_int64)]


DEFAULT_RESERVED = ("[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]")


class LearnSpec(C.Structure):
    """wp_learn_spec: the arguments of a learn call (slack: a number of entries; hash_bits 0: 64)."""
    _fields_ = [("reserved_tokens", C.c_char_p), ("reserved_off", C.POINTER(C.c_int64)), ("n_reserved", C.c_int64),
                ("vocab_size", C.c_int64), ("lower_thresh", C.c_int64), ("upper_thresh", C.c_int64), ("slack", C.c_int64),
                ("num_iterations", C.c_int32), ("max_token_chars", C.c_int32), ("max_unique_chars", C.c_int32),
                ("terminator", C.c_int32), ("hash_bits", C.c_int32), ("reserved", C.c_int32)]


class LearnedVocab(C.Structure):
    """wp_learned_vocab: the list of a learn call (host blocks, or device memory owned by the handle)."""
    _fields_ = [("tokens", C.c_void_p), ("token_off", C.c_void_p), ("scores", C.c_void_p), ("n_tokens", C.c_int64),
                ("n_bytes", C.c_int64), ("thresh", C.c_int64)]


class LearnStats(C.Structure):
    """wp_learn_stats: the statistics of the last learn call (Vocab.learn_stats())."""
    _fields_ = [("n_words", C.c_int64), ("n_reserved", C.c_int64), ("n_long", C.c_int64), ("n_char_dropped", C.c_int64),
                ("n_chars", C.c_int64), ("n_occurrences", C.c_int64), ("n_tokens", C.c_int64), ("n_steps", C.c_int64),
                ("thresh", C.c_int64), ("n_rounds", C.c_int64), ("n_collided", C.c_int64)]


WP_DEDUP_WANT_INVERSE = 1
WP_DEDUP_WANT_COMPACT = 2


class DedupSpec(C.Structure):
    """wp_dedup_spec: the arguments of a dedup call (elem_bytes 1: text, 4: ids; hash_bits 0: 64)."""
    _fields_ = [("elem_bytes", C.c_int32), ("want", C.c_int32), ("hash_bits", C.c_int32), ("reserved", C.c_int32)]


class DedupResult(C.Structure):
    """wp_dedup_result: the arrays of a dedup call (host blocks, or device memory owned by the handle)."""
    _fields_ = [("first", C.c_void_p), ("kept", C.c_void_p), ("inverse", C.c_void_p), ("counts", C.c_void_p), ("row_off", C.c_void_p),
                ("data", C.c_void_p), ("n_rows", C.c_int64), ("n_unique", C.c_int64), ("n_elems", C.c_int64)]


class DedupStats(C.Structure):
    """wp_dedup_stats: the statistics of the last dedup call (Vocab.dedup_stats())."""
    _fields_ = [("n_rows", C.c_int64), ("n_unique", C.c_int64), ("n_empty", C.c_int64), ("n_elems", C.c_int64), ("n_chunks", C.c_int64),
                ("n_compared", C.c_int64), ("n_rounds", C.c_int64), ("n_collided", C.c_int64)]


WP_NEARDUP_WANT_INVERSE = 1
WP_NEARDUP_WANT_COMPACT = 2
WP_NEARDUP_WANT_SIGNATURES = 4


class NearDupSpec(C.Structure):
    """wp_neardup_spec: the arguments of a neardup call (elem_bytes 1: text, 4: ids; shingle: elements per shingle)."""
    _fields_ = [("elem_bytes", C.c_int32), ("want", C.c_int32), ("shingle", C.c_int32), ("n_perm", C.c_int32), ("bands", C.c_int32),
                ("min_agree", C.c_int32), ("seed", C.c_uint64), ("reserved", C.c_int32 * 2)]


class NearDupResult(C.Structure):
    """wp_neardup_result: the arrays of a neardup call (host blocks, or device memory owned by the handle)."""
    _fields_ = [("cluster", C.c_void_p), ("kept", C.c_void_p), ("inverse", C.c_void_p), ("counts", C.c_void_p), ("row_off", C.c_void_p),
                ("data", C.c_void_p), ("signatures", C.c_void_p), ("n_rows", C.c_int64), ("n_unique", C.c_int64), ("n_elems", C.c_int64),
                ("n_perm", C.c_int64)]


class NearDupStats(C.Structure):
    """wp_neardup_stats: the statistics of the last neardup call (Vocab.neardup_stats())."""
    _fields_ = [("n_rows", C.c_int64), ("n_unique", C.c_int64), ("n_empty", C.c_int64), ("n_elems", C.c_int64), ("n_shingles", C.c_int64),
                ("n_buckets", C.c_int64), ("n_candidates", C.c_int64), ("n_edges", C.c_int64), ("n_rounds", C.c_int64)]


WP_OVERLAP_WANT_MASK = 1
WP_OVERLAP_WANT_REF = 2
WP_OVERLAP_WANT_COMPACT = 4


class OverlapSpec(C.Structure):
    """wp_overlap_spec: the arguments of an overlap call (elem_bytes 1: text, 4: ids; ngram: elements per window)."""
    _fields_ = [("elem_bytes", C.c_int32), ("want", C.c_int32), ("ngram", C.c_int32), ("max_hits", C.c_int32), ("hash_bits", C.c_int32),
                ("reserved", C.c_int32 * 3)]


class OverlapResult(C.Structure):
    """wp_overlap_result: the arrays of an overlap call (host blocks, or device memory owned by the handle)."""
    _fields_ = [("hits", C.c_void_p), ("first_hit", C.c_void_p), ("covered", C.c_void_p), ("ref_hits", C.c_void_p), ("row_off", C.c_void_p),
                ("first_ref", C.c_void_p), ("kept", C.c_void_p), ("mask", C.c_void_p), ("data", C.c_void_p), ("n_rows", C.c_int64),
                ("n_ref", C.c_int64), ("n_kept", C.c_int64), ("n_elems", C.c_int64)]


class OverlapStats(C.Structure):
    """wp_overlap_stats: the statistics of the last overlap call (Vocab.overlap_stats())."""
    _fields_ = [("n_rows", C.c_int64), ("n_ref", C.c_int64), ("n_elems", C.c_int64), ("n_ref_elems", C.c_int64), ("n_windows", C.c_int64),
                ("n_ref_windows", C.c_int64), ("n_ref_distinct", C.c_int64), ("n_hits", C.c_int64), ("n_hit_rows", C.c_int64),
                ("n_covered", C.c_int64), ("n_candidates", C.c_int64), ("n_collided", C.c_int64)]


WP_REPEAT_WANT_MASK = 1
WP_REPEAT_WANT_SRC = 2
WP_REPEAT_WANT_COMPACT = 4
WP_REPEAT_WANT_CUT = 8
WP_REPEAT_UTF8 = 1


class RepeatSpec(C.Structure):
    """wp_repeat_spec: the arguments of a repeat call (elem_bytes 1: text, 4: ids; ngram: elements per window; scope 0:
    anywhere, 1: earlier rows only; flags: WP_REPEAT_UTF8)."""
    _fields_ = [("elem_bytes", C.c_int32), ("want", C.c_int32), ("ngram", C.c_int32), ("scope", C.c_int32), ("max_repeats", C.c_int32),
                ("hash_bits", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32)]


class RepeatResult(C.Structure):
    """wp_repeat_result: the arrays of a repeat call (host blocks, or device memory owned by the handle)."""
    _fields_ = [("repeats", C.c_void_p), ("first_repeat", C.c_void_p), ("first_src_pos", C.c_void_p), ("covered", C.c_void_p), ("src", C.c_void_p),
                ("row_off", C.c_void_p), ("cut_off", C.c_void_p), ("first_src_row", C.c_void_p), ("kept", C.c_void_p), ("mask", C.c_void_p),
                ("data", C.c_void_p), ("cut_data", C.c_void_p), ("n_rows", C.c_int64), ("n_kept", C.c_int64), ("n_elems", C.c_int64),
                ("n_cut_elems", C.c_int64)]


class RepeatStats(C.Structure):
    """wp_repeat_stats: the statistics of the last repeat call (Vocab.repeat_stats())."""
    _fields_ = [("n_rows", C.c_int64), ("n_elems", C.c_int64), ("n_windows", C.c_int64), ("n_distinct", C.c_int64), ("n_repeats", C.c_int64),
                ("n_repeat_rows", C.c_int64), ("n_covered", C.c_int64), ("n_cut_elems", C.c_int64), ("n_collided", C.c_int64)]


WP_QUALITY_WANT_DUP_LINES = 1
WP_QUALITY_WANT_COMPACT = 2
# the signals and the rules of a quality call, by index (WP_QS_*, WP_QR_*)
QUALITY_SIGNALS = ("bytes", "chars", "invalid", "space_chars", "alpha_chars", "digit_chars", "upper_chars", "punct_chars", "words", "text_words",
                   "text_word_chars", "alpha_words", "stop_words", "hashes", "ellipses", "newlines", "lines", "bullet_lines", "ellipsis_lines",
                   "terminal_lines", "short_lines", "dup_lines", "dup_line_chars")
QUALITY_RULES = ("min_text_words", "max_text_words", "min_mean_word_x1000", "max_mean_word_x1000", "max_hash_per_word", "max_ellipsis_per_word",
                 "max_bullet_lines", "max_ellipsis_lines", "min_alpha_words", "min_stop_words", "max_dup_lines", "max_dup_line_chars",
                 "min_terminal_lines", "max_short_lines", "max_newlines_per_word", "reserved")
_QUALITY_PRESETS = {
    # the thresholds of the MassiveText (Gopher) quality and repetition filters, over this library's words and lines
    "gopher": dict(min_text_words=50, max_text_words=100000, min_mean_word_x1000=3000, max_mean_word_x1000=10000, max_hash_per_word=100,
                   max_ellipsis_per_word=100, max_bullet_lines=900, max_ellipsis_lines=300, min_alpha_words=800, min_stop_words=2,
                   max_dup_lines=300, max_dup_line_chars=200, stop_words=("the", "be", "to", "of", "and", "that", "have", "with")),
    # the thresholds of FineWeb's custom filters
    "fineweb": dict(min_terminal_lines=120, max_short_lines=670, max_dup_line_chars=10, max_newlines_per_word=300),
}


def quality_rules(name):
    """The rules of a published pipeline as keyword arguments of the quality calls: "gopher" or "fineweb".  They are those
    papers' thresholds over THIS library's words and lines; parity with another tokeniser's word count is not claimed."""
    if name not in _QUALITY_PRESETS:
        raise WordPieceError("quality: no such preset: %r (known: %s)" % (name, ", ".join(sorted(_QUALITY_PRESETS))))
    return dict(_QUALITY_PRESETS[name])


class QualitySpec(C.Structure):
    """wp_quality_spec: the arguments of a quality call (want: WP_QUALITY_WANT_*; limit: -1 or the threshold of rule r)."""
    _fields_ = [("elem_bytes", C.c_int32), ("want", C.c_int32), ("short_line_chars", C.c_int32), ("n_stop_words", C.c_int32),
                ("stop_pool", C.c_void_p), ("stop_off", C.c_void_p), ("limit", C.c_int64 * 16), ("reserved", C.c_int64)]


class QualityResult(C.Structure):
    """wp_quality_result: the arrays of a quality call (host blocks, or device memory owned by the handle)."""
    _fields_ = [("signals", C.c_void_p), ("row_off", C.c_void_p), ("reasons", C.c_void_p), ("kept", C.c_void_p), ("data", C.c_void_p),
                ("n_rows", C.c_int64), ("n_kept", C.c_int64), ("n_elems", C.c_int64)]


class QualityStats(C.Structure):
    """wp_quality_stats: the statistics of the last quality call (Vocab.quality_stats())."""
    _fields_ = [("n_rows", C.c_int64), ("n_bytes", C.c_int64), ("n_chars", C.c_int64), ("n_invalid", C.c_int64), ("n_words", C.c_int64),
                ("n_lines", C.c_int64), ("n_dup_lines", C.c_int64), ("n_kept", C.c_int64), ("rule_failed", C.c_int64 * 16)]


def lsh_min_agree(threshold, n_perm):
    """The min_agree that stands for a Jaccard threshold: ceil(threshold * n_perm) signature slots."""
    return int(math.ceil(threshold * n_perm))


# ---- the corpus layers as data ("The Python side of a corpus layer") -------------------------------------------
_BATCH = [C.c_void_p, C.c_void_p, C.c_size_t]  # data, offsets, n_rows
# layer: (host entry point ("_device": its twin), Spec, Result, Stats, what stands between the handle and the spec: host, device)
_CORPUS_LAYERS = {
    "count": ("wp_count_words", CountSpec, WordCounts, CountStats, [C.c_char_p, C.c_size_t], [C.c_void_p, C.c_size_t]),
    "learn": ("wp_learn_vocab", LearnSpec, LearnedVocab, LearnStats, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t],
              [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t]),
    "dedup": ("wp_dedup_rows", DedupSpec, DedupResult, DedupStats, _BATCH, _BATCH),
    "neardup": ("wp_neardup_rows", NearDupSpec, NearDupResult, NearDupStats, _BATCH, _BATCH),
    "overlap": ("wp_overlap_rows", OverlapSpec, OverlapResult, OverlapStats, _BATCH * 2, _BATCH * 2),
    "repeat": ("wp_repeat_rows", RepeatSpec, RepeatResult, RepeatStats, _BATCH, _BATCH),
    "quality": ("wp_quality_rows", QualitySpec, QualityResult, QualityStats, _BATCH, _BATCH),
}
# element kind: (numpy dtype of a host result, typestr and torch dtype of a device result)
_KINDS = {"u8": (np.uint8, "|u1", "uint8"), "i32": (np.int32, "<i4", "int32"), "i64": (np.int64, "<i8", "int64"),
          "u32": (np.uint32, "<i4", "int32")}  # (torch has no uint32 arithmetic: the device form gives the bit patterns as int32)
# The arrays of a layer's result, in the order of the dict: (key = field of the Result struct, element kind, shape, the
# keyword that switches it on).  Kinds beside _KINDS: "elem", the batch's own, and "off", int64 offsets with one entry
# more than the shape says.  A size is a count field of the struct, or "rows" / "ref" (the rows of the batch / of the
# reference), "elems" (the elements of the batch), "n_perm", "n_signals".
_RESULTS = {
    "count": (("words", "u8", ("n_bytes",), None), ("word_off", "off", ("n_distinct",), None), ("counts", "i64", ("n_distinct",), None),
              ("word_index", "i32", ("n_words",), "index")),
    "learn": (("tokens", "u8", ("n_bytes",), None), ("token_off", "off", ("n_tokens",), None), ("scores", "i64", ("n_tokens",), None)),
    "dedup": (("first", "i32", ("rows",), None), ("kept", "i32", ("n_unique",), None), ("counts", "i64", ("n_unique",), None),
              ("inverse", "i32", ("rows",), "inverse"), ("data", "elem", ("n_elems",), "compact"), ("row_off", "off", ("n_unique",), "compact")),
    "neardup": (("cluster", "i32", ("rows",), None), ("kept", "i32", ("n_unique",), None), ("counts", "i64", ("n_unique",), None),
                ("inverse", "i32", ("rows",), "inverse"), ("data", "elem", ("n_elems",), "compact"), ("row_off", "off", ("n_unique",), "compact"),
                ("signatures", "u32", ("rows", "n_perm"), "signatures")),
    "overlap": (("hits", "i64", ("rows",), None), ("first_hit", "i64", ("rows",), None), ("first_ref", "i32", ("rows",), None),
                ("covered", "i64", ("rows",), None), ("mask", "u8", ("elems",), "mask"), ("ref_hits", "i64", ("ref",), "ref"),
                ("kept", "i32", ("n_kept",), "compact"), ("data", "elem", ("n_elems",), "compact"), ("row_off", "off", ("n_kept",), "compact")),
    "repeat": (("repeats", "i64", ("rows",), None), ("first_repeat", "i64", ("rows",), None), ("first_src_row", "i32", ("rows",), None),
               ("first_src_pos", "i64", ("rows",), None), ("covered", "i64", ("rows",), None), ("mask", "u8", ("elems",), "mask"),
               ("src", "i64", ("elems",), "src"), ("kept", "i32", ("n_kept",), "compact"), ("data", "elem", ("n_elems",), "compact"),
               ("row_off", "off", ("n_kept",), "compact"), ("cut_data", "elem", ("n_cut_elems",), "cut"), ("cut_off", "off", ("rows",), "cut")),
    "quality": (("signals", "i64", ("n_signals", "rows"), None), ("reasons", "u32", ("rows",), None), ("kept", "i32", ("n_kept",), "compact"),
                ("data", "elem", ("n_elems",), "compact"), ("row_off", "off", ("n_kept",), "compact")),
}

_TEXT_SOURCE = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t))
_IDS_SINK = C.CFUNCTYPE(None, C.c_void_p, C.c_size_t, C.POINTER(C.c_int32), C.c_size_t)

_lib = None


def lib():
    """Loads the HIP extension; fails loudly if it has not been built (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise WordPieceError("HIP extension missing: %s (run `python -m wordpiece_amd.build`)" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        vp, i32p = C.c_void_p, C.POINTER(C.c_int32)
        L.wp_vocab_create.argtypes = [C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_size_t, C.POINTER(vp)]
        L.wp_vocab_create_packed.argtypes = [C.c_char_p, C.POINTER(C.c_int64), C.c_int64, C.POINTER(vp)]
        L.wp_vocab_from_file.argtypes = [C.c_char_p, C.POINTER(vp)]
        L.wp_vocab_destroy.argtypes = [vp]
        L.wp_vocab_destroy.restype = None
        L.wp_vocab_size.argtypes = [vp]
        L.wp_vocab_size.restype = C.c_int64
        L.wp_vocab_unk_id.argtypes = [vp]
        L.wp_vocab_unk_id.restype = C.c_int32
        L.wp_vocab_token_flags.argtypes = [vp, C.c_int64]
        L.wp_vocab_token_flags.restype = C.c_int32
        L.wp_vocab_token_len.argtypes = [vp, C.c_int64]
        L.wp_vocab_token_len.restype = C.c_int64
        L.wp_linear_encode.argtypes = [vp, C.c_char_p, C.c_size_t, C.POINTER(i32p), C.POINTER(C.c_size_t)]
        L.wp_linear_encode_device.argtypes = [vp, vp, C.c_size_t, C.POINTER(vp), C.POINTER(C.c_size_t)]
        u32p = C.POINTER(C.c_uint32)
        L.wp_linear_encode_offsets.argtypes = [vp, C.c_char_p, C.c_size_t, C.c_int, C.POINTER(i32p), C.POINTER(u32p),
                                               C.POINTER(C.c_size_t)]
        L.wp_linear_encode_offsets_device.argtypes = [vp, vp, C.c_size_t, C.c_int, C.POINTER(vp), C.POINTER(vp),
                                                      C.POINTER(C.c_size_t)]
        i64p = C.POINTER(C.c_int64)
        L.wp_linear_encode_rows.argtypes = [vp, C.c_char_p, C.c_size_t, i64p, C.c_size_t, C.c_int, C.POINTER(i32p),
                                            C.POINTER(i64p), C.POINTER(u32p), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
        L.wp_linear_encode_rows_device.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, C.c_int, C.POINTER(vp), C.POINTER(vp),
                                                   C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
        L.wp_linear_encode_padded.argtypes = [vp, C.c_char_p, C.c_size_t, i64p, C.c_size_t, C.c_int, C.c_int32, C.c_int32,
                                              C.c_int32, C.POINTER(i32p), C.POINTER(i32p), C.POINTER(C.c_size_t)]
        L.wp_linear_encode_padded_device.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, C.c_int, C.c_int32, C.c_int32,
                                                     C.c_int32, vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
        L.wp_linear_encode_inputs.argtypes = [vp, C.c_char_p, C.c_size_t, i64p, C.c_size_t, C.POINTER(InputsSpec),
                                              C.POINTER(Inputs), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
        L.wp_linear_encode_inputs_device.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, C.POINTER(InputsSpec),
                                                     C.POINTER(Inputs), C.c_size_t, C.POINTER(C.c_size_t),
                                                     C.POINTER(C.c_size_t)]
        L.wp_get_inputs_stats.argtypes = [vp, C.POINTER(InputsStats)]
        L.wp_word_ids.argtypes = [vp, i32p, i32p, C.c_size_t, C.POINTER(MaskSpec), C.POINTER(i32p)]
        L.wp_word_ids_device.argtypes = [vp, vp, vp, C.c_size_t, C.POINTER(MaskSpec), vp]
        L.wp_mlm_mask.argtypes = [vp, i32p, i32p, C.c_size_t, C.POINTER(MaskSpec), C.POINTER(i32p), C.POINTER(i32p),
                                  C.POINTER(i32p)]
        L.wp_mlm_mask_device.argtypes = [vp, vp, vp, C.c_size_t, C.POINTER(MaskSpec), vp, vp, vp]
        L.wp_get_mask_stats.argtypes = [vp, C.POINTER(MaskStats)]
        L.wp_detokenize.argtypes = [vp, i32p, C.POINTER(C.c_int64), i32p, C.c_size_t, C.POINTER(DetokSpec),
                                    C.POINTER(C.c_void_p), C.POINTER(C.POINTER(C.c_int64)), C.POINTER(C.c_size_t)]
        L.wp_detokenize_device.argtypes = [vp, vp, vp, vp, C.c_size_t, C.POINTER(DetokSpec), C.POINTER(C.c_void_p),
                                           C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
        L.wp_detok_piece.argtypes = [vp, C.c_int64, C.c_int, C.c_int, C.c_char_p, C.c_size_t]
        L.wp_detok_piece.restype = C.c_int64
        L.wp_get_detok_stats.argtypes = [vp, C.POINTER(DetokStats)]
        if hasattr(L, "wp_pack_sequences"):  # (WP_LIB may name a build from before the call: A/B runs against a parent)
            L.wp_pack_sequences.argtypes = [vp, i32p, i64p, C.c_size_t, C.POINTER(PackSpec), C.POINTER(Packed),
                                            C.POINTER(C.c_size_t)]
            L.wp_pack_sequences_device.argtypes = [vp, vp, vp, C.c_size_t, C.POINTER(PackSpec), C.POINTER(Packed), C.c_size_t,
                                                   C.POINTER(C.c_size_t)]
            L.wp_get_pack_stats.argtypes = [vp, C.POINTER(PackStats)]
        if hasattr(L, "wp_linear_encode_special"):  # (WP_LIB, as above)
            sp = C.POINTER(SpecialSpec)
            L.wp_linear_encode_special.argtypes = [vp, C.c_char_p, C.c_size_t, sp, C.c_int, C.POINTER(i32p), C.POINTER(u32p),
                                                   C.POINTER(C.c_size_t)]
            L.wp_linear_encode_special_device.argtypes = [vp, vp, C.c_size_t, sp, C.c_int, C.POINTER(vp), C.POINTER(vp),
                                                          C.POINTER(C.c_size_t)]
            L.wp_linear_encode_special_rows.argtypes = [vp, C.c_char_p, C.c_size_t, i64p, C.c_size_t, sp, C.c_int, C.POINTER(i32p),
                                                        C.POINTER(i64p), C.POINTER(u32p), C.POINTER(C.c_size_t),
                                                        C.POINTER(C.c_size_t)]
            L.wp_linear_encode_special_rows_device.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, sp, C.c_int, C.POINTER(vp),
                                                               C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_size_t),
                                                               C.POINTER(C.c_size_t)]
            L.wp_get_special_stats.argtypes = [vp, C.POINTER(SpecialStats)]
        if hasattr(L, "wp_align"):  # (WP_LIB, as above)
            ap = C.POINTER(AlignSpec)
            L.wp_align.argtypes = [vp, u32p, i32p, i32p, i32p, C.c_size_t, i64p, C.c_size_t, u32p, i32p, C.c_size_t, ap,
                                   C.POINTER(i32p), C.POINTER(i32p), C.POINTER(i32p), C.POINTER(i32p)]
            L.wp_align_device.argtypes = [vp, vp, vp, vp, vp, C.c_size_t, vp, C.c_size_t, vp, vp, C.c_size_t, ap, vp, vp, vp, vp]
            L.wp_align_rows.argtypes = [vp, u32p, i64p, C.c_size_t, i64p, u32p, i32p, C.c_size_t, ap, C.POINTER(i32p),
                                        C.POINTER(i32p)]
            L.wp_align_rows_device.argtypes = [vp, vp, vp, C.c_size_t, C.c_size_t, vp, vp, vp, C.c_size_t, ap, vp, vp]
            L.wp_get_align_stats.argtypes = [vp, C.POINTER(AlignStats)]
        for layer, (fn, spec, result, stats, host_args, device_args) in _CORPUS_LAYERS.items():
            if hasattr(L, fn):  # (WP_LIB, as above)
                getattr(L, fn).argtypes = [vp] + host_args + [C.POINTER(spec), C.POINTER(result)]
                getattr(L, fn + "_device").argtypes = [vp] + device_args + [C.POINTER(spec), C.POINTER(result)]
                getattr(L, "wp_get_%s_stats" % layer).argtypes = [vp, C.POINTER(stats)]
        if hasattr(L, "wp_quality_class"):  # (WP_LIB, as above)
            L.wp_quality_class.argtypes = [C.c_uint32]
            L.wp_quality_class.restype = C.c_int32
        L.wp_linear_encode_multi.argtypes = [vp, C.c_char_p, C.c_size_t, C.POINTER(C.c_int), C.c_int, C.POINTER(i32p),
                                             C.POINTER(C.c_size_t)]
        L.wp_reserve.argtypes = [vp, C.c_size_t]
        L.wp_linear_encode_stream.argtypes = [vp, _TEXT_SOURCE, _IDS_SINK, vp]
        L.wp_linear_encode_batch.argtypes = [vp, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_size_t, C.POINTER(i32p),
                                             C.POINTER(C.c_size_t)]
        L.wp_trim.argtypes = [vp]
        L.wp_fast_encode.argtypes = [vp, C.c_char_p, C.c_size_t, C.POINTER(i32p), C.POINTER(C.c_size_t)]
        L.wp_fast_encode_device.argtypes = [vp, vp, C.c_size_t, C.POINTER(vp), C.POINTER(C.c_size_t)]
        L.wp_fast_encode_file.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(i32p), C.POINTER(C.c_size_t)]
        L.wp_fast_encode_external.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_size_t]
        L.wp_vocab_token_utf8.argtypes = [vp, C.c_int64, C.c_char_p, C.c_size_t]
        L.wp_vocab_token_utf8.restype = C.c_int64
        L.wp_linear_encode_file.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(i32p), C.POINTER(C.c_size_t)]
        L.wp_linear_encode_external.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_size_t]
        L.wp_normalize_cp.argtypes = [C.c_int, C.c_uint32, C.POINTER(C.c_uint32)]
        L.wp_normalize_device.argtypes = [vp, vp, C.c_size_t, C.c_int, C.POINTER(vp), C.POINTER(C.c_size_t)]
        L.wp_normalize.argtypes = [vp, C.c_char_p, C.c_size_t, C.c_int, C.POINTER(vp), C.POINTER(C.c_size_t)]
        L.wp_set_option.argtypes = [vp, C.c_int, C.c_int64]
        L.wp_get_stats.argtypes = [vp, C.POINTER(Stats)]
        L.wp_get_norm_stats.argtypes = [vp, C.POINTER(NormStats)]
        L.wp_get_walk_stats.argtypes = [vp, C.POINTER(WalkStats)]
        L.wp_get_refine_stats.argtypes = [vp, C.POINTER(RefineStats)]
        if hasattr(L, "wp_get_refine_sched"):  # (WP_LIB may name a build from before the struct: A/B runs against a parent)
            L.wp_get_refine_sched.argtypes = [vp, C.POINTER(RefineSched)]
        if hasattr(L, "wp_get_step_stats"):
            L.wp_get_step_stats.argtypes = [vp, C.POINTER(StepStats)]
        L.wp_linear_debug_fetch.argtypes = [vp, C.c_int, i32p, C.c_size_t, C.POINTER(C.c_size_t)]
        L.wp_free.argtypes = [vp]
        L.wp_free.restype = None
        L.wp_last_error.restype = C.c_char_p
        L.wp_device_count.restype = C.c_int
        _lib = L
    return _lib


def _check(rc):
    if rc != 0:
        raise WordPieceError(lib().wp_last_error().decode("utf8", "replace"))


def _bytes(x):
    return bytes(x) if isinstance(x, (bytes, bytearray, memoryview)) else x.encode("utf8")


class Vocab:
    """Opaque vocabulary handle (wp_vocab): parsed like utils.cpp:81-137, cached on the device."""

    def __init__(self, lines=None, file=None, device=None, normalize=0):
        self._h = C.c_void_p()
        if file is not None:
            _check(lib().wp_vocab_from_file(_bytes(file), C.byref(self._h)))
        else:
            ls = [_bytes(w) for w in lines]
            off = _offsets_of([len(w) for w in ls])
            _check(lib().wp_vocab_create_packed(b"".join(ls), off.ctypes.data_as(C.POINTER(C.c_int64)), len(ls),
                                                C.byref(self._h)))
        self._device = None if device is None else int(device)  # (None: the device that is current at the first call)
        if device is not None:
            self.set_option(WP_OPT_DEVICE, device)
        if normalize:  # WP_NORM_* flags: every encode of this handle normalises its text on the device first
            self.set_option(WP_OPT_NORMALIZE, normalize)
        self._normalize = int(normalize)

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.wp_vocab_destroy(self._h)
            self._h = None

    def __len__(self):
        return lib().wp_vocab_size(self._h)

    @property
    def unk_id(self):
        return lib().wp_vocab_unk_id(self._h)

    def token_flags(self, i):
        return lib().wp_vocab_token_flags(self._h, i)

    def token_len(self, i):
        return lib().wp_vocab_token_len(self._h, i)

    def set_option(self, opt, value):
        _check(lib().wp_set_option(self._h, opt, int(value)))
        if opt == WP_OPT_NORMALIZE:
            self._normalize = int(value)
        if opt == WP_OPT_DEVICE:
            self._device = int(value)

    def normalize(self, text, flags=None):
        """The normalisation pre-pass alone (wp_normalize): host UTF-8 bytes/str -> the normalised UTF-8 as bytes.
        flags: WP_NORM_* (default: the handle's WP_OPT_NORMALIZE)."""
        b = _bytes(text)
        out = C.c_void_p()
        n = C.c_size_t()
        _check(lib().wp_normalize(self._h, b, len(b), self._normalize if flags is None else int(flags), C.byref(out), C.byref(n)))
        if n.value == 0:
            return b""
        try:
            return C.string_at(out, n.value)
        finally:
            lib().wp_free(out)

    def normalize_tensor(self, text, flags=None, copy=True):
        """The pre-pass alone on a uint8 text tensor on this handle's GPU (wp_normalize_device) -> a uint8 tensor there.
        copy=False: a view of the library's buffer, valid until the next call on this handle."""
        import torch
        if text.dtype != torch.uint8 or not text.is_cuda or not text.is_contiguous():
            raise WordPieceError("normalize_tensor needs a contiguous uint8 CUDA/HIP tensor")
        (text, nbytes), = _whole_words(text)
        d_out = C.c_void_p()
        n = C.c_size_t()
        _check(lib().wp_normalize_device(self._h, C.c_void_p(text.data_ptr()), nbytes,
                                         self._normalize if flags is None else int(flags), C.byref(d_out), C.byref(n)))
        if n.value == 0:
            return torch.zeros(0, dtype=torch.uint8, device=text.device)
        view = torch.as_tensor(DeviceIds(d_out.value, n.value, typestr="|u1"), device=text.device)
        return view.clone() if copy else view

    def stats(self):
        s = Stats()
        _check(lib().wp_get_stats(self._h, C.byref(s)))
        d = s.as_dict()
        ns = NormStats()
        _check(lib().wp_get_norm_stats(self._h, C.byref(ns)))
        d.update({k: getattr(ns, k) for k, _ in ns._fields_})
        return d

    def _stats(self, struct, getter, drop=()):
        """one of the smaller statistics structs of the last call as a dict (an array field as a list), without `drop`"""
        s = struct()
        _check(getattr(lib(), getter)(self._h, C.byref(s)))
        values = ((k, getattr(s, k)) for k, _ in s._fields_ if k not in drop)
        return {k: list(x) if isinstance(x, C.Array) else x for k, x in values}

    def walk_stats(self):
        """wp_walk_stats of the last encode (Linear or fast) as a dict: n_wide_words, n_long_words, lean,
        max_anchor_gap."""
        return self._stats(WalkStats, "wp_get_walk_stats")

    def refine_stats(self):
        """wp_refine_stats of the last encode as a dict: n_groups, n_entries, n_large_groups, n_large_entries,
        trie_nodes, sort_bits, key_lookup, symbol_bytes."""
        return self._stats(RefineStats, "wp_get_refine_stats", drop=("reserved",))

    def refine_sched(self):
        """wp_refine_sched of the last encode as a dict: early (1: the refinement ran beside the round-0 passes),
        ms_sort_to_scan (WP_OPT_STAGE_TIMING: last round-0 pass to the scanline stage, in ms)."""
        return self._stats(RefineSched, "wp_get_refine_sched", drop=("reserved",))

    def step_stats(self):
        """wp_step_stats of the last encode as a dict: n_marks, n_steps, n_tiles, n_groups_of_tiles, bucket_shift,
        bucket_shift_all, key_shift, key_shift_all, packed, key_lookup."""
        return self._stats(StepStats, "wp_get_step_stats")

    def encode(self, text):
        """Host UTF-8 bytes/str -> numpy int32 ids (wp_linear_encode)."""
        b = _bytes(text)
        ids = C.POINTER(C.c_int32)()
        n = C.c_size_t()
        _check(lib().wp_linear_encode(self._h, b, len(b), C.byref(ids), C.byref(n)))
        return _adopt_ids(ids, n.value)

    def encode_with_offsets(self, text, unit="byte"):
        """Host UTF-8 bytes/str -> (ids: numpy int32 [n], offsets: numpy uint32 [n, 2]) (wp_linear_encode_offsets):
        offsets[k] = [begin, end) of id k in the input, unit "byte" (offsets into the UTF-8 bytes) or "char" (code
        points: str indices for valid UTF-8).  Both arrays are views of the library's blocks."""
        b = _bytes(text)
        ids = C.POINTER(C.c_int32)()
        offs = C.POINTER(C.c_uint32)()
        n = C.c_size_t()
        _check(lib().wp_linear_encode_offsets(self._h, b, len(b), _offset_unit(unit), C.byref(ids), C.byref(offs),
                                              C.byref(n)))
        if n.value == 0:
            return np.zeros(0, dtype=np.int32), np.zeros((0, 2), dtype=np.uint32)
        return _adopt_ids(ids, n.value), _adopt_block(offs, (n.value, 2))

    def encode_device_with_offsets(self, d_ptr, nbytes, unit="byte"):
        """Text already in HBM -> (device pointer of int32 ids, device pointer of uint32 [n, 2] offsets, n); both
        buffers are owned by the handle and valid until the next call (wp_linear_encode_offsets_device)."""
        d_ids = C.c_void_p()
        d_offs = C.c_void_p()
        n = C.c_size_t()
        _check(lib().wp_linear_encode_offsets_device(self._h, C.c_void_p(d_ptr), nbytes, _offset_unit(unit), C.byref(d_ids),
                                                     C.byref(d_offs), C.byref(n)))
        return d_ids.value, d_offs.value, n.value

    def encode_rows(self, docs=None, text=None, doc_offsets=None, offsets=None):
        """Many documents in one call (wp_linear_encode_rows) -> (ids int32 [n], row_splits int64 [n_rows + 1]) and,
        with offsets="byte" / "char", offsets uint32 [n, 2] relative to the id's own document; row i is
        ids[row_splits[i]:row_splits[i + 1]] and equals encode_with_offsets(document i).  `docs`: a list of str / bytes
        (joined here, join_docs); or `text` in joined form (every document followed by one "\\n") with `doc_offsets`
        (int64 [n_docs + 1]), or alone: the rows are its lines.  The arrays are views of the library's blocks."""
        b, off = _docs_arg(docs, text, doc_offsets)
        unit = -1 if offsets is None else _offset_unit(offsets)
        ids, splits, offs = C.POINTER(C.c_int32)(), C.POINTER(C.c_int64)(), C.POINTER(C.c_uint32)()
        n, rows = C.c_size_t(), C.c_size_t()
        _check(lib().wp_linear_encode_rows(self._h, b, len(b), _i64_ptr(off), 0 if off is None else len(off) - 1, unit,
                                           C.byref(ids), C.byref(splits), C.byref(offs), C.byref(n), C.byref(rows)))
        out = (_adopt_ids(ids, n.value), _adopt_block(splits, (rows.value + 1,)))
        if offsets is None:
            return out
        return out + (_adopt_block(offs, (n.value, 2)) if n.value else np.zeros((0, 2), dtype=np.uint32),)

    def encode_padded(self, docs=None, text=None, doc_offsets=None, max_len=128, cls_id=None, sep_id=None, pad_id=0):
        """Padded batch (wp_linear_encode_padded) -> (input_ids int32 [n_rows, max_len], lengths int32 [n_rows]): row r is
        [cls] + ids of document r cut to fit + [sep] + pad...; lengths[r] counts everything but the padding (attention
        mask: arange(max_len) < lengths[:, None]).  Documents as in encode_rows."""
        b, off = _docs_arg(docs, text, doc_offsets)
        ids, lens = C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)()
        rows = C.c_size_t()
        _check(lib().wp_linear_encode_padded(self._h, b, len(b), _i64_ptr(off), 0 if off is None else len(off) - 1,
                                             int(max_len), _special(cls_id), _special(sep_id), int(pad_id), C.byref(ids),
                                             C.byref(lens), C.byref(rows)))
        if rows.value == 0:
            return np.zeros((0, int(max_len)), dtype=np.int32), np.zeros(0, dtype=np.int32)
        return _adopt_block(ids, (rows.value, int(max_len))), _adopt_block(lens, (rows.value,))

    def _rows_tensor_args(self, text, doc_offsets):
        import torch
        if text.dtype != torch.uint8 or not text.is_cuda or not text.is_contiguous():
            raise WordPieceError("a documents call on tensors needs a contiguous uint8 CUDA/HIP text tensor")
        if doc_offsets is not None:
            if doc_offsets.dtype != torch.int64 or doc_offsets.device != text.device or doc_offsets.dim() != 1 or \
                    doc_offsets.numel() < 1:
                raise WordPieceError("doc_offsets must be a 1-d int64 tensor on the text's device")
            doc_offsets = doc_offsets.contiguous()
        (text, nbytes), = _whole_words(text)  # (last: it waits for torch's stream, the copy above included)
        return text, nbytes, doc_offsets

    def encode_rows_tensor(self, text, doc_offsets=None, offsets=None, copy=True):
        """encode_rows for a uint8 text tensor in joined form (and an optional int64 offsets tensor) on this handle's
        GPU (wp_linear_encode_rows_device) -> tensors there: (ids int32 [n], row_splits int64 [n_rows + 1][, offsets
        uint32 [n, 2]]).  copy=False: views of the library's buffers, valid until the next call on this handle."""
        import torch
        text, nbytes, doc_offsets = self._rows_tensor_args(text, doc_offsets)
        unit = -1 if offsets is None else _offset_unit(offsets)
        d_ids, d_splits, d_offs = C.c_void_p(), C.c_void_p(), C.c_void_p()
        n, rows = C.c_size_t(), C.c_size_t()
        _check(lib().wp_linear_encode_rows_device(
            self._h, C.c_void_p(text.data_ptr()), nbytes, None if doc_offsets is None else C.c_void_p(doc_offsets.data_ptr()),
            0 if doc_offsets is None else doc_offsets.numel() - 1, unit, C.byref(d_ids), C.byref(d_splits), C.byref(d_offs),
            C.byref(n), C.byref(rows)))
        dev = text.device
        ids = torch.as_tensor(DeviceIds(d_ids.value, n.value), device=dev) if n.value else \
            torch.zeros(0, dtype=torch.int32, device=dev)
        splits = torch.as_tensor(DeviceIds(d_splits.value, rows.value + 1, typestr="<i8"), device=dev)
        out = (ids, splits)
        if offsets is not None:
            out += (torch.as_tensor(DeviceIds(d_offs.value, n.value, cols=2), device=dev).view(torch.uint32) if n.value else
                    torch.zeros((0, 2), dtype=torch.uint32, device=dev),)
        return tuple(t.clone() for t in out) if copy else out

    def encode_padded_tensor(self, text, doc_offsets=None, max_len=128, cls_id=None, sep_id=None, pad_id=0, n_rows=None,
                             out=None):
        """encode_padded for tensors on this handle's GPU (wp_linear_encode_padded_device) -> (input_ids int32
        [n_rows, max_len], lengths int32 [n_rows]) written by the library into torch.empty tensors (no copy).  The row
        count of explicit offsets is known; in lines mode pass `n_rows` (an upper bound will do) or the call runs twice
        when the first guess was too small.  out=(input_ids, lengths): caller-owned tensors to write into (views of the
        first n_rows rows are returned)."""
        import torch
        text, nbytes, doc_offsets = self._rows_tensor_args(text, doc_offsets)
        max_len = int(max_len)
        cap = doc_offsets.numel() - 1 if doc_offsets is not None else int(n_rows) if n_rows is not None else nbytes // 32 + 1
        rows = C.c_size_t()
        for _ in range(2):
            if out is not None:
                ids, lens = out
                if ids.dtype != torch.int32 or lens.dtype != torch.int32 or not ids.is_contiguous() or \
                        not lens.is_contiguous() or ids.device != text.device or lens.device != text.device or \
                        ids.dim() != 2 or ids.shape[1] != max_len:
                    raise WordPieceError("out must be contiguous int32 tensors [rows, max_len] and [rows] on the text's device")
                cap = min(ids.shape[0], lens.numel())
            else:
                ids = torch.empty((cap, max_len), dtype=torch.int32, device=text.device)
                lens = torch.empty(cap, dtype=torch.int32, device=text.device)
            torch.cuda.current_stream(text.device).synchronize()
            rc = lib().wp_linear_encode_padded_device(
                self._h, C.c_void_p(text.data_ptr()), nbytes, None if doc_offsets is None else C.c_void_p(doc_offsets.data_ptr()),
                0 if doc_offsets is None else doc_offsets.numel() - 1, max_len, _special(cls_id), _special(sep_id), int(pad_id),
                C.c_void_p(ids.data_ptr()), C.c_void_p(lens.data_ptr()), cap, C.byref(rows))
            if rc != 0 and out is None and rows.value > cap:  # (lines mode, guess too small: the call said how many)
                cap = rows.value
                continue
            _check(rc)
            break
        return ids[:rows.value], lens[:rows.value]

    def inputs_stats(self):
        """wp_inputs_stats of the last call as a dict (n_out -1: it was no inputs call)."""
        return self._stats(InputsStats, "wp_get_inputs_stats", drop=("reserved",))

    def encode_inputs(self, a=None, b=None, text=None, doc_offsets=None, pairs=None, max_len=128, cls_id=None, sep_id=None,
                      pad_id=0, truncation="longest_first", stride=None, offsets=None):
        """Model inputs (wp_linear_encode_inputs) -> a dict of numpy arrays: input_ids, token_type_ids int32 [n_out,
        max_len], lengths, sample int32 [n_out] and, with offsets="byte" / "char", offsets uint32 [n_out, max_len, 2].
        Row r is [cls] A' [sep] (B' [sep]) pad...; `a` (and `b`, of the same length, for pairs) are lists of str / bytes,
        interleaved and joined here; or `text` in joined form (with `doc_offsets`, or alone: its lines) and `pairs`
        (True: rows 2s, 2s + 1 are A and B of sample s).  truncation: "longest_first", "only_first", "only_second";
        stride=None: one row per sample; stride >= 0 (only_first / only_second): every sample gives as many overlapping
        windows as cover its windowed side, sample[r] names the sample of row r."""
        if a is not None:
            if text is not None or doc_offsets is not None or pairs is not None:
                raise WordPieceError("text, doc_offsets and pairs go with the joined form, not with a / b")
            if b is not None and len(b) != len(a):
                raise WordPieceError("a and b must have the same length")
            pairs = b is not None
            docs = [d for ab in zip(a, b) for d in ab] if pairs else list(a)
            bt, off = join_docs(docs)
        else:
            if b is not None:
                raise WordPieceError("b goes with a")
            if text is None:
                raise WordPieceError("give either a (and b) or text")
            bt, off = _docs_arg(None, text, doc_offsets)
        spec = _inputs_spec(max_len, cls_id, sep_id, pad_id, pairs, truncation, stride, offsets)
        out = Inputs()
        n, ns = C.c_size_t(), C.c_size_t()
        _check(lib().wp_linear_encode_inputs(self._h, bt, len(bt), _i64_ptr(off), 0 if off is None else len(off) - 1,
                                             C.byref(spec), C.byref(out), C.byref(n), C.byref(ns)))
        rows, L = n.value, int(max_len)
        i32p = C.POINTER(C.c_int32)
        if rows == 0:
            res = {"input_ids": np.zeros((0, L), np.int32), "token_type_ids": np.zeros((0, L), np.int32),
                   "lengths": np.zeros(0, np.int32), "sample": np.zeros(0, np.int32)}
            if offsets is not None:
                res["offsets"] = np.zeros((0, L, 2), np.uint32)
            return res
        res = {"input_ids": _adopt_block(C.cast(out.input_ids, i32p), (rows, L)),
               "token_type_ids": _adopt_block(C.cast(out.token_type_ids, i32p), (rows, L)),
               "lengths": _adopt_block(C.cast(out.lengths, i32p), (rows,)),
               "sample": _adopt_block(C.cast(out.sample, i32p), (rows,))}
        if offsets is not None:
            res["offsets"] = _adopt_block(C.cast(out.offsets, C.POINTER(C.c_uint32)), (rows, L, 2))
        return res

    def encode_inputs_tensor(self, text, doc_offsets=None, pairs=False, max_len=128, cls_id=None, sep_id=None, pad_id=0,
                             truncation="longest_first", stride=None, offsets=None, n_out=None, out=None):
        """encode_inputs for tensors on this handle's GPU (wp_linear_encode_inputs_device) -> a dict of tensors written by
        the library into torch.empty tensors (no copy); offsets come as int32 [n_out, max_len, 2] viewed as uint32.
        Without windows the row count of explicit offsets is known; otherwise pass `n_out` (an upper bound will do) or
        the call runs twice when the first guess was too small.  out=dict of caller-owned tensors (the same keys) to
        write into: views of the first n_out rows are returned."""
        import torch
        text, nbytes, doc_offsets = self._rows_tensor_args(text, doc_offsets)
        L = int(max_len)
        spec = _inputs_spec(L, cls_id, sep_id, pad_id, pairs, truncation, stride, offsets)
        keys = ["input_ids", "token_type_ids", "lengths", "sample"] + (["offsets"] if offsets is not None else [])
        if n_out is not None:
            cap = int(n_out)
        elif doc_offsets is not None:
            cap = (doc_offsets.numel() - 1) // (2 if pairs else 1)
        else:
            cap = nbytes // 32 + 1
        dev = text.device
        rows, ns = C.c_size_t(), C.c_size_t()
        for _ in range(2):
            if out is not None:
                t = {k: out[k] for k in keys}
                for k in keys:
                    x = t[k]
                    shape_ok = (x.dim() == 1 if k in ("lengths", "sample") else
                                x.dim() == 2 and x.shape[1] == L if k != "offsets" else
                                x.dim() == 3 and x.shape[1] == L and x.shape[2] == 2)
                    if x.dtype not in ((torch.int32, torch.uint32) if k == "offsets" else (torch.int32,)) or \
                            not x.is_contiguous() or x.device != dev or not shape_ok:
                        raise WordPieceError("out must hold contiguous int32 tensors [rows, max_len], [rows] (offsets: "
                                             "[rows, max_len, 2], int32 or uint32) on the text's device")
                cap = min(x.shape[0] for x in t.values())
            else:
                t = {"input_ids": torch.empty((cap, L), dtype=torch.int32, device=dev),
                     "token_type_ids": torch.empty((cap, L), dtype=torch.int32, device=dev),
                     "lengths": torch.empty(cap, dtype=torch.int32, device=dev),
                     "sample": torch.empty(cap, dtype=torch.int32, device=dev)}
                if offsets is not None:
                    t["offsets"] = torch.empty((cap, L, 2), dtype=torch.int32, device=dev).view(torch.uint32)
            bufs = Inputs(*[t[k].data_ptr() if k in t else None
                            for k in ("input_ids", "token_type_ids", "lengths", "sample", "offsets")])
            torch.cuda.current_stream(dev).synchronize()
            rc = lib().wp_linear_encode_inputs_device(
                self._h, C.c_void_p(text.data_ptr()), nbytes, None if doc_offsets is None else C.c_void_p(doc_offsets.data_ptr()),
                0 if doc_offsets is None else doc_offsets.numel() - 1, C.byref(spec), C.byref(bufs), cap, C.byref(rows),
                C.byref(ns))
            if rc != 0 and out is None and rows.value > cap:  # (guess too small: the call said how many)
                cap = rows.value
                continue
            _check(rc)
            break
        return {k: t[k][:rows.value] for k in keys}

    def mask_stats(self):
        """wp_mask_stats of the last call as a dict (n_rows -1: it was no mask or word-ids call)."""
        return self._stats(MaskStats, "wp_get_mask_stats", drop=("reserved",))

    def word_ids(self, input_ids, lengths=None, cls_id=None, sep_id=None, pad_id=None):
        """The word index of every cell of an id batch (wp_word_ids): input_ids int32 [n_rows, max_len] (and lengths
        [n_rows]) -> numpy int32 [n_rows, max_len], -1 for specials, padding and ids outside the vocabulary; the count
        restarts behind every special (HF Encoding.word_ids())."""
        ids, lens = _mask_batch(input_ids, lengths)
        spec = MaskSpec(max_len=ids.shape[1], cls_id=_special(cls_id), sep_id=_special(sep_id), pad_id=_special(pad_id))
        out = C.POINTER(C.c_int32)()
        _check(lib().wp_word_ids(self._h, _i32_ptr(ids), _i32_ptr(lens), ids.shape[0], C.byref(spec), C.byref(out)))
        return _adopt_block(out, ids.shape) if ids.shape[0] else np.zeros(ids.shape, np.int32)

    def mask_inputs(self, input_ids, lengths=None, mask_id=None, prob=0.15, mask_share=0.8, random_share=0.1,
                    whole_word=True, seed=0, row_base=0, ignore_id=-100, cls_id=None, sep_id=None, pad_id=None,
                    word_ids=False):
        """The masked-language-model transform of an id batch (wp_mlm_mask): input_ids int32 [n_rows, max_len] (and
        lengths [n_rows]) -> a dict of numpy int32 arrays of that shape: input_ids (masked), labels (ignore_id where
        nothing is to be predicted) and, with word_ids=True, word_ids.  About `prob` of the cells are selected, whole
        words at a time (whole_word=False: cell by cell); of those mask_share become mask_id, random_share a uniform
        id of the vocabulary, the rest stay.  The same seed gives the same batch; row_base is the row number of row 0
        (a slice of a batch gives the rows of the whole batch).  cls_id / sep_id / pad_id: never selected, and words
        do not run across them."""
        ids, lens = _mask_batch(input_ids, lengths)
        spec = _mask_spec(ids.shape[1], mask_id, prob, mask_share, random_share, whole_word, seed, row_base, ignore_id, cls_id,
                          sep_id, pad_id)
        i32p = C.POINTER(C.c_int32)
        masked, labels, wids = i32p(), i32p(), i32p()
        _check(lib().wp_mlm_mask(self._h, _i32_ptr(ids), _i32_ptr(lens), ids.shape[0], C.byref(spec), C.byref(masked),
                                 C.byref(labels), C.byref(wids) if word_ids else None))
        if ids.shape[0] == 0:
            return {k: np.zeros(ids.shape, np.int32) for k in ["input_ids", "labels"] + (["word_ids"] if word_ids else [])}
        res = {"input_ids": _adopt_block(masked, ids.shape), "labels": _adopt_block(labels, ids.shape)}
        if word_ids:
            res["word_ids"] = _adopt_block(wids, ids.shape)
        return res

    def _mask_tensor_args(self, input_ids, lengths):
        import torch
        if isinstance(input_ids, dict):  # what encode_inputs_tensor returns
            if lengths is None:
                lengths = input_ids.get("lengths")
            input_ids = input_ids["input_ids"]
        if input_ids.dtype != torch.int32 or not input_ids.is_cuda or not input_ids.is_contiguous() or input_ids.dim() != 2:
            raise WordPieceError("a mask call on tensors needs a contiguous int32 CUDA/HIP tensor [n_rows, max_len]")
        if lengths is not None and (lengths.dtype != torch.int32 or lengths.device != input_ids.device or
                                    not lengths.is_contiguous() or lengths.shape != (input_ids.shape[0],)):
            raise WordPieceError("lengths must be a contiguous int32 tensor [n_rows] on the device of input_ids")
        if self._device is not None and input_ids.device.index != self._device:  # (raw pointers go to the handle's device)
            raise WordPieceError("the tensors lie on %s, the handle on device %d" % (input_ids.device, self._device))
        return input_ids, lengths

    def word_ids_tensor(self, input_ids, lengths=None, cls_id=None, sep_id=None, pad_id=None):
        """word_ids for an int32 tensor [n_rows, max_len] on this handle's GPU (or the dict encode_inputs_tensor returns)
        -> an int32 tensor there (wp_word_ids_device); nothing leaves the device."""
        import torch
        ids, lens = self._mask_tensor_args(input_ids, lengths)
        spec = MaskSpec(max_len=ids.shape[1], cls_id=_special(cls_id), sep_id=_special(sep_id), pad_id=_special(pad_id))
        out = torch.empty_like(ids)
        torch.cuda.current_stream(ids.device).synchronize()  # the library runs on its own HIP streams
        _check(lib().wp_word_ids_device(self._h, C.c_void_p(ids.data_ptr()), None if lens is None else C.c_void_p(lens.data_ptr()),
                                        ids.shape[0], C.byref(spec), C.c_void_p(out.data_ptr())))
        return out

    def mask_inputs_tensor(self, input_ids, lengths=None, mask_id=None, prob=0.15, mask_share=0.8, random_share=0.1,
                           whole_word=True, seed=0, row_base=0, ignore_id=-100, cls_id=None, sep_id=None, pad_id=None,
                           word_ids=False, in_place=False):
        """mask_inputs for an int32 tensor [n_rows, max_len] on this handle's GPU, or the dict encode_inputs_tensor
        returns (its lengths are used unless others are given) -> a dict of int32 tensors there: input_ids, labels[,
        word_ids] (wp_mlm_mask_device); nothing leaves the device.  in_place=True: the masked ids overwrite the tensor
        that was passed (which is then also the dict's input_ids)."""
        import torch
        ids, lens = self._mask_tensor_args(input_ids, lengths)
        spec = _mask_spec(ids.shape[1], mask_id, prob, mask_share, random_share, whole_word, seed, row_base, ignore_id, cls_id,
                          sep_id, pad_id)
        res = {"input_ids": ids if in_place else torch.empty_like(ids), "labels": torch.empty_like(ids)}
        if word_ids:
            res["word_ids"] = torch.empty_like(ids)
        torch.cuda.current_stream(ids.device).synchronize()  # the library runs on its own HIP streams
        _check(lib().wp_mlm_mask_device(self._h, C.c_void_p(ids.data_ptr()), None if lens is None else C.c_void_p(lens.data_ptr()),
                                        ids.shape[0], C.byref(spec), C.c_void_p(res["input_ids"].data_ptr()),
                                        C.c_void_p(res["labels"].data_ptr()),
                                        C.c_void_p(res["word_ids"].data_ptr()) if word_ids else None))
        return res

    def detok_stats(self):
        """wp_detok_stats of the last detokenize call as a dict (n_rows -1: no such call yet)."""
        return self._stats(DetokStats, "wp_get_detok_stats")

    def detok_piece(self, id, form, cleanup=True):
        """The bytes id `id` contributes to a row's text (wp_detok_piece; no GPU needed): form 0 as the first kept
        token of a row, form 1 behind another; None for an id out of range, a malformed one or another form."""
        n = lib().wp_detok_piece(self._h, int(id), int(form), int(cleanup), None, 0)
        if n < 0:
            return None
        buf = C.create_string_buffer(max(int(n), 1))
        lib().wp_detok_piece(self._h, int(id), int(form), int(cleanup), buf, n)
        return buf.raw[:n]

    def detokenize(self, ids, row_splits=None, lengths=None, skip_ids=(), cleanup=True, terminator=None, raw=False):
        """Ids back to text on the GPU (wp_detokenize), as tokenizers' WordPiece decoder gives it row by row: a 1-d
        int32 array with row_splits [n_rows + 1] (what encode_rows returns; without row_splits: one row), or a 2-d
        array [n_rows, max_len] with optional lengths -> a list of n_rows str (invalid UTF-8, which only a cut through
        a token's bytes by the clean-up could give, is replaced).  skip_ids: up to 8 ids left out ([CLS], [SEP],
        [PAD]: skip_special_tokens); ids outside the vocabulary and malformed ones are always dropped.  terminator: a
        byte (int or 1-char str) behind every row of the raw text.  raw=True: (text bytes, text_off int64 [n_rows + 1])
        as the library returns them."""
        a = np.ascontiguousarray(ids, dtype=np.int32)
        splits = lens = None
        if a.ndim == 2:
            if row_splits is not None:
                raise WordPieceError("row_splits go with a 1-d ids array")
            n_rows, max_len = a.shape
            if max_len < 1:
                raise WordPieceError("a padded batch needs max_len >= 1")
            if lengths is not None:
                lens = np.ascontiguousarray(lengths, dtype=np.int32)
                if lens.shape != (n_rows,):
                    raise WordPieceError("lengths must be a 1-d array of n_rows entries")
        elif a.ndim == 1:
            if lengths is not None:
                raise WordPieceError("lengths go with a 2-d ids array")
            splits = np.array([0, len(a)], dtype=np.int64) if row_splits is None else \
                np.ascontiguousarray(row_splits, dtype=np.int64)
            if splits.ndim != 1 or len(splits) < 1:
                raise WordPieceError("row_splits must be a 1-d array of n_rows + 1 entries")
            if len(splits) > 1 and splits[-1] > len(a):
                raise WordPieceError("row_splits end behind the ids")
            n_rows, max_len = len(splits) - 1, 0
        else:
            raise WordPieceError("ids must be a 1-d or 2-d array")
        spec = _detok_spec(max_len, skip_ids, cleanup, terminator)
        text, off, nb = C.c_void_p(), C.POINTER(C.c_int64)(), C.c_size_t()
        _check(lib().wp_detokenize(self._h, _i32_ptr(a), _i64_ptr(splits), _i32_ptr(lens), n_rows, C.byref(spec), C.byref(text),
                                   C.byref(off), C.byref(nb)))
        text_off = _adopt_block(off, (n_rows + 1,))
        data = b""
        if text.value:
            data = C.string_at(text.value, nb.value)
            lib().wp_free(text)
        if raw:
            return data, text_off
        t = 1 if spec.terminator >= 0 else 0
        return [data[text_off[r]:text_off[r + 1] - t].decode("utf-8", "replace") for r in range(n_rows)]

    def detokenize_tensor(self, ids, row_splits=None, lengths=None, skip_ids=(), cleanup=True, terminator=None, copy=True):
        """detokenize for tensors on this handle's GPU (wp_detokenize_device): ids int32 [n] with row_splits int64
        [n_rows + 1] (what encode_rows_tensor returns; without row_splits: one row), or ids int32 [n_rows, max_len] with
        optional lengths int32 [n_rows] -> (text uint8 [n_bytes], text_off int64 [n_rows + 1]) there; nothing leaves
        the device.  copy=False: views of the library's buffers, valid until the next call on this handle."""
        import torch
        if ids.dtype != torch.int32 or not ids.is_cuda or not ids.is_contiguous() or ids.dim() not in (1, 2):
            raise WordPieceError("detokenize on tensors needs a contiguous int32 CUDA/HIP tensor [n] or [n_rows, max_len]")
        if self._device is not None and ids.device.index != self._device:  # (raw pointers go to the handle's device)
            raise WordPieceError("the tensors lie on %s, the handle on device %d" % (ids.device, self._device))
        dev = ids.device
        if ids.dim() == 2:
            if row_splits is not None:
                raise WordPieceError("row_splits go with a 1-d ids tensor")
            n_rows, max_len = ids.shape
            if max_len < 1:
                raise WordPieceError("a padded batch needs max_len >= 1")
            if lengths is not None and (lengths.dtype != torch.int32 or lengths.device != dev or not lengths.is_contiguous() or
                                        lengths.shape != (n_rows,)):
                raise WordPieceError("lengths must be a contiguous int32 tensor [n_rows] on the device of ids")
            rows = lengths
        else:
            if lengths is not None:
                raise WordPieceError("lengths go with a 2-d ids tensor")
            if row_splits is None:
                row_splits = torch.tensor([0, ids.numel()], dtype=torch.int64, device=dev)
            if row_splits.dtype != torch.int64 or row_splits.device != dev or row_splits.dim() != 1 or row_splits.numel() < 1:
                raise WordPieceError("row_splits must be a 1-d int64 tensor on the device of ids")
            rows = row_splits = row_splits.contiguous()
            n_rows, max_len = row_splits.numel() - 1, 0
        for t in (ids, rows):  # (a view of a tensor may start anywhere)
            if t is not None and t.data_ptr() % t.element_size() != 0:
                raise WordPieceError("the tensors must be aligned to their element size")
        spec = _detok_spec(max_len, skip_ids, cleanup, terminator)
        d_text, d_off, nb = C.c_void_p(), C.c_void_p(), C.c_size_t()
        torch.cuda.current_stream(dev).synchronize()  # the library runs on its own HIP streams
        _check(lib().wp_detokenize_device(
            self._h, C.c_void_p(ids.data_ptr()) if ids.numel() else None,
            C.c_void_p(row_splits.data_ptr()) if max_len == 0 else None,
            C.c_void_p(lengths.data_ptr()) if max_len and lengths is not None else None, n_rows, C.byref(spec),
            C.byref(d_text), C.byref(d_off), C.byref(nb)))
        text = torch.as_tensor(DeviceIds(d_text.value, nb.value, typestr="|u1"), device=dev) if nb.value else \
            torch.zeros(0, dtype=torch.uint8, device=dev)
        off = torch.as_tensor(DeviceIds(d_off.value, n_rows + 1, typestr="<i8"), device=dev)
        return (text.clone(), off.clone()) if copy else (text, off)

    def pack_stats(self):
        """wp_pack_stats of the last pack call as a dict (n_docs -1: no such call yet)."""
        return self._stats(PackStats, "wp_get_pack_stats")

    def pack_sequences(self, ids, row_splits, max_len=128, mode="next_fit", bos_id=None, eos_id=None, pad_id=0,
                       long_docs="truncate", want=("segment_ids", "position_ids", "source")):
        """Several encoded documents per row (wp_pack_sequences): ids int32 [n] with row_splits int64 [n_docs + 1] (what
        encode_rows returns) -> a dict of numpy int32 arrays: input_ids [n_out, max_len], lengths [n_out] and the wanted
        ones of segment_ids, position_ids, source [n_out, max_len].  Every document becomes [bos] ids [eos]; mode
        "next_fit": a unit opens a new row when it does not fit behind the ones before it (long_docs: "truncate" cuts a
        document to one row, "split" cuts it into several units); "stream": the units back to back, cut every max_len
        cells.  segment_ids count the units of a row from 1 (0: padding), position_ids restart with every unit, source
        is the index into ids of an id cell (-1: specials, padding)."""
        a = np.ascontiguousarray(ids, dtype=np.int32)
        splits = np.ascontiguousarray(row_splits, dtype=np.int64)
        if a.ndim != 1 or splits.ndim != 1 or len(splits) < 1:
            raise WordPieceError("ids must be a 1-d array and row_splits a 1-d array of n_docs + 1 entries")
        if splits[-1] > len(a):
            raise WordPieceError("row_splits end behind the ids")
        spec = _pack_spec(max_len, mode, bos_id, eos_id, pad_id, long_docs, want)
        out, n = Packed(), C.c_size_t()
        _check(lib().wp_pack_sequences(self._h, _i32_ptr(a), _i64_ptr(splits), len(splits) - 1, C.byref(spec), C.byref(out),
                                       C.byref(n)))
        rows, L = n.value, int(max_len)
        keys = ["input_ids"] + [k for k, bit in _PACK_WANT.items() if spec.want & bit]
        if rows == 0:
            res = {k: np.zeros((0, L), np.int32) for k in keys}
            res["lengths"] = np.zeros(0, np.int32)
            return res
        i32p = C.POINTER(C.c_int32)
        res = {k: _adopt_block(C.cast(getattr(out, k), i32p), (rows, L)) for k in keys}
        res["lengths"] = _adopt_block(C.cast(out.lengths, i32p), (rows,))
        return res

    def pack_sequences_tensor(self, ids, row_splits, max_len=128, mode="next_fit", bos_id=None, eos_id=None, pad_id=0,
                              long_docs="truncate", want=("segment_ids", "position_ids", "source"), n_out=None, out=None):
        """pack_sequences for tensors on this handle's GPU (wp_pack_sequences_device): ids int32 [n] and row_splits int64
        [n_docs + 1] (what encode_rows_tensor returns, views included) -> a dict of int32 tensors written by the library
        into torch.empty tensors (no copy); nothing leaves the device.  n_out: the row count if it is known (an upper
        bound will do); without it the rows are sized by the stream bound ceil((n + 2 n_docs) / max_len) in stream mode
        and by min(n_docs, twice that bound + 1) otherwise, and the call runs twice when that was too small (split mode).  out=dict of caller-owned
        tensors (the same keys) to write into: views of the first n_out rows are returned."""
        import torch
        if ids.dtype != torch.int32 or not ids.is_cuda or not ids.is_contiguous() or ids.dim() != 1:
            raise WordPieceError("pack on tensors needs a contiguous 1-d int32 CUDA/HIP tensor of ids")
        dev = ids.device
        if self._device is not None and dev.index != self._device:  # (raw pointers go to the handle's device)
            raise WordPieceError("the tensors lie on %s, the handle on device %d" % (dev, self._device))
        if row_splits.dtype != torch.int64 or row_splits.device != dev or row_splits.dim() != 1 or row_splits.numel() < 1 or \
                not row_splits.is_contiguous():
            raise WordPieceError("row_splits must be a contiguous 1-d int64 tensor on the device of ids")
        for t in (ids, row_splits):  # (a view of a tensor may start anywhere)
            if t.data_ptr() % t.element_size() != 0:
                raise WordPieceError("the tensors must be aligned to their element size")
        L = int(max_len)
        spec = _pack_spec(L, mode, bos_id, eos_id, pad_id, long_docs, want)
        n_docs = row_splits.numel() - 1
        keys = ["input_ids"] + [k for k, bit in _PACK_WANT.items() if spec.want & bit] + ["lengths"]
        if n_out is not None:
            cap = int(n_out)
        elif spec.mode == WP_PACK_STREAM:
            cap = (ids.numel() + 2 * n_docs + L - 1) // L
        else:  # (two neighbouring rows hold more than max_len cells between them, and a document gives a row at most)
            cap = min(n_docs, 2 * (ids.numel() + 2 * n_docs) // L + 1)
        rows = C.c_size_t()
        for _ in range(2):
            if out is not None:
                t = {k: out[k] for k in keys}
                for k, x in t.items():
                    if x.dtype != torch.int32 or not x.is_contiguous() or x.device != dev or \
                            not (x.dim() == 1 if k == "lengths" else x.dim() == 2 and x.shape[1] == L):
                        raise WordPieceError("out must hold contiguous int32 tensors [rows, max_len] and lengths [rows] on the "
                                             "device of ids")
                cap = min(x.shape[0] for x in t.values())
            else:
                t = {k: torch.empty(cap if k == "lengths" else (cap, L), dtype=torch.int32, device=dev) for k in keys}
            bufs = Packed(*[t[k].data_ptr() if k in t and cap else None
                            for k in ("input_ids", "segment_ids", "position_ids", "source", "lengths")])
            torch.cuda.current_stream(dev).synchronize()  # the library runs on its own HIP streams
            rc = lib().wp_pack_sequences_device(
                self._h, C.c_void_p(ids.data_ptr()) if ids.numel() else None, C.c_void_p(row_splits.data_ptr()), n_docs,
                C.byref(spec), C.byref(bufs), cap, C.byref(rows))
            if rc != 0 and out is None and rows.value > cap:  # (guess too small: the call said how many)
                cap = rows.value
                continue
            _check(rc)
            break
        return {k: t[k][:rows.value] for k in keys}

    def encode_packed_tensor(self, text, doc_offsets=None, max_len=128, mode="next_fit", bos_id=None, eos_id=None, pad_id=0,
                             long_docs="truncate", want=("segment_ids", "position_ids", "source"), n_out=None):
        """Text to a packed batch without leaving the device: encode_rows_tensor without a copy (the rows stay in the
        library's buffers), then pack_sequences_tensor, which has buffers of its own.  text, doc_offsets as in
        encode_rows_tensor; the rest as in pack_sequences_tensor."""
        ids, splits = self.encode_rows_tensor(text, doc_offsets, copy=False)
        return self.pack_sequences_tensor(ids, splits, max_len=max_len, mode=mode, bos_id=bos_id, eos_id=eos_id, pad_id=pad_id,
                                          long_docs=long_docs, want=want, n_out=n_out)

    def count_stats(self):
        """wp_count_stats of the last count call as a dict (n_words -1: no such call yet)."""
        return self._stats(CountStats, "wp_get_count_stats")

    @staticmethod
    def _count_spec(order, min_count, max_word_bytes, terminator, index, hash_bits):
        if order not in _COUNT_ORDERS:
            raise WordPieceError("count: order must be 'first' or 'count'")
        return CountSpec(_COUNT_ORDERS[order], int(max_word_bytes), _terminator_byte("count", terminator), WP_COUNT_WANT_INDEX if index else 0,
                         int(hash_bits), 0, int(min_count))

    def count_words(self, text, order="first", min_count=1, max_word_bytes=256, terminator=None, index=False, raw=False,
                    hash_bits=0):
        """The distinct words of a text with their counts (wp_count_words): the words of the handle's normalised text by
        the encoder's own word rule, in order of first occurrence ("first") or of Counter.most_common() ("count").
        -> {"words": [str...], "counts": np.int64[...]} and, with index, "word_index": np.int32 per word occurrence (-1:
        long or below min_count).  raw: "words" is the byte pool (np.uint8; each word followed by `terminator`, a byte or
        one-byte str, if given) and "word_off" (np.int64) comes along.  hash_bits: for tests of the collision rounds."""
        b = _bytes(text)
        spec = self._count_spec(order, min_count, max_word_bytes, terminator, index, hash_bits)
        out = WordCounts()
        _check(lib().wp_count_words(self._h, b, len(b), C.byref(spec), C.byref(out)))
        res = _host_result("count", out, dict(index=index))
        if not raw:
            data, off, cut = res["words"].tobytes(), res.pop("word_off"), 1 if spec.terminator >= 0 else 0
            res["words"] = [data[off[k]:off[k + 1] - cut].decode("utf8") for k in range(len(off) - 1)]
        return res

    def count_words_tensor(self, text, order="first", min_count=1, max_word_bytes=256, terminator=None, index=False, copy=True,
                           hash_bits=0):
        """count_words for a uint8 text tensor on this handle's GPU (wp_count_words_device) -> {"words": uint8 pool,
        "word_off": int64 [n + 1], "counts": int64 [n]} and, with index, "word_index": int32 per word occurrence, tensors
        on that device.  copy=False: views of the library's buffers, valid until the next call on this handle."""
        import torch
        if text.dtype != torch.uint8 or not text.is_cuda or not text.is_contiguous():
            raise WordPieceError("count_words_tensor needs a contiguous uint8 CUDA/HIP tensor")
        spec = self._count_spec(order, min_count, max_word_bytes, terminator, index, hash_bits)
        (text, nbytes), = _whole_words(text)
        out = WordCounts()
        _check(lib().wp_count_words_device(self._h, C.c_void_p(text.data_ptr()), nbytes, C.byref(spec), C.byref(out)))
        return _layer_result("count", out, _DeviceViews(text.device, copy), dict(index=index))

    def learn_stats(self):
        """wp_learn_stats of the last learn call as a dict (n_words -1: no such call yet)."""
        return self._stats(LearnStats, "wp_get_learn_stats")

    @staticmethod
    def _learn_spec(vocab_size, reserved, lower_thresh, upper_thresh, num_iterations, max_token_chars, max_unique_chars, slack_ratio,
                    slack, terminator, hash_bits):
        """-> (LearnSpec, what it points into: keep both alive over the call)"""
        res = [_bytes(r) for r in reserved]
        off = _offsets_of([len(r) for r in res])
        pool = b"".join(res)
        if slack is None:
            slack = int(slack_ratio * vocab_size)
        spec = LearnSpec(pool, off.ctypes.data_as(C.POINTER(C.c_int64)), len(res), int(vocab_size), int(lower_thresh), int(upper_thresh),
                         int(slack), int(num_iterations), int(max_token_chars), int(max_unique_chars), _terminator_byte("learn", terminator),
                         int(hash_bits), 0)
        return spec, (pool, off)

    def learn_vocab(self, table, vocab_size, reserved=DEFAULT_RESERVED, lower_thresh=10, upper_thresh=10_000_000, num_iterations=4,
                    max_token_chars=50, max_unique_chars=1000, slack_ratio=0.05, slack=None, hash_bits=0):
        """A WordPiece vocabulary learned from a word table on the device (wp_learn_vocab).  table: the dict count_words
        returns ("words": strs or bytes, "counts"), or its raw form ("words": the byte pool, "word_off", "counts", and
        "terminator" if the pool has one).  -> {"tokens": [str...], "scores": np.int64[...], "thresh": int}; the tokens
        are the lines of a vocab.txt.  slack: entries the list may stay below vocab_size (default: slack_ratio * vocab_size)."""
        counts = np.ascontiguousarray(table["counts"], dtype=np.int64)
        if "word_off" in table:
            pool = np.ascontiguousarray(table["words"], dtype=np.uint8)
            off = np.ascontiguousarray(table["word_off"], dtype=np.int64)
            terminator = table.get("terminator")
        else:
            ws = [_bytes(w) for w in table["words"]]
            pool = np.frombuffer(b"".join(ws), dtype=np.uint8)
            off = _offsets_of([len(w) for w in ws])
            terminator = None
        n = len(off) - 1
        if n < 0 or len(counts) != n:
            raise WordPieceError("learn: word_off needs one entry more than counts")
        if n and off[n] > pool.size:  # (the library reads word_off[n] bytes of the pool)
            raise WordPieceError("learn: word_off ends behind the pool")
        spec, keep = self._learn_spec(vocab_size, reserved, lower_thresh, upper_thresh, num_iterations, max_token_chars, max_unique_chars,
                                      slack_ratio, slack, terminator, hash_bits)
        out = LearnedVocab()
        _check(lib().wp_learn_vocab(self._h, pool.ctypes.data if pool.size else None, off.ctypes.data if n else None,
                                    counts.ctypes.data if n else None, n, C.byref(spec), C.byref(out)))
        res = _host_result("learn", out)
        data, toff = res["tokens"].tobytes(), res.pop("token_off")
        res["tokens"] = [data[toff[j]:toff[j + 1] - 1].decode("utf8") for j in range(len(toff) - 1)]
        res["thresh"] = int(out.thresh)
        return res

    def learn_vocab_tensor(self, words, word_off, counts, vocab_size, reserved=DEFAULT_RESERVED, lower_thresh=10, upper_thresh=10_000_000,
                           num_iterations=4, max_token_chars=50, max_unique_chars=1000, slack_ratio=0.05, slack=None, terminator=None,
                           hash_bits=0, copy=True):
        """learn_vocab for a table in tensors on this handle's GPU, as count_words_tensor gives it (wp_learn_vocab_device)
        -> {"tokens": uint8 text of the list, every token followed by a line feed, "token_off": int64 [n + 1], "scores":
        int64 [n], "thresh": int}, tensors on that device.  copy=False: views of the library's buffers, valid until the
        next learn call on this handle."""
        import torch
        if words.dtype != torch.uint8 or word_off.dtype != torch.int64 or counts.dtype != torch.int64:
            raise WordPieceError("learn_vocab_tensor needs uint8 words and int64 word_off and counts")
        for t in (words, word_off, counts):
            if not t.is_cuda or not t.is_contiguous():
                raise WordPieceError("learn_vocab_tensor needs contiguous CUDA/HIP tensors")
        n = word_off.numel() - 1
        if n < 0 or counts.numel() != n:
            raise WordPieceError("learn: word_off needs one entry more than counts")
        spec, keep = self._learn_spec(vocab_size, reserved, lower_thresh, upper_thresh, num_iterations, max_token_chars, max_unique_chars,
                                      slack_ratio, slack, terminator, hash_bits)
        torch.cuda.current_stream(words.device).synchronize()  # the library runs on its own HIP streams
        out = LearnedVocab()
        _check(lib().wp_learn_vocab_device(self._h, C.c_void_p(words.data_ptr()) if words.numel() else None, words.numel(),
                                           C.c_void_p(word_off.data_ptr()), C.c_void_p(counts.data_ptr()) if n else None, n,
                                           C.byref(spec), C.byref(out)))
        res = _layer_result("learn", out, _DeviceViews(words.device, copy))
        res["thresh"] = int(out.thresh)
        return res

    def _rows_host(self, layer, spec, batches, on, raw=False, **sizes):
        """The host form of a ragged-batch layer: its entry point over the batches _ragged_batch returned -> the dict of
        its arrays (_RESULTS), text as bytes unless raw."""
        data, off, n = batches[0]
        out = _CORPUS_LAYERS[layer][2]()
        args = [a for d, o, k in batches for a in (d.ctypes.data if d.size else None, o.ctypes.data if k else None, k)]
        _check(getattr(lib(), _CORPUS_LAYERS[layer][0])(self._h, *args, C.byref(spec), C.byref(out)))
        text = data.dtype == np.uint8
        res = _host_result(layer, out, on, "u8" if text else "i32", rows=n, ref=batches[-1][-1], elems=int(off[n]) if n else 0, **sizes)
        if text and not raw:
            res.update((k, res[k].tobytes()) for k in ("data", "cut_data") if k in res)
        return res

    def _rows_device(self, layer, spec, batches, on, copy, **sizes):
        """The tensor form of a ragged-batch layer: its device entry point over the batches _ragged_tensors returned -> the
        dict of its arrays (_RESULTS) as tensors on the batch's device."""
        data, nbytes, row_off, n = batches[0]
        out = _CORPUS_LAYERS[layer][2]()
        args = [a for d, nb, o, k in batches for a in (C.c_void_p(d.data_ptr()) if nb else None, C.c_void_p(o.data_ptr()), k)]
        _check(getattr(lib(), _CORPUS_LAYERS[layer][0] + "_device")(self._h, *args, C.byref(spec), C.byref(out)))
        n_elems = nbytes // data.element_size()
        return _layer_result(layer, out, _DeviceViews(data.device, copy), on, "u8" if data.element_size() == 1 else "i32", rows=n,
                             ref=batches[-1][-1], elems=lambda: min(n_elems, int(row_off[n])) if n else 0, **sizes)

    def dedup_stats(self):
        """wp_dedup_stats of the last dedup call as a dict (n_rows -1: no such call yet)."""
        return self._stats(DedupStats, "wp_get_dedup_stats")

    @staticmethod
    def _dedup_spec(elem_bytes, inverse, compact, hash_bits):
        want = (WP_DEDUP_WANT_INVERSE if inverse else 0) | (WP_DEDUP_WANT_COMPACT if compact else 0)
        return DedupSpec(elem_bytes, want, int(hash_bits), 0)

    def dedup_rows(self, data, row_off=None, inverse=False, compact=False, hash_bits=0, raw=False):
        """The duplicate rows of a ragged batch dropped on the device, exactly (wp_dedup_rows).  data: bytes / str / a
        uint8 array (text, one byte per element) or an int32 array (ids); row_off: int64 [n_rows + 1] in elements,
        ascending from 0 — or None for the lines form of a text: a row per line, its line feed included, one appended
        where the text does not end in one.  -> {"first": np.int32 [n_rows], "kept": np.int32 [n_unique], "counts":
        np.int64 [n_unique]}, with inverse "inverse": np.int32 [n_rows] (first[i] == kept[inverse[i]]), with compact
        "data" and "row_off" of the kept rows back to back.  raw: text data comes back as np.uint8 rather than bytes.
        hash_bits: for tests of the collision rounds."""
        batch = _ragged_batch("dedup", data, row_off)
        spec = self._dedup_spec(batch[0].dtype.itemsize, inverse, compact, hash_bits)
        return self._rows_host("dedup", spec, [batch], dict(inverse=inverse, compact=compact), raw)

    def dedup_rows_tensor(self, data, row_off, inverse=False, compact=False, copy=True, hash_bits=0):
        """dedup_rows for a batch in tensors on this handle's GPU (wp_dedup_rows_device): data uint8 (text) or int32
        (ids), row_off int64 [n_rows + 1] — the ids and row_splits of encode_rows_tensor, a joined text and its doc_off,
        the words and word_off of count_words_tensor.  -> a dict of tensors on that device: "first", "kept", "counts",
        with inverse "inverse", with compact "data" and "row_off" (what encode_rows_tensor and pack_sequences_tensor
        take).  copy=False: views of the library's buffers, valid until the next call on this handle."""
        batches = _ragged_tensors("dedup", self._device, [(data, row_off)])
        spec = self._dedup_spec(data.element_size(), inverse, compact, hash_bits)
        return self._rows_device("dedup", spec, batches, dict(inverse=inverse, compact=compact), copy)

    def dedup_docs(self, docs):
        """The documents of a list (str / bytes) without their repeats, in order of first occurrence, and how often each
        occurred -> ([documents as given: str or bytes], np.int64 counts); through join_docs and dedup_rows."""
        docs = list(docs)
        text, off = join_docs(docs)
        r = self.dedup_rows(text, off)
        return [docs[k] for k in r["kept"]], r["counts"]

    def neardup_stats(self):
        """wp_neardup_stats of the last neardup call as a dict (n_rows -1: no such call yet)."""
        return self._stats(NearDupStats, "wp_get_neardup_stats")

    @staticmethod
    def _neardup_spec(elem_bytes, shingle, n_perm, bands, min_agree, seed, inverse, compact, signatures):
        want = (WP_NEARDUP_WANT_INVERSE if inverse else 0) | (WP_NEARDUP_WANT_COMPACT if compact else 0) | \
            (WP_NEARDUP_WANT_SIGNATURES if signatures else 0)
        return NearDupSpec(elem_bytes, want, int(shingle), int(n_perm), int(bands), int(min_agree), int(seed) & (2 ** 64 - 1), (C.c_int32 * 2)(0, 0))

    def neardup_rows(self, data, row_off=None, shingle=5, n_perm=128, bands=16, min_agree=0, seed=0, inverse=False, compact=False,
                     signatures=False, raw=False):
        """The rows of a ragged batch clustered into near-duplicates on the device (wp_neardup_rows): MinHash signatures
        of n_perm permutations over shingles of `shingle` elements, LSH over `bands` bands, a member of a bucket joined to
        the bucket's first row where at least min_agree signature slots agree (lsh_min_agree turns a Jaccard threshold
        into that number), clusters = connected components.  data and row_off as dedup_rows takes them (row_off None:
        the lines of a text).  -> {"cluster": np.int32 [n_rows] (the smallest row of the cluster), "kept": np.int32
        [n_unique], "counts": np.int64 [n_unique]}, with inverse "inverse", with compact "data" and "row_off" of the kept
        rows back to back, with signatures "signatures": np.uint32 [n_rows, n_perm].  raw: text data comes back as
        np.uint8 rather than bytes."""
        batch = _ragged_batch("neardup", data, row_off)
        spec = self._neardup_spec(batch[0].dtype.itemsize, shingle, n_perm, bands, min_agree, seed, inverse, compact, signatures)
        return self._rows_host("neardup", spec, [batch], dict(inverse=inverse, compact=compact, signatures=signatures), raw, n_perm=int(n_perm))

    def neardup_rows_tensor(self, data, row_off, shingle=5, n_perm=128, bands=16, min_agree=0, seed=0, inverse=False, compact=False,
                            signatures=False, copy=True):
        """neardup_rows for a batch in tensors on this handle's GPU (wp_neardup_rows_device): data uint8 (text) or int32
        (ids), row_off int64 [n_rows + 1] — the ids and row_splits of encode_rows_tensor, the compact form of
        dedup_rows_tensor, a joined text and its doc_off.  -> a dict of tensors on that device: "cluster", "kept",
        "counts", with inverse "inverse", with compact "data" and "row_off" (what pack_sequences_tensor takes), with
        signatures "signatures" (int32 bit patterns of the uint32 values, [n_rows, n_perm]: torch has no uint32
        arithmetic; .cpu().numpy().view(np.uint32) reads them).  copy=False: views of the library's buffers, valid until
        the next call on this handle."""
        batches = _ragged_tensors("neardup", self._device, [(data, row_off)])
        spec = self._neardup_spec(data.element_size(), shingle, n_perm, bands, min_agree, seed, inverse, compact, signatures)
        return self._rows_device("neardup", spec, batches, dict(inverse=inverse, compact=compact, signatures=signatures), copy, n_perm=int(n_perm))

    def neardup_docs(self, docs, **kw):
        """The documents of a list (str / bytes) without their near-duplicates: the first document of every cluster, in
        order, and the sizes of the clusters -> ([documents as given], np.int64 counts); through join_docs and
        neardup_rows, whose keyword arguments (shingle, n_perm, bands, min_agree, seed) pass through."""
        docs = list(docs)
        text, off = join_docs(docs)
        r = self.neardup_rows(text, off, **kw)
        return [docs[k] for k in r["kept"]], r["counts"]

    def overlap_stats(self):
        """wp_overlap_stats of the last overlap call as a dict (n_rows -1: no such call yet)."""
        return self._stats(OverlapStats, "wp_get_overlap_stats")

    @staticmethod
    def _overlap_spec(elem_bytes, ngram, max_hits, mask, ref, compact, hash_bits):
        want = (WP_OVERLAP_WANT_MASK if mask else 0) | (WP_OVERLAP_WANT_REF if ref else 0) | (WP_OVERLAP_WANT_COMPACT if compact else 0)
        return OverlapSpec(elem_bytes, want, int(ngram), int(max_hits), int(hash_bits), (C.c_int32 * 3)(0, 0, 0))

    @staticmethod
    def _overlap_batch(data, row_off, name):
        """one batch of a host overlap call, and the batch of a repeat call, whose messages read the same"""
        return _ragged_batch("overlap", data, row_off, name, "the offsets of " + name, "")

    def overlap_rows(self, data, row_off, ref_data, ref_off, ngram=13, max_hits=0, mask=False, ref=False, compact=False, hash_bits=0,
                     raw=False):
        """The rows of a ragged batch that share an n-gram with a reference set, found on the device, exactly
        (wp_overlap_rows).  data / row_off: the corpus, ref_data / ref_off: the reference set, each as dedup_rows takes a
        batch (text or int32 ids, the same kind for both; offsets None: the lines of a text).  A window is `ngram`
        consecutive elements of a row.  -> {"hits": np.int64 [n_rows] (the windows of the row that equal a reference
        window), "first_hit": np.int64 (the first such position, or -1), "first_ref": np.int32 (the smallest reference
        row that holds it, or -1), "covered": np.int64 (the elements inside a hitting window)}, with mask "mask": np.uint8
        per element, with ref "ref_hits": np.int64 [n_ref] (the windows of a reference row found in the corpus), with
        compact "kept": np.int32 (the rows with hits <= max_hits) and their "data" and "row_off" back to back.  raw: text
        data comes back as np.uint8 rather than bytes.  hash_bits: for tests of key collisions."""
        batches = [self._overlap_batch(data, row_off, "data"), self._overlap_batch(ref_data, ref_off, "ref_data")]
        if batches[0][0].dtype != batches[1][0].dtype:
            raise WordPieceError("overlap: data and ref_data must both be text or both be ids")
        spec = self._overlap_spec(batches[0][0].dtype.itemsize, ngram, max_hits, mask, ref, compact, hash_bits)
        return self._rows_host("overlap", spec, batches, dict(mask=mask, ref=ref, compact=compact), raw)

    def overlap_rows_tensor(self, data, row_off, ref_data, ref_off, ngram=13, max_hits=0, mask=False, ref=False, compact=False, copy=True,
                            hash_bits=0):
        """overlap_rows for batches in tensors on this handle's GPU (wp_overlap_rows_device): data and ref_data uint8
        (text) or int32 (ids), row_off and ref_off int64 — the ids and row_splits of encode_rows_tensor, the compact
        forms of dedup_rows_tensor and neardup_rows_tensor, a joined text and its doc_off.  -> a dict of tensors on that
        device: "hits", "first_hit", "first_ref", "covered", with mask "mask" (torch.uint8), with ref "ref_hits", with
        compact "kept", "data" and "row_off" (what pack_sequences_tensor takes).  copy=False: views of the library's
        buffers, valid until the next call on this handle."""
        batches = _ragged_tensors("overlap", self._device, [(data, row_off), (ref_data, ref_off)], offsets="offsets", s="")
        spec = self._overlap_spec(data.element_size(), ngram, max_hits, mask, ref, compact, hash_bits)
        return self._rows_device("overlap", spec, batches, dict(mask=mask, ref=ref, compact=compact), copy)

    def overlap_docs(self, docs, ref_docs, ngram=13, max_hits=0):
        """The documents of a list (str / bytes) that share at most max_hits windows of `ngram` bytes with the documents
        of ref_docs -> ([those documents as given], np.int64 hits of every document of docs); through join_docs and
        overlap_rows."""
        docs, ref_docs = list(docs), list(ref_docs)
        text, off = join_docs(docs)
        ref_text, ref_off = join_docs(ref_docs)
        r = self.overlap_rows(text, off, ref_text, ref_off, ngram=ngram, max_hits=max_hits, compact=True)
        return [docs[k] for k in r["kept"]], r["hits"]

    def repeat_stats(self):
        """wp_repeat_stats of the last repeat call as a dict (n_rows -1: no such call yet)."""
        return self._stats(RepeatStats, "wp_get_repeat_stats")

    @staticmethod
    def _repeat_spec(elem_bytes, ngram, scope, max_repeats, mask, src, compact, cut, utf8, hash_bits):
        want = (WP_REPEAT_WANT_MASK if mask else 0) | (WP_REPEAT_WANT_SRC if src else 0) | (WP_REPEAT_WANT_COMPACT if compact else 0) | \
            (WP_REPEAT_WANT_CUT if cut else 0)
        if utf8 is None:  # (on for text, off for ids)
            utf8 = elem_bytes == 1
        return RepeatSpec(elem_bytes, want, int(ngram), int(scope), int(max_repeats), int(hash_bits), WP_REPEAT_UTF8 if utf8 else 0, 0)

    def repeat_rows(self, data, row_off, ngram=50, scope=0, max_repeats=0, mask=False, src=False, compact=False, cut=False, utf8=None,
                    hash_bits=0, lines=False):
        """The spans a ragged batch repeats, found on the device, exactly, and cut out there (wp_repeat_rows).  data /
        row_off: the batch as dedup_rows takes it (text or int32 ids; lines=True, or offsets None: the lines of a text).
        A window is `ngram` consecutive elements of a row; it is a repeat where an equal window begins at a smaller flat
        position (scope 0) or in an earlier row (scope 1).  -> {"repeats": np.int64 [n_rows], "first_repeat": np.int64
        (the first repeating position, or -1), "first_src_row": np.int32 and "first_src_pos": np.int64 (where that window
        first occurred, or -1), "covered": np.int64 (the elements inside a repeat window)}, with mask "mask": np.uint8 per
        element, with src "src": np.int64 per element (the flat position of the first occurrence of a repeat, else -1),
        with compact "kept": np.int32 (the rows with repeats <= max_repeats) and their "data" and "row_off" back to
        back, with cut "cut_data" and "cut_off": every row without its covered elements.  utf8 (None: on for text, off
        for ids): windows begin and end at code point boundaries, so the cut of valid UTF-8 is valid.  Text comes back as
        bytes.  hash_bits: for tests of key collisions."""
        if lines and row_off is not None:
            raise WordPieceError("repeat: the lines form takes no offsets")
        batch = self._overlap_batch(data, row_off, "data")
        spec = self._repeat_spec(batch[0].dtype.itemsize, ngram, scope, max_repeats, mask, src, compact, cut, utf8, hash_bits)
        return self._rows_host("repeat", spec, [batch], dict(mask=mask, src=src, compact=compact, cut=cut))

    def repeat_rows_tensor(self, data, row_off, ngram=50, scope=0, max_repeats=0, mask=False, src=False, compact=False, cut=False, utf8=None,
                           hash_bits=0, copy=True):
        """repeat_rows for a batch in tensors on this handle's GPU (wp_repeat_rows_device): data uint8 (text) or int32
        (ids), row_off int64 — the ids and row_splits of encode_rows_tensor, the compact form of dedup_rows_tensor, a
        joined text and its doc_off.  -> a dict of tensors on that device with the keys of repeat_rows; "data" + "row_off"
        and "cut_data" + "cut_off" are what pack_sequences_tensor takes.  copy=False: views of the library's buffers,
        valid until the next call on this handle."""
        batches = _ragged_tensors("repeat", self._device, [(data, row_off)], offsets="offsets", s="")
        spec = self._repeat_spec(data.element_size(), ngram, scope, max_repeats, mask, src, compact, cut, utf8, hash_bits)
        return self._rows_device("repeat", spec, batches, dict(mask=mask, src=src, compact=compact, cut=cut), copy)

    def repeat_docs(self, docs, ngram=50, scope=0):
        """The documents of a list (str / bytes) with the spans cut out that occurred before in the list (windows of
        `ngram` bytes, at code point boundaries) -> ([the documents, each of the type it was given in], np.int64 covered
        bytes of every document, the line feed of the join included where a span takes it along); through join_docs and
        repeat_rows."""
        docs = list(docs)
        text, off = join_docs(docs)
        r = self.repeat_rows(text, off, ngram=ngram, scope=scope, mask=True, cut=True)
        co = r["cut_off"]
        out = []
        for i, d in enumerate(docs):
            b = r["cut_data"][int(co[i]):int(co[i + 1])]
            if not r["mask"][int(off[i + 1]) - 1]:  # (the line feed of the join is still there)
                b = b[:-1]
            out.append(b.decode("utf8") if isinstance(d, str) else b)
        return out, r["covered"]

    def quality_stats(self):
        """wp_quality_stats of the last quality call as a dict (n_rows -1: no such call yet; rule_failed: a list by rule)."""
        return self._stats(QualityStats, "wp_get_quality_stats")

    @staticmethod
    def _quality_spec(rules, stop_words, short_line_chars, dup_lines, compact):
        """-> (QualitySpec, what it points into).  rules: {rule name: threshold}, and "stop_words" among them as a preset has it"""
        rules = quality_rules(rules) if isinstance(rules, str) else dict(rules or {})
        if "stop_words" in rules:
            preset_stop = rules.pop("stop_words")
            stop_words = preset_stop if stop_words is None else stop_words
        limit = [-1] * len(QUALITY_RULES)
        for name, value in rules.items():
            if name not in QUALITY_RULES or name == "reserved":
                raise WordPieceError("quality: no such rule: %r" % (name,))
            limit[QUALITY_RULES.index(name)] = int(value)
        if dup_lines is None:  # (on where a rule needs it)
            dup_lines = limit[10] >= 0 or limit[11] >= 0
        words = [_bytes(w) for w in (stop_words or ())]
        pool = np.frombuffer(b"".join(words) + b"\0", dtype=np.uint8)
        off = _offsets_of([len(w) for w in words])
        want = (WP_QUALITY_WANT_DUP_LINES if dup_lines else 0) | (WP_QUALITY_WANT_COMPACT if compact else 0)
        spec = QualitySpec(1, want, int(short_line_chars), len(words), pool.ctypes.data if words else None, off.ctypes.data if words else None,
                           (C.c_int64 * 16)(*limit), 0)
        return spec, (pool, off)

    def quality_rows(self, data, row_off, rules=None, stop_words=None, short_line_chars=0, dup_lines=None, compact=False, raw=False):
        """The quality signals of every row of a ragged batch of text and the rules over them, on the device, exactly
        (wp_quality_rows).  data / row_off: the batch as dedup_rows takes it (offsets None: the lines of a text).  rules:
        {name of QUALITY_RULES: threshold} (quality_rules("gopher") is such a dict); stop_words: at most 64 lower-case
        words; short_line_chars (0: 30); dup_lines (None: on where a rule needs it): the duplicate-line signals.  ->
        {"signals": np.int64 [23, n_rows] (rows of QUALITY_SIGNALS), "reasons": np.uint32 [n_rows] (bit r: rule r
        failed)}, with compact "kept": np.int32 (the rows that failed no rule) and their "data" and "row_off" back to
        back.  raw: the data comes back as np.uint8 rather than bytes."""
        batch = _ragged_batch("quality", data, row_off)
        if batch[0].dtype != np.uint8:
            raise WordPieceError("quality: data must be text")
        spec, keep = self._quality_spec(rules, stop_words, short_line_chars, dup_lines, compact)
        return self._rows_host("quality", spec, [batch], dict(compact=compact), raw, n_signals=len(QUALITY_SIGNALS))

    def quality_rows_tensor(self, data, row_off, rules=None, stop_words=None, short_line_chars=0, dup_lines=None, compact=False, copy=True):
        """quality_rows for a batch in tensors on this handle's GPU (wp_quality_rows_device): data uint8, row_off int64 — a
        joined text and its doc_off, the compact form of another layer.  -> a dict of tensors on that device: "signals"
        (torch.int64 [23, n_rows]), "reasons" (the uint32 bitmasks as torch.int32), with compact "kept", "data" and
        "row_off" (what dedup_rows_tensor and, once encoded, pack_sequences_tensor take).  copy=False: views of the
        library's buffers, valid until the next call on this handle."""
        batches = _ragged_tensors("quality", self._device, [(data, row_off)], ids=False, offsets="offsets", s="")
        spec, keep = self._quality_spec(rules, stop_words, short_line_chars, dup_lines, compact)
        return self._rows_device("quality", spec, batches, dict(compact=compact), copy, n_signals=len(QUALITY_SIGNALS))

    def quality_docs(self, docs, rules=None, stop_words=None, short_line_chars=0):
        """The documents of a list (str / bytes) that fail none of `rules` -> ([those documents as given], np.uint32
        reasons of every document of docs); through quality_rows over the documents back to back (no byte is added)."""
        docs = list(docs)
        bs = [_bytes(d) for d in docs]
        r = self.quality_rows(b"".join(bs), _offsets_of([len(b) for b in bs]), rules=rules, stop_words=stop_words, short_line_chars=short_line_chars)
        return [d for d, x in zip(docs, r["reasons"]) if x == 0], r["reasons"]

    def align_stats(self):
        """wp_align_stats of the last call as a dict (n_rows -1: it was no align call)."""
        return self._stats(AlignStats, "wp_get_align_stats")

    def align_spans(self, batch=None, spans=None, side=0, outside_label=0, inside_add=0, ignore_id=-100, no_answer=0,
                    labels=True, span_index=False, positions=False, offsets=None, token_type_ids=None, lengths=None,
                    sample=None):
        """Labelled character spans against a batch of model inputs (wp_align).  batch: the dict encode_inputs returns
        (its offsets, token_type_ids, lengths and sample are used unless others are given), or None with the arrays one
        by one: offsets uint32 [n_rows, max_len, 2], and optionally token_type_ids, lengths, sample.  spans: a list, per
        sample, of (begin, end[, label]) in the unit of the offsets — sorted, disjoint, non-empty — or what join_spans
        returns.  side: the sequence the spans label (1: B, the context of a question-first pair).
        -> a dict of numpy int32 arrays: labels [n_rows, max_len] (ignore_id where there is no token of that side,
        outside_label on a token no span overlaps, else the span's label, + inside_add unless the token starts at or
        before the span's begin), span_index (the flat index of the span, -1) and, with positions=True,
        start_positions / end_positions [n_rows] of the sample's first span (no_answer where the row does not hold it
        whole)."""
        offs, types, lens, samp = _align_batch(batch, offsets, token_type_ids, lengths, sample, np.asarray)
        offs = np.ascontiguousarray(offs, dtype=np.uint32)
        if offs.ndim != 3 or offs.shape[2] != 2:
            raise WordPieceError("offsets must be a 3-d array [n_rows, max_len, 2]")
        n_rows, L = offs.shape[0], offs.shape[1]
        types = None if types is None else np.ascontiguousarray(types, dtype=np.int32)
        lens = None if lens is None else np.ascontiguousarray(lens, dtype=np.int32)
        samp = None if samp is None else np.ascontiguousarray(samp, dtype=np.int32)
        if (types is not None and types.shape != (n_rows, L)) or any(x is not None and x.shape != (n_rows,) for x in (lens, samp)):
            raise WordPieceError("token_type_ids must be [n_rows, max_len], lengths and sample [n_rows]")
        splits, sp, sl = _spans_arg(spans)
        spec = AlignSpec(max_len=L, side=side, outside_label=outside_label, inside_add=inside_add, ignore_id=ignore_id,
                         no_answer=no_answer, want=_align_want(labels, span_index, positions))
        i32p = C.POINTER(C.c_int32)
        o_lab, o_idx, o_start, o_end = i32p(), i32p(), i32p(), i32p()
        _check(lib().wp_align(self._h, offs.ctypes.data_as(C.POINTER(C.c_uint32)), _i32_ptr(types), _i32_ptr(lens), _i32_ptr(samp),
                              n_rows, _i64_ptr(splits), len(splits) - 1, sp.ctypes.data_as(C.POINTER(C.c_uint32)), _i32_ptr(sl),
                              len(sp), C.byref(spec), C.byref(o_lab), C.byref(o_idx), C.byref(o_start), C.byref(o_end)))
        res = {}
        for want, key, ptr, shape in ((labels, "labels", o_lab, (n_rows, L)), (span_index, "span_index", o_idx, (n_rows, L)),
                                      (positions, "start_positions", o_start, (n_rows,)),
                                      (positions, "end_positions", o_end, (n_rows,))):
            if want:
                res[key] = _adopt_block(ptr, shape) if n_rows else np.zeros(shape, np.int32)
        return res

    def align_rows(self, offsets, row_splits, spans, outside_label=0, inside_add=0, labels=True, span_index=False):
        """The same cell rule over the ragged result of encode_rows (wp_align_rows): offsets uint32 [n_ids, 2], row_splits
        [n_rows + 1]; row i is sample i and every cell is a token -> a dict of numpy int32 arrays [n_ids]: labels,
        span_index.  x[source] of a packed batch carries them into it."""
        offs = np.ascontiguousarray(offsets, dtype=np.uint32).reshape(-1, 2)
        rows = np.ascontiguousarray(row_splits, dtype=np.int64)
        if rows.ndim != 1 or len(rows) < 1:
            raise WordPieceError("row_splits must be a 1-d array of n_rows + 1 entries")
        if rows[-1] > len(offs):
            raise WordPieceError("row_splits end behind the offsets")
        splits, sp, sl = _spans_arg(spans)
        if len(splits) != len(rows):
            raise WordPieceError("the ragged form needs one list of spans per row")
        spec = AlignSpec(outside_label=outside_label, inside_add=inside_add, want=_align_want(labels, span_index, False))
        i32p = C.POINTER(C.c_int32)
        o_lab, o_idx = i32p(), i32p()
        _check(lib().wp_align_rows(self._h, offs.ctypes.data_as(C.POINTER(C.c_uint32)), _i64_ptr(rows), len(rows) - 1, _i64_ptr(splits),
                                   sp.ctypes.data_as(C.POINTER(C.c_uint32)), _i32_ptr(sl), len(sp), C.byref(spec), C.byref(o_lab),
                                   C.byref(o_idx)))
        n = int(rows[-1])
        res = {}
        for want, key, ptr in ((labels, "labels", o_lab), (span_index, "span_index", o_idx)):
            if want:
                res[key] = _adopt_block(ptr, (n,)) if n else np.zeros(0, np.int32)
        return res

    def _align_tensor_spans(self, spans, dev):
        """(span_splits int64, spans uint32-as-int32 [n, 2], span_labels int32) as contiguous tensors on dev"""
        import torch
        if not (isinstance(spans, tuple) and len(spans) == 3 and all(isinstance(x, torch.Tensor) for x in spans)):
            splits, sp, sl = _spans_arg(spans)
            spans = (torch.from_numpy(splits), torch.from_numpy(sp.view(np.int32)), torch.from_numpy(sl))
        splits, sp, sl = (x.to(dev) for x in spans)
        if sp.dtype == torch.uint32:
            sp = sp.view(torch.int32)
        if splits.dtype != torch.int64 or sp.dtype != torch.int32 or sl.dtype != torch.int32 or splits.dim() != 1 or \
                splits.numel() < 1 or sp.shape != (sl.numel(), 2) or sl.dim() != 1:
            raise WordPieceError("spans on tensors: span_splits int64 [n_samples + 1], spans int32 / uint32 [n_spans, 2], "
                                 "span_labels int32 [n_spans]")
        return splits.contiguous(), sp.contiguous(), sl.contiguous()

    def align_spans_tensor(self, batch=None, spans=None, side=0, outside_label=0, inside_add=0, ignore_id=-100, no_answer=0,
                           labels=True, span_index=False, positions=False, offsets=None, token_type_ids=None, lengths=None,
                           sample=None):
        """align_spans for tensors on this handle's GPU (wp_align_device): batch is the dict encode_inputs_tensor returns
        (or the tensors one by one: offsets int32 / uint32 [n_rows, max_len, 2], ...), spans what join_spans returns — as
        tensors, or as numpy arrays / a list of lists, which are uploaded -> a dict of int32 tensors there.  Nothing
        leaves the device."""
        import torch
        offs, types, lens, samp = _align_batch(batch, offsets, token_type_ids, lengths, sample, lambda x: x)
        if offs.dtype == torch.uint32:
            offs = offs.view(torch.int32)
        if offs.dtype != torch.int32 or not offs.is_cuda or not offs.is_contiguous() or offs.dim() != 3 or offs.shape[2] != 2:
            raise WordPieceError("align on tensors needs contiguous int32 / uint32 CUDA/HIP offsets [n_rows, max_len, 2]")
        dev, (n_rows, L) = offs.device, offs.shape[:2]
        if self._device is not None and dev.index != self._device:  # (raw pointers go to the handle's device)
            raise WordPieceError("the tensors lie on %s, the handle on device %d" % (dev, self._device))
        for x, shape, name in ((types, (n_rows, L), "token_type_ids"), (lens, (n_rows,), "lengths"), (samp, (n_rows,), "sample")):
            if x is not None and (x.dtype != torch.int32 or x.device != dev or not x.is_contiguous() or tuple(x.shape) != shape):
                raise WordPieceError("%s must be a contiguous int32 tensor %s on the device of the offsets" % (name, list(shape)))
        splits, sp, sl = self._align_tensor_spans(spans, dev)
        spec = AlignSpec(max_len=L, side=side, outside_label=outside_label, inside_add=inside_add, ignore_id=ignore_id,
                         no_answer=no_answer, want=_align_want(labels, span_index, positions))
        res = {}
        if labels:
            res["labels"] = torch.empty((n_rows, L), dtype=torch.int32, device=dev)
        if span_index:
            res["span_index"] = torch.empty((n_rows, L), dtype=torch.int32, device=dev)
        if positions:
            res["start_positions"] = torch.empty(n_rows, dtype=torch.int32, device=dev)
            res["end_positions"] = torch.empty(n_rows, dtype=torch.int32, device=dev)
        if n_rows == 0:  # (nothing to write, and an empty tensor has no address to name an output by)
            return res
        torch.cuda.current_stream(dev).synchronize()  # the library runs on its own HIP streams
        _check(lib().wp_align_device(self._h, _tensor_ptr(offs), _tensor_ptr(types), _tensor_ptr(lens), _tensor_ptr(samp), n_rows,
                                     _tensor_ptr(splits), splits.numel() - 1, _tensor_ptr(sp), _tensor_ptr(sl), sl.numel(),
                                     C.byref(spec), *[_tensor_ptr(res.get(k)) for k in ("labels", "span_index", "start_positions",
                                                                                        "end_positions")]))
        return res

    def align_rows_tensor(self, offsets, row_splits, spans, outside_label=0, inside_add=0, labels=True, span_index=False):
        """align_rows for tensors on this handle's GPU (wp_align_rows_device): offsets int32 / uint32 [n_ids, 2] and
        row_splits int64 [n_rows + 1] as encode_rows_tensor returns them -> a dict of int32 tensors [n_ids] there."""
        import torch
        offs = offsets.view(torch.int32) if offsets.dtype == torch.uint32 else offsets
        if offs.dtype != torch.int32 or not offs.is_cuda or not offs.is_contiguous() or offs.dim() != 2 or offs.shape[1] != 2:
            raise WordPieceError("align on tensors needs contiguous int32 / uint32 CUDA/HIP offsets [n_ids, 2]")
        dev, n = offs.device, offs.shape[0]
        if self._device is not None and dev.index != self._device:
            raise WordPieceError("the tensors lie on %s, the handle on device %d" % (dev, self._device))
        if row_splits.dtype != torch.int64 or row_splits.device != dev or row_splits.dim() != 1 or row_splits.numel() < 1 or \
                not row_splits.is_contiguous():
            raise WordPieceError("row_splits must be a contiguous 1-d int64 tensor on the device of the offsets")
        splits, sp, sl = self._align_tensor_spans(spans, dev)
        spec = AlignSpec(outside_label=outside_label, inside_add=inside_add, want=_align_want(labels, span_index, False))
        res = {}
        if labels:
            res["labels"] = torch.empty(n, dtype=torch.int32, device=dev)
        if span_index:
            res["span_index"] = torch.empty(n, dtype=torch.int32, device=dev)
        if n == 0:
            return res
        torch.cuda.current_stream(dev).synchronize()  # the library runs on its own HIP streams
        _check(lib().wp_align_rows_device(self._h, _tensor_ptr(offs), _tensor_ptr(row_splits), row_splits.numel() - 1, n,
                                          _tensor_ptr(splits), _tensor_ptr(sp), _tensor_ptr(sl), sl.numel(), C.byref(spec),
                                          _tensor_ptr(res.get("labels")), _tensor_ptr(res.get("span_index"))))
        return res

    def special_stats(self):
        """wp_special_stats of the last special-tokens call as a dict (n_literals -1: no such call yet)."""
        return self._stats(SpecialStats, "wp_get_special_stats")

    def special_ids(self, tokens=None):
        """Strings -> ids for the special_ids= of the encode_special calls.  tokens=None: every line that may be listed
        (a "[...]" line the vocabulary flags as special, at most 64 bytes of 0x21..0x7E, no further bracket), the first
        copy of a line that repeats.  A string that is no such line raises."""
        table = getattr(self, "_special_lines", None)
        if table is None:
            table = {}
            for i in range(len(self)):
                if (self.token_flags(i) & 6) == 2:
                    w = self.token_utf8(i)
                    if len(w) <= 64 and all(0x21 <= c <= 0x7E for c in w) and b"[" not in w[1:] and b"]" not in w[:-1]:
                        table.setdefault(w, i)
            self._special_lines = table
        if tokens is None:
            return sorted(table.values())
        out = []
        for t in tokens:
            if _bytes(t) not in table:
                raise WordPieceError("%r is no special token of the vocabulary that can be listed" % (t,))
            out.append(table[_bytes(t)])
        return out

    def _special_spec(self, special_ids):
        """-> (wp_special_spec, the array it points into)"""
        a = np.ascontiguousarray(self.special_ids() if special_ids is None else special_ids, dtype=np.int32)
        if a.ndim != 1:
            raise WordPieceError("special_ids must be a 1-d sequence of ids")
        return SpecialSpec(_i32_ptr(a) if len(a) else None, len(a)), a

    def encode_special(self, text, special_ids=None, offsets=None):
        """encode / encode_with_offsets that keeps special-token literals whole (wp_linear_encode_special): every listed
        line ("[MASK]", "[SEP]" ...) that stands in the text becomes its id, as HF's BertTokenizer does it; everything
        else is encoded as if the literal were blanks.  special_ids: ids (Vocab.special_ids(["[MASK]"])); None: every
        line that may be listed.  -> ids int32 [n], or with offsets="byte" / "char" (ids, offsets uint32 [n, 2])."""
        b = _bytes(text)
        spec, keep = self._special_spec(special_ids)
        unit = -1 if offsets is None else _offset_unit(offsets)
        ids, offs, n = C.POINTER(C.c_int32)(), C.POINTER(C.c_uint32)(), C.c_size_t()
        _check(lib().wp_linear_encode_special(self._h, b, len(b), C.byref(spec), unit, C.byref(ids), C.byref(offs), C.byref(n)))
        if offsets is None:
            return _adopt_ids(ids, n.value)
        return _adopt_ids(ids, n.value), (_adopt_block(offs, (n.value, 2)) if n.value else np.zeros((0, 2), dtype=np.uint32))

    def encode_special_rows(self, docs=None, text=None, doc_offsets=None, special_ids=None, offsets=None):
        """encode_rows that keeps special-token literals whole (wp_linear_encode_special_rows): row i is
        encode_special(document i).  Documents and results as in encode_rows, special_ids as in encode_special."""
        b, off = _docs_arg(docs, text, doc_offsets)
        spec, keep = self._special_spec(special_ids)
        unit = -1 if offsets is None else _offset_unit(offsets)
        ids, splits, offs = C.POINTER(C.c_int32)(), C.POINTER(C.c_int64)(), C.POINTER(C.c_uint32)()
        n, rows = C.c_size_t(), C.c_size_t()
        _check(lib().wp_linear_encode_special_rows(self._h, b, len(b), _i64_ptr(off), 0 if off is None else len(off) - 1,
                                                   C.byref(spec), unit, C.byref(ids), C.byref(splits), C.byref(offs), C.byref(n),
                                                   C.byref(rows)))
        out = (_adopt_ids(ids, n.value), _adopt_block(splits, (rows.value + 1,)))
        if offsets is None:
            return out
        return out + (_adopt_block(offs, (n.value, 2)) if n.value else np.zeros((0, 2), dtype=np.uint32),)

    def encode_special_tensor(self, text, special_ids=None, offsets=None, copy=True):
        """encode_special for a uint8 text tensor on this handle's GPU (wp_linear_encode_special_device) -> ids int32 [n]
        there, or (ids, offsets uint32 [n, 2]).  copy=False: views of the library's buffers, valid until the next call."""
        import torch
        text, nbytes, _ = self._rows_tensor_args(text, None)
        spec, keep = self._special_spec(special_ids)
        unit = -1 if offsets is None else _offset_unit(offsets)
        d_ids, d_offs, n = C.c_void_p(), C.c_void_p(), C.c_size_t()
        _check(lib().wp_linear_encode_special_device(self._h, C.c_void_p(text.data_ptr()), nbytes, C.byref(spec), unit,
                                                     C.byref(d_ids), C.byref(d_offs), C.byref(n)))
        dev = text.device
        ids = torch.as_tensor(DeviceIds(d_ids.value, n.value), device=dev) if n.value else torch.zeros(0, dtype=torch.int32, device=dev)
        if offsets is None:
            return ids.clone() if copy else ids
        offs = torch.as_tensor(DeviceIds(d_offs.value, n.value, cols=2), device=dev).view(torch.uint32) if n.value else \
            torch.zeros((0, 2), dtype=torch.uint32, device=dev)
        return (ids.clone(), offs.clone()) if copy else (ids, offs)

    def encode_special_rows_tensor(self, text, doc_offsets=None, special_ids=None, offsets=None, copy=True):
        """encode_special_rows for tensors on this handle's GPU (wp_linear_encode_special_rows_device): arguments and
        results of encode_rows_tensor, special_ids as in encode_special.  The result feeds pack_sequences_tensor,
        detokenize_tensor and, once padded, mask_inputs_tensor without leaving the device."""
        import torch
        text, nbytes, doc_offsets = self._rows_tensor_args(text, doc_offsets)
        spec, keep = self._special_spec(special_ids)
        unit = -1 if offsets is None else _offset_unit(offsets)
        d_ids, d_splits, d_offs = C.c_void_p(), C.c_void_p(), C.c_void_p()
        n, rows = C.c_size_t(), C.c_size_t()
        _check(lib().wp_linear_encode_special_rows_device(
            self._h, C.c_void_p(text.data_ptr()), nbytes, None if doc_offsets is None else C.c_void_p(doc_offsets.data_ptr()),
            0 if doc_offsets is None else doc_offsets.numel() - 1, C.byref(spec), unit, C.byref(d_ids), C.byref(d_splits),
            C.byref(d_offs), C.byref(n), C.byref(rows)))
        dev = text.device
        ids = torch.as_tensor(DeviceIds(d_ids.value, n.value), device=dev) if n.value else \
            torch.zeros(0, dtype=torch.int32, device=dev)
        splits = torch.as_tensor(DeviceIds(d_splits.value, rows.value + 1, typestr="<i8"), device=dev)
        out = (ids, splits)
        if offsets is not None:
            out += (torch.as_tensor(DeviceIds(d_offs.value, n.value, cols=2), device=dev).view(torch.uint32) if n.value else
                    torch.zeros((0, 2), dtype=torch.uint32, device=dev),)
        return tuple(t.clone() for t in out) if copy else out

    def fast_encode(self, text):
        """word_piece::fast::encode on the GPU (wp_fast_encode): host bytes/str -> numpy int32 ids."""
        b = _bytes(text)
        ids = C.POINTER(C.c_int32)()
        n = C.c_size_t()
        _check(lib().wp_fast_encode(self._h, b, len(b), C.byref(ids), C.byref(n)))
        return _adopt_ids(ids, n.value)

    def fast_encode_device(self, d_ptr, nbytes):
        d_ids = C.c_void_p()
        n = C.c_size_t()
        _check(lib().wp_fast_encode_device(self._h, C.c_void_p(d_ptr), nbytes, C.byref(d_ids), C.byref(n)))
        return d_ids.value, n.value

    def token_utf8(self, i):
        """Stored word of vocab line i as UTF-8 bytes (without "##"), or None."""
        n = lib().wp_vocab_token_utf8(self._h, i, None, 0)
        if n < 0:
            return None
        buf = C.create_string_buffer(max(n, 1))
        lib().wp_vocab_token_utf8(self._h, i, buf, n)
        return buf.raw[:n]

    def encode_multi(self, text, devices=None):
        """Host bytes -> numpy int32 ids, sharded over several GPUs behind the C ABI
        (wp_linear_encode_multi).  devices: list of HIP ordinals (may repeat), an int (the first k
        visible GPUs) or None (all visible GPUs)."""
        b = _bytes(text)
        ids = C.POINTER(C.c_int32)()
        n = C.c_size_t()
        if isinstance(devices, (list, tuple)):
            arr = (C.c_int * len(devices))(*devices)
            rc = lib().wp_linear_encode_multi(self._h, b, len(b), arr, len(devices), C.byref(ids), C.byref(n))
        else:
            rc = lib().wp_linear_encode_multi(self._h, b, len(b), None, int(devices or 0), C.byref(ids), C.byref(n))
        _check(rc)
        return _adopt_ids(ids, n.value)

    def encode_batch(self, texts):
        """A sequence of host texts through the shard pipeline (wp_linear_encode_batch): uploads, kernels and id
        downloads of neighbouring texts overlap.  Returns one numpy int32 array per text."""
        bs = [_bytes(t) for t in texts]
        k = len(bs)
        ptrs = (C.c_char_p * k)(*bs)
        sizes = (C.c_size_t * k)(*[len(b) for b in bs])
        ids = (C.POINTER(C.c_int32) * k)()
        ns = (C.c_size_t * k)()
        _check(lib().wp_linear_encode_batch(self._h, ptrs, sizes, k, ids, ns))
        return [_adopt_ids(C.cast(ids[i], C.POINTER(C.c_int32)), ns[i]) for i in range(k)]

    def encode_stream(self, texts, sink):
        """A corpus of any length through the shard pipeline with constant memory (wp_linear_encode_stream): `texts` is
        an iterable of bytes, `sink(index, ids)` receives each text's ids as a numpy view that is valid during the call
        only."""
        it = iter(texts)
        keep = {}

        @_TEXT_SOURCE
        def next_text(_user, index, out_ptr, out_len):
            try:
                b = _bytes(next(it))
            except StopIteration:
                return 0
            keep["text"] = b  # (the one before may go: the library asks for text i + 1 after text i has been uploaded)
            out_ptr[0] = C.cast(C.c_char_p(b), C.c_void_p).value
            out_len[0] = len(b)
            return 1

        @_IDS_SINK
        def got(_user, index, ids, n):
            sink(index, np.ctypeslib.as_array(ids, shape=(n,)) if n else np.zeros(0, dtype=np.int32))

        _check(lib().wp_linear_encode_stream(self._h, next_text, got, None))

    def reserve(self, nbytes):
        """Pre-sizes the device arenas and host staging for inputs of up to nbytes (wp_reserve)."""
        _check(lib().wp_reserve(self._h, int(nbytes)))

    def trim(self):
        """Releases this handle's device arenas, the parked contexts' arenas and the pooled id blocks (wp_trim)."""
        _check(lib().wp_trim(self._h))

    def encode_device(self, d_ptr, nbytes):
        """Text already in HBM at `d_ptr` -> (device pointer of int32 ids, count).  The id buffer is
        owned by the handle and valid until the next call."""
        d_ids = C.c_void_p()
        n = C.c_size_t()
        _check(lib().wp_linear_encode_device(self._h, C.c_void_p(d_ptr), nbytes, C.byref(d_ids), C.byref(n)))
        return d_ids.value, n.value

    def encode_tensor(self, text, copy=True, offsets=False, unit="byte"):
        """On-device consumer path: `text` is a uint8 torch tensor on the GPU of this
        handle; returns the ids as an int32 torch tensor on the same device.  copy=False returns a
        zero-copy view of the library's buffer, valid until the next call on this handle.
        offsets=True: returns (ids, offsets), offsets an (n, 2) tensor of [begin, end) per id in `unit`
        (encode_with_offsets) on the same device (copy=False: a uint32 view of the library's buffer).
        (Import torch before the first call into this package: both load a HIP runtime, and torch only
        sees the GPU through its own copy.)"""
        import torch
        if text.dtype != torch.uint8 or not text.is_cuda or not text.is_contiguous():
            raise WordPieceError("encode_tensor needs a contiguous uint8 CUDA/HIP tensor")
        (text, nbytes), = _whole_words(text)
        if offsets:
            d_ids, d_offs, n = self.encode_device_with_offsets(text.data_ptr(), nbytes, unit)
            if n == 0:
                return (torch.zeros(0, dtype=torch.int32, device=text.device),
                        torch.zeros((0, 2), dtype=torch.uint32, device=text.device))
            ids = torch.as_tensor(DeviceIds(d_ids, n), device=text.device)
            offs = torch.as_tensor(DeviceIds(d_offs, n, cols=2), device=text.device).view(torch.uint32)
            return (ids.clone(), offs.clone()) if copy else (ids, offs)
        d_ids, n = self.encode_device(text.data_ptr(), nbytes)
        if n == 0:
            return torch.zeros(0, dtype=torch.int32, device=text.device)
        view = torch.as_tensor(DeviceIds(d_ids, n), device=text.device)
        return view.clone() if copy else view

    def debug_fetch(self, which, capacity):
        out = np.zeros(max(capacity, 1), dtype=np.int32)
        n = C.c_size_t()
        _check(lib().wp_linear_debug_fetch(self._h, which, out.ctypes.data_as(C.POINTER(C.c_int32)), capacity,
                                           C.byref(n)))
        return out[:n.value]


def _adopt_ids(ids, n):
    """numpy view of the malloc'd id buffer the library returned (no copy); wp_free runs when the
    array (and every view of it) is gone."""
    if n == 0:
        return np.zeros(0, dtype=np.int32)
    return _adopt_block(ids, (n,))


def _adopt_block(ptr, shape):
    out = np.ctypeslib.as_array(ptr, shape=shape)
    weakref.finalize(out.base if out.base is not None else out, lib().wp_free, ptr)  # the bottom of the view chain
    return out


def normalize_cp(flags, cp):
    """The normalisation rule for one code point, from the tables the kernels read (wp_normalize_cp; no GPU needed):
    the list of 0..3 code points it gives, or None for a surrogate, a value >= 0x110000 or unknown flag bits."""
    out = (C.c_uint32 * 3)()
    n = lib().wp_normalize_cp(int(flags), int(cp), out)
    return None if n < 0 else [int(out[i]) for i in range(n)]


def join_docs(docs):
    """The joined form of a list of documents (str / bytes): every document followed by one "\\n" -> (bytes, int64
    offsets [n_docs + 1]); document i is bytes[offsets[i]:offsets[i + 1] - 1]."""
    bs = [_bytes(d) for d in docs]
    return b"".join(b + b"\n" for b in bs), _offsets_of([len(b) + 1 for b in bs])


def _offsets_of(lengths):
    """int64 offsets [n + 1] of n pieces back to back: 0, then the running sums of their lengths"""
    off = np.zeros(len(lengths) + 1, dtype=np.int64)
    if len(lengths):
        off[1:] = np.cumsum(lengths)
    return off


def _terminator_byte(prefix, terminator):
    """The terminator of a count, learn or detokenize call as the C ABI takes it: a one-byte str / bytes or an int -> that
    byte, None -> -1 (none).  prefix: the layer's name in front of the message; None: the detokenize calls' wording."""
    if terminator is None:
        return -1
    if not isinstance(terminator, (str, bytes, bytearray, memoryview)):
        return int(terminator)
    t = _bytes(terminator)
    if len(t) != 1:
        raise WordPieceError("%s: terminator must be one byte" % prefix if prefix else "the terminator is one byte")
    return t[0]


def line_rows(text):
    """The lines form of a text for the dedup calls: a row per line with its line feed, one appended where the text does
    not end in one -> (np.uint8 text, int64 row_off [n_lines + 1]).  The empty text has no line."""
    t = np.frombuffer(_bytes(text), dtype=np.uint8) if isinstance(text, (str, bytes, bytearray, memoryview)) else np.ascontiguousarray(text, dtype=np.uint8)
    if t.size and t[-1] != 10:
        t = np.concatenate((t, np.array([10], dtype=np.uint8)))
    ends = np.flatnonzero(t == 10).astype(np.int64) + 1
    return t, np.concatenate((np.zeros(1, dtype=np.int64), ends))


# ---- what the wrappers of the corpus layers share (count, learn, dedup, neardup, overlap, repeat, quality; both forms) --
def _ragged_batch(prefix, data, row_off, name="data", offsets="row_off", s="s"):
    """One batch of a host call -> (flat uint8 / int32 array, int64 offsets, n_rows).  name, offsets, s: what the layer's
    messages call the data and the offsets, and the ending of the verb behind the latter."""
    if isinstance(data, (str, bytes, bytearray, memoryview)):
        data = np.frombuffer(_bytes(data), dtype=np.uint8)
    else:
        data = np.ascontiguousarray(data)
    if data.dtype not in (np.uint8, np.int32) or data.ndim != 1:
        raise WordPieceError("%s: %s must be text (bytes, uint8) or a flat int32 array" % (prefix, name))
    if row_off is None:
        if data.dtype != np.uint8:
            raise WordPieceError("%s: the lines form takes text" % prefix)
        data, row_off = line_rows(data)
    off = np.ascontiguousarray(row_off, dtype=np.int64)
    n = off.size - 1
    if off.ndim != 1 or n < 0:
        raise WordPieceError("%s: %s need%s n_rows + 1 entries" % (prefix, offsets, s))
    if n and off[n] > data.size:  # (the library reads the last offset's elements of the data)
        raise WordPieceError("%s: %s end%s behind the data" % (prefix, offsets, s))
    return data, off, n


def _ragged_tensors(prefix, device, batches, ids=True, offsets="row_off", s="s"):
    """The batches [(data, offsets)] of a tensor call, as _ragged_batch takes those of a host call -> [(the data or its
    padded copy (_whole_words), its bytes, the offsets, n_rows)]; torch's stream has been waited for.  ids: int32 data is
    taken beside uint8; offsets, s: what the layer's messages call the offsets, and the ending of the verb behind them."""
    import torch
    fn = prefix + "_rows_tensor"
    kinds = (torch.uint8, torch.int32) if ids else (torch.uint8,)
    if any(d.dtype not in kinds or d.dtype != batches[0][0].dtype or o.dtype != torch.int64 for d, o in batches):
        words = ("uint8 or int32 data" if ids else "uint8 data") + (" of one kind" if len(batches) > 1 else "")
        raise WordPieceError("%s needs %s and int64 %s" % (fn, words, offsets))
    _flat_device_tensors(fn, device, *[t for batch in batches for t in batch])
    if any(o.numel() < 1 for _, o in batches):
        raise WordPieceError("%s: %s need%s n_rows + 1 entries" % (prefix, offsets, s))
    padded = _whole_words(*[d for d, _ in batches])
    return [(d, nbytes, o, o.numel() - 1) for (d, nbytes), (_, o) in zip(padded, batches)]


def _host_block(ptr, k, kind, absent=0):
    """a copy of the k elements of a block the library returned (k == 0: an empty array; NULL: `absent` zeros)"""
    if not k or not ptr:
        return np.zeros(0 if ptr else absent, dtype=_KINDS[kind][0])
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(np.ctypeslib.as_ctypes_type(_KINDS[kind][0]))), (k,)).copy()


def _free_blocks(result):
    """frees the blocks of a host result: every pointer field of the struct, so no list of them can go stale"""
    for name, ctype in result._fields_:
        if (ctype is C.c_void_p or issubclass(ctype, C._Pointer)) and getattr(result, name):
            lib().wp_free(getattr(result, name))


def _layer_result(layer, out, read, on=None, elem=None, **sizes):
    """The dict of a corpus call from its filled Result struct, by the layer's rows of _RESULTS.  read: _host_block, or a
    _DeviceViews; on: {keyword: whether it is switched on}; elem: the kind of the batch's own elements; sizes: what the
    struct does not count.  A size that is a function is called once, and only for an array that came back: the tensor
    form reads one offset from the device for "elems"."""
    def size(name, ptr):
        k = sizes[name] if name in sizes else getattr(out, name)
        if callable(k):
            if not ptr:
                return 0
            k = sizes[name] = k()
        return k
    res = {}
    for key, kind, shape, flag in _RESULTS[layer]:
        if flag is not None and not (on and on.get(flag)):
            continue
        ptr = getattr(out, key)
        dims = [size(name, ptr) for name in shape]
        if kind == "off":  # (one entry more, and [0] where the library handed none out: a call without rows)
            res[key] = read(ptr, dims[0] + 1, "i64", absent=1)
        else:
            a = read(ptr, math.prod(dims), elem if kind == "elem" else kind)
            res[key] = a.reshape(dims) if len(dims) > 1 else a
    return res


def _host_result(layer, out, on=None, elem=None, **sizes):
    """_layer_result of a host call: copies of the library's blocks, which are freed here"""
    try:
        return _layer_result(layer, out, _host_block, on, elem, **sizes)
    finally:
        _free_blocks(out)


def _flat_device_tensors(fn, device, *tensors):
    """the tensors of a device call: flat, contiguous, on the handle's device (raw pointers go there)"""
    for t in tensors:
        if not t.is_cuda or not t.is_contiguous() or t.dim() != 1:
            raise WordPieceError("%s needs flat contiguous CUDA/HIP tensors" % fn)
        if device is not None and t.device.index != device:
            raise WordPieceError("the tensors lie on %s, the handle on device %d" % (t.device, device))


def _whole_words(*tensors):
    """The data tensors of a device call where the kernels can read whole aligned words -> [(the tensor, or a padded copy
    of uint8 data that is not such, its bytes)]; then waits for torch's stream: the library runs on its own HIP streams."""
    import torch
    out = []
    for t in tensors:
        nbytes = t.numel() * t.element_size()
        if t.dtype == torch.uint8 and (t.data_ptr() % 4 != 0 or nbytes % 4 != 0):
            padded = torch.zeros((nbytes + 19) // 16 * 16, dtype=torch.uint8, device=t.device)
            padded[:nbytes] = t
            t = padded
        out.append((t, nbytes))
    torch.cuda.current_stream(tensors[0].device).synchronize()
    return out


class _DeviceViews:
    """the arrays of a device result as tensors on dev: clones, or with copy=False views of the library's buffers"""

    def __init__(self, dev, copy):
        self.dev, self.copy = dev, copy

    def __call__(self, ptr, k, kind, absent=0):
        import torch
        _, typestr, dtype = _KINDS[kind]
        if not k or not ptr:  # (k == 0: an empty tensor; NULL: `absent` zeros)
            return torch.zeros(0 if ptr else absent, dtype=getattr(torch, dtype), device=self.dev)
        t = torch.as_tensor(DeviceIds(ptr, k, typestr=typestr), device=self.dev)
        return t.clone() if self.copy else t


def join_spans(spans):
    """The flat form of labelled spans given per sample: a list, per sample, of (begin, end) or (begin, end, label)
    (label 0 where there is none) -> (span_splits int64 [n_samples + 1], spans uint32 [n_spans, 2], span_labels int32
    [n_spans]), what the align calls take.  The rules — non-empty, sorted, disjoint — are the library's to check."""
    splits = _offsets_of([len(s) for s in spans])
    flat = [t for s in spans for t in s]
    sp = np.array([(t[0], t[1]) for t in flat], dtype=np.uint32).reshape(-1, 2)
    sl = np.array([t[2] if len(t) > 2 else 0 for t in flat], dtype=np.int32)
    return splits, sp, sl


def _spans_arg(spans):
    """what join_spans returns, from that or from the list of lists"""
    if spans is None:
        raise WordPieceError("spans is required")
    if isinstance(spans, tuple) and len(spans) == 3 and all(isinstance(x, np.ndarray) for x in spans):
        splits = np.ascontiguousarray(spans[0], dtype=np.int64)
        sp = np.ascontiguousarray(spans[1], dtype=np.uint32).reshape(-1, 2)
        sl = np.ascontiguousarray(spans[2], dtype=np.int32)
    else:
        splits, sp, sl = join_spans(spans)
    if splits.ndim != 1 or len(splits) < 1 or sl.shape != (len(sp),):
        raise WordPieceError("spans: span_splits [n_samples + 1], spans [n_spans, 2] and span_labels [n_spans]")
    return splits, sp, sl


def _align_batch(batch, offsets, token_type_ids, lengths, sample, conv):
    """the four arrays of an align call from the dict of an inputs call and / or one by one (given ones win)"""
    if batch is not None:
        if not isinstance(batch, dict):
            raise WordPieceError("batch is the dict an inputs call returns; pass single arrays by name")
        offsets = batch.get("offsets") if offsets is None else offsets
        token_type_ids = batch.get("token_type_ids") if token_type_ids is None else token_type_ids
        lengths = batch.get("lengths") if lengths is None else lengths
        sample = batch.get("sample") if sample is None else sample
    if offsets is None:
        raise WordPieceError("an align call needs the offsets of the batch (encode_inputs(..., offsets=...))")
    return tuple(None if x is None else conv(x) for x in (offsets, token_type_ids, lengths, sample))


def _align_want(labels, span_index, positions):
    want = (WP_ALIGN_LABELS if labels else 0) | (WP_ALIGN_SPAN_INDEX if span_index else 0) | (WP_ALIGN_POSITIONS if positions else 0)
    if want == 0:
        raise WordPieceError("an align call needs an output: labels, span_index or positions")
    return want


def _tensor_ptr(t):
    return None if t is None or t.numel() == 0 else C.c_void_p(t.data_ptr())


def _docs_arg(docs, text, doc_offsets):
    if (docs is None) == (text is None):
        raise WordPieceError("give either docs or text")
    if docs is not None:
        if doc_offsets is not None:
            raise WordPieceError("doc_offsets go with text, not with docs")
        return join_docs(docs)
    if doc_offsets is None:
        return _bytes(text), None
    off = np.ascontiguousarray(doc_offsets, dtype=np.int64)
    if off.ndim != 1 or len(off) < 1:
        raise WordPieceError("doc_offsets must be a 1-d array of n_docs + 1 entries")
    return _bytes(text), off


def _i64_ptr(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_int64))


def q32(p):
    """A share p in [0, 1] as the C ABI takes it: min(floor(p * 2^32), 2^32)."""
    return min(int(p * 4294967296.0), 1 << 32)


def _mask_batch(input_ids, lengths):
    ids = np.ascontiguousarray(input_ids, dtype=np.int32)
    if ids.ndim != 2:
        raise WordPieceError("input_ids must be a 2-d array [n_rows, max_len]")
    lens = None
    if lengths is not None:
        lens = np.ascontiguousarray(lengths, dtype=np.int32)
        if lens.shape != (ids.shape[0],):
            raise WordPieceError("lengths must be a 1-d array of n_rows entries")
    return ids, lens


def _i32_ptr(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))


def _mask_spec(max_len, mask_id, prob, mask_share, random_share, whole_word, seed, row_base, ignore_id, cls_id, sep_id, pad_id):
    if mask_id is None:
        raise WordPieceError("mask_id is required")
    for name, p in (("prob", prob), ("mask_share", mask_share), ("random_share", random_share)):
        if not 0.0 <= p <= 1.0:
            raise WordPieceError("%s must lie in [0, 1], not %r" % (name, p))
    return MaskSpec(int(max_len), _special(cls_id), _special(sep_id), _special(pad_id), int(mask_id), int(ignore_id),
                    int(whole_word), 0, q32(prob), q32(mask_share), q32(random_share), int(seed) & (2 ** 64 - 1),
                    int(row_base) & (2 ** 64 - 1))


def _pack_spec(max_len, mode, bos_id, eos_id, pad_id, long_docs, want):
    if mode not in _PACK_MODES:
        raise WordPieceError("mode must be one of %s" % ", ".join(sorted(_PACK_MODES)))
    if long_docs not in _PACK_LONG_DOCS:
        raise WordPieceError("long_docs must be one of %s" % ", ".join(sorted(_PACK_LONG_DOCS)))
    if isinstance(want, int):
        bits = want
    else:
        unknown = [k for k in want if k not in _PACK_WANT]
        if unknown:
            raise WordPieceError("want names %s; known: %s" % (", ".join(map(str, unknown)), ", ".join(_PACK_WANT)))
        bits = sum(_PACK_WANT[k] for k in set(want))
    return PackSpec(int(max_len), _PACK_MODES[mode], _special(bos_id), _special(eos_id), int(pad_id), _PACK_LONG_DOCS[long_docs],
                    int(bits), 0)


def _detok_spec(max_len, skip_ids, cleanup, terminator):
    skip = [int(i) for i in skip_ids]
    if len(skip) > 8:
        raise WordPieceError("at most 8 skip ids")
    return DetokSpec(int(max_len), int(bool(cleanup)), _terminator_byte(None, terminator), len(skip), (C.c_int32 * 8)(*skip))


def _special(i):
    return -1 if i is None else int(i)


def _inputs_spec(max_len, cls_id, sep_id, pad_id, pairs, truncation, stride, offsets):
    if truncation not in _TRUNCATIONS:
        raise WordPieceError("truncation must be one of %s, not %r" % (", ".join(sorted(_TRUNCATIONS)), truncation))
    return InputsSpec(int(max_len), _special(cls_id), _special(sep_id), int(pad_id), 0 if pairs is None else int(pairs), _TRUNCATIONS[truncation],
                      -1 if stride is None else int(stride), -1 if offsets is None else _offset_unit(offsets))


def _offset_unit(unit):
    if unit not in _OFFSET_UNITS:
        raise WordPieceError("offsets unit must be 'byte' or 'char', not %r" % (unit,))
    return _OFFSET_UNITS[unit]


class DeviceIds:
    """`__cuda_array_interface__` view of an id buffer in HBM owned by the library (torch.as_tensor,
    cupy.asarray, numba … accept it without a copy)."""

    def __init__(self, ptr, n, cols=0, typestr="<i4"):
        shape = (n, cols) if cols else (n,)
        self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (ptr, False), "version": 2}


class _Linear:
    """word_piece::linear of the reference (src/word_piece.hpp:10-21)."""

    @staticmethod
    def encode(text, vocab):
        if isinstance(vocab, (str, bytes)):  # (text_file, vocab_file) overload, linear.cpp:337-341
            ids = C.POINTER(C.c_int32)()
            n = C.c_size_t()
            _check(lib().wp_linear_encode_file(_bytes(text), _bytes(vocab), C.byref(ids), C.byref(n)))
            return _adopt_ids(ids, n.value).tolist()
        return Vocab(vocab).encode(text).tolist()  # linear.cpp:332-335

    @staticmethod
    def encodeExternal(text_file, vocab_file, out_file, memory_limit):  # linear.cpp:343-374
        _check(lib().wp_linear_encode_external(_bytes(text_file), _bytes(vocab_file), _bytes(out_file),
                                               int(memory_limit)))


linear = _Linear()


class _Fast:
    """word_piece::fast of the reference (src/word_piece.hpp:23-36, src/fast.cpp:159-220)."""

    @staticmethod
    def encode(text, vocab):
        if isinstance(vocab, (str, bytes)):  # (text_file, vocab_file) overload, fast.cpp:166-170
            ids = C.POINTER(C.c_int32)()
            n = C.c_size_t()
            _check(lib().wp_fast_encode_file(_bytes(text), _bytes(vocab), C.byref(ids), C.byref(n)))
            return _adopt_ids(ids, n.value).tolist()
        return Vocab(vocab).fast_encode(text).tolist()  # fast.cpp:161-164

    @staticmethod
    def decode(vocab_file, ids):  # fast.cpp:172-187
        import sys
        v = Vocab(file=vocab_file)
        out = []
        for i in ids:
            if i < 0 or i >= len(v):
                print("no token %d" % i, file=sys.stderr)
                continue
            flags = v.token_flags(i)
            if flags & 4:
                print("trying to access malformed token", file=sys.stderr)
                continue
            w = v.token_utf8(i)
            out.append(w if flags & 1 else b"##" + w)
        return out

    @staticmethod
    def encodeExternal(text_file, vocab_file, out_file, memory_limit):  # fast.cpp:189-220
        _check(lib().wp_fast_encode_external(_bytes(text_file), _bytes(vocab_file), _bytes(out_file),
                                             int(memory_limit)))


fast = _Fast()


def learn_vocab(text_or_docs, vocab_size, normalize=0, device=None, min_count=1, max_word_bytes=256, **kw):
    """Text to the handle of a vocabulary learned from it: a bootstrap handle counts the words of the text (normalised
    with the WP_NORM_* flags `normalize`) and learns the list from that table, both on the device; only the token list
    comes to the host, where the returned Vocab (same `normalize`) is built from it.  text_or_docs: str, bytes, or a list
    of documents; kw: the arguments of Vocab.learn_vocab_tensor (reserved, lower_thresh, ..., slack)."""
    import torch
    if isinstance(text_or_docs, (str, bytes, bytearray, memoryview)):
        data = _bytes(text_or_docs)
    else:
        data = b"\n".join(_bytes(d) for d in text_or_docs)
    boot = Vocab(["[UNK]"], device=device, normalize=normalize)
    dev = torch.device("cuda", torch.cuda.current_device() if device is None else int(device))
    text = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev) if data else torch.zeros(0, dtype=torch.uint8, device=dev)
    table = boot.count_words_tensor(text, order="count", min_count=min_count, max_word_bytes=max_word_bytes, copy=False)
    r = boot.learn_vocab_tensor(table["words"], table["word_off"], table["counts"], vocab_size, copy=False, **kw)
    lines = bytes(r["tokens"].cpu().numpy()).split(b"\n")[:-1]
    return Vocab(lines, device=device, normalize=normalize)


def shard_bounds(data, world_size):
    """Cuts `data` (bytes) into world_size byte ranges at ASCII whitespace: each cut
    is advanced to the next whitespace byte so no word straddles two shards."""
    n = len(data)
    mv = memoryview(data)
    cuts = [0]
    for r in range(1, world_size):
        p = max(cuts[-1], n * r // world_size)
        while p < n and mv[p] not in (9, 10, 11, 12, 13, 32):
            p += 1
        cuts.append(p)
    cuts.append(n)
    return [(cuts[i], cuts[i + 1]) for i in range(world_size)]
