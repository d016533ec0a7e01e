// binpack_path.h — best-fit-decreasing packing on a context (include/wordpiece_amd_binpack.h; kernels: binpack.h): the
// argument rules, the planner, and the passes over device buffers.  The plan of the documents, the pieces, the batch
// buffers and the write pass are those of pack_path.h.
#pragma once
#include "binpack.h"
#include "group_path.h"  // check_arena_guard
#include "pack_path.h"
#include "radix_sort.h"

namespace wp {

// every argument rule that needs neither the rows nor a device (the texts follow check_pack_spec)
static PackGeom check_binpack_spec(const wp_binpack_spec *spec, size_t n_docs) {
  if (!spec) throw std::invalid_argument("binpack: spec is NULL");
  if (spec->long_docs != WP_PACK_LONG_TRUNCATE && spec->long_docs != WP_PACK_LONG_SPLIT) throw std::invalid_argument("binpack: unknown long_docs");
  if ((spec->want & ~7) != 0) throw std::invalid_argument("binpack: want has bits outside 7");
  if (spec->max_len < 1) throw std::invalid_argument("binpack: max_len must be at least 1");
  if (spec->max_len > WP_BINPACK_MAX_LEN) throw std::invalid_argument("binpack: max_len must be at most 8192");
  const int specials = (spec->bos_id >= 0 ? 1 : 0) + (spec->eos_id >= 0 ? 1 : 0);
  if (spec->max_len - specials < 1) throw std::invalid_argument("binpack: max_len leaves no room for an id beside the specials");
  if (spec->reserved0 != 0) throw std::invalid_argument("binpack: reserved0 must be 0");
  if (spec->reserved1 != 0) throw std::invalid_argument("binpack: reserved1 must be 0");
  if (n_docs > static_cast<size_t>(INT32_MAX)) throw std::length_error("binpack: more documents than INT32_MAX");
  PackGeom g{};
  g.max_len = spec->max_len;
  g.budget = spec->max_len - specials;
  g.stream = 0;
  g.split = spec->long_docs == WP_PACK_LONG_SPLIT;
  g.bos_id = spec->bos_id;
  g.eos_id = spec->eos_id;
  g.pad_id = spec->pad_id;
  g.want = spec->want;
  return g;
}

static wp_binpack_stats &begin_binpack_stats(wp_vocab *v, size_t n_docs) {
  v->stats.binpack_call = 1;
  v->stats.binpack = wp_binpack_stats{};
  v->stats.binpack.n_docs = static_cast<int64_t>(n_docs);
  return v->stats.binpack;
}

// ---- the planner ---------------------------------------------------------------------------------------------------
// The procedure of the header over groups of rows.  Every remaining capacity r has a FIFO list of groups; a group is a
// stretch of consecutive rows (row0, n) that share one history: `slot` units each, L - r cells each.  Units of u cells
// go to the head group of the smallest r >= u that has one — floor(r / u) into every row, since a row that has taken a
// unit and still has room for another is alone in its new queue, below every other candidate — or open new rows.  A
// group that c units do not fill splits into the rows they fill, one partly filled row, and the rest, which stays at
// the head.  Queue 0 collects the full rows.  The groups at the end, in row order, are the row ranges.
struct BinPlan {
  long long n_out = 0, n_units = 0, n_cells = 0;
  std::vector<wp_binpack_run> runs;
  std::vector<wp_binpack_row_range> ranges;
};

class BinPlanner {
  struct Group {
    long long row0, n;
    int32_t slot, next;
  };
  const int L;
  std::vector<Group> pool;
  std::vector<int32_t> head, tail;   // per r in 0 .. L: the list of its groups (-1: none)
  std::vector<uint64_t> nonempty;    // bit r: queue r has a group (r >= 1)
  BinPlan plan;

  int find(int u) const {  // the smallest r >= u with a group, or -1
    size_t w = static_cast<size_t>(u) >> 6;
    uint64_t m = nonempty[w] & (~0ull << (u & 63));
    while (!m) {
      if (++w >= nonempty.size()) return -1;
      m = nonempty[w];
    }
    return static_cast<int>(w * 64 + static_cast<size_t>(__builtin_ctzll(m)));
  }
  void push(int r, long long row0, long long n, int32_t slot) {
    const int32_t at = static_cast<int32_t>(pool.size());
    if (at == INT32_MAX) throw std::length_error("binpack: the plan has more groups than INT32_MAX");
    pool.push_back(Group{row0, n, slot, -1});
    if (tail[r] < 0) {
      head[r] = at;
      if (r > 0) nonempty[static_cast<size_t>(r) >> 6] |= 1ull << (r & 63);
    } else {
      pool[tail[r]].next = at;
    }
    tail[r] = at;
  }
  void pop(int r) {
    head[r] = pool[head[r]].next;
    if (head[r] < 0) {
      tail[r] = -1;
      nonempty[static_cast<size_t>(r) >> 6] &= ~(1ull << (r & 63));
    }
  }
  // n_rows rows from row0 on take per_row units of u cells each, from sigma-rank `rank` on
  void emit(long long rank, long long row0, long long n_rows, int u, int per_row, int slot0, int col0) {
    if (!plan.runs.empty()) {  // the rows behind the last run with the same pattern: one run
      wp_binpack_run &b = plan.runs.back();
      if (b.unit == u && b.per_row == per_row && b.slot0 == slot0 && b.col0 == col0 && b.row0 + b.n_rows == row0) {
        b.n_rows += n_rows;
        return;
      }
    }
    plan.runs.push_back(wp_binpack_run{rank, row0, n_rows, u, per_row, slot0, col0});
  }

 public:
  explicit BinPlanner(int max_len)
      : L(max_len), head(static_cast<size_t>(max_len) + 1, -1), tail(static_cast<size_t>(max_len) + 1, -1),
        nonempty((static_cast<size_t>(max_len) >> 6) + 1, 0) {}

  BinPlan run(const int64_t *hist) {
    long long rank = 0;
    for (int u = L; u >= 1; u--) {
      long long c = hist[u];
      if (c < 0) throw std::invalid_argument("binpack: hist[" + std::to_string(u) + "] is negative");
      if (c == 0) continue;
      // (n_out <= n_units <= n_cells and every product below is at most n_out * L)
      if (c > (1ll << 48) / u || plan.n_cells + c * u > (1ll << 48)) throw std::length_error("binpack: more than 2^48 cells in the units");
      plan.n_units += c;
      plan.n_cells += c * u;
      while (c > 0) {
        int r = find(u);
        const bool fresh = r < 0;
        Group g;
        if (fresh) {  // no row takes the unit: new rows, as many as the c units need
          r = L;
          const long long per = L / u;
          g = Group{plan.n_out, (c + per - 1) / per, 0, -1};
          plan.n_out += g.n;
        } else {
          g = pool[head[r]];
        }
        const int per = r / u, col0 = L - r;
        const long long cap = g.n * per;
        if (c >= cap) {  // the whole group
          emit(rank, g.row0, g.n, u, per, g.slot, col0);
          if (!fresh) pop(r);
          push(r - per * u, g.row0, g.n, g.slot + per);
          rank += cap;
          c -= cap;
          continue;
        }
        const long long full = c / per;
        const int rem = static_cast<int>(c % per);
        if (full) {
          emit(rank, g.row0, full, u, per, g.slot, col0);
          push(r - per * u, g.row0, full, g.slot + per);
          rank += full * per;
        }
        if (rem) {
          emit(rank, g.row0 + full, 1, u, rem, g.slot, col0);
          push(r - rem * u, g.row0 + full, 1, g.slot + rem);
          rank += rem;
        }
        const long long used = full + (rem ? 1 : 0);
        if (!fresh) {  // (new rows are opened as needed: none is left over)
          if (used == g.n) {
            pop(r);
          } else {
            pool[head[r]].row0 += used;
            pool[head[r]].n -= used;
          }
        }
        c = 0;
      }
    }
    // the groups as they ended, in row order; neighbours with one pattern are one range
    struct End {
      long long row0, n;
      int32_t units, cells;
    };
    std::vector<End> ends;
    for (int r = 0; r <= L; r++) {
      for (int32_t at = head[r]; at >= 0; at = pool[at].next) ends.push_back(End{pool[at].row0, pool[at].n, pool[at].slot, L - r});
    }
    std::sort(ends.begin(), ends.end(), [](const End &a, const End &b) { return a.row0 < b.row0; });
    long long units = 0, cells = 0;
    for (const End &e : ends) {
      if (!plan.ranges.empty() && plan.ranges.back().units_per_row == e.units && plan.ranges.back().cells_per_row == e.cells) {
        plan.ranges.back().n_rows += e.n;
      } else {
        plan.ranges.push_back(wp_binpack_row_range{e.row0, e.n, units, cells, e.units, e.cells});
      }
      units += e.n * e.units;
      cells += e.n * e.cells;
    }
    if (units != plan.n_units || cells != plan.n_cells) throw std::logic_error("binpack: the row ranges do not add up to the units");
    return std::move(plan);
  }
};

static BinPlan binpack_plan_host(const int64_t *hist, int max_len) { return BinPlanner(max_len).run(hist); }

// ---- the device path -----------------------------------------------------------------------------------------------
// The passes over device buffers on c's stream; place(n_out) as in pack_on_device.  Returns n_out.  Nothing is written
// through the caller's pointers before every check has passed.
template <typename Place>
static size_t binpack_on_device(wp_vocab *v, Context *c, const int32_t *d_ids, const long long *d_splits, size_t n_docs, PackGeom g,
                                Place &&place) {
  wp_binpack_stats &bs = begin_binpack_stats(v, n_docs);
  if (n_docs == 0) return 0;
  hipStream_t st = c->stream;
  const dim3 block(kBlock);
  const bool guard = v->arena_guard || EnvOptions::get().arena_guard;
  const PackDocs docs = pack_plan_docs(c, "binpack", d_ids, d_splits, n_docs, g, bs);
  if (g.n_pieces == 0) return 0;
  const size_t n_p = g.n_pieces, L = static_cast<size_t>(g.max_len);
  const size_t tmp_words = radix_tmp_words<uint32_t>(n_p);
  if (!c->h_binpack_hist) WP_HIP(hipHostMalloc(&c->h_binpack_hist, (kBinMaxLen + 1) * sizeof(int64_t)));
  Arena tab(&c->pack_tab, guard);
  uint32_t *d_P = nullptr, *d_P2 = nullptr, *d_row_first = nullptr, *d_k0 = nullptr, *d_k1 = nullptr, *d_v0 = nullptr, *d_v1 = nullptr, *d_rtmp = nullptr;
  int32_t *d_src0 = nullptr, *d_src2 = nullptr;
  unsigned long long *d_hist = nullptr;
  for (int pass = 0; pass < 2; pass++) {
    // + 1: P[n_p] = P2[n_p] = N and row_first[n_out] = n_p (n_out <= n_p); src0 and src2 are sized alike
    d_P = tab.take<uint32_t>(n_p + 1);
    d_src0 = tab.take<int32_t>(n_p + 1);
    d_P2 = tab.take<uint32_t>(n_p + 1);
    d_src2 = tab.take<int32_t>(n_p + 1);
    d_row_first = tab.take<uint32_t>(n_p + 1);
    d_k0 = tab.take<uint32_t>(n_p);
    d_k1 = tab.take<uint32_t>(n_p);
    d_v0 = tab.take<uint32_t>(n_p);
    d_v1 = tab.take<uint32_t>(n_p);
    d_rtmp = tab.take<uint32_t>(tmp_words);
    d_hist = tab.take<unsigned long long>(L + 1);
    if (pass == 0) tab.commit();
  }
  tab.arm(st);
  pack_pieces(c, docs, d_splits, n_docs, g, d_P, d_src0);
  WP_HIP(hipMemsetAsync(d_hist, 0, (L + 1) * sizeof(unsigned long long), st));
  hipLaunchKernelGGL(binpack_hist_kernel, dim3(std::min<unsigned>(cdiv(n_p, kBinTile), kBinHistGrid)), block, 0, st, d_P, g.n_pieces,
                     static_cast<uint32_t>(L), d_k0, d_hist);
  WP_LAUNCH_CHECK();
  WP_HIP(hipMemcpyAsync(c->h_binpack_hist, d_hist, (L + 1) * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  WP_HIP(hipEventRecord(c->evs[kEvScalars], st));
  // the stream sorts while the host plans: sigma = the pieces by key (L - u) ascending, stable
  const int key_bits = std::max(1, bit_length(L - 1));
  const int cur = radix_sort_pairs<uint32_t>(d_k0, d_v0, d_k1, d_v1, n_p, 0, key_bits, d_rtmp, tmp_words, st, nullptr, true);
  const uint32_t *d_sigma = cur ? d_v1 : d_v0;
  WP_HIP(hipEventSynchronize(c->evs[kEvScalars]));
  const BinPlan plan = binpack_plan_host(c->h_binpack_hist, g.max_len);
  if (plan.n_units != static_cast<long long>(n_p) || plan.n_cells != static_cast<long long>(g.n_cells)) {
    throw HipError("binpack: the histogram of the unit lengths does not add up to the pieces");
  }
  const unsigned long long n_out = static_cast<unsigned long long>(plan.n_out);
  bs.n_out = plan.n_out;
  bs.n_runs = static_cast<int64_t>(plan.runs.size());
  bs.n_row_ranges = static_cast<int64_t>(plan.ranges.size());
  check_pack_rows("binpack", n_out, g.max_len);
  g.n_out = static_cast<uint32_t>(n_out);
  const PackOut o = place(static_cast<size_t>(n_out));
  Arena pa(&c->binpack_plan, guard);
  wp_binpack_run *d_runs = nullptr;
  wp_binpack_row_range *d_ranges = nullptr;
  for (int pass = 0; pass < 2; pass++) {
    d_runs = pa.take<wp_binpack_run>(plan.runs.size());
    d_ranges = pa.take<wp_binpack_row_range>(plan.ranges.size());
    if (pass == 0) pa.commit();
  }
  pa.arm(st);
  // (the tables are read from `plan`, which lives until the wait at the end of this call)
  WP_HIP(hipMemcpyAsync(d_runs, plan.runs.data(), plan.runs.size() * sizeof(wp_binpack_run), hipMemcpyHostToDevice, st));
  WP_HIP(hipMemcpyAsync(d_ranges, plan.ranges.data(), plan.ranges.size() * sizeof(wp_binpack_row_range), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(binpack_place_kernel, dim3(cdiv(n_p, kBinTile)), block, 0, st, d_sigma, d_P, d_src0, d_runs, static_cast<uint32_t>(plan.runs.size()),
                     d_ranges, static_cast<uint32_t>(plan.ranges.size()), g.n_pieces, g.n_cells, d_P2, d_src2);
  hipLaunchKernelGGL(binpack_rows_kernel, dim3(cdiv(static_cast<size_t>(n_out) + 1, kBlock)), block, 0, st, d_ranges,
                     static_cast<uint32_t>(plan.ranges.size()), g.n_out, g.n_pieces, d_row_first);
  const size_t cell_tiles = cdiv(static_cast<size_t>(n_out) * L, kPackCellTile);
  hipLaunchKernelGGL(seqpack_write_kernel, dim3(static_cast<unsigned>(std::min<size_t>(cell_tiles, kPackMaxGrid))), block, 0, st, d_ids, d_P2,
                     d_src2, d_row_first, g, o, docs.d_tot);
  WP_LAUNCH_CHECK();
  queue_scalar_slots(c, kScalarPack, kScalarPack, st);
  WP_HIP(hipStreamSynchronize(st));
  throw_if_oob(kSitePack, "binpack", "gathers or stores outside their buffers skipped");
  check_arena_guard(c, tab, st, "binpack");
  check_arena_guard(c, pa, st, "binpack");
  bs.n_cells = static_cast<int64_t>(docs.h_tot[kPackCells]);
  bs.n_segments = static_cast<int64_t>(docs.h_tot[kPackSegments]);
  return static_cast<size_t>(n_out);
}

}  // namespace wp
