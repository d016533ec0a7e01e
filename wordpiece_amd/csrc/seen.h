// seen.h — the kernels of the persistent key set (include/wordpiece_amd_seen.h; host path: seen_path.h).  The set is an
// open-addressing table of 64-bit keys in device memory that the handle owns across calls: 0 is an empty slot, the home
// of a key is the slot its TOP log2(capacity) bits name, and a probe walks forward from there with wrap.  A call never
// brings two equal keys to the table: the batch is grouped first (stable radix sort of (key, row), run heads: group.h),
// and only the heads of the runs probe.  The heads ascend in key and so in home slot: the probes of a wave walk the table
// in ascending order and neighbouring probes read neighbouring lines; a table of twice the size keeps the order of the
// keys, so the rehash is close to a streaming pass; and the slots in order are nearly the sorted export.
// A probe is made by a group of kSeenGroup = 8 lanes over one 64-byte line of 8 slots: one coalesced load a step, match
// and empty slot found by a ballot inside the group.  In the line of the home slot the slots in front of it are not the
// key's.  Nothing is ever deleted, so a key that is in the table lies in front of the first empty slot behind its home: a
// line with a match answers "found", a line with an empty slot and no match "not found".  The host keeps the load at 1/2
// or below, so every probe ends; all the same a probe is capped at one pass over the table, and one that runs out raises
// a counter that fails the call.  The row keys themselves are the dedup's (dedup.h, seed 0).
#pragma once
#include "common.h"
#include "dedup.h"
#include "group.h"

namespace wp {

constexpr int kSeenGroup = 8;                            // lanes of a probe: the slots of a 64-byte line
constexpr int kSeenPerBlock = kBlock / kSeenGroup;       // probes of a workgroup
constexpr unsigned kSeenGrid = 2048;                     // workgroups of the kernels that count: 8 for each of 256 CUs
// the counters of a call, 32 bits each, in d_scalars from kScalarSeen on (words 4, 5: the lines the lookup read, 64 bits)
enum SeenCounter { kSeenNew = 0, kSeenRepeat = 1, kSeenBefore = 2, kSeenRanOut = 3, kSeenProbes = 4, kSeenCounters = 8 };

// the bits of the lane's group of 8 in a ballot over the wave (every lane of the wave must be here)
__device__ __forceinline__ uint32_t seen_group_ballot(bool p) {
  const unsigned long long b = __ballot(p);
  return static_cast<uint32_t>(b >> (lane_id() & ~(kSeenGroup - 1))) & 0xffu;
}

// key[j] = in[j], 1 where that is 0 (the empty slot's value); in == key: in place
__global__ __launch_bounds__(kBlock) void seen_keys_kernel(const uint64_t *in, uint64_t *key, size_t m) {
  const size_t j = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (j >= m) return;
  const uint64_t k = in[j];
  key[j] = k ? k : 1ull;
}

// The sum of v over the workgroup in *slot (an LDS word, zero before): whole on every lane behind the barrier.  The counters
// of a call are words that every workgroup adds to, and atomics on one address queue up behind each other: the kernels
// that count run a fixed grid over their items and add once a workgroup, not once a wave.
__device__ __forceinline__ uint32_t seen_block_sum(uint32_t v, uint32_t *slot) {
  v = wave_reduce_sum(v);
  if (lane_id() == 0 && v != 0) atomicAdd(slot, v);
  __syncthreads();
  return *slot;
}

// Run r of the sorted keys (r < *n_runs; 8 lanes each, the grid strides over m): found[r] = 1 where the key of its head
// is in the table.  Read-only.  Counted: the heads not found (kSeenNew), the lines read (kSeenProbes), the probes that ran
// out (kSeenRanOut).
__global__ __launch_bounds__(kBlock) void seen_lookup_kernel(const uint64_t *__restrict__ key, const uint32_t *__restrict__ head_pos,
                                                             const uint32_t *__restrict__ n_runs, size_t m, const uint64_t *__restrict__ slots,
                                                             uint32_t log2cap, uint32_t *__restrict__ found, uint32_t *__restrict__ counters) {
  __shared__ uint32_t sums[3];
  if (threadIdx.x < 3) sums[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t sub = threadIdx.x & (kSeenGroup - 1);
  const size_t lines = (size_t(1) << log2cap) / kSeenGroup, runs = min(static_cast<size_t>(*n_runs), m);
  uint32_t n_new = 0, n_loads = 0, n_out = 0;
  // (the bounds of the loop are the workgroup's: every lane of a wave makes the same rounds, as the ballots need)
  for (size_t base = static_cast<size_t>(blockIdx.x) * kSeenPerBlock; base < runs; base += static_cast<size_t>(gridDim.x) * kSeenPerBlock) {
    const size_t r = base + threadIdx.x / kSeenGroup;
    bool live = r < runs;
    uint64_t k = 0;
    if (live) {
      const uint32_t hs = head_pos[r];
      live = wp_checked(hs < m, kSiteDedup);
      if (live) k = key[hs];
    }
    const size_t home = static_cast<size_t>(k >> (64u - log2cap));
    size_t line = home / kSeenGroup, step = 0;
    uint32_t from = static_cast<uint32_t>(home) & (kSeenGroup - 1), hit = 0;
    bool done = !live;
    while (__any(!done)) {
      const bool in = !done && sub >= from;
      const uint64_t s = in ? slots[line * kSeenGroup + sub] : 0ull;
      const uint32_t match = seen_group_ballot(in && s == k), empty = seen_group_ballot(in && s == 0ull);
      if (!done) {
        if (sub == 0) n_loads++;
        if (match != 0 || empty != 0) {
          hit = match != 0 ? 1u : 0u;
          done = true;
        } else if (++step > lines) {  // (one pass and the home line again, whole: every slot has been read)
          if (sub == 0) n_out++;
          done = true;
        } else {
          line = (line + 1) & (lines - 1);
          from = 0;
        }
      }
    }
    if (live && sub == 0) {
      found[r] = hit;
      n_new += hit ? 0u : 1u;
    }
  }
  n_new = seen_block_sum(n_new, sums + 0);
  n_loads = seen_block_sum(n_loads, sums + 1);
  n_out = seen_block_sum(n_out, sums + 2);
  if (threadIdx.x == 0) {
    if (n_new != 0) atomicAdd(counters + kSeenNew, n_new);
    if (n_loads != 0) atomicAdd(reinterpret_cast<unsigned long long *>(counters + kSeenProbes), static_cast<unsigned long long>(n_loads));
    if (n_out != 0) atomicAdd(counters + kSeenRanOut, n_out);
  }
}

// The key k of the lane's group (live: whether the group has one) into the table, by the whole wave: the first empty slot
// behind its home takes it by a 64-bit compare-and-swap against 0.  The key is in no slot and no other group brings it, so
// a swap that fails found another key, and the probe goes on behind it: no equality is ever tested.  The empty slots of a
// line are tried from the one load of it (a slot seen empty may be taken by now, which the swap answers; one seen taken
// stays taken).  Returns whether the probe ran out.
__device__ __forceinline__ bool seen_insert(uint64_t *__restrict__ slots, uint32_t log2cap, uint64_t k, bool live) {
  const uint32_t sub = threadIdx.x & (kSeenGroup - 1);
  const size_t lines = (size_t(1) << log2cap) / kSeenGroup;
  const size_t home = static_cast<size_t>(k >> (64u - log2cap));
  size_t line = home / kSeenGroup, step = 0;
  uint32_t from = static_cast<uint32_t>(home) & (kSeenGroup - 1), empty = 0;
  bool done = !live, load = true, ran_out = false;
  while (__any(!done)) {
    const bool in = !done && load && sub >= from;
    const uint64_t s = in ? slots[line * kSeenGroup + sub] : 1ull;
    const uint32_t e = seen_group_ballot(in && s == 0ull);
    if (!done && load) {
      empty = e;
      load = false;
    }
    bool won = false;
    if (!done && empty != 0 && sub == static_cast<uint32_t>(__ffs(empty)) - 1u) {
      won = atomicCAS(reinterpret_cast<unsigned long long *>(slots + line * kSeenGroup + sub), 0ull, static_cast<unsigned long long>(k)) == 0ull;
    }
    const uint32_t placed = seen_group_ballot(won);
    if (!done) {
      if (placed != 0) {
        done = true;
      } else if (empty != 0) {
        empty &= empty - 1u;  // (another key's by now)
      } else if (++step > lines) {
        ran_out = true;
        done = true;
      } else {
        line = (line + 1) & (lines - 1);
        from = 0;
        load = true;
      }
    }
  }
  return ran_out;
}

// Run r (8 lanes each): the key of its head into the table where the lookup did not find it.
__global__ __launch_bounds__(kBlock) void seen_insert_kernel(const uint64_t *__restrict__ key, const uint32_t *__restrict__ head_pos,
                                                             const uint32_t *__restrict__ n_runs, size_t m, const uint32_t *__restrict__ found,
                                                             uint64_t *__restrict__ slots, uint32_t log2cap, uint32_t *__restrict__ counters) {
  const size_t r = (static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x) / kSeenGroup;
  bool live = r < *n_runs && r < m && found[r] == 0u;
  uint64_t k = 0;
  if (live) {
    const uint32_t hs = head_pos[r];
    live = wp_checked(hs < m, kSiteDedup);
    if (live) k = key[hs];
  }
  if (seen_insert(slots, log2cap, k, live) && (threadIdx.x & (kSeenGroup - 1)) == 0) atomicAdd(counters + kSeenRanOut, 1u);
}

// Line L of the old table (8 lanes each, one slot a lane): its keys into the new one, one after the other.
__global__ __launch_bounds__(kBlock) void seen_rehash_kernel(const uint64_t *__restrict__ old_slots, size_t old_lines, uint64_t *__restrict__ slots,
                                                             uint32_t log2cap, uint32_t *__restrict__ counters) {
  const size_t L = (static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x) / kSeenGroup;
  const uint32_t sub = threadIdx.x & (kSeenGroup - 1);
  const uint64_t mine = L < old_lines ? old_slots[L * kSeenGroup + sub] : 0ull;
  uint32_t held = seen_group_ballot(mine != 0ull);
  bool ran_out = false;
  while (__any(held != 0)) {
    const int src = (lane_id() & ~(kSeenGroup - 1)) + (held ? __ffs(held) - 1 : 0);
    const uint64_t k = __shfl(static_cast<unsigned long long>(mine), src, kWave);
    ran_out = seen_insert(slots, log2cap, k, held != 0) || ran_out;
    held &= held - 1u;
  }
  if (ran_out && sub == 0) atomicAdd(counters + kSeenRanOut, 1u);
}

// Sorted position s: its row (val[s]) learns the head of its run — first[row] = the head's row, the smallest of the key —
// and its state: 2 where the table had the key, else 0 for the head and 1 for the others.  key_out (optional): the key by
// row.  Counted: the rows of state 1 and 2.
__global__ __launch_bounds__(kBlock) void seen_settle_kernel(const uint64_t *__restrict__ key, const uint32_t *__restrict__ val,
                                                             const uint32_t *__restrict__ head, const uint32_t *__restrict__ run,
                                                             const uint32_t *__restrict__ head_pos, const uint32_t *__restrict__ found, size_t m,
                                                             int32_t *__restrict__ state, int32_t *__restrict__ first, uint64_t *__restrict__ key_out,
                                                             uint32_t *__restrict__ counters) {
  __shared__ uint32_t sums[2];
  if (threadIdx.x < 2) sums[threadIdx.x] = 0;
  __syncthreads();
  uint32_t n1 = 0, n2 = 0;
  for (size_t s = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x; s < m; s += static_cast<size_t>(gridDim.x) * kBlock) {
    const uint32_t r = run_of(head, run, s), row = val[s];
    if (!wp_checked(r < m && row < m, kSiteDedup)) continue;
    const uint32_t hs = head_pos[r];
    if (!wp_checked(hs <= s, kSiteDedup)) continue;
    const uint32_t hrow = val[hs];
    if (!wp_in_bounds(hrow <= row, kSiteDedup)) continue;
    const int st = found[r] ? 2 : (hs == s ? 0 : 1);
    state[row] = st;
    first[row] = static_cast<int32_t>(hrow);
    if (key_out) key_out[row] = key[s];
    n1 += st == 1 ? 1u : 0u;
    n2 += st == 2 ? 1u : 0u;
  }
  n1 = seen_block_sum(n1, sums + 0);
  n2 = seen_block_sum(n2, sums + 1);
  if (threadIdx.x == 0) {
    if (n1 != 0) atomicAdd(counters + kSeenRepeat, n1);
    if (n2 != 0) atomicAdd(counters + kSeenBefore, n2);
  }
}

// keep[i] = 1 where row i is new; entry n_rows closes the array for its scan
__global__ __launch_bounds__(kBlock) void seen_keep_kernel(const int32_t *__restrict__ state, size_t n_rows, uint32_t *__restrict__ keep) {
  const size_t i = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (i > n_rows) return;
  keep[i] = i < n_rows && state[i] == 0 ? 1u : 0u;
}

// The kept rows (keep_pos: the exclusive scan of keep, *n_kept its total): kept[k] = the k-th new row and out_len[k] its
// bytes; out_len[k] = 0 from *n_kept through n_rows.  The host does not know *n_kept yet, so the compact form behind this
// is laid out over n_rows entries: those behind the kept ones are empty rows at the end of the data.
__global__ __launch_bounds__(kBlock) void seen_kept_kernel(const int32_t *__restrict__ state, const uint32_t *__restrict__ keep_pos,
                                                           const uint32_t *__restrict__ n_kept, const uint32_t *__restrict__ byte_off, size_t n_rows,
                                                           int32_t *__restrict__ kept, uint32_t *__restrict__ out_len) {
  const size_t i = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (i > n_rows) return;
  if (i >= *n_kept) out_len[i] = 0;
  if (i == n_rows || state[i] != 0) return;
  const uint32_t k = keep_pos[i];
  if (!wp_checked(k < *n_kept && k <= i, kSiteDedup)) return;
  kept[k] = static_cast<int32_t>(i);
  out_len[k] = byte_off[i + 1] - byte_off[i];
}

// ---- export: the slots that hold a key, flagged, scanned and scattered in slot order (the sort follows: seen_path.h) -----
__global__ __launch_bounds__(kBlock) void seen_flag_kernel(const uint64_t *__restrict__ slots, size_t cap, uint32_t *__restrict__ flag) {
  const size_t i = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (i > cap) return;
  flag[i] = i < cap && slots[i] != 0ull ? 1u : 0u;
}
__global__ __launch_bounds__(kBlock) void seen_scatter_kernel(const uint64_t *__restrict__ slots, size_t cap, const uint32_t *__restrict__ flag,
                                                              const uint32_t *__restrict__ pos, uint64_t *__restrict__ out, size_t room) {
  const size_t i = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= cap || !flag[i]) return;
  if (wp_checked(pos[i] < room, kSiteDedup)) out[pos[i]] = slots[i];
}

}  // namespace wp
