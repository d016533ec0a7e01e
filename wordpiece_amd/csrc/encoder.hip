// encoder.hip — the C ABI of the HIP Linear-WordPiece path (include/wordpiece_amd.h) and the one translation unit the
// device code is compiled in: the entry points (out-pointers, the answers that need no device, uploads and downloads),
// the pinned pool, the multi-GPU, batch, stream, file and external calls.  The device path itself: linear_path.h
// (word_piece::linear, stage by stage) and fast_path.h (word_piece::fast); the layers on top of it, one host header
// each: rows_path.h, inputs_path.h, mask_path.h, detok_path.h, pack_path.h, special_path.h, align_path.h, count_path.h, learn_path.h, dedup_path.h, neardup_path.h, overlap_path.h, repeat_path.h, quality_path.h; what a handle owns
// on a device: context.h.
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <atomic>
#include <chrono>
#include <cstring>
#include <fstream>
#include <future>
#include <memory>
#include <mutex>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/wordpiece_amd.h"
#include "align_path.h"
#include "context.h"
#include "count_path.h"
#include "dedup_path.h"
#include "detok_path.h"
#include "fast_path.h"
#include "format.h"
#include "inputs_path.h"
#include "learn_path.h"
#include "linear_path.h"
#include "mask_path.h"
#include "neardup_path.h"
#include "overlap_path.h"
#include "quality_path.h"
#include "repeat_path.h"
#include "pack_path.h"
#include "rows_path.h"
#include "special_path.h"


wp_vocab::~wp_vocab() {
  park_context(std::move(ctx));
  for (auto &c : multi) park_context(std::move(c));
}

// ======================================================================================
// C ABI
// ======================================================================================
// Nothing leaves the C ABI as an exception, and the caller's current HIP device is the same after the call as before.
template <typename F>
static int guarded(F &&f) {
  DeviceGuard keep_device;
  try {
    f();
    return WP_OK;
  } catch (const HipError &e) {
    g_last_error = e.what();
    return std::string(e.what()).find("no HIP device") != std::string::npos ? WP_ERR_NO_DEVICE : WP_ERR_HIP;
  } catch (const std::length_error &e) {
    g_last_error = e.what();
    return WP_ERR_TOO_LARGE;
  } catch (const std::invalid_argument &e) {
    g_last_error = e.what();
    return WP_ERR_ARG;
  } catch (const std::ios_base::failure &e) {
    g_last_error = e.what();
    return WP_ERR_IO;
  } catch (const InternalError &e) {
    g_last_error = e.what();
    return WP_ERR_INTERNAL;
  } catch (const std::exception &e) {
    g_last_error = e.what();
    return WP_ERR_HIP;
  } catch (...) {
    g_last_error = "unknown exception inside the HIP WordPiece library";
    return WP_ERR_HIP;
  }
}

// ---- argument rules that several entry points share -----------------------------------------------------------------
// a pointer the kernels load or store `bytes` (4 or 8) at a time through
static void check_aligned(const void *p, size_t bytes, const char *message) {
  if ((reinterpret_cast<uintptr_t>(p) & (bytes - 1)) != 0) throw std::invalid_argument(message);
}
static void check_device_text(const void *d_utf8) { check_aligned(d_utf8, 4, "device text must be 4-byte aligned"); }
static void check_device_doc_off(const void *d_doc_off) { check_aligned(d_doc_off, 8, "device document offsets must be 8-byte aligned"); }
// a device documents call without text has no rows: explicit rows cannot end at 0 unless there are none
static void check_doc_off_without_text(const void *d_doc_off, size_t n_docs) {
  if (d_doc_off && n_docs != 0) throw std::invalid_argument("document offsets must increase from 0 to nbytes");
}
static bool known_norm_flags(int64_t flags) { return flags >= 0 && (flags & ~static_cast<int64_t>(kNormKnownFlags)) == 0; }

// row_splits of a host call: start at 0, never descend; returns the last entry (its bound is the caller's, in its own words)
static int64_t check_row_splits(const char *prefix, const int64_t *row_splits, size_t n) {
  if (row_splits[0] != 0) throw std::invalid_argument(std::string(prefix) + ": row_splits must start at 0");
  for (size_t r = 0; r < n; r++) {
    if (row_splits[r + 1] < row_splits[r]) throw std::invalid_argument(std::string(prefix) + ": row_splits must never descend");
  }
  return row_splits[n];
}

static int vocab_from_lines(const std::vector<std::pair<const char *, size_t>> &lines, wp_vocab **out) {
  if (!out) {
    g_last_error = "null output pointer";
    return WP_ERR_ARG;
  }
  try {
  std::unique_ptr<wp_vocab> v(new wp_vocab());
  if (const char *e = getenv("WP_DEVICES")) {  // default of WP_OPT_DEVICES ("all" or a count): the C++ API has no handle to set it on
    v->n_devices = std::strcmp(e, "all") == 0 ? -1 : std::max(1, atoi(e));
  }
  std::string err = v->hv.build(lines);
  if (!err.empty()) {
    g_last_error = err;
    return WP_ERR_EMPTY_WORD;
  }
  *out = v.release();
  return WP_OK;
  } catch (const std::exception &e) {
    g_last_error = e.what();
    return WP_ERR_ARG;
  } catch (...) {
    g_last_error = "unknown exception while building the vocabulary";
    return WP_ERR_ARG;
  }
}

extern "C" {

int wp_vocab_create(const char *const *lines, const size_t *line_bytes, size_t n_lines, wp_vocab **out) {
  std::vector<std::pair<const char *, size_t>> ls;
  ls.reserve(n_lines);
  for (size_t i = 0; i < n_lines; i++) ls.emplace_back(lines[i], line_bytes[i]);
  return vocab_from_lines(ls, out);
}

int wp_vocab_create_packed(const char *buf, const int64_t *offsets, int64_t n_lines, wp_vocab **out) {
  std::vector<std::pair<const char *, size_t>> ls;
  ls.reserve(static_cast<size_t>(n_lines));
  for (int64_t i = 0; i < n_lines; i++) ls.emplace_back(buf + offsets[i], static_cast<size_t>(offsets[i + 1] - offsets[i]));
  return vocab_from_lines(ls, out);
}

int wp_vocab_from_file(const char *vocab_file, wp_vocab **out) {
  // utils.cpp:123-137: a missing file yields an empty vocabulary (ifstream fails silently)
  std::ifstream fin(vocab_file);
  std::vector<std::string> words;
  std::string w;
  while (std::getline(fin, w)) words.push_back(w);
  std::vector<std::pair<const char *, size_t>> ls;
  for (auto &s : words) ls.emplace_back(s.data(), s.size());
  return vocab_from_lines(ls, out);
}

void wp_vocab_destroy(wp_vocab *v) {
  if (!v) return;
  try {
    delete v;  // (parks the handle's contexts: park_context keeps the caller's current device)
  } catch (...) {
  }
}
int64_t wp_vocab_size(const wp_vocab *v) { return static_cast<int64_t>(v->hv.tokens.size()); }
int32_t wp_vocab_unk_id(const wp_vocab *v) { return v->hv.unk_id; }
int32_t wp_vocab_token_flags(const wp_vocab *v, int64_t i) {
  return token_flags(v->hv.tokens[static_cast<size_t>(i)]);
}
int64_t wp_vocab_token_len(const wp_vocab *v, int64_t i) {
  return static_cast<int64_t>(v->hv.tokens[static_cast<size_t>(i)].word.size());
}

int wp_set_option(wp_vocab *v, int option, int64_t value) {
  switch (option) {
    case WP_OPT_FULL_DEPTH: v->full_depth = value != 0; return WP_OK;
    case WP_OPT_DEVICE:
      if (v->ctx) {
        g_last_error = "device already bound";
        return WP_ERR_ARG;
      }
      v->device = static_cast<int>(value);
      return WP_OK;
    case WP_OPT_KEEP_DEBUG:  // (2: the step views by position alone; the layout stays the default one)
      v->keep_debug = value != 0 && value != 2;
      v->keep_step_views = value == 2;
      return WP_OK;
    case WP_OPT_STAGE_TIMING: v->stage_timing = value != 0; return WP_OK;
    case WP_OPT_LCP_KASAI: v->lcp_kasai = value != 0; return WP_OK;
    case WP_OPT_COVER_ANCHORS: v->cover_anchors = value != 0; return WP_OK;
    case WP_OPT_ARENA_GUARD: v->arena_guard = value != 0; return WP_OK;
    case WP_OPT_VOCAB_IN_S: v->vocab_in_s = value != 0; return WP_OK;
    case WP_OPT_SPARSE_EMIT: v->sparse_emit = value != 0; return WP_OK;
    case WP_OPT_INDEXED_ROUND0: v->indexed_round0 = value != 0; return WP_OK;
    case WP_OPT_SORT_BLANKS: v->sort_blanks = value != 0; return WP_OK;
    case WP_OPT_LATE_REFINE: v->late_refine = value != 0; return WP_OK;
    case WP_OPT_NORMALIZE:
      if (!known_norm_flags(value)) {
        g_last_error = "WP_OPT_NORMALIZE: unknown flag bits (WP_NORM_CLEAN | WP_NORM_LOWER | WP_NORM_STRIP_ACCENTS)";
        return WP_ERR_ARG;
      }
      v->normalize = static_cast<int>(value);
      return WP_OK;
    case WP_OPT_DEVICES: v->n_devices = value < 0 ? -1 : static_cast<int>(std::max<int64_t>(value, 1)); return WP_OK;
  }
  g_last_error = "unknown option";
  return WP_ERR_ARG;
}

int wp_normalize_cp(int flags, uint32_t cp, uint32_t out[3]) {
  if (!known_norm_flags(flags) || cp >= 0x110000u || (cp >= 0xd800u && cp < 0xe000u)) return -1;
  uint32_t o[3] = {0, 0, 0};
  const int n = norm_cp(host_norm_tables(), flags, cp, o);
  for (int i = 0; i < n; i++) out[i] = o[i];
  return n;
}

int wp_normalize_device(wp_vocab *v, const void *d_utf8, size_t nbytes, int flags, const void **d_out, size_t *out_bytes) {
  return guarded([&] {
    *d_out = nullptr;
    *out_bytes = 0;
    if (!known_norm_flags(flags)) throw std::invalid_argument("normalize: unknown flag bits");
    if (nbytes == 0) return;
    check_device_text(d_utf8);
    Context *c = get_context(v);
    NormResult r;
    normalize_on_device(c, static_cast<const uint8_t *>(d_utf8), nbytes, flags, false, false, r);
    WP_HIP(hipStreamSynchronize(c->stream));
    *d_out = r.nbytes ? r.text : nullptr;
    *out_bytes = r.nbytes;
  });
}

int wp_get_stats(const wp_vocab *v, wp_stats *out) {
  *out = v->stats;
  return WP_OK;
}

int wp_get_norm_stats(const wp_vocab *v, wp_norm_stats *out) {
  out->normalize = v->stats.normalize;
  out->norm_bytes = v->stats.norm_bytes;
  out->ms_normalize = v->stats.ms_normalize;
  return WP_OK;
}

int wp_get_walk_stats(const wp_vocab *v, wp_walk_stats *out) {
  *out = v->stats.walk;
  return WP_OK;
}

int wp_get_refine_stats(const wp_vocab *v, wp_refine_stats *out) {
  *out = v->stats.refine;
  return WP_OK;
}

int wp_get_step_stats(const wp_vocab *v, wp_step_stats *out) {
  if (!v || !out) {
    g_last_error = "wp_get_step_stats: NULL handle or out pointer";
    return WP_ERR_ARG;
  }
  *out = v->stats.step;
  return WP_OK;
}

int wp_get_refine_sched(const wp_vocab *v, wp_refine_sched *out) {
  if (!v || !out) {
    g_last_error = "wp_get_refine_sched: NULL handle or out pointer";
    return WP_ERR_ARG;
  }
  *out = v->stats.sched;
  return WP_OK;
}

int wp_get_inputs_stats(const wp_vocab *v, wp_inputs_stats *out) {
  *out = v->stats.inputs;
  if (!v->stats.inputs_call) out->n_out = -1;
  return WP_OK;
}

int wp_linear_encode_device(wp_vocab *v, const void *d_utf8, size_t nbytes, const int32_t **d_ids, size_t *n_ids) {
  return guarded([&] {
    check_device_text(d_utf8);
    size_t n = 0;
    Context *c = get_context(v);
    encode_on_device(v, c, static_cast<const uint8_t *>(d_utf8), nbytes, &n, v->stats);
    v->stats.n_devices = 1;
    *d_ids = n ? c->d_ids : nullptr;
    *n_ids = n;
  });
}

}  // extern "C"

// ---- host buffers for the ids ------------------------------------------------------------------------
// The ids leave the device into page-locked host memory (a download into freshly malloc'd pages runs
// at 13-26 GB/s, into pinned memory at the link rate) and that very block is handed to the caller;
// wp_free() recognises it and puts it back into a small pool instead of unpinning it.
namespace {
struct PinnedPool {
  std::mutex mu;
  std::unordered_map<void *, size_t> owned;       // every live pinned block (handed out or pooled) -> capacity
  std::vector<std::pair<size_t, void *>> pooled;  // free blocks
  static constexpr size_t kMaxPooledBlocks = 4;
  static constexpr size_t kMaxPooledBytes = size_t(6) << 30;
  void *take(size_t bytes) {
    {
      std::lock_guard<std::mutex> g(mu);
      size_t best = pooled.size();
      for (size_t i = 0; i < pooled.size(); i++) {
        if (pooled[i].first >= bytes && (best == pooled.size() || pooled[i].first < pooled[best].first)) best = i;
      }
      if (best != pooled.size()) {
        void *p = pooled[best].second;
        pooled.erase(pooled.begin() + static_cast<long>(best));
        return p;
      }
    }
    void *p = nullptr;
    const size_t want = bytes + bytes / 8 + 4096;
    WP_HIP(hipHostMalloc(&p, want));
    std::lock_guard<std::mutex> g(mu);
    owned[p] = want;
    return p;
  }
  // true: p was one of ours (now pooled or released)
  bool give_back(void *p) {
    size_t cap = 0;
    {
      std::lock_guard<std::mutex> g(mu);
      auto it = owned.find(p);
      if (it == owned.end()) return false;
      cap = it->second;
      size_t bytes = cap;
      for (auto &b : pooled) bytes += b.first;
      if (pooled.size() < kMaxPooledBlocks && bytes <= kMaxPooledBytes) {
        pooled.emplace_back(cap, p);
        return true;
      }
      owned.erase(it);
    }
    (void)hipHostFree(p);
    return true;
  }
  void trim() {  // pooled (free) blocks go back to the driver
    std::vector<std::pair<size_t, void *>> drop;
    {
      std::lock_guard<std::mutex> g(mu);
      drop.swap(pooled);
      for (auto &b : drop) owned.erase(b.second);
    }
    for (auto &b : drop) (void)hipHostFree(b.second);
  }
};
PinnedPool &id_pool() {
  static PinnedPool *pool = new PinnedPool();  // never destroyed: blocks may outlive static destruction order
  return *pool;
}
struct PinnedBlock {  // returns the block to the pool unless release()d to the caller
  void *p = nullptr;
  explicit PinnedBlock(size_t bytes) : p(id_pool().take(bytes)) {}
  ~PinnedBlock() {
    if (p) id_pool().give_back(p);
  }
  void *release() {
    void *r = p;
    p = nullptr;
    return r;
  }
};

// Device ranges on their way to the caller as pinned blocks.  add() takes a block from id_pool() and queues the copy on
// the stream; finish() waits once and only then stores the blocks through the caller's out-pointers.  Whatever throws
// before that, every block goes back to the pool.
class Downloads {
  hipStream_t st;
  std::vector<std::pair<void *, void *>> items;  // block, the caller's pointer to hand it over through

 public:
  explicit Downloads(hipStream_t stream) : st(stream) {}
  ~Downloads() {
    for (auto &it : items) id_pool().give_back(it.first);
  }
  template <typename T>
  void add(T **out, const void *d_src, size_t bytes) {
    items.reserve(items.size() + 1);
    items.emplace_back(id_pool().take(bytes), out);
    WP_HIP(hipMemcpyAsync(items.back().first, d_src, bytes, hipMemcpyDeviceToHost, st));
  }
  // a field of a result copied from the device's: the device range it names is queued and the field cleared until
  // finish(); a field that is NULL stays NULL
  template <typename T>
  void swap(T **field, size_t bytes) {
    const void *d_src = *field;
    *field = nullptr;
    if (d_src) add(field, d_src, bytes);
  }
  void finish() {
    WP_HIP(hipStreamSynchronize(st));
    for (auto &it : items) std::memcpy(it.second, &it.first, sizeof(void *));  // (*out = block, for every T * alike)
    items.clear();
  }
};

// the compact form in a result h copied from the device's: n_kept rows (kept: their indices, where the result lists them)
template <typename Result>
void swap_compact(Downloads &down, Result &h, int64_t n_kept, uint32_t elem_bytes) {
  down.swap(&h.kept, static_cast<size_t>(n_kept) * sizeof(int32_t));
  down.swap(&h.row_off, static_cast<size_t>(n_kept + 1) * sizeof(int64_t));
  down.swap(&h.data, static_cast<size_t>(h.n_elems) * elem_bytes);
}
// the five fields that the results of dedup and neardup share
template <typename Result>
void swap_table(Downloads &down, Result &h, uint32_t elem_bytes) {
  down.swap(&h.counts, static_cast<size_t>(h.n_unique) * sizeof(int64_t));
  down.swap(&h.inverse, static_cast<size_t>(h.n_rows) * sizeof(int32_t));
  swap_compact(down, h, h.n_unique, elem_bytes);
}

// the batch of a device call: the alignment its arrays need, under the names a message calls them
RaggedIn device_batch(const char *layer, const void *d_data, const int64_t *d_row_off, size_t n_rows, uint32_t elem_bytes, const char *off_name = "row_off",
                      const char *data_name = "data") {
  if ((reinterpret_cast<uintptr_t>(d_row_off) & 7) != 0) throw std::invalid_argument(std::string(layer) + ": " + off_name + " must be 8-byte aligned");
  if ((reinterpret_cast<uintptr_t>(d_data) & 3) != 0) throw std::invalid_argument(std::string(layer) + ": " + data_name + " must be 4-byte aligned");
  return RaggedIn{d_data, reinterpret_cast<const long long *>(d_row_off), n_rows, elem_bytes};
}

using wp_clock = std::chrono::steady_clock;
double ms_since(wp_clock::time_point t0) { return std::chrono::duration<double, std::milli>(wp_clock::now() - t0).count(); }

// The batch of a call whose documents are all empty, on the host: n rows of specials and padding, and their lengths.
// token_types / sample: the two further arrays of an inputs call (nullptr: a padded call); second_sep: its pair form.
void fill_empty_rows(size_t n, int max_len, int32_t cls_id, int32_t sep_id, int32_t pad_id, bool second_sep, int32_t *ids,
                     int32_t *lengths, int32_t *token_types, int32_t *sample) {
  for (size_t r = 0; r < n; r++) {
    int32_t *row = ids + r * static_cast<size_t>(max_len);
    int col = 0;
    if (cls_id >= 0) row[col++] = cls_id;
    if (sep_id >= 0) row[col++] = sep_id;
    if (second_sep && sep_id >= 0) {
      token_types[r * static_cast<size_t>(max_len) + col] = 1;
      row[col++] = sep_id;
    }
    lengths[r] = col;
    while (col < max_len) row[col++] = pad_id;
    if (sample) sample[r] = static_cast<int32_t>(r);
  }
}

bool ascii_space(uint8_t b) { return (b >= 0x09 && b <= 0x0d) || b == 0x20; }

// Cuts [0, nbytes) into `parts` ranges at ASCII whitespace (no word straddles two shards),
// balanced by code points rather than bytes: the cost of a shard follows its symbol count, and a
// mixed-script corpus has 1-3 bytes per code point depending on where one looks.  Code points are
// estimated from every 64th 4 KB page (lead bytes = bytes that are not 10xxxxxx).
// kept_only: cut only at the blanks WP_NORM_CLEAN keeps (it drops U+000B and U+000C, which then join their neighbours).
std::vector<size_t> shard_cuts(const char *utf8, size_t nbytes, int parts, bool kept_only = false) {
  std::vector<size_t> cuts(static_cast<size_t>(parts) + 1, nbytes);
  cuts[0] = 0;
  if (parts <= 1) return cuts;
  const uint8_t *b = reinterpret_cast<const uint8_t *>(utf8);
  const size_t blocks = std::min<size_t>(static_cast<size_t>(parts) * 256, std::max<size_t>(1, nbytes / 4096));
  const size_t blk = (nbytes + blocks - 1) / blocks;
  std::vector<double> cum(blocks + 1, 0.0);
  for (size_t i = 0; i < blocks; i++) {
    const size_t lo = i * blk, hi = std::min(nbytes, lo + blk);
    size_t leads = 0, seen = 0;
    for (size_t page = lo; page < hi; page += 64 * 4096) {
      const size_t e = std::min(hi, page + 4096);
      for (size_t q = page; q < e; q++) leads += (b[q] & 0xc0u) != 0x80u;
      seen += e - page;
    }
    const double density = seen ? static_cast<double>(leads) / static_cast<double>(seen) : 1.0;
    cum[i + 1] = cum[i] + density * static_cast<double>(hi > lo ? hi - lo : 0);
  }
  size_t i = 0;
  for (int r = 1; r < parts; r++) {
    const double want = cum[blocks] * r / parts;
    while (i + 1 < blocks && cum[i + 1] < want) i++;
    const double span = cum[i + 1] - cum[i];
    size_t pos = i * blk + (span > 0 ? static_cast<size_t>((want - cum[i]) / span * static_cast<double>(blk)) : 0);
    pos = std::max(pos, cuts[static_cast<size_t>(r) - 1]);
    while (pos < nbytes && (!ascii_space(b[pos]) || (kept_only && (b[pos] == 0x0b || b[pos] == 0x0c)))) pos++;
    cuts[static_cast<size_t>(r)] = std::min(pos, nbytes);
  }
  return cuts;
}

// One shard per entry of `devices` (ordinals may repeat: several contexts on one GPU), one host thread
// per shard for upload + device path, then every shard's ids are downloaded straight to their place in
// one pinned host block (exact sizes, no padded gather).
void encode_multi(wp_vocab *v, const char *utf8, size_t nbytes, const std::vector<int> &devices_in, int32_t **ids,
                  size_t *n_ids) {
  // a vocabulary with whitespace inside a token can match across a cut (the reference's own chunking has the
  // same caveat): such a text stays in one piece on the first device
  const std::vector<int> devices = v->hv.space_in_token ? std::vector<int>(devices_in.begin(), devices_in.begin() + 1)
                                                        : devices_in;
  const int G = static_cast<int>(devices.size());
  const auto t_all = wp_clock::now();
  const std::vector<size_t> cuts = shard_cuts(utf8, nbytes, G, (v->normalize & WP_NORM_CLEAN) != 0);
  if (v->multi.size() < static_cast<size_t>(G)) v->multi.resize(static_cast<size_t>(G));
  for (int g = 0; g < G; g++) {  // (contexts are made on the calling thread: a failure here is a plain exception)
    if (cuts[static_cast<size_t>(g)] == cuts[static_cast<size_t>(g) + 1]) continue;  // an empty shard needs none
    Context *c = v->multi[static_cast<size_t>(g)].get();
    if (c && c->device != devices[static_cast<size_t>(g)]) park_context(std::move(v->multi[static_cast<size_t>(g)]));
    if (!v->multi[static_cast<size_t>(g)]) v->multi[static_cast<size_t>(g)] = make_context(v, devices[static_cast<size_t>(g)]);
  }
  std::vector<size_t> counts(static_cast<size_t>(G), 0);
  std::vector<EncodeStats> stats(static_cast<size_t>(G));
  std::vector<std::string> errors(static_cast<size_t>(G));
  std::vector<int> codes(static_cast<size_t>(G), WP_OK);
  auto work = [&](int g) {
    Context *c = v->multi[static_cast<size_t>(g)].get();
    const size_t lo = cuts[static_cast<size_t>(g)], hi = cuts[static_cast<size_t>(g) + 1];
    codes[static_cast<size_t>(g)] = guarded([&] {
      WP_HIP(hipSetDevice(c->device));
      std::memset(&stats[static_cast<size_t>(g)], 0, sizeof(EncodeStats));
      if (hi == lo) return;
      upload_text(c, utf8 + lo, hi - lo);
      encode_on_device(v, c, static_cast<const uint8_t *>(c->text_buf.p), hi - lo, &counts[static_cast<size_t>(g)],
                       stats[static_cast<size_t>(g)]);
    });
    if (codes[static_cast<size_t>(g)] != WP_OK) {
      try {
        errors[static_cast<size_t>(g)] = g_last_error;
      } catch (...) {  // (out of memory while copying the message: the code alone is reported)
      }
    }
  };
  {
    // Worker threads are joined on every way out of this scope (a std::thread that is still joinable when it is
    // destroyed ends the process: std::terminate), work() itself cannot throw (everything that can sits inside
    // guarded(), the error slots are sized up front), and a shard without bytes gets no thread at all.
    struct Joiner {
      std::vector<std::thread> threads;
      ~Joiner() {
        for (auto &t : threads) {
          if (t.joinable()) t.join();
        }
      }
    } pool;
    pool.threads.reserve(static_cast<size_t>(G));
    int own = -1;  // the first non-empty shard runs on the calling thread
    for (int g = 0; g < G; g++) {
      if (cuts[static_cast<size_t>(g)] == cuts[static_cast<size_t>(g) + 1]) {
        std::memset(&stats[static_cast<size_t>(g)], 0, sizeof(EncodeStats));
        continue;
      }
      if (own < 0) {
        own = g;
        continue;
      }
      try {
        pool.threads.emplace_back(work, g);
      } catch (const std::exception &e) {  // (no thread to be had: the shard runs here, after the others were started)
        work(g);
      }
    }
    if (own >= 0) work(own);
  }
  for (int g = 0; g < G; g++) {
    if (codes[static_cast<size_t>(g)] == WP_OK) continue;
    const std::string msg = "shard " + std::to_string(g) + " (device " + std::to_string(devices[static_cast<size_t>(g)]) + "): " +
                            errors[static_cast<size_t>(g)];
    if (codes[static_cast<size_t>(g)] == WP_ERR_TOO_LARGE) throw std::length_error(errors[static_cast<size_t>(g)]);
    throw HipError(msg);
  }
  size_t total = 0;
  std::vector<size_t> offs(static_cast<size_t>(G), 0);
  for (int g = 0; g < G; g++) {
    offs[static_cast<size_t>(g)] = total;
    total += counts[static_cast<size_t>(g)];
  }
  const auto t_d2h = wp_clock::now();
  if (total) {
    PinnedBlock blk(total * sizeof(int32_t));
    int32_t *h = static_cast<int32_t *>(blk.p);
    for (int g = 0; g < G; g++) {  // all downloads in flight together, each on its own device's stream
      Context *c = v->multi[static_cast<size_t>(g)].get();
      if (!counts[static_cast<size_t>(g)]) continue;
      WP_HIP(hipSetDevice(c->device));
      WP_HIP(hipMemcpyAsync(h + offs[static_cast<size_t>(g)], c->d_ids, counts[static_cast<size_t>(g)] * sizeof(int32_t),
                            hipMemcpyDeviceToHost, c->stream));
    }
    for (int g = 0; g < G; g++) {
      Context *c = v->multi[static_cast<size_t>(g)].get();
      if (!counts[static_cast<size_t>(g)]) continue;
      WP_HIP(hipSetDevice(c->device));
      WP_HIP(hipStreamSynchronize(c->stream));
    }
    *ids = static_cast<int32_t *>(blk.release());
    *n_ids = total;
  }
  // statistics of the call: sums over the shards, the slowest shard's device times
  EncodeStats &S = v->stats;
  S = stats[0];
  for (int g = 1; g < G; g++) {
    const EncodeStats &T = stats[static_cast<size_t>(g)];
    S.n_bytes += T.n_bytes;
    S.n_text += T.n_text;
    S.n_total += T.n_total;
    S.n_ids += T.n_ids;
    S.n_anchors += T.n_anchors;
    S.alphabet = std::max(S.alphabet, T.alphabet);
    S.rounds = std::max(S.rounds, T.rounds);
    S.radix_passes += T.radix_passes;
    S.radix_pass_elems += T.radix_pass_elems;
    S.radix_digit_bytes += T.radix_digit_bytes;
    S.radix_pass_bytes += T.radix_pass_bytes;
    S.round0_sorted += T.round0_sorted;
    S.norm_bytes += T.norm_bytes;
    S.ms_normalize = std::max(S.ms_normalize, T.ms_normalize);
    S.walk.n_wide_words += T.walk.n_wide_words;
    S.walk.n_long_words += T.walk.n_long_words;
    S.walk.max_anchor_gap = std::max(S.walk.max_anchor_gap, T.walk.max_anchor_gap);
    S.refine.n_groups += T.refine.n_groups;
    S.refine.n_entries += T.refine.n_entries;
    S.refine.n_large_groups += T.refine.n_large_groups;
    S.refine.n_large_entries += T.refine.n_large_entries;
    S.ms_total = std::max(S.ms_total, T.ms_total);
    S.ms_decode = std::max(S.ms_decode, T.ms_decode);
    S.ms_sa = std::max(S.ms_sa, T.ms_sa);
    S.ms_lcp = std::max(S.ms_lcp, T.ms_lcp);
    S.ms_scan = std::max(S.ms_scan, T.ms_scan);
    S.ms_walk = std::max(S.ms_walk, T.ms_walk);
  }
  S.normalize = v->normalize;  // (shard 0 may have been empty)
  S.n_devices = G;
  S.ms_d2h = ms_since(t_d2h);
  S.ms_host_total = ms_since(t_all);
}

std::vector<int> resolve_devices(const int *devices, int n_devices) {
  std::vector<int> out;
  if (devices && n_devices > 0) {
    out.assign(devices, devices + n_devices);
    return out;
  }
  const int count = device_count_or_throw();
  const int want = n_devices <= 0 ? count : std::min(n_devices, count);
  for (int d = 0; d < want; d++) out.push_back(d);
  return out;
}
}  // namespace

extern "C" {

int wp_linear_encode_multi(wp_vocab *v, const char *utf8, size_t nbytes, const int *devices, int n_devices,
                           int32_t **ids, size_t *n_ids) {
  return guarded([&] {
    *ids = nullptr;
    *n_ids = 0;
    if (nbytes == 0) return;  // linear.cpp:323-325
    encode_multi(v, utf8, nbytes, resolve_devices(devices, n_devices), ids, n_ids);
  });
}

int wp_linear_encode(wp_vocab *v, const char *utf8, size_t nbytes, int32_t **ids, size_t *n_ids) {
  return guarded([&] {
    *ids = nullptr;
    *n_ids = 0;
    if (nbytes == 0) return;  // linear.cpp:323-325: the vocab path is not touched
    // WP_OPT_DEVICES / env WP_DEVICES: shard over several GPUs (inputs too small to be worth it stay on one)
    if (v->n_devices != 1 && nbytes >= (size_t(1) << 22)) {
      std::vector<int> devs = resolve_devices(nullptr, v->n_devices);
      const size_t per = size_t(1) << 21;  // at least 2 MB per shard
      if (devs.size() > nbytes / per) devs.resize(std::max<size_t>(1, nbytes / per));
      if (devs.size() > 1) {
        encode_multi(v, utf8, nbytes, devs, ids, n_ids);
        return;
      }
    }
    const auto t_all = wp_clock::now();
    Context *c = get_context(v);
    auto t0 = wp_clock::now();
    upload_text(c, utf8, nbytes);
    if (v->stage_timing) WP_HIP(hipStreamSynchronize(c->stream));
    const double ms_h2d = ms_since(t0);
    size_t n = 0;
    encode_on_device(v, c, static_cast<const uint8_t *>(c->text_buf.p), nbytes, &n, v->stats);
    t0 = wp_clock::now();
    if (n) {
      Downloads down(c->stream);
      down.add(ids, c->d_ids, n * sizeof(int32_t));
      down.finish();
      *n_ids = n;
    }
    v->stats.n_devices = 1;
    v->stats.ms_h2d = v->stage_timing ? ms_h2d : 0.0;
    v->stats.ms_d2h = ms_since(t0);
    v->stats.ms_host_total = ms_since(t_all);
  });
}

// offsets mode (include/wordpiece_amd.h): the unit and the byte unit's size limit, before any memory is touched
static void check_offsets_call(int unit, size_t nbytes) {
  if (unit != WP_OFFSETS_BYTES && unit != WP_OFFSETS_CODE_POINTS) throw std::invalid_argument("offsets unit must be 0 (bytes) or 1 (code points)");
  if (unit == WP_OFFSETS_BYTES && nbytes > static_cast<size_t>(UINT32_MAX)) {
    throw std::length_error("byte offsets need nbytes <= UINT32_MAX");
  }
}

int wp_linear_encode_offsets(wp_vocab *v, const char *utf8, size_t nbytes, int unit, int32_t **ids, uint32_t **offsets,
                             size_t *n_ids) {
  return guarded([&] {
    *ids = nullptr;
    *offsets = nullptr;
    *n_ids = 0;
    check_offsets_call(unit, nbytes);
    if (nbytes == 0) return;  // (no device needed, as wp_linear_encode)
    const auto t_all = wp_clock::now();
    Context *c = get_context(v);  // (the handle's own device: never sharded)
    upload_text(c, utf8, nbytes);
    size_t n = 0;
    encode_on_device(v, c, static_cast<const uint8_t *>(c->text_buf.p), nbytes, &n, v->stats, unit);
    const auto t0 = wp_clock::now();
    if (n) {
      Downloads down(c->stream);
      down.add(ids, c->d_ids, n * sizeof(int32_t));
      down.add(offsets, c->d_offs, n * 2 * sizeof(uint32_t));
      down.finish();
      *n_ids = n;
    }
    v->stats.n_devices = 1;
    v->stats.ms_d2h = ms_since(t0);
    v->stats.ms_host_total = ms_since(t_all);
  });
}

int wp_normalize(wp_vocab *v, const char *utf8, size_t nbytes, int flags, char **out, size_t *out_bytes) {
  return guarded([&] {
    *out = nullptr;
    *out_bytes = 0;
    if (!known_norm_flags(flags)) throw std::invalid_argument("normalize: unknown flag bits");
    if (nbytes == 0) return;  // (no device needed)
    Context *c = get_context(v);
    upload_text(c, utf8, nbytes);
    NormResult r;
    normalize_on_device(c, static_cast<const uint8_t *>(c->text_buf.p), nbytes, flags, false, false, r);
    if (r.nbytes) {
      Downloads down(c->stream);
      down.add(out, r.text, r.nbytes);
      down.finish();
      *out_bytes = r.nbytes;
    }
  });
}

int wp_linear_encode_offsets_device(wp_vocab *v, const void *d_utf8, size_t nbytes, int unit, const int32_t **d_ids,
                                    const uint32_t **d_offsets, size_t *n_ids) {
  return guarded([&] {
    *d_ids = nullptr;
    *d_offsets = nullptr;
    *n_ids = 0;
    check_offsets_call(unit, nbytes);
    if (nbytes == 0) return;
    check_device_text(d_utf8);
    size_t n = 0;
    Context *c = get_context(v);
    encode_on_device(v, c, static_cast<const uint8_t *>(d_utf8), nbytes, &n, v->stats, unit);
    v->stats.n_devices = 1;
    *d_ids = n ? c->d_ids : nullptr;
    *d_offsets = n ? c->d_offs : nullptr;
    *n_ids = n;
  });
}

}  // extern "C"

// ---- documents (include/wordpiece_amd.h, section "documents"; host path: rows_path.h) -------------------------------
extern "C" {

int wp_linear_encode_rows(wp_vocab *v, const char *utf8, size_t nbytes, const int64_t *doc_off, size_t n_docs, int unit,
                          int32_t **ids, int64_t **row_splits, uint32_t **offsets, size_t *n_ids, size_t *n_rows) {
  return guarded([&] {
    *ids = nullptr;
    *row_splits = nullptr;
    if (offsets) *offsets = nullptr;
    *n_ids = 0;
    *n_rows = 0;
    check_rows_call(unit, nbytes);
    if (unit >= 0 && !offsets) throw std::invalid_argument("offsets asked for without a place to return them");
    if (doc_off) check_doc_off_host(utf8, nbytes, doc_off, n_docs);
    if (nbytes == 0 || (doc_off && nbytes == n_docs)) {  // no text, or empty documents only: no device needed
      const size_t rows = doc_off ? n_docs : 0;
      *row_splits = static_cast<int64_t *>(zeroed((rows + 1) * sizeof(int64_t)));
      *n_rows = rows;
      return;
    }
    const auto t_all = wp_clock::now();
    RowsResult r;
    Context *c = rows_from_host(v, utf8, nbytes, doc_off, n_docs, unit, r);
    const auto t0 = wp_clock::now();
    Downloads down(c->stream);
    down.add(row_splits, r.d_row_splits, (r.n_rows + 1) * sizeof(int64_t));
    if (r.n_ids) down.add(ids, r.d_ids, r.n_ids * sizeof(int32_t));
    if (r.n_ids && unit >= 0) down.add(offsets, r.d_offs, r.n_ids * 2 * sizeof(uint32_t));
    down.finish();
    *n_ids = r.n_ids;
    *n_rows = r.n_rows;
    v->stats.ms_d2h = ms_since(t0);
    v->stats.ms_host_total = ms_since(t_all);
  });
}

int wp_linear_encode_rows_device(wp_vocab *v, const void *d_utf8, size_t nbytes, const int64_t *d_doc_off, size_t n_docs,
                                 int unit, const int32_t **d_ids, const int64_t **d_row_splits, const uint32_t **d_offsets,
                                 size_t *n_ids, size_t *n_rows) {
  return guarded([&] {
    *d_ids = nullptr;
    *d_row_splits = nullptr;
    if (d_offsets) *d_offsets = nullptr;
    *n_ids = 0;
    *n_rows = 0;
    check_rows_call(unit, nbytes);
    if (unit >= 0 && !d_offsets) throw std::invalid_argument("offsets asked for without a place to return them");
    check_device_text(d_utf8);
    check_device_doc_off(d_doc_off);
    Context *c = get_context(v);
    if (nbytes == 0) {  // no text: no rows (explicit rows cannot end at 0 unless there are none)
      check_doc_off_without_text(d_doc_off, n_docs);
      c->rows_out.ensure(sizeof(int64_t));
      WP_HIP(hipMemsetAsync(c->rows_out.p, 0, sizeof(int64_t), c->stream));
      WP_HIP(hipStreamSynchronize(c->stream));
      *d_row_splits = static_cast<const int64_t *>(c->rows_out.p);
      return;
    }
    RowsResult r;
    rows_on_device(v, c, static_cast<const uint8_t *>(d_utf8), nbytes, reinterpret_cast<const long long *>(d_doc_off), n_docs, unit,
                   SIZE_MAX, r);
    *d_ids = r.d_ids;
    *d_row_splits = reinterpret_cast<const int64_t *>(r.d_row_splits);
    if (d_offsets) *d_offsets = r.d_offs;
    *n_ids = r.n_ids;
    *n_rows = r.n_rows;
  });
}

int wp_linear_encode_padded(wp_vocab *v, const char *utf8, size_t nbytes, const int64_t *doc_off, size_t n_docs, int max_len,
                            int32_t cls_id, int32_t sep_id, int32_t pad_id, int32_t **input_ids, int32_t **lengths,
                            size_t *n_rows) {
  return guarded([&] {
    *input_ids = nullptr;
    *lengths = nullptr;
    *n_rows = 0;
    check_rows_call(-1, nbytes);
    (void)padded_specials(max_len, cls_id, sep_id);
    if (doc_off) check_doc_off_host(utf8, nbytes, doc_off, n_docs);
    if (nbytes == 0 || (doc_off && nbytes == n_docs)) {  // rows of specials and padding only: no device needed
      const size_t rows = doc_off ? n_docs : 0;
      int32_t *out = static_cast<int32_t *>(zeroed(rows * static_cast<size_t>(max_len) * sizeof(int32_t)));
      int32_t *len = static_cast<int32_t *>(zeroed(rows * sizeof(int32_t)));
      fill_empty_rows(rows, max_len, cls_id, sep_id, pad_id, false, out, len, nullptr, nullptr);
      *input_ids = out;
      *lengths = len;
      *n_rows = rows;
      return;
    }
    const auto t_all = wp_clock::now();
    RowsResult r;
    Context *c = rows_from_host(v, utf8, nbytes, doc_off, n_docs, -1, r);
    const PaddedBatch b = padded_batch(c, r.n_rows, max_len);
    pad_rows_on_device(v, c, r, max_len, cls_id, sep_id, pad_id, b.d_input_ids, b.d_lengths);
    Downloads down(c->stream);
    down.add(input_ids, b.d_input_ids, r.n_rows * static_cast<size_t>(max_len) * sizeof(int32_t));
    down.add(lengths, b.d_lengths, r.n_rows * sizeof(int32_t));
    down.finish();
    *n_rows = r.n_rows;
    v->stats.ms_host_total = ms_since(t_all);
  });
}

int wp_linear_encode_padded_device(wp_vocab *v, const void *d_utf8, size_t nbytes, const int64_t *d_doc_off, size_t n_docs,
                                   int max_len, int32_t cls_id, int32_t sep_id, int32_t pad_id, int32_t *d_input_ids,
                                   int32_t *d_lengths, size_t capacity_rows, size_t *n_rows) {
  return guarded([&] {
    *n_rows = 0;
    check_rows_call(-1, nbytes);
    (void)padded_specials(max_len, cls_id, sep_id);
    check_device_text(d_utf8);
    check_device_doc_off(d_doc_off);
    if (nbytes == 0) {
      check_doc_off_without_text(d_doc_off, n_docs);
      return;
    }
    if (!d_input_ids || !d_lengths) throw std::invalid_argument("null output buffer");
    Context *c = get_context(v);
    RowsResult r;
    try {
      rows_on_device(v, c, static_cast<const uint8_t *>(d_utf8), nbytes, reinterpret_cast<const long long *>(d_doc_off), n_docs, -1,
                     capacity_rows, r);
    } catch (...) {
      *n_rows = r.n_rows;  // (too many rows for the caller's buffers: the count it needs)
      throw;
    }
    pad_rows_on_device(v, c, r, max_len, cls_id, sep_id, pad_id, d_input_ids, d_lengths);
    *n_rows = r.n_rows;
  });
}

}  // extern "C"

// ---- masking (include/wordpiece_amd.h, section "masking"; host path: mask_path.h) ------------------------------------
// the host entry points behind their argument rules: mask_from_host, then the 1..3 blocks the caller asked for come down
static void mask_host_call(wp_vocab *v, const int32_t *input_ids, const int32_t *lengths, size_t n_rows, const MaskGeom &g, int32_t **masked,
                           int32_t **labels, int32_t **word_ids) {
  Context *c = get_context(v);
  const MaskBatch b = mask_from_host(v, c, input_ids, lengths, n_rows, g, masked != nullptr, word_ids != nullptr);
  const size_t bytes = n_rows * static_cast<size_t>(g.max_len) * sizeof(int32_t);
  Downloads down(c->stream);
  if (masked) {
    down.add(masked, b.d_masked, bytes);
    down.add(labels, b.d_labels, bytes);
  }
  if (word_ids) down.add(word_ids, b.d_word_ids, bytes);
  down.finish();
}

extern "C" {

int wp_get_mask_stats(const wp_vocab *v, wp_mask_stats *out) {
  *out = v->stats.mask;
  if (!v->stats.mask_call) out->n_rows = -1;
  return WP_OK;
}

int wp_word_ids(wp_vocab *v, const int32_t *input_ids, const int32_t *lengths, size_t n_rows, const wp_mask_spec *spec,
                int32_t **word_ids) {
  return guarded([&] {
    if (!word_ids) throw std::invalid_argument("mask: word_ids is NULL");
    *word_ids = nullptr;
    const MaskGeom g = check_mask_spec(v, spec, n_rows, false);
    if (n_rows != 0 && !input_ids) throw std::invalid_argument("mask: input_ids is NULL");
    if (n_rows == 0) {
      begin_mask_stats(v, 0, 0);
      return;
    }
    mask_host_call(v, input_ids, lengths, n_rows, g, nullptr, nullptr, word_ids);
  });
}

int wp_word_ids_device(wp_vocab *v, const int32_t *d_input_ids, const int32_t *d_lengths, size_t n_rows,
                       const wp_mask_spec *spec, int32_t *d_word_ids) {
  return guarded([&] {
    const MaskGeom g = check_mask_spec(v, spec, n_rows, false);
    if (n_rows != 0 && !d_input_ids) throw std::invalid_argument("mask: input_ids is NULL");
    if (n_rows != 0 && !d_word_ids) throw std::invalid_argument("mask: word_ids is NULL");
    if (n_rows == 0) {
      begin_mask_stats(v, 0, 0);
      return;
    }
    mask_on_device(v, get_context(v), d_input_ids, d_lengths, n_rows, g, nullptr, nullptr, d_word_ids);
  });
}

int wp_mlm_mask(wp_vocab *v, const int32_t *input_ids, const int32_t *lengths, size_t n_rows, const wp_mask_spec *spec,
                int32_t **masked, int32_t **labels, int32_t **word_ids) {
  return guarded([&] {
    if (!masked) throw std::invalid_argument("mask: masked is NULL");
    if (!labels) throw std::invalid_argument("mask: labels is NULL");
    *masked = nullptr;
    *labels = nullptr;
    if (word_ids) *word_ids = nullptr;
    const MaskGeom g = check_mask_spec(v, spec, n_rows, true);
    if (n_rows != 0 && !input_ids) throw std::invalid_argument("mask: input_ids is NULL");
    if (n_rows == 0) {
      begin_mask_stats(v, 0, g.whole_word);
      return;
    }
    mask_host_call(v, input_ids, lengths, n_rows, g, masked, labels, word_ids);
  });
}

int wp_mlm_mask_device(wp_vocab *v, const int32_t *d_input_ids, const int32_t *d_lengths, size_t n_rows,
                       const wp_mask_spec *spec, int32_t *d_masked, int32_t *d_labels, int32_t *d_word_ids) {
  return guarded([&] {
    const MaskGeom g = check_mask_spec(v, spec, n_rows, true);
    if (n_rows != 0 && !d_input_ids) throw std::invalid_argument("mask: input_ids is NULL");
    if (n_rows != 0 && !d_masked) throw std::invalid_argument("mask: masked is NULL");
    if (n_rows != 0 && !d_labels) throw std::invalid_argument("mask: labels is NULL");
    if (n_rows == 0) {
      begin_mask_stats(v, 0, g.whole_word);
      return;
    }
    mask_on_device(v, get_context(v), d_input_ids, d_lengths, n_rows, g, d_masked, d_labels, d_word_ids);
  });
}

}  // extern "C"

// ---- detokenize (include/wordpiece_amd.h, section "detokenize"; host path: detok_path.h) -----------------------------
extern "C" {

int wp_get_detok_stats(const wp_vocab *v, wp_detok_stats *out) {
  *out = v->stats.detok;
  if (!v->stats.detok_call) out->n_rows = -1;
  return WP_OK;
}

int64_t wp_detok_piece(const wp_vocab *v, int64_t id, int form, int cleanup, char *buf, size_t cap) {
  if (id < 0 || static_cast<size_t>(id) >= v->hv.tokens.size() || (form != 0 && form != 1) || (cleanup != 0 && cleanup != 1)) return -1;
  const HostToken &t = v->hv.tokens[static_cast<size_t>(id)];
  if (t.is_malformed) return -1;
  const std::string piece = detok_piece_bytes(t, form, cleanup);
  if (buf && cap) std::memcpy(buf, piece.data(), std::min(cap, piece.size()));
  return static_cast<int64_t>(piece.size());
}

int wp_detokenize(wp_vocab *v, const int32_t *ids, const int64_t *row_splits, const int32_t *lengths, size_t n_rows,
                  const wp_detok_spec *spec, char **text, int64_t **text_off, size_t *n_bytes) {
  return guarded([&] {
    if (!text || !text_off || !n_bytes) throw std::invalid_argument("detokenize: an out-pointer is NULL");
    *text = nullptr;
    *text_off = nullptr;
    *n_bytes = 0;
    DetokGeom g = check_detok_spec(v, spec, n_rows);
    if (g.max_len == 0) {
      if (!row_splits) throw std::invalid_argument("detokenize: a ragged call needs row_splits");
      g.n_cells = check_row_splits("detokenize", row_splits, n_rows);
      if (g.n_cells > INT32_MAX) throw std::length_error("detokenize: more cells than INT32_MAX");
    }
    if (g.n_cells > 0 && !ids) throw std::invalid_argument("detokenize: ids is NULL");
    if (n_rows == 0) {
      *text_off = static_cast<int64_t *>(zeroed(sizeof(int64_t)));
      begin_detok_stats(v, 0);
      return;
    }
    Context *c = get_context(v);
    const bool ragged = g.max_len == 0;
    const void *rows = ragged ? static_cast<const void *>(row_splits) : static_cast<const void *>(lengths);
    const StagedRows in = stage_ids_and_rows(c->detok_in, c->stream, ids, static_cast<size_t>(g.n_cells), rows,
                                             ragged ? (n_rows + 1) * sizeof(int64_t) : n_rows * sizeof(int32_t), n_rows);
    const void *d_text = nullptr;
    const long long *d_off = nullptr;
    size_t nb = 0;
    detok_on_device(v, c, in.d_ids, ragged ? in.d_rows : nullptr, !ragged && lengths ? reinterpret_cast<const int32_t *>(in.d_rows) : nullptr,
                    g, spec->cleanup, &d_text, &d_off, &nb);
    Downloads down(c->stream);
    if (nb) down.add(text, d_text, nb);
    down.add(text_off, d_off, (n_rows + 1) * sizeof(int64_t));
    down.finish();
    *n_bytes = nb;
  });
}

int wp_detokenize_device(wp_vocab *v, const int32_t *d_ids, const int64_t *d_row_splits, const int32_t *d_lengths,
                         size_t n_rows, const wp_detok_spec *spec, const void **d_text, const int64_t **d_text_off,
                         size_t *n_bytes) {
  return guarded([&] {
    if (!d_text || !d_text_off || !n_bytes) throw std::invalid_argument("detokenize: an out-pointer is NULL");
    *d_text = nullptr;
    *d_text_off = nullptr;
    *n_bytes = 0;
    DetokGeom g = check_detok_spec(v, spec, n_rows);
    if (g.max_len == 0 && !d_row_splits) throw std::invalid_argument("detokenize: a ragged call needs row_splits");
    const char *aligned = "detokenize: device ids and lengths must be 4-byte aligned, row_splits 8-byte aligned";
    check_aligned(d_ids, 4, aligned);
    check_aligned(d_lengths, 4, aligned);
    check_aligned(d_row_splits, 8, aligned);
    const long long *d_off = nullptr;
    detok_on_device(v, get_context(v), d_ids, g.max_len == 0 ? reinterpret_cast<const long long *>(d_row_splits) : nullptr,
                    g.max_len == 0 ? nullptr : d_lengths, g, spec->cleanup, d_text, &d_off, n_bytes);
    *d_text_off = reinterpret_cast<const int64_t *>(d_off);
  });
}

}  // extern "C"

// ---- pack (include/wordpiece_amd.h, section "pack"; host path: pack_path.h) ------------------------------------------
extern "C" {

int wp_get_pack_stats(const wp_vocab *v, wp_pack_stats *out) {
  *out = v->stats.pack;
  if (!v->stats.pack_call) out->n_docs = -1;
  return WP_OK;
}

int wp_pack_sequences(wp_vocab *v, const int32_t *ids, const int64_t *row_splits, size_t n_docs, const wp_pack_spec *spec,
                      wp_packed *out, size_t *n_out) {
  return guarded([&] {
    if (!out || !n_out) throw std::invalid_argument("pack: an out-pointer is NULL");
    *out = wp_packed{};
    *n_out = 0;
    const PackGeom g = check_pack_spec(spec, n_docs);
    if (!row_splits) throw std::invalid_argument("pack: row_splits is NULL");
    const size_t n_ids = static_cast<size_t>(check_row_splits("pack", row_splits, n_docs));
    const unsigned long long s = static_cast<unsigned long long>(g.max_len - g.budget), B = static_cast<unsigned long long>(g.budget);
    unsigned long long n_cells = 0, n_pieces = 0, n_empty = 0;
    for (size_t r = 0; r < n_docs; r++) {
      const unsigned long long l = static_cast<unsigned long long>(row_splits[r + 1] - row_splits[r]);
      if (l == 0) {
        n_empty++;
        continue;
      }
      const unsigned long long np = g.split ? (l - 1) / B + 1 : 1ull;
      n_pieces += np;
      n_cells += (g.stream || g.split ? l : std::min(l, B)) + np * s;  // (l < 2^63, np * s <= 2 l: no wrap before the check of n_ids)
      if (n_cells > (1ull << 62)) n_cells = 1ull << 62;
    }
    check_pack_totals(n_ids, n_cells);
    if (g.stream) check_pack_rows((n_cells + g.max_len - 1) / static_cast<unsigned long long>(g.max_len), g.max_len);
    if (n_ids > 0 && !ids) throw std::invalid_argument("pack: ids is NULL");
    if (n_pieces == 0) {  // no document, or empty ones only: no device
      begin_pack_stats(v, n_docs).n_empty = static_cast<int64_t>(n_empty);
      return;
    }
    Context *c = get_context(v);
    const StagedRows in = stage_ids_and_rows(c->pack_in, c->stream, ids, n_ids, row_splits, (n_docs + 1) * sizeof(int64_t), n_docs);
    PackOut o{};
    const size_t rows = pack_on_device(v, c, in.d_ids, in.d_rows, n_docs, g, [&](size_t n) { return o = pack_batch(c, n, g.max_len); });
    if (rows == 0) return;
    const size_t cells = rows * static_cast<size_t>(g.max_len) * sizeof(int32_t);
    Downloads down(c->stream);
    down.add(&out->input_ids, o.input_ids, cells);
    if (g.want & WP_PACK_WANT_SEGMENTS) down.add(&out->segment_ids, o.segment_ids, cells);
    if (g.want & WP_PACK_WANT_POSITIONS) down.add(&out->position_ids, o.position_ids, cells);
    if (g.want & WP_PACK_WANT_SOURCE) down.add(&out->source, o.source, cells);
    down.add(&out->lengths, o.lengths, rows * sizeof(int32_t));
    down.finish();
    *n_out = rows;
  });
}

int wp_pack_sequences_device(wp_vocab *v, const int32_t *d_ids, const int64_t *d_row_splits, size_t n_docs, const wp_pack_spec *spec,
                             const wp_packed *d_out, size_t capacity_rows, size_t *n_out) {
  return guarded([&] {
    if (!n_out) throw std::invalid_argument("pack: an out-pointer is NULL");
    *n_out = 0;
    const PackGeom g = check_pack_spec(spec, n_docs);
    if (!d_row_splits) throw std::invalid_argument("pack: row_splits is NULL");
    if (!d_out) throw std::invalid_argument("pack: an out-pointer is NULL");
    // (buffers of no rows may be NULL: any row at all then fails the capacity rule, with the count)
    if (capacity_rows > 0 && (!d_out->input_ids || !d_out->lengths || ((g.want & WP_PACK_WANT_SEGMENTS) && !d_out->segment_ids) ||
                              ((g.want & WP_PACK_WANT_POSITIONS) && !d_out->position_ids) || ((g.want & WP_PACK_WANT_SOURCE) && !d_out->source))) {
      throw std::invalid_argument("pack: an output buffer is NULL");
    }
    PackOut o{d_out->input_ids, (g.want & WP_PACK_WANT_SEGMENTS) ? d_out->segment_ids : nullptr,
              (g.want & WP_PACK_WANT_POSITIONS) ? d_out->position_ids : nullptr, (g.want & WP_PACK_WANT_SOURCE) ? d_out->source : nullptr,
              d_out->lengths};
    for (const int32_t *p : {d_ids, static_cast<const int32_t *>(o.input_ids), static_cast<const int32_t *>(o.segment_ids),
                             static_cast<const int32_t *>(o.position_ids), static_cast<const int32_t *>(o.source),
                             static_cast<const int32_t *>(o.lengths)}) {
      check_aligned(p, 4, "pack: device ids and outputs must be 4-byte aligned");
    }
    check_aligned(d_row_splits, 8, "pack: device row_splits must be 8-byte aligned");
    if (n_docs == 0) {
      begin_pack_stats(v, 0);
      return;
    }
    *n_out = pack_on_device(v, get_context(v), d_ids, reinterpret_cast<const long long *>(d_row_splits), n_docs, g, [&](size_t n) {
      if (n > capacity_rows) {
        *n_out = n;
        throw std::invalid_argument("pack: capacity_rows is smaller than the number of output rows");
      }
      return o;
    });
  });
}

}  // extern "C"

// ---- span alignment (include/wordpiece_amd.h, section "span alignment"; host path: align_path.h) ---------------------
// the host entry points behind their argument rules: align_from_host, then the blocks the caller asked for come down
static void align_host_call(wp_vocab *v, const AlignIn &in, const AlignGeom &g, bool ragged, int want, int32_t **labels, int32_t **span_index,
                            int32_t **start, int32_t **end) {
  Context *c = get_context(v);
  const AlignOut o = align_from_host(v, c, in, g, ragged, want);
  const size_t cells = (ragged ? in.n_ids : in.n_rows * static_cast<size_t>(g.max_len)) * sizeof(int32_t);
  Downloads down(c->stream);
  if (want & WP_ALIGN_LABELS) down.add(labels, o.labels, cells);
  if (want & WP_ALIGN_SPAN_INDEX) down.add(span_index, o.span_index, cells);
  if (want & WP_ALIGN_POSITIONS) {
    down.add(start, o.start, in.n_rows * sizeof(int32_t));
    down.add(end, o.end, in.n_rows * sizeof(int32_t));
  }
  down.finish();
}

// the alignment rule of the device entry points
static void check_align_pointers(const AlignIn &in, const AlignOut &out) {
  const char *aligned = "align: device offsets, spans and splits must be 8-byte aligned, everything else 4-byte aligned";
  for (const void *p : {static_cast<const void *>(in.offsets), static_cast<const void *>(in.spans), static_cast<const void *>(in.span_splits),
                        static_cast<const void *>(in.row_splits)}) {
    check_aligned(p, 8, aligned);
  }
  for (const int32_t *p : {in.types, in.lengths, in.sample, in.span_labels, static_cast<const int32_t *>(out.labels),
                           static_cast<const int32_t *>(out.span_index), static_cast<const int32_t *>(out.start),
                           static_cast<const int32_t *>(out.end)}) {
    check_aligned(p, 4, aligned);
  }
}

extern "C" {

int wp_get_align_stats(const wp_vocab *v, wp_align_stats *out) {
  *out = v->stats.align;
  if (!v->stats.align_call) out->n_rows = -1;
  return WP_OK;
}

int wp_align(wp_vocab *v, const uint32_t *offsets, const int32_t *token_type_ids, const int32_t *lengths, const int32_t *sample,
             size_t n_rows, const int64_t *span_splits, size_t n_samples, const uint32_t *spans, const int32_t *span_labels, size_t n_spans,
             const wp_align_spec *spec, int32_t **labels, int32_t **span_index, int32_t **start_positions, int32_t **end_positions) {
  return guarded([&] {
    for (int32_t **p : {labels, span_index, start_positions, end_positions}) {
      if (p) *p = nullptr;
    }
    AlignIn in;
    in.offsets = offsets;
    in.types = token_type_ids;
    in.lengths = lengths;
    in.sample = sample;
    in.span_splits = span_splits;
    in.spans = spans;
    in.span_labels = span_labels;
    in.n_rows = n_rows;
    in.n_samples = n_samples;
    in.n_spans = n_spans;
    const int want = spec ? spec->want : 0;
    const AlignGeom g = check_align_spec(spec, in, false, want, true);
    if (((want & WP_ALIGN_LABELS) && !labels) || ((want & WP_ALIGN_SPAN_INDEX) && !span_index) ||
        ((want & WP_ALIGN_POSITIONS) && (!start_positions || !end_positions))) {
      throw std::invalid_argument("align: the out-pointer of a wanted output is NULL");
    }
    if (n_rows != 0 && !offsets) throw std::invalid_argument("align: offsets is NULL");
    check_align_arrays(in, false);
    if (n_rows == 0) {
      begin_align_stats(v, 0, n_spans);
      return;
    }
    align_host_call(v, in, g, false, want, labels, span_index, start_positions, end_positions);
  });
}

int wp_align_device(wp_vocab *v, const uint32_t *d_offsets, const int32_t *d_token_type_ids, const int32_t *d_lengths, const int32_t *d_sample,
                    size_t n_rows, const int64_t *d_span_splits, size_t n_samples, const uint32_t *d_spans, const int32_t *d_span_labels,
                    size_t n_spans, const wp_align_spec *spec, int32_t *d_labels, int32_t *d_span_index, int32_t *d_start_positions,
                    int32_t *d_end_positions) {
  return guarded([&] {
    AlignIn in;
    in.offsets = d_offsets;
    in.types = d_token_type_ids;
    in.lengths = d_lengths;
    in.sample = d_sample;
    in.span_splits = d_span_splits;
    in.spans = d_spans;
    in.span_labels = d_span_labels;
    in.n_rows = n_rows;
    in.n_samples = n_samples;
    in.n_spans = n_spans;
    const AlignOut out{d_labels, d_span_index, d_start_positions, d_end_positions};
    if ((d_start_positions == nullptr) != (d_end_positions == nullptr)) {
      throw std::invalid_argument("align: start_positions and end_positions go together");
    }
    const int want = (d_labels ? WP_ALIGN_LABELS : 0) | (d_span_index ? WP_ALIGN_SPAN_INDEX : 0) | (d_start_positions ? WP_ALIGN_POSITIONS : 0);
    const AlignGeom g = check_align_spec(spec, in, false, want, false);
    if (n_rows != 0 && !d_offsets) throw std::invalid_argument("align: offsets is NULL");
    check_align_pointers(in, out);
    align_on_device(v, get_context(v), in, g, false, out, true);
  });
}

int wp_align_rows(wp_vocab *v, const uint32_t *offsets, const int64_t *row_splits, size_t n_rows, const int64_t *span_splits,
                  const uint32_t *spans, const int32_t *span_labels, size_t n_spans, const wp_align_spec *spec, int32_t **labels,
                  int32_t **span_index) {
  return guarded([&] {
    for (int32_t **p : {labels, span_index}) {
      if (p) *p = nullptr;
    }
    AlignIn in;
    in.offsets = offsets;
    in.row_splits = row_splits;
    in.span_splits = span_splits;
    in.spans = spans;
    in.span_labels = span_labels;
    in.n_rows = n_rows;
    in.n_samples = n_rows;
    in.n_spans = n_spans;
    if (!row_splits) throw std::invalid_argument("align: row_splits is NULL");
    if (n_rows > static_cast<size_t>(INT32_MAX)) throw std::length_error("align: more rows than INT32_MAX");
    // (the last entry is taken on trust only as far as the size rule; check_align_arrays holds it against the others)
    if (row_splits[n_rows] < 0) throw_align_bad(align_bad_key(kAlignBadRowSplits, n_rows));
    in.n_ids = static_cast<size_t>(row_splits[n_rows]);
    const int want = spec ? spec->want : 0;
    const AlignGeom g = check_align_spec(spec, in, true, want, true);
    if (((want & WP_ALIGN_LABELS) && !labels) || ((want & WP_ALIGN_SPAN_INDEX) && !span_index)) {
      throw std::invalid_argument("align: the out-pointer of a wanted output is NULL");
    }
    if (in.n_ids != 0 && !offsets) throw std::invalid_argument("align: offsets is NULL");
    check_align_arrays(in, true);
    if (in.n_ids == 0) {
      begin_align_stats(v, n_rows, n_spans);
      return;
    }
    align_host_call(v, in, g, true, want, labels, span_index, nullptr, nullptr);
  });
}

int wp_align_rows_device(wp_vocab *v, const uint32_t *d_offsets, const int64_t *d_row_splits, size_t n_rows, size_t n_ids,
                         const int64_t *d_span_splits, const uint32_t *d_spans, const int32_t *d_span_labels, size_t n_spans,
                         const wp_align_spec *spec, int32_t *d_labels, int32_t *d_span_index) {
  return guarded([&] {
    AlignIn in;
    in.offsets = d_offsets;
    in.row_splits = d_row_splits;
    in.span_splits = d_span_splits;
    in.spans = d_spans;
    in.span_labels = d_span_labels;
    in.n_rows = n_rows;
    in.n_samples = n_rows;
    in.n_spans = n_spans;
    in.n_ids = n_ids;
    const AlignOut out{d_labels, d_span_index, nullptr, nullptr};
    const int want = (d_labels ? WP_ALIGN_LABELS : 0) | (d_span_index ? WP_ALIGN_SPAN_INDEX : 0);
    if (!d_row_splits) throw std::invalid_argument("align: row_splits is NULL");
    const AlignGeom g = check_align_spec(spec, in, true, want, false);
    if (n_ids != 0 && !d_offsets) throw std::invalid_argument("align: offsets is NULL");
    check_align_pointers(in, out);
    align_on_device(v, get_context(v), in, g, true, out, true);
  });
}

}  // extern "C"

// ---- word counts (include/wordpiece_amd.h, section "word counts"; host path: count_path.h) ----------------------------
extern "C" {

int wp_get_count_stats(const wp_vocab *v, wp_count_stats *out) {
  *out = v->stats.count;
  if (!v->stats.count_call) out->n_words = -1;
  return WP_OK;
}

int wp_count_words(wp_vocab *v, const char *utf8, size_t nbytes, const wp_count_spec *spec, wp_word_counts *out) {
  return guarded([&] {
    if (out) *out = wp_word_counts{};
    const CountPlan plan = check_count_spec(spec, out);
    if (nbytes > static_cast<size_t>(UINT32_MAX)) throw std::length_error("count: nbytes above UINT32_MAX");
    if (nbytes == 0) {
      *out = count_of_nothing(v);
      return;
    }
    if (!utf8) throw std::invalid_argument("count: utf8 is NULL");
    Context *c = get_context(v);
    upload_text(c, utf8, nbytes);
    wp_word_counts d;
    count_on_device(v, c, static_cast<const uint8_t *>(c->text_buf.p), nbytes, plan, &d);
    wp_word_counts h = d;
    h.words = nullptr;
    h.word_off = h.counts = nullptr;
    h.word_index = nullptr;
    Downloads down(c->stream);
    if (d.n_bytes) down.add(&h.words, d.words, static_cast<size_t>(d.n_bytes));
    down.add(&h.word_off, d.word_off, static_cast<size_t>(d.n_distinct + 1) * sizeof(int64_t));
    if (d.n_distinct) down.add(&h.counts, d.counts, static_cast<size_t>(d.n_distinct) * sizeof(int64_t));
    if (d.word_index) down.add(&h.word_index, d.word_index, static_cast<size_t>(d.n_words) * sizeof(int32_t));
    down.finish();
    *out = h;
  });
}

int wp_count_words_device(wp_vocab *v, const void *d_utf8, size_t nbytes, const wp_count_spec *spec, wp_word_counts *d_out) {
  return guarded([&] {
    if (d_out) *d_out = wp_word_counts{};
    const CountPlan plan = check_count_spec(spec, d_out);
    if (nbytes > static_cast<size_t>(UINT32_MAX)) throw std::length_error("count: nbytes above UINT32_MAX");
    if (nbytes != 0) {
      if (!d_utf8) throw std::invalid_argument("count: utf8 is NULL");
      check_device_text(d_utf8);
    }
    count_on_device(v, get_context(v), static_cast<const uint8_t *>(d_utf8), nbytes, plan, d_out);
  });
}

}  // extern "C"

// ---- vocabulary learner (include/wordpiece_amd.h, section "vocabulary learner"; host path: learn_path.h) -------------
extern "C" {

int wp_get_learn_stats(const wp_vocab *v, wp_learn_stats *out) {
  *out = v->stats.learn;
  if (!v->stats.learn_call) out->n_words = -1;
  return WP_OK;
}

int wp_learn_vocab(wp_vocab *v, const uint8_t *words, const int64_t *word_off, const int64_t *counts, size_t n_words, const wp_learn_spec *spec,
                   wp_learned_vocab *out) {
  return guarded([&] {
    if (out) *out = wp_learned_vocab{};
    const LearnPlan plan = check_learn_spec(spec, out);
    if (n_words != 0 && !word_off) throw std::invalid_argument("learn: word_off is NULL");
    if (n_words != 0 && !counts) throw std::invalid_argument("learn: counts is NULL");
    const int64_t n_bytes = n_words ? word_off[n_words] : 0;
    if (n_bytes < 0) throw std::invalid_argument("learn: word_off ends below 0");
    check_learn_sizes(static_cast<size_t>(n_bytes), n_words);
    if (n_bytes != 0 && !words) throw std::invalid_argument("learn: words is NULL");
    if (n_words == 0) {
      *out = learn_reserved_only(v, plan);
      return;
    }
    Context *c = get_context(v);
    Arena in(&c->learn_in);
    uint8_t *d_pool = nullptr;
    long long *d_off = nullptr, *d_cnt = nullptr;
    for (int pass = 0; pass < 2; pass++) {
      d_pool = in.take<uint8_t>(static_cast<size_t>(n_bytes) + 8);
      d_off = in.take<long long>(n_words + 1);
      d_cnt = in.take<long long>(n_words);
      if (pass == 0) in.commit();
    }
    if (n_bytes) WP_HIP(hipMemcpyAsync(d_pool, words, static_cast<size_t>(n_bytes), hipMemcpyHostToDevice, c->stream));
    WP_HIP(hipMemcpyAsync(d_off, word_off, (n_words + 1) * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    WP_HIP(hipMemcpyAsync(d_cnt, counts, n_words * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    wp_learned_vocab d;
    learn_on_device(v, c, LearnIn{d_pool, static_cast<size_t>(n_bytes), d_off, d_cnt, n_words}, plan, &d);
    wp_learned_vocab h = d;
    h.tokens = nullptr;
    h.token_off = h.scores = nullptr;
    Downloads down(c->stream);
    if (d.n_bytes) down.add(&h.tokens, d.tokens, static_cast<size_t>(d.n_bytes));
    down.add(&h.token_off, d.token_off, static_cast<size_t>(d.n_tokens + 1) * sizeof(int64_t));
    if (d.n_tokens) down.add(&h.scores, d.scores, static_cast<size_t>(d.n_tokens) * sizeof(int64_t));
    down.finish();
    *out = h;
  });
}

int wp_learn_vocab_device(wp_vocab *v, const void *d_words, size_t n_bytes, const int64_t *d_word_off, const int64_t *d_counts, size_t n_words,
                          const wp_learn_spec *spec, wp_learned_vocab *d_out) {
  return guarded([&] {
    if (d_out) *d_out = wp_learned_vocab{};
    const LearnPlan plan = check_learn_spec(spec, d_out);
    check_learn_sizes(n_bytes, n_words);
    if (n_words != 0 && !d_word_off) throw std::invalid_argument("learn: word_off is NULL");
    if (n_words != 0 && !d_counts) throw std::invalid_argument("learn: counts is NULL");
    if (n_bytes != 0 && !d_words) throw std::invalid_argument("learn: words is NULL");
    check_aligned(d_word_off, 8, "learn: word_off must be 8-byte aligned");
    check_aligned(d_counts, 8, "learn: counts must be 8-byte aligned");
    const LearnIn t{static_cast<const uint8_t *>(d_words), n_bytes, reinterpret_cast<const long long *>(d_word_off),
                    reinterpret_cast<const long long *>(d_counts), n_words};
    learn_on_device(v, get_context(v), t, plan, d_out);
  });
}

}  // extern "C"

// ---- duplicate rows (include/wordpiece_amd.h, section "duplicate rows"; host path: dedup_path.h) ----------------------
extern "C" {

int wp_get_dedup_stats(const wp_vocab *v, wp_dedup_stats *out) {
  *out = v->stats.dedup;
  if (!v->stats.dedup_call) out->n_rows = -1;
  return WP_OK;
}

int wp_dedup_rows(wp_vocab *v, const void *data, const int64_t *row_off, size_t n_rows, const wp_dedup_spec *spec, wp_dedup_result *out) {
  return guarded([&] {
    if (out) *out = wp_dedup_result{};
    const DedupPlan plan = check_dedup_spec(spec, out);
    if (n_rows != 0 && !row_off) throw std::invalid_argument("dedup: row_off is NULL");
    check_row_count("dedup", n_rows);
    const unsigned long long n_elems = check_ragged_host("dedup", data, row_off, n_rows, plan.elem_bytes);
    if (n_elems == 0) {
      *out = dedup_all_empty(v, n_rows, plan);
      return;
    }
    Context *c = get_context(v);
    const RaggedIn in = upload_ragged(c->dedup_in, c->stream, data, row_off, n_rows, static_cast<size_t>(n_elems) * plan.elem_bytes, plan.elem_bytes);
    wp_dedup_result d;
    dedup_on_device(v, c, in, plan, &d);
    wp_dedup_result h = d;
    Downloads down(c->stream);
    down.swap(&h.first, n_rows * sizeof(int32_t));
    swap_table(down, h, plan.elem_bytes);
    down.finish();
    *out = h;
  });
}

int wp_dedup_rows_device(wp_vocab *v, const void *d_data, const int64_t *d_row_off, size_t n_rows, const wp_dedup_spec *spec,
                         wp_dedup_result *d_out) {
  return guarded([&] {
    if (d_out) *d_out = wp_dedup_result{};
    const DedupPlan plan = check_dedup_spec(spec, d_out);
    if (n_rows != 0 && !d_row_off) throw std::invalid_argument("dedup: row_off is NULL");
    check_row_count("dedup", n_rows);
    const RaggedIn in = device_batch("dedup", d_data, d_row_off, n_rows, plan.elem_bytes);
    if (n_rows == 0) {  // (nothing to read and nothing to hand out: every pointer of the result stays NULL)
      begin_dedup_stats(v, 0);
      return;
    }
    dedup_on_device(v, get_context(v), in, plan, d_out);
  });
}

}  // extern "C"

// ---- near-duplicate rows (include/wordpiece_amd.h, section "near-duplicate rows"; host path: neardup_path.h) -----------
extern "C" {

int wp_get_neardup_stats(const wp_vocab *v, wp_neardup_stats *out) {
  *out = v->stats.neardup;
  if (!v->stats.neardup_call) out->n_rows = -1;
  return WP_OK;
}

int wp_neardup_rows(wp_vocab *v, const void *data, const int64_t *row_off, size_t n_rows, const wp_neardup_spec *spec, wp_neardup_result *out) {
  return guarded([&] {
    if (out) *out = wp_neardup_result{};
    const NearDupPlan plan = check_neardup_spec(spec, out);
    if (n_rows != 0 && !row_off) throw std::invalid_argument("neardup: row_off is NULL");
    check_neardup_rows(n_rows, plan);
    const unsigned long long n_elems = check_ragged_host("neardup", data, row_off, n_rows, plan.elem_bytes);
    if (n_elems == 0) {
      *out = neardup_all_empty(v, n_rows, plan);
      return;
    }
    Context *c = get_context(v);
    const RaggedIn in = upload_ragged(c->neardup_in, c->stream, data, row_off, n_rows, static_cast<size_t>(n_elems) * plan.elem_bytes, plan.elem_bytes);
    wp_neardup_result d;
    neardup_on_device(v, c, in, plan, &d);
    wp_neardup_result h = d;
    Downloads down(c->stream);
    down.swap(&h.cluster, n_rows * sizeof(int32_t));
    swap_table(down, h, plan.elem_bytes);
    down.swap(&h.signatures, n_rows * plan.n_perm * sizeof(uint32_t));
    down.finish();
    *out = h;
  });
}

int wp_neardup_rows_device(wp_vocab *v, const void *d_data, const int64_t *d_row_off, size_t n_rows, const wp_neardup_spec *spec,
                           wp_neardup_result *d_out) {
  return guarded([&] {
    if (d_out) *d_out = wp_neardup_result{};
    const NearDupPlan plan = check_neardup_spec(spec, d_out);
    if (n_rows != 0 && !d_row_off) throw std::invalid_argument("neardup: row_off is NULL");
    check_neardup_rows(n_rows, plan);
    const RaggedIn in = device_batch("neardup", d_data, d_row_off, n_rows, plan.elem_bytes);
    if (n_rows == 0) {  // (nothing to read and nothing to hand out: every pointer of the result stays NULL)
      begin_neardup_stats(v, 0);
      return;
    }
    neardup_on_device(v, get_context(v), in, plan, d_out);
  });
}

}  // extern "C"

// ---- n-gram overlap (include/wordpiece_amd.h, section "n-gram overlap"; host path: overlap_path.h) ---------------------
extern "C" {

int wp_get_overlap_stats(const wp_vocab *v, wp_overlap_stats *out) {
  *out = v->stats.overlap;
  if (!v->stats.overlap_call) out->n_rows = -1;
  return WP_OK;
}

int wp_overlap_rows(wp_vocab *v, const void *data, const int64_t *row_off, size_t n_rows, const void *ref_data, const int64_t *ref_off, size_t n_ref,
                    const wp_overlap_spec *spec, wp_overlap_result *out) {
  return guarded([&] {
    if (out) *out = wp_overlap_result{};
    const OverlapPlan plan = check_overlap_spec(spec, out);
    check_overlap_rows(row_off, n_rows, ref_off, n_ref);
    const unsigned long long n_elems = check_ragged_host("overlap", data, row_off, n_rows, plan.elem_bytes);
    const unsigned long long n_ref_elems = check_ragged_host("overlap", ref_data, ref_off, n_ref, plan.elem_bytes, "ref_off", "ref_data");
    if (n_rows == 0) {  // (nothing to hand out: every pointer of the result stays NULL)
      begin_overlap_stats(v, 0, n_ref);
      out->n_ref = static_cast<int64_t>(n_ref);
      return;
    }
    const unsigned long long n_windows = host_windows(row_off, n_rows, plan.ngram), n_ref_windows = host_windows(ref_off, n_ref, plan.ngram);
    if (n_windows == 0 || n_ref_windows == 0) {
      *out = overlap_no_window(v, plan, data, row_off, n_rows, ref_data, ref_off, n_ref, n_windows, n_ref_windows);
      return;
    }
    Context *c = get_context(v);
    const uint32_t eb = plan.elem_bytes;
    const RaggedIn in = upload_ragged(c->overlap_in, c->stream, data, row_off, n_rows, static_cast<size_t>(n_elems) * eb, eb);
    const RaggedIn ref = upload_ragged(c->overlap_ref_in, c->stream, ref_data, ref_off, n_ref, static_cast<size_t>(n_ref_elems) * eb, eb);
    wp_overlap_result d;
    overlap_on_device(v, c, in, ref, plan, &d);
    wp_overlap_result h = d;
    Downloads down(c->stream);
    down.swap(&h.hits, n_rows * sizeof(int64_t));
    down.swap(&h.first_hit, n_rows * sizeof(int64_t));
    down.swap(&h.covered, n_rows * sizeof(int64_t));
    down.swap(&h.first_ref, n_rows * sizeof(int32_t));
    down.swap(&h.mask, static_cast<size_t>(n_elems));
    down.swap(&h.ref_hits, n_ref * sizeof(int64_t));
    swap_compact(down, h, h.n_kept, eb);
    down.finish();
    *out = h;
  });
}

int wp_overlap_rows_device(wp_vocab *v, const void *d_data, const int64_t *d_row_off, size_t n_rows, const void *d_ref_data, const int64_t *d_ref_off,
                           size_t n_ref, const wp_overlap_spec *spec, wp_overlap_result *d_out) {
  return guarded([&] {
    if (d_out) *d_out = wp_overlap_result{};
    const OverlapPlan plan = check_overlap_spec(spec, d_out);
    check_overlap_rows(d_row_off, n_rows, d_ref_off, n_ref);
    const RaggedIn in = device_batch("overlap", d_data, d_row_off, n_rows, plan.elem_bytes);
    const RaggedIn ref = device_batch("overlap", d_ref_data, d_ref_off, n_ref, plan.elem_bytes, "ref_off", "ref_data");
    if (n_rows == 0) {  // (nothing to read and nothing to hand out: every pointer of the result stays NULL)
      begin_overlap_stats(v, 0, n_ref);
      d_out->n_ref = static_cast<int64_t>(n_ref);
      return;
    }
    overlap_on_device(v, get_context(v), in, ref, plan, d_out);
  });
}

}  // extern "C"

// ---- repeated spans (include/wordpiece_amd.h, section "repeated spans"; host path: repeat_path.h) ----------------------
extern "C" {

int wp_get_repeat_stats(const wp_vocab *v, wp_repeat_stats *out) {
  *out = v->stats.repeat;
  if (!v->stats.repeat_call) out->n_rows = -1;
  return WP_OK;
}

int wp_repeat_rows(wp_vocab *v, const void *data, const int64_t *row_off, size_t n_rows, const wp_repeat_spec *spec, wp_repeat_result *out) {
  return guarded([&] {
    if (out) *out = wp_repeat_result{};
    const RepeatPlan plan = check_repeat_spec(spec, out);
    check_repeat_rows(row_off, n_rows);
    const unsigned long long n_elems = check_ragged_host("repeat", data, row_off, n_rows, plan.elem_bytes);
    if (n_rows == 0) {  // (nothing to hand out: every pointer of the result stays NULL)
      begin_repeat_stats(v, 0);
      return;
    }
    if (host_windows(row_off, n_rows, plan.ngram) == 0) {
      *out = repeat_no_window(v, plan, data, row_off, n_rows);
      return;
    }
    Context *c = get_context(v);
    const uint32_t eb = plan.elem_bytes;
    const RaggedIn in = upload_ragged(c->repeat_in, c->stream, data, row_off, n_rows, static_cast<size_t>(n_elems) * eb, eb);
    wp_repeat_result d;
    repeat_on_device(v, c, in, plan, &d);
    wp_repeat_result h = d;
    Downloads down(c->stream);
    down.swap(&h.repeats, n_rows * sizeof(int64_t));
    down.swap(&h.first_repeat, n_rows * sizeof(int64_t));
    down.swap(&h.first_src_pos, n_rows * sizeof(int64_t));
    down.swap(&h.covered, n_rows * sizeof(int64_t));
    down.swap(&h.first_src_row, n_rows * sizeof(int32_t));
    down.swap(&h.mask, static_cast<size_t>(n_elems));
    down.swap(&h.src, static_cast<size_t>(n_elems) * sizeof(int64_t));
    swap_compact(down, h, h.n_kept, eb);
    down.swap(&h.cut_off, (n_rows + 1) * sizeof(int64_t));
    down.swap(&h.cut_data, static_cast<size_t>(h.n_cut_elems) * eb);
    down.finish();
    *out = h;
  });
}

int wp_repeat_rows_device(wp_vocab *v, const void *d_data, const int64_t *d_row_off, size_t n_rows, const wp_repeat_spec *spec, wp_repeat_result *d_out) {
  return guarded([&] {
    if (d_out) *d_out = wp_repeat_result{};
    const RepeatPlan plan = check_repeat_spec(spec, d_out);
    check_repeat_rows(d_row_off, n_rows);
    const RaggedIn in = device_batch("repeat", d_data, d_row_off, n_rows, plan.elem_bytes);
    if (n_rows == 0) {  // (nothing to read and nothing to hand out: every pointer of the result stays NULL)
      begin_repeat_stats(v, 0);
      return;
    }
    repeat_on_device(v, get_context(v), in, plan, d_out);
  });
}

}  // extern "C"

// ---- quality signals (include/wordpiece_amd.h, section "quality signals"; host path: quality_path.h) -------------------
extern "C" {

int wp_get_quality_stats(const wp_vocab *v, wp_quality_stats *out) {
  *out = v->stats.quality;
  if (!v->stats.quality_call) out->n_rows = -1;
  return WP_OK;
}

int32_t wp_quality_class(uint32_t cp) {
  if (cp >= 0x110000u || (cp >= 0xd800u && cp < 0xe000u)) return -1;
  return quality_class_bits(cp, kClassIndex, kClassPageData) >> 3;
}

int wp_quality_rows(wp_vocab *v, const void *data, const int64_t *row_off, size_t n_rows, const wp_quality_spec *spec, wp_quality_result *out) {
  return guarded([&] {
    if (out) *out = wp_quality_result{};
    const QualityPlan plan = check_quality_spec(spec, out);
    check_quality_rows(row_off, n_rows);
    const unsigned long long n_bytes = check_ragged_host("quality", data, row_off, n_rows, 1);
    if (n_rows == 0) {  // (nothing to hand out: every pointer of the result stays NULL)
      begin_quality_stats(v, 0);
      return;
    }
    if (n_bytes == 0) {
      *out = quality_no_bytes(v, plan, n_rows);
      return;
    }
    Context *c = get_context(v);
    const RaggedIn in = upload_ragged(c->quality_in, c->stream, data, row_off, n_rows, static_cast<size_t>(n_bytes), 1);
    wp_quality_result d;
    quality_on_device(v, c, in, plan, &d);
    wp_quality_result h = d;
    Downloads down(c->stream);
    down.swap(&h.signals, n_rows * WP_QUALITY_SIGNALS * sizeof(int64_t));
    down.swap(&h.reasons, n_rows * sizeof(uint32_t));
    swap_compact(down, h, h.n_kept, 1);
    down.finish();
    *out = h;
  });
}

int wp_quality_rows_device(wp_vocab *v, const void *d_data, const int64_t *d_row_off, size_t n_rows, const wp_quality_spec *spec, wp_quality_result *d_out) {
  return guarded([&] {
    if (d_out) *d_out = wp_quality_result{};
    const QualityPlan plan = check_quality_spec(spec, d_out);
    check_quality_rows(d_row_off, n_rows);
    const RaggedIn in = device_batch("quality", d_data, d_row_off, n_rows, 1);
    if (n_rows == 0) {  // (nothing to read and nothing to hand out: every pointer of the result stays NULL)
      begin_quality_stats(v, 0);
      return;
    }
    quality_on_device(v, get_context(v), in, plan, d_out);
  });
}

}  // extern "C"

// ---- special tokens (include/wordpiece_amd.h, section "special tokens"; host path: special_path.h) -------------------
extern "C" {

int wp_get_special_stats(const wp_vocab *v, wp_special_stats *out) {
  *out = v->stats.special;
  if (!v->stats.special_call) out->n_literals = -1;
  return WP_OK;
}

int wp_linear_encode_special(wp_vocab *v, const char *utf8, size_t nbytes, const wp_special_spec *spec, int unit, int32_t **ids,
                             uint32_t **offsets, size_t *n_ids) {
  return guarded([&] {
    *ids = nullptr;
    if (offsets) *offsets = nullptr;
    *n_ids = 0;
    check_special_call(unit, nbytes);
    if (unit >= 0 && !offsets) throw std::invalid_argument("offsets asked for without a place to return them");
    const SpecialList list = check_special_spec(v, spec);
    if (nbytes == 0) {  // (no device needed, as wp_linear_encode_offsets)
      set_special_stats(v, list, 0, 0, false, 0);
      return;
    }
    const auto t_all = wp_clock::now();
    Context *c = get_context(v);
    upload_text(c, utf8, nbytes);
    RowsResult r;
    special_on_device(v, c, static_cast<const uint8_t *>(c->text_buf.p), nbytes, false, nullptr, 0, unit, SIZE_MAX, list, r);
    const auto t0 = wp_clock::now();
    if (r.n_ids) {
      Downloads down(c->stream);
      down.add(ids, r.d_ids, r.n_ids * sizeof(int32_t));
      if (unit >= 0) down.add(offsets, r.d_offs, r.n_ids * 2 * sizeof(uint32_t));
      down.finish();
      *n_ids = r.n_ids;
    }
    v->stats.ms_d2h = ms_since(t0);
    v->stats.ms_host_total = ms_since(t_all);
  });
}

int wp_linear_encode_special_device(wp_vocab *v, const void *d_utf8, size_t nbytes, const wp_special_spec *spec, int unit,
                                    const int32_t **d_ids, const uint32_t **d_offsets, size_t *n_ids) {
  return guarded([&] {
    *d_ids = nullptr;
    if (d_offsets) *d_offsets = nullptr;
    *n_ids = 0;
    check_special_call(unit, nbytes);
    if (unit >= 0 && !d_offsets) throw std::invalid_argument("offsets asked for without a place to return them");
    const SpecialList list = check_special_spec(v, spec);
    if (nbytes == 0) {
      set_special_stats(v, list, 0, 0, false, 0);
      return;
    }
    check_device_text(d_utf8);
    RowsResult r;
    special_on_device(v, get_context(v), static_cast<const uint8_t *>(d_utf8), nbytes, false, nullptr, 0, unit, SIZE_MAX, list, r);
    *d_ids = r.d_ids;
    if (d_offsets) *d_offsets = r.d_offs;
    *n_ids = r.n_ids;
  });
}

int wp_linear_encode_special_rows(wp_vocab *v, const char *utf8, size_t nbytes, const int64_t *doc_off, size_t n_docs,
                                  const wp_special_spec *spec, int unit, int32_t **ids, int64_t **row_splits, uint32_t **offsets,
                                  size_t *n_ids, size_t *n_rows) {
  return guarded([&] {
    *ids = nullptr;
    *row_splits = nullptr;
    if (offsets) *offsets = nullptr;
    *n_ids = 0;
    *n_rows = 0;
    check_special_call(unit, nbytes);
    if (unit >= 0 && !offsets) throw std::invalid_argument("offsets asked for without a place to return them");
    if (doc_off) check_doc_off_host(utf8, nbytes, doc_off, n_docs);
    const SpecialList list = check_special_spec(v, spec);
    if (nbytes == 0 || (doc_off && nbytes == n_docs)) {  // no text, or empty documents only: no device needed
      const size_t rows = doc_off ? n_docs : 0;
      *row_splits = static_cast<int64_t *>(zeroed((rows + 1) * sizeof(int64_t)));
      *n_rows = rows;
      set_special_stats(v, list, 0, 0, true, rows);
      return;
    }
    const auto t_all = wp_clock::now();
    Context *c = get_context(v);
    upload_text(c, utf8, nbytes);
    if (doc_off) {
      c->rows_in.ensure((n_docs + 1) * sizeof(int64_t));
      WP_HIP(hipMemcpyAsync(c->rows_in.p, doc_off, (n_docs + 1) * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    }
    RowsResult r;
    special_rows_on_device(v, c, static_cast<const uint8_t *>(c->text_buf.p), nbytes,
                           doc_off ? static_cast<const long long *>(c->rows_in.p) : nullptr, n_docs, unit, SIZE_MAX, list, r);
    const auto t0 = wp_clock::now();
    Downloads down(c->stream);
    down.add(row_splits, r.d_row_splits, (r.n_rows + 1) * sizeof(int64_t));
    if (r.n_ids) down.add(ids, r.d_ids, r.n_ids * sizeof(int32_t));
    if (r.n_ids && unit >= 0) down.add(offsets, r.d_offs, r.n_ids * 2 * sizeof(uint32_t));
    down.finish();
    *n_ids = r.n_ids;
    *n_rows = r.n_rows;
    v->stats.ms_d2h = ms_since(t0);
    v->stats.ms_host_total = ms_since(t_all);
  });
}

int wp_linear_encode_special_rows_device(wp_vocab *v, const void *d_utf8, size_t nbytes, const int64_t *d_doc_off, size_t n_docs,
                                         const wp_special_spec *spec, int unit, const int32_t **d_ids, const int64_t **d_row_splits,
                                         const uint32_t **d_offsets, size_t *n_ids, size_t *n_rows) {
  return guarded([&] {
    *d_ids = nullptr;
    *d_row_splits = nullptr;
    if (d_offsets) *d_offsets = nullptr;
    *n_ids = 0;
    *n_rows = 0;
    check_special_call(unit, nbytes);
    if (unit >= 0 && !d_offsets) throw std::invalid_argument("offsets asked for without a place to return them");
    const SpecialList list = check_special_spec(v, spec);
    check_device_text(d_utf8);
    check_device_doc_off(d_doc_off);
    Context *c = get_context(v);
    if (nbytes == 0) {  // no text: no rows (explicit rows cannot end at 0 unless there are none)
      check_doc_off_without_text(d_doc_off, n_docs);
      c->special_out.ensure(sizeof(int64_t));
      WP_HIP(hipMemsetAsync(c->special_out.p, 0, sizeof(int64_t), c->stream));
      WP_HIP(hipStreamSynchronize(c->stream));
      *d_row_splits = static_cast<const int64_t *>(c->special_out.p);
      set_special_stats(v, list, 0, 0, true, 0);
      return;
    }
    RowsResult r;
    special_rows_on_device(v, c, static_cast<const uint8_t *>(d_utf8), nbytes, reinterpret_cast<const long long *>(d_doc_off), n_docs, unit,
                           SIZE_MAX, list, r);
    *d_ids = r.d_ids;
    *d_row_splits = reinterpret_cast<const int64_t *>(r.d_row_splits);
    if (d_offsets) *d_offsets = r.d_offs;
    *n_ids = r.n_ids;
    *n_rows = r.n_rows;
  });
}

}  // extern "C"

// ---- model inputs (include/wordpiece_amd.h, section "model inputs"; host path: inputs_path.h) -------------------------
extern "C" {

int wp_linear_encode_inputs(wp_vocab *v, const char *utf8, size_t nbytes, const int64_t *doc_off, size_t n_docs,
                            const wp_inputs_spec *spec, wp_inputs *out, size_t *n_out, size_t *n_samples) {
  return guarded([&] {
    if (!out || !n_out || !n_samples) throw std::invalid_argument("inputs: null result pointer");
    *out = wp_inputs{};
    *n_out = 0;
    *n_samples = 0;
    const InputsGeom g = check_inputs_spec(spec, nbytes);
    const int unit = spec->unit;
    if (doc_off) check_doc_off_host(utf8, nbytes, doc_off, n_docs);
    const size_t rows = doc_off ? n_docs : count_lines_host(utf8, nbytes);
    check_inputs_rows(g, rows);
    const size_t max_len = static_cast<size_t>(g.max_len);
    if (nbytes == 0 || (doc_off && nbytes == n_docs)) {  // rows of specials and padding only: no device needed
      const size_t n = rows / (g.pairs ? 2 : 1);
      check_inputs_size(n, g.max_len);
      wp_inputs h{};
      h.input_ids = static_cast<int32_t *>(zeroed(n * max_len * sizeof(int32_t)));
      h.token_type_ids = static_cast<int32_t *>(zeroed(n * max_len * sizeof(int32_t)));
      h.lengths = static_cast<int32_t *>(zeroed(n * sizeof(int32_t)));
      h.sample = static_cast<int32_t *>(zeroed(n * sizeof(int32_t)));
      fill_empty_rows(n, g.max_len, g.cls_id, g.sep_id, g.pad_id, g.pairs != 0, h.input_ids, h.lengths, h.token_type_ids, h.sample);
      if (unit >= 0) h.offsets = static_cast<uint32_t *>(zeroed(n * max_len * 2 * sizeof(uint32_t)));
      *out = h;
      *n_out = n;
      *n_samples = n;
      return;
    }
    const auto t_all = wp_clock::now();
    RowsResult r;
    Context *c = rows_from_host(v, utf8, nbytes, doc_off, n_docs, unit, r);
    check_inputs_rows(g, r.n_rows);
    wp_inputs o{};  // the batch in c->pad_buf
    const size_t n = inputs_on_device(v, c, r, g, unit, [&](size_t rows_out) { return o = inputs_batch(c, unit, rows_out, g.max_len); });
    const size_t cells = n * max_len;
    *n_samples = r.n_rows / (g.pairs ? 2 : 1);
    *n_out = n;
    if (n == 0) return;
    Downloads down(c->stream);
    down.add(&out->input_ids, o.input_ids, cells * sizeof(int32_t));
    down.add(&out->token_type_ids, o.token_type_ids, cells * sizeof(int32_t));
    down.add(&out->lengths, o.lengths, n * sizeof(int32_t));
    down.add(&out->sample, o.sample, n * sizeof(int32_t));
    if (unit >= 0) down.add(&out->offsets, o.offsets, cells * 2 * sizeof(uint32_t));
    down.finish();
    v->stats.ms_host_total = ms_since(t_all);
  });
}

int wp_linear_encode_inputs_device(wp_vocab *v, const void *d_utf8, size_t nbytes, const int64_t *d_doc_off, size_t n_docs,
                                   const wp_inputs_spec *spec, const wp_inputs *d_out, size_t capacity_rows, size_t *n_out,
                                   size_t *n_samples) {
  return guarded([&] {
    if (!n_out || !n_samples) throw std::invalid_argument("inputs: null result pointer");
    *n_out = 0;
    *n_samples = 0;
    const InputsGeom g = check_inputs_spec(spec, nbytes);
    const int unit = spec->unit;
    check_device_text(d_utf8);
    check_device_doc_off(d_doc_off);
    if (d_doc_off) check_inputs_rows(g, n_docs);
    if (nbytes == 0) {
      check_doc_off_without_text(d_doc_off, n_docs);
      return;
    }
    if (!d_out || !d_out->input_ids || !d_out->token_type_ids || !d_out->lengths || !d_out->sample || (unit >= 0 && !d_out->offsets)) {
      throw std::invalid_argument("null output buffer");
    }
    check_aligned(d_out->offsets, 8, "the offsets buffer must be 8-byte aligned");
    const size_t mult = g.pairs ? 2 : 1;
    // without windows the rows say how many output rows there are: too little room is found before the encode
    const size_t rows_cap = (g.stride >= 0 || capacity_rows > (SIZE_MAX - 1) / 2) ? SIZE_MAX : capacity_rows * mult + (mult - 1);
    Context *c = get_context(v);
    RowsResult r;
    try {
      rows_on_device(v, c, static_cast<const uint8_t *>(d_utf8), nbytes, reinterpret_cast<const long long *>(d_doc_off), n_docs, unit,
                     rows_cap, r);
    } catch (...) {
      check_inputs_rows(g, r.n_rows);
      *n_out = *n_samples = r.n_rows / mult;  // (too many rows for the caller's buffers: the count it needs)
      throw;
    }
    check_inputs_rows(g, r.n_rows);
    *n_samples = r.n_rows / mult;
    *n_out = inputs_on_device(v, c, r, g, unit, [&](size_t rows_out) {
      if (rows_out > capacity_rows) {
        *n_out = rows_out;
        throw std::invalid_argument("capacity_rows is smaller than the number of output rows");
      }
      return *d_out;
    });
  });
}

int wp_reserve(wp_vocab *v, size_t nbytes) {
  return guarded([&] {
    Context *c = get_context(v);
    // arenas as an encode of `nbytes` of ASCII text would size them in the default layout (39
    // bytes per symbol — no rank table: the ranks of the needed list stand over their keys — + the refinement list for
    // an eighth of the text; an estimate — an encode that needs more, a larger alphabet or the reference layout, grows
    // them as before; the bounds-checking build keeps the rank table)
    const size_t n = nbytes + 1 + v->hv.stream.size();
    const size_t per_symbol = (v->keep_debug || v->vocab_in_s || v->full_depth) ? 108 : (kRankOverKey ? 52 : 56);
    c->text_buf.ensure(text_room(nbytes), false);
    c->a_buf.ensure(nbytes + nbytes / 512 + (size_t(1) << 20) + (v->keep_debug ? 4 * nbytes : 0), false);
    c->b_buf.ensure(per_symbol * n + (v->keep_debug ? 4 * n : 0) + (v->keep_step_views ? 16 * n : 0) + (size_t(64) << 20), false);
    PinnedBlock warm(nbytes + (size_t(1) << 20));  // about a quarter of an id per byte, 4 bytes each
  });
}

// A sequence of shards through one handle as a pipeline: while shard i is on the GPU, shard i + 1 is uploaded (a
// helper thread, its own stream, the second text buffer) and the ids of shard i - 1 are downloaded (their own
// stream, out of a staging buffer — the next encode overwrites the arena the ids were produced in).  For one call
// nothing can overlap the sort; for a corpus that arrives as shards (the reference's own encodeExternal batches,
// linear.cpp:355-371; the per-GPU stream of a sharded run) host to host then costs what the device path costs.
//   next(i, &ptr, &len) -> false: no text i;   deliver(i, block, n): the ids of text i have arrived in `block`
//   (called in order, one text behind the encodes; a block that is not release()d goes back to the pinned pool)
}  // extern "C"

namespace {
template <typename Next, typename Deliver>
void encode_pipeline(wp_vocab *v, Next &&next, Deliver &&deliver) {
  const auto t_all = wp_clock::now();
  Context *c = get_context(v);
  if (!c->up_stream) {
    WP_HIP(hipStreamCreateWithFlags(&c->up_stream, hipStreamNonBlocking));
    WP_HIP(hipStreamCreateWithFlags(&c->down_stream, hipStreamNonBlocking));
    for (auto &e : c->pipe_ev) WP_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  }
  DeviceBuffer *tb[2] = {&c->text_buf, &c->text_buf2};
  const int device = c->device;
  std::atomic<long long> up_us{0};
  // upload of a text into text buffer `slot`, on the upload stream, finished when the call returns
  auto upload = [&](const char *text, size_t len, int slot) -> std::string {
    try {
      if (len == 0) return "";
      const auto t_up = wp_clock::now();
      WP_HIP(hipSetDevice(device));
      upload_text(*tb[slot], c->up_stream, text, len);  // (the buffer has its room already: grown on the calling thread)
      WP_HIP(hipStreamSynchronize(c->up_stream));
      up_us += static_cast<long long>(ms_since(t_up) * 1e3);
      return "";
    } catch (const std::exception &e) {
      return e.what()[0] ? e.what() : "upload failed";
    }
  };
  EncodeStats total{};
  const char *cur_text = nullptr, *next_text = nullptr;
  size_t cur_len = 0, next_len = 0;
  bool have = next(0, &cur_text, &cur_len);
  if (have) {
    tb[0]->ensure(text_room(cur_len));
    const std::string err = upload(cur_text, cur_len, 0);
    if (!err.empty()) throw HipError(err);
  }
  std::unique_ptr<PinnedBlock> in_flight;  // ids of the text before the current one, on their way down
  size_t in_flight_n = 0, in_flight_i = 0;
  int in_flight_slot = 0;
  for (size_t i = 0; have; i++) {
    const int slot = static_cast<int>(i & 1);
    const bool more = next(i + 1, &next_text, &next_len);
    std::future<std::string> next_up;
    if (more) {
      tb[slot ^ 1]->ensure(text_room(next_len));  // (the encode that read this buffer, of text i - 1, is over)
      next_up = std::async(std::launch::async, upload, next_text, next_len, slot ^ 1);
    }
    struct Wait {  // the helper must be done with the text buffers before anything unwinds
      std::future<std::string> &f;
      ~Wait() {
        if (f.valid()) f.wait();
      }
    } wait_up{next_up};
    size_t n = 0;
    EncodeStats st{};
    if (cur_len) encode_on_device(v, c, static_cast<const uint8_t *>(tb[slot]->p), cur_len, &n, st);
    std::unique_ptr<PinnedBlock> blk(new PinnedBlock(std::max<size_t>(n, 1) * sizeof(int32_t)));
    if (n) {
      // (the staging buffer of this slot was last read by the download of text i - 2, which has been delivered)
      c->ids_stage[slot].ensure(n * sizeof(int32_t));
      WP_HIP(hipMemcpyAsync(c->ids_stage[slot].p, c->d_ids, n * sizeof(int32_t), hipMemcpyDeviceToDevice, c->stream));
      WP_HIP(hipEventRecord(c->pipe_ev[slot], c->stream));
      WP_HIP(hipStreamWaitEvent(c->down_stream, c->pipe_ev[slot], 0));
      WP_HIP(hipMemcpyAsync(blk->p, c->ids_stage[slot].p, n * sizeof(int32_t), hipMemcpyDeviceToHost, c->down_stream));
      WP_HIP(hipEventRecord(c->pipe_ev[2 + slot], c->down_stream));
      // (the next encode may overwrite the arena: the copy into the staging buffer is ordered in front of it on c->stream)
    }
    if (in_flight) {  // the text before this one: its download ran beside this encode
      if (in_flight_n) WP_HIP(hipEventSynchronize(c->pipe_ev[2 + in_flight_slot]));
      deliver(in_flight_i, *in_flight, in_flight_n);
    }
    in_flight = std::move(blk);
    in_flight_n = n;
    in_flight_i = i;
    in_flight_slot = slot;
    total.n_bytes += st.n_bytes;
    total.n_text += st.n_text;
    total.n_total += st.n_total;
    total.n_ids += st.n_ids;
    total.ms_total += st.ms_total;
    total.normalize = std::max(total.normalize, st.normalize);
    total.norm_bytes += st.norm_bytes;
    total.ms_normalize += st.ms_normalize;
    total.walk.n_wide_words += st.walk.n_wide_words;
    total.walk.n_long_words += st.walk.n_long_words;
    total.walk.max_anchor_gap = std::max(total.walk.max_anchor_gap, st.walk.max_anchor_gap);
    if (i == 0) total.walk.lean = st.walk.lean;
    {
      const wp_refine_stats sum = total.refine;
      if (i == 0) total.refine = st.refine;  // (the first text's other fields)
      total.refine.n_groups = sum.n_groups + st.refine.n_groups;
      total.refine.n_entries = sum.n_entries + st.refine.n_entries;
      total.refine.n_large_groups = sum.n_large_groups + st.refine.n_large_groups;
      total.refine.n_large_entries = sum.n_large_entries + st.refine.n_large_entries;
    }
    if (i == 0) total.sched = st.sched;  // (the first text's placement)
    if (i == 0) total.step = st.step;
    total.rounds = std::max(total.rounds, st.rounds);
    if (next_up.valid()) {
      const std::string err = next_up.get();
      if (!err.empty()) throw HipError(err);
    }
    have = more;
    cur_text = next_text;
    cur_len = next_len;
  }
  if (in_flight) {
    if (in_flight_n) WP_HIP(hipEventSynchronize(c->pipe_ev[2 + in_flight_slot]));
    deliver(in_flight_i, *in_flight, in_flight_n);
  }
  v->stats = total;
  v->stats.n_devices = 1;
  v->stats.ms_h2d = static_cast<double>(up_us.load()) / 1e3;  // wall time inside the uploads (beside the encodes, all but the first)
  v->stats.ms_host_total = ms_since(t_all);
}
}  // namespace

extern "C" {

int wp_linear_encode_batch(wp_vocab *v, const char *const *texts, const size_t *nbytes, size_t n_texts, int32_t **ids,
                           size_t *n_ids) {
  return guarded([&] {
    for (size_t i = 0; i < n_texts; i++) {
      ids[i] = nullptr;
      n_ids[i] = 0;
    }
    std::vector<void *> got(n_texts, nullptr);  // (handed to the caller only when every text is through)
    try {
      encode_pipeline(
          v,
          [&](size_t i, const char **t, size_t *len) {
            if (i >= n_texts) return false;
            *t = texts[i];
            *len = nbytes[i];
            return true;
          },
          [&](size_t i, PinnedBlock &blk, size_t n) {
            n_ids[i] = n;
            if (n) got[i] = blk.release();
          });
    } catch (...) {
      for (void *p : got) {
        if (p) id_pool().give_back(p);
      }
      for (size_t i = 0; i < n_texts; i++) n_ids[i] = 0;
      throw;
    }
    for (size_t i = 0; i < n_texts; i++) ids[i] = static_cast<int32_t *>(got[i]);
  });
}

int wp_linear_encode_stream(wp_vocab *v, wp_text_source next, wp_ids_sink out, void *user) {
  return guarded([&] {
    if (!next || !out) throw std::invalid_argument("wp_linear_encode_stream: null callback");
    encode_pipeline(
        v, [&](size_t i, const char **t, size_t *len) { return next(user, i, t, len) != 0; },
        [&](size_t i, PinnedBlock &blk, size_t n) { out(user, i, n ? static_cast<const int32_t *>(blk.p) : nullptr, n); });
  });
}

// Gives cached memory back to the driver: the device arenas of this handle's contexts (v may be NULL), the arenas
// of the parked contexts of destroyed handles, and the pooled pinned id blocks.  The next encode allocates again.
int wp_trim(wp_vocab *v) {
  return guarded([&] {
    auto drop = [](Context *c) {
      if (!c) return;
      WP_HIP(hipSetDevice(c->device));
      WP_HIP(hipStreamSynchronize(c->stream));
      WP_HIP(hipStreamSynchronize(c->stream2));
      release_arenas(c);
    };
    if (v) {
      drop(v->ctx.get());
      for (auto &c : v->multi) drop(c.get());
    }
    {
      std::lock_guard<std::mutex> g(g_pool_mu);
      for (auto &c : context_pool()) drop(c.get());
    }
    id_pool().trim();
  });
}

struct MappedFile {
  const char *data = nullptr;
  size_t size = 0;
  int fd = -1;
  explicit MappedFile(const char *path) {
    fd = ::open(path, O_RDONLY);
    if (fd < 0) throw std::ios_base::failure(std::string("cannot open ") + path);
    struct stat sb;
    if (fstat(fd, &sb) != 0) {
      ::close(fd);
      throw std::ios_base::failure(std::string("cannot stat ") + path);
    }
    size = static_cast<size_t>(sb.st_size);
    if (size) {
      void *p = mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0);
      if (p == MAP_FAILED) {
        ::close(fd);
        throw std::ios_base::failure(std::string("cannot mmap ") + path);
      }
      data = static_cast<const char *>(p);
    }
  }
  ~MappedFile() {
    if (data) munmap(const_cast<char *>(data), size);
    if (fd >= 0) ::close(fd);
  }
};

// the one-shot file forms: vocabulary and text from files, through wp_linear_encode or wp_fast_encode
static int encode_file(int (*encode)(wp_vocab *, const char *, size_t, int32_t **, size_t *), const char *text_file,
                       const char *vocab_file, int32_t **ids, size_t *n_ids) {
  wp_vocab *v = nullptr;
  int rc = wp_vocab_from_file(vocab_file, &v);
  if (rc != WP_OK) return rc;
  std::unique_ptr<wp_vocab> guard(v);
  return guarded([&] {
    MappedFile mm(text_file);
    if (encode(v, mm.data, mm.size, ids, n_ids) != WP_OK) throw std::runtime_error(g_last_error);
  });
}

int wp_linear_encode_file(const char *text_file, const char *vocab_file, int32_t **ids, size_t *n_ids) {
  return encode_file(wp_linear_encode, text_file, vocab_file, ids, n_ids);
}

// Host side of encodeExternal (linear.cpp:343-374): same batch rule and file format as the reference.
// Per batch: upload, encode, format the ids as text on the device (format.h), download into one of
// two pinned buffers; a writer thread appends that buffer to the file while the next batch is on the
// GPU.
namespace {
struct PinnedText {
  char *p = nullptr;
  size_t cap = 0;
  void ensure(size_t bytes) {
    if (bytes <= cap) return;
    if (p) WP_HIP(hipHostFree(p));
    p = nullptr;
    cap = 0;
    const size_t want = bytes + bytes / 8 + (1 << 20);
    WP_HIP(hipHostMalloc(reinterpret_cast<void **>(&p), want));
    cap = want;
  }
  ~PinnedText() {
    if (p) (void)hipHostFree(p);
  }
};
}  // namespace

static int encode_external_impl(const char *text_file, const char *vocab_file, const char *out_file,
                                size_t max_batch, bool fast) {
  wp_vocab *v = nullptr;
  int rc = wp_vocab_from_file(vocab_file, &v);
  if (rc != WP_OK) return rc;
  std::unique_ptr<wp_vocab> guard(v);
  return guarded([&] {
    if (max_batch == 0) throw std::invalid_argument("memory_limit too small");
    MappedFile mm(text_file);
    const char *begin = mm.data;
    size_t size = mm.size;
    FILE *fout = std::fopen(out_file, "wb");
    if (!fout) throw std::ios_base::failure(std::string("cannot open ") + out_file);
    struct Closer {
      FILE *f;
      ~Closer() { std::fclose(f); }
    } closer{fout};
    PinnedText host_text[2];
    std::future<void> pending[2];
    struct Drain {  // a failing batch must not leave a writer thread behind
      std::future<void> *p;
      ~Drain() {
        for (int i = 0; i < 2; i++) {
          if (p[i].valid()) p[i].wait();
        }
      }
    } drain{pending};
    size_t batch_no = 0;
    while (size > 0) {
      size_t batch;
      if (size > max_batch) {  // linear.cpp:357-362: grow until the batch's last byte starts a space
        batch = max_batch;
        while (batch < size) {
          const uint8_t *p = reinterpret_cast<const uint8_t *>(begin + batch - 1);
          uint32_t cp = ((p[0] & 0xc0u) == 0x80u) ? kInvalidUnicode : decode_one(p, static_cast<int64_t>(size - batch));
          if (is_space(cp)) break;
          batch++;
        }
      } else {
        batch = size;
      }
      Context *c = get_context(v);
      hipStream_t st = c->stream;
      upload_text(c, begin, batch);
      size_t n = 0;
      if (fast) {
        encode_fast_on_device(v, c, static_cast<const uint8_t *>(c->text_buf.p), batch, &n, v->stats);
      } else {
        encode_on_device(v, c, static_cast<const uint8_t *>(c->text_buf.p), batch, &n, v->stats);
      }
      if (n > 0) {
        // utils.cpp:30-35 format ("<id> " per id) on the device: byte counts, 64-bit offsets, text
        const size_t tiles = cdiv(n, kFmtTile);
        const size_t head = (tiles * (sizeof(uint32_t) + sizeof(unsigned long long)) + 8 + 255) & ~static_cast<size_t>(255);
        c->fmt_buf.ensure(head + n * 7);  // typical: <= 6 digits + space; grown below if the ids are longer
        uint32_t *tb;
        unsigned long long *to, *total;
        char *d_out;
        auto count_bytes = [&] {  // lays the buffer out (tile offsets | total | tile byte counts | text) and counts into it
          char *base = static_cast<char *>(c->fmt_buf.p);
          to = reinterpret_cast<unsigned long long *>(base);
          total = to + tiles;
          tb = reinterpret_cast<uint32_t *>(total + 1);
          d_out = base + head;
          hipLaunchKernelGGL(fmt_count_kernel, dim3(tiles), dim3(kBlock), 0, st, c->d_ids, n, tb);
          hipLaunchKernelGGL(fmt_offsets_kernel, dim3(1), dim3(1024), 0, st, tb, tiles, to, total);
        };
        count_bytes();
        WP_LAUNCH_CHECK();
        unsigned long long nbytes_out = 0;
        WP_HIP(hipMemcpyAsync(&nbytes_out, total, sizeof(nbytes_out), hipMemcpyDeviceToHost, st));
        WP_HIP(hipStreamSynchronize(st));
        if (head + nbytes_out > c->fmt_buf.cap) {  // longer ids than assumed: regrow and redo the (cheap) counts
          c->fmt_buf.ensure(head + nbytes_out);
          count_bytes();
        }
        hipLaunchKernelGGL(fmt_write_kernel, dim3(tiles), dim3(kBlock), 0, st, c->d_ids, n, to, d_out);
        WP_LAUNCH_CHECK();
        const int slot = static_cast<int>(batch_no & 1);
        if (pending[slot].valid()) pending[slot].get();  // the writer of batch_no - 2 is done with this buffer
        host_text[slot].ensure(nbytes_out);
        WP_HIP(hipMemcpyAsync(host_text[slot].p, d_out, nbytes_out, hipMemcpyDeviceToHost, st));
        WP_HIP(hipStreamSynchronize(st));
        if (batch_no > 0 && pending[slot ^ 1].valid()) pending[slot ^ 1].get();  // keep the file in batch order
        const char *src = host_text[slot].p;
        const size_t cnt = static_cast<size_t>(nbytes_out);
        pending[slot] = std::async(std::launch::async, [fout, src, cnt] {
          if (std::fwrite(src, 1, cnt, fout) != cnt) throw std::ios_base::failure("short write to the id file");
        });
        batch_no++;
      }
      begin += batch;
      size -= batch;
    }
    for (int i = 0; i < 2; i++) {
      if (pending[i].valid()) pending[i].get();
    }
  });
}

int wp_linear_encode_external(const char *text_file, const char *vocab_file, const char *out_file,
                              size_t memory_limit) {
  return encode_external_impl(text_file, vocab_file, out_file, memory_limit / 20, false);  // linear.cpp:349
}

// ---- word_piece::fast (fast.cpp:152-220) ----------------------------------------------------------------
int wp_fast_encode_device(wp_vocab *v, const void *d_utf8, size_t nbytes, const int32_t **d_ids, size_t *n_ids) {
  return guarded([&] {
    check_device_text(d_utf8);
    size_t n = 0;
    Context *c = get_context(v);
    encode_fast_on_device(v, c, static_cast<const uint8_t *>(d_utf8), nbytes, &n, v->stats);
    *d_ids = n ? c->d_ids : nullptr;
    *n_ids = n;
  });
}

int wp_fast_encode(wp_vocab *v, const char *utf8, size_t nbytes, int32_t **ids, size_t *n_ids) {
  return guarded([&] {
    *ids = nullptr;
    *n_ids = 0;
    if (nbytes == 0) return;  // fast.cpp:154-156
    const auto t_all = wp_clock::now();
    Context *c = get_context(v);
    upload_text(c, utf8, nbytes);
    size_t n = 0;
    encode_fast_on_device(v, c, static_cast<const uint8_t *>(c->text_buf.p), nbytes, &n, v->stats);
    if (n) {
      Downloads down(c->stream);
      down.add(ids, c->d_ids, n * sizeof(int32_t));
      down.finish();
      *n_ids = n;
    }
    v->stats.ms_host_total = ms_since(t_all);
  });
}

int wp_fast_encode_file(const char *text_file, const char *vocab_file, int32_t **ids, size_t *n_ids) {
  return encode_file(wp_fast_encode, text_file, vocab_file, ids, n_ids);
}

int wp_fast_encode_external(const char *text_file, const char *vocab_file, const char *out_file, size_t memory_limit) {
  return encode_external_impl(text_file, vocab_file, out_file, memory_limit / 2, true);  // fast.cpp:195
}

// UTF-8 of the stored word of line i (without the "##" of continuation tokens: utils.cpp:83-85), for
// word_piece::fast::decode (fast.cpp:163-187).  Returns the byte length; copies at most `cap` bytes.
int64_t wp_vocab_token_utf8(const wp_vocab *v, int64_t i, char *buf, size_t cap) {
  if (i < 0 || static_cast<size_t>(i) >= v->hv.tokens.size()) return -1;
  std::string out;
  for (uint32_t cp : v->hv.tokens[static_cast<size_t>(i)].word) {  // utf8.cpp:98-121 utf8_to_chars
    if (cp < 0x80) {
      out.push_back(static_cast<char>(cp));
    } else if (cp < 0x800) {
      out.push_back(static_cast<char>(0xc0 | (cp >> 6)));
      out.push_back(static_cast<char>(0x80 | (cp & 0x3f)));
    } else if (cp < 0x10000) {
      out.push_back(static_cast<char>(0xe0 | (cp >> 12)));
      out.push_back(static_cast<char>(0x80 | ((cp >> 6) & 0x3f)));
      out.push_back(static_cast<char>(0x80 | (cp & 0x3f)));
    } else {
      out.push_back(static_cast<char>(0xf0 | (cp >> 18)));
      out.push_back(static_cast<char>(0x80 | ((cp >> 12) & 0x3f)));
      out.push_back(static_cast<char>(0x80 | ((cp >> 6) & 0x3f)));
      out.push_back(static_cast<char>(0x80 | (cp & 0x3f)));
    }
  }
  if (buf && cap) std::memcpy(buf, out.data(), std::min(cap, out.size()));
  return static_cast<int64_t>(out.size());
}

int wp_linear_debug_fetch(const wp_vocab *v, int which, int32_t *out, size_t capacity, size_t *n_out) {
  return guarded([&] {
    if (!v->ctx || v->ctx->dbg.n == 0) throw std::invalid_argument("no encode has run on this handle");
    Context *c = v->ctx.get();
    WP_HIP(hipSetDevice(c->device));
    const auto &d = c->dbg;
    const void *src = nullptr;
    size_t cnt = d.n;
    switch (which) {
      case 0: src = d.sym; break;
      case 1:
        if (!d.sa) throw std::invalid_argument("the suffix array is kept only with WP_OPT_KEEP_DEBUG");
        src = d.sa;
        break;
      case 2:  // (key lookup: the ranks of the needed list stand over their keys, there is no table; linear_path.h, rank_out)
        if (!d.rank) throw std::invalid_argument("the rank table is kept only with WP_OPT_KEEP_DEBUG, full depth or the reference layout");
        src = d.rank;
        break;
      case 3: src = d.lcp; cnt = d.n - 1; break;
      case 4:
      case 5: {  // materialise the reference's per-slot arrays from the step functions
        hipLaunchKernelGGL(step_expand_kernel, dim3(cdiv(d.n, kBlock)), dim3(kBlock), 0, c->stream, d.steps, d.n,
                           d.best_scratch, d.best_scratch + d.n);
        WP_LAUNCH_CHECK();
        WP_HIP(hipStreamSynchronize(c->stream));
        src = which == 4 ? d.best_scratch : d.best_scratch + d.n;
        break;
      }
      case 6:
        if (!d.cps) throw std::invalid_argument("code points are kept only with WP_OPT_KEEP_DEBUG");
        src = d.cps;
        cnt = d.n_text;
        break;
      case 7:
        if (!d.cls) throw std::invalid_argument("class bytes are kept only with WP_OPT_KEEP_DEBUG");
        src = d.cls;
        cnt = d.n_text;
        break;
      case 8:
      case 9:
      case 10:
      case 11:
        if (!d.step_views) throw std::invalid_argument("the step views are kept only with WP_OPT_KEEP_DEBUG = 2");
        src = d.step_views + static_cast<size_t>(which - 8) * d.n_text;
        cnt = d.n_text;
        break;
      default: throw std::invalid_argument("unknown debug array");
    }
    if (cnt > capacity) throw std::invalid_argument("debug buffer too small");
    *n_out = cnt;
    if (cnt == 0) return;
    if ((which == 0 && d.sym_bytes == 1) || which == 7) {
      std::vector<uint8_t> tmp(cnt);
      WP_HIP(hipMemcpy(tmp.data(), src, cnt, hipMemcpyDeviceToHost));
      for (size_t i = 0; i < cnt; i++) out[i] = tmp[i];
    } else {
      WP_HIP(hipMemcpy(out, src, cnt * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
  });
}

void wp_free(void *p) {
  if (!p) return;
  if (!id_pool().give_back(p)) std::free(p);
}
const char *wp_last_error(void) { return g_last_error.c_str(); }
int wp_device_count(void) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess) return 0;
  return count;
}

}  // extern "C"
