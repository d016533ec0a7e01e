// encoder.hip — the C ABI of the HIP Linear-WordPiece path (include/wordpiece_amd.h) and the one translation unit the
// device code is compiled in.  The device path itself: linear_path.h (word_piece::linear, stage by stage) and
// fast_path.h (word_piece::fast); what a handle owns on a device: context.h.
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <atomic>
#include <chrono>
#include <cstring>
#include <fstream>
#include <functional>
#include <future>
#include <memory>
#include <mutex>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/wordpiece_amd.h"
#include "context.h"
#include "detok.h"
#include "fast_path.h"
#include "format.h"
#include "inputs.h"
#include "linear_path.h"
#include "mask.h"
#include "packing.h"


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
  } catch (const std::exception &e) {
    g_last_error = e.what();
    return WP_ERR_HIP;
  } catch (...) {
    g_last_error = "unknown exception inside the HIP WordPiece library";
    return WP_ERR_HIP;
  }
}

// ---- argument rules that several entry points share -----------------------------------------------------------------
static void check_device_text(const void *d_utf8) {
  if ((reinterpret_cast<uintptr_t>(d_utf8) & 3u) != 0) throw std::invalid_argument("device text must be 4-byte aligned");
}
static void check_device_doc_off(const void *d_doc_off) {
  if ((reinterpret_cast<uintptr_t>(d_doc_off) & 7u) != 0) throw std::invalid_argument("device document offsets must be 8-byte aligned");
}
// a device documents call without text has no rows: explicit rows cannot end at 0 unless there are none
static void check_doc_off_without_text(const void *d_doc_off, size_t n_docs) {
  if (d_doc_off && n_docs != 0) throw std::invalid_argument("document offsets must increase from 0 to nbytes");
}
static bool known_norm_flags(int64_t flags) { return flags >= 0 && (flags & ~static_cast<int64_t>(kNormKnownFlags)) == 0; }

// wp_vocab_token_flags, and the class byte of an id on the device (mask.h)
static int32_t token_flags(const HostToken &t) { return (t.is_prefix ? 1 : 0) | (t.is_special ? 2 : 0) | (t.is_malformed ? 4 : 0); }

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
  void finish() {
    WP_HIP(hipStreamSynchronize(st));
    for (auto &it : items) std::memcpy(it.second, &it.first, sizeof(void *));  // (*out = block, for every T * alike)
    items.clear();
  }
};

using wp_clock = std::chrono::steady_clock;
double ms_since(wp_clock::time_point t0) { return std::chrono::duration<double, std::milli>(wp_clock::now() - t0).count(); }

// uploads [utf8, utf8 + nbytes) into a text buffer (grown and padded as the decoder expects: context.h) on stream st
void upload_text(DeviceBuffer &buf, hipStream_t st, const char *utf8, size_t nbytes) {
  buf.ensure(text_room(nbytes));
  zero_text_tail(buf.p, nbytes, st);
  WP_HIP(hipMemcpyAsync(buf.p, utf8, nbytes, hipMemcpyHostToDevice, st));
}
void upload_text(Context *c, const char *utf8, size_t nbytes) { upload_text(c->text_buf, c->stream, utf8, nbytes); }

// lanes of a wave that share a row of max_len cells (pack_rows_kernel, inputs_pack_kernel, mask_kernel)
int lanes_for(int max_len) {
  int lanes = 4;
  while (lanes < kWave && lanes < max_len) lanes *= 2;
  return lanes;
}

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

// ---- documents (include/wordpiece_amd.h, section "documents"; kernels: rows.h) --------------------------------------
namespace {
struct RowsResult {  // device pointers, valid until the handle's next call
  const int32_t *d_ids = nullptr;
  const long long *d_row_splits = nullptr;
  const uint32_t *d_offs = nullptr;
  size_t n_ids = 0, n_rows = 0;
};

// A vocabulary that can match differently inside a joined text than in a document of its own: an eligible token with
// U+000A matches across the separator; a token with U+0000 / U+0001 can match into the 1 . vocab tail of S, which only
// the end of a text has; with duplicate eligible lines the copy a match at the end of a text names depends on what
// follows it.  Such batches are encoded document by document.
bool rows_per_document(const wp_vocab *v) { return v->hv.newline_in_token || v->hv.low_cp || v->hv.n_dup_eligible > 0; }

void check_rows_call(int unit, size_t nbytes) {
  if (unit != -1 && unit != WP_OFFSETS_BYTES && unit != WP_OFFSETS_CODE_POINTS) {
    throw std::invalid_argument("offsets unit must be -1 (none), 0 (bytes) or 1 (code points)");
  }
  // (row membership goes through the 32-bit first-byte table of the code points in every unit)
  if (nbytes > static_cast<size_t>(UINT32_MAX)) throw std::length_error("a documents call needs nbytes <= UINT32_MAX");
}

int padded_specials(int max_len, int32_t cls_id, int32_t sep_id) {
  const int specials = (cls_id >= 0 ? 1 : 0) + (sep_id >= 0 ? 1 : 0);
  if (max_len < 1 || max_len < specials) throw std::invalid_argument("max_len must be at least 1 and at least the number of specials");
  return specials;
}

void check_doc_off_host(const char *utf8, size_t nbytes, const int64_t *doc_off, size_t n_docs) {
  bool ok = doc_off[0] == 0 && static_cast<uint64_t>(doc_off[n_docs]) == nbytes && doc_off[n_docs] >= 0;
  for (size_t i = 1; ok && i <= n_docs; i++) {
    ok = doc_off[i] > doc_off[i - 1] && static_cast<uint64_t>(doc_off[i]) <= nbytes && utf8[doc_off[i] - 1] == '\n';
  }
  if (!ok) throw std::invalid_argument("document offsets must increase from 0 to nbytes with a '\\n' in front of each");
}

// The per-document route: the rows' starts come to the host (explicit: checked and copied; lines: found by the kernels
// of the joined route), every document is copied into the context's second text buffer (a document starts at any byte,
// the decoder wants 4-byte alignment) and encoded through the existing ids-only / offsets path, and the assembled result
// goes back into c->rows_out.  A correctness route: it syncs per document.
void rows_by_document(wp_vocab *v, Context *c, const uint8_t *d_text, size_t nbytes, const long long *d_doc_off, size_t n_docs,
                      int unit, size_t capacity, RowsResult &out) {
  hipStream_t st = c->stream;
  clear_scalars(c, kScalarRows, kScalarRowsCut, st);
  size_t n_rows = n_docs;
  const void *d_starts = d_doc_off;
  auto check_capacity = [&] {
    out.n_rows = n_rows;
    if (n_rows > capacity) throw std::invalid_argument("capacity_rows is smaller than the number of rows");
  };
  if (d_doc_off) {
    hipLaunchKernelGGL(rows_check_kernel, dim3(cdiv(n_docs + 1, kBlock)), dim3(kBlock), 0, st, d_text, nbytes, d_doc_off, n_docs,
                       c->d_scalars + kScalarRowsBad);
    WP_LAUNCH_CHECK();
    fetch_scalars(c, kScalarRowsCut);
    if (c->h_scalars[kScalarRowsBad] != 0) {
      throw std::invalid_argument("document offsets must increase from 0 to nbytes with a '\\n' in front of each");
    }
    check_capacity();
  } else {
    const unsigned tiles = cdiv(nbytes, kLineTile);
    const size_t tmp_words = cdiv(tiles, kScanTile) + 8;
    c->rows_in.ensure((tiles + 1 + tmp_words) * sizeof(uint32_t));
    uint32_t *d_cnt = static_cast<uint32_t *>(c->rows_in.p);
    hipLaunchKernelGGL(line_count_kernel, dim3(tiles), dim3(kBlock), 0, st, d_text, nbytes, d_cnt);
    device_exclusive_scan(d_cnt, d_cnt, tiles, d_cnt + tiles + 1, c->d_scalars + kScalarRows, st);
    fetch_scalars(c, kScalarRowsCut);
    n_rows = c->h_scalars[kScalarRows];
    check_capacity();
    c->rows_out.ensure((n_rows + 1) * sizeof(long long));
    hipLaunchKernelGGL(line_write_kernel, dim3(tiles), dim3(kBlock), 0, st, d_text, nbytes, static_cast<const uint32_t *>(d_cnt), n_rows,
                       static_cast<long long *>(c->rows_out.p));
    WP_LAUNCH_CHECK();
    d_starts = c->rows_out.p;
  }
  std::vector<long long> starts(n_rows + 1);
  WP_HIP(hipMemcpyAsync(starts.data(), d_starts, (n_rows + 1) * sizeof(long long), hipMemcpyDeviceToHost, st));
  WP_HIP(hipStreamSynchronize(st));
  uint8_t last = '\n';
  WP_HIP(hipMemcpyAsync(&last, d_text + nbytes - 1, 1, hipMemcpyDeviceToHost, st));
  WP_HIP(hipStreamSynchronize(st));
  auto doc_end = [&](size_t i) {  // (a last line without a separator runs to the end of the text)
    return static_cast<size_t>(starts[i + 1]) - ((i + 1 == n_rows && last != '\n') ? 0 : 1);
  };
  size_t longest = 0;
  for (size_t i = 0; i < n_rows; i++) longest = std::max(longest, doc_end(i) - static_cast<size_t>(starts[i]));
  c->text_buf2.ensure(text_room(longest));
  std::vector<int32_t> h_ids;
  std::vector<uint32_t> h_offs;
  std::vector<long long> splits(n_rows + 1, 0);
  EncodeStats last_stats;
  std::memset(&last_stats, 0, sizeof(last_stats));
  int32_t guard_zones = 0;
  int64_t norm_bytes = 0;  // (WP_OPT_NORMALIZE: every document is normalised by its own encode)
  for (size_t i = 0; i < n_rows; i++) {
    splits[i] = static_cast<long long>(h_ids.size());
    const size_t a = static_cast<size_t>(starts[i]), len = doc_end(i) - a;
    if (len == 0) continue;
    char *dst = static_cast<char *>(c->text_buf2.p);
    zero_text_tail(dst, len, st);
    WP_HIP(hipMemcpyAsync(dst, d_text + a, len, hipMemcpyDeviceToDevice, st));
    size_t n = 0;
    encode_on_device(v, c, reinterpret_cast<const uint8_t *>(dst), len, &n, last_stats, unit);
    guard_zones = std::max(guard_zones, last_stats.guard_zones);
    norm_bytes += last_stats.norm_bytes;
    if (n == 0) continue;
    const size_t at = h_ids.size();
    h_ids.resize(at + n);
    WP_HIP(hipMemcpyAsync(h_ids.data() + at, c->d_ids, n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (unit >= 0) {
      h_offs.resize(2 * (at + n));
      WP_HIP(hipMemcpyAsync(h_offs.data() + 2 * at, c->d_offs, 2 * n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    }
    WP_HIP(hipStreamSynchronize(st));
  }
  const size_t n_ids = h_ids.size();
  splits[n_rows] = static_cast<long long>(n_ids);
  // result block: row_splits | offsets | ids
  const size_t split_bytes = (n_rows + 1) * sizeof(long long), offs_bytes = unit >= 0 ? n_ids * 2 * sizeof(uint32_t) : 0;
  c->rows_out.ensure(split_bytes + offs_bytes + n_ids * sizeof(int32_t) + 16);
  char *base = static_cast<char *>(c->rows_out.p);
  WP_HIP(hipMemcpyAsync(base, splits.data(), split_bytes, hipMemcpyHostToDevice, st));
  if (offs_bytes) WP_HIP(hipMemcpyAsync(base + split_bytes, h_offs.data(), offs_bytes, hipMemcpyHostToDevice, st));
  if (n_ids) WP_HIP(hipMemcpyAsync(base + split_bytes + offs_bytes, h_ids.data(), n_ids * sizeof(int32_t), hipMemcpyHostToDevice, st));
  WP_HIP(hipStreamSynchronize(st));
  c->d_ids = nullptr;  // (the arenas hold the last document only)
  c->d_offs = nullptr;
  out.d_row_splits = reinterpret_cast<const long long *>(base);
  out.d_offs = (offs_bytes && n_ids) ? reinterpret_cast<const uint32_t *>(base + split_bytes) : nullptr;
  out.d_ids = n_ids ? reinterpret_cast<const int32_t *>(base + split_bytes + offs_bytes) : nullptr;
  out.n_ids = n_ids;
  v->stats = last_stats;  // (of the last non-empty document; the sums of the call below)
  v->stats.guard_zones = guard_zones;
  v->stats.normalize = v->normalize;
  v->stats.norm_bytes = norm_bytes;
  v->stats.n_bytes = static_cast<int64_t>(nbytes);
  v->stats.n_ids = static_cast<int64_t>(n_ids);
  v->stats.n_rows = static_cast<int64_t>(n_rows);
  v->stats.rows_route = 0;
}

// both routes: d_text as wp_linear_encode_device wants it, nbytes > 0; d_doc_off in device memory or nullptr (lines)
void rows_on_device(wp_vocab *v, Context *c, const uint8_t *d_text, size_t nbytes, const long long *d_doc_off, size_t n_docs, int unit,
                    size_t capacity, RowsResult &out) {
  if (rows_per_document(v)) {
    rows_by_document(v, c, d_text, nbytes, d_doc_off, n_docs, unit, capacity, out);
  } else {
    RowsCall rc{d_doc_off, n_docs, unit, capacity};
    size_t n = 0;
    try {  // (row membership comes from the spans: without a unit they stay in code points, which need no second pass)
      encode_on_device(v, c, d_text, nbytes, &n, v->stats, unit >= 0 ? unit : WP_OFFSETS_CODE_POINTS, &rc);
    } catch (...) {
      out.n_rows = rc.n_rows;
      throw;
    }
    out.d_ids = n ? c->d_ids : nullptr;
    out.d_row_splits = rc.d_row_splits;
    out.d_offs = (n && unit >= 0) ? c->d_offs : nullptr;
    out.n_ids = n;
    out.n_rows = rc.n_rows;
  }
  v->stats.offsets_unit = unit;
  v->stats.n_devices = 1;
}

// the padded batch of a rows result, into device buffers of n_rows * max_len and n_rows int32; waits for it
void pack_on_device(wp_vocab *v, Context *c, const RowsResult &r, int max_len, int32_t cls_id, int32_t sep_id, int32_t pad_id,
                    int32_t *d_input_ids, int32_t *d_lengths) {
  v->stats.rows_truncated = 0;
  if (r.n_rows == 0) return;
  const int lanes = lanes_for(max_len);
  clear_scalars(c, kScalarRowsCut, kScalarRowsCut, c->stream);
  hipLaunchKernelGGL(pack_rows_kernel, dim3(cdiv(r.n_rows, static_cast<size_t>(kBlock / lanes))), dim3(kBlock), 0, c->stream, r.d_ids,
                     r.d_row_splits, r.n_rows, max_len, cls_id, sep_id, pad_id, lanes, d_input_ids, d_lengths,
                     c->d_scalars + kScalarRowsCut);
  WP_LAUNCH_CHECK();
  fetch_scalars(c, kScalarRowsCut);
  v->stats.rows_truncated = c->h_scalars[kScalarRowsCut];
}

// the host form of a documents call as far as its rows: the text and the explicit row starts go up, then rows_on_device
Context *rows_from_host(wp_vocab *v, const char *utf8, size_t nbytes, const int64_t *doc_off, size_t n_docs, int unit, RowsResult &r) {
  Context *c = get_context(v);
  upload_text(c, utf8, nbytes);
  if (doc_off) {
    c->rows_in.ensure((n_docs + 1) * sizeof(int64_t));
    WP_HIP(hipMemcpyAsync(c->rows_in.p, doc_off, (n_docs + 1) * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
  }
  rows_on_device(v, c, static_cast<const uint8_t *>(c->text_buf.p), nbytes, doc_off ? static_cast<const long long *>(c->rows_in.p) : nullptr,
                 n_docs, unit, SIZE_MAX, r);
  return c;
}

void *zeroed(size_t bytes) {
  void *p = std::calloc(std::max<size_t>(bytes, 1), 1);
  if (!p) throw std::bad_alloc();
  return p;
}
}  // namespace

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
    const size_t cells = r.n_rows * static_cast<size_t>(max_len);
    c->pad_buf.ensure((cells + r.n_rows) * sizeof(int32_t));
    int32_t *d_out = static_cast<int32_t *>(c->pad_buf.p), *d_len = d_out + cells;
    pack_on_device(v, c, r, max_len, cls_id, sep_id, pad_id, d_out, d_len);
    Downloads down(c->stream);
    down.add(input_ids, d_out, cells * sizeof(int32_t));
    down.add(lengths, d_len, r.n_rows * sizeof(int32_t));
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
    pack_on_device(v, c, r, max_len, cls_id, sep_id, pad_id, d_input_ids, d_lengths);
    *n_rows = r.n_rows;
  });
}

}  // extern "C"

// ---- masking (include/wordpiece_amd.h, section "masking"; kernel: mask.h) --------------------------------------------
namespace {
constexpr unsigned long long kQ32One = 1ull << 32;

// every argument rule of a mask (mask_call) or word-ids call that needs no device
MaskGeom check_mask_spec(const wp_vocab *v, const wp_mask_spec *spec, size_t n_rows, bool mask_call) {
  if (!spec) throw std::invalid_argument("mask: spec is NULL");
  if (spec->max_len < 1) throw std::invalid_argument("mask: max_len must be at least 1");
  MaskGeom g{};
  g.max_len = spec->max_len;
  g.cls_id = spec->cls_id;
  g.sep_id = spec->sep_id;
  g.pad_id = spec->pad_id;
  g.vocab_size = static_cast<long long>(v->hv.tokens.size());
  if (mask_call) {
    if (spec->whole_word != 0 && spec->whole_word != 1) throw std::invalid_argument("mask: whole_word must be 0 or 1");
    if (spec->select_q32 > kQ32One) throw std::invalid_argument("mask: select_q32 must be at most 2^32");
    if (spec->mask_q32 > kQ32One) throw std::invalid_argument("mask: mask_q32 must be at most 2^32");
    if (spec->random_q32 > kQ32One) throw std::invalid_argument("mask: random_q32 must be at most 2^32");
    if (spec->mask_q32 + spec->random_q32 > kQ32One) throw std::invalid_argument("mask: mask_q32 + random_q32 must be at most 2^32");
    if (spec->mask_id < 0) throw std::invalid_argument("mask: mask_id must be at least 0");
    g.mask_id = spec->mask_id;
    g.ignore_id = spec->ignore_id;
    g.whole_word = spec->whole_word;
    g.select_q32 = spec->select_q32;
    g.mask_q32 = spec->mask_q32;
    g.random_q32 = spec->random_q32;
    g.seed = spec->seed;
    g.row_base = spec->row_base;
  }
  if (n_rows > static_cast<size_t>(INT32_MAX)) throw std::length_error("mask: more rows than INT32_MAX");
  if (n_rows > SIZE_MAX / sizeof(int32_t) / static_cast<size_t>(spec->max_len)) {
    throw std::length_error("mask: n_rows * max_len is too large");
  }
  return g;
}

// the statistics of a mask or word-ids call before its counters are known (all there is to say of a call without rows)
wp_mask_stats &begin_mask_stats(wp_vocab *v, size_t n_rows, int whole_word) {
  v->stats.mask_call = 1;
  v->stats.mask = wp_mask_stats{};
  v->stats.mask.n_rows = static_cast<int64_t>(n_rows);
  v->stats.mask.whole_word = whole_word;
  return v->stats.mask;
}

// One launch of mask_kernel over device buffers on c's stream, one wait (for the counters), the statistics of the call.
// d_masked == nullptr: the word-ids form.
void mask_on_device(wp_vocab *v, Context *c, const int32_t *d_in, const int32_t *d_lengths, size_t n_rows, const MaskGeom &g,
                    int32_t *d_masked, int32_t *d_labels, int32_t *d_word_ids) {
  const bool mask_call = d_masked != nullptr;
  wp_mask_stats &ms = begin_mask_stats(v, n_rows, mask_call ? g.whole_word : 0);
  if (n_rows == 0) return;
  hipStream_t st = c->stream;
  if (!c->d_tok_class) {  // one byte per id: wp_vocab_token_flags
    std::vector<uint8_t> cls(v->hv.tokens.size());
    for (size_t i = 0; i < cls.size(); i++) cls[i] = static_cast<uint8_t>(token_flags(v->hv.tokens[i]));
    c->d_tok_class = upload(cls, st);
    WP_HIP(hipStreamSynchronize(st));  // cls is a local
  }
  unsigned long long *d_cnt = reinterpret_cast<unsigned long long *>(c->d_scalars + kScalarMask);
  WP_HIP(hipMemsetAsync(d_cnt, 0, kMaskCounters * sizeof(unsigned long long), st));
  const int lanes = lanes_for(g.max_len);
  const size_t n_blocks = (n_rows + static_cast<size_t>(kBlock / lanes) - 1) / static_cast<size_t>(kBlock / lanes);
  const dim3 grid(static_cast<unsigned>(std::min<size_t>(n_blocks, kMaskMaxGrid))), block(kBlock);
  if (!mask_call) {
    hipLaunchKernelGGL((mask_kernel<false, true>), grid, block, 0, st, d_in, d_lengths, n_rows, n_blocks, g, lanes,
                       c->d_tok_class, d_masked, d_labels,
                       d_word_ids, d_cnt);
  } else if (d_word_ids) {
    hipLaunchKernelGGL((mask_kernel<true, true>), grid, block, 0, st, d_in, d_lengths, n_rows, n_blocks, g, lanes,
                       c->d_tok_class, d_masked, d_labels,
                       d_word_ids, d_cnt);
  } else {
    hipLaunchKernelGGL((mask_kernel<true, false>), grid, block, 0, st, d_in, d_lengths, n_rows, n_blocks, g, lanes,
                       c->d_tok_class, d_masked, d_labels,
                       d_word_ids, d_cnt);
  }
  WP_LAUNCH_CHECK();
  unsigned long long *h_cnt = reinterpret_cast<unsigned long long *>(c->h_scalars + kScalarMask);
  WP_HIP(hipMemcpyAsync(h_cnt, d_cnt, kMaskCounters * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  WP_HIP(hipStreamSynchronize(st));
#ifdef WP_DEBUG_BOUNDS
  {
    unsigned int oob = 0;
    take_oob(kSiteMask, 1, &oob);
    if (oob != 0) throw HipError("debug bounds: masking: " + std::to_string(oob) + " class lookups outside the vocabulary skipped");
  }
#endif
  ms.n_words = static_cast<int64_t>(h_cnt[kMaskWords]);
  ms.n_selected = static_cast<int64_t>(h_cnt[kMaskSelected]);
  ms.n_selected_units = static_cast<int64_t>(h_cnt[kMaskUnits]);
  ms.n_masked = static_cast<int64_t>(h_cnt[kMaskMasked]);
  ms.n_random = static_cast<int64_t>(h_cnt[kMaskRandom]);
  ms.n_kept = static_cast<int64_t>(h_cnt[kMaskKept]);
}

// the host entry points: ids (and lengths) up, one launch, 1..3 blocks of n_rows * max_len int32 down
void mask_from_host(wp_vocab *v, const int32_t *input_ids, const int32_t *lengths, size_t n_rows, const MaskGeom &g, int32_t **masked,
                    int32_t **labels, int32_t **word_ids) {
  const size_t cells = n_rows * static_cast<size_t>(g.max_len);
  Context *c = get_context(v);
  const int n_out = (masked ? 2 : 0) + (word_ids ? 1 : 0);
  // ids | outputs | lengths
  c->pad_buf.ensure((cells * (1 + static_cast<size_t>(n_out)) + n_rows) * sizeof(int32_t) + 16);
  int32_t *d_in = static_cast<int32_t *>(c->pad_buf.p);
  int32_t *d_masked = masked ? d_in + cells : nullptr, *d_labels = masked ? d_in + 2 * cells : nullptr;
  int32_t *d_wid = word_ids ? d_in + (masked ? 3 : 1) * cells : nullptr;
  int32_t *d_len = lengths ? d_in + (1 + static_cast<size_t>(n_out)) * cells : nullptr;
  WP_HIP(hipMemcpyAsync(d_in, input_ids, cells * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
  if (lengths) WP_HIP(hipMemcpyAsync(d_len, lengths, n_rows * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
  mask_on_device(v, c, d_in, d_len, n_rows, g, d_masked, d_labels, d_wid);
  Downloads down(c->stream);
  if (masked) {
    down.add(masked, d_masked, cells * sizeof(int32_t));
    down.add(labels, d_labels, cells * sizeof(int32_t));
  }
  if (word_ids) down.add(word_ids, d_wid, cells * sizeof(int32_t));
  down.finish();
}
}  // namespace

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
    mask_from_host(v, input_ids, lengths, n_rows, g, nullptr, nullptr, word_ids);
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
    mask_from_host(v, input_ids, lengths, n_rows, g, masked, labels, word_ids);
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

// ---- detokenize (include/wordpiece_amd.h, section "detokenize"; kernels: detok.h) -----------------------------------
namespace {
size_t up256(size_t bytes) { return (bytes + 255) & ~static_cast<size_t>(255); }

// every argument rule that needs neither the ids nor a device; n_cells of a padded call, -1 of a ragged one
DetokGeom check_detok_spec(const wp_vocab *v, const wp_detok_spec *spec, size_t n_rows) {
  if (!spec) throw std::invalid_argument("detokenize: spec is NULL");
  if (spec->cleanup != 0 && spec->cleanup != 1) throw std::invalid_argument("detokenize: cleanup must be 0 or 1");
  if (spec->terminator < -1 || spec->terminator > 255) throw std::invalid_argument("detokenize: terminator must lie in [-1, 255]");
  if (spec->n_skip < 0 || spec->n_skip > 8) throw std::invalid_argument("detokenize: n_skip must lie in [0, 8]");
  if (spec->max_len < 0) throw std::invalid_argument("detokenize: max_len must be at least 0");
  if (n_rows > static_cast<size_t>(INT32_MAX)) throw std::length_error("detokenize: more rows than INT32_MAX");
  DetokGeom g{};
  g.n_rows = static_cast<long long>(n_rows);
  g.max_len = spec->max_len;
  g.term = spec->terminator;
  g.n_skip = spec->n_skip;
  for (int k = 0; k < 8; k++) g.skip_ids[k] = k < spec->n_skip ? spec->skip_ids[k] : -1;
  g.vocab_size = static_cast<long long>(v->hv.tokens.size());
  g.n_cells = -1;
  if (spec->max_len > 0) {  // (n_rows <= 2^31 - 1 and max_len <= 2^31 - 1: the product fits 64 bits)
    g.n_cells = static_cast<long long>(n_rows) * spec->max_len;
    if (g.n_cells > INT32_MAX) throw std::length_error("detokenize: more cells than INT32_MAX");
  }
  return g;
}

wp_detok_stats &begin_detok_stats(wp_vocab *v, size_t n_rows) {
  v->stats.detok_call = 1;
  v->stats.detok = wp_detok_stats{};
  v->stats.detok.n_rows = static_cast<int64_t>(n_rows);
  return v->stats.detok;
}

// the pieces of every id, both forms, both cleanup values: records [cleanup][form][id] and the pool of their bytes
void ensure_detok_table(const wp_vocab *v, Context *c) {
  if (c->d_detok_rec) return;
  const size_t V = v->hv.tokens.size();
  std::vector<DetokRec> rec(4 * V);
  std::vector<uint8_t> pool;
  for (int cleanup = 0; cleanup < 2; cleanup++) {
    for (int form = 0; form < 2; form++) {
      for (size_t i = 0; i < V; i++) {
        const HostToken &t = v->hv.tokens[i];
        DetokRec &r = rec[(static_cast<size_t>(cleanup) * 2 + static_cast<size_t>(form)) * V + i];
        if (t.is_malformed) {
          r = DetokRec{kDetokNoPiece, 0};
          continue;
        }
        const std::string piece = detok_piece_bytes(t, form, cleanup);
        if (cleanup == 1 && piece == detok_piece_bytes(t, form, 0)) {  // the clean-up changes few pieces: the bytes are shared
          r = rec[static_cast<size_t>(form) * V + i];
          continue;
        }
        if (pool.size() + piece.size() >= static_cast<size_t>(kDetokNoPiece)) throw std::length_error("detokenize: the pieces of the vocabulary exceed 4 GB");
        r = DetokRec{static_cast<uint32_t>(pool.size()), static_cast<uint32_t>(piece.size())};
        pool.insert(pool.end(), piece.begin(), piece.end());
      }
    }
  }
  c->d_detok_rec = upload(rec, c->stream);
  c->d_detok_pool = upload(pool, c->stream);
  c->detok_pool_bytes = pool.size();
  WP_HIP(hipStreamSynchronize(c->stream));  // rec and pool are locals
}

// The three passes over device buffers on c's stream.  g.n_cells < 0: a ragged call whose row_splits have not been
// checked (the device entry point).  The result lies in c->detok_out until the handle's next call.
void detok_on_device(wp_vocab *v, Context *c, const int32_t *d_ids, const long long *d_splits, const int32_t *d_lengths, DetokGeom g,
                     int cleanup, const void **d_text, const long long **d_text_off, size_t *n_bytes) {
  wp_detok_stats &ds = begin_detok_stats(v, static_cast<size_t>(g.n_rows));
  hipStream_t st = c->stream;
  const size_t n_rows = static_cast<size_t>(g.n_rows);
  if (g.n_cells < 0) {
    clear_scalars(c, kScalarDetokLast, kScalarDetokBad, st);
    hipLaunchKernelGGL(detok_check_splits_kernel, dim3(std::min<unsigned>(cdiv(n_rows + 1, kBlock), 1024u)), dim3(kBlock), 0, st, d_splits,
                       n_rows, c->d_scalars + kScalarDetokBad, reinterpret_cast<long long *>(c->d_scalars + kScalarDetokLast));
    WP_LAUNCH_CHECK();
    WP_HIP(hipMemcpyAsync(c->h_scalars + kScalarDetokLast, c->d_scalars + kScalarDetokLast,
                          sizeof(uint32_t) * (scalar_end(kScalarDetokBad) - kScalarDetokLast), hipMemcpyDeviceToHost, st));
    WP_HIP(hipStreamSynchronize(st));
    if (c->h_scalars[kScalarDetokBad] != 0) throw std::invalid_argument("detokenize: row_splits must start at 0 and never descend");
    long long last;
    std::memcpy(&last, c->h_scalars + kScalarDetokLast, sizeof(last));
    if (last > INT32_MAX) throw std::length_error("detokenize: more cells than INT32_MAX");
    g.n_cells = last;
  }
  if (g.n_cells > 0 && !d_ids) throw std::invalid_argument("detokenize: ids is NULL");
  ensure_detok_table(v, c);
  g.pool_bytes = c->detok_pool_bytes;
  const size_t n_tiles = static_cast<size_t>(g.n_cells) / kDetokTile + 1;
  // tile records | tile offsets | tile carries
  const size_t off_rec = 0, off_off = up256(n_tiles * sizeof(DetokTile)), off_carry = off_off + up256(n_tiles * sizeof(unsigned long long));
  c->detok_aux.ensure(off_carry + up256(n_tiles * sizeof(uint32_t)));
  char *aux = static_cast<char *>(c->detok_aux.p);
  DetokTile *d_tiles = reinterpret_cast<DetokTile *>(aux + off_rec);
  unsigned long long *d_tile_off = reinterpret_cast<unsigned long long *>(aux + off_off);
  uint32_t *d_tile_carry = reinterpret_cast<uint32_t *>(aux + off_carry);
  const DetokRec *d_rec = c->d_detok_rec + static_cast<size_t>(cleanup) * 2 * static_cast<size_t>(g.vocab_size);
  unsigned long long *d_tot = reinterpret_cast<unsigned long long *>(c->d_scalars + kScalarDetok);
  const dim3 grid(static_cast<unsigned>(n_tiles)), block(kBlock);
  hipLaunchKernelGGL((detok_tile_kernel<false>), grid, block, 0, st, d_ids, d_splits, d_lengths, g, d_rec, c->d_detok_pool, d_tiles,
                     static_cast<const unsigned long long *>(nullptr), static_cast<const uint32_t *>(nullptr),
                     static_cast<uint8_t *>(nullptr), static_cast<long long *>(nullptr));
  hipLaunchKernelGGL(detok_spine_kernel, dim3(1), block, 0, st, d_tiles, n_tiles, d_tile_off, d_tile_carry, d_tot);
  WP_LAUNCH_CHECK();
  unsigned long long *h_tot = reinterpret_cast<unsigned long long *>(c->h_scalars + kScalarDetok);
  WP_HIP(hipMemcpyAsync(h_tot, d_tot, kDetokCounters * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  WP_HIP(hipStreamSynchronize(st));
  const unsigned long long total = h_tot[kDetokBytes] + (g.term >= 0 ? static_cast<unsigned long long>(n_rows) : 0ull);
  if (total >= (1ull << 32)) throw std::length_error("detokenize: the text has 2^32 bytes or more");
  g.n_bytes = total;
  // text_off | text (a whole number of words)
  const size_t off_text = up256((n_rows + 1) * sizeof(long long));
  c->detok_out.ensure(off_text + up256(static_cast<size_t>(total) + 4));
  long long *d_off = static_cast<long long *>(c->detok_out.p);
  uint8_t *d_txt = static_cast<uint8_t *>(c->detok_out.p) + off_text;
  hipLaunchKernelGGL((detok_tile_kernel<true>), grid, block, 0, st, d_ids, d_splits, d_lengths, g, d_rec, c->d_detok_pool,
                     static_cast<DetokTile *>(nullptr), d_tile_off, d_tile_carry, d_txt, d_off);
  WP_LAUNCH_CHECK();
  WP_HIP(hipStreamSynchronize(st));
#ifdef WP_DEBUG_BOUNDS
  {
    unsigned int oob = 0;
    take_oob(kSiteDetok, 1, &oob);
    if (oob != 0) throw HipError("debug bounds: detokenize: " + std::to_string(oob) + " gathers or stores outside their buffers skipped");
  }
#endif
  ds.n_kept = static_cast<int64_t>(h_tot[kDetokKept]);
  ds.n_skipped = static_cast<int64_t>(h_tot[kDetokSkipped]);
  ds.n_dropped = static_cast<int64_t>(h_tot[kDetokDropped]);
  ds.n_cells = ds.n_kept + ds.n_skipped + ds.n_dropped;
  ds.n_bytes = static_cast<int64_t>(total);
  *d_text = total ? d_txt : nullptr;
  *d_text_off = d_off;
  *n_bytes = static_cast<size_t>(total);
}
}  // namespace

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
      if (row_splits[0] != 0) throw std::invalid_argument("detokenize: row_splits must start at 0");
      for (size_t r = 0; r < n_rows; r++) {
        if (row_splits[r + 1] < row_splits[r]) throw std::invalid_argument("detokenize: row_splits must never descend");
      }
      if (row_splits[n_rows] > INT32_MAX) throw std::length_error("detokenize: more cells than INT32_MAX");
      g.n_cells = row_splits[n_rows];
    }
    if (g.n_cells > 0 && !ids) throw std::invalid_argument("detokenize: ids is NULL");
    if (n_rows == 0) {
      int64_t *off = static_cast<int64_t *>(std::calloc(1, sizeof(int64_t)));
      if (!off) throw std::bad_alloc();
      *text_off = off;
      begin_detok_stats(v, 0);
      return;
    }
    Context *c = get_context(v);
    const size_t n_cells = static_cast<size_t>(g.n_cells);
    const bool ragged = g.max_len == 0;
    // ids | row_splits or lengths
    const size_t off_rows = up256(n_cells * sizeof(int32_t));
    c->detok_in.ensure(off_rows + up256((n_rows + 1) * sizeof(int64_t)));
    int32_t *d_ids = static_cast<int32_t *>(c->detok_in.p);
    void *d_rows = static_cast<char *>(c->detok_in.p) + off_rows;
    if (n_cells) WP_HIP(hipMemcpyAsync(d_ids, ids, n_cells * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    if (ragged) {
      WP_HIP(hipMemcpyAsync(d_rows, row_splits, (n_rows + 1) * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    } else if (lengths) {
      WP_HIP(hipMemcpyAsync(d_rows, lengths, n_rows * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    }
    const void *d_text = nullptr;
    const long long *d_off = nullptr;
    size_t nb = 0;
    detok_on_device(v, c, d_ids, ragged ? static_cast<const long long *>(d_rows) : nullptr,
                    !ragged && lengths ? static_cast<const int32_t *>(d_rows) : nullptr, g, spec->cleanup, &d_text, &d_off, &nb);
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
    if ((reinterpret_cast<uintptr_t>(d_ids) & 3u) != 0 || (reinterpret_cast<uintptr_t>(d_lengths) & 3u) != 0 ||
        (reinterpret_cast<uintptr_t>(d_row_splits) & 7u) != 0) {
      throw std::invalid_argument("detokenize: device ids and lengths must be 4-byte aligned, row_splits 8-byte aligned");
    }
    const long long *d_off = nullptr;
    detok_on_device(v, get_context(v), d_ids, g.max_len == 0 ? reinterpret_cast<const long long *>(d_row_splits) : nullptr,
                    g.max_len == 0 ? nullptr : d_lengths, g, spec->cleanup, d_text, &d_off, n_bytes);
    *d_text_off = reinterpret_cast<const int64_t *>(d_off);
  });
}

}  // extern "C"

// ---- pack (include/wordpiece_amd.h, section "pack"; kernels: packing.h) ---------------------------------------------
namespace {
// every argument rule that needs neither the rows nor a device
PackGeom check_pack_spec(const wp_pack_spec *spec, size_t n_docs) {
  if (!spec) throw std::invalid_argument("pack: spec is NULL");
  if (spec->mode != WP_PACK_NEXT_FIT && spec->mode != WP_PACK_STREAM) throw std::invalid_argument("pack: unknown mode");
  if (spec->mode == WP_PACK_NEXT_FIT && spec->long_docs != WP_PACK_LONG_TRUNCATE && spec->long_docs != WP_PACK_LONG_SPLIT) {
    throw std::invalid_argument("pack: unknown long_docs");
  }
  if ((spec->want & ~7) != 0) throw std::invalid_argument("pack: want has bits outside 7");
  if (spec->max_len < 1) throw std::invalid_argument("pack: max_len must be at least 1");
  const int specials = (spec->bos_id >= 0 ? 1 : 0) + (spec->eos_id >= 0 ? 1 : 0);
  if (spec->max_len - specials < 1) throw std::invalid_argument("pack: max_len leaves no room for an id beside the specials");
  if (n_docs > static_cast<size_t>(INT32_MAX)) throw std::length_error("pack: more documents than INT32_MAX");
  PackGeom g{};
  g.max_len = spec->max_len;
  g.budget = spec->max_len - specials;
  g.stream = spec->mode == WP_PACK_STREAM;
  g.split = !g.stream && spec->long_docs == WP_PACK_LONG_SPLIT;
  g.bos_id = spec->bos_id;
  g.eos_id = spec->eos_id;
  g.pad_id = spec->pad_id;
  g.want = spec->want;
  return g;
}

wp_pack_stats &begin_pack_stats(wp_vocab *v, size_t n_docs) {
  v->stats.pack_call = 1;
  v->stats.pack = wp_pack_stats{};
  v->stats.pack.n_docs = static_cast<int64_t>(n_docs);
  return v->stats.pack;
}

void check_pack_totals(unsigned long long n_ids, unsigned long long n_cells) {
  if (n_ids > static_cast<unsigned long long>(INT32_MAX)) throw std::length_error("pack: more ids than INT32_MAX");
  if (n_cells > static_cast<unsigned long long>(INT32_MAX)) throw std::length_error("pack: more cells in the units than INT32_MAX");
}
void check_pack_rows(unsigned long long n_out, int max_len) {
  if (n_out * static_cast<unsigned long long>(max_len) > static_cast<unsigned long long>(INT32_MAX)) {
    throw std::length_error("pack: n_out * max_len exceeds INT32_MAX");
  }
}

// The passes over device buffers on c's stream; the row_splits are checked here in a kernel.  out_for(n_out): the
// buffers of the batch once the number of rows is known (throws where there is no room); not called for n_out == 0.
// Returns n_out.  Nothing is written through the caller's pointers before every check has passed.
template <typename OutFor>
size_t pack_on_device(wp_vocab *v, Context *c, const int32_t *d_ids, const long long *d_splits, size_t n_docs, PackGeom g, OutFor &&out_for) {
  wp_pack_stats &ps = begin_pack_stats(v, n_docs);
  if (n_docs == 0) return 0;
  hipStream_t st = c->stream;
  const dim3 block(kBlock);
  // pieces | cells per document, scanned in place | the scans' tile sums
  const size_t scan_tmp = up256((cdiv(n_docs, kScanTile) + 1) * sizeof(uint32_t));
  const size_t off_cells = up256(n_docs * sizeof(uint32_t)), off_tmp = 2 * off_cells;
  c->pack_plan.ensure(off_tmp + scan_tmp);
  char *plan = static_cast<char *>(c->pack_plan.p);
  uint32_t *d_piece_base = reinterpret_cast<uint32_t *>(plan), *d_cell_base = reinterpret_cast<uint32_t *>(plan + off_cells);
  uint32_t *d_scan_tmp = reinterpret_cast<uint32_t *>(plan + off_tmp);
  unsigned long long *d_tot = reinterpret_cast<unsigned long long *>(c->d_scalars + kScalarPack);
  const unsigned long long *h_tot = reinterpret_cast<const unsigned long long *>(c->h_scalars + kScalarPack);
  clear_scalars(c, kScalarPackLast, kScalarPack, st);
  hipLaunchKernelGGL(detok_check_splits_kernel, dim3(std::min<unsigned>(cdiv(n_docs + 1, kBlock), 1024u)), block, 0, st, d_splits, n_docs,
                     c->d_scalars + kScalarPackBad, reinterpret_cast<long long *>(c->d_scalars + kScalarPackLast));
  hipLaunchKernelGGL(seqpack_plan_kernel, dim3(std::min<unsigned>(cdiv(n_docs, kBlock), kPackMaxGrid)), block, 0, st, d_splits, n_docs, g,
                     d_piece_base, d_cell_base, d_tot);
  WP_LAUNCH_CHECK();
  queue_scalar_slots(c, kScalarPackLast, kScalarPack, st);
  WP_HIP(hipStreamSynchronize(st));
  if (c->h_scalars[kScalarPackBad] != 0) throw std::invalid_argument("pack: row_splits must start at 0 and never descend");
  long long last;
  std::memcpy(&last, c->h_scalars + kScalarPackLast, sizeof(last));
  check_pack_totals(static_cast<unsigned long long>(last), h_tot[kPackStream]);
  if (last > 0 && !d_ids) throw std::invalid_argument("pack: ids is NULL");
  ps.n_empty = static_cast<int64_t>(h_tot[kPackEmpty]);
  ps.n_cut = static_cast<int64_t>(h_tot[kPackCut]);
  ps.n_ids_cut = static_cast<int64_t>(h_tot[kPackIdsCut]);
  ps.n_pieces = static_cast<int64_t>(h_tot[kPackPieces]);
  g.n_ids = static_cast<uint32_t>(last);
  g.n_cells = static_cast<uint32_t>(h_tot[kPackStream]);
  g.n_pieces = static_cast<uint32_t>(h_tot[kPackPieces]);  // (every unit holds a cell: n_pieces <= n_cells)
  if (g.n_pieces == 0) return 0;
  const size_t n_p = g.n_pieces, n_tiles = cdiv(n_p, kPackPieceTile);
  // P | src0 | nx | row_first | tile_entry | tile_row | records
  const size_t per_piece = up256((n_p + 1) * sizeof(uint32_t)), per_tile = up256(n_tiles * sizeof(uint32_t));
  const size_t off_entry = 4 * per_piece, off_rec = off_entry + 2 * per_tile;
  c->pack_tab.ensure(off_rec + up256(n_p * sizeof(unsigned long long)));
  char *tab = static_cast<char *>(c->pack_tab.p);
  uint32_t *d_P = reinterpret_cast<uint32_t *>(tab), *d_nx = reinterpret_cast<uint32_t *>(tab + 2 * per_piece);
  int32_t *d_src0 = reinterpret_cast<int32_t *>(tab + per_piece);
  uint32_t *d_row_first = reinterpret_cast<uint32_t *>(tab + 3 * per_piece);
  uint32_t *d_tile_entry = reinterpret_cast<uint32_t *>(tab + off_entry), *d_tile_row = reinterpret_cast<uint32_t *>(tab + off_entry + per_tile);
  unsigned long long *d_rec = reinterpret_cast<unsigned long long *>(tab + off_rec);
  device_exclusive_scan(d_piece_base, d_piece_base, n_docs, d_scan_tmp, nullptr, st);
  device_exclusive_scan(d_cell_base, d_cell_base, n_docs, d_scan_tmp, nullptr, st);
  hipLaunchKernelGGL(seqpack_pieces_kernel, dim3(cdiv(n_p, kBlock)), block, 0, st, d_splits, static_cast<uint32_t>(n_docs), d_piece_base,
                     d_cell_base, g, d_P, d_src0);
  WP_LAUNCH_CHECK();
  unsigned long long n_out = (static_cast<unsigned long long>(g.n_cells) + g.max_len - 1) / static_cast<unsigned long long>(g.max_len);
  if (!g.stream) {
    WP_HIP(hipMemsetAsync(d_tile_entry, 0xFF, n_tiles * sizeof(uint32_t), st));
    hipLaunchKernelGGL(seqpack_tile_kernel, dim3(static_cast<unsigned>(n_tiles)), block, 0, st, d_P, g.n_pieces, static_cast<uint32_t>(g.max_len),
                       d_nx, d_rec);
    hipLaunchKernelGGL(seqpack_spine_kernel, dim3(1), dim3(kWave), 0, st, d_rec, g.n_pieces, d_tile_entry, d_tile_row, d_row_first, d_tot);
    WP_LAUNCH_CHECK();
    queue_scalar_slots(c, kScalarPack, kScalarPack, st);
    WP_HIP(hipStreamSynchronize(st));
    n_out = h_tot[kPackRows];
  }
  ps.n_out = static_cast<int64_t>(n_out);
  check_pack_rows(n_out, g.max_len);
  g.n_out = static_cast<uint32_t>(n_out);
  const PackOut o = out_for(static_cast<size_t>(n_out));
  if (!g.stream) {
    hipLaunchKernelGGL(seqpack_apply_kernel, dim3(static_cast<unsigned>(n_tiles)), block, 0, st, d_nx, g.n_pieces, static_cast<uint32_t>(g.max_len),
                       d_tile_entry, d_tile_row, d_row_first);
  }
  const size_t cell_tiles = cdiv(static_cast<size_t>(n_out) * static_cast<size_t>(g.max_len), kPackCellTile);
  hipLaunchKernelGGL(seqpack_write_kernel, dim3(static_cast<unsigned>(std::min<size_t>(cell_tiles, kPackMaxGrid))), block, 0, st, d_ids, d_P,
                     d_src0, d_row_first, g, o, d_tot);
  WP_LAUNCH_CHECK();
  queue_scalar_slots(c, kScalarPack, kScalarPack, st);
  WP_HIP(hipStreamSynchronize(st));
#ifdef WP_DEBUG_BOUNDS
  {
    unsigned int oob = 0;
    take_oob(kSitePack, 1, &oob);
    if (oob != 0) throw HipError("debug bounds: pack: " + std::to_string(oob) + " gathers or stores outside their buffers skipped");
  }
#endif
  ps.n_cells = static_cast<int64_t>(h_tot[kPackCells]);
  ps.n_segments = static_cast<int64_t>(h_tot[kPackSegments]);
  return static_cast<size_t>(n_out);
}
}  // namespace

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
    if (row_splits[0] != 0) throw std::invalid_argument("pack: row_splits must start at 0");
    const unsigned long long s = static_cast<unsigned long long>(g.max_len - g.budget), B = static_cast<unsigned long long>(g.budget);
    unsigned long long n_cells = 0, n_pieces = 0, n_empty = 0;
    for (size_t r = 0; r < n_docs; r++) {
      if (row_splits[r + 1] < row_splits[r]) throw std::invalid_argument("pack: row_splits must never descend");
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
    const size_t n_ids = static_cast<size_t>(row_splits[n_docs]);
    check_pack_totals(n_ids, n_cells);
    if (g.stream) check_pack_rows((n_cells + g.max_len - 1) / static_cast<unsigned long long>(g.max_len), g.max_len);
    if (n_ids > 0 && !ids) throw std::invalid_argument("pack: ids is NULL");
    if (n_pieces == 0) {  // no document, or empty ones only: no device
      begin_pack_stats(v, n_docs).n_empty = static_cast<int64_t>(n_empty);
      return;
    }
    Context *c = get_context(v);
    // ids | row_splits
    const size_t off_rows = up256(n_ids * sizeof(int32_t));
    c->pack_in.ensure(off_rows + up256((n_docs + 1) * sizeof(int64_t)));
    int32_t *d_ids = static_cast<int32_t *>(c->pack_in.p);
    long long *d_rows = reinterpret_cast<long long *>(static_cast<char *>(c->pack_in.p) + off_rows);
    WP_HIP(hipMemcpyAsync(d_ids, ids, n_ids * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    WP_HIP(hipMemcpyAsync(d_rows, row_splits, (n_docs + 1) * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    PackOut o{};
    const size_t rows = pack_on_device(v, c, d_ids, d_rows, n_docs, g, [&](size_t n) {
      // input_ids | segment_ids | position_ids | source | lengths
      const size_t block = up256(n * static_cast<size_t>(g.max_len) * sizeof(int32_t));
      c->pack_out.ensure(4 * block + up256(n * sizeof(int32_t)));
      char *p = static_cast<char *>(c->pack_out.p);
      o = PackOut{reinterpret_cast<int32_t *>(p), reinterpret_cast<int32_t *>(p + block), reinterpret_cast<int32_t *>(p + 2 * block),
                  reinterpret_cast<int32_t *>(p + 3 * block), reinterpret_cast<int32_t *>(p + 4 * block)};
      return o;
    });
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
    for (const void *p : {static_cast<const void *>(d_ids), static_cast<const void *>(o.input_ids), static_cast<const void *>(o.segment_ids),
                          static_cast<const void *>(o.position_ids), static_cast<const void *>(o.source), static_cast<const void *>(o.lengths)}) {
      if ((reinterpret_cast<uintptr_t>(p) & 3u) != 0) throw std::invalid_argument("pack: device ids and outputs must be 4-byte aligned");
    }
    if ((reinterpret_cast<uintptr_t>(d_row_splits) & 7u) != 0) throw std::invalid_argument("pack: device row_splits must be 8-byte aligned");
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

// ---- model inputs (include/wordpiece_amd.h, section "model inputs"; kernels: inputs.h) -------------------------------
namespace {
// every argument rule that needs neither the text nor a device
InputsGeom check_inputs_spec(const wp_inputs_spec *spec, size_t nbytes) {
  if (!spec) throw std::invalid_argument("inputs: spec is NULL");
  check_rows_call(spec->unit, nbytes);
  if (spec->truncation != WP_TRUNC_LONGEST_FIRST && spec->truncation != WP_TRUNC_ONLY_FIRST && spec->truncation != WP_TRUNC_ONLY_SECOND) {
    throw std::invalid_argument("inputs: unknown truncation strategy");
  }
  if (spec->stride < -1) throw std::invalid_argument("inputs: stride must be -1 (no windows) or at least 0");
  if (spec->pairs != 0 && spec->pairs != 1) throw std::invalid_argument("inputs: pairs must be 0 or 1");
  InputsGeom g;
  g.max_len = spec->max_len;
  g.head = spec->cls_id >= 0 ? 1 : 0;
  g.nsep = spec->sep_id >= 0 ? 1 : 0;
  const int specials = g.head + g.nsep * (spec->pairs ? 2 : 1);
  if (spec->max_len < 1 || spec->max_len < specials) {
    throw std::invalid_argument("max_len must be at least 1 and at least the number of specials");
  }
  g.budget = spec->max_len - specials;
  g.pairs = spec->pairs;
  g.truncation = spec->truncation;
  g.stride = spec->stride;
  g.cls_id = spec->cls_id;
  g.sep_id = spec->sep_id;
  g.pad_id = spec->pad_id;
  if (spec->truncation == WP_TRUNC_LONGEST_FIRST) {
    if (spec->stride >= 0) throw std::invalid_argument("inputs: windows (stride >= 0) need the truncation only_first or only_second");
  } else {
    if (spec->truncation == WP_TRUNC_ONLY_SECOND && !spec->pairs) throw std::invalid_argument("inputs: only_second needs pairs");
    if (static_cast<long long>(g.budget) < static_cast<long long>(std::max(spec->stride, 0)) + 1) {
      throw std::invalid_argument("inputs: max_len leaves no room for a window");
    }
  }
  return g;
}

void check_inputs_rows(const InputsGeom &g, size_t n_rows) {
  if (g.pairs && (n_rows & 1) != 0) throw std::invalid_argument("inputs: pairs need an even number of rows");
}

// n_out * max_len cells of 8 bytes must be addressable
void check_inputs_size(size_t n_out, int max_len) {
  if (n_out > static_cast<size_t>(UINT32_MAX) || n_out > SIZE_MAX / 8 / static_cast<size_t>(max_len)) {
    throw std::length_error("inputs: too many output rows");
  }
}

// The model inputs of a rows result.  place(n_out) names the buffers of the batch once the number of output rows is
// known (and throws where they do not fit); returns n_out.  Waits for the batch.  Without windows the host waits once,
// behind the packer (as pack_on_device does); with windows once more, for the row count.
size_t inputs_on_device(wp_vocab *v, Context *c, const RowsResult &r, const InputsGeom &g, int unit,
                        const std::function<wp_inputs(size_t)> &place) {
  hipStream_t st = c->stream;
  const size_t n_samples = r.n_rows / (g.pairs ? 2 : 1);
  v->stats.rows_truncated = 0;
  v->stats.inputs_call = 1;
  wp_inputs_stats &is = v->stats.inputs;
  is = wp_inputs_stats{};
  is.n_samples = static_cast<int64_t>(n_samples);
  is.pairs = g.pairs;
  is.truncation = g.truncation;
  is.stride = g.stride;
  if (n_samples > static_cast<size_t>(INT32_MAX)) throw std::length_error("inputs: too many samples");
  if (n_samples == 0) {
    (void)place(0);
    return 0;
  }
  const bool windows = g.stride >= 0;
  // scratch: a record per sample | window counts (scanned in place) | the scan's tile sums
  const size_t scan_words = cdiv(n_samples, kScanTile) + 8;
  c->inputs_buf.ensure(n_samples * sizeof(InputsRec) + (n_samples + scan_words) * sizeof(uint32_t));
  InputsRec *d_rec = static_cast<InputsRec *>(c->inputs_buf.p);
  uint32_t *d_win = reinterpret_cast<uint32_t *>(d_rec + n_samples), *d_tmp = d_win + n_samples;
  clear_scalars(c, kScalarInCut, kScalarInWindowed, st);
  hipLaunchKernelGGL(inputs_plan_kernel, dim3(cdiv(n_samples, kBlock)), dim3(kBlock), 0, st, r.d_row_splits, n_samples, g, d_win, d_rec,
                     c->d_scalars + kScalarInCut, c->d_scalars + kScalarInWindowed);
  WP_LAUNCH_CHECK();
  size_t n_out = n_samples;
  if (windows) {
    device_exclusive_scan(d_win, d_win, n_samples, d_tmp, nullptr, st, nullptr,
                          reinterpret_cast<unsigned long long *>(c->d_scalars + kScalarInRows));
    fetch_scalars(c, kScalarInWindowed);
    unsigned long long total;
    std::memcpy(&total, c->h_scalars + kScalarInRows, sizeof(total));
    if (total > static_cast<unsigned long long>(UINT32_MAX)) throw std::length_error("inputs: too many output rows");
    n_out = static_cast<size_t>(total);
  }
  check_inputs_size(n_out, g.max_len);
  is.n_out = static_cast<int64_t>(n_out);
  const wp_inputs o = place(n_out);
  const int lanes = lanes_for(g.max_len);
  hipLaunchKernelGGL(inputs_pack_kernel, dim3(cdiv(n_out, static_cast<size_t>(kBlock / lanes))), dim3(kBlock), 0, st, r.d_ids,
                     reinterpret_cast<const uint2 *>(r.d_offs), r.n_ids, r.d_row_splits, static_cast<const InputsRec *>(d_rec),
                     windows ? static_cast<const uint32_t *>(d_win) : nullptr, n_samples, n_out, g, lanes, o.input_ids, o.token_type_ids,
                     unit >= 0 ? reinterpret_cast<uint2 *>(o.offsets) : nullptr, o.lengths, o.sample);
  WP_LAUNCH_CHECK();
  if (windows) {
    WP_HIP(hipStreamSynchronize(st));
  } else {
    fetch_scalars(c, kScalarInWindowed);
  }
#ifdef WP_DEBUG_BOUNDS
  {
    unsigned int oob = 0;
    take_oob(kSiteInputs, 1, &oob);
    if (oob != 0) throw HipError("debug bounds: model inputs: " + std::to_string(oob) + " gathers outside the id list skipped");
  }
#endif
  is.n_cut = c->h_scalars[kScalarInCut];
  is.n_windowed = c->h_scalars[kScalarInWindowed];
  return n_out;
}

size_t count_lines_host(const char *utf8, size_t nbytes) {
  if (nbytes == 0) return 0;
  size_t n = utf8[nbytes - 1] != '\n' ? 1 : 0;
  for (const char *p = utf8, *end = utf8 + nbytes; (p = static_cast<const char *>(std::memchr(p, '\n', end - p))) != nullptr; p++) n++;
  return n;
}
}  // namespace

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
    size_t cells = 0;
    wp_inputs o{};  // the batch in c->pad_buf
    const size_t n = inputs_on_device(v, c, r, g, unit, [&](size_t rows_out) {
      cells = rows_out * max_len;  // offsets | input_ids | token_type_ids | lengths | sample
      const size_t offs_bytes = unit >= 0 ? cells * 2 * sizeof(uint32_t) : 0;
      c->pad_buf.ensure(offs_bytes + (2 * cells + 2 * rows_out) * sizeof(int32_t) + 16);
      char *base = static_cast<char *>(c->pad_buf.p);
      o.offsets = unit >= 0 ? reinterpret_cast<uint32_t *>(base) : nullptr;
      o.input_ids = reinterpret_cast<int32_t *>(base + offs_bytes);
      o.token_type_ids = o.input_ids + cells;
      o.lengths = o.token_type_ids + cells;
      o.sample = o.lengths + rows_out;
      return o;
    });
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
    if ((reinterpret_cast<uintptr_t>(d_out->offsets) & 7u) != 0) throw std::invalid_argument("the offsets buffer must be 8-byte aligned");
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
    // arenas as an encode of `nbytes` of ASCII text would size them in the default layout (43
    // bytes per symbol + the refinement list for an eighth of the text; an estimate — an encode that needs more,
    // a larger alphabet or the reference layout, grows them as before)
    const size_t n = nbytes + 1 + v->hv.stream.size();
    const size_t per_symbol = (v->keep_debug || v->vocab_in_s || v->full_depth) ? 108 : 56;
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
      case 2: src = d.rank; break;
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
