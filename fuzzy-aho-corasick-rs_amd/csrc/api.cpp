// api.cpp — the extern "C" boundary declared in include/fac.h.
//
// fac_search_raw is the drop-in for FuzzyAhoCorasick::search_raw (src/search.rs:187-395):
// host staging (is_ascii + grapheme segmentation/folding, :196-203 / :296-302), then the GPU
// window kernel over every start position. fac_search_prefiltered is the drop-in for
// Prefiltered::raw (src/prefilter.rs:146-155, 304-374): k_for on the host, the bitap scan and the
// window merge on the GPU, then the window kernel over the merged slices. There is no CPU search
// path: without a usable gfx950 device every search entry point returns FAC_E_NO_DEVICE.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <new>
#include <string>
#include <thread>
#include <tuple>

#include "fac_internal.h"
#include "host_util.h"

struct fac_engine {
  fac::Engine e;
};
struct fac_haystack {
  fac::Haystack h;
};
struct fac_stream {
  fac::StreamCore* s = nullptr;
};
struct fac_replace_stream {
  fac::StreamCore* s = nullptr;
};
struct fac_batch {
  fac::Batch b;
};
struct fac_replacements {
  fac::ReplaceTable t;
};

namespace fac {

const char* diag_env(const char* name) {
  static const bool on = [] {
    const char* d = std::getenv("FAC_DIAGNOSTICS");
    return d && *d && std::strcmp(d, "0") != 0;
  }();
  return on ? std::getenv(name) : nullptr;
}

uint64_t grapheme_limit() {
  const char* v = diag_env("FAC_GRAPHEME_LIMIT");
  return v ? std::strtoull(v, nullptr, 10) : 0xFFFFFFFFull;
}

namespace {
// Result buffers handed across the C ABI. A search's records are copied D2H straight into the
// buffer the caller receives; buffers of >= 1 MiB are pinned and go back to this pool on
// fac_matches_free, so repeated searches land their records in already-mapped, already-pinned
// pages (a fresh malloc'd buffer faults every page on first touch: C2's 72 MB of records per call
// cost 20-40 ms of page faults, varying by box).
struct PoolBlock {
  void* p;
  uint64_t bytes;
  bool used;
};
std::mutex g_pool_mu;
std::vector<PoolBlock> g_pool;
constexpr uint64_t kPinnedMin = 1ull << 20;
constexpr uint64_t kPoolKeep = 4ull << 30;  // pinned bytes kept while unused
}  // namespace

fac_match* result_alloc(uint64_t n_records) {
  const uint64_t bytes = std::max<uint64_t>(n_records, 1) * sizeof(fac_match);
  if (bytes < kPinnedMin) return static_cast<fac_match*>(std::malloc(bytes));
  std::lock_guard<std::mutex> g(g_pool_mu);
  PoolBlock* best = nullptr;
  for (PoolBlock& b : g_pool)
    if (!b.used && b.bytes >= bytes && b.bytes <= 4 * bytes && (!best || b.bytes < best->bytes)) best = &b;
  if (best) {
    best->used = true;
    return static_cast<fac_match*>(best->p);
  }
  const uint64_t want = bytes + bytes / 4;  // headroom: the next call's count differs a little
  void* p = nullptr;
  if (hipHostMalloc(&p, want, hipHostMallocDefault) != hipSuccess || !p)
    return static_cast<fac_match*>(std::malloc(bytes));  // unpinned: result_free recognises it
  g_pool.push_back({p, want, true});
  return static_cast<fac_match*>(p);
}

void result_free(void* p) {
  if (!p) return;
  {
    std::lock_guard<std::mutex> g(g_pool_mu);
    for (size_t i = 0; i < g_pool.size(); ++i)
      if (g_pool[i].p == p) {
        g_pool[i].used = false;
        uint64_t idle = 0;
        for (const PoolBlock& b : g_pool)
          if (!b.used) idle += b.bytes;
        // trim the largest idle blocks beyond the keep budget
        while (idle > kPoolKeep) {
          size_t big = g_pool.size();
          for (size_t k = 0; k < g_pool.size(); ++k)
            if (!g_pool[k].used && (big == g_pool.size() || g_pool[k].bytes > g_pool[big].bytes)) big = k;
          if (big == g_pool.size()) break;
          (void)hipHostFree(g_pool[big].p);
          idle -= g_pool[big].bytes;
          g_pool.erase(g_pool.begin() + (std::ptrdiff_t)big);
        }
        return;
      }
  }
  std::free(p);
}

namespace {
int grow_pinned(MatchSink& s, uint64_t need, std::string& err) {
  if (need <= s.pinned_cap) return FAC_OK;
  const uint64_t cap = std::max<uint64_t>(need, 2 * s.pinned_cap);
  fac_match* p = result_alloc(cap);
  if (!p) {
    err = "out of host memory";
    return FAC_E_OOM;
  }
  if (s.n) std::memcpy(p, s.pinned, s.n * sizeof(fac_match));
  result_free(s.pinned);
  s.pinned = p;
  s.pinned_cap = cap;
  return FAC_OK;
}
}  // namespace

int sink_append_device(MatchSink& s, const fac_match* d_src, uint64_t cnt, hipStream_t stream, std::string& err) {
  if (!cnt) return FAC_OK;
  hipError_t he = hipSuccess;
  if (s.dev) {
    const uint64_t fit = s.n >= s.dev_cap ? 0 : std::min(cnt, s.dev_cap - s.n);
    if (fit) he = hipMemcpyAsync(s.dev + s.n, d_src, fit * sizeof(fac_match), hipMemcpyDeviceToDevice, stream);
  } else if (s.vec) {
    s.vec->resize(s.n + cnt);
    he = hipMemcpyAsync(s.vec->data() + s.n, d_src, cnt * sizeof(fac_match), hipMemcpyDeviceToHost, stream);
    if (he == hipSuccess) he = hipStreamSynchronize(stream);  // pageable destination
  } else {
    if (int rc = grow_pinned(s, s.n + cnt, err)) return rc;
    he = hipMemcpyAsync(s.pinned + s.n, d_src, cnt * sizeof(fac_match), hipMemcpyDeviceToHost, stream);
  }
  if (he != hipSuccess) {
    err = std::string("record copy: ") + hipGetErrorString(he);
    return FAC_E_HIP;
  }
  s.n += cnt;
  return FAC_OK;
}

int sink_append_host(MatchSink& s, const fac_match* src, uint64_t cnt, hipStream_t stream, std::string& err) {
  if (!cnt) return FAC_OK;
  if (s.dev) {
    const uint64_t fit = s.n >= s.dev_cap ? 0 : std::min(cnt, s.dev_cap - s.n);
    if (fit) {
      hipError_t he = hipMemcpyAsync(s.dev + s.n, src, fit * sizeof(fac_match), hipMemcpyHostToDevice, stream);
      if (he == hipSuccess) he = hipStreamSynchronize(stream);  // pageable source
      if (he != hipSuccess) {
        err = std::string("record copy: ") + hipGetErrorString(he);
        return FAC_E_HIP;
      }
    }
  } else if (s.vec) {
    s.vec->resize(s.n + cnt);
    std::memcpy(s.vec->data() + s.n, src, cnt * sizeof(fac_match));
  } else {
    if (int rc = grow_pinned(s, s.n + cnt, err)) return rc;
    std::memcpy(s.pinned + s.n, src, cnt * sizeof(fac_match));
  }
  s.n += cnt;
  return FAC_OK;
}

}  // namespace fac

namespace {

thread_local std::string g_err;

int fail(int rc, const std::string& msg) {
  g_err = msg;
  return rc;
}

// hands a pinned sink's buffer to the C ABI caller (freed by fac_matches_free)
int hand_out(fac::MatchSink& s, fac_match** out, uint64_t* n_out) {
  if (!s.pinned) {
    s.pinned = fac::result_alloc(1);
    if (!s.pinned) return fail(FAC_E_OOM, "out of host memory");
  }
  *out = s.pinned;
  *n_out = s.n;
  s.pinned = nullptr;
  return FAC_OK;
}

int check_device(int device) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count == 0)
    return fail(FAC_E_NO_DEVICE, "no HIP device available (the engine has no CPU fallback)");
  if (device < 0 || device >= count) return fail(FAC_E_NO_DEVICE, "device ordinal out of range");
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) return fail(FAC_E_HIP, "hipGetDeviceProperties failed");
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(FAC_E_NO_DEVICE, std::string("kernels are built for gfx950, device is ") + prop.gcnArchName);
  return FAC_OK;
}

int copy_out(const std::vector<fac_match>& v, fac_match** out, uint64_t* n_out) {
  *n_out = v.size();
  *out = static_cast<fac_match*>(std::malloc(std::max<size_t>(v.size(), 1) * sizeof(fac_match)));
  if (!*out) return fail(FAC_E_OOM, "out of host memory");
  if (!v.empty()) std::memcpy(*out, v.data(), v.size() * sizeof(fac_match));
  return FAC_OK;
}

// The staged haystack as search_raw's text: a shard whose text continues past its resident halo
// (open_end) has no end inside the resident bytes (the kernels flag any window that would read
// past them), and only its owned start windows are searched.
constexpr uint64_t kOpenEnd = 1ull << 62;
fac::SegDesc whole(const fac::Haystack& h) {
  fac::SegDesc s{};
  s.text_base = 0;
  s.n = h.open_end ? kOpenEnd : h.n;
  s.avail = h.n;
  s.hay_len = h.open_end ? kOpenEnd : h.len;
  s.byte_base = 0;
  s.w_begin = 0;
  s.w_end = std::min(h.n, h.owned);
  s.ascii = h.ascii ? 1u : 0u;
  return s;
}

// k_for (prefilter.rs:285-302). Returns false if some pattern needs k > 24 (full-search fallback).
bool prefilter_ks(const fac::Engine& e, float threshold, std::vector<uint32_t>& ks) {
  ks.clear();
  for (size_t i = 0; i < e.bp_m.size(); ++i) {
    const float nf = (float)e.bp_m[i];
    volatile float ratio = threshold / e.bp_weight[i];
    volatile float p_max = nf * (1.0f - ratio);
    uint64_t k_pen;
    if (p_max <= 0.0f) {
      k_pen = 0;
    } else {
      volatile float prod = p_max * e.edit_cost_mult;
      const float kf = std::floor((float)prod);
      if (std::isnan(kf)) k_pen = 0;  // Rust `as usize` saturates; NaN -> 0
      else if (kf >= 1.8446744e19f) k_pen = UINT64_MAX;
      else k_pen = (uint64_t)kf;
    }
    uint64_t k = e.bp_k_limit[i] >= 0 ? std::min<uint64_t>(k_pen, (uint64_t)e.bp_k_limit[i]) : k_pen;
    if (k > 24) return false;
    ks.push_back((uint32_t)k);
  }
  return true;
}

int search_staged_all(const fac::Engine& e, const fac::Haystack& h, float thr, hipStream_t stream,
                      fac::MatchSink& res, fac_stats* stats) {
  std::string err;
  std::vector<fac::SegDesc> segs{whole(h)};
  int rc = fac::launch_search_sink(e, h, segs, thr, stream, 0, res, stats, err);
  if (rc) return fail(rc, err);
  return FAC_OK;
}

}  // namespace

extern "C" {

const char* fac_last_error(void) { return g_err.c_str(); }

int fac_build(const fac_pattern* patterns, uint64_t n_patterns, const fac_config* cfg, fac_engine** out) {
  if (!out || !cfg || (n_patterns && !patterns)) return fail(FAC_E_INVALID, "NULL argument");
  *out = nullptr;
  if (cfg->beam_width == 0 && cfg->has_auto_beam && cfg->auto_beam_width == 0)
    return fail(FAC_E_INVALID, "auto_beam width must be >= 1");
  int rc = check_device(cfg->device);
  if (rc) return rc;
  fac_engine* fe = new (std::nothrow) fac_engine();
  if (!fe) return fail(FAC_E_OOM, "out of host memory");
  std::string err;
  rc = fac::build_engine(patterns, n_patterns, cfg, fe->e, err);
  if (!rc) rc = fac::upload_engine(fe->e, err);
  if (rc) {
    fac::free_engine_device(fe->e);
    delete fe;
    return fail(rc, err);
  }
  *out = fe;
  return FAC_OK;
}

void fac_engine_free(fac_engine* engine) {
  if (!engine) return;
  fac::free_engine_device(engine->e);
  delete engine;
  fac::call_scratch_trim();  // the kept call scratch is invisible to callers' allocators
}

void fac_trim_scratch(void) { fac::call_scratch_trim(); }

uint64_t fac_engine_num_nodes(const fac_engine* engine) { return engine ? engine->e.nodes.size() : 0; }
uint32_t fac_engine_max_edits_fast(const fac_engine* engine) { return engine ? engine->e.max_edits_fast : 0; }
uint64_t fac_max_match_graphemes(const fac_engine* engine) { return engine ? engine->e.max_match_graphemes : 0; }
int fac_prefilter_active(const fac_engine* engine) { return engine && engine->e.bitap_ok ? 1 : 0; }

void fac_matches_free(fac_match* matches) { fac::result_free(matches); }

static int stage_common(const fac_engine* engine, const uint8_t* utf8, uint64_t len, int force_ascii, fac_haystack** out,
                 uint64_t* err_graphemes, fac_haystack*& fh) {
  fh = new (std::nothrow) fac_haystack();
  if (!fh) return fail(FAC_E_OOM, "out of host memory");
  std::string err;
  int rc = fac::stage_haystack(engine->e, utf8, len, fh->h, err, force_ascii);
  if (rc == FAC_E_HAYSTACK_TOO_LARGE) {
    if (err_graphemes) *err_graphemes = fh->h.n;
    fac::free_haystack(fh->h);
    delete fh;
    fh = nullptr;
    return fail(rc, "haystack has more than u32::MAX grapheme clusters");
  }
  if (rc) {
    fac::free_haystack(fh->h);
    delete fh;
    fh = nullptr;
    return fail(rc, err);
  }
  *out = fh;
  return FAC_OK;
}

int fac_haystack_stage(const fac_engine* engine, const uint8_t* utf8, uint64_t len, fac_haystack** out,
                       uint64_t* err_graphemes) {
  if (!engine || !out || (len && !utf8)) return fail(FAC_E_INVALID, "NULL argument");
  *out = nullptr;
  // the UTF-8 check and search.rs:196's is_ascii run on the device after the upload (validate_kernel:
  // 256 MiB in well under a millisecond against ~19 ms on 16 host threads)
  const auto t0 = std::chrono::steady_clock::now();
  fac_haystack* fh = nullptr;
  const int rc = stage_common(engine, utf8, len, -2, out, err_graphemes, fh);
  if (fac::diag_env("FAC_TIMING"))
    std::fprintf(stderr, "FAC_TIMING stage: upload + device check + staging %.2f ms (host wall clock)\n",
                 std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
  return rc;
}

int fac_haystack_stage_device(const fac_engine* engine, const uint8_t* d_utf8, uint64_t len, void* stream,
                              fac_haystack** hay, uint64_t* err_graphemes) {
  if (!engine || !hay || (len && !d_utf8)) return fail(FAC_E_INVALID, "NULL argument");
  fac_haystack* fh = *hay;
  const bool fresh = fh == nullptr;
  if (fresh) {
    fh = new (std::nothrow) fac_haystack();
    if (!fh) return fail(FAC_E_OOM, "out of host memory");
  } else if (fh->h.own_utf8 && fh->h.d_utf8) {
    return fail(FAC_E_INVALID, "haystack was not staged from device memory");
  }
  std::string err;
  const int rc = fac::stage_haystack_device(engine->e, d_utf8, len, fh->h, err, static_cast<hipStream_t>(stream));
  if (rc) {
    if (rc == FAC_E_HAYSTACK_TOO_LARGE && err_graphemes) *err_graphemes = fh->h.failed_n;
    if (fresh) {
      fac::free_haystack(fh->h);
      delete fh;
    }
    return fail(rc, rc == FAC_E_HAYSTACK_TOO_LARGE ? std::string("haystack has more than u32::MAX grapheme clusters") : err);
  }
  *hay = fh;
  return FAC_OK;
}

int fac_haystack_stage_shard_device(const fac_engine* engine, const uint8_t* d_utf8, uint64_t len, uint64_t owned_bytes,
                                    int32_t global_ascii, int32_t open_end, uint64_t base, void* stream, fac_haystack** hay,
                                    uint64_t* err_graphemes) {
  if (!engine || !hay || (len && !d_utf8) || owned_bytes > len) return fail(FAC_E_INVALID, "bad argument");
  fac_haystack* fh = *hay;
  const bool fresh = fh == nullptr;
  if (fresh) {
    fh = new (std::nothrow) fac_haystack();
    if (!fh) return fail(FAC_E_OOM, "out of host memory");
  } else if (fh->h.own_utf8 && fh->h.d_utf8) {
    return fail(FAC_E_INVALID, "haystack was not staged from device memory");
  }
  std::string err;
  hipStream_t st = stream ? static_cast<hipStream_t>(stream) : engine->e.stream;
  // the whole haystack's is_ascii decides the grapheme mode (search.rs:196); a Unicode shard's bytes
  // are UTF-8 checked by the segmentation
  int rc = fac::stage_haystack_device(engine->e, d_utf8, len, fh->h, err, st, global_ascii ? 1 : 0);
  uint64_t owned = 0;
  if (!rc) rc = fac::graphemes_before(fh->h, owned_bytes, st, owned, err);
  if (rc) {
    if (rc == FAC_E_HAYSTACK_TOO_LARGE && err_graphemes) *err_graphemes = fh->h.failed_n;
    if (fresh) {
      fac::free_haystack(fh->h);
      delete fh;
    } else {  // a failed restage leaves the haystack empty (searchable)
      fh->h.n = 0;
      fh->h.len = 0;
    }
    return fail(rc, rc == FAC_E_HAYSTACK_TOO_LARGE ? std::string("haystack has more than u32::MAX grapheme clusters") : err);
  }
  fh->h.base = base;
  fh->h.open_end = open_end != 0;
  fh->h.owned = owned;
  *hay = fh;
  return FAC_OK;
}

int fac_shard_plan(uint64_t max_match_graphemes, const uint8_t* utf8, uint64_t len, int32_t is_ascii, uint64_t n_shards,
                   uint64_t shard, uint64_t plan[4]) {
  if (!plan || (len && !utf8) || n_shards == 0 || shard >= n_shards) return fail(FAC_E_INVALID, "bad argument");
  const bool ascii = is_ascii < 0 ? fac::ascii_only(utf8, len) : is_ascii != 0;
  // cut r: the first safe cut at or after r * len / n (ASCII text: graphemes are bytes, any byte)
  auto cut = [&](uint64_t r) -> uint64_t {
    if (r == 0) return 0;
    if (r >= n_shards) return len;
    uint64_t p = (uint64_t)((unsigned __int128)len * r / n_shards);
    if (ascii) return p;
    while (p < len && !fac::safe_cut(utf8, len, p)) ++p;
    return p;
  };
  const uint64_t a = cut(shard), b = std::max(a, cut(shard + 1));
  // halo: max_match_graphemes() + 2 graphemes past b (the +1 of stream_overlap, stream.rs:256-258,
  // and the text[j + 1] lookahead of the last owned window's deepest state)
  const uint64_t halo = max_match_graphemes + 2;
  uint64_t e = b;
  if (ascii) {
    e = std::min<uint64_t>(len, b + halo);
  } else if (b < len) {
    // segment forward from b (a safe cut, or the text end) until `halo` graphemes are complete:
    // boundaries before the last character of the segmented piece are exact (UAX #29 rules look
    // at most one character ahead)
    std::vector<uint64_t> st;
    for (uint64_t span = 16 * halo + 64;; span *= 2) {
      const uint64_t end = std::min(len, b + span);
      uint64_t endc = end;
      while (endc < len && (utf8[endc] & 0xC0) == 0x80) ++endc;  // whole code points
      fac::segment_graphemes(utf8 + b, endc - b, st);
      if (st.size() > halo + 1) {
        e = b + st[halo];
        break;
      }
      if (endc >= len) {
        e = len;
        break;
      }
    }
  }
  plan[0] = a;
  plan[1] = b;
  plan[2] = e;
  plan[3] = (ascii ? 1u : 0u) | (e < len ? 2u : 0u);
  return FAC_OK;
}

int fac_haystack_stage_shard(const fac_engine* engine, const uint8_t* utf8, uint64_t len, uint64_t owned_bytes,
                             int32_t global_ascii, int32_t open_end, uint64_t base, fac_haystack** out,
                             uint64_t* err_graphemes) {
  if (!engine || !out || (len && !utf8) || owned_bytes > len) return fail(FAC_E_INVALID, "bad argument");
  *out = nullptr;
  if (!fac::utf8_valid(utf8, len)) return fail(FAC_E_INVALID, "shard is not valid UTF-8 (cut inside a code point)");
  fac_haystack* fh = nullptr;
  int rc = stage_common(engine, utf8, len, global_ascii ? 1 : 0, out, err_graphemes, fh);
  if (rc) return rc;
  fac::Haystack& h = fh->h;
  h.base = base;
  h.open_end = open_end != 0;
  if (h.ascii) {
    h.owned = owned_bytes;
  } else {
    std::string err;
    if (int hrc = fac::ensure_host(h, err)) {
      fac_haystack_free(fh);
      *out = nullptr;
      return fail(hrc, err);
    }
    h.owned = (uint64_t)(std::lower_bound(h.starts.begin(), h.starts.end(), owned_bytes) - h.starts.begin());
  }
  return FAC_OK;
}

uint64_t fac_haystack_owned_windows(const fac_haystack* hay) { return hay ? std::min(hay->h.n, hay->h.owned) : 0; }

int fac_haystack_set_key_partition(const fac_engine* engine, fac_haystack* hay, uint32_t parts, uint32_t part) {
  if (!engine || !hay || parts == 0 || part >= parts) return fail(FAC_E_INVALID, "bad argument");
  // auto-beam switches the beam on after a running count over the windows in order
  // (search.rs:1096-1103): a key partition has no such order
  if (parts > 1 && engine->e.has_auto_beam) return fail(FAC_E_UNSUPPORTED, "key partitions do not support auto_beam");
  hay->h.kparts = parts;
  hay->h.kpart = part;
  return FAC_OK;
}

uint64_t fac_haystack_graphemes(const fac_haystack* hay) { return hay ? hay->h.n : 0; }

uint64_t fac_haystack_grapheme_starts(const fac_haystack* hay, uint64_t* out, uint64_t cap) {
  if (!hay) return 0;
  const fac::Haystack& h = hay->h;
  std::string err;
  if (!h.ascii && fac::ensure_host(h, err)) return 0;
  for (uint64_t g = 0; g < h.n && g < cap; ++g) out[g] = h.ascii ? g : h.starts[g];
  return h.n;
}

uint64_t fac_haystack_text_chars(const fac_haystack* hay, uint32_t* out, uint64_t cap) {
  if (!hay) return 0;
  const fac::Haystack& h = hay->h;
  if (h.ascii || !h.d_text32 || h.n == 0) return 0;
  const uint64_t k = std::min(h.n, cap);
  if (out && k &&
      (hipSetDevice(h.device) != hipSuccess || hipMemcpy(out, h.d_text32, k * 4, hipMemcpyDeviceToHost) != hipSuccess))
    return 0;
  return h.n;
}

int64_t fac_haystack_symbol_ids(const fac_engine* engine, const fac_haystack* hay, void* stream, uint8_t* out,
                                uint64_t cap) {
  if (!engine || !hay || (cap && !out)) return -(int64_t)fail(FAC_E_INVALID, "NULL argument");
  const fac::Engine& e = engine->e;
  const fac::Haystack& h = hay->h;
  if (!e.bitap_ok) return -1;
  if (h.device != e.device) return -(int64_t)fail(FAC_E_INVALID, "haystack was staged for another device");
  if (h.n == 0) return 0;
  if (hipSetDevice(e.device) != hipSuccess) return -(int64_t)fail(FAC_E_HIP, "hipSetDevice failed");
  hipStream_t st = stream ? static_cast<hipStream_t>(stream) : e.stream;
  hipError_t he = hipSuccess;
  uint8_t* d_ids = static_cast<uint8_t*>(fac::call_scratch_take(h.n, st, &he));
  if (he != hipSuccess || !d_ids) return -(int64_t)fail(FAC_E_OOM, std::string("hipMalloc: ") + hipGetErrorString(he));
  std::string err;
  int rc = FAC_OK;
  if (h.ascii) rc = fac::transcode_ascii_device(e, h.d_utf8, h.n, d_ids, st, err);
  else rc = fac::symbol_ids_device(e, h, 0, h.n, d_ids, st, err);
  const uint64_t take = std::min(cap, h.n);
  if (!rc && ((take && hipMemcpyAsync(out, d_ids, take, hipMemcpyDeviceToHost, st) != hipSuccess) ||
              hipStreamSynchronize(st) != hipSuccess)) {
    rc = FAC_E_HIP;
    err = "copy of the symbol ids failed";
  }
  if (rc) (void)hipStreamSynchronize(st);
  fac::call_scratch_give(d_ids, st);
  if (rc) return -(int64_t)fail(rc, err);
  return (int64_t)h.n;
}

// fac_haystack_grapheme_ids / fac_batch_grapheme_ids: the search path's own ids (ensure_gids), copied out
static int64_t grapheme_ids_out(const fac::Engine& e, const fac::Haystack& h, void* stream, uint32_t* out, uint64_t cap) {
  if (cap && !out) return -(int64_t)fail(FAC_E_INVALID, "NULL argument");
  if (!e.has_map) return -1;
  if (h.device != e.device) return -(int64_t)fail(FAC_E_INVALID, "haystack was staged for another device");
  if (h.ascii || h.n == 0) return 0;
  if (hipSetDevice(e.device) != hipSuccess) return -(int64_t)fail(FAC_E_HIP, "hipSetDevice failed");
  hipStream_t st = stream ? static_cast<hipStream_t>(stream) : e.stream;
  std::string err;
  if (int rc = fac::ensure_gids(e, h, st, err)) return -(int64_t)fail(rc, err);
  const uint64_t take = std::min(cap, h.n);
  if ((take && hipMemcpyAsync(out, h.d_gid, take * 4, hipMemcpyDeviceToHost, st) != hipSuccess) ||
      hipStreamSynchronize(st) != hipSuccess)
    return -(int64_t)fail(FAC_E_HIP, "copy of the grapheme ids failed");
  return (int64_t)h.n;
}

int64_t fac_haystack_grapheme_ids(const fac_engine* engine, const fac_haystack* hay, void* stream, uint32_t* out,
                                  uint64_t cap) {
  if (!engine || !hay) return -(int64_t)fail(FAC_E_INVALID, "NULL argument");
  return grapheme_ids_out(engine->e, hay->h, stream, out, cap);
}

uint32_t fac_engine_grapheme_id(const fac_engine* engine, const uint8_t* utf8, uint64_t len) {
  if (!engine || !engine->e.has_map || !utf8 || len == 0) return 0;
  std::u32string g;
  fac::fold_grapheme(utf8, 0, len, engine->e.case_insensitive, g);
  const auto it = engine->e.gid_of.find(g);
  return it == engine->e.gid_of.end() ? 0u : it->second;
}

void fac_haystack_free(fac_haystack* hay) {
  if (!hay) return;
  fac::free_haystack(hay->h);
  delete hay;
}

int fac_search_staged(const fac_engine* engine, const fac_haystack* hay, uint64_t window_begin,
                      uint64_t window_end, float threshold, void* stream, fac_match** out, uint64_t* n_out,
                      fac_stats* stats) {
  if (!engine || !hay || !out || !n_out) return fail(FAC_E_INVALID, "NULL argument");
  fac_search_args a{};
  a.window_begin = window_begin;
  a.window_end = window_end;
  a.threshold = threshold;
  a.stream = stream;
  return fac_search_staged_ex(engine, hay, &a, out, n_out, stats);
}

int fac_search_staged_ex(const fac_engine* engine, const fac_haystack* hay, const fac_search_args* args,
                         fac_match** out, uint64_t* n_out, fac_stats* stats) {
  if (!engine || !hay || !args || !n_out || (!out && !args->device_out)) return fail(FAC_E_INVALID, "NULL argument");
  if (out) *out = nullptr;
  *n_out = 0;
  const fac::Haystack& h = hay->h;
  fac::SegDesc s = whole(h);
  s.w_begin = std::min(args->window_begin, s.w_end);
  s.w_end = std::min(args->window_end, s.w_end);
  fac::MatchSink sink;
  sink.dev = static_cast<fac_match*>(args->device_out);
  sink.dev_cap = args->device_cap;
  std::string err;
  int rc = fac::launch_search_sink(engine->e, h, {s}, args->threshold, static_cast<hipStream_t>(args->stream),
                                   args->auto_beam_prefix, sink, stats, err);
  if (rc) {
    fac::result_free(sink.pinned);
    return fail(rc, err);
  }
  if (sink.dev) {
    *n_out = sink.n;
    if (sink.n > sink.dev_cap) return fail(FAC_E_OUTPUT_CAPACITY, "device output buffer too small (*n_out = records needed)");
    return FAC_OK;
  }
  return hand_out(sink, out, n_out);
}

int fac_auto_beam_total(const fac_engine* engine, const fac_haystack* hay, uint64_t window_begin, uint64_t window_end,
                        float threshold, void* stream, uint64_t* total) {
  if (!engine || !hay || !total) return fail(FAC_E_INVALID, "NULL argument");
  *total = 0;
  const fac::Haystack& h = hay->h;
  fac::SegDesc s = whole(h);
  s.w_begin = std::min(window_begin, s.w_end);
  s.w_end = std::min(window_end, s.w_end);
  std::string err;
  const int rc = fac::auto_beam_total(engine->e, h, {s}, threshold, static_cast<hipStream_t>(stream), *total, err);
  if (rc) return fail(rc, err);
  return FAC_OK;
}

int fac_search_raw(const fac_engine* engine, const uint8_t* utf8, uint64_t len, float threshold, fac_match** out,
                   uint64_t* n_out, uint64_t* err_graphemes) {
  if (!engine || !out || !n_out) return fail(FAC_E_INVALID, "NULL argument");
  *out = nullptr;
  *n_out = 0;
  fac_haystack* hay = nullptr;
  int rc = fac_haystack_stage(engine, utf8, len, &hay, err_graphemes);
  if (rc) return rc;
  fac::MatchSink sink;
  rc = search_staged_all(engine->e, hay->h, threshold, nullptr, sink, nullptr);
  fac_haystack_free(hay);
  if (rc) {
    fac::result_free(sink.pinned);
    return rc;
  }
  return hand_out(sink, out, n_out);
}

}  // extern "C"

namespace {

// scratch device memory of one call on stream s (reused by the thread's later calls on s)
struct DevMem {
  void* p = nullptr;
  hipStream_t s = nullptr;
  explicit DevMem(hipStream_t st) : s(st) {}
  ~DevMem() {
    if (p) fac::call_scratch_give(p, s);
  }
  int alloc(size_t bytes, std::string& err) {
    hipError_t he = hipSuccess;
    if (p) fac::call_scratch_give(p, s);
    p = fac::call_scratch_take(std::max<size_t>(bytes, 16), s, &he);
    if (he != hipSuccess) {
      p = nullptr;
      err = std::string("hipMalloc: ") + hipGetErrorString(he);
      return FAC_E_OOM;
    }
    return FAC_OK;
  }
};

// The staged bytes [bs, be) = graphemes [g0, g1) searched as a text of their own (search_raw on a
// slice: is_ascii is re-decided on the slice, search.rs:196, prefilter.rs:349-350). A Unicode
// haystack's host copies must be fetched first (ensure_host); slice_descs_device computes the same
// on the device, with no host copy.
fac::SegDesc slice_view(const fac::Haystack& h, uint64_t g0, uint64_t g1) {
  const uint64_t bs = h.ascii ? g0 : (g0 < h.n ? h.starts[g0] : h.len);
  const uint64_t be = h.ascii ? g1 : (g1 < h.n ? h.starts[g1] : h.len);
  const bool asc = h.ascii || fac::ascii_only(h.utf8.data() + bs, be - bs);
  fac::SegDesc s{};
  s.ascii = asc ? 1u : 0u;
  s.text_base = asc ? bs : g0;
  s.n = asc ? be - bs : g1 - g0;
  s.avail = s.n;
  s.hay_len = be - bs;
  s.byte_base = bs;
  s.w_begin = 0;
  s.w_end = s.n;
  return s;
}

}  // namespace

namespace fac {

static uint64_t seg_windows(const std::vector<SegDesc>& segs) {
  uint64_t w = 0;
  for (const SegDesc& s : segs) w += std::min(s.w_end, s.n) > s.w_begin ? std::min(s.w_end, s.n) - s.w_begin : 0;
  return w;
}

// Prefiltered::raw on a text view of a staged haystack (prefilter.rs:304-374): bitap windows on the
// device, each merged window re-searched as its own sub-haystack, best per (start, end, pattern) by
// strictly greater similarity, sorted. Falls back to the full search of the view where the
// reference does (:311-317). Nothing of the text or of its grapheme starts is copied to the host:
// what comes back are the merged-window pairs, for Unicode text their descriptors, and the records.
int prefiltered_view(const Engine& e, const Haystack& h, const SegDesc& view, float threshold, hipStream_t stream,
                     std::vector<fac_match>& merged, fac_stats* stats, std::string& err, uint64_t* searched) {
  merged.clear();
  std::vector<uint32_t> ks;
  if (!e.bitap_ok || !prefilter_ks(e, threshold, ks)) {  // prefilter.rs:151-155, 311-317
    if (searched) *searched += seg_windows({view});
    return launch_search(e, h, {view}, threshold, stream, merged, stats, err);
  }
  std::vector<std::pair<uint64_t, uint64_t>> windows;
  int rc = prefilter_windows(e, h, view, ks, stream, windows, stats, err);
  if (rc) return rc;
  // Re-search each merged window as its own haystack (prefilter.rs:344-350): the slice re-decides
  // is_ascii, so an all-ASCII slice of a Unicode haystack is searched byte-wise.
  std::vector<SegDesc> segs;
  segs.reserve(windows.size());
  if (view.ascii) {  // byte-wise view: windows are bytes of h.d_utf8 from view.text_base
    for (auto& w : windows) {
      const uint64_t gs = w.first, ge = std::min<uint64_t>(w.second, view.n);
      SegDesc s{};
      s.ascii = 1u;
      s.text_base = view.text_base + gs;
      s.n = ge - gs;
      s.avail = s.n;
      s.hay_len = s.n;
      s.byte_base = view.text_base + gs;
      s.w_begin = 0;
      s.w_end = s.n;
      segs.push_back(s);
    }
  } else {  // graphemes of the staged text: byte ranges and is_ascii per window from the device
    for (auto& w : windows) w = {view.text_base + w.first, view.text_base + std::min<uint64_t>(w.second, view.n)};
    if ((rc = slice_descs_device(h, windows, stream ? stream : e.stream, segs, err))) return rc;
  }
  if (segs.empty()) return FAC_OK;
  if (searched) *searched += seg_windows(segs);
  std::vector<fac_match> res;
  rc = launch_search(e, h, segs, threshold, stream, res, stats, err);
  if (rc) return rc;
  std::map<std::tuple<uint64_t, uint64_t, uint32_t>, fac_match> best;
  for (const fac_match& m : res) {
    auto key = std::make_tuple(m.start, m.end, m.pattern_index);
    auto it = best.find(key);
    if (it == best.end()) best.emplace(key, m);
    else if (m.similarity > it->second.similarity) it->second = m;
  }
  merged.reserve(best.size());
  for (auto& kv : best) merged.push_back(kv.second);
  return FAC_OK;
}

}  // namespace fac

namespace {

using fac::prefiltered_view;

// A stream window's view of a whole staged haystack: graphemes [g0, g1) as a text of their own.
// A Unicode haystack's view comes from the device (no host copy of the text or the starts).
int window_view(const fac::Engine& e, const fac::Haystack& h, uint64_t g0, uint64_t g1, hipStream_t st, fac::SegDesc& view,
                std::string& err) {
  if (h.ascii) {
    view = slice_view(h, g0, g1);
    return FAC_OK;
  }
  if (hipSetDevice(e.device) != hipSuccess) {
    err = "hipSetDevice failed";
    return FAC_E_HIP;
  }
  std::vector<fac::SegDesc> v;
  if (int rc = fac::slice_descs_device(h, {{g0, g1}}, st ? st : e.stream, v, err)) return rc;
  view = v[0];
  return FAC_OK;
}

int prefiltered_staged(const fac::Engine& e, const fac::Haystack& h, float threshold, hipStream_t stream,
                       std::vector<fac_match>& merged, fac_stats* stats, std::string& err) {
  if (h.open_end) {
    err = "the pre-filtered search needs a whole haystack, not an open-ended shard";
    return FAC_E_INVALID;
  }
  return prefiltered_view(e, h, whole(h), threshold, stream, merged, stats, err);
}


}  // namespace

namespace fac {

// A batch of stream windows of one staged ASCII haystack searched together (stream.rs
// window_matches for each, :262-297): wins holds (g_begin, g_end, commit_bytes, base) per window,
// sorted by g_begin, each overlapping only its neighbours. With the pre-filter, one q-gram pass over
// the windows' union gives every window its own merged bitap windows (the automaton starts at the
// window's first byte, its coverage stays inside it); without it each window is one segment. All
// segments, tagged with their window, go to one launch; then every window's records are ranked
// sorted().non_overlapping() and cut at its commit point on the host. FAC_E_UNSUPPORTED (nothing
// done) when the batch does not qualify: a Unicode haystack (a window's grapheme segmentation
// depends on where its text starts and ends), windows out of order or overlapping beyond their
// neighbours, or pre-filter tables that need the packed full scan. (Its counterpart for every other
// task, stream_windows_docs, stands at the end of this file: it calls batch_kept, defined below.)
int stream_windows_batch(const Engine& e, const Haystack& h, const uint64_t* wins, uint64_t n_windows, float threshold,
                         bool prefilter, hipStream_t st, std::vector<fac_match>& owned, fac_stats* stats, std::string& err,
                         std::vector<uint64_t>* win_off, uint64_t* searched, const StreamBoundary* sb) {
  owned.clear();
  if (win_off) win_off->assign(n_windows + 1, 0);  // (the early returns below: no records at all)
  if (!h.ascii || h.open_end || h.base || n_windows == 0 || n_windows >= (1u << 24) || h.len >= (1ull << kWinTagShift))
    return FAC_E_UNSUPPORTED;
  std::vector<std::pair<uint64_t, uint64_t>> span(n_windows);
  std::vector<WinOwn> own(n_windows);
  uint64_t u0 = UINT64_MAX, u1 = 0;
  for (uint64_t w = 0; w < n_windows; ++w) {
    const uint64_t ge = std::min<uint64_t>(wins[4 * w + 1], h.n), gb = std::min<uint64_t>(wins[4 * w], ge);
    span[w] = {gb, ge};
    own[w] = WinOwn{gb, wins[4 * w + 2], wins[4 * w + 3]};  // ASCII: grapheme = byte
    u0 = std::min(u0, gb);
    u1 = std::max(u1, ge);
    if (w && gb < span[w - 1].first) return FAC_E_UNSUPPORTED;
    if (w >= 2 && span[w - 2].second >= gb) return FAC_E_UNSUPPORTED;  // same parity must not touch
  }
  if (u1 <= u0) return FAC_OK;
  const SegDesc view = slice_view(h, u0, u1);
  std::vector<SegDesc> segs;
  std::vector<uint32_t> ks;
  if (prefilter && e.bitap_ok && prefilter_ks(e, threshold, ks)) {
    std::vector<std::pair<uint64_t, uint64_t>> rel(n_windows), runs;
    for (uint64_t w = 0; w < n_windows; ++w) rel[w] = {span[w].first - u0, span[w].second - u0};
    std::vector<uint32_t> run_win;
    // (one window is the whole view: the plain pass, no window bounds or second bitmap)
    if (int rc = prefilter_windows_ex(e, h, view, ks, st, n_windows > 1 ? &rel : nullptr, runs, &run_win, stats, err))
      return rc;
    if (n_windows == 1) run_win.assign(runs.size(), 0u);
    segs.reserve(runs.size());
    for (size_t r = 0; r < runs.size(); ++r) {
      SegDesc s{};
      s.ascii = 1u;
      s.text_base = view.text_base + runs[r].first;
      s.n = runs[r].second - runs[r].first;
      s.avail = s.n;
      s.hay_len = s.n;
      s.byte_base = s.text_base | ((uint64_t)run_win[r] << kWinTagShift);  // the window tag (WinOwn)
      s.w_begin = 0;
      s.w_end = s.n;
      segs.push_back(s);
    }
  } else {  // no pre-filter (or the reference's fallback to a full search, prefilter.rs:311-317)
    for (uint64_t w = 0; w < n_windows; ++w) {
      if (span[w].second <= span[w].first) continue;
      SegDesc s = slice_view(h, span[w].first, span[w].second);
      s.byte_base |= (uint64_t)w << kWinTagShift;  // the window tag (WinOwn)
      segs.push_back(s);
    }
  }
  if (segs.empty()) return FAC_OK;
  if (searched) *searched += seg_windows(segs);
  // whole-token matches (fac.h fac_stream_open_opts): the windows' sources and lengths, the carried
  // context and the kernel's counter, one upload; the raw set is filtered in HBM into the record
  // buffer's other half before it comes to the host
  const bool flagged = sb && sb->sides;
  DevMem d_sb(st);
  StreamFilter sf;
  unsigned long long* d_count = nullptr;
  std::vector<uint64_t> sbt;
  if (flagged) {
    sbt.assign(2 * n_windows + kBoundaryCarry / 8 + 1, 0);
    for (uint64_t w = 0; w < n_windows; ++w) {
      sbt[w] = span[w].first;
      sbt[n_windows + w] = span[w].second - span[w].first;
    }
    const uint32_t cn = std::min<uint32_t>(sb->before_len, kBoundaryCarry);
    if (cn) std::memcpy(sbt.data() + 2 * n_windows, sb->before + (sb->before_len - cn), cn);
    if (int rc = d_sb.alloc(sbt.size() * 8, err)) return rc;
    if (hipMemcpyAsync(d_sb.p, sbt.data(), sbt.size() * 8, hipMemcpyHostToDevice, st) != hipSuccess) {
      err = "upload of a stream task's boundary context failed";
      return FAC_E_HIP;
    }
    const uint64_t* dt = static_cast<const uint64_t*>(d_sb.p);
    sf.sides = sb->sides;
    sf.d_text = h.d_utf8;
    sf.text_len = h.len;
    sf.d_src = dt;
    sf.d_len = dt + n_windows;
    sf.n_windows = n_windows;
    sf.d_before = reinterpret_cast<const uint8_t*>(dt + 2 * n_windows);
    sf.before_len = cn;
    d_count = reinterpret_cast<unsigned long long*>(static_cast<uint64_t*>(d_sb.p) + sbt.size() - 1);
  }
  uint64_t cap = 1u << 16;
  for (;;) {  // raw records into a device buffer, grown and searched again if it was too small
    DevMem raw(st);
    if (int rc = raw.alloc((flagged ? 2 : 1) * cap * sizeof(fac_match), err)) return rc;
    MatchSink sink;
    sink.dev = static_cast<fac_match*>(raw.p);
    sink.dev_cap = cap;
    if (int rc = launch_search_sink(e, h, segs, threshold, st, 0, sink, stats, err)) return rc;
    if (sink.n > cap) {
      cap = sink.n;
      continue;
    }
    if (flagged && sink.n) {
      uint64_t kept = 0;
      if (int rc = stream_boundary_filter_device(e.device, sf, sink.dev, sink.n, sink.dev + cap, d_count, st, &kept, err))
        return rc;
      sink.dev += cap;
      sink.n = kept;
    }
    std::vector<fac_match> recs(sink.n);
    if (sink.n) {
      if (hipMemcpyAsync(recs.data(), sink.dev, sink.n * sizeof(fac_match), hipMemcpyDeviceToHost, st) != hipSuccess ||
          hipStreamSynchronize(st) != hipSuccess) {
        err = "hipMemcpyAsync of a stream batch's records failed";
        return FAC_E_HIP;
      }
    }
    windows_owned_host(e, recs, own, owned, win_off);
    return FAC_OK;
  }
}

}  // namespace fac

namespace {
}  // namespace

extern "C" {

int fac_search_prefiltered(const fac_engine* engine, const uint8_t* utf8, uint64_t len, float threshold,
                           fac_match** out, uint64_t* n_out, uint64_t* err_graphemes) {
  if (!engine || !out || !n_out) return fail(FAC_E_INVALID, "NULL argument");
  *out = nullptr;
  *n_out = 0;
  fac_haystack* hay = nullptr;
  int rc = fac_haystack_stage(engine, utf8, len, &hay, err_graphemes);
  if (rc) return rc;
  std::vector<fac_match> merged;
  std::string err;
  rc = prefiltered_staged(engine->e, hay->h, threshold, nullptr, merged, nullptr, err);
  fac_haystack_free(hay);
  if (rc) return fail(rc, err);
  return copy_out(merged, out, n_out);
}

int fac_search_staged_prefiltered(const fac_engine* engine, const fac_haystack* hay, float threshold, void* stream,
                                  fac_match** out, uint64_t* n_out, fac_stats* stats) {
  if (!engine || !hay || !out || !n_out) return fail(FAC_E_INVALID, "NULL argument");
  *out = nullptr;
  *n_out = 0;
  std::vector<fac_match> merged;
  std::string err;
  const int rc =
      prefiltered_staged(engine->e, hay->h, threshold, static_cast<hipStream_t>(stream), merged, stats, err);
  if (rc) return fail(rc, err);
  return copy_out(merged, out, n_out);
}

int fac_stream_window_staged(const fac_engine* engine, const fac_haystack* hay, uint64_t g_begin, uint64_t g_end,
                             uint64_t commit_bytes, uint64_t base, float threshold, int32_t prefilter, void* stream,
                             fac_match** out, uint64_t* n_out, fac_stats* stats) {
  if (!engine || !hay || !out || !n_out) return fail(FAC_E_INVALID, "NULL argument");
  *out = nullptr;
  *n_out = 0;
  const fac::Haystack& h = hay->h;
  if (h.open_end || h.base) return fail(FAC_E_INVALID, "stream windows are cut from a whole staged haystack");
  g_end = std::min(g_end, h.n);
  g_begin = std::min(g_begin, g_end);
  const fac::Engine& e = engine->e;
  hipStream_t st = static_cast<hipStream_t>(stream);
  std::vector<fac_match> v;
  std::string err;
  fac::SegDesc view{};
  if (int vrc = window_view(e, h, g_begin, g_end, st, view, err)) return fail(vrc, err);
  int rc = prefilter ? prefiltered_view(e, h, view, threshold, st, v, stats, err)
                     : fac::launch_search(e, h, {view}, threshold, st, v, stats, err);
  if (rc) return fail(rc, err);
  // window_matches (stream.rs:262-297): sorted().non_overlapping() within the window, then the
  // matches the window owns (start < commit), at absolute offsets
  if (!v.empty() && (rc = fac::apply_matches(e, v, 1, 1, nullptr, err))) return fail(rc, err);
  std::vector<fac_match> owned;
  owned.reserve(v.size());
  for (fac_match m : v) {
    m.start -= view.byte_base;
    m.end -= view.byte_base;
    if (m.start < commit_bytes) {
      m.start += base;
      m.end += base;
      owned.push_back(m);
    }
  }
  return copy_out(owned, out, n_out);
}

int fac_stream_window_staged_device(const fac_engine* engine, const fac_haystack* hay, uint64_t g_begin, uint64_t g_end,
                                    uint64_t commit_bytes, uint64_t base, float threshold, int32_t prefilter, void* stream,
                                    void* device_out, uint64_t device_cap, uint64_t* n_out, fac_stats* stats) {
  if (!engine || !hay || !n_out || (!device_out && device_cap)) return fail(FAC_E_INVALID, "NULL argument");
  *n_out = 0;
  const fac::Haystack& h = hay->h;
  if (h.open_end || h.base) return fail(FAC_E_INVALID, "stream windows are cut from a whole staged haystack");
  g_end = std::min(g_end, h.n);
  g_begin = std::min(g_begin, g_end);
  std::string err;
  const fac::Engine& e = engine->e;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (hipSetDevice(e.device) != hipSuccess) return fail(FAC_E_HIP, "hipSetDevice failed");
  fac::SegDesc view{};
  if (int vrc = window_view(e, h, g_begin, g_end, st, view, err)) return fail(vrc, err);
  // the window's searched segments: Prefiltered::raw's merged bitap windows (disjoint and not
  // adjacent, so their records never share a (start, end, pattern) key and the reference's
  // best-per-key merge is a no-op before the ranking), or the whole view where it falls back
  std::vector<fac::SegDesc> segs;
  std::vector<uint32_t> ks;
  const bool timing = fac::diag_env("FAC_TIMING") != nullptr;  // diagnostics: host wall-clock phases
  const auto t0 = std::chrono::steady_clock::now();
  auto ms_since = [&](std::chrono::steady_clock::time_point t) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
  };
  double t_pf = 0, t_segs = 0, t_search = 0;
  if (prefilter && e.bitap_ok && prefilter_ks(e, threshold, ks)) {
    std::vector<std::pair<uint64_t, uint64_t>> windows;
    if (int rc = fac::prefilter_windows(e, h, view, ks, st, windows, stats, err)) return fail(rc, err);
    t_pf = ms_since(t0);
    if (view.ascii) {
      for (auto& w : windows) {
        const uint64_t gs = w.first, ge = std::min<uint64_t>(w.second, view.n);
        fac::SegDesc s{};
        s.ascii = 1u;
        s.text_base = view.text_base + gs;
        s.n = ge - gs;
        s.avail = s.n;
        s.hay_len = s.n;
        s.byte_base = view.text_base + gs;
        s.w_begin = 0;
        s.w_end = s.n;
        segs.push_back(s);
      }
    } else {
      for (auto& w : windows) w = {view.text_base + w.first, view.text_base + std::min<uint64_t>(w.second, view.n)};
      if (int rc = fac::slice_descs_device(h, windows, st ? st : e.stream, segs, err)) return fail(rc, err);
    }
  } else {
    segs.push_back(view);
  }
  t_segs = ms_since(t0);
  if (segs.empty()) return FAC_OK;
  // raw records into a device buffer (grown and searched again if a window ever needs more)
  uint64_t cap = 1u << 16;
  for (;;) {
    DevMem raw(st);
    if (int rc = raw.alloc(2 * cap * sizeof(fac_match), err)) return fail(rc, err);
    fac::MatchSink sink;
    sink.dev = static_cast<fac_match*>(raw.p);
    sink.dev_cap = cap;
    if (int rc = fac::launch_search_sink(e, h, segs, threshold, st, 0, sink, stats, err)) return fail(rc, err);
    if (sink.n > cap) {
      cap = sink.n;
      continue;
    }
    t_search = ms_since(t0);
    const int rc = fac::window_owned_device(e, sink.dev, sink.dev + cap, sink.n, view.byte_base, commit_bytes, base, st,
                                            static_cast<fac_match*>(device_out), device_cap, n_out, err);
    if (timing)
      std::fprintf(stderr, "FAC_TIMING window: prefilter %.3f, segs %.3f (%zu), search %.3f, owned %.3f ms\n", t_pf,
                   t_segs - t_pf, segs.size(), t_search - t_segs, ms_since(t0) - t_search);
    if (rc == FAC_E_OUTPUT_CAPACITY) return fail(rc, "device output buffer too small (*n_out = records needed)");
    if (rc) return fail(rc, err);
    return FAC_OK;
  }
}

// The owned records of a run of stream windows, in window order (win_off, optional: their CSR
// index): batched where the run qualifies (stream_windows_batch), window by window otherwise.
static int owned_windows(const fac_engine* engine, const fac_haystack* hay, const uint64_t* windows, uint64_t n_windows,
                         float threshold, int32_t prefilter, void* stream, std::vector<fac_match>& owned,
                         std::vector<uint64_t>* win_off, fac_stats* stats) {
  const fac::Haystack& h = hay->h;
  if (h.open_end || h.base) return fail(FAC_E_INVALID, "stream windows are cut from a whole staged haystack");
  const fac::Engine& e = engine->e;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (hipSetDevice(e.device) != hipSuccess) return fail(FAC_E_HIP, "hipSetDevice failed");
  std::string err;
  int rc = fac::stream_windows_batch(e, h, windows, n_windows, threshold, prefilter != 0, st, owned, stats, err, win_off);
  if (rc == FAC_E_UNSUPPORTED) {  // window by window (fac_stream_window_staged)
    owned.clear();
    for (uint64_t w = 0; w < n_windows; ++w) {
      fac_match* part = nullptr;
      uint64_t np = 0;
      rc = fac_stream_window_staged(engine, hay, windows[4 * w], windows[4 * w + 1], windows[4 * w + 2], windows[4 * w + 3],
                                    threshold, prefilter, stream, &part, &np, stats);
      if (rc) return rc;
      if (win_off) (*win_off)[w] = owned.size();
      owned.insert(owned.end(), part, part + np);
      fac_matches_free(part);
    }
    if (win_off) (*win_off)[n_windows] = owned.size();
  } else if (rc) {
    return fail(rc, err);
  }
  return FAC_OK;
}

int fac_stream_windows_staged_device(const fac_engine* engine, const fac_haystack* hay, const uint64_t* windows,
                                     uint64_t n_windows, float threshold, int32_t prefilter, void* stream, void* device_out,
                                     uint64_t device_cap, uint64_t* n_out, fac_stats* stats) {
  if (!engine || !hay || !n_out || (!windows && n_windows) || (!device_out && device_cap))
    return fail(FAC_E_INVALID, "NULL argument");
  *n_out = 0;
  hipStream_t st = static_cast<hipStream_t>(stream);
  std::vector<fac_match> owned;
  if (int rc = owned_windows(engine, hay, windows, n_windows, threshold, prefilter, stream, owned, nullptr, stats)) return rc;
  *n_out = owned.size();
  if (owned.size() > device_cap) return fail(FAC_E_OUTPUT_CAPACITY, "device output buffer too small (*n_out = records needed)");
  if (!owned.empty() &&
      (hipMemcpyAsync(device_out, owned.data(), owned.size() * sizeof(fac_match), hipMemcpyHostToDevice, st) != hipSuccess ||
       hipStreamSynchronize(st) != hipSuccess))
    return fail(FAC_E_HIP, "hipMemcpyAsync of the owned records failed");
  return FAC_OK;
}

int fac_replace_windows_staged_device(const fac_engine* engine, const fac_haystack* hay, const uint64_t* windows,
                                      uint64_t n_windows, const fac_replacements* replacements, float threshold,
                                      int32_t prefilter, void* stream, uint64_t* emitted, void* device_out,
                                      uint64_t device_cap, uint64_t* out_len, uint64_t* n_applied, uint64_t* n_skipped,
                                      fac_stats* stats) {
  if (!engine || !hay || !replacements || !emitted || !out_len || (!windows && n_windows) || (!device_out && device_cap))
    return fail(FAC_E_INVALID, "NULL argument");
  *out_len = 0;
  if (n_applied) *n_applied = 0;
  if (n_skipped) *n_skipped = 0;
  const fac::Engine& e = engine->e;
  const fac::Haystack& h = hay->h;
  const fac::ReplaceTable& t = replacements->t;
  if (h.open_end || h.base) return fail(FAC_E_INVALID, "stream windows are cut from a whole staged haystack");
  if (h.device != e.device) return fail(FAC_E_INVALID, "haystack was staged for another device");
  if (t.device != e.device || t.n_patterns != e.pats.size())
    return fail(FAC_E_INVALID, "the replacement table was built for another engine");
  if (n_windows == 0) return FAC_OK;  // (no window, no commit point: the cursor stays)
  std::string err;
  if (!h.ascii)
    if (int hrc = fac::ensure_host(h, err)) return fail(hrc, err);
  // the windows in bytes of the staged text: records come back at those offsets (base = the window's
  // first byte), and base - that byte must be one value, the stream offset of the text's byte 0
  auto byte_of = [&](uint64_t g) { return h.ascii ? g : (g < h.n ? h.starts[g] : h.len); };
  std::vector<uint64_t> local(windows, windows + 4 * n_windows), commit(n_windows);
  uint64_t shift = 0;
  for (uint64_t w = 0; w < n_windows; ++w) {
    const uint64_t g1 = std::min(windows[4 * w + 1], h.n), g0 = std::min(windows[4 * w], g1);
    const uint64_t b0 = byte_of(g0), b1 = byte_of(g1), base = windows[4 * w + 3];
    if (base < b0 || (w && base - b0 != shift))
      return fail(FAC_E_INVALID, "every window's base must place the staged text at the same stream offset");
    shift = base - b0;
    local[4 * w + 3] = b0;
    commit[w] = b0 + std::min(windows[4 * w + 2], b1 - b0);
  }
  if (*emitted < shift || *emitted - shift > h.len)
    return fail(FAC_E_INVALID, "*emitted lies outside the staged text");
  hipStream_t st = stream ? static_cast<hipStream_t>(stream) : e.stream;
  std::vector<fac_match> owned;
  std::vector<uint64_t> win_off(n_windows + 1, 0);
  if (int rc = owned_windows(engine, hay, local.data(), n_windows, threshold, prefilter, stream, owned, &win_off, stats))
    return rc;
  fac::StreamReplacePlan plan;
  if (int rc = fac::replace_stream_plan_device(t, owned, win_off, commit, *emitted - shift, st, plan, err))
    return fail(rc, err);
  *out_len = plan.total;
  if (plan.total >= (1ull << fac::kDocTagShift)) return fail(FAC_E_UNSUPPORTED, "the output would hold 2^40 bytes or more");
  if (plan.total > device_cap)
    return fail(FAC_E_OUTPUT_CAPACITY, "device output buffer too small (*out_len = bytes needed)");
  if (int rc = fac::replace_stream_copy_device(h.d_utf8, t, plan, static_cast<uint8_t*>(device_out), err))
    return fail(rc, err);
  if (hipStreamSynchronize(st) != hipSuccess) return fail(FAC_E_HIP, "the splice of the stream windows failed");
  *emitted = plan.e_out + shift;
  if (n_applied) *n_applied = plan.n_replaced;
  if (n_skipped) *n_skipped = plan.n_skipped;
  return FAC_OK;
}

int fac_matches_apply(const fac_engine* engine, fac_match* matches, uint64_t n, int32_t order, int32_t overlap,
                      const uint64_t* unique_ids, uint64_t* n_out) {
  if (!engine || (!matches && n) || !n_out) return fail(FAC_E_INVALID, "NULL argument");
  if (order < 0 || order > 3 || overlap < 0 || overlap > 2) return fail(FAC_E_INVALID, "bad order/overlap");
  std::vector<fac_match> v(matches, matches + n);
  std::string err;
  const int rc = fac::apply_matches(engine->e, v, order, overlap, unique_ids, err);
  if (rc) return fail(rc, err);
  if (!v.empty()) std::memcpy(matches, v.data(), v.size() * sizeof(fac_match));
  *n_out = v.size();
  return FAC_OK;
}

// ---- batches (fac.h "Batches"): staging, search and per-document apply on the device

// Whether a batch call takes the pre-filtered path, and if so every document's merged windows.
// The reference falls back to the plain search when the engine has no filter or some pattern's
// k_for exceeds 24 (prefilter.rs:151-155, 311-317): engine and threshold alone decide, so a fallback
// call is the plain batch call for any batch. Where the filter runs, the batch must be all ASCII
// (its one scan resets at document starts in byte coordinates) or opted in
// (fac_batch_allow_unicode_prefilter: the scan runs over symbols, fac_internal.h Batch::unicode_pf).
static int batch_prefilter(const fac::Engine& e, const fac::Batch& b, float threshold, bool prefilter, hipStream_t st,
                           fac::BatchWindows& pw, bool& filtered, fac_stats* stats, std::string& err) {
  filtered = false;
  std::vector<uint32_t> ks;
  if (!prefilter || !e.bitap_ok || !prefilter_ks(e, threshold, ks)) return FAC_OK;
  if (!b.h.ascii && !b.unicode_pf) {
    err = "pre-filtered batches need an all-ASCII batch (search the other documents one by one)";
    return FAC_E_UNSUPPORTED;
  }
  filtered = true;
  return fac::batch_prefilter_windows(e, b, ks, st, pw, stats, err);
}

static int batch_limits(uint64_t n_docs, uint64_t total_len) {
  if (n_docs > fac::kBatchMaxDocs || total_len >= (1ull << fac::kDocTagShift))
    return fail(FAC_E_UNSUPPORTED, "a batch holds at most 2^24 documents and fewer than 2^40 bytes");
  return FAC_OK;
}

static int batch_stage_fail(fac_batch* fb, bool fresh, int rc, const std::string& err, uint64_t* err_doc,
                            uint64_t* err_graphemes) {
  if ((rc == FAC_E_INVALID || rc == FAC_E_HAYSTACK_TOO_LARGE) && fb->b.err_doc != ~0ull && err_doc) *err_doc = fb->b.err_doc;
  if (rc == FAC_E_HAYSTACK_TOO_LARGE && err_graphemes) *err_graphemes = fb->b.err_graphemes;
  if (fresh) {
    fac::free_batch(fb->b);
    delete fb;
  } else {  // a failed restage leaves an empty batch
    fb->b.n_docs = 0;
    fb->b.n_segs = 0;
    fb->b.windows = 0;
    fb->b.h.len = 0;
    fb->b.h.n = 0;
  }
  return fail(rc, rc == FAC_E_HAYSTACK_TOO_LARGE ? std::string("a document has more than u32::MAX grapheme clusters") : err);
}

int fac_batch_stage(const fac_engine* engine, const uint8_t* utf8, const uint64_t* offsets, uint64_t n_docs,
                    fac_batch** out, uint64_t* err_doc, uint64_t* err_graphemes) {
  if (!engine || !out || (n_docs && !offsets)) return fail(FAC_E_INVALID, "NULL argument");
  *out = nullptr;
  // the last offset is the byte count; everything else about the offsets is checked on the device
  const uint64_t len = n_docs ? offsets[n_docs] : 0;
  if (len && !utf8) return fail(FAC_E_INVALID, "NULL argument");
  if (int rc = batch_limits(n_docs, len)) return rc;
  const fac::Engine& e = engine->e;
  if (hipSetDevice(e.device) != hipSuccess) return fail(FAC_E_HIP, "hipSetDevice failed");
  fac_batch* fb = new (std::nothrow) fac_batch();
  if (!fb) return fail(FAC_E_OOM, "out of host memory");
  fac::Batch& b = fb->b;
  b.h.device = e.device;
  b.h.len = len;
  b.n_docs = n_docs;
  std::string err;
  int rc = FAC_OK;
  hipStream_t st = e.stream;
  if (hipMalloc((void**)&b.h.d_utf8, std::max<uint64_t>(len, 16)) != hipSuccess ||
      hipMalloc((void**)&b.d_offsets, (n_docs + 1) * 8) != hipSuccess) {
    rc = FAC_E_OOM;
    err = "hipMalloc of the batch failed";
  }
  b.h.own_utf8 = true;
  b.own_offsets = true;
  b.offsets_cap = n_docs + 1;
  if (!rc && ((len && hipMemcpyAsync(b.h.d_utf8, utf8, len, hipMemcpyHostToDevice, st) != hipSuccess) ||
              (n_docs && hipMemcpyAsync(b.d_offsets, offsets, (n_docs + 1) * 8, hipMemcpyHostToDevice, st) != hipSuccess))) {
    rc = FAC_E_HIP;
    err = "hipMemcpyAsync of the batch failed";
  }
  if (!rc) rc = fac::stage_batch_device(e, b, st, err);
  if (rc) return batch_stage_fail(fb, true, rc, err, err_doc, err_graphemes);
  *out = fb;
  return FAC_OK;
}

int fac_batch_stage_device(const fac_engine* engine, const uint8_t* d_utf8, const uint64_t* d_offsets, uint64_t n_docs,
                           uint64_t total_len, void* stream, fac_batch** batch, uint64_t* err_doc,
                           uint64_t* err_graphemes) {
  if (!engine || !batch || (n_docs && !d_offsets) || (total_len && !d_utf8)) return fail(FAC_E_INVALID, "NULL argument");
  if (!n_docs && total_len) return fail(FAC_E_INVALID, "bytes without documents");
  if (int rc = batch_limits(n_docs, total_len)) return rc;
  const fac::Engine& e = engine->e;
  if (hipSetDevice(e.device) != hipSuccess) return fail(FAC_E_HIP, "hipSetDevice failed");
  fac_batch* fb = *batch;
  const bool fresh = fb == nullptr;
  if (fresh) {
    fb = new (std::nothrow) fac_batch();
    if (!fb) return fail(FAC_E_OOM, "out of host memory");
  } else if (fb->b.h.own_utf8 && fb->b.h.d_utf8) {
    return fail(FAC_E_INVALID, "batch was not staged from device memory");
  }
  fac::Batch& b = fb->b;
  b.h.device = e.device;
  b.h.len = total_len;
  b.h.d_utf8 = const_cast<uint8_t*>(d_utf8);
  b.h.own_utf8 = false;
  b.d_offsets = const_cast<uint64_t*>(d_offsets);
  b.own_offsets = false;
  b.n_docs = n_docs;
  std::string err;
  hipStream_t st = stream ? static_cast<hipStream_t>(stream) : e.stream;
  const int rc = fac::stage_batch_device(e, b, st, err);
  if (rc) {
    b.h.d_utf8 = nullptr;
    b.d_offsets = nullptr;
    return batch_stage_fail(fb, fresh, rc, err, err_doc, err_graphemes);
  }
  *batch = fb;
  return FAC_OK;
}

void fac_batch_free(fac_batch* batch) {
  if (!batch) return;
  fac::free_batch(batch->b);
  delete batch;
}

uint64_t fac_batch_docs(const fac_batch* batch) { return batch ? batch->b.n_docs : 0; }

int fac_batch_allow_unicode_prefilter(fac_batch* batch, int32_t on) {
  if (!batch) return fail(FAC_E_INVALID, "NULL argument");
  batch->b.unicode_pf = on != 0;
  return FAC_OK;
}

int fac_batch_allow_unicode_mappings(fac_batch* batch, int32_t on) {
  if (!batch) return fail(FAC_E_INVALID, "NULL argument");
  batch->b.unicode_map = on != 0;
  return FAC_OK;
}

int fac_batch_require_boundaries(fac_batch* batch, int32_t sides) {
  if (!batch) return fail(FAC_E_INVALID, "NULL argument");
  if (sides < 0 || sides > FAC_BOUNDARY_WHOLE) return fail(FAC_E_INVALID, "sides must be 0..3");
  batch->b.boundaries = sides;
  return FAC_OK;
}

int fac_batch_require_anchors(fac_batch* batch, int32_t sides) {
  if (!batch) return fail(FAC_E_INVALID, "NULL argument");
  if (sides < 0 || sides > FAC_ANCHOR_WHOLE) return fail(FAC_E_INVALID, "sides must be 0..3");
  batch->b.anchors = sides;
  return FAC_OK;
}

int32_t fac_anchor_ok(uint64_t doc_len, uint64_t start, uint64_t end, int32_t sides) {
  if (sides < 0 || sides > FAC_ANCHOR_WHOLE) return -(int32_t)fail(FAC_E_INVALID, "sides must be 0..3");
  if (start > end || end > doc_len) return -(int32_t)fail(FAC_E_INVALID, "span outside the document");
  if ((sides & FAC_ANCHOR_START) && start != 0) return 0;
  if ((sides & FAC_ANCHOR_END) && end != doc_len) return 0;
  return 1;
}

int32_t fac_boundary_class(uint32_t cp) { return (int32_t)fac::boundary_class(cp); }

int32_t fac_boundary_ok(const uint8_t* utf8, uint64_t len, uint64_t start, uint64_t end, int32_t sides) {
  if ((len && !utf8) || sides < 0 || sides > FAC_BOUNDARY_WHOLE) return -(int32_t)fail(FAC_E_INVALID, "bad argument");
  if (start > end || end > len) return -(int32_t)fail(FAC_E_INVALID, "span outside the text");
  if ((start < len && (utf8[start] & 0xC0) == 0x80) || (end < len && (utf8[end] & 0xC0) == 0x80))
    return -(int32_t)fail(FAC_E_INVALID, "span not on a character boundary");
  return fac::boundary_ok(utf8, len, start, end, sides) ? 1 : 0;
}

int32_t fac_boundary_ok_after(const uint8_t* before, uint64_t before_len, int32_t more_before, const uint8_t* utf8,
                              uint64_t len, uint64_t start, uint64_t end, int32_t sides) {
  if ((len && !utf8) || (before_len && !before) || sides < 0 || sides > FAC_BOUNDARY_WHOLE)
    return -(int32_t)fail(FAC_E_INVALID, "bad argument");
  if (start > end || end > len) return -(int32_t)fail(FAC_E_INVALID, "span outside the text");
  if ((start < len && (utf8[start] & 0xC0) == 0x80) || (end < len && (utf8[end] & 0xC0) == 0x80))
    return -(int32_t)fail(FAC_E_INVALID, "span not on a character boundary");
  const int ok = fac::boundary_ok_after(before, before_len, more_before != 0, utf8, len, start, end, sides);
  if (ok < 0) return -(int32_t)fail(FAC_E_INVALID, "the context before the text is too short to decide the start side");
  return ok;
}

int64_t fac_batch_grapheme_ids(const fac_engine* engine, const fac_batch* batch, void* stream, uint32_t* out, uint64_t cap) {
  if (!engine || !batch) return -(int64_t)fail(FAC_E_INVALID, "NULL argument");
  return grapheme_ids_out(engine->e, batch->b.h, stream, out, cap);
}

uint64_t fac_batch_doc_graphemes(const fac_batch* batch, uint64_t d, int32_t* is_ascii) {
  if (is_ascii) *is_ascii = 1;
  if (!batch || d >= batch->b.n_docs) return 0;
  const fac::Batch& b = batch->b;
  uint32_t f = 0;
  fac::BatchTri t{0, 0, 0};
  if (hipSetDevice(b.h.device) != hipSuccess || hipMemcpy(&f, b.d_flags + d, 4, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(&t, b.d_tri_in + d, sizeof(t), hipMemcpyDeviceToHost) != hipSuccess)
    return 0;
  if (is_ascii) *is_ascii = (f & 2u) ? 0 : 1;
  return t.w;
}

uint64_t fac_batch_grapheme_starts(const fac_batch* batch, uint64_t d, uint64_t* out, uint64_t cap) {
  if (!batch || d >= batch->b.n_docs) return 0;
  const fac::Batch& b = batch->b;
  uint32_t f = 0;
  fac::BatchTri t{0, 0, 0}, ex{0, 0, 0};
  uint64_t lo = 0;
  if (hipSetDevice(b.h.device) != hipSuccess || hipMemcpy(&f, b.d_flags + d, 4, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(&t, b.d_tri_in + d, sizeof(t), hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(&ex, b.d_tri_ex + d, sizeof(ex), hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(&lo, b.d_offsets + d, 8, hipMemcpyDeviceToHost) != hipSuccess)
    return 0;
  const uint64_t n = t.w, k = std::min(n, cap);
  if (!out || !k) return n;
  if (!(f & 2u)) {
    for (uint64_t g = 0; g < k; ++g) out[g] = g;
    return n;
  }
  if (hipMemcpy(out, b.h.d_off + ex.u, k * 8, hipMemcpyDeviceToHost) != hipSuccess) return 0;
  for (uint64_t g = 0; g < k; ++g) out[g] = (out[g] & ((1ull << fac::kDocTagShift) - 1)) - lo;
  return n;
}

uint64_t fac_batch_text_chars(const fac_batch* batch, uint64_t d, uint32_t* out, uint64_t cap) {
  if (!batch || d >= batch->b.n_docs) return 0;
  const fac::Batch& b = batch->b;
  uint32_t f = 0;
  fac::BatchTri t{0, 0, 0}, ex{0, 0, 0};
  if (hipSetDevice(b.h.device) != hipSuccess || hipMemcpy(&f, b.d_flags + d, 4, hipMemcpyDeviceToHost) != hipSuccess)
    return 0;
  if (!(f & 2u) || !b.h.d_text32) return 0;  // an ASCII document has no folded characters
  if (hipMemcpy(&t, b.d_tri_in + d, sizeof(t), hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(&ex, b.d_tri_ex + d, sizeof(ex), hipMemcpyDeviceToHost) != hipSuccess)
    return 0;
  const uint64_t n = t.w, k = std::min(n, cap);
  if (out && k && hipMemcpy(out, b.h.d_text32 + ex.u, k * 4, hipMemcpyDeviceToHost) != hipSuccess) return 0;
  return n;
}

// The shared front of every batch call: the pre-filter where the reference's Prefiltered::search
// would run it (prefilter.rs:151-155, 311-317), the search into a device buffer (grown and searched
// again if it was too small) and the per-document apply. The kept records stay in HBM (`res`, inside
// `raw`), grouped by document, with their CSR index in `d_doc`; nothing but counts visits the host.
struct BatchKept {
  DevMem raw, doff;
  fac_match* res = nullptr;
  uint64_t n_res = 0;
  uint64_t* d_doc = nullptr;
  explicit BatchKept(hipStream_t st) : raw(st), doff(st) {}
};

// d_doc_user: where the index goes instead of the call's own scratch (may be NULL); searched
// (optional): += the start windows handed to the search launcher; anchors: the FAC_ANCHOR_* mask of
// the call (-1: the batch's own, fac_batch_require_anchors)
static int batch_kept(const fac::Engine& e, const fac::Batch& b, float threshold, int order, int overlap,
                      const uint64_t* unique_ids, bool prefilter, hipStream_t st, uint64_t* d_doc_user, fac_stats* stats,
                      BatchKept& k, std::string& err, uint64_t* searched = nullptr, const fac::StreamFilter* sf = nullptr,
                      int anchors = -1) {
  const uint64_t nd = b.n_docs;
  if (anchors < 0) anchors = b.anchors;
  fac::BatchWindows pw;  // pre-filtered: every document's merged windows, found once
  bool filtered = false;
  if (int rc = batch_prefilter(e, b, threshold, prefilter, st, pw, filtered, stats, err)) return rc;
  // anchored matches (fac.h fac_batch_require_anchors): a plain call searches only the start windows
  // a kept record can come from, through descriptors of its own (the batch's stay as they are). An
  // auto-beam-only engine's running total needs every window in order, and a pre-filtered call keeps
  // its merged windows: both get the filter below and nothing else.
  if (anchors && !prefilter && !(e.has_auto_beam && e.beam_width == 0) && b.n_segs) {
    if (int rc = fac::anchor_windows_device(e, b, anchors, st, pw, err)) return rc;
    filtered = true;
  }
  if (searched) *searched += filtered ? pw.windows : b.windows;
  uint64_t cap = std::max<uint64_t>({4096, (filtered ? pw.windows : b.windows) / 64, filtered ? pw.out_hint : 0});
  for (;;) {
    if (int rc = k.raw.alloc(2 * cap * sizeof(fac_match), err)) return rc;
    if (int rc = k.doff.alloc((nd + 1) * 8, err)) return rc;
    fac::MatchSink sink;
    sink.dev = static_cast<fac_match*>(k.raw.p);
    sink.dev_cap = cap;
    if (int rc = filtered ? fac::launch_search_batch_windows(e, b, pw, threshold, st, sink, stats, err)
                          : fac::launch_search_batch(e, b, threshold, st, sink, stats, err))
      return rc;
    if (stats) stats->graphemes = b.windows;
    if (sink.n > cap) {
      cap = sink.n;
      continue;
    }
    k.d_doc = d_doc_user ? d_doc_user : static_cast<uint64_t*>(k.doff.p);
    fac_match *recs = sink.dev, *other = sink.dev + cap;
    uint64_t n = sink.n;
    if (b.boundaries && n) {
      // whole-token matches (fac.h fac_batch_require_boundaries): the complete raw set is filtered
      // into the buffer's other half, before any overlap walk sees it; the index scratch lends the
      // kernel its counter (the apply writes the index afterwards)
      if (int rc = fac::boundary_filter_device(b, b.boundaries, recs, n, other, static_cast<unsigned long long*>(k.doff.p),
                                               st, &n, err))
        return rc;
      std::swap(recs, other);
    } else if (sf && n) {
      // the window documents of a flagged stream (fac.h fac_stream_open_opts): the stream's filter at
      // the same point, which reads a window's neighbours from the task's text and the carried
      // context (a document's start is no boundary there)
      if (int rc = fac::stream_boundary_filter_device(b.h.device, *sf, recs, n, other,
                                                      static_cast<unsigned long long*>(k.doff.p), st, &n, err))
        return rc;
      std::swap(recs, other);
    }
    if (anchors && n) {
      // the anchor rule on the complete raw set, at the same point and in the same way (a pure
      // predicate like the whole-token rule, so the order of the two passes does not matter); for a
      // narrowed START search it only drops what window 0 found away from byte 0
      if (int rc = fac::anchor_filter_device(b, anchors, recs, n, other, static_cast<unsigned long long*>(k.doff.p), st, &n,
                                             err))
        return rc;
      std::swap(recs, other);
    }
    return fac::apply_batch_device(e, recs, other, n, b.d_offsets, nd, order, overlap, unique_ids, st, k.d_doc, &k.res,
                                   &k.n_res, err);
  }
}

// The records of a batch call (d_res, n of them, and their CSR index d_doc) to the caller: into
// args->device_out, or a pinned host buffer handed out as *out; doc_offsets (host, may be NULL).
static int deliver_records(const fac_batch_args* args, const fac_match* d_res, uint64_t n, const uint64_t* d_doc,
                           uint64_t nd, hipStream_t st, fac_match** out, uint64_t* n_out, uint64_t* doc_offsets) {
  std::string err;
  fac::MatchSink fin;
  fin.dev = static_cast<fac_match*>(args->device_out);
  fin.dev_cap = args->device_cap;
  if (int rc = fac::sink_append_device(fin, d_res, n, st, err)) {
    fac::result_free(fin.pinned);
    return fail(rc, err);
  }
  if ((doc_offsets && hipMemcpyAsync(doc_offsets, d_doc, (nd + 1) * 8, hipMemcpyDeviceToHost, st) != hipSuccess) ||
      hipStreamSynchronize(st) != hipSuccess) {
    fac::result_free(fin.pinned);
    return fail(FAC_E_HIP, "copy of the batch's records failed");
  }
  if (fin.dev) return FAC_OK;
  return hand_out(fin, out, n_out);
}

// The body of fac_search_batch and fac_search_batch_prefiltered (prefilter: take the pre-filtered
// path where the reference's Prefiltered::search would, prefilter.rs:151-155, 311-317)
static int search_batch_impl(const fac_engine* engine, const fac_batch* batch, const fac_batch_args* args, fac_match** out,
                             uint64_t* n_out, uint64_t* doc_offsets, fac_stats* stats, bool prefilter) {
  if (!engine || !batch || !args || !n_out || (!out && !args->device_out)) return fail(FAC_E_INVALID, "NULL argument");
  if (args->order < 0 || args->order > 3 || args->overlap < 0 || args->overlap > 2)
    return fail(FAC_E_INVALID, "bad order/overlap");
  if (out) *out = nullptr;
  *n_out = 0;
  const fac::Engine& e = engine->e;
  const fac::Batch& b = batch->b;
  if (b.h.device != e.device) return fail(FAC_E_INVALID, "batch was staged for another device");
  if (e.has_map && !b.h.ascii && !b.unicode_map)
    return fail(FAC_E_UNSUPPORTED, "batches with non-ASCII documents do not support multi-character mappings");
  if (hipSetDevice(e.device) != hipSuccess) return fail(FAC_E_HIP, "hipSetDevice failed");
  hipStream_t st = args->stream ? static_cast<hipStream_t>(args->stream) : e.stream;
  const uint64_t nd = b.n_docs;
  std::string err;
  BatchKept k(st);
  if (int rc = batch_kept(e, b, args->threshold, args->order, args->overlap, args->unique_ids, prefilter, st,
                          args->device_doc_offsets, stats, k, err))
    return fail(rc, err);
  *n_out = k.n_res;
  if (args->device_out && k.n_res > args->device_cap)
    return fail(FAC_E_OUTPUT_CAPACITY, "device output buffer too small (*n_out = records needed)");
  return deliver_records(args, k.res, k.n_res, k.d_doc, nd, st, out, n_out, doc_offsets);
}

int fac_search_batch(const fac_engine* engine, const fac_batch* batch, const fac_batch_args* args, fac_match** out,
                     uint64_t* n_out, uint64_t* doc_offsets, fac_stats* stats) {
  return search_batch_impl(engine, batch, args, out, n_out, doc_offsets, stats, false);
}

int fac_search_batch_prefiltered(const fac_engine* engine, const fac_batch* batch, const fac_batch_args* args,
                                 fac_match** out, uint64_t* n_out, uint64_t* doc_offsets, fac_stats* stats) {
  return search_batch_impl(engine, batch, args, out, n_out, doc_offsets, stats, true);
}

// fac.h "Dictionary lookup of a batch": fac_search_batch's search with the WHOLE anchor and
// apply(order, Keep), then the dense table from the kept records in HBM
int fac_lookup_batch(const fac_engine* engine, const fac_batch* batch, const fac_lookup_args* args, fac_match** out,
                     uint32_t* found, fac_stats* stats) {
  if (!args) return fail(FAC_E_INVALID, "NULL argument");
  if (args->k == 0) return fail(FAC_E_INVALID, "k must be at least 1");
  if (args->order < 0 || args->order > 3) return fail(FAC_E_INVALID, "bad order");
  if (!engine || !batch || (!out && !args->device_out)) return fail(FAC_E_INVALID, "NULL argument");
  if (out) *out = nullptr;
  const fac::Engine& e = engine->e;
  const fac::Batch& b = batch->b;
  if (b.h.device != e.device) return fail(FAC_E_INVALID, "batch was staged for another device");
  if (e.has_map && !b.h.ascii && !b.unicode_map)
    return fail(FAC_E_UNSUPPORTED, "batches with non-ASCII documents do not support multi-character mappings");
  const uint64_t nd = b.n_docs, total = nd * (uint64_t)args->k;  // (nd <= 2^24, k < 2^32: no overflow)
  if (total >= (1ull << fac::kDocTagShift)) return fail(FAC_E_UNSUPPORTED, "a lookup table holds fewer than 2^40 records");
  if (args->device_out && args->device_cap < total)
    return fail(FAC_E_OUTPUT_CAPACITY, "device output buffer too small (n_docs * k records needed)");
  if (hipSetDevice(e.device) != hipSuccess) return fail(FAC_E_HIP, "hipSetDevice failed");
  hipStream_t st = args->stream ? static_cast<hipStream_t>(args->stream) : e.stream;
  const int order = args->order == 0 ? 1 : args->order;
  std::string err;
  BatchKept k(st);
  if (int rc = batch_kept(e, b, args->threshold, order, /*Keep*/ 0, nullptr, false, st, nullptr, stats, k, err, nullptr, nullptr,
                          FAC_ANCHOR_WHOLE))
    return fail(rc, err);
  DevMem tab(st), fnd(st);
  if (int rc = fnd.alloc(std::max<uint64_t>(nd, 1) * sizeof(uint32_t), err)) return fail(rc, err);
  fac_match* d_tab = static_cast<fac_match*>(args->device_out);
  if (!d_tab) {
    if (int rc = tab.alloc(std::max<uint64_t>(total, 1) * sizeof(fac_match), err)) return fail(rc, err);
    d_tab = static_cast<fac_match*>(tab.p);
  }
  if (int rc = fac::lookup_table_device(k.res, k.d_doc, nd, args->k, d_tab, static_cast<uint32_t*>(fnd.p), st, err))
    return fail(rc, err);
  fac::MatchSink fin;  // the host form: a pinned buffer handed out as *out
  if (!args->device_out)
    if (int rc = fac::sink_append_device(fin, d_tab, total, st, err)) {
      fac::result_free(fin.pinned);
      return fail(rc, err);
    }
  if ((found && nd && hipMemcpyAsync(found, fnd.p, nd * sizeof(uint32_t), hipMemcpyDeviceToHost, st) != hipSuccess) ||
      hipStreamSynchronize(st) != hipSuccess) {
    fac::result_free(fin.pinned);
    return fail(FAC_E_HIP, "copy of the lookup table failed");
  }
  if (args->device_out) return FAC_OK;
  uint64_t n_out = 0;
  return hand_out(fin, out, &n_out);
}

// ---- term counts (fac.h "Term counts of a batch"): search + apply with the options as passed, then
// the group-by of count_kernels.hip over the kept records in HBM

// The pattern -> key table's checks, made before anything runs; *eff: the keys the totals hold
static int count_keys_check(const uint32_t* keys, uint64_t n_patterns, uint64_t n_keys, uint64_t* eff) {
  if (!keys) {
    if (n_keys != 0 && n_keys != n_patterns)
      return fail(FAC_E_INVALID, "n_keys must be 0 or the pattern count when keys is NULL");
    *eff = n_patterns;
    return FAC_OK;
  }
  if (n_keys > 0xFFFFFFFFull) return fail(FAC_E_INVALID, "n_keys must be at most 2^32 - 1");
  for (uint64_t p = 0; p < n_patterns; ++p)
    if (keys[p] >= n_keys) return fail(FAC_E_INVALID, "a key is not below n_keys");
  *eff = n_keys;
  return FAC_OK;
}

// Pass 2, the totals and the copies of a planned count: the capacity is checked first, so a refused
// call has written to no device output.
static int count_deliver(const fac::CountPlan& plan, uint64_t n_keys, hipStream_t st, fac_term* device_out,
                         uint64_t device_cap, uint64_t* device_doc_offsets, fac_term_total* device_totals, fac_term** out,
                         uint64_t* n_out, uint64_t* doc_offsets, fac_term_total* totals) {
  const uint64_t nd = plan.n_docs, total = plan.total;
  *n_out = total;
  if (device_out && total > device_cap)
    return fail(FAC_E_OUTPUT_CAPACITY, "device output buffer too small (*n_out = terms needed)");
  std::string err;
  DevMem tbuf(st), totbuf(st);
  fac_term* d_terms = device_out;
  if (!d_terms) {
    if (int rc = tbuf.alloc(total * sizeof(fac_term), err)) return fail(rc, err);
    d_terms = static_cast<fac_term*>(tbuf.p);
  }
  if (int rc = fac::count_write_device(plan, d_terms, err)) return fail(rc, err);
  fac_term_total* d_tot = device_totals;
  if ((totals || device_totals) && n_keys) {
    if (!d_tot) {
      if (int rc = totbuf.alloc(n_keys * sizeof(fac_term_total), err)) return fail(rc, err);
      d_tot = static_cast<fac_term_total*>(totbuf.p);
    }
    if (int rc = fac::count_totals_device(d_terms, total, n_keys, d_tot, st, err)) return fail(rc, err);
  }
  fac_term* h_terms = nullptr;
  if (!device_out) {
    h_terms = static_cast<fac_term*>(std::malloc(std::max<uint64_t>(total, 1) * sizeof(fac_term)));
    if (!h_terms) return fail(FAC_E_OOM, "out of host memory");
  }
  if ((h_terms && total && hipMemcpyAsync(h_terms, d_terms, total * sizeof(fac_term), hipMemcpyDeviceToHost, st) != hipSuccess) ||
      (doc_offsets && hipMemcpyAsync(doc_offsets, plan.d_term_off, (nd + 1) * 8, hipMemcpyDeviceToHost, st) != hipSuccess) ||
      (device_doc_offsets &&
       hipMemcpyAsync(device_doc_offsets, plan.d_term_off, (nd + 1) * 8, hipMemcpyDeviceToDevice, st) != hipSuccess) ||
      (totals && n_keys &&
       hipMemcpyAsync(totals, d_tot, n_keys * sizeof(fac_term_total), hipMemcpyDeviceToHost, st) != hipSuccess) ||
      hipStreamSynchronize(st) != hipSuccess) {
    (void)hipStreamSynchronize(st);
    std::free(h_terms);
    return fail(FAC_E_HIP, "copy of the batch's terms failed");
  }
  if (h_terms) *out = h_terms;
  return FAC_OK;
}

// The body of fac_count_batch and fac_count_batch_prefiltered (prefilter: as search_batch_impl)
static int count_batch_impl(const fac_engine* engine, const fac_batch* batch, const fac_count_args* args, fac_term** out,
                            uint64_t* n_out, uint64_t* doc_offsets, fac_term_total* totals, fac_stats* stats,
                            bool prefilter) {
  if (!engine || !batch || !args || !n_out || (!out && !args->device_out)) return fail(FAC_E_INVALID, "NULL argument");
  if (args->order < 0 || args->order > 3 || args->overlap < 0 || args->overlap > 2)
    return fail(FAC_E_INVALID, "bad order/overlap");
  if (out) *out = nullptr;
  *n_out = 0;
  const fac::Engine& e = engine->e;
  const fac::Batch& b = batch->b;
  uint64_t n_keys = 0;
  if (int rc = count_keys_check(args->keys, e.pats.size(), args->n_keys, &n_keys)) return rc;
  if (b.h.device != e.device) return fail(FAC_E_INVALID, "batch was staged for another device");
  if (e.has_map && !b.h.ascii && !b.unicode_map)
    return fail(FAC_E_UNSUPPORTED, "batches with non-ASCII documents do not support multi-character mappings");
  if (hipSetDevice(e.device) != hipSuccess) return fail(FAC_E_HIP, "hipSetDevice failed");
  hipStream_t st = args->stream ? static_cast<hipStream_t>(args->stream) : e.stream;
  std::string err;
  BatchKept k(st);
  if (int rc = batch_kept(e, b, args->threshold, args->order, args->overlap, args->unique_ids, prefilter, st, nullptr, stats,
                          k, err))
    return fail(rc, err);
  fac::CountPlan plan;
  if (int rc = fac::count_plan_device(k.res, k.d_doc, b.n_docs, args->keys, e.pats.size(), 0, 0, st, plan, err))
    return fail(rc, err);
  return count_deliver(plan, n_keys, st, static_cast<fac_term*>(args->device_out), args->device_cap,
                       args->device_doc_offsets, args->device_totals, out, n_out, doc_offsets, totals);
}

int fac_count_batch(const fac_engine* engine, const fac_batch* batch, const fac_count_args* args, fac_term** out,
                    uint64_t* n_out, uint64_t* doc_offsets, fac_term_total* totals, fac_stats* stats) {
  return count_batch_impl(engine, batch, args, out, n_out, doc_offsets, totals, stats, false);
}

int fac_count_batch_prefiltered(const fac_engine* engine, const fac_batch* batch, const fac_count_args* args,
                                fac_term** out, uint64_t* n_out, uint64_t* doc_offsets, fac_term_total* totals,
                                fac_stats* stats) {
  return count_batch_impl(engine, batch, args, out, n_out, doc_offsets, totals, stats, true);
}

int64_t fac_count_records(const fac_match* recs, uint64_t n, const uint32_t* keys, uint64_t n_patterns, uint64_t n_keys,
                          fac_term* out, uint64_t cap) {
  if (n && !recs) return -(int64_t)fail(FAC_E_INVALID, "NULL argument");
  if (n >> 32) return -(int64_t)fail(FAC_E_UNSUPPORTED, "a document has 2^32 or more kept records");
  uint64_t eff = 0;
  if (int rc = count_keys_check(keys, n_patterns, n_keys, &eff)) return -(int64_t)rc;
  for (uint64_t i = 0; i < n; ++i)
    if (recs[i].pattern_index >= n_patterns) return -(int64_t)fail(FAC_E_INVALID, "a pattern_index is not below n_patterns");
  std::vector<fac_term> terms;
  fac::count_records_host(recs, n, keys, terms);
  if (out) {
    if (terms.size() > cap) return -(int64_t)fail(FAC_E_OUTPUT_CAPACITY, "term buffer too small");
    std::copy(terms.begin(), terms.end(), out);
  }
  return (int64_t)terms.size();
}

int fac_diag_count_terms(const fac_match* recs, uint64_t n, const uint64_t* doc_offsets, uint64_t n_docs,
                         const uint32_t* keys, uint64_t n_patterns, uint64_t n_keys, uint32_t lane_max, uint32_t group_max,
                         fac_term** out, uint64_t* n_out, uint64_t* term_offsets, fac_term_total* totals) {
  if (!doc_offsets || !out || !n_out || !term_offsets || (n && !recs)) return fail(FAC_E_INVALID, "NULL argument");
  *out = nullptr;
  *n_out = 0;
  if (lane_max > fac::kCountLaneMax || group_max > fac::kCountGroupMax)
    return fail(FAC_E_INVALID, "a tier ceiling above the built-in maximum");
  if (n_docs > fac::kBatchMaxDocs || n >= (1ull << fac::kDocTagShift)) return fail(FAC_E_UNSUPPORTED, "at most 2^24 documents");
  if (doc_offsets[0] != 0 || doc_offsets[n_docs] != n) return fail(FAC_E_INVALID, "doc_offsets must run from 0 to n");
  for (uint64_t d = 0; d < n_docs; ++d)
    if (doc_offsets[d] > doc_offsets[d + 1]) return fail(FAC_E_INVALID, "doc_offsets must ascend");
  uint64_t eff = 0;
  if (int rc = count_keys_check(keys, n_patterns, n_keys, &eff)) return rc;
  for (uint64_t i = 0; i < n; ++i)
    if (recs[i].pattern_index >= n_patterns) return fail(FAC_E_INVALID, "a pattern_index is not below n_patterns");
  if (int rc = check_device(0)) return rc;
  if (hipSetDevice(0) != hipSuccess) return fail(FAC_E_HIP, "hipSetDevice failed");
  hipStream_t st = nullptr;
  std::string err;
  DevMem drecs(st), ddoc(st);
  if (int rc = drecs.alloc(n * sizeof(fac_match), err)) return fail(rc, err);
  if (int rc = ddoc.alloc((n_docs + 1) * 8, err)) return fail(rc, err);
  if ((n && hipMemcpyAsync(drecs.p, recs, n * sizeof(fac_match), hipMemcpyHostToDevice, st) != hipSuccess) ||
      hipMemcpyAsync(ddoc.p, doc_offsets, (n_docs + 1) * 8, hipMemcpyHostToDevice, st) != hipSuccess)
    return fail(FAC_E_HIP, "upload of the records failed");
  fac::CountPlan plan;
  if (int rc = fac::count_plan_device(static_cast<const fac_match*>(drecs.p), static_cast<const uint64_t*>(ddoc.p), n_docs, keys,
                                      n_patterns, lane_max, group_max, st, plan, err))
    return fail(rc, err);
  return count_deliver(plan, eff, st, nullptr, 0, nullptr, nullptr, out, n_out, term_offsets, totals);
}

int64_t fac_batch_prefilter_windows(const fac_engine* engine, const fac_batch* batch, float threshold, void* stream,
                                    uint64_t* out, uint64_t cap) {
  if (!engine || !batch || (cap && !out)) return -(int64_t)fail(FAC_E_INVALID, "NULL argument");
  const fac::Engine& e = engine->e;
  const fac::Batch& b = batch->b;
  if (b.h.device != e.device) return -(int64_t)fail(FAC_E_INVALID, "batch was staged for another device");
  if (hipSetDevice(e.device) != hipSuccess) return -(int64_t)fail(FAC_E_HIP, "hipSetDevice failed");
  hipStream_t st = stream ? static_cast<hipStream_t>(stream) : e.stream;
  std::string err;
  fac::BatchWindows pw;
  pw.want_tri = !b.h.ascii;
  bool filtered = false;
  if (int rc = batch_prefilter(e, b, threshold, true, st, pw, filtered, nullptr, err)) return -(int64_t)fail(rc, err);
  if (!filtered) return -1;
  if (!b.h.ascii) {  // symbol offsets: a slice's descriptor holds bytes or batch-wide graphemes
    const uint64_t k = std::min(pw.n, cap);
    if (k && (hipMemcpyAsync(out, pw.d_tri, k * 24, hipMemcpyDeviceToHost, st) != hipSuccess ||
              hipStreamSynchronize(st) != hipSuccess))
      return -(int64_t)fail(FAC_E_HIP, "copy of the batch's merged windows failed");
    return (int64_t)pw.n;
  }
  // (diagnostics: the descriptors and the offsets come back to the host)
  std::vector<fac::SegDesc> segs(pw.n);
  std::vector<uint64_t> off(b.n_docs + 1, 0);
  if ((pw.n && hipMemcpyAsync(segs.data(), pw.d_segs, pw.n * sizeof(fac::SegDesc), hipMemcpyDeviceToHost, st) != hipSuccess) ||
      (b.n_docs && hipMemcpyAsync(off.data(), b.d_offsets, (b.n_docs + 1) * 8, hipMemcpyDeviceToHost, st) != hipSuccess) ||
      hipStreamSynchronize(st) != hipSuccess)
    return -(int64_t)fail(FAC_E_HIP, "copy of the batch's merged windows failed");
  for (uint64_t i = 0; i < pw.n && i < cap; ++i) {
    const uint64_t d = segs[i].byte_base >> fac::kDocTagShift, s0 = segs[i].text_base - off[d];
    out[3 * i] = d;
    out[3 * i + 1] = s0;
    out[3 * i + 2] = s0 + segs[i].n;
  }
  return (int64_t)pw.n;
}

// ---- batched replace (fac.h "Batched replace"): the table, then search + apply + splice

// insert_at NULL: fac_replacements_create
int fac_replacements_create_templates(const fac_engine* engine, const uint8_t* utf8, const uint64_t* offsets,
                                      const uint8_t* keep, const uint64_t* insert_at, uint64_t n_patterns,
                                      fac_replacements** out) {
  if (!engine || !out || !offsets) return fail(FAC_E_INVALID, "NULL argument");
  *out = nullptr;
  const fac::Engine& e = engine->e;
  if (n_patterns != e.pats.size()) return fail(FAC_E_INVALID, "the table needs one replacement per pattern of the engine");
  if (offsets[0] != 0) return fail(FAC_E_INVALID, "replacement offsets must start at 0");
  for (uint64_t p = 0; p < n_patterns; ++p)
    if (offsets[p + 1] < offsets[p]) return fail(FAC_E_INVALID, "replacement offsets must not decrease");
  const uint64_t bytes = offsets[n_patterns];
  if (bytes && !utf8) return fail(FAC_E_INVALID, "NULL argument");
  if (bytes >= (1ull << 32)) return fail(FAC_E_UNSUPPORTED, "a replacement table holds fewer than 2^32 bytes");
  std::vector<uint2> tab(std::max<uint64_t>(n_patterns, 1), make_uint2(0, 0));
  std::vector<uint32_t> ins;  // filled only once a template entry is met
  for (uint64_t p = 0; p < n_patterns; ++p) {
    const uint64_t b = offsets[p], len = offsets[p + 1] - b;
    if (keep && keep[p]) {
      tab[p] = make_uint2(0, fac::kReplaceKeep);
      continue;
    }
    if (!fac::utf8_valid(utf8 + b, len)) return fail(FAC_E_INVALID, "a replacement is not valid UTF-8");
    tab[p] = make_uint2((uint32_t)b, (uint32_t)len);
    if (insert_at && insert_at[p] != FAC_NO_INSERT) {
      const uint64_t k = insert_at[p];
      if (k > len) return fail(FAC_E_INVALID, "a template's insert position lies behind its replacement");
      if (k < len && (utf8[b + k] & 0xC0) == 0x80)
        return fail(FAC_E_INVALID, "a template's insert position lies inside a character");
      if (ins.empty()) ins.assign(tab.size(), fac::kReplaceNoInsert);
      ins[p] = (uint32_t)k;
    }
  }
  if (hipSetDevice(e.device) != hipSuccess) return fail(FAC_E_HIP, "hipSetDevice failed");
  fac_replacements* fr = new (std::nothrow) fac_replacements();
  if (!fr) return fail(FAC_E_OOM, "out of host memory");
  fac::ReplaceTable& t = fr->t;
  t.device = e.device;
  t.n_patterns = n_patterns;
  if (hipMalloc((void**)&t.d_tab, tab.size() * sizeof(uint2)) != hipSuccess ||
      hipMalloc((void**)&t.d_bytes, std::max<uint64_t>(bytes, 16)) != hipSuccess ||
      (!ins.empty() && hipMalloc((void**)&t.d_ins, ins.size() * sizeof(uint32_t)) != hipSuccess)) {
    fac_replacements_free(fr);
    return fail(FAC_E_OOM, "hipMalloc of the replacement table failed");
  }
  if (hipMemcpy(t.d_tab, tab.data(), tab.size() * sizeof(uint2), hipMemcpyHostToDevice) != hipSuccess ||
      (bytes && hipMemcpy(t.d_bytes, utf8, bytes, hipMemcpyHostToDevice) != hipSuccess) ||
      (t.d_ins && hipMemcpy(t.d_ins, ins.data(), ins.size() * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess)) {
    fac_replacements_free(fr);
    return fail(FAC_E_HIP, "upload of the replacement table failed");
  }
  *out = fr;
  return FAC_OK;
}

int fac_replacements_create(const fac_engine* engine, const uint8_t* utf8, const uint64_t* offsets,
                            const uint8_t* keep, uint64_t n_patterns, fac_replacements** out) {
  return fac_replacements_create_templates(engine, utf8, offsets, keep, nullptr, n_patterns, out);
}

void fac_replacements_free(fac_replacements* replacements) {
  if (!replacements) return;
  if (replacements->t.d_tab || replacements->t.d_bytes) (void)hipSetDevice(replacements->t.device);
  if (replacements->t.d_tab) (void)hipFree(replacements->t.d_tab);
  if (replacements->t.d_bytes) (void)hipFree(replacements->t.d_bytes);
  if (replacements->t.d_ins) (void)hipFree(replacements->t.d_ins);
  delete replacements;
}

// The output bytes of a batch call (d_out, total of them, and the n_docs + 1 offsets d_out_off) to
// the caller: they are in args->device_out already, or go to a host buffer handed out as *out; the
// offsets to args->device_out_offsets and out_offsets (host), where given.
static int deliver_bytes(const fac_replace_args* args, const uint8_t* d_out, uint64_t total, const uint64_t* d_out_off,
                         uint64_t nd, hipStream_t st, uint8_t** out, uint64_t* out_offsets) {
  uint8_t* host = nullptr;
  if (!args->device_out) {
    host = static_cast<uint8_t*>(std::malloc(std::max<uint64_t>(total, 1)));
    if (!host) return fail(FAC_E_OOM, "out of host memory");
  }
  if ((host && total && hipMemcpyAsync(host, d_out, total, hipMemcpyDeviceToHost, st) != hipSuccess) ||
      (args->device_out_offsets &&
       hipMemcpyAsync(args->device_out_offsets, d_out_off, (nd + 1) * 8, hipMemcpyDeviceToDevice, st) != hipSuccess) ||
      (out_offsets && hipMemcpyAsync(out_offsets, d_out_off, (nd + 1) * 8, hipMemcpyDeviceToHost, st) != hipSuccess) ||
      hipStreamSynchronize(st) != hipSuccess) {
    std::free(host);
    return fail(FAC_E_HIP, "copy of the batch's output failed");
  }
  if (host) *out = host;
  return FAC_OK;
}

// The body of fac_replace_batch and fac_replace_batch_prefiltered (prefilter: as search_batch_impl)
static int replace_batch_impl(const fac_engine* engine, const fac_batch* batch, const fac_replacements* replacements,
                              const fac_replace_args* args, uint8_t** out, uint64_t* out_len, uint64_t* out_offsets,
                              uint64_t* n_replaced, fac_stats* stats, bool prefilter) {
  if (!engine || !batch || !replacements || !args || !out_len || (!out && !args->device_out))
    return fail(FAC_E_INVALID, "NULL argument");
  if (args->order < 0 || args->order > 3 || args->overlap < 0 || args->overlap > 2)
    return fail(FAC_E_INVALID, "bad order/overlap");
  if (out) *out = nullptr;
  *out_len = 0;
  if (n_replaced) *n_replaced = 0;
  const fac::Engine& e = engine->e;
  const fac::Batch& b = batch->b;
  const fac::ReplaceTable& t = replacements->t;
  if (b.h.device != e.device) return fail(FAC_E_INVALID, "batch was staged for another device");
  if (t.device != e.device || t.n_patterns != e.pats.size())
    return fail(FAC_E_INVALID, "the replacement table was built for another engine");
  if (e.has_map && !b.h.ascii && !b.unicode_map)
    return fail(FAC_E_UNSUPPORTED, "batches with non-ASCII documents do not support multi-character mappings");
  if (hipSetDevice(e.device) != hipSuccess) return fail(FAC_E_HIP, "hipSetDevice failed");
  hipStream_t st = args->stream ? static_cast<hipStream_t>(args->stream) : e.stream;
  // `segmented` (query.rs:46-64): the splice needs start order and disjoint spans
  const int order = args->order == 0 ? 1 : args->order, overlap = args->overlap == 0 ? 1 : args->overlap;
  const uint64_t nd = b.n_docs;
  std::string err;
  // fac_search_batch's search and per-document apply, then the splice from the kept records in HBM
  BatchKept k(st);
  if (int rc = batch_kept(e, b, args->threshold, order, overlap, args->unique_ids, prefilter, st, nullptr, stats, k, err))
    return fail(rc, err);
  DevMem obuf(st);
  fac::ReplacePlan plan;
  if (int rc = fac::replace_plan_device(b, t, k.res, k.n_res, k.d_doc, st, plan, err)) return fail(rc, err);
  *out_len = plan.total;
  if (n_replaced) *n_replaced = plan.n_replaced;
  if (plan.total >= (1ull << fac::kDocTagShift))
    return fail(FAC_E_UNSUPPORTED, "the replaced batch would hold 2^40 bytes or more");
  if (args->device_out && plan.total > args->device_cap)
    return fail(FAC_E_OUTPUT_CAPACITY, "device output buffer too small (*out_len = bytes needed)");
  uint8_t* d_out = static_cast<uint8_t*>(args->device_out);
  if (!d_out) {
    if (int rc = obuf.alloc(plan.total, err)) return fail(rc, err);
    d_out = static_cast<uint8_t*>(obuf.p);
  }
  if (int rc = fac::replace_copy_device(b, t, k.res, k.d_doc, plan, d_out, err)) return fail(rc, err);
  return deliver_bytes(args, d_out, plan.total, plan.d_out_off, nd, st, out, out_offsets);
}

int fac_replace_batch(const fac_engine* engine, const fac_batch* batch, const fac_replacements* replacements,
                      const fac_replace_args* args, uint8_t** out, uint64_t* out_len, uint64_t* out_offsets,
                      uint64_t* n_replaced, fac_stats* stats) {
  return replace_batch_impl(engine, batch, replacements, args, out, out_len, out_offsets, n_replaced, stats, false);
}

int fac_replace_batch_prefiltered(const fac_engine* engine, const fac_batch* batch, const fac_replacements* replacements,
                                  const fac_replace_args* args, uint8_t** out, uint64_t* out_len, uint64_t* out_offsets,
                                  uint64_t* n_replaced, fac_stats* stats) {
  return replace_batch_impl(engine, batch, replacements, args, out, out_len, out_offsets, n_replaced, stats, true);
}

// ---- batched extraction (fac.h "Batched extraction"): search + apply with the options as passed,
// then one string per kept record

// The body of fac_extract_batch and fac_extract_batch_prefiltered (prefilter: as search_batch_impl)
static int extract_batch_impl(const fac_engine* engine, const fac_batch* batch, const fac_replacements* table,
                              const fac_extract_args* args, fac_match** records, uint64_t* n_items, uint64_t* doc_offsets,
                              uint8_t** text, uint64_t* text_len, uint64_t** item_offsets, fac_stats* stats,
                              bool prefilter) {
  if (!engine || !batch || !args || !n_items || !text_len) return fail(FAC_E_INVALID, "NULL argument");
  if (!args->device_records != !args->device_text)
    return fail(FAC_E_INVALID, "device_records and device_text are set together or not at all");
  if (!args->device_records && (!records || !text)) return fail(FAC_E_INVALID, "NULL argument");
  if (args->order < 0 || args->order > 3 || args->overlap < 0 || args->overlap > 2)
    return fail(FAC_E_INVALID, "bad order/overlap");
  if (records) *records = nullptr;
  if (text) *text = nullptr;
  if (item_offsets) *item_offsets = nullptr;
  *n_items = 0;
  *text_len = 0;
  const fac::Engine& e = engine->e;
  const fac::Batch& b = batch->b;
  const fac::ReplaceTable* t = table ? &table->t : nullptr;
  if (b.h.device != e.device) return fail(FAC_E_INVALID, "batch was staged for another device");
  if (t && (t->device != e.device || t->n_patterns != e.pats.size()))
    return fail(FAC_E_INVALID, "the replacement table was built for another engine");
  if (e.has_map && !b.h.ascii && !b.unicode_map)
    return fail(FAC_E_UNSUPPORTED, "batches with non-ASCII documents do not support multi-character mappings");
  if (hipSetDevice(e.device) != hipSuccess) return fail(FAC_E_HIP, "hipSetDevice failed");
  hipStream_t st = args->stream ? static_cast<hipStream_t>(args->stream) : e.stream;
  const uint64_t nd = b.n_docs;
  std::string err;
  BatchKept k(st);
  if (int rc = batch_kept(e, b, args->threshold, args->order, args->overlap, args->unique_ids, prefilter, st,
                          args->device_doc_offsets, stats, k, err))
    return fail(rc, err);
  DevMem obuf(st);
  fac::ExtractPlan plan;
  if (int rc = fac::extract_plan_device(b, t, k.res, k.n_res, k.d_doc, st, plan, err)) return fail(rc, err);
  *n_items = k.n_res;
  *text_len = plan.total;
  if (plan.total >= (1ull << fac::kDocTagShift))
    return fail(FAC_E_UNSUPPORTED, "the extracted text would hold 2^40 bytes or more");
  if (args->device_records && (k.n_res > args->device_record_cap || plan.total > args->device_text_cap))
    return fail(FAC_E_OUTPUT_CAPACITY,
                "device output buffer too small (*n_items = records, *text_len = bytes needed)");
  uint8_t* d_text = static_cast<uint8_t*>(args->device_text);
  if (!d_text) {
    if (int rc = obuf.alloc(plan.total, err)) return fail(rc, err);
    d_text = static_cast<uint8_t*>(obuf.p);
  }
  if (int rc = fac::extract_copy_device(b, t, k.res, plan, d_text, err)) return fail(rc, err);
  // the text and the item offsets travel on st; deliver_records synchronises it
  uint8_t* h_text = nullptr;
  uint64_t* h_off = nullptr;
  if (!args->device_text) {
    h_text = static_cast<uint8_t*>(std::malloc(std::max<uint64_t>(plan.total, 1)));
    if (!h_text) return fail(FAC_E_OOM, "out of host memory");
  }
  if (item_offsets) {
    h_off = static_cast<uint64_t*>(std::malloc((k.n_res + 1) * 8));
    if (!h_off) {
      std::free(h_text);
      return fail(FAC_E_OOM, "out of host memory");
    }
  }
  if ((h_text && plan.total && hipMemcpyAsync(h_text, d_text, plan.total, hipMemcpyDeviceToHost, st) != hipSuccess) ||
      (h_off && hipMemcpyAsync(h_off, plan.d_item_off, (k.n_res + 1) * 8, hipMemcpyDeviceToHost, st) != hipSuccess) ||
      (args->device_item_offsets && hipMemcpyAsync(args->device_item_offsets, plan.d_item_off, (k.n_res + 1) * 8,
                                                   hipMemcpyDeviceToDevice, st) != hipSuccess)) {
    (void)hipStreamSynchronize(st);
    std::free(h_text);
    std::free(h_off);
    return fail(FAC_E_HIP, "copy of the batch's extracted text failed");
  }
  fac_batch_args ra{};
  ra.device_out = args->device_records;
  ra.device_cap = args->device_record_cap;
  uint64_t n_recs = 0;
  if (int rc = deliver_records(&ra, k.res, k.n_res, k.d_doc, nd, st, records, &n_recs, doc_offsets)) {
    (void)hipStreamSynchronize(st);
    std::free(h_text);
    std::free(h_off);
    return rc;
  }
  if (h_text) *text = h_text;
  if (h_off) *item_offsets = h_off;
  return FAC_OK;
}

int fac_extract_batch(const fac_engine* engine, const fac_batch* batch, const fac_replacements* table,
                      const fac_extract_args* args, fac_match** records, uint64_t* n_items, uint64_t* doc_offsets,
                      uint8_t** text, uint64_t* text_len, uint64_t** item_offsets, fac_stats* stats) {
  return extract_batch_impl(engine, batch, table, args, records, n_items, doc_offsets, text, text_len, item_offsets,
                            stats, false);
}

int fac_extract_batch_prefiltered(const fac_engine* engine, const fac_batch* batch, const fac_replacements* table,
                                  const fac_extract_args* args, fac_match** records, uint64_t* n_items,
                                  uint64_t* doc_offsets, uint8_t** text, uint64_t* text_len, uint64_t** item_offsets,
                                  fac_stats* stats) {
  return extract_batch_impl(engine, batch, table, args, records, n_items, doc_offsets, text, text_len, item_offsets,
                            stats, true);
}

// ---- batched segmentation (fac.h "Batched segmentation"): search + apply, then the walk of
// matches.rs:218-594 over the kept records in HBM

// The body of fac_segment_batch and fac_segment_batch_prefiltered (prefilter: as search_batch_impl)
static int segment_batch_impl(const fac_engine* engine, const fac_batch* batch, const fac_batch_args* args,
                              fac_match** out, uint64_t* n_out, uint64_t* doc_offsets, fac_stats* stats, bool prefilter) {
  if (!engine || !batch || !args || !n_out || (!out && !args->device_out)) return fail(FAC_E_INVALID, "NULL argument");
  if (args->order < 0 || args->order > 3 || args->overlap < 0 || args->overlap > 2)
    return fail(FAC_E_INVALID, "bad order/overlap");
  if (out) *out = nullptr;
  *n_out = 0;
  const fac::Engine& e = engine->e;
  const fac::Batch& b = batch->b;
  if (b.h.device != e.device) return fail(FAC_E_INVALID, "batch was staged for another device");
  if (e.has_map && !b.h.ascii && !b.unicode_map)
    return fail(FAC_E_UNSUPPORTED, "batches with non-ASCII documents do not support multi-character mappings");
  if (hipSetDevice(e.device) != hipSuccess) return fail(FAC_E_HIP, "hipSetDevice failed");
  hipStream_t st = args->stream ? static_cast<hipStream_t>(args->stream) : e.stream;
  // `segmented` (query.rs:46-64): the walk needs start order and disjoint spans
  const int order = args->order == 0 ? 1 : args->order, overlap = args->overlap == 0 ? 1 : args->overlap;
  const uint64_t nd = b.n_docs;
  std::string err;
  BatchKept k(st);
  if (int rc = batch_kept(e, b, args->threshold, order, overlap, args->unique_ids, prefilter, st, nullptr, stats, k, err))
    return fail(rc, err);
  fac::SegmentPlan plan;
  if (int rc = fac::segment_plan_device(b, fac::kSegmentRecords, k.res, k.d_doc, st, plan, err)) return fail(rc, err);
  *n_out = plan.n_segs;
  if (args->device_out && plan.n_segs > args->device_cap)
    return fail(FAC_E_OUTPUT_CAPACITY, "device output buffer too small (*n_out = segments needed)");
  // (the caller's buffer may have any alignment: the segments are written to scratch and copied)
  DevMem segs(st);
  if (int rc = segs.alloc(plan.n_segs * sizeof(fac_match), err)) return fail(rc, err);
  if (int rc = fac::segment_write_device(b, k.res, k.d_doc, plan, static_cast<fac_match*>(segs.p), err))
    return fail(rc, err);
  if (args->device_doc_offsets &&
      hipMemcpyAsync(args->device_doc_offsets, plan.d_seg_off, (nd + 1) * 8, hipMemcpyDeviceToDevice, st) != hipSuccess)
    return fail(FAC_E_HIP, "copy of the batch's segment index failed");
  return deliver_records(args, static_cast<fac_match*>(segs.p), plan.n_segs, plan.d_seg_off, nd, st, out, n_out,
                         doc_offsets);
}

int fac_segment_batch(const fac_engine* engine, const fac_batch* batch, const fac_batch_args* args, fac_match** out,
                      uint64_t* n_out, uint64_t* doc_offsets, fac_stats* stats) {
  return segment_batch_impl(engine, batch, args, out, n_out, doc_offsets, stats, false);
}

int fac_segment_batch_prefiltered(const fac_engine* engine, const fac_batch* batch, const fac_batch_args* args,
                                  fac_match** out, uint64_t* n_out, uint64_t* doc_offsets, fac_stats* stats) {
  return segment_batch_impl(engine, batch, args, out, n_out, doc_offsets, stats, true);
}

// The body of fac_render_batch and fac_render_batch_prefiltered (prefilter: as search_batch_impl)
static int render_batch_impl(const fac_engine* engine, const fac_batch* batch, int32_t mode, const fac_replace_args* args,
                             uint8_t** out, uint64_t* out_len, uint64_t* out_offsets, fac_stats* stats, bool prefilter) {
  if (!engine || !batch || !args || !out_len || (!out && !args->device_out)) return fail(FAC_E_INVALID, "NULL argument");
  if (mode != FAC_RENDER_STRIP_PREFIX && mode != FAC_RENDER_STRIP_SUFFIX && mode != FAC_RENDER_SEGMENT_TEXT)
    return fail(FAC_E_INVALID, "bad render mode");
  if (args->order < 0 || args->order > 3 || args->overlap < 0 || args->overlap > 2)
    return fail(FAC_E_INVALID, "bad order/overlap");
  if (out) *out = nullptr;
  *out_len = 0;
  const fac::Engine& e = engine->e;
  const fac::Batch& b = batch->b;
  if (b.h.device != e.device) return fail(FAC_E_INVALID, "batch was staged for another device");
  if (e.has_map && !b.h.ascii && !b.unicode_map)
    return fail(FAC_E_UNSUPPORTED, "batches with non-ASCII documents do not support multi-character mappings");
  if (hipSetDevice(e.device) != hipSuccess) return fail(FAC_E_HIP, "hipSetDevice failed");
  hipStream_t st = args->stream ? static_cast<hipStream_t>(args->stream) : e.stream;
  const int order = args->order == 0 ? 1 : args->order, overlap = args->overlap == 0 ? 1 : args->overlap;
  const uint64_t nd = b.n_docs;
  std::string err;
  BatchKept k(st);
  if (int rc = batch_kept(e, b, args->threshold, order, overlap, args->unique_ids, prefilter, st, nullptr, stats, k, err))
    return fail(rc, err);
  DevMem obuf(st);
  fac::SegmentPlan plan;
  if (int rc = fac::segment_plan_device(b, mode, k.res, k.d_doc, st, plan, err)) return fail(rc, err);
  *out_len = plan.total;
  if (plan.total >= (1ull << fac::kDocTagShift))
    return fail(FAC_E_UNSUPPORTED, "the rendered batch would hold 2^40 bytes or more");
  if (args->device_out && plan.total > args->device_cap)
    return fail(FAC_E_OUTPUT_CAPACITY, "device output buffer too small (*out_len = bytes needed)");
  uint8_t* d_out = static_cast<uint8_t*>(args->device_out);
  if (!d_out) {
    if (int rc = obuf.alloc(plan.total, err)) return fail(rc, err);
    d_out = static_cast<uint8_t*>(obuf.p);
  }
  if (int rc = fac::render_copy_device(b, k.res, k.d_doc, plan, d_out, err)) return fail(rc, err);
  return deliver_bytes(args, d_out, plan.total, plan.d_out_off, nd, st, out, out_offsets);
}

int fac_render_batch(const fac_engine* engine, const fac_batch* batch, int32_t mode, const fac_replace_args* args,
                     uint8_t** out, uint64_t* out_len, uint64_t* out_offsets, fac_stats* stats) {
  return render_batch_impl(engine, batch, mode, args, out, out_len, out_offsets, stats, false);
}

int fac_render_batch_prefiltered(const fac_engine* engine, const fac_batch* batch, int32_t mode,
                                 const fac_replace_args* args, uint8_t** out, uint64_t* out_len, uint64_t* out_offsets,
                                 fac_stats* stats) {
  return render_batch_impl(engine, batch, mode, args, out, out_len, out_offsets, stats, true);
}

int fac_stream_open(const fac_engine* engine, float threshold, uint64_t window_bytes, fac_stream** out) {
  return fac_stream_open_ex(engine, threshold, window_bytes, 0, out);
}

int fac_stream_open_ex(const fac_engine* engine, float threshold, uint64_t window_bytes, int32_t prefilter,
                       fac_stream** out) {
  const fac_stream_options o{threshold, window_bytes, prefilter, 0};
  return fac_stream_open_opts(engine, &o, out);
}

int fac_stream_open_opts(const fac_engine* engine, const fac_stream_options* options, fac_stream** out) {
  if (!engine || !options || !out) return fail(FAC_E_INVALID, "NULL argument");
  if (options->boundaries < 0 || options->boundaries > FAC_BOUNDARY_WHOLE) return fail(FAC_E_INVALID, "boundaries must be 0..3");
  fac_stream* fs = new (std::nothrow) fac_stream();
  if (!fs) return fail(FAC_E_OOM, "out of host memory");
  fs->s = fac::stream_open(engine->e, options->threshold, options->window_bytes, nullptr, options->prefilter != 0,
                           options->boundaries);
  *out = fs;
  return FAC_OK;
}

uint64_t fac_stream_windows_searched(const fac_stream* stream) { return stream ? stream->s->windows_searched : 0; }

static void task_counts(const fac::StreamCore* s, uint64_t* batched, uint64_t* single) {
  if (batched) *batched = s ? s->tasks_batched : 0;
  if (single) *single = s ? s->tasks_single : 0;
}

void fac_stream_task_counts(const fac_stream* stream, uint64_t* batched, uint64_t* single) {
  task_counts(stream ? stream->s : nullptr, batched, single);
}

void fac_replace_stream_task_counts(const fac_replace_stream* stream, uint64_t* batched, uint64_t* single) {
  task_counts(stream ? stream->s : nullptr, batched, single);
}

int fac_stream_feed(fac_stream* stream, const uint8_t* data, uint64_t len, int32_t eof, fac_match** out,
                    uint64_t* n_out, uint8_t** text, uint64_t* text_len) {
  if (!stream || !out || !n_out || !text || !text_len || (len && !data)) return fail(FAC_E_INVALID, "NULL argument");
  *out = nullptr;
  *n_out = 0;
  *text = nullptr;
  *text_len = 0;
  std::string err;
  fac::StreamCore& s = *stream->s;
  const int rc = fac::stream_feed(s, data, len, eof != 0, err);
  if (rc) return fail(rc, err);
  int r = copy_out(s.ready, out, n_out);
  if (r) return r;
  *text_len = s.ready_text.size();
  *text = static_cast<uint8_t*>(std::malloc(std::max<size_t>(s.ready_text.size(), 1)));
  if (!*text) return fail(FAC_E_OOM, "out of host memory");
  if (!s.ready_text.empty()) std::memcpy(*text, s.ready_text.data(), s.ready_text.size());
  s.ready.clear();
  s.ready_text.clear();
  return FAC_OK;
}

uint64_t fac_stream_total(const fac_stream* stream) { return stream ? stream->s->total : 0; }
uint64_t fac_stream_committed(const fac_stream* stream) { return stream ? fac::stream_committed(*stream->s) : 0; }

void fac_stream_close(fac_stream* stream) {
  if (!stream) return;
  fac::stream_close(stream->s);
  delete stream;
}

int fac_replace_stream_open(const fac_engine* engine, const fac_replacements* replacements, float threshold,
                            uint64_t window_bytes, fac_replace_stream** out) {
  return fac_replace_stream_open_ex(engine, replacements, threshold, window_bytes, 0, out);
}

uint64_t fac_replace_stream_windows_searched(const fac_replace_stream* stream) {
  return stream ? stream->s->windows_searched : 0;
}

int fac_replace_stream_open_ex(const fac_engine* engine, const fac_replacements* replacements, float threshold,
                               uint64_t window_bytes, int32_t prefilter, fac_replace_stream** out) {
  const fac_stream_options o{threshold, window_bytes, prefilter, 0};
  return fac_replace_stream_open_opts(engine, replacements, &o, out);
}

int fac_replace_stream_open_opts(const fac_engine* engine, const fac_replacements* replacements,
                                 const fac_stream_options* options, fac_replace_stream** out) {
  if (!engine || !replacements || !options || !out) return fail(FAC_E_INVALID, "NULL argument");
  *out = nullptr;
  if (options->boundaries < 0 || options->boundaries > FAC_BOUNDARY_WHOLE) return fail(FAC_E_INVALID, "boundaries must be 0..3");
  if (replacements->t.device != engine->e.device || replacements->t.n_patterns != engine->e.pats.size())
    return fail(FAC_E_INVALID, "the replacement table was built for another engine");
  fac_replace_stream* fs = new (std::nothrow) fac_replace_stream();
  if (!fs) return fail(FAC_E_OOM, "out of host memory");
  fs->s = fac::stream_open(engine->e, options->threshold, options->window_bytes, &replacements->t, options->prefilter != 0,
                           options->boundaries);
  *out = fs;
  return FAC_OK;
}

int fac_replace_stream_feed(fac_replace_stream* stream, const uint8_t* data, uint64_t len, int32_t eof, uint8_t** out,
                            uint64_t* out_len) {
  if (!stream || !out || !out_len || (len && !data)) return fail(FAC_E_INVALID, "NULL argument");
  *out = nullptr;
  *out_len = 0;
  std::string err;
  fac::StreamCore& s = *stream->s;
  const int rc = fac::stream_feed(s, data, len, eof != 0, err);
  if (rc) return fail(rc, err);
  *out = static_cast<uint8_t*>(std::malloc(std::max<size_t>(s.ready_out.size(), 1)));
  if (!*out) return fail(FAC_E_OOM, "out of host memory");
  if (!s.ready_out.empty()) std::memcpy(*out, s.ready_out.data(), s.ready_out.size());
  *out_len = s.ready_out.size();
  s.ready_out.clear();
  return FAC_OK;
}

uint64_t fac_replace_stream_written(const fac_replace_stream* stream) { return stream ? stream->s->written : 0; }

void fac_replace_stream_counts(const fac_replace_stream* stream, uint64_t* applied, uint64_t* skipped) {
  if (applied) *applied = stream ? stream->s->applied : 0;
  if (skipped) *skipped = stream ? stream->s->skipped : 0;
}

void fac_replace_stream_close(fac_replace_stream* stream) {
  if (!stream) return;
  fac::stream_close(stream->s);
  delete stream;
}

void fac_buffer_free(void* p) { std::free(p); }

int64_t fac_prefilter_windows(const fac_engine* engine, const uint8_t* utf8, uint64_t len, float threshold,
                              uint64_t* out, uint64_t cap) {
  if (!engine) return fail(FAC_E_INVALID, "NULL argument"), -1;
  const fac::Engine& e = engine->e;
  std::vector<uint32_t> ks;
  if (!e.bitap_ok || !prefilter_ks(e, threshold, ks)) return -1;
  fac_haystack* hay = nullptr;
  if (fac_haystack_stage(engine, utf8, len, &hay, nullptr)) return -1;
  std::string err;
  std::vector<std::pair<uint64_t, uint64_t>> windows;
  int rc = fac::prefilter_windows(e, hay->h, whole(hay->h), ks, nullptr, windows, nullptr, err);
  fac_haystack_free(hay);
  if (rc) return fail(rc, err), -1;
  for (size_t i = 0; i < windows.size() && i < cap; ++i) {
    out[2 * i] = windows[i].first;
    out[2 * i + 1] = windows[i].second;
  }
  return (int64_t)windows.size();
}

uint64_t fac_segment_graphemes(const uint8_t* utf8, uint64_t len, uint64_t* starts, uint64_t cap) {
  std::vector<uint64_t> s;
  fac::segment_graphemes(utf8, len, s);
  for (uint64_t i = 0; i < s.size() && i < cap; ++i) starts[i] = s[i];
  return s.size();
}

uint32_t fac_fold_first_char(const uint8_t* utf8, uint64_t len, int32_t case_insensitive) {
  return fac::fold_first_char(utf8, 0, len, case_insensitive != 0);
}

void fac_edge_order(const uint32_t* cps, const uint64_t* off, uint64_t n, uint32_t* order) {
  std::vector<std::u32string> g(n);
  for (uint64_t i = 0; i < n; ++i) g[i].assign(cps + off[i], cps + off[i + 1]);
  const std::vector<uint32_t> o = fac::transitions_order(g);
  for (uint64_t i = 0; i < n; ++i) order[i] = o[i];
}

int fac_diag_beam_select(const float* keys, const uint64_t* offs, uint64_t count, uint32_t bw, int32_t lds,
                         int32_t sel_limit, uint32_t* perm) {
  if (!keys || !offs || !perm) return fail(FAC_E_INVALID, "null argument");
  if (int rc = check_device(0)) return rc;
  std::string err;
  int rc = fac::diag_beam_select(keys, offs, count, bw, lds, sel_limit, perm, err);
  return rc ? fail(rc, err) : FAC_OK;
}

void fac_engine_drop_prefix_cache(fac_engine* engine) {
  if (!engine) return;
  fac::Engine& e = engine->e;
  if (hipSetDevice(e.device) != hipSuccess) return;
  std::lock_guard<std::mutex> lk(e.rc_store.mu);  // waits for a search that holds the store
  fac::rc_store_drop(e.rc_store);
}

int fac_diag_rc_store_decide(int32_t valid, uint64_t calls, uint64_t used, uint64_t cap, uint64_t last_call,
                             int32_t pending, const uint32_t* have_sig, const uint32_t* want_sig, uint64_t want_cap,
                             uint64_t cap_limit, const uint64_t* dir_slots, const uint64_t* dir_keys, int32_t busy,
                             uint32_t sleep) {
  if (!have_sig || !want_sig || !dir_slots || !dir_keys) return fail(FAC_E_INVALID, "null argument");
  fac::RcStore s;
  s.valid = valid != 0;
  s.calls = calls;
  s.sleep = sleep;
  s.used = used;
  s.cap = cap;
  s.last_call = last_call;
  s.pending = pending;
  std::memcpy(s.sig, have_sig, sizeof(s.sig));
  for (int k = 0; k < 9; ++k) {
    s.dir[k].n_slots = (uint32_t)dir_slots[k];
    s.dir[k].count = dir_keys[k];
  }
  // the call's own steps: try-lock first (from a second thread, as a second call would), then decide
  std::unique_lock<std::mutex> held(s.mu, std::defer_lock);
  if (busy) held.lock();
  int r = fac::kRcBusy;
  std::thread t([&] {
    std::unique_lock<std::mutex> lk(s.mu, std::try_to_lock);
    if (lk.owns_lock()) r = fac::rc_store_decide(s, want_sig, want_cap, cap_limit);
  });
  t.join();
  return r;
}

const char* fac_diag_rc_reset_name(int32_t reset) { return fac::rc_reset_name(reset); }

uint32_t fac_diag_rc_store_gate(uint64_t carried, uint64_t built, uint32_t backoff, uint64_t gate_min) {
  return fac::rc_store_gate(carried, built, backoff, gate_min);
}

uint32_t fac_diag_rc_emptied_gate(int32_t decision, int32_t after_fill, uint32_t backoff) {
  return fac::rc_store_emptied_gate(decision, after_fill != 0, backoff);
}

int32_t fac_diag_rc_direct_decide(uint32_t unknown_pm, int32_t floor_pm, uint32_t margin_pm, uint64_t sampled,
                                  uint64_t windows, uint64_t min_windows) {
  return fac::rc_direct_decide(unknown_pm, floor_pm, margin_pm, sampled, windows, min_windows) ? 1 : 0;
}

int fac_diag_stream_gather(const fac_engine* engine, const uint8_t* utf8, uint64_t len, const uint64_t* windows,
                           uint64_t n_windows, uint8_t* out, uint64_t cap, uint64_t* offsets) {
  if (!engine || !offsets || (len && !utf8) || (n_windows && !windows) || (cap && !out))
    return fail(FAC_E_INVALID, "NULL argument");
  if (n_windows > fac::kBatchMaxDocs) return fail(FAC_E_UNSUPPORTED, "at most 2^24 windows");
  const fac::Engine& e = engine->e;
  if (hipSetDevice(e.device) != hipSuccess) return fail(FAC_E_HIP, "hipSetDevice failed");
  std::vector<uint64_t> tab(2 * n_windows + 1, 0);  // sources, then lengths and their closing entry
  uint64_t total = 0;
  for (uint64_t w = 0; w < n_windows; ++w) {
    const uint64_t off = windows[2 * w], wl = windows[2 * w + 1];
    if (off > len || wl > len - off) return fail(FAC_E_INVALID, "a window lies outside the text");
    tab[w] = off;
    tab[n_windows + w] = wl;
    total += wl;
  }
  if (total > cap) return fail(FAC_E_OUTPUT_CAPACITY, "output buffer too small");
  hipStream_t st = e.stream;
  std::string err;
  DevMem d_text(st), d_tab(st), d_off(st), d_out(st);
  if (int rc = d_text.alloc(len, err)) return fail(rc, err);
  if (int rc = d_tab.alloc(tab.size() * 8, err)) return fail(rc, err);
  if (int rc = d_off.alloc((n_windows + 1) * 8, err)) return fail(rc, err);
  if (int rc = d_out.alloc(total, err)) return fail(rc, err);
  const uint64_t* dt = static_cast<const uint64_t*>(d_tab.p);
  int rc = FAC_OK;
  if ((len && hipMemcpyAsync(d_text.p, utf8, len, hipMemcpyHostToDevice, st) != hipSuccess) ||
      hipMemcpyAsync(d_tab.p, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, st) != hipSuccess) {
    rc = FAC_E_HIP;
    err = "upload of the windows failed";
  }
  if (!rc)
    rc = fac::stream_gather_device(static_cast<const uint8_t*>(d_text.p), len, dt, dt + n_windows, n_windows, total,
                                   static_cast<uint8_t*>(d_out.p), static_cast<uint64_t*>(d_off.p), st, err);
  if (!rc && ((total && hipMemcpyAsync(out, d_out.p, total, hipMemcpyDeviceToHost, st) != hipSuccess) ||
              hipMemcpyAsync(offsets, d_off.p, (n_windows + 1) * 8, hipMemcpyDeviceToHost, st) != hipSuccess)) {
    rc = FAC_E_HIP;
    err = "copy of the expanded text failed";
  }
  if (hipStreamSynchronize(st) != hipSuccess && !rc) {
    rc = FAC_E_HIP;
    err = "the gather of the windows failed";
  }
  return rc ? fail(rc, err) : FAC_OK;
}

}  // extern "C"

namespace fac {

// A task of stream windows as one batch of window documents (stream.rs window_matches for each,
// :262-297): document w is window w's text, staged as if it were staged alone (stage_batch_device),
// so a window's segmentation starts and ends with its own bytes whatever its neighbours hold. The
// table of the windows (sources, lengths, commit points, rebase offsets) is the only upload; the
// expanded text, the offsets, the staging, the search, the per-document rank and overlap walk and
// the commit cut run on the device, and only the owned records and their index come back.
int stream_windows_docs(const Engine& e, WindowDocs& wd, const uint8_t* d_text, uint64_t text_len, const uint64_t* wins,
                        uint64_t n_windows, float threshold, bool prefilter, hipStream_t st, std::vector<fac_match>& owned,
                        std::string& err, std::vector<uint64_t>& win_off, uint64_t* searched, const StreamBoundary* sb) {
  owned.clear();
  win_off.assign(n_windows + 1, 0);
  if (n_windows == 0) return FAC_OK;
  if (n_windows > kBatchMaxDocs) return FAC_E_UNSUPPORTED;
  const uint64_t n = n_windows;
  const bool flagged = sb && sb->sides;
  // sources [0, n), lengths and their closing entry [n, 2n], commit points, rebase offsets; for
  // whole-token matches (fac.h fac_stream_open_opts) the carried context travels behind them
  std::vector<uint64_t> tab(4 * n + 1 + (flagged ? kBoundaryCarry / 8 : 0), 0);
  const uint32_t cn = flagged ? std::min<uint32_t>(sb->before_len, kBoundaryCarry) : 0;
  if (cn) std::memcpy(tab.data() + 4 * n + 1, sb->before + (sb->before_len - cn), cn);
  uint64_t total = 0;
  for (uint64_t w = 0; w < n; ++w) {
    const uint64_t off = wins[4 * w], end = wins[4 * w + 1];
    if (off > end || end > text_len) {
      err = "a stream window lies outside its task's text";
      return FAC_E_INTERNAL;
    }
    tab[w] = off;
    tab[n + w] = end - off;
    tab[2 * n + 1 + w] = wins[4 * w + 2];
    tab[3 * n + 1 + w] = wins[4 * w + 3];
    total += end - off;
  }
  if (total >= (1ull << kDocTagShift)) return FAC_E_UNSUPPORTED;
  Batch& b = wd.b;
  b.h.device = e.device;
  if (wd.text_cap < std::max<uint64_t>(total, 16)) {
    if (b.h.d_utf8) HIP_TRY(hipFree(b.h.d_utf8));
    b.h.d_utf8 = nullptr;
    wd.text_cap = 0;
    const uint64_t want = std::max<uint64_t>(total + total / 8, 16);
    HIP_TRY(hipMalloc((void**)&b.h.d_utf8, want));
    wd.text_cap = want;
  }
  b.h.own_utf8 = true;
  if (b.offsets_cap < n + 1) {
    if (b.d_offsets) HIP_TRY(hipFree(b.d_offsets));
    b.d_offsets = nullptr;
    b.offsets_cap = 0;
    HIP_TRY(hipMalloc((void**)&b.d_offsets, (n + 1 + n / 8) * 8));
    b.offsets_cap = n + 1 + n / 8;
  }
  b.own_offsets = true;
  b.h.len = total;
  b.n_docs = n;
  b.unicode_pf = true;
  b.unicode_map = true;
  b.long_docs = true;  // a window is 256 KiB: segmented by chunks, not by one thread
  DevMem d_tab(st);
  if (int rc = d_tab.alloc(tab.size() * 8, err)) return rc;
  const uint64_t* dt = static_cast<const uint64_t*>(d_tab.p);
  int rc = FAC_OK;
  if (hipMemcpyAsync(d_tab.p, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, st) != hipSuccess) {
    rc = FAC_E_HIP;
    err = "upload of a stream task's windows failed";
  }
  if (!rc) rc = stream_gather_device(d_text, text_len, dt, dt + n, n, total, b.h.d_utf8, b.d_offsets, st, err);
  if (!rc) rc = stage_batch_device(e, b, st, err);  // (synchronises: the table has been read)
  if (rc) {
    (void)hipStreamSynchronize(st);
    b.n_docs = 0;  // a failed staging leaves an empty batch
    b.n_segs = 0;
    b.windows = 0;
    b.h.len = 0;
    b.h.n = 0;
    // search_raw's error of the first window that fails: HaystackTooLarge has no message of its own
    if (rc == FAC_E_HAYSTACK_TOO_LARGE) err.clear();
    return rc;
  }
  BatchKept k(st);
  StreamFilter sf;
  if (flagged) {  // the window documents never take the batch filter: a document's start is no boundary here
    sf.sides = sb->sides;
    sf.d_text = d_text;
    sf.text_len = text_len;
    sf.d_src = dt;
    sf.d_len = dt + n;
    sf.d_doc_off = b.d_offsets;
    sf.n_windows = n;
    sf.d_before = reinterpret_cast<const uint8_t*>(dt + 4 * n + 1);
    sf.before_len = cn;
  }
  if ((rc = batch_kept(e, b, threshold, /*Default*/ 1, /*NonOverlapping*/ 1, nullptr, prefilter, st, nullptr, nullptr, k, err,
                       searched, flagged ? &sf : nullptr)))
    return rc;
  return windows_owned_device(k.res, k.n_res, k.d_doc, n, dt + 2 * n + 1, dt + 3 * n + 1, st, owned, win_off, err);
}

}  // namespace fac
