// device_state.cpp — host-only device state: the engine's tables and streams, a haystack's device
// buffers and host copies, the per-worker scratch sets. Allocations and copies only, no kernel.
#include <cstring>

#include "host_util.h"

namespace fac {

void scratch_free(ScratchSet& s) {
  if (s.aux) {
    call_scratch_release_stream(s.aux);
    (void)hipStreamDestroy(s.aux);
    s.aux = nullptr;
  }
  for (int i = 0; i < ScratchSet::kSlots; ++i)
    if (s.p[i]) {
      (void)hipFree(s.p[i]);
      s.p[i] = nullptr;
      s.n[i] = 0;
    }
}

int aux_priority() {
  int least = 0, greatest = 0;
  if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) return 0;
  return diag_env("FAC_L1_HIGH") ? greatest : least;
}

int upload_engine(Engine& e, std::string& err) {
  HIP_TRY(hipSetDevice(e.device));
  if (!e.stream) HIP_TRY(hipStreamCreateWithFlags(&e.stream, hipStreamNonBlocking));
  if (!e.aux_stream) HIP_TRY(hipStreamCreateWithPriority(&e.aux_stream, hipStreamNonBlocking, aux_priority()));
  int rc;
  if ((rc = upload(e.dnodes, &e.d_nodes, err))) return rc;
  if ((rc = upload(e.out_range, &e.d_out_range, err))) return rc;
  if ((rc = upload(e.node_pidx, &e.d_pidx, err))) return rc;
  if ((rc = upload(e.edges, &e.d_edges, err))) return rc;
  if ((rc = upload(e.out_pat, &e.d_out_pat, err))) return rc;
  if ((rc = upload(e.sb_edge, &e.d_sb_edge, err))) return rc;
  if ((rc = upload(e.gt, &e.d_gt, err))) return rc;
  if ((rc = upload(e.aux, &e.d_aux, err))) return rc;
  if ((rc = upload(e.pat_bytes, &e.d_pat_bytes, err))) return rc;
  if ((rc = upload(e.pats, &e.d_pats, err))) return rc;
  if ((rc = upload(e.sim_ascii, &e.d_sim_ascii, err))) return rc;
  if ((rc = upload(e.sim_keys, &e.d_sim_keys, err))) return rc;
  if ((rc = upload(e.sim_vals, &e.d_sim_vals, err))) return rc;
  if (e.has_map) {
    if ((rc = upload(e.edge_gid, &e.d_edge_gid, err))) return rc;
    std::vector<uint32_t> ag(e.ascii_gid, e.ascii_gid + 128);
    if ((rc = upload(ag, &e.d_ascii_gid, err))) return rc;
    if ((rc = upload(e.map_range, &e.d_map_range, err))) return rc;
    if ((rc = upload(e.map_ent, &e.d_map_ent, err))) return rc;
    if ((rc = upload(e.map_hay, &e.d_map_hay, err))) return rc;
    // folded grapheme -> dictionary id, for the ids of Unicode text (grapheme_ids_kernel); sorted, so
    // the table does not depend on the hash map's iteration order
    std::vector<std::pair<std::u32string, uint32_t>> keys(e.gid_of.begin(), e.gid_of.end());
    std::sort(keys.begin(), keys.end());
    if ((rc = grapheme_table_build(keys, e.gid_tab, e.stream, err))) return rc;
  }
  if (e.bitap_ok) {
    // the packed masks depend on the per-call edit budgets: prefilter_windows builds them
    std::vector<uint8_t> aid(e.ascii_id, e.ascii_id + 128);
    if ((rc = upload(aid, &e.d_ascii_id, err))) return rc;
    // folded pattern grapheme -> symbol id, for the transcode of Unicode text (symbol_ids_kernel)
    if ((rc = grapheme_table_build(e.symbol_ids, e.sym_tab, e.stream, err))) return rc;
  }
  // Pageable hipMemcpy may return before the DMA lands and the engine's stream is non-blocking:
  // make the tables visible to every stream before the first launch.
  HIP_TRY(hipDeviceSynchronize());
  return FAC_OK;
}

// ---------------------------------------------------------------- the engine's snapshot store
// (launch_pass in search_kernels.hip is the only user)
const char* rc_reset_name(int r) {
  switch (r) {
    case kRcKeep: return "none";
    case kRcFresh: return "fresh";
    case kRcSignature: return "signature";
    case kRcPool: return "pool";
    case kRcDirectory: return "directory";
    case kRcBusy: return "busy";
    case kRcGated: return "gated";
    default: return "off";
  }
}

bool rc_dir_fits(const RcStoreDir& d, uint64_t n) { return d.n_slots && 2 * (d.count + n) <= d.n_slots; }

// Unlike text must not pay for the store (its probes, inserts and the directories' clears; measured
// +1.0 % per call on fresh-word C3 haystacks): a carrying call of at least gate_min
// entries that found under a tenth of them doubles the back-off (1 .. 64 calls), any other ends it.
uint32_t rc_store_gate(uint64_t carried, uint64_t built, uint32_t backoff, uint64_t gate_min) {
  if (carried + built < gate_min || 10 * carried >= carried + built) return 0;
  return backoff ? std::min<uint32_t>(64, 2 * backoff) : 1;
}

// Fresh-word text fills the pool in one call, so every call after it starts the store empty for `pool`
// or `directory` and pays the clears and inserts for nothing, and the gate above, which judges carrying
// calls only, never sees one. A call that empties the store for either reason right after the call that
// filled it from empty doubles the back-off as a carrying call under a tenth does, and goes without the
// store itself. (A signature reset is the caller's doing, not the text's: it does not count.)
uint32_t rc_store_emptied_gate(int decision, bool after_fill, uint32_t backoff) {
  if (!after_fill || (decision != kRcPool && decision != kRcDirectory)) return 0;
  return backoff ? std::min<uint32_t>(64, 2 * backoff) : 1;
}

// Keys seen once are never selected, so some share of a text's windows is unknown even on the call
// after a full one over the same text: the floor. A call within margin_pm of it would build next to
// nothing. Below min_windows the sample says little (and few windows cost little either way).
bool rc_direct_decide(uint32_t unknown_pm, int32_t floor_pm, uint32_t margin_pm, uint64_t sampled, uint64_t windows,
                      uint64_t min_windows) {
  if (floor_pm < 0 || sampled == 0 || windows < min_windows) return false;
  return (uint64_t)unknown_pm <= (uint64_t)floor_pm + margin_pm;
}

int rc_store_decide(const RcStore& s, const uint32_t sig[kRcSigWords], uint64_t want_cap, uint64_t cap_limit) {
  if (s.sleep) return kRcGated;  // (the caller counts the call and goes without the store)
  if (!s.valid || s.used == 0) return kRcFresh;
  if (s.pending != kRcKeep) return s.pending;  // the previous call ran out of pool, or filled a directory
  if (std::memcmp(s.sig, sig, sizeof(s.sig)) != 0) return kRcSignature;
  // The pool never moves while it holds snapshots. A call's new snapshots are taken to need what the
  // previous call's took, and half of that after the store's first call, which built every key; a
  // pool sized for calls less than half this one's size is given up as well. (A call that runs out
  // all the same leaves keys uncached and asks the next one to start empty: rc_store_finish.)
  const uint64_t cap = std::min(s.cap, cap_limit);
  const uint64_t need = std::min(want_cap, s.calls <= 1 ? s.last_call / 2 : s.last_call);
  if (want_cap > 2 * s.cap || cap < s.used || cap - s.used < need) return kRcPool;
  for (const RcStoreDir& d : s.dir)
    if (d.n_slots && 2 * d.count > d.n_slots) return kRcDirectory;
  return kRcKeep;
}

int rc_store_prepare(RcStore& s, int decision, const uint32_t sig[kRcSigWords], uint64_t want_cap, hipStream_t st,
                     std::string& err) {
  if (!s.last) HIP_TRY(hipEventCreateWithFlags(&s.last, hipEventDisableTiming));
  if (!s.dev) HIP_TRY(hipMalloc((void**)&s.dev, RcStore::kDevWords * sizeof(unsigned long long)));
  if (decision == kRcKeep) {  // this call's carried counts start at zero
    HIP_TRY(hipMemsetAsync(s.dev + 1, 0, 9 * sizeof(unsigned long long), st));
    ++s.calls;
    s.filled = false;
    return FAC_OK;
  }
  s.valid = false;
  s.filled = true;
  if (!s.pool || s.cap < want_cap) {
    if (s.pool) HIP_TRY(hipFree(s.pool));
    s.pool = nullptr;
    s.cap = 0;
    HIP_TRY(hipMalloc((void**)&s.pool, want_cap * sizeof(uint4)));
    s.cap = want_cap;
  }
  HIP_TRY(hipMemsetAsync(s.dev, 0, RcStore::kDevWords * sizeof(unsigned long long), st));
  for (RcStoreDir& d : s.dir) {
    d.count = 0;
    if (d.slots) HIP_TRY(hipMemsetAsync(d.slots, 0, (size_t)d.n_slots * 2 * sizeof(uint4), st));
  }
  std::memcpy(s.sig, sig, sizeof(s.sig));
  s.used = 0;
  s.last_call = 0;
  s.pending = kRcKeep;
  std::memset(s.last_built, 0, sizeof(s.last_built));
  std::memset(s.carried, 0, sizeof(s.carried));
  s.lv_n = 0;
  s.kstart = 0;
  s.floor_pm = -1;
  s.has_dense = false;
  s.calls = 1;
  s.valid = true;
  return FAC_OK;
}

int rc_store_dense(RcStore& s, size_t words, std::string& err) {
  if (!s.dense) HIP_TRY(hipMalloc((void**)&s.dense, words * sizeof(uint32_t)));
  return FAC_OK;
}

int rc_store_dir(RcStore& s, uint32_t k, uint64_t n_ent, hipStream_t st, std::string& err) {
  RcStoreDir& d = s.dir[k];
  // the most keys it has held count too: a directory emptied because it was full comes back larger
  n_ent = std::max(n_ent, d.peak);
  if (d.count || rc_dir_fits(d, n_ent)) return FAC_OK;
  // empty and too small (or none yet): four slots per key, so the keys of later calls fit until the
  // load reaches one half (rc_store_decide then empties the store)
  uint32_t n = 1u << 12;
  while (n < 4 * n_ent && n < (1u << 27)) n <<= 1;
  if (d.slots) HIP_TRY(hipFree(d.slots));
  d.slots = nullptr;
  d.n_slots = 0;
  HIP_TRY(hipMalloc((void**)&d.slots, (size_t)n * 2 * sizeof(uint4)));
  d.n_slots = n;
  HIP_TRY(hipMemsetAsync(d.slots, 0, (size_t)n * 2 * sizeof(uint4), st));
  return FAC_OK;
}

int rc_store_finish(RcStore& s, uint64_t cap_limit, bool carrying, uint64_t gate_min, std::string& err) {
  unsigned long long w[RcStore::kDevWords];
  HIP_TRY(hipMemcpy(w, s.dev, sizeof(w), hipMemcpyDeviceToHost));
  s.last_call = w[0] - std::min<uint64_t>(w[0], s.used);
  s.used = w[0];
  // the bump allocator ran past the pool: the keys that did not fit are stored as uncached
  if (s.used > cap_limit) s.pending = kRcPool;
  for (int k = 0; k < 9; ++k) {
    s.carried[k] = w[1 + k];
    s.last_built[k] = w[10 + k] - std::min<uint64_t>(w[10 + k], s.dir[k].count);
    s.dir[k].count = w[10 + k];
    s.dir[k].peak = std::max(s.dir[k].peak, s.dir[k].count);
  }
  if (carrying) {
    uint64_t c = 0, b = 0;
    for (int k = 0; k < 9; ++k) c += s.carried[k], b += s.last_built[k];
    s.backoff = rc_store_gate(c, b, s.backoff, gate_min);
    s.sleep = s.backoff;
    if (s.sleep) s.valid = false;  // what it holds did not pay: empty when the store is used again
  }
  return FAC_OK;
}

void rc_store_drop(RcStore& s) {
  if (s.pool) (void)hipFree(s.pool);
  if (s.dev) (void)hipFree(s.dev);
  for (RcStoreDir& d : s.dir) {
    if (d.slots) (void)hipFree(d.slots);
    const uint64_t peak = d.peak;
    d = RcStoreDir{};
    d.peak = peak;
  }
  if (s.last) (void)hipEventDestroy(s.last);
  if (s.dense) (void)hipFree(s.dense);
  s.pool = nullptr;
  s.dev = nullptr;
  s.last = nullptr;
  s.dense = nullptr;
  s.cap = s.used = s.last_call = 0;
  s.valid = false;
  s.pending = kRcKeep;
  std::memset(s.sig, 0, sizeof(s.sig));
  s.lv_n = 0;
  s.kstart = 0;
  s.floor_pm = -1;
  s.has_dense = false;
  s.filled = false;
}

void free_engine_device(Engine& e) {
  if (e.d_nodes == nullptr && e.stream == nullptr) return;
  (void)hipSetDevice(e.device);
  {
    std::lock_guard<std::mutex> lk(e.rc_store.mu);
    rc_store_drop(e.rc_store);
  }
  void* ptrs[] = {e.d_nodes, e.d_out_range, e.d_pidx, e.d_edges, e.d_out_pat, e.d_sb_edge, e.d_gt, e.d_aux, e.d_pat_bytes, e.d_pats, e.d_sim_ascii, e.d_sim_keys,
                  e.d_sim_vals, e.d_ascii_id, e.d_edge_gid, e.d_ascii_gid, e.d_map_range,
                  e.d_map_ent, e.d_map_hay};
  for (void* p : ptrs)
    if (p) (void)hipFree(p);
  grapheme_table_free(e.sym_tab);
  grapheme_table_free(e.gid_tab);
  e.pf_cache.clear();
  for (int i = 0; i < Engine::kScratch; ++i)
    if (e.scratch_p[i]) {
      (void)hipFree(e.scratch_p[i]);
      e.scratch_p[i] = nullptr;
      e.scratch_n[i] = 0;
    }
  if (e.stream) {
    call_scratch_release_stream(e.stream);
    (void)hipStreamDestroy(e.stream);
  }
  e.stream = nullptr;
  if (e.aux_stream) {
    call_scratch_release_stream(e.aux_stream);
    (void)hipStreamDestroy(e.aux_stream);
  }
  e.aux_stream = nullptr;
  e.d_nodes = nullptr;
}

int stage_haystack(const Engine& e, const uint8_t* utf8, uint64_t len, Haystack& h, std::string& err,
                   int force_ascii, hipStream_t stream) {
  h.device = e.device;
  h.len = len;
  // force_ascii -2: the bytes are validated and classified on the device after the upload
  const bool check_on_device = force_ascii == -2;
  h.ascii = check_on_device ? false : force_ascii < 0 ? ascii_only(utf8, len) : force_ascii != 0;
  h.n = h.ascii ? len : 0;
  HIP_TRY(hipSetDevice(e.device));
  // All uploads go through one stream (the engine's, or the caller's) and are synchronized before
  // returning, so kernels on any stream see complete data (pageable copies may otherwise still be
  // in flight).
  hipStream_t st = stream ? stream : e.stream;
  HIP_TRY(hipMalloc((void**)&h.d_utf8, std::max<uint64_t>(len, 16)));
  h.own_utf8 = true;
  if (len) HIP_TRY(hipMemcpyAsync(h.d_utf8, utf8, len, hipMemcpyHostToDevice, st));
  // UTF-8 check / is_ascii, UAX #29 segmentation + folding on the device (stage_kernels.hip)
  if (int rc = stage_device(e, h, st, err, check_on_device ? -2 : h.ascii ? 1 : 0)) return rc;
  if (h.n > grapheme_limit()) return FAC_E_HAYSTACK_TOO_LARGE;
  HIP_TRY(hipStreamSynchronize(st));
  return FAC_OK;
}

int stage_haystack_device(const Engine& e, const uint8_t* d_utf8, uint64_t len, Haystack& h, std::string& err,
                          hipStream_t stream, int mode) {
  HIP_TRY(hipSetDevice(e.device));
  if (h.d_utf8 && h.own_utf8) HIP_TRY(hipFree(h.d_utf8));
  h.device = e.device;
  h.len = len;
  h.d_utf8 = const_cast<uint8_t*>(d_utf8);
  h.own_utf8 = false;
  h.base = 0;
  h.open_end = false;
  h.owned = UINT64_MAX;
  {
    std::lock_guard<std::mutex> lk(h.host_mu);
    h.host_ready = false;
    h.utf8.clear();
    h.starts.clear();
  }
  {  // the grapheme ids follow the text: the contents are stale, the array stays (ensure_gids)
    std::lock_guard<std::mutex> lk(h.gid_mu);
    h.gid_engine = nullptr;
  }
  hipStream_t st = stream ? stream : e.stream;
  int rc = stage_device(e, h, st, err, mode);
  if (!rc) {
    const hipError_t se = hipStreamSynchronize(st);
    if (se != hipSuccess) {
      err = std::string("hipStreamSynchronize: ") + hipGetErrorString(se);
      rc = FAC_E_HIP;
    }
  }
  if (rc) {  // a failed restage leaves a valid empty haystack (no stale grapheme offsets over new bytes)
    h.failed_n = h.n;  // HaystackTooLarge reports the count
    h.ascii = true;
    h.len = 0;
    h.n = 0;
    h.d_utf8 = nullptr;
  }
  return rc;
}

int ensure_host(const Haystack& h, std::string& err) {
  std::lock_guard<std::mutex> lk(h.host_mu);
  if (h.host_ready) return FAC_OK;
  HIP_TRY(hipSetDevice(h.device));
  h.utf8.resize(h.len);
  if (h.len) HIP_TRY(hipMemcpy(h.utf8.data(), h.d_utf8, h.len, hipMemcpyDeviceToHost));
  if (!h.ascii) {
    h.starts.resize(h.n);
    if (h.n) HIP_TRY(hipMemcpy(h.starts.data(), h.d_off, h.n * 8, hipMemcpyDeviceToHost));
  }
  h.host_ready = true;
  return FAC_OK;
}

void free_haystack(Haystack& h) {
  (void)hipSetDevice(h.device);
  if (h.d_utf8 && h.own_utf8) (void)hipFree(h.d_utf8);
  if (h.d_text32) (void)hipFree(h.d_text32);
  if (h.d_off) (void)hipFree(h.d_off);
  if (h.d_gid) (void)hipFree(h.d_gid);
  if (h.d_stage) (void)hipFree(h.d_stage);
  h.d_utf8 = nullptr;
  h.d_text32 = nullptr;
  h.d_off = nullptr;
  h.d_gid = nullptr;
  h.d_stage = nullptr;
  h.gid_cap = 0;
  h.gid_engine = nullptr;
  h.off_cap = 0;
  h.stage_cap = 0;
}

// Grapheme ids of a Unicode haystack, or of a batch's non-ASCII documents, for an engine with
// mappings (gs_text compared as whole folded graphemes, grapheme.rs:61-63): looked up on the device
// by the first search after a staging (grapheme_ids_device) and kept for that engine. The build is
// ordered on the call's stream and synchronised once, so a search on any other stream that finds the
// cache valid reads complete ids.
int ensure_gids(const Engine& e, const Haystack& h, hipStream_t st, std::string& err) {
  if (h.ascii) return FAC_OK;
  std::lock_guard<std::mutex> lk(h.gid_mu);
  if (h.d_gid && h.gid_engine == &e) return FAC_OK;
  HIP_TRY(hipSetDevice(h.device));
  h.gid_engine = nullptr;
  if (!h.d_gid || h.gid_cap < h.n) {
    if (h.d_gid) HIP_TRY(hipFree(h.d_gid));
    h.d_gid = nullptr;
    h.gid_cap = 0;
    HIP_TRY(hipMalloc((void**)&h.d_gid, std::max<uint64_t>(h.n * sizeof(uint32_t), 16)));
    h.gid_cap = h.n;
  }
  if (!st) st = e.stream;
  if (int rc = grapheme_ids_device(e, h, h.d_gid, st, err)) return rc;
  HIP_TRY(hipStreamSynchronize(st));
  h.gid_engine = &e;
  return FAC_OK;
}

}  // namespace fac
