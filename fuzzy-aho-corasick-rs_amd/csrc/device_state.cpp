// device_state.cpp — host-only device state: the engine's tables and streams, a haystack's device
// buffers and host copies, the per-worker scratch sets. Allocations and copies only, no kernel.
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

void free_engine_device(Engine& e) {
  if (e.d_nodes == nullptr && e.stream == nullptr) return;
  (void)hipSetDevice(e.device);
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
