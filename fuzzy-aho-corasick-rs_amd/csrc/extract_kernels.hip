// extract_kernels.hip — the strings of a batch's kept records on the MI355X:
// FuzzyMatches::matched_strings (src/matches.rs:513-515) for every document of a staged batch, or,
// with a replacement table, the piece fac_replace_batch would write for each record. The per-document
// apply (rank_kernels.hip apply_batch_device) left the kept records grouped by document; item i is
// the string of record i, so the records' CSR index is the items' as well.
//
// * extract_len_kernel: one thread per item (and one for the sentinel entry) finds the item's
//   document by bisection of the CSR index and writes the item's length and the global byte its
//   matched text starts at, so the mover needs no document lookup.
// * one rocPRIM exclusive scan turns the lengths into the n_items + 1 item offsets.
// * extract_copy_kernel: output-stationary byte mover, replace_copy_kernel's shape. A workgroup owns
//   kExtractTile consecutive output bytes, a lane 16 of them. The tile's first and last items are
//   found once per tile; a lane bisects only between them and then advances an (item, pre | text |
//   suf) cursor over the runs of fac_internal.h piece_run until its 16 bytes are full: empty items
//   and empty runs are runs of length 0 the cursor steps over. No atomics, no LDS beyond the two
//   tile bounds, one 16-byte store per lane.
#include <hip/hip_runtime.h>

#include <algorithm>

#include <rocprim/device/device_scan.hpp>

#include "fac_internal.h"
#include "host_util.h"

namespace fac {
namespace {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kChunk = 16;  // output bytes per lane
constexpr uint32_t kExtractTile = kThreads * kChunk;  // output bytes one workgroup owns

// A NULL table is "keep" for every pattern.
__device__ inline void entry_of(const uint2* __restrict__ tab, const uint32_t* __restrict__ ins, uint32_t p, uint2& t,
                                uint32_t& k) {
  t = tab ? tab[p] : make_uint2(0, kReplaceKeep);
  k = ins ? ins[p] : kReplaceNoInsert;
}

// len has n_items + 1 entries, the last one 0, so the exclusive scan's last output is the total.
__global__ void extract_len_kernel(const fac_match* __restrict__ m, uint64_t n_items,
                                   const uint64_t* __restrict__ doc_off, const uint64_t* __restrict__ offsets,
                                   uint64_t n_docs, const uint2* __restrict__ tab, const uint32_t* __restrict__ ins,
                                   uint64_t* __restrict__ len, uint64_t* __restrict__ src) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i > n_items) return;
  if (i == n_items) {
    len[i] = 0;
    return;
  }
  // the document d with doc_off[d] <= i < doc_off[d + 1]: the first entry above i, less one (empty
  // documents repeat values; doc_off[n_docs] = n_items > i bounds the search)
  uint64_t lo = 0, hi = n_docs;
  while (lo < hi) {
    const uint64_t mid = (lo + hi) >> 1;
    if (doc_off[mid] <= i) lo = mid + 1;
    else hi = mid;
  }
  const uint64_t ms = m[i].start, me = m[i].end;
  uint2 t;
  uint32_t k;
  entry_of(tab, ins, m[i].pattern_index, t, k);
  len[i] = piece_len(t, k, me - ms);
  src[i] = offsets[lo - 1] + ms;
}

// last item i in [lo, hi] with item_off[i] <= x (item_off[lo] <= x holds)
__device__ inline uint64_t item_of(const uint64_t* __restrict__ item_off, uint64_t lo, uint64_t hi, uint64_t x) {
  while (lo < hi) {
    const uint64_t mid = (lo + hi + 1) >> 1;
    if (item_off[mid] <= x) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(kThreads) void extract_copy_kernel(
    const uint8_t* __restrict__ utf8, const fac_match* __restrict__ m, uint64_t n_items,
    const uint64_t* __restrict__ item_off, const uint64_t* __restrict__ item_src, const uint2* __restrict__ tab,
    const uint32_t* __restrict__ ins, const uint8_t* __restrict__ rep, uint8_t* __restrict__ out, uint64_t total,
    int wide) {
  __shared__ uint64_t s_item[2];
  const uint64_t tile0 = (uint64_t)blockIdx.x * kExtractTile;
  if (tile0 >= total) return;
  if (threadIdx.x == 0) {
    const uint64_t tile_last = (total - tile0 < kExtractTile ? total : tile0 + kExtractTile) - 1;
    const uint64_t i0 = item_of(item_off, 0, n_items - 1, tile0);
    s_item[0] = i0;
    s_item[1] = item_of(item_off, i0, n_items - 1, tile_last);
  }
  __syncthreads();
  const uint64_t g = tile0 + (uint64_t)threadIdx.x * kChunk;
  if (g >= total) return;
  const uint32_t n = total - g < kChunk ? (uint32_t)(total - g) : kChunk;

  // the lane's first byte: the last item that starts at or before it, from that item's first run;
  // the bytes before g are skipped run by run
  uint64_t i = item_of(item_off, s_item[0], s_item[1], g);
  uint64_t skip = g - item_off[i];
  int run = 0;  // 0 pre, 1 text, 2 suf

  Chunk16 c;  // the lane's 16 bytes
  for (;;) {
    const uint8_t* src;
    uint64_t rl;
    uint2 t;
    uint32_t k;
    entry_of(tab, ins, m[i].pattern_index, t, k);
    piece_run(t, k, rep, utf8 + item_src[i], m[i].end - m[i].start, run, src, rl);
    if (skip) {
      const uint64_t s = skip < rl ? skip : rl;
      src += s;
      rl -= s;
      skip -= s;
    }
    if (rl) {
      const uint32_t take = rl < (uint64_t)(n - c.filled) ? (uint32_t)rl : n - c.filled;
      if (take == kChunk) chunk_load16(c, src);
      else chunk_put(c, src, take);
      if (c.filled == n) break;
    }
    // next run
    if (run < 2) {
      ++run;
    } else {
      if (++i >= n_items) break;
      run = 0;
    }
  }

  chunk_store(c, out + g, wide);
}

}  // namespace

int extract_plan_device(const Batch& b, const ReplaceTable* t, const fac_match* d_recs, uint64_t n_recs,
                        const uint64_t* d_doc_off, hipStream_t s, ExtractPlan& plan, std::string& err) {
  const uint64_t ni = n_recs;
  size_t scan_bytes = 0;
  HIP_TRY(rocprim::exclusive_scan(nullptr, scan_bytes, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint64_t)0, ni + 1,
                                 rocprim::plus<uint64_t>(), s));
  // one block of call scratch: lengths, offsets, source words, the scan's own
  const size_t o_len = 0, o_off = o_len + up256((ni + 1) * 8), o_src = o_off + up256((ni + 1) * 8);
  const size_t o_tmp = o_src + up256((ni + 1) * 8), bytes = o_tmp + up256(std::max<size_t>(scan_bytes, 16));
  hipError_t he = hipSuccess;
  plan.s = s;
  plan.n_items = ni;
  plan.mem = call_scratch_take(bytes, s, &he);
  if (he != hipSuccess || !plan.mem) {
    plan.mem = nullptr;
    err = std::string("hipMalloc: ") + hipGetErrorString(he);
    return FAC_E_OOM;
  }
  char* base = static_cast<char*>(plan.mem);
  uint64_t* d_len = reinterpret_cast<uint64_t*>(base + o_len);
  plan.d_item_off = reinterpret_cast<uint64_t*>(base + o_off);
  plan.d_src = reinterpret_cast<uint64_t*>(base + o_src);
  hipLaunchKernelGGL(extract_len_kernel, dim3((uint32_t)((ni + 1 + kThreads - 1) / kThreads)), dim3(kThreads), 0, s,
                     d_recs, ni, d_doc_off, b.d_offsets, b.n_docs, t ? t->d_tab : nullptr, t ? t->d_ins : nullptr, d_len,
                     plan.d_src);
  HIP_TRY(hipGetLastError());
  HIP_TRY(rocprim::exclusive_scan(base + o_tmp, scan_bytes, d_len, plan.d_item_off, (uint64_t)0, ni + 1,
                                 rocprim::plus<uint64_t>(), s));
  unsigned long long total = 0;
  HIP_TRY(hipMemcpyAsync(&total, plan.d_item_off + ni, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  plan.total = total;
  return FAC_OK;
}

int extract_copy_device(const Batch& b, const ReplaceTable* t, const fac_match* d_recs, const ExtractPlan& plan,
                        uint8_t* d_out, std::string& err) {
  if (!plan.total) return FAC_OK;  // (then every item is empty, and n_items may be 0)
  const uint64_t tiles = (plan.total + kExtractTile - 1) / kExtractTile;  // < 2^28: total < 2^40
  const int wide = (reinterpret_cast<uintptr_t>(d_out) & 15u) == 0 ? 1 : 0;
  hipLaunchKernelGGL(extract_copy_kernel, dim3((uint32_t)tiles), dim3(kThreads), 0, plan.s, b.h.d_utf8, d_recs,
                     plan.n_items, plan.d_item_off, plan.d_src, t ? t->d_tab : nullptr, t ? t->d_ins : nullptr,
                     t ? t->d_bytes : nullptr, d_out, plan.total, wide);
  HIP_TRY(hipGetLastError());
  return FAC_OK;
}

}  // namespace fac
