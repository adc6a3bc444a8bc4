// anchor_kernels.hip — anchored matches of a batch (fac.h fac_batch_require_anchors, fac_lookup_batch;
// DESIGN.md 6a "Anchored matches"): "which dictionary entry IS this string" instead of "where in
// this string does an entry occur". A raw record (start, end) of a document doc[0, n) is kept when
//   start == 0, if FAC_ANCHOR_START is requested, and
//   end == n,   if FAC_ANCHOR_END is requested.
// Three kernels:
//  - anchor_desc_kernel: the batch's segment descriptors with the window range narrowed to the start
//    windows that can produce a kept record (window 0 for START / WHOLE, the last T for END alone),
//    searched through launch_search_batch_windows. Everything but w_begin / w_end stays the
//    document's, so the narrowed search is the unrestricted one minus whole windows.
//  - anchor_filter_kernel: the rule itself over the raw records, shaped like boundary_filter_kernel
//    (one thread per record, two 16 B halves, wave-ballot compaction into the buffer's other half).
//    It reads the record and the document's two offsets, never the text.
//  - lookup_table_kernel: the dense n_docs x k table of fac_lookup_batch from the applied records
//    and their CSR index.
#include <hip/hip_runtime.h>

#include "fac_internal.h"
#include "host_util.h"
#include "wave_util.h"

namespace fac {
namespace {

constexpr uint64_t kDocLow = (1ull << kDocTagShift) - 1;
constexpr uint32_t kThreads = 256;
constexpr uint32_t kMaxBlocks = 2048;  // the rest of a large set is grid-strided

// One thread per non-empty document (Batch::d_segs holds only those, n >= 1 each): its descriptor
// with the narrowed range, and the range's length for the prefix; thread 0 also writes the closing 0.
// tail: T = max_match_graphemes + 2 (END alone: windows [n - min(n, T), n)).
__global__ __launch_bounds__(kThreads) void anchor_desc_kernel(const SegDesc* __restrict__ in, uint64_t n_segs, uint32_t sides,
                                                               uint64_t tail, SegDesc* __restrict__ out,
                                                               uint64_t* __restrict__ counts) {
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i == 0) counts[n_segs] = 0;
  if (i >= n_segs) return;
  SegDesc S = in[i];
  const uint64_t n = S.w_end < S.n ? S.w_end : S.n;  // (== S.n for a batch's descriptors)
  if (sides & FAC_ANCHOR_START) {
    S.w_begin = 0;
    S.w_end = n ? 1 : 0;
  } else {
    S.w_begin = n - (n < tail ? n : tail);
    S.w_end = n;
  }
  out[i] = S;
  counts[i] = S.w_end - S.w_begin;
}

// One thread per raw record (start / end tagged with the document, fac_internal.h Batch); `count`
// receives the kept total.
__global__ __launch_bounds__(kThreads) void anchor_filter_kernel(const uint4* __restrict__ in, uint64_t n,
                                                                 const uint64_t* __restrict__ offsets, uint64_t n_docs,
                                                                 uint32_t sides, uint4* __restrict__ out,
                                                                 unsigned long long* count) {
  const uint32_t lane = lane_id();
  for (uint64_t base = (uint64_t)blockIdx.x * kThreads; base < n; base += (uint64_t)gridDim.x * kThreads) {
    const uint64_t i = base + threadIdx.x;
    bool keep = false;
    uint4 a = make_uint4(0, 0, 0, 0), b = a;
    if (i < n) {
      a = in[2 * i];
      b = in[2 * i + 1];
      const uint64_t ts = ((uint64_t)a.y << 32) | a.x, te = ((uint64_t)a.w << 32) | a.z;
      const uint64_t d = ts >> kDocTagShift;
      if (d < n_docs) {  // (always, for the records of a search)
        keep = true;
        if (sides & FAC_ANCHOR_START) keep = (ts & kDocLow) == offsets[d];
        if (keep && (sides & FAC_ANCHOR_END)) keep = (te & kDocLow) == offsets[d + 1];
      }
    }
    const uint64_t m = __ballot(keep);
    if (m == 0) continue;  // wave-uniform
    unsigned long long at = 0;
    if (lane == 0) at = atomicAdd(count, (unsigned long long)__popcll(m));
    at = shfl_u64(at, 0) + prefix_below(m);
    if (keep) {
      out[2 * at] = a;
      out[2 * at + 1] = b;
    }
  }
}

// One thread per (document, slot) pair of the n_docs x k table: slot s of row d takes record
// doc_off[d] + s of the applied set (document-relative offsets already), or the filler
// {start = end = 0, pattern_index = FAC_UNMATCHED, similarity 0, counts 0}; slot 0 writes found[d].
__global__ __launch_bounds__(kThreads) void lookup_table_kernel(const uint4* __restrict__ recs,
                                                                const uint64_t* __restrict__ doc_off, uint64_t n_docs,
                                                                uint32_t k, uint4* __restrict__ table,
                                                                uint32_t* __restrict__ found) {
  const uint64_t total = n_docs * k;
  for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (uint64_t)gridDim.x * kThreads) {
    const uint64_t d = i / k;
    const uint32_t s = (uint32_t)(i - d * k);
    const uint64_t lo = doc_off[d], m = doc_off[d + 1] - lo;
    uint4 a = make_uint4(0, 0, 0, 0), b = make_uint4(FAC_UNMATCHED, 0, 0, 0);
    if (s < m) {
      a = recs[2 * (lo + s)];
      b = recs[2 * (lo + s) + 1];
    }
    table[2 * i] = a;
    table[2 * i + 1] = b;
    if (s == 0) found[d] = (uint32_t)(m < k ? m : k);
  }
}

}  // namespace

int anchor_windows_device(const Engine& e, const Batch& b, int sides, hipStream_t st, BatchWindows& out, std::string& err) {
  out.s = st;
  out.n = 0;
  out.windows = 0;
  const uint64_t ns = b.n_segs;
  if (ns == 0) return FAC_OK;
  hipError_t he = hipSuccess;
  out.d_segs = static_cast<SegDesc*>(call_scratch_take(ns * sizeof(SegDesc), st, &he));
  HIP_TRY(he);
  out.d_prefix = static_cast<uint64_t*>(call_scratch_take((ns + 1) * 8, st, &he));
  HIP_TRY(he);
  PoolBuf counts;
  HIP_TRY(counts.alloc((ns + 1) * 8, st));
  hipLaunchKernelGGL(anchor_desc_kernel, dim3((uint32_t)((ns + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, b.d_segs, ns,
                     (uint32_t)sides, e.max_match_graphemes + 2, out.d_segs, static_cast<uint64_t*>(counts.p));
  HIP_TRY(hipGetLastError());
  if (int rc = exclusive_sum_u64(static_cast<const uint64_t*>(counts.p), out.d_prefix, ns + 1, st, err)) return rc;
  uint64_t total = 0;
  HIP_TRY(hipMemcpyAsync(&total, out.d_prefix + ns, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (total > b.windows) {  // a narrowed range is a sub-range of the document's
    err = "anchored window ranges exceed the batch's windows";
    return FAC_E_INTERNAL;
  }
  out.n = ns;
  out.windows = total;
  out.out_hint = 2 * ns;  // (the unrestricted search of 64-byte documents starts at one record per document)
  return FAC_OK;
}

int anchor_filter_device(const Batch& b, int sides, const fac_match* d_in, uint64_t n, fac_match* d_out,
                         unsigned long long* d_count, hipStream_t s, uint64_t* n_kept, std::string& err) {
  *n_kept = 0;
  if (n == 0) return FAC_OK;
  HIP_TRY(hipMemsetAsync(d_count, 0, sizeof(unsigned long long), s));
  const uint32_t grid = (uint32_t)std::min<uint64_t>((n + kThreads - 1) / kThreads, kMaxBlocks);
  hipLaunchKernelGGL(anchor_filter_kernel, dim3(grid), dim3(kThreads), 0, s, reinterpret_cast<const uint4*>(d_in), n,
                     b.d_offsets, b.n_docs, (uint32_t)sides, reinterpret_cast<uint4*>(d_out), d_count);
  HIP_TRY(hipGetLastError());
  unsigned long long kept = 0;
  HIP_TRY(hipMemcpyAsync(&kept, d_count, sizeof(kept), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  *n_kept = kept;
  return FAC_OK;
}

int lookup_table_device(const fac_match* d_recs, const uint64_t* d_doc_off, uint64_t n_docs, uint32_t k, fac_match* d_table,
                        uint32_t* d_found, hipStream_t s, std::string& err) {
  if (n_docs == 0) return FAC_OK;
  const uint64_t total = n_docs * k;
  const uint32_t grid = (uint32_t)std::min<uint64_t>((total + kThreads - 1) / kThreads, kMaxBlocks);
  hipLaunchKernelGGL(lookup_table_kernel, dim3(grid), dim3(kThreads), 0, s, reinterpret_cast<const uint4*>(d_recs), d_doc_off,
                     n_docs, k, reinterpret_cast<uint4*>(d_table), d_found);
  HIP_TRY(hipGetLastError());
  return FAC_OK;
}

}  // namespace fac
