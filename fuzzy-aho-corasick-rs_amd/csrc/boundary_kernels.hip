// boundary_kernels.hip — whole-token matches of a batch (fac.h fac_batch_require_boundaries,
// DESIGN.md 6a "Whole-token matches"): one pass over the raw records a batch search left in HBM,
// between the search and the per-document apply (rank_kernels.hip apply_batch_device). A record is
// kept when every requested side of it is a boundary of its own document:
//   end side:   end == document length, or the code point that begins at byte `end` is not alphanumeric;
//   start side: walking left from `start`, transparent code points (General_Category M* and not
//               alphanumeric) are skipped and the first other code point decides: a boundary when it
//               is not alphanumeric. Byte 0 of the document is a boundary, and so is having skipped
//               kBoundaryMaxSkip transparent code points without a decision.
// unicode.cpp boundary_ok is the same rule on the host. Kept records are compacted into the other
// half of the call's record buffer (wave ballot, lane prefix, one atomic per wave); the order of the
// compacted records is not the order of the raw ones, which no caller relies on (every order the
// apply produces is a total order; Unsorted + Keep is unspecified within a document).
//
// The same pass for the raw records of a stream task (fac.h fac_stream_open_opts; stream.cpp
// run_window_task), where the document is the stream and not the window: the start side's walk goes
// on to the left of the window's first byte, into the task's text and then into the up to
// kBoundaryCarry bytes the task carries over from its predecessor, and only byte 0 of the stream is
// a boundary by position; the end side is decided inside the window's text. It reads the task's
// original text, never the gathered per-window copies, which have no left context.
#include <hip/hip_runtime.h>

#include <mutex>

#include "fac_internal.h"
#include "host_util.h"
#include "wave_util.h"

namespace fac {
namespace {

struct GcbRange { uint32_t lo, hi; uint8_t prop; };

#define FAC_UNICODE_QUAL __device__
#include "unicode_boundary.inc"
#undef FAC_UNICODE_QUAL

constexpr uint32_t kCodePoints = 0x110000u;
constexpr uint32_t kClassBytes = kCodePoints / 4;  // two bits per code point
constexpr uint64_t kDocLow = (1ull << kDocTagShift) - 1;
constexpr uint32_t kThreads = 256;
constexpr uint32_t kMaxBlocks = 2048;  // the rest of a large record set is grid-strided

__device__ uint32_t class_search(uint32_t cp) {  // unicode.cpp boundary_class
  uint32_t lo = 0, hi = sizeof(kBoundaryRanges) / sizeof(kBoundaryRanges[0]);
  const uint32_t n = hi;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (kBoundaryRanges[mid].hi < cp) lo = mid + 1;
    else hi = mid;
  }
  return (lo < n && kBoundaryRanges[lo].lo <= cp) ? kBoundaryRanges[lo].prop : 0u;
}

// The class table of a device, built once from the ranges above: byte b holds code points
// 4b .. 4b + 3, two bits each (bit 0 alphanumeric, bit 1 transparent).
__global__ void boundary_table_kernel(uint8_t* tab) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= kClassBytes) return;
  uint32_t v = 0;
  for (uint32_t k = 0; k < 4; ++k) v |= class_search(4 * b + k) << (2 * k);
  tab[b] = (uint8_t)v;
}

// ASCII neighbours (the common case) are classified in registers and never touch the table
__device__ __forceinline__ uint32_t class_of(const uint8_t* __restrict__ tab, uint32_t cp) {
  if (cp < 0x80u) return ((cp | 0x20u) - 'a' < 26u || cp - '0' < 10u) ? 1u : 0u;
  if (cp >= kCodePoints) return 0u;
  return (tab[cp >> 2] >> ((cp & 3u) * 2)) & 3u;
}

// The code point that begins at byte i of s, reading no byte at or past `lim` (i < lim). The
// documents are valid UTF-8, so the checks against lim only ever bound a malformed input.
__device__ __forceinline__ uint32_t decode_at(const uint8_t* __restrict__ s, uint64_t i, uint64_t lim) {
  const uint32_t b0 = s[i];
  if (b0 < 0x80u) return b0;
  if ((b0 & 0xE0u) == 0xC0u && i + 1 < lim) return ((b0 & 0x1Fu) << 6) | (s[i + 1] & 0x3Fu);
  if ((b0 & 0xF0u) == 0xE0u && i + 2 < lim) return ((b0 & 0x0Fu) << 12) | ((s[i + 1] & 0x3Fu) << 6) | (s[i + 2] & 0x3Fu);
  if ((b0 & 0xF8u) == 0xF0u && i + 3 < lim)
    return ((b0 & 0x07u) << 18) | ((s[i + 1] & 0x3Fu) << 12) | ((s[i + 2] & 0x3Fu) << 6) | (s[i + 3] & 0x3Fu);
  return 0xFFFDu;
}

__device__ __forceinline__ bool end_is_boundary(const uint8_t* __restrict__ s, const uint8_t* __restrict__ tab, uint64_t end,
                                                uint64_t hi) {
  if (end >= hi) return true;
  return (class_of(tab, decode_at(s, end, hi)) & 1u) == 0;
}

__device__ __forceinline__ bool start_is_boundary(const uint8_t* __restrict__ s, const uint8_t* __restrict__ tab,
                                                  uint64_t start, uint64_t lo) {
  uint64_t p = start;
  for (uint32_t skipped = 0; skipped < kBoundaryMaxSkip; ++skipped) {
    if (p <= lo) return true;
    uint64_t q = p - 1;  // the first byte of the code point that ends at p
    while (q > lo && p - q < 4 && (s[q] & 0xC0u) == 0x80u) --q;
    const uint32_t c = class_of(tab, decode_at(s, q, p));
    if (!(c & 2u)) return (c & 1u) == 0;
    p = q;
  }
  return true;
}

// One thread per raw record (start / end tagged with the document, fac_internal.h Batch). The 32 B
// record travels as two 16 B halves; `count` receives the kept total.
__global__ __launch_bounds__(kThreads) void boundary_filter_kernel(const uint4* __restrict__ in, uint64_t n,
                                                                   const uint8_t* __restrict__ utf8,
                                                                   const uint64_t* __restrict__ offsets, uint64_t n_docs,
                                                                   const uint8_t* __restrict__ tab, uint32_t sides,
                                                                   uint4* __restrict__ out, unsigned long long* count) {
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
      keep = true;
      if (d < n_docs) {
        const uint64_t lo = offsets[d], hi = offsets[d + 1];
        const uint64_t st = ts & kDocLow, en = te & kDocLow;
        if (lo <= st && st <= en && en <= hi) {  // (always, for the records of a search: only such a span is read around)
          if (sides & FAC_BOUNDARY_END) keep = end_is_boundary(utf8, tab, en, hi);
          if (keep && (sides & FAC_BOUNDARY_START)) keep = start_is_boundary(utf8, tab, st, lo);
        }
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

// The start side of a stream window's record at byte `start` of the task's text s: the walk of
// start_is_boundary, going on to the left of s[0] into the cn bytes at ctx (the stream's text just
// before the task). Positions are relative to s[0]; the context holds [-cn, 0). Its front is the
// start of the stream, or kBoundaryCarry bytes away, which the walk's kBoundaryMaxSkip code points
// cannot cross undecided.
__device__ __forceinline__ bool stream_start_is_boundary(const uint8_t* __restrict__ s, const uint8_t* __restrict__ ctx,
                                                         int64_t cn, const uint8_t* __restrict__ tab, uint64_t start) {
  const int64_t front = -cn;
  int64_t p = (int64_t)start;
  for (uint32_t skipped = 0; skipped < kBoundaryMaxSkip; ++skipped) {
    if (p <= front) return true;
    // the code point that ends at p: its bytes, last first (a commit point is a character boundary,
    // so no code point has bytes on both sides of s[0]; reading byte by byte needs no such promise)
    uint32_t b[4];
    uint32_t k = 0;
    int64_t q = p;
    do {
      --q;
      b[k++] = q >= 0 ? s[q] : ctx[cn + q];
    } while (q > front && k < 4 && (b[k - 1] & 0xC0u) == 0x80u);
    const uint32_t b0 = b[k - 1];
    uint32_t cp = 0xFFFDu;
    if (b0 < 0x80u) cp = b0;
    else if ((b0 & 0xE0u) == 0xC0u && k == 2) cp = ((b0 & 0x1Fu) << 6) | (b[0] & 0x3Fu);
    else if ((b0 & 0xF0u) == 0xE0u && k == 3) cp = ((b0 & 0x0Fu) << 12) | ((b[1] & 0x3Fu) << 6) | (b[0] & 0x3Fu);
    else if ((b0 & 0xF8u) == 0xF0u && k == 4)
      cp = ((b0 & 0x07u) << 18) | ((b[2] & 0x3Fu) << 12) | ((b[1] & 0x3Fu) << 6) | (b[0] & 0x3Fu);
    const uint32_t c = class_of(tab, cp);
    if (!(c & 2u)) return (c & 1u) == 0;
    p = q;
  }
  return true;
}

// One thread per raw record of a stream task (fac_internal.h StreamFilter): start / end tagged with
// the window; the same compaction as boundary_filter_kernel.
__global__ __launch_bounds__(kThreads) void stream_boundary_filter_kernel(
    const uint4* __restrict__ in, uint64_t n, const uint8_t* __restrict__ text, uint64_t text_len,
    const uint64_t* __restrict__ src, const uint64_t* __restrict__ len, const uint64_t* __restrict__ doc_off,
    uint64_t n_windows, const uint8_t* __restrict__ ctx, uint32_t ctx_len, const uint8_t* __restrict__ tab, uint32_t sides,
    uint4* __restrict__ out, unsigned long long* count) {
  const uint32_t lane = lane_id();
  for (uint64_t base = (uint64_t)blockIdx.x * kThreads; base < n; base += (uint64_t)gridDim.x * kThreads) {
    const uint64_t i = base + threadIdx.x;
    bool keep = false;
    uint4 a = make_uint4(0, 0, 0, 0), b = a;
    if (i < n) {
      a = in[2 * i];
      b = in[2 * i + 1];
      const uint64_t ts = ((uint64_t)a.y << 32) | a.x, te = ((uint64_t)a.w << 32) | a.z;
      const uint64_t w = ts >> kDocTagShift;
      keep = true;
      if (w < n_windows) {
        const uint64_t lo = src[w], hi = lo + len[w];
        // the record's span in the task's text
        const uint64_t shift = doc_off ? lo - doc_off[w] : 0;
        const uint64_t st = (ts & kDocLow) + shift, en = (te & kDocLow) + shift;
        if (lo <= st && st <= en && en <= hi && hi <= text_len) {  // (always: only such a span is read around)
          if (sides & FAC_BOUNDARY_END) keep = end_is_boundary(text, tab, en, hi);
          if (keep && (sides & FAC_BOUNDARY_START)) keep = stream_start_is_boundary(text, ctx, (int64_t)ctx_len, tab, st);
        }
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

// the class table of `device`, built on first use (kept for the process)
int boundary_table(int device, hipStream_t st, const uint8_t*& out, std::string& err) {
  static std::mutex mu;
  static uint8_t* tabs[64];
  if (device < 0 || device >= 64) {
    err = "device ordinal out of range";
    return FAC_E_INVALID;
  }
  std::lock_guard<std::mutex> lk(mu);
  if (!tabs[device]) {
    uint8_t* t = nullptr;
    HIP_TRY(hipMalloc((void**)&t, kClassBytes));
    hipLaunchKernelGGL(boundary_table_kernel, dim3((kClassBytes + 255) / 256), dim3(256), 0, st, t);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
      (void)hipFree(t);
      err = "building the boundary class table failed";
      return FAC_E_HIP;
    }
    tabs[device] = t;
  }
  out = tabs[device];
  return FAC_OK;
}

}  // namespace

int boundary_filter_device(const Batch& b, int sides, const fac_match* d_in, uint64_t n, fac_match* d_out,
                           unsigned long long* d_count, hipStream_t s, uint64_t* n_kept, std::string& err) {
  *n_kept = 0;
  if (n == 0) return FAC_OK;
  const uint8_t* tab = nullptr;
  if (int rc = boundary_table(b.h.device, s, tab, err)) return rc;
  HIP_TRY(hipMemsetAsync(d_count, 0, sizeof(unsigned long long), s));
  const uint32_t grid = (uint32_t)std::min<uint64_t>((n + kThreads - 1) / kThreads, kMaxBlocks);
  hipLaunchKernelGGL(boundary_filter_kernel, dim3(grid), dim3(kThreads), 0, s, reinterpret_cast<const uint4*>(d_in), n,
                     b.h.d_utf8, b.d_offsets, b.n_docs, tab, (uint32_t)sides, reinterpret_cast<uint4*>(d_out), d_count);
  HIP_TRY(hipGetLastError());
  unsigned long long kept = 0;
  HIP_TRY(hipMemcpyAsync(&kept, d_count, sizeof(kept), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  *n_kept = kept;
  return FAC_OK;
}

int stream_boundary_filter_device(int device, const StreamFilter& f, const fac_match* d_in, uint64_t n, fac_match* d_out,
                                  unsigned long long* d_count, hipStream_t s, uint64_t* n_kept, std::string& err) {
  *n_kept = 0;
  if (n == 0) return FAC_OK;
  if (f.before_len > kBoundaryCarry || (f.before_len && !f.d_before)) {
    err = "a stream task's boundary context is malformed";
    return FAC_E_INTERNAL;
  }
  const uint8_t* tab = nullptr;
  if (int rc = boundary_table(device, s, tab, err)) return rc;
  HIP_TRY(hipMemsetAsync(d_count, 0, sizeof(unsigned long long), s));
  const uint32_t grid = (uint32_t)std::min<uint64_t>((n + kThreads - 1) / kThreads, kMaxBlocks);
  hipLaunchKernelGGL(stream_boundary_filter_kernel, dim3(grid), dim3(kThreads), 0, s, reinterpret_cast<const uint4*>(d_in), n,
                     f.d_text, f.text_len, f.d_src, f.d_len, f.d_doc_off, f.n_windows, f.d_before, f.before_len, tab,
                     (uint32_t)f.sides, reinterpret_cast<uint4*>(d_out), d_count);
  HIP_TRY(hipGetLastError());
  unsigned long long kept = 0;
  HIP_TRY(hipMemcpyAsync(&kept, d_count, sizeof(kept), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  *n_kept = kept;
  return FAC_OK;
}

}  // namespace fac
