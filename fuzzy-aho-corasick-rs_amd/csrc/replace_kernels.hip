// replace_kernels.hip — the splice of a batch on the MI355X: FuzzyMatches::replace
// (src/matches.rs:165-188) for every document of a staged batch, after the per-document apply
// (rank_kernels.hip apply_batch_device) left the kept records in (document, start, acceptance) order.
//
// A document's output is gap 0, piece 0, gap 1, piece 1, ..., tail: gap k = the document's bytes
// from `last` to record k's start, piece k = record k's replacement (or its matched text for a
// "keep" pattern), tail = the bytes after the last applied record. A record that starts before
// `last` is skipped by the reference's guard (matches.rs:173); here it is a zero-length gap and a
// zero-length piece, so the walk below never branches on it twice.
//
// * replace_plan_kernel: one thread per document walks its records once and writes, per record, the
//   output offset of its piece and the source offset of its gap, and per document the output length.
// * one rocPRIM exclusive scan turns the lengths into the n_docs + 1 output offsets.
// * replace_copy_kernel: output-stationary byte mover. A workgroup owns kReplaceTile consecutive
//   output bytes, a lane 16 of them. The tile's first and last documents are found once per tile;
//   a lane bisects only between them, finds its piece, and then advances a (document, record,
//   gap | piece) cursor over runs of source bytes until its 16 bytes are full: documents of 0-3
//   bytes, empty gaps and empty replacements are runs of length 0 the cursor steps over. No atomics,
//   no LDS beyond the two tile bounds, one 16-byte store per lane.
//
// Both kernels are templates on TPL, chosen by the table: false is the code above and nothing else;
// true (a table with template entries, ReplaceTable::d_ins) makes a piece the up to three runs of
// fac_internal.h piece_run -- entry[..k], the matched text, entry[k..] -- and the cursor's state
// (gap | pre | text | suf).
#include <hip/hip_runtime.h>

#include <algorithm>

#include <rocprim/device/device_scan.hpp>

#include "fac_internal.h"

namespace fac {
namespace {

constexpr uint64_t kSkip = 1ull << 63;  // ReplacePlan::d_plan[i].x: the guard skipped record i
constexpr uint32_t kThreads = 256;
constexpr uint32_t kChunk = 16;  // output bytes per lane
static_assert(kThreads * kChunk == kReplaceTile, "one 16-byte chunk per lane");

// One thread per document (batch_walk_kernel's shape, and its limit: a document with very many
// records is walked by one lane). out_len has n_docs + 1 entries, the last one 0, so the exclusive
// scan's last output is the batch's total.
template <bool TPL>
__global__ void replace_plan_kernel(const fac_match* __restrict__ m, const uint64_t* __restrict__ doc_off,
                                    const uint64_t* __restrict__ offsets, uint64_t n_docs,
                                    const uint2* __restrict__ tab, const uint32_t* __restrict__ ins,
                                    ulonglong2* __restrict__ plan, uint64_t* __restrict__ out_len,
                                    unsigned long long* __restrict__ n_applied) {
  const uint64_t d = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t applied = 0;
  if (d < n_docs) {
    const uint64_t b = doc_off[d], e = doc_off[d + 1];
    const uint64_t dlen = offsets[d + 1] - offsets[d];
    uint64_t last = 0, o = 0;  // matches.rs:170-187
    for (uint64_t i = b; i < e; ++i) {
      const uint64_t ms = m[i].start, me = m[i].end;
      if (ms >= last) {
        const uint64_t gap = ms - last;
        plan[i] = make_ulonglong2(o + gap, last);
        if constexpr (TPL) {
          const uint32_t p = m[i].pattern_index;
          o += gap + piece_len(tab[p], ins[p], me - ms);
        } else {
          const uint32_t rl = tab[m[i].pattern_index].y;
          o += gap + (rl == kReplaceKeep ? me - ms : (uint64_t)rl);
        }
        last = me;
        ++applied;
      } else {
        plan[i] = make_ulonglong2(o | kSkip, last);
      }
    }
    out_len[d] = o + (dlen - last);
  } else if (d == n_docs) {
    out_len[d] = 0;
  }
  for (int off = 32; off > 0; off >>= 1) applied += __shfl_down(applied, off);
  if ((threadIdx.x & 63u) == 0 && applied) atomicAdd(n_applied, (unsigned long long)applied);
}

// last document d in [lo, hi] with out_off[d] <= x (out_off[lo] <= x holds)
__device__ inline uint64_t doc_of(const uint64_t* __restrict__ out_off, uint64_t lo, uint64_t hi, uint64_t x) {
  while (lo < hi) {
    const uint64_t mid = (lo + hi + 1) >> 1;
    if (out_off[mid] <= x) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

template <bool TPL>
__global__ __launch_bounds__(kThreads) void replace_copy_kernel(
    const uint8_t* __restrict__ utf8, const uint64_t* __restrict__ offsets, const uint64_t* __restrict__ out_off,
    uint64_t n_docs, const fac_match* __restrict__ m, const uint64_t* __restrict__ doc_off,
    const ulonglong2* __restrict__ plan, const uint2* __restrict__ tab, const uint32_t* __restrict__ ins,
    const uint8_t* __restrict__ rep, uint8_t* __restrict__ out, uint64_t total, int wide) {
  __shared__ uint64_t s_doc[2];
  const uint64_t tile0 = (uint64_t)blockIdx.x * kReplaceTile;
  if (tile0 >= total) return;
  if (threadIdx.x == 0) {
    const uint64_t tile_last = (total - tile0 < kReplaceTile ? total : tile0 + kReplaceTile) - 1;
    const uint64_t d0 = doc_of(out_off, 0, n_docs - 1, tile0);
    s_doc[0] = d0;
    s_doc[1] = doc_of(out_off, d0, n_docs - 1, tile_last);
  }
  __syncthreads();
  const uint64_t g = tile0 + (uint64_t)threadIdx.x * kChunk;
  if (g >= total) return;
  const uint32_t n = total - g < kChunk ? (uint32_t)(total - g) : kChunk;

  // the lane's first byte: document, then the last record whose piece starts at or before it
  uint64_t d = doc_of(out_off, s_doc[0], s_doc[1], g);
  uint64_t b = doc_off[d], e = doc_off[d + 1];
  uint64_t dbase = offsets[d], dlen = offsets[d + 1] - dbase;
  const uint64_t r = g - out_off[d];
  uint64_t k, skip;
  // 0: the gap before record k (the tail for k == e), 1: record k's piece; TPL: 1-3 = the piece's
  // pre, text and suf runs
  int piece;
  {
    uint64_t lo = b, hi = e;
    while (lo < hi) {
      const uint64_t mid = (lo + hi) >> 1;
      if ((plan[mid].x & ~kSkip) <= r) lo = mid + 1;
      else hi = mid;
    }
    if (lo > b) {  // from the start of that piece; the bytes before r are skipped run by run
      k = lo - 1;
      piece = 1;
      skip = r - (plan[k].x & ~kSkip);
    } else {
      k = b;
      piece = 0;
      skip = r;
    }
  }

  Chunk16 c;  // the lane's 16 bytes
  for (;;) {
    const uint8_t* src = utf8;
    uint64_t rl = 0;
    if (piece == 0) {
      if (k < e) {
        const ulonglong2 pl = plan[k];
        if (!(pl.x & kSkip)) {
          src = utf8 + dbase + pl.y;
          rl = m[k].start - pl.y;
        }
      } else {
        uint64_t last = 0;
        if (e > b) {
          const ulonglong2 pl = plan[e - 1];
          last = (pl.x & kSkip) ? pl.y : m[e - 1].end;
        }
        src = utf8 + dbase + last;
        rl = dlen - last;
      }
    } else if (!(plan[k].x & kSkip)) {
      const uint2 t = tab[m[k].pattern_index];
      if constexpr (TPL) {
        piece_run(t, ins[m[k].pattern_index], rep, utf8 + dbase + m[k].start, m[k].end - m[k].start, piece - 1, src,
                  rl);
      } else if (t.y == kReplaceKeep) {
        src = utf8 + dbase + m[k].start;
        rl = m[k].end - m[k].start;
      } else {
        src = rep + t.x;
        rl = t.y;
      }
    }
    if (skip) {
      const uint64_t t = skip < rl ? skip : rl;
      src += t;
      rl -= t;
      skip -= t;
    }
    if (rl) {
      const uint32_t take = rl < (uint64_t)(n - c.filled) ? (uint32_t)rl : n - c.filled;
      if (take == kChunk) chunk_load16(c, src);
      else chunk_put(c, src, take);
      if (c.filled == n) break;
    }
    // next run
    if (piece) {
      if (!TPL || piece == 3) {
        ++k;
        piece = 0;
      } else {
        ++piece;
      }
    } else if (k < e) {
      piece = 1;
    } else {
      if (++d >= n_docs) break;
      b = doc_off[d];
      e = doc_off[d + 1];
      dbase = offsets[d];
      dlen = offsets[d + 1] - dbase;
      k = b;
    }
  }

  chunk_store(c, out + g, wide);
}

#define RP_TRY(x)                                              \
  do {                                                         \
    hipError_t e_ = (x);                                       \
    if (e_ != hipSuccess) {                                    \
      err = std::string(#x ": ") + hipGetErrorString(e_);      \
      return FAC_E_HIP;                                        \
    }                                                          \
  } while (0)

inline size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace

int replace_plan_device(const Batch& b, const ReplaceTable& t, const fac_match* d_recs, uint64_t n_recs,
                        const uint64_t* d_doc_off, hipStream_t s, ReplacePlan& plan, std::string& err) {
  const uint64_t nd = b.n_docs;
  size_t scan_bytes = 0;
  RP_TRY(rocprim::exclusive_scan(nullptr, scan_bytes, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint64_t)0, nd + 1,
                                 rocprim::plus<uint64_t>(), s));
  // one block of call scratch: plan records, lengths, offsets, {n_applied, total}, the scan's own
  const size_t o_plan = 0, o_len = o_plan + up256(std::max<uint64_t>(n_recs, 1) * sizeof(ulonglong2));
  const size_t o_off = o_len + up256((nd + 1) * 8), o_scal = o_off + up256((nd + 1) * 8);
  const size_t o_tmp = o_scal + 256, bytes = o_tmp + up256(std::max<size_t>(scan_bytes, 16));
  hipError_t he = hipSuccess;
  plan.s = s;
  plan.mem = call_scratch_take(bytes, s, &he);
  if (he != hipSuccess || !plan.mem) {
    plan.mem = nullptr;
    err = std::string("hipMalloc: ") + hipGetErrorString(he);
    return FAC_E_OOM;
  }
  char* base = static_cast<char*>(plan.mem);
  plan.d_plan = reinterpret_cast<ulonglong2*>(base + o_plan);
  uint64_t* d_len = reinterpret_cast<uint64_t*>(base + o_len);
  plan.d_out_off = reinterpret_cast<uint64_t*>(base + o_off);
  unsigned long long* d_scal = reinterpret_cast<unsigned long long*>(base + o_scal);
  RP_TRY(hipMemsetAsync(d_scal, 0, 16, s));
  const auto plan_kernel = t.d_ins ? replace_plan_kernel<true> : replace_plan_kernel<false>;
  hipLaunchKernelGGL(plan_kernel, dim3((uint32_t)((nd + 1 + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, d_recs,
                     d_doc_off, b.d_offsets, nd, t.d_tab, t.d_ins, plan.d_plan, d_len, d_scal);
  RP_TRY(hipGetLastError());
  RP_TRY(rocprim::exclusive_scan(base + o_tmp, scan_bytes, d_len, plan.d_out_off, (uint64_t)0, nd + 1,
                                 rocprim::plus<uint64_t>(), s));
  RP_TRY(hipMemcpyAsync(d_scal + 1, plan.d_out_off + nd, 8, hipMemcpyDeviceToDevice, s));
  unsigned long long scal[2] = {0, 0};
  RP_TRY(hipMemcpyAsync(scal, d_scal, 16, hipMemcpyDeviceToHost, s));
  RP_TRY(hipStreamSynchronize(s));
  plan.n_replaced = scal[0];
  plan.total = scal[1];
  return FAC_OK;
}

int replace_copy_device(const Batch& b, const ReplaceTable& t, const fac_match* d_recs, const uint64_t* d_doc_off,
                        const ReplacePlan& plan, uint8_t* d_out, std::string& err) {
  if (!plan.total) return FAC_OK;  // (then no document has output, and n_docs may be 0)
  const uint64_t tiles = (plan.total + kReplaceTile - 1) / kReplaceTile;  // < 2^28: total < 2^40
  const int wide = (reinterpret_cast<uintptr_t>(d_out) & 15u) == 0 ? 1 : 0;
  const auto copy_kernel = t.d_ins ? replace_copy_kernel<true> : replace_copy_kernel<false>;
  hipLaunchKernelGGL(copy_kernel, dim3((uint32_t)tiles), dim3(kThreads), 0, plan.s, b.h.d_utf8, b.d_offsets,
                     plan.d_out_off, b.n_docs, d_recs, d_doc_off, plan.d_plan, t.d_tab, t.d_ins, t.d_bytes, d_out,
                     plan.total, wide);
  RP_TRY(hipGetLastError());
  return FAC_OK;
}

}  // namespace fac
