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
//
// A run of consecutive stream windows (fac_replace_windows_staged_device, the replace stream's tasks)
// is one long document with a plan of its own -- stream_carry_kernel, stream_delta_kernel,
// stream_plan_kernel below -- and the same copy kernel.
#include <hip/hip_runtime.h>

#include <algorithm>

#include <rocprim/device/device_scan.hpp>

#include "fac_internal.h"
#include "host_util.h"

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

// ---- the plan of one long document: a run of consecutive stream windows (stream.rs:465-517 with
// ReplaceCursor::emit_window, :645-705). The records of window w are m[win_off[w], win_off[w + 1]),
// sorted by (start, end); commit[w] is the window's commit point; every offset is a byte of the
// resident text. The guard `match_start < emitted` (:671) skips a prefix of each window's records and
// nothing else: kept records of one window do not overlap, so once a record is applied `emitted` is
// its end and every later record of the window starts at or after it. The cursor on entering window
// w + 1 is therefore max(commit[w], end of w's last record if that record is applied, else the cursor
// on entering w): a chain of W steps that reads one record per window, after which every record
// knows its fate from its own window's cursor.

constexpr uint32_t kCarryThreads = 256;

// One workgroup. Per round, 256 windows' last records and commit points are loaded in parallel into
// LDS, lane 0 runs the 256 chain steps out of LDS, and the cursors go back in parallel. cur has W + 1
// entries (cur[w] = `emitted` on entering window w, cur[W] = on leaving the last one), prev has W
// (the end of the last record applied before window w, e_in if none: where the verbatim text before
// the window's first applied record starts).
__global__ __launch_bounds__(kCarryThreads) void stream_carry_kernel(
    const fac_match* __restrict__ m, const uint64_t* __restrict__ win_off, const uint64_t* __restrict__ commit,
    uint64_t n_windows, uint64_t e_in, uint64_t* __restrict__ cur, uint64_t* __restrict__ prev) {
  __shared__ uint64_t s_start[kCarryThreads], s_end[kCarryThreads], s_commit[kCarryThreads];
  __shared__ uint64_t s_cur[kCarryThreads], s_prev[kCarryThreads];
  __shared__ uint64_t s_carry[2];  // the cursor and the last applied end between rounds
  constexpr uint64_t kNone = ~0ull;  // a window without records (no start is this large)
  if (threadIdx.x == 0) {
    s_carry[0] = e_in;
    s_carry[1] = e_in;
  }
  for (uint64_t w0 = 0; w0 < n_windows; w0 += kCarryThreads) {
    const uint64_t w = w0 + threadIdx.x;
    if (w < n_windows) {
      const uint64_t lo = win_off[w], hi = win_off[w + 1];
      s_start[threadIdx.x] = hi > lo ? m[hi - 1].start : kNone;
      s_end[threadIdx.x] = hi > lo ? m[hi - 1].end : 0;
      s_commit[threadIdx.x] = commit[w];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      uint64_t e = s_carry[0], p = s_carry[1];
      const uint32_t cnt = n_windows - w0 < kCarryThreads ? (uint32_t)(n_windows - w0) : kCarryThreads;
      for (uint32_t i = 0; i < cnt; ++i) {
        s_cur[i] = e;
        s_prev[i] = p;
        if (s_start[i] != kNone && s_start[i] >= e) e = p = s_end[i];
        if (s_commit[i] > e) e = s_commit[i];
      }
      s_carry[0] = e;
      s_carry[1] = p;
    }
    __syncthreads();
    if (w < n_windows) {
      cur[w] = s_cur[threadIdx.x];
      prev[w] = s_prev[threadIdx.x];
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) cur[n_windows] = s_carry[0];
}

// the window of record i: win_off[w] <= i < win_off[w + 1] (windows without records are stepped over)
__device__ inline uint64_t window_of(const uint64_t* __restrict__ win_off, uint64_t n_windows, uint64_t i) {
  uint64_t lo = 0, hi = n_windows;  // first w in [0, n_windows] with win_off[w] > i, minus one
  while (lo < hi) {
    const uint64_t mid = (lo + hi) >> 1;
    if (win_off[mid] <= i) lo = mid + 1;
    else hi = mid;
  }
  return lo - 1;
}

// One thread per record: what the record adds to the output beyond its own span's bytes (wrapping:
// a deletion adds a negative length), 0 for a skipped record and for entry n, so that the exclusive
// sum's entry n is the whole call's.
template <bool TPL>
__global__ void stream_delta_kernel(const fac_match* __restrict__ m, uint64_t n, const uint64_t* __restrict__ win_off,
                                    uint64_t n_windows, const uint64_t* __restrict__ cur,
                                    const uint2* __restrict__ tab, const uint32_t* __restrict__ ins,
                                    uint64_t* __restrict__ delta) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i > n) return;
  uint64_t d = 0;
  if (i < n) {
    const uint64_t ms = m[i].start, me = m[i].end;
    if (ms >= cur[window_of(win_off, n_windows, i)]) {
      const uint32_t p = m[i].pattern_index;
      uint64_t pl;
      if constexpr (TPL) {
        pl = piece_len(tab[p], ins[p], me - ms);
      } else {
        const uint32_t rl = tab[p].y;
        pl = rl == kReplaceKeep ? me - ms : (uint64_t)rl;
      }
      d = pl - (me - ms);
    }
  }
  delta[i] = d;
}

// One thread per record: its ReplacePlan entry and its copy rebased to the call's source range, the
// one "document" replace_copy_kernel then walks: bytes [e_in, cur[W]) of the text. dsum is the
// exclusive sum of stream_delta_kernel's values. The verbatim text before an applied record starts at
// the end of the record before it if that one is applied too (it is in the same window), else at
// prev[w]; the flush up to a commit point is part of that run, or of the tail. Thread n writes the
// view (view[0..1] the document's byte range, view[2..3] its record range, view[4..5] its output
// range) and scal = {applied records, output bytes, cur[W]}.
__global__ void stream_plan_kernel(const fac_match* __restrict__ m, uint64_t n, const uint64_t* __restrict__ win_off,
                                   uint64_t n_windows, const uint64_t* __restrict__ cur,
                                   const uint64_t* __restrict__ prev, const uint64_t* __restrict__ dsum, uint64_t e_in,
                                   ulonglong2* __restrict__ plan, fac_match* __restrict__ out_m,
                                   uint64_t* __restrict__ view, unsigned long long* __restrict__ scal) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t applied = 0;
  if (i < n) {
    const uint64_t w = window_of(win_off, n_windows, i), e = cur[w];
    fac_match r = m[i];
    uint64_t last = prev[w];
    if (r.start >= e) {
      applied = 1;
      if (i > win_off[w] && m[i - 1].start >= e) last = m[i - 1].end;
      plan[i] = make_ulonglong2((r.start - e_in) + dsum[i], last - e_in);
    } else {
      plan[i] = make_ulonglong2(((last - e_in) + dsum[i]) | kSkip, last - e_in);
    }
    r.start -= e_in;  // (a skipped record may start before e_in: the copy never reads its span)
    r.end -= e_in;
    out_m[i] = r;
  } else if (i == n) {
    const uint64_t e_out = cur[n_windows], total = (e_out - e_in) + dsum[n];
    view[0] = e_in;
    view[1] = e_out;
    view[2] = 0;
    view[3] = n;
    view[4] = 0;
    view[5] = total;
    scal[1] = total;
    scal[2] = e_out;
  }
  for (int off = 32; off > 0; off >>= 1) applied += __shfl_down(applied, off);
  if ((threadIdx.x & 63u) == 0 && applied) atomicAdd(scal, (unsigned long long)applied);
}

}  // namespace

int replace_plan_device(const Batch& b, const ReplaceTable& t, const fac_match* d_recs, uint64_t n_recs,
                        const uint64_t* d_doc_off, hipStream_t s, ReplacePlan& plan, std::string& err) {
  const uint64_t nd = b.n_docs;
  size_t scan_bytes = 0;
  HIP_TRY(rocprim::exclusive_scan(nullptr, scan_bytes, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint64_t)0, nd + 1,
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
  HIP_TRY(hipMemsetAsync(d_scal, 0, 16, s));
  const auto plan_kernel = t.d_ins ? replace_plan_kernel<true> : replace_plan_kernel<false>;
  hipLaunchKernelGGL(plan_kernel, dim3((uint32_t)((nd + 1 + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, d_recs,
                     d_doc_off, b.d_offsets, nd, t.d_tab, t.d_ins, plan.d_plan, d_len, d_scal);
  HIP_TRY(hipGetLastError());
  HIP_TRY(rocprim::exclusive_scan(base + o_tmp, scan_bytes, d_len, plan.d_out_off, (uint64_t)0, nd + 1,
                                 rocprim::plus<uint64_t>(), s));
  HIP_TRY(hipMemcpyAsync(d_scal + 1, plan.d_out_off + nd, 8, hipMemcpyDeviceToDevice, s));
  unsigned long long scal[2] = {0, 0};
  HIP_TRY(hipMemcpyAsync(scal, d_scal, 16, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  plan.n_replaced = scal[0];
  plan.total = scal[1];
  return FAC_OK;
}

namespace {
// replace_copy_kernel over n_docs documents [d_offsets[d], d_offsets[d + 1]) of d_utf8
int launch_copy(const uint8_t* d_utf8, const uint64_t* d_offsets, uint64_t n_docs, const ReplaceTable& t,
                const fac_match* d_recs, const uint64_t* d_doc_off, const ReplacePlan& plan, uint8_t* d_out,
                std::string& err) {
  if (!plan.total) return FAC_OK;  // (then no document has output, and n_docs may be 0)
  const uint64_t tiles = (plan.total + kReplaceTile - 1) / kReplaceTile;  // < 2^28: total < 2^40
  const int wide = (reinterpret_cast<uintptr_t>(d_out) & 15u) == 0 ? 1 : 0;
  const auto copy_kernel = t.d_ins ? replace_copy_kernel<true> : replace_copy_kernel<false>;
  hipLaunchKernelGGL(copy_kernel, dim3((uint32_t)tiles), dim3(kThreads), 0, plan.s, d_utf8, d_offsets, plan.d_out_off,
                     n_docs, d_recs, d_doc_off, plan.d_plan, t.d_tab, t.d_ins, t.d_bytes, d_out, plan.total, wide);
  HIP_TRY(hipGetLastError());
  return FAC_OK;
}
}  // namespace

int replace_copy_device(const Batch& b, const ReplaceTable& t, const fac_match* d_recs, const uint64_t* d_doc_off,
                        const ReplacePlan& plan, uint8_t* d_out, std::string& err) {
  return launch_copy(b.h.d_utf8, b.d_offsets, b.n_docs, t, d_recs, d_doc_off, plan, d_out, err);
}

int replace_stream_plan_device(const ReplaceTable& t, std::vector<fac_match>& recs, const std::vector<uint64_t>& win_off,
                               const std::vector<uint64_t>& commit, uint64_t e_in, hipStream_t s, StreamReplacePlan& plan,
                               std::string& err) {
  const uint64_t n = recs.size(), nw = commit.size();
  // (start, end) order within a window (stream.rs:515); the ranking leaves records of equal start in
  // acceptance order, which differs only where an empty span shares its start (matches.rs:93-99)
  auto by_span = [](const fac_match& a, const fac_match& b) { return a.start != b.start ? a.start < b.start : a.end < b.end; };
  if (!std::is_sorted(recs.begin(), recs.end(), by_span))  // (a whole run in order: every window is)
    for (uint64_t w = 0; w < nw; ++w)
      std::sort(recs.begin() + (ptrdiff_t)win_off[w], recs.begin() + (ptrdiff_t)win_off[w + 1], by_span);
  // one block of call scratch: records in and out, plan, delta and its sum, the windows, the cursors
  const size_t rec_b = up256(std::max<uint64_t>(n, 1) * sizeof(fac_match));
  const size_t o_in = 0, o_out = o_in + rec_b, o_plan = o_out + rec_b;
  const size_t o_delta = o_plan + up256(std::max<uint64_t>(n, 1) * sizeof(ulonglong2)), o_sum = o_delta + up256((n + 1) * 8);
  const size_t o_woff = o_sum + up256((n + 1) * 8), o_commit = o_woff + up256((nw + 1) * 8);
  const size_t o_cur = o_commit + up256((nw + 1) * 8), o_prev = o_cur + up256((nw + 1) * 8);
  const size_t o_view = o_prev + up256((nw + 1) * 8), o_scal = o_view + 256, bytes = o_scal + 256;
  hipError_t he = hipSuccess;
  plan.s = s;
  plan.mem = call_scratch_take(bytes, s, &he);
  if (he != hipSuccess || !plan.mem) {
    plan.mem = nullptr;
    err = std::string("hipMalloc: ") + hipGetErrorString(he);
    return FAC_E_OOM;
  }
  char* base = static_cast<char*>(plan.mem);
  fac_match* d_in = reinterpret_cast<fac_match*>(base + o_in);
  plan.d_recs = reinterpret_cast<fac_match*>(base + o_out);
  plan.d_plan = reinterpret_cast<ulonglong2*>(base + o_plan);
  uint64_t* d_delta = reinterpret_cast<uint64_t*>(base + o_delta);
  uint64_t* d_sum = reinterpret_cast<uint64_t*>(base + o_sum);
  uint64_t* d_woff = reinterpret_cast<uint64_t*>(base + o_woff);
  uint64_t* d_commit = reinterpret_cast<uint64_t*>(base + o_commit);
  uint64_t* d_cur = reinterpret_cast<uint64_t*>(base + o_cur);
  uint64_t* d_prev = reinterpret_cast<uint64_t*>(base + o_prev);
  plan.d_view = reinterpret_cast<uint64_t*>(base + o_view);
  plan.d_out_off = plan.d_view + 4;
  unsigned long long* d_scal = reinterpret_cast<unsigned long long*>(base + o_scal);
  HIP_TRY(hipMemsetAsync(d_scal, 0, 24, s));
  if (n) HIP_TRY(hipMemcpyAsync(d_in, recs.data(), n * sizeof(fac_match), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(d_woff, win_off.data(), (nw + 1) * 8, hipMemcpyHostToDevice, s));
  if (nw) HIP_TRY(hipMemcpyAsync(d_commit, commit.data(), nw * 8, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(stream_carry_kernel, dim3(1), dim3(kCarryThreads), 0, s, d_in, d_woff, d_commit, nw, e_in, d_cur,
                     d_prev);
  const dim3 grid((uint32_t)((n + 1 + kThreads - 1) / kThreads));
  const auto delta_kernel = t.d_ins ? stream_delta_kernel<true> : stream_delta_kernel<false>;
  hipLaunchKernelGGL(delta_kernel, grid, dim3(kThreads), 0, s, d_in, n, d_woff, nw, d_cur, t.d_tab, t.d_ins, d_delta);
  HIP_TRY(hipGetLastError());
  if (int rc = exclusive_sum_u64(d_delta, d_sum, n + 1, s, err)) return rc;
  hipLaunchKernelGGL(stream_plan_kernel, grid, dim3(kThreads), 0, s, d_in, n, d_woff, nw, d_cur, d_prev, d_sum, e_in,
                     plan.d_plan, plan.d_recs, plan.d_view, d_scal);
  HIP_TRY(hipGetLastError());
  unsigned long long scal[3] = {0, 0, 0};
  HIP_TRY(hipMemcpyAsync(scal, d_scal, 24, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));  // (also: the pageable uploads above were read)
  plan.n_replaced = scal[0];
  plan.n_skipped = n - scal[0];
  plan.total = scal[1];
  plan.e_out = scal[2];
  return FAC_OK;
}

int replace_stream_copy_device(const uint8_t* d_text, const ReplaceTable& t, const StreamReplacePlan& plan, uint8_t* d_out,
                               std::string& err) {
  return launch_copy(d_text, plan.d_view, 1, t, plan.d_recs, plan.d_view + 2, plan, d_out, err);
}

}  // namespace fac
