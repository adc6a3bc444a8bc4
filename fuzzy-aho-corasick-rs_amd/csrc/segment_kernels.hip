// segment_kernels.hip — the segmentation helpers of a batch on the MI355X: segment_iter, split,
// strip_prefix, strip_suffix and segment_text (src/matches.rs:218-594) for every document of a
// staged batch, after the per-document apply (rank_kernels.hip apply_batch_device) left the kept
// records in (document, start, acceptance) order.
//
// A document's segments are gap 0, record 0, gap 1, record 1, ..., tail (matches.rs:526-553): a
// record that starts before `last` is dropped by the guard, an empty gap emits nothing, a kept
// record always emits a matched segment (an empty one for an empty span). They tile [0, len).
//
// * segment_plan_kernel<mode>: one thread per document walks its records once (replace_plan_kernel's
//   shape and limit) and writes what the mode needs: the segment count; for a strip the offset of
//   the kept suffix / the length of the kept prefix; for segment_text the output length.
// * one rocPRIM exclusive scan per output turns counts and lengths into n_docs + 1 offsets.
// * segment_write_kernel: the same walk again, every segment written as a fac_match.
// * segment_pieces_kernel (segment_text): the same walk again, one "piece" per segment.
// * piece_copy_kernel: output-stationary byte mover over pieces, each an optional U+0020 plus a run
//   of source bytes. A strip is one piece per document, segment_text one piece per segment, so one
//   mover serves the three render modes. A workgroup owns kSegmentTile consecutive output bytes, a
//   lane 16 of them; the tile's first and last pieces are found once per tile, a lane bisects only
//   between them and then steps from piece to piece (pieces of length 0 are stepped over) until
//   its 16 bytes are full. No atomics, no LDS beyond the two tile bounds, one 16-byte store per lane.
#include <hip/hip_runtime.h>

#include <algorithm>

#include <rocprim/device/device_scan.hpp>

#include "fac_internal.h"
#include "host_util.h"

namespace fac {
namespace {

constexpr uint64_t kSpace = 1ull << 63;  // piece source: a U+0020 goes before the run
constexpr uint32_t kThreads = 256;
constexpr uint32_t kChunk = 16;  // output bytes per lane
static_assert(kThreads * kChunk == kSegmentTile, "one 16-byte chunk per lane");

// Rust's char::is_whitespace (the Unicode White_Space property, 25 code points, all <= 3 bytes of
// UTF-8) on the character that starts at p; `n` bytes are readable. Returns its byte length, 0 if
// the character is not whitespace.
__device__ inline uint32_t white_space_at(const uint8_t* __restrict__ p, uint64_t n) {
  const uint32_t b0 = p[0];
  if ((b0 >= 0x09 && b0 <= 0x0D) || b0 == 0x20) return 1;
  if (b0 < 0xC2 || b0 > 0xE3 || n < 2) return 0;
  const uint32_t b1 = p[1];
  if (b0 == 0xC2) return (b1 == 0x85 || b1 == 0xA0) ? 2 : 0;  // U+0085, U+00A0
  if (n < 3) return 0;
  const uint32_t b2 = p[2];
  if (b0 == 0xE1) return (b1 == 0x9A && b2 == 0x80) ? 3 : 0;  // U+1680
  if (b0 == 0xE2) {
    if (b1 == 0x80)  // U+2000-U+200A, U+2028, U+2029, U+202F
      return ((b2 >= 0x80 && b2 <= 0x8A) || b2 == 0xA8 || b2 == 0xA9 || b2 == 0xAF) ? 3 : 0;
    return (b1 == 0x81 && b2 == 0x9F) ? 3 : 0;  // U+205F
  }
  if (b0 == 0xE3) return (b1 == 0x80 && b2 == 0x80) ? 3 : 0;  // U+3000
  return 0;
}

// trim_start of doc[s, e): the offset of its first non-whitespace character, e if there is none
__device__ inline uint64_t trim_start(const uint8_t* __restrict__ doc, uint64_t s, uint64_t e) {
  while (s < e) {
    const uint32_t w = white_space_at(doc + s, e - s);
    if (!w) break;
    s += w;
  }
  return s;
}

// trim_end of doc[s, e): the end of its last non-whitespace character, s if there is none. Steps
// back over continuation bytes (the documents are validated UTF-8, segments end at boundaries).
__device__ inline uint64_t trim_end(const uint8_t* __restrict__ doc, uint64_t s, uint64_t e) {
  while (e > s) {
    uint64_t p = e - 1;
    while (p > s && (doc[p] & 0xC0u) == 0x80u) --p;
    if (white_space_at(doc + p, e - p) != e - p) break;
    e = p;
  }
  return e;
}

// matches.rs:560-564: an unmatched segment that starts with one of , . ? ! ; : — - … gets no space
__device__ inline bool no_leading_space(const uint8_t* __restrict__ p, uint64_t n) {
  const uint32_t b0 = p[0];
  if (b0 == ',' || b0 == '.' || b0 == '?' || b0 == '!' || b0 == ';' || b0 == ':' || b0 == '-') return true;
  return b0 == 0xE2 && n >= 3 && p[1] == 0x80 && (p[2] == 0x94 || p[2] == 0xA6);  // U+2014, U+2026
}

// segment_iter (matches.rs:526-553) over records [b, e) of a document of dlen bytes:
// f(matched, record index, start, end) per segment, in order.
template <class F>
__device__ inline void walk_segments(const fac_match* __restrict__ m, uint64_t b, uint64_t e, uint64_t dlen, F&& f) {
  uint64_t last = 0;
  for (uint64_t i = b; i < e; ++i) {
    const uint64_t ms = m[i].start, me = m[i].end;
    if (ms < last) continue;
    if (ms > last) f(false, i, last, ms);
    f(true, i, ms, me);
    last = me;
  }
  if (last < dlen) f(false, e, last, dlen);
}

// The segment_text walker (matches.rs:566-594): whether a U+0020 goes before the next segment. It
// carries the accumulated result's emptiness and last byte (both space characters are ASCII), since
// an empty matched segment pushes no bytes.
struct TextWalker {
  bool prev_matched = false, empty = true;
  uint32_t last_byte = 0;
  __device__ inline bool step(const uint8_t* __restrict__ doc, bool matched, uint64_t s, uint64_t e) {
    bool space;
    if (matched) {
      space = prev_matched || (!empty && last_byte != 0x20 && last_byte != 0x09);
      prev_matched = true;
    } else {
      space = prev_matched && !no_leading_space(doc + s, e - s);
      prev_matched = false;
    }
    if (space) {
      empty = false;
      last_byte = 0x20;
    }
    if (e > s) {
      empty = false;
      last_byte = doc[e - 1];
    }
    return space;
  }
};

// One thread per document. cnt / len have n_docs + 1 entries, the last one 0, so an exclusive
// scan's last output is the batch's total. src (strips): the global byte the document's piece
// starts at.
template <int MODE>
__global__ void segment_plan_kernel(const fac_match* __restrict__ m, const uint64_t* __restrict__ doc_off,
                                    const uint8_t* __restrict__ utf8, const uint64_t* __restrict__ offsets,
                                    uint64_t n_docs, uint64_t* __restrict__ cnt, uint64_t* __restrict__ len,
                                    uint64_t* __restrict__ src) {
  const uint64_t d = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (d > n_docs) return;
  if (d == n_docs) {
    if (MODE >= kRenderSegmentText) cnt[d] = 0;
    if (MODE <= kRenderSegmentText) len[d] = 0;
    return;
  }
  const uint64_t base = offsets[d], dlen = offsets[d + 1] - base;
  const uint8_t* doc = utf8 + base;
  const uint64_t b = doc_off[d], e = doc_off[d + 1];
  if (MODE == kRenderStripPrefix) {  // matches.rs:218-245: doc[a..]
    uint64_t a = dlen;
    walk_segments(m, b, e, dlen, [&](bool matched, uint64_t, uint64_t s, uint64_t t) {
      if (matched || a != dlen) return;
      const uint64_t x = trim_start(doc, s, t);
      if (x < t) a = x;
    });
    len[d] = dlen - a;
    src[d] = base + a;
  } else if (MODE == kRenderStripSuffix) {  // matches.rs:276-307: doc[..z]
    uint64_t z = 0;
    walk_segments(m, b, e, dlen, [&](bool matched, uint64_t, uint64_t s, uint64_t t) {
      if (matched) return;
      const uint64_t x = trim_end(doc, s, t);
      if (x > s) z = x;
    });
    len[d] = z;
    src[d] = base;
  } else if (MODE == kRenderSegmentText) {
    TextWalker w;
    uint64_t n = 0, o = 0;
    walk_segments(m, b, e, dlen, [&](bool matched, uint64_t, uint64_t s, uint64_t t) {
      ++n;
      o += (w.step(doc, matched, s, t) ? 1u : 0u) + (t - s);
    });
    cnt[d] = n;
    len[d] = o;
  } else {
    uint64_t n = 0;
    walk_segments(m, b, e, dlen, [&](bool, uint64_t, uint64_t, uint64_t) { ++n; });
    cnt[d] = n;
  }
}

// One thread per document: segment k of document d is out[seg_off[d] + k]. A matched segment is the
// kept record verbatim, an unmatched one {start, end, FAC_UNMATCHED, 0, ...}. `out` is 8-byte aligned.
__global__ void segment_write_kernel(const fac_match* __restrict__ m, const uint64_t* __restrict__ doc_off,
                                     const uint64_t* __restrict__ offsets, uint64_t n_docs,
                                     const uint64_t* __restrict__ seg_off, fac_match* __restrict__ out) {
  const uint64_t d = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= n_docs) return;
  const uint64_t dlen = offsets[d + 1] - offsets[d];
  uint64_t k = seg_off[d];
  const uint64_t k_end = seg_off[d + 1];
  walk_segments(m, doc_off[d], doc_off[d + 1], dlen, [&](bool matched, uint64_t i, uint64_t s, uint64_t t) {
    if (k >= k_end) return;  // (the plan counted the same walk)
    const uint64_t* from = reinterpret_cast<const uint64_t*>(m + i);
    uint64_t* to = reinterpret_cast<uint64_t*>(out + k);
    to[0] = s;
    to[1] = t;
    to[2] = matched ? from[2] : (uint64_t)FAC_UNMATCHED;  // pattern_index, similarity (0.0f)
    to[3] = matched ? from[3] : 0;                        // the counts and the padding
    ++k;
  });
}

// One thread per document (segment_text): piece seg_off[d] + k is segment k of document d, its
// output offset and its source {global byte | kSpace}. Thread n_docs writes the closing offset.
__global__ void segment_pieces_kernel(const fac_match* __restrict__ m, const uint64_t* __restrict__ doc_off,
                                      const uint8_t* __restrict__ utf8, const uint64_t* __restrict__ offsets,
                                      uint64_t n_docs, const uint64_t* __restrict__ seg_off,
                                      const uint64_t* __restrict__ out_off, uint64_t* __restrict__ piece_out,
                                      uint64_t* __restrict__ piece_src) {
  const uint64_t d = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (d > n_docs) return;
  if (d == n_docs) {
    piece_out[seg_off[d]] = out_off[d];
    return;
  }
  const uint64_t base = offsets[d], dlen = offsets[d + 1] - base;
  const uint8_t* doc = utf8 + base;
  TextWalker w;
  uint64_t k = seg_off[d], o = out_off[d];
  const uint64_t k_end = seg_off[d + 1];
  walk_segments(m, doc_off[d], doc_off[d + 1], dlen, [&](bool matched, uint64_t, uint64_t s, uint64_t t) {
    if (k >= k_end) return;
    const bool space = w.step(doc, matched, s, t);
    piece_out[k] = o;
    piece_src[k] = (base + s) | (space ? kSpace : 0);
    o += (space ? 1u : 0u) + (t - s);
    ++k;
  });
}

// last piece p in [lo, hi] with piece_out[p] <= x (piece_out[lo] <= x holds)
__device__ inline uint64_t piece_of(const uint64_t* __restrict__ piece_out, uint64_t lo, uint64_t hi, uint64_t x) {
  while (lo < hi) {
    const uint64_t mid = (lo + hi + 1) >> 1;
    if (piece_out[mid] <= x) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// piece_out has n_pieces + 1 entries (the last one = total), n_pieces >= 1, total >= 1.
__global__ __launch_bounds__(kThreads) void piece_copy_kernel(const uint8_t* __restrict__ utf8,
                                                              const uint64_t* __restrict__ piece_out,
                                                              const uint64_t* __restrict__ piece_src, uint64_t n_pieces,
                                                              uint8_t* __restrict__ out, uint64_t total, int wide) {
  __shared__ uint64_t s_piece[2];
  const uint64_t tile0 = (uint64_t)blockIdx.x * kSegmentTile;
  if (tile0 >= total) return;
  if (threadIdx.x == 0) {
    const uint64_t tile_last = (total - tile0 < kSegmentTile ? total : tile0 + kSegmentTile) - 1;
    const uint64_t p0 = piece_of(piece_out, 0, n_pieces - 1, tile0);
    s_piece[0] = p0;
    s_piece[1] = piece_of(piece_out, p0, n_pieces - 1, tile_last);
  }
  __syncthreads();
  const uint64_t g = tile0 + (uint64_t)threadIdx.x * kChunk;
  if (g >= total) return;
  const uint32_t n = total - g < kChunk ? (uint32_t)(total - g) : kChunk;

  // the lane's first byte lies in piece p (the last one that starts at or before it, so not empty)
  uint64_t p = piece_of(piece_out, s_piece[0], s_piece[1], g);
  uint64_t po = piece_out[p];
  uint64_t skip = g - po;
  Chunk16 c;  // the lane's 16 bytes
  for (;;) {
    const uint64_t pn = piece_out[p + 1], ps = piece_src[p];
    const uint8_t* src = utf8 + (ps & ~kSpace);
    uint64_t rl = pn - po;  // the piece's bytes: the space, then the run
    if ((ps & kSpace) && rl) {
      --rl;
      if (skip) {
        --skip;
      } else {
        chunk_put(c, 0x20);
        if (c.filled == n) break;
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
    if (++p >= n_pieces) break;
    po = pn;
  }

  chunk_store(c, out + g, wide);
}

inline dim3 doc_grid(uint64_t nd) { return dim3((uint32_t)((nd + 1 + kThreads - 1) / kThreads)); }

}  // namespace

int segment_plan_device(const Batch& b, int mode, const fac_match* d_recs, const uint64_t* d_doc_off, hipStream_t s,
                        SegmentPlan& plan, std::string& err) {
  const uint64_t nd = b.n_docs;
  const bool want_cnt = mode >= kRenderSegmentText, want_len = mode <= kRenderSegmentText;
  size_t scan_bytes = 0;
  HIP_TRY(rocprim::exclusive_scan(nullptr, scan_bytes, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint64_t)0, nd + 1,
                                 rocprim::plus<uint64_t>(), s));
  // one block of call scratch: counts, segment offsets, lengths, output offsets, sources, the scan's own
  const size_t col = up256((nd + 1) * 8);
  const size_t o_cnt = 0, o_seg = col, o_len = 2 * col, o_off = 3 * col, o_src = 4 * col, o_tmp = 5 * col;
  const size_t bytes = o_tmp + up256(std::max<size_t>(scan_bytes, 16));
  hipError_t he = hipSuccess;
  plan.s = s;
  plan.mode = mode;
  plan.mem = call_scratch_take(bytes, s, &he);
  if (he != hipSuccess || !plan.mem) {
    plan.mem = nullptr;
    err = std::string("hipMalloc: ") + hipGetErrorString(he);
    return FAC_E_OOM;
  }
  char* base = static_cast<char*>(plan.mem);
  uint64_t* d_cnt = reinterpret_cast<uint64_t*>(base + o_cnt);
  uint64_t* d_len = reinterpret_cast<uint64_t*>(base + o_len);
  plan.d_seg_off = reinterpret_cast<uint64_t*>(base + o_seg);
  plan.d_out_off = reinterpret_cast<uint64_t*>(base + o_off);
  plan.d_src = reinterpret_cast<uint64_t*>(base + o_src);
#define SG_PLAN(M)                                                                                             \
  hipLaunchKernelGGL(segment_plan_kernel<M>, doc_grid(nd), dim3(kThreads), 0, s, d_recs, d_doc_off, b.h.d_utf8, \
                     b.d_offsets, nd, d_cnt, d_len, plan.d_src)
  switch (mode) {
    case kRenderStripPrefix: SG_PLAN(kRenderStripPrefix); break;
    case kRenderStripSuffix: SG_PLAN(kRenderStripSuffix); break;
    case kRenderSegmentText: SG_PLAN(kRenderSegmentText); break;
    default: SG_PLAN(kSegmentRecords); break;
  }
#undef SG_PLAN
  HIP_TRY(hipGetLastError());
  unsigned long long scal[2] = {0, 0};  // {segments, output bytes}
  if (want_cnt) {
    HIP_TRY(rocprim::exclusive_scan(base + o_tmp, scan_bytes, d_cnt, plan.d_seg_off, (uint64_t)0, nd + 1,
                                   rocprim::plus<uint64_t>(), s));
    HIP_TRY(hipMemcpyAsync(&scal[0], plan.d_seg_off + nd, 8, hipMemcpyDeviceToHost, s));
  }
  if (want_len) {
    HIP_TRY(rocprim::exclusive_scan(base + o_tmp, scan_bytes, d_len, plan.d_out_off, (uint64_t)0, nd + 1,
                                   rocprim::plus<uint64_t>(), s));
    HIP_TRY(hipMemcpyAsync(&scal[1], plan.d_out_off + nd, 8, hipMemcpyDeviceToHost, s));
  }
  HIP_TRY(hipStreamSynchronize(s));
  plan.n_segs = scal[0];
  plan.total = scal[1];
  return FAC_OK;
}

int segment_write_device(const Batch& b, const fac_match* d_recs, const uint64_t* d_doc_off, const SegmentPlan& plan,
                         fac_match* d_out, std::string& err) {
  if (!plan.n_segs) return FAC_OK;
  hipLaunchKernelGGL(segment_write_kernel, doc_grid(b.n_docs), dim3(kThreads), 0, plan.s, d_recs, d_doc_off, b.d_offsets,
                     b.n_docs, plan.d_seg_off, d_out);
  HIP_TRY(hipGetLastError());
  return FAC_OK;
}

int render_copy_device(const Batch& b, const fac_match* d_recs, const uint64_t* d_doc_off, SegmentPlan& plan,
                       uint8_t* d_out, std::string& err) {
  if (!plan.total) return FAC_OK;  // (then no document has output, and n_docs may be 0)
  const uint64_t nd = b.n_docs;
  const uint64_t* piece_out = plan.d_out_off;  // a strip: one piece per document
  const uint64_t* piece_src = plan.d_src;
  uint64_t n_pieces = nd;
  if (plan.mode == kRenderSegmentText) {
    const size_t o_src = up256((plan.n_segs + 1) * 8);
    hipError_t he = hipSuccess;
    plan.mem_pieces = call_scratch_take(o_src + up256(std::max<uint64_t>(plan.n_segs, 1) * 8), plan.s, &he);
    if (he != hipSuccess || !plan.mem_pieces) {
      plan.mem_pieces = nullptr;
      err = std::string("hipMalloc: ") + hipGetErrorString(he);
      return FAC_E_OOM;
    }
    uint64_t* po = reinterpret_cast<uint64_t*>(plan.mem_pieces);
    uint64_t* ps = reinterpret_cast<uint64_t*>(static_cast<char*>(plan.mem_pieces) + o_src);
    hipLaunchKernelGGL(segment_pieces_kernel, doc_grid(nd), dim3(kThreads), 0, plan.s, d_recs, d_doc_off, b.h.d_utf8,
                       b.d_offsets, nd, plan.d_seg_off, plan.d_out_off, po, ps);
    HIP_TRY(hipGetLastError());
    piece_out = po;
    piece_src = ps;
    n_pieces = plan.n_segs;
  }
  const uint64_t tiles = (plan.total + kSegmentTile - 1) / kSegmentTile;  // < 2^28: total < 2^40
  const int wide = (reinterpret_cast<uintptr_t>(d_out) & 15u) == 0 ? 1 : 0;
  hipLaunchKernelGGL(piece_copy_kernel, dim3((uint32_t)tiles), dim3(kThreads), 0, plan.s, b.h.d_utf8, piece_out,
                     piece_src, n_pieces, d_out, plan.total, wide);
  HIP_TRY(hipGetLastError());
  return FAC_OK;
}

}  // namespace fac
