// stage_kernels.hip — search_raw's Unicode staging on the MI355X (search.rs:296-302, 398-416):
// UAX #29 extended grapheme clusters (the reference's `unicode-segmentation`
// `grapheme_indices(true)`) and the folded first code point per grapheme (`to_lowercase`).
//
// The segmenter is the host state machine of unicode.cpp (same generated tables), run per
// 256-byte chunk: the state a boundary decision needs (left properties, regional-indicator parity,
// "ExtPict Extend*" / "... ZWJ" for GB11, the InCB conjunct state for GB9c) is fully reset after any
// code point that is not RI, ZWJ, Extend, Extended_Pictographic or InCB-classified, so each
// thread starts at the last such "resync" code point before its chunk (any letter, digit, space or
// punctuation of ordinary text) and decides every boundary inside its chunk exactly. Text with no
// resync point within 1 KiB before a chunk (long emoji / RI / combining runs) is segmented by one
// sequential device thread instead. Grapheme starts are compacted per 16 KiB unit: one wave counts
// each unit, one workgroup scans the counts, one wave writes each unit's starts in order.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>

#include <rocprim/device/device_scan.hpp>

#include "fac_internal.h"
#include "host_util.h"

namespace fac {
namespace {

struct GcbRange { uint32_t lo, hi; uint8_t prop; };
struct CpRange { uint32_t lo, hi; };
struct LowerMap { uint32_t cp; uint32_t out[3]; uint8_t n; };

#define FAC_UNICODE_QUAL __device__
#include "unicode_data.inc"
#undef FAC_UNICODE_QUAL

enum Gcb : uint8_t {
  GCB_Other = 0, GCB_CR, GCB_LF, GCB_Control, GCB_Extend, GCB_ZWJ, GCB_RI, GCB_Prepend,
  GCB_SpacingMark, GCB_L, GCB_V, GCB_T, GCB_LV, GCB_LVT
};
enum Incb : uint8_t { INCB_None = 0, INCB_Linker, INCB_Consonant, INCB_Extend };

constexpr uint32_t kLookback = 1024;   // bytes searched backwards for a resync code point

template <typename R>
__device__ const R* find_range(const R* tab, uint32_t n, uint32_t cp) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (tab[mid].hi < cp) lo = mid + 1;
    else hi = mid;
  }
  return (lo < n && tab[lo].lo <= cp && cp <= tab[lo].hi) ? &tab[lo] : nullptr;
}

struct Props {
  uint8_t g, ib;
  bool pict;
};

__device__ Props props(uint32_t cp) {  // unicode.cpp gcb / ext_pict / incb
  Props p{GCB_Other, INCB_None, false};
  if (cp < 0x80) {
    p.g = cp == '\r' ? GCB_CR : cp == '\n' ? GCB_LF : (cp < 0x20 || cp == 0x7F) ? GCB_Control : GCB_Other;
    return p;
  }
  const GcbRange* r = find_range(kGcbRanges, sizeof(kGcbRanges) / sizeof(kGcbRanges[0]), cp);
  p.g = r ? r->prop : GCB_Other;
  if (cp >= 0xA9) p.pict = find_range(kExtPictRanges, sizeof(kExtPictRanges) / sizeof(kExtPictRanges[0]), cp) != nullptr;
  if (cp >= 0x300) {
    const GcbRange* q = find_range(kIncbRanges, sizeof(kIncbRanges) / sizeof(kIncbRanges[0]), cp);
    p.ib = q ? q->prop : INCB_None;
  }
  return p;
}

__device__ uint32_t decode(const uint8_t* s, uint64_t n, uint64_t& i) {  // unicode.cpp utf8_decode
  const uint8_t b0 = s[i];
  if (b0 < 0x80) {
    i += 1;
    return b0;
  }
  if ((b0 & 0xE0) == 0xC0 && i + 1 < n) {
    const uint32_t cp = ((b0 & 0x1Fu) << 6) | (s[i + 1] & 0x3Fu);
    i += 2;
    return cp;
  }
  if ((b0 & 0xF0) == 0xE0 && i + 2 < n) {
    const uint32_t cp = ((b0 & 0x0Fu) << 12) | ((s[i + 1] & 0x3Fu) << 6) | (s[i + 2] & 0x3Fu);
    i += 3;
    return cp;
  }
  if ((b0 & 0xF8) == 0xF0 && i + 3 < n) {
    const uint32_t cp = ((b0 & 0x07u) << 18) | ((s[i + 1] & 0x3Fu) << 12) | ((s[i + 2] & 0x3Fu) << 6) | (s[i + 3] & 0x3Fu);
    i += 4;
    return cp;
  }
  i += 1;
  return 0xFFFD;
}

__device__ inline bool is_ctl(uint8_t g) { return g == GCB_Control || g == GCB_CR || g == GCB_LF; }

// a code point after which the segmenter state is the initial state of its own properties
__device__ inline bool resync(const Props& p) {
  return p.g != GCB_RI && p.g != GCB_ZWJ && p.g != GCB_Extend && !p.pict && p.ib == INCB_None;
}

struct SegState {  // unicode.cpp segment_graphemes, the text ending at the left code point
  Props L;
  uint32_t ri_run;
  bool pict, gb11;
  int incb_state;
};

__device__ SegState seg_init(const Props& L) {
  return SegState{L, L.g == GCB_RI ? 1u : 0u, L.pict, false, L.ib == INCB_Consonant ? 1 : 0};
}

// boundary before code point R (GB3-GB999), then R becomes the left code point
__device__ bool seg_step(SegState& st, const Props& R) {
  const Props& L = st.L;
  // two plain code points (GCB Other, not Extended_Pictographic, no InCB: letters, digits, spaces,
  // most punctuation) -- no rule but GB999 applies, and the state resets; most of the text
  if (L.g == GCB_Other && R.g == GCB_Other && !L.pict && !R.pict && L.ib == INCB_None && R.ib == INCB_None) {
    st = SegState{R, 0u, false, false, 0};
    return true;
  }
  bool brk;
  if (L.g == GCB_CR && R.g == GCB_LF) brk = false;                                              // GB3
  else if (is_ctl(L.g)) brk = true;                                                             // GB4
  else if (is_ctl(R.g)) brk = true;                                                             // GB5
  else if (L.g == GCB_L && (R.g == GCB_L || R.g == GCB_V || R.g == GCB_LV || R.g == GCB_LVT)) brk = false;  // GB6
  else if ((L.g == GCB_LV || L.g == GCB_V) && (R.g == GCB_V || R.g == GCB_T)) brk = false;   // GB7
  else if ((L.g == GCB_LVT || L.g == GCB_T) && R.g == GCB_T) brk = false;                    // GB8
  else if (R.g == GCB_Extend || R.g == GCB_ZWJ) brk = false;                                   // GB9
  else if (R.g == GCB_SpacingMark) brk = false;                                                // GB9a
  else if (L.g == GCB_Prepend) brk = false;                                                    // GB9b
  else if (st.incb_state == 2 && R.ib == INCB_Consonant) brk = false;                          // GB9c
  else if (st.gb11 && R.pict) brk = false;                                                     // GB11
  else if (L.g == GCB_RI && R.g == GCB_RI && (st.ri_run & 1)) brk = false;                     // GB12/13
  else brk = true;                                                                             // GB999
  st.ri_run = R.g == GCB_RI ? st.ri_run + 1 : 0;
  st.gb11 = R.g == GCB_ZWJ && st.pict;
  st.pict = R.pict ? true : (R.g == GCB_Extend ? st.pict : false);
  if (R.ib == INCB_Consonant) st.incb_state = 1;
  else if (R.ib == INCB_Linker && st.incb_state >= 1) st.incb_state = 2;
  else if (R.ib == INCB_Extend && st.incb_state >= 1) { /* unchanged */ }
  else st.incb_state = 0;
  st.L = R;
  return brk;
}

__device__ uint32_t lower_first(uint32_t cp) {  // unicode.cpp lower_full, first code point
  if (cp < 0x80) return (cp >= 'A' && cp <= 'Z') ? cp + 32 : cp;
  uint32_t lo = 0, hi = sizeof(kLowerMap) / sizeof(kLowerMap[0]);
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (kLowerMap[mid].cp < cp) lo = mid + 1;
    else hi = mid;
  }
  return (lo < sizeof(kLowerMap) / sizeof(kLowerMap[0]) && kLowerMap[lo].cp == cp) ? kLowerMap[lo].out[0] : cp;
}

// ---- BMP property / lowercase tables (built once per device from the range tables above): one
// byte per code point (GCB | Extended_Pictographic << 4 | InCB << 5) and the first code point of its
// full lowercase (0 when it lies outside the BMP: the range search decides then)
__global__ void bmp_tables_kernel(uint8_t* ptab, uint16_t* ltab) {
  const uint32_t cp = blockIdx.x * blockDim.x + threadIdx.x;
  if (cp >= 0x10000u) return;
  const Props p = props(cp);
  ptab[cp] = (uint8_t)(p.g | (p.pict ? 16u : 0u) | ((uint32_t)p.ib << 5));
  const uint32_t l = lower_first(cp);
  ltab[cp] = l < 0x10000u ? (uint16_t)l : (uint16_t)0;
}

__device__ __forceinline__ Props props_fast(const uint8_t* __restrict__ ptab, uint32_t cp) {
  if (cp < 0x80u)
    return Props{(uint8_t)(cp == '\r' ? GCB_CR : cp == '\n' ? GCB_LF : (cp < 0x20u || cp == 0x7Fu) ? GCB_Control : GCB_Other),
                 INCB_None, false};
  if (cp < 0x10000u) {
    const uint32_t v = ptab[cp];
    return Props{(uint8_t)(v & 15u), (uint8_t)(v >> 5), (v & 16u) != 0};
  }
  return props(cp);
}

__device__ __forceinline__ uint32_t fold_fast(const uint16_t* __restrict__ ltab, uint32_t cp) {
  if (cp < 0x80u) return (cp - 'A' < 26u) ? cp + 32u : cp;
  if (cp < 0x10000u) {
    const uint32_t v = ltab[cp];
    if (v) return v;
  }
  return lower_first(cp);
}

constexpr uint32_t kPropLds = 0x800;  // code points whose property / lowercase bytes the staging kernels keep in LDS
__device__ __forceinline__ Props props_of(uint32_t v) { return Props{(uint8_t)(v & 15u), (uint8_t)(v >> 5), (v & 16u) != 0}; }

// Per 16 KiB tile (one workgroup, 64 bytes per thread, the tile staged in LDS): the C ABI's UTF-8
// check (unicode.cpp utf8_valid_serial = Rust's str::from_utf8) over the code points starting in the
// thread's bytes -- a segment runs from the first byte that is not a continuation byte to the next
// thread's, so every sequence lies in one segment and stray continuation bytes are caught -- fused
// with the UAX #29 boundary decisions of those code points (seg_step from the last resync code point
// before them, usually the previous one). Boundaries go out as one 64-bit mask per thread, the
// tile's grapheme count to ucnt. A thread without a resync point within kLookback marks its bytes
// hard (seg_hard_kernel). scal: [0] flags (bit 0 invalid, bit 1 a byte >= 0x80), [1] any hard.
constexpr uint32_t kTile = 16384;
__global__ __launch_bounds__(256) void seg_tile_kernel(const uint8_t* __restrict__ s, uint64_t n, int aligned,
                                                       const uint8_t* __restrict__ ptab, unsigned long long* __restrict__ bits,
                                                       uint32_t* __restrict__ ucnt, uint8_t* __restrict__ hard,
                                                       unsigned long long* __restrict__ scal, int skip_if_ascii) {
  if (skip_if_ascii && !(scal[0] & 2ull)) return;  // ascii_or_kernel found no byte >= 0x80
  // the tile, transposed: word w of thread t's 64 bytes at word w * 256 + t, so the threads' reads
  // of their own bytes (byte j of each, together) fall in 64 different banks; the row-major tile made
  // every such read a 32-way conflict (lanes 64 bytes apart)
  __shared__ __attribute__((aligned(16))) uint32_t tileT[kTile / 4];
  __shared__ uint8_t s_pt[kPropLds];  // ptab[0, kPropLds): Latin, Greek, Cyrillic, ... in LDS
  __shared__ uint32_t red[8];
  uint8_t* const tileB = reinterpret_cast<uint8_t*>(tileT);
  auto tix = [](uint32_t q) { return ((((q >> 2) & 15u) << 8 | (q >> 6)) << 2) | (q & 3u); };  // tile byte q -> LDS byte
  const uint64_t t0 = (uint64_t)blockIdx.x * kTile, t1 = min(n, t0 + (uint64_t)kTile);
  for (uint32_t i = threadIdx.x; i < kPropLds; i += 256u) s_pt[i] = ptab[i];
  if (aligned && t1 - t0 == kTile) {
    for (uint32_t i = threadIdx.x * 16u; i < kTile; i += 256u * 16u) {
      const uint4 v = *reinterpret_cast<const uint4*>(s + t0 + i);
      const uint32_t tp = i >> 6, w0 = (i >> 2) & 15u;
      tileT[(w0 << 8) | tp] = v.x;
      tileT[((w0 + 1) << 8) | tp] = v.y;
      tileT[((w0 + 2) << 8) | tp] = v.z;
      tileT[((w0 + 3) << 8) | tp] = v.w;
    }
  } else {
    for (uint32_t i = threadIdx.x; i < kTile; i += 256u) tileB[tix(i)] = t0 + i < n ? s[t0 + i] : 0;
  }
  __syncthreads();
  auto at = [&](uint64_t p) -> uint32_t { return (p >= t0 && p < t1) ? tileB[tix((uint32_t)(p - t0))] : s[p]; };
  auto props_fast = [&](const uint8_t* tab, uint32_t cp) { return cp >= 0x80u && cp < kPropLds ? props_of(s_pt[cp]) : fac::props_fast(tab, cp); };
  auto cont = [&](uint64_t p) { return (at(p) & 0xC0u) == 0x80u; };
  auto dec = [&](uint64_t& i) -> uint32_t {  // unicode.cpp utf8_decode, bounded by n
    const uint32_t b0 = at(i);
    if (b0 < 0x80u) { i += 1; return b0; }
    if ((b0 & 0xE0u) == 0xC0u && i + 1 < n) { const uint32_t c = ((b0 & 0x1Fu) << 6) | (at(i + 1) & 0x3Fu); i += 2; return c; }
    if ((b0 & 0xF0u) == 0xE0u && i + 2 < n) {
      const uint32_t c = ((b0 & 0x0Fu) << 12) | ((at(i + 1) & 0x3Fu) << 6) | (at(i + 2) & 0x3Fu);
      i += 3;
      return c;
    }
    if ((b0 & 0xF8u) == 0xF0u && i + 3 < n) {
      const uint32_t c = ((b0 & 0x07u) << 18) | ((at(i + 1) & 0x3Fu) << 12) | ((at(i + 2) & 0x3Fu) << 6) | (at(i + 3) & 0x3Fu);
      i += 4;
      return c;
    }
    i += 1;
    return 0xFFFD;
  };
  auto seg_start = [&](uint64_t p, bool& bad) {  // first non-continuation byte at or after p
    uint32_t k = 0;
    while (p < n && cont(p) && k < 4) ++p, ++k;
    bad = p < n && cont(p);
    return p;
  };
  const uint64_t a = t0 + threadIdx.x * 64ull;
  unsigned long long mask = 0;
  bool bad = false, is_hard = false;
  uint32_t hi = 0;
  if (a < n) {
    const uint64_t b = min(a + 64, n);
#pragma unroll
    for (uint32_t w = 0; w < 16; ++w) hi |= tileT[(w << 8) | threadIdx.x];  // own bytes (0 past n)
    uint64_t i = seg_start(a, bad);
    if (a == 0 && i != 0) bad = true;
    bool bad2 = false;
    const uint64_t e = b < n ? seg_start(b, bad2) : n;
    SegState st{};
    if (!bad && i < e && i > 0) {  // the segmenter's state before the code point at i
      uint64_t q = i;
      bool found = false;
      while (q > 0 && i - q < kLookback) {
        do --q;
        while (q > 0 && cont(q));
        uint64_t t = q;
        if (resync(props_fast(ptab, dec(t)))) {
          found = true;
          break;
        }
      }
      if (!found && q > 0) {
        is_hard = true;
      } else {  // from the resync point (or the text's first code point) up to i
        uint64_t k = q;
        st = seg_init(props_fast(ptab, dec(k)));
        while (k < i) seg_step(st, props_fast(ptab, dec(k)));
      }
    }
    // the UTF-8 check covers every thread's code points, hard ones included (their boundaries are
    // decided by seg_hard_kernel, which decodes leniently and never flags a bad sequence)
    for (uint64_t k = i; !bad && k < e;) {
      const uint64_t pos = k;
      const uint32_t b0 = at(k);
      uint32_t cp;
      if (b0 < 0x80u) {
        cp = b0;
        k += 1;
      } else {
        uint32_t len, mn;
        if ((b0 & 0xE0u) == 0xC0u) len = 2, mn = 0x80;
        else if ((b0 & 0xF0u) == 0xE0u) len = 3, mn = 0x800;
        else if ((b0 & 0xF8u) == 0xF0u) len = 4, mn = 0x10000;
        else {
          bad = true;
          break;
        }
        if (k + len > e) {
          bad = true;
          break;
        }
        for (uint32_t c = 1; c < len; ++c) bad = bad || !cont(k + c);
        if (bad) break;
        cp = dec(k);
        if (cp < mn || cp > 0x10FFFFu || (cp >= 0xD800u && cp <= 0xDFFFu)) {
          bad = true;
          break;
        }
      }
      if (is_hard) continue;
      const Props R = props_fast(ptab, cp);
      bool br;
      if (pos == 0) {
        st = seg_init(R);
        br = true;
      } else {
        br = seg_step(st, R);
      }
      if (br) mask |= 1ull << (pos - a);
    }
    bits[a >> 6] = is_hard ? 0ull : mask;
    hard[a >> 6] = is_hard ? 1 : 0;
  }
  uint32_t c = (uint32_t)__popcll(mask);
  uint32_t f = (bad ? 1u : 0u) | ((hi & 0x80808080u) ? 2u : 0u) | (is_hard ? 4u : 0u);
  for (int o = 32; o > 0; o >>= 1) {
    c += __shfl_down(c, o, 64);
    f |= (uint32_t)__shfl_down((int)f, o, 64);
  }
  if ((threadIdx.x & 63u) == 0) {
    red[threadIdx.x >> 6] = c;
    red[4 + (threadIdx.x >> 6)] = f;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    ucnt[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
    const uint32_t ff = red[4] | red[5] | red[6] | red[7];
    if (ff & 3u) atomicOr(scal, (unsigned long long)(ff & 3u));
    if (ff & 4u) atomicOr(scal + 1, 1ull);
  }
}

// search.rs:196's is_ascii on the device: bit 1 of scal[0] when some byte is >= 0x80
__global__ __launch_bounds__(256) void ascii_or_kernel(const uint8_t* __restrict__ s, uint64_t n, int aligned,
                                                       unsigned long long* scal) {
  uint32_t hi = 0;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  const uint64_t nv = aligned ? n / 16 : 0;
  for (uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; v < nv; v += stride) {
    const uint4 w = reinterpret_cast<const uint4*>(s)[v];
    hi |= w.x | w.y | w.z | w.w;
  }
  for (uint64_t p = nv * 16 + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += stride) hi |= s[p];
  if (__ballot((hi & 0x80808080u) != 0) && (threadIdx.x & 63u) == 0) atomicOr(scal, 2ull);
}

// Threads without a resync code point within kLookback (long emoji / RI / combining runs): one
// thread walks each maximal run of such 64-byte ranges once, from the run's own (unbounded) resync
// point -- linear in the text overall. Then every tile is recounted.
__global__ void seg_hard_kernel(const uint8_t* s, uint64_t n, const uint8_t* ptab, const uint8_t* hard, uint64_t ranges,
                                unsigned long long* bits, const unsigned long long* scal) {
  if (blockIdx.x != 0 || threadIdx.x != 0 || !scal[1]) return;
  for (uint64_t c = 0; c < ranges; ++c) {
    if (!hard[c]) continue;
    uint64_t r = c;
    while (r + 1 < ranges && hard[r + 1]) ++r;
    const uint64_t a = c * 64, b = min((r + 1) * 64, n);
    uint64_t q = a;
    while (q > 0) {
      do --q;
      while (q > 0 && (s[q] & 0xC0) == 0x80);
      uint64_t t = q;
      if (resync(props_fast(ptab, decode(s, n, t)))) break;
    }
    uint64_t i = q;
    SegState st = seg_init(props_fast(ptab, decode(s, n, i)));
    for (uint64_t w = c; w <= r; ++w) bits[w] = 0;
    while (i < b) {
      const uint64_t pos = i;
      const bool br = seg_step(st, props_fast(ptab, decode(s, n, i)));
      if (pos >= a && br) bits[pos >> 6] |= 1ull << (pos & 63);
    }
    c = r;
  }
}
__global__ __launch_bounds__(256) void recount_kernel(const unsigned long long* bits, uint64_t ranges, uint32_t* ucnt,
                                                      uint64_t n_units, const unsigned long long* scal) {
  if (!scal[1]) return;
  const uint64_t u = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / 64;
  const uint32_t lane = threadIdx.x & 63u;
  if (u >= n_units) return;
  uint32_t c = 0;
  for (uint64_t w = u * (kTile / 64) + lane; w < min(ranges, (u + 1) * (kTile / 64)); w += 64) c += __popcll(bits[w]);
  for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o, 64);
  if (lane == 0) ucnt[u] = c;
}

__global__ __launch_bounds__(1024) void unit_scan_kernel(const uint32_t* ucnt, uint64_t* ubase, uint64_t n_units,
                                                         unsigned long long* total) {
  __shared__ unsigned long long wsum[16];
  const uint32_t t = threadIdx.x, lane = t & 63, w = t >> 6;
  const uint64_t per = (n_units + 1023) / 1024;
  const uint64_t a = min(n_units, (uint64_t)t * per), b = min(n_units, a + per);
  unsigned long long sum = 0;
  for (uint64_t i = a; i < b; ++i) sum += ucnt[i];
  unsigned long long x = sum;  // inclusive scan over the wave
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned long long y = __shfl_up(x, o, 64);
    if (lane >= (uint32_t)o) x += y;
  }
  if (lane == 63) wsum[w] = x;
  __syncthreads();
  if (t == 0) {
    unsigned long long run = 0;
    for (int i = 0; i < 16; ++i) {
      const unsigned long long v = wsum[i];
      wsum[i] = run;
      run += v;
    }
    *total = run;
  }
  __syncthreads();
  unsigned long long run = wsum[w] + x - sum;
  for (uint64_t i = a; i < b; ++i) {
    ubase[i] = run;
    run += ucnt[i];
  }
}

// Grapheme starts (h.d_off) and text_chars (h.d_text32: the folded first code point per grapheme,
// search.rs:406-412, grapheme.rs:112-119), one wave per tile in byte order: four boundary bits per
// lane per step, a wave scan gives each start its slot, so consecutive lanes write consecutive slots.
// A lane reads its 4 bytes and the next 4 as two words with its boundary word (one round trip per
// step: every code point starting in its 4 bytes decodes from those 8), and folds through an LDS copy
// of ltab below kPropLds (was: a dependent byte load per continuation byte and a global ltab load).
__global__ __launch_bounds__(256) void write_tile_kernel(const uint8_t* __restrict__ s, uint64_t n, int aligned,
                                                         const unsigned long long* __restrict__ bits,
                                                         const uint64_t* __restrict__ ubase, uint64_t n_units,
                                                         const uint16_t* __restrict__ ltab, int ci, uint64_t* __restrict__ off,
                                                         uint32_t* __restrict__ text32) {
  __shared__ uint16_t s_lt[kPropLds];
  __shared__ uint64_t s_off[4][256];  // a step's grapheme starts and chars, written out coalesced
  __shared__ uint32_t s_tx[4][256];
  if (ci)
    for (uint32_t i = threadIdx.x; i < kPropLds; i += blockDim.x) s_lt[i] = ltab[i];
  __syncthreads();
  uint64_t* const w_off = s_off[threadIdx.x / 64];
  uint32_t* const w_tx = s_tx[threadIdx.x / 64];
  const uint64_t u = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / 64;
  const uint32_t lane = threadIdx.x & 63u;
  if (u >= n_units) return;  // whole waves
  uint64_t base = ubase[u];
  const uint64_t b = u * kTile, e = min(n, b + (uint64_t)kTile);
  for (uint64_t p0 = b; p0 < e; p0 += 256) {
    const uint64_t p = p0 + 4ull * lane;
    uint32_t f = 0, wa = 0, wb = 0;
    if (p < e) {
      f = (uint32_t)(bits[p >> 6] >> (p & 63)) & 0xFu;
      if (p + 4 > e) f &= (1u << (uint32_t)(e - p)) - 1u;
      if (aligned && p + 8 <= n) {
        wa = *reinterpret_cast<const uint32_t*>(s + p);
        wb = *reinterpret_cast<const uint32_t*>(s + p + 4);
      } else {
        for (uint32_t q = 0; q < 8; ++q)
          if (p + q < n) (q < 4 ? wa : wb) |= (uint32_t)s[p + q] << (8 * (q & 3u));
      }
    }
    const uint32_t c = __popc(f);
    uint32_t x = c;
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t y = __shfl_up(x, o, 64);
      if (lane >= (uint32_t)o) x += y;
    }
    uint32_t o = x - c;  // the grapheme's slot in this step
    const uint64_t w8 = (uint64_t)wa | ((uint64_t)wb << 32);
    for (uint32_t k = 0; k < 4; ++k)
      if ((f >> k) & 1u) {
        const uint64_t i = p + k;
        auto at = [&](uint32_t d) { return (uint32_t)(w8 >> (8 * (k + d))) & 0xFFu; };  // byte i + d (d <= 3)
        const uint32_t b0 = at(0);
        uint32_t cp;  // decode(s, n, i) on the registers
        if (b0 < 0x80u) cp = b0;
        else if ((b0 & 0xE0u) == 0xC0u && i + 1 < n) cp = ((b0 & 0x1Fu) << 6) | (at(1) & 0x3Fu);
        else if ((b0 & 0xF0u) == 0xE0u && i + 2 < n) cp = ((b0 & 0x0Fu) << 12) | ((at(1) & 0x3Fu) << 6) | (at(2) & 0x3Fu);
        else if ((b0 & 0xF8u) == 0xF0u && i + 3 < n)
          cp = ((b0 & 0x07u) << 18) | ((at(1) & 0x3Fu) << 12) | ((at(2) & 0x3Fu) << 6) | (at(3) & 0x3Fu);
        else cp = 0xFFFD;
        uint32_t fc = cp;
        if (ci) fc = cp >= 0x80u && cp < kPropLds && s_lt[cp] ? (uint32_t)s_lt[cp] : fold_fast(ltab, cp);
        w_off[o] = i;
        w_tx[o] = fc;
        ++o;
      }
    const uint32_t tot = __shfl(x, 63, 64);
    __builtin_amdgcn_wave_barrier();
    for (uint32_t q = lane; q < tot; q += 64) {
      off[base + q] = w_off[q];
      text32[base + q] = w_tx[q];
    }
    __builtin_amdgcn_wave_barrier();
    base += tot;
  }
}

}  // namespace

namespace {
struct BmpTabs {
  uint8_t* p = nullptr;
  uint16_t* l = nullptr;
};
// the BMP tables of `device`, built on first use (kept for the process)
int bmp_tables(int device, hipStream_t st, BmpTabs& out, std::string& err) {
  static std::mutex mu;
  static BmpTabs tabs[64];
  if (device < 0 || device >= 64) {
    err = "device ordinal out of range";
    return FAC_E_INVALID;
  }
  std::lock_guard<std::mutex> lk(mu);
  BmpTabs& t = tabs[device];
  if (!t.p) {
    HIP_TRY(hipMalloc((void**)&t.p, 0x10000));
    HIP_TRY(hipMalloc((void**)&t.l, 0x10000 * sizeof(uint16_t)));
    hipLaunchKernelGGL(bmp_tables_kernel, dim3(256), dim3(256), 0, st, t.p, t.l);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
  }
  out = t;
  return FAC_OK;
}
}  // namespace

// Device staging of a haystack whose bytes are resident at h.d_utf8 (search.rs:196-203, 296-302):
// mode -2 checks the UTF-8 and decides is_ascii on the device, 0 stages Unicode graphemes (the caller
// checked the bytes / decided is_ascii for the whole text), 1 is an ASCII haystack (nothing to do).
// Unicode: h.n, h.d_off (grapheme byte starts + off[n] = len) and h.d_text32 (folded first code
// points); the scratch and the grapheme arrays are kept in h and reused when it is staged again.
int stage_device(const Engine& e, Haystack& h, hipStream_t st, std::string& err, int mode) {
  const uint64_t len = h.len;
  if (mode == 1 || len == 0) {
    h.ascii = mode != 0;
    h.n = h.ascii ? len : 0;
    if (!h.ascii) {
      if (h.off_cap < 1) {
        if (h.d_off) HIP_TRY(hipFree(h.d_off));
        h.d_off = nullptr;
        HIP_TRY(hipMalloc((void**)&h.d_off, 16));
        if (h.d_text32) HIP_TRY(hipFree(h.d_text32));
        h.d_text32 = nullptr;
        HIP_TRY(hipMalloc((void**)&h.d_text32, 16));
        h.off_cap = 1;
      }
      HIP_TRY(hipMemcpyAsync(h.d_off, &h.len, 8, hipMemcpyHostToDevice, st));
    }
    return FAC_OK;
  }
  BmpTabs tabs;
  if (int trc = bmp_tables(h.device, st, tabs, err)) return trc;
  const uint64_t ranges = (len + 63) / 64, n_units = (len + kTile - 1) / kTile;
  // scratch: scal[4] | bits[ranges] | ubase[n_units] | ucnt[n_units] | hard[ranges]
  const size_t need = 32 + ranges * 8 + n_units * 8 + n_units * 4 + ranges + 16;
  if (h.stage_cap < need) {
    if (h.d_stage) HIP_TRY(hipFree(h.d_stage));
    h.d_stage = nullptr;
    h.stage_cap = 0;
    HIP_TRY(hipMalloc(&h.d_stage, need));
    h.stage_cap = need;
  }
  unsigned long long* scal = static_cast<unsigned long long*>(h.d_stage);
  unsigned long long* bits = scal + 4;
  uint64_t* ubase = reinterpret_cast<uint64_t*>(bits + ranges);
  uint32_t* ucnt = reinterpret_cast<uint32_t*>(ubase + n_units);
  uint8_t* hard = reinterpret_cast<uint8_t*>(ucnt + n_units);
  const int aligned = (reinterpret_cast<uintptr_t>(h.d_utf8) & 15u) == 0 ? 1 : 0;
  HIP_TRY(hipMemsetAsync(scal, 0, 32, st));
  if (mode == -2) {
    int cus = 256;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h.device);
    const uint64_t want = (len / 16 + 255) / 256;
    hipLaunchKernelGGL(ascii_or_kernel, dim3((uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(want, (uint64_t)cus * 8))),
                       dim3(256), 0, st, h.d_utf8, len, aligned, scal);
    HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(seg_tile_kernel, dim3((uint32_t)n_units), dim3(256), 0, st, h.d_utf8, len, aligned, tabs.p, bits,
                     ucnt, hard, scal, mode == -2 ? 1 : 0);
  hipLaunchKernelGGL(seg_hard_kernel, dim3(1), dim3(64), 0, st, h.d_utf8, len, tabs.p, hard, ranges, bits, scal);
  hipLaunchKernelGGL(recount_kernel, dim3((uint32_t)((n_units + 3) / 4)), dim3(256), 0, st, bits, ranges, ucnt, n_units,
                     scal);
  hipLaunchKernelGGL(unit_scan_kernel, dim3(1), dim3(1024), 0, st, ucnt, ubase, n_units, scal + 2);
  HIP_TRY(hipGetLastError());
  unsigned long long sc[4] = {0, 0, 0, 0};
  HIP_TRY(hipMemcpyAsync(sc, scal, sizeof(sc), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (sc[0] & 1ull) {  // seg_tile_kernel checks every code point (modes -2 and 0)
    err = "haystack is not valid UTF-8";
    return FAC_E_INVALID;
  }
  if (mode == -2) {
    h.ascii = !(sc[0] & 2ull);
    if (h.ascii) {
      h.n = len;
      return FAC_OK;
    }
  }
  h.ascii = false;
  h.n = sc[2];
  if (h.n > grapheme_limit()) return FAC_E_HAYSTACK_TOO_LARGE;
  if (h.off_cap < h.n + 1) {  // grapheme starts + off[n] = len (a shard's halo end), folded first chars
    if (h.d_off) HIP_TRY(hipFree(h.d_off));
    if (h.d_text32) HIP_TRY(hipFree(h.d_text32));
    h.d_off = nullptr;
    h.d_text32 = nullptr;
    h.off_cap = 0;
    HIP_TRY(hipMalloc((void**)&h.d_off, (h.n + 1) * 8));
    HIP_TRY(hipMalloc((void**)&h.d_text32, std::max<uint64_t>(h.n * 4, 16)));
    h.off_cap = h.n + 1;
  }
  HIP_TRY(hipMemcpyAsync(h.d_off + h.n, &h.len, 8, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(write_tile_kernel, dim3((uint32_t)((n_units + 3) / 4)), dim3(256), 0, st, h.d_utf8, len, aligned, bits, ubase,
                     n_units, tabs.l, e.case_insensitive ? 1 : 0, h.d_off, h.d_text32);
  HIP_TRY(hipGetLastError());
  return FAC_OK;
}

// graphemes starting before byte `b` (a grapheme boundary) of a staged Unicode haystack: lower_bound
// over the device grapheme starts, one thread
__global__ void starts_before_kernel(const uint64_t* off, uint64_t n, uint64_t b, unsigned long long* out) {
  uint64_t lo = 0, hi = n;
  while (lo < hi) {
    const uint64_t mid = (lo + hi) >> 1;
    if (off[mid] < b) lo = mid + 1;
    else hi = mid;
  }
  *out = lo;
}

int graphemes_before(const Haystack& h, uint64_t b, hipStream_t st, uint64_t& out, std::string& err) {
  // an empty (e.g. the last, empty shard of a short text) or unstaged haystack: stage_device returned
  // before allocating d_stage, and no grapheme starts before any byte
  if (h.ascii || h.n == 0 || !h.d_stage) {
    out = std::min(b, h.n);
    return FAC_OK;
  }
  unsigned long long* d = static_cast<unsigned long long*>(h.d_stage);  // scal[3]: free after staging
  hipLaunchKernelGGL(starts_before_kernel, dim3(1), dim3(1), 0, st, h.d_off, h.n, b, d + 3);
  HIP_TRY(hipGetLastError());
  unsigned long long v = 0;
  HIP_TRY(hipMemcpyAsync(&v, d + 3, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  out = v;
  return FAC_OK;
}

// ---------------------------------------------------------------- grapheme lookup (GraphemeTable)
// The pre-filter's transcode of a Unicode haystack (prefilter.rs:262-280): the symbol id of every
// folded grapheme, looked up in the engine's table of pattern graphemes. The key of a grapheme is its
// folded code-point sequence (unicode.cpp fold_grapheme); the hash only picks the first slot, a hit
// is decided by comparing the code points.
namespace {

constexpr uint32_t kGtSlotsLds = 1024, kGtKeysLds = 512, kGtPoolLds = 2048;  // 20 KiB of LDS per workgroup

__device__ __forceinline__ uint32_t gt_hash_step(uint32_t h, uint32_t cp) { return (h ^ cp) * 16777619u; }  // FNV-1a
constexpr uint32_t kGtHashInit = 2166136261u;
__device__ __forceinline__ uint32_t gt_hash_end(uint32_t h) { return h ^ (h >> 15); }

// unicode.cpp lower_full: the full lowercase of one code point, up to 3 outputs. A BMP code point
// whose first lowercase code point is itself has no entry (an entry maps to something else first).
__device__ __forceinline__ int lower_full_dev(const uint16_t* __restrict__ ltab, uint32_t cp, uint32_t out[3]) {
  if (cp < 0x80u) {
    out[0] = (cp - 'A' < 26u) ? cp + 32u : cp;
    return 1;
  }
  if (cp < 0x10000u && ltab[cp] == cp) {
    out[0] = cp;
    return 1;
  }
  uint32_t lo = 0, hi = sizeof(kLowerMap) / sizeof(kLowerMap[0]);
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (kLowerMap[mid].cp < cp) lo = mid + 1;
    else hi = mid;
  }
  if (lo < sizeof(kLowerMap) / sizeof(kLowerMap[0]) && kLowerMap[lo].cp == cp) {
    const int k = kLowerMap[lo].n;
    for (int t = 0; t < k; ++t) out[t] = kLowerMap[lo].out[t];
    return k;
  }
  out[0] = cp;
  return 1;
}

// f(code point) -> bool for every folded code point of bytes [b, e), in order, until f returns false
template <typename F>
__device__ __forceinline__ void for_folded(const uint8_t* __restrict__ s, uint64_t b, uint64_t e,
                                           const uint16_t* __restrict__ ltab, int ci, F f) {
  uint64_t i = b;
  while (i < e) {
    const uint32_t cp = decode(s, e, i);
    if (!ci) {
      if (!f(cp)) return;
      continue;
    }
    uint32_t lo[3];
    const int k = lower_full_dev(ltab, cp, lo);
    for (int t = 0; t < k; ++t)
      if (!f(lo[t])) return;
  }
}

// One thread per key: its entry {hash, pool offset, length, id}, and the first free slot from its
// hash on takes the entry (slots = a power of two > the key count, so a free slot exists).
__global__ void grapheme_table_build_kernel(const uint32_t* __restrict__ pool, const uint2* __restrict__ keys,
                                            const uint32_t* __restrict__ ids, uint32_t n_keys, uint32_t mask,
                                            uint32_t* __restrict__ slots, uint4* __restrict__ ents) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n_keys) return;
  const uint2 key = keys[k];  // {pool offset, code points}
  uint32_t h = kGtHashInit;
  for (uint32_t i = 0; i < key.y; ++i) h = gt_hash_step(h, pool[key.x + i]);
  h = gt_hash_end(h);
  ents[k] = make_uint4(h, key.x, key.y, ids[k]);
  for (uint32_t s = h & mask, probes = 0; probes <= mask; s = (s + 1) & mask, ++probes)
    if (atomicCAS(&slots[s], 0u, k + 1) == 0u) return;
}

// The engine's table as a lookup reads it: from LDS when it fits (lds != 0: mask + 1 <= kGtSlotsLds,
// n_keys <= kGtKeysLds, n_pool <= kGtPoolLds, checked by the host), else from global memory.
struct GtView {
  const uint32_t* slots;
  const uint4* ents;
  const uint32_t* pool;
  uint32_t mask;
};
// Called by every thread of the workgroup (it synchronises when it copies).
__device__ __forceinline__ GtView gt_view(const uint32_t* __restrict__ g_slots, const uint4* __restrict__ g_ents,
                                          const uint32_t* __restrict__ g_pool, uint32_t mask, uint32_t n_keys,
                                          uint32_t n_pool, int lds) {
  __shared__ uint32_t s_slots[kGtSlotsLds];
  __shared__ uint4 s_ents[kGtKeysLds];
  __shared__ uint32_t s_pool[kGtPoolLds];
  if (!lds) return GtView{g_slots, g_ents, g_pool, mask};
  for (uint32_t i = threadIdx.x; i <= mask; i += blockDim.x) s_slots[i] = g_slots[i];
  for (uint32_t i = threadIdx.x; i < n_keys; i += blockDim.x) s_ents[i] = g_ents[i];
  for (uint32_t i = threadIdx.x; i < n_pool; i += blockDim.x) s_pool[i] = g_pool[i];
  __syncthreads();
  return GtView{s_slots, s_ents, s_pool, mask};
}

// The id of the grapheme at bytes [b, e), 0 = no pattern grapheme: the bytes are decoded and folded
// twice -- once for the hash and the length, once per probed entry of equal hash and length to
// compare its key -- so a grapheme of any length needs no buffer.
__device__ __forceinline__ uint32_t grapheme_symbol_id(const uint8_t* __restrict__ utf8, uint64_t b, uint64_t e,
                                                       const uint16_t* __restrict__ ltab, int ci, const GtView& t) {
  uint32_t h = kGtHashInit, cnt = 0;
  for_folded(utf8, b, e, ltab, ci, [&](uint32_t cp) {
    h = gt_hash_step(h, cp);
    ++cnt;
    return true;
  });
  h = gt_hash_end(h);
  for (uint32_t s = h & t.mask, probes = 0; probes <= t.mask; s = (s + 1) & t.mask, ++probes) {
    const uint32_t v = t.slots[s];
    if (v == 0u) break;
    const uint4 en = t.ents[v - 1];
    if (en.x != h || en.z != cnt) continue;
    uint32_t at = 0;
    bool same = true;
    for_folded(utf8, b, e, ltab, ci, [&](uint32_t cp) {
      same = t.pool[en.y + at] == cp;
      ++at;
      return same;
    });
    if (same) return en.w;
  }
  return 0;
}

// One thread per grapheme g of [g0, g1): bytes [off[g], off[g + 1]) (the last grapheme ends at len).
// The table is copied to LDS when it fits; the loads of off are coalesced and a wave's graphemes are
// contiguous bytes. ids[g - g0] = the id, 0 = not a key. Id = uint8_t: the pre-filter's symbols
// (<= 255, ascii_ids null); uint32_t: the grapheme dictionary of an engine with mappings
// (grapheme_ids_kernel below), where a one-byte grapheme takes its id from ascii_ids
// (Engine::ascii_gid, indexed by the byte as it stands) without a lookup.
template <typename Id>
__global__ __launch_bounds__(256) void symbol_ids_kernel(const uint8_t* __restrict__ utf8, uint64_t len,
                                                         const uint64_t* __restrict__ off, uint64_t n, uint64_t g0,
                                                         uint64_t g1, const uint16_t* __restrict__ ltab, int ci,
                                                         const uint32_t* __restrict__ g_slots, const uint4* __restrict__ g_ents,
                                                         const uint32_t* __restrict__ g_pool, uint32_t mask, uint32_t n_keys,
                                                         uint32_t n_pool, int lds, const uint32_t* __restrict__ ascii_ids,
                                                         Id* __restrict__ ids) {
  const GtView t = gt_view(g_slots, g_ents, g_pool, mask, n_keys, n_pool, lds);
  const uint64_t g = g0 + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= g1 || g >= n) return;
  const uint64_t b = off[g], e = g + 1 < n ? off[g + 1] : len;
  if (b >= e || e > len) {  // (never for a staged haystack)
    ids[g - g0] = 0;
    return;
  }
  if (ascii_ids && e - b == 1) {
    ids[g - g0] = (Id)ascii_ids[utf8[b] & 0x7Fu];
    return;
  }
  ids[g - g0] = (Id)grapheme_symbol_id(utf8, b, e, ltab, ci, t);
}
constexpr auto grapheme_ids_kernel = symbol_ids_kernel<uint32_t>;

// The same for the graphemes of a batch's non-ASCII documents (h.d_off of Batch::h: document order,
// the index space of d_text32 and of SegDesc::text_base), one thread per grapheme g of n: it begins
// at byte off[g] & kByte of document off[g] >> kDocTagShift and ends where the next grapheme begins
// if that one carries the same tag, else at its document's end doc_off[doc + 1] -- off[g + 1] then
// belongs to the next non-ASCII document, whatever lies between them, or is past the last grapheme.
__global__ __launch_bounds__(256) void batch_grapheme_ids_kernel(
    const uint8_t* __restrict__ utf8, uint64_t len, const uint64_t* __restrict__ off, uint64_t n,
    const uint64_t* __restrict__ doc_off, uint64_t n_docs, const uint16_t* __restrict__ ltab, int ci,
    const uint32_t* __restrict__ g_slots, const uint4* __restrict__ g_ents, const uint32_t* __restrict__ g_pool,
    uint32_t mask, uint32_t n_keys, uint32_t n_pool, int lds, const uint32_t* __restrict__ ascii_ids,
    uint32_t* __restrict__ ids) {
  const GtView t = gt_view(g_slots, g_ents, g_pool, mask, n_keys, n_pool, lds);
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n) return;
  constexpr uint64_t kByte = (1ull << kDocTagShift) - 1;
  const uint64_t w = off[g], b = w & kByte, doc = w >> kDocTagShift;
  uint64_t e = 0;
  if (g + 1 < n && (off[g + 1] >> kDocTagShift) == doc) e = off[g + 1] & kByte;
  else if (doc < n_docs) e = doc_off[doc + 1];
  if (b >= e || e > len) {  // (never for a staged batch)
    ids[g] = 0;
    return;
  }
  if (e - b == 1) {
    ids[g] = ascii_ids[utf8[b] & 0x7Fu];
    return;
  }
  ids[g] = grapheme_symbol_id(utf8, b, e, ltab, ci, t);
}

// The last k of [lo, hi] with prefix[k] <= p (prefix ascends strictly: the non-empty documents)
__device__ __forceinline__ uint64_t doc_of(const uint64_t* __restrict__ prefix, uint64_t lo, uint64_t hi, uint64_t p) {
  while (lo < hi) {
    const uint64_t mid = (lo + hi + 1) / 2;
    if (prefix[mid] <= p) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// The same for every symbol of a batch that holds non-ASCII documents, in the batch's start-window
// space: symbol p is local symbol i = p - prefix[k] of non-empty document k -- byte text_base + i of
// an ASCII document, grapheme text_base + i of h.d_off (tagged) of any other. A document's last
// grapheme ends at the document's end byte: off[g + 1] there belongs to the next non-ASCII document,
// or lies past the array. One thread per symbol; the tile's first and last document are bisected
// once per workgroup, a thread bisects only between them (piece_copy_kernel's idiom).
__global__ __launch_bounds__(256) void batch_symbol_ids_kernel(
    const uint8_t* __restrict__ utf8, uint64_t len, const uint64_t* __restrict__ off, const SegDesc* __restrict__ segs,
    const uint64_t* __restrict__ prefix, uint64_t n_segs, uint64_t S, const uint8_t* __restrict__ ascii_id,
    const uint16_t* __restrict__ ltab, int ci, const uint32_t* __restrict__ g_slots, const uint4* __restrict__ g_ents,
    const uint32_t* __restrict__ g_pool, uint32_t mask, uint32_t n_keys, uint32_t n_pool, int lds,
    uint8_t* __restrict__ ids) {
  __shared__ uint64_t s_doc[2];
  const uint64_t tile0 = (uint64_t)blockIdx.x * blockDim.x;
  if (tile0 >= S) return;
  if (threadIdx.x == 0) {
    const uint64_t tile_last = (S - tile0 < blockDim.x ? S : tile0 + blockDim.x) - 1;
    const uint64_t d0 = doc_of(prefix, 0, n_segs - 1, tile0);
    s_doc[0] = d0;
    s_doc[1] = doc_of(prefix, d0, n_segs - 1, tile_last);
  }
  __syncthreads();
  const GtView t = gt_view(g_slots, g_ents, g_pool, mask, n_keys, n_pool, lds);
  const uint64_t p = tile0 + threadIdx.x;
  if (p >= S) return;
  const uint64_t k = doc_of(prefix, s_doc[0], s_doc[1], p);
  const uint64_t i = p - prefix[k];
  const SegDesc* D = segs + k;
  const uint64_t base = D->text_base;
  if (D->ascii) {
    ids[p] = base + i < len ? ascii_id[utf8[base + i] & 0x7Fu] : (uint8_t)0;
    return;
  }
  constexpr uint64_t kByte = (1ull << kDocTagShift) - 1;
  const uint64_t g = base + i;
  const uint64_t b = off[g] & kByte;
  const uint64_t e = i + 1 < D->n ? off[g + 1] & kByte : (D->byte_base & kByte) + D->hay_len;
  ids[p] = (b < e && e <= len) ? (uint8_t)grapheme_symbol_id(utf8, b, e, ltab, ci, t) : (uint8_t)0;
}

// The document-start bitmap of that space: one thread per non-empty document
__global__ void batch_symbol_starts_kernel(const uint64_t* __restrict__ prefix, uint64_t n_segs, uint32_t* __restrict__ bits) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n_segs) return;
  const uint64_t p = prefix[k];
  atomicOr(bits + (p >> 5), 1u << (uint32_t)(p & 31));
}

// One workgroup per merged window w = graphemes [gs, ge) of a staged Unicode haystack: its SegDesc
// as a text of its own (api.cpp slice_view). bs = off[gs], be = off[ge] or len; the workgroup ORs the
// bytes [bs, be) (aligned 8-byte words between a byte head and tail) to decide is_ascii.
__global__ __launch_bounds__(256) void slice_desc_kernel(const uint8_t* __restrict__ utf8, uint64_t len,
                                                         const uint64_t* __restrict__ off, uint64_t n,
                                                         const uint64_t* __restrict__ spans, uint32_t n_spans,
                                                         SegDesc* __restrict__ out) {
  const uint32_t w = blockIdx.x;
  if (w >= n_spans) return;
  const uint64_t gs = spans[2 * w], ge = spans[2 * w + 1];
  const uint64_t be = ge < n ? off[ge] : len;
  const uint64_t bs = gs < n ? off[gs] : len;
  uint64_t acc = 0;
  if (bs < be && be <= len) {
    const uint8_t* p = utf8 + bs;
    const uint64_t cnt = be - bs;
    const uint64_t mis = (8u - (uint32_t)(reinterpret_cast<uintptr_t>(p) & 7u)) & 7u;
    const uint64_t head = mis < cnt ? mis : cnt;
    const uint64_t words = (cnt - head) / 8, tail = head + words * 8;
    for (uint64_t i = threadIdx.x; i < head; i += blockDim.x) acc |= p[i];
    const uint64_t* q = reinterpret_cast<const uint64_t*>(p + head);
    for (uint64_t i = threadIdx.x; i < words; i += blockDim.x) acc |= q[i];
    for (uint64_t i = tail + threadIdx.x; i < cnt; i += blockDim.x) acc |= p[i];
  }
  const int hi = __syncthreads_or((acc & 0x8080808080808080ull) != 0 ? 1 : 0);
  if (threadIdx.x != 0) return;
  const bool asc = hi == 0;
  SegDesc s{};
  s.ascii = asc ? 1u : 0u;
  s.text_base = asc ? bs : gs;
  s.n = asc ? be - bs : ge - gs;
  s.avail = s.n;
  s.hay_len = be - bs;
  s.byte_base = bs;
  s.w_begin = 0;
  s.w_end = s.n;
  out[w] = s;
}

}  // namespace

int grapheme_table_build(const std::vector<std::pair<std::u32string, uint32_t>>& keys, GraphemeTable& t, hipStream_t st,
                         std::string& err) {
  grapheme_table_free(t);
  std::vector<uint32_t> pool, ids;
  std::vector<uint2> ks;
  for (const auto& kv : keys) {
    ks.push_back(make_uint2((uint32_t)pool.size(), (uint32_t)kv.first.size()));
    ids.push_back(kv.second);
    for (char32_t c : kv.first) pool.push_back((uint32_t)c);
  }
  if (pool.size() >= (1ull << 31) || keys.size() >= (1ull << 30)) {
    err = "grapheme table too large";
    return FAC_E_UNSUPPORTED;
  }
  uint32_t slots = 16;
  while (slots < 2 * keys.size() + 1) slots *= 2;
  t.mask = slots - 1;
  t.n_keys = (uint32_t)keys.size();
  t.n_pool = (uint32_t)pool.size();
  HIP_TRY(hipMalloc((void**)&t.d_slots, (size_t)slots * 4));
  HIP_TRY(hipMalloc((void**)&t.d_ents, std::max<size_t>(keys.size() * sizeof(uint4), 16)));
  HIP_TRY(hipMalloc((void**)&t.d_pool, std::max<size_t>(pool.size() * 4, 16)));
  HIP_TRY(hipMemsetAsync(t.d_slots, 0, (size_t)slots * 4, st));
  if (keys.empty()) return FAC_OK;
  uint2* d_keys = nullptr;
  uint32_t* d_ids = nullptr;
  HIP_TRY(hipMalloc((void**)&d_keys, ks.size() * sizeof(uint2)));
  hipError_t he = hipMalloc((void**)&d_ids, ids.size() * 4);
  if (he == hipSuccess && !pool.empty()) he = hipMemcpyAsync(t.d_pool, pool.data(), pool.size() * 4, hipMemcpyHostToDevice, st);
  if (he == hipSuccess) he = hipMemcpyAsync(d_keys, ks.data(), ks.size() * sizeof(uint2), hipMemcpyHostToDevice, st);
  if (he == hipSuccess) he = hipMemcpyAsync(d_ids, ids.data(), ids.size() * 4, hipMemcpyHostToDevice, st);
  if (he == hipSuccess) {
    hipLaunchKernelGGL(grapheme_table_build_kernel, dim3((t.n_keys + 255) / 256), dim3(256), 0, st, t.d_pool, d_keys, d_ids,
                       t.n_keys, t.mask, t.d_slots, t.d_ents);
    he = hipGetLastError();
  }
  if (he == hipSuccess) he = hipStreamSynchronize(st);  // (the host vectors and the two temporaries go away)
  (void)hipFree(d_keys);
  if (d_ids) (void)hipFree(d_ids);
  HIP_TRY(he);
  return FAC_OK;
}

void grapheme_table_free(GraphemeTable& t) {
  if (t.d_slots) (void)hipFree(t.d_slots);
  if (t.d_ents) (void)hipFree(t.d_ents);
  if (t.d_pool) (void)hipFree(t.d_pool);
  t = GraphemeTable{};
}

int symbol_ids_device(const Engine& e, const Haystack& h, uint64_t g0, uint64_t g1, uint8_t* d_ids, hipStream_t st,
                      std::string& err) {
  g1 = std::min(g1, h.n);
  if (g0 >= g1) return FAC_OK;
  const GraphemeTable& t = e.sym_tab;
  if (h.ascii || !t.d_slots || !h.d_off) {
    err = "internal: symbol_ids_device needs a staged Unicode haystack and an engine with a pre-filter";
    return FAC_E_INTERNAL;
  }
  BmpTabs tabs;
  if (int trc = bmp_tables(h.device, st, tabs, err)) return trc;
  const int lds = (t.mask < kGtSlotsLds && t.n_keys <= kGtKeysLds && t.n_pool <= kGtPoolLds) ? 1 : 0;
  const uint64_t blocks = (g1 - g0 + 255) / 256;  // (h.n <= u32::MAX graphemes: the grid fits)
  hipLaunchKernelGGL(symbol_ids_kernel<uint8_t>, dim3((uint32_t)blocks), dim3(256), 0, st, h.d_utf8, h.len, h.d_off, h.n, g0,
                     g1, tabs.l, e.case_insensitive ? 1 : 0, t.d_slots, t.d_ents, t.d_pool, t.mask, t.n_keys, t.n_pool, lds,
                     (const uint32_t*)nullptr, d_ids);
  HIP_TRY(hipGetLastError());
  return FAC_OK;
}

int grapheme_ids_device(const Engine& e, const Haystack& h, uint32_t* d_ids, hipStream_t st, std::string& err) {
  if (h.n == 0) return FAC_OK;
  const GraphemeTable& t = e.gid_tab;
  if (h.ascii || !t.d_slots || !e.d_ascii_gid || !h.d_off || !d_ids) {
    err = "internal: grapheme_ids_device needs staged Unicode text and an engine with mappings";
    return FAC_E_INTERNAL;
  }
  const uint64_t blocks = (h.n + 255) / 256;
  if (blocks > 0x7FFFFFFFull) {
    err = "a batch's non-ASCII documents hold fewer than 2^39 graphemes";
    return FAC_E_UNSUPPORTED;
  }
  BmpTabs tabs;
  if (int trc = bmp_tables(h.device, st, tabs, err)) return trc;
  const int lds = (t.mask < kGtSlotsLds && t.n_keys <= kGtKeysLds && t.n_pool <= kGtPoolLds) ? 1 : 0;
  const int ci = e.case_insensitive ? 1 : 0;
  if (h.d_doc_off)
    hipLaunchKernelGGL(batch_grapheme_ids_kernel, dim3((uint32_t)blocks), dim3(256), 0, st, h.d_utf8, h.len, h.d_off, h.n,
                       h.d_doc_off, h.n_docs, tabs.l, ci, t.d_slots, t.d_ents, t.d_pool, t.mask, t.n_keys, t.n_pool, lds,
                       e.d_ascii_gid, d_ids);
  else
    hipLaunchKernelGGL(grapheme_ids_kernel, dim3((uint32_t)blocks), dim3(256), 0, st, h.d_utf8, h.len, h.d_off, h.n,
                       (uint64_t)0, h.n, tabs.l, ci, t.d_slots, t.d_ents, t.d_pool, t.mask, t.n_keys, t.n_pool, lds,
                       e.d_ascii_gid, d_ids);
  HIP_TRY(hipGetLastError());
  return FAC_OK;
}

int batch_symbol_ids_device(const Engine& e, const Batch& b, uint8_t* d_ids, hipStream_t st, std::string& err) {
  const Haystack& h = b.h;
  const uint64_t S = b.windows;
  if (S == 0 || b.n_segs == 0) return FAC_OK;
  const GraphemeTable& t = e.sym_tab;
  if (h.ascii || !t.d_slots || !h.d_off || !b.d_segs || !b.d_prefix) {
    err = "internal: batch_symbol_ids_device needs a staged batch with non-ASCII documents and an engine with a pre-filter";
    return FAC_E_INTERNAL;
  }
  const uint64_t blocks = (S + 255) / 256;
  if (blocks > 0x7FFFFFFFull) {
    err = "a pre-filtered batch with non-ASCII documents holds fewer than 2^39 symbols";
    return FAC_E_UNSUPPORTED;
  }
  BmpTabs tabs;
  if (int trc = bmp_tables(h.device, st, tabs, err)) return trc;
  const int lds = (t.mask < kGtSlotsLds && t.n_keys <= kGtKeysLds && t.n_pool <= kGtPoolLds) ? 1 : 0;
  hipLaunchKernelGGL(batch_symbol_ids_kernel, dim3((uint32_t)blocks), dim3(256), 0, st, h.d_utf8, h.len, h.d_off, b.d_segs,
                     b.d_prefix, b.n_segs, S, e.d_ascii_id, tabs.l, e.case_insensitive ? 1 : 0, t.d_slots, t.d_ents, t.d_pool,
                     t.mask, t.n_keys, t.n_pool, lds, d_ids);
  HIP_TRY(hipGetLastError());
  return FAC_OK;
}

int batch_symbol_starts_device(const Batch& b, uint32_t* d_bits, hipStream_t st, std::string& err) {
  if (b.n_segs == 0) return FAC_OK;
  hipLaunchKernelGGL(batch_symbol_starts_kernel, dim3((uint32_t)((b.n_segs + 255) / 256)), dim3(256), 0, st, b.d_prefix,
                     b.n_segs, d_bits);
  HIP_TRY(hipGetLastError());
  return FAC_OK;
}

int slice_descs_device(const Haystack& h, const std::vector<std::pair<uint64_t, uint64_t>>& spans, hipStream_t st,
                       std::vector<SegDesc>& out, std::string& err) {
  out.assign(spans.size(), SegDesc{});
  if (spans.empty()) return FAC_OK;
  if (h.ascii || !h.d_off || spans.size() >= (1ull << 31)) {
    err = "internal: slice_descs_device needs a staged Unicode haystack";
    return FAC_E_INTERNAL;
  }
  std::vector<uint64_t> flat(2 * spans.size());
  for (size_t i = 0; i < spans.size(); ++i) {
    flat[2 * i + 1] = std::min(spans[i].second, h.n);
    flat[2 * i] = std::min(spans[i].first, flat[2 * i + 1]);
  }
  hipError_t he = hipSuccess;
  const size_t in_b = flat.size() * 8, out_b = spans.size() * sizeof(SegDesc);
  uint8_t* mem = static_cast<uint8_t*>(call_scratch_take(in_b + out_b, st, &he));
  HIP_TRY(he);
  uint64_t* d_spans = reinterpret_cast<uint64_t*>(mem);
  SegDesc* d_out = reinterpret_cast<SegDesc*>(mem + in_b);  // (in_b is a multiple of 16)
  he = hipMemcpyAsync(d_spans, flat.data(), in_b, hipMemcpyHostToDevice, st);
  if (he == hipSuccess) {
    hipLaunchKernelGGL(slice_desc_kernel, dim3((uint32_t)spans.size()), dim3(256), 0, st, h.d_utf8, h.len, h.d_off, h.n,
                       d_spans, (uint32_t)spans.size(), d_out);
    he = hipGetLastError();
  }
  if (he == hipSuccess) he = hipMemcpyAsync(out.data(), d_out, out_b, hipMemcpyDeviceToHost, st);
  if (he == hipSuccess) he = hipStreamSynchronize(st);
  else (void)hipStreamSynchronize(st);  // (the upload may be in flight: flat goes away)
  call_scratch_give(mem, st);
  HIP_TRY(he);
  return FAC_OK;
}

// ---------------------------------------------------------------- batch staging (fac_batch_*)
// Every document of a batch is staged as if it were staged alone: the UTF-8 check and is_ascii
// (search.rs:196) per document, UAX #29 segmentation of the non-ASCII documents from start-of-text
// at each document's first byte, and one SegDesc per non-empty document, all on the device.
// scal: [0] bit 0 bad offsets, bit 1 some document is not ASCII; [1] first invalid document,
// [2] first document over the grapheme limit (both ~0: none).
namespace {

__global__ void batch_offsets_kernel(const uint64_t* __restrict__ off, uint64_t n_docs, uint64_t total,
                                     unsigned long long* __restrict__ scal) {
  const uint64_t d = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (d > n_docs) return;
  bool bad = false;
  if (d == 0) bad = off[0] != 0;
  if (d == n_docs) bad = bad || off[d] != total;
  else bad = bad || off[d] > off[d + 1] || off[d + 1] > total;
  if (bad) atomicOr(scal, 1ull);
}

// One wave per document: str::from_utf8 and str::is_ascii of its bytes alone. Each lane checks the
// bytes it reads: a lead byte's whole sequence (inside the document, continuation bytes, shortest
// form, no surrogate, <= U+10FFFF), a continuation byte that a lead byte at most three bytes before
// it, inside the document, covers it.
__global__ __launch_bounds__(256) void batch_doc_scan_kernel(const uint8_t* __restrict__ s, const uint64_t* __restrict__ off,
                                                             uint64_t n_docs, uint32_t* __restrict__ flags,
                                                             unsigned long long* __restrict__ scal) {
  const uint64_t d = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / 64;
  const uint32_t lane = threadIdx.x & 63u;
  if (d >= n_docs) return;  // whole waves
  const uint64_t a = off[d], b = off[d + 1];
  auto lead_len = [](uint32_t c) -> uint32_t {
    return (c & 0xE0u) == 0xC0u ? 2u : (c & 0xF0u) == 0xE0u ? 3u : (c & 0xF8u) == 0xF0u ? 4u : 0u;
  };
  bool hi = false, bad = false;
  for (uint64_t p = a + lane; p < b; p += 64) {
    const uint32_t c = s[p];
    if (c < 0x80u) continue;
    hi = true;
    if ((c & 0xC0u) == 0x80u) {
      uint32_t k = 1;
      while (k <= 3 && p >= a + k && (s[p - k] & 0xC0u) == 0x80u) ++k;
      if (k > 3 || p < a + k || lead_len(s[p - k]) <= k) bad = true;
      continue;
    }
    const uint32_t len = lead_len(c);
    if (len == 0 || p + len > b) {
      bad = true;
      continue;
    }
    uint32_t cp = len == 2 ? (c & 0x1Fu) : len == 3 ? (c & 0x0Fu) : (c & 0x07u);
    for (uint32_t k = 1; k < len; ++k) {
      const uint32_t x = s[p + k];
      if ((x & 0xC0u) != 0x80u) bad = true;
      cp = (cp << 6) | (x & 0x3Fu);
    }
    const uint32_t mn = len == 2 ? 0x80u : len == 3 ? 0x800u : 0x10000u;
    if (cp < mn || cp > 0x10FFFFu || (cp >= 0xD800u && cp <= 0xDFFFu)) bad = true;
  }
  const bool any_hi = __ballot(hi) != 0, any_bad = __ballot(bad) != 0;
  if (lane == 0) {
    flags[d] = (any_bad ? 1u : 0u) | (any_hi ? 2u : 0u);
    if (any_hi) atomicOr(scal, 2ull);
    if (any_bad) atomicMin(scal + 1, (unsigned long long)d);
  }
}

// One thread per non-ASCII document: unicode.cpp segment_graphemes over its bytes, the segmenter
// starting from start-of-text at the document's first code point (so no left context crosses a
// document boundary, whatever the run: regional indicators pair from the document's start, GB9/GB11/
// GB9c see nothing before it). WRITE = false counts the graphemes (tri_in[d].u); WRITE = true writes
// their tagged byte starts and folded first code points from the document's scanned base.
template <bool WRITE>
__global__ __launch_bounds__(64) void batch_seg_kernel(const uint8_t* __restrict__ s, const uint64_t* __restrict__ off,
                                                       uint64_t n_docs, const uint32_t* __restrict__ flags,
                                                       const uint8_t* __restrict__ ptab, const uint16_t* __restrict__ ltab,
                                                       int ci, BatchTri* __restrict__ tri_in,
                                                       const BatchTri* __restrict__ tri_ex, uint64_t* __restrict__ goff,
                                                       uint32_t* __restrict__ text32) {
  const uint64_t d = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= n_docs) return;
  const uint32_t f = flags[d];
  if (!(f & 2u) || (f & 1u)) {
    if (!WRITE) tri_in[d].u = 0;
    return;
  }
  const uint64_t a = off[d], b = off[d + 1];
  const uint64_t tag = d << kDocTagShift;
  uint64_t i = a, cnt = 0;
  uint64_t base = 0;
  if (WRITE) base = tri_ex[d].u;
  SegState st{};
  while (i < b) {
    const uint64_t pos = i;
    const uint32_t cp = decode(s, b, i);
    const Props R = props_fast(ptab, cp);
    bool br;
    if (pos == a) {
      st = seg_init(R);
      br = true;
    } else {
      br = seg_step(st, R);
    }
    if (br) {
      if (WRITE) {
        goff[base + cnt] = pos | tag;
        text32[base + cnt] = ci ? fold_fast(ltab, cp) : cp;
      }
      ++cnt;
    }
  }
  if (!WRITE) tri_in[d].u = cnt;
}

// last document d in [lo, hi] with off[d] <= x (off[lo] <= x holds)
__device__ inline uint64_t window_of(const uint64_t* __restrict__ off, uint64_t lo, uint64_t hi, uint64_t x) {
  while (lo < hi) {
    const uint64_t mid = (lo + hi + 1) >> 1;
    if (off[mid] <= x) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// The same segmentation for long documents (Batch::long_docs: a stream task's 256 KiB windows, where
// one thread per document walks for milliseconds): one thread per kSegChunk bytes of the batch's
// text, whatever documents they belong to. A thread decides the boundaries of the code points that
// start in its bytes; the segmenter's state before the first of them comes from the nearest resync
// code point before it, or from the document's first code point, whichever is nearer (so a long
// combining, emoji or regional-indicator run costs its threads a walk back to the run's start, at
// worst the one-thread-per-document walk). ASCII and invalid documents are stepped over, as there.
// WRITE = false: the chunk's grapheme count to ccnt[chunk], and added to tri_in[d].u (zeroed by the
// caller) for every document it touches. WRITE = true: cbase = the exclusive sums of ccnt; documents
// lie in the text in order, so that is the chunk's first slot in goff / text32.
constexpr uint32_t kSegChunk = 256;
template <bool WRITE>
__global__ __launch_bounds__(256) void batch_seg_chunk_kernel(const uint8_t* __restrict__ s, uint64_t total,
                                                              const uint64_t* __restrict__ off, uint64_t n_docs,
                                                              const uint32_t* __restrict__ flags,
                                                              const uint8_t* __restrict__ ptab, const uint16_t* __restrict__ ltab,
                                                              int ci, BatchTri* __restrict__ tri_in, uint64_t* __restrict__ ccnt,
                                                              const uint64_t* __restrict__ cbase, uint64_t* __restrict__ goff,
                                                              uint32_t* __restrict__ text32) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t c0 = k * kSegChunk;
  if (c0 >= total) return;
  const uint64_t c1 = total - c0 < kSegChunk ? total : c0 + kSegChunk;
  uint64_t d = window_of(off, 0, n_docs - 1, c0);  // (off[0] = 0, off[n_docs] = total: checked before)
  uint64_t cnt = 0;
  uint64_t base = 0;
  if (WRITE) base = cbase[k];
  uint64_t i = c0;
  while (i < c1) {
    while (i >= off[d + 1]) ++d;  // (i < total = off[n_docs]: d stays below n_docs)
    const uint64_t a = off[d], b = off[d + 1];
    const uint64_t e = b < c1 ? b : c1;
    const uint32_t f = flags[d];
    if (!(f & 2u) || (f & 1u)) {
      i = e;
      continue;
    }
    // the first code point that starts in [i, e): the bytes before it belong to the chunk before
    uint64_t p = i;
    while (p < e && p > a && (s[p] & 0xC0u) == 0x80u) ++p;
    SegState st{};
    if (p < e && p > a) {  // the state before p
      uint64_t q = p;
      for (;;) {
        do --q;
        while (q > a && (s[q] & 0xC0u) == 0x80u);
        if (q == a) break;
        uint64_t t = q;
        if (resync(props_fast(ptab, decode(s, b, t)))) break;
      }
      st = seg_init(props_fast(ptab, decode(s, b, q)));
      while (q < p) seg_step(st, props_fast(ptab, decode(s, b, q)));
    }
    const uint64_t tag = d << kDocTagShift;
    uint64_t here = 0;
    while (p < e) {
      const uint64_t pos = p;
      const uint32_t cp = decode(s, b, p);
      const Props R = props_fast(ptab, cp);
      bool br;
      if (pos == a) {
        st = seg_init(R);
        br = true;
      } else {
        br = seg_step(st, R);
      }
      if (br) {
        if (WRITE) {
          goff[base + cnt] = pos | tag;
          text32[base + cnt] = ci ? fold_fast(ltab, cp) : cp;
        }
        ++cnt;
        ++here;
      }
    }
    if (!WRITE && here) atomicAdd(reinterpret_cast<unsigned long long*>(&tri_in[d].u), (unsigned long long)here);
    i = e;  // (a code point may run past c1: the next chunk skips its continuation bytes)
  }
  if (!WRITE) ccnt[k] = cnt;
}

// windows and the "not empty" flag per document (an ASCII document's graphemes are its bytes); the
// first document over the grapheme limit
__global__ void batch_tri_kernel(const uint64_t* __restrict__ off, uint64_t n_docs, const uint32_t* __restrict__ flags,
                                 BatchTri* __restrict__ tri_in, uint64_t limit, unsigned long long* __restrict__ scal) {
  const uint64_t d = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (d > n_docs) return;
  if (d == n_docs) {
    tri_in[d] = BatchTri{0, 0, 0};
    return;
  }
  const uint64_t n = (flags[d] & 2u) ? tri_in[d].u : off[d + 1] - off[d];
  if (!(flags[d] & 2u)) tri_in[d].u = 0;
  tri_in[d].w = n;
  tri_in[d].s = n ? 1u : 0u;
  if (n > limit) atomicMin(scal + 2, (unsigned long long)d);
}

struct TriPlus {
  __host__ __device__ BatchTri operator()(const BatchTri& a, const BatchTri& b) const {
    return BatchTri{a.u + b.u, a.w + b.w, a.s + b.s};
  }
};

// One thread per document: the SegDesc of a non-empty document at its slot among the non-empty
// ones, its window prefix, and (thread 0) the closing prefix entry.
__global__ void batch_desc_kernel(const uint64_t* __restrict__ off, uint64_t n_docs, const uint32_t* __restrict__ flags,
                                  const BatchTri* __restrict__ tri_in, const BatchTri* __restrict__ tri_ex,
                                  SegDesc* __restrict__ segs, uint64_t* __restrict__ prefix) {
  const uint64_t d = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= n_docs) return;
  if (d == 0) prefix[tri_ex[n_docs].s] = tri_ex[n_docs].w;
  const uint64_t n = tri_in[d].w;
  if (n == 0) return;
  const bool ascii = !(flags[d] & 2u);
  SegDesc S;
  S.text_base = ascii ? off[d] : tri_ex[d].u;
  S.n = n;
  S.avail = n;
  S.hay_len = off[d + 1] - off[d];
  S.byte_base = off[d] | (d << kDocTagShift);
  S.w_begin = 0;
  S.w_end = n;
  S.ascii = ascii ? 1u : 0u;
  S.pad = 0;
  const uint64_t k = tri_ex[d].s;
  segs[k] = S;
  prefix[k] = tri_ex[d].w;
}

}  // namespace

int exclusive_sum_u64(const uint64_t* d_in, uint64_t* d_out, uint64_t n, hipStream_t st, std::string& err) {
  size_t bytes = 0;
  HIP_TRY(rocprim::exclusive_scan(nullptr, bytes, d_in, d_out, uint64_t(0), n, rocprim::plus<uint64_t>(), st));
  hipError_t he = hipSuccess;
  void* tmp = call_scratch_take(std::max<size_t>(bytes, 16), st, &he);
  HIP_TRY(he);
  he = rocprim::exclusive_scan(tmp, bytes, d_in, d_out, uint64_t(0), n, rocprim::plus<uint64_t>(), st);
  call_scratch_give(tmp, st);
  HIP_TRY(he);
  return FAC_OK;
}

void free_batch(Batch& b) {
  (void)hipSetDevice(b.h.device);
  if (b.d_dstart) (void)hipFree(b.d_dstart);
  b.d_dstart = nullptr;
  b.dstart_cap = 0;
  b.dstart_ready = false;
  if (b.d_sstart) (void)hipFree(b.d_sstart);
  b.d_sstart = nullptr;
  b.sstart_cap = 0;
  b.sstart_ready = false;
  if (b.own_offsets && b.d_offsets) (void)hipFree(b.d_offsets);
  b.d_offsets = nullptr;
  if (b.d_meta) (void)hipFree(b.d_meta);
  b.d_meta = nullptr;
  if (b.d_segs) (void)hipFree(b.d_segs);
  if (b.d_prefix) (void)hipFree(b.d_prefix);
  b.d_segs = nullptr;
  b.d_prefix = nullptr;
  free_haystack(b.h);
}

int stage_batch_device(const Engine& e, Batch& b, hipStream_t st, std::string& err) {
  Haystack& h = b.h;
  const uint64_t nd = b.n_docs, len = h.len;
  b.n_segs = 0;
  b.windows = 0;
  b.err_doc = b.err_graphemes = 0;
  b.dstart_ready = false;  // the pre-filter's document-start bitmaps are rebuilt for the new offsets
  b.sstart_ready = false;
  h.ascii = true;
  h.n = 0;
  {
    std::lock_guard<std::mutex> lk(h.host_mu);
    h.host_ready = false;
    h.utf8.clear();
    h.starts.clear();
  }
  {  // the grapheme ids of the text staged before are stale (the array is kept: ensure_gids)
    std::lock_guard<std::mutex> lk(h.gid_mu);
    h.gid_engine = nullptr;
  }
  h.d_doc_off = nullptr;
  h.n_docs = 0;
  if (nd == 0) return FAC_OK;
  // flags | tri_in | tri_ex | scal
  const size_t tri_b = (nd + 1) * sizeof(BatchTri), flag_b = (nd * 4 + 15) & ~size_t(15);
  const size_t need = flag_b + 2 * tri_b + 64;
  if (b.meta_cap < need) {
    if (b.d_meta) HIP_TRY(hipFree(b.d_meta));
    b.d_meta = nullptr;
    b.meta_cap = 0;
    HIP_TRY(hipMalloc(&b.d_meta, need));
    b.meta_cap = need;
  }
  uint8_t* m = static_cast<uint8_t*>(b.d_meta);
  b.d_flags = reinterpret_cast<uint32_t*>(m);
  b.d_tri_in = reinterpret_cast<BatchTri*>(m + flag_b);
  b.d_tri_ex = reinterpret_cast<BatchTri*>(m + flag_b + tri_b);
  b.d_scal = reinterpret_cast<unsigned long long*>(m + flag_b + 2 * tri_b);
  const unsigned long long scal0[4] = {0ull, ~0ull, ~0ull, 0ull};
  HIP_TRY(hipMemcpyAsync(b.d_scal, scal0, sizeof(scal0), hipMemcpyHostToDevice, st));
  const uint32_t T = 256;
  const uint32_t G1 = (uint32_t)((nd + 1 + T - 1) / T);
  // the offsets are checked before anything is read through them
  hipLaunchKernelGGL(batch_offsets_kernel, dim3(G1), dim3(T), 0, st, b.d_offsets, nd, len, b.d_scal);
  HIP_TRY(hipGetLastError());
  unsigned long long sc[4] = {0, 0, 0, 0};
  HIP_TRY(hipMemcpyAsync(sc, b.d_scal, sizeof(sc), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (sc[0] & 1ull) {
    err = "batch offsets must start at 0, not decrease, and end at the byte count";
    b.err_doc = ~0ull;
    return FAC_E_INVALID;
  }
  BmpTabs tabs;
  if (int trc = bmp_tables(h.device, st, tabs, err)) return trc;
  hipLaunchKernelGGL(batch_doc_scan_kernel, dim3((uint32_t)((nd + 3) / 4)), dim3(T), 0, st, h.d_utf8, b.d_offsets, nd,
                     b.d_flags, b.d_scal);
  // long documents are segmented by chunks of the text: per chunk its count and its first slot
  const uint64_t n_chunks = b.long_docs ? (len + kSegChunk - 1) / kSegChunk : 0;
  struct Chunks {
    uint64_t* p = nullptr;
    hipStream_t st;
    ~Chunks() {
      if (p) call_scratch_give(p, st);
    }
  } chunks;
  chunks.st = st;
  if (n_chunks) {
    hipError_t he = hipSuccess;
    chunks.p = static_cast<uint64_t*>(call_scratch_take(2 * n_chunks * 8, st, &he));
    if (he != hipSuccess) chunks.p = nullptr;
    HIP_TRY(he);
    HIP_TRY(hipMemsetAsync(b.d_tri_in, 0, tri_b, st));
    hipLaunchKernelGGL(batch_seg_chunk_kernel<false>, dim3((uint32_t)((n_chunks + T - 1) / T)), dim3(T), 0, st, h.d_utf8, len,
                       b.d_offsets, nd, b.d_flags, tabs.p, tabs.l, e.case_insensitive ? 1 : 0, b.d_tri_in, chunks.p,
                       (const uint64_t*)nullptr, (uint64_t*)nullptr, (uint32_t*)nullptr);
    HIP_TRY(hipGetLastError());
    if (int rc = exclusive_sum_u64(chunks.p, chunks.p + n_chunks, n_chunks, st, err)) return rc;
  } else {
    // (every thread returns at once in an all-ASCII batch: no segmentation work)
    hipLaunchKernelGGL(batch_seg_kernel<false>, dim3((uint32_t)((nd + 63) / 64)), dim3(64), 0, st, h.d_utf8, b.d_offsets, nd,
                       b.d_flags, tabs.p, tabs.l, e.case_insensitive ? 1 : 0, b.d_tri_in, b.d_tri_ex, (uint64_t*)nullptr,
                       (uint32_t*)nullptr);
  }
  hipLaunchKernelGGL(batch_tri_kernel, dim3(G1), dim3(T), 0, st, b.d_offsets, nd, b.d_flags, b.d_tri_in, grapheme_limit(),
                     b.d_scal);
  HIP_TRY(hipGetLastError());
  {
    size_t bytes = 0;
    HIP_TRY(rocprim::exclusive_scan(nullptr, bytes, b.d_tri_in, b.d_tri_ex, BatchTri{0, 0, 0}, nd + 1, TriPlus{}, st));
    hipError_t he = hipSuccess;
    void* tmp = call_scratch_take(std::max<size_t>(bytes, 16), st, &he);
    HIP_TRY(he);
    he = rocprim::exclusive_scan(tmp, bytes, b.d_tri_in, b.d_tri_ex, BatchTri{0, 0, 0}, nd + 1, TriPlus{}, st);
    call_scratch_give(tmp, st);
    HIP_TRY(he);
  }
  BatchTri tot{0, 0, 0};
  HIP_TRY(hipMemcpyAsync(sc, b.d_scal, sizeof(sc), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(&tot, b.d_tri_ex + nd, sizeof(tot), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  // search_raw applied to the documents in order: the first document that fails decides the error
  // (an invalid document has no grapheme count, so only the valid ones can be too large)
  if (sc[1] != ~0ull || sc[2] != ~0ull) {
    if (sc[1] < sc[2]) {
      b.err_doc = sc[1];
      err = "a document of the batch is not valid UTF-8";
      return FAC_E_INVALID;
    }
    b.err_doc = sc[2];
    BatchTri t{0, 0, 0};
    HIP_TRY(hipMemcpyAsync(&t, b.d_tri_in + sc[2], sizeof(t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    b.err_graphemes = t.w;
    return FAC_E_HAYSTACK_TOO_LARGE;
  }
  h.ascii = !(sc[0] & 2ull);
  h.n = tot.u;
  h.d_doc_off = b.d_offsets;
  h.n_docs = nd;
  if (!h.ascii) {
    if (h.off_cap < h.n + 1) {
      if (h.d_off) HIP_TRY(hipFree(h.d_off));
      if (h.d_text32) HIP_TRY(hipFree(h.d_text32));
      h.d_off = nullptr;
      h.d_text32 = nullptr;
      h.off_cap = 0;
      HIP_TRY(hipMalloc((void**)&h.d_off, (h.n + 1) * 8));
      HIP_TRY(hipMalloc((void**)&h.d_text32, std::max<uint64_t>(h.n * 4, 16)));
      h.off_cap = h.n + 1;
    }
    if (n_chunks)
      hipLaunchKernelGGL(batch_seg_chunk_kernel<true>, dim3((uint32_t)((n_chunks + T - 1) / T)), dim3(T), 0, st, h.d_utf8, len,
                         b.d_offsets, nd, b.d_flags, tabs.p, tabs.l, e.case_insensitive ? 1 : 0, b.d_tri_in, (uint64_t*)nullptr,
                         chunks.p + n_chunks, h.d_off, h.d_text32);
    else
      hipLaunchKernelGGL(batch_seg_kernel<true>, dim3((uint32_t)((nd + 63) / 64)), dim3(64), 0, st, h.d_utf8, b.d_offsets, nd,
                         b.d_flags, tabs.p, tabs.l, e.case_insensitive ? 1 : 0, b.d_tri_in, b.d_tri_ex, h.d_off, h.d_text32);
  }
  if (b.seg_cap < tot.s + 1) {
    if (b.d_segs) HIP_TRY(hipFree(b.d_segs));
    if (b.d_prefix) HIP_TRY(hipFree(b.d_prefix));
    b.d_segs = nullptr;
    b.d_prefix = nullptr;
    b.seg_cap = 0;
    HIP_TRY(hipMalloc((void**)&b.d_segs, (tot.s + 1) * sizeof(SegDesc)));
    HIP_TRY(hipMalloc((void**)&b.d_prefix, (tot.s + 1) * 8));
    b.seg_cap = tot.s + 1;
  }
  hipLaunchKernelGGL(batch_desc_kernel, dim3((uint32_t)((nd + T - 1) / T)), dim3(T), 0, st, b.d_offsets, nd, b.d_flags,
                     b.d_tri_in, b.d_tri_ex, b.d_segs, b.d_prefix);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(st));
  b.n_segs = tot.s;
  b.windows = tot.w;
  return FAC_OK;
}

// ---------------------------------------------------------------- stream tasks as window documents
// The expanded text of a stream task (stream.cpp): consecutive windows overlap (the next one starts
// at this one's commit point) and a batch's documents are disjoint, so every window's bytes, overlap
// included, are copied one after the other into a second buffer. An output-stationary byte mover in
// piece_copy_kernel's idiom: a workgroup owns a tile of kGatherTile output bytes, thread 0 bisects the
// tile's first and last window once, a lane bisects only between them and moves its 16 bytes. Where
// they come from one window: one 16-byte load if the source is 16-byte aligned like the destination,
// else aligned words shifted into place (chunk_load16) if those words lie inside the text; bytes in
// every other case (a lane across a window boundary, the text's last bytes, the output's tail).
// Reads stay inside [0, text_len), writes inside [0, total).
namespace {

constexpr uint32_t kGatherTile = 4096, kGatherThreads = kGatherTile / 16;

// doc_off has n_windows + 1 entries (the last one = total), n_windows >= 1, total >= 1.
__global__ __launch_bounds__(kGatherThreads) void stream_gather_kernel(const uint8_t* __restrict__ text, uint64_t text_len,
                                                                       const uint64_t* __restrict__ src,
                                                                       const uint64_t* __restrict__ doc_off,
                                                                       uint64_t n_windows, uint8_t* __restrict__ out,
                                                                       uint64_t total, int wide) {
  __shared__ uint64_t s_win[2];
  const uint64_t tile0 = (uint64_t)blockIdx.x * kGatherTile;
  if (tile0 >= total) return;
  if (threadIdx.x == 0) {
    const uint64_t tile_last = (total - tile0 < kGatherTile ? total : tile0 + kGatherTile) - 1;
    const uint64_t w0 = window_of(doc_off, 0, n_windows - 1, tile0);
    s_win[0] = w0;
    s_win[1] = window_of(doc_off, w0, n_windows - 1, tile_last);
  }
  __syncthreads();
  const uint64_t g = tile0 + (uint64_t)threadIdx.x * 16;
  if (g >= total) return;
  const uint32_t n = total - g < 16 ? (uint32_t)(total - g) : 16u;
  // the lane's first byte lies in window w (the last one that starts at or before it, so not empty)
  uint64_t w = window_of(doc_off, s_win[0], s_win[1], g);
  uint64_t lo = doc_off[w], hi = doc_off[w + 1];
  Chunk16 c;
  if (n == 16 && g + 16 <= hi) {  // one window's bytes
    const uint64_t sp = src[w] + (g - lo);
    const uint32_t a16 = (uint32_t)(reinterpret_cast<uintptr_t>(text + sp) & 15u), a4 = a16 & 3u;
    if (a16 == 0 && wide && sp + 16 <= text_len) {
      *reinterpret_cast<uint4*>(out + g) = *reinterpret_cast<const uint4*>(text + sp);
      return;
    }
    if (sp >= a4 && sp - a4 + (a4 ? 20u : 16u) <= text_len) chunk_load16(c, text + sp);
  }
  if (c.filled == 0) {
    for (uint32_t t = 0; t < n; ++t) {
      const uint64_t pos = g + t;
      while (pos >= hi) {  // (pos < total = doc_off[n_windows]: w stays below n_windows)
        ++w;
        lo = hi;
        hi = doc_off[w + 1];
      }
      const uint64_t sp = src[w] + (pos - lo);
      chunk_put(c, sp < text_len ? (uint64_t)text[sp] : 0ull);
    }
  }
  chunk_store(c, out + g, wide);
}

}  // namespace

int stream_gather_device(const uint8_t* d_text, uint64_t text_len, const uint64_t* d_src, const uint64_t* d_len,
                         uint64_t n_windows, uint64_t total, uint8_t* d_out, uint64_t* d_offsets, hipStream_t st,
                         std::string& err) {
  if (int rc = exclusive_sum_u64(d_len, d_offsets, n_windows + 1, st, err)) return rc;
  if (!total || !n_windows) return FAC_OK;
  const uint64_t tiles = (total + kGatherTile - 1) / kGatherTile;  // < 2^28: total < 2^40
  const int wide = (reinterpret_cast<uintptr_t>(d_out) & 15u) == 0 ? 1 : 0;
  hipLaunchKernelGGL(stream_gather_kernel, dim3((uint32_t)tiles), dim3(kGatherThreads), 0, st, d_text, text_len, d_src,
                     d_offsets, n_windows, d_out, total, wide);
  HIP_TRY(hipGetLastError());
  return FAC_OK;
}

}  // namespace fac
