// prefilter_kernels.hip — CDNA4 (gfx950) kernels and host side of the bit-parallel pre-filter
// (prefilter.rs:247-435): the ASCII transcode, the packed bitap scan, the pigeonhole q-gram scan and
// verify, the coverage runs of one text and of a batch of documents, and the launchers that turn a
// view, a batch of stream windows or a batch of documents into merged windows for the search.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <tuple>

#include "fac_internal.h"
#include "host_util.h"
#include "wave_util.h"

namespace fac {
namespace {

// ------------------------------------------------------------------------------------------
// Bit-parallel pre-filter (prefilter.rs:247-435)
// ------------------------------------------------------------------------------------------

// transcode, ASCII fast path (prefilter.rs:253-260): ids[i] = ascii_id[byte]
__global__ void transcode_ascii_kernel(const uint8_t* __restrict__ utf8, uint64_t n, const uint8_t* __restrict__ ascii_id,
                                       uint8_t* __restrict__ ids) {
  const uint64_t i0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * 16;
  if (i0 + 16 <= n) {
    const uint4 v = *reinterpret_cast<const uint4*>(utf8 + i0);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t o[4];
    for (int q = 0; q < 4; ++q) {
      uint32_t r = 0;
      for (int b = 0; b < 4; ++b) r |= (uint32_t)ascii_id[(w[q] >> (8 * b)) & 0x7Fu] << (8 * b);
      o[q] = r;
    }
    *reinterpret_cast<uint4*>(ids + i0) = make_uint4(o[0], o[1], o[2], o[3]);
  } else {
    for (uint64_t i = i0; i < n; ++i) ids[i] = ascii_id[utf8[i] & 0x7Fu];
  }
}

struct BitapParams {
  const uint8_t* ids;
  uint64_t n;
  const void* mask_t;      // [(alphabet+1)][n_words] transposed packed masks (uint32_t or uint64_t words)
  const void* top;         // per word: the top (match) bit of every pattern packed into it
  const uint32_t* k;       // per word: the edit budget shared by its patterns
  uint32_t n_words;
  uint32_t seg_len;        // text positions owned by one wave
  uint32_t* cover;         // coverage bitmap, 1 bit per grapheme
  const uint32_t* dstart;  // DOCS: 1 bit per text position, set where a document of a batch starts
};

// The document-start bitmap of a batch (one bit per byte of the concatenated text, set at the first
// byte of every non-empty document; (n + 31) / 32 words). Documents are disjoint, so these two
// lookups are all the pre-filter needs to keep automaton state and coverage inside a document.
// The last document start in [lo, hi] (hi < n), or lo if there is none.
__device__ __forceinline__ uint64_t doc_start_back(const uint32_t* __restrict__ ds, uint64_t lo, uint64_t hi) {
  for (uint64_t w = hi >> 5;; --w) {
    uint32_t v = ds[w];
    if (w == (hi >> 5)) v &= 0xFFFFFFFFu >> (31u - (uint32_t)(hi & 31));
    if (w == (lo >> 5)) v &= 0xFFFFFFFFu << (uint32_t)(lo & 31);
    if (v) return w * 32 + (31u - (uint32_t)__builtin_clz(v));
    if (w == (lo >> 5)) return lo;
  }
}
// (a call: inlined into bitap_kernel's unrolled hit loop it doubled the scan's registers)
__device__ __attribute__((noinline)) uint64_t doc_start_back_call(const uint32_t* __restrict__ ds, uint64_t lo, uint64_t hi) {
  return doc_start_back(ds, lo, hi);
}
// The first document start in [lo, hi) (hi <= n), or hi if there is none.
__device__ __forceinline__ uint64_t doc_start_fwd(const uint32_t* __restrict__ ds, uint64_t lo, uint64_t hi) {
  if (lo >= hi) return hi;
  const uint64_t wl = (hi - 1) >> 5;
  for (uint64_t w = lo >> 5; w <= wl; ++w) {
    uint32_t v = ds[w];
    if (w == (lo >> 5)) v &= 0xFFFFFFFFu << (uint32_t)(lo & 31);
    if (v) return min(hi, w * 32 + (uint32_t)__builtin_ctz(v));
  }
  return hi;
}

// Shift-AND over several patterns per automaton word: the patterns of one edit budget are packed
// side by side (pattern f in bits lo_f..top_f). Every recurrence of bitap_windows
// (prefilter.rs:410-435) only moves bits upwards by one, so a pattern's top bit carries into the next
// pattern's bit 0 only, and that bit is forced to 1 in every level (the `| 1` of the recurrence,
// here `| first`) -- level 0 ANDs the carried bit with the same mask bit as the forced one. Bits
// 0..m-1 of every field therefore evolve exactly as in a word of their own; the reference's bits at
// and above m never reach below m, so dropping them changes nothing observable.
template <typename W>
__device__ __forceinline__ W low_bits(uint32_t n) {
  return n >= sizeof(W) * 8 ? ~(W)0 : (((W)1 << n) - (W)1);
}

// bitap_kernel<.., DOCS>'s rolled loop: the coverage [end - span, end) of every hit of the symbol at i,
// clipped to the start of the document holding it (as the scan's own hit loop)
template <typename W>
__device__ __attribute__((noinline)) void bitap_cover_docs(const uint32_t* __restrict__ dstart, uint32_t* __restrict__ cover, W hits, W top,
                                                           uint32_t k, uint64_t i) {
  const uint64_t end = i + 1;
  do {
    const uint32_t hi = (uint32_t)__builtin_ctzll((unsigned long long)hits);
    hits &= hits - 1;
    const W below = top & low_bits<W>(hi);
    const uint32_t lo = below ? 64u - (uint32_t)__builtin_clzll((unsigned long long)below) : 0u;
    const uint64_t span = (uint64_t)(hi + 1 - lo) + k;
    const uint64_t ws = doc_start_back(dstart, end > span ? end - span : 0, i);
    for (uint64_t x = ws; x < end;) {
      const uint64_t w = x >> 5;
      const uint32_t l = (uint32_t)(x & 31);
      const uint32_t cnt = (uint32_t)min((uint64_t)(32 - l), end - x);
      const uint32_t bits = (cnt == 32 ? 0xFFFFFFFFu : ((1u << cnt) - 1u)) << l;
      atomicOr(cover + w, bits);
      x += cnt;
    }
  } while (hits);
}

// Each lane runs one packed word over the wave's text segment. The state after `m + k` symbols no
// longer depends on the initial state, so a segment starts `m + k` symbols early from the
// reference's initial state and only reports ends inside its own range. Every hit of pattern f
// covers [end - m_f - k, end) in the bitmap; maximal runs of the bitmap are exactly the sorted +
// merged windows of prefilter.rs:334-342.
// W: the automaton word (uint32_t when every pattern has m <= 32: half the VALU work of uint64_t);
// KMAX: the largest edit budget (levels above a word's own k are computed but never read).
// DOCS: the text is a batch of documents (B.dstart). Every lane of a wave steps the same position, so
// "this symbol starts a document" is wave-uniform: the state goes back to the initial one there
// (a document's automaton starts at its first symbol, prefilter.rs:415-418), which also makes the
// warm-up exact from the last document start inside it, and a hit's coverage is clipped to its
// document's start instead of the text's.
template <int KMAX, typename W, bool DOCS = false>
__global__ __launch_bounds__(256) void bitap_kernel(BitapParams B) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const uint32_t word_groups = (B.n_words + 63) / 64;
  const uint64_t seg = wave / word_groups;
  const uint32_t p = (wave % word_groups) * 64 + lane;
  const uint64_t a = seg * B.seg_len;
  if (a >= B.n) return;
  const uint64_t b = min(a + (uint64_t)B.seg_len, B.n);
  const bool live = p < B.n_words;
  const W top = live ? static_cast<const W*>(B.top)[p] : (W)0;
  const uint32_t k = live ? B.k[p] : 0;
  const W first = (W)(top << 1) | (W)1;  // bit 0 of every field
  W r[KMAX + 1];
  // initial state R[d] = (1 << d) - 1 per pattern (prefilter.rs:417), clipped to the field
#pragma unroll
  for (int d = 0; d <= KMAX; ++d) r[d] = 0;
  {
    uint32_t lo = 0;
    for (W t = top; t;) {
      const uint32_t hi = (uint32_t)__builtin_ctzll((unsigned long long)t);
      t &= t - 1;
      const uint32_t m = hi + 1 - lo;
#pragma unroll
      for (int d = 1; d <= KMAX; ++d) r[d] |= low_bits<W>(min((uint32_t)d, m)) << lo;
      lo = hi + 1;
    }
  }
  // Start 87 = 63 + 24 symbols early: from there on the automaton state equals the one obtained by
  // scanning from the text start (an alignment with <= k errors spans <= m + k symbols).
  const uint64_t warm = 63 + 24;
  const uint64_t s0 = a > warm ? a - warm : 0;
  // Symbols come in 64 at a time (lane l loads symbol i0 + l, broadcast by readlane) and each lane
  // issues the masks of 8 symbols before stepping through them, so the loop waits on one memory
  // round trip per 8 symbols instead of two per symbol.
  // (DOCS with 64-bit words and 24 levels: 4, which keeps the second loop's registers out of scratch)
  constexpr uint32_t U = (DOCS && sizeof(W) == 8 && KMAX > 16) ? 4 : 8;
  const W* mask_p = static_cast<const W*>(B.mask_t) + (live ? p : 0u);  // this lane's column
  for (uint64_t i0 = s0; i0 < b; i0 += 64) {
    const uint32_t cl = i0 + lane < b ? (uint32_t)B.ids[i0 + lane] : 0u;
    const uint32_t nsym = (uint32_t)min((uint64_t)64, b - i0);
    uint64_t dmask = 0;  // DOCS: bit u = position i0 + u starts a document (wave-uniform)
    if constexpr (DOCS) {
      const uint64_t w0 = i0 >> 5, nwd = (B.n + 31) >> 5;
      const uint32_t sh = (uint32_t)(i0 & 31);
      const uint64_t lo = (uint64_t)B.dstart[w0] | ((w0 + 1 < nwd ? (uint64_t)B.dstart[w0 + 1] : 0ull) << 32);
      const uint64_t hi = (sh && w0 + 2 < nwd) ? (uint64_t)B.dstart[w0 + 2] : 0ull;
      dmask = sh ? (lo >> sh) | (hi << (64 - sh)) : lo;
      dmask = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)dmask) |
              ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(dmask >> 32)) << 32);
    }
    for (uint32_t u0 = 0; u0 < nsym; u0 += U) {
      W bcs[U];
#pragma unroll
      for (uint32_t q = 0; q < U; ++q) {
        const uint32_t c = (uint32_t)__builtin_amdgcn_readlane((int)cl, (int)(u0 + q));  // u0 + q < 64: wave-uniform
        bcs[q] = (live && u0 + q < nsym) ? mask_p[(size_t)c * B.n_words] : (W)0;
      }
      if constexpr (DOCS) {
        // A document starts among these U symbols (wave-uniform): they are stepped one by one in a
        // rolled loop (the masks rotate through bcs[0], so nothing is indexed by the loop counter),
        // the state going back to the initial one -- level d holds the low min(d, m) bits of every
        // field -- before the document's first symbol. Every other group takes the loop below as it is.
        if ((dmask >> u0) & ((1ull << U) - 1ull)) {
#pragma unroll 1
          for (uint32_t q = 0; q < U && u0 + q < nsym; ++q) {
            if ((dmask >> (u0 + q)) & 1ull) {  // (bits above the last field are never read, as in the steps)
              r[0] = (W)0;
#pragma unroll
              for (int d = 1; d <= KMAX; ++d) r[d] = d == 1 ? first : (W)(r[d - 1] | ((W)(r[d - 1] << 1) & ~first));
            }
            const W bc = bcs[0];
#pragma unroll
            for (uint32_t x = 0; x + 1 < U; ++x) bcs[x] = bcs[x + 1];
            W prev_old = r[0];
            W prev_new = ((r[0] << 1) | first) & bc;
            r[0] = prev_new;
            W hit_level = (k == 0) ? prev_new : (W)0;
#pragma unroll
            for (int d = 1; d <= KMAX; ++d) {
              const W old = r[d];
              const W nv = ((old << 1) & bc) | ((prev_old | prev_new) << 1) | prev_old | first;
              r[d] = nv;
              prev_old = old;
              prev_new = nv;
              if ((uint32_t)d == k) hit_level = nv;
            }
            const W hits = hit_level & top;
            if (live && hits && i0 + u0 + q >= a) bitap_cover_docs<W>(B.dstart, B.cover, hits, top, k, i0 + u0 + q);
          }
          continue;
        }
      }
      // the hits of the 8 symbols are kept and only looked at when one of them is set (rare): the
      // per-symbol path carries no segment-range compare and no divergent branch
      W hq[U];
#pragma unroll
      for (uint32_t q = 0; q < U; ++q) hq[q] = (W)0;
#pragma unroll
      for (uint32_t q = 0; q < U; ++q) {
        if (u0 + q >= nsym) break;
        const W bc = bcs[q];
        W prev_old = r[0];
        W prev_new = ((r[0] << 1) | first) & bc;
        r[0] = prev_new;
        W hit_level = (k == 0) ? prev_new : (W)0;
#pragma unroll
        for (int d = 1; d <= KMAX; ++d) {
          const W old = r[d];
          const W nv = ((old << 1) & bc) | ((prev_old | prev_new) << 1) | prev_old | first;
          r[d] = nv;  // levels above k are computed but never read
          prev_old = old;
          prev_new = nv;
          if ((uint32_t)d == k) hit_level = nv;
        }
        hq[q] = hit_level & top;  // R[k] subsumes the lower levels
      }
      W any = (W)0;
#pragma unroll
      for (uint32_t q = 0; q < U; ++q) any |= hq[q];
      if (live && any) {
#pragma unroll
        for (uint32_t q = 0; q < U; ++q) {
          W hits = hq[q];
          const uint64_t i = i0 + u0 + q;
          if (!hits || i < a) continue;  // ends before the segment belong to the previous wave
          const uint64_t end = i + 1;
          do {
            const uint32_t hi = (uint32_t)__builtin_ctzll((unsigned long long)hits);
            hits &= hits - 1;
            const W below = top & low_bits<W>(hi);  // tops of the fields under this one
            const uint32_t lo = below ? 64u - (uint32_t)__builtin_clzll((unsigned long long)below) : 0u;
            const uint64_t span = (uint64_t)(hi + 1 - lo) + k;
            uint64_t ws = end > span ? end - span : 0;
            if constexpr (DOCS) ws = doc_start_back_call(B.dstart, ws, i);  // the document holding the end
            for (uint64_t x = ws; x < end;) {  // set bits [ws, end)
              const uint64_t w = x >> 5;
              const uint32_t l = (uint32_t)(x & 31);
              const uint32_t cnt = (uint32_t)min((uint64_t)(32 - l), end - x);
              const uint32_t bits = (cnt == 32 ? 0xFFFFFFFFu : ((1u << cnt) - 1u)) << l;
              atomicOr(B.cover + w, bits);
              x += cnt;
            }
          } while (hits);
        }
      }
    }
  }
}

// ---- Pigeonhole q-gram filter in front of the bitap scan (exact) ----
// A pattern of m symbols within k Levenshtein edits of a text window keeps at least one of k + 1
// disjoint pieces of itself untouched, i.e. that piece occurs verbatim in the window. Each piece
// contributes its first q symbols (q = min(4, shortest piece), >= 3) as a gram; qgram_scan_kernel
// looks every text position's 3- and 4-gram up in a small cache-resident table and lists the
// (position, pattern, piece offset) candidates. qgram_verify_kernel runs the pattern's own bitap
// recurrence (prefilter.rs:410-435) over the only ends the candidate allows -- piece at text t,
// pattern offset o: end in [t + m - o - k, t + m - o + k] -- starting m + k symbols early, where the
// automaton state no longer depends on where the scan began (bitap_kernel's warm-up), and sets the
// same coverage bits as bitap_kernel. Every hit of every gram-eligible pattern is thus found (and no
// other: the recurrence is exact), so the merged windows equal the full scan's.
struct QgramParams {
  // the text: symbol ids (ids mode), or an ASCII haystack's bytes read directly (bytes mode: the
  // grams are keyed by case-folded bytes, verify maps bytes to ids through aid); text position i is
  // buffer byte off + i (the buffer 16-byte aligned), and bytes at or past nsafe are never read
  const uint8_t* ids;
  uint64_t n;
  uint64_t nsafe;
  uint32_t off, bytes, ci;
  const uint8_t* aid;
  const uint2* tab;        // open addressing: {gram key, first entry << 8 | entries} (0: empty slot)
  uint32_t tab_mask;
  const uint2* ent;        // entries: {pattern << 8 | piece offset, m | k << 8} (one load per candidate)
  uint32_t use3, use4;     // gram lengths in use
  uint32_t use5;           // 4-gram probes screened by the 5-gram (pieces of >= 5 symbols)
  // candidates (text position << 24 | entry index): scan block b fills region b of cand (region
  // entries, rcnt[b] of them valid), and what does not fit goes to the overflow list ovf
  unsigned long long* cand;
  uint64_t region;
  uint32_t* rcnt;
  uint32_t nreg;
  unsigned long long* ovf;
  unsigned long long* n_ovf;
  uint64_t ovf_cap;
  const uint64_t* pmask;   // per pattern: [rows] symbol masks (bit j = the pattern's j-th symbol)
  const uint32_t* pm;      // per pattern: m | k << 8
  uint32_t rows;
  uint32_t* cover;
  const uint32_t* bits;    // QG_BITS_WORDS: screening bitmap of the grams (qgram_bit)
  const uint32_t* m16;     // every q-gram pattern m <= 16: [pattern][rows] 16-bit masks, m16_words words
  uint32_t m16_words;
  // stream windows (a batch of stream.rs windows searched by one pass over their union, the view):
  // window w is the text [wlo[w], whi[w]) of the view, sorted by wlo, overlapping only its neighbours;
  // its coverage goes to cover (w even) or cover2 (w odd), so same-parity windows never touch.
  // wtab[t >> QG_WSH]: the last window starting at or before that bucket's first position.
  uint32_t nwin;
  const uint64_t* wlo;
  const uint64_t* whi;
  const uint32_t* wtab;
  uint32_t* cover2;
  // wsh != 0: window w is [w << wsh, min(n, (w + 1) << wsh) + wov)) -- the crate's fixed-size cut,
  // bounds computed instead of loaded
  uint32_t wsh, wov;
  // a batch of documents (qgram_verify_docs_kernel): the document-start bitmap, (n + 31) / 32 words
  const uint32_t* dstart;
};
constexpr uint32_t QG_WSH = 16;  // window-table buckets of 64 Ki positions
__host__ __device__ inline uint32_t qgram_key(uint32_t a, uint32_t b, uint32_t c, uint32_t d, bool q4) {
  return q4 ? (a | (b << 8) | (c << 16) | (d << 24)) : (a | (b << 8) | (c << 16) | 0xFF000000u);
}
__host__ __device__ inline uint32_t qgram_hash(uint32_t h) {  // murmur3 finalizer: every key bit reaches the low bits
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  return h ^ (h >> 16);
}

__device__ __forceinline__ uint32_t qgram_find(const QgramParams& Q, uint32_t key) {  // 0: none
  uint32_t s = qgram_hash(key) & Q.tab_mask;
  for (;;) {
    const uint2 e = Q.tab[s];
    if (e.y == 0u) return 0u;
    if (e.x == key) return e.y;
    s = (s + 1) & Q.tab_mask;
  }
}

// The screening bitmap's hash (64 Kbit; the table probe behind it keeps qgram_hash). Built on the
// host, copied into LDS per block. Bit = the top 18 bits of P = key[0:24) * A for a 3-gram, of
// P + key[8:32) * B for a 4-gram: full-rate 24-bit multiplies (a 32-bit v_mul_lo is quarter rate, and
// the scan's VALU count bounds it); a position's 3- and 4-gram share P (their first three symbols), so
// the pair costs one multiply and one v_mad_u32_u24, and the scan reads the bit as byte hash >> 17,
// bit (hash >> 14) & 7 with no masking. 3-gram keys carry 0xFF as their fourth symbol (qgram_key).
// 256 Kbit: every false pass costs a queue round and a table probe (C5 scan per GiB, profiles/r05_scan:
// 64 / 128 / 256 Kbit 1.49 / 1.14 / 1.11 ms).
__host__ __device__ inline uint32_t qg_mul24(uint32_t a, uint32_t b) { return (a & 0xFFFFFFu) * (b & 0xFFFFFFu); }
constexpr uint32_t QG_HA = 0x9E3779u, QG_HB = 0x85EBCAu;
#ifndef FAC_QG_BITS_LOG
#define FAC_QG_BITS_LOG 18
#endif
constexpr uint32_t QG_BITS_LOG = FAC_QG_BITS_LOG;  // log2 of the bitmap's bits
__host__ __device__ inline uint32_t qgram_bit(uint32_t key) {
  const uint32_t p = qg_mul24(key, QG_HA);
  return ((key >> 24) == 0xFFu ? p : p + qg_mul24(key >> 8, QG_HB)) >> (32 - QG_BITS_LOG);
}
constexpr uint32_t QG_BITS_WORDS = (1u << QG_BITS_LOG) / 32;
// A piece of >= 5 symbols is screened by its first five (round 6): its table key stays the 4-gram,
// but its bit is qgram_bit5 of the 4-gram and the fifth symbol, so a text position whose 4-gram
// matches a piece while its fifth symbol does not (C5: most of the 34 M candidates per GiB of
// 4-gram screening -- random vocabulary words sharing four letters with a pattern piece) rarely
// passes, and the verify no longer runs for it. Exact: a true hit keeps a whole piece, whose first
// five symbols lie in the text.
constexpr uint32_t QG_HC = 0xC2B2AEu;
__host__ __device__ inline uint32_t qgram_bit5(uint32_t key4, uint32_t c5) {
  const uint32_t h4 = qg_mul24(key4, QG_HA) + qg_mul24(key4 >> 8, QG_HB);
  return (h4 + qg_mul24((key4 >> 16) | (c5 << 16), QG_HC)) >> (32 - QG_BITS_LOG);
}

// Candidates go to the block's own region of the list, reserved with an LDS counter: one global
// list counter took a same-address atomic per flush of a per-wave buffer, and those atomics
// serialised at one L2 channel (C5, 34 M candidates per GiB: 256-entry flushes 1.87 ms per GiB,
// 128-entry 3.68, one atomic per wave turn 175 ms; per-block regions 1.14; profiles/r05_scan). 16 waves
// per block share the screening bitmap: 32 KB + 1.5 KB per wave = 56 KB, 2 blocks = 32 waves per CU
// (8-wave blocks: 44 KB, 3 blocks = 24 waves, 1.09 against 1.00 ms per GiB).
#ifndef FAC_QG_WAVES
#define FAC_QG_WAVES 16
#endif
constexpr uint32_t QG_WAVES = FAC_QG_WAVES;
// The bitmap screens every position first: only the ~3 % that pass (C5) probe the table in global
// memory, 64 at a time from a per-wave LDS queue (one table round trip per 64 passing grams: probing
// where they stood cost a round trip per wave step, since some lane of 64 passes almost every one).
// Round 5: a thread's 32 grams (16 positions x 3-/4-gram, one 16-byte load) are screened together
// into a pass mask, and the passes join the queue in rounds of one per lane (one ballot per round)
// instead of a ballot per gram.
constexpr uint32_t QG_PQ = 128;  // per-wave probe queue (LDS): < 64 left after a drain + one round
// 4 buffer bytes from byte b (4-aligned), zero at and past nsafe
__device__ __forceinline__ uint32_t qg_word(const QgramParams& Q, uint64_t b) {
  if (b + 4 <= Q.nsafe) return reinterpret_cast<const uint32_t*>(Q.ids)[b >> 2];
  uint32_t w = 0;
  for (uint32_t u = 0; u < 4; ++u)
    if (b + u < Q.nsafe) w |= (uint32_t)Q.ids[b + u] << (8 * u);
  return w;
}
// ASCII case folding of four bytes < 0x80 (the engine's fold for ASCII haystacks, builder.cpp ascii_id)
__device__ __forceinline__ uint32_t qg_fold(uint32_t w) {
  const uint32_t t = w | 0x80808080u;
  const uint32_t up = ((t - 0x41414141u) & ~(t - 0x5B5B5B5Bu)) & 0x80808080u;  // bytes in 'A'..'Z'
  return w + (up >> 2);
}
// U3 / U4: 3- / 4-grams in use (C5: 4-grams only, so the 3-grams' bitmap reads are not issued)
template <bool U3, bool U4, bool U5>
__global__ __launch_bounds__(64 * QG_WAVES) void qgram_scan_kernel(QgramParams Q) {
  __shared__ uint32_t s_bits[QG_BITS_WORDS];
  __shared__ uint32_t s_cnt, s_fail;  // region entries reserved; the first reservation that did not fit
  __shared__ uint32_t s_pk[QG_WAVES][QG_PQ];
  __shared__ uint64_t s_pp[QG_WAVES][QG_PQ];
  for (uint32_t x = threadIdx.x; x < QG_BITS_WORDS; x += blockDim.x) s_bits[x] = Q.bits[x];
  if (threadIdx.x == 0) {
    s_cnt = 0;
    s_fail = (uint32_t)Q.region;
  }
  __syncthreads();
  unsigned long long* const reg = Q.cand + (uint64_t)blockIdx.x * Q.region;
  uint32_t* pk = s_pk[threadIdx.x / 64];
  uint64_t* pp = s_pp[threadIdx.x / 64];
  uint32_t nq = 0;  // wave-uniform
  auto drain = [&](bool all) {
    while (nq >= 64 || (all && nq > 0)) {
      const uint32_t take = min(nq, 64u), lane = lane_id();
      uint32_t h = 0;
      uint64_t pos = 0;
      __builtin_amdgcn_wave_barrier();
      if (lane < take) {
        pos = pp[nq - take + lane];
        h = qgram_find(Q, pk[nq - take + lane]);
      }
      __builtin_amdgcn_wave_barrier();
      nq -= take;
      const uint32_t cnt = h & 0xFFu;
      if (!__ballot(cnt)) continue;
      const uint32_t incl = wave_inclusive_sum(cnt), tot = shfl_u32(incl, 63);
      uint32_t r0 = 0;
      if (lane == 63) r0 = atomicAdd(&s_cnt, tot);
      r0 = shfl_u32(r0, 63);
      unsigned long long* dst = reg;
      uint64_t at = r0 + (incl - cnt), lim = Q.region;
      if ((uint64_t)r0 + tot > Q.region) {  // region full: the overflow list
        unsigned long long o0 = 0;
        if (lane == 63) {
          atomicMin(&s_fail, r0);
          o0 = atomicAdd(Q.n_ovf, (unsigned long long)tot);
        }
        dst = Q.ovf;
        at = shfl_u64(o0, 63) + (incl - cnt);
        lim = Q.ovf_cap;
      }
      for (uint32_t y = 0; y < cnt; ++y, ++at)
        if (at < lim) dst[at] = (pos << 24) | ((h >> 8) + y);
    }
  };
  // a thread takes 16 consecutive positions from one aligned 16-byte load plus the next word
  // (positions whose gram would cross the text's end are not looked up)
  const uint4* ids16 = reinterpret_cast<const uint4*>(Q.ids);
  const uint32_t* ids32 = reinterpret_cast<const uint32_t*>(Q.ids);
  const uint8_t* s_bytes = reinterpret_cast<const uint8_t*>(s_bits);
  const uint64_t nbuf = Q.off + Q.n;  // buffer bytes of the text
  const uint64_t n16 = (nbuf + 15) / 16;  // buffer sixteens
  // sixteens whose 20 bytes lie below nsafe: read with plain loads
  const uint64_t gdir = min(n16, Q.nsafe >= 20 ? (Q.nsafe - 20) / 16 + 1 : (uint64_t)0);
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  const uint64_t lane64 = threadIdx.x % 64;
  uint64_t g0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x - lane64;  // whole waves iterate together
  auto turn = [&](uint64_t g, uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t w4)
                  __attribute__((always_inline)) {
    if (Q.bytes && Q.ci) {
      w0 = qg_fold(w0);
      w1 = qg_fold(w1);
      w2 = qg_fold(w2);
      w3 = qg_fold(w3);
      w4 = qg_fold(w4);
    }
    // symbols j .. j + 3 of this thread's sixteen (value selects: a select of references became a
    // pointer array in scratch)
    auto gram4 = [w0, w1, w2, w3, w4](uint32_t j) -> uint32_t {
      const uint32_t q = j >> 2;
      uint32_t lo = w0, hi = w1;
      lo = q >= 1u ? w1 : lo;
      hi = q >= 1u ? w2 : hi;
      lo = q >= 2u ? w2 : lo;
      hi = q >= 2u ? w3 : hi;
      lo = q >= 3u ? w3 : lo;
      hi = q >= 3u ? w4 : hi;
      return __builtin_amdgcn_alignbyte(hi, lo, j & 3u);
    };
    // pass mask: bit 2j = the 4-gram at buffer byte 16g + j (text position 16g + j - off), bit
    // 2j + 1 = its 3-gram. Every bitmap read is unconditional (the text bounds are a mask applied
    // after), so the LDS reads go out in batches: per-gram conditions had made each a branch with its
    // own wait.
    uint32_t pm = 0;
    auto screen = [&](auto all_in) {  // all_in: every gram of the sixteen lies inside the text
#pragma unroll
      for (uint32_t j = 0; j < 16; ++j) {
        // qgram_bit of the 3-gram (h3) and the 4-gram (h4) at this position, qgram_bit5 (h5)
        const uint32_t k4 = gram4(j), h3 = qg_mul24(k4, QG_HA), h4 = h3 + qg_mul24(k4 >> 8, QG_HB);
        constexpr uint32_t sh = 32 - QG_BITS_LOG;
        if constexpr (U4) pm |= __builtin_amdgcn_ubfe(s_bytes[h4 >> (sh + 3)], (h4 >> sh) & 7u, 1u) << (2 * j);
        if constexpr (U5) {
          const uint32_t wq = (j + 4) >> 2;  // symbol j + 4: in w1..w4 (j + 4 <= 19)
          const uint32_t c5 = ((wq == 1u ? w1 : wq == 2u ? w2 : wq == 3u ? w3 : w4) >> (8 * ((j + 4) & 3u))) & 0xFFu;
          const uint32_t h5 = h4 + qg_mul24((k4 >> 16) | (c5 << 16), QG_HC);
          pm |= __builtin_amdgcn_ubfe(s_bytes[h5 >> (sh + 3)], (h5 >> sh) & 7u, 1u) << (2 * j);
        }
        if constexpr (U3) pm |= __builtin_amdgcn_ubfe(s_bytes[h3 >> (sh + 3)], (h3 >> sh) & 7u, 1u) << (2 * j + 1);
      }
      if (!all_in) {
        uint32_t ok = 0;
        for (uint32_t j = 0; j < 16; ++j) {
          const uint64_t i = 16 * g + j;
          if (i >= Q.off && i + 4 <= nbuf) ok |= 1u << (2 * j);
          if (i >= Q.off && i + 3 <= nbuf) ok |= 1u << (2 * j + 1);
        }
        pm &= ok;
      }
    };
    if (g < n16) {
      if (16 * g >= Q.off && 16 * g + 19 <= nbuf) screen(std::true_type{});
      else screen(std::false_type{});
    }
    // rounds: each lane's next pass joins the queue (in lane order within a round)
    for (;;) {
      const bool has = pm != 0;
      const uint64_t m = __ballot(has);
      if (!m) break;
      if (nq + 64 > QG_PQ) drain(false);
      if (has) {
        const uint32_t bit = (uint32_t)__builtin_ctz(pm);
        pm &= pm - 1;
        const uint32_t j = bit >> 1;
        const uint32_t k4 = gram4(j);
        const uint32_t at = nq + prefix_below(m);
        pk[at] = (bit & 1u) ? ((k4 & 0xFFFFFFu) | 0xFF000000u) : k4;
        pp[at] = 16 * g + j - Q.off;
      }
      nq += (uint32_t)__popcll(m);
    }
  };
  // Turns whose every sixteen reads directly: the next turn's loads are issued before this turn's
  // screening, unconditionally (past the direct range they read sixteen 0 and are not used) -- under
  // a branch, the load's join waited for it and the prefetch hid nothing. A full probe queue goes out
  // before the prefetch (loads retire in order: a wait on the probe would wait for the prefetch too).
  if (g0 + 64 <= gdir) {
    uint4 an = ids16[g0 + lane64];
    uint32_t xn = ids32[4 * (g0 + lane64) + 4];
    for (; g0 + 64 <= gdir; g0 += stride) {
      const uint32_t w0 = an.x, w1 = an.y, w2 = an.z, w3 = an.w, w4 = xn;
      if (nq >= 64) drain(false);
      const uint64_t gn = g0 + stride + lane64 < gdir ? g0 + stride + lane64 : 0;
      an = ids16[gn];
      xn = ids32[4 * gn + 4];
      turn(g0 + lane64, w0, w1, w2, w3, w4);
    }
  }
  // the text's last sixteens (no read at or past nsafe)
  for (; g0 < n16; g0 += stride) {
    const uint64_t g = g0 + lane64;
    if (nq >= 64) drain(false);
    turn(g, qg_word(Q, 16 * g), qg_word(Q, 16 * g + 4), qg_word(Q, 16 * g + 8), qg_word(Q, 16 * g + 12),
         qg_word(Q, 16 * g + 16));
  }
  drain(true);
  __syncthreads();
  if (threadIdx.x == 0) Q.rcnt[blockIdx.x] = min(s_cnt, s_fail);
}

// coverage [end - span, end) clipped to the text start wlo, as bitap_kernel (a hit: rare, kept out
// of the verify's unrolled symbol loop)
__device__ __attribute__((noinline)) void qgram_cover(uint32_t* cover, uint64_t wlo, uint64_t span, uint64_t end) {
  const uint64_t ws = end > wlo + span ? end - span : wlo;
  for (uint64_t y = ws; y < end;) {
    const uint64_t w = y >> 5;
    const uint32_t l = (uint32_t)(y & 31);
    const uint32_t cnt = (uint32_t)min((uint64_t)(32 - l), end - y);
    const uint32_t bits = (cnt == 32 ? 0xFFFFFFFFu : ((1u << cnt) - 1u)) << l;
    atomicOr(cover + w, bits);
    y += cnt;
  }
}

// W: the automaton word, uint32_t when every q-gram pattern has m <= 32 (half the 64-bit VALU work)
// One candidate (qgram_verify_kernel). LM: every q-gram pattern has m <= 16 and their masks fit in
// LDS (16-bit, pattern-major): the mask reads are LDS reads instead of L2 round trips.
// The text is [wlo, whi) of the view (the whole view, or one stream window of a batch): the
// recurrence starts from its initial state at wlo (prefilter.rs:415-418, a window's text begins
// there) or m + k symbols before the first end it reports, and coverage bits go to `cover`.
template <int KMAX, typename W, bool LM>
__device__ __forceinline__ void verify_one(const QgramParams& Q, unsigned long long cd, uint2 en, const uint8_t* s_aid,
                                           const uint16_t* s_m16, uint64_t wlo, uint64_t whi, uint32_t* cover) {
  const uint64_t t = cd >> 24;
  const uint32_t p = en.x >> 8, o = en.x & 0xFFu, m = en.y & 0xFFu, k = en.y >> 8;
  // ends the candidate allows, 1-based: [t + m - o - k, t + m - o + k], clipped to the text
  const int64_t lo = (int64_t)t + m - o - k, hi = (int64_t)t + m - o + k;
  const uint64_t e_min = (uint64_t)max<int64_t>((int64_t)wlo + 1, lo);
  const uint64_t e_max = (uint64_t)min<int64_t>((int64_t)whi, hi);
  if (e_min > e_max) return;
  const uint64_t warm = (uint64_t)m + k;
  const uint64_t s0 = e_min - 1 > wlo + warm ? e_min - 1 - warm : wlo;
  const uint64_t* mask = Q.pmask + (size_t)p * Q.rows;
  const uint16_t* mask16 = s_m16 + (size_t)p * Q.rows;  // LM: the pattern's masks in LDS
  const W top = (W)1 << (m - 1);
  W r[KMAX + 1];
#pragma unroll
  for (int d = 0; d <= KMAX; ++d) r[d] = d ? (((W)1 << d) - (W)1) : (W)0;  // prefilter.rs:415-418
  // the symbols [s0, e_max) in aligned 4-symbol words, up to 64 per pass, loaded together; their masks
  // 16 at a time (one round trip for the words and one per 16 masks: C5's candidates span ~23
  // symbols, three round trips instead of six); W = uint32_t reads the masks' low halves only
  // (text positions; buffer byte = position + off, both 4-aligned when base is: off % 4 folded in)
  const uint32_t* mask32 = reinterpret_cast<const uint32_t*>(mask);
  const uint32_t sh = Q.off & 3u;
  auto cover_end = [&](uint64_t end) { qgram_cover(cover, wlo, (uint64_t)m + k, end); };
  {
    // Short spans (every C5 candidate: m + 3k + 1 <= 23 symbols): the symbols [s0, e_max) from eight
    // words realigned to s0 (v_alignbyte), stepped exactly -- the general loop below runs whole
    // 16-symbol chunks from the aligned word before s0 (32 steps for C5's ~20; round 5: 941 VALU
    // instructions per candidate)
    const uint64_t ns = e_max - s0;
    const uint64_t wb = (s0 + sh) & ~3ull, bb = wb + (Q.off - sh);
    if (ns <= 28 && bb + 32 <= Q.nsafe) {
      const uint32_t* w32 = reinterpret_cast<const uint32_t*>(Q.ids) + (bb >> 2);
      uint32_t wd[8];
#pragma unroll
      for (uint32_t u = 0; u < 8; ++u) wd[u] = w32[u];
      const uint32_t al = (uint32_t)(s0 + sh - wb);
      uint32_t sw[7];
#pragma unroll
      for (uint32_t u = 0; u < 7; ++u) sw[u] = __builtin_amdgcn_alignbyte(wd[u + 1], wd[u], al);
      const uint32_t nsym = (uint32_t)ns, t_end = (uint32_t)(e_min - 1 - s0);
#pragma unroll
      for (uint32_t t = 0; t < 28; ++t) {
        if (t >= nsym) continue;  // (not break: the loop must unroll -- sw is indexed by t)
        uint32_t sym = (sw[t >> 2] >> (8 * (t & 3u))) & 0xFFu;
        if (Q.bytes) sym = s_aid[sym & 0x7Fu];
        const W bc = LM ? (W)mask16[sym] : sizeof(W) == 4 ? (W)mask32[2 * sym] : (W)mask[sym];
        W prev_old = r[0];
        W prev_new = ((r[0] << 1) | (W)1) & bc;
        r[0] = prev_new;
        W hit = (k == 0) ? prev_new : (W)0;
#pragma unroll
        for (int d = 1; d <= KMAX; ++d) {
          const W old = r[d];
          const W nv = ((old << 1) & bc) | ((prev_old | prev_new) << 1) | prev_old | (W)1;
          r[d] = nv;
          prev_old = old;
          prev_new = nv;
          if ((uint32_t)d == k) hit = nv;
        }
        if (t >= t_end && (hit & top)) cover_end(s0 + t + 1);
      }
      return;
    }
  }
  // per pass, 32-bit bounds relative to the pass's first buffer word (u = 16c + v indexes its
  // symbols): symbols u in [u_lo, u_hi) are stepped, ends at u >= u_end report (a pass spans 64
  // symbols, so every bound fits; 64-bit compares per symbol cost as much as the recurrence)
  for (uint64_t base = (s0 + sh) & ~3ull; base < e_max + sh; base += 64) {  // buffer bytes - (off - sh)
    uint32_t wd[16];
    const uint64_t nw = min<uint64_t>(16, (e_max + sh - base + 3) / 4);
    const uint64_t bb = base + (Q.off - sh);  // the buffer byte of word 0 (4-aligned)
    if (bb + 64 <= Q.nsafe) {
      const uint32_t* w32 = reinterpret_cast<const uint32_t*>(Q.ids) + (bb >> 2);
#pragma unroll
      for (uint32_t u = 0; u < 16; ++u) wd[u] = u < nw ? w32[u] : 0u;
    } else {  // the text's end: no read at or past nsafe
      for (uint32_t u = 0; u < 16; ++u) wd[u] = u < nw ? qg_word(Q, bb + 4 * u) : 0u;
    }
    const int32_t u_lo = (int32_t)min<int64_t>((int64_t)(s0 + sh) - (int64_t)base, 64);
    const int32_t u_hi = (int32_t)min<uint64_t>(e_max + sh - base, 64);
    // end (1-based text position) of symbol u: base + u - sh + 1 >= e_min
    const int32_t u_end = (int32_t)max<int64_t>(-1, min<int64_t>((int64_t)(e_min + sh) - (int64_t)base - 1, 64));
#pragma unroll
    for (uint32_t c = 0; c < 4; ++c) {
      if ((int32_t)(16 * c) >= u_hi) break;
      W bcs[16];
#pragma unroll
      for (uint32_t v = 0; v < 16; ++v) {
        const int32_t u = (int32_t)(16 * c + v);
        uint32_t sym = (wd[4 * c + v / 4] >> (8 * (v % 4))) & 0xFFu;
        if (Q.bytes) sym = s_aid[sym & 0x7Fu];
        if (u >= u_lo && u < u_hi)
          bcs[v] = LM ? (W)mask16[sym] : sizeof(W) == 4 ? (W)mask32[2 * sym] : (W)mask[sym];
        else bcs[v] = (W)0;
      }
#pragma unroll
      for (uint32_t v = 0; v < 16; ++v) {
        const int32_t u = (int32_t)(16 * c + v);
        if (u >= u_hi) break;
        if (u < u_lo) continue;
        const W bc = bcs[v];
        W prev_old = r[0];
        W prev_new = ((r[0] << 1) | (W)1) & bc;
        r[0] = prev_new;
        W hit = (k == 0) ? prev_new : (W)0;
#pragma unroll
        for (int d = 1; d <= KMAX; ++d) {
          const W old = r[d];
          const W nv = ((old << 1) & bc) | ((prev_old | prev_new) << 1) | prev_old | (W)1;
          r[d] = nv;
          prev_old = old;
          prev_new = nv;
          if ((uint32_t)d == k) hit = nv;
        }
        if (u >= u_end && (hit & top)) cover_end(base + (uint64_t)u - sh + 1);
      }
    }
  }
}

// WIN: a batch of stream windows -- each candidate is verified for the window(s) holding its gram
// position (two in an overlap), with that window's bounds and coverage bitmap
template <int KMAX, typename W, bool LM, bool WIN>
__global__ __launch_bounds__(LM ? 512 : 256) void qgram_verify_kernel(QgramParams Q) {
  __shared__ uint8_t s_aid[128];  // bytes mode: byte -> symbol id
  extern __shared__ uint16_t s_m16[];  // LM: Q.m16_words 32-bit words of 16-bit masks
  if (Q.bytes)
    for (uint32_t i = threadIdx.x; i < 128; i += blockDim.x) s_aid[i] = Q.aid[i];
  if constexpr (LM)
    for (uint32_t i = threadIdx.x; i < Q.m16_words; i += blockDim.x) reinterpret_cast<uint32_t*>(s_m16)[i] = Q.m16[i];
  __syncthreads();
  // persistent: block b takes the scan's regions b, b + grid, ..., then (region nreg) the overflow list.
  // (Loading two candidates and their entries per thread before verifying either measured no faster:
  // 1.37 ms per GiB held to 128 VGPRs, 1.96 at 133 VGPRs, against 1.36; profiles/r05_scan.)
  for (uint32_t r = blockIdx.x; r <= Q.nreg; r += gridDim.x) {
    const unsigned long long* base = r < Q.nreg ? Q.cand + (uint64_t)r * Q.region : Q.ovf;
    const uint64_t cnt = r < Q.nreg ? (uint64_t)Q.rcnt[r] : min((uint64_t)*Q.n_ovf, Q.ovf_cap);
    for (uint64_t x = threadIdx.x; x < cnt; x += blockDim.x) {
      const unsigned long long cd = base[x];
      if constexpr (!WIN) {
        verify_one<KMAX, W, LM>(Q, cd, Q.ent[cd & 0xFFFFFFu], s_aid, s_m16, 0, Q.n, Q.cover);
      } else {
        const uint64_t t = cd >> 24;
        uint32_t w;
        if (Q.wsh) {
          w = (uint32_t)min(t >> Q.wsh, (uint64_t)(Q.nwin - 1));
        } else {
          w = Q.wtab[t >> QG_WSH];
          while (w + 1 < Q.nwin && Q.wlo[w + 1] <= t) ++w;
        }
        const uint2 en = Q.ent[cd & 0xFFFFFFu];
        for (uint32_t d = 0; d < 2; ++d) {  // the window holding t, then its predecessor if they overlap at t
          if (d > w) break;
          const uint32_t ww = w - d;
          const uint64_t lo = Q.wsh ? (uint64_t)ww << Q.wsh : Q.wlo[ww];
          const uint64_t hi = Q.wsh ? min(Q.n, lo + (1ull << Q.wsh) + Q.wov) : Q.whi[ww];
          if (t >= lo && t < hi) verify_one<KMAX, W, LM>(Q, cd, en, s_aid, s_m16, lo, hi, (ww & 1u) ? Q.cover2 : Q.cover);
        }
      }
    }
  }
}

// The verify of a batch of documents (Q.dstart, the document-start bitmap): a candidate is verified
// once, for the document holding its gram position t. Only the part of that document the candidate
// can reach matters -- the recurrence starts at most m + 2k + 1 <= 112 symbols before t and ends at
// most m + k <= 87 after it -- so its bounds are the document starts found within 128 positions
// before t and 96 after it (none found: the range's own end, which verify_one then never reaches).
// A gram that straddles a boundary is a harmless extra candidate of the document it starts in.
template <int KMAX, typename W, bool LM>
__global__ __launch_bounds__(LM ? 512 : 256) void qgram_verify_docs_kernel(QgramParams Q) {
  __shared__ uint8_t s_aid[128];  // bytes mode: byte -> symbol id
  extern __shared__ uint16_t s_m16[];  // LM: Q.m16_words 32-bit words of 16-bit masks
  if (Q.bytes)
    for (uint32_t i = threadIdx.x; i < 128; i += blockDim.x) s_aid[i] = Q.aid[i];
  if constexpr (LM)
    for (uint32_t i = threadIdx.x; i < Q.m16_words; i += blockDim.x) reinterpret_cast<uint32_t*>(s_m16)[i] = Q.m16[i];
  __syncthreads();
  for (uint32_t r = blockIdx.x; r <= Q.nreg; r += gridDim.x) {  // regions as qgram_verify_kernel
    const unsigned long long* base = r < Q.nreg ? Q.cand + (uint64_t)r * Q.region : Q.ovf;
    const uint64_t cnt = r < Q.nreg ? (uint64_t)Q.rcnt[r] : min((uint64_t)*Q.n_ovf, Q.ovf_cap);
    for (uint64_t x = threadIdx.x; x < cnt; x += blockDim.x) {
      const unsigned long long cd = base[x];
      const uint64_t t = cd >> 24;
      if (t >= Q.n) continue;
      const uint64_t lo = doc_start_back(Q.dstart, t > 128 ? t - 128 : 0, t);
      const uint64_t hi = doc_start_fwd(Q.dstart, t + 1, min(Q.n, t + 96));
      verify_one<KMAX, W, LM>(Q, cd, Q.ent[cd & 0xFFFFFFu], s_aid, s_m16, lo, hi, Q.cover);
    }
  }
}

// Runs of a batch's coverage bitmap, cut at document starts (two documents' coverage can touch:
// "...hello" | "hello..."): a run starts at a set bit whose predecessor is clear or which starts a
// document, and ends at the first clear bit or the next document start. Counted per bitmap word,
// scanned, then written in place (runs_docs_write_kernel), so the runs come out sorted by start with
// no list to overflow and no sort.
__device__ __forceinline__ uint32_t run_starts(const uint32_t* __restrict__ cover, const uint32_t* __restrict__ ds,
                                               uint64_t w, uint64_t n) {
  const uint32_t cur = cover[w];
  const uint32_t prev_hi = w > 0 ? (cover[w - 1] >> 31) : 0u;
  uint32_t starts = cur & (~((cur << 1) | prev_hi) | ds[w]);
  if (n - w * 32 < 32) starts &= (1u << (uint32_t)(n - w * 32)) - 1u;  // (the bitmap's last word)
  return starts;
}
__global__ void runs_docs_count_kernel(const uint32_t* __restrict__ cover, const uint32_t* __restrict__ ds,
                                       uint64_t n_words, uint64_t n, uint64_t* __restrict__ cnt) {
  const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w > n_words) return;
  cnt[w] = w < n_words ? (uint64_t)__popc(run_starts(cover, ds, w, n)) : 0ull;  // (entry n_words: the scan's total)
}
// One SegDesc per run (a merged window searched as a haystack of its own, prefilter.rs:346-350,
// tagged with its document like batch_desc_kernel's) and its length for the window prefix.
__global__ void runs_docs_write_kernel(const uint32_t* __restrict__ cover, const uint32_t* __restrict__ ds,
                                       uint64_t n_words, uint64_t n, const uint64_t* __restrict__ pos,
                                       const uint64_t* __restrict__ off, uint64_t n_docs, SegDesc* __restrict__ segs,
                                       uint64_t* __restrict__ lens) {
  const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= n_words) return;
  uint32_t starts = run_starts(cover, ds, w, n);
  uint64_t idx = pos[w];
  while (starts) {
    const uint32_t b = __ffs(starts) - 1;
    starts &= starts - 1;
    const uint64_t s = w * 32 + b;
    uint64_t e = n;  // the first clear bit or document start after s
    for (uint64_t ww = w; ww < n_words; ++ww) {
      uint32_t stop = ~cover[ww] | ds[ww];
      if (ww == w) stop &= b == 31 ? 0u : (0xFFFFFFFFu << (b + 1));
      if (stop) {
        e = min(n, ww * 32 + (uint64_t)__builtin_ctz(stop));
        break;
      }
    }
    uint64_t lo = 0, hi = n_docs;  // the last document with off[d] <= s: the non-empty one holding s
    while (hi - lo > 1) {
      const uint64_t mid = (lo + hi) / 2;
      if (off[mid] <= s) lo = mid;
      else hi = mid;
    }
    SegDesc S;
    S.text_base = s;
    S.n = e - s;
    S.avail = S.n;
    S.hay_len = S.n;
    S.byte_base = s | (lo << kDocTagShift);
    S.w_begin = 0;
    S.w_end = S.n;
    S.ascii = 1u;
    S.pad = 0;
    segs[idx] = S;
    lens[idx] = S.n;
    ++idx;
  }
}
// The same for a batch that holds non-ASCII documents, whose runs are in the batch's start-window
// space (Batch::d_prefix): run [s, e) lies in non-empty document k, found by bisection, at local
// symbols [i, i + e - s). In an ASCII document that is runs_docs_write_kernel's descriptor. In any
// other it is the slice of graphemes [gs, ge) = bytes [bs, be) (stage_kernels.hip slice_desc_kernel,
// tagged), written here as a Unicode slice; slice_ascii_kernel then turns the all-ASCII slices into
// byte texts (search_raw decides is_ascii per slice, prefilter.rs:349-350). tri (optional): the
// window as {document, start, end} in document-relative symbols.
__global__ void runs_docs_write_mixed_kernel(const uint32_t* __restrict__ cover, const uint32_t* __restrict__ ds,
                                             uint64_t n_words, uint64_t n, const uint64_t* __restrict__ pos,
                                             const uint64_t* __restrict__ off, const SegDesc* __restrict__ dsegs,
                                             const uint64_t* __restrict__ dprefix, uint64_t n_segs,
                                             SegDesc* __restrict__ segs, uint64_t* __restrict__ lens,
                                             uint64_t* __restrict__ tri) {
  const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= n_words) return;
  uint32_t starts = run_starts(cover, ds, w, n);
  uint64_t idx = pos[w];
  constexpr uint64_t kByte = (1ull << kDocTagShift) - 1;
  while (starts) {
    const uint32_t b = __ffs(starts) - 1;
    starts &= starts - 1;
    const uint64_t s = w * 32 + b;
    uint64_t e = n;  // the first clear bit or document start after s
    for (uint64_t ww = w; ww < n_words; ++ww) {
      uint32_t stop = ~cover[ww] | ds[ww];
      if (ww == w) stop &= b == 31 ? 0u : (0xFFFFFFFFu << (b + 1));
      if (stop) {
        e = min(n, ww * 32 + (uint64_t)__builtin_ctz(stop));
        break;
      }
    }
    uint64_t lo = 0, hi = n_segs;  // the last non-empty document with dprefix[k] <= s
    while (hi - lo > 1) {
      const uint64_t mid = (lo + hi) / 2;
      if (dprefix[mid] <= s) lo = mid;
      else hi = mid;
    }
    const SegDesc D = dsegs[lo];
    const uint64_t doc = D.byte_base >> kDocTagShift, i = s - dprefix[lo], cnt = e - s;
    SegDesc S;
    if (D.ascii) {
      S.text_base = D.text_base + i;
      S.n = cnt;
      S.hay_len = cnt;
      S.byte_base = S.text_base | (doc << kDocTagShift);
      S.ascii = 1u;
    } else {
      const uint64_t gs = D.text_base + i, ge = gs + cnt;
      const uint64_t bs = off[gs] & kByte;
      const uint64_t be = i + cnt < D.n ? off[ge] & kByte : (D.byte_base & kByte) + D.hay_len;
      S.text_base = gs;
      S.n = cnt;
      S.hay_len = be - bs;
      S.byte_base = bs | (doc << kDocTagShift);
      S.ascii = 0u;
    }
    S.avail = S.n;
    S.w_begin = 0;
    S.w_end = S.n;
    S.pad = 0;
    segs[idx] = S;
    lens[idx] = S.n;
    if (tri) {
      tri[3 * idx] = doc;
      tri[3 * idx + 1] = i;
      tri[3 * idx + 2] = i + cnt;
    }
    ++idx;
  }
}
// One wave per merged window: the OR of the bytes of a Unicode slice (a window can be long); a slice
// without a high bit becomes the ASCII text of its bytes. Windows of ASCII documents return at once.
__global__ __launch_bounds__(256) void slice_ascii_kernel(const uint8_t* __restrict__ utf8, uint64_t len,
                                                          SegDesc* __restrict__ segs, uint64_t* __restrict__ lens,
                                                          uint64_t n_runs) {
  const uint64_t r = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= n_runs) return;
  if (segs[r].ascii) return;
  constexpr uint64_t kByte = (1ull << kDocTagShift) - 1;
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t bs = segs[r].byte_base & kByte, cnt = segs[r].hay_len;
  if (bs + cnt > len) return;  // (never for a staged batch)
  const uint8_t* p = utf8 + bs;
  const uint64_t mis = (8u - (uint32_t)(reinterpret_cast<uintptr_t>(p) & 7u)) & 7u;
  const uint64_t head = mis < cnt ? mis : cnt;
  const uint64_t words = (cnt - head) / 8, tail = head + words * 8;
  uint64_t acc = 0;
  for (uint64_t i = lane; i < head; i += 64) acc |= p[i];
  const uint64_t* q = reinterpret_cast<const uint64_t*>(p + head);
  for (uint64_t i = lane; i < words; i += 64) acc |= q[i];
  for (uint64_t i = tail + lane; i < cnt; i += 64) acc |= p[i];
  const bool high = __ballot((acc & 0x8080808080808080ull) != 0) != 0;
  if (high || lane != 0) return;
  SegDesc S = segs[r];
  S.ascii = 1u;
  S.text_base = bs;
  S.n = cnt;
  S.avail = cnt;
  S.w_end = cnt;
  segs[r] = S;
  lens[r] = cnt;
}
// The document-start bitmap: one thread per document, one bit per non-empty document
__global__ void doc_starts_kernel(const uint64_t* __restrict__ off, uint64_t n_docs, uint32_t* __restrict__ ds) {
  const uint64_t d = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= n_docs) return;
  const uint64_t a = off[d];
  if (off[d + 1] > a) atomicOr(ds + (a >> 5), 1u << (uint32_t)(a & 31));
}

// Maximal runs of set bits -> [start, end) windows (unordered; the host sorts them).
__global__ void runs_kernel(const uint32_t* __restrict__ cover, uint64_t n_words, uint64_t n,
                            unsigned long long* __restrict__ out, unsigned long long* __restrict__ count,
                            uint64_t cap) {
  const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= n_words) return;
  const uint32_t cur = cover[w];
  const uint32_t prev_hi = w > 0 ? (cover[w - 1] >> 31) : 0u;
  uint32_t starts = cur & ~((cur << 1) | prev_hi);  // bit set, previous bit clear
  while (starts) {
    const uint32_t b = __ffs(starts) - 1;
    starts &= starts - 1;
    const uint64_t s = w * 32 + b;
    if (s >= n) break;
    uint64_t e;  // first clear bit at or after s
    uint64_t ww = w;
    uint32_t bits = cur | (b ? ((1u << b) - 1u) : 0u);
    for (;;) {
      const uint32_t inv = ~bits;
      if (inv) {
        e = ww * 32 + (uint64_t)__builtin_ctz(inv);
        break;
      }
      if (++ww >= n_words) {
        e = n_words * 32;
        break;
      }
      bits = cover[ww];
    }
    if (e > n) e = n;
    const unsigned long long idx = atomicAdd(count, 1ull);
    if (idx < cap) {
      out[2 * idx] = s;
      out[2 * idx + 1] = e;
    }
  }
}

// The pre-filter's device tables for the edit budgets ks (PfTables), built once per engine, ks and
// mode: the packed full-scan words and the q-gram path's tables (want_bytes: keyed by case-folded
// bytes when the q-gram path takes every pattern). Host work and uploads measured 0.41 ms per C5
// stream window when rebuilt per call.
int pf_tables(const Engine& e, const std::vector<uint32_t>& ks, bool want_bytes, const PfTables*& out, std::string& err) {
  const bool qgram_on = !diag_env("FAC_NO_QGRAM");
  std::lock_guard<std::mutex> lk(e.pf_mu);
  for (const auto& t : e.pf_cache)
    if (t->ks == ks && t->want_bytes == want_bytes && t->qgram_on == qgram_on) {
      out = t.get();
      return FAC_OK;
    }
  auto T = std::make_unique<PfTables>();
  T->ks = ks;
  T->want_bytes = want_bytes;
  T->qgram_on = qgram_on;
  const uint32_t np = (uint32_t)e.bp_m.size();
  const uint32_t rows = e.alphabet + 1;
  auto upload_raw = [&](const void* src, size_t bytes, void*& dst) -> int {
    HIP_TRY(hipMalloc(&dst, std::max<size_t>(bytes, 16)));
    if (bytes) HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
    return FAC_OK;
  };
  // Pigeonhole q-gram path (qgram_scan_kernel / qgram_verify_kernel) for the patterns whose k + 1
  // pieces are at least 3 symbols long; the rest go through the full bitap scan.
  std::vector<uint8_t> qlen(np, 0);
  std::vector<std::pair<uint32_t, uint32_t>> grams;  // (gram key, pattern << 8 | piece offset)
  std::vector<uint32_t> gram5;                       // per gram: its piece's fifth symbol (0xFFFF: none)
  if (qgram_on && rows <= 256) {
    std::vector<uint32_t> sym(64);
    // 5-gram screens only when no piece is screened by its 3-gram: 3-grams pass so often that they
    // make most candidates, and the extra screen then costs more than it removes (C5: 33.0 M
    // candidates per GiB either way, scan 1.02 -> 1.16 ms per GiB)
    bool any3 = false;
    for (uint32_t i = 0; i < np; ++i) any3 = any3 || (e.bp_m[i] <= 63 && e.bp_m[i] / (ks[i] + 1) == 3);
    for (uint32_t i = 0; i < np; ++i) {
      const uint32_t m = e.bp_m[i], k = ks[i], L = m / (k + 1);
      if (L < 3 || m > 63) continue;
      bool one = true;  // every pattern position is exactly one symbol
      for (uint32_t j = 0; j < m; ++j) {
        uint32_t hits = 0;
        for (uint32_t c = 0; c < rows; ++c)
          if ((e.bp_mask[(size_t)i * rows + c] >> j) & 1ull) sym[j] = c, ++hits;
        one = one && hits == 1;
      }
      if (!one) continue;
      const bool five = L >= 5 && !any3 && !diag_env("FAC_QG_NO5");
      const uint32_t q = std::min<uint32_t>(4, L);
      qlen[i] = (uint8_t)(five ? 5 : q);
      for (uint32_t r = 0; r <= k; ++r) {
        const uint32_t o = (uint32_t)((uint64_t)r * m / (k + 1));
        grams.push_back({qgram_key(sym[o], sym[o + 1], sym[o + 2], q == 4 ? sym[o + 3] : 0u, q == 4), (i << 8) | o});
      }
    }
    std::sort(grams.begin(), grams.end());
    for (const auto& g : grams) {  // (after the sort: gram5 follows grams' order)
      const uint32_t i = g.second >> 8, o = g.second & 0xFFu;
      if (qlen[i] != 5) {
        gram5.push_back(0xFFFFu);
        continue;
      }
      uint32_t c = 0;
      for (uint32_t cc = 0; cc < rows; ++cc)
        if ((e.bp_mask[(size_t)i * rows + cc] >> (o + 4)) & 1ull) c = cc;
      gram5.push_back(c);
    }
    for (size_t a = 0, b; a < grams.size(); a = b) {  // at most 255 entries per gram (table word)
      for (b = a; b < grams.size() && grams[b].first == grams[a].first; ++b) {}
      if (b - a > 255) {
        std::fill(qlen.begin(), qlen.end(), 0);
        grams.clear();
        gram5.clear();
        break;
      }
    }
  }
  // Pack the full-scan patterns into automaton words: patterns of one edit budget, longest first,
  // each into the first word with room (first-fit decreasing); 32-bit words when every pattern fits.
  std::vector<uint32_t> order;
  for (uint32_t i = 0; i < np; ++i)
    if (!qlen[i]) order.push_back(i);
  uint32_t mmax = 0;
  for (uint32_t i : order) mmax = std::max(mmax, e.bp_m[i]);
  const bool w32 = mmax <= 32;
  const uint32_t wbits = w32 ? 32u : 64u;
  std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
    return ks[x] != ks[y] ? ks[x] < ks[y] : (e.bp_m[x] != e.bp_m[y] ? e.bp_m[x] > e.bp_m[y] : x < y);
  });
  std::vector<uint32_t> wk, wused;                   // per word: edit budget, bits used
  std::vector<std::pair<uint32_t, uint32_t>> place(np);  // pattern -> (word, bit offset)
  uint32_t k_first_word = 0;                         // words of the current budget start here
  for (uint32_t idx = 0; idx < (uint32_t)order.size(); ++idx) {
    const uint32_t i = order[idx], m = e.bp_m[i];
    if (idx && ks[i] != ks[order[idx - 1]]) k_first_word = (uint32_t)wk.size();
    uint32_t w = k_first_word;
    while (w < wk.size() && wused[w] + m > wbits) ++w;
    if (w == wk.size()) {
      wk.push_back(ks[i]);
      wused.push_back(0);
    }
    place[i] = {w, wused[w]};
    wused[w] += m;
  }
  const uint32_t nw = (uint32_t)wk.size();
  T->nw = nw;
  T->w32 = w32;
  for (uint32_t i : order) T->kmax = std::max(T->kmax, ks[i]);
  // Every pattern on the q-gram path: an ASCII text's bytes are read by the scan itself, so its grams
  // are keyed by each id's folded ASCII char (0x80: none, never in the text)
  T->bytes = want_bytes && nw == 0 && !grams.empty();
  if (T->bytes) {
    uint8_t byte_of_id[256];
    std::memset(byte_of_id, 0x80, sizeof(byte_of_id));
    for (uint32_t b = 0; b < 128; ++b) {
      const uint32_t id = e.ascii_id[b];
      if (id && byte_of_id[id] == 0x80) byte_of_id[id] = (uint8_t)(e.case_insensitive && b - 'A' < 26u ? b + 32u : b);
    }
    std::vector<std::pair<std::pair<uint32_t, uint32_t>, uint32_t>> g5(grams.size());
    for (size_t x = 0; x < grams.size(); ++x) {
      const uint32_t k = grams[x].first, q4 = (k >> 24) != 0xFFu;
      g5[x] = {{qgram_key(byte_of_id[k & 0xFFu], byte_of_id[(k >> 8) & 0xFFu], byte_of_id[(k >> 16) & 0xFFu],
                          q4 ? byte_of_id[k >> 24] : 0u, q4), grams[x].second},
               gram5[x] == 0xFFFFu ? 0xFFFFu : (uint32_t)byte_of_id[gram5[x]]};
    }
    std::sort(g5.begin(), g5.end());
    for (size_t x = 0; x < g5.size(); ++x) {
      grams[x] = g5[x].first;
      gram5[x] = g5[x].second;
    }
  }
  std::vector<uint64_t> pmask((size_t)rows * nw, 0), ptop(nw, 0);
  for (uint32_t i : order) {
    const uint32_t w = place[i].first, off = place[i].second;
    ptop[w] |= 1ull << (off + e.bp_m[i] - 1);
    for (uint32_t c = 0; c < rows; ++c) pmask[(size_t)c * nw + w] |= e.bp_mask[(size_t)i * rows + c] << off;
  }
  if (w32) {
    std::vector<uint32_t> m32(pmask.begin(), pmask.end()), t32(ptop.begin(), ptop.end());
    if (int rc = upload_raw(m32.data(), m32.size() * 4, T->pmask)) return rc;
    if (int rc = upload_raw(t32.data(), t32.size() * 4, T->ptop)) return rc;
  } else {
    if (int rc = upload_raw(pmask.data(), pmask.size() * 8, T->pmask)) return rc;
    if (int rc = upload_raw(ptop.data(), ptop.size() * 8, T->ptop)) return rc;
  }
  if (int rc = upload_raw(wk.data(), wk.size() * 4, T->wk)) return rc;
  if (!grams.empty()) {
    T->q = true;
    std::vector<uint2> ent(grams.size());
    std::vector<std::pair<uint32_t, uint32_t>> keys;  // (key, first entry << 8 | entries)
    for (size_t a = 0, b; a < grams.size(); a = b) {
      for (b = a; b < grams.size() && grams[b].first == grams[a].first; ++b) {
        const uint32_t i = grams[b].second >> 8;
        ent[b] = make_uint2(grams[b].second, e.bp_m[i] | (ks[i] << 8));
      }
      keys.push_back({grams[a].first, (uint32_t)(a << 8) | (uint32_t)(b - a)});
    }
    uint32_t ts = 64;
    while (ts < 2 * keys.size()) ts <<= 1;
    std::vector<uint2> tab(ts, make_uint2(0u, 0u));
    for (const auto& kv : keys) {
      uint32_t sl = qgram_hash(kv.first) & (ts - 1);
      while (tab[sl].y) sl = (sl + 1) & (ts - 1);
      tab[sl] = make_uint2(kv.first, kv.second);
    }
    std::vector<uint32_t> qbits(QG_BITS_WORDS, 0u);  // the scan's screening bitmap
    for (size_t x = 0; x < grams.size(); ++x) {
      const uint32_t b = gram5[x] == 0xFFFFu ? qgram_bit(grams[x].first) : qgram_bit5(grams[x].first, gram5[x]);
      qbits[b >> 5] |= 1u << (b & 31u);
    }
    std::vector<uint32_t> pm(np, 0);
    for (uint32_t i = 0; i < np; ++i)
      if (qlen[i]) {
        pm[i] = e.bp_m[i] | (ks[i] << 8);
        T->kq = std::max(T->kq, ks[i]);
        T->mq = std::max(T->mq, e.bp_m[i]);
        (qlen[i] == 5 ? T->use5 : qlen[i] == 4 ? T->use4 : T->use3) = 1u;
        T->n_qpat += 1;
      }
    T->ts = ts;
    T->n_grams = grams.size();
    T->n_keys = keys.size();
    if (int rc = upload_raw(tab.data(), tab.size() * sizeof(uint2), T->tab)) return rc;
    if (int rc = upload_raw(ent.data(), ent.size() * sizeof(uint2), T->ent)) return rc;
    if (int rc = upload_raw(e.bp_mask.data(), e.bp_mask.size() * 8, T->qmask)) return rc;
    if (int rc = upload_raw(pm.data(), pm.size() * 4, T->qpm)) return rc;
    if (int rc = upload_raw(qbits.data(), qbits.size() * 4, T->qbits)) return rc;
    // m <= 16 everywhere and a table within the 64 KB of dynamic LDS a block takes (two blocks per
    // CU, C5: 1 000 patterns x 27 rows = 54 KB): verify reads its masks from LDS
    const size_t n16 = ((size_t)np * rows + 1) & ~(size_t)1;
    if (T->mq <= 16 && n16 * 2 <= (64u << 10) - 256 && !diag_env("FAC_QGRAM_NO_LDS")) {
      std::vector<uint16_t> m16(n16, 0);
      for (size_t i = 0; i < (size_t)np * rows; ++i) m16[i] = (uint16_t)e.bp_mask[i];
      if (int rc = upload_raw(m16.data(), n16 * 2, T->m16)) return rc;
      T->m16_words = (uint32_t)(n16 / 2);
    }
  }
  out = T.get();
  e.pf_cache.push_back(std::move(T));
  return FAC_OK;
}

// qgram_verify_kernel for the tables' edit budget and mask layout: LDS masks in persistent blocks (two
// per CU), else global masks, 32- or 64-bit automaton words
// MODE 0: one text; 1: a batch of stream windows; 2: a batch of documents (qgram_verify_docs_kernel)
template <int KMAX, typename W, bool LM, int MODE>
constexpr auto qverify_fn() {
  if constexpr (MODE == 2) return &qgram_verify_docs_kernel<KMAX, W, LM>;
  else return &qgram_verify_kernel<KMAX, W, LM, MODE == 1>;
}
template <int MODE>
void launch_qverify(const PfTables& T, const QgramParams& Q, dim3 vg, hipStream_t stream) {
  const uint32_t kq = T.kq;
  // (MODE 2 with more than 8 levels reads its masks from global memory: 24 levels under the LDS
  // variant's 512-thread bound spill to scratch, and no kernel of the batch path may)
  if (T.m16 && (MODE != 2 || kq <= 8)) {
    const size_t lds = (size_t)T.m16_words * 4;
    if (kq <= 1) hipLaunchKernelGGL((qverify_fn<1, uint32_t, true, MODE>()), vg, dim3(512), lds, stream, Q);
    else if (kq <= 2) hipLaunchKernelGGL((qverify_fn<2, uint32_t, true, MODE>()), vg, dim3(512), lds, stream, Q);
    else if (kq <= 4) hipLaunchKernelGGL((qverify_fn<4, uint32_t, true, MODE>()), vg, dim3(512), lds, stream, Q);
    else if (kq <= 8) hipLaunchKernelGGL((qverify_fn<8, uint32_t, true, MODE>()), vg, dim3(512), lds, stream, Q);
    else if constexpr (MODE != 2) hipLaunchKernelGGL((qverify_fn<24, uint32_t, true, MODE>()), vg, dim3(512), lds, stream, Q);
  } else if (T.mq <= 32) {
    if (kq <= 1) hipLaunchKernelGGL((qverify_fn<1, uint32_t, false, MODE>()), vg, dim3(256), 0, stream, Q);
    else if (kq <= 2) hipLaunchKernelGGL((qverify_fn<2, uint32_t, false, MODE>()), vg, dim3(256), 0, stream, Q);
    else if (kq <= 4) hipLaunchKernelGGL((qverify_fn<4, uint32_t, false, MODE>()), vg, dim3(256), 0, stream, Q);
    else if (kq <= 8) hipLaunchKernelGGL((qverify_fn<8, uint32_t, false, MODE>()), vg, dim3(256), 0, stream, Q);
    else hipLaunchKernelGGL((qverify_fn<24, uint32_t, false, MODE>()), vg, dim3(256), 0, stream, Q);
  } else {
    if (kq <= 1) hipLaunchKernelGGL((qverify_fn<1, uint64_t, false, MODE>()), vg, dim3(256), 0, stream, Q);
    else if (kq <= 2) hipLaunchKernelGGL((qverify_fn<2, uint64_t, false, MODE>()), vg, dim3(256), 0, stream, Q);
    else if (kq <= 4) hipLaunchKernelGGL((qverify_fn<4, uint64_t, false, MODE>()), vg, dim3(256), 0, stream, Q);
    else if (kq <= 8) hipLaunchKernelGGL((qverify_fn<8, uint64_t, false, MODE>()), vg, dim3(256), 0, stream, Q);
    else hipLaunchKernelGGL((qverify_fn<24, uint64_t, false, MODE>()), vg, dim3(256), 0, stream, Q);
  }
}

// bitap_kernel for the tables' word size and largest edit budget
template <bool DOCS>
void launch_bitap(const PfTables& T, const BitapParams& B, dim3 bgrid, hipStream_t stream) {
  const uint32_t kmax = T.kmax;
  if (T.w32) {
    if (kmax == 0) hipLaunchKernelGGL((bitap_kernel<0, uint32_t, DOCS>), bgrid, dim3(256), 0, stream, B);
    else if (kmax == 1) hipLaunchKernelGGL((bitap_kernel<1, uint32_t, DOCS>), bgrid, dim3(256), 0, stream, B);
    else if (kmax == 2) hipLaunchKernelGGL((bitap_kernel<2, uint32_t, DOCS>), bgrid, dim3(256), 0, stream, B);
    else if (kmax <= 4) hipLaunchKernelGGL((bitap_kernel<4, uint32_t, DOCS>), bgrid, dim3(256), 0, stream, B);
    else if (kmax <= 8) hipLaunchKernelGGL((bitap_kernel<8, uint32_t, DOCS>), bgrid, dim3(256), 0, stream, B);
    else if (kmax <= 16) hipLaunchKernelGGL((bitap_kernel<16, uint32_t, DOCS>), bgrid, dim3(256), 0, stream, B);
    else hipLaunchKernelGGL((bitap_kernel<24, uint32_t, DOCS>), bgrid, dim3(256), 0, stream, B);
  } else {
    if (kmax <= 1) hipLaunchKernelGGL((bitap_kernel<1, uint64_t, DOCS>), bgrid, dim3(256), 0, stream, B);
    else if (kmax <= 2) hipLaunchKernelGGL((bitap_kernel<2, uint64_t, DOCS>), bgrid, dim3(256), 0, stream, B);
    else if (kmax <= 4) hipLaunchKernelGGL((bitap_kernel<4, uint64_t, DOCS>), bgrid, dim3(256), 0, stream, B);
    else if (kmax <= 8) hipLaunchKernelGGL((bitap_kernel<8, uint64_t, DOCS>), bgrid, dim3(256), 0, stream, B);
    else if (kmax <= 16) hipLaunchKernelGGL((bitap_kernel<16, uint64_t, DOCS>), bgrid, dim3(256), 0, stream, B);
    else hipLaunchKernelGGL((bitap_kernel<24, uint64_t, DOCS>), bgrid, dim3(256), 0, stream, B);
  }
}

// The q-gram path's parameters for a text of n symbols: the tables, the text buffer (the ids at d_ids,
// or with T.bytes the staged bytes from vb read in place) and the coverage bitmap
QgramParams qgram_params(const Engine& e, const Haystack& h, const PfTables& T, const uint8_t* vb, const void* d_ids,
                         uint64_t n, void* d_cover) {
  QgramParams Q{};
  Q.ids = static_cast<const uint8_t*>(d_ids);
  Q.n = n;
  Q.nsafe = n + 80;
  if (T.bytes) {
    Q.ids = reinterpret_cast<const uint8_t*>((uintptr_t)vb & ~(uintptr_t)15);
    Q.off = (uint32_t)(vb - Q.ids);
    Q.nsafe = (uint64_t)(h.d_utf8 + h.len - Q.ids);
    Q.bytes = 1;
    Q.ci = e.case_insensitive ? 1u : 0u;
    Q.aid = e.d_ascii_id;
  }
  Q.tab = static_cast<const uint2*>(T.tab);
  Q.tab_mask = T.ts - 1;
  Q.ent = static_cast<const uint2*>(T.ent);
  Q.use3 = T.use3;
  Q.use4 = T.use4;
  Q.use5 = T.use5;
  Q.pmask = static_cast<const uint64_t*>(T.qmask);
  Q.pm = static_cast<const uint32_t*>(T.qpm);
  Q.rows = e.alphabet + 1;
  Q.cover = static_cast<uint32_t*>(d_cover);
  Q.bits = static_cast<const uint32_t*>(T.qbits);
  Q.m16 = static_cast<const uint32_t*>(T.m16);
  Q.m16_words = T.m16_words;
  return Q;
}

// qgram_scan_kernel over the text: fills Q's candidate lists (held by b), scanning again with room for
// all of them if the overflow list overflowed. vg: the verify's grid; nc: the overflow entries.
struct QgramBufs {
  PoolBuf cand, n, ovf, rcnt;
};
int qgram_candidates(const Engine& e, const PfTables& T, QgramParams& Q, uint64_t n, hipStream_t stream, QgramBufs& b,
                     dim3& vg, unsigned long long& nc, std::string& err) {
  HIP_TRY(b.n.alloc(8, stream));
  Q.n_ovf = static_cast<unsigned long long*>(b.n.p);
  int cus = 256;
  HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, e.device));
  // two full resident rounds of scan blocks (2 per CU at 56 KB of LDS): the scan strides over the
  // text, so every block does the same work, and a grid of 8 per CU ran 2.7 rounds (the last one 2/3
  // full); one round left the verify's 2 persistent blocks per CU 1.5 regions each (1.21 vs 1.15 ms)
  // instantiations by the gram kinds in use (3-grams alone, 4-grams, 5-gram screens, or mixed)
  const uint32_t qk = (Q.use3 ? 1u : 0u) | (Q.use4 ? 2u : 0u) | (Q.use5 ? 4u : 0u);
  const void* scan_fns[8] = {reinterpret_cast<const void*>(&qgram_scan_kernel<true, false, false>),
                             reinterpret_cast<const void*>(&qgram_scan_kernel<true, false, false>),
                             reinterpret_cast<const void*>(&qgram_scan_kernel<false, true, false>),
                             reinterpret_cast<const void*>(&qgram_scan_kernel<true, true, false>),
                             reinterpret_cast<const void*>(&qgram_scan_kernel<false, false, true>),
                             reinterpret_cast<const void*>(&qgram_scan_kernel<true, false, true>),
                             reinterpret_cast<const void*>(&qgram_scan_kernel<false, true, true>),
                             reinterpret_cast<const void*>(&qgram_scan_kernel<true, true, true>)};
  const void* scan_fn = scan_fns[qk];
  int per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, scan_fn, 64 * QG_WAVES, 0) != hipSuccess || per_cu < 1)
    per_cu = 1;
  const uint32_t sgrid =
      (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n + 8191) / 8192, (uint64_t)cus * (uint64_t)per_cu * 2));
  // regions of 1/16 of a block's positions (C5 fills ~half); the overflow list is checked after
  Q.nreg = sgrid;
  Q.region = std::max<uint64_t>(256, (n / sgrid + 15) / 16);
  HIP_TRY(b.cand.alloc(Q.region * sgrid * 8, stream));
  HIP_TRY(b.rcnt.alloc((size_t)sgrid * 4, stream));
  Q.cand = static_cast<unsigned long long*>(b.cand.p);
  Q.rcnt = static_cast<uint32_t*>(b.rcnt.p);
  uint64_t ocap = 1 << 20;
  nc = 0;  // overflow entries
  for (;;) {  // candidates: one scan, again with room for all of them if the overflow list overflowed
    HIP_TRY(b.ovf.alloc(ocap * 8, stream));
    Q.ovf = static_cast<unsigned long long*>(b.ovf.p);
    Q.ovf_cap = ocap;
    HIP_TRY(hipMemsetAsync(b.n.p, 0, 8, stream));
    switch (qk) {
      case 2: hipLaunchKernelGGL((qgram_scan_kernel<false, true, false>), dim3(sgrid), dim3(64 * QG_WAVES), 0, stream, Q); break;
      case 3: hipLaunchKernelGGL((qgram_scan_kernel<true, true, false>), dim3(sgrid), dim3(64 * QG_WAVES), 0, stream, Q); break;
      case 4: hipLaunchKernelGGL((qgram_scan_kernel<false, false, true>), dim3(sgrid), dim3(64 * QG_WAVES), 0, stream, Q); break;
      case 5: hipLaunchKernelGGL((qgram_scan_kernel<true, false, true>), dim3(sgrid), dim3(64 * QG_WAVES), 0, stream, Q); break;
      case 6: hipLaunchKernelGGL((qgram_scan_kernel<false, true, true>), dim3(sgrid), dim3(64 * QG_WAVES), 0, stream, Q); break;
      case 7: hipLaunchKernelGGL((qgram_scan_kernel<true, true, true>), dim3(sgrid), dim3(64 * QG_WAVES), 0, stream, Q); break;
      default: hipLaunchKernelGGL((qgram_scan_kernel<true, false, false>), dim3(sgrid), dim3(64 * QG_WAVES), 0, stream, Q); break;
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&nc, b.n.p, 8, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (nc <= ocap) break;
    // which candidates overflow depends on wave timing (a block's first failed reservation varies
    // by up to one drain, 64 x 255 entries): regrow with headroom so the re-scan fits
    ocap = nc + nc / 4 + (uint64_t)sgrid * 64 * 255;
  }
  if (diag_env("FAC_TIMING")) {
    std::vector<uint32_t> rc(sgrid);
    HIP_TRY(hipMemcpyAsync(rc.data(), b.rcnt.p, (size_t)sgrid * 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    uint64_t tot = nc, mx = 0;
    for (uint32_t c : rc) tot += c, mx = std::max<uint64_t>(mx, c);
    std::fprintf(stderr, "FAC_QGRAM text %llu symbols, %llu candidates (%llu overflow, region %llu, fullest %llu), use3 %u use4 %u use5 %u\n",
                 (unsigned long long)n, (unsigned long long)tot, nc, (unsigned long long)Q.region,
                 (unsigned long long)mx, Q.use3, Q.use4, Q.use5);
  }
  vg = dim3((uint32_t)std::min<uint64_t>(sgrid + 1, (uint64_t)cus * (T.m16 ? 2 : 8)));
  return FAC_OK;
}

}  // namespace

int transcode_ascii_device(const Engine& e, const uint8_t* d_utf8, uint64_t n, uint8_t* d_ids, hipStream_t stream,
                           std::string& err) {
  if (n == 0) return FAC_OK;
  const uint64_t threads = (n + 15) / 16;
  hipLaunchKernelGGL(transcode_ascii_kernel, dim3((uint32_t)((threads + 255) / 256)), dim3(256), 0, stream, d_utf8, n,
                     e.d_ascii_id, d_ids);
  HIP_TRY(hipGetLastError());
  return FAC_OK;
}

int prefilter_windows(const Engine& e, const Haystack& h, const SegDesc& view, const std::vector<uint32_t>& ks,
                      hipStream_t stream, std::vector<std::pair<uint64_t, uint64_t>>& windows, fac_stats* stats,
                      std::string& err) {
  return prefilter_windows_ex(e, h, view, ks, stream, nullptr, windows, nullptr, stats, err);
}

// wins (optional): a batch of stream windows, [lo, hi) text positions of the view sorted by lo,
// each overlapping only its neighbours and not adjacent to the next-but-one (lo[w + 2] > hi[w]).
// Every window's bitap windows are its own -- the automaton starts at its lo, its coverage stays in
// it -- from one scan of the view; run_win receives each merged window's stream window. Returns
// FAC_E_UNSUPPORTED when some pattern needs the packed full scan (not window-aware).
int prefilter_windows_ex(const Engine& e, const Haystack& h, const SegDesc& view, const std::vector<uint32_t>& ks,
                         hipStream_t stream, const std::vector<std::pair<uint64_t, uint64_t>>* wins,
                         std::vector<std::pair<uint64_t, uint64_t>>& windows, std::vector<uint32_t>* run_win,
                         fac_stats* stats, std::string& err) {
  windows.clear();
  if (run_win) run_win->clear();
  HIP_TRY(hipSetDevice(e.device));
  if (!stream) stream = e.stream;
  const uint64_t n = view.n;
  if (n == 0) return FAC_OK;
  // An ASCII text whose bytes lie 16-byte aligned can be read by the q-gram scan itself, with no
  // transcode pass (0.66 ms per GiB at C5), when the q-gram path takes every pattern (pf_tables)
  const uint8_t* vb = h.d_utf8 + view.text_base;
  const bool want_bytes = view.ascii && ((uintptr_t)h.d_utf8 & 15u) == 0 && !diag_env("FAC_QGRAM_IDS");
  const PfTables* T = nullptr;
  if (int rc = pf_tables(e, ks, want_bytes, T, err)) return rc;
  const uint32_t nw = T->nw;
  const bool win = wins && !wins->empty();
  if (win && (nw != 0 || !T->q)) return FAC_E_UNSUPPORTED;  // the packed full scan has no window bounds
  PoolBuf d_ids, d_cover, d_runs, d_cnt, d_cover2, d_wlo, d_whi, d_wtab;
  if (!T->bytes) {  // the text's symbol ids (prefilter.rs:253-260)
    HIP_TRY(d_ids.alloc(n + 80, stream));  // padded: the scan's 16-byte loads and next word, verify's 64-symbol passes
    if (view.ascii) {  // transcode, ASCII text (prefilter.rs:253-258): one byte per grapheme
      const uint64_t threads = (n + 15) / 16;
      hipLaunchKernelGGL(transcode_ascii_kernel, dim3((uint32_t)((threads + 255) / 256)), dim3(256), 0, stream, vb, n,
                         e.d_ascii_id, static_cast<uint8_t*>(d_ids.p));
      HIP_TRY(hipGetLastError());
    } else {  // Unicode text (prefilter.rs:262-280): the id of every folded grapheme, looked up on the device
      if (int rc = symbol_ids_device(e, h, view.text_base, view.text_base + n, static_cast<uint8_t*>(d_ids.p), stream, err))
        return rc;
    }
  }
  const uint64_t n_words = (n + 31) / 32;
  HIP_TRY(d_cover.alloc(n_words * 4, stream));
  HIP_TRY(hipMemsetAsync(d_cover.p, 0, n_words * 4, stream));
  std::vector<uint64_t> wlo, whi;
  std::vector<uint32_t> wtab;
  if (win) {  // the batch's window bounds and bucket table (QgramParams::wtab)
    const size_t nwin = wins->size();
    wlo.resize(nwin);
    whi.resize(nwin);
    for (size_t w = 0; w < nwin; ++w) {
      wlo[w] = (*wins)[w].first;
      whi[w] = std::min<uint64_t>((*wins)[w].second, n);
    }
    wtab.resize((size_t)((n >> QG_WSH) + 1));
    uint32_t w = 0;
    for (size_t b = 0; b < wtab.size(); ++b) {
      while (w + 1 < nwin && wlo[w + 1] <= ((uint64_t)b << QG_WSH)) ++w;
      wtab[b] = w;
    }
    HIP_TRY(d_cover2.alloc(n_words * 4, stream));
    HIP_TRY(hipMemsetAsync(d_cover2.p, 0, n_words * 4, stream));
    HIP_TRY(d_wlo.alloc(nwin * 8, stream));
    HIP_TRY(d_whi.alloc(nwin * 8, stream));
    HIP_TRY(d_wtab.alloc(wtab.size() * 4, stream));
    HIP_TRY(hipMemcpyAsync(d_wlo.p, wlo.data(), nwin * 8, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(d_whi.p, whi.data(), nwin * 8, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(d_wtab.p, wtab.data(), wtab.size() * 4, hipMemcpyHostToDevice, stream));
  }
  Events ev;
  HIP_TRY(hipEventCreate(&ev.a));
  HIP_TRY(hipEventCreate(&ev.b));
  HIP_TRY(hipEventRecord(ev.a, stream));
  BitapParams B{};
  B.ids = static_cast<const uint8_t*>(d_ids.p);
  B.n = n;
  B.mask_t = T->pmask;
  B.top = T->ptop;
  B.k = static_cast<const uint32_t*>(T->wk);
  B.n_words = nw;
  B.seg_len = 4096;
  B.cover = static_cast<uint32_t*>(d_cover.p);
  const uint64_t segs = (n + B.seg_len - 1) / B.seg_len;
  const uint64_t waves = segs * ((nw + 63) / 64);
  const dim3 bgrid((uint32_t)std::max<uint64_t>(1, (waves + 3) / 4));
  if (nw != 0) launch_bitap<false>(*T, B, bgrid, stream);  // (0: every pattern takes the q-gram path)
  HIP_TRY(hipGetLastError());
  QgramBufs qb;
  if (T->q) {
    QgramParams Q = qgram_params(e, h, *T, vb, d_ids.p, n, d_cover.p);
    if (win) {
      Q.nwin = (uint32_t)wlo.size();
      Q.wlo = static_cast<const uint64_t*>(d_wlo.p);
      Q.whi = static_cast<const uint64_t*>(d_whi.p);
      Q.wtab = static_cast<const uint32_t*>(d_wtab.p);
      Q.cover2 = static_cast<uint32_t*>(d_cover2.p);
      // the fixed-size cut (window w at w * 2^sh, its text 2^sh + ov bytes): bounds by arithmetic
      if (wlo.size() > 1 && wlo[0] == 0 && (wlo[1] & (wlo[1] - 1)) == 0 && wlo[1] >= 64 && whi[0] > wlo[1]) {
        const uint32_t sh = (uint32_t)__builtin_ctzll(wlo[1]);
        const uint64_t ov = whi[0] - wlo[1];
        bool uni = ov < (1ull << 31);
        for (size_t w = 0; w < wlo.size() && uni; ++w)
          uni = wlo[w] == ((uint64_t)w << sh) && whi[w] == std::min<uint64_t>(n, wlo[w] + (1ull << sh) + ov);
        if (uni) {
          Q.wsh = sh;
          Q.wov = (uint32_t)ov;
        }
      }
    }
    dim3 vg;
    unsigned long long nc = 0;
    if (int rc = qgram_candidates(e, *T, Q, n, stream, qb, vg, nc, err)) return rc;
    if (Q.nwin) launch_qverify<1>(*T, Q, vg, stream);
    else launch_qverify<0>(*T, Q, vg, stream);
    HIP_TRY(hipGetLastError());
    if (diag_env("FAC_RC_DEBUG"))
      std::fprintf(stderr, "FAC_QGRAM patterns=%zu/%zu grams=%zu keys=%zu candidates=%llu full-scan words=%u bytes=%d\n",
                   T->n_qpat, e.bp_m.size(), T->n_grams, T->n_keys, nc, nw, (int)T->bytes);
  }
  // maximal runs of each bitmap (with windows: cover holds the even windows', cover2 the odd ones';
  // same-parity windows are not adjacent, so no run spans two of them)
  std::vector<uint32_t> par[2];  // the windows of each parity, ascending lo
  if (win)
    for (uint32_t w = 0; w < (uint32_t)wlo.size(); ++w) par[w & 1].push_back(w);
  std::vector<std::tuple<uint64_t, uint64_t, uint32_t>> runs;  // (start, end, stream window)
  const int npass = win ? 2 : 1;
  PoolBuf d_runs2;
  PoolBuf* rbuf[2] = {&d_runs, &d_runs2};
  uint64_t cap[2] = {1u << 16, 1u << 16};
  HIP_TRY(d_cnt.alloc(16, stream));
  for (;;) {  // both bitmaps' runs in one round trip; again with room for all of them if a list overflowed
    HIP_TRY(hipMemsetAsync(d_cnt.p, 0, 16, stream));
    for (int pass = 0; pass < npass; ++pass) {
      const uint32_t* cov = static_cast<const uint32_t*>(pass ? d_cover2.p : d_cover.p);
      HIP_TRY(rbuf[pass]->alloc(cap[pass] * 16, stream));
      hipLaunchKernelGGL(runs_kernel, dim3((uint32_t)((n_words + 255) / 256)), dim3(256), 0, stream, cov, n_words, n,
                         static_cast<unsigned long long*>(rbuf[pass]->p), static_cast<unsigned long long*>(d_cnt.p) + pass,
                         cap[pass]);
      HIP_TRY(hipGetLastError());
    }
    unsigned long long c[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(c, d_cnt.p, 16, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    bool again = false;
    for (int pass = 0; pass < npass; ++pass)
      if (c[pass] > cap[pass]) {
        cap[pass] = c[pass];
        again = true;
      }
    if (again) continue;
    std::vector<unsigned long long> buf[2];
    for (int pass = 0; pass < npass; ++pass) {
      buf[pass].resize(2 * c[pass]);
      if (c[pass]) HIP_TRY(hipMemcpyAsync(buf[pass].data(), rbuf[pass]->p, c[pass] * 16, hipMemcpyDeviceToHost, stream));
    }
    HIP_TRY(hipEventRecord(ev.b, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    for (int pass = 0; pass < npass; ++pass)
      for (uint64_t i = 0; i < c[pass]; ++i) {
        const uint64_t r0 = buf[pass][2 * i], r1 = buf[pass][2 * i + 1];
        uint32_t w = 0xFFFFFFFFu;
        if (win) {  // the window of this bitmap's parity whose [lo, hi) holds the run
          const auto& v = par[pass];
          auto it = std::upper_bound(v.begin(), v.end(), r0, [&](uint64_t x, uint32_t ww) { return x < wlo[ww]; });
          if (it != v.begin() && r0 < whi[*(it - 1)]) w = *(it - 1);
          if (w == 0xFFFFFFFFu) {
            err = "internal: a pre-filter run outside every stream window";
            return FAC_E_INTERNAL;
          }
        }
        runs.emplace_back(r0, r1, w);
      }
    break;
  }
  std::sort(runs.begin(), runs.end(), [](const auto& x, const auto& y) {
    return std::get<2>(x) != std::get<2>(y) ? std::get<2>(x) < std::get<2>(y) : std::get<0>(x) < std::get<0>(y);
  });
  windows.resize(runs.size());
  if (run_win) run_win->resize(runs.size());
  for (size_t r = 0; r < runs.size(); ++r) {
    windows[r] = {std::get<0>(runs[r]), std::get<1>(runs[r])};
    if (run_win) (*run_win)[r] = std::get<2>(runs[r]);
  }
  if (stats) {
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, ev.a, ev.b));
    stats->prefilter_ms += ms;
  }
  return FAC_OK;
}


// ---- Pre-filtered batches (fac.h fac_search_batch_prefiltered) -----------------------------------
// One pass over the batch's concatenated bytes gives every document its own merged bitap windows:
// the packed full scan resets its automaton at every document start (bitap_kernel<.., DOCS>), the
// q-gram verify takes the bounds of the candidate's document (qgram_verify_docs_kernel), both from
// the document-start bitmap, and the runs of the one coverage bitmap are cut at document starts
// (documents are disjoint, so no second bitmap and no window table). Runs are counted per bitmap
// word, scanned and written in place as segment descriptors, so they are sorted by start -- by
// document, then by start -- without a sort, and nothing per document or per run visits the host.
// A batch with non-ASCII documents (Batch::unicode_pf) is scanned in its start-window space instead:
// one symbol per byte of an ASCII document and per grapheme of any other (batch_symbol_ids_kernel),
// the document starts of that space (Batch::d_sstart), always in ids mode; its runs become byte or
// grapheme slices (runs_docs_write_mixed_kernel, slice_ascii_kernel). The scan, verify and count
// kernels are the same instantiations: they see ids, a start bitmap, a coverage bitmap and a length.
int batch_prefilter_windows(const Engine& e, const Batch& b, const std::vector<uint32_t>& ks, hipStream_t stream,
                            BatchWindows& out, fac_stats* stats, std::string& err) {
  HIP_TRY(hipSetDevice(e.device));
  if (!stream) stream = e.stream;
  const Haystack& h = b.h;
  // a batch with non-ASCII documents (opted in): the scan's positions are the batch's start windows
  const bool mixed = !h.ascii;
  const uint64_t n = mixed ? b.windows : h.len;
  out.s = stream;
  out.n = out.windows = 0;
  if (mixed && !b.unicode_pf) {
    err = "pre-filtered batches need an all-ASCII batch";
    return FAC_E_UNSUPPORTED;
  }
  if (n == 0 || b.n_segs == 0) return FAC_OK;
  const uint64_t n_words = (n + 31) / 32;
  {  // the document-start bitmap of the scan's positions, once per staging
    std::lock_guard<std::mutex> lk(b.dstart_mu);
    uint32_t*& d_bits = mixed ? b.d_sstart : b.d_dstart;
    uint64_t& cap = mixed ? b.sstart_cap : b.dstart_cap;
    bool& ready = mixed ? b.sstart_ready : b.dstart_ready;
    if (!ready) {
      if (cap < n_words) {
        if (d_bits) HIP_TRY(hipFree(d_bits));
        d_bits = nullptr;
        cap = 0;
        HIP_TRY(hipMalloc((void**)&d_bits, n_words * 4));
        cap = n_words;
      }
      HIP_TRY(hipMemsetAsync(d_bits, 0, n_words * 4, stream));
      if (mixed) {
        if (int rc = batch_symbol_starts_device(b, d_bits, stream, err)) return rc;
      } else {
        hipLaunchKernelGGL(doc_starts_kernel, dim3((uint32_t)((b.n_docs + 255) / 256)), dim3(256), 0, stream, b.d_offsets,
                           b.n_docs, d_bits);
        HIP_TRY(hipGetLastError());
      }
      HIP_TRY(hipStreamSynchronize(stream));  // (another stream's search may use it next)
      ready = true;
    }
  }
  const uint32_t* d_starts = mixed ? b.d_sstart : b.d_dstart;
  const uint8_t* vb = h.d_utf8;
  const bool want_bytes = !mixed && ((uintptr_t)h.d_utf8 & 15u) == 0 && !diag_env("FAC_QGRAM_IDS");
  const PfTables* T = nullptr;
  if (int rc = pf_tables(e, ks, want_bytes, T, err)) return rc;
  const uint32_t nw = T->nw;
  PoolBuf d_ids, d_cover, d_cnt, d_pos, d_lens;
  if (!T->bytes) {  // transcode (prefilter.rs:253-280): the symbol ids of every document
    HIP_TRY(d_ids.alloc(n + 80, stream));
    if (mixed) {
      if (int rc = batch_symbol_ids_device(e, b, static_cast<uint8_t*>(d_ids.p), stream, err)) return rc;
    } else {
      const uint64_t threads = (n + 15) / 16;
      hipLaunchKernelGGL(transcode_ascii_kernel, dim3((uint32_t)((threads + 255) / 256)), dim3(256), 0, stream, vb, n,
                         e.d_ascii_id, static_cast<uint8_t*>(d_ids.p));
      HIP_TRY(hipGetLastError());
    }
  }
  HIP_TRY(d_cover.alloc(n_words * 4, stream));
  HIP_TRY(hipMemsetAsync(d_cover.p, 0, n_words * 4, stream));
  Events ev;
  HIP_TRY(hipEventCreate(&ev.a));
  HIP_TRY(hipEventCreate(&ev.b));
  HIP_TRY(hipEventRecord(ev.a, stream));
  if (nw != 0) {
    BitapParams B{};
    B.ids = static_cast<const uint8_t*>(d_ids.p);
    B.n = n;
    B.mask_t = T->pmask;
    B.top = T->ptop;
    B.k = static_cast<const uint32_t*>(T->wk);
    B.n_words = nw;
    B.seg_len = 4096;
    B.cover = static_cast<uint32_t*>(d_cover.p);
    B.dstart = d_starts;
    const uint64_t waves = ((n + B.seg_len - 1) / B.seg_len) * ((nw + 63) / 64);
    launch_bitap<true>(*T, B, dim3((uint32_t)std::max<uint64_t>(1, (waves + 3) / 4)), stream);
    HIP_TRY(hipGetLastError());
  }
  QgramBufs qb;
  if (T->q) {
    QgramParams Q = qgram_params(e, h, *T, vb, d_ids.p, n, d_cover.p);
    Q.dstart = d_starts;
    dim3 vg;
    unsigned long long nc = 0;
    if (int rc = qgram_candidates(e, *T, Q, n, stream, qb, vg, nc, err)) return rc;
    launch_qverify<2>(*T, Q, vg, stream);
    HIP_TRY(hipGetLastError());
  }
  // runs: per-word counts, their scan (entry n_words: the total), then the descriptors in place
  const uint32_t* cov = static_cast<const uint32_t*>(d_cover.p);
  HIP_TRY(d_cnt.alloc((n_words + 1) * 8, stream));
  HIP_TRY(d_pos.alloc((n_words + 1) * 8, stream));
  hipLaunchKernelGGL(runs_docs_count_kernel, dim3((uint32_t)((n_words + 1 + 255) / 256)), dim3(256), 0, stream, cov,
                     d_starts, n_words, n, static_cast<uint64_t*>(d_cnt.p));
  HIP_TRY(hipGetLastError());
  if (int rc = exclusive_sum_u64(static_cast<const uint64_t*>(d_cnt.p), static_cast<uint64_t*>(d_pos.p), n_words + 1, stream, err))
    return rc;
  uint64_t n_runs = 0;
  HIP_TRY(hipMemcpyAsync(&n_runs, static_cast<uint64_t*>(d_pos.p) + n_words, 8, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  if (n_runs > 0xFFFFFFFFull) {
    err = "a pre-filtered batch holds at most 2^32 - 1 merged windows";
    return FAC_E_UNSUPPORTED;
  }
  uint64_t total = 0;
  if (n_runs) {
    hipError_t he = hipSuccess;
    out.d_segs = static_cast<SegDesc*>(call_scratch_take(n_runs * sizeof(SegDesc), stream, &he));
    HIP_TRY(he);
    out.d_prefix = static_cast<uint64_t*>(call_scratch_take((n_runs + 1) * 8, stream, &he));
    HIP_TRY(he);
    HIP_TRY(d_lens.alloc((n_runs + 1) * 8, stream));
    HIP_TRY(hipMemsetAsync(static_cast<uint64_t*>(d_lens.p) + n_runs, 0, 8, stream));
    if (mixed) {
      if (out.want_tri) {
        out.d_tri = static_cast<uint64_t*>(call_scratch_take(n_runs * 24, stream, &he));
        HIP_TRY(he);
      }
      hipLaunchKernelGGL(runs_docs_write_mixed_kernel, dim3((uint32_t)((n_words + 255) / 256)), dim3(256), 0, stream, cov,
                         d_starts, n_words, n, static_cast<const uint64_t*>(d_pos.p), h.d_off, b.d_segs, b.d_prefix, b.n_segs,
                         out.d_segs, static_cast<uint64_t*>(d_lens.p), out.d_tri);
      HIP_TRY(hipGetLastError());
      hipLaunchKernelGGL(slice_ascii_kernel, dim3((uint32_t)((n_runs + 3) / 4)), dim3(256), 0, stream, h.d_utf8, h.len,
                         out.d_segs, static_cast<uint64_t*>(d_lens.p), n_runs);
    } else {
      hipLaunchKernelGGL(runs_docs_write_kernel, dim3((uint32_t)((n_words + 255) / 256)), dim3(256), 0, stream, cov, d_starts,
                         n_words, n, static_cast<const uint64_t*>(d_pos.p), b.d_offsets, b.n_docs, out.d_segs,
                         static_cast<uint64_t*>(d_lens.p));
    }
    HIP_TRY(hipGetLastError());
    if (int rc = exclusive_sum_u64(static_cast<const uint64_t*>(d_lens.p), out.d_prefix, n_runs + 1, stream, err)) return rc;
    HIP_TRY(hipMemcpyAsync(&total, out.d_prefix + n_runs, 8, hipMemcpyDeviceToHost, stream));
  }
  HIP_TRY(hipEventRecord(ev.b, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  out.n = n_runs;
  out.windows = total;
  if (diag_env("FAC_RC_DEBUG"))
    std::fprintf(stderr, "FAC_BATCH_PF docs=%llu bytes=%llu full-scan words=%u qgram patterns=%zu/%zu bytes-mode=%d merged windows=%llu start windows=%llu unicode=%d symbols=%llu\n",
                 (unsigned long long)b.n_docs, (unsigned long long)h.len, nw, T->n_qpat, e.bp_m.size(), (int)T->bytes,
                 (unsigned long long)n_runs, (unsigned long long)total, (int)mixed, (unsigned long long)n);
  if (stats) {
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, ev.a, ev.b));
    stats->prefilter_ms += ms;
  }
  return FAC_OK;
}

}  // namespace fac
