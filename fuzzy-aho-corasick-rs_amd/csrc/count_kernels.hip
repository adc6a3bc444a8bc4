// count_kernels.hip — per-document term counts of a batch (fac.h "Term counts of a batch";
// DESIGN.md 6a "Term counts"): the applied records of a batch, grouped by document in HBM, are grouped
// again by key(pattern_index) inside every document. A record becomes the entry
//   (key, v = similarity order word << 32 | ~pattern_index)
// so that sorting a document's entries by (key, v) puts every key's records in one run whose LAST
// entry carries the greatest similarity under total_cmp and, among equal bits, the least pattern.
// A term is then (key, run length, the last entry's similarity bits and pattern): no segmented
// reduction is needed behind the sort.
// Documents are classified by their record count m_d (count_classify_kernel, ballot compaction into
// four lists):
//  - lane tier,  m_d <= lane_max (8): one lane per document, a compare-exchange network in registers;
//  - group tier, m_d <= group_max (2048), in two kernels: up to 64 records one wave per document with a
//    shuffle bitonic sort and no LDS (count_wave_kernel, four documents to a workgroup), above that
//    one workgroup of 256 per document with a bitonic sort in LDS (count_group_kernel);
//  - sorted tier, the rest: one rocPRIM merge sort of (document << 32 | key, v) entries of all such
//    documents, run heads by a scan.
// Pass 1 writes every document's distinct-key count, exclusive_sum_u64 makes the term index, pass 2
// writes each term as one 16-byte store (the lane and group tiers sort again; the sorted tier keeps
// its sorted entries). The totals are integer atomics, so nothing depends on arrival order.
#include <hip/hip_runtime.h>

#include <algorithm>

#include <rocprim/device/device_merge_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "fac_internal.h"
#include "host_util.h"
#include "wave_util.h"

namespace fac {
namespace {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kMaxBlocks = 2048;     // the rest of a large set is grid-strided
constexpr uint32_t kNoKey = 0xFFFFFFFFu;  // above every key (keys are < n_keys <= 2^32 - 1): pads a sort
constexpr uint32_t kGroupPer = kCountGroupMax / kThreads;  // sorted positions one thread of the group tier walks
constexpr uint32_t kHistChunk = 16 * kThreads;  // terms one workgroup adds to its LDS histogram (< 2^16)
constexpr uint32_t kHistSmall = 1u << 16;       // term counts below this go through the histogram: sums stay < 2^32
// counters of a call: documents per tier, records of the sorted tier, documents of 2^32 records or
// more, the sorted tier's fill cursor
enum { kCtrLane = 0, kCtrWave, kCtrGroup, kCtrSorted, kCtrSortedRecs, kCtrTooLarge, kCtrFill, kCtrWords = 8 };

static_assert(kCountLaneMax == 8, "count_lane_kernel's network holds 8 entries");
static_assert(kCountGroupMax % kThreads == 0 && (kCountGroupMax & (kCountGroupMax - 1)) == 0, "a power of two");
static_assert(kHistChunk <= kHistSmall, "a workgroup's histogram sums must fit 32 bits");

struct Entry {  // sorted tier
  uint64_t dk;  // document << 32 | key
  uint32_t ow, npat;
};
struct EntryLess {
  __host__ __device__ bool operator()(const Entry& a, const Entry& b) const {
    if (a.dk != b.dk) return a.dk < b.dk;
    if (a.ow != b.ow) return a.ow < b.ow;
    return a.npat < b.npat;
  }
};

// record i's entry: only the record's second half is read (pattern_index, similarity)
__device__ __forceinline__ void load_entry(const uint4* __restrict__ recs, uint64_t i, const uint32_t* __restrict__ keys,
                                           uint32_t& k, uint64_t& v) {
  const uint4 b = recs[2 * i + 1];
  k = keys ? keys[b.x] : b.x;
  v = ((uint64_t)total_key(__uint_as_float(b.y)) << 32) | (uint32_t)~b.x;
}

__device__ __forceinline__ uint4 make_term(uint32_t key, uint32_t count, uint64_t best) {
  return make_uint4(key, count, total_key_bits((uint32_t)(best >> 32)), ~(uint32_t)best);
}

// One thread per document: cnt[d] = 0, and d goes to the list of its tier (empty documents to none).
__global__ __launch_bounds__(kThreads) void count_classify_kernel(const uint64_t* __restrict__ d_doc, uint64_t n_docs,
                                                                  uint32_t lane_max, uint32_t group_max,
                                                                  uint32_t* __restrict__ lane, uint32_t* __restrict__ wave,
                                                                  uint32_t* __restrict__ group, uint32_t* __restrict__ sorted,
                                                                  uint64_t* __restrict__ cnt,
                                                                  unsigned long long* ctr) {
  const uint32_t l = lane_id();
  for (uint64_t base = (uint64_t)blockIdx.x * kThreads; base < n_docs; base += (uint64_t)gridDim.x * kThreads) {
    const uint64_t d = base + threadIdx.x;
    int tier = -1;
    if (d < n_docs) {
      const uint64_t m = d_doc[d + 1] - d_doc[d];
      cnt[d] = 0;
      if (d == 0) cnt[n_docs] = 0;
      if (m >> 32) atomicAdd(&ctr[kCtrTooLarge], 1ull);
      else if (m) tier = m <= lane_max ? 0 : m > group_max ? 3 : m <= 64 ? 1 : 2;
      if (tier == 3) atomicAdd(&ctr[kCtrSortedRecs], (unsigned long long)m);
    }
    for (int t = 0; t < 4; ++t) {
      const uint64_t mask = __ballot(tier == t);
      if (mask == 0) continue;  // wave-uniform
      unsigned long long at = 0;
      if (l == 0) at = atomicAdd(&ctr[t], (unsigned long long)__popcll(mask));
      at = shfl_u64(at, 0) + prefix_below(mask);
      if (tier == t) (t == 0 ? lane : t == 1 ? wave : t == 2 ? group : sorted)[at] = (uint32_t)d;
    }
  }
}

// Lane tier: one thread per listed document of 1..8 records. kWrite false: cnt[d] = distinct keys;
// true: the terms at term_off[d].
template <bool kWrite>
__global__ __launch_bounds__(kThreads) void count_lane_kernel(const uint4* __restrict__ recs, const uint64_t* __restrict__ d_doc,
                                                              const uint32_t* __restrict__ keys,
                                                              const uint32_t* __restrict__ list, uint64_t n_list,
                                                              uint64_t* __restrict__ cnt, const uint64_t* __restrict__ term_off,
                                                              uint4* __restrict__ terms) {
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n_list) return;
  const uint32_t d = list[i];
  const uint64_t lo = d_doc[d];
  const uint32_t m = (uint32_t)(d_doc[d + 1] - lo);
  uint32_t k[kCountLaneMax + 1];
  uint64_t v[kCountLaneMax];
#pragma unroll
  for (uint32_t j = 0; j < kCountLaneMax; ++j) {
    k[j] = kNoKey;
    v[j] = 0;
    if (j < m) load_entry(recs, lo + j, keys, k[j], v[j]);
  }
  k[kCountLaneMax] = kNoKey;
  // insertion sort by key as a fixed network (indices are compile-time: the arrays stay in registers)
#pragma unroll
  for (uint32_t a = 1; a < kCountLaneMax; ++a) {
#pragma unroll
    for (uint32_t b = a; b > 0; --b) {
      const bool sw = k[b - 1] > k[b];
      const uint32_t k0 = sw ? k[b] : k[b - 1], k1 = sw ? k[b - 1] : k[b];
      const uint64_t v0 = sw ? v[b] : v[b - 1], v1 = sw ? v[b - 1] : v[b];
      k[b - 1] = k0;
      k[b] = k1;
      v[b - 1] = v0;
      v[b] = v1;
    }
  }
  uint32_t nt = 0, run = 0;
  uint64_t best = 0;
  const uint64_t at = kWrite ? term_off[d] : 0;
#pragma unroll
  for (uint32_t j = 0; j < kCountLaneMax; ++j) {
    if (k[j] == kNoKey) continue;
    ++run;
    best = v[j] > best ? v[j] : best;
    if (k[j + 1] != k[j]) {
      if (kWrite) terms[at + nt] = make_term(k[j], run, best);
      ++nt;
      run = 0;
      best = 0;
    }
  }
  if (!kWrite) cnt[d] = nt;
}

__device__ __forceinline__ bool entry_less(uint32_t ka, uint64_t va, uint32_t kb, uint64_t vb) {
  return ka < kb || (ka == kb && va < vb);
}

// Group tier, documents of at most 64 records: one wave per listed document (four to a workgroup),
// one entry per lane, a bitonic sort by lane exchanges; no LDS.
template <bool kWrite>
__global__ __launch_bounds__(kThreads) void count_wave_kernel(const uint4* __restrict__ recs, const uint64_t* __restrict__ d_doc,
                                                              const uint32_t* __restrict__ keys,
                                                              const uint32_t* __restrict__ list, uint64_t n_list,
                                                              uint64_t* __restrict__ cnt, const uint64_t* __restrict__ term_off,
                                                              uint4* __restrict__ terms) {
  const uint64_t w = (uint64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  if (w >= n_list) return;  // (the whole wave)
  const uint32_t d = list[w];
  const uint64_t lo = d_doc[d];
  const uint32_t m = (uint32_t)(d_doc[d + 1] - lo);  // 1..64
  const uint32_t l = threadIdx.x & 63;
  uint32_t k = kNoKey;
  uint64_t v = ~0ull;
  if (l < m) load_entry(recs, lo + l, keys, k, v);
  for (uint32_t size = 2; size <= 64; size <<= 1) {
    for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
      const uint32_t pk = __shfl_xor(k, (int)stride);
      const uint64_t pv = __shfl_xor((unsigned long long)v, (int)stride);
      const bool keep_min = ((l & stride) == 0) == ((l & size) == 0);
      const bool take = keep_min ? entry_less(pk, pv, k, v) : entry_less(k, v, pk, pv);
      k = take ? pk : k;
      v = take ? pv : v;
    }
  }
  const uint32_t prev = __shfl_up(k, 1), next = __shfl_down(k, 1);
  const bool in = l < m;
  const bool head = in && (l == 0 || prev != k), tail = in && (l == m - 1 || next != k);
  const uint64_t heads = __ballot(head);
  if (!kWrite) {
    if (l == 0) cnt[d] = (uint64_t)__popcll(heads);
    return;
  }
  if (tail) {
    const uint64_t below = heads & ((2ull << l) - 1);  // (l == 63: every lane)
    const uint32_t r = (uint32_t)__popcll(below) - 1, first = 63u - (uint32_t)__clzll(below);
    terms[term_off[d] + r] = make_term(k, l - first + 1, v);
  }
}

// Group tier, documents of 65..kCountGroupMax records: one workgroup per listed document, a bitonic
// sort of P (a power of two >= m) entries in LDS.
// LDS: sk 8 KiB + sv 16 KiB + shead 8 KiB + swave 16 B = 32 KiB + 16 B.
template <bool kWrite>
__global__ __launch_bounds__(kThreads) void count_group_kernel(const uint4* __restrict__ recs, const uint64_t* __restrict__ d_doc,
                                                               const uint32_t* __restrict__ keys,
                                                               const uint32_t* __restrict__ list, uint64_t* __restrict__ cnt,
                                                               const uint64_t* __restrict__ term_off,
                                                               uint4* __restrict__ terms) {
  __shared__ uint32_t sk[kCountGroupMax];
  __shared__ uint64_t sv[kCountGroupMax];
  __shared__ uint32_t shead[kCountGroupMax];  // sorted position of every run's first entry
  __shared__ uint32_t swave[kThreads / 64];
  const uint32_t d = list[blockIdx.x];
  const uint64_t lo = d_doc[d];
  const uint32_t m = (uint32_t)(d_doc[d + 1] - lo);  // (block-uniform)
  const uint32_t tid = threadIdx.x;
  uint32_t P = 128;
  while (P < m) P <<= 1;
  for (uint32_t i = tid; i < P; i += kThreads) {
    uint32_t k = kNoKey;
    uint64_t v = ~0ull;
    if (i < m) load_entry(recs, lo + i, keys, k, v);
    sk[i] = k;
    sv[i] = v;
  }
  __syncthreads();
  for (uint32_t size = 2; size <= P; size <<= 1) {
    for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
      for (uint32_t t = tid; t < P / 2; t += kThreads) {
        const uint32_t i = ((t & ~(stride - 1)) << 1) | (t & (stride - 1)), j = i | stride;
        const uint32_t ki = sk[i], kj = sk[j];
        const uint64_t vi = sv[i], vj = sv[j];
        const bool up = (i & size) == 0;
        if (up ? entry_less(kj, vj, ki, vi) : entry_less(ki, vi, kj, vj)) {
          sk[i] = kj;
          sk[j] = ki;
          sv[i] = vj;
          sv[j] = vi;
        }
      }
      __syncthreads();
    }
  }
  // thread t walks sorted positions [t * kGroupPer, (t + 1) * kGroupPer): its run heads, then their
  // rank in the document by a block-wide prefix sum
  const uint32_t p0 = tid * kGroupPer;
  uint32_t mine = 0;
  for (uint32_t q = 0; q < kGroupPer; ++q) {
    const uint32_t i = p0 + q;
    if (i < m && (i == 0 || sk[i - 1] != sk[i])) ++mine;
  }
  const uint32_t incl = wave_inclusive_sum(mine);
  if ((tid & 63) == 63) swave[tid >> 6] = incl;
  __syncthreads();
  uint32_t before = incl - mine, total = 0;
  for (uint32_t w = 0; w < kThreads / 64; ++w) {
    if (w < (tid >> 6)) before += swave[w];
    total += swave[w];
  }
  if (!kWrite) {
    if (tid == 0) cnt[d] = total;
    return;
  }
  uint32_t r = before;
  for (uint32_t q = 0; q < kGroupPer; ++q) {
    const uint32_t i = p0 + q;
    if (i < m && (i == 0 || sk[i - 1] != sk[i])) shead[r++] = i;
  }
  __syncthreads();
  const uint64_t at = term_off[d];
  r = before;
  for (uint32_t q = 0; q < kGroupPer; ++q) {
    const uint32_t i = p0 + q;
    if (i >= m) break;
    if (i == 0 || sk[i - 1] != sk[i]) ++r;  // r - 1: the rank of the run position i lies in
    if (i == m - 1 || sk[i + 1] != sk[i]) terms[at + r - 1] = make_term(sk[i], i - shead[r - 1] + 1, sv[i]);
  }
}

// Sorted tier. One workgroup per listed document: its entries, tagged with the document, at a range of
// `out` drawn from the fill cursor (any order: the sort follows).
__global__ __launch_bounds__(kThreads) void count_fill_kernel(const uint4* __restrict__ recs, const uint64_t* __restrict__ d_doc,
                                                              const uint32_t* __restrict__ keys,
                                                              const uint32_t* __restrict__ list, Entry* __restrict__ out,
                                                              unsigned long long* ctr) {
  __shared__ unsigned long long sbase;
  const uint32_t d = list[blockIdx.x];
  const uint64_t lo = d_doc[d], m = d_doc[d + 1] - lo;
  if (threadIdx.x == 0) sbase = atomicAdd(&ctr[kCtrFill], (unsigned long long)m);
  __syncthreads();
  const uint64_t base = sbase;
  for (uint64_t i = threadIdx.x; i < m; i += kThreads) {
    uint32_t k;
    uint64_t v;
    load_entry(recs, lo + i, keys, k, v);
    out[base + i] = Entry{((uint64_t)d << 32) | k, (uint32_t)(v >> 32), (uint32_t)v};
  }
}

// flag[i] = 1 where sorted entry i starts a run of one (document, key)
__global__ __launch_bounds__(kThreads) void count_flags_kernel(const Entry* __restrict__ e, uint64_t n,
                                                               uint64_t* __restrict__ flag) {
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i < n) flag[i] = (i == 0 || e[i - 1].dk != e[i].dk) ? 1 : 0;
}

// hid: the inclusive scan of the flags (1-based run id). Per entry: a run's first entry records its
// position, a document's first entry the runs before the document, its last entry the document's
// run count (a document's m entries are contiguous).
__global__ __launch_bounds__(kThreads) void count_runs_kernel(const Entry* __restrict__ e, uint64_t n,
                                                              const uint64_t* __restrict__ hid,
                                                              const uint64_t* __restrict__ d_doc, uint64_t* __restrict__ hpos,
                                                              uint64_t* __restrict__ aux, uint64_t* __restrict__ cnt) {
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const uint64_t dk = e[i].dk, d = dk >> 32;
  const uint64_t pdk = i ? e[i - 1].dk : ~0ull, ndk = i + 1 < n ? e[i + 1].dk : ~0ull;
  if (i == 0 || pdk != dk) hpos[hid[i] - 1] = i;
  if (i == 0 || (pdk >> 32) != d) aux[d] = hid[i] - 1;
  if (i + 1 == n || (ndk >> 32) != d) {
    const uint64_t m = d_doc[d + 1] - d_doc[d];
    cnt[d] = hid[i] - hid[i - (m - 1)] + 1;
  }
}

// One thread per sorted entry: a run's last entry writes the run's term.
__global__ __launch_bounds__(kThreads) void count_sorted_write_kernel(const Entry* __restrict__ e, uint64_t n,
                                                                      const uint64_t* __restrict__ hid,
                                                                      const uint64_t* __restrict__ hpos,
                                                                      const uint64_t* __restrict__ aux,
                                                                      const uint64_t* __restrict__ term_off,
                                                                      uint4* __restrict__ terms) {
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const Entry x = e[i];
  if (i + 1 < n && e[i + 1].dk == x.dk) return;
  const uint64_t d = x.dk >> 32, g = hid[i] - 1;
  terms[term_off[d] + (g - aux[d])] =
      make_term((uint32_t)x.dk, (uint32_t)(i - hpos[g] + 1), ((uint64_t)x.ow << 32) | x.npat);
}

// Totals, n_keys <= kCountHistKeys: a (count, docs) pair of 32-bit bins per key in LDS (32 KiB at
// kCountHistKeys), one workgroup per kHistChunk terms, flushed with one 64-bit atomic per non-zero bin.
__global__ __launch_bounds__(kThreads) void count_totals_hist_kernel(const uint4* __restrict__ terms, uint64_t n,
                                                                     uint32_t n_keys, unsigned long long* totals) {
  __shared__ uint32_t h[2 * kCountHistKeys];
  for (uint32_t i = threadIdx.x; i < 2 * n_keys; i += kThreads) h[i] = 0;
  __syncthreads();
  const uint64_t base = (uint64_t)blockIdx.x * kHistChunk;
  for (uint32_t j = 0; j < kHistChunk / kThreads; ++j) {
    const uint64_t i = base + (uint64_t)j * kThreads + threadIdx.x;
    if (i >= n) break;
    const uint4 t = terms[i];
    if (t.y < kHistSmall) {
      atomicAdd(&h[2 * t.x], t.y);
      atomicAdd(&h[2 * t.x + 1], 1u);
    } else {  // (a count that could overflow the 32-bit bin)
      atomicAdd(&totals[2 * (uint64_t)t.x], (unsigned long long)t.y);
      atomicAdd(&totals[2 * (uint64_t)t.x + 1], 1ull);
    }
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < 2 * n_keys; i += kThreads)
    if (h[i]) atomicAdd(&totals[i], (unsigned long long)h[i]);
}

// Totals, any n_keys: 64-bit global atomics, after lanes with equal neighbouring keys (hot keys of
// neighbouring documents; a document's own keys are distinct) are merged inside the wave.
__global__ __launch_bounds__(kThreads) void count_totals_direct_kernel(const uint4* __restrict__ terms, uint64_t n,
                                                                       unsigned long long* totals) {
  const uint32_t l = lane_id();
  for (uint64_t base = (uint64_t)blockIdx.x * kThreads; base < n; base += (uint64_t)gridDim.x * kThreads) {
    const uint64_t i = base + threadIdx.x;
    uint32_t key = kNoKey;
    unsigned long long x = 0;
    if (i < n) {
      const uint4 t = terms[i];
      key = t.x;
      x = t.y;
    }
    const unsigned long long own = x;
    const uint32_t prev = __shfl_up(key, 1);
    const bool head = l == 0 || prev != key;
    const uint64_t heads = __ballot(head);
    for (uint32_t o = 1; o < 64; o <<= 1) {  // inclusive sum of the counts over the wave
      const unsigned long long y = __shfl_up(x, o);
      if (l >= o) x += y;
    }
    const uint64_t above = heads & ~((2ull << l) - 1);  // (l == 63: none)
    const uint32_t last = above ? (uint32_t)__builtin_ctzll(above) - 1 : 63u;  // the run's last lane
    const unsigned long long xe = __shfl(x, (int)last);
    if (head && i < n) {
      atomicAdd(&totals[2 * (uint64_t)key], xe - x + own);
      atomicAdd(&totals[2 * (uint64_t)key + 1], (unsigned long long)(last - l + 1));
    }
  }
}

int plan_take(CountPlan& plan, int slot, size_t bytes, void** p, std::string& err) {
  hipError_t he = hipSuccess;
  plan.mem[slot] = call_scratch_take(std::max<size_t>(bytes, 16), plan.s, &he);
  if (he != hipSuccess) {
    plan.mem[slot] = nullptr;
    err = std::string("hipMalloc: ") + hipGetErrorString(he);
    return FAC_E_OOM;
  }
  *p = plan.mem[slot];
  return FAC_OK;
}

inline uint32_t blocks_for(uint64_t n) { return (uint32_t)((n + kThreads - 1) / kThreads); }

// The sorted tier's pass 1: entries, sort, run ids, run heads, per-document counts.
int sorted_prepare(CountPlan& plan, uint64_t* d_cnt, unsigned long long* d_ctr, std::string& err) {
  const uint64_t n = plan.sorted_recs;
  hipStream_t s = plan.s;
  void* p = nullptr;
  if (int rc = plan_take(plan, 5, 2 * n * sizeof(Entry), &p, err)) return rc;
  Entry *e_in = static_cast<Entry*>(p), *e_out = e_in + n;
  if (int rc = plan_take(plan, 6, (n + plan.n_docs) * 8, &p, err)) return rc;
  plan.d_hid = static_cast<uint64_t*>(p);
  plan.d_aux = plan.d_hid + n;
  hipLaunchKernelGGL(count_fill_kernel, dim3((uint32_t)plan.n_sorted), dim3(kThreads), 0, s,
                     reinterpret_cast<const uint4*>(plan.d_recs), plan.d_doc, plan.d_keys, plan.d_sorted, e_in, d_ctr);
  HIP_TRY(hipGetLastError());
  {
    size_t bytes = 0;
    HIP_TRY(rocprim::merge_sort(nullptr, bytes, e_in, e_out, n, EntryLess(), s));
    PoolBuf tmp;
    HIP_TRY(tmp.alloc(bytes, s));
    HIP_TRY(rocprim::merge_sort(tmp.p, bytes, e_in, e_out, n, EntryLess(), s));
  }
  // the unsorted half is free again: the flags, then the run heads
  uint64_t* flag = reinterpret_cast<uint64_t*>(e_in);
  plan.d_hpos = flag + n;
  plan.d_entries = e_out;
  hipLaunchKernelGGL(count_flags_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, s, e_out, n, flag);
  HIP_TRY(hipGetLastError());
  {
    size_t bytes = 0;
    HIP_TRY(rocprim::inclusive_scan(nullptr, bytes, flag, plan.d_hid, n, rocprim::plus<uint64_t>(), s));
    PoolBuf tmp;
    HIP_TRY(tmp.alloc(bytes, s));
    HIP_TRY(rocprim::inclusive_scan(tmp.p, bytes, flag, plan.d_hid, n, rocprim::plus<uint64_t>(), s));
  }
  hipLaunchKernelGGL(count_runs_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, s, e_out, n, plan.d_hid, plan.d_doc,
                     plan.d_hpos, plan.d_aux, d_cnt);
  HIP_TRY(hipGetLastError());
  return FAC_OK;
}

}  // namespace

int count_plan_device(const fac_match* d_recs, const uint64_t* d_doc, uint64_t n_docs, const uint32_t* keys,
                      uint64_t n_patterns, uint32_t lane_max, uint32_t group_max, hipStream_t s, CountPlan& plan,
                      std::string& err) {
  plan.s = s;
  plan.d_recs = d_recs;
  plan.d_doc = d_doc;
  plan.n_docs = n_docs;
  plan.lane_max = std::min(lane_max ? lane_max : kCountLaneMax, kCountLaneMax);
  plan.group_max = std::min(group_max ? group_max : kCountGroupMax, kCountGroupMax);
  plan.total = 0;
  void* p = nullptr;
  if (int rc = plan_take(plan, 1, (n_docs + 1) * 8, &p, err)) return rc;
  plan.d_term_off = static_cast<uint64_t*>(p);
  if (n_docs == 0) {
    HIP_TRY(hipMemsetAsync(plan.d_term_off, 0, 8, s));
    return FAC_OK;
  }
  if (int rc = plan_take(plan, 0, (n_docs + 1) * 8, &p, err)) return rc;
  uint64_t* d_cnt = static_cast<uint64_t*>(p);
  if (int rc = plan_take(plan, 2, 4 * n_docs * 4, &p, err)) return rc;
  plan.d_lane = static_cast<uint32_t*>(p);
  plan.d_wave = plan.d_lane + n_docs;
  plan.d_group = plan.d_wave + n_docs;
  plan.d_sorted = plan.d_group + n_docs;
  if (int rc = plan_take(plan, 3, kCtrWords * 8, &p, err)) return rc;
  unsigned long long* d_ctr = static_cast<unsigned long long*>(p);
  if (keys) {
    if (int rc = plan_take(plan, 4, n_patterns * 4, &p, err)) return rc;
    HIP_TRY(hipMemcpyAsync(p, keys, n_patterns * 4, hipMemcpyHostToDevice, s));
    plan.d_keys = static_cast<const uint32_t*>(p);
  }
  HIP_TRY(hipMemsetAsync(d_ctr, 0, kCtrWords * 8, s));
  hipLaunchKernelGGL(count_classify_kernel, dim3(std::min(blocks_for(n_docs), kMaxBlocks)), dim3(kThreads), 0, s, d_doc, n_docs,
                     plan.lane_max, plan.group_max, plan.d_lane, plan.d_wave, plan.d_group, plan.d_sorted, d_cnt, d_ctr);
  HIP_TRY(hipGetLastError());
  unsigned long long ctr[kCtrWords] = {};
  HIP_TRY(hipMemcpyAsync(ctr, d_ctr, sizeof(ctr), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (ctr[kCtrTooLarge]) {
    err = "a document has 2^32 or more kept records";
    return FAC_E_UNSUPPORTED;
  }
  plan.n_lane = ctr[kCtrLane];
  plan.n_wave = ctr[kCtrWave];
  plan.n_group = ctr[kCtrGroup];
  plan.n_sorted = ctr[kCtrSorted];
  plan.sorted_recs = ctr[kCtrSortedRecs];
  const uint4* recs = reinterpret_cast<const uint4*>(d_recs);
  if (plan.n_lane) {
    hipLaunchKernelGGL((count_lane_kernel<false>), dim3(blocks_for(plan.n_lane)), dim3(kThreads), 0, s, recs, d_doc, plan.d_keys,
                       plan.d_lane, plan.n_lane, d_cnt, nullptr, nullptr);
    HIP_TRY(hipGetLastError());
  }
  if (plan.n_wave) {
    hipLaunchKernelGGL((count_wave_kernel<false>), dim3((uint32_t)((plan.n_wave + 3) / 4)), dim3(kThreads), 0, s, recs, d_doc,
                       plan.d_keys, plan.d_wave, plan.n_wave, d_cnt, nullptr, nullptr);
    HIP_TRY(hipGetLastError());
  }
  if (plan.n_group) {
    hipLaunchKernelGGL((count_group_kernel<false>), dim3((uint32_t)plan.n_group), dim3(kThreads), 0, s, recs, d_doc, plan.d_keys,
                       plan.d_group, d_cnt, nullptr, nullptr);
    HIP_TRY(hipGetLastError());
  }
  if (plan.n_sorted)
    if (int rc = sorted_prepare(plan, d_cnt, d_ctr, err)) return rc;
  if (int rc = exclusive_sum_u64(d_cnt, plan.d_term_off, n_docs + 1, s, err)) return rc;
  uint64_t total = 0;
  HIP_TRY(hipMemcpyAsync(&total, plan.d_term_off + n_docs, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  plan.total = total;
  return FAC_OK;
}

int count_write_device(const CountPlan& plan, fac_term* d_terms, std::string& err) {
  if (plan.total == 0) return FAC_OK;
  hipStream_t s = plan.s;
  const uint4* recs = reinterpret_cast<const uint4*>(plan.d_recs);
  uint4* terms = reinterpret_cast<uint4*>(d_terms);
  if (plan.n_lane) {
    hipLaunchKernelGGL((count_lane_kernel<true>), dim3(blocks_for(plan.n_lane)), dim3(kThreads), 0, s, recs, plan.d_doc,
                       plan.d_keys, plan.d_lane, plan.n_lane, nullptr, plan.d_term_off, terms);
    HIP_TRY(hipGetLastError());
  }
  if (plan.n_wave) {
    hipLaunchKernelGGL((count_wave_kernel<true>), dim3((uint32_t)((plan.n_wave + 3) / 4)), dim3(kThreads), 0, s, recs, plan.d_doc,
                       plan.d_keys, plan.d_wave, plan.n_wave, nullptr, plan.d_term_off, terms);
    HIP_TRY(hipGetLastError());
  }
  if (plan.n_group) {
    hipLaunchKernelGGL((count_group_kernel<true>), dim3((uint32_t)plan.n_group), dim3(kThreads), 0, s, recs, plan.d_doc,
                       plan.d_keys, plan.d_group, nullptr, plan.d_term_off, terms);
    HIP_TRY(hipGetLastError());
  }
  if (plan.n_sorted) {
    hipLaunchKernelGGL(count_sorted_write_kernel, dim3(blocks_for(plan.sorted_recs)), dim3(kThreads), 0, s,
                       static_cast<const Entry*>(plan.d_entries), plan.sorted_recs, plan.d_hid, plan.d_hpos, plan.d_aux,
                       plan.d_term_off, terms);
    HIP_TRY(hipGetLastError());
  }
  return FAC_OK;
}

int count_totals_device(const fac_term* d_terms, uint64_t n_terms, uint64_t n_keys, fac_term_total* d_totals, hipStream_t s,
                        std::string& err) {
  if (n_keys == 0) return FAC_OK;
  HIP_TRY(hipMemsetAsync(d_totals, 0, n_keys * sizeof(fac_term_total), s));
  if (n_terms == 0) return FAC_OK;
  const uint4* terms = reinterpret_cast<const uint4*>(d_terms);
  unsigned long long* tot = reinterpret_cast<unsigned long long*>(d_totals);
  if (n_keys <= kCountHistKeys)
    hipLaunchKernelGGL(count_totals_hist_kernel, dim3((uint32_t)((n_terms + kHistChunk - 1) / kHistChunk)), dim3(kThreads), 0, s,
                       terms, n_terms, (uint32_t)n_keys, tot);
  else
    hipLaunchKernelGGL(count_totals_direct_kernel, dim3(std::min(blocks_for(n_terms), kMaxBlocks)), dim3(kThreads), 0, s, terms,
                       n_terms, tot);
  HIP_TRY(hipGetLastError());
  return FAC_OK;
}

void count_records_host(const fac_match* recs, uint64_t n, const uint32_t* keys, std::vector<fac_term>& out) {
  std::vector<std::pair<uint32_t, uint64_t>> e(n);
  for (uint64_t i = 0; i < n; ++i) {
    const uint32_t p = recs[i].pattern_index;
    e[i] = {keys ? keys[p] : p, ((uint64_t)total_key_host(recs[i].similarity) << 32) | (uint32_t)~p};
  }
  std::sort(e.begin(), e.end());
  out.clear();
  for (uint64_t i = 0, first = 0; i < n; ++i) {
    if (i + 1 < n && e[i + 1].first == e[i].first) continue;
    fac_term t;
    t.key = e[i].first;
    t.count = (uint32_t)(i - first + 1);
    const uint32_t bits = total_key_bits((uint32_t)(e[i].second >> 32));
    std::memcpy(&t.best_similarity, &bits, 4);
    t.best_pattern = ~(uint32_t)e[i].second;
    out.push_back(t);
    first = i + 1;
  }
}

}  // namespace fac
