// host_util.h — host-side HIP utilities shared by every kernel file and the staging code: the
// error-return macro, table uploads and the RAII scratch buffers.
#pragma once
#include <algorithm>

#include "fac_internal.h"

// for functions that return a FAC_* code and have a std::string `err` in scope
#define HIP_TRY(x)                                          \
  do {                                                      \
    hipError_t _e = (x);                                    \
    if (_e != hipSuccess) {                                 \
      err = std::string(#x) + ": " + hipGetErrorString(_e); \
      return FAC_E_HIP;                                     \
    }                                                       \
  } while (0)

namespace fac {

inline size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

template <typename T>
int upload(const std::vector<T>& v, T** d, std::string& err) {
  *d = nullptr;
  const size_t bytes = std::max<size_t>(v.size() * sizeof(T), 16);
  HIP_TRY(hipMalloc((void**)d, bytes));
  if (!v.empty()) HIP_TRY(hipMemcpy(*d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  return FAC_OK;
}

// One pinned, device-mapped host word per host thread (kept for the thread's lifetime): kernels
// store small results there directly, with no copy to queue behind other streams' work.
int pinned_word(unsigned int*& host, unsigned int*& dev, std::string& err);

// RAII scratch. Plain hipMalloc/hipFree: with the stream-ordered pool (hipMallocAsync /
// hipFreeAsync) on ROCm 7.2 the match counter of a recycled block intermittently came back short
// (reproduced 6/60 calls; 0/60 with hipMalloc), so the pool is not used.
struct DevBuf {
  void* p = nullptr;
  hipStream_t s = nullptr;
  void** slot = nullptr;  // engine scratch slot (kept across calls) or null (owned, freed here)
  size_t* slot_n = nullptr;
  ~DevBuf() { release(); }
  void bind(void** sp, size_t* sn) {
    slot = sp;
    slot_n = sn;
  }
  void release() {
    if (!p) return;
    if (slot) {  // the engine keeps it; the next user orders after us on its own stream
      (void)hipStreamSynchronize(s);
      p = nullptr;
      return;
    }
    (void)hipStreamSynchronize(s);
    (void)hipFree(p);
    p = nullptr;
  }
  hipError_t alloc(size_t bytes, hipStream_t stream) {
    bytes = std::max<size_t>(bytes, 16);
    if (slot) {
      p = nullptr;
      s = stream;
      if (*slot_n < bytes) {
        if (*slot) {
          (void)hipStreamSynchronize(stream);
          (void)hipFree(*slot);
          *slot = nullptr;
          *slot_n = 0;
        }
        const size_t want = bytes + bytes / 4;
        const hipError_t err = hipMalloc(slot, want);
        if (err != hipSuccess) return err;
        *slot_n = want;
      }
      p = *slot;
      return hipSuccess;
    }
    release();
    s = stream;
    return hipMalloc(&p, bytes);
  }
};

// Stream-ordered call scratch (call_scratch_take / give, pooled per thread and size class): the
// pre-filter's per-call buffers -- hipMalloc + hipFree of C5's 0.5 GB candidate list and 134 MB
// coverage bitmap per stream window stalled the device ~0.5 ms a window
struct PoolBuf {
  void* p = nullptr;
  hipStream_t s = nullptr;
  ~PoolBuf() {
    if (p) call_scratch_give(p, s);
  }
  hipError_t alloc(size_t bytes, hipStream_t stream) {
    if (p) call_scratch_give(p, s);
    s = stream;
    hipError_t e = hipSuccess;
    p = call_scratch_take(std::max<size_t>(bytes, 16), stream, &e);
    return e;
  }
};

struct Events {
  hipEvent_t a = nullptr, b = nullptr;
  ~Events() {
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
  }
};

}  // namespace fac
