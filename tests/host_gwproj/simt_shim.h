// TEST-ONLY: just enough of the HIP programming model on the CPU to run siddhi_amd/csrc/gw_proj.h under the host
// sanitizers.  A launch runs the grid's workgroups one after the other; a workgroup is blockDim.x host threads with a
// pthread barrier for __syncthreads and one per wave of 64 for the shuffles (which every lane of a wave must reach
// together, as on the GPU).  `__shared__` variables are function-local statics, dynamic LDS is a heap block of exactly
// the launch's size, so an access past either is the sanitizer's to report.
#pragma once
#include <pthread.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <thread>
#include <vector>

#define __host__
#define __device__
#define __global__
#define __forceinline__ inline
#define __launch_bounds__(...)
#define __shared__ static

struct dim3 {
  unsigned x, y, z;
  dim3(unsigned x_ = 1, unsigned y_ = 1, unsigned z_ = 1) : x(x_), y(y_), z(z_) {}
};
typedef void* hipStream_t;
typedef int hipError_t;
static const hipError_t hipSuccess = 0;
enum { hipFuncAttributeMaxDynamicSharedMemorySize = 8 };
static inline hipError_t hipGetLastError() { return hipSuccess; }
static inline hipError_t hipFuncSetAttribute(const void*, int, int) { return hipSuccess; }
#define HIPCHK(x)                                 \
  do {                                            \
    if ((x) != hipSuccess) {                      \
      fprintf(stderr, "HIPCHK failed: %s\n", #x); \
      abort();                                    \
    }                                             \
  } while (0)

static thread_local dim3 threadIdx(0), blockIdx(0);

struct SimtBlock {
  pthread_barrier_t all;
  pthread_barrier_t wave[16];
  unsigned long long xch[1024];
  char* dyn = nullptr;
};
static SimtBlock simt_blk;

static inline void __syncthreads() { pthread_barrier_wait(&simt_blk.all); }
// lane `src` of the caller's wave hands its `v` to the caller
static inline unsigned long long simt_shfl(unsigned long long v, unsigned src) {
  const unsigned t = threadIdx.x, w = t >> 6;
  simt_blk.xch[t] = v;
  pthread_barrier_wait(&simt_blk.wave[w]);
  const unsigned long long r = simt_blk.xch[(w << 6) + (src & 63u)];
  pthread_barrier_wait(&simt_blk.wave[w]);
  return r;
}
static inline int __shfl_xor(int v, int o) { return (int)(unsigned)simt_shfl((unsigned)v, (threadIdx.x & 63u) ^ (unsigned)o); }
static inline unsigned long long __shfl_up(unsigned long long v, int o) {
  const unsigned lane = threadIdx.x & 63u;
  return simt_shfl(v, lane >= (unsigned)o ? lane - (unsigned)o : lane);
}
static inline uint32_t atomicAdd(uint32_t* p, uint32_t v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
#define GW_DYN_LDS(name) char* name = simt_blk.dyn

static inline void simt_launch(dim3 grid, dim3 block, size_t lds, const std::function<void()>& kernel) {
  if (block.x % 64 || block.x > 1024) abort();
  pthread_barrier_init(&simt_blk.all, nullptr, block.x);
  for (unsigned w = 0; w < block.x / 64; ++w) pthread_barrier_init(&simt_blk.wave[w], nullptr, 64);
  simt_blk.dyn = lds ? new char[lds] : nullptr;
  std::vector<std::thread> th;
  for (unsigned t = 0; t < block.x; ++t)
    th.emplace_back([&, t] {
      for (unsigned b = 0; b < grid.x; ++b) {
        threadIdx = dim3(t);
        blockIdx = dim3(b);
        kernel();
        pthread_barrier_wait(&simt_blk.all);   // the statics are the next workgroup's LDS
      }
    });
  for (auto& x : th) x.join();
  delete[] simt_blk.dyn;
  simt_blk.dyn = nullptr;
  pthread_barrier_destroy(&simt_blk.all);
  for (unsigned w = 0; w < block.x / 64; ++w) pthread_barrier_destroy(&simt_blk.wave[w]);
}
#define hipLaunchKernelGGL(kern, grid, block, lds, st, ...) simt_launch((grid), (block), (lds), [&] { kern(__VA_ARGS__); })
