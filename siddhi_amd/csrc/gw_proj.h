// gw_proj.h -- the group walker's delivery side (gwalk.h): the trigger-word format, the per-tile match counts
// (k_gtile_count) and the projection of a push's matches into output records (k_gscan_project), with their launches.
// Nothing here knows the engine: the launches take raw device pointers, so tests/host_gwproj compiles this file for
// the CPU (SG_HOST_ONLY: a workgroup is 256 host threads) and runs it under the address and undefined-behaviour
// sanitizers.
#pragma once
#ifndef SG_HOST_ONLY
#include <hip/hip_runtime.h>

#include "sg_engine.h"
#define GW_DYN_LDS(name) extern __shared__ __attribute__((aligned(16))) char name[]
#endif
#include <algorithm>
#include <cstdint>
#include <cstdlib>

#include "../../include/siddhi_gpu.h"

// Trigger word: unit (32) | matches (24) | epoch (8).  The buffer is not cleared per push: a word counts only when
// its epoch is the push's (run_group_walk hands the epochs out and clears what could hold anything else).
static const uint32_t GW_MATCH_MAX = (1u << 24) - 1;
__device__ __forceinline__ uint64_t gw_trig_word(uint64_t unit, uint32_t m, uint32_t epoch) {
  return unit | ((uint64_t)m << 32) | ((uint64_t)epoch << 56);
}
// matches of a trigger word under `epoch` (0: the row triggered nothing in this push)
__device__ __forceinline__ uint32_t gw_trig_matches(uint64_t w, uint32_t epoch) {
  return (uint32_t)(w >> 56) == epoch ? (uint32_t)(w >> 32) & GW_MATCH_MAX : 0u;
}

// Output records in delivery order (trigger order = arrival order).  A trigger's matches are read from its header in
// the match area (one 16-byte header + 8 bytes per match, contiguous) and assembled in LDS at their position inside
// the tile's output range, which is then stored contiguously (whole lines, 16-byte stores by consecutive threads); a
// tile that delivers more than GW_PROJ_S records does it in rounds.
struct GwSel {
  int32_t n_select, stride, multi, b_slot, pzero, vfloat;
  uint32_t nmask;      // null-mask bits of the record: the columns of code 4
  uint32_t pad;
  uint64_t codes[2];   // 4 bits per select column: 0 e1 payload, 1 e1 value, 2 e2 value, 3 e2 payload, 4 null
};
static_assert(SG_MAX_SELECT <= 32, "GwSel packs 32 select codes");
static const int GW_PROJ_S = 256;   // records staged per round
static const int GW_PROJ_RPT = 2;   // rows per projection thread: 1, 2 or 4 (a tile is 256 times that)
static const int GW_COUNT_ROWS = 2048;   // trigger words per workgroup of k_gtile_count
static const int GW_AREA_PAD = 2;   // units behind the match area: the projection reads two entries with every header

typedef uint64_t GwW2 __attribute__((ext_vector_type(2)));   // two trigger words: one 16-byte load

// trigger words of rows r, r + 1 (r even: the workspace base is 16-byte aligned) as one 16-byte load; the batch's
// last, single row as one word; rows from n on read as no trigger
__device__ __forceinline__ GwW2 gw_load_words2(const uint64_t* __restrict__ trig, int64_t r, int64_t n) {
  GwW2 w = {0ull, 0ull};
  if (r + 1 < n) w = __builtin_nontemporal_load((const GwW2*)(trig + r));
  else if (r < n) w.x = __builtin_nontemporal_load(trig + r);
  return w;
}

// matches per tile of `1 << lg_tile` rows (a multiple of 256 and at most GW_COUNT_ROWS: the projection's tile, its
// bases come from a scan over these).  A workgroup takes GW_COUNT_ROWS consecutive words, 16 bytes per lane and load,
// four loads in flight; a wave's 128 rows of one load lie in one tile.
static __global__ void __launch_bounds__(256) k_gtile_count(int64_t n, const uint64_t* __restrict__ trig, uint32_t epoch,
                                                            uint32_t* __restrict__ tcount, int64_t ntile, uint32_t lg_tile) {
  __shared__ uint32_t red[GW_COUNT_ROWS / 256];
  const uint32_t t = threadIdx.x, lane = t & 63;
  const int64_t r0 = (int64_t)blockIdx.x * GW_COUNT_ROWS;
  if (t < GW_COUNT_ROWS / 256) red[t] = 0;
  __syncthreads();
  GwW2 w[GW_COUNT_ROWS / 512];
#pragma unroll
  for (int j = 0; j < GW_COUNT_ROWS / 512; ++j) w[j] = gw_load_words2(trig, r0 + j * 512 + 2 * t, n);
#pragma unroll
  for (int j = 0; j < GW_COUNT_ROWS / 512; ++j) {
    uint32_t c = gw_trig_matches(w[j].x, epoch) + gw_trig_matches(w[j].y, epoch);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += (uint32_t)__shfl_xor((int)c, o);
    if (lane == 0 && c) atomicAdd(&red[(uint32_t)(j * 512 + 2 * (t - lane)) >> lg_tile], c);
  }
  __syncthreads();
  const uint32_t per = (uint32_t)GW_COUNT_ROWS >> lg_tile;   // tiles of this workgroup
  if (t < per) {
    const int64_t tile = (int64_t)blockIdx.x * per + t;
    if (tile < ntile) tcount[tile] = red[t];
  }
}

// (triggers, matches) of a thread's rows scanned over the workgroup in one pass: triggers in the high word, matches
// in the low one (a tile's matches are part of the push's 32-bit total)
__device__ __forceinline__ uint64_t gw_excl_scan256_pair(uint64_t x, uint64_t* wsum) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint64_t inc = x;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint64_t y = (uint64_t)__shfl_up((unsigned long long)inc, o);
    if (lane >= o) inc += y;
  }
  if (lane == 63) wsum[w] = inc;
  __syncthreads();
  uint64_t add = 0;
  for (int i = 0; i < w; ++i) add += wsum[i];
  return add + inc - x;
}

// Output records: one workgroup per tile of 256 * RPT arrival rows.  Thread t reads the trigger words of rows
// t * RPT .. t * RPT + RPT - 1 (16-byte loads); a block scan over (triggers, matches) places the tile's triggers, in
// arrival order, in a compact list in LDS: match-area unit, matches, first output slot inside the tile, in-tile row.
// Then thread t takes list entries t, t + 256, ... -- every lane has a trigger while the list lasts, whatever share
// of the rows trigger -- and issues all their reads before it uses one: the 16-byte header and the 16 bytes behind it,
// which are the first two entries (a trigger of one match reads a unit it does not use; the key's region, or the pad
// behind the area, holds it).  Only a trigger of three or more matches reads further entries, one by one.  The tile's
// first output slot comes from the scanned tile counts; the records are assembled in LDS in slot order and stored
// contiguously (GW_PROJ_S records per round).  Dynamic LDS: the list (256 * RPT entries of 16 bytes) and, in its
// place once the entries are in registers, the stage -- the larger of the two, since the kernel's time follows the
// workgroups resident per CU (profiles/r09/gw_project_loads.md).
template <int RPT>
static __global__ void __launch_bounds__(256) k_gscan_project(int64_t n, int64_t t0, uint64_t base_index,
                                                              const uint64_t* __restrict__ index,
                                                              const uint64_t* __restrict__ trig, uint32_t epoch,
                                                              const uint64_t* __restrict__ area, GwSel sel,
                                                              int64_t out_base, char* __restrict__ out,
                                                              const uint32_t* __restrict__ tbase) {
  typedef uint32_t U4 __attribute__((ext_vector_type(4)));
  GW_DYN_LDS(lds_proj);
  __shared__ uint64_t wsum[4];
  U4* list = (U4*)lds_proj;
  char* stage = lds_proj;   // (over the list, once every thread holds its entries in registers)
  const uint32_t t = threadIdx.x;
  const int64_t tile0 = (int64_t)blockIdx.x * (256 * RPT);
  uint64_t tw[RPT];
  if constexpr (RPT == 1) {
    tw[0] = tile0 + t < n ? __builtin_nontemporal_load(trig + tile0 + t) : 0ull;
  } else {
#pragma unroll
    for (int s = 0; s < RPT; s += 2) {
      const GwW2 w = gw_load_words2(trig, tile0 + (int64_t)t * RPT + s, n);
      tw[s] = w.x;
      tw[s + 1] = w.y;
    }
  }
  uint32_t cnt = 0, sum = 0;
#pragma unroll
  for (int s = 0; s < RPT; ++s) {
    const uint32_t m = gw_trig_matches(tw[s], epoch);
    cnt += m ? 1u : 0u;
    sum += m;
  }
  const uint64_t ex = gw_excl_scan256_pair(((uint64_t)cnt << 32) | sum, wsum);
  const uint64_t all = wsum[0] + wsum[1] + wsum[2] + wsum[3];
  {
    uint32_t li = (uint32_t)(ex >> 32), slot = (uint32_t)ex;
#pragma unroll
    for (int s = 0; s < RPT; ++s) {
      const uint32_t m = gw_trig_matches(tw[s], epoch);
      if (m) {
        const U4 ent = {(uint32_t)tw[s], m, slot, t * RPT + s};
        list[li++] = ent;
        slot += m;
      }
    }
  }
  __syncthreads();
  const uint32_t ntrig = (uint32_t)(all >> 32);
  const uint32_t pre = tbase[blockIdx.x];
  const uint32_t o_lo = pre, o_hi = pre + (uint32_t)all;
  // this thread's triggers: everything read from HBM for them is in flight before the first use
  uint32_t u[RPT], m[RPT], o[RPT];
  uint64_t h0[RPT], h1[RPT], e0[RPT], e1[RPT], tg[RPT];
#pragma unroll
  for (int s = 0; s < RPT; ++s) {
    const uint32_t i = t + 256 * s;
    m[s] = 0;
    u[s] = o[s] = 0;
    h0[s] = h1[s] = e0[s] = e1[s] = tg[s] = 0;
    if (i < ntrig) {
      const U4 ent = list[i];
      u[s] = ent.x;
      m[s] = ent.y;
      o[s] = pre + ent.z;
      const int64_t b = tile0 + ent.w;
      const uint64_t* a = area + (uint64_t)ent.x;
      h0[s] = a[0];
      h1[s] = a[1];
      e0[s] = a[2];
      e1[s] = a[3];
      tg[s] = index ? index[b] : base_index + (uint64_t)b;
    }
  }
  __syncthreads();   // the list has been read: the stage takes its place
  auto wid = [&](uint32_t bits, bool zero) { return zero ? (int64_t)bits : (int64_t)(int32_t)bits; };
  // (the select codes and the null mask come packed in registers: nothing is read from the arguments per match)
  const uint64_t cw0 = sel.codes[0], cw1 = sel.codes[1];
  const int nsel = sel.n_select;
  const int64_t nmask = (int64_t)sel.nmask;
  for (uint32_t sub = o_lo; sub < o_hi; sub += GW_PROJ_S) {
    const uint32_t se = (o_hi - sub < (uint32_t)GW_PROJ_S) ? o_hi : sub + GW_PROJ_S;
#pragma unroll
    for (int s = 0; s < RPT; ++s) {
      if (m[s] && o[s] < se && o[s] + m[s] > sub) {
        const int64_t ts = t0 + (int64_t)(int32_t)(uint32_t)h0[s];
        const uint32_t key = (uint32_t)(h0[s] >> 32);
        const int64_t v2 = wid((uint32_t)h1[s], sel.vfloat), p2 = wid((uint32_t)(h1[s] >> 32), sel.pzero);
        const uint32_t qa = o[s] < sub ? sub - o[s] : 0u, qe = (o[s] + m[s] > se) ? se - o[s] : m[s];
        for (uint32_t q = qa; q < qe; ++q) {
          const uint64_t e = q == 0 ? e0[s] : q == 1 ? e1[s] : area[(uint64_t)u[s] + 2 + q];
          const int64_t v1 = wid((uint32_t)e, sel.vfloat), p1 = wid((uint32_t)(e >> 32), sel.pzero);
          int64_t* r = (int64_t*)(stage + (size_t)(o[s] + q - sub) * sel.stride);
          r[0] = (int64_t)tg[s];
          r[1] = ts;
          r[2] = (int64_t)((uint64_t)key | ((uint64_t)((1u << 24) | (sel.multi ? (uint32_t)sel.b_slot : (0x800000u | q))) << 32));
          r[3] = nmask;
          for (int c = 0; c < nsel; ++c) {
            const uint32_t code = (uint32_t)((c < 16 ? cw0 >> (4 * c) : cw1 >> (4 * (c - 16))) & 15u);
            r[4 + c] = code == 0 ? p1 : code == 1 ? v1 : code == 2 ? v2 : code == 3 ? p2 : 0;
          }
        }
      }
    }
    __syncthreads();
    const size_t bytes = (size_t)(se - sub) * sel.stride;
    char* dst = out + (size_t)(out_base + sub) * sel.stride;
    if ((((uintptr_t)dst) & 15) == 0) {
      // (an odd select count makes the stride 8 mod 16: an odd number of records ends on a half word, which a 16-byte
      // store would carry 8 bytes into the next tile's first record -- another workgroup's, or past the buffer)
      for (size_t x = (size_t)t * 16; x + 16 <= bytes; x += 256 * 16) *(U4*)(dst + x) = *(const U4*)(stage + x);
      if ((bytes & 8) && t == 255) *(uint64_t*)(dst + bytes - 8) = *(const uint64_t*)(stage + bytes - 8);
    } else {
      for (size_t x = (size_t)t * 8; x < bytes; x += 256 * 8) *(uint64_t*)(dst + x) = *(const uint64_t*)(stage + x);
    }
    __syncthreads();
  }
}

// ---- launches

// rows per projection thread: the default (measured on C5, profiles/r09/gw_project_loads.md) or the test hook's
static int gw_proj_rpt() {
  const char* e = getenv("SG_DEBUG_GW_PROJ_RPT");   // (test hook)
  const int r = e ? atoi(e) : GW_PROJ_RPT;
  return r == 1 || r == 2 || r == 4 ? r : GW_PROJ_RPT;
}
static uint32_t gw_proj_lg_tile(int rpt) { return rpt == 1 ? 8u : rpt == 2 ? 9u : 10u; }

// tcount[tile] = matches of the tile's rows, for the ntile tiles of n rows
static void launch_gtile_count(int64_t n, const uint64_t* trig, uint32_t epoch, uint32_t* tcount, int64_t ntile,
                               uint32_t lg_tile, hipStream_t st) {
  hipLaunchKernelGGL(k_gtile_count, dim3((unsigned)((n + GW_COUNT_ROWS - 1) / GW_COUNT_ROWS)), dim3(256), 0, st, n, trig,
                     epoch, tcount, ntile, lg_tile);
  HIPCHK(hipGetLastError());
}

template <int RPT>
static void launch_gscan_project_rpt(int64_t n, int64_t t0, uint64_t base_index, const uint64_t* index,
                                     const uint64_t* trig, uint32_t epoch, const uint64_t* area, const GwSel& sel,
                                     int64_t ntile, int64_t out_base, char* out, const uint32_t* tbase, hipStream_t st) {
  // the trigger list and the stage share the block: 16 KB for C5's 64-byte records, eight workgroups per CU
  const size_t plds = std::max((size_t)256 * RPT * 16, (size_t)GW_PROJ_S * sel.stride);
  if (plds > 65536)
    HIPCHK(hipFuncSetAttribute((const void*)k_gscan_project<RPT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)plds));
  hipLaunchKernelGGL(k_gscan_project<RPT>, dim3((unsigned)ntile), dim3(256), plds, st, n, t0, base_index, index, trig,
                     epoch, area, sel, out_base, out, tbase);
  HIPCHK(hipGetLastError());
}
// tbase: the exclusive scan of launch_gtile_count's counts for the same rpt
static void launch_gscan_project(int rpt, int64_t n, int64_t t0, uint64_t base_index, const uint64_t* index,
                                 const uint64_t* trig, uint32_t epoch, const uint64_t* area, const GwSel& sel,
                                 int64_t ntile, int64_t out_base, char* out, const uint32_t* tbase, hipStream_t st) {
  if (rpt == 1) launch_gscan_project_rpt<1>(n, t0, base_index, index, trig, epoch, area, sel, ntile, out_base, out, tbase, st);
  else if (rpt == 2) launch_gscan_project_rpt<2>(n, t0, base_index, index, trig, epoch, area, sel, ntile, out_base, out, tbase, st);
  else launch_gscan_project_rpt<4>(n, t0, base_index, index, trig, epoch, area, sel, ntile, out_base, out, tbase, st);
}
