// keypart.h -- the closed form's key partition: the push's virtual rows -> per-key walker records in arrival order.
// LDS counting-sort kernels (k_part1*, k_part2*, k_part_segs), pass 1 beyond 256 key groups (k_hist_wide, k_part1b,
// part1_wide), and the stage functions run_every_next (engine_impl.h) calls, one per route.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "sg_engine.h"
#include "sg_prim.h"
#include "walk_rec.h"

// ---------------------------------------------------------------------------------------------
// 2'. Key partition without a general sort (K <= 65536).  A stable MSD counting sort in one pass (K <= 256:
// digit = key) or two (digit = key group = high bits, then key within its group = low bits).  Each pass
// cuts its input into segments; a histogram kernel counts digits per segment, one exclusive scan over the
// (digit, segment) table gives every segment's output position per digit, and the scatter kernel ranks each
// 2048-row sub-tile stably by digit in LDS (wave ballots over the digit bits) and writes every digit run out
// as whole lines.  Pass 1 reads the raw columns and builds the walker records on the way (no pack pass);
// pass 2 reads pass 1's records and 1-byte in-group keys.  The per-key segments are read off the last
// pass's offsets (no bounds pass).  Same result as the radix sort: per key its rows in arrival order.
// Rows per thread per LDS-staged sub-tile, per pass (measured on C2, 100M events / 10k keys: pass 1 -- raw columns in,
// 16-B records out, 79 key-group digits -- is fastest with 1024-row sub-tiles (more resident workgroups: part_group
// 1.26 -> 1.04 ms); pass 2 -- records in, 128 in-group digits -- with 4096-row ones (longer runs per digit: part_key
// 0.90 -> 0.78 ms))
#ifndef SG_PT1
#define SG_PT1 4
#endif
#ifndef SG_PT2
#define SG_PT2 16
#endif
static const int PT1 = SG_PT1, PT1_ROWS = 256 * SG_PT1;
static const int PT2 = SG_PT2, PT2_ROWS = 256 * SG_PT2;
static const int PT_D = 256;       // digit values per pass (8 bits)

struct PartPlan {
  uint32_t K, lb, ng, two;    // keys; pass-2 digit bits (key & (2^lb - 1)); pass-1 digit values (key >> lb); 2 passes?
  uint32_t nb1, nb2;          // bits that tell the digits apart (ballots per 64-row step)
  uint32_t seg1, ns1;         // rows per pass-1 segment (multiple of PT1_ROWS); pass-1 segments
  uint32_t ts2, nj;           // pass-1 segments per pass-2 segment; pass-2 segments per group
  uint32_t w1, nc1;           // group table o1: pass-1 segments per column; columns per group (its stride).  One
                              // column per segment (w1 = 1, nc1 = ns1) up to 65,536 keys, P1_COL_SEGS beyond (part1_wide)
};

template <class R, int PT, class TG = uint16_t>
struct PartLds {
  R stage[256 * PT];          // the sub-tile's records, sorted by digit
  TG tag[256 * PT];           // key (pass 1) / in-group key (pass 2) of each staged record
  uint32_t cw[4][PT_D];       // per-wave digit counts, then per-wave slot cursors
  uint32_t ls[PT_D];          // sub-tile start of each digit
  uint32_t tot[PT_D];         // sub-tile count of each digit
  uint32_t run[PT_D];         // next output position of each digit
  uint32_t wsum[4];
};

__device__ __forceinline__ uint32_t block_excl_scan256(uint32_t x, uint32_t* wsum) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint32_t inc = x;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t y = (uint32_t)__shfl_up((int)inc, o);
    if (lane >= o) inc += y;
  }
  if (lane == 63) wsum[w] = inc;
  __syncthreads();
  uint32_t add = 0;
  for (int i = 0; i < w; ++i) add += wsum[i];
  return add + inc - x;
}

// lanes of the wave holding the same digit: rank among them (arrival order) and their count
__device__ __forceinline__ void peer_rank(bool valid, uint32_t d, uint32_t nb, uint32_t& rank, uint32_t& cnt) {
  uint64_t m = __ballot(valid);
  for (uint32_t b = 0; b < nb; ++b) {
    const bool bit = (d >> b) & 1u;
    const uint64_t bb = __ballot(bit);
    m &= bit ? bb : ~bb;
  }
  rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
  cnt = (uint32_t)__popcll(m);
}

// digit counts -> per-wave slot cursors and sub-tile digit starts; returns the sub-tile's staged rows
template <class R, int PT, class TG>
__device__ __forceinline__ uint32_t part_cursors(PartLds<R, PT, TG>& L) {
  const uint32_t t = threadIdx.x;
  const uint32_t c0 = L.cw[0][t], c1 = L.cw[1][t], c2 = L.cw[2][t], c3 = L.cw[3][t];
  const uint32_t tot = c0 + c1 + c2 + c3;
  const uint32_t ex = block_excl_scan256(tot, L.wsum);
  L.ls[t] = ex;
  L.tot[t] = tot;
  L.cw[0][t] = ex;
  L.cw[1][t] = ex + c0;
  L.cw[2][t] = ex + c0 + c1;
  L.cw[3][t] = ex + c0 + c1 + c2;
  __syncthreads();
  return L.ls[PT_D - 1] + L.tot[PT_D - 1];
}

// pass-1 histogram: segment j = virtual rows [j*seg1, (j+1)*seg1); h1[group * ns1 + j].  Per-wave counters
// (fewer same-address LDS atomics), eight rows per thread in flight.
static __global__ void __launch_bounds__(256) k_part1_hist(KeyOf kf, PartPlan pp, int64_t nt, uint32_t* __restrict__ h1,
                                                           uint32_t* __restrict__ flags) {
  __shared__ uint32_t cnt[4][PT_D];
  const uint32_t j = blockIdx.x, t = threadIdx.x, w = t >> 6;
#pragma unroll
  for (int q = 0; q < 4; ++q) cnt[q][t] = 0;
  __syncthreads();
  const int64_t r0 = (int64_t)j * pp.seg1, r1 = (nt < r0 + pp.seg1) ? nt : r0 + pp.seg1;
  uint32_t bad = 0;
  for (int64_t rb = r0; rb < r1; rb += 256 * 8) {
    uint32_t k[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const int64_t r = rb + s * 256 + t;
      k[s] = r < r1 ? kf((uint32_t)r) : 0xffffffffu;
    }
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      if (k[s] < pp.K) atomicAdd(&cnt[w][k[s] >> pp.lb], 1u);
      else if (k[s] != 0xffffffffu) bad |= PK_KEY_RANGE;   // beyond the caller's key_bound
    }
  }
  __syncthreads();
  if (t < pp.ng) h1[(size_t)t * pp.ns1 + j] = cnt[0][t] + cnt[1][t] + cnt[2][t] + cnt[3][t];
  if (bad) atomicOr(flags, bad);
}

// pass-1 scatter: records of segment j, grouped (two passes) or final (one pass).  TG holds a staged record's key
// (32 bits beyond 65536 keys), LK its in-group key.
template <class T, bool N, class TG = uint16_t, class LK = uint8_t, int P = PT1>
__global__ void __launch_bounds__(256) k_part1(PackFn<T, N> pk, KeyOf kf, PartPlan pp, int64_t nt,
                                               const uint32_t* __restrict__ o1, WRec<T, N>* __restrict__ orec,
                                               LK* __restrict__ olk, uint32_t* __restrict__ flags) {
  typedef WRec<T, N> R;
  extern __shared__ __attribute__((aligned(16))) char lds_raw[];
  PartLds<R, P, TG>& L = *(PartLds<R, P, TG>*)lds_raw;
  constexpr uint32_t PROWS = 256 * P;
  const uint32_t j = blockIdx.x, t = threadIdx.x, w = t >> 6, lane = t & 63;
  const uint32_t lmask = (1u << pp.lb) - 1u;
  if (t < pp.ng) L.run[t] = o1[(size_t)t * pp.ns1 + j];
  const int64_t rb = (int64_t)j * pp.seg1, re = (nt < rb + pp.seg1) ? nt : rb + pp.seg1;
  const int64_t t0 = N ? v_ts(pk.v, 0) : 0;
  uint32_t bad = 0;
  // the sub-tile's loads, all issued before the first use (one memory latency per sub-tile)
  auto load = [&](int64_t base, uint32_t* tg, R* rc) {
    const uint32_t rows = (uint32_t)((re - base < PROWS) ? re - base : PROWS);
    if (base >= (int64_t)pk.v.nc) {
      // batch rows only: branch-free loads (rows past the end re-read the last row and are dropped)
      const uint32_t b0 = (uint32_t)(base - pk.v.nc), last = rows - 1;
#pragma unroll
      for (int s = 0; s < P; ++s) {
        const uint32_t i = w * (P * 64) + s * 64 + lane;
        const uint32_t b = b0 + (i < rows ? i : last);
        const uint32_t k = (uint32_t)pk.v.key[b];
        uint32_t bd = 0;
        rc[s] = pk.batch(b, t0, bd);
        tg[s] = (i < rows && k < pp.K) ? k : 0xffffffffu;
        bad |= (i < rows && k != 0xffffffffu) ? bd : 0u;
      }
    } else {
#pragma unroll
      for (int s = 0; s < P; ++s) {
        const uint32_t i = w * (P * 64) + s * 64 + lane;
        const uint32_t r = (uint32_t)(base + i);
        const uint32_t k = i < rows ? kf(r) : 0xffffffffu;
        tg[s] = k < pp.K ? k : 0xffffffffu;
        if (k < pp.K) {
          rc[s] = pk(r);
          if (N) {
            const int64_t dt = v_ts(pk.v, r) - t0;
            if (dt != (int64_t)(int32_t)dt) bad |= PK_TS_RANGE;
            if (R::has_pay && pk.v.pcol && pk.v.pw == 8) {
              const int64_t pv = v_payload(pk.v, r);
              if (pv != (int64_t)(int32_t)pv) bad |= PK_PAY_RANGE;
            }
          }
        }
      }
    }
  };
  uint32_t tg[P], tn[P];
  R rc[P], rn[P];
  if (rb < re) load(rb, tg, rc);
  for (int64_t base = rb; base < re; base += PROWS) {
#pragma unroll
    for (int q = 0; q < 4; ++q) L.cw[q][t] = 0;
    __syncthreads();
#pragma unroll
    for (int s = 0; s < P; ++s)
      if (tg[s] != 0xffffffffu) atomicAdd(&L.cw[w][tg[s] >> pp.lb], 1u);
    __syncthreads();
    const uint32_t staged = part_cursors(L);
#pragma unroll
    for (int s = 0; s < P; ++s) {
      const bool valid = tg[s] != 0xffffffffu;
      const uint32_t d = valid ? tg[s] >> pp.lb : 0u;
      uint32_t rank, cnt;
      peer_rank(valid, d, pp.nb1, rank, cnt);
      if (valid) {
        const uint32_t slot = L.cw[w][d] + rank;
        if (rank == 0) L.cw[w][d] = slot + cnt;
        L.stage[slot] = rc[s];
        L.tag[slot] = (TG)tg[s];
      }
    }
    if (base + PROWS < re) load(base + PROWS, tn, rn);   // next sub-tile in flight during the write-out
    __syncthreads();
    for (uint32_t q = t; q < staged; q += 256) {
      const uint32_t k = L.tag[q], d = k >> pp.lb;
      const uint32_t dst = L.run[d] + q - L.ls[d];
      if ((int64_t)dst >= nt) { bad |= PK_INTERNAL; continue; }
      orec[dst] = L.stage[q];
      if (olk) olk[dst] = (LK)(k & lmask);
    }
    __syncthreads();
    L.run[t] += L.tot[t];
#pragma unroll
    for (int s = 0; s < P; ++s) { tg[s] = tn[s]; rc[s] = rn[s]; }
  }
  if (bad) atomicOr(flags, bad);
}

// pass-2 segment (g, jj): group g's rows that came from pass-1 segments [jj*ts2, (jj+1)*ts2) -- whole columns of o1
// (ts2 is a multiple of w1)
__device__ __forceinline__ void part2_range(const PartPlan& pp, const uint32_t* o1, uint32_t g, uint32_t jj,
                                            uint32_t& lo, uint32_t& hi) {
  const uint32_t cs = pp.ts2 / pp.w1;
  lo = o1[(size_t)g * pp.nc1 + jj * cs];
  hi = o1[(size_t)g * pp.nc1 + min(pp.nc1, (jj + 1) * cs)];
}

static __global__ void __launch_bounds__(256) k_part2_hist(PartPlan pp, const uint32_t* __restrict__ o1,
                                                           const uint8_t* __restrict__ glk, uint32_t* __restrict__ h2) {
  __shared__ uint32_t cnt[4][PT_D];
  const uint32_t g = blockIdx.x / pp.nj, jj = blockIdx.x % pp.nj, t = threadIdx.x, w = t >> 6;
#pragma unroll
  for (int q = 0; q < 4; ++q) cnt[q][t] = 0;
  __syncthreads();
  uint32_t lo, hi;
  part2_range(pp, o1, g, jj, lo, hi);
  for (uint32_t pb = lo; pb < hi; pb += 256 * 8) {
    uint32_t d[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const uint32_t p = pb + s * 256 + t;
      d[s] = p < hi ? (uint32_t)glk[p] : 0xffffffffu;
    }
#pragma unroll
    for (int s = 0; s < 8; ++s)
      if (d[s] != 0xffffffffu) atomicAdd(&cnt[w][d[s]], 1u);
  }
  __syncthreads();
  if (t < (1u << pp.lb)) h2[(size_t)((g << pp.lb) + t) * pp.nj + jj] = cnt[0][t] + cnt[1][t] + cnt[2][t] + cnt[3][t];
}

template <class R>
__global__ void __launch_bounds__(256) k_part2(PartPlan pp, const uint32_t* __restrict__ o1, const uint32_t* __restrict__ o2,
                                               const R* __restrict__ grec, const uint8_t* __restrict__ glk,
                                               R* __restrict__ srec, uint32_t cap, uint32_t* __restrict__ flags) {
  extern __shared__ __attribute__((aligned(16))) char lds_raw[];
  PartLds<R, PT2>& L = *(PartLds<R, PT2>*)lds_raw;
  const uint32_t g = blockIdx.x / pp.nj, jj = blockIdx.x % pp.nj;
  const uint32_t t = threadIdx.x, w = t >> 6, lane = t & 63;
  if (t < (1u << pp.lb)) L.run[t] = o2[(size_t)((g << pp.lb) + t) * pp.nj + jj];
  uint32_t lo, hi;
  part2_range(pp, o1, g, jj, lo, hi);
  auto load = [&](uint32_t base, uint32_t* tg, R* rc) {
    const uint32_t rows = (hi - base < (uint32_t)PT2_ROWS) ? hi - base : (uint32_t)PT2_ROWS;
#pragma unroll
    for (int s = 0; s < PT2; ++s) {
      const uint32_t i = w * (PT2 * 64) + s * 64 + lane;
      const uint32_t p = base + (i < rows ? i : rows - 1);   // (clamped: branch-free loads)
      const uint32_t lk = glk[p];
      rc[s] = grec[p];
      tg[s] = i < rows ? lk : 0xffffffffu;
    }
  };
  uint32_t tg[PT2], tn[PT2];
  R rc[PT2], rn[PT2];
  if (lo < hi) load(lo, tg, rc);
  for (uint32_t base = lo; base < hi; base += PT2_ROWS) {
#pragma unroll
    for (int q = 0; q < 4; ++q) L.cw[q][t] = 0;
    __syncthreads();
#pragma unroll
    for (int s = 0; s < PT2; ++s)
      if (tg[s] != 0xffffffffu) atomicAdd(&L.cw[w][tg[s]], 1u);
    __syncthreads();
    const uint32_t staged = part_cursors(L);
#pragma unroll
    for (int s = 0; s < PT2; ++s) {
      const bool valid = tg[s] != 0xffffffffu;
      const uint32_t d = valid ? tg[s] : 0u;
      uint32_t rank, cnt;
      peer_rank(valid, d, pp.nb2, rank, cnt);
      if (valid) {
        const uint32_t slot = L.cw[w][d] + rank;
        if (rank == 0) L.cw[w][d] = slot + cnt;
        L.stage[slot] = rc[s];
        L.tag[slot] = (uint16_t)d;
      }
    }
    if (hi - base > (uint32_t)PT2_ROWS) load(base + PT2_ROWS, tn, rn);   // next sub-tile in flight during the write-out
    __syncthreads();
    for (uint32_t q = t; q < staged; q += 256) {
      const uint32_t d = L.tag[q];
      const uint32_t dst = L.run[d] + q - L.ls[d];
      if (dst >= cap) { atomicOr(flags, PK_INTERNAL); continue; }
      srec[dst] = L.stage[q];
    }
    __syncthreads();
    L.run[t] += L.tot[t];
#pragma unroll
    for (int s = 0; s < PT2; ++s) { tg[s] = tn[s]; rc[s] = rn[s]; }
  }
}

// pass 2 moves records as opaque words (vector / scalar members keep the 16 per thread in registers)
typedef uint32_t PtU4 __attribute__((ext_vector_type(4)));
struct PtB24 { uint64_t a, b, c; };
template <class R>
using PtRaw = typename std::conditional<sizeof(R) == 16, PtU4, PtB24>::type;

// per-key segments [seg_b, seg_e) of the sorted records from the last pass's offsets (stride = its segments)
static __global__ void k_part_segs(uint32_t K, const uint32_t* __restrict__ o, uint32_t stride,
                                   uint32_t* __restrict__ seg_b, uint32_t* __restrict__ seg_e) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= K) return;
  seg_b[k] = o[(size_t)k * stride];
  seg_e[k] = o[(size_t)(k + 1) * stride];
}

static PartPlan part_plan(uint32_t K, int64_t nt) {
  PartPlan p;
  memset(&p, 0, sizeof(p));
  p.K = K;
  uint32_t bits = 0;
  while ((1ull << bits) < (uint64_t)K) ++bits;
  auto nbits = [](uint32_t nd) { uint32_t b = 0; while ((1u << b) < nd) ++b; return b; };
  if (K <= (uint32_t)PT_D) {
    p.two = 0; p.lb = 0; p.ng = K;
  } else {
    const uint32_t hb = (bits + 1) / 2;
    p.two = 1; p.lb = bits - hb; p.ng = (K + (1u << p.lb) - 1) >> p.lb;
  }
  p.nb1 = nbits(p.ng);
  p.nb2 = p.lb;
  // >= ~2048 pass-1 segments when the batch allows (8 workgroups per CU), at most 32 sub-tiles each
  const int64_t sub = std::max<int64_t>(1, std::min<int64_t>(32, nt / ((int64_t)PT1_ROWS * 2048)));
  p.seg1 = (uint32_t)(PT1_ROWS * sub);
  p.ns1 = (uint32_t)std::max<int64_t>(1, (nt + p.seg1 - 1) / p.seg1);
  // pass-2 segments of ~8192 rows of one group
  p.ts2 = (uint32_t)std::max<int64_t>(1, std::min<int64_t>(p.ns1, (int64_t)8192 * p.ng / p.seg1));
  p.nj = (p.ns1 + p.ts2 - 1) / p.ts2;
  p.w1 = 1;
  p.nc1 = p.ns1;
  return p;
}

// ---- more than 256 key groups (C5's 1M keys): the group domain in two passes.  Pass 1a groups rows by supergroup
// (k_part1 with 32-bit staged keys and 16-bit in-supergroup keys); pass 1b splits each supergroup into its groups,
// arrival order kept, straight into the group-domain positions of the group table (o1).  Pass 1a needs offsets per
// pass-1 segment (oa); every reader of the group table reads it at a multiple of tsb or ts2 segments or at a group's
// first row, so that table has one column per P1_COL_SEGS segments, and tsb and ts2 are multiples of that.
static const uint32_t P1_COL_SEGS = 8;

// per column jj of w1 part1 segments: rows of each group g -> h[g * nc1 + jj] (up to 4096 groups, LDS counters that
// run on over the column's segments), and per segment j the rows of each supergroup (2^lbs consecutive groups; at most
// 64 of them) -> ha[sg * ns1 + j] from the same counters (one pass over the keys)
static __global__ void __launch_bounds__(256) k_hist_wide(KeyOf kf, uint32_t K, uint32_t lb, uint32_t ng, uint32_t seg1,
                                                          uint32_t ns1, uint32_t w1, uint32_t nc1, int64_t nt,
                                                          uint32_t* __restrict__ h, uint32_t lbs, uint32_t nsg,
                                                          uint32_t* __restrict__ ha, uint32_t* __restrict__ flags) {
  __shared__ uint32_t cnt[4096];
  __shared__ uint32_t sgc[64];   // each supergroup's rows in the column's segments so far
  const uint32_t jj = blockIdx.x, t = threadIdx.x, w = t >> 6, lane = t & 63;
  for (uint32_t g = t; g < ng; g += 256) cnt[g] = 0;
  if (t < 64) sgc[t] = 0;
  __syncthreads();
  uint32_t bad = 0;
  const uint32_t j1 = min(ns1, (jj + 1) * w1), nd = 1u << lbs;
  for (uint32_t j = jj * w1; j < j1; ++j) {
    const int64_t r0 = (int64_t)j * seg1, r1 = min(nt, r0 + seg1);
    for (int64_t rb = r0; rb < r1; rb += 256 * 8) {   // eight rows per thread in flight
      uint32_t k[8];
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        const int64_t r = rb + s * 256 + t;
        k[s] = r < r1 ? kf((uint32_t)r) : 0xffffffffu;
      }
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        if (k[s] < K) atomicAdd(&cnt[k[s] >> lb], 1u);
        else if (k[s] != 0xffffffffu) bad |= PK_KEY_RANGE;
      }
    }
    __syncthreads();
    // a wave per supergroup: its groups' counters summed across the lanes
    for (uint32_t sg = w; sg < nsg; sg += 4) {
      uint32_t c = 0;
      for (uint32_t i = lane; i < nd; i += 64) {
        const uint32_t g = (sg << lbs) + i;
        c += g < ng ? cnt[g] : 0u;
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) c += (uint32_t)__shfl_xor((int)c, o);
      if (lane == 0) {
        ha[(size_t)sg * ns1 + j] = c - sgc[sg];
        sgc[sg] = c;
      }
    }
    __syncthreads();
  }
  for (uint32_t g = t; g < ng; g += 256) h[(size_t)g * nc1 + jj] = cnt[g];
  if (bad) atomicOr(flags, bad);
}

struct Part1bArgs {
  uint32_t lb;          // in-group key bits
  uint32_t lbs;         // group bits inside a supergroup
  uint32_t ns1, tsb;    // part1 segments; per pass-1b segment (a multiple of w1)
  uint32_t nsb;         // pass-1b segments per supergroup
  uint32_t ng, w1, nc1; // groups; part1 segments per column of o1; its columns per group
  const uint32_t* oa;   // pass-1a offsets [sg * ns1 + j]
  const uint32_t* o1;   // group-domain offsets [g * nc1 + j / w1]
};

template <int PT>
struct Part1bLds {
  PtU4 stage[256 * PT];
  uint16_t tag[256 * PT];
  uint32_t cw[4][256];
  uint32_t ls[256], tot[256], run[256];
  uint32_t wsum[4];
};

template <int PT>
__global__ void __launch_bounds__(256) k_part1b(Part1bArgs B, const PtU4* __restrict__ grecA, const uint16_t* __restrict__ glkA,
                                                PtU4* __restrict__ grec, uint8_t* __restrict__ glk, uint32_t cap,
                                                uint32_t* __restrict__ flags) {
  extern __shared__ __attribute__((aligned(16))) char lds_raw[];
  Part1bLds<PT>& L = *(Part1bLds<PT>*)lds_raw;
  const uint32_t sg = blockIdx.x / B.nsb, jj = blockIdx.x % B.nsb;
  const uint32_t t = threadIdx.x, w = t >> 6, lane = t & 63;
  const uint32_t jf = min(B.ns1, jj * B.tsb), jl = min(B.ns1, jf + B.tsb);
  const uint32_t lo = B.oa[(size_t)sg * B.ns1 + jf], hi = B.oa[(size_t)sg * B.ns1 + jl];
  const uint32_t nd = 1u << B.lbs, lmask = (1u << B.lb) - 1u;
  if (t < nd && ((sg << B.lbs) | t) < B.ng) L.run[t] = B.o1[(size_t)((sg << B.lbs) | t) * B.nc1 + jf / B.w1];
  const int ROWS = 256 * PT;
  auto load = [&](uint32_t base, PtU4* rc, uint32_t* tg) {
    const uint32_t rows = min((uint32_t)ROWS, hi - base);
#pragma unroll
    for (int s = 0; s < PT; ++s) {
      const uint32_t i = w * (PT * 64) + s * 64 + lane;
      const uint32_t p = base + (i < rows ? i : rows - 1);
      rc[s] = grecA[p];
      const uint32_t k = glkA[p];
      tg[s] = i < rows ? k : 0xffffffffu;
    }
  };
  PtU4 rc[PT], rn[PT];
  uint32_t tg[PT], tn[PT];
  if (lo < hi) load(lo, rc, tg);
  for (uint32_t base = lo; base < hi; base += ROWS) {
#pragma unroll
    for (int q = 0; q < 4; ++q) L.cw[q][t] = 0;
    __syncthreads();
#pragma unroll
    for (int s = 0; s < PT; ++s)
      if (tg[s] != 0xffffffffu) atomicAdd(&L.cw[w][tg[s] >> B.lb], 1u);
    __syncthreads();
    uint32_t staged;
    {
      const uint32_t c0 = L.cw[0][t], c1 = L.cw[1][t], c2 = L.cw[2][t], c3 = L.cw[3][t];
      const uint32_t tt = c0 + c1 + c2 + c3;
      const uint32_t ex = block_excl_scan256(tt, L.wsum);
      L.ls[t] = ex;
      L.tot[t] = tt;
      L.cw[0][t] = ex;
      L.cw[1][t] = ex + c0;
      L.cw[2][t] = ex + c0 + c1;
      L.cw[3][t] = ex + c0 + c1 + c2;
      __syncthreads();
      staged = L.ls[255] + L.tot[255];
    }
#pragma unroll
    for (int s = 0; s < PT; ++s) {
      const bool valid = tg[s] != 0xffffffffu;
      const uint32_t d = valid ? tg[s] >> B.lb : 0u;
      uint32_t rank, cnt;
      peer_rank(valid, d, B.lbs, rank, cnt);
      if (valid) {
        const uint32_t slot = L.cw[w][d] + rank;
        if (rank == 0) L.cw[w][d] = slot + cnt;
        L.stage[slot] = rc[s];
        L.tag[slot] = (uint16_t)tg[s];
      }
    }
    if (base + ROWS < hi) load(base + ROWS, rn, tn);
    __syncthreads();
    for (uint32_t q = t; q < staged; q += 256) {
      const uint32_t k = L.tag[q], d = k >> B.lb;
      const uint32_t dst = L.run[d] + q - L.ls[d];
      if (dst >= cap) { atomicOr(flags, PK_INTERNAL); continue; }
      grec[dst] = L.stage[q];
      glk[dst] = (uint8_t)(k & lmask);
    }
    __syncthreads();
    if (t < nd) L.run[t] += L.tot[t];
#pragma unroll
    for (int s = 0; s < PT; ++s) { rc[s] = rn[s]; tg[s] = tn[s]; }
  }
}

// Pass 1 of the key partition beyond 256 key groups (up to 4096 groups of 2^pp.lb keys, e.g. C5's 1M keys): rows ->
// narrow walker records grouped by key group, arrival order kept inside a group, in two LDS counting passes --
// supergroups of 2^lbs groups (<= 64 of them, k_part1 with 32-bit staged keys), then the groups inside each
// supergroup (k_part1b) straight into the group positions of the group table: o1[g * nc1 + c] is the first position of
// group g's rows from part1 segment c * w1 on (after every row of the groups before it), o1[ng * nc1] the row count.
// Output: grec, glk (in-group key), o1.
template <class T>
static void part1_wide(SgHandle* h, const PackFn<T, true>& pk, KeyOf kf, uint32_t kb, int64_t nt, const PartPlan& pp,
                       uint32_t* h1, uint32_t* o1, WRec<T, true>* grec, uint8_t* glk, uint32_t* pk_flags) {
  typedef WRec<T, true> R;
  hipStream_t st = h->stream;
  const uint32_t lb = pp.lb, ng = pp.ng;
  const size_t n1 = (size_t)pp.ng * pp.nc1 + 1;
  {
    // two passes: supergroups of 2^lbs groups (<= 64 of them), then groups inside each supergroup.  (C5, 4096 groups,
    // per 500M-row push: 256 supergroups part_group 7.7 + part_split 3.8 ms; 64 supergroups 6.0 + 4.2 ms -- pass 1's
    // runs per supergroup are 4x longer; 32 supergroups 5.8 + 4.7 ms; profiles/r06/ab_lbs.sh)
    uint32_t lbs = 0;
    while (((ng + (1u << lbs) - 1) >> lbs) > 64u && lbs < 8) ++lbs;
    PartPlan pa2 = pp;
    pa2.lb = lb + lbs;
    pa2.ng = (kb + (1u << pa2.lb) - 1) >> pa2.lb;
    uint32_t nbA = 0;
    while ((1u << nbA) < pa2.ng) ++nbA;
    pa2.nb1 = nbA;
    const size_t nA = (size_t)pa2.ng * pp.ns1 + 1;
    uint32_t* hA = (uint32_t*)h->ws.get("part_hA", sizeof(uint32_t) * nA, st);
    uint32_t* oA = (uint32_t*)h->ws.get("part_oA", sizeof(uint32_t) * nA, st);
    R* grecA = (R*)h->ws.get("grecA", sizeof(R) * nt, st);
    uint16_t* glkA = (uint16_t*)h->ws.get("glkA", 2 * nt, st);
    h->kbeg("part_hist");
    HIPCHK(hipMemsetAsync(hA + nA - 1, 0, sizeof(uint32_t), st));
    HIPCHK(hipMemsetAsync(h1 + n1 - 1, 0, sizeof(uint32_t), st));
    hipLaunchKernelGGL(k_hist_wide, dim3(pp.nc1), dim3(256), 0, st, kf, kb, lb, ng, pp.seg1, pp.ns1, pp.w1, pp.nc1, nt, h1,
                       lbs, pa2.ng, hA, pk_flags);
    HIPCHK(hipGetLastError());
    sg_exclusive_scan(h->ws, st, "part_scan_tmpA", (const uint32_t*)hA, oA, (uint32_t)0, nA, rocprim::plus<uint32_t>());
    sg_exclusive_scan(h->ws, st, "part_scan_tmp", (const uint32_t*)h1, o1, (uint32_t)0, n1, rocprim::plus<uint32_t>());
    h->kend();
    h->kbeg("part_group");
    // (rows per thread per LDS sub-tile of this 256-digit pass: SG_DEBUG_P1_PT test hook)
    const char* pe = getenv("SG_DEBUG_P1_PT");
    const int p1 = pe ? atoi(pe) : 8;   // (C5: 8.1 -> 7.3 ms per 500M-row push against 4, profiles/r06/ab_p1.sh)
    auto launch_a = [&](auto pt) {
      constexpr int P = decltype(pt)::value;
      const size_t ldsA = sizeof(PartLds<R, P, uint32_t>);
      HIPCHK(hipFuncSetAttribute((const void*)k_part1<T, true, uint32_t, uint16_t, P>,
                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsA));
      hipLaunchKernelGGL((k_part1<T, true, uint32_t, uint16_t, P>), dim3(pp.ns1), dim3(256), ldsA, st, pk, kf, pa2, nt, oA,
                         grecA, glkA, pk_flags);
    };
    if (p1 == 8) launch_a(std::integral_constant<int, 8>());
    else if (p1 == 16) launch_a(std::integral_constant<int, 16>());
    else launch_a(std::integral_constant<int, PT1>());
    HIPCHK(hipGetLastError());
    h->kend();
    h->kbeg("part_split");
    Part1bArgs B;
    B.lb = lb;
    B.lbs = lbs;
    B.ns1 = pp.ns1;
    const int64_t per_sg = std::max<int64_t>(1, nt / pa2.ng);
    // (rows of a supergroup per pass-1b segment: SG_DEBUG_P1B_ROWS test hook, several segments in a small push)
    const char* be = getenv("SG_DEBUG_P1B_ROWS");
    const int64_t rows_b = be ? std::max(atoi(be), 1) : 32768;
    B.nsb = (uint32_t)std::max<int64_t>(1, std::min<int64_t>(pp.ns1, per_sg / rows_b));
    B.tsb = (pp.ns1 + B.nsb - 1) / B.nsb;
    B.tsb = (B.tsb + pp.w1 - 1) / pp.w1 * pp.w1;   // whole columns of o1
    B.nsb = (pp.ns1 + B.tsb - 1) / B.tsb;
    B.ng = ng;
    B.w1 = pp.w1;
    B.nc1 = pp.nc1;
    B.oa = oA;
    B.o1 = o1;
    const size_t ldsB = sizeof(Part1bLds<16>);
    HIPCHK(hipFuncSetAttribute((const void*)k_part1b<16>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsB));
    hipLaunchKernelGGL((k_part1b<16>), dim3(pa2.ng * B.nsb), dim3(256), ldsB, st, B, (const PtU4*)grecA, glkA,
                       (PtU4*)grec, glk, (uint32_t)nt, pk_flags);
    HIPCHK(hipGetLastError());
    h->kend();
  }
}

// ---------------------------------------------------------------------------------------------
// Key partition stage of the closed form: the push's virtual rows -> per-key walker records in arrival order.
// One function per route; each fills a KeyPart.

// The facts of one push that every stage reads and none changes.
struct PushCtx {
  SgHandle* h;
  const BatchView& bv;
  int64_t n, nc, nt;          // batch rows, carried rows, virtual rows
  uint32_t kb, K;             // key bound; keys the walkers see (1 if unpartitioned)
  int op, val_col_a, val_col_b;
  KeyOf kf;                   // partition key of a virtual row
};

template <class T, bool N>
struct KeyPart {
  Src<T, N> src;              // position -> record (srec: the key-sorted records)
  uint32_t* seg_b;            // per key: its positions [seg_b, seg_e)
  uint32_t* seg_e;
  uint32_t* pk_flags;         // PK_* flags raised while the records were built
  WRec<T, N>* prec;           // records in arrival order (radix-sort and unpartitioned routes)
};

template <class T, bool N>
static KeyPart<T, N> part_begin(const PushCtx& c, const Virt& v) {
  typedef WRec<T, N> R;
  SgHandle* h = c.h;
  hipStream_t st = h->stream;
  KeyPart<T, N> kp;
  kp.src.srec = nullptr;
  kp.src.pk.v = v;
  kp.pk_flags = (uint32_t*)h->ws.get("pack_flags", sizeof(uint32_t), st);
  HIPCHK(hipMemsetAsync(kp.pk_flags, 0, sizeof(uint32_t), st));
  kp.prec = (R*)h->ws.get("prec", sizeof(R) * c.nt, st);
  kp.seg_b = (uint32_t*)h->ws.get("seg_b", sizeof(uint32_t) * c.K, st);
  kp.seg_e = (uint32_t*)h->ws.get("seg_e", sizeof(uint32_t) * c.K, st);
  return kp;
}

// Plan and workspaces of the LDS partition (one pass up to 256 keys, two up to 65,536, and beyond that pass 1 in two:
// part1_wide).
template <class T, bool N>
struct PartLdsBufs {
  PartPlan pp;
  size_t n1, n2;              // entries of the pass-1 / pass-2 (digit, segment) tables
  uint32_t *h1, *o1, *h2, *o2;
  WRec<T, N>* srec;           // the key-sorted records
  WRec<T, N>* grec;           // two passes: pass 1's records, grouped by key group
  uint8_t* glk;               //             and their in-group keys
};
template <class T, bool N>
static PartLdsBufs<T, N> part_lds_bufs(const PushCtx& c) {
  typedef WRec<T, N> R;
  typedef PtRaw<R> RW;
  static_assert(sizeof(RW) == sizeof(R), "raw record layout");
  SgHandle* h = c.h;
  hipStream_t st = h->stream;
  PartLdsBufs<T, N> b;
  memset(&b, 0, sizeof(b));
  PartPlan& pp = b.pp;
  pp = part_plan(c.kb, c.nt);
  if (c.kb > 65536u) {   // groups of 256 keys: pass 2 sorts by the low 8 bits
    pp.two = 1;
    pp.lb = 8;
    pp.ng = (c.kb + 255u) >> 8;
    pp.nb1 = 0;
    while ((1u << pp.nb1) < pp.ng) ++pp.nb1;
    pp.nb2 = 8;
    pp.w1 = P1_COL_SEGS;
    pp.nc1 = (pp.ns1 + pp.w1 - 1) / pp.w1;
    pp.ts2 = (uint32_t)std::max<int64_t>(1, std::min<int64_t>(pp.ns1, (int64_t)8192 * pp.ng / pp.seg1));
    pp.ts2 = (pp.ts2 + pp.w1 - 1) / pp.w1 * pp.w1;   // whole columns of o1
    pp.nj = (pp.ns1 + pp.ts2 - 1) / pp.ts2;
  }
  b.n1 = (size_t)pp.ng * pp.nc1 + 1;
  b.h1 = (uint32_t*)h->ws.get("part_h1", sizeof(uint32_t) * b.n1, st);
  b.o1 = (uint32_t*)h->ws.get("part_o1", sizeof(uint32_t) * b.n1, st);
  b.srec = (R*)h->ws.get("srec", sizeof(R) * c.nt, st);
  HIPCHK(hipFuncSetAttribute((const void*)k_part1<T, N>, hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)sizeof(PartLds<R, PT1>)));
  HIPCHK(hipFuncSetAttribute((const void*)k_part2<RW>, hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)sizeof(PartLds<RW, PT2>)));
  if (pp.two) {
    b.grec = (R*)h->ws.get("grec", sizeof(R) * c.nt, st);
    b.glk = (uint8_t*)h->ws.get("glk", c.nt, st);
    b.n2 = ((size_t)pp.ng << pp.lb) * pp.nj + 1;
    b.h2 = (uint32_t*)h->ws.get("part_h2", sizeof(uint32_t) * b.n2, st);
    b.o2 = (uint32_t*)h->ws.get("part_o2", sizeof(uint32_t) * b.n2, st);
  }
  return b;
}

// LDS route up to 65,536 keys, pass 1: the histogram, then the scatter -- final (one pass: srec and the segments) or
// by key group (two passes: grec / glk, for part_lds_pass2).
template <class T, bool N>
static void part_lds_pass1(const PushCtx& c, KeyPart<T, N>& kp, const PartLdsBufs<T, N>& b) {
  SgHandle* h = c.h;
  hipStream_t st = h->stream;
  const PartPlan& pp = b.pp;
  const size_t lds1 = sizeof(PartLds<WRec<T, N>, PT1>);
  h->kbeg("part_hist");
  HIPCHK(hipMemsetAsync(b.h1 + b.n1 - 1, 0, sizeof(uint32_t), st));
  hipLaunchKernelGGL(k_part1_hist, dim3(pp.ns1), dim3(256), 0, st, c.kf, pp, c.nt, b.h1, kp.pk_flags);
  HIPCHK(hipGetLastError());
  sg_exclusive_scan(h->ws, st, "part_scan_tmp", b.h1, b.o1, (uint32_t)0, b.n1, rocprim::plus<uint32_t>());
  h->kend();
  h->kbeg(pp.two ? "part_group" : "part_scatter");
  hipLaunchKernelGGL((k_part1<T, N>), dim3(pp.ns1), dim3(256), lds1, st, kp.src.pk, c.kf, pp, c.nt, b.o1,
                     pp.two ? b.grec : b.srec, b.glk, kp.pk_flags);   // (b.glk is null when one pass does it)
  HIPCHK(hipGetLastError());
  h->kend();
  if (!pp.two)
    hipLaunchKernelGGL(k_part_segs, dim3((c.kb + 255) / 256), dim3(256), 0, st, c.kb, b.o1, pp.ns1, kp.seg_b, kp.seg_e);
}

// LDS route, pass 2: the grouped records (grec / glk / o1, from part_lds_pass1 or part1_wide) sorted by in-group key
// -> srec and the segments.
template <class T, bool N>
static void part_lds_pass2(const PushCtx& c, KeyPart<T, N>& kp, const PartLdsBufs<T, N>& b) {
  typedef PtRaw<WRec<T, N>> RW;
  SgHandle* h = c.h;
  hipStream_t st = h->stream;
  const PartPlan& pp = b.pp;
  h->kbeg("part_hist2");
  HIPCHK(hipMemsetAsync(b.h2 + b.n2 - 1, 0, sizeof(uint32_t), st));
  hipLaunchKernelGGL(k_part2_hist, dim3(pp.ng * pp.nj), dim3(256), 0, st, pp, b.o1, b.glk, b.h2);
  HIPCHK(hipGetLastError());
  sg_exclusive_scan(h->ws, st, "part_scan_tmp2", b.h2, b.o2, (uint32_t)0, b.n2, rocprim::plus<uint32_t>());
  h->kend();
  h->kbeg("part_key");
  hipLaunchKernelGGL((k_part2<RW>), dim3(pp.ng * pp.nj), dim3(256), sizeof(PartLds<RW, PT2>), st, pp, b.o1, b.o2,
                     (const RW*)b.grec, b.glk, (RW*)b.srec, (uint32_t)c.nt, kp.pk_flags);
  HIPCHK(hipGetLastError());
  h->kend();
  hipLaunchKernelGGL(k_part_segs, dim3((c.kb + 255) / 256), dim3(256), 0, st, c.kb, b.o2, pp.nj, kp.seg_b, kp.seg_e);
}

// Radix-sort route (sg_options.partition_sort, or more keys than the LDS partition takes): pack, a stable sort of the
// records by key (rocPRIM onesweep), and the segments from the sorted keys.
template <class T, bool N>
static void part_sort(const PushCtx& c, KeyPart<T, N>& kp) {
  typedef WRec<T, N> R;
  SgHandle* h = c.h;
  hipStream_t st = h->stream;
  const int64_t nt = c.nt;
  int end_bit = 1;
  while ((1ull << end_bit) <= (uint64_t)c.kb) ++end_bit;
  uint32_t* skeys = (uint32_t*)h->ws.get("skeys", sizeof(uint32_t) * nt, st);
  R* srec = (R*)h->ws.get("srec", sizeof(R) * nt, st);
  uint32_t* pkeys = (uint32_t*)h->ws.get("pkeys", sizeof(uint32_t) * nt, st);
  h->kbeg("pack");
  hipLaunchKernelGGL((k_pack<T, N>), dim3((unsigned)std::min<int64_t>((nt + 255) / 256, 256 * 32)), dim3(256), 0, st,
                     kp.src.pk, c.kf, c.kb, nt, kp.prec, pkeys, kp.pk_flags);
  HIPCHK(hipGetLastError());
  h->kend();
  h->kbeg("key_sort");
  if constexpr (sizeof(R) == 16)   // one onesweep instantiation for every 16-byte record format
    sg_radix_sort_pairs(h->ws, st, "sort_tmp", pkeys, skeys, (Blob16*)kp.prec, (Blob16*)srec, (size_t)nt, end_bit);
  else
    sg_radix_sort_pairs(h->ws, st, "sort_tmp", pkeys, skeys, kp.prec, srec, (size_t)nt, end_bit);
  h->kend();
  kp.src.srec = srec;
  HIPCHK(hipMemsetAsync(kp.seg_b, 0, sizeof(uint32_t) * c.K, st));
  HIPCHK(hipMemsetAsync(kp.seg_e, 0, sizeof(uint32_t) * c.K, st));
  h->kbeg("bounds");
  hipLaunchKernelGGL(k_bounds, dim3((unsigned)std::min<int64_t>((nt + 1023) / 1024, 256 * 16)), dim3(256), 0, st, skeys,
                     nt, c.kb, kp.seg_b, kp.seg_e);
  h->kend();
  HIPCHK(hipGetLastError());
}

// Unpartitioned: one key whose rows are already in arrival order -- pack only, one segment [0, nt).
template <class T, bool N>
static void part_none(const PushCtx& c, KeyPart<T, N>& kp) {
  hipStream_t st = c.h->stream;
  KeyOf kf{nullptr, nullptr, 0};
  hipLaunchKernelGGL((k_pack<T, N>), dim3((unsigned)std::min<int64_t>((c.nt + 255) / 256, 256 * 32)), dim3(256), 0, st,
                     kp.src.pk, kf, c.kb, c.nt, kp.prec, (uint32_t*)nullptr, kp.pk_flags);
  HIPCHK(hipGetLastError());
  kp.src.srec = kp.prec;
  const uint32_t seg[2] = {0u, (uint32_t)c.nt};
  HIPCHK(hipMemcpyAsync(kp.seg_b, &seg[0], sizeof(uint32_t), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(kp.seg_e, &seg[1], sizeof(uint32_t), hipMemcpyHostToDevice, st));
}
