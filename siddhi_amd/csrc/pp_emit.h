// pp_emit.h -- match emission of both lane routes (partial.hip).  A lane writes a compact record of positions per
// match into its own slot; once the delivery order of the slots is known, emit_in_order turns every record into a
// match record at its delivery position in the handle's output.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

#include "pp_rows.h"

__global__ void k_pp_iota(int64_t n, uint32_t* __restrict__ x) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) x[i] = (uint32_t)i;
}
__global__ void k_pp_take(int64_t n, const uint64_t* __restrict__ src, const uint32_t* __restrict__ idx, uint64_t* __restrict__ dst) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = src[idx[i]];
}

// Compact emission records {trigger position, trigger combined row, key, group, timestamp row position, position per
// select slot} -> match records {trigger index, ts, key, group, null mask, values}.
// one match record from its compact emission record e
__device__ __forceinline__ void em_build(const uint32_t* __restrict__ e, char* rec, const PpPacked& P,
                                         const DevDesc* __restrict__ dd, const uint64_t* __restrict__ index,
                                         uint64_t base_index) {
  int64_t* h64 = (int64_t*)rec;
  // the trigger row's own columns are read straight from the batch where the slot is lazy; other rows go through
  // their key-sorted position, and a row selected twice in a row is read once
  const uint32_t tq = e[0];
  const int64_t r = (int64_t)e[1] - P.nc;
  h64[0] = (int64_t)(index ? index[r] : base_index + (uint64_t)r);
  const int32_t tp = (int32_t)e[4];
  h64[1] = tp < 0 ? -1 : P.ts ? P.ts[tp] : (uint32_t)tp == tq ? P.bts[r] : pp_lazy_ts(&P, tp);
  uint64_t* h2 = (uint64_t*)(rec + 16);   // {key, group} and {null mask, 0} as two 8-byte stores
  h2[0] = (uint64_t)e[2] | ((uint64_t)e[3] << 32);
  uint32_t nm = 0;
  int64_t* vals = (int64_t*)(rec + 32);
  const int ns = dd->n_select;
  int32_t pq = -1;
  int prs = -1;
  int64_t pv = 0;
  for (int s = 0; s < ns; ++s) {
    const int32_t q = (int32_t)e[5 + s];
    const int rs = dd->sel_ret[s];
    if (q < 0 || (P.nul && ((P.nul[q] >> rs) & 1u))) { nm |= 1u << s; vals[s] = 0; continue; }
    if (q == pq && rs == prs) { vals[s] = pv; continue; }   // e.g. e2[0] and e2[last] of a one-event count
    int64_t bits;
    if ((uint32_t)q == tq && !P.val[rs]) bits = P.wide[rs] ? ((const int64_t*)P.bcol[rs])[r] : (int64_t)((const int32_t*)P.bcol[rs])[r];
    else if (P.val[rs]) bits = P.wide[rs] ? ((const int64_t*)P.val[rs])[q] : (int64_t)((const int32_t*)P.val[rs])[q];
    else bits = pp_lazy_bits(&P, q, rs);
    pv = sg_val_bits(sg_val_from_bits(bits, dd->ret_type[rs], 0));
    pq = q;
    prs = rs;
    vals[s] = pv;
  }
  h2[1] = (uint64_t)nm;
}

// delivery position of every slot (slots without a match keep ~0)
__global__ void k_em_dest(int64_t n, const uint32_t* __restrict__ idx, uint32_t* __restrict__ dest) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dest[idx[i]] = (uint32_t)i;
}

// Partial lanes: slot order is start-row order, i.e. key-ordered, so walking the slots reads the compact records and
// the packed rows they point at nearly coalesced; each record is then written to its delivery position.  The block's
// records are assembled in LDS first and written out by consecutive threads taking consecutive 8-byte words of the
// same record, so one store instruction covers whole records instead of one word of 64 scattered ones.
__global__ void __launch_bounds__(256) k_em_scatter(int64_t T, const uint32_t* __restrict__ dest,
                                                    const char* __restrict__ em, int32_t estride, char* __restrict__ out,
                                                    int32_t ostride, PpPacked P, const DevDesc* __restrict__ dd,
                                                    const uint64_t* __restrict__ index, uint64_t base_index) {
  extern __shared__ __align__(16) char em_lds[];
  __shared__ uint32_t dl[256];
  const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t d = 0xFFFFFFFFu;
  if (w < T) {
    d = dest[w];
    if (d != 0xFFFFFFFFu)
      em_build((const uint32_t*)(em + (size_t)w * estride), em_lds + (size_t)threadIdx.x * ostride, P, dd, index,
               base_index);
  }
  dl[threadIdx.x] = d;
  __syncthreads();
  const int words = ostride / 8;
  const int all = (int)blockDim.x * words;
  for (int x = threadIdx.x; x < all; x += blockDim.x) {
    const int rec = x / words, wd = x - rec * words;
    const uint32_t to = dl[rec];
    if (to == 0xFFFFFFFFu) continue;
    ((uint64_t*)(out + (size_t)to * ostride))[wd] = ((const uint64_t*)(em_lds + (size_t)rec * ostride))[wd];
  }
}

// ---- host side ------------------------------------------------------------------------------------------------
// First component of a slot's delivery key: (trigger batch row << low) | low bits (partial lanes: the visit slot, 8
// bits; sequence lanes: the emission index within the row, 16).  `none` marks a slot without a match and sorts behind
// every match of the push.
struct K1Layout {
  int rb;                     // bits of a batch row
  int bits;                   // bits of the whole component (the radix sort's end bit)
  uint64_t none;
};
static K1Layout k1_layout(int64_t n, int low) {
  K1Layout k;
  k.rb = 1;
  while ((1ll << k.rb) < n + 1) ++k.rb;
  k.bits = std::min(64, k.rb + low);
  k.none = k.bits >= 64 ? ~0ull : (1ull << k.bits) - 1;
  return k;
}

// Compact match records are 20 + 4 * n_select bytes (k_em_scatter writes the 32 + 8 * n_select-byte ones).
static int32_t em_compact_stride(int nsel) { return 20 + 4 * nsel; }

// order[0, total) lists the slots that hold a match, in delivery order: their match records are appended to h->out.
// Records are built in slot order (a lane's slots hold one key's matches: the compact records and the packed rows
// they name are read nearly in order) and scattered to their delivery positions.
static void emit_in_order(SgHandle* h, const BatchView& bv, const PpPacked& P, const char* dest_name, int64_t slots,
                          int64_t total, const uint32_t* order, const char* em) {
  hipStream_t st = h->stream;
  const int nsel = h->desc.n_select;
  const int32_t rstride = 32 + 8 * nsel;
  const dim3 blk(256);
  char* out = h->out.reserve(total, nsel, st);
  uint32_t* dest = (uint32_t*)h->ws.get(dest_name, 4 * (size_t)(slots + 1), st);
  HIPCHK(hipMemsetAsync(dest, 0xFF, 4 * (size_t)slots, st));
  hipLaunchKernelGGL(k_em_dest, dim3((unsigned)((total + 255) / 256)), blk, 0, st, total, order, dest);
  if ((size_t)256 * rstride > 65536)   // (up to SG_MAX_SELECT selected attributes: 256 * 288 B of LDS)
    HIPCHK(hipFuncSetAttribute((const void*)k_em_scatter, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(256 * rstride)));
  hipLaunchKernelGGL(k_em_scatter, dim3((unsigned)((slots + 255) / 256)), blk, (size_t)256 * rstride, st, slots, dest, em,
                     em_compact_stride(nsel), out + (size_t)h->out.n * rstride, rstride, P, h->ddesc, bv.index,
                     bv.base_index);
  HIPCHK(hipGetLastError());
  h->out.n += total;
}
