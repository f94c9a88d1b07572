// ranges.h -- the hold pass of range routing, shared by the device range router (ranges.hip, sg_range_*) and the node
// pipeline (node.hip, sg_node_set_ranges): descriptor checks, the descriptor's HBM image and the kernel that runs the
// range conditions of a row's stream through the postfix VM (sg_device.h, register stack sized by the programs' depth
// as in pred.h) into a 32-bit hold mask per row (RangePartitionExecutor.execute,
// C/partition/executor/RangePartitionExecutor.java:38-43).  Everything here is per translation unit.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "sg_device.h"
#include "sg_engine.h"

namespace {

const int RR_TILE = 256;

struct RrDev {   // what the kernels read of the descriptor (HBM copy)
  int32_t playback, n_ranges;
  uint32_t ranged_streams;   // bit s: stream s has ranges
  int32_t range_stream[SG_MAX_RANGES], range_label[SG_MAX_RANGES], prog_off[SG_MAX_RANGES], prog_len[SG_MAX_RANGES];
  int64_t code[SG_MAX_CODE];
};

struct RrIn {   // the input batch in HBM
  int64_t n;
  uint64_t base_index;
  const int64_t* ts;
  const int32_t* stream;   // nullptr: every row stream 0
  const int32_t* key;      // nullptr: every row key -1
  const uint64_t* index;   // nullptr: base_index + row
};

struct ColReader {   // VAR word 3 = batch column
  const SgCols* c;
  int64_t row;
  __device__ SgVal read(int, int, int col, int type) { return sg_read_col(*c, col, type, row); }
};

__device__ __forceinline__ bool rr_ranged(uint32_t ranged_streams, int s) {
  return s >= 0 && s < SG_MAX_STREAMS && ((ranged_streams >> s) & 1u);
}
__device__ __forceinline__ bool rr_ranged(const RrDev* d, int s) { return rr_ranged(d->ranged_streams, s); }

// output rows of one input row: a ranged row one per holding range (none: dropped, or one clock row under playback),
// every other row one
__device__ __forceinline__ uint32_t rr_count(uint32_t mask, bool ranged, int playback) {
  if (!ranged) return 1u;
  return mask ? (uint32_t)__popc(mask) : (playback ? 1u : 0u);
}

template <int D>
__global__ void __launch_bounds__(RR_TILE) k_rr_hold(RrIn in, SgCols cols, const RrDev* __restrict__ d,
                                                     const int32_t* __restrict__ label_key,
                                                     uint32_t* __restrict__ mask_out, int64_t* __restrict__ tile_cnt,
                                                     unsigned long long* __restrict__ mins) {
  typedef SgRegStack<D> Stack;
  __shared__ uint32_t s_cnt[RR_TILE / 64];
  __shared__ uint32_t s_first[RR_TILE / 64][SG_MAX_RANGES];   // per wave and range: first holding row in tile, or ~0
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t row = (int64_t)blockIdx.x * RR_TILE + t;
  const int nr = d->n_ranges;
  uint32_t mask = 0, cnt = 0;
  if (row < in.n) {
    const int s = in.stream ? in.stream[row] : 0;
    const bool ranged = rr_ranged(d, s);
    if (ranged) {
      ColReader rd{&cols, row};
      for (int r = 0; r < nr; ++r)
        if (d->range_stream[r] == s && sg_eval<ColReader, Stack>(d->code + d->prog_off[r], d->prog_len[r], rd))
          mask |= 1u << r;
    }
    cnt = rr_count(mask, ranged, d->playback);
    mask_out[row] = mask;
  }
  // tile count: wave reduce, then LDS
  uint32_t c = cnt;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o, 64);
  if (lane == 0) s_cnt[wave] = c;
  // first holder per range with an unassigned label (rows grow with the lane: the lowest set ballot bit)
  for (int r = 0; r < nr; ++r) {
    if (label_key[d->range_label[r]] >= 0) continue;   // (wave-uniform)
    const uint64_t b = __ballot((mask >> r) & 1u);
    if (lane == 0) s_first[wave][r] = b ? (uint32_t)(wave * 64 + __builtin_ctzll(b)) : ~0u;
  }
  __syncthreads();
  if (t == 0) tile_cnt[blockIdx.x] = (int64_t)s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
  if (t < nr && label_key[d->range_label[t]] < 0) {
    uint32_t f = ~0u;
#pragma unroll
    for (int w = RR_TILE / 64 - 1; w >= 0; --w)
      if (s_first[w][t] != ~0u) f = s_first[w][t];
    if (f != ~0u) {
      const unsigned long long v = ((unsigned long long)((int64_t)blockIdx.x * RR_TILE + f) << 5) | (unsigned)t;
      // most tiles come after the first holder: look before paying for an atomic on one hot address
      if (__hip_atomic_load(&mins[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > v) atomicMin(&mins[t], v);
    }
  }
}

// A range program is well formed: known opcodes with their operands inside the program, VAR on a batch column of the
// range's stream with the column's type, no stack underflow, one value left.  Returns the stack depth.
int check_prog(const sg_range_desc& d, int r) {
  const int off = d.prog_off[r], len = d.prog_len[r];
  if (off < 0 || len < 1 || off + len > d.code_len) throw SgError(SG_EINVAL, "range program outside the code");
  const int64_t* c = d.code + off;
  int sp = 0, mx = 0, pc = 0;
  auto need = [&](int words, int pops) {
    if (pc + words > len) throw SgError(SG_EINVAL, "range program: truncated instruction");
    if (sp < pops) throw SgError(SG_EINVAL, "range program: operand stack underflow");
  };
  while (pc < len) {
    switch ((int)c[pc]) {
      case SG_OP_VAR: {
        need(5, 0);
        const int64_t col = c[pc + 3], type = c[pc + 4];
        if (col < 0 || col >= d.n_cols) throw SgError(SG_EINVAL, "range program: column out of range");
        if (type != d.col_type[col]) throw SgError(SG_EINVAL, "range program: column type mismatch");
        if (d.col_stream[col] != d.range_stream[r])
          throw SgError(SG_EINVAL, "range program reads a column of another stream");
        ++sp;
        pc += 5;
        break;
      }
      case SG_OP_CONST:
        need(3, 0);
        if (c[pc + 1] < SG_T_STRING || c[pc + 1] > SG_T_BOOL) throw SgError(SG_EINVAL, "range program: bad constant type");
        ++sp;
        pc += 3;
        break;
      case SG_OP_CMP:
        need(3, 2);
        if (c[pc + 1] < 0 || c[pc + 1] > 5 || c[pc + 2] < 0 || c[pc + 2] > 3)
          throw SgError(SG_EINVAL, "range program: bad compare");
        --sp;
        pc += 3;
        break;
      case SG_OP_MATH:
        need(3, 2);
        if (c[pc + 1] < 0 || c[pc + 1] > 4 || c[pc + 2] < SG_T_INT || c[pc + 2] > SG_T_DOUBLE)
          throw SgError(SG_EINVAL, "range program: bad arithmetic");
        --sp;
        pc += 3;
        break;
      case SG_OP_AND:
      case SG_OP_OR:
        need(1, 2);
        --sp;
        pc += 1;
        break;
      case SG_OP_NOT:
      case SG_OP_ISNULL:
        need(1, 1);
        pc += 1;
        break;
      default:
        throw SgError(SG_EINVAL, "range program: unknown opcode");
    }
    mx = std::max(mx, sp);
  }
  if (sp != 1) throw SgError(SG_EINVAL, "range program must leave one value");
  return mx;
}

// The descriptor is well formed (SG_EINVAL) and its programs fit the VM stack (SG_EUNSUPPORTED); returns their depth.
int rr_validate(const sg_range_desc& d) {
  if (d.abi_version != SG_ABI_VERSION) throw SgError(SG_EINVAL, "sg_range_desc ABI version mismatch");
  if (d.n_cols < 0 || d.n_cols > SG_MAX_COLS) throw SgError(SG_EINVAL, "bad n_cols");
  if (d.n_ranges < 1 || d.n_ranges > SG_MAX_RANGES) throw SgError(SG_EINVAL, "bad n_ranges");
  if (d.n_labels < 1 || d.n_labels > d.n_ranges) throw SgError(SG_EINVAL, "bad n_labels");
  if (d.code_len < 0 || d.code_len > SG_MAX_CODE) throw SgError(SG_EINVAL, "bad code_len");
  for (int c = 0; c < d.n_cols; ++c) {
    if (d.col_type[c] < SG_T_STRING || d.col_type[c] > SG_T_BOOL) throw SgError(SG_EINVAL, "bad column type");
    if (d.col_stream[c] < 0 || d.col_stream[c] >= SG_MAX_STREAMS) throw SgError(SG_EINVAL, "bad column stream");
  }
  int depth = 0;
  for (int k = 0; k < d.n_ranges; ++k) {
    if (d.range_stream[k] < 0 || d.range_stream[k] >= SG_MAX_STREAMS) throw SgError(SG_EINVAL, "range stream out of range");
    if (d.range_label[k] < 0 || d.range_label[k] >= d.n_labels) throw SgError(SG_EINVAL, "range label out of range");
    depth = std::max(depth, check_prog(d, k));
  }
  if (depth > SG_VM_STACK) throw SgError(SG_EUNSUPPORTED, "range program deeper than the VM stack");
  return depth;
}

// the descriptor's HBM image (the caller uploads it)
RrDev rr_dev_image(const sg_range_desc& d) {
  RrDev hd;
  memset(&hd, 0, sizeof(hd));
  hd.playback = d.playback ? 1 : 0;
  hd.n_ranges = d.n_ranges;
  for (int k = 0; k < d.n_ranges; ++k) {
    hd.ranged_streams |= 1u << d.range_stream[k];
    hd.range_stream[k] = d.range_stream[k];
    hd.range_label[k] = d.range_label[k];
    hd.prog_off[k] = d.prog_off[k];
    hd.prog_len[k] = d.prog_len[k];
  }
  memcpy(hd.code, d.code, sizeof(int64_t) * d.code_len);
  return hd;
}

// f(c) for every batch column a range program reads
template <class F>
void rr_for_each_read_col(const sg_range_desc& d, F f) {
  for (int k = 0; k < d.n_ranges; ++k) {
    const int64_t* c = d.code + d.prog_off[k];
    for (int pc = 0; pc < d.prog_len[k];) {
      const int op = (int)c[pc];
      if (op == SG_OP_VAR) {
        f((int)c[pc + 3]);
        pc += 5;
      } else {
        pc += (op == SG_OP_CONST || op == SG_OP_CMP || op == SG_OP_MATH) ? 3 : 1;
      }
    }
  }
}

// the hold pass over `ntiles` tiles of RR_TILE rows, instantiated for the programs' depth
void rr_launch_hold(int depth, hipStream_t st, unsigned ntiles, const RrIn& in, const SgCols& cols, const RrDev* ddev,
                    const int32_t* lk, uint32_t* masks, int64_t* cnt, unsigned long long* mins) {
  const dim3 grd(ntiles), blk(RR_TILE);
  if (depth <= 2) hipLaunchKernelGGL(k_rr_hold<2>, grd, blk, 0, st, in, cols, ddev, lk, masks, cnt, mins);
  else if (depth <= 4) hipLaunchKernelGGL(k_rr_hold<4>, grd, blk, 0, st, in, cols, ddev, lk, masks, cnt, mins);
  else if (depth <= 8) hipLaunchKernelGGL(k_rr_hold<8>, grd, blk, 0, st, in, cols, ddev, lk, masks, cnt, mins);
  else hipLaunchKernelGGL(k_rr_hold<SG_VM_STACK>, grd, blk, 0, st, in, cols, ddev, lk, masks, cnt, mins);
  HIPCHK(hipGetLastError());
}

}  // namespace
