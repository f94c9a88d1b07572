// ranges.hip -- the device range router (sg_range_*, include/siddhi_gpu.h): PartitionStreamReceiver with
// RangePartitionExecutors (C/partition/PartitionStreamReceiver.java:94-100,110-125,270-275;
// C/partition/executor/RangePartitionExecutor.java:38-43) over one SoA batch, in three passes:
//
//   hold    one thread per row runs the range conditions of the row's stream through the postfix VM (sg_device.h,
//           register stack sized by the programs' depth as in pred.h) -> a 32-bit hold mask per row, the copy count
//           of every 256-row tile, and per range with an unassigned label the smallest (row << 5 | range) holding it
//   scan    rocPRIM exclusive scan of the tile counts; one pinned readback of the total and the minima; the host hands
//           out the new label ids in order of the minima, sizes the output for the total and uploads the label keys
//   expand  one workgroup per tile lists (source row, range) of each of its output slots in LDS, 256 slots at a time,
//           and stores destination-major: consecutive threads write consecutive output rows of every array
//
// The count of a row is one function of (mask, stream) used by both kernels (rr_count), so the expand pass's stores
// land inside [0, total) by construction; the output is allocated from the total before the expand launch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "sg_device.h"
#include "sg_engine.h"
#include "sg_prim.h"

namespace {

const int RR_TILE = 256;
const uint64_t RR_NONE = ~0ull;
// slot entries of the expand pass: row in tile | what << 8 (what < 32: a range; else one of these)
const uint32_t RR_PASS = 0x40, RR_CLOCK = 0x41;

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

struct RrOut {
  int64_t cap;   // rows allocated (= the scanned total)
  int64_t* ts;
  int32_t* stream;
  int32_t* key;
  uint64_t* index;
  void* col[SG_MAX_COLS];
  uint8_t* nul[SG_MAX_COLS];
  int32_t width[SG_MAX_COLS];
  int32_t n_cols;
};

struct ColReader {   // VAR word 3 = batch column
  const SgCols* c;
  int64_t row;
  __device__ SgVal read(int, int, int col, int type) { return sg_read_col(*c, col, type, row); }
};

__device__ __forceinline__ bool rr_ranged(const RrDev* d, int s) {
  return s >= 0 && s < SG_MAX_STREAMS && ((d->ranged_streams >> s) & 1u);
}

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

__global__ void __launch_bounds__(RR_TILE) k_rr_expand(RrIn in, SgCols cols, const RrDev* __restrict__ d,
                                                       const int32_t* __restrict__ label_key,
                                                       const uint32_t* __restrict__ masks,
                                                       const int64_t* __restrict__ tile_off, RrOut out) {
  __shared__ uint32_t s_wtot[RR_TILE / 64];
  __shared__ uint32_t s_slot[RR_TILE];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t row0 = (int64_t)blockIdx.x * RR_TILE;
  const int64_t row = row0 + t;
  const int nr = d->n_ranges;
  uint32_t mask = 0;
  bool ranged = false, live = row < in.n;
  if (live) {
    const int s = in.stream ? in.stream[row] : 0;
    ranged = rr_ranged(d, s);
    mask = ranged ? masks[row] : 0u;
  }
  const uint32_t cnt = live ? rr_count(mask, ranged, d->playback) : 0u;
  // in-tile exclusive prefix of cnt: per range one ballot (plus one for the rows that are a single row), lanes below
  const uint64_t below = (1ull << lane) - 1ull;
  uint32_t pre = 0, wtot = 0;
  {
    const uint64_t b = __ballot(cnt != 0 && mask == 0);   // pass-through and clock rows
    pre += __popcll(b & below);
    wtot += __popcll(b);
  }
  for (int r = 0; r < nr; ++r) {
    const uint64_t b = __ballot((mask >> r) & 1u);
    pre += __popcll(b & below);
    wtot += __popcll(b);
  }
  if (lane == 0) s_wtot[wave] = wtot;
  __syncthreads();
  uint32_t total = 0;
#pragma unroll
  for (int w = 0; w < RR_TILE / 64; ++w) {
    if (w < wave) pre += s_wtot[w];
    total += s_wtot[w];
  }
  const int64_t base = tile_off[blockIdx.x];
  // this thread's slots are [pre, pre + cnt); `q` walks them as the 256-slot windows pass, `rm` holds the ranges left
  uint32_t q = pre, rm = mask;
  const uint32_t end = pre + cnt;
  for (uint32_t lo = 0; lo < total; lo += RR_TILE) {
    const uint32_t hi = lo + RR_TILE;
    while (q < end && q < hi) {
      uint32_t what;
      if (mask) {
        what = (uint32_t)__builtin_ctz(rm);
        rm &= rm - 1;
      } else {
        what = ranged ? RR_CLOCK : RR_PASS;
      }
      s_slot[q - lo] = (uint32_t)t | (what << 8);
      ++q;
    }
    __syncthreads();
    const uint32_t j = lo + t;
    const int64_t dst = base + j;
    if (j < total && dst < out.cap) {
      const uint32_t e = s_slot[t];
      const int64_t src = row0 + (e & 0xffu);
      const uint32_t what = e >> 8;
      out.ts[dst] = in.ts[src];
      out.index[dst] = in.index ? in.index[src] : in.base_index + (uint64_t)src;
      int32_t st, ky;
      if (what < SG_MAX_RANGES) {
        st = d->range_stream[what];
        ky = label_key[d->range_label[what]];
      } else if (what == RR_CLOCK) {
        st = -1;
        ky = -1;
      } else {
        st = in.stream ? in.stream[src] : 0;
        ky = in.key ? in.key[src] : -1;
      }
      out.stream[dst] = st;
      out.key[dst] = ky;
      for (int c = 0; c < out.n_cols; ++c) {   // (uniform branches: the same columns for every thread)
        if (out.col[c]) {
          if (out.width[c] == 8) ((uint64_t*)out.col[c])[dst] = gptr<uint64_t>(cols.col[c])[src];
          else ((uint32_t*)out.col[c])[dst] = gptr<uint32_t>(cols.col[c])[src];
        }
        if (out.nul[c]) out.nul[c][dst] = gptr<uint8_t>(cols.nul[c])[src];
      }
    }
    __syncthreads();
  }
}

struct Readback {
  int64_t total;
  uint64_t mins[SG_MAX_RANGES];
};

}  // namespace

struct sg_range_router {
  int device = 0;
  bool ok = false;
  sg_range_desc desc;
  int depth = 0;
  RrDev* ddev = nullptr;
  hipStream_t stream = nullptr;
  hipEvent_t ev[4] = {};
  Workspace ws;
  Readback* rb = nullptr;   // pinned
  const void* out_cols[SG_MAX_COLS] = {};
  const uint8_t* out_nuls[SG_MAX_COLS] = {};
  sg_range_stats stats = {};
  std::string err;
};

namespace {

template <class F>
int rr_guard(sg_range_router* r, F&& f) {
  try {
    f();
    return SG_OK;
  } catch (SgError& e) {
    if (r) r->err = e.msg;
    return e.code;
  } catch (std::exception& e) {
    if (r) r->err = e.what();
    return SG_EINVAL;
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

void rr_validate(sg_range_router& r) {
  const sg_range_desc& d = r.desc;
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
  r.depth = depth;
}

void launch_hold(sg_range_router& r, unsigned ntiles, const RrIn& in, const SgCols& cols, const int32_t* lk,
                 uint32_t* masks, int64_t* cnt, unsigned long long* mins) {
  const dim3 grd(ntiles), blk(RR_TILE);
  hipStream_t st = r.stream;
  if (r.depth <= 2) hipLaunchKernelGGL(k_rr_hold<2>, grd, blk, 0, st, in, cols, r.ddev, lk, masks, cnt, mins);
  else if (r.depth <= 4) hipLaunchKernelGGL(k_rr_hold<4>, grd, blk, 0, st, in, cols, r.ddev, lk, masks, cnt, mins);
  else if (r.depth <= 8) hipLaunchKernelGGL(k_rr_hold<8>, grd, blk, 0, st, in, cols, r.ddev, lk, masks, cnt, mins);
  else hipLaunchKernelGGL(k_rr_hold<SG_VM_STACK>, grd, blk, 0, st, in, cols, r.ddev, lk, masks, cnt, mins);
  HIPCHK(hipGetLastError());
}

std::string col_name(const char* what, int c) { return std::string(what) + std::to_string(c); }

void rr_route(sg_range_router& r, const sg_batch* b, int32_t* label_key, int32_t* next_key, sg_batch* out) {
  const sg_range_desc& d = r.desc;
  hipStream_t st = r.stream;
  const int64_t n = b->n;
  if (n < 0 || n >= (1ll << 30) - 1) throw SgError(SG_EINVAL, "batch too large (max 2^30-2 rows)");
  if (*next_key < 0) throw SgError(SG_EINVAL, "next_key is negative");
  int32_t lk_max = -1;
  for (int l = 0; l < d.n_labels; ++l) {
    if (label_key[l] >= *next_key) throw SgError(SG_EINVAL, "label_key holds an id that next_key has not reached");
    lk_max = std::max(lk_max, label_key[l]);
  }
  memset(out, 0, sizeof(*out));
  out->base_index = b->base_index;
  out->on_device = 1;
  out->cols = r.out_cols;
  out->nulls = r.out_nuls;
  out->key_bound = std::max(b->key_bound, lk_max + 1);
  memset(r.out_cols, 0, sizeof(r.out_cols));
  memset(r.out_nuls, 0, sizeof(r.out_nuls));
  r.stats.calls++;
  r.stats.hold_ms = r.stats.expand_ms = 0.f;
  if (n == 0) return;
  if (!b->ts) throw SgError(SG_EINVAL, "batch without timestamps");
  r.stats.rows += n;

  // the input in HBM: a device batch as it is, a host batch through the router's own buffers
  RrIn in;
  SgCols cols;
  memset(&cols, 0, sizeof(cols));
  in.n = n;
  in.base_index = b->base_index;
  if (b->on_device) {
    in.ts = b->ts;
    in.stream = b->stream;
    in.key = b->key;
    in.index = b->index;
    for (int c = 0; c < d.n_cols; ++c) {
      cols.col[c] = b->cols ? b->cols[c] : nullptr;
      cols.nul[c] = b->nulls ? b->nulls[c] : nullptr;
    }
  } else {
    auto up = [&](const std::string& name, const void* src, size_t width) -> void* {
      if (!src) return nullptr;
      void* dst = r.ws.get(name, width * (size_t)n, st);
      HIPCHK(hipMemcpyAsync(dst, src, width * (size_t)n, hipMemcpyHostToDevice, st));
      return dst;
    };
    in.ts = (const int64_t*)up("in_ts", b->ts, 8);
    in.stream = (const int32_t*)up("in_stream", b->stream, 4);
    in.key = (const int32_t*)up("in_key", b->key, 4);
    in.index = (const uint64_t*)up("in_index", b->index, 8);
    for (int c = 0; c < d.n_cols; ++c) {
      cols.col[c] = b->cols ? up(col_name("in_col", c), b->cols[c], (size_t)sg_col_width(d.col_type[c])) : nullptr;
      cols.nul[c] = (const uint8_t*)(b->nulls ? up(col_name("in_nul", c), b->nulls[c], 1) : nullptr);
    }
  }
  for (int k = 0; k < d.n_ranges; ++k) {   // every column a range program reads must be there
    const int64_t* c = d.code + d.prog_off[k];
    for (int pc = 0; pc < d.prog_len[k];) {
      const int op = (int)c[pc];
      if (op == SG_OP_VAR) {
        if (!cols.col[c[pc + 3]]) throw SgError(SG_EINVAL, "batch is missing a column a range condition reads");
        pc += 5;
      } else {
        pc += (op == SG_OP_CONST || op == SG_OP_CMP || op == SG_OP_MATH) ? 3 : 1;
      }
    }
  }

  const int64_t ntiles = (n + RR_TILE - 1) / RR_TILE;
  uint32_t* masks = (uint32_t*)r.ws.get("masks", sizeof(uint32_t) * (size_t)n, st);
  int64_t* cnt = (int64_t*)r.ws.get("tile_cnt", sizeof(int64_t) * (size_t)(ntiles + 1), st);
  // tile offsets, then [total = off[ntiles], minima] as one readback record
  int64_t* off = (int64_t*)r.ws.get("tile_off", sizeof(int64_t) * (size_t)ntiles + sizeof(Readback), st);
  unsigned long long* mins = (unsigned long long*)(off + ntiles + 1);
  int32_t* lk = (int32_t*)r.ws.get("label_key", sizeof(int32_t) * SG_MAX_RANGES, st);
  HIPCHK(hipMemcpyAsync(lk, label_key, sizeof(int32_t) * d.n_labels, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(mins, 0xff, sizeof(uint64_t) * SG_MAX_RANGES, st));
  HIPCHK(hipMemsetAsync(cnt + ntiles, 0, sizeof(int64_t), st));

  HIPCHK(hipEventRecord(r.ev[0], st));
  launch_hold(r, (unsigned)ntiles, in, cols, lk, masks, cnt, mins);
  HIPCHK(hipEventRecord(r.ev[1], st));
  sg_exclusive_scan(r.ws, st, "scan_tmp", cnt, off, (int64_t)0, (size_t)(ntiles + 1), rocprim::plus<int64_t>());
  HIPCHK(hipMemcpyAsync(r.rb, off + ntiles, sizeof(Readback), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));

  const int64_t total = r.rb->total;
  if (total < 0 || total > n * (int64_t)SG_MAX_RANGES) throw SgError(SG_EHIP, "range router: implausible copy count");
  // new labels in first-seen order: by the smallest (row, range position) holding them
  std::vector<std::pair<uint64_t, int>> seen;
  for (int k = 0; k < d.n_ranges; ++k) {
    const int l = d.range_label[k];
    if (label_key[l] >= 0 || r.rb->mins[k] == RR_NONE) continue;
    auto it = std::find_if(seen.begin(), seen.end(), [&](const std::pair<uint64_t, int>& x) { return x.second == l; });
    if (it == seen.end()) seen.emplace_back(r.rb->mins[k], l);
    else it->first = std::min<uint64_t>(it->first, r.rb->mins[k]);
  }
  std::sort(seen.begin(), seen.end());
  if ((int64_t)*next_key + (int64_t)seen.size() > INT32_MAX) throw SgError(SG_ECAPACITY, "more than 2^31 keys");
  for (auto& x : seen) {
    label_key[x.second] = (*next_key)++;
    lk_max = std::max(lk_max, label_key[x.second]);
  }
  if (!seen.empty()) HIPCHK(hipMemcpyAsync(lk, label_key, sizeof(int32_t) * d.n_labels, hipMemcpyHostToDevice, st));
  out->key_bound = std::max(b->key_bound, lk_max + 1);
  r.stats.copies += total;
  out->n = total;
  if (total == 0) {
    HIPCHK(hipEventElapsedTime(&r.stats.hold_ms, r.ev[0], r.ev[1]));
    return;
  }

  // the output, sized from the total that was read back, before the launch that fills it
  RrOut o;
  memset(&o, 0, sizeof(o));
  o.cap = total;
  o.n_cols = d.n_cols;
  o.ts = (int64_t*)r.ws.get("out_ts", 8 * (size_t)total, st);
  o.stream = (int32_t*)r.ws.get("out_stream", 4 * (size_t)total, st);
  o.key = (int32_t*)r.ws.get("out_key", 4 * (size_t)total, st);
  o.index = (uint64_t*)r.ws.get("out_index", 8 * (size_t)total, st);
  for (int c = 0; c < d.n_cols; ++c) {
    o.width[c] = sg_col_width(d.col_type[c]);
    if (cols.col[c]) o.col[c] = r.ws.get(col_name("out_col", c), (size_t)o.width[c] * (size_t)total, st);
    if (cols.nul[c]) o.nul[c] = (uint8_t*)r.ws.get(col_name("out_nul", c), (size_t)total, st);
  }
  HIPCHK(hipEventRecord(r.ev[2], st));
  hipLaunchKernelGGL(k_rr_expand, dim3((unsigned)ntiles), dim3(RR_TILE), 0, st, in, cols, r.ddev, lk, masks, off, o);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(r.ev[3], st));
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipEventElapsedTime(&r.stats.hold_ms, r.ev[0], r.ev[1]));
  HIPCHK(hipEventElapsedTime(&r.stats.expand_ms, r.ev[2], r.ev[3]));

  out->ts = o.ts;
  out->stream = o.stream;
  out->key = o.key;
  out->index = o.index;
  for (int c = 0; c < d.n_cols; ++c) {
    r.out_cols[c] = o.col[c];
    r.out_nuls[c] = o.nul[c];
  }
}

}  // namespace

extern "C" {

int sg_range_open(int hip_device, const sg_range_desc* d, sg_range_router** out) {
  if (!d || !out) return SG_EINVAL;
  sg_range_router* r = new sg_range_router();
  *out = r;
  return rr_guard(r, [&] {
    r->desc = *d;
    r->device = hip_device;
    rr_validate(*r);
    HIPCHK(hipSetDevice(hip_device));
    HIPCHK(hipStreamCreateWithFlags(&r->stream, hipStreamNonBlocking));
    for (auto& e : r->ev) HIPCHK(hipEventCreate(&e));
    HIPCHK(hipHostMalloc((void**)&r->rb, sizeof(Readback), hipHostMallocDefault));
    RrDev hd;
    memset(&hd, 0, sizeof(hd));
    hd.playback = d->playback ? 1 : 0;
    hd.n_ranges = d->n_ranges;
    for (int k = 0; k < d->n_ranges; ++k) {
      hd.ranged_streams |= 1u << d->range_stream[k];
      hd.range_stream[k] = d->range_stream[k];
      hd.range_label[k] = d->range_label[k];
      hd.prog_off[k] = d->prog_off[k];
      hd.prog_len[k] = d->prog_len[k];
    }
    memcpy(hd.code, d->code, sizeof(int64_t) * d->code_len);
    HIPCHK(hipMalloc((void**)&r->ddev, sizeof(RrDev)));
    HIPCHK(hipMemcpy(r->ddev, &hd, sizeof(RrDev), hipMemcpyHostToDevice));
    r->ok = true;
  });
}

int sg_range_route(sg_range_router* r, const sg_batch* in, int32_t* label_key, int32_t* next_key, sg_batch* out) {
  if (!r || !in || !label_key || !next_key || !out) return SG_EINVAL;
  return rr_guard(r, [&] {
    if (!r->ok) throw SgError(SG_EINVAL, "router did not open");
    HIPCHK(hipSetDevice(r->device));
    rr_route(*r, in, label_key, next_key, out);
  });
}

int sg_range_stats_get(const sg_range_router* r, sg_range_stats* st) {
  if (!r || !st) return SG_EINVAL;
  *st = r->stats;
  return SG_OK;
}

int sg_range_close(sg_range_router* r) {
  if (!r) return SG_EINVAL;
  if (r->stream || r->ddev || r->rb) hipSetDevice(r->device);
  if (r->stream) hipStreamSynchronize(r->stream);
  r->ws.release();
  if (r->ddev) hipFree(r->ddev);
  if (r->rb) hipHostFree(r->rb);
  for (auto& e : r->ev) if (e) hipEventDestroy(e);
  if (r->stream) hipStreamDestroy(r->stream);
  delete r;
  return SG_OK;
}

const char* sg_range_last_error(const sg_range_router* r) { return r ? r->err.c_str() : "null router"; }

}  // extern "C"
