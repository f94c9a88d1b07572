// ranges.hip -- the device range router (sg_range_*, include/siddhi_gpu.h): PartitionStreamReceiver with
// RangePartitionExecutors (C/partition/PartitionStreamReceiver.java:94-100,110-125,270-275;
// C/partition/executor/RangePartitionExecutor.java:38-43) over one SoA batch, in three passes:
//
//   hold    (ranges.h, shared with the node pipeline) one thread per row runs the range conditions of the row's stream
//           through the postfix VM (sg_device.h) -> a 32-bit hold mask per row, the copy count
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

#include "ranges.h"
#include "sg_prim.h"

namespace {

const uint64_t RR_NONE = ~0ull;
// slot entries of the expand pass: row in tile | what << 8 (what < 32: a range; else one of these)
const uint32_t RR_PASS = 0x40, RR_CLOCK = 0x41;

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
  rr_for_each_read_col(d, [&](int c) {   // every column a range program reads must be there
    if (!cols.col[c]) throw SgError(SG_EINVAL, "batch is missing a column a range condition reads");
  });

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
  rr_launch_hold(r.depth, st, (unsigned)ntiles, in, cols, r.ddev, lk, masks, cnt, mins);
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
    r->depth = rr_validate(r->desc);
    HIPCHK(hipSetDevice(hip_device));
    HIPCHK(hipStreamCreateWithFlags(&r->stream, hipStreamNonBlocking));
    for (auto& e : r->ev) HIPCHK(hipEventCreate(&e));
    HIPCHK(hipHostMalloc((void**)&r->rb, sizeof(Readback), hipHostMallocDefault));
    const RrDev hd = rr_dev_image(*d);
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
