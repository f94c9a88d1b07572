// The selector's aggregation stage: count / sum / avg / min / max per partition key and group-by key
// (QuerySelector.processGroupBy and processNoGroupBy, C/query/selector/QuerySelector.java:125-216, one match at a time
// in delivery order -- pattern output chunks are not batch chunks, so never the processInBatch* forms; aggregator
// state per partition instance and per group key, PartitionRuntime.clonePartition / AttributeAggregator.
// cloneAggregator).  Per push, over the n output records k_select made (aggregate columns hold their arguments):
//   k_agg_groups    group-by programs per record -> canonical key words -> slot of (partition key, values) in an
//                   open-addressing table in HBM (find or insert); without `group by` the slot is the partition key
//   radix sort      (slot, position) by slot, stable: each group's matches become one run, in delivery order
//   k_agg_tiles / k_agg_carry / k_agg_scan  (marked agg_tiles, agg_carry, agg_scan)
//                   segmented inclusive scan over the sorted order with the operators of agg_ops.h, every scannable
//                   column in one pass; each run seeded from its group's carried state; two-level (tile aggregates,
//                   their exclusive prefix, then the tiles again with the prefix carried in)
//   k_agg_serial    FP sum / avg (and avg over INT / LONG once a partial sum reaches 2^53): one lane walks one run
//   k_agg_writeback each run's final state back to its group
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "agg.h"
#include "agg_ops.h"
#include "sg_prim.h"

#define AGG_KW 5                 // key words per group: header (partition key | null mask << 32) + 4 values
#define AGG_EMPTY (-1)
#define AGG_BUSY (-2)
#define AGG_BLOCK 256            // threads per block = records per scan tile
#define AGG_INIT_CAP 1024        // table entries at first use (groups: half of it)
#define AGG_SPIN_LIMIT (1 << 22)

struct AggCtr {      // device counters of one push
  uint32_t n_groups;   // hashed: slots handed out; direct: 1 + the largest partition key seen
  uint32_t overflow;   // hashed: the table ran out of slots (the pass is repeated after growth)
  uint32_t error;      // a record without a partition key, or a probe that never ended
  uint32_t fallback;   // avg over INT / LONG: a run left the exact range and was redone serially
};

struct AggDev {      // kernel-argument view of the query's aggregates
  int n_out, n_agg, n_group, partitioned;
  int col[SG_MAX_AGG], kind[SG_MAX_AGG], atype[SG_MAX_AGG];
  int scan[SG_MAX_AGG];       // 1: the scan takes the column; 0: k_agg_serial
  int gtype[SG_MAX_GROUP_BY], goff[SG_MAX_GROUP_BY], glen[SG_MAX_GROUP_BY];
  int64_t code[SG_AGG_MAX_CODE];
};

struct AggStage {
  sg_agg_desc desc;
  AggDev dev;
  AggDev* ddev = nullptr;
  AggCtr* ctr = nullptr;
  int32_t* idx = nullptr;       // hashed: table entry -> slot, AGG_EMPTY, AGG_BUSY
  int64_t* keys = nullptr;      // hashed: AGG_KW words per slot
  SgAggState* st = nullptr;     // n_agg states per slot
  uint8_t* live = nullptr;      // direct: 1 once the slot's group has had a match
  int64_t cap = 0;              // hashed: table entries (power of two); slots <= cap / 2
  int64_t slots = 0;            // allocated slots of st / live / keys
  uint32_t n_groups = 0;        // hashed: groups; direct: slot bound
  bool any_scan = false, any_serial = false, any_avg_int = false;
};

struct AggReader {
  const int64_t* vals;
  uint32_t vnull;
  __device__ SgVal read(int, int, int slot, int type) { return sg_val_from_bits(vals[slot], type, (vnull >> slot) & 1); }
};

__device__ __forceinline__ uint64_t agg_mix(uint64_t x) {
  x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33;
  return x;
}
__device__ __forceinline__ uint64_t agg_hash(const int64_t* w) {
  uint64_t x = 0x9e3779b97f4a7c15ull;
  for (int k = 0; k < AGG_KW; ++k) x = agg_mix(x ^ (uint64_t)w[k]) + 0x9e3779b97f4a7c15ull;
  return x;
}

// One group-by value as the word two values share iff their Java strings are equal (GroupByKeyGenerator.java:63-73:
// the concatenated toString): every NaN one pattern, -0.0 and 0.0 as they are, null flagged by the caller.
__device__ __forceinline__ int64_t agg_canon(const SgVal& v, int type) {
  if (type == SG_T_FLOAT) { float f = (float)v.d; return f != f ? 0x7fc00000ll : (int64_t)__float_as_uint(f); }
  if (type == SG_T_DOUBLE) return v.d != v.d ? 0x7ff8000000000000ll : __double_as_longlong(v.d);
  return v.i;
}

// slot[i] of record i.  Hashed mode: entries go EMPTY -> BUSY -> slot; the claimer writes the slot's key words before
// it publishes the slot, readers take both with device-scope atomics.  A waiting lane never blocks the claimer: the
// claim runs to its end inside one iteration of the probe loop.
__global__ void __launch_bounds__(AGG_BLOCK) k_agg_groups(int64_t n, const char* __restrict__ base, int bstride,
                                                          const AggDev* __restrict__ a, int32_t* idx, int64_t* keys,
                                                          int64_t cap, uint32_t max_groups, AggCtr* ctr,
                                                          uint32_t* __restrict__ slot_out, uint32_t* __restrict__ pos_out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const char* r = base + (size_t)i * bstride;
  const int32_t pkey = *(const int32_t*)(r + 16);
  pos_out[i] = (uint32_t)i;
  if (a->n_group == 0) {   // direct: one group per partition instance, or one in all
    uint32_t s = 0;
    if (a->partitioned) {
      if (pkey < 0) { ctr->error = 1; slot_out[i] = 0; return; }
      s = (uint32_t)pkey;
    }
    if (__hip_atomic_load(&ctr->n_groups, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < s + 1) atomicMax(&ctr->n_groups, s + 1);
    slot_out[i] = s;
    return;
  }
  // a pass that has run out of slots is thrown away whole (sg_agg_run grows the table and repeats it): no more work
  if (__hip_atomic_load(&ctr->overflow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) { slot_out[i] = 0; return; }
  AggReader rd;
  rd.vals = (const int64_t*)(r + 32);
  rd.vnull = *(const uint32_t*)(r + 24);
  int64_t w[AGG_KW];
  uint64_t nullmask = 0;
  for (int g = 0; g < 4; ++g) {
    w[1 + g] = 0;
    if (g >= a->n_group) continue;
    SgVal top;
    if (!sg_run(a->code + a->goff[g], a->glen[g], rd, top)) top.null = 1;
    if (top.null) nullmask |= 1ull << g;
    else w[1 + g] = agg_canon(top, a->gtype[g]);
  }
  w[0] = (int64_t)((uint64_t)(uint32_t)(a->partitioned ? pkey : 0) | (nullmask << 32));
  uint64_t e = agg_hash(w) & (uint64_t)(cap - 1);
  uint32_t found = 0;
  int spins = 0;
  bool done = false;
  for (int64_t probes = 0; probes < cap;) {
    int32_t cur = __hip_atomic_load(&idx[e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == AGG_EMPTY) {
      cur = atomicCAS(&idx[e], AGG_EMPTY, AGG_BUSY);
      if (cur == AGG_EMPTY) {
        const uint32_t s = atomicAdd(&ctr->n_groups, 1u);
        if (s >= max_groups) {
          ctr->overflow = 1;
          atomicExch(&idx[e], AGG_EMPTY);
          done = true;
          break;
        }
        for (int k = 0; k < AGG_KW; ++k)
          __hip_atomic_store(&keys[(size_t)s * AGG_KW + k], w[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __threadfence();
        atomicExch(&idx[e], (int32_t)s);
        found = s;
        done = true;
        break;
      }
    }
    if (cur == AGG_BUSY || cur == AGG_EMPTY) {   // being claimed (or just released by an overflow): look again
      if (__hip_atomic_load(&ctr->overflow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) { done = true; break; }
      if (++spins > AGG_SPIN_LIMIT) { ctr->error = 2; break; }
      continue;
    }
    __threadfence();
    bool same = true;
    for (int k = 0; k <= a->n_group; ++k)   // (the words past the query's group-by attributes are zero in every key)
      same = same && __hip_atomic_load(&keys[(size_t)cur * AGG_KW + k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == w[k];
    if (same) { found = (uint32_t)cur; done = true; break; }
    e = (e + 1) & (uint64_t)(cap - 1);
    ++probes;
  }
  if (!done && !ctr->error) ctr->error = 2;
  slot_out[i] = found;
}

// rebuild the table from the slots' keys (no two slots share a key)
__global__ void k_agg_rehash(uint32_t n_groups, const int64_t* __restrict__ keys, int32_t* idx, int64_t cap) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_groups) return;
  uint64_t e = agg_hash(keys + (size_t)s * AGG_KW) & (uint64_t)(cap - 1);
  for (int64_t probes = 0; probes < cap; ++probes) {
    if (atomicCAS(&idx[e], AGG_EMPTY, (int32_t)s) == AGG_EMPTY) return;
    e = (e + 1) & (uint64_t)(cap - 1);
  }
}

__global__ void k_agg_heads(int64_t n, const uint32_t* __restrict__ sslot, uint32_t* __restrict__ head) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  head[j] = (j == 0 || sslot[j] != sslot[j - 1]) ? 1u : 0u;
}

__global__ void k_agg_run_starts(int64_t n, const uint32_t* __restrict__ head, const uint32_t* __restrict__ rid,
                                 uint32_t* __restrict__ run_start) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n || !head[j]) return;
  run_start[rid[j] - 1] = (uint32_t)j;
}

// ---- segmented scan -----------------------------------------------------------------------------------------------
__device__ __forceinline__ SgAggState agg_shfl_up(const SgAggState& x, int d) {
  SgAggState y;
  y.v = __shfl_up((long long)x.v, d);
  y.n = __shfl_up((long long)x.n, d);
  y.m = (uint64_t)__shfl_up((long long)x.m, d);
  y.f = (uint32_t)__shfl_up((int)x.f, d);
  y.pad = 0;
  return y;
}

// Inclusive segmented scan of one element per thread over the block, operand order kept (the operator is not
// commutative).  head: the element starts a segment.  On return x is the fold of the thread's segment from its start
// (or from the block's first element) up to the thread, and head tells whether a segment starts at or before the thread
// inside the block.  lds_x / lds_f: one entry per wave.
__device__ __forceinline__ void agg_block_segscan(int kind, int atype, SgAggState& x, int& head, SgAggState* lds_x,
                                                  int* lds_f) {
  const int lane = threadIdx.x & (warpSize - 1), wave = threadIdx.x / warpSize, nwave = blockDim.x / warpSize;
  for (int d = 1; d < warpSize; d <<= 1) {
    const SgAggState y = agg_shfl_up(x, d);
    const int yf = __shfl_up(head, d);
    if (lane >= d) {
      if (!head) x = sg_agg_combine(kind, atype, y, x);
      head |= yf;
    }
  }
  __syncthreads();   // (the previous column's readers are done with the LDS entries)
  if (lane == warpSize - 1) { lds_x[wave] = x; lds_f[wave] = head; }
  __syncthreads();
  if (wave > 0) {
    SgAggState c = lds_x[0];
    int cf = lds_f[0];
    for (int w = 1; w < wave && w < nwave; ++w) {
      if (lds_f[w]) c = lds_x[w];
      else c = sg_agg_combine(kind, atype, c, lds_x[w]);
      cf |= lds_f[w];
    }
    if (!head) x = sg_agg_combine(kind, atype, c, x);
    head |= cf;
  }
}

// element j of the sorted order for aggregate column k: the match's argument lifted, at a run's head folded onto the
// group's carried state
__device__ __forceinline__ SgAggState agg_element(const AggDev* a, int k, const SgAggState* __restrict__ st,
                                                  const char* __restrict__ out, int ostride, uint32_t slot, uint32_t pos,
                                                  int head) {
  const char* o = out + (size_t)pos * ostride;
  const uint32_t vn = *(const uint32_t*)(o + 24);
  const int c = a->col[k];
  const int64_t bits = ((const int64_t*)(o + 32))[c];
  SgAggState x = sg_agg_lift(a->kind[k], a->atype[k], bits, (vn >> c) & 1);
  if (head) x = sg_agg_combine(a->kind[k], a->atype[k], sg_agg_seed(a->kind[k], a->atype[k], st[(size_t)slot * a->n_agg + k]), x);
  return x;
}

// pass 1: per tile and scannable column, the fold of the tile's last segment and whether a segment starts in the tile
__global__ void __launch_bounds__(AGG_BLOCK) k_agg_tiles(int64_t n, const AggDev* __restrict__ a,
                                                         const SgAggState* __restrict__ st, const char* __restrict__ out,
                                                         int ostride, const uint32_t* __restrict__ sslot,
                                                         const uint32_t* __restrict__ spos, const uint32_t* __restrict__ headv,
                                                         SgAggState* __restrict__ tile_x, uint32_t* __restrict__ tile_f) {
  __shared__ SgAggState lds_x[AGG_BLOCK / 32];
  __shared__ int lds_f[AGG_BLOCK / 32];
  const int64_t j = (int64_t)blockIdx.x * AGG_BLOCK + threadIdx.x;
  const bool valid = j < n;
  const uint32_t slot = valid ? sslot[j] : 0, pos = valid ? spos[j] : 0;
  const int h0 = valid ? (int)headv[j] : 1;
  const int64_t left = n - (int64_t)blockIdx.x * AGG_BLOCK;
  const int64_t last = (left < AGG_BLOCK ? left : AGG_BLOCK) - 1;
  for (int k = 0; k < a->n_agg; ++k) {
    if (!a->scan[k]) continue;
    SgAggState x = valid ? agg_element(a, k, st, out, ostride, slot, pos, h0) : sg_agg_empty();
    int head = h0;
    agg_block_segscan(a->kind[k], a->atype[k], x, head, lds_x, lds_f);
    if ((int64_t)threadIdx.x == last) {
      tile_x[(size_t)blockIdx.x * a->n_agg + k] = x;
      tile_f[(size_t)blockIdx.x * a->n_agg + k] = (uint32_t)head;
    }
  }
}

// pass 2 (one block): tile_x becomes the exclusive prefix of the tile aggregates -- the fold of the segment that
// reaches into each tile from the tiles before it.  Every thread folds a contiguous chunk of tiles, the chunk folds are
// scanned over the block, and the chunk is walked again with its prefix.
__global__ void __launch_bounds__(AGG_BLOCK) k_agg_carry(int64_t n_tiles, const AggDev* __restrict__ a,
                                                         SgAggState* __restrict__ tile_x, const uint32_t* __restrict__ tile_f) {
  __shared__ SgAggState lds_x[AGG_BLOCK / 32];
  __shared__ int lds_f[AGG_BLOCK / 32];
  __shared__ SgAggState incl[AGG_BLOCK];
  const int64_t chunk = (n_tiles + AGG_BLOCK - 1) / AGG_BLOCK;
  const int64_t lo0 = (int64_t)threadIdx.x * chunk, lo = lo0 < n_tiles ? lo0 : n_tiles;
  const int64_t hi = lo + chunk < n_tiles ? lo + chunk : n_tiles;
  const int na = a->n_agg;
  for (int k = 0; k < na; ++k) {
    if (!a->scan[k]) continue;
    const int kind = a->kind[k], atype = a->atype[k];
    SgAggState x = sg_agg_empty();
    int head = lo >= hi ? 1 : 0;   // an empty chunk is a segment of its own: nothing flows through it
    bool have = false;
    for (int64_t t = lo; t < hi; ++t) {
      const SgAggState y = tile_x[(size_t)t * na + k];
      if (tile_f[(size_t)t * na + k] || !have) x = y;
      else x = sg_agg_combine(kind, atype, x, y);
      head |= (int)tile_f[(size_t)t * na + k];
      have = true;
    }
    agg_block_segscan(kind, atype, x, head, lds_x, lds_f);
    __syncthreads();
    incl[threadIdx.x] = x;
    __syncthreads();
    SgAggState run = threadIdx.x > 0 ? incl[threadIdx.x - 1] : sg_agg_empty();
    have = threadIdx.x > 0;
    for (int64_t t = lo; t < hi; ++t) {
      const SgAggState y = tile_x[(size_t)t * na + k];
      const uint32_t f = tile_f[(size_t)t * na + k];
      tile_x[(size_t)t * na + k] = run;
      if (f || !have) run = y;
      else run = sg_agg_combine(kind, atype, run, y);
      have = true;
    }
    __syncthreads();
  }
}

// pass 3: the tiles again with the prefix carried in; every record's aggregate columns take the running value, and a
// run's last element leaves the run's final state
__global__ void __launch_bounds__(AGG_BLOCK) k_agg_scan(int64_t n, const AggDev* __restrict__ a,
                                                        const SgAggState* __restrict__ st, char* __restrict__ out,
                                                        int ostride, const uint32_t* __restrict__ sslot,
                                                        const uint32_t* __restrict__ spos, const uint32_t* __restrict__ headv,
                                                        const uint32_t* __restrict__ rid, const SgAggState* __restrict__ tile_x,
                                                        SgAggState* __restrict__ run_state, AggCtr* ctr,
                                                        int64_t* __restrict__ avg_res, uint32_t* __restrict__ avg_null) {
  __shared__ SgAggState lds_x[AGG_BLOCK / 32];
  __shared__ int lds_f[AGG_BLOCK / 32];
  const int64_t j = (int64_t)blockIdx.x * AGG_BLOCK + threadIdx.x;
  const bool valid = j < n;
  const uint32_t slot = valid ? sslot[j] : 0, pos = valid ? spos[j] : 0;
  const int h0 = valid ? (int)headv[j] : 1;
  const bool tail = valid && (j == n - 1 || headv[j + 1]);
  const int na = a->n_agg;
  uint32_t vn = 0, an = 0;
  int64_t* ov = nullptr;
  if (valid) {
    char* o = out + (size_t)pos * ostride;
    vn = *(const uint32_t*)(o + 24);
    ov = (int64_t*)(o + 32);
  }
  // One column at a time: its argument is read (agg_element), scanned, and its result written to the same word.  Each
  // aggregate column is a word of its own, so a later column's argument is still intact; the null bits share one word,
  // which is read once above (every column's argument null bit), updated in the register vn and stored at the end.
  for (int k = 0; k < na; ++k) {
    if (!a->scan[k]) continue;
    const int kind = a->kind[k], atype = a->atype[k];
    SgAggState x = valid ? agg_element(a, k, st, out, ostride, slot, pos, h0) : sg_agg_empty();
    int head = h0;
    agg_block_segscan(kind, atype, x, head, lds_x, lds_f);
    if (valid) {
      if (!head) x = sg_agg_combine(kind, atype, tile_x[(size_t)blockIdx.x * na + k], x);
      int null = 0;
      const int c = a->col[k];
      const int64_t res = sg_agg_result(kind, atype, sg_agg_unseed(kind, atype, x), &null);
      if (kind == SG_AGG_AVG) {   // kept aside: the run may turn out inexact further on, and its redo reads the arguments
        avg_res[(size_t)j * na + k] = res;
        an |= (uint32_t)null << k;
      } else {
        ov[c] = res;
        vn = null ? (vn | (1u << c)) : (vn & ~(1u << c));
      }
      if (tail) {
        SgAggState s = sg_agg_unseed(kind, atype, x);
        s.f |= x.f & SG_AF_INEXACT;   // (k_agg_serial redoes the run)
        if (x.f & SG_AF_INEXACT) ctr->fallback = 1;
        run_state[(size_t)(rid[j] - 1) * na + k] = s;
      }
    }
  }
  if (valid) {
    *(uint32_t*)(out + (size_t)pos * ostride + 24) = vn;
    if (avg_null) avg_null[j] = an;
  }
}

// avg over INT / LONG: the scan's results into the records of the runs that stayed exact (the others were redone by
// k_agg_serial, which leaves SG_AF_INEXACT on their run state)
__global__ void k_agg_avg_apply(int64_t n, const AggDev* __restrict__ a, char* __restrict__ out, int ostride,
                                const uint32_t* __restrict__ spos, const uint32_t* __restrict__ rid,
                                const SgAggState* __restrict__ run_state, const int64_t* __restrict__ avg_res,
                                const uint32_t* __restrict__ avg_null) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const int na = a->n_agg;
  char* o = out + (size_t)spos[j] * ostride;
  uint32_t vn = *(uint32_t*)(o + 24);
  for (int k = 0; k < na; ++k) {
    if (!a->scan[k] || a->kind[k] != SG_AGG_AVG) continue;
    if (run_state[(size_t)(rid[j] - 1) * na + k].f & SG_AF_INEXACT) continue;
    const int c = a->col[k];
    ((int64_t*)(o + 32))[c] = avg_res[(size_t)j * na + k];
    vn = ((avg_null[j] >> k) & 1u) ? (vn | (1u << c)) : (vn & ~(1u << c));
  }
  *(uint32_t*)(o + 24) = vn;
}

// One lane per run for the columns whose additions must keep the serial order (FP sum / avg), and for the runs of avg
// over INT / LONG the scan marked inexact.
__global__ void __launch_bounds__(AGG_BLOCK) k_agg_serial(int64_t n, uint32_t n_runs, const AggDev* __restrict__ a,
                                                          const SgAggState* __restrict__ st, char* __restrict__ out,
                                                          int ostride, const uint32_t* __restrict__ sslot,
                                                          const uint32_t* __restrict__ spos, const uint32_t* __restrict__ run_start,
                                                          SgAggState* __restrict__ run_state) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_runs) return;
  const int64_t lo = run_start[r], hi = r + 1 < n_runs ? (int64_t)run_start[r + 1] : n;
  const uint32_t slot = sslot[lo];
  const int na = a->n_agg;
  for (int k = 0; k < na; ++k) {
    if (a->scan[k] && !(run_state[(size_t)r * na + k].f & SG_AF_INEXACT)) continue;
    const int kind = a->kind[k], atype = a->atype[k], c = a->col[k];
    SgAggState s = st[(size_t)slot * na + k];
    for (int64_t j = lo; j < hi; ++j) {
      char* o = out + (size_t)spos[j] * ostride;
      uint32_t vn = *(uint32_t*)(o + 24);
      int64_t* ov = (int64_t*)(o + 32);
      sg_agg_step(kind, atype, s, ov[c], (vn >> c) & 1);
      int null = 0;
      ov[c] = sg_agg_result(kind, atype, s, &null);
      *(uint32_t*)(o + 24) = null ? (vn | (1u << c)) : (vn & ~(1u << c));
    }
    if (a->scan[k]) s.f |= SG_AF_INEXACT;   // (k_agg_avg_apply leaves the run's records alone)
    run_state[(size_t)r * na + k] = s;
  }
}

__global__ void k_agg_writeback(uint32_t n_runs, int na, const uint32_t* __restrict__ sslot,
                                const uint32_t* __restrict__ run_start, const SgAggState* __restrict__ run_state,
                                SgAggState* __restrict__ st, uint8_t* __restrict__ live) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_runs) return;
  const uint32_t slot = sslot[run_start[r]];
  for (int k = 0; k < na; ++k) {
    SgAggState s = run_state[(size_t)r * na + k];
    s.f &= ~SG_AF_INEXACT;
    st[(size_t)slot * na + k] = s;
  }
  live[slot] = 1;
}

// ---- host ---------------------------------------------------------------------------------------------------------
static dim3 agg_grid(int64_t n) { return dim3((unsigned)((n + AGG_BLOCK - 1) / AGG_BLOCK)); }

AggStage* sg_agg_new(SgHandle& h, const sg_agg_desc* a) {
  const sg_nfa_desc& d = h.desc;
  if (a->abi_version != SG_AGG_ABI_VERSION) throw SgError(SG_EINVAL, "sg_agg_desc ABI version mismatch");
  if (a->n_out <= 0 || a->n_out != d.n_out) throw SgError(SG_EINVAL, "sg_agg_desc.n_out is not the query's");
  if (a->n_group < 0 || a->n_group > SG_MAX_GROUP_BY) throw SgError(SG_EINVAL, "bad n_group");
  if (a->code_len < 0 || a->code_len > SG_AGG_MAX_CODE) throw SgError(SG_EINVAL, "bad group-by code_len");
  AggDev v;
  memset(&v, 0, sizeof v);
  v.n_out = a->n_out;
  v.n_group = a->n_group;
  v.partitioned = d.partitioned ? 1 : 0;
  for (int k = 0; k < a->n_out; ++k) {
    if (a->kind[k] == SG_AGG_NONE) continue;
    if (a->kind[k] < SG_AGG_COUNT || a->kind[k] > SG_AGG_MAX) throw SgError(SG_EINVAL, "bad aggregate kind");
    const int rt = a->kind[k] == SG_AGG_COUNT ? SG_T_LONG : sg_agg_result_type(a->kind[k], a->arg_type[k]);
    if (rt < 0) throw SgError(SG_EINVAL, "aggregate over a type it does not take");
    if (a->res_type[k] != rt || d.out_type[k] != rt) throw SgError(SG_EINVAL, "aggregate result type mismatch");
    if (v.n_agg >= SG_MAX_AGG) throw SgError(SG_EINVAL, "more aggregate columns than SG_MAX_AGG");
    v.col[v.n_agg] = k;
    v.kind[v.n_agg] = a->kind[k];
    v.atype[v.n_agg] = a->arg_type[k];
    v.scan[v.n_agg] = sg_agg_scannable(a->kind[k], a->arg_type[k]) ? 1 : 0;
    ++v.n_agg;
  }
  if (v.n_agg == 0) throw SgError(SG_EINVAL, "sg_agg_desc without an aggregate column");
  for (int g = 0; g < a->n_group; ++g) {
    if (a->group_type[g] < SG_T_STRING || a->group_type[g] > SG_T_BOOL) throw SgError(SG_EINVAL, "bad group-by type");
    if (a->group_off[g] < 0 || a->group_len[g] < 1 || a->group_off[g] + a->group_len[g] > a->code_len)
      throw SgError(SG_EINVAL, "bad group-by program range");
    if (sg_prog_depth(a->code + a->group_off[g], a->group_len[g]) > SG_VM_STACK)
      throw SgError(SG_EUNSUPPORTED, "group-by program deeper than the VM stack");
    for (int pc = a->group_off[g]; pc < a->group_off[g] + a->group_len[g];) {   // VAR operands stay inside the record
      const int op = (int)a->code[pc];
      const int width = op == SG_OP_VAR ? 5 : (op == SG_OP_CONST || op == SG_OP_CMP || op == SG_OP_MATH) ? 3 : 1;
      if (pc + width > a->group_off[g] + a->group_len[g])
        throw SgError(SG_EINVAL, "group-by program ends inside an instruction");
      if (op == SG_OP_VAR) {
        if (a->code[pc + 3] < 0 || a->code[pc + 3] >= d.n_select) throw SgError(SG_EINVAL, "group-by slot out of range");
        pc += 5;
      } else {
        pc += (op == SG_OP_CONST || op == SG_OP_CMP || op == SG_OP_MATH) ? 3 : 1;
      }
    }
    v.gtype[g] = a->group_type[g];
    v.goff[g] = a->group_off[g];
    v.glen[g] = a->group_len[g];
  }
  memcpy(v.code, a->code, sizeof(int64_t) * (size_t)a->code_len);
  AggStage* ag = new AggStage();
  ag->desc = *a;
  ag->dev = v;
  for (int k = 0; k < v.n_agg; ++k) {
    ag->any_scan |= v.scan[k] != 0;
    ag->any_serial |= v.scan[k] == 0;
    ag->any_avg_int |= v.kind[k] == SG_AGG_AVG && !sg_agg_is_fp(v.atype[k]);
  }
  try {
    HIPCHK(hipMalloc(&ag->ddev, sizeof(AggDev)));
    HIPCHK(hipMemcpy(ag->ddev, &ag->dev, sizeof(AggDev), hipMemcpyHostToDevice));
    HIPCHK(hipMalloc(&ag->ctr, sizeof(AggCtr)));
    HIPCHK(hipMemset(ag->ctr, 0, sizeof(AggCtr)));
  } catch (...) {
    sg_agg_free(ag);
    throw;
  }
  return ag;
}

void sg_agg_free(AggStage* ag) {
  if (!ag) return;
  for (void* p : {(void*)ag->ddev, (void*)ag->ctr, (void*)ag->idx, (void*)ag->keys, (void*)ag->st, (void*)ag->live})
    if (p) hipFree(p);
  delete ag;
}

// st / live (and keys) hold at least `want` slots; new slots are empty groups (all-zero states)
static void agg_grow_slots(SgHandle& h, AggStage* ag, int64_t want) {
  if (want <= ag->slots) return;
  const int64_t ns = std::max<int64_t>(want + want / 2, 256);
  const int na = ag->dev.n_agg;
  hipStream_t s = h.stream;
  auto regrow = [&](void** p, size_t unit) {
    void* np = nullptr;
    HIPCHK(hipMalloc(&np, unit * (size_t)ns));
    HIPCHK(hipMemsetAsync(np, 0, unit * (size_t)ns, s));
    if (*p && ag->slots) HIPCHK(hipMemcpyAsync(np, *p, unit * (size_t)ag->slots, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    if (*p) HIPCHK(hipFree(*p));
    *p = np;
  };
  regrow((void**)&ag->st, sizeof(SgAggState) * (size_t)na);
  regrow((void**)&ag->live, 1);
  if (ag->dev.n_group) regrow((void**)&ag->keys, sizeof(int64_t) * AGG_KW);
  ag->slots = ns;
}

// the table holds `cap` entries, rebuilt from the keys of slots [0, n_groups)
static void agg_rebuild(SgHandle& h, AggStage* ag, int64_t cap) {
  hipStream_t s = h.stream;
  if (cap != ag->cap) {
    HIPCHK(hipStreamSynchronize(s));
    if (ag->idx) HIPCHK(hipFree(ag->idx));
    ag->idx = nullptr;
    ag->cap = 0;
    HIPCHK(hipMalloc(&ag->idx, sizeof(int32_t) * (size_t)cap));
    ag->cap = cap;
  }
  HIPCHK(hipMemsetAsync(ag->idx, 0xff, sizeof(int32_t) * (size_t)cap, s));   // AGG_EMPTY
  agg_grow_slots(h, ag, cap / 2);
  if (ag->n_groups) {
    hipLaunchKernelGGL(k_agg_rehash, agg_grid(ag->n_groups), dim3(AGG_BLOCK), 0, s, ag->n_groups, ag->keys, ag->idx, cap);
    HIPCHK(hipGetLastError());
  }
}

void sg_agg_reset(SgHandle& h, AggStage* ag) {
  if (!ag) return;
  hipStream_t s = h.stream;
  ag->n_groups = 0;
  if (ag->idx) HIPCHK(hipMemsetAsync(ag->idx, 0xff, sizeof(int32_t) * (size_t)ag->cap, s));
  if (ag->st) HIPCHK(hipMemsetAsync(ag->st, 0, sizeof(SgAggState) * (size_t)ag->dev.n_agg * (size_t)ag->slots, s));
  if (ag->live) HIPCHK(hipMemsetAsync(ag->live, 0, (size_t)ag->slots, s));
  HIPCHK(hipStreamSynchronize(s));
}

void sg_agg_run(SgHandle& h, AggStage* ag, const char* base, int bstride, char* out, int ostride, int64_t n) {
  if (n <= 0) return;
  hipStream_t s = h.stream;
  const AggDev& v = ag->dev;
  const int na = v.n_agg;
  const dim3 grd = agg_grid(n), blk(AGG_BLOCK);
  uint32_t* slot = (uint32_t*)h.ws.get("agg_slot", 4 * (size_t)n, s);
  uint32_t* pos = (uint32_t*)h.ws.get("agg_pos", 4 * (size_t)n, s);
  uint32_t* sslot = (uint32_t*)h.ws.get("agg_sslot", 4 * (size_t)n, s);
  uint32_t* spos = (uint32_t*)h.ws.get("agg_spos", 4 * (size_t)n, s);
  uint32_t* head = (uint32_t*)h.ws.get("agg_head", 4 * (size_t)(n + 1), s);
  uint32_t* rid = (uint32_t*)h.ws.get("agg_rid", 4 * (size_t)n, s);

  // ---- group slots
  h.kbeg("agg_groups");
  if (v.n_group && !ag->cap) agg_rebuild(h, ag, AGG_INIT_CAP);
  AggCtr c;
  for (;;) {
    c = AggCtr{ag->n_groups, 0, 0, 0};
    HIPCHK(hipMemcpyAsync(ag->ctr, &c, sizeof c, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_agg_groups, grd, blk, 0, s, n, base, bstride, ag->ddev, ag->idx, ag->keys, ag->cap,
                       (uint32_t)(ag->cap / 2), ag->ctr, slot, pos);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(&c, ag->ctr, sizeof c, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (c.error) throw SgError(SG_EINVAL, c.error == 1 ? "aggregation: a match without a partition key" : "aggregation: group table probe did not end");
    if (!c.overflow) break;
    // out of slots in the middle of the push: nothing of the pass is kept (slots at and above n_groups are dropped by
    // the rebuild), the table grows, the pass runs again
    if (ag->cap >= ((int64_t)1 << 31)) throw SgError(SG_ECAPACITY, "aggregation: too many groups");
    agg_rebuild(h, ag, ag->cap * 4);
  }
  ag->n_groups = c.n_groups;
  if (!v.n_group) agg_grow_slots(h, ag, ag->n_groups);
  h.kend();

  // ---- runs: stable sort by slot over the bits the slot bound needs
  h.kbeg("agg_sort");
  unsigned bits = 1;
  while (bits < 32 && (1ull << bits) < (uint64_t)ag->n_groups) ++bits;
  sg_radix_sort_pairs(h.ws, s, "agg_sort_tmp", slot, sslot, pos, spos, (size_t)n, bits);
  hipLaunchKernelGGL(k_agg_heads, grd, blk, 0, s, n, sslot, head);
  HIPCHK(hipGetLastError());
  sg_inclusive_scan(h.ws, s, "agg_scan_tmp", head, rid, (size_t)n, rocprim::plus<uint32_t>());
  const uint32_t n_runs = sg_read_back(rid + (n - 1), s);
  uint32_t* run_start = (uint32_t*)h.ws.get("agg_run_start", 4 * (size_t)n_runs, s);
  SgAggState* run_state = (SgAggState*)h.ws.get("agg_run_state", sizeof(SgAggState) * (size_t)n_runs * na, s);
  hipLaunchKernelGGL(k_agg_run_starts, grd, blk, 0, s, n, head, rid, run_start);
  HIPCHK(hipGetLastError());
  h.kend();

  // ---- scan
  int64_t* avg_res = nullptr;
  uint32_t* avg_null = nullptr;
  if (ag->any_scan) {
    const int64_t n_tiles = (n + AGG_BLOCK - 1) / AGG_BLOCK;
    SgAggState* tile_x = (SgAggState*)h.ws.get("agg_tile_x", sizeof(SgAggState) * (size_t)n_tiles * na, s);
    uint32_t* tile_f = (uint32_t*)h.ws.get("agg_tile_f", 4 * (size_t)n_tiles * na, s);
    if (ag->any_avg_int) {
      avg_res = (int64_t*)h.ws.get("agg_avg_res", 8 * (size_t)n * na, s);
      avg_null = (uint32_t*)h.ws.get("agg_avg_null", 4 * (size_t)n, s);
    }
    if (n_tiles > 1) {
      h.kbeg("agg_tiles");
      hipLaunchKernelGGL(k_agg_tiles, grd, blk, 0, s, n, ag->ddev, ag->st, out, ostride, sslot, spos, head, tile_x, tile_f);
      HIPCHK(hipGetLastError());
      h.kend();
      h.kbeg("agg_carry");
      hipLaunchKernelGGL(k_agg_carry, dim3(1), blk, 0, s, n_tiles, ag->ddev, tile_x, tile_f);
      HIPCHK(hipGetLastError());
      h.kend();
    }
    h.kbeg("agg_scan");
    hipLaunchKernelGGL(k_agg_scan, grd, blk, 0, s, n, ag->ddev, ag->st, out, ostride, sslot, spos, head, rid, tile_x,
                       run_state, ag->ctr, avg_res, avg_null);
    HIPCHK(hipGetLastError());
    h.kend();
  }
  bool fallback = false;
  if (ag->any_avg_int) fallback = sg_read_back(&ag->ctr->fallback, s) != 0;
  if (ag->any_serial || fallback) {
    h.kbeg(fallback ? "agg_serial_avg53" : "agg_serial");
    hipLaunchKernelGGL(k_agg_serial, agg_grid(n_runs), blk, 0, s, n, n_runs, ag->ddev, ag->st, out, ostride, sslot, spos,
                       run_start, run_state);
    HIPCHK(hipGetLastError());
    h.kend();
  }
  h.kbeg("agg_writeback");
  if (ag->any_avg_int) {
    hipLaunchKernelGGL(k_agg_avg_apply, grd, blk, 0, s, n, ag->ddev, out, ostride, spos, rid, run_state, avg_res, avg_null);
    HIPCHK(hipGetLastError());
  }
  hipLaunchKernelGGL(k_agg_writeback, agg_grid(n_runs), blk, 0, s, n_runs, na, sslot, run_start, run_state, ag->st, ag->live);
  HIPCHK(hipGetLastError());
  h.kend();
}

// ---- snapshot section: the groups sorted by key content (slot numbers come from atomics and differ between runs) ----
static const char AGG_MAGIC[8] = {'S', 'G', 'A', 'G', 'G', 'R', '0', '1'};

void sg_agg_snapshot(SgHandle& h, AggStage* ag, SnapW& w) {
  const int na = ag->dev.n_agg;
  const uint32_t G = ag->n_groups;
  std::vector<int64_t> keys((size_t)G * AGG_KW);
  std::vector<SgAggState> st((size_t)G * na);
  std::vector<uint8_t> live(G);
  hipStream_t s = h.stream;
  if (G) {
    HIPCHK(hipMemcpyAsync(st.data(), ag->st, sizeof(SgAggState) * st.size(), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(live.data(), ag->live, G, hipMemcpyDeviceToHost, s));
    if (ag->dev.n_group) HIPCHK(hipMemcpyAsync(keys.data(), ag->keys, 8 * keys.size(), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
  }
  if (!ag->dev.n_group)
    for (uint32_t g = 0; g < G; ++g) keys[(size_t)g * AGG_KW] = g;
  std::vector<uint32_t> order;
  for (uint32_t g = 0; g < G; ++g)
    if (live[g]) order.push_back(g);
  std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
    return std::lexicographical_compare(&keys[(size_t)x * AGG_KW], &keys[(size_t)x * AGG_KW] + AGG_KW,
                                        &keys[(size_t)y * AGG_KW], &keys[(size_t)y * AGG_KW] + AGG_KW);
  });
  w.put(AGG_MAGIC, 8);
  w.pod((uint32_t)order.size());
  w.pod((uint32_t)na);
  for (uint32_t g : order) {
    w.put(&keys[(size_t)g * AGG_KW], 8 * AGG_KW);   // header word (partition key | null flags << 32), then the values
    for (int k = 0; k < na; ++k) {
      const SgAggState& x = st[(size_t)g * na + k];
      w.pod(x.v);
      w.pod(x.n);
      w.pod(x.f);
    }
  }
}

void sg_agg_restore(SgHandle& h, AggStage* ag, SnapR& r) {
  const int na = ag->dev.n_agg;
  if (memcmp(r.take(8), AGG_MAGIC, 8) != 0) throw SgError(SG_EINVAL, "snapshot without the aggregation section");
  const uint32_t G = r.pod<uint32_t>();
  if (r.pod<uint32_t>() != (uint32_t)na) throw SgError(SG_EINVAL, "snapshot of other aggregates");
  if ((size_t)(r.e - r.p) / (8 * AGG_KW + 20 * (size_t)na) < G) throw SgError(SG_EINVAL, "snapshot blob truncated");
  std::vector<int64_t> keys((size_t)G * AGG_KW);
  std::vector<SgAggState> st((size_t)G * na);
  for (uint32_t g = 0; g < G; ++g) {
    memcpy(&keys[(size_t)g * AGG_KW], r.take(8 * AGG_KW), 8 * AGG_KW);
    for (int k = 0; k < na; ++k) {
      SgAggState x = sg_agg_empty();
      x.v = r.pod<int64_t>();
      x.n = r.pod<int64_t>();
      x.f = r.pod<uint32_t>();
      st[(size_t)g * na + k] = x;
    }
  }
  // the groups as sg_agg_snapshot writes them: strictly increasing key words (so no key twice), the words past the
  // query's group-by attributes zero; without `group by` the header word alone, a partition key below 2^28 (0 for an
  // unpartitioned query).  A damaged section is refused before anything is sized by it.
  for (uint32_t g = 0; g < G; ++g) {
    const int64_t* k = &keys[(size_t)g * AGG_KW];
    if (g && !std::lexicographical_compare(k - AGG_KW, k, k, k + AGG_KW)) throw SgError(SG_EINVAL, "snapshot: group keys out of order");
    for (int j = 1 + ag->dev.n_group; j < AGG_KW; ++j)
      if (k[j]) throw SgError(SG_EINVAL, "snapshot: bad group key");
    if (!ag->dev.n_group && (k[0] < 0 || k[0] >= ((int64_t)1 << 28) || (!ag->dev.partitioned && k[0])))
      throw SgError(SG_EINVAL, "snapshot: bad group key");
  }
  sg_agg_reset(h, ag);
  if (!G) return;
  hipStream_t s = h.stream;
  if (ag->dev.n_group) {
    int64_t cap = std::max<int64_t>(ag->cap, AGG_INIT_CAP);
    while (cap / 2 < (int64_t)G) cap *= 4;
    ag->n_groups = 0;
    agg_rebuild(h, ag, cap);   // (sizes the slots; nothing to rehash yet)
    HIPCHK(hipMemcpyAsync(ag->keys, keys.data(), 8 * keys.size(), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(ag->st, st.data(), sizeof(SgAggState) * st.size(), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(ag->live, 1, G, s));
    ag->n_groups = G;
    hipLaunchKernelGGL(k_agg_rehash, agg_grid(G), dim3(AGG_BLOCK), 0, s, G, ag->keys, ag->idx, ag->cap);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    return;
  }
  // direct: the header word is the slot
  int64_t bound = 0;
  for (uint32_t g = 0; g < G; ++g) {
    const int64_t k = keys[(size_t)g * AGG_KW];
    bound = k + 1;   // (checked above: increasing, below 2^28)
  }
  agg_grow_slots(h, ag, bound);
  std::vector<SgAggState> dense((size_t)bound * na, sg_agg_empty());
  std::vector<uint8_t> live((size_t)bound, 0);
  for (uint32_t g = 0; g < G; ++g) {
    const int64_t k = keys[(size_t)g * AGG_KW];
    for (int c = 0; c < na; ++c) dense[(size_t)k * na + c] = st[(size_t)g * na + c];
    live[k] = 1;
  }
  HIPCHK(hipMemcpyAsync(ag->st, dense.data(), sizeof(SgAggState) * dense.size(), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(ag->live, live.data(), live.size(), hipMemcpyHostToDevice, s));
  HIPCHK(hipStreamSynchronize(s));
  ag->n_groups = (uint32_t)bound;
}

uint64_t sg_agg_fingerprint(const AggStage* ag, uint64_t x) {
  const sg_agg_desc& a = ag->desc;
  auto mix = [&](int64_t v) {
    for (int b = 0; b < 8; ++b) { x ^= (uint64_t)((v >> (8 * b)) & 0xff); x *= 1099511628211ull; }
  };
  mix(0x41474752);
  mix(a.n_out);
  for (int k = 0; k < a.n_out; ++k) { mix(a.kind[k]); mix(a.kind[k] ? a.arg_type[k] : 0); mix(a.kind[k] ? a.res_type[k] : 0); }
  mix(a.n_group);
  for (int g = 0; g < a.n_group; ++g) {
    mix(a.group_type[g]);
    mix(a.group_len[g]);
    for (int k = 0; k < a.group_len[g]; ++k) mix(a.code[a.group_off[g] + k]);
  }
  return x;
}
