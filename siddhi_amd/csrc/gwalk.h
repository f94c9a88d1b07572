// gwalk.h -- the closed form's group walker: `every A[l] -> B[l' and B.x OP A.x] within T` when the partition has
// many keys with few rows each (C5: 1M keys, ~500 rows per key per 500M-row push, ~10 rows per `within` window).
// Kernels first, then the host side (gw_plan, run_group_walk); run_every_next (engine_impl.h) tries run_group_walk
// after the partition's group passes (keypart.h part1_wide).  The delivery side -- the trigger-word format, the tile
// counts and the projection kernel -- is gw_proj.h.
//
// Semantics are those of the tiled walker (walk.h Walker::step, itself StreamPreStateProcessor.isExpired /
// processAndReturn, C/query/input/stream/state/StreamPreStateProcessor.java:102-113,292-337, and
// StreamPostStateProcessor.process, StreamPostStateProcessor.java:53-72): per key, e2's pending list in arrival order,
// an arriving row first drops the partials older than `within`, then completes every pending partial its compare
// accepts (delivered oldest first), then appends itself when it passes A's filter.
//
// What differs is where the work happens.  The tiled path sorts every group's rows by key into HBM (part_key),
// re-lays them out as lane-interleaved tiles (tile_transpose), walks them twice (walk_count, then walk_record with a
// random read of every emitting row's output offset) and projects.  Here one workgroup owns one group of 256 keys --
// lane t walks key 256g + t -- and streams the group's rows (pass 1b's output: the group's rows in arrival order,
// 16-byte walker records plus a 1-byte in-group key) through LDS in chunks: a stable counting sort of the chunk by
// in-group key in LDS, then every lane walks its own rows from LDS with its pending list in an LDS ring.  One walk,
// no key-sorted copy in HBM, no tiles.  Each trigger row writes one 8-byte word at its arrival position (where its
// matches start in the match area, and how many); the matches themselves go to the key's region of the match area
// in walk order: a 16-byte header per trigger (e2's time, key, compared value, payload) and 8 bytes per completed
// partial (e1's compared value, payload) -- written sequentially by the lane.  A scan over the trigger words in
// arrival order gives each trigger's first output slot, and the projection walks the triggers in arrival order,
// so the output records are written contiguously and in delivery order.
//
// Trigger words are not cleared per push.  A word is unit (32) | matches (24) | epoch (8); the epoch
// is a per-handle counter in 1..255 that advances with every group-walked push, and a word of any other epoch reads
// as "no trigger" -- what an earlier push, or a push the walker declined half way, left behind.  The buffer is
// cleared only where it could hold untagged bytes (a new allocation, words past the high-water mark) and when the
// epochs wrap (gw_tagged_words).
//
// The fast path declines (run_group_walk returns 0, nothing changed) when a push needs what only the tiled path has: a key
// whose time goes back (the exact HBM-list walker), a pending list longer than the LDS ring, e1 attributes gathered
// by row, or a select reading anything but the compared values and the carried payload.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "gw_proj.h"
#include "keypart.h"
#include "sg_engine.h"
#include "sg_prim.h"
#include "walk.h"

struct GwArgs {
  int64_t n, nc;              // batch rows; carried rows (virtual rows [0, nc))
  int64_t within;
  int64_t t0;                 // narrow records' time origin (the push's first virtual row)
  uint32_t K, nc1;            // keys; columns per group of the group table (o1 stride)
  int32_t stack_mode;
  int32_t cap;                // LDS ring entries per lane (power of two)
  int32_t chunk;              // rows per LDS chunk (multiple of 256)
  int32_t carry_out;
  int32_t pzero;              // payload bits zero-extended (FLOAT) rather than sign-extended
  const uint32_t* o1;         // group g's rows: [o1[g * nc1], o1[(g + 1) * nc1])
  const PtU4* grec;           // pass 1b's records, grouped by group, arrival order within a group
  const uint8_t* glk;         // in-group key of each record
  const uint32_t* kbase;      // per key: its first row in the group domain (k_gw_count); kbase[K]: the row count
  uint64_t* trig;             // per batch row: gw_trig_word(match-area unit of its header, matches, epoch)
  uint32_t epoch;             // this push's tag (1..255): a word tagged otherwise is no trigger
  uint64_t* area;             // match area, 8-byte units: 3 per row of the key
  int64_t* cv_ts;             // carry: every key's final pending list as values
  int32_t* cv_key;
  int64_t* cv_val;
  int64_t* cv_pay;
  uint32_t* cv_n;
  uint32_t cv_cap;
  uint32_t* flags;            // GW_ORDER | GW_OVERFLOW | GW_INTERNAL | GW_CARRY_FULL
  uint32_t* ovf_keys;         // keys whose pending list outgrew the LDS ring (walked again by k_gw_redo)
  uint32_t* ovf_n;
  uint32_t ovf_cap;
  uint32_t* match_n;          // matches of the push (the projection's output size)
};
static const uint32_t GW_ORDER = 1, GW_OVERFLOW = 2, GW_INTERNAL = 4, GW_CARRY_FULL = 8;

// per-key rows of every group (LDS counters over the group's in-group keys, read 16 bytes per lane between a scalar
// head and tail) -> each key's first row in the group domain: the group's keys lie one after the other from the
// group's own first row, so kbase[k] = o1[g * nc1] + the rows of the group's keys before k; kbase[K] = the row count
static __global__ void __launch_bounds__(256) k_gw_count(const uint32_t* __restrict__ o1, uint32_t nc1, uint32_t K,
                                                         const uint8_t* __restrict__ glk, uint32_t* __restrict__ kbase) {
  __shared__ uint32_t c[4][256];
  __shared__ uint32_t wsum[4];
  const uint32_t g = blockIdx.x, t = threadIdx.x, w = t >> 6;
#pragma unroll
  for (int q = 0; q < 4; ++q) c[q][t] = 0;
  __syncthreads();
  const uint32_t lo = o1[(size_t)g * nc1], hi = o1[(size_t)(g + 1) * nc1];
  const uint32_t mis = (uint32_t)(16u - ((uintptr_t)(glk + lo) & 15u)) & 15u;
  const uint32_t a0 = min(hi, lo + mis);   // the first 16-byte aligned position (or the end)
  const uint32_t nv = (hi - a0) >> 4;      // whole 16-byte words from there
  const uint32_t a1 = a0 + (nv << 4);
  if (t < a0 - lo) atomicAdd(&c[w][glk[lo + t]], 1u);
  if (t < hi - a1) atomicAdd(&c[w][glk[a1 + t]], 1u);
  const PtU4* v = (const PtU4*)(glk + a0);
  auto count = [&](const PtU4& x) {
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int b = 0; b < 32; b += 8) atomicAdd(&c[w][(x[q] >> b) & 255u], 1u);
  };
  for (uint32_t i = t; i < nv; i += 512) {   // two words per lane in flight
    const PtU4 x0 = v[i];
    const bool two = i + 256 < nv;
    const PtU4 x1 = v[two ? i + 256 : i];
    count(x0);
    if (two) count(x1);
  }
  __syncthreads();
  const uint32_t n = c[0][t] + c[1][t] + c[2][t] + c[3][t];
  const uint32_t first = lo + block_excl_scan256(n, wsum);
  const uint32_t k = (g << 8) + t;
  if (k < K) kbase[k] = first;
  if (k + 1 == K) kbase[K] = first + n;
}

template <int PT>
struct GwLds {
  PtU4 stage[256 * PT];
  uint32_t cw[4][256];
  uint32_t ls[256], tot[256];
  uint32_t wsum[4];
};

// Pending list of one key: an LDS ring of `cap` entries per lane (lane-strided planes: conflict-free), or -- for a key
// whose list outgrew the ring (k_gw_redo) -- unbounded HBM planes over the key's own rows.
template <class T>
struct GwLdsRing {
  T* v;
  int32_t* t;
  int32_t* p;
  uint32_t cmask, lane;
  __device__ __forceinline__ uint32_t ix(uint32_t s) const { return (s & cmask) * 256 + lane; }
  __device__ __forceinline__ bool full(uint32_t head, uint32_t top) const { return top - head == cmask + 1; }
};
template <class T>
struct GwHbmRing {
  T* v;
  int32_t* t;
  int32_t* p;
  __device__ __forceinline__ uint32_t ix(uint32_t s) const { return s; }
  __device__ __forceinline__ bool full(uint32_t, uint32_t) const { return false; }
};

// One key's walk state and step (the reference's per-event processing of e2's pending list, see the file header).
template <class T, int OP, bool STACK, class RING>
struct GwLane {
  RING R;
  uint32_t head = 0, top = 0;
  int32_t hts = 0, prev = INT32_MIN;
  T tv = T();
  bool bad = false;
  bool big = false;   // a trigger completed more partials than a trigger word counts (an unbounded list only)
  uint64_t cur = 0;   // next free unit of the key's match-area region
  uint32_t k = 0;
  uint32_t nm = 0;    // matches delivered
  // `within` compares in 32 bits: a key's times never go back on this path (such a push is redone on the tiled
  // path), so dts - hts is a non-negative difference of two 32-bit offsets and fits an unsigned 32-bit word
  uint32_t wi = 0;
  // returns false when the row would overflow the ring: the lane stops and k_gw_redo walks the whole key again
  __device__ __forceinline__ bool step(const GwArgs& a, const PtU4& q) {
    const int32_t dts = (int32_t)q.x;
    const uint32_t rowf = q.y;
    T x;
    const uint32_t xb = q.z;
    __builtin_memcpy(&x, &xb, sizeof(T));
    const int32_t pay = (int32_t)q.w;
    const uint32_t f = rowf >> 30;
    bad |= dts < prev;   // every row of the key takes part in the order check
    prev = dts;
    if (!f) return true;
    const bool live = !is_nan_val<T>(x);
    // lazy `within` expiry of the oldest partials (isExpired :102-113)
    if (head != top && (uint32_t)(dts - hts) > wi) {
      ++head;
      while (head != top) {
        hts = R.t[R.ix(head)];
        if ((uint32_t)(dts - hts) <= wi) break;
        ++head;
      }
    }
    const uint32_t r = rowf & ROW_MASK;
    uint32_t m = 0;
    if ((f & F_CONS) && live) {
      const bool emit = r >= (uint32_t)a.nc;   // a carried row completes nothing it did not complete before
      const uint64_t hdr = cur;
      if constexpr (STACK) {
        // monotone stack: the completed partials are exactly a suffix, delivered oldest first
        if (top != head && cmp_op<T>(OP, x, tv)) {
          --top;
          ++m;
          while (top != head) {
            tv = R.v[R.ix(top - 1)];
            if (!cmp_op<T>(OP, x, tv)) break;
            --top;
            ++m;
          }
        }
        if (emit && m) {
          for (uint32_t e = 0; e < m; ++e) {
            const uint32_t s = R.ix(top + e);
            a.area[hdr + 2 + e] = (uint64_t)(uint32_t)val_bits<T>(R.v[s]) | ((uint64_t)(uint32_t)R.p[s] << 32);
          }
        }
      } else {
        uint32_t wr = head;
        for (uint32_t s = head; s != top; ++s) {
          const uint32_t si = R.ix(s);
          const T e = R.v[si];
          if (cmp_op<T>(OP, x, e)) {
            if (emit) a.area[hdr + 2 + m] = (uint64_t)(uint32_t)val_bits<T>(e) | ((uint64_t)(uint32_t)R.p[si] << 32);
            ++m;
          } else {
            if (wr != s) {
              const uint32_t wx = R.ix(wr);
              R.v[wx] = e;
              R.t[wx] = R.t[si];
              R.p[wx] = R.p[si];
            }
            ++wr;
          }
        }
        top = wr;
        if (head != top) {
          hts = R.t[R.ix(head)];
          tv = R.v[R.ix(top - 1)];
        }
      }
      if (emit && m) {
        const uint64_t b = r - (uint32_t)a.nc;
        a.area[hdr] = (uint64_t)(uint32_t)dts | ((uint64_t)k << 32);
        a.area[hdr + 1] = (uint64_t)(uint32_t)val_bits<T>(x) | ((uint64_t)(uint32_t)pay << 32);
        big |= m > GW_MATCH_MAX;
        a.trig[b] = gw_trig_word(hdr, m & GW_MATCH_MAX, a.epoch);
        cur = hdr + 2 + m;
        nm += m;
      }
    }
    if ((f & F_CAND) && live) {
      if (R.full(head, top)) return false;
      const uint32_t s = R.ix(top);
      R.v[s] = x;
      R.t[s] = dts;
      R.p[s] = pay;
      if (top == head) hts = dts;
      tv = x;
      ++top;
    }
    return true;
  }
  // the key's final pending list as carried value rows
  __device__ __forceinline__ void carry(const GwArgs& a, uint32_t o) const {
    for (uint32_t e = 0; e < top - head; ++e) {
      const uint32_t s = R.ix(head + e);
      a.cv_ts[o + e] = a.t0 + (int64_t)R.t[s];
      a.cv_key[o + e] = (int32_t)k;
      a.cv_val[o + e] = val_bits<T>(R.v[s]);
      a.cv_pay[o + e] = a.pzero ? (int64_t)(uint32_t)R.p[s] : (int64_t)R.p[s];
    }
  }
};

template <class T, int OP, int PT, bool STACK>
__global__ void __launch_bounds__(256, 1) k_gwalk(GwArgs a) {
  extern __shared__ __attribute__((aligned(16))) char lds_raw[];
  GwLds<PT>& L = *(GwLds<PT>*)lds_raw;
  const uint32_t cap = (uint32_t)a.cap;
  const uint32_t t = threadIdx.x, w = t >> 6, lane = t & 63;
  const uint32_t g = xcd_block(blockIdx.x, gridDim.x);
  const uint32_t k = (g << 8) + t;
  const bool active = k < a.K;
  const uint32_t lo = a.o1[(size_t)g * a.nc1], hi = a.o1[(size_t)(g + 1) * a.nc1];
  GwLane<T, OP, STACK, GwLdsRing<T>> W;
  W.R.v = (T*)(lds_raw + sizeof(GwLds<PT>));            // ring planes [cap][256]: value, time, payload
  W.R.t = (int32_t*)(W.R.v + (size_t)cap * 256);
  W.R.p = W.R.t + (size_t)cap * 256;
  W.R.cmask = cap - 1;
  W.R.lane = t;
  W.k = k;
  W.wi = a.within > 0xffffffffll ? 0xffffffffu : (uint32_t)a.within;
  W.cur = active ? 3ull * a.kbase[k] : 0ull;
  bool ovf = false;
  const uint32_t ROWS = 256 * PT;
  PtU4 rc[PT], rn[PT];
  uint32_t tg[PT], tn[PT];
  // (the loads only issue here: nothing reads the registers before the next chunk's sort, so the next chunk's loads
  // stay in flight during this chunk's walk; rows past the group's end re-read its last row and are masked at use)
  auto load = [&](uint32_t base, PtU4* r, uint32_t* d) {
    const uint32_t rows = min(ROWS, hi - base);
#pragma unroll
    for (int s = 0; s < PT; ++s) {
      const uint32_t i = w * (PT * 64) + s * 64 + lane;
      const uint32_t p = base + (i < rows ? i : rows - 1);
      r[s] = __builtin_nontemporal_load(a.grec + p);
      d[s] = a.glk[p];
    }
  };
  if (lo < hi) load(lo, rc, tg);
  for (uint32_t base = lo; base < hi; base += ROWS) {
    {
      const uint32_t rows = min(ROWS, hi - base);
#pragma unroll
      for (int s = 0; s < PT; ++s)
        if (w * (PT * 64) + s * 64 + lane >= rows) tg[s] = 0xffffffffu;
    }
    // stable counting sort of the chunk by in-group key (wave ballots rank equal keys in arrival order)
#pragma unroll
    for (int q = 0; q < 4; ++q) L.cw[q][t] = 0;
    __syncthreads();
#pragma unroll
    for (int s = 0; s < PT; ++s)
      if (tg[s] != 0xffffffffu) atomicAdd(&L.cw[w][tg[s]], 1u);
    __syncthreads();
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
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < PT; ++s) {
      const bool valid = tg[s] != 0xffffffffu;
      const uint32_t d = valid ? tg[s] : 0u;
      uint32_t rank, cnt;
      peer_rank(valid, d, 8, rank, cnt);
      if (valid) {
        const uint32_t slot = L.cw[w][d] + rank;
        if (rank == 0) L.cw[w][d] = slot + cnt;
        L.stage[slot] = rc[s];
      }
    }
    if (base + ROWS < hi) load(base + ROWS, rn, tn);   // next chunk in flight during the walk
    __syncthreads();
    // walk: lane t's rows of this chunk, in arrival order
    const uint32_t i0 = L.ls[t], i1 = i0 + L.tot[t];
    for (uint32_t i = i0; i < i1 && active && !ovf; ++i)
      if (!W.step(a, L.stage[i])) ovf = true;
    __syncthreads();
#pragma unroll
    for (int s = 0; s < PT; ++s) { rc[s] = rn[s]; tg[s] = tn[s]; }
  }
  uint32_t fl = W.bad ? GW_ORDER : 0u;
  // (3 units per row bound the key's region: a header per trigger row, one unit per completed candidate row)
  if (active && W.cur > 3ull * a.kbase[k + 1]) fl |= GW_INTERNAL;
  if (ovf) {   // the key's list outgrew the ring: the whole key again on an HBM list (k_gw_redo)
    const uint32_t o = atomicAdd(a.ovf_n, 1u);
    if (o < a.ovf_cap) a.ovf_keys[o] = k;
    else fl |= GW_OVERFLOW;
  }
  if (fl) atomicOr(a.flags, fl);
  {
    uint32_t c = (active && !ovf) ? W.nm : 0u;   // (a redone key counts its matches in k_gw_redo)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += (uint32_t)__shfl_xor((int)c, o);
    if (lane == 0 && c) atomicAdd(a.match_n, c);
  }
  if (!a.carry_out) return;
  // the key's final pending list is the carry: slots reserved once per wave
  const uint32_t m = (active && !ovf) ? W.top - W.head : 0u;
  uint32_t incl = m;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t y = (uint32_t)__shfl_up((int)incl, o);
    if ((int)lane >= o) incl += y;
  }
  const uint32_t tot = (uint32_t)__shfl((int)incl, 63);
  if (!tot) return;
  uint32_t cb = 0;
  if (lane == 63) cb = atomicAdd(a.cv_n, tot);
  cb = (uint32_t)__shfl((int)cb, 63);
  if ((uint64_t)cb + tot > (uint64_t)a.cv_cap) {
    if (lane == 63) atomicOr(a.flags, GW_CARRY_FULL);
    return;
  }
  if (m) W.carry(a, cb + incl - m);
}

// A key whose pending list outgrew the LDS ring, walked again from its first row with an unbounded list: one
// workgroup per such key gathers the key's rows from its group (arrival order kept) into the key's slice of `rows`,
// then one lane walks them (staged in LDS with the list when the key has at most GW_REDO_LDS rows, else from HBM with
// the list in HBM planes over the key's rows), rewriting the key's match-area region,
// its trigger words (under the push's epoch, as the first walk tagged them) and its carry from the start (same walk,
// same rows: the same words the first walk wrote up to the overflow, then the rest).
static const uint32_t GW_REDO_LDS = 2048;   // rows of a redone key walked from LDS
template <class T, int OP, bool STACK>
__global__ void __launch_bounds__(256) k_gw_redo(GwArgs a, uint32_t* __restrict__ rows, T* __restrict__ hv,
                                                 int32_t* __restrict__ ht, int32_t* __restrict__ hp) {
  __shared__ uint32_t wc[4], base_s;
  __shared__ PtU4 red_stage[GW_REDO_LDS];
  __shared__ T red_v[GW_REDO_LDS];
  __shared__ int32_t red_t[GW_REDO_LDS], red_p[GW_REDO_LDS];
  const uint32_t k = a.ovf_keys[blockIdx.x];
  const uint32_t g = k >> 8, d = k & 255u, t = threadIdx.x, w = t >> 6, lane = t & 63;
  const uint32_t lo = a.o1[(size_t)g * a.nc1], hi = a.o1[(size_t)(g + 1) * a.nc1];
  const uint32_t kb = a.kbase[k], ke = a.kbase[k + 1];
  if (t == 0) base_s = 0;
  __syncthreads();
  for (uint32_t p0 = lo; p0 < hi; p0 += 256) {
    const uint32_t p = p0 + t;
    const bool mine = p < hi && a.glk[p] == d;
    const uint64_t bm = __ballot(mine);
    const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(bm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bm, 0u));
    if (lane == 0) wc[w] = (uint32_t)__popcll(bm);
    __syncthreads();
    uint32_t before = base_s;
    for (uint32_t q = 0; q < w; ++q) before += wc[q];
    if (mine && kb + before + below < ke) rows[kb + before + below] = p;
    __syncthreads();
    if (t == 0) base_s += wc[0] + wc[1] + wc[2] + wc[3];
    __syncthreads();
  }
  const uint32_t nk = ke - kb;
  const bool in_lds = nk <= GW_REDO_LDS;   // (C5's keys: ~500 rows) records and list in LDS, else both in HBM
  if (in_lds)
    for (uint32_t i = t; i < nk; i += 256) red_stage[i] = a.grec[rows[kb + i]];
  __syncthreads();
  if (t != 0) return;
  if (kb + base_s != ke) { atomicOr(a.flags, GW_INTERNAL); return; }
  GwLane<T, OP, STACK, GwHbmRing<T>> W;
  if (in_lds) {
    W.R.v = red_v;
    W.R.t = red_t;
    W.R.p = red_p;
  } else {
    W.R.v = hv + kb;
    W.R.t = ht + kb;
    W.R.p = hp + kb;
  }
  W.k = k;
  W.wi = a.within > 0xffffffffll ? 0xffffffffu : (uint32_t)a.within;
  W.cur = 3ull * kb;
  if (in_lds) for (uint32_t i = 0; i < nk; ++i) W.step(a, red_stage[i]);
  else for (uint32_t i = kb; i < ke; ++i) W.step(a, a.grec[rows[i]]);
  uint32_t fl = W.bad ? GW_ORDER : 0u;
  if (W.cur > 3ull * ke) fl |= GW_INTERNAL;
  if (W.big) fl |= GW_OVERFLOW;   // 2^24 or more matches of one trigger: the tiled path (the LDS ring holds 32)
  if (fl) atomicOr(a.flags, fl);
  if (W.nm) atomicAdd(a.match_n, W.nm);
  if (!a.carry_out) return;
  const uint32_t m = W.top - W.head;
  if (!m) return;
  const uint32_t o = atomicAdd(a.cv_n, m);
  if ((uint64_t)o + m > (uint64_t)a.cv_cap) { atomicOr(a.flags, GW_CARRY_FULL); return; }
  W.carry(a, o);
}

// ---------------------------------------------------------------------------------------------
// Host side of the group walker: whether a query and a push can take it (gw_plan), and one push through it
// (run_group_walk).
struct GwPlan {
  bool ok = false;
  int cap = 0;
  GwSel sel;
};
// span_ms: time from the push's first to its last batch row (the ring is sized as the tiled walker sizes it)
template <class T>
static GwPlan gw_plan(SgHandle* h, const BatchView& bv, int64_t n, int64_t nc, uint32_t kb, const PushPlan& plan,
                      bool same_col, int64_t span_ms) {
  const sg_nfa_desc& d = h->desc;
  GwPlan g;
  memset(&g.sel, 0, sizeof(g.sel));
  if (!d.partitioned || !same_col || plan.e1_row || d.n_select > SG_MAX_SELECT) return g;
  for (int c = 0; c < d.n_cols; ++c)
    if (bv.cols.nul[c]) return g;
  for (int s = 0; s < d.n_select; ++s) {
    const int src = plan.pp.src[s], kind = plan.pp.kind[s];
    int code = -1;
    if (kind == 2) code = 4;
    else if (kind == 0 && src == 0) code = 0;
    else if (kind == 1) code = src ? 2 : 1;
    else if (kind == 3 && src == 1 && plan.pcol >= 0 && plan.pp.col[s] == plan.pcol) code = 3;
    if (code < 0) return g;
    g.sel.codes[s >> 4] |= (uint64_t)code << (4 * (s & 15));
    if (code == 4) g.sel.nmask |= 1u << s;
  }
  const int64_t win = window_rows(kb, nc + n, d.within, span_ms);
  // the ring as the tiled walker sizes it (a key whose list outgrows it is walked again on an unbounded list by
  // k_gw_redo); the LDS chunk shrinks as the ring grows so two workgroups share a CU (launch_gwalk)
  const char* e = getenv("SG_DEBUG_GW_CAP");   // (test hook)
  int cap = h->opt.ring_cap > 0 ? h->opt.ring_cap : (e ? atoi(e) : pick_cap(win));
  if (cap > 32 || cap < 2 || (cap & (cap - 1))) return g;
  g.cap = cap;
  g.sel.n_select = d.n_select;
  g.sel.stride = 32 + 8 * d.n_select;
  g.sel.vfloat = std::is_same<T, float>::value ? 1 : 0;
  g.ok = true;
  return g;
}

template <class T, int OP, int PT, bool STACK>
static void launch_gwalk_pt(const GwArgs& ga, uint32_t ng, hipStream_t st) {
  const size_t lds = sizeof(GwLds<PT>) + (size_t)ga.cap * 256 * (sizeof(T) + 8);
  HIPCHK(hipFuncSetAttribute((const void*)k_gwalk<T, OP, PT, STACK>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL((k_gwalk<T, OP, PT, STACK>), dim3(ng), dim3(256), lds, st, ga);
  HIPCHK(hipGetLastError());
}
template <class T, int OP>
static void launch_gw_redo(const GwArgs& ga, uint32_t nk, uint32_t* rows, T* hv, int32_t* ht, int32_t* hp, hipStream_t st) {
  if (ga.stack_mode) hipLaunchKernelGGL((k_gw_redo<T, OP, true>), dim3(nk), dim3(256), 0, st, ga, rows, hv, ht, hp);
  else hipLaunchKernelGGL((k_gw_redo<T, OP, false>), dim3(nk), dim3(256), 0, st, ga, rows, hv, ht, hp);
  HIPCHK(hipGetLastError());
}
template <class T, int OP>
static void launch_gwalk(const GwArgs& ga, uint32_t ng, hipStream_t st) {
  // rows per thread per LDS chunk: the largest that leaves room for two workgroups per CU beside the ring (measured on
  // C5, profiles/r06/ab_gw.sh: 8 with an 8-entry ring, 6 with 16; with 32 one workgroup per CU whatever the chunk)
  const char* e = getenv("SG_DEBUG_GW_PT");   // (test hook)
  const int pt = e ? atoi(e) : (ga.cap <= 8 ? 8 : ga.cap <= 16 ? 6 : 4);
  if (ga.stack_mode) {
    if (pt == 4) launch_gwalk_pt<T, OP, 4, true>(ga, ng, st);
    else if (pt == 12) launch_gwalk_pt<T, OP, 12, true>(ga, ng, st);
    else if (pt == 10) launch_gwalk_pt<T, OP, 10, true>(ga, ng, st);
    else if (pt == 6) launch_gwalk_pt<T, OP, 6, true>(ga, ng, st);
    else launch_gwalk_pt<T, OP, 8, true>(ga, ng, st);
  } else {
    launch_gwalk_pt<T, OP, 8, false>(ga, ng, st);
  }
}

// Words of a named workspace that are tagged with the push's epoch instead of being cleared per push: clears what
// could hold anything but zero or a word tagged since the last clear -- everything after the workspace was allocated
// anew (ws.get never zeroes), the words past the high-water mark of the pushes so far, and, when the epochs wrap
// (`wrap`: this push starts them again at 1), the words used so far.
static uint64_t* gw_tagged_words(SgHandle* h, SgHandle::GwTagged& tw, const char* name, size_t words, bool wrap,
                                 hipStream_t st) {
  uint64_t* p = (uint64_t*)h->ws.get(name, sizeof(uint64_t) * words, st);
  const size_t cap = h->ws.bufs[name].bytes;
  if (p != tw.p || cap != tw.cap) {
    tw.p = p;
    tw.cap = cap;
    tw.hw = 0;
  }
  if (wrap && tw.hw) HIPCHK(hipMemsetAsync(p, 0, sizeof(uint64_t) * tw.hw, st));
  if (words > tw.hw) {
    HIPCHK(hipMemsetAsync(p + tw.hw, 0, sizeof(uint64_t) * (words - tw.hw), st));
    tw.hw = words;
  }
  return p;
}

// the delivered matches of a group-walked push -> output records: per-tile match counts -> tile bases (scan) ->
// output records per tile (block scan inside the tile)
static void gw_project(SgHandle* h, const BatchView& bv, int64_t n, const GwArgs& ga, const GwSel& sel, uint32_t total) {
  const sg_nfa_desc& d = h->desc;
  hipStream_t st = h->stream;
  char* out = h->out.reserve(total, d.n_select, st);
  const int rpt = gw_proj_rpt();   // rows per projection thread: a tile is 256 times that
  const uint32_t lg_tile = gw_proj_lg_tile(rpt);
  const int64_t tile = (int64_t)1 << lg_tile;
  const int64_t ntile = (n + tile - 1) / tile;
  uint32_t* tcount = (uint32_t*)h->ws.get("gw_tcount", sizeof(uint32_t) * ((size_t)ntile + 1), st);
  uint32_t* tbase = (uint32_t*)h->ws.get("gw_tbase", sizeof(uint32_t) * ((size_t)ntile + 1), st);
  h->kbeg("gw_tiles");
  HIPCHK(hipMemsetAsync(tcount + ntile, 0, sizeof(uint32_t), st));
  launch_gtile_count(n, (const uint64_t*)ga.trig, ga.epoch, tcount, ntile, lg_tile, st);
  sg_exclusive_scan(h->ws, st, "gw_tscan_tmp", tcount, tbase, (uint32_t)0, (size_t)ntile + 1, rocprim::plus<uint32_t>());
  h->kend();
  uint32_t tsum = 0;
  HIPCHK(hipMemcpyAsync(&tsum, tbase + ntile, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  h->kbeg("gw_project");
  launch_gscan_project(rpt, n, ga.t0, bv.base_index, bv.index, (const uint64_t*)ga.trig, ga.epoch,
                       (const uint64_t*)ga.area, sel, ntile, (int64_t)h->out.n, out, (const uint32_t*)tbase, st);
  h->kend();
  HIPCHK(hipStreamSynchronize(st));
  if (tsum != total) throw SgError(SG_EINVAL, "internal: group walker match count mismatch");
  h->out.n += total;
}

// One push whose partition ran pass 1 in two (more than 65,536 keys) through the group walker.  Returns 1 when it
// delivered the push, 2 when the push needs wide records (the caller returns false), 0 when it declines.  A declined
// call has only read o1 / grec / glk / pk_flags and written workspaces of its own (gw_*, and cv_*, which the record
// pass acquires again): nothing was delivered, and neither h->out, the carry sets nor the push counters changed, so
// the caller goes on with pass 2 of the partition and the tiled walker.
template <class T>
static int run_group_walk(SgHandle* h, const BatchView& bv, int64_t n, int64_t nc, uint32_t kb, const PartPlan& pp,
                          const uint32_t* o1, const WRec<T, true>* grec, const uint8_t* glk, uint32_t* pk_flags,
                          const GwPlan& gp, const PushPlan& plan, const Virt& v, const SgCols& cc, int op, int stack_mode,
                          int val_col_a, EveryNextState* es) {
  const sg_nfa_desc& d = h->desc;
  hipStream_t st = h->stream;
  const int64_t nt = nc + n;
  const uint32_t ng = (kb + 255) >> 8;
  // per-key rows -> each key's first row in the group domain (its match-area region starts at 3x that)
  uint32_t* kbase = (uint32_t*)h->ws.get("gw_kbase", sizeof(uint32_t) * ((size_t)kb + 1), st);
  h->kbeg("gw_count");
  hipLaunchKernelGGL(k_gw_count, dim3(ng), dim3(256), 0, st, o1, pp.nc1, kb, glk, kbase);
  HIPCHK(hipGetLastError());
  h->kend();
  uint32_t pkf = 0;
  int64_t t0 = 0;   // narrow records' time origin: the push's first virtual row
  HIPCHK(hipMemcpyAsync(&pkf, pk_flags, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(&t0, nc ? v.c_ts : v.ts, sizeof(int64_t), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  const PackRange pr = pack_range(pkf);
  if (pr == PACK_TS_RANGE) return 2;
  if (pr == PACK_PAY_RANGE) return 0;   // a payload wider than 32 bits: the tiled path gathers e1 by row
  h->mark(2);

  GwArgs ga;
  memset(&ga, 0, sizeof(ga));
  ga.n = n;
  ga.nc = nc;
  ga.within = d.within;
  ga.t0 = t0;
  ga.K = kb;
  ga.nc1 = pp.nc1;
  ga.stack_mode = stack_mode;
  ga.cap = gp.cap;
  ga.chunk = 4096;
  ga.carry_out = h->opt.no_carry ? 0 : 1;
  ga.pzero = v.pfloat;
  ga.o1 = o1;
  ga.grec = (const PtU4*)grec;
  ga.glk = glk;
  ga.kbase = kbase;
  // this push's epoch, and the words it tags: nothing is cleared in steady state (gw_tagged_words)
  const char* ee = getenv("SG_DEBUG_GW_EPOCHS");   // (test hook: wrap after that many epochs)
  const uint32_t epochs = ee ? (uint32_t)std::min(std::max(atoi(ee), 1), 255) : 255u;
  const bool wrap = h->gw_epoch >= epochs;
  h->gw_epoch = wrap ? 1u : h->gw_epoch + 1;
  ga.epoch = h->gw_epoch;
  ga.trig = gw_tagged_words(h, h->gw_trig, "gw_trig", (size_t)std::max<int64_t>(n, 1), wrap, st);
  // (a key's rows bound its region with three units to spare -- its first row triggers nothing -- so the projection's
  // read of two entries behind every header stays inside the region; the pad keeps that true of the last key by
  // construction, not by that argument)
  ga.area = (uint64_t*)h->ws.get("gw_area", sizeof(uint64_t) * (3 * (size_t)std::max<int64_t>(nt, 1) + GW_AREA_PAD), st);
  uint32_t* gflags = (uint32_t*)h->ws.get("gw_flags", sizeof(uint32_t) * 4, st);
  ga.flags = gflags;
  ga.cv_n = gflags + 1;
  ga.ovf_n = gflags + 2;
  ga.ovf_cap = std::min<uint32_t>(kb, 1u << 16);
  ga.ovf_keys = (uint32_t*)h->ws.get("gw_ovf_keys", sizeof(uint32_t) * ga.ovf_cap, st);
  ga.match_n = gflags + 3;
  // carry: at most `cap` entries per key from the LDS rings, and a redone key's whole list -- room for 4M of those
  // (more sends the push to the tiled path)
  ga.cv_cap = (uint32_t)std::max<int64_t>(1, std::min<int64_t>(nt, (int64_t)kb * gp.cap + (1 << 22)));
  ga.cv_ts = (int64_t*)h->ws.get("cv_ts", sizeof(int64_t) * (size_t)ga.cv_cap, st);
  ga.cv_val = (int64_t*)h->ws.get("cv_val", sizeof(int64_t) * (size_t)ga.cv_cap, st);
  ga.cv_pay = (int64_t*)h->ws.get("cv_pay", sizeof(int64_t) * (size_t)ga.cv_cap, st);
  ga.cv_key = (int32_t*)h->ws.get("cv_key", sizeof(int32_t) * (size_t)ga.cv_cap, st);
  HIPCHK(hipMemsetAsync(gflags, 0, sizeof(uint32_t) * 4, st));
  h->kbeg("group_walk");
  dispatch_op(op, [&](auto opc) { launch_gwalk<T, decltype(opc)::value>(ga, ng, st); });
  h->kend();
  uint32_t hf[4] = {0, 0, 0, 0}, total = 0;
  HIPCHK(hipMemcpyAsync(hf, gflags, sizeof(hf), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (hf[0] & GW_INTERNAL) throw SgError(SG_EINVAL, "internal: group walker guard tripped");
  if (hf[0]) return 0;   // a key whose time goes back (or more ring overflows than the list holds): the tiled path
  if (hf[2]) {
    // keys whose pending list outgrew the LDS ring: each walked again with an unbounded HBM list
    h->kbeg("gw_redo");
    uint32_t* rrows = (uint32_t*)h->ws.get("gw_redo_rows", sizeof(uint32_t) * (size_t)nt, st);
    char* rl = (char*)h->ws.get("gw_redo_list", (sizeof(T) + 8) * (size_t)nt, st);
    T* hv = (T*)rl;
    int32_t* ht = (int32_t*)(rl + sizeof(T) * (size_t)nt);
    int32_t* hp = ht + nt;
    dispatch_op(op, [&](auto opc) { launch_gw_redo<T, decltype(opc)::value>(ga, hf[2], rrows, hv, ht, hp, st); });
    h->kend();
    HIPCHK(hipMemcpyAsync(hf, gflags, sizeof(hf), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (hf[0] & GW_INTERNAL) throw SgError(SG_EINVAL, "internal: group walker redo guard tripped");
    if (hf[0]) return 0;
  }
  // (last decline point: from here on the push is delivered)
  h->last_spilled = hf[2];
  total = hf[3];   // matches, counted by the walkers
  h->mark(3);
  h->split_out = 1;
  h->mark(5);
  if (total) {
    GwSel sel = gp.sel;
    recv_slot(d, d.shape_args[1], sel.multi, sel.b_slot);
    sel.pzero = v.pfloat;
    gw_project(h, bv, n, ga, sel, total);
  }
  h->mark(4);
  if (ga.carry_out) {
    WalkArgs wa;
    memset(&wa, 0, sizeof(wa));
    wa.alive = (uint32_t*)h->ws.get("alive_rows", sizeof(uint32_t), st);
    wa.alive_n = (uint32_t*)h->ws.get("gw_alive_n", sizeof(uint32_t), st);
    HIPCHK(hipMemsetAsync(wa.alive_n, 0, sizeof(uint32_t), st));
    wa.cv_n = ga.cv_n;
    wa.cv_ts = ga.cv_ts;
    wa.cv_key = ga.cv_key;
    wa.cv_val = ga.cv_val;
    wa.cv_pay = ga.cv_pay;
    carry_out_rows<T, true>(h, es, nt, v, bv, cc, wa, val_col_a, v.pcol ? plan.pcol : -1, v.pw);
  }
  h->last_events = n;
  h->last_matches = total;
  return 1;
}
