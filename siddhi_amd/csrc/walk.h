// walk.h -- the closed form's tiled walker (count, exact / HBM redo and record passes), the projection, the
// per-candidate search for unpartitioned streams (k_nge, run_nge) and the carry into the next push.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>

#include "keypart.h"
#include "sg_engine.h"
#include "sg_prim.h"
#include "walk_rec.h"

// Records per group load: G records = a whole number of 128-B lines, loaded by one lane at once so a
// line is fetched into registers exactly once (thousands of per-lane streams would otherwise thrash L2).
template <class T, bool N>
struct Grp {
  static constexpr int G = sizeof(WRec<T, N>) == 16 ? 8 : 16;
  static constexpr int QW = G * (int)sizeof(WRec<T, N>) / 16;
  typedef uint32_t U4 __attribute__((ext_vector_type(4)));
  U4 q[QW];
  __device__ __forceinline__ void load(const WRec<T, N>* base) {
    const U4* p = (const U4*)base;
#pragma unroll
    for (int j = 0; j < QW; ++j) q[j] = __builtin_nontemporal_load(p + j);
  }
  __device__ __forceinline__ WRec<T, N> rec(int i) const {
    WRec<T, N> r;
    __builtin_memcpy(&r, (const char*)q + i * sizeof(WRec<T, N>), sizeof(WRec<T, N>));
    return r;
  }
};

// ---------------------------------------------------------------------------------------------
struct ProjPlan {
  // per select column: src 0 = e1 row (pending partial), 1 = e2 row (trigger); kind 0 = e1 payload carried
  // in the pending list, 1 = the compared value, 2 = null (chain index beyond a single-event slot),
  // 3 = column gather by row
  int32_t src[SG_MAX_SELECT], kind[SG_MAX_SELECT], col[SG_MAX_SELECT], type[SG_MAX_SELECT];
};

// A delivered match as the record walk leaves it at its final slot: e1/e2 virtual rows, e1's compared value
// and e1's payload attribute (both taken from the pending list, so no gather reaches back into the window).
struct MRec {
  uint32_t r1, r2;
  int64_t v1;                 // e1 compared-value bits
  int64_t p1;                 // e1 payload bits
};

// Where the record walk leaves each delivered match (k_project builds the output record from it).  Narrow form
// (narrow walker records of a 4-byte value type, whose LDS ring already keeps 32-bit payloads): 16 B per match in
// one store; wide form: MRec.
struct MRec16 {
  uint32_t r1, r2, v1, p1;
};
struct MatchSink {
  void* rec;
  int32_t narrow;
  uint32_t cap;               // slots allocated (a slot beyond it trips the internal guard)
  uint32_t* err;
  __device__ __forceinline__ void put(uint32_t slot, uint32_t r1, uint32_t r2, int64_t v1, int64_t p1) const {
    if (slot >= cap) { atomicOr(err, 8u); return; }
    if (narrow) {
      PtU4 q;
      q.x = r1; q.y = r2; q.z = (uint32_t)v1; q.w = (uint32_t)p1;
      ((PtU4*)rec)[slot] = q;
    } else {
      MRec m;
      m.r1 = r1; m.r2 = r2; m.v1 = v1; m.p1 = p1;
      ((MRec*)rec)[slot] = m;
    }
  }
};

struct UnitDesc {
  uint32_t p0, p1, w, ovf;     // chunk positions [p0, p1), replay from w; ovf = 1 + first entry of its HBM list
};

struct WalkStats {
  uint32_t order_err;
  uint32_t n_ovf;             // units on the HBM-list walker
  uint32_t ovf_total;         // HBM-list entries they take (each unit: one entry per row it walks)
  uint32_t internal;          // internal consistency guards tripped (bit 1 unit range, 2 tile source, 4 count row,
                              // 8 match slot, 16 HBM-list space): reported as SG_EINVAL instead of touching memory
                              // out of range
};

// an HBM list for unit u walking rows [w, p1): its first entry (the lists of a push are packed back to back)
__device__ __forceinline__ uint32_t take_hbm_list(WalkStats* st, uint32_t w, uint32_t p1) {
  const uint32_t need = p1 - w + 1;
  const uint32_t o = atomicAdd(&st->ovf_total, need);
  atomicAdd(&st->n_ovf, 1u);
  if (o > 0xffffffffu - need) atomicOr(&st->internal, 16u);
  return o;
}

struct LdsPlan {   // per-push layout of the walkers' LDS rings (count walk: value + time only)
  int32_t pay;     // 1: narrow payload plane
  int32_t row;     // 1: e1 row plane
  int32_t cap;     // ring entries per lane (power of two; deeper for long `within` windows)
};

struct WalkArgs {
  int64_t nt;                 // virtual rows
  int64_t within;
  uint32_t K;                 // keys (1 if unpartitioned)
  uint32_t C;                 // time chunks
  uint32_t R;                 // virtual rows per chunk
  uint32_t n_units;
  int32_t partitioned;
  int32_t op;                 // 2 > 3 >= 4 < 5 <=
  int32_t stack_mode;         // 1: monotone stack, 0: scanned list
  int32_t carry_out;          // WRITE pass: record per-key carry suffixes
  uint64_t base_index;
  const uint64_t* index;
  int32_t multi, b_slot;
  int32_t n_select;
  int32_t stride;
  int64_t out_base;
  uint32_t big_total;         // entries of all HBM lists of the push (BIG)
  LdsPlan lp;                 // record walk LDS planes
  int32_t pay_in_rec;         // e1 payload rides in the (narrow) walker records
  // Keys whose rows (carried ones included) go back in time take the exact walker (see Walker::step_exact): one
  // unit per key on the HBM-list path.  kexact: per-key flag (null: no key does).
  const uint8_t* kexact;
  // Carry: the record pass of each key's last unit leaves the key's final pending list -- as virtual rows (alive,
  // alive_n: HBM lists, and LDS rings that keep e1's row) or as the entries' own time / value / payload (cv: LDS rings
  // without a row plane; the select needs no other e1 attribute then)
  uint32_t* alive;
  uint32_t* alive_n;
  int64_t* cv_ts;
  int32_t* cv_key;
  int64_t* cv_val;
  int64_t* cv_pay;
  uint32_t* cv_n;
  uint32_t cv_cap;
};

template <class T> __device__ __forceinline__ bool is_nan_val(T) { return false; }
template <> __device__ __forceinline__ bool is_nan_val<float>(float x) { return x != x; }
template <> __device__ __forceinline__ bool is_nan_val<double>(double x) { return x != x; }

template <class T>
__device__ __forceinline__ bool cmp_op(int op, T b, T a) {   // B.x OP A.x
  switch (op) {
    case 2: return b > a;
    case 3: return b >= a;
    case 4: return b < a;
    default: return b <= a;
  }
}

template <class T> __device__ __forceinline__ int64_t val_bits(T v);
template <> __device__ __forceinline__ int64_t val_bits<float>(float v) { return (int64_t)(uint32_t)__float_as_uint(v); }
template <> __device__ __forceinline__ int64_t val_bits<double>(double v) { return __double_as_longlong(v); }
template <> __device__ __forceinline__ int64_t val_bits<int32_t>(int32_t v) { return (int64_t)v; }
template <> __device__ __forceinline__ int64_t val_bits<int64_t>(int64_t v) { return v; }

// Pending list: value + timestamp per partial, plus (record walk only) e1's payload attribute and e1's row
// when a select gathers other e1 attributes.  LDS: ring of `cap` (power of two) entries per lane, SoA planes,
// lane-strided (conflict-free); timestamps relative to the unit's first replayed row; payload narrowed to
// 32 bits (a LONG that does not fit sends the unit to the HBM path).  The count walk keeps 8 B per entry, so
// it runs at twice the residency of the record walk.  HBM (BIG): one unbounded list per overflowed unit,
// indexed by push count (no wrap), 64-bit times and payloads.
template <class T, bool BIG>
struct PendList {
  T* val;
  int32_t* dts;
  int64_t* ts;
  uint32_t* row;              // null: not kept
  int32_t* pay32;             // LDS narrow payload (null: none)
  int64_t* pay64;             // HBM payload
  int32_t pzero;              // narrow payload is zero-extended (FLOAT bits) rather than sign-extended
  int64_t base;
  uint32_t cmask;             // LDS ring: capacity - 1
  __device__ __forceinline__ uint32_t ix(uint32_t s) const { return BIG ? s : (s & cmask) * WALK_BLOCK; }
  __device__ __forceinline__ T gv(uint32_t s) const { return val[ix(s)]; }
  __device__ __forceinline__ int64_t gts(uint32_t s) const { return BIG ? ts[ix(s)] : base + (int64_t)dts[ix(s)]; }
  __device__ __forceinline__ uint32_t grow(uint32_t s) const { return row ? row[ix(s)] : 0u; }
  __device__ __forceinline__ int64_t gpay(uint32_t s) const {
    if (BIG) return pay64 ? pay64[ix(s)] : 0;
    if (!pay32) return 0;
    int32_t x = pay32[ix(s)];
    return pzero ? (int64_t)(uint32_t)x : (int64_t)x;
  }
  __device__ __forceinline__ void put(uint32_t s, T v, int64_t t, uint32_t r, int64_t p) {
    uint32_t i = ix(s);
    val[i] = v;
    if (BIG) ts[i] = t; else dts[i] = (int32_t)(t - base);
    if (row) row[i] = r;
    if (BIG) { if (pay64) pay64[i] = p; } else if (pay32) pay32[i] = (int32_t)p;
  }
};
template <class T>
struct PendBytes {   // bytes per entry
  static int lds(bool write, const LdsPlan& lp) { return (int)sizeof(T) + 4 + (write ? 4 * (lp.pay + lp.row) : 0); }
  static constexpr int hbm = sizeof(T) + 20;   // val, ts, row, payload
};
// LDS planes of one block: [val][dts][pay32?][row?], each cap * WALK_BLOCK entries
template <class T, bool BIG>
__device__ __forceinline__ void lds_planes(PendList<T, BIG>& L, char* lds, bool write, const LdsPlan& lp) {
  const size_t E = (size_t)(lp.cap) * WALK_BLOCK;
  L.cmask = (uint32_t)lp.cap - 1;
  char* p = lds;
  L.val = (T*)p + threadIdx.x; p += E * sizeof(T);
  L.dts = (int32_t*)p + threadIdx.x; p += E * 4;
  L.pay32 = nullptr;
  L.row = nullptr;
  if (write && lp.pay) { L.pay32 = (int32_t*)p + threadIdx.x; p += E * 4; }
  if (write && lp.row) { L.row = (uint32_t*)p + threadIdx.x; p += E * 4; }
  L.ts = nullptr;
  L.pay64 = nullptr;
}
template <class T, bool BIG>
__device__ __forceinline__ void hbm_planes(PendList<T, BIG>& L, char* big, uint32_t first, size_t total) {
  L.ts = (int64_t*)big + first;
  L.pay64 = (int64_t*)(big + total * 8) + first;
  L.val = (T*)(big + total * 16) + first;
  L.row = (uint32_t*)(big + total * (16 + sizeof(T))) + first;
  L.dts = nullptr;
  L.pay32 = nullptr;
}

template <class T, bool N>
__device__ __forceinline__ uint32_t lb_row(const Src<T, N>& src, uint32_t lo, uint32_t hi, uint32_t target, bool part) {
  if (!part) return target < lo ? lo : (target > hi ? hi : target);
  while (lo < hi) {
    uint32_t mid = lo + ((hi - lo) >> 1);
    if (src.row(mid) < target) lo = mid + 1; else hi = mid;
  }
  return lo;
}
template <class T, bool N>
__device__ __forceinline__ uint32_t lb_ts(const Src<T, N>& src, uint32_t lo, uint32_t hi, int64_t tmin) {
  while (lo < hi) {
    uint32_t mid = lo + ((hi - lo) >> 1);
    if (src.ts(mid) < tmin) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ uint32_t xcd_block(uint32_t b, uint32_t nb) {
  // blocks are dealt round-robin over the 8 XCDs: give XCD x a contiguous range of logical blocks
  uint32_t x = b & 7, i = b >> 3, per = nb >> 3, rem = nb & 7;
  return x < rem ? x * (per + 1) + i : rem * (per + 1) + (x - rem) * per + i;
}

// Match projection (QuerySelector.processNoGroupBy, C/query/selector/QuerySelector.java:125-163, with
// SelectiveStateEventPopulator, C/event/state/populater/SelectiveStateEventPopulator.java:36-56): one
// thread per delivered match builds its AoS record from the (e1 row, e2 row) pair the walker placed at the
// match's final slot.  Slots are in delivery order, so the e2 gathers stream and the e1 gathers stay within
// one `within` window behind them.
template <class T>
__global__ void __launch_bounds__(256) k_project(WalkArgs a, Virt v, ProjPlan pp, SgCols bc, SgCols cc,
                                                 const MatchSink ms, const uint32_t* __restrict__ off,
                                                 int64_t total, char* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) char stage[];   // 256 records, written out contiguously
  const int64_t per = (int64_t)blockDim.x;
  // one match per thread (every gather in flight at once); each XCD takes a contiguous slot range so the
  // trigger-ordered gathers of neighbouring slots share its L2 instead of being fetched by all eight
  const int64_t s0 = (int64_t)xcd_block(blockIdx.x, gridDim.x) * per;
  const int64_t sl = s0 + threadIdx.x;
  if (sl < total) {
    MRec mr;
    if (ms.narrow) {   // 32-bit value / payload bits widened as val_bits and the LDS ring (pzero) widen them
      const PtU4 q = ((const PtU4*)ms.rec)[sl];
      mr.r1 = q.x;
      mr.r2 = q.y;
      mr.v1 = std::is_same<T, float>::value ? (int64_t)q.z : (int64_t)(int32_t)q.z;
      mr.p1 = v.pfloat ? (int64_t)q.w : (int64_t)(int32_t)q.w;
    } else {
      mr = ((const MRec*)ms.rec)[sl];
    }
    const uint32_t r1 = mr.r1, r2 = mr.r2;
    const uint64_t b = r2 - v.nc;
    const uint32_t ob = off[b];
    const uint32_t key = a.partitioned ? (uint32_t)v.key[b] : 0u;
    const int64_t t2 = v.ts[b];
    const uint64_t trig = a.index ? a.index[b] : a.base_index + b;
    int64_t* o = (int64_t*)(stage + (size_t)threadIdx.x * a.stride);
    uint32_t nm = 0;
    for (int s = 0; s < a.n_select; ++s) {
      const bool s2 = pp.src[s] != 0;
      const int kind = pp.kind[s];
      int64_t bits = 0;
      if (kind == 0) {
        bits = mr.p1;
      } else if (kind == 1) {
        bits = s2 ? val_bits<T>(v_val<T>(v, r2, v.val_a == v.val_b)) : mr.v1;
      } else if (kind == 2) {
        nm |= 1u << s;
      } else {
        const uint32_t r = s2 ? r2 : r1;
        SgVal x = r < v.nc ? sg_read_col(cc, pp.col[s], pp.type[s], r) : sg_read_col(bc, pp.col[s], pp.type[s], r - v.nc);
        if (x.null) nm |= 1u << s;
        bits = sg_val_bits(x);
      }
      o[4 + s] = bits;
    }
    const uint32_t rank = (uint32_t)(sl - (int64_t)ob);
    o[0] = (int64_t)trig;
    o[1] = t2;
    o[2] = (int64_t)((uint64_t)key | ((uint64_t)((1u << 24) | (a.multi ? (uint32_t)a.b_slot : (0x800000u | rank))) << 32));
    o[3] = (int64_t)nm;
  }
  __syncthreads();
  const int64_t nrec = (total - s0 < per) ? (total - s0) : per;
  const size_t bytes = (size_t)nrec * a.stride;
  char* dst = out + (size_t)(a.out_base + s0) * a.stride;
  if ((((uintptr_t)dst) & 15) == 0) {
    typedef uint32_t U4 __attribute__((ext_vector_type(4)));
    for (size_t q = (size_t)threadIdx.x * 16; q < bytes; q += (size_t)per * 16)
      *(U4*)(dst + q) = *(const U4*)(stage + q);
  } else {
    for (size_t q = (size_t)threadIdx.x * 8; q < bytes; q += (size_t)per * 8)
      *(uint64_t*)(dst + q) = *(const uint64_t*)(stage + q);
  }
}

// The reference's pending list for one event of one key (see the file header).
template <int OP, class T>
__device__ __forceinline__ bool cmp_sel(int op, T b, T a) { return cmp_op<T>(OP ? OP : op, b, a); }

template <class T, bool WRITE, bool BIG, int OP = 0>
struct Walker {
  // LDS path: times relative to the unit's first replayed row (the unit's span was checked to fit 31 bits);
  // HBM-list path: absolute 64-bit times.
  typedef typename std::conditional<BIG, int64_t, int32_t>::type TT;
  PendList<T, BIG> L;
  uint32_t head = 0, top = 0;
  TT hts = 0;                 // register copies (valid while head != top): time of the oldest partial and
  T tv = T();                 // value of the newest one -- the common step touches no LDS for either
  int64_t prev_t;             // time of the previous row (the records' own time domain): the order check
  int32_t prev32;             // (narrow records: their 32-bit times, compared as such)
  TT within;
  bool bad = false;
  // exact mode (a key whose time goes back; HBM list only): min / max time over the list while head != top
  bool exact = false;
  int64_t lo_t = 0, hi_t = 0;
  bool oob = false;           // internal guard: a row outside the batch (never expected)
  bool overflow = false;
  uint32_t ew = 0xffffffffu, ebits = 0;   // count pass: emit bitmap word being built
  __device__ __forceinline__ void set_within(int64_t w) {
    within = BIG ? (TT)w : (TT)(w > 0x7fffffffll ? 0x7fffffffll : w);   // a wider window never expires in-unit
  }
  __device__ __forceinline__ TT rel(int64_t t) const { return BIG ? (TT)t : (TT)(t - L.base); }
  // order check against the row before the replay window
  __device__ __forceinline__ void init_prev(int64_t before) {
    prev_t = before;
    prev32 = (int32_t)(before < INT32_MIN ? INT32_MIN : (before > INT32_MAX ? INT32_MAX : before));
  }
  __device__ __forceinline__ TT at(uint32_t s) const {
    return BIG ? (TT)L.ts[L.ix(s)] : (TT)L.dts[L.ix(s)];
  }
  __device__ __forceinline__ void flush_bits(uint32_t* __restrict__ emap) {
    if (ebits) atomicOr(&emap[ew], ebits);
    ebits = 0;
  }
  __device__ __forceinline__ void mark_emit(uint32_t pos, uint32_t* __restrict__ emap) {
    const uint32_t wi = pos >> 5;
    if (wi != ew) { flush_bits(emap); ew = wi; }
    ebits |= 1u << (pos & 31);
  }
  __device__ __forceinline__ void push(T x, int64_t tabs, uint32_t r, int64_t pay) {
    L.put(top, x, tabs, r, pay);
    if (top == head) hts = rel(tabs);
    tv = x;
    ++top;
  }
  // returns true when this event (inside the unit's chunk) completed partials
  template <class R>
  __device__ __forceinline__ bool step(const WalkArgs& a, const Virt& v, const R& rc, bool in_chunk,
                                       uint32_t ofs, uint32_t* __restrict__ cnt, const MatchSink& em,
                                       bool payload, int64_t pay = 0, bool pay_ready = false) {
    const uint32_t f = rc.rowf >> 30;
    // every row of the key takes part in the order check (a row that fails both filters still expires partials in
    // the reference): a key whose time goes back is redone by the exact walker
    const int64_t tabs = rc.t();
    if constexpr (R::narrow) {   // (a narrow record's time is a 32-bit offset: one 32-bit compare)
      bad |= rc.dts < prev32;
      prev32 = rc.dts;
    } else {
      bad |= tabs < prev_t;
      prev_t = tabs;
    }
    if (!f) return false;
    const T x = rc.val;
    const TT t = rel(tabs);
    // lazy `within` expiry of the oldest partials (StreamPreStateProcessor.isExpired :102-113)
    if (head != top && t - hts > within) {
      ++head;
      while (head != top) {
        hts = at(head);
        if (t - hts <= within) break;
        ++head;
      }
    }
    const uint32_t r = rc.rowf & ROW_MASK;
    const bool live = !is_nan_val<T>(x);
    uint32_t m = 0;
    if ((f & F_CONS) && live) {
      if (a.stack_mode) {
        // monotone stack: the completed partials are exactly a suffix, delivered oldest first
        if (top != head && cmp_sel<OP, T>(a.op, x, tv)) {
          --top;
          ++m;
          while (top != head) {
            tv = L.gv(top - 1);
            if (!cmp_sel<OP, T>(a.op, x, tv)) break;
            --top;
            ++m;
          }
        }
        if (WRITE && in_chunk && r >= v.nc) {
          for (uint32_t q = 0; q < m; ++q)
            em.put(ofs + q, L.grow(top + q), r, val_bits<T>(L.gv(top + q)), L.gpay(top + q));
        }
      } else {
        const bool emit = in_chunk && (r >= v.nc);
        uint32_t wr = head;
        for (uint32_t s = head; s != top; ++s) {
          T e = L.gv(s);
          if (cmp_sel<OP, T>(a.op, x, e)) {
            if (WRITE && emit) em.put(ofs + m, L.grow(s), r, val_bits<T>(e), L.gpay(s));
            ++m;
          } else {
            if (wr != s) L.put(wr, e, BIG ? (int64_t)at(s) : L.base + (int64_t)at(s), L.grow(s), L.gpay(s));
            ++wr;
          }
        }
        top = wr;
        if (head != top) {   // (compaction moved entries: refresh the register copies)
          hts = at(head);
          tv = L.gv(top - 1);
        }
      }
    }
    const bool emitted = m && in_chunk && (r >= v.nc);
    if (!WRITE && emitted) {
      if (r - v.nc < (uint64_t)v.n) cnt[r - v.nc] = m;
      else oob = true;
    }
    if ((f & F_CAND) && live) {
      if (!BIG && top - head == L.cmask + 1) { overflow = true; return emitted; }
      int64_t pv = 0;
      if (WRITE && payload) {
        if (R::has_pay && a.pay_in_rec) pv = rc.p(v.pfloat);
        else pv = pay_ready ? pay : v_payload(v, r);
      }
      // the LDS ring keeps 32 payload bits: a wider LONG value sends the unit to the HBM path
      if (!BIG && WRITE && payload && L.pay32 && !L.pzero && pv != (int64_t)(int32_t)pv) { overflow = true; return emitted; }
      push(x, rc.t(), r, pv);
    }
    return emitted;
  }
  __device__ __forceinline__ void keep(uint32_t& wr, uint32_t s, T e, int64_t ti) {
    if (wr != s) L.put(wr, e, ti, L.grow(s), L.gpay(s));
    ++wr;
    if (wr == head + 1) { lo_t = ti; hi_t = ti; } else { lo_t = ti < lo_t ? ti : lo_t; hi_t = ti > hi_t ? ti : hi_t; }
  }
  // The reference's list for any arrival order (HBM list only): a row of B's stream first drops every pending
  // partial with |e1.ts - ts| > within -- on either side, not only the oldest (StreamPreStateProcessor.isExpired,
  // C/query/input/stream/state/StreamPreStateProcessor.java:102-113) -- then a B consumer completes, in pending
  // order, every partial its compare accepts (processAndReturn :292-337), then a candidate appends itself.
  template <class R>
  __device__ __forceinline__ bool step_exact(const WalkArgs& a, const Virt& v, const R& rc, bool in_chunk,
                                             uint32_t ofs, uint32_t* __restrict__ cnt, const MatchSink& em,
                                             bool payload) {
    const uint32_t f = rc.rowf >> 30;
    const uint32_t r = rc.rowf & ROW_MASK;
    const int64_t t = rc.t();
    const T x = rc.val;
    const bool live = !is_nan_val<T>(x);
    if (BIG && head != top && (t - lo_t > (int64_t)within || hi_t - t > (int64_t)within) && v_visit(v, r)) {
      uint32_t wr = head;
      for (uint32_t s = head; s != top; ++s) {
        const int64_t ti = (int64_t)at(s);
        if (t - ti > (int64_t)within || ti - t > (int64_t)within) continue;
        keep(wr, s, L.gv(s), ti);
      }
      top = wr;
    }
    uint32_t m = 0;
    if ((f & F_CONS) && live && head != top) {
      const bool emit = in_chunk && (r >= v.nc);
      uint32_t wr = head;
      for (uint32_t s = head; s != top; ++s) {
        const T e = L.gv(s);
        if (cmp_sel<OP, T>(a.op, x, e)) {
          if (WRITE && emit) em.put(ofs + m, L.grow(s), r, val_bits<T>(e), L.gpay(s));
          ++m;
        } else {
          keep(wr, s, e, (int64_t)at(s));
        }
      }
      top = wr;
    }
    const bool emitted = m && in_chunk && (r >= v.nc);
    if (!WRITE && emitted) {
      if (r - v.nc < (uint64_t)v.n) cnt[r - v.nc] = m;
      else oob = true;
    }
    if ((f & F_CAND) && live) {
      int64_t pv = 0;
      if (WRITE && payload) pv = (R::has_pay && a.pay_in_rec) ? rc.p(v.pfloat) : v_payload(v, r);
      if (head == top) { lo_t = t; hi_t = t; } else { lo_t = t < lo_t ? t : lo_t; hi_t = t > hi_t ? t : hi_t; }
      L.put(top, x, t, r, pv);
      ++top;
    }
    return emitted;
  }
};

// HBM-list walker: one lane per unit whose pending list outgrew the LDS ring, whose time span does not fit the ring's
// 31-bit times, or whose key's time goes back (exact mode: the key's whole segment in one unit).  WRITE=false: count
// pass; WRITE=true: record pass.
template <class T, bool N, bool WRITE, bool BIG>
__global__ void __launch_bounds__(WALK_BLOCK) k_walk(WalkArgs a, Src<T, N> src, const uint32_t* __restrict__ seg_b,
                                                     const uint32_t* __restrict__ seg_e, UnitDesc* __restrict__ ud,
                                                     uint32_t* __restrict__ cnt, const uint32_t* __restrict__ off,
                                                     const MatchSink em, uint32_t* __restrict__ emap,
                                                     WalkStats* __restrict__ st, char* __restrict__ big) {
  static_assert(BIG, "the LDS-ring units run on the tiled walker (k_walk_t)");
  const uint32_t u = xcd_block(blockIdx.x, gridDim.x) * WALK_BLOCK + threadIdx.x;
  if (u >= a.n_units) return;
  const Virt& v = src.pk.v;
  const bool part = a.partitioned != 0;
  const uint32_t k = u % a.K;
  uint32_t sb, se;
  if (part) {
    sb = seg_b[k];
    se = seg_e[k];
  } else {
    sb = 0;
    se = (uint32_t)a.nt;
  }
  const UnitDesc d = ud[u];
  const uint32_t p0 = d.p0, p1 = d.p1, w = d.w, ovf = d.ovf;
  if (p0 >= p1 || ovf == 0) return;
  Walker<T, WRITE, BIG> W;
  hbm_planes<T, BIG>(W.L, big, ovf - 1, a.big_total);
  W.L.pzero = v.pfloat;
  W.exact = a.kexact && a.kexact[k];
  const bool payload = v.pcol != nullptr;
  const int64_t tw = src.ts(w);
  W.L.base = tw;
  W.set_within(a.within);
  W.init_prev((w > sb) ? src.ts(w - 1) : tw);
  // record walk: output offsets only for the positions the count pass marked as emitting
  auto off_of = [&](const WRec<T, N>& rc, uint32_t pos, uint32_t bits) -> uint32_t {
    uint32_t r = rc.rowf & ROW_MASK;
    return (bits && pos >= p0 && pos < p1 && r >= v.nc) ? off[r - v.nc] : 0u;
  };
  auto one = [&](const WRec<T, N>& rc, uint32_t p, uint32_t o) {
    const bool e = W.exact ? W.step_exact(a, v, rc, p >= p0, o, cnt, em, payload)
                           : W.step(a, v, rc, p >= p0, o, cnt, em, payload);
    if (e && !WRITE) W.mark_emit(p, emap);
  };
  if (src.srec) {
    // key-sorted records: whole-line group loads, next group in flight while this one is walked
    typedef Grp<T, N> GT;
    const uint32_t G = GT::G;
    GT cur, nxt;
    uint32_t g = w & ~(G - 1);
    cur.load(src.srec + g);
    uint32_t ofs[GT::G], nofs[GT::G];
    uint32_t eb = 0, neb = 0;
    if (WRITE) {
      eb = emap[g >> 5] >> (g & 31);
#pragma unroll
      for (int i = 0; i < GT::G; ++i) ofs[i] = off_of(cur.rec(i), g + i, (eb >> i) & 1u);
    }
    for (; g < p1; g += G) {
      const uint32_t gn = g + G;
      if (gn < p1) {
        nxt.load(src.srec + gn);
        if (WRITE) neb = emap[gn >> 5] >> (gn & 31);
      }
#pragma unroll
      for (int i = 0; i < GT::G; ++i) {
        const uint32_t p = g + i;
        if (p < w || p >= p1) continue;
        one(cur.rec(i), p, WRITE ? ofs[i] : 0u);
      }
      cur = nxt;
      if (WRITE) {
#pragma unroll
        for (int i = 0; i < GT::G; ++i) nofs[i] = (gn < p1) ? off_of(cur.rec(i), gn + i, (neb >> i) & 1u) : 0u;
#pragma unroll
        for (int i = 0; i < GT::G; ++i) ofs[i] = nofs[i];
      }
    }
  } else {
    // unpartitioned: the rows themselves, in order
    for (uint32_t p = w; p < p1; ++p) {
      WRec<T, N> rc = src.pk(p);
      one(rc, p, WRITE ? off_of(rc, p, (emap[p >> 5] >> (p & 31)) & 1u) : 0u);
    }
  }
  if (!WRITE) W.flush_bits(emap);
  if (W.oob) atomicOr(&st->internal, 4u);
  if (W.bad && !W.exact) atomicOr(&st->order_err, 1u);
  if (WRITE && a.carry_out && p1 == se) {
    // the key's pending list survives: its partials as rows, in pending order (replaying them as candidates rebuilds
    // the list -- a carried row neither expires nor completes anything)
    const uint32_t m = W.top - W.head;
    const uint32_t o = m ? atomicAdd(a.alive_n, m) : 0u;
    if ((uint64_t)o + m > (uint64_t)a.nt) atomicOr(&st->internal, 32u);
    else for (uint32_t s = 0; s < m; ++s) a.alive[o + s] = W.L.grow(W.head + s);
  }
}

// ---------------------------------------------------------------------------------------------
// Lane-interleaved ("transposed") walker tiles for partitioned queries.  Logical wave W owns units
// 64W..64W+63; row i of its tile holds record (w_u + i) of each of its units, so one wave-wide record load
// is one contiguous 1 KB access and the emit flags of a row are one ballot word.

// unit replay ranges (p0, p1, w) + per-wave tile length (rows, padded to TROWS)
static const int TROWS = 16;
template <class T, bool N>
__global__ void __launch_bounds__(256) k_units(WalkArgs a, Src<T, N> src, const uint32_t* __restrict__ seg_b,
                                               const uint32_t* __restrict__ seg_e, UnitDesc* __restrict__ ud,
                                               uint32_t* __restrict__ wlen, WalkStats* __restrict__ st) {
  const uint32_t u = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t len = 0;
  if (u < a.n_units) {
    const uint32_t c = u / a.K, k = u % a.K;
    uint32_t sb = seg_b[k], se = seg_e[k];
    UnitDesc d{0, 0, 0, 0};
    if (se > a.nt || sb > se) { atomicOr(&st->internal, 1u); sb = se = 0; }
    if (sb < se && a.kexact && a.kexact[k]) {
      // a key whose time goes back: its whole segment in one exact unit (chunk 0) on the HBM-list walker
      if (c == 0) d = UnitDesc{sb, se, sb, take_hbm_list(st, sb, se) + 1};
    } else if (sb < se) {
      uint64_t lo_row = (uint64_t)c * a.R, hi_row = lo_row + a.R;
      uint32_t p0 = c == 0 ? sb : lb_row(src, sb, se, (uint32_t)(lo_row < (uint64_t)a.nt ? lo_row : a.nt), true);
      uint32_t p1 = c + 1 >= a.C ? se : lb_row(src, p0, se, (uint32_t)(hi_row < (uint64_t)a.nt ? hi_row : a.nt), true);
      d = UnitDesc{p0, p0, p0, 0};
      if (p0 < p1) {
        uint32_t w = lb_ts(src, sb, p0, src.ts(p0) - a.within);
        d = UnitDesc{p0, p1, w, 0};
        int64_t tw = src.ts(w), tl = src.ts(p1 - 1);
        if (tl - tw > 0x7fffffffll || tl < tw) {   // relative ts would not fit: HBM-list walker
          d.ovf = take_hbm_list(st, w, p1) + 1;
        } else {
          len = p1 - w;
        }
      }
    }
    ud[u] = d;
  }
  // wave max -> tile rows
  uint32_t m = len;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o));
  if ((threadIdx.x & 63) == 0 && (u >> 6) < (a.n_units + 63) / 64) wlen[u >> 6] = (m + TROWS - 1) / TROWS * TROWS;
}

// row-block -> wave map
static __global__ void k_rowmap(const uint32_t* __restrict__ wlen, const uint32_t* __restrict__ wrow, uint32_t nw,
                         uint32_t* __restrict__ map) {
  uint32_t W = blockIdx.x * blockDim.x + threadIdx.x;
  if (W >= nw) return;
  for (uint32_t q = wrow[W] / TROWS, e = (wrow[W] + wlen[W]) / TROWS; q < e; ++q) map[q] = W;
}

// sorted records -> tiles, through an LDS transpose (coalesced reads per unit, 1 KB rows out)
template <class T, bool N>
__global__ void __launch_bounds__(256) k_transpose(const WRec<T, N>* __restrict__ srec, const UnitDesc* __restrict__ ud,
                                                   const uint32_t* __restrict__ wrow, const uint32_t* __restrict__ map,
                                                   uint32_t nq, WRec<T, N>* __restrict__ tile, uint32_t nsrc,
                                                   uint32_t n_units, WalkStats* __restrict__ st) {
  __shared__ WRec<T, N> t[TROWS][64];
  for (uint32_t q = blockIdx.x; q < nq; q += gridDim.x) {
    const uint32_t W = map[q];
    const uint32_t i0 = q * TROWS - wrow[W];
    for (uint32_t idx = threadIdx.x; idx < TROWS * 64; idx += blockDim.x) {
      const uint32_t l = idx / TROWS, ii = idx % TROWS;
      const uint32_t u = W * 64 + l;   // (the last wave's lanes past n_units have no descriptor)
      const UnitDesc d = u < n_units ? ud[u] : UnitDesc{0, 0, 0, 0};
      WRec<T, N> r;
      const uint32_t len = (d.p1 > d.p0 && !d.ovf) ? d.p1 - d.w : 0;
      const uint32_t p = d.w + i0 + ii;
      if (i0 + ii < len && p < nsrc) {
        r = srec[p];
      } else {
        if (i0 + ii < len) atomicOr(&st->internal, 2u);
        memset(&r, 0, sizeof(r));
      }
      t[ii][l ^ ii] = r;
    }
    __syncthreads();
    for (uint32_t idx = threadIdx.x; idx < TROWS * 64; idx += blockDim.x) {
      const uint32_t ii = idx / 64, l = idx % 64;
      tile[(size_t)(q * TROWS + ii) * 64 + l] = t[ii][l ^ ii];
    }
    __syncthreads();
  }
}

// walker over tiles (partitioned, LDS list).  All 64 lanes step through rows together.
// (launch bounds: the record walk's LDS ring (12 B per entry, 16 entries per lane) fits three blocks per CU -- three
// waves per SIMD -- which its registers must allow too: at 2 waves per SIMD C2's record walk took 3.2 ms, at 3 1.6 ms)
template <class T, bool N, int OP, bool WRITE>
__global__ void __launch_bounds__(WALK_BLOCK, WRITE ? 3 : 5) k_walk_t(WalkArgs a, Src<T, N> src, const uint32_t* __restrict__ seg_b,
                                                       const uint32_t* __restrict__ seg_e,
                                                       const UnitDesc* __restrict__ ud,
                                                       const uint32_t* __restrict__ wlen,
                                                       const uint32_t* __restrict__ wrow,
                                                       const WRec<T, N>* __restrict__ tile, uint32_t* __restrict__ cnt,
                                                       const uint32_t* __restrict__ off, const MatchSink em,
                                                       uint64_t* __restrict__ emask, WalkStats* __restrict__ st,
                                                       UnitDesc* __restrict__ ud_w) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const uint32_t u = xcd_block(blockIdx.x, gridDim.x) * WALK_BLOCK + threadIdx.x;
  const uint32_t W = __builtin_amdgcn_readfirstlane(u >> 6), lane = threadIdx.x & 63;
  if ((W << 6) >= a.n_units) return;   // whole wave out of range (n_units need not be a multiple of 64)
  const Virt& v = src.pk.v;
  const UnitDesc d = u < a.n_units ? ud[u] : UnitDesc{0, 0, 0, 0};
  bool active = d.p0 < d.p1 && !d.ovf;
  const uint32_t p0 = d.p0, p1 = d.p1, w = d.w;
  const uint32_t len = active ? p1 - w : 0;
  const uint32_t rows = __builtin_amdgcn_readfirstlane(wlen[W]), base = __builtin_amdgcn_readfirstlane(wrow[W]);
  Walker<T, WRITE, false, OP> Wk;
  lds_planes<T, false>(Wk.L, lds, WRITE, a.lp);
  Wk.L.pzero = v.pfloat;
  const uint32_t k = u % a.K;
  const uint32_t sb = active ? seg_b[k] : 0;
  const int64_t tw = active ? src.ts(w) : 0;
  Wk.L.base = tw;
  Wk.set_within(a.within);
  Wk.init_prev((active && w > sb) ? src.ts(w - 1) : tw);
  const bool payload = v.pcol != nullptr;
  const uint32_t chunk_i = active ? p0 - w : 0;   // rows before this index only rebuild the pending list
  const WRec<T, N>* tp = tile + (size_t)base * 64 + lane;
  WRec<T, N> ba[PF], bb[PF];
  uint32_t oa[PF], ob[PF];
  auto load_rows = [&](WRec<T, N>* buf, uint32_t i0) {
#pragma unroll
    for (int j = 0; j < PF; ++j) buf[j] = (i0 + j < rows) ? tp[(size_t)(i0 + j) * 64] : WRec<T, N>{};
  };
  auto gather_offs = [&](const WRec<T, N>* buf, uint32_t i0, uint32_t* ofs) {   // rows the count pass marked
#pragma unroll
    for (int j = 0; j < PF; ++j) {
      const uint64_t mj = (i0 + j < rows) ? emask[base + i0 + j] : 0ull;
      const uint32_t r = buf[j].rowf & ROW_MASK;
      ofs[j] = ((mj >> lane) & 1ull) ? off[r - v.nc] : 0u;
    }
  };
  auto process = [&](const WRec<T, N>* buf, uint32_t i0, const uint32_t* ofs) {
#pragma unroll
    for (int j = 0; j < PF; ++j) {
      bool e = false;
      if (active && i0 + j < len && !Wk.overflow)
        e = Wk.step(a, v, buf[j], i0 + j >= chunk_i, WRITE ? ofs[j] : 0u, cnt, em, payload);
      if (!WRITE) {
        const uint64_t b = __ballot(e);
        if (lane == 0) emask[base + i0 + j] = b;
      }
    }
  };
  // Explicit drain at each batch boundary: the batch about to be walked (loaded one batch earlier) and the
  // stores of the last batch are complete, so the branchy walk of a batch never waits on memory -- without it
  // the compiler drains every outstanding access (including the prefetch) inside each step.
  load_rows(ba, 0);
  if (WRITE) gather_offs(ba, 0, oa);
  for (uint32_t i = 0; i < rows; i += 2 * PF) {   // rows is a multiple of TROWS = 2 * PF
    __builtin_amdgcn_s_waitcnt(0);
    load_rows(bb, i + PF);
    if (WRITE) gather_offs(bb, i + PF, ob);
    process(ba, i, oa);
    __builtin_amdgcn_s_waitcnt(0);
    load_rows(ba, i + 2 * PF);
    if (WRITE) gather_offs(ba, i + 2 * PF, oa);
    process(bb, i + PF, ob);
  }
  if (Wk.oob) atomicOr(&st->internal, 4u);
  if (active && Wk.overflow && !WRITE) ud_w[u].ovf = take_hbm_list(st, w, p1) + 1;
  if (active && !Wk.overflow && Wk.bad) atomicOr(&st->order_err, 1u);
  if (!WRITE || !a.carry_out) return;
  // the key's last unit: its final pending list is the carry -- slots reserved once per wave (every lane of the wave
  // is still here), not by one atomic per key on a single counter
  const uint32_t m = (active && !Wk.overflow && p1 == seg_e[k]) ? Wk.top - Wk.head : 0u;
  uint32_t incl = m;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t y = (uint32_t)__shfl_up((int)incl, o);
    if ((int)lane >= o) incl += y;
  }
  const uint32_t tot = (uint32_t)__shfl((int)incl, 63);
  if (!tot) return;
  const bool by_row = Wk.L.row != nullptr;
  uint32_t cbase = 0;
  if (lane == 63) cbase = atomicAdd(by_row ? a.alive_n : a.cv_n, tot);
  cbase = (uint32_t)__shfl((int)cbase, 63);
  const uint32_t o = cbase + incl - m;
  if ((uint64_t)cbase + tot > (by_row ? (uint64_t)a.nt : (uint64_t)a.cv_cap)) {
    if (lane == 63) atomicOr(&st->internal, 32u);
    return;
  }
  if (by_row) {
    for (uint32_t s = 0; s < m; ++s) a.alive[o + s] = Wk.L.grow(Wk.head + s);
  } else {
    const int64_t t0 = N ? v_ts(v, 0) : 0;   // (narrow records keep times relative to the push's first row)
    for (uint32_t s = 0; s < m; ++s) {
      const uint32_t q = Wk.head + s;
      a.cv_ts[o + s] = t0 + Wk.L.gts(q);
      a.cv_key[o + s] = (int32_t)k;
      a.cv_val[o + s] = val_bits<T>(Wk.L.gv(q));
      a.cv_pay[o + s] = Wk.L.gpay(q);
    }
  }
}

// carry copy: one lane per key copies its surviving suffix (virtual rows) into the new carry buffers
struct CarryBufs {
  int64_t* ts;
  int32_t* key;
  uint8_t* flags;
  void* col[SG_MAX_COLS];
  uint8_t* nul[SG_MAX_COLS];
};

// Carry of rows (HBM-list keys, and LDS rings that keep e1's row): the listed rows mark a bitmask, a count per
// 8192-row block and a scan place every survivor, and the survivors are copied in arrival order (per-key order stays
// arrival order = pending order, which is all the next push's stable key partition needs).
static const int CARRY_BLK = 8192;   // rows per block of the survivor count (256 bitmask words)

static __global__ void __launch_bounds__(256) k_carry_bcount(int64_t nt, const uint32_t* __restrict__ bits,
                                                             uint32_t* __restrict__ bcnt) {
  __shared__ uint32_t red[4];
  const int64_t wi = (int64_t)blockIdx.x * 256 + threadIdx.x;
  uint32_t c = wi * 32 < nt ? (uint32_t)__popc(bits[wi]) : 0u;
  for (int o = 32; o > 0; o >>= 1) c += (uint32_t)__shfl_xor((int)c, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) bcnt[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

static __global__ void __launch_bounds__(256) k_carry_gather(Virt v, int64_t nt, const uint32_t* __restrict__ bits,
                                                             const uint32_t* __restrict__ boff, int n_cols,
                                                             const int32_t* __restrict__ widths, SgCols bc, SgCols cc,
                                                             CarryBufs dst) {
  // 256 consecutive rows per step, one per thread: survivors of a step get consecutive slots (coalesced stores)
  __shared__ uint32_t wc[2][4];
  const uint32_t t = threadIdx.x, w = t >> 6, lane = t & 63;
  uint32_t base_d = boff[blockIdx.x];
  const int64_t r0 = (int64_t)blockIdx.x * CARRY_BLK;
  for (int step = 0; step < CARRY_BLK / 256; ++step) {
    const int64_t r64 = r0 + step * 256 + t;
    const bool live = r64 < nt && ((bits[r64 >> 5] >> (r64 & 31)) & 1u);
    const uint64_t m = __ballot(live);
    const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    if (lane == 0) wc[step & 1][w] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t before = 0;
    for (uint32_t q = 0; q < w; ++q) before += wc[step & 1][q];
    const uint32_t tot = wc[step & 1][0] + wc[step & 1][1] + wc[step & 1][2] + wc[step & 1][3];
    if (live) {
      const uint32_t d = base_d + before + below;
      const uint32_t r = (uint32_t)r64;
      dst.ts[d] = v_ts(v, r);
      dst.key[d] = r < v.nc ? v.c_key[r] : (v.key ? v.key[r - v.nc] : 0);
      dst.flags[d] = (uint8_t)(v_flags(v, r) | (v_visit(v, r) ? F_VISIT : 0u));
      const SgCols& s = r < v.nc ? cc : bc;
      const uint32_t rr = r < v.nc ? r : (uint32_t)(r - v.nc);
      for (int c = 0; c < n_cols; ++c) {
        if (!s.col[c]) continue;
        if (widths[c] == 8) ((int64_t*)dst.col[c])[d] = ((const int64_t*)s.col[c])[rr];
        else ((int32_t*)dst.col[c])[d] = ((const int32_t*)s.col[c])[rr];
        dst.nul[c][d] = s.nul[c] ? s.nul[c][rr] : 0;
      }
    }
    base_d += tot;
  }
}

// ----------------------------------------------------------------------------------------------
struct CarrySet {
  int64_t n = 0, cap = 0;
  int64_t* ts = nullptr;
  int32_t* key = nullptr;
  uint8_t* flags = nullptr;
  void* col[SG_MAX_COLS] = {};
  uint8_t* nul[SG_MAX_COLS] = {};
  void release() {
    hipFree(ts); hipFree(key); hipFree(flags);
    for (int c = 0; c < SG_MAX_COLS; ++c) { hipFree(col[c]); hipFree(nul[c]); col[c] = nullptr; nul[c] = nullptr; }
    ts = nullptr; key = nullptr; flags = nullptr;
    n = cap = 0;
  }
  void ensure(int64_t need, int n_cols, const int32_t* col_type) {
    if (need <= cap) return;
    release();
    int64_t c = std::max<int64_t>(need + need / 4, 1024);
    auto al = [](void** p, size_t b) { if (hipMalloc(p, b) != hipSuccess) throw SgError(SG_EHIP, "hipMalloc carry"); };
    al((void**)&ts, c * 8); al((void**)&key, c * 4); al((void**)&flags, c);
    for (int i = 0; i < n_cols; ++i) {
      al(&col[i], c * sg_col_width(col_type[i]));
      al((void**)&nul[i], c);
    }
    cap = c;
  }
};

struct EveryNextState {
  CarrySet carry[2];
  int cur = 0;
  bool nul_seen[SG_MAX_COLS] = {};   // a column that ever had nulls is gathered by row, never carried
};

// the carry copy's view of the set it fills, and the per-column byte widths (hw on the host, the result in HBM)
static CarryBufs carry_bufs(const sg_nfa_desc& d, const CarrySet& nx) {
  CarryBufs cb;
  memset(&cb, 0, sizeof(cb));
  cb.ts = nx.ts;
  cb.key = nx.key;
  cb.flags = nx.flags;
  for (int c = 0; c < d.n_cols; ++c) { cb.col[c] = nx.col[c]; cb.nul[c] = nx.nul[c]; }
  return cb;
}
static const int32_t* carry_widths(SgHandle* h, int32_t (&hw)[SG_MAX_COLS]) {
  int32_t* widths = (int32_t*)h->ws.get("col_widths", sizeof(int32_t) * SG_MAX_COLS, h->stream);
  for (int c = 0; c < SG_MAX_COLS; ++c) hw[c] = c < h->desc.n_cols ? sg_col_width(h->desc.col_type[c]) : 4;
  HIPCHK(hipMemcpyAsync(widths, hw, sizeof(int32_t) * SG_MAX_COLS, hipMemcpyHostToDevice, h->stream));
  return widths;
}

// Time chunks per key.  More chunks = more resident walker lanes, but every unit also replays the `within`
// window before its chunk: keep units at >= 2 windows of rows (estimated from the batch's time span) and at
// most one round of resident lanes (LDS holds 160 KiB / (STACK_CAP * entry) lanes per CU).
static int64_t window_rows(uint32_t K, int64_t nt, int64_t within, int64_t span_ms) {   // rows per key per window
  int64_t per_key = std::max<int64_t>(1, nt / std::max<uint32_t>(K, 1));
  return span_ms > 0 ? (int64_t)((double)per_key * (double)within / (double)span_ms) : per_key;
}
static int pick_cap(int64_t win) {   // a monotone stack over w random rows holds ~ln(w) partials
  return win < 300 ? 16 : (win < 5000 ? 32 : 64);
}
static constexpr int64_t WALK_LDS_MAX = 160 * 1024;   // gfx950 LDS per CU = per workgroup ceiling
// Largest ring (power of two) whose write-walk planes fit one workgroup's LDS.
static int clamp_cap(int cap, int entry_bytes_write) {
  while (cap > 2 && (int64_t)cap * WALK_BLOCK * entry_bytes_write > WALK_LDS_MAX) cap >>= 1;
  return cap;
}
// Chunks per key.  Each (key, chunk) unit replays the `within` window before its chunk, so chunks shorter
// than ~2 windows waste walker steps -- unless even such chunks leave the chip short of one walker lane
// per SIMD slot (few keys, long windows: the C1 shape), where parallelism beats replay cost.
static int pick_chunks(uint32_t K, int64_t nt, int entry_bytes, int cap, int64_t win) {
  int64_t blocks_per_cu = WALK_LDS_MAX / ((int64_t)cap * WALK_BLOCK * entry_bytes);
  int64_t target = std::max<int64_t>(blocks_per_cu, 1) * WALK_BLOCK * 256;
  int64_t per_key = std::max<int64_t>(1, nt / std::max<uint32_t>(K, 1));
  int64_t C = std::max<int64_t>(1, target / K);
  const int64_t c_cheap = std::max<int64_t>(1, per_key / std::max<int64_t>(256, 2 * win));
  const int64_t c_short = std::max<int64_t>(1, per_key / 256);
  const bool starved = (int64_t)K * c_cheap < 64 * 256;
  C = std::min<int64_t>(C, starved ? c_short : c_cheap);
  return (int)std::min<int64_t>(C, 1 << 16);
}

struct PushPlan {
  ProjPlan pp;
  int pcol = -1;              // e1 payload column carried in the pending list
  bool e1_row = false;        // some select gathers another e1 attribute by row
};

// f(std::integral_constant<int, OP>()) for the query's compare operator: 2 >, 3 >=, 4 <, anything else 5 <=
template <class F>
static void dispatch_op(int op, F&& f) {
  switch (op) {
    case 2: f(std::integral_constant<int, 2>()); break;
    case 3: f(std::integral_constant<int, 3>()); break;
    case 4: f(std::integral_constant<int, 4>()); break;
    default: f(std::integral_constant<int, 5>()); break;
  }
}

// B's place in its stream receiver: a receiver shared by several states delivers in reversed init order
// (eventSequence), so B's slot is its position from the end
static void recv_slot(const sg_nfa_desc& d, int b_state, int32_t& multi, int32_t& b_slot) {
  const sg_receiver_desc& r = d.receivers[d.recv_of_stream[d.states[b_state].stream]];
  multi = r.multi;
  b_slot = 0;
  if (multi)
    for (int q = 0; q < r.n; ++q)
      if (r.pres[r.n - 1 - q] == b_state) b_slot = q;
}

// What k_pack / k_part1 flagged about a push's narrow walker records.  A key beyond key_bound and an offset out of
// range are errors; a time or payload outside 32 bits sends the push to another record format.
enum PackRange { PACK_FITS, PACK_TS_RANGE, PACK_PAY_RANGE };
static PackRange pack_range(uint32_t pkf) {
  if (pkf & PK_KEY_RANGE) throw SgError(SG_EINVAL, "a partition key id is >= the batch's key_bound");
  if (pkf & PK_INTERNAL) throw SgError(SG_EINVAL, "internal: key partition offsets out of range");
  if (pkf & PK_TS_RANGE) return PACK_TS_RANGE;
  if (pkf & PK_PAY_RANGE) return PACK_PAY_RANGE;
  return PACK_FITS;
}

template <class T, bool N, bool WRITE>
static void launch_walk_t(int op, dim3 g, dim3 b, size_t lds, hipStream_t st, const WalkArgs& wa, const Src<T, N>& src,
                          const uint32_t* seg_b, const uint32_t* seg_e, UnitDesc* ud, const uint32_t* wlen,
                          const uint32_t* wrow, const WRec<T, N>* tile, uint32_t* cnt, const uint32_t* off, const MatchSink& ms,
                          uint64_t* emask, WalkStats* wst) {
  dispatch_op(op, [&](auto opc) {
    constexpr int OP = decltype(opc)::value;
    if (lds > 65536)
      HIPCHK(hipFuncSetAttribute((const void*)k_walk_t<T, N, OP, WRITE>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (int)lds));
    hipLaunchKernelGGL((k_walk_t<T, N, OP, WRITE>), g, b, lds, st, wa, src, seg_b, seg_e, ud, wlen, wrow, tile, cnt, off,
                       ms, emask, wst, ud);
  });
  HIPCHK(hipGetLastError());
}

// One push through the closed-form pipeline with walker records of format N (narrow / wide).  Returns false
// (having changed no state) when narrow records cannot represent the push (time span beyond 2^31 ms).
// ---------------------------------------------------------------------------------------------
// Unpartitioned streams: per-candidate search instead of the walker.  One key means the walker's units are
// time chunks of a single row sequence, each replaying a whole `within` window before it: few, long,
// latency-bound lanes (C1: 1000-row windows).  Every partial of this shape is independent:
// partial i leaves e2's list at the first later row of B's stream that either expires it (|ts_j - ts_i| > T,
// StreamPreStateProcessor.isExpired, C/query/input/stream/state/StreamPreStateProcessor.java:102-113 -- for any
// arrival order, so time going back needs no special case) or, as a consumer with x_j OP x_i, completes it
// (processAndReturn :292-337).  So one lane per candidate scans forward (lanes of a wave read neighbouring rows:
// coalesced); matches go to their slots by per-trigger counts, and a candidate whose scan reaches the end of the
// push is still pending: exactly those rows are carried into the next push.  A search longer than NGE_MAX_SCAN
// rows sends the push to the walker (bounded work per lane).
static const uint32_t NGE_MAX_SCAN = 4096;
static const uint32_t NGE_NONE = 0xffffffffu;

// per 64-row block of virtual rows: the most completing consumer value (max for > >=, min for < <=), whether the
// block has a live consumer at all, and the time range of its rows of B's stream -- a search skips a block that
// can neither complete nor expire its partial
template <class T, int OP>
__global__ void k_nge_blocks(Virt v, int64_t nt, T* __restrict__ best, uint8_t* __restrict__ has,
                             int64_t* __restrict__ bmin, int64_t* __restrict__ bmax) {
  const int64_t nb = (nt + 63) >> 6;
  for (int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; b < nb; b += (int64_t)gridDim.x * blockDim.x) {
    T m{};
    bool any = false;
    int64_t lo = INT64_MAX, hi = INT64_MIN;
    for (int64_t q = b << 6, e = (q + 64 < nt ? q + 64 : nt); q < e; ++q) {
      if (v_visit(v, (uint32_t)q)) {
        const int64_t t = v_ts(v, (uint32_t)q);
        lo = t < lo ? t : lo;
        hi = t > hi ? t : hi;
      }
      if (!(v_flags(v, (uint32_t)q) & F_CONS)) continue;
      const T x = v_val<T>(v, (uint32_t)q, false);
      if (is_nan_val<T>(x)) continue;
      if (!any || ((OP == 2 || OP == 3) ? x > m : x < m)) m = x;
      any = true;
    }
    best[b] = m;
    has[b] = any ? 1 : 0;
    bmin[b] = lo;
    bmax[b] = hi;
  }
}

template <class T, int OP>
__global__ void __launch_bounds__(256) k_nge(Virt v, int64_t nt, int64_t within, int op, uint32_t* __restrict__ mj,
                                             uint32_t* __restrict__ rank, uint32_t* __restrict__ cnt,
                                             uint32_t* __restrict__ st_flags, const T* __restrict__ best,
                                             const uint8_t* __restrict__ has, const int64_t* __restrict__ bmin,
                                             const int64_t* __restrict__ bmax, uint32_t* __restrict__ alive) {
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < nt; p += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t f = v_flags(v, (uint32_t)p);
    uint32_t j = NGE_NONE;
    if (f & F_CAND) {
      const T xp = v_val<T>(v, (uint32_t)p, true);
      const int64_t tp = v_ts(v, (uint32_t)p);
      if (!is_nan_val<T>(xp)) {
        uint32_t steps = 0;
        bool open = true;   // still pending when the scan reaches the end of the push
        bool done = false;
        int64_t q = p + 1;
        while (q < nt && !done) {
          if ((q & 63) == 0 && q + 64 <= nt && !(has[q >> 6] && cmp_sel<OP, T>(op, best[q >> 6], xp)) &&
              bmax[q >> 6] <= tp + within && bmin[q >> 6] >= tp - within) {
            if (++steps > NGE_MAX_SCAN) { atomicOr(&st_flags[1], 1u); open = false; break; }
            q += 64;                                                       // nothing in this block ends i
            continue;
          }
          // the rows up to the next multiple of 8: every load issued before the first test (one memory latency per
          // eight rows instead of one per row; most searches end within a few rows)
          const int64_t ge = ((q & ~(int64_t)7) + 8) < nt ? (q & ~(int64_t)7) + 8 : nt;
          int64_t tq[8];
          uint32_t fq[8];
          bool vq[8];
          T xq[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            const int64_t r = q + u < ge ? q + u : ge - 1;
            tq[u] = v_ts(v, (uint32_t)r);
            fq[u] = v_flags(v, (uint32_t)r);
            vq[u] = v_visit(v, (uint32_t)r);
            xq[u] = v_val<T>(v, (uint32_t)r, false);
          }
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            if (done || q + u >= ge) continue;
            if (++steps > NGE_MAX_SCAN) { atomicOr(&st_flags[1], 1u); open = false; done = true; continue; }
            if ((tq[u] - tp > within || tp - tq[u] > within) && vq[u]) { open = false; done = true; continue; }   // expired
            if ((fq[u] & F_CONS) && !is_nan_val<T>(xq[u]) && cmp_sel<OP, T>(op, xq[u], xp)) {
              if (q + u >= v.nc) j = (uint32_t)(q + u);                    // (carried triggers were emitted before)
              open = false;
              done = true;
            }
          }
          q = ge;
        }
        if (open && alive) atomicOr(&alive[p >> 5], 1u << (p & 31));
      }
    }
    mj[p] = j;
    if (j != NGE_NONE) rank[p] = atomicAdd(&cnt[j - v.nc], 1u);   // (rank among the trigger's matches: any order)
  }
}

// every match to its delivery slot: the trigger's offset + the rank the search drew; then each trigger's matches in
// pending (= arrival) order of their partials
template <class T>
__global__ void k_nge_place(Virt v, int64_t nt, const uint32_t* __restrict__ mj, const uint32_t* __restrict__ rank,
                            const uint32_t* __restrict__ off, MRec* __restrict__ mrec) {
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < nt; p += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t j = mj[p];
    if (j == NGE_NONE) continue;
    MRec m;
    m.r1 = (uint32_t)p;
    m.r2 = j;
    m.v1 = val_bits<T>(v_val<T>(v, (uint32_t)p, true));
    m.p1 = v.pcol ? v_payload(v, (uint32_t)p) : 0;
    mrec[off[j - v.nc] + rank[p]] = m;
  }
}

// Each trigger's matches into pending order (ascending e1 row).  Triggers with up to NGE_ORDER_SMALL matches are
// insertion-sorted by their own lane; larger ones (a long run of candidates completed by one row) are flagged and
// sorted by a segmented radix sort afterwards, so no lane does quadratic work.
static const uint32_t NGE_ORDER_SMALL = 32;
static __global__ void k_nge_order(int64_t n, const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ off,
                                   MRec* __restrict__ mrec, uint32_t* __restrict__ nbig) {
  for (int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; b < n; b += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t c = cnt[b];
    if (c < 2) continue;
    if (c > NGE_ORDER_SMALL) { atomicAdd(nbig, c); continue; }
    MRec* e = mrec + off[b];
    for (uint32_t i = 1; i < c; ++i) {
      const MRec x = e[i];
      uint32_t k = i;
      while (k > 0 && e[k - 1].r1 > x.r1) {
        e[k] = e[k - 1];
        --k;
      }
      e[k] = x;
    }
  }
}

// large triggers: (trigger slot, e1 row) keys of their matches, then one stable radix sort orders every match
static __global__ void k_nge_bigkeys(int64_t total, const MRec* __restrict__ mrec, const uint32_t* __restrict__ mj,
                                     const uint32_t* __restrict__ off, int64_t nc, uint64_t* __restrict__ key,
                                     uint32_t* __restrict__ idx) {
  for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < total; s += (int64_t)gridDim.x * blockDim.x) {
    const MRec m = mrec[s];
    key[s] = ((uint64_t)off[m.r2 - nc] << 32) | m.r1;
    idx[s] = (uint32_t)s;
  }
}
static __global__ void k_nge_permute(int64_t total, const MRec* __restrict__ src, const uint32_t* __restrict__ idx,
                                     MRec* __restrict__ dst) {
  for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < total; s += (int64_t)gridDim.x * blockDim.x)
    dst[s] = src[idx[s]];
}

template <class T>
static bool run_nge(SgHandle* h, const BatchView& bv, int64_t n, int64_t nc, const PushPlan& plan, const Virt& v,
                    const SgCols& cc, int op, EveryNextState* es) {
  const sg_nfa_desc& d = h->desc;
  hipStream_t st = h->stream;
  const int64_t nt = nc + n;
  const int b_state = d.shape_args[1];
  auto grid = [](int64_t m) { return dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>((m + 255) / 256, 256 * 16))); };
  uint32_t* mj = (uint32_t*)h->ws.get("nge_mj", 4 * nt, st);
  uint32_t* rank = (uint32_t*)h->ws.get("nge_rank", 4 * nt, st);
  uint32_t* cnt = (uint32_t*)h->ws.get("cnt", sizeof(uint32_t) * (n + 1), st);
  uint32_t* off = (uint32_t*)h->ws.get("off", sizeof(uint32_t) * (n + 1), st);
  uint32_t* stf = (uint32_t*)h->ws.get("nge_flags", 16, st);
  const bool carry = !h->opt.no_carry && nt > 0;
  const int64_t cnb = (nt + CARRY_BLK - 1) / CARRY_BLK;
  uint32_t* cbits = carry ? (uint32_t*)h->ws.get("carry_bits", sizeof(uint32_t) * (size_t)(cnb * 256), st) : nullptr;
  HIPCHK(hipMemsetAsync(cnt, 0, sizeof(uint32_t) * (n + 1), st));
  HIPCHK(hipMemsetAsync(stf, 0, 16, st));
  if (carry) HIPCHK(hipMemsetAsync(cbits, 0, sizeof(uint32_t) * (size_t)(cnb * 256), st));
  const int64_t nb = (nt + 63) >> 6;
  T* best = (T*)h->ws.get("nge_best", sizeof(T) * (nb + 1), st);
  uint8_t* has = (uint8_t*)h->ws.get("nge_has", nb + 1, st);
  int64_t* bmin = (int64_t*)h->ws.get("nge_bmin", sizeof(int64_t) * (nb + 1), st);
  int64_t* bmax = (int64_t*)h->ws.get("nge_bmax", sizeof(int64_t) * (nb + 1), st);
  h->kbeg("nge_search");
  dispatch_op(op, [&](auto opc) {
    constexpr int OP = decltype(opc)::value;
    hipLaunchKernelGGL((k_nge_blocks<T, OP>), grid(nb), dim3(256), 0, st, v, nt, best, has, bmin, bmax);
    hipLaunchKernelGGL((k_nge<T, OP>), grid(nt), dim3(256), 0, st, v, nt, d.within, op, mj, rank, cnt, stf, best, has,
                       bmin, bmax, cbits);
  });
  HIPCHK(hipGetLastError());
  h->kend();
  h->mark(2);
  sg_exclusive_scan(h->ws, st, "scan_tmp", cnt, off, (uint32_t)0, (size_t)n + 1, rocprim::plus<uint32_t>());
  uint32_t hflags[4] = {0, 0, 0, 0};
  uint32_t total = 0;
  HIPCHK(hipMemcpyAsync(hflags, stf, 16, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(&total, off + n, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (hflags[1]) return false;   // a search outgrew NGE_MAX_SCAN: the walker takes this push
  MRec* mrec = nullptr;
  if (total) {
    mrec = (MRec*)h->ws.get("mrec", sizeof(MRec) * total, st);
    hipLaunchKernelGGL((k_nge_place<T>), grid(nt), dim3(256), 0, st, v, nt, mj, rank, off, mrec);
    hipLaunchKernelGGL(k_nge_order, grid(n), dim3(256), 0, st, n, cnt, off, mrec, stf + 2);
    HIPCHK(hipGetLastError());
    uint32_t nbig = sg_read_back(stf + 2, st);
    if (nbig) {
      // a trigger completed more than NGE_ORDER_SMALL partials: order every match by (trigger slot, e1 row)
      uint64_t* k1 = (uint64_t*)h->ws.get("nge_k1", 8 * (size_t)total, st);
      uint64_t* k2 = (uint64_t*)h->ws.get("nge_k2", 8 * (size_t)total, st);
      uint32_t* i1 = (uint32_t*)h->ws.get("nge_i1", 4 * (size_t)total, st);
      uint32_t* i2 = (uint32_t*)h->ws.get("nge_i2", 4 * (size_t)total, st);
      MRec* m2 = (MRec*)h->ws.get("mrec2", sizeof(MRec) * total, st);
      hipLaunchKernelGGL(k_nge_bigkeys, grid(total), dim3(256), 0, st, (int64_t)total, mrec, mj, off, nc, k1, i1);
      sg_radix_sort_pairs(h->ws, st, "nge_sort_tmp", k1, k2, i1, i2, (size_t)total, 64);
      hipLaunchKernelGGL(k_nge_permute, grid(total), dim3(256), 0, st, (int64_t)total, mrec, i2, m2);
      HIPCHK(hipGetLastError());
      mrec = m2;
    }
  }
  h->mark(3);
  h->extra_marks = 0;
  h->split_out = 1;
  WalkArgs wa;
  memset(&wa, 0, sizeof(wa));
  wa.partitioned = 0;
  wa.base_index = bv.base_index;
  wa.index = bv.index;
  recv_slot(d, b_state, wa.multi, wa.b_slot);
  wa.n_select = d.n_select;
  wa.stride = 32 + 8 * d.n_select;
  char* out = h->out.reserve(total, d.n_select, st);
  wa.out_base = h->out.n;
  h->mark(5);
  if (total) {
    h->kbeg("project");
    hipLaunchKernelGGL((k_project<T>), dim3((unsigned)(((int64_t)total + 255) / 256)), dim3(256), (size_t)256 * wa.stride, st,
                       wa, v, plan.pp, bv.cols, cc, MatchSink{mrec, 0, (uint32_t)total, nullptr}, off, (int64_t)total, out);
    h->kend();
    HIPCHK(hipGetLastError());
  }
  h->out.n += total;
  h->mark(4);
  // carry: the partials still pending at the end of the push
  if (carry) {
    CarrySet& cs = es->carry[es->cur];
    uint32_t* cboff = (uint32_t*)h->ws.get("carry_boff", sizeof(uint32_t) * (size_t)(cnb + 1), st);
    uint32_t* bcnt = (uint32_t*)h->ws.get("carry_bcnt", sizeof(uint32_t) * (size_t)(cnb + 1), st);
    hipLaunchKernelGGL(k_carry_bcount, dim3((unsigned)cnb), dim3(256), 0, st, nt, cbits, bcnt);
    HIPCHK(hipMemsetAsync(bcnt + cnb, 0, sizeof(uint32_t), st));
    sg_exclusive_scan(h->ws, st, "carry_scan_tmp", bcnt, cboff, (uint32_t)0, (size_t)cnb + 1, rocprim::plus<uint32_t>());
    uint32_t ncar = sg_read_back(cboff + cnb, st);
    CarrySet& nx = es->carry[es->cur ^ 1];
    nx.ensure(std::max<int64_t>(ncar, 1), d.n_cols, d.col_type);
    int32_t hw[SG_MAX_COLS];
    const int32_t* widths = carry_widths(h, hw);
    const CarryBufs cbuf = carry_bufs(d, nx);
    if (ncar)
      hipLaunchKernelGGL(k_carry_gather, dim3((unsigned)cnb), dim3(256), 0, st, v, nt, cbits, cboff, d.n_cols, widths,
                         bv.cols, cc, cbuf);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    nx.n = ncar;
    cs.n = 0;
    es->cur ^= 1;
  }
  h->last_events = n;
  h->last_matches = total;
  h->last_spilled = 0;
  return true;
}

// keys whose rows (sorted positions of one key, carried rows first) go back in time
template <class T, bool N>
__global__ void k_order_keys(Src<T, N> src, KeyOf kf, const uint32_t* __restrict__ seg_b, uint32_t K, int64_t nt,
                             uint8_t* __restrict__ kx) {
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x + 1; p < nt; p += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t k = kf(src.row((uint32_t)p));
    if (k < K && (uint32_t)p > seg_b[k] && src.ts((uint32_t)p) < src.ts((uint32_t)(p - 1))) kx[k] = 1;
  }
}

// rows listed in rows[0, *n) -> carry bitmask (the pending partials of every key the rows list)
static __global__ void k_carry_mark_list(const uint32_t* __restrict__ rows, const uint32_t* __restrict__ n,
                                         uint32_t* __restrict__ bits) {
  const uint32_t m = *n;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < m; i += gridDim.x * blockDim.x)
    atomicOr(&bits[rows[i] >> 5], 1u << (rows[i] & 31));
}

// pending entries kept as values (LDS rings without a row plane) -> carried candidate rows [base, base + n): time,
// key, the compared value and e1's payload attribute; every other column of such a row is never read (no select
// gathers an e1 attribute by row when the ring has no row plane, and a carried row is never a B row)
template <class T>
__global__ void k_carry_vals(uint32_t n, const int64_t* __restrict__ cts, const int32_t* __restrict__ ckey,
                             const int64_t* __restrict__ cval, const int64_t* __restrict__ cpay, int val_col, int pay_col,
                             int pay_w, int n_cols, uint32_t base, CarryBufs dst) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t d = base + i;
  dst.ts[d] = cts[i];
  dst.key[d] = ckey[i];
  dst.flags[d] = (uint8_t)F_CAND;
  const uint64_t vb = (uint64_t)cval[i];
  T x;
  if constexpr (sizeof(T) == 4) { const uint32_t w = (uint32_t)vb; __builtin_memcpy(&x, &w, 4); }
  else __builtin_memcpy(&x, &vb, 8);
  ((T*)dst.col[val_col])[d] = x;
  if (pay_col >= 0) {
    if (pay_w == 8) ((int64_t*)dst.col[pay_col])[d] = cpay[i];
    else ((int32_t*)dst.col[pay_col])[d] = (int32_t)cpay[i];
  }
  for (int c = 0; c < n_cols; ++c) dst.nul[c][d] = 0;
}

// The next push's carried rows: every key's final pending list -- listed rows (alive) copied in arrival order, then
// the entries kept as values (cv) appended.  Per key one of the two; per key pending order.
template <class T, bool N>
static void carry_out_rows(SgHandle* h, EveryNextState* es, int64_t nt, const Virt& v, const BatchView& bv,
                           const SgCols& cc, const WalkArgs& wa, int val_col, int pay_col, int pay_w) {
  const sg_nfa_desc& d = h->desc;
  hipStream_t st = h->stream;
  CarrySet& cs = es->carry[es->cur];
  uint32_t* ccount = (uint32_t*)h->ws.get("carry_count", sizeof(uint32_t) * 2, st);
  h->kbeg("carry");
  const int64_t nb = (nt + CARRY_BLK - 1) / CARRY_BLK;
  uint32_t* cbits = (uint32_t*)h->ws.get("carry_bits", sizeof(uint32_t) * (size_t)(nb * 256), st);
  uint32_t* cboff = (uint32_t*)h->ws.get("carry_boff", sizeof(uint32_t) * (size_t)(nb + 1), st);
  uint32_t* bcnt = (uint32_t*)h->ws.get("carry_bcnt", sizeof(uint32_t) * (size_t)(nb + 1), st);
  HIPCHK(hipMemsetAsync(cbits, 0, sizeof(uint32_t) * (size_t)(nb * 256), st));
  hipLaunchKernelGGL(k_carry_mark_list, dim3((unsigned)std::min<int64_t>((nt + 255) / 256, 4096)), dim3(256), 0, st,
                     wa.alive, wa.alive_n, cbits);
  hipLaunchKernelGGL(k_carry_bcount, dim3((unsigned)nb), dim3(256), 0, st, nt, cbits, bcnt);
  HIPCHK(hipMemsetAsync(bcnt + nb, 0, sizeof(uint32_t), st));
  HIPCHK(hipGetLastError());
  sg_exclusive_scan(h->ws, st, "carry_scan_tmp", bcnt, cboff, (uint32_t)0, (size_t)nb + 1, rocprim::plus<uint32_t>());
  HIPCHK(hipMemcpyAsync(ccount, cboff + nb, sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
  HIPCHK(hipMemcpyAsync(ccount + 1, wa.cv_n, sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
  h->kend();
  uint32_t hc[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(hc, ccount, sizeof(hc), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  const uint32_t nrow = hc[0], nval = hc[1];
  CarrySet& nx = es->carry[es->cur ^ 1];
  nx.ensure(std::max<int64_t>((int64_t)nrow + nval, 1), d.n_cols, d.col_type);
  int32_t hw[SG_MAX_COLS];
  const int32_t* widths = carry_widths(h, hw);
  const CarryBufs cb = carry_bufs(d, nx);
  if (nrow)
    hipLaunchKernelGGL(k_carry_gather, dim3((unsigned)nb), dim3(256), 0, st, v, nt, cbits, cboff, d.n_cols, widths,
                       bv.cols, cc, cb);
  if (nval) {
    for (int c = 0; c < d.n_cols; ++c)   // (columns the value entries do not set: deterministic snapshots)
      if (c != val_col && c != pay_col)
        HIPCHK(hipMemsetAsync((char*)nx.col[c] + (size_t)hw[c] * nrow, 0, (size_t)hw[c] * nval, st));
    hipLaunchKernelGGL(k_carry_vals<T>, dim3((nval + 255) / 256), dim3(256), 0, st, nval, wa.cv_ts, wa.cv_key, wa.cv_val,
                       wa.cv_pay, val_col, pay_col, pay_w, d.n_cols, nrow, cb);
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st));
  nx.n = (int64_t)nrow + nval;
  cs.n = 0;
  es->cur ^= 1;
}
