// walk_rec.h -- what the closed form's key partition and its walkers share: the virtual row domain of a push (Virt,
// KeyOf), the walker record formats (WRec) and how a record is built from a row (PackFn, k_pack), the walkers' view of
// the records (Src), and the per-key segments of radix-sorted records (k_bounds).
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>

#include "pred.h"
#include "sg_device.h"
#include "sg_engine.h"

static const uint32_t F_CAND = 1, F_CONS = 2;
static const int WALK_BLOCK = 256;
static const int STACK_CAP = 16;   // default LDS pending-list ring entries per lane (runtime: 16/32/64)
static const int PF = 8;           // rows prefetched per lane per step

// ---------------------------------------------------------------------------------------------
// virtual row domain: [0, nc) carried rows of earlier pushes, [nc, nc + n) this batch
struct Virt {
  int64_t nc, n;
  const int64_t* ts;
  const int32_t* key;
  const uint64_t* cand_m;
  const uint64_t* cons_m;     // null: every batch row is a B consumer
  const void* val_a;
  const void* val_b;
  const int64_t* c_ts;
  const int32_t* c_key;
  const uint8_t* c_flags;
  const void* c_val_a;
  const void* c_val_b;
  const void* pcol;           // e1 payload column (one projected attribute carried in the pending list)
  const void* c_pcol;
  int32_t pw, pfloat;         // width 4/8; FLOAT bits zero-extended, integral sign-extended
  const int32_t* stream;      // batch stream column (null: every row is stream 0)
  int32_t s_b;                // B's stream: its rows visit e2's pending list (expiry), whatever their filters say
};

struct KeyOf {   // sort key of virtual row r (the dense partition key; -1 sorts last)
  const int32_t* key;
  const int32_t* c_key;
  uint32_t nc;
  __host__ __device__ uint32_t operator()(uint32_t r) const {
    return (uint32_t)(r < nc ? c_key[r] : key[r - nc]);
  }
};

// carried rows keep F_CAND / F_CONS in bits 0-1 and F_VISIT (a row of B's stream) in bit 2
static const uint32_t F_VISIT = 4;
__device__ __forceinline__ uint32_t v_flags(const Virt& v, uint32_t r) {
  if (r < v.nc) return v.c_flags[r] & 3u;
  uint64_t b = r - v.nc;
  uint32_t f = mask_bit(v.cand_m, b);
  f |= v.cons_m ? (mask_bit(v.cons_m, b) << 1) : F_CONS;
  return f;
}
// Does virtual row r visit e2's pending list?  Every row of B's stream does (MultiProcessStreamReceiver.receive ->
// StreamPreStateProcessor.processAndReturn, C/query/input/stream/state/StreamPreStateProcessor.java:292-337): its
// `within` expiry applies whether or not the row passes a filter.
__device__ __forceinline__ bool v_visit(const Virt& v, uint32_t r) {
  if (r < v.nc) return (v.c_flags[r] & F_VISIT) != 0;
  return (v.stream ? v.stream[r - v.nc] : 0) == v.s_b;
}
__device__ __forceinline__ int64_t v_ts(const Virt& v, uint32_t r) { return r < v.nc ? v.c_ts[r] : v.ts[r - v.nc]; }
template <class T>
__device__ __forceinline__ T v_val(const Virt& v, uint32_t r, bool side_a) {
  if (r < v.nc) return ((const T*)(side_a ? v.c_val_a : v.c_val_b))[r];
  return ((const T*)(side_a ? v.val_a : v.val_b))[r - v.nc];
}

__device__ __forceinline__ int64_t v_payload(const Virt& v, uint32_t r) {
  const void* c = r < v.nc ? v.c_pcol : v.pcol;
  uint32_t rr = r < v.nc ? r : (uint32_t)(r - v.nc);
  if (v.pw == 8) return ((const int64_t*)c)[rr];
  int32_t x = ((const int32_t*)c)[rr];
  return v.pfloat ? (int64_t)(uint32_t)x : (int64_t)x;
}

// Walker record: one row of one key as the walkers read it (key-sorted for partitioned queries).
// rowf = virtual row | condition flags << 30.  Narrow format (default): time as a 32-bit offset from the
// push's first virtual row, plus (4-byte values) e1's payload attribute in 32 bits -- 16 bytes, rocPRIM's
// tuned 8-bit-digit onesweep path and 8 records per 128-B line.  Wide format (fallback when a push spans
// more than 2^31 ms): 64-bit time, no payload.
static const uint32_t ROW_MASK = 0x3fffffffu;
template <class T, bool N, int S = (int)sizeof(T)>
struct WRec {   // wide
  int64_t ts;
  uint32_t rowf;
  T val;
  static constexpr bool has_pay = false;
  static constexpr bool narrow = false;
  __host__ __device__ int64_t t() const { return ts; }
  __host__ __device__ int64_t p(int) const { return 0; }
};
template <class T>
struct WRec<T, true, 4> {   // narrow, 4-byte value: room for a 32-bit payload
  int32_t dts;
  uint32_t rowf;
  T val;
  int32_t pay;
  static constexpr bool has_pay = true;
  static constexpr bool narrow = true;
  __host__ __device__ int64_t t() const { return dts; }
  __host__ __device__ int64_t p(int pzero) const { return pzero ? (int64_t)(uint32_t)pay : (int64_t)pay; }
};
template <class T>
struct WRec<T, true, 8> {   // narrow, 8-byte value
  int32_t dts;
  uint32_t rowf;
  T val;
  static constexpr bool has_pay = false;
  static constexpr bool narrow = true;
  __host__ __device__ int64_t t() const { return dts; }
  __host__ __device__ int64_t p(int) const { return 0; }
};
struct alignas(16) Blob16 { uint32_t w[4]; };   // 16-byte records sort as one opaque type

static const uint32_t PK_TS_RANGE = 1, PK_PAY_RANGE = 2, PK_KEY_RANGE = 4, PK_INTERNAL = 8;   // k_pack flags

template <class T, bool N>
struct PackFn {   // builds the walker record of virtual row r (coalesced when r is sequential)
  Virt v;
  __host__ __device__ WRec<T, N> operator()(uint32_t r) const {
    WRec<T, N> o;
#ifdef __HIP_DEVICE_COMPILE__
    uint32_t f = v_flags(v, r);
    if constexpr (N) {
      o.dts = (int32_t)(v_ts(v, r) - v_ts(v, 0));
      if constexpr (WRec<T, N>::has_pay) o.pay = v.pcol ? (int32_t)v_payload(v, r) : 0;
    } else {
      o.ts = v_ts(v, r);
    }
    o.rowf = r | (f << 30);
    o.val = v_val<T>(v, r, (f & F_CAND) || v.val_a == v.val_b);
#else
    (void)r;
    memset(&o, 0, sizeof(o));
#endif
    return o;
  }
  // batch row b (virtual row nc + b) without the carried-row branches, so a run of rows issues its loads
  // back to back; also flags a time / payload outside the narrow format's 32 bits
  __device__ __forceinline__ WRec<T, N> batch(uint32_t b, int64_t t0, uint32_t& bad) const {
    WRec<T, N> o;
    uint32_t f = mask_bit(v.cand_m, b);
    f |= v.cons_m ? (mask_bit(v.cons_m, b) << 1) : F_CONS;
    const int64_t ts = v.ts[b];
    if constexpr (N) {
      const int64_t dt = ts - t0;
      bad |= (dt != (int64_t)(int32_t)dt) ? PK_TS_RANGE : 0u;
      o.dts = (int32_t)dt;
      if constexpr (WRec<T, N>::has_pay) {
        int64_t pv = 0;
        if (v.pcol) {   // (uniform)
          if (v.pw == 8) {
            pv = ((const int64_t*)v.pcol)[b];
            bad |= (pv != (int64_t)(int32_t)pv) ? PK_PAY_RANGE : 0u;
          } else {
            pv = ((const int32_t*)v.pcol)[b];
          }
        }
        o.pay = (int32_t)pv;
      }
    } else {
      o.ts = ts;
    }
    o.rowf = (uint32_t)(v.nc + b) | (f << 30);
    const T* src = ((f & F_CAND) || v.val_a == v.val_b) ? (const T*)v.val_a : (const T*)v.val_b;
    o.val = src[b];
    return o;
  }
};

template <class T, bool N>
struct Src {   // position -> record: the key-sorted records, or (unpartitioned) the rows themselves
  const WRec<T, N>* srec;
  PackFn<T, N> pk;
  __device__ __forceinline__ WRec<T, N> at(uint32_t p) const { return srec ? srec[p] : pk(p); }
  __device__ __forceinline__ uint32_t row(uint32_t p) const { return srec ? (srec[p].rowf & ROW_MASK) : p; }
  __device__ __forceinline__ int64_t ts(uint32_t p) const { return srec ? srec[p].t() : pk(p).t(); }
};

// walker records + sort keys of every virtual row, in arrival order (coalesced).  Narrow records flag a
// time outside +-2^31 ms of the first virtual row, or a payload that does not fit 32 bits.
template <class T, bool N>
__global__ void __launch_bounds__(256) k_pack(PackFn<T, N> pk, KeyOf kf, uint32_t kbound, int64_t nt,
                                              WRec<T, N>* __restrict__ rec, uint32_t* __restrict__ keys,
                                              uint32_t* __restrict__ flags) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  uint32_t bad = 0;
  const int64_t t0 = N ? v_ts(pk.v, 0) : 0;
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < nt; r += stride) {
    rec[r] = pk((uint32_t)r);
    if (keys) {
      const uint32_t kk = kf((uint32_t)r);
      if (kk >= kbound && kk != 0xffffffffu) bad |= PK_KEY_RANGE;   // beyond the caller's key_bound
      keys[r] = kk;
    }
    if (N) {
      const int64_t d = v_ts(pk.v, (uint32_t)r) - t0;
      if (d != (int64_t)(int32_t)d) bad |= PK_TS_RANGE;
      if (WRec<T, N>::has_pay && pk.v.pcol && pk.v.pw == 8) {
        const int64_t pv = v_payload(pk.v, (uint32_t)r);
        if (pv != (int64_t)(int32_t)pv) bad |= PK_PAY_RANGE;
      }
    }
  }
  if (bad) atomicOr(flags, bad);
}

static __global__ void __launch_bounds__(256) k_bounds(const uint32_t* __restrict__ skey, int64_t n, uint32_t kb,
                                                       uint32_t* __restrict__ seg_b, uint32_t* __restrict__ seg_e) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x * 4;
  for (int64_t t0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4; t0 < n; t0 += stride) {
    uint32_t k[6];
    k[0] = t0 > 0 ? skey[t0 - 1] : 0xffffffffu;
#pragma unroll
    for (int j = 0; j < 5; ++j) k[j + 1] = (t0 + j < n) ? skey[t0 + j] : 0xfffffffeu;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      int64_t t = t0 + j;
      uint32_t x = k[j + 1];
      if (t >= n || x >= kb) continue;
      if (k[j] != x) seg_b[x] = (uint32_t)t;
      if (k[j + 2] != x) seg_e[x] = (uint32_t)(t + 1);
    }
  }
}
