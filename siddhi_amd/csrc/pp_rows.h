// pp_rows.h -- what both lane routes (partial.hip) share around the lanes themselves: the carried rows, the front end
// that puts the push's rows (carried rows first, then the batch) in key order and packs what a lane reads at every
// step, and the carry that hands rows on to the next push.  Kernels first, then the host side (key_ordered_rows,
// carry_rows).
#pragma once
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include <algorithm>
#include <cstring>
#include <string>

#include "sg_engine.h"
#include "sg_prim.h"
#include "pred.h"
#include "pp_state.h"

struct PpArgs {
  int64_t nc;                 // carried rows (combined rows [0, nc)); batch row r is combined row nc + r
  int64_t n;
  uint64_t base_index;
  const uint64_t* index;
  const int64_t* bts;
  const int64_t* cts;
  const int32_t* stream;
  const int32_t* bkey;
  const int32_t* ckey;
  const uint64_t* lbits[SG_MAX_STATES];
  int32_t any_bits;
  const uint8_t* cstart;      // partial lanes: carried row starts a lane
  uint32_t* keep;             // partial lanes: per sorted position, 1 = carried into the next push
  uint8_t* kstart;            // partial lanes: per sorted position, 1 = the carried row starts a lane
  const uint8_t* kback;       // partial lanes: per key, its time goes back somewhere in this push (carried rows included)
  int64_t drop_before;        // partial lanes: a pending partial whose e1 is older than this is not carried
                              // (sg_options.bounded_lateness; INT64_MIN = carry every pending partial)
  int64_t dead_after;         // partial lanes: a partial at a row more than this after e1 is dead (within + lateness;
                              // INT64_MAX without bounded_lateness)
};

// Key-ordered packed rows (position q = the q-th row of the key partition): what a lane reads at every step, so the
// 64 lanes of a wave (consecutive start rows of one key) read neighbouring addresses.
struct PpPacked {
  int64_t* ts;                  // (nullptr: read through sid, lazy -- sequence lanes only need it for matches)
  void* val[SG_MAX_RET];        // retained slot k: 4- or 8-byte bit patterns (nullptr: lazy, read through sid)
  int32_t wide[SG_MAX_RET];
  uint32_t* nul;                // null mask over retained slots (nullptr: no nulls in this push)
  uint32_t* lb;                 // condition bits of the event-local filters (rule.local_mask)
  // lazy reads: the row's own column through the combined row id (carried rows first)
  const uint32_t* sid;
  int64_t nc;
  const int64_t* bts;
  const int64_t* cts;
  const void* bcol[SG_MAX_RET];
  const void* ccol[SG_MAX_RET];
  // wait skipping (chain.h PpLane::wait_on): per wait attribute, {min, max} encodings of every 8 key-ordered rows
  const uint2* wsum;            // nullptr: no skipping in this push (no wait term, or nulls in a column)
  int64_t wnb;                  // 8-row blocks
  int8_t wix[SG_MAX_RET];       // retained slot -> summary index
};
__device__ __forceinline__ int64_t pp_lazy_ts(const PpPacked* P, int64_t q) {
  const int64_t c = P->sid[q];
  return c < P->nc ? P->cts[c] : P->bts[c - P->nc];
}
__device__ __forceinline__ int64_t pp_lazy_bits(const PpPacked* P, int64_t q, int k) {
  const int64_t c = P->sid[q];
  const bool cr = c < P->nc;
  const void* col = cr ? P->ccol[k] : P->bcol[k];
  const int64_t r = cr ? c : c - P->nc;
  return P->wide[k] ? ((const int64_t*)col)[r] : (int64_t)((const int32_t*)col)[r];
}

struct PpSrc {
  const PpPacked* P;
  __device__ int64_t ts(int64_t q) const { return P->ts[q]; }
  __device__ SgVal read(int64_t q, int slotk, int type) const {
    const int null = P->nul ? (int)((P->nul[q] >> slotk) & 1u) : 0;
    const int64_t bits = P->wide[slotk] ? ((const int64_t*)P->val[slotk])[q] : (int64_t)((const int32_t*)P->val[slotk])[q];
    return sg_val_from_bits(bits, type, null);
  }
  __device__ int lbit(int s, int64_t q) const { return (int)((P->lb[q] >> s) & 1u); }
  __device__ void read_bits(int64_t q, int slotk, int type, int64_t& bits, int& null) const {
    null = P->nul ? (int)((P->nul[q] >> slotk) & 1u) : 0;
    bits = P->wide[slotk] ? ((const int64_t*)P->val[slotk])[q] : (int64_t)((const int32_t*)P->val[slotk])[q];
  }
};

__global__ void k_pp_route(PpArgs a, const DevDesc* __restrict__ dd, int partitioned, uint32_t sentinel,
                           uint32_t* __restrict__ okey, uint32_t* __restrict__ orow, int32_t* __restrict__ err) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.nc + a.n) return;
  uint32_t k = sentinel;
  if (i < a.nc) {
    k = partitioned ? (uint32_t)a.ckey[i] : 0u;
  } else {
    const int64_t r = i - a.nc;
    const int s = a.stream ? a.stream[r] : 0;
    if (s >= 0 && s < SG_MAX_STREAMS && dd->recv_of_stream[s] >= 0) {
      if (!partitioned) k = 0;
      else {
        const int32_t kk = a.bkey ? a.bkey[r] : -1;
        if (kk >= 0) {
          if ((uint32_t)kk >= sentinel) atomicOr(err, 2);
          else k = (uint32_t)kk;
        }
      }
    }
  }
  okey[i] = k;
  orow[i] = (uint32_t)i;
}

// ---- record sort: the rows' per-step fields travel through the key sort as one 16-byte record, so the key-ordered
// rows come out of the sort instead of a gather over the whole batch.  Record: {combined row (| start flag << 31 for
// partial lanes), timestamp - tbase (partial lanes) or event-local condition bits (sequence lanes), hot word 0,
// hot word 1}.
struct alignas(16) PpRec { uint32_t w[4]; };

struct RecArgs {
  int32_t mode, start, partitioned;
  uint32_t sentinel;
  int64_t tbase;
  int8_t hot[SG_MAX_RET];
};

__global__ void __launch_bounds__(256) k_pp_rec(PpArgs a, SgCols bc, SgCols cc, const DevDesc* dd, RecArgs ra,
                                                uint32_t* __restrict__ okey, PpRec* __restrict__ orec,
                                                int32_t* __restrict__ err) {
  __shared__ SgCols colsl[2];
  __shared__ DevDesc dl;
  {
    const uint32_t* s1 = (const uint32_t*)&bc;
    const uint32_t* s2 = (const uint32_t*)&cc;
    for (uint32_t i = threadIdx.x; i < sizeof(SgCols) / 4; i += blockDim.x) {
      ((uint32_t*)&colsl[0])[i] = s1[i];
      ((uint32_t*)&colsl[1])[i] = s2[i];
    }
    const uint32_t* src = (const uint32_t*)dd;
    for (uint32_t i = threadIdx.x; i < sizeof(DevDesc) / 4; i += blockDim.x) ((uint32_t*)&dl)[i] = src[i];
    __syncthreads();
  }
  dd = &dl;
  // grid-stride: a few thousand blocks each stage the descriptors once and walk many rows
  const int64_t m_ = a.nc + a.n;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m_; i += (int64_t)gridDim.x * blockDim.x) {
    const bool carried = i < a.nc;
    const int64_t r = carried ? i : i - a.nc;
    uint32_t k = ra.sentinel;
    if (carried) {
      k = ra.partitioned ? (uint32_t)a.ckey[r] : 0u;
    } else {
      const int s = a.stream ? a.stream[r] : 0;
      if (s >= 0 && s < SG_MAX_STREAMS && dd->recv_of_stream[s] >= 0) {
        if (!ra.partitioned) k = 0;
        else {
          const int32_t kk = a.bkey ? a.bkey[r] : -1;
          if (kk >= 0) {
            if ((uint32_t)kk >= ra.sentinel) atomicOr(err, 2);
            else k = (uint32_t)kk;
          }
        }
      }
    }
    okey[i] = k;
    PpRec rec;
    rec.w[0] = (uint32_t)i;
    rec.w[1] = rec.w[2] = rec.w[3] = 0;
    if (k != ra.sentinel) {
      const SgCols& cols = colsl[carried ? 1 : 0];
      uint32_t lb = 0;
      for (int s = 0; s < dd->n_states; ++s) {
        const sg_state_desc& x = dd->states[s];
        if (!x.local || (ra.mode == 1 && s != ra.start)) continue;
        bool ok;
        if (x.prog_len <= 0) ok = true;
        else if (!carried && a.lbits[s]) ok = mask_bit(a.lbits[s], (uint64_t)r) != 0;
        else {
          RowReader rd{&cols, dd->ret_col, r};
          ok = sg_eval(dd->code + x.prog_off, x.prog_len, rd);
        }
        if (ok) lb |= 1u << s;
      }
      if (ra.mode == 1) {
        rec.w[0] |= ((lb >> ra.start) & (carried ? (uint32_t)a.cstart[r] : 1u) & 1u) << 31;
        const int64_t dt = (carried ? a.cts[r] : a.bts[r]) - ra.tbase;
        if (dt != (int64_t)(int32_t)dt) atomicOr(err, 4);
        rec.w[1] = (uint32_t)(int32_t)dt;
      } else {
        rec.w[1] = lb;
      }
      for (int q = 0; q < dd->n_ret; ++q) {
        const int hw = ra.hot[q];
        if (hw < 0) continue;
        const int64_t bits = sg_val_bits(sg_read_col(cols, dd->ret_col[q], dd->ret_type[q], r));
        if (hw == 2) { rec.w[2] = (uint32_t)bits; rec.w[3] = (uint32_t)((uint64_t)bits >> 32); }
        else rec.w[2 + hw] = (uint32_t)bits;
      }
    }
    orec[i] = rec;
  }
}

// sorted records -> the key-ordered SoA rows the lanes read (retained slots outside the record are gathered)
__global__ void __launch_bounds__(256) k_pp_unpack(PpArgs a, SgCols bc, SgCols cc, const DevDesc* dd, RecArgs ra,
                                                   const uint32_t* __restrict__ skey, const PpRec* __restrict__ srec,
                                                   PpPacked P, uint32_t* __restrict__ sid, uint32_t* __restrict__ flag) {
  __shared__ SgCols colsl[2];
  __shared__ DevDesc dl;
  {
    const uint32_t* s1 = (const uint32_t*)&bc;
    const uint32_t* s2 = (const uint32_t*)&cc;
    for (uint32_t i = threadIdx.x; i < sizeof(SgCols) / 4; i += blockDim.x) {
      ((uint32_t*)&colsl[0])[i] = s1[i];
      ((uint32_t*)&colsl[1])[i] = s2[i];
    }
    const uint32_t* src = (const uint32_t*)dd;
    for (uint32_t i = threadIdx.x; i < sizeof(DevDesc) / 4; i += blockDim.x) ((uint32_t*)&dl)[i] = src[i];
    __syncthreads();
  }
  dd = &dl;
  // grid-stride: a few thousand blocks each stage the descriptors once and walk many rows
  const int64_t m_ = a.nc + a.n;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < m_; q += (int64_t)gridDim.x * blockDim.x) {
    const PpRec rec = srec[q];
    const uint32_t c = rec.w[0] & 0x7FFFFFFFu;
    sid[q] = c;
    if (skey[q] == ra.sentinel) { flag[q] = 0; continue; }
    const bool carried = (int64_t)c < a.nc;
    const int64_t r = carried ? (int64_t)c : (int64_t)c - a.nc;
    if (ra.mode == 1) {
      const uint32_t f = rec.w[0] >> 31;
      P.ts[q] = ra.tbase + (int64_t)(int32_t)rec.w[1];
      P.lb[q] = f << ra.start;
      flag[q] = f;
    } else {
      P.lb[q] = rec.w[1];
      flag[q] = (rec.w[1] >> ra.start) & 1u;
    }
    const SgCols& cols = colsl[carried ? 1 : 0];
    for (int k = 0; k < dd->n_ret; ++k) {
      const int hw = ra.hot[k];
      if (!P.val[k]) continue;   // lazy slot
      int64_t bits;
      if (hw == 2) bits = (int64_t)(((uint64_t)rec.w[3] << 32) | rec.w[2]);
      else if (hw >= 0) bits = (int64_t)(int32_t)rec.w[2 + hw];
      else bits = sg_val_bits(sg_read_col(cols, dd->ret_col[k], dd->ret_type[k], r));
      if (P.wide[k]) ((int64_t*)P.val[k])[q] = bits;
      else ((int32_t*)P.val[k])[q] = (int32_t)bits;
    }
  }
}

// per-key bounds; check_order: kback[k] = 1 when the key's timestamps go back somewhere (carried rows included)
__global__ void k_pp_segments(int64_t m, PpArgs a, const uint32_t* __restrict__ skey, const uint32_t* __restrict__ sid,
                              const int64_t* __restrict__ qts, int check_order, uint32_t sentinel,
                              uint32_t* __restrict__ beg, uint32_t* __restrict__ end, uint8_t* __restrict__ kback) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= m) return;
  const uint32_t k = skey[p];
  if (k == sentinel) return;
  auto ts_at = [&](int64_t q) -> int64_t {
    if (qts) return qts[q];
    const int64_t c = sid[q];
    return c < a.nc ? a.cts[c] : a.bts[c - a.nc];
  };
  if (p == 0 || skey[p - 1] != k) beg[k] = (uint32_t)p;
  else if (check_order && ts_at(p - 1) > ts_at(p)) kback[k] = 1;
  if (p == m - 1 || skey[p + 1] != k) end[k] = (uint32_t)p + 1;
}

// pack: key-ordered rows (ts, retained values, nulls, event-local condition bits) and the start-row flags
__global__ void __launch_bounds__(256) k_pp_pack(PpArgs a, SgCols bc, SgCols cc, const DevDesc* dd,
                                                 uint32_t local_mask, int start, const uint32_t* __restrict__ skey,
                                                 const uint32_t* __restrict__ sid, uint32_t sentinel, PpPacked P,
                                                 uint32_t* __restrict__ flag) {
  __shared__ SgCols colsl[2];
  __shared__ DevDesc dl;
  {
    const uint32_t* s1 = (const uint32_t*)&bc;
    const uint32_t* s2 = (const uint32_t*)&cc;
    for (uint32_t i = threadIdx.x; i < sizeof(SgCols) / 4; i += blockDim.x) {
      ((uint32_t*)&colsl[0])[i] = s1[i];
      ((uint32_t*)&colsl[1])[i] = s2[i];
    }
    const uint32_t* src = (const uint32_t*)dd;
    for (uint32_t i = threadIdx.x; i < sizeof(DevDesc) / 4; i += blockDim.x) ((uint32_t*)&dl)[i] = src[i];
    __syncthreads();
  }
  dd = &dl;
  // grid-stride: a few thousand blocks each stage the descriptors once and walk many rows
  const int64_t m_ = a.nc + a.n;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < m_; q += (int64_t)gridDim.x * blockDim.x) {
    if (skey[q] == sentinel) { flag[q] = 0; continue; }
    const int64_t c = sid[q];
    const bool carried = c < a.nc;
    const int64_t r = carried ? c : c - a.nc;
    const SgCols& cols = colsl[carried ? 1 : 0];
    P.ts[q] = carried ? a.cts[r] : a.bts[r];
    uint32_t nm = 0;
    for (int k = 0; k < dd->n_ret; ++k) {
      const SgVal v = sg_read_col(cols, dd->ret_col[k], dd->ret_type[k], r);
      if (v.null) nm |= 1u << k;
      const int64_t bits = sg_val_bits(v);
      if (P.wide[k]) ((int64_t*)P.val[k])[q] = bits;
      else ((int32_t*)P.val[k])[q] = (int32_t)bits;
    }
    if (P.nul) P.nul[q] = nm;
    uint32_t lb = 0;
    for (int s = 0; s < dd->n_states; ++s) {
      if (!((local_mask >> s) & 1u)) continue;
      const sg_state_desc& x = dd->states[s];
      bool ok;
      if (x.prog_len <= 0) ok = true;
      else if (!carried && a.lbits[s]) ok = mask_bit(a.lbits[s], (uint64_t)r) != 0;
      else {
        RowReader rd{&cols, dd->ret_col, r};
        ok = sg_eval(dd->code + x.prog_off, x.prog_len, rd);
      }
      if (ok) lb |= 1u << s;
    }
    P.lb[q] = lb;
    flag[q] = (lb >> start) & (carried && a.cstart ? (uint32_t)a.cstart[r] : 1u) & 1u;
  }
}

struct PpCopyCols {
  const void* bsrc[SG_MAX_COLS];
  const uint8_t* bnul[SG_MAX_COLS];
  const void* csrc[SG_MAX_COLS];
  const uint8_t* cnul[SG_MAX_COLS];
  void* dst[SG_MAX_COLS];
  uint8_t* dnul[SG_MAX_COLS];
  int32_t bytes[SG_MAX_COLS];
  int32_t ncols;
};

__global__ void k_pp_carry(int64_t m, PpArgs a, const uint32_t* __restrict__ skey, const uint32_t* __restrict__ sid,
                           const uint32_t* __restrict__ keep, const uint32_t* __restrict__ pos, PpCopyCols cc,
                           int64_t* __restrict__ nts, int32_t* __restrict__ nkey, uint8_t* __restrict__ nstart) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= m || !keep[p]) return;
  const int64_t c = sid[p];
  const int64_t o = pos[p];
  const bool carried = c < a.nc;
  const int64_t r = carried ? c : c - a.nc;
  nts[o] = carried ? a.cts[r] : a.bts[r];
  nkey[o] = (int32_t)skey[p];
  nstart[o] = a.kstart ? a.kstart[p] : 0;
  for (int j = 0; j < cc.ncols; ++j) {
    if (!cc.dst[j]) continue;
    const void* s = carried ? cc.csrc[j] : cc.bsrc[j];
    const uint8_t* sn = carried ? cc.cnul[j] : cc.bnul[j];
    if (cc.bytes[j] == 8) ((int64_t*)cc.dst[j])[o] = ((const int64_t*)s)[r];
    else ((int32_t*)cc.dst[j])[o] = ((const int32_t*)s)[r];
    cc.dnul[j][o] = sn ? sn[r] : 0;
  }
}

// ---- host side ------------------------------------------------------------------------------------------------
static void rows_free(PpRows& r) {
  if (r.ts) hipFree(r.ts);
  if (r.key) hipFree(r.key);
  if (r.start) hipFree(r.start);
  for (int c = 0; c < SG_MAX_COLS; ++c) {
    if (r.col[c]) hipFree(r.col[c]);
    if (r.nul[c]) hipFree(r.nul[c]);
  }
  r = PpRows();
}

static void rows_reserve(PartialState* ps, PpRows& r, int64_t need) {
  if (need <= r.cap) return;
  const int64_t cap = std::max<int64_t>(need + need / 4, 1024);
  PpRows nr;
  nr.cap = cap;
  if (hipMalloc(&nr.ts, 8 * cap) != hipSuccess || hipMalloc(&nr.key, 4 * cap) != hipSuccess ||
      hipMalloc(&nr.start, cap) != hipSuccess)
    throw SgError(SG_EHIP, "hipMalloc carried rows");
  for (int c = 0; c < SG_MAX_COLS; ++c) {
    if (!ps->used_col[c]) continue;
    if (hipMalloc(&nr.col[c], (size_t)ps->col_bytes[c] * cap) != hipSuccess || hipMalloc(&nr.nul[c], cap) != hipSuccess)
      throw SgError(SG_EHIP, "hipMalloc carried rows");
  }
  rows_free(r);
  r = nr;
}

static SgCols carried_cols(const PartialState* ps, const PpRows& r) {
  SgCols c;
  for (int j = 0; j < SG_MAX_COLS; ++j) { c.col[j] = ps->used_col[j] ? r.col[j] : nullptr; c.nul[j] = ps->used_col[j] ? r.nul[j] : nullptr; }
  return c;
}

// The push's rows in key order: what the front end hands to either route's lanes.
struct PpOrdered {
  PpPacked P;
  uint32_t* skeys;            // per position: its key (the sentinel = the key bound for a row no receiver takes)
  uint32_t* sids;             // per position: its combined row
  uint32_t* beg;              // per key: its positions [beg, end)
  uint32_t* end;
  uint32_t* flag;             // per position: 1 = the row starts a partial
  uint8_t* kback;             // partial lanes: per key, its time goes back somewhere in this push
};

static void throw_if_key_out_of_bound(int32_t herr) {
  if (herr & 2) throw SgError(SG_EINVAL, "a partition key id is >= the batch's key_bound");
}

// Record sort: one 16-B record per row through the key sort, unpacked into the SoA rows (no batch-wide gather).
// Returns false, with nothing of `o` written, when a timestamp lies more than 2^31 ms from the push's first: the
// gather path carries full timestamps.
static bool order_by_records(SgHandle* h, PartialState* ps, const BatchView& bv, const PpArgs& a, const SgCols& cc,
                             uint32_t kb, int end_bit, uint32_t* keys, int32_t* err, PpOrdered& o) {
  const sg_nfa_desc& d = h->desc;
  hipStream_t st = h->stream;
  const int64_t m = a.nc + a.n;
  const dim3 blk(256), grd((unsigned)((m + 255) / 256));
  const dim3 grs((unsigned)std::max<int64_t>(1, std::min<int64_t>((m + 255) / 256, 4096)));
  RecArgs ra;
  memset(&ra, 0, sizeof(ra));
  ra.mode = ps->mode;
  ra.start = ps->rule.start;
  ra.partitioned = d.partitioned;
  ra.sentinel = kb;
  for (int k = 0; k < SG_MAX_RET; ++k) ra.hot[k] = ps->hot[k];
  ra.tbase = sg_read_back<int64_t>(a.n ? a.bts : a.cts, st);
  PpRec* recs = (PpRec*)h->ws.get("pp_recs", sizeof(PpRec) * m, st);
  PpRec* srecs = (PpRec*)h->ws.get("pp_srecs", sizeof(PpRec) * m, st);
  h->kbeg("route");
  hipLaunchKernelGGL(k_pp_rec, grs, blk, 0, st, a, bv.cols, cc, h->ddesc, ra, keys, recs, err);
  HIPCHK(hipGetLastError());
  h->kend();
  h->kbeg("key_sort");
  sg_radix_sort_pairs(h->ws, st, "pp_rsort_tmp", keys, o.skeys, recs, srecs, (size_t)m, end_bit);
  h->kend();
  const int32_t herr = sg_read_back(err, st);
  throw_if_key_out_of_bound(herr);
  if (herr & 4) {
    HIPCHK(hipMemsetAsync(err, 0, 8, st));
    return false;
  }
  // the lanes read only the record's hot slots (every slot a non-local filter reads); the others are read for
  // matches only, lazily at record build.  Sequence lanes read timestamps only for matches as well.
  if (ps->mode == 2) o.P.ts = nullptr;
  for (int k = 0; k < d.n_ret; ++k) if (ps->hot[k] < 0) o.P.val[k] = nullptr;
  h->kbeg("pack");
  hipLaunchKernelGGL(k_pp_unpack, grs, blk, 0, st, a, bv.cols, cc, h->ddesc, ra, o.skeys, srecs, o.P, o.sids, o.flag);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemsetAsync(o.beg, 0, 4 * (size_t)kb, st));
  HIPCHK(hipMemsetAsync(o.end, 0, 4 * (size_t)kb, st));
  hipLaunchKernelGGL(k_pp_segments, grd, blk, 0, st, m, a, o.skeys, o.sids, o.P.ts, ps->mode == 1 ? 1 : 0, kb, o.beg,
                     o.end, o.kback);
  HIPCHK(hipGetLastError());
  h->kend();
  return true;
}

// Gather path: sort (key, combined row), then read every row's fields through its row id.
static void order_by_gather(SgHandle* h, PartialState* ps, const BatchView& bv, const PpArgs& a, const SgCols& cc,
                            uint32_t kb, int end_bit, uint32_t* keys, int32_t* err, PpOrdered& o) {
  const sg_nfa_desc& d = h->desc;
  hipStream_t st = h->stream;
  const int64_t m = a.nc + a.n;
  const dim3 blk(256), grd((unsigned)((m + 255) / 256));
  const dim3 grs((unsigned)std::max<int64_t>(1, std::min<int64_t>((m + 255) / 256, 4096)));
  uint32_t* ids = (uint32_t*)h->ws.get("pp_ids", 4 * m, st);
  h->kbeg("route");
  hipLaunchKernelGGL(k_pp_route, grd, blk, 0, st, a, h->ddesc, d.partitioned, kb, keys, ids, err);
  HIPCHK(hipGetLastError());
  h->kend();
  h->kbeg("key_sort");
  sg_radix_sort_pairs(h->ws, st, "pp_sort_tmp", keys, o.skeys, ids, o.sids, (size_t)m, end_bit);
  HIPCHK(hipMemsetAsync(o.beg, 0, 4 * (size_t)kb, st));
  HIPCHK(hipMemsetAsync(o.end, 0, 4 * (size_t)kb, st));
  if (m) hipLaunchKernelGGL(k_pp_segments, grd, blk, 0, st, m, a, o.skeys, o.sids, (const int64_t*)nullptr,
                            ps->mode == 1 ? 1 : 0, kb, o.beg, o.end, o.kback);
  HIPCHK(hipGetLastError());
  h->kend();
  h->kbeg("pack");
  if (m) hipLaunchKernelGGL(k_pp_pack, grs, blk, 0, st, a, bv.cols, cc, h->ddesc, ps->rule.local_mask, ps->rule.start,
                            o.skeys, o.sids, kb, o.P, o.flag);
  HIPCHK(hipGetLastError());
  h->kend();
}

// Steps 1 and 2 of the push: the combined rows (carried, then the batch) in key order, each key's in arrival order,
// packed for the lanes; per-key bounds; for partial lanes the keys whose time goes back (a.kback: their lanes skip
// rows only while waiting in a count state).  The key bound doubles as the key of a row no receiver takes; err[0]
// (zeroed by the caller) takes the kernels' flags.
static PpOrdered key_ordered_rows(SgHandle* h, PartialState* ps, const BatchView& bv, PpArgs& a, uint32_t kb,
                                  int32_t* err) {
  const sg_nfa_desc& d = h->desc;
  hipStream_t st = h->stream;
  const PpRows& cr = ps->rows[ps->cur];
  const int64_t m = a.nc + a.n;
  const SgCols cc = carried_cols(ps, cr);
  int end_bit = 1;
  while ((1ull << end_bit) <= (uint64_t)kb) ++end_bit;
  uint32_t* keys = (uint32_t*)h->ws.get("pp_keys", 4 * m, st);
  bool batch_nul = false;
  for (int k = 0; k < d.n_ret; ++k) batch_nul |= bv.cols.nul[d.ret_col[k]] != nullptr;
  if (batch_nul) ps->nulls_seen = 1;
  const bool any_nul = batch_nul || (a.nc > 0 && ps->nulls_seen);
  PpOrdered o;
  memset(&o, 0, sizeof(o));
  o.skeys = (uint32_t*)h->ws.get("pp_skeys", 4 * m, st);
  o.sids = (uint32_t*)h->ws.get("pp_sids", 4 * m, st);
  PpPacked& P = o.P;
  P.ts = (int64_t*)h->ws.get("pp_qts", 8 * m, st);
  for (int k = 0; k < d.n_ret; ++k) {
    P.wide[k] = (d.ret_type[k] == SG_T_LONG || d.ret_type[k] == SG_T_DOUBLE) ? 1 : 0;
    P.val[k] = h->ws.get("pp_qv" + std::to_string(k), (P.wide[k] ? 8 : 4) * m, st);
  }
  P.nul = any_nul ? (uint32_t*)h->ws.get("pp_qnul", 4 * m, st) : nullptr;
  P.lb = (uint32_t*)h->ws.get("pp_qlb", 4 * m, st);
  P.sid = o.sids;
  P.nc = a.nc;
  P.bts = bv.ts;
  P.cts = cr.ts;
  for (int k = 0; k < d.n_ret; ++k) {
    P.bcol[k] = bv.cols.col[d.ret_col[k]];
    P.ccol[k] = cc.col[d.ret_col[k]];
  }
  o.flag = (uint32_t*)h->ws.get("pp_flag", 4 * (m + 1), st);
  o.beg = (uint32_t*)h->ws.get("pp_beg", 4 * (size_t)kb, st);
  o.end = (uint32_t*)h->ws.get("pp_end", 4 * (size_t)kb, st);
  if (ps->mode == 1) {
    o.kback = (uint8_t*)h->ws.get("pp_kback", (size_t)kb, st);
    HIPCHK(hipMemsetAsync(o.kback, 0, (size_t)kb, st));
    a.kback = o.kback;
  }
  const bool by_records = ps->rec_ok && !any_nul && m > 0;
  if (!by_records || !order_by_records(h, ps, bv, a, cc, kb, end_bit, keys, err, o))
    order_by_gather(h, ps, bv, a, cc, kb, end_bit, keys, err, o);
  throw_if_key_out_of_bound(sg_read_back(err, st));
  return o;
}

// The carry: the rows marked in `keep` (per position; one spare word behind them), in key order and each key's in
// arrival order, become the carried rows of the next push.
static void carry_rows(SgHandle* h, PartialState* ps, const BatchView& bv, const PpArgs& a, int64_t m,
                       const uint32_t* skeys, const uint32_t* sids, uint32_t* keep) {
  const sg_nfa_desc& d = h->desc;
  hipStream_t st = h->stream;
  const dim3 blk(256), grd((unsigned)((m + 255) / 256));
  const PpRows& cr = ps->rows[ps->cur];
  h->kbeg("carry");
  uint32_t* pos = (uint32_t*)h->ws.get("pp_pos", 4 * (m + 1), st);
  HIPCHK(hipMemsetAsync(keep + m, 0, 4, st));
  sg_exclusive_scan(h->ws, st, "pp_scan_tmp", keep, pos, (uint32_t)0, (size_t)m + 1, rocprim::plus<uint32_t>());
  uint32_t nn = sg_read_back(pos + m, st);
  PpRows& nr = ps->rows[1 - ps->cur];
  rows_reserve(ps, nr, nn);
  PpCopyCols c2;
  memset(&c2, 0, sizeof(c2));
  c2.ncols = d.n_cols;
  for (int j = 0; j < d.n_cols; ++j) {
    if (!ps->used_col[j]) continue;
    c2.bsrc[j] = bv.cols.col[j];
    c2.bnul[j] = bv.cols.nul[j];
    c2.csrc[j] = cr.col[j];
    c2.cnul[j] = cr.nul[j];
    c2.dst[j] = nr.col[j];
    c2.dnul[j] = nr.nul[j];
    c2.bytes[j] = ps->col_bytes[j];
  }
  hipLaunchKernelGGL(k_pp_carry, grd, blk, 0, st, m, a, skeys, sids, keep, pos, c2, nr.ts, nr.key, nr.start);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st));
  nr.n = nn;
  ps->rows[ps->cur].n = 0;
  ps->cur = 1 - ps->cur;
  h->kend();
}
