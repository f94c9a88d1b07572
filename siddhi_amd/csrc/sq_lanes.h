// sq_lanes.h -- sequence lanes (seq.h): one lane per key resumes the key's compact machine over its rows, cut into
// speculative (key, chunk) units.  Kernels first, then the host stages and their driver, seq_lanes_push, which
// sg_partial_push (partial.hip) hands the key-ordered rows of pp_rows.h.
#pragma once
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include <algorithm>
#include <cstdlib>
#include <string>

#include "seq.h"
#include "pp_emit.h"
#include "pp_rows.h"

struct SeqSrcD {
  const PpPacked* P;
  int64_t base;
  __device__ int64_t ts(int64_t pos) const { return P->ts ? P->ts[base + pos] : pp_lazy_ts(P, base + pos); }
  __device__ void read_bits(int64_t pos, int slotk, int type, int64_t& bits, int& null) const {
    const int64_t q = base + pos;
    null = P->nul ? (int)((P->nul[q] >> slotk) & 1u) : 0;
    if (!P->val[slotk]) { bits = pp_lazy_bits(P, q, slotk); return; }
    bits = P->wide[slotk] ? ((const int64_t*)P->val[slotk])[q] : (int64_t)((const int32_t*)P->val[slotk])[q];
  }
  __device__ SgVal read(int64_t pos, int slotk, int type) const {
    int64_t bits;
    int null;
    read_bits(pos, slotk, type, bits, null);
    return sg_val_from_bits(bits, type, null);
  }
  __device__ int lbit(int s, int64_t pos) const { return (int)((P->lb[base + pos] >> s) & 1u); }
};

struct SqOut {
  char* rec;
  uint64_t* k1;               // (trigger row << 16) | emission index within the row
  uint32_t* runit;            // unit that wrote the slot (| 0x80000000 when written by a rerun)
  uint32_t* rerun;            // per unit: 1 = its speculative matches are void
  unsigned long long* dropped;
  unsigned long long* reserved;
  unsigned long long* count;
  int32_t* fail;
  int64_t cap;
  int32_t rstride;
  uint64_t k1_none;
};

constexpr int SQ_BLOCK = 64;
constexpr int SQ_CHUNK = 16;   // match slots a lane reserves at a time

// Units (key, c): the key's new rows [s0, s1) = [beg + ncar + c R, ...).  Unit 0 starts from the key's carried state;
// unit c > 0 from a guess -- a zeroed state warmed up over the W rows before it -- verified afterwards.
struct SqPlan {
  const uint32_t* beg;
  const uint32_t* end;
  const uint32_t* ncar;       // carried rows at the start of each key's positions
  const uint32_t* uoff;       // key -> first unit
  const uint32_t* umap;       // unit -> key
  int64_t R, W;
  int64_t nunits;
  void* kst;                  // per key (carried), SeqStateT<G>: the states the push starts from (read only)
  void* kst_out;              // per key: the states the push ends in
  void* ust;                  // per unit: start state
  void* uen;                  // per unit: end state
  unsigned long long* reruns;
};

__global__ void k_sq_ucount(int64_t kb, const uint32_t* __restrict__ beg, const uint32_t* __restrict__ end,
                            const uint32_t* __restrict__ sid, int64_t nc, int64_t R, uint32_t* __restrict__ ncar,
                            uint32_t* __restrict__ nu) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k > kb) return;
  if (k == kb) { nu[k] = 0; return; }
  const int64_t b0 = beg[k], e0 = end[k];
  int64_t c = 0;
  while (b0 + c < e0 && (int64_t)sid[b0 + c] < nc) ++c;
  ncar[k] = (uint32_t)c;
  const int64_t own = e0 > b0 ? e0 - b0 - c : 0;
  nu[k] = (uint32_t)((own + R - 1) / R);
}

__global__ void k_sq_umap(int64_t kb, const uint32_t* __restrict__ uoff, uint32_t* __restrict__ umap) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= kb) return;
  for (uint32_t u = uoff[k]; u < uoff[k + 1]; ++u) umap[u] = (uint32_t)k;
}

template <class T>
__device__ __forceinline__ void sq_copy(T* __restrict__ dst, const T* __restrict__ src) {
  static_assert(sizeof(T) % 4 == 0, "state words");
  const uint32_t* s = (const uint32_t*)src;
  uint32_t* d = (uint32_t*)dst;
  for (uint32_t i = 0; i < sizeof(T) / 4; ++i) d[i] = s[i];
}
template <class T>
__device__ __forceinline__ void sq_zero(T* dst) {
  uint32_t* d = (uint32_t*)dst;
  for (uint32_t i = 0; i < sizeof(T) / 4; ++i) d[i] = 0;
}

struct SqEmit {   // match writer of the emitting pass (off: the warm-up, same code so the machine is inlined once)
  bool on;
  const PpArgs* a;
  const DevDesc* dd;
  const uint32_t* sid;
  SqOut o;
  int64_t slot, slot_end;
  uint32_t key, seq, nemit, unit;
  template <class Mach>
  __device__ void operator()(Mach& mm, int p, int grp) {
    if (!on) return;
    if (slot == slot_end) {
      slot = (int64_t)atomicAdd(o.reserved, (unsigned long long)SQ_CHUNK);
      slot_end = slot + SQ_CHUNK;
      if (slot_end > o.cap) { mm.fail(5); slot = slot_end; return; }
    }
    const int64_t w = slot++;
    ++nemit;
    const int64_t q = mm.src.base + mm.cur;   // the trigger row's sorted position; its batch row through sid
    const int64_t r = (int64_t)sid[q] - a->nc;
    o.k1[w] = ((uint64_t)r << 16) | seq++;
    o.runit[w] = unit;
    // positions only: k_em_scatter turns them into the match record, in slot order, once the delivery order is known (one thread
    // per match instead of dependent reads in the lane's critical path)
    uint32_t* em32 = (uint32_t*)(o.rec + (size_t)w * (size_t)o.rstride);
    const int64_t pp = mm.dec(mm.M->P[p].pts);
    em32[0] = (uint32_t)q;
    em32[1] = (uint32_t)(r + a->nc);
    em32[2] = key;
    em32[3] = (1u << 24) | (uint32_t)grp;
    em32[4] = (uint32_t)(pp >= 0 ? mm.src.base + pp : -1);
    for (int s = 0; s < dd->n_select; ++s) {
      const int64_t ev = mm.get_event(p, dd->sel_state[s], dd->sel_index[s]);
      em32[5 + s] = (uint32_t)(ev < 0 ? -1 : mm.src.base + ev);
    }
  }
};

// rows [q0, q1) of a key whose positions start at b0; emit != null: the emitting pass
template <class E, class Mach>
__device__ __forceinline__ void sq_run(Mach& m, int64_t b0, int64_t q0, int64_t q1, E& emit, uint32_t* seq) {
  m.begin();
  for (int64_t q = q0; q < q1 && !m.failed; ++q) {
    if (seq) *seq = 0;
    m.receive(q - b0, emit);
  }
  m.finish();
}

// The descriptor stays in global memory (L1-resident: every lane reads the same few hundred bytes of it); LDS holds
// the lanes' machine states, so more waves fit per CU.
#define SQ_KERNEL_PROLOGUE                                                                                     \
  const DevDesc& dl = *ddg;                                                                                    \
  __shared__ SgSeqRule rl;                                                                                     \
  __shared__ PpPacked pl;                                                                                      \
  __shared__ SeqStateT<G> lanes[SQ_BLOCK];                                                                         \
  {                                                                                                            \
    const uint32_t* s3 = (const uint32_t*)&P;                                                                  \
    for (uint32_t i = threadIdx.x; i < sizeof(PpPacked) / 4; i += blockDim.x) ((uint32_t*)&pl)[i] = s3[i];    \
    const uint32_t* rs = (const uint32_t*)rug;                                                                 \
    for (uint32_t i = threadIdx.x; i < sizeof(SgSeqRule) / 4; i += blockDim.x) ((uint32_t*)&rl)[i] = rs[i];   \
    __syncthreads();                                                                                           \
  }

// pass A: every unit from its (guessed) start state, emitting; its start and end states are kept for the check
template <class G, bool FAST = false, class SH = SqShapeAny>
__global__ void __launch_bounds__(SQ_BLOCK) k_sq_spec(PpArgs a, PpPacked P, const DevDesc* __restrict__ ddg,
                                                      const SgSeqRule* __restrict__ rug, const uint32_t* __restrict__ sid,
                                                      SqPlan pl_, SqOut o) {
  SQ_KERNEL_PROLOGUE
  const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= pl_.nunits) return;
  const uint32_t k = pl_.umap[u];
  const int64_t c = u - pl_.uoff[k];
  const int64_t b0 = pl_.beg[k], e0 = pl_.end[k];
  const int64_t s0 = b0 + pl_.ncar[k] + c * pl_.R, s1 = s0 + pl_.R < e0 ? s0 + pl_.R : e0;
  SeqStateT<G>& M = lanes[threadIdx.x];
  SeqMachine<SeqSrcD, G, FAST, SH> m;
  m.d = &dl;
  m.ru = &rl;
  m.src = SeqSrcD{&pl, b0};
  m.M = &M;
  m.cur = 0;
  int64_t q0 = s0;
  if (c == 0) {
    sq_copy(&M, (const SeqStateT<G>*)pl_.kst + k);
  } else {
    sq_zero(&M);
    q0 = s0 - pl_.W > b0 ? s0 - pl_.W : b0;
  }
  SqEmit em;
  em.on = false;
  em.a = &a;
  em.dd = &dl;
  em.sid = sid;
  em.o = o;
  em.slot = em.slot_end = 0;
  em.key = k;
  em.nemit = 0;
  em.seq = 0;
  em.unit = (uint32_t)u;
  // one loop over the warm-up rows [q0, s0) (emitter off) and the unit's rows [s0, s1): one inlined machine
  bool started = false;
  m.begin();
  for (int64_t q = q0; q < s1 && !m.failed; ++q) {
    if (q == s0) {
      m.finish();
      sq_copy((SeqStateT<G>*)pl_.ust + u, &M);
      started = true;
      em.on = true;
    }
    em.seq = 0;
    m.receive(q - b0, em);
  }
  m.finish();
  if (!started) sq_copy((SeqStateT<G>*)pl_.ust + u, &M);   // (a warm-up that failed: the push is rerun elsewhere)
  for (int64_t q = em.slot; q < em.slot_end && q < o.cap; ++q) o.k1[q] = o.k1_none;
  if (em.nemit) atomicAdd(o.count, (unsigned long long)em.nemit);
  if (m.failed) atomicCAS(o.fail, 0, m.failed);
  sq_copy((SeqStateT<G>*)pl_.uen + u, &M);
}

// pass B: per key, in unit order, a unit whose guessed start differs from its predecessor's end is rerun from that end
// (emitting again; its speculative matches are voided); then the key's final state is kept for the next push
template <class G>
__global__ void __launch_bounds__(SQ_BLOCK) k_sq_fix(PpArgs a, PpPacked P, const DevDesc* __restrict__ ddg,
                                                     const SgSeqRule* __restrict__ rug, const uint32_t* __restrict__ sid,
                                                     SqPlan pl_, int64_t kb, SqOut o) {
  SQ_KERNEL_PROLOGUE
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= kb) return;
  const uint32_t u0 = pl_.uoff[k], u1 = pl_.uoff[k + 1];
  if (u1 == u0) {   // no rows this push: the key's state carries over unchanged
    sq_copy((SeqStateT<G>*)pl_.kst_out + k, (const SeqStateT<G>*)pl_.kst + k);
    return;
  }
  const int64_t b0 = pl_.beg[k], e0 = pl_.end[k];
  SeqStateT<G>& M = lanes[threadIdx.x];
  SeqMachine<SeqSrcD, G> m;
  m.d = &dl;
  m.ru = &rl;
  m.src = SeqSrcD{&pl, b0};
  m.M = &M;
  m.cur = 0;
  SqEmit em;
  em.a = &a;
  em.dd = &dl;
  em.sid = sid;
  em.o = o;
  em.slot = em.slot_end = 0;
  em.key = (uint32_t)k;
  em.nemit = 0;
  em.seq = 0;
  em.on = true;
  uint32_t reruns = 0;
  for (uint32_t u = u0 + 1; u < u1; ++u) {
    if (sg_seq_equiv(((const SeqStateT<G>*)pl_.ust)[u], ((const SeqStateT<G>*)pl_.uen)[u - 1], dl, rl)) continue;
    ++reruns;
    o.rerun[u] = 1;
    em.unit = u | 0x80000000u;
    const int64_t c = u - u0;
    const int64_t s0 = b0 + pl_.ncar[k] + c * pl_.R, s1 = s0 + pl_.R < e0 ? s0 + pl_.R : e0;
    sq_copy(&M, (const SeqStateT<G>*)pl_.uen + (u - 1));
    sq_run(m, b0, s0, s1, em, &em.seq);
    if (m.failed) { atomicCAS(o.fail, 0, m.failed); return; }
    sq_copy((SeqStateT<G>*)pl_.uen + u, &M);
  }
  for (int64_t q = em.slot; q < em.slot_end && q < o.cap; ++q) o.k1[q] = o.k1_none;
  if (em.nemit) atomicAdd(o.count, (unsigned long long)em.nemit);
  if (reruns) atomicAdd(pl_.reruns, (unsigned long long)reruns);
  sq_copy(&M, (const SeqStateT<G>*)pl_.uen + (u1 - 1));
  const int64_t nk = e0 - b0;
  m.rebase(nk - 1, nk > rl.horizon ? nk - rl.horizon : 0);
  sq_copy((SeqStateT<G>*)pl_.kst_out + k, &M);
}

// void the speculative matches of rerun units
__global__ void k_sq_drop(int64_t n, SqOut o) {
  const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= n || o.k1[w] == o.k1_none) return;
  const uint32_t u = o.runit[w];
  if (!(u & 0x80000000u) && o.rerun[u]) {
    o.k1[w] = o.k1_none;
    atomicAdd(o.dropped, 1ull);
  }
}

// carry for sequence lanes: the last H rows of every key
__global__ void k_seq_keep(int64_t m, const uint32_t* __restrict__ skey, const uint32_t* __restrict__ end, uint32_t sentinel,
                           int64_t H, uint32_t* __restrict__ keep) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= m) return;
  const uint32_t k = skey[p];
  keep[p] = (k != sentinel && p >= (int64_t)end[k] - H) ? 1u : 0u;
}

// ---- host side ------------------------------------------------------------------------------------------------
// per-key machine states (grown with the key bound; new keys start zeroed = no runtime yet)
static void seq_grow_states(SgHandle* h, PartialState* ps, uint32_t kb) {
  hipStream_t st = h->stream;
  if ((int64_t)kb <= ps->kst_keys && ps->kst_out) return;
  const int64_t nk = std::max<int64_t>((int64_t)kb, ps->kst_keys * 3 / 2);
  void* ns = nullptr;
  void* no = nullptr;
  if (hipMalloc(&ns, ps->sq_bytes * (size_t)nk) != hipSuccess || hipMalloc(&no, ps->sq_bytes * (size_t)nk) != hipSuccess) {
    if (ns) hipFree(ns);
    throw SgError(SG_ECAPACITY, "hipMalloc sequence states");
  }
  HIPCHK(hipMemsetAsync(ns, 0, ps->sq_bytes * (size_t)nk, st));
  HIPCHK(hipMemsetAsync(no, 0, ps->sq_bytes * (size_t)nk, st));
  if (ps->kst) {
    HIPCHK(hipMemcpyAsync(ns, ps->kst, ps->sq_bytes * (size_t)ps->kst_keys, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    hipFree(ps->kst);
  }
  if (ps->kst_out) hipFree(ps->kst_out);
  ps->kst = ns;
  ps->kst_out = no;
  ps->kst_keys = nk;
}

// the push's counters {reserved, count, fail, reruns, dropped}, zeroed; the match space comes with each attempt
static SqOut seq_output(SgHandle* h, const K1Layout& k1) {
  hipStream_t st = h->stream;
  SqOut o;
  o.reserved = (unsigned long long*)h->ws.get("sq_cnt", 64, st);
  o.count = o.reserved + 1;
  o.fail = (int32_t*)(o.reserved + 2);
  o.dropped = o.reserved + 4;
  o.cap = 0;
  o.rstride = em_compact_stride(h->desc.n_select);
  o.k1_none = k1.none;
  HIPCHK(hipMemsetAsync(o.reserved, 0, 64, st));
  return o;
}

// unit plan: every key's new rows cut into units of R rows, each warmed up over the W rows before it
static SqPlan seq_unit_plan(SgHandle* h, PartialState* ps, int64_t n, uint32_t kb, const PpArgs& a, const PpOrdered& r,
                            const SqOut& o) {
  hipStream_t st = h->stream;
  const dim3 blk(256);
  SqPlan pl_;
  pl_.R = std::max<int64_t>(64, (n + 262143) / 262144);
  if (h->opt.chunk_rows > 0) pl_.R = h->opt.chunk_rows;
  pl_.W = std::max<int64_t>(4 * (int64_t)ps->srule.horizon, 16);
  uint32_t* ncar = (uint32_t*)h->ws.get("sq_ncar", 4 * ((size_t)kb + 1), st);
  uint32_t* nu = (uint32_t*)h->ws.get("sq_nu", 4 * ((size_t)kb + 1), st);
  uint32_t* uoff = (uint32_t*)h->ws.get("sq_uoff", 4 * ((size_t)kb + 1), st);
  h->kbeg("sequence_units");
  hipLaunchKernelGGL(k_sq_ucount, dim3((unsigned)((kb + 1 + 255) / 256)), blk, 0, st, (int64_t)kb, r.beg, r.end, r.sids,
                     a.nc, pl_.R, ncar, nu);
  sg_exclusive_scan(h->ws, st, "sq_uscan_tmp", nu, uoff, (uint32_t)0, (size_t)kb + 1, rocprim::plus<uint32_t>());
  const uint32_t U = sg_read_back(uoff + kb, st);
  uint32_t* umap = (uint32_t*)h->ws.get("sq_umap", 4 * ((size_t)U + 1), st);
  hipLaunchKernelGGL(k_sq_umap, dim3((unsigned)((kb + 255) / 256)), blk, 0, st, (int64_t)kb, uoff, umap);
  pl_.beg = r.beg;
  pl_.end = r.end;
  pl_.ncar = ncar;
  pl_.uoff = uoff;
  pl_.umap = umap;
  pl_.nunits = U;
  pl_.kst = ps->kst;
  pl_.kst_out = ps->kst_out;
  pl_.ust = h->ws.get("sq_ust", ps->sq_bytes * ((size_t)U + 1), st);
  pl_.uen = h->ws.get("sq_uen", ps->sq_bytes * ((size_t)U + 1), st);
  pl_.reruns = o.reserved + 3;
  h->kend();
  return pl_;
}

// match space: every lane reserves SQ_CHUNK slots at a time; a push whose matches outgrow it is rerun from the
// unchanged start states (kst) with four times the space -- the reference's lists are unbounded
static int64_t seq_match_space(const PartialState* ps, int64_t n, int64_t U, uint32_t kb) {
  int64_t cap = n + (int64_t)SQ_CHUNK * (U + (int64_t)kb) + 65536;
  if (ps->sq_cap_hint > cap) cap = ps->sq_cap_hint;
  if (const char* e = getenv("SG_DEBUG_SQ_MATCH_CAP")) {   // (debug: a tiny match space exercises the regrowth)
    const int64_t v = atoll(e);
    if (v > 0) cap = std::max<int64_t>(v, SQ_CHUNK);
  }
  return cap;
}

// the speculative pass's kernel variant
static const void* seq_spec_fn(const PartialState* ps) {
  return ps->sq_small && ps->lanes_fast && ps->shape_c3b ? (const void*)k_sq_spec<SqSmall, true, SqShapeC3b>
         : ps->sq_small && ps->lanes_fast                ? (const void*)k_sq_spec<SqSmall, true>
         : ps->sq_small                                  ? (const void*)k_sq_spec<SqSmall>
                                                         : (const void*)k_sq_spec<SqBig>;
}

// One attempt with `cap` match slots: the speculative pass over every unit, the fix pass per key, and the counters
// read back into cnt[0..4].  Returns the failure code (5: out of match space; ps->kst is unchanged, so the push can
// be run again).
static int32_t seq_attempt(SgHandle* h, PartialState* ps, const PpArgs& a, const PpOrdered& r, SqPlan pl_, SqOut& o,
                           int64_t cap, int attempt, uint32_t kb, unsigned long long* cnt) {
  hipStream_t st = h->stream;
  const int32_t rstride = 32 + 8 * h->desc.n_select;
  const size_t U = (size_t)pl_.nunits;
  const dim3 gu((unsigned)((U + SQ_BLOCK - 1) / SQ_BLOCK)), gq((unsigned)((kb + SQ_BLOCK - 1) / SQ_BLOCK));
  const uint32_t* sids = r.sids;
  o.cap = cap;
  o.rec = (char*)h->ws.get("sq_rec", (size_t)cap * rstride, st);
  o.k1 = (uint64_t*)h->ws.get("sq_k1", 8 * cap, st);
  o.runit = (uint32_t*)h->ws.get("sq_runit", 4 * (size_t)cap, st);
  o.rerun = (uint32_t*)h->ws.get("sq_rerun", 4 * (U + 1), st);
  HIPCHK(hipMemsetAsync(o.rerun, 0, 4 * (U + 1), st));
  if (attempt) HIPCHK(hipMemsetAsync(o.reserved, 0, 64, st));
  h->kbeg("sequence_lanes");
  if (U) {
    const DevDesc* dd_ = h->ddesc;
    const SgSeqRule* ru_ = ps->dsrule;
    PpArgs a_ = a;
    PpPacked P_ = r.P;
    void* args[] = {&a_, &P_, &dd_, &ru_, &sids, &pl_, &o};
    HIPCHK(hipLaunchKernel(seq_spec_fn(ps), gu, dim3(SQ_BLOCK), args, 0, st));
  }
  HIPCHK(hipGetLastError());
  h->kend();
  h->kbeg("sequence_fix");
  if (U && ps->sq_small) hipLaunchKernelGGL(k_sq_fix<SqSmall>, gq, dim3(SQ_BLOCK), 0, st, a, r.P, h->ddesc, ps->dsrule, sids, pl_, (int64_t)kb, o);
  else if (U) hipLaunchKernelGGL(k_sq_fix<SqBig>, gq, dim3(SQ_BLOCK), 0, st, a, r.P, h->ddesc, ps->dsrule, sids, pl_, (int64_t)kb, o);
  HIPCHK(hipGetLastError());
  h->kend();
  // keys past this push's key bound keep their states as well
  if (ps->kst_keys > (int64_t)kb)
    HIPCHK(hipMemcpyAsync((char*)ps->kst_out + ps->sq_bytes * (size_t)kb, (const char*)ps->kst + ps->sq_bytes * (size_t)kb,
                          ps->sq_bytes * (size_t)(ps->kst_keys - (int64_t)kb), hipMemcpyDeviceToDevice, st));
  HIPCHK(hipMemcpyAsync(cnt, o.reserved, 40, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return (int32_t)(cnt[2] & 0xffffffffu);
}

// some units were rerun: void their speculative matches among the `slots` written; returns how many were dropped
static unsigned long long seq_drop_reruns(SgHandle* h, const SqOut& o, int64_t slots) {
  hipStream_t st = h->stream;
  unsigned long long dropped = 0;
  hipLaunchKernelGGL(k_sq_drop, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, st, slots, o);
  HIPCHK(hipMemcpyAsync(&dropped, o.dropped, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return dropped;
}

// delivery order: one stable sort of the slots by (trigger row, emission index); voided and unused slots sort behind
static void seq_order_and_emit(SgHandle* h, const BatchView& bv, const PpPacked& P, const SqOut& o, const K1Layout& k1,
                               int64_t slots, int64_t total) {
  hipStream_t st = h->stream;
  uint32_t* ia = (uint32_t*)h->ws.get("sq_ia", 4 * slots, st);
  uint32_t* ib = (uint32_t*)h->ws.get("sq_ib", 4 * slots, st);
  uint64_t* kb2 = (uint64_t*)h->ws.get("sq_kb", 8 * slots, st);
  h->kbeg("match_order");
  hipLaunchKernelGGL(k_pp_iota, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, st, slots, ia);
  sg_radix_sort_pairs(h->ws, st, "sq_sorttmp", o.k1, kb2, ia, ib, (size_t)slots, k1.bits);
  emit_in_order(h, bv, P, "sq_dest", slots, total, ib, o.rec);
  h->kend();
}

// Returns 1 when the push ran on sequence lanes, 0 when the sequence machine ran out of capacity on a first push with
// nothing carried (the states are zeroed again: the per-key machine can take the stream exactly).
static int seq_lanes_push(SgHandle* h, PartialState* ps, const BatchView& bv, int64_t n, uint32_t kb, const PpArgs& a,
                          const PpOrdered& r) {
  hipStream_t st = h->stream;
  const int64_t m = a.nc + a.n;
  seq_grow_states(h, ps, kb);
  const K1Layout k1 = k1_layout(n, 16);
  SqOut o = seq_output(h, k1);
  const SqPlan pl_ = seq_unit_plan(h, ps, n, kb, a, r, o);
  int64_t cap = seq_match_space(ps, n, pl_.nunits, kb);
  unsigned long long cnt[5] = {0, 0, 0, 0, 0};   // {reserved, count, fail, reruns, dropped}
  int32_t fail = 0;
  for (int attempt = 0;; ++attempt) {
    fail = seq_attempt(h, ps, a, r, pl_, o, cap, attempt, kb, cnt);
    if (fail != 5) break;
    cap = std::max<int64_t>(4 * cap, (int64_t)std::min<unsigned long long>(cnt[0], (1ull << 40)) + cap);
    ps->sq_cap_hint = cap;
  }
  const int64_t slots = std::min<int64_t>((int64_t)cnt[0], cap);
  if (cnt[3]) cnt[4] = seq_drop_reruns(h, o, slots);
  h->mark(3);
  ps->last_reruns = (int64_t)cnt[3];
  if (fail) {
    if (ps->seq_pushes == 0 && a.nc == 0) {   // nothing carried yet: the per-key machine can take the stream exactly
      HIPCHK(hipMemsetAsync(ps->kst, 0, ps->sq_bytes * (size_t)ps->kst_keys, st));
      return 0;
    }
    throw SgError(SG_ECAPACITY, "sequence machine capacity exceeded (reason " + std::to_string(fail) +
                                    ": 1 partials, 2 list, 3 returned, 4 chain)");
  }
  std::swap(ps->kst, ps->kst_out);   // the push's end states become the carried states
  const int64_t total = (int64_t)(cnt[1] - cnt[4]);
  if (total) seq_order_and_emit(h, bv, r.P, o, k1, slots, total);
  if (!h->opt.no_carry && m) {
    uint32_t* keep = (uint32_t*)h->ws.get("pp_keep", 4 * (m + 1), st);
    hipLaunchKernelGGL(k_seq_keep, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, m, r.skeys, r.end, kb,
                       (int64_t)ps->srule.horizon, keep);
    carry_rows(h, ps, bv, a, m, r.skeys, r.sids, keep);
  } else if (h->opt.no_carry) {
    HIPCHK(hipMemsetAsync(ps->kst, 0, ps->sq_bytes * (size_t)ps->kst_keys, st));
  }
  ps->seq_pushes++;
  h->mark(4);
  h->last_events = n;
  h->last_spilled = 0;
  h->last_matches = total;
  return 1;
}
