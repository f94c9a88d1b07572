// pp_lanes.h -- partial lanes (chain.h PpLane) over the key-ordered rows of pp_rows.h: one lane per row that starts a
// partial.  Kernels first, then the host stages sg_partial_push (partial.hip) runs in this order: start_rows,
// lane_output, carry_marks, wait_summaries, run_lanes, read_lane_counts, delivery_order.
#pragma once
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include <algorithm>
#include <string>

#include "chain.h"
#include "pp_emit.h"
#include "pp_rows.h"

struct PpOut {
  char* rec;                  // match records (sg_match_records layout, 32 + 8 * n_select bytes)
  uint64_t* k1;               // (trigger row << 8) | visit slot
  uint64_t* th;               // tie words
  uint64_t* tl;
  unsigned long long* count;
  int32_t* fail;
  uint32_t* jp;               // sorted position of the trigger row
  uint32_t* maxoff;           // largest (trigger position - start position) of a match
  int32_t rstride;
  uint64_t k1_none;           // k1 of a start row without a match (above every (row << 8 | slot) of this push)
};

__global__ void k_pp_compact(int64_t m, const uint32_t* __restrict__ flag, const uint32_t* __restrict__ pos,
                             uint32_t* __restrict__ cand) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q < m && flag[q]) cand[pos[q]] = (uint32_t)q;
}

// Block summaries of the wait attributes (chain.h pp_wenc): one thread per 8 key-ordered rows and attribute.
__global__ void k_pp_wsum(int64_t m, PpPacked P, uint32_t slots, uint32_t fslots, uint2* __restrict__ out) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= P.wnb) return;
  const int64_t q0 = b * 8;
  const int nr = (int)(m - q0 < 8 ? m - q0 : 8);
  for (int k = 0; k < SG_MAX_RET; ++k) {
    if (!((slots >> k) & 1u)) continue;
    const int fast = ((fslots >> k) & 1u) ? 2 : 1;
    const uint32_t* v = (const uint32_t*)P.val[k] + q0;
    uint32_t mn = 0xffffffffu, mx = 0;
    if (nr == 8) {
      const uint4 a = *(const uint4*)v, c = *(const uint4*)(v + 4);
      const uint32_t x[8] = {a.x, a.y, a.z, a.w, c.x, c.y, c.z, c.w};
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        if (pp_wnan(x[i], fast)) continue;
        const uint32_t e = pp_wenc(x[i], fast);
        mn = e < mn ? e : mn;
        mx = e > mx ? e : mx;
      }
    } else {
      for (int i = 0; i < nr; ++i) {
        if (pp_wnan(v[i], fast)) continue;
        const uint32_t e = pp_wenc(v[i], fast);
        mn = e < mn ? e : mn;
        mx = e > mx ? e : mx;
      }
    }
    out[(int64_t)P.wix[k] * P.wnb + b] = make_uint2(mn, mx);
  }
}

constexpr int PP_BLOCK = 256;
constexpr int64_t PP_WAVE_CANDS = 512;    // start rows per wave (C3c sweep 128..8192: 512 and below 20.4-20.5 ms, 2048 21.5, 8192 26.0; profiles/r04/lanes_ab.log)
template <class G, bool FAST = false, class SH = PpShapeAny>
__global__ void __launch_bounds__(PP_BLOCK, G::S <= 4 ? 8 : 4) k_pp_lanes(PpArgs a, PpPacked P, const DevDesc* __restrict__ ddg,
                                                       const SgPpRule* __restrict__ rug, const uint32_t* __restrict__ cand,
                                                       int64_t ncand, const uint32_t* __restrict__ skey,
                                                       const uint32_t* __restrict__ sid, const uint32_t* __restrict__ end,
                                                       PpOut o, int64_t wave_cands) {
  // the descriptor (9.6 KB) stays in global memory (cache-resident: every lane reads the same few hundred bytes of
  // it), so LDS holds more lanes
  __shared__ SgPpRule rl;
  __shared__ PpPacked pl;
  __shared__ PpArraysT<G> lanes[PP_BLOCK];
  {
    const uint32_t* s3 = (const uint32_t*)&P;
    for (uint32_t i = threadIdx.x; i < sizeof(PpPacked) / 4; i += blockDim.x) ((uint32_t*)&pl)[i] = s3[i];
    const uint32_t* rs = (const uint32_t*)rug;
    uint32_t* rd = (uint32_t*)&rl;
    for (uint32_t i = threadIdx.x; i < sizeof(SgPpRule) / 4; i += blockDim.x) rd[i] = rs[i];
    __syncthreads();
  }
  const DevDesc* dd = ddg;
  // each wave owns PP_WAVE_CANDS consecutive start rows; a lane whose partial is finished takes the next one, so the
  // wave never waits on its longest partial (ballot + popcount hand-out, no atomics)
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t lo = wave * wave_cands;
  const int64_t hi = lo + wave_cands < ncand ? lo + wave_cands : ncand;
  if (lo >= ncand) return;
  PpSrc src{&pl};
  PpLane<PpSrc, G, FAST, SH> L;
  L.d = dd;
  L.ru = &rl;
  L.src = src;
  L.A = &lanes[threadIdx.x];
  const int64_t within = dd->within;
  int64_t nxt = lo + 64;   // wave-uniform
  int64_t i = lo + lane;
  bool active = i < hi;
  int64_t q = 0, e = 0, p0 = 0;
  uint32_t k = 0;
  bool back = false;   // the key's time goes back in this push: skip rows only while waiting in a count state
  if (active) {
    const int64_t p = cand[i];
    k = skey[p];
    L.start(p);
    q = p + 1;
    p0 = p;
    e = end[k];
    back = a.kback && a.kback[k];
  }
  const uint64_t lt = (1ull << lane) - 1ull;
  bool emitted = false;
  uint32_t nemit = 0, maxoff = 0;
  while (__ballot(active)) {
    bool done = false;
    if (active) {
      // wait skipping: the 8-row blocks in which no row can pass the partial's wait term change nothing
      // (PpLane::wait_on); at most 16 blocks per step, the row landed on is checked for expiry below (a key whose time
      // goes back skips only while the partial waits in a count state, which nothing expires)
      int ws, wop, wf;
      int64_t wc;
      if (pl.wsum && q < e && L.wait_on(ws, wop, wf, wc) && (L.wait_count || !back)) {
        // blocks whose summary rules the term out are skipped whole; in a block that may pass, the lane reads its 8
        // values at once and lands on the first row that passes (or moves on to the next block)
        const uint2* S = pl.wsum + (int64_t)pl.wix[ws] * pl.wnb;
        const uint32_t* V = (const uint32_t*)pl.val[ws];
        const int64_t mrows = a.nc + a.n;
        int64_t qq = q;
        for (int lim = 0; lim < 16 && qq < e; ++lim) {
          const int64_t b = qq >> 3;
          const uint2 mm = S[b];
          if (pp_may_pass(mm.x, mm.y, wop, wf, wc)) {
            uint32_t x[8];
            if ((b << 3) + 8 <= mrows) {
              const uint4 x0 = *(const uint4*)(V + (b << 3)), x1 = *(const uint4*)(V + (b << 3) + 4);
              x[0] = x0.x; x[1] = x0.y; x[2] = x0.z; x[3] = x0.w; x[4] = x1.x; x[5] = x1.y; x[6] = x1.z; x[7] = x1.w;
            } else {
#pragma unroll
              for (int k = 0; k < 8; ++k) x[k] = (b << 3) + k < mrows ? V[(b << 3) + k] : 0u;
            }
            uint32_t pm = 0;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
              const bool ok = wf == 1 ? pp_cmp_i(wop, (int64_t)(int32_t)x[k], wc) : pp_cmp_f(wop, pp_f32((int64_t)x[k]), pp_f32(wc));
              pm |= (ok ? 1u : 0u) << k;
            }
            pm &= ~((1u << (qq & 7)) - 1u);
            if (pm) {
              qq = (b << 3) + __builtin_ctz(pm);
              break;
            }
          }
          qq = (b + 1) << 3;
        }
        q = qq < e ? qq : e;
      }
      const int64_t sdt = q < e ? src.ts(q) - L.e1_ts : 0;
      const int64_t dt = sdt < 0 ? -sdt : sdt;
      if (q < e && sdt > a.dead_after) {
        // bounded lateness: the clock is at least this row's time, so no later row can lie inside `within` of e1 --
        // the partial never emits again, in this push or a later one (not carried)
        done = true;
      } else if (q >= e) {
        done = true;
        // still pending after the key's last row (and not finished: a partial completes at most once): the rows it
        // holds are carried, its e1 marked as the start of its lane in the next push
        if (a.keep && !emitted && !L.overflow && !L.dead() && (L.waiting_count() || L.live_other()) &&
            L.e1_ts >= a.drop_before)
          L.witnesses([&](int32_t pos, bool st) {
            atomicOr(&a.keep[pos], 1u);
            if (st) a.kstart[pos] = 1;
          });
      } else if (dt > within && (!(a.keep || back) || !L.waiting_count())) {
        // expired everywhere it can still emit (sg_pp_rule).  A partial waiting in a count state never expires
        // (CountPreStateProcessor.java:53-93) and walks on -- but only a later row back inside `within` of e1 could
        // complete it: with no push after this one (no carry) and a key whose time never goes back here, none can
        done = true;
      } else {
        const int em = L.step(q);
        if (L.overflow) atomicCAS(o.fail, 0, SG_EUNSUPPORTED);
        if (em >= 0) {
          const int64_t c = sid[q];
          if (c >= a.nc) {
            // a partial completes at most once (sg_pp_rule): its match record goes to its start row's slot
            const int64_t w = i;
            emitted = true;
            const int64_t r = c - a.nc;
            o.k1[w] = ((uint64_t)r << 8) | (uint32_t)em;
            L.tie(o.th[w], o.tl[w]);
            o.jp[w] = (uint32_t)q;
            const uint32_t off = (uint32_t)(q - p0);
            maxoff = off > maxoff ? off : maxoff;
            uint32_t* em32 = (uint32_t*)(o.rec + (size_t)w * (size_t)o.rstride);   // compact: positions (k_em_scatter)
            em32[0] = (uint32_t)q;
            em32[1] = (uint32_t)c;
            em32[2] = k;
            em32[3] = (1u << 24) | (uint32_t)em;
            em32[4] = (uint32_t)L.pts_pos;
            for (int s = 0; s < dd->n_select; ++s) em32[5 + s] = (uint32_t)L.get_event(dd->sel_state[s], dd->sel_index[s]);
          }
        }
        ++q;
        done = L.dead() || L.overflow;
      }
    }
    const uint64_t dm = __ballot(done);
    if (dm) {
      if (done) {
        if (emitted) ++nemit;
        else o.k1[i] = o.k1_none;   // no match: sorts behind every match
        emitted = false;
        i = nxt + __popcll(dm & lt);
        active = i < hi;
        if (active) {
          const int64_t p = cand[i];
          k = skey[p];
          L.start(p);
          q = p + 1;
          p0 = p;
          e = end[k];
          back = a.kback && a.kback[k];
        }
      }
      nxt += __popcll(dm);
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    nemit += __shfl_down(nemit, off, 64);
    const uint32_t x = __shfl_down(maxoff, off, 64);
    maxoff = x > maxoff ? x : maxoff;
  }
  if (lane == 0 && nemit) {
    atomicAdd(o.count, (unsigned long long)nemit);
    atomicMax(o.maxoff, maxoff);
  }
}

// One 64-bit delivery key per match when it fits: (trigger row, visit slot), then the insertion history as offsets
// back from the trigger's position (a later insertion = a smaller offset), newest first.
__global__ void k_pp_key(int64_t n, const uint64_t* __restrict__ k1, const uint64_t* __restrict__ th,
                         const uint64_t* __restrict__ tl, const uint32_t* __restrict__ jp, uint64_t k1_none, int n_hist,
                         uint32_t maxoff, int ob, uint64_t none, uint64_t* __restrict__ key, uint32_t* __restrict__ idx) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  idx[i] = (uint32_t)i;
  const uint64_t a = k1[i];
  if (a == k1_none) { key[i] = none; return; }
  uint64_t x = ((a >> 8) << 4) | (a & 15u);
  const uint32_t J = jp[i];
  for (int j = 0; j < n_hist; ++j) {
    const uint64_t w = j < 2 ? th[i] : tl[i];
    const uint32_t c = (uint32_t)((j & 1) ? (w & 0x7FFFFFFFu) : ((w >> 31) & 0x7FFFFFFFu));
    const uint32_t off = J - (c >> 4);
    x = (x << (ob + 4)) | ((uint64_t)(maxoff - off) << 4) | (c & 15u);
  }
  key[i] = x;
}

// After the stable sort by k1, the matches of one (trigger row, visit slot) sit together in start-row order: order each
// such run by its insertion history (th, then tl) in place -- what the two LSD tie sorts over all T slots would give,
// for the cost of the runs alone.  A run longer than max_run sets *over and the caller takes the LSD sorts.
__global__ void k_pp_ties(int64_t m, const uint64_t* __restrict__ key, uint32_t* __restrict__ idx,
                          const uint64_t* __restrict__ th, const uint64_t* __restrict__ tl, uint64_t tl_mask, int max_run,
                          int32_t* __restrict__ over) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const uint64_t k = key[i];
  if (i > 0 && key[i - 1] == k) return;   // not the head of its run
  int64_t e = i + 1;
  while (e < m && key[e] == k) {
    if (e - i >= max_run) { atomicOr(over, 1); return; }
    ++e;
  }
  for (int64_t a = i + 1; a < e; ++a) {   // stable insertion sort: equal histories keep start-row order
    const uint32_t v = idx[a];
    const uint64_t hv = th[v], lv = tl[v] & tl_mask;
    int64_t b = a;
    while (b > i) {
      const uint32_t u = idx[b - 1];
      const uint64_t hu = th[u], lu = tl[u] & tl_mask;
      if (hu < hv || (hu == hv && lu <= lv)) break;
      idx[b] = u;
      --b;
    }
    idx[b] = v;
  }
}

// ---- host side ------------------------------------------------------------------------------------------------
// the rows that start a partial, compacted: cand[i] = the position of the i-th start row
static uint32_t start_rows(SgHandle* h, int64_t m, uint32_t* flag, uint32_t** cand) {
  hipStream_t st = h->stream;
  uint32_t* fpos = (uint32_t*)h->ws.get("pp_fpos", 4 * (m + 1), st);
  *cand = (uint32_t*)h->ws.get("pp_cand", 4 * (m + 1), st);
  h->kbeg("start_rows");
  HIPCHK(hipMemsetAsync(flag + m, 0, 4, st));
  sg_exclusive_scan(h->ws, st, "pp_fscan_tmp", flag, fpos, (uint32_t)0, (size_t)m + 1, rocprim::plus<uint32_t>());
  if (m) hipLaunchKernelGGL(k_pp_compact, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, m, flag, fpos, *cand);
  HIPCHK(hipGetLastError());
  h->kend();
  return sg_read_back(fpos + m, st);
}

// one output slot per start row: a partial completes at most once (sg_pp_rule)
static PpOut lane_output(SgHandle* h, uint32_t ncand, const K1Layout& k1, int32_t* fail) {
  hipStream_t st = h->stream;
  const int nsel = h->desc.n_select;
  const int64_t cap = std::max<int64_t>(ncand, 1);
  PpOut o;
  o.rec = (char*)h->ws.get("pp_rec", (size_t)cap * (32 + 8 * nsel), st);
  o.k1 = (uint64_t*)h->ws.get("pp_k1", 8 * cap, st);
  o.th = (uint64_t*)h->ws.get("pp_th", 8 * cap, st);
  o.tl = (uint64_t*)h->ws.get("pp_tl", 8 * cap, st);
  o.count = (unsigned long long*)h->ws.get("pp_count", 16, st);
  o.maxoff = (uint32_t*)(o.count + 1);
  o.jp = (uint32_t*)h->ws.get("pp_jp", 4 * cap, st);
  o.fail = fail;
  o.rstride = em_compact_stride(nsel);
  o.k1_none = k1.none;
  HIPCHK(hipMemsetAsync(o.count, 0, 16, st));
  return o;
}

// the carry: lanes still pending after their key's last row mark the rows they hold (PpLane::witnesses) in a.keep
static uint32_t* carry_marks(SgHandle* h, int64_t m, PpArgs& a) {
  hipStream_t st = h->stream;
  if (h->opt.no_carry || !m) return nullptr;
  uint32_t* keep = (uint32_t*)h->ws.get("pp_keep", 4 * (m + 1), st);
  uint8_t* kst = (uint8_t*)h->ws.get("pp_kstart", (size_t)m + 1, st);
  HIPCHK(hipMemsetAsync(keep, 0, 4 * (m + 1), st));
  HIPCHK(hipMemsetAsync(kst, 0, (size_t)m + 1, st));
  a.keep = keep;
  a.kstart = kst;
  return keep;
}

// wait-term block summaries (chain.h PpWait): only without nulls (a null row passes `!=`), 4-byte attributes
static void wait_summaries(SgHandle* h, const PartialState* ps, int64_t m, PpPacked& P) {
  const sg_nfa_desc& d = h->desc;
  hipStream_t st = h->stream;
  P.wsum = nullptr;
  if (!ps->rule.wait_slots || P.nul || m <= 0) return;
  uint32_t slots = 0, fslots = 0;
  int nw = 0;
  for (int k = 0; k < SG_MAX_RET; ++k) P.wix[k] = -1;
  for (int s = 0; s < d.n_states; ++s) {
    const PpWait& w = ps->rule.wait[s];
    if (!w.ok || w.slot >= d.n_ret || P.wide[w.slot] || !P.val[w.slot] || ((slots >> w.slot) & 1u)) continue;
    slots |= 1u << w.slot;
    if (w.fast == 2) fslots |= 1u << w.slot;
    P.wix[w.slot] = (int8_t)nw++;
  }
  bool all = true;   // every wait term's attribute summarized (wait_on may return any of them)
  for (int s = 0; s < d.n_states; ++s)
    if (ps->rule.wait[s].ok && !((slots >> ps->rule.wait[s].slot) & 1u)) all = false;
  if (!nw || !all) return;
  P.wnb = (m + 7) / 8;
  uint2* ws = (uint2*)h->ws.get("pp_wsum", sizeof(uint2) * (size_t)nw * (size_t)P.wnb, st);
  P.wsum = ws;
  h->kbeg("wait_sum");
  hipLaunchKernelGGL(k_pp_wsum, dim3((unsigned)((P.wnb + 255) / 256)), dim3(256), 0, st, m, P, slots, fslots, ws);
  HIPCHK(hipGetLastError());
  h->kend();
}

// the lane kernel's variant: FAST whenever the query's terms allow it (sg_terms_fast)
static const void* lanes_fn(const PartialState* ps) {
  return ps->pp_small && ps->lanes_fast && ps->shape_c3 ? (const void*)k_pp_lanes<PpSmall, true, PpShapeC3>
         : ps->pp_small && ps->lanes_fast               ? (const void*)k_pp_lanes<PpSmall, true>
         : ps->pp_small                                 ? (const void*)k_pp_lanes<PpSmall>
                                                        : (const void*)k_pp_lanes<PpBig>;
}

static void run_lanes(SgHandle* h, const PartialState* ps, PpArgs a, const PpOrdered& r, const uint32_t* cand,
                      int64_t ncand, PpOut o) {
  h->kbeg("partial_lanes");
  if (ncand) {
    int64_t wcands = PP_WAVE_CANDS;
    const dim3 gl((unsigned)((ncand + wcands * (PP_BLOCK / 64) - 1) / (wcands * (PP_BLOCK / 64))));
    PpPacked P = r.P;
    const DevDesc* dd = h->ddesc;
    const SgPpRule* ru = ps->drule;
    const uint32_t *skeys = r.skeys, *sids = r.sids, *end = r.end;
    void* args[] = {&a, &P, &dd, &ru, &cand, &ncand, &skeys, &sids, &end, &o, &wcands};
    HIPCHK(hipLaunchKernel(lanes_fn(ps), gl, dim3(PP_BLOCK), args, 0, h->stream));
  }
  HIPCHK(hipGetLastError());
  h->kend();
}

struct PpCounts {
  int64_t total;              // matches
  uint32_t maxoff;            // largest (trigger position - start position) of a match
};
static PpCounts read_lane_counts(SgHandle* h, const PpOut& o) {
  hipStream_t st = h->stream;
  unsigned long long total = 0;
  uint32_t hmaxoff = 0;
  int32_t fail = 0;
  HIPCHK(hipMemcpyAsync(&total, o.count, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(&hmaxoff, o.maxoff, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(&fail, o.fail, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (fail) throw SgError(fail, "partial lane capacity exceeded (query outside the route's shape)");
  return PpCounts{(int64_t)total, hmaxoff};
}

// ---- delivery order: the T slots (one per start row; slots without a match sort behind, k1 = k1_none) sorted by
// (trigger row, visit slot), ties by insertion history (th, then tl).  Each way returns the sorted slot ids.
struct PpOrderBufs {
  uint32_t *ia, *ib;
  uint64_t *ka, *kb;
};

static void sort_pairs64(SgHandle* h, const char* tag, uint64_t* k_in, uint64_t* k_out, uint32_t* v_in, uint32_t* v_out,
                         int64_t n, int end_bit) {
  sg_radix_sort_pairs(h->ws, h->stream, std::string("pp_sorttmp_") + tag, k_in, k_out, v_in, v_out, (size_t)n, end_bit);
}

// one radix sort over a single composed key of `need` bits (k_pp_key)
static const uint32_t* order_by_composed_key(SgHandle* h, const PpOrderBufs& b, const PpOut& o, int64_t T, int n_hist,
                                             uint32_t maxoff, int ob, int need) {
  const uint64_t none = (1ull << need) - 1;
  hipLaunchKernelGGL(k_pp_key, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, h->stream, T, o.k1, o.th, o.tl, o.jp,
                     o.k1_none, n_hist, maxoff, ob, none, b.ka, b.ia);
  sort_pairs64(h, "one", b.ka, b.kb, b.ia, b.ib, T, need);
  return b.ib;
}

// k1 first, then the tie runs in place (k_pp_ties); nullptr when a run is longer than 256 matches
static const uint32_t* order_by_tie_runs(SgHandle* h, const PpOrderBufs& b, const PpOut& o, int64_t T, int64_t total,
                                         int k1_bits, uint64_t tl_mask) {
  hipStream_t st = h->stream;
  const dim3 blk(256);
  int32_t hover = 1;
  int32_t* over = (int32_t*)h->ws.get("pp_over", 4, st);
  HIPCHK(hipMemsetAsync(over, 0, 4, st));
  hipLaunchKernelGGL(k_pp_iota, dim3((unsigned)((T + 255) / 256)), blk, 0, st, T, b.ia);
  sort_pairs64(h, "k1", o.k1, b.kb, b.ia, b.ib, T, k1_bits);
  hipLaunchKernelGGL(k_pp_ties, dim3((unsigned)((total + 255) / 256)), blk, 0, st, total, b.kb, b.ib, o.th, o.tl, tl_mask,
                     256, over);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(&hover, over, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return hover ? nullptr : b.ib;
}

// LSD stable sorts: tie low word (histories of three insertions), tie high word, then trigger row and visit slot
static const uint32_t* order_by_lsd_sorts(SgHandle* h, PpOrderBufs b, const PpOut& o, int64_t T, int n_hist, int k1_bits,
                                          int eb) {
  hipStream_t st = h->stream;
  const dim3 blk(256), g2((unsigned)((T + 255) / 256));
  hipLaunchKernelGGL(k_pp_iota, g2, blk, 0, st, T, b.ia);
  if (n_hist > 2) {
    hipLaunchKernelGGL(k_pp_take, g2, blk, 0, st, T, o.tl, b.ia, b.ka);
    sort_pairs64(h, "lo", b.ka, b.kb, b.ia, b.ib, T, eb);
    std::swap(b.ia, b.ib);
  }
  hipLaunchKernelGGL(k_pp_take, g2, blk, 0, st, T, o.th, b.ia, b.ka);
  sort_pairs64(h, "hi", b.ka, b.kb, b.ia, b.ib, T, 64);
  std::swap(b.ia, b.ib);
  hipLaunchKernelGGL(k_pp_take, g2, blk, 0, st, T, o.k1, b.ia, b.ka);
  sort_pairs64(h, "k1", b.ka, b.kb, b.ia, b.ib, T, k1_bits);
  return b.ib;
}

// One composed key where the history fits 63 bits; else the tie runs; else (a run too long) the LSD sorts.
// sg_options.partial_lanes 1 / 2 forces the tie runs / the LSD sorts even where one key fits (testing).
static const uint32_t* delivery_order(SgHandle* h, const PartialState* ps, const PpOut& o, const K1Layout& k1, int64_t m,
                                      int64_t T, const PpCounts& c) {
  hipStream_t st = h->stream;
  PpOrderBufs b;
  b.ia = (uint32_t*)h->ws.get("pp_ia", 4 * T, st);
  b.ib = (uint32_t*)h->ws.get("pp_ib", 4 * T, st);
  b.ka = (uint64_t*)h->ws.get("pp_ka", 8 * T, st);
  b.kb = (uint64_t*)h->ws.get("pp_kb", 8 * T, st);
  const int n_hist = ps->rule.n_hist;
  int ob = 1;
  while ((1ull << ob) <= (uint64_t)c.maxoff) ++ob;
  const int need = k1.rb + 4 + n_hist * (ob + 4);
  const int order_path = h->opt.partial_lanes;
  if (need <= 63 && order_path == 0) return order_by_composed_key(h, b, o, T, n_hist, c.maxoff, ob, need);
  int tb = 1;
  while ((1ll << tb) < m) ++tb;
  const int comp_bits = tb + 4;   // one history component: combined row << 4 | visit slot
  const int eb = std::min(64, 31 + comp_bits);
  if (order_path != 2) {
    const uint64_t tl_mask = n_hist <= 2 ? 0ull : (eb >= 64 ? ~0ull : (1ull << eb) - 1);
    if (const uint32_t* order = order_by_tie_runs(h, b, o, T, c.total, k1.bits, tl_mask)) return order;
  }
  return order_by_lsd_sorts(h, b, o, T, n_hist, k1.bits, eb);
}
