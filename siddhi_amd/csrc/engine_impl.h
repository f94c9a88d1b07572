#pragma once
// engine_impl.h — MI355X closed-form pipeline for  every A[l] -> B[l' and B.x OP A.x] within T
// (SG_SHAPE_EVERY_NEXT_CMP: configs C1/C2/C5): the stages of one push and their driver, run_every_next.
//
// Semantics, restated from StreamPreStateProcessor.processAndReturn
// (C/query/input/stream/state/StreamPreStateProcessor.java:292-337: lazy `within` expiry, bind,
// filter, remove on state change), the `every` re-arm in StreamPostStateProcessor.process (:53-72) and
// the reverse-registration visit order of MultiProcessStreamReceiver (C/query/input/
// MultiProcessStreamReceiver.java:98-309, B's state is visited before A's for the same event):
//   per key, e2's pending list holds the e1 partials in arrival order; an event j of the key first
//   drops the partials whose e1 is older than ts_j - T, then (if it is a B event passing B's local
//   filter) completes every pending partial i with x_j OP x_i -- delivered in pending order -- and
//   finally (if it passes A's filter) appends itself as a new partial.
//
// One sg_push runs on one HIP stream with its inputs resident in HBM.  Which route a push takes, with the
// thresholds and the kernels of each, is tabled in DESIGN.md section 3; in pipeline order:
//   predicate pass  (pred.h) A's filter and B's local conjuncts per row -> two condition bitmasks.
//   k_nge           (walk.h) unpartitioned streams: one lane per candidate searches forward for the row that
//                   completes or expires it; a search that grows too long sends the push to the walker.
//   key partition   (keypart.h) per key its walker records in arrival order: the LDS counting sort in one or two
//                   passes up to 65,536 keys, with pass 1 in two beyond that (part1_wide), or a rocPRIM radix sort.
//   group walker    (gwalk.h) beyond 65,536 keys: one workgroup per group of 256 keys walks pass 1's output in one
//                   go; when it declines, pass 2 of the partition and the tiled walker go on from the same records.
//   tiled walker    (walk.h) one lane per (key, time chunk) unit runs the reference's pending list: count passes
//                   (a second one with the exact walker for keys whose time goes back, and an HBM-list redo of
//                   units that outgrow the LDS ring), an exclusive scan over arrival order, then the record pass
//                   and the projection into output records.
//   carry           (walk.h) per key its final pending list survives into the next push as candidate-only virtual
//                   rows [0, nc), replayed but never emitting.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>

#include "gwalk.h"
#include "keypart.h"
#include "pred.h"
#include "sg_device.h"
#include "sg_engine.h"
#include "sg_prim.h"
#include "walk.h"
#include "walk_rec.h"

// (instantiated per value type by engine_{f32,f64,i32,i64}.hip so the build parallelises)

// ---------------------------------------------------------------------------------------------
// The stages of one push, in pipeline order (run_every_next below is the driver).

// Key bound of a partitioned push: the caller's, or the largest key of the batch + 1; never below an earlier push's.
static uint32_t key_bound(SgHandle* h, const BatchView& bv, int64_t n) {
  hipStream_t st = h->stream;
  uint32_t kb = bv.key_bound > 0 ? (uint32_t)bv.key_bound : 0;
  if (kb == 0) {
    int32_t* dmax = (int32_t*)h->ws.get("kmax", sizeof(int32_t), st);
    sg_reduce(h->ws, st, "kmax_tmp", bv.key, dmax, (int32_t)-1, (size_t)n, rocprim::maximum<int32_t>());
    kb = (uint32_t)std::max(sg_read_back(dmax, st) + 1, 1);
  }
  if (kb < h->key_bound_seen) kb = h->key_bound_seen;
  h->key_bound_seen = kb;
  return kb;
}

// 1. predicate pass: A's filter and B's local conjuncts per batch row -> condition bitmasks
struct PredOut {
  PredArgs pa;
  uint64_t* cand_m;
  uint64_t* cons_m;           // null: every batch row is a B consumer
};
static PredOut pred_pass(SgHandle* h, const BatchView& bv, int64_t n, int val_col_a, int val_col_b) {
  const sg_nfa_desc& d = h->desc;
  hipStream_t st = h->stream;
  const int a_state = d.shape_args[0], b_state = d.shape_args[1];
  PredOut p;
  PredArgs& pa = p.pa;
  memset(&pa, 0, sizeof(pa));
  pa.n = n;
  pa.stream = bv.stream;
  pa.s_a = d.states[a_state].stream;
  pa.s_b = d.states[b_state].stream;
  pa.val_col_a = val_col_a;
  pa.val_col_b = val_col_b;
  pa.prog_a_off = d.states[a_state].prog_off;
  pa.prog_a_len = d.states[a_state].prog_len;
  pa.prog_b_off = d.shape_prog_off;
  pa.prog_b_len = d.shape_prog_len;
  pa.cons_all = (!bv.stream && pa.s_b == 0 && pa.prog_b_len == 0 && !bv.cols.nul[val_col_b]) ? 1 : 0;
  const int64_t ntiles = (n + 255) / 256;
  p.cand_m = (uint64_t*)h->ws.get("cand_m", sizeof(uint64_t) * 4 * (ntiles + 1), st);
  p.cons_m = pa.cons_all ? nullptr : (uint64_t*)h->ws.get("cons_m", sizeof(uint64_t) * 4 * (ntiles + 1), st);
  h->mark(0);
  h->kbeg("pred");
  launch_pred(d, pa, bv.stream, bv.cols, h->ddesc, p.cand_m, p.cons_m, st);
  HIPCHK(hipGetLastError());
  h->kend();
  h->mark(1);
  return p;
}

// The virtual row domain of the push (carried rows, then the batch) and the carried columns.
struct VirtOut {
  Virt v;
  SgCols cc;
};
static VirtOut make_virt(const PushCtx& c, const CarrySet& cs, const PredOut& pred, const PushPlan& plan) {
  const sg_nfa_desc& d = c.h->desc;
  VirtOut o;
  Virt& v = o.v;
  memset(&v, 0, sizeof(v));
  v.nc = c.nc;
  v.n = c.n;
  v.ts = c.bv.ts;
  v.key = c.bv.key;
  v.cand_m = pred.cand_m;
  v.cons_m = pred.cons_m;
  v.val_a = c.bv.cols.col[c.val_col_a];
  v.val_b = c.bv.cols.col[c.val_col_b];
  v.c_ts = cs.ts;
  v.c_key = cs.key;
  v.c_flags = cs.flags;
  v.stream = c.bv.stream;
  v.s_b = pred.pa.s_b;
  v.c_val_a = cs.col[c.val_col_a];
  v.c_val_b = cs.col[c.val_col_b];
  if (plan.pcol >= 0) {
    const int pc = plan.pcol;
    v.pcol = c.bv.cols.col[pc];
    v.c_pcol = cs.col[pc];
    v.pw = sg_col_width(d.col_type[pc]);
    v.pfloat = d.col_type[pc] == SG_T_FLOAT;
  }
  memset(&o.cc, 0, sizeof(o.cc));
  for (int q = 0; q < d.n_cols; ++q) { o.cc.col[q] = cs.col[q]; o.cc.nul[q] = cs.nul[q]; }
  return o;
}

// Time from the push's first to its last batch row (sizes the pending-list rings and the time chunks).
static int64_t push_span_ms(SgHandle* h, const BatchView& bv, int64_t n) {
  int64_t tfl[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(&tfl[0], bv.ts, sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(&tfl[1], bv.ts + (n - 1), sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return tfl[1] - tfl[0];
}

// 3. walk plan: ring capacity and time chunks from the rows per key per `within` window, and the walkers' arguments
struct WalkPlan {
  WalkArgs wa;
  size_t lds_count, lds_write;   // LDS bytes per workgroup of the count / record walk
  dim3 grid;                     // one lane per (key, chunk) unit
  uint32_t nw;                   // waves of units
};
template <class T, bool N>
static WalkPlan walk_plan(const PushCtx& c, const PushPlan& plan, const PredArgs& pa, int64_t span_ms) {
  SgHandle* h = c.h;
  const sg_nfa_desc& d = h->desc;
  WalkPlan wp;
  WalkArgs& wa = wp.wa;
  memset(&wa, 0, sizeof(wa));
  wa.nt = c.nt;
  wa.within = d.within;
  wa.K = c.K;
  wa.lp.pay = plan.pcol >= 0 ? 1 : 0;
  wa.lp.row = plan.e1_row ? 1 : 0;
  wa.pay_in_rec = (WRec<T, N>::has_pay && plan.pcol >= 0) ? 1 : 0;
  const int64_t win = window_rows(c.K, c.nt, d.within, span_ms);
  wa.lp.cap = clamp_cap(h->opt.ring_cap > 0 ? h->opt.ring_cap : pick_cap(win), PendBytes<T>::lds(true, wa.lp));
  wp.lds_count = (size_t)wa.lp.cap * WALK_BLOCK * PendBytes<T>::lds(false, wa.lp);
  wp.lds_write = (size_t)wa.lp.cap * WALK_BLOCK * PendBytes<T>::lds(true, wa.lp);
  wa.C = (uint32_t)pick_chunks(c.K, c.nt, PendBytes<T>::lds(true, wa.lp), wa.lp.cap, win);   // record walk's ring
  wa.R = (uint32_t)((c.nt + wa.C - 1) / wa.C);
  const uint64_t units = (uint64_t)c.K * wa.C;
  if (units >= (1ull << 32)) throw SgError(SG_EINVAL, "too many (key, chunk) units");
  wa.n_units = (uint32_t)units;
  wa.partitioned = d.partitioned;
  wa.op = c.op;
  const bool same_col = (c.val_col_a == c.val_col_b) && (pa.s_a == pa.s_b);
  wa.stack_mode = (same_col && pa.prog_b_len == 0) ? 1 : 0;
  wa.carry_out = h->opt.no_carry ? 0 : 1;
  wa.base_index = c.bv.base_index;
  wa.index = c.bv.index;
  recv_slot(d, d.shape_args[1], wa.multi, wa.b_slot);
  wa.n_select = d.n_select;
  wa.stride = 32 + 8 * d.n_select;
  wp.grid = dim3((unsigned)((units + WALK_BLOCK - 1) / WALK_BLOCK));
  wp.nw = (uint32_t)((units + 63) / 64);
  return wp;
}

// Workspaces of the count and record passes.
template <class T, bool N>
struct WalkBufs {
  UnitDesc* ud;
  WalkStats* wst;
  uint32_t *cnt, *off, *emap, *wlen, *wrow;
  WRec<T, N>* tile = nullptr;   // lane-interleaved tiles of the sorted records (sized per count pass)
  uint64_t* emask = nullptr;
  char* big = nullptr;          // HBM pending lists of the redone units
  MatchSink ms;                 // (record pass: set once the match list is allocated)
};
template <class T, bool N>
static WalkBufs<T, N> walk_bufs(const PushCtx& c, const WalkPlan& wp) {
  SgHandle* h = c.h;
  hipStream_t st = h->stream;
  WalkBufs<T, N> b;
  b.ud = (UnitDesc*)h->ws.get("units", sizeof(UnitDesc) * (size_t)wp.wa.n_units, st);
  b.wst = (WalkStats*)h->ws.get("walkstats", sizeof(WalkStats), st);
  b.cnt = (uint32_t*)h->ws.get("cnt", sizeof(uint32_t) * (c.n + 1), st);
  b.off = (uint32_t*)h->ws.get("off", sizeof(uint32_t) * (c.n + 1), st);
  b.emap = (uint32_t*)h->ws.get("emap", sizeof(uint32_t) * (c.nt / 32 + 2), st);
  b.ms = MatchSink{nullptr, 0, 0, &b.wst->internal};
  b.wlen = (uint32_t*)h->ws.get("wlen", sizeof(uint32_t) * (wp.nw + 1), st);
  b.wrow = (uint32_t*)h->ws.get("wrow", sizeof(uint32_t) * (wp.nw + 1), st);
  return b;
}

// A payload value wider than 32 bits (PK_PAY_RANGE) fits neither the narrow records nor the rings' payload plane:
// e1's attributes are gathered by row instead.  Rewrites
//   PushPlan: pp.kind[s] 0 -> 3 for every select, e1_row = true, pcol = -1;
//   WalkArgs: lp.pay = 0, lp.row = 1, pay_in_rec = 0;
//   both copies of the Virt view (the projection's and the record source's): pcol = null.
// The LDS sizes and the chunking of the walk plan stay as planned.
static void demote_payload(const sg_nfa_desc& d, PushPlan& plan, WalkArgs& wa, Virt& v, Virt& src_v) {
  for (int s = 0; s < d.n_select; ++s)
    if (plan.pp.kind[s] == 0) { plan.pp.kind[s] = 3; plan.e1_row = true; }
  plan.pcol = -1;
  wa.lp.pay = 0;
  wa.lp.row = 1;
  wa.pay_in_rec = 0;
  v.pcol = nullptr;
  src_v.pcol = nullptr;
}

// One count pass's tiles: unit ranges -> per-wave rows -> LDS transpose of the sorted records into lane-interleaved
// tiles.  Returns what the partition flagged about the records (known once the unit scan has been read back).
template <class T, bool N>
static PackRange build_tiles(const PushCtx& c, const KeyPart<T, N>& kp, const WalkPlan& wp, WalkBufs<T, N>& b) {
  typedef WRec<T, N> R;
  SgHandle* h = c.h;
  hipStream_t st = h->stream;
  const uint32_t nw = wp.nw;
  HIPCHK(hipMemsetAsync(b.wlen, 0, sizeof(uint32_t) * (nw + 1), st));
  h->kbeg("units");
  hipLaunchKernelGGL((k_units<T, N>), dim3((unsigned)(nw * 64 + 255) / 256), dim3(256), 0, st, wp.wa, kp.src, kp.seg_b,
                     kp.seg_e, b.ud, b.wlen, b.wst);
  HIPCHK(hipGetLastError());
  sg_exclusive_scan(h->ws, st, "wscan_tmp", b.wlen, b.wrow, (uint32_t)0, (size_t)nw + 1, rocprim::plus<uint32_t>());
  h->kend();
  uint32_t rows_total = 0, pkf = 0;
  HIPCHK(hipMemcpyAsync(&rows_total, b.wrow + nw, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(&pkf, kp.pk_flags, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  const PackRange pr = pack_range(pkf);
  if (pr == PACK_TS_RANGE) return pr;
  b.tile = (R*)h->ws.get("tile", sizeof(R) * 64 * (size_t)std::max<uint32_t>(rows_total, 1), st);
  b.emask = (uint64_t*)h->ws.get("emask", sizeof(uint64_t) * std::max<uint32_t>(rows_total, 1), st);
  const uint32_t nq = rows_total / TROWS;
  if (nq) {
    uint32_t* rmap = (uint32_t*)h->ws.get("rowmap", sizeof(uint32_t) * nq, st);
    hipLaunchKernelGGL(k_rowmap, dim3((nw + 255) / 256), dim3(256), 0, st, b.wlen, b.wrow, nw, rmap);
    HIPCHK(hipGetLastError());
    h->kbeg("tile_transpose");
    hipLaunchKernelGGL((k_transpose<T, N>), dim3(std::min<uint32_t>(nq, 256 * 32)), dim3(256), 0, st, kp.src.srec, b.ud,
                       b.wrow, rmap, nq, b.tile, (uint32_t)c.nt, wp.wa.n_units, b.wst);
    HIPCHK(hipGetLastError());
    h->kend();
  }
  return pr;
}

// 4. count passes: matches per trigger row and their exclusive scan (output offsets in delivery order).
// Pass 0 walks every key on the fast path, which needs each key's time not to go back.  When some key's does (its
// rows, carried ones included, out of time order), pass 1 redoes the count with those keys on the exact walker
// (wa.kexact).  Within a pass, units whose pending list outgrew the LDS ring (or that walk exact) are redone with
// unbounded HBM lists (wa.big_total, b.big).  A payload outside 32 bits demotes the plan (demote_payload).
struct CountOut {
  bool fits = true;           // false: the push spans more than 2^31 ms and needs wide records (nothing changed)
  uint32_t total = 0;         // matches of the push
  WalkStats hs;
};
template <class T, bool N>
static CountOut count_passes(const PushCtx& c, KeyPart<T, N>& kp, WalkPlan& wp, WalkBufs<T, N>& b, PushPlan& plan,
                             Virt& v) {
  SgHandle* h = c.h;
  const sg_nfa_desc& d = h->desc;
  hipStream_t st = h->stream;
  WalkArgs& wa = wp.wa;
  const dim3 wblk(WALK_BLOCK);
  const int64_t n = c.n;
  auto scan_counts = [&]() {
    sg_exclusive_scan(h->ws, st, "scan_tmp", b.cnt, b.off, (uint32_t)0, (size_t)n + 1, rocprim::plus<uint32_t>());
  };
  CountOut co;
  h->extra_marks = 0;
  for (int pass = 0;; ++pass) {
    HIPCHK(hipMemsetAsync(b.cnt, 0, sizeof(uint32_t) * (n + 1), st));
    HIPCHK(hipMemsetAsync(b.emap, 0, sizeof(uint32_t) * (c.nt / 32 + 2), st));
    HIPCHK(hipMemsetAsync(b.wst, 0, sizeof(WalkStats), st));
    const PackRange pr = build_tiles<T, N>(c, kp, wp, b);
    if (pr == PACK_TS_RANGE) { co.fits = false; return co; }
    if (pr == PACK_PAY_RANGE) demote_payload(d, plan, wa, v, kp.src.pk.v);
    h->kbeg("walk_count");
    launch_walk_t<T, N, false>(c.op, wp.grid, wblk, wp.lds_count, st, wa, kp.src, kp.seg_b, kp.seg_e, b.ud, b.wlen, b.wrow,
                               b.tile, b.cnt, b.off, b.ms, b.emask, b.wst);
    h->kend();
    h->kbeg("count_scan");
    scan_counts();
    h->kend();
    h->mark(3);
    HIPCHK(hipMemcpyAsync(&co.total, b.off + n, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&co.hs, b.wst, sizeof(WalkStats), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (co.hs.n_ovf) {
      // units whose pending list outgrew the LDS ring (or that walk exact): redo them with unbounded HBM lists
      if (co.hs.internal & 16u) throw SgError(SG_ECAPACITY, "HBM pending lists exceed 2^32 entries: push smaller batches");
      wa.big_total = co.hs.ovf_total;
      b.big = (char*)h->ws.get("big_lists", (size_t)co.hs.ovf_total * PendBytes<T>::hbm, st);
      h->mark(6);
      hipLaunchKernelGGL((k_walk<T, N, false, true>), wp.grid, wblk, 0, st, wa, kp.src, kp.seg_b, kp.seg_e, b.ud, b.cnt,
                         b.off, b.ms, b.emap, b.wst, b.big);
      HIPCHK(hipGetLastError());
      scan_counts();
      h->mark(7);
      h->extra_marks = 1;
      HIPCHK(hipMemcpyAsync(&co.total, b.off + n, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(&co.hs, b.wst, sizeof(WalkStats), hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
    }
    if (co.hs.internal) throw SgError(SG_EINVAL, "internal: walker guard tripped (" + std::to_string(co.hs.internal) + ")");
    if (!co.hs.order_err) break;
    if (pass) throw SgError(SG_EINVAL, "internal: a key's time went back on the fast walker after the exact pass");
    // keys whose time goes back (StreamPreStateProcessor.isExpired compares |e1.ts - ts| with `within`, and a playback
    // clock that stays put still processes the row, TimestampGeneratorImpl.java:106-125): exact walker
    uint8_t* kx = (uint8_t*)h->ws.get("kexact", c.K, st);
    if (d.partitioned) {
      HIPCHK(hipMemsetAsync(kx, 0, c.K, st));
      hipLaunchKernelGGL((k_order_keys<T, N>), dim3((unsigned)std::min<int64_t>((c.nt + 255) / 256, 256 * 64)), dim3(256), 0,
                         st, kp.src, c.kf, kp.seg_b, c.K, c.nt, kx);
      HIPCHK(hipGetLastError());
    } else {
      HIPCHK(hipMemsetAsync(kx, 1, c.K, st));
    }
    wa.kexact = kx;
  }
  return co;
}

// 5. record pass: the walkers again, now leaving every match at its slot (and each key's final pending list for the
// carry), then the projection into output records.
template <class T, bool N>
static void record_pass(const PushCtx& c, const KeyPart<T, N>& kp, WalkPlan& wp, WalkBufs<T, N>& b, const PushPlan& plan,
                        const VirtOut& vo, const CountOut& co) {
  SgHandle* h = c.h;
  const sg_nfa_desc& d = h->desc;
  hipStream_t st = h->stream;
  WalkArgs& wa = wp.wa;
  const dim3 wblk(WALK_BLOCK);
  const uint32_t total = co.total;
  h->split_out = 1;
  if (!(total || wa.carry_out)) { h->mark(5); return; }
  char* out = h->out.reserve(total, d.n_select, st);
  wa.out_base = h->out.n;
  // narrow match records when the value type is 4 bytes and every payload fits 32 bits (narrow walker records)
  b.ms.narrow = (N && sizeof(T) == 4) ? 1 : 0;
  b.ms.cap = total;
  b.ms.rec = h->ws.get("mrec", (b.ms.narrow ? sizeof(MRec16) : sizeof(MRec)) * std::max<uint32_t>(total, 1), st);
  h->mark(5);
  if (wa.carry_out) {   // each key's final pending list (k_walk / k_walk_t, record pass)
    wa.alive = (uint32_t*)h->ws.get("alive_rows", sizeof(uint32_t) * (size_t)std::max<int64_t>(c.nt, 1), st);
    wa.alive_n = (uint32_t*)h->ws.get("alive_n", sizeof(uint32_t) * 2, st);
    wa.cv_n = wa.alive_n + 1;
    HIPCHK(hipMemsetAsync(wa.alive_n, 0, sizeof(uint32_t) * 2, st));
    wa.cv_cap = (uint32_t)std::max<int64_t>(1, std::min<int64_t>(c.nt, (int64_t)c.K * wa.lp.cap));
    wa.cv_ts = (int64_t*)h->ws.get("cv_ts", sizeof(int64_t) * (size_t)wa.cv_cap, st);
    wa.cv_val = (int64_t*)h->ws.get("cv_val", sizeof(int64_t) * (size_t)wa.cv_cap, st);
    wa.cv_pay = (int64_t*)h->ws.get("cv_pay", sizeof(int64_t) * (size_t)wa.cv_cap, st);
    wa.cv_key = (int32_t*)h->ws.get("cv_key", sizeof(int32_t) * (size_t)wa.cv_cap, st);
  }
  h->kbeg("walk_record");
  launch_walk_t<T, N, true>(c.op, wp.grid, wblk, wp.lds_write, st, wa, kp.src, kp.seg_b, kp.seg_e, b.ud, b.wlen, b.wrow,
                            b.tile, b.cnt, b.off, b.ms, b.emask, b.wst);
  h->kend();
  if (co.hs.n_ovf) {
    hipLaunchKernelGGL((k_walk<T, N, true, true>), wp.grid, wblk, 0, st, wa, kp.src, kp.seg_b, kp.seg_e, b.ud, b.cnt, b.off,
                       b.ms, b.emap, b.wst, b.big);
    HIPCHK(hipGetLastError());
  }
  if (total) {
    h->kbeg("project");
    hipLaunchKernelGGL((k_project<T>), dim3((unsigned)(((int64_t)total + 255) / 256)), dim3(256), (size_t)256 * wa.stride,
                       st, wa, vo.v, plan.pp, c.bv.cols, vo.cc, b.ms, b.off, (int64_t)total, out);
    HIPCHK(hipGetLastError());
    h->kend();
  }
  h->out.n += total;
}

// 6. carry: each key's final pending list (left by the record pass) becomes the next push's carried rows
template <class T, bool N>
static void carry_pass(const PushCtx& c, EveryNextState* es, const WalkPlan& wp, const WalkBufs<T, N>& b,
                       const PushPlan& plan, const VirtOut& vo) {
  const uint32_t guard = sg_read_back(&b.wst->internal, c.h->stream);   // record-pass guards
  if (guard) throw SgError(SG_EINVAL, "internal: record-pass guard tripped (" + std::to_string(guard) + ")");
  carry_out_rows<T, N>(c.h, es, c.nt, vo.v, c.bv, vo.cc, wp.wa, c.val_col_a, vo.v.pcol ? plan.pcol : -1, vo.v.pw);
}

// One push through the closed-form pipeline with walker records of format N (narrow / wide).  Returns false
// (having changed no state) when narrow records cannot represent the push (time span beyond 2^31 ms).
template <class T, bool N>
static bool run_every_next(SgHandle* h, const BatchView& bv, int64_t n, PushPlan plan) {
  typedef WRec<T, N> R;
  const sg_nfa_desc& d = h->desc;
  const int* sa = d.shape_args;
  EveryNextState* es = (EveryNextState*)h->state;
  CarrySet& cs = es->carry[es->cur];
  const int64_t nc = h->opt.no_carry ? 0 : cs.n;
  if (nc + n >= (1ll << 30)) throw SgError(SG_EINVAL, "batch plus carried rows exceed 2^30");
  const uint32_t kb = d.partitioned ? key_bound(h, bv, n) : 1;
  const PushCtx c{h, bv, n, nc, nc + n, kb, d.partitioned ? kb : 1, sa[2], d.ret_col[sa[4]], d.ret_col[sa[3]],
                  KeyOf{bv.key, cs.key, (uint32_t)nc}};

  const PredOut pred = pred_pass(h, bv, n, c.val_col_a, c.val_col_b);
  VirtOut vo = make_virt(c, cs, pred, plan);
  if (!d.partitioned && !h->opt.walker_only && run_nge<T>(h, bv, n, nc, plan, vo.v, vo.cc, c.op, es)) return true;
  const int64_t span_ms = push_span_ms(h, bv, n);

  // ---- 2. key partition: per-key walker records in arrival order
  KeyPart<T, N> kp = part_begin<T, N>(c, vo.v);
  // beyond 65536 keys (C5: 1M per GPU) the LDS partition runs its first pass in two (part1_wide: narrow records only,
  // up to 4096 groups of 256 keys) -- three counting passes in place of pack + a 3-pass onesweep sort + bounds
  constexpr bool wide_ok = N && sizeof(R) == 16 && sizeof(T) == 4;
  const bool wide_part = wide_ok && kb > 65536u && kb <= (4096u << 8);
  if (d.partitioned && (kb <= 65536u || wide_part) && h->opt.partition_sort == 0) {
    const PartLdsBufs<T, N> pb = part_lds_bufs<T, N>(c);
    if (kb <= 65536u) {
      part_lds_pass1<T, N>(c, kp, pb);
    } else if constexpr (wide_ok) {
      // many keys: the group walker (gwalk.h) when the query and the push allow it; when it declines, pass 2 and the
      // tiled walker go on from the grec / glk / o1 that part1_wide left
      const bool same = (c.val_col_a == c.val_col_b) && (pred.pa.s_a == pred.pa.s_b);
      const GwPlan gp = gw_plan<T>(h, bv, n, nc, kb, plan, same, span_ms);
      part1_wide<T>(h, kp.src.pk, c.kf, kb, c.nt, pb.pp, pb.h1, pb.o1, pb.grec, pb.glk, kp.pk_flags);
      if (gp.ok) {
        const int rc = run_group_walk<T>(h, bv, n, nc, kb, pb.pp, pb.o1, pb.grec, pb.glk, kp.pk_flags, gp, plan, vo.v, vo.cc,
                                         c.op, (same && pred.pa.prog_b_len == 0) ? 1 : 0, c.val_col_a, es);
        if (rc == 1) return true;
        if (rc == 2) return false;
      }
    }
    if (pb.pp.two) part_lds_pass2<T, N>(c, kp, pb);
    HIPCHK(hipGetLastError());
    kp.src.srec = pb.srec;
  } else if (d.partitioned) {
    part_sort<T, N>(c, kp);
  } else {
    part_none<T, N>(c, kp);
  }
  h->mark(2);

  // ---- 3-6. walk plan, count passes, record pass + projection, carry
  WalkPlan wp = walk_plan<T, N>(c, plan, pred.pa, span_ms);
  WalkBufs<T, N> wb = walk_bufs<T, N>(c, wp);
  const CountOut co = count_passes<T, N>(c, kp, wp, wb, plan, vo.v);
  if (!co.fits) return false;   // the push spans more than 2^31 ms: wide records
  record_pass<T, N>(c, kp, wp, wb, plan, vo, co);
  h->mark(4);
  if (wp.wa.carry_out) carry_pass<T, N>(c, es, wp, wb, plan, vo);
  h->last_events = n;
  h->last_matches = co.total;
  h->last_spilled = co.hs.n_ovf;
  return true;
}

// Projection plan: which select columns are the compared value and which are gathered by row at emission.
static PushPlan make_plan(SgHandle* h, const BatchView& bv) {
  const sg_nfa_desc& d = h->desc;
  EveryNextState* es = (EveryNextState*)h->state;
  for (int c = 0; c < d.n_cols; ++c) if (bv.cols.nul[c]) es->nul_seen[c] = true;
  const int b_state = d.shape_args[1];
  const int val_col_a = d.ret_col[d.shape_args[4]], val_col_b = d.ret_col[d.shape_args[3]];
  PushPlan pl;
  memset(&pl.pp, 0, sizeof(pl.pp));
  for (int s = 0; s < d.n_select; ++s) {
    ProjPlan& pp = pl.pp;
    pp.src[s] = (d.sel_state[s] == b_state) ? 1 : 0;
    int col = d.ret_col[d.sel_ret[s]];
    int idx = d.sel_index[s];
    pp.col[s] = col;
    pp.type[s] = d.sel_type[s];
    if (idx != 0 && idx != -1) pp.kind[s] = 2;
    else if (col == (pp.src[s] ? val_col_b : val_col_a)) pp.kind[s] = 1;
    else if (pp.src[s] == 0 && !es->nul_seen[col] && d.col_type[col] != SG_T_DOUBLE && (pl.pcol < 0 || pl.pcol == col)) {
      pp.kind[s] = 0;
      pl.pcol = col;
    } else {
      pp.kind[s] = 3;
      if (pp.src[s] == 0) pl.e1_row = true;
    }
  }
  return pl;
}

template <class T>
static void dispatch_np(SgHandle* h, const BatchView& bv, int64_t n) {
  if (!h->state) { h->state = new EveryNextState(); h->state_kind = 1; }
  PushPlan pl = make_plan(h, bv);   // (needs the state: null history)
  // narrow walker records whenever the push fits them (partitioned queries); wide otherwise
  if (!run_every_next<T, true>(h, bv, n, pl)) run_every_next<T, false>(h, bv, n, pl);
}
