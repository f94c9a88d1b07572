// Partial lanes (chain.h): the general machine's route for patterns whose partial matches never interact
// (sg_pp_rule: `every e1=S[local] -> ... within T` over stream / count / logical states of one stream) -- and, behind
// the same front end, sequence lanes (seq.h, sq_lanes.h) for `every`-started sequences.
//
// Per sg_push, with the rows carried from earlier pushes listed first ("carried rows": the rows every partial still
// pending holds -- its e1, its bound slots, its count chains -- with the e1 rows marked as starts; replaying them
// rebuilds exactly those partials, whatever the order of time, chain.h PpLane::witnesses); sg_partial_push below runs
// these in order:
//   1. predicate pass  condition bits of every event-local filter over the batch (pred.h local_pred_pass)
//   2. key order       (pp_rows.h key_ordered_rows) combined rows (carried, then the batch) -> partition key
//                      (PartitionStreamReceiver routing), a stable radix sort of (key, combined row): each key's rows
//                      contiguous, in arrival order -- the rows' fields travel through the sort as one record
//                      (k_pp_rec, k_pp_unpack) or are gathered after it (k_pp_route, k_pp_pack); k_pp_segments: per-key
//                      bounds and the keys whose timestamps go back somewhere (also across pushes)
//      -- sequence lanes go on in sq_lanes.h seq_lanes_push from here --
//   3. start rows      (pp_lanes.h) the rows that start a partial, compacted; block summaries of the wait attributes
//   4. k_pp_lanes      one lane per row that starts a partial (a batch row passing the start state's filter, or a
//                      carried start): chain.h's PpLane runs that partial alone over the key's following rows until it
//                      dies (|ts - e1.ts| > within drops it everywhere but in a count state short of its minimum); a
//                      match is written as a compact record of positions with its sort key (trigger row, visit slot)
//                      and its insertion history (tie key); a partial still pending at the key's last row marks the
//                      rows it holds for the carry
//   5. match order     (pp_lanes.h delivery_order) stable radix sorts: tie words, then (trigger, visit slot) -> the
//                      reference's delivery order; k_em_scatter (pp_emit.h) writes the match records
//   6. carry           (pp_rows.h carry_rows) the marked rows, in arrival order, with their start flags
// Time going back needs no special case: expiry compares |e1.ts - ts| with `within` in every step, a partial parked in
// a count state (CountPreStateProcessor never expires one, CountPreStateProcessor.java:53-93) keeps walking the key's
// rows and is carried however old it is, and a key whose time goes back skips rows only while it waits in a count
// state.
#include <cstdlib>
#include <cstring>
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include <algorithm>

#include "sg_engine.h"
#include "sg_prim.h"
#include "pred.h"
#include "pp_rows.h"
#include "pp_emit.h"
#include "pp_lanes.h"
#include "sq_lanes.h"

// Record sort (see k_pp_rec): the retained slots the non-local filters read must fit two 32-bit words; partial
// lanes carry the timestamp in the record instead of condition bits, so only the start state may be event-local.
// Fills ps->hot and ps->rec_ok.
static void rec_plan(PartialState* ps, const sg_nfa_desc& d) {
  for (int k = 0; k < SG_MAX_RET; ++k) ps->hot[k] = -1;
  int words = 0;
  bool fits = true;
  for (int k = 0; k < d.n_ret && fits; ++k) {
    bool used = false;
    for (int s2 = 0; s2 < d.n_states && !used; ++s2) {
      const sg_state_desc& x = d.states[s2];
      if (x.local) continue;
      for (int pc = 0; pc < x.prog_len;) {
        const int64_t op = d.code[x.prog_off + pc];
        if (op == SG_OP_VAR) { if (d.code[x.prog_off + pc + 3] == k) used = true; pc += 5; }
        else if (op == SG_OP_CONST || op == SG_OP_CMP || op == SG_OP_MATH) pc += 3;
        else pc += 1;
      }
    }
    if (!used) continue;
    const bool wide = d.ret_type[k] == SG_T_LONG || d.ret_type[k] == SG_T_DOUBLE;
    if (words + (wide ? 2 : 1) > 2) { fits = false; break; }
    ps->hot[k] = (int8_t)(wide ? 2 : words);
    words += wide ? 2 : 1;
  }
  uint32_t local_mask = 0;
  for (int s2 = 0; s2 < d.n_states; ++s2) if (d.states[s2].local) local_mask |= 1u << s2;
  ps->rec_ok = fits && (ps->mode == 2 || (local_mask & ~(1u << ps->rule.start)) == 0);
}

PartialState* sg_partial_new(const sg_nfa_desc& d) {
  SgPpRule ru = sg_pp_rule(d);
  SgSeqRule sr = sg_seq_rule(d);
  if (!ru.ok && !sr.ok) return nullptr;
  PartialState* ps = new PartialState();
  ps->mode = ru.ok ? 1 : 2;
  ps->rule = ru;
  ps->srule = sr;
  ps->pp_small = sg_pp_small(ru, d) ? 1 : 0;
  if (ps->mode == 2) {
    ps->rule.local_mask = sr.local_mask;
    ps->rule.start = sr.start;
    ps->rule.recv = sr.recv;
    ps->sq_small = sg_seq_small(sr, d) ? 1 : 0;
    ps->sq_bytes = ps->sq_small ? sizeof(SeqStateT<SqSmall>) : sizeof(SeqState);
    if (hipMalloc(&ps->dsrule, sizeof(SgSeqRule)) != hipSuccess) { delete ps; throw SgError(SG_EHIP, "hipMalloc rule"); }
    hipMemcpy(ps->dsrule, &ps->srule, sizeof(SgSeqRule), hipMemcpyHostToDevice);
  }
  ps->lanes_fast = (ps->mode == 2 ? sg_terms_fast(sr, d.n_states) : sg_terms_fast(ru, d.n_states)) ? 1 : 0;
  ps->shape_c3 = (ps->mode == 1 && sg_pp_shape_is<PpShapeC3>(d, ru)) ? 1 : 0;
  ps->shape_c3b = (ps->mode == 2 && sg_sq_shape_is<SqShapeC3b>(d, sr)) ? 1 : 0;
  for (int s = 0; s < d.n_states; ++s) ps->has_count |= d.states[s].kind == SG_K_COUNT;
  for (int k = 0; k < d.n_ret; ++k) {
    const int c = d.ret_col[k];
    ps->used_col[c] = 1;
    ps->col_bytes[c] = (d.col_type[c] == SG_T_LONG || d.col_type[c] == SG_T_DOUBLE) ? 8 : 4;
  }
  rec_plan(ps, d);
  if (hipMalloc(&ps->drule, sizeof(SgPpRule)) != hipSuccess) { delete ps; throw SgError(SG_EHIP, "hipMalloc rule"); }
  hipMemcpy(ps->drule, &ps->rule, sizeof(SgPpRule), hipMemcpyHostToDevice);
  return ps;
}

void sg_partial_free(PartialState* ps) {
  if (!ps) return;
  rows_free(ps->rows[0]);
  rows_free(ps->rows[1]);
  if (ps->drule) hipFree(ps->drule);
  if (ps->dsrule) hipFree(ps->dsrule);
  if (ps->kst) hipFree(ps->kst);
  if (ps->kst_out) hipFree(ps->kst_out);
  delete ps;
}

void sg_partial_reset(PartialState* ps) {
  if (!ps) return;
  ps->rows[0].n = ps->rows[1].n = 0;
  ps->active = 1;
  ps->seq_pushes = 0;
  if (ps->kst) hipMemset(ps->kst, 0, ps->sq_bytes * (size_t)ps->kst_keys);
}

int sg_partial_active(const PartialState* ps) { return ps && ps->active; }
void sg_partial_deactivate(PartialState* ps) {
  if (ps) ps->active = 0;
}

int64_t sg_partial_carried(const PartialState* ps) { return ps->rows[ps->cur].n; }

// Rows the next push may carry (carried rows included) before a tie component's 27-bit combined row overflows:
// larger pushes are cut into sub-pushes by the caller (a stream without carry runs on the machine instead).
int64_t sg_partial_max_rows(SgHandle* h, PartialState* ps) {
  if (ps->mode != 1 || h->opt.no_carry) return INT64_MAX;
  const char* e = getenv("SG_DEBUG_PP_ROW_BUDGET");   // (debug: a lower budget exercises sub-pushes)
  const int64_t v = e ? atoll(e) : 0;
  const int64_t lim = v > 0 && v < ((int64_t)1 << 27) ? v : ((int64_t)1 << 27);
  return lim - 1 - ps->rows[ps->cur].n;
}

// sg_options.bounded_lateness: with every later row at most max_lateness_ms behind the largest timestamp so far, a
// partial whose e1 is more than `within` before (that - max_lateness_ms) never sees a row it could emit at again.
// Sets a.drop_before / a.dead_after -- only when every state a partial can emit from expires it by `within`: a count
// state never does, so a query whose count state is a final one keeps every partial.
static void lateness_bound(SgHandle* h, const BatchView& bv, int64_t n, PpArgs& a) {
  const sg_nfa_desc& d = h->desc;
  hipStream_t st = h->stream;
  a.drop_before = INT64_MIN;
  a.dead_after = INT64_MAX;
  bool lat_ok = h->opt.bounded_lateness && n > 0 && d.within >= 0;
  for (int s = 0; s < d.n_states; ++s)
    if (d.states[s].kind == SG_K_COUNT && d.states[s].has_selector) lat_ok = false;
  if (!lat_ok) return;
  int64_t* dmax = (int64_t*)h->ws.get("pp_tsmax", sizeof(int64_t), st);
  sg_reduce(h->ws, st, "pp_tsmax_tmp", bv.ts, dmax, INT64_MIN, (size_t)n, rocprim::maximum<int64_t>());
  int64_t hm = sg_read_back(dmax, st);
  h->ts_max_seen = std::max(h->ts_max_seen, hm);
  const int64_t lat = std::max<int64_t>(0, h->opt.max_lateness_ms);
  const int64_t w = std::max<int64_t>(0, d.within);
  if (h->ts_max_seen > INT64_MIN / 2 && w < (int64_t)1 << 60 && lat < (int64_t)1 << 60) {
    a.drop_before = h->ts_max_seen - lat - w;
    a.dead_after = w + lat;
  }
}

// Returns 1 when the push ran on partial lanes, 0 when it breaks the route's precondition (nothing was changed).
int sg_partial_push(SgHandle* h, PartialState* ps, const BatchView& bv, int64_t n, uint32_t kb) {
  hipStream_t st = h->stream;
  const PpRows& cr = ps->rows[ps->cur];
  const int64_t nc = h->opt.no_carry ? 0 : cr.n;
  const int64_t m = nc + n;
  if (ps->mode == 1 && m >= ((int64_t)1 << 27)) {   // tie components hold a combined row in 27 bits
    // (the caller cuts pushes into sub-pushes of sg_partial_max_rows; the carried partials cannot leave the route)
    if (nc > 0) throw SgError(SG_ECAPACITY, "partial-lane route: push at most 2^27 rows at a time (carried rows included)");
    return 0;
  }
  PpArgs a;
  memset(&a, 0, sizeof(a));
  a.nc = nc;
  a.n = n;
  a.base_index = bv.base_index;
  a.index = bv.index;
  a.bts = bv.ts;
  a.cts = cr.ts;
  a.stream = bv.stream;
  a.bkey = bv.key;
  a.ckey = cr.key;
  a.cstart = ps->mode == 1 && nc > 0 ? cr.start : nullptr;
  lateness_bound(h, bv, n, a);
  int32_t* err = (int32_t*)h->ws.get("pp_err", 8, st);   // {route and record flags, lane failure}
  HIPCHK(hipMemsetAsync(err, 0, 8, st));
  h->mark(0);
  local_pred_pass(h, bv, n, "pp_lbits", a.lbits);
  h->mark(1);
  PpOrdered r = key_ordered_rows(h, ps, bv, a, kb, err);
  h->mark(2);
  if (ps->mode == 2) return seq_lanes_push(h, ps, bv, n, kb, a, r);
  uint32_t* cand = nullptr;
  const uint32_t ncand = start_rows(h, m, r.flag, &cand);
  const K1Layout k1 = k1_layout(n, 8);
  const PpOut o = lane_output(h, ncand, k1, err + 1);
  uint32_t* keep = carry_marks(h, m, a);
  wait_summaries(h, ps, m, r.P);
  run_lanes(h, ps, a, r, cand, ncand, o);
  h->mark(3);
  const PpCounts c = read_lane_counts(h, o);
  if (c.total) {
    h->kbeg("match_order");
    const uint32_t* order = delivery_order(h, ps, o, k1, m, ncand, c);
    emit_in_order(h, bv, r.P, "pp_dest", ncand, c.total, order, o.rec);
    h->kend();
  }
  if (keep) carry_rows(h, ps, bv, a, m, r.skeys, r.sids, keep);
  h->mark(4);
  h->last_events = n;
  h->last_spilled = 0;
  h->last_matches = c.total;
  return 1;
}

// Snapshot of the route's state: the carried rows (the rows pending partials hold, each flagged when a partial starts at
// it -- replaying them rebuilds every partial the reference still holds in StreamPreStateProcessor.pendingStateEventList /
// newAndEveryStateEventList, C/query/input/stream/state/StreamPreStateProcessor.java:352-367) and the latest timestamp.
void sg_partial_snapshot(SgHandle* h, PartialState* ps, SnapW& w) {
  const PpRows& r = ps->rows[ps->cur];
  w.pod((int32_t)ps->mode);
  if (ps->mode == 2) {   // sequence lanes: the per-key machine states as well (seq.h SeqState, positions over the rows)
    w.pod((int64_t)ps->sq_bytes);   // (the state layout: a snapshot restores only into the same geometry)
    w.pod(ps->kst_keys);
    w.pod(ps->seq_pushes);
    if (ps->kst_keys) w.dev(ps->kst, ps->sq_bytes * (size_t)ps->kst_keys, h->stream);
  }
  w.pod(r.n);
  if (!r.n) return;
  w.dev(r.ts, 8 * r.n, h->stream);
  w.dev(r.key, 4 * r.n, h->stream);
  w.dev(r.start, r.n, h->stream);
  for (int j = 0; j < SG_MAX_COLS; ++j) {
    if (!ps->used_col[j]) continue;
    w.dev(r.col[j], (size_t)ps->col_bytes[j] * r.n, h->stream);
    w.dev(r.nul[j], r.n, h->stream);
  }
}

void sg_partial_restore(SgHandle* h, PartialState* ps, SnapR& rd) {
  sg_partial_reset(ps);
  ps->nulls_seen = 1;   // the restored rows may hold nulls
  if (rd.pod<int32_t>() != ps->mode) throw SgError(SG_EINVAL, "snapshot: lane route differs");
  if (ps->mode == 2) {
    if (rd.pod<int64_t>() != (int64_t)ps->sq_bytes) throw SgError(SG_EINVAL, "snapshot: sequence state layout differs");
    const int64_t keys = rd.pod<int64_t>();
    const int64_t pushes = rd.pod<int64_t>();
    if (keys < 0 || keys > ((int64_t)1 << 31)) throw SgError(SG_EINVAL, "snapshot: bad sequence state count");
    if (keys > ps->kst_keys) {
      if (ps->kst) hipFree(ps->kst);
      if (ps->kst_out) hipFree(ps->kst_out);
      ps->kst = ps->kst_out = nullptr;
      if (hipMalloc(&ps->kst, ps->sq_bytes * (size_t)keys) != hipSuccess ||
          hipMalloc(&ps->kst_out, ps->sq_bytes * (size_t)keys) != hipSuccess)
        throw SgError(SG_ECAPACITY, "hipMalloc sequence states");
      ps->kst_keys = keys;
    }
    if (ps->kst_keys) HIPCHK(hipMemset(ps->kst, 0, ps->sq_bytes * (size_t)ps->kst_keys));
    if (keys) rd.dev(ps->kst, ps->sq_bytes * (size_t)keys, h->stream);
    ps->seq_pushes = pushes;
  }
  const int64_t n = rd.pod<int64_t>();
  if (n < 0 || n >= ((int64_t)1 << 31)) throw SgError(SG_EINVAL, "snapshot: bad carried row count");
  PpRows& r = ps->rows[ps->cur];
  rows_reserve(ps, r, n);
  if (n) {
    rd.dev(r.ts, 8 * n, h->stream);
    rd.dev(r.key, 4 * n, h->stream);
    rd.dev(r.start, n, h->stream);
    for (int j = 0; j < SG_MAX_COLS; ++j) {
      if (!ps->used_col[j]) continue;
      rd.dev(r.col[j], (size_t)ps->col_bytes[j] * n, h->stream);
      rd.dev(r.nul[j], n, h->stream);
    }
  }
  r.n = n;
}
