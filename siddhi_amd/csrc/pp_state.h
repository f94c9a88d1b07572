// State of the two lane routes of the general family (partial.hip): the carried rows and what the query allows.
#pragma once
#include <cstdint>

#include "sg_engine.h"
#include "chain.h"
#include "seq.h"

// Carried rows: SoA in the batch's own column formats (so the general machine can replay them as a batch).
struct PpRows {
  int64_t n = 0, cap = 0;
  int64_t* ts = nullptr;
  int32_t* key = nullptr;
  uint8_t* start = nullptr;     // partial lanes: the row is the e1 of a pending partial (its lane restarts there)
  void* col[SG_MAX_COLS] = {};
  uint8_t* nul[SG_MAX_COLS] = {};
};

struct PartialState {
  int mode = 1;         // 1: partial lanes (patterns, chain.h), 2: sequence lanes (seq.h)
  SgPpRule rule;
  SgPpRule* drule = nullptr;
  SgSeqRule srule;
  SgSeqRule* dsrule = nullptr;
  void* kst = nullptr;          // sequence lanes: per-key machine state SeqStateT<G> (zero = no runtime yet)
  void* kst_out = nullptr;      // the push's end states (swapped into kst when the push succeeds: a push that runs
                                // out of match space is rerun from kst with more space, StreamPreStateProcessor's
                                // lists being unbounded, C/query/input/stream/state/StreamPreStateProcessor.java:57-58)
  int sq_small = 0;             // the query fits seq.h's small state geometry (SqSmall)
  int pp_small = 0;             // the query fits chain.h's small lane geometry (PpSmall)
  int lanes_fast = 0;           // every filter is fast compares or event-local bits (chain.h sg_terms_fast): the FAST
                                // lane kernels
  int shape_c3 = 0;             // the state table is C3c's family (chain.h PpShapeC3): the specialised lane kernel
  int shape_c3b = 0;            // the state table is C3b's family (seq.h SqShapeC3b): the specialised sequence lanes
  size_t sq_bytes = sizeof(SeqState);
  int64_t kst_keys = 0;
  int64_t seq_pushes = 0;       // pushes that left state behind (after the first, the route cannot be left exactly)
  int64_t last_reruns = 0;      // sequence units rerun from their predecessor's end state in the last push
  int64_t sq_cap_hint = 0;      // match space the last push that outgrew its default needed
  int nulls_seen = 0;           // a push had null flags in a column the query reads (carried rows may hold nulls)
  int8_t hot[SG_MAX_RET];       // record sort: slot -> word of the 16-B record (-1: gathered), see rec_plan
  int rec_ok = 0;
  int used_col[SG_MAX_COLS] = {};
  int col_bytes[SG_MAX_COLS] = {};
  PpRows rows[2];       // carried rows (cur) and the next push's (double buffer)
  int cur = 0;
  int has_count = 0;
  int active = 1;
};
