// The selector's aggregation stage (QuerySelector.processGroupBy / processNoGroupBy with attribute aggregators,
// C/query/selector/QuerySelector.java:125-216): host interface of agg.hip, called by api.hip.
#pragma once
#include "sg_engine.h"

struct AggStage;

// validate the descriptor against the handle's query and build the stage (throws SgError)
AggStage* sg_agg_new(SgHandle& h, const sg_agg_desc* a);
void sg_agg_free(AggStage* ag);
void sg_agg_reset(SgHandle& h, AggStage* ag);
// n base records (delivery order) and the n output records k_select made of them: every aggregate column of `out`
// holds its argument's value on entry and the aggregator's running value on return
void sg_agg_run(SgHandle& h, AggStage* ag, const char* base, int bstride, char* out, int ostride, int64_t n);
void sg_agg_snapshot(SgHandle& h, AggStage* ag, SnapW& w);
void sg_agg_restore(SgHandle& h, AggStage* ag, SnapR& r);
uint64_t sg_agg_fingerprint(const AggStage* ag, uint64_t x);
