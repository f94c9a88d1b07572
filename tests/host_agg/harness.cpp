// TEST-ONLY: siddhi_amd/csrc/agg_ops.h compiled for the CPU (SG_HOST_ONLY), so that tests/test_agg_cases.py can check
// the scan's combine operators against the serial step without a GPU.
#define SG_HOST_ONLY
#include "../../siddhi_amd/csrc/agg_ops.h"

extern "C" {

int ha_state_bytes() { return (int)sizeof(SgAggState); }
void ha_empty(SgAggState* s) { *s = sg_agg_empty(); }
void ha_step(int kind, int atype, SgAggState* s, int64_t bits, int null) { sg_agg_step(kind, atype, *s, bits, null); }
int64_t ha_result(int kind, int atype, const SgAggState* s, int* null) { return sg_agg_result(kind, atype, *s, null); }
int ha_scannable(int kind, int atype) { return sg_agg_scannable(kind, atype) ? 1 : 0; }
void ha_lift(int kind, int atype, int64_t bits, int null, SgAggState* e) { *e = sg_agg_lift(kind, atype, bits, null); }
void ha_seed(int kind, int atype, const SgAggState* s, SgAggState* e) { *e = sg_agg_seed(kind, atype, *s); }
void ha_unseed(int kind, int atype, const SgAggState* e, SgAggState* s) { *s = sg_agg_unseed(kind, atype, *e); }
void ha_combine(int kind, int atype, const SgAggState* a, const SgAggState* b, SgAggState* o) {
  *o = sg_agg_combine(kind, atype, *a, *b);
}
int ha_result_type(int kind, int atype) { return sg_agg_result_type(kind, atype); }

// what the scan must NOT use for max: the IEEE-style operator, a NaN on either side winning (the test shows that the
// fold-against-serial check tells it from the real one)
void ha_naive_max_combine(int atype, const SgAggState* a, const SgAggState* b, SgAggState* o) {
  *o = *a;
  if (!(a->f & SG_AF_HAS)) { *o = *b; return; }
  if (!(b->f & SG_AF_HAS)) return;
  const bool an = (a->f & SG_AF_NANFIRST) || !(a->f & SG_AF_EXT), bn = (b->f & SG_AF_NANFIRST) || !(b->f & SG_AF_EXT);
  if (an || bn) { o->f = SG_AF_HAS | SG_AF_NANFIRST; o->v = 0; return; }
  if (sg_agg_less(atype, a->v, b->v)) o->v = b->v;
}

}  // extern "C"
