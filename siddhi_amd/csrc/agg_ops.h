// Attribute aggregators of the selector (C/query/selector/attribute/aggregator/{Count,Sum,Avg,Min,Max}
// AttributeAggregator.java), as plain __host__ __device__ code: the per-group state, the serial step (processAdd, one
// match at a time) and the associative combine operator the segmented scan of agg.hip runs on.  Compiled for the CPU
// by tests/host_agg (SG_HOST_ONLY), which checks combine against the serial step.
//
// Only processAdd is restated: no expired event reaches a pattern's selector.
//   count   count++ for every match, null argument or not (CountAttributeAggregator.java:77-85); LONG.
//   sum     INT / LONG in a long with wraparound, LONG (SumAttributeAggregator.java:251-336); FLOAT / DOUBLE in a
//           double, one `sum += data` per match, DOUBLE (:160-249).  A null argument returns currentValue(): null while
//           count == 0, else the sum, and changes nothing (:109-113,221-227,314-320).  The FLOAT class's own null test
//           (:234-237) is never reached: the outer aggregator answers a null first (:109-113).
//   avg     a double `value += data` and a long count for every argument type, value / count, DOUBLE
//           (AvgAttributeAggregator.java:153-406); null argument as sum (:102-107,209-214).
//   max     `maxValue == null || maxValue < value` replaces (MaxAttributeAggregator.java:191,274,358,441); min mirrors
//           it with > (MinAttributeAggregator.java).  With NaN every compare is false: a NaN never replaces a value,
//           and a NaN that came first is never replaced; of 0.0 and -0.0 the earlier one stays.
#pragma once
#ifdef SG_HOST_ONLY
#include "sg_host_shim.h"
#else
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>
#include "../../include/siddhi_gpu.h"

// SgAggState.f
#define SG_AF_HAS 1u        // a non-null argument was added
#define SG_AF_NANFIRST 2u   // min / max: the first non-null argument was a NaN (the result stays NaN)
#define SG_AF_EXT 4u        // min / max: v holds the extreme of the non-NaN arguments
#define SG_AF_INEXACT 8u    // scan of avg over INT / LONG only: |value| + sum |x| reached 2^53 (m saturated)

#define SG_AGG_2P53 (1ull << 53)

// One aggregator of one group.  v: the long sum | the bits of the double sum / value | the extreme in the argument's
// type (INT / LONG sign-extended, FLOAT / DOUBLE its bits).  n: count (count: matches; sum / avg: non-null arguments).
struct SgAggState {
  int64_t v;
  int64_t n;
  uint64_t m;     // scan elements of avg over INT / LONG: |carried value| + sum |x| so far, saturating; else 0
  uint32_t f;
  uint32_t pad;
};

__host__ __device__ __forceinline__ SgAggState sg_agg_empty() {
  SgAggState s;
  s.v = 0; s.n = 0; s.m = 0; s.f = 0; s.pad = 0;
  return s;
}

__host__ __device__ __forceinline__ bool sg_agg_is_fp(int t) { return t == SG_T_FLOAT || t == SG_T_DOUBLE; }

// argument bits (a record's value word) as the double `sum += data` / `value += data` adds
__host__ __device__ __forceinline__ double sg_agg_as_double(int atype, int64_t bits) {
  if (atype == SG_T_FLOAT) return (double)__uint_as_float((uint32_t)bits);
  if (atype == SG_T_DOUBLE) return __longlong_as_double(bits);
  return (double)bits;
}

__host__ __device__ __forceinline__ bool sg_agg_isnan(int atype, int64_t bits) {
  if (atype == SG_T_FLOAT) { float x = __uint_as_float((uint32_t)bits); return x != x; }
  if (atype == SG_T_DOUBLE) { double x = __longlong_as_double(bits); return x != x; }
  return false;
}

// a < b in the argument's type (false whenever either is a NaN)
__host__ __device__ __forceinline__ bool sg_agg_less(int atype, int64_t a, int64_t b) {
  if (atype == SG_T_FLOAT) return __uint_as_float((uint32_t)a) < __uint_as_float((uint32_t)b);
  if (atype == SG_T_DOUBLE) return __longlong_as_double(a) < __longlong_as_double(b);
  return a < b;
}

__host__ __device__ __forceinline__ int64_t sg_agg_nan_bits(int atype) {
  return atype == SG_T_FLOAT ? (int64_t)0x7fc00000ll : (int64_t)0x7ff8000000000000ll;
}

__host__ __device__ __forceinline__ uint64_t sg_agg_sat_add(uint64_t a, uint64_t b) {
  uint64_t c = a + b;
  return c < a ? ~0ull : c;
}

__host__ __device__ __forceinline__ uint64_t sg_agg_abs(int64_t x) { return x < 0 ? 0ull - (uint64_t)x : (uint64_t)x; }

// ---- the serial step: processAdd of one match on the group's state ------------------------------------------------
__host__ __device__ __forceinline__ void sg_agg_step(int kind, int atype, SgAggState& s, int64_t bits, int null) {
  switch (kind) {
    case SG_AGG_COUNT:
      s.n++;
      break;
    case SG_AGG_SUM:
      if (null) break;
      if (sg_agg_is_fp(atype)) s.v = __double_as_longlong(__longlong_as_double(s.v) + sg_agg_as_double(atype, bits));
      else s.v = (int64_t)((uint64_t)s.v + (uint64_t)bits);
      s.n++;
      s.f |= SG_AF_HAS;
      break;
    case SG_AGG_AVG:
      if (null) break;
      s.v = __double_as_longlong(__longlong_as_double(s.v) + sg_agg_as_double(atype, bits));
      s.n++;
      s.f |= SG_AF_HAS;
      break;
    case SG_AGG_MIN:
    case SG_AGG_MAX: {
      if (null) break;
      if (!(s.f & SG_AF_HAS)) {
        s.f |= SG_AF_HAS;
        if (sg_agg_isnan(atype, bits)) { s.f |= SG_AF_NANFIRST; break; }
      }
      if (sg_agg_isnan(atype, bits)) break;
      const bool better = kind == SG_AGG_MAX ? sg_agg_less(atype, s.v, bits) : sg_agg_less(atype, bits, s.v);
      if (!(s.f & SG_AF_EXT) || better) { s.v = bits; s.f |= SG_AF_EXT; }
      break;
    }
    default:
      break;
  }
}

// The aggregator's return value after a step (the output column): bits in the result type, or null.
__host__ __device__ __forceinline__ int64_t sg_agg_result(int kind, int atype, const SgAggState& s, int* null) {
  *null = 0;
  switch (kind) {
    case SG_AGG_COUNT:
      return s.n;
    case SG_AGG_SUM:
      if (!(s.f & SG_AF_HAS)) { *null = 1; return 0; }
      return s.v;
    case SG_AGG_AVG:
      if (!(s.f & SG_AF_HAS)) { *null = 1; return 0; }
      return __double_as_longlong(__longlong_as_double(s.v) / (double)s.n);
    case SG_AGG_MIN:
    case SG_AGG_MAX:
      if (!(s.f & SG_AF_HAS)) { *null = 1; return 0; }
      if (s.f & SG_AF_NANFIRST) return sg_agg_nan_bits(atype);
      return s.v;
    default:
      *null = 1;
      return 0;
  }
}

// ---- the scan's operator ------------------------------------------------------------------------------------------
// Which (kind, argument type) pairs the scan may take: everything but the double additions of FP sum / avg, whose
// order bit-exact parity fixes.  avg over INT / LONG is scanned as an exact integer sum while SG_AF_INEXACT stays
// clear (below).
__host__ __device__ __forceinline__ bool sg_agg_scannable(int kind, int atype) {
  return kind == SG_AGG_COUNT || kind == SG_AGG_MIN || kind == SG_AGG_MAX ||
         ((kind == SG_AGG_SUM || kind == SG_AGG_AVG) && !sg_agg_is_fp(atype));
}

// One match as a scan element.  In scan elements of avg over INT / LONG, v is the long sum and m the sum of |x|: while
// |carried value| + sum |x| < 2^53 every partial sum of every sub-range is an integer below 2^53, so the double
// additions of the serial step are all exact and equal the integer sum in any grouping.
__host__ __device__ __forceinline__ SgAggState sg_agg_lift(int kind, int atype, int64_t bits, int null) {
  SgAggState e = sg_agg_empty();
  if (kind == SG_AGG_AVG && !sg_agg_is_fp(atype)) {
    if (!null) {
      e.v = bits;
      e.n = 1;
      e.m = sg_agg_abs(bits);
      e.f = SG_AF_HAS | (e.m >= SG_AGG_2P53 ? SG_AF_INEXACT : 0u);
    }
    return e;
  }
  sg_agg_step(kind, atype, e, bits, null);
  return e;
}

// A group's carried state as the scan element in front of its run (avg over INT / LONG: the double value back to a
// long, exact below 2^53).
__host__ __device__ __forceinline__ SgAggState sg_agg_seed(int kind, int atype, const SgAggState& s) {
  SgAggState e = s;
  e.m = 0;
  if (kind == SG_AGG_AVG && !sg_agg_is_fp(atype)) {
    const double d = __longlong_as_double(s.v);
    const double a = d < 0 ? -d : d;
    if (a < 9007199254740992.0) {   // (false for NaN)
      e.v = (int64_t)d;
      e.m = (uint64_t)a;
    } else {
      e.v = 0;
      e.m = ~0ull;
      e.f |= SG_AF_INEXACT;
    }
  }
  return e;
}

// combine(a, b): a's matches, then b's.  Associative, not commutative (min / max keep the leftmost extreme).
//   min / max: the extreme of the non-NaN arguments, strict compare so the left one stays on a tie (0.0 / -0.0), a NaN
//   being the identity; NANFIRST comes from the leftmost side that has any argument, and makes the result a NaN.
__host__ __device__ __forceinline__ SgAggState sg_agg_combine(int kind, int atype, const SgAggState& a,
                                                              const SgAggState& b) {
  SgAggState o = a;
  switch (kind) {
    case SG_AGG_COUNT:
      o.n = a.n + b.n;
      break;
    case SG_AGG_SUM:
    case SG_AGG_AVG:
      o.v = (int64_t)((uint64_t)a.v + (uint64_t)b.v);
      o.n = a.n + b.n;
      o.m = sg_agg_sat_add(a.m, b.m);
      o.f = (a.f | b.f) & (SG_AF_HAS | SG_AF_INEXACT);
      if (kind == SG_AGG_AVG && o.m >= SG_AGG_2P53) o.f |= SG_AF_INEXACT;
      break;
    case SG_AGG_MIN:
    case SG_AGG_MAX: {
      uint32_t f = (a.f | b.f) & SG_AF_HAS;
      f |= ((a.f & SG_AF_HAS) ? a.f : b.f) & SG_AF_NANFIRST;
      if (!(a.f & SG_AF_EXT)) {
        o.v = b.v;
        f |= b.f & SG_AF_EXT;
      } else {
        f |= SG_AF_EXT;
        if (b.f & SG_AF_EXT) {
          const bool better = kind == SG_AGG_MAX ? sg_agg_less(atype, a.v, b.v) : sg_agg_less(atype, b.v, a.v);
          if (better) o.v = b.v;
        }
      }
      o.f = f;
      o.n = 0;
      o.m = 0;
      break;
    }
    default:
      break;
  }
  return o;
}

// A scan element back to the state the serial step would hold (avg over INT / LONG: the long sum as the double value;
// only valid while SG_AF_INEXACT is clear).
__host__ __device__ __forceinline__ SgAggState sg_agg_unseed(int kind, int atype, const SgAggState& e) {
  SgAggState s = e;
  s.m = 0;
  if (kind == SG_AGG_AVG && !sg_agg_is_fp(atype)) s.v = __double_as_longlong((double)e.v);
  s.f &= ~SG_AF_INEXACT;
  return s;
}

// Result types (each class's getReturnType): count LONG; sum LONG for INT / LONG, DOUBLE for FLOAT / DOUBLE; avg
// DOUBLE; min / max the argument's type.  -1: the aggregator does not take that type.
static inline int sg_agg_result_type(int kind, int atype) {
  if (kind == SG_AGG_COUNT) return SG_T_LONG;
  if (atype != SG_T_INT && atype != SG_T_LONG && atype != SG_T_FLOAT && atype != SG_T_DOUBLE) return -1;
  if (kind == SG_AGG_SUM) return sg_agg_is_fp(atype) ? SG_T_DOUBLE : SG_T_LONG;
  if (kind == SG_AGG_AVG) return SG_T_DOUBLE;
  if (kind == SG_AGG_MIN || kind == SG_AGG_MAX) return atype;
  return -1;
}
