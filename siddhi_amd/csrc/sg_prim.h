// rocPRIM device primitives on a handle's stream: each wrapper asks for the temporary storage size, takes that much
// from the named grow-only workspace buffer and runs the primitive.  Arguments are forwarded by value, so a call
// instantiates exactly the rocPRIM kernels the spelled-out three-line form did.
#pragma once
#include <rocprim/rocprim.hpp>

#include "sg_engine.h"

// run(tmp, bytes) is the primitive: called with tmp == nullptr it only reports the bytes it needs
template <class Run>
static void sg_with_tmp(Workspace& ws, hipStream_t st, const std::string& tmp_name, Run run) {
  size_t tb = 0;
  HIPCHK(run(nullptr, tb));
  void* tmp = ws.get(tmp_name, tb, st);
  HIPCHK(run(tmp, tb));
}

template <class In, class Out, class Init, class Op>
static void sg_exclusive_scan(Workspace& ws, hipStream_t st, const std::string& tmp_name, In in, Out out, Init init,
                              size_t n, Op op) {
  sg_with_tmp(ws, st, tmp_name, [&](void* t, size_t& tb) { return rocprim::exclusive_scan(t, tb, in, out, init, n, op, st); });
}

template <class In, class Out, class Op>
static void sg_inclusive_scan(Workspace& ws, hipStream_t st, const std::string& tmp_name, In in, Out out, size_t n, Op op) {
  sg_with_tmp(ws, st, tmp_name, [&](void* t, size_t& tb) { return rocprim::inclusive_scan(t, tb, in, out, n, op, st); });
}

template <class In, class Out, class Init, class Op>
static void sg_reduce(Workspace& ws, hipStream_t st, const std::string& tmp_name, In in, Out out, Init init, size_t n,
                      Op op) {
  sg_with_tmp(ws, st, tmp_name, [&](void* t, size_t& tb) { return rocprim::reduce(t, tb, in, out, init, n, op, st); });
}

// stable sort of (key, value) pairs by key bits [0, end_bit)
template <class KI, class KO, class VI, class VO>
static void sg_radix_sort_pairs(Workspace& ws, hipStream_t st, const std::string& tmp_name, KI k_in, KO k_out, VI v_in,
                                VO v_out, size_t n, unsigned end_bit) {
  sg_with_tmp(ws, st, tmp_name, [&](void* t, size_t& tb) {
    return rocprim::radix_sort_pairs(t, tb, k_in, k_out, v_in, v_out, n, 0, end_bit, st);
  });
}
