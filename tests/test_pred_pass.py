"""Filter constants on rounding edges through the predicate kernels of csrc/pred.h, on the GPU.

One engine per query, pushed as consecutive batches of 1, 3, 4, 255, 256, 257, 1023, 1024, 1025 and 4,099 rows (a lane
takes 4 rows, a tile 256, a wave 1,024, a block 4,096: the full-tile loads and every tail), with and without nulls, and
(one stream) with the stream column absent and present.  Constants of every type against an INT and a FLOAT column,
each where the compare domain decides the answer (value_cases.CONSTANTS), the six operators:

  P1  every e1=S[v OP c] -> e2=S                 the general family's local_pred_pass; exactly (i, i + 1) per passing row
  P2  every e1=S[v OP c] -> e2=S[v >= e1.v]      the closed form's pred_pass, the filter on the compared column
  P3  every e1=A[price OP c] -> e2=B[price > e1.price]          two streams, nulls in A's price only
  P4  e1=A[price OP c] -> e2=B[price > e1.price], partitioned   the once route's pass, nulls in A's price only: a null
      price passes `!=` and binds e1, which then never completes and holds its key
  depth  right-nested and / or filters whose program depth picks k_pred<2>, <4>, <8> and <16>

Which kernel a run reaches, read off launch_pred (all three are timed as "pred", so the test cannot see it; the
16-byte alignment they ask for holds: api.hip's upload copies every column of a host push to the start of a buffer):

  k_pred_simple     no stream column and `col OP const` with the column on the left: P1 with and without nulls (the null
                    array is passed, a null row passes `!=`), depth-1 (`w > 300`), P2 without nulls
  k_pred_simple_s   a stream column, a FLOAT column, B's compared column without a null array: P3 and P4 with nulls
                    (the null array is A's price: a null row is no candidate in P3, passes `!=` in P4) and without,
                    and P2 on a FLOAT column with a stream column and no nulls
  k_pred<D>         everything else: the constant on the left, P1 and the depth cases with a stream column, P2 with
                    nulls (the compared column's nulls make B's consumers a mask of their own) or on an INT column with
                    a stream column

k_pred_simple with a null array whose nulls are not candidates cannot be reached: on one stream A and B compare one
column, whose nulls send the closed form to k_pred<D>.

All outputs equal the oracle's bit for bit and the row-at-a-time reference's (trigger, e1.id, e2.id)."""
import pytest

import value_cases as V
from oracle import OracleEngine
from parity_util import assert_same, run_engine

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", V.PRED + V.DEPTH, ids=str)
def test_pred_pass(case):
    for c in (case, V.without_nulls(case)):
        want = run_engine(OracleEngine, c.app, V.pushes(c))
        ref = V.reference(c)
        assert V.triples(want) == ref
        for stream_column in (True, False) if c.streams == 1 else (True,):
            got, log = V.run_gpu(c, stream_column)
            where = f"{c.name}, {'with a' if stream_column else 'no'} stream column"
            assert len(log) == len(V.PRED_SIZES) and all("pred" in push for push, _ in log), where
            assert len(got) == len(want), (where, len(got), len(want))
            assert V.triples(got) == ref, where
            assert_same(got, want)
