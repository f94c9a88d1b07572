"""The select / having pass (sg_math, sg_cmp over output columns, k_select, k_having_scatter) on the GPU, behind every
route, at the edge values of select_ref.py: the pair sweep's expression groups on the tiled walker, the unpartitioned
search and walker, the per-key machine and the once route; the `having` cases; the compaction cases; 32 outputs over 32
base slots; programs of exactly the VM's depth; and expression twins on the absence closed form and both lane routes.

Values are compared with the reference restatement (nulls agree, NaN equals NaN of its width, all else bit for bit),
trigger / ts / key / group with the oracle on the same query, exactly; the route is read off the kernels the handle timed.
test_select_cases.py guards the cases themselves on the CPU."""
import pytest

import select_ref as S
from parity_util import context
from siddhi_amd import lowering as L

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", S.ALL, ids=str)
def test_select_values(case):
    got, log = S.run_gpu(case)
    print(case.name, log)
    S.check(case, got, "gpu")
    S.assert_where(got, S.oracle(case), f"gpu against the oracle, {case.name}")
    S.check_route(case, log)


@pytest.mark.parametrize("clause", ["select", "having", "filter"])
def test_sg_open_refuses_depth_17(clause, monkeypatch):
    """a descriptor the lowering would not make: sg_open refuses it before anything is launched (no push here)"""
    from siddhi_amd._native import SG_EUNSUPPORTED, GpuEngine, SgError
    case = {c.name.split("-")[1]: c for c in S.depth_cases(17)}[clause]
    monkeypatch.setattr(L, "VM_STACK", 64)
    with pytest.raises(SgError) as e:
        GpuEngine(context(case.app()))
    assert e.value.code == SG_EUNSUPPORTED and "deeper than the VM stack" in str(e.value)
