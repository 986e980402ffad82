"""-m gpu: the adversarial cases of tests/coarse_tight.py through the device. tests/test_coarse_tight.py proves on the CPU
that every query of every case has a row of its true top K within a few per cent of the bound term its family presses, in
every segment of the scan, and that a term lost, understated by 1 % or read from a neighbour drops such a row. Here each case
goes through the product's own route, IndexFlatIP(E, coarse=..., wide_768=True).search, and once through the measurement hook
of its path: ids and scores are the oracle's bits, the index reports the coarse route, and the exact fallback - which would
hide a dropped row - did not answer (the wide hook reports fallback_armed == 0; the 64-query hooks re-score fewer than 2^18
pairs per query, a list's capacity and the only way into the fallback, as
test_topk_gpu.py::test_coarse_anisotropic_db_exact_and_survivors has it).

Queries beyond the first 64 of a case repeat its construction with other sign vectors; a search of the first Q queries of a
case is a case (a query's fences and targets do not depend on the others)."""
import numpy as np
import pytest

import coarse_tight as ct
from test_coarse_tight import BF16_CASES, INT8_CASES

pytestmark = pytest.mark.gpu

BUILT = {(f, E, N): Q for f, E, N, Q in INT8_CASES + BF16_CASES}           # queries each case is built (and proved) with

# (kernel the search reaches, family, E, rows, Q)
CASES = (
    [("scan_coarse", f, E, 70_001, Q) for f in ("R", "Q", "B") for E in (512, 768) for Q in (5, 17, 64)]
    + [("wide<8>", f, 512, 70_001, Q) for f in ("R", "Q") for Q in (65, 191)]
    + [("wide2<4,2>", f, 512, 70_001, Q) for f in ("R", "Q") for Q in (192, 513)]
    + [("wide<4,0,24>", f, 768, 70_001, Q) for f in ("R", "Q") for Q in (65, 130)]
    # three segments of the 64-query passes (int8 and bf16), two of the wide pass
    + [("scan_coarse", "R", 512, 200_003, 64), ("scan_coarse", "B", 512, 200_003, 64), ("wide<8>", "R", 512, 200_003, 65)]
)


def case_id(c):
    return f"{c[0]}-{c[1]}-E{c[2]}-N{c[3]}-Q{c[4]}"


_index, _ref = {}, {}


def setup(clipmi, gpu, topk_oracle, f, E, N):
    """Per (family, E, rows), once: the case, its index and the oracle's answer for all of its queries."""
    key = (f, E, N)
    if key not in _index:
        c = ct.case(f, E, N, BUILT[key], topk_oracle)
        idx = clipmi.IndexFlatIP(E, device=gpu, coarse="bf16" if f == "B" else "int8", wide_768=True)
        idx.add(c.db)
        assert idx.uses_coarse()
        _index[key] = (c, idx)
        _ref[key] = topk_oracle.topk(c.db, c.q, c.K)
    return _index[key] + _ref[key]


@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_tight_case_is_exact_on_the_coarse_route_without_the_fallback(clipmi, gpu, topk_oracle, case):
    _, f, E, N, Q = case
    c, idx, So, Io = setup(clipmi, gpu, topk_oracle, f, E, N)
    assert np.array_equal(np.sort(Io[:Q], axis=1), np.sort(c.targets[:Q], axis=1))      # the oracle's top K are the targets
    D, I = idx.search(c.q[:Q], c.K)
    assert idx.uses_coarse()
    lost = np.flatnonzero((np.asarray(I) != Io[:Q]).any(axis=1))
    assert lost.size == 0, f"{case_id(case)}: search: queries {lost[:8]} (of {lost.size}) miss rows of the oracle's top K"
    assert np.array_equal(np.asarray(D, np.float32).view(np.uint32), So[:Q].view(np.uint32))
    Dh, Ih, surv, armed = ct.scan_hook(clipmi, gpu, idx, c.q[:Q], c.K, "bf16" if f == "B" else "int8")
    print(f"{case_id(case)}: {surv / Q:.0f} re-scored pairs per query, fallback armed {armed}")
    lost = np.flatnonzero((Ih != Io[:Q]).any(axis=1))
    assert lost.size == 0, f"{case_id(case)}: hook: queries {lost[:8]} (of {lost.size}) miss rows of the oracle's top K"
    assert np.array_equal(Dh.view(np.uint32), So[:Q].view(np.uint32))
    if Q > 64:
        assert armed == 0
    else:
        assert 0 < surv / Q < (1 << 18)
