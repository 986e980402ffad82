"""-m gpu: every search entry on rows and queries scaled by powers of two (tests/topk_magnitude.py; the inputs and the
restatements are proved on the CPU by tests/test_topk_magnitude.py). Every result is compared with topk_oracle.topk on the
SCALED data - ids, and scores by their uint32 view -, never with a kernel and never with ldexp.

PLAIN grid (every f32 quantity of the keep tests scales exactly): the measurement hook of the path re-scores exactly as many
pairs as on the unscaled case, and the wide hook reports fallback_armed == 0 - a library that sent everything to the exact
fallback would be exact and fail here. EXTREME grid (squares, scales or scores under- or overflow): only exactness; the pair
count and whether the fallback was armed are printed per point and path.

A library whose norms are f32 sums of squares (topk_magnitude.legacy) loses rows of the true top K from 2^-64 on - the table
in topk_magnitude.LEGACY_DROPS; the assertion messages name the queries."""
import numpy as np
import pytest

import coarse_tight as ct
import topk_magnitude as tm
from conftest import unit_rows

pytestmark = pytest.mark.gpu
f32 = np.float32
N_TIGHT = 70_001
E768_POINTS = tm.E768_POINTS


def pt_id(pt):
    return f"r{pt[0]:+d}q{pt[1]:+d}"


# ---- the exact scan ----------------------------------------------------------------------------------------------------------

_exact = {}


def exact_data(N, E):
    """Rows of norm U[0.1, 3], unit queries; per query j three planted rows 2.5 q_j, 1.5 q_j (both +inf where scores overflow:
    a tie) and -2 q_j (their partial sums are monotone: no inf - inf)."""
    if (N, E) not in _exact:
        rng = np.random.default_rng(N + E)
        db = (unit_rows(rng, N, E) * rng.uniform(0.1, 3.0, size=(N, 1))).astype(f32)
        q = unit_rows(rng, 5, E)
        for j in range(5):
            db[100 + 7 * j], db[N - 50 - 3 * j], db[N // 2 + j] = 2.5 * q[j], 1.5 * q[j], -2.0 * q[j]
        _exact[(N, E)] = (db, q)
    return _exact[(N, E)]


@pytest.mark.parametrize("pt", tm.GRID, ids=pt_id)
@pytest.mark.parametrize("E", (512, 768))
@pytest.mark.parametrize("N", (3_000, N_TIGHT))
def test_exact_scan_matches_the_oracle_at_any_magnitude(clipmi, gpu, topk_oracle, N, E, pt):
    db0, q0 = exact_data(N, E)
    with np.errstate(over="ignore", under="ignore"):
        db, q = (db0 * f32(2.0 ** pt[0])).astype(f32), (q0 * f32(2.0 ** pt[1])).astype(f32)
    So, Io = topk_oracle.topk(db, q, 51)
    idx = clipmi.IndexFlatIP(E, device=gpu)
    idx.add(db)
    D, I = idx.search(q, 51)
    sub = int((np.abs(So) < tm.FLT_MIN).sum())
    print(f"exact N={N} E={E} {pt_id(pt)}: {sub} subnormal or zero and {int(np.isinf(So).sum())} infinite scores of {So.size}")
    lost = np.flatnonzero((np.asarray(I) != Io).any(axis=1))
    assert lost.size == 0, f"queries {lost} differ from the oracle's ids: {np.asarray(I)[lost[0]][:8]} != {Io[lost[0]][:8]}"
    assert np.array_equal(np.asarray(D, f32).view(np.uint32), So.view(np.uint32))


# ---- the coarse paths --------------------------------------------------------------------------------------------------------

_held = {}          # one scaled index at a time: key -> (case, index, oracle scores, oracle ids)
_base_pairs = {}


def setup(clipmi, gpu, oracle, f, E, built, pt):
    key = (f, E, built, pt)
    if key not in _held:
        _held.clear()
        c = ct.case(f, E, N_TIGHT, built, oracle)
        if pt != (0, 0):
            c = tm.scaled(c, *pt)
        idx = clipmi.IndexFlatIP(E, device=gpu, coarse="bf16" if f == "B" else "int8", wide_768=True)
        idx.add(c.db)
        assert idx.uses_coarse()
        _held[key] = (c, idx) + oracle.topk(c.db, c.q, c.K)
    return _held[key]


def base_pairs(clipmi, gpu, oracle, f, E, built, Q):
    """Pairs the hook re-scores on the unscaled case (once per case, for every query count searched here)."""
    if (f, E, built, Q) not in _base_pairs:
        c, idx, _, _ = setup(clipmi, gpu, oracle, f, E, built, (0, 0))
        for n in (5, 64, 65, 130):
            if n <= built and (f != "B" or n == 64):
                _base_pairs[(f, E, built, n)] = ct.scan_hook(clipmi, gpu, idx, c.q[:n], c.K, "bf16" if f == "B" else "int8")[2]
    return _base_pairs[(f, E, built, Q)]


def check(clipmi, gpu, oracle, f, E, built, Q, pt):
    name = f"{f}-E{E}-Q{Q} {pt_id(pt)}"
    plain = pt in tm.PLAIN
    want = base_pairs(clipmi, gpu, oracle, f, E, built, Q) if plain else None
    c, idx, So, Io = setup(clipmi, gpu, oracle, f, E, built, pt)
    D, I = idx.search(c.q[:Q], c.K)
    lost = np.flatnonzero((np.asarray(I) != Io[:Q]).any(axis=1))
    assert lost.size == 0, f"{name}: search: queries {lost[:8]} (of {lost.size}) miss rows of the oracle's top K: " \
                           f"ids {np.asarray(I)[lost[0]]} != {Io[lost[0]]}"
    assert np.array_equal(np.asarray(D, f32).view(np.uint32), So[:Q].view(np.uint32)), name
    Dh, Ih, surv, armed = ct.scan_hook(clipmi, gpu, idx, c.q[:Q], c.K, "bf16" if f == "B" else "int8")
    print(f"{name}: {surv} re-scored pairs ({surv / Q:.0f} per query; every pair: {N_TIGHT}), fallback armed {armed}, "
          f"route by the table: {tm.ROUTE[(f, pt)]}")
    lost = np.flatnonzero((Ih != Io[:Q]).any(axis=1))
    assert lost.size == 0, f"{name}: hook: queries {lost[:8]} (of {lost.size}) miss rows of the oracle's top K"
    assert np.array_equal(Dh.view(np.uint32), So[:Q].view(np.uint32)), name
    # the literal table: a finite margin keeps the scan selective; no coarse bound means every pair (or, in the wide pass, whose
    # lists are shorter than the matrix, the exact fallback)
    if tm.ROUTE[(f, pt)] == "coarse":
        assert surv < Q * N_TIGHT and armed in (None, 0), f"{name}: the table says coarse"
    else:
        assert armed == 1 if Q > 64 else surv >= Q * N_TIGHT, f"{name}: the table says no coarse bound"
    if plain:
        assert surv == want, f"{name}: {surv} pairs re-scored, {want} on the unscaled case"
        assert 0 < surv / Q < N_TIGHT
        if Q > 64:
            assert armed == 0


INT8 = ([(f, 512, 65, Q, pt) for f in "RQ" for pt in tm.GRID for Q in (5, 64)]
        + [(f, 768, 130, Q, pt) for f in "RQ" for pt in E768_POINTS for Q in (5, 64)])
WIDE = ([(f, 512, 65, 65, pt) for f in "RQ" for pt in tm.GRID]
        + [(f, 768, 130, Q, pt) for f in "RQ" for pt in E768_POINTS for Q in (65, 130)])


def case_id(p):
    return f"{p[0]}-E{p[1]}-Q{p[3]}-{pt_id(p[4])}"


@pytest.mark.parametrize("p", INT8, ids=case_id)
def test_int8_64_query_pass_is_exact_at_any_magnitude(clipmi, gpu, topk_oracle, p):
    f, E, built, Q, pt = p
    check(clipmi, gpu, topk_oracle, f, E, built, Q, pt)


@pytest.mark.parametrize("p", WIDE, ids=case_id)
def test_int8_wide_pass_is_exact_at_any_magnitude(clipmi, gpu, topk_oracle, p):
    f, E, built, Q, pt = p
    check(clipmi, gpu, topk_oracle, f, E, built, Q, pt)


@pytest.mark.parametrize("pt", tm.GRID, ids=pt_id)
def test_bf16_coarse_is_exact_at_any_magnitude(clipmi, gpu, topk_oracle, pt):
    check(clipmi, gpu, topk_oracle, "B", 512, 64, 64, pt)


# ---- the build side ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("a", tm.ROW_EXPONENTS)
@pytest.mark.parametrize("E", (512, 768))
def test_error_norms_are_upper_bounds_at_any_magnitude(clipmi, gpu, E, a):
    """The device's own codes and scales against the f64 norm of what they leave (as test_quantize_rows_i8_matches_numpy reads
    the copy): every a_r, every block maximum, amax and rmax is an upper bound - and none is loose: within 0.2 % and two steps
    of the subnormal grid - or, where the literal table says so, search_device's guard leaves the coarse path."""
    import torch
    rng = np.random.default_rng(81)
    N = 1000
    x = (unit_rows(rng, N, E) * rng.uniform(0.1, 3.0, size=(N, 1))).astype(f32)
    x[7] = 0.0
    x[32:64] = 0.0
    x = (x * f32(2.0 ** a)).astype(f32)
    idx = clipmi.IndexFlatIP(E, device=gpu, coarse="int8")
    idx.add(x)
    q8, meta, amax, rmax = idx.matrix_i8()
    torch.cuda.synchronize()
    guard_keeps_coarse = bool(rmax > 0.0 and np.isfinite(rmax) and np.isfinite(amax))          # index.py search_device
    if tm.BUILD_SIDE[a] == "exact":
        assert not guard_keeps_coarse
        return
    assert guard_keeps_coarse
    N32 = (N + 31) // 32 * 32
    nblk = N32 // 32
    q8, meta = q8.cpu().numpy(), meta.cpu().numpy()
    rmeta = meta[:2 * (N32 + 32)].reshape(-1, 2)
    bmeta = meta[2 * (N32 + 32):2 * (N32 + 32) + 2 * (nblk + 1)].reshape(-1, 2)
    slot_rows = meta[2 * (N32 + 32) + 2 * (nblk + 1):].view(np.uint32)
    perm = np.argsort(np.abs(x).max(axis=1), kind="stable")
    assert np.array_equal(slot_rows[:N], perm.astype(np.uint32))
    xp = np.zeros((N32, E), np.float64)
    xp[:N] = x[perm]
    got = q8.reshape(nblk, E // 32, 2, 32, 16).transpose(0, 3, 1, 2, 4).reshape(N32, E).astype(np.float64)
    s = rmeta[:N32, 0].astype(np.float64)
    assert np.isfinite(s).all() and (s > 0).all() and np.array_equal(rmeta[:N32, 0], np.repeat(bmeta[:nblk, 0], 32))
    err = np.linalg.norm(xp - s[:, None] * got, axis=1)
    a_r = rmeta[:N32, 1].astype(np.float64)
    print(f"E={E} rows x 2^{a}: scales {s.min():.3g} .. {s.max():.3g}, a_r / ||x - s q|| up to {np.max(a_r[err > 0] / err[err > 0]):.6f}, "
          f"blocks with zero codes {int((np.abs(got).reshape(nblk, -1).max(axis=1) == 0).sum())} of {nblk}")
    assert (a_r >= err).all(), f"slots {np.flatnonzero(a_r < err)[:8]}: a_r below the f64 error norm"
    assert (a_r <= err * 1.002 + 2.0 ** -148).all()
    blk = bmeta[:nblk, 1].astype(np.float64)
    assert (blk >= err.reshape(nblk, 32).max(axis=1)).all() and np.array_equal(bmeta[:nblk, 1], rmeta[:N32, 1].reshape(nblk, 32).max(axis=1))
    norm = np.linalg.norm(x.astype(np.float64), axis=1).max()
    assert amax >= a_r.max() and norm <= rmax <= norm * 1.00001 + 2.0 ** -148
