"""The scaled cases of tests/topk_magnitude.py, proved on the CPU: conditions on the INPUTS that
tests/test_topk_magnitude_gpu.py runs through the device, and on the restatements (no kernel runs here).

PLAIN grid: the oracle's top 2K ids are the base case's and its scores are bitwise ldexp(base, a + b); every f32 intermediate
of the `current` restatement is finite and normal (or exactly zero: a spacer's a_r and family R's ||f_q|| are 0 at every scale);
the keep test's verdicts are the base case's.
EXTREME grid, one exponent 0 and the other <= -64 (scores stay normal, only squares underflow): the oracle's top K is still
the targets, and the `legacy` restatement - f32 sums of squares - drops a pair of the true top K as topk_magnitude.LEGACY_DROPS
has it: what the device test would show on a library that computes its norms that way.
Every grid point: the bound in real numbers (f64, true norms, with the absolute term E 2^-149 for roundings on the subnormal
grid) holds for every row of the oracle's top K wherever the scores are finite, and `current` does what the literal table
topk_magnitude.ROUTE says: a finite margin for every query and every such row passes, or margin +inf for every query."""
import numpy as np
import pytest

import coarse_tight as ct
import topk_magnitude as tm

f32 = np.float32
CASES = [("R", 512, 70_001, 65), ("Q", 512, 70_001, 65), ("R", 768, 70_001, 65), ("Q", 768, 70_001, 65), ("B", 512, 70_001, 64)]
PATHS = {"R": ("i8-64", "i8-wide"), "Q": ("i8-64", "i8-wide"), "B": ("bf16",)}

_base = {}


def ids(specs):
    return [f"{f}-E{E}-N{N}-Q{Q}" for f, E, N, Q in specs]


def pt_id(pt):
    return f"r{pt[0]:+d}q{pt[1]:+d}"


def proof(c, oracle, form, rows, taus=True):
    """The restatement of every path of the case's family on the pairs (query i, rows[i]): {path: pairs dict}, with the copy
    and the query constants under "cp" / "qm". taus=False: thresholds from zeros (where only the margins are asked for -
    a margin of +inf makes the threshold -inf whatever tau is - and a product of subnormals would take a minute)."""
    ex = ct.exact_scores(c.db, c.q, c.special, oracle) if taus else np.zeros((c.N, c.Q), f32)
    out = {}
    if c.family == "B":
        cp = ct.Bf16Copy(c.db)
        b = ct.coarse_segments(c.N, c.K)
        out["bf16"] = ct.bf16_pairs(cp, c.q, c.K, ct.running_taus(ex, c.K, b, cp.slot_row), b, rows, form=form)
        out["cp"], out["qm"] = cp, None
    else:
        cp, qm = ct.I8Copy(c.db, form), ct.I8Queries(c.q, form)
        for path, b in (("i8-64", ct.coarse_segments(c.N, c.K)), ("i8-wide", ct.wide_segments(c.N))):
            out[path] = ct.i8_pairs(cp, qm, c.q, c.K, ct.running_taus(ex, c.K, b, cp.slot_row), b, rows, path == "i8-wide")
        out["cp"], out["qm"] = cp, qm
    return out


def base(spec, oracle):
    if spec not in _base:
        c = ct.case(*spec, oracle)
        S, I = oracle.topk(c.db, c.q, 2 * c.K)
        _base[spec] = (c, S, I, proof(c, oracle, tm.current, c.targets))
    return _base[spec]


def normal_or_zero(v):
    v = np.asarray(v)
    return bool((np.isfinite(v) & ((v == 0) | (np.abs(v) >= tm.FLT_MIN))).all())


@pytest.mark.parametrize("pt", tm.PLAIN, ids=pt_id)
@pytest.mark.parametrize("spec", CASES, ids=ids(CASES))
def test_plain_grid_scales_every_quantity_exactly(topk_oracle, spec, pt):
    c0, S0, I0, p0 = base(spec, topk_oracle)
    c = tm.scaled(c0, *pt)
    S, I = topk_oracle.topk(c.db, c.q, 2 * c.K)
    assert np.array_equal(I, I0)
    assert np.array_equal(S.view(np.uint32), np.ldexp(S0, pt[0] + pt[1]).astype(f32).view(np.uint32))
    p = proof(c, topk_oracle, tm.current, c.targets)
    cp, qm = p["cp"], p["qm"]
    for path in PATHS[c.family]:
        r = p[path]
        assert np.array_equal(r["passed"], p0[path]["passed"]) and r["passed"].all(), path
        for name in ("lhs", "thr", "margin"):
            assert normal_or_zero(r[name]), (path, name)
        assert (r["margin"] > 0).all()
    assert normal_or_zero(cp.rmax) and cp.rmax > 0
    if qm is not None:
        for name, v in (("t", qm.t), ("inv", qm.inv), ("Y", qm.Y), ("F", qm.F), ("a_r", cp.a), ("s", cp.s), ("amax", cp.amax)):
            assert normal_or_zero(v), name
        assert (qm.t > 0).all() and (qm.Y > 0).all() and (cp.s > 0).all()
        # ... and they ARE the base case's, scaled
        q0, c0p = p0["qm"], p0["cp"]
        assert np.array_equal(qm.Y, np.ldexp(q0.Y, pt[1])) and np.array_equal(qm.F, np.ldexp(q0.F, pt[1]))
        assert np.array_equal(cp.a, np.ldexp(c0p.a, pt[0])) and np.array_equal(cp.q8, c0p.q8) and np.array_equal(qm.p, q0.p)


def one_sided_small(pt):
    return (pt[0] == 0 and pt[1] <= -64) or (pt[1] == 0 and pt[0] <= -64)


SMALL = [pt for pt in tm.EXTREME if one_sided_small(pt)]


@pytest.mark.parametrize("pt", SMALL, ids=pt_id)
@pytest.mark.parametrize("spec", CASES, ids=ids(CASES))
def test_squares_underflow_and_the_legacy_norms_drop_true_pairs(topk_oracle, spec, pt):
    c0, S0, I0, _ = base(spec, topk_oracle)
    c = tm.scaled(c0, *pt)
    _, I = topk_oracle.topk(c.db, c.q, c.K)
    assert np.array_equal(np.sort(I, axis=1), np.sort(c.targets, axis=1))          # the oracle's top K is still the targets
    operand, e = ("queries", pt[1]) if pt[0] == 0 else ("rows", pt[0])
    claim = tm.LEGACY_DROPS.get((c.family, operand), {}).get(e)
    p = proof(c, topk_oracle, tm.legacy, c.targets)
    for path in PATHS[c.family]:
        dropped = ~p[path]["passed"].all(axis=1)
        print(f"{ids([spec])[0]} {pt_id(pt)} {path}: legacy norms drop a true top-K pair for {int(dropped.sum())} of {c.Q} queries"
              f" (claimed: {claim})")
        if claim == "all":
            assert dropped.all(), path
        elif claim == "some":
            assert dropped.any(), path


def real_bound_holds(c, p, S, I):
    """The superset bound in real numbers for the pairs (query i, I[i]) with finite scores S: f64, true norms of the copy
    `current` makes, gamma_E = E u / (1 - E u) for the score's fmaf chain and E 2^-149 for its roundings on the subnormal grid."""
    E = c.E
    q = c.q.astype(np.float64)
    x = c.db[I].astype(np.float64)                                           # [Q][K][E]
    Y = np.linalg.norm(q, axis=1)
    R = np.linalg.norm(c.db.astype(np.float64), axis=1).max()
    gam = E * ct.U24 / (1 - E * ct.U24)
    absterm = E * 2.0 ** -149
    fin = np.isfinite(S)
    if c.family == "B":
        xh, qh = ct.bf16_round(c.db[I]).astype(np.float64), ct.bf16_round(c.q).astype(np.float64)
        coarse = np.einsum("qke,qe->qk", xh, qh)
        u8 = 2.0 ** -8
        # a bf16 below 2^-126 keeps fewer bits: its rounding is absolute, half a step of the bf16 subnormal grid (2^-134)
        slack = (2 * u8 + u8 * u8 + gam) * R * Y[:, None] + absterm + 2.0 ** -134 * (np.abs(q).sum(axis=1)[:, None] + np.abs(x).sum(axis=2)) * 1.01
        ok = coarse + slack >= S
    else:
        cp, qm = p["cp"], p["qm"]
        slots = cp.row_slot[I]
        sq = cp.srow[slots].astype(np.float64)[:, :, None] * cp.q8[slots].astype(np.float64)     # s_r q_r
        a = np.linalg.norm(x - sq, axis=2)
        t = qm.t.astype(np.float64)
        f = q - t[:, None] * qm.p.astype(np.float64)
        D = np.einsum("qke,qe->qk", cp.q8[slots].astype(np.float64), qm.p.astype(np.float64))
        A = np.linalg.norm(c.db[cp.perm].astype(np.float64) - cp.srow[:c.N].astype(np.float64)[:, None] * cp.q8[:c.N], axis=1).max()
        lhs = cp.srow[slots].astype(np.float64) * t[:, None] * D + a * Y[:, None]
        ok = lhs + (R + A) * np.linalg.norm(f, axis=1)[:, None] + gam * R * Y[:, None] + absterm >= S
    return bool(ok[fin].all()), bool(fin.all())


SUBNORMAL_SCORES = ((-60, -60), (-75, -75), (-126, 60))


@pytest.mark.parametrize("pt", tm.EVERY_POINT, ids=pt_id)
@pytest.mark.parametrize("spec", CASES, ids=ids(CASES))
def test_every_point_has_a_valid_bound_or_none(topk_oracle, spec, pt):
    c0, _, _, _ = base(spec, topk_oracle)
    c = tm.scaled(c0, *pt)
    if pt in SUBNORMAL_SCORES:                   # the first 16 queries (a case of its own): a host's fmaf on subnormals can be 100 x slower
        c.q, c.Q, c.targets, c.fences = c.q[:16], 16, c.targets[:16], c.fences[:16]
    S, I = topk_oracle.topk(c.db, c.q, c.K)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        p = proof(c, topk_oracle, tm.current, I, taus=tm.ROUTE[(c.family, pt)] == "coarse")
        holds, finite = real_bound_holds(c, p, S, I)
    assert holds, "the bound in real numbers, with its absolute term, misses a row of the oracle's top K"
    route = tm.ROUTE[(c.family, pt)]
    for path in PATHS[c.family]:
        m = p[path]["margin"]
        if route == "coarse":
            assert finite and np.isfinite(m).all(), f"{path}: queries {np.flatnonzero(~np.isfinite(m))[:8]} have no bound"
            assert p[path]["passed"].all(), f"{path}: `current` drops a row of the oracle's top K"
        else:
            assert np.isposinf(m).all(), f"{path}: queries {np.flatnonzero(np.isfinite(m))[:8]} keep a finite margin"
            assert p[path]["passed"].all()                                        # a threshold of -inf passes everything
    print(f"{ids([spec])[0]} {pt_id(pt)}: {route}; scores finite: {finite}")
