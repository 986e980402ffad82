"""The adversarial cases of tests/coarse_tight.py, proved on the CPU: conditions on the INPUTS that
tests/test_coarse_tight_gpu.py runs through the device, and on the restatements it relies on.

For every case: the oracle's top K of every query is exactly its targets (2K distinct f32 scores, targets above fences);
in the unmutated restatement every target passes in its segment; every query has a target with room <= 0.1 x the term its
family presses; every segment of the path's plan holds such a target; and each mutant of the restatement - a term of the
bound lost or taken from a neighbour - drops a pair of the true top K for every query. (The neighbour mutants are monotone:
a larger ||y||, ||f_q|| or t_q only loosens the test. They must drop a pair for every query that HAS a neighbour, one to
either side, with a smaller value - three in four, the scales being 2^-(q % 4).)

bf16 (family B): red on the coefficient 0.0041 the header derived from a rounding unit of 2^-9, green on 0.0080."""
import numpy as np
import pytest

import coarse_tight as ct
from conftest import unit_rows

# (family, E, N, queries built) - what tests/test_coarse_tight_gpu.py searches, whole or the first Q' queries of
INT8_CASES = [("R", 512, 70_001, 513), ("Q", 512, 70_001, 513), ("R", 768, 70_001, 130), ("Q", 768, 70_001, 130),
              ("R", 512, 200_003, 65)]
BF16_CASES = [("B", 512, 70_001, 64), ("B", 768, 70_001, 64), ("B", 512, 200_003, 64)]
CAP = 0.1

_proof = {}


def proof(c, topk_oracle):
    """Per case, once: the exact score matrix, and per path the copy, thresholds and the unmutated pairs."""
    key = (c.family, c.E, c.N, c.Q)
    if key not in _proof:
        ex = ct.exact_scores(c.db, c.q, c.special, topk_oracle)
        p = {"exact": ex, "paths": {}}
        if c.family == "B":
            cp = ct.Bf16Copy(c.db)
            b = ct.coarse_segments(c.N, c.K)
            p["paths"]["bf16"] = (cp, None, b, ct.running_taus(ex, c.K, b, cp.slot_row))
        else:
            cp, qm = ct.I8Copy(c.db), ct.I8Queries(c.q)
            for name, b in (("i8-64", ct.coarse_segments(c.N, c.K)), ("i8-wide", ct.wide_segments(c.N))):
                p["paths"][name] = (cp, qm, b, ct.running_taus(ex, c.K, b, cp.slot_row))
        _proof[key] = p
    return _proof[key]


def pairs(c, path, pr, mut=None, nb=1):
    cp, qm, b, taus = pr["paths"][path]
    if path == "bf16":
        return ct.bf16_pairs(cp, c.q, c.K, taus, b, c.targets, mut)
    return ct.i8_pairs(cp, qm, c.q, c.K, taus, b, c.targets, path == "i8-wide", mut, nb)


def ids(cases):
    return [f"{f}-E{E}-N{N}-Q{Q}" for f, E, N, Q in cases]


@pytest.mark.parametrize("spec", INT8_CASES + BF16_CASES, ids=ids(INT8_CASES + BF16_CASES))
def test_inputs_are_what_they_claim(topk_oracle, spec):
    c = ct.case(*spec, topk_oracle)
    S, I = topk_oracle.topk(c.db, c.q, 2 * c.K)
    for i in range(c.Q):
        assert np.array_equal(I[i, :c.K], c.targets[i][::-1]), i                 # best first; targets were built ascending
        assert np.array_equal(I[i, c.K:], c.fences[i][::-1]), i
        assert np.all(np.diff(S[i]) < 0), i                                       # 2K distinct scores
    rel = (S[:, c.K - 1] - S[:, c.K]) / S[:, c.K]
    assert rel.max() < 2e-6 and (S[:, 0] - S[:, -1] < 1e-5 * S[:, 0]).all()
    assert (c.fences < ct.S1).all()                                               # the fences are in the sample
    # every filler lies below half of the K-th best: its f32-product score in `exact_scores` cannot matter
    ex = proof(c, topk_oracle)["exact"]
    fill = np.ones(c.N, bool)
    fill[c.special] = False
    assert (ex[fill].max(axis=0) < 0.5 * S[:, -1]).all()
    norms = np.linalg.norm(c.db.astype(np.float64), axis=1)
    if c.family in ("Q", "B"):                                                    # the targets carry the largest norm
        assert norms[c.targets].min() > 0.998 * norms.max()     # the groups' spikes differ: 0.1 %
        assert norms[fill].max() < 0.9 * norms.max() and norms[fill].std() > 0.2 * norms[fill].mean()


def tight_check(c, path, pr):
    r = pairs(c, path, pr)
    term = r["term_row"] if c.family == "R" else r["term_q"]
    ratio = r["room"] / term
    assert r["passed"].all(), f"{path}: a target fails the unmutated test"
    assert (r["room"] > 0).all()
    tight = ratio <= CAP
    assert tight.any(axis=1).all(), f"{path}: a query without a tight target (largest of the per-query minima {ratio.min(axis=1).max():.4f})"
    nseg = len(pr["paths"][path][2])
    assert set(np.unique(r["seg"][tight])) == set(range(nseg)), f"{path}: tight targets in segments {np.unique(r['seg'][tight])} of {nseg}"
    print(f"{c.family} E={c.E} N={c.N} Q={c.Q} {path}: room/term per query: smallest {ratio.min():.4f}, "
          f"largest of the per-query minima {ratio.min(axis=1).max():.4f}, over all targets {ratio.max():.4f}; {nseg} segments")
    return r


def has_smaller_neighbour(c):
    pw = 2.0 ** -(np.arange(c.Q) % 4)
    return (np.roll(pw, -1) < pw) | (np.roll(pw, 1) < pw)


def mutants_check(c, path, pr, muts):
    """Runs the mutants of `muts` that the case's family presses; returns them (test_every_listed_mutant_runs holds every list
    to its cases: no listed mutant is skipped everywhere)."""
    ran = [mut for mut in muts if c.family in ct.PRESSED_BY[mut]]
    for mut in ran:
        if mut.endswith("_nb"):
            dropped = np.zeros(c.Q, bool)
            for nb in (1, -1):
                dropped |= ~pairs(c, path, pr, mut, nb)["passed"].all(axis=1)
            want = has_smaller_neighbour(c)
            assert want.sum() >= 0.7 * c.Q
            assert dropped[want].all(), f"{path}: mutant {mut} drops nothing for queries {np.flatnonzero(want & ~dropped)[:8]}"
        else:
            dropped = ~pairs(c, path, pr, mut)["passed"].all(axis=1)
            assert dropped.all(), f"{path}: mutant {mut} drops nothing for queries {np.flatnonzero(~dropped)[:8]}"
    return ran


def test_every_listed_mutant_runs():
    """Every mutant of every list is pressed by the family of at least one case that list is checked on, and every family
    named in PRESSED_BY has such a case: a listed mutant cannot silently not run."""
    for muts, cases in ((ct.I8_MUTANTS_64, INT8_CASES), (ct.I8_MUTANTS_WIDE, INT8_CASES), (ct.BF16_MUTANTS, BF16_CASES)):
        fams = {spec[0] for spec in cases}
        for mut in muts:
            assert ct.PRESSED_BY[mut] & fams, f"mutant {mut} runs on none of {sorted(fams)}"
    listed = set(ct.I8_MUTANTS_64) | set(ct.I8_MUTANTS_WIDE) | set(ct.BF16_MUTANTS)
    assert listed == set(ct.PRESSED_BY)
    for mut, fams in ct.PRESSED_BY.items():
        for f in fams:
            lists = [m for m, cases in ((ct.I8_MUTANTS_64 + ct.I8_MUTANTS_WIDE, INT8_CASES), (ct.BF16_MUTANTS, BF16_CASES))
                     if f in {spec[0] for spec in cases}]
            assert any(mut in m for m in lists), f"mutant {mut} is never run on family {f}"


@pytest.mark.parametrize("spec", INT8_CASES, ids=ids(INT8_CASES))
def test_int8_cases_are_tight_and_every_mutant_drops_a_true_pair(topk_oracle, spec):
    c = ct.case(*spec, topk_oracle)
    pr = proof(c, topk_oracle)
    for path, muts in (("i8-64", ct.I8_MUTANTS_64), ("i8-wide", ct.I8_MUTANTS_WIDE)):
        tight_check(c, path, pr)
        ran = mutants_check(c, path, pr, muts)
        assert set(ran) == {m for m in muts if c.family in ct.PRESSED_BY[m]} and len(ran) >= 3


@pytest.mark.parametrize("spec", BF16_CASES, ids=ids(BF16_CASES))
def test_bf16_case_is_red_on_the_old_coefficient_and_tight_on_the_new(topk_oracle, spec):
    c = ct.case(*spec, topk_oracle)
    pr = proof(c, topk_oracle)
    r = tight_check(c, "bf16", pr)
    # the reference stays inside the corrected bound: |s - c| <= (2 u8 + u8^2 + 2 E u) ||x|| ||q|| for every target
    cp = pr["paths"]["bf16"][0]
    s = pr["exact"][c.targets, np.arange(c.Q)[:, None]].astype(np.float64)
    coarse = np.einsum("qke,qe->qk", cp.dbh[c.targets].astype(np.float64), ct.bf16_round(c.q).astype(np.float64))
    nn = np.linalg.norm(c.db[c.targets].astype(np.float64), axis=2) * np.linalg.norm(c.q.astype(np.float64), axis=1)[:, None]
    loss = (s - coarse) / nn
    need = 2 * 2.0 ** -8 + 2.0 ** -16 + 2 * c.E * 2.0 ** -24
    print(f"B E={c.E}: (s - c) / (|x||q|) up to {loss.max():.6f}; needed coefficient {need:.7f}, taken {float(ct.bf16_coef(c.E)):.7f}, "
          f"before {float(ct.bf16_coef(c.E, old=True)):.7f}")
    assert 0.0076 < loss.min() and loss.max() <= need < float(ct.bf16_coef(c.E))
    assert r["seg"].max() == len(pr["paths"]["bf16"][2]) - 1
    assert mutants_check(c, "bf16", pr, ct.BF16_MUTANTS) == list(ct.BF16_MUTANTS)      # family B presses both: none skipped
    old = pairs(c, "bf16", pr, "coef_old")
    assert not old["passed"].any(), "every target is lost on the old coefficient"


def test_the_restatements_agree_with_the_suites_own_on_unit_rows(topk_oracle):
    """The three forms of the int8 restatement agree on unit rows (N = 70 001, E = 512, Q = 16, K = 51, seed 4242): the
    whole-matrix form that tests/test_topk_e768.py::_int8_bound_survivors and tests/test_topk_wide768.py::_wide_bound_survivors
    run (f64 scores), the band form (the oracle's f32 scores: the same count of fresh survivors, inside the band's 4 ulp) and
    the pair form (the same superset verdict on the oracle's top K)."""
    from test_topk_e768 import _int8_bound_survivors
    from test_topk_wide768 import _wide_bound_survivors
    E, N, Q, K = 512, 70_001, 16, 51
    ok, nseg, mean, _ = _int8_bound_survivors(E, N, Q, K, 4242)
    okw, pre_ok, nsegw, _, _ = _wide_bound_survivors(E, N, Q, K, 4242)
    rng = np.random.default_rng(4242)
    db, q = unit_rows(rng, N, E), unit_rows(rng, Q, E)
    ex = np.stack([topk_oracle.scores(db, q[i]) for i in range(Q)], axis=1)
    sure, maybe, n = ct.count_band(db, q, K, ex, "int8")
    assert n == nseg == 2 and nsegw == 1
    assert sure <= round(mean * Q) <= maybe and maybe - sure < 0.01 * sure + 8
    _, top = topk_oracle.topk(db, q, K)
    cp, qm = ct.I8Copy(db), ct.I8Queries(q)
    for wide, b, verdict in ((False, ct.coarse_segments(N, K), ok), (True, ct.wide_segments(N), okw and pre_ok)):
        r = ct.i8_pairs(cp, qm, q, K, ct.running_taus(ex, K, b, cp.slot_row), b, top, wide)
        assert bool(r["passed"].all()) == verdict == True
