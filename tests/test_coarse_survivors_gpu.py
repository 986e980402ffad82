"""-m gpu: how many (query, row) pairs each coarse scan hands to the exact re-scoring pass, against the counts recorded from
the parent commit of csrc/coarse_scan.hpp (tests/golden/coarse_survivors_parent.json, never written from here; its bf16
entries were recorded again, under `commit_bf16`, when the bf16 margin coefficient was corrected - a change of the counts by
design -, and two int8 entries under `commit_norms`, when the norms of the bound became f64 sums rounded up: one pair more,
which tests/coarse_tight.py::i8_survivors reproduces on the CPU - 395 574 with topk_magnitude.legacy, 395 575 with `current`,
154 929 for the first 200 queries with both), and - the 64-query `unit` cases - against the band of the numpy restatement of the scan's test
(tests/coarse_tight.py::count_band), so that a recorded count is not merely the code's own word.

The bit-exact suites cannot see a scan that keeps too many or too few pairs outside the top K: the lists are supersets. The
measurement hooks return the number of exactly re-scored pairs, a deterministic function of the data (the thresholds are exact
K-th bests; atomics only change the order inside a list), so every case reproduces its count EXACTLY - a count that differs is
a change of behaviour, not a reason to record again. Each case also compares the hook's ids with the oracle (all queries up to
200; beyond that with the exact scan on the GPU, and 64 evenly spaced queries with the oracle)."""
import json
import os

import numpy as np
import pytest

import coarse_tight as ct
from conftest import unit_rows

pytestmark = pytest.mark.gpu

N, K = 70_001, 51            # above the coarse path's 65 536 minimum, no multiple of 32, two segments of the 64-query passes
NQ = 1024
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "coarse_survivors_parent.json")

# (kernel the case reaches, rows, E, copy, Q)
CASES = (
    # scan_coarse_kernel<E, QG = 1 | 2 | 4, pre and main, bf16 | int8>; Q = 5 and 17 leave an inactive-column tail
    [("scan_coarse", "unit", E, kind, Q) for E in (512, 768) for kind in ("bf16", "int8") for Q in (5, 17, 64)]
    + [("wide<8>", "unit", 512, "int8", Q) for Q in (65, 191)]
    + [("wide<4,0,24>", "unit", 768, "int8", Q) for Q in (65, 130, 1024)]
    # tiles whose waves own 0, 1 and 2 groups; Q no multiple of 32
    + [("wide2<4,2>", "unit", 512, "int8", Q) for Q in (192, 200, 513, 1024)]
    # 4 096 consecutive duplicates of the row that ranks first for every query: a wave holds more than COARSE_FLUSH /
    # WIDE_FLUSH pending pairs in mid-scan (the flush path), and the global lists do not overflow (no fallback)
    + [("scan_coarse", "dup", 512, "bf16", 64), ("scan_coarse", "dup", 512, "int8", 64),
       ("wide<8>", "dup", 512, "int8", 130), ("wide2<4,2>", "dup", 512, "int8", 256)]
)


def case_id(c):
    return f"{c[0]}-{c[1]}-E{c[2]}-{c[3]}-Q{c[4]}"


_rows, _index, _ref = {}, {}, {}


def rows(kind, E):
    """(db, queries) of a row set, built once: seeded unit rows, or the duplicate cluster of
    test_topk_gpu.py::test_coarse_duplicate_cluster_many_queries (256 similar queries)."""
    if (kind, E) not in _rows:
        rng = np.random.default_rng(70_001 + E + (7 if kind == "dup" else 0))
        db = unit_rows(rng, N, E)
        if kind == "dup":
            base = unit_rows(rng, 1, E)[0]
            db[30000:34096] = base
            db[77777 % N] = base
            q = base[None, :] + 0.02 * unit_rows(rng, 256, E)
            q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
        else:
            q = unit_rows(rng, NQ, E)
        _rows[(kind, E)] = (db, q)
    return _rows[(kind, E)]


def index(clipmi, gpu, kind, E, copy):
    """One index per (rows, E, copy), built once per module."""
    key = (kind, E, copy)
    if key not in _index:
        idx = clipmi.IndexFlatIP(E, device=gpu, coarse=copy, wide_768=True)
        idx.add(rows(kind, E)[0])
        assert idx.uses_coarse()
        _index[key] = idx
    return _index[key]


def measure(clipmi, gpu, c):
    """The measurement hook of the case's path, one repetition -> (ids, re-scored pairs, fallback armed or None)."""
    _, kind, E, copy, Q = c
    _, ids, surv, armed = ct.scan_hook(clipmi, gpu, index(clipmi, gpu, kind, E, copy), rows(kind, E)[1][:Q], K, copy, case_id(c))
    return ids, surv, armed


def reference(clipmi, gpu, topk_oracle, kind, E):
    """Per row set, once: the oracle's ids of the first 200 queries and of 64 evenly spaced later ones, and the exact GPU
    scan's ids of all of them (pinned to the oracle on those)."""
    if (kind, E) not in _ref:
        db, q = rows(kind, E)
        nq = q.shape[0]
        pick = np.unique(np.concatenate([np.arange(200), np.linspace(200, nq - 1, 64).astype(np.int64)]))
        _, Io = topk_oracle.topk(db, q[pick], K)
        ex = clipmi.IndexFlatIP(E, device=gpu)
        ex.add(db)
        _, Ie = ex.search(q, K)
        assert np.array_equal(Ie[pick], Io), "exact scan vs oracle"
        _ref[(kind, E)] = (pick, Io, Ie)
    return _ref[(kind, E)]


def test_the_recorded_cases_are_these():
    g = json.load(open(GOLDEN))
    assert len(g["commit"]) == 40 and int(g["commit"], 16) >= 0
    assert len(g["commit_bf16"]) == 40 and int(g["commit_bf16"], 16) >= 0 and g["commit_bf16"] != g["commit"] and g["reason_bf16"]
    assert [e["id"] for e in g["cases"] if e.get("recorded") == "commit_bf16"] == [case_id(c) for c in CASES if c[3] == "bf16"]
    assert len(g["commit_norms"]) == 40 and int(g["commit_norms"], 16) >= 0 and g["commit_norms"] not in (g["commit"], g["commit_bf16"]) and g["reason_norms"]
    assert [e["id"] for e in g["cases"] if e.get("recorded") == "commit_norms"] == ["wide2<4,2>-unit-E512-int8-Q513", "wide2<4,2>-unit-E512-int8-Q1024"]
    assert [e["id"] for e in g["cases"]] == [case_id(c) for c in CASES]


@pytest.mark.parametrize("c", CASES, ids=[case_id(c) for c in CASES])
def test_survivor_count_equals_the_parents(clipmi, gpu, topk_oracle, c):
    want = {e["id"]: e for e in json.load(open(GOLDEN))["cases"]}[case_id(c)]
    _, kind, E, _, Q = c
    ids, surv, armed = measure(clipmi, gpu, c)
    print(f"{case_id(c)}: {surv} re-scored pairs (parent {want['survivors']}), fallback armed {armed} (parent {want['fallback_armed']})")
    assert surv == want["survivors"]
    assert armed == want["fallback_armed"]
    if kind == "dup":
        assert armed in (None, 0)
    pick, Io, Ie = reference(clipmi, gpu, topk_oracle, kind, E)
    if Q <= 200:
        assert np.array_equal(ids, Io[:Q])          # pick starts with 0 .. 199
    else:
        assert np.array_equal(ids, Ie[:Q])
        sub = pick < Q
        assert np.array_equal(ids[pick[sub]], Io[sub])


BAND_CASES = [c for c in CASES if c[1] == "unit" and c[4] <= 64]
_exact, _copy = {}, {}


@pytest.mark.parametrize("c", BAND_CASES, ids=[case_id(c) for c in BAND_CASES])
def test_survivor_count_lies_in_the_restatements_band(clipmi, gpu, topk_oracle, c):
    """What the 64-query hooks count, read from csrc/topk.hip: select_topk_kernel writes its list length M to m_out after every
    segment's re-scoring (rescore_select: overwritten after segment 0, added after the later ones). The sample's select has no
    m_out and leaves its list empty, so segment 0's list is that segment's fresh survivors alone; each later list is the K
    heads the previous select kept plus the segment's fresh survivors. Hook = fresh pairs of all segments + K x (segments - 1)
    per query (every list here is longer than K). The count must lie between the restatement's pairs that pass by more than
    the f32 rounding of the two compared quantities and its pairs that pass or miss by no more than that (count_band states
    the band: 4 ulp for int8; for bf16 the accumulation bound E 2^-24 ||x^|| ||q^|| + 2 ulp of the threshold)."""
    _, kind, E, copy, Q = c
    db, q = rows(kind, E)
    if E not in _exact:
        _exact[E] = np.stack([topk_oracle.scores(db, q[i]) for i in range(64)], axis=1)      # the oracle's f32 scores
    if (E, copy) not in _copy:
        _copy[(E, copy)] = ct.I8Copy(db) if copy == "int8" else ct.Bf16Copy(db)
    _, surv, _ = measure(clipmi, gpu, c)
    sure, maybe, nseg = ct.count_band(db, q[:Q], K, _exact[E][:, :Q], copy, cp=_copy[(E, copy)])
    heads = K * Q * (nseg - 1)
    print(f"{case_id(c)}: hook {surv}, restatement {sure + heads} .. {maybe + heads} ({heads} kept heads, {nseg} segments)")
    assert nseg == 2
    assert sure + heads <= surv <= maybe + heads
