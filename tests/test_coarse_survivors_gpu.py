"""-m gpu: how many (query, row) pairs each coarse scan hands to the exact re-scoring pass, against the counts recorded from
the parent commit of csrc/coarse_scan.hpp (tests/golden/coarse_survivors_parent.json, never written from here).

The bit-exact suites cannot see a scan that keeps too many or too few pairs outside the top K: the lists are supersets. The
measurement hooks return the number of exactly re-scored pairs, a deterministic function of the data (the thresholds are exact
K-th bests; atomics only change the order inside a list), so every case reproduces its count EXACTLY - a count that differs is
a change of behaviour, not a reason to record again. Each case also compares the hook's ids with the oracle (all queries up to
200; beyond that with the exact scan on the GPU, and 64 evenly spaced queries with the oracle)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

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
    idx = index(clipmi, gpu, kind, E, copy)
    L = clipmi._lib.lib()
    qd = torch.from_numpy(rows(kind, E)[1][:Q].copy()).to(gpu)
    need = max(L.clipmi_topk_ip_coarse_workspace_bytes(N, E, Q, K), L.clipmi_topk_ip_wide_workspace_bytes(N, E, Q, K))
    assert need > 0, clipmi._lib.last_error()
    ws = torch.empty(need, dtype=torch.uint8, device=gpu)
    os_ = torch.empty((Q, K), dtype=torch.float32, device=gpu)
    oi_ = torch.full((Q, K), -7, dtype=torch.int64, device=gpu)
    ms, surv, nl, armed = C.c_float(0), C.c_longlong(-1), C.c_int(-1), C.c_int(-1)
    db = idx.matrix()
    tail = (qd.data_ptr(), Q, K, os_.data_ptr(), oi_.data_ptr(), ws.data_ptr(), ws.numel(), None, 1, C.byref(ms), C.byref(surv))
    if copy == "bf16":
        dbh, rmax = idx.matrix_bf16()
        rc = L.clipmi_dbg_topk_coarse_scan_ms(db.data_ptr(), dbh.data_ptr(), N, E, rmax, *tail)
    else:
        db8, meta, amax, rmax = idx.matrix_i8()
        if Q <= 64:
            rc = L.clipmi_dbg_topk_coarse_i8_scan_ms(db.data_ptr(), db8.data_ptr(), meta.data_ptr(), amax, N, E, rmax, *tail)
        else:
            rc = L.clipmi_dbg_topk_wide_i8_scan_ms(db.data_ptr(), db8.data_ptr(), meta.data_ptr(), amax, N, E, rmax, *tail,
                                                   C.byref(nl), C.byref(armed))
    clipmi._lib.check(rc, case_id(c))
    torch.cuda.synchronize()
    return oi_.cpu().numpy(), surv.value, (armed.value if Q > 64 else None)


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
