"""-m gpu: no search entry depends on what its workspace or its outputs held on entry (tests/ws_cases.py has the table and the
harness). Every workspace-taking entry of csrc/topk.hip and csrc/rowcopy.hip goes through the C ABI with a guarded workspace of
exactly *_workspace_bytes, once per fill; the outputs must be byte-identical across the fills and equal oracle/topk_oracle.c bit
for bit. Then the production pattern (IndexFlatIP._ws): one workspace, sized for the largest call of a sequence and never cleared,
and the last call must give what it gives on its own - in both orders.

N = 65576 = 2049 32-row blocks + 8 rows (a ragged last block and 16-row tile), just above SAMPLE_MIN_N, so the exact scan's pre-pass
and every coarse path run; N = 5000 (no pre-pass) and N = 5 < K (empty slots) apply to clipmi_topk_ip alone."""
import os

import numpy as np
import pytest
import torch

import test_topk_krange as kr
import ws_cases as W
from conftest import unit_rows

pytestmark = pytest.mark.gpu

N_BIG = 65576
EXACT, COARSE, COARSE_I8, WIDE_I8 = "clipmi_topk_ip", "clipmi_topk_ip_coarse", "clipmi_topk_ip_coarse_i8", "clipmi_topk_ip_wide_i8"
WS_OF = {EXACT: kr.EXACT_WS, COARSE: kr.COARSE_WS, COARSE_I8: kr.COARSE_WS, WIDE_I8: kr.WIDE_WS}
_cache = {}


def _rows(E):
    if ("db", E) not in _cache:
        rng = np.random.default_rng(7000 + E)
        _cache["db", E] = unit_rows(rng, N_BIG, E)
        q = unit_rows(rng, 65, E)
        qn = q[:5].copy()
        qn[1, 5] = np.nan                          # no usable coarse bound: the sample's select arms the exact fallback
        _cache["q", E], _cache["qnan", E] = q, qn
    return _cache["db", E]


def _index(clipmi, gpu, E, N=N_BIG, kind=None, sort=True):
    """One IndexFlatIP per (width, rows, copy, row order of the int8 copy), its copies built once"""
    key = ("idx", E, N, kind, sort)
    if key not in _cache:
        idx = clipmi.IndexFlatIP(E, device=gpu, coarse=kind)
        idx.add(_rows(E)[:N])
        if kind == "int8":
            old = os.environ.get("CLIPMI_I8_SORT")
            os.environ["CLIPMI_I8_SORT"] = "1" if sort else "0"
            try:
                idx.matrix_i8()
            finally:
                if old is None:
                    del os.environ["CLIPMI_I8_SORT"]
                else:
                    os.environ["CLIPMI_I8_SORT"] = old
        elif kind == "bf16":
            idx.matrix_bf16()
        torch.cuda.synchronize()
        _cache[key] = idx
    return _cache[key]


def _queries(E, Q, nan=False):
    _rows(E)
    return _cache["qnan" if nan else "q", E][:Q]


def _oracle(topk_oracle, E, N, Q, K, nan=False, id_base=0):
    key = ("ref", E, N, Q, K, nan, id_base)
    if key not in _cache:
        _cache[key] = topk_oracle.topk(_rows(E)[:N], _queries(E, Q, nan), K, id_base=id_base)
    return _cache[key]


def _k_near_max(E):
    return kr.KMAX[E] - 7


class Search:
    """One library call: entry, its leading arguments, queries on the device, Q, K"""

    def __init__(self, clipmi, gpu, entry, idx, q, K, id_base=0):
        self.lib, self.L, self.gpu, self.entry = clipmi._lib, clipmi._lib.lib(), gpu, entry
        db = idx.matrix()
        self.N, self.E, self.Q, self.K, self.id_base = db.shape[0], idx.d, q.shape[0], K, id_base
        if entry == EXACT:
            self.lead = (db.data_ptr(), clipmi._lib.F32, self.N, self.E)
        elif entry == COARSE:
            dbh, rmax = idx.matrix_bf16()
            self.lead = (db.data_ptr(), dbh.data_ptr(), self.N, self.E, rmax)
        else:
            db8, meta, amax, rmax = idx.matrix_i8()
            self.lead = (db.data_ptr(), db8.data_ptr(), meta.data_ptr(), amax, self.N, self.E, rmax)
        self.keep = idx
        self.qd = torch.from_numpy(np.ascontiguousarray(q)).to(gpu)
        self.ws_bytes = getattr(self.L, WS_OF[entry])(self.N, self.E, self.Q, K)
        assert self.ws_bytes > 0, clipmi._lib.last_error()
        self.outputs = [("scores", self.Q * K * 4), ("ids", self.Q * K * 8)]

    def __call__(self, ws, out_s, out_i):
        rc = getattr(self.L, self.entry)(*self.lead, self.qd.data_ptr(), self.Q, self.K, self.id_base, out_s.data_ptr(),
                                         out_i.data_ptr(), ws.data_ptr(), ws.numel(), self.lib.stream_ptr(self.gpu))
        self.lib.check(rc, self.entry)

    def before(self):
        """The call as an EARLIER call of a sequence: the shared workspace, outputs of its own"""
        own_s = torch.empty(self.Q * self.K * 4, dtype=torch.uint8, device=self.gpu)
        own_i = torch.empty(self.Q * self.K * 8, dtype=torch.uint8, device=self.gpu)
        return lambda ws, *_: self(ws, own_s, own_i)


def _assert_oracle(got, s, ref, tag):
    D = got["scores"].view(np.float32).reshape(s.Q, s.K)
    I = got["ids"].view(np.int64).reshape(s.Q, s.K)
    Ds, Is = ref
    bad = np.nonzero((I != Is) | (D.view(np.uint32) != Ds.view(np.uint32)))
    assert bad[0].size == 0, (f"{tag}: {bad[0].size} slots differ from the oracle, first at q={bad[0][0]} k={bad[1][0]}: got "
                              f"({D[bad[0][0], bad[1][0]]!r}, {I[bad[0][0], bad[1][0]]}) want "
                              f"({Ds[bad[0][0], bad[1][0]]!r}, {Is[bad[0][0], bad[1][0]]})")


def _alone(s, topk_oracle, nan=False):
    got = W.run_independent(s, s.outputs, s.ws_bytes, device=s.gpu)
    _assert_oracle(got, s, _oracle(topk_oracle, s.E, s.N, s.Q, s.K, nan, s.id_base), f"{s.entry} E={s.E} N={s.N} Q={s.Q} K={s.K}")
    return got


# ---- section 2: every entry on its own ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [512, 768])
@pytest.mark.parametrize("N,Q,K", [(N_BIG, 3, "near max"), (N_BIG, 17, 100), (5000, 3, 100), (5000, 17, 100), (5, 3, 100)])
def test_exact_scan(clipmi, gpu, topk_oracle, E, N, Q, K):
    """clipmi_topk_ip: K near the maximum leaves room for ONE query per pass (three passes inside the call, each with its
    pre-pass: every select must leave its counter zero for the next scan); Q = 17 at K = 100 is one pass at 512 and a pass of 16
    queries with a ragged second pass of one at 768. N = 5 < K: the empty slots hold (-FLT_MAX, -1) whatever the outputs held."""
    K = _k_near_max(E) if K == "near max" else K
    s = Search(clipmi, gpu, EXACT, _index(clipmi, gpu, E, N), _queries(E, Q), K, id_base=1000)
    plan = kr.make_plan(N, E, Q, K)
    assert plan["QA"] == (1 if K > 100 else min(Q, 32 if E == 512 else 16)), plan
    got = _alone(s, topk_oracle)
    if N < K:
        assert (got["ids"].view(np.int64).reshape(Q, K)[:, N:] == -1).all()
        assert (got["scores"].view(np.float32).reshape(Q, K)[:, N:] == -np.finfo(np.float32).max).all()


@pytest.mark.parametrize("E", [512, 768])
@pytest.mark.parametrize("Q,K", [(1, 10), (64, 100), (65, 100)])
def test_bf16_coarse(clipmi, gpu, topk_oracle, E, Q, K):
    """clipmi_topk_ip_coarse: Q = 65 is two 64-query passes inside the call - prep must clear what the first pass left"""
    _alone(Search(clipmi, gpu, COARSE, _index(clipmi, gpu, E, kind="bf16"), _queries(E, Q), K), topk_oracle)


@pytest.mark.parametrize("sort", [True, False], ids=["permuted", "add-order"])
@pytest.mark.parametrize("E", [512, 768])
@pytest.mark.parametrize("Q,K", [(1, 10), (64, 100), (65, 100)])
def test_int8_coarse(clipmi, gpu, topk_oracle, E, Q, K, sort):
    """clipmi_topk_ip_coarse_i8, rows of the copy ordered by their largest component and in add order: Q = 65 is the wide pass at
    512 and two 64-query passes inside the call at 768"""
    _alone(Search(clipmi, gpu, COARSE_I8, _index(clipmi, gpu, E, kind="int8", sort=sort), _queries(E, Q), K, id_base=7), topk_oracle)


def test_int8_wide_768(clipmi, gpu, topk_oracle):
    _alone(Search(clipmi, gpu, WIDE_I8, _index(clipmi, gpu, 768, kind="int8"), _queries(768, 65), 100), topk_oracle)


@pytest.mark.parametrize("entry,E,kind,wide", [(COARSE, 512, "bf16", False), (COARSE_I8, 768, "int8", False), (WIDE_I8, 768, "int8", True)])
def test_the_exact_fallback_answers(clipmi, gpu, topk_oracle, entry, E, kind, wide):
    """A query with a NaN component has no usable coarse bound: the sample's select arms the fallback, whose scan and select
    use cand_e and gcnt_e. wide: the same query among the 65 of a wide pass at 768."""
    if wide:
        q = _queries(E, 65).copy()
        q[1, 5] = np.nan
        s = Search(clipmi, gpu, entry, _index(clipmi, gpu, E, kind=kind), q, 51)
        got = W.run_independent(s, s.outputs, s.ws_bytes, device=gpu)
        _assert_oracle(got, s, topk_oracle.topk(_rows(E), q, 51), "wide pass with a NaN query")
    else:
        s = Search(clipmi, gpu, entry, _index(clipmi, gpu, E, kind=kind), _queries(E, 5, nan=True), 51)
        got = _alone(s, topk_oracle, nan=True)
    assert (got["ids"].view(np.int64).reshape(s.Q, 51)[1] == -1).all()


def _lists(rng, R, Q, K):
    """R sorted lists per query with distinct ids, the tails of some of them empty"""
    S = np.sort(rng.standard_normal((R, Q, K)).astype(np.float32), axis=2)[:, :, ::-1].copy()
    I = rng.permutation(R * Q * K).astype(np.int64).reshape(R, Q, K)
    for r in range(R):
        for q in range(Q):
            n = int(rng.integers(0, K + 1)) if (r + q) % 2 else K
            S[r, q, n:], I[r, q, n:] = -np.finfo(np.float32).max, -1
    S[0, 0, :], I[0, 0, :] = -np.finfo(np.float32).max, -1          # a wholly empty list
    return S, I


@pytest.mark.parametrize("packed", [False, True], ids=["lists", "packed"])
@pytest.mark.parametrize("R", [2, 8])
def test_merge(clipmi, gpu, topk_oracle, R, packed):
    L, lib = clipmi._lib.lib(), clipmi._lib
    Q, K = 5, 51
    S, I = _lists(np.random.default_rng(30 + R), R, Q, K)
    if R == 2:
        S[1, 1, :], I[1, 1, :] = -np.finfo(np.float32).max, -1
        S[0, 1, 3:], I[0, 1, 3:] = -np.finfo(np.float32).max, -1    # query 1: three entries in all, the rest of the result is padding
    ws_bytes = L.clipmi_merge_topk_workspace_bytes(R, Q, K)
    if packed:
        ids_off = (Q * K * 4 + 7) // 8 * 8
        rec = ids_off + Q * K * 8
        buf = np.zeros((R, rec), np.uint8)
        for r in range(R):
            buf[r, :Q * K * 4] = S[r].view(np.uint8).reshape(-1)
            buf[r, ids_off:] = I[r].view(np.uint8).reshape(-1)
        gath = torch.from_numpy(buf).to(gpu)

        def call(ws, out_s, out_i):
            lib.check(L.clipmi_merge_topk_packed(gath.data_ptr(), rec, R, Q, K, out_s.data_ptr(), out_i.data_ptr(), lib.stream_ptr(gpu)),
                      "clipmi_merge_topk_packed")
    else:
        Sd, Id = torch.from_numpy(S).to(gpu), torch.from_numpy(I).to(gpu)

        def call(ws, out_s, out_i):
            lib.check(L.clipmi_merge_topk(Sd.data_ptr(), Id.data_ptr(), R, Q, K, out_s.data_ptr(), out_i.data_ptr(), ws.data_ptr(),
                                          ws.numel(), lib.stream_ptr(gpu)), "clipmi_merge_topk")
    got = W.run_independent(call, [("scores", Q * K * 4), ("ids", Q * K * 8)], ws_bytes, device=gpu)
    Ms, Mi = topk_oracle.merge(S, I, K)
    assert np.array_equal(got["ids"].view(np.int64).reshape(Q, K), Mi)
    assert np.array_equal(got["scores"].view(np.uint32).reshape(Q, K), Ms.view(np.uint32))
    assert (Mi[1, 3:] == -1).all() if R == 2 else True


@pytest.mark.parametrize("N", [2049, 40000])
def test_rows_order_by_absmax(clipmi, gpu, N):
    """N = 2049: one item past a 2048-item tile; N = 40000: 20 blocks x 256 digits = 5120 histogram entries, so the one-workgroup
    scan runs a second 4096-entry chunk with a carry. The order is the stable sort of the rows' largest |component|."""
    L, lib, E = clipmi._lib.lib(), clipmi._lib, 512
    db = _rows(E)[:N]
    dbd = torch.from_numpy(db).to(gpu)
    assert 256 * ((N + 2047) // 2048) > 4096 if N == 40000 else True

    def call(ws, perm):
        lib.check(L.clipmi_rows_order_by_absmax(dbd.data_ptr(), N, E, perm.data_ptr(), ws.data_ptr(), ws.numel(), lib.stream_ptr(gpu)),
                  "clipmi_rows_order_by_absmax")
    got = W.run_independent(call, [("perm", N * 4)], L.clipmi_rows_order_workspace_bytes(N), device=gpu)
    want = np.argsort(np.abs(db).max(axis=1), kind="stable").astype(np.uint32)
    assert np.array_equal(got["perm"].view(np.uint32), want)


def test_rows_stats_clears_its_own_output(clipmi, gpu):
    """stats2_dev is an output the kernel only raises (atomic max): the call itself must clear it"""
    L, lib, E = clipmi._lib.lib(), clipmi._lib, 512
    idx = _index(clipmi, gpu, E, kind="int8")
    db, meta = idx.matrix(), idx.matrix_i8()[1]

    def call(ws, stats):
        lib.check(L.clipmi_rows_stats(db.data_ptr(), N_BIG, E, meta.data_ptr(), stats.data_ptr(), lib.stream_ptr(gpu)), "clipmi_rows_stats")
    got = W.run_independent(call, [("stats", 8)], 0, device=gpu)
    rmax, amax = (float(v) for v in got["stats"].view(np.float32))
    assert (rmax * (1.0 + 1e-6), amax * (1.0 + 1e-6)) == idx._stats(meta)
    norms = np.sqrt((_rows(E).astype(np.float64) ** 2).sum(axis=1))
    assert abs(float(rmax) - norms.max()) <= 1e-5 and 0.0 < amax < 0.11 * rmax


# ---- section 3: one workspace for a sequence of calls, never cleared ------------------------------------------------------------
def _sequence(seq, topk_oracle, nan_at):
    """seq: Search calls in order. The last call's outputs, behind the others in one workspace sized for the largest, must equal
    its outputs on its own (which equal the oracle's)"""
    last = seq[-1]
    alone = _alone(last, topk_oracle, nan=nan_at == len(seq) - 1)
    ws_bytes = max(s.ws_bytes for s in seq)
    W.run_after([s.before() for s in seq[:-1]], last, last.outputs, ws_bytes, alone, device=last.gpu)


@pytest.mark.parametrize("order", ["forward", "reverse"])
@pytest.mark.parametrize("entry,E,kind", [(COARSE, 512, "bf16"), (COARSE, 768, "bf16"), (COARSE_I8, 512, "int8"), (COARSE_I8, 768, "int8"),
                                          (WIDE_I8, 768, "int8")])
def test_coarse_calls_share_one_workspace(clipmi, gpu, topk_oracle, entry, E, kind, order):
    """IndexFlatIP._ws: K near the maximum, a call the fallback answers, Q = 65 (two passes or a wide pass: another carve of the
    same bytes), then Q = 1 at K = 10 - and the other way round, where the last call is the one with K near the maximum"""
    idx = _index(clipmi, gpu, E, kind=kind)
    seq = [Search(clipmi, gpu, entry, idx, _queries(E, 3), _k_near_max(E)),
           Search(clipmi, gpu, entry, idx, _queries(E, 5, nan=True), 51),
           Search(clipmi, gpu, entry, idx, _queries(E, 65), 100),
           Search(clipmi, gpu, entry, idx, _queries(E, 1), 10)]
    _sequence(seq if order == "forward" else seq[::-1], topk_oracle, nan_at=1 if order == "forward" else 2)


@pytest.mark.parametrize("order", ["forward", "reverse"])
@pytest.mark.parametrize("E", [512, 768])
def test_exact_calls_share_one_workspace(clipmi, gpu, topk_oracle, E, order):
    idx = _index(clipmi, gpu, E)
    seq = [Search(clipmi, gpu, EXACT, idx, _queries(E, 3), _k_near_max(E)), Search(clipmi, gpu, EXACT, idx, _queries(E, 17), 100)]
    _sequence(seq if order == "forward" else seq[::-1], topk_oracle, nan_at=-1)
