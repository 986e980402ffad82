"""-m gpu: the exact search of a chosen subset of the rows - clipmi_topk_ip_rows, IndexFlatIP.subset, shard_rows, the REPL behind
CLIPMI_WITHIN - bit for bit against oracle/topk_oracle.c.

The reference of every case is topk_oracle.topk(db[rows], q, K) with the positions mapped back through `rows` (+ id_base),
compared as tests/test_topk_krange_gpu.py compares: uint32 view of the scores, ids, every slot. The lists are ascending, so
position order is row-id order and ties break identically.

One seeded database of 131 101 unit rows per width, with three things planted:
  * rows 0 .. 65 535 are near-copies of query 0 (score ~ 0.99; everything else scores ~ +-0.1 against it);
  * a run of 200 identical rows at 30 000 .. 30 199 and one more copy at 130 000;
  * a row with a NaN component, one with a +inf and one with a -inf component at 6 000, 6 002, 6 004 and again at 100 000,
    100 002, 100 004 (even rows inside the contiguous subset, the every-second-row subset, the pre-pass trap's subset; the random
    subsets force them in)."""
import numpy as np
import pytest
import torch

import test_topk_krange as kr
import ws_cases as W
from conftest import unit_rows

pytestmark = pytest.mark.gpu

FMAX = np.finfo(np.float32).max
NMAX, QMAX = 131101, 65
BIG_BASE = 2 ** 40 + 5
RUN_LO, RUN_HI, RUN_FAR = 30000, 30200, 130000
SPECIAL = (6000, 6002, 6004, 100000, 100002, 100004)
LEAD = 65536

_data, _dev, _idx, _ref = {}, {}, {}, {}


def _rows(E):
    if E not in _data:
        rng = np.random.default_rng(52000 + E)
        db, q = unit_rows(rng, NMAX, E), unit_rows(rng, QMAX, E)
        lead = q[0][None, :] + 0.1 / np.sqrt(E) * rng.standard_normal((LEAD, E), dtype=np.float32) * np.sqrt(2.0)
        db[:LEAD] = (lead / np.linalg.norm(lead, axis=1, keepdims=True)).astype(np.float32)
        run = unit_rows(rng, 1, E)[0]
        db[RUN_LO:RUN_HI] = run
        db[RUN_FAR] = run
        for base in SPECIAL[::3]:
            db[base, 7] = np.nan
            db[base + 2, 11] = np.inf
            db[base + 4, 13] = -np.inf
        db.setflags(write=False)
        q.setflags(write=False)
        _data[E] = (db, q)
    return _data[E]


def _rows_dev(gpu, E):
    if E not in _dev:
        _dev[E] = torch.from_numpy(_rows(E)[0].copy()).to(gpu)
    return _dev[E]


def _parent(clipmi, gpu, E):
    if E not in _idx:
        idx = clipmi.IndexFlatIP(E, device=gpu)
        idx.add(_rows_dev(gpu, E))
        _idx[E] = idx
    return _idx[E]


def _want(topk_oracle, E, rows, q, K, id_base=0, key=None):
    """The oracle over the listed rows, positions mapped back to row ids (+ id_base). key: cache the K-independent part."""
    rows = np.asarray(rows, dtype=np.int64)
    if key is not None and (E, key, K) in _ref:
        D, P = _ref[(E, key, K)]
    else:
        D, P = topk_oracle.topk(_rows(E)[0][rows] if rows.size else np.empty((0, E), np.float32), q, K)
        if key is not None:
            _ref[(E, key, K)] = (D, P)
    I = np.where(P >= 0, rows[np.maximum(P, 0)] + id_base if rows.size else -1, -1).astype(np.int64)
    return D.copy(), I


def _assert_exact(D, I, Ds, Is, tag):
    assert D.shape == Ds.shape and I.shape == Is.shape, (tag, D.shape, Ds.shape)
    bad = np.nonzero((I != Is) | (D.view(np.uint32) != Ds.view(np.uint32)))
    assert bad[0].size == 0, (f"{tag}: {bad[0].size} mismatching slots, first at q={bad[0][0]} k={bad[1][0]}: "
                              f"got ({D[bad[0][0], bad[1][0]]!r}, {I[bad[0][0], bad[1][0]]}) "
                              f"want ({Ds[bad[0][0], bad[1][0]]!r}, {Is[bad[0][0], bad[1][0]]})")


def _abi(clipmi, gpu, db_dev, N, E, lst, q, K, id_base=0):
    """clipmi_topk_ip_rows through the C ABI: list and queries as given (numpy), a workspace of exactly the stated size, outputs
    pre-filled with NaN / -7 so that a slot nobody wrote shows."""
    L, lib = clipmi._lib.lib(), clipmi._lib
    lst = np.ascontiguousarray(lst, dtype=np.uint32)
    M, Q = lst.size, q.shape[0]
    need = L.clipmi_topk_ip_rows_workspace_bytes(M, E, Q, K)
    assert 0 < need <= kr.GIB2, lib.last_error()
    ws = torch.empty(need, dtype=torch.uint8, device=gpu)
    ld = torch.from_numpy(lst.view(np.int32).copy()).to(gpu)
    qd = torch.from_numpy(np.ascontiguousarray(q, dtype=np.float32)).to(gpu)
    out_s = torch.full((Q, K), float("nan"), dtype=torch.float32, device=gpu)
    out_i = torch.full((Q, K), -7, dtype=torch.int64, device=gpu)
    rc = L.clipmi_topk_ip_rows(db_dev.data_ptr(), lib.F32, N, E, ld.data_ptr() if M else None, M, qd.data_ptr(), Q, K, id_base,
                               out_s.data_ptr(), out_i.data_ptr(), ws.data_ptr(), ws.numel(), lib.stream_ptr(gpu))
    lib.check(rc, "clipmi_topk_ip_rows")
    torch.cuda.synchronize()
    return out_s.cpu().numpy(), out_i.cpu().numpy()


# ---- 1. shapes of the list ------------------------------------------------------------------------------------------------------
def _shape_rows(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "contiguous":
        return np.arange(4099, 74100)                                      # M = 70 001, unaligned at both ends, pre-pass runs
    if name == "every second":
        return np.arange(0, 40000, 2)                                      # M = 20 000, no pre-pass
    if name == "random 1 in 50":
        pick = np.flatnonzero(rng.random(NMAX) < 0.02)
        return np.unique(np.concatenate([pick, [0, NMAX - 1], SPECIAL]))
    if name == "random 70001":
        rest = np.setdiff1d(np.arange(NMAX), SPECIAL)
        return np.sort(np.concatenate([rng.choice(rest, 70001 - len(SPECIAL), replace=False), SPECIAL]))    # pre-pass, gathered
    if name.startswith("M="):
        M = int(name[2:])
        return np.sort(rng.choice(NMAX, M, replace=False)) if M else np.empty(0, np.int64)
    assert name == "all rows"
    return np.arange(NMAX)


SHAPES = ("contiguous", "every second", "random 1 in 50", "random 70001", "M=1", "M=15", "M=16", "M=17", "M=0", "all rows")


@pytest.mark.parametrize("E", kr.WIDTHS)
@pytest.mark.parametrize("shape", SHAPES, ids=[s.replace(" ", "_") for s in SHAPES])
def test_shapes_of_the_list(clipmi, gpu, topk_oracle, E, shape):
    """Q = 1 and 33 at K = 51 over every shape of list: contiguous and unaligned (M = 70 001: the pre-pass runs), every second row
    (M = 20 000: it does not), sparse random with the first and the last row of the matrix, dense random (the pre-pass over a
    gathered list), lists around one 16-entry tile (pads behind M), the empty list (pads only, nothing read), and all rows in
    order - which must also equal the parent's own search bit for bit. id_base = 1000; the sparse random case carries
    2^40 + 5."""
    rows = _shape_rows(shape)
    M = len(rows)
    p = kr.make_plan(M, E, 33, 51)
    assert p["sample"] == (shape in ("contiguous", "random 70001", "all rows")) and M == {"contiguous": 70001, "every second": 20000,
                                                                                          "random 70001": 70001}.get(shape, M)
    base = BIG_BASE if shape == "random 1 in 50" else 1000
    parent = _parent(clipmi, gpu, E)
    sub = parent.subset(rows)
    sub.id_base = base
    assert sub.ntotal == M
    db, q = _rows(E)
    for Q in (1, 33):
        D, I = sub.search(q[:Q], 51)
        Ds, Is = _want(topk_oracle, E, rows, q[:33], 51, key=shape)
        Ds, Is = Ds[:Q], np.where(Is[:Q] >= 0, Is[:Q] + base, -1)
        _assert_exact(D, I, Ds, Is, f"{shape} E={E} Q={Q}")
        if M < 51:
            assert (I[:, M:] == -1).all() and (D[:, M:] == -FMAX).all()
        if shape == "all rows":
            parent.id_base = base
            try:
                Dp, Ip = parent.search(q[:Q], 51)
            finally:
                parent.id_base = 0
            _assert_exact(D, I, Dp, Ip, f"all rows against the parent's search E={E} Q={Q}")
    if base == BIG_BASE:
        assert I[I >= 0].min() >= BIG_BASE


# ---- 2. query counts ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", kr.WIDTHS)
@pytest.mark.parametrize("Q", [1, 16, 17, 32, 65])
def test_query_counts(clipmi, gpu, topk_oracle, E, Q):
    """The contiguous subset with one and two 16-query column groups, full and ragged, and Q = 65: several passes over the same
    lists and counters with a ragged last one (three passes of 32 queries at 512; at 768 two query images leave room for 24
    lists, so 17 queries still go in one pass of two column groups, 32 and 65 in passes of 16)."""
    rows = _shape_rows("contiguous")
    p = kr.make_plan(len(rows), E, Q, 51)
    assert p["QA"] == {512: {65: 32}, 768: {32: 16, 65: 16}}[E].get(Q, Q) and p["QG"] == (2 if p["QA"] > 16 else 1) and p["sample"], p
    if Q == 65:
        assert -(-Q // p["QA"]) == (3 if E == 512 else 5) and Q % p["QA"] == 1
    sub = _parent(clipmi, gpu, E).subset(rows)
    sub.id_base = 1000
    D, I = sub.search(_rows(E)[1][:Q], 51)
    Ds, Is = _want(topk_oracle, E, rows, _rows(E)[1], 51, key="contiguous all queries")
    _assert_exact(D, I, Ds[:Q], np.where(Is[:Q] >= 0, Is[:Q] + 1000, -1), f"E={E} Q={Q}")


# ---- 3. K ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", kr.WIDTHS)
@pytest.mark.parametrize("case", ["K=1", "Kmax, fewer rows than K", "Kmax"])
def test_k_range(clipmi, gpu, topk_oracle, E, case):
    """K = 1; K = KMAX over a list of KMAX - 7 entries (pads, and every listed row exactly once); K = KMAX over 70 001 entries
    (one query per pass, three passes, each with its pre-pass)."""
    kmax = kr.KMAX[E]
    K = 1 if case == "K=1" else kmax
    rng = np.random.default_rng(5 + E)
    rows = np.sort(rng.choice(NMAX, kmax - 7, replace=False)) if "fewer" in case else _shape_rows("contiguous")
    Q = 3
    L = clipmi._lib.lib()
    assert 0 < L.clipmi_topk_ip_rows_workspace_bytes(len(rows), E, Q, K) <= kr.GIB2
    sub = _parent(clipmi, gpu, E).subset(rows)
    sub.id_base = 1000
    q = _rows(E)[1][1:1 + Q]
    D, I = sub.search(q, K)
    Ds, Is = _want(topk_oracle, E, rows, q, K, id_base=1000)
    _assert_exact(D, I, Ds, Is, f"{case} E={E}")
    if "fewer" in case:
        M = len(rows)
        listed_nan = int(np.isin(rows, SPECIAL[::3]).sum())                         # NaN rows are never returned
        assert (I[:, M:] == -1).all() and (D[:, M:] == -FMAX).all()
        for j in range(Q):
            got = I[j][I[j] >= 0] - 1000
            assert len(got) == len(set(got.tolist())) == M - listed_nan and np.isin(got, rows).all()


# ---- 4. the pre-pass trap -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", kr.WIDTHS)
def test_prepass_samples_list_entries_not_matrix_rows(clipmi, gpu, topk_oracle, E):
    """THE BUG THIS CATCHES: a threshold pre-pass that runs over the first rows OF THE MATRIX instead of the first entries OF
    THE LIST. The subset is rows [65 536, 131 101) (M = 65 565 >= SAMPLE_MIN_N: the pre-pass runs) and query 0 is the vector
    that the 65 536 EXCLUDED leading rows copy: their K-th best score (~ 0.99) lies above every listed score (~ 0.1), so a
    threshold taken from them is no lower bound for the list and the main scan keeps nothing - short or empty result lists.
    The result must be the oracle's full K entries."""
    rows = np.arange(LEAD, NMAX)
    assert kr.make_plan(len(rows), E, 3, 51)["sample"] and len(rows) == 65565
    q = _rows(E)[1][:3]
    sub = _parent(clipmi, gpu, E).subset(rows)
    for K in (51, 500):
        D, I = sub.search(q, K)
        Ds, Is = _want(topk_oracle, E, rows, q, K)
        assert (Is >= LEAD).all()                                         # the oracle's lists are full, and of listed rows only
        _assert_exact(D, I, Ds, Is, f"pre-pass trap E={E} K={K}")


# ---- 5. excluded winners and ties -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", kr.WIDTHS)
@pytest.mark.parametrize("K", [51, 120])
def test_excluded_winners_and_ties(clipmi, gpu, topk_oracle, E, K):
    """Queries that ARE excluded rows (their own row, the best hit of an unfiltered search, must not appear), over a subset that
    holds only the odd rows of the identical run plus its far copy: 101 equal scores for the query that equals the run, in row-id
    order. K = 51 ends inside the run, K = 120 behind it."""
    db, _ = _rows(E)
    tail = np.arange(66000, NMAX)
    rows = np.setdiff1d(np.concatenate([np.arange(RUN_LO + 1, RUN_HI, 2), [RUN_FAR], tail[tail % 3 != 0]]), SPECIAL)
    excluded = (RUN_LO, 66000, 99999, 10)
    assert not np.isin(excluded, rows).any() and RUN_FAR in rows
    q = db[list(excluded)].copy()
    sub = _parent(clipmi, gpu, E).subset(rows)
    D, I = sub.search(q, K)
    Ds, Is = _want(topk_oracle, E, rows, q, K)
    _assert_exact(D, I, Ds, Is, f"E={E} K={K}")
    for j, r in enumerate(excluded):
        assert r not in I[j]
    run = list(range(RUN_LO + 1, RUN_HI, 2)) + [RUN_FAR]
    assert I[0][:min(K, 101)].tolist() == run[:min(K, 101)] and len(set(D[0][:min(K, 101)].view(np.uint32).tolist())) == 1


# ---- 6. non-finite ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", kr.WIDTHS)
def test_non_finite_rows_and_queries(clipmi, gpu, topk_oracle, E):
    """A query with a NaN component (every score NaN: nothing is selected, all pads) and queries with a +-inf component, beside
    finite ones, over subsets that hold the planted NaN / +inf / -inf rows - with and without the pre-pass."""
    q = _rows(E)[1][:5].copy()
    q[1, 3] = np.nan
    q[2, 11] = np.inf                          # the component in which the planted +inf row is infinite: inf * inf
    q[3, 13] = np.inf                          # ... and -inf * inf
    q[4, 20] = -np.inf
    for shape in ("contiguous", "every second"):
        rows = _shape_rows(shape)
        assert np.isin(SPECIAL[:3], rows).all()
        sub = _parent(clipmi, gpu, E).subset(rows)
        D, I = sub.search(q, 51)
        Ds, Is = _want(topk_oracle, E, rows, q, 51)
        _assert_exact(D, I, Ds, Is, f"non-finite {shape} E={E}")
        assert (I[1] == -1).all() and not np.isnan(D).any()


# ---- 7. entries >= N are skipped ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", kr.WIDTHS)
@pytest.mark.parametrize("order", ["ascending", "interleaved"])
def test_entries_past_the_matrix_are_skipped(clipmi, gpu, topk_oracle, E, order):
    """Through the C ABI only (subset() refuses such lists): db_dev is the first 5 000 rows of a 20 000-row device tensor and
    N = 5 000 is passed; rows 5 000 .. 19 999 of the allocation are copies of the queries, so an implementation that forms an
    address from an entry >= N reads allocated memory and fails BY VALUE (scores of 1.0), not by a fault. Expected: the oracle
    over the valid entries alone. "ascending": the valid entries, the last of them row 4 999, then the invalid ones - 4 999 sits
    in a tile with invalid neighbours and M is no multiple of 16. "interleaved": valid and invalid entries alternating (not
    ascending: ordering is by row id, so the answer is the same set's), ending on row 4 999 in an unaligned tail."""
    rng = np.random.default_rng(700 + E)
    N, NALLOC, K = 5000, 20000, 51
    q = unit_rows(rng, 3, E)
    host = unit_rows(rng, NALLOC, E)
    host[N:] = q[rng.integers(0, 3, NALLOC - N)]
    big = torch.from_numpy(host).to(gpu)
    valid = np.unique(np.concatenate([rng.choice(N - 1, 2999, replace=False), [N - 1]]))
    invalid = np.sort(rng.choice(np.arange(N, NALLOC), 1503, replace=False))
    invalid[-1] = 0xFFFFFFFE                                            # and one far outside any allocation
    if order == "ascending":
        lst = np.concatenate([valid, invalid])
    else:
        lst = np.empty(2 * 1503, np.int64)
        lst[0::2], lst[1::2] = invalid, valid[:1503]
        lst = np.concatenate([lst, valid[1503:]])
    assert len(lst) % 16 != 0 and len(lst) <= N and valid[-1] == N - 1 and (lst[-1] == N - 1 or order == "ascending")
    D, I = _abi(clipmi, gpu, big, N, E, lst, q, K, id_base=1000)
    Ds, P = topk_oracle.topk(host[valid], q, K)
    _assert_exact(D, I, Ds, valid[P] + 1000, f"entries >= N, {order}, E={E}")
    assert (D < 0.9).all()


# ---- 8. workspace independence -----------------------------------------------------------------------------------------------------
class RowsSearch:
    """One clipmi_topk_ip_rows call for tests/ws_cases.py's harness"""

    def __init__(self, clipmi, gpu, E, rows, q, K, id_base=0):
        self.lib, self.L, self.gpu = clipmi._lib, clipmi._lib.lib(), gpu
        self.db = _rows_dev(gpu, E)
        self.rows, self.E, self.Q, self.K, self.id_base, self.M = rows, E, q.shape[0], K, id_base, len(rows)
        self.ld = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.uint32).view(np.int32).copy()).to(gpu)
        self.q = q
        self.qd = torch.from_numpy(np.array(q, dtype=np.float32, order="C")).to(gpu)
        self.ws_bytes = self.L.clipmi_topk_ip_rows_workspace_bytes(self.M, E, self.Q, K)
        assert self.ws_bytes > 0
        self.outputs = [("scores", self.Q * K * 4), ("ids", self.Q * K * 8)]

    def __call__(self, ws, out_s, out_i):
        rc = self.L.clipmi_topk_ip_rows(self.db.data_ptr(), self.lib.F32, NMAX, self.E, self.ld.data_ptr(), self.M, self.qd.data_ptr(),
                                        self.Q, self.K, self.id_base, out_s.data_ptr(), out_i.data_ptr(), ws.data_ptr(), ws.numel(),
                                        self.lib.stream_ptr(self.gpu))
        self.lib.check(rc, "clipmi_topk_ip_rows")

    def before(self):
        own_s = torch.empty(self.Q * self.K * 4, dtype=torch.uint8, device=self.gpu)
        own_i = torch.empty(self.Q * self.K * 8, dtype=torch.uint8, device=self.gpu)
        return lambda ws, *_: self(ws, own_s, own_i)

    def alone(self, topk_oracle):
        got = W.run_independent(self, self.outputs, self.ws_bytes, device=self.gpu)
        Ds, Is = _want(topk_oracle, self.E, self.rows, self.q, self.K, id_base=self.id_base)
        _assert_exact(got["scores"].view(np.float32).reshape(self.Q, self.K), got["ids"].view(np.int64).reshape(self.Q, self.K), Ds, Is,
                      f"rows E={self.E} M={self.M} Q={self.Q} K={self.K}")
        return got


def _ws_rows(M):
    return np.sort(np.random.default_rng(M).choice(NMAX, M, replace=False))


@pytest.mark.parametrize("E", kr.WIDTHS)
@pytest.mark.parametrize("M,Q,K", [(65576, 3, "near max"), (65576, 17, 100), (5000, 17, 100), (5, 3, 100)])
def test_workspace_independence(clipmi, gpu, topk_oracle, E, M, Q, K):
    """clipmi_topk_ip_rows with a guarded workspace of exactly its stated size under the four fills (zeros, words of 1, random,
    0xFF): byte-identical outputs, equal to the oracle, intact guard bands. M = 65 576 runs the pre-pass (K near the maximum: one
    query per pass, three passes, each select must leave its counter zero), M = 5 000 does not, M = 5 < K leaves pads."""
    K = kr.KMAX[E] - 7 if K == "near max" else K
    s = RowsSearch(clipmi, gpu, E, _ws_rows(M), _rows(E)[1][:Q], K, id_base=1000)
    assert kr.make_plan(M, E, Q, K)["sample"] == (M >= kr.SAMPLE_MIN_N)
    got = s.alone(topk_oracle)
    if M < K:
        assert (got["ids"].view(np.int64).reshape(Q, K)[:, M:] == -1).all()


@pytest.mark.parametrize("E", kr.WIDTHS)
@pytest.mark.parametrize("order", ["forward", "reverse"])
def test_calls_share_one_workspace(clipmi, gpu, topk_oracle, E, order):
    """The production pattern (IndexSubset._ws): one workspace sized for the largest call, never cleared; the last call gives what
    it gives on its own, in both orders."""
    q = _rows(E)[1]
    seq = [RowsSearch(clipmi, gpu, E, _ws_rows(65576), q[:3], kr.KMAX[E] - 7), RowsSearch(clipmi, gpu, E, _ws_rows(5000), q[:17], 100),
           RowsSearch(clipmi, gpu, E, _ws_rows(5), q[:3], 100)]
    seq = seq if order == "forward" else seq[::-1]
    last = seq[-1]
    alone = last.alone(topk_oracle)
    W.run_after([s.before() for s in seq[:-1]], last, last.outputs, max(s.ws_bytes for s in seq), alone, device=gpu)


# ---- 9. shards ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", kr.WIDTHS)
def test_subsets_of_three_shards_merge_to_the_subset_of_the_whole(clipmi, gpu, topk_oracle, E):
    """Three IndexFlatIP shards of the one matrix (shard_bounds), each searched through subset(shard_rows(rows, lo, hi)) with
    id_base = lo straight into its slot of the packed all-gather record, merged by clipmi_merge_topk_packed: equal to the subset
    search of the whole index and to the oracle. One shard's part of the list is empty."""
    L, lib = clipmi._lib.lib(), clipmi._lib
    rng = np.random.default_rng(9 + E)
    third = clipmi.shard_bounds(NMAX, 3, 1)
    rows = np.sort(np.concatenate([rng.choice(third[0], 3000, replace=False), np.arange(RUN_LO + 1, RUN_HI, 2),
                                   third[1] + rng.choice(NMAX - third[1], 2000, replace=False), [RUN_FAR]]))
    rows = np.unique(rows)
    Q, K = 33, 51
    q = _rows(E)[1][:Q].copy()
    q[5] = _rows(E)[0][RUN_LO]                               # ties across shards 0 and 2
    ids_off = (Q * K * 4 + 7) // 8 * 8
    rec = ids_off + Q * K * 8
    gath = torch.empty(3 * rec, dtype=torch.uint8, device=gpu)
    qd = torch.from_numpy(q).to(gpu)
    sizes = []
    for r in range(3):
        lo, hi = clipmi.shard_bounds(NMAX, 3, r)
        shard = clipmi.IndexFlatIP(E, device=gpu)
        shard.add(_rows_dev(gpu, E)[lo:hi])
        sub = shard.subset(clipmi.shard_rows(rows, lo, hi))
        sub.id_base = lo
        sizes.append(sub.ntotal)
        part = gath[r * rec:(r + 1) * rec]
        sub.search_device(qd, K, out=(part[:Q * K * 4].view(torch.float32).view(Q, K), part[ids_off:].view(torch.int64).view(Q, K)))
    assert sizes[1] == 0 and sum(sizes) == len(rows) and sizes[0] > K and sizes[2] > K
    out_s = torch.full((Q, K), float("nan"), dtype=torch.float32, device=gpu)
    out_i = torch.full((Q, K), -7, dtype=torch.int64, device=gpu)
    lib.check(L.clipmi_merge_topk_packed(gath.data_ptr(), rec, 3, Q, K, out_s.data_ptr(), out_i.data_ptr(), lib.stream_ptr(gpu)),
              "clipmi_merge_topk_packed")
    torch.cuda.synchronize()
    D, I = out_s.cpu().numpy(), out_i.cpu().numpy()
    Ds, Is = _want(topk_oracle, E, rows, q, K)
    _assert_exact(D, I, Ds, Is, f"merged shards E={E}")
    Dw, Iw = _parent(clipmi, gpu, E).subset(rows).search(q, K)
    _assert_exact(D, I, Dw, Iw, f"merged shards against the whole index's subset E={E}")


def test_a_subset_stands_in_as_a_shards_local_index(clipmi, gpu):
    """ShardedFlatIP(local_index=...) needs `device`, a settable `id_base` and search_device(q, K, out=): IndexSubset has them."""
    sub = _parent(clipmi, gpu, 512).subset([1, 2, 3])
    assert sub.device == gpu and hasattr(sub, "search_device")
    sub.id_base = 77
    _, I = sub.search(_rows(512)[1][:1], 5)
    assert sorted(I[0][:3].tolist()) == [78, 79, 80] and (I[0][3:] == -1).all()


# ---- 10. the REPL behind CLIPMI_WITHIN --------------------------------------------------------------------------------------------
class _TextModel:
    context_length = 77

    def __init__(self, vec):
        self.vec = vec

    def encode_text(self, tokens):
        return torch.from_numpy(self.vec.copy())


def test_repl_over_a_subset(clipmi, gpu, topk_oracle, tmp_path, monkeypatch):
    """A packed store of 300 vectors under dirA/, dirB/, dirC/ and an index over them; the prompt loop runs over
    index.subset(within_rows(db, "dirB/")) exactly as repl.main() builds it for CLIPMI_WITHIN=dirB/. "i 5" (an image of dirA:
    its own row is excluded), then an empty line (ignored until a text query was made, as in the reference), "q". Then a text
    query (the tokenizer and the tower replaced by a fixed vector) and the "more results" page, which asks for K = 101 of
    dirB's 100 rows. Every printed id lies in dirB's rows; the lines are the oracle's list in the reference's format."""
    rng = np.random.default_rng(10)
    vecs = unit_rows(rng, 300, 512)
    keys = [f"dir{'ABC'[i % 3]}/{i:04d}.jpg" for i in range(300)]
    db = clipmi.store.VectorStore(str(tmp_path / "vectors"), dim=512, backend="packed")
    db.put_vectors(keys, vecs)
    mat, paths = db.assemble()
    index = clipmi.IndexFlatIP(512, device=gpu)
    index.add(mat)
    rows = clipmi.repl.within_rows(db, "dirB/")
    lo, hi = db.prefix_rows(b"dirB/")
    assert (lo, hi) == (100, 200) and rows.tolist() == list(range(100, 200))
    sub = index.subset(rows)

    def run(model, script):
        it, lines = iter(script), []
        clipmi.repl.repl(model, sub, db, inp=lambda p: next(it), out=lines.append)
        return lines

    def want(f, K, offset):
        D, P = topk_oracle.topk(mat[rows], f, K)
        return [f"{D[0][j]:.4f} {rows[P[0][j]]} {paths[rows[P[0][j]]].decode()}" for j in range(K) if j > offset and P[0][j] >= 0]

    lines = run(None, ["i 5", "", "q"])
    f5 = db.get_vector(db.idx_get(5))
    res = [l for l in lines if not l.startswith(("Similar to", "Search time"))]
    assert lines[0] == f"Similar to {paths[5].decode()}:" and sum(l.startswith("Search time") for l in lines) == 1
    assert res == want(f5, 51, 0) and len(res) == 50
    assert all(lo <= int(l.split()[1]) < hi and l.split()[2].startswith("dirB/") for l in res)

    monkeypatch.setattr(clipmi.tokenizer, "tokenize", lambda texts, context_length=77: texts)
    tv = unit_rows(rng, 1, 512)
    lines = run(_TextModel(tv), ["a photo", "", "q"])
    f = clipmi.repl.normalize(tv)
    res = [l for l in lines if not l.startswith("Search time")]
    assert sum(l.startswith("Search time") for l in lines) == 2
    assert res == want(f, 51, 0) + want(f, 101, 50) and len(res) == 50 + 49            # 100 rows: the first dropped, 99 shown
    assert all(lo <= int(l.split()[1]) < hi for l in res)
    db.close()
