"""-m gpu: every search path across the whole range of K it accepts, bit for bit (uint32 view of the scores, ids) against
oracle/topk_oracle.c, and the merge kernel on lists built by hand against topk_oracle_merge.

The K values are not typed in: tests/test_topk_krange.py finds KMAX by bisection on the library's workspace functions and
the regime edges from a restatement of make_plan that it checks against the library (and it checks, without a GPU, that no
shape used here needs more than 2 GiB of workspace). A refused K is only ever checked through host-side argument validation:
nothing refused is launched; K = KMAX and the largest mergeable R*K are calls inside the documented contract.

One database of 131 101 rows and 130 queries per row width serves every case (prefixes of it are the smaller databases), and the
oracle runs once per (width, N) at KMAX: the top-K of a smaller K is the prefix of that list (the order is total).
Run with -s for the table: per case (waves, queries per pass, stage), workspace bytes, survivors, fallback armed."""
import ctypes as C

import numpy as np
import pytest
import torch

import test_topk_krange as kr
from conftest import unit_rows

pytestmark = pytest.mark.gpu

FMAX = np.finfo(np.float32).max
NMAX, QMAX = 131101, 130
BIG_BASE = 2 ** 40 + 5


def _assert_exact(D, I, Ds, Is, tag):
    assert D.shape == Ds.shape and I.shape == Is.shape, (tag, D.shape, Ds.shape)
    bad = np.nonzero((I != Is) | (D.view(np.uint32) != Ds.view(np.uint32)))
    assert bad[0].size == 0, (f"{tag}: {bad[0].size} mismatching slots, first at q={bad[0][0]} k={bad[1][0]}: "
                              f"got ({D[bad[0][0], bad[1][0]]!r}, {I[bad[0][0], bad[1][0]]}) "
                              f"want ({Ds[bad[0][0], bad[1][0]]!r}, {Is[bad[0][0], bad[1][0]]})")


# ---- shared data and references (computed once, never modified) ---------------------------------------------------------------
_data, _dev, _ref, _idx = {}, {}, {}, {}


def _rows(E):
    if E not in _data:
        rng = np.random.default_rng(90000 + E)
        db, q = unit_rows(rng, NMAX, E), unit_rows(rng, QMAX, E)
        db.setflags(write=False)
        q.setflags(write=False)
        _data[E] = (db, q)
    return _data[E]


def _rows_dev(gpu, E):
    if E not in _dev:
        _dev[E] = torch.from_numpy(_rows(E)[0].copy()).to(gpu)
    return _dev[E]


def _oracle(topk_oracle, E, N, Q, K, id_base=0):
    """The oracle's top-K of the first N rows for the first Q queries: one run per (E, N) at KMAX for all 130 queries."""
    if (E, N) not in _ref:
        db, q = _rows(E)
        D, I = topk_oracle.topk(db[:N], q, kr.KMAX[E])
        D.setflags(write=False)
        I.setflags(write=False)
        _ref[(E, N)] = (D, I)
    D, I = _ref[(E, N)]
    D, I = D[:Q, :K].copy(), I[:Q, :K].copy()
    I[I >= 0] += id_base
    return D, I


def _index(clipmi, gpu, kind, E, N):
    """One index per (copy, width, rows); they share the f32 rows on the device. kind: None, "bf16", "int8" (with the opt-in
    wide pass at 768: it only changes searches of more than 64 queries), "int8 default" (without it: index.py's default route)."""
    key = (kind, E, N)
    if key not in _idx:
        idx = clipmi.IndexFlatIP(E, device=gpu, coarse=None if kind is None else kind.split()[0], wide_768=(kind == "int8"))
        idx.add(_rows_dev(gpu, E)[:N])
        assert kind is None or idx.uses_coarse()
        _idx[key] = idx
    return _idx[key]


# The case lists need the library (KMAX): where it is missing, the failure belongs to this file's tests, not to collection.
def _cases(build):
    try:
        return build()
    except Exception as e:                                   # noqa: BLE001 - reported by test_the_case_lists_were_built
        _case_errors.append(repr(e))
        return []


_case_errors = []


def test_the_case_lists_were_built():
    assert not _case_errors, _case_errors
    assert len(EXACT_CASES) == 36 and len(COARSE_CASES) == 60 and len(PIPELINED_CASES) == 30 and len(MERGE_CASES) == 48


# ---- 2. the exact scan across its plan regimes ------------------------------------------------------------------------------
EXACT_CASES = _cases(lambda: [(E, lab, K, waves, QA, nc) for E in kr.WIDTHS for lab, K, waves, QA in kr.exact_regimes(E)
               for nc in ("prepass", "no prepass", "fewer rows than K")])


@pytest.mark.parametrize("E,lab,K,waves,QA,nc", EXACT_CASES, ids=[f"E{c[0]}-{c[1]}-K{c[2]}-{c[5]}".replace(" ", "_") for c in EXACT_CASES])
def test_exact_scan_in_every_plan_regime(clipmi, gpu, topk_oracle, E, lab, K, waves, QA, nc):
    """clipmi_topk_ip with 4 waves per workgroup and 32, 16 and 3 queries per pass, with 2 waves, with 1 wave, at KMAX; each
    with N = 70 001 (pre-pass and its sample select run), N = 20 000 (no pre-pass) and N = K - 7 (pads), and Q = 2 QA + 1: three
    passes over the same lists and counters, the last one ragged. One case per width carries id_base = 2^40 + 5."""
    N = {"prepass": 70001, "no prepass": 20000}.get(nc, K - 7)
    Q = kr.exact_q(QA)
    p = kr.make_plan(N, E, Q, K)
    assert (p["waves"], p["QA"]) == (waves, QA) and p["sample"] == (nc == "prepass")
    base = BIG_BASE if (lab == "2 waves" and nc == "prepass") else 1000
    db, q = _rows(E)
    idx = _index(clipmi, gpu, None, E, N)
    idx.id_base = base
    D, I = idx.search(q[:Q], K)
    Ds, Is = _oracle(topk_oracle, E, N, Q, K, id_base=base)
    print(f"exact E={E} {lab}: K={K} N={N} Q={Q} waves={waves} QA={QA} stage={p['stage']} "
          f"workspace={kr.exact_workspace_bytes(p)} B id_base={base}")
    _assert_exact(D, I, Ds, Is, f"exact E={E} {lab} K={K} N={N} Q={Q}")
    if N < K:
        assert (I[:, N:] == -1).all() and (D[:, N:] == -FMAX).all() and (I[:, :N] >= base).all()
        assert (np.sort(I[:, :N], axis=1) == base + np.arange(N)[None, :]).all()          # every row, once
    if base == BIG_BASE:
        assert I.min() >= BIG_BASE and I.max() < BIG_BASE + N


# ---- 3. coarse bf16, coarse int8, the wide passes -----------------------------------------------------------------------------
COARSE_CASES = _cases(lambda: [(path, E, lab, K, N) for path, E in kr.COARSE_PATHS for lab, K in kr.coarse_ks(E)
                               for N in kr.COARSE_NS])
PIPELINED_CASES = _cases(lambda: [(path, E, lab, K, N) for path, E in kr.PIPELINED_PATHS for lab, K in kr.coarse_ks(E)
                                  for N in kr.COARSE_NS])


def _hook(clipmi, gpu, idx, path, E, N, qd, Q, K):
    """The measurement hook of the path, one repetition -> (scores, ids, survivors, fallback armed or None, workspace)."""
    L = clipmi._lib.lib()
    need = getattr(L, kr.path_workspace_fn(path, E))(N, E, Q, K)
    if path == "wide":
        need = max(need, L.clipmi_topk_ip_wide_workspace_bytes(N, E, Q, K))
    assert 0 < need <= kr.GIB2
    ws = torch.empty(need, dtype=torch.uint8, device=gpu)
    os_ = torch.full((Q, K), float("nan"), dtype=torch.float32, device=gpu)
    oi_ = torch.full((Q, K), -7, dtype=torch.int64, device=gpu)
    ms, surv, nl, armed = C.c_float(0), C.c_longlong(-1), C.c_int(0), C.c_int(-1)
    dbt = idx.matrix()
    if path == "bf16":
        dbh, rmax = idx.matrix_bf16()
        rc = L.clipmi_dbg_topk_coarse_scan_ms(dbt.data_ptr(), dbh.data_ptr(), N, E, rmax, qd.data_ptr(), Q, K, os_.data_ptr(),
                                              oi_.data_ptr(), ws.data_ptr(), ws.numel(), None, 1, C.byref(ms), C.byref(surv))
    else:
        db8, meta, amax, rmax = idx.matrix_i8()
        if path == "int8":
            rc = L.clipmi_dbg_topk_coarse_i8_scan_ms(dbt.data_ptr(), db8.data_ptr(), meta.data_ptr(), amax, N, E, rmax, qd.data_ptr(),
                                                     Q, K, os_.data_ptr(), oi_.data_ptr(), ws.data_ptr(), ws.numel(), None, 1,
                                                     C.byref(ms), C.byref(surv))
        else:
            rc = L.clipmi_dbg_topk_wide_i8_scan_ms(dbt.data_ptr(), db8.data_ptr(), meta.data_ptr(), amax, N, E, rmax, qd.data_ptr(),
                                                   Q, K, os_.data_ptr(), oi_.data_ptr(), ws.data_ptr(), ws.numel(), None, 1,
                                                   C.byref(ms), C.byref(surv), C.byref(nl), C.byref(armed))
    clipmi._lib.check(rc, f"{path} scan hook")
    torch.cuda.synchronize()
    return os_.cpu().numpy(), oi_.cpu().numpy(), surv.value, (armed.value if path == "wide" else None), need


@pytest.mark.parametrize("path,E,lab,K,N", COARSE_CASES, ids=[f"{c[0]}{c[1]}-{c[2]}-K{c[3]}-N{c[4]}".replace(" ", "_") for c in COARSE_CASES])
def test_coarse_and_wide_paths_across_k(clipmi, gpu, topk_oracle, path, E, lab, K, N):
    """clipmi_topk_ip_coarse (bf16), clipmi_topk_ip_coarse_i8 and the wide passes (at 768: clipmi_topk_ip_wide_i8) at a K with the
    select's staging whole, just past where it starts to shrink inside the 100-KiB plan, at the last K of that plan, at the first
    that takes the full-LDS fallback plan, and at KMAX; two and three segments; Q = 1, 33, 64 (64-query passes) or 65, 130
    (wide). Through IndexFlatIP.search and through the path's measurement hook (one repetition), which also reports how many
    (query, row) pairs were exactly re-scored and - wide passes - whether the exact fallback was armed. Exact either way.

    At the largest K of a wide pass the fallback IS armed (both widths, both N): the sample's K-th best is the 8128th of 12 112
    rows (7104th of 12 288), so about 60 % of the first segment's 65 536 rows pass it - more than the 2^15 slots a wide list
    has. The answer is then the exact scan's, one query per launch group (QA = 1). The 64-query passes hold 2^18 slots per
    query, more than either N here: their lists cannot overflow."""
    kind = "bf16" if path == "bf16" else "int8"
    idx = _index(clipmi, gpu, kind, E, N)
    idx.id_base = 7
    db, q = _rows(E)
    p = kr.coarse_plan(N, E, 64, K)
    for Q in (kr.WIDE_Q if path == "wide" else kr.PASS64_Q):
        tag = f"{path} E={E} {lab} K={K} N={N} Q={Q}"
        Ds, Is = _oracle(topk_oracle, E, N, Q, K, id_base=7)
        D, I = idx.search(q[:Q], K)
        _assert_exact(D, I, Ds, Is, tag)
        qd = torch.from_numpy(q[:Q].copy()).to(gpu)
        Dh, Ih, surv, armed, ws = _hook(clipmi, gpu, idx, path, E, N, qd, Q, K)
        print(f"{tag}: plan in {p['limit'] // 1024} KiB waves={p['waves']} QA={p['QA']} stage={p['stage']} workspace={ws} B "
              f"survivors/query={surv / Q:.0f} fallback_armed={'n/a (2^18 slots > N)' if armed is None else armed}")
        Ih[Ih >= 0] += 7
        _assert_exact(Dh, Ih, Ds, Is, tag + " (hook)")
        assert surv >= Q * K                                   # every returned pair was exactly re-scored at least once


@pytest.mark.parametrize("path,E,lab,K,N", PIPELINED_CASES,
                         ids=[f"{c[0]}{c[1]}-{c[2]}-K{c[3]}-N{c[4]}".replace(" ", "_") for c in PIPELINED_CASES])
def test_pipelined_searches_across_k(clipmi, gpu, topk_oracle, path, E, lab, K, N):
    """More than 64 queries where the library has no wide pass for the index: the bf16 copy at both widths and the int8 copy at
    768 as index.py routes it by default (no wide_768). IndexFlatIP._search_pipelined alternates 64-query calls between the
    caller's stream and a side stream, each with its own workspace (170-200 MB at these K), and ends on a ragged call: Q = 65
    is 64 + 1 queries, Q = 130 is 64 + 64 + 2. Same five K, both N, bit-exact against the oracle; then once more on one stream
    (batches_in_flight = 1: the library loops over the 64-query passes inside one call, on the one workspace)."""
    idx = _index(clipmi, gpu, "bf16" if path == "bf16" else "int8 default", E, N)
    idx.id_base = 7
    assert not idx._wide_768_on() and idx.batches_in_flight == 2
    db, q = _rows(E)
    for Q in kr.PIPELINED_Q:
        route = clipmi.index.search_route(idx.coarse, E, idx._wide_768_on(), Q)
        assert route.chunk == 64 and route.entry == ("clipmi_topk_ip_coarse" if path == "bf16" else "clipmi_topk_ip_coarse_i8")
        Ds, Is = _oracle(topk_oracle, E, N, Q, K, id_base=7)
        D, I = idx.search(q[:Q], K)
        _assert_exact(D, I, Ds, Is, f"pipelined {path} E={E} {lab} K={K} N={N} Q={Q}")
        assert len(idx._ws) >= 2                               # the caller's stream and the side stream: a workspace each
    try:
        idx.batches_in_flight = 1
        D, I = idx.search(q[:130], K)
    finally:
        del idx.batches_in_flight                              # back to the class default
    _assert_exact(D, I, *_oracle(topk_oracle, E, N, 130, K, id_base=7), f"one stream {path} E={E} {lab} K={K} N={N} Q=130")


# ---- 4. ties at large K -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", kr.WIDTHS)
@pytest.mark.parametrize("kind", [None, "int8"])
@pytest.mark.parametrize("which", ["3000", "Kmax"])
def test_ties_at_large_k(clipmi, gpu, topk_oracle, E, kind, which):
    """The K-th boundary inside a tie group, with r in the thousands: the radix select descends through every score digit into
    the id bits. (i) 70 001 identical rows: ids 0 .. K - 1, every score the oracle's bits; (ii) a cluster of 5 000 duplicates of
    the best row among random ones: the oracle's result (at K = 3000 the boundary lies inside the cluster, at KMAX behind it).
    Exact scan and int8 coarse path, both widths, K = 3000 and KMAX: neither path needs a fallback before KMAX here (the exact
    scan has none; the 64-query lists hold 2^18 > 70 001 entries)."""
    K = 3000 if which == "3000" else kr.KMAX[E]
    Q = 3 if kind is None else 5
    rng = np.random.default_rng(1234 + E)
    v = unit_rows(rng, 1, E)
    q = unit_rows(rng, Q, E)
    idx = clipmi.IndexFlatIP(E, device=gpu, coarse=kind)
    idx.add(np.repeat(v, kr.TIE_N, axis=0))
    D, I = idx.search(q, K)
    assert (I == np.arange(K)[None, :]).all(), f"identical rows E={E} {kind} K={K}"
    for j in range(Q):
        s = topk_oracle.scores(v, q[j])
        assert (D[j].view(np.uint32) == s.view(np.uint32)[0]).all()
    key = ("cluster", E)
    if key not in _ref:
        db = _rows(E)[0][:kr.TIE_N].copy()
        base = unit_rows(np.random.default_rng(77 + E), 1, E)[0]
        db[30000:35000] = base
        db[69999] = base                                      # one more copy far away: loses every tie to the run
        qc = base[None, :] + 0.02 * unit_rows(np.random.default_rng(78 + E), 5, E)
        qc = (qc / np.linalg.norm(qc, axis=1, keepdims=True)).astype(np.float32)
        _ref[key] = (torch.from_numpy(db).to(gpu), qc) + topk_oracle.topk(db, qc, kr.KMAX[E])
    dbd, qc, Ds, Is = _ref[key]
    idx = clipmi.IndexFlatIP(E, device=gpu, coarse=kind)
    idx.add(dbd)
    D, I = idx.search(qc[:Q], K)
    _assert_exact(D, I, Ds[:Q, :K], Is[:Q, :K], f"duplicate cluster E={E} {kind} K={K}")
    assert (I[:, :3000] == 30000 + np.arange(3000)[None, :]).all()


# ---- 5. the merge kernel on lists built by hand -------------------------------------------------------------------------------
def _hand_lists(R, Q, K, seed):
    """scores f32 [R][Q][K], ids i64 [R][Q][K] (unsorted: the merge ranks a set). Per query: few distinct scores (ties across
    shards and inside a list), equal scores with ids interleaved over the shards, ids above 2^40, and - as far as R K leaves room,
    in an order that rotates with the query - NaN scores under valid ids, +inf, -inf, -0.0 against +0.0, a real -FLT_MAX, empty
    slots in the middle (some with a garbage score) and at the end of a list. Odd queries empty one whole shard; with Q >= 3
    the last query has all R lists empty; with Q = 7 query 4 holds fewer than K valid entries in total."""
    rng = np.random.default_rng(seed)
    n = R * K
    S = np.empty((R, Q, K), np.float32)
    I = np.empty((R, Q, K), np.int64)
    for qi in range(Q):
        ids = rng.permutation(4 * n + 8)[:n].astype(np.int64)
        ids[rng.random(n) < 0.3] += 1 << 40
        s = (rng.integers(-3, 4, n) * 0.25).astype(np.float32)
        ids, s = ids.reshape(R, K), s.reshape(R, K)
        for r in range(R):
            for j in range(min(K, 4)):
                s[r, j] = 1.0
                ids[r, j] = (1 << 41) + r + R * j
        flat_s, flat_i = s.reshape(-1), ids.reshape(-1)
        pos = rng.permutation(n)
        specials = [(np.nan, None), (np.inf, None), (-np.inf, None), (-0.0, None), (0.0, None), (-FMAX, None), (-FMAX, -1),
                    (np.inf, -1), (np.nan, None), (-0.0, None), (0.0, None), (-FMAX, -1), (np.nan, -1), (-np.inf, None)]
        specials = specials[qi % len(specials):] + specials[:qi % len(specials)]
        for t, (sv, iv) in enumerate(specials):
            if t < n:
                flat_s[pos[t]] = sv
                if iv is not None:
                    flat_i[pos[t]] = iv
        if K >= 8:                                              # empty slots in the middle and at the end of every list
            mid = rng.random((R, K)) < 0.1
            mid[:, -2:] = True
            s[mid], ids[mid] = -FMAX, -1
        if qi % 2 == 1 and R >= 2:
            s[qi % R], ids[qi % R] = -FMAX, -1
        if Q == 7 and qi == 4:
            few = rng.random((R, K)) < 0.7
            few[0, 0] = False
            s[few], ids[few] = -FMAX, -1
        if Q >= 3 and qi == Q - 1:
            s[:], ids[:] = -FMAX, -1
        S[:, qi, :], I[:, qi, :] = s, ids
    return S, I


MERGE_CASES = _cases(lambda: [(R, K, Q) for R in kr.MERGE_R for K in (1, 2, 51, kr.merge_kmax(R)) for Q in (1, 3, 7)])


@pytest.mark.parametrize("R,K,Q", MERGE_CASES)
def test_merge_on_hand_built_lists(clipmi, gpu, topk_oracle, R, K, Q):
    """clipmi_merge_topk and clipmi_merge_topk_packed (a record larger than the minimum, the 4-byte pad before the ids when Q K is
    odd) against topk_oracle_merge - and that against index.py's merge_lists_host, a third statement of the rule. The outputs
    hold NaN beforehand: a slot nobody wrote shows. K runs up to the largest one LDS pass takes for R lists."""
    S, I = _hand_lists(R, Q, K, seed=1000 * R + 10 * Q + K)
    Ms, Mi = topk_oracle.merge(S, I, K)
    Hs, Hi = clipmi.merge_lists_host(S, I, K)
    _assert_exact(Hs, Hi, Ms, Mi, "merge_lists_host vs oracle merge")
    assert not np.isnan(Ms).any()
    if Q >= 3:
        assert (Mi[Q - 1] == -1).all() and (Ms[Q - 1] == -FMAX).all()
    L = clipmi._lib.lib()
    Sd, Id = torch.from_numpy(S).to(gpu), torch.from_numpy(I).to(gpu)
    out_s = torch.full((Q, K), float("nan"), dtype=torch.float32, device=gpu)
    out_i = torch.full((Q, K), -7, dtype=torch.int64, device=gpu)
    ws = torch.empty(L.clipmi_merge_topk_workspace_bytes(R, Q, K), dtype=torch.uint8, device=gpu)
    rc = L.clipmi_merge_topk(Sd.data_ptr(), Id.data_ptr(), R, Q, K, out_s.data_ptr(), out_i.data_ptr(), ws.data_ptr(), ws.numel(),
                             clipmi._lib.stream_ptr(gpu))
    assert rc == 0, clipmi._lib.last_error()
    torch.cuda.synchronize()
    _assert_exact(out_s.cpu().numpy(), out_i.cpu().numpy(), Ms, Mi, f"merge R={R} K={K} Q={Q}")
    # packed: [scores | pad to 8 | ids | slack] per shard, garbage in the pad and the slack
    ids_off = (Q * K * 4 + 7) // 8 * 8
    rec = ids_off + Q * K * 8 + 24
    host = np.full((R, rec), 0xFF, np.uint8)
    for r in range(R):
        host[r, :Q * K * 4] = S[r].reshape(-1).view(np.uint8)
        host[r, ids_off:ids_off + Q * K * 8] = I[r].reshape(-1).view(np.uint8)
    gath = torch.from_numpy(host.reshape(-1)).to(gpu)
    out_s.fill_(float("nan"))
    out_i.fill_(-7)
    rc = L.clipmi_merge_topk_packed(gath.data_ptr(), rec, R, Q, K, out_s.data_ptr(), out_i.data_ptr(), clipmi._lib.stream_ptr(gpu))
    assert rc == 0, clipmi._lib.last_error()
    torch.cuda.synchronize()
    _assert_exact(out_s.cpu().numpy(), out_i.cpu().numpy(), Ms, Mi, f"merge packed R={R} K={K} Q={Q}")
    # a record too small, or not a multiple of 8 bytes: refused by the argument check (nothing runs)
    for bad in (ids_off + Q * K * 8 - 8, ids_off + Q * K * 8 + 4):
        assert L.clipmi_merge_topk_packed(gath.data_ptr(), bad, R, Q, K, out_s.data_ptr(), out_i.data_ptr(), None) == 1
        assert "record_bytes" in clipmi._lib.last_error()


@pytest.mark.parametrize("R", [1, 2, 8])
def test_merge_limit_is_refused_by_argument_validation(clipmi, gpu, R):
    """One past the largest K of one LDS pass: CLIPMI_EUNSUPPORTED with R*K in the text - a host-side check, nothing is launched
    (the accepted side of the limit runs in test_merge_on_hand_built_lists). ShardedFlatIP's GPU path hands this refusal to its
    caller as a ClipmiError through _lib.check; its gloo path merges on the host and answers exactly
    (tests/test_topk_krange.py)."""
    K = kr.merge_kmax(R) + 1
    L = clipmi._lib.lib()
    S = torch.zeros((R, 1, K), dtype=torch.float32, device=gpu)
    I = torch.zeros((R, 1, K), dtype=torch.int64, device=gpu)
    out_s = torch.full((1, K), float("nan"), dtype=torch.float32, device=gpu)
    out_i = torch.full((1, K), -7, dtype=torch.int64, device=gpu)
    rc = L.clipmi_merge_topk(S.data_ptr(), I.data_ptr(), R, 1, K, out_s.data_ptr(), out_i.data_ptr(), None, 0, None)
    assert rc == 4 and f"R*K={R * K}" in clipmi._lib.last_error(), clipmi._lib.last_error()
    with pytest.raises(clipmi.ClipmiError, match=r"R\*K=%d" % (R * K)):
        clipmi._lib.check(rc, "clipmi_merge_topk")
    ids_off = (K * 4 + 7) // 8 * 8
    gath = torch.zeros(R * (ids_off + K * 8), dtype=torch.uint8, device=gpu)
    rc = L.clipmi_merge_topk_packed(gath.data_ptr(), ids_off + K * 8, R, 1, K, out_s.data_ptr(), out_i.data_ptr(), None)
    assert rc == 4 and f"R*K={R * K}" in clipmi._lib.last_error()
    torch.cuda.synchronize()
    assert torch.isnan(out_s).all() and (out_i == -7).all()              # nothing ran
