"""-m gpu: the opt-in one-pass wide int8 search at E = 768. Every case goes through clipmi_topk_ip_wide_i8 directly (ctypes)
and through IndexFlatIP(768, coarse="int8", wide_768=True), and is compared bit for bit (uint32 view of the scores, ids) with
oracle/topk_oracle.c - or, where the query count would make the host side long, with the exact scan on the GPU (which the
existing suite pins to the oracle at 768) plus the oracle on a subset."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from conftest import unit_rows

pytestmark = pytest.mark.gpu

E = 768
CHUNK = 1024          # csrc/topk.hip WIDE768_MAX_Q
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _assert_exact(D, I, Ds, Is, tag):
    bad = np.nonzero((I != Is) | (D.view(np.uint32) != Ds.view(np.uint32)))
    assert bad[0].size == 0, (f"{tag}: {bad[0].size} mismatching slots, first at q={bad[0][0]} k={bad[1][0]}: "
                              f"got ({D[bad[0][0], bad[1][0]]!r}, {I[bad[0][0], bad[1][0]]}) "
                              f"want ({Ds[bad[0][0], bad[1][0]]!r}, {Is[bad[0][0], bad[1][0]]})")


def _anisotropic_rows(rng, n, d=E, strong=8, gain=6.0):
    x = rng.standard_normal((n, d), dtype=np.float32)
    x[:, :strong] *= np.float32(gain)
    x[:, 0] += np.float32(2.0 * gain)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x.astype(np.float32)


def _wide_index(clipmi, gpu, db, id_base=0, d=E):
    idx = clipmi.IndexFlatIP(d, device=gpu, coarse="int8", wide_768=True)
    idx.add(db)
    idx.id_base = id_base
    assert idx.uses_coarse()
    return idx


def _direct(clipmi, gpu, idx, q, K, entry="clipmi_topk_ip_wide_i8", ws_fn="clipmi_topk_ip_wide_workspace_bytes"):
    """One call of the C entry point on the current stream -> (scores, ids) as numpy."""
    L = clipmi._lib.lib()
    N, Q, d = idx.ntotal, q.shape[0], idx.d
    db = idx.matrix()
    db8, meta, amax, rmax = idx.matrix_i8()
    qd = q if isinstance(q, torch.Tensor) else torch.from_numpy(q).to(gpu)
    need = getattr(L, ws_fn)(N, d, Q, K)
    assert need > 0, clipmi._lib.last_error()
    ws = torch.empty(need, dtype=torch.uint8, device=gpu)
    os_ = torch.empty((Q, K), dtype=torch.float32, device=gpu)
    oi_ = torch.empty((Q, K), dtype=torch.int64, device=gpu)
    rc = getattr(L, entry)(db.data_ptr(), db8.data_ptr(), meta.data_ptr(), amax, N, d, rmax, qd.data_ptr(), Q, K, idx.id_base,
                           os_.data_ptr(), oi_.data_ptr(), ws.data_ptr(), ws.numel(), clipmi._lib.stream_ptr(gpu))
    clipmi._lib.check(rc, entry)
    torch.cuda.synchronize()
    return os_.cpu().numpy(), oi_.cpu().numpy()


def _both(clipmi, gpu, idx, q, K, Ds, Is, tag):
    D, I = _direct(clipmi, gpu, idx, q, K)
    _assert_exact(D, I, Ds, Is, tag + " (clipmi_topk_ip_wide_i8)")
    D, I = idx.search(q, K)
    _assert_exact(D, I, Ds, Is, tag + " (IndexFlatIP wide_768)")


def _exact_gpu(clipmi, gpu, idx, q, K):
    ex = clipmi.IndexFlatIP(idx.d, device=gpu)
    ex.add(idx.matrix())
    ex.id_base = idx.id_base
    return ex.search(q, K)


# ---- bit-exact against the oracle ---------------------------------------------------------------------------------
SMALL_Q = [65, 95, 96, 97, 127, 128, 129, 191, 192, 193, 256, 257]      # every boundary of 32-query groups, 64-query sets, tiles
_case = {}


def _shared_case(clipmi, gpu, topk_oracle, N, K):
    """One index, CHUNK + 1 queries and their references per (N, K): the oracle for the first 257 queries (a query's answer
    does not depend on how many travel with it) and for 64 spread over the rest, the GPU's exact scan for all."""
    if _case.get("key") != (N, K):
        _case.clear()
        rng = np.random.default_rng(7680 + N + K)
        db = unit_rows(rng, N, E)
        q = unit_rows(rng, CHUNK + 1, E)
        idx = _wide_index(clipmi, gpu, db, id_base=1000)
        pick = np.concatenate([np.arange(257), np.linspace(257, CHUNK, 64).astype(np.int64)])
        Do, Io = topk_oracle.topk(db, q[pick], K, id_base=1000)
        De, Ie = _exact_gpu(clipmi, gpu, idx, q, K)
        _assert_exact(De[pick], Ie[pick], Do, Io, "exact scan vs oracle")
        _case.update(key=(N, K), idx=idx, q=q, pick=pick, Do=Do, Io=Io, De=De, Ie=Ie)
    return _case


@pytest.mark.parametrize("Q", SMALL_Q + [CHUNK, CHUNK + 1])
@pytest.mark.parametrize("N,K", [(65536, 51), (70001, 11), (131101, 51), (70001, 300)])
def test_wide_768_is_bit_exact(clipmi, gpu, topk_oracle, N, K, Q):
    """One segment; a ragged last block; two segments; a large K."""
    c = _shared_case(clipmi, gpu, topk_oracle, N, K)
    q = c["q"][:Q]
    if Q <= 257:
        _both(clipmi, gpu, c["idx"], q, K, c["Do"][:Q], c["Io"][:Q], f"N={N} K={K} Q={Q}")
    else:
        _both(clipmi, gpu, c["idx"], q, K, c["De"][:Q], c["Ie"][:Q], f"N={N} K={K} Q={Q} vs exact scan")
        sub = c["pick"] < Q
        D, I = c["idx"].search(q, K)
        _assert_exact(D[c["pick"][sub]], I[c["pick"][sub]], c["Do"][sub], c["Io"][sub], f"N={N} K={K} Q={Q} vs oracle")


def test_three_segments(clipmi, gpu, topk_oracle):
    _case.clear()
    rng = np.random.default_rng(524301)
    N, Q, K = 524_301, 130, 51
    db = unit_rows(rng, N, E)
    q = unit_rows(rng, Q, E)
    idx = _wide_index(clipmi, gpu, db, id_base=1000)
    De, Ie = _exact_gpu(clipmi, gpu, idx, q, K)
    _both(clipmi, gpu, idx, q, K, De, Ie, "three segments vs exact scan")
    pick = np.arange(0, Q, 8)[:16]
    Do, Io = topk_oracle.topk(db, q[pick], K, id_base=1000)
    _assert_exact(De[pick], Ie[pick], Do, Io, "three segments: exact scan vs oracle")


@pytest.mark.parametrize("Q", [1100, 2200])
def test_beyond_the_chunk(clipmi, gpu, topk_oracle, Q):
    """More than one chunk: alternating streams (two workspaces), one stream (batches_in_flight = 1: the library loops over
    the chunks inside one call), three calls back to back with the same index."""
    _case.clear()
    rng = np.random.default_rng(65536 + Q)
    N, K = 65536, 51
    db = unit_rows(rng, N, E)
    q = unit_rows(rng, Q, E)
    idx = _wide_index(clipmi, gpu, db, id_base=1000)
    De, Ie = _exact_gpu(clipmi, gpu, idx, q, K)
    pick = np.linspace(0, Q - 1, 64).astype(np.int64)
    Do, Io = topk_oracle.topk(db, q[pick], K, id_base=1000)
    _assert_exact(De[pick], Ie[pick], Do, Io, "exact scan vs oracle")
    tq = torch.from_numpy(q).to(gpu)
    assert idx.batches_in_flight == 2
    outs = [idx.search_device(tq, K) for _ in range(3)]
    torch.cuda.synchronize()
    assert len(idx._ws) == 2
    for s, i in outs:
        _assert_exact(s.cpu().numpy(), i.cpu().numpy(), De, Ie, f"Q={Q} alternating streams")
    idx.batches_in_flight = 1
    outs = [idx.search_device(tq, K) for _ in range(3)]
    torch.cuda.synchronize()
    for s, i in outs:
        _assert_exact(s.cpu().numpy(), i.cpu().numpy(), De, Ie, f"Q={Q} one stream")
    D, I = _direct(clipmi, gpu, idx, q, K)
    _assert_exact(D, I, De, Ie, f"Q={Q} clipmi_topk_ip_wide_i8")


# ---- list limits and hard data ------------------------------------------------------------------------------------
def _hook(clipmi, gpu, idx, q, K):
    """clipmi_dbg_topk_wide_i8_scan_ms, one repetition -> (ids, re-scored pairs, scan launches, fallback armed, scan ms)."""
    L = clipmi._lib.lib()
    N, Q = idx.ntotal, q.shape[0]
    db = idx.matrix()
    db8, meta, amax, rmax = idx.matrix_i8()
    qd = torch.from_numpy(q).to(gpu)
    need = L.clipmi_topk_ip_wide_workspace_bytes(N, idx.d, Q, K)
    assert need > 0, clipmi._lib.last_error()
    ws = torch.empty(need, dtype=torch.uint8, device=gpu)
    os_ = torch.empty((Q, K), dtype=torch.float32, device=gpu)
    oi_ = torch.empty((Q, K), dtype=torch.int64, device=gpu)
    ms, surv, nl, armed = C.c_float(0), C.c_longlong(-1), C.c_int(-1), C.c_int(-1)
    rc = L.clipmi_dbg_topk_wide_i8_scan_ms(db.data_ptr(), db8.data_ptr(), meta.data_ptr(), amax, N, idx.d, rmax, qd.data_ptr(), Q, K,
                                           os_.data_ptr(), oi_.data_ptr(), ws.data_ptr(), ws.numel(), None, 1, C.byref(ms),
                                           C.byref(surv), C.byref(nl), C.byref(armed))
    clipmi._lib.check(rc, "clipmi_dbg_topk_wide_i8_scan_ms")
    torch.cuda.synchronize()
    return oi_.cpu().numpy(), surv.value, nl.value, armed.value, ms.value


def test_identical_rows_arm_the_fallback(clipmi, gpu, topk_oracle):
    """300 000 identical rows with one scaled row: every pair passes, the lists reach WIDE_CAP, the exact fallback answers."""
    _case.clear()
    rng = np.random.default_rng(781)
    N, Q, K = 300000, 130, 20
    v = unit_rows(rng, 1, E)
    db = np.repeat(v, N, axis=0)
    db[123456] *= np.float32(1.5)
    q = unit_rows(rng, Q, E)
    idx = _wide_index(clipmi, gpu, db)
    Ds, Is = topk_oracle.topk(db, q, K)
    _both(clipmi, gpu, idx, q, K, Ds, Is, "identical rows")
    ids, _, _, armed, _ = _hook(clipmi, gpu, idx, q, K)
    assert armed == 1
    assert np.array_equal(ids, Is)


def test_duplicate_cluster(clipmi, gpu, topk_oracle):
    """4096 consecutive duplicates of the row that ranks first for every query."""
    rng = np.random.default_rng(791)
    N, Q = 100000, 200
    db = unit_rows(rng, N, E)
    base = unit_rows(rng, 1, E)[0]
    db[30000:34096] = base
    db[77777] = base
    q = base[None, :] + 0.02 * unit_rows(rng, Q, E)
    q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    idx = _wide_index(clipmi, gpu, db)
    Ds, Is = topk_oracle.topk(db, q, 51)
    _both(clipmi, gpu, idx, q, 51, Ds, Is, "duplicate cluster")
    assert (Is[:, 0] == 30000).all() and (Is[:, 50] == 30050).all()


def test_sample_threshold_filters_nothing(clipmi, gpu, topk_oracle):
    """The first 40 k rows - the whole sample - score about -280 against every query: the scan accepts every pair."""
    rng = np.random.default_rng(802)
    N, Q = 70001, 200
    u = unit_rows(rng, 1, E)[0]
    q = unit_rows(rng, Q, E) + np.float32(0.3) * u[None, :]          # every query has a positive component along u
    q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    assert (q @ u > 0.1).all()
    db = unit_rows(rng, N, E)
    db[:40000] = (-1000.0 * u)[None, :] * (1.0 + 1e-6 * np.arange(40000, dtype=np.float32))[:, None]
    idx = _wide_index(clipmi, gpu, db)
    Ds, Is = topk_oracle.topk(db, q, 51)
    _both(clipmi, gpu, idx, q, 51, Ds, Is, "useless sample threshold")
    assert (Is >= 40000).all()


def test_anisotropic_rows(clipmi, gpu, topk_oracle):
    rng = np.random.default_rng(4245)
    db = _anisotropic_rows(rng, 150000)
    q = _anisotropic_rows(rng, 200)
    idx = _wide_index(clipmi, gpu, db)
    Ds, Is = topk_oracle.topk(db, q, 51)
    _both(clipmi, gpu, idx, q, 51, Ds, Is, "anisotropic")


def test_unnormalised_rows_permute_the_copy(clipmi, gpu, topk_oracle):
    """Row norms over three decades: the copy is really a permutation; near-duplicates of the best row and an exact tie."""
    rng = np.random.default_rng(78)
    N, Q = 90000, 130
    db = (unit_rows(rng, N, E) * (10.0 ** rng.uniform(-1.5, 1.5, size=(N, 1)))).astype(np.float32)
    q = unit_rows(rng, Q, E) * np.float32(1.7)
    base = db[np.argmax(db @ q[0])].copy()
    for j in range(200):
        db[1000 + 7 * j] = base * np.float32(1.0 - 1e-6 * j)
    db[50000] = db[1000]
    idx = _wide_index(clipmi, gpu, db)
    slot_rows = idx.matrix_i8()[1].cpu().numpy().view(np.uint32)[-((N + 31) // 32 * 32 + 32):][:N]
    assert not np.array_equal(slot_rows, np.arange(N, dtype=np.uint32))
    Ds, Is = topk_oracle.topk(db, q, 51)
    _both(clipmi, gpu, idx, q, 51, Ds, Is, "unnormalised rows")


def test_non_finite_queries_beside_ordinary_ones(clipmi, gpu, topk_oracle):
    rng = np.random.default_rng(98)
    N, Q = 70000, 130
    db = (unit_rows(rng, N, E) * rng.uniform(0.2, 2.0, size=(N, 1))).astype(np.float32)
    q = unit_rows(rng, Q, E)
    q[1, 5] = np.nan
    q[2, 9] = np.inf
    q[3, 9] = -np.inf
    q[4, :] = 0.0
    q[33, 700] = np.nan
    q[40, 0], q[40, 1] = np.inf, -np.inf
    q[100, 767] = np.nan
    q[129, :] = 0.0
    idx = _wide_index(clipmi, gpu, db)
    Ds, Is = topk_oracle.topk(db, q, 51)
    _both(clipmi, gpu, idx, q, 51, Ds, Is, "non-finite queries")
    assert (Is[1] == -1).all() and (Is[0] >= 0).all()


# ---- the hook -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q", [128, 1100])
def test_hook_counts_launches_and_survivors(clipmi, gpu, topk_oracle, Q):
    """N = 200 000 has two segments: the copy is streamed once per chunk (scan launches = 2 x chunks), nothing overflows,
    and fewer than N / 16 rows per query are exactly re-scored (the numpy restatement predicts ~1.3 k fresh + the kept heads).
    Ids against the oracle: all of them at Q = 128; at Q = 1100 all against the exact scan and 64 against the oracle."""
    if _case.get("key") != "hook":
        _case.clear()
        rng = np.random.default_rng(4242)
        db = unit_rows(rng, 200_000, E)
        _case.update(key="hook", db=db, rng=rng, idx=_wide_index(clipmi, gpu, db))
    N, K = 200_000, 51
    db, idx = _case["db"], _case["idx"]
    q = unit_rows(_case["rng"], Q, E)
    ids, surv, launches, armed, ms = _hook(clipmi, gpu, idx, q, K)
    chunks = (Q + CHUNK - 1) // CHUNK
    print(f"wide 768 hook: N={N} Q={Q} K={K}: {launches} scan launches, {surv / Q:.0f} re-scored rows per query, scan {ms:.3f} ms")
    assert launches == 2 * chunks
    assert armed == 0
    assert surv / Q < N / 16
    if Q <= 257:
        Ds, Is = topk_oracle.topk(db, q, K)
        assert np.array_equal(ids, Is)
    else:
        De, Ie = _exact_gpu(clipmi, gpu, idx, q, K)
        assert np.array_equal(ids, Ie)
        pick = np.linspace(0, Q - 1, 64).astype(np.int64)
        Ds, Is = topk_oracle.topk(db, q[pick], K)
        assert np.array_equal(ids[pick], Is)


# ---- plumbing -----------------------------------------------------------------------------------------------------
def test_at_512_the_new_entry_is_the_old_one(clipmi, gpu):
    _case.clear()
    rng = np.random.default_rng(512)
    db, q = unit_rows(rng, 90_000, 512), unit_rows(rng, 200, 512)
    idx = _wide_index(clipmi, gpu, db, d=512)
    Dn, In = _direct(clipmi, gpu, idx, q, 51)
    Do, Io = _direct(clipmi, gpu, idx, q, 51, "clipmi_topk_ip_coarse_i8", "clipmi_topk_ip_coarse_workspace_bytes")
    _assert_exact(Dn, In, Do, Io, "E = 512: wide entry vs coarse entry")


def test_one_workspace_with_the_flag_two_without(clipmi, gpu, topk_oracle):
    rng = np.random.default_rng(4243)
    N, Q, K = 90_000, 200, 51
    db, q = unit_rows(rng, N, E), unit_rows(rng, Q, E)
    tq = torch.from_numpy(q).to(gpu)
    Ds, Is = topk_oracle.topk(db, q, K)
    on = _wide_index(clipmi, gpu, db)
    s, i = on.search_device(tq, K)
    _assert_exact(s.cpu().numpy(), i.cpu().numpy(), Ds, Is, "flag on")
    assert len(on._ws) == 1
    L = clipmi._lib.lib()
    assert next(iter(on._ws.values())).numel() == L.clipmi_topk_ip_wide_workspace_bytes(N, E, Q, K)
    off = clipmi.IndexFlatIP(E, device=gpu, coarse="int8", wide_768=False)
    off.add(db)
    s, i = off.search_device(tq, K)
    _assert_exact(s.cpu().numpy(), i.cpu().numpy(), Ds, Is, "flag off")
    assert len(off._ws) == 2


def _sharded_worker(rank, world, port, tmp):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch.distributed as dist
    import clipmi
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        rng = np.random.default_rng(140)                  # the same rows on every rank; each keeps its shard
        N, Q, K = 140_001, 130, 51
        db = unit_rows(rng, N, E)
        db[N - 1] = db[7]                                  # duplicate across the shard boundary
        q = unit_rows(rng, Q, E)
        lo, hi = clipmi.shard_bounds(N, world, rank)
        local = clipmi.IndexFlatIP(E, device="cuda:0", coarse="int8", wide_768=True)
        local.add(db[lo:hi])
        # both ranks share the one GPU: the shards' partial results travel over gloo, the searches are the local index's
        sh = clipmi.ShardedFlatIP(local, N, local_search=lambda qq, k, base: local.search(np.asarray(qq), k))
        assert local.id_base == lo and local.uses_coarse() and local._wide_768_on()
        D, I = sh.search(q, K)
        ok = True
        if rank == 0:
            single = clipmi.IndexFlatIP(E, device="cuda:0", coarse="int8", wide_768=True)
            single.add(db)
            Ds, Is = single.search(q, K)
            ok = np.array_equal(I, Is) and np.array_equal(D.view(np.uint32), Ds.view(np.uint32)) and (Is[:, 0] >= 0).all()
        open(os.path.join(tmp, f"ok{rank}"), "w").write("1" if ok else "0")
    finally:
        dist.destroy_process_group()


def test_sharded_over_two_shards_equals_the_single_index(tmp_path):
    """ShardedFlatIP over two shards (two ranks on the one GPU, partial results over gloo) with the flag on == one index."""
    import torch.multiprocessing as mp
    mp.spawn(_sharded_worker, args=(2, 29500 + (os.getpid() + 768) % 2000, str(tmp_path)), nprocs=2, join=True)
    assert (tmp_path / "ok0").read_text() == "1" and (tmp_path / "ok1").read_text() == "1"
