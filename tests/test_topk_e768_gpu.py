"""-m gpu: 768-wide indexes (ViT-L/14) through the int8 and bf16 coarse paths return what the exact scan returns, bit for
bit - the cases of tests/test_topk_gpu.py's 512 suite at E = 768, against oracle/topk_oracle.c."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import unit_rows

pytestmark = pytest.mark.gpu

E = 768
KINDS = ["int8", "bf16"]


def _assert_exact(D, I, Ds, Is, tag):
    bad = np.nonzero((I != Is) | (D.view(np.uint32) != Ds.view(np.uint32)))
    assert bad[0].size == 0, (f"{tag}: {bad[0].size} mismatching slots, first at q={bad[0][0]} k={bad[1][0]}: "
                              f"got ({D[bad[0][0], bad[1][0]]!r}, {I[bad[0][0], bad[1][0]]}) "
                              f"want ({Ds[bad[0][0], bad[1][0]]!r}, {Is[bad[0][0], bad[1][0]]})")


def _run_coarse(clipmi, gpu, db, q, K, id_base=0, kind="int8", expect_coarse=True):
    idx = clipmi.IndexFlatIP(E, device=gpu, coarse=kind)
    idx.add(db)
    idx.id_base = id_base
    assert idx.uses_coarse() == expect_coarse
    return idx.search(q, K)


def _anisotropic_rows(rng, n, d=E, strong=8, gain=6.0):
    x = rng.standard_normal((n, d), dtype=np.float32)
    x[:, :strong] *= np.float32(gain)
    x[:, 0] += np.float32(2.0 * gain)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x.astype(np.float32)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N,Q,K", [(65536, 1, 51), (70001, 16, 51), (100000, 33, 11), (131072, 64, 51), (200003, 64, 101),
                                   (70001, 5, 300)])
def test_coarse_paths_are_bit_exact_at_768(clipmi, gpu, topk_oracle, kind, N, Q, K):
    rng = np.random.default_rng(N + Q + K + (1 if kind == "int8" else 0))
    db = unit_rows(rng, N, E)
    q = unit_rows(rng, Q, E)
    D, I = _run_coarse(clipmi, gpu, db, q, K, id_base=1000, kind=kind)
    Ds, Is = topk_oracle.topk(db, q, K, id_base=1000)
    _assert_exact(D, I, Ds, Is, f"{kind} E=768 N={N} Q={Q} K={K}")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("Q", [65, 130, 200])
def test_more_than_64_queries_are_pipelined_64_query_passes(clipmi, gpu, topk_oracle, kind, Q):
    """No wide pass at 768: both kinds run a large search as 64-query passes alternating between the caller's stream and
    the side stream (two workspaces); with batches_in_flight = 1 the library loops over the passes inside one call."""
    rng = np.random.default_rng(4242 + Q)
    N, K = 90_000, 51
    db = unit_rows(rng, N, E)
    q = unit_rows(rng, Q, E)
    idx = clipmi.IndexFlatIP(E, device=gpu, coarse=kind)
    idx.add(db)
    assert idx.uses_coarse() and idx.batches_in_flight == 2
    tq = torch.from_numpy(q).to(gpu)
    outs = [idx.search_device(tq, K) for _ in range(3)]
    outs = [(s.clone(), i.clone()) for s, i in outs]
    assert len(idx._ws) >= 2
    idx.batches_in_flight = 1
    s1, i1 = idx.search_device(tq, K)
    torch.cuda.synchronize()
    D, I = topk_oracle.topk(db, q, K)
    _assert_exact(s1.cpu().numpy(), i1.cpu().numpy(), D, I, f"{kind} Q={Q} one stream")
    for s, i in outs:
        _assert_exact(s.cpu().numpy(), i.cpu().numpy(), D, I, f"{kind} Q={Q} pipelined")
    idx.batches_in_flight = 2
    Dn, In = idx.search(q, K)
    _assert_exact(Dn, In, D, I, f"{kind} Q={Q} search()")


@pytest.mark.parametrize("kind", KINDS)
def test_unnormalised_rows_permute_the_copy(clipmi, gpu, topk_oracle, kind):
    """Row norms 0.2 ... 2: the int8 copy is a non-trivial permutation (rows ordered by their largest |component|), the
    margins scale with the largest norm; near-duplicates of the best row and an exact tie."""
    rng = np.random.default_rng(77)
    N = 90000
    db = (unit_rows(rng, N, E) * rng.uniform(0.2, 2.0, size=(N, 1))).astype(np.float32)
    q = unit_rows(rng, 9, E) * np.float32(1.7)
    base = db[np.argmax(db @ q[0])].copy()
    for j in range(200):
        db[1000 + 7 * j] = base * np.float32(1.0 - 1e-6 * j)
    db[50000] = db[1000]
    D, I = _run_coarse(clipmi, gpu, db, q, 51, kind=kind)
    Ds, Is = topk_oracle.topk(db, q, 51)
    _assert_exact(D, I, Ds, Is, f"{kind} unnormalised rows")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("Q", [64, 130])
def test_identical_rows_many_queries(clipmi, gpu, topk_oracle, kind, Q):
    """300 k identical rows: every (query, row) pair passes, the lists overflow, the exact fallback answers."""
    rng = np.random.default_rng(780 + Q)
    N = 300000
    v = unit_rows(rng, 1, E)
    db = np.repeat(v, N, axis=0)
    db[123456] *= np.float32(1.5)
    q = unit_rows(rng, Q, E)
    D, I = _run_coarse(clipmi, gpu, db, q, 20, kind=kind)
    Ds, Is = topk_oracle.topk(db, q, 20)
    _assert_exact(D, I, Ds, Is, f"{kind} identical rows Q={Q}")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("Q", [64, 130])
def test_duplicate_cluster_many_queries(clipmi, gpu, topk_oracle, kind, Q):
    """4096 consecutive duplicates of the row that ranks first for every query: answered by the coarse path itself."""
    rng = np.random.default_rng(790 + Q)
    N = 100000
    db = unit_rows(rng, N, E)
    base = unit_rows(rng, 1, E)[0]
    db[30000:34096] = base
    db[77777] = base
    q = base[None, :] + 0.02 * unit_rows(rng, Q, E)
    q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    D, I = _run_coarse(clipmi, gpu, db, q, 51, kind=kind)
    Ds, Is = topk_oracle.topk(db, q, 51)
    _assert_exact(D, I, Ds, Is, f"{kind} duplicate cluster Q={Q}")
    assert (I[:, 0] == 30000).all() and (I[:, 50] == 30050).all()


@pytest.mark.parametrize("kind", KINDS)
def test_prepass_threshold_useless(clipmi, gpu, topk_oracle, kind):
    """The first 40 k rows - all of both sample levels - score about -125 against every query: the later segments accept
    every pair (70 k survivors per query, below the lists' 2^18: no fallback)."""
    rng = np.random.default_rng(801)
    N = 70001
    q = unit_rows(rng, 64, E)
    u = q.sum(axis=0); u /= np.linalg.norm(u)
    db = unit_rows(rng, N, E)
    db[:40000] = (-1000.0 * u)[None, :] * (1.0 + 1e-6 * np.arange(40000, dtype=np.float32))[:, None]
    D, I = _run_coarse(clipmi, gpu, db, q, 51, kind=kind)
    Ds, Is = topk_oracle.topk(db, q, 51)
    _assert_exact(D, I, Ds, Is, f"{kind} useless pre-pass threshold")
    assert (I >= 40000).all()


@pytest.mark.parametrize("kind", KINDS)
def test_anisotropic_rows(clipmi, gpu, topk_oracle, kind):
    rng = np.random.default_rng(4243)
    db = _anisotropic_rows(rng, 150000)
    q = _anisotropic_rows(rng, 64)
    D, I = _run_coarse(clipmi, gpu, db, q, 51, kind=kind)
    Ds, Is = topk_oracle.topk(db, q, 51)
    _assert_exact(D, I, Ds, Is, f"{kind} anisotropic")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("Q", [5, 64, 130])
def test_non_finite_queries_beside_ordinary_ones(clipmi, gpu, topk_oracle, kind, Q):
    """NaN / +inf / -inf / all-zero queries: no usable coarse bound (threshold -inf), the exact fallback answers the pass."""
    rng = np.random.default_rng(97 + Q)
    N = 70000
    db = (unit_rows(rng, N, E) * rng.uniform(0.2, 2.0, size=(N, 1))).astype(np.float32)
    q = unit_rows(rng, Q, E)
    q[1, 5] = np.nan
    q[2, 9] = np.inf
    q[3, 9] = -np.inf
    q[4, :] = 0.0
    if Q > 40:
        q[33, 700] = np.nan
        q[40, 0], q[40, 1] = np.inf, -np.inf
    D, I = _run_coarse(clipmi, gpu, db, q, 51, kind=kind)
    Ds, Is = topk_oracle.topk(db, q, 51)
    _assert_exact(D, I, Ds, Is, f"{kind} non-finite queries, Q = {Q}")
    assert (I[1] == -1).all() and (I[0] >= 0).all()


@pytest.mark.parametrize("poison", ["nan", "inf"])
def test_non_finite_row_keeps_the_index_on_the_exact_scan(clipmi, gpu, topk_oracle, poison):
    rng = np.random.default_rng(29)
    db = unit_rows(rng, 70000, E)
    db[4321, 700] = np.nan if poison == "nan" else np.inf
    idx = clipmi.IndexFlatIP(E, device=gpu, coarse="int8")
    idx.add(db)
    assert idx.uses_coarse()
    for Q in (3, 200):
        q = np.abs(unit_rows(rng, Q, E)) + 0.01
        D, I = idx.search(q, 20)
        Ds, Is = topk_oracle.topk(db, q, 20)
        _assert_exact(D, I, Ds, Is, f"{poison} row, Q = {Q}")
    assert not np.isfinite(idx.matrix_i8()[3]) or not np.isfinite(idx.matrix_i8()[2])
    if poison == "nan":
        assert 4321 not in I


@pytest.mark.parametrize("kind", KINDS)
def test_overflow_falls_back_to_exact(clipmi, gpu, topk_oracle, kind):
    rng = np.random.default_rng(80)
    N = 300000
    v = unit_rows(rng, 1, E)
    db = np.repeat(v, N, axis=0)
    db[123456] *= np.float32(1.5)
    q = unit_rows(rng, 2, E)
    D, I = _run_coarse(clipmi, gpu, db, q, 20, kind=kind)
    Ds, Is = topk_oracle.topk(db, q, 20)
    _assert_exact(D, I, Ds, Is, f"{kind} overflow fallback")


def _hook_survivors(clipmi, gpu, idx, q, K, kind="int8"):
    """(ids of the measurement hook's last call, exactly re-scored rows per query) - clipmi_dbg_topk_coarse*_scan_ms."""
    L = clipmi._lib.lib()
    N, Q = idx.ntotal, q.shape[0]
    dbt = idx.matrix()
    qd = torch.from_numpy(q).to(gpu)
    os_ = torch.empty((Q, K), dtype=torch.float32, device=gpu)
    oi_ = torch.empty((Q, K), dtype=torch.int64, device=gpu)
    need = L.clipmi_topk_ip_coarse_workspace_bytes(N, E, Q, K)
    assert need > 0, clipmi._lib.last_error()
    ws = torch.empty(need, dtype=torch.uint8, device=gpu)
    ms, surv = C.c_float(0), C.c_longlong(-1)
    if kind == "int8":
        db8, meta, amax, rmax = idx.matrix_i8()
        rc = L.clipmi_dbg_topk_coarse_i8_scan_ms(dbt.data_ptr(), db8.data_ptr(), meta.data_ptr(), amax, N, E, rmax,
                                                 qd.data_ptr(), Q, K, os_.data_ptr(), oi_.data_ptr(), ws.data_ptr(), ws.numel(),
                                                 None, 1, C.byref(ms), C.byref(surv))
    else:
        dbh, rmax = idx.matrix_bf16()
        rc = L.clipmi_dbg_topk_coarse_scan_ms(dbt.data_ptr(), dbh.data_ptr(), N, E, rmax, qd.data_ptr(), Q, K,
                                              os_.data_ptr(), oi_.data_ptr(), ws.data_ptr(), ws.numel(), None, 1,
                                              C.byref(ms), C.byref(surv))
    clipmi._lib.check(rc, "coarse scan hook")
    torch.cuda.synchronize()
    return oi_.cpu().numpy(), surv.value / Q


def test_int8_coarse_filter_really_filters_at_768(clipmi, gpu, topk_oracle):
    """A condition, not a measurement: at N = 200 000 unit rows, Q = 64, K = 51 the int8 scan must leave fewer than N / 16
    exactly re-scored rows per query (tests/test_topk_e768.py's numpy restatement predicts 1.1 - 1.4 k fresh survivors + the K
    kept heads per segment: ~8 x below the cap; a broken bound or a permanent fallback crosses it). The anisotropic
    figure is printed beside it without a cap."""
    N, Q, K = 200_000, 64, 51
    report = {}
    for name, gen in (("isotropic", unit_rows), ("anisotropic", _anisotropic_rows)):
        rng = np.random.default_rng(4242)
        db = gen(rng, N, E)
        q = gen(rng, Q, E)
        idx = clipmi.IndexFlatIP(E, device=gpu, coarse="int8")
        idx.add(db)
        assert idx.uses_coarse()
        ids, per_q = _hook_survivors(clipmi, gpu, idx, q, K)
        Ds, Is = topk_oracle.topk(db, q, K)
        assert np.array_equal(ids, Is), name
        report[name] = per_q
    print(f"int8, E = 768: exactly re-scored rows per query (N={N}, K={K}): isotropic {report['isotropic']:.0f}, "
          f"anisotropic {report['anisotropic']:.0f}")
    assert report["isotropic"] < N / 16


def test_bf16_scan_hook_accepts_768(clipmi, gpu, topk_oracle):
    rng = np.random.default_rng(4244)
    N, Q, K = 100_000, 33, 51
    db, q = unit_rows(rng, N, E), unit_rows(rng, Q, E)
    idx = clipmi.IndexFlatIP(E, device=gpu, coarse="bf16")
    idx.add(db)
    ids, per_q = _hook_survivors(clipmi, gpu, idx, q, K, kind="bf16")
    Ds, Is = topk_oracle.topk(db, q, K)
    assert np.array_equal(ids, Is)
    print(f"bf16, E = 768: exactly re-scored rows per query (N={N}, K={K}): {per_q:.0f}")
    assert per_q < (1 << 18)


def test_quantize_rows_i8_matches_numpy_at_768(clipmi, gpu):
    rng = np.random.default_rng(81)
    N = 1000
    x = (unit_rows(rng, N, E) * rng.uniform(0.1, 3.0, size=(N, 1))).astype(np.float32)
    x[7] = 0.0
    x[32:64] = 0.0
    idx = clipmi.IndexFlatIP(E, device=gpu, coarse="int8")
    idx.add(x)
    q8, meta, amax, rmax = idx.matrix_i8()
    torch.cuda.synchronize()
    L = clipmi._lib.lib()
    N32 = (N + 31) // 32 * 32
    nblk = N32 // 32
    assert q8.numel() == L.clipmi_i8_copy_bytes(N, E) == N32 * E
    assert meta.numel() * 4 == L.clipmi_i8_meta_bytes(N) == ((N32 + 32) + (nblk + 1)) * 8 + (N32 + 32) * 4
    q8, meta = q8.cpu().numpy(), meta.cpu().numpy()
    rmeta = meta[:2 * (N32 + 32)].reshape(-1, 2)
    bmeta = meta[2 * (N32 + 32):2 * (N32 + 32) + 2 * (nblk + 1)].reshape(-1, 2)
    slot_rows = meta[2 * (N32 + 32) + 2 * (nblk + 1):].view(np.uint32)
    perm = np.argsort(np.abs(x).max(axis=1), kind="stable")
    assert np.array_equal(slot_rows[:N], perm.astype(np.uint32)) and (slot_rows[N:N32] == 0xffffffff).all()
    xp = np.zeros((N32, E), np.float32)
    xp[:N] = x[perm]
    s = np.abs(xp).reshape(nblk, -1).max(axis=1) / np.float32(127.0)
    s[s == 0] = 1.0
    s = s.astype(np.float32)
    srow = np.repeat(s, 32)
    assert np.array_equal(rmeta[:N32, 0], srow) and np.array_equal(bmeta[:nblk, 0], s)
    ref = np.clip(np.rint(xp * (np.float32(1.0) / srow)[:, None]), -127, 127).astype(np.int8)
    # un-tile: [blk][24 k-steps][h][r][16] -> [blk*32 + r][32 ks + 16 h + b]
    got = q8.reshape(nblk, 24, 2, 32, 16).transpose(0, 3, 1, 2, 4).reshape(N32, E)
    assert np.array_equal(got, ref)
    err = np.linalg.norm(xp.astype(np.float64) - srow[:, None].astype(np.float64) * got.astype(np.float64), axis=1)
    assert (rmeta[:N, 1] >= err[:N]).all() and (rmeta[:N, 1] <= err[:N] * 1.002 + 1e-12).all()
    assert (rmeta[N:, 1] == 0).all() and (rmeta[N32:] == 0).all() and (bmeta[nblk:] == 0).all()
    assert np.array_equal(bmeta[:nblk, 1], rmeta[:N32, 1].reshape(nblk, 32).max(axis=1))
    assert amax >= rmeta[:, 1].max() and rmax >= np.linalg.norm(x, axis=1).max()


def test_sharded_equals_single_at_768(clipmi, gpu, topk_oracle):
    """300 000 x 768 rows in 8 contiguous shards, coarse kinds alternating (shards of 37 500 rows answer with the exact scan
    whatever was asked; the same rows in 4 shards of 75 000 go through the coarse copies): clipmi_merge_topk of the parts ==
    the single exact search == the oracle's merge. Duplicates planted across shard boundaries."""
    rng = np.random.default_rng(21)
    N, Q, K = 300000, 16, 51
    db = torch.from_numpy(unit_rows(rng, N, E)).to(gpu)
    q = unit_rows(rng, Q, E)
    db[N // 8] = db[5]
    db[N // 4] = db[5]
    db[N - 1] = db[5]
    full = clipmi.IndexFlatIP(E, device=gpu)
    full.add(db)
    D, I = full.search(q, K)
    L = clipmi._lib.lib()
    for R in (8, 4):
        parts_s, parts_i = [], []
        for r in range(R):
            lo, hi = clipmi.shard_bounds(N, R, r)
            sh = clipmi.IndexFlatIP(E, device=gpu, coarse="bf16" if r % 2 else "int8")
            sh.add(db[lo:hi])
            sh.id_base = lo
            assert sh.uses_coarse() == (R == 4)
            s, i = sh.search(q, K)
            parts_s.append(s)
            parts_i.append(i)
        S = torch.from_numpy(np.stack(parts_s)).to(gpu)
        Iall = torch.from_numpy(np.stack(parts_i)).to(gpu)
        out_s = torch.empty((Q, K), dtype=torch.float32, device=gpu)
        out_i = torch.empty((Q, K), dtype=torch.int64, device=gpu)
        ws = torch.empty(256, dtype=torch.uint8, device=gpu)
        rc = L.clipmi_merge_topk(S.data_ptr(), Iall.data_ptr(), R, Q, K, out_s.data_ptr(), out_i.data_ptr(),
                                 ws.data_ptr(), ws.numel(), None)
        clipmi._lib.check(rc, "merge")
        _assert_exact(out_s.cpu().numpy(), out_i.cpu().numpy(), D, I, f"{R} shards vs single")
        Ms, Mi = topk_oracle.merge(np.stack(parts_s), np.stack(parts_i), K)
        _assert_exact(out_s.cpu().numpy(), out_i.cpu().numpy(), Ms, Mi, f"{R} shards: merge vs oracle merge")
    Ds, Is = topk_oracle.topk(db.cpu().numpy(), q[:4], K)
    _assert_exact(D[:4], I[:4], Ds, Is, "single exact search vs oracle")


def test_full_size_10m_x_768_properties(clipmi, gpu, topk_oracle):
    """10 M x 768 (30.7 GB f32 + 7.7 GB int8 / 15.4 GB bf16), Q = 64, K = 51, generated on the device: int8 coarse == bf16
    coarse == exact f32 scan bit for bit; returned scores equal the oracle's scores of those rows; no row of a 200 000-row
    random subset beats the K-th score; one call of Q = 1024 (sixteen 64-query passes on two streams) equals the exact scan on
    the first 64 and on 32 more queries."""
    N, Q, K = 10_000_000, 64, 51
    g = torch.Generator(device=gpu); g.manual_seed(42)
    db = torch.empty((N, E), dtype=torch.float32, device=gpu)
    for s in range(0, N, 1 << 20):
        e = min(N, s + (1 << 20))
        blk = torch.randn((e - s, E), generator=g, device=gpu)
        db[s:e] = blk / blk.norm(dim=1, keepdim=True)
    del blk
    db[N - 1] = db[17]
    q = torch.randn((Q, E), generator=g, device=gpu)
    q = q / q.norm(dim=1, keepdim=True)
    q[3] = db[17]
    exact = clipmi.IndexFlatIP(E, device=gpu); exact.add(db)
    De, Ie = exact.search(q, K)
    coarse = clipmi.IndexFlatIP(E, device=gpu, coarse="bf16"); coarse.add(db)
    assert coarse.uses_coarse()
    Dc, Ic = coarse.search(q, K)
    _assert_exact(Dc, Ic, De, Ie, "bf16 coarse vs exact at 10M x 768")
    del coarse
    torch.cuda.empty_cache()
    coarse8 = clipmi.IndexFlatIP(E, device=gpu, coarse="int8"); coarse8.add(db)
    assert coarse8.uses_coarse()
    D8, I8 = coarse8.search(q, K)
    _assert_exact(D8, I8, De, Ie, "int8 coarse vs exact at 10M x 768")
    assert list(Ie[3, :2]) == [17, N - 1] and De[3, 0] == De[3, 1]
    qh = q.cpu().numpy()
    for j in (0, 3, 31, 63):
        rows = Ie[j]
        assert len(set(rows.tolist())) == K
        sc = topk_oracle.scores(db[torch.from_numpy(rows).to(gpu)].cpu().numpy(), qh[j])
        assert np.array_equal(sc.view(np.uint32), De[j].view(np.uint32))
        order = np.lexsort((rows, -De[j].astype(np.float64)))
        assert np.array_equal(order, np.arange(K))
    rng = np.random.default_rng(7)
    sub = np.sort(rng.choice(N, 200_000, replace=False))
    subdb = db[torch.from_numpy(sub).to(gpu)].cpu().numpy()
    for j in (0, 63):
        sc = topk_oracle.scores(subdb, qh[j])
        inside = set(Ie[j].tolist())
        better = [(s_, int(i_)) for s_, i_ in zip(sc, sub) if int(i_) not in inside and
                  (s_ > De[j, -1] or (s_ == De[j, -1] and i_ < Ie[j, -1]))]
        assert not better, better[:3]
    qw = torch.cat([q, torch.randn((960, E), generator=g, device=gpu)])
    qw[64:] = qw[64:] / qw[64:].norm(dim=1, keepdim=True)
    Dw, Iw = coarse8.search(qw, K)
    _assert_exact(Dw[:64], Iw[:64], De, Ie, "Q = 1024 vs exact at full size, first 64 queries")
    pick = torch.arange(64, 1024, 31, device=gpu)[:32]
    Dx, Ix = exact.search(qw[pick], K)
    _assert_exact(Dw[pick.cpu().numpy()], Iw[pick.cpu().numpy()], Dx, Ix, "Q = 1024 vs exact at full size, 32 more")
