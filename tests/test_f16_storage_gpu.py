"""-m gpu: an index kept in fp16 - clipmi_rows_to_f16, clipmi_topk_ip / clipmi_topk_ip_rows with CLIPMI_F16, IndexFlatIP(storage=
"f16"), its subsets, files and shards - bit for bit against numpy's conversion and oracle/topk_oracle.c.

The reference of every search is topk_oracle.topk(h, q, K) with h = db.astype(float16).astype(float32): fp16 -> f32 is exact and
the scan runs the f32 form's own fmaf chain on the converted values, so the unchanged oracle is the bit-exact reference
(tests/test_f16_storage.py pins that it answers with OTHER score bits on db itself). Compared as tests/test_topk_subset_gpu.py
compares: uint32 view of the scores, ids, every slot; outputs of the C-ABI calls pre-filled with NaN / -7.

One seeded database of 131 101 unit rows per width, built like that file's (rows 0 .. 65 535 near-copies of query 0, a run of 200
identical rows and a far copy, NaN / +inf / -inf components at six rows) plus twelve rows with components of 65 504, +-2^-24
and -0 (fp16's largest finite value, its smallest subnormals, the signed zero). Converted once, by clipmi_rows_to_f16."""
import numpy as np
import pytest
import torch

import test_f16_storage as fs
import test_topk_krange as kr
import ws_cases as W
from conftest import unit_rows

pytestmark = pytest.mark.gpu

FMAX = np.finfo(np.float32).max
NMAX, QMAX = 131101, 65
BIG_BASE = 2 ** 40 + 5
RUN_LO, RUN_HI, RUN_FAR = 30000, 30200, 130000
SPECIAL = (6000, 6002, 6004, 100000, 100002, 100004)
EDGE_ROWS = tuple(range(7000, 7006)) + tuple(range(120000, 120006))
LEAD = 65536
G = 64

_data, _dev, _ref, _idx = {}, {}, {}, {}


def _rows(E):
    """(db f32, h = f32(f16(db)), q)"""
    if E not in _data:
        rng = np.random.default_rng(61000 + E)
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
        for j, r in enumerate(EDGE_ROWS):
            db[r, 3 + j] = (65504.0, -65504.0)[j & 1]
            db[r, 40 + j::16][:8] = (2.0 ** -24, -2.0 ** -24, -0.0, 2.0 ** -24 * 3, -2.0 ** -14, 2.0 ** -25 * 1.5, -2.0 ** -26, 0.0)
        with np.errstate(over="ignore"):
            h = db.astype(np.float16).astype(np.float32)
        for a in (db, h, q):
            a.setflags(write=False)
        _data[E] = (db, h, q)
    return _data[E]


def _convert(clipmi, gpu, x, counts=None, out=None):
    """clipmi_rows_to_f16 through the C ABI on a device f32 tensor -> device fp16 tensor."""
    L, lib = clipmi._lib.lib(), clipmi._lib
    out = torch.empty(x.shape, dtype=torch.float16, device=gpu) if out is None else out
    lib.check(L.clipmi_rows_to_f16(x.data_ptr(), x.shape[0], x.shape[1], out.data_ptr(), counts.data_ptr() if counts is not None else None,
                                   lib.stream_ptr(gpu)), "clipmi_rows_to_f16")
    return out


def _dev16(clipmi, gpu, E):
    """The database's fp16 matrix on the device, inside a larger tensor whose G rows in front and G rows behind are
    fp16(1000 q[0]): a row read outside [G, G + N) shows as a wrong best hit of query 0. -> (whole tensor, counts)"""
    if E not in _dev:
        db, _, q = _rows(E)
        whole = torch.empty((NMAX + 2 * G, E), dtype=torch.float16, device=gpu)
        guard = torch.from_numpy((1000.0 * q[0]).astype(np.float16)).to(gpu)
        whole[:G] = guard
        whole[G + NMAX:] = guard
        counts = torch.zeros(2, dtype=torch.int64, device=gpu)
        _convert(clipmi, gpu, torch.from_numpy(db.copy()).to(gpu), counts, out=whole[G:G + NMAX])
        torch.cuda.synchronize()
        _dev[E] = (whole, counts.cpu().numpy().copy())
    return _dev[E]


def _db16(clipmi, gpu, E, N=NMAX):
    return _dev16(clipmi, gpu, E)[0][G:G + N]


def _want(topk_oracle, E, N, Q, K, id_base=0, rows=None, key=None, src=1):
    """The oracle on h[:N] (rows: on h[rows], positions mapped back), for the first Q of the queries. key: cache per (E, key, K)."""
    q = _rows(E)[2]
    k = (E, key, K, src)
    if key is None or k not in _ref:
        m = _rows(E)[src]
        m = m[:N] if rows is None else (m[rows] if len(rows) else np.empty((0, E), np.float32))
        res = topk_oracle.topk(m, q if key is not None else q[:Q], K)
        if key is None:
            D, P = res
            return _ids(D, P, rows, id_base)
        _ref[k] = res
    D, P = _ref[k]
    return _ids(D[:Q].copy(), P[:Q], rows, id_base)


def _ids(D, P, rows, id_base):
    if rows is not None:
        rows = np.asarray(rows, dtype=np.int64)
        P = np.where(P >= 0, rows[np.maximum(P, 0)] if rows.size else -1, -1)
    return D, np.where(P >= 0, P + id_base, -1).astype(np.int64)


def _assert_exact(D, I, Ds, Is, tag):
    assert D.shape == Ds.shape and I.shape == Is.shape, (tag, D.shape, Ds.shape)
    bad = np.nonzero((I != Is) | (D.view(np.uint32) != Ds.view(np.uint32)))
    assert bad[0].size == 0, (f"{tag}: {bad[0].size} mismatching slots, first at q={bad[0][0]} k={bad[1][0]}: "
                              f"got ({D[bad[0][0], bad[1][0]]!r}, {I[bad[0][0], bad[1][0]]}) "
                              f"want ({Ds[bad[0][0], bad[1][0]]!r}, {Is[bad[0][0], bad[1][0]]})")


def _abi(clipmi, gpu, db_dev, dtype, N, E, q, K, id_base=0, lst=None):
    """clipmi_topk_ip (lst None) or clipmi_topk_ip_rows through the C ABI with a workspace of exactly the stated size and outputs
    pre-filled with NaN / -7."""
    L, lib = clipmi._lib.lib(), clipmi._lib
    Q = q.shape[0]
    M = N if lst is None else len(lst)
    need = L.clipmi_topk_ip_workspace_bytes(M, E, Q, K)
    assert 0 < need <= kr.GIB2, lib.last_error()
    assert lst is None or need == L.clipmi_topk_ip_rows_workspace_bytes(M, E, Q, K)
    ws = torch.empty(need, dtype=torch.uint8, device=gpu)
    qd = torch.from_numpy(np.ascontiguousarray(q, dtype=np.float32)).to(gpu)
    out_s = torch.full((Q, K), float("nan"), dtype=torch.float32, device=gpu)
    out_i = torch.full((Q, K), -7, dtype=torch.int64, device=gpu)
    tail = (qd.data_ptr(), Q, K, id_base, out_s.data_ptr(), out_i.data_ptr(), ws.data_ptr(), ws.numel(), lib.stream_ptr(gpu))
    if lst is None:
        lib.check(L.clipmi_topk_ip(db_dev.data_ptr(), dtype, N, E, *tail), "clipmi_topk_ip")
    else:
        ld = torch.from_numpy(np.ascontiguousarray(lst, dtype=np.uint32).view(np.int32).copy()).to(gpu)
        lib.check(L.clipmi_topk_ip_rows(db_dev.data_ptr(), dtype, N, E, ld.data_ptr() if M else None, M, *tail), "clipmi_topk_ip_rows")
    torch.cuda.synchronize()
    return out_s.cpu().numpy(), out_i.cpu().numpy()


def _parent(clipmi, gpu, E):
    """IndexFlatIP(storage="f16") over the database, added in three uneven chunks."""
    if E not in _idx:
        idx = clipmi.IndexFlatIP(E, device=gpu, storage="f16")
        db = _rows(E)[0]
        for lo, hi in ((0, 1), (1, 70002), (70002, NMAX)):
            idx.add(db[lo:hi])
        _idx[E] = idx
    return _idx[E]


# ---- 1. the conversion ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", kr.WIDTHS)
def test_conversion_equals_numpy(clipmi, gpu, E):
    """The whole database and the edge-value rows (ties both ways, the subnormal seam, 65 519.996, +-65 520 -> inf) against
    numpy.astype(float16) bit for bit, both counters against numpy's, a second call ADDING to them, counts NULL, and N = 1, 3,
    1 001 rows into a buffer whose following row must stay untouched."""
    db = _rows(E)[0]
    whole, cnt = _dev16(clipmi, gpu, E)
    with np.errstate(over="ignore"):
        want = db.astype(np.float16)
    got = whole[G:G + NMAX].cpu().numpy()
    assert (got.view(np.uint16) == want.view(np.uint16)).all()
    assert tuple(cnt) == fs.counts(db) and cnt[1] == 0 and cnt[0] > NMAX * E // 2
    assert (whole[:G].cpu().numpy() == whole[G + NMAX:].cpu().numpy()).all()            # the guard rows were not written

    x = fs.edge_rows(E, with_overflow=True)
    xd = torch.from_numpy(x).to(gpu)
    counts = torch.zeros(2, dtype=torch.int64, device=gpu)
    out = _convert(clipmi, gpu, xd, counts)
    with np.errstate(over="ignore"):
        want = x.astype(np.float16)
    assert (out.cpu().numpy().view(np.uint16) == want.view(np.uint16)).all()
    c = fs.counts(x)
    assert tuple(counts.cpu().numpy()) == c and c[1] > 0
    _convert(clipmi, gpu, xd, counts)
    assert tuple(counts.cpu().numpy()) == (2 * c[0], 2 * c[1])
    assert (_convert(clipmi, gpu, xd).cpu().numpy().view(np.uint16) == want.view(np.uint16)).all()

    for N in (1, 3, 1001):
        buf = torch.full((N + 1, E), 0.3333, dtype=torch.float16, device=gpu)
        counts.zero_()
        _convert(clipmi, gpu, torch.from_numpy(db[5990:5990 + N].copy()).to(gpu), counts, out=buf[:N])
        got = buf.cpu().numpy()
        with np.errstate(over="ignore"):
            assert (got[:N].view(np.uint16) == db[5990:5990 + N].astype(np.float16).view(np.uint16)).all()
        assert (got[N] == np.float16(0.3333)).all() and tuple(counts.cpu().numpy()) == fs.counts(db[5990:5990 + N])


# ---- 2. the plain scan through the C ABI ------------------------------------------------------------------------------------------
PLAIN = [(N, 33) for N in (1, 15, 16, 17, 4099, 70001, NMAX)] + [(70001, Q) for Q in (1, 16, 17, 32, 65)]


@pytest.mark.parametrize("E", kr.WIDTHS)
@pytest.mark.parametrize("N,Q", PLAIN)
def test_plain_scan(clipmi, gpu, topk_oracle, E, N, Q):
    """Rows around one 16-row tile (pads behind N), several blocks without and with the pre-pass, one and two column groups full
    and ragged, several passes. id_base = 1000; N = 4 099 carries 2^40 + 5."""
    p = kr.make_plan(N, E, Q, 51)
    assert p["sample"] == (N >= kr.SAMPLE_MIN_N)
    base = BIG_BASE if N == 4099 else 1000
    D, I = _abi(clipmi, gpu, _db16(clipmi, gpu, E, N), clipmi._lib.F16, N, E, _rows(E)[2][:Q], 51, id_base=base)
    Ds, Is = _want(topk_oracle, E, N, Q, 51, id_base=base, key=("plain", N))
    _assert_exact(D, I, Ds, Is, f"plain E={E} N={N} Q={Q}")
    if N < 51:
        assert (I[:, N:] == -1).all() and (D[:, N:] == -FMAX).all()
    assert not np.isnan(D).any()


@pytest.mark.parametrize("E", kr.WIDTHS)
@pytest.mark.parametrize("case", ["K=1", "Kmax", "Kmax, fewer rows than K"])
def test_plain_scan_k_range(clipmi, gpu, topk_oracle, E, case):
    kmax = kr.KMAX[E]
    K = 1 if case == "K=1" else kmax
    N = kmax - 7 if "fewer" in case else 70001
    q = _rows(E)[2][1:4]
    D, I = _abi(clipmi, gpu, _db16(clipmi, gpu, E, N), clipmi._lib.F16, N, E, q, K)
    Ds, Is = topk_oracle.topk(_rows(E)[1][:N], q, K)
    _assert_exact(D, I, Ds, Is, f"{case} E={E}")
    if "fewer" in case:
        nan_rows = sum(r < N for r in SPECIAL[::3])
        assert (I[:, N:] == -1).all() and (D[:, N:] == -FMAX).all() and ((I >= 0).sum(axis=1) == N - nan_rows).all()


# ---- 3. nothing outside the matrix is read; the pitch is 2 E --------------------------------------------------------------------
@pytest.mark.parametrize("E", kr.WIDTHS)
@pytest.mark.parametrize("N", [17, 70001])
def test_guard_rows_are_never_read(clipmi, gpu, topk_oracle, E, N):
    """The matrix is rows [G, G + N) of a larger fp16 tensor; the row in front of it and the row behind it are fp16(1000 q[0]). A
    stray row - a wrong pitch, a tile read past N, a list entry used unclamped - is a hit of query 0 with a score near 1000
    that the oracle does not have. Plain form and list form (every second row and the last one)."""
    whole, _ = _dev16(clipmi, gpu, E)
    view = whole[G:G + N]
    if N < NMAX:                                            # put the guard directly behind row N - 1 for the time of the test
        saved = whole[G + N:G + N + G].clone()
        whole[G + N:G + N + G] = whole[:G]
    try:
        q = _rows(E)[2][:33]
        D, I = _abi(clipmi, gpu, view, clipmi._lib.F16, N, E, q, 51)
        lst = np.unique(np.concatenate([np.arange(0, N, 2), [N - 1]]))
        Dl, Il = _abi(clipmi, gpu, view, clipmi._lib.F16, N, E, q, 51, lst=lst)
    finally:
        if N < NMAX:
            whole[G + N:G + N + G] = saved
    _assert_exact(D, I, *_want(topk_oracle, E, N, 33, 51, key=("plain", N)), f"guarded plain E={E} N={N}")
    _assert_exact(Dl, Il, *_want(topk_oracle, E, N, 33, 51, rows=lst), f"guarded list E={E} N={N}")


# ---- 4. the list form -----------------------------------------------------------------------------------------------------------
def _shape_rows(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "contiguous":
        return np.arange(4099, 74100)                                      # M = 70 001: the pre-pass runs
    if name == "every second":
        return np.arange(0, 40000, 2)
    if name == "random 1 in 50":
        pick = np.flatnonzero(rng.random(NMAX) < 0.02)
        return np.unique(np.concatenate([pick, [0, NMAX - 1], SPECIAL, EDGE_ROWS]))
    if name.startswith("M="):
        M = int(name[2:])
        return np.sort(rng.choice(NMAX, M, replace=False)) if M else np.empty(0, np.int64)
    assert name == "all rows"
    return np.arange(NMAX)


SHAPES = ("contiguous", "every second", "random 1 in 50", "M=0", "M=1", "M=15", "M=16", "M=17", "all rows")


@pytest.mark.parametrize("E", kr.WIDTHS)
@pytest.mark.parametrize("shape", SHAPES, ids=[s.replace(" ", "_") for s in SHAPES])
def test_subsets_of_an_fp16_index(clipmi, gpu, topk_oracle, E, shape):
    """index.subset(rows) on an fp16 parent, Q = 1 and 33, K = 51; "all rows" also equals the parent's own search bit for bit."""
    rows = _shape_rows(shape)
    M = len(rows)
    assert kr.make_plan(M, E, 33, 51)["sample"] == (shape in ("contiguous", "all rows"))
    parent = _parent(clipmi, gpu, E)
    sub = parent.subset(rows)
    sub.id_base = 1000
    assert sub.ntotal == M
    q = _rows(E)[2]
    for Q in (1, 33):
        D, I = sub.search(q[:Q], 51)
        Ds, Is = _want(topk_oracle, E, NMAX, Q, 51, id_base=1000, rows=None if shape == "all rows" else rows,
                       key=("plain", NMAX) if shape == "all rows" else ("list", shape))
        _assert_exact(D, I, Ds, Is, f"{shape} E={E} Q={Q}")
        if M < 51:
            assert (I[:, M:] == -1).all() and (D[:, M:] == -FMAX).all()
        if shape == "all rows":
            parent.id_base = 1000
            try:
                Dp, Ip = parent.search(q[:Q], 51)
            finally:
                parent.id_base = 0
            _assert_exact(D, I, Dp, Ip, f"all rows against the parent's search E={E} Q={Q}")


@pytest.mark.parametrize("E", kr.WIDTHS)
def test_list_entries_past_the_matrix_are_skipped(clipmi, gpu, topk_oracle, E):
    """C ABI only: N = 5 000 of the database's rows is passed and the list holds valid entries, entries in [N, allocation) - rows
    that exist in memory, the near-copies of query 0 among them - and 0xFFFFFFFE. Expected: the oracle over the valid entries."""
    rng = np.random.default_rng(700 + E)
    N = 5000
    valid = np.unique(np.concatenate([rng.choice(N - 1, 2999, replace=False), [N - 1]]))
    invalid = np.sort(rng.choice(np.arange(N, NMAX), 1503, replace=False))
    invalid[-1] = 0xFFFFFFFE
    lst = np.concatenate([valid, invalid])
    assert len(lst) % 16 != 0 and len(lst) <= N
    q = _rows(E)[2][:3]
    D, I = _abi(clipmi, gpu, _db16(clipmi, gpu, E, N), clipmi._lib.F16, N, E, q, 51, id_base=1000, lst=lst)
    _assert_exact(D, I, *_want(topk_oracle, E, N, 3, 51, id_base=1000, rows=valid), f"entries >= N, E={E}")
    assert np.isin(I - 1000, valid).all()


# ---- 5. IndexFlatIP(storage="f16") end to end -------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", kr.WIDTHS)
def test_index_end_to_end(clipmi, gpu, topk_oracle, E, tmp_path):
    db, h, q = _rows(E)
    idx = _parent(clipmi, gpu, E)
    # add in three chunks = the one-shot conversion, counts included
    whole, cnt = _dev16(clipmi, gpu, E)
    m = idx.matrix_f16()
    assert m.dtype == torch.float16 and m.shape == (NMAX, E) and idx.ntotal == NMAX
    assert torch.equal(m.view(torch.int16), whole[G:G + NMAX].view(torch.int16))
    assert (idx.f16_changed, idx.f16_overflowed) == (int(cnt[0]), 0) and not idx.uses_coarse()
    up = idx.matrix()
    assert up.dtype == torch.float32 and (up[6000:7010].cpu().numpy().view(np.uint32) == h[6000:7010].view(np.uint32)).all()
    del up
    # the search is the oracle's on h, and not the f32 index's
    D, I = idx.search(q[:33], 51)
    _assert_exact(D, I, *_want(topk_oracle, E, NMAX, 33, 51, key=("plain", NMAX)), f"fp16 index E={E}")
    f32 = clipmi.IndexFlatIP(E, device=gpu)
    f32.add(db)
    Df, If = f32.search(q[:33], 51)
    _assert_exact(Df, If, *_want(topk_oracle, E, NMAX, 33, 51, key=("f32", NMAX), src=0), f"f32 index E={E}")
    differ = float((D.view(np.uint32) != Df.view(np.uint32)).mean())
    print(f"E={E}: fp16 and f32 index differ in the score bits of {differ:.4f} of the slots")
    assert differ >= 0.5
    # rows that are fp16 values already: the two kinds of index agree bit for bit, and nothing was changed
    f32 = clipmi.IndexFlatIP(E, device=gpu)
    f32.add(h)
    f16 = clipmi.IndexFlatIP(E, device=gpu, storage="f16")
    f16.add(h)
    assert f16.f16_changed == 0 and torch.equal(f16.matrix_f16().view(torch.int16), m.view(torch.int16))
    Dh, Ih = f32.search(q[:33], 51)
    _assert_exact(Dh, Ih, D, I, f"f32 index of fp16-representable rows E={E}")
    _assert_exact(*f16.search(q[:33], 51), D, I, f"fp16 index of fp16-representable rows E={E}")
    del f32, f16
    # file round trip on the GPU, whole and as two shards
    path = str(tmp_path / "images.index")
    clipmi.write_index(idx, path)
    assert clipmi.index.index_rows(path) == (NMAX, E)
    back = clipmi.read_index(path, device=gpu)
    assert back.storage == "f16" and back.f16_changed == 0 and torch.equal(back.matrix_f16().view(torch.int16), m.view(torch.int16))
    _assert_exact(*back.search(q[:33], 51), D, I, f"read back E={E}")
    del back
    parts = []
    for r in range(2):
        lo, hi = clipmi.shard_bounds(NMAX, 2, r)
        shard = clipmi.read_index(path, device=gpu, rows=(lo, hi))
        assert (shard.storage, shard.ntotal, shard.id_base, shard.n_file) == ("f16", hi - lo, lo, NMAX)
        parts.append(shard.search(q[:33], 51))
    Dm, Im = clipmi.merge_lists_host(np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts]), 51)
    _assert_exact(Dm, Im, D, I, f"two shards merged E={E}")


class _TextModel:
    context_length = 77

    def __init__(self, vec):
        self.vec = vec

    def encode_text(self, tokens):
        return torch.from_numpy(self.vec.copy())


def test_repl_answers_from_a_version_2_file(clipmi, gpu, topk_oracle, tmp_path, monkeypatch):
    """What CLIPMI_STORAGE=f16 query-index.py does after its model is loaded: read_index(storage=storage_from_env()) of a
    version-2 images.index, .coarse assigned as repl.main assigns it, then the prompt loop - whole, and over the CLIPMI_WITHIN
    subset. The printed lines are the oracle's list on the fp16 rows in the reference's format."""
    rng = np.random.default_rng(10)
    vecs = unit_rows(rng, 300, 512)
    keys = [f"dir{'ABC'[i % 3]}/{i:04d}.jpg" for i in range(300)]
    db = clipmi.store.VectorStore(str(tmp_path / "vectors"), dim=512, backend="packed")
    db.put_vectors(keys, vecs)
    mat, paths = db.assemble()
    built = clipmi.IndexFlatIP(512, device=gpu, storage="f16")
    built.add(mat)
    path = str(tmp_path / "images.index")
    clipmi.write_index(built, path)
    assert open(path, "rb").read(12) == b"CLIPMIIX" + (2).to_bytes(4, "little")
    index = clipmi.read_index(path, device=gpu, storage=clipmi.index.storage_from_env({"CLIPMI_STORAGE": "f16"}))
    index.coarse = "int8"
    assert index.storage == "f16" and not index.uses_coarse()
    h = np.asarray(mat, np.float32).astype(np.float16).astype(np.float32)
    monkeypatch.setattr(clipmi.tokenizer, "tokenize", lambda texts, context_length=77: texts)
    tv = unit_rows(rng, 1, 512)
    f = clipmi.repl.normalize(tv)
    rows = clipmi.repl.within_rows(db, "dirB/")
    for target, sel in ((index, np.arange(300)), (index.subset(rows), np.asarray(rows))):
        it, lines = iter(["a photo", "q"]), []
        clipmi.repl.repl(_TextModel(tv), target, db, inp=lambda p: next(it), out=lines.append)
        D, P = topk_oracle.topk(h[sel], f, 51)
        want = [f"{D[0][j]:.4f} {sel[P[0][j]]} {paths[sel[P[0][j]]].decode()}" for j in range(51) if j > 0 and P[0][j] >= 0]
        assert [l for l in lines if not l.startswith("Search time")] == want and len(want) == 50
    db.close()


# ---- 6. workspace independence ----------------------------------------------------------------------------------------------------
class F16Search:
    """One clipmi_topk_ip / clipmi_topk_ip_rows call with CLIPMI_F16 for tests/ws_cases.py's harness"""

    def __init__(self, clipmi, gpu, E, N, q, K, lst=None):
        self.lib, self.L, self.gpu = clipmi._lib, clipmi._lib.lib(), gpu
        self.db, self.E, self.N, self.Q, self.K, self.lst = _db16(clipmi, gpu, E, N), E, N, q.shape[0], K, lst
        self.M = N if lst is None else len(lst)
        self.ld = None if lst is None else torch.from_numpy(np.ascontiguousarray(lst, dtype=np.uint32).view(np.int32).copy()).to(gpu)
        self.qd = torch.from_numpy(np.array(q, dtype=np.float32, order="C")).to(gpu)
        self.ws_bytes = self.L.clipmi_topk_ip_workspace_bytes(self.M, E, self.Q, K)
        assert self.ws_bytes > 0
        self.outputs = [("scores", self.Q * K * 4), ("ids", self.Q * K * 8)]

    def __call__(self, ws, out_s, out_i):
        tail = (self.qd.data_ptr(), self.Q, self.K, 1000, out_s.data_ptr(), out_i.data_ptr(), ws.data_ptr(), ws.numel(),
                self.lib.stream_ptr(self.gpu))
        if self.lst is None:
            rc = self.L.clipmi_topk_ip(self.db.data_ptr(), self.lib.F16, self.N, self.E, *tail)
        else:
            rc = self.L.clipmi_topk_ip_rows(self.db.data_ptr(), self.lib.F16, self.N, self.E, self.ld.data_ptr(), self.M, *tail)
        self.lib.check(rc, "clipmi_topk_ip(_rows)")


@pytest.mark.parametrize("E", kr.WIDTHS)
@pytest.mark.parametrize("form", ["plain", "list"])
def test_workspace_independence(clipmi, gpu, topk_oracle, E, form):
    """A guarded workspace of exactly the stated size under the harness's four fills (zeros and 0xFF among them): byte-identical
    outputs, equal to the oracle, intact guard bands. Both run the pre-pass; Q = 17 is two column groups."""
    lst = None if form == "plain" else np.sort(np.random.default_rng(65576).choice(NMAX, 65576, replace=False))
    N = 70001 if form == "plain" else NMAX
    s = F16Search(clipmi, gpu, E, N, _rows(E)[2][:17], 100, lst)
    assert kr.make_plan(s.M, E, 17, 100)["sample"]
    got = W.run_independent(s, s.outputs, s.ws_bytes, device=gpu)
    Ds, Is = _want(topk_oracle, E, N, 17, 100, id_base=1000, rows=lst)
    _assert_exact(got["scores"].view(np.float32).reshape(17, 100), got["ids"].view(np.int64).reshape(17, 100), Ds, Is, f"{form} E={E}")


# ---- 7. the f32 paths did not move -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", kr.WIDTHS)
def test_f32_searches_beside_the_fp16_ones(clipmi, gpu, topk_oracle, E):
    """The recompiled f32 instantiations, plain and list, on this file's database against the oracle on db itself."""
    db, _, q = _rows(E)
    dbd = torch.from_numpy(db[:70001].copy()).to(gpu)
    D, I = _abi(clipmi, gpu, dbd, clipmi._lib.F32, 70001, E, q[:33], 51)
    _assert_exact(D, I, *_want(topk_oracle, E, 70001, 33, 51, key=("f32", 70001), src=0), f"f32 plain E={E}")
    lst = np.arange(4099, 70001, 3)
    Dl, Il = _abi(clipmi, gpu, dbd, clipmi._lib.F32, 70001, E, q[:33], 51, lst=lst)
    _assert_exact(Dl, Il, *_want(topk_oracle, E, 70001, 33, 51, rows=lst, src=0), f"f32 list E={E}")
