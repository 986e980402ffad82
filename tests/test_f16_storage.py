"""fp16 storage (IndexFlatIP(storage="f16"), CLIPMI_F16) without a GPU: the two new library entries (declared,
exported, bound; argument validation is host code and launches nothing), the constructor and the routing on a CPU-device index,
the conversion's edge values through the CPU `add` path against numpy bit for bit, the version-2 file format against bytes
built by hand, and the premise of the GPU tests: the oracle on the fp16-rounded rows answers with other score bits than on the
f32 rows, so a search that "passes" by reading f32 rows cannot. tests/test_f16_storage_gpu.py runs the kernels."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest
import torch

import test_topk_krange as kr
from conftest import unit_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("clipmi_rows_to_f16", "clipmi_dbg_topk_scan_f16_ms")

F = np.float32
# (value, what it is): every one converts to a finite or already-infinite half; 65 520 (the first value that overflows) is apart
EDGES = [
    (F(0.0), "+0"), (F(-0.0), "-0"),
    (F(2.0 ** -24), "the smallest subnormal"), (F(-2.0 ** -24), "its negative"),
    (F(2.0 ** -25), "tie between 0 and 2^-24: to even, 0"), (F(-2.0 ** -25), "... keeping the sign: -0"),
    (F(2.0 ** -25) * (F(1) + F(2.0 ** -23)), "one ulp above that tie: 2^-24"),
    (F(2.0 ** -14) - F(2.0 ** -25), "tie at the subnormal / normal seam: up to 2^-14"),
    (F(1) + F(2.0 ** -11), "tie: down to 1 (even)"), (F(1) + F(3 * 2.0 ** -11), "tie: up to 1 + 2^-9 (even)"),
    (F(65504.0), "the largest finite half"), (np.nextafter(F(65520.0), F(0)), "65 519.996: the largest f32 that stays finite"),
    (F(np.nan), "NaN"), (F(np.inf), "+inf"), (F(-np.inf), "-inf"),
    (F(1.0), "exact"), (F(0.1), "inexact"), (F(-1e-8), "underflow to -0"),
]
OVERFLOW = F(65520.0)


def edge_rows(E, with_overflow=False):
    """[2][E] f32: the edge values tiled over a row and, reversed, over a second one (every value at several lane positions)."""
    vals = np.array([v for v, _ in EDGES] + ([OVERFLOW, -OVERFLOW] if with_overflow else []), dtype=np.float32)
    row = np.resize(vals, E)
    return np.stack([row, row[::-1]]).astype(np.float32)


def counts(x):
    """numpy's (changed, overflowed) of a conversion: the contract of clipmi_rows_to_f16's two counters."""
    with np.errstate(over="ignore"):
        back = x.astype(np.float16).astype(np.float32)
    return int(((back != x) & ~np.isnan(x)).sum()), int((np.isfinite(x) & np.isinf(back)).sum())


def test_numpy_rounds_the_edges_as_the_contract_says():
    """The reference of the conversion tests is numpy.astype(float16); this pins that it IS round-to-nearest-even with the
    contract's overflow rule, from the half bit patterns written out by hand."""
    want = [0x0000, 0x8000, 0x0001, 0x8001, 0x0000, 0x8000, 0x0001, 0x0400, 0x3C00, 0x3C02, 0x7BFF, 0x7BFF, None, 0x7C00, 0xFC00,
            0x3C00, 0x2E66, 0x8000]
    with np.errstate(over="ignore"):
        got = np.array([v for v, _ in EDGES], np.float32).astype(np.float16).view(np.uint16)
        assert np.array([OVERFLOW, -OVERFLOW]).astype(np.float16).view(np.uint16).tolist() == [0x7C00, 0xFC00]
    for (v, what), w, g in zip(EDGES, want, got):
        assert (np.isnan(np.uint16(g).view(np.float16)) if w is None else g == w), (what, hex(g))
    # the counters' contract on a row written out by hand: changed = 65 520, -65 520, 70 000, 0.1; overflowed = the first three
    assert counts(np.array([[65520, -65520, 70000, 65504, np.inf, np.nan, 0.1, -0.0]], np.float32)) == (4, 3)


# ---- the library entries ----------------------------------------------------------------------------------------------------------
def test_entries_are_declared_exported_and_bound(clipmi):
    header = open(os.path.join(ROOT, "include", "clipmi.h")).read()
    L = clipmi._lib.lib()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in clipmi._lib.SYMBOLS
        assert getattr(L, name).argtypes is not None
    assert L.clipmi_abi_version() == 8 and clipmi._lib.ABI_VERSION == 8
    assert re.search(r"#define CLIPMI_ABI_VERSION 8\b", header)
    assert clipmi._lib.F16 == 3 and re.search(r"\bCLIPMI_F16 = 3\b", header)
    assert (clipmi._lib.F32, clipmi._lib.BF16, clipmi._lib.U8) == (0, 1, 2)


def test_argument_validation_launches_nothing(clipmi):
    """Every refusal below is decided on the host before anything touches a device: this machine has none. With CLIPMI_F16
    the two searches refuse what they refuse with CLIPMI_F32; bf16 and u8 rows stay unsupported."""
    L, lib = clipmi._lib.lib(), clipmi._lib
    fake = C.c_void_p(256)
    rows = lambda db_dtype, N, lst, M, K=10: L.clipmi_topk_ip_rows(fake, db_dtype, N, 512, lst, M, fake, 1, K, 0, fake, fake, fake,
                                                                   1 << 30, None)
    plain = lambda db_dtype, K=10, q=fake, E=512: L.clipmi_topk_ip(fake, db_dtype, 100, E, q, 1, K, 0, fake, fake, fake, 1 << 30, None)
    for dt in (lib.F32, lib.F16):
        assert rows(dt, 100, None, 3) == 1 and "NULL row list" in lib.last_error()
        assert rows(dt, 100, fake, 101) == 1 and "M=101" in lib.last_error()
        assert rows(dt, 100, fake, -1) == 1
        assert rows(dt, 100, fake, 3, K=kr.KMAX[512] + 1) == 1
        assert plain(dt, K=kr.KMAX[512] + 1) == 1
        assert plain(dt, q=None) == 1 and "NULL" in lib.last_error()
        assert plain(dt, E=500) == 1
    for dt in (lib.BF16, lib.U8, 4, -1):
        assert rows(dt, 100, fake, 3) == 4 and "db_dtype" in lib.last_error()
        assert plain(dt) == 4 and "db_dtype" in lib.last_error()
    conv = lambda db, N, E, out: L.clipmi_rows_to_f16(db, N, E, out, None, None)
    assert conv(fake, 10, 510, fake) == 1 and "multiple of 4" in lib.last_error()
    assert conv(fake, 0, 512, fake) == 1 and conv(None, 10, 512, fake) == 1 and conv(fake, 10, 512, None) == 1
    ms = C.c_float(0)
    hook = lambda lst, M, Q: L.clipmi_dbg_topk_scan_f16_ms(fake, 100, 512, lst, M, fake, Q, 10, fake, fake, fake, 1 << 30, None, 1,
                                                           C.byref(ms))
    assert hook(None, 0, 33) == 1 and hook(fake, 3, 33) == 1 and hook(fake, 0, 1) == 1


# ---- constructor and routing on a CPU-device index --------------------------------------------------------------------------------
def test_constructor_refuses_what_it_cannot_store(clipmi):
    for bad in ("f64", "bf16", None, "", 16):
        with pytest.raises(ValueError, match="storage"):
            clipmi.IndexFlatIP(512, device="cpu", storage=bad)
    for coarse in ("bf16", "int8"):
        with pytest.raises(ValueError, match="coarse"):
            clipmi.IndexFlatIP(512, device="cpu", coarse=coarse, storage="f16")
    idx = clipmi.IndexFlatIP(512, "cpu", None, None, "f16")                 # the new keyword is the last positional
    assert idx.storage == "f16" and (idx.f16_changed, idx.f16_overflowed) == (0, 0)
    assert clipmi.IndexFlatIP(512, "cpu").storage == "f32"


def test_an_f32_index_is_what_it_was(clipmi):
    idx = clipmi.IndexFlatIP(512, device="cpu")
    x = np.full((3, 512), 0.1, np.float32)
    idx.add(x)
    assert idx.matrix().dtype == torch.float32 and idx.matrix() is idx.matrix() and (idx.matrix().numpy() == x).all()
    assert (idx.f16_changed, idx.f16_overflowed) == (0, 0)
    with pytest.raises(ValueError, match="f32"):
        idx.matrix_f16()


def test_uses_coarse_stays_false_on_an_fp16_index(clipmi):
    """repl.main and open_sharded assign .coarse after construction; an fp16 index must stay on its exact scan."""
    idx = clipmi.IndexFlatIP(512, device="cpu", storage="f16")
    idx.add(np.zeros((70000, 512), np.float32))
    idx.coarse = "int8"
    assert idx.ntotal == 70000 and not idx.uses_coarse()
    ref = clipmi.IndexFlatIP(512, device="cpu")
    ref.add(np.zeros((70000, 512), np.float32))
    ref.coarse = "int8"
    assert ref.uses_coarse()
    for m in (idx.matrix_bf16, idx.matrix_i8):
        with pytest.raises(ValueError, match="coarse"):
            m()


def test_add_stores_halves_and_counts_changes(clipmi):
    rng = np.random.default_rng(3)
    a, b = unit_rows(rng, 7, 512), unit_rows(rng, 5, 512).astype(np.float16).astype(np.float32)
    idx = clipmi.IndexFlatIP(512, device="cpu", storage="f16")
    idx.add(a)
    assert idx.f16_changed == counts(a)[0] > 3000
    idx.add(torch.from_numpy(b))
    idx.add(np.empty((0, 512), np.float32))
    assert idx.f16_changed == counts(a)[0] and idx.f16_overflowed == 0 and idx.ntotal == 12       # b is representable
    m = idx.matrix_f16()
    assert m.dtype == torch.float16 and m.shape == (12, 512) and m is idx.matrix_f16()
    assert (m.numpy().view(np.uint16) == np.concatenate([a, b]).astype(np.float16).view(np.uint16)).all()
    up = idx.matrix()
    assert up.dtype == torch.float32 and up is not idx.matrix() and (up.numpy() == m.numpy().astype(np.float32)).all()
    with pytest.raises(ValueError):
        idx.add(np.zeros((2, 768), np.float32))


def test_a_row_beyond_the_fp16_range_is_refused_and_changes_nothing(clipmi):
    idx = clipmi.IndexFlatIP(512, device="cpu", storage="f16")
    idx.add(np.full((4, 512), 0.1, np.float32))
    before = (idx.ntotal, idx.f16_changed, idx.matrix_f16().clone())
    x = np.zeros((3, 512), np.float32)
    x[1, 5] = 70000.0
    x[2, 9] = -65520.0
    with pytest.raises(ValueError, match=r"2 element.*65504"):
        idx.add(x)
    assert (idx.ntotal, idx.f16_changed, idx.f16_overflowed) == (before[0], before[1], 0)
    assert torch.equal(idx.matrix_f16(), before[2])
    inf = np.zeros((1, 512), np.float32)
    inf[0, 3] = np.inf                                   # an infinite input did not BECOME infinite: stored as it is
    idx.add(inf)
    assert idx.ntotal == 5 and idx.f16_changed == before[1]


def test_no_cpu_search(clipmi):
    idx = clipmi.IndexFlatIP(512, device="cpu", storage="f16")
    idx.add(np.zeros((20, 512), np.float32))
    with pytest.raises(clipmi._lib.ClipmiError, match="no CPU fallback"):
        idx.search(np.zeros((1, 512), np.float32), 5)
    with pytest.raises(clipmi._lib.ClipmiError, match="no CPU fallback"):
        idx.subset([1, 2]).search(np.zeros((1, 512), np.float32), 5)


@pytest.mark.parametrize("E", kr.WIDTHS)
def test_edge_values_through_the_cpu_add_path(clipmi, E):
    """torch's conversion on the CPU path against numpy, bit for bit (NaN as NaN), with both counts; 65 520 is refused."""
    x = edge_rows(E)
    idx = clipmi.IndexFlatIP(E, device="cpu", storage="f16")
    idx.add(x)
    got, want = idx.matrix_f16().numpy().view(np.uint16), x.astype(np.float16).view(np.uint16)
    nan = np.isnan(x)
    assert (got[~nan] == want[~nan]).all() and np.isnan(got.view(np.float16)[nan]).all()
    assert idx.f16_changed == counts(x)[0] and counts(x)[1] == 0
    bad = edge_rows(E, with_overflow=True)
    with pytest.raises(ValueError, match=f"{counts(bad)[1]} element"):
        idx.add(bad)
    assert idx.ntotal == 2


# ---- files ------------------------------------------------------------------------------------------------------------------------
def _db(n=5, E=512, seed=11):
    return unit_rows(np.random.default_rng(seed), n, E)


def _v2_bytes(h):
    return b"CLIPMIIX" + struct.pack("<IIQ", 2, h.shape[1], h.shape[0]) + struct.pack("<II", 3, 0) + h.astype("<f2").tobytes()


def _v1_bytes(x):
    return b"CLIPMIIX" + struct.pack("<IIQ", 1, x.shape[1], x.shape[0]) + x.astype("<f4").tobytes()


def _index(clipmi, x, storage):
    idx = clipmi.IndexFlatIP(x.shape[1], device="cpu", storage=storage)
    idx.add(x)
    return idx


def test_write_index_bytes(clipmi, tmp_path):
    """An fp16 index writes version 2 (magic, <IIQ (2, d, n), <II (3, 0), halves); an f32 index the version-1 bytes it always
    wrote; the faiss format of an fp16 index is the faiss file of the f32 index of its up-converted rows."""
    x = _db()
    h = x.astype(np.float16)
    p = lambda n: str(tmp_path / n)
    clipmi.write_index(_index(clipmi, x, "f16"), p("h.index"))
    assert open(p("h.index"), "rb").read() == _v2_bytes(h) and os.path.getsize(p("h.index")) == 32 + 5 * 512 * 2
    clipmi.write_index(_index(clipmi, x, "f32"), p("f.index"))
    assert open(p("f.index"), "rb").read() == _v1_bytes(x)
    clipmi.write_index(_index(clipmi, x, "f16"), p("h.faiss"), format="faiss")
    clipmi.write_index(_index(clipmi, h.astype(np.float32), "f32"), p("f.faiss"), format="faiss")
    assert open(p("h.faiss"), "rb").read() == open(p("f.faiss"), "rb").read()
    assert open(p("h.faiss"), "rb").read()[:4] == b"IxFI"
    with pytest.raises(ValueError):
        clipmi.write_index(_index(clipmi, x, "f16"), p("x"), format="other")


@pytest.mark.parametrize("kind", ["v1", "v2", "faiss"])
@pytest.mark.parametrize("storage", [None, "f32", "f16"])
def test_read_index_round_trips(clipmi, tmp_path, kind, storage):
    x = _db()
    h = x.astype(np.float16)
    path = str(tmp_path / "images.index")
    if kind == "faiss":
        clipmi.write_index(_index(clipmi, x, "f32"), path, format="faiss")
    else:
        open(path, "wb").write(_v1_bytes(x) if kind == "v1" else _v2_bytes(h))
    idx = clipmi.read_index(path, device="cpu", storage=storage)
    want_storage = storage or ("f16" if kind == "v2" else "f32")
    assert idx.storage == want_storage and idx.ntotal == 5 and idx.d == 512 and idx.id_base == 0 and idx.n_file == 5
    if want_storage == "f16":
        m = idx.matrix_f16()
        assert m.dtype == torch.float16 and (m.numpy().view(np.uint16) == h.view(np.uint16)).all()
        assert idx.f16_changed == (0 if kind == "v2" else counts(x)[0])
    else:
        m = idx.matrix()
        assert m.dtype == torch.float32 and (m.numpy() == (h.astype(np.float32) if kind == "v2" else x)).all()
        assert idx.f16_changed == 0
    assert clipmi.index.index_rows(path) == (5, 512)
    with pytest.raises(ValueError, match="storage"):
        clipmi.read_index(path, device="cpu", storage="bf16")


def test_read_index_converts_in_bounded_add_calls(clipmi, tmp_path, monkeypatch):
    """storage="f16" on an f32 file goes through `add` in pieces of at most F16_ADD_ROWS rows (2^20 in the product)."""
    assert clipmi.index.F16_ADD_ROWS == 1 << 20
    monkeypatch.setattr(clipmi.index, "F16_ADD_ROWS", 2)
    x = _db()
    path = str(tmp_path / "images.index")
    open(path, "wb").write(_v1_bytes(x))
    idx = clipmi.read_index(path, device="cpu", storage="f16")
    assert [c.shape[0] for c in idx._chunks] == [2, 2, 1] and idx.f16_changed == counts(x)[0]
    assert (idx.matrix_f16().numpy().view(np.uint16) == x.astype(np.float16).view(np.uint16)).all()


@pytest.mark.parametrize("storage", [None, "f32"])
def test_rows_of_a_version_2_file(clipmi, tmp_path, storage):
    h = _db().astype(np.float16)
    path = str(tmp_path / "images.index")
    open(path, "wb").write(_v2_bytes(h))
    idx = clipmi.read_index(path, device="cpu", rows=(1, 4), storage=storage)
    assert (idx.ntotal, idx.id_base, idx.n_file) == (3, 1, 5)
    got = idx.matrix_f16().numpy() if storage is None else idx.matrix().numpy()
    assert (got == (h[1:4] if storage is None else h[1:4].astype(np.float32))).all()
    assert clipmi.read_index(path, device="cpu", rows=(5, 5)).ntotal == 0
    with pytest.raises(ValueError):
        clipmi.read_index(path, device="cpu", rows=(2, 6))


def test_malformed_version_2_files_raise(clipmi, tmp_path):
    h = _db().astype(np.float16)
    good = _v2_bytes(h)
    cases = {"truncated rows": good[:-2], "truncated header": good[:28],
             "version 3": good[:8] + struct.pack("<I", 3) + good[12:],
             "dtype code 1": good[:24] + struct.pack("<II", 1, 0) + good[32:],
             "dtype code 0": good[:24] + struct.pack("<II", 0, 0) + good[32:]}
    for name, data in cases.items():
        path = str(tmp_path / "bad.index")
        open(path, "wb").write(data)
        with pytest.raises(ValueError):
            clipmi.read_index(path, device="cpu")
        with pytest.raises(ValueError):
            clipmi.read_index(path, device="cpu", storage="f32")


def test_storage_from_env(clipmi):
    f = clipmi.index.storage_from_env
    assert f({}) is None and f({"CLIPMI_STORAGE": ""}) is None and f({"CLIPMI_STORAGE": "f32"}) is None
    assert f({"CLIPMI_STORAGE": "f16"}) == "f16"
    for bad in ("F16", "fp16", "bf16", "1"):
        with pytest.raises(ValueError, match="CLIPMI_STORAGE"):
            f({"CLIPMI_STORAGE": bad})


# ---- the premise of the GPU tests -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", kr.WIDTHS)
def test_the_oracle_tells_fp16_rows_from_f32_rows(topk_oracle, E):
    """70 001 seeded unit rows, Q = 33, K = 51: the oracle on h = f32(f16(db)) and on db disagree in the score bits of at least
    half of the slots (0.9988 of them at E = 512 and all at 768 on this seed). A GPU search that equals the oracle on h bit
    for bit has therefore read the fp16 rows. It is still the same search to fp16's precision: each element moves by a
    relative 2^-11 at most, so each score of a unit row against a unit query by 2^-11 at most (Cauchy-Schwarz), and so does
    each slot's score (order statistics are 1-Lipschitz in the largest perturbation)."""
    rng = np.random.default_rng(1)
    db, q = unit_rows(rng, 70001, E), unit_rows(rng, 33, E)
    h = db.astype(np.float16).astype(np.float32)
    Dh, Ih = topk_oracle.topk(h, q, 51)
    Df, If = topk_oracle.topk(db, q, 51)
    differ = float((Dh.view(np.uint32) != Df.view(np.uint32)).mean())
    print(f"E={E}: score bits differ in {differ:.4f} of the slots, ids differ in {float((Ih != If).mean()):.4f}")
    assert differ >= 0.5
    assert np.abs(Dh - Df).max() <= 2.0 ** -11 + 1e-6
