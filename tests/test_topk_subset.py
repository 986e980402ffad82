"""The subset search without a GPU: the two new library entries and the hook (declared, exported, bound; argument validation is
host code and launches nothing), IndexFlatIP.subset's construction-time checks, shard_rows, and VectorStore.prefix_rows /
repl.within_rows on a packed store whose keys are chosen so that BYTE order matters. tests/test_topk_subset_gpu.py runs the
searches."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import test_topk_krange as kr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("clipmi_topk_ip_rows_workspace_bytes", "clipmi_topk_ip_rows", "clipmi_dbg_topk_rows_scan_ms")


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


def test_argument_validation_launches_nothing(clipmi):
    """Every refusal below is decided on the host before anything touches a device: this machine has none."""
    L, lib = clipmi._lib.lib(), clipmi._lib
    ws = L.clipmi_topk_ip_rows_workspace_bytes
    assert ws(70001, 512, 33, 51) > 0
    assert ws(70001, 500, 33, 51) == 0
    for E in kr.WIDTHS:
        assert ws(70001, E, 1, kr.KMAX[E]) > 0 and ws(70001, E, 1, kr.KMAX[E] + 1) == 0
    fake = C.c_void_p(256)
    call = lambda db_dtype, N, rows, M: L.clipmi_topk_ip_rows(fake, db_dtype, N, 512, rows, M, fake, 1, 10, 0, fake, fake, fake,
                                                              1 << 30, None)
    assert call(lib.F32, 100, None, 3) == 1 and "NULL row list" in lib.last_error()
    assert call(lib.F32, 100, fake, 101) == 1 and "M=101" in lib.last_error()
    assert call(lib.F32, 100, fake, -1) == 1
    assert call(lib.BF16, 100, fake, 3) == 4
    # K out of range, as clipmi_topk_ip refuses it
    assert L.clipmi_topk_ip_rows(fake, lib.F32, 100, 512, fake, 3, fake, 1, kr.KMAX[512] + 1, 0, fake, fake, fake, 1 << 30, None) == 1
    ms = C.c_float(0)
    assert L.clipmi_dbg_topk_rows_scan_ms(fake, 100, 512, fake, 3, fake, 33, 10, fake, fake, fake, 1 << 30, None, 1, C.byref(ms)) == 1


@pytest.mark.parametrize("E", kr.WIDTHS)
def test_workspace_is_the_exact_scans_for_m_rows(clipmi, E):
    """The list form needs no more workspace than clipmi_topk_ip over M rows: the same plan (make_plan(M, ...)), the same lists
    and counters. Checked against the Python restatement on test_topk_krange.py's probes, and against the exact entry itself."""
    L = clipmi._lib.lib()
    for M, Q in ((70001, 1), (70001, 17), (70001, 65), (20000, 33), (1000, 1024), (10_000_000, 32), (9, 3), (0, 3)):
        for K in kr._probes(kr.KMAX[E]):
            p = kr.make_plan(M, E, Q, K)
            got = L.clipmi_topk_ip_rows_workspace_bytes(M, E, Q, K)
            assert got == (kr.exact_workspace_bytes(p) if p else 0), (M, E, Q, K)
            assert got == L.clipmi_topk_ip_workspace_bytes(M, E, Q, K)


# ---- IndexFlatIP.subset on a CPU-device index -----------------------------------------------------------------------------------
def _cpu_index(clipmi, n=100):
    idx = clipmi.IndexFlatIP(512, device="cpu")
    idx.add(np.zeros((n, 512), np.float32))
    return idx


def test_subset_builds_a_sorted_unique_list(clipmi):
    idx = _cpu_index(clipmi)
    idx.id_base = 40
    sub = idx.subset([7, 3, 99, 3, 0, 7])
    assert isinstance(sub, clipmi.IndexSubset)
    assert sub.rows().tolist() == [0, 3, 7, 99] and sub.rows().dtype == torch.int64
    assert sub._list.dtype == torch.int32 and sub._list.tolist() == [0, 3, 7, 99] and sub._list.is_contiguous()
    assert (sub.ntotal, sub.d, sub.device, sub.id_base, sub.nprobe) == (4, 512, torch.device("cpu"), 40, 1)
    sub.nprobe = 32                                          # accepted, ignored
    sub.id_base = 5                                          # its own: the parent keeps its value
    assert idx.id_base == 40
    mask = np.zeros(100, bool)
    mask[[0, 3, 7, 99]] = True
    for m in (mask, torch.from_numpy(mask)):
        assert idx.subset(m).rows().tolist() == [0, 3, 7, 99]
    for rows in (np.array([99, 0], np.int32), torch.tensor([99, 0], dtype=torch.int16), np.array([99, 0], np.uint8)):
        assert idx.subset(rows).rows().tolist() == [0, 99]
    assert idx.subset([]).ntotal == 0 and idx.subset(np.zeros(100, bool)).ntotal == 0


def test_subset_refuses_bad_rows(clipmi):
    idx = _cpu_index(clipmi)
    with pytest.raises(ValueError, match="row numbers"):
        idx.subset([3, -1])
    with pytest.raises(ValueError, match="row numbers"):
        idx.subset([3, 100])
    with pytest.raises(ValueError, match="mask"):
        idx.subset(np.ones(99, bool))
    with pytest.raises(ValueError, match="integers"):
        idx.subset(np.array([1.0, 2.0]))
    with pytest.raises(ValueError, match="integers"):
        idx.subset(torch.tensor([1.0]))


def test_subset_search_has_no_cpu_fallback_and_notices_growth(clipmi):
    idx = _cpu_index(clipmi)
    sub = idx.subset([1, 2])
    with pytest.raises(clipmi.ClipmiError, match="no CPU fallback"):
        sub.search(np.zeros((1, 512), np.float32), 5)
    with pytest.raises(ValueError):
        sub.search(np.zeros((1, 100), np.float32), 5)
    idx.add(np.zeros((1, 512), np.float32))                  # the parent has grown: refused before anything else is looked at
    with pytest.raises(clipmi.ClipmiError, match="grown"):
        sub.search(np.zeros((1, 512), np.float32), 5)


def test_shard_rows(clipmi):
    f = clipmi.shard_rows
    rows = [0, 9, 10, 11, 19, 20, 21, 35]
    assert f(rows, 10, 20).tolist() == [0, 1, 9] and f(rows, 10, 20).dtype == np.int64           # both edges: 10 in, 20 out
    assert f(rows, 0, 10).tolist() == [0, 9]
    assert f(rows, 20, 36).tolist() == [0, 1, 15]
    assert f(rows, 12, 19).tolist() == []                                                          # rows on both sides only
    assert f(rows, 15, 15).tolist() == [] and f([], 0, 10).tolist() == []                         # an empty shard, no rows
    assert f([21, 11, 11, 35], 10, 36).tolist() == [1, 11, 25]                                    # unsorted, duplicated
    for world in (1, 3, 4):                                                                        # the shards partition the list
        parts = [f(rows, *clipmi.shard_bounds(36, world, r)) + clipmi.shard_bounds(36, world, r)[0] for r in range(world)]
        assert np.concatenate(parts).tolist() == rows


# ---- prefix_rows / within_rows ----------------------------------------------------------------------------------------------------
KEYS = [b"a-b/x", b"a/", b"a/x", b"a/y/z", b"a0", b"b/1", b"b/2", "b/é".encode(), b"b/\xff\xfe", "cé/1".encode(), b"c\xc3\xaa"]


def _store(clipmi, tmp_path, keys):
    db = clipmi.store.VectorStore(str(tmp_path / "v"), dim=4, backend="packed")
    db.b.put_many("fn_db", [(k, np.zeros(4, "<f4").tobytes()) for k in keys])
    _, paths = db.assemble()
    assert paths == sorted(keys)                          # bytewise
    return db, paths


def _brute(paths, p):
    hit = [i for i, k in enumerate(paths) if k.startswith(p)]
    return (hit[0], hit[-1] + 1) if hit else None


def test_prefix_rows_in_byte_order(clipmi, tmp_path):
    """'-' (0x2d) < '/' (0x2f) < '0' (0x30): "a-b/x" sorts BEFORE "a/" and "a0" behind every "a/..." - the run of "a/" is
    rows 1..3, and "a" is rows 0..4. Non-ASCII bytes sort behind every ASCII one."""
    db, paths = _store(clipmi, tmp_path, KEYS)
    n = len(paths)
    assert paths[:5] == [b"a-b/x", b"a/", b"a/x", b"a/y/z", b"a0"]
    assert db.prefix_rows(b"a/") == (1, 4) and db.prefix_rows("a/") == (1, 4) and db.prefix_rows(b"a") == (0, 5)
    assert db.prefix_rows(b"") == (0, n)
    prefixes = {k[:j] for k in KEYS for j in range(1, len(k) + 1)}
    for p in sorted(prefixes):
        assert db.prefix_rows(p) == _brute(paths, p), p
    for p in (b"A", b"\x00", b"a.", b"a/w", b"a/z", b"b/3", b"b0", b"c\xc3\xab", b"d", b"\xff", b"a/x/", b"b/\xff\xff"):
        lo, hi = db.prefix_rows(p)                        # before the first key, between keys, behind the last: empty
        assert _brute(paths, p) is None and lo == hi and 0 <= lo <= n, p
    db.close()


def test_within_rows_union_and_complement(clipmi, tmp_path):
    db, paths = _store(clipmi, tmp_path, KEYS)
    n = len(paths)
    w = clipmi.repl.within_rows
    a, b = list(range(1, 4)), [i for i, k in enumerate(paths) if k.startswith(b"b/")]
    assert w(db, "a/").tolist() == a and w(db, "a/").dtype == np.int64
    assert w(db, os.pathsep.join(["b/", "a/"])).tolist() == sorted(a + b)
    assert w(db, os.pathsep.join(["a/", "a/x", "a"])).tolist() == list(range(5))                   # overlapping prefixes: a union
    assert w(db, "!" + os.pathsep.join(["a/", "b/"])).tolist() == [i for i in range(n) if i not in a + b]
    assert w(db, "nothing/").tolist() == [] and w(db, "!nothing/").tolist() == list(range(n))
    assert w(db, "cé").tolist() == [paths.index("cé/1".encode())]
    db.close()


def test_prefix_rows_takes_logarithmically_many_gets(clipmi, tmp_path):
    n = 1000
    keys = [b"dir%02d/%04d.jpg" % (i % 7, i) for i in range(n)]
    db, paths = _store(clipmi, tmp_path, keys)
    calls = []
    inner = db.idx_get
    db.idx_get = lambda i: (calls.append(i), inner(i))[1]
    bound = 2 * math.ceil(math.log2(n)) + 4
    for p in (b"dir03/", b"dir00/", b"dir06/", b"dir", b"dir03/0003.jpg", b"zzz", b"", b"a", b"dir031"):
        calls.clear()
        lo, hi = db.prefix_rows(p)
        assert len(calls) <= bound, (p, len(calls), bound)
        assert all(k.startswith(p) for k in paths[lo:hi]) and hi - lo == sum(k.startswith(p) for k in paths)
    db.close()
