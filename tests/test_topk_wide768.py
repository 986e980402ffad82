"""The opt-in one-pass wide int8 search at E = 768 (clipmi_topk_ip_wide_i8, IndexFlatIP(wide_768=True)): what can be checked
without a GPU - the new workspace function, the ABI version, the constructor flag and a numpy restatement of the wide scan's
test (per-row test with the block's largest error norm, integer pre-test, the wide segment plan) with the constants the
library uses at E = 768."""
import numpy as np
import pytest

from coarse_tight import i8_survivors, wide_segments
from conftest import unit_rows

CHUNK = 1024          # csrc/topk.hip WIDE768_MAX_Q


def test_wide_workspace_at_512_is_the_coarse_workspace(clipmi):
    L = clipmi._lib.lib()
    for N, Q, K in ((100000, 64, 51), (100000, 200, 51), (10000000, 64, 51), (70001, 5, 300), (200003, 1024, 101)):
        want = L.clipmi_topk_ip_coarse_workspace_bytes(N, 512, Q, K)
        assert want > 0 and L.clipmi_topk_ip_wide_workspace_bytes(N, 512, Q, K) == want, (N, Q, K)


def test_wide_workspace_at_768(clipmi):
    L = clipmi._lib.lib()
    N, K = 100000, 51
    base = L.clipmi_topk_ip_coarse_workspace_bytes(N, 768, 64, K)
    assert base > 0
    sizes = {}
    for Q in (1, 64, 65, 200, 1024, 2200):
        sizes[Q] = L.clipmi_topk_ip_wide_workspace_bytes(N, 768, Q, K)
        assert sizes[Q] > 0, (Q, clipmi._lib.last_error())
        assert sizes[Q] >= base, Q
    assert sizes[1] == sizes[64] == base                   # up to 64 queries it IS the 64-query pass
    # monotone in Q up to the chunk, constant beyond it
    qs = [1, 63, 64, 65, 127, 128, 129, 200, 512, 1000, CHUNK]
    ws = [L.clipmi_topk_ip_wide_workspace_bytes(N, 768, Q, K) for Q in qs]
    assert all(a <= b for a, b in zip(ws, ws[1:])), list(zip(qs, ws))
    assert ws[-1] > ws[qs.index(200)] > base               # the lists of a wide chunk really grow with its queries
    for Q in (CHUNK + 1, 2 * CHUNK, 2200, 100000):
        assert L.clipmi_topk_ip_wide_workspace_bytes(N, 768, Q, K) == ws[-1], Q
    assert L.clipmi_topk_ip_wide_workspace_bytes(N, 640, 200, K) == 0
    assert "unsupported" in clipmi._lib.last_error()
    assert L.clipmi_topk_ip_wide_workspace_bytes(65535, 768, 200, K) == 0
    assert "unsupported" in clipmi._lib.last_error()
    # the parent's entry point keeps its size: more than 64 queries on the 64-query workspace
    assert L.clipmi_topk_ip_coarse_workspace_bytes(100000, 768, 200, 51) == L.clipmi_topk_ip_coarse_workspace_bytes(100000, 768, 64, 51)


def test_abi_version_is_8(clipmi):
    assert clipmi._lib.lib().clipmi_abi_version() == 8 == clipmi._lib.ABI_VERSION


def test_constructor_flag(clipmi, monkeypatch):
    monkeypatch.delenv("CLIPMI_WIDE_768", raising=False)
    mk = lambda **kw: clipmi.IndexFlatIP(kw.pop("d", 768), device="cpu", coarse=kw.pop("coarse", "int8"), **kw)
    assert mk().wide_768 is False and not mk()._wide_768_on()                     # default: off
    assert mk(wide_768=True).wide_768 is True and mk(wide_768=True)._wide_768_on()
    for off in ("", "0"):
        monkeypatch.setenv("CLIPMI_WIDE_768", off)
        assert mk().wide_768 is False
    monkeypatch.setenv("CLIPMI_WIDE_768", "1")
    assert mk().wide_768 is True and mk()._wide_768_on()
    assert mk(wide_768=False).wide_768 is False and not mk(wide_768=False)._wide_768_on()     # explicit beats the environment
    # inert anywhere but d = 768 with the int8 copy
    assert not mk(d=512)._wide_768_on() and not mk(d=512, wide_768=True)._wide_768_on()
    assert not mk(coarse="bf16", wide_768=True)._wide_768_on() and not mk(coarse=None, wide_768=True)._wide_768_on()
    assert clipmi.IndexFlatIP.WIDE_Q_768 == CHUNK


def test_read_index_passes_the_flag(clipmi, tmp_path, monkeypatch):
    monkeypatch.delenv("CLIPMI_WIDE_768", raising=False)
    idx = clipmi.IndexFlatIP(768, device="cpu")
    idx.add(np.zeros((3, 768), np.float32))
    path = str(tmp_path / "w.index")
    clipmi.write_index(idx, path)
    assert clipmi.read_index(path, device="cpu", coarse="int8", wide_768=True)._wide_768_on()
    assert not clipmi.read_index(path, device="cpu", coarse="int8")._wide_768_on()


def test_wide_segment_plan():
    assert wide_segments(70001) == [70001]
    assert wide_segments(65536) == [65536]
    assert wide_segments(131101) == [65536, 131101]
    assert wide_segments(200000) == [65536, 200000]
    assert wide_segments(524301) == [65536, 262144, 524301]


def _wide_bound_survivors(E, N, Q, K, seed):
    """The wide scan's test as csrc/topk.hip computes it (quantize_rows_i8_kernel, coarse_prep_kernel's wide form,
    scan_coarse_wide_kernel), in f32 where the kernels use f32 - tests/coarse_tight.py::i8_survivors in its wide form: each
    row's error norm replaced by its block's largest, the wide segment plan, the sample of the first 12 288 rows -; exact
    scores in f64.
    Returns (superset held in every segment, the integer pre-test rejected no lane with a passing row, segments, mean and
    largest count of fresh survivors per query)."""
    rng = np.random.default_rng(seed)
    db = unit_rows(rng, N, E)
    q = unit_rows(rng, Q, E)
    exact = db.astype(np.float64) @ q.astype(np.float64).T
    ok, pre_ok, nseg, tot = i8_survivors(db, q, K, exact, wide=True)
    return ok, pre_ok, nseg, tot.mean(), tot.max()


def test_wide_int8_bound_restated_in_numpy_at_768():
    """200 000 unit rows, Q = 128, K = 51, seed 4242: every row of the true top-K passes in both segments, the integer
    pre-test rejects no lane that holds a passing row, and the largest count of fresh survivors per query stays under
    N / 16 (a condition; the figures are printed: about 1.3 k mean, 1.7 k largest)."""
    N, Q, K = 200_000, 128, 51
    ok, pre_ok, nseg, mean, worst = _wide_bound_survivors(768, N, Q, K, 4242)
    print(f"E=768 wide: fresh survivors per query mean {mean:.0f}, largest {worst:.0f} (N={N}, Q={Q}, K={K}, {nseg} segments)")
    assert nseg == 2
    assert ok, "a row of the true top-K fails the wide int8 test"
    assert pre_ok, "the integer pre-test rejects a passing row"
    assert worst < N / 16
