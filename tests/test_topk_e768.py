"""768-wide indexes (ViT-L/14) on the coarse search paths: what can be checked without a GPU - the library's argument
validation and workspace sizing, the index's one predicate for "this search goes through a coarse copy", and a numpy
restatement of the int8 superset bound with the constants the library uses at E = 768."""
import numpy as np
import pytest

from coarse_tight import i8_survivors
from conftest import unit_rows


def test_coarse_workspace_accepts_768_and_keeps_512(clipmi):
    L = clipmi._lib.lib()
    for Q in (1, 64, 200):
        assert L.clipmi_topk_ip_coarse_workspace_bytes(100000, 768, Q, 51) > 0, (Q, clipmi._lib.last_error())
    # no wide pass at 768: more than 64 queries run as 64-query passes on the 64-query workspace
    assert (L.clipmi_topk_ip_coarse_workspace_bytes(100000, 768, 200, 51)
            == L.clipmi_topk_ip_coarse_workspace_bytes(100000, 768, 64, 51))
    assert L.clipmi_topk_ip_coarse_workspace_bytes(100000, 640, 1, 51) == 0
    assert "unsupported" in clipmi._lib.last_error()
    assert L.clipmi_topk_ip_coarse_workspace_bytes(65535, 768, 1, 51) == 0
    assert "unsupported" in clipmi._lib.last_error()
    assert L.clipmi_topk_ip_coarse_workspace_bytes(65535, 512, 1, 51) == 0
    assert "unsupported" in clipmi._lib.last_error()
    # E = 512: byte for byte what the library returned before 768 was accepted - less, in the 64-query workspaces, the 9 216 bytes
    # of the live-threshold scan's ladder (64 x 32 words of the control block), keys and edges (512 bytes each), which left with
    # that scan; the wide workspaces (Q = 200, 1024) never held them. (70 001 rows at K = 300: the exact
    # fallback's 64 lists are capped at one entry per row, 70 016 slots instead of 1024 waves x 320 - make_plan's row bound,
    # tests/test_topk_krange.py - which takes 64 x 257 664 x 8 bytes off this one)
    for (N, Q, K), want in (((100000, 64, 51), 176238336 - 9216), ((100000, 200, 51), 235020800),
                            ((10000000, 64, 51), 218181376 - 9216), ((70001, 5, 300), 302067456 - 9216 - 64 * 257664 * 8),
                            ((200003, 1024, 101), 1342734848)):
        assert L.clipmi_topk_ip_coarse_workspace_bytes(N, 512, Q, K) == want, (N, Q, K)
    # the 768 workspace is the 512 one + the larger query image (bf16: four 16-query groups x 24 k-steps x 1 KiB instead of x 16)
    assert L.clipmi_topk_ip_coarse_workspace_bytes(100000, 768, 64, 51) - (176238336 - 9216) == 4 * (24 - 16) * 1024


@pytest.mark.parametrize("kind", ["int8", "bf16"])
def test_uses_coarse_is_one_predicate_for_512_and_768(clipmi, kind):
    idx = clipmi.IndexFlatIP(768, device="cpu", coarse=kind)
    idx.add(np.zeros((65535, 768), np.float32))
    assert not idx.uses_coarse()
    idx.add(np.zeros((1, 768), np.float32))
    assert idx.ntotal == 65536 and idx.uses_coarse()
    idx.coarse = None
    assert not idx.uses_coarse()
    from clipmi.index import coarse_eligible
    assert coarse_eligible(kind, 768, 65536) and coarse_eligible(kind, 512, 65536)
    assert not coarse_eligible(kind, 768, 65535) and not coarse_eligible(None, 768, 10 ** 6) and not coarse_eligible("none", 768, 10 ** 6)
    assert not coarse_eligible(kind, 640, 10 ** 6)


def test_repl_gates_use_the_same_predicate(clipmi):
    """open_sharded and main decide with index.coarse_eligible, not with a width of their own."""
    import inspect
    from clipmi import repl
    src = inspect.getsource(repl)
    assert src.count("coarse_eligible(") == 2 and "d == 512" not in src


def _int8_bound_survivors(E, N, Q, K, seed):
    """The int8 coarse test as csrc/topk.hip computes it (quantize_rows_i8_kernel, coarse_prep_kernel, scan_coarse_kernel),
    in f32 where the kernels use f32 - tests/coarse_tight.py::i8_survivors, the one restatement of the suite -; exact scores in
    f64 (so this checks the bound's shape and constants, not its last ulp).
    Returns (superset held in every segment, segments, mean and largest count of fresh survivors per query)."""
    rng = np.random.default_rng(seed)
    db = unit_rows(rng, N, E)
    q = unit_rows(rng, Q, E)
    exact = db.astype(np.float64) @ q.astype(np.float64).T              # [row][query]
    ok, _, nseg, tot = i8_survivors(db, q, K, exact, wide=False)
    return ok, nseg, tot.mean(), tot.max()


def test_int8_superset_bound_restated_in_numpy_at_768():
    N, Q, K = 200_000, 64, 51
    ok, nseg, mean, worst = _int8_bound_survivors(768, N, Q, K, 4242)
    print(f"E=768: fresh survivors per query mean {mean:.0f}, largest {worst:.0f} (N={N}, K={K})")
    assert nseg == 3
    assert ok, "a row of the true top-K fails the int8 coarse test"
    assert worst < N / 16
