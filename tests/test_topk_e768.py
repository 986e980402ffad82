"""768-wide indexes (ViT-L/14) on the coarse search paths: what can be checked without a GPU - the library's argument
validation and workspace sizing, the index's one predicate for "this search goes through a coarse copy", and a numpy
restatement of the int8 superset bound with the constants the library uses at E = 768."""
import numpy as np
import pytest

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
    in f32 where the kernels use f32; exact scores in f64 (so this checks the bound's shape and constants, not its last ulp).
    Returns (superset held in every segment, mean and largest count of fresh survivors per query)."""
    f32 = np.float32
    rng = np.random.default_rng(seed)
    db = unit_rows(rng, N, E)
    q = unit_rows(rng, Q, E)
    perm = np.argsort(np.abs(db).max(axis=1), kind="stable")          # rows ordered by their largest |component|
    N32 = (N + 31) // 32 * 32
    xp = np.zeros((N32, E), f32)
    xp[:N] = db[perm]
    s = np.abs(xp).reshape(N32 // 32, -1).max(axis=1) / f32(127.0)    # one scale per 32-row block
    s[s == 0] = 1.0
    srow = np.repeat(s.astype(f32), 32)
    q8 = np.clip(np.rint(xp * (f32(1.0) / srow)[:, None]), -127, 127).astype(f32)
    a = (np.linalg.norm(xp - srow[:, None] * q8, axis=1).astype(f32) * f32(1.001)).astype(f32)      # error norms x 1.001
    a[N:] = 0
    rmax = f32(np.linalg.norm(db.astype(np.float64), axis=1).max() * (1 + 1e-6))
    amax = f32(a.max() * (1 + 1e-6))
    t = (np.abs(q).max(axis=1) / f32(127.0)).astype(f32)               # the query digit
    inv = (f32(1.0) / t).astype(f32)
    p = np.clip(np.rint(q * inv[:, None]), -127, 127).astype(f32)
    f = q - t[:, None] * p
    F = (np.linalg.norm(f, axis=1).astype(f32) * f32(1.001)).astype(f32)
    Y = np.linalg.norm(q, axis=1).astype(f32)
    slack = f32(1e-4) * f32(E / 512.0)                                 # i8_round_slack<E>: 1e-4 at 512, 1.5e-4 at 768
    margin = (f32(1.001) * (rmax + amax) * F + slack * rmax * Y).astype(f32)
    yt = (f32(1.001) * Y * inv).astype(f32)
    D = q8 @ p.T                                                       # exact: |D| <= E * 127^2 < 2^24
    assert np.abs(D).max() < 2 ** 24 and np.array_equal(D, np.rint(D))
    lhs = (D * srow[:, None] + (a[:, None] * yt[None, :])).astype(f32)
    exact = db.astype(np.float64) @ q.astype(np.float64).T              # [row][query]
    slot_row = np.full(N32, -1)
    slot_row[:N] = perm

    def kth(rows):
        return np.sort(exact[rows], axis=0)[-K]

    S1 = 12288
    S2 = max(min((N * K // 2048 + 31) & ~31, (N // 8) & ~31), 32768, S1)
    N1 = max((N // 4) & ~31, 4 * S2)
    segs = [(0, S2), (S2, N1), (N1, N32)] if N1 + 65536 <= N else [(0, S2), (S2, N32)]
    final = np.sort(exact, axis=0)[-K]
    tau = kth(np.arange(S1))                                           # level 1: the first S1 ROWS, exactly scored
    tot = np.zeros(Q)
    seen = np.zeros(N, bool)
    ok = True
    for r0, r1 in segs:
        sl = np.arange(r0, r1)
        sl = sl[slot_row[sl] >= 0]
        thr = ((tau.astype(f32) - margin) * inv).astype(f32)           # select_topk_kernel: (tau - margin) / t_q
        passed = lhs[sl] >= thr[None, :]
        tot += passed.sum(axis=0)
        need = exact[slot_row[sl]] >= final[None, :]                   # rows of the true top-K in this segment
        ok &= bool((passed | ~need).all())
        seen[slot_row[sl]] = True
        tau = np.sort(exact[seen], axis=0)[-K]                         # exact K-th best of the rows seen so far
    return ok, len(segs), tot.mean(), tot.max()


def test_int8_superset_bound_restated_in_numpy_at_768():
    N, Q, K = 200_000, 64, 51
    ok, nseg, mean, worst = _int8_bound_survivors(768, N, Q, K, 4242)
    print(f"E=768: fresh survivors per query mean {mean:.0f}, largest {worst:.0f} (N={N}, K={K})")
    assert nseg == 3
    assert ok, "a row of the true top-K fails the int8 coarse test"
    assert worst < N / 16
