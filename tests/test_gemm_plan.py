"""csrc/gemm_plan.hpp from the CPU: which kernel every GEMM of the encode path runs on, through the host-only hooks
clipmi_dbg_gemm_plan / clipmi_dbg_gemm_fp8_plan (no device, no operand).

(a) tests/golden/gemm_plan_parent.json pins the answers of the commit BEFORE the plan existed. It was recorded from a stubbed
    host build of that commit's dispatcher: its csrc/gemm.hip compiled into a stand-alone program whose launch macros write
    down (kernel, grid, block, LDS, arguments) instead of launching, fed every GEMM of ViT-B/32 at B = 1 ... 1024, the text tower at Q = 1, 2, 64 (77 tokens and trimmed
    lengths), ViT-L/14 at B = 1, 64, 256, the FP8 tower below and above one round of tiles, the patch GEMM and the head. Nothing
    in it comes from the code under test. Row: [[kind, M, N, K, epi, algo | mx, leaf flags | block-scaled A, out_bscale],
    refused, [[rows, kernel, epilogue, scratch, leaves, persistent grid, persistent LDS], ...]].
(b) gemm_rule() below restates the rule in Python from that commit's source (the part make_plan plays in
    tests/test_topk_krange.py) and is compared with the hook over a sweep of shapes, epilogues and forced kernels.
(c) the refusals keep their error codes and messages; (d) the two queries encode.hip asks are the plans' own answers."""
import ctypes as C
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NUM_CU, LDS_BYTES, G256_LDS, G256P_MAX_N, SKINNY_MAX_M = 256, 160 * 1024, 128 * 1024, 8192, 128
EINVAL, EUNSUPPORTED = 1, 4
K128, K256, K256P, SKINNY, F8, F8_BSA = range(6)
STORE_ONLY = (0, 1, 2, 5, 6, 7)                      # the persistent kernel's epilogues
N_OUT = 23                                          # 1 + 3 parts x 7 fields, then the query slot


def _lib():
    import clipmi
    return clipmi._lib.lib()


def _dev():
    import clipmi
    return clipmi._lib.DEV_LIB          # CLIPMI_DEV_LIB=1: the development library (other algo-4 text, more block-scaled-A epilogues)


def _parts(out):
    return [tuple(out[1 + 7 * i:8 + 7 * i]) for i in range(out[0])]


def plan(M, N, K, epi, algo=0, leaf=0, leaf_in=0, dbg=0):
    """-> (0, parts) or (error code, message)"""
    import clipmi
    out = (C.c_int32 * N_OUT)()
    rc = _lib().clipmi_dbg_gemm_plan(M, N, K, epi, algo, leaf, leaf_in, dbg, out, N_OUT)
    return (rc, clipmi._lib.last_error()) if rc else (0, _parts(out))


def fp8_plan(M, N, K, epi, mx=1, bsa=0, out_bs=0):
    import clipmi
    out = (C.c_int32 * N_OUT)()
    rc = _lib().clipmi_dbg_gemm_fp8_plan(M, N, K, epi, mx, bsa, out_bs, out, N_OUT)
    return (rc, clipmi._lib.last_error()) if rc else (0, _parts(out))


def queries(M, N, K):
    """(gemm_resid_writes_leaves(M, N, K), gemm_fp8_emits_mx(M, N, K)): the hooks report them in out[22], refusal or not"""
    a, b = (C.c_int32 * N_OUT)(), (C.c_int32 * N_OUT)()
    _lib().clipmi_dbg_gemm_plan(M, N, K, 7, 0, 1, 0, 0, a, N_OUT)
    _lib().clipmi_dbg_gemm_fp8_plan(M, N, K, 1, 1, 0, 0, b, N_OUT)
    return bool(a[22]), bool(b[22])


# ---- the rule, restated from the parent commit's launch_gemm_algo / launch_gemm_fp8 -----------------------------------------
def p_lds(epi, fp8, N, K, dbg=0):
    nseg = K >> 8
    extra = 1024 if fp8 else (1024 + 256 * nseg * 8 + (8 if nseg < 4 else 0)) if epi in (5, 6) else 0
    return G256_LDS + N * 4 * (2 if fp8 else 1) + extra + (8192 + 2048 if dbg & 12 else 0)


def tiles256(M, N):
    return (N // 256) * ((M + 255) // 256)


def gemm_rule(M, N, K, epi, algo=0, leaf=False, leaf_in=False, dbg=0):
    """-> list of parts, or None where the launcher refuses. The split is written as the recursion the parent ran."""
    ln = epi in (5, 6)
    if ln and (K % 256 or K > 1024):
        return None
    if epi == 7 and (N % 256 or N > 1024):
        return None
    if algo in (4, 5):
        return None
    ok256 = N % 256 == 0 and K % 64 == 0 and K >= 128
    if algo == 2 and not ok256:
        return None
    ok256p = (ok256 and K % 128 == 0 and N <= G256P_MAX_N and epi in STORE_ONLY and K <= 1 << 20
              and p_lds(epi, False, N, K, dbg) <= LDS_BYTES)
    if algo == 3 and not ok256p:
        return None
    use256, use256p = algo in (2, 3), algo == 3
    if algo == 0 and ok256 and M >= 1024:
        tiles = tiles256(M, N)
        rounds = (tiles + NUM_CU - 1) // NUM_CU
        use256 = tiles * 100 >= rounds * NUM_CU * (72 if K >= 2048 else 78)
        use256p = use256 and ok256p and (tiles > NUM_CU or epi == 7)
        if ok256p and tiles > NUM_CU and epi != 4 and tiles % NUM_CU and (tiles % NUM_CU) * 100 < NUM_CU * 40:
            rows_main = (tiles // NUM_CU) * NUM_CU // (N // 256) * 256
            if 256 <= rows_main < M:
                main = gemm_rule(rows_main, N, K, epi, 3, leaf, leaf_in, dbg)
                rest = gemm_rule(M - rows_main, N, K, epi, 0, leaf, leaf_in, dbg)
                return None if main is None or rest is None else main + rest
    if M < 1:
        return None
    skinny = algo == 0 and M <= SKINNY_MAX_M and N % 16 == 0 and K % 32 == 0 and K >= 32
    if skinny and epi != 7:
        return [(M, SKINNY, epi, 0, 0, 0, 0)] if 0 <= epi <= 7 else None
    if skinny and epi == 7 and leaf:
        return [(M, SKINNY, 7, 0, 1, 0, 0)]
    if leaf_in:
        return None
    if use256p:
        return [(M, K256P, epi, 0, 0, min(tiles256(M, N), NUM_CU), p_lds(epi, False, N, K, dbg))]
    scratch = epi == 7
    ran = 3 if scratch else epi
    if skinny:
        return [(M, SKINNY, ran, 1, 0, 0, 0)]
    if not use256 and (N < 1 or K < 1 or N % 128 or K % 64):
        return None
    return [(M, K256 if use256 else K128, ran, int(scratch), 0, 0, 0)] if 0 <= ran <= 6 else None


def fp8_rule(M, N, K, epi, mx=1, bsa=False, out_bs=False):
    if M < 1 or N % 256 or K % 128 or K < 256:
        return None
    if bsa:
        if K > 4096 or epi not in ((2, 3, 5, 6, 8) if _dev() else (2, 3)):
            return None
        if (epi == 8 and N > 1024) or (epi in (5, 6) and (K % 256 or K > 1024)) or (epi == 5 and out_bs):
            return None
        return [(M, F8_BSA, epi, 0, 0, 0, 0)]
    tiles = tiles256(M, N)
    persist = mx == 1 and tiles > NUM_CU and K % 256 == 0 and N <= 3840
    if out_bs and not (persist and epi == 1):
        return None
    if persist and epi in (0, 1):
        return [(M, K256P, epi, 0, 0, min(tiles, NUM_CU), p_lds(epi, True, N, K))]
    return [(M, F8, epi, 0, 0, 0, 0)] if 0 <= epi <= 3 else None


# ---- (a) ---------------------------------------------------------------------------------------------------------------------
def test_pinned_table_of_the_parent_commit(clipmi):
    rows = json.load(open(os.path.join(ROOT, "tests", "golden", "gemm_plan_parent.json")))
    assert len(rows) >= 380
    kernels = set()
    for (kind, M, N, K, epi, a, b, c), refused, parts in rows:
        got = plan(M, N, K, epi, a, b & 1, b >> 1) if kind == "b" else fp8_plan(M, N, K, epi, a, b, c)
        want = [tuple(p) for p in parts]
        assert (got[0] != 0) == bool(refused), (kind, M, N, K, epi, a, b, c, got)
        if not refused:
            assert got[1] == want, (kind, M, N, K, epi, a, b, c, got, want)
            kernels.update(p[1] for p in want)
    assert kernels == {K128, K256, K256P, SKINNY, F8, F8_BSA}          # the table reaches every kernel family
    # the anchor row, derived by hand from the rule's text: 300 tiles = 1.17 rounds, 44 ragged tiles < 40 % of 256 -> 21 760 rows on the
    # persistent kernel, the other 3 840 on the 128 x 128 kernel into the f32 scratch rows + split_stats
    assert plan(25600, 768, 768, 7) == (0, [(21760, K256P, 7, 0, 0, 255, G256_LDS + 768 * 4), (3840, K128, 3, 1, 0, 0, 0)])


# ---- (b) ---------------------------------------------------------------------------------------------------------------------
SWEEP_M = sorted(set(range(1, 1101)) | {k * 256 + d for k in range(1, 30000 // 256 + 1) for d in (-1, 0, 1)})
SWEEP_N = (512, 768, 1024, 1536, 2304, 3072, 4096)
SWEEP_K = (512, 768, 1024, 3072, 4096)


@pytest.mark.parametrize("N", SWEEP_N)
def test_restated_rule_matches_the_plan(clipmi, N):
    L = _lib()
    out = (C.c_int32 * N_OUT)()
    for K in SWEEP_K:
        for epi in range(0, 9):
            for algo in range(0, 6):
                for leaf, leaf_in in ((0, 0), (1, 0), (0, 1), (1, 1)):
                    for M in SWEEP_M:
                        want = gemm_rule(M, N, K, epi, algo, leaf, leaf_in)
                        rc = L.clipmi_dbg_gemm_plan(M, N, K, epi, algo, leaf, leaf_in, 0, out, N_OUT)
                        assert (rc != 0) == (want is None), (M, N, K, epi, algo, leaf, leaf_in, rc, want)
                        if want is not None:
                            assert _parts(out) == want, (M, N, K, epi, algo, leaf, leaf_in, _parts(out), want)


def test_restated_rule_matches_the_plan_with_leaves_and_fp8(clipmi):
    for N in SWEEP_N:
        for K in SWEEP_K:
            for M in (1, 2, 50, 77, 100, 128, 129, 150, 1024, 4096, 21761, 21800):
                for epi in (5, 6, 7, 0):
                    for leaf, leaf_in in ((1, 0), (0, 1), (1, 1)):
                        want = gemm_rule(M, N, K, epi, 0, leaf, leaf_in)
                        got = plan(M, N, K, epi, 0, leaf, leaf_in)
                        assert (got[0] != 0) == (want is None) and (want is None or got[1] == want), (M, N, K, epi, leaf, leaf_in, got, want)
            for M in SWEEP_M[::5]:
                for epi in range(0, 9):
                    for mx in (0, 1, 2):
                        for bsa, out_bs in ((0, 0), (1, 0), (0, 1)):
                            want = fp8_rule(M, N, K, epi, mx, bsa, out_bs)
                            got = fp8_plan(M, N, K, epi, mx, bsa, out_bs)
                            assert (got[0] != 0) == (want is None) and (want is None or got[1] == want), (M, N, K, epi, mx, bsa, out_bs, got, want)


# ---- (c) ---------------------------------------------------------------------------------------------------------------------
def test_refusals_keep_their_codes_and_messages(clipmi):
    assert plan(512, 640, 768, 0, algo=2) == (EINVAL, "gemm256: N=640 K=768 (need N % 256 == 0, K % 64 == 0, K >= 128)")
    rc, msg = plan(512, 768, 768, 3, algo=3)                   # EPI_F32 is no store-only epilogue
    assert rc == EINVAL and msg.startswith("gemm256p: M=512 N=768 K=768 epi=3 (need N % 256 == 0, K % 128 == 0, a store-only epilogue")
    rc, msg = plan(512, 768, 64, 0, algo=3)
    assert rc == EINVAL and "gemm256p: M=512 N=768 K=64 epi=0" in msg
    rc, msg = plan(512, 768, 768, 0, algo=4)
    assert rc == EUNSUPPORTED and ("algo 4 (gemm2w, DESIGN 4.4g) was removed" if _dev() else "algo 4 exists in the development build only") in msg
    rc, msg = plan(512, 768, 768, 0, algo=5)
    assert rc == EUNSUPPORTED and "algo 5 (W-direct gemm256, DESIGN 4.4h) was removed" in msg
    for M, epi in ((129, 5), (4096, 6), (100, 7), (25600, 5)):             # ln_leaf_in off the skinny consumers
        rc, msg = plan(M, 768, 768, epi, leaf_in=1)
        assert rc == EINVAL and msg == "gemm: ln_leaf_in is read by the skinny LN-folded consumers only (M <= 128)", (M, epi, msg)
    assert plan(100, 2304, 768, 5, leaf_in=1) == (0, [(100, SKINNY, 5, 0, 0, 0, 0)])
    want = "gemm_fp8: e4m3 + block-scale output exists for the persistent QuickGELU form only"
    assert fp8_plan(43500, 3072, 768, 1, out_bs=1)[0] == 0
    for args in ((4100, 3072, 768, 1, 1), (43500, 3072, 768, 0, 1), (43500, 3072, 768, 1, 2), (43500, 3072, 768, 1, 0), (43500, 4096, 768, 1, 1)):
        assert fp8_plan(*args, out_bs=1) == (EINVAL, want), args
    assert plan(0, 768, 768, 0) == (EINVAL, "gemm: bad arguments")
    assert plan(512, 768, 768, 8) == (EINVAL, "gemm: unknown epilogue 8")
    assert plan(512, 768, 512, 5)[0] == 0 and "LN-folded epilogue 5 needs" in plan(512, 768, 2048, 5)[1]
    assert fp8_plan(512, 768, 768, 7) == (EINVAL, "gemm_fp8: epilogue 7")
    assert fp8_plan(512, 768, 768, 1, bsa=1) == (EINVAL, "gemm_fp8: block-scaled A with epilogue 1")
    assert (fp8_plan(512, 768, 768, 8, bsa=1)[0] == 0) == _dev()


# ---- (d) ---------------------------------------------------------------------------------------------------------------------
def test_queries_are_the_plans_answers(clipmi):
    """gemm_resid_writes_leaves / gemm_fp8_emits_mx (what encode.hip asks before it sizes and routes a buffer; slot 22 of the
    hooks' output) against the plans, in both directions, over the sweep: leaves = the residual producer's plan with a leaf
    buffer is ONE skinny launch that writes leaves; emits = the FP8 plan's QuickGELU case is the persistent kernel, which is
    also exactly where e4m3 + block-scale output is accepted. Both also against the shapes' closed forms."""
    yes = [0, 0]
    for N in SWEEP_N + (640,):
        for K in SWEEP_K + (48,):
            for M in [0] + SWEEP_M:
                leaves, emits = queries(M, N, K)
                p = plan(M, N, K, 7, 0, leaf=1)
                assert leaves == (p[0] == 0 and len(p[1]) == 1 and p[1][0][1] == SKINNY and p[1][0][4] == 1), (M, N, K, leaves, p)
                assert leaves == (1 <= M <= 128 and N % 256 == 0 and N <= 1024 and K % 32 == 0), (M, N, K)
                f = fp8_plan(M, N, K, 1)
                assert emits == (f[0] == 0 and f[1][0][1] == K256P), (M, N, K, emits, f)
                assert emits == (M >= 1 and N % 256 == 0 and K % 256 == 0 and tiles256(M, N) > NUM_CU and N <= 3840), (M, N, K)
                assert (fp8_plan(M, N, K, 1, out_bs=1)[0] == 0) == emits, (M, N, K)
                yes[0] += leaves
                yes[1] += emits
    assert min(yes) > 1000, yes           # both answers occur, often
