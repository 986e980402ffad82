"""-m gpu: every bf16 GEMM kernel (128 x 128, 256 x 256, persistent, skinny), the shared epilogues 0 - 7 and a split plan on EXACT
data at their edges, against float64 (data, conditions and comparisons: tests/gemm_exact.py).

Cases 1 - 6 are integers end to end and compare with torch.equal: one dropped, duplicated, stale or misplaced product, bias
column, residual row or statistic is a wrong integer. Case 7 (the LN-folded consumers 5, 6) has an exact accumulator and rounds
only in ln_row_stats / ln_apply; it is held element by element to

    |got - ref| <= 2^-8 |ref| + C_LN 2^-23 (|acc| + |mean colsum|) rstd + 2^-23 |cb|      (+ 2^-16 |ref| behind QuickGELU)

The first term is the bf16 store. C_LN = 16: four times the worst ratio that a float32 numpy restatement of ln_row_stats and
ln_apply (gemm_exact.ln_restated_ratio, on the CPU, on these very inputs, never from a kernel's output) reaches against the
float64 reference over all cases of test_ln_consumers and the split plan's: measured 3.86 at K = 768 (4 x 3.86 = 15.4, rounded up to 16;
test_ln_bound_constant recomputes it). A row that reads its neighbour's statistics is off by whole units of the mean
((m mod 7 - 3) * 4 per row): thousands of times the bound.

Every output buffer is NaN-filled (split rows: a byte pattern) with one guard row behind row M that must stay untouched; every
case asserts |result| <= 256, the float32 round trip of its reference, and that the reference has no two equal rows or columns.
A hook may refuse a forced kernel only where clipmi_dbg_gemm_plan refuses the same arguments."""
import pytest
import torch

import gemm_exact as ge

pytestmark = pytest.mark.gpu

K128, K256, K256P, SKINNY = range(4)        # GemmKernel of csrc/gemm_plan.hpp
C_LN = 16.0
PLAIN = [0, 2, 3]


# ---- 1. the 128 x 128 kernel (algo 1) -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("epi", PLAIN)
@pytest.mark.parametrize("M,N,K", [(1, 128, 64), (1, 128, 128), (1, 128, 192),          # one K-tile (no prefetch), two, an odd count whose
                                   (129, 128, 128), (129, 128, 192),                     # last tile sits in buffer 0; one row and two row tiles
                                   (127, 128, 64), (128, 128, 64), (129, 128, 64)])      # M around the tile edge (1: above)
def test_gemm128_edges(clipmi, gpu, M, N, K, epi):
    ge.run_plain(clipmi, gpu, M, N, K, epi, 1)


TILES_128 = [(r, c) for r in (1, 7, 8, 9, 17) for c in (1, 7, 8, 9, 17)]


@pytest.mark.parametrize("rt,ct", TILES_128)
def test_gemm128_tile_order(clipmi, gpu, rt, ct):
    """gemm_tile_coords with 8 x 8 panels: grids that are and are not multiples of 8 (the XCD split), row and column counts below,
    at and above a panel, a ragged last row tile. A tile computed twice leaves another one NaN."""
    ge.run_plain(clipmi, gpu, 128 * rt - 5, 128 * ct, 64, 3, 1)


# ---- 2. the 256 x 256 kernel (algo 2) -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("epi", PLAIN)
@pytest.mark.parametrize("M,N,K", [(1, 256, 128), (1, 256, 192), (1, 256, 256), (257, 256, 192), (257, 256, 256),
                                   (255, 256, 128), (256, 256, 128), (257, 256, 128)])
def test_gemm256_edges(clipmi, gpu, M, N, K, epi):
    ge.run_plain(clipmi, gpu, M, N, K, epi, 2)


TILES_256 = [(r, c) for r in (1, 7, 8, 9, 17) for c in (1, 3, 4, 5, 9)]


@pytest.mark.parametrize("rt,ct", TILES_256)
def test_gemm256_tile_order(clipmi, gpu, rt, ct):
    """gemm_tile_coords with this kernel's 8 x 4 panels."""
    ge.run_plain(clipmi, gpu, 256 * rt - 5, 256 * ct, 128, 3, 2)


# ---- 3. the persistent kernel (algo 3), with bias ---------------------------------------------------------------------------------
@pytest.mark.parametrize("epi", [0, 2])
@pytest.mark.parametrize("K", [128, 256, 384])
@pytest.mark.parametrize("M", [1, 257, 32768, 32769])
def test_gemm256p_edges(clipmi, gpu, M, K, epi):
    """N = 512: M = 257 two tiles per column panel; M = 32768 is 256 tiles, exactly one per workgroup; M = 32769 is 258 tiles: two
    workgroups walk a second tile, and the extra tiles are ragged M-edge tiles."""
    rc, parts = ge.plan(clipmi, M, 512, K, epi, 3)
    assert rc == 0 and len(parts) == 1 and parts[0][1] == K256P and parts[0][5] == min(256, 2 * ((M + 255) // 256))
    ge.run_plain(clipmi, gpu, M, 512, K, epi, 3)


# ---- 4. a split plan (algo 0) -----------------------------------------------------------------------------------------------------
SPLIT = (65836, 256, 256)


def _assert_split_plan(clipmi, epi):
    M, N, K = SPLIT
    rc, parts = ge.plan(clipmi, M, N, K, epi, 0)
    assert rc == 0 and len(parts) == 2, f"epilogue {epi}: the plan no longer splits this shape: {parts}"
    assert parts[0][:2] == (65536, K256P) and parts[1][0] == M - 65536 and parts[1][1] != K256P, parts


@pytest.mark.parametrize("epi", [0, 2])
def test_split_plan_plain(clipmi, gpu, epi):
    """65536 rows on the persistent kernel and 300 on another one: every row is compared, so both sides of the seam are."""
    _assert_split_plan(clipmi, epi)
    ge.run_plain(clipmi, gpu, *SPLIT, epi, 0)


def test_split_plan_resid_producer(clipmi, gpu):
    """Epilogue 7 across the seam: the persistent part's fused store pass, the remainder through the scratch rows and split_stats."""
    _assert_split_plan(clipmi, 7)
    assert ge.check_resid(clipmi, gpu, *SPLIT, 0)


def test_split_plan_ln_consumer(clipmi, gpu):
    """Epilogue 5 across the seam (rstd is no integer: the bound of case 7, every row)."""
    _assert_split_plan(clipmi, 5)
    ratio = ge.ln_restated_ratio(ge.ln_case(*SPLIT, gpu))
    print(f"restated ln_row_stats / ln_apply: worst ratio {ratio}")
    assert 4 * ratio <= C_LN
    assert ge.check_ln(clipmi, gpu, *SPLIT, 5, 0, C_LN) is not None


# ---- 5. the skinny kernel (algo 0, M <= 128) ----------------------------------------------------------------------------------------
SKINNY_SHAPES = (
    # K: one real K-step in the prefetch ring; the depth-16 ring (K <= 512) partly and exactly full; the depth-32 ring (K > 512)
    # partly full (544), exactly full (1024), and wrapped to step counts that are no multiple of it (33, 63, 65 steps)
    [(17, 48, K) for K in (32, 64, 96, 480, 512, 544, 1024, 1056, 2016, 2080)]
    + [(M, 48, 96) for M in (1, 15, 16, 127, 128)]          # (17: above)
    + [(1, 16, 32), (17, 16, 32), (1, 528, 32), (17, 528, 32),
       (128, 2048, 32),          # 1024 waves: the last shape with one-wave workgroups
       (128, 2064, 32),          # 1032 waves: four-wave workgroups, the last one holds one strip
       (17, 128, 64)])           # the 128 x 128 kernel takes it too


@pytest.mark.parametrize("epi", PLAIN)
@pytest.mark.parametrize("M,N,K", SKINNY_SHAPES)
def test_gemm_skinny_edges(clipmi, gpu, M, N, K, epi):
    rc, parts = ge.plan(clipmi, M, N, K, epi, 0)
    assert rc == 0 and len(parts) == 1 and parts[0][1] == SKINNY
    out = ge.run_plain(clipmi, gpu, M, N, K, epi, 0)
    if N % 128 == 0 and K % 64 == 0:
        assert torch.equal(ge.run_plain(clipmi, gpu, M, N, K, epi, 1), out), "skinny kernel differs from the tiled kernel's bits"


# ---- epilogue 1 on the plain kernels, one shape each ----------------------------------------------------------------------------------
@pytest.mark.parametrize("algo,M,N,K", [(0, 17, 48, 96), (1, 129, 128, 192), (2, 257, 256, 192), (3, 257, 512, 256)])
def test_gemm_qgelu_on_exact_arguments(clipmi, gpu, algo, M, N, K):
    ge.run_plain_qgelu(clipmi, gpu, M, N, K, algo)


# ---- 6. the split-residual producer (epilogue 7) ------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 17, 128, 129, 257, 300])
@pytest.mark.parametrize("K", [128, 256])
@pytest.mark.parametrize("N", [256, 1024])
def test_resid_producers(clipmi, gpu, M, N, K):
    """x3 (hi = the integer as bf16, every remainder byte 128) += a w^T + bias: new hi halves, remainder bytes, the (sum, sum of
    squares) of every 256-column segment and, on the skinny leaf path, of every 4-column group equal the exact integers."""
    ran = [algo for algo in (0, 1, 2, 3) if ge.check_resid(clipmi, gpu, M, N, K, algo)]
    assert ran == [0, 1, 2, 3]                 # (these shapes suit every kernel; check_resid holds a refusal to the plan's)
    if M <= 128:
        assert ge.check_resid(clipmi, gpu, M, N, K, 0, leaf=True)


# ---- 7. the LN-folded consumers (epilogues 5, 6) --------------------------------------------------------------------------------------
LN_M, LN_K = [1, 17, 128, 129, 257], [256, 512, 768, 1024]


@pytest.mark.parametrize("epi", [5, 6])
@pytest.mark.parametrize("M", LN_M)
@pytest.mark.parametrize("K", LN_K)
def test_ln_consumers(clipmi, gpu, M, K, epi):
    """One to four statistics segments; N = 256 on every kernel, N = 48 on the skinny kernel; leaves for M <= 128."""
    outs = [ge.check_ln(clipmi, gpu, M, 256, K, epi, algo, C_LN) for algo in (0, 1, 2, 3)]
    assert all(o is not None for o in outs)
    if M <= 128:
        assert ge.check_ln(clipmi, gpu, M, 256, K, epi, 0, C_LN, leaf=True) is not None
        assert ge.plan(clipmi, M, 48, K, epi, 0)[1][0][1] == SKINNY
        assert ge.check_ln(clipmi, gpu, M, 48, K, epi, 0, C_LN) is not None
        assert ge.check_ln(clipmi, gpu, M, 48, K, epi, 0, C_LN, leaf=True) is not None
    else:
        assert all(ge.check_ln(clipmi, gpu, M, 48, K, epi, algo, C_LN) is None for algo in (0, 1, 2, 3))      # refused, as the plan does


def test_ln_bound_constant(gpu):
    """C_LN is four times the worst ratio of the float32 restatement over the cases above, rounded up: measured 3.86 (K = 768, whose 1 / K is no power of two)."""
    worst = max(ge.ln_restated_ratio(ge.ln_case(M, N, K, gpu)) for M in LN_M for K in LN_K for N in (256, 48) if N == 256 or M <= 128)
    print(f"restated ln_row_stats / ln_apply: worst ratio {worst}")
    assert 4 * worst <= C_LN <= 8 * worst
