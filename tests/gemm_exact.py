"""Exact data for the bf16 GEMM family (helper of tests/test_gemm_exact_gpu.py; no test in here).

The recipe of tests/test_gemm256_exact_gpu.py: A dense in {-1, 0, 1}, W in {-1, 1} at about 5 % density, bias, residual and
old residual rows small integers, so that every product, partial sum and add is exact in f32 and every result an integer that
bf16 holds: a kernel's output must EQUAL the float64 reference. Three more conditions, asserted per case, so that a misplaced
row, column or statistic cannot hide: the expected output has no two equal rows and no two equal columns; rows that feed row
statistics carry a per-row offset (m mod 7 - 3) * 4 on top of integers in [-8, 8], so neighbouring rows differ in mean by whole
units; sums of squares per 256-column segment stay below 2^24.

Two places where the recipe has to give:
* W's density is max(5 %, 8 / K). At K = 32 .. 128 a 5 % row holds 1.6 .. 6.4 entries, so among a few hundred columns two W
  rows are empty or equal and their output columns could differ in the bias alone (seven values): equal columns are certain.
* M = 1. One row of sums of a dozen +-1 cannot be N distinct integers, so the bias is chosen from the float64 products such
  that the row is a shuffled run of consecutive integers (and the residual such that it stays one): single_row(). A row holds
  at most 2 * BOUND distinct integers of magnitude <= BOUND; N = 1024 at M = 1 repeats them and asserts exactly that many.
The data of a case is redrawn (next seed) until its reference meets the conditions: they are properties of the reference alone.

References are float64: on the CPU for small shapes, on the device (a.double() @ w.double().t()) for the large ones, never one of
the project's kernels."""
import ctypes as C
import functools

import numpy as np
import torch

BOUND = 256                  # |result| stays at or below it: integers that bf16 holds exactly
CPU_MACS = 1 << 27           # references up to this many multiply-adds are computed on the CPU
NAN = float("nan")
GUARD_BYTE = 0xA5            # guard rows of byte buffers (split residual rows)
LN_EPS = float(np.float32(1e-5))
N_PLAN = 23


def density(K):
    return max(0.05, 8.0 / K)


def row_offset(M):
    return ((torch.arange(M) % 7 - 3) * 4).double()[:, None]


def matmul64(a, w, gpu):
    """a w^T in float64 -> on `gpu`"""
    M, K = a.shape
    if M * w.shape[0] * K <= CPU_MACS:
        return (a.double() @ w.double().t()).to(gpu)
    return a.to(gpu).double() @ w.to(gpu).double().t()


def single_row(N, g):
    """M = 1: -> (t, r), integers [N]: t and t + r are both injective on any run of min(N, 2 BOUND) columns, |r| <= 3"""
    span = min(N, 2 * BOUND)
    assert span % 4 == 0
    v = torch.randperm(span, generator=g).repeat(N // span + 1)[:N]
    perm = torch.stack([torch.randperm(4, generator=g) for _ in range(span // 4)])
    v2 = v // 4 * 4 + perm[v // 4, v % 4]                  # the values of each aligned block of four, shuffled among themselves
    return (v - span // 2).double(), (v2 - v).double()


def count_distinct(x):
    """number of distinct rows of x (float64 [R][C]): distinct hashes of the bit patterns, so never an overcount"""
    g = torch.Generator(device="cpu"); g.manual_seed(12345)
    r = (torch.randint(0, 1 << 62, (2 * x.shape[1],), generator=g) * 2 + 1).to(x.device)
    # a linear hash modulo 2^64 of the rows' 32-bit words (+ 0.0: -0 and +0 are one value)
    words = (x + 0.0).reshape(-1).view(torch.int32).reshape(x.shape[0], 2 * x.shape[1])
    h = (words.to(torch.int64) * r).sum(1)
    return torch.unique(h).numel()


def assert_distinct(ref, what):
    M, N = ref.shape
    want_cols = N if (M > 1 or N <= 2 * BOUND) else 2 * BOUND
    rows, cols = count_distinct(ref), count_distinct(ref.t())
    assert rows == M and cols == want_cols, f"{what}: {rows} distinct rows of {M}, {cols} distinct columns (want {want_cols})"


def is_distinct(ref):
    try:
        assert_distinct(ref, "")
    except AssertionError:
        return False
    return True


def assert_exact_reference(ref, what, bound=BOUND):
    peak = ref.abs().max().item()
    print(f"{what}: max |result| {peak}")
    assert peak <= bound and torch.equal(ref.float().double(), ref), f"{what}: max |result| {peak}"
    assert_distinct(ref, what)


def redraw(make, seed, ok):
    """make(seed), make(seed + 1000003), ... until ok(case): the conditions on the reference select the data"""
    for attempt in range(64):
        c = make(seed + 1000003 * attempt)
        if ok(c):
            return c
    raise AssertionError("no data met the conditions in 64 draws")


def sparse_pm1(N, K, g):
    return (torch.rand(N, K, generator=g) < density(K)).float() * (torch.randint(0, 2, (N, K), generator=g).float() * 2 - 1)


# ---- plain epilogues 0-3 ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=3)
def plain_case(M, N, K, gpu):
    """Operands (bf16 / f32 on the device) and the float64 references of one shape, shared by its epilogues and kernels:
    ref = a w^T + bias, ref2 = ref + res."""
    def make(seed):
        g = torch.Generator(device="cpu"); g.manual_seed(seed)
        a = torch.randint(-1, 2, (M, K), generator=g).float()
        w = sparse_pm1(N, K, g)
        bias = torch.randint(-3, 4, (N,), generator=g).double()
        res = torch.randint(-3, 4, (M, N), generator=g).double()
        acc = matmul64(a, w, gpu)
        if M == 1:
            t, r = single_row(N, g)
            bias, res = t - acc[0].cpu(), r[None, :]
        bias, res = bias.to(gpu), res.to(gpu)
        ref = acc + bias
        return dict(a=a.to(torch.bfloat16).to(gpu), w=w.to(torch.bfloat16).to(gpu), bias=bias.float(), res=res.float(),
                    ref=ref, ref2=ref + res)
    return redraw(make, M * 5 + N * 3 + K, lambda c: is_distinct(c["ref"]) and is_distinct(c["ref2"]))


def run_plain(clipmi, gpu, M, N, K, epi, algo):
    """One launch of clipmi_dbg_gemm_bf16 on exact data; -> the M output rows, which equal the float64 reference."""
    L = clipmi._lib.lib()
    c = plain_case(M, N, K, gpu)
    what = f"algo={algo} M={M} N={N} K={K} epi={epi}"
    ref = c["ref2"] if epi == 2 else c["ref"]
    assert_exact_reference(ref, what)
    ref = ref.float().to(torch.bfloat16) if epi == 0 else ref.float()
    out = torch.full((M + 1, N), NAN, dtype=ref.dtype, device=gpu)           # + 1 guard row
    if epi == 2:
        out[:M] = c["res"]
    rc = L.clipmi_dbg_gemm_bf16(c["a"].data_ptr(), c["w"].data_ptr(), c["bias"].data_ptr(), out.data_ptr(), M, N, K, epi | (algo << 8), None)
    clipmi._lib.check(rc, what)
    torch.cuda.synchronize()
    assert torch.isnan(out[M]).all(), f"{what}: wrote past row M"
    bad = out[:M] != ref
    nbad = int(bad.sum().item())
    assert nbad == 0, f"{what}: {nbad} of {bad.numel()} differ, max |diff| {(out[:M].double() - ref.double()).abs().max().item()}, " \
                      f"first at (row, column) {tuple(bad.nonzero()[0].tolist())}"
    return out[:M]


def qgelu64(x):
    return x * torch.sigmoid(1.702 * x)


def run_plain_qgelu(clipmi, gpu, M, N, K, algo):
    """Epilogue 1: x = a w^T + bias is exact, quick_gelu4 is one v_exp_f32 and one v_rcp_f32 of about 1 ulp each plus the rounding
    of the exponent's argument (1.7e-6 relative at |x| <= 32 in a restatement): 2^-16 |ref|, and 2^-8 |ref| for the bf16 store."""
    L = clipmi._lib.lib()
    c = plain_case(M, N, K, gpu)
    what = f"algo={algo} M={M} N={N} K={K} epi=1"
    assert_exact_reference(c["ref"], what, bound=32)
    ref = qgelu64(c["ref"])
    out = torch.full((M + 1, N), NAN, dtype=torch.bfloat16, device=gpu)
    clipmi._lib.check(L.clipmi_dbg_gemm_bf16(c["a"].data_ptr(), c["w"].data_ptr(), c["bias"].data_ptr(), out.data_ptr(), M, N, K,
                                             1 | (algo << 8), None), what)
    torch.cuda.synchronize()
    assert torch.isnan(out[M]).all(), f"{what}: wrote past row M"
    err, tol = (out[:M].double() - ref).abs(), (2.0 ** -8 + 2.0 ** -16) * ref.abs()
    assert torch.isfinite(out[:M].float()).all() and (err <= tol).all(), f"{what}: worst err / bound {(err / tol.clamp_min(1e-300)).max().item()}"


def plan(clipmi, M, N, K, epi, algo=0, leaf=0, leaf_in=0):
    """clipmi_dbg_gemm_plan -> (0, [(rows, kernel, epilogue, scratch, leaves, grid, lds), ...]) or (error code, [])"""
    out = (C.c_int32 * N_PLAN)()
    rc = clipmi._lib.lib().clipmi_dbg_gemm_plan(M, N, K, epi, algo, leaf, leaf_in, 0, out, N_PLAN)
    return rc, ([] if rc else [tuple(out[1 + 7 * i:8 + 7 * i]) for i in range(out[0])])


# ---- split residual rows and their statistics -----------------------------------------------------------------------------------
def split_rows(x, gpu):
    """x: integers that bf16 holds, [M][W] -> split rows uint8 [M + 1][3 W] on the device: hi = the integer as bf16, every
    remainder byte 128, and a guard row of GUARD_BYTE"""
    M, W = x.shape
    x3 = torch.full((M + 1, 3 * W), GUARD_BYTE, dtype=torch.uint8, device=gpu)
    hi = x.to(gpu).to(torch.bfloat16)
    assert torch.equal(hi.double(), x.to(gpu).double())
    x3[:M, :2 * W] = hi.contiguous().view(torch.uint8)
    x3[:M, 2 * W:] = 128
    return x3


def exact_stats(x):
    """x: float64 integers [M][W] -> (part [M][W / 256][2], leaves [M][W / 4][2]) as f32: the exact (sum, sum of squares)"""
    M, W = x.shape
    def pairs(width):
        xs = x.reshape(M, W // width, width)
        p = torch.stack([xs.sum(-1), (xs * xs).sum(-1)], dim=-1)
        assert p.abs().max().item() < 2 ** 24
        return p.float()
    return pairs(256), pairs(4)


def with_guard(t):
    """t [M][...] f32 -> [M + 1][...] with a NaN guard row"""
    return torch.cat([t, torch.full_like(t[:1], NAN)], dim=0).contiguous()


@functools.lru_cache(maxsize=2)
def resid_case(M, N, K, gpu):
    """Epilogue 7: new = old + a w^T + bias, all integers; old carries the per-row offset (the new rows feed the statistics)."""
    def make(seed):
        g = torch.Generator(device="cpu"); g.manual_seed(seed)
        a = torch.randint(-1, 2, (M, K), generator=g).float()
        w = sparse_pm1(N, K, g)
        bias = torch.randint(-3, 4, (N,), generator=g).double()
        old = torch.randint(-8, 9, (M, N), generator=g).double() + row_offset(M)
        acc = matmul64(a, w, gpu)
        if M == 1:
            bias = single_row(N, g)[0] - acc[0].cpu() - old[0]
        new = acc + bias.to(gpu) + old.to(gpu)
        return dict(a=a.to(torch.bfloat16).to(gpu), w=w.to(torch.bfloat16).to(gpu), bias=bias.float().to(gpu), old=old, new=new)
    return redraw(make, M * 7 + N * 3 + K + 1, lambda c: is_distinct(c["new"]))


def check_resid(clipmi, gpu, M, N, K, algo, leaf=False):
    """One launch of the split-residual producer; every output equals the exact integers. -> False where the hook refuses."""
    L = clipmi._lib.lib()
    c = resid_case(M, N, K, gpu)
    what = f"resid_ln {'leaf' if leaf else 'algo=%d' % algo} M={M} N={N} K={K}"
    assert_exact_reference(c["new"], what)
    x3 = split_rows(c["old"], gpu)
    want_x3 = split_rows(c["new"], gpu)
    want_part, want_leaf = exact_stats(c["new"])
    if leaf:
        stat = torch.full((M + 1, N // 4, 2), NAN, dtype=torch.float32, device=gpu)
        rc = L.clipmi_dbg_gemm_resid_ln_leaf(c["a"].data_ptr(), c["w"].data_ptr(), c["bias"].data_ptr(), x3.data_ptr(), stat.data_ptr(),
                                             M, N, K, None)
        want = want_leaf
    else:
        stat = torch.full((M + 1, N // 256, 2), NAN, dtype=torch.float32, device=gpu)
        tmp = torch.full((M + 1, N), NAN, dtype=torch.float32, device=gpu)
        rc = L.clipmi_dbg_gemm_resid_ln(c["a"].data_ptr(), c["w"].data_ptr(), c["bias"].data_ptr(), x3.data_ptr(), stat.data_ptr(),
                                        tmp.data_ptr(), M, N, K, algo, None)
        want = want_part
    accepted = plan(clipmi, M, N, K, 7, algo, 1 if leaf else 0)[0] == 0
    assert (rc == 0) == accepted, f"{what}: hook returned {rc} ({clipmi._lib.last_error()}), the plan {'accepts' if accepted else 'refuses'}"
    if rc:
        return False
    torch.cuda.synchronize()
    assert torch.isnan(stat[M]).all() and (leaf or torch.isnan(tmp[M]).all()) and (x3[M] == GUARD_BYTE).all(), f"{what}: wrote past row M"
    assert torch.equal(x3[:M, :2 * N].view(torch.bfloat16), want_x3[:M, :2 * N].view(torch.bfloat16)), f"{what}: hi halves"
    assert torch.equal(x3[:M, 2 * N:], want_x3[:M, 2 * N:]), f"{what}: remainder bytes"
    assert torch.equal(stat[:M], want), f"{what}: statistics"
    return True


# ---- LN-folded consumers --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def ln_case(M, N, K, gpu):
    """Epilogues 5, 6, every operand built here: x3 from integers with the per-row offset, part / leaves their exact sums, integer
    folded weights, colsum their exact row sums, integer cb. acc = x wg^T is exact in f32; only ln_row_stats and ln_apply round.
    The float64 terms of the reference stay in the case for the bound."""
    def make(seed):
        g = torch.Generator(device="cpu"); g.manual_seed(seed)
        x = torch.randint(-8, 9, (M, K), generator=g).double() + row_offset(M)
        # 16 entries of +-1 per row of the folded weights whatever K, so that |rstd (acc - mean colsum)| stays near 4 sigma = 17 and
        # the QuickGELU argument within 32 with cb in [-12, 12]
        wg = (torch.rand(N, K, generator=g) < 16.0 / K).float() * (torch.randint(0, 2, (N, K), generator=g).float() * 2 - 1)
        cb = torch.randint(-12, 13, (N,), generator=g).double()
        colsum = wg.double().sum(1)
        part, leaf = exact_stats(x)
        acc = matmul64(x.float(), wg, gpu)
        assert acc.abs().max().item() < 2 ** 24 / 64            # every partial sum of a row is exact in f32 with room to spare
        s, q = x.sum(1), (x * x).sum(1)
        mean = s / K
        rstd = 1.0 / torch.sqrt(q / K - mean * mean + LN_EPS)
        mean, rstd, cs, cbd = mean.to(gpu)[:, None], rstd.to(gpu)[:, None], colsum.to(gpu)[None, :], cb.to(gpu)[None, :]
        pre = rstd * (acc - mean * cs) + cbd
        return dict(x3=split_rows(x, gpu), wg=wg.to(torch.bfloat16).to(gpu), cb=cb.float().to(gpu), colsum=colsum.float().to(gpu),
                    part=with_guard(part.to(gpu)), leaf=with_guard(leaf.to(gpu)), acc=acc, mean=mean, rstd=rstd, cs=cs, cbd=cbd, pre=pre,
                    part_cpu=part)
    c = redraw(make, M * 11 + N * 3 + K + 2,
               lambda c: c["pre"].abs().max().item() <= 32 and is_distinct(c["pre"]) and is_distinct(qgelu64(c["pre"])))
    assert torch.equal(c["wg"].double().sum(1), c["cs"][0]) and c["pre"].abs().max().item() <= 32          # QuickGELU: |x| <= 32
    return c


def ln_restated_ratio(c):
    """ln_row_stats and ln_apply of csrc/gemm.hpp restated in float32 numpy on the case's own inputs (fma = one rounding of the
    float64 value, exact to far below an f32 ulp here) -> the worst |restated - float64 reference| in units of
    2^-23 (|acc| + |mean colsum|) rstd + 2^-23 |cb|  with c = 1."""
    f32 = np.float32
    part = c["part_cpu"].numpy()
    K = part.shape[1] * 256
    s, q = part[:, 0, 0].copy(), part[:, 0, 1].copy()
    for j in range(1, part.shape[1]):
        s, q = (s + part[:, j, 0]).astype(f32), (q + part[:, j, 1]).astype(f32)
    inv = f32(1.0) / f32(K)
    mean = (s * inv).astype(f32)
    var = (-mean.astype(np.float64) * mean.astype(np.float64) + (q * inv).astype(f32).astype(np.float64)).astype(f32)
    var = np.maximum(var, f32(0))
    rstd = (1.0 / np.sqrt((var + f32(1e-5)).astype(f32).astype(np.float64))).astype(f32)
    acc, cs, cb = c["acc"].cpu().numpy(), c["cs"].cpu().numpy(), c["cbd"].cpu().numpy()
    t = (-mean.astype(np.float64)[:, None] * cs + acc).astype(f32)
    r = (t.astype(np.float64) * rstd.astype(np.float64)[:, None] + cb).astype(f32)
    err = np.abs(r.astype(np.float64) - c["pre"].cpu().numpy())
    unit = ln_bound_terms(c)
    unit, cbt = unit[0].cpu().numpy(), unit[1].cpu().numpy()
    return float(np.max(np.maximum(err - cbt, 0) / np.maximum(unit, 1e-300)))


def ln_bound_terms(c):
    """(2^-23 (|acc| + |mean colsum|) rstd, 2^-23 |cb|), float64 [M][N]"""
    return 2.0 ** -23 * (c["acc"].abs() + (c["mean"] * c["cs"]).abs()) * c["rstd"], 2.0 ** -23 * c["cbd"].abs().expand_as(c["acc"])


def check_ln(clipmi, gpu, M, N, K, epi, algo, c_ln, leaf=False):
    """One launch of an LN-folded consumer, element by element under
        |got - ref| <= 2^-8 |ref| + c 2^-23 (|acc| + |mean colsum|) rstd + 2^-23 |cb|    (+ 2^-16 |ref| behind QuickGELU).
    -> the output rows, or None where the hook refuses (which the plan must then do too)."""
    L = clipmi._lib.lib()
    c = ln_case(M, N, K, gpu)
    what = f"gemm_ln {'leaf' if leaf else 'algo=%d' % algo} M={M} N={N} K={K} epi={epi}"
    ref = qgelu64(c["pre"]) if epi == 6 else c["pre"]
    peak = ref.abs().max().item()
    print(f"{what}: max |result| {peak}")
    assert peak <= BOUND
    assert_distinct(ref, what)
    out = torch.full((M + 1, N), NAN, dtype=torch.bfloat16, device=gpu)
    if leaf:
        rc = L.clipmi_dbg_gemm_ln_leaf(c["x3"].data_ptr(), c["wg"].data_ptr(), c["cb"].data_ptr(), c["colsum"].data_ptr(), c["leaf"].data_ptr(),
                                       out.data_ptr(), M, N, K, epi, None)
    else:
        rc = L.clipmi_dbg_gemm_ln(c["x3"].data_ptr(), c["wg"].data_ptr(), c["cb"].data_ptr(), c["colsum"].data_ptr(), c["part"].data_ptr(),
                                  out.data_ptr(), M, N, K, epi | (algo << 8), None)
    accepted = plan(clipmi, M, N, K, epi, algo, 0, 1 if leaf else 0)[0] == 0
    assert (rc == 0) == accepted, f"{what}: hook returned {rc} ({clipmi._lib.last_error()}), the plan {'accepts' if accepted else 'refuses'}"
    if rc:
        return None
    torch.cuda.synchronize()
    assert torch.isnan(out[M]).all(), f"{what}: wrote past row M"
    unit, cbt = ln_bound_terms(c)
    tol = 2.0 ** -8 * ref.abs() + c_ln * unit + cbt + (2.0 ** -16 * ref.abs() if epi == 6 else 0)
    err = (out[:M].double() - ref).abs()
    bad = ~(err <= tol)                                   # (a NaN is bad)
    nbad = int(bad.sum().item())
    assert nbad == 0, f"{what}: {nbad} of {bad.numel()} outside the bound, worst err / bound {(err / tol.clamp_min(1e-300)).nan_to_num(1e30).max().item()}, " \
                      f"first at (row, column) {tuple(bad.nonzero()[0].tolist())}"
    return out[:M]
