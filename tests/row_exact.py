"""Data, float64 references and bounds for the towers' row kernels (helper of tests/test_rows_exact_gpu.py and
tests/test_rows_exact.py; no test in here): LayerNorm in every form LnArgs selects, gather_rows, split_stats and the two FP8
row quantisers. House style of tests/gemm_exact.py: float64 references, NaN- or byte-pattern-filled outputs with one guard row
behind row M, per-row offsets (m mod 7 - 3) * 4, data redrawn until the reference has no two equal rows or columns.

LayerNorm data comes in two classes.
* exact: row m is c_m + a_m s_m, s_m a balanced +-1 vector shuffled per row, a_m = 2^-3 .. 2^3, c_m the per-row offset, gamma
  signed powers of two 2^-2 .. 2^2, beta a shuffled run of distinct eighths. Sum, mean (= c_m), deviations (= +-a_m) and
  variance (= a_m^2) are then exact in f32 in the kernel's order (ln_restated below asserts it for every case), only the
  addition of eps, rsqrtf and the final multiply-add round. From M = 3 on, row 1 is constant (variance 0: the output is beta
  exactly) and row 2 has the mean 10000 with unit deviations. The `beta0` variant (the FP8 form's) has beta = 0, so that the
  constant row is a row of zeros, and from M = 4 on a row 3 of magnitude 2^-60.
  LayerNorm removes c_m, so two rows are equal in the reference exactly when their deviations a_m s_m are: at W = 4 there are six
  balanced sign vectors, rows cycle through 6 x 21 (vector, magnitude) pairs and M = 1001 must repeat them; every wider case
  has M distinct rows. The condition asserted is: as many distinct reference rows as distinct deviation rows, and M of them
  from W = 128 on.
* random: the data of test_kernels_gpu.py::test_layernorm - N(1.5, 3) with one outlier of 80, gamma = 1 + 0.1 N, beta = 0.1 N.

Bound, per element:  |got - ref| <= C 2^-23 (A rstd |gamma| + |beta|)  (+ 2^-8 |ref| behind a bf16 store), A = |x - mean| in the
exact class (mean and deviations carry no error there) and |x| + |mean| in the random class. C is four times the worst ratio
that ln_restated - the kernel's own order in float32 numpy: per-lane sums over the four column groups, the xor butterfly, two
passes - reaches against float64 over all cases of the class, rounded up; the factor four also carries v_rsq_f32 (about 1 ulp),
which numpy's correctly rounded 1 / sqrt does not model. tests/test_rows_exact.py recomputes the ratios on the CPU."""
import functools

import numpy as np
import torch

import gemm_exact as ge

NAN = float("nan")
GUARD_BYTE = ge.GUARD_BYTE
EPS = ge.LN_EPS
EINVAL = 1

LN_M = (1, 3, 4, 5, 1001)                    # four rows a block: one partly filled block, a full one, ragged last blocks
LN_W_256 = (256, 512, 768, 1024)             # the widths of the split and FP8 forms
LN_W = (4, 128, 252, 260, 1020) + LN_W_256   # f32 input: one lane, half a wave, groups that end inside a 256-column step
# C per class: 4 x the worst restated ratio, rounded up (test_rows_exact.py::test_ln_bound_constants; the measured ratios are
# in its docstring)
C_EXACT = 3.0
C_RANDOM = 11.0
C_OF = {"exact": C_EXACT, "beta0": C_EXACT, "random": C_RANDOM}


# ---- LayerNorm ------------------------------------------------------------------------------------------------------------------
def ln64(x, gamma, beta):
    """float64 LayerNorm(eps = float32(1e-5)) of the f32 values x -> (ref, mean, rstd), all float64"""
    xd = x.double()
    mean = xd.mean(1, keepdim=True)
    var = ((xd - mean) ** 2).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + EPS)
    return (xd - mean) * rstd * gamma.double() + beta.double(), mean, rstd


def _distinct_rows_ok(ref, dev, W):
    rows = ge.count_distinct(ref)
    return rows == ge.count_distinct(dev) and (W < 128 or rows == ref.shape[0]) and ge.count_distinct(ref.t()) == ref.shape[1]


def _exact_rows(M, W, g, beta0):
    """-> (c [M][1], a [M][1], s [M][W]) float64"""
    base = torch.cat([torch.ones(W // 2), -torch.ones(W // 2)]).double()
    if W == 4:
        pats = torch.tensor([[1, 1, -1, -1], [1, -1, 1, -1], [1, -1, -1, 1], [-1, 1, 1, -1], [-1, 1, -1, 1], [-1, -1, 1, 1]]).double()
        m = torch.arange(M)
        s, e = pats[m % 6], ((m // 6) % 21 - 10).double()
    else:
        s = base[torch.rand(M, W, generator=g).argsort(1)]
        e = torch.randint(-3, 4, (M,), generator=g).double()
    a, c = torch.exp2(e)[:, None], ge.row_offset(M).clone()
    if M >= 3:
        a[1] = 0.0                       # the constant row
        c[2], a[2] = 10000.0, 1.0        # a mean near 1e4 with unit deviations
    if beta0 and M >= 4:
        c[3], a[3] = 0.0, 2.0 ** -60     # tiny magnitudes
    return c, a, s


@functools.lru_cache(maxsize=None)
def ln_case(cls, M, W):
    """One LayerNorm case on the CPU: x, gamma, beta (f32), ref (float64) and `unit` = 2^-23 (A rstd |gamma| + |beta|)."""
    def make(seed):
        g = torch.Generator(device="cpu"); g.manual_seed(seed)
        if cls == "random":
            x = torch.randn(M, W, generator=g) * 3 + 1.5
            x[0, 3] = 80.0                                # an outlier channel
            gamma = 1 + 0.1 * torch.randn(W, generator=g)
            beta = 0.1 * torch.randn(W, generator=g)
            ref, mean, rstd = ln64(x, gamma, beta)
            A = x.double().abs() + mean.abs()
            dev = x.double()
        else:
            c, a, s = _exact_rows(M, W, g, cls == "beta0")
            xd = c + a * s
            x = xd.float()
            assert torch.equal(x.double(), xd)
            gamma = (torch.exp2(torch.randint(-2, 3, (W,), generator=g).float()) * (torch.randint(0, 2, (W,), generator=g).float() * 2 - 1))
            beta = torch.zeros(W) if cls == "beta0" else (torch.randperm(W, generator=g).float() - W // 2) / 8
            ref, mean, rstd = ln64(x, gamma, beta)
            assert torch.equal(mean, c) and torch.equal(1.0 / torch.sqrt(a * a + EPS), rstd)      # mean and variance are exact
            A = (xd - mean).abs()
            dev = a * s
        unit = 2.0 ** -23 * (A * rstd * gamma.double().abs() + beta.double().abs())
        return dict(x=x, gamma=gamma, beta=beta, ref=ref, unit=unit, dev=dev, cls=cls)
    if cls == "beta0":                   # (equal columns cannot be avoided without beta: the rows are what the FP8 form can misplace)
        ok = lambda c: ge.count_distinct(c["ref"]) == M          # noqa: E731
    elif cls == "exact":
        ok = lambda c: _distinct_rows_ok(c["ref"], c["dev"], W)          # noqa: E731
    else:
        ok = lambda c: ge.is_distinct(c["ref"]) or (M == 1 and ge.count_distinct(c["ref"].t()) == W)      # noqa: E731
    return ge.redraw(make, M * 13 + W, ok)


def ln_restated(x, gamma, beta, exact=False):
    """layernorm_kernel (csrc/vit_kernels.hpp) restated in float32 numpy in the kernel's own order: lane l holds columns
    256 i + 4 l .. + 3 of group i < 4 (zeros beyond W), adds them left to right group by group, the wave adds over the xor butterfly
    32, 16 .. 1; mean = s / W; the same again for the squared deviations; rstd = 1 / sqrt(q / W + eps) correctly rounded;
    y = ((x - mean) rstd) gamma + beta. exact: assert that sum, mean, deviations and variance carry no rounding (the exact
    class). x, gamma, beta: torch f32 -> numpy f32 [M][W]."""
    f32 = np.float32
    x, gamma, beta = x.numpy(), gamma.numpy(), beta.numpy()
    M, W = x.shape
    lanes = np.arange(64)
    xp = np.zeros((M, 1024), f32)
    xp[:, :W] = x
    v = xp.reshape(M, 4, 64, 4)
    live = (np.arange(1024) < W).reshape(1, 4, 64, 4)[..., 0]

    def wave(t):
        for o in (32, 16, 8, 4, 2, 1):
            t = t + t[:, lanes ^ o]
        assert (t == t[:, :1]).all()
        return t[:, 0]

    s = np.zeros((M, 64), f32)
    for i in range(4):
        s = s + (((v[:, i, :, 0] + v[:, i, :, 1]) + v[:, i, :, 2]) + v[:, i, :, 3])
    s = wave(s)
    mean = s / f32(W)
    d = v - mean[:, None, None, None]
    q = np.zeros((M, 64), f32)
    for i in range(4):
        t = ((d[:, i, :, 0] * d[:, i, :, 0] + d[:, i, :, 1] * d[:, i, :, 1]) + d[:, i, :, 2] * d[:, i, :, 2]) + d[:, i, :, 3] * d[:, i, :, 3]
        q = q + np.where(live[:, i], t, f32(0))
    var = wave(q) / f32(W)
    assert s.dtype == f32 and mean.dtype == f32 and d.dtype == f32 and var.dtype == f32
    if exact:
        xd = x.astype(np.float64)
        m64 = xd.mean(1)
        assert (s == xd.sum(1)).all() and (mean == m64).all() and (var == ((xd - m64[:, None]) ** 2).mean(1)).all()
        assert (d.reshape(M, 1024)[:, :W] == xd - m64[:, None]).all()
    rstd = (1.0 / np.sqrt((var + f32(1e-5)).astype(f32).astype(np.float64))).astype(f32)
    y = (d.reshape(M, 1024)[:, :W] * rstd[:, None]) * gamma[None, :] + beta[None, :]
    assert y.dtype == f32
    return y


def ln_restated_ratio(c):
    """worst |restated - float64 reference| / unit of one case (unit = 0 only where the result is exactly 0: there the error must be too)"""
    y = ln_restated(c["x"], c["gamma"], c["beta"], exact=c["cls"] != "random").astype(np.float64)
    err, unit = np.abs(y - c["ref"].numpy()), c["unit"].numpy()
    assert (err[unit == 0] == 0).all()
    return float(np.max(err / np.where(unit == 0, 1.0, unit)))


def ln_class_ratio(cls):
    """the worst restated ratio over all cases of a class (the exact class includes its beta0 variants)"""
    worst = max(ln_restated_ratio(ln_case(cls, M, W)) for M in LN_M for W in LN_W)
    if cls == "exact":
        worst = max([worst] + [ln_restated_ratio(ln_case("beta0", M, W)) for M in LN_M for W in LN_W_256])
    return worst


def ln_forms(clipmi, M, W, w, b, x=None, x3=None, rowidx=None, row_step=1, out=None, out_bf16=0, out8=None, scale8=None, out_x3=None,
             out_part=None):
    """clipmi_dbg_layernorm_forms on device tensors (None = NULL) -> the return code"""
    p = lambda t: None if t is None else t.data_ptr()          # noqa: E731
    return clipmi._lib.lib().clipmi_dbg_layernorm_forms(p(x), p(x3), p(rowidx), row_step, p(w), p(b), p(out), out_bf16, p(out8), p(scale8),
                                                        p(out_x3), p(out_part), M, W, None)


def ln_dense(clipmi, gpu, x, gamma, beta, out_bf16, x3=None):
    """The dense form on device tensors -> [M][W] rows (NaN-filled before, the guard row checked)."""
    M = (x if x3 is None else x3).shape[0]
    W = gamma.numel()
    out = torch.full((M + 1, W), NAN, dtype=torch.bfloat16 if out_bf16 else torch.float32, device=gpu)
    clipmi._lib.check(ln_forms(clipmi, M, W, gamma, beta, x=x if x3 is None else None, x3=x3, out=out, out_bf16=out_bf16), "layernorm")
    torch.cuda.synchronize()
    assert torch.isnan(out[M]).all(), f"layernorm M={M} W={W}: wrote past row M"
    return out[:M]


def assert_ln_bound(got, c, out_bf16, what):
    """got [M][W] on any device against the case's float64 reference under the class's bound -> worst err / bound"""
    ref, unit = c["ref"], c["unit"]
    tol = C_OF[c["cls"]] * unit + (2.0 ** -8 * ref.abs() if out_bf16 else 0)
    err = (got.cpu().double() - ref).abs()
    bad = ~(err <= tol)                                    # (a NaN is bad)
    worst = (err / tol.clamp_min(1e-300)).nan_to_num(1e30).max().item()
    print(f"{what}: worst err / bound {worst:.3f}")
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.numel()} outside the bound, worst err / bound {worst}, " \
                          f"first at (row, column) {tuple(bad.nonzero()[0].tolist())}"
    return worst


def bits(t):
    """the bit patterns of a bf16 / f32 / u8 tensor, for equality that tells -0 from +0 and compares NaNs"""
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 1: torch.uint8}[t.element_size()])


# ---- split rows -------------------------------------------------------------------------------------------------------------------
def join(x3, W):
    """f32 values of split rows uint8 [M][3 W]: bits = (bits(hi) << 16) + (u << 8) - 0x8000  (csrc/gemm.hpp split_join)"""
    hi, lo = x3[:, :2 * W].contiguous().view(torch.int16), x3[:, 2 * W:]
    return ((hi.to(torch.int32) << 16) + (lo.to(torch.int32) << 8) - 0x8000).view(torch.float32)


def split_case_rows(cls, M, W):
    """split rows uint8 [M][3 W] on the CPU: hi = bf16 of the case's x, remainder bytes random (not all 128)"""
    g = torch.Generator(device="cpu"); g.manual_seed(M * 17 + W)
    x3 = torch.empty(M, 3 * W, dtype=torch.uint8)
    x3[:, :2 * W] = ln_case(cls, M, W)["x"].to(torch.bfloat16).view(torch.uint8)
    x3[:, 2 * W:] = torch.randint(0, 256, (M, W), generator=g).to(torch.uint8)
    assert (x3[:, 2 * W:] != 128).float().mean().item() > 0.9
    return x3


def nan_split_rows(R, W, gpu):
    """R split rows that must not be read: every hi half a bf16 NaN (0x7fc0), the remainder bytes GUARD_BYTE"""
    x3 = torch.full((R, 3 * W), GUARD_BYTE, dtype=torch.uint8, device=gpu)
    x3[:, :2 * W] = torch.tensor([0xc0, 0x7f], dtype=torch.uint8, device=gpu).repeat(W)
    return x3


# ---- the FP8 quantisers, restated in torch -----------------------------------------------------------------------------------------
def quant_rows(t):
    """the row quantiser (tests/test_fp8_gpu.py _quant_rows): scale = max |x| / 448 (1 for a row of zeros), RNE to e4m3 ->
    (uint8 e4m3 bytes, f32 scales)"""
    t = t.float()
    amax = t.abs().amax(dim=1)
    scale = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax))
    q = (t * (1.0 / scale)[:, None]).to(torch.float8_e4m3fn)
    return q.view(torch.uint8), scale


def quant_mx(t):
    """the MX rule (tests/test_fp8_gpu.py _quant_mx): 32 consecutive values share 2^(e - 7), e = floor(log2(block max)), a block
    of zeros takes 2^0 -> (uint8 e4m3 bytes [M][K], uint8 e8m0 scale bytes [M][K / 32])"""
    M, K = t.shape
    x = t.float().reshape(M, K // 32, 32)
    amax = x.abs().amax(-1)
    e_biased = ((amax.view(torch.int32) >> 23) & 0xff)
    sb = torch.where(amax == 0, torch.full_like(e_biased, 127), (e_biased - 7).clamp(min=0))
    inv = torch.ldexp(torch.ones_like(amax), 127 - sb)
    q = (x * inv[..., None]).to(torch.float8_e4m3fn).view(torch.uint8).reshape(M, K)
    return q, sb.to(torch.uint8)


def assert_e4m3_equal(got, want, what):
    """byte equality up to the sign of zero, e4m3's only representational freedom"""
    same = (got == want) | (((got & 0x7f) == 0) & ((want & 0x7f) == 0))
    assert same.all(), f"{what}: {int((~same).sum())} of {same.numel()} e4m3 bytes differ, first at {tuple((~same).nonzero()[0].tolist())}"
