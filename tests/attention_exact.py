"""Exact data, float64 references and float32 models for the attention kernels (helper of tests/test_attention_exact.py and
tests/test_attention_exact_gpu.py; no test in here).

Layout as the kernels take it: qkv bf16 [B L][3 W], W = 64 heads, head h at columns 64 h .. 64 h + 63 of each third.

EXACT CLASSES. K rows are A * code(j + 31 item) (item = b heads + h, so that a neighbouring head's K is another set of codes),
code(.) in {-1, +1}^64 with any two differing in >= 6 of their first 62 places, A = 10; V holds integers in [-16, 16] drawn per
(b, h, key). A query A * code(p) scores 800 against key p and <= 650 against every other key: after the softmax's
max-subtraction every other exponential is exp(<= -128) = 2^(<= -184), which is 0 in f32, so P is exactly one-hot and the output
row is V[p]. Classes that need them overwrite the two reserved places 62, 63 of Q and K (the winner then scores 775, the others
<= 625). Each class states its winners as a 0/1 array; winners_case() asserts from the float64 scores alone that the winners of
a row tie exactly and beat every other valid key by >= MARGIN, and the expected row is the mean of the winners' V rows:
    selection   Q[q] = A code(pi(q)); unmasked pi is a permutation per item with 0 -> L - 1 and L - 1 -> 0; causal pi(q) = q,
                0 or q // 2
    trap        causal, pi(q) = q, place 63 of K[j] = j and of Q = 16384 (2048 j on the score): every FUTURE key outscores the
                diagonal (by >= 2048 - 2 * 775) while the diagonal still wins among the allowed keys
    ties        K[kb] = K[ka] (the one pair of equal codes), Q = A code(ka): P = 1/2, 1/2, out = (V[ka] + V[kb]) / 2
    ramps       (long sequences) K[j] places 62, 63 = (j // 32, j % 32), Q = g (32, 1) there and 0 elsewhere, |g| >= 1024: the score
                is g j / 8, adjacent keys >= 128 apart. Up: the maximum moves in every block (alpha = 0), out = V[L - 1]; down: it
                rests at key 0 (alpha = 1), out = V[0]. The flash kernel keeps its maximum as the ROUNDED product m = f32(s c) and
                takes e = exp2(fma(s, c, -m)): for the winner that is 2^(the product's rounding error), up to 1 +- 0.0027 at
                s c = 10^5, which need not round to a bf16 P of 1. g is therefore the first of 1024, 1088, ... for which
                |2^error - 1| <= 2^-10 at the last key (ramp_case): P = 1 and v / l rounds back to v for every |v| <= 16
    uniform     Q = 0: every score 0, P = 1 / n; the expected rows follow the kernels' two roundings (uniform_expected)
Every product and partial sum of these classes is an integer (or an integer times one bf16 factor) below 2^24: exact in f32 in any
order. The references are float64 on the CPU and never one of the project's kernels; the float32 models restate the kernels'
documented rounding points (P rounded to bf16, f32 accumulation, bf16 output) and serve the CPU test only.

RANDOM DATA is held per element to   |got - o| <= 2^-8 (|o| + pav) (1 + 2^-6),   pav = softmax(s) |v|   (bound64)."""
import functools

import numpy as np
import torch

A = 10.0
VMAX = 16
MARGIN = 128.0
NAN = float("nan")
GUARD_ROWS = 3
GUARD_BYTE = 0xA5
NCODES = 640
RESIDENT_52X4 = 256 * 5          # attention52x4_kernel's grid limit: NUM_CU * 5 workgroups
TRAP_Q = 16384.0
RAMP_G = 1024.0
LOG2E_8 = float(np.float32(0.125) * np.float32(1.4426950408889634))    # the flash kernel's c


def gen(seed):
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    return g


@functools.lru_cache(maxsize=1)
def codes():
    """[NCODES][64] in {-1, +1}, float64; any two differ in at least 6 of the first 62 places"""
    c = torch.randint(0, 2, (NCODES, 64), generator=gen(64)).double() * 2 - 1
    d = (62 - c[:, :62] @ c[:, :62].t()) / 2
    d.fill_diagonal_(64)
    assert d.min().item() >= 6, d.min().item()
    return c


def key_codes(B, L, heads):
    """code index of key j of item (b, h): [B][L][heads]"""
    item = torch.arange(B)[:, None, None] * heads + torch.arange(heads)[None, None, :]
    return (torch.arange(L)[None, :, None] + 31 * item) % NCODES


def draw_v(B, L, heads, g):
    return torch.randint(-VMAX, VMAX + 1, (B, L, heads, 64), generator=g).double()


def assemble(q, k, v):
    """q, k, v float64 [B][L][heads][64] -> qkv bf16 [B L][3 W]; every value must be one bf16 holds"""
    B, L, H, _ = q.shape
    x = torch.stack([q, k, v], dim=2).reshape(B * L, 3 * H * 64)
    b = x.to(torch.bfloat16)
    assert torch.equal(b.double(), x), "the data is not exact in bf16"
    return b


def split64(qkv, B, L, heads):
    """qkv [B L][3 W] -> q, k, v float64 [B][heads][L][64]"""
    x = qkv.double().reshape(B, L, 3, heads, 64)
    return [x[:, :, i].permute(0, 2, 1, 3).contiguous() for i in range(3)]


def valid_mask(L, causal):
    """[L][L] bool: key (column) valid for query (row)"""
    m = torch.ones(L, L, dtype=torch.bool)
    return m.tril() if causal else m


def scores64(qkv, B, L, heads):
    q, k, _ = split64(qkv, B, L, heads)
    return q @ k.transpose(-1, -2) * 0.125                  # [B][heads][L][L], unmasked


def rows_of(x):
    """[B][heads][L][64] -> [B L][W]"""
    B, H, L, _ = x.shape
    return x.permute(0, 2, 1, 3).reshape(B * L, H * 64)


def attention64(qkv, B, L, heads, causal):
    """float64 reference -> (o, pav) [B L][W]: softmax(q k^T / 8 (+ mask)) v, and the same weights applied to |v|"""
    q, k, v = split64(qkv, B, L, heads)
    s = q @ k.transpose(-1, -2) * 0.125
    if causal:
        s = s.masked_fill(~valid_mask(L, True), float("-inf"))
    p = torch.softmax(s, -1)
    return rows_of(p @ v), rows_of(p @ v.abs())


def bound64(o, pav):
    return 2.0 ** -8 * (o.abs() + pav) * (1 + 2.0 ** -6)


# ---- the exact classes ----------------------------------------------------------------------------------------------------------
def permutations(B, L, heads, g):
    """pi [B][heads][L]: a permutation per item with 0 -> L - 1 and L - 1 -> 0, no two items' alike (L >= 4)"""
    pis = []
    for _ in range(B * heads):
        for _ in range(64):
            pi = torch.cat([torch.tensor([L - 1]), torch.randperm(max(L - 2, 0), generator=g) + 1, torch.tensor([0])])[:L]
            if not any(torch.equal(pi, p) for p in pis):
                break
        pis.append(pi)
    return torch.stack(pis).reshape(B, heads, L)


def one_hot_winners(pi, L):
    """pi [B][heads][L] -> 0/1 [B][heads][L][L]"""
    return torch.nn.functional.one_hot(pi, L).bool()


def winners_case(q, k, v, win, causal, what, future_wins=False):
    """The conditions of a class whose P is exactly 0 / 1 / n on its winners, from the float64 scores alone; -> the case.
    win: bool [B][heads][L][L]"""
    B, L, H, _ = q.shape
    qkv = assemble(q, k, v)
    s = scores64(qkv, B, L, H)
    ok = valid_mask(L, causal)
    assert (win & ~ok).sum().item() == 0 and (win.sum(-1) >= 1).all(), f"{what}: a row without an allowed winner"
    hi = s.masked_fill(~win, float("inf")).amin(-1)
    lo = s.masked_fill(~win, float("-inf")).amax(-1)
    assert torch.equal(hi, lo), f"{what}: a row's winners do not tie"
    rest = s.masked_fill(win | ~ok, float("-inf")).amax(-1)
    margin = (hi - rest).min().item()
    assert margin >= MARGIN, f"{what}: margin {margin}"
    assert s.abs().max().item() * 8 < 2 ** 24, f"{what}: a score is no exact f32 integer"
    if future_wins:             # the mask alone keeps the strongest key out: all rows but the last
        fut = s.masked_fill(ok, float("-inf")).amax(-1)[..., :-1]
        assert (fut > hi[..., :-1]).all(), f"{what}: a future key does not outscore the winner"
    vv = split64(qkv, B, L, H)[2]
    w = win.double()
    expect = rows_of((w @ vv) / w.sum(-1, keepdim=True))
    eb = expect.to(torch.bfloat16)
    assert torch.equal(eb.double(), expect), f"{what}: the expected rows are not exact in bf16"
    return dict(qkv=qkv, expect=eb, B=B, L=L, heads=H, causal=causal, what=what, margin=margin)


def count_distinct(x):
    return torch.unique(x, dim=0).shape[0]


def assert_distinct_rows(c):
    """the expected output has B L distinct rows, and no head's 64-column slice of a row equals another (row, head)'s"""
    e = c["expect"].double()
    n = e.shape[0]
    assert count_distinct(e) == n, f"{c['what']}: {count_distinct(e)} distinct rows of {n}"
    sl = e.reshape(n * c["heads"], 64)
    assert count_distinct(sl) == sl.shape[0], f"{c['what']}: equal 64-column slices"


def base_qk(B, L, heads):
    kc = key_codes(B, L, heads)                     # [B][L][heads]
    return kc, A * codes()[kc]                      # k [B][L][heads][64]


@functools.lru_cache(maxsize=4)
def selection_case(B, L, heads, causal, mode):
    """mode: 'perm' (unmasked), 'diag', 'zero', 'half', 'trap' (causal)"""
    what = f"selection {mode} B={B} L={L} heads={heads} causal={causal}"
    assert (mode == "perm") == (not causal)
    g = gen(L * 1009 + B * 31 + heads + causal)
    kc, k = base_qk(B, L, heads)
    v = draw_v(B, L, heads, g)
    if mode == "perm":
        pi = permutations(B, L, heads, g)
        flat = pi.reshape(B * heads, L)
        assert (flat[:, 0] == L - 1).all() and (flat[:, -1] == 0).all() and (flat.sort(-1).values == torch.arange(L)).all()
        assert L < 8 or count_distinct(flat) == B * heads, f"{what}: two items share a permutation"       # (L - 2)! >= 720
    else:
        ar = torch.arange(L)
        pi = {"diag": ar, "trap": ar, "zero": ar * 0, "half": ar // 2}[mode].expand(B, heads, L)
    # Q[b][q][h] = A code(code index of key pi(q) of item (b, h))
    qc = torch.gather(kc.permute(0, 2, 1), 2, pi)                       # [B][heads][L]
    q = (A * codes()[qc]).permute(0, 2, 1, 3).contiguous()              # [B][L][heads][64]
    if mode == "trap":
        k = k.clone()
        q[..., 62], k[..., 62] = 0.0, 0.0
        q[..., 63] = TRAP_Q
        k[..., 63] = torch.arange(L).double()[None, :, None]
    c = winners_case(q, k, v, one_hot_winners(pi, L), causal, what, future_wins=(mode == "trap" and L > 1))
    if mode in ("perm", "diag", "trap"):
        assert_distinct_rows(c)
    return c


def tie_pairs(L, flash):
    """(ka, kb) pairs: different 16-key tiles and 32-key steps where L allows; flash: block 0 and the last (masked) block"""
    if flash:
        last = (L - 1) // 64 * 64
        return [(0, L - 1), (63, last), (17, L - 1), (40, last)]
    if L >= 33:
        return [(0, L - 1), (31, 32), (5, 32 + (L - 33) // 2), (16, L - 1)]
    if L >= 17:
        return [(0, L - 1), (15, 16), (3, 16 + (L - 17) // 2)]
    return [(0, L - 1), (0, 1), ((L - 1) // 2, L - 1)]


@functools.lru_cache(maxsize=4)
def ties_case(B, L, heads):
    assert L >= 2
    what = f"ties B={B} L={L} heads={heads}"
    g = gen(L * 2003 + B * 31 + heads)
    kc, _ = base_qk(B, L, heads)
    pairs = tie_pairs(L, L > 80)
    kc = kc.clone()
    qc = torch.zeros(B, L, heads, dtype=torch.long)
    win = torch.zeros(B, heads, L, L, dtype=torch.bool)
    for b in range(B):
        for h in range(heads):
            ka, kb = pairs[(b * heads + h) % len(pairs)]
            assert ka != kb and (ka // 16 != kb // 16 or L <= 16) and (ka // 32 != kb // 32 or L <= 32)
            kc[b, kb, h] = kc[b, ka, h]
            qc[b, :, h] = kc[b, ka, h]
            win[b, h, :, ka] = True
            win[b, h, :, kb] = True
    v = draw_v(B, L, heads, g)
    c = winners_case(A * codes()[qc], A * codes()[kc], v, win, 0, what)
    assert (c["expect"].double() * 2 % 2 != 0).any(), f"{what}: no odd sum: the halves are never seen"
    return c


RAMP_TILES = "tile 0: up and down rows alternate (a mixed wave for the alpha skip); tile 1: down only; then up only, mixed, ..."


def ramp_directions(L):
    """+1 (up) / -1 (down) per query: 16-query tile 0 alternates, tile 1 is all down, tile 2 all up, tile 3 alternates, ..."""
    qi = torch.arange(L)
    t = (qi // 16) % 4
    alt = torch.where(qi % 2 == 0, 1, -1)
    return torch.where(t == 1, -1, torch.where(t == 2, 1, alt))


@functools.lru_cache(maxsize=4)
def ramp_case(B, L, heads):
    what = f"ramps B={B} L={L} heads={heads}"
    g = gen(L * 3001 + B * 31 + heads)
    _, k = base_qk(B, L, heads)
    k = k.clone()
    j = torch.arange(L)
    k[..., 62] = (j // 32).double()[None, :, None]
    k[..., 63] = (j % 32).double()[None, :, None]
    d = ramp_directions(L).double()
    for step in range(16):
        gain = RAMP_G + 64 * step
        sc = np.float64(gain * (L - 1)) * np.float64(np.float32(LOG2E_8))
        if abs(2.0 ** float(sc - np.float64(np.float32(sc))) - 1) <= 2.0 ** -10:
            break
    else:
        raise AssertionError(f"{what}: no gain keeps the winner's exponential within 2^-10 of 1")
    q = torch.zeros(B, L, heads, 64, dtype=torch.float64)
    q[..., 62] = (32 * gain * d)[None, :, None]
    q[..., 63] = (gain * d)[None, :, None]
    pi = torch.where(d > 0, L - 1, 0).long().expand(B, heads, L)
    c = winners_case(q, k, draw_v(B, L, heads, g), one_hot_winners(pi, L), 0, what)
    c["directions"], c["gain"] = d, gain
    return c


def bf16r(x):
    """float32 tensor -> rounded to bf16 (nearest even), as float32"""
    return x.to(torch.bfloat16).float()


def uniform_expected(vsum, n, flash):
    """vsum float64 (exact integers), n int64 (broadcastable) -> the kernels' rows as float32 values of bf16:
    short kernels  bf16( bf16(f32(1 / n)) * sum V )     (P = 1 / n is rounded to bf16, the products and their sum are exact)
    flash kernel   bf16( f32( f32(sum V) * f32(1 / n) ) )"""
    inv = torch.ones((), dtype=torch.float32) / n.float()           # IEEE division: correctly rounded
    assert vsum.abs().max().item() < 2 ** 24 / 256                  # 8 bits of P on top of the sum stay within 24
    if flash:
        return bf16r(vsum.float() * inv)
    p = bf16r(inv).double()
    prod = p * vsum
    assert torch.equal(prod.float().double(), prod)                 # exact in f32
    return bf16r(prod.float())


@functools.lru_cache(maxsize=4)
def uniform_case(B, L, heads, causal):
    what = f"uniform B={B} L={L} heads={heads} causal={causal}"
    g = gen(L * 4001 + B * 31 + heads + causal)
    _, k = base_qk(B, L, heads)
    v = draw_v(B, L, heads, g)
    qkv = assemble(torch.zeros_like(k), k, v)
    assert scores64(qkv, B, L, heads).abs().max().item() == 0
    vv = split64(qkv, B, L, heads)[2]                               # [B][heads][L][64]
    if causal:
        vsum, n = vv.cumsum(2), (torch.arange(L) + 1)[None, None, :, None]
    else:
        vsum, n = vv.sum(2, keepdim=True).expand(B, heads, L, 64), torch.full((1, 1, L, 1), L)
    expect = rows_of(uniform_expected(vsum, n, L > 80)).to(torch.bfloat16)
    c = dict(qkv=qkv, expect=expect, B=B, L=L, heads=heads, causal=causal, what=what)
    o64 = attention64(qkv, B, L, heads, causal)[0]
    assert ((expect.double() - o64).abs() <= 2.0 ** -6 * o64.abs() + 1e-12).all(), f"{what}: the expected rows are not the mean"    # two bf16 roundings
    if causal:
        assert count_distinct(expect.double()) == B * L, f"{what}: causal rows are not all distinct"
    return c


@functools.lru_cache(maxsize=2)
def single_key_case(B, heads):
    """L = 1, any data: out == V"""
    g = gen(B * 31 + heads)
    qkv = (torch.randn(B, 3 * heads * 64, generator=g) * 3).to(torch.bfloat16)
    return dict(qkv=qkv, expect=qkv[:, 2 * heads * 64:].contiguous(), B=B, L=1, heads=heads, causal=0, what=f"L=1 B={B} heads={heads}")


# ---- random data ------------------------------------------------------------------------------------------------------------------
SHORT_RANDOM = [(3, 50, 12, 0), (2, 77, 8, 1), (5, 5, 2, 0), (4, 16, 2, 1), (1, 64, 12, 0), (2, 80, 8, 1), (7, 33, 3, 0), (257, 50, 12, 0)]
LONG_RANDOM = [(2, 197, 12), (1, 257, 16), (2, 577, 16), (3, 81, 2), (1, 128, 1), (1, 129, 3)]
SCALES = ["0.25", "1.5", "4", "outliers"]


@functools.lru_cache(maxsize=2)
def random_case(B, L, heads, causal, scale):
    """test_attention's (L <= 80: seed B 100 + L) and test_attention_long_sequences' (seed B 1000 + L) inputs at a scale of
    0.25, 1.5 or 4, or at 1.5 with a few outlier rows times 6 (a sharp query, a loud key, a loud value row) -> the case with its
    float64 reference o and bound."""
    W = heads * 64
    x = torch.randn(B * L, 3 * W, generator=gen(B * 1000 + L if L > 80 else B * 100 + L))
    qkv = (x * (1.5 if scale == "outliers" else float(scale))).to(torch.bfloat16)
    if scale == "outliers":
        qkv[3 % (B * L), :64] *= 6.0
        qkv[(B * L) // 2, W:W + 64] *= 6.0
        qkv[B * L - 1, 2 * W:] *= 6.0
    o, pav = attention64(qkv, B, L, heads, causal)
    return dict(qkv=qkv, o=o, bound=bound64(o, pav), B=B, L=L, heads=heads, causal=causal,
                what=f"random x {scale} B={B} L={L} heads={heads} causal={causal}")


def worst_ratio(got, c):
    """got [B L][W] -> (largest |got - o| / bound, elements outside the bound); a NaN is outside"""
    err = (got.double().cpu() - c["o"]).abs()
    ratio = (err / c["bound"].clamp_min(1e-300)).nan_to_num(float("inf"))
    return ratio.max().item(), int((~(err <= c["bound"])).sum().item())


# ---- float32 models of the kernels (CPU) ----------------------------------------------------------------------------------------
def _to_bf16(x, truncate):
    if truncate:
        return (x.contiguous().view(torch.int32) & -65536).view(torch.float32)
    return bf16r(x)


def model_short(qkv, B, L, heads, causal, truncate=False):
    """attention_kernel / attention52*_kernel in float32: scores, * 1/8, mask, max, exp, sum, 1 / sum, P to bf16, P V in f32,
    bf16 rows. truncate: P is cut to bf16 instead of rounded (the model the bound must reject)."""
    q, k, v = [t.float() for t in split64(qkv, B, L, heads)]
    x = (q @ k.transpose(-1, -2)) * 0.125
    if causal:
        x = x.masked_fill(~valid_mask(L, True), float("-inf"))
    e = torch.exp(x - x.amax(-1, keepdim=True))
    inv = 1.0 / e.sum(-1, keepdim=True)
    p = _to_bf16(e * inv, truncate)
    return rows_of(p @ v).to(torch.bfloat16)


def model_flash(qkv, B, L, heads, truncate=False):
    """attention_flash_kernel in float32: 64-key blocks, running maximum in the exp2 domain, unnormalised P to bf16, the
    accumulator rescaled by alpha, 1 / l at the end."""
    q, k, v = [t.float() for t in split64(qkv, B, L, heads)]
    s = q @ k.transpose(-1, -2)
    c = torch.tensor(LOG2E_8, dtype=torch.float32)
    m = torch.full(s.shape[:-1] + (1,), float("-inf"))
    l = torch.zeros_like(m)
    o = torch.zeros(s.shape[:-1] + (64,))
    for k0 in range(0, L, 64):
        sb = s[..., k0:k0 + 64]
        m_new = torch.maximum(m, sb.amax(-1, keepdim=True) * c)
        alpha = torch.exp2(m - m_new)
        e = torch.exp2((sb.double() * c.double() - m_new.double()).float())          # one fma
        l = l * alpha + e.sum(-1, keepdim=True)
        o = o * alpha + _to_bf16(e, truncate) @ v[..., k0:k0 + 64, :]
        m = m_new
    return rows_of(o * (1.0 / l)).to(torch.bfloat16)


def model(qkv, B, L, heads, causal, truncate=False):
    return model_flash(qkv, B, L, heads, truncate) if L > 80 else model_short(qkv, B, L, heads, causal, truncate)


# ---- running a case on the GPU ------------------------------------------------------------------------------------------------------
def guarded(rows, width, dtype, gpu, fill):
    """[rows + GUARD_ROWS][width] on the device: `fill` in the rows, GUARD_BYTE in every byte of the guard rows"""
    t = torch.full((rows + GUARD_ROWS, width), fill, dtype=dtype, device=gpu)
    t[rows:].view(torch.uint8).fill_(GUARD_BYTE)
    return t


def guards_intact(t, rows):
    return bool((t[rows:].view(torch.uint8) == GUARD_BYTE).all().item())


def run_attention(clipmi, gpu, c, flags):
    """clipmi_dbg_attention on the case's qkv into a NaN-filled, guarded buffer -> the B L rows (device), finite, guards intact"""
    B, L, H = c["B"], c["L"], c["heads"]
    what = f"{c['what']} flags={flags}"
    out = guarded(B * L, H * 64, torch.bfloat16, gpu, NAN)
    qd = c["qkv"].to(gpu)
    clipmi._lib.check(clipmi._lib.lib().clipmi_dbg_attention(qd.data_ptr(), out.data_ptr(), B, L, H, flags, None), what)
    torch.cuda.synchronize()
    assert guards_intact(out, B * L), f"{what}: wrote past row B L"
    assert torch.isfinite(out[:B * L].float()).all(), f"{what}: rows left unwritten or not finite"
    return out[:B * L]


def assert_same_bytes(got, want, what):
    """bf16 (or uint8) tensors, byte for byte"""
    got, want = got.cpu().contiguous(), want.cpu().contiguous()
    assert got.shape == want.shape and got.dtype == want.dtype, what
    gi, wi = (got.view(torch.int16), want.view(torch.int16)) if got.dtype == torch.bfloat16 else (got, want)
    bad = gi != wi
    nbad = int(bad.sum().item())
    if nbad:
        r, col = bad.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {nbad} of {bad.numel()} differ in {int(bad.any(1).sum().item())} rows, first at (row, column) "
                             f"({r}, {col}): got {got[r, col].item()!r}, want {want[r, col].item()!r}")


def check_exact(clipmi, gpu, c, flags):
    got = run_attention(clipmi, gpu, c, flags | c["causal"])
    assert_same_bytes(got, c["expect"], f"{c['what']} flags={flags | c['causal']}")


# ---- the case lists -----------------------------------------------------------------------------------------------------------------
SHORT_SHAPES = {1: (3, 1), 5: (1, 3), 15: (5, 1), 16: (7, 3), 17: (1, 1), 31: (3, 2), 32: (1, 12), 33: (5, 1), 48: (1, 3), 53: (7, 3),
                64: (1, 1), 65: (3, 1), 77: (5, 2), 79: (1, 3), 80: (21, 1)}                    # L -> (B, heads)
FENCE_SHAPES = {49: (1, 1), 50: (7, 3), 51: (3, 2), 52: (1, 3)}
FLASH_SHAPES = {81: (1, 1), 96: (3, 1), 127: (1, 3), 128: (5, 1), 129: (1, 2), 192: (1, 1), 197: (1, 12), 257: (7, 3), 577: (1, 3)}
MANY_ITEMS = (129, 50, 10)                                                                     # 1290 items > RESIDENT_52X4


def exact_shapes():
    """(B, L, heads, causal, flags to run) of the exact classes - the smallest shapes that reach every instantiation and edge:
    * attention_kernel<NT, causal, TR>, L in SHORT_SHAPES, each with and without the mask, flags 0 (transposed V reads) and 2
      (2-byte reads): NT = 1 at L = 1, 5, 15, 16 (below, one below and at the tile), NT = 2 at 17, 31, 32 (one key step whose second
      tile is partly, then wholly valid), NT = 4 at 33, 48 (three tiles on the NT = 4 instantiation: a wholly masked key tile), 53
      (one past the ViT-B/32 fence: the generic kernel) and 64, NT = 5 at 65 (the odd last step whose second P half is zero), 77,
      79, 80 (the last L of the short kernels).
    * the ViT-B/32 fence L = 49 .. 52 unmasked on attention52x4_kernel<false> (flags 0), attention52_kernel (4) and
      attention_kernel<4, false, false> (2); L = 50 and 52 causal leave the fence for attention_kernel<4, true, .>.
    * MANY_ITEMS: 1290 (image, head) items against the 1280 resident workgroups of attention52x4_kernel: its item loop, the
      prefetch of the next item and the last-item exit run (ten workgroups take a second item).
    * attention_flash_kernel, L in FLASH_SHAPES: one past the short kernels (81: two blocks, the last masked to 17 keys), 96, 127
      (63 keys in the last block), 128 (a whole last block), 129 (1 key), 192 (whole), 197 (5 keys), 257 (1 key), 577 (1 key, ten
      blocks); the last workgroup has idle waves at every L but 127 and 128 (81, 96: three of four waves work; 129, 257: one).
    * B heads in {1, 3, 5, 21} (never a multiple of a workgroup's four waves) and 6, 10, 12; heads in {1, 2, 3, 12}: heads = 1 is the
      row stride of three heads' widths, heads = 12 the towers' own."""
    out = []
    for L, (B, h) in SHORT_SHAPES.items():
        out += [(B, L, h, 0, (0, 2)), (B, L, h, 1, (0, 2))]
    for L, (B, h) in FENCE_SHAPES.items():
        out.append((B, L, h, 0, (0, 4, 2)))
    out.append((1, 50, 12, 0, (0, 4, 2)))
    out += [(1, 52, 3, 1, (0, 2)), (1, 50, 3, 1, (0, 2))]
    out.append(MANY_ITEMS + (0, (0,)))
    for L, (B, h) in FLASH_SHAPES.items():
        out.append((B, L, h, 0, (0,)))
    return out


def instantiation(L, causal, flags):
    """the kernel launch_attention picks (csrc/vit_kernels.hip), by name"""
    if L > 80:
        return "flash"
    if 49 <= L <= 52 and not causal and not flags & 2:
        return "attention52" if flags & 4 else "attention52x4"
    nt = next(n for n in (1, 2, 4, 5) if (L + 15) // 16 <= n)
    return f"attention<{nt},{int(bool(causal))},{int(not flags & 2)}>"


ALL_INSTANTIATIONS = {f"attention<{nt},{c},{tr}>" for nt in (1, 2, 4, 5) for c in (0, 1) for tr in (0, 1)} | {"attention52", "attention52x4", "flash"}


def case_id(s):
    return "B%d-L%d-h%d-c%d" % s[:4]


def classes_of(B, L, heads, causal):
    """the exact classes a shape runs: (name, builder of the case)"""
    if causal:
        modes = ["diag", "zero", "half", "trap"]
        cl = [(m, functools.partial(selection_case, B, L, heads, 1, m)) for m in modes]
    else:
        cl = [("perm", functools.partial(selection_case, B, L, heads, 0, "perm"))]
        if L >= 2:
            cl.append(("ties", functools.partial(ties_case, B, L, heads)))
        if L == 1:
            cl.append(("single", functools.partial(single_key_case, B, heads)))
        if L > 80:
            cl.append(("ramps", functools.partial(ramp_case, B, L, heads)))
    cl.append(("uniform", functools.partial(uniform_case, B, L, heads, causal)))
    return cl


def exact_params():
    """[(id, class name, builder, flags)] over exact_shapes() x classes_of()"""
    return [(f"{name}-{case_id(s)}", name, build, s[4]) for s in exact_shapes() for name, build in classes_of(*s[:4])]
