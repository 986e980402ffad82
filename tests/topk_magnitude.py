"""Rows and queries of any magnitude for the search paths (no tests here: tests/test_topk_magnitude.py proves the inputs and
the restatements on the CPU, tests/test_topk_magnitude_gpu.py runs them on the device).

`scaled(case, a, b)` multiplies the rows of a tests/coarse_tight.py case by 2^a and its queries by 2^b. On the PLAIN grid every
f32 quantity of the keep tests scales exactly; on the EXTREME grid squares, scales or scores under- or overflow.

The norms of the superset bounds (||y||, ||f_q||, a_r) in two forms:
  legacy   f32 sums of squares, as coarse_prep_kernel and quantize_rows_i8_kernel computed them before this file existed: the
           square of a component below 2^-63 is subnormal or zero, the norm comes out too small or as 0, the margin is 0 and
           finite, and the keep test runs with no margin at all;
  current  what the kernels compute now (csrc/i8_layout.hpp norm_up, I8_TINY ..): f64 sums of squares, roots rounded UP to
           f32; a block of rows below 2^-110 keeps scale 1 and zero codes; a query or database outside the range the f32
           arithmetic of the bound is proved for has no coarse bound - margin +inf, the exact fallback answers.
tests/coarse_tight.py (I8Copy, I8Queries, bf16_margin) computes its norms through one of these; there is no other copy.

ROUTE is the literal table of what `current` must do at every grid point: "coarse" - a finite margin for every query, and every
row of the oracle's top K passes - or "none" - margin +inf for every query."""
import numpy as np

f32 = np.float32
I8_TINY, BF16_TINY, COARSE_HUGE, COARSE_HUGE_RY = f32(2.0 ** -110), f32(2.0 ** -90), f32(2.0 ** 110), f32(2.0 ** 120)
FLT_MIN = f32(2.0 ** -126)

PLAIN = ((-40, 0), (0, -40), (40, 40), (-40, 40), (40, -40))
EXTREME = ((0, -64), (0, -70), (0, -75), (0, -90), (-64, 0), (-70, 0), (-90, 0), (-60, -60), (-75, -75), (-126, 60),
           (0, 64), (64, 0), (64, 64), (100, 0))
GRID = PLAIN + EXTREME
E768_POINTS = ((-40, 40), (0, -75), (-75, 0))             # what the device test runs at E = 768; (-75, 0) is on neither grid
EVERY_POINT = GRID + ((-75, 0),)
ROW_EXPONENTS = sorted({a for a, _ in GRID})

# Where the coarse bound is used (family R / Q: both int8 passes; B: bf16). Derived by hand from the thresholds above and the
# families' magnitudes (R: |q| in 2^-3 .. 1, R_max ~ 2^-4; Q: largest |q| 2^-4 .. 2^-1, R_max ~ 2^-1; B: largest |q| 2^-8 .. 2^-5,
# R_max ~ 2^-0.5; ||y|| <= sqrt(E) largest |q|), asserted - not discovered - by tests/test_topk_magnitude.py:
#   (-60, -60), (-75, -75), (-126, 60): R_max ||y|| < 2^-110 (scores at or under the subnormal grid);  (64, 64): R_max ||y|| > 2^120
#   (scores overflow);  bf16 at 2^-90 on either side: largest |q| or R_max under 2^-90.
_NONE_ALL = {(-60, -60), (-75, -75), (-126, 60), (64, 64)}
ROUTE = {(fam, pt): "none" if pt in _NONE_ALL or (fam == "B" and pt in ((0, -90), (-90, 0))) else "coarse"
         for fam in "RQB" for pt in EVERY_POINT}
# Build side (tests/test_topk_magnitude_gpu.py, unit rows x U[0.1, 3] x 2^a): "bounds" - every a_r, block maximum and rmax is
# an upper bound of the f64 norm -, or "exact" - search_device's guard leaves the coarse path. The bounds hold at every
# exponent (2^-126: subnormal rows, stored as zero codes with a_r = ||x||); rmax overflows nowhere on the grid.
BUILD_SIDE = {a: "bounds" for a in ROW_EXPONENTS}

# The legacy form drops a row of the true top K: for every query ("all") or for at least one ("some") - the table of the issue
# that asked for this file (E = 512, N = 70 001), measured there on the CPU. (family, scaled operand) -> {exponent: claim}
LEGACY_DROPS = {("Q", "queries"): {-64: "some", -70: "all", -75: "all", -90: "all"},
                ("R", "queries"): {-75: "all", -90: "all"},
                ("R", "rows"): {-64: "all", -70: "all"},
                ("B", "queries"): {-75: "all", -90: "all"}}


class Scaled:
    pass


def scaled(case, a, b):
    """The case with db * 2^a and q * 2^b (f32 products); fences, targets and the rest unchanged."""
    c = Scaled()
    c.__dict__.update(case.__dict__)
    c.db = (case.db * f32(2.0 ** a)).astype(f32)
    c.q = (case.q * f32(2.0 ** b)).astype(f32)
    c.a, c.b = a, b
    return c


def up32(x):
    """f64 -> f32, rounded up (csrc/i8_layout.hpp norm_up after the root)."""
    x = np.asarray(x, np.float64)
    with np.errstate(over="ignore"):
        f = x.astype(f32)
    return np.where(f.astype(np.float64) < x, np.nextafter(f, f32(np.inf)), f).astype(f32)


def digits(x, inv):
    """rint(x * inv) clamped to [-127, 127] as the kernels' fminf(fmaxf(.., -127), 127) does it: a NaN (0 * inf) becomes -127."""
    with np.errstate(over="ignore", invalid="ignore"):
        r = np.rint(x * inv)
    return np.where(np.isnan(r), f32(-127), np.clip(r, -127, 127)).astype(f32)


class Legacy:
    name = "legacy"

    @staticmethod
    def block_scale(mx):
        s = (mx / f32(127.0)).astype(f32)
        s[mx == 0] = 1.0
        return s

    @staticmethod
    def err_norm(xp, sr, q8):
        return (np.linalg.norm(xp - sr[:, None] * q8, axis=1).astype(f32) * f32(1.001)).astype(f32)

    @staticmethod
    def query_norms(q, t, p):
        """(||y||, 1.001 ||f_q|| - None without digits)"""
        Y = np.linalg.norm(q, axis=1).astype(f32)
        if p is None:
            return Y, None
        return Y, (np.linalg.norm(q - t[:, None] * p, axis=1).astype(f32) * f32(1.001)).astype(f32)

    @staticmethod
    def in_range(mx, Y, rmax, i8):
        return np.ones(mx.shape, bool)


class Current:
    name = "current"

    @staticmethod
    def block_scale(mx):
        s = (mx / f32(127.0)).astype(f32)
        s[mx < I8_TINY] = 1.0
        return s

    @staticmethod
    def err_norm(xp, sr, q8):
        e = xp.astype(np.float64) - sr.astype(np.float64)[:, None] * q8.astype(np.float64)
        return (up32(np.sqrt((e * e).sum(axis=1))) * f32(1.001)).astype(f32)

    @staticmethod
    def query_norms(q, t, p):
        q64 = q.astype(np.float64)
        Y = up32(np.sqrt((q64 * q64).sum(axis=1)))
        if p is None:
            return Y, None
        f = q64 - t.astype(np.float64)[:, None] * p.astype(np.float64)
        return Y, (up32(np.sqrt((f * f).sum(axis=1))) * f32(1.001)).astype(f32)

    @staticmethod
    def in_range(mx, Y, rmax, i8):
        """coarse_prep_kernel's in_range, in f32."""
        tiny = I8_TINY if i8 else BF16_TINY
        rmax = f32(rmax)
        with np.errstate(over="ignore", under="ignore"):
            RY = (rmax * Y).astype(f32)
        return (mx >= tiny) & (mx <= COARSE_HUGE) & bool(rmax >= tiny) & bool(rmax <= COARSE_HUGE) & (RY >= tiny) & (RY <= COARSE_HUGE_RY)


legacy, current = Legacy, Current
