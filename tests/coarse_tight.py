"""Adversarial inputs for the two coarse search paths and numpy restatements of their keep tests (no tests here:
tests/test_coarse_tight.py proves the inputs on the CPU, tests/test_coarse_tight_gpu.py runs them on the device,
tests/test_coarse_survivors_gpu.py holds the hooks' survivor counts to the restatements' bands).

The scans may drop a (query, row) pair only if the row provably cannot reach the running K-th best tau:
  int8:  s_r t_q D + 1.001 a_r ||y||  >=  tau - 1.001 (R_max + A_max) 1.001 ||f_q|| - c(E) R_max ||y||      (both sides / t_q)
  bf16:  c  >=  tau - 1.001 coef(E) R_max ||q||
(csrc/coarse_scan.hpp). On random rows e_r.y is ~1/sqrt(E) of its Cauchy-Schwarz bound, so a kernel could lose a term and stay
bit-exact. The families below put the error ALONG the query, so that each bound is met to within a few per cent of the term
it presses, and every term that is wrong by 1 % drops a row of the true top K.

Restatements: f32 where the kernels use f32 (the fma of the scan's left side through f64: one rounding); exact scores are the
oracle's (the kernel's fmaf order) for every row that can matter - fences, targets and spacers - and an f32 matrix product for
the fillers, which lie below half of the K-th best (asserted). Layout as tests/test_topk_e768.py::_int8_bound_survivors and
tests/test_topk_wide768.py::_wide_bound_survivors have it: rmax, amax, the sample of the first 12 288 ROWS, the segment
boundaries in SLOTS of the copy, the running tau = exact K-th best of the rows of the segments already scanned.

Every restatement returns, for the (query, row) pairs asked for: `passed` (the f32 compare), `room` = (lhs - thr) t_q in score
units, `term_row` = 1.001 a_r ||y|| (the int8 row term; the block's largest a_r in the wide form), `term_q` = the margin
(int8: its query half 1.001 (R_max + A_max) F_q; bf16: all of it) and `seg`, the segment the row's slot is scanned in."""
import numpy as np

import topk_magnitude as tm

f32 = np.float32
S1 = 12288                              # csrc/topk.hip sample_rows: the sample is the first 12 288 rows, exactly scored
FRAC = 125.0 / 256.0                    # 1/2 - delta, delta = 0.0117: a digit's error just under half a step, exact in binary
U24 = 2.0 ** -24

I8_MUTANTS_64 = ("row_off", "a_next", "a_99", "q_off", "inv_nb", "Y_nb", "F_nb", "rmax_mean")
I8_MUTANTS_WIDE = ("row_off", "blk_prev", "a_99", "q_off", "inv_nb", "Y_nb", "F_nb", "rmax_mean")
BF16_MUTANTS = ("coef_old", "rmax_mean")
# which families press which term: a mutant must drop a true top-K pair of EVERY query of these families' cases
PRESSED_BY = {"row_off": {"R"}, "a_next": {"R"}, "a_99": {"R"}, "blk_prev": {"R"}, "Y_nb": {"R"}, "inv_nb": {"R"},
              "q_off": {"Q"}, "F_nb": {"Q"}, "rmax_mean": {"Q", "B"}, "coef_old": {"B"}}


def coarse_segments(N, K):
    """csrc/topk.hip coarse_segments: [0, S2), [S2, N1), [N1, N) - the middle one only when N1 + 65536 <= N."""
    S2 = max(min((N * K // 2048 + 31) & ~31, (N // 8) & ~31), 32768)
    N1 = max((N // 4) & ~31, 4 * S2)
    return [S2, N1, N] if N1 + 65536 <= N else [S2, N]


def wide_segments(N):
    """csrc/topk.hip wide_segments: boundaries from 64 k rows, ratio 4."""
    s = (max(65536, S1) + 31) & ~31
    b = []
    while len(b) < 7 and s * 2 <= N and s + 65536 <= N:
        b.append(s)
        s = (s * 4) & ~31
    return b + [N]


def bf16_round(x):
    """f32 -> bf16 (round to nearest even) -> f32."""
    u = np.ascontiguousarray(x, f32).view(np.uint32)
    r = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return r.view(f32)


def bf16_coef(E, old=False):
    """bf16_margin_coef<E>; old: the constant before tests/coarse_tight.py (derived from 2^-9 instead of 2^-8)."""
    return f32(f32(0.0041 if old else 0.0080) + f32(2.0) * f32(E - 512) * f32(U24))


# ---- the copies ------------------------------------------------------------------------------------------------------------

class I8Copy:
    """quantize_rows_i8_kernel + clipmi_rows_stats: slots ordered by largest |component| (stable), one scale per 32 slots."""

    def __init__(self, db, form=None):
        """form: the norm computations (tests/topk_magnitude.py; None: `current`, what the kernels compute)."""
        form = self.form = form or tm.current
        N, E = db.shape
        self.N, self.E = N, E
        self.perm = np.argsort(np.abs(db).max(axis=1), kind="stable")
        self.N32 = N32 = (N + 31) // 32 * 32
        self.slot_row = np.full(N32, -1, np.int64)
        self.slot_row[:N] = self.perm
        self.row_slot = np.empty(N, np.int64)
        self.row_slot[self.perm] = np.arange(N)
        s = np.zeros(N32 // 32, f32)
        a = np.zeros(N32, f32)
        self.q8 = np.zeros((N32, E), np.int8)
        for b0 in range(0, N32, 1 << 15):                  # in pieces: the f32 image of 200 k x 768 need not exist at once
            b1 = min(b0 + (1 << 15), N32)
            xp = np.zeros((b1 - b0, E), f32)
            live = min(b1, N) - b0
            xp[:live] = db[self.perm[b0:b0 + live]]
            sb = form.block_scale(np.abs(xp).reshape((b1 - b0) // 32, -1).max(axis=1))
            sr = np.repeat(sb, 32)
            q8 = tm.digits(xp, (f32(1.0) / sr)[:, None])
            a[b0:b1] = form.err_norm(xp, sr, q8)
            s[b0 // 32:b1 // 32] = sb
            self.q8[b0:b1] = q8.astype(np.int8)
        a[N:] = 0
        self.s, self.srow, self.a = s, np.repeat(s, 32), a
        self.ablk = a.reshape(-1, 32).max(axis=1)
        norms = np.linalg.norm(db.astype(np.float64), axis=1)
        self.rmax = f32(norms.max() * (1 + 1e-6))
        self.rmean = f32(norms.mean())
        self.amax = f32(a.max() * (1 + 1e-6))


class I8Queries:
    """coarse_prep_kernel<I8 = true>: t_q, 1 / t_q, the digits p_q, 1.001 ||f_q||, ||y||."""

    def __init__(self, q, form=None):
        form = self.form = form or tm.current
        self.mx = np.abs(q).max(axis=1).astype(f32)
        self.t = np.where(self.mx > 0, self.mx / f32(127.0), f32(1.0)).astype(f32)
        with np.errstate(over="ignore"):
            self.inv = (f32(1.0) / self.t).astype(f32)
        self.p = tm.digits(q, self.inv[:, None])
        self.Y, self.F = form.query_norms(q, self.t, self.p)


def exact_scores(db, q, special, oracle):
    """[row][query] f32: the oracle's fmaf chain on the rows `special` (those that can reach a top K), an f32 product on the
    rest (callers assert those stay far below)."""
    ex = db @ q.T
    sp = np.ascontiguousarray(db[special])
    for i in range(q.shape[0]):
        ex[special, i] = oracle.scores(sp, q[i])
    return ex


def running_taus(exact, K, bounds, slot_row):
    """[segment][query]: the threshold each segment is scanned with - the sample's K-th best (first S1 ROWS), then the K-th
    best of the rows in the slots of the segments already scanned."""
    kth = lambda rows: np.partition(exact[rows], len(rows) - K, axis=0)[len(rows) - K]
    taus = [kth(np.arange(S1))]
    for r1 in bounds[:-1]:
        rows = slot_row[:r1]
        taus.append(kth(rows[rows >= 0]))
    return np.stack(taus).astype(f32)


def _seg_of(slots, bounds):
    return np.searchsorted(np.asarray(bounds[:-1]), slots, side="right")


def _fma32(d, s, c):
    """fmaf(d, s, c) for f32 arrays: the product is exact in f64."""
    return (d.astype(np.float64) * s.astype(np.float64) + c.astype(np.float64)).astype(f32)


def _nb(v, d):
    return np.roll(v, -d)                   # entry q becomes entry q + d (cyclic): "the neighbouring query's"


def i8_sides(cp, qm, E, wide, mut=None, nb=1):
    """The per-row and per-query constants of the int8 test, with one term mutated: (a_r per slot, yt, margin, inv)."""
    a = np.repeat(cp.ablk, 32) if wide else cp.a
    rmax, inv, Y, F = cp.rmax, qm.inv, qm.Y, qm.F
    if mut == "row_off": a = np.zeros_like(a)
    elif mut == "a_next": a = np.roll(a, -1)
    elif mut == "blk_prev": a = np.repeat(np.roll(cp.ablk, 1), 32)
    elif mut == "a_99": a = (a * f32(0.99)).astype(f32)
    elif mut == "inv_nb": inv = _nb(inv, nb)
    elif mut == "Y_nb": Y = _nb(Y, nb)
    elif mut == "F_nb": F = _nb(F, nb)
    elif mut == "rmax_mean": rmax = cp.rmean
    else: assert mut in (None, "q_off"), mut
    slack = f32(1e-4) * f32(E / 512.0)                                   # i8_round_slack<E>
    qhalf = (f32(1.001) * (rmax + cp.amax) * F).astype(f32)
    if mut == "q_off": qhalf = np.zeros_like(qhalf)
    with np.errstate(over="ignore", invalid="ignore"):
        margin = (qhalf + slack * rmax * Y).astype(f32)
        yt = (f32(1.001) * Y * inv).astype(f32)
    # no usable bound (coarse_prep_kernel's finite_q: a magnitude outside the proved range, or a non-finite margin): margin
    # +inf - the threshold is then -inf -, 1 / t_q read as 1 and the row term as 0
    ok = qm.form.in_range(qm.mx, qm.Y, cp.rmax, True) & np.isfinite(margin)
    return a, np.where(ok, yt, f32(0)), np.where(ok, margin, f32(np.inf)), np.where(ok, inv, f32(1))


def _thr(taus, margin, inv):
    """select_topk_kernel: (tau - margin) * (1 / t_q), and -inf whatever tau is where the margin is +inf."""
    with np.errstate(invalid="ignore", over="ignore"):
        thr = ((taus - margin[None, :]) * inv[None, :]).astype(f32)
    return np.where(np.isinf(margin)[None, :], f32(-np.inf), thr)


def i8_pairs(cp, qm, q, K, taus, bounds, rows, wide, mut=None, nb=1):
    """The int8 keep test (scan_coarse_kernel; wide: the wide scans with the block's largest a_r and the integer pre-test) on
    the pairs (query i, row rows[i][j]). `mut`: one term of the bound mutated (I8_MUTANTS_*), `nb` the neighbour's distance."""
    Q, E = q.shape
    a, yt, margin, inv = i8_sides(cp, qm, E, wide, mut, nb)
    slots = cp.row_slot[rows]                                            # [Q][k]
    seg = _seg_of(slots, bounds)
    D = np.einsum("qke,qe->qk", cp.q8[slots].astype(f32), qm.p).astype(f32)
    assert np.abs(D).max() < 2 ** 24 and np.array_equal(D, np.rint(D))
    ay = (a[slots] * yt[:, None]).astype(f32)
    lhs = _fma32(D, cp.srow[slots], ay)
    thr_seg = _thr(taus, margin, inv)
    thr = thr_seg[seg, np.arange(Q)[:, None]]
    passed = lhs >= thr
    if wide:                                                             # i8_pretest_dmin of the slot's block
        blk = slots // 32
        bmy = a[slots]                                                   # the (mutated) block maximum
        xq = (_fma32(-bmy, np.broadcast_to(yt[:, None], bmy.shape), thr) * (f32(1.0) / cp.s[blk]).astype(f32)).astype(f32)
        xq = np.clip(xq, f32(-1e9), f32(1e9))
        xq = ((xq - f32(2.0)).astype(f32) - (np.abs(xq) * f32(2e-6)).astype(f32)).astype(f32)
        passed &= D >= np.floor(xq)
    t64 = qm.t.astype(np.float64)[:, None]
    return dict(passed=passed, seg=seg, room=(lhs.astype(np.float64) - thr) * t64, lhs=lhs, thr=thr, margin=margin,
                term_row=f32(1.001) * cp.a[slots].astype(np.float64) * qm.Y[:, None] if not wide
                else f32(1.001) * cp.ablk[slots // 32].astype(np.float64) * qm.Y[:, None],
                term_q=(f32(1.001) * (cp.rmax + cp.amax) * qm.F).astype(np.float64)[:, None] * np.ones(rows.shape))


class Bf16Copy:
    def __init__(self, db):
        self.N, self.E = db.shape
        self.dbh = bf16_round(db)
        norms = np.linalg.norm(db.astype(np.float64), axis=1)
        self.rmax = f32(norms.max() * (1 + 1e-6))
        self.rmean = f32(norms.mean())
        self.row_slot = np.arange(self.N)
        self.slot_row = np.arange(self.N)


def bf16_margin(cp, q, mut=None, form=None):
    """coarse_prep_kernel<I8 = false>: bf16_margin_coef<E> * rmax * ||q|| * 1.001; +inf where there is no usable bound."""
    form = form or tm.current
    Y = form.query_norms(q, None, None)[0]
    rmax = cp.rmean if mut == "rmax_mean" else cp.rmax
    assert mut in (None, "coef_old", "rmax_mean"), mut
    with np.errstate(over="ignore"):
        margin = (bf16_coef(cp.E, old=(mut == "coef_old")) * rmax * Y * f32(1.001)).astype(f32)
    ok = form.in_range(np.abs(q).max(axis=1).astype(f32), Y, cp.rmax, False) & np.isfinite(margin)
    return np.where(ok, margin, f32(np.inf))


def bf16_pairs(cp, q, K, taus, bounds, rows, mut=None, form=None):
    """The bf16 keep test of scan_coarse_kernel<.., I8 = false>: c = f32 sum of the products of the bf16-rounded operands."""
    Q = q.shape[0]
    margin = bf16_margin(cp, q, mut, form)
    seg = _seg_of(rows, bounds)
    c = np.einsum("qke,qe->qk", cp.dbh[rows], bf16_round(q)).astype(f32)
    thr = _thr(taus, margin, np.ones(Q, f32))[seg, np.arange(Q)[:, None]]
    return dict(passed=c >= thr, seg=seg, room=c.astype(np.float64) - thr, lhs=c, thr=thr, margin=margin,
                term_q=margin.astype(np.float64)[:, None] * np.ones(rows.shape))


def i8_survivors(db, q, K, exact, wide, form=None):
    """The int8 keep test on EVERY (query, row) pair, segment by segment (what tests/test_topk_e768.py and
    tests/test_topk_wide768.py check on unit rows). exact: [row][query] scores (f64 or the oracle's f32).
    Returns (every row of the true top K passes in its segment, the wide form's integer pre-test rejects no passing row -
    True on the 64-query form -, number of segments, fresh survivors per query)."""
    N, E = db.shape
    Q = q.shape[0]
    cp, qm = I8Copy(db, form), I8Queries(q, form)
    a, yt, margin, inv = i8_sides(cp, qm, E, wide)
    bounds = wide_segments(N) if wide else coarse_segments(N, K)
    taus = running_taus(exact, K, bounds, cp.slot_row)
    final = np.partition(exact, N - K, axis=0)[N - K]
    thr_seg = _thr(taus, margin, inv)
    tot = np.zeros(Q)
    ok = pre_ok = True
    for b0 in range(0, cp.N32, 1 << 15):
        b1 = min(b0 + (1 << 15), cp.N32)
        sl = np.arange(b0, b1)
        seg = _seg_of(sl, bounds)
        live = cp.slot_row[sl] >= 0
        D = cp.q8[sl].astype(f32) @ qm.p.T
        assert np.abs(D).max() <= E * 127 * 127 < 2 ** 24 and np.array_equal(D, np.rint(D))
        lhs = _fma32(D, cp.srow[sl, None], (a[sl, None] * yt[None, :]).astype(f32))
        thr = thr_seg[seg]                                               # [slot][query]
        passed = (lhs >= thr) & live[:, None]                            # slots beyond the last row never pass
        tot += passed.sum(axis=0)
        need = np.zeros_like(passed)
        need[live] = exact[cp.slot_row[sl[live]]] >= final[None, :]
        ok &= bool((passed | ~need).all())
        if wide:                                                         # i8_pretest_dmin per (block, query)
            xq = (_fma32(-a[sl, None], np.broadcast_to(yt[None, :], thr.shape), thr) * (f32(1.0) / cp.srow[sl, None]).astype(f32)).astype(f32)
            xq = np.clip(xq, f32(-1e9), f32(1e9))
            xq = ((xq - f32(2.0)).astype(f32) - (np.abs(xq) * f32(2e-6)).astype(f32)).astype(f32)
            pre_ok &= bool((~passed | (D >= np.floor(xq))).all())
    return ok, pre_ok, len(bounds), tot


# ---- the measurement hooks (GPU tests) --------------------------------------------------------------------------------------

def scan_hook(clipmi, gpu, idx, q, K, copy, what="coarse scan hook"):
    """The measurement hook of the path the queries q take on index idx (copy: "bf16" or "int8"; more than 64 queries: the
    wide hook), one repetition -> (scores, ids, re-scored pairs, fallback armed - None on the 64-query hooks)."""
    import ctypes as C
    import torch
    L = clipmi._lib.lib()
    N, E, Q = idx.ntotal, idx.d, q.shape[0]
    qd = torch.from_numpy(np.ascontiguousarray(q, f32)).to(gpu)
    need = max(L.clipmi_topk_ip_coarse_workspace_bytes(N, E, Q, K), L.clipmi_topk_ip_wide_workspace_bytes(N, E, Q, K))
    assert need > 0, clipmi._lib.last_error()
    ws = torch.empty(need, dtype=torch.uint8, device=gpu)
    os_ = torch.empty((Q, K), dtype=torch.float32, device=gpu)
    oi_ = torch.full((Q, K), -7, dtype=torch.int64, device=gpu)
    ms, surv, nl, armed = C.c_float(0), C.c_longlong(-1), C.c_int(-1), C.c_int(-1)
    db = idx.matrix()
    tail = (qd.data_ptr(), Q, K, os_.data_ptr(), oi_.data_ptr(), ws.data_ptr(), ws.numel(), None, 1, C.byref(ms), C.byref(surv))
    if copy == "bf16":
        dbh, rmax = idx.matrix_bf16()
        rc = L.clipmi_dbg_topk_coarse_scan_ms(db.data_ptr(), dbh.data_ptr(), N, E, rmax, *tail)
    else:
        db8, meta, amax, rmax = idx.matrix_i8()
        if Q <= 64:
            rc = L.clipmi_dbg_topk_coarse_i8_scan_ms(db.data_ptr(), db8.data_ptr(), meta.data_ptr(), amax, N, E, rmax, *tail)
        else:
            rc = L.clipmi_dbg_topk_wide_i8_scan_ms(db.data_ptr(), db8.data_ptr(), meta.data_ptr(), amax, N, E, rmax, *tail,
                                                   C.byref(nl), C.byref(armed))
    clipmi._lib.check(rc, what)
    torch.cuda.synchronize()
    return os_.cpu().numpy(), oi_.cpu().numpy(), surv.value, (armed.value if Q > 64 else None)


# ---- survivor counts with a rounding band (tests/test_coarse_survivors_gpu.py) ------------------------------------------------

def count_band(db, q, K, exact, kind, mut=None, cp=None):
    """Fresh survivors of a 64-query search, summed over queries and segments: (pairs that pass by more than the rounding
    band, pairs that pass or miss by no more than it), and the number of segments. The band, from the operations of the
    kernel's test (u = 2^-24, an ulp of x is at most 2 u |x|):
      int8  lhs = fmaf(D, s_r, fl(a_r yt)), D exact: half an ulp of lhs + half an ulp of a_r yt <= |lhs| near the threshold;
            thr = fl(fl(tau - margin) / t_q): two half ulps; the inputs a_r, ||y||, ||f_q|| (f64 sums of E squares, in another
            order than numpy's, rounded up to f32: an ulp at the most apart) move a_r yt and the margin, both < 0.1 |thr| on
            unit rows, by an ulp of THEIRS: under one ulp of thr. Taken: 4 ulp of max(|lhs|, |thr|).
      bf16  lhs = c is an f32 accumulation of E exact products in the matrix core's order: within E u ||x^|| ||q^|| of the sum
            in real numbers (computed here in f64); thr as above: + 2 ulp of |thr|."""
    N, E = db.shape
    Q = q.shape[0]
    bounds = coarse_segments(N, K)
    if kind == "int8":
        cp, qm = cp or I8Copy(db), I8Queries(q)
        a, yt, margin, inv = i8_sides(cp, qm, E, False, mut)
        D = cp.q8.astype(f32) @ qm.p.T
        lhs = _fma32(D, cp.srow[:, None], (a[:, None] * yt[None, :]).astype(f32)).astype(np.float64)
        live = cp.slot_row >= 0
        band_l = 4 * 2 * U24 * np.abs(lhs)
        thr_ulps = 4
    else:
        cp = cp or Bf16Copy(db)
        margin, inv = bf16_margin(cp, q, mut), np.ones(Q, f32)
        qh = bf16_round(q).astype(np.float64)
        lhs = cp.dbh.astype(np.float64) @ qh.T
        live = np.ones(N, bool)
        band_l = E * U24 * np.linalg.norm(cp.dbh.astype(np.float64), axis=1)[:, None] * np.linalg.norm(qh, axis=1)[None, :]
        thr_ulps = 2
    taus = running_taus(exact, K, bounds, cp.slot_row)
    thr_seg = _thr(taus, margin, inv)
    sure = maybe = 0
    r0 = 0
    for g, r1 in enumerate(bounds):
        r1 = min((r1 + 31) // 32 * 32, lhs.shape[0]) if r1 == N else r1
        m = live[r0:r1]
        T = thr_seg[g].astype(np.float64)[None, :]
        band = np.maximum(band_l[r0:r1][m], thr_ulps * 2 * U24 * np.abs(T)) if kind == "int8" else band_l[r0:r1][m] + thr_ulps * 2 * U24 * np.abs(T)
        diff = lhs[r0:r1][m] - T
        sure += int((diff > band).sum())
        maybe += int((diff >= -band).sum())
        r0 = r1
    return sure, maybe, len(bounds)


# ---- the row families ---------------------------------------------------------------------------------------------------------

K_TIGHT = 8


class Case:
    """db [N][E], q [Q][E], targets / fences [Q][K] row ids, special = ids of every row that is not a filler."""


def _signs(rng, n, E):
    return (rng.integers(0, 2, (n, E)) * 2 - 1).astype(np.float64)


def _mags(rng, E):
    """digits 0..3 in equal numbers over components 1 .. E-1, shuffled (component 0 carries the 127)."""
    m = np.zeros(E)
    m[1:] = rng.permutation(np.arange(E - 1) % 4)
    return m


def _tune(db, q, rows_q, oracle, K):
    """Moves component 1 of query i's 2K rows (fences then targets) until the oracle's scores are S0 + 4 ulp * (-K .. -1,
    1 .. K): all distinct, targets above fences by ~1e-6 relative."""
    for i, rows in enumerate(rows_q):
        sc = oracle.scores(db[rows], q[i]).astype(np.float64)
        S0 = f32(sc[K])
        want = S0 + 4.0 * np.spacing(S0) * np.concatenate([np.arange(-K, 0), np.arange(1, K + 1)])
        for _ in range(6):
            sc = oracle.scores(db[rows], q[i]).astype(np.float64)
            if np.array_equal(sc.astype(f32), want.astype(f32)):
                break
            db[rows, 1] = (db[rows, 1].astype(np.float64) + (want - sc) / float(q[i, 1])).astype(f32)
        sc = oracle.scores(db[rows], q[i])
        assert np.array_equal(sc, want.astype(f32)), (i, sc - want)


def _fillers(rng, n, E, h, bmax):
    """body (a Gaussian direction of norm U[0.2, 1] bmax, clipped under the spike) + one spike of height h: the spike is the
    row's largest |component| and so decides its slot; norms and error norms vary."""
    x = rng.standard_normal((n, E), dtype=f32)
    x *= ((rng.uniform(0.2, 1.0, n) * bmax) / np.linalg.norm(x, axis=1))[:, None].astype(f32)
    np.clip(x, -(0.9 * h)[:, None].astype(f32), (0.9 * h)[:, None].astype(f32), out=x)
    x[np.arange(n), rng.integers(4, E, n)] = (h * (rng.integers(0, 2, n) * 2 - 1)).astype(f32)
    return x


def group_starts(N):
    """slots where the three target groups start: in segment 0, 1 and the last of both segment plans (N = 70 001: two
    64-query segments, one wide; N = 200 003: three and two)."""
    return [16000, 36000, (N - 12000) & ~31]


def int8_case(family, E, N, Q, oracle, seed=1, K=K_TIGHT):
    """Family R (row term) or Q (query term) for the int8 copy. Row ids: Q K fences (in the sample, smallest |component|s:
    the first slots), three groups of targets (query i belongs to group i % 3), fillers. A group's rows share their largest
    |component| 127 s_g, so the stable order keeps them together in id order, from a slot that is a multiple of 32:
    blocks of 16 (target, spacer) pairs alternate with blocks of 32 spacers (spacer: integer multiples of s_g, a_r = 0)."""
    rng = np.random.default_rng(seed * 1000 + E + (7 if family == "Q" else 0))
    sig = _signs(rng, Q, E)
    pw = 2.0 ** -(np.arange(Q) % 4)                                       # neighbours differ by a factor
    grp = np.arange(Q) % 3
    if family == "R":
        q = sig * pw[:, None]                                             # f_q = 0
        sg = 2.0 ** -10 * np.array([0.8125, 0.875, 1.0])
        bmax, level = 60.0 * sg[2], None
    else:
        tq = 2.0 ** -8 * pw
        q = np.stack([tq[i] * sig[i] * (_mags(rng, E) + FRAC) for i in range(Q)])
        q[:, 0] = sig[:, 0] * 127.0 * tq
        rho = 96 * 88 * 80 * 2.0 ** -25                                   # the targets' level: 96 s_0 = 88 s_1 = 80 s_2
        sg = rho / np.array([96.0, 88.0, 80.0])
        bmax, level = 5.0 * rho, rho
    A = 127.0 * sg
    nf = Q * K
    fences = np.arange(nf).reshape(Q, K)
    starts = group_starts(N)
    sizes = [(-(-(int((grp == g).sum()) * K) // 16)) * 64 for g in range(3)]
    assert nf <= min(S1, starts[0]) and all(starts[g] + sizes[g] <= (starts + [N])[g + 1] for g in range(3))
    db = np.zeros((N, E), f32)
    targets = np.zeros((Q, K), np.int64)
    rid = nf
    spans = []
    for g in range(3):
        blockrows = np.zeros((sizes[g], E))
        blockrows[:] = sg[g] * rng.integers(-3, 4, (sizes[g], E))         # spacers everywhere first
        blockrows[:, 3] = 127.0 * sg[g]
        pairs = [(i, j) for i in np.flatnonzero(grp == g) for j in range(K)]
        rng.shuffle(pairs)                                                # a block holds targets of several queries
        for n, (i, j) in enumerate(pairs):
            pos = (n // 16) * 64 + 2 * (n % 16)
            if family == "R":
                x = sg[g] * sig[i] * (_mags(rng, E) + FRAC)
                x[0] = sig[i, 0] * 127.0 * sg[g]
            else:
                x = level * sig[i]
                x[2] = sig[i, 2] * 127.0 * sg[g]
            blockrows[pos] = x
            targets[i, j] = rid + pos
        db[rid:rid + sizes[g]] = blockrows
        spans.append((rid, rid + sizes[g]))
        rid += sizes[g]
    nspecial = rid
    for i in range(Q):                                                    # fences: flat along the query, the targets' score
        x = db[targets[i, 0]].astype(np.float64)
        c = float(x @ q[i]) / float(np.abs(q[i]).sum())
        db[fences[i]] = (c * sig[i]).astype(f32)
    # fillers: exactly as many spikes under each group's 127 s_g as put the group at its slot
    cnt = [starts[0] - nf, starts[1] - starts[0] - sizes[0], starts[2] - starts[1] - sizes[1]]
    cnt.append(N - nspecial - sum(cnt))
    edges = [0.85 * A[0], A[0], A[1], A[2], 1.15 * A[2]]
    h = np.concatenate([rng.uniform(edges[k] * 1.002, edges[k + 1] * 0.998, cnt[k]) for k in range(4)])
    h = h[rng.permutation(len(h))]
    db[nspecial:] = _fillers(rng, N - nspecial, E, h, bmax)
    q = q.astype(f32)
    _tune(db, q, [np.concatenate([fences[i], targets[i]]) for i in range(Q)], oracle, K)
    c = Case()
    c.family, c.E, c.N, c.Q, c.K = family, E, N, Q, K
    c.db, c.q, c.targets, c.fences, c.special, c.starts = db, q, targets, fences, np.arange(nspecial), starts
    return c


def bf16_case(E, N, Q, oracle, seed=1, K=K_TIGHT, delta=0.004):
    """Family B. Queries and targets are sigma_q * 2^-5 (2^-5-i%4 for the query) * (1 + (1 - delta) 2^-8): every mantissa just
    under a rounding tie, both round down, the coarse score loses 2 (1 - delta) 2^-8 of the exact one. Slots are rows here:
    query i's targets lie in segment i % (number of segments); targets and fences carry the largest norm."""
    rng = np.random.default_rng(seed * 1000 + E + 13)
    sig = _signs(rng, Q, E)
    m = 1.0 + (1.0 - delta) * 2.0 ** -8
    q = (sig * (2.0 ** -(5 + np.arange(Q) % 4))[:, None] * m).astype(f32)
    bounds = coarse_segments(N, K)
    nseg = len(bounds)
    base = [14000, bounds[0] + 6000, N - 9000] if nseg == 3 else [14000, N - 9000]
    nf = Q * K
    assert nf <= S1 and nf <= base[0]
    fences = np.arange(nf).reshape(Q, K)
    targets = np.stack([base[i % nseg] + (i // nseg) * K + np.arange(K) for i in range(Q)])
    db = rng.standard_normal((N, E), dtype=f32)
    R = 2.0 ** -5 * m * np.sqrt(E)
    db *= ((rng.uniform(0.2, 0.8, N) * R) / np.linalg.norm(db, axis=1))[:, None].astype(f32)
    for i in range(Q):
        db[fences[i]] = db[targets[i]] = (sig[i] * 2.0 ** -5 * m).astype(f32)
    _tune(db, q, [np.concatenate([fences[i], targets[i]]) for i in range(Q)], oracle, K)
    c = Case()
    c.family, c.E, c.N, c.Q, c.K = "B", E, N, Q, K
    c.db, c.q, c.targets, c.fences = db, q, targets, fences
    c.special = np.unique(np.concatenate([fences.ravel(), targets.ravel()]))
    return c


_cases = {}


def case(family, E, N, Q, oracle):
    """Built once per process. Queries beyond the first 64 repeat the construction with other sign vectors; a search of the
    first Q' < Q queries is a case of its own (their fences and targets are all there)."""
    key = (family, E, N, Q)
    if key not in _cases:
        _cases[key] = bf16_case(E, N, Q, oracle) if family == "B" else int8_case(family, E, N, Q, oracle)
    return _cases[key]
