"""The range of K every search entry point accepts, found from the library itself (no GPU: the workspace functions and the
merge's argument checks are host code), and the map of plan regimes over that range which tests/test_topk_krange_gpu.py runs.

K is the one search argument a user raises without limit while the program runs (query-index.py:111 asks for k + offset + 1,
repl.py adds 50 per "more"), and K decides which code runs: csrc/topk.hip make_plan picks waves per workgroup, queries per pass
and the select's staging from it, coarse_plan first plans inside COARSE_SIDE_LDS and falls back to the full LDS.

Everything numeric below is COMPUTED: KMAX by bisection on workspace_bytes > 0, the regime edges by a Python restatement of
make_plan that this file checks against the library for every K from 1 to KMAX + 64 (accept / refuse AND the exact scan's
workspace bytes, which pin waves, queries per pass and list capacity)."""
import ctypes as C
import functools
import os
import re
import sys

import numpy as np
import pytest

from conftest import unit_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- csrc/topk.hip's constants, restated (test_restated_plan_matches_the_library fails when one of them moves) ---------------
LDS_LIMIT = 160 * 1024 - 512
COARSE_SIDE_LDS = 100 * 1024
SEL_STAGE = 12288
SEL_FIXED = 32 * 8 + (256 + 8 + 8) * 4
NUM_CU = 256
SAMPLE_MIN_N = 65536
COARSE_CAP = 1 << 18
WIDE_CAP = 1 << 15
GIB2 = 2 << 30

WIDTHS = (512, 768)
EXACT_WS, COARSE_WS, WIDE_WS = ("clipmi_topk_ip_workspace_bytes", "clipmi_topk_ip_coarse_workspace_bytes",
                                "clipmi_topk_ip_wide_workspace_bytes")


def _lib():
    import clipmi
    return clipmi._lib.lib()


def sel_stage_entries(K, limit=LDS_LIMIT):
    room = int((limit - SEL_FIXED - K * 8) / 8)           # C++ division truncates toward zero
    return SEL_STAGE if room >= SEL_STAGE else max(room, 0)


def make_plan(N, E, Q, K, limit=LDS_LIMIT):
    """csrc/topk.hip make_plan: None where it refuses, else the plan's fields."""
    if N < 0 or Q < 1 or K < 1 or E not in WIDTHS:
        return None
    Cc = (K + 16 + 15) // 16 * 16
    found = None
    for w in (4, 2, 1):
        for qg in ((2, 1) if Q > 16 else (1,)):
            qimg = qg * (E // 16) * 1024
            per_wave = int((limit - qimg) / w) - 256
            fit = int(per_wave / (Cc * 8)) - 1
            qwant = min(Q, 16 * qg)
            if fit >= qwant or (qg == 1 and fit >= 1):
                found = (w, qg, min(fit, qwant))
                break
        if found:
            break
    if not found or SEL_FIXED + K * 8 > limit:
        return None
    waves, QG, QA = found
    stage = sel_stage_entries(K, limit)
    lds_sel = SEL_FIXED + K * 8 + stage * 8
    if lds_sel > limit:
        return None
    wave_bytes = (QA + 1) * Cc * 8 + 256
    grid = max(1, min(NUM_CU, ((N + 15) // 16 + waves - 1) // waves))
    S = 4096
    while S < 65536 and S * S < N * K:
        S *= 2
    grid_sample = (S // 16 + waves - 1) // waves
    nl = max(grid * waves, grid_sample * waves)
    cap = min(nl * Cc, (max(N, 1) + 15) // 16 * 16)       # never more entries per query than rows scanned
    return dict(C=Cc, waves=waves, QG=QG, QA=QA, stage=stage, lds_sel=lds_sel, lds_scan=QG * (E // 16) * 1024 + waves * wave_bytes,
                grid=grid, sample=N >= SAMPLE_MIN_N, sample_rows=S, grid_sample=grid_sample, cap=cap, limit=limit)


def coarse_plan(N, E, Q, K):
    """csrc/topk.hip coarse_plan: the side kernels' plan, inside COARSE_SIDE_LDS when K allows, else inside the full LDS."""
    q = min(Q, 32)
    return make_plan(N, E, q, K, COARSE_SIDE_LDS) or make_plan(N, E, q, K)


def exact_workspace_bytes(p):
    return (p["QA"] * p["cap"] * 8 + 255) // 256 * 256 + 768


def bisect_kmax(fn, N, E, Q, hi=1 << 20):
    """Largest K with fn(N, E, Q, K) > 0 (0 when even K = 1 is refused), by bisection; `hi` must be refused."""
    f = getattr(_lib(), fn)
    assert f(N, E, Q, hi) == 0
    if f(N, E, Q, 1) == 0:
        return 0
    lo = 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if f(N, E, Q, mid) > 0:
            lo = mid
        else:
            hi = mid
    return lo


# ---- the bound, exported: computed (on first use, so that collecting the suite loads no library), never typed in --------------
class _KmaxByWidth(dict):
    def __missing__(self, E):
        assert E in WIDTHS
        self[E] = bisect_kmax(EXACT_WS, 70001, E, 1)
        return self[E]


KMAX = _KmaxByWidth()


def merge_kmax(R):
    """Largest K clipmi_merge_topk takes for R lists: R K 12 + 16 bytes of LDS in one pass."""
    return (LDS_LIMIT - 16) // (12 * R)


MERGE_R = (1, 2, 3, 8)


def _last(pred, lo, hi):
    """Largest K in [lo, hi] with pred(K), None if none (pred need not be monotone: a plain scan)."""
    best = None
    for K in range(lo, hi + 1):
        if pred(K):
            best = K
    return best


@functools.lru_cache(maxsize=None)
def exact_regimes(E):
    """[(label, K, waves, QA)] - one K inside every regime of the exact scan's plan at row width E: the LAST K of each of
    (4 waves, 32 queries per pass), (4, 16), (4, 3), 2 waves, then the FIRST K with one wave, then KMAX. QA is the plan's for a
    large batch (it is what Q = 2 QA + 1 then gets: test_the_gpu_cases_reach_their_regimes)."""
    kmax = KMAX[E]
    big = {K: make_plan(70001, E, 1024, K) for K in range(1, kmax + 1)}
    at = lambda w, qa: _last(lambda K: (big[K]["waves"], big[K]["QA"]) == (w, qa), 1, kmax)
    k2 = _last(lambda K: big[K]["waves"] == 2, 1, kmax)
    out = [("4 waves, QA 32", at(4, 32)), ("4 waves, QA 16", at(4, 16)), ("4 waves, QA 3", at(4, 3)), ("2 waves", k2),
           ("1 wave", k2 + 1), ("Kmax", kmax)]
    return [(lab, K, big[K]["waves"], big[K]["QA"]) for lab, K in out]


@functools.lru_cache(maxsize=None)
def coarse_ks(E):
    """[(label, K)] for the coarse and wide paths at row width E: staging still whole (the last such K), just past where
    sel_stage_entries(K, COARSE_SIDE_LDS) starts to shrink, the last K the 100-KiB plan takes, the first that falls back to the
    full LDS, KMAX."""
    kmax = KMAX[E]
    whole = _last(lambda K: sel_stage_entries(K, COARSE_SIDE_LDS) == SEL_STAGE, 1, kmax)
    side = _last(lambda K: make_plan(70001, E, 32, K, COARSE_SIDE_LDS) is not None, 1, kmax)
    return [("stage whole", whole), ("stage shrinks", whole + 1), ("last in 100 KiB", side), ("full LDS", side + 1), ("Kmax", kmax)]


def exact_q(QA):
    return 3 if QA == 1 else 2 * QA + 1


EXACT_NS = (70001, 20000)                      # above SAMPLE_MIN_N (pre-pass + its select run), below it; N = K - 7 per case
COARSE_NS = (70001, 131101)                    # two and three segments
PASS64_Q = (1, 33, 64)
WIDE_Q = (65, 130)
PIPELINED_Q = (65, 130)                        # index.py _search_pipelined: 64-query calls on two streams, a ragged last call
PIPELINED_PATHS = (("bf16", 512), ("bf16", 768), ("int8", 768))       # int8 at 768 WITHOUT wide_768: search_route's default
TIE_N = 70001
COARSE_PATHS = (("bf16", 512), ("bf16", 768), ("int8", 512), ("int8", 768), ("wide", 512), ("wide", 768))


def path_workspace_fn(path, E):
    return WIDE_WS if (path == "wide" and E == 768) else COARSE_WS


def gpu_shapes():
    """Every (workspace function, N, E, Q, K) tests/test_topk_krange_gpu.py calls with."""
    shapes = []
    for E in WIDTHS:
        for _, K, _, QA in exact_regimes(E):
            for N in EXACT_NS + (K - 7,):
                if N >= 1:
                    shapes.append((EXACT_WS, N, E, exact_q(QA), K))
        for path, Ep in COARSE_PATHS:
            if Ep != E:
                continue
            for _, K in coarse_ks(E):
                for N in COARSE_NS:
                    for Q in (WIDE_Q if path == "wide" else PASS64_Q):
                        shapes.append((path_workspace_fn(path, E), N, E, Q, K))
                        if path == "wide":                    # the hook sizes its workspace by the larger of the two
                            shapes.append((WIDE_WS, N, E, Q, K))
        for path, Ep in PIPELINED_PATHS:
            if Ep != E:
                continue
            for _, K in coarse_ks(E):
                for N in COARSE_NS:
                    for Q in PIPELINED_Q:                     # every call of a pipelined search: 64 queries, then the rest
                        shapes.append((COARSE_WS, N, E, 64, K))
                        shapes.append((COARSE_WS, N, E, Q % 64, K))
                    shapes.append((COARSE_WS, N, E, 130, K))  # and the same search as one call on one stream
        for K in (3000, KMAX[E]):
            shapes.append((EXACT_WS, TIE_N, E, 3, K))
            shapes.append((COARSE_WS, TIE_N, E, 5, K))
    return shapes


# ---- tests -------------------------------------------------------------------------------------------------------------------
QS = (1, 16, 17, 32, 64, 1024)
NS = (1000, 70001, 10_000_000)


def _probes(kmax):
    ks = {1, 2, 3, kmax - 1, kmax, kmax + 1, kmax + 2, kmax + 64, 2 * kmax, 100000, (1 << 20) - 1, (1 << 31) - 1}
    ks |= {1 << i for i in range(1, 20)} | {(1 << i) + 1 for i in range(1, 20)} | {(1 << i) - 1 for i in range(2, 20)}
    ks |= set(range(16, kmax + 64, 97))
    return sorted(k for k in ks if k >= 1)


@pytest.mark.parametrize("E", WIDTHS)
def test_kmax_is_one_number_per_width(clipmi, E):
    """Bisection for the three workspace functions over every Q and N: acceptance is monotone in K (every probed K <= Kmax is
    accepted, every probed K above is refused), Kmax depends neither on N nor on Q, and the exact, coarse and wide entries agree
    on it - so index.py's route can never send a K to an entry that refuses it while the exact scan would take it."""
    L = _lib()
    seen = {}
    for fn in (EXACT_WS, COARSE_WS, WIDE_WS):
        f = getattr(L, fn)
        for N in NS:
            for Q in QS:
                kmax = bisect_kmax(fn, N, E, Q)
                if fn != EXACT_WS and N < SAMPLE_MIN_N:
                    assert kmax == 0, f"{fn} takes N = {N}"          # no coarse path below SAMPLE_MIN_N, whatever K
                    continue
                seen[(fn, N, Q)] = kmax
                for K in _probes(kmax):
                    got = f(N, E, Q, K)
                    assert (got > 0) == (K <= kmax), f"{fn}(N={N}, E={E}, Q={Q}, K={K}) = {got}, Kmax = {kmax}"
    assert set(seen.values()) == {KMAX[E]}, {k: v for k, v in seen.items() if v != KMAX[E]}
    # every K of the range, one N and the Q on both sides of a pass width: no hole anywhere
    for fn in (EXACT_WS, COARSE_WS, WIDE_WS):
        f = getattr(L, fn)
        for Q in (1, 17, 1024):
            bad = [K for K in range(1, KMAX[E] + 65) if (f(70001, E, Q, K) > 0) != (K <= KMAX[E])]
            assert not bad, (fn, Q, bad[:5])
    print(f"E={E}: Kmax = {KMAX[E]} for clipmi_topk_ip, _coarse, _coarse_i8, _wide_i8; any N, any Q")


def _promised(text, E):
    """The K bound a message or comment states for row width E: 'K <= 8128 at E = 512, <= 7104 at E = 768'."""
    m = re.search(r"<=\s*(\d+)\s+at\s+E\s*=\s*%d" % E, text)
    assert m, f"no K bound for E = {E} in: {text!r}"
    return int(m.group(1))


@pytest.mark.parametrize("E", WIDTHS)
def test_the_stated_bound_is_the_true_one(clipmi, E):
    """The error text of a refused K and include/clipmi.h state, for each row width, exactly the largest K the library takes
    (the text used to say "~8000" for both widths; 768 stops about 900 earlier)."""
    L = _lib()
    assert L.clipmi_topk_ip_workspace_bytes(1000, E, 1, KMAX[E] + 1) == 0
    msg = clipmi._lib.last_error()
    assert _promised(msg, E) == KMAX[E], msg
    assert L.clipmi_topk_ip_coarse_workspace_bytes(70001, E, 1, KMAX[E] + 1) == 0
    msg = clipmi._lib.last_error()
    assert _promised(msg, E) == KMAX[E], msg
    # the search entry itself: argument validation only (a refused K launches nothing - N = 0 would not even need a database)
    fake = C.c_void_p(256)
    rc = L.clipmi_topk_ip(fake, clipmi._lib.F32, 1000, E, fake, 1, KMAX[E] + 1, 0, fake, fake, fake, 1 << 30, None)
    assert rc == 1 and _promised(clipmi._lib.last_error(), E) == KMAX[E]
    header = open(os.path.join(ROOT, "include", "clipmi.h")).read()
    assert _promised(header, E) == KMAX[E]
    assert "~8000" not in header and "~8000" not in msg
    m = re.search(r"R \* K <= (\d+)", header)
    assert m and int(m.group(1)) == merge_kmax(1)
    m = re.search(r"eight shards merge on the device up to K = (\d+)", header)
    assert m and int(m.group(1)) == merge_kmax(8)


@pytest.mark.parametrize("E", WIDTHS)
def test_restated_plan_matches_the_library(clipmi, E):
    """The Python restatement of make_plan / coarse_plan that picks the GPU file's K values answers accept / refuse as the
    library does for K = 1 .. Kmax + 64, and gives the exact scan's workspace to the byte (QA x list capacity: a wrong wave count,
    queries per pass or capacity shows)."""
    L = _lib()
    for N, Q in ((70001, 1), (70001, 17), (70001, 65), (20000, 33), (1000, 1024), (10_000_000, 32), (9, 3)):
        for K in range(1, KMAX[E] + 65):
            p = make_plan(N, E, Q, K)
            want = L.clipmi_topk_ip_workspace_bytes(N, E, Q, K)
            assert (exact_workspace_bytes(p) if p else 0) == want, (N, E, Q, K, p, want)
    for K in range(1, KMAX[E] + 65):
        assert (coarse_plan(70001, E, 64, K) is not None) == (L.clipmi_topk_ip_coarse_workspace_bytes(70001, E, 64, K) > 0), K
    assert make_plan(70001, E, 1, KMAX[E]) and not make_plan(70001, E, 1, KMAX[E] + 1)


def test_the_gpu_cases_reach_their_regimes(clipmi):
    """The K values the GPU file runs: every regime exists at both widths, the chosen Q = 2 QA + 1 really plans QA queries per
    pass (three passes, a ragged last one), the coarse K values straddle the 100-KiB plan's limit and the staging switch."""
    rows = []
    for E in WIDTHS:
        reg = exact_regimes(E)
        assert [r[2] for r in reg] == [4, 4, 4, 2, 1, 1] and [r[3] for r in reg][:3] == [32, 16, 3], reg
        assert all(K is not None and 1 <= K <= KMAX[E] for _, K, _, _ in reg) and len({K for _, K, _, _ in reg}) == 6
        for lab, K, waves, QA in reg:
            Q = exact_q(QA)
            for N in EXACT_NS + (K - 7,):
                p = make_plan(N, E, Q, K)
                assert (p["waves"], p["QA"]) == (waves, QA) and -(-Q // QA) == 3 and (Q % QA != 0 or QA == 1), (lab, N, p)
                assert p["sample"] == (N >= SAMPLE_MIN_N)
            p = make_plan(70001, E, Q, K)
            rows.append(f"exact E={E} {lab:15s} K={K:5d} Q={Q:3d}: waves {waves} QA {QA:2d} stage {p['stage']:5d} C {p['C']:5d} "
                        f"sample rows {p['sample_rows']:5d} workspace {exact_workspace_bytes(p):>10d} B")
        ck = dict(coarse_ks(E))
        assert 1 < ck["stage whole"] < ck["last in 100 KiB"] < ck["full LDS"] < ck["Kmax"] == KMAX[E], ck
        assert sel_stage_entries(ck["stage whole"], COARSE_SIDE_LDS) == SEL_STAGE > sel_stage_entries(ck["stage shrinks"], COARSE_SIDE_LDS)
        for lab, K in coarse_ks(E):
            p = coarse_plan(70001, E, 64, K)
            assert (p["limit"] == COARSE_SIDE_LDS) == (K <= ck["last in 100 KiB"])
            ws = _lib().clipmi_topk_ip_coarse_workspace_bytes(70001, E, 64, K)
            rows.append(f"coarse E={E} {lab:15s} K={K:5d}: plan in {p['limit'] // 1024:3d} KiB, waves {p['waves']} QA {p['QA']:2d} "
                        f"stage {p['stage']:5d}, 64-query workspace at 70 001 rows {ws:>10d} B")
    print("\n" + "\n".join(rows))


@pytest.mark.parametrize("E", WIDTHS)
def test_workspace_at_kmax_is_finite_and_sane(clipmi, E):
    """A list never holds more than one entry per row, so no workspace needs more than (queries in flight) x (rows + the coarse
    lists' fixed capacity) entries of 8 bytes, plus the query image and counters (< 2 MiB). (make_plan used to size the exact
    lists by waves x (K + 16) whatever N: 133 MB per query at Kmax for 70 001 rows, 8.5 GB for a 64-query coarse search.)"""
    L = _lib()
    for N in (1000, 70001, 10_000_000):
        for Q in QS:
            for K in (KMAX[E], KMAX[E] // 2):
                rows16 = (N + 15) // 16 * 16
                ws = L.clipmi_topk_ip_workspace_bytes(N, E, Q, K)
                assert 0 < ws <= min(Q, 32) * rows16 * 8 + 1024, (N, Q, K, ws)
                line = f"E={E} N={N} Q={Q} K={K}: exact {ws} B"
                if N >= SAMPLE_MIN_N:
                    qs = (min(Q, 1024) + 63) // 64 * 64
                    for fn in (COARSE_WS, WIDE_WS):
                        wc = getattr(L, fn)(N, E, Q, K)
                        assert 0 < wc <= qs * (rows16 + COARSE_CAP) * 8 + (2 << 20), (fn, N, Q, K, wc)
                        line += f", {fn[12:-16]} {wc} B"
                print(line)


def test_no_gpu_case_needs_more_than_2_gib_of_workspace(clipmi):
    L = _lib()
    shapes = gpu_shapes()
    assert len(shapes) > 100
    worst = max((getattr(L, fn)(N, E, Q, K), fn, N, E, Q, K) for fn, N, E, Q, K in shapes)
    for fn, N, E, Q, K in shapes:
        ws = getattr(L, fn)(N, E, Q, K)
        assert 0 < ws <= GIB2, (fn, N, E, Q, K, ws)
    print(f"largest workspace of a GPU case: {worst}")


def test_merge_limit_arithmetic(clipmi):
    """The K the GPU file calls clipmi_merge_topk's limit for each R: R K 12 + 16 <= LDS_LIMIT holds at it and fails one past it
    (the GPU file asserts rc == 0 there and CLIPMI_EUNSUPPORTED at K + 1: both need real buffers, the NULL check comes first)."""
    for R in MERGE_R:
        K = merge_kmax(R)
        assert R * K * 12 + 16 <= LDS_LIMIT < R * (K + 1) * 12 + 16
    assert _lib().clipmi_merge_topk(None, None, 2, 1, merge_kmax(2) + 1, None, None, None, 0, None) == 1     # NULL first


def _sharded_worker(rank, world, port, tmp, K):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch.distributed as dist
    import clipmi
    from conftest import TopkOracle
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        rng = np.random.default_rng(4040)          # same data on every rank
        N, Q = K + 901, 2                          # each shard holds fewer than K rows: pads in both partial lists
        db = unit_rows(rng, N, 512)
        db[N - 1] = db[3]                          # a duplicate across the shards
        q = unit_rows(rng, Q, 512)
        orc = TopkOracle()
        lo, hi = clipmi.shard_bounds(N, world, rank)
        sh = clipmi.ShardedFlatIP(None, N, local_search=lambda qq, k, base: orc.topk(db[lo:hi], np.asarray(qq), k, id_base=base))
        verdict = "wrong"
        try:
            D, I = sh.search(q, K)
            Dw, Iw = orc.topk(db, q, K)
            if np.array_equal(I, Iw) and np.array_equal(D.view(np.uint32), Dw.view(np.uint32)):
                verdict = "exact"
        except clipmi.ClipmiError as e:
            verdict = "refused" if re.search(r"\bK\b", str(e)) else "refused without naming K"
        open(os.path.join(tmp, f"verdict{rank}"), "w").write(verdict)
    finally:
        dist.destroy_process_group()


def test_sharded_search_past_the_device_merge_limit_gloo_world2(tmp_path):
    """World 2, K one past what clipmi_merge_topk takes for two lists: the gloo path merges on the host (merge_lists_host has no
    such limit) and must return the oracle's answer - or refuse with a ClipmiError that names K; never a wrong or empty result.
    Pinned: it returns the exact answer. (The GPU path merges with clipmi_merge_topk_packed, whose refusal - naming R*K - reaches
    the caller as a ClipmiError through _lib.check: tests/test_topk_krange_gpu.py checks that text.)"""
    import torch.multiprocessing as mp
    K = merge_kmax(2) + 1
    assert K <= KMAX[512]
    mp.spawn(_sharded_worker, args=(2, 29500 + (os.getpid() + 31) % 2000, str(tmp_path), K), nprocs=2, join=True)
    assert (tmp_path / "verdict0").read_text() == "exact" and (tmp_path / "verdict1").read_text() == "exact"
