"""Search of a 768-wide index (ViT-L/14): exact f32 scan (coarse=None - what every 768 index ran before the coarse paths took that width) against the int8 and bf16 coarse paths, ONE process, same rows. usage: python tools/search_e768.py [N] [calls]
Device events around `calls` (>= 40) calls after warm-up, the three forms alternated three times (best round reported, all rounds printed): K = 51,
Q = 1, 16, 64 with one call in flight and with two on two streams, one call of Q = 1024; per coarse kind the scan time of
the measurement hook, GB/s on N (E + 8) resp. N 2 E bytes, exactly re-scored rows per query. Results asserted identical.
Many-query legs (Q = 128, 256, 512, 1024, int8 copy): the opt-in one-pass wide call (IndexFlatIP(wide_768=True) ->
clipmi_topk_ip_wide_i8) against the pipelined 64-query form (the default), alternated in three rounds on ONE index copy, `calls`
calls per round; per Q the wide scan launches' summed duration and the re-scored rows per query from the hook.
--many-only: only those legs (and only the int8 copy is built). --out PATH: the many-query lines are also written to PATH
(profiles/r06_search_wide768.txt is the record DESIGN 4.1l quotes)."""
import sys, os, ctypes as C
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import clipmi
L = clipmi._lib.lib()
dev = torch.device("cuda:0")
argv = [a for a in sys.argv[1:] if not a.startswith("--")]
MANY_ONLY = "--many-only" in sys.argv
OUT = None
if "--out" in sys.argv:
    OUT = sys.argv[sys.argv.index("--out") + 1]
    argv.remove(OUT)
N = int(argv[0]) if len(argv) > 0 else 10_000_000
CALLS = max(40, int(argv[1])) if len(argv) > 1 else 40
E, K = 768, 51
FORMS = ("int8",) if MANY_ONLY else (None, "int8", "bf16")
g = torch.Generator(device=dev); g.manual_seed(1)
db = torch.empty((N, E), dtype=torch.float32, device=dev)
for lo in range(0, N, 1 << 20):
    blk = torch.randn((min(1 << 20, N - lo), E), generator=g, device=dev)
    db[lo:lo + blk.shape[0]] = blk / blk.norm(dim=1, keepdim=True)
del blk
idx = {}
for kind in FORMS:
    idx[kind] = clipmi.IndexFlatIP(E, device=dev, coarse=kind)
    idx[kind].add(db)
    assert idx[kind].uses_coarse() == (kind is not None)
idx["int8"].matrix_i8()
if not MANY_ONLY: idx["bf16"].matrix_bf16()
cur, side = clipmi._lib.side_stream(dev)
torch.cuda.synchronize()


def timed(ix, q, calls, two):
    """ms per call: `calls` searches back to back on the current stream, or dealt over it and the side stream (two in flight)."""
    lanes = [cur, side] if two else [cur]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    side.wait_stream(cur)
    e0.record(cur)
    for c in range(calls):
        with torch.cuda.stream(lanes[c % len(lanes)]):
            out = ix.search_device(q, K)
    cur.wait_stream(side)
    e1.record(cur)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls, out


def many_query_legs():
    """The wide call against the pipelined 64-query form, same process, same int8 copy."""
    lines = []

    def log(t):
        print(t, flush=True)
        lines.append(t)

    pipe = idx["int8"]
    wide = clipmi.IndexFlatIP(E, device=dev, coarse="int8", wide_768=True)
    wide.add(db)
    wide._db8, wide._rmax = pipe._db8, pipe._rmax                      # one copy for both forms
    forms = (("pipelined-64", pipe), ("wide", wide))
    qs = {}
    for Q in (128, 256, 512, 1024):
        q = torch.randn((Q, E), generator=g, device=dev)
        qs[Q] = q / q.norm(dim=1, keepdim=True)
    bestm, outs = {}, {}
    for rnd in range(3):
        for Q in qs:
            for name, ix in forms:
                if rnd == 0:
                    for _ in range(2): ix.search_device(qs[Q], K)
                    torch.cuda.synchronize()
                ms, out = timed(ix, qs[Q], CALLS, False)
                bestm[(name, Q)] = min(bestm.get((name, Q), 1e30), ms)
                outs[(name, Q)] = (out[0].clone(), out[1].clone())
                log(f"round {rnd} {name:12s} Q={Q:4d}: {ms:8.3f} ms per call = {Q / ms * 1e3:9.0f} q/s")
    for Q in qs:
        a, b = outs[("pipelined-64", Q)], outs[("wide", Q)]
        assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1]), Q
    log("results identical, wide vs pipelined 64-query form at Q = 128, 256, 512, 1024: True")
    log(f"N = {N} x {E}, K = {K}: best of 3 alternated rounds, {CALLS} calls each")
    d8, meta, amax, rmax = pipe.matrix_i8()
    for Q in qs:
        p_, w_ = bestm[("pipelined-64", Q)], bestm[("wide", Q)]
        ws = torch.empty(L.clipmi_topk_ip_wide_workspace_bytes(N, E, Q, K), dtype=torch.uint8, device=dev)
        sm, sv, nl, fa = C.c_float(0), C.c_longlong(0), C.c_int(0), C.c_int(0)
        os_ = torch.empty((Q, K), dtype=torch.float32, device=dev)
        oi_ = torch.empty((Q, K), dtype=torch.int64, device=dev)
        rc = L.clipmi_dbg_topk_wide_i8_scan_ms(db.data_ptr(), d8.data_ptr(), meta.data_ptr(), amax, N, E, rmax, qs[Q].data_ptr(), Q, K,
                                               os_.data_ptr(), oi_.data_ptr(), ws.data_ptr(), ws.numel(), None, 5, C.byref(sm),
                                               C.byref(sv), C.byref(nl), C.byref(fa))
        clipmi._lib.check(rc, "wide scan hook")
        assert torch.equal(oi_, outs[("wide", Q)][1])
        log(f"Q={Q:4d}: pipelined-64 {p_:8.3f} ms {Q / p_ * 1e3:8.0f} q/s | wide {w_:8.3f} ms {Q / w_ * 1e3:8.0f} q/s ({p_ / w_:5.2f} x) | "
            f"wide scans {sm.value:.3f} ms in {nl.value} launches = {2.0 * N * Q * E / sm.value / 1e9:.0f} int8 TOP/s, "
            f"re-scored rows per query {sv.value / Q:.0f}, fallback armed {fa.value}")
        del ws
    if OUT:
        with open(OUT, "w") as f:
            f.write("\n".join(lines) + "\n")


if MANY_ONLY:
    many_query_legs()
    sys.exit(0)

best, results = {}, {}
shapes = [(1, False), (1, True), (16, False), (16, True), (64, False), (64, True), (1024, False)]
queries = {}
for Q in (1, 16, 64, 1024):
    q = torch.randn((Q, E), generator=g, device=dev)
    queries[Q] = q / q.norm(dim=1, keepdim=True)
for rnd in range(3):
    for Q, two in shapes:
        calls = CALLS if Q <= 64 else 3
        for kind in FORMS:
            if rnd == 0:
                for _ in range(2): idx[kind].search_device(queries[Q], K)      # warm-up: workspaces, LDS opt-ins, copies
                torch.cuda.synchronize()
            ms, out = timed(idx[kind], queries[Q], calls, two)
            key = (kind, Q, two)
            best[key] = min(best.get(key, 1e30), ms)
            results[(kind, Q)] = (out[0].clone(), out[1].clone())
            print(f"round {rnd} {str(kind):5s} Q={Q:4d} {'two' if two else 'one'} in flight: {ms:8.3f} ms per call = {Q / ms * 1e3:9.0f} q/s", flush=True)
for Q in (1, 16, 64, 1024):
    a = results[(None, Q)]
    for kind in ("int8", "bf16"):
        b = results[(kind, Q)]
        assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1]), (kind, Q)
print("results identical across exact / int8 / bf16 at Q = 1, 16, 64, 1024: True")
print(f"\nN = {N} x {E}, K = {K}: best of 3 rounds, {CALLS} calls each (Q = 1024: 3 calls)")
for Q, two in shapes:
    ex = best[(None, Q, two)]
    line = f"Q={Q:4d} {'two' if two else 'one'} in flight: exact {ex:8.3f} ms {Q / ex * 1e3:8.0f} q/s"
    for kind in ("int8", "bf16"):
        ms = best[(kind, Q, two)]
        line += f" | {kind} {ms:8.3f} ms {Q / ms * 1e3:8.0f} q/s ({ex / ms:5.2f} x)"
    print(line)
for kind in ("int8", "bf16"):
    for Q in (1, 16, 64):
        q = queries[Q]
        ws = torch.empty(L.clipmi_topk_ip_coarse_workspace_bytes(N, E, Q, K), dtype=torch.uint8, device=dev)
        sm, sv = C.c_float(0), C.c_longlong(0)
        os_ = torch.empty((Q, K), dtype=torch.float32, device=dev)
        oi_ = torch.empty((Q, K), dtype=torch.int64, device=dev)
        if kind == "bf16":
            dbh, rmax = idx[kind].matrix_bf16()
            rc = L.clipmi_dbg_topk_coarse_scan_ms(db.data_ptr(), dbh.data_ptr(), N, E, rmax, q.data_ptr(), Q, K, os_.data_ptr(), oi_.data_ptr(),
                                                  ws.data_ptr(), ws.numel(), None, 5, C.byref(sm), C.byref(sv))
            byt = N * 2 * E
        else:
            d8, meta, amax, rmax = idx[kind].matrix_i8()
            rc = L.clipmi_dbg_topk_coarse_i8_scan_ms(db.data_ptr(), d8.data_ptr(), meta.data_ptr(), amax, N, E, rmax, q.data_ptr(), Q, K,
                                                     os_.data_ptr(), oi_.data_ptr(), ws.data_ptr(), ws.numel(), None, 5, C.byref(sm), C.byref(sv))
            byt = N * (E + 8)
        clipmi._lib.check(rc, "coarse scan hook")
        torch.cuda.synchronize()
        assert torch.equal(oi_, results[(None, Q)][1])
        print(f"{kind} Q={Q:2d}: scans {sm.value:.3f} ms = {byt / sm.value / 1e6:.0f} GB/s on {byt / 1e9:.2f} GB; exactly re-scored rows per query {sv.value / Q:.0f}", flush=True)
many_query_legs()
