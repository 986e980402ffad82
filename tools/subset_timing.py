"""Subset search (clipmi_topk_ip_rows through IndexFlatIP.subset) at full size against the two ways of answering the same question
without it: clipmi_topk_ip over all rows and the default int8 coarse search, each then filtered on the host (development aid).

10 M x 512 unit rows generated on the device from a seed, K = 51, Q = 1 and 32. Every figure is the median of event-timed calls
after warm-up (REPS >= 20 per figure); the exact scan and each subset ALTERNATE call by call in one process, so both see the
same clocks. Per subset: ms per call, the main list scan's own time (clipmi_dbg_topk_rows_scan_ms), bytes = M E 4 + M 4 and TB/s
over the call. usage: subset_timing.py [N] [--out FILE]   (FILE: default profiles/subset_timing.txt, appended to)"""
import ctypes as C
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import clipmi  # noqa: E402

args = sys.argv[1:]
out_path = os.path.join(ROOT, "profiles", "subset_timing.txt")
if "--out" in args:
    out_path = args[args.index("--out") + 1]
    del args[args.index("--out"):args.index("--out") + 2]
N = int(args[0]) if args else 10_000_000
E, K, REPS, WARM = 512, 51, 20, 3
L = clipmi._lib.lib()
dev = torch.device("cuda:0")
g = torch.Generator(device=dev)
g.manual_seed(1)
db = torch.empty((N, E), dtype=torch.float32, device=dev)
for lo in range(0, N, 1 << 20):
    blk = torch.randn((min(1 << 20, N - lo), E), generator=g, device=dev)
    db[lo:lo + blk.shape[0]] = blk / blk.norm(dim=1, keepdim=True)
exact = clipmi.IndexFlatIP(E, device=dev)
exact.add(db)
coarse = clipmi.IndexFlatIP(E, device=dev, coarse="int8")
coarse.add(db)
coarse.matrix_i8()

small, big = min(100_000, N // 4), min(1_000_000, N // 2)
perm = torch.randperm(N, generator=g, device=dev)
subsets = [(f"contiguous {small}", torch.arange(N // 2, N // 2 + small, device=dev)),
           (f"random {small}", perm[:small]),
           (f"random {big}", perm[:big]),
           (f"every second row ({(N + 1) // 2})", torch.arange(0, N, 2, device=dev)),
           (f"all {N} in order", torch.arange(N, device=dev))]
subsets = [(name, exact.subset(rows)) for name, rows in subsets]
del perm
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def timed(calls, q):
    """calls: [search_device-like]; REPS rounds, each round runs every call once (alternating), an event pair around each call
    -> per call [median ms, min, max]"""
    for _ in range(WARM):
        for c in calls:
            c(q, K)
    torch.cuda.synchronize()
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(REPS)] for _ in calls]
    for r in range(REPS):
        for ci, c in enumerate(calls):
            ev[ci][r][0].record()
            c(q, K)
            ev[ci][r][1].record()
    torch.cuda.synchronize()
    out = []
    for per in ev:
        ms = [a.elapsed_time(b) for a, b in per]
        out.append((statistics.median(ms), min(ms), max(ms)))
    return out


def scan_ms(sub, q):
    M, Q = sub.ntotal, q.shape[0]
    ws = torch.empty(L.clipmi_topk_ip_rows_workspace_bytes(M, E, Q, K), dtype=torch.uint8, device=dev)
    os_ = torch.empty((Q, K), dtype=torch.float32, device=dev)
    oi_ = torch.empty((Q, K), dtype=torch.int64, device=dev)
    ms = C.c_float(0)
    clipmi._lib.check(L.clipmi_dbg_topk_rows_scan_ms(db.data_ptr(), N, E, sub._list.data_ptr(), M, q.data_ptr(), Q, K, os_.data_ptr(),
                                                     oi_.data_ptr(), ws.data_ptr(), ws.numel(), None, 5, C.byref(ms)), "rows scan hook")
    return ms.value


say(f"subset_timing: N={N} E={E} K={K}, {REPS} event-timed calls per figure after {WARM} warm-up rounds, median (min .. max) ms; "
    f"{torch.cuda.get_device_name(0)}")
for Q in (1, 32):
    q = torch.randn((Q, E), generator=g, device=dev)
    q /= q.norm(dim=1, keepdim=True)
    say(f"Q = {Q}")
    (c_ms,) = timed([coarse.search_device], q)
    say(f"  int8 coarse search, all rows          : {c_ms[0]:8.3f} ({c_ms[1]:.3f} .. {c_ms[2]:.3f}) ms per call")
    for name, sub in subsets:
        M = sub.ntotal
        e_ms, s_ms = timed([exact.search_device, sub.search_device], q)
        byt = M * E * 4 + M * 4
        say(f"  {name:38s}: {s_ms[0]:8.3f} ({s_ms[1]:.3f} .. {s_ms[2]:.3f}) ms per call, list scan alone {scan_ms(sub, q):.3f} ms, "
            f"{byt / 1e9:.3f} GB = {byt / s_ms[0] / 1e9:.3f} TB/s | clipmi_topk_ip over all rows beside it: {e_ms[0]:.3f} "
            f"({e_ms[1]:.3f} .. {e_ms[2]:.3f}) ms = {N * E * 4 / e_ms[0] / 1e9:.3f} TB/s")
    # the same answers: the M = N list against the unfiltered search
    a, b = exact.search_device(q, K), subsets[-1][1].search_device(q, K)
    say(f"  all rows in order == clipmi_topk_ip bit for bit: {bool(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]))}")
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "a") as f:
    f.write("\n".join(lines) + "\n")
