"""fp16 storage (IndexFlatIP(storage="f16"), clipmi_topk_ip with CLIPMI_F16) at full size against the f32 exact scan of the same
rows (development aid).

N x E unit rows generated on the device from a seed (default 10 M x 512), K = 51, Q = 1, 16 and 32. The f32 index and the fp16
index of the same rows ALTERNATE call by call in one process, so both see the same clocks; every figure is the median of
event-timed calls after warm-up (REPS >= 20 per figure) with min .. max printed - the spread is the margin of any comparison.
Per form: ms per call, the main scan's own time (clipmi_dbg_topk_scan_ms / clipmi_dbg_topk_rows_scan_ms against
clipmi_dbg_topk_scan_f16_ms), bytes and TB/s over the call. Then the same for a 100 k-row and a 1 M-row random subset.
usage: f16_timing.py [N] [E] [--out FILE]   (FILE: default profiles/f16_storage_timing.txt, appended to)"""
import ctypes as C
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import clipmi  # noqa: E402

args = sys.argv[1:]
out_path = os.path.join(ROOT, "profiles", "f16_storage_timing.txt")
if "--out" in args:
    out_path = args[args.index("--out") + 1]
    del args[args.index("--out"):args.index("--out") + 2]
N = int(args[0]) if args else 10_000_000
E = int(args[1]) if len(args) > 1 else 512
K, REPS, WARM = 51, 20, 3
L = clipmi._lib.lib()
dev = torch.device("cuda:0")
g = torch.Generator(device=dev)
g.manual_seed(1)
f32 = clipmi.IndexFlatIP(E, device=dev)
f16 = clipmi.IndexFlatIP(E, device=dev, storage="f16")
db = torch.empty((N, E), dtype=torch.float32, device=dev)
for lo in range(0, N, 1 << 20):
    blk = torch.randn((min(1 << 20, N - lo), E), generator=g, device=dev)
    db[lo:lo + blk.shape[0]] = blk / blk.norm(dim=1, keepdim=True)
    f16.add(db[lo:lo + blk.shape[0]])
f32.add(db)
dbh = f16.matrix_f16()

small, big = min(100_000, N // 4), min(1_000_000, N // 2)
perm = torch.randperm(N, generator=g, device=dev)
subsets = [(f"random {small}", perm[:small]), (f"random {big}", perm[:big])]
subsets = [(name, f32.subset(rows), f16.subset(rows)) for name, rows in subsets]
del perm
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def timed(calls, q):
    """REPS rounds, each round runs every call once (alternating), an event pair around each call -> per call (median, min, max)"""
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


def scan_ms(half, lst, q):
    """the main scan alone: average of 5 through the library's hooks"""
    M, Q = (lst.shape[0] if lst is not None else N), q.shape[0]
    ws = torch.empty(L.clipmi_topk_ip_workspace_bytes(M, E, Q, K), dtype=torch.uint8, device=dev)
    os_ = torch.empty((Q, K), dtype=torch.float32, device=dev)
    oi_ = torch.empty((Q, K), dtype=torch.int64, device=dev)
    ms = C.c_float(0)
    tail = (q.data_ptr(), Q, K, os_.data_ptr(), oi_.data_ptr(), ws.data_ptr(), ws.numel(), None, 5, C.byref(ms))
    if half:
        rc = L.clipmi_dbg_topk_scan_f16_ms(dbh.data_ptr(), N, E, lst.data_ptr() if lst is not None else None, M, *tail)
    elif lst is None:
        rc = L.clipmi_dbg_topk_scan_ms(db.data_ptr(), N, E, *tail)
    else:
        rc = L.clipmi_dbg_topk_rows_scan_ms(db.data_ptr(), N, E, lst.data_ptr(), M, *tail)
    clipmi._lib.check(rc, "scan hook")
    return ms.value


def fmt(t):
    return f"{t[0]:8.3f} ({t[1]:.3f} .. {t[2]:.3f})"


say(f"f16_timing: N={N} E={E} K={K}, {REPS} event-timed calls per figure after {WARM} warm-up rounds, f32 and fp16 alternating call by "
    f"call, median (min .. max) ms; {torch.cuda.get_device_name(0)}")
say(f"fp16 index: {f16.f16_changed} of {N * E} elements changed by the rounding, {dbh.numel() * 2 / 1e9:.2f} GB against {db.numel() * 4 / 1e9:.2f} GB")
for Q in (1, 16, 32):
    q = torch.randn((Q, E), generator=g, device=dev)
    q /= q.norm(dim=1, keepdim=True)
    say(f"Q = {Q}")
    a, b = timed([f32.search_device, f16.search_device], q)
    sa, sb = scan_ms(False, None, q), scan_ms(True, None, q)
    say(f"  all rows, f32 : {fmt(a)} ms per call, main scan alone {sa:.3f} ms, {N * E * 4 / 1e9:.3f} GB = {N * E * 4 / sa / 1e9:.3f} TB/s in the scan")
    say(f"  all rows, fp16: {fmt(b)} ms per call, main scan alone {sb:.3f} ms, {N * E * 2 / 1e9:.3f} GB = {N * E * 2 / sb / 1e9:.3f} TB/s in the scan"
        f" | fp16 / f32: {b[0] / a[0]:.3f} per call, {sb / sa:.3f} scan")
    for name, s32, s16 in subsets:
        M = s32.ntotal
        a, b = timed([s32.search_device, s16.search_device], q)
        sa, sb = scan_ms(False, s32._list, q), scan_ms(True, s16._list, q)
        say(f"  {name:14s}, f32 : {fmt(a)} ms per call, list scan alone {sa:.3f} ms, {(M * E * 4 + M * 4) / 1e9:.3f} GB = "
            f"{(M * E * 4 + M * 4) / sa / 1e9:.3f} TB/s in the scan")
        say(f"  {name:14s}, fp16: {fmt(b)} ms per call, list scan alone {sb:.3f} ms, {(M * E * 2 + M * 4) / 1e9:.3f} GB = "
            f"{(M * E * 2 + M * 4) / sb / 1e9:.3f} TB/s in the scan | fp16 / f32: {b[0] / a[0]:.3f} per call, {sb / sa:.3f} scan")
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "a") as f:
    f.write("\n".join(lines) + "\n")
