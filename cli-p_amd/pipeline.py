"""Host image pipeline for the build side: threaded decode + the CLIP
transform's geometry on the host, pinned staging, asynchronous H2D, encode on the GPU in batches.

Reference per-image sequence (build-index.py:47-51): Image.open -> transform -> unsqueeze(0).to(device)
-> encode_image -> /norm -> .cpu(). Here the same images travel as uint8 [B,3,R,R] (resize / centre
crop / RGB done with Pillow exactly as `transform` does; the /255, -mean, /std tail is fused into the
device patch kernel), B at a time, decode of batch i+1 overlapping the GPU work of batch i.
Failures are per file (build-index.py:55-58): a file that does not decode is reported, not fatal.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch


# the Pillow part of the transform and the kinds of regions (decode_worker.Kind) live beside the worker script
from .decode_worker import (FULL_SIZE, HDR, KIND_BASELINE, KIND_PNG, KIND_PNG_ALPHA, KIND_PNG_INDEX, KIND_PROGRESSIVE, PARSED, PARSED_KINDS, PLAN_INTS,  # noqa: E402,F401
                            REGION_TAGS, WANTED_TAG, load_uint8)


class DecodePool:
    """Worker PROCESSES for the Pillow part of the transform (decode_worker.py): decode throughput that scales with
    the host cores also for small images, where threads are bound by the GIL. The workers are plain `python
    decode_worker.py` children started HERE - create the pool BEFORE the process initialises the GPU (indexer.main
    does): a process that has touched the GPU should not spawn programs on this platform. Pixels come back through
    shared memory (workers write their slots; no pickling, no copies through pipes): two segments used in turn, so that
    a batch can be decoded while the previous one is still being copied out."""

    def __init__(self, workers):
        import os
        import subprocess
        import sys
        self.n = max(1, int(workers))
        script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "decode_worker.py")
        # own session: a Ctrl-C at the terminal reaches the ranks (which finish their round: indexer.StopFlag), not the
        # workers - a worker that exited on SIGINT used to turn its current file into a "failed" file that was then
        # written to skip_db and never retried. The workers also ignore SIGINT themselves and leave at EOF on stdin.
        import signal
        import threading
        restore = None
        if threading.current_thread() is threading.main_thread():
            restore = signal.signal(signal.SIGINT, signal.SIG_IGN)      # inherited across exec: ignored from the first instruction
        try:
            self.procs = [subprocess.Popen([sys.executable, script], stdin=subprocess.PIPE, stdout=subprocess.PIPE,
                                           start_new_session=True)
                          for _ in range(self.n)]
        finally:
            if restore is not None:
                signal.signal(signal.SIGINT, restore)
        self.lost = set()           # files a worker DIED on: failed for this run, but not proven undecodable (never skip_db)
        self._all_procs = list(self.procs)
        self.threads = ThreadPoolExecutor(max_workers=self.n)
        self.segs = [None, None, None, None]      # 0, 1: the n_px x n_px slots of two batches in turn; 2, 3: their full-size regions
        self.jpeg_wanted = 0                      # largest region a JPEG file asked for and did not get (encode_files sizes by it)
        self.jpeg_cap_hint = 0                    # the region size the last encode_files call ended with

    def _segment(self, nbytes, which=0):
        from multiprocessing import shared_memory
        seg = self.segs[which]
        if seg is None or seg.size < nbytes:
            self._drop_segment(which)
            seg = self.segs[which] = shared_memory.SharedMemory(create=True, size=int(nbytes))
        return seg

    @staticmethod
    def shm_room():
        """Bytes of /dev/shm THIS process may count on for its segments (/dev/shm is a tmpfs whose pages exist only once
        written: a segment larger than what is free is created without complaint and kills the writer later; containers
        default to 64 MB). The ranks of one node all see the same free space before any of them has written a page, so
        each takes its share: free / LOCAL_WORLD_SIZE."""
        import os
        try:
            st = os.statvfs("/dev/shm")
            return st.f_bavail * st.f_frsize // max(1, int(os.environ.get("LOCAL_WORLD_SIZE", "1")))
        except (OSError, ValueError):
            return 0

    def pin_segment(self, which):
        """Page-lock segment `which` for the GPU (hipHostRegister through torch's runtime handle) so that it can be copied
        to the device where it lies - no packing copy in this process. True when it is (already) locked."""
        seg = self.segs[which]
        if seg is None:
            return False
        reg = self.__dict__.setdefault("_pinned", {})
        if reg.get(which) == seg.name:
            return True
        try:
            import ctypes
            addr = ctypes.addressof(ctypes.c_char.from_buffer(seg.buf))
            rc = torch.cuda.cudart().cudaHostRegister(addr, seg.size, 0)
            ok = int(rc) == 0
        except Exception:
            ok = False
        if ok:
            reg[which] = seg.name
            self.__dict__.setdefault("_pinned_addr", {})[which] = addr
        return ok

    def _unpin_segment(self, which):
        reg = self.__dict__.get("_pinned", {})
        if which in reg:
            try:
                torch.cuda.cudart().cudaHostUnregister(self._pinned_addr[which])
            except Exception:
                pass
            reg.pop(which, None)

    def _drop_segment(self, which):
        """Unlink first (always possible), then unmap (refused while a caller still holds a view: the mapping then goes
        with the last reference)."""
        seg = self.segs[which]
        if seg is None:
            return
        self._unpin_segment(which)
        try:
            seg.unlink()
        except Exception:
            pass
        try:
            seg.close()
        except BufferError:
            seg.close = lambda: None          # a view is still alive: the mapping goes with it; keep __del__ quiet
        self.segs[which] = None

    def _run(self, w, jobs, n_px, name, seg, big=None):
        """Worker w decodes its share of the batch: (slot, path) pairs -> (slot, status) with status False (failed), True
        (the transform's pixels are in the slot) or (kind, w, h, bytes): the image is in its region of the big segment, as one
        of decode_worker's FULL_SIZE and PARSED kinds. If the worker process dies (a file that crashes the decoder, an OOM kill), that
        file is reported as failed and the rest of the share - and of every later batch - is decoded in this process: no
        program is spawned once the GPU may have been initialised."""
        import struct
        p = self.procs[w]
        ok = []
        per = 3 * n_px * n_px
        bname, bcap, bmode = (big[0], big[1], big[2]) if big else (b"-", 0, 0)
        if p is not None:
            # the whole share in one write: this thread sleeps in read() while the worker decodes (one request per round
            # trip kept 16 parent threads busy handing the GIL around)
            # the path travels hex-encoded: a file name may hold '\n' or '\t' (legal on Linux, and os.listdir returns them) -
            # raw, such a name split into two request lines and shifted every later reply of the worker by one
            req = b"".join(b"%d\t%s\t%d\t%s\t%d\t%d\t%d\t" % (n_px, name, slot * per, bname, slot * bcap, bcap, bmode) +
                           path.encode("utf-8", "surrogateescape").hex().encode() + b"\n" for slot, path in jobs)
            try:
                p.stdin.write(req)
                p.stdin.flush()
                # one read for the whole share: the worker answers every file with a 17-byte record (status + <iiq), and a
                # short read means it died - the number of whole records says on which file (a read per file kept the 16
                # parent threads handing the GIL around: 5 ms per 435-image batch)
                raw = p.stdout.read(17 * len(jobs))
                for k in range(len(raw) // 17):
                    st = raw[17 * k:17 * k + 1]
                    if st in REGION_TAGS:
                        ok.append((jobs[k][0], (int(st),) + struct.unpack_from("<iiq", raw, 17 * k + 1)))
                    elif st == WANTED_TAG:                 # Pillow decoded it; a larger region would have taken the file itself
                        self.jpeg_wanted = max(self.jpeg_wanted, struct.unpack_from("<iiq", raw, 17 * k + 1)[2])
                        ok.append((jobs[k][0], True))
                    else:
                        ok.append((jobs[k][0], st == b"1"))
            except (BrokenPipeError, OSError):
                pass
            if len(ok) < len(jobs):                # the worker died on file len(ok): that one failed, the rest in-process
                self.procs[w] = None
                self.lost.add(jobs[len(ok)][1])    # ... for this run only: the caller must not record it as undecodable
                ok.append((jobs[len(ok)][0], False))
        for slot, path in jobs[len(ok):]:
            try:
                load_uint8(path, n_px, out=np.frombuffer(seg.buf, dtype=np.uint8, count=per, offset=slot * per).reshape(3, n_px, n_px))
                ok.append((slot, True))
            except KeyboardInterrupt:
                raise
            except Exception:
                ok.append((slot, False))
        return ok

    def decode(self, paths, n_px, copy=True, segment=0, full_cap=0, full_mode=1):
        """-> (uint8 array [n_ok,3,n_px,n_px], ok_paths, failed_paths), file order kept. copy=False returns a VIEW of
        the pool's shared-memory segment `segment` (all slots, plus a boolean mask of the good ones instead of the
        compacted array): valid until the next decode() into the same segment - encode_files copies it straight into
        pinned memory. One decode() at a time (the workers take one request stream).
        full_cap > 0 (with copy=False): 8-bit RGB images that need resampling and fit full_cap bytes are delivered at FULL
        size in a second segment, one region of full_cap bytes per slot (tmpfs pages exist only where written), for the
        resize on the device; the result is then ((slots view, good mask, big view, {slot: (kind, w, h, bytes)}), ok, bad).
        full_mode: what a region may take - the bits of decode_worker's FULL_SIZE and PARSED kinds."""
        n = len(paths)
        per = 3 * n_px * n_px
        seg = self._segment(max(1, n * per), segment)
        name = seg.name.encode()
        big = bseg = None
        if full_cap > 0 and not copy:
            full_cap = (int(full_cap) + 15) // 16 * 16
            bseg = self._segment(max(1, n * full_cap), 2 + segment)
            big = (bseg.name.encode(), full_cap, int(full_mode))
        live = [w for w in range(self.n) if self.procs[w] is not None] or [0]
        futs = [self.threads.submit(self._run, w, [(i, paths[i]) for i in range(k, n, len(live))], n_px, name, seg, big)
                for k, w in enumerate(live) if k < n]
        good = np.zeros(n, dtype=bool)
        full = {}
        for f in futs:
            for slot, st in f.result():
                good[slot] = bool(st)
                if isinstance(st, tuple):
                    full[slot] = st
        arr = np.frombuffer(seg.buf, dtype=np.uint8, count=n * per).reshape(n, 3, n_px, n_px)
        ok = [p for p, g_ in zip(paths, good) if g_]
        bad = [p for p, g_ in zip(paths, good) if not g_]
        if not copy:
            if big is not None:
                return (arr, good, np.frombuffer(bseg.buf, dtype=np.uint8, count=n * full_cap), full), ok, bad
            return (arr, good), ok, bad
        out = arr[good].copy() if not good.all() else arr.copy()
        return out, ok, bad

    def close(self):
        procs = [p for p in getattr(self, "_all_procs", self.procs) if p is not None]
        for p in procs:
            try:
                p.stdin.close()
            except Exception:
                pass
        for p in procs:
            try:
                p.wait(timeout=5)
            except Exception:
                p.kill()
        self.threads.shutdown(wait=False)
        for which in range(4):
            self._drop_segment(which)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def _load_safe(args):
    path, n_px = args
    try:
        return load_uint8(path, n_px)
    except KeyboardInterrupt:
        raise
    except Exception:
        return None


def _headers(bigview, n, cap, slots):
    """The region headers (decode_worker.HDR) of `slots` as int64 [len(slots)][JPEG_HDR_INTS]: one strided gather out of the
    segment (uint8, n regions of cap bytes)"""
    from .decode_worker import JPEG_HDR_INTS
    hd = np.lib.stride_tricks.as_strided(bigview[:4 * JPEG_HDR_INTS].view(np.int32), shape=(n, JPEG_HDR_INTS), strides=(cap, 4))
    return hd[slots].astype(np.int64)


def _resize_jobs(src_off, w, h, plan, n_hcoef, hcoef_off, out_index, n_px, px=3):
    """clipmi_resize_job records. plan: [n][8] r0 nrows need_h need_v left top hk vk (HDR.PLAN); hcoef_off: where each image's
    horizontal coefficient block starts, in ints from the segment's start - the vertical block follows it; the rows the
    vertical pass leaves for the horizontal one lie back to back in the scratch buffer (tmp_off), px bytes a pixel."""
    from .resize import JOB
    jobs = np.zeros(len(w), dtype=JOB)
    jobs["src_off"], jobs["w"], jobs["h"], jobs["out_index"] = src_off, w, h, out_index
    for k, f in enumerate(("r0", "nrows", "need_h", "need_v", "left", "top", "hk", "vk")):
        jobs[f] = plan[:, k]
    jobs["hcoef_off"] = hcoef_off
    jobs["vcoef_off"] = jobs["hcoef_off"] + n_hcoef
    tmp = plan[:, 1] * n_px * px
    jobs["tmp_off"] = np.cumsum(tmp) - tmp
    return jobs


def _decoded_jobs(hd, cap, slots, comp, n_px, px=3):
    """-> (the transform's jobs for parsed files whose decoded rows, px bytes a pixel, lie back to back, 16-byte aligned, in the
    decoder's output: the order of `slots`; their offsets there; their sizes). px 3 and 4: clipmi_resize_job records; px 1 (index
    rows): clipmi_nearest_job records that point at the palette and the two tables in the file's region."""
    w, h = hd[:, HDR.W], hd[:, HDR.H]
    out_sz = (w * h * px + 15) // 16 * 16
    out_off = np.cumsum(out_sz) - out_sz
    if px == 1:
        from .decode_worker import JPEG_TABLES_OFF
        from .resize import NEAREST_JOB
        jobs = np.zeros(len(w), dtype=NEAREST_JOB)
        jobs["src_off"], jobs["w"], jobs["h"], jobs["out_index"] = out_off, w, h, np.asarray(comp)[slots]
        jobs["pal_off"] = slots * cap + JPEG_TABLES_OFF
        jobs["col_off"] = (slots * cap + hd[:, HDR.COEF_OFF]) // 4
        jobs["row_off"] = jobs["col_off"] + hd[:, HDR.N_HCOEF]
        return jobs, out_off, out_sz
    jobs = _resize_jobs(out_off, w, h, hd[:, HDR.PLAN], hd[:, HDR.N_HCOEF], (slots * cap + hd[:, HDR.COEF_OFF]) // 4,
                        np.asarray(comp)[slots], n_px, px)
    return jobs, out_off, out_sz


def jpeg_records(bigview, n, cap, slots, comp, n_px):
    """The device decoder's records out of a batch's regions of the big segment (decode_worker.stage_jpeg wrote them): every field
    comes out of the regions' headers as one strided numpy gather - no Python per image except the table-set look-up.
    bigview: the segment (uint8, n regions of cap bytes); slots: the regions that hold a parsed JPEG file; comp: slot -> row of the
    batch's tensor. -> (clipmi_jpeg_image records with offsets into the segment, distinct raw Huffman tables uint8, clipmi_resize_job
    records whose sources are the decoder's outputs laid out back to back, output bytes per image, blocks per image, number of tables)"""
    from . import jpeg as J
    from .decode_worker import JPEG_QUANT_OFF, JPEG_TABLES_OFF
    slots = np.asarray(slots, dtype=np.int64)
    n3 = len(slots)
    st = np.lib.stride_tricks.as_strided
    hd = _headers(bigview, n, cap, slots)
    jobs, out_off, out_sz = _decoded_jobs(hd, cap, slots, comp, n_px)
    blocks = hd[:, HDR.BLOCKS]
    recs = np.zeros(n3, dtype=J.IMAGE)
    recs["stream_off"], recs["coef_off"], recs["out_off"] = slots * cap + hd[:, HDR.DATA_OFF], np.cumsum(blocks) - blocks, out_off
    recs["stream_bytes"], recs["width"], recs["height"] = hd[:, HDR.COUNT], hd[:, HDR.W], hd[:, HDR.H]
    recs["ncomp"], recs["hs"], recs["vs"] = hd[:, HDR.NCOMP], hd[:, HDR.HS], hd[:, HDR.VS]
    recs["restart_interval"], recs["n_intervals"] = hd[:, HDR.RESTART_INTERVAL], hd[:, HDR.N_INTERVALS]
    recs["intervals_off"], recs["stuffed"] = slots * cap + hd[:, HDR.INTERVALS_OFF], hd[:, HDR.STUFFED]
    recs["quant"] = st(bigview[JPEG_QUANT_OFF:], shape=(n, 192), strides=(cap, 1))[slots].reshape(n3, 3, 64)
    # the Huffman tables: distinct six-table sets first (files of one encoder share theirs), then distinct tables
    tabs = st(bigview[JPEG_TABLES_OFF:], shape=(n, 6 * J.TABLE_BYTES), strides=(cap, 1))[slots]
    sets, pool_t, set_idx = {}, {}, np.zeros((n3, 6), np.int32)
    for k in range(n3):
        key = tabs[k].tobytes()
        idx = sets.get(key)
        if idx is None:
            idx = sets[key] = [pool_t.setdefault(key[t * J.TABLE_BYTES:(t + 1) * J.TABLE_BYTES], len(pool_t)) for t in range(6)]
        set_idx[k] = idx
    recs["dc_tbl"], recs["ac_tbl"] = set_idx[:, 0::2], set_idx[:, 1::2]
    tables = np.frombuffer(b"".join(pool_t), np.uint8)
    return recs, tables, jobs, out_sz, blocks, len(pool_t)


def progressive_records(bigview, n, cap, slots, comp, n_px):
    """jpeg_records for progressive files (decode_worker.stage_jpeg_progressive wrote the regions). -> (clipmi_jpeg_progressive_image
    records, clipmi_jpeg_scan records with offsets into the segment, distinct raw Huffman tables uint8, clipmi_resize_job records
    whose sources are the decoder's outputs laid out back to back, output bytes per image, blocks per image, number of tables)"""
    from . import jpeg as J
    from .decode_worker import JPEG_QUANT_OFF, PROG_SCAN_BYTES
    slots = np.asarray(slots, dtype=np.int64)
    n4 = len(slots)
    hd = _headers(bigview, n, cap, slots)
    jobs, out_off, out_sz = _decoded_jobs(hd, cap, slots, comp, n_px)
    nscans, blocks = hd[:, HDR.COUNT], hd[:, HDR.BLOCKS]
    recs = np.zeros(n4, dtype=J.PIMAGE)
    recs["coef_off"], recs["out_off"], recs["width"], recs["height"] = np.cumsum(blocks) - blocks, out_off, hd[:, HDR.W], hd[:, HDR.H]
    recs["ncomp"], recs["hs"], recs["vs"] = hd[:, HDR.NCOMP], hd[:, HDR.HS], hd[:, HDR.VS]
    recs["first_scan"], recs["n_scans"] = np.cumsum(nscans) - nscans, nscans
    recs["quant"] = np.lib.stride_tricks.as_strided(bigview[JPEG_QUANT_OFF:], shape=(n, 192), strides=(cap, 1))[slots].reshape(n4, 3, 64)
    scans = np.zeros(int(nscans.sum()), dtype=J.SCAN)
    pool_t = {}
    for k in range(n4):
        base = int(slots[k]) * cap
        o_scans, o_tab, nt = int(hd[k, HDR.DATA_OFF]), int(hd[k, HDR.TABLES_OFF]), int(hd[k, HDR.N_TABLES])
        local = bigview[base + o_scans:base + o_scans + PROG_SCAN_BYTES * int(nscans[k])].copy().view(J.SCAN)
        remap = np.array([pool_t.setdefault(bigview[base + o_tab + t * J.TABLE_BYTES:base + o_tab + (t + 1) * J.TABLE_BYTES].tobytes(),
                                            len(pool_t)) for t in range(nt)] + [-1], dtype=np.int32)
        local["stream_off"] += base
        local["tbl"] = remap[np.where(local["tbl"] >= 0, local["tbl"], nt)]
        f = int(recs["first_scan"][k])
        scans[f:f + len(local)] = local
    tables = np.frombuffer(b"".join(pool_t), np.uint8)
    return recs, scans, tables, jobs, out_sz, blocks, len(pool_t)


def png_records(bigview, n, cap, slots, comp, n_px):
    """jpeg_records for PNG files (decode_worker.stage_png wrote the regions). -> (clipmi_png_image records with stream offsets into
    the segment and the scanline and output buffers laid out back to back, clipmi_resize_job records whose sources are the decoder's
    outputs, output bytes per image, scanline bytes per image, each rounded up to 16)"""
    from . import png as P
    slots = np.asarray(slots, dtype=np.int64)
    hd = _headers(bigview, n, cap, slots)
    jobs, out_off, out_sz = _decoded_jobs(hd, cap, slots, comp, n_px)
    w, h, ch = hd[:, HDR.W], hd[:, HDR.H], hd[:, HDR.NCOMP]
    recs = np.zeros(len(slots), dtype=P.IMAGE)
    raw_sz = (h * (1 + w * ch) + 15) // 16 * 16
    recs["stream_off"], recs["raw_off"], recs["out_off"] = slots * cap + hd[:, HDR.DATA_OFF], np.cumsum(raw_sz) - raw_sz, out_off
    recs["stream_bytes"], recs["width"], recs["height"], recs["channels"] = hd[:, HDR.COUNT], w, h, ch
    return recs, jobs, out_sz, raw_sz


def _png_mode_records(px):
    """png_records for the files of one of png_parse's other kinds (decode_worker.stage_png(modes=True) wrote the regions): px bytes
    per decoded pixel - 4 "alpha", 1 "index"; the records carry colour type, depth and palette entries for clipmi_png_decode_px8"""
    def records(bigview, n, cap, slots, comp, n_px):
        from . import png as P
        slots = np.asarray(slots, dtype=np.int64)
        hd = _headers(bigview, n, cap, slots)
        jobs, out_off, out_sz = _decoded_jobs(hd, cap, slots, comp, n_px, px)
        w, h, ch, depth = hd[:, HDR.W], hd[:, HDR.H], hd[:, HDR.NCOMP], hd[:, HDR.DEPTH]
        recs = np.zeros(len(slots), dtype=P.IMAGE)
        raw_sz = (h * (1 + (w * ch * depth + 7) // 8) + 15) // 16 * 16
        recs["stream_off"], recs["raw_off"], recs["out_off"] = slots * cap + hd[:, HDR.DATA_OFF], np.cumsum(raw_sz) - raw_sz, out_off
        recs["stream_bytes"], recs["width"], recs["height"], recs["channels"] = hd[:, HDR.COUNT], w, h, ch
        recs["reserved"] = np.stack([hd[:, HDR.CTYPE] << 8 | depth, hd[:, HDR.ENTRIES]], axis=1)
        return recs, jobs, out_sz, raw_sz
    return records


def _groups(need, budget):
    """[lo, hi) ranges of consecutive files whose `need` sums stay within the budget: a group closes when the next file would
    exceed it, and a file above the budget is a group of its own. No files, no group."""
    groups, lo, acc = [], 0, 0
    for k in range(len(need)):
        if k > lo and acc + need[k] > budget:
            groups.append((lo, k))
            lo, acc = k, 0
        acc += int(need[k])
    return groups + [(lo, len(need))] if len(need) else groups


def _pack16(arrays):
    """Arrays -> (one uint8 buffer that holds their bytes at 16-byte-aligned offsets, the offsets)"""
    offs, end = [], 0
    for a in arrays:
        offs.append((end + 15) // 16 * 16)
        end = offs[-1] + a.nbytes
    buf = np.zeros(end, np.uint8)
    for a, o in zip(arrays, offs):
        buf[o:o + a.nbytes] = a.view(np.uint8).reshape(-1)
    return buf, offs


def _baseline_group(L, r):
    recs, tables, jobs, out_sz, blocks, nt = r
    total, most, pixels = int(blocks.sum()), int(blocks.max()), int((recs["width"].astype(np.int64) * recs["height"]).max())
    ws_bytes = int(L.clipmi_jpeg_workspace_bytes(total, nt))
    return [recs, tables, jobs], out_sz, ws_bytes, "clipmi_jpeg_decode_rgb8", lambda base, sb, offs, rgb, status, ws, stream: (
        L.clipmi_jpeg_decode_rgb8(base, sb, len(recs), sb + offs[1], nt, total, most, pixels, rgb, status, ws, ws_bytes, stream))


def _progressive_group(L, r):
    recs, scans, tables, jobs, out_sz, blocks, nt = r
    total, most, pixels = int(blocks.sum()), int(blocks.max()), int((recs["width"].astype(np.int64) * recs["height"]).max())
    ws_bytes = int(L.clipmi_jpeg_progressive_workspace_bytes(len(recs), total, nt))
    return [recs, scans, tables, jobs], out_sz, ws_bytes, "clipmi_jpeg_decode_progressive_rgb8", (
        lambda base, sb, offs, rgb, status, ws, stream: L.clipmi_jpeg_decode_progressive_rgb8(
            base, sb, len(recs), sb + offs[1], len(scans), sb + offs[2], nt, total, most, pixels, rgb, status, ws, ws_bytes, stream))


def _baseline_fused_group(L, r):
    """_baseline_group for clipmi_jpeg_decode_transform_rgb8: the call also takes tr = (the group's largest nrows, n_px, the batch's
    tensor, the scratch rows) and no RGB rows; the jobs' coefficient offsets count from the segment's start, as for the resize entry"""
    recs, tables, jobs, out_sz, blocks, nt = r
    total, most = int(blocks.sum()), int(blocks.max())
    ws_bytes = int(L.clipmi_jpeg_workspace_bytes(total, nt))
    return [recs, tables, jobs], out_sz, ws_bytes, "clipmi_jpeg_decode_transform_rgb8", lambda base, sb, offs, rgb, status, ws, stream, tr: (
        L.clipmi_jpeg_decode_transform_rgb8(base, sb, len(recs), sb + offs[1], nt, total, most, sb + offs[2], tr[0], base, tr[1], tr[2],
                                            tr[3], status, ws, ws_bytes, stream))


def _progressive_fused_group(L, r):
    recs, scans, tables, jobs, out_sz, blocks, nt = r
    total, most = int(blocks.sum()), int(blocks.max())
    ws_bytes = int(L.clipmi_jpeg_progressive_workspace_bytes(len(recs), total, nt))
    return [recs, scans, tables, jobs], out_sz, ws_bytes, "clipmi_jpeg_decode_progressive_transform_rgb8", (
        lambda base, sb, offs, rgb, status, ws, stream, tr: L.clipmi_jpeg_decode_progressive_transform_rgb8(
            base, sb, len(recs), sb + offs[1], len(scans), sb + offs[2], nt, total, most, sb + offs[3], tr[0], base, tr[1], tr[2], tr[3],
            status, ws, ws_bytes, stream))


def _png_group(L, r):
    recs, jobs, out_sz, raw_sz = r
    total, most = int(raw_sz.sum()), int(raw_sz.max())
    ws_bytes = int(L.clipmi_png_workspace_bytes(len(recs), total))
    return [recs, jobs], out_sz, ws_bytes, "clipmi_png_decode_rgb8", lambda base, sb, offs, rgb, status, ws, stream: (
        L.clipmi_png_decode_rgb8(base, sb, len(recs), total, most, rgb, status, ws, ws_bytes, stream))


def _png_mode_group(L, r):
    recs, jobs, out_sz, raw_sz = r
    total, most = int(raw_sz.sum()), int(raw_sz.max())
    ws_bytes = int(L.clipmi_png_px8_workspace_bytes(len(recs), total))
    return [recs, jobs], out_sz, ws_bytes, "clipmi_png_decode_px8", lambda base, sb, offs, rgb, status, ws, stream: (
        L.clipmi_png_decode_px8(base, sb, len(recs), total, most, rgb, status, ws, ws_bytes, stream))


# What differs between the parsed kinds in device_stage, by decode_worker.Kind.kind:
#   the records function |
#   the bytes of HBM a file's decoder needs beside its RGB rows and the resize's rows, out of the headers (coefficients; scanlines) |
#   (library, what the records function returned) -> (the arrays that travel to the device, 16-byte aligned in this order, the
#   resize jobs last; output bytes per image; workspace bytes; the decode entry's name; its call, given where things lie) |
#   the bytes per decoded pixel | the transform entry that takes them (clipmi_nearest_crop_p8 needs no scratch rows)
def _png_mode_scanlines(hd):
    return hd[:, HDR.H] * (1 + (hd[:, HDR.W] * hd[:, HDR.NCOMP] * hd[:, HDR.DEPTH] + 7) // 8)


_FORMATS = {KIND_BASELINE: (jpeg_records, lambda hd: hd[:, HDR.BLOCKS] * 192, _baseline_group, 3, "clipmi_resize_crop_rgb8"),
            KIND_PROGRESSIVE: (progressive_records, lambda hd: hd[:, HDR.BLOCKS] * 192, _progressive_group, 3, "clipmi_resize_crop_rgb8"),
            KIND_PNG: (png_records, lambda hd: hd[:, HDR.H] * (1 + hd[:, HDR.W] * hd[:, HDR.NCOMP]), _png_group, 3,
                       "clipmi_resize_crop_rgb8"),
            KIND_PNG_ALPHA: (_png_mode_records(4), _png_mode_scanlines, _png_mode_group, 4, "clipmi_resize_crop_rgba8"),
            KIND_PNG_INDEX: (_png_mode_records(1), _png_mode_scanlines, _png_mode_group, 1, "clipmi_nearest_crop_p8")}


# With jpeg_fused the two JPEG kinds go through the entries that decode and transform in one call (transform entry None: the
# decode entry's call did it): no full-size RGB rows exist for them.
_FUSED_FORMATS = {KIND_BASELINE: _FORMATS[KIND_BASELINE][:2] + (_baseline_fused_group, 3, None),
                  KIND_PROGRESSIVE: _FORMATS[KIND_PROGRESSIVE][:2] + (_progressive_fused_group, 3, None)}


def formats(jpeg_fused=False):
    """_FORMATS, with the fused rows in place of the two JPEG kinds' when jpeg_fused"""
    return {**_FORMATS, **_FUSED_FORMATS} if jpeg_fused else _FORMATS


def jpeg_fused_default():
    """$CLIPMI_DEVICE_JPEG_FUSED ("1" = on), off when unset"""
    import os
    return os.environ.get("CLIPMI_DEVICE_JPEG_FUSED", "0") not in ("", "0")


def file_need(hd, fmt, n_px):
    """Bytes of HBM each file of one kind needs while its group is decoded, out of the region headers hd ([n][JPEG_HDR_INTS]) and the
    kind's row fmt of formats(): what its decoder needs, its full-size decoded rows (none where the decode entry transforms too)
    and the rows between the resize's two passes. device_stage sizes its groups by it."""
    records, decoder_bytes, group, px, entry = fmt
    tmp_px = 0 if entry == "clipmi_nearest_crop_p8" else px      # scratch bytes per pixel of the rows between the passes
    rows = 0 if entry is None else (hd[:, HDR.W] * hd[:, HDR.H] * px + 15) // 16 * 16
    return decoder_bytes(hd) + rows + hd[:, HDR.NROWS] * n_px * tmp_px


def encode_files(model, paths, batch=256, workers=8, pool=None, device_resize_mb=None, device_jpeg_kb=None, stats=None,
                 jpeg_group_mb=32768, device_progressive=None, device_png=None, device_png_modes=None, jpeg_fused=None):
    """Generator over batches: yields (ok_paths, features f32 [n,E] numpy normalised, failed_paths).
    Decode runs in the worker processes of `pool` (a DecodePool) when given, else on `workers` threads (Pillow
    releases the GIL while decoding, which is enough for large photos and not for small images).
    device_resize_mb (default $CLIPMI_DEVICE_RESIZE_MB, 0 = off; needs `pool` and a GPU): 8-bit RGB images of up to that
    many MB decoded travel at full size and are resized + cropped by clipmi_resize_crop_rgb8 - the same pixels, with the
    workers left to decode only (Pillow's bicubic resize is half of a photo-sized file's host time).
    device_jpeg_kb (default $CLIPMI_DEVICE_JPEG_KB, else 8192; 0 = off; needs `pool` and a GPU): baseline JPEG files of up to that
    many KB are not decoded on the host at all - a worker reads the file, walks its markers and removes the byte stuffing
    (jpeg_parse.py), and clipmi_jpeg_decode_rgb8 + clipmi_resize_crop_rgb8 produce the transform's pixels in HBM, the same
    bytes as Pillow's. Every other file (progressive, PNG, CMYK ...) and every file the device reports corrupt takes the
    Pillow path as before.
    device_progressive (default $CLIPMI_DEVICE_PROGRESSIVE, else off; "1" = on; needs the JPEG decode on the device above):
    progressive JPEG files take the device too (jpeg_parse.parse_progressive in the workers, clipmi_jpeg_decode_progressive_rgb8
    + clipmi_resize_crop_rgb8 beside the baseline decode), the same bytes as Pillow's; files it reports go back to Pillow.
    device_png (default $CLIPMI_DEVICE_PNG, else off; "1" = on; needs the JPEG decode on the device above, whose regions it
    shares): 8-bit grey and RGB PNG files that are not interlaced and hold at most decode_worker.PNG_MAX_RAW (16 MiB) of
    scanlines take the device too (png_parse.parse in the workers,
    clipmi_png_decode_rgb8 + clipmi_resize_crop_rgb8 on the side stream beside the JPEG decodes, grouped under jpeg_group_mb
    like them), the same bytes as Pillow's; every other PNG file and every file the device reports goes back to Pillow. With
    the flag off nothing changes for any file.
    device_png_modes (default $CLIPMI_DEVICE_PNG_MODES, else off; "1" = on; takes effect only with device_png on): RGBA, grey +
    alpha, palette (depth 1/2/4/8, with or without tRNS) and grey depth 1/2/4 files that are not interlaced take the device as
    well (png_parse.parse(modes=True), clipmi_png_decode_px8, then clipmi_resize_crop_rgba8 or clipmi_nearest_crop_p8: Pillow
    resamples such files in their own mode), the same bytes as Pillow's. Off, such files stay with Pillow as before.
    jpeg_fused (default $CLIPMI_DEVICE_JPEG_FUSED, else off; "1" = on): baseline and progressive files on the device go through
    clipmi_jpeg_decode_transform_rgb8 / clipmi_jpeg_decode_progressive_transform_rgb8, which convert and resample straight from
    the decoder's sample planes: the same bytes, and no full-size RGB rows (3 bytes per pixel) in HBM, so that a group under
    jpeg_group_mb holds more files. Off, nothing changes for any file.
    jpeg_group_mb: the device decodes a batch's JPEG files in groups whose decoded form (~22 bytes per pixel) stays under that
    many MB of HBM - one group for a batch of thumbnails, several for a batch of photos.
    stats: a dict that receives the seconds each of the three pipelined stages was busy (decode_s: worker processes, copy_s:
    shared memory -> device incl. the decode / resize kernels, encode_s) and the files that took the device decoders, under the
    keys of decode_worker.PARSED (jpeg_files, jpeg_progressive_files: files staged for the device; png_files: files it decoded and
    did not hand back; png_mode_files: the same for the files device_png_modes adds - png_files keeps counting grey / RGB only)."""
    import os
    import time
    n_px = model.visual.input_resolution
    dev = model.device
    use_gpu = dev.type == "cuda"
    copy_stream = None
    if use_gpu:
        from . import _lib as _l
        copy_stream = _l.copy_stream(dev)
    if device_resize_mb is None:
        device_resize_mb = float(os.environ.get("CLIPMI_DEVICE_RESIZE_MB", "0"))
    if pool is not None and pool.shm_room() < 2 * batch * 3 * n_px * n_px + (64 << 20):
        print(f"(shared memory too small for decode workers' batches: {pool.shm_room() >> 20} MB free in /dev/shm; "
              f"decoding on {workers} threads)")
        pool = None
    if device_jpeg_kb is None:
        device_jpeg_kb = float(os.environ.get("CLIPMI_DEVICE_JPEG_KB", "8192"))
    on_device = use_gpu and pool is not None
    resize_cap = int(device_resize_mb * (1 << 20)) if on_device else 0
    jpeg_cap = int(device_jpeg_kb * 1024) if on_device else 0
    jpeg_group_bytes = int(jpeg_group_mb) << 20

    def room_for(cap):
        return pool.shm_room() >= 2 * batch * (3 * n_px * n_px + cap) + (256 << 20)

    if resize_cap and not room_for(resize_cap):
        resize_cap = 0
    if jpeg_cap:
        # the largest region /dev/shm has room for (two segments of `batch` regions beside the n_px slots), found once per pool:
        # regions start small and grow with the files, so a large configured size costs nothing until files of that size come
        if not getattr(pool, "jpeg_fit_cap", 0):
            room = pool.shm_room() - 2 * batch * 3 * n_px * n_px - (256 << 20)
            pool.jpeg_fit_cap = max(1, room // (2 * batch) // 65536 * 65536)
        jpeg_cap = min(jpeg_cap, pool.jpeg_fit_cap)
        if jpeg_cap < (64 << 10):
            jpeg_cap = 0
    # regions are copied to the device whole, so JPEG regions start small (or where the pool's last call ended) and follow the
    # files: a file that does not fit is decoded by Pillow this once and says what it would have needed (DecodePool.jpeg_wanted)
    jpeg_now = min(jpeg_cap, pool.jpeg_cap_hint or (128 << 10)) if jpeg_cap else 0
    full_cap = [max(resize_cap, jpeg_now)]               # bytes per region of the big segment; [0]: mutable (may be switched off)
    if device_progressive is None:
        device_progressive = os.environ.get("CLIPMI_DEVICE_PROGRESSIVE", "0") not in ("", "0")
    if device_png is None:
        device_png = os.environ.get("CLIPMI_DEVICE_PNG", "0") not in ("", "0")
    if device_png_modes is None:
        device_png_modes = os.environ.get("CLIPMI_DEVICE_PNG_MODES", "0") not in ("", "0")
    if jpeg_fused is None:
        jpeg_fused = jpeg_fused_default()
    kind_formats = formats(jpeg_fused)
    full_mode = ((1 if resize_cap else 0) | (2 if jpeg_cap else 0) | (4 if jpeg_cap and device_progressive else 0) |
                 (8 if jpeg_cap and device_png else 0) | (16 if jpeg_cap and device_png and device_png_modes else 0))

    # three pinned staging buffers used in turn (GPU): batch i may still be in its H2D copy while batch i+1 is filled;
    # a buffer is reused only after the copy that read it has finished. Pixels go shared memory -> pinned -> device:
    # ONE host copy (the first version copied out of the segment, then again into freshly pinned memory: 55 ms per
    # 435-image batch against 23 ms of decode on 16 workers).
    ring = []

    def staging(n):
        slot = ring.pop(0) if len(ring) >= 3 else {"buf": None, "ev": None}
        if slot["ev"] is not None:
            slot["ev"].synchronize()
        if slot["buf"] is None or slot["buf"].shape[0] < n:
            slot["buf"] = torch.empty((max(n, batch), 3, n_px, n_px), dtype=torch.uint8).pin_memory()
            slot["np"] = slot["buf"].numpy()              # the same pinned bytes as a numpy array
        ring.append(slot)
        return slot

    big_ring = []

    def big_staging(nbytes):
        slot = big_ring.pop(0) if len(big_ring) >= 3 else {"buf": None, "ev": None}
        if slot["ev"] is not None:
            slot["ev"].synchronize()
        if slot["buf"] is None or slot["buf"].numel() < nbytes:
            slot["buf"] = torch.empty(int(nbytes * 1.25) + 4096, dtype=torch.uint8).pin_memory()
            slot["np"] = slot["buf"].numpy()
        big_ring.append(slot)
        return slot

    def device_stage(devt, bigview, full, good):
        """The batch's regions of the big segment -> their rows of devt, on the copy stream behind devt's own copy: ONE H2D copy
        of the segment where it lies (it is page-locked: no packing copy on the host - packing 1 GB per batch of photo-sized
        images with one thread was slower than Pillow's resize), then clipmi_resize_crop_rgb8 for the full-size images
        (decode_worker.FULL_SIZE) and, for each kind of parsed file in decode_worker.PARSED's order, its decode entry (_FORMATS) +
        clipmi_resize_crop_rgb8.
        The copy stream carries the copies only; the kernels go to the process's ONE side stream (_lib.side_stream: this ROCm gives a
        process three hardware queues) behind an event, so that the next batch's copy runs beside this batch's kernels instead of
        behind them, and the consumer finds them queued in front of its encode step.
        -> (event behind the kernels, pending: what the consumer checks afterwards - the decoder's per-file status). Returns when the
        segment has been copied (it is decoded into again two batches later)."""
        from . import _lib
        L = _lib.lib()
        n = len(good)
        comp = np.cumsum(good) - 1                           # slot -> row of devt
        cap = bigview.size // n
        used = (max(full) + 1) * cap
        e2 = np.array(sorted(s_ for s_, v in full.items() if v[0] == FULL_SIZE.kind), dtype=np.int64)
        parsed = [np.array(sorted(s_ for s_, v in full.items() if v[0] == k.kind), dtype=np.int64) for k in PARSED]
        n_status = sum(len(slots) for slots in parsed)      # one status tensor: the kinds in PARSED's order
        if not pool.pin_segment(2 + seg_index[0]):
            # the segment could not be page-locked (locked-memory limit?): this batch goes through a pinned copy of it, the
            # following ones take the host path
            full_cap[0] = 0
            slot = big_staging(used)
            np.copyto(slot["np"][:used], bigview[:used])
            src = slot["buf"][:used]
        else:
            slot = None
            src = torch.from_numpy(bigview[:used])
        pending = {"keep": [], "status": None, "launch": [], "count_ok": []}
        with torch.cuda.stream(copy_stream):
            dbig = src.to(dev, non_blocking=True)
            base = dbig.data_ptr()
            if n_status:
                pending["status"] = torch.empty(n_status, dtype=torch.int32, device=dev)
                pending["slots"] = np.concatenate(parsed)

            def resize_into_devt(src_ptr, jobs_ptr, n_jobs, max_rows, scratch, entry="clipmi_resize_crop_rgb8"):
                if entry == "clipmi_nearest_crop_p8":
                    rc = L.clipmi_nearest_crop_p8(src_ptr, jobs_ptr, n_jobs, base, n_px, devt.data_ptr(), _lib.stream_ptr(dev))
                else:
                    rc = getattr(L, entry)(src_ptr, jobs_ptr, n_jobs, max_rows, base, n_px, devt.data_ptr(), scratch.data_ptr(),
                                           _lib.stream_ptr(dev))
                _lib.check(rc, entry)

            if len(e2):
                # decode_full's regions: [pixels | pad to 16 | PLAN_INTS header: w h, the plan, n_hcoef n_vcoef | coefficient blocks]
                wh = np.array([full[s_][1:3] for s_ in e2], dtype=np.int64)
                o_hdr = e2 * cap + (wh[:, 0] * wh[:, 1] * 3 + 15) // 16 * 16
                hd = np.stack([np.frombuffer(bigview, dtype=np.int32, count=PLAN_INTS, offset=int(o)) for o in o_hdr]).astype(np.int64)
                jobs = _resize_jobs(e2 * cap, wh[:, 0], wh[:, 1], hd[:, 2:10], hd[:, 10], o_hdr // 4 + PLAN_INTS, comp[e2], n_px)
                djobs = torch.from_numpy(jobs.view(np.uint8).reshape(-1).copy()).to(dev)
                scratch = torch.empty(max(int((hd[:, 3] * n_px * 3).sum()), 1), dtype=torch.uint8, device=dev)
                pending["keep"] += [djobs, scratch]

                def resize_full(djobs=djobs, scratch=scratch, n2=len(e2), max_rows=max(1, int(hd[:, 3].max()))):
                    resize_into_devt(base, djobs.data_ptr(), n2, max_rows, scratch)

                pending["launch"].append(resize_full)
            status_at = 0                                    # where this kind's statuses start in the tensor
            for kind, slots in zip(PARSED, parsed):
                if not len(slots):
                    continue
                # groups of files whose decoded form (for JPEG coefficients, sample planes, RGB rows: ~22 bytes per pixel; for PNG
                # scanlines and RGB rows) fits a budget: a batch of thumbnails is one group, a batch of 12-megapixel photos many -
                # they run one after the other through ONE workspace per kind (the side stream is in order), so that HBM holds a
                # group, not a batch, of decoded photos. The kinds follow each other on the side stream in PARSED's order.
                records, decoder_bytes, group, px, entry = kind_formats[kind.kind]
                tmp_px = 0 if entry == "clipmi_nearest_crop_p8" else px      # scratch bytes per pixel of the rows between the passes
                hd = _headers(bigview, n, cap, slots)
                need = file_need(hd, kind_formats[kind.kind], n_px)
                calls, ws_max, rgb_max, tmp_max = [], 0, 0, 0
                for lo, hi in _groups(need, jpeg_group_bytes):
                    arrays, out_sz, ws_bytes, name, decode = group(L, records(bigview, n, cap, slots[lo:hi], comp, n_px))
                    small, offs = _pack16(arrays)
                    dsmall = torch.from_numpy(small).to(dev)
                    nrows = hd[lo:hi, HDR.NROWS]
                    ws_max, rgb_max = max(ws_max, ws_bytes), max(rgb_max, int(out_sz.sum()) if entry is not None else 0)
                    tmp_max = max(tmp_max, int((nrows * n_px * tmp_px).sum()))
                    calls.append((dsmall, offs, hi - lo, int(nrows.max()), name, decode, 4 * (status_at + lo)))
                    pending["keep"].append(dsmall)
                ws = torch.empty(ws_max, dtype=torch.uint8, device=dev)
                rgb = torch.empty(max(rgb_max, 16), dtype=torch.uint8, device=dev) if entry is not None else None
                scratch = torch.empty(max(tmp_max, 1), dtype=torch.uint8, device=dev)

                def decode_kind(calls=calls, ws=ws, rgb=rgb, scratch=scratch, status=pending["status"], entry=entry):
                    for dsmall, offs, n_files, max_rows, name, decode, status_off in calls:
                        sb = dsmall.data_ptr()
                        if entry is None:                    # (the decode entry transforms too: no full-size rows)
                            _lib.check(decode(base, sb, offs, None, status.data_ptr() + status_off, ws.data_ptr(), _lib.stream_ptr(dev),
                                              (max_rows, n_px, devt.data_ptr(), scratch.data_ptr())), name)
                            continue
                        _lib.check(decode(base, sb, offs, rgb.data_ptr(), status.data_ptr() + status_off, ws.data_ptr(),
                                          _lib.stream_ptr(dev)), name)
                        resize_into_devt(rgb.data_ptr(), sb + offs[-1], n_files, max_rows, scratch, entry)

                pending["launch"].append(decode_kind)
                pending["keep"] += [ws, rgb, scratch]
                if kind.counts == "decoded":
                    pending["count_ok"].append((kind.stat, status_at, status_at + len(slots)))
                status_at += len(slots)
            ev_copy = torch.cuda.Event()
            ev_copy.record(copy_stream)
        side = _lib.side_stream(dev)[1]
        with torch.cuda.stream(side):
            side.wait_event(ev_copy)
            for launch in pending["launch"]:
                launch()
            ev = torch.cuda.Event()
            ev.record(side)
        ev_copy.synchronize()                                 # the segment is decoded into again two batches later
        pending["keep"].append(dbig)
        if slot is not None:
            slot["ev"] = ev_copy
        return ev, pending

    def to_device(host, slot):
        with torch.cuda.stream(copy_stream):
            devt = host.to(dev, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(copy_stream)
        if slot is not None:
            slot["ev"] = ev
        return devt, ev

    seg_index = [0]
    pin_small = os.environ.get("CLIPMI_PIN_SHM", "1") != "0"

    def copy_out(decoded, chunk):
        """shared memory -> pinned staging (GPU) or a private tensor (CPU) -> device. numpy copies on purpose: a 65-MB torch
        copy_ fans out over every CPU the host shows (256 here) and its OpenMP team then spins through the container's CPU
        share - every other batch's decode took 80 ms instead of 15 (tools/attic/pipe_probe.py: 26.7 k images/s decode only,
        5.9 k with a torch copy behind each batch)."""
        bigview = full = None
        if len(decoded[0]) == 4:
            (view, good, bigview, full), ok, bad = decoded
        else:
            (view, good), ok, bad = decoded
        if not ok:
            return ok, bad, None, None
        if not use_gpu:
            return ok, bad, torch.from_numpy(view[good] if len(ok) != len(chunk) else view.copy()), None
        small_used = any(g_ and k not in full for k, g_ in enumerate(good)) if full else True
        if not small_used:
            # every image of the batch sits in the big segment (full size, or as a parsed JPEG file): nothing to copy out of
            # the n_px x n_px slots
            with torch.cuda.stream(copy_stream):
                devt = torch.empty((len(ok), 3, n_px, n_px), dtype=torch.uint8, device=dev)
            ev = None
        elif len(ok) == len(chunk) and pin_small and pool.pin_segment(seg_index[0]):
            # the segment itself is page-locked (hipHostRegister): copy it to the device where it lies, and let this
            # thread wait for the copy (1-2 ms) - the segment is decoded into again two batches later
            devt, ev = to_device(torch.from_numpy(view), None)
            ev.synchronize()
        else:
            slot = staging(len(ok))
            if len(ok) == len(chunk):
                np.copyto(slot["np"][:len(ok)], view)
            else:
                np.compress(good, view, axis=0, out=slot["np"][:len(ok)])
            devt, ev = to_device(slot["buf"][:len(ok)], slot)
        pending = None
        if full:
            ev, pending = device_stage(devt, bigview, full, good)
            pending["chunk"], pending["good"] = chunk, good.copy()
        if jpeg_cap and full_cap[0]:
            # the next batches' JPEG regions: 1.25 x the largest file this batch held or turned away
            used3 = max([int(v[3]) for v in (full or {}).values() if v[0] in PARSED_KINDS] + [pool.jpeg_wanted])
            pool.jpeg_wanted = 0
            if used3:
                pool.jpeg_cap_hint = min(jpeg_cap, max(1 << 16, (used3 + used3 // 4 + 65535) // 65536 * 65536))
                full_cap[0] = max(resize_cap, pool.jpeg_cap_hint)
        return ok, bad, devt, ev, pending

    def redo_on_host(bad_slots, chunk, good, ok, bad, devt):
        """Files the device decoder reported corrupt: Pillow decides (its error handling is the reference's) - its pixels replace
        the row, or the file joins the failed ones and its row leaves the batch."""
        comp = np.cumsum(good) - 1
        drop = []
        for s_ in bad_slots:
            try:
                px = torch.from_numpy(load_uint8(chunk[s_], n_px)).to(dev)
                devt[comp[s_]].copy_(px)
            except KeyboardInterrupt:
                raise
            except Exception:
                drop.append(s_)
        if drop:
            gone = {chunk[s_] for s_ in drop}
            keep_rows = torch.tensor([r for r in range(len(ok)) if r not in {int(comp[s_]) for s_ in drop}], dtype=torch.long, device=dev)
            devt = devt.index_select(0, keep_rows)
            ok = [p_ for p_ in ok if p_ not in gone]
            bad = [p_ for p_ in chunk if p_ in gone or p_ in set(bad)]
        torch.cuda.synchronize(dev)
        return ok, bad, devt

    def stage(chunk):
        """The thread form: decode on `workers` threads, stack, pin, copy."""
        arrs = list(tpool.map(_load_safe, [(p, n_px) for p in chunk]))
        ok = [p for p, a in zip(chunk, arrs) if a is not None]
        bad = [p for p, a in zip(chunk, arrs) if a is None]
        if not ok:
            return ok, bad, None, None
        good_arrs = [a for a in arrs if a is not None]
        if not use_gpu:
            return ok, bad, torch.from_numpy(np.stack(good_arrs)), None
        slot = staging(len(ok))                            # numpy writes straight into pinned memory (no torch copy: see copy_out)
        np.stack(good_arrs, out=slot["np"][:len(ok)])
        devt, ev = to_device(slot["buf"][:len(ok)], slot)
        return ok, bad, devt, ev

    chunks = [paths[i:i + batch] for i in range(0, len(paths), batch)]

    def consume(item):
        ok, bad, devt, ev = item[:4]
        pending = item[4] if len(item) > 4 else None
        feats = None
        t0 = time.perf_counter()
        if devt is not None:
            if ev is not None:
                torch.cuda.current_stream(dev).wait_event(ev)
            feats = model.encode_image(devt, normalize=True).cpu().numpy().astype("float32")
            if pending is not None and pending["status"] is not None:
                stc = pending["status"].cpu().numpy()         # (behind the encode step: nothing waits for it in the common case)
                if stats is not None:
                    for key, lo, hi in pending["count_ok"]:
                        stats[key] = stats.get(key, 0) + int((stc[lo:hi] == 0).sum())
                if stc.any():
                    ok, bad, devt = redo_on_host([int(s_) for s_ in pending["slots"][stc != 0]], pending["chunk"],
                                                 pending["good"], ok, bad, devt)
                    feats = model.encode_image(devt, normalize=True).cpu().numpy().astype("float32") if len(ok) else None
        if stats is not None:
            stats["encode_s"] = stats.get("encode_s", 0.0) + time.perf_counter() - t0
        return ok, feats, bad

    if pool is not None:
        # three stages, one thread each: decode batch j+1 (worker processes, shared-memory segment (j+1) & 1) | copy batch j
        # out of its segment and to the device | encode batch j-1 here. A segment is decoded into again only after its
        # previous batch has been copied out.
        with ThreadPoolExecutor(max_workers=1) as dec, ThreadPoolExecutor(max_workers=1) as cpy:
            copies = {}

            def decode_job(j):
                if j - 2 in copies:
                    copies[j - 2].result()                 # segment j & 1 is free again
                t0 = time.perf_counter()
                r = [pool.decode(chunks[j], n_px, copy=False, segment=j & 1, full_cap=full_cap[0], full_mode=full_mode)]
                if stats is not None:
                    stats["decode_s"] = stats.get("decode_s", 0.0) + time.perf_counter() - t0
                return r

            def copy_job(d, j):
                seg_index[0] = j & 1
                dec_ = d.result().pop()
                t0 = time.perf_counter()
                r = copy_out(dec_, chunks[j])
                if stats is not None:
                    stats["copy_s"] = stats.get("copy_s", 0.0) + time.perf_counter() - t0
                    if len(dec_[0]) == 4:
                        for k in PARSED:
                            if k.counts == "staged":
                                stats[k.stat] = stats.get(k.stat, 0) + sum(1 for v in dec_[0][3].values() if v[0] == k.kind)
                return r

            def submit(j):
                d = dec.submit(decode_job, j)              # (the result travels in a list the copy stage empties: no
                copies[j] = cpy.submit(copy_job, d, j)     # view outlives its copy)

            for j in range(min(2, len(chunks))):
                submit(j)
            for ci in range(len(chunks)):
                item = copies[ci].result()
                if ci + 2 < len(chunks):
                    submit(ci + 2)
                copies.pop(ci - 2, None)
                yield consume(item)
        return
    with ThreadPoolExecutor(max_workers=workers) as tpool, ThreadPoolExecutor(max_workers=1) as stager:
        nxt = stager.submit(stage, chunks[0]) if chunks else None
        for ci in range(len(chunks)):
            item = nxt.result()
            nxt = stager.submit(stage, chunks[ci + 1]) if ci + 1 < len(chunks) else None
            yield consume(item)
