"""Host image pipeline for the build side: threaded decode + the CLIP
transform's geometry on the host, pinned staging, asynchronous H2D, encode on the GPU in batches.

Reference per-image sequence (build-index.py:47-51): Image.open -> transform -> unsqueeze(0).to(device)
-> encode_image -> /norm -> .cpu(). Here the same images travel as uint8 [B,3,R,R] (resize / centre
crop / RGB done with Pillow exactly as `transform` does; the /255, -mean, /std tail is fused into the
device patch kernel), B at a time, decode of batch i+1 overlapping the GPU work of batch i.
Failures are per file (build-index.py:55-58): a file that does not decode is reported, not fatal.
"""
import os
import time
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

# the Pillow part of the transform and the kinds of regions (decode_worker.Kind) live beside the worker script
from .decode_worker import (ALL_PARSED, KIND_JPEG_CMYK, LAYOUTS_BIT, LAYOUTS_STAT, PARSED, PARSED_KINDS, PARSED_MORE, PNG_INTERLACED_BIT,  # noqa: F401
                            PNG_CHUNKS_BIT, PNG_CHUNKS_STAT, PNG_DEEP_BIT, PNG_DEEP_STAT, PNG_INTERLACED_STAT, REGION_TAGS, WANTED_TAG, load_uint8)
from .device_stage import (DeviceStage, PinnedRing, _FORMATS, _groups, _headers, _pack16, all_formats, file_need, formats, jpeg_cmyk_default,  # noqa: F401 (the moved names stay reachable as pipeline.<name>)
                           jpeg_fused_default, jpeg_layouts_default, jpeg_records, png_records, progressive_records)


class DecodePool:
    """Worker PROCESSES for the Pillow part of the transform (decode_worker.py): decode throughput that scales with
    the host cores also for small images, where threads are bound by the GIL. The workers are plain `python
    decode_worker.py` children started HERE - create the pool BEFORE the process initialises the GPU (indexer.main
    does): a process that has touched the GPU should not spawn programs on this platform. Pixels come back through
    shared memory (workers write their slots; no pickling, no copies through pipes): two segments used in turn, so that
    a batch can be decoded while the previous one is still being copied out."""

    def __init__(self, workers):
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


# A batch in the pool's segments, as DecodePool.decode(copy=False) left it: all n_px x n_px slots, the mask of the good ones and, where
# regions were asked for, the big segment and {slot: (kind, w, h, bytes)} of the files that sit there (else None, None)
Decoded = namedtuple("Decoded", "view good big full", defaults=(None, None))
# A batch on its way to the device: the paths that decoded and that failed, the uint8 batch tensor (None: no file decoded), the event
# behind the last work queued for it (None: nothing to wait for) and the device decoders' Pending (None: no region held a file)
Staged = namedtuple("Staged", "ok bad devt ev pending", defaults=(None, None, None))


class _Encoder:
    """encode_files' stages and the state they share. One thread each runs decode_job, copy_job and consume (the pool form), or stage and
    consume (the thread form): seg_index, full_cap and the pool's region hints belong to the copy stage; decode_job j + 2 waits for copy_job j."""

    def __init__(self, model, chunks, batch, pool, stats, copy_stream, resize_cap, jpeg_cap, full_cap, full_mode, group_bytes, kind_formats):
        self.model, self.chunks, self.pool, self.stats, self.copy_stream = model, chunks, pool, stats, copy_stream
        self.resize_cap, self.jpeg_cap, self.full_mode = resize_cap, jpeg_cap, full_mode
        self.full_cap = full_cap                             # bytes per region of the big segment; 0 once a segment could not be pinned
        self.n_px, self.dev = n_px, dev = model.visual.input_resolution, model.device
        self.use_gpu = dev.type == "cuda"
        self.seg_index = 0                                   # which pair of segments the copy stage is reading
        self.pin_small = os.environ.get("CLIPMI_PIN_SHM", "1") != "0"
        self.copies = {}                                     # batch -> its copy stage's future
        # pinned staging for the n_px x n_px slots. Pixels go shared memory -> pinned -> device: ONE host copy (the first version
        # copied out of the segment, then again into freshly pinned memory: 55 ms per 435-image batch against 23 ms of decode on
        # 16 workers).
        self.ring = PinnedRing(lambda n: torch.empty((max(n, batch), 3, n_px, n_px), dtype=torch.uint8).pin_memory())
        self.device_stage = DeviceStage(pool, dev, copy_stream, n_px, group_bytes, kind_formats) if full_cap else None

    def count(self, key, value):
        if self.stats is not None:
            self.stats[key] = self.stats.get(key, 0) + value

    def to_device(self, host, slot):
        with torch.cuda.stream(self.copy_stream):
            devt = host.to(self.dev, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self.copy_stream)
        if slot is not None:
            slot.ev = ev
        return devt, ev

    def copy_out(self, d, ok, bad, chunk):
        """shared memory -> pinned staging (GPU) or a private tensor (CPU) -> device. numpy copies on purpose: a 65-MB torch
        copy_ fans out over every CPU the host shows (256 here) and its OpenMP team then spins through the container's CPU
        share - every other batch's decode took 80 ms instead of 15 (tools/attic/pipe_probe.py: 26.7 k images/s decode only,
        5.9 k with a torch copy behind each batch)."""
        n_px, pool, full, good = self.n_px, self.pool, d.full, d.good
        if not ok:
            return Staged(ok, bad)
        if not self.use_gpu:
            return Staged(ok, bad, torch.from_numpy(d.view[d.good] if len(ok) != len(chunk) else d.view.copy()))
        small_used = any(g_ and k not in full for k, g_ in enumerate(good)) if full else True
        if not small_used:
            # every image of the batch sits in the big segment (full size, or as a parsed JPEG file): nothing to copy out of
            # the n_px x n_px slots
            with torch.cuda.stream(self.copy_stream):
                devt = torch.empty((len(ok), 3, n_px, n_px), dtype=torch.uint8, device=self.dev)
            ev = None
        elif len(ok) == len(chunk) and self.pin_small and pool.pin_segment(self.seg_index):
            # the segment itself is page-locked (hipHostRegister): copy it to the device where it lies, and let this
            # thread wait for the copy (1-2 ms) - the segment is decoded into again two batches later
            devt, ev = self.to_device(torch.from_numpy(d.view), None)
            ev.synchronize()
        else:
            slot = self.ring.take(len(ok))
            if len(ok) == len(chunk):
                np.copyto(slot.np[:len(ok)], d.view)
            else:
                np.compress(d.good, d.view, axis=0, out=slot.np[:len(ok)])
            devt, ev = self.to_device(slot.buf[:len(ok)], slot)
        pending = None
        if d.full:
            ev, pending, in_place = self.device_stage.run(devt, d.big, d.full, d.good, self.seg_index)
            pending.chunk, pending.good = chunk, d.good.copy()
            if not in_place:
                self.full_cap = 0                            # this batch went through a pinned copy; the following ones take the host path
        if self.jpeg_cap and self.full_cap:
            # the next batches' JPEG regions: 1.25 x the largest file this batch held or turned away
            used3 = max([int(v[3]) for v in (d.full or {}).values() if v[0] in PARSED_KINDS] + [pool.jpeg_wanted])
            pool.jpeg_wanted = 0
            if used3:
                pool.jpeg_cap_hint = min(self.jpeg_cap, max(1 << 16, (used3 + used3 // 4 + 65535) // 65536 * 65536))
                self.full_cap = max(self.resize_cap, pool.jpeg_cap_hint)
        return Staged(ok, bad, devt, ev, pending)

    def redo_on_host(self, bad_slots, p, ok, bad, devt):
        """Files the device decoder reported corrupt: Pillow decides (its error handling is the reference's) - its pixels replace
        the row, or the file joins the failed ones and its row leaves the batch."""
        chunk, comp = p.chunk, np.cumsum(p.good) - 1
        drop = []
        for s_ in bad_slots:
            try:
                px = torch.from_numpy(load_uint8(chunk[s_], self.n_px)).to(self.dev)
                devt[comp[s_]].copy_(px)
            except KeyboardInterrupt:
                raise
            except Exception:
                drop.append(s_)
        if drop:
            gone = {chunk[s_] for s_ in drop}
            keep_rows = torch.tensor([r for r in range(len(ok)) if r not in {int(comp[s_]) for s_ in drop}], dtype=torch.long, device=self.dev)
            devt = devt.index_select(0, keep_rows)
            ok = [p_ for p_ in ok if p_ not in gone]
            bad = [p_ for p_ in chunk if p_ in gone or p_ in set(bad)]
        torch.cuda.synchronize(self.dev)
        return ok, bad, devt

    def stage(self, tpool, chunk):
        """The thread form: decode on tpool's threads, stack, pin, copy."""
        arrs = list(tpool.map(_load_safe, [(p, self.n_px) for p in chunk]))
        ok = [p for p, a in zip(chunk, arrs) if a is not None]
        bad = [p for p, a in zip(chunk, arrs) if a is None]
        if not ok:
            return Staged(ok, bad)
        good_arrs = [a for a in arrs if a is not None]
        if not self.use_gpu:
            return Staged(ok, bad, torch.from_numpy(np.stack(good_arrs)))
        slot = self.ring.take(len(ok))                     # numpy writes straight into pinned memory (no torch copy: see copy_out)
        np.stack(good_arrs, out=slot.np[:len(ok)])
        return Staged(ok, bad, *self.to_device(slot.buf[:len(ok)], slot))

    def encode(self, devt):
        return self.model.encode_image(devt, normalize=True).cpu().numpy().astype("float32")

    def consume(self, item):
        ok, bad, devt, ev, pending = item
        feats = None
        t0 = time.perf_counter()
        if devt is not None:
            if ev is not None:
                torch.cuda.current_stream(self.dev).wait_event(ev)
            feats = self.encode(devt)
            if pending is not None and pending.status is not None:
                stc = pending.status.cpu().numpy()            # (behind the encode step: nothing waits for it in the common case)
                for key, lo, hi in pending.count_ok:       # (a file that a switch added counts under that switch's key, not its kind's:
                    kept = stc[lo:hi] == 0                 # a 16-bit file first, else an Adam7 file, else one with metadata chunks)
                    for stat, mark in ((PNG_DEEP_STAT, pending.deep), (PNG_INTERLACED_STAT, pending.interlaced), (PNG_CHUNKS_STAT, pending.chunked)):
                        self.count(stat, int((kept & mark[lo:hi]).sum()))
                        kept = kept & ~mark[lo:hi]
                    self.count(key, int(kept.sum()))
                if stc.any():
                    ok, bad, devt = self.redo_on_host([int(s_) for s_ in pending.slots[stc != 0]], pending, ok, bad, devt)
                    feats = self.encode(devt) if len(ok) else None
        self.count("encode_s", time.perf_counter() - t0)
        return ok, feats, bad

    def decode_job(self, j):
        if j - 2 in self.copies:
            self.copies[j - 2].result()                    # segment j & 1 is free again
        t0 = time.perf_counter()
        r = [self.pool.decode(self.chunks[j], self.n_px, copy=False, segment=j & 1, full_cap=self.full_cap, full_mode=self.full_mode)]
        self.count("decode_s", time.perf_counter() - t0)
        return r

    def copy_job(self, decoding, j):
        self.seg_index = j & 1
        head, ok, bad = decoding.result().pop()
        d = Decoded(*head)                                 # (view, good) or, called with full_cap > 0, (view, good, big, full)
        t0 = time.perf_counter()
        r = self.copy_out(d, ok, bad, self.chunks[j])
        self.count("copy_s", time.perf_counter() - t0)
        if self.stats is not None and d.full is not None:
            for k in ALL_PARSED:
                if k.counts == "staged":
                    self.count(k.stat, sum(1 for v in d.full.values() if v[0] == k.kind))
            self.count(LAYOUTS_STAT, r.pending.layout_files if r.pending is not None else 0)      # (DeviceStage counted: it read the headers)
            for stat in (PNG_INTERLACED_STAT, PNG_CHUNKS_STAT, PNG_DEEP_STAT):
                self.count(stat, 0)                        # (the keys exist from here on; consume() counts, behind the statuses)
        return r

    def submit(self, dec, cpy, j):
        d = dec.submit(self.decode_job, j)                 # (the result travels in a list the copy stage empties: no
        self.copies[j] = cpy.submit(self.copy_job, d, j)   # view outlives its copy)


def encode_files(model, paths, batch=256, workers=8, pool=None, device_resize_mb=None, device_jpeg_kb=None, stats=None,
                 jpeg_group_mb=32768, device_progressive=None, device_png=None, device_png_modes=None, jpeg_fused=None,
                 device_jpeg_layouts=None, device_png_interlaced=None, device_jpeg_cmyk=None, device_png_chunks=None,
                 device_png_deep=None):
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
    shares): 8-bit grey and RGB PNG files that are not interlaced (see device_png_interlaced) and hold at most decode_worker.PNG_MAX_RAW (16 MiB) of
    scanlines take the device too (png_parse.parse in the workers,
    clipmi_png_decode_rgb8 + clipmi_resize_crop_rgb8 on the side stream beside the JPEG decodes, grouped under jpeg_group_mb
    like them), the same bytes as Pillow's; every other PNG file and every file the device reports goes back to Pillow. With
    the flag off nothing changes for any file.
    device_png_modes (default $CLIPMI_DEVICE_PNG_MODES, else off; "1" = on; takes effect only with device_png on): RGBA, grey +
    alpha, palette (depth 1/2/4/8, with or without tRNS) and grey depth 1/2/4 files that are not interlaced take the device as
    well (png_parse.parse(modes=True), clipmi_png_decode_px8, then clipmi_resize_crop_rgba8 or clipmi_nearest_crop_p8: Pillow
    resamples such files in their own mode), the same bytes as Pillow's. Off, such files stay with Pillow as before.
    device_png_interlaced (default $CLIPMI_DEVICE_PNG_INTERLACED, else off; "1" = on; takes effect only with device_png on):
    Adam7-interlaced files of the colour types and depths the two switches above let through take the device as well
    (png_parse.parse(interlaced=True); the same two decode entries reconstruct the seven passes and leave the pixels laid out as
    those of the picture stored without interlace, so the transform behind them is the same), the same bytes as Pillow's.
    Interlaced alpha, palette and low-depth files need device_png_modes too. Off, every interlaced file stays with Pillow as before.
    device_png_chunks (default $CLIPMI_DEVICE_PNG_CHUNKS, else off; "1" = on; takes effect only with device_png on): files that
    carry iCCP, zTXt, iTXt, eXIf, tRNS (8-bit grey, RGB) or chunks Pillow has no handler for - what screenshots and editors' exports
    carry - take the device as well, each chunk under the rule of Pillow's handler (png_parse.parse(chunks=True): the workers
    inflate the compressed ones, bounded like Pillow); the device sees the same stream. Off, such files stay with Pillow as before.
    device_png_deep (default $CLIPMI_DEVICE_PNG_DEEP, else off; "1" = on; takes effect only with device_png on): RGB files of depth
    16 take the device as well, and with device_png_modes RGBA and grey + alpha files of depth 16 (png_parse.parse(deep=True);
    clipmi_png_decode_px8 keeps the samples' high bytes as Pillow does, then the transform of the 8-bit file), the same bytes as
    Pillow's. 16-bit grey stays with Pillow, which resamples it in 16 bits. Off, every 16-bit file stays with Pillow as before.
    jpeg_fused (default $CLIPMI_DEVICE_JPEG_FUSED, else off; "1" = on): baseline and progressive files on the device go through
    clipmi_jpeg_decode_transform_rgb8 / clipmi_jpeg_decode_progressive_transform_rgb8, which convert and resample straight from
    the decoder's sample planes: the same bytes, and no full-size RGB rows (3 bytes per pixel) in HBM, so that a group under
    jpeg_group_mb holds more files. Off, nothing changes for any file.
    device_jpeg_layouts (default $CLIPMI_DEVICE_JPEG_LAYOUTS, else off; "1" = on; takes effect only with the JPEG decode on the
    device above): YCbCr files with luma sampling 1x2 (4:4:0: what a lossless 90-degree rotation makes of a 4:2:2 file), 4x1
    (4:1:1) or 1x4 and the three-component files libjpeg takes for RGB-coded take the device too - baseline files, and progressive
    ones with device_progressive, plain or through the jpeg_fused entries (jpeg_parse.parse(layouts=True)) -, the same bytes as
    Pillow's; files the device reports go back to Pillow. Off, such files stay with Pillow as before.
    device_jpeg_cmyk (default $CLIPMI_DEVICE_JPEG_CMYK, else off; "1" = on; takes effect only with the JPEG decode on the device
    above): four-component baseline files - CMYK as stored (no Adobe marker, or Adobe transform 0) and YCCK (Adobe transform 2),
    components 1-3 sampled 1x1 - take the device too (jpeg_parse.parse(cmyk=True), clipmi_jpeg_decode_cmyk8, then
    clipmi_resize_crop_cmyk8: Pillow resamples such files in mode CMYK and converts afterwards; also with jpeg_fused, whose entries
    do not take four components), the same bytes as Pillow's; files the device reports go back to Pillow. Progressive
    four-component files, Adobe transform 1 and a fourth component sampled like the first stay with Pillow. Off, every
    four-component file stays with Pillow as before.
    jpeg_group_mb: the device decodes a batch's JPEG files in groups whose decoded form (~22 bytes per pixel) stays under that
    many MB of HBM - one group for a batch of thumbnails, several for a batch of photos.
    stats: a dict that receives the seconds each of the three pipelined stages was busy (decode_s: worker processes, copy_s:
    shared memory -> device incl. the decode / resize kernels, encode_s) and the files that took the device decoders, under the
    keys of decode_worker.PARSED (jpeg_files, jpeg_progressive_files: files staged for the device; png_files: files it decoded and
    did not hand back; png_mode_files: the same for the files device_png_modes adds - png_files keeps counting grey / RGB only;
    jpeg_layout_files: those of jpeg_files and jpeg_progressive_files that device_jpeg_layouts added, 0 with it off;
    png_interlaced_files: the interlaced files of every kind that device_png_interlaced added and the device did not hand back, 0
    with it off - png_files and png_mode_files keep counting files that are not interlaced only; png_deep_files: the 16-bit
    files device_png_deep added and the device did not hand back, interlaced ones included; png_chunk_files: the same for the files
    with metadata chunks that device_png_chunks added and neither of the two keys before counts; both 0 with their switch off;
    jpeg_cmyk_files: the
    four-component files staged for the device, 0 with device_jpeg_cmyk off)."""
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
    full_cap = max(resize_cap, jpeg_now)                 # bytes per region of the big segment, to start with
    if device_progressive is None:
        device_progressive = os.environ.get("CLIPMI_DEVICE_PROGRESSIVE", "0") not in ("", "0")
    if device_png is None:
        device_png = os.environ.get("CLIPMI_DEVICE_PNG", "0") not in ("", "0")
    if device_png_modes is None:
        device_png_modes = os.environ.get("CLIPMI_DEVICE_PNG_MODES", "0") not in ("", "0")
    if device_png_interlaced is None:
        device_png_interlaced = os.environ.get("CLIPMI_DEVICE_PNG_INTERLACED", "0") not in ("", "0")
    if device_png_chunks is None:
        device_png_chunks = os.environ.get("CLIPMI_DEVICE_PNG_CHUNKS", "0") not in ("", "0")
    if device_png_deep is None:
        device_png_deep = os.environ.get("CLIPMI_DEVICE_PNG_DEEP", "0") not in ("", "0")
    if jpeg_fused is None:
        jpeg_fused = jpeg_fused_default()
    if device_jpeg_layouts is None:
        device_jpeg_layouts = jpeg_layouts_default()
    if device_jpeg_cmyk is None:
        device_jpeg_cmyk = jpeg_cmyk_default()
    kind_formats = all_formats(jpeg_fused)
    full_mode = ((1 if resize_cap else 0) | (2 if jpeg_cap else 0) | (4 if jpeg_cap and device_progressive else 0) |
                 (8 if jpeg_cap and device_png else 0) | (16 if jpeg_cap and device_png and device_png_modes else 0) |
                 (LAYOUTS_BIT if jpeg_cap and device_jpeg_layouts else 0) |
                 (PNG_INTERLACED_BIT if jpeg_cap and device_png and device_png_interlaced else 0) |
                 (PNG_CHUNKS_BIT if jpeg_cap and device_png and device_png_chunks else 0) |
                 (PNG_DEEP_BIT if jpeg_cap and device_png and device_png_deep else 0) |
                 (PARSED_MORE[0].bit if jpeg_cap and device_jpeg_cmyk else 0))
    chunks = [paths[i:i + batch] for i in range(0, len(paths), batch)]
    enc = _Encoder(model, chunks, batch, pool, stats, copy_stream, resize_cap, jpeg_cap, full_cap, full_mode, jpeg_group_bytes, kind_formats)
    if pool is not None:
        # three stages, one thread each: decode batch j+1 (worker processes, shared-memory segment (j+1) & 1) | copy batch j
        # out of its segment and to the device | encode batch j-1 here. A segment is decoded into again only after its
        # previous batch has been copied out.
        with ThreadPoolExecutor(max_workers=1) as dec, ThreadPoolExecutor(max_workers=1) as cpy:
            for j in range(min(2, len(chunks))):
                enc.submit(dec, cpy, j)
            for ci in range(len(chunks)):
                item = enc.copies[ci].result()
                if ci + 2 < len(chunks):
                    enc.submit(dec, cpy, ci + 2)
                enc.copies.pop(ci - 2, None)
                yield enc.consume(item)
        return
    with ThreadPoolExecutor(max_workers=workers) as tpool, ThreadPoolExecutor(max_workers=1) as stager:
        nxt = stager.submit(enc.stage, tpool, chunks[0]) if chunks else None
        for ci in range(len(chunks)):
            item = nxt.result()
            nxt = stager.submit(enc.stage, tpool, chunks[ci + 1]) if ci + 1 < len(chunks) else None
            yield enc.consume(item)
