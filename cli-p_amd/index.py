"""Flat inner-product index: the host-side mirror of the faiss objects the reference scripts use.

Reference call sites (paths under the reference tree):
  build-index.py:80-81   faiss.IndexFlatIP(512) / IndexIVFFlat(..., METRIC_INNER_PRODUCT)
  build-index.py:96,99   index.train(images) / index.add(images)
  build-index.py:109     faiss.write_index(index, "images.index")
  query-index.py:29-30   faiss.read_index("images.index"); index.nprobe = 32
  query-index.py:111     D, I = index.search(features, k + offset + 1)

Search here is EXACT (the reference's IVF list scan is approximate): `train` is a
no-op and `nprobe` is accepted and ignored. The packed [N][d] f32 matrix lives in HBM; search
calls clipmi_topk_ip through the C ABI. Multi-GPU: one process per GPU, rows split contiguously
by rank, per-rank top-K, ONE all-gather (RCCL when the tensors are on the GPU), then the same
K-way merge on every rank (clipmi_merge_topk) — SURVEY.md §8e.
"""
import collections
import os
import struct

import numpy as np
import torch

from . import _lib

MAGIC = b"CLIPMIIX"   # own packed file format, see write_index
METRIC_INNER_PRODUCT = 0


def shard_bounds(n_total, world_size, rank):
    """Contiguous row split: rank r owns [lo, hi). Every rank computes the same bounds."""
    base, rem = divmod(int(n_total), int(world_size))
    lo = rank * base + min(rank, rem)
    hi = lo + base + (1 if rank < rem else 0)
    return lo, hi


def merge_lists_host(scores, ids, K):
    """Host restatement of the merge rule for the CPU (gloo) path of ShardedFlatIP tests:
    scores f32 [R,Q,K], ids i64 [R,Q,K] -> (f32 [Q,K], i64 [Q,K]); score desc, id asc, -1 = empty."""
    R, Q, _ = scores.shape
    out_s = np.full((Q, K), -np.finfo(np.float32).max, dtype=np.float32)
    out_i = np.full((Q, K), -1, dtype=np.int64)
    for q in range(Q):
        s = scores[:, q, :].reshape(-1)
        i = ids[:, q, :].reshape(-1)
        ok = (i >= 0) & ~np.isnan(s)
        s, i = s[ok], i[ok]
        order = np.lexsort((i, -s.astype(np.float64)))[:K]
        out_s[q, :len(order)] = s[order]
        out_i[q, :len(order)] = i[order]
    return out_s, out_i


COARSE_DIMS = (512, 768)        # widths the coarse-then-exact paths are built for (csrc/topk.hip scan_coarse_kernel<E, ...>)
COARSE_MIN_ROWS = 65536        # below this the library answers CLIPMI_EUNSUPPORTED (csrc/topk.hip SAMPLE_MIN_N)


def coarse_eligible(coarse, d, ntotal):
    """THE predicate of the coarse path: a coarse copy was asked for, the width has coarse kernels, the shard is large enough.
    IndexFlatIP.uses_coarse(), repl.open_sharded and repl.main all decide with it."""
    return coarse in ("bf16", "int8") and d in COARSE_DIMS and ntotal >= COARSE_MIN_ROWS


Route = collections.namedtuple("Route", "entry workspace chunk")


def search_route(coarse, d, wide_768, Q):
    """(library entry, its workspace function, queries per call of a pipelined search) for one search of Q queries.
    coarse: "bf16", "int8", or None when the coarse path is not usable (not eligible, or a non-finite or zero rmax / amax);
    wide_768: IndexFlatIP._wide_768_on(). Pure: touches no device and no library. A search of more than `chunk` queries
    alternates chunk-sized calls between two streams (IndexFlatIP._search_pipelined); chunk None: one call, whatever Q."""
    if coarse is None:
        return Route("clipmi_topk_ip", "clipmi_topk_ip_workspace_bytes", None)
    if coarse == "bf16":
        return Route("clipmi_topk_ip_coarse", "clipmi_topk_ip_coarse_workspace_bytes", IndexFlatIP.PASS_Q)
    # more than 64 queries: the int8 path takes the whole search as wide passes inside the library (one stream of the
    # copy per <= 1024 queries, csrc/topk.hip "Wide coarse pass"); the bf16 path pipelines its 64-query passes here, and so
    # does the int8 path at d = 768 by default: clipmi_topk_ip_coarse_i8 has no wide pass there (a 256-query tile of 768
    # bytes does not fit in LDS) and would run the 64-query passes one after the other on one stream
    if d == 512:
        # int8, more than one wide chunk (1024 queries): the chunks alternate between two streams the same way - one chunk's
        # re-scoring and selects run beside the other's matrix-bound scan (10 M rows, 2 x 1024 queries: 6.37 -> 6.07 ms per
        # chunk, 160.9 -> 168.8 k q/s; a single chunk cut in two halves gains nothing: 162.4 k)
        return Route("clipmi_topk_ip_coarse_i8", "clipmi_topk_ip_coarse_workspace_bytes", IndexFlatIP.WIDE_Q)
    # (opt-in at d = 768, `wide_768`: the library's wide pass there - clipmi_topk_ip_wide_i8 -, chunks of WIDE_Q_768 queries)
    if wide_768 and Q > IndexFlatIP.PASS_Q:
        return Route("clipmi_topk_ip_wide_i8", "clipmi_topk_ip_wide_workspace_bytes", IndexFlatIP.WIDE_Q_768)
    return Route("clipmi_topk_ip_coarse_i8", "clipmi_topk_ip_coarse_workspace_bytes", IndexFlatIP.PASS_Q)


def _alloc_out(out, Q, K, device):
    """The caller's (scores, ids) views, or fresh f32 / i64 [Q,K] tensors."""
    if out is not None:
        return out
    return (torch.empty((Q, K), dtype=torch.float32, device=device), torch.empty((Q, K), dtype=torch.int64, device=device))


class IndexFlatIP:
    """Exact inner-product index over f32 vectors resident in HBM (storage="f16": over fp16 vectors, half the bytes)."""

    def __init__(self, d, device="cuda:0", coarse=None, wide_768=None, storage="f32"):
        """coarse="bf16": keep a bf16 copy of the matrix beside the f32 one (+50 % HBM) and search through
        clipmi_topk_ip_coarse — a bf16-MFMA scan that keeps a provable superset, then exact f32
        re-scoring: same bit-exact results, half the bytes per pass, 64 queries per pass.
        coarse="int8": the same with a per-row-scaled int8 copy (+25 % HBM + 8 B per row): a quarter of the
        f32 bytes per pass; the superset bound uses each row's exact quantisation-error norm, so rows with
        one dominant component loosen it (more survivors, or the exact fallback) but never change results.
        wide_768 (opt-in; d = 768 with coarse="int8" only, ignored otherwise): searches of more than 64 queries go through
        clipmi_topk_ip_wide_i8 - one pass of the int8 copy per <= 1024 queries instead of one per 64. Same bit-exact
        results. None takes $CLIPMI_WIDE_768 ("" or "0": off, anything else: on); the default is off.
        storage="f16" (opt-in): the rows are kept as IEEE binary16 - `add` rounds each chunk to nearest even as
        it arrives and drops the f32 chunk - and searched EXACTLY as the f32 values of those halves (clipmi_topk_ip with
        CLIPMI_F16: the same fmaf chain on the up-converted rows), at half the HBM and file bytes. `f16_changed` counts the
        elements the rounding changed (0: the index lost nothing, e.g. rows a GPU build of the reference produced in fp16),
        `f16_overflowed` stays 0: an element beyond the fp16 range makes `add` raise. No coarse copy: coarse= must be None."""
        if coarse not in (None, "bf16", "int8"):
            raise ValueError("IndexFlatIP: coarse must be None, 'bf16' or 'int8'")
        if storage not in ("f32", "f16"):
            raise ValueError(f"IndexFlatIP: storage must be 'f32' or 'f16', got {storage!r}")
        if storage == "f16" and coarse is not None:
            raise ValueError("IndexFlatIP: storage='f16' has no coarse path (the coarse passes re-score from the f32 matrix); "
                             "coarse must be None")
        self.storage = storage
        self.f16_changed = 0
        self.f16_overflowed = 0
        self.coarse = coarse
        if wide_768 is None:
            wide_768 = os.environ.get("CLIPMI_WIDE_768", "") not in ("", "0")
        self.wide_768 = bool(wide_768)
        self._dbh = None
        self._rmax = None
        self._db8 = None
        if d not in (512, 768):
            raise ValueError("IndexFlatIP: d must be 512 (ViT-B/32) or 768 (ViT-L/14)")
        self.d = int(d)
        self.device = torch.device(device)
        self.nprobe = 1          # accepted for drop-in compatibility (query-index.py:30,51); ignored
        self.is_trained = True
        self.metric_type = METRIC_INNER_PRODUCT
        self.id_base = 0         # global id of local row 0 (non-zero on shards)
        self._chunks = []
        self._db = None
        self._ws = {}            # workspace per HIP stream: searches in flight on different streams never share one

    # -- build side ---------------------------------------------------------------------------
    def train(self, x):
        """No-op: exact search needs no k-means (build-index.py:96,105)."""
        return None

    def add(self, x):
        """Append rows (numpy f32 [n,d] as in build-index.py:99,107, or a torch tensor)."""
        if not isinstance(x, torch.Tensor):
            x = np.asarray(x)
            if not x.flags.writeable:
                x = x.copy()                # torch warns on (and may alias) read-only buffers, e.g. np.frombuffer views
            t = torch.as_tensor(x)
        else:
            t = x
        if t.dim() != 2 or t.shape[1] != self.d:
            raise ValueError(f"add: expected [n,{self.d}], got {tuple(t.shape)}")
        t = t.to(device=self.device, dtype=torch.float32).contiguous()
        if self.storage == "f16":
            t = self._to_f16(t)             # raises, with the index untouched, if an element leaves the fp16 range
        self._chunks.append(t)
        self._db = None
        self._dbh = None
        self._db8 = None
        self._rmax = None

    def _to_f16(self, t):
        """One f32 chunk -> its fp16 rows (nearest even), with the counts added to f16_changed: clipmi_rows_to_f16 on a GPU,
        torch's own conversion on a CPU device (host-logic tests). ValueError if a finite element became infinite."""
        if t.shape[0] == 0:
            return torch.empty(t.shape, dtype=torch.float16, device=t.device)
        if self.device.type == "cuda":
            h = torch.empty(t.shape, dtype=torch.float16, device=t.device)
            counts = torch.zeros(2, dtype=torch.int64, device=t.device)
            _lib.check(_lib.lib().clipmi_rows_to_f16(t.data_ptr(), t.shape[0], self.d, h.data_ptr(), counts.data_ptr(),
                                                     _lib.stream_ptr(self.device)), "clipmi_rows_to_f16")
            changed, over = (int(v) for v in counts.cpu())
        else:
            h = t.to(torch.float16)
            back = h.to(torch.float32)
            changed = int(((back != t) & ~torch.isnan(t)).sum())
            over = int((torch.isfinite(t) & torch.isinf(back)).sum())
        if over:
            raise ValueError(f"add: {over} element(s) beyond the fp16 range (largest finite fp16 value: 65504) would become "
                             "infinite; storage='f16' cannot hold these rows")
        self.f16_changed += changed
        return h

    def _add_f16(self, h):
        """Append rows that ARE fp16 already (a version-2 file): nothing is rounded, nothing counted."""
        self._chunks.append(torch.as_tensor(h).to(device=self.device, dtype=torch.float16).contiguous())
        self._db = None

    @property
    def ntotal(self):
        return sum(c.shape[0] for c in self._chunks)

    def _packed(self, dtype):
        if self._db is None:
            if not self._chunks:
                self._db = torch.empty((0, self.d), dtype=dtype, device=self.device)
            elif len(self._chunks) == 1:
                self._db = self._chunks[0]
            else:
                self._db = torch.cat(self._chunks, dim=0)
                self._chunks = [self._db]
        return self._db

    def matrix_f16(self):
        """The stored [N][d] torch.float16 device matrix of an fp16 index (concatenated once, like matrix())."""
        if self.storage != "f16":
            raise ValueError("matrix_f16: the index stores f32 rows (storage='f32')")
        return self._packed(torch.float16)

    def _stored(self):
        """(the stored matrix, its CLIPMI dtype code): what the exact searches read."""
        return (self.matrix_f16(), _lib.F16) if self.storage == "f16" else (self.matrix(), _lib.F32)

    def matrix(self):
        """The packed [N][d] f32 device matrix (rows in add order = LMDB key order, build-index.py:75-89).
        On an fp16 index (storage="f16"): a FRESH f32 up-conversion of the stored halves on every call (exact; 4 N d bytes,
        never cached - the index itself keeps only the fp16 rows)."""
        if self.storage == "f16":
            return self.matrix_f16().to(torch.float32)
        if self._db is None:
            if not self._chunks:
                self._db = torch.empty((0, self.d), dtype=torch.float32, device=self.device)
            elif len(self._chunks) == 1:
                self._db = self._chunks[0]
            else:
                self._db = torch.cat(self._chunks, dim=0)
                self._chunks = [self._db]
        return self._db

    def matrix_bf16(self):
        """(bf16 copy [N][d], upper bound of the largest row norm) for the coarse path; built once (clipmi_rows_to_bf16)."""
        if self.storage == "f16":
            raise ValueError("matrix_bf16: an fp16 index has no coarse copy")
        if self._dbh is None:
            db = self.matrix()
            dbh = torch.empty(db.shape, dtype=torch.bfloat16, device=db.device)
            if db.shape[0]:
                _lib.check(_lib.lib().clipmi_rows_to_bf16(db.data_ptr(), db.shape[0], self.d, dbh.data_ptr(),
                                                          _lib.stream_ptr(self.device)), "clipmi_rows_to_bf16")
            self._dbh = dbh
        return self._dbh, self._row_norm_max()

    def _stats(self, meta=None):
        """(largest row norm, largest error norm of the int8 copy's meta) by clipmi_rows_stats, each with a 1e-6 margin."""
        db = self.matrix()
        if db.shape[0] == 0:
            return 0.0, 0.0
        if self.device.type != "cuda":
            raise _lib.ClipmiError("the coarse copies need the HIP path (device is not a GPU); no CPU fallback")
        out = torch.empty(2, dtype=torch.float32, device=db.device)
        _lib.check(_lib.lib().clipmi_rows_stats(db.data_ptr(), db.shape[0], self.d, meta.data_ptr() if meta is not None else None,
                                                out.data_ptr(), _lib.stream_ptr(self.device)), "clipmi_rows_stats")
        rmax, amax = (float(v) for v in out.cpu())
        return rmax * (1.0 + 1e-6), amax * (1.0 + 1e-6)

    def _row_norm_max(self):
        if self._rmax is None:
            self._rmax = self._stats()[0]
        return self._rmax

    def matrix_i8(self):
        """(int8 copy in 32-row blocks of [d / 32][64][16 B] - include/clipmi.h clipmi_quantize_rows_i8 -, f32 meta:
        (block scale, error norm) per row padded to 32 rows (+32) then (scale, largest error norm) per block, largest
        error norm, largest row norm) for the int8 coarse path; built once by clipmi_quantize_rows_i8 + clipmi_rows_stats."""
        if self.storage == "f16":
            raise ValueError("matrix_i8: an fp16 index has no coarse copy")
        if self._db8 is None:
            L = _lib.lib()
            db = self.matrix()
            N = db.shape[0]
            q8 = torch.empty(L.clipmi_i8_copy_bytes(N, self.d), dtype=torch.int8, device=db.device)
            meta = torch.zeros(L.clipmi_i8_meta_bytes(N) // 4, dtype=torch.float32, device=db.device)
            # The copy holds the rows ORDERED BY THEIR LARGEST |COMPONENT| (round 4): the 32 rows of a block then share a scale
            # that is nearly each row's own (error norms x 1.265 -> x 1.000 on unit rows, ~12 % fewer exactly re-scored rows);
            # the library maps surviving slots back to row ids, results are row ids in add order as ever. The order is built
            # once per index by the library itself (clipmi_rows_order_by_absmax: row maxima + a stable radix sort on the device;
            # round 5 - a framework sort did this before). CLIPMI_I8_SORT=0: rows in add order.
            perm = ws = None
            if os.environ.get("CLIPMI_I8_SORT", "1") != "0" and N > 32:
                perm = torch.empty(N, dtype=torch.int32, device=db.device)
                ws = torch.empty(L.clipmi_rows_order_workspace_bytes(N), dtype=torch.uint8, device=db.device)
                _lib.check(L.clipmi_rows_order_by_absmax(db.data_ptr(), N, self.d, perm.data_ptr(), ws.data_ptr(), ws.numel(),
                                                         _lib.stream_ptr(self.device)), "clipmi_rows_order_by_absmax")
            _lib.check(L.clipmi_quantize_rows_i8(db.data_ptr(), N, self.d, perm.data_ptr() if perm is not None else None,
                                                 q8.data_ptr(), q8.numel(), meta.data_ptr(), meta.numel() * 4,
                                                 _lib.stream_ptr(self.device)), "clipmi_quantize_rows_i8")
            if perm is not None:
                torch.cuda.current_stream(self.device).synchronize()      # perm / ws are read by the kernels just enqueued
            del perm, ws
            self._rmax, amax = self._stats(meta)
            self._db8 = (q8, meta, amax)
        return self._db8 + (self._row_norm_max(),)

    def uses_coarse(self):
        """True when searches go through a coarse-then-exact path (coarse copy requested, d = 512 or 768, N >= 65536).
        Never on an fp16 index, whatever `.coarse` was set to after construction: its searches are the exact fp16 scan."""
        return self.storage != "f16" and coarse_eligible(self.coarse, self.d, self.ntotal)

    # -- query side ---------------------------------------------------------------------------
    def search_device(self, q, K, out=None, _one_pass=False):
        """q: f32 [Q,d] device tensor -> (scores f32 [Q,K], ids i64 [Q,K]) device tensors. Async.
        `out` = (scores, ids) views to write into (the packed all-gather record of ShardedFlatIP)."""
        L = _lib.lib()
        db, db_dtype = self._stored()
        if self.device.type != "cuda":
            raise _lib.ClipmiError("IndexFlatIP.search needs the HIP path (device is not a GPU); no CPU fallback")
        q = q.to(device=self.device, dtype=torch.float32).contiguous()
        Q = q.shape[0]
        N = db.shape[0]
        # build the copy; a non-finite or zero bound leaves the search on the exact path
        coarse = self.coarse if self.uses_coarse() else None
        if coarse == "int8":
            db8, meta, amax, rmax = self.matrix_i8()
            if not (rmax > 0.0 and np.isfinite(rmax) and np.isfinite(amax)):
                coarse = None
        elif coarse:
            dbh, rmax = self.matrix_bf16()
            if not (rmax > 0.0 and np.isfinite(rmax)):
                coarse = None
        route = search_route(coarse, self.d, self._wide_768_on(), Q)
        if route.chunk and Q > route.chunk and self.batches_in_flight > 1 and not _one_pass:
            return self._search_pipelined(q, K, out, route.chunk)
        need = getattr(L, route.workspace)(N, self.d, Q, K)
        if need == 0:
            raise _lib.ClipmiError("topk_ip: " + _lib.last_error())
        # the workspace belongs to the stream the call is enqueued on (torch's current stream): two batches in flight on
        # two streams each get their own, and the caching allocator hands a block back only to the stream that owned it
        skey = torch.cuda.current_stream(self.device).cuda_stream
        ws = self._ws.get(skey)
        if ws is None or ws.numel() < need:
            ws = self._ws[skey] = torch.empty(need, dtype=torch.uint8, device=self.device)
        out_s, out_i = _alloc_out(out, Q, K, self.device)
        # one library call; only its leading arguments depend on the copy
        if coarse == "int8":
            lead = (db.data_ptr(), db8.data_ptr(), meta.data_ptr(), amax, N, self.d, rmax)
        elif coarse:
            lead = (db.data_ptr(), dbh.data_ptr(), N, self.d, rmax)
        else:
            lead = (db.data_ptr(), db_dtype, N, self.d)
        rc = getattr(L, route.entry)(*lead, q.data_ptr(), Q, K, self.id_base, out_s.data_ptr(), out_i.data_ptr(), ws.data_ptr(),
                                     ws.numel(), _lib.stream_ptr(self.device))
        _lib.check(rc, route.entry)
        return out_s, out_i

    PASS_Q = 64                   # queries of one coarse pass (csrc/topk.hip COARSE_Q)
    WIDE_Q = 1024                 # queries of one wide pass of the int8 copy (csrc/topk.hip WIDE_MAX_Q)
    WIDE_Q_768 = 1024             # ... at d = 768, when `wide_768` is on (csrc/topk.hip WIDE768_MAX_Q)
    batches_in_flight = 2         # 64-query passes of ONE large search kept in flight on internal streams (1 = off)

    def _wide_768_on(self):
        """The opt-in wide pass applies: asked for, d = 768, int8 copy (the flag is inert anywhere else)."""
        return self.wide_768 and self.d == 768 and self.coarse == "int8"

    def _search_pipelined(self, q, K, out, chunk):
        """A search of more than 64 queries on the bf16 coarse path or the int8 path at d = 768 (`chunk` = 64), or of more than 1024
        on the int8 path at d = 512 or - with `wide_768` - at d = 768 (`chunk` = 1024 = one wide pass): its passes alternate between the caller's stream and an
        internal HIP stream (each with its own workspace), so one pass's latency-bound side kernels run beside the other's
        HBM-bound scan -
        what bench.py measures as "two batches in flight" (0.97-1.03 vs 1.09-1.10 ms per pass at 10 M rows). Same calls,
        same results; the caller's stream waits for the side stream before anything after the search runs."""
        Q = q.shape[0]
        out_s, out_i = _alloc_out(out, Q, K, self.device)
        # lanes = the caller's stream + ONE side stream, the process-wide one that CLIP.encode_image's second kernel sequence uses
        # too (_lib.side_stream: this ROCm gives only the first three streams of a process their own hardware queue and every
        # later one shares the fourth - two side streams created after a caller's own two ran on ONE queue, back to back:
        # rocprofv3 Queue_Id; a side stream per model and index did the same to bench.py's search leg in round 5)
        cur, side1 = _lib.side_stream(self.device)
        side = [side1]
        lanes = [cur] + side
        for s_ in side:
            s_.wait_stream(cur)                       # q, the outputs and the index copies are ready
        for gi, lo in enumerate(range(0, Q, chunk)):
            hi = min(Q, lo + chunk)
            with torch.cuda.stream(lanes[gi % len(lanes)]):
                self.search_device(q[lo:hi], K, out=(out_s[lo:hi], out_i[lo:hi]), _one_pass=True)
        for s_ in side:
            cur.wait_stream(s_)
        return out_s, out_i

    def search(self, x, K):
        """D, I = index.search(features, K) (query-index.py:111): numpy in, numpy out."""
        q = torch.from_numpy(np.array(x, dtype=np.float32, order="C")) if not isinstance(x, torch.Tensor) else x
        if q.dim() != 2 or q.shape[1] != self.d:
            raise ValueError(f"search: expected [Q,{self.d}], got {tuple(q.shape)}")
        s, i = self.search_device(q, int(K))
        return s.cpu().numpy(), i.cpu().numpy()

    def subset(self, rows):
        """The exact search restricted to `rows` (faiss: an IDSelector) -> IndexSubset. rows: an integer array or tensor of
        local row numbers (add order; sorted and de-duplicated here), or a bool mask of length ntotal. Negative or >= ntotal
        entries, a mask of another length and a float dtype raise ValueError - here, once, never in a search."""
        return IndexSubset(self, rows)


def shard_rows(rows, lo, hi):
    """Global row numbers -> the local ones of the shard [lo, hi) (`shard_bounds`): those inside it, minus lo, sorted, int64.
    Pure; `index_of_shard.subset(shard_rows(rows, lo, hi))` with id_base = lo answers in global ids again."""
    r = np.unique(np.asarray(rows, dtype=np.int64).reshape(-1))
    return r[(r >= lo) & (r < hi)] - int(lo)


def _subset_list(rows, ntotal):
    """subset()'s argument -> sorted, de-duplicated int64 tensor of row numbers (on the argument's device for a tensor)."""
    if isinstance(rows, (list, tuple)) and len(rows) == 0:
        rows = np.empty(0, dtype=np.int64)     # (numpy would make an empty list float64)
    t = rows if isinstance(rows, torch.Tensor) else torch.as_tensor(np.asarray(rows))
    if t.dtype == torch.bool:
        if t.dim() != 1 or t.shape[0] != ntotal:
            raise ValueError(f"subset: a bool mask must have length ntotal = {ntotal}, got shape {tuple(t.shape)}")
        return torch.nonzero(t).reshape(-1).to(torch.int64)
    if t.dtype.is_floating_point or t.dtype.is_complex:
        raise ValueError(f"subset: rows must be integers or a bool mask, got {t.dtype}")
    t = t.reshape(-1).to(torch.int64)
    if t.numel() and (int(t.min()) < 0 or int(t.max()) >= ntotal):
        raise ValueError(f"subset: row numbers must lie in [0, {ntotal}), got {int(t.min())} .. {int(t.max())}")
    return torch.unique(t)                     # sorted ascending


class IndexSubset:
    """IndexFlatIP.subset(rows): the exact top-K among the chosen rows only, reading only those rows.

    Over an fp16 parent (storage="f16") the list scan reads the stored halves (CLIPMI_F16), M (2 d + 4) bytes.
    Same contracts as IndexFlatIP - search(x, K) numpy in / numpy out, search_device(q, K, out=None) device tensors, async -
    and the same results as searching everything and discarding the other rows: bit-exact scores, descending score then
    ascending row id, ids = parent row + id_base, pads (-FLT_MAX, -1) beyond min(K, M). Every search goes through
    clipmi_topk_ip_rows - the exact f32 list scan - WHATEVER `coarse=` the parent has: the coarse copies have no list form,
    and the list scan reads M (d + 1) 4 bytes, fewer than the int8 copy's pass for any subset under a quarter of the rows.
    `id_base` is the subset's own (initialised from the parent's; ShardedFlatIP sets it), `nprobe` is accepted and ignored.
    The u32 list lives on the parent's device and is built once, here. A parent that has grown since (`add`) makes every
    later search raise ClipmiError: the list was checked against the rows of then."""

    def __init__(self, parent, rows):
        self.parent = parent
        self.d, self.device = parent.d, parent.device
        self.nprobe = 1
        self.id_base = parent.id_base
        self._n_parent = parent.ntotal
        lst = _subset_list(rows, self._n_parent)
        self._rows = lst.to(self.device)                # int64, for rows()
        # the u32 list the library reads: the low four bytes of each little-endian int64 (row numbers < 2^32 - 1)
        self._list = self._rows.view(torch.int32)[0::2].contiguous() if lst.numel() else torch.empty(0, dtype=torch.int32, device=self.device)
        self._ws = {}

    @property
    def ntotal(self):
        return int(self._list.shape[0])

    def rows(self):
        """The sorted row numbers (int64 tensor on the index's device)."""
        return self._rows

    def search_device(self, q, K, out=None):
        """q: f32 [Q,d] -> (scores f32 [Q,K], ids i64 [Q,K]) device tensors. Async."""
        if self.parent.ntotal != self._n_parent:
            raise _lib.ClipmiError(f"IndexSubset: the parent index has grown from {self._n_parent} to {self.parent.ntotal} rows "
                                   "since subset(); take a new subset")
        if self.device.type != "cuda":
            raise _lib.ClipmiError("IndexSubset.search needs the HIP path (device is not a GPU); no CPU fallback")
        L = _lib.lib()
        db, db_dtype = self.parent._stored()
        q = q.to(device=self.device, dtype=torch.float32).contiguous()
        Q, M = q.shape[0], self.ntotal
        need = L.clipmi_topk_ip_rows_workspace_bytes(M, self.d, Q, K)
        if need == 0:
            raise _lib.ClipmiError("topk_ip_rows: " + _lib.last_error())
        skey = torch.cuda.current_stream(self.device).cuda_stream
        ws = self._ws.get(skey)
        if ws is None or ws.numel() < need:
            ws = self._ws[skey] = torch.empty(need, dtype=torch.uint8, device=self.device)
        out_s, out_i = _alloc_out(out, Q, K, self.device)
        rc = L.clipmi_topk_ip_rows(db.data_ptr(), db_dtype, db.shape[0], self.d, self._list.data_ptr() if M else None, M,
                                   q.data_ptr(), Q, K, self.id_base, out_s.data_ptr(), out_i.data_ptr(), ws.data_ptr(),
                                   ws.numel(), _lib.stream_ptr(self.device))
        _lib.check(rc, "clipmi_topk_ip_rows")
        return out_s, out_i

    def search(self, x, K):
        """D, I = subset.search(features, K): numpy in, numpy out."""
        q = torch.from_numpy(np.array(x, dtype=np.float32, order="C")) if not isinstance(x, torch.Tensor) else x
        if q.dim() != 2 or q.shape[1] != self.d:
            raise ValueError(f"search: expected [Q,{self.d}], got {tuple(q.shape)}")
        s, i = self.search_device(q, int(K))
        return s.cpu().numpy(), i.cpu().numpy()


def IndexIVFFlat(quantizer, d, nlist=100, metric=METRIC_INNER_PRODUCT):
    """faiss.IndexIVFFlat(quantizer, 512, 100, faiss.METRIC_INNER_PRODUCT) (build-index.py:81) — returns
    the EXACT flat index: the inverted lists exist to avoid a full scan, which this build performs
    at HBM speed instead. `nlist` is accepted and ignored; only inner product is supported."""
    if metric != METRIC_INNER_PRODUCT:
        raise ValueError("IndexIVFFlat: only METRIC_INNER_PRODUCT is supported")
    dev = getattr(quantizer, "device", "cuda:0")
    return IndexFlatIP(d, device=dev)


class ShardedFlatIP:
    """Rank-local shard + the one all-gather merge. One process per GPU.

    Each rank holds rows [lo, hi) of the global matrix (`shard_bounds`), searches them with
    global ids, all-gathers the [Q,K] partials and merges. On GPUs the collective is RCCL
    (`backend="nccl"`) over xGMI and the merge is clipmi_merge_topk; on the gloo/CPU path (tests
    of the host logic, no GPU) `local_search` must be supplied and the merge is merge_lists_host.
    """

    def __init__(self, local_index, n_total, group=None, local_search=None):
        import torch.distributed as dist
        self.dist = dist
        self.group = group
        self.rank = dist.get_rank(group)
        self.world = dist.get_world_size(group)
        self.local = local_index
        self.n_total = int(n_total)
        self.lo, self.hi = shard_bounds(n_total, self.world, self.rank)
        if local_index is not None:
            local_index.id_base = self.lo
        self._local_search = local_search
        self.nprobe = 1

    def _record(self, Q, K, device):
        """Per-rank packed record [scores f32 Q*K | pad | ids i64 Q*K] and the gather buffer, cached per (Q, K, stream)."""
        skey = torch.cuda.current_stream(device).cuda_stream if device.type == "cuda" else 0
        key = (Q, K, str(device), skey)
        cache = self.__dict__.setdefault("_rec_cache", {})
        ent = cache.get(key)
        if ent is None:
            ids_off = (Q * K * 4 + 7) // 8 * 8
            nbytes = ids_off + Q * K * 8
            rec = torch.empty(nbytes, dtype=torch.uint8, device=device)
            gath = torch.empty(self.world * nbytes, dtype=torch.uint8, device=device)
            ent = cache[key] = (rec, gath, rec[:Q * K * 4].view(torch.float32).view(Q, K), rec[ids_off:].view(torch.int64).view(Q, K))
        return ent

    def search_device(self, q, K, out=None):
        """-> (scores f32 [Q,K], ids i64 [Q,K]) of the WHOLE index, on every rank. `out` = (scores, ids) to write into;
        otherwise fresh tensors per call (a caller holding two results keeps both: the record and gather buffers are
        reused, the results are not)."""
        dist = self.dist
        Q = q.shape[0]
        if self._local_search is None:
            # GPU path: local top-K written straight into the packed record, ONE all-gather (RCCL),
            # merge kernel on the gathered buffer — three enqueues, no host round trip
            dev = self.local.device
            rec, gath, rec_s, rec_i = self._record(Q, K, dev)
            self.local.search_device(q, K, out=(rec_s, rec_i))
            dist.all_gather_into_tensor(gath, rec, group=self.group)
            L = _lib.lib()
            out_s, out_i = _alloc_out(out, Q, K, dev)
            rc = L.clipmi_merge_topk_packed(gath.data_ptr(), rec.numel(), self.world, Q, K, out_s.data_ptr(),
                                            out_i.data_ptr(), _lib.stream_ptr(dev))
            _lib.check(rc, "clipmi_merge_topk_packed")
            return out_s, out_i
        # CPU / gloo path (tests of the host logic): same record, host merge
        s, i = self._local_search(q, K, self.lo)
        s = torch.as_tensor(np.ascontiguousarray(s, dtype=np.float32))
        i = torch.as_tensor(np.ascontiguousarray(i, dtype=np.int64))
        rec, gath, rec_s, rec_i = self._record(Q, K, torch.device("cpu"))
        rec_s.copy_(s)
        rec_i.copy_(i)
        dist.all_gather_into_tensor(gath, rec, group=self.group)
        n = rec.numel()
        ids_off = (Q * K * 4 + 7) // 8 * 8
        S = np.stack([gath[r * n:r * n + Q * K * 4].view(torch.float32).view(Q, K).numpy() for r in range(self.world)])
        I = np.stack([gath[r * n + ids_off:(r + 1) * n].view(torch.int64).view(Q, K).numpy() for r in range(self.world)])
        ms, mi = merge_lists_host(S, I, K)
        if out is not None:
            out[0].copy_(torch.from_numpy(ms))
            out[1].copy_(torch.from_numpy(mi))
            return out
        return torch.from_numpy(ms), torch.from_numpy(mi)

    def search(self, x, K):
        q = torch.from_numpy(np.array(x, dtype=np.float32, order="C")) if not isinstance(x, torch.Tensor) else x
        s, i = self.search_device(q, int(K))
        return s.cpu().numpy(), i.cpu().numpy()


FAISS_FOURCC_FLAT_IP = b"IxFI"


def write_index(index, path, format="clipmi"):
    """faiss.write_index stand-in (build-index.py:109).
    format="clipmi": own packed format, little-endian: 8-byte magic, u32 version, u32 d, u64 ntotal, then
        ntotal*d f32 rows (version 1: an f32 index, the bytes as ever). An fp16 index (storage="f16") writes VERSION 2:
        magic, <IIQ (2, d, ntotal), <II (dtype code 3 = CLIPMI_F16, 0), then ntotal*d little-endian halves.
    format="faiss": the serialisation of a faiss IndexFlatIP as published in faiss/impl/index_write.cpp
        (fourcc "IxFI"; header d:i32, ntotal:i64, two i64 placeholders = 1<<20, is_trained:u8,
        metric_type:i32 = 0; then u64 count of floats + the f32 rows), so that the ORIGINAL
        query-index.py:29 (`faiss.read_index("images.index")`) can open an index built here
        (SURVEY.md §8f next-3). faiss is not available offline: this layout is restated from the
        upstream source, PARITY UNPINNED until checked against a real faiss build.
        An fp16 index writes its rows up-converted to f32 here (exact), so the reference can still open the file."""
    if format == "clipmi" and getattr(index, "storage", "f32") == "f16":
        dbh = np.ascontiguousarray(index.matrix_f16().cpu().numpy(), dtype="<f2")
        with open(path, "wb") as f:
            f.write(MAGIC + struct.pack("<IIQ", 2, index.d, dbh.shape[0]) + struct.pack("<II", _lib.F16, 0))
            f.write(dbh.tobytes())
        return
    db = np.ascontiguousarray(index.matrix().cpu().numpy(), dtype="<f4")
    with open(path, "wb") as f:
        if format == "faiss":
            f.write(FAISS_FOURCC_FLAT_IP)
            f.write(struct.pack("<iqqq", index.d, db.shape[0], 1 << 20, 1 << 20))
            f.write(struct.pack("<Bi", 1, METRIC_INNER_PRODUCT))
            f.write(struct.pack("<Q", db.size))
        elif format == "clipmi":
            f.write(MAGIC + struct.pack("<IIQ", 1, index.d, db.shape[0]))
        else:
            raise ValueError(f"write_index: unknown format {format!r}")
        f.write(db.tobytes())


def _read_faiss_header(f):
    """faiss write_index_header: d i32, ntotal i64, two dummy i64, is_trained u8, metric i32."""
    d, n, _, _ = struct.unpack("<iqqq", f.read(28))
    trained, metric = struct.unpack("<Bi", f.read(5))
    return d, n, metric


def _read_faiss_ivfflat(f, path):
    """The file the REFERENCE writes (build-index.py:80-81,109: IndexIVFFlat(IndexFlatIP(512), 512, 100,
    METRIC_INNER_PRODUCT) -> faiss.write_index): fourcc "IwFl", index header, nlist u64, nprobe u64, the
    quantizer as a nested index ("IxFI" + centroids), the direct map (u8 type, i64 vector[, hashtable]),
    then ArrayInvertedLists: fourcc "ilar", nlist u64, code_size u64, list sizes ("full": u64 vector of nlist
    sizes; "sprs": u64 vector of (list, size) pairs), then per non-empty list its codes (n * code_size bytes =
    n rows of d f32) and its ids (n i64). Layout as in faiss impl/index_write.cpp (write_ivf_header,
    write_direct_map, write_InvertedLists). Returns the rows in ID order: exact search over them returns a
    superset-quality answer of what the IVF index (nprobe of 100 lists) would.
    PARITY UNPINNED: no faiss build exists in this environment to produce or check a real file; the test
    fixture is written by tests/ from the same layout."""
    d, n, metric = _read_faiss_header(f)
    if metric != METRIC_INNER_PRODUCT:
        raise ValueError(f"{path}: faiss IVF index with metric {metric}; only inner product is supported")
    nlist, _nprobe = struct.unpack("<QQ", f.read(16))
    q4 = f.read(4)
    if q4 not in (b"IxFI", b"IxF2", b"IxFl"):
        raise ValueError(f"{path}: IVF quantizer {q4!r} is not a flat index")
    qd, qn, _ = _read_faiss_header(f)
    (cnt,) = struct.unpack("<Q", f.read(8))
    if qd != d or cnt != qn * qd:
        raise ValueError(f"{path}: malformed IVF quantizer")
    f.seek(cnt * 4, 1)                                   # centroids: not needed for exact search
    (dm_type,) = struct.unpack("<B", f.read(1))
    (dm_n,) = struct.unpack("<Q", f.read(8))
    f.seek(dm_n * 8, 1)
    if dm_type == 2:                                     # hashtable: vector of (key, value) pairs
        (hn,) = struct.unpack("<Q", f.read(8))
        f.seek(hn * 16, 1)
    if f.read(4) != b"ilar":
        raise ValueError(f"{path}: only ArrayInvertedLists ('ilar') are supported")
    il_nlist, code_size = struct.unpack("<QQ", f.read(16))
    if il_nlist != nlist or code_size != 4 * d:
        raise ValueError(f"{path}: inverted lists nlist {il_nlist} / code size {code_size} do not match IVFFlat d={d}")
    kind = f.read(4)
    (sz_n,) = struct.unpack("<Q", f.read(8))
    raw = np.fromfile(f, dtype="<u8", count=sz_n)
    sizes = np.zeros(nlist, dtype=np.int64)
    if kind == b"full":
        if sz_n != nlist:
            raise ValueError(f"{path}: 'full' list sizes vector has {sz_n} entries for {nlist} lists")
        sizes[:] = raw
    elif kind == b"sprs":
        sizes[raw[0::2].astype(np.int64)] = raw[1::2]
    else:
        raise ValueError(f"{path}: unknown inverted-list size encoding {kind!r}")
    if int(sizes.sum()) != n:
        raise ValueError(f"{path}: inverted lists hold {int(sizes.sum())} vectors, header says {n}")
    mat = np.empty((n, d), dtype=np.float32)
    seen = np.zeros(n, dtype=bool)
    for ln in sizes:
        ln = int(ln)
        if ln == 0:
            continue
        codes = np.fromfile(f, dtype="<f4", count=ln * d)
        ids = np.fromfile(f, dtype="<i8", count=ln)
        if codes.size != ln * d or ids.size != ln:
            raise ValueError(f"{path}: truncated inverted list")
        if ids.min() < 0 or ids.max() >= n or seen[ids].any():
            raise ValueError(f"{path}: ids are not a permutation of 0..{n - 1} (custom ids are not supported)")
        seen[ids] = True
        mat[ids] = codes.reshape(ln, d)
    return d, mat


def storage_from_env(environ=os.environ):
    """$CLIPMI_STORAGE -> the `storage=` of read_index / IndexFlatIP on the command-line paths: None (unset, "" or "f32":
    the file's own kind, an f32 index when building) or "f16". Anything else raises ValueError with the line to print."""
    v = environ.get("CLIPMI_STORAGE", "")
    if v in ("", "f32"):
        return None
    if v == "f16":
        return "f16"
    raise ValueError(f"CLIPMI_STORAGE must be f32 or f16, got {v!r}.")


F16_ADD_ROWS = 1 << 20      # rows per `add` when read_index converts an f32 file into an fp16 index


def read_index(path, device="cuda:0", rows=None, coarse=None, wide_768=None, storage=None):
    """faiss.read_index stand-in (query-index.py:29): reads both formats write_index produces and the
    IndexIVFFlat file the reference's build-index.py writes (rows come back in id order and are searched
    exactly; `nprobe` is accepted and ignored).
    rows=(lo, hi): load only that contiguous row range (one rank's shard) — the flat formats
    seek straight to it (by the file's element size); the returned index has `id_base = lo` and `n_file` = the file's row count.
    storage: None keeps the file's own kind (a version-2 clipmi file gives an fp16 index, everything else an f32 one); "f16" on
    an f32 file converts while loading, in `add` calls of at most 2^20 rows; "f32" on a version-2 file up-converts (exact)."""
    if storage not in (None, "f32", "f16"):
        raise ValueError(f"read_index: storage must be None, 'f32' or 'f16', got {storage!r}")
    esize, ftype = 4, "<f4"
    with open(path, "rb") as f:
        head = f.read(8)
        if head[:4] == FAISS_FOURCC_FLAT_IP or head == MAGIC:
            if head == MAGIC:
                ver, d, n = struct.unpack("<IIQ", f.read(16))
                if ver not in (1, 2):
                    raise ValueError(f"{path}: unsupported version {ver}")
                if ver == 2:
                    ext = f.read(8)
                    if len(ext) != 8:
                        raise ValueError(f"{path}: truncated version-2 header")
                    code, _reserved = struct.unpack("<II", ext)
                    if code != _lib.F16:
                        raise ValueError(f"{path}: version-2 file with dtype code {code}; only 3 (fp16) is defined")
                    esize, ftype = 2, "<f2"
            else:
                f.seek(4)
                d, n, metric = _read_faiss_header(f)
                if metric != METRIC_INNER_PRODUCT:
                    raise ValueError(f"{path}: faiss flat index with metric {metric}; only inner product is supported")
                (count,) = struct.unpack("<Q", f.read(8))
                if count != n * d:
                    raise ValueError(f"{path}: vector count {count} != ntotal*d {n * d}")
            lo, hi = (0, n) if rows is None else (int(rows[0]), int(rows[1]))
            if not (0 <= lo <= hi <= n):
                raise ValueError(f"{path}: rows {rows} outside 0..{n}")
            f.seek((lo * d) * esize, 1)
            data = np.fromfile(f, dtype=ftype, count=(hi - lo) * d)
        elif head[:4] == b"IwFl":
            f.seek(4)
            d, mat = _read_faiss_ivfflat(f, path)
            n = mat.shape[0]
            lo, hi = (0, n) if rows is None else (int(rows[0]), int(rows[1]))
            if not (0 <= lo <= hi <= n):
                raise ValueError(f"{path}: rows {rows} outside 0..{n}")
            data = np.ascontiguousarray(mat[lo:hi]).reshape(-1)
        else:
            raise ValueError(f"{path}: not a clipmi, faiss IndexFlatIP or faiss IndexIVFFlat file")
    if data.size != (hi - lo) * d:
        raise ValueError(f"{path}: truncated ({data.size} of {(hi - lo) * d} floats)")
    file_f16 = esize == 2
    if storage is None:
        storage = "f16" if file_f16 else "f32"
    idx = IndexFlatIP(d, device=device, coarse=coarse, wide_768=wide_768, storage=storage)
    data = data.reshape(hi - lo, d)
    if hi > lo:
        if storage == "f16" and file_f16:
            idx._add_f16(data)                                # the halves themselves
        elif storage == "f16":
            for r0 in range(0, hi - lo, F16_ADD_ROWS):        # the f32 matrix is never resident as a whole
                idx.add(data[r0:r0 + F16_ADD_ROWS])
        else:
            idx.add(data.astype(np.float32) if file_f16 else data)
    idx.id_base = lo
    idx.n_file = n
    return idx


def index_rows(path):
    """(ntotal, d) of an index file without loading its rows (flat formats: header only)."""
    with open(path, "rb") as f:
        head = f.read(8)
        if head == MAGIC:
            _, d, n = struct.unpack("<IIQ", f.read(16))      # versions 1 and 2 share these 16 bytes
            return n, d
        if head[:4] in (FAISS_FOURCC_FLAT_IP, b"IwFl"):
            f.seek(4)
            d, n, _ = _read_faiss_header(f)
            return n, d
    raise ValueError(f"{path}: not a clipmi, faiss IndexFlatIP or faiss IndexIVFFlat file")
