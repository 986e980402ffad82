"""No entry point may depend on what its workspace, its scratch rows or its outputs held on entry (include/clipmi.h: "a
caller-owned workspace", "no global mutable state"). This module holds no tests: it is the table that says why that should hold,
and the harness (fills, guarded, run_independent, run_after) that tests/test_ws_*_gpu.py drive every entry point through.
tests/test_ws_harness.py runs the harness itself on numpy stand-ins, so that it is known to fail on the defects it exists for.

THE TABLE. Per entry point: every region its Arena takes (or carves by hand), what ESTABLISHES the region inside the call before
anything of the call reads it, and the output slots the call writes. "wbr" = written before read in the same kernel.

csrc/topk.hip, clipmi_topk_ip (topk_ip_impl; N == 0: fill_empty_kernel writes every output slot, no workspace)
  cand   uint2 [QA][cap]    scan_topk_f32_kernel publishes entries [0, gcnt[q]); select_topk_kernel reads exactly those (M = gcnt[q],
                            clamped to cap). Entries behind gcnt[q] are stale and never read.
  gcnt   u32 [32]           zero_async (a kernel, common.hpp) clears its 128 B at the head of the call. Every select_topk_kernel stores 0 to the counter it
                            consumed (its last statement, on every path: staged, dense, streamed, need < K), so the next scan of the
                            same call - pre-pass -> main scan, pass -> next QA pass - starts from 0 again.
  thr0   f32 [32]           select_topk_kernel(sample) writes thr_out[q] for each of its qa blocks (rank K-1, or -inf when the list is
                            shorter than K) before the main scan reads thr_in[0..qa). Not read without the pre-pass.
  outputs  out_score[Q][K], out_id[Q][K]: the result select writes ranks [0, need) and pads [need, K) with (-FLT_MAX, -1).

csrc/topk.hip, clipmi_topk_ip_coarse / _coarse_i8 / _wide_i8 (coarse_search over carve(); once per chunk of 64 or <= 1024 queries)
  cand_e uint2 [qs][p.cap]  the exact fallback's lists: scan_topk_f32_kernel(run_if) publishes [0, gcnt_e[q]) and its select reads those;
                            both launches return at once when the flag is 0, and then the region is not touched.
  cand_c uint2 [qs][cap]    sample_scores_kernel writes entries [0, S1) of each query and sets gcnt_c[q] = S1; the scans append
                            (0xffffffff, slot) behind gcnt_c[q] under a bound check; rescore_pairs*_kernel and select_topk_kernel read
                            [0, min(gcnt_c[q], cap)) only. A stale 0xffffffff behind the counter is never read.
  ctl    u32 [nctl]         gcnt_e [qs] | gcnt_c [qs] | flag block: coarse_prep_kernel's block 0 stores 0 to all nctl words, first
                            launch of every chunk. gcnt_c: every select leaves min(M, K) (keep) or 0. gcnt_e: only the fallback scan
                            adds to it, its select zeroes it. flag word 0: set by the sample's select (non-finite query) or a scan's
                            overflow; read by the two fallback launches; cleared by the next chunk's prep.
  thr0   f32 [qs]           the sample's select and every segment's non-final select write thr_out[q], q < Q of the chunk; the
                            fallback scan reads thr_in[q] for q < Q only.
  tauc   f32 [qs]           (64-query passes only) carried in CoarseArgs, read by no kernel.
  last_m u32 [qs]           select_topk_kernel m_out: segment 0 overwrites (keep bit 1 clear), later segments add. Read by the
                            measurement hooks alone, never by a kernel.
  qmeta  f32 [4][qs]        coarse_prep_kernel writes rows 0, 1, 3 and -inf to row 2 for q < Q; the selects rewrite row 2. Columns
                            q >= Q of a used 16-query group are NOT written: a scan may read them, for queries whose image is zero
                            and whose pairs nobody consumes (lists, counters and the flag are per query or bound-checked).
  qimage uint4 [image]      coarse_prep_kernel: every query of the used groups, zero for the padding queries of a group.
  outputs  as clipmi_topk_ip: the last segment's select, or - flag set - the fallback's select behind it, writes all K slots of
           each of the Q rows.

csrc/topk.hip, clipmi_merge_topk / clipmi_merge_topk_packed: the 256-byte workspace is never touched (LDS only); every slot of
  out_score / out_id is written (ranks < min(valid, K), then the padding loop).

csrc/rowcopy.hip, clipmi_rows_order_by_absmax (carved by hand, no Arena: keys A | keys B | ids B | hist [256][blocks])
  keys A                    clipmi_rows_absmax writes all N; passes 1 and 3 rewrite all N (a scatter is a permutation).
  keys B, ids B             order_scatter_kernel of pass 0 writes all N before pass 1 reads them; pass 2 rewrites.
  hist                      order_hist_kernel stores (not adds) all 256 x blocks words each pass; order_scan_kernel scans in place.
  output   perm[N]: passes 1 and 3 write all N.
csrc/rowcopy.hip, clipmi_rows_stats: no workspace; stats2_dev[2] is cleared by the call's own zero_async, then atomicMax'ed.

csrc/encode.hip, clipmi_encode_image / clipmi_encode_text (carve(); B images or prompts, rows = B * tokens)
  patches bf16 [B np][patch_k]  patchify_kernel writes all patch_k columns (zeros behind 3 P P) before the patch GEMM.
  x      f32 [rows][W]      vision: the patch GEMM (EPI_PATCH_F32) writes the patch rows, cls_rows_kernel the class rows, ln_pre in
                            place; text: text_embed_kernel. LN-folded towers use it only as the residual GEMMs' wbr scratch.
  h      bf16 [rows][W]     LayerNorm or attention writes all rows before the GEMM that reads them.
  big    bf16 [rows][4W]    the qkv GEMM writes [rows][3W], attention reads that; c_fc writes [rows][4W], c_proj reads that.
  pooled bf16 [B][W]        the head's LayerNorm writes B rows before the projection GEMM.
  rowidx i32 [B]            text: eot_rows_kernel / text_embed_split_kernel; vision: not used (null).
  a8, a_scale, a_bs (FP8)   LayerNorm (out8 + scale8), attention or quantize_rows_fp8mx_kernel write rows [0, rows) of a8 and the
                            scales of those rows. a_bs is padded to 256 rows and the padding is never written: a GEMM tile may load
                            the scales of rows >= rows, which only feed accumulators of rows that are not stored.
  x8, x8_bs                 development library only (FP8 with folded LayerNorms); as a8 / a_bs.
  x3, ln_part, ln_leaf      ln_pre (out_x3 + out_part) or text_embed_split_kernel / split_stats write all rows; every residual GEMM
                            rewrites the rows and their partials (leaves: M <= 128) before the next LN-folded GEMM reads them.
  x3c, partc, leafc, xc     the pruned tail: gather_rows_kernel writes the B class rows, the out_proj GEMM their statistics.
  output   out[B][E]: the head's projection GEMM (EPI_F32) writes every element; l2_normalize in place.

csrc/jpeg.hip, clipmi_jpeg_decode_rgb8 / _transform_rgb8 (jpeg_baseline_planes)
  luts   JpLut [ntables]    jpeg_build_luts_kernel, whole.
  coef   i16 [blocks][64]   zero_async, then jpeg_huffman_kernel stores the non-zero coefficients, jpeg_dc_kernel in place.
  planes u8 [blocks][64]    jpeg_idct_kernel writes every block of an image's MCU grid; the colour kernels read inside it.
  outputs  status_dev[i]: jpeg_huffman_kernel stores on every path out (3, 1 / 2, 0), jpeg_idct_kernel then only replaces a 0 by 4.
           out_dev: jpeg_color_kernel writes W H 3 bytes of each image (the 16-byte padding between images is not written).
           transform entries: scratch rows by jpeg_color_resize_h_kernel (wbr for the vertical pass), out block out_index whole.
csrc/jpeg.hip, clipmi_jpeg_decode_progressive_rgb8 / _transform_rgb8 (jpeg_progressive_planes)
  luts   JppLut [ntables]   jpeg_build_pluts_kernel, whole.
  images JpegImage [n]      jpeg_progressive_kernel thread 0 stores the whole record before any return - an empty grey image for a
                            record it refuses - so jpeg_idct_kernel and the colour kernels never read a stale geometry.
  coef, planes              as the baseline entries (zero_async, then the scans' chains; idct).
  outputs  status_dev[i] on every path out of jpeg_progressive_kernel (1, 1, bad / ran out / 0); the rest as above.

csrc/png.hip, clipmi_png_decode_rgb8 / clipmi_png_decode_px8 (png_decode)
  raw    u8 [total_raw]     png_inflate_kernel writes an image's scanlines [raw_off, + raw bytes); png_unfilter_kernel<0> / <1> (one
                            per entry) and png_adler_kernel return at once when status != 0, else read exactly those bytes.
  want   u32 [n]            png_inflate_kernel stores the stream's Adler-32; png_adler_kernel reads it for status-0 images only.
  outputs  status_dev[i]: png_inflate_kernel stores on every path out; the later kernels only replace a 0. out_dev: W H px bytes.

csrc/resize.hip, clipmi_resize_crop_rgb8 / _rgba8: no Arena. scratch rows [tmp_off, + nrows n_px px) of a job are written by the
  first pass before the second reads them; out block out_index whole. clipmi_nearest_crop_p8: no scratch; out block whole.

Reading found no region that nothing establishes. (The clears were hipMemsetAsync calls when this table was written; they became
zero_async kernels when a captured call was seen to run with its memset node out of order - tests/test_graph_capture_gpu.py.) Two places rest on "garbage in, nothing of it out" instead of "never read" -
qmeta's padding columns and the FP8 block-scale padding - and are the first suspects should a fill change a result.
"""
import contextlib
from collections import namedtuple

import numpy as np

GUARD = 4096                # bytes of each guard band: keeps the 256-byte alignment Arena assumes for the interior
GUARD_BYTE = 0xA5           # the fifth pattern: no fill writes it over a whole band

Fill = namedtuple("Fill", "name")
ZEROS, ONES32, RANDOM, ALL_FF = Fill("0x00"), Fill("words=1"), Fill("random"), Fill("0xFF")


def fills():
    """The workspace patterns, benign first: zeros; every 32-bit word 1 (flags read as set, counters are off by one); seeded
    pseudo-random bytes; all 0xFF (NaN as f32, bf16 and e4m3, counters at their maximum, ids -1)."""
    return [ZEROS, ONES32, RANDOM, ALL_FF]


class WsFailure(AssertionError):
    """What the harness found. kind: "guard-band", "workspace-dependent", "unwritten-output" or "leftover-dependent"."""

    def __init__(self, kind, message):
        super().__init__(f"{kind}: {message}")
        self.kind = kind


def _is_np(buf):
    return isinstance(buf, np.ndarray)


def apply_fill(buf, fill, seed=20260):
    """Fill a flat uint8 buffer (numpy array, or torch tensor: then on torch's current stream, no synchronisation)."""
    n = buf.size if _is_np(buf) else buf.numel()
    if n == 0:
        return
    if fill == ZEROS or fill == ONES32:
        buf[:] = 0
        if fill == ONES32:
            buf[0::4] = 1                                   # little-endian words of value 1 (the interior is word-aligned)
    elif fill == ALL_FF:
        buf[:] = 0xFF
    elif fill == RANDOM:
        if _is_np(buf):
            buf[:] = np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)
        else:
            import torch
            g = torch.Generator(device=buf.device)
            g.manual_seed(seed)
            buf.copy_(torch.randint(0, 256, (n,), dtype=torch.uint8, device=buf.device, generator=g))
    else:
        raise ValueError(fill)


class Guarded:
    """One allocation of nbytes + 2 GUARD: .interior is what a call receives, exactly nbytes long; the bands before and behind it
    hold GUARD_BYTE."""

    def __init__(self, nbytes, device=None):
        self.nbytes = int(nbytes)
        if device is None:
            self.whole = np.empty(self.nbytes + 2 * GUARD, np.uint8)
        else:
            import torch
            self.whole = torch.empty(self.nbytes + 2 * GUARD, dtype=torch.uint8, device=device)
        self.interior = self.whole[GUARD:GUARD + self.nbytes]

    def arm(self, fill):
        self.whole[:GUARD] = GUARD_BYTE
        self.whole[GUARD + self.nbytes:] = GUARD_BYTE
        apply_fill(self.interior, fill)
        return self

    def snapshot(self, interior=True):
        """(band in front, band behind, the interior or None): copies, taken in stream order"""
        cp = (lambda a: a.copy()) if _is_np(self.whole) else (lambda a: a.clone())
        return cp(self.whole[:GUARD]), cp(self.whole[GUARD + self.nbytes:]), cp(self.interior) if interior else None


def guarded(nbytes, fill, device=None):
    """A Guarded buffer of exactly nbytes, its interior holding `fill`, both bands the guard pattern."""
    return Guarded(nbytes, device).arm(fill)


def _host(a):
    return a if a is None or _is_np(a) else a.cpu().numpy()


def _check_bands(snap, what, when):
    for band, where in ((snap[0], "in front of"), (snap[1], "behind")):
        bad = np.flatnonzero(_host(band) != GUARD_BYTE)
        if bad.size:
            off = int(bad[0]) - GUARD if where == "in front of" else int(bad[0])
            raise WsFailure("guard-band", f"{when}: the call wrote {where} {what}: byte {off:+d} from the "
                            f"{'start' if where == 'in front of' else 'end'} of the buffer is 0x{int(_host(band)[bad[0]]):02x}, "
                            f"{bad.size} byte(s) of the band changed")


_STREAMS = {}


@contextlib.contextmanager
def _stream(device):
    """numpy stand-ins: nothing. A device: ONE non-default stream per device (torch's pool), entered behind whatever the current
    stream holds; left with the stream drained - the only synchronisation of a harness run."""
    if device is None:
        yield
        return
    import torch
    s = _STREAMS.get(str(device))
    if s is None:
        s = _STREAMS[str(device)] = torch.cuda.Stream(device=device)
    s.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(s):
        yield
        s.synchronize()


def _first_diff(a, b):
    d = np.flatnonzero(a != b)
    return None if d.size == 0 else int(d[0])


def run_independent(call, outputs, ws_bytes, device=None, canon=None):
    """call(ws, *outs) once per fill of the workspace, on a non-default stream, fills and launches queued back to back; the
    outputs prefilled with 0x00 on the first run and 0xFF on the others. outputs: [(name, nbytes)]; ws and outs are flat uint8
    buffers (numpy arrays when device is None, else torch tensors on it) inside guard bands. canon({name: bytes}) -> {name: bytes}
    may blank what the contract leaves unspecified (the pixels of a reported file) before the runs are compared.
    Raises WsFailure unless every run leaves byte-identical outputs and intact bands; -> {name: uint8 array} of the first run."""
    names = [n for n, _ in outputs]
    runs = []
    with _stream(device):
        ws = Guarded(ws_bytes, device)
        outs = [Guarded(nb, device) for _, nb in outputs]
        for k, f in enumerate(fills()):
            ws.arm(f)
            for o in outs:
                o.arm(ZEROS if k == 0 else ALL_FF)
            call(ws.interior, *[o.interior for o in outs])
            runs.append((ws.snapshot(interior=False), [o.snapshot() for o in outs]))
    got = []
    for (wsnap, osnaps), f in zip(runs, fills()):
        when = f"workspace fill {f.name}"
        _check_bands(wsnap, f"its workspace of {ws_bytes} bytes", when)
        for n, s in zip(names, osnaps):
            _check_bands(s, f"output '{n}'", when)
        raw = {n: _host(s[2]) for n, s in zip(names, osnaps)}
        got.append((raw, canon({n: v.copy() for n, v in raw.items()}) if canon else raw))
    for k in range(1, len(got)):
        for n in names:
            pos = _first_diff(got[0][1][n], got[k][1][n])
            if pos is None:
                continue
            a, b = int(got[0][0][n][pos]), int(got[k][0][n][pos])
            ndiff = int((got[0][1][n] != got[k][1][n]).sum())
            where = (f"workspace fill {fills()[k].name} differs from fill {fills()[0].name} in output '{n}' at byte offset {pos} "
                     f"(0x{b:02x} against 0x{a:02x}; {ndiff} byte(s) of the output differ)")
            if a == 0x00 and b == 0xFF:
                raise WsFailure("unwritten-output", where + ": both runs still hold what the output was prefilled with - the call "
                                "never wrote the slot")
            raise WsFailure("workspace-dependent", where + ": the call read workspace it had not written")
    return got[0][0]


def run_after(calls_before, call, outputs, ws_bytes, expect, device=None, canon=None):
    """The production pattern: ONE workspace of ws_bytes (the largest call's), seeded-random at first, is handed to every
    b(ws, *outs) of calls_before and then to call(ws, *outs) without being cleared in between; the outputs start as 0xFF. What
    `call` leaves in the outputs must equal `expect` - {name: uint8 array, or (byte offset, uint8 array) for a window of a shared
    output} -, which is what the call gave on its own (run_independent). Bands as there. Raises WsFailure("leftover-dependent")."""
    names = [n for n, _ in outputs]
    with _stream(device):
        ws = guarded(ws_bytes, RANDOM, device)
        outs = [guarded(nb, ALL_FF, device) for _, nb in outputs]
        for b in calls_before:
            b(ws.interior, *[o.interior for o in outs])
        call(ws.interior, *[o.interior for o in outs])
        wsnap, osnaps = ws.snapshot(interior=False), [o.snapshot() for o in outs]
    when = f"after {len(calls_before)} earlier call(s) in the same workspace"
    _check_bands(wsnap, f"the shared workspace of {ws_bytes} bytes", when)
    for n, s in zip(names, osnaps):
        _check_bands(s, f"output '{n}'", when)
    raw = {n: _host(s[2]) for n, s in zip(names, osnaps)}
    got = canon({n: v.copy() for n, v in raw.items()}) if canon else raw
    for n in names:
        if n not in expect:
            continue
        off, want = expect[n] if isinstance(expect[n], tuple) else (0, expect[n])
        want = np.asarray(want, np.uint8).reshape(-1)
        have = got[n][off:off + want.size]
        pos = _first_diff(have, want) if have.size == want.size else 0
        if pos is not None:
            raise WsFailure("leftover-dependent", f"{when}, output '{n}' differs from the call on its own at byte offset {off + pos} "
                            f"(0x{int(have[pos]) if have.size > pos else -1:02x} against 0x{int(want[pos]):02x}; "
                            f"{int((have != want).sum()) if have.size == want.size else want.size} byte(s) differ): the call depends "
                            "on what an earlier call left in the workspace")
    return raw


# ---- the calls themselves, through the C ABI: shared by the test_ws_*_gpu.py files and test_graph_capture_gpu.py ----------------
def encode_image_call(clipmi, model, px):
    """-> (call(ws, out), outputs, ws_bytes) for clipmi_encode_image of the model's vision tower over the device pixels px
    (uint8 / f32 / bf16 [B,3,R,R]); what CLIP.encode_image does for one kernel sequence"""
    from clipmi.model import _DTYPES
    lib, L, B = clipmi._lib, clipmi._lib.lib(), px.shape[0]
    ws_bytes = L.clipmi_encode_image_workspace_bytes(model.vision, B)
    assert ws_bytes > 0, lib.last_error()

    def call(ws, out):
        lib.check(L.clipmi_encode_image(model.vision, model._vblob.data_ptr(), px.data_ptr(), _DTYPES[px.dtype], B, out.data_ptr(), 0,
                                        ws.data_ptr(), ws.numel(), lib.stream_ptr(model.device)), "clipmi_encode_image")
    return call, [("embeddings", B * model.embed_dim * 4)], ws_bytes


def text_tower(model, ids):
    """(the tower trimmed to the longest prompt as CLIP.encode_text builds it, the prompts' int32 ids on the device)"""
    Lp = min(model.context_length, int(ids.argmax(dim=1).max()) + 1)
    tower = type(model.text).from_buffer_copy(model.text)
    tower.tokens = Lp
    import torch
    return tower, ids[:, :Lp].to(device=model.device, dtype=torch.int32).contiguous()


def encode_text_call(clipmi, model, tower, ids_dev):
    """-> (call(ws, out), outputs, ws_bytes) for clipmi_encode_text over text_tower()'s pair"""
    lib, L, Q = clipmi._lib, clipmi._lib.lib(), ids_dev.shape[0]
    ws_bytes = L.clipmi_encode_text_workspace_bytes(tower, Q)
    assert ws_bytes > 0, lib.last_error()

    def call(ws, out):
        lib.check(L.clipmi_encode_text(tower, model._tblob.data_ptr(), ids_dev.data_ptr(), Q, out.data_ptr(), 0, ws.data_ptr(),
                                       ws.numel(), lib.stream_ptr(model.device)), "clipmi_encode_text")
    return call, [("embeddings", Q * model.embed_dim * 4)], ws_bytes


def prompts(model, Q):
    """Q prompts of different lengths as clip.tokenize lays them out: start token, random tokens, the end token (the highest id)"""
    import torch
    ctx, vocab = model.context_length, model.dims["vocab"]
    g = torch.Generator(device="cpu")
    g.manual_seed(77 + Q)
    ids = torch.zeros(Q, ctx, dtype=torch.int64)
    for r, eot in enumerate((5, ctx - 4, 3, 9, ctx // 2)[:Q]):
        ids[r, 0] = vocab - 2
        ids[r, 1:eot] = torch.randint(1, vocab - 2, (eot - 1,), generator=g)
        ids[r, eot] = vocab - 1
    return ids
