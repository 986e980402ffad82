"""JPEG files of luma sampling 1x2, 4x1, 1x4 and RGB-coded files on the CPU: the host parsers' opt-in (jpeg_parse.parse(layouts=True),
parse_progressive(layouts=True)), the forged fixtures and their CPU restatement (tests/jpeg_layouts.py) against Pillow live and the
committed Pillow pixels, and the way the sampling factors and the colour transform travel into the device's records."""
import inspect
import io
import os

import numpy as np
import pytest
from PIL import Image

import clipmi
import jpeg_corpus
import jpeg_layouts as jl
from clipmi import jpeg_parse

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_layout_cases.npz")
FORMS = ("baseline", "restart", "progressive")
_fixtures = {}


def fixtures(form):
    if form not in _fixtures:
        _fixtures[form] = jl.fixtures(form)
    return _fixtures[form]


def parser(progressive):
    return jpeg_parse.parse_progressive if progressive else jpeg_parse.parse


@pytest.mark.parametrize("form", FORMS)
def test_parsers_take_every_fixture_with_the_switch_and_none_without(form):
    fx = fixtures(form)
    accepted = 0
    for f in fx:
        parse = parser(f.progressive)
        with pytest.raises(jpeg_parse.Unsupported, match="RGB-coded JPEG" if f.rgb else "sampling factors"):
            parse(f.blob)
        with pytest.raises(jpeg_parse.Unsupported):
            parse(f.blob, layouts=False)
        for kw in ({},) if f.progressive else ({}, dict(keep_stuffing=True)):
            p = parse(f.blob, layouts=True, **kw)
            hs, vs = f.hs_vs()
            assert (p.width, p.height, p.ncomp, p.hs, p.vs, p.transform) == (f.W, f.H, 3, hs, vs, int(f.rgb)), f.name
            mcus = -(-f.W // (8 * hs)) * -(-f.H // (8 * vs))
            assert (p.mcus(), p.blocks()) == (mcus, mcus * (hs * vs + 2)), f.name
            assert jpeg_parse.is_layout(p)
            if form == "restart":
                assert p.ri == 3 and len(p.starts) == -(-mcus // 3)
            if kw:
                assert p.stuffed == (0 if form == "restart" else 1)
        # the relabelled header holds the source file's data: as many MCUs, as many blocks
        if f.layout in jl.FACTORS:
            (h, w), sub = jl.source_shape(f.layout, f.H, f.W)
            assert jl.pillow(f.src).shape == (h, w, 3) and -(-w // 16) * -(-h // (8 * sub)) == p.mcus(), f.name
        accepted += 1
    assert accepted == len(fx) == len(jl.PROGRESSIVE_SPECS if form == "progressive" else jl.SPECS)
    layouts = {(f.layout, f.rgb) for f in fx}
    assert {("1x2", False), ("4x1", False), ("1x4", False), ("1x1", True), ("2x2", True), ("1x2", True)} <= layouts


def test_ordinary_files_parse_the_same_with_the_switch():
    rng = np.random.default_rng(2)
    for sub in (0, 1, 2):
        for prog in (False, True):
            blob = jl.encode(jl.smooth(rng, 37, 53), quality=80, subsampling=sub, progressive=prog)
            a, b = parser(prog)(blob), parser(prog)(blob, layouts=True)
            assert (a.hs, a.vs, a.transform) == (b.hs, b.vs, b.transform) == ((1, 2, 2)[sub], (1, 1, 2)[sub], 0)
            assert not jpeg_parse.is_layout(b)
    g = jpeg_parse.parse(jl.encode(jl.smooth(rng, 20, 30)[..., 0], quality=70), layouts=True)
    assert (g.ncomp, g.hs, g.vs, g.transform) == (1, 1, 1, 0) and not jpeg_parse.is_layout(g)


def test_what_stays_refused_with_the_switch():
    rng = np.random.default_rng(3)
    for prog in (False, True):
        parse = parser(prog)
        base = jl.encode(jl.smooth(rng, 48, 64), quality=80, subsampling=0, progressive=prog)
        parse(base, layouts=True)
        for luma in (0x42, 0x24, 0x31, 0x13, 0x33, 0x32, 0x23, 0x34, 0x43, 0x44):           # 4x2, 2x4, every factor 3, 4x4
            with pytest.raises(jpeg_parse.Unsupported, match="sampling factors"):
                parse(jl.relabel(base, luma=luma), layouts=True)
        for comp in (1, 2):                                                            # chroma 2x1, 1x2 - under luma 1x1 and 2x2
            for chroma in (0x21, 0x12):
                with pytest.raises(jpeg_parse.Unsupported, match="sampling factors"):
                    parse(jl.relabel(base, luma=chroma, comp=comp), layouts=True)
                with pytest.raises(jpeg_parse.Unsupported, match="sampling factors"):
                    parse(jl.relabel(jl.relabel(base, luma=0x22), luma=chroma, comp=comp), layouts=True)
        buf = io.BytesIO()
        Image.fromarray(jl.smooth(rng, 40, 40)).convert("CMYK").save(buf, format="JPEG", progressive=prog)
        with pytest.raises(jpeg_parse.Unsupported, match="frame"):
            parse(buf.getvalue(), layouts=True)
        for sub in (1, 2):                                                             # two chroma columns at 2x sampling
            with pytest.raises(jpeg_parse.Unsupported, match="too narrow"):
                parse(jl.encode(jl.smooth(rng, 40, 4), quality=80, subsampling=sub, progressive=prog), layouts=True)
            with pytest.raises(jpeg_parse.Unsupported, match="too narrow"):
                parse(jl.rgb_coded(jl.encode(jl.smooth(rng, 40, 3), quality=80, subsampling=sub, progressive=prog)), layouts=True)
        # ... a rule of 2x sampling only: one column wide at 1x2, 4x1 and 1x4 is taken
        for layout, (H, W) in (("1x2", (9, 1)), ("4x1", (8, 1)), ("1x4", (9, 1))):
            if not prog or layout == "1x2":
                assert parse(jl.forge(layout, H, W, rng, progressive=prog)[0], layouts=True).width == 1
    # every header refused for another reason stays refused: a progressive file with restart intervals, 12-bit precision
    with pytest.raises(jpeg_parse.Unsupported, match="restart intervals"):
        jpeg_parse.parse_progressive(jl.forge("1x2", 40, 40, rng, progressive=True, restart_marker_blocks=2)[0], layouts=True)
    blob = jl.forge("1x2", 40, 40, rng)[0]
    s = jl._sof(blob)
    with pytest.raises(jpeg_parse.Unsupported, match="frame header"):
        jpeg_parse.parse(blob[:s + 4] + b"\x0c" + blob[s + 5:], layouts=True)


def test_adobe_and_component_id_rules():
    """jdapimin.c default_decompress_parms: JFIF wins; else Adobe's transform byte (0: RGB); else the ids R, G, B"""
    rng = np.random.default_rng(4)
    base = jl.encode(jl.smooth(rng, 24, 32), quality=80, subsampling=0)
    adobe = jl.rgb_coded(base)
    assert jpeg_parse.parse(adobe, layouts=True).transform == 1
    ycc = adobe.replace(jl.ADOBE_RGB, jl.ADOBE_RGB[:-1] + b"\x01")
    assert jpeg_parse.parse(ycc).transform == 0 and np.array_equal(jl.pillow(ycc), jl.pillow(base))
    both = base[:2] + jl.ADOBE_RGB + base[2:]                 # JFIF and Adobe transform 0: YCbCr
    assert jpeg_parse.parse(both).transform == 0 and np.array_equal(jl.pillow(both), jl.pillow(base))
    s = jl._sof(base)
    ids = bytearray(base[:2] + base[4 + ((base[4] << 8) | base[5]):])      # no JFIF, no Adobe; ids R G B in frame and scan header
    s -= len(base) - len(ids)
    sos = ids.index(b"\xff\xda")
    for c, v in enumerate(b"RGB"):
        ids[s + 10 + 3 * c] = v
        ids[sos + 5 + 2 * c] = v
    ids = bytes(ids)
    with pytest.raises(jpeg_parse.Unsupported, match="RGB-coded JPEG"):
        jpeg_parse.parse(ids)
    assert jpeg_parse.parse(ids, layouts=True).transform == 1
    assert np.array_equal(jl.pillow(ids), jl.pillow(adobe)) and not np.array_equal(jl.pillow(ids), jl.pillow(base))


def test_parser_never_accepts_a_mutated_header_pillow_refuses():
    """jpeg_corpus.header_mutations (one replaced byte each, from offset 2 to the end of the first SOS header) over fixtures of
    every new layout: a file the parsers let through with layouts=True, Pillow loads."""
    rng = np.random.default_rng(6)
    bases = [(f"{layout}{' rgb' if rgb else ''}{' progressive' if kw.get('progressive') else ''}", kw.get("progressive", False),
              jl.forge(layout, H, W, rng, rgb=rgb, **kw)[0])
             for layout, H, W, rgb, kw in (("1x2", 9, 17, False, {}), ("4x1", 8, 33, False, {}), ("1x4", 33, 8, False, dict(restart_marker_blocks=2)),
                                           ("1x1", 9, 10, True, {}), ("2x2", 17, 24, True, {}), ("1x2", 16, 24, False, dict(progressive=True)),
                                           ("4x1", 8, 32, True, dict(progressive=True)))]
    accepted, total, wrong = 0, 0, []
    for name, prog, blob in bases:
        for fam, _, mutated in jpeg_corpus.header_mutations([(name, blob)]):
            total += 1
            try:
                parser(prog)(mutated, layouts=True)
            except jpeg_parse.Unsupported:
                continue
            accepted += 1
            if jpeg_corpus.pillow(mutated) is None:
                wrong.append((fam, name))
    assert not wrong, f"{len(wrong)} files the parser accepts and Pillow refuses, e.g. {wrong[:8]}"
    assert total > 10000 and accepted > 2000


@pytest.mark.parametrize("form", FORMS)
def test_restatement_equals_pillow_live(form):
    n = 0
    for f in fixtures(form):
        assert np.array_equal(f.restate(), jl.pillow(f.blob)), f.name
        n += 1
    assert n == len(jl.PROGRESSIVE_SPECS if form == "progressive" else jl.SPECS)


def test_restatement_and_pillow_equal_the_committed_pixels():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_jpeg_layouts_golden", os.path.join(os.path.dirname(GOLDEN), "make_jpeg_layouts_golden.py"))
    maker = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(maker)
    d = np.load(GOLDEN)
    assert int(d["n"]) == len(maker.CASES) >= 20 and os.path.getsize(GOLDEN) <= os.path.getsize(os.path.join(os.path.dirname(GOLDEN), "jpeg_cases.npz"))
    for i, (form, layout, H, W, rgb, noise) in enumerate(maker.CASES):
        blob = d[f"file_{i}"].tobytes()
        src = jl.source_of(blob, layout, H, W, rgb)         # (the Pillow file it was forged from, as far as the oracle's parser cares)
        ref = d[f"rgb_{i}"]
        assert ref.shape == (H, W, 3)
        assert np.array_equal(jl.pillow(blob), ref), str(d["names"][i])
        got = jl.restate_progressive(blob) if form == "progressive" else jl.restate_baseline(src, layout, H, W, rgb)
        assert np.array_equal(got, ref), str(d["names"][i])
        assert jpeg_parse.is_layout(parser(form == "progressive")(blob, layouts=True))


def test_worker_regions_and_both_record_types_carry_the_factors_and_the_flag(tmp_path):
    """What decode_worker.stage_jpeg / stage_jpeg_progressive lay out with layouts=True, read back by device_stage.jpeg_records /
    progressive_records, is what jpeg.pack / pack_progressive build from the parsed files (the pattern of
    test_jpeg.test_worker_regions_and_the_records_built_from_them), sampling factors and colour transform included."""
    from clipmi import decode_worker as dw
    from clipmi import device_stage, jpeg
    rng = np.random.default_rng(12)
    specs = [("1x2", 60, 45, False), ("4x1", 40, 70, False), ("1x4", 70, 40, True), ("2x2", 50, 60, True), ("2x1", 30, 40, False)]
    cap, n_px = 1 << 16, 224
    for prog, stage, records, pack, parse in ((False, dw.stage_jpeg, device_stage.jpeg_records, jpeg.pack, jpeg_parse.parse),
                                              (True, dw.stage_jpeg_progressive, device_stage.progressive_records, jpeg.pack_progressive,
                                               jpeg_parse.parse_progressive)):
        sizes = [("1x2", 64, 48, False), ("4x1", 32, 64, False), ("1x4", 64, 32, True), ("2x2", 50, 60, True), ("2x1", 30, 40, False)] if prog else specs
        big = np.zeros(len(sizes) * cap, np.uint8)
        items = []
        for k, (layout, H, W, rgb) in enumerate(sizes):
            path = str(tmp_path / f"{int(prog)}{k}.jpg")
            with open(path, "wb") as f:
                f.write(jl.forge(layout, H, W, rng, rgb=rgb, progressive=prog, **(dict(restart_marker_blocks=2) if k == 1 and not prog else {}))[0])
            region = big[k * cap:(k + 1) * cap]
            if k < 4:
                with pytest.raises(jpeg_parse.Unsupported):
                    stage(path, n_px, region)                   # without the switch: Pillow's, as ever
            got = stage(path, n_px, region, layouts=True)
            assert got[:2] == (W, H) and 0 < got[2] <= cap
            assert stage(path, n_px, big[k * cap:k * cap + 256], layouts=True)[2] < 0 and stage(path, n_px, region, layouts=True) == got
            items.append(parse(open(path, "rb").read(), layouts=True, **({} if prog else dict(keep_stuffing=True))))
            ints = np.frombuffer(region, np.int32, count=dw.JPEG_HDR_INTS)
            assert (ints[dw.HDR.HS], ints[dw.HDR.VS], ints[dw.HDR.TRANSFORM], ints[dw.HDR.LAYOUT]) == \
                (items[-1].hs, items[-1].vs, int(rgb), int(k < 4)) and not ints[26:].any()
        assert list(device_stage._headers(big, len(sizes), cap, np.arange(len(sizes)))[:, dw.HDR.LAYOUT]) == [1, 1, 1, 1, 0]
        recs, *_ = records(big, len(sizes), cap, np.arange(len(sizes)), np.arange(len(sizes)), n_px)
        with pytest.raises(jpeg_parse.Unsupported):
            pack(items)                                         # opt-in here too
        ref = pack(items, layouts=True)[0]
        for f in ("width", "height", "ncomp", "hs", "vs", "reserved", "coef_off", "out_off", "quant"):
            assert np.array_equal(recs[f], ref[f]), (prog, f)
        flag = ref["reserved"][:, 0] if prog else ref["reserved"]
        assert list(flag) == [0, 0, 1, 1, 0] and list(ref["hs"]) == [1, 4, 1, 2, 2] and list(ref["vs"]) == [2, 1, 4, 2, 1]
        if prog:
            assert not ref["reserved"][:, 1:].any()
        assert pack(items[4:])[0]["hs"][0] == 2                  # an ordinary file needs no switch


def test_decode_workers_take_the_files_only_with_the_mode_bit(tmp_path):
    """The worker protocol: with LAYOUTS_BIT in the request's mode the two JPEG stagers run with layouts=True; without it the
    files come back as Pillow's pixels, as before."""
    from clipmi import decode_worker as dw
    from clipmi import device_stage
    rng = np.random.default_rng(14)
    files = [jl.forge("1x2", 60, 45, rng)[0], jl.forge("4x1", 32, 64, rng, rgb=True, progressive=True)[0],
             jl.encode(jl.smooth(rng, 40, 50), quality=80, subsampling=2), jl.forge("1x4", 70, 40, rng)[0]]
    paths = []
    for k, b in enumerate(files):
        paths.append(str(tmp_path / f"{k}.jpg"))
        with open(paths[-1], "wb") as f:
            f.write(b)
    assert dw.LAYOUTS_BIT not in [k.bit for k in dw.PARSED + (dw.FULL_SIZE,)] and dw.LAYOUTS_STAT == "jpeg_layout_files"
    want = {2 | 4: {2: dw.KIND_BASELINE}, 2 | dw.LAYOUTS_BIT: {0: dw.KIND_BASELINE, 2: dw.KIND_BASELINE, 3: dw.KIND_BASELINE},
            2 | 4 | dw.LAYOUTS_BIT: {0: dw.KIND_BASELINE, 1: dw.KIND_PROGRESSIVE, 2: dw.KIND_BASELINE, 3: dw.KIND_BASELINE}}
    with clipmi.pipeline.DecodePool(2) as pool:
        for mode, kinds in want.items():
            (view, good, big, full), ok, bad = pool.decode(paths, 32, copy=False, full_cap=1 << 16, full_mode=mode)
            assert good.all() and not bad
            assert {s: v[0] for s, v in full.items()} == kinds, mode
            hd = device_stage._headers(big, len(paths), 1 << 16, np.array(sorted(full), dtype=np.int64))
            assert int(hd[:, dw.HDR.LAYOUT].sum()) == len(kinds) - 1 and list(hd[:, dw.HDR.KIND]) == [kinds[s] for s in sorted(full)]
            for s in range(len(paths)):                          # the others: Pillow's transform in the slot
                if s not in full:
                    assert np.array_equal(view[s], dw.load_uint8(paths[s], 32))
            del view, big


def test_the_switch_is_a_keyword_and_off_by_default(monkeypatch):
    from clipmi import device_stage, jpeg, pipeline
    sig = inspect.signature(pipeline.encode_files)
    assert sig.parameters["device_jpeg_layouts"].default is None
    for fn in (jpeg_parse.parse, jpeg_parse.parse_progressive, jpeg.pack, jpeg.pack_progressive, jpeg.decode_device, jpeg.decode_files,
               jpeg.decode_progressive_device, jpeg.decode_progressive_files, jpeg.stage_transform, jpeg.transform_files):
        assert inspect.signature(fn).parameters["layouts"].default is False, fn.__name__
    monkeypatch.delenv("CLIPMI_DEVICE_JPEG_LAYOUTS", raising=False)
    assert device_stage.jpeg_layouts_default() is False
    for v, on in (("", False), ("0", False), ("1", True)):
        monkeypatch.setenv("CLIPMI_DEVICE_JPEG_LAYOUTS", v)
        assert device_stage.jpeg_layouts_default() is on
    assert "CLIPMI_DEVICE_JPEG_LAYOUTS" in clipmi.indexer.__doc__
