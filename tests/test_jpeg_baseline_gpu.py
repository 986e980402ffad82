"""The device JPEG decoder (csrc/jpeg.hip) on baseline files Pillow's encoder never writes (tests/jpeg_baseline.py): Huffman
tables of every shape jp_lookup distinguishes, table and quantisation ids 0-3, SOF1, any restart interval, every header layout
the parser accepts, blocks longer than a subsequence, symbols of up to 31 bits, runs past coefficient 63. Bit for bit against
Pillow live, each file plain and with its byte stuffing left to the device. For a well-formed file a non-zero status is a
failure here, not a fallback."""
import collections
import io

import numpy as np
import pytest
from PIL import Image

import jpeg_baseline as jb
from clipmi import jpeg, jpeg_parse
from oracle import jpeg_oracle
from test_jpeg import encode, smooth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_ref = {}


def pillow(blob):
    if blob not in _ref:
        _ref[blob] = np.asarray(Image.open(io.BytesIO(blob)).convert("RGB"))
    return _ref[blob]


def device(blobs, keep_stuffing):
    """-> (pixels of every file as the device left them, status of every file); every file must pass the parser"""
    items = [jpeg_parse.parse(b, keep_stuffing=keep_stuffing) for b in blobs]
    out, recs, status = jpeg.decode_device(items, DEV)
    st, host = status.cpu().numpy(), out.cpu().numpy()
    pix = [host[int(r["out_off"]):int(r["out_off"]) + int(r["height"]) * int(r["width"]) * 3].reshape(int(r["height"]), int(r["width"]), 3)
           for r in recs]
    return pix, [int(s) for s in st[:len(blobs)]]


def both_forms(cases):
    """Every case through the device plain and with keep_stuffing: status 0 and Pillow's pixels"""
    for ks in (False, True):
        pix, st = device([c.blob for c in cases], ks)
        bad = [(c.name, s) for c, s in zip(cases, st) if s]
        assert not bad, f"keep_stuffing={ks}: non-zero status for well-formed files: {bad[:10]} ({len(bad)} of {len(cases)})"
        wrong = [c.name for c, g in zip(cases, pix) if not np.array_equal(g, pillow(c.blob))]
        assert not wrong, f"keep_stuffing={ks}: status 0 with pixels that are not Pillow's: {wrong[:10]} ({len(wrong)} of {len(cases)})"


@pytest.mark.parametrize("family", ["profile", "table_ids", "quant_ids", "sof1", "ri", "layout"])
def test_every_well_formed_case_returns_pillows_pixels(family):
    cases = [c for c in jb.written() if c.family == family]
    assert len(cases) >= 14
    for c in cases:                                        # (the coefficients are the base file's: so are the pixels)
        assert np.array_equal(pillow(c.blob), pillow(jb.bases()[c.base][0])), c.name
    both_forms(cases)


def test_dc_differences_of_every_category_under_every_profile():
    both_forms([c for c in jb.synthetic_cases() if c.family == "dc_walk"])


def test_one_batch_mixes_every_case_with_plain_pillow_files():
    """Several hundred distinct tables in one call, the cases in a shuffled order between plain Pillow files"""
    rng = np.random.default_rng(3)
    cases = [c for c in jb.written() if c.family != "unsupported"] + [c for c in jb.synthetic_cases() if c.family in ("dc_walk", "long_blocks")]
    cases = [cases[k] for k in rng.permutation(len(cases))]
    for k in range(6):
        c = jb.Case("plain", f"pillow{k}", None, {})
        c.blob = encode(smooth(rng, 30 + 11 * k, 70 - 7 * k), quality=70 + 5 * k, subsampling=k % 3, optimize=bool(k & 1))
        cases.insert(1 + 40 * k, c)
    assert len(jpeg.pack([jpeg_parse.parse(c.blob) for c in cases])[1]) >= 200
    both_forms(cases)


def test_flat16_stream_of_many_chunks():
    """160 x 240, 4:4:4, every symbol a 16-bit code the bit-by-bit walk finds: a stream of more than 128 subsequences x several
    chunks, with blocks that straddle subsequences"""
    big = jb.big_flat16()
    assert len(jpeg_parse.parse(big.blob).stream) > 4 * 128 * (1024 // 8)
    assert max(big.rep["block_bits"]) > 1024
    assert np.array_equal(pillow(big.blob), pillow(big.base_blob))
    both_forms([big])


def test_blocks_longer_than_a_subsequence():
    """Every block 63 AC coefficients of category 9 under flat16 (25 bits each): the shortest block exceeds 1 024 bits, the
    longest stays under 2 048, so every second subsequence holds no block end, over several chunks of 128 subsequences. (The
    issue's category 10 cannot come back: 63 coefficients >= 512 put the block's pixels at >= 508 rms by Parseval, outside the
    IDCT's [-512, 511] for any signs - that file is in the extreme family below, status 4 on the device and in the oracle.)"""
    cases = [c for c in jb.synthetic_cases() if c.family == "long_blocks"]
    assert len(cases) >= 2
    for c in cases:
        bb = c.rep["block_bits"]
        print(c.name, "block bits", min(bb), "to", max(bb), "stream bytes", len(jpeg_parse.parse(c.blob).stream))
        assert 1024 < min(bb) and max(bb) < 2048
        assert len(jpeg_parse.parse(c.blob).stream) > 3 * 128 * (1024 // 8)
        assert np.array_equal(jpeg_oracle.decode(c.blob), pillow(c.blob))
    both_forms(cases)


def test_extreme_categories_agree_with_the_oracle_file_by_file():
    """Single AC coefficients and DC differences of categories 11-15 under Annex K-shaped tables extended with those symbols and
    under flat16 (16-bit code + up to 15 value bits: jp_entry at 31), and the 63 x category 10 long-block file. The device
    returns status 0 with Pillow's pixels or status 4, and 4 exactly where jpeg_oracle.decode raises Reported.
    Counts (oracle, CPU; the device must give the same): 61 files, 44 with status 0, 17 with status 4 - at a step of 1: AC 11 and
    12 status 0 (4 + 4 files), AC 13-15 status 4 (12: a single coefficient >= 4 096 leaves [-512, 511] whatever the rest of the
    block, its basis function's 1-norm x 511 being 3 705 at most), DC 11-13 status 0 (6), DC 14-15 status 4 (4: a difference
    >= 8 192 cannot join two DC values inside the range); with a step of 0 at the coefficient every category status 0 (20 AC,
    10 DC): the symbol is decoded and skipped correctly, the value does not reach the pixels; the category 10 long-block file 4."""
    cases = [c for c in jb.synthetic_cases() if c.family == "extreme"]
    want = []
    for c in cases:
        try:
            assert np.array_equal(jpeg_oracle.decode(c.blob), pillow(c.blob)), c.name
            want.append(0)
        except jpeg_oracle.Reported:
            want.append(4)
    assert (len(cases), want.count(0), want.count(4)) == (61, 44, 17)
    for ks in (False, True):
        pix, st = device([c.blob for c in cases], ks)
        print(f"keep_stuffing={ks}: status counts {sorted(collections.Counter(st).items())}")
        assert st == want, [(c.name, s, w) for c, s, w in zip(cases, st, want) if s != w]
        ok = collections.Counter()
        for c, g, s in zip(cases, pix, st):
            if s == 0:
                assert np.array_equal(g, pillow(c.blob)), c.name
                ok[c.name.split("/")[0]] += 1
        assert all(ok[f"{k}{s}"] >= 1 for k in ("ac", "dc") for s in range(11, 16)), ok


def test_run_past_coefficient_63():
    """The rule, from live Pillow: libjpeg stores the value of a run that passes coefficient 63 at index 63 (jutils.c
    jpeg_natural_order's 16 guard entries) and ends the block; Pillow returns pixels without an error. The oracle does the
    same, so the device gives Pillow's pixels with status 0 - or a status the oracle also reports (none in this corpus)."""
    cases = [c for c in jb.synthetic_cases() if c.family == "overrun"]
    assert len(cases) >= 12
    want = []
    for c in cases:
        assert not np.array_equal(pillow(c.blob), pillow(jb.bases()[c.name.split("/")[1]][0])), c.name       # (the rewrite shows)
        try:
            assert np.array_equal(jpeg_oracle.decode(c.blob), pillow(c.blob)), c.name
            want.append(0)
        except jpeg_oracle.Reported:
            want.append(4)
    for ks in (False, True):
        pix, st = device([c.blob for c in cases], ks)
        assert st == want, [(c.name, s, w) for c, s, w in zip(cases, st, want) if s != w]
        for c, g, s in zip(cases, pix, st):
            assert s or np.array_equal(g, pillow(c.blob)), c.name


def test_progressive_decoder_under_the_same_profiles():
    """The progressive decoder keeps its own table form (JppLut) and walks every code longer than 10 bits bit by bit: the
    split-band script under flat16, flat11 and the two edge profiles, through decode_progressive_files directly"""
    cases = jb.progressive_cases()
    got = jpeg.decode_progressive_files([b for _, b, _ in cases], DEV)
    for (name, blob, base), g in zip(cases, got):
        assert g is not None, name
        assert np.array_equal(g, pillow(blob)) and np.array_equal(g, pillow(base)), name
