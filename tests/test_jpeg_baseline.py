"""The baseline JPEG writer of tests/jpeg_baseline.py on the CPU: every file it writes with unchanged coefficients decodes, by
Pillow live and by the oracle, to the base file's pixels; the host parser accepts every well-formed case in both stuffing forms
and refuses exactly the listed ones; every table profile is covered or uncovered (csrc/jpeg.hip JpLut.covered) as it is named;
jpeg.pack gives every image the tables its scan names. tests/test_jpeg_baseline_gpu.py runs the same files on the device."""
import collections
import io
import warnings

import numpy as np
import pytest
from PIL import Image

import jpeg_baseline as jb
from clipmi import jpeg_parse
from oracle import jpeg_oracle


def pillow(blob):
    """Pillow's pixels; a warning is an error (a case meant to be well-formed must not draw one)"""
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        return np.asarray(Image.open(io.BytesIO(blob)).convert("RGB"))


def well_formed():
    return [c for c in jb.written() if c.family != "unsupported"]


def test_parity_set_holds_the_cases():
    fams = collections.Counter(c.family for c in jb.written())
    for fam, n in sorted(fams.items()):
        print(f"{fam:12s} {n:4d} files")
    names = {c.name.split("/")[0] for c in jb.written()}
    assert set(jb.PROFILES) <= names and set(jb.ID_CASES) <= names and set(jb.WELL_FORMED_LAYOUTS) <= names
    assert {"quant_123", "sof1", "ri_1", "ri_nondivisor", "ri_row", "ri_all", "ri_more", "fill+ri"} <= {n.split("=")[0] for n in names}
    assert fams["profile"] >= 7 * 14 and fams["ri"] >= 30 and fams["layout"] >= 40 and fams["table_ids"] >= 20
    bases = {c.base for c in well_formed() if c.family == "profile"}
    assert {"37x53_0", "37x53_1", "37x53_2", "37x53_grey", "64x96_0", "64x96_1", "64x96_2", "64x96_grey"} <= bases
    # ri_more: DRI present and no RSTn marker at all; ri_1: one per MCU
    for c in well_formed():
        if c.name.startswith("ri_more"):
            assert b"\xff\xdd" in c.blob and jpeg_parse.parse(c.blob).ri > jpeg_parse.parse(c.blob).mcus() and len(jpeg_parse.parse(c.blob).starts) == 1
        if c.name.startswith("ri_1="):
            assert len(jpeg_parse.parse(c.blob).starts) == jpeg_parse.parse(c.blob).mcus()
        if c.name.startswith("app1_thumb"):
            k = c.blob.index(b"\xff\xe1")
            assert int.from_bytes(c.blob[k + 2:k + 4], "big") == 65535 and b"\xff\xd8" in c.blob[k + 4:k + 65535]


def test_every_profile_is_covered_or_uncovered_as_named():
    """The restated predicate on the 16 counts of every table written, against the profile's name; and the data really uses
    the codes the profile is about: AC symbols under prefix 1016 / 1015 for the edge profiles, under all eight last prefixes
    for second_full, under many prefixes from 0 upward for flat11, 16-bit codes under prefix 0 for flat16."""
    seen = collections.Counter()
    cases = jb.written() + jb.synthetic_cases() + [jb.big_flat16()]
    for c in cases:
        for (cls, tid), (bits, vals) in c.rep["tables"].items():
            prof = c.profile(cls)
            want = jb.NAMED_COVERED[prof]
            if want is not None:
                assert jb.covered(bits) == want, (c.name, cls, prof, bits)
            used = jb.long_prefixes(bits, vals, c.rep["used"][(cls, tid)])
            kind = "ac" if cls else "dc"
            if prof == "edge_covered" and used:
                assert used[0] == 1016
                seen[prof, kind] += 1
            if prof == "edge_uncovered" and used:
                assert used[0] == 1015
                seen[prof, kind] += 1
            if prof == "second_full" and cls and used == list(range(1016, 1024)):
                assert len({l for l in range(11, 17) if bits[l - 1]}) >= 3
                seen[prof, kind] += 1
            if prof == "flat11" and len(used) >= (8 if cls else 2) and used[0] == 0:
                seen[prof, kind] += 1
            if prof == "flat16" and used == [0]:
                seen[prof, kind] += 1
            if prof == "optimal":
                seen[prof, "covered" if jb.covered(bits) else "uncovered"] += 1
    for k, n in sorted(seen.items()):
        print(k, n)
    for prof in ("edge_covered", "edge_uncovered", "flat16", "flat11"):
        assert seen[prof, "ac"] >= 10 and seen[prof, "dc"] >= 1, (prof, seen)
    assert seen["second_full", "ac"] >= 3
    # the shapes themselves, as the issue names them
    assert jb.profile_lengths("edge_covered", 1, 20) == [1, 2, 3, 4, 5, 6] + [10] * 8 + [16] * 6
    assert jb.profile_lengths("edge_uncovered", 1, 20) == [1, 2, 3, 4, 5, 6] + [10] * 7 + [16] * 7
    bits = [jb.profile_lengths("edge_covered", 1, 20).count(l) for l in range(1, 17)]
    codes = jb._codes(bits, list(range(20)))
    assert [codes[s][0] for s in range(6, 14)] == list(range(1008, 1016)) and codes[14] == (1016 << 6, 16)
    for n in (20, 60, 100, 162, 200):
        for cls in (0, 1):
            for prof in jb.PROFILES:
                if prof != "optimal" and (cls or n <= 16) and (prof != "annexk" or n <= 162):
                    ls = jb.profile_lengths(prof, cls, n)
                    jb.check_canonical([ls.count(l) for l in range(1, 17)])
                    assert ls == sorted(ls) and len(ls) == n


def test_written_files_decode_to_the_base_files_pixels():
    """Four things equal for every well-formed case: the oracle on the written file, Pillow on it, Pillow on the base file,
    and - for the bases out of tests/golden/jpeg_cases.npz - the base file's committed Pillow pixels."""
    B = jb.bases()
    live = {n: pillow(b) for n, (b, _) in B.items()}
    committed = 0
    for n, (b, rgb) in B.items():
        if rgb is not None:
            assert np.array_equal(live[n], rgb), n
    for c in well_formed():
        got = pillow(c.blob)
        assert np.array_equal(got, live[c.base]), c.name
        assert np.array_equal(jpeg_oracle.decode(c.blob), got), c.name
        if B[c.base][1] is not None:
            assert np.array_equal(got, B[c.base][1]), c.name
            committed += 1
    assert committed >= 100
    big = jb.big_flat16()
    assert np.array_equal(pillow(big.blob), pillow(big.base_blob)) and np.array_equal(jpeg_oracle.decode(big.blob), pillow(big.blob))


def test_parser_accepts_every_well_formed_case_and_refuses_the_listed_ones():
    accepted = set()
    for c in jb.written():
        for ks in (False, True):
            try:
                p = jpeg_parse.parse(c.blob, keep_stuffing=ks)
            except jpeg_parse.Unsupported as e:
                assert c.family == "unsupported", f"{c.name} (keep_stuffing={ks}): {e}"
                continue
            assert c.family != "unsupported", f"{c.name}: a listed layout was accepted"
            accepted.add(c.name)
            o = jpeg_oracle.parse(c.blob)
            assert (p.width, p.height, p.ri) == (o["width"], o["height"], o["ri"])
            if p.stuffed:
                assert p.stream.replace(b"\xff\x00", b"\xff") == o["stream"] and not p.ri
            else:
                assert p.stream == o["stream"] and (p.starts is None or list(p.starts) == o["starts"])
    assert accepted == {c.name for c in well_formed()}
    listed = {c.opt["layout"] for c in jb.written() if c.family == "unsupported"}
    assert listed == set(jb.EXPECTED_UNSUPPORTED)
    # a file that ends with its EOI is only sliced, fill bytes in front of the EOI or not: they are not the segment's
    n = 0
    for c in well_formed():
        lay = c.opt.get("layout", ())
        if not c.opt.get("ri") and "trailing" not in lay:
            p = jpeg_parse.parse(c.blob, keep_stuffing=True)
            assert p.stuffed == 1 and not p.stream.endswith(b"\xff")
            n += "fill" in lay
    assert n >= 4


def _record(bits, vals, cls):
    return (bytes(bits) + bytes(vals)).ljust(272, b"\0") + bytes([cls]) + b"\0" * 15


def test_pack_gives_every_image_the_tables_its_scan_names():
    """One batch of every well-formed case and a few plain Pillow files: dc_tbl / ac_tbl of every image index the record of
    the table its scan names (read back from the file by the oracle's parser), identical tables are stored once, and most
    tables of the batch differ."""
    from clipmi import jpeg
    blobs = [c.blob for c in well_formed()] + [b for b, _ in list(jb.bases().values())[:6]]
    items = [jpeg_parse.parse(b) for b in blobs]
    recs, tables = jpeg.pack(items)[:2]
    stored = [tables[k].tobytes() for k in range(len(tables))]
    assert len(set(stored)) == len(stored)
    distinct = set()
    for b, r in zip(blobs, recs):
        o = jpeg_oracle.parse(b)
        for ci, (_, td, ta) in enumerate(o["scan"]):
            for cls, tid, idx in ((0, td, r["dc_tbl"][ci]), (1, ta, r["ac_tbl"][ci])):
                want = _record(*o["huff"][(cls, tid)], cls)
                assert stored[int(idx)] == want
                distinct.add(want)
    assert distinct == set(stored) and len(stored) >= 200
    three = [r for b, r in zip(blobs, recs) if len({*r["dc_tbl"]}) == 3 and len({*r["ac_tbl"]}) == 3]
    assert len(three) >= 6                                  # three distinct DC / AC pairs in one image


def test_synthetic_families_are_what_they_claim():
    """Long blocks are longer than a subsequence of 1 024 bits and shorter than two; the extreme files hold the symbols they
    are named after, at up to 31 bits; the oracle equals Pillow live on every synthetic file it does not report, and reports
    only files of the extreme family."""
    fams = collections.Counter()
    for c in jb.synthetic_cases():
        fams[c.family] += 1
        bb = c.rep["block_bits"]
        if "long_blocks" in c.name or c.family == "long_blocks":
            assert 1024 < min(bb) and max(bb) < 2048, (c.name, min(bb), max(bb))
        if c.family == "extreme" and c.name[:2] in ("ac", "dc"):
            s, cls = int(c.name[2:4]), int(c.name[:2] == "ac")
            syms = set().union(*[u for (k, _), u in c.rep["used"].items() if k == cls])
            assert any(x & 15 == s for x in syms), c.name
            if "flat16" in c.name:
                (bits, vals), = [t for (k, _), t in c.rep["tables"].items() if k == cls][:1]
                assert bits[15] == len(vals) and 16 + s <= 31
        if c.family == "dc_walk":
            assert all(set(range(11)) <= u for (k, _), u in c.rep["used"].items() if k == 0), c.name
        ref = pillow(c.blob)
        try:
            assert np.array_equal(jpeg_oracle.decode(c.blob), ref), c.name
        except jpeg_oracle.Reported:
            assert c.family == "extreme", c.name
        for ks in (False, True):
            jpeg_parse.parse(c.blob, keep_stuffing=ks)
    for fam, n in sorted(fams.items()):
        print(f"{fam:12s} {n:4d} files")
    assert fams["long_blocks"] >= 2 and fams["extreme"] >= 60 and fams["overrun"] >= 12


def test_progressive_writer_under_the_profiles_round_trips():
    """jpeg_progressive.write(tables=...): Pillow, the progressive restatement and the base file agree, and the tables have
    the shape asked for (all codes at 16 bits under flat16)"""
    import jpeg_progressive
    cases = jb.progressive_cases()
    assert len(cases) == 12
    for name, blob, base in cases:
        ref = pillow(blob)
        assert np.array_equal(ref, pillow(base)), name
        assert np.array_equal(jpeg_progressive.decode(blob), ref), name
        p = jpeg_parse.parse_progressive(blob)
        recs = {t for s in p.scans for t in (s.dc or s.ac) if t is not None}
        want = jb.NAMED_COVERED[name.split("/")[0]]
        assert all(jb.covered(list(t[:16])) == want for t in recs), name
        if name.startswith("flat16"):
            assert all(t[15] == sum(t[:16]) for t in recs), name
