"""CPU checks of the instrument tests/test_embed_gpu.py measures the embedding front end with (tests/embed_cases.py): its
references agree with a plain torch f32 evaluation within the very tolerances the GPU tests apply, and its comparison
functions reject what the end-to-end rule of tests/test_encode_gpu.py (err <= 3 x bf16 noise + 1e-3, cosine >= 0.9995)
lets through - measured on the fp32 oracle, that rule does not notice a last patch token without its positional row,
patches 0 and 1 swapped, a last pixel column read as zero, the last 8 pixels of the last row zero, the blue channel
divided by the green channel's std, or a zero class embedding (testing section).

Each mutation is applied to the reference's own output - reference against mutated reference. Required: in tolerance
mode the mutation exceeds the tolerance at least 10 x; in exact mode at least one bit differs."""
import pytest
import torch
import torch.nn.functional as F

import embed_cases as ec

SMALL = ["G1", "G2", "G3", "G4"]


def _f32_rows(image_f32, sd, name):
    """cat(cls, conv) + pos the way oracle/clip_oracle.py encode_image spells it, in f32, on the bf16-rounded weights."""
    d = ec.dims(name)
    w = sd["visual.conv1.weight"].to(torch.bfloat16).float()
    x = F.conv2d(image_f32, w, bias=None, stride=d["P"])
    B = x.shape[0]
    x = x.reshape(B, d["W"], -1).permute(0, 2, 1)
    cls = sd["visual.class_embedding"].reshape(1, 1, -1).expand(B, 1, -1)
    return (torch.cat([cls, x], dim=1) + sd["visual.positional_embedding"]).reshape(B * d["L"], d["W"])


def test_u8_table_equals_plain_f32_evaluation():
    """All 768 (byte, channel) pairs: IEEE f32 evaluation of ((float)byte / 255 - mean) / std, rounded to bf16, is the
    bf16 rounding of the float64 value - so the device's f32 arithmetic has to match the table exactly."""
    table = ec.u8_table()
    byte = torch.arange(256, dtype=torch.float32)[None, :]
    f32 = ((byte / 255.0 - torch.from_numpy(ec.MEAN)[:, None]) / torch.from_numpy(ec.STD)[:, None]).to(torch.bfloat16)
    assert ec.same_bits(f32, table)[0]
    assert len(set(table[0].float().tolist())) > 200          # the table is not degenerate


def test_bf16_rne_rounds_ties_to_even():
    x = [1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8), 1.0 + 2.0 ** -8 + 2.0 ** -30, 0.3]
    want = torch.tensor([1.0, 1.0 + 2.0 ** -6, -1.0, 1.0 + 2.0 ** -7, 0.30078125]).to(torch.bfloat16)
    assert ec.same_bits(ec.bf16_rne(x), want)[0]
    # x[3] is the double rounding that torch's float64 -> f32 -> bf16 gets wrong and one rounding gets right
    assert torch.tensor(x, dtype=torch.float64).to(torch.bfloat16)[3].item() == 1.0


@pytest.mark.parametrize("name", SMALL + ["G5"])
def test_patch_layout_is_conv1_weight_flattened(name):
    """to_patches against torch's unfold (the im2col of a stride-P convolution), and the zero columns."""
    d = ec.dims(name)
    x = ec.exact_pixels(name, 2)
    want = F.unfold(x, kernel_size=d["P"], stride=d["P"]).permute(0, 2, 1).reshape(2 * d["np"], d["k"])
    got = ec.to_patches(x, name)
    assert got.shape == (2 * d["np"], d["patch_k"]) and torch.equal(got[:, :d["k"]], want)
    assert ec.same_bits(got[:, d["k"]:], torch.zeros(2 * d["np"], d["patch_k"] - d["k"]))[0]


def test_u8_pixels_show_every_byte_in_every_channel():
    for name in ec.GEOMS:
        x = ec.u8_pixels(name, 2)
        for c in range(3):
            assert len(torch.unique(x[0, c])) == 256
        assert len(torch.unique(x[1])) == 256


@pytest.mark.parametrize("name", SMALL + ["G5"])
def test_exact_reference_equals_f32_evaluation(name):
    """Exact mode: the float64 reference is representable in f32 and a plain f32 conv2d gives its very bits."""
    B = 3
    sd = ec.vision_state_dict(name, "exact")
    x = ec.exact_pixels(name, B)
    ref = ec.ref_rows(ec.ref_patches(x, name), sd, name)
    ok, bad = ec.rows_exact(_f32_rows(x, sd, name), ref)
    assert ok, f"{bad} elements differ"
    assert ref.abs().max().item() < 2 ** 24 / 8


@pytest.mark.parametrize("name", SMALL + ["G5"])
def test_tolerance_references_satisfy_their_own_tolerances(name):
    B = 3
    d = ec.dims(name)
    sd = ec.vision_state_dict(name, "gauss")
    x = ec.u8_pixels(name, B)
    patches = ec.ref_patches(x, name)
    ref = ec.ref_rows(patches, sd, name)
    c = torch.arange(3).reshape(1, 3, 1, 1).expand_as(x)
    image = ec.u8_table()[c, x.long()].float()               # the pixel values the device multiplies
    ok, ratio = ec.rows_within(_f32_rows(image, sd, name), ref, ec.GEMM_REL)
    assert ok, f"f32 evaluation at {ratio:.3g} of the GEMM tolerance"
    lnw, lnb = sd["visual.ln_pre.weight"], sd["visual.ln_pre.bias"]
    rows32 = ref.float()
    ok, ratio = ec.rows_within(F.layer_norm(rows32, (d["W"],), lnw, lnb, 1e-5), ec.ref_ln(rows32, lnw, lnb), ec.LN_REL)
    assert ok, f"f32 LayerNorm at {ratio:.3g} of the LayerNorm tolerance"


@pytest.mark.parametrize("mutation", ec.MUTATIONS)
@pytest.mark.parametrize("name", SMALL + ["G5"])
def test_tolerance_mode_rejects_mutation(name, mutation):
    """u8 pixels, Gaussian weights: the mutated reference misses the GEMM tolerance by 10 x or more, and a mutation of
    the pixels also changes bits of the patch matrix."""
    B = 3
    sd = ec.vision_state_dict(name, "gauss")
    x = ec.u8_pixels(name, B)
    patches = ec.ref_patches(x, name)
    ref = ec.ref_rows(patches, sd, name)
    if mutation in ec.PIXEL_MUTATIONS:
        mpatches = ec.ref_patches(x, name, mutation)
        assert not ec.same_bits(mpatches, patches)[0]
        mrows = ec.ref_rows(mpatches, sd, name)
    else:
        mrows = ec.ref_rows(patches, sd, name, mutation)
    ok, ratio = ec.rows_within(mrows.float(), ref, ec.GEMM_REL)
    print(f"{name} {mutation}: {ratio:.4g} x the tolerance")
    assert not ok and ratio >= 10.0, f"{mutation}: only {ratio:.3g} x the tolerance"


@pytest.mark.parametrize("mutation", [m for m in ec.MUTATIONS if m != "blue_by_green_std"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name", SMALL + ["G5"])
def test_exact_mode_rejects_mutation(name, dtype, mutation):
    """f32 / bf16 pixels (already normalised: the channel constants play no part, so that mutation has no exact-mode
    form), integer data: at least one bit of the rows differs."""
    B = 3
    sd = ec.vision_state_dict(name, "exact")
    x = ec.exact_pixels(name, B).to(dtype)
    patches = ec.ref_patches(x, name)
    ref = ec.ref_rows(patches, sd, name)
    if mutation in ec.PIXEL_MUTATIONS:
        mpatches = ec.ref_patches(x, name, mutation)
        assert not ec.same_bits(mpatches, patches)[0]
        mrows = ec.ref_rows(mpatches, sd, name)
    else:
        mrows = ec.ref_rows(patches, sd, name, mutation)
    ok, bad = ec.rows_exact(mrows.float(), ref)
    assert not ok and bad >= 1


def test_nan_rows_are_rejected():
    """An unwritten row (the buffers are pre-filled with NaN) fails both comparisons."""
    sd = ec.vision_state_dict("G4", "exact")
    ref = ec.ref_rows(ec.ref_patches(ec.exact_pixels("G4", 1), "G4"), sd, "G4")
    got = ref.float()
    got[5] = float("nan")
    assert not ec.rows_exact(got, ref)[0] and not ec.rows_within(got, ref, ec.GEMM_REL)[0]


@pytest.mark.parametrize("width", sorted(ec.TEXT_TOWERS))
def test_text_references(width):
    t = ec.TEXT_TOWERS[width]
    L, vocab = t["ctx"], t["vocab"]
    sd = ec.text_state_dict(width)
    ids = ec.text_ids(width, 65)
    idx = ec.ref_rowidx(ids)
    assert idx.dtype == torch.int32
    assert idx[0] == 0 and idx[1] == L + L - 1 and idx[2] == 2 * L + 3 and idx[3] == 3 * L and idx[4] == 4 * L + 5
    rows = ec.ref_text_rows(sd, ids).reshape(65, L, width)
    tok, pos = sd["token_embedding.weight"], sd["positional_embedding"]
    assert torch.equal(rows[4, 2], tok[0] + pos[2]) and torch.equal(rows[4, 5], tok[vocab - 1] + pos[5])
    assert torch.equal(rows[9, 7], tok[ids[9, 7]] + pos[7])
    # a shifted positional row changes bits of every row
    shifted = ec.ref_text_rows(sd, ids, "pos_shifted")
    assert (shifted.view(torch.int32) != rows.reshape(-1, width).view(torch.int32)).any(dim=1).all()
