"""The CPU part of the attention tests (tests/attention_exact.py): every condition that the exact classes and the per-element
bound rest on is a property of the data and its float64 reference, and is checked here without a GPU - the builders assert
margins, exact ties, distinct rows, 24-bit sums and bf16-exact expectations as they build - together with float32 models of the
kernels' documented rounding points: the models must reproduce the exact classes to the bit and stay inside the random-data
bound, and a model that truncates P to bf16 instead of rounding it must not."""
import ctypes as C

import pytest
import torch

import attention_exact as ax


def test_case_list_reaches_every_instantiation():
    reached = {ax.instantiation(s[1], s[3], f) for s in ax.exact_shapes() for f in s[4]}
    assert reached == ax.ALL_INSTANTIATIONS
    shapes = ax.exact_shapes()
    assert {s[1] for s in shapes if s[1] <= 80} >= {1, 5, 15, 16, 17, 31, 32, 33, 48, 49, 50, 51, 52, 53, 64, 65, 77, 79, 80}
    assert {s[1] for s in shapes if s[1] > 80} == {81, 96, 127, 128, 129, 192, 197, 257, 577}
    assert {s[0] * s[2] for s in shapes} >= {1, 3, 5, 21} and {s[2] for s in shapes} >= {1, 2, 3, 12}
    assert ax.MANY_ITEMS[0] * ax.MANY_ITEMS[2] > ax.RESIDENT_52X4 and ax.instantiation(ax.MANY_ITEMS[1], 0, 0) == "attention52x4"
    for L in (49, 50, 51, 52):
        assert {ax.instantiation(L, 0, f) for f in (0, 4, 2)} == {"attention52x4", "attention52", "attention<4,0,0>"}
    assert ax.instantiation(52, 1, 0) == "attention<4,1,1>" and ax.instantiation(53, 0, 0) == "attention<4,0,1>"
    assert ax.instantiation(48, 0, 0) == "attention<4,0,1>" and ax.instantiation(65, 1, 2) == "attention<5,1,0>"


@pytest.mark.parametrize("name,build", [pytest.param(n, b, id=i) for i, n, b, _ in ax.exact_params() if "B129" not in i])
def test_float32_models_reproduce_the_exact_classes(name, build):
    """Building a case asserts its conditions; the float32 model of the kernel that runs its shape then gives the expected bytes."""
    c = build()
    got = ax.model(c["qkv"], c["B"], c["L"], c["heads"], c["causal"])
    ax.assert_same_bytes(got, c["expect"], c["what"])


def test_many_items_case_builds():
    B, L, heads = ax.MANY_ITEMS
    for name, build in ax.classes_of(B, L, heads, 0):
        c = build()
        assert c["expect"].shape == (B * L, heads * 64)


def test_exact_classes_catch_a_truncated_p():
    """The uniform class sees P cut to bf16 instead of rounded in the short kernels (1 / n is no bf16 for most n). The flash
    kernel's P is the unnormalised exponential, exactly 0 or 1 in every exact class: there only the random-data bound sees it."""
    for B, L, heads, causal in [(1, 50, 3, 0), (1, 77, 2, 1)]:
        c = ax.uniform_case(B, L, heads, causal)
        assert not torch.equal(ax.model(c["qkv"], B, L, heads, causal, truncate=True), c["expect"])


def test_ramp_rows_mix_directions_in_one_tile_and_fill_another():
    d = ax.ramp_directions(81)
    assert set(d[:16].tolist()) == {1, -1} and set(d[16:32].tolist()) == {-1} and set(d[32:48].tolist()) == {1}


RANDOM = [(B, L, h, c) for B, L, h, c in ax.SHORT_RANDOM] + [(B, L, h, 0) for B, L, h in ax.LONG_RANDOM]


@pytest.mark.parametrize("scale", ax.SCALES)
@pytest.mark.parametrize("B,L,heads,causal", RANDOM)
def test_bound_holds_for_the_float32_model_and_rejects_truncation(B, L, heads, causal, scale):
    """|model - o| <= 2^-8 (|o| + pav) (1 + 2^-6) for the faithful float32 model of the shape's kernel (largest ratio 0.94). The
    model that truncates P loses half a bf16 ulp of every weight on average: it crosses the bound wherever few weights carry a row
    (the x 4 scale: every case of 128 (query, head) rows or more; x 1.5: the short kernels' cases, 26 to 33 elements at ratio 1.19
    for the towers' shapes), and averages out below it where hundreds of weights share a row - there the uniform class catches it
    (test_exact_classes_catch_a_truncated_p)."""
    c = ax.random_case(B, L, heads, causal, scale)
    ratio, outside = ax.worst_ratio(ax.model(c["qkv"], B, L, heads, causal), c)
    t_ratio, t_outside = ax.worst_ratio(ax.model(c["qkv"], B, L, heads, causal, truncate=True), c)
    print(f"{c['what']}: model {ratio:.3f} ({outside} outside), truncating model {t_ratio:.3f} ({t_outside} outside)")
    assert outside == 0 and ratio <= 1.0
    assert t_outside > 0 or scale != "4" or B * L * heads < 128


def test_launcher_answers_without_a_launch(clipmi):
    """launch_attention's refusals come before any device call: they answer on a machine without a GPU."""
    L = clipmi._lib.lib()
    p = C.c_void_p(256)
    einval, eunsupported = 1, 4
    assert L.clipmi_dbg_attention(p, p, 1, 0, 2, 0, None) == einval and "L=0" in clipmi._lib.last_error()
    for Lq in (81, 578):
        assert L.clipmi_dbg_attention(p, p, 1, Lq, 2, 1, None) == eunsupported and "causal" in clipmi._lib.last_error()
    assert L.clipmi_dbg_attention(p, p, 0, 50, 2, 0, None) == 0
    assert L.clipmi_dbg_attention(None, p, 1, 50, 2, 0, None) == einval and L.clipmi_dbg_attention(p, None, 1, 50, 2, 0, None) == einval
    fused = C.c_int(7)
    assert L.clipmi_dbg_attention_fp8mx(p, p, p, p, 1, 0, 2, C.byref(fused), None) == einval and fused.value == 0
    assert L.clipmi_dbg_attention_fp8mx(p, p, p, p, 0, 50, 2, C.byref(fused), None) == 0 and fused.value == 0
    for args in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        assert L.clipmi_dbg_attention_fp8mx(*args, 1, 50, 2, C.byref(fused), None) == einval
    assert L.clipmi_dbg_attention_fp8mx(p, p, p, p, 1, 50, 2, None, None) == einval
