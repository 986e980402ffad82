"""CPU checks of the constants and data behind tests/test_rows_exact_gpu.py (tests/row_exact.py): the bound constants of the two
LayerNorm data classes follow from a float32 restatement of the kernel's own order of operations, never from a kernel's output.

Measured worst |restated - float64| in units of 2^-23 (A rstd |gamma| + |beta|):
  exact class  (sum, mean, deviations and variance exact; eps, 1 / sqrt and the multiply-add round): 0.636 -> C_EXACT = 3
  random class (the sums round too)                                                                : 2.623 -> C_RANDOM = 11"""
import torch

import row_exact as rx


def test_ln_bound_constants():
    """C = four times the worst restated ratio of the class, rounded up. Measured: exact class 0.636 (4 x = 2.54), random class
    2.623 (4 x = 10.49)."""
    for cls, C in (("exact", rx.C_EXACT), ("random", rx.C_RANDOM)):
        worst = rx.ln_class_ratio(cls)
        print(f"restated layernorm_kernel, {cls} class: worst ratio {worst}")
        assert 4 * worst <= C <= 8 * worst, (cls, worst, C)


def test_exact_class_is_exact_in_f32():
    """Sum, mean, deviations and variance of every exact-class row come out of the float32 restatement without rounding
    (ln_restated asserts it), the constant row's reference is beta, and rows carry the per-row offset."""
    for cls, widths in (("exact", rx.LN_W), ("beta0", rx.LN_W_256)):
        for M in rx.LN_M:
            for W in widths:
                c = rx.ln_case(cls, M, W)
                rx.ln_restated(c["x"], c["gamma"], c["beta"], exact=True)
                if M >= 3:
                    assert torch.equal(c["ref"][1], c["beta"].double()) and (c["x"][1] == c["x"][1, 0]).all()
                    assert c["x"][2].double().mean().item() == 10000.0
                assert c["x"][0].double().mean().item() == -12.0
                if M >= 5:
                    assert c["x"][4].double().mean().item() == 4.0


def test_quantiser_restatements_on_known_values():
    """The torch restatements that serve as references, on values worked out by hand."""
    t = torch.tensor([[448.0, -224.0, 0.0, 1.0] + [0.0] * 28, [0.0] * 32]).to(torch.bfloat16)
    q, s = rx.quant_rows(t)
    assert s.tolist() == [1.0, 1.0] and q[0, :4].tolist() == [0x7e, 0xf6, 0x00, 0x38] and not q[1].any()
    q, sb = rx.quant_mx(t)
    # block max 448 = 1.75 x 2^8: scale 2^(8 - 7), byte 128; 448 / 2 = 224 = 1.75 x 2^7 -> 0x76; a block of zeros: byte 127
    assert sb[:, 0].tolist() == [128, 127] and q[0, :4].tolist() == [0x76, 0xee, 0x00, 0x30] and not q[1].any()
    x3 = torch.tensor([[0x80, 0x3f, 0x80, 0x3f, 128, 129]], dtype=torch.uint8)          # two bf16 1.0, remainders 0 and +1
    assert rx.join(x3, 2).view(torch.int32).tolist() == [[0x3f800000, 0x3f800100]]
