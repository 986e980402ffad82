"""CPU, oracle only: tests/test_wiring_gpu.py has the power it claims. For every form, every case of tests/wiring_cases.py
and every wrong dict of faults(case) - the loud tensor stale, taken from or given to another layer, exchanged with its
sibling, its Q / K / V thirds rotated - the oracle on the wrong dict must differ from the oracle on the loud dict

  bf16 forms: by at least BF16_MARGIN (8) x the tolerance the GPU test applies to that case, 3 x the oracle's bf16-emulation
              noise on the loud dict + 1e-3. A tower with that fault then misses the GPU test by at least 7 tolerances.
  FP8 forms:  in the product's emulation (clip_oracle.linear_fp8(act="product") under act_round(bfloat16)), by at least
              FP8_MARGIN (3) x the distance between the row-scale and the product emulation of the loud dict: the yardstick
              tests/test_fp8_gpu.py holds the device to. A device within one yardstick of the right emulation is then at
              least two from every wrong one, which is what the GPU test's nearest-candidate rule needs.

Each test prints its form's weakest fault. With wiring_cases.LOUDNESS and LOUD_SEED as committed, the weakest faults were, in
tolerances: plain-vision 11.6, plain-text 10.2, fold-vision-leaves 12.6, -partials 10.9, -wide-tail 11.0, fold-text-leaves 9.5,
-partials 9.4; in yardsticks: fp8-vision 3.7, fp8-vision-persistent 3.9. The weakest fault of a few hundred is an extreme
value and moves with the seed (7.1 .. 13.8 tolerances over six seeds): a seed or a loudness that misses a margin is replaced,
the margin stays."""
import pytest
import torch

import wiring_cases as wc


def _weakest(rows):
    ratio, what = min(rows)
    return f"weakest fault {what}: {ratio:.2f}"


@pytest.mark.parametrize("form", wc.BF16_FORMS)
def test_every_fault_moves_the_oracle_by_eight_tolerances(form):
    rows, noises = [], []
    for case in wc.cases(form):
        ref, noise, tol = wc.bf16_rule(form, wc.loud_sd(form, case))
        assert torch.isfinite(ref).all()
        noises.append(noise)
        for name, sd in wc.faults(form, case):
            rows.append((wc.dist(wc.oracle(form, sd), ref) / tol, f"{wc.case_id(form, case)}/{name}"))
    print(f"{form}: {len(wc.cases(form))} cases, {len(rows)} faults, bf16-emulation noise on the loud dicts "
          f"{min(noises):.4g} .. {max(noises):.4g}, {_weakest(rows)} tolerances")
    missed = sorted(r for r in rows if r[0] < wc.BF16_MARGIN)
    assert not missed, f"{form}: {len(missed)} faults move the oracle by less than {wc.BF16_MARGIN} tolerances: {missed[:10]}"


@pytest.mark.parametrize("form", wc.FP8_FORMS)
def test_every_fault_separates_the_fp8_emulations_by_three_yardsticks(form):
    rows, yards = [], []
    for case in wc.cases(form):
        ld = wc.loud_sd(form, case)
        emu = wc.emulate_fp8(form, ld, "product")
        yard = wc.dist(wc.emulate_fp8(form, ld, "row"), emu)
        assert torch.isfinite(emu).all() and yard > 0
        yards.append(yard)
        for name, sd in wc.faults(form, case):
            rows.append((wc.dist(wc.emulate_fp8(form, sd, "product"), emu) / yard, f"{wc.case_id(form, case)}/{name}"))
    print(f"{form}: {len(wc.cases(form))} cases, {len(rows)} faults, row-scale to product emulation "
          f"{min(yards):.4g} .. {max(yards):.4g}, {_weakest(rows)} yardsticks")
    missed = sorted(r for r in rows if r[0] < wc.FP8_MARGIN)
    assert not missed, f"{form}: {len(missed)} faults separate the emulations by less than {wc.FP8_MARGIN} yardsticks: {missed[:10]}"


@pytest.mark.parametrize("form", ["plain-vision", "plain-text", "fold-vision-partials", "fold-text-leaves"])
def test_the_k_third_of_in_proj_bias_does_not_reach_the_oracle(form):
    """Why it is no case: a constant added to every key moves every score of a query by the same amount, which softmax
    drops. Made loud, it moves the oracle by less than a tenth of the tolerance (f32 rounding is all that is left)."""
    for l in range(wc.n_layers(form)):
        case = wc.Case(wc._layer_key(form, l, "attn.in_proj_bias"), 1)
        assert case not in wc.cases(form)
        ref, _, tol = wc.bf16_rule(form, wc.base_sd(form))
        moved = wc.dist(wc.oracle(form, wc.loud_sd(form, case)), ref)
        print(f"{form} layer {l}: loud K bias moves the oracle by {moved:.3g} = {moved / tol:.4f} tolerances")
        assert moved < 0.1 * tol


def test_the_case_list_covers_every_tensor_of_every_layer():
    for form in wc.FORMS:
        f, sd = wc.FORMS[form], wc.base_sd(form)
        own = [k for k in sd if k.startswith("visual.") == (f["tower"] == "vision") and k != "logit_scale"]
        assert sorted({c.key for c in wc.cases(form)}) == sorted(own), form
        ids = [wc.case_id(form, c) for c in wc.cases(form)]
        assert len(set(ids)) == len(ids)
        # a loud dict differs from the base dict in its case's tensor (or third) only, and there everywhere
        case = wc.cases(form)[-8]
        ld = wc.loud_sd(form, case)
        assert [k for k in sd if not torch.equal(sd[k], ld[k])] == [case.key]
        for name, bad in wc.faults(form, case):
            assert any(not torch.equal(bad[k], ld[k]) for k in sd), (form, name)


def test_the_forms_have_the_shapes_they_are_named_for():
    """toy-256: 101 tokens; the text toys: 16 positions with an EOT at the last one, so the host trims nothing"""
    import clipmi
    for form, f in wc.FORMS.items():
        a = clipmi.weights.ARCHS[f["arch"]]
        x = wc.full_inputs(form)
        if f["tower"] == "vision":
            assert x.shape[0] == f["n"] and torch.equal(x[list(f["rows"])], wc.compared_inputs(form))
            tokens, width = (a["res"] // a["patch"]) ** 2 + 1, a["v_width"]
        else:
            assert int(x.argmax(dim=1).max()) == a["ctx"] - 1
            tokens, width = a["ctx"], a["t_width"]
        assert (width % 256 == 0) == bool(f["fold"] or f["fp8"]), form
        if "leaves" in f:
            assert (x.shape[0] * tokens <= 128) == f["leaves"], form
        if "tail_leaves" in f:
            assert (x.shape[0] <= 128) == f["tail_leaves"], form
