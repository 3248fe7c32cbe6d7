"""FreeU on the host: the closed form of the skip filter against diffusers' `torch.fft` form, the structure backbone
on a constant map, the bit identities of the float64 restatement, the oracle hooks' margin for tests/test_gpu_freeu.py, and the flags of
inference.py / eval_dreambooth.py with every refusal.  No device."""
import json
import os
import sys

import pytest
import torch

import freeu_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FILTER_SHAPES = sorted({(8, 8), (16, 16), (5, 7), (2, 2), (1, 1), (2, 3), (3, 3), (12, 24), (1, 4), (4, 1)} | {(s[1], s[2]) for s in R.SHAPES})
UNET_FACTORS = (1.5, 1.6, 0.9, 0.2)     # (b1, b2, s1, s2) of the tiny-UNet tests
PRED_BOUND = 3e-3                       # the rel-L2 bound of the tiny UNet's prediction (tests/test_gpu_model.py)
MARGIN = 10.0                           # FreeU must move the prediction by at least this many bounds


@pytest.mark.parametrize("hw", FILTER_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("offset", [0.0, 8.0])
def test_closed_form_is_the_fft_filter(hw, offset):
    g = torch.Generator().manual_seed(7)
    x = torch.randn(2, 3, *hw, generator=g, dtype=torch.float64) + offset
    for s in (0.2, 0.9, 1.0, 2.5):
        err = (R.fourier_filter_closed(x, s) - R.fourier_filter_fft(x, s)).abs().max().item()
        assert err <= 1e-12, (hw, s, err)


def test_a_two_by_two_map_is_scaled_whole_and_a_single_pixel_too():
    g = torch.Generator().manual_seed(1)
    for hw in ((2, 2), (1, 1), (1, 2), (2, 1)):
        x = torch.randn(1, 4, *hw, generator=g, dtype=torch.float64)
        assert (R.fourier_filter_closed(x, 0.25) - 0.25 * x).abs().max().item() <= 1e-15


def test_structure_backbone_on_a_constant_map_and_on_a_known_one():
    x = torch.full((2, 8, 3, 3), 0.75, dtype=torch.float64)
    x[:, 1::2] = -0.25                                        # channels differ, every pixel's mean is the same
    assert torch.equal(R.backbone(x, 1.6, "structure"), x)    # n = 0 where the published code divides by zero
    h = torch.zeros(1, 4, 1, 3, dtype=torch.float64)
    h[0, :, 0, 0], h[0, :, 0, 1], h[0, :, 0, 2] = 1.0, 2.0, 3.0      # means 1, 2, 3 -> n = 0, 0.5, 1
    out = R.backbone(h, 1.5, "structure")
    assert torch.equal(out[0, :2, 0], torch.tensor([[1.0, 2.5, 4.5]] * 2, dtype=torch.float64)) and torch.equal(out[0, 2:], h[0, 2:])
    assert torch.equal(R.backbone(h, 1.5, "scalar")[0, :2], 1.5 * h[0, :2])


@pytest.mark.parametrize("mode", R.MODES)
def test_identities_of_the_restatement(mode):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 24 + 40, 5, 7, generator=g, dtype=torch.float64)
    assert torch.equal(R.apply_freeu(x, 40, 1.0, 1.0, mode), x)
    y = R.apply_freeu(x, 40, 1.5, 1.0, mode)
    assert torch.equal(y[:, 24:], x[:, 24:]) and torch.equal(y[:, 12:24], x[:, 12:24]) and not torch.equal(y[:, :12], x[:, :12])
    y = R.apply_freeu(x, 40, 1.0, 0.2, mode)
    assert torch.equal(y[:, :24], x[:, :24]) and not torch.equal(y[:, 24:], x[:, 24:])
    rows = R.nchw_to_rows(x)
    assert torch.equal(R.rows_to_nchw(rows, 2, 5, 7), x)
    d = R.reference_rows(rows, 2, 5, 7, 24, 1.5, 0.2, mode) - R.nchw_to_rows(R.apply_freeu(x, 40, 1.5, 0.2, mode))
    assert d.abs().max().item() <= 1e-13          # (a strided view is summed in another order)


@pytest.mark.parametrize("sd2", [False, True], ids=["sd1", "sd2"])
def test_hooked_oracle_moves_the_tiny_prediction_by_a_clear_margin(sd2):
    from excite_ref import tiny_oracle, unet_inputs
    ref = tiny_oracle(sd2)
    x, t, ehs = unet_inputs(sd2=sd2)
    with torch.no_grad():
        plain = ref(x, t, ehs)
        hs = R.install_hooks(ref, 1.0, 1.0, 1.0, 1.0)
        assert len(hs) == 6 and torch.equal(ref(x, t, ehs), plain)
        for h in hs:
            h.remove()
        for mode in R.MODES:
            hs = R.install_hooks(ref, *UNET_FACTORS, mode=mode)
            moved = ref(x, t, ehs)
            for h in hs:
                h.remove()
            d = ((moved - plain).norm() / plain.norm()).item()
            print(f"[freeu] tiny oracle sd2={sd2} {mode}: FreeU moves the prediction by rel-L2 {d:.3e}")
            assert d >= MARGIN * PRED_BOUND
        assert torch.equal(ref(x, t, ehs), plain)


# ------------------------------------------------------------------------------------------------------------------ flags
def _model_dir(tmp_path, dim):
    d = tmp_path / f"m{dim}"
    (d / "unet").mkdir(parents=True)
    with open(d / "unet" / "config.json", "w") as f:
        json.dump({"cross_attention_dim": dim}, f)
    return str(d)


def _inference_freeu(argv):
    import inference
    from textboost_amd import freeu as F
    p = inference.build_parser()
    args = p.parse_args(["run"] + argv)
    F.check_count(p, args)
    return inference.check_freeu_flags(args)


def test_defaults_per_model_family_and_given_values(tmp_path):
    assert _inference_freeu(["--model", _model_dir(tmp_path, 768), "--freeu"]) == (1.5, 1.6, 0.9, 0.2, "scalar")
    assert _inference_freeu(["--model", _model_dir(tmp_path, 1024), "--freeu", "--freeu-backbone", "structure"]) == (1.4, 1.6, 0.9, 0.2, "structure")
    assert _inference_freeu(["--model", "/nowhere", "--freeu", "1.1", "1.2", "0.5", "0.25"]) == (1.1, 1.2, 0.5, 0.25, "scalar")
    assert _inference_freeu(["--model", "/nowhere"]) is None
    assert _inference_freeu(["--model", "/nowhere", "--freeu", "1", "1", "1", "1", "--region", "a=0,0,1,1", "--edit-prompt", "x", "--width", "1024"]) \
        == (1.0, 1.0, 1.0, 1.0, "scalar")       # forward-only companions are not this check's business


@pytest.mark.parametrize("argv, why", [
    (["--freeu", "1.5", "1.6", "0.9"], "expected zero or four values"),
    (["--freeu", "1.5"], "expected zero or four values"),
    (["--freeu", "1", "1", "1", "1", "1"], "expected zero or four values"),
    (["--freeu", "1.5", "x", "0.9", "0.2"], "invalid float value"),
    (["--freeu", "--freeu-backbone", "mean"], "invalid choice"),
    (["--freeu", "1.5", "1.6", "0", "0.2"], "S1 = 0.0: finite and > 0"),
    (["--freeu", "-1.5", "1.6", "0.9", "0.2"], "B1 = -1.5: finite and > 0"),
    (["--freeu", "1.5", "nan", "0.9", "0.2"], "B2 = nan: finite and > 0"),
    (["--freeu", "1.5", "1.6", "0.9", "inf"], "S2 = inf: finite and > 0"),
    (["--freeu-backbone", "structure"], "--freeu-backbone needs --freeu"),
    (["--freeu", "1", "1", "1", "1", "--excite", "dog"], "--freeu does not go with --excite"),
    (["--freeu", "--excite", "dog"], "--freeu does not go with --excite"),
    (["--freeu"], "no published factors for a UNet with cross_attention_dim 64"),
], ids=lambda v: "_".join(v).replace("--", "") if isinstance(v, list) else None)
def test_inference_refusals(argv, why, tmp_path, capsys):
    with pytest.raises(SystemExit) as e:
        _inference_freeu(["--model", _model_dir(tmp_path, 64)] + argv)
    said = str(e.value) if e.value.code not in (0, 2) else capsys.readouterr().err
    assert why in said, said


def test_defaults_need_a_readable_model_directory():
    with pytest.raises(SystemExit, match="default factors are chosen by the UNet's cross_attention_dim"):
        _inference_freeu(["--model", "/nowhere", "--freeu"])


def test_eval_dreambooth_flags(tmp_path):
    import eval_dreambooth as E
    p = E.build_parser()
    m = _model_dir(tmp_path, 768)
    assert E.check_freeu_args(p, p.parse_args(["run", "--model", m, "--freeu"])) == (1.5, 1.6, 0.9, 0.2, "scalar")
    assert E.check_freeu_args(p, p.parse_args(["run", "--model", m, "--freeu", "1.2", "1.3", "0.8", "0.4", "--freeu-backbone", "structure"])) \
        == (1.2, 1.3, 0.8, 0.4, "structure")
    assert E.check_freeu_args(p, p.parse_args(["run", "--skip-gen"])) is None
    for argv, why in ((["--skip-gen", "--freeu"], "--freeu shapes the images"),
                      (["--skip-gen", "--freeu-backbone", "scalar"], "--freeu-backbone shapes the images"),
                      (["--model", m, "--freeu-backbone", "scalar"], "--freeu-backbone needs --freeu"),
                      (["--model", m, "--freeu", "1", "0", "1", "1"], "B2 = 0.0: finite and > 0")):
        with pytest.raises(SystemExit, match=why):
            E.check_freeu_args(p, p.parse_args(["run"] + argv))
    with pytest.raises(SystemExit):
        E.check_freeu_args(p, p.parse_args(["run", "--model", m, "--freeu", "1", "1"]))
    with pytest.raises(SystemExit, match="--freeu shapes the images"):      # main refuses before anything else is looked at
        E.main(["run", "--skip-gen", "--freeu"])
