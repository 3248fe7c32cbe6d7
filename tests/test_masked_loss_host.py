"""Host side of the masked training loss (--instance_mask_dir): the float64 / numpy references the GPU tests compare
against, the new flags and their validation, the mask files' checks, and that the reference's flag table and sweep commands are untouched.
No GPU."""
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import masked_loss_ref as R  # noqa: E402
from textboost_amd import cli, sweep  # noqa: E402
from textboost_amd import data as tbdata  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
BASE = ["--pretrained_model_name_or_path", "m"]


# ------------------------------------------------------------------------------------------------------------------ the references
def _case(seed=0, B=3, C=4, h=5, w=7):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, C, h, w, generator=g, dtype=torch.float64), torch.randn(B, C, h, w, generator=g, dtype=torch.float64),
            torch.rand(B, 1, h, w, generator=g, dtype=torch.float64))


def test_all_ones_weights_give_the_plain_mse():
    pred, target, _ = _case()
    ones = torch.ones(3, 1, 5, 7, dtype=torch.float64)
    torch.testing.assert_close(R.weighted_mse(pred, target, ones), F.mse_loss(pred, target), rtol=1e-14, atol=0)


def test_autograd_gradient_equals_the_closed_form():
    pred, target, weight = _case(1)
    weight[1] *= 0.01          # W_1 = 0.35 * 0.01-ish < 1: the max(W_b, 1) branch
    assert weight[1].sum() < 1 < weight[0].sum()
    p = pred.clone().requires_grad_(True)
    (R.weighted_mse(p, target, weight) * 8.0).backward()
    torch.testing.assert_close(p.grad, R.weighted_mse_grad(pred, target, weight, 8.0), rtol=1e-13, atol=1e-16)


def test_an_all_zero_sample_is_finite_and_has_no_gradient():
    pred, target, weight = _case(2)
    weight[2] = 0
    p = pred.clone().requires_grad_(True)
    loss = R.weighted_mse(p, target, weight)
    loss.backward()
    assert torch.isfinite(loss) and torch.isfinite(p.grad).all()
    assert p.grad[2].abs().max().item() == 0.0 and p.grad[0].abs().max().item() > 0.0


def test_pool_ref_arithmetic():
    m = np.random.default_rng(0).integers(0, 256, (24, 40), dtype=np.uint8)
    out = R.pool_ref(m, 8, 3, 2, 3, 8, 0.0)
    assert out.dtype == np.float32 and out.shape == (2, 3)
    want = m[3:19, 8:32].astype(np.float64).reshape(2, 8, 3, 8).mean(axis=(1, 3)) / 255.0
    np.testing.assert_allclose(out, want, rtol=2e-7)
    white = np.full((16, 16), 255, np.uint8)
    assert np.array_equal(R.pool_ref(white, 0, 0, 2, 2, 8, 0.25), np.ones((2, 2), np.float32))
    assert np.array_equal(R.pool_ref(np.zeros((16, 16), np.uint8), 0, 0, 2, 2, 8, 0.25), np.full((2, 2), 0.25, np.float32))
    with pytest.raises(AssertionError):
        R.pool_ref(m, 30, 0, 2, 2, 8, 0.0)


# ------------------------------------------------------------------------------------------------------------------ the flags
def test_new_flags_parse_and_defaults():
    a = cli.parse_args(BASE)
    assert a.instance_mask_dir is None and a.mask_floor == 0.0
    a = cli.parse_args(BASE + ["--instance_mask_dir", "masks", "--mask_floor", "0.25"])
    assert a.instance_mask_dir == "masks" and a.mask_floor == 0.25
    help_text = cli.build_parser().format_help()
    assert "threshold" in help_text and "--mask_floor" in help_text


def test_mask_floor_without_a_mask_dir_raises():
    with pytest.raises(ValueError, match="instance_mask_dir"):
        cli.parse_args(BASE + ["--mask_floor", "0.1"])


@pytest.mark.parametrize("value", ["1.0", "-0.1", "1.5", "nan"])
def test_mask_floor_out_of_range_raises(value):
    with pytest.raises(ValueError, match="mask_floor"):
        cli.parse_args(BASE + ["--instance_mask_dir", "masks", "--mask_floor", value])


def test_new_flags_are_extensions_and_the_reference_flag_table_is_unchanged():
    with open(os.path.join(GOLDEN, "cli_flags.json")) as f:
        golden = json.load(f)
    golden = golden["flags"] if isinstance(golden, dict) else golden
    assert cli.flag_table() == sorted(golden, key=lambda s: s["flags"][0])
    assert [n for n, _ in cli.MASKED_LOSS_FLAGS] == ["--instance_mask_dir", "--mask_floor"]     # extension flags, in a list of their own
    assert not {"--instance_mask_dir", "--mask_floor"} & {n for n, _ in cli.FLAGS}


# ------------------------------------------------------------------------------------------------------------------ the mask files
def _png(path, w, h, mode="RGB"):
    from PIL import Image
    Image.new(mode, (w, h), 128).save(str(path))


def test_masks_are_matched_by_stem_and_checked_for_size(tmp_path):
    images, masks = tmp_path / "images", tmp_path / "masks"
    images.mkdir(), masks.mkdir()
    _png(images / "a.png", 6, 4)
    _png(images / "b.png", 5, 7)
    paths = tbdata.instance_image_paths(str(images))
    assert [os.path.basename(p) for p in paths] == ["a.png", "b.png"]
    # both missing: both named
    with pytest.raises(ValueError) as e:
        tbdata.instance_mask_paths(paths, str(masks))
    assert "a.png" in str(e.value) and "b.png" in str(e.value)
    # one present with another extension, one missing
    _png(masks / "a.bmp", 6, 4, "L")
    with pytest.raises(ValueError) as e:
        tbdata.instance_mask_paths(paths, str(masks))
    assert "b.png" in str(e.value) and "a.png" not in str(e.value)
    # a size mismatch names the mask and the image
    _png(masks / "b.png", 7, 5, "L")
    with pytest.raises(ValueError) as e:
        tbdata.instance_mask_paths(paths, str(masks))
    assert str(masks / "b.png") in str(e.value) and str(images / "b.png") in str(e.value) and "7 x 5" in str(e.value)
    _png(masks / "b.png", 5, 7, "L")
    assert tbdata.instance_mask_paths(paths, str(masks)) == [str(masks / "a.bmp"), str(masks / "b.png")]
    assert tbdata.decode_mask(str(masks / "b.png")).shape == (7, 5) and tbdata.decode_mask(str(masks / "b.png")).dtype == np.uint8


def test_concept_masks_per_concept_and_floor_without_masks(tmp_path):
    images, masks, other = tmp_path / "images", tmp_path / "masks", tmp_path / "other"
    images.mkdir(), masks.mkdir(), other.mkdir()
    _png(images / "a.png", 6, 4)
    _png(masks / "a.png", 6, 4, "L")
    _png(other / "c.png", 3, 3)
    concepts = [{"instance_data_dir": str(images), "instance_mask_dir": str(masks)}, {"instance_data_dir": str(other)}]
    assert tbdata.concept_masks(concepts, 0.5) == [[str(masks / "a.png")], None]     # the second concept trains unmasked
    assert tbdata.concept_masks(concepts[1:], 0.0) is None
    with pytest.raises(ValueError, match="mask_floor"):
        tbdata.concept_masks(concepts[1:], 0.5)
    with pytest.raises(ValueError, match="no such directory"):
        tbdata.concept_masks([{"instance_data_dir": str(images), "instance_mask_dir": str(tmp_path / "nowhere")}])


# ------------------------------------------------------------------------------------------------------------------ the sweep drivers
with open(os.path.join(GOLDEN, "sweep_commands.json")) as _f:
    SWEEP_CASES = {c["name"]: c for c in json.load(_f)["cases"]}
MODEL_TOKEN = "--pretrained_model_name_or_path="


def _jobs(case, extra):
    parser, builder = (sweep.db_parser(), sweep.build_db) if case["driver"] == "db" else (sweep.sdrp_parser(), sweep.build_sdrp)
    return builder(parser.parse_args(case["flags"] + ["--model-dir", "/m"] + extra))[1]


@pytest.mark.parametrize("name", sorted(SWEEP_CASES))
def test_sweep_commands_gain_exactly_one_argument_with_mask_root(name):
    case = SWEEP_CASES[name]
    plain, masked = _jobs(case, []), _jobs(case, ["--mask-root", "/masks"])
    assert len(plain) == len(masked) == len(case["subjects"]) > 0
    for (subject, cmd), (subject_m, cmd_m), want in zip(plain, masked, case["subjects"]):
        # without --mask-root: the golden's argv, but for the model token
        assert [t for t in cmd if not t.startswith(MODEL_TOKEN)] == [t for t in want["cmd"] if not t.startswith(MODEL_TOKEN)]
        assert subject == subject_m and cmd_m[:len(cmd)] == cmd and cmd_m[len(cmd):] == [f"--instance_mask_dir=/masks/{subject}"]
