"""Host side of the cross-attention localisation loss (--attn_loss_weight): the closed-form gradient against autograd, the
coefficient reference, the flags and their refusals (all before any device use), the sweep drivers' switch and the C header."""
import json
import os
import sys

import pytest
import torch

import attn_loss_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from textboost_amd import _abi, cli, sweep  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
BASE = ["--pretrained_model_name_or_path", "m", "--instance_data_dir", "d"]


# ------------------------------------------------------------------------------------------------------------------ the math
@pytest.mark.parametrize("B,H,Sq,Skv,hd", [(2, 3, 20, 13, 8), (1, 1, 1, 1, 8), (2, 2, 9, 77, 16)])
def test_closed_form_gradient_equals_autograd_in_float64(B, H, Sq, Skv, hd):
    gen = torch.Generator().manual_seed(B * 100 + Sq)
    q = torch.randn(B * Sq, H * hd, generator=gen, dtype=torch.float64)
    k = torch.randn(B * Skv, H * hd, generator=gen, dtype=torch.float64)
    g = torch.randn(B, Sq, generator=gen, dtype=torch.float64)
    tok_w = (torch.rand(B, Skv, generator=gen) < 0.2).double()
    tok_w[0, 0] = 1.0
    scale, coef = hd ** -0.5, 0.37
    total, dq, dk = R.attn_loss_ref(q, k, tok_w, g, H, scale, coef)
    fq, fk = R.attn_loss_grad_formula(q, k, tok_w, g, H, scale, coef)
    assert (dq - fq).abs().max().item() <= 1e-15 and (dk - fk).abs().max().item() <= 1e-15
    if Skv == 1:        # one key: p = 1, tok_w - P_J = 0
        assert fq.abs().max().item() == 0.0 and fk.abs().max().item() == 0.0
    # a sample without a placeholder token: zero loss and zero gradient
    tok_w[B - 1] = 0
    total0, dq0, dk0 = R.attn_loss_ref(q, k, tok_w, g, H, scale, coef)
    assert dq0[(B - 1) * Sq:].abs().max().item() == 0.0 and dk0[(B - 1) * Skv:].abs().max().item() == 0.0
    # the loss lies in [-1, 1] per sample and layer for coefficients of coef_ref
    target = (torch.rand(B, 1, 8, 8, generator=gen) > 0.5).double()
    gg = R.coef_ref(target, 0)
    qq = torch.randn(B * 64, H * hd, generator=gen, dtype=torch.float64)
    per = R.attn_loss_terms(qq, k, torch.ones(B, Skv, dtype=torch.float64), gg, H, scale) / B
    assert -1.0 <= per.item() <= 1.0


def test_coef_ref_properties():
    gen = torch.Generator().manual_seed(1)
    target = torch.rand(3, 1, 16, 16, generator=gen)
    for level in (0, 1, 2):
        g = R.coef_ref(target, level)
        assert g.dtype == torch.float64 and tuple(g.shape) == (3, (16 >> level) ** 2)
        assert g.sum(dim=1).abs().max().item() < 1e-14              # fg, bg >= 1: the coefficients of a sample add up to zero
    for fill, want in ((1.0, -1.0 / 16), (0.0, 1.0 / 16)):            # all white / all black stay finite: max(., 1)
        g = R.coef_ref(torch.full((1, 1, 16, 16), fill), 2)
        assert torch.isfinite(g).all() and torch.equal(g, torch.full((1, 16), want, dtype=torch.float64))
    tiny = torch.zeros(1, 1, 16, 16)
    tiny[0, 0, 0, 0] = 0.5                                            # fg = 0.5 < 1: divided by 1, not by 0.5
    g = R.coef_ref(tiny, 0)
    assert abs(g[0, 0].item() - (0.5 / 255.5 - 0.5)) < 1e-15
    # pooling a 16 x 16 target to 4 x 4 is the direct 4 x 4 box mean
    t = torch.rand(1, 1, 16, 16, generator=gen, dtype=torch.float64)
    m = torch.stack([t[0, 0, 4 * i:4 * i + 4, 4 * j:4 * j + 4].mean() for i in range(4) for j in range(4)])
    fg, bg = m.sum(), (1 - m).sum()
    assert (R.coef_ref(t, 2)[0] - ((1 - m) / bg - m / fg)).abs().max().item() < 1e-15


# ------------------------------------------------------------------------------------------------------------------ the flags
def test_flags_parse_and_the_defaults_are_off():
    a = cli.parse_args(BASE)
    assert a.attn_loss_weight == 0.0 and a.attn_loss_levels == [2]
    cli.check_attn_loss_flags(a, (True, True, True, False))          # off: nothing to refuse, whatever the rest says
    a = cli.parse_args(BASE + ["--instance_mask_dir", "masks", "--mixed_precision", "fp16", "--attn_loss_weight", "0.01", "--attn_loss_levels", "1", "2"])
    assert a.attn_loss_weight == 0.01 and a.attn_loss_levels == [1, 2]
    cli.check_attn_loss_flags(a, (True, True, True, False))
    assert [n for n, _ in cli.ATTN_LOSS_FLAGS] == ["--attn_loss_weight", "--attn_loss_levels"]
    assert not {"--attn_loss_weight", "--attn_loss_levels"} & {n for n, _ in cli.FLAGS}
    with open(os.path.join(GOLDEN, "cli_flags.json")) as f:
        golden = json.load(f)
    golden = golden["flags"] if isinstance(golden, dict) else golden
    assert cli.flag_table() == sorted(golden, key=lambda s: s["flags"][0])     # the reference's flag table is unchanged


def test_every_refusal_is_raised_on_the_host():
    on = ["--instance_mask_dir", "masks", "--mixed_precision", "fp16", "--attn_loss_weight", "0.1"]
    levels = (True, True, True, False)
    with pytest.raises(ValueError, match="attn_loss_weight"):
        cli.parse_args(BASE + ["--attn_loss_weight", "-0.5"])
    with pytest.raises(ValueError, match="attn_loss_weight"):
        cli.parse_args(BASE + ["--attn_loss_weight", "nan"])
    for bad in (["3"], ["4"], ["2", "7"], ["-1"]):
        with pytest.raises(ValueError, match="attn_loss_levels"):
            cli.check_attn_loss_flags(cli.parse_args(BASE + on + ["--attn_loss_levels", *bad]), levels)
    with pytest.raises(ValueError, match="instance_mask_dir"):
        cli.check_attn_loss_flags(cli.parse_args(BASE + ["--mixed_precision", "fp16", "--attn_loss_weight", "0.1"]), levels)
    for fp32 in ([], ["--mixed_precision", "no"]):
        with pytest.raises(NotImplementedError, match="mixed_precision"):
            cli.check_attn_loss_flags(cli.parse_args(BASE + ["--instance_mask_dir", "masks", "--attn_loss_weight", "0.1"] + fp32), levels)


def test_setup_shared_refuses_before_it_touches_a_device(tmp_path, monkeypatch):
    """train_textboost.setup_shared runs the checks ahead of torch.cuda.set_device: with CUDA made unreachable every refusal still arrives as
    its own exception, not as the missing device"""
    from PIL import Image
    import train_textboost as T
    monkeypatch.setattr(torch.cuda, "is_available", lambda: (_ for _ in ()).throw(AssertionError("the device was asked for")))
    monkeypatch.setattr(torch.cuda, "set_device", lambda *a: (_ for _ in ()).throw(AssertionError("the device was asked for")))
    images, masks = tmp_path / "images", tmp_path / "masks"
    images.mkdir(), masks.mkdir()
    Image.new("RGB", (16, 16), 128).save(str(images / "a.png"))
    Image.new("L", (16, 16), 255).save(str(masks / "a.png"))
    base = ["--pretrained_model_name_or_path", str(tmp_path / "no_model"), "--instance_data_dir", str(images), "--resolution", "128"]
    on = ["--attn_loss_weight", "0.1", "--mixed_precision", "fp16"]
    with pytest.raises(ValueError, match="attn_loss_levels"):
        T.setup_shared(T.parse_args(base + on + ["--instance_mask_dir", str(masks), "--attn_loss_levels", "3"]))
    with pytest.raises(ValueError, match="instance_mask_dir"):
        T.setup_shared(T.parse_args(base + on))
    with pytest.raises(NotImplementedError, match="mixed_precision"):
        T.setup_shared(T.parse_args(base + ["--attn_loss_weight", "0.1", "--instance_mask_dir", str(masks)]))
    # a --concepts_list none of whose concepts has masks
    cl = tmp_path / "concepts.json"
    cl.write_text(json.dumps([{"instance_data_dir": str(images), "placeholder_token": "<a>"}]))
    with pytest.raises(ValueError, match="no concept has any"):
        T.setup_shared(T.parse_args(["--pretrained_model_name_or_path", str(tmp_path / "no_model"), "--concepts_list", str(cl), "--resolution",
                                     "128"] + on))
    # tensor inputs carry no masks: refused by the same check
    tens = tmp_path / "tensors"
    tens.mkdir()
    torch.save(torch.zeros(2, 4, 16, 16), str(tens / "latents.pt"))
    torch.save(torch.ones(2, 1, 16, 16), str(tens / "loss_weight.pt"))
    with pytest.raises(ValueError, match="instance_mask_dir"):
        T.setup_shared(T.parse_args(["--pretrained_model_name_or_path", str(tmp_path / "no_model"), "--instance_data_dir", str(tens),
                                     "--resolution", "128"] + on))
    # with everything in place the checks pass and the next thing asked for is the device
    with pytest.raises(AssertionError, match="the device was asked for"):
        T.setup_shared(T.parse_args(base + on + ["--instance_mask_dir", str(masks)]))


# ------------------------------------------------------------------------------------------------------------------ the sweep drivers
with open(os.path.join(GOLDEN, "sweep_commands.json")) as _f:
    SWEEP_CASES = {c["name"]: c for c in json.load(_f)["cases"]}
MODEL_TOKEN = "--pretrained_model_name_or_path="


def _jobs(case, extra):
    parser, builder = (sweep.db_parser(), sweep.build_db) if case["driver"] == "db" else (sweep.sdrp_parser(), sweep.build_sdrp)
    return builder(parser.parse_args(case["flags"] + ["--model-dir", "/m"] + extra))[1]


@pytest.mark.parametrize("name", sorted(SWEEP_CASES))
def test_sweep_commands_gain_the_flag_only_when_given(name):
    case = SWEEP_CASES[name]
    plain, masked = _jobs(case, []), _jobs(case, ["--mask-root", "/masks"])
    for (subject, cmd), (_, cmd_m), want in zip(plain, masked, case["subjects"]):
        assert [t for t in cmd if not t.startswith(MODEL_TOKEN)] == [t for t in want["cmd"] if not t.startswith(MODEL_TOKEN)]
        assert not any("attn_loss" in t for t in cmd + cmd_m)
    if case["driver"] != "db":   # the StyleDrop sweep trains in fp32: refused on the host, before any subject starts
        with pytest.raises(SystemExit, match="attn-loss-weight"):
            _jobs(case, ["--mask-root", "/masks", "--attn-loss-weight", "0.02"])
        return
    both = _jobs(case, ["--mask-root", "/masks", "--attn-loss-weight", "0.02"])
    assert len(plain) == len(both) == len(case["subjects"]) > 0
    for (subject, cmd), (_, cmd_m), (subject_b, cmd_b) in zip(plain, masked, both):
        assert any(t.startswith("--mixed_precision") for t in cmd_b)          # a 16-bit mode: the flag can work there
        assert subject == subject_b and cmd_b[:len(cmd_m)] == cmd_m and cmd_b[len(cmd_m):] == ["--attn_loss_weight=0.02"]


# ------------------------------------------------------------------------------------------------------------------ the header
def test_header_declares_the_entry_points_and_the_state_slot():
    structs, sigs, consts = _abi.load()
    assert {"tb_attn_loss_coef", "tb_attn_loss_bwd", "tb_attn_loss_final", "tb_attn_loss_workspace_bytes"} <= set(sigs)
    assert consts["TB_ST_LOSS_ATTN"] == 14 and consts["TB_ST_COUNT"] == 16
    from textboost_amd import _lib as L
    assert L.ST_LOSS_ATTN == consts["TB_ST_LOSS_ATTN"] and L.ST_COUNT == consts["TB_ST_COUNT"]
    assert len(sigs["tb_attn_loss_bwd"][0]) == 11 and len(sigs["tb_attn_loss_coef"][0]) == 7 and len(sigs["tb_attn_loss_final"][0]) == 6
