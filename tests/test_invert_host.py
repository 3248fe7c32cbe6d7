"""Editing a photo by its prompt (inference.py --invert-image), host side: the inversion scalars as the algebraic inverse of the
solver's first-order step, first-order convergence of the inversion on a model with a closed-form flow (tests/invert_ref.py), the layers'
declarations, and every CLI refusal."""
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

import invert_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the layers exist and agree
def test_header_bindings_wrappers_and_source_exist():
    from tests.test_edit_host import _header_args
    from textboost_amd import _lib as L
    from textboost_amd import ops
    src = open(os.path.join(ROOT, "textboost_amd", "csrc", "invert.hip")).read()
    for name, n_args in (("tb_invert_step", 10), ("tb_dpm_step_pin", 17)):
        assert len(_header_args(name)) == n_args, name
        assert name in L._SIGS and len(L._SIGS[name][0]) == n_args, name
        assert f'extern "C" int {name}(' in src
    # the step's own arguments come first and in tb_dpm_step's order, so both are called alike
    assert L._SIGS["tb_dpm_step_pin"][0][:12] == L._SIGS["tb_dpm_step"][0][:12]
    assert list(inspect.signature(ops.dpm_step_pin).parameters)[:12] == list(inspect.signature(ops.dpm_step).parameters)
    assert list(inspect.signature(ops.invert_step).parameters) == ["x", "eps2", "x2", "traj_out", "n_per_b", "B", "guidance", "cx", "ce"]


# ------------------------------------------------------------------------------------------------ inversion_scalars
def _sch(steps, spacing="leading", offset=1, pred="epsilon"):
    from textboost_amd.sampler import DPMSolverPP2M
    sch = DPMSolverPP2M(timestep_spacing=spacing, steps_offset=offset, prediction_type=pred)
    sch.set_timesteps(steps)
    return sch


@pytest.mark.parametrize("spacing", ["leading", "linspace", "trailing"])
@pytest.mark.parametrize("steps", [1, 2, 3, 25, 50])
def test_inversion_step_is_the_algebraic_inverse_of_the_first_order_step(steps, spacing):
    sch = _sch(steps, spacing)
    assert sch.noise_scalars(steps) == (1.0, 0.0)
    g = torch.Generator().manual_seed(steps)
    worst = 0.0
    for k in range(steps - 1, -1, -1):
        x, eps = torch.randn(64, generator=g, dtype=torch.float64), torch.randn(64, generator=g, dtype=torch.float64)
        cx, ce = sch.inversion_scalars(k)
        a_k, s_k = sch.noise_scalars(k)
        a_n, s_n = sch.noise_scalars(k + 1)
        assert cx == a_k / a_n and ce == s_k - a_k * s_n / a_n
        xk = cx * x + ce * eps
        back = R.first_order_step(sch, k, xk, eps)
        worst = max(worst, ((back - x).abs().max() / x.abs().max()).item())
    print(f"[invert] {steps} steps, {spacing}: inversion then the first-order step, worst relative difference {worst:.2e}")
    assert worst <= 1e-12
    for k in (-1, steps):
        with pytest.raises(IndexError):
            sch.inversion_scalars(k)


def test_inversion_converges_at_first_order_on_a_gaussian_model():
    """data ~ N(0, 0.9^2): eps and the probability-flow ODE are closed form (tests/invert_ref.py).  Default SD betas, leading spacing, offset 1,
    x0 = (0.7, -1.3).  Measured in float64: 25 steps 5.2e-2, 50 2.9e-2, 100 1.5e-2, 200 7.5e-3."""
    from textboost_amd.sampler import DPMSolverPP2M
    err = {n: R.gaussian_inversion_error(DPMSolverPP2M, n) for n in (25, 50, 100, 200)}
    print("[invert] relative error of traj[0] against the exact flow: " + ", ".join(f"{n} steps {e:.3e}" for n, e in err.items()))
    for n in (25, 50, 100):
        assert err[2 * n] <= 0.6 * err[n], (n, err)
    assert err[50] <= 3.5e-2


def test_v_prediction_and_the_ancestral_scheduler_have_no_inversion():
    from textboost_amd.sampler import DDPMAncestral
    with pytest.raises(NotImplementedError, match="one level off the timestep the model is asked about"):
        _sch(4, pred="v_prediction").inversion_scalars(0)
    assert not hasattr(DDPMAncestral, "inversion_scalars")
    assert _sch(7).noise_scalars(7) == (1.0, 0.0)


# ------------------------------------------------------------------------------------------------ the CLI's refusals
def test_parser_accepts_the_invert_flags():
    import inference
    p = inference.build_parser()
    a = p.parse_args(["run"])
    assert a.invert_image is None and a.invert_guidance is None
    a = p.parse_args(["run", "--invert-image", "photo.jpg", "--invert-guidance", "2.5", "--mask", "m.png", "--no-paste"])
    assert (a.invert_image, a.invert_guidance, a.mask, a.no_paste) == ("photo.jpg", 2.5, "m.png", True)


def test_invert_refusals_come_before_the_device_is_consulted(tmp_path, monkeypatch):
    pytest.importorskip("transformers")
    from PIL import Image
    from safetensors.torch import save_file
    import inference
    from tests.test_compose_host import write_run
    from tests.test_gpu_generate import _write_tokenizer
    mdir, rdir = str(tmp_path / "model"), str(tmp_path / "runs" / "dog")
    _write_tokenizer(os.path.join(mdir, "tokenizer"))
    for sub in ("unet", "vae", "scheduler"):
        os.makedirs(os.path.join(mdir, sub))
    with open(os.path.join(mdir, "unet", "config.json"), "w") as f:
        json.dump({"sample_size": 16}, f)
    sched = os.path.join(mdir, "scheduler", "scheduler_config.json")

    def write_sched(pred):
        with open(sched, "w") as f:
            json.dump({"prediction_type": pred, "steps_offset": 1}, f)
    write_sched("epsilon")
    write_run(rdir, ["<dog>"], ["<hflip>"], seed=1, rank=4, keep_rows="even")
    vae_file = os.path.join(mdir, "vae", "diffusion_pytorch_model.safetensors")
    whole = {"decoder.conv_in.bias": torch.zeros(4), "post_quant_conv.bias": torch.zeros(4), "encoder.conv_in.bias": torch.zeros(4),
             "quant_conv.bias": torch.zeros(8)}
    save_file(whole, vae_file)
    photo, mask, small, junk = (str(tmp_path / n) for n in ("photo.png", "mask.png", "small.png", "junk.png"))
    Image.fromarray(np.full((96, 160, 3), 90, dtype=np.uint8)).save(photo)
    Image.fromarray(np.zeros((96, 160), dtype=np.uint8)).save(mask)
    Image.fromarray(np.zeros((96, 128), dtype=np.uint8)).save(small)
    with open(junk, "wb") as f:
        f.write(b"not a picture")

    def consulted():
        raise AssertionError("torch.cuda was consulted")
    monkeypatch.setattr(torch.cuda, "is_available", consulted)
    common = [rdir, "--model", mdir, "--prompt", "a dog on a beach", "--steps", "8"]
    E = ["--edit-prompt", "a fluffy <dog> dog on a beach"]
    inv = ["--invert-image", photo]
    today = "would need the photo inverted to noise first, which is not built"
    refusals = [
        (inv, "--invert-image needs --edit-prompt TEXT or --reweight WORD=F"),
        (["--invert-guidance", "2"], "--invert-guidance needs --invert-image"),
        (E + ["--invert-guidance", "2"], "--invert-guidance needs --invert-image"),
        (E + inv + ["--init-image", photo], "--invert-image does not go with --init-image"),
        (E + inv + ["--strength", "0.5"], "--invert-image does not go with --strength"),
        (E + inv + ["--region", "dog=0,0,0.5,1"], "--invert-image does not go with --region"),
        (E + inv + ["--attn-map"], "--invert-image does not go with --attn-map"),
        (E + inv + ["--attn-map", "dog"], "--invert-image does not go with --attn-map"),
        (E + inv + ["--mask", "auto:dog"], "--invert-image does not go with --mask auto:dog"),
        (E + inv + ["--dilate", "2"], "--invert-image does not go with --dilate"),
        (E + inv + ["--invert-guidance", "-0.5"], "--invert-guidance -0.5: a finite number >= 0"),
        (E + inv + ["--invert-guidance", "nan"], "--invert-guidance nan: a finite number >= 0"),
        (E + inv + ["--invert-guidance", "inf"], "--invert-guidance inf: a finite number >= 0"),
        (E + ["--invert-image", str(tmp_path / "absent.png")], "--invert-image " + str(tmp_path / "absent.png") + ": cannot be read"),
        (E + ["--invert-image", junk], "cannot be read as a picture"),
        (E + inv + ["--mask", junk], "--mask " + junk + ": cannot be read"),
        (E + inv + ["--mask", small], "is 128 x 96, --invert-image " + photo + " is 160 x 96"),
        # what was refused before keeps its text
        (E + ["--init-image", photo], "--edit-prompt does not go with --init-image: editing a photo by its prompt " + today),
        (["--reweight", "dog=2", "--init-image", photo], "--reweight does not go with --init-image: editing a photo by its prompt " + today),
        (["--mask", mask], "--mask needs --init-image FILE (the photo to edit)"),
        (E + ["--mask", mask], "--mask needs --init-image FILE (the photo to edit)"),
    ]
    for extra, msg in refusals:
        with pytest.raises(SystemExit, match=re.escape(msg)) as ei:
            inference.main(common + extra)
        assert ei.value.code not in (0, None), extra
    # a v-prediction model, from scheduler/scheduler_config.json
    write_sched("v_prediction")
    with pytest.raises(SystemExit, match=re.escape("says prediction_type 'v_prediction'; inversion is built for epsilon models only")):
        inference.main(common + E + inv)
    write_sched("epsilon")
    # a VAE file without the encoder half
    save_file({k: v for k, v in whole.items() if k.startswith(("decoder.", "post_quant_conv."))}, vae_file)
    with pytest.raises(SystemExit, match=r"--invert-image: .*holds no encoder\.\* / quant_conv\.\* tensors"):
        inference.main(common + E + inv)
    save_file(whole, vae_file)
    # accepted arguments pass every host check and reach the device question
    for extra in (E + inv, E + inv + ["--invert-guidance", "0"], E + inv + ["--mask", mask], E + inv + ["--mask", mask, "--no-paste"],
                  inv + ["--reweight", "dog=0.5", "--invert-guidance", "3", "--cross-steps", "0.5", "--self-steps", "0"]):
        with pytest.raises(AssertionError, match="consulted"):
            inference.main(common + extra)
    args = inference.build_parser().parse_args(common + E + inv + ["--mask", mask])
    got = inference.check_invert_args(args)
    assert got["guidance"] == 1.0 and got["rgb"].shape == (96, 160, 3) and got["mask"].size == (160, 96)
    assert inference.check_invert_args(inference.build_parser().parse_args(common + E)) is None
