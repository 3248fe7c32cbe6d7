"""Image editing (inference.py --init-image / --mask; textboost_amd/edit.py), host side: the C-ABI declarations and bindings, the
strength -> first step table, the scheduler started mid-schedule against tests/edit_ref.py, the mask preparation, and the CLI's refusals."""
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BEGIN_TABLE = [(8, 0.5, 4), (8, 1.0, 0), (8, 0.3, 6), (8, 0.125, 7), (25, 0.6, 10), (50, 0.75, 13)]
NO_STEP = [(8, 0.124), (8, 0.1)]


# ------------------------------------------------------------------------------------------------ the layers exist and agree
def _header_args(name):
    hdr = open(os.path.join(ROOT, "include", "textboost_hip.h")).read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
    assert m, f"{name} is not declared in include/textboost_hip.h"
    return [a for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",") if a.strip()]


def test_header_bindings_wrappers_and_source_exist():
    from textboost_amd import _lib as L
    from textboost_amd import ops
    assert os.path.exists(os.path.join(ROOT, "textboost_amd", "csrc", "edit.hip"))
    for name, n_args in (("tb_dpm_step_blend", 19), ("tb_img_paste", 11)):
        args = _header_args(name)
        assert len(args) == n_args, (name, args)
        assert name in L._SIGS and len(L._SIGS[name][0]) == n_args, name
    # the step's own arguments come first and in tb_dpm_step's order, so both are called alike
    assert L._SIGS["tb_dpm_step_blend"][0][:12] == L._SIGS["tb_dpm_step"][0][:12]
    src = open(os.path.join(ROOT, "textboost_amd", "csrc", "edit.hip")).read()
    assert 'extern "C" int tb_dpm_step_blend(' in src and 'extern "C" int tb_img_paste(' in src
    assert callable(ops.dpm_step_blend) and callable(ops.img_paste)
    assert list(inspect.signature(ops.dpm_step_blend).parameters)[:12] == list(inspect.signature(ops.dpm_step).parameters)


# ------------------------------------------------------------------------------------------------ strength
def test_strength_begin_reproduces_the_table():
    from tests.edit_ref import ref_begin
    from textboost_amd.edit import strength_begin
    for steps, s, begin in BEGIN_TABLE:
        assert strength_begin(steps, s) == begin == ref_begin(steps, s), (steps, s)
    for steps, s in NO_STEP:
        assert ref_begin(steps, s) is None
        with pytest.raises(ValueError, match="none of the"):
            strength_begin(steps, s)
    for s in (0.0, -0.5, 1.0000001, 2.0, float("nan")):
        with pytest.raises(ValueError, match="outside"):
            strength_begin(8, s)


# ------------------------------------------------------------------------------------------------ the scheduler started mid-schedule
def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300) if b != 0.0 else abs(a)


@pytest.mark.parametrize("pred", ["epsilon", "v_prediction"])
@pytest.mark.parametrize("spacing,offset", [("leading", 1), ("linspace", 0), ("trailing", 0)])
def test_scheduler_scalars_match_the_reference(spacing, offset, pred):
    from tests.edit_ref import EditDPMSolverPP2M
    from textboost_amd.sampler import DPMSolverPP2M
    steps = 8
    sch = DPMSolverPP2M.from_config({"prediction_type": pred, "timestep_spacing": spacing, "steps_offset": offset})
    ref = EditDPMSolverPP2M(prediction_type=pred, timestep_spacing=spacing, steps_offset=offset)
    assert sch.set_timesteps(steps) == ref.set_timesteps(steps).tolist()
    worst = 0.0
    for begin in (0, 1, 4, 7):
        ref.set_begin(begin)
        for i in range(begin, steps):
            for got, want in zip(sch.coefficients(i, begin) + sch.data_prediction_scalars(i), ref.coefficients(i) + ref.data_prediction_scalars(i)):
                worst = max(worst, _rel(got, want))
                assert _rel(got, want) <= 1e-9, (begin, i, got, want)
        # step `begin` is first order (no history), and so is the last; between them the steps use the previous data prediction
        assert sch.coefficients(begin, begin)[2] == 0.0 and sch.coefficients(steps - 1, begin)[2] == 0.0
        assert all(sch.coefficients(i, begin)[2] != 0.0 for i in range(begin + 1, steps - 1))
    for i in range(steps + 1):
        for got, want in zip(sch.noise_scalars(i), ref.noise_scalars(i)):
            assert _rel(got, want) <= 1e-9, (i, got, want)
        a, s = sch.noise_scalars(i)
        assert abs(a * a + s * s - 1.0) < 1e-12
    assert sch.noise_scalars(steps) == (1.0, 0.0)
    print(f"[edit] scheduler scalars vs reference ({spacing}, {pred}): worst relative difference {worst:.2e}")


def test_coefficients_with_begin_zero_are_todays_values():
    """`coefficients(i)` restated as it stood before `begin` existed: the values are the same floats"""
    from textboost_amd.sampler import DPMSolverPP2M

    def before(sch, i):
        a0, st0 = sch.alpha_sigma(sch.sigmas[i])
        a1, st1 = sch.alpha_sigma(sch.sigmas[i + 1])
        if i == len(sch.timesteps) - 1:
            return 0.0, a1, 0.0
        lam0, lam1 = math.log(a0 / st0), math.log(a1 / st1)
        h = lam1 - lam0
        e = math.expm1(-h)
        ca = st1 / st0
        if i == 0:
            return ca, -a1 * e, 0.0
        ap, stp = sch.alpha_sigma(sch.sigmas[i - 1])
        r0 = (lam0 - math.log(ap / stp)) / h
        return ca, -a1 * e * (1.0 + 0.5 / r0), a1 * e * (0.5 / r0)

    for steps in (8, 25, 50):
        sch = DPMSolverPP2M.from_config(None)
        sch.set_timesteps(steps)
        for i in range(steps):
            assert sch.coefficients(i) == before(sch, i) == sch.coefficients(i, 0), (steps, i)


def test_reference_loop_properties_on_a_stand_in_unet():
    """the properties the GPU loop is held to, on the reference itself: kept cells end as z0 bit for bit, an all-ones mask equals no mask, an
    all-zero mask returns z0"""
    from tests.edit_ref import edit_latents
    g = torch.Generator().manual_seed(3)
    B, h, w = 2, 6, 5
    wmix = torch.randn(4, 4, generator=g) * 0.3

    def unet(x, t, ehs):
        return torch.tanh(torch.einsum("oc,bchw->bohw", wmix, x)) * (1.0 + ehs.mean() + t.float().mean() * 1e-3)

    cond, uncond = torch.randn(B, 3, 4, generator=g), torch.randn(B, 3, 4, generator=g)
    z0, noise = torch.randn(1, 4, h, w, generator=g), torch.randn(B, 4, h, w, generator=g)
    mask = torch.zeros(h, w, dtype=torch.uint8)
    mask[1:4, 2:5] = 1
    x = edit_latents(unet, cond, uncond, z0, noise, 0.5, steps=8, mask=mask)
    keep = ~mask.bool()
    assert torch.equal(x[:, :, keep], z0.expand(B, -1, -1, -1)[:, :, keep])
    plain = edit_latents(unet, cond, uncond, z0, noise, 0.5, steps=8)
    assert torch.equal(edit_latents(unet, cond, uncond, z0, noise, 0.5, steps=8, mask=torch.ones(h, w, dtype=torch.uint8)), plain)
    assert torch.equal(edit_latents(unet, cond, uncond, z0, noise, 0.5, steps=8, mask=torch.zeros(h, w, dtype=torch.uint8)), z0.expand(B, -1, -1, -1))
    assert (x[:, :, mask.bool()] - z0.expand(B, -1, -1, -1)[:, :, mask.bool()]).abs().max() > 1e-3


# ------------------------------------------------------------------------------------------------ masks
def test_mask_threshold_and_any_pool():
    from PIL import Image
    from tests.edit_ref import pool_mask_any as ref_pool
    from textboost_amd.edit import pool_mask_any, prepare_mask
    m = np.zeros((128, 128), dtype=np.uint8)
    m[17, 42] = 255
    pixel, latent = prepare_mask(Image.fromarray(m), 128)
    assert pixel.shape == (128, 128) and pixel.dtype == np.uint8 and latent.shape == (16, 16) and latent.dtype == np.uint8
    assert pixel.sum() == 1 and pixel[17, 42] == 1
    assert latent.sum() == 1 and latent[2, 5] == 1                    # one white pixel marks its whole cell, and only that one
    # grey 127 stays black, 128 becomes white
    grey = np.zeros((128, 128), dtype=np.uint8)
    grey[0, 0], grey[64, 64] = 127, 128
    pixel, latent = prepare_mask(Image.fromarray(grey), 128)
    assert pixel[0, 0] == 0 and pixel[64, 64] == 1 and pixel.sum() == 1 and latent[8, 8] == 1 and latent.sum() == 1
    # pooling against the loop reference, and without touching its input
    rng = np.random.default_rng(0)
    p = (rng.random((64, 40)) < 0.02).astype(np.uint8)
    before = p.copy()
    assert np.array_equal(pool_mask_any(p), ref_pool(p)) and np.array_equal(p, before)
    assert 0 < pool_mask_any(p).sum() < pool_mask_any(p).size
    with pytest.raises(ValueError):
        pool_mask_any(np.zeros((12, 16), dtype=np.uint8))
    # an RGB mask of another size and aspect: the photo's geometry (short edge to S, centre crop), NEAREST
    from textboost_amd.edit import edit_geometry
    assert edit_geometry(300, 200, 128) == (192, 128, 32, 0) and edit_geometry(200, 300, 128) == (128, 192, 0, 32)
    assert edit_geometry(128, 128, 128) == (128, 128, 0, 0)
    wide = np.zeros((200, 300, 3), dtype=np.uint8)
    wide[:, :150] = 255                                               # the left half is white
    pixel, latent = prepare_mask(Image.fromarray(wide), 128)
    assert pixel[:, :64].all() and not pixel[:, 64:].any() and latent[:, :8].all() and not latent[:, 8:].any()


# ------------------------------------------------------------------------------------------------ inference.py
def test_parser_accepts_the_edit_flags():
    import inference
    p = inference.build_parser()
    a = p.parse_args(["run"])
    assert a.init_image is None and a.mask is None and a.strength is None and a.no_paste is False
    a = p.parse_args(["run", "--init-image", "photo.jpg", "--mask", "m.png", "--strength", "0.9", "--no-paste"])
    assert (a.init_image, a.mask, a.strength, a.no_paste) == ("photo.jpg", "m.png", 0.9, True)
    assert inference.DEFAULT_STRENGTH == 0.8


def test_edit_refusals_come_before_the_device_is_consulted(tmp_path, monkeypatch):
    pytest.importorskip("transformers")
    from PIL import Image
    from safetensors.torch import save_file
    import inference
    from tests.test_gpu_generate import _write_tokenizer, write_trained_run
    mdir, rdir = str(tmp_path / "model"), str(tmp_path / "runs" / "dog")
    _write_tokenizer(os.path.join(mdir, "tokenizer"))
    write_trained_run(rdir, ["<dog>"], ["<hflip>"], seed=1)
    os.makedirs(os.path.join(mdir, "vae"))
    vae_file = os.path.join(mdir, "vae", "diffusion_pytorch_model.safetensors")
    save_file({"decoder.conv_in.bias": torch.zeros(4), "post_quant_conv.bias": torch.zeros(4)}, vae_file)
    photo, mask, small, junk = (str(tmp_path / n) for n in ("photo.png", "mask.png", "small.png", "junk.png"))
    Image.fromarray(np.full((96, 160, 3), 90, dtype=np.uint8)).save(photo)
    Image.fromarray(np.zeros((96, 160), dtype=np.uint8)).save(mask)
    Image.fromarray(np.zeros((96, 128), dtype=np.uint8)).save(small)
    with open(junk, "wb") as f:
        f.write(b"not a picture")

    def consulted():
        raise AssertionError("torch.cuda was consulted")
    monkeypatch.setattr(torch.cuda, "is_available", consulted)
    common = [rdir, "--model", mdir, "--prompt", "photo of a <dog> dog", "--steps", "8"]
    init = ["--init-image", photo]
    refusals = [
        (["--mask", mask], "--mask needs --init-image"),
        (["--strength", "0.5"], "--strength needs --init-image"),
        (init + ["--strength", "0"], "outside"),
        (init + ["--strength", "-0.1"], "outside"),
        (init + ["--strength", "1.5"], "outside"),
        (init + ["--strength", "0.124"], "none of the 8 steps"),
        (init + ["--strength", "0.1"], "none of the 8 steps"),
        (["--init-image", str(tmp_path / "absent.png")], "cannot be read"),
        (["--init-image", junk], "cannot be read"),
        (init + ["--mask", str(tmp_path / "absent_mask.png")], "cannot be read"),
        (init + ["--mask", junk], "cannot be read"),
        (init + ["--mask", small], "128 x 96.*160 x 96"),
        (init, "encoder"),                                  # a decoder-only VAE file
        (init + ["--mask", mask, "--strength", "0.5"], "encoder"),
    ]
    for extra, match in refusals:
        with pytest.raises(SystemExit, match=match):
            inference.main(common + extra)
    # the refusals of before still come first
    with pytest.raises(SystemExit, match="cat"):
        inference.main(common + init + ["--strength", "7", "--attn-map", "cat"])
    # with the encoder half in the file, valid combinations pass every host check and reach the device question
    save_file({"decoder.conv_in.bias": torch.zeros(4), "post_quant_conv.bias": torch.zeros(4), "encoder.conv_in.bias": torch.zeros(4),
               "quant_conv.bias": torch.zeros(8)}, vae_file)
    for extra in (init, init + ["--strength", "0.125"], init + ["--mask", mask], init + ["--mask", mask, "--strength", "1.0", "--no-paste"],
                  init + ["--mask", mask, "--attn-map", "<dog>"], []):
        with pytest.raises(AssertionError, match="consulted"):
            inference.main(common + extra)
