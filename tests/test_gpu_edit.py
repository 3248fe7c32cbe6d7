"""Image editing on the GPU (inference.py --init-image / --mask; csrc/edit.hip, `HipSampler.denoise_from`, `Pipeline.edit_images`):
the two kernels against `tb_dpm_step` / float64 / numpy, the loop against tests/edit_ref.py on the tiny models of tests/test_gpu_sampler.py,
and the whole path on the tiny model directory of tests/test_gpu_generate.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
dev = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TB_EINVAL = -22


def f32(v):
    """the float the C ABI receives for a Python float"""
    return float(np.float32(v))


# ------------------------------------------------------------------------------------------------ tb_dpm_step_blend
@pytest.mark.parametrize("shape", [(3, 4, 5, 7), (2, 4, 16, 16)])      # 420 elements: a partial last block, hw = 35 does not divide 256
@pytest.mark.parametrize("half", ["fp16", "bf16"])
def test_dpm_step_blend_is_dpm_step_plus_the_select(half, shape):
    from textboost_amd import _lib as L
    from textboost_amd import ops
    B, C, h, w = shape
    n, hw = C * h * w, h * w
    with L.use_half(half):
        hd = L.half_dtype()
        g = torch.Generator().manual_seed(11)
        x0, mp = torch.randn(B, n, generator=g).to(dev), torch.randn(B, n, generator=g).to(dev)
        e = (torch.randn(2 * B, n, generator=g) * 0.8).to(hd).to(dev)
        z0, noise = (torch.randn(n, generator=g) * 0.9).to(dev), torch.randn(B, n, generator=g).to(dev)
        step = (7.5, 0.8, 0.6, 0.9, 0.3, -0.1)          # guidance, alpha_t, sigma_t, ca, cb, cc
        xs, ms, x2s = x0.clone(), mp.clone(), torch.zeros(2 * B, n, device=dev, dtype=hd)
        ops.dpm_step(xs, e, ms, x2s, n, B, *step)
        masks = {"random": (torch.rand(hw, generator=g) < 0.5).to(torch.uint8), "ones": torch.ones(hw, dtype=torch.uint8),
                 "zeros": torch.zeros(hw, dtype=torch.uint8)}
        assert 0 < masks["random"].sum() < hw
        z0b = z0[None].expand(B, n)
        for name, mask in masks.items():
            rep = mask.bool().repeat(C)[None].expand(B, n).to(dev)        # element j of an image belongs to cell j % hw
            for ka, ks in ((0.7, 0.714), (1.0, 0.0)):
                xb, mb, x2b = x0.clone(), mp.clone(), torch.zeros(2 * B, n, device=dev, dtype=hd)
                ops.dpm_step_blend(xb, e, mb, x2b, n, B, *step, z0, noise, mask.to(dev), ka, ks)
                assert torch.equal(mb, ms), (name, "m_prev is the unblended data prediction")
                assert torch.equal(xb[rep], xs[rep]), (name, "repainted elements are tb_dpm_step's bits")
                want = f32(ka) * z0b.double() + f32(ks) * noise.double()
                bound = 2.0 ** -22 * ((f32(ka) * z0b.double()).abs() + (f32(ks) * noise.double()).abs())
                err = (xb.double() - want).abs()
                print(f"[edit] blend {half} {shape} {name} ({ka}, {ks}): kept max err / bound "
                      f"{(err / bound.clamp_min(1e-300))[~rep].max().item() if (~rep).any() else 0.0:.3f}")
                assert (err <= bound)[~rep].all(), name
                if (ka, ks) == (1.0, 0.0):
                    assert torch.equal(xb[~rep], z0b[~rep]), name
                assert torch.equal(x2b[:B], xb.to(hd)) and torch.equal(x2b[B:], xb.to(hd)), name
        # argument checks
        lib = L.lib()
        mk = masks["random"].to(dev)
        xb, mb, x2b = x0.clone(), mp.clone(), torch.zeros(2 * B, n, device=dev, dtype=hd)
        good = [L.ptr(xb), L.ptr(e), L.ptr(mb), L.ptr(x2b), n, B, *step, L.ptr(z0), L.ptr(noise), L.ptr(mk), hw, 0.5, 0.5, L.stream()]
        for k in (0, 1, 2, 3, 12, 13, 14):
            bad = list(good)
            bad[k] = None
            assert lib.tb_dpm_step_blend(*bad) == TB_EINVAL, k
        for k, v in ((15, hw + 1), (15, 0), (4, 0), (5, 0), (7, 0.0)):     # n_per_b % hw != 0, empty sizes, alpha_t = 0
            bad = list(good)
            bad[k] = v
            assert lib.tb_dpm_step_blend(*bad) == TB_EINVAL, (k, v)
        assert torch.equal(xb, x0)                  # a refused call launched nothing
        assert lib.tb_dpm_step_blend(*good) == 0
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ tb_img_paste
def test_img_paste_is_a_per_pixel_select():
    from textboost_amd import _lib as L
    from textboost_amd import ops
    g = torch.Generator().manual_seed(5)

    def rnd(h, w):
        return torch.randint(-2 ** 31, 2 ** 31 - 1, (h, w), generator=g, dtype=torch.int64).to(torch.int32)

    for (h, w), stride in (((13, 9), 16), ((128, 128), 128)):
        gen, orig, out = rnd(h, stride).to(dev), rnd(h, stride).to(dev), torch.full((h, stride), 77, dtype=torch.int32, device=dev)
        mask = ((torch.rand(h, stride, generator=g) < 0.4) * torch.randint(1, 256, (h, stride), generator=g)).to(torch.uint8).to(dev)
        got = ops.img_paste(gen[:, :w], orig[:, :w], mask[:, :w], out=out[:, :w])
        want = np.where(mask.cpu().numpy()[:, :w] != 0, gen.cpu().numpy()[:, :w], orig.cpu().numpy()[:, :w])
        assert np.array_equal(got.cpu().numpy(), want)
        assert (out[:, w:] == 77).all()             # nothing beyond the row's w pixels is written
        assert 0 < (mask[:, :w] != 0).sum() < h * w
        assert np.array_equal(ops.img_paste(gen[:, :w], orig[:, :w], mask[:, :w]).cpu().numpy(), want)
    lib = L.lib()
    good = [L.ptr(gen), 128, L.ptr(orig), 128, L.ptr(mask), 128, L.ptr(out), 128, 128, 128, L.stream()]
    for k, v in ((0, None), (2, None), (4, None), (6, None), (1, 127), (3, 127), (5, 127), (7, 127), (8, 0), (9, 0)):
        bad = list(good)
        bad[k] = v
        assert lib.tb_img_paste(*bad) == TB_EINVAL, (k, v)
    assert lib.tb_img_paste(*good) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the loop against tests/edit_ref.py
B_, HW_, D_, STEPS_ = 2, 16, 64, 8
BOUND = 3e-2      # the bound tests/test_gpu_sampler.py holds for the (longer) text-to-image loop on the same models


def rel_l2(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


@pytest.fixture(scope="module")
def rig():
    """the models of test_guided_sampling_loop_matches_oracle_on_tiny_models, one sampler, one set of inputs"""
    from oracle.vae_encoder import VAEConfig
    from tests.test_gpu_model import make_unet
    from tests.test_gpu_sampler import _decoder_pair
    from textboost_amd import _lib as L
    from textboost_amd.sampler import HipSampler
    from textboost_amd.vae import VAEGeometry
    L.set_half("fp16")
    ref_unet, hip_unet, _ = make_unet(2 * B_, HW_, D_, seed=5)
    _, hip_dec = _decoder_pair(VAEConfig.tiny(), VAEGeometry(block_out_channels=(64, 64, 128, 128), layers_per_block=1), 14, B_, HW_, HW_)
    g = torch.Generator().manual_seed(7)
    cond = torch.randn(B_, 77, D_, generator=g).half().float()
    uncond = torch.randn(B_, 77, D_, generator=g).half().float() * 0.5
    z0 = torch.randn(1, 4, HW_, HW_, generator=g) * 0.9
    noise = torch.randn(B_, 4, HW_, HW_, generator=g)
    mask = torch.zeros(HW_, HW_, dtype=torch.uint8)
    mask[4:11, 3:9] = 1                                   # rows 4..10, cols 3..8
    r = dict(ref_unet=ref_unet, unet=hip_unet, dec=hip_dec, smp=HipSampler(hip_unet, hip_dec, steps=STEPS_, guidance=7.5), cond=cond,
             uncond=uncond, z0=z0, noise=noise, mask=mask, refs={})
    return r


def _hip(rig, strength, mask=None, smp=None):
    smp = smp or rig["smp"]
    c, u = rig["cond"].view(B_ * 77, D_).to(dev), rig["uncond"].view(B_ * 77, D_).to(dev)
    return smp.denoise_from(c, u, rig["z0"].to(dev), rig["noise"].to(dev), strength, mask=None if mask is None else mask.to(dev)).clone()


def _ref(rig, strength, mask=None):
    from tests.edit_ref import edit_latents
    key = (strength, None if mask is None else bytes(mask.numpy().tobytes()))
    if key not in rig["refs"]:
        with torch.no_grad():
            rig["refs"][key] = edit_latents(lambda x, t, e: rig["ref_unet"](x.half().float(), t, e), rig["cond"], rig["uncond"], rig["z0"],
                                            rig["noise"], strength, steps=STEPS_, guidance=7.5, mask=mask)
    return rig["refs"][key]


@pytest.mark.parametrize("case,strength,masked", [("a", 0.5, False), ("b", 0.5, True), ("c", 1.0, False), ("d", 0.125, False)])
def test_edit_loop_matches_the_reference(rig, case, strength, masked):
    from textboost_amd.edit import strength_begin
    mask = rig["mask"] if masked else None
    x, x_ref = _hip(rig, strength, mask), _ref(rig, strength, mask)
    z0b = rig["z0"].expand(B_, -1, -1, -1)
    if masked:
        m = mask.bool()
        e = rel_l2(x.cpu()[:, :, m], x_ref[:, :, m])
        assert torch.equal(x.cpu()[:, :, ~m], z0b[:, :, ~m]) and torch.equal(x_ref[:, :, ~m], z0b[:, :, ~m])   # kept cells are z0 bit for bit
    else:
        e = rel_l2(x, x_ref)
    moved = rel_l2(x_ref, z0b)
    print(f"[edit] loop ({case}) strength {strength}, begin {strength_begin(STEPS_, strength)}, {'masked' if masked else 'no mask'}: rel-L2 "
          f"{e:.3e} (bound {BOUND}); the reference moved {moved:.3f} from z0")
    assert moved > BOUND                 # the result is not the photo: returning z0 would miss the bound
    assert e < BOUND


def test_all_ones_mask_is_no_mask_and_all_zero_mask_is_the_photo(rig):
    plain = _hip(rig, 0.5)
    assert torch.equal(_hip(rig, 0.5, torch.ones(HW_, HW_, dtype=torch.uint8)), plain)
    assert torch.equal(_hip(rig, 0.5, torch.zeros(HW_, HW_, dtype=torch.uint8)).cpu(), rig["z0"].expand(B_, -1, -1, -1))
    assert not torch.equal(_hip(rig, 0.5, rig["mask"]), plain)


def test_no_state_leaks_between_calls(rig):
    from textboost_amd.sampler import HipSampler
    c, u = rig["cond"].view(B_ * 77, D_).to(dev), rig["uncond"].view(B_ * 77, D_).to(dev)
    lat = torch.randn(B_, 4, HW_, HW_, generator=torch.Generator().manual_seed(9)).to(dev)
    t2i = rig["smp"].denoise(c, u, latents=lat).clone()
    _hip(rig, 0.5, rig["mask"])
    after = _hip(rig, 1.0)
    fresh = _hip(rig, 1.0, smp=HipSampler(rig["unet"], rig["dec"], steps=STEPS_, guidance=7.5))
    assert torch.equal(after, fresh)                                    # strength 0.5 first, then 1.0 == a fresh sampler's 1.0
    assert torch.equal(rig["smp"].denoise(c, u, latents=lat), t2i)       # text-to-image before and after an edit: the same bits
    with pytest.raises(ValueError):
        _hip(rig, 0.1)
    from textboost_amd.sampler import DDPMAncestral
    anc = HipSampler(rig["unet"], rig["dec"], steps=STEPS_, guidance=7.5, scheduler="DDPMScheduler")
    assert isinstance(anc.sch, DDPMAncestral)
    with pytest.raises(NotImplementedError, match="DPM-Solver"):
        _hip(rig, 0.5, smp=anc)


# ------------------------------------------------------------------------------------------------ the whole path
def _photo(h=150, w=200):
    """a smooth colour picture with some texture, uint8 [h, w, 3]"""
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    rng = np.random.default_rng(4)
    img = np.stack([128 + 100 * np.sin(x / 23) * np.cos(y / 31), 128 + 90 * np.cos(x / 17 + y / 29), 60 + 0.8 * x + 0.2 * y], axis=-1)
    return np.clip(img + rng.normal(0, 6, img.shape), 0, 255).astype(np.uint8)


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    from PIL import Image
    from safetensors.torch import load_file, save_file
    from tests.test_gpu_generate import write_model_dir, write_trained_run
    from textboost_amd import generate as G
    from textboost_amd import models
    from textboost_amd.vae import VAEGeometry, vae_encoder_shapes
    d = tmp_path_factory.mktemp("edit")
    mdir, rdir = str(d / "model"), str(d / "runs" / "dog")
    write_model_dir(mdir)
    vfile = os.path.join(mdir, "vae", "diffusion_pytorch_model.safetensors")
    dec_sd = load_file(vfile)
    plain = str(d / "decoder_only")                       # a model directory whose VAE file has no encoder half
    os.makedirs(os.path.join(plain, "vae"))
    save_file(dec_sd, os.path.join(plain, "vae", "diffusion_pytorch_model.safetensors"))
    with open(os.path.join(plain, "vae", "config.json"), "w") as f:
        json.dump({"block_out_channels": [64, 64, 128, 128], "layers_per_block": 1, "scaling_factor": 0.18215}, f)
    vgeo = VAEGeometry(block_out_channels=(64, 64, 128, 128), layers_per_block=1)
    enc_sd = {k: v.half().float() for k, v in models.random_state_dict(vae_encoder_shapes(vgeo), 15, device="cpu").items()}
    save_file({**dec_sd, **enc_sd}, vfile)
    write_trained_run(rdir, ["<dog>"], ["<hflip>"], seed=2)
    photo, maskf = str(d / "photo.png"), str(d / "mask.png")
    rgb = _photo()
    Image.fromarray(rgb).save(photo)
    m = np.zeros(rgb.shape[:2], dtype=np.uint8)
    m[40:110, 60:150] = 255
    Image.fromarray(m).save(maskf)
    n, steps = 2, 8
    with torch.no_grad():
        pipe = G.Pipeline.from_model_dir(mdir, n, steps=steps, guidance=7.5, device=dev)
        base = G.load_base_text(mdir, dev)
        run = G.read_run_dir(rdir)
        te, tok = G.load_text_encoder(mdir, run, 2 * n, dev, base=base)
        pipe.set_run(run)
        ids = G.tokenize(tok, [""] * n + ["photo of a <dog> dog"] * n, 77).to(dev)
        states = te.forward(ids, pins=False).view(2, n * 77, -1).clone()
    return dict(mdir=mdir, rdir=rdir, plain=plain, photo=photo, maskf=maskf, rgb=rgb, mask=m, pipe=pipe, cond=states[1], uncond=states[0], d=d)


def test_edit_images_pastes_the_repainted_region_into_the_photo(world):
    from tests.test_gpu_generate import unpack
    from textboost_amd import edit as E
    from textboost_amd import generate as G
    pipe = world["pipe"]
    with torch.no_grad():
        enc = E.EditEncoder(world["mdir"], pipe.size)
        assert enc.S == 128
        init_rgbx, pixels = E.prepare_image(world["rgb"], enc.S)
        assert init_rgbx.shape == (128, 128) and pixels.shape == (1, 3, 128, 128) and float(pixels.abs().max()) <= 1.0
        z0 = enc.encode(pixels)
        assert z0.shape == (1, 4, 16, 16) and torch.isfinite(z0).all()
        assert torch.equal(enc.encode(pixels), z0)          # the mode: no draw, the same latents every time
        pm, lm = E.prepare_mask(E.load_mask(world["maskf"]), enc.S)
        assert 0 < pm.sum() < pm.size and 0 < lm.sum() < lm.size
        pm_d, lm_d = torch.from_numpy(pm).to(dev), torch.from_numpy(lm).to(dev)
        noise = torch.cat([G.seeded_latent(s, pipe.size) for s in (0, 1)]).to(dev)
        args = (world["cond"], world["uncond"], noise, z0, 0.5)
        out = pipe.edit_images(*args, latent_mask=lm_d, pixel_mask=pm_d, init_rgbx=init_rgbx).clone()
        again = pipe.edit_images(*args, latent_mask=lm_d, pixel_mask=pm_d, init_rgbx=init_rgbx).clone()
        plain = pipe.edit_images(*args, latent_mask=lm_d).clone()                    # --no-paste
        x = pipe.sampler.denoise_from(world["cond"], world["uncond"], z0, noise, 0.5, mask=lm_d)
        decoded = pipe.vae.decode_rgbx(x).clone()
    assert out.shape == (2, 128, 128) and out.dtype == torch.int32
    inside = torch.from_numpy(pm.astype(bool))
    o, p, init = unpack(out)[..., :3], unpack(plain)[..., :3], unpack(init_rgbx)[..., :3]
    for b in range(2):
        assert torch.equal(o[b][~inside], init[~inside])              # outside the mask: the prepared photo's bytes
        assert torch.equal(o[b][inside], p[b][inside])                # inside: the decode
        assert (o[b][inside] != init[inside]).any()
    assert (o[0][inside] != o[1][inside]).any()                       # two seeds differ inside the mask
    assert torch.equal(out, again)                                    # a repeat is byte-identical
    assert torch.equal(plain, decoded)                                # without the paste: the plain decode of the edited latents
    assert (p[0][~inside] != init[~inside]).any()                     # ... which is not the photo outside the mask (the VAE round trip)
    with pytest.raises(ValueError, match="both"):
        pipe.edit_images(*args, latent_mask=lm_d, pixel_mask=pm_d)
    # the prepared photo is Pillow's: short edge to 128 with Lanczos, centre crop
    from PIL import Image
    im = Image.fromarray(world["rgb"]).resize((170, 128), Image.LANCZOS).crop((21, 0, 149, 128))
    assert E.edit_geometry(200, 150, 128) == (170, 128, 21, 0)
    assert np.array_equal(init.numpy(), np.asarray(im))


def test_a_decoder_only_vae_file_is_refused_by_name(world):
    from textboost_amd import edit as E
    with pytest.raises(ValueError, match=r"no encoder\.\* / quant_conv\.\* tensors"):
        E.EditEncoder(world["plain"], 16)


def test_cli_edits_a_photo_and_repeats_byte_for_byte(world):
    pytest.importorskip("transformers")
    from PIL import Image
    d = world["d"]
    outs = []
    for name in ("grid.jpg", "grid2.jpg"):
        out = str(d / name)
        cmd = [sys.executable, os.path.join(ROOT, "inference.py"), world["rdir"], "--model", world["mdir"], "--prompt", "photo of a <dog> dog",
               "--init-image", world["photo"], "--mask", world["maskf"], "--strength", "0.5", "--steps", "8", "--seeds", "0", "1", "--output", out]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(d))
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        outs.append(out)
    assert Image.open(outs[0]).size == (256, 128)
    assert open(outs[0], "rb").read() == open(outs[1], "rb").read()
