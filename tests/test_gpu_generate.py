"""Image generation from a trained output directory on the GPU (textboost_amd/generate.py, eval_dreambooth.py without --skip-gen, inference.py):
the byte-image kernel bit for bit, the loaded text encoder against the oracle encoder, the whole path against the oracle loop, and the CLIs."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
dev = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TB_EINVAL = -22
D_TEXT, RANK = 64, 4


def byte_expression(x):
    """diffusers: (image / 2 + 0.5).clamp(0, 1), then numpy_to_pil's (images * 255).round().astype("uint8") -- on the CPU in fp32"""
    return ((x / 2 + 0.5).clamp(0, 1) * 255).round().to(torch.uint8)


def unpack(rgbx):
    """int32 RGBX [...] -> uint8 [..., 4] (little endian: R, G, B, X)"""
    a = rgbx.cpu().numpy()
    return torch.from_numpy(a.view(np.uint8).reshape(*a.shape, 4).copy())


# ------------------------------------------------------------------------------------------------ the kernel
def _edge_values():
    k = torch.arange(256, dtype=torch.float32)
    exact = (k / 255 - 0.5) * 2                                   # every k / 255 mapped back to x
    half = ((torch.arange(255, dtype=torch.float32) + 0.5) / 255 - 0.5) * 2      # every half-way point (k + 0.5) / 255
    pts = torch.cat([exact, half])
    up, down = torch.nextafter(pts, torch.tensor(9.0)), torch.nextafter(pts, torch.tensor(-9.0))
    inf = float("inf")
    outside = torch.tensor([-1.5, 1.5, -1.0000001, 1.0000001, -3e38, 3e38, inf, -inf, -0.0, 0.0, 1e-45, -1e-45, 1e-38, -1e-38, 2.0, -2.0])
    v = torch.cat([pts, up, down, torch.nextafter(up, torch.tensor(9.0)), torch.nextafter(down, torch.tensor(-9.0)), outside])
    return v[: v.numel() // 3 * 3] if v.numel() % 3 == 0 else torch.cat([v, v[: 3 - v.numel() % 3]])


@pytest.mark.parametrize("half", ["fp16", "bf16"])
def test_vae_image_rgbx_is_bit_exact(half):
    from textboost_amd import _lib as L
    from textboost_amd import augment, ops
    with L.use_half(half):
        v = _edge_values()
        for shift in (0, 1, 2):         # every value in every channel
            x = torch.roll(v, shift).view(-1, 3)
            n = x.shape[0]
            want = byte_expression(x)
            for ld in (3, 4, 5):
                buf = torch.full((n, ld), float("nan"))
                buf[:, :3] = x
                out = torch.full((n,), -1, dtype=torch.int32, device=dev)
                ops.vae_image_rgbx(buf.to(dev), out, 1, n)
                got = unpack(out)
                assert torch.equal(got[:, :3], want), (half, shift, ld, (got[:, :3] != want).nonzero()[:5])
                assert (got[:, 3] == 0).all()
        # NaN -> 0
        out = torch.empty(2, dtype=torch.int32, device=dev)
        ops.vae_image_rgbx(torch.tensor([[float("nan"), 1.0, float("nan"), 0.0], [0.0, float("nan"), -1.0, 0.0]], device=dev), out, 1, 2)
        assert unpack(out).tolist() == [[0, 255, 0, 0], [128, 0, 0, 0]]
        # a random 512 x 512 batch, ld = 4, junk in the fourth column
        g = torch.Generator().manual_seed(3)
        B, S = 2, 512
        x = torch.randn(B * S * S, 4, generator=g) * 0.8
        x[:, 3] = torch.randn(B * S * S, generator=g) * 1e30
        x[::7, 3] = float("nan")
        out = torch.empty(B, S, S, dtype=torch.int32, device=dev)
        ops.vae_image_rgbx(x.to(dev), out, B, S * S)
        want = byte_expression(x[:, :3]).view(B, S, S, 3)
        got = unpack(out)
        assert torch.equal(got[..., :3], want) and (got[..., 3] == 0).all()
        # the resident image format: augment.to_host_rgb downloads it, augment.to_device_image writes the same words
        assert np.array_equal(augment.to_host_rgb(out[1]), want[1].numpy())
        assert torch.equal(augment.to_device_image(want[0].numpy()), out[0])
        # argument checks
        lib, ok = L.lib(), torch.zeros(4, 4, device=dev)
        o = torch.zeros(4, dtype=torch.int32, device=dev)
        assert lib.tb_vae_image_rgbx(None, 4, L.ptr(o), 1, 4, L.stream()) == TB_EINVAL
        assert lib.tb_vae_image_rgbx(L.ptr(ok), 4, None, 1, 4, L.stream()) == TB_EINVAL
        assert lib.tb_vae_image_rgbx(L.ptr(ok), 2, L.ptr(o), 1, 4, L.stream()) == TB_EINVAL
        assert lib.tb_vae_image_rgbx(L.ptr(ok), 4, L.ptr(o), 0, 4, L.stream()) == TB_EINVAL
        assert lib.tb_vae_image_rgbx(L.ptr(ok), 4, L.ptr(o), 1, 4, L.stream()) == 0
        torch.cuda.synchronize()


def test_decode_rgbx_equals_decode_through_the_byte_expression():
    from oracle.vae_encoder import VAEConfig
    from tests.test_gpu_sampler import _decoder_pair
    from textboost_amd.vae import VAEGeometry
    geo = VAEGeometry(block_out_channels=(64, 64, 128, 128), layers_per_block=1)
    B, h, w = 3, 8, 8
    _, hip = _decoder_pair(VAEConfig.tiny(), geo, 12, B, h, w)
    z = torch.randn(B, 4, h, w, generator=torch.Generator().manual_seed(1)) * 0.18215 * 3     # (x 3: part of the image saturates)
    img = hip.decode(z.to(dev)).clone()
    rgbx = hip.decode_rgbx(z.to(dev))
    assert rgbx.shape == (B, 8 * h, 8 * w) and rgbx.dtype == torch.int32
    want = (img.cpu() * 255).round().to(torch.uint8).permute(0, 2, 3, 1)        # `decode` has applied (x / 2 + 0.5).clamp(0, 1)
    got = unpack(rgbx)
    assert torch.equal(got[..., :3], want) and (got[..., 3] == 0).all()
    print(f"[generate] decode_rgbx: {(want == 0).float().mean():.3f} of the bytes are 0, {(want == 255).float().mean():.3f} are 255")
    assert torch.equal(hip.decode(z.to(dev)), img)          # `decode` is unchanged by the call in between


# ------------------------------------------------------------------------------------------------ a tiny diffusers model directory + trained runs
def _bytes_to_unicode():
    bs = list(range(ord("!"), ord("~") + 1)) + list(range(ord("\xa1"), ord("\xac") + 1)) + list(range(ord("\xae"), ord("\xff") + 1))
    cs, n = bs[:], 0
    for b in range(256):
        if b not in bs:
            bs.append(b)
            cs.append(256 + n)
            n += 1
    return dict(zip(bs, [chr(c) for c in cs]))


def _write_tokenizer(d):
    """a byte-level CLIP vocabulary without merges (as tests/test_gpu_clip_score.py builds one), filled up to CLIP's 49408 entries so that the
    start / end tokens have the ids the TextBoost pins test for (49406 / 49407)"""
    os.makedirs(d, exist_ok=True)
    chars = list(_bytes_to_unicode().values())
    vocab = {c: i for i, c in enumerate(chars)}
    vocab.update({c + "</w>": 256 + i for i, c in enumerate(chars)})
    for i in range(512, 49406):
        vocab[f"fill{i}</w>"] = i
    vocab["<|startoftext|>"], vocab["<|endoftext|>"] = 49406, 49407
    with open(os.path.join(d, "vocab.json"), "w") as f:
        json.dump(vocab, f)
    with open(os.path.join(d, "merges.txt"), "w") as f:
        f.write("#version: 0.2\n")


def _oracle_text(seed=0):
    from oracle.clip_text import CLIPTextCfg, TextBoostEncoder
    torch.manual_seed(seed)
    ccfg = CLIPTextCfg.tiny(D_TEXT)
    base = TextBoostEncoder(ccfg, r=0)
    with torch.no_grad():
        for n, p in base.named_parameters():
            if "ln" in n or n.endswith("bias"):
                p.add_(torch.randn_like(p) * 0.1)
        base.token_embedding.weight.mul_(0.5)
    return ccfg, base


def write_model_dir(d, hw=16):
    """tiny UNet / VAE / text encoder of the oracle's shapes in the layout of a diffusers model directory -> (oracle UNet, oracle decoder, oracle
    base text encoder, its config)"""
    from safetensors.torch import save_file
    from oracle.sampler import VAEDecoder
    from oracle.unet_sd import UNet2DCondition, UNetConfig
    from oracle.vae_encoder import VAEConfig
    from tests.test_gpu_model import round_fp16_
    from textboost_amd import models
    from textboost_amd.vae import VAEGeometry, vae_decoder_shapes
    torch.manual_seed(5)
    ucfg = UNetConfig.tiny(D_TEXT)
    unet = round_fp16_(UNet2DCondition(ucfg))
    with torch.no_grad():
        for n, p in unet.named_parameters():
            if "norm" in n:
                p.add_(torch.randn_like(p) * 0.1)
        round_fp16_(unet)
    os.makedirs(os.path.join(d, "unet"))
    with open(os.path.join(d, "unet", "config.json"), "w") as f:
        json.dump({"block_out_channels": list(ucfg.block_out_channels), "attention_head_dim": list(ucfg.num_heads),
                   "cross_attention_dim": D_TEXT, "sample_size": hw, "layers_per_block": ucfg.layers_per_block}, f)
    save_file({k: v.contiguous() for k, v in unet.state_dict().items()}, os.path.join(d, "unet", "diffusion_pytorch_model.safetensors"))
    vgeo = VAEGeometry(block_out_channels=(64, 64, 128, 128), layers_per_block=1)
    vsd = {k: v.half().float() for k, v in models.random_state_dict(vae_decoder_shapes(vgeo), 14, device="cpu").items()}
    with torch.device("meta"):
        dec = VAEDecoder(VAEConfig.tiny())
    dec = dec.to_empty(device="cpu")
    dec.load_state_dict(vsd)
    os.makedirs(os.path.join(d, "vae"))
    with open(os.path.join(d, "vae", "config.json"), "w") as f:
        json.dump({"block_out_channels": [64, 64, 128, 128], "layers_per_block": 1, "scaling_factor": 0.18215}, f)
    save_file(vsd, os.path.join(d, "vae", "diffusion_pytorch_model.safetensors"))
    ccfg, base = _oracle_text()
    os.makedirs(os.path.join(d, "text_encoder"))
    with open(os.path.join(d, "text_encoder", "config.json"), "w") as f:
        json.dump({"vocab_size": ccfg.vocab_size, "hidden_size": D_TEXT, "intermediate_size": ccfg.intermediate_size,
                   "num_hidden_layers": ccfg.num_layers, "num_attention_heads": ccfg.num_heads, "max_position_embeddings": 77,
                   "hidden_act": "quick_gelu", "layer_norm_eps": 1e-5}, f)
    params = dict(base.named_parameters())
    save_file({hf: params[ours].detach().contiguous() for ours, hf in base.hf_key_map().items()},
              os.path.join(d, "text_encoder", "model.safetensors"))
    _write_tokenizer(os.path.join(d, "tokenizer"))
    os.makedirs(os.path.join(d, "scheduler"))
    with open(os.path.join(d, "scheduler", "scheduler_config.json"), "w") as f:
        json.dump({"_class_name": "PNDMScheduler", "num_train_timesteps": 1000, "beta_start": 0.00085, "beta_end": 0.012,
                   "beta_schedule": "scaled_linear", "prediction_type": "epsilon", "steps_offset": 1}, f)
    return unet, dec, base, ccfg


def write_trained_run(d, tokens, aug, seed):
    """what train_textboost.py leaves in <output_dir>, through checkpoint.py: a rank-4 adapter with non-zero B, placeholder rows [D] and
    augmentation rows [1, D].  -> (lora_A [L, 3r, D], lora_B [L, 3D, r], {token: row})"""
    from textboost_amd import checkpoint as ckpt
    g = torch.Generator().manual_seed(seed)
    L_, D, r = 2, D_TEXT, RANK
    names = list(tokens) + list(aug)
    te = types.SimpleNamespace(geo=types.SimpleNamespace(hidden_size=D, num_layers=L_), r=r, lora_A=torch.randn(L_, 3 * r, D, generator=g) / r,
                               lora_B=torch.randn(L_, 3 * D, r, generator=g) * 0.05, token_table=torch.randn(len(names), D, generator=g) * 0.01)
    ckpt.save_text_encoder_adapter(te, os.path.join(d, "text_encoder"), "tiny")
    ckpt.save_token_embeddings(te, d, {t: i for i, t in enumerate(tokens)}, {t: len(tokens) + i for i, t in enumerate(aug)})
    return te.lora_A, te.lora_B, {t: te.token_table[i] for i, t in enumerate(names)}


def oracle_student(base, ccfg, lora_A, lora_B, rows):
    """the oracle encoder with the same adapter and the same added rows (in id order), its own CPU null embedding"""
    from oracle.clip_text import TextBoostEncoder, add_tokens
    student = TextBoostEncoder(ccfg, r=RANK)
    student.load_state_dict(base.state_dict(), strict=False)
    with torch.no_grad():
        null = base.transformer(torch.tensor([[49406] + [49407] * 76]))[0]
        r, D = RANK, D_TEXT
        for i, layer in enumerate(student.layers):
            for p, m in enumerate((layer.q, layer.k, layer.v)):
                m.lora_A.copy_(lora_A[i, p * r:(p + 1) * r])
                m.lora_B.copy_(lora_B[i, p * D:(p + 1) * D])
        ids = add_tokens(student, [0] * len(rows))
        for tid, row in zip(ids, rows):
            student.token_embedding.weight[tid] = row
    student.set_null_embedding(null)
    return student.eval()


def test_loaded_text_encoder_matches_the_oracle_encoder(tmp_path):
    from parity import parity
    from textboost_amd import generate as G
    mdir, rdir = str(tmp_path / "model"), str(tmp_path / "runs" / "dog")
    _, _, base, ccfg = write_model_dir(mdir)
    A, Bm, rows = write_trained_run(rdir, ["<dog>"], ["<hflip>"], seed=1)
    run = G.read_run_dir(rdir)
    assert [n for n, _ in run.tokens] == ["<dog>", "<hflip>"] and run.rank == RANK
    with torch.no_grad():
        te, tok = G.load_text_encoder(mdir, run, 4, dev)
        assert tok.convert_tokens_to_ids(["<dog>", "<hflip>"]) == [49408, 49409] and te.token_table.shape[0] == 49410
        prompts = ["a <dog> dog in the jungle", "", "a <hflip> photo of a <dog> dog wearing a black top hat and a monocle", "a red <dog> dog"]
        ids = G.tokenize(tok, prompts, 77)
        assert (ids[0] == 49408).sum() == 1 and ids[1, 1] == 49407 and (ids[2] == 49409).sum() == 1
        out = te.forward(ids.to(dev)).view(4, 77, D_TEXT)
        student = oracle_student(base, ccfg, A, Bm, [rows["<dog>"], rows["<hflip>"]])
        ref = student(ids)
    # the bound of tests/test_gpu_model.py for the autocast encoder forward
    parity("loaded encoder hidden states", out, ref, rel=5e-4, maxabs=1e-3, ch_dim=2, ch_rel=2e-3)
    null = te.null_embedding
    assert null.shape == (77, D_TEXT) and te.use_fixed_special_embedding
    assert torch.equal(out[1], null)                                   # the empty prompt yields the null embedding whole
    assert all(torch.equal(out[b, 0], null[0]) for b in range(4))      # row 0 of every prompt is null[0]
    parity("null embedding", null, student.null_embedding, rel=5e-4, maxabs=1e-3)
    # the adapter matters: without it the states are further from the loaded encoder's than 10 x the parity bound above, so that bound could not
    # hold had the adapter not been applied
    with torch.no_grad():
        plain, _ = G.load_text_encoder(mdir, G.TrainedRun(path=rdir, rank=0, lora={}, tokens=run.tokens, files=run.files), 4, dev)
        far = plain.forward(ids.to(dev)).view(4, 77, D_TEXT)
    assert ((far[0] - out[0]).norm() / out[0].norm()).item() > 10 * 5e-4


def test_whole_path_pngs_match_the_oracle_loop(tmp_path):
    """trained directory -> text states -> 8 guided DPM-Solver++ steps (the setting of tests/test_gpu_sampler.py) -> decoder -> PNG, against
    oracle encoder -> oracle.sampler.sample_latents -> decode_latents -> the byte expression.  Bound: mean |delta| <= 2e-2 * 255 + 0.5 levels
    (the bound tests/test_gpu_sampler.py holds for the same loop on [0, 1] images, plus half a level for the rounding to bytes)."""
    from PIL import Image
    from oracle.sampler import sample_latents
    from textboost_amd import generate as G
    mdir, rroot = str(tmp_path / "model"), str(tmp_path / "runs" / "tb-sd15-n1")
    unet, dec, base, ccfg = write_model_dir(mdir)
    A, Bm, rows = write_trained_run(os.path.join(rroot, "dog"), ["<dog>"], ["<hflip>"], seed=2)
    run = G.read_run_dir(os.path.join(rroot, "dog"))
    steps, seed = 8, 5
    out_root = str(tmp_path / "bench" / "tb-sd15-n1")
    with torch.no_grad():
        pipe = G.Pipeline.from_model_dir(mdir, 13, steps=steps, guidance=7.5, device=dev)
        text = G.load_base_text(mdir, dev)
        written = G.generate_instance(pipe, text, run, "dog", [seed], out_root, prompt_batch=16)
    ident = "<dog> dog"
    prompts = G.instance_prompts("dog", ident)
    assert written == [os.path.join(out_root, f"seed{seed}", "dog", G.image_filename(p, ident, "dog")) for p in prompts] and len(written) == 25
    got = torch.stack([torch.from_numpy(np.array(Image.open(p))) for p in written])
    assert got.shape == (25, 128, 128, 3) and got.dtype == torch.uint8
    # the oracle
    _, tok = G.load_text_encoder(mdir, run, 2, dev, base=text)
    student = oracle_student(base, ccfg, A, Bm, [rows["<dog>"], rows["<hflip>"]])
    with torch.no_grad():
        cond = student(G.tokenize(tok, prompts, 77))
        uncond = student(G.tokenize(tok, [""] * 25, 77))
        lat = G.seeded_latent(seed, 16).repeat(25, 1, 1, 1)
        x_ref = sample_latents(lambda x, t, e: unet(x.half().float(), t, e), cond, uncond, lat, steps=steps, guidance=7.5)
        want = byte_expression(dec(x_ref / dec.cfg.scaling_factor)).permute(0, 2, 3, 1)
    delta = (got.float() - want.float()).abs()
    per_image = delta.mean(dim=(1, 2, 3))
    print(f"[generate] PNG vs oracle: mean |delta| {delta.mean():.3f} levels (bound {2e-2 * 255 + 0.5:.2f}), worst image {per_image.max():.3f}, "
          f"max {delta.max():.0f}; image std {want.float().std():.1f} levels")
    assert want.float().std() > 5                  # the images are not flat: the comparison means something
    assert delta.mean() <= 2e-2 * 255 + 0.5
    # results do not depend on the batch an image shares (13 + 12 against 7 + 6 + 6 + 6), beyond fp16 noise
    with torch.no_grad():
        pipe7 = G.Pipeline.from_model_dir(mdir, 7, steps=steps, guidance=7.5, device=dev)
        again = G.generate_instance(pipe7, text, run, "dog", [seed], str(tmp_path / "bench7"), prompt_batch=8)
    got7 = torch.stack([torch.from_numpy(np.array(Image.open(p))) for p in again])
    d7 = (got7.float() - got.float()).abs().mean()
    print(f"[generate] batches 13 + 12 vs 7 + 6 + 6 + 6: mean |delta| {d7:.4f} levels")
    assert d7 <= 2e-2 * 255 + 0.5
    # non-finite latents raise before anything is written
    real = pipe.unet.forward
    pipe.unet.forward = lambda *a, **k: real(*a, **k).fill_(float("nan"))
    try:
        with pytest.raises(FloatingPointError, match="subject dog, seed 5"):
            G.generate_instance(pipe, text, run, "dog", [seed], str(tmp_path / "never"), prompt_batch=16)
    finally:
        pipe.unet.forward = real
    assert not any(f.endswith(".png") for _, _, fs in os.walk(str(tmp_path / "never")) for f in fs)


# ------------------------------------------------------------------------------------------------ the CLIs, end to end in child processes
def _child(cmd, cwd):
    r = subprocess.run([sys.executable] + cmd, capture_output=True, text=True, timeout=900, cwd=cwd)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def test_cli_generates_scores_and_repeats_byte_for_byte(tmp_path):
    pytest.importorskip("transformers")
    from PIL import Image
    from tests.test_gpu_clip_score import _write_clip_model
    from textboost_amd import generate as G
    from textboost_amd import models
    from textboost_amd.clip_score import clip_model_geometry_from_config
    mdir, rroot = str(tmp_path / "model"), str(tmp_path / "runs" / "tb-sd15-n1")
    write_model_dir(mdir)
    write_trained_run(os.path.join(rroot, "dog"), ["<dog>"], ["<hflip>"], seed=3)                 # live subject, one vector
    write_trained_run(os.path.join(rroot, "can"), ["<can_0>", "<can_1>"], [], seed=4)             # object, two vectors
    os.makedirs(os.path.join(rroot, "logs"))
    V = 514
    ccfg = {"projection_dim": 64,
            "vision_config": {"image_size": 224, "patch_size": 14, "hidden_size": 128, "intermediate_size": 512, "num_hidden_layers": 2,
                              "num_attention_heads": 2, "hidden_act": "quick_gelu", "layer_norm_eps": 1e-5},
            "text_config": {"vocab_size": V, "hidden_size": 64, "intermediate_size": 256, "num_hidden_layers": 2, "num_attention_heads": 2,
                            "max_position_embeddings": 77, "hidden_act": "quick_gelu", "layer_norm_eps": 1e-5, "eos_token_id": V - 1,
                            "bos_token_id": V - 2, "pad_token_id": V - 1}}
    vg, tg, _ = clip_model_geometry_from_config(ccfg)
    cdir = str(tmp_path / "clip")
    _write_clip_model(cdir, ccfg, models.random_state_dict(models.clip_model_shapes(vg, tg), 13))
    bench = str(tmp_path / "bench")
    common = [rroot, "--outdir", bench, "--seeds", "0", "1", "--metric", "clip-t", "--clip-model", cdir, "--batch-size", "8"]
    script = os.path.join(ROOT, "eval_dreambooth.py")
    out = _child([script, *common, "--model", mdir], str(tmp_path))              # subjects: the sub-directories that are subjects (not logs/)
    assert "generated 100 images" in out and "wrote" in out
    csv_path = os.path.join(rroot, "metric_last.csv")
    csv_one_shot = open(csv_path, "rb").read()
    idents = {"dog": "<dog> dog", "can": "<can_0> can <can_1> can"}
    first = {}
    for s in (0, 1):
        for inst, ident in idents.items():
            d = os.path.join(bench, "tb-sd15-n1", f"seed{s}", inst)
            names = sorted(os.listdir(d))
            assert names == sorted(G.image_filename(p, ident, inst) for p in G.instance_prompts(inst, ident)) and len(names) == 25
            for n in names:
                assert Image.open(os.path.join(d, n)).size == (128, 128) and Image.open(os.path.join(d, n)).mode == "RGB"
                first[(s, inst, n)] = open(os.path.join(d, n), "rb").read()
    assert len(first) == 100
    for inst in idents:      # different seeds differ; different prompts of a seed differ
        a = np.asarray(Image.open(os.path.join(bench, "tb-sd15-n1", "seed0", inst, f"a_red_{inst}.png"))).astype(int)
        b = np.asarray(Image.open(os.path.join(bench, "tb-sd15-n1", "seed1", inst, f"a_red_{inst}.png"))).astype(int)
        c = np.asarray(Image.open(os.path.join(bench, "tb-sd15-n1", "seed0", inst, f"a_wet_{inst}.png"))).astype(int)
        assert np.abs(a - b).mean() > 1.0 and np.abs(a - c).max() > 0
    os.remove(csv_path)
    _child([script, *common, "--skip-gen"], str(tmp_path))
    assert open(csv_path, "rb").read() == csv_one_shot
    rows = [l.split(",") for l in csv_one_shot.decode().split()]
    assert rows[0][0] == "seed" and [r[0] for r in rows[1:]] == ["0", "1"]
    # a second run: byte-identical files and CSV; --instances picks the subjects by name
    os.remove(csv_path)
    _child([script, *common, "--model", mdir, "--instances", "dog", "can"], str(tmp_path))
    for (s, inst, n), data in first.items():
        assert open(os.path.join(bench, "tb-sd15-n1", f"seed{s}", inst, n), "rb").read() == data, (s, inst, n)
    assert open(csv_path, "rb").read() == csv_one_shot
    # inference.py: one grid of len(seeds) images, or one file per seed
    inf = os.path.join(ROOT, "inference.py")
    grid = str(tmp_path / "grid.jpg")
    _child([inf, os.path.join(rroot, "dog"), "--model", mdir, "--prompt", "photo of a <dog> dog", "--seeds", "0", "1", "2", "--output", grid,
            "--steps", "10"], str(tmp_path))
    assert Image.open(grid).size == (3 * 128, 128)
    _child([inf, os.path.join(rroot, "can"), "--model", mdir, "--prompt", "a <can_0> <can_1> can", "--seeds", "4", "--steps", "10"], str(tmp_path))
    assert Image.open(str(tmp_path / "a_<can_0>_<can_1>_can_4.jpg")).size == (128, 128)
