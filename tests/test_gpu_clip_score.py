"""GPU tests of the CLIP-T / CLIP-I evaluation: tb_clip_patch_embed against fp32 conv2d, the device preprocessing against Pillow's bytes, both
towers against the golden fixture (transformers) and the fp32 restatement at full ViT-L/14@336px size, and eval_dreambooth.py end to end."""
import csv
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import clip_ref as R
from parity import parity

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return torch.load(os.path.join(golden_dir, "clip_vit_tiny.pt"), weights_only=False)


def _rgbx(u8, junk=None):
    """uint8 [B, S, S, 3] -> resident int32 RGBX [B, S, S]; junk: uint8 [B, S, S] for the X byte"""
    x = torch.as_tensor(np.asarray(u8)).to(torch.int32)
    v = x[..., 0] | (x[..., 1] << 8) | (x[..., 2] << 16)
    if junk is not None:
        v = v | (junk.to(torch.int32) << 24)
    return v.cuda().contiguous()


@pytest.mark.parametrize("half", ["fp16", "bf16"])
@pytest.mark.parametrize("S", [224, 336])
def test_patch_embed_matches_conv(S, half):
    from textboost_amd import _lib as L, ops
    from textboost_amd.clip_score import pack_patch_weight
    torch.cuda.set_device(0)
    g = torch.Generator().manual_seed(S)
    B, D, p = 3, 1024, 14
    P = (S // p) ** 2
    w = torch.randn(D, 3, p, p, generator=g) * 0.03 + torch.linspace(-0.02, 0.03, p)[None, None, None, :]   # asymmetric in kx
    w[:, 1] *= 1.7                                                                                           # and per channel
    cls, pos = torch.randn(D, generator=g), torch.randn(1 + P, D, generator=g) * 0.5
    u8 = torch.randint(0, 256, (B, S, S, 3), generator=g, dtype=torch.uint8)
    ref = torch.cat([cls.expand(B, 1, D), torch.nn.functional.conv2d(R.normalise(u8.numpy()), w, stride=p).flatten(2).transpose(1, 2)], 1)
    ref = (ref + pos[None]).reshape(B * (1 + P), D)
    with L.use_half(half):
        wp, bias = pack_patch_weight(w)
        wp, bias = wp.cuda(), bias.cuda()
        out = torch.full((B * (1 + P), D), float("nan"), device="cuda")
        ops.clip_patch_embed(_rgbx(u8), p, wp, bias, cls.cuda(), pos.cuda(), out)
        junk = torch.randint(0, 256, (B, S, S), generator=g, dtype=torch.uint8)
        out2 = torch.full_like(out, float("nan"))
        ops.clip_patch_embed(_rgbx(u8, junk), p, wp, bias, cls.cuda(), pos.cuda(), out2)
        # a strided crop view of a larger image batch: the tower reads centre crops without a copy
        big = torch.zeros(B, S + 5, S + 9, dtype=torch.int32, device="cuda")
        big[:, 2:2 + S, 3:3 + S] = _rgbx(u8)
        out3 = torch.empty_like(out)
        ops.clip_patch_embed(big[:, 2:2 + S, 3:3 + S], p, wp, bias, cls.cuda(), pos.cuda(), out3)
        torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    parity(f"patch embed S={S} {half}", out, ref, rel=2e-3 if half == "fp16" else 1e-2, ch_dim=1,
           ch_rel=4e-3 if half == "fp16" else 2e-2)
    assert torch.equal(out, out2), "the X byte changed the output"
    assert torch.equal(out, out3)


def test_patch_embed_refuses_bad_shapes():
    from textboost_amd import _lib as L
    buf = torch.zeros(4096, dtype=torch.int32, device="cuda")
    rc = L.lib().tb_clip_patch_embed(L.ptr(buf), 224 * 224, 224, 1, 224, 15, L.ptr(buf), 928, 928, L.ptr(buf), L.ptr(buf), L.ptr(buf),
                                     L.ptr(buf), 64, 64, L.stream())
    assert rc == -22   # odd patch
    rc = L.lib().tb_clip_patch_embed(L.ptr(buf), 224 * 224, 224, 1, 224, 14, L.ptr(buf), 800, 784, L.ptr(buf), L.ptr(buf), L.ptr(buf),
                                     L.ptr(buf), 64, 64, L.stream())
    assert rc == -22   # K not padded to the MFMA step


def _digest(u8):
    a = np.ascontiguousarray(np.asarray(u8, dtype=np.uint8))
    return f"{a.shape[0]}x{a.shape[1]}x{a.shape[2]}:" + hashlib.sha256(a.tobytes()).hexdigest()


def _device_preprocessed(fixture, name):
    """the fixture's images through the device preprocessing named `clip_{i,t}_<size>`, checked byte for byte against Pillow's (by digest):
    -> resident int32 RGBX [B, size, size]"""
    from textboost_amd import augment
    from textboost_amd.clip_score import preprocess
    kind, size = name.rsplit("_", 1)
    out = []
    for i, a in enumerate(fixture["images"]):
        img = preprocess(augment.to_device_image(a.numpy()), int(size), clip_i=kind == "clip_i").contiguous()
        assert _digest(augment.to_host_rgb(img)) == fixture["preprocessed_sha256"][name][i], (name, i, tuple(a.shape))
        out.append(img)
    return torch.stack(out)


def test_preprocessing_matches_pillow(fixture):
    from textboost_amd import augment
    for i, a in enumerate(fixture["images"]):
        got512 = augment.to_host_rgb(augment.resize(augment.to_device_image(a.numpy()), (512, 512), augment.BILINEAR))
        assert _digest(got512) == fixture["preprocessed_sha256"]["bilinear_512"][i], (i, tuple(a.shape))
    for name in ("clip_i_224", "clip_t_224", "clip_i_336", "clip_t_336"):
        _device_preprocessed(fixture, name)


def _towers(fixture):
    from textboost_amd.clip_score import HipCLIPText, HipCLIPVision, clip_model_geometry_from_config
    vg, tg, eos = clip_model_geometry_from_config(fixture["config"])
    sd = {k: v.float() for k, v in fixture["state_dict_fp16"].items()}   # stored as fp16; the fixture's model ran on these values
    return HipCLIPVision(vg, sd), HipCLIPText(tg, sd, eos, batch=4)


def test_tiny_fixture_embeddings_and_clip_t(fixture):
    from textboost_amd.clip_score import clip_t_scores
    vision, text = _towers(fixture)
    for name in ("clip_i_224", "clip_t_224"):
        emb = vision.encode(_device_preprocessed(fixture, name))
        parity(f"tiny image_embeds {name}", emb, fixture["image_embeds"][name], rel=2e-3)
    te = text.encode(fixture["input_ids"])
    parity("tiny text_embeds", te, fixture["text_embeds"], rel=2e-3)
    s = clip_t_scores(vision.encode(_device_preprocessed(fixture, "clip_t_224")), te).cpu()
    assert (s - fixture["clip_t_scores"]).abs().max().item() < 1e-3, (s, fixture["clip_t_scores"])


def test_full_size_vit_l14_336():
    from textboost_amd import models
    from textboost_amd.clip_score import HipCLIPVision
    torch.set_num_threads(min(16, torch.get_num_threads()))
    vg = models.CLIP_VIT_L14_336
    sd = models.random_state_dict(models.clip_model_shapes(vg, models.CLIP_VIT_L14_TEXT), 9)
    cfg = {"vision_config": {"num_hidden_layers": vg.num_layers, "num_attention_heads": vg.num_heads, "layer_norm_eps": vg.eps}}
    g = torch.Generator().manual_seed(2)
    u8 = torch.randint(0, 256, (3, 336, 336, 3), generator=g, dtype=torch.uint8)
    got = HipCLIPVision(vg, sd).encode(_rgbx(u8)).cpu()
    with torch.no_grad():
        ref = R.image_embeds(sd, cfg, R.normalise(u8.numpy()))
    parity("ViT-L/14-336 image_embeds", got, ref, rel=5e-3)
    cos = torch.cosine_similarity(got, ref, dim=1)
    assert cos.min().item() >= 0.9999, cos


# recorded from HipCLIPVision.encode at the commit before the two towers moved onto vit.HipViT (this geometry, B = 3; the same in fp16 and bf16)
_G = "gemm_kernel<64, 64, 0, 64, 4>"
_BLOCK = ["layernorm_fwd", _G, "attn_fwd_kernel", _G, "layernorm_fwd", _G, _G]   # LN1, qkv, attention, out-proj, LN2, fc1, fc2
TINY_TOWER_LAUNCHES = ["clip_patch_embed_kernel", "layernorm_fwd"] + 2 * _BLOCK + ["layernorm_fwd", _G]


def test_tiny_tower_launch_schedule():
    """the tower's launches, in order, by kernel: patch embedding, pre-LayerNorm, per block LN / qkv / attention / out-proj / LN / fc1 / fc2,
    the final LayerNorm on the CLS rows, the projection"""
    from textboost_amd import models, ops
    from textboost_amd.clip_score import CLIPVisionGeometry, HipCLIPVision
    from textboost_amd.text_encoder import CLIPGeometry
    vg = CLIPVisionGeometry(image_size=224, patch_size=14, hidden_size=128, intermediate_size=512, num_layers=2, num_heads=2, projection_dim=64)
    tg = CLIPGeometry(vocab_size=64, hidden_size=32, intermediate_size=64, num_layers=1, num_heads=2, max_pos=8)
    tower = HipCLIPVision(vg, models.random_state_dict(models.clip_model_shapes(vg, tg), 9))
    g = torch.Generator().manual_seed(3)
    x = _rgbx(torch.randint(0, 256, (3, 224, 224, 3), generator=g, dtype=torch.uint8))
    tower.encode(x)
    ops.start_recording()
    tower.encode(x)
    names = [r[0] for r in ops.stop_recording()]
    assert names == TINY_TOWER_LAUNCHES, names


# ------------------------------------------------------------------------------------------------------------------ CLI end to end
def _bytes_to_unicode():
    bs = list(range(ord("!"), ord("~") + 1)) + list(range(ord("¡"), ord("¬") + 1)) + list(range(ord("®"), ord("ÿ") + 1))
    cs, n = bs[:], 0
    for b in range(256):
        if b not in bs:
            bs.append(b)
            cs.append(256 + n)
            n += 1
    return dict(zip(bs, [chr(c) for c in cs]))


def _write_clip_model(d, cfg, sd):
    """a CLIPModel directory: config.json + model.safetensors + a byte-level vocab.json / merges.txt (no merges: one token per byte)"""
    from safetensors.torch import save_file
    os.makedirs(d, exist_ok=True)
    chars = list(_bytes_to_unicode().values())
    vocab = {c: i for i, c in enumerate(chars)}
    vocab.update({c + "</w>": 256 + i for i, c in enumerate(chars)})
    vocab["<|startoftext|>"], vocab["<|endoftext|>"] = 512, 513
    with open(os.path.join(d, "vocab.json"), "w") as f:
        json.dump(vocab, f)
    with open(os.path.join(d, "merges.txt"), "w") as f:
        f.write("#version: 0.2\n")
    with open(os.path.join(d, "config.json"), "w") as f:
        json.dump(dict(cfg, architectures=["CLIPModel"], model_type="clip"), f)
    save_file({k: v.contiguous() for k, v in sd.items()}, os.path.join(d, "model.safetensors"))


def test_cli_end_to_end(tmp_path):
    pytest.importorskip("transformers")
    from PIL import Image
    from transformers import CLIPTokenizer
    from textboost_amd import models
    from textboost_amd.clip_score import clip_model_geometry_from_config
    V = 514
    cfg = {"projection_dim": 64,
           "vision_config": {"image_size": 224, "patch_size": 14, "hidden_size": 128, "intermediate_size": 512, "num_hidden_layers": 2,
                             "num_attention_heads": 2, "hidden_act": "quick_gelu", "layer_norm_eps": 1e-5},
           "text_config": {"vocab_size": V, "hidden_size": 64, "intermediate_size": 256, "num_hidden_layers": 2, "num_attention_heads": 2,
                           "max_position_embeddings": 77, "hidden_act": "quick_gelu", "layer_norm_eps": 1e-5, "eos_token_id": V - 1,
                           "bos_token_id": V - 2, "pad_token_id": V - 1}}
    vg, tg, _ = clip_model_geometry_from_config(cfg)
    sd = models.random_state_dict(models.clip_model_shapes(vg, tg), 13)
    mdir = str(tmp_path / "clip")
    _write_clip_model(mdir, cfg, sd)
    rng = np.random.default_rng(5)
    prompts = ["a_dog_in_the_snow", "a_red_dog", "a_dog_on_the_beach"]

    def img(h, w):
        y, x = np.mgrid[0:h, 0:w]
        c = rng.integers(40, 200, 3)
        return np.clip(c + 60 * np.sin(x / rng.uniform(5, 20))[..., None] + rng.normal(0, 10, (h, w, 3)) + y[..., None] * 0.1, 0,
                       255).astype(np.uint8)
    gen, real = {}, {"train": {}, "val": {}}
    for s in (0, 1):
        for inst in ("dog", "can"):
            d = tmp_path / "bench" / "run-sd15" / f"seed{s}" / inst
            d.mkdir(parents=True)
            for k, pr in enumerate(prompts):
                p = d / f"{pr.replace('dog', inst)}.png"
                Image.fromarray(img(256 + 16 * k, 256)).save(p)
                gen.setdefault(s, {}).setdefault(inst, []).append(str(p))
    for split, n in (("train", 1), ("val", 2)):
        for inst in ("dog", "can"):
            d = tmp_path / split / inst
            d.mkdir(parents=True)
            for k in range(n):
                p = d / f"{k:02d}.jpg"
                Image.fromarray(img(300 + 40 * k, 217)).save(p, quality=95)
                real[split].setdefault(inst, []).append(str(p))
    run = tmp_path / "runs" / "run-sd15"
    run.mkdir(parents=True)
    cmd = [sys.executable, os.path.join(ROOT, "eval_dreambooth.py"), str(run), "--outdir", str(tmp_path / "bench"), "--skip-gen", "--metric",
           "clip-t", "clip-i", "--seeds", "0", "1", "--train-dir", str(tmp_path / "train"), "--val-dir", str(tmp_path / "val"),
           "--clip-model", mdir, "--batch-size", "4"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "images/s" in r.stdout
    rows = list(csv.reader(open(run / "metric_last.csv")))
    assert rows[0] == ["seed", "clip_score", "vqa_score", "clip_i", "clip_i_unseen", "dino", "dino_unseen"]

    # the restatement's metrics: Pillow preprocessing, fp32 towers, the reference's loops
    tok = CLIPTokenizer.from_pretrained(mdir, local_files_only=True)

    def emb(paths, clip_i):
        u8 = np.stack([R.pil_preprocess(np.asarray(Image.open(p).convert("RGB")), 224, clip_i) for p in paths])
        return R.image_embeds(sd, cfg, R.normalise(u8))
    with torch.no_grad():
        real_e = {sp: {i: emb(real[sp][i], True) for i in real[sp]} for sp in real}
        for s, row in zip((0, 1), rows[1:]):
            paths = [p for i in sorted(gen[s]) for p in gen[s][i]]
            ids = tok([R.prompt_of(p) for p in paths], truncation=True, padding="max_length", max_length=77, return_tensors="pt").input_ids
            ct = R.clip_t(emb(paths, False), R.text_embeds(sd, cfg, ids)).mean().item()
            ge = {i: emb(gen[s][i], True) for i in gen[s]}
            ci = R.clip_i(ge, real_e["train"]).mean().item()
            cu = R.clip_i(ge, real_e["val"]).mean().item()
            got = [float(v) for v in row[1:]]
            print(f"[e2e] seed {s}: csv {row[1:]}  restatement {ct:.5f} {ci:.5f} {cu:.5f}")
            assert row[0] == str(s) and got[1] == 0.0 and got[4] == 0.0 and got[5] == 0.0
            for v, want in ((got[0], ct), (got[2], ci), (got[3], cu)):
                assert abs(v - want) <= 1e-3 + 5e-4, (row, ct, ci, cu)   # 1e-3 on the means, plus the CSV's %.3f rounding
