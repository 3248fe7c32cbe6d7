"""CPU tests of the weight sets the two evaluation towers hand to the shared ViT (textboost_amd/vit.py): packed on the host (device="cpu", no
GPU library), in both 16-bit builds.  They pin the points where the CLIP and the DINOv2 tower differ: CLIP's Linear biases pass through the
16-bit operand type and DINOv2's do not, DINOv2's patch bias is the float64 sum of the Normalize fold and the conv bias, and which of
pre-LayerNorm / LayerScale / projection each tower carries."""
import pytest
import torch

LINEAR = ("qkv", "out", "fc1", "fc2")


def _off_grid_biases(sd, seed):
    """0.02 * randn: values that neither fp16 nor bf16 represents"""
    g = torch.Generator().manual_seed(seed)
    for k in sd:
        if k.endswith(".bias") and "norm" not in k:
            sd[k] = 0.02 * torch.randn(sd[k].shape, generator=g)
    return sd


def _clip_tower():
    from textboost_amd import models
    from textboost_amd.clip_score import CLIPVisionGeometry, HipCLIPVision
    from textboost_amd.text_encoder import CLIPGeometry
    vg = CLIPVisionGeometry(image_size=56, patch_size=14, hidden_size=64, intermediate_size=128, num_layers=2, num_heads=2, projection_dim=32)
    tg = CLIPGeometry(vocab_size=64, hidden_size=32, intermediate_size=64, num_layers=1, num_heads=2, max_pos=8)
    sd = _off_grid_biases(models.random_state_dict(models.clip_model_shapes(vg, tg), 3), 4)
    return vg, sd, HipCLIPVision(vg, sd, device="cpu")


def _dino_tower():
    from textboost_amd import models
    from textboost_amd.dino_score import DINOv2Geometry, HipDINOv2, hub_state_shapes
    geo = DINOv2Geometry(image_size=56, hidden_size=64, intermediate_size=128, num_layers=2, num_heads=2, pos_grid=7)
    sd = _off_grid_biases(models.random_state_dict(hub_state_shapes(geo), 5), 6)
    return geo, sd, HipDINOv2(geo, sd, device="cpu")


@pytest.mark.parametrize("half", ["fp16", "bf16"])
def test_clip_weight_set(half):
    from textboost_amd import _lib as L
    with L.use_half(half):
        hd = L.half_dtype()
        vg, sd, tower = _clip_tower()
    assert tower.act == L.ACT_QUICK_GELU
    assert tower.pre_ln is not None and tower.proj is not None and tower.proj.dtype == hd and tower.out_dim == vg.projection_dim
    assert torch.equal(tower.proj, sd["visual_projection.weight"].to(hd))
    assert torch.equal(tower.pre_ln[0], sd["vision_model.pre_layrnorm.weight"]) and torch.equal(tower.norm[1], sd["vision_model.post_layernorm.bias"])
    names = {"out": "self_attn.out_proj", "fc1": "mlp.fc1", "fc2": "mlp.fc2"}
    for i, W in enumerate(tower.layers):
        lp = f"vision_model.encoder.layers.{i}."
        assert W["ls1"] is None and W["ls2"] is None
        src = {n: sd[lp + k + ".bias"] for n, k in names.items()}
        src["qkv"] = torch.cat([sd[f"{lp}self_attn.{x}_proj.bias"] for x in "qkv"])
        for n in LINEAR:
            assert W[n + ".b"].dtype == torch.float32 and W[n + ".w"].dtype == hd
            assert torch.equal(W[n + ".b"], src[n].to(hd).float()), (half, i, n)
            assert not torch.equal(W[n + ".b"], src[n]), "the source bias is representable: the test would not see the rounding"


@pytest.mark.parametrize("half", ["fp16", "bf16"])
def test_dino_weight_set(half):
    from textboost_amd import _lib as L
    from textboost_amd.dino_score import IMAGENET_MEAN, IMAGENET_STD
    from textboost_amd.vit import pack_patch_weight
    with L.use_half(half):
        hd = L.half_dtype()
        geo, sd, tower = _dino_tower()
        _, fold = pack_patch_weight(sd["patch_embed.proj.weight"], IMAGENET_MEAN, IMAGENET_STD)
    assert tower.act == L.ACT_GELU
    assert tower.pre_ln is None and tower.proj is None and tower.out_dim == geo.hidden_size
    conv_b = sd["patch_embed.proj.bias"]
    assert tower.patch_b.dtype == torch.float32 and torch.equal(tower.patch_b, (fold.double() + conv_b.double()).float())
    names = {"qkv": "attn.qkv", "out": "attn.proj", "fc1": "mlp.fc1", "fc2": "mlp.fc2"}
    for i, W in enumerate(tower.layers):
        b = f"blocks.{i}."
        assert torch.equal(W["ls1"], sd[b + "ls1.gamma"]) and torch.equal(W["ls2"], sd[b + "ls2.gamma"])
        for n in LINEAR:
            src = sd[b + names[n] + ".bias"]
            assert W[n + ".b"].dtype == torch.float32 and W[n + ".w"].dtype == hd
            assert torch.equal(W[n + ".b"], src), (half, i, n)
            assert not torch.equal(src, src.to(hd).float()), "the source bias is representable: the test would not see a rounding"
