"""The DINO score of generated images on a HIP DINOv2 ViT-L/14 (the reference's eval_dreambooth.py:456-543, `dino_score`).

The reference runs `torch.hub.load('facebookresearch/dinov2', 'dinov2_vitl14')` in fp32 and takes `model(x)`: the CLS row after the final
LayerNorm (the head is Identity) [3P restated: torch.hub and the dinov2 package are not installed here; dinov2/models/vision_transformer.py,
hub entry `vit_large(patch_size=14, img_size=518, init_values=1.0, block_chunks=0, num_register_tokens=0, interpolate_antialias=False,
interpolate_offset=0.1)`].  ViT-L/14: D 1024, 24 blocks, 16 heads (hd 64), MLP 4096 with erf GELU, every LayerNorm eps 1e-6, qkv packed
[q | k | v] with a bias, a patch conv with a bias, no register tokens.  Each block applies LayerScale, a learned per-channel gamma:
    x = x + ls1.gamma * attn(norm1(x));    x = x + ls2.gamma * mlp(norm2(x))
The position embeddings were trained on a 37 x 37 grid (518 px).  At 224 px (16 x 16 patches, T = 257) the hub interpolates them with
`F.interpolate(mode="bicubic", antialias=False, scale_factor=((16 + 0.1) / 37,) * 2)`, its `interpolate_offset` of 0.1 [3P restated];
transformers' Dinov2Model passes `size=(16, 16)` instead, which maps coordinates differently.  The tower uses the hub's formula whichever format
the weights come in (`interpolate_pos_embed`: on the host, once, in fp32).

Preprocessing [3P restated: torchvision's v2 transforms on PIL images]: Resize((512, 512)) then Resize((224, 224)), both Pillow BILINEAR with
uint8 rounding in between, ToTensor, ImageNet Normalize.  Here the two resizes are the Pillow-exact kernels of csrc/image.hip and Normalize is
folded into the patch weight of `tb_clip_patch_embed` (vit.pack_patch_weight), the conv bias added to the fold's bias.

Weights: the hub's checkpoint file (`dinov2_vitl14_pretrain.pth`, ViT-L/14 only) or a local transformers `Dinov2Model` directory (config.json +
model.safetensors).  Both map onto one internal layout, the hub's parameter names and shapes.

The tower is vit.HipViT, the schedule the CLIP metrics run too: fp32 residual stream and LayerNorm statistics, 16-bit GEMM and attention operands.
LayerScale is applied in fp32 in the epilogue of the GEMM that writes the residual stream (`tb_gemm_desc.col_scale`), never folded into the 16-bit
weight: DINOv2 trains gamma from 1e-5, and gamma * W of that size would fall into fp16's subnormal range.  Linear biases stay fp32.
"""
from __future__ import annotations

import json
import os
from dataclasses import dataclass
from typing import Dict, Sequence, Tuple

import torch
import torch.nn.functional as F

from . import _lib as L
from . import augment
from .vit import HipViT, ImageEvaluator, pack_patch_weight

IMAGENET_MEAN = (0.485, 0.456, 0.406)   # eval_dreambooth.py:462 `v2.Normalize`
IMAGENET_STD = (0.229, 0.224, 0.225)
DINO_PRE_SIZE = 512                    # eval_dreambooth.py:459 `v2.Resize((512, 512))`


@dataclass
class DINOv2Geometry:
    """defaults: the hub's dinov2_vitl14, evaluated at 224 px"""
    image_size: int = 224        # the tower's input (eval_dreambooth.py:460 `v2.Resize((224, 224))`)
    patch_size: int = 14
    hidden_size: int = 1024
    intermediate_size: int = 4096
    num_layers: int = 24
    num_heads: int = 16
    pos_grid: int = 37           # side of the patch grid the position embeddings were trained on (518 / 14)
    eps: float = 1e-6
    interpolate_offset: float = 0.1

    @property
    def grid(self) -> int:
        return self.image_size // self.patch_size

    @property
    def num_tokens(self) -> int:
        return 1 + self.grid ** 2


DINOV2_VITL14 = DINOv2Geometry()


def hub_state_shapes(geo: DINOv2Geometry) -> Dict[str, Tuple[int, ...]]:
    """the hub checkpoint's parameters (DinoVisionTransformer with block_chunks = 0, no mask_token): this module's internal layout"""
    D, I, p = geo.hidden_size, geo.intermediate_size, geo.patch_size
    S = {"cls_token": (1, 1, D), "pos_embed": (1, 1 + geo.pos_grid ** 2, D), "patch_embed.proj.weight": (D, 3, p, p),
         "patch_embed.proj.bias": (D,), "norm.weight": (D,), "norm.bias": (D,)}
    for i in range(geo.num_layers):
        b = f"blocks.{i}."
        for n in ("norm1", "norm2"):
            S[b + n + ".weight"] = (D,); S[b + n + ".bias"] = (D,)
        S[b + "attn.qkv.weight"] = (3 * D, D); S[b + "attn.qkv.bias"] = (3 * D,)
        S[b + "attn.proj.weight"] = (D, D); S[b + "attn.proj.bias"] = (D,)
        S[b + "ls1.gamma"] = (D,); S[b + "ls2.gamma"] = (D,)
        S[b + "mlp.fc1.weight"] = (I, D); S[b + "mlp.fc1.bias"] = (I,)
        S[b + "mlp.fc2.weight"] = (D, I); S[b + "mlp.fc2.bias"] = (D,)
    return S


def check_hub_state(sd: Dict[str, torch.Tensor], geo: DINOv2Geometry, what: str = "DINOv2 state dict") -> None:
    """exactly the parameters of `hub_state_shapes(geo)` (plus an unused mask_token), or ValueError / NotImplementedError"""
    if "register_tokens" in sd:
        raise NotImplementedError(f"{what}: DINOv2 with register tokens is not built")
    want = hub_state_shapes(geo)
    missing = sorted(set(want) - set(sd))
    extra = sorted(set(sd) - set(want) - {"mask_token"})
    if missing or extra:
        raise ValueError(f"{what}: not a {geo.num_layers}-block DINOv2 (D {geo.hidden_size}, MLP {geo.intermediate_size}, patch "
                         f"{geo.patch_size}): missing {missing[:4]}, unexpected {extra[:4]}")
    for k, s in want.items():
        if tuple(sd[k].shape) != s:
            raise ValueError(f"{what}: {k} has shape {tuple(sd[k].shape)}, expected {s}")


# ------------------------------------------------------------------------------------------------------------------ transformers' format
def geometry_from_transformers_config(cfg: dict, image_size: int = 224) -> DINOv2Geometry:
    """a transformers `Dinov2Config` (config.json) -> the geometry.  What this path does not build is refused instead of being ignored."""
    if cfg.get("model_type", "dinov2") != "dinov2" or cfg.get("num_register_tokens", 0):
        raise NotImplementedError(f"model_type {cfg.get('model_type')!r}: only Dinov2Model without register tokens is built")
    if cfg.get("use_swiglu_ffn", False):
        raise NotImplementedError("DINOv2 use_swiglu_ffn (the ViT-g MLP) is not built")
    if cfg.get("hidden_act", "gelu") != "gelu":
        raise NotImplementedError(f"DINOv2 hidden_act={cfg.get('hidden_act')!r} is not built (only erf GELU)")
    if not cfg.get("qkv_bias", True) or cfg.get("num_channels", 3) != 3:
        raise NotImplementedError("DINOv2 without a qkv bias or with num_channels != 3 is not built")
    D = cfg.get("hidden_size", 768)
    p, trained = cfg.get("patch_size", 14), cfg.get("image_size", 224)
    geo = DINOv2Geometry(image_size=image_size, patch_size=p, hidden_size=D, intermediate_size=int(D * cfg.get("mlp_ratio", 4)),
                         num_layers=cfg.get("num_hidden_layers", 12), num_heads=cfg.get("num_attention_heads", 12), pos_grid=trained // p,
                         eps=cfg.get("layer_norm_eps", 1e-6))
    if image_size % p or p % 2 or D % geo.num_heads or D % 16:
        raise NotImplementedError(f"DINOv2 geometry {geo} is not built (the patch must be even and divide {image_size})")
    return geo


def hub_state_from_transformers(sd: Dict[str, torch.Tensor], geo: DINOv2Geometry) -> Dict[str, torch.Tensor]:
    """a transformers `Dinov2Model` state dict (an optional `dinov2.` prefix is dropped) -> the hub's names and shapes"""
    sd = {(k[len("dinov2."):] if k.startswith("dinov2.") else k): v for k, v in sd.items()}
    top = {"cls_token": "embeddings.cls_token", "pos_embed": "embeddings.position_embeddings",
           "patch_embed.proj.weight": "embeddings.patch_embeddings.projection.weight",
           "patch_embed.proj.bias": "embeddings.patch_embeddings.projection.bias", "norm.weight": "layernorm.weight", "norm.bias": "layernorm.bias"}
    per_block = {"norm1.weight": "norm1.weight", "norm1.bias": "norm1.bias", "norm2.weight": "norm2.weight", "norm2.bias": "norm2.bias",
                 "attn.proj.weight": "attention.output.dense.weight", "attn.proj.bias": "attention.output.dense.bias",
                 "ls1.gamma": "layer_scale1.lambda1", "ls2.gamma": "layer_scale2.lambda1", "mlp.fc1.weight": "mlp.fc1.weight",
                 "mlp.fc1.bias": "mlp.fc1.bias", "mlp.fc2.weight": "mlp.fc2.weight", "mlp.fc2.bias": "mlp.fc2.bias"}
    used = {"embeddings.mask_token"}
    out = {}
    try:
        for dst, src in top.items():
            out[dst] = sd[src]
            used.add(src)
        for i in range(geo.num_layers):
            t, b = f"encoder.layer.{i}.", f"blocks.{i}."
            for dst, src in per_block.items():
                out[b + dst] = sd[t + src]
                used.add(t + src)
            for kind in ("weight", "bias"):   # the hub's packed [q | k | v]
                parts = [f"{t}attention.attention.{n}.{kind}" for n in ("query", "key", "value")]
                out[b + "attn.qkv." + kind] = torch.cat([sd[k] for k in parts], dim=0)
                used.update(parts)
    except KeyError as e:
        raise ValueError(f"Dinov2Model state dict: missing {e.args[0]}") from None
    extra = sorted(set(sd) - used)
    if extra:
        raise ValueError(f"Dinov2Model state dict: unexpected parameters {extra[:4]}")
    check_hub_state(out, geo, "Dinov2Model state dict")
    return out


def load_dino_model(path: str, image_size: int = 224) -> Tuple[DINOv2Geometry, Dict[str, torch.Tensor]]:
    """-> (geometry, fp32 state dict in the hub's layout) from the hub's checkpoint file (dinov2_vitl14_pretrain.pth; ViT-L/14 only) or a local
    transformers Dinov2Model directory (config.json + model.safetensors)."""
    if os.path.isdir(path):
        from safetensors.torch import load_file
        with open(os.path.join(path, "config.json")) as f:
            geo = geometry_from_transformers_config(json.load(f), image_size)
        sd = {k: v.float() for k, v in load_file(os.path.join(path, "model.safetensors")).items()}
        return geo, hub_state_from_transformers(sd, geo)
    sd = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(sd, dict) or not all(isinstance(v, torch.Tensor) for v in sd.values()):
        raise ValueError(f"{path}: not a state dict")
    geo = DINOv2Geometry(image_size=image_size)
    check_hub_state(sd, geo, f"{path} (the hub's dinov2_vitl14 checkpoint: ViT-L/14 shapes only)")
    return geo, {k: v.float() for k, v in sd.items() if k != "mask_token"}


def interpolate_pos_embed(pos_embed: torch.Tensor, grid: int, offset: float = 0.1) -> torch.Tensor:
    """the hub's `interpolate_pos_encoding` for a square input of grid x grid patches: pos_embed [1, 1 + M^2, D] (M x M trained grid) ->
    fp32 [1 + grid^2, D].  Bicubic, no antialias, scale_factor = (grid + offset) / M on both axes; unchanged when grid == M."""
    pe = pos_embed.detach().float().reshape(-1, pos_embed.shape[-1])
    N, D = pe.shape[0] - 1, pe.shape[1]
    M = int(round(N ** 0.5))
    if M * M != N:
        raise ValueError(f"{N} position embeddings are not a square grid")
    if grid == M:
        return pe.clone()
    s = float(grid + offset) / M
    patch = F.interpolate(pe[1:].reshape(1, M, M, D).permute(0, 3, 1, 2), mode="bicubic", antialias=False, scale_factor=(s, s))
    if tuple(patch.shape[-2:]) != (grid, grid):
        raise ValueError(f"interpolating {M}x{M} position embeddings by {s} gave {tuple(patch.shape[-2:])}, not {grid}x{grid}")
    return torch.cat([pe[:1], patch.permute(0, 2, 3, 1).reshape(grid * grid, D)], dim=0)


# ------------------------------------------------------------------------------------------------------------------ the tower
class HipDINOv2(HipViT):
    """DinoVisionTransformer's forward (the CLS row after the final LayerNorm): a state dict in the hub's layout on the shared tower
    (vit.HipViT)."""

    def __init__(self, geo: DINOv2Geometry, state: Dict[str, torch.Tensor], device="cuda"):
        check_hub_state(state, geo)
        patch_w, fold_b = pack_patch_weight(state["patch_embed.proj.weight"], IMAGENET_MEAN, IMAGENET_STD)
        layers = []
        for i in range(geo.num_layers):
            b = f"blocks.{i}."
            W = {"ls1": state[b + "ls1.gamma"], "ls2": state[b + "ls2.gamma"]}
            for n, k in (("ln1", "norm1"), ("qkv", "attn.qkv"), ("out", "attn.proj"), ("ln2", "norm2"), ("fc1", "mlp.fc1"), ("fc2", "mlp.fc2")):
                W[n + ".w"], W[n + ".b"] = state[b + k + ".weight"], state[b + k + ".bias"]
            layers.append(W)
        super().__init__(geo, patch_w=patch_w, patch_b=(fold_b.double() + state["patch_embed.proj.bias"].double()).float(),
                         cls=state["cls_token"], pos=interpolate_pos_embed(state["pos_embed"], geo.grid, geo.interpolate_offset),
                         layers=layers, norm=(state["norm.weight"], state["norm.bias"]), act=L.ACT_GELU, round_bias=False, device=device)


# ------------------------------------------------------------------------------------------------------------------ evaluation
def preprocess(img: torch.Tensor, size: int = 224) -> torch.Tensor:
    """resident RGBX image [H, W] -> [size, size]: `v2.Resize((512, 512))`, `v2.Resize((size, size))`, both Pillow BILINEAR"""
    img = augment.resize(img, (DINO_PRE_SIZE, DINO_PRE_SIZE), augment.BILINEAR)
    return augment.resize(img, (size, size), augment.BILINEAR)


class DINOEvaluator(ImageEvaluator):
    """the tower of one DINOv2 checkpoint plus the image batching of the metric"""

    def __init__(self, model_path: str, batch_size: int = 32, device="cuda"):
        geo, state = load_dino_model(model_path)
        super().__init__(HipDINOv2(geo, state, device=device), batch_size, device)

    def encode_images(self, paths: Sequence[str]) -> torch.Tensor:
        """-> fp32 [len(paths), D] features, in batches of `batch_size`"""
        return self.encode_paths(paths, preprocess)


def dino_scores(generated: torch.Tensor, real: torch.Tensor, n_seen: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """eval_dreambooth.py:512-534 for one instance: generated [G, D], real [R, D] in sorted order (the first n_seen are the seen images, the
    rest the unseen ones) -> (seen [G], unseen [G]): per generated image the mean cosine to the seen / unseen real images.  No clamp at 0."""
    if not 0 < n_seen < real.shape[0]:
        raise ValueError(f"{real.shape[0]} real images: the DINO score needs 0 < N = {n_seen} < their number")
    cos = torch.cosine_similarity(generated[:, None, :], real[None, :, :], dim=-1)   # [G, R]
    return cos[:, :n_seen].mean(dim=1), cos[:, n_seen:].mean(dim=1)
