"""CLIP-T / CLIP-I evaluation of generated images on a HIP CLIP ViT-L/14 (the reference's eval_dreambooth.py:353-453).

Both metrics run OpenAI CLIP ViT-L/14@336px:
  * CLIP-T (`clip_score`, :353-374) -- t2v_metrics `CLIPScore('openai:ViT-L-14-336')`: per image, the cosine of the L2-normalised image and text
    embeddings [3P restated: t2v_metrics is not installed here; its CLIPScore normalises open_clip's `encode_image` / `encode_text` outputs and
    returns their dot product].  open_clip's val transform: BICUBIC resize of the shortest edge to S, centre crop S.
  * CLIP-I (`clip_i`, :377-453) -- `clip.load("ViT-L/14@336px")` image features; for every generated image of an instance and every real image of
    it, max(cos, 0); concatenated over instances, then the mean.  Preprocessing `v2.Resize((512, 512))` (PIL BILINEAR) in front of clip's own
    BICUBIC shortest-edge resize + centre crop.

The weights come from a local transformers `CLIPModel` directory (config.json + model.safetensors; no download).  Every image is decoded by PIL
on the host and becomes a resident RGBX image (augment.py); the resizes are the Pillow-exact kernels of csrc/image.hip, the centre crop is a
strided view and the tower reads it through `tb_clip_patch_embed` (csrc/clip_vision.hip), which folds CLIP's Normalize into its weight.

Arithmetic is the text encoder's "autocast" mode for both towers: fp32 residual stream and LayerNorm statistics, 16-bit GEMM and attention
operands; the image tower's schedule is vit.HipViT.  (The reference runs CLIP-I in clip.load's fp16 model and CLIP-T in fp32 open_clip: DESIGN.md.)
"""
from __future__ import annotations

import json
import os
from dataclasses import dataclass
from typing import Dict, Sequence, Tuple

import torch

from . import _lib as L
from . import augment, ops
from .text_encoder import HF_LAYER, CLIPGeometry, HipTextEncoder
from .vit import CLIP_MEAN, CLIP_STD, HipViT, ImageEvaluator, load_rgb, pack_patch_weight  # noqa: F401  (load_rgb: imported from here too)

CLIP_I_PRE_SIZE = 512   # eval_dreambooth.py:381 `v2.Resize((512, 512))`


@dataclass
class CLIPVisionGeometry:
    """transformers `CLIPVisionConfig` + the model's `projection_dim` (defaults: OpenAI ViT-L/14@336px)."""
    image_size: int = 336
    patch_size: int = 14
    hidden_size: int = 1024
    intermediate_size: int = 4096
    num_layers: int = 24
    num_heads: int = 16
    projection_dim: int = 768
    act: str = "quick_gelu"
    eps: float = 1e-5

    @property
    def num_patches(self) -> int:
        return (self.image_size // self.patch_size) ** 2


def clip_model_geometry_from_config(cfg: dict) -> Tuple[CLIPVisionGeometry, CLIPGeometry, int]:
    """a transformers `CLIPModel` config.json -> (vision geometry, text geometry, the text tower's EOS id).  Anything this path does not build is
    refused instead of being ignored."""
    v, t = cfg.get("vision_config", {}), cfg.get("text_config", {})
    proj = cfg.get("projection_dim", 768)
    for name, c in (("vision", v), ("text", t)):
        if c.get("hidden_act", "quick_gelu") != "quick_gelu":
            raise NotImplementedError(f"CLIP {name} hidden_act={c.get('hidden_act')!r} is not built")
    if v.get("num_channels", 3) != 3:
        raise NotImplementedError("CLIP vision num_channels != 3 is not built")
    vg = CLIPVisionGeometry(image_size=v.get("image_size", 224), patch_size=v.get("patch_size", 32), hidden_size=v.get("hidden_size", 768),
                            intermediate_size=v.get("intermediate_size", 3072), num_layers=v.get("num_hidden_layers", 12),
                            num_heads=v.get("num_attention_heads", 12), projection_dim=proj, eps=v.get("layer_norm_eps", 1e-5))
    tg = CLIPGeometry(vocab_size=t.get("vocab_size", 49408), hidden_size=t.get("hidden_size", 512),
                      intermediate_size=t.get("intermediate_size", 2048), num_layers=t.get("num_hidden_layers", 12),
                      num_heads=t.get("num_attention_heads", 8), max_pos=t.get("max_position_embeddings", 77), act="quick_gelu",
                      eps=t.get("layer_norm_eps", 1e-5))
    if vg.image_size % vg.patch_size or vg.patch_size % 2 or vg.hidden_size % vg.num_heads:
        raise NotImplementedError(f"CLIP vision geometry {vg} is not built (patch must be even and divide image_size)")
    return vg, tg, int(t.get("eos_token_id", 49407))


def load_clip_model(model_dir: str):
    """-> (vision geometry, text geometry, EOS id, fp32 state dict) from a local `CLIPModel` directory."""
    from safetensors.torch import load_file
    with open(os.path.join(model_dir, "config.json")) as f:
        cfg = json.load(f)
    vg, tg, eos = clip_model_geometry_from_config(cfg)
    sd = {k: v.float() for k, v in load_file(os.path.join(model_dir, "model.safetensors")).items()}
    return vg, tg, eos, sd


class HipCLIPVision(HipViT):
    """CLIPVisionModelWithProjection's forward (image_embeds): the `vision_model.*` parameters of a transformers `CLIPModel` state dict and
    `visual_projection` on the shared tower (vit.HipViT)."""

    def __init__(self, geo: CLIPVisionGeometry, state_dict: Dict[str, torch.Tensor], device="cuda"):
        sd, pre = state_dict, "vision_model."
        patch_w, patch_b = pack_patch_weight(sd[pre + "embeddings.patch_embedding.weight"], CLIP_MEAN, CLIP_STD)
        layers = []
        for i in range(geo.num_layers):
            lp = f"{pre}encoder.layers.{i}."
            W = {"qkv.w": torch.cat([sd[lp + HF_LAYER[x] + ".weight"] for x in "qkv"], dim=0),
                 "qkv.b": torch.cat([sd[lp + HF_LAYER[x] + ".bias"] for x in "qkv"], dim=0)}
            for n in ("out", "fc1", "fc2", "ln1", "ln2"):
                W[n + ".w"], W[n + ".b"] = sd[lp + HF_LAYER[n] + ".weight"], sd[lp + HF_LAYER[n] + ".bias"]
            layers.append(W)
        super().__init__(geo, patch_w=patch_w, patch_b=patch_b, cls=sd[pre + "embeddings.class_embedding"],
                         pos=sd[pre + "embeddings.position_embedding.weight"], layers=layers,
                         norm=(sd[pre + "post_layernorm.weight"], sd[pre + "post_layernorm.bias"]), act=L.ACT_QUICK_GELU, round_bias=True,
                         pre_ln=(sd[pre + "pre_layrnorm.weight"], sd[pre + "pre_layrnorm.bias"]), proj=sd["visual_projection.weight"],
                         device=device)


class HipCLIPText:
    """CLIPTextModelWithProjection's forward (text_embeds): HipTextEncoder (autocast, no LoRA, no pins), the row at the first EOS of each prompt
    (what transformers and open_clip pool), text_projection."""

    def __init__(self, geo: CLIPGeometry, state_dict: Dict[str, torch.Tensor], eos_id: int, batch: int = 32, device="cuda"):
        self.geo, self.eos_id, self.dev = geo, eos_id, device
        self.enc = HipTextEncoder(geo, state_dict, batch, mode="autocast", lora_rank=0, device=device)
        self.proj = state_dict["text_projection.weight"].detach().to(L.half_dtype()).to(device).contiguous()

    def encode(self, input_ids: torch.Tensor) -> torch.Tensor:
        """input_ids int64 [B, max_pos], each row holding the EOS id -> fp32 [B, projection_dim]."""
        ids = input_ids.to(self.dev, torch.int64).contiguous()
        B, T = ids.shape
        if T != self.geo.max_pos:
            raise ValueError(f"input_ids are {T} long, the text tower takes {self.geo.max_pos}")
        is_eos = ids == self.eos_id
        if not bool(is_eos.any(dim=1).all()):
            raise ValueError("every prompt needs an EOS token")
        out = self.enc.forward(ids, pins=False)
        rows = torch.arange(B, device=self.dev) * T + is_eos.int().argmax(dim=1)
        pooled = torch.empty(B, self.geo.hidden_size, device=self.dev, dtype=L.half_dtype())
        ops.convert(out[rows], pooled)
        emb = torch.empty(B, self.proj.shape[0], device=self.dev, dtype=torch.float32)
        ops.gemm(pooled, self.proj, emb)
        return emb


# ------------------------------------------------------------------------------------------------------------------ preprocessing
def preprocess(img: torch.Tensor, size: int, clip_i: bool) -> torch.Tensor:
    """resident RGBX image [H, W] -> [size, size] view.  clip_i: BILINEAR to 512 x 512 first (eval_dreambooth.py:381); then BICUBIC resize of the
    shortest edge to `size` and centre crop (clip.load's / open_clip's val transform)."""
    if clip_i:
        img = augment.resize(img, (CLIP_I_PRE_SIZE, CLIP_I_PRE_SIZE), augment.BILINEAR)
    img = augment.resize_short_edge(img, size, augment.BICUBIC)
    H, W = img.shape
    ox, oy = augment._center_crop_offsets(W, H, size, size)   # the short edge is `size`: the crop lies inside the image
    return img[oy:oy + size, ox:ox + size]


class CLIPEvaluator(ImageEvaluator):
    """Both towers of one CLIPModel directory plus the image / text batching of the two metrics."""

    def __init__(self, model_dir: str, batch_size: int = 32, device="cuda", tokenizer=None):
        vg, tg, eos, sd = load_clip_model(model_dir)
        super().__init__(HipCLIPVision(vg, sd, device=device), batch_size, device)
        self.text = HipCLIPText(tg, sd, eos, batch=batch_size, device=device)
        self.tokenizer = tokenizer if tokenizer is not None else load_tokenizer(model_dir)

    def encode_images(self, paths: Sequence[str], clip_i: bool) -> torch.Tensor:
        """-> fp32 [len(paths), projection_dim] image_embeds, in batches of `batch_size`."""
        return self.encode_paths(paths, lambda img, size: preprocess(img, size, clip_i))

    def encode_texts(self, texts: Sequence[str]) -> torch.Tensor:
        out = torch.empty(len(texts), self.geo.projection_dim, device=self.dev)
        T = self.text.geo.max_pos
        for i in range(0, len(texts), self.batch_size):
            chunk = list(texts[i:i + self.batch_size])
            ids = self.tokenizer(chunk, truncation=True, padding="max_length", max_length=T, return_tensors="pt").input_ids
            out[i:i + len(chunk)] = self.text.encode(ids)
        return out

def load_tokenizer(model_dir: str):
    """CLIPTokenizer from the model directory's vocab.json / merges.txt (local files only)."""
    if not os.path.exists(os.path.join(model_dir, "vocab.json")):
        raise FileNotFoundError(f"{model_dir}: no vocab.json / merges.txt for the CLIP tokenizer")
    from transformers import CLIPTokenizer
    return CLIPTokenizer.from_pretrained(model_dir, local_files_only=True)


# ------------------------------------------------------------------------------------------------------------------ metrics
def clip_t_scores(image_embeds: torch.Tensor, text_embeds: torch.Tensor) -> torch.Tensor:
    """per pair: cos of the L2-normalised embeddings (t2v_metrics CLIPScore, [3P restated])."""
    a = image_embeds / image_embeds.norm(dim=-1, keepdim=True)
    b = text_embeds / text_embeds.norm(dim=-1, keepdim=True)
    return (a * b).sum(dim=-1)


def clip_i_scores(generated: torch.Tensor, real: torch.Tensor) -> torch.Tensor:
    """eval_dreambooth.py:426-442 for one instance: max(cos, 0) of every (real, generated) pair, real-major -> flat [R * G]."""
    g = generated / generated.norm(dim=-1, keepdim=True).clamp_min(1e-8)
    r = real / real.norm(dim=-1, keepdim=True).clamp_min(1e-8)
    return (r @ g.t()).clamp_min(0.0).reshape(-1)


def prompt_of(path: str) -> str:
    """eval_dreambooth.py:357-359: the file name without `.png`, `_` -> space."""
    return os.path.basename(path).replace(".png", "").replace("_", " ")
