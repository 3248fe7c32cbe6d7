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
operands.  (The reference runs CLIP-I in clip.load's fp16 model and CLIP-T in fp32 open_clip: DESIGN.md states the deviation.)
"""
from __future__ import annotations

import json
import os
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _lib as L
from . import augment, ops
from .text_encoder import HF_LAYER, CLIPGeometry, HipTextEncoder

# OpenAI CLIP's Normalize (clip/clip.py `_transform`, open_clip OPENAI_DATASET_MEAN / STD)
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
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


def pack_patch_weight(w: torch.Tensor, mean=CLIP_MEAN, std=CLIP_STD, dtype=None):
    """conv weight [D, 3, p, p] -> (W' half [D, Kp], bias fp32 [D]) for `tb_clip_patch_embed`: Normalize folded in, K in the pixel layout's order
    (ky, kx, R G B X) with a zero X column, zero columns up to the MFMA step."""
    D, C, p, _ = w.shape
    assert C == 3
    w64 = w.detach().double().cpu()
    m = torch.tensor(mean, dtype=torch.float64)
    s = torch.tensor(std, dtype=torch.float64)
    wk = torch.zeros(D, p, p, 4, dtype=torch.float64)
    wk[..., :3] = (w64 / (255.0 * s[None, :, None, None])).permute(0, 2, 3, 1)
    K = 4 * p * p
    Kp = (K + 31) // 32 * 32
    packed = torch.zeros(D, Kp, dtype=torch.float64)
    packed[:, :K] = wk.reshape(D, K)
    bias = -(w64 * (m / s)[None, :, None, None]).sum(dim=(1, 2, 3))
    return packed.to(dtype or L.half_dtype()), bias.float()


class HipCLIPVision:
    """CLIPVisionModelWithProjection's forward (image_embeds), forward only, on the HIP kernels."""

    def __init__(self, geo: CLIPVisionGeometry, state_dict: Dict[str, torch.Tensor], device="cuda"):
        self.geo, self.dev = geo, device
        sd, pre = state_dict, "vision_model."
        hd = L.half_dtype()
        f16 = lambda t: t.detach().to(hd).to(device).contiguous()
        f32 = lambda t: t.detach().float().to(device).contiguous()
        f32r = lambda t: t.detach().to(hd).float().to(device).contiguous()   # bias rounded like the GEMM operands (text_encoder.py)
        w, b = pack_patch_weight(sd[pre + "embeddings.patch_embedding.weight"])
        self.patch_w, self.patch_b = w.to(device), b.to(device)
        self.cls = f32(sd[pre + "embeddings.class_embedding"])
        self.pos = f32(sd[pre + "embeddings.position_embedding.weight"])
        assert self.pos.shape == (1 + geo.num_patches, geo.hidden_size), self.pos.shape
        self.pre_g, self.pre_b = f32(sd[pre + "pre_layrnorm.weight"]), f32(sd[pre + "pre_layrnorm.bias"])
        self.post_g, self.post_b = f32(sd[pre + "post_layernorm.weight"]), f32(sd[pre + "post_layernorm.bias"])
        self.proj = f16(sd["visual_projection.weight"])
        self.Wl: List[Dict[str, torch.Tensor]] = []
        for i in range(geo.num_layers):
            lp = f"{pre}encoder.layers.{i}."
            W = {"qkv.w": f16(torch.cat([sd[lp + HF_LAYER[x] + ".weight"] for x in "qkv"], dim=0)),
                 "qkv.b": f32r(torch.cat([sd[lp + HF_LAYER[x] + ".bias"] for x in "qkv"], dim=0))}
            for n in ("out", "fc1", "fc2"):
                W[n + ".w"], W[n + ".b"] = f16(sd[lp + HF_LAYER[n] + ".weight"]), f32r(sd[lp + HF_LAYER[n] + ".bias"])
            for n in ("ln1", "ln2"):
                W[n + ".g"], W[n + ".b"] = f32(sd[lp + HF_LAYER[n] + ".weight"]), f32(sd[lp + HF_LAYER[n] + ".bias"])
            self.Wl.append(W)
        self._bufs: Dict[int, Dict[str, torch.Tensor]] = {}

    def _buffers(self, B: int):
        b = self._bufs.get(B)
        if b is None:
            g = self.geo
            M, D, I = B * (1 + g.num_patches), g.hidden_size, g.intermediate_size
            hd, f32 = L.half_dtype(), torch.float32
            z = lambda r, c, dt: torch.empty(r, c, device=self.dev, dtype=dt)
            b = {"e": z(M, D, f32), "h": z(M, D, f32), "h2": z(M, D, f32), "x": z(M, D, hd), "qkv": z(M, 3 * D, hd), "o": z(M, D, hd),
                 "a": z(M, I, hd), "ls": z(M, 2, f32), "lse": z(B * g.num_heads, 1 + g.num_patches, f32), "cls": z(B, D, hd),
                 "cls_s": z(B, 2, f32)}
            self._bufs = {B: b}   # one batch size at a time: the evaluation encodes full batches and one ragged tail
        return b

    def encode(self, images: torch.Tensor) -> torch.Tensor:
        """images: int32 RGBX [B, S, S] (S = image_size; rows and images may be strided) -> fp32 [B, projection_dim] (unnormalised image_embeds)."""
        g = self.geo
        B, S, S2 = images.shape
        if S != g.image_size or S2 != g.image_size:
            raise ValueError(f"images are {S}x{S2}, the tower takes {g.image_size}x{g.image_size}")
        T, D, H = 1 + g.num_patches, g.hidden_size, g.num_heads
        bf = self._buffers(B)
        e, h, h2, x, qkv, o, a, ls, lse = (bf[k] for k in ("e", "h", "h2", "x", "qkv", "o", "a", "ls", "lse"))
        ops.clip_patch_embed(images, g.patch_size, self.patch_w, self.patch_b, self.cls, self.pos, e)
        ops.layernorm_fwd(e, h, self.pre_g, self.pre_b, ls, g.eps)                       # pre_layrnorm: its output is the residual stream
        for W in self.Wl:
            ops.layernorm_fwd(h, x, W["ln1.g"], W["ln1.b"], ls, g.eps)
            ops.gemm(x, W["qkv.w"], qkv, bias=W["qkv.b"])
            ops.attention_fwd(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], o, lse, B, H, T, T, D // H, causal=False)
            ops.gemm(o, W["out.w"], h2, bias=W["out.b"], R=h)
            ops.layernorm_fwd(h2, x, W["ln2.g"], W["ln2.b"], ls, g.eps)
            ops.gemm(x, W["fc1.w"], a, bias=W["fc1.b"], act=L.ACT_QUICK_GELU)
            ops.gemm(a, W["fc2.w"], h, bias=W["fc2.b"], R=h2)
        cls_rows = h.as_strided((B, D), (T * D, 1))                                     # the CLS row of every image
        ops.layernorm_fwd(cls_rows, bf["cls"], self.post_g, self.post_b, bf["cls_s"], g.eps)
        out = torch.empty(B, g.projection_dim, device=self.dev, dtype=torch.float32)
        ops.gemm(bf["cls"], self.proj, out)
        return out


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


def load_rgb(path: str):
    import numpy as np
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB"))


class CLIPEvaluator:
    """Both towers of one CLIPModel directory plus the image / text batching of the two metrics."""

    def __init__(self, model_dir: str, batch_size: int = 32, device="cuda", tokenizer=None):
        vg, tg, eos, sd = load_clip_model(model_dir)
        self.geo, self.batch_size, self.dev = vg, batch_size, device
        self.vision = HipCLIPVision(vg, sd, device=device)
        self.text = HipCLIPText(tg, sd, eos, batch=batch_size, device=device)
        self.tokenizer = tokenizer if tokenizer is not None else load_tokenizer(model_dir)
        self.tower_seconds, self.tower_images = 0.0, 0

    def encode_images(self, paths: Sequence[str], clip_i: bool) -> torch.Tensor:
        """-> fp32 [len(paths), projection_dim] image_embeds, in batches of `batch_size`."""
        S = self.geo.image_size
        out = torch.empty(len(paths), self.geo.projection_dim, device=self.dev)
        for i in range(0, len(paths), self.batch_size):
            chunk = paths[i:i + self.batch_size]
            batch = torch.empty(len(chunk), S, S, dtype=torch.int32, device=self.dev)
            for j, p in enumerate(chunk):
                batch[j].copy_(preprocess(augment.to_device_image(load_rgb(p)), S, clip_i))
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            out[i:i + len(chunk)] = self.vision.encode(batch)
            t1.record()
            t1.synchronize()
            self.tower_seconds += t0.elapsed_time(t1) / 1e3
            self.tower_images += len(chunk)
        return out

    def encode_texts(self, texts: Sequence[str]) -> torch.Tensor:
        out = torch.empty(len(texts), self.geo.projection_dim, device=self.dev)
        T = self.text.geo.max_pos
        for i in range(0, len(texts), self.batch_size):
            chunk = list(texts[i:i + self.batch_size])
            ids = self.tokenizer(chunk, truncation=True, padding="max_length", max_length=T, return_tensors="pt").input_ids
            out[i:i + len(chunk)] = self.text.encode(ids)
        return out

    def images_per_second(self) -> float:
        return self.tower_images / self.tower_seconds if self.tower_seconds > 0 else 0.0


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
