"""The pre-LN ViT image tower of the evaluation metrics, forward only, on the HIP kernels, and what the metrics share around it.

`HipViT` is the one schedule of both towers (clip_score.HipCLIPVision, dino_score.HipDINOv2): each of them maps its checkpoint onto the weight
layout below and names the five points where the two networks differ.  Arithmetic is the text encoder's "autocast" mode: fp32 residual stream
and LayerNorm statistics, 16-bit GEMM and attention operands.  Also here: `pack_patch_weight`, `load_rgb` and `ImageEvaluator`, the image
batching and tower timing of both metrics.
"""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Sequence

import torch

from . import _lib as L
from . import augment, ops

# OpenAI CLIP's Normalize (clip/clip.py `_transform`, open_clip OPENAI_DATASET_MEAN / STD)
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


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


def load_rgb(path: str):
    import numpy as np
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB"))


class HipViT:
    """geo: image_size, patch_size, hidden_size, intermediate_size, num_layers, num_heads, eps.  Weights arrive as fp32 source values (only
    `patch_w` is packed already: pack_patch_weight) and are cast and placed here: patch_w half [D, Kp], patch_b [D], cls [D], pos [T, D]
    (T = 1 + patches), norm = the final LayerNorm's (weight, bias), layers[i] = {"ln1.w", "ln1.b", "qkv.w" ([q | k | v] rows), "qkv.b",
    "out.w", "out.b", "ln2.w", "ln2.b", "fc1.w", "fc1.b", "fc2.w", "fc2.b"}.  Where the towers differ, and nowhere else:
      act         fc1's activation: L.ACT_QUICK_GELU (OpenAI CLIP) or L.ACT_GELU (erf; DINOv2).
      round_bias  Linear biases pass through the 16-bit operand type before they are stored as fp32: True reproduces a model whose Linear
                  layers were cast to 16 bit whole, as the text encoder does for CLIP; False keeps a checkpoint's fp32 bias (DINOv2).
      pre_ln      CLIP's `pre_layrnorm` (weight, bias): the patch embedding lands in a buffer of its own and this LayerNorm writes the
                  residual stream.  Without it the patch embedding is the residual stream.
      layers[i]["ls1"], ["ls2"]   DINOv2's LayerScale, both or neither: fp32 `col_scale` of the two GEMMs that write the residual stream
                  (not folded into the 16-bit weight: gamma trains from 1e-5 and gamma * W would fall into fp16's subnormal range).
      proj        the head.  With a projection [out_dim, D] (CLIP's `visual_projection`) the final LayerNorm writes 16-bit rows that feed the
                  projection GEMM.  Without one it writes the fp32 result, and a non-finite feature raises: the headroom of real DINOv2-L
                  activations under 16-bit operands is not measured, and an overflow must not become a score."""

    def __init__(self, geo, *, patch_w: torch.Tensor, patch_b: torch.Tensor, cls: torch.Tensor, pos: torch.Tensor,
                 layers: Sequence[Dict[str, torch.Tensor]], norm, act: int, round_bias: bool, pre_ln=None,
                 proj: Optional[torch.Tensor] = None, device="cuda"):
        self.geo, self.dev, self.act = geo, device, act
        hd = L.half_dtype()
        f16 = lambda t: t.detach().to(hd).to(device).contiguous()
        f32 = lambda t: t.detach().float().reshape(-1).to(device).contiguous()
        bias = (lambda t: t.detach().to(hd).float().to(device).contiguous()) if round_bias else f32
        self.tokens = 1 + (geo.image_size // geo.patch_size) ** 2
        self.patch_w, self.patch_b, self.cls = f16(patch_w), f32(patch_b), f32(cls)
        self.pos = pos.detach().float().to(device).contiguous()
        assert self.pos.shape == (self.tokens, geo.hidden_size), self.pos.shape
        self.pre_ln = tuple(map(f32, pre_ln)) if pre_ln is not None else None
        self.norm = tuple(map(f32, norm))
        self.proj = f16(proj) if proj is not None else None
        self.out_dim = proj.shape[0] if proj is not None else geo.hidden_size
        self.layers: List[Dict[str, torch.Tensor]] = []
        for src in layers:
            W = {}
            for n in ("qkv", "out", "fc1", "fc2"):
                W[n + ".w"], W[n + ".b"] = f16(src[n + ".w"]), bias(src[n + ".b"])
            for n in ("ln1", "ln2"):
                W[n + ".w"], W[n + ".b"] = f32(src[n + ".w"]), f32(src[n + ".b"])
            W["ls1"], W["ls2"] = (f32(src["ls1"]), f32(src["ls2"])) if "ls1" in src else (None, None)
            self.layers.append(W)
        self._bufs: Dict[int, Dict[str, torch.Tensor]] = {}

    def _buffers(self, B: int):
        b = self._bufs.get(B)
        if b is None:
            g = self.geo
            T, D, I, M = self.tokens, g.hidden_size, g.intermediate_size, B * self.tokens
            hd, f32 = L.half_dtype(), torch.float32
            z = lambda r, c, dt: torch.empty(r, c, device=self.dev, dtype=dt)
            b = {"h": z(M, D, f32), "h2": z(M, D, f32), "x": z(M, D, hd), "qkv": z(M, 3 * D, hd), "o": z(M, D, hd), "a": z(M, I, hd),
                 "ls": z(M, 2, f32), "lse": z(B * g.num_heads, T, f32), "cls_s": z(B, 2, f32)}
            if self.pre_ln is not None:
                b["e"] = z(M, D, f32)
            if self.proj is not None:
                b["cls"] = z(B, D, hd)
            self._bufs = {B: b}   # one batch size at a time: the evaluation encodes full batches and one ragged tail
        return b

    def _blocks(self, images: torch.Tensor, n_layers: int):
        """patch embedding, pre-LayerNorm and the first `n_layers` blocks -> (the fp32 residual stream [B * T, D], this batch size's buffers)"""
        g = self.geo
        B, S, S2 = images.shape
        if S != g.image_size or S2 != g.image_size:
            raise ValueError(f"images are {S}x{S2}, the tower takes {g.image_size}x{g.image_size}")
        T, D, H = self.tokens, g.hidden_size, g.num_heads
        bf = self._buffers(B)
        h, h2, x, qkv, o, a, ls, lse = (bf[k] for k in ("h", "h2", "x", "qkv", "o", "a", "ls", "lse"))
        e = h if self.pre_ln is None else bf["e"]
        ops.clip_patch_embed(images, g.patch_size, self.patch_w, self.patch_b, self.cls, self.pos, e)
        if self.pre_ln is not None:
            ops.layernorm_fwd(e, h, *self.pre_ln, ls, g.eps)
        for W in self.layers[:n_layers]:
            ops.layernorm_fwd(h, x, W["ln1.w"], W["ln1.b"], ls, g.eps)
            ops.gemm(x, W["qkv.w"], qkv, bias=W["qkv.b"])
            ops.attention_fwd(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], o, lse, B, H, T, T, D // H, causal=False)
            ops.gemm(o, W["out.w"], h2, bias=W["out.b"], R=h, col_scale=W["ls1"])        # x + [ls1 *] attn
            ops.layernorm_fwd(h2, x, W["ln2.w"], W["ln2.b"], ls, g.eps)
            ops.gemm(x, W["fc1.w"], a, bias=W["fc1.b"], act=self.act)
            ops.gemm(a, W["fc2.w"], h, bias=W["fc2.b"], R=h2, col_scale=W["ls2"])        # x + [ls2 *] mlp
        return h, bf

    def hidden_states(self, images: torch.Tensor, n_layers: int) -> torch.Tensor:
        """images as for `encode` -> the fp32 residual stream [B, T, D] after the first `n_layers` blocks (n_layers = num_layers - 1: the
        penultimate layer LLaVA-style projectors read).  A view of the tower's buffer: the next call overwrites it."""
        if not 0 <= n_layers <= len(self.layers):
            raise ValueError(f"n_layers = {n_layers}, the tower has {len(self.layers)} blocks")
        h, _ = self._blocks(images, n_layers)
        return h.view(images.shape[0], self.tokens, self.geo.hidden_size)

    def encode(self, images: torch.Tensor) -> torch.Tensor:
        """images: int32 RGBX [B, S, S] (S = image_size; rows and images may be strided) -> fp32 [B, out_dim]: the CLS rows after the final
        LayerNorm, projected (unnormalised) where the tower has a projection"""
        g = self.geo
        h, bf = self._blocks(images, len(self.layers))
        B, T, D = images.shape[0], self.tokens, g.hidden_size
        cls_rows = h.as_strided((B, D), (T * D, 1))                                       # the CLS row of every image
        out = torch.empty(B, self.out_dim, device=self.dev, dtype=torch.float32)
        y = out if self.proj is None else bf["cls"]
        ops.layernorm_fwd(cls_rows, y, *self.norm, bf["cls_s"], g.eps)
        if self.proj is not None:
            ops.gemm(y, self.proj, out)
        elif not bool(torch.isfinite(out).all()):
            raise FloatingPointError(f"{type(self).__name__}: non-finite CLS feature (a 16-bit GEMM / attention operand overflowed)")
        return out


class ImageEvaluator:
    """the image batching of a metric around one tower, and the tower's throughput over everything it encoded"""

    def __init__(self, tower: HipViT, batch_size: int, device):
        self.tower, self.geo, self.batch_size, self.dev = tower, tower.geo, batch_size, device
        self.tower_seconds, self.tower_images = 0.0, 0

    def encode_paths(self, paths: Sequence[str], preprocess_fn: Callable[[torch.Tensor, int], torch.Tensor]) -> torch.Tensor:
        """-> fp32 [len(paths), out_dim] in batches of `batch_size`; preprocess_fn(resident RGBX image [H, W], S) -> an [S, S] view"""
        S = self.geo.image_size
        out = torch.empty(len(paths), self.tower.out_dim, device=self.dev)
        for i in range(0, len(paths), self.batch_size):
            chunk = paths[i:i + self.batch_size]
            batch = torch.empty(len(chunk), S, S, dtype=torch.int32, device=self.dev)
            for j, p in enumerate(chunk):
                batch[j].copy_(preprocess_fn(augment.to_device_image(load_rgb(p)), S))
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            out[i:i + len(chunk)] = self.tower.encode(batch)
            t1.record()
            t1.synchronize()
            self.tower_seconds += t0.elapsed_time(t1) / 1e3
            self.tower_images += len(chunk)
        return out

    def images_per_second(self) -> float:
        return self.tower_images / self.tower_seconds if self.tower_seconds > 0 else 0.0
