"""Token attention maps: where a prompt token lands in a generated image.

    rec = AttnMapRecorder(pipe.unet)                      # the conditional half of the guided batch
    rgbx = pipe.images(cond, uncond, latents, maps=rec)   # the same images, byte for byte
    maps = rec.result()                                   # fp32 [images, T, h, w] on the device; sums to 1 over the T tokens at every pixel
    m = word_map(maps, token_positions(tokenizer, prompt, "<dog>", T))

Device work: `ops.attn_token_maps` (csrc/attn_maps.hip) behind every cross-attention forward of `HipUNet.forward` while `unet.attn_maps` is
set: the head mean of softmax(scale q k^T) of that layer, added into one fp32 accumulator per cross-attention resolution.  Aggregation rule
(`result`): every resolution's accumulator is divided by its number of launches (layers x steps), upsampled bicubically to the latent grid,
and the resolutions are averaged with equal weight.  Everything else here is host arithmetic on small arrays."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn.functional as F

MAX_TOKENS = 128   # csrc/attn_maps.hip: all keys of a query in one tile


def cross_attention_maps(unet) -> Dict[Tuple[int, int], int]:
    """{(h_l, w_l): cross-attention layers at that resolution} of a HipUNet, from the names of its attn2 layers"""
    nl = len(unet.geo.block_out_channels)
    out: Dict[Tuple[int, int], int] = {}
    for prefix, _ in unet.xattn:
        part = prefix.split(".")
        level = nl - 1 if part[0] == "mid_block" else (int(part[1]) if part[0] == "down_blocks" else nl - 1 - int(part[1]))
        hw = (unet.H >> level, unet.W >> level)
        out[hw] = out.get(hw, 0) + 1
    return out


class AttnMapRecorder:
    """One fp32 accumulator [nb, T, h_l * w_l] and one launch count per distinct cross-attention resolution of `unet`, for the images
    `rows` = [b0, b1) of its batch (default: the second half -- the conditional rows of a guided call).  All buffers exist after
    construction, so recording allocates nothing and can be captured in a HIP graph; the counts are host integers, so a captured region must
    contain the `zero()` that opens it (as `HipSampler.denoise` does): every replay then accumulates exactly what the capture counted."""

    def __init__(self, unet, rows: Optional[Tuple[int, int]] = None):
        b0, b1 = rows if rows is not None else (unet.B // 2, unet.B)
        if not (0 <= b0 < b1 <= unet.B):
            raise ValueError(f"rows {(b0, b1)} are not a range of the UNet's batch of {unet.B}")
        if not 1 <= unet.T <= MAX_TOKENS:
            raise ValueError(f"token attention maps take at most {MAX_TOKENS} prompt tokens; the UNet is built for {unet.T}")
        self.B, self.b0, self.nb, self.T, self.h, self.w = unet.B, b0, b1 - b0, unet.T, unet.H, unet.W
        self.layers = cross_attention_maps(unet)
        self.acc = {hw: torch.zeros(self.nb, self.T, hw[0] * hw[1], device=unet.dev, dtype=torch.float32) for hw in self.layers}
        self.count = {hw: 0 for hw in self.layers}

    def zero(self):
        for hw, a in self.acc.items():
            a.zero_()
            self.count[hw] = 0

    def record(self, q, k, heads: int, hw: Tuple[int, int], hd: int):
        """one cross-attention layer: q [B * h_l * w_l, heads * hd], k [B * T, heads * hd] (a column slice of the hoisted K/V buffer)"""
        from . import ops
        ops.attn_token_maps(q, k, self.acc[hw], self.B, heads, hw[0] * hw[1], self.T, hd, b0=self.b0, nb=self.nb, w=1.0 / heads, accumulate=True)
        self.count[hw] += 1

    def result(self) -> torch.Tensor:
        """fp32 [nb, T, h, w]: per resolution accumulator / count, bicubic to the latent grid, then the mean over the resolutions"""
        out = None
        for hw, a in self.acc.items():
            if self.count[hw] == 0:
                raise RuntimeError(f"no cross-attention launch was recorded at {hw[0]}x{hw[1]}")
            m = (a / self.count[hw]).view(self.nb, self.T, hw[0], hw[1])
            if hw != (self.h, self.w):
                m = F.interpolate(m, size=(self.h, self.w), mode="bicubic", align_corners=False)
            out = m if out is None else out + m
        return out / len(self.acc)


# ------------------------------------------------------------------------------------------------ host helpers
def run_tokenizer(model_dir: str, run):
    """the model's CLIP tokenizer with the run's learned tokens registered (host only; what `generate.load_text_encoder` hands out)"""
    import os
    from transformers import CLIPTokenizer
    tdir = os.path.join(model_dir, "tokenizer")
    if not os.path.exists(os.path.join(tdir, "vocab.json")):
        raise FileNotFoundError(f"{tdir}: no vocab.json (only local tokenizer files can be loaded)")
    tokenizer = CLIPTokenizer.from_pretrained(tdir, local_files_only=True)
    names = [n for n, _ in run.tokens]
    if names and tokenizer.add_tokens(names) != len(names):
        raise ValueError(f"{run.path}: the tokenizer already contains one of {names}")
    return tokenizer


def token_positions(tokenizer, prompt: str, word: str, T: int) -> List[int]:
    """positions (in the prompt tokenised to length T) of every occurrence of `word`'s tokens: several per occurrence when the word splits
    into sub-tokens or is a multi-vector placeholder.  The start token, the end token and the padding behind it are never returned.
    ValueError when the word does not occur within the first T positions."""
    ids = list(tokenizer(prompt, truncation=True, padding="max_length", max_length=T).input_ids)
    want = list(tokenizer(word, add_special_tokens=False).input_ids)
    if not want:
        raise ValueError(f"{word!r} has no tokens")
    bos, eos = getattr(tokenizer, "bos_token_id", None), getattr(tokenizer, "eos_token_id", None)
    lo = 1 if ids and ids[0] == bos else 0
    hi = ids.index(eos, lo) if eos in ids[lo:] else len(ids)      # everything from the first end token on is end token / padding
    pos: List[int] = []
    n = len(want)
    for i in range(lo, hi - n + 1):
        if ids[i:i + n] == want:
            pos += range(i, i + n)
    if not pos:
        raise ValueError(f"{word!r} does not occur in the first {T} tokens of {prompt!r}")
    return sorted(set(pos))


def word_map(maps, positions: Sequence[int]):
    """[..., T, h, w] -> [..., h, w]: the sum over a word's token positions"""
    return maps[..., list(positions), :, :].sum(-3)


# the overlay's colour ramp: (value in [0, 1], R, G, B), linear in between -- dark blue, cyan, yellow, red
RAMP = ((0.0, 0, 0, 96), (0.35, 0, 200, 255), (0.65, 255, 230, 0), (1.0, 220, 0, 0))
OVERLAY_ALPHA = 0.55


def overlay(rgb_uint8, amap) -> np.ndarray:
    """uint8 [H, W, 3] image + one [h, w] map -> the image blended with the map: min-max rescaled (a constant map becomes all zeros), resized
    bilinearly to the image, coloured through RAMP.  Deterministic host arithmetic."""
    img = np.asarray(rgb_uint8)
    if img.ndim != 3 or img.shape[2] != 3 or img.dtype != np.uint8:
        raise ValueError(f"overlay takes a uint8 [H, W, 3] image, not {img.dtype} {img.shape}")
    m = torch.as_tensor(np.asarray(amap.detach().cpu() if isinstance(amap, torch.Tensor) else amap), dtype=torch.float32)
    lo, hi = float(m.min()), float(m.max())
    m = (m - lo) / (hi - lo) if hi > lo else torch.zeros_like(m)
    m = F.interpolate(m[None, None], size=img.shape[:2], mode="bilinear", align_corners=False)[0, 0].clamp(0, 1).numpy()
    xs = np.array([r[0] for r in RAMP], dtype=np.float32)
    colour = np.stack([np.interp(m, xs, np.array([r[1 + c] for r in RAMP], dtype=np.float32)) for c in range(3)], axis=-1)
    out = (1.0 - OVERLAY_ALPHA) * img.astype(np.float32) + OVERLAY_ALPHA * colour
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)
