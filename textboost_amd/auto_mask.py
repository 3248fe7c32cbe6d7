"""Subject masks from cross-attention (make_masks.py, inference.py --mask auto:WORD): where the class word of a prompt
("dog", "sofa") attends in a noised real photo is a training-free segmenter of Stable Diffusion (DAAM and its follow-ups).

    maker = MaskMaker(unet, encoder, text_encode, tokenizer, alphas_cumprod)      # executors the caller already holds
    score = maker.score(rgb, "dog")                                               # fp32 [H, W] on the device, the photo's own size
    mask, stats = maker.mask(rgb, "dog", dilate=4)                                # uint8 [H, W] (255 = subject); stats = (lo, hi, thr, Otsu bin)

One photo is one UNet forward: the photo is squashed to the model's resolution, encoded (the mode, as in editing), noised once per UNet row --
row r at timesteps[r % len(timesteps)] with the noise of seed + r -- and the recorder of attn_maps.py collects the prompt's cross-attention.
The rest is csrc/auto_mask.hip, stream-ordered with no host read in between: the word's maps summed over rows and positions and resized
bilinearly to the photo (`tb_map_word_upsample`, one launch per cross-attention resolution, each resolution divided by its launches and rows,
the resolutions averaged), min / max, a 256-bin histogram, Otsu's threshold, the mask bytes, an optional square dilation.

Stated differences and choices:
  * geometry: the WHOLE photo is squashed to S x S (Pillow-exact Lanczos), not short edge + centre crop as a training image: map <-> photo is
    then a pure axis scaling and no part of the subject is cut off.  Above an aspect ratio of 2 a warning is issued.
  * the resize of the maps is bilinear, not the recorder's bicubic (`AttnMapRecorder.result`): bicubic overshoots below zero next to a peak, and
    the min-max normalisation in front of the threshold would move with the overshoot.
  * timesteps (100, 300, 500) and two draws each are taken from the range the literature uses for attention on real images; they are not
    measured here (no pretrained weights): both are arguments.
"""
from __future__ import annotations

import warnings
from typing import Callable, Sequence, Tuple

import numpy as np
import torch

DEFAULT_TIMESTEPS = (100, 300, 500)
DEFAULT_DRAWS = 2
DEFAULT_PROMPT = "a photo of a {}"
MAX_ASPECT = 2.0
MAX_DILATE = 64      # csrc/auto_mask.hip


def check_photo_size(W: int, H: int, grid_w: int, grid_h: int, what: str = "the photo"):
    """ValueError for a photo smaller than the latent grid in either direction (the map would be shrunk past its own cells); a warning above
    an aspect ratio of MAX_ASPECT (the squash distorts the subject the model sees).  Host only."""
    if W < grid_w or H < grid_h:
        raise ValueError(f"{what} is {W} x {H}: smaller than the {grid_w} x {grid_h} latent grid the attention maps live on")
    if max(W, H) > MAX_ASPECT * min(W, H):
        warnings.warn(f"{what} is {W} x {H}: an aspect ratio above {MAX_ASPECT:g} is squashed hard to the model's square resolution, the mask "
                      "may be poor")


def parse_auto_mask(value):
    """--mask VALUE -> ("auto", word) for `auto:WORD`, ("file", VALUE) otherwise; ValueError for `auto:` without a word"""
    if value.startswith("auto:"):
        word = value[len("auto:"):].strip()
        if not word:
            raise ValueError("auto: needs a word (--mask auto:dog)")
        return "auto", word
    return "file", value


class MaskMaker:
    """`unet`: a HipUNet, all of whose R = unet.B rows run conditional here (no guidance); `encoder`: an `edit.EditEncoder` for the UNet's
    latent size; `text_encode`: int64 ids [R, T] on the device -> text states [R * T, D]; `alphas_cumprod`: the scheduler's table.  Owns one
    `AttnMapRecorder(unet, rows=(0, R))` and every buffer whose size does not depend on the photo.  The UNet is left as it was found
    (`attn_maps` restored)."""

    def __init__(self, unet, encoder, text_encode: Callable, tokenizer, alphas_cumprod, timesteps: Sequence[int] = DEFAULT_TIMESTEPS, seed: int = 0):
        from . import _lib as L
        from .attn_maps import AttnMapRecorder
        from .generate import seeded_latent
        if not timesteps:
            raise ValueError("MaskMaker needs at least one timestep")
        n_train = int(alphas_cumprod.numel())
        for t in timesteps:
            if not 0 <= int(t) < n_train:
                raise ValueError(f"timestep {t} is outside the scheduler's [0, {n_train})")
        if unet.H != unet.W or unet.H != encoder.size:
            raise ValueError(f"the UNet runs {unet.W} x {unet.H} latents, the encoder makes {encoder.size} x {encoder.size}")
        self.unet, self.encoder, self.text_encode, self.tokenizer = unet, encoder, text_encode, tokenizer
        self.R, self.T, self.size, self.S, self.dev = unet.B, unet.T, unet.H, encoder.S, unet.dev
        self.timesteps, self.seed = tuple(int(t) for t in timesteps), int(seed)
        R, size, dev = self.R, self.size, self.dev
        self.recorder = AttnMapRecorder(unet, rows=(0, R))
        self.t_dev = torch.tensor([self.timesteps[r % len(self.timesteps)] for r in range(R)], dtype=torch.int64, device=dev)
        self.acp = alphas_cumprod.to(device=dev, dtype=torch.float32).contiguous()
        self.noise = torch.cat([seeded_latent(self.seed + r, size) for r in range(R)]).to(dev).contiguous()
        self.x0 = torch.zeros(R, 4, size, size, device=dev)
        self.noisy = torch.zeros(R, 4, size, size, device=dev, dtype=L.half_dtype())
        self.pixels = torch.zeros(1, 3, self.S, self.S, device=dev)
        self.stats = torch.zeros(4, device=dev)                   # lo, hi | threshold, Otsu bin
        self.hist = torch.zeros(256, dtype=torch.int32, device=dev)
        from . import ops
        self.range_ws = torch.zeros(ops.SCORE_RANGE_WS, device=dev)

    def weight(self, hw: Tuple[int, int]) -> float:
        """of one resolution in the fused score: 1 / (launches recorded there * rows * resolutions)"""
        rec = self.recorder
        return 1.0 / (rec.count[hw] * rec.nb * len(rec.acc))

    def record(self, rgb_uint8, word: str, prompt: str = DEFAULT_PROMPT):
        """steps 1-5: squash, encode, noise, prompt, one UNet forward with the recorder set -> the word's token positions"""
        from . import _lib as L
        from . import augment, ops
        from .attn_maps import token_positions
        from .generate import tokenize
        rgb = np.asarray(rgb_uint8)
        if rgb.ndim != 3 or rgb.shape[2] != 3 or rgb.dtype != np.uint8:
            raise ValueError(f"MaskMaker takes a uint8 [H, W, 3] photo, not {rgb.dtype} {rgb.shape}")
        check_photo_size(rgb.shape[1], rgb.shape[0], self.size, self.size)
        text = prompt.format(word)
        positions = token_positions(self.tokenizer, text, word, self.T)
        img = augment.resize(augment.to_device_image(rgb), (self.S, self.S), augment.LANCZOS)
        ops.img_to_pixels(img, 0, 0, self.pixels[0])
        z0 = self.encoder.encode(self.pixels)
        self.x0.copy_(z0.expand(self.R, -1, -1, -1))
        ops.add_noise(self.x0, self.noise, self.t_dev, self.acp, self.noisy)
        ids = tokenize(self.tokenizer, [text] * self.R, self.T).to(self.dev)
        ehs = self.text_encode(ids).reshape(self.R * self.T, -1).to(L.half_dtype()).contiguous()
        rec, unet = self.recorder, self.unet
        rec.zero()
        prev, unet.attn_maps = unet.attn_maps, rec
        try:
            unet.forward(self.noisy, self.t_dev, ehs)      # the epsilon prediction is not used
        finally:
            unet.attn_maps = prev
        return positions

    def fuse(self, positions, H: int, W: int) -> torch.Tensor:
        """step 6: the recorder's accumulators -> the score fp32 [H, W]"""
        from . import ops
        score = torch.empty(H, W, device=self.dev, dtype=torch.float32)
        for k, (hw, acc) in enumerate(self.recorder.acc.items()):
            if self.recorder.count[hw] == 0:
                raise RuntimeError(f"no cross-attention launch was recorded at {hw[0]}x{hw[1]}")
            ops.map_word_upsample(acc, hw[0], hw[1], positions, self.weight(hw), score, accumulate=k > 0)
        return score

    def score(self, rgb_uint8, word: str, prompt: str = DEFAULT_PROMPT) -> torch.Tensor:
        """fp32 [H, W] on the device at the photo's own pixel size: the word's share of the cross-attention, averaged over rows, layers and
        resolutions"""
        positions = self.record(rgb_uint8, word, prompt)
        return self.fuse(positions, int(np.asarray(rgb_uint8).shape[0]), int(np.asarray(rgb_uint8).shape[1]))

    def mask_of(self, score: torch.Tensor, soft: bool = False, dilate: int = 0):
        """score fp32 [H, W] -> (mask uint8 [H, W], stats fp32 [4] = lo, hi, threshold, Otsu bin), all on the device: range -> histogram ->
        Otsu -> mask bytes -> optional dilation"""
        from . import ops
        if not 0 <= int(dilate) <= MAX_DILATE:
            raise ValueError(f"dilate {dilate}: 0 .. {MAX_DILATE} pixels")
        minmax, thr = self.stats[0:2], self.stats[2:4]
        ops.score_range(score, minmax, self.range_ws)
        ops.score_hist(score, minmax, self.hist)
        ops.otsu_threshold(self.hist, thr)
        mask = ops.mask_from_score(score, minmax, thr, torch.empty(score.shape, dtype=torch.uint8, device=score.device), soft=soft)
        if dilate:
            mask = ops.mask_dilate(mask, int(dilate))
        return mask, self.stats

    def mask(self, rgb_uint8, word: str, prompt: str = DEFAULT_PROMPT, soft: bool = False, dilate: int = 0):
        """-> (mask uint8 [H, W] on the device: 255 = subject (soft: 0 .. 255), stats fp32 [4] on the device = lo, hi, threshold, Otsu bin;
        a view of a buffer the next call overwrites)"""
        return self.mask_of(self.score(rgb_uint8, word, prompt), soft=soft, dilate=dilate)


def describe(mask: torch.Tensor, stats: torch.Tensor) -> str:
    """the log line's tail: min, max, Otsu bin, foreground share (one device-to-host read)"""
    lo, hi, _, k = (float(v) for v in stats.cpu())
    share = float((mask >= 128).float().mean())
    return f"min {lo:.6g} max {hi:.6g} otsu bin {int(k)} foreground {100.0 * share:.1f}%"
