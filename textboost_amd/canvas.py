"""Window geometry of the MultiDiffusion canvas (Bar-Tal et al. 2023, diffusers' StableDiffusionPanoramaPipeline): host
arithmetic only, no device and no kernel library.

A latent canvas of Hc x Wc cells is covered by S x S windows (S = the model's own latent size).  Per axis, with length L and stride s:

    n = ceil((L - S) / s) + 1          o_k = min(k s, L - S)

so the last window is clamped to the edge, the offsets are strictly increasing and L == S gives [0].  Windows are the cartesian product,
k = iy * nx + ix; image-window pairs p = img * nw + k are cut into chunks of `unet_batch`, the last of which may be ragged.  The same
tables, scaled by the VAE's factor, place the decoded tiles (`tile_plan`).
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Tuple

import torch

MAX_WINDOWS = 4096   # per image


class CanvasError(ValueError):
    pass


def axis_offsets(L: int, S: int, stride: int) -> List[int]:
    """the window origins of one axis"""
    L, S, stride = int(L), int(S), int(stride)
    if S < 1:
        raise CanvasError(f"window {S}: at least 1")
    if L < S:
        raise CanvasError(f"a side of {L} is below the window's {S}")
    if not 1 <= stride <= S:
        raise CanvasError(f"stride {stride}: 1 .. {S} (a larger stride leaves cells that no window covers)")
    n = -(-(L - S) // stride) + 1
    return [min(k * stride, L - S) for k in range(n)]


@dataclass
class CanvasPlan:
    S: int
    Hc: int
    Wc: int
    stride: int
    n_images: int = 1
    unet_batch: int = 13
    oy: List[int] = field(init=False)
    ox: List[int] = field(init=False)

    def __post_init__(self):
        self.S, self.Hc, self.Wc, self.stride = int(self.S), int(self.Hc), int(self.Wc), int(self.stride)
        self.n_images, self.unet_batch = int(self.n_images), int(self.unet_batch)
        if self.n_images < 1:
            raise CanvasError(f"{self.n_images} images: at least 1")
        if self.unet_batch < 1:
            raise CanvasError(f"UNet batch {self.unet_batch}: at least 1")
        self.oy = axis_offsets(self.Hc, self.S, self.stride)
        self.ox = axis_offsets(self.Wc, self.S, self.stride)
        if self.nw > MAX_WINDOWS:
            raise CanvasError(f"{self.ny} x {self.nx} = {self.nw} windows per image: at most {MAX_WINDOWS} (raise the stride)")
        self._dev = {}

    @property
    def ny(self) -> int:
        return len(self.oy)

    @property
    def nx(self) -> int:
        return len(self.ox)

    @property
    def nw(self) -> int:
        return self.ny * self.nx

    @property
    def pairs(self) -> int:
        return self.n_images * self.nw

    @property
    def n_chunks(self) -> int:
        return -(-self.pairs // self.unet_batch)

    def windows(self) -> List[Tuple[int, int]]:
        """(oy, ox) of window k = iy * nx + ix"""
        return [(y, x) for y in self.oy for x in self.ox]

    def pair(self, p: int) -> Tuple[int, int]:
        """(image, window) of pair p"""
        if not 0 <= p < self.pairs:
            raise IndexError(f"pair {p}: 0 .. {self.pairs - 1}")
        return divmod(p, self.nw)

    def chunks(self) -> List[List[int]]:
        """the pairs of every chunk, in order; all of `unet_batch` pairs but possibly the last"""
        Bu = self.unet_batch
        return [list(range(c * Bu, min((c + 1) * Bu, self.pairs))) for c in range(self.n_chunks)]

    def tables(self, device, scale: int = 1):
        """(oy_host, ox_host, oy_dev, ox_dev): the origins times `scale` as int32 tensors, what the canvas kernels take (the host copies are
        checked, the device ones read); made once per (device, scale)"""
        key = (str(device), int(scale))
        if key not in self._dev:
            oy, ox = torch.tensor(self.oy, dtype=torch.int32) * int(scale), torch.tensor(self.ox, dtype=torch.int32) * int(scale)
            self._dev[key] = (oy, ox, oy.to(device), ox.to(device))
        return self._dev[key]


def tile_plan(S: int, Hc: int, Wc: int, decode_stride: int, n_images: int, decoder_batch: int) -> CanvasPlan:
    """the decoded tiles of a canvas: S x S latents at `decode_stride`, decoded `decoder_batch` at a time (origins in latent cells; times the
    VAE's factor in pixels)"""
    return CanvasPlan(S, Hc, Wc, decode_stride, n_images, decoder_batch)


def blend_ramp(S: int, decode_stride: int, factor: int) -> int:
    """the feather of `tb_tile_blend` in pixels: the overlap of two neighbouring tiles, at least 1"""
    return max(1, int(factor) * (int(S) - int(decode_stride)))
