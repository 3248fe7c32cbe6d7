"""Editing a photo with a trained run (inference.py --init-image / --mask): what diffusers 0.29's
`StableDiffusionImg2ImgPipeline` does, and with a mask the latent blend of `StableDiffusionInpaintPipeline` for a 4-channel UNet
[3P: diffusers is not installed here; both are restated from their published `__call__`, as sampler.py restates the scheduler].

    strength_begin(steps, strength)            -> the first step that runs (`get_timesteps`: t_start = max(steps - min(int(steps s), steps), 0))
    prepare_image(rgb, S)                      -> (resident RGBX [S, S], pixel_values fp32 [1, 3, S, S]): short edge to S (Lanczos), centre crop --
                                                  the geometry of a training image (augment.DeviceFeeder with center_crop)
    prepare_mask(mask, S)                      -> (pixel mask uint8 [S, S], latent mask uint8 [S/8, S/8]) on the host: convert("L"), the same
                                                  resize (NEAREST) and crop, >= 128 = repaint; a latent cell is repainted if ANY of its pixels is
    EditEncoder(model_dir, size).encode(px)    -> z0 = mean * scaling_factor, fp32 [1, 4, size, size]: `HipVAEEncoder` at batch 1, noise zero

The sampler side is `HipSampler.denoise_from` (one `tb_dpm_step_blend` launch per step: the step and the select), the pixel side
`generate.Pipeline.edit_images` (`tb_img_paste` on the resident RGBX bytes).

Stated differences from diffusers:
  * z0 is the mode of the encoder's distribution, not a sample of it (`retrieve_latents(..., generator)` samples): the same photo gives the
    same z0 for every seed, so a seed changes the noise only.
  * the latent mask is the any-pool of the pixel mask (diffusers interpolates the mask to the latent grid and so picks one pixel per 8 x 8
    cell): every cell the marked region touches is regenerated, none of it is kept from the photo.
  * with a mask at strength 1 the loop still starts from alpha_0 z0 + sigma_0 noise (sigma_0 / alpha_0 is above 10 at SD's betas, so the photo is
    under a tenth of the noise's scale there); diffusers' inpaint pipeline starts from pure noise in that case.
"""
from __future__ import annotations

import os
from typing import Optional, Tuple

import numpy as np

VAE_FILE = os.path.join("vae", "diffusion_pytorch_model.safetensors")


def strength_begin(steps: int, strength: float) -> int:
    """the index of the first step that runs: steps begin .. steps-1.  ValueError for a strength outside (0, 1] or one that runs no step."""
    s = float(strength)
    if not 0.0 < s <= 1.0:
        raise ValueError(f"strength {strength} is outside (0, 1]")
    begin = max(steps - min(int(steps * s), steps), 0)
    if begin >= steps:
        raise ValueError(f"strength {strength} runs none of the {steps} steps (int({steps} * {strength}) = 0): raise the strength or the steps")
    return begin


def edit_geometry(W: int, H: int, S: int) -> Tuple[int, int, int, int]:
    """(resized width, resized height, crop x, crop y) of a W x H photo: `v2.Resize(S)` (augment.resize_short_edge) + the centre crop of
    augment.DeviceFeeder"""
    short, long = (W, H) if W <= H else (H, W)
    new_long = int(S * long / short)
    nw, nh = (S, new_long) if W <= H else (new_long, S)
    return nw, nh, max(0, int(round((nw - S) / 2.0))), max(0, int(round((nh - S) / 2.0)))


def load_rgb(path: str) -> np.ndarray:
    """a picture file -> uint8 [H, W, 3]; OSError (Pillow's UnidentifiedImageError is one) when it cannot be read"""
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB"))


def load_mask(path: str):
    """a mask file -> PIL "L" image"""
    from PIL import Image
    with Image.open(path) as im:
        return im.convert("L")


def pool_mask_any(pixel_mask: np.ndarray, cell: int = 8) -> np.ndarray:
    """uint8 [H, W] (non-zero = repaint) -> uint8 [H / cell, W / cell]: 1 where ANY pixel of the cell is marked.  The input is not changed."""
    H, W = pixel_mask.shape
    if H % cell or W % cell:
        raise ValueError(f"a {W} x {H} mask does not divide into {cell} x {cell} cells")
    return (pixel_mask.reshape(H // cell, cell, W // cell, cell) != 0).any(axis=(1, 3)).astype(np.uint8)


def prepare_mask(mask, S: int, cell: int = 8) -> Tuple[np.ndarray, np.ndarray]:
    """mask: a PIL image (or uint8 [H, W] array) of the init image's size -> (pixel mask uint8 [S, S] of 0 / 1, latent mask uint8 [S/cell, S/cell]),
    on the host: convert("L"), the photo's resize with NEAREST and its centre crop, then >= 128 = repaint (white)."""
    from PIL import Image
    im = Image.fromarray(np.asarray(mask, dtype=np.uint8)) if isinstance(mask, np.ndarray) else mask
    im = im.convert("L")
    nw, nh, x1, y1 = edit_geometry(im.width, im.height, S)
    im = im.resize((nw, nh), Image.NEAREST).crop((x1, y1, x1 + S, y1 + S))
    pixel = (np.asarray(im) >= 128).astype(np.uint8)
    return pixel, pool_mask_any(pixel, cell)


def prepare_image(rgb: np.ndarray, S: int):
    """uint8 [H, W, 3] -> (resident RGBX int32 [S, S]: the prepared photo, kept for the paste; pixel_values fp32 [1, 3, S, S] in [-1, 1])"""
    import torch
    from . import augment, ops
    img = augment.resize_short_edge(augment.to_device_image(rgb), S, augment.LANCZOS)
    nw, nh, x1, y1 = edit_geometry(rgb.shape[1], rgb.shape[0], S)
    assert tuple(img.shape) == (nh, nw)
    pixels = torch.empty(1, 3, S, S, dtype=torch.float32, device=img.device)
    ops.img_to_pixels(img, x1, y1, pixels[0])
    return img[y1:y1 + S, x1:x1 + S].contiguous(), pixels


def check_vae_has_encoder(model_dir: str, keys=None):
    """FileNotFoundError / ValueError unless <model_dir>/vae/diffusion_pytorch_model.safetensors holds the encoder half.  Reads the file's
    header only (no tensor)."""
    path = os.path.join(model_dir, VAE_FILE)
    if keys is None:
        if not os.path.exists(path):
            raise FileNotFoundError(f"{path} is missing: --model must be a local diffusers model directory")
        from safetensors import safe_open
        with safe_open(path, framework="pt") as f:
            keys = list(f.keys())
    if not any(k.startswith("encoder.") for k in keys) or not any(k.startswith("quant_conv.") for k in keys):
        raise ValueError(f"{path} holds no encoder.* / quant_conv.* tensors (a decoder-only VAE file): --init-image encodes the photo with the "
                         "VAE encoder, so the model directory must ship the whole AutoencoderKL")


class EditEncoder:
    """the VAE encoder of --init-image: `HipVAEEncoder` at batch 1 for size x size latents, built only when a photo is given"""

    def __init__(self, model_dir: str, size: int, device="cuda"):
        import json
        from safetensors.torch import load_file
        from .vae import HipVAEEncoder, vae_encoder_shapes, vae_geometry_from_config
        check_vae_has_encoder(model_dir)
        with open(os.path.join(model_dir, "vae", "config.json")) as f:
            geo = vae_geometry_from_config(json.load(f))
        sd = load_file(os.path.join(model_dir, VAE_FILE))
        missing = [k for k in vae_encoder_shapes(geo) if k not in sd]
        if missing:
            raise ValueError(f"{os.path.join(model_dir, VAE_FILE)}: encoder tensors are missing: {missing[:4]}{' ...' if len(missing) > 4 else ''}")
        self.S = size << (len(geo.block_out_channels) - 1)       # pixels per edge
        self.size, self.geo, self.dev = size, geo, device
        self.enc = HipVAEEncoder(geo, {k: v for k, v in sd.items() if k.startswith(("encoder.", "quant_conv."))}, 1, self.S, self.S, device=device)

    def encode(self, pixel_values):
        """fp32 [1, 3, S, S] in [-1, 1] -> z0 fp32 [1, 4, size, size] = mean * scaling_factor (noise zero: the mode), a copy the caller owns"""
        import torch
        L4 = self.geo.latent_channels
        zero = torch.zeros(1, L4, self.size, self.size, device=self.dev, dtype=torch.float32)
        return self.enc.encode(pixel_values, noise=zero).clone()
