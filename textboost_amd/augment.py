"""Device-side image augmentation + tokenised-prompt feeder.

Host mirror of the reference's data path for the instance images, with the same names, arguments, random-draw order and prompt edits:

    textboost/augment/paired_augmentation.py:20-351   adjust_scale, crop, horizontal_translate, horizontal_flip, grayscale,
                                                      square_photo_collage, PairedAugmentation
    textboost/dataset.py:324-381, :420-457            Resize(size, LANCZOS) -> Center/RandomCrop -> ToImage/ToDtype/Normalize, the template
                                                      draw, tokenize_prompt, collate_fn's {"input_ids", "pixel_values"}

The reference does this per sample in Pillow on DataLoader workers (8 x 512^2 Lanczos resizes per step at batch 8); here the few instance images
of a DreamBooth run are decoded once, stay resident in HBM as RGBX u8, and every op is a HIP kernel of csrc/image.hip that is bit-exact with
Pillow.  The host only draws the random parameters (np.random / random / torch, in the reference's order, so equal seeds give equal samples)
and builds O(W + H) index / coefficient tables.  There is no CPU fallback: a missing library raises.

An image is an int32 CUDA tensor [H, W] (one RGBX pixel per element).

A subject mask (--instance_mask_dir) is such an image with R = G = B = the mask byte (`to_device_mask`): it rides
through the same kernels as the image's `companion`, with the image's drawn parameters, and draws nothing itself.
"""
from __future__ import annotations

import collections
import math
import random
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from . import ops

NEAREST, LANCZOS, BILINEAR, BICUBIC = 0, L.IMG_LANCZOS, L.IMG_BILINEAR, L.IMG_BICUBIC

# resample tables per (in, out, filter, device): an LRU, because `crop` draws a new source size for almost every sample
_coeff_cache: "collections.OrderedDict[tuple, tuple]" = collections.OrderedDict()
_COEFF_CACHE_MAX = 1024


def clear_caches():
    """drop the resident resample tables (they are rebuilt, with the same values, when a size comes up again)"""
    _coeff_cache.clear()


def _dev_table(a: np.ndarray, device) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(device)


def to_device_image(rgb) -> torch.Tensor:
    """uint8 [H, W, 3] (numpy / CPU or CUDA tensor; e.g. `np.asarray(PIL.Image.open(p).convert("RGB"))`) -> resident RGBX image."""
    t = torch.from_numpy(np.array(rgb, copy=True)) if isinstance(rgb, np.ndarray) else torch.as_tensor(rgb)
    if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3:
        raise ValueError("expected a uint8 [H, W, 3] RGB image")
    return ops.img_pack_rgb(t.cuda().contiguous())


def to_device_mask(mask) -> torch.Tensor:
    """uint8 [H, W] (Pillow "L": white = subject) -> resident grey RGBX image (R = G = B = mask byte), the form in which a mask rides through
    the image kernels unchanged: they zero X and treat R, G and B alike."""
    t = torch.from_numpy(np.array(mask, copy=True)) if isinstance(mask, np.ndarray) else torch.as_tensor(mask)
    if t.dtype != torch.uint8 or t.dim() != 2:
        raise ValueError("expected a uint8 [H, W] mask")
    return ops.img_pack_rgb(t.cuda()[:, :, None].expand(-1, -1, 3).contiguous())


def to_host_rgb(img: torch.Tensor) -> np.ndarray:
    return ops.img_unpack_rgb(img).cpu().numpy()


def resize(img: torch.Tensor, size_wh: Tuple[int, int], filt: int) -> torch.Tensor:
    """`PIL.Image.resize((w, h), resample)`: horizontal pass then vertical pass; a pass whose size does not change is skipped."""
    w, h = int(size_wh[0]), int(size_wh[1])
    H, W = img.shape
    out = img
    for vertical, n_in, n_out in ((0, W, w), (1, H, h)):
        if n_in == n_out:
            continue
        key = (n_in, n_out, filt, img.device)
        if key not in _coeff_cache:
            _, bounds, kk = ops.resample_coeffs(n_in, n_out, filt)
            _coeff_cache[key] = (bounds.to(img.device), kk.to(img.device), ops.resample_fit24(kk))
            if len(_coeff_cache) > _COEFF_CACHE_MAX:
                _coeff_cache.popitem(last=False)
        else:
            _coeff_cache.move_to_end(key)
        bounds, kk, fit24 = _coeff_cache[key]
        out = ops.img_resample(out, n_out, bounds, kk, vertical, fit24)
    return out.clone() if out is img else out


def _gather(img, xt: np.ndarray, yt: np.ndarray, gray=False):
    return ops.img_gather(img, _dev_table(xt, img.device), _dev_table(yt, img.device), gray)


def _gather_pair(img, companion, xt: np.ndarray, yt: np.ndarray):
    """`_gather` on the image and, through the same device tables, on its companion (the subject mask of --instance_mask_dir: a grey RGBX image
    of the image's shape that every geometric op replays with the image's drawn parameters).  companion None: exactly `_gather`."""
    if companion is None:
        return _gather(img, xt, yt), None
    dx, dy = _dev_table(xt, img.device), _dev_table(yt, img.device)
    return ops.img_gather(img, dx, dy, False), ops.img_gather(companion, dx, dy, False)


def _ret(image, prompt, companion):
    """the ops return (image, prompt), and (image, prompt, companion) when they were handed a companion"""
    return (image, prompt) if companion is None else (image, prompt, companion)


def _center_crop_offsets(W: int, H: int, crop_h: int, crop_w: int):
    """torchvision `center_crop(image, (crop_h, crop_w))` on a W x H image: output pixel (x, y) is source pixel (x + ox, y + oy), zero where
    that falls outside (the zero padding it applies first when the image is smaller than the crop)."""
    pl = (crop_w - W) // 2 if crop_w > W else 0
    pt = (crop_h - H) // 2 if crop_h > H else 0
    pr = (crop_w - W + 1) // 2 if crop_w > W else 0
    pb = (crop_h - H + 1) // 2 if crop_h > H else 0
    left = int(round((W + pl + pr - crop_w) / 2.0))
    top = int(round((H + pt + pb - crop_h) / 2.0))
    return left - pl, top - pt


def _center_crop_tables(W: int, H: int, crop_h: int, crop_w: int):
    ox, oy = _center_crop_offsets(W, H, crop_h, crop_w)
    xs, ys = np.arange(crop_w) + ox, np.arange(crop_h) + oy
    return np.where((xs >= 0) & (xs < W), xs, -1), np.where((ys >= 0) & (ys < H), ys, -1)


def inverse_affine_matrix(center, angle, translate, scale, shear):
    """torchvision `_get_inverse_affine_matrix` (what `v2.functional.affine` hands to `PIL.Image.transform`)."""
    rot = math.radians(angle)
    sx, sy = math.radians(shear[0]), math.radians(shear[1])
    cx, cy = center
    tx, ty = translate
    a = math.cos(rot - sy) / math.cos(sy)
    b = -math.cos(rot - sy) * math.tan(sx) / math.cos(sy) - math.sin(rot)
    c = math.sin(rot - sy) / math.cos(sy)
    d = -math.sin(rot - sy) * math.tan(sx) / math.cos(sy) + math.cos(rot)
    m = [v / scale for v in [d, -b, 0.0, -c, a, 0.0]]
    m[2] += m[0] * (-cx - tx) + m[1] * (-cy - ty)
    m[5] += m[3] * (-cx - tx) + m[4] * (-cy - ty)
    m[2] += cx
    m[5] += cy
    return m


# ------------------------------------------------------------------------------------ the reference's ops, draw order kept
def _compute_padding(h, w, scale):
    return round(((h / scale) - h) / 2), round(((w / scale) - w) / 2)


def adjust_scale(image, prompt, inversion=False, companion=None):
    """paired_augmentation.py:20-49 -- pad(edge) + affine(scale, BICUBIC) + center_crop in ONE launch."""
    scale_factor = np.random.uniform(0.34, 1.4)
    H, W = image.shape
    h, w = W, H  # the reference unpacks PIL's (width, height) as `h, w`
    pad_h, pad_w = _compute_padding(h, w, scale_factor)
    px, py = (pad_w, pad_h) if (pad_h > 0 and pad_w > 0) else (0, 0)  # v2.functional.pad(image, (pad_w, pad_h)): left/right, top/bottom
    PW, PH = W + 2 * px, H + 2 * py
    m = inverse_affine_matrix([PW * 0.5, PH * 0.5], 0.0, [0.0, 0.0], scale_factor, [0.0, 0.0])
    crop_h, crop_w = h, w  # center_crop(image, (h, w))
    ox, oy = _center_crop_offsets(PW, PH, crop_h, crop_w)
    image = ops.img_affine_bicubic(image, m, px, py, ox, oy, crop_w, crop_h)
    if companion is not None:
        companion = ops.img_affine_bicubic(companion, m, px, py, ox, oy, crop_w, crop_h)
    if inversion:
        add = "<zoom-out_0> <zoom-out_1>" if scale_factor < 0.6 else "<zoom-in_0> <zoom-in_1>" if scale_factor > 1.2 else ""
    else:
        if scale_factor <= 0.6:
            add = np.random.choice(["a far away ", "very small "])
        elif scale_factor >= 1.2:
            add = np.random.choice(["zoomed in ", "close up "])
        else:
            add = ""
    return _ret(image, add + prompt, companion)


def horizontal_flip(image, prompt, inversion=False, companion=None):
    """paired_augmentation.py:79-92."""
    H, W = image.shape
    image, companion = _gather_pair(image, companion, np.arange(W - 1, -1, -1), np.arange(H))
    word = "<hflip>" if inversion else "horizontally flipped"
    if np.random.rand() < 0.5:
        prompt = word + " " + prompt
    else:
        prompt = prompt + ", " + word
    return _ret(image, prompt, companion)


def horizontal_translate(image, prompt, inversion=False, companion=None):
    """paired_augmentation.py:95-134 -- pad(edge) + affine(translate, NEAREST) + center_crop composed into one index map, one launch."""
    shift_dir = np.random.randint(0, 2)
    H, W = image.shape
    w, h = W, H
    shift_str = np.random.uniform(low=0.15, high=0.3)
    shift = int(shift_str * w)
    trans = [-shift, 0] if shift_dir == 0 else [shift, 0]
    if inversion:
        add = " <left_0> <left_1> <left_2>" if shift_dir == 0 else " <right_0> <right_0> <right_0>"
    else:
        add = " on the left" if shift_dir == 0 else " on the right"
    prompt = prompt + add
    PW = W + 2 * shift
    pad_x = np.clip(np.arange(-shift, W + shift), 0, W - 1)  # padded column -> source column
    m = inverse_affine_matrix([PW * 0.5, H * 0.5], 0.0, [float(trans[0]), float(trans[1])], 1, [0.0, 0.0])
    ax, ay = ops.affine_nearest_tables(m, PW, H, PW, H)
    ax, ay = ax.numpy(), ay.numpy()
    cx, cy = _center_crop_tables(PW, H, w, h)  # center_crop(image, [w, h]): crop_h = w, crop_w = h
    fx = np.where(cx >= 0, ax[np.maximum(cx, 0)], -1)
    fy = np.where(cy >= 0, ay[np.maximum(cy, 0)], -1)
    fx = np.where(fx >= 0, pad_x[np.maximum(fx, 0)], -1)
    image, companion = _gather_pair(image, companion, fx, fy)
    return _ret(image, prompt, companion)


def grayscale(image, prompt, inversion=False, size=None, companion=None):
    """paired_augmentation.py:163-174.  A companion mask passes through untouched: the luma of a grey pixel is the pixel itself
    (19595 + 38470 + 7471 = 65536), so skipping the launch changes no byte."""
    H, W = image.shape
    image = _gather(image, np.arange(W), np.arange(H), gray=True)
    return _ret(image, f"{prompt}, " + ("<grayscale_0> <grayscale_1>" if inversion else "grayscale"), companion)


def random_resized_crop(image, target_size, scale=(0.08, 1.0), ratio=(3. / 4., 4. / 3.), companion=None):
    """paired_augmentation.py:177-217 (`random` module draws); the crop is a strided view, only the BICUBIC resize touches memory."""
    height, width = image.shape
    area = width * height * random.uniform(*scale)
    aspect_ratio = random.uniform(*ratio)
    new_width = min(int(round(math.sqrt(area * aspect_ratio))), width)
    new_height = min(int(round(math.sqrt(area / aspect_ratio))), height)
    x = random.randint(0, width - new_width)
    y = random.randint(0, height - new_height)
    out = resize(image[y:y + new_height, x:x + new_width], target_size, BICUBIC)
    if companion is None:
        return out
    return out, resize(companion[y:y + new_height, x:x + new_width], target_size, BICUBIC)


def crop(image, prompt, inversion=False, companion=None):
    """paired_augmentation.py:220-233."""
    H, W = image.shape
    if companion is None:
        image = random_resized_crop(image, (W, H), ratio=(1.0, 1.0))
    else:
        image, companion = random_resized_crop(image, (W, H), ratio=(1.0, 1.0), companion=companion)
    add = "<crop>" if inversion else "cropped"
    if np.random.random() < 0.5:
        prompt = f"{add} {prompt}"
    else:
        prompt = f"{prompt}, {add}"
    return _ret(image, prompt, companion)


def square_photo_collage(image, prompt, inversion=False, companion=None):
    """paired_augmentation.py:253-277: BICUBIC resize to one cell, black 1-pixel frame, axis x axis tiling (frame + tiling = one index map)."""
    axis = np.random.randint(2, 4)
    H, W = image.shape
    grid_w, grid_h = W // axis, H // axis
    small = resize(image, (grid_h, grid_w), BICUBIC)  # PIL size (width = grid_h, height = grid_w)
    sh, sw = small.shape
    xs, ys = np.arange(sw), np.arange(sh)
    xs[[0, -1]] = -1
    ys[[0, -1]] = -1
    small_c = None if companion is None else resize(companion, (grid_h, grid_w), BICUBIC)
    image, companion = _gather_pair(small, small_c, np.tile(xs, axis), np.tile(ys, axis))
    prompt = ("<collage_0> <collage_1> " if inversion else "photo collage of ") + prompt
    return _ret(image, prompt, companion)


class PairedAugmentation:
    """paired_augmentation.py:280-351: same constructor, same gates and op choice (np.random), returns (image, prompt, mask).

    `mask` (optional) is a resident grey RGBX image of the image's shape: the subject mask of --instance_mask_dir.  It goes through the same
    geometric ops, collage and hflip as the image, with the image's drawn parameters and the same kernels; the colour op skips it (the
    identity on grey).  It draws nothing: a call with a mask consumes the same np.random / random / torch sequence as one without."""

    def __init__(self, hflip="false", inversion=False, p=0.5, color_prob=0.2, augment_prompt=True, ops="object"):
        assert hflip.lower() in ("true", "false", "inversion"), f"Invalid hflip value: {hflip}"
        self.hflip = False
        self.inversion = inversion
        self.p = p
        self.color_prob = color_prob
        self.augment_prompt = augment_prompt
        if ops == "object":
            self.geometric_ops = [adjust_scale, crop, horizontal_translate]
            self.color_ops = [grayscale]
            self.other_ops = [square_photo_collage]
        else:  # "style"
            self.geometric_ops = []
            self.color_ops = [grayscale]
            self.other_ops = []
        if hflip == "inversion":
            self.geometric_ops.append(horizontal_flip)
        elif hflip == "true":
            self.hflip = True

    def __call__(self, image, prompt, mask=None):
        if not (isinstance(image, torch.Tensor) and image.is_cuda and image.dtype == torch.int32 and image.dim() == 2):
            raise TypeError("PairedAugmentation takes a resident RGBX image (int32 CUDA tensor [H, W]); see to_device_image()")
        if mask is not None and not (isinstance(mask, torch.Tensor) and mask.device == image.device and mask.dtype == torch.int32
                                     and mask.shape == image.shape):
            raise TypeError("the mask is a resident grey RGBX image of the image's shape; see to_device_mask()")
        if self.hflip and np.random.rand() < 0.5:
            H, W = image.shape
            image, mask = _gather_pair(image, mask, np.arange(W - 1, -1, -1), np.arange(H))
        for op_list, prob in ((self.geometric_ops, self.p), (self.other_ops, self.p), (self.color_ops, self.color_prob)):
            if len(op_list) > 0 and np.random.rand() < prob:
                op = np.random.choice(op_list)
                if mask is None:
                    image, new_prompt = op(image, prompt, self.inversion)
                else:
                    image, new_prompt, mask = op(image, prompt, self.inversion, companion=mask)
                if self.augment_prompt:
                    prompt = new_prompt
        return image, prompt, mask


# ------------------------------------------------------------------------------------------------------------------ the feeder
def resize_short_edge(image, size: int, filt=LANCZOS):
    """`v2.Resize(size, interpolation=LANCZOS)` with an int size (dataset.py:324)."""
    H, W = image.shape
    short, long = (W, H) if W <= H else (H, W)
    new_long = int(size * long / short)
    nw, nh = (size, new_long) if W <= H else (new_long, size)
    return resize(image, (nw, nh), filt)


class PromptFeeder:
    """`tokenize_prompt` (dataset.py:79-93) behind a cache: the prompt space of a run is the templates x the augmentation captions, so after a few
    steps every prompt is a dictionary hit and the tokenizer leaves the step."""

    def __init__(self, tokenizer, max_length: Optional[int] = None):
        self.tokenizer = tokenizer
        self.max_length = max_length
        self.cache: Dict[str, torch.Tensor] = {}
        self.hits = 0

    def __call__(self, prompt: str) -> torch.Tensor:
        ids = self.cache.get(prompt)
        if ids is None:
            max_length = self.max_length if self.max_length is not None else self.tokenizer.model_max_length
            out = self.tokenizer(prompt, truncation=True, padding="max_length", max_length=max_length, return_tensors="pt")
            ids = self.cache[prompt] = out.input_ids
        else:
            self.hits += 1
        return ids


class DeviceFeeder:
    """`TextBoostDataset.__getitem__` + `collate_fn` (dataset.py:353-381, :420-457) for the instance images, on the device.

    images: list of (resident RGBX image, instance_token) or (image, instance_token, mask), mask a resident grey RGBX image of the image's
    shape (`to_device_mask`) or None.  `batch(indices)` returns {"input_ids": int64 [B, 77] (CPU, as the reference's collate_fn),
    "pixel_values": fp32 [B, 3, size, size] on the device, "prompts": list[str]} and, when any image carries a mask, "loss_weight": fp32
    [B, 1, size / 8, size / 8]: the mask after the image's augmentation, Lanczos resize and crop, box-averaged over the VAE's 8 x 8 cells,
    w = mask_floor + (1 - mask_floor) * mean / 255.  An image without a mask in such a run gets an all-white one (it trains unmasked).  The
    mask draws nothing: pixel_values, prompts and the random streams are those of the same feeder without masks.  attn_target = True (the
    localisation loss) adds "attn_target": the same pooling of the same crop with floor 0 -- the very tensor of
    "loss_weight" when mask_floor is 0."""

    LATENT_CELL = 8   # pixels per latent cell of every supported VAE

    def __init__(self, images: Sequence[tuple], tokenizer, templates: Sequence[str], size=512, center_crop=False,
                 augment_pipe: Optional[PairedAugmentation] = None, mask_floor: float = 0.0, attn_target: bool = False):
        if len(images) == 0:
            raise ValueError("no instance images")
        if not 0.0 <= mask_floor < 1.0:
            raise ValueError(f"mask_floor {mask_floor}: 0 <= F < 1")
        items = [tuple(it) + (None,) * (3 - len(it)) for it in images]
        self.has_mask = any(m is not None for _, _, m in items)
        if self.has_mask:
            if size % self.LATENT_CELL:
                raise ValueError(f"the masked loss needs a resolution that is a multiple of {self.LATENT_CELL}, not {size}")
            items = [(im, tok, m if m is not None else torch.full_like(im, 0x00FFFFFF)) for im, tok, m in items]
            for im, _, m in items:
                if m.shape != im.shape or m.dtype != torch.int32 or m.device != im.device:
                    raise ValueError("a mask is a resident grey RGBX image of its image's shape (to_device_mask)")
        self.images = [(im, tok) for im, tok, _ in items]
        self.masks = [m for _, _, m in items] if self.has_mask else None
        self.mask_floor = float(mask_floor)
        if attn_target and not self.has_mask:
            raise ValueError("attn_target needs masks: no image of this feeder carries one")
        self.attn_target = bool(attn_target)
        self.templates = list(templates)
        self.size = size
        self.center_crop = center_crop
        self.augment_pipe = augment_pipe
        self.tokenize = PromptFeeder(tokenizer)

    def __len__(self):
        return len(self.images)

    def item_into(self, index: int, dst: torch.Tensor, weight_dst: Optional[torch.Tensor] = None, target_dst: Optional[torch.Tensor] = None):
        """One sample; pixel_values written into dst [3, size, size] and, with masks, the loss weights into weight_dst [1, size/8, size/8] (and
        their floor-0 form into target_dst when given).  Returns (input_ids [1, 77], prompt)."""
        image, instance_token = self.images[index % len(self.images)]
        mask = self.masks[index % len(self.images)] if self.has_mask else None
        if self.has_mask and weight_dst is None:
            raise ValueError("this feeder carries masks: item_into needs weight_dst")
        prompt_idx = random.randint(0, len(self.templates) - 1)
        prompt = self.templates[prompt_idx].format(instance_token)
        if self.augment_pipe is not None:
            image, prompt, mask = self.augment_pipe(image, prompt, mask)
        image = resize_short_edge(image, self.size, LANCZOS)
        if mask is not None:
            mask = resize_short_edge(mask, self.size, LANCZOS)
        H, W = image.shape
        if self.center_crop:
            y1 = max(0, int(round((H - self.size) / 2.0)))
            x1 = max(0, int(round((W - self.size) / 2.0)))
        elif W == self.size and H == self.size:
            y1, x1 = 0, 0
        else:  # v2.RandomCrop.get_params: two torch.randint draws from the global generator
            y1 = int(torch.randint(0, H - self.size + 1, size=(1,)).item())
            x1 = int(torch.randint(0, W - self.size + 1, size=(1,)).item())
        ops.img_to_pixels(image, x1, y1, dst)
        if mask is not None:
            ops.img_to_loss_weight(mask, x1, y1, weight_dst, cell=self.LATENT_CELL, floor=self.mask_floor)
            if target_dst is not None:
                ops.img_to_loss_weight(mask, x1, y1, target_dst, cell=self.LATENT_CELL, floor=0.0)
        return self.tokenize(prompt), prompt

    def batch(self, indices: Sequence[int], out: Optional[torch.Tensor] = None, weight_out: Optional[torch.Tensor] = None,
              target_out: Optional[torch.Tensor] = None):
        B = len(indices)
        dev = self.images[0][0].device
        if out is None:
            out = torch.empty(B, 3, self.size, self.size, dtype=torch.float32, device=dev)
        if self.has_mask and weight_out is None:
            weight_out = torch.empty(B, 1, self.size // self.LATENT_CELL, self.size // self.LATENT_CELL, dtype=torch.float32, device=dev)
        second = self.attn_target and self.mask_floor != 0.0   # (floor 0: the target IS the weights)
        if second and target_out is None:
            target_out = torch.empty_like(weight_out)
        ids, prompts = [], []
        for b, i in enumerate(indices):
            t, p = self.item_into(i, out[b], weight_out[b] if self.has_mask else None, target_out[b] if second else None)
            ids.append(t)
            prompts.append(p)
        res = {"input_ids": torch.cat(ids, dim=0), "pixel_values": out, "prompts": prompts}
        if self.has_mask:
            res["loss_weight"] = weight_out
        if self.attn_target:
            res["attn_target"] = target_out if second else weight_out
        return res


class PrefetchFeeder:
    """Overlaps the feeder with the training step.  `DeviceFeeder.batch` is host-bound (random draws, O(W + H) table uploads, a handful of
    launches per sample: ~0.3 ms / sample with augmentation) and its uploads are stream-ordered, so on the step's stream the host would sit
    behind the running step.  Here batch k+1 is produced on a side stream into a staging buffer while step k runs; `commit()` makes the step's
    stream wait for it and copies pixels / ids into the step's static inputs (one device-to-device copy)."""

    def __init__(self, feeder: DeviceFeeder, batch: int, pixel_values: torch.Tensor, input_ids: torch.Tensor,
                 loss_weight: Optional[torch.Tensor] = None, attn_target: Optional[torch.Tensor] = None):
        self.feeder, self.batch = feeder, batch
        self.pixel_values, self.input_ids = pixel_values, input_ids
        if (loss_weight is not None) != bool(getattr(feeder, "has_mask", False)):
            raise ValueError("a feeder with masks needs the step's loss_weight input, and one without must not be given it")
        self.loss_weight = loss_weight   # the masked loss's static input (TextBoostStep.enable_loss_weight), staged beside the pixels
        self.weight_staging = torch.empty_like(loss_weight) if loss_weight is not None else None
        if (attn_target is not None) != bool(getattr(feeder, "attn_target", False)):
            raise ValueError("a feeder with attn_target needs the step's attn_target input, and one without must not be given it")
        self.attn_target = attn_target   # the localisation loss's static input (TextBoostStep.enable_attn_loss), staged beside the weights
        self.target_staging = torch.empty_like(attn_target) if attn_target is not None and feeder.mask_floor != 0.0 else None
        self.staging = torch.empty_like(pixel_values)
        self.ids_staging = torch.empty_like(input_ids)
        self.side = torch.cuda.Stream(device=pixel_values.device)
        self.ready = torch.cuda.Event()
        self.consumed = None  # recorded on the step's stream right after a commit's copies: the staging buffers are free from there on
        self.pending = None

    def prefetch(self, indices: Sequence[int]):
        if self.consumed is not None:
            self.side.wait_event(self.consumed)  # NOT wait_stream(main): that would put the side stream (and the host's uploads) behind the step
        with torch.cuda.stream(self.side):
            if self.loss_weight is None:   # (the call of a run without masks is what it was)
                b = self.feeder.batch(indices, out=self.staging)
            elif self.target_staging is None:
                b = self.feeder.batch(indices, out=self.staging, weight_out=self.weight_staging)
            else:
                b = self.feeder.batch(indices, out=self.staging, weight_out=self.weight_staging, target_out=self.target_staging)
            self.ids_staging.copy_(b["input_ids"], non_blocking=True)
            self.ready.record(self.side)
        self.pending = b

    def commit(self):
        """-> the prompts of the committed batch."""
        if self.pending is None:
            raise RuntimeError("commit() without a prefetch()")
        torch.cuda.current_stream().wait_event(self.ready)
        self.pixel_values.copy_(self.staging)
        self.input_ids.copy_(self.ids_staging)
        if self.loss_weight is not None:
            self.loss_weight.copy_(self.weight_staging)
        if self.attn_target is not None:
            self.attn_target.copy_(self.target_staging if self.target_staging is not None else self.weight_staging)
        self.consumed = torch.cuda.Event()
        self.consumed.record(torch.cuda.current_stream())
        b, self.pending = self.pending, None
        return b["prompts"]
