"""FreeU restated in float64: diffusers' `fourier_filter` in its `torch.fft` form and in the closed form the kernel
computes, the two backbone modes, the oracle UNet's pre-hooks, and the error bound of csrc/freeu.hip derived from its arithmetic.  Shared by
tests/test_freeu_host.py and tests/test_gpu_freeu.py; nothing here touches a device."""
import math

import numpy as np
import torch

# (B, H, W, hc, sc): the kernel cases of tests/test_gpu_freeu.py; the host test holds the two filter forms together on every (H, W) of them
SHAPES = [(2, 8, 8, 64, 64),
          (1, 5, 7, 24, 40),        # odd, non-square, hc / 2 = 12 and sc = 40 off a 64-lane slab
          (3, 2, 2, 16, 8),         # the whole spectrum is scaled
          (2, 1, 1, 8, 8), (1, 1, 4, 8, 8),
          (1, 16, 16, 1280, 640),   # the real stage-1 row
          (1, 24, 24, 32, 32)]      # a 768-pixel model's stage-1 map
MODES = ("scalar", "structure")
B_S = (1.5, 0.2)                    # (b, s) of the kernel cases; the reference takes `f32` of them, the values the C entry point is given


def f32(v):
    """the value a float argument of the C entry point carries"""
    return float(np.float32(v))


# ------------------------------------------------------------------------------------------------------------------ the skip filter
def fourier_filter_fft(x, scale, threshold=1):
    """diffusers.utils.torch_utils.fourier_filter on x float64 [B, C, H, W]"""
    B, C, H, W = x.shape
    xf = torch.fft.fftshift(torch.fft.fftn(x, dim=(-2, -1)), dim=(-2, -1))
    mask = torch.ones((B, C, H, W), dtype=x.dtype)
    crow, ccol = H // 2, W // 2
    mask[..., crow - threshold:crow + threshold, ccol - threshold:ccol + threshold] = scale
    xf = xf * mask
    return torch.fft.ifftn(torch.fft.ifftshift(xf, dim=(-2, -1)), dim=(-2, -1)).real


def freqs(n):
    """the scaled frequencies of an axis of length n: {0, -1}; 0 only where n = 1 (with n = 2 that is the whole axis)"""
    return [0] if n == 1 else [0, -1]


def fourier_filter_closed(x, scale):
    """y = x + (s - 1) / (H W) sum_{(u, v)} (C_uv cos t_uv + S_uv sin t_uv) on x float64 [B, C, H, W]"""
    H, W = x.shape[-2:]
    h = torch.arange(H, dtype=torch.float64)[:, None]
    w = torch.arange(W, dtype=torch.float64)[None, :]
    y = x.clone()
    for u in freqs(H):
        for v in freqs(W):
            th = 2.0 * math.pi * (u * h / H + v * w / W)
            c, s = torch.cos(th), torch.sin(th)
            Cm = (x * c).sum((-2, -1), keepdim=True)
            Sm = (x * s).sum((-2, -1), keepdim=True)
            y = y + (scale - 1.0) / (H * W) * (Cm * c + Sm * s)
    return y


# ------------------------------------------------------------------------------------------------------------------ the backbone
def structure_map(hidden):
    """n float64 [B, 1, H, W]: the channel mean of hidden [B, C, H, W], min-max normalised per image; 0 where the image's map is constant"""
    m = hidden.mean(1, keepdim=True)
    lo = m.amin((-2, -1), keepdim=True)
    hi = m.amax((-2, -1), keepdim=True)
    rng = hi - lo
    return torch.where(rng > 0, (m - lo) / torch.where(rng > 0, rng, torch.ones_like(rng)), torch.zeros_like(m))


def backbone(hidden, b, mode):
    out = hidden.clone()
    half = hidden.shape[1] // 2
    f = b if mode == "scalar" else (b - 1.0) * structure_map(hidden) + 1.0
    out[:, :half] = hidden[:, :half] * f
    return out


def apply_freeu(x, skip_ch, b, s, mode, filt=fourier_filter_closed):
    """FreeU on a concat input x float64 [B, hc + sc, H, W] (hidden first)"""
    hc = x.shape[1] - skip_ch
    return torch.cat([backbone(x[:, :hc], b, mode), filt(x[:, hc:], s)], dim=1)


def install_hooks(unet, b1, b2, s1, s2, mode="scalar"):
    """FreeU on the oracle UNet: a forward pre-hook on every resnet of up_blocks 0 and 1 (the stage is the block's index, as in diffusers'
    `apply_freeu`).  The hook sees the concatenated input and splits it at x.shape[1] - skip_ch.  -> the handles (call .remove())"""
    cfg = unet.cfg
    ch = cfg.block_out_channels
    skip_chs = [ch[0]]
    for i, c in enumerate(ch):
        skip_chs += [c] * cfg.layers_per_block + ([] if i == len(ch) - 1 else [c])
    handles = []
    for i, (b, s) in enumerate(((b1, s1), (b2, s2))):
        for j, res in enumerate(unet.up_blocks[i].resnets):
            sc = skip_chs[len(skip_chs) - 1 - (i * (cfg.layers_per_block + 1) + j)]

            def hook(mod, args, sc=sc, b=b, s=s):
                x = args[0]
                return (apply_freeu(x.double(), sc, b, s, mode).to(x.dtype),) + tuple(args[1:])
            handles.append(res.register_forward_pre_hook(hook))
    return handles


# ------------------------------------------------------------------------------------------------------------------ kernel operands, bound
def rows_to_nchw(rows, B, H, W):
    return rows.view(B, H, W, -1).permute(0, 3, 1, 2)


def nchw_to_rows(x):
    B, C, H, W = x.shape
    return x.permute(0, 2, 3, 1).reshape(B * H * W, C)


def reference_rows(rows, B, H, W, hc, b, s, mode):
    """the float64 result on the kernel's layout: rows float64 [B H W, hc + sc] -> the same shape"""
    x = rows_to_nchw(rows, B, H, W)
    return nchw_to_rows(apply_freeu(x, x.shape[1] - hc, b, s, mode))


U32 = 2.0 ** -24
K_FILTER = 64     # see bound_rows
K_MEAN = 8


def gamma(n):
    return n * U32 / (1.0 - n * U32)


def bound_rows(rows, ref, B, H, W, hc, b, s, mode, half):
    """|kernel - float64| allowed per element, from the kernel's arithmetic (rows: the rounded operands in float64, ref: reference_rows).

    Every output is one fp32 value e-close to the true one, rounded once to 16 bits: e (1 + u) + u |y| + the subnormal floor, u = 2^-11
    (fp16) or 2^-8 (bf16).
    skip:  the correction (s - 1) / (H W) sum over the |S| frequencies of (C cos t + S sin t) has, per frequency, the error gamma_n sum|x|
           of a length-(H W) sum of products whose factors |cos t cos t'| + |sin t sin t'| <= 1, so e = |s - 1| |S| / (H W) gamma_(HW + k) sum|x|
           + 2 u32 |y| (the final multiply-add).  k = 64 counts what touches a term besides the H W additions: a table twiddle is
           sincospif of a once-rounded quotient (<= 8 u32 absolute), the diagonal twiddle two products and a sum of those (<= 20 u32), used once
           in the moment and once in the correction (40), two products (2), the 3 partial-sum additions of the four waves, the 7-term sum
           and its weights (10), g = (s - 1) / (H W) rounded once and its product (2): 57 <= 64.
    scalar backbone:  e = u32 |y| (one fp32 product).
    structure backbone:  a pixel's mean carries D_p = gamma_(hc + 8) mean|x_p| (hc additions, the division); with D the largest D_p of the
           image and R = max m - min m, n = (m - lo) / (hi - lo) is off by at most 4 D / (R - 2 D) + 4 u32, the factor f = (b - 1) n + 1
           by |b - 1| times that + 2 u32 |f|, so e = |x| (|b - 1| dn + 3 u32 |f|).  R = 0 (one pixel, or a constant map whose pixels are
           summed identically): n = 0 exactly, e = 0."""
    u = 2.0 ** -11 if half == "fp16" else 2.0 ** -8
    floor = 2.0 ** -25 if half == "fp16" else 2.0 ** -134
    sc = rows.shape[1] - hc
    HW = H * W
    e = torch.zeros_like(rows)
    x = rows_to_nchw(rows, B, H, W)
    y = rows_to_nchw(ref, B, H, W)
    if s != 1.0:
        nS = len(freqs(H)) * len(freqs(W))
        sabs = x[:, hc:].abs().sum((-2, -1), keepdim=True)
        ef = abs(s - 1.0) * nS / HW * gamma(HW + K_FILTER) * sabs + 2 * U32 * y[:, hc:].abs()
        e = rows_to_nchw(e, B, H, W)
        e[:, hc:] = ef
        e = nchw_to_rows(e)
    if b != 1.0:
        en = rows_to_nchw(e, B, H, W).clone()
        if mode == "scalar":
            en[:, :hc // 2] = U32 * y[:, :hc // 2].abs()
        else:
            hid = x[:, :hc]
            D = (gamma(hc + K_MEAN) * hid.abs().mean(1, keepdim=True)).amax((-2, -1), keepdim=True)
            m = hid.mean(1, keepdim=True)
            R = m.amax((-2, -1), keepdim=True) - m.amin((-2, -1), keepdim=True)
            assert bool(((R == 0) | (R > 4 * D)).all()), "the test data leave the normalised map undetermined in fp32"
            dn = torch.where(R > 0, 4 * D / (R - 2 * D).clamp_min(1e-300) + 4 * U32, torch.zeros_like(R))
            f = (b - 1.0) * structure_map(hid) + 1.0
            en[:, :hc // 2] = hid[:, :hc // 2].abs() * (abs(b - 1.0) * dn + 3 * U32 * f.abs()) * (R > 0)
        e = nchw_to_rows(en)
    return e * (1 + u) + u * ref.abs() + floor


def kernel_rows(B, H, W, hc, sc, offset, seed, dtype):
    """N(0, 1) + offset operands, rounded to `dtype`: -> (rounded rows in `dtype`, the same in float64)"""
    g = torch.Generator().manual_seed(seed)
    r = (torch.randn(B * H * W, hc + sc, generator=g) + offset).to(dtype)
    return r, r.double()
