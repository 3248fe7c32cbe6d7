"""The LocalBlend mask, restated (csrc/local_blend.hip) -- the reference of tests/test_blend_host.py and tests/test_gpu_blend.py.

n pairs; `acc` fp32 [2n, T, hl * wl] (rows j and n + j are pair j's source and edited conditional rows), `words` int32 [2n, n_pos], -1 padded,
each row's word positions in its own prompt.  Per row r:

    m_r[s]   = sum over the table, in table order, of acc[r][p][s]            fp32 adds; positions outside [0, T) are ignored
    P_r      = 3 x 3 max of m_r, stride 1, windows clipped at the borders
    mx_r     = max_s P_r[s]   (= max m_r)
    bit_r[s] = P_r[s] > fl32(th * mx_r)                                        one rounded fp32 multiply, strict compare; an empty table: all 0

    mask_j[y][x] = (bit_j | bit_{n+j})[y * hl // h][x * wl // w]   [& limit[y][x] != 0]    -> 255 / 0;      area[j] = the set cells

`blend_mask` is that definition in numpy float32, operation for operation: the GPU tests compare BYTES with it.  `blend_mask_literal` is the
published formulation taken literally in float64 torch -- sum, F.max_pool2d(3, 1, 1) on the coarse map, F.interpolate(nearest) to the
latent grid, division by the maximum, .gt(th) -- with the margin |P / mx - th| of every coarse cell, so that the host test can show that
no cell of any case lies within rounding of the threshold (MARGIN: 8 n_pos 2^-24, n_pos - 1 fp32 adds and one multiply, with room)."""
from __future__ import annotations

import numpy as np

# (n, T, hl, wl, h, w) of tests/test_gpu_blend.py; test_blend_host.py runs the same cases
SHAPES = [(2, 77, 16, 16, 64, 64), (1, 77, 4, 4, 16, 16), (3, 20, 5, 7, 20, 28), (1, 2, 2, 2, 2, 2), (1, 77, 1, 3, 4, 3)]
SEEDS = [100, 115, 102, 103, 104]     # chosen on the reference alone: no cell within the margin of the threshold, and no mask of a map of >= 16 cells trivial
CASES = list(zip(SHAPES, SEEDS))
TH = 0.3


def margin(n_pos: int) -> float:
    return 8.0 * n_pos * 2.0 ** -24


def make_case(shape, seed: int, n_pos: int = 16, multi: bool = True):
    """-> (acc fp32 [2n, T, hl wl], words int32 [2n, n_pos]).  The maps look like accumulated attention: non-negative, a few peaked blobs per
    token on a small floor.  Row j's word takes several positions when `multi` (and T allows), the edited row one that the source row has
    not; the table also carries a position outside [0, T), which the definition ignores."""
    n, T, hl, wl, h, w = shape
    rng = np.random.RandomState(seed)
    acc = rng.uniform(0.0, 0.05, size=(2 * n, T, hl * wl)).astype(np.float32)
    ys, xs = np.mgrid[0:hl, 0:wl]
    for r in range(2 * n):
        for t in range(T):
            cy, cx = rng.uniform(0, hl), rng.uniform(0, wl)
            blob = np.exp(-((ys - cy) ** 2 + (xs - cx) ** 2) / (2.0 * (rng.uniform(0.04, 0.12) * max(hl, wl) + 0.3) ** 2))
            acc[r, t] += (1.5 * rng.uniform(0.2, 1.0) ** 2 * blob).reshape(-1).astype(np.float32)
    words = np.full((2 * n, n_pos), -1, dtype=np.int32)
    for r in range(2 * n):
        cand = np.arange(1, T) if T > 2 else np.arange(T)
        pos = rng.choice(cand, size=min(3 if multi else 1, len(cand), n_pos - 1), replace=False)
        words[r, :len(pos)] = pos            # (unsorted: the order of the table is the order of the adds)
        if len(pos) < n_pos:
            words[r, len(pos)] = T + 5       # outside [0, T): ignored
    return acc, words


def row_maps(acc, words, hl: int, wl: int):
    """-> (P fp32 [2n, hl, wl], mx fp32 [2n]): the pooled word-sum maps of the definition and their maxima"""
    n2, T, HW = acc.shape
    assert HW == hl * wl and acc.dtype == np.float32
    P = np.zeros((n2, hl, wl), dtype=np.float32)
    for r in range(n2):
        m = np.zeros(HW, dtype=np.float32)
        for p in words[r]:
            if 0 <= p < T:
                m = (m + acc[r, p]).astype(np.float32)
        m = m.reshape(hl, wl)
        for y in range(hl):
            for x in range(wl):
                P[r, y, x] = m[max(y - 1, 0):y + 2, max(x - 1, 0):x + 2].max()
    return P, P.reshape(n2, -1).max(axis=1)


def blend_mask(acc, words, hl: int, wl: int, h: int, w: int, th: float, limit=None):
    """the definition in float32 -> (mask uint8 [n, h, w] of 0 / 255, area int32 [n])"""
    assert h % hl == 0 and w % wl == 0
    n = acc.shape[0] // 2
    P, mx = row_maps(acc, words, hl, wl)
    thr = (np.float32(th) * mx.astype(np.float32)).astype(np.float32)     # one rounded fp32 multiply
    bit = P > thr[:, None, None]
    both = bit[:n] | bit[n:]
    yy = (np.arange(h) * hl) // h
    xx = (np.arange(w) * wl) // w
    mask = both[:, yy][:, :, xx]
    if limit is not None:
        mask = mask & (np.asarray(limit).reshape(h, w) != 0)[None]
    return (mask * 255).astype(np.uint8), mask.reshape(n, -1).sum(axis=1).astype(np.int32)


def blend_mask_literal(acc, words, hl: int, wl: int, h: int, w: int, th: float, limit=None):
    """the literal formulation in float64 torch -> (mask uint8 [n, h, w], the smallest |P / mx - th| over the coarse cells of the rows with a
    non-empty table and a positive maximum)"""
    import torch
    import torch.nn.functional as F
    n2, T, HW = acc.shape
    n = n2 // 2
    a = torch.from_numpy(acc).double().view(n2, T, hl, wl)
    bits, closest = [], float("inf")
    for r in range(n2):
        pos = [int(p) for p in words[r] if 0 <= p < T]
        if not pos:
            bits.append(torch.zeros(h, w, dtype=torch.bool))
            continue
        m = a[r, pos].sum(0)[None, None]
        pooled = F.max_pool2d(m, kernel_size=3, stride=1, padding=1)          # (-inf padding: the windows are clipped)
        up = F.interpolate(pooled, size=(h, w), mode="nearest")
        mx = up.max()
        if float(mx) > 0.0:
            closest = min(closest, float(((pooled / pooled.max()) - th).abs().min()))
            bits.append((up / mx).gt(th)[0, 0])
        else:
            bits.append(torch.zeros(h, w, dtype=torch.bool))
    bits = torch.stack(bits)
    mask = bits[:n] | bits[n:]
    if limit is not None:
        mask = mask & torch.from_numpy(np.asarray(limit).reshape(h, w) != 0)[None]
    return (mask.to(torch.uint8) * 255).numpy(), closest
