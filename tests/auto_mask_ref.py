"""numpy / torch-CPU restatement of the six stages of csrc/auto_mask.hip, for tests/test_auto_mask_host.py and
tests/test_gpu_auto_mask.py.  The word map and its bilinear resize are float64 (the kernel is held to an fp32 error bound against them); the
histogram and the mask bytes restate the kernel's fp32 expressions operation by operation (bit equality); Otsu's criterion is float64 on
exact integer prefix sums, as in the kernel."""
import numpy as np

F32 = np.float32


# ------------------------------------------------------------------------------------------------ stage 1: word map + bilinear resize
def bilinear_axis(n_in, n_out):
    """F.interpolate(mode="bilinear", align_corners=False) along one axis -> (lower index [n_out], upper index [n_out], upper weight [n_out]),
    float64: source coordinate (dst + 0.5) * (n_in / n_out) - 0.5 clamped at 0, upper neighbour clamped at n_in - 1"""
    src = (np.arange(n_out, dtype=np.float64) + 0.5) * (np.float64(n_in) / np.float64(n_out)) - 0.5
    src = np.maximum(src, 0.0)
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    return i0, i1, src - i0


def bilinear(m, H, W):
    """float64 [h, w] -> [H, W]"""
    m = np.asarray(m, dtype=np.float64)
    i0, i1, ly = bilinear_axis(m.shape[0], H)
    j0, j1, lx = bilinear_axis(m.shape[1], W)
    top = (1 - lx)[None, :] * m[i0][:, j0] + lx[None, :] * m[i0][:, j1]
    bot = (1 - lx)[None, :] * m[i1][:, j0] + lx[None, :] * m[i1][:, j1]
    return (1 - ly)[:, None] * top + ly[:, None] * bot


def word_upsample(acc, h, w, positions, weight, H, W):
    """acc [nb, T, h * w] -> (weight * bilinear(sum_b sum_p acc[b, positions[p]]), the same of |acc|: the sum of the absolute terms that the
    fp32 error bound scales with), float64 [H, W] each.  weight is taken as the fp32 number the C ABI receives."""
    a = np.asarray(acc, dtype=np.float64)[:, list(positions), :]
    wt = np.float64(F32(weight))
    m = a.sum(axis=(0, 1)).reshape(h, w)
    mabs = np.abs(a).sum(axis=(0, 1)).reshape(h, w)
    return wt * bilinear(m, H, W), abs(wt) * bilinear(mabs, H, W)


def upsample_bound(nb, npos, abs_terms):
    """per-element fp32 bound of the stated summation: nb * npos additions, then 6 more roundings (two lerps, weight, accumulate)"""
    return (nb * npos + 6) * 2.0 ** -23 * abs_terms


# ------------------------------------------------------------------------------------------------ stages 2-3: range, histogram
def normalised(score, lo, hi):
    """t = (s - lo) / (hi - lo), every operation rounded to fp32; 0 everywhere when hi == lo"""
    s, lo, hi = np.asarray(score, dtype=F32), F32(lo), F32(hi)
    if hi == lo:
        return np.zeros(s.shape, dtype=F32)
    with np.errstate(all="ignore"):
        return ((s - lo) / (hi - lo)).astype(F32)


def hist256(score, lo, hi):
    t = normalised(score, lo, hi)
    b = np.minimum(255, (t * F32(256.0)).astype(np.int64))
    return np.bincount(b.ravel(), minlength=256).astype(np.int64)


# ------------------------------------------------------------------------------------------------ stage 4: Otsu
def otsu_criterion(hist):
    """c(k) = (S w0 - N s0)^2 / (w0 (N - w0)) in float64 for the k with 0 < w0 < N, -1 elsewhere"""
    h = np.asarray(hist, dtype=np.int64)
    i = np.arange(256, dtype=np.int64)
    w0, s0 = np.cumsum(h), np.cumsum(h * i)
    N, S = int(w0[-1]), int(s0[-1])
    ok = (w0 > 0) & (w0 < N)
    num = np.float64(S) * w0.astype(np.float64) - np.float64(N) * s0.astype(np.float64)
    den = w0.astype(np.float64) * (N - w0).astype(np.float64)
    c = np.full(256, -1.0)
    c[ok] = (num[ok] * num[ok]) / den[ok]
    return c


def otsu(hist):
    """-> (threshold (k + 1) / 256 as fp32, k): the smallest k of maximal c; (1.0, 255) when no k splits the mass"""
    c = otsu_criterion(hist)
    if c.max() < 0:
        return F32(1.0), 255
    k = int(np.argmax(c))      # the first maximum
    return F32((k + 1) / 256.0), k


def otsu_margin(hist):
    """(best - runner-up) / best of the criterion: the test inputs must have a unique maximiser"""
    c = np.sort(otsu_criterion(hist))[::-1]
    return (c[0] - c[1]) / c[0] if c[0] > 0 else 0.0


def otsu_brute_force(hist):
    """the k that minimises the summed within-class squared deviation of the two classes {i <= k}, {i > k}, from the samples themselves"""
    v = np.repeat(np.arange(256), np.asarray(hist, dtype=np.int64)).astype(np.float64)
    best, best_k = None, None
    for k in range(255):
        a, b = v[v <= k], v[v > k]
        if a.size == 0 or b.size == 0:
            continue
        ss = ((a - a.mean()) ** 2).sum() + ((b - b.mean()) ** 2).sum()
        if best is None or ss < best:
            best, best_k = ss, k
    return best_k


# ------------------------------------------------------------------------------------------------ stages 5-6: mask bytes, dilation
def mask_from_score(score, lo, hi, thr, soft):
    t = normalised(score, lo, hi)
    if soft:
        return np.rint(F32(255.0) * np.clip(t, F32(0), F32(1))).astype(np.uint8)      # np.rint: round half to even
    return np.where(t >= F32(thr), 255, 0).astype(np.uint8)


def dilate(mask, r):
    """uint8 [H, W] -> the maximum over the (2r + 1)^2 square clipped at the borders: numpy maximum over shifted views of a zero-padded copy"""
    m = np.asarray(mask, dtype=np.uint8)
    H, W = m.shape
    p = np.zeros((H + 2 * r, W + 2 * r), dtype=np.uint8)
    p[r:r + H, r:r + W] = m
    rows = np.zeros((H + 2 * r, W), dtype=np.uint8)
    for d in range(2 * r + 1):
        np.maximum(rows, p[:, d:d + W], out=rows)
    out = np.zeros((H, W), dtype=np.uint8)
    for d in range(2 * r + 1):
        np.maximum(out, rows[d:d + H], out=out)
    return out
