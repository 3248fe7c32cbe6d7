"""numpy reference of the MultiDiffusion canvas (textboost_amd/canvas.py, csrc/canvas.hip): the window offsets, the gather, the
canvas step in float64 (and restated in float32 in the kernel's summation order: the yardstick of the GPU tests' bound), the blend weights
and the tile blend.  Written from the definitions, not from the package: tests/test_canvas_host.py holds `canvas.CanvasPlan` against it."""
import numpy as np


def offsets(L, S, s):
    """o_k = min(k s, L - S), k = 0 .. ceil((L - S) / s)"""
    n = -(-(L - S) // s) + 1
    return [min(k * s, L - S) for k in range(n)]


def pairs(n, oy, ox):
    """(img, oy, ox) of pair p = img * nw + iy * nx + ix"""
    return [(img, y, x) for img in range(n) for y in oy for x in ox]


def to_half(a, kind):
    """float32 array -> the library's 16-bit type (torch tensor), round to nearest even"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16 if kind == "bf16" else torch.float16)


def gather(x, S, oy, ox, Bu, chunk, kind):
    """x float32 [n, 4, Hc, Wc] -> x2 16-bit [2 Bu, 4, S, S] (torch): rows r and Bu + r = the crop of pair chunk * Bu + r, rows past the pair
    list = the last valid pair"""
    import torch
    pl = pairs(x.shape[0], oy, ox)
    rows = []
    for r in range(Bu):
        img, y, xx = pl[min(chunk * Bu + r, len(pl) - 1)]
        rows.append(x[img, :, y:y + S, xx:xx + S])
    h = to_half(np.stack(rows), kind)
    return torch.cat([h, h])


def scatter_eps(eps_pairs, Bu, fill=0.0):
    """per-pair (e_u, e_c) float arrays [pairs, 4, S, S] -> eps_all float32 [n_chunks, 2 Bu, 4, S, S] (unused rows = fill)"""
    eu, ec = eps_pairs
    P = eu.shape[0]
    nch = -(-P // Bu)
    out = np.full((nch, 2 * Bu) + eu.shape[1:], fill, dtype=np.float32)
    for p in range(P):
        out[p // Bu, p % Bu] = eu[p]
        out[p // Bu, Bu + p % Bu] = ec[p]
    return out


def step(x, m_prev, eps_all, S, oy, ox, Bu, g, alpha_t, sigma_t, ca, cb, cc, dtype=np.float64):
    """the canvas step in `dtype`: per element, over the covering windows in ascending k, eps = sum(e_u + g (e_c - e_u)) / count, then
    m0 = (x - sigma_t eps) / alpha_t, xn = ca x + cb m0 + cc m_prev.  -> (xn, m0).  float32: every operation rounded to float32, in the
    kernel's order (it may fuse a multiply-add, which this restatement does not: that is inside the bound's factor)."""
    T = dtype
    n, C, Hc, Wc = x.shape
    e = eps_all.astype(T)
    g, alpha_t, sigma_t, ca, cb, cc = (T(v) for v in (g, alpha_t, sigma_t, ca, cb, cc))
    total = np.zeros(x.shape, dtype=T)
    count = np.zeros(x.shape, dtype=T)
    for p, (img, y, xx) in enumerate(pairs(n, oy, ox)):        # ascending k within an image
        eu, ec = e[p // Bu, p % Bu], e[p // Bu, Bu + p % Bu]
        guided = (eu + g * (ec - eu)).astype(T)
        total[img, :, y:y + S, xx:xx + S] = (total[img, :, y:y + S, xx:xx + S] + guided).astype(T)
        count[img, :, y:y + S, xx:xx + S] += 1
    assert (count > 0).all()
    eps = (total / count).astype(T)
    xv, mp = x.astype(T), m_prev.astype(T)
    m0 = ((xv - (sigma_t * eps).astype(T)).astype(T) / alpha_t).astype(T)
    xn = (((ca * xv).astype(T) + (cb * m0).astype(T)).astype(T) + (cc * mp).astype(T)).astype(T)
    return xn, m0


def axis_weight(t, O, P, Lp, R):
    lo = R if O == 0 else min(t - O + 1, R)
    hi = R if O + P == Lp else min(O + P - t, R)
    return min(lo, hi) / R


def weight_map(O_y, O_x, P, Hp, Wp, R, dtype=np.float64):
    """w = w_y w_x of one tile, [P, P]"""
    wy = np.array([axis_weight(O_y + i, O_y, P, Hp, R) for i in range(P)], dtype=dtype)
    wx = np.array([axis_weight(O_x + j, O_x, P, Wp, R) for j in range(P)], dtype=dtype)
    return (wy[:, None] * wx[None, :]).astype(dtype)


def blend(tiles, n, P, ty, tx, Hp, Wp, R, dtype=np.float64):
    """tiles float32 [n * nty * ntx, P, P, 3] (NHWC) -> (value [n, 3, Hp, Wp] = sum w v / sum w in `dtype`, weight sum [Hp, Wp])"""
    T = dtype
    acc = np.zeros((n, Hp, Wp, 3), dtype=T)
    ws = np.zeros((Hp, Wp), dtype=T)
    for k, (img, y, x) in enumerate(pairs(n, ty, tx)):
        w = weight_map(y, x, P, Hp, Wp, R, T)
        acc[img, y:y + P, x:x + P] = (acc[img, y:y + P, x:x + P] + (w[:, :, None] * tiles[k].astype(T)).astype(T)).astype(T)
        if img == 0:
            ws[y:y + P, x:x + P] = (ws[y:y + P, x:x + P] + w).astype(T)
    val = (acc / ws[None, :, :, None]).astype(T)
    return val.transpose(0, 3, 1, 2), ws


def image_of(val):
    """clamp(v / 2 + 0.5, 0, 1)"""
    return np.clip(val * 0.5 + 0.5, 0.0, 1.0)


def rel_err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))
