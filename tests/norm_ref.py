"""Float64 references for GroupNorm(+SiLU) / LayerNorm (forward and input gradient), an elementwise error bound derived from the conditioning of
the data, and the table of cases and data regimes shared by tests/test_norm_ref_host.py (CPU) and tests/test_gpu_norm_scale.py (the kernels).

Nothing here calls torch.nn.functional and nothing is taken from the code under test: the bound is a function of the (rounded) inputs, the number
formats and `k`, the number of fp32 additions an input passes through on the path under test, which is read off the kernel's STRUCTURE (below).

Notation: u = 2^-24 (unit roundoff of fp32).  Per group (GroupNorm) or row (LayerNorm) of n elements: mean, var (biased), rstd = 1/sqrt(var + eps),
xhat = (x - mean) rstd, z = xhat gamma + beta, y = silu?(z).

FORWARD BOUND  |y_kernel - y_ref| <= f (t_stat + t_apply) + t_silu + t_round
  t_stat   first-order propagation of the statistics' error:  |gamma| (|xhat| e_r + rstd e_m), where
           e_m = k u mean|x|                      (textbook bound of a k-addition fp32 sum, divided by n)
           e_v = k u (mean x^2 + 2 |mean| mean|x|)  one-pass form  var = Q/n - mean^2: the error of Q/n plus 2 |mean| e_m;
           e_v = k u var + e_m^2                    mean-first form var = mean (x - mean')^2: a shifted mean changes the centred sum in 2nd order only
           e_r = relative error of rstd.  With rho = e_v / (var + eps) its first-order value is rho / 2; it is evaluated in closed form,
                 max(1/sqrt(max(1 - rho, eps/(var+eps))) - 1, 1 - 1/sqrt(1 + rho)), which is >= rho/2, equals it to first order, and stays TRUE when rho is
                 not small (the envelope regime; the variance is clamped at zero, so var' + eps >= eps).
  t_apply  A u (|x sc| + |mean sc| + |beta|), sc = rstd gamma, for the one-pass apply  z = x sc + (beta - mean sc):  rsqrt (1 ulp = 2u) and
           rstd*gamma (u) give sc to 3u; x sc: +u; mean sc: +u; beta - mean sc: u (|beta| + |mean sc|); the last add: u |z|.  Sum <= 5u|x sc| + 6u|mean sc|
           + 2u|beta| <= 8u (...): A = 8.  (|beta| + |mean sc| >= |sh|: the rounding of mean*sc does not shrink when beta cancels it.)
           Mean-first apply  z = (x - mean) rstd gamma + beta:  A u (|xhat gamma| + |beta|) with the same A.
  f        1.1 >= sup|silu'| when SiLU is on (the error of z passes through silu), else 1
  t_silu   S u (|y| + 0.6), S = 8: silu is evaluated as z / (1 + exp(-z)) with a fast exp whose relative error grows like |z| u; the induced absolute error
           of silu is ~ z^2 s (1 - s) u <= 0.6 u-multiples (sup of z^2 e^-|z| is 0.54), plus the division and the add.
  t_round  half an ulp of the OUTPUT type at |y_ref| + the terms above -- the value's true ulp, so an element near zero is held tightly.

BACKWARD BOUND  dx = rstd (d - m1 - xhat m2) (+ add),  d = dy silu'(z) gamma,  m1 = mean d,  m2 = mean(d xhat);  the kernel reads (mean, rstd) from the
forward launch, so they carry e_m and e_r (+ 2u):
  dxh = |xhat| (e_r + 3u) + rstd e_m                                     error of xhat
  dz  = |gamma| dxh + 3u (|xhat gamma| + |beta|)                           error of the silu' argument
  dd  = |dy gamma| (0.5 dz + 32u) + 3u |d|   (|silu''| <= 0.5; 32u: silu' = s (1 + z (1 - s)) loses |z| u in 1 - s while 1 - s matters, |z| < 17, + exp)
        (no SiLU: dd = 2u |d|)
  dm1 = mean dd + kb u mean|d|,   dm2 = mean(dd |xhat| + |d| dxh) + kb u mean|d xhat|     (kb: additions on the backward path)
  e   = rstd (dd + dm1 + |xhat| dm2 + |m2| dxh) + (e_r + 2u) |dx - add| + 4u rstd (|d| + |m1| + |xhat m2|) + u |dx|,   + half an output ulp at |dx| + e.

k PER PATH (`path_stages`): a path is a list of stage lengths; a stage of length L is a strictly sequential fp32 sum of L values (L - 1 roundings for the
value added first), a tree level is a stage of length 2.  k = sum(L - 1) + 4 (the divisions by n, mean^2 and the subtraction).
  twopass  gn_stats_kernel: a thread sums ceil(rpc / nrl) rows of one channel; gn_block_group_reduce: one thread adds nrl * gs values; gn_block_finalize:
           ceil(nchunks / 8) chunk partials per lane, then 8 sequentially.
  fused    gn_fused_fwd/bwd_kernel (256 threads per slice; also the split-K consumer): 8 * ceil(HW gs / 8 / 256) values per thread, 6 butterfly levels, 2 tree levels.
  slice    gn_slice_fwd/bwd_kernel (1024 threads per slice): the two channels of a dword are added first (2), then ceil(HW / (1024 // (gs/2))) dwords per thread,
           6 butterfly levels, 16 wave totals sequentially.
  f32      gn_f32_*_kernel (mean first): ceil(HW gs / 256) per thread, 6 butterfly levels, 4 wave totals.
  ln       ln_fwd/bwd_kernel (mean first, one wave per row): 8 * ceil(C / 8 / 64) per lane, 6 butterfly levels.

THE LAYERNORMS THAT RIDE IN OTHER LAUNCHES (tests/test_gpu_fused_norm_scale.py); all mean first, on the 16-bit-ROUNDED row the launch writes:
  epi      gemm8.hip, TB_ACT_LN_FWD / TB_ACT_LN_BWD epilogue of the row-spanning Linear tiles (N = 320): a thread adds the 8 values of its column
           group sequentially (8), the C / 8 = 40 partials of a row go through the LDS to 8 reducer lanes that add C / 64 = 5 each sequentially (5),
           then 3 xor-shuffle levels (2, 2, 2).  k = 7 + 4 + 3 + 4 = 18 at C = 320.  LN_BWD sums g and g xhat over the same structure (kb = k) and
           reads (mean, rstd) as the preceding LN_FWD launch wrote them (k of this path).
  chain    ff_chain.h ff_chain_layernorm (tb_chain320; tb_ff_fwd with pre_W): four threads per row, each adds its C / 4 = 80 values sequentially
           (80), then 2 shuffle levels (2, 2).  k = 79 + 2 + 4 = 85 at C = 320.
  ffbwd    ff_fused.hip, tb_ff_bwd with ln_x (backward sums only, kb): a lane adds its 10 x 4 = C / 8 accumulator values sequentially (40), 2 shuffle
           levels (2, 2), one addition across the two waves of the row band (2).  kb = 39 + 3 + 4 = 46; (mean, rstd) are tb_ff_fwd's pre_stats (chain).

THE FOLDED LAYERNORM (`fold_stages`, `fold_forward_bound`; one pass: var = Q / K - mean^2, clamped at zero).  Producer (gemm8.hip, rs_out): a thread adds
the 8 rounded outputs of its column group and their squares sequentially (8), thread t < PR adds the tile's (tile width / 8) unit partials sequentially
(tile width = C / slots) and writes slot tn; consumer (gemm8.hip rs_in: 8 + 8 slots; gemm.hip: 16, unused ones exact zeros): up to 16 slots added
sequentially (16).  k = 7 + (C / slots / 8 - 1) + 15 + 4: 35 where the producers take 80-column tiles, 45 with 160-column tiles.
  out = rstd (alpha acc - mean c1) + c2 (+ R),  acc = sum_k x_k W'_nk  (x: the written 16-bit row, W' = half(gamma (.) W), c1 = row sums of W', c2 = b + W beta:
  the reference takes all of them AS THE KERNEL SEES THEM; the rounding of gamma (.) W is a stated divergence of the fold, not under test).
  |out_kernel - out_ref| <= t_stat + t_acc + t_apply + t_round:
  t_stat   |rstd (acc - mean c1)| e_r + rstd |c1| e_m, (e_m, e_r) = _stat_errors(row of width K, k, "onepass")
  t_acc    rstd K u sum_k |x_k W'_nk|: the fp32 accumulation of acc (any order: at most K roundings at the magnitude of the absolute sum).  It is what
           matters when |mean| / std is large: acc and mean c1 are both ~ |mean| |c1| and cancel to the size of the fluctuation.
  t_apply  A u (rstd (|acc| + |mean c1|) + |c2| + |R|), A = 8: mean c1 (u), the subtraction (u), rsqrt + the product with rstd (3u), + c2 (u), + R (u), each
           at most at the magnitude of the terms it combines
  t_round  half an ulp of the output type at |out_ref| + the terms above.
"""
import torch

U = 2.0 ** -24
A_APPLY, S_SILU = 8.0, 8.0
_FMT = {torch.float16: (10, -14), torch.bfloat16: (7, -126), torch.float32: (23, -126)}   # (mantissa bits, exponent of the smallest normal)


def ulp(v, dtype):
    """the spacing of `dtype` at |v| (float64 tensor): 2^(floor(log2 |v|) - p), subnormals included"""
    p, emin = _FMT[dtype]
    _, e = torch.frexp(v.abs().double().clamp_min(2.0 ** emin))     # |v| = m 2^e, m in [0.5, 1); below the smallest normal the spacing is constant
    e = (e - 1).double()
    return torch.pow(torch.tensor(2.0, dtype=torch.float64, device=v.device), e - p)


class _Core:
    pass


def _core(x, gamma, beta, B, HW, C, G, eps, silu, dy=None, add=None):
    gs = C // G
    c = _Core()
    c.shape = (B, HW, G, gs)
    c.X = x.double().reshape(B, HW, G, gs)
    c.ga = gamma.double().reshape(1, 1, G, gs)
    c.be = beta.double().reshape(1, 1, G, gs) if beta is not None else torch.zeros_like(c.ga)
    c.mean = c.X.mean((1, 3), keepdim=True)
    xc = c.X - c.mean
    c.var = (xc * xc).mean((1, 3), keepdim=True)
    c.rstd = 1.0 / torch.sqrt(c.var + eps)
    c.xh = xc * c.rstd
    c.z = c.xh * c.ga + c.be
    c.sg = torch.sigmoid(c.z) if silu else None
    c.y = c.z * c.sg if silu else c.z
    c.dx = None
    if dy is not None:
        d = dy.double().reshape(B, HW, G, gs)
        c.dyg = d * c.ga
        if silu:
            c.sp = c.sg * (1.0 + c.z * (1.0 - c.sg))
            d = d * c.sp
        c.d = d * c.ga
        c.m1 = c.d.mean((1, 3), keepdim=True)
        c.m2 = (c.d * c.xh).mean((1, 3), keepdim=True)
        c.dxn = c.rstd * (c.d - c.m1 - c.xh * c.m2)
        c.dx = c.dxn + (add.double().reshape(B, HW, G, gs) if add is not None else 0.0)
    return c


def groupnorm_ref(x, gamma, beta, B, HW, C, G, eps, silu, dy=None, add=None):
    """float64 GroupNorm(+SiLU) over x [B*HW, C] (NHWC rows; the values the kernel reads, i.e. already rounded to its input type).
    Returns (y [B*HW, C], (mean, rstd) each [B, G], dx [B*HW, C] or None)."""
    c = _core(x, gamma, beta, B, HW, C, G, eps, silu, dy, add)
    return (c.y.reshape(B * HW, C), (c.mean.reshape(B, G), c.rstd.reshape(B, G)), None if c.dx is None else c.dx.reshape(B * HW, C))


def layernorm_ref(x, gamma, beta, eps, dy=None, add=None):
    """float64 LayerNorm over the rows of x [M, C].  Returns (y, (mean, rstd) each [M], dx or None).  (`beta` = None for the backward alone.)"""
    M, C = x.shape
    y, (mean, rstd), dx = groupnorm_ref(x, gamma, beta, M, 1, C, 1, eps, False, dy, add)
    return y, (mean.reshape(M), rstd.reshape(M)), dx


def _stat_errors(c, eps, k, form):
    amean = c.X.abs().mean((1, 3), keepdim=True)
    e_m = k * U * amean
    if form == "onepass":
        e_v = k * U * ((c.X * c.X).mean((1, 3), keepdim=True) + 2.0 * c.mean.abs() * amean)
    else:
        assert form == "meanfirst", form
        e_v = k * U * c.var + e_m * e_m
    rho = e_v / (c.var + eps)
    low = 1.0 / torch.sqrt(torch.maximum(1.0 - rho, eps / (c.var + eps))) - 1.0
    high = 1.0 - 1.0 / torch.sqrt(1.0 + rho)
    return e_m, torch.maximum(low, high)


def forward_bound(x, gamma, beta, B, HW, C, G, eps, silu, k, out_dtype, form, parts=False):
    """elementwise bound [B*HW, C] on |kernel y - groupnorm_ref y| (module docstring).  parts=True: also (t_stat, (e_m, rstd e_r) per group)."""
    c = _core(x, gamma, beta, B, HW, C, G, eps, silu)
    e_m, e_r = _stat_errors(c, eps, k, form)
    t_stat = c.ga.abs() * (c.xh.abs() * e_r + c.rstd * e_m)
    sc = c.rstd * c.ga
    if form == "onepass":
        t_apply = A_APPLY * U * ((c.X * sc).abs() + (c.mean * sc).abs() + c.be.abs())
    else:
        t_apply = A_APPLY * U * ((c.xh * c.ga).abs() + c.be.abs())
    e = t_stat + t_apply
    if silu:
        e = 1.1 * e + S_SILU * U * (c.y.abs() + 0.6)
    e = e + 0.5 * ulp(c.y.abs() + e, out_dtype)
    e = e.reshape(B * HW, C)
    if parts:
        return e, t_stat.reshape(B * HW, C), (e_m.reshape(B, G), (c.rstd * (e_r + 3 * U)).reshape(B, G))
    return e


def backward_bound(x, dy, add, gamma, beta, B, HW, C, G, eps, silu, k, kb, out_dtype, form):
    """elementwise bound [B*HW, C] on |kernel dx - groupnorm_ref dx| (module docstring); k: the forward path's additions (it made the statistics the
    backward reads), kb: the backward path's."""
    c = _core(x, gamma, beta, B, HW, C, G, eps, silu, dy, add)
    e_m, e_r = _stat_errors(c, eps, k, form)
    axh = c.xh.abs()
    dxh = axh * (e_r + 3 * U) + c.rstd * e_m
    if silu:
        dz = c.ga.abs() * dxh + 3 * U * ((c.xh * c.ga).abs() + c.be.abs())
        dd = c.dyg.abs() * (0.5 * dz + 32 * U) + 3 * U * c.d.abs()
    else:
        dd = 2 * U * c.d.abs()
    mean = lambda t: t.mean((1, 3), keepdim=True)
    dm1 = mean(dd) + kb * U * mean(c.d.abs())
    dm2 = mean(dd * axh + c.d.abs() * dxh) + kb * U * mean((c.d * c.xh).abs())
    e = (c.rstd * (dd + dm1 + axh * dm2 + c.m2.abs() * dxh) + (e_r + 2 * U) * c.dxn.abs()
         + 4 * U * c.rstd * (c.d.abs() + c.m1.abs() + (c.xh * c.m2).abs()) + U * c.dx.abs())
    e = e + 0.5 * ulp(c.dx.abs() + e, out_dtype)
    return e.reshape(B * HW, C)


def layernorm_forward_bound(x, gamma, beta, eps, k, out_dtype, parts=False):
    M, C = x.shape
    return forward_bound(x, gamma, beta, M, 1, C, 1, eps, False, k, out_dtype, "meanfirst", parts)


def layernorm_backward_bound(x, dy, add, gamma, eps, k, out_dtype):
    M, C = x.shape
    return backward_bound(x, dy, add, gamma, None, M, 1, C, 1, eps, False, k, k, out_dtype, "meanfirst")


RESULTS = []   # (name, worst error / bound) of every check() of the process, for the summary tables


def check(name, got, ref, bound, info=None, verbose=True):
    """assert |got - ref| <= bound elementwise (and that `got` is finite).  Prints the worst error / bound, its index and -- `info(index)`, a string --
    the group or row statistics there.  Returns the worst ratio."""
    a, b, bd = got.detach().double(), ref.detach().double(), bound.detach().double()
    assert a.shape == b.shape == bd.shape, (name, a.shape, b.shape, bd.shape)
    finite = bool(torch.isfinite(a).all())
    ratio = torch.where(torch.isfinite(a), (a - b).abs() / bd.clamp_min(1e-300), torch.full_like(a, float("inf")))
    ratio = torch.where(((a - b) == 0) & torch.isfinite(a), torch.zeros_like(ratio), ratio)
    flat = int(ratio.argmax())
    idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), ratio.shape))
    w = ratio.reshape(-1)[flat].item()
    msg = (f"{name}: worst error/bound {w:.3f} at {idx}: got {a.reshape(-1)[flat].item():.6e} ref {b.reshape(-1)[flat].item():.6e} "
           f"bound {bd.reshape(-1)[flat].item():.3e}" + (f"  [{info(idx)}]" if info is not None else "") + ("" if finite else "  NON-FINITE OUTPUT"))
    if verbose:
        print("[norm-bound]", msg)
    RESULTS.append((name, w))
    assert finite and w <= 1.0, msg
    return w


def sliced(rows, C, dtype, fill, sliced, device):
    """a [rows, C] tensor, when `sliced` a column slice of a wider buffer whose margins hold `fill`.  Returns (view, buffer or None)."""
    if not sliced:
        return torch.full((rows, C), fill, device=device, dtype=dtype), None
    buf = torch.full((rows, C + 24), fill, device=device, dtype=dtype)
    return buf[:, 8:8 + C], buf


def margins_untouched(buf, C, fill):
    return buf is None or (bool((buf[:, :8] == fill).all()) and bool((buf[:, 8 + C:] == fill).all()))


# ------------------------------------------------------------------------------------------------------------------ dispatch and k, from the structure
def _cdiv(a, b):
    return (a + b - 1) // b


def gn_chunks(B, HW, C):
    """row chunks per image of the two-pass kernels (norm.hip gn_chunks)"""
    cols = C >> 3
    cw = min(cols, 256)
    nrl = 256 // cw
    n = _cdiv(HW, nrl * 4)
    for r in (16, 8):
        nr = _cdiv(HW, nrl * r)
        if nr * B >= 640:
            n = nr
            break
    return max(1, min(n, max(1, 2048 // B)))


def gn_path(B, HW, C, G, bwd=False, variant=11):
    """which 16-bit GroupNorm kernels a shape takes (norm.hip gn_fused_ok / gn_slice_nv): 'fused', 'slice<NV>' or 'twopass'"""
    gs = C // G
    if (variant & 1) and gs % 8 == 0 and HW * (gs // 8) <= 2560 and B * G >= 128:
        return "fused"
    if (variant & 2) and gs % 2 == 0 and gs <= 128 and B * G >= 128:
        nv = _cdiv(HW, 1024 // (gs // 2))
        if nv <= 11:
            return "slice11"
        if not (bwd and not (variant & 4)):
            if nv <= 22:
                return "slice22"
            if not bwd:
                if nv <= 33:
                    return "slice33"
                if nv <= 44:
                    return "slice44"
    return "twopass"


def path_stages(path, B, HW, C, G):
    """stage lengths of the path's summation (module docstring)"""
    gs = C // G
    if path == "twopass":
        cw = min(C >> 3, 256)
        nrl = 256 // cw
        nch = gn_chunks(B, HW, C)
        rpc = _cdiv(HW, nch)
        return [_cdiv(rpc, nrl), nrl * gs, _cdiv(nch, 8), 8]
    if path in ("fused", "splitk"):
        return [8 * _cdiv(HW * (gs // 8), 256)] + [2] * 8
    if path.startswith("slice"):
        return [2, _cdiv(HW, 1024 // (gs // 2))] + [2] * 6 + [16]
    if path == "f32":
        return [_cdiv(HW * gs, 256)] + [2] * 6 + [4]
    if path == "ln":
        return [8 * _cdiv(C // 8, 64)] + [2] * 6
    if path == "epi":
        assert C % 64 == 0, C
        return [8, C // 64, 2, 2, 2]
    if path == "chain":
        assert C % 4 == 0, C
        return [C // 4, 2, 2]
    if path == "ffbwd":
        assert C % 8 == 0, C
        return [C // 8, 2, 2, 2]
    raise ValueError(path)


def k_of(stages):
    return sum(s - 1 for s in stages) + 4


def k_path(path, B, HW, C, G):
    return k_of(path_stages(path, B, HW, C, G))


def fold_stages(C, slots):
    """stage lengths of the folded LayerNorm's (sum, sum of squares) over a row of width C that the producers cut into `slots` column tiles"""
    assert 1 <= slots <= 16 and C % (8 * slots) == 0, (C, slots)
    return [8, C // slots // 8, 16]


def fold_ref(x, Wp, c1, c2, R, eps):
    """float64 value of the folded consumer's output [M, N] from the operands the kernel reads, (mean, rstd) [M], and the magnitudes the bound needs"""
    X, W = x.double(), Wp.double()
    mean = X.mean(1, keepdim=True)
    var = ((X - mean) ** 2).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    acc = X @ W.T
    mc1 = mean * c1.double()[None, :]
    out = rstd * (acc - mc1) + c2.double()[None, :] + (R.double() if R is not None else 0.0)
    return out, (mean.reshape(-1), rstd.reshape(-1)), (acc, mc1, X.abs() @ W.abs().T)


def fold_forward_bound(x, Wp, c1, c2, R, eps, k, out_dtype, parts=False):
    """elementwise bound [M, N] on |kernel out - fold_ref out| (module docstring).  parts=True: also (e_m, rstd e_r) per row."""
    M, K = x.shape
    out, (mean, rstd), (acc, mc1, aabs) = fold_ref(x, Wp, c1, c2, R, eps)
    c = _core(x, torch.ones(K, device=x.device), None, M, 1, K, 1, eps, False)
    e_m, e_r = _stat_errors(c, eps, k, "onepass")
    e_m, e_r, rs = e_m.reshape(M, 1), e_r.reshape(M, 1), rstd.reshape(M, 1)
    t_stat = (rs * (acc - mc1)).abs() * e_r + rs * c1.double().abs()[None, :] * e_m
    t_acc = rs * K * U * aabs
    t_apply = A_APPLY * U * (rs * (acc.abs() + mc1.abs()) + c2.double().abs()[None, :] + (R.double().abs() if R is not None else 0.0))
    e = t_stat + t_acc + t_apply
    e = e + 0.5 * ulp(out.abs() + e, out_dtype)
    if parts:
        return e, (e_m.reshape(M), (rs * (e_r + 3 * U)).reshape(M))
    return e


def offset_ratio(k, xmax=4.0):
    """the largest power of two r <= 32 for |mean| / std that keeps the CAP for a one-pass path with k additions: the statistics term of the forward
    bound, |gamma| (|xhat| e_r + rstd e_m) at its largest element (|xhat| ~ xmax, unit variance: e_r = k u (3 r^2 + 1) / 2, e_m = k u (r + 0.8)),
    within 2 ulps of the fp16 output there; 2 ulps >= 2^-10 |z| wherever |z| sits in its binade, and |z| ~ |gamma| xmax.  (fp16 is the stricter of
    the two half types; the bf16 build runs the same data.)"""
    r = 32
    while r > 1 and 0.5 * k * U * (3 * r * r + 1) + k * U * (r + 0.8) / xmax > 2.0 ** -10:
        r //= 2
    return r


# ------------------------------------------------------------------------------------------------------------------ cases
class GNCase:
    def __init__(self, B, HW, C, path, bwd_path=None, variant=None, f32=False, splitk=False):
        self.B, self.HW, self.C, self.G = B, HW, C, 32
        self.path, self.bwd_path, self.variant, self.f32, self.splitk = path, bwd_path, variant, f32, splitk
        self.form = "meanfirst" if f32 else "onepass"
        self.k = k_path(path, B, HW, C, 32)
        self.kb = k_path(bwd_path, B, HW, C, 32) if bwd_path else None
        self.ratio = 32 if f32 else offset_ratio(self.k)

    @property
    def id(self):
        return f"{self.path}{'-forced' if self.variant == 0 else ''}-{self.B}x{self.HW}x{self.C}"


GN_CASES = [
    GNCase(2, 100, 64, "twopass", "twopass"), GNCase(1, 25, 2560, "twopass", "twopass"),                 # B * G < 128
    GNCase(4, 64, 256, "twopass", "twopass", variant=0), GNCase(4, 100, 512, "twopass", "twopass", variant=0),   # forced on the fused shapes
    GNCase(4, 64, 256, "fused", "fused"), GNCase(4, 100, 512, "fused", "fused"),
    GNCase(4, 640, 1024, "fused", "fused"),                                                              # HW * gs / 8 = 2560: the edge of its condition
    GNCase(4, 256, 320, "slice11", "slice11"), GNCase(4, 256, 64, "slice11", "slice11"),
    GNCase(4, 576, 1280, "slice22"), GNCase(4, 1296, 1280, "slice33"), GNCase(4, 1764, 1280, "slice44"),   # forward only
    GNCase(4, 64, 256, "splitk", splitk=True),
    GNCase(2, 64, 64, "f32", "f32", f32=True), GNCase(1, 16, 1280, "f32", "f32", f32=True),
]
LN_CASES = [(5, 64), (5, 520), (5, 1536), (130, 768)]
LN_DTYPES = [("f32", "h"), ("h", "h"), ("f32", "f32")]    # (x, y): h = the library's 16-bit type
LN_OFFSETS = (256.0, -32.0, 8.0, -128.0, 1.0)             # |mean| / std per row, cycled

REGIMES = ("tiny", "offset", "huge", "mixed", "degenerate")
ENVELOPE = ("envelope32", "envelope")    # 16-bit GroupNorm only: randn + 32 and randn + 256 in every group, whatever the cap says; asserted against
                                         # the full worst-case bound (which stays true) and finiteness, the measured error is recorded
REGIME_EPS = {"tiny": (1e-5, 1e-6), "offset": (1e-5,), "huge": (1e-6,), "mixed": (1e-5,), "degenerate": (1e-6,), "envelope": (1e-5,),
              "envelope32": (1e-5,)}
UNIT = "unit"    # the data of the existing tests (randn * 2 + 0.5), for the host test's statement of what they cannot see


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def gn_params(regime, C, seed=7):
    """gamma with zeros and negative entries (and +-32 on a few channels in `huge`: SiLU arguments past +-90), beta nonzero; fp32"""
    g = _gen(seed)
    gamma = torch.randn(C, generator=g) * 0.5 + 1.0
    beta = torch.randn(C, generator=g) * 0.3 + 0.1
    gamma[1::7] *= -1.0
    gamma[5::16] = 0.0
    if regime in ("huge", "mixed"):
        gamma[3], gamma[C // 2 + 1], gamma[C - 1] = 32.0, -32.0, 32.0
    beta[beta.abs() < 0.02] = 0.05
    return gamma, beta


_KINDS = ("tiny", "huge", "offset", "unit")


def _scale_offset(kind, ratio, sign_size):
    if kind == "tiny":
        return 2.0 ** -9, 0.0
    if kind == "huge":
        return 2.0 ** 10, 0.0
    if kind == "offset":
        return 1.0, ratio * sign_size
    return 1.0, 0.0


def gn_input(regime, B, HW, C, G, dtype, ratio=32, seed=11):
    """x [B*HW, C] of `dtype` (CPU), seeded; rounded to the input type here, so the reference sees what the kernel reads"""
    gs = C // G
    x = torch.randn(B, HW, G, gs, generator=_gen(seed + B + HW + C))
    if regime == UNIT:
        x = x * 2 + 0.5
    elif regime.startswith("envelope"):
        x = x + float(regime[len("envelope"):] or 256)
    elif regime in ("tiny", "huge"):
        x = x * _scale_offset(regime, 0, 0)[0]
    elif regime in ("offset", "mixed"):
        sc = torch.ones(B, 1, G, 1)
        of = torch.zeros(B, 1, G, 1)
        for b in range(B):
            for g in range(G):
                ss = (-1.0 if (b + g) & 1 else 1.0) * (1.0, 0.5, 0.75)[(b + 2 * g) % 3]     # sign and size differ per group and per image
                kind = "offset" if regime == "offset" else _KINDS[(b + 2 * (g & 1)) % 4]     # mixed: image b is kind b, its odd groups trade scale
                if regime == "offset" and g == 0:
                    ss = 1.0 if b & 1 else -1.0                                               # the full ratio, in every image
                sc[b, 0, g, 0], of[b, 0, g, 0] = _scale_offset(kind, ratio, ss)
        x = x * sc + of
    elif regime == "degenerate":
        x[0, :, 0, :] = 0.0
        x[0, :, 1, :] = 2.0
        x[B - 1, :, G - 1, :] = 3.1
    else:
        raise ValueError(regime)
    return x.reshape(B * HW, C).to(dtype)


def fold_offsets(k):
    """LN_OFFSETS scaled so that the largest is what offset_ratio admits for a one-pass path with k additions"""
    r = offset_ratio(k)
    return tuple(o * r / 256.0 for o in LN_OFFSETS)


def ln_input(regime, M, C, dtype, seed=13, offsets=None):
    """x [M, C] of `dtype` (CPU), seeded.  offsets: |mean| / std per row of `offset`, cycled (default LN_OFFSETS; the one-pass fold: fold_offsets(k))"""
    LN_OFFSETS = offsets or globals()["LN_OFFSETS"]
    x = torch.randn(M, C, generator=_gen(seed + M + C))
    if regime == UNIT:
        x = x * 1.5 + 0.2
    elif regime in ("tiny", "huge"):
        x = x * _scale_offset(regime, 0, 0)[0]
    elif regime == "offset":
        x = x + torch.tensor([LN_OFFSETS[m % len(LN_OFFSETS)] for m in range(M)]).reshape(M, 1)
    elif regime == "mixed":
        for m in range(M):
            s, o = _scale_offset(_KINDS[m % 4], max(abs(v) for v in offsets) if offsets else 32.0, -1.0 if m & 4 else 1.0)    # (its offset rows: 32, or the path's cap)
            x[m] = x[m] * s + o
    elif regime == "degenerate":
        x[0] = 0.0
        x[1] = 2.0
        x[M - 1] = 3.1
    else:
        raise ValueError(regime)
    return x.to(dtype)


def ln_params(regime, C, seed=17):
    return gn_params("unit" if regime != "huge" else "huge", C, seed)


# ------------------------------------------------------------------------------------------------------------------ split-K consumer operands
def splitk_operands(target, B, half, S=3, pad=8, seed=29):
    """fp32 k-slices [S, M, C + pad] and epilogue operands (bias [C], rowbias [B, C], 16-bit residual [M, C]) that add up to about `target` [M, C].
    Slice 0 carries +1000 and slice 2 -1000 on every element: they cancel only if the slices are ADDED (in fp32) before anything is squared or
    rounded.  The pad columns hold 7.0 and belong to nobody."""
    assert S == 3
    M, C = target.shape
    g = _gen(seed)
    bias = torch.randn(C, generator=g) * 0.1
    rowbias = torch.randn(B, C, generator=g) * 0.1
    res = (torch.randn(M, C, generator=g) * 0.5).to(half)
    t = target.double() - bias.double() - rowbias.double().repeat_interleave(M // B, 0) - res.double()
    s0 = (0.5 * t + 1000.0).float()
    s2 = (0.25 * t - 1000.0).float()
    s1 = (t - s0.double() - s2.double()).float()
    part = torch.full((S, M, C + pad), 7.0)
    for i, s in enumerate((s0, s1, s2)):
        part[i, :, :C] = s
    return dict(slices=[s0, s1, s2], part=part, npad=C + pad, bias=bias, rowbias=rowbias, R=res)


def splitk_sum64(sk, B):
    """float64 value of the x the consumer forms, and sum |terms| (the magnitude its fp32 additions round at)"""
    M = sk["R"].shape[0]
    terms = [s.double() for s in sk["slices"]] + [sk["bias"].double().expand(M, -1), sk["R"].double(), sk["rowbias"].double().repeat_interleave(M // B, 0)]
    return sum(terms), sum(t.abs() for t in terms)


def splitk_written_x(sk, B, half):
    """the x the consumer documents that it writes (norm.hip gnf_splitk_load_all): the slices added in slice order, + bias, + residual, + row bias, all
    in fp32, ONE rounding to the 16-bit type; the statistics are those of the rounded x"""
    s0, s1, s2 = sk["slices"]
    M = s0.shape[0]
    t = ((s0 + s1) + s2 + sk["bias"]) + sk["R"].float()
    t = t + sk["rowbias"].repeat_interleave(M // B, 0)
    return t.to(half)
