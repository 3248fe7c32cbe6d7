"""The LayerNorms that ride in OTHER launches, off unit scale, elementwise against the float64 references of tests/norm_ref.py under its derived bounds
(regimes tiny / offset / huge / mixed / degenerate, both eps, the fp16 and the bf16 build):
  site 1  TB_ACT_LN_FWD epilogue   ops.gemm(ln_fwd=)            path "epi"
  site 2  TB_ACT_LN_BWD epilogue   ops.gemm(ln_bwd=)            path "epi" (statistics from site 1)
  site 3  the folded LayerNorm     ops.gemm(rs_out=) -> ops.gemm(lnfold=)     fold_stages / fold_forward_bound, both consumer kernels
  site 4  tb_chain320              ops.chain320                 path "chain"
  site 5  tb_ff_fwd with pre_W     ops.ff_fwd(pre=)             path "chain"
  site 6  tb_ff_bwd with ln_x      ops.ff_bwd(ln=)              path "ffbwd" (statistics from site 5)
The products around the LayerNorm are made EXACT so that its arithmetic is what is measured: the producing Linear gets an identity weight (x I^T is
exact in fp32), the regime's data rides in A ("A") or is split over A, bias and R ("split"; in `offset` the offset sits in R and the fluctuation in A,
as in a residual stream).  The reference input is always the row the launch WROTE, which is checked separately against the float64 sum.  Where the
normalised row never reaches memory (sites 4, 5) the product behind it is an identity / sign / permutation block that copies it out; one case per
site takes a random weight there under the composite bound  sum_k |W_nk| bound_k + K u sum_k |l_k W_nk| + half an output ulp.

Every check prints a [norm-bound] line; the last test of each build prints the worst error / bound per (build, site, regime, output)."""
import collections
import ctypes

import pytest
import torch

import act_ref as A
import norm_ref as R

pytestmark = pytest.mark.gpu
dev = "cuda"
C, INNER = 320, 1280
DISTINCT = 200      # sites 1 / 2: the rows repeat with this period (no multiple of the tile height: every tile sees another alignment)
SUMMARY = collections.defaultdict(float)     # (build, site, regime, output) -> worst error / bound
FOLD_KERNELS = collections.defaultdict(set)  # build -> consumer kernels that ran


@pytest.fixture(scope="module", params=["fp16", "bf16"])
def half(request):
    """the build of the kernel library under test (this module only; restored on the way out)"""
    from textboost_amd import _lib as L
    prev = L.set_half(request.param)
    try:
        L.lib()
        yield L.half_dtype()
    finally:
        L.set_half(prev)


def _hname(dt):
    return {torch.float16: "fp16", torch.bfloat16: "bf16"}[dt]


def _chk(half, site, regime, what, name, got, ref, bound, info=None):
    w = R.check(f"{name} {what}", got, ref, bound, info)
    key = (_hname(half), site, regime, what)
    SUMMARY[key] = max(SUMMARY[key], w)
    return w


def _operands(regime, variant, rows, Cw, half, offsets=None):
    """(A 16-bit [rows, Cw], bias fp32 [Cw] or None, residual 16-bit [rows, Cw] or None) on the device: their sum is the regime's LayerNorm input"""
    x = R.ln_input(regime, rows, Cw, torch.float32, offsets=offsets)
    if variant == "A":
        return x.to(half).to(dev), None, None
    g = torch.Generator().manual_seed(101 + rows + Cw)
    if regime == "offset":       # the offset in the residual, the fluctuation in A
        offs = offsets or R.LN_OFFSETS
        off = torch.tensor([offs[m % len(offs)] for m in range(rows)]).reshape(rows, 1)
        a, r, bias = (x - off).to(half), off.expand(rows, Cw).to(half).contiguous(), torch.randn(Cw, generator=g) * 0.25
    elif regime == "degenerate":  # halves of the rounded data: the constant rows stay constant
        x16 = x.to(half).float()
        a = (0.5 * x16).to(half)
        r, bias = (x16 - a.float()).to(half), torch.zeros(Cw)
    else:
        a = (0.5 * x).to(half)
        r = (x - a.float()).to(half)
        bias = torch.randn(Cw, generator=g) * 0.25 * {"tiny": 2.0 ** -9, "huge": 2.0 ** 10}.get(regime, 1.0)
    return a.to(dev), bias.to(dev), r.to(dev)


def _check_written(half, site, regime, name, t, a, bias, r):
    """the row the launch wrote against the float64 sum of its operands: acc + bias, + R -- at most 3 fp32 roundings at the magnitude of the terms --
    and half an output ulp"""
    terms = [a.double()] + ([bias.double().expand_as(a)] if bias is not None else []) + ([r.double()] if r is not None else [])
    t64, mag = sum(terms), sum(v.abs() for v in terms)
    ex = 3 * R.U * mag
    _chk(half, site, regime, "written row", name, t, t64, ex + 0.5 * R.ulp(t64.abs() + ex, half))


def _row_info(mean, rstd, period=None):
    def info(i):
        m = i[0] % period if period else i[0]
        return f"row {i[0]}: mean {mean[m].item():.4e} rstd {rstd[m].item():.4e}"
    return info


def _eye(n, half):
    return torch.eye(n, device=dev).to(half)


def _dy_add(rows, Cw, half, seed=5):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(rows, Cw, generator=g).to(half).to(dev), torch.randn(rows, Cw, generator=g).to(half).to(dev)


def _gemm8_tile(L):
    """(rows, columns) of the 8-wave tile of the most recent tb_gemm, or None"""
    c8 = (ctypes.c_int * 6)()
    return (c8[0] * c8[2] * 16, c8[1] * c8[3] * 16) if L.lib().tb_gemm8_last(c8) else None


# ------------------------------------------------------------------------------------------------------------------ sites 1 and 2: the gemm8 epilogue
def _epilogue_rows(ops, half):
    """the smallest M the library takes a LayerNorm epilogue for (64-row tiles) and twice that (128-row tiles); the tile height is confirmed per launch"""
    m64 = next((M for M in range(64, 1 << 16, 64) if ops.gemm_ln_ok(M, C, C, half)), None)
    if m64 is None or not ops.gemm_ln_ok(2 * m64, C, C, half):
        pytest.skip("gemm_ln_ok refuses the LayerNorm epilogue in this build")
    return {64: m64, 128: 2 * m64}


def _run_epilogue(half, tile, regime, variant, eps, launch_eps=None):
    """sites 1 and 2 at one eps.  Returns what the checks need; `launch_eps` (the negative control) hands the kernel another eps than the reference."""
    from textboost_amd import _lib as L, ops
    M = _epilogue_rows(ops, half)[tile]
    assert M % DISTINCT == 0 and DISTINCT % 64 != 0
    reps, sliced = M // DISTINCT, regime in ("offset", "mixed")
    a, bias, r = _operands(regime, variant, DISTINCT, C, half)
    gamma, beta = (t.to(dev) for t in R.ln_params(regime, C))
    dy, add = _dy_add(DISTINCT, C, half)
    big = lambda v: v.repeat(reps, *([1] * (v.dim() - 1)))
    t, tbuf = R.sliced(M, C, half, -3.0, sliced, dev)
    y, ybuf = R.sliced(M, C, half, -3.0, sliced, dev)
    dx, dxbuf = R.sliced(M, C, half, -3.0, sliced, dev)
    dyM, dybuf = R.sliced(M, C, half, 2.0, sliced, dev)
    addM, addbuf = R.sliced(M, C, half, 2.0, sliced, dev)
    dyM.copy_(big(dy)); addM.copy_(big(add))
    stats = torch.full((M, 2), float("nan"), device=dev)
    ops.gemm(big(a), _eye(C, half), t, bias=bias, R=big(r) if r is not None else None, ln_fwd=(gamma, beta, stats, y, launch_eps or eps))
    assert _gemm8_tile(L) == (tile, C), _gemm8_tile(L)
    ops.gemm(dyM, _eye(C, half), dx, R=addM, ln_bwd=(gamma, stats, t))
    assert _gemm8_tile(L) == (tile, C), _gemm8_tile(L)
    torch.cuda.synchronize()
    for buf, fill in ((tbuf, -3.0), (ybuf, -3.0), (dxbuf, -3.0), (dybuf, 2.0), (addbuf, 2.0)):
        assert R.margins_untouched(buf, C, fill), "a margin of the wider buffer was written"
    return dict(M=M, big=big, a=a, bias=bias, r=r, gamma=gamma, beta=beta, dy=dy, add=add, t=t, y=y, dx=dx, stats=stats)


@pytest.mark.parametrize("variant", ["A", "split"])
@pytest.mark.parametrize("regime", R.REGIMES)
@pytest.mark.parametrize("tile", [64, 128])
def test_layernorm_epilogue_forward_and_backward_off_unit_scale(half, tile, regime, variant):
    k = R.k_path("epi", 1, 1, C, 1)
    for eps in R.REGIME_EPS[regime]:
        o = _run_epilogue(half, tile, regime, variant, eps)
        big, t, gamma, beta = o["big"], o["t"], o["gamma"], o["beta"]
        name = f"ln epilogue {_hname(half)} {tile}-row tiles M {o['M']} {variant} {regime} eps {eps:g}"
        t0 = t[:DISTINCT].contiguous()
        assert torch.equal(t.reshape(-1, DISTINCT, C), t0.expand(o["M"] // DISTINCT, DISTINCT, C)), name + ": equal operands, different rows"
        _check_written(half, "1 ln_fwd", regime, name, t0, o["a"], o["bias"], o["r"])
        yr, (mean, rstd), dxr = R.layernorm_ref(t0, gamma, beta, eps, o["dy"], o["add"])
        bound, _, (e_m, e_rstd) = R.layernorm_forward_bound(t0, gamma, beta, eps, k, half, parts=True)
        info = _row_info(mean, rstd, DISTINCT)
        _chk(half, "1 ln_fwd", regime, "y", name, o["y"], big(yr), big(bound), info)
        _chk(half, "1 ln_fwd", regime, "mean", name, o["stats"][:, 0], big(mean), big(e_m.reshape(-1) + 2 * R.U * mean.abs()))
        _chk(half, "1 ln_fwd", regime, "rstd", name, o["stats"][:, 1], big(rstd), big(e_rstd.reshape(-1)))
        bb = R.layernorm_backward_bound(t0, o["dy"], o["add"], gamma, eps, k, half)
        _chk(half, "2 ln_bwd", regime, "dx", name, o["dx"], big(dxr), big(bb), info)


def test_layernorm_epilogue_negative_control_a_wrong_eps_is_rejected(half):
    """the launch gets eps 1e-6 where the reference uses 1e-5, on `tiny` data (row variance ~ 4e-6): the bound must not admit it"""
    k = R.k_path("epi", 1, 1, C, 1)
    o = _run_epilogue(half, 64, "tiny", "A", 1e-5, launch_eps=1e-6)
    t0 = o["t"][:DISTINCT].contiguous()
    yr, _, _ = R.layernorm_ref(t0, o["gamma"], o["beta"], 1e-5)
    with pytest.raises(AssertionError):
        R.check("ln epilogue, eps 1e-6 against the 1e-5 reference", o["y"][:DISTINCT], yr, R.layernorm_forward_bound(t0, o["gamma"], o["beta"], 1e-5, k, half))


# ------------------------------------------------------------------------------------------------------------------ site 4: tb_chain320
def _chain_w2(N2, half, seed=3):
    """the block that copies the normalised row out: I (N2 = 320) or [I; -I; permutation] (960); returns (W2, [(column slice, sign, source columns)])"""
    eye = torch.eye(C)
    if N2 == C:
        return eye.to(half).to(dev), [(slice(0, C), 1.0, torch.arange(C))]
    perm = torch.randperm(C, generator=torch.Generator().manual_seed(seed))
    assert N2 == 3 * C
    return torch.cat([eye, -eye, eye[perm]], 0).to(half).to(dev), [(slice(0, C), 1.0, torch.arange(C)), (slice(C, 2 * C), -1.0, torch.arange(C)),
                                                                     (slice(2 * C, 3 * C), 1.0, perm)]


def _run_chain(half, M, N2, regime, variant, eps, w2, b2=None, launch_eps=None):
    from textboost_amd import ops
    if not ops.chain320_ok(M, N2, half):
        pytest.skip("chain320_ok refuses this build")
    sliced = regime in ("offset", "mixed")
    a, bias, r = _operands(regime, variant, M, C, half)
    gamma, beta = (t.to(dev) for t in R.ln_params(regime, C))
    t, tbuf = R.sliced(M, C, half, -3.0, sliced, dev)
    y, ybuf = R.sliced(M, N2, half, -3.0, sliced, dev)
    stats = torch.full((M, 2), float("nan"), device=dev)
    ops.chain320(a, _eye(C, half), bias, r, t, gamma, beta, stats, w2, b2, y, eps=launch_eps or eps)
    torch.cuda.synchronize()
    assert R.margins_untouched(tbuf, C, -3.0) and R.margins_untouched(ybuf, N2, -3.0), "a margin of the wider buffer was written"
    return dict(a=a, bias=bias, r=r, gamma=gamma, beta=beta, t=t.contiguous(), y=y, stats=stats)


def _check_forward_stats(half, site, regime, name, o, eps, k):
    """the written row, and (mean, rstd) against float64 under e_m / e_rstd; returns (yr, elementwise bound of the normalised row, info)"""
    t, gamma, beta = o["t"], o["gamma"], o["beta"]
    _check_written(half, site, regime, name, t, o["a"], o["bias"], o["r"])
    yr, (mean, rstd), _ = R.layernorm_ref(t, gamma, beta, eps)
    bound, _, (e_m, e_rstd) = R.layernorm_forward_bound(t, gamma, beta, eps, k, half, parts=True)
    _chk(half, site, regime, "mean", name, o["stats"][:, 0], mean, e_m.reshape(-1) + 2 * R.U * mean.abs())
    _chk(half, site, regime, "rstd", name, o["stats"][:, 1], rstd, e_rstd.reshape(-1))
    return yr, bound, _row_info(mean, rstd)


def _composite(yr, bound_ln, W, b, K, half):
    """reference and bound of a product behind the (16-bit rounded) normalised row: sum_k |W_nk| bound_k + K u sum_k |l_k W_nk| (+ the bias add) + half
    an output ulp"""
    Wd = W.double()
    ref = yr @ Wd.T + (b.double() if b is not None else 0.0)
    e = bound_ln @ Wd.abs().T + K * R.U * (yr.abs() @ Wd.abs().T) + 2 * R.U * (ref.abs() + (b.double().abs() if b is not None else 0.0))
    return ref, e + 0.5 * R.ulp(ref.abs() + e, half)


@pytest.mark.parametrize("variant", ["A", "split"])
@pytest.mark.parametrize("regime", R.REGIMES)
@pytest.mark.parametrize("M,N2", [(128, 320), (128, 960), (384, 320), (384, 960)])
def test_chain320_layernorm_off_unit_scale(half, M, N2, regime, variant):
    k = R.k_path("chain", 1, 1, C, 1)
    w2, blocks = _chain_w2(N2, half)
    for eps in R.REGIME_EPS[regime]:
        o = _run_chain(half, M, N2, regime, variant, eps, w2)
        name = f"chain320 {_hname(half)} {M}x{N2} {variant} {regime} eps {eps:g}"
        yr, bound, info = _check_forward_stats(half, "4 chain320", regime, name, o, eps, k)
        for cols, sign, src in blocks:      # Y = the rounded LN(T), up to sign and column order
            _chk(half, "4 chain320", regime, "y", name, o["y"][:, cols], sign * yr[:, src.to(dev)], bound[:, src.to(dev)], info)


@pytest.mark.parametrize("regime", R.REGIMES)
@pytest.mark.parametrize("M,N2", [(128, 320), (384, 960)])
def test_chain320_with_a_random_second_weight_under_the_composite_bound(half, M, N2, regime):
    k = R.k_path("chain", 1, 1, C, 1)
    g = torch.Generator().manual_seed(21)
    w2 = (torch.randn(N2, C, generator=g) / C ** 0.5).to(half).to(dev)
    b2 = (torch.randn(N2, generator=g) * 0.3).to(dev) if N2 == C else None
    eps = R.REGIME_EPS[regime][0]
    o = _run_chain(half, M, N2, regime, "split", eps, w2, b2)
    name = f"chain320 random W2 {_hname(half)} {M}x{N2} {regime} eps {eps:g}"
    yr, bound, info = _check_forward_stats(half, "4 chain320 W2", regime, name, o, eps, k)
    ref, cb = _composite(yr, bound, w2, b2, C, half)
    _chk(half, "4 chain320 W2", regime, "y", name, o["y"], ref, cb, info)


def test_chain320_negative_control_a_wrong_eps_is_rejected(half):
    k = R.k_path("chain", 1, 1, C, 1)
    w2, _ = _chain_w2(C, half)
    o = _run_chain(half, 128, C, "tiny", "A", 1e-5, w2, launch_eps=1e-6)
    yr, _, _ = R.layernorm_ref(o["t"], o["gamma"], o["beta"], 1e-5)
    with pytest.raises(AssertionError):
        R.check("chain320, eps 1e-6 against the 1e-5 reference", o["y"], yr, R.layernorm_forward_bound(o["t"], o["gamma"], o["beta"], 1e-5, k, half))


# ------------------------------------------------------------------------------------------------------------------ sites 5 and 6: tb_ff_fwd (pre), tb_ff_bwd (ln)
def _hcol(j):
    """packed column of h_j in HG / packed row of W1 ([h32 | g32] blocks)"""
    return (j // 32) * 64 + j % 32


def _run_ff_pre(half, M, regime, variant, eps, w1p, b1p):
    from textboost_amd import ops
    if not ops.ff_fused_ok(M, C, INNER, half):
        pytest.skip("ff_fused_ok refuses this build")
    sliced = regime in ("offset", "mixed")
    a, bias, r = _operands(regime, variant, M, C, half)
    gamma, beta = (t.to(dev) for t in R.ln_params(regime, C))
    t, tbuf = R.sliced(M, C, half, -3.0, sliced, dev)
    y, ybuf = R.sliced(M, C, half, -3.0, sliced, dev)
    hg = torch.full((M, 2 * INNER), float("nan"), device=dev, dtype=half)
    w2 = torch.zeros(C, INNER, device=dev, dtype=half)
    stats = torch.full((M, 2), float("nan"), device=dev)
    ops.ff_fwd(a, w1p, b1p, w2, None, hg, y, R=t, pre=(_eye(C, half), bias, r, t, gamma, beta, stats, eps))
    torch.cuda.synchronize()
    assert R.margins_untouched(tbuf, C, -3.0) and R.margins_untouched(ybuf, C, -3.0), "a margin of the wider buffer was written"
    assert torch.equal(y, t), "a zero second weight and no bias: the feed-forward's output is its residual, the written row"
    return dict(a=a, bias=bias, r=r, gamma=gamma, beta=beta, t=t, tc=t.contiguous(), hg=hg, stats=stats)


@pytest.mark.parametrize("variant", ["A", "split"])
@pytest.mark.parametrize("regime", R.REGIMES)
@pytest.mark.parametrize("M", [128, 384])
def test_ff_chained_layernorm_forward_and_backward_off_unit_scale(half, M, regime, variant):
    """site 5: W1 rows chosen so that the 320 packed h columns of the first ten blocks of HG carry the rounded l3 (every other projection is zero);
    site 6: W2^T = [I; 0], h = 0, g = 16 -- gelu(16) = 16 exactly in fp32 (Phi(16) rounds to 1), so dh = 16 dy and, through 2^-4 on the packed h
    rows of W1^T, the gradient entering the LayerNorm backward is dy itself: the launch without `ln` must return dy bit for bit."""
    from textboost_amd import ops
    k, kb = R.k_path("chain", 1, 1, C, 1), R.k_path("ffbwd", 1, 1, C, 1)
    hcols = torch.tensor([_hcol(j) for j in range(C)], device=dev)
    w1p = torch.zeros(2 * INNER, C, device=dev, dtype=half)
    w1p[hcols, torch.arange(C, device=dev)] = 1.0
    w2d = torch.zeros(INNER, C, device=dev, dtype=half)
    w2d[torch.arange(C), torch.arange(C)] = 1.0
    w1d = torch.zeros(C, 2 * INNER, device=dev, dtype=half)
    w1d[torch.arange(C, device=dev), hcols] = 2.0 ** -4
    hg_b = torch.zeros(M, INNER // 32, 2, 32, device=dev, dtype=half)
    hg_b[:, :, 1, :] = 16.0
    hg_b = hg_b.reshape(M, 2 * INNER)
    dy, add = _dy_add(M, C, half)
    plain = torch.full((M, C), float("nan"), device=dev, dtype=half)
    ops.ff_bwd(dy, w2d, w1d, hg_b, plain)
    torch.cuda.synchronize()
    assert torch.equal(plain, dy), "the products around the LayerNorm backward are not exact"
    sliced = regime in ("offset", "mixed")
    for eps in R.REGIME_EPS[regime]:
        o = _run_ff_pre(half, M, regime, variant, eps, w1p, None)
        name = f"ff {_hname(half)} M {M} {variant} {regime} eps {eps:g}"
        yr, bound, info = _check_forward_stats(half, "5 ff_fwd pre", regime, name, dict(o, t=o["tc"]), eps, k)
        hg = o["hg"]
        _chk(half, "5 ff_fwd pre", regime, "l3", name, hg[:, hcols], yr, bound, info)
        rest = torch.ones(2 * INNER, dtype=torch.bool, device=dev)
        rest[hcols] = False
        assert bool((hg[:, rest] == 0).all()), name + ": a projection with a zero weight row is not zero"
        dx, dxbuf = R.sliced(M, C, half, -3.0, sliced, dev)
        ops.ff_bwd(dy, w2d, w1d, hg_b, dx, R=add, ln=(o["t"], o["stats"], o["gamma"]))
        torch.cuda.synchronize()
        assert R.margins_untouched(dxbuf, C, -3.0)
        _, _, dxr = R.layernorm_ref(o["tc"], o["gamma"], None, eps, dy, add)
        bb = R.backward_bound(o["tc"], dy, add, o["gamma"], None, M, 1, C, 1, eps, False, k, kb, half, "meanfirst")
        _chk(half, "6 ff_bwd ln", regime, "dx", name, dx, dxr, bb, info)


@pytest.mark.parametrize("regime", R.REGIMES)
def test_ff_chained_layernorm_with_a_random_projection_under_the_composite_bound(half, regime):
    M, k = 128, R.k_path("chain", 1, 1, C, 1)
    g = torch.Generator().manual_seed(23)
    w1p = (torch.randn(2 * INNER, C, generator=g) / C ** 0.5).to(half).to(dev)
    b1p = (torch.randn(2 * INNER, generator=g) * 0.3).to(dev)
    eps = R.REGIME_EPS[regime][0]
    # (a zero W2 keeps y = t whatever the gate gives)
    o = _run_ff_pre(half, M, regime, "split", eps, w1p, b1p)
    name = f"ff random W1 {_hname(half)} M {M} {regime} eps {eps:g}"
    yr, bound, info = _check_forward_stats(half, "5 ff_fwd pre W1", regime, name, dict(o, t=o["tc"]), eps, k)
    ref, cb = _composite(yr, bound, w1p, b1p, C, half)
    _chk(half, "5 ff_fwd pre W1", regime, "hg", name, o["hg"], ref, cb, info)


# ------------------------------------------------------------------------------------------------------------------ site 3: the folded LayerNorm
_FOLD_ROWS = {}


def _fold_rows(ops, Cw, half):
    """the smallest M that lnfold_slots accepts for width Cw AND whose N = 3C consumer runs on the kernel this width is here to cover (C = 1280: the
    4-wave kernel's copy of the fold, C = 640: the 8-wave kernel's).  Which kernel a shape takes is the dispatch's business, so the accepted M are
    probed in increasing order with a consumer launch on zeros (once per build)."""
    from textboost_amd import _lib as L
    want = {1280: "4-wave", 640: "8-wave"}[Cw]
    key = (_hname(half), Cw)
    if key not in _FOLD_ROWS:
        _FOLD_ROWS[key] = None
        for M in range(64, (1 << 14) + 1, 64):
            slots = ops.lnfold_slots(M, Cw, half)
            if slots <= 0:
                continue
            x, W = torch.zeros(M, Cw, device=dev, dtype=half), torch.zeros(3 * Cw, Cw, device=dev, dtype=half)
            out, rs = torch.empty(M, 3 * Cw, device=dev, dtype=half), torch.zeros(M, 16, 2, device=dev)
            ops.gemm(x, W, out, bias=torch.zeros(3 * Cw, device=dev), lnfold=(rs, slots, torch.zeros(3 * Cw, device=dev), None, 1e-5))
            if _consumer_kernel(L)[0] == want:
                _FOLD_ROWS[key] = (M, slots)
                break
        torch.cuda.synchronize()
    if _FOLD_ROWS[key] is None:
        pytest.skip(f"lnfold_slots accepts no M <= 16384 at C = {Cw} whose consumer takes the {want} kernel in this build")
    return _FOLD_ROWS[key]


def _consumer_kernel(L):
    cfg = (ctypes.c_int * 5)()
    L.lib().tb_gemm_last_config(cfg)
    tile = _gemm8_tile(L)
    return ("8-wave", tile) if tile else ("4-wave", tuple(cfg))


def _run_producer(half, Cw, regime, variant):
    """the residual-stream producer with an identity weight: writes x and the per-tile (sum, sum of squares) slots"""
    from textboost_amd import _lib as L, ops
    M, slots = _fold_rows(ops, Cw, half)
    k = R.k_of(R.fold_stages(Cw, slots))
    sliced = regime in ("offset", "mixed")
    a, bias, r = _operands(regime, variant, M, Cw, half, offsets=R.fold_offsets(k))
    x, xbuf = R.sliced(M, Cw, half, -3.0, sliced, dev)
    rs = torch.full((M, 16, 2), 7.0, device=dev)
    if bias is None:   # the producers of a residual stream always carry a bias and a residual (what lnfold_slots asked the dispatch about): zeros here
        bias, r = torch.zeros(Cw, device=dev), torch.zeros(M, Cw, device=dev, dtype=half)
    ops.gemm(a, _eye(Cw, half), x, bias=bias, R=r, rs_out=rs, rs_slots=slots)
    tile = _gemm8_tile(L)
    torch.cuda.synchronize()
    assert tile is not None and tile[1] == Cw // slots, (tile, slots)
    assert R.margins_untouched(xbuf, Cw, -3.0) and bool((rs[:, slots:] == 7.0).all()), "an unused statistics slot or a margin was written"
    return dict(M=M, slots=slots, k=k, a=a, bias=bias, r=r, x=x, xc=x.contiguous(), rs=rs)


def _check_producer(half, regime, name, p, Cw):
    _check_written(half, "3 fold rs_out", regime, name, p["xc"], p["a"], p["bias"], p["r"])
    slots = p["slots"]
    tw = Cw // slots
    xs = p["xc"].double().reshape(p["M"], slots, tw)
    ks = 7 + tw // 8 - 1     # additions inside one slot: 8 per unit, tw / 8 units
    S, Q = xs.sum(-1), (xs * xs).sum(-1)
    _chk(half, "3 fold rs_out", regime, "slot sum", name, p["rs"][:, :slots, 0], S, ks * R.U * xs.abs().sum(-1) + 1e-300)
    _chk(half, "3 fold rs_out", regime, "slot sumsq", name, p["rs"][:, :slots, 1], Q, (ks + 1) * R.U * Q + 1e-300)


def _check_fold_operands(half, regime, name, W, gamma, beta, b, Wp, c1, c2):
    """what ops.fold_layernorm hands the kernel (the reference takes them as returned, so they are checked on their own): W' is gamma (.) W rounded once,
    c1 the row sums of the ROUNDED W', c2 = b + W beta -- fp32 sums of K terms in any order: K u sum |terms|"""
    K = W.shape[1]
    assert torch.equal(Wp, (W.float() * gamma.float()[None, :]).to(half))
    Wd = Wp.double()
    _chk(half, "3 fold operands", regime, "c1", name, c1, Wd.sum(1), K * R.U * Wd.abs().sum(1))
    t = W.double() * beta.double()[None, :]
    ref = t.sum(1) + (b.double() if b is not None else 0.0)
    _chk(half, "3 fold operands", regime, "c2", name, c2, ref, (K + 1) * R.U * (t.abs().sum(1) + (b.double().abs() if b is not None else 0.0)))


@pytest.mark.parametrize("variant", ["A", "split"])
@pytest.mark.parametrize("regime", R.REGIMES)
@pytest.mark.parametrize("Cw", [1280, 640])
def test_folded_layernorm_off_unit_scale(half, Cw, regime, variant):
    """producer -> consumers N = C (with a bias, so c2 = b + W beta) and N = 3C (without); the N = 3C consumer of C = 1280 runs on the 4-wave kernel's copy of the fold,
    that of C = 640 on the 8-wave kernel's"""
    from textboost_amd import _lib as L, ops
    p = _run_producer(half, Cw, regime, variant)
    M, slots, k, x = p["M"], p["slots"], p["k"], p["x"]
    name = f"fold {_hname(half)} {M}x{Cw} slots {slots} {variant} {regime}"
    _check_producer(half, regime, name, p, Cw)
    gamma, beta = (t.to(dev) for t in R.ln_params(regime, Cw))
    sliced = regime in ("offset", "mixed")
    g = torch.Generator().manual_seed(41)
    for eps in R.REGIME_EPS[regime]:
        for N, full in ((Cw, True), (3 * Cw, False)):
            W = (torch.randn(N, Cw, generator=g) / Cw ** 0.5).to(dev)
            b = (torch.randn(N, generator=g) * 0.3).to(dev) if full else None
            Rres = None
            Wp, c1, c2 = ops.fold_layernorm(W, gamma, beta, b)
            _check_fold_operands(half, regime, f"{name} N {N}", W, gamma, beta, b, Wp, c1, c2)
            out, obuf = R.sliced(M, N, half, -3.0, sliced, dev)
            st = torch.full((M, 2), float("nan"), device=dev)
            ops.gemm(x, Wp, out, bias=c2, R=Rres, lnfold=(p["rs"], slots, c1, st, eps))
            kern = _consumer_kernel(L)
            torch.cuda.synchronize()
            FOLD_KERNELS[_hname(half)].add(kern[0])
            if not full:
                assert kern[0] == {1280: "4-wave", 640: "8-wave"}[Cw], kern
            assert R.margins_untouched(obuf, N, -3.0)
            cname = f"{name} eps {eps:g} consumer N {N} ({kern[0]})"
            ref, (mean, rstd), _ = R.fold_ref(p["xc"], Wp, c1, c2, Rres, eps)
            bound, (e_m, e_rstd) = R.fold_forward_bound(p["xc"], Wp, c1, c2, Rres, eps, k, half, parts=True)
            site = f"3 fold C {Cw}"
            _chk(half, site, regime, f"out N={N // Cw}C", cname, out, ref, bound, _row_info(mean, rstd))
            _chk(half, site, regime, "mean", cname, st[:, 0], mean, e_m + 2 * R.U * mean.abs())
            _chk(half, site, regime, "rstd", cname, st[:, 1], rstd, e_rstd)


@pytest.mark.parametrize("Cw", [1280, 640])
def test_folded_layernorm_into_the_geglu_projection(half, Cw):
    """the GEGLU consumer (N = 8C, packed rows), once per width on `mixed` data: the written pre-gate projections under the fold's bound, the gated
    output against the float64 gate of the WRITTEN projections under tests/act_ref.py's bound"""
    from textboost_amd import _lib as L, ops
    from textboost_amd.unet import pack_geglu_rows
    regime, eps = "mixed", 1e-5
    p = _run_producer(half, Cw, regime, "split")
    M, slots, k = p["M"], p["slots"], p["k"]
    gamma, beta = (t.to(dev) for t in R.ln_params(regime, Cw))
    g = torch.Generator().manual_seed(43)
    W = pack_geglu_rows(torch.randn(8 * Cw, Cw, generator=g) / Cw ** 0.5).to(dev)
    b = pack_geglu_rows(torch.randn(8 * Cw, generator=g) * 0.3).to(dev)
    Wp, c1, c2 = ops.fold_layernorm(W, gamma, beta, b)
    gated = torch.full((M, 4 * Cw), float("nan"), device=dev, dtype=half)
    raw = torch.full((M, 8 * Cw), float("nan"), device=dev, dtype=half)
    st = torch.full((M, 2), float("nan"), device=dev)
    ops.gemm(p["x"], Wp, gated, bias=c2, act=L.ACT_GEGLU, C2=raw, lnfold=(p["rs"], slots, c1, st, eps))
    kern = _consumer_kernel(L)
    torch.cuda.synchronize()
    FOLD_KERNELS[_hname(half)].add(kern[0])
    name = f"fold {_hname(half)} {M}x{Cw} GEGLU consumer ({kern[0]})"
    ref, (mean, rstd), _ = R.fold_ref(p["xc"], Wp, c1, c2, None, eps)
    bound, (e_m, e_rstd) = R.fold_forward_bound(p["xc"], Wp, c1, c2, None, eps, k, half, parts=True)
    site = f"3 fold C {Cw}"
    _chk(half, site, regime, "geglu raw", name, raw, ref, bound, _row_info(mean, rstd))
    _chk(half, site, regime, "rstd", name, st[:, 1], rstd, e_rstd)
    rb = raw.reshape(M, 8 * Cw // 64, 2, 32)
    hh, gg = rb[:, :, 0].reshape(M, 4 * Cw), rb[:, :, 1].reshape(M, 4 * Cw)
    gref, ge = A.geglu(hh, gg)
    _chk(half, site, regime, "geglu gated", name, gated, gref, A.bound(gref, ge, half))


def test_folded_layernorm_negative_control_a_wrong_eps_is_rejected(half):
    from textboost_amd import ops
    Cw = 1280
    p = _run_producer(half, Cw, "tiny", "A")
    gamma, beta = (t.to(dev) for t in R.ln_params("tiny", Cw))
    W = (torch.randn(Cw, Cw, generator=torch.Generator().manual_seed(41)) / Cw ** 0.5).to(dev)
    Wp, c1, c2 = ops.fold_layernorm(W, gamma, beta, None)
    out = torch.full((p["M"], Cw), float("nan"), device=dev, dtype=half)
    st = torch.full((p["M"], 2), float("nan"), device=dev)
    ops.gemm(p["x"], Wp, out, bias=c2, lnfold=(p["rs"], p["slots"], c1, st, 1e-6))
    torch.cuda.synchronize()
    ref, _, _ = R.fold_ref(p["xc"], Wp, c1, c2, None, 1e-5)
    with pytest.raises(AssertionError):
        R.check("fold, eps 1e-6 against the 1e-5 reference", out, ref, R.fold_forward_bound(p["xc"], Wp, c1, c2, None, 1e-5, p["k"], half))


# ------------------------------------------------------------------------------------------------------------------ summary
def test_summary_of_the_worst_error_over_bound(half, capsys):
    """prints what the cases of this build recorded, past the capture: one line per (build, site, regime, output); and that both copies of the fold's
    consumer ran"""
    hname = _hname(half)
    assert any(k[0] == hname for k in SUMMARY), "no case of this build has run before its summary"
    with capsys.disabled():
        print(f"\n[norm-bound] k per path at C = {C}: epi {R.k_path('epi', 1, 1, C, 1)}, chain {R.k_path('chain', 1, 1, C, 1)}, "
              f"ffbwd {R.k_path('ffbwd', 1, 1, C, 1)}; fold consumer kernels that ran: {sorted(FOLD_KERNELS[hname])}")
        print("[norm-bound] worst error / bound per (build, site, regime, output):")
        for key in sorted(k for k in SUMMARY if k[0] == hname):
            print("[norm-bound]   " + " ".join(f"{k:<16s}" for k in key) + f" {SUMMARY[key]:.3f}")
    if FOLD_KERNELS[hname]:
        assert FOLD_KERNELS[hname] == {"4-wave", "8-wave"}, FOLD_KERNELS[hname]
