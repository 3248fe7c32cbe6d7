"""tests/norm_ref.py on the host: the float64 references against torch.nn.functional + autograd, the bound against fp32 models of every formula
(it must contain them: not too tight) and against a list of numpy mutants (each must be rejected somewhere: not vacuous), and the cap that
chooses the offsets.  Prints the mutant x regime table, and shows that the data of the existing tests (randn * 2 + 0.5, rel-L2 tolerances) admits
the eps and shift-after-rounding mutants."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import norm_ref as R
from parity import parity

F32 = np.float32


# ------------------------------------------------------------------------------------------------------------------ references vs torch
@pytest.mark.parametrize("silu", [False, True])
def test_groupnorm_ref_matches_functional_and_autograd(silu):
    B, HW, C, G, eps = 2, 9, 48, 4, 1e-5
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(B * HW, C, generator=g, dtype=torch.float64) * 2 + 3).requires_grad_(True)
    gamma, beta = torch.randn(C, generator=g, dtype=torch.float64), torch.randn(C, generator=g, dtype=torch.float64)
    dy, add = torch.randn(B * HW, C, generator=g, dtype=torch.float64), torch.randn(B * HW, C, generator=g, dtype=torch.float64)
    y, (mean, rstd), dx = R.groupnorm_ref(x.detach(), gamma, beta, B, HW, C, G, eps, silu, dy, add)
    t = F.group_norm(x.view(B, HW, C).permute(0, 2, 1), G, gamma, beta, eps)
    t = F.silu(t) if silu else t
    t.backward(dy.view(B, HW, C).permute(0, 2, 1))
    torch.testing.assert_close(y, t.permute(0, 2, 1).reshape(B * HW, C), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(dx, x.grad + add, rtol=1e-11, atol=1e-12)
    xg = x.detach().view(B, HW, G, C // G)
    torch.testing.assert_close(mean, xg.mean((1, 3)), rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(rstd, (xg.var((1, 3), unbiased=False) + eps).rsqrt(), rtol=1e-12, atol=0)


def test_layernorm_ref_matches_functional_and_autograd():
    M, C, eps = 7, 40, 1e-6
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(M, C, generator=g, dtype=torch.float64) - 5).requires_grad_(True)
    gamma, beta = torch.randn(C, generator=g, dtype=torch.float64), torch.randn(C, generator=g, dtype=torch.float64)
    dy, add = torch.randn(M, C, generator=g, dtype=torch.float64), torch.randn(M, C, generator=g, dtype=torch.float64)
    y, (mean, rstd), dx = R.layernorm_ref(x.detach(), gamma, beta, eps, dy, add)
    t = F.layer_norm(x, (C,), gamma, beta, eps)
    t.backward(dy)
    torch.testing.assert_close(y, t, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(dx, x.grad + add, rtol=1e-11, atol=1e-12)
    torch.testing.assert_close(mean, x.detach().mean(1), rtol=1e-13, atol=1e-13)


def test_ulp_is_the_spacing_of_the_format():
    v = torch.tensor([1.0, 1.999, 2.0, 0.3, 1e-7, 0.0, 300.0], dtype=torch.float64)
    assert R.ulp(v, torch.float16).tolist() == [2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 2.0 ** -12, 2.0 ** -24, 2.0 ** -24, 2.0 ** -2]
    assert R.ulp(v, torch.bfloat16)[:4].tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -9]
    for dt in (torch.float16, torch.bfloat16):   # against the format itself
        w = torch.tensor([0.37, 5.5, 130.0]).to(dt)
        nxt = torch.nextafter(w, torch.full_like(w, float("inf")))
        assert torch.equal((nxt.double() - w.double()), R.ulp(w.double(), dt))


def test_case_table_takes_the_paths_it_names():
    for c in R.GN_CASES:
        if c.f32 or c.splitk:
            continue
        variant = 11 if c.variant is None else c.variant
        assert R.gn_path(c.B, c.HW, c.C, c.G, False, variant) == c.path, c.id
        assert R.gn_path(c.B, c.HW, c.C, c.G, True, variant) == (c.bwd_path or "twopass"), c.id
        st = R.path_stages(c.path, c.B, c.HW, c.C, c.G)
        assert int(np.prod(st)) >= c.HW * (c.C // c.G), (c.id, st)      # the stages cover the group
    c = [c for c in R.GN_CASES if c.splitk][0]
    assert R.gn_path(c.B, c.HW, c.C, c.G) == "fused"                    # the split-K consumer is the fused kernel
    assert R.gn_path(4, 641, 1024, 32) != "fused" and R.gn_path(4, 640, 1024, 32) == "fused"


# ------------------------------------------------------------------------------------------------------------------ fp32 models
def rnd(a, dtype):
    """round an fp32 numpy array to `dtype` (a torch dtype) and back"""
    if dtype == torch.float32:
        return a.astype(F32)
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F32)).to(dtype).float().numpy()


def staged_sum(v, stages):
    """fp32 sum over the last axis in the order of `stages` (norm_ref.path_stages): every stage a strictly sequential sum (np.cumsum)"""
    n, tot = v.shape[-1], int(np.prod(stages))
    assert tot >= n, (n, stages)
    if tot > n:
        v = np.concatenate([v, np.zeros(v.shape[:-1] + (tot - n,), F32)], axis=-1)
    for s in stages:
        v = np.cumsum(v.reshape(v.shape[:-1] + (-1, s)), axis=-1, dtype=F32)[..., -1]
    return v[..., 0]


def seq_sum_rounded(v, dtype):
    """sequential sum over the last axis, the accumulator rounded to `dtype` after every addition (a mutant)"""
    acc = np.zeros(v.shape[:-1], F32)
    for j in range(v.shape[-1]):
        acc = rnd(acc + v[..., j], dtype)
    return acc


def _silu(z):
    with np.errstate(over="ignore"):
        return (z / (F32(1) + np.exp(-z, dtype=F32))).astype(F32)


def _silu_grad(z):
    with np.errstate(over="ignore", invalid="ignore"):
        s = (F32(1) / (F32(1) + np.exp(-z, dtype=F32))).astype(F32)
        return (s * (F32(1) + z * (F32(1) - s))).astype(F32)


def model(x, gamma, beta, B, HW, C, G, eps, silu, stages, form, half, out_dtype, mut=None, dy=None, add=None, slices=None):
    """fp32 numpy model of GroupNorm(+SiLU) forward (+ backward): form 'onepass' (var = Q/n - mean^2, z = x sc + (beta - mean sc)) or 'meanfirst'
    (centred variance, z = (x - mean) rstd gamma + beta; LayerNorm = one group per row).  `mut` names a mutant.  Returns (y, dx) as float64 tensors of
    the rounded outputs."""
    gs = C // G
    n = HW * gs
    X = x.float().numpy().reshape(B, HW, G, gs)
    ga, be = gamma.float().numpy().reshape(1, 1, G, gs), beta.float().numpy().reshape(1, 1, G, gs)
    xg = np.ascontiguousarray(X.transpose(0, 2, 1, 3)).reshape(B, G, n)
    eps_k = eps
    if mut == "eps dropped":
        eps_k = 0.0
    elif mut == "eps 1e-5 for 1e-6" and eps == 1e-6:
        eps_k = 1e-5
    elif mut == "eps 1e-6 for 1e-5" and eps == 1e-5:
        eps_k = 1e-6
    nf = F32((HW - 1) * gs) if mut == "n short by one row" else F32(n)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        S = seq_sum_rounded(xg, half) if mut == "sum of x in 16 bits" else staged_sum(xg, stages)
        mean = (S / nf).astype(F32)
        if mut == "mean in 16 bits":
            mean = rnd(mean, half)
        if form == "onepass":
            if mut == "split-K slices squared before they are added":
                sq = sum((s.float().numpy().reshape(B, HW, G, gs) ** 2).astype(F32) for s in slices)
                sq = np.ascontiguousarray(sq.transpose(0, 2, 1, 3)).reshape(B, G, n)
            else:
                sq = (xg * xg).astype(F32)
            Q = seq_sum_rounded(sq, half) if mut == "sum of x*x in 16 bits" else staged_sum(sq, stages)
            var = (Q / nf - mean * mean).astype(F32)
            if mut != "variance not clamped":
                var = np.maximum(var, F32(0))
        else:
            dlt = (xg - mean[..., None]).astype(F32)
            var = (staged_sum((dlt * dlt).astype(F32), stages) / nf).astype(F32)
        if mut == "unbiased variance":
            var = (var * F32(n) / F32(n - 1)).astype(F32)
        rstd = (F32(1) / np.sqrt((var + F32(eps_k)).astype(F32))).astype(F32)
        if mut == "statistics of group g^1":
            idx = np.arange(G) ^ 1
            mean, rstd = mean[:, idx], rstd[:, idx]
        if mut == "statistics of image b^1" and B > 1:
            idx = np.minimum(np.arange(B) ^ 1, B - 1)
            mean, rstd = mean[idx], rstd[idx]
        mu, rs = mean.reshape(B, 1, G, 1), rstd.reshape(B, 1, G, 1)
        if form == "onepass":
            sc = (rs * ga).astype(F32)
            sh = (be - (mu * sc).astype(F32)).astype(F32)
            xs = (X * sc).astype(F32)
            if mut == "x*sc in 16 bits before the shift":
                xs = rnd(xs, half)
            z = (xs + sh).astype(F32)
        else:
            z = ((((X - mu).astype(F32) * rs).astype(F32) * ga).astype(F32) + be).astype(F32)
        y = _silu(z) if silu else z
        yo = torch.from_numpy(rnd(y, out_dtype).reshape(B * HW, C)).double()
        if dy is None:
            return yo, None
        xh = ((X - mu).astype(F32) * rs).astype(F32)
        d = dy.float().numpy().reshape(B, HW, G, gs)
        if silu and mut != "silu' replaced by 1":
            d = (d * _silu_grad(((xh * ga).astype(F32) + be).astype(F32))).astype(F32)
        d = (d * ga).astype(F32)
        grp = lambda t: np.ascontiguousarray(t.transpose(0, 2, 1, 3)).reshape(B, G, n)
        m1 = (staged_sum(grp(d), stages) / F32(n)).astype(F32).reshape(B, 1, G, 1)
        m2 = (staged_sum(grp((d * xh).astype(F32)), stages) / F32(n)).astype(F32).reshape(B, 1, G, 1)
        dx = (rs * ((d - m1).astype(F32) - (xh * m2).astype(F32)).astype(F32)).astype(F32)
        if add is not None:
            dx = (dx + add.float().numpy().reshape(B, HW, G, gs)).astype(F32)
        return yo, torch.from_numpy(rnd(dx, out_dtype).reshape(B * HW, C)).double()


def _gn_data(case, regime, half, with_bwd=True):
    dt = torch.float32 if case.f32 else half
    x = R.gn_input(regime, case.B, case.HW, case.C, case.G, dt, case.ratio)
    gamma, beta = R.gn_params(regime, case.C)
    g = torch.Generator().manual_seed(23)
    dy = torch.randn(x.shape, generator=g).to(dt) if with_bwd else None
    add = torch.randn(x.shape, generator=g).to(dt) if with_bwd else None
    return x, gamma, beta, dy, add


def _group_info(case, mean, rstd):
    def info(idx):
        b, g = idx[0] // case.HW, idx[1] // (case.C // case.G)
        return f"image {b} group {g}: mean {mean[b, g].item():.4e} rstd {rstd[b, g].item():.4e}"
    return info


def _check_model_case(case, regime, eps, half, silu, mut=None, bwd=True, verbose=False):
    """run the model (or a mutant) of the case's formula on the regime's data and check() it against the float64 reference under the bound"""
    dt = torch.float32 if case.f32 else half
    x, gamma, beta, dy, add = _gn_data(case, regime, half, bwd and case.bwd_path is not None)
    a = (case.B, case.HW, case.C, case.G)
    stages = R.path_stages(case.path, *a)
    y, dx = model(x, gamma, beta, *a, eps, silu, stages, case.form, half, dt, mut, dy, add)
    yr, (mean, rstd), dxr = R.groupnorm_ref(x, gamma, beta, *a, eps, silu, dy, add)
    info = _group_info(case, mean, rstd)
    name = f"model {case.id} {regime} eps {eps:g}{' silu' if silu else ''}{' [' + mut + ']' if mut else ''}"
    w = R.check(name + " y", y, yr, R.forward_bound(x, gamma, beta, *a, eps, silu, case.k, dt, case.form), info, verbose)
    if dx is not None:
        w = max(w, R.check(name + " dx", dx, dxr, R.backward_bound(x, dy, add, gamma, beta, *a, eps, silu, case.k, case.kb, dt, case.form), info, verbose))
    return w


HOST_CASES = [c for c in R.GN_CASES if not c.splitk and c.HW * c.C <= 600 * 1280]     # (the two largest maps: the same slice formula as 576 x 1280)


@pytest.mark.parametrize("case", HOST_CASES, ids=lambda c: c.id)
def test_fp32_models_stay_inside_the_bound(case):
    """the arithmetic inside the bound: an fp32 model of the case's formula, summed in the order of its path with every stage strictly sequential,
    on every regime; forward and backward, with and without SiLU"""
    worst = 0.0
    for regime in R.REGIMES + (() if case.f32 else R.ENVELOPE):
        for eps in R.REGIME_EPS[regime]:
            for half in ((torch.float16,) if case.f32 or case.HW * case.C > 70000 else (torch.float16, torch.bfloat16)):
                w = _check_model_case(case, regime, eps, half, silu=regime != "tiny" or eps == 1e-5)
                worst = max(worst, w)
    print(f"[norm-bound] {case.id}: k = {case.k}, offset ratio {case.ratio}, worst model error / bound {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("M,C", R.LN_CASES)
def test_layernorm_model_stays_inside_the_bound(M, C):
    k = R.k_path("ln", M, 1, C, 1)
    stages = R.path_stages("ln", M, 1, C, 1)
    for regime in R.REGIMES:
        for eps in R.REGIME_EPS[regime]:
            for xk, yk in R.LN_DTYPES:
                for half in (torch.float16, torch.bfloat16):
                    xdt, ydt = (torch.float32 if xk == "f32" else half), (torch.float32 if yk == "f32" else half)
                    x = R.ln_input(regime, M, C, xdt)
                    gamma, beta = R.ln_params(regime, C)
                    g = torch.Generator().manual_seed(5)
                    dy, add = torch.randn(M, C, generator=g).to(ydt), torch.randn(M, C, generator=g).to(xdt)
                    y, _ = model(x, gamma, beta, M, 1, C, 1, eps, False, stages, "meanfirst", half, ydt)
                    _, dx = model(x, gamma, beta, M, 1, C, 1, eps, False, stages, "meanfirst", half, xdt, None, dy, add)
                    yr, (mean, rstd), dxr = R.layernorm_ref(x, gamma, beta, eps, dy, add)
                    info = lambda i: f"row {i[0]}: mean {mean[i[0]].item():.4e} rstd {rstd[i[0]].item():.4e}"
                    name = f"model layernorm {M}x{C} {regime} eps {eps:g} {xk}->{yk} {half}"
                    R.check(name + " y", y, yr, R.layernorm_forward_bound(x, gamma, beta, eps, k, ydt), info, verbose=False)
                    R.check(name + " dx", dx, dxr, R.layernorm_backward_bound(x, dy, add, gamma, eps, k, xdt), info, verbose=False)


# ------------------------------------------------------------------------------------------------------------------ mutants
MUTANTS = ["eps dropped", "eps 1e-5 for 1e-6", "eps 1e-6 for 1e-5", "sum of x in 16 bits", "sum of x*x in 16 bits",
           "x*sc in 16 bits before the shift", "mean in 16 bits", "n short by one row", "unbiased variance", "statistics of group g^1",
           "statistics of image b^1", "variance not clamped", "silu' replaced by 1", "split-K slices squared before they are added"]
MUTANT_CASES = [R.GN_CASES[0], R.GN_CASES[4]]     # two-pass 2 x 100 x 64 (200 elements per group) and fused 4 x 64 x 256 (512)


def _splitk_rejected(regime, eps):
    c = [c for c in R.GN_CASES if c.splitk][0]
    a = (c.B, c.HW, c.C, c.G)
    target = R.gn_input(regime, *a, torch.float32, c.ratio)
    gamma, beta = R.gn_params(regime, c.C)
    sk = R.splitk_operands(target, c.B, torch.float16)
    x = R.splitk_written_x(sk, c.B, torch.float16)
    stages = R.path_stages("splitk", *a)
    yr, _, _ = R.groupnorm_ref(x, gamma, beta, *a, eps, True)
    bound = R.forward_bound(x, gamma, beta, *a, eps, True, c.k, torch.float16, "onepass")
    out = []
    for mut in (None, "split-K slices squared before they are added"):
        y, _ = model(x, gamma, beta, *a, eps, True, stages, "onepass", torch.float16, torch.float16, mut, slices=sk["slices"])
        try:
            R.check(f"split-K model {regime} [{mut}]", y, yr, bound, verbose=False)
            out.append(False)
        except AssertionError:
            out.append(True)
    assert out[0] is False, "the unmutated split-K model left the bound"
    return out[1]


def test_every_mutant_is_rejected_by_some_regime_and_unit_scale_data_admits_the_named_ones(capsys):
    lines = []
    say = lines.append     # printed past the capture below: the table belongs in the output of a plain run
    table = {m: [] for m in MUTANTS}
    for regime in R.REGIMES:
        for eps in R.REGIME_EPS[regime]:
            for case in MUTANT_CASES:
                for mut in MUTANTS[:-1]:
                    try:
                        _check_model_case(case, regime, eps, torch.float16, silu=True, mut=mut)
                    except AssertionError:
                        table[mut].append(f"{regime}/{eps:g}/{case.path}")
            if _splitk_rejected(regime, eps):
                table[MUTANTS[-1]].append(f"{regime}/{eps:g}/splitk")
    say("")
    say("[mutants] rejected by (regime/eps/path):")
    for mut in MUTANTS:
        say(f"[mutants]   {mut:46s} {', '.join(table[mut]) or '-- NOWHERE --'}")
    with capsys.disabled():
        print("\n".join(lines))
    lines.clear()
    missing = [m for m in MUTANTS if not table[m]]
    assert not missing, f"no regime rejects: {missing}"

    # the data and tolerances of tests/test_gpu_norm_attn.py::test_groupnorm_fwd_bwd (randn * 2 + 0.5; rel-L2 2e-3, max-abs 3e-3, channel 3e-3; backward
    # 3e-3 / 4e-3 / 4e-3) on one of its shapes: which mutants does it let through?
    B, HW, C, G, eps = 2, 256, 320, 32, 1e-5
    a = (B, HW, C, G)
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(B * HW, C, generator=g) * 2 + 0.5).half()
    gamma, beta = torch.randn(C, generator=g) * 0.5 + 1, torch.randn(C, generator=g) * 0.3
    dy, add = torch.randn(B * HW, C, generator=g).half(), torch.randn(B * HW, C, generator=g).half()
    yr, _, dxr = R.groupnorm_ref(x, gamma, beta, *a, eps, True, dy, add)
    stages = R.path_stages("twopass", *a)
    admitted = []
    for mut in [None] + MUTANTS[:-1]:
        if mut in ("sum of x in 16 bits", "sum of x*x in 16 bits"):
            continue    # (5120 sequential rounded additions per group: rejected by anything; not worth the loop)
        y, dx = model(x, gamma, beta, *a, eps, True, stages, "onepass", torch.float16, torch.float16, "eps 1e-6 for 1e-5" if mut == "eps 1e-5 for 1e-6" else mut,
                      dy, add)
        try:
            parity(f"unit scale [{mut}] fwd", y.view(B, HW, C), yr.view(B, HW, C), rel=2e-3, maxabs=3e-3, ch_dim=2, ch_rel=3e-3, verbose=False)
            parity(f"unit scale [{mut}] bwd", dx, dxr, rel=3e-3, maxabs=4e-3, ch_dim=1, ch_rel=4e-3, verbose=False)
            admitted.append(mut)
        except AssertionError:
            pass
    say(f"[mutants] admitted by the unit-scale data (randn * 2 + 0.5) under the rel-L2 tolerances: {admitted}")
    with capsys.disabled():
        print("\n".join(lines))
    assert None in admitted
    for m in ("eps dropped", "eps 1e-5 for 1e-6", "eps 1e-6 for 1e-5", "x*sc in 16 bits before the shift"):
        assert m in admitted, m


# ------------------------------------------------------------------------------------------------------------------ the cap
@pytest.mark.parametrize("case", [c for c in R.GN_CASES if not c.f32 and not c.splitk and c.HW * c.C <= 600 * 1280], ids=lambda c: c.id)
def test_statistics_term_stays_within_two_output_ulps(case):
    """A condition on the table, not a measurement: in every regime but the envelope the statistics term of the forward bound, at the element where it is
    largest, is within 2 ulps of the 16-bit output.  The ulp is taken at the normalised-and-affine value z there: that is what the statistics perturb,
    and after SiLU a negative z leaves |y| << |z|, whose ulp says nothing about the conditioning.  The offset ratio is the largest power of two <= 32
    that norm_ref.offset_ratio admits for the path's k."""
    a = (case.B, case.HW, case.C, case.G)
    assert case.ratio in (2, 4, 8, 16, 32)
    if case.ratio < 32:
        k, r2 = case.k, 2 * case.ratio
        assert 0.5 * k * R.U * (3 * r2 * r2 + 1) + k * R.U * (r2 + 0.8) / 4.0 > 2.0 ** -10     # the next power of two breaks the cap
    for regime in R.REGIMES:
        eps = R.REGIME_EPS[regime][0]
        for half in (torch.float16, torch.bfloat16):
            x = R.gn_input(regime, *a, half, case.ratio)
            gamma, beta = R.gn_params(regime, case.C)
            _, t_stat, _ = R.forward_bound(x, gamma, beta, *a, eps, False, case.k, half, "onepass", parts=True)
            z, _, _ = R.groupnorm_ref(x, gamma, beta, *a, eps, False)
            # the constant groups of `degenerate` are exempt: there xhat = (x - mean) / sqrt(eps), an error of the mean is magnified by 1000 whatever
            # the offset, and no choice of data keeps the term small (their sums are exact or near it; the bound there stays the worst case)
            X = x.double().view(case.B, case.HW, case.G, -1)
            const = (X.amax((1, 3), keepdim=True) == X.amin((1, 3), keepdim=True)).expand_as(X).reshape(t_stat.shape)
            t_stat = torch.where(const, torch.zeros_like(t_stat), t_stat)
            i = int(t_stat.argmax())
            ts, zz = t_stat.reshape(-1)[i].item(), z.reshape(-1)[i]
            assert ts <= 2 * R.ulp(zz, half).item(), (case.id, regime, half, ts, zz.item())


# ------------------------------------------------------------------------------------------------------------------ the LayerNorms fused into other launches
FUSED_PATHS = ("epi", "chain")     # norm_ref.path_stages: the gemm8 LN_FWD / LN_BWD epilogue, the ff / chain320 stage
FUSED_C, FUSED_M, FUSED_TILE = 320, 130, 64
FUSED_MUTANTS = ["statistics of the un-rounded fp32 row", "statistics of row m^1", "statistics of row m + tile height", "LN_BWD with mean(g xhat) dropped"]


def _fused_operands(regime, half, M=FUSED_M, C=FUSED_C):
    """the fp32 row an epilogue holds before it rounds it (a sum of three operands: not representable in 16 bits), its LayerNorm parameters, dy, add"""
    t32 = R.ln_input(regime, M, C, torch.float32)
    gamma, beta = R.ln_params(regime, C)
    g = torch.Generator().manual_seed(5)
    dy, add = torch.randn(M, C, generator=g).to(half), torch.randn(M, C, generator=g).to(half)
    return t32, gamma, beta, dy, add


def fused_model(t32, gamma, beta, eps, stages, half, dy, add, mut=None):
    """fp32 numpy model of sites 1 / 4 / 5 (forward) and 2 / 6 (backward): the row is rounded to the 16-bit type FIRST, the statistics are those of the
    rounded row (mean, then centred squares, summed in the order of `stages`), y = (o - mean) rstd gamma + beta rounded; the backward reads o and the
    forward's (mean, rstd): dx = rstd (g - mean g - xhat mean(g xhat)) + add, g = dy gamma.  Returns (o, y, dx) as torch tensors (o in `half`)."""
    M, C = t32.shape
    T = t32.numpy().astype(F32)
    o = rnd(T, half)
    ga, be = gamma.numpy().astype(F32), beta.numpy().astype(F32)
    src = T if mut == "statistics of the un-rounded fp32 row" else o
    n = F32(C)
    mean = (staged_sum(src, stages) / n).astype(F32)
    dl = (src - mean[:, None]).astype(F32)
    var = (staged_sum((dl * dl).astype(F32), stages) / n).astype(F32)
    rstd = (F32(1) / np.sqrt((var + F32(eps)).astype(F32))).astype(F32)
    if mut == "statistics of row m^1":
        idx = np.minimum(np.arange(M) ^ 1, M - 1)
        mean, rstd = mean[idx], rstd[idx]
    if mut == "statistics of row m + tile height":
        idx = (np.arange(M) + FUSED_TILE) % M
        mean, rstd = mean[idx], rstd[idx]
    mu, rs = mean[:, None], rstd[:, None]
    xh = ((o - mu).astype(F32) * rs).astype(F32)
    y = ((xh * ga).astype(F32) + be).astype(F32)
    g = (dy.float().numpy() * ga).astype(F32)
    m1 = (staged_sum(g, stages) / n).astype(F32)[:, None]
    m2 = (staged_sum((g * xh).astype(F32), stages) / n).astype(F32)[:, None]
    if mut == "LN_BWD with mean(g xhat) dropped":
        m2 = np.zeros_like(m2)
    dx = ((rs * ((g - m1).astype(F32) - (xh * m2).astype(F32)).astype(F32)).astype(F32) + add.float().numpy()).astype(F32)
    tt = lambda a: torch.from_numpy(rnd(a, half)).double()
    return torch.from_numpy(o).to(half), tt(y), tt(dx)


def _check_fused_model(path, regime, eps, half, mut=None):
    t32, gamma, beta, dy, add = _fused_operands(regime, half)
    stages = R.path_stages(path, FUSED_M, 1, FUSED_C, 1)
    k = R.k_of(stages)
    o, y, dx = fused_model(t32, gamma, beta, eps, stages, half, dy, add, mut)
    yr, _, dxr = R.layernorm_ref(o, gamma, beta, eps, dy, add)
    name = f"model fused {path} {regime} eps {eps:g} {half}{' [' + mut + ']' if mut else ''}"
    w = R.check(name + " y", y, yr, R.layernorm_forward_bound(o, gamma, beta, eps, k, half), verbose=False)
    return max(w, R.check(name + " dx", dx, dxr, R.layernorm_backward_bound(o, dy, add, gamma, eps, k, half), verbose=False))


@pytest.mark.parametrize("path", FUSED_PATHS)
def test_fused_layernorm_models_stay_inside_the_bound(path):
    assert int(np.prod(R.path_stages(path, 1, 1, FUSED_C, 1))) >= FUSED_C
    worst = 0.0
    for regime in R.REGIMES:
        for eps in R.REGIME_EPS[regime]:
            for half in (torch.float16, torch.bfloat16):
                worst = max(worst, _check_fused_model(path, regime, eps, half))
    print(f"[norm-bound] fused path {path}: stages {R.path_stages(path, 1, 1, FUSED_C, 1)}, k = {R.k_path(path, 1, 1, FUSED_C, 1)}, "
          f"offsets |mean| / std {R.LN_OFFSETS}, worst model error / bound {worst:.3f}")
    assert worst <= 1.0


def test_every_fused_site_mutant_is_rejected_by_some_regime(capsys):
    table = {m: [] for m in FUSED_MUTANTS}
    for regime in R.REGIMES:
        for eps in R.REGIME_EPS[regime]:
            for path in FUSED_PATHS:
                for mut in FUSED_MUTANTS:
                    try:
                        _check_fused_model(path, regime, eps, torch.float16, mut)
                    except AssertionError:
                        table[mut].append(f"{regime}/{eps:g}/{path}")
    with capsys.disabled():
        print("\n[mutants] fused LayerNorm sites, rejected by (regime/eps/path):")
        for mut in FUSED_MUTANTS:
            print(f"[mutants]   {mut:46s} {', '.join(table[mut]) or '-- NOWHERE --'}")
    missing = [m for m in FUSED_MUTANTS if not table[m]]
    assert not missing, f"no regime rejects: {missing}"


@pytest.mark.parametrize("path", FUSED_PATHS)
def test_statistics_term_of_the_fused_paths_stays_within_two_output_ulps(path):
    """the cap of test_statistics_term_stays_within_two_output_ulps as a checked condition for the mean-first paths of the fused sites, on the LayerNorm
    regimes (|mean| / std up to 256): the statistics term at the element where it is largest is within 2 ulps of the 16-bit output there"""
    M, C = FUSED_M, FUSED_C
    k = R.k_path(path, M, 1, C, 1)
    for regime in R.REGIMES:
        eps = R.REGIME_EPS[regime][0]
        for half in (torch.float16, torch.bfloat16):
            x = R.ln_input(regime, M, C, half)
            gamma, beta = R.ln_params(regime, C)
            _, t_stat, _ = R.layernorm_forward_bound(x, gamma, beta, eps, k, half, parts=True)
            z, _, _ = R.layernorm_ref(x, gamma, beta, eps)
            X = x.double()
            const = (X.amax(1, keepdim=True) == X.amin(1, keepdim=True)).expand_as(X)     # (the constant rows of `degenerate`: exempt as above)
            t_stat = torch.where(const, torch.zeros_like(t_stat), t_stat)
            i = int(t_stat.argmax())
            ts, zz = t_stat.reshape(-1)[i].item(), z.reshape(-1)[i]
            assert ts <= 2 * R.ulp(zz, half).item(), (path, regime, half, ts, zz.item())


# ------------------------------------------------------------------------------------------------------------------ the folded LayerNorm (site 3)
FOLD_MUTANTS = ["c1 summed from the un-rounded gamma W", "mean c1 term dropped", "c2 without W beta", "a slot too few summed", "fold: statistics of row m^1",
                "fold: eps dropped"]
FOLD_CASES = [(320, 4), (640, 4), (1280, 16)]     # (C, slots): 80-, 160- and 80-column producer tiles


def _fold_data(regime, Cw, slots, half, M=24, N=48):
    k = R.k_of(R.fold_stages(Cw, slots))
    x = R.ln_input(regime, M, Cw, half, offsets=R.fold_offsets(k))
    gamma, beta = R.ln_params(regime, Cw)
    g = torch.Generator().manual_seed(41)
    W = torch.randn(N, Cw, generator=g) / Cw ** 0.5
    b = torch.randn(N, generator=g) * 0.3
    return k, x, gamma, beta, W, b


def fold_model(x, W, gamma, beta, b, eps, slots, half, mut=None):
    """fp32 numpy model of the fold: W' = half(gamma W), c1 = row sums of W', c2 = b + W beta; the producer's per-tile (sum, sum of squares) of the 16-bit
    row, 8 values per unit and the units of a tile sequentially; the consumer adds the slots sequentially; var = Q / K - mean^2 clamped at zero;
    out = rstd (acc - mean c1) + c2 with the cancellation in fp32.  Returns (out float64 of the rounded result, W', c1, c2 as the reference takes them)."""
    M, K = x.shape
    X = x.float().numpy()
    gW = (W.numpy().astype(F32) * gamma.numpy().astype(F32)[None, :]).astype(F32)
    Wp = rnd(gW, half)
    c1 = Wp.sum(1, dtype=F32)
    c2 = ((W.numpy().astype(F32) @ beta.numpy().astype(F32)).astype(F32) + b.numpy().astype(F32)).astype(F32)
    c1_k = gW.sum(1, dtype=F32) if mut == "c1 summed from the un-rounded gamma W" else c1
    c2_k = b.numpy().astype(F32) if mut == "c2 without W beta" else c2
    tw = K // slots
    xs = X.reshape(M, slots, tw)
    S = staged_sum(xs, [8, tw // 8])
    Q = staged_sum((xs * xs).astype(F32), [8, tw // 8])
    n_sum = slots - 1 if mut == "a slot too few summed" else slots
    sx, sq = staged_sum(S[:, :n_sum], [n_sum]), staged_sum(Q[:, :n_sum], [n_sum])
    inv_k = F32(1) / F32(K)
    mean = (sx * inv_k).astype(F32)
    var = np.maximum(((sq * inv_k).astype(F32) - (mean * mean).astype(F32)).astype(F32), F32(0))
    with np.errstate(divide="ignore"):
        rstd = (F32(1) / np.sqrt((var + F32(0.0 if mut == "fold: eps dropped" else eps)).astype(F32))).astype(F32)
    if mut == "fold: statistics of row m^1":
        idx = np.arange(M) ^ 1
        mean, rstd = mean[idx], rstd[idx]
    acc = (X @ Wp.T).astype(F32)
    mc1 = np.zeros_like(acc) if mut == "mean c1 term dropped" else (mean[:, None] * c1_k[None, :]).astype(F32)
    with np.errstate(invalid="ignore", over="ignore"):
        out = ((rstd[:, None] * (acc - mc1).astype(F32)).astype(F32) + c2_k[None, :]).astype(F32)
    t = torch.from_numpy
    return t(rnd(out, half)).double(), t(Wp).to(half), t(c1), t(c2)


def _check_fold_model(Cw, slots, regime, eps, half, mut=None):
    k, x, gamma, beta, W, b = _fold_data(regime, Cw, slots, half)
    out, Wp, c1, c2 = fold_model(x, W, gamma, beta, b, eps, slots, half, mut)
    ref, _, _ = R.fold_ref(x, Wp, c1, c2, None, eps)
    return R.check(f"model fold C {Cw} slots {slots} {regime} eps {eps:g} {half}{' [' + mut + ']' if mut else ''}", out, ref,
                   R.fold_forward_bound(x, Wp, c1, c2, None, eps, k, half), verbose=False)


@pytest.mark.parametrize("Cw,slots", FOLD_CASES)
def test_fold_model_stays_inside_the_bound_at_the_chosen_offset_ratio(Cw, slots):
    """the reference alone -- the fp32 model -- stays within fold_forward_bound at the |mean| / std that offset_ratio admits for the path's k"""
    k = R.k_of(R.fold_stages(Cw, slots))
    worst = 0.0
    for regime in R.REGIMES:
        for eps in R.REGIME_EPS[regime]:
            for half in (torch.float16, torch.bfloat16):
                worst = max(worst, _check_fold_model(Cw, slots, regime, eps, half))
    print(f"[norm-bound] fold C {Cw}: stages {R.fold_stages(Cw, slots)}, k = {k}, offset ratio {R.offset_ratio(k)} (|mean| / std per row "
          f"{R.fold_offsets(k)}), worst model error / bound {worst:.3f}")
    assert worst <= 1.0 and R.offset_ratio(k) < 256


def test_every_fold_mutant_is_rejected_by_some_regime(capsys):
    table = {m: [] for m in FOLD_MUTANTS}
    for regime in R.REGIMES:
        for eps in R.REGIME_EPS[regime]:
            for Cw, slots in FOLD_CASES[1:]:
                for mut in FOLD_MUTANTS:
                    # (both half types: the rounding of gamma W that the c1 mutant leaves out is 8 times larger in bfloat16, and under the worst-case
                    # accumulation term K u sum |x W'| only that one shows it)
                    for half, hn in ((torch.float16, "fp16"), (torch.bfloat16, "bf16")):
                        try:
                            _check_fold_model(Cw, slots, regime, eps, half, mut)
                        except AssertionError:
                            table[mut].append(f"{regime}/{eps:g}/C{Cw}/{hn}")
    with capsys.disabled():
        print("\n[mutants] folded LayerNorm, rejected by (regime/eps/width/half type):")
        for mut in FOLD_MUTANTS:
            print(f"[mutants]   {mut:46s} {', '.join(table[mut][:8]) or '-- NOWHERE --'}{' ... (%d)' % len(table[mut]) if len(table[mut]) > 8 else ''}")
    missing = [m for m in FOLD_MUTANTS if not table[m]]
    assert not missing, f"no regime rejects: {missing}"


@pytest.mark.parametrize("Cw,slots", FOLD_CASES)
def test_statistics_term_of_the_fold_stays_within_two_output_ulps(Cw, slots):
    """the cap for the one-pass fold, on the normalised row it stands for: with the offsets of fold_offsets(k) the statistics term of the one-pass
    forward bound is within 2 ulps of the 16-bit normalised value; the next power of two would break offset_ratio's condition"""
    k = R.k_of(R.fold_stages(Cw, slots))
    r = R.offset_ratio(k)
    assert r in (2, 4, 8, 16, 32)
    if r < 32:
        assert 0.5 * k * R.U * (3 * (2 * r) ** 2 + 1) + k * R.U * (2 * r + 0.8) / 4.0 > 2.0 ** -10
    M = 24
    for regime in R.REGIMES:
        eps = R.REGIME_EPS[regime][0]
        for half in (torch.float16, torch.bfloat16):
            x = R.ln_input(regime, M, Cw, half, offsets=R.fold_offsets(k))
            gamma, beta = R.ln_params(regime, Cw)
            _, t_stat, _ = R.forward_bound(x, gamma, beta, M, 1, Cw, 1, eps, False, k, half, "onepass", parts=True)
            z, _, _ = R.layernorm_ref(x, gamma, beta, eps)
            X = x.double()
            const = (X.amax(1, keepdim=True) == X.amin(1, keepdim=True)).expand_as(X)
            t_stat = torch.where(const, torch.zeros_like(t_stat), t_stat)
            i = int(t_stat.argmax())
            ts, zz = t_stat.reshape(-1)[i].item(), z.reshape(-1)[i]
            assert ts <= 2 * R.ulp(zz, half).item(), (Cw, regime, half, ts, zz.item())
