"""GroupNorm(+SiLU) and LayerNorm kernels OFF unit scale, elementwise against the float64 references of tests/norm_ref.py under its derived bound:
tiny inputs (group variance below eps, both eps), offsets (|mean| / std up to what the cap of tests/test_norm_ref_host.py admits for the path; 256
for LayerNorm), huge inputs (fp32 squares and sums, SiLU arguments past +-90), mixed scales per image and group (a statistic read from a neighbour
is off by orders of magnitude), degenerate groups (zeros, constants) and -- 16-bit GroupNorm only -- the documented envelope at |mean| / std = 256.
Every dispatch path of norm.hip and the fp32 GroupNorm of f32_path.hip, forward and backward, in the fp16 and the bf16 build; the fused LoRA
down projection; and the eps every model hands to its norms, counted against the oracle's modules.

The worst error / bound of every check is printed ([norm-bound] lines) and summarised per path, regime and half type by the last test of each build."""
import collections

import pytest
import torch

import norm_ref as R

pytestmark = pytest.mark.gpu
dev = "cuda"

SUMMARY = collections.defaultdict(float)     # (half, path, regime, what) -> worst error / bound
ENVELOPE = {}                                # (half, case id, ratio) -> (worst |error| of the normalised value, worst error / bound)


@pytest.fixture(scope="module", params=["fp16", "bf16"])
def half(request):
    """the build of the kernel library under test: every 16-bit case runs in both (this module only; restored on the way out)"""
    from textboost_amd import _lib as L
    prev = L.set_half(request.param)
    try:
        L.lib()
        yield L.half_dtype()
    finally:
        L.set_half(prev)


@pytest.fixture
def fp16_build():
    """the models of the eps tests run on the fp16 build, wherever pytest places them among the cases of the `half` fixture"""
    from textboost_amd import _lib as L
    prev = L.set_half("fp16")
    try:
        yield
    finally:
        L.set_half(prev)


def _note(hname, path, regime, what, w):
    key = (hname, path, regime, what)
    SUMMARY[key] = max(SUMMARY[key], w)


def _hname(dt):
    return {torch.float16: "fp16", torch.bfloat16: "bf16", torch.float32: "fp32"}[dt]


def _sliced(rows, C, dtype, fill, sliced):
    return R.sliced(rows, C, dtype, fill, sliced, dev)


_margins_untouched = R.margins_untouched


# ------------------------------------------------------------------------------------------------------------------ GroupNorm
def _run_groupnorm(case, regime, dt):
    from textboost_amd import _lib as L
    from textboost_amd import ops
    B, HW, C, G = a = (case.B, case.HW, case.C, case.G)
    M, gs, hname = B * HW, case.C // case.G, _hname(dt)
    sliced = regime in ("offset", "mixed")
    if not case.f32:   # what the library reports about the shape (the one-pass 256-thread condition is the split-K consumer's)
        assert ops.groupnorm_splitk_ok(*a) == (R.gn_path(*a) == "fused")
    gamma, beta = (t.to(dev) for t in R.gn_params(regime, C))
    x, xbuf = _sliced(M, C, dt, 5.0, sliced)
    x.copy_(R.gn_input(regime, *a, dt, case.ratio).to(dev))
    g = torch.Generator().manual_seed(23)
    dy_h, add_h = torch.randn(M, C, generator=g).to(dt), torch.randn(M, C, generator=g).to(dt)
    ws = torch.empty(max(1, ops.groupnorm_ws(*a)), device=dev)
    for eps in R.REGIME_EPS[regime]:
        for silu in (True, False):
            y, ybuf = _sliced(M, C, dt, -3.0, sliced)
            stats = torch.full((B, G, 2), float("nan"), device=dev)
            prev = L.lib().tb_groupnorm_set_variant(case.variant) if case.variant is not None else None
            try:
                ops.groupnorm_fwd(x, y, gamma, beta, stats, ws, *a, eps=eps, silu=silu)
                if case.bwd_path:
                    dy, dybuf = _sliced(M, C, dt, 2.0, sliced)
                    add, addbuf = _sliced(M, C, dt, 2.0, sliced)
                    dy.copy_(dy_h.to(dev)); add.copy_(add_h.to(dev))
                    dx, dxbuf = _sliced(M, C, dt, -3.0, sliced)
                    ops.groupnorm_bwd(dy, x, gamma, beta, stats, dx, ws, *a, silu=silu, add=add)
            finally:
                if prev is not None:
                    L.lib().tb_groupnorm_set_variant(prev)
            torch.cuda.synchronize()
            yr, (mean, rstd), _ = R.groupnorm_ref(x, gamma, beta, *a, eps, silu)
            bound, _, (e_m, e_rstd) = R.forward_bound(x, gamma, beta, *a, eps, silu, case.k, dt, case.form, parts=True)

            def info(idx, mean=mean, rstd=rstd):
                b, gi = idx[0] // HW, idx[1] // gs
                return f"image {b} group {gi}: mean {mean[b, gi].item():.4e} rstd {rstd[b, gi].item():.4e}"
            name = f"groupnorm {hname} {case.id} {regime} eps {eps:g}{' silu' if silu else ''}"
            if regime in R.ENVELOPE:
                # asserted against the full worst-case bound only (it stays true), + finiteness.  Recorded: the error of the normalised value that the
                # kernel's own statistics give, (x - mean') rstd' against float64 -- free of the output rounding, comparable with a CPU emulation
                w = R.check(name + " y", y, yr, bound, info)
                Xg = x.double().reshape(B, HW, G, gs)
                mk, rk = stats[:, :, 0].double().reshape(B, 1, G, 1), stats[:, :, 1].double().reshape(B, 1, G, 1)
                xh_err = ((Xg - mk) * rk - (Xg - mean.reshape(B, 1, G, 1)) * rstd.reshape(B, 1, G, 1)).abs().max().item()
                key = (hname, case.id, int(regime[len("envelope"):] or 256))
                ENVELOPE[key] = (max(xh_err, ENVELOPE.get(key, (0.0, 0.0))[0]), max(w, ENVELOPE.get(key, (0.0, 0.0))[1]))
                _note(hname, case.path, regime, "y", w)
                continue
            _note(hname, case.path, regime, "y", R.check(name + " y", y, yr, bound, info))
            _note(hname, case.path, regime, "mean", R.check(name + " mean", stats[:, :, 0], mean, e_m + 2 * R.U * mean.abs()))
            _note(hname, case.path, regime, "rstd", R.check(name + " rstd", stats[:, :, 1], rstd, e_rstd))
            assert _margins_untouched(ybuf, C, -3.0) and _margins_untouched(xbuf, C, 5.0), name + ": a margin of the wider buffer was written"
            if regime == "degenerate":
                # the all-zero group and the group of 2.0: every sum is exact, so k = 0 -- y = silu?(beta) to the apply arithmetic and output rounding
                b0 = R.forward_bound(x, gamma, beta, *a, eps, silu, 0, dt, case.form)
                rows, cols = slice(0, HW), slice(0, 2 * gs)
                R.check(name + " y of the exact groups", y[rows, cols], yr[rows, cols], b0[rows, cols], info)
            if case.bwd_path:
                _, _, dxr = R.groupnorm_ref(x, gamma, beta, *a, eps, silu, dy, add)
                bb = R.backward_bound(x, dy, add, gamma, beta, *a, eps, silu, case.k, case.kb, dt, case.form)
                _note(hname, case.bwd_path, regime, "dx", R.check(name + " dx", dx, dxr, bb, info))
                assert _margins_untouched(dxbuf, C, -3.0) and _margins_untouched(dybuf, C, 2.0) and _margins_untouched(addbuf, C, 2.0), name


H_CASES = [c for c in R.GN_CASES if not c.f32 and not c.splitk]


@pytest.mark.parametrize("regime", R.REGIMES + R.ENVELOPE)
@pytest.mark.parametrize("case", H_CASES, ids=lambda c: c.id)
def test_groupnorm_16bit_off_unit_scale(half, case, regime):
    _run_groupnorm(case, regime, half)


@pytest.mark.parametrize("regime", R.REGIMES)
@pytest.mark.parametrize("case", [c for c in R.GN_CASES if c.f32], ids=lambda c: c.id)
def test_groupnorm_fp32_off_unit_scale(case, regime):
    _run_groupnorm(case, regime, torch.float32)


@pytest.mark.parametrize("regime", R.REGIMES)
def test_groupnorm_splitk_consumer_adds_the_slices_before_it_squares(half, regime):
    """tb_groupnorm_fwd_splitk on hand-built partials: S = 3 fp32 k-slices whose +1000 / -1000 components cancel, + bias, + row bias, + residual.
    What the kernel documents for the x it writes (norm.hip, GnSplitK): the slices added in slice order, + bias, + residual, + row bias, all in fp32, ONE
    rounding to the 16-bit type -- and the statistics are those of that rounded x.  So: the written x is checked against the float64 sum (half an
    output ulp + (S + 3) fp32 roundings at the magnitude of the terms, 1000 here), and y / the statistics against the float64 GroupNorm of the
    WRITTEN x under the one-pass bound of the fused path."""
    from textboost_amd import ops
    c = [c for c in R.GN_CASES if c.splitk][0]
    B, HW, C, G = a = (c.B, c.HW, c.C, c.G)
    M, hname = B * HW, _hname(half)
    assert ops.groupnorm_splitk_ok(*a)
    sk = R.splitk_operands(R.gn_input(regime, *a, torch.float32, c.ratio), B, half)
    x64, mag = R.splitk_sum64(sk, B)
    gamma, beta = (t.to(dev) for t in R.gn_params(regime, C))
    part = sk["part"].to(dev).contiguous()
    for eps in R.REGIME_EPS[regime]:
        x = torch.full((M, C), 9.0, device=dev, dtype=half)
        y = torch.full((M, C), -3.0, device=dev, dtype=half)
        stats = torch.full((B, G, 2), float("nan"), device=dev)
        pk = ops.SplitKPartials(part, 3, sk["npad"], sk["bias"].to(dev), sk["rowbias"].to(dev), sk["R"].to(dev), x)
        ops.groupnorm_fwd(x, y, gamma, beta, stats, None, *a, eps=eps, silu=True, partials=pk)
        torch.cuda.synchronize()
        name = f"groupnorm split-K {hname} {regime} eps {eps:g}"
        ex = 6 * R.U * mag
        _note(hname, "splitk", regime, "x", R.check(name + " written x", x.cpu(), x64, ex + 0.5 * R.ulp(x64.abs() + ex, half)))
        yr, (mean, rstd), _ = R.groupnorm_ref(x, gamma, beta, *a, eps, True)
        bound, _, (e_m, e_rstd) = R.forward_bound(x, gamma, beta, *a, eps, True, c.k, half, "onepass", parts=True)
        _note(hname, "splitk", regime, "y", R.check(name + " y", y, yr, bound))
        R.check(name + " mean", stats[:, :, 0], mean, e_m + 2 * R.U * mean.abs())
        R.check(name + " rstd", stats[:, :, 1], rstd, e_rstd)
        assert bool((part[:, :, C:] == 7.0).all())
        # tb_groupnorm_bwd_splitk: dy is the sum of the dgrad convolution's k-slices, never stored; documented the same way -- slice order in fp32,
        # one rounding to the 16-bit type -- so the reference's dy is exactly that (fp32 additions are deterministic), again with +-1000 in the slices
        g = torch.Generator().manual_seed(37)
        sk2 = R.splitk_operands(torch.randn(M, C, generator=g), B, half, seed=41)
        s0, s1, s2 = (t.to(dev) for t in sk2["slices"])
        dy = ((s0 + s1) + s2).to(half)
        add = torch.randn(M, C, generator=g).to(half).to(dev)
        dx = torch.full((M, C), -3.0, device=dev, dtype=half)
        pk2 = ops.SplitKPartials(sk2["part"].to(dev).contiguous(), 3, sk2["npad"], None, None, None, None)
        ops.groupnorm_bwd(None, x, gamma, beta, stats, dx, None, *a, silu=True, add=add, partials=pk2)
        torch.cuda.synchronize()
        _, _, dxr = R.groupnorm_ref(x, gamma, beta, *a, eps, True, dy, add)
        bb = R.backward_bound(x, dy, add, gamma, beta, *a, eps, True, c.k, c.k, half, "onepass")
        _note(hname, "splitk", regime, "dx", R.check(name + " dx", dx, dxr, bb))


# ------------------------------------------------------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("regime", R.REGIMES)
@pytest.mark.parametrize("xk,yk", R.LN_DTYPES)
@pytest.mark.parametrize("M,C", R.LN_CASES)
def test_layernorm_off_unit_scale(half, M, C, xk, yk, regime):
    """ln_fwd_kernel / ln_bwd_kernel: M = 5 leaves a ragged last block of four rows, C = 520 puts a second vector on one lane, 1536 is the widest row;
    `offset` runs |mean| / std up to 256 per row -- the mean-first form holds its bound there, a one-pass rewrite would not"""
    from textboost_amd import ops
    xdt, ydt = (torch.float32 if xk == "f32" else half), (torch.float32 if yk == "f32" else half)
    hname, sliced = _hname(half), regime in ("offset", "mixed")
    k = R.k_path("ln", M, 1, C, 1)
    gamma, beta = (t.to(dev) for t in R.ln_params(regime, C))
    x, xbuf = _sliced(M, C, xdt, 5.0, sliced)
    x.copy_(R.ln_input(regime, M, C, xdt).to(dev))
    g = torch.Generator().manual_seed(5)
    dy, dybuf = _sliced(M, C, ydt, 2.0, sliced)
    add, addbuf = _sliced(M, C, xdt, 2.0, sliced)
    dy.copy_(torch.randn(M, C, generator=g).to(ydt).to(dev)); add.copy_(torch.randn(M, C, generator=g).to(xdt).to(dev))
    for eps in R.REGIME_EPS[regime]:
        y, ybuf = _sliced(M, C, ydt, -3.0, sliced)
        dx, dxbuf = _sliced(M, C, xdt, -3.0, sliced)
        stats = torch.full((M, 2), float("nan"), device=dev)
        ops.layernorm_fwd(x, y, gamma, beta, stats, eps=eps)
        ops.layernorm_bwd(dy, x, gamma, stats, dx, add=add)
        torch.cuda.synchronize()
        yr, (mean, rstd), dxr = R.layernorm_ref(x, gamma, beta, eps, dy, add)
        bound, _, (e_m, e_rstd) = R.layernorm_forward_bound(x, gamma, beta, eps, k, ydt, parts=True)
        info = lambda i: f"row {i[0]}: mean {mean[i[0]].item():.4e} rstd {rstd[i[0]].item():.4e}"
        name = f"layernorm {hname} {M}x{C} {xk}->{yk} {regime} eps {eps:g}"
        path = f"ln {xk}->{yk}"
        _note(hname, path, regime, "y", R.check(name + " y", y, yr, bound, info))
        R.check(name + " mean", stats[:, 0], mean, e_m.reshape(M) + 2 * R.U * mean.abs())
        R.check(name + " rstd", stats[:, 1], rstd, e_rstd.reshape(M))
        _note(hname, path, regime, "dx", R.check(name + " dx", dx, dxr, R.layernorm_backward_bound(x, dy, add, gamma, eps, k, xdt), info))
        for buf, fill in ((xbuf, 5.0), (ybuf, -3.0), (dxbuf, -3.0), (dybuf, 2.0), (addbuf, 2.0)):
            assert _margins_untouched(buf, C, fill), name + ": a margin of the wider buffer was written"


@pytest.mark.parametrize("regime", ["offset", "huge"])
@pytest.mark.parametrize("M,C,Rk", [(130, 768, 12), (5, 1024, 12), (130, 768, 24), (5, 1536, 12)])
def test_layernorm_fused_lora_down_projection(half, M, C, Rk, regime):
    """the LoRA down projection fused into the LayerNorm launch (x fp32, y 16-bit): the RF = 12 kernel (R <= 12, C <= 1024) and the generic one (R = 24,
    or C = 1536), with lora_rows < M -- the rows behind them get zeros.  t against the float64 product of the ROUNDED y the kernel wrote with the
    adapter rounded to the 16-bit type: half an output ulp + (k + 4) fp32 roundings of sum |y a|, k the additions of the row reduction."""
    from textboost_amd import ops
    hname = _hname(half)
    k = R.k_path("ln", M, 1, C, 1)
    eps = R.REGIME_EPS[regime][0]
    gamma, beta = (t.to(dev) for t in R.ln_params(regime, C))
    x = R.ln_input(regime, M, C, torch.float32).to(dev)
    g = torch.Generator().manual_seed(31)
    A = (torch.randn(Rk, C, generator=g) / 4).to(dev)
    lora_rows = M - 3
    y = torch.full((M, C), -3.0, device=dev, dtype=half)
    t = torch.full((M, 64), 5.0, device=dev, dtype=half)
    stats = torch.empty(M, 2, device=dev)
    ops.layernorm_fwd(x, y, gamma, beta, stats, eps=eps, lora_A=A, t=t, lora_rows=lora_rows)
    torch.cuda.synchronize()
    yr, _, _ = R.layernorm_ref(x, gamma, beta, eps)
    name = f"layernorm+lora {hname} {M}x{C} R {Rk} {regime}"
    _note(hname, f"ln+lora R{Rk}", regime, "y", R.check(name + " y", y, yr, R.layernorm_forward_bound(x, gamma, beta, eps, k, half)))
    A16 = A.to(half).double()
    tref = y.double() @ A16.T
    et = (k + 4) * R.U * (y.double().abs() @ A16.abs().T)
    _note(hname, f"ln+lora R{Rk}", regime, "t", R.check(name + " t", t[:lora_rows, :Rk], tref[:lora_rows], (et + 0.5 * R.ulp(tref.abs() + et, half))[:lora_rows]))
    assert bool((t[lora_rows:, :Rk] == 0).all()) and bool((t[:, Rk:] == 5.0).all())


# ------------------------------------------------------------------------------------------------------------------ eps plumbing
class _EpsRecorder:
    """records the eps of every norm a HIP model issues during one forward: ops.groupnorm_fwd, ops.layernorm_fwd, and the LayerNorms that ride in
    other launches -- gemm(ln_fwd= / lnfold=), chain320(eps=), ff_fwd(pre=) -- one entry per normalisation"""

    def __init__(self):
        self.calls = collections.Counter()

    def __enter__(self):
        from textboost_amd import ops
        self.ops = ops
        self.saved = {n: getattr(ops, n) for n in ("groupnorm_fwd", "layernorm_fwd", "gemm", "chain320", "ff_fwd")}
        sv, calls = self.saved, self.calls

        def groupnorm_fwd(*a, **kw):
            calls[("groupnorm", float(kw["eps"] if "eps" in kw else a[10] if len(a) > 10 else 1e-5))] += 1
            return sv["groupnorm_fwd"](*a, **kw)

        def layernorm_fwd(*a, **kw):
            calls[("layernorm", float(kw["eps"] if "eps" in kw else a[5] if len(a) > 5 else 1e-5))] += 1
            return sv["layernorm_fwd"](*a, **kw)

        def gemm(*a, **kw):
            if kw.get("ln_fwd") is not None:
                calls[("layernorm", float(kw["ln_fwd"][4]))] += 1
            if kw.get("lnfold") is not None:
                calls[("layernorm", float(kw["lnfold"][4]))] += 1
            return sv["gemm"](*a, **kw)

        def chain320(*a, **kw):
            calls[("layernorm", float(kw["eps"] if "eps" in kw else a[11] if len(a) > 11 else 1e-5))] += 1
            return sv["chain320"](*a, **kw)

        def ff_fwd(*a, **kw):
            pre = kw.get("pre", a[8] if len(a) > 8 else None)
            if pre is not None:
                calls[("layernorm", float(pre[7]))] += 1
            return sv["ff_fwd"](*a, **kw)

        for n, f in (("groupnorm_fwd", groupnorm_fwd), ("layernorm_fwd", layernorm_fwd), ("gemm", gemm), ("chain320", chain320), ("ff_fwd", ff_fwd)):
            setattr(ops, n, f)
        return self

    def __exit__(self, *exc):
        for n, f in self.saved.items():
            setattr(self.ops, n, f)


def _oracle_norm_calls(module, run):
    """(kind, eps) -> number of nn.GroupNorm / nn.LayerNorm calls of `module` during run()"""
    calls, hooks = collections.Counter(), []
    for m in module.modules():
        if isinstance(m, torch.nn.GroupNorm):
            hooks.append(m.register_forward_hook(lambda mod, i, o: calls.update([("groupnorm", float(mod.eps))])))
        elif isinstance(m, torch.nn.LayerNorm):
            hooks.append(m.register_forward_hook(lambda mod, i, o: calls.update([("layernorm", float(mod.eps))])))
    try:
        with torch.no_grad():
            run()
    finally:
        for h in hooks:
            h.remove()
    return calls


def _same_eps(got, want):
    """the counters agree per (kind, eps); eps compared as the fp32 the kernels receive"""
    f = lambda c: collections.Counter({(k, torch.tensor(e, dtype=torch.float32).item()): n for (k, e), n in c.items()})
    return f(got) == f(want)


def test_unet_hands_every_norm_the_eps_of_the_oracle_module(fp16_build):
    """resnet and output GroupNorms get geo.norm_eps (3e-5 here, unlike anything hard-wired), the transformers' GroupNorm the literal 1e-6 of
    diffusers' Transformer2DModel, every LayerNorm nn.LayerNorm's 1e-5 -- whichever launch carries it.  Every norm module of the oracle runs once per
    forward and the HIP UNet normalises once per module, so the counts per (kind, eps) are compared for the whole model."""
    from oracle.unet_sd import UNet2DCondition, UNetConfig
    from textboost_amd.unet import HipUNet, UNetGeometry
    B, hw, D = 2, 16, 64
    torch.manual_seed(0)
    cfg = UNetConfig.tiny(D)
    cfg.norm_eps = 3e-5
    ref = UNet2DCondition(cfg)
    geo = UNetGeometry(block_out_channels=cfg.block_out_channels, num_heads=cfg.num_heads, cross_attention_dim=D,
                       cross_attn_levels=cfg.cross_attn_levels, use_linear_projection=cfg.use_linear_projection, norm_eps=cfg.norm_eps)
    hip = HipUNet(geo, ref.state_dict(), B, hw, hw, text_len=77, device=dev)
    g = torch.Generator().manual_seed(1)
    x, t, ehs = torch.randn(B, 4, hw, hw, generator=g), torch.tensor([17, 801]), torch.randn(B, 77, D, generator=g)
    want = _oracle_norm_calls(ref, lambda: ref(x, t, ehs))
    with _EpsRecorder() as rec:
        pred = hip.forward(x.half().to(dev), t.to(dev), ehs.half().view(B * 77, D).to(dev).contiguous())
    assert torch.isfinite(pred).all()
    print("[eps] UNet   oracle", dict(want), " HIP", dict(rec.calls))
    assert {e for (k, e) in want if k == "groupnorm"} == {3e-5, 1e-6} and ("layernorm", 1e-5) in want
    assert _same_eps(rec.calls, want), (dict(rec.calls), dict(want))


def test_vae_encoder_hands_every_groupnorm_the_eps_of_the_oracle_module(fp16_build):
    from oracle.vae_encoder import VAEConfig, VAEEncoder
    from textboost_amd import models
    from textboost_amd.vae import HipVAEEncoder, VAEGeometry, vae_encoder_shapes
    B, H, W = 1, 64, 64     # (the smallest map the mid-block attention's GEMMs take: 8 x 8 tokens)
    geo = VAEGeometry(block_out_channels=(64, 64, 128, 128), layers_per_block=1, norm_eps=2e-6)
    cfg = VAEConfig.tiny()
    cfg.norm_eps = 2e-6
    sd = {k: v.half().float() for k, v in models.random_state_dict(vae_encoder_shapes(geo), 5, device="cpu").items()}
    with torch.device("meta"):
        ref = VAEEncoder(cfg)
    ref = ref.to_empty(device="cpu")
    ref.load_state_dict(sd)
    hip = HipVAEEncoder(geo, {k: v.to(dev) for k, v in sd.items()}, B, H, W, device=dev)
    x = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(3)) * 2 - 1
    want = _oracle_norm_calls(ref, lambda: ref.moments(x))
    with _EpsRecorder() as rec:
        mom = hip.moments(x.to(dev))[0]
    assert torch.isfinite(mom).all()
    print("[eps] VAE    oracle", dict(want), " HIP", dict(rec.calls))
    assert set(want) == {("groupnorm", 2e-6)}
    assert _same_eps(rec.calls, want), (dict(rec.calls), dict(want))


def test_text_encoder_hands_every_layernorm_the_eps_of_the_oracle_module(fp16_build):
    from oracle.clip_text import CLIPTextCfg, TextBoostEncoder
    from textboost_amd.text_encoder import CLIPGeometry, HipTextEncoder
    B, D = 2, 64
    torch.manual_seed(0)
    ccfg = CLIPTextCfg.tiny(D)
    ccfg.eps = 3e-6
    base = TextBoostEncoder(ccfg, r=0)
    with torch.no_grad():
        null = base.transformer(torch.tensor([[49406] + [49407] * 76]))[0]
    base.set_null_embedding(null)
    geo = CLIPGeometry(hidden_size=D, intermediate_size=ccfg.intermediate_size, num_layers=ccfg.num_layers, num_heads=ccfg.num_heads, eps=ccfg.eps)
    sd = {hf: dict(base.named_parameters())[ours].detach() for ours, hf in base.hf_key_map().items()}
    hip = HipTextEncoder(geo, sd, B, mode="half", lora_rank=0, device=dev)
    hip.set_null_embedding(null)
    ids = torch.randint(1000, 40000, (B, 77), generator=torch.Generator().manual_seed(2))
    ids[:, 0], ids[:, 20:] = 49406, 49407
    want = _oracle_norm_calls(base, lambda: base(ids))
    with _EpsRecorder() as rec:
        out = hip.forward(ids.to(dev), slot=0)
    assert torch.isfinite(out).all()
    print("[eps] CLIP   oracle", dict(want), " HIP", dict(rec.calls))
    assert set(want) == {("layernorm", 3e-6)} and want[("layernorm", 3e-6)] == 2 * ccfg.num_layers + 1
    assert _same_eps(rec.calls, want), (dict(rec.calls), dict(want))


# ------------------------------------------------------------------------------------------------------------------ summary
def test_summary_of_the_worst_error_over_bound(half, capsys):
    """prints what the cases of this build (and the fp32 ones so far) recorded, past the capture: one line per (build, path, regime, output)"""
    hname = _hname(half)
    assert any(k[0] == hname for k in SUMMARY), "no case of this build has run before its summary"
    with capsys.disabled():
        print("\n[norm-bound] worst error / bound per (build, path, regime, output):")
        for key in sorted(k for k in SUMMARY if k[0] in (hname, "fp32")):
            print("[norm-bound]   " + " ".join(f"{k:<11s}" for k in key) + f" {SUMMARY[key]:.3f}")
        for key in sorted(k for k in ENVELOPE if k[0] == hname):
            print(f"[norm-envelope] {key[0]} {key[1]} |mean|/std {key[2]}: worst error of the normalised value {ENVELOPE[key][0]:.3e}, "
                  f"error / bound {ENVELOPE[key][1]:.3f}")
