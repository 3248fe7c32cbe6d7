"""The activations of the GEMM / feed-forward epilogues over EVERY finite 16-bit pre-activation, elementwise against the float64 references of
tests/act_ref.py under its derived bound, in the fp16 and the bf16 build: the tails unit-scale data never reaches (gelu below -5, exp overflow in the
sigmoid forms, subnormal outputs, bfloat16's exponent range).  The patterns ride through tb_gemm with an identity weight and no bias, so the
pre-activation IS the pattern (x * 1 + zeros is exact in fp32), on the 4-wave kernel through its lean and its generic epilogue (an output pitch that
is no multiple of 8 forces the scalar / generic one); the same sweep goes through tb_geglu_bwd and tb_gated_gelu_tanh.

The worst error / bound is printed per case ([act-bound] lines) and per (build, act, path) by the last test of each build."""
import collections
import ctypes

import pytest
import torch

import act_ref as A
import norm_ref as R

pytestmark = pytest.mark.gpu
dev = "cuda"
N = 256                                                   # patterns per row: 256 rows x 256 columns hold all 65536 bit patterns
V_MAGNITUDES = (1.0, -0.37109375, 3 * 2.0 ** -10, 200.0)     # incoming gradients of the derivative forms, per row (exact in both half types; |f'| < 1.2)
H_MAGNITUDES = (1.0, -0.37109375, 3 * 2.0 ** -10, -2.0 ** -20)   # h / gradients of the GEGLU forms: |h| <= 1, h gelu(g) stays inside the output type
SUMMARY = collections.defaultdict(float)


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


def _patterns(half, rows):
    """[rows, 65536 / rows] of `half`: every bit pattern once, the non-finite ones replaced by zero; and the mask of the finite ones"""
    v = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(half)
    ok = torch.isfinite(v.float())
    v = torch.where(ok, v, torch.zeros_like(v))
    return v.reshape(rows, -1).to(dev), ok.reshape(rows, -1).to(dev)


def _out(rows, cols, half, aligned):
    """an output tensor filled with NaN; `aligned` = False: a view whose row pitch is no multiple of 8 elements (scalar stores, the generic epilogue)"""
    if aligned:
        return torch.full((rows, cols), float("nan"), device=dev, dtype=half)
    return torch.full((rows, cols + 4), float("nan"), device=dev, dtype=half)[:, :cols]


def _four_wave_kernel_ran():
    from textboost_amd import _lib as L
    cfg = (ctypes.c_int * 5)()
    L.lib().tb_gemm_last_config(cfg)
    return not L.lib().tb_gemm8_last(None) and cfg[2] == L.A_LINEAR and cfg[4] == 1, list(cfg)


def _check(half, act, path, got, fe, ok):
    """non-finite INPUTS excluded and nothing else: their slots carry zero, whose result is checked like any other"""
    ref, e = fe
    name = f"{_hname(half)} {act} {path}"
    w = R.check(name, got, ref, A.bound(ref, e, half), verbose=False)
    print(f"[act-bound] {name}: worst error / bound {w:.3f} over {int(ok.sum())} finite patterns")
    key = (_hname(half), act, path)
    SUMMARY[key] = max(SUMMARY[key], w)


def _eye(n, half):
    return torch.eye(n, device=dev).to(half)


@pytest.mark.parametrize("aligned", [True, False], ids=["lean", "generic"])
@pytest.mark.parametrize("act", ["QUICK_GELU", "GELU", "SILU"])
def test_forward_activation_over_every_finite_pattern(half, act, aligned):
    from textboost_amd import _lib as L, ops
    x, ok = _patterns(half, N)
    out = _out(N, N, half, aligned)
    pre = torch.full((N, N), float("nan"), device=dev, dtype=half) if act != "SILU" else None
    ops.gemm(x, _eye(N, half), out, act=getattr(L, "ACT_" + act), C2=pre)
    torch.cuda.synchronize()
    ran, cfg = _four_wave_kernel_ran()
    assert ran, cfg
    if pre is not None:
        assert torch.equal(pre.float(), x.float()), "the stored pre-activation is not the pattern"     # (as values: -0 + 0 = +0 in the accumulator)
    _check(half, act, "lean" if aligned else "generic", out, A.ACTS[act](x), ok)


@pytest.mark.parametrize("aligned", [True, False], ids=["lean", "generic"])
@pytest.mark.parametrize("act", ["QUICK_GELU_GRAD", "GELU_GRAD"])
def test_activation_gradient_over_every_finite_pattern(half, act, aligned):
    """the pattern is the saved pre-activation (C2), the incoming gradient a few magnitudes per row"""
    from textboost_amd import _lib as L, ops
    x, ok = _patterns(half, N)
    v = torch.tensor([V_MAGNITUDES[m % 4] for m in range(N)], device=dev).reshape(N, 1).expand(N, N).to(half).contiguous()
    out = _out(N, N, half, aligned)
    ops.gemm(v, _eye(N, half), out, act=getattr(L, "ACT_" + act), C2=x)
    torch.cuda.synchronize()
    ran, cfg = _four_wave_kernel_ran()
    assert ran, cfg
    _check(half, act, "lean" if aligned else "generic", out, A.times(v, A.ACTS[act](x)), ok)


def _geglu_operands(half):
    """512 rows: g sweeps every pattern (128 per row), h cycles H_MAGNITUDES.  Gate column j < 128 reads g = A[m, j], h = A[m, 128 + j]; gate column
    128 + j reads the same g and -h (weights 0 / 1 / -1: exact).  Returns A [512, 256], the packed weight [512, 256], h, g [512, 256] and the mask."""
    M = 512
    gp, okp = _patterns(half, M)                                        # [512, 128]
    hv = torch.tensor([[H_MAGNITUDES[(m + j) % 4] for j in range(128)] for m in range(M)], device=dev).to(half)
    a = torch.cat([gp, hv], 1).contiguous()
    W = torch.zeros(2 * N, N, device=dev)
    for j in range(N):
        hrow = (j // 32) * 64 + j % 32
        W[hrow, 128 + j % 128] = 1.0 if j < 128 else -1.0
        W[hrow + 32, j % 128] = 1.0
    h = torch.cat([hv, -hv], 1)
    return a, W.to(half), h, torch.cat([gp, gp], 1), torch.cat([okp, okp], 1)


def _packed(h, g):
    M, n = h.shape
    return torch.stack([h.reshape(M, n // 32, 32), g.reshape(M, n // 32, 32)], 2).reshape(M, 2 * n).contiguous()


@pytest.mark.parametrize("aligned", [True, False], ids=["lean", "generic"])
def test_geglu_gate_over_every_finite_pattern(half, aligned):
    from textboost_amd import _lib as L, ops
    a, W, h, g, ok = _geglu_operands(half)
    out = _out(512, N, half, aligned)
    raw = _out(512, 2 * N, half, aligned)
    ops.gemm(a, W, out, act=L.ACT_GEGLU, C2=raw)
    torch.cuda.synchronize()
    ran, cfg = _four_wave_kernel_ran()
    assert ran, cfg
    assert torch.equal(raw.float(), _packed(h, g).float()), "the written pre-gate projections are not the operands"
    _check(half, "GEGLU", "lean" if aligned else "generic", out, A.geglu(h, g), ok)


def _geglu_bwd_check(half, act, path, dproj, v, h, g, ok):
    M, n = h.shape
    d = dproj.reshape(M, n // 32, 2, 32)
    (rdh, edh), (rdg, edg) = A.geglu_bwd(v, h, g)
    _check(half, act + " dh", path, d[:, :, 0].reshape(M, n), (rdh, edh), ok)
    _check(half, act + " dg", path, d[:, :, 1].reshape(M, n), (rdg, edg), ok)


@pytest.mark.parametrize("aligned", [True, False], ids=["lean", "generic"])
def test_geglu_backward_in_the_dgrad_epilogue_over_every_finite_pattern(half, aligned):
    from textboost_amd import _lib as L, ops
    _, _, h, g, ok = _geglu_operands(half)
    v = torch.tensor([H_MAGNITUDES[m % 2] for m in range(512)], device=dev).reshape(512, 1).expand(512, N).to(half).contiguous()
    dproj = _out(512, 2 * N, half, aligned)
    ops.gemm(v, _eye(N, half), dproj, act=L.ACT_GEGLU_GRAD, C2=_packed(h, g))
    torch.cuda.synchronize()
    ran, cfg = _four_wave_kernel_ran()
    assert ran, cfg
    _geglu_bwd_check(half, "GEGLU_GRAD", "lean" if aligned else "generic", dproj, v, h, g, ok)


def test_geglu_backward_kernel_over_every_finite_pattern(half):
    from textboost_amd import ops
    _, _, h, g, ok = _geglu_operands(half)
    v = torch.tensor([H_MAGNITUDES[m % 2] for m in range(512)], device=dev).reshape(512, 1).expand(512, N).to(half).contiguous()
    dproj = torch.full((512, 2 * N), float("nan"), device=dev, dtype=half)
    ops.geglu_bwd(v, _packed(h, g), dproj)
    torch.cuda.synchronize()
    _geglu_bwd_check(half, "tb_geglu_bwd", "kernel", dproj, v, h, g, ok)


def _gated_tanh(half, path, h, ok):
    from textboost_amd import ops
    rows, F = h.shape
    gm = torch.tensor([[H_MAGNITUDES[(m + j) % 4] for j in range(F)] for m in range(rows)], device=dev).to(half)
    out = torch.full((rows, F), float("nan"), device=dev, dtype=half)
    ops.gated_gelu_tanh(torch.cat([h, gm], 1).contiguous(), out)
    torch.cuda.synchronize()
    _check(half, "gelu_new gate", path, out, A.gated_gelu_new(h, gm), ok)


def test_gated_tanh_gelu_over_every_finite_pattern(half):
    """tb_gated_gelu_tanh: out = gelu_new(h) g, h sweeping every pattern, g a few magnitudes; the 8-wide kernel, and the scalar one (F no multiple of 8:
    252 columns, then the 4 columns that leaves over)"""
    x, ok = _patterns(half, N)
    _gated_tanh(half, "vector", x, ok)
    _gated_tanh(half, "scalar", x[:, :N - 4].contiguous(), ok[:, :N - 4])
    _gated_tanh(half, "scalar", x[:, N - 4:].contiguous(), ok[:, N - 4:])


def test_summary_of_the_worst_error_over_bound(half, capsys):
    hname = _hname(half)
    assert any(k[0] == hname for k in SUMMARY), "no case of this build has run before its summary"
    with capsys.disabled():
        print("\n[act-bound] worst error / bound per (build, act, path):")
        for key in sorted(k for k in SUMMARY if k[0] == hname):
            print("[act-bound]   " + " ".join(f"{k:<18s}" for k in key) + f" {SUMMARY[key]:.3f}")
