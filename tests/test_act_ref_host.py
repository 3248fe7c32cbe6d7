"""tests/act_ref.py on the host: the float64 references against torch.nn.functional + autograd, the bound against fp32 numpy models of every formula
of csrc/common.h / csrc/t5.hip over ALL finite inputs of fp16 and of bfloat16 (it must contain them: not too tight), and against mutants (each must
be rejected: not vacuous).  Prints the worst error / bound per (type, formula) and the mutant table."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import act_ref as A
import norm_ref as R

F32 = np.float32
HALVES = (torch.float16, torch.bfloat16)


def rnd(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F32)).to(dtype).float().numpy()


def f32(*c):
    return [F32(v) for v in c]


# ------------------------------------------------------------------------------------------------------------------ references vs torch
def test_references_match_functional_and_autograd():
    x = torch.linspace(-9, 9, 2001, dtype=torch.float64).requires_grad_(True)
    for ref, grad, fn in ((A.gelu, A.gelu_grad, F.gelu), (A.silu, A.silu_grad, F.silu), (A.quick_gelu, A.quick_gelu_grad, lambda t: t * torch.sigmoid(1.702 * t)),
                          (A.gelu_new, None, lambda t: F.gelu(t, approximate="tanh"))):
        y = fn(x)
        torch.testing.assert_close(ref(x.detach())[0], y.detach(), rtol=1e-12, atol=1e-15)    # (torch forms 1 + erf: absolute accuracy only in the negative tail)
        if grad is not None:
            (g,) = torch.autograd.grad(y.sum(), x)
            torch.testing.assert_close(grad(x.detach())[0], g, rtol=1e-11, atol=1e-15)
    h, g, v = (torch.randn(500, dtype=torch.float64, generator=torch.Generator().manual_seed(i)).requires_grad_(i < 2) for i in range(3))
    out = h * F.gelu(g)
    dh, dg = torch.autograd.grad(out, (h, g), v)
    (rdh, _), (rdg, _) = A.geglu_bwd(v, h.detach(), g.detach())
    torch.testing.assert_close(A.geglu(h.detach(), g.detach())[0], out.detach(), rtol=1e-12, atol=0)
    torch.testing.assert_close(rdh, dh, rtol=1e-12, atol=0)
    torch.testing.assert_close(rdg, dg, rtol=1e-11, atol=1e-15)


def test_every_finite_pattern_is_enumerated():
    assert A.all_finite(torch.float16).numel() == 63488 and A.all_finite(torch.bfloat16).numel() == 65280
    for dt in HALVES:
        v = A.all_finite(dt)
        assert v.unique().numel() == v.numel() - 1          # (+0 and -0 compare equal)
        assert v.float().abs().max().item() == torch.finfo(dt).max


# ------------------------------------------------------------------------------------------------------------------ fp32 models of the formulas
def m_cdf(x):
    """normal_cdf_f of common.h in numpy fp32"""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        z = (np.abs(x) * F32(0.70710678118654752)).astype(F32)
        t = (F32(1) / (F32(1) + F32(0.5) * z)).astype(F32)
        q = np.full_like(x, F32(0.17087277))
        for c in f32(-0.82215223, 1.48851587, -1.13520398, 0.27886807, -0.18628806, 0.09678418, 0.37409196, 1.00002368, -1.26551223):
            q = (q * t + c).astype(F32)
        half = (F32(0.5) * t * np.exp((q - z * z).astype(F32), dtype=F32)).astype(F32)
        return np.where(x < 0, half, F32(1) - half).astype(F32)


def m_pdf_x(x):
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return (x * F32(0.3989422804014327) * np.exp((F32(-0.5) * x * x).astype(F32), dtype=F32)).astype(F32)


def m_sig(a):
    with np.errstate(over="ignore", under="ignore"):
        return (F32(1) / (F32(1) + np.exp(-a, dtype=F32))).astype(F32)


def m_xsig(x, a):
    with np.errstate(over="ignore", under="ignore"):
        return (x / (F32(1) + np.exp(-a, dtype=F32))).astype(F32)


def m_sig_grad(a):
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        s = m_sig(a)
        return (s * (F32(1) + a * (F32(1) - s))).astype(F32)


def m_gelu_new_arg(x):
    with np.errstate(over="ignore", invalid="ignore"):
        return (F32(2) * (F32(0.7978845608028654) * (x + F32(0.044715) * x * x * x).astype(F32))).astype(F32)


MODELS = {
    "GELU": lambda x: (x * m_cdf(x)).astype(F32),
    "GELU_GRAD": lambda x: (m_cdf(x) + m_pdf_x(x)).astype(F32),
    "QUICK_GELU": lambda x: m_xsig(x, (F32(1.702) * x).astype(F32)),
    # (the argument is clamped to +-65536 first: in bfloat16 1.702 x overflows past 2e38 and inf * (1 - s) = inf * 0 would be NaN)
    "QUICK_GELU_GRAD": lambda x: m_sig_grad((F32(1.702) * np.clip(x, F32(-65536), F32(65536))).astype(F32)),
    "SILU": lambda x: m_xsig(x, x),
    "SILU_GRAD": lambda x: m_sig_grad(x),
    "GELU_NEW": lambda x: m_xsig(x, m_gelu_new_arg(x)),
}
MUTANTS = {
    "tanh-GELU for erf-GELU": ("GELU", lambda x: m_xsig(x, m_gelu_new_arg(x))),
    "1.7 for 1.702": ("QUICK_GELU", lambda x: m_xsig(x, (F32(1.7) * x).astype(F32))),
    "1.7 for 1.702 in the derivative": ("QUICK_GELU_GRAD", lambda x: m_sig_grad((F32(1.7) * x).astype(F32))),
    "gelu' without the x pdf term": ("GELU_GRAD", lambda x: m_cdf(x)),
    "1 + tanh evaluated directly": ("GELU_NEW", lambda x: (F32(0.5) * x * (F32(1) + np.tanh((F32(0.5) * m_gelu_new_arg(x)).astype(F32), dtype=F32))).astype(F32)),
}
V_MAGNITUDES = (1.0, -0.37109375, 3 * 2.0 ** -10, 200.0)     # incoming gradients of the derivative forms (exact in both half types; |f'| < 1.2)
H_MAGNITUDES = (1.0, -0.37109375, 3 * 2.0 ** -10, -2.0 ** -20)    # h / gradients of the GEGLU forms: |h| <= 1, so that h gelu(g) stays inside the output type


def _worst(name, got, ref, e, dtype, verbose=False):
    if callable(got):
        with np.errstate(over="ignore", under="ignore", invalid="ignore"):
            got = got()
    return R.check(name, torch.from_numpy(rnd(got, dtype)).double(), ref, A.bound(ref, e, dtype), verbose=verbose)


@pytest.mark.parametrize("dtype", HALVES, ids=["fp16", "bf16"])
def test_fp32_models_stay_inside_the_bound_over_every_finite_input(dtype, capsys):
    x = A.all_finite(dtype)
    xn = x.float().numpy()
    lines = []
    for act, fn in MODELS.items():
        ref, e = A.ACTS[act](x)
        lines.append(f"[act-bound] {dtype} {act:16s} worst model error / bound {_worst(f'model {act} {dtype}', lambda: fn(xn), ref, e, dtype):.3f}")
        if act.endswith("_GRAD"):
            for v in V_MAGNITUDES:
                vt = torch.full_like(ref, v)
                pr, pe = A.times(vt, (ref, e))
                _worst(f"model {v:g} * {act} {dtype}", lambda: (F32(v) * fn(xn)).astype(F32), pr, pe, dtype)
    # the GEGLU gate and its backward pair: g sweeps every pattern, h / the incoming gradient cycle a few magnitudes
    for hv in H_MAGNITUDES:
        h = torch.full(x.shape, hv).to(dtype)
        hn = h.float().numpy()
        ge, dge = (xn * m_cdf(xn)).astype(F32), (m_cdf(xn) + m_pdf_x(xn)).astype(F32)
        ref, e = A.geglu(h, x)
        w = _worst(f"model GEGLU h {hv:g} {dtype}", (hn * ge).astype(F32), ref, e, dtype)
        for v in H_MAGNITUDES[:2]:
            (rdh, edh), (rdg, edg) = A.geglu_bwd(torch.full(x.shape, v), h, x)
            w = max(w, _worst(f"model GEGLU dh {dtype}", (F32(v) * ge).astype(F32), rdh, edh, dtype))
            w = max(w, _worst(f"model GEGLU dg {dtype}", ((F32(v) * hn).astype(F32) * dge).astype(F32), rdg, edg, dtype))
        ref, e = A.gated_gelu_new(x, h)
        w = max(w, _worst(f"model gelu_new(h) g {dtype}", (MODELS["GELU_NEW"](xn) * hn).astype(F32), ref, e, dtype))
        lines.append(f"[act-bound] {dtype} GEGLU fwd / bwd, gelu_new gate, h = {hv:g}: worst model error / bound {w:.3f}")
    with capsys.disabled():
        print("\n" + "\n".join(lines))


def test_every_activation_mutant_is_rejected(capsys):
    table = {}
    for name, (act, fn) in MUTANTS.items():
        table[name] = []
        for dtype in HALVES:
            x = A.all_finite(dtype)
            ref, e = A.ACTS[act](x)
            try:
                _worst(f"mutant {name} {dtype}", lambda: fn(x.float().numpy()), ref, e, dtype)
            except AssertionError:
                table[name].append(str(dtype))
    # the gate on the un-rounded projection: the fp32 projection sits 0.4 of a 16-bit ulp beyond the value it rounds to; the kernel gates on the ROUNDED one
    name = "the gate on the un-rounded projection"
    table[name] = []
    for dtype in HALVES:
        g = A.all_finite(dtype)
        g = g[(g.float().abs() > 2.0 ** -10) & (g.float().abs() < 100)]
        p32 = (g.double() + 0.4 * torch.sign(g.double()) * R.ulp(g.double(), dtype)).float().numpy()     # (away from zero: the same binade)
        assert np.array_equal(rnd(p32, dtype), g.float().numpy())
        h = torch.full(g.shape, 1.0).to(dtype)
        ref, e = A.geglu(h, g)
        _worst(f"model GEGLU on the rounded projection {dtype}", (rnd(p32, dtype) * m_cdf(rnd(p32, dtype))).astype(F32), ref, e, dtype)
        try:
            _worst(f"mutant {name} {dtype}", (p32 * m_cdf(p32)).astype(F32), ref, e, dtype)
        except AssertionError:
            table[name].append(str(dtype))
    with capsys.disabled():
        print("\n[mutants] activations, rejected over every finite input of:")
        for name, where in table.items():
            print(f"[mutants]   {name:42s} {', '.join(where) or '-- NOWHERE --'}")
    assert all(len(w) == len(HALVES) for w in table.values()), table
