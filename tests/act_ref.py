"""Float64 references for the activations that ride in the GEMM / feed-forward epilogues (csrc/common.h: gelu_erf_f, gelu_erf_grad_f, gelu_erf_both_f,
quick_gelu_f, quick_gelu_grad_f, silu_f; csrc/t5.hip: gelu_new_f) and an elementwise bound derived from the formulas, for tests/test_act_ref_host.py
(CPU) and tests/test_gpu_act_range.py (the kernels, over every finite 16-bit input).  Nothing here is taken from the code under test but the FORM of
each formula (which operations it performs in fp32), and nothing calls torch.nn.functional.

BOUND  |out_kernel - ref| <= half an ulp of the output type at (|ref| + e + TINY) + e + TINY
  u = 2^-24; TINY = 2^-126, the smallest normal fp32 (= the smallest normal bfloat16): below it an fp32 evaluation may flush.
  e = the fp32 evaluation error of the formula (every function below returns (ref, e)):

  sigmoid forms  y = x s, s = 1 / (1 + E), E = exp(-a); a = x (SiLU), 1.702 x (quick-GELU), 2 sqrt(2/pi) (x + 0.044715 x^3) (gelu_new).
    The argument carries ka relative roundings (0, 1, 5), the exponential is exp2(a log2 e): one more rounding of the argument and 2u of its own, so
    eps_E = ((ka + 2) |a| + 4) u -- the relative error of a fast exp grows like |a| u, as in norm_ref's t_silu.  s: d s / s = (1 - s) eps_E + 6u (the
    add, the division or rcp).  e = |y| (eps_s + u) + |x| TINY: s is an fp32 number, so where E overflows (a < -88.7) or 1 / (1 + E) falls below the
    smallest normal it is only good to TINY absolutely, and y = x s inherits |x| TINY.  (That is the floor placed where the flush happens.)
    Derivative d = s (1 + a (1 - s)): 1 - s is formed as 1.f - s, its ABSOLUTE error is e1 = s eps_s + u (where 1 - s < u / 2 the computed s is
    exactly 1 and e1 = 1 - s itself); e = s (|a| e1 + 2u |a| (1 - s) + u |1 + a (1 - s)|) + |d| (eps_s + u) + (1 + |a|) TINY.
  erf forms  Phi(x) = hc for x < 0, 1 - hc otherwise, hc = erfc(|x| / sqrt 2) / 2 = t exp(P(t) - z^2) / 2 (Numerical Recipes 6.2: fractional error
    < 1.2e-7 for every z >= 0, quoted in common.h).  In fp32: eps_c = 1.2e-7 + (3 (z^2 + 2) + 16) u (the exponent z^2 - P, |P| <= 2, is formed with
    3 roundings and scaled by log2 e; rcp, nine FMAs and the exp's own 2u in the 16).  e_Phi = hc eps_c + u [x >= 0] + TINY.
    gelu = x Phi: e = |x| e_Phi + u |y|.   gelu' = Phi + x phi, phi = exp(-x^2 / 2) / sqrt(2 pi): e = e_Phi + |x| phi (x^2 + 8) u + |x| TINY + u |d|.
  products  v f(x) (the *_GRAD epilogues; v = the exact fp32 accumulator): |v| e_f + u |out|.   GEGLU h gelu(g): |h| e + u |out|;  its backward
    dh = v gelu(g): |v| e + u |dh|;  dg = v h gelu'(g): |v h| e' + 2u |dg|.   gelu_new(h) g: |g| e + u |out|.
"""
import math

import torch

from norm_ref import U, ulp

TINY = 2.0 ** -126
_SQRT2 = math.sqrt(2.0)
_INV_SQRT_2PI = 1.0 / math.sqrt(2.0 * math.pi)


def all_finite(dtype):
    """every finite value of a 16-bit float type, in bit-pattern order (63488 of fp16, 65280 of bfloat16)"""
    v = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(dtype)
    return v[torch.isfinite(v.float())]


def bound(ref, e, dtype):
    return 0.5 * ulp(ref.abs() + e + TINY, dtype) + e + TINY


# ------------------------------------------------------------------------------------------------------------------ sigmoid forms
def _sigmoid_form(x, a, ka):
    """(s, 1 - s, eps_s) of s = sigmoid(a) with `ka` relative roundings in the argument (module docstring)"""
    s, c = torch.sigmoid(a), torch.sigmoid(-a)
    eps_e = ((ka + 2) * a.abs() + 4) * U
    return s, c, c * eps_e + 6 * U


def _x_sigmoid(x, a, ka):
    x = x.double()
    s, c, eps_s = _sigmoid_form(x, a, ka)
    y = x * s
    return y, y.abs() * (eps_s + U) + x.abs() * TINY


def _sigmoid_grad(a, ka):
    s, c, eps_s = _sigmoid_form(None, a, ka)
    d = s * (1.0 + a * c)
    e1 = torch.where(c < 0.5 * U, c, s * eps_s + U)
    e = s * (a.abs() * e1 + 2 * U * a.abs() * c + U * (1.0 + a * c).abs()) + d.abs() * (eps_s + U) + (1.0 + a.abs()) * TINY
    return d, e


def silu(x):
    return _x_sigmoid(x, x.double(), 0)


def silu_grad(x):
    return _sigmoid_grad(x.double(), 0)


def quick_gelu(x, slope=1.702):
    return _x_sigmoid(x, slope * x.double(), 1)


def quick_gelu_grad(x, slope=1.702):
    return _sigmoid_grad(slope * x.double(), 1)


def gelu_new(x):
    xd = x.double()
    return _x_sigmoid(x, 2.0 * math.sqrt(2.0 / math.pi) * (xd + 0.044715 * xd * xd * xd), 5)


# ------------------------------------------------------------------------------------------------------------------ erf forms
def _phi_cdf(x):
    x = x.double()
    z = x.abs() / _SQRT2
    hc = 0.5 * torch.special.erfc(z)
    eps_c = 1.2e-7 + (3.0 * (z * z + 2.0) + 16.0) * U
    cdf = 0.5 * torch.special.erfc(-x / _SQRT2)
    return cdf, hc * eps_c + U * (x >= 0).double() + TINY


def gelu(x):
    cdf, e_cdf = _phi_cdf(x)
    y = x.double() * cdf
    return y, x.double().abs() * e_cdf + U * y.abs()


def gelu_grad(x):
    xd = x.double()
    cdf, e_cdf = _phi_cdf(x)
    pdf = torch.exp(-0.5 * xd * xd) * _INV_SQRT_2PI
    d = cdf + xd * pdf
    return d, e_cdf + xd.abs() * pdf * (xd * xd + 8.0) * U + xd.abs() * TINY + U * d.abs()


# ------------------------------------------------------------------------------------------------------------------ products
def times(v, fe):
    """v f(x) for (f, e_f) = fe"""
    f, e = fe
    out = v.double() * f
    return out, v.double().abs() * e + U * out.abs()


def geglu(h, g):
    return times(h, gelu(g))


def geglu_bwd(v, h, g):
    """((dh, e), (dg, e)) of the GEGLU gate's backward for the incoming gradient v: dh = v gelu(g), dg = v h gelu'(g)"""
    d, e = gelu_grad(g)
    vh = v.double() * h.double()
    dg = vh * d
    return times(v, gelu(g)), (dg, vh.abs() * e + 2 * U * dg.abs())


def gated_gelu_new(h, g):
    return times(g, gelu_new(h))


ACTS = {"GELU": gelu, "QUICK_GELU": quick_gelu, "SILU": silu, "GELU_GRAD": gelu_grad, "QUICK_GELU_GRAD": quick_gelu_grad, "SILU_GRAD": silu_grad,
        "GELU_NEW": gelu_new}
