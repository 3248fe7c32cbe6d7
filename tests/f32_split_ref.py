"""CPU emulation of the split mode of the fp32 contractions (textboost_amd/csrc/f32_path.hip, tb_f32_set_mode(1)) -- test infrastructure.

Every fp32 operand is written as hi + lo with hi = bf16(a) (round to nearest even) and lo = bf16(a - hi); a product a.w is evaluated as
lo_a hi_w + hi_a lo_w + hi_a hi_w (small terms first) with fp32 accumulation.  The bf16 values are held in fp32 tensors here: a product of
two bf16 values is exact in fp32, so an fp32 matmul of them is what the matrix instruction computes up to summation order.

`split_products()` is a TorchDispatchMode in the manner of oracle/fp16_mode.py: it reroutes aten.mm / addmm / bmm / baddbmm / convolution /
convolution_backward (what the oracle's Linear, `@`, conv2d and their autograd lower to) to that evaluation.  Running the UNCHANGED oracle
under it gives, on the CPU, the error the split adds to any quantity the suite compares: the yardstick the GPU tolerances of
tests/test_gpu_f32_split.py are tied to.  It is measured against the oracle, never against the kernel."""
from __future__ import annotations

import torch
from torch.utils._python_dispatch import TorchDispatchMode

TERMS = ("lh", "hl", "hh")   # the kernel's order: lo_a hi_w, hi_a lo_w, hi_a hi_w


def split(t):
    """fp32 tensor -> (hi, lo) as fp32 tensors holding bf16 values; lo = 0 where hi is not finite"""
    hi = t.to(torch.bfloat16).to(torch.float32)
    lo = (t - hi).to(torch.bfloat16).to(torch.float32)
    return hi, torch.where(torch.isfinite(hi), lo, torch.zeros_like(lo))


def split_apply(fn, a, w, terms=TERMS):
    """sum over `terms` of fn(part of a, part of w), accumulated in fp32 in the given order"""
    parts_a = dict(zip("hl", split(a)))
    parts_w = dict(zip("hl", split(w)))
    acc = None
    for t in terms:
        y = fn(parts_a[t[0]], parts_w[t[1]])
        acc = y if acc is None else acc + y
    return acc


def split_matmul(a, w, terms=TERMS):
    """a [.., M, K] @ w [.., K, N] in the split mode (terms: which of the three products are kept -- the tests drop one to show that the
    bound notices)"""
    return split_apply(torch.matmul, a, w, terms)


def product_bound(K, S, alpha=1.0):
    """elementwise bound on |C - C64| for C = alpha * sum_k a_k w_k in the split mode, S = sum_k |a_k||w_k| (float64): the representation error
    (3 * 2^-18 per product, 2^-16 covers the second-order terms) plus at most one fp32 rounding per accumulated term (3 K products + the
    epilogue).  Discriminates up to K ~ 64; at K >= 772 the accumulation term swamps it."""
    return (2.0 ** -16 + (3 * K + 8) * 2.0 ** -24) * S * abs(alpha)


def _f32(*ts):
    return all(isinstance(t, torch.Tensor) and t.dtype == torch.float32 for t in ts)


class split_products(TorchDispatchMode):
    """`with split_products(): y = module(x)`: every fp32 contraction (forward and backward alike) is evaluated as the three-term bf16 split"""

    def __init__(self):
        super().__init__()
        self.calls = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        name = str(func)
        if name in ("aten.mm.default", "aten.bmm.default") and _f32(*args[:2]):
            self.calls += 1
            return split_matmul(args[0], args[1])
        if name in ("aten.addmm.default", "aten.baddbmm.default") and _f32(*args[:3]):
            self.calls += 1
            beta, alpha = kwargs.get("beta", 1), kwargs.get("alpha", 1)
            return beta * args[0] + alpha * split_matmul(args[1], args[2])
        if name == "aten.convolution.default" and _f32(*args[:2]):
            self.calls += 1
            x, w, bias, rest = args[0], args[1], args[2], args[3:]
            y = split_apply(lambda xa, wa: func(xa, wa, None, *rest), x, w)
            return y if bias is None else y + bias.view(1, -1, *([1] * (y.dim() - 2)))
        if name == "aten.convolution_backward.default" and _f32(*args[:3]):
            self.calls += 1
            g, x, w, rest = args[0], args[1], args[2], args[3:]
            mask = rest[-1]
            (gh, gl), (xh, xl), (wh, wl) = split(g), split(x), split(w)
            # one call gives grad_input(g, w) and grad_weight(g, x): the three calls below are lo hi + hi lo + hi hi of both at once
            outs = [func(gl, xh, wh, *rest), func(gh, xl, wl, *rest), func(gh, xh, wh, *rest)]
            gi = outs[0][0] + outs[1][0] + outs[2][0] if mask[0] else None
            gw = outs[0][1] + outs[1][1] + outs[2][1] if mask[1] else None
            gb = g.sum([d for d in range(g.dim()) if d != 1]) if mask[2] else None
            return gi, gw, gb
        return func(*args, **kwargs)


def rel_l2(a, b):
    a, b = a.detach().double(), b.detach().double()
    return ((a - b).norm() / (b.norm() + 1e-300)).item()


def measures(got, ref, ch_dim=None):
    """the three figures tests/parity.py asserts on: rel-L2, max-abs / max|ref|, worst-channel rel-L2 (None without ch_dim)"""
    a, b = got.detach().float().cpu(), ref.detach().float().cpu()
    r = ((a - b).norm() / (b.norm() + 1e-30)).item()
    m = ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()
    c = None
    if ch_dim is not None:
        dims = [d for d in range(a.dim()) if d != ch_dim]
        c = ((a - b).pow(2).sum(dims).sqrt() / b.pow(2).sum(dims).sqrt().clamp_min(1e-30)).max().item()
    return r, m, c


# ------------------------------------------------------------------------------------------------ the oracle's tiny models (CPU only)
def tiny_unet(D=64, seed=0):
    """the oracle UNet of the small configuration of tests/test_gpu_f32.py (same seed -> same weights as its _small_unet_f32)"""
    from oracle.unet_sd import UNet2DCondition, UNetConfig
    torch.manual_seed(seed)
    ref = UNet2DCondition(UNetConfig.tiny(D))
    with torch.no_grad():
        for n, p in ref.named_parameters():
            if "norm" in n:
                p.add_(torch.randn_like(p) * 0.1)
    return ref


def unet_pred_and_dehs(ref, x, t, ehs, dpred):
    e = ehs.detach().clone().requires_grad_(True)
    pred = ref(x, t, e)
    pred.backward(dpred)
    for p in ref.parameters():
        p.grad = None
    return pred.detach(), e.grad.detach()


def tiny_encoders(D=64, r=4, n_added=3, seed=0):
    """student / teacher oracles of tests/test_gpu_f32.py's _encoders_f32 (same seed -> same weights)"""
    from oracle import train_step as ts
    from oracle.clip_text import CLIPTextCfg, TextBoostEncoder, add_tokens
    torch.manual_seed(seed)
    ccfg = CLIPTextCfg.tiny(D)
    base = TextBoostEncoder(ccfg, r=0)
    with torch.no_grad():
        for n, p in base.named_parameters():
            if "ln" in n or n.endswith("bias"):
                p.add_(torch.randn_like(p) * 0.1)
        base.token_embedding.weight.mul_(0.5)
        null = base.transformer(torch.tensor([[49406] + [49407] * 76]))[0]
    base.set_null_embedding(null)
    teacher = ts.make_teacher(base)
    student = TextBoostEncoder(ccfg, r=r)
    student.load_state_dict(base.state_dict(), strict=False)
    student.set_null_embedding(null)
    with torch.no_grad():
        for n, p in student.named_parameters():
            if "lora_B" in n:
                p.normal_(std=0.05)
    added = add_tokens(student, [100, 200, 300][:n_added])
    return student, teacher, added
