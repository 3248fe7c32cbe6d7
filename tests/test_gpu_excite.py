"""Attend-and-Excite on the GPU (inference.py --excite): the kernels of csrc/excite.hip against the float64 references of
tests/excite_ref.py, conv_in's input gradient, `HipUNet.backward_sample`, the excite pass on the tiny UNet against oracle autograd, one descent
step, the sampler and the command line.

Kernel bound: the fp32 CPU evaluation of the same formulas (excite_ref, dtype=float32) has a maximum error against float64 on the same
operands; every element of a kernel's output must lie within 8 x that yardstick (the convention of tests/test_gpu_attn_loss.py), plus, for
16-bit outputs, half an ulp of the output dtype at the reference value.  Arg-max decisions are compared exactly: tests/test_excite_host.py
holds every input used here to a 2 % margin between the best and the second best candidate."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import excite_ref as R

pytestmark = pytest.mark.gpu
dev = "cuda"
TB_EINVAL = -22
MARGIN = 8.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _table(words, nb, n_words=8, n_pos=16):
    t = torch.full((nb, n_words, n_pos), -1, dtype=torch.int32)
    for w, pos in enumerate(words):
        t[:, w, :len(pos)] = torch.tensor(sorted(pos), dtype=torch.int32)
    return t


def _loss_launch(A, last, words, h, w, loss_scale, check=False):
    from textboost_amd import ops
    nb, T, _ = A.shape
    out = dict(loss=torch.full((nb,), 7.0, device=dev), word=torch.full((nb,), 7, dtype=torch.int32, device=dev),
               sel=torch.full((nb, 9), 7, dtype=torch.int32, device=dev), dA=torch.full((nb, 9, T), 7.0, device=dev))
    ops.excite_loss(A.to(dev), torch.full((nb,), last, dtype=torch.int32, device=dev), _table(words, nb).to(dev), h, w, loss_scale,
                    out["loss"], out["word"], out["sel"], out["dA"], check=check)
    return {k: v.cpu() for k, v in out.items()}


# ------------------------------------------------------------------------------------------------------------------ tb_excite_loss
@pytest.mark.parametrize("half", ["fp16", "bf16"])
@pytest.mark.parametrize("case", R.LOSS_CASES, ids=lambda c: f"{c[0]}x{c[1]}x{c[2]}")
def test_loss_kernel_matches_the_float64_reference(case, half):
    from textboost_amd import _lib as L
    h, w, T, last, words = case
    A = R.loss_inputs(case)
    with L.use_half(half):      # (fp32 / int32 operands only: the same code in both builds)
        for loss_scale in (1.0, 256.0):
            got = _loss_launch(A, last, words, h, w, loss_scale, check=True)
            again = _loss_launch(A, last, words, h, w, loss_scale)
            for k in got:
                assert torch.equal(got[k], again[k]), k                  # a relaunch (and check = 0) gives the same bits
            yl = yd = 0.0
            refs = []
            for b in range(R.NB):
                ref = R.excite_loss_ref(A[b], last, words, h, w, loss_scale)
                r32 = R.excite_loss_ref(A[b], last, words, h, w, loss_scale, dtype=torch.float32)
                assert r32["sel"] == ref["sel"] and r32["word"] == ref["word"]
                yl = max(yl, abs(r32["loss"] - ref["loss"]))
                yd = max(yd, (r32["dA"].double() - ref["dA"]).abs().max().item())
                refs.append(ref)
            for b, ref in enumerate(refs):
                assert got["word"][b].item() == ref["word"] and got["sel"][b].tolist() == ref["sel"], (b, got["sel"][b].tolist(), ref["sel"])
                el = abs(got["loss"][b].item() - ref["loss"])
                ed = (got["dA"][b].double() - ref["dA"]).abs().max().item()
                print(f"[excite] loss {half} {case[:4]} scale {loss_scale:g} image {b}: loss {got['loss'][b].item():.7f} err {el:.2e} "
                      f"(yardstick {yl:.2e}), dA err {ed:.2e} (yardstick {yd:.2e}, max |dA| {ref['dA'].abs().max().item():.3e})")
                assert el <= MARGIN * yl and ed <= MARGIN * yd
                assert (got["dA"][b][:, 0] == 0).all() and (got["dA"][b][:, last:] == 0).all()


def test_loss_kernel_ties_saturation_and_absent_words():
    h, w, T, last = 4, 5, 12, 7
    A = torch.full((2, T, h * w), 0.25)
    got = _loss_launch(A, last, [[3], [1, 2], [5]], h, w, 1.0)
    assert got["word"].tolist() == [0, 0] and got["sel"][0].tolist() == [0, 1, w, w + 1] + [-1] * 5       # lowest word, lowest position
    ref = R.excite_loss_ref(A[0], last, [[3], [1, 2], [5]], h, w)
    assert abs(got["loss"][0].item() - ref["loss"]) <= 2.0 ** -24
    got = _loss_launch(A, last, [[1, 2], [3], [5]], h, w, 1.0)
    assert got["word"].tolist() == [1, 1]
    # l = 0: token 1 owns every position
    A = torch.zeros(2, 8, 16)
    A[:, 1] = 1.0
    got = _loss_launch(A, 4, [[1]], 4, 4, 256.0)
    assert got["loss"].tolist() == [0.0, 0.0] and got["word"].tolist() == [0, 0] and (got["sel"] == -1).all() and (got["dA"] == 0).all()
    # no word has a position: nothing to excite
    got = _loss_launch(torch.rand(2, 8, 16), 4, [], 4, 4, 1.0)
    assert got["loss"].tolist() == [0.0, 0.0] and got["word"].tolist() == [-1, -1] and (got["sel"] == -1).all() and (got["dA"] == 0).all()


def test_loss_kernel_refusals_write_nothing():
    from textboost_amd import _lib as L

    def call(h=4, w=4, T=8, last=4, pos=2, n_words=8, n_pos=16, check=1, loss_scale=1.0):
        nb = 2
        A = torch.rand(nb, max(T, 1), max(h * w, 1), device=dev)
        lst = torch.full((nb,), last, dtype=torch.int32, device=dev)
        words = torch.full((nb, max(n_words, 1), max(n_pos, 1)), -1, dtype=torch.int32, device=dev)
        words[:, 0, 0] = pos
        outs = [torch.full((nb,), 7.0, device=dev), torch.full((nb,), 7, dtype=torch.int32, device=dev),
                torch.full((nb, 9), 7, dtype=torch.int32, device=dev), torch.full((nb, 9, max(T, 1)), 7.0, device=dev)]
        rc = L.lib().tb_excite_loss(L.ptr(A), L.ptr(lst), L.ptr(words), nb, T, h, w, n_words, n_pos, loss_scale, check,
                                    *[L.ptr(o) for o in outs], L.stream())
        torch.cuda.synchronize()
        return rc, all(bool((o == 7).all()) for o in outs)

    rc, untouched = call()
    assert rc == 0 and not untouched
    for kw in (dict(h=1), dict(w=1), dict(T=129), dict(T=1), dict(pos=4), dict(pos=0), dict(pos=-2), dict(last=9), dict(last=0), dict(n_words=9),
               dict(n_pos=17), dict(h=64, w=64), dict(loss_scale=0.0), dict(check=2)):
        rc, untouched = call(**kw)
        assert rc == TB_EINVAL and untouched, kw
    rc, untouched = call(pos=4, check=0)         # unchecked: the kernel ignores the position -- no word is left
    assert rc == 0 and not untouched


# ------------------------------------------------------------------------------------------------------------------ tb_excite_bwd
BWD_CASES = [(2, 8, 64, 77, 40), (2, 5, 100, 77, 64), (1, 8, 36, 77, 160), (2, 2, 16, 33, 80), (1, 1, 4, 1, 8)]
BWD_COEF_LAYERS = 5


def _bwd_inputs(case, seed, dtype, nb=None):
    B, H, Sq, Skv, hd = case
    nb = B if nb is None else nb
    gen = torch.Generator().manual_seed(seed)
    Q = torch.randn(B * Sq, H * hd, generator=gen).to(dtype)
    K = torch.randn(B * Skv, H * hd, generator=gen).to(dtype)
    sel = torch.full((nb, 9), -1, dtype=torch.int32)
    for b in range(nb):       # 9 positions, or fewer on a small map and in every second image (reflect folding), ascending
        n = min(Sq, 9 if b % 2 == 0 else 6)
        sel[b, :n] = torch.sort(torch.randperm(Sq, generator=gen)[:n]).values.to(torch.int32)
    dA = torch.randn(nb, 9, Skv, generator=gen) * 50.0       # |loss_scale 100 kappa pt (1 - M)| of a 256-scaled loss
    return Q, K, sel, dA


def _bwd_launch(Q, K, sel, dA, case, coef, dq0=None, b0=0, nb=None):
    from textboost_amd import ops
    B, H, Sq, Skv, hd = case
    q, k = Q.to(dev), K.to(dev)
    dq = torch.zeros_like(q) if dq0 is None else dq0.to(dev)
    ops.excite_bwd(q, k, dq, sel.to(dev), dA.to(dev), B, H, Sq, Skv, hd, coef, b0=b0, nb=nb)
    return dq.cpu()


@pytest.mark.parametrize("half", ["fp16", "bf16"])
@pytest.mark.parametrize("case", BWD_CASES, ids=lambda c: "x".join(map(str, c)))
def test_bwd_kernel_matches_the_float64_reference(case, half):
    from tests.test_gpu_attn_loss import _check, _same_bits
    from textboost_amd import _lib as L
    B, H, Sq, Skv, hd = case
    scale, coef = hd ** -0.5, 1.0 / (BWD_COEF_LAYERS * H)
    with L.use_half(half):
        dt = L.half_dtype()
        Q, K, sel, dA = _bwd_inputs(case, 7, dt)
        ref = R.excite_dq_ref(Q, K, sel, dA, B, H, Sq, Skv, hd, scale, coef)
        r32 = R.excite_dq_ref(Q, K, sel, dA, B, H, Sq, Skv, hd, scale, coef, dtype=torch.float32)
        yard = (r32.double() - ref).abs().max().item()
        tag = f"excite bwd {half} {case}"
        dq = _bwd_launch(Q, K, sel, dA, case, coef)
        _check(tag + " dQ", dq, ref, yard, half)
        gen = torch.Generator().manual_seed(99)
        dq0 = (torch.randn(ref.shape, generator=gen) * max(ref.abs().max().item(), 1e-3)).to(dt)
        dq0[::3, ::5] = -0.0                                    # "bit-unchanged" includes the sign of a zero
        dq1 = _bwd_launch(Q, K, sel, dA, case, coef, dq0)
        _check(tag + " dQ prefilled", dq1, dq0.double() + ref, yard, half, 1)
        rows = torch.zeros(B * Sq, dtype=torch.bool)
        for b in range(B):
            rows[[b * Sq + int(s) for s in sel[b] if s >= 0]] = True
        assert _same_bits(dq1[~rows], dq0[~rows]) and (dq[~rows] == 0).all()        # rows that are not selected
        assert _same_bits(_bwd_launch(Q, K, sel, dA, case, coef, dq0), dq1)         # a relaunch on the same inputs
        if Skv == 1:      # p = 1, so ds = dA - dA = 0: exactly nothing is added
            assert _same_bits(dq1, dq0) and (dq == 0).all()
        else:
            assert not torch.equal(dq1[rows], dq0[rows])


@pytest.mark.parametrize("half", ["fp16", "bf16"])
def test_bwd_kernel_image_range_empty_selection_and_unaligned_rows(half):
    from tests.test_gpu_attn_loss import _check, _same_bits
    from textboost_amd import _lib as L
    from textboost_amd import ops
    case = B, H, Sq, Skv, hd = (3, 2, 36, 77, 40)
    C = H * hd
    scale, coef = hd ** -0.5, 1.0 / (BWD_COEF_LAYERS * H)
    with L.use_half(half):
        dt = L.half_dtype()
        Q, K, sel, dA = _bwd_inputs(case, 21, dt, nb=2)           # the images [1, 3)
        sel[1] = -1                                              # image 2: nothing selected (its loss is zero)
        ref = R.excite_dq_ref(Q, K, sel, dA, B, H, Sq, Skv, hd, scale, coef, b0=1, nb=2)
        r32 = R.excite_dq_ref(Q, K, sel, dA, B, H, Sq, Skv, hd, scale, coef, b0=1, nb=2, dtype=torch.float32)
        yard = (r32.double() - ref).abs().max().item()
        gen = torch.Generator().manual_seed(5)
        dq0 = torch.randn(B * Sq, C, generator=gen).to(dt)
        dq0[::7, ::5] = -0.0
        dq = _bwd_launch(Q, K, sel, dA, case, coef, dq0, b0=1, nb=2)
        assert _same_bits(dq[:Sq], dq0[:Sq]) and _same_bits(dq[2 * Sq:], dq0[2 * Sq:])        # b outside [b0, b0 + nb), and the empty selection
        assert not torch.equal(dq[Sq:2 * Sq], dq0[Sq:2 * Sq])
        _check(f"excite bwd {half} image range", dq, dq0.double() + ref, yard, half, 1)
        # q / dq column slices at an odd element offset of buffers with an odd row pitch: the rows are 2-byte aligned only
        outs = []
        for _ in range(2):
            qbuf = torch.full((B * Sq, C + 7), 3.0, dtype=dt)
            kbuf = torch.full((B * Skv, 3 * C + 5), 3.0, dtype=dt)
            qbuf[:, 3:3 + C] = Q
            kbuf[:, C + 1:2 * C + 1] = K
            qd, kd = qbuf.to(dev), kbuf.to(dev)
            dqb = torch.full((B * Sq, C + 3), 5.0, dtype=dt, device=dev)
            dqv = dqb[:, 1:1 + C]
            dqv.zero_()
            ops.excite_bwd(qd[:, 3:3 + C], kd[:, C + 1:2 * C + 1], dqv, sel.to(dev), dA.to(dev), B, H, Sq, Skv, hd, coef, b0=1, nb=2)
            outs.append(dqb.cpu())
        assert torch.equal(outs[0], outs[1]) and (outs[0][:, 0] == 5).all() and (outs[0][:, 1 + C:] == 5).all()
        _check(f"excite bwd {half} unaligned", outs[0][:, 1:1 + C], ref, yard, half)


def test_bwd_kernel_refusals_touch_nothing():
    from textboost_amd import _lib as L
    B, H, Sq, Skv, hd = 2, 2, 32, 16, 16

    def call(hd=hd, Skv=Skv, dtype=L.TB_F16, b0=0, nb=B, ld=None, tdtype=torch.float16, coef=1.0):
        C = H * max(hd, 1)
        gen = torch.Generator().manual_seed(1)
        q = torch.randn(B * Sq, C, generator=gen).to(tdtype).to(dev)
        k = torch.randn(B * Skv, C, generator=gen).to(tdtype).to(dev)
        dq = torch.full_like(q, 2.0)
        d = L.AttnDesc()
        d.B, d.H, d.Sq, d.Skv, d.hd, d.causal, d.scale = B, H, Sq, Skv, hd, 0, 0.25
        d.Q, d.ldq, d.K, d.ldk, d.dQ, d.lddq = L.ptr(q), C, L.ptr(k), C, L.ptr(dq), C if ld is None else ld
        sel = torch.zeros(B, 9, dtype=torch.int32, device=dev)
        sel[:, 1:] = -1
        dA = torch.rand(B, 9, Skv, device=dev)
        rc = L.lib().tb_excite_bwd(d, dtype, b0, nb, L.ptr(sel), L.ptr(dA), coef, L.stream())
        torch.cuda.synchronize()
        return rc, bool((dq == 2).all())

    rc, untouched = call()
    assert rc == 0 and not untouched
    for kw in (dict(hd=12), dict(hd=168), dict(Skv=129), dict(dtype=L.TB_F32, tdtype=torch.float32), dict(b0=1, nb=2), dict(nb=0), dict(b0=-1),
               dict(ld=H * hd - 8), dict(coef=float("nan"))):
        rc, untouched = call(**kw)
        assert rc == TB_EINVAL and untouched, kw


# ------------------------------------------------------------------------------------------------------------------ tb_excite_update
@pytest.mark.parametrize("half", ["fp16", "bf16"])
def test_update_kernel_is_exact_and_guarded(half):
    from textboost_amd import _lib as L
    from textboost_amd import ops
    B, shape = 4, (4, 8, 12)
    with L.use_half(half):
        dt = L.half_dtype()
        gen = torch.Generator().manual_seed(3)
        x0 = torch.randn(B, *shape, generator=gen)
        x0[3, 0, 0, :4] = -0.0
        g = (torch.randn(B, *shape, generator=gen) * 300.0).to(dt)
        g[1, 2, 3, 4] = float("inf")
        g[3, 1, 1, 1] = float("nan")                             # (image 3 has step 0: not looked at)
        step = torch.tensor([2.5, 1.0, 0.75, 0.0])
        x, x2 = x0.clone().to(dev), torch.full((2 * B, *shape), 7.0, dtype=dt, device=dev)
        bad = torch.full((B,), 9, dtype=torch.int32, device=dev)
        ops.excite_update(x, g.to(dev), step.to(dev), x2, bad, 256.0)
        want, wbad = R.update_ref(x0.numpy(), g.float().numpy(), step.numpy(), 256.0)
        got = x.cpu()
        assert bad.tolist() == wbad.tolist() == [0, 1, 0, 0]
        assert np.array_equal(got.numpy().view(np.uint32), want.view(np.uint32))               # bit-equal to the fma-free fp32 expression
        for b in (1, 3):      # the image with an inf in g and the image with step 0: x and both of its x2 rows untouched
            assert np.array_equal(got[b].numpy().view(np.uint32), x0[b].numpy().view(np.uint32))
            assert (x2[b] == 7).all() and (x2[B + b] == 7).all()
        for b in (0, 2):
            assert not torch.equal(got[b], x0[b])
            assert torch.equal(x2[b].cpu(), got[b].to(dt)) and torch.equal(x2[B + b].cpu(), got[b].to(dt))
        for kw in (dict(n=0), dict(B=0), dict(ls=0.0)):
            rc = L.lib().tb_excite_update(L.ptr(x), L.ptr(g.to(dev)), L.ptr(step.to(dev)), L.ptr(x2), L.ptr(bad), kw.get("n", 8), kw.get("B", B),
                                          kw.get("ls", 1.0), L.stream())
            assert rc == TB_EINVAL, kw


# ------------------------------------------------------------------------------------------------------------------ conv_in's input gradient
@pytest.mark.parametrize("half", ["fp16", "bf16"])
@pytest.mark.parametrize("shape", [(2, 16, 16, 64), (1, 6, 10, 64)], ids=["mfma", "valu"])
def test_conv_in_input_gradient_matches_conv_transpose2d(shape, half):
    """(B, H, W, C): W % 16 == 0 takes tb_conv_to4's MFMA variant, 6 x 10 the VALU one.  Bound: the fp32 accumulation of 9 C products,
    2 (9 C) 2^-24 sum |w| |g|, plus half an ulp of the 16-bit output."""
    from tests.test_gpu_attn_loss import _half_ulp
    from textboost_amd import _lib as L
    from textboost_amd import ops
    from textboost_amd.unet import pack_conv4_dgrad
    B, H, W, C = shape
    with L.use_half(half):
        dt = L.half_dtype()
        gen = torch.Generator().manual_seed(4)
        wgt = (torch.randn(C, 4, 3, 3, generator=gen) * 0.1).to(dt).float()         # conv_in.weight, representable in the build's 16-bit type
        g = torch.randn(B, C, H, W, generator=gen).to(dt)
        ref = torch.nn.functional.conv_transpose2d(g.double(), wgt.double(), padding=1)
        mag = torch.nn.functional.conv_transpose2d(g.double().abs(), wgt.double().abs(), padding=1)
        g_nhwc = g.permute(0, 2, 3, 1).reshape(B * H * W, C).contiguous().to(dev)
        out = torch.full((B, 4, H, W), 7.0, dtype=dt, device=dev)
        ops.conv_to4(g_nhwc, pack_conv4_dgrad(wgt).to(dev), None, out, B, H, W, C)
        got = out.cpu().double()
        bound = 2 * (9 * C) * 2.0 ** -24 * mag + _half_ulp(ref, half)
        err = (got - ref).abs()
        print(f"[excite] conv_in gradient {half} {shape}: max err {err.max().item():.3e}, worst err / bound {(err / bound).max().item():.3f}")
        assert (err <= bound).all()


# ------------------------------------------------------------------------------------------------------------------ HipUNet.backward_sample
def _tiny(sd2):
    from tests.test_gpu_model import make_unet
    ref, hip, cfg = make_unet(2, 16, 64, sd2=sd2)
    twin = R.tiny_oracle(sd2)
    for (n, p), (n2, p2) in zip(ref.state_dict().items(), twin.state_dict().items()):
        assert n == n2 and torch.equal(p, p2), n              # tests/test_excite_host.py checked the margins on the same weights
    return ref, hip


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-300)).item()


@pytest.mark.parametrize("sd2", [False, True], ids=["sd1", "sd2"])
def test_backward_sample_matches_oracle_autograd_and_leaves_backward_alone(sd2):
    from oracle.fp16_mode import fp16_rounding
    B, hw, D = 2, 16, 64
    ref, hip = _tiny(sd2)
    x, t, ehs = R.unet_inputs(sd2=sd2)
    g = torch.Generator().manual_seed(2)
    dpred = torch.randn(B, 4, hw, hw, generator=g)
    xs = x.clone().requires_grad_(True)
    ref(xs, t, ehs).backward(dpred)
    x16 = x.clone().requires_grad_(True)
    with fp16_rounding():
        ref(x16, t, ehs).backward(dpred.half().float())
    f = _rel(x16.grad, xs.grad)
    args = (x.half().to(dev), t.to(dev), ehs.half().view(B * 77, D).to(dev).contiguous())
    pred0 = hip.forward(*args).clone()
    d_ehs0 = hip.backward(dpred.to(dev)).clone()              # before the new path has run once
    hip.forward(*args)
    d_sample = hip.backward_sample(dpred.to(dev)).clone()
    e = _rel(d_sample, xs.grad)
    print(f"[excite] backward_sample sd2={sd2}: d_sample rel err {e:.3e}, fp16-faithful oracle {f:.3e}")
    assert tuple(d_sample.shape) == (B, 4, hw, hw) and torch.isfinite(d_sample.float()).all()
    assert e < f
    hip.enable_excite(rows=(0, 2))                           # enabled, not recording: forward / backward launch what they launched
    assert torch.equal(hip.forward(*args), pred0)
    assert torch.equal(hip.backward(dpred.to(dev)), d_ehs0)
    assert torch.equal(hip.backward_sample(dpred.to(dev)), d_sample)
    with pytest.raises(ValueError, match="truncated tape"):
        hip.backward_sample()
    hip.forward(*args, until="excite")
    with pytest.raises(ValueError, match="needs a full forward"):
        hip.backward_sample(dpred.to(dev))


def test_enable_excite_refusals():
    from tests.test_gpu_model import make_unet
    from textboost_amd import models
    from textboost_amd.unet import HipUNet, UNetGeometry
    _, hip, cfg = make_unet(2, 16, 64)
    with pytest.raises(RuntimeError, match="enable_excite"):
        hip.forward(None, None, None, until="excite")
    with pytest.raises(ValueError, match="only \"excite\""):
        hip.forward(None, None, None, until="mid")
    with pytest.raises(ValueError, match="rows"):
        hip.enable_excite(rows=(1, 3))
    ex = hip.enable_excite()
    assert (ex.b0, ex.nb, ex.n, ex.h, ex.w) == (1, 1, 5, 4, 4) and ex.last_layer == "up_blocks.1.attentions.2.transformer_blocks.0.attn2"
    _, hip8, _ = make_unet(2, 8, 64)                          # 8 x 8 latents: a 2 x 2 map on level 2 still works, 1 x 1 does not exist
    assert hip8.enable_excite().h == 2
    geo = UNetGeometry(block_out_channels=cfg.block_out_channels, num_heads=cfg.num_heads, cross_attention_dim=64,
                       cross_attn_levels=(True, True, False, False))
    sd = {k: v for k, v in hip_state(cfg, geo).items()}
    with pytest.raises(ValueError, match="level 2"):
        HipUNet(geo, sd, 2, 16, 16, device=dev).enable_excite()
    with pytest.raises(NotImplementedError, match="16-bit"):
        HipUNet(geo, sd, 2, 16, 16, device=dev, dtype=torch.float32).enable_excite()


def hip_state(cfg, geo):
    """a state dict of the oracle UNet with `geo`'s cross-attention levels"""
    import copy
    from oracle.unet_sd import UNet2DCondition
    c = copy.copy(cfg)
    c.cross_attn_levels = geo.cross_attn_levels
    torch.manual_seed(0)
    return UNet2DCondition(c).state_dict()


# ------------------------------------------------------------------------------------------------------------------ the excite pass
def _oracle_pass(ref, x, t, ehs, rounding=False):
    """-> (d sum_b L_b / d sample, [reference dicts per image]) of the oracle; rounding: the UNet's forward and backward run fp16-faithful
    (oracle/fp16_mode.py) from `sample` to the q / k of the supervised layers and back, while the softmax of those layers and the loss are
    float64 on the rounded q / k, as the HIP path computes them on its 16-bit q / k"""
    import contextlib
    from oracle.fp16_mode import fp16_rounding
    ctx = fp16_rounding() if rounding else contextlib.nullcontext()
    xs = x.clone().requires_grad_(True)
    with ctx:
        _, _, names, qk = R.oracle_maps(ref, xs, t, ehs)
    assert len(names) == 5
    leaves = [(q.detach().double().requires_grad_(True), k.detach().double()) for q, k in qk]
    A = R.maps_from_qk(leaves, ref.cfg.heads(2))
    L = sum(R.loss_torch(A[b], R.UNET_LAST, R.UNET_WORDS, 4, 4) for b in range(A.shape[0]))
    L.backward()
    with ctx:
        torch.autograd.backward([q for q, _ in qk], [lq.grad.to(q.dtype) for (lq, _), (q, _) in zip(leaves, qk)])
    refs = [R.excite_loss_ref(A[b].detach(), R.UNET_LAST, R.UNET_WORDS, 4, 4) for b in range(A.shape[0])]
    return xs.grad, refs


def _hip_pass(hip, args, loss_scale, full=False):
    if full:
        hip.excite.record = True
        try:
            hip.forward(*args)
        finally:
            hip.excite.record = False
    else:
        assert hip.forward(*args, until="excite") is None
    hip.excite_loss(loss_scale, check=True)
    ex = hip.excite
    out = dict(loss=ex.loss.cpu(), word=ex.word.cpu().tolist(), sel=ex.sel.cpu().tolist(), A=ex.acc.cpu())
    if full:
        d = hip.backward_sample(torch.zeros(hip.B, 4, hip.H, hip.W, device=dev), excite=True)
    else:
        d = hip.backward_sample()
    out["d"] = d.float().cpu() / loss_scale
    return out


@pytest.mark.parametrize("sd2", [False, True], ids=["sd1", "sd2"])
def test_excite_pass_matches_oracle_autograd_of_the_loss(sd2):
    B, D = 2, 64
    ref, hip = _tiny(sd2)
    x, t, ehs = R.unet_inputs(sd2=sd2)
    g_ref, refs = _oracle_pass(ref, x, t, ehs)
    g_16, refs16 = _oracle_pass(ref, x, t, ehs, rounding=True)
    f = _rel(g_16, g_ref)
    print(f"[excite] pass sd2={sd2}: fp16-faithful oracle vs fp32 oracle {f:.3e}; its selection "
          f"{'equals' if [r['sel'] for r in refs16] == [r['sel'] for r in refs] else 'DIFFERS from'} the fp32 oracle's")
    ex = hip.enable_excite(rows=(0, 2))
    ex.words.copy_(_table(R.UNET_WORDS, B))
    ex.last.fill_(R.UNET_LAST)
    args = (x.half().to(dev), t.to(dev), ehs.half().view(B * 77, D).to(dev).contiguous())
    outs = {ls: _hip_pass(hip, args, ls) for ls in (1.0, 256.0, 4096.0)}
    for ls, o in outs.items():
        for b in range(B):         # the selection is pinned to the reference's: equal by the margin condition
            assert o["word"][b] == refs[b]["word"] and o["sel"][b] == refs[b]["sel"], (ls, b, o["sel"][b], refs[b]["sel"])
            assert abs(o["loss"][b].item() - refs[b]["loss"]) <= 2e-2 * refs[b]["loss"]
        e = _rel(o["d"], g_ref)
        zeros = (o["d"] == 0).float().mean().item()
        print(f"[excite] pass sd2={sd2} loss_scale {ls:g}: d_sample rel err {e:.3e} (yardstick {f:.3e}), zero elements {zeros:.3f}, "
              f"losses {o['loss'].tolist()}")
        assert torch.isfinite(o["d"]).all() and e < f, (ls, e, f)
    assert _rel(outs[1.0]["d"], outs[256.0]["d"]) < f and _rel(outs[4096.0]["d"], outs[256.0]["d"]) < f
    # the truncated pass against the same pass on a full forward, started from a zero dpred
    full = _hip_pass(hip, args, 256.0, full=True)
    e_full = _rel(full["d"], g_ref)
    print(f"[excite] pass sd2={sd2}: full forward + zero dpred rel err {e_full:.3e}, truncated vs full {_rel(outs[256.0]['d'], full['d']):.3e}")
    assert torch.equal(full["A"], outs[256.0]["A"]) and full["sel"] == outs[256.0]["sel"]
    assert _rel(outs[256.0]["d"], full["d"]) < f and e_full < f
    again = _hip_pass(hip, args, 256.0)
    assert torch.equal(again["d"], outs[256.0]["d"]) and torch.equal(again["loss"], outs[256.0]["loss"])         # a relaunch: the same bits
    assert not hip.excite.record and not hip.excite.inject and not hip._bwd_through


def test_one_update_descends_as_the_reference_does():
    """eta is chosen on the CPU: the largest of 2^k (k = 12 .. -4) at which the float64 loss of BOTH images falls along the oracle's own
    gradient; the loss recomputed by the HIP path after one tb_excite_update with that step must fall by at least half as much"""
    from textboost_amd import ops
    B, D = 2, 64
    ref, hip = _tiny(False)
    x, t, ehs = R.unet_inputs(sd2=False)
    g_ref, refs = _oracle_pass(ref, x, t, ehs)
    eta = drop = None
    for k in range(12, -5, -1):
        with torch.no_grad():
            A, _, _, _ = R.oracle_maps(ref, x - 2.0 ** k * g_ref, t, ehs)
        after = [R.excite_loss_ref(A[b], R.UNET_LAST, R.UNET_WORDS, 4, 4)["loss"] for b in range(B)]
        d = [refs[b]["loss"] - after[b] for b in range(B)]
        if min(d) > 0:
            eta, drop = 2.0 ** k, d
            break
    assert eta is not None
    ex = hip.enable_excite(rows=(0, 2))
    ex.words.copy_(_table(R.UNET_WORDS, B))
    ex.last.fill_(R.UNET_LAST)
    ls = 256.0
    xf = x.clone().to(dev)
    x2 = torch.cat([x, x]).half().to(dev)
    tt, e16 = t.to(dev), ehs.half().view(B * 77, D).to(dev).contiguous()
    hip.forward(x2[:B], tt, e16, until="excite")
    before = hip.excite_loss(ls).cpu().clone()
    bad = torch.zeros(B, dtype=torch.int32, device=dev)
    ops.excite_update(xf, hip.backward_sample(), torch.full((B,), eta, device=dev), x2, bad, ls)
    assert bad.tolist() == [0, 0] and torch.equal(x2[:B], x2[B:])
    hip.forward(x2[:B], tt, e16, until="excite")
    after = hip.excite_loss(ls).cpu()
    for b in range(B):
        fall = (before[b] - after[b]).item()
        print(f"[excite] descent image {b}: eta {eta:g}, reference loss falls by {drop[b]:.4e}, HIP path {before[b].item():.5f} -> "
              f"{after[b].item():.5f} ({fall:.4e})")
        assert fall >= 0.5 * drop[b]


# ------------------------------------------------------------------------------------------------------------------ sampler, command line
@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    from tests import test_gpu_sweep as TS
    from tests.test_compose_host import write_run
    from tests.test_gpu_generate import D_TEXT
    from textboost_amd import generate as G
    root = tmp_path_factory.mktemp("excite")
    mdir = TS._prepare(str(root))
    da, db = str(root / "runs" / "dog"), str(root / "runs" / "cat")
    write_run(da, ["<dog>"], ["<hflip>"], seed=1, rank=4, keep_rows="even")
    write_run(db, ["<cat>"], [], seed=2, rank=4, keep_rows="odd")
    B = 2
    with torch.no_grad():
        pipe = G.Pipeline.from_model_dir(mdir, B, steps=4, guidance=7.5, device=dev)
    g = torch.Generator().manual_seed(3)
    cond = torch.randn(B * 77, D_TEXT, generator=g).half().float().to(dev)
    uncond = torch.randn(77, D_TEXT, generator=g).half().float().repeat(B, 1).to(dev)
    lat = torch.cat([G.seeded_latent(s, 16) for s in (0, 1)]).to(dev)
    return dict(root=root, mdir=mdir, da=da, db=db, pipe=pipe, B=B, cond=cond, uncond=uncond, lat=lat)


def test_sampler_with_and_without_excite(tiny):
    from textboost_amd.attn_maps import AttnMapRecorder
    from textboost_amd.excite import ExciteControl
    pipe = tiny["pipe"]
    args = (tiny["cond"], tiny["uncond"])
    with torch.no_grad():
        plain = pipe.sampler.denoise(*args, latents=tiny["lat"]).clone()
        assert torch.equal(pipe.sampler.denoise(*args, latents=tiny["lat"], excite=None), plain)
        ctl = ExciteControl(pipe.unet, [[2], [5, 6]], 9, words=["dog", "cat"], max_refine=2)
        out = pipe.sampler.denoise(*args, latents=tiny["lat"], excite=ctl).clone()
        trace = [dict(e) for e in ctl.trace]
        assert torch.isfinite(out).all() and not torch.equal(out[0], plain[0]) and not torch.equal(out[1], plain[1])
        # 4 steps at excite_steps 0.5: steps 0 and 1, both refinement steps at N = 4 (thresholds 0.5 and 0.8), at most 2 updates each
        assert [e["step"] for e in trace] == [0, 1] and [e["threshold"] for e in trace] == [0.5, 0.8]
        for e in trace:
            assert 0 <= e["iterations"] <= 2 and len(e["loss_before"]) == len(e["loss_after"]) == len(e["word"]) == 2
            assert all(0.0 <= l <= 1.0 for l in e["loss_before"] + e["loss_after"]) and all(w in (0, 1) for w in e["word"]) and e["skipped"] == 0
        assert trace[0]["step_size"] == 20.0 and abs(trace[1]["step_size"] - 20.0 * (1.0 - 0.5 / 3.0) ** 0.5) < 1e-12
        assert sum(e["iterations"] for e in trace) >= 1 and ctl.skipped == 0
        print("[excite] sampler trace: " + json.dumps(trace))
        assert torch.equal(pipe.sampler.denoise(*args, latents=tiny["lat"], excite=ctl), out)                # a second run: the same bits
        assert [dict(e) for e in ctl.trace] == trace
        off = ExciteControl(pipe.unet, [[2], [5, 6]], 9, refine=False)
        o2 = pipe.sampler.denoise(*args, latents=tiny["lat"], excite=off).clone()
        assert torch.isfinite(o2).all() and not torch.equal(o2, plain) and not torch.equal(o2, out)
        assert [e["iterations"] for e in off.trace] == [1, 1] and all(e["loss_after"] is None and len(e["loss_before"]) == 2 for e in off.trace)
        none = ExciteControl(pipe.unet, [[2], [5, 6]], 9, excite_steps=0.0)
        assert torch.equal(pipe.sampler.denoise(*args, latents=tiny["lat"], excite=none), plain) and none.trace == []
        with pytest.raises(ValueError, match="does not go with maps"):
            pipe.sampler.denoise(*args, latents=tiny["lat"], excite=ctl, maps=AttnMapRecorder(pipe.unet))
        for kw in (dict(regions=object()), dict(p2p=object()), dict(pin=object())):
            with pytest.raises(ValueError, match="does not go with " + list(kw)[0]):
                pipe.sampler.denoise(*args, latents=tiny["lat"], excite=ctl, **kw)
        assert torch.equal(pipe.sampler.denoise(*args, latents=tiny["lat"]), plain)                          # nothing is left behind
        rgbx = pipe.images(*args, tiny["lat"], excite=ctl)
        assert rgbx.shape[0] == 2 and rgbx.dtype == torch.int32


def test_cli_excite_writes_the_grid_and_the_report(tiny):
    pytest.importorskip("transformers")
    from PIL import Image
    wd = str(tiny["root"] / "cli")
    os.makedirs(wd)
    cmd = [tiny["da"], "--with", tiny["db"], "--model", tiny["mdir"], "--prompt", "a <dog> dog and a <cat> cat", "--seeds", "0", "1", "--steps", "4",
           "--output", "g.png", "--excite", "<dog>", "<cat>"]
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, os.path.join(ROOT, "inference.py")] + cmd, capture_output=True, text=True, cwd=wd)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "wrote g_excite.json: 2 guided step(s)" in r.stdout
    grid = np.asarray(Image.open(os.path.join(wd, "g.png")))
    assert grid.shape == (128, 2 * 128, 3)
    with open(os.path.join(wd, "g_excite.json")) as f:
        rep = json.load(f)
    assert rep["words"] == ["<dog>", "<cat>"] and rep["seeds"] == [0, 1] and len(rep["positions"]) == 2 and rep["loss_scale"] == 256.0
    assert [e["step"] for e in rep["steps"]] == [0, 1] and all(len(e["loss_before"]) == 2 and len(e["word"]) == 2 for e in rep["steps"])
