"""The cross-attention localisation loss on the GPU (--attn_loss_weight): the kernels of csrc/attn_loss.hip against the float64
references of tests/attn_loss_ref.py, the step against the oracle step with the loss, the captured graph, the feeder and the command line.

Kernel bound: the fp32 CPU evaluation of the same gradient (attn_loss_ref(dtype=float32)) has a maximum error against float64 on the same
operands; every element of the kernel's dQ / dK must lie within 8 x that yardstick (the convention of tests/test_gpu_attn_maps.py) plus half an
ulp of the output dtype at the reference value (2^-11 relative for fp16, 2^-8 for bf16; fp16's subnormal spacing below 2^-14)."""
import numpy as np
import pytest
import torch

import attn_loss_ref as R

pytestmark = pytest.mark.gpu
dev = "cuda"
TB_EINVAL = -22
MARGIN = 8.0
CASES = [(2, 8, 64, 77, 40), (2, 5, 100, 77, 64), (1, 8, 36, 77, 160), (2, 2, 64, 33, 80), (2, 2, 96, 128, 64), (1, 1, 1, 1, 8)]
COEF = 0.05   # lambda / (B * supervised layers) of the kernel cases


def _half_ulp(ref, half):
    a = ref.abs()
    return torch.clamp(a * 2.0 ** -11, min=2.0 ** -25) if half == "fp16" else a * 2.0 ** -8


def _inputs(case, seed, dtype, qk_gain=1.0):
    B, H, Sq, Skv, hd = case
    gen = torch.Generator().manual_seed(seed)
    Q = (torch.randn(B * Sq, H * hd, generator=gen) * qk_gain).to(dtype)
    K = (torch.randn(B * Skv, H * hd, generator=gen) * qk_gain).to(dtype)
    g = torch.rand(B, Sq, generator=gen) * 2 - 1
    tok_w = torch.zeros(B, Skv)
    for b in range(B):   # 1 to 3 ones per sample
        n = min(Skv, 1 + (seed + b) % 3)
        tok_w[b, torch.randperm(Skv, generator=gen)[:n]] = 1.0
    return Q, K, tok_w, g


def _launch(Q, K, tok_w, g, case, coef, loss_scale, dq0=None, dk0=None):
    """-> (dq, dk, partial sum) on the host"""
    from textboost_amd import ops
    B, H, Sq, Skv, hd = case
    q, k = Q.to(dev), K.to(dev)
    dq = torch.zeros_like(q) if dq0 is None else dq0.to(dev)
    dk = torch.zeros_like(k) if dk0 is None else dk0.to(dev)
    ws = ops.attn_loss_workspace(dev, B, H, 2)
    ws.fill_(float("nan"))
    ls = torch.tensor([loss_scale], device=dev) if loss_scale is not None else None
    ops.attn_loss_bwd(q, k, dq, dk, tok_w.to(dev), g.to(dev), B, H, Sq, Skv, hd, coef, ls, ws, 1)
    part = ws.cpu()
    assert torch.isnan(part[0]).all()                   # the other slot is not this launch's
    return dq.cpu(), dk.cpu(), part[1].double().sum().item()


def _check(name, got, ref, yard, half, extra_half_ulps=0):
    bound = MARGIN * yard + (1 + extra_half_ulps) * _half_ulp(ref, half)
    err = (got.double() - ref).abs()
    rel = err / bound
    ratio, at = rel.max().item(), np.unravel_index(int(rel.argmax()), rel.shape)
    print(f"[attn loss] {name}: max err {err.max().item():.3e}, fp32 yardstick {yard:.3e}, worst err / bound {ratio:.3f} at {at} "
          f"(got {got[at].item():.9g}, reference {ref[at].item():.9g})")
    assert torch.isfinite(got.float()).all()
    assert (err <= bound).all(), (name, ratio)


@pytest.mark.parametrize("loss_scale", [1.0, 65536.0])
@pytest.mark.parametrize("half", ["fp16", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_kernel_matches_the_float64_reference(case, half, loss_scale):
    from textboost_amd import _lib as L
    B, H, Sq, Skv, hd = case
    scale = hd ** -0.5
    with L.use_half(half):
        dt = L.half_dtype()
        Q, K, tok_w, g = _inputs(case, 7, dt)
        c = COEF * loss_scale
        tot, dq_ref, dk_ref = R.attn_loss_ref(Q, K, tok_w, g, H, scale, c)
        tot32, dq32, dk32 = R.attn_loss_ref(Q, K, tok_w, g, H, scale, c, dtype=torch.float32)
        yq, yk = (dq32.double() - dq_ref).abs().max().item(), (dk32.double() - dk_ref).abs().max().item()
        # zero-filled outputs
        dq, dk, part = _launch(Q, K, tok_w, g, case, COEF, loss_scale)
        tag = f"{half} {case} scale {loss_scale:g}"
        _check(tag + " dQ", dq, dq_ref, yq, half)
        _check(tag + " dK", dk, dk_ref, yk, half)
        # the loss value: N = the number of summed terms
        N = B * H * Sq * Skv
        rel = abs(part - tot.item()) / max(abs(tot.item()), 1e-300)
        print(f"[attn loss] {tag} loss {part:.9e} vs {tot.item():.9e}: rel err {rel:.3e}, bound {N * 2.0 ** -23:.3e}")
        assert rel <= N * 2.0 ** -23
        # outputs that hold a gradient already: rounded(float(old) + add)
        gen = torch.Generator().manual_seed(99)
        mag = max(dq_ref.abs().max().item(), dk_ref.abs().max().item(), 1e-3)
        dq0 = (torch.randn(dq_ref.shape, generator=gen) * mag).to(dt)
        dk0 = (torch.randn(dk_ref.shape, generator=gen) * mag).to(dt)
        dq1, dk1, _ = _launch(Q, K, tok_w, g, case, COEF, loss_scale, dq0, dk0)
        _check(tag + " dQ prefilled", dq1, dq0.double() + dq_ref, yq, half, 1)
        _check(tag + " dK prefilled", dk1, dk0.double() + dk_ref, yk, half, 1)
        if case == (1, 1, 1, 1, 8):   # p = 1, so tok_w - P_J = 0: exactly nothing is added
            assert torch.equal(dq1, dq0) and torch.equal(dk1, dk0)
            assert (dq == 0).all() and (dk == 0).all()


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))     # (torch.equal alone takes -0 for +0)


@pytest.mark.parametrize("half", ["fp16", "bf16"])
def test_sample_without_placeholder_and_zero_g_leave_their_rows_bit_unchanged(half):
    from textboost_amd import _lib as L
    case = B, H, Sq, Skv, hd = (2, 5, 100, 77, 64)
    with L.use_half(half):
        dt = L.half_dtype()
        Q, K, tok_w, g = _inputs(case, 21, dt)
        gen = torch.Generator().manual_seed(5)
        dq0 = torch.randn(B * Sq, H * hd, generator=gen).to(dt)
        dk0 = torch.randn(B * Skv, H * hd, generator=gen).to(dt)
        dq0[::7, ::5] = -0.0                            # "bit-unchanged" includes the sign of a zero
        dk0[::3, ::4] = -0.0
        tw = tok_w.clone()
        tw[1] = 0                                       # sample 1 has no placeholder token
        dq, dk, _ = _launch(Q, K, tw, g, case, COEF, 65536.0, dq0, dk0)
        assert _same_bits(dq[Sq:], dq0[Sq:]) and _same_bits(dk[Skv:], dk0[Skv:])
        assert not torch.equal(dq[:Sq], dq0[:Sq]) and not torch.equal(dk[:Skv], dk0[:Skv])
        g0 = g.clone()
        g0[0] = 0                                       # sample 0 has zero coefficients
        dq, dk, _ = _launch(Q, K, tok_w, g0, case, COEF, 65536.0, dq0, dk0)
        assert _same_bits(dq[:Sq], dq0[:Sq]) and _same_bits(dk[:Skv], dk0[:Skv])
        assert not torch.equal(dq[Sq:], dq0[Sq:])


@pytest.mark.parametrize("half", ["fp16", "bf16"])
def test_saturated_logits_stay_finite_and_within_the_bound(half):
    """q and k scaled so that |scale q . k| reaches about 60: the softmax is nearly one-hot for many queries"""
    from textboost_amd import _lib as L
    case = B, H, Sq, Skv, hd = (2, 8, 64, 77, 40)
    scale = hd ** -0.5
    with L.use_half(half):
        dt = L.half_dtype()
        Q, K, tok_w, g = _inputs(case, 31, dt, qk_gain=15.0 ** 0.5)
        logits = scale * (Q.double().reshape(B, Sq, H, hd).permute(0, 2, 1, 3) @ K.double().reshape(B, Skv, H, hd).permute(0, 2, 3, 1))
        print(f"[attn loss] saturated: max |logit| {logits.abs().max().item():.1f}")
        assert 50 <= logits.abs().max().item() <= 90
        tot, dq_ref, dk_ref = R.attn_loss_ref(Q, K, tok_w, g, H, scale, COEF)
        assert torch.isfinite(dq_ref).all() and torch.isfinite(dk_ref).all() and torch.isfinite(tot)
        _, dq32, dk32 = R.attn_loss_ref(Q, K, tok_w, g, H, scale, COEF, dtype=torch.float32)
        yq, yk = (dq32.double() - dq_ref).abs().max().item(), (dk32.double() - dk_ref).abs().max().item()
        dq, dk, part = _launch(Q, K, tok_w, g, case, COEF, 1.0)
        _check(f"{half} saturated dQ", dq, dq_ref, yq, half)
        _check(f"{half} saturated dK", dk, dk_ref, yk, half)
        assert np.isfinite(part)
        assert abs(part - tot.item()) <= B * H * Sq * Skv * 2.0 ** -23 * abs(tot.item())


@pytest.mark.parametrize("half", ["fp16", "bf16"])
def test_unaligned_rows_and_bit_identical_relaunch(half):
    """q / dq are column slices at an odd multiple of 2 bytes, k / dk slices of a wider buffer with an odd row pitch: the 2-byte load path; the
    columns around the slices stay as they were, and a second launch on the same inputs gives the same bits"""
    from textboost_amd import _lib as L
    from textboost_amd import ops
    case = B, H, Sq, Skv, hd = (2, 2, 100, 77, 40)
    C = H * hd
    scale = hd ** -0.5
    with L.use_half(half):
        dt = L.half_dtype()
        Q, K, tok_w, g = _inputs(case, 41, dt)
        _, dq_ref, dk_ref = R.attn_loss_ref(Q, K, tok_w, g, H, scale, COEF)
        _, dq32, dk32 = R.attn_loss_ref(Q, K, tok_w, g, H, scale, COEF, dtype=torch.float32)
        yq, yk = (dq32.double() - dq_ref).abs().max().item(), (dk32.double() - dk_ref).abs().max().item()
        outs = []
        for _ in range(2):
            qbuf = torch.full((B * Sq, C + 6), 3.0, dtype=dt)
            kbuf = torch.full((B * Skv, 3 * C + 7), 3.0, dtype=dt)
            qbuf[:, 3:3 + C] = Q
            kbuf[:, C + 1:2 * C + 1] = K
            qd, kd = qbuf.to(dev), kbuf.to(dev)
            dqb = torch.full((B * Sq, C + 2), 5.0, dtype=dt, device=dev)
            dkb = torch.full((B * Skv, 2 * C + 3), 5.0, dtype=dt, device=dev)
            dqv, dkv = dqb[:, 1:1 + C], dkb[:, C + 1:2 * C + 1]
            dqv.zero_()
            dkv.zero_()
            ws = ops.attn_loss_workspace(dev, B, H, 1)
            ops.attn_loss_bwd(qd[:, 3:3 + C], kd[:, C + 1:2 * C + 1], dqv, dkv, tok_w.to(dev), g.to(dev), B, H, Sq, Skv, hd, COEF, None, ws, 0)
            outs.append((dqb.cpu(), dkb.cpu(), ws.cpu()))
        (dqb, dkb, ws0), (dqb2, dkb2, ws1) = outs
        assert torch.equal(dqb, dqb2) and torch.equal(dkb, dkb2) and torch.equal(ws0, ws1)
        assert (dqb[:, 0] == 5).all() and (dqb[:, 1 + C:] == 5).all() and (dkb[:, :C + 1] == 5).all() and (dkb[:, 2 * C + 1:] == 5).all()
        _check(f"{half} unaligned dQ", dqb[:, 1:1 + C], dq_ref, yq, half)
        _check(f"{half} unaligned dK", dkb[:, C + 1:2 * C + 1], dk_ref, yk, half)


def test_coef_kernel_matches_the_reference():
    from textboost_amd import ops
    gen = torch.Generator().manual_seed(3)
    B, h, w = 3, 16, 24
    target = torch.rand(B, 1, h, w, generator=gen)
    target[1] = (target[1] > 0.7).float()
    for level in (0, 1, 2):
        f = 1 << level
        ref = R.coef_ref(target, level)
        g = torch.full((B, (h // f) * (w // f)), float("nan"), device=dev)
        ops.attn_loss_coef(target.to(dev), g, f)
        got = g.cpu()
        ulp = torch.from_numpy(np.spacing(np.abs(ref.float().numpy())))
        err = ((got.double() - ref).abs() / ulp.double()).max().item()
        print(f"[attn loss] coef factor {f}: max err {err:.2f} ulp")
        assert err <= 4.0
        for fill, want in ((1.0, -1.0 / ((h // f) * (w // f))), (0.0, 1.0 / ((h // f) * (w // f)))):   # all white, all black: exact
            flat = torch.full((B, 1, h, w), fill, device=dev)
            ops.attn_loss_coef(flat, g, f)
            assert torch.equal(g.cpu(), torch.full(g.shape, want, dtype=torch.float64).float())


def test_bad_arguments_return_einval_and_touch_nothing():
    from textboost_amd import _lib as L
    B, H, Sq, Skv, hd = 1, 2, 32, 16, 16

    def call(hd=hd, Skv=Skv, dtype=L.TB_F16, ws_floats=B * H, slot=0, tdtype=torch.float16):
        C = H * max(hd, 1)
        q = torch.ones(B * Sq, C, device=dev, dtype=tdtype)
        k = torch.ones(B * Skv, C, device=dev, dtype=tdtype)
        dq, dk = torch.full_like(q, 2.0), torch.full_like(k, 2.0)
        ws = torch.full((max(ws_floats, 1),), 9.0, device=dev)
        d = L.AttnDesc()
        d.B, d.H, d.Sq, d.Skv, d.hd, d.causal, d.scale = B, H, Sq, Skv, hd, 0, 0.25
        d.Q, d.ldq, d.K, d.ldk = L.ptr(q), C, L.ptr(k), C
        d.dQ, d.lddq, d.dK, d.lddk = L.ptr(dq), C, L.ptr(dk), C
        tw = torch.ones(B, Skv, device=dev)
        g = torch.ones(B, Sq, device=dev)
        rc = L.lib().tb_attn_loss_bwd(d, dtype, L.ptr(tw), L.ptr(g), 1.0, None, L.ptr(ws), ws_floats * 4, slot, B * H, L.stream())
        torch.cuda.synchronize()
        return rc, bool((dq == 2).all() and (dk == 2).all() and (ws == 9).all())

    assert call()[0] == 0
    for kw in (dict(hd=12), dict(hd=168), dict(Skv=129), dict(dtype=L.TB_F32, tdtype=torch.float32), dict(ws_floats=B * H - 1),
               dict(slot=1)):
        rc, untouched = call(**kw)
        assert rc == TB_EINVAL and untouched, kw


# ------------------------------------------------------------------------------------------------------------------ the step
LAMBDA = 4.0        # see test_step_matches_the_oracle_step_with_the_attention_loss
LEVELS = [1, 2]     # the 8 x 8 and 4 x 4 maps of the tiny UNet at 16 x 16 latents: 4 + 6 cross-attention layers


def _build_step(half="fp16"):
    """the tiny models with the masked loss and the localisation loss on: fp16 = those of tests/test_gpu_masked_loss.py (GradScaler at 65536),
    bf16 = the harness of tests/test_gpu_bf16.py, test_gpu_model.build_step(use_scaler=False) on the bf16 library (call it inside
    `L.use_half("bf16")`); the oracle is the same fp32 models either way"""
    if half == "fp16":
        from tests import test_gpu_masked_loss as TM
        st0, step, added = TM._build("fp16")
    else:
        from tests import test_gpu_model as GM
        st0, step, added = GM.build_step(2, 16, 64, use_scaler=False)
    st_ref = R.AttnLossTrainState(st0.te, st0.teacher, st0.unet, added, st0.cfg, attn_weight=LAMBDA, attn_levels=LEVELS,
                                  placeholder_ids=[added[0]])
    step.enable_loss_weight()
    target = step.enable_attn_loss(LAMBDA, LEVELS, (added[0], added[0] + 1))   # added[1:] play the augmentation tokens: weight 0
    return st_ref, step, added, target


def _step_inputs(g, it, B, hw, added):
    from tests import test_gpu_masked_loss as TM
    ids, pids, x0, noise, t = TM._inputs(g, B, hw, added)
    weight = torch.rand(B, 1, hw, hw, generator=g)
    weight[it % B] = 0
    target = (torch.rand(B, 1, hw, hw, generator=g) > 0.6).float()
    return ids, pids, x0, noise, t, weight, target


# (rel-L2, max-abs) of the gradients and the relative / absolute loss bound: fp16 = test_masked_step_matches_the_oracle_step_with_the_weighted_loss,
# bf16 = test_bf16_full_step_runs_without_a_grad_scaler_and_matches_oracle (tests/test_gpu_bf16.py: 8 x the fp16 bounds, 8 significand bits for 11)
STEP_BOUNDS = {"fp16": dict(rel=4e-3, maxabs=6e-3, loss_rel=2e-2, loss_abs=1e-4), "bf16": dict(rel=3.2e-2, maxabs=5e-2, loss_rel=5e-2, loss_abs=1e-3)}


@pytest.mark.parametrize("half", ["fp16", "bf16"])
def test_step_matches_the_oracle_step_with_the_attention_loss(half):
    """Two optimizer steps against AttnLossTrainState in both builds; the gradient and loss bounds are those of the build's own step test
    (STEP_BOUNDS), loss_attn held to loss_mse's.  lambda = 4: in the reference the added-row gradient with the loss differs from the gradient
    with lambda = 0 by 0.84 of its largest element on both steps (computed on the CPU), at least 10 x the build's max-abs parity bound (6e-3 /
    5e-2) -- the test cannot pass on the denoising gradient alone (0.80 / 0.78 with the bf16 case's all-ones weights).  bf16 runs without a
    GradScaler (loss scale 1) and with all-ones loss weights: its bounds were set for the unweighted bf16 step, and the bf16 step with the fp16
    case's weights (one sample weighted zero) misses them WITHOUT the localisation loss already -- measured on an MI355X with lambda = 0:
    grad lora_A rel-L2 4.55e-2, max-abs 5.77e-2 (lambda = 4: 4.72e-2 / 5.57e-2), so that figure says nothing about this loss."""
    from parity import parity
    from tests import test_gpu_masked_loss as TM
    from textboost_amd import _lib as L
    B, hw = 2, 16
    bd = STEP_BOUNDS[half]
    with L.use_half(half):
        st_ref, step, added, target_buf = _build_step(half)
        assert step.unet.dtype == L.half_dtype()
        assert tuple(target_buf.shape) == (B, 1, hw, hw) and float(target_buf.min()) == 1.0
        assert step.attn_loss.n == 10
        heads = step.unet.geo.heads
        g = torch.Generator().manual_seed(5)
        te_ref = st_ref.te
        for it in range(2):
            ids, pids, x0, noise, t, weight, target = _step_inputs(g, it, B, hw, added)
            if half == "bf16":   # the bf16 bounds are those of the UNWEIGHTED step (all-ones weights are tb_mse_loss's loss): see the docstring
                weight = torch.ones_like(weight)
            off = st_ref.step(x0, noise, t, ids, pids, weight, target, heads, attn_weight=0.0, update=False)
            out = st_ref.step(x0, noise, t, ids, pids, weight, target, heads)
            moved = ((out["g_emb_added"] - off["g_emb_added"]).abs().max() / out["g_emb_added"].abs().max()).item()
            print(f"[attn loss] {half} step {it}: the loss moves the reference's added-row gradient by {moved:.3f} of its largest element")
            assert moved >= 10 * bd["maxabs"]
            TM._load(step, ids, pids, x0, noise, t)
            step.loss_weight.copy_(weight)
            step.attn_target.copy_(target)
            step.step_eager()
            sc = step.scalars()
            assert sc["found_inf"] == 0.0
            tok_w = step.unet.attn_tok_w.cpu()
            assert torch.equal(tok_w, (ids == added[0]).float()) and tok_w.sum() >= 1
            L_ = len(te_ref.layers)
            gA = torch.stack([torch.cat(out["g_lora"][6 * l + 0: 6 * l + 6: 2]) for l in range(L_)])
            gB = torch.stack([torch.cat(out["g_lora"][6 * l + 1: 6 * l + 6: 2]) for l in range(L_)])
            clip = min(1.0, 1.0 / (out["lora_grad_norm"] + 1e-6))
            w, wr = step.te.token_table.cpu(), te_ref.token_embedding.weight.detach()
            A_ref = torch.stack([torch.cat([l.q.lora_A, l.k.lora_A, l.v.lora_A]) for l in te_ref.layers]).detach()
            torch.testing.assert_close(w[:49408], wr[:49408], rtol=1e-6, atol=1e-7)
            if half == "fp16":
                inv = 1.0 / 65536.0 if it == 0 else 1.0 / sc["loss_scale"]
            else:
                assert sc["loss_scale"] == 1.0
                inv = 1.0
            print(f"[attn loss] {half} step {it}: loss_attn {sc['loss_attn']:.6e} (reference {out['attn']:.6e}), loss_mse {sc['loss_mse']:.6f} "
                  f"({out['mse']:.6f})")
            assert abs(sc["loss_mse"] - out["mse"]) < bd["loss_rel"] * abs(out["mse"]) + bd["loss_abs"], (sc, out["mse"])
            assert abs(sc["loss_attn"] - out["attn"]) < bd["loss_rel"] * abs(out["attn"]) + bd["loss_abs"], (sc, out["attn"])
            assert abs(sc["loss"] - out["loss"]) < bd["loss_rel"] * abs(out["loss"]) + 2 * bd["loss_abs"]
            parity(f"attn-loss {half} step {it} grad lora_A", step.te.grad_A * inv * clip, gA, rel=bd["rel"], maxabs=bd["maxabs"])
            parity(f"attn-loss {half} step {it} grad lora_B", step.te.grad_B * inv * clip, gB, rel=bd["rel"], maxabs=bd["maxabs"])
            parity(f"attn-loss {half} step {it} grad added rows", step.te.grad_added * inv, out["g_emb_added"], rel=bd["rel"], maxabs=bd["maxabs"])
            if half == "fp16":   # (the bf16 step test of tests/test_gpu_bf16.py bounds the losses and the gradients only)
                assert abs(sc["grad_norm"] - out["lora_grad_norm"]) < 5e-2 * out["lora_grad_norm"]
                assert (w[added] - wr[added]).abs().max().item() < 2.5e-3
                assert ((w[added] - wr[added]).norm() / wr[added].norm()).item() < 2e-3
                assert (step.te.lora_A.cpu() - A_ref).abs().max().item() < 1.5e-4
        assert step.scalars()["opt_steps"] == 2.0


# the tiny masked step's graph (tests/test_gpu_masked_loss.py: 883 nodes) plus 3 torch launches for tok_w, one coefficient launch per supervised
# level (2), one loss launch per supervised layer (10) and the final reduction
ATTN_LOSS_TINY_STEP_NODES = 883 + 3 + 2 + 10 + 1


def test_graph_replay_equals_eager_and_counts_the_added_launches(monkeypatch):
    from tests import test_gpu_masked_loss as TM
    B, hw = 2, 16
    graph_class = torch.cuda.CUDAGraph
    monkeypatch.setattr(torch.cuda, "CUDAGraph", lambda *a, **k: graph_class(keep_graph=True))
    outs = []
    for mode in ("eager", "graph"):
        _, step, added, _ = _build_step()
        g = torch.Generator().manual_seed(6)
        ids, pids, x0, noise, t, weight, target = _step_inputs(g, 1, B, hw, added)
        TM._load(step, ids, pids, x0, noise, t)
        step.loss_weight.copy_(weight)
        step.attn_target.copy_(target)
        if mode == "eager":
            for _ in range(4):
                step.step_eager()
        else:
            step.capture(warmup=2)
            step.replay(); step.replay()
            nodes = TM._graph_nodes(step)
            with pytest.raises(RuntimeError):
                step.enable_attn_loss(LAMBDA, LEVELS, (added[0], added[0] + 1))
        torch.cuda.synchronize()
        outs.append((step.te.lora_A.clone(), step.te.lora_B.clone(), step.te.token_table[49408:].clone(), step.state.clone()))
    for a, b in zip(*outs):
        torch.testing.assert_close(a, b, rtol=0, atol=0)
    assert outs[0][3][14].item() != 0.0      # state[TB_ST_LOSS_ATTN]
    print(f"[attn loss] tiny step graph nodes with the loss on: {nodes}")
    assert nodes == ATTN_LOSS_TINY_STEP_NODES


# ------------------------------------------------------------------------------------------------------------------ the feeder
def test_feeder_fills_attn_target_with_the_floor_0_pooling_of_the_same_crop():
    import masked_loss_ref as MR
    from tests import test_gpu_masked_loss as TM
    L, D, ops = TM._mods()
    size = 32
    rgbs, masks = [TM._rgb(3, 70, 90), TM._rgb(4, 96, 80)], [TM._mask(5, 70, 90), TM._mask(6, 96, 80)]
    templates = ["a photo of {}", "{} on a table"]

    def feeder(kind, floor, target=True):
        cfg = dict(hflip="inversion", inversion=True, p=1.0, color_prob=1.0)
        if kind == "masked":
            items = [(D.to_device_image(a), "<s>", D.to_device_mask(m)) for a, m in zip(rgbs, masks)]
        else:   # the mask images as the images: pixel_values then hold the cropped mask bytes
            items = [(D.to_device_mask(m), "<s>") for m in masks]
        return D.DeviceFeeder(items, TM.FakeTokenizer(), templates, size=size, center_crop=False, augment_pipe=D.PairedAugmentation(**cfg),
                              mask_floor=floor if kind == "masked" else 0.0, attn_target=target and kind == "masked")

    idx = [0, 1, 1, 0, 1]
    TM._seed(11)
    b2 = feeder("mask_alone", 0.0).batch(idx)
    bytes_ = ((b2["pixel_values"][:, 0].cpu().double() * 0.5 + 0.5) * 255).round().to(torch.uint8).numpy()
    for floor in (0.25, 0.0):
        TM._seed(11)
        b1 = feeder("masked", floor).batch(idx)
        TM._seed(11)
        b0 = feeder("masked", floor, target=False).batch(idx)
        assert "attn_target" not in b0 and torch.equal(b0["loss_weight"], b1["loss_weight"]) and torch.equal(b0["pixel_values"], b1["pixel_values"])
        tg, lw = b1["attn_target"], b1["loss_weight"]
        assert tuple(tg.shape) == (len(idx), 1, size // 8, size // 8) and tg.dtype == torch.float32
        for b in range(len(idx)):
            want = MR.pool_ref(bytes_[b], 0, 0, size // 8, size // 8, 8, 0.0)
            assert np.array_equal(tg[b, 0].cpu().numpy().view(np.uint32), want.view(np.uint32)), (floor, b)
            wantw = MR.pool_ref(bytes_[b], 0, 0, size // 8, size // 8, 8, floor)
            assert np.array_equal(lw[b, 0].cpu().numpy().view(np.uint32), wantw.view(np.uint32)), (floor, b)
        if floor == 0.0:
            assert tg.data_ptr() == lw.data_ptr()          # --mask_floor 0: one tensor
        else:
            assert float(tg.min()) < float(lw.min()) and floor <= float(lw.min())     # w = F + (1 - F) m > m
        # the prefetcher stages and commits the target beside the weights
        pv, ids = torch.zeros(2, 3, size, size, device=dev), torch.zeros(2, 77, dtype=torch.int64, device=dev)
        w_in, t_in = torch.ones(2, 1, 4, 4, device=dev), torch.ones(2, 1, 4, 4, device=dev)
        TM._seed(11)
        pre = D.PrefetchFeeder(feeder("masked", floor), 2, pv, ids, loss_weight=w_in, attn_target=t_in)
        pre.prefetch(idx[:2])
        pre.commit()
        torch.cuda.synchronize()
        assert torch.equal(w_in, lw[:2]) and torch.equal(t_in, tg[:2])
        with pytest.raises(ValueError):
            D.PrefetchFeeder(feeder("masked", floor), 2, pv, ids, loss_weight=w_in)
    with pytest.raises(ValueError):
        D.DeviceFeeder([(D.to_device_image(rgbs[0]), "<s>")], TM.FakeTokenizer(), templates, size=size, attn_target=True)


# ------------------------------------------------------------------------------------------------------------------ the command line
def test_cli_trains_with_masks_and_the_attention_loss(tmp_path):
    """train_textboost.py on the tiny model directory of tests/test_gpu_sweep.py, one instance image with a mask, 3 steps: it trains and
    checkpoints, the step line carries loss_attn, training.log names the weight and the levels"""
    import os
    import re
    import sys
    pytest.importorskip("PIL")
    from PIL import Image
    from tests import test_gpu_sweep as TS
    sys.path.insert(0, TS.ROOT)
    import train_textboost as T
    root = str(tmp_path)
    mdir = TS._prepare(root)
    data = os.path.join(root, "data", "s1")
    with Image.open(os.path.join(data, "00.png")) as im:
        w, h = im.size
    m = np.zeros((h, w), np.uint8)
    m[h // 4: 3 * h // 4, w // 3: 2 * w // 3] = 255
    os.makedirs(os.path.join(root, "masks"))
    Image.fromarray(m, "L").save(os.path.join(root, "masks", "00.png"))
    out = os.path.join(root, "run")
    cwd = os.getcwd()
    os.chdir(root)
    try:
        T.main(T.parse_args(["--pretrained_model_name_or_path", mdir, "--instance_data_dir", data, "--instance_mask_dir",
                             os.path.join(root, "masks"), "--output_dir", out, "--train_batch_size", "2", "--resolution", "128",
                             "--max_train_steps", "3", "--checkpointing_steps", "3", "--placeholder_token", "<s1>", "--initializer_token", "a b",
                             "--lora_rank", "4", "--mixed_precision", "fp16", "--seed", "1", "--mask_floor", "0.25", "--attn_loss_weight", "0.5",
                             "--attn_loss_levels", "1", "2"]))
    finally:
        os.chdir(cwd)
    log = open(os.path.join(out, "training.log")).read()
    assert "attention loss: on, --attn_loss_weight 0.5, --attn_loss_levels 1 2 (10 cross-attention layer(s))" in log, log[-3000:]
    line = re.search(r"step 3 loss \S+ mse \S+ kpl \S+ loss_attn (\S+) scale", log)
    assert line and np.isfinite(float(line.group(1))) and float(line.group(1)) != 0.0, log[-3000:]
    assert {"text_encoder", "checkpoint-3", "training.log"} <= set(os.listdir(out))


def test_scalars_carry_loss_attn_only_when_the_loss_is_on():
    """a step without the localisation loss reports exactly the keys it always did (bench.py --dump-outputs writes one file per key)"""
    from tests import test_gpu_masked_loss as TM
    _, step, added = TM._build("fp16", masked_oracle=False)
    assert set(step.scalars()) == {"loss_mse", "loss_kpl", "loss", "loss_scale", "grad_norm", "found_inf", "opt_steps"}
    step.enable_loss_weight()
    step.enable_attn_loss(LAMBDA, LEVELS, (added[0], added[0] + 1))
    assert set(step.scalars()) == {"loss_mse", "loss_kpl", "loss_attn", "loss", "loss_scale", "grad_norm", "found_inf", "opt_steps"}
