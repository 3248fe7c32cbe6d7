"""--lora_target_modules on the GPU: text-encoder LoRA on out_proj / fc1 / fc2 beside q/k/v.  One adapter (P = 1) on rectangular layers: the
adapter gradients against autograd, the two-source GEMM with every epilogue it now meets, the tiny encoder and whole optimizer steps against the
oracle in the three numeric modes, graph replay, the default list spelled out, and the CLI with the run-directory reader and composition.
Bounds are those of tests/test_gpu_lora_wide.py for the same quantities (named in each docstring)."""
import json
import os
import sys
import types

import pytest
import torch

import lora_targets_ref as LT
from parity import parity

pytestmark = pytest.mark.gpu
dev = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIX = LT.ALL
ENC = dict(rel=5e-4, maxabs=1e-3, ch_dim=2, ch_rel=2e-3)       # tests/test_gpu_lora_wide.py:175
GRAD = dict(rel=1.5e-3, maxabs=2e-3)                           # :180-181


def rel_err(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


# ------------------------------------------------------------------------------------------------ 1. adapter gradients and dt, P = 1
NARROW = [(4, 128, 64, 77), (8, 64, 128, 154), (8, 3072, 768, 154), (5, 768, 3072, 154), (8, 5120, 1280, 77), (8, 3072, 768, 1848)]
WIDE = [(12, 128, 64, 77), (33, 64, 128, 154), (16, 3072, 768, 154), (64, 768, 3072, 154), (16, 3072, 768, 1848)]


@pytest.mark.parametrize("r,Dm,K,M", NARROW + WIDE)
def test_rectangular_adapter_gradients_match_autograd(r, Dm, K, M):
    """one adapter y += s (x A^T) B^T, A [r, K], B [Dm, r], through ops.lora_rect_bwd (dt as a GEMM on w2_t, then tb_lora_bwd_panels up to rank 8
    and tb_lora_wide_wgrad above) against autograd at the bounds of tests/test_gpu_lora_wide.py:84-86 (dA, dB rel-L2 < 5e-3, dt < 3e-3; scaling
    0.5).  M is never a multiple of a 16- or 64-row slab, M = 1848 picks other tile routes.  The gradient buffers start from constants (the
    launches add); rows >= M of every operand and the padding columns of t are poisoned in a second run, which must give the same bits."""
    from textboost_amd import ops
    torch.manual_seed(r + Dm)
    sc = 0.5
    A = torch.randn(r, K, device=dev) / r
    Bm = torch.randn(Dm, r, device=dev) * 0.1
    rp, Rp = ops.lora_rect_dims(r)
    assert Rp == 64 and rp >= r
    a_pad = torch.full((1, Rp, K), 7.0, device=dev, dtype=torch.float16)
    w2f = torch.full((1, Dm, Rp), 7.0, device=dev, dtype=torch.float16)
    w2t = torch.full((1, Rp, Dm), 7.0, device=dev, dtype=torch.float16)
    w2d = torch.full((1, K, Rp), 7.0, device=dev, dtype=torch.float16)
    ops.lora_wide_pack(A, Bm, a_pad, w2f, w2t, w2d, Dm, K, r, rp, 1, scaling=sc)
    assert torch.equal(w2t[0, :r].float(), (sc * Bm).half().float().T) and not w2t[0, r:].any() and torch.equal(w2t[0], w2f[0].T)
    assert torch.equal(a_pad[0, :r].float(), A.half().float()) and not a_pad[0, r:].any() and torch.equal(w2d[0], a_pad[0].T)
    PADR = 7   # rows behind M in every operand's allocation
    xb = torch.randn(M + PADR, K, device=dev).half()
    dYb = torch.randn(M + PADR, Dm, device=dev).half()
    tb = torch.full((M + PADR, Rp), 3.0, device=dev, dtype=torch.float16)
    x, dY, t = xb[:M], dYb[:M], tb[:M]
    if r <= ops.LORA_NARROW_MAX:
        t.zero_()
        ops.lora_down(x, A, t)
    else:
        ops.gemm(x, a_pad[0], t)
    assert not t[:, r:].any() and torch.equal(tb[M:], torch.full_like(tb[M:], 3.0))
    xr = x.float()
    e_d = rel_err(t[:, :r], xr @ A.half().float().T)
    outs = []
    for poison in (False, True):
        if poison:
            xb[M:] = float("nan"); dYb[M:] = float("inf"); tb[M:] = float("nan")
            if r <= ops.LORA_NARROW_MAX:   # (the MFMA tiles multiply the padding columns: the executor keeps zeros there, and 0 * nan is nan)
                t[:, r:] = float("nan")
        dtb = torch.full((M + PADR, Rp), 3.0, device=dev, dtype=torch.float16)
        dA = torch.full_like(A, 0.25); dB = torch.full_like(Bm, -0.5)
        ops.lora_rect_bwd(dY, x, t, w2t[0], dtb[:M], dA, dB, Dm, K, r, scaling=sc)
        assert torch.equal(dtb[M:], torch.full_like(dtb[M:], 3.0)) and not dtb[:M, r:].any()
        outs.append((dA, dB, dtb[:M].clone()))
    for a_, b_ in zip(*outs):
        assert torch.isfinite(b_).all() and torch.equal(a_, b_)
    dA, dB, dt = outs[0][0] - 0.25, outs[0][1] + 0.5, outs[0][2]
    Ar = A.clone().requires_grad_(True); Br = Bm.clone().requires_grad_(True)
    (sc * (xr @ Ar.T) @ Br.T).backward(dY.float())
    ref_dt = sc * dY.float() @ Bm.half().float()
    e_a, e_b, e_t = rel_err(dA, Ar.grad), rel_err(dB, Br.grad), rel_err(dt[:, :r], ref_dt)
    print(f"[lora targets] r {r} D {Dm} K {K} M {M}: dA {e_a:.3e} dB {e_b:.3e} dt {e_t:.3e} t {e_d:.3e}")
    assert e_a < 5e-3 and e_b < 5e-3
    assert e_t < 3e-3
    assert e_d < 2e-3


# ------------------------------------------------------------------------------------------------ 2. the two-source GEMM's epilogues
def _qgelu(x):
    return x * torch.sigmoid(1.702 * x)


@pytest.mark.parametrize("M", [154, 1848])
@pytest.mark.parametrize("K1,N", [(64, 128), (128, 64), (768, 3072), (3072, 768)])
def test_two_source_gemm_with_each_epilogue(K1, N, M):
    """x W^T + t W2^T (t, W2: the 64-column K-extension of a rank-8 adapter) with the three epilogues the extra modules bring: bias + activation +
    C2 (fc1), bias + fp32 residual into an fp32 output (out_proj, fc2), and the activation-gradient epilogue of the fc2 dgrad.  Against fp32
    torch at the two-source bound of tests/test_gpu_lora_wide.py:153-154 (rel-L2 < 3e-3); without the adapter term every result is further than
    ten times the bound away, so a route that dropped it would fail."""
    from textboost_amd import _lib as L
    from textboost_amd import ops
    torch.manual_seed(K1 + N + M)
    r, bound = 8, 3e-3
    x = torch.randn(M, K1, device=dev).half()
    W = (torch.randn(N, K1, device=dev) / 11).half()
    t = torch.zeros(M, 64, device=dev, dtype=torch.float16)
    t[:, :r] = torch.randn(M, r, device=dev).half()
    W2 = torch.zeros(N, 64, device=dev, dtype=torch.float16)
    W2[:, :r] = (torch.randn(N, r, device=dev) * 0.4).half()
    bias = torch.randn(N, device=dev).half().float()
    main, lo = x.float() @ W.float().T, t.float() @ W2.float().T
    res = {}
    # (a) fc1: act(x W^T + t W2^T + b), C2 = the pre-activation
    y = torch.empty(M, N, device=dev, dtype=torch.float16); pre = torch.empty_like(y)
    ops.gemm(x, W, y, A2=t, W2=W2, bias=bias, act=L.ACT_QUICK_GELU, C2=pre)
    res["act+C2"] = (rel_err(y, _qgelu(main + lo + bias)), rel_err(y, _qgelu(main + bias)))
    res["C2"] = (rel_err(pre, main + lo + bias), rel_err(pre, main + bias))
    # (b) out_proj / fc2: fp32 residual stream
    R = torch.randn(M, N, device=dev)
    h = torch.empty(M, N, device=dev)
    ops.gemm(x, W, h, A2=t, W2=W2, bias=bias, R=R)
    res["bias+R fp32"] = (rel_err(h, main + lo + bias + R), rel_err(h, main + bias + R))
    # (c) fc2 dgrad: (dy Wd^T + dt W2d^T) * act'(pre)
    pre_in = torch.randn(M, N, device=dev).half()
    g = torch.empty(M, N, device=dev, dtype=torch.float16)
    ops.gemm(x, W, g, A2=t, W2=W2, act=L.ACT_QUICK_GELU_GRAD, C2=pre_in)
    pf = pre_in.float()
    sg = torch.sigmoid(1.702 * pf)
    dact = sg * (1 + 1.702 * pf * (1 - sg))
    res["act-grad"] = (rel_err(g, (main + lo) * dact), rel_err(g, main * dact))
    for k, (e, far) in res.items():
        print(f"[lora targets] two-source GEMM {M}x{N}x({K1}+64) {k}: {e:.3e}; without the adapter term {far:.3e}")
    for k, (e, far) in res.items():
        assert e < bound, k
        assert far > 10 * bound, k


# ------------------------------------------------------------------------------------------------ 3. the tiny encoder
def encoders(B, D, r, modules, seed=0, mode="autocast", n_added=3):
    """tests/test_gpu_model.py::make_encoders / tests/test_gpu_f32.py::_encoders_f32 with the adapted modules as a parameter"""
    from oracle import train_step as ts
    from oracle.clip_text import CLIPTextCfg, TextBoostEncoder, add_tokens
    from textboost_amd.text_encoder import CLIPGeometry, HipTextEncoder
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
                p.normal_(std=0.05)     # non-zero B so every LoRA gradient path is exercised
    LT.add_adapters(student, [m for m in modules if m in LT.EXTRA], r, seed=seed + 50)
    added = add_tokens(student, [100, 200, 300][:n_added])
    geo = CLIPGeometry(hidden_size=D, intermediate_size=ccfg.intermediate_size, num_layers=ccfg.num_layers, num_heads=ccfg.num_heads)
    sd = {hf: dict(base.named_parameters())[ours].detach() for ours, hf in base.hf_key_map().items()}
    hip = HipTextEncoder(geo, sd, B, mode=mode, lora_rank=r, n_slots=2, device=dev, seed=0, lora_targets=modules)
    hip.set_null_embedding(null)
    hip.add_tokens([100, 200, 300][:n_added])
    LT.copy_to_hip(student, hip)
    hip_teacher = HipTextEncoder(geo, sd, B, mode="fp32" if mode == "fp32" else "half", lora_rank=0, device=dev)
    hip_teacher.set_null_embedding(null)
    return student, teacher, hip, hip_teacher, added, null


@pytest.mark.parametrize("r,modules", [(4, SIX), (16, SIX), (4, LT.QKV + ("fc2",))], ids=["r4-six", "r16-six", "r4-qkv-fc2"])
def test_tiny_encoder_with_extra_modules_matches_oracle(r, modules):
    """the body and the bounds of tests/test_gpu_lora_wide.py::test_text_encoder_wide_ranks_match_oracle (states 5e-4 / 1e-3 / 2e-3, gradients
    1.5e-3 / 2e-3) with adapters on out_proj / fc1 / fc2 too: every adapter gradient, the added rows, and the frozen teacher rows inside the
    student's launches, which must come out as the un-adapted encoder's on every module"""
    from oracle import train_step as ts
    B, D = 3, 64
    student, teacher, hip, hip_teacher, added, null = encoders(B, D, r, modules)
    assert tuple(hip.extra) == tuple(modules[3:]) and hip.wide == (r > 8)
    g = torch.Generator().manual_seed(2)
    ids = ts.synthetic_ids(B, added, g)
    ids[1, 1:] = 49407   # a null prompt row -> pinned, zero gradient
    out_ref = student(ids)
    R = torch.randn(B, 77, D, generator=g)
    (out_ref * R).sum().backward()
    hip.pack_lora()
    out = hip.forward(ids.to(dev), slot=0)
    parity(f"r={r} {len(modules)} modules: hidden states", out.view(B, 77, D), out_ref, **ENC)
    assert torch.equal(out.view(B, 77, D)[1].cpu(), null)
    hip.zero_grad()
    hip.backward(R.view(B * 77, D).to(dev).contiguous(), slot=0)
    gA, gB, gx = LT.oracle_grads(student)
    parity(f"r={r} grad lora_A (q/k/v)", hip.grad_A, gA, ch_dim=0, ch_rel=2e-3, **GRAD)
    parity(f"r={r} grad lora_B (q/k/v)", hip.grad_B, gB, ch_dim=0, ch_rel=2e-3, **GRAD)
    for n, X in hip.extra.items():
        parity(f"r={r} grad {n} lora_A", X.grad_A, gx[n][0], ch_dim=0, ch_rel=2e-3, **GRAD)
        parity(f"r={r} grad {n} lora_B", X.grad_B, gx[n][1], ch_dim=0, ch_rel=2e-3, **GRAD)
    parity(f"r={r} grad added rows", hip.grad_added, student.token_embedding.weight.grad[added], rel=1e-3, maxabs=1.5e-3)
    pids = ts.synthetic_ids(B, added, g, prior=True)
    with torch.no_grad():
        t_ref = teacher(pids)
    merged = hip.forward(ids.to(dev), slot=0, extra_ids=pids.to(dev), extra_table=hip_teacher.token_table.float())
    assert torch.equal(merged[:B * 77], out)
    parity(f"r={r} teacher rows inside the student pass", merged[B * 77:].view(B, 77, D), t_ref, rel=5e-4, maxabs=1e-3)
    for n in hip.extra:      # the teacher rows' K-extension operand rows are zero on every module
        assert not hip._bufs[f"s0.l1.t_{n}"][B * 77:].any(), n
    keep = [hip.grad_A.clone(), hip.grad_B.clone(), hip.grad_added.clone()] + [t_.clone() for X in hip.extra.values() for t_ in (X.grad_A, X.grad_B)]
    hip.zero_grad()
    hip.backward(R.view(B * 77, D).to(dev).contiguous(), slot=0)
    again = [hip.grad_A, hip.grad_B, hip.grad_added] + [t_ for X in hip.extra.values() for t_ in (X.grad_A, X.grad_B)]
    assert all(torch.equal(a_, b_) for a_, b_ in zip(keep, again))


# ------------------------------------------------------------------------------------------------ 4. whole steps
def build_step(r, modules, B=2, hw=16, D=64, use_scaler=True, mode="autocast", mixing=None):
    from oracle import train_step as ts
    from textboost_amd.trainer import StepHyper, TextBoostStep
    if mode == "fp32":
        from test_gpu_f32 import _small_unet_f32
        ref_unet, hip_unet = _small_unet_f32(B, hw, D, seed=3)
    else:
        from test_gpu_model import make_unet
        ref_unet, hip_unet, _ = make_unet(B, hw, D, seed=3)
    student, teacher, hip_te, hip_teacher, added, null = encoders(B, D, r, modules, seed=4, mode=mode)
    st_ref = ts.TrainState(student, teacher, ref_unet, added, ts.StepConfig(mixing=mixing))
    hp = StepHyper(use_grad_scaler=use_scaler, init_scale=65536.0 if use_scaler else 1.0, mixing=mixing)
    step = TextBoostStep(hip_unet, hip_te, hip_teacher, hp, (B, 4, hw, hw), device=dev)
    step.external_noise = True
    return st_ref, step, added


def _draw(step, added, g, B, hw):
    from oracle import train_step as ts
    ids, pids = ts.synthetic_ids(B, added, g), ts.synthetic_ids(B, added, g, prior=True)
    x0, noise = torch.randn(B, 4, hw, hw, generator=g), torch.randn(B, 4, hw, hw, generator=g)
    t = torch.randint(0, 1000, (B,), generator=g)
    step.x0.copy_(x0); step.noise.copy_(noise); step.timesteps.copy_(t); step.input_ids.copy_(ids); step.prior_ids.copy_(pids)
    return x0, noise, t, ids, pids


def _masters(te_ref):
    """(A, B) of every adapted module of the oracle, stacked over layers, keyed like HipTextEncoder.extra (+ "qkv")"""
    out = {"qkv": (torch.stack([torch.cat([l.q.lora_A, l.k.lora_A, l.v.lora_A]) for l in te_ref.layers]).detach(),
                   torch.stack([torch.cat([l.q.lora_B, l.k.lora_B, l.v.lora_B]) for l in te_ref.layers]).detach())}
    for n in LT.adapted(te_ref)[3:]:
        out[n] = (torch.stack([getattr(l, LT.ATTR[n]).lora_A for l in te_ref.layers]).detach(),
                  torch.stack([getattr(l, LT.ATTR[n]).lora_B for l in te_ref.layers]).detach())
    return out


def _hip_sets(te):
    return {"qkv": (te.lora_A, te.lora_B, te.grad_A, te.grad_B), **{n: (X.A, X.B, X.grad_A, X.grad_B) for n, X in te.extra.items()}}


def test_two_steps_fp16_mixing_six_modules_match_oracle_elementwise():
    """two optimizer steps, fp16 with the grad scaler, r = 4, six modules, mixing = "object": the bounds of
    tests/test_gpu_lora_wide.py::test_full_step_rank16_matches_oracle_elementwise (:238-252) on every adapter set; the odd rows of every
    lora_B gradient -- out_proj / fc1 / fc2 included -- are exactly zero, so those rows only decay"""
    B, hw, D = 2, 16, 64
    st_ref, step, added = build_step(4, SIX, B, hw, D, mixing="object")
    assert step.n_lora == sum(a.numel() + b.numel() for a, b, _, _ in _hip_sets(step.te).values()) == step.flat_lora.numel()
    g = torch.Generator().manual_seed(5)
    te_ref = st_ref.te
    for it in range(2):
        x0, noise, t, ids, pids = _draw(step, added, g, B, hw)
        out = st_ref.step(x0, noise, t, ids, pids)
        step.step_eager()
        sc = step.scalars()
        assert sc["found_inf"] == 0.0
        assert abs(sc["loss_mse"] - out["mse"]) < 2e-2 * abs(out["mse"]) + 1e-4, (sc, out["mse"])
        assert abs(sc["loss_kpl"] - out["kpl"]) < 5e-2 * abs(out["kpl"]) + 1e-5, (sc, out["kpl"])
        inv = 1.0 / 65536.0 if it == 0 else 1.0 / sc["loss_scale"]
        clip = min(1.0, 1.0 / (out["lora_grad_norm"] + 1e-6))       # the oracle's g_lora are post-clip
        assert abs(sc["grad_norm"] - out["lora_grad_norm"]) < 5e-2 * out["lora_grad_norm"]
        gA, gB, gx = LT.split_step_grads(out["g_lora"], te_ref)
        want = {"qkv": (gA, gB), **gx}
        ref = _masters(te_ref)
        for n, (A_, B_, gA_, gB_) in _hip_sets(step.te).items():
            parity(f"six modules step {it} grad {n} lora_A", gA_ * inv * clip, want[n][0], rel=4e-3, maxabs=6e-3)
            parity(f"six modules step {it} grad {n} lora_B", gB_ * inv * clip, want[n][1], rel=4e-3, maxabs=6e-3)
            odd = gB_[:, 1::2]      # (D and I are even: the parity of a row of the stacked [3D, r] is its parity inside its projection)
            assert odd.numel() and not odd.any(), n
            assert gB_[:, 0::2].abs().max() > 0, n
            assert (A_.cpu() - ref[n][0]).abs().max().item() < 1.5e-4, n             # <= ~2 * lr
            torch.testing.assert_close(B_.cpu()[:, 1::2], ref[n][1][:, 1::2], rtol=1e-6, atol=1e-7)    # rows without a gradient only decay
        parity(f"six modules step {it} grad added rows", step.te.grad_added * inv, out["g_emb_added"], rel=4e-3, maxabs=6e-3)
        w = step.te.token_table.cpu()
        wr = te_ref.token_embedding.weight.detach()
        torch.testing.assert_close(w[:49408], wr[:49408], rtol=1e-6, atol=1e-7)       # decay-only rows
        assert (w[added] - wr[added]).abs().max().item() < 2.5e-3                     # <= ~2 * emb_lr (Adam step-1 sign flips)
        assert rel_err(w[added], wr[added]) < 2e-3
    assert step.scalars()["opt_steps"] == 2.0


def test_two_steps_bf16_six_modules_match_oracle():
    """the bfloat16 build, r = 4, six modules, at the bounds of tests/test_gpu_lora_wide.py::test_bf16_full_step_rank16_matches_oracle (:293-296)"""
    from textboost_amd import _lib as L
    with L.use_half("bf16"):
        B, hw, D = 2, 16, 64
        st_ref, step, added = build_step(4, SIX, B, hw, D, use_scaler=False)
        assert step.te.extra["fc1"].w2_t.dtype == torch.bfloat16
        g = torch.Generator().manual_seed(5)
        for it in range(2):
            x0, noise, t, ids, pids = _draw(step, added, g, B, hw)
            out = st_ref.step(x0, noise, t, ids, pids)
            step.step_eager()
            sc = step.scalars()
            assert sc["found_inf"] == 0.0 and sc["loss_scale"] == 1.0
            assert abs(sc["loss_mse"] - out["mse"]) < 5e-2 * abs(out["mse"]) + 1e-3, (sc, out["mse"])
            clip = min(1.0, 1.0 / (out["lora_grad_norm"] + 1e-6))
            gA, gB, gx = LT.split_step_grads(out["g_lora"], st_ref.te)
            want = {"qkv": (gA, gB), **gx}
            for n, (A_, B_, gA_, gB_) in _hip_sets(step.te).items():
                parity(f"bf16 six modules step {it} grad {n} lora_A", gA_ * clip, want[n][0], rel=3.2e-2, maxabs=5e-2)
            parity(f"bf16 six modules step {it} grad added rows", step.te.grad_added, out["g_emb_added"], rel=3.2e-2, maxabs=5e-2)
        assert step.scalars()["opt_steps"] == 2.0


def test_two_steps_f32_six_modules_match_oracle():
    """the no-AMP mode, r = 4, six modules, at the bounds of tests/test_gpu_lora_wide.py::test_f32_full_step_rank32_matches_oracle (:322-333)"""
    B, hw, D = 2, 16, 64
    st_ref, step, added = build_step(4, SIX, B, hw, D, use_scaler=False, mode="fp32")
    assert step.te.extra["fc2"].w2_fwd.dtype == torch.float32 and step.te.extra["fc2"].w2_t is None
    g = torch.Generator().manual_seed(5)
    te_ref = st_ref.te
    for it in range(2):
        x0, noise, t, ids, pids = _draw(step, added, g, B, hw)
        before = {n: s_[0].clone() for n, s_ in _hip_sets(step.te).items()}
        out = st_ref.step(x0, noise, t, ids, pids)
        step.step_eager()
        sc = step.scalars()
        assert sc["found_inf"] == 0.0 and sc["loss_scale"] == 1.0
        assert abs(sc["loss_mse"] - out["mse"]) < 1e-5 * abs(out["mse"]) + 1e-7, (sc, out["mse"])
        assert abs(sc["loss_kpl"] - out["kpl"]) < 1e-4 * abs(out["kpl"]) + 1e-7, (sc, out["kpl"])
        clip = min(1.0, 1.0 / (out["lora_grad_norm"] + 1e-6))
        assert abs(sc["grad_norm"] - out["lora_grad_norm"]) < 1e-4 * out["lora_grad_norm"]
        gA, gB, gx = LT.split_step_grads(out["g_lora"], te_ref)
        want = {"qkv": (gA, gB), **gx}
        ref = _masters(te_ref)
        for n, (A_, B_, gA_, gB_) in _hip_sets(step.te).items():
            parity(f"fp32 six modules step {it} grad {n} lora_A", gA_ * clip, want[n][0], rel=1e-4, maxabs=1e-4)
            parity(f"fp32 six modules step {it} grad {n} lora_B", gB_ * clip, want[n][1], rel=1e-4, maxabs=1e-4)
            assert (A_.cpu() - ref[n][0]).abs().max().item() < 2e-5, n            # < lr / 2: no element moved the other way
            assert not torch.equal(A_, before[n]), n
        parity(f"fp32 six modules step {it} grad added rows", step.te.grad_added, out["g_emb_added"], rel=1e-4, maxabs=1e-4)
        w, wr = step.te.token_table.cpu(), te_ref.token_embedding.weight.detach()
        torch.testing.assert_close(w[:49408], wr[:49408], rtol=1e-6, atol=1e-7)
        parity(f"fp32 six modules step {it} updated added rows", w[added], wr[added], rel=2e-4, maxabs=5e-4)
    assert step.scalars()["opt_steps"] == 2.0


# ------------------------------------------------------------------------------------------------ 5. / 6. replay, the default list
def _params(step):
    return [step.flat_lora.clone(), step.te.token_table[49408:].clone(), step.state.clone()]


def test_graph_replay_equals_eager_six_modules():
    """as tests/test_gpu_lora_wide.py::test_graph_replay_equals_eager_rank16: nothing on the extra modules' path allocates or synchronises"""
    B, hw, D = 2, 16, 64
    outs = []
    for mode in ("eager", "graph"):
        st_ref, step, added = build_step(4, SIX, B, hw, D)
        _draw(step, added, torch.Generator().manual_seed(6), B, hw)
        if mode == "graph":
            step.capture(warmup=2)
            step.replay(); step.replay()
        else:
            for _ in range(4):
                step.step_eager()
        torch.cuda.synchronize()
        outs.append(_params(step))
    assert outs[0][0].numel() == step.n_lora
    for a, b in zip(*outs):
        torch.testing.assert_close(a, b, rtol=0, atol=0)


def test_default_list_spelled_out_is_the_default_bit_for_bit():
    """lora_targets = q_proj k_proj v_proj given explicitly: the same flat buffers, launches and bytes as an encoder built without the argument"""
    from test_gpu_lora_wide import build_step as build_default
    B, hw, D = 2, 16, 64
    outs = []
    for explicit in (False, True):
        if explicit:
            st_ref, step, added = build_step(4, list(LT.QKV), B, hw, D)
        else:
            st_ref, step, added = build_default(4, B, hw, D)
        assert step.te.extra == {} and step.te.lora_targets == LT.QKV
        assert step.flat_lora.numel() == step.te.lora_A.numel() + step.te.lora_B.numel() == step.n_lora
        _draw(step, added, torch.Generator().manual_seed(6), B, hw)
        for _ in range(2):
            step.step_eager()
        torch.cuda.synchronize()
        outs.append(_params(step) + [step.flat_grad.clone()])
    for a, b in zip(*outs):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ 7. the CLI, the reader, composition
# The composed encoder against the fp32 oracle on the CLI's tiny model directory (hidden 128, 4 heads, erf GELU, the CLI's seeded random weights --
# not the D = 64 oracle model ENC was set on).  The q/k/v-only list run through this same test -- the arithmetic of the code before
# --lora_target_modules -- measures rel-L2 5.200e-4, max-abs 5.900e-4, worst channel 1.840e-3: above ENC's 5e-4 on its own.  The bound here is
# therefore the larger of ENC and twice that figure (independent roundings add in quadrature; six adapted products instead of three, one of them
# four times as long, multiply the variance by about 3); the six-module list measures 5.164e-4 / 7.273e-4 / 2.046e-3.  DESIGN 7.3.
QKV_ON_CLI_MODEL = dict(rel=5.200e-4, maxabs=5.900e-4, ch_rel=1.840e-3)
COMPOSED = dict(ch_dim=2, **{k: max(ENC[k], 2 * v) for k, v in QKV_ON_CLI_MODEL.items()})


@pytest.mark.parametrize("modules", [LT.QKV, SIX], ids=["qkv", "six"])
def test_cli_trains_reads_back_and_composes(tmp_path, monkeypatch, modules):
    """train_textboost.py --lora_target_modules <list> --mixed_precision fp16, two steps on the tiny model directory of
    tests/test_gpu_lora_wide.py; the adapter files list and hold the trained modules; generate.read_run_dir + load_text_encoder reproduce the
    trainer's encoder (the reader bound of tests/test_gpu_lora_wide.py:406); composed with a q/k/v-only run, the loaded encoder equals the oracle
    encoder with sum_i w_i B_i A_i merged into every adapted weight, at COMPOSED (above).  The q/k/v-only list is the baseline the bound is
    derived from and runs through the same body."""
    pytest.importorskip("transformers")
    from safetensors.torch import load_file, save_file
    sys.path.insert(0, ROOT)
    import train_textboost as T
    from oracle.clip_text import CLIPTextCfg, TextBoostEncoder, add_tokens
    from test_gpu_generate import _write_tokenizer
    from test_gpu_lora_wide import _tiny_model_dir
    from textboost_amd import checkpoint as ckpt
    from textboost_amd import generate as G
    from textboost_amd import text_encoder as TE
    from textboost_amd.compose import compose_runs
    m = tmp_path / "sd2-tiny"
    _tiny_model_dir(m)
    monkeypatch.chdir(tmp_path)
    students = []

    class Recorded(TE.HipTextEncoder):     # the trainer's student encoder and the base weights it was built from
        def __init__(self, geo, state_dict, *a, **k):
            super().__init__(geo, state_dict, *a, **k)
            if k.get("lora_rank", 0):
                students.append((self, state_dict))

    monkeypatch.setattr(TE, "HipTextEncoder", Recorded)
    out = str(tmp_path / "run")
    args = T.parse_args(["--pretrained_model_name_or_path", str(m), "--output_dir", out, "--train_batch_size", "2", "--resolution", "128",
                         "--max_train_steps", "2", "--placeholder_token", "<dog>", "--lora_rank", "4", "--mixed_precision", "fp16", "--seed", "5",
                         "--lora_target_modules", *modules])
    T.main(args)
    monkeypatch.setattr(TE, "HipTextEncoder", Recorded.__mro__[1])
    cfg = json.load(open(os.path.join(out, "text_encoder", "adapter_config.json")))
    assert cfg["r"] == 4 and cfg["lora_alpha"] == 4 and cfg["target_modules"] == list(modules)
    sd = load_file(os.path.join(out, "text_encoder", "adapter_model.safetensors"))
    assert len(sd) == 2 * len(modules) * 2
    if modules == SIX:
        assert sd[LT.key(1, "fc1", "A")].shape == (4, 128) and sd[LT.key(1, "fc1", "B")].shape == (256, 4)
        assert sd[LT.key(0, "fc2", "A")].shape == (4, 256) and sd[LT.key(0, "fc2", "B")].shape == (128, 4)
        assert sd[LT.key(1, "out_proj", "A")].shape == (4, 128) and sd[LT.key(1, "out_proj", "B")].shape == (128, 4)
    for n in modules:                                                                         # every module's adapter trained
        assert any(sd[LT.key(i, n, "B")].abs().max() > 0 for i in range(2)), n
    (te, csd), = students
    assert tuple(te.extra) == modules[3:]
    save_file({k: v.detach().float().cpu().contiguous() for k, v in csd.items()}, str(m / "text_encoder" / "model.safetensors"))
    _write_tokenizer(str(m / "tokenizer"))
    run = G.read_run_dir(out)
    assert run.rank == 4 and G.lora_targets_of(run.lora) == modules and [n for n, _ in run.tokens] == ["<dog>"]
    ids = torch.randint(1000, 40000, (2, 77), generator=torch.Generator().manual_seed(0))
    ids[:, 0] = 49406
    ids[0, 3] = 49408
    ids[0, 9:] = 49407
    ids[1, 30:] = 49407
    with torch.no_grad():
        loaded, tok = G.load_text_encoder(str(m), run, 2, dev)
        assert tuple(loaded.extra) == modules[3:] and tok.convert_tokens_to_ids(["<dog>"]) == [49408]
        got = loaded.forward(ids.to(dev)).view(2, 77, 128).clone()
        te.pack_lora()
        want = te.forward(ids.to(dev)).view(2, 77, 128)
    parity(f"loaded {len(modules)}-module encoder vs the trainer's", got, want, **ENC)
    # ---- composed with a q/k/v-only run of rank 4 (written through checkpoint.py, non-zero B)
    g = torch.Generator().manual_seed(9)
    stub = types.SimpleNamespace(geo=types.SimpleNamespace(hidden_size=128, num_layers=2), r=4, lora_A=torch.randn(2, 12, 128, generator=g) / 4,
                                 lora_B=torch.randn(2, 3 * 128, 4, generator=g) * 0.05, token_table=torch.randn(1, 128, generator=g) * 0.01)
    sdir = str(tmp_path / "style")
    ckpt.save_text_encoder_adapter(stub, os.path.join(sdir, "text_encoder"), "tiny")
    ckpt.save_token_embeddings(stub, sdir, {"<style>": 0}, None)
    style = G.read_run_dir(sdir)
    w = (1.0, 0.7)
    both = compose_runs([run, style], w)
    assert both.rank == 8 and G.lora_targets_of(both.lora) == modules
    ccfg = CLIPTextCfg(hidden_size=128, intermediate_size=256, num_layers=2, num_heads=4, act="gelu")
    with torch.no_grad():
        comp, tok2 = G.load_text_encoder(str(m), both, 2, dev)
        assert comp.r == 8 and tok2.convert_tokens_to_ids(["<dog>", "<style>"]) == [49408, 49409]
        ids[1, 5] = 49409
        got = comp.forward(ids.to(dev)).view(2, 77, 128).clone()
        ref = TextBoostEncoder(ccfg, r=0)
        ref.load_hf_state_dict({k: v.detach().float().cpu() for k, v in csd.items()})
        for i, layer in enumerate(ref.layers):
            for n in SIX:
                for r_, w_ in ((run, w[0]), (style, w[1])):
                    if LT.key(i, n, "A") in r_.lora:
                        getattr(layer, LT.ATTR[n]).weight.add_(w_ * (r_.lora[LT.key(i, n, "B")] @ r_.lora[LT.key(i, n, "A")]))
        rows = add_tokens(ref, [0, 0])
        for tid, (_, v) in zip(rows, both.tokens):
            ref.token_embedding.weight[tid] = v
        ref.set_null_embedding(comp.null_embedding.cpu())      # (the pins copy this tensor: the loaded encoder's own, so pinned rows compare exactly)
        want = ref(ids)
        ids_alone = ids.clone()
        ids_alone[1, 5] = 1000                                 # (the six-module run's own table has no <style> row)
        alone = loaded.forward(ids_alone.to(dev)).view(2, 77, 128)
    parity(f"composed {len(modules)}-module + q/k/v run vs the oracle with merged weights", got, want, **COMPOSED)
    gap = rel_err(got[0], alone[0])
    print(f"[lora targets] composed vs the six-module run alone: rel-L2 {gap:.3e}")
    assert gap > 10 * ENC["rel"]                               # the second run matters at this bound
