"""Text-encoder LoRA at ranks 9 .. 64 (csrc/lora_wide.hip): the MFMA weight-gradient kernel, the packed operands, the encoder against the oracle,
whole optimizer steps in the three numeric modes, the CLI and the run-directory reader.  Every check at r > 8 is refused with -22 by the rank <= 8
kernels; the bounds are those of the rank-4 / rank-8 tests named in each docstring."""
import json
import os
import sys

import pytest
import torch

from parity import parity

pytestmark = pytest.mark.gpu
dev = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rel_err(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _amax(x):
    """largest magnitude; 0 for an empty selection (r = 64 leaves no padding columns)"""
    return x.abs().max().item() if x.numel() else 0.0


def _packed(A, Bc, Dm, K, r, P, scaling, dtype=torch.float16, layers=1):
    from textboost_amd import ops
    rp, Rp = ops.lora_wide_dims(r, P)
    a_pad = torch.full((layers, Rp, K), 7.0, device=dev, dtype=dtype)     # (pre-filled: the launch writes the padding zeros itself)
    w2f = torch.full((layers, P * Dm, Rp), 7.0, device=dev, dtype=dtype)
    w2t = torch.full((layers, Rp, P * Dm), 7.0, device=dev, dtype=dtype)
    w2d = torch.full((layers, K, Rp), 7.0, device=dev, dtype=dtype)
    ops.lora_wide_pack(A, Bc, a_pad, w2f, w2t, w2d, Dm, K, r, rp, P, scaling=scaling, layers=layers)
    return rp, Rp, a_pad, w2f, w2t, w2d


def _pad_mask(r, rp, Rp, P):
    live = torch.zeros(Rp, dtype=torch.bool)
    for p_ in range(P):
        live[p_ * rp:p_ * rp + r] = True
    return live.to(dev)


# ------------------------------------------------------------------------------------------------ 1. the weight-gradient kernel
@pytest.mark.parametrize("r,Dm,K,M", [(12, 192, 256, 77), (16, 192, 256, 154), (33, 192, 256, 154), (32, 768, 768, 154), (64, 768, 768, 616),
                                      (64, 1024, 1024, 154)])
def test_wide_weight_gradients_match_autograd(r, Dm, K, M):
    """tb_lora_wide_wgrad vs autograd, by the protocol and at the bounds of tests/test_gpu_small.py::test_lora_backward_ranks (scaling 0.5; dA, dB
    rel-L2 < 5e-3, dt < 3e-3).  M is never a multiple of the 64-row slab (tails of 13, 26 and 40 rows); r = 12 and 33 leave rank tiles partly
    live, r = 33 gives dB rows that are not 8-byte aligned.  The gradient buffers start from constants (the launch adds), the padding columns of
    t / dt are exactly zero, and a second run on the same inputs gives the same bits."""
    from textboost_amd import ops
    torch.manual_seed(r)
    P = 3
    x = torch.randn(M, K, device=dev).half()
    A = torch.randn(P * r, K, device=dev) / r
    Bc = torch.randn(P * Dm, r, device=dev) * 0.1
    rp, Rp, a_pad, w2f, w2t, w2d = _packed(A, Bc, Dm, K, r, P, 0.5)
    live = _pad_mask(r, rp, Rp, P)
    t = torch.full((M, Rp), 3.0, device=dev, dtype=torch.float16)
    ops.gemm(x, a_pad[0], t)                                   # the new down projection
    dY = torch.randn(M, P * Dm, device=dev).half()
    dt = torch.full((M, Rp), 3.0, device=dev, dtype=torch.float16)
    ops.gemm(dY, w2t[0], dt)
    assert _amax(t[:, ~live]) == 0 and _amax(dt[:, ~live]) == 0
    runs = []
    for _ in range(2):
        dA = torch.full_like(A, 0.25); dB = torch.full_like(Bc, -0.5)
        ops.lora_wide_wgrad(dY, x, t, dt, dA, dB, Dm, K, r, rp, P, scaling=0.5)
        runs.append((dA, dB))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    dA, dB = runs[0][0] - 0.25, runs[0][1] + 0.5
    xr = x.float()
    Ar = A.clone().requires_grad_(True); Br = Bc.clone().requires_grad_(True)
    lo = 0.5 * torch.cat([(xr @ Ar[p_ * r:(p_ + 1) * r].T) @ Br[p_ * Dm:(p_ + 1) * Dm].T for p_ in range(P)], dim=1)
    lo.backward(dY.float())
    e_a, e_b = rel_err(dA, Ar.grad), rel_err(dB, Br.grad)
    ref_dt = 0.5 * torch.cat([dY.float()[:, p_ * Dm:(p_ + 1) * Dm] @ Bc[p_ * Dm:(p_ + 1) * Dm].half().float() for p_ in range(P)], dim=1)
    e_t = rel_err(dt[:, live], ref_dt)
    ref_t = torch.cat([xr @ A[p_ * r:(p_ + 1) * r].half().float().T for p_ in range(P)], dim=1)
    print(f"[lora wide] r {r} D {Dm} K {K} M {M}: dA {e_a:.3e} dB {e_b:.3e} dt {e_t:.3e} t {rel_err(t[:, live], ref_t):.3e}")
    assert rel_err(t[:, live], ref_t) < 2e-3
    assert e_a < 5e-3 and e_b < 5e-3
    assert e_t < 3e-3


def test_wide_weight_gradients_ignore_the_padding_columns():
    """columns j >= r inside an adapter's rp columns are neither accumulated into a live element nor stored: non-finite values planted there
    (the executor keeps zeros there) leave both gradients bit-identical"""
    from textboost_amd import ops
    torch.manual_seed(1)
    r, Dm, K, M, P = 12, 64, 64, 77, 3
    rp, Rp = ops.lora_wide_dims(r, P)
    live = _pad_mask(r, rp, Rp, P)
    x = torch.randn(M, K, device=dev).half(); dY = torch.randn(M, P * Dm, device=dev).half()
    t = torch.randn(M, Rp, device=dev).half(); dt = torch.randn(M, Rp, device=dev).half()
    t[:, ~live] = 0; dt[:, ~live] = 0
    outs = []
    for poison in (False, True):
        if poison:
            t[:, ~live] = float("nan"); dt[:, ~live] = float("inf")
        dA = torch.zeros(P * r, K, device=dev); dB = torch.zeros(P * Dm, r, device=dev)
        ops.lora_wide_wgrad(dY, x, t, dt, dA, dB, Dm, K, r, rp, P)
        outs.append((dA, dB))
    assert torch.isfinite(outs[1][0]).all() and torch.isfinite(outs[1][1]).all()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


# ------------------------------------------------------------------------------------------------ 2. forward pieces
@pytest.mark.parametrize("r", [12, 16, 64])
def test_wide_packed_operands_and_two_source_forward(r):
    """the packed operands equal their definitions (as the lora_pack asserts of tests/test_gpu_small.py), stacked layers equal per-layer launches,
    and x W^T + scaling (x A^T) B^T through the two-source GEMM: rel-L2 < 3e-3"""
    from textboost_amd import ops
    torch.manual_seed(100 + r)
    M, K, Dm, P, sc = 154, 128, 128, 3, 0.5
    A = torch.randn(2, P * r, K, device=dev) / r
    Bc = torch.randn(2, P * Dm, r, device=dev) * 0.1
    rp, Rp, a_pad, w2f, w2t, w2d = _packed(A, Bc, Dm, K, r, P, sc, layers=2)
    assert rp % 8 == 0 and rp >= r and Rp % 64 == 0 and Rp >= P * rp
    live = _pad_mask(r, rp, Rp, P)
    for l in range(2):
        ref = torch.zeros(P * Dm, Rp, device=dev)
        refa = torch.zeros(Rp, K, device=dev)
        for p_ in range(P):
            ref[p_ * Dm:(p_ + 1) * Dm, p_ * rp:p_ * rp + r] = sc * Bc[l, p_ * Dm:(p_ + 1) * Dm]
            refa[p_ * rp:p_ * rp + r] = A[l, p_ * r:(p_ + 1) * r]
        assert torch.equal(w2f[l].float(), ref.half().float())
        assert torch.equal(w2t[l], w2f[l].T)
        assert torch.equal(a_pad[l].float(), refa.half().float())
        assert torch.equal(w2d[l], a_pad[l].T)
        assert _amax(a_pad[l][~live]) == 0 and _amax(w2f[l][:, ~live]) == 0
        one = _packed(A[l].contiguous(), Bc[l].contiguous(), Dm, K, r, P, sc)
        assert all(torch.equal(o[0], s[l]) for o, s in zip(one[2:], (a_pad, w2f, w2t, w2d)))
    # the fp32 form of the same launch (no w2_t: the fp32 backward multiplies by w2_fwd through a transposed view)
    a32 = torch.empty(2, Rp, K, device=dev); f32 = torch.empty(2, P * Dm, Rp, device=dev); d32 = torch.empty(2, K, Rp, device=dev)
    ops.lora_wide_pack(A, Bc, a32, f32, None, d32, Dm, K, r, rp, P, scaling=sc, layers=2)
    assert torch.equal(a32.half(), a_pad) and torch.equal(f32.half(), w2f) and torch.equal(d32, a32.transpose(1, 2))
    assert torch.equal(a32[0][live], A[0]) and torch.equal(f32[0][:Dm, :r], sc * Bc[0, :Dm])
    # forward
    x = torch.randn(M, K, device=dev).half()
    t = torch.empty(M, Rp, device=dev, dtype=torch.float16)
    ops.gemm(x, a_pad[0], t)
    W = (torch.randn(P * Dm, K, device=dev) / 11).half()
    y = torch.empty(M, P * Dm, device=dev, dtype=torch.float16)
    ops.gemm(x, W, y, A2=t, W2=w2f[0])
    xr = x.float()
    lo = sc * torch.cat([(xr @ A[0, p_ * r:(p_ + 1) * r].T) @ Bc[0, p_ * Dm:(p_ + 1) * Dm].T for p_ in range(P)], dim=1)
    e = rel_err(y, xr @ W.float().T + lo)
    print(f"[lora wide] r {r}: two-source forward {e:.3e}")
    assert e < 3e-3
    assert rel_err(y, xr @ W.float().T) > 10 * 3e-3      # the adapter term matters at this bound


# ------------------------------------------------------------------------------------------------ 3. the encoder against the oracle
@pytest.mark.parametrize("r", [12, 16, 64])
def test_text_encoder_wide_ranks_match_oracle(r):
    """the body and the bounds of tests/test_gpu_model.py::test_text_encoder_forward_backward_match_oracle at make_encoders(B=3, D=64, r=r),
    including the frozen `extra_ids` rows riding in the student's launches"""
    from oracle import train_step as ts
    from test_gpu_model import lora_grads_from_oracle, make_encoders
    B, D = 3, 64
    student, teacher, hip, hip_teacher, added, null = make_encoders(B, D, r=r)
    assert hip.wide and hip.rp >= r
    g = torch.Generator().manual_seed(2)
    ids = ts.synthetic_ids(B, added, g)
    ids[1, 1:] = 49407   # a null prompt row -> pinned, zero gradient
    out_ref = student(ids)
    R = torch.randn(B, 77, D, generator=g)
    (out_ref * R).sum().backward()
    hip.pack_lora()
    out = hip.forward(ids.to(dev), slot=0)
    parity(f"r={r} tiny encoder hidden states", out.view(B, 77, D), out_ref, rel=5e-4, maxabs=1e-3, ch_dim=2, ch_rel=2e-3)
    assert torch.equal(out.view(B, 77, D)[1].cpu(), null)
    hip.zero_grad()
    hip.backward(R.view(B * 77, D).to(dev).contiguous(), slot=0)
    gA, gB = lora_grads_from_oracle(student)
    parity(f"r={r} tiny encoder grad lora_A", hip.grad_A, gA, rel=1.5e-3, maxabs=2e-3, ch_dim=0, ch_rel=2e-3)
    parity(f"r={r} tiny encoder grad lora_B", hip.grad_B, gB, rel=1.5e-3, maxabs=2e-3, ch_dim=0, ch_rel=2e-3)
    parity(f"r={r} tiny encoder grad added rows", hip.grad_added, student.token_embedding.weight.grad[added], rel=1e-3, maxabs=1.5e-3)
    pids = ts.synthetic_ids(B, added, g, prior=True)
    with torch.no_grad():
        t_ref = teacher(pids)
    merged = hip.forward(ids.to(dev), slot=0, extra_ids=pids.to(dev), extra_table=hip_teacher.token_table.float())
    assert torch.equal(merged[:B * 77], out)
    parity(f"r={r} teacher rows inside the student pass", merged[B * 77:].view(B, 77, D), t_ref, rel=5e-4, maxabs=1e-3)
    gA0, gB0, gE0 = hip.grad_A.clone(), hip.grad_B.clone(), hip.grad_added.clone()
    hip.zero_grad()
    hip.backward(R.view(B * 77, D).to(dev).contiguous(), slot=0)
    assert torch.equal(hip.grad_A, gA0) and torch.equal(hip.grad_B, gB0) and torch.equal(hip.grad_added, gE0)


# ------------------------------------------------------------------------------------------------ 4. whole steps
def build_step(r, B=2, hw=16, D=64, use_scaler=True):
    """tests/test_gpu_model.py::build_step with the adapter rank as a parameter"""
    from oracle import train_step as ts
    from test_gpu_model import make_encoders, make_unet
    from textboost_amd.trainer import StepHyper, TextBoostStep
    ref_unet, hip_unet, _ = make_unet(B, hw, D, seed=3)
    student, teacher, hip_te, hip_teacher, added, null = make_encoders(B, D, r=r, seed=4)
    st_ref = ts.TrainState(student, teacher, ref_unet, added, ts.StepConfig())
    hp = StepHyper(use_grad_scaler=use_scaler, init_scale=65536.0 if use_scaler else 1.0)
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


def _oracle_lora_grads(out, n_layers):
    gA = torch.stack([torch.cat(out["g_lora"][6 * l + 0: 6 * l + 6: 2]) for l in range(n_layers)])
    gB = torch.stack([torch.cat(out["g_lora"][6 * l + 1: 6 * l + 6: 2]) for l in range(n_layers)])
    return gA, gB, min(1.0, 1.0 / (out["lora_grad_norm"] + 1e-6))   # the oracle's g_lora are post-clip


def test_full_step_rank16_matches_oracle_elementwise():
    """two optimizer steps at r = 16 at the bounds of tests/test_gpu_model.py::test_full_step_matches_oracle_elementwise"""
    B, hw, D = 2, 16, 64
    st_ref, step, added = build_step(16, B, hw, D)
    assert step.te.wide
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
        gA, gB, clip = _oracle_lora_grads(out, len(te_ref.layers))
        assert abs(sc["grad_norm"] - out["lora_grad_norm"]) < 5e-2 * out["lora_grad_norm"]
        parity(f"r=16 step {it} grad lora_A", step.te.grad_A * inv * clip, gA, rel=4e-3, maxabs=6e-3)
        parity(f"r=16 step {it} grad lora_B", step.te.grad_B * inv * clip, gB, rel=4e-3, maxabs=6e-3)
        parity(f"r=16 step {it} grad added rows", step.te.grad_added * inv, out["g_emb_added"], rel=4e-3, maxabs=6e-3)
        w = step.te.token_table.cpu()
        wr = te_ref.token_embedding.weight.detach()
        torch.testing.assert_close(w[:49408], wr[:49408], rtol=1e-6, atol=1e-7)       # decay-only rows
        assert (w[added] - wr[added]).abs().max().item() < 2.5e-3                     # <= ~2 * emb_lr (Adam step-1 sign flips)
        assert rel_err(w[added], wr[added]) < 2e-3
        A_ref = torch.stack([torch.cat([l.q.lora_A, l.k.lora_A, l.v.lora_A]) for l in te_ref.layers]).detach()
        assert (step.te.lora_A.cpu() - A_ref).abs().max().item() < 1.5e-4             # <= ~2 * lr
    assert step.scalars()["opt_steps"] == 2.0


def _replay_vs_eager(use_scaler):
    B, hw, D = 2, 16, 64
    outs = []
    for mode in ("eager", "graph"):
        st_ref, step, added = build_step(16, B, hw, D, use_scaler=use_scaler)
        _draw(step, added, torch.Generator().manual_seed(6), B, hw)
        if mode == "graph":
            step.capture(warmup=2)
            step.replay(); step.replay()
        else:
            for _ in range(4):
                step.step_eager()
        torch.cuda.synchronize()
        outs.append((step.te.lora_A.clone(), step.te.lora_B.clone(), step.te.token_table[49408:].clone(), step.state.clone()))
    for a, b in zip(*outs):
        torch.testing.assert_close(a, b, rtol=0, atol=0)


def test_graph_replay_equals_eager_rank16():
    """as tests/test_gpu_model.py::test_graph_replay_equals_eager: nothing in the wide path allocates or synchronises inside a launch"""
    _replay_vs_eager(True)


def test_bf16_full_step_rank16_matches_oracle():
    """the same two steps on the bfloat16 build, at the bounds of tests/test_gpu_bf16.py::test_bf16_full_step_runs_without_a_grad_scaler_and_matches_oracle"""
    from textboost_amd import _lib as L
    with L.use_half("bf16"):
        B, hw, D = 2, 16, 64
        st_ref, step, added = build_step(16, B, hw, D, use_scaler=False)
        assert step.te.wide and step.te.w2_t.dtype == torch.bfloat16
        g = torch.Generator().manual_seed(5)
        for it in range(2):
            x0, noise, t, ids, pids = _draw(step, added, g, B, hw)
            out = st_ref.step(x0, noise, t, ids, pids)
            step.step_eager()
            sc = step.scalars()
            assert sc["found_inf"] == 0.0 and sc["loss_scale"] == 1.0
            assert abs(sc["loss_mse"] - out["mse"]) < 5e-2 * abs(out["mse"]) + 1e-3, (sc, out["mse"])
            gA, gB, clip = _oracle_lora_grads(out, len(st_ref.te.layers))
            parity(f"bf16 r=16 step {it} grad lora_A", step.te.grad_A * clip, gA, rel=3.2e-2, maxabs=5e-2)
            parity(f"bf16 r=16 step {it} grad added rows", step.te.grad_added, out["g_emb_added"], rel=3.2e-2, maxabs=5e-2)
        assert step.scalars()["opt_steps"] == 2.0


def test_f32_full_step_rank32_matches_oracle():
    """the no-AMP mode at r = 32 (3 r > 64: the width the fp32 pack refused), at the step bounds of
    tests/test_gpu_f32.py::test_full_step_f32_matches_oracle_elementwise"""
    from oracle import train_step as ts
    from test_gpu_f32 import _encoders_f32, _small_unet_f32
    from textboost_amd.trainer import StepHyper, TextBoostStep
    B, hw, D = 2, 16, 64
    ref_unet, hip_unet = _small_unet_f32(B, hw, D, seed=3)
    student, teacher, hip_te, hip_teacher, added, null = _encoders_f32(B, D, r=32, seed=4)
    assert hip_te.wide and hip_te.w2_fwd.dtype == torch.float32
    st_ref = ts.TrainState(student, teacher, ref_unet, added, ts.StepConfig())
    step = TextBoostStep(hip_unet, hip_te, hip_teacher, StepHyper(use_grad_scaler=False, init_scale=1.0), (B, 4, hw, hw), device=dev)
    step.external_noise = True
    g = torch.Generator().manual_seed(5)
    te_ref = st_ref.te
    for it in range(2):
        x0, noise, t, ids, pids = _draw(step, added, g, B, hw)
        A_before = step.te.lora_A.clone()
        out = st_ref.step(x0, noise, t, ids, pids)
        step.step_eager()
        sc = step.scalars()
        assert sc["found_inf"] == 0.0 and sc["loss_scale"] == 1.0
        assert abs(sc["loss_mse"] - out["mse"]) < 1e-5 * abs(out["mse"]) + 1e-7, (sc, out["mse"])
        assert abs(sc["loss_kpl"] - out["kpl"]) < 1e-4 * abs(out["kpl"]) + 1e-7, (sc, out["kpl"])
        gA, gB, clip = _oracle_lora_grads(out, len(te_ref.layers))
        assert abs(sc["grad_norm"] - out["lora_grad_norm"]) < 1e-4 * out["lora_grad_norm"]
        parity(f"fp32 r=32 step {it} grad lora_A", step.te.grad_A * clip, gA, rel=1e-4, maxabs=1e-4)
        parity(f"fp32 r=32 step {it} grad lora_B", step.te.grad_B * clip, gB, rel=1e-4, maxabs=1e-4)
        parity(f"fp32 r=32 step {it} grad added rows", step.te.grad_added, out["g_emb_added"], rel=1e-4, maxabs=1e-4)
        w, wr = step.te.token_table.cpu(), te_ref.token_embedding.weight.detach()
        torch.testing.assert_close(w[:49408], wr[:49408], rtol=1e-6, atol=1e-7)
        parity(f"fp32 r=32 step {it} updated added rows", w[added], wr[added], rel=2e-4, maxabs=5e-4)
        A_ref = torch.stack([torch.cat([l.q.lora_A, l.k.lora_A, l.v.lora_A]) for l in te_ref.layers]).detach()
        assert (step.te.lora_A.cpu() - A_ref).abs().max().item() < 2e-5           # < lr / 2: no element moved the other way
        assert not torch.equal(step.te.lora_A, A_before)
    assert step.scalars()["opt_steps"] == 2.0


# ------------------------------------------------------------------------------------------------ 5. the CLI and the reader
def _tiny_model_dir(m):
    """the model directory of tests/test_gpu_edge.py::test_cli_reads_the_architecture_from_the_model_directory (no weights: seeded random init)"""
    for sub in ("unet", "text_encoder", "scheduler"):
        (m / sub).mkdir(parents=True)
    json.dump({"attention_head_dim": [2, 4, 8, 8], "block_out_channels": [64, 128, 256, 256], "cross_attention_dim": 128,
               "down_block_types": ["CrossAttnDownBlock2D"] * 3 + ["DownBlock2D"], "up_block_types": ["UpBlock2D"] + ["CrossAttnUpBlock2D"] * 3,
               "in_channels": 4, "out_channels": 4, "layers_per_block": 2, "norm_num_groups": 32, "norm_eps": 1e-5,
               "use_linear_projection": True, "act_fn": "silu"}, open(m / "unet" / "config.json", "w"))
    json.dump({"hidden_act": "gelu", "hidden_size": 128, "intermediate_size": 256, "num_attention_heads": 4, "num_hidden_layers": 2,
               "max_position_embeddings": 77, "vocab_size": 49408, "layer_norm_eps": 1e-5}, open(m / "text_encoder" / "config.json", "w"))
    json.dump({"prediction_type": "v_prediction"}, open(m / "scheduler" / "scheduler_config.json", "w"))


def test_cli_rank16_trains_and_the_reader_reproduces_the_encoder(tmp_path, monkeypatch):
    """train_textboost.py --lora_rank 16 --mixed_precision fp16, three steps at the tiny settings of tests/test_gpu_edge.py; the adapter files say
    r = 16; generate.read_run_dir + load_text_encoder on the output directory reproduce the trainer's encoder on the same ids at the bound
    tests/test_gpu_generate.py uses for r = 4 (the encoder-forward bound: 5e-4 / 1e-3 / 2e-3)."""
    pytest.importorskip("transformers")
    from safetensors.torch import load_file, save_file
    sys.path.insert(0, ROOT)
    import train_textboost as T
    from test_gpu_generate import _write_tokenizer
    from textboost_amd import generate as G
    from textboost_amd import text_encoder as TE
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
                         "--max_train_steps", "3", "--placeholder_token", "<dog>", "--lora_rank", "16", "--mixed_precision", "fp16", "--seed", "5"])
    T.main(args)
    monkeypatch.setattr(TE, "HipTextEncoder", Recorded.__mro__[1])
    cfg = json.load(open(os.path.join(out, "text_encoder", "adapter_config.json")))
    assert cfg["r"] == 16 and cfg["lora_alpha"] == 16
    sd = load_file(os.path.join(out, "text_encoder", "adapter_model.safetensors"))
    assert len(sd) == 2 * 3 * 2
    assert sd["base_model.model.text_model.encoder.layers.1.self_attn.q_proj.lora_A.weight"].shape == (16, 128)
    assert sd["base_model.model.text_model.encoder.layers.1.self_attn.v_proj.lora_B.weight"].shape == (128, 16)
    assert any(k.endswith("lora_B.weight") and v.abs().max() > 0 for k, v in sd.items())      # the adapters trained
    d = torch.load(os.path.join(out, "dog.bin"))
    assert d["<dog>"].shape == (128,) and torch.isfinite(d["<dog>"]).all()
    # the reader: the model directory gets the base weights the trainer drew and a tokenizer
    (te, csd), = students
    save_file({k: v.detach().float().cpu().contiguous() for k, v in csd.items()}, str(m / "text_encoder" / "model.safetensors"))
    _write_tokenizer(str(m / "tokenizer"))
    run = G.read_run_dir(out)
    assert run.rank == 16 and [n for n, _ in run.tokens] == ["<dog>"]
    ids = torch.randint(1000, 40000, (2, 77), generator=torch.Generator().manual_seed(0))
    ids[:, 0] = 49406
    ids[0, 3] = 49408
    ids[0, 9:] = 49407
    ids[1, 30:] = 49407
    with torch.no_grad():
        loaded, tok = G.load_text_encoder(str(m), run, 2, dev)
        assert loaded.wide and tok.convert_tokens_to_ids(["<dog>"]) == [49408]
        got = loaded.forward(ids.to(dev)).view(2, 77, 128).clone()
        te.pack_lora()
        want = te.forward(ids.to(dev)).view(2, 77, 128)
    parity("loaded rank-16 encoder vs the trainer's", got, want, rel=5e-4, maxabs=1e-3, ch_dim=2, ch_rel=2e-3)


def test_cli_refuses_rank_65_by_name(tmp_path):
    sys.path.insert(0, ROOT)
    import train_textboost as T
    args = T.parse_args(["--pretrained_model_name_or_path", "/nonexistent/sd15", "--output_dir", str(tmp_path / "o"), "--train_batch_size", "1",
                         "--resolution", "128", "--max_train_steps", "1", "--mixed_precision", "fp16", "--lora_rank", "65"])
    with pytest.raises(NotImplementedError, match="--lora_rank 65"):
        T.main(args)
