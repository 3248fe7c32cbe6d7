"""--use_dora on the GPU (csrc/dora.hip): the three kernels against float64 on the same rounded operands, the tiny encoder and whole
optimizer steps against the oracle with DoRA layers (tests/dora_ref.py) in the three numeric modes, graph replay, resume, and the CLI with the
run-directory reader and inference.py.  Bounds are inherited from the tests of the same quantities (named where they are used); the one bound
of its own is the row norm's 1e-5 against float64 (the band of the project's fp32 kernels is 2e-6 .. 1e-5)."""
import json
import os
import sys

import pytest
import torch

import dora_ref as DR
import lora_targets_ref as LT
from parity import parity

pytestmark = pytest.mark.gpu
dev = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIX = LT.ALL
ENC = dict(rel=5e-4, maxabs=1e-3, ch_dim=2, ch_rel=2e-3)       # tests/test_gpu_lora_targets.py:20
GRAD = dict(rel=1.5e-3, maxabs=2e-3)                           # :21
# hidden states / adapter + magnitude gradients / added rows per mode.  fp16: tests/test_gpu_lora_targets.py:195-205; bf16: its only bf16 bounds
# (:321-322, gradients) and tests/test_gpu_bf16.py:228 for the states; fp32: :348-352 and tests/test_gpu_f32.py:393 for the states
MODE_BOUNDS = {
    "fp16": (ENC, dict(ch_dim=0, ch_rel=2e-3, **GRAD), dict(rel=1e-3, maxabs=1.5e-3)),
    "bf16": (dict(rel=4e-3, maxabs=8e-3), dict(rel=3.2e-2, maxabs=5e-2), dict(rel=3.2e-2, maxabs=5e-2)),
    "fp32": (dict(rel=1e-5, maxabs=2e-5, ch_dim=2, ch_rel=1e-4), dict(rel=1e-4, maxabs=1e-4), dict(rel=1e-4, maxabs=1e-4)),
}


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-300)).item()


# ------------------------------------------------------------------------------------------------ 1. row norms and scales
SHAPES = [(64, 128, 1), (128, 64, 1), (768, 3072, 1), (3072, 768, 1), (64, 192, 3)]      # (K, N, P): the last is q/k/v stacked at D = 64


def _module(K, N, P, r, dtype, seed, layers=2):
    g = torch.Generator().manual_seed(seed)
    W = [(torch.randn(N, K, generator=g) / K ** 0.5).to(dtype).to(dev) for _ in range(layers)]
    A = (torch.randn(layers, P * r, K, generator=g) / r).to(dev)
    B = (torch.randn(layers, N, r, generator=g) * 0.05).to(dev)
    return W, A, B


def _delta64(A, B, P, r, s):
    """s * B A per layer in float64, adapter p on its own rows"""
    D = B.shape[1] // P
    return torch.stack([torch.cat([s * (B[l, p * D:(p + 1) * D].double() @ A[l, p * r:(p + 1) * r].double()) for p in range(P)]) for l in range(B.shape[0])])


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
@pytest.mark.parametrize("r", [4, 16])
@pytest.mark.parametrize("K,N,P", SHAPES)
def test_row_norms_and_scales_against_float64(K, N, P, r, dtype):
    """n = || W + s B A || per row over all layers in one launch and c = m / n, against float64 on the SAME stored W: max relative error 1e-5
    (measured at K = 3072: n 1.14e-7, c 1.50e-7; at K = 64: n 9.6e-8, c 1.3e-7 -- DESIGN 7.4).  The elements behind the outputs stay untouched, and the init form (no m, no c)
    gives the same n."""
    from textboost_amd import ops
    s = 0.5
    W, A, B = _module(K, N, P, r, dtype, seed=K + N + r)
    wp = ops.dora_weight_ptrs(W)
    m = (torch.rand(2, N, device=dev) + 0.5)
    nb = torch.full((2 * N + 5,), 7.0, device=dev)
    cb = torch.full((2 * N + 5,), 7.0, device=dev)
    n, c = nb[:2 * N].view(2, N), cb[:2 * N].view(2, N)
    ops.dora_norms(wp, dtype, A, B, m, n, c, N // P, K, r, P, scaling=s, layers=2)
    assert torch.equal(nb[2 * N:], torch.full_like(nb[2 * N:], 7.0)) and torch.equal(cb[2 * N:], torch.full_like(cb[2 * N:], 7.0))
    n64 = (torch.stack([w.double() for w in W]) + _delta64(A, B, P, r, s)).norm(dim=2)
    e_n = ((n.double() - n64).abs() / n64).max().item()
    e_c = ((c.double() - m.double() / n64).abs() / (m.double() / n64)).max().item()
    plain = torch.stack([w.double() for w in W]).norm(dim=2)
    far = ((plain - n64).abs() / n64).max().item()
    print(f"[dora] norms K {K} N {N} P {P} r {r} {dtype}: n max-rel {e_n:.3e}  c max-rel {e_c:.3e}  (||W|| alone is {far:.3e} away)")
    assert e_n < 1e-5 and e_c < 1e-5
    assert far > 1e-3                                     # the B A term matters at this bound
    n2 = torch.empty(2, N, device=dev)
    ops.dora_norms(wp, dtype, A, B, None, n2, None, N // P, K, r, P, scaling=s, layers=2)
    assert torch.equal(n2, n)


# ------------------------------------------------------------------------------------------------ 2. forward application and backward
def _qgelu(x):
    return x * torch.sigmoid(1.702 * x)


@pytest.mark.parametrize("Mt", [154, 231], ids=["student-only", "with-77-teacher-rows"])
@pytest.mark.parametrize("r", [4, 16])
@pytest.mark.parametrize("K,N,P", SHAPES)
def test_apply_and_backward_against_float64(K, N, P, r, Mt):
    """u from the two-source GEMM (no bias), then tb_dora_apply with the three epilogues the adapted Linears have and tb_dora_bwd, against
    float64 on the same 16-bit operands.  m = 1.5 n on odd columns, n on even ones.  Bounds: y the two-source bound of
    tests/test_gpu_lora_targets.py:106 (3e-3), dU the bound of its t check (2e-3), dm the bound of dB (5e-3); every result is more than ten times
    its bound away from the plain-LoRA one; guard rows and the frozen rows behind the student rows never see m; two launches give the same dm."""
    from textboost_amd import _lib as L
    from textboost_amd import ops
    Ms, PAD, s = 154, 7, 1.0
    f16 = torch.float16
    W, A, B = _module(K, N, P, r, f16, seed=K + N + r + Mt, layers=1)
    D = N // P
    g = torch.Generator().manual_seed(3)
    xb = torch.randn(Mt + PAD, K, generator=g).half().to(dev)
    x = xb[:Mt]
    t = torch.zeros(Mt, 64, device=dev, dtype=f16)
    t[:Ms, :P * r] = (x[:Ms].float() @ A[0].half().float().T).half()          # the frozen rows' K-extension operand stays zero
    W2 = torch.zeros(N, 64, device=dev, dtype=f16)
    for p in range(P):
        W2[p * D:(p + 1) * D, p * r:(p + 1) * r] = (s * B[0, p * D:(p + 1) * D]).half()
    bias = torch.randn(N, generator=g).half().float().to(dev)
    u = torch.empty(Mt, N, device=dev, dtype=f16)
    ops.gemm(x, W[0], u, A2=t, W2=W2)
    n = torch.empty(1, N, device=dev)
    ops.dora_norms(ops.dora_weight_ptrs(W), f16, A, B, None, n, None, D, K, r, P, scaling=s, layers=1)
    c = torch.ones(N, device=dev)          # m = 1.5 n on odd columns, n on even ones: the scale itself, set exactly (fp32 (1.5 n) / n may miss 1.5 by an ulp)
    c[1::2] = 1.5
    ones = torch.ones_like(c)
    u64 = x.double() @ W[0].double().T + t.double() @ W2.double().T
    c64 = c.double()
    v64 = u64 + bias.double()
    v64[:Ms] = c64 * u64[:Ms] + bias.double()
    R = torch.randn(Mt, N, generator=g).to(dev)
    res = {}

    def run(cs):
        yb = torch.full((Mt + PAD, N), 3.0, device=dev, dtype=f16)
        ops.dora_apply(u, cs, bias, yb[:Mt], Ms)
        hb = torch.full((Mt + PAD, N), 3.0, device=dev)
        ops.dora_apply(u, cs, bias, hb[:Mt], Ms, R=R)
        ab = torch.full((Mt + PAD, N), 3.0, device=dev, dtype=f16)
        pb = torch.full((Mt + PAD, N), 3.0, device=dev, dtype=f16)
        ops.dora_apply(u, cs, bias, ab[:Mt], Ms, act=L.ACT_QUICK_GELU, pre=pb[:Mt])
        for o in (yb, hb, ab, pb):
            assert torch.equal(o[Mt:], torch.full_like(o[Mt:], 3.0))
        return yb[:Mt], hb[:Mt], ab[:Mt], pb[:Mt]

    y, h, a, pre = run(c)
    y1, h1, a1, pre1 = run(ones)
    want = {"bias": (y, y1, v64), "bias+R fp32": (h, h1, v64 + R.double()), "act": (a, a1, _qgelu(v64)), "C2": (pre, pre1, v64)}
    for k, (got, plain, ref) in want.items():
        res[k] = (rel_err(got[:Ms], ref[:Ms]), rel_err(plain[:Ms], ref[:Ms]))
        assert torch.equal(got[Ms:], plain[Ms:]), k                    # the frozen rows do not depend on m
        if Mt > Ms:
            assert rel_err(got[Ms:], ref[Ms:]) < 3e-3, k
    # ---- backward: student rows only
    dYb = torch.randn(Ms + PAD, N, generator=g).half().to(dev)
    dY = dYb[:Ms]
    dms = []
    for _ in range(2):
        dUb = torch.full((Ms + PAD, N), 3.0, device=dev, dtype=f16)
        dm = torch.full((N,), 0.25, device=dev)
        ops.dora_bwd(dY, u[:Ms], c, n[0], dUb[:Ms], dm)
        assert torch.equal(dUb[Ms:], torch.full_like(dUb[Ms:], 3.0))
        dms.append(dm)
    assert torch.equal(dms[0], dms[1])
    dU = dUb[:Ms]
    n64 = (W[0].double() + _delta64(A, B, P, r, s)[0]).norm(dim=1)
    ref_dm = (dY.double() * u64[:Ms]).sum(0) / n64
    e_u, far_u = rel_err(dU, dY.double() * c64), rel_err(dY, dY.double() * c64)
    e_m = rel_err(dms[0] - 0.25, ref_dm)
    for k, (e, far) in res.items():
        print(f"[dora] apply {Mt}x{N}x({K}+64) P {P} r {r} {k}: {e:.3e}; plain LoRA {far:.3e}")
    print(f"[dora] bwd   {Ms}x{N} P {P} r {r}: dU {e_u:.3e} (dY itself {far_u:.3e})  dm {e_m:.3e}")
    for k, (e, far) in res.items():
        assert e < 3e-3, k
        assert far > 10 * 3e-3, k
    assert e_u < 2e-3 and far_u > 10 * 2e-3
    assert e_m < 5e-3


def test_kernels_refuse_what_they_cannot_address():
    """odd widths, unaligned pitches and ranks outside 1 .. 64 are TB_EINVAL, not a launch"""
    from textboost_amd import _lib as L
    lib = L.lib()
    u = torch.zeros(8, 64, device=dev, dtype=torch.float16)
    c = torch.ones(64, device=dev)
    st = L.stream()
    ok = lambda N, ldu: lib.tb_dora_apply(L.ptr(u), ldu, L.TB_F16, L.ptr(c), L.ptr(c), 4, 4, N, L.ACT_NONE, None, 0, L.ptr(u), ldu, L.TB_F16, None, 0, st)  # noqa: E731
    assert ok(64, 64) == 0 and ok(60, 64) == -22 and ok(56, 60) == -22
    assert lib.tb_dora_apply(L.ptr(u), 64, L.TB_F16, L.ptr(c), L.ptr(c), 4, 5, 64, L.ACT_NONE, None, 0, L.ptr(u), 64, L.TB_F16, None, 0, st) == -22
    assert lib.tb_dora_bwd(L.ptr(u), 64, L.ptr(u), 64, L.TB_F16, L.ptr(c), L.ptr(c), L.ptr(u), 60, L.ptr(c), 4, 64, st) == -22
    wp = torch.tensor([u.data_ptr()], dtype=torch.int64, device=dev)
    A = torch.zeros(65, 64, device=dev)
    for D, K, r in ((8, 64, 4), (16, 63, 4), (16, 64, 0), (16, 64, 65)):
        assert lib.tb_dora_norms(L.ptr(wp), L.TB_F16, L.ptr(A), L.ptr(A), None, L.ptr(c), None, D, K, r, 1, 1, 1.0, st) == -22
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 3. the tiny encoder
def encoders(B, D, r, modules, seed=0, mode="autocast", n_added=3, perturb=0.2, b_std=0.05):
    """tests/test_gpu_lora_targets.py::encoders with DoRA layers on both sides: B != 0 and m perturbed, so that every path is live
    -> (student, teacher, hip, hip_teacher, added, null, geo, sd)"""
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
                p.normal_(std=b_std)
    LT.add_adapters(student, [m for m in modules if m in LT.EXTRA], r, seed=seed + 50, b_std=b_std)
    DR.add_dora(student, perturb=perturb, seed=seed + 60)
    added = add_tokens(student, [100, 200, 300][:n_added])
    geo = CLIPGeometry(hidden_size=D, intermediate_size=ccfg.intermediate_size, num_layers=ccfg.num_layers, num_heads=ccfg.num_heads)
    sd = {hf: dict(base.named_parameters())[ours].detach() for ours, hf in base.hf_key_map().items()}
    hip = HipTextEncoder(geo, sd, B, mode=mode, lora_rank=r, n_slots=2, device=dev, seed=0, lora_targets=modules, use_dora=True)
    hip.set_null_embedding(null)
    hip.add_tokens([100, 200, 300][:n_added])
    DR.copy_to_hip(student, hip)
    hip_teacher = HipTextEncoder(geo, sd, B, mode="fp32" if mode == "fp32" else "half", lora_rank=0, device=dev)
    hip_teacher.set_null_embedding(null)
    return student, teacher, hip, hip_teacher, added, null, geo, sd


def _half_ctx(mode):
    from textboost_amd import _lib as L
    return L.use_half("bf16" if mode == "bf16" else "fp16")


@pytest.mark.parametrize("r", [4, 16])
@pytest.mark.parametrize("modules", [LT.QKV, SIX], ids=["qkv", "six"])
@pytest.mark.parametrize("mode", ["fp16", "bf16", "fp32"])
def test_tiny_dora_encoder_matches_oracle(mode, modules, r):
    """hidden states, dA, dB, dm and the added rows' gradient of the tiny encoder with DoRA on `modules`, B != 0 and m perturbed by 20 %, against
    the oracle with tests/dora_ref.py's layers, at MODE_BOUNDS (dm at dB's bound); two backward passes give the same bits"""
    from oracle import train_step as ts
    B, D = 3, 64
    b_enc, b_grad, b_add = MODE_BOUNDS[mode]
    with _half_ctx(mode):
        student, teacher, hip, hip_teacher, added, null, _, _ = encoders(B, D, r, modules, mode="fp32" if mode == "fp32" else "autocast")
        assert hip.use_dora and hip.dora_modules() == ("qkv",) + tuple(modules[3:])
        g = torch.Generator().manual_seed(2)
        ids = ts.synthetic_ids(B, added, g)
        ids[1, 1:] = 49407
        out_ref = student(ids)
        R = torch.randn(B, 77, D, generator=g)
        (out_ref * R).sum().backward()
        hip.pack_lora()
        out = hip.forward(ids.to(dev), slot=0)
        tag = f"dora {mode} r={r} {len(modules)} modules"
        parity(f"{tag}: hidden states", out.view(B, 77, D), out_ref, **b_enc)
        assert torch.equal(out.view(B, 77, D)[1].cpu(), null)
        hip.zero_grad()
        hip.backward(R.view(B * 77, D).to(dev).contiguous(), slot=0)
        gA, gB, gx, gm = DR.oracle_grads(student)
        parity(f"{tag}: grad lora_A (q/k/v)", hip.grad_A, gA, **b_grad)
        parity(f"{tag}: grad lora_B (q/k/v)", hip.grad_B, gB, **b_grad)
        parity(f"{tag}: grad magnitude (q/k/v)", hip.grad_mag, gm["qkv"], **b_grad)
        for n, X in hip.extra.items():
            parity(f"{tag}: grad {n} lora_A", X.grad_A, gx[n][0], **b_grad)
            parity(f"{tag}: grad {n} lora_B", X.grad_B, gx[n][1], **b_grad)
            parity(f"{tag}: grad {n} magnitude", X.grad_mag, gm[n], **b_grad)
        parity(f"{tag}: grad added rows", hip.grad_added, student.token_embedding.weight.grad[added], **b_add)
        keep = [hip._dora_of(n).grad_mag.clone() for n in hip.dora_modules()] + [hip.grad_A.clone(), hip.grad_B.clone()]
        hip.zero_grad()
        hip.backward(R.view(B * 77, D).to(dev).contiguous(), slot=0)
        again = [hip._dora_of(n).grad_mag for n in hip.dora_modules()] + [hip.grad_A, hip.grad_B]
        assert all(torch.equal(a_, b_) for a_, b_ in zip(keep, again))


@pytest.mark.parametrize("r", [4, 16])
def test_teacher_rows_never_see_the_magnitudes_and_init_is_plain_lora(r):
    """(a) a KPL-teacher batch riding along: its rows are bit-equal between two runs whose m differs, equal to the un-adapted oracle encoder at
    the teacher bound of tests/test_gpu_lora_targets.py:211, while the student rows move; (b) m = ||W||, B = 0: the DoRA encoder's output equals
    the plain-LoRA encoder's within the forward bound ENC"""
    from oracle import train_step as ts
    from textboost_amd.text_encoder import HipTextEncoder
    B, D = 3, 64
    student, teacher, hip, hip_teacher, added, null, geo, sd = encoders(B, D, r, SIX)
    g = torch.Generator().manual_seed(2)
    ids, pids = ts.synthetic_ids(B, added, g), ts.synthetic_ids(B, added, g, prior=True)
    table = hip_teacher.token_table.float()
    hip.pack_lora()
    first = hip.forward(ids.to(dev), slot=0, extra_ids=pids.to(dev), extra_table=table).clone()
    for n in hip.dora_modules():
        hip._dora_of(n).mag.mul_(1.3)
    hip.pack_lora()
    second = hip.forward(ids.to(dev), slot=0, extra_ids=pids.to(dev), extra_table=table)
    assert torch.equal(first[B * 77:], second[B * 77:])
    assert rel_err(second[:B * 77], first[:B * 77]) > 10 * ENC["rel"]
    with torch.no_grad():
        t_ref = teacher(pids)
    parity(f"dora r={r} teacher rows inside the student pass", second[B * 77:].view(B, 77, D), t_ref, rel=5e-4, maxabs=1e-3)
    # (b)
    kw = dict(mode="autocast", lora_rank=r, device=dev, seed=0, lora_targets=SIX)
    plain, fresh = HipTextEncoder(geo, sd, B, **kw), HipTextEncoder(geo, sd, B, use_dora=True, **kw)
    assert torch.equal(plain.lora_A, fresh.lora_A) and not fresh.lora_B.any()
    w_q = sd["text_model.encoder.layers.1.self_attn.q_proj.weight"].half().double()
    assert ((fresh.mag[1, :D].double().cpu() - w_q.norm(dim=1)).abs() / w_q.norm(dim=1)).max().item() < 1e-5      # m = ||W|| of the STORED weight
    for e in (plain, fresh):
        e.set_null_embedding(null)
        e.add_tokens([100, 200, 300])        # (the ids name the three added rows)
        e.pack_lora()
    assert (fresh.dora_c - 1).abs().max().item() < 1e-6
    parity(f"dora r={r} at init vs the plain LoRA encoder", fresh.forward(ids.to(dev)).view(B, 77, D), plain.forward(ids.to(dev)).view(B, 77, D), **ENC)


# ------------------------------------------------------------------------------------------------ 4. whole steps
def build_step(r, modules, B=2, hw=16, D=64, use_scaler=True, mode="autocast"):
    from oracle import train_step as ts
    from textboost_amd.trainer import StepHyper, TextBoostStep
    if mode == "fp32":
        from test_gpu_f32 import _small_unet_f32
        ref_unet, hip_unet = _small_unet_f32(B, hw, D, seed=3)
    else:
        from test_gpu_model import make_unet
        ref_unet, hip_unet, _ = make_unet(B, hw, D, seed=3)
    student, teacher, hip_te, hip_teacher, added, null, _, _ = encoders(B, D, r, modules, seed=4, mode=mode)
    st_ref = ts.TrainState(student, teacher, ref_unet, added, ts.StepConfig())
    hp = StepHyper(use_grad_scaler=use_scaler, init_scale=65536.0 if use_scaler else 1.0)
    step = TextBoostStep(hip_unet, hip_te, hip_teacher, hp, (B, 4, hw, hw), device=dev)
    step.external_noise = True
    return st_ref, step, added


def _hip_sets(te):
    out = {"qkv": (te.lora_A, te.lora_B, te.mag, te.grad_A, te.grad_B, te.grad_mag)}
    out.update({n: (X.A, X.B, X.mag, X.grad_A, X.grad_B, X.grad_mag) for n, X in te.extra.items()})
    return out


def _masters(te_ref):
    from test_gpu_lora_targets import _masters as ab
    mags = DR.magnitudes(te_ref)
    return {n: (a, b, mags[n]) for n, (a, b) in ab(te_ref).items()}


def test_flat_layout_puts_the_magnitudes_behind_the_adapters_and_before_the_added_rows():
    st_ref, step, added = build_step(4, SIX)
    te = step.te
    sets = _hip_sets(te)
    n_ab = sum(s[0].numel() + s[1].numel() for s in sets.values())
    n_m = sum(s[2].numel() for s in sets.values())
    assert step.n_lora == n_ab + n_m == step.flat_lora.numel() == step.m_lora.numel()
    o = n_ab
    for n in te.dora_modules():
        H = te._dora_of(n)
        k = H.mag.numel()
        assert H.mag.data_ptr() == step.flat_lora[o:].data_ptr() and H.grad_mag.data_ptr() == step.flat_grad[o:].data_ptr(), n
        o += k
    assert te.grad_added.data_ptr() == step.flat_grad[o:].data_ptr()
    assert te.mag.abs().min() > 0                              # the masters moved into the flat buffer with their values


def test_two_steps_fp16_dora_six_modules_match_oracle():
    """two optimizer steps, fp16 with the grad scaler, r = 4, six modules: the bounds of
    tests/test_gpu_lora_targets.py::test_two_steps_fp16_mixing_six_modules_match_oracle_elementwise on every adapter set -- gradients 4e-3 / 6e-3
    (dm like dB), updated A, B and m within 1.5e-4 (~2 lr), the added rows within 2.5e-3 and 2e-3 rel"""
    B, hw, D = 2, 16, 64
    st_ref, step, added = build_step(4, SIX, B, hw, D)
    from test_gpu_lora_targets import _draw
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
        clip = min(1.0, 1.0 / (out["lora_grad_norm"] + 1e-6))
        assert abs(sc["grad_norm"] - out["lora_grad_norm"]) < 5e-2 * out["lora_grad_norm"]
        gA, gB, gx, gm = DR.split_step_grads(out["g_lora"], te_ref)
        want = {"qkv": (gA, gB, gm["qkv"]), **{n: (gx[n][0], gx[n][1], gm[n]) for n in gx}}
        ref = _masters(te_ref)
        for n, (A_, B_, m_, gA_, gB_, gm_) in _hip_sets(step.te).items():
            parity(f"dora step {it} grad {n} lora_A", gA_ * inv * clip, want[n][0], rel=4e-3, maxabs=6e-3)
            parity(f"dora step {it} grad {n} lora_B", gB_ * inv * clip, want[n][1], rel=4e-3, maxabs=6e-3)
            parity(f"dora step {it} grad {n} magnitude", gm_ * inv * clip, want[n][2], rel=4e-3, maxabs=6e-3)
            for what, mine, theirs in (("A", A_, ref[n][0]), ("B", B_, ref[n][1]), ("m", m_, ref[n][2])):
                d = (mine.cpu() - theirs).abs().max().item()
                print(f"[dora] step {it} updated {n} {what}: max |delta| {d:.3e}")
                assert d < 1.5e-4, (n, what)
        parity(f"dora step {it} grad added rows", step.te.grad_added * inv, out["g_emb_added"], rel=4e-3, maxabs=6e-3)
        w, wr = step.te.token_table.cpu(), te_ref.token_embedding.weight.detach()
        torch.testing.assert_close(w[:49408], wr[:49408], rtol=1e-6, atol=1e-7)
        assert (w[added] - wr[added]).abs().max().item() < 2.5e-3
        assert rel_err(w[added], wr[added]) < 2e-3
    assert step.scalars()["opt_steps"] == 2.0


def test_two_steps_f32_dora_six_modules_match_oracle():
    """the no-AMP mode at the bounds of tests/test_gpu_lora_targets.py::test_two_steps_f32_six_modules_match_oracle: gradients 1e-4, updated A, B
    and m within 2e-5 (< lr / 2), the updated added rows 2e-4 / 5e-4"""
    B, hw, D = 2, 16, 64
    st_ref, step, added = build_step(4, SIX, B, hw, D, use_scaler=False, mode="fp32")
    from test_gpu_lora_targets import _draw
    assert step.te.dora_c.dtype == torch.float32 and step.te.op_dtype == torch.float32
    g = torch.Generator().manual_seed(5)
    te_ref = st_ref.te
    for it in range(2):
        x0, noise, t, ids, pids = _draw(step, added, g, B, hw)
        before = {n: s_[2].clone() for n, s_ in _hip_sets(step.te).items()}
        out = st_ref.step(x0, noise, t, ids, pids)
        step.step_eager()
        sc = step.scalars()
        assert sc["found_inf"] == 0.0 and sc["loss_scale"] == 1.0
        assert abs(sc["loss_mse"] - out["mse"]) < 1e-5 * abs(out["mse"]) + 1e-7, (sc, out["mse"])
        assert abs(sc["loss_kpl"] - out["kpl"]) < 1e-4 * abs(out["kpl"]) + 1e-7, (sc, out["kpl"])
        clip = min(1.0, 1.0 / (out["lora_grad_norm"] + 1e-6))
        assert abs(sc["grad_norm"] - out["lora_grad_norm"]) < 1e-4 * out["lora_grad_norm"]
        gA, gB, gx, gm = DR.split_step_grads(out["g_lora"], te_ref)
        want = {"qkv": (gA, gB, gm["qkv"]), **{n: (gx[n][0], gx[n][1], gm[n]) for n in gx}}
        ref = _masters(te_ref)
        for n, (A_, B_, m_, gA_, gB_, gm_) in _hip_sets(step.te).items():
            parity(f"dora fp32 step {it} grad {n} lora_A", gA_ * clip, want[n][0], rel=1e-4, maxabs=1e-4)
            parity(f"dora fp32 step {it} grad {n} lora_B", gB_ * clip, want[n][1], rel=1e-4, maxabs=1e-4)
            parity(f"dora fp32 step {it} grad {n} magnitude", gm_ * clip, want[n][2], rel=1e-4, maxabs=1e-4)
            for what, mine, theirs in (("A", A_, ref[n][0]), ("B", B_, ref[n][1]), ("m", m_, ref[n][2])):
                d = (mine.cpu() - theirs).abs().max().item()
                print(f"[dora] fp32 step {it} updated {n} {what}: max |delta| {d:.3e}")
                assert d < 2e-5, (n, what)
            assert not torch.equal(m_, before[n]), n
        parity(f"dora fp32 step {it} grad added rows", step.te.grad_added, out["g_emb_added"], rel=1e-4, maxabs=1e-4)
        w, wr = step.te.token_table.cpu(), te_ref.token_embedding.weight.detach()
        torch.testing.assert_close(w[:49408], wr[:49408], rtol=1e-6, atol=1e-7)
        parity(f"dora fp32 step {it} updated added rows", w[added], wr[added], rel=2e-4, maxabs=5e-4)
    assert step.scalars()["opt_steps"] == 2.0


def _params(step):
    return [step.flat_lora.clone(), step.te.token_table[49408:].clone(), step.state.clone(), step.m_lora.clone(), step.v_lora.clone()]


def test_graph_replay_equals_eager_and_resume_is_bit_identical(tmp_path):
    """four steps eagerly == two warm-up steps + two replays of the captured step, bit for bit (nothing on the DoRA path allocates or
    synchronises); and two steps, save_trainer_state, a fresh trainer, load_trainer_state, two more steps == the four uninterrupted ones: the
    checkpoint carries the magnitudes and their moments"""
    from safetensors.torch import load_file
    from test_gpu_lora_targets import _draw
    from textboost_amd import checkpoint as ckpt
    B, hw, D = 2, 16, 64
    outs = []
    for mode in ("eager", "graph", "resume"):
        st_ref, step, added = build_step(4, SIX, B, hw, D)
        _draw(step, added, torch.Generator().manual_seed(6), B, hw)
        if mode == "graph":
            step.capture(warmup=2)
            step.replay(); step.replay()
        elif mode == "eager":
            for _ in range(4):
                step.step_eager()
        else:
            for _ in range(2):
                step.step_eager()
            ckpt.save_trainer_state(step, str(tmp_path / "checkpoint-2"))
            model = load_file(str(tmp_path / "checkpoint-2" / "model.safetensors"))
            assert torch.equal(model[DR.mkey(1, "fc1")], step.te.extra["fc1"].mag[1].cpu()) and torch.equal(model[DR.mkey(0, "v_proj")], step.te.mag[0, 2 * D:].cpu())
            assert torch.load(str(tmp_path / "checkpoint-2" / "optimizer.bin"))["m_lora"].numel() == step.n_lora
            _, step, _ = build_step(4, SIX, B, hw, D)
            _draw(step, added, torch.Generator().manual_seed(6), B, hw)
            for n in step.te.dora_modules():
                step.te._dora_of(n).mag.fill_(9.0)             # (whatever the fresh trainer holds is overwritten)
            ckpt.load_trainer_state(step, str(tmp_path / "checkpoint-2"))
            for _ in range(2):
                step.step_eager()
        torch.cuda.synchronize()
        outs.append(_params(step))
    assert outs[0][0].numel() == step.n_lora
    for a, b, c in zip(*outs):
        torch.testing.assert_close(a, b, rtol=0, atol=0)
        torch.testing.assert_close(a, c, rtol=0, atol=0)


# ------------------------------------------------------------------------------------------------ 5. the CLI, the reader, inference.py
def test_cli_trains_checkpoints_resumes_and_generates(tmp_path, monkeypatch):
    """train_textboost.py --use_dora --lora_target_modules <six> --checkpointing_steps 1 on the tiny diffusers directory of
    tests/test_gpu_generate.py, data from latents.pt / input_ids.pt / prior_input_ids.pt (indexed by the step, so that a resumed run sees the batches
    the uninterrupted one saw): the adapter directory and the checkpoint hold the specified layout; a run resumed from checkpoint-1 ends with the
    bits of the uninterrupted run; generate.read_run_dir + load_text_encoder build a DoRA encoder from the output directory, and inference.py
    writes an image from it."""
    pytest.importorskip("transformers")
    from PIL import Image
    from safetensors.torch import load_file
    sys.path.insert(0, ROOT)
    import inference
    import train_textboost as T
    from tests.test_gpu_generate import write_model_dir
    from textboost_amd import generate as G
    mdir = str(tmp_path / "model")
    write_model_dir(mdir)
    data = tmp_path / "data"
    data.mkdir()
    g = torch.Generator().manual_seed(0)
    torch.save(torch.randn(4, 4, 16, 16, generator=g), str(data / "latents.pt"))
    ids = torch.randint(1000, 40000, (4, 77), generator=g)
    ids[:, 0], ids[:, 3], ids[:, 12:] = 49406, 49408, 49407
    torch.save(ids, str(data / "input_ids.pt"))
    pid = torch.randint(1000, 40000, (1, 77), generator=g)
    pid[:, 0], pid[:, 20:] = 49406, 49407
    torch.save(pid, str(data / "prior_input_ids.pt"))
    monkeypatch.chdir(tmp_path)

    def train(out, *extra):
        T.main(T.parse_args(["--pretrained_model_name_or_path", mdir, "--instance_data_dir", str(data), "--output_dir", out, "--train_batch_size", "2",
                             "--resolution", "128", "--placeholder_token", "<dog>", "--initializer_token", "a", "--lora_rank", "4",
                             "--mixed_precision", "fp16", "--seed", "5", "--use_dora", "--lora_target_modules", *SIX, "--checkpointing_steps", "1", *extra]))
        return load_file(os.path.join(out, "text_encoder", "adapter_model.safetensors")), torch.load(os.path.join(out, "dog.bin"))["<dog>"]

    full, part = str(tmp_path / "full"), str(tmp_path / "part")
    sd, tok = train(full, "--max_train_steps", "2")
    cfg = json.load(open(os.path.join(full, "text_encoder", "adapter_config.json")))
    assert cfg["use_dora"] is True and cfg["r"] == cfg["lora_alpha"] == 4 and cfg["target_modules"] == list(SIX)
    assert set(sd) == {LT.key(i, n, w) for i in range(2) for n in SIX for w in "AB"} | {DR.mkey(i, n) for i in range(2) for n in SIX}
    assert sd[DR.mkey(1, "fc1")].shape == (128,) and sd[DR.mkey(0, "fc2")].shape == (64,) and sd[DR.mkey(0, "k_proj")].dtype == torch.float32
    ck = os.path.join(full, "checkpoint-1")
    assert json.load(open(os.path.join(ck, "text_encoder", "adapter_config.json")))["use_dora"] is True
    ck_sd = load_file(os.path.join(ck, "text_encoder", "adapter_model.safetensors"))
    assert set(ck_sd) == set(sd) and set(sd) < set(load_file(os.path.join(ck, "model.safetensors")))
    for n in SIX:                                              # every magnitude moved away from its checkpoint-1 value: it trains
        assert any(not torch.equal(sd[DR.mkey(i, n)], ck_sd[DR.mkey(i, n)]) for i in range(2)), n
    train(part, "--max_train_steps", "1")
    sd2, tok2 = train(part, "--max_train_steps", "2", "--resume_from_checkpoint", "latest")
    assert all(torch.equal(sd[k], sd2[k]) for k in sd) and torch.equal(tok, tok2)
    # ---- the reader and generation
    run = G.read_run_dir(full)
    assert run.use_dora and run.rank == 4 and G.lora_targets_of(run.lora) == SIX
    with torch.no_grad():
        loaded, tk = G.load_text_encoder(mdir, run, 2, dev)
    assert loaded.use_dora and tuple(loaded.extra) == SIX[3:] and tk.convert_tokens_to_ids(["<dog>"]) == [49408]
    assert torch.equal(loaded.extra["fc2"].mag[1].cpu(), sd[DR.mkey(1, "fc2")]) and torch.equal(loaded.mag[0, 64:128].cpu(), sd[DR.mkey(0, "k_proj")])
    img = str(tmp_path / "dog.jpg")
    inference.main([full, "--model", mdir, "--prompt", "photo of a <dog> dog", "--seeds", "0", "--steps", "2", "--output", img])
    assert Image.open(img).size == (128, 128)
    with pytest.raises(SystemExit, match="use_dora"):
        inference.main([full, "--model", mdir, "--prompt", "a <dog> dog", "--weights", "0.5", "--output", img])
