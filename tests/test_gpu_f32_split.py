"""Split mode of the fp32 contractions (tb_f32_set_mode(1); the trainer's --allow_tf32) on the GPU: csrc/f32_path.hip's second kernel body.

Layout is checked bit for bit (small-integer operands make every product and partial sum exact in both modes), accuracy against float64
with the derived elementwise bound  |C - C64| <= (2^-16 + (3K + 8) 2^-24) S |alpha|,  S = sum_k |a_k||w_k|  (f32_split_ref.product_bound),
and everything that has no closed bound against 4 x the error of the CPU emulation (tests/f32_split_ref.py) on the same inputs.  Every test
leaves the process in mode 0 (the `exact_after` fixture)."""
import copy
import json
import os
import sys

import pytest
import torch
import torch.nn.functional as F

import f32_split_ref as R
from parity import parity

pytestmark = pytest.mark.gpu
dev = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TB_EINVAL = -22


def _ops():
    from textboost_amd import ops
    return ops


def _L():
    from textboost_amd import _lib as L
    return L


@pytest.fixture(autouse=True)
def exact_after():
    """whatever a test does, the next one (and the rest of the suite) starts in mode 0"""
    yield
    L = _L()
    L.set_f32_mode(0)
    assert L.lib().tb_f32_get_mode() == 0


def test_setter_default_return_value_and_invalid_mode():
    L = _L()
    lib = L.lib()
    assert lib.tb_f32_get_mode() == 0
    assert lib.tb_f32_set_mode(1) == 0 and lib.tb_f32_get_mode() == 1
    assert lib.tb_f32_set_mode(7) == TB_EINVAL and lib.tb_f32_get_mode() == 1
    assert lib.tb_f32_set_mode(-1) == TB_EINVAL and lib.tb_f32_get_mode() == 1
    assert lib.tb_f32_set_mode(0) == 1 and lib.tb_f32_get_mode() == 0


def test_mode_reaches_both_builds_of_the_library_and_is_restored_by_the_context_manager():
    ops, L = _ops(), _L()
    L.lib()
    with L.use_half("bf16" if L.half_kind() == "fp16" else "fp16"):
        L.lib()                                    # both builds loaded
    assert len(L._libs) == 2
    with ops.f32_mode(1):
        assert [h.tb_f32_get_mode() for h in L._libs.values()] == [1, 1] and L.get_f32_mode() == 1
        with ops.f32_mode(0):
            assert [h.tb_f32_get_mode() for h in L._libs.values()] == [0, 0]
        assert [h.tb_f32_get_mode() for h in L._libs.values()] == [1, 1]
    assert [h.tb_f32_get_mode() for h in L._libs.values()] == [0, 0] and L.get_f32_mode() == 0


# ------------------------------------------------------------------------------------------------ the launches of the layout / accuracy cases
def _nhwc(x):
    B, C, H, W = x.shape
    return x.permute(0, 2, 3, 1).reshape(B * H * W, C).contiguous()


def _draw(shape, g, ints):
    return torch.randint(-8, 9, shape, generator=g).float() if ints else torch.randn(shape, generator=g)


def _linear(M, N, K):
    def make(g, ints):
        return _draw((M, K), g, ints), _draw((N, K), g, ints)

    def run(A, W):
        return _ops().gemm(A.to(dev), W.to(dev), torch.empty(M, N, device=dev))

    return make, run, lambda A, W: A @ W.t(), K


def _kext(M, N, K1, K2):
    def make(g, ints):
        return tuple(_draw(s, g, ints) for s in ((M, K1), (M, K2), (N, K1), (N, K2)))

    def run(A, A2, W, W2):
        return _ops().gemm(A.to(dev), W.to(dev), torch.empty(M, N, device=dev), A2=A2.to(dev), W2=W2.to(dev))

    return make, run, lambda A, A2, W, W2: A @ W.t() + A2 @ W2.t(), K1 + K2


def _trans(M, N, K, a_trans, w_trans):
    def make(g, ints):
        return _draw((K, M) if a_trans else (M, K), g, ints), _draw((K, N) if w_trans else (N, K), g, ints)

    def run(A, W):
        return _ops().gemm_f32_t(A.to(dev), W.to(dev), torch.empty(M, N, device=dev), M, N, K, a_trans=a_trans, w_trans=w_trans)

    return make, run, lambda A, W: (A.t() if a_trans else A) @ (W if w_trans else W.t()), K


def _conv(kind, H):
    """3x3 convolutions of a [1, 4, H, H] image with 8 output channels through every gather of load_a.  The dgrad kinds gather the 8-channel
    output gradient and produce the 4-channel input gradient."""
    Ci, Co, B = 4, 8, 1
    stride = 2 if kind in ("s2", "tr") else 1
    Ho = (H + 2 - 3) // stride + 1

    def make(g, ints):
        x, w = _draw((B, Ci, H, H), g, ints), _draw((Co, Ci, 3, 3), g, ints)
        if kind in ("dgrad", "tr"):
            return _draw((B, Co, Ho, Ho), g, ints), w
        return x, w

    def run(x, w):
        ops = _ops()
        wf = w.permute(0, 2, 3, 1).reshape(Co, 9 * Ci).contiguous().to(dev)
        wd = w.permute(1, 2, 3, 0).reshape(Ci, 9 * Co).contiguous().to(dev)
        a = _nhwc(x).to(dev)
        if kind == "s1":
            return ops.gemm(a, wf, torch.empty(B * H * H, Co, device=dev),
                            conv=dict(B=B, Hin=H, Win=H, Cin=Ci, Hout=H, Wout=H, stride=1, sign=1, upsample=0, transposed=0))
        if kind == "s2":
            return ops.gemm(a, wf, torch.empty(B * Ho * Ho, Co, device=dev),
                            conv=dict(B=B, Hin=H, Win=H, Cin=Ci, Hout=Ho, Wout=Ho, stride=2, sign=1, upsample=0, transposed=0))
        if kind == "up":
            return ops.gemm(a, wf, torch.empty(B * 4 * H * H, Co, device=dev),
                            conv=dict(B=B, Hin=H, Win=H, Cin=Ci, Hout=2 * H, Wout=2 * H, stride=1, sign=1, upsample=1, transposed=0))
        if kind == "dgrad":
            return ops.gemm(a, wd, torch.empty(B * H * H, Ci, device=dev),
                            conv=dict(B=B, Hin=H, Win=H, Cin=Co, Hout=H, Wout=H, stride=1, sign=-1, upsample=0, transposed=0))
        return ops.gemm(a, wd, torch.empty(B * H * H, Ci, device=dev),
                        conv=dict(B=B, Hin=Ho, Win=Ho, Cin=Co, Hout=H, Wout=H, stride=2, sign=1, upsample=0, transposed=1))

    def ref(x, w):   # linear in both arguments: called with (x, w) for C64 and with (|x|, |w|) for S
        if kind == "s1":
            return _nhwc(F.conv2d(x, w, padding=1))
        if kind == "s2":
            return _nhwc(F.conv2d(x, w, padding=1, stride=2))
        if kind == "up":
            return _nhwc(F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, padding=1))
        return _nhwc(F.conv_transpose2d(x, w, padding=1, stride=stride, output_padding=H + 2 - 3 - (Ho - 1) * stride))

    return make, run, ref, 9 * (Co if kind in ("dgrad", "tr") else Ci)


CASES = {
    "linear": _linear(65, 33, 20),
    "k_extension": _kext(33, 9, 16, 4),
    "a_trans": _trans(33, 9, 70, True, False),
    "w_trans": _trans(33, 9, 70, False, True),
    "both_trans": _trans(33, 9, 70, True, True),
    "conv_5x5": _conv("s1", 5),
    "conv_6x6_stride2": _conv("s2", 6),
    "conv_5x5_upsample": _conv("up", 5),
    "conv_5x5_transposed_dgrad": _conv("tr", 5),
    "conv_5x5_sign_minus": _conv("dgrad", 5),
}


@pytest.mark.parametrize("name", list(CASES))
def test_layout_bit_for_bit_on_small_integers(name):
    """operands are integers in [-8, 8]: every product and partial sum is exact in both modes, so any difference is a misplaced element"""
    make, run, ref, K = CASES[name]
    ops = _ops()
    inp = make(torch.Generator().manual_seed(7), True)
    exact = run(*inp).cpu()
    with ops.f32_mode(1):
        got = run(*inp).cpu()
    assert torch.equal(exact, ref(*[t.double() for t in inp]).float())   # (the case itself is set up right)
    assert torch.equal(got, exact), (name, (got - exact).abs().max().item())


def test_layout_of_the_batched_launch_bit_for_bit_through_attention():
    """the only exported way into a batched launch (grid.z = B * H, bdiv = H) is attention: with small-integer Q / K and a power-of-two scale
    the score matrix is exact in both modes, so softmax sees the same bits and LSE (all of it) must agree bit for bit"""
    ops = _ops()
    B, H, Sq, Skv, hd = 2, 2, 33, 7, 16
    g = torch.Generator().manual_seed(8)
    q = torch.randint(-2, 3, (B * Sq, H * hd), generator=g).float().to(dev)
    k = torch.randint(-2, 3, (B * Skv, H * hd), generator=g).float().to(dev)
    v = torch.randn(B * Skv, H * hd, generator=g).to(dev)
    outs = []
    for mode in (0, 1):
        o, lse = torch.empty(B * Sq, H * hd, device=dev), torch.empty(B, H, Sq, device=dev)
        with ops.f32_mode(mode):
            ops.attention_fwd(q, k, v, o, lse, B, H, Sq, Skv, hd)
        outs.append((o.cpu(), lse.cpu()))
    assert torch.equal(outs[0][1], outs[1][1])
    assert not torch.equal(outs[0][0], outs[1][0])   # P V has random operands: mode 1 was live


@pytest.mark.parametrize("name", list(CASES))
def test_accuracy_inside_the_derived_bound(name):
    make, run, ref, K = CASES[name]
    ops = _ops()
    inp = make(torch.Generator().manual_seed(9), False)
    exact = run(*inp).cpu()
    with ops.f32_mode(1):
        got = run(*inp).cpu()
    C64 = ref(*[t.double() for t in inp])
    S = ref(*[t.double().abs() for t in inp])
    bound = R.product_bound(K, S)
    err = (got.double() - C64).abs()
    print(f"[split {name}] max error / S {(err / S.clamp_min(1e-300)).max().item():.2e}  bound / S {R.product_bound(K, 1.0):.2e}")
    assert bool((err <= bound).all()), (name, (err / S.clamp_min(1e-300)).max().item())
    assert not torch.equal(got, exact), "mode 1 gave mode 0's bits: the mode is not live"


# ------------------------------------------------------------------------------------------------ epilogues
def _gelu_grad(z):
    z = z.detach().clone().requires_grad_(True)
    F.gelu(z).sum().backward()
    return z.grad


def _epilogue_cases():
    from textboost_amd.unet import pack_geglu_rows
    L = _L()
    M, N, K = 65, 64, 20
    g = torch.Generator().manual_seed(10)
    A, W = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g)
    bias, Rr = torch.randn(N, generator=g), torch.randn(M, N, generator=g)
    pre = torch.randn(M, 2 * N, generator=g)       # packed pre-gate projections [h | g] per 32 columns for GEGLU_GRAD

    def prod(dt):   # the product as the mode under test evaluates it (float64: the reference; float32: the emulation)
        return A.double() @ W.double().t() if dt == torch.float64 else R.split_matmul(A, W.t())

    def plain(dt):
        return 0.5 * prod(dt) + bias.to(dt) + Rr.to(dt)

    def geglu(dt):     # W rows [h (32) | g (32)] -> h * gelu(g)
        z = prod(dt) + bias.to(dt)
        return z[:, :32] * F.gelu(z[:, 32:])

    def geglu_grad(dt):
        v, p = prod(dt), pre.to(dt)
        out = torch.empty(M, 2 * N, dtype=dt)
        for blk in range(N // 32):
            h, gt = p[:, 64 * blk:64 * blk + 32], p[:, 64 * blk + 32:64 * blk + 64]
            vb = v[:, 32 * blk:32 * blk + 32]
            out[:, 64 * blk:64 * blk + 32] = vb * F.gelu(gt)
            out[:, 64 * blk + 32:64 * blk + 64] = vb * h * _gelu_grad(gt)
        return out

    a, w, b, r = A.to(dev), W.to(dev), bias.to(dev), Rr.to(dev)
    wp, bp = pack_geglu_rows(W).to(dev), pack_geglu_rows(bias).to(dev)
    assert torch.equal(wp.cpu(), W)   # one 64-row block: the packing is the identity here

    def out(n=N):
        return torch.empty(M, n, device=dev)

    ops = _ops()
    return {
        "bias_residual_alpha": (lambda: ops.gemm(a, w, out(), bias=b, R=r, alpha=0.5), plain),
        "gelu": (lambda: ops.gemm(a, w, out(), bias=b, act=L.ACT_GELU, C2=out()), lambda dt: F.gelu(prod(dt) + bias.to(dt))),
        "silu": (lambda: ops.gemm(a, w, out(), bias=b, act=L.ACT_SILU), lambda dt: F.silu(prod(dt) + bias.to(dt))),
        "quick_gelu": (lambda: ops.gemm(a, w, out(), bias=b, act=L.ACT_QUICK_GELU, C2=out()),
                       lambda dt: (lambda z: z * torch.sigmoid(1.702 * z))(prod(dt) + bias.to(dt))),
        "geglu": (lambda: ops.gemm(a, wp, out(32), bias=bp, act=L.ACT_GEGLU, C2=out()), geglu),
        "geglu_grad": (lambda: ops.gemm(a, w, out(2 * N), act=L.ACT_GEGLU_GRAD, C2=pre.to(dev)), geglu_grad),
    }


@pytest.mark.parametrize("name", ["bias_residual_alpha", "gelu", "silu", "quick_gelu", "geglu", "geglu_grad"])
def test_epilogues_within_four_times_the_emulation_error(name):
    """N = 64, M = 65, K = 20 against float64 torch: rel-L2 <= 4 x the CPU emulation's rel-L2 on the same inputs (4: tile summation order
    differs from the CPU's; the representation error, which dominates, does not depend on order)"""
    run, formula = _epilogue_cases()[name]
    with _ops().f32_mode(1):
        got = run().cpu()
    ref = formula(torch.float64)
    emu, gpu = R.rel_l2(formula(torch.float32), ref), R.rel_l2(got, ref)
    print(f"[split epilogue {name}] rel-L2 GPU {gpu:.3e}  emulation {emu:.3e}  ratio {gpu / emu:.2f}")
    assert emu > 0 and gpu <= 4 * emu, (name, gpu, emu)


# ------------------------------------------------------------------------------------------------ attention
def _attention_formulae(q, k, v, do, scale, mm):
    """tb_attention_f32_fwd / _bwd's formulae on [B, H, S, hd] tensors with `mm` as the product"""
    s = mm(q, k.transpose(-1, -2)) * scale
    lse = torch.logsumexp(s, -1)
    p = torch.exp(s - lse[..., None])
    o = mm(p, v)
    delta = (o * do).sum(-1, keepdim=True)
    dv = mm(p.transpose(-1, -2), do)
    ds = p * (mm(do, v.transpose(-1, -2)) - delta)
    return {"O": o, "LSE": lse, "dQ": mm(ds, k) * scale, "dK": mm(ds.transpose(-1, -2), q) * scale, "dV": dv}


@pytest.mark.parametrize("B,H,Sq,Skv,hd", [(1, 2, 33, 7, 8), (2, 2, 64, 77, 40)])
def test_attention_within_four_times_the_emulation_error(B, H, Sq, Skv, hd):
    ops = _ops()
    g = torch.Generator().manual_seed(11)
    C = H * hd
    q, k, v, do = (torch.randn(B * S, C, generator=g) for S in (Sq, Skv, Skv, Sq))
    heads = lambda t: t.reshape(B, -1, H, hd).transpose(1, 2)    # noqa: E731
    ref = _attention_formulae(*[heads(t).double() for t in (q, k, v, do)], hd ** -0.5, torch.matmul)
    emu = _attention_formulae(*[heads(t) for t in (q, k, v, do)], hd ** -0.5, R.split_matmul)
    qd, kd, vd = q.to(dev), k.to(dev), v.to(dev)
    o, lse, delta = torch.empty(B * Sq, C, device=dev), torch.empty(B, H, Sq, device=dev), torch.empty(B, H, Sq, device=dev)
    dq, dk, dv = torch.empty(B * Sq, C, device=dev), torch.empty(B * Skv, C, device=dev), torch.empty(B * Skv, C, device=dev)
    with ops.f32_mode(1):
        ops.attention_fwd(qd, kd, vd, o, lse, B, H, Sq, Skv, hd)
        ops.attention_bwd(qd, kd, vd, o, lse, do.to(dev), delta, dq, dk, dv, B, H, Sq, Skv, hd)
    got = {"O": o, "LSE": lse, "dQ": dq, "dK": dk, "dV": dv}
    for name in ("O", "LSE", "dQ", "dK", "dV"):
        r64 = ref[name] if name == "LSE" else ref[name].transpose(1, 2).reshape(-1, C)
        e32 = emu[name] if name == "LSE" else emu[name].transpose(1, 2).reshape(-1, C)
        er, em, _ = R.measures(e32, r64)
        # 4 x the emulation's error; where that error is below the bound tests/test_gpu_f32.py holds the quantity to (1e-5 / 5e-5), that bound
        rel, mab = (4 * er if er >= 1e-5 else 1e-5), (4 * em if em >= 5e-5 else 5e-5)
        print(f"[split attention {name}] emulation rel-L2 {er:.3e} max-abs {em:.3e}")
        parity(f"split attention {name}", got[name], r64, rel=rel, maxabs=mab)


# ------------------------------------------------------------------------------------------------ non-finite inputs, determinism
def test_one_infinite_input_poisons_its_row_and_nothing_else():
    ops = _ops()
    M, N, K = 65, 33, 20
    g = torch.Generator().manual_seed(12)
    A, W = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g).to(dev)
    out = lambda: torch.empty(M, N, device=dev)   # noqa: E731
    with ops.f32_mode(1):
        clean = ops.gemm(A.to(dev), W, out()).cpu()
        A[3, 5] = float("inf")
        got = ops.gemm(A.to(dev), W, out()).cpu()
    assert not torch.isfinite(got[3]).any()
    rest = [i for i in range(M) if i != 3]
    assert torch.equal(got[rest], clean[rest])


def test_graph_replay_equals_the_eager_run_bit_for_bit_and_keeps_its_mode():
    ops = _ops()
    g = torch.Generator().manual_seed(13)
    A, W = torch.randn(130, 52, generator=g).to(dev), torch.randn(70, 52, generator=g).to(dev)
    x, w = CASES["conv_5x5"][0](g, False)
    with ops.f32_mode(1):
        eager, eager_c = ops.gemm(A, W, torch.empty(130, 70, device=dev)).clone(), CASES["conv_5x5"][1](x, w).clone()
        again = ops.gemm(A, W, torch.empty(130, 70, device=dev))
        assert torch.equal(eager, again)
        out = torch.zeros(130, 70, device=dev)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=s):
                ops.gemm(A, W, out)
        torch.cuda.current_stream().wait_stream(s)
    exact = ops.gemm(A, W, torch.empty(130, 70, device=dev)).clone()
    assert not torch.equal(exact, eager)
    graph.replay()          # replayed in mode 0: the graph keeps the mode it was captured under
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    with ops.f32_mode(1):
        assert torch.equal(CASES["conv_5x5"][1](x, w), eager_c)


# ------------------------------------------------------------------------------------------------ model level (small config of test_gpu_f32.py)
def _bounded(name, got, ref, emu, rel, maxabs, ch_dim=None, ch_rel=None):
    """parity against the fp32 oracle with, per figure, max(the bound tests/test_gpu_f32.py uses, 4 x the emulation's figure)"""
    yr, ym, yc = R.measures(emu, ref, ch_dim)
    print(f"[yardstick] {name}: emulation rel-L2 {yr:.3e} max-abs {ym:.3e}" + (f" worst-channel {yc:.3e}" if yc is not None else ""))
    return parity(name, got, ref, rel=max(rel, 4 * yr), maxabs=max(maxabs, 4 * ym), ch_dim=ch_dim,
                  ch_rel=None if ch_rel is None else max(ch_rel, 4 * yc))


def test_unet_prediction_and_d_ehs_in_split_mode_vs_oracle():
    from test_gpu_f32 import _small_unet_f32
    B, hw, D = 2, 16, 64
    ref, hip = _small_unet_f32(B, hw, D)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, 4, hw, hw, generator=g)
    t = torch.tensor([17, 801])
    ehs = torch.randn(B, 77, D, generator=g)
    dpred = torch.randn(B, 4, hw, hw, generator=g)
    pred_ref, dehs_ref = R.unet_pred_and_dehs(ref, x, t, ehs, dpred)
    with R.split_products():
        pred_emu, dehs_emu = R.unet_pred_and_dehs(ref, x, t, ehs, dpred)
    with _ops().f32_mode(1):
        pred = hip.forward(x.to(dev), t.to(dev), ehs.view(B * 77, D).to(dev).contiguous()).clone()
        d_ehs = hip.backward(dpred.to(dev)).clone()
    _bounded("split UNet pred", pred, pred_ref, pred_emu, 1e-4, 1e-4, ch_dim=1, ch_rel=1e-4)
    _bounded("split UNet d_ehs", d_ehs.view(B, 77, D), dehs_ref, dehs_emu, 1e-4, 1e-4, ch_dim=2, ch_rel=2e-4)


def _lora_grads(student):
    gA = torch.stack([torch.cat([l.q.lora_A.grad, l.k.lora_A.grad, l.v.lora_A.grad]) for l in student.layers])
    gB = torch.stack([torch.cat([l.q.lora_B.grad, l.k.lora_B.grad, l.v.lora_B.grad]) for l in student.layers])
    return gA.clone(), gB.clone()


def test_text_encoder_hidden_states_and_lora_gradients_in_split_mode_vs_oracle():
    from oracle import train_step as ts
    from test_gpu_f32 import _encoders_f32
    B, D = 3, 64
    student, teacher, hip, hip_teacher, added, null = _encoders_f32(B, D)
    g = torch.Generator().manual_seed(2)
    ids = ts.synthetic_ids(B, added, g)
    Rw = torch.randn(B, 77, D, generator=g)

    def oracle():
        for p in student.parameters():
            p.grad = None
        out = student(ids)
        (out * Rw).sum().backward()
        return (out.detach(), *_lora_grads(student))

    out_ref, gA_ref, gB_ref = oracle()
    with R.split_products():
        out_emu, gA_emu, gB_emu = oracle()
    with _ops().f32_mode(1):
        hip.pack_lora()
        out = hip.forward(ids.to(dev), slot=0)[:B * 77].clone()
        hip.zero_grad()
        hip.backward(Rw.view(B * 77, D).to(dev).contiguous(), slot=0)
        torch.cuda.synchronize()
    _bounded("split encoder hidden states", out.view(B, 77, D), out_ref, out_emu, 1e-5, 2e-5, ch_dim=2, ch_rel=1e-4)
    _bounded("split encoder grad lora_A", hip.grad_A, gA_ref, gA_emu, 1e-4, 1e-4, ch_dim=0, ch_rel=1e-4)
    _bounded("split encoder grad lora_B", hip.grad_B, gB_ref, gB_emu, 1e-4, 1e-4, ch_dim=0, ch_rel=1e-4)


def test_two_optimizer_steps_in_split_mode_vs_oracle():
    """two whole steps with the step built and run in mode 1: the updated LoRA tensors and added rows against the fp32 oracle.  Bounds: what
    tests/test_gpu_f32.py holds mode 0 to, or 4 x what the emulated oracle step differs by, whichever is larger."""
    from oracle import train_step as ts
    from test_gpu_f32 import _encoders_f32, _small_unet_f32
    from textboost_amd.trainer import StepHyper, TextBoostStep
    B, hw, D = 2, 16, 64
    ref_unet, hip_unet = _small_unet_f32(B, hw, D, seed=3)
    student, teacher, hip_te, hip_teacher, added, null = _encoders_f32(B, D, seed=4)
    st_ref = ts.TrainState(student, teacher, ref_unet, added, ts.StepConfig())
    st_emu = copy.deepcopy(st_ref)
    stack = lambda te, n: torch.stack([torch.cat([getattr(l.q, n), getattr(l.k, n), getattr(l.v, n)]) for l in te.layers]).detach()  # noqa: E731
    g = torch.Generator().manual_seed(5)
    with _ops().f32_mode(1):
        step = TextBoostStep(hip_unet, hip_te, hip_teacher, StepHyper(use_grad_scaler=False, init_scale=1.0), (B, 4, hw, hw), device=dev)
        step.external_noise = True
        for it in range(2):
            ids, pids = ts.synthetic_ids(B, added, g), ts.synthetic_ids(B, added, g, prior=True)
            x0, noise = torch.randn(B, 4, hw, hw, generator=g), torch.randn(B, 4, hw, hw, generator=g)
            t = torch.randint(0, 1000, (B,), generator=g)
            out = st_ref.step(x0, noise, t, ids, pids)
            with R.split_products():
                out_emu = st_emu.step(x0, noise, t, ids, pids)
            step.x0.copy_(x0); step.noise.copy_(noise); step.timesteps.copy_(t)
            step.input_ids.copy_(ids); step.prior_ids.copy_(pids)
            step.step_eager()
            sc = step.scalars()
            assert sc["found_inf"] == 0.0 and sc["loss_scale"] == 1.0
            y = abs(out_emu["mse"] - out["mse"]) / abs(out["mse"])
            print(f"[yardstick] step {it} mse: emulation relative difference {y:.3e}")
            assert abs(sc["loss_mse"] - out["mse"]) <= max(1e-5, 4 * y) * abs(out["mse"]) + 1e-7, (sc, out["mse"])
            _bounded(f"split step {it} grad added rows", step.te.grad_added, out["g_emb_added"], out_emu["g_emb_added"], 1e-4, 1e-4)
            w, wr, we = step.te.token_table.cpu(), st_ref.te.token_embedding.weight.detach(), st_emu.te.token_embedding.weight.detach()
            _bounded(f"split step {it} updated added rows", w[added], wr[added], we[added], 2e-4, 5e-4)
            for n, mine in (("lora_A", step.te.lora_A), ("lora_B", step.te.lora_B)):
                yard = (stack(st_emu.te, n) - stack(st_ref.te, n)).abs().max().item()
                diff = (mine.cpu() - stack(st_ref.te, n)).abs().max().item()
                print(f"[yardstick] step {it} updated {n}: emulation max-abs {yard:.3e}; GPU max-abs {diff:.3e}")
                assert diff <= max(2e-5, 4 * yard), (n, diff, yard)
    assert step.scalars()["opt_steps"] == 2.0


# ------------------------------------------------------------------------------------------------ CLI end to end on tiny models
def _tiny_model_dir(tmp_path):
    m = tmp_path / "sd-tiny"
    for sub in ("unet", "text_encoder"):
        (m / sub).mkdir(parents=True)
    json.dump({"attention_head_dim": [2, 2, 4, 4], "block_out_channels": [64, 128, 128, 128], "cross_attention_dim": 64,
               "down_block_types": ["CrossAttnDownBlock2D"] * 3 + ["DownBlock2D"], "up_block_types": ["UpBlock2D"] + ["CrossAttnUpBlock2D"] * 3,
               "in_channels": 4, "out_channels": 4, "layers_per_block": 2, "norm_num_groups": 32, "norm_eps": 1e-5, "act_fn": "silu"},
              open(m / "unet" / "config.json", "w"))
    json.dump({"hidden_act": "quick_gelu", "hidden_size": 64, "intermediate_size": 128, "num_attention_heads": 2, "num_hidden_layers": 2,
               "max_position_embeddings": 77, "vocab_size": 49408, "layer_norm_eps": 1e-5}, open(m / "text_encoder" / "config.json", "w"))
    return str(m)


def _files(out):
    got = {}
    for base, _, names in os.walk(out):
        for n in names:
            if n.endswith((".safetensors", ".bin", ".json")):
                got[os.path.relpath(os.path.join(base, n), out)] = open(os.path.join(base, n), "rb").read()
    return got


def test_cli_readme_command_with_and_without_allow_tf32(tmp_path):
    """the README command on a tiny model directory.  With --allow_tf32: trains in mode 1, says so in training.log, writes the reference
    layout, and a second run with the same seed writes identical files.  Without it: mode 0, and the files are byte for byte those of a
    run whose every launch is pinned to the exact kernel body (mode 0 set explicitly around it) -- and differ from the split run's."""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import train_textboost as T
    L = _L()
    mdir = _tiny_model_dir(tmp_path)

    def run(name, *extra):
        out = str(tmp_path / name)
        T.main(T.parse_args(["--pretrained_model_name_or_path", mdir, "--output_dir", out, "--train_batch_size", "2", "--resolution", "128",
                             "--max_train_steps", "4", "--checkpointing_steps", "4", "--placeholder_token", "<dog>", "--augment_inversion",
                             "--lora_rank", "4", "--learning_rate", "5e-5", "--emb_learning_rate", "1e-3", "--seed", "42", "--kpl_weight", "0.1",
                             *extra]))
        assert L.lib().tb_f32_get_mode() == 0        # restored after the subject
        return out, _files(out), open(os.path.join(out, "training.log")).read()

    out_a, split_a, log_a = run("split_a", "--allow_tf32")
    assert "f32 mode 1" in log_a and "precision fp32" in log_a and " scale 1 " in log_a
    assert {"dog.bin", os.path.join("text_encoder", "adapter_model.safetensors"), os.path.join("text_encoder", "adapter_config.json")} <= set(split_a)
    assert os.path.isdir(os.path.join(out_a, "checkpoint-4"))
    _, split_b, _ = run("split_b", "--allow_tf32")
    assert split_a.keys() == split_b.keys() and all(split_a[k] == split_b[k] for k in split_a)
    _, exact_a, log_e = run("exact_a")
    assert "f32 mode" not in log_e and "allow_tf32" not in log_e
    with _ops().f32_mode(0):
        _, exact_b, _ = run("exact_b")
    assert exact_a.keys() == exact_b.keys() and all(exact_a[k] == exact_b[k] for k in exact_a)
    key = os.path.join("text_encoder", "adapter_model.safetensors")
    assert exact_a[key] != split_a[key], "--allow_tf32 changed nothing"
    _, half, log_h = run("half", "--allow_tf32", "--mixed_precision", "fp16")
    assert "no effect under --mixed_precision fp16" in log_h
