"""The masked training loss on the GPU (--instance_mask_dir): the mask -> latent-weights kernel bit-exact against numpy,
the weighted MSE kernels of the three precision modes against float64, the augmentation replay (a mask never perturbs the image path), the
step against the oracle step with the weighted loss, and the command line on `loss_weight.pt`.

Measured on an MI355X (figures printed by the tests): see DESIGN.md section 16."""
import os
import random
import sys
import types

import numpy as np
import pytest
import torch

import masked_loss_ref as R
from parity import parity

pytestmark = pytest.mark.gpu
dev = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _mods():
    from textboost_amd import _lib as L
    from textboost_amd import augment as D
    from textboost_amd import ops
    return L, D, ops


# ------------------------------------------------------------------------------------------------------------------ 1. the pool kernel
def _mask(seed, h, w):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


@pytest.mark.parametrize("h,w,x0,y0,oh,ow", [(16, 24, 5, 0, 2, 2), (24, 16, 0, 7, 2, 2), (40, 33, 11, 17, 2, 2), (40, 33, 17, 24, 2, 2),
                                              (512, 512, 0, 0, 64, 64)])
@pytest.mark.parametrize("floor", [0.0, 0.25])
def test_pool_kernel_is_bit_exact_against_numpy(h, w, x0, y0, oh, ow, floor):
    L, D, ops = _mods()
    m = _mask(h * 1000 + w, h, w)
    img = D.to_device_mask(m)
    assert img.dtype == torch.int32 and tuple(img.shape) == (h, w)
    out = torch.full((1, oh, ow), -1.0, device=dev)
    ops.img_to_loss_weight(img, x0, y0, out, cell=8, floor=floor)
    want = R.pool_ref(m, x0, y0, oh, ow, 8, floor)
    assert np.array_equal(out[0].cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert float(out.min()) >= floor and float(out.max()) <= 1.0


def test_pool_kernel_other_cells_and_a_strided_view():
    """`cell` is an argument: 4 (16 cells per block row), 5 (12 cells and four idle lanes) and 64 (one); the source may be a strided view"""
    L, D, ops = _mods()
    m = _mask(7, 200, 330)
    img = D.to_device_mask(m)
    for cell, oh, ow, x0, y0 in ((4, 9, 37, 3, 2), (5, 7, 29, 1, 4), (64, 3, 5, 6, 5), (1, 6, 70, 9, 9)):
        out = torch.empty(1, oh, ow, device=dev)
        ops.img_to_loss_weight(img, x0, y0, out, cell=cell, floor=0.125)
        assert np.array_equal(out[0].cpu().numpy().view(np.uint32), R.pool_ref(m, x0, y0, oh, ow, cell, 0.125).view(np.uint32)), cell
    view = img[10:90, 20:140]
    out = torch.empty(1, 10, 15, device=dev)
    ops.img_to_loss_weight(view, 0, 0, out, cell=8, floor=0.0)
    assert np.array_equal(out[0].cpu().numpy().view(np.uint32), R.pool_ref(m[10:90, 20:140], 0, 0, 10, 15, 8, 0.0).view(np.uint32))


@pytest.mark.parametrize("x0,y0,oh,ow,cell,floor", [(9, 0, 2, 2, 8, 0.0), (0, 1, 2, 2, 8, 0.0), (-1, 0, 2, 2, 8, 0.0), (0, 0, 2, 4, 8, 0.0),
                                                     (0, 0, 2, 2, 0, 0.0), (0, 0, 1, 1, 65, 0.0), (0, 0, 2, 2, 8, 1.0), (0, 0, 2, 2, 8, -0.5)])
def test_pool_kernel_refuses_a_crop_that_leaves_the_image_and_bad_arguments(x0, y0, oh, ow, cell, floor):
    L, D, ops = _mods()
    img = D.to_device_mask(_mask(1, 16, 24))
    out = torch.zeros(1, oh, ow, device=dev)
    with pytest.raises(RuntimeError, match="-22"):
        ops.img_to_loss_weight(img, x0, y0, out, cell=cell, floor=floor)
    assert float(out.abs().max()) == 0.0    # nothing was launched


# ------------------------------------------------------------------------------------------------------------------ 2. the loss kernels
def _ordered(t):
    """fp32 bits as integers that are monotone in the value: differences count units in the last place"""
    i = t.contiguous().view(torch.int32).to(torch.int64)
    return torch.where(i < 0, -(i & 0x7FFFFFFF), i)


def _weights(kind, B, h, w, g):
    if kind == "uniform":
        return torch.rand(B, 1, h, w, generator=g)
    if kind == "ones":
        return torch.ones(B, 1, h, w)
    if kind == "one_sample_zero":
        wt = torch.rand(B, 1, h, w, generator=g)
        wt[B // 2] = 0
        return wt
    wt = torch.zeros(B, 1, h, w)            # "single_pixel": W_b = 0.75 < 1 for that sample, 0 for the others: the max(W_b, 1) branch
    wt[B - 1, 0, h // 2, w - 1] = 0.75
    return wt


@pytest.mark.parametrize("shape", [(1, 4, 8, 8), (3, 4, 5, 7), (8, 4, 64, 64)])
@pytest.mark.parametrize("mode", ["fp16", "bf16", "f32"])
def test_weighted_mse_kernels_against_float64(mode, shape):
    """loss within N * 2^-23 relative (the worst case of a sequential fp32 accumulation of N = B C h w products); dpred elementwise within
    8 * 2^-24 relative (its fp32 roundings: pred - target, w * d, the coefficient, their product -- four half-ulps, doubled) and exactly zero
    where w = 0; bit-identical on a second launch; with all-ones weights within 4 ulp of ops.mse_loss's dpred."""
    L, D, ops = _mods()
    B, C, h, w = shape
    N = B * C * h * w
    g = torch.Generator().manual_seed(N)
    pdt = torch.float32 if mode == "f32" else (torch.bfloat16 if mode == "bf16" else torch.float16)
    pred_h = torch.randn(B, C, h, w, generator=g).to(pdt)
    target_h = torch.randn(B, C, h, w, generator=g)
    worst_loss, worst_grad = 0.0, 0.0
    with L.use_half(None if mode == "f32" else mode):
        pred, target = pred_h.to(dev), target_h.to(dev)
        for kind in ("uniform", "ones", "one_sample_zero", "single_pixel"):
            wt_h = _weights(kind, B, h, w, g)
            wt = wt_h.to(dev)
            for scale in (1.0, 65536.0):
                ls = torch.tensor([scale], device=dev)
                dpred, loss = torch.full((B, C, h, w), float("nan"), device=dev), torch.zeros(1, device=dev)
                ops.mse_loss_weighted(pred, target, wt, dpred, loss, ls)
                dpred2, loss2 = torch.full_like(dpred, float("nan")), torch.zeros(1, device=dev)
                ops.mse_loss_weighted(pred, target, wt, dpred2, loss2, ls)
                assert torch.equal(dpred.view(torch.int32), dpred2.view(torch.int32)) and torch.equal(loss, loss2), (kind, scale)
                ref_loss = R.weighted_mse(pred_h, target_h, wt_h).item()
                ref_grad = R.weighted_mse_grad(pred_h, target_h, wt_h, scale)
                if ref_loss == 0.0:     # (B = 1 with its only sample all zero)
                    assert loss.item() == 0.0 and float(dpred.abs().max()) == 0.0
                    continue
                e_loss = abs(loss.item() - ref_loss) / abs(ref_loss)
                err = (dpred.double().cpu() - ref_grad).abs()
                nz = ref_grad != 0
                e_grad = (err[nz] / ref_grad[nz].abs()).max().item()
                worst_loss, worst_grad = max(worst_loss, e_loss), max(worst_grad, e_grad)
                assert e_loss <= N * 2.0 ** -23, (kind, scale, e_loss)
                assert e_grad <= 8 * 2.0 ** -24, (kind, scale, e_grad)
                zero = (wt_h == 0).expand(B, C, h, w)
                assert (dpred.cpu()[zero] == 0).all() and torch.isfinite(dpred).all() and bool(torch.isfinite(loss))
                if kind == "ones":
                    plain, ploss = torch.empty_like(dpred), torch.zeros(1, device=dev)
                    ops.mse_loss(pred, target, plain, ploss, ls)
                    ulps = (_ordered(dpred) - _ordered(plain)).abs().max().item()
                    assert ulps <= 4, (scale, ulps)
                    assert abs(loss.item() - ploss.item()) <= N * 2.0 ** -23 * abs(ploss.item())
    print(f"[masked loss] {mode} {shape}: loss rel err {worst_loss:.3e} (bound {N * 2.0 ** -23:.3e}), dpred rel err {worst_grad:.3e} "
          f"(bound {8 * 2.0 ** -24:.3e})")


def test_weighted_mse_refuses_a_short_workspace_and_bad_shapes():
    L, D, ops = _mods()
    lib = L.lib()
    assert lib.tb_mse_loss_weighted_workspace_bytes(8, 4, 64, 64) == 8 * 17 * 4
    assert lib.tb_mse_loss_weighted_workspace_bytes(3, 4, 5, 7) == 3 * 2 * 4
    assert lib.tb_mse_loss_weighted_workspace_bytes(0, 4, 5, 7) < 0
    t = torch.zeros(2, 4, 8, 8, device=dev)
    ws = torch.zeros(2, device=dev)
    rc = lib.tb_mse_loss_weighted_f32(L.ptr(t), L.ptr(t), L.ptr(t), L.ptr(t), L.ptr(ws), None, 2, 4, 8, 8, L.ptr(ws), 8, L.stream())
    assert rc == -22


# ------------------------------------------------------------------------------------------------------------------ 3. replay
class FakeTokenizer:
    model_max_length = 77

    def __call__(self, prompt, truncation=True, padding="max_length", max_length=77, return_tensors="pt"):
        ids = [49406] + [sum(map(ord, w)) % 49405 for w in prompt.split()][:max_length - 2]
        return types.SimpleNamespace(input_ids=torch.tensor([ids + [49407] * (max_length - len(ids))], dtype=torch.int64))


def _seed(s):
    np.random.seed(s)
    random.seed(s)
    torch.manual_seed(s)


def _states():
    a = np.random.get_state()
    return (a[0], a[1].tobytes(), a[2], a[3], a[4]), random.getstate(), torch.get_rng_state().numpy().tobytes()


def _rgb(seed, h, w):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def test_a_mask_replays_the_images_augmentation_and_never_perturbs_it():
    L, D, ops = _mods()
    pipe = D.PairedAugmentation(hflip="inversion", inversion=True, p=1.0, color_prob=1.0)
    a, m = _rgb(1, 48, 64), _mask(2, 48, 64)
    img, msk = D.to_device_image(a), D.to_device_mask(m)
    assert np.array_equal(D.to_host_rgb(msk), np.repeat(m[:, :, None], 3, axis=2))
    seen = set()
    for s in range(40):
        _seed(s)
        i0, p0, none = pipe(img, "a photo of <x>")
        st0 = _states()
        _seed(s)
        i1, p1, m1 = pipe(img, "a photo of <x>", msk)
        st1 = _states()
        _seed(s)
        m2, _, _ = pipe(msk, "a photo of <x>")          # the mask image on its own through the same pipeline under the same seeds
        assert none is None and p0 == p1 and st0 == st1, s
        assert i0.shape == i1.shape == m1.shape and torch.equal(i0, i1), s
        assert torch.equal(m1, m2), s
        g = D.to_host_rgb(m1)
        assert np.array_equal(g[..., 0], g[..., 1]) and np.array_equal(g[..., 0], g[..., 2])      # still grey
        seen |= {w for w in ("<zoom", "<crop>", "<left", "<right", "<hflip>", "<collage", "<grayscale") if w in p1}
    assert len(seen) == 7, seen    # every op came up
    with pytest.raises(TypeError):
        pipe(img, "x", msk[:, :10])


def test_the_feeder_applies_resize_and_crop_to_the_mask_and_fills_loss_weight():
    L, D, ops = _mods()
    size, floor = 32, 0.25
    rgbs, masks = [_rgb(3, 70, 90), _rgb(4, 96, 80)], [_mask(5, 70, 90), _mask(6, 96, 80)]
    templates = ["a photo of {}", "{} on a table"]

    def feeder(kind):
        cfg = dict(hflip="inversion", inversion=True, p=1.0, color_prob=1.0)
        if kind == "plain":
            items = [(D.to_device_image(a), "<s>") for a in rgbs]
        elif kind == "masked":
            items = [(D.to_device_image(a), "<s>", D.to_device_mask(m)) for a, m in zip(rgbs, masks)]
        else:   # the mask images as the images
            items = [(D.to_device_mask(m), "<s>") for m in masks]
        return D.DeviceFeeder(items, FakeTokenizer(), templates, size=size, center_crop=False, augment_pipe=D.PairedAugmentation(**cfg),
                              mask_floor=floor if kind == "masked" else 0.0)

    idx = [0, 1, 1, 0, 1]
    out = {}
    for kind in ("plain", "masked", "mask_alone"):
        _seed(11)
        out[kind] = (feeder(kind).batch(idx), _states())
    (b0, st0), (b1, st1), (b2, _) = out["plain"], out["masked"], out["mask_alone"]
    assert "loss_weight" not in b0 and st0 == st1
    assert b0["prompts"] == b1["prompts"] and torch.equal(b0["input_ids"], b1["input_ids"]) and torch.equal(b0["pixel_values"], b1["pixel_values"])
    lw = b1["loss_weight"]
    assert tuple(lw.shape) == (len(idx), 1, size // 8, size // 8) and lw.dtype == torch.float32
    bytes_ = ((b2["pixel_values"][:, 0].cpu().double() * 0.5 + 0.5) * 255).round().to(torch.uint8).numpy()   # the cropped mask bytes
    for b in range(len(idx)):
        want = R.pool_ref(bytes_[b], 0, 0, size // 8, size // 8, 8, floor)
        assert np.array_equal(lw[b, 0].cpu().numpy().view(np.uint32), want.view(np.uint32)), b
    assert floor <= float(lw.min()) < float(lw.max()) <= 1.0
    # one image without a mask in a masked run trains unmasked: all-white
    _seed(11)
    mixed = D.DeviceFeeder([(D.to_device_image(rgbs[0]), "<s>", D.to_device_mask(masks[0])), (D.to_device_image(rgbs[1]), "<s>")], FakeTokenizer(),
                           templates, size=size, center_crop=True, augment_pipe=None, mask_floor=floor).batch([0, 1])
    assert torch.equal(mixed["loss_weight"][1], torch.ones(1, size // 8, size // 8, device=dev)) and float(mixed["loss_weight"][0].min()) < 1.0
    # the prefetcher stages and commits the weights beside the pixels
    pv, ids, w_in = torch.zeros(2, 3, size, size, device=dev), torch.zeros(2, 77, dtype=torch.int64, device=dev), torch.ones(2, 1, 4, 4, device=dev)
    _seed(11)
    pre = D.PrefetchFeeder(feeder("masked"), 2, pv, ids, loss_weight=w_in)
    pre.prefetch(idx[:2])
    assert pre.commit() == b1["prompts"][:2]
    torch.cuda.synchronize()
    assert torch.equal(w_in, lw[:2]) and torch.equal(pv, b1["pixel_values"][:2])
    with pytest.raises(ValueError):
        D.PrefetchFeeder(feeder("masked"), 2, pv, ids)


# ------------------------------------------------------------------------------------------------------------------ 4. the step
def _graph_nodes(step):
    import ctypes
    hip_path = next(l.split()[-1] for l in open("/proc/self/maps") if "libamdhip64" in l)    # the HIP runtime this process already uses
    n = ctypes.c_size_t(0)
    rc = ctypes.CDLL(hip_path).hipGraphGetNodes(ctypes.c_void_p(step.graph[0].raw_cuda_graph()), None, ctypes.byref(n))
    assert rc == 0, rc
    return int(n.value)


def _build(mode, masked_oracle=True):
    """the tiny models of tests/test_gpu_model.py (fp16) / tests/test_gpu_f32.py (fp32) -> (oracle state, HIP step, added ids)"""
    from oracle import train_step as ts
    from textboost_amd.trainer import StepHyper, TextBoostStep
    B, hw, D = 2, 16, 64
    if mode == "fp16":
        from tests import test_gpu_model as TM
        ref_unet, hip_unet, _ = TM.make_unet(B, hw, D, seed=3)
        student, teacher, hip_te, hip_teacher, added, null = TM.make_encoders(B, D, seed=4)
        hp = StepHyper(use_grad_scaler=True, init_scale=65536.0)
    else:
        from tests import test_gpu_f32 as TF
        ref_unet, hip_unet = TF._small_unet_f32(B, hw, D, seed=3)
        student, teacher, hip_te, hip_teacher, added, null = TF._encoders_f32(B, D, seed=4)
        hp = StepHyper(use_grad_scaler=False, init_scale=1.0)
    cls = R.MaskedTrainState if masked_oracle else ts.TrainState
    st_ref = cls(student, teacher, ref_unet, added, ts.StepConfig())
    step = TextBoostStep(hip_unet, hip_te, hip_teacher, hp, (B, 4, hw, hw), device=dev)
    step.external_noise = True
    return st_ref, step, added


def _inputs(g, B, hw, added):
    from oracle import train_step as ts
    return (ts.synthetic_ids(B, added, g), ts.synthetic_ids(B, added, g, prior=True), torch.randn(B, 4, hw, hw, generator=g),
            torch.randn(B, 4, hw, hw, generator=g), torch.randint(0, 1000, (B,), generator=g))


def _load(step, ids, pids, x0, noise, t):
    step.x0.copy_(x0); step.noise.copy_(noise); step.timesteps.copy_(t)
    step.input_ids.copy_(ids); step.prior_ids.copy_(pids)


@pytest.mark.parametrize("mode", ["fp16", "fp32"])
def test_masked_step_matches_the_oracle_step_with_the_weighted_loss(mode):
    """two optimizer steps, random weights with one all-zero sample; the bounds are those of test_full_step_matches_oracle_elementwise (fp16) and
    test_full_step_f32_matches_oracle_elementwise (fp32) for the unmasked step"""
    B, hw = 2, 16
    st_ref, step, added = _build(mode)
    lw = step.enable_loss_weight()
    assert tuple(lw.shape) == (B, 1, hw, hw) and float(lw.min()) == 1.0
    g = torch.Generator().manual_seed(5)
    te_ref = st_ref.te
    for it in range(2):
        ids, pids, x0, noise, t = _inputs(g, B, hw, added)
        weight = torch.rand(B, 1, hw, hw, generator=g)
        weight[it % B] = 0
        out = st_ref.step(x0, noise, t, ids, pids, weight)
        _load(step, ids, pids, x0, noise, t)
        step.loss_weight.copy_(weight)
        step.step_eager()
        sc = step.scalars()
        assert sc["found_inf"] == 0.0
        L_ = len(te_ref.layers)
        gA = torch.stack([torch.cat(out["g_lora"][6 * l + 0: 6 * l + 6: 2]) for l in range(L_)])
        gB = torch.stack([torch.cat(out["g_lora"][6 * l + 1: 6 * l + 6: 2]) for l in range(L_)])
        clip = min(1.0, 1.0 / (out["lora_grad_norm"] + 1e-6))   # the oracle's g_lora are post-clip
        w, wr = step.te.token_table.cpu(), te_ref.token_embedding.weight.detach()
        A_ref = torch.stack([torch.cat([l.q.lora_A, l.k.lora_A, l.v.lora_A]) for l in te_ref.layers]).detach()
        torch.testing.assert_close(w[:49408], wr[:49408], rtol=1e-6, atol=1e-7)       # decay-only rows
        if mode == "fp16":
            inv = 1.0 / 65536.0 if it == 0 else 1.0 / sc["loss_scale"]
            assert abs(sc["loss_mse"] - out["mse"]) < 2e-2 * abs(out["mse"]) + 1e-4, (sc, out["mse"])
            assert abs(sc["grad_norm"] - out["lora_grad_norm"]) < 5e-2 * out["lora_grad_norm"]
            parity(f"masked step {it} grad lora_A", step.te.grad_A * inv * clip, gA, rel=4e-3, maxabs=6e-3)
            parity(f"masked step {it} grad lora_B", step.te.grad_B * inv * clip, gB, rel=4e-3, maxabs=6e-3)
            parity(f"masked step {it} grad added rows", step.te.grad_added * inv, out["g_emb_added"], rel=4e-3, maxabs=6e-3)
            assert (w[added] - wr[added]).abs().max().item() < 2.5e-3
            assert ((w[added] - wr[added]).norm() / wr[added].norm()).item() < 2e-3
            assert (step.te.lora_A.cpu() - A_ref).abs().max().item() < 1.5e-4
        else:
            assert sc["loss_scale"] == 1.0
            assert abs(sc["loss_mse"] - out["mse"]) < 1e-5 * abs(out["mse"]) + 1e-7, (sc, out["mse"])
            assert abs(sc["grad_norm"] - out["lora_grad_norm"]) < 1e-4 * out["lora_grad_norm"]
            parity(f"masked fp32 step {it} grad lora_A", step.te.grad_A * clip, gA, rel=1e-4, maxabs=1e-4)
            parity(f"masked fp32 step {it} grad lora_B", step.te.grad_B * clip, gB, rel=1e-4, maxabs=1e-4)
            parity(f"masked fp32 step {it} grad added rows", step.te.grad_added, out["g_emb_added"], rel=1e-4, maxabs=1e-4)
            parity(f"masked fp32 step {it} updated added rows", w[added], wr[added], rel=2e-4, maxabs=5e-4)
            assert (step.te.lora_A.cpu() - A_ref).abs().max().item() < 2e-5
    assert step.scalars()["opt_steps"] == 2.0


def test_all_ones_weights_train_like_the_unmasked_step():
    B, hw = 2, 16
    res = []
    for masked in (False, True):
        _, step, added = _build("fp16", masked_oracle=False)
        if masked:
            step.enable_loss_weight()
        g = torch.Generator().manual_seed(5)
        for it in range(2):
            _load(step, *_inputs(g, B, hw, added))
            step.step_eager()
        assert step.scalars()["opt_steps"] == 2.0
        res.append((step.te.token_table[added].cpu(), step.te.lora_A.cpu(), step.te.lora_B.cpu(), step.scalars()["loss_mse"]))
    (w0, A0, B0, l0), (w1, A1, B1, l1) = res
    assert (w1 - w0).abs().max().item() < 2.5e-3 and ((w1 - w0).norm() / w0.norm()).item() < 2e-3
    assert (A1 - A0).abs().max().item() < 1.5e-4 and (B1 - B0).abs().max().item() < 1.5e-4
    assert abs(l1 - l0) < 2e-2 * abs(l0) + 1e-4


def test_masked_graph_replay_equals_eager_and_the_unmasked_graph_is_unchanged(monkeypatch):
    """replay = eager bit for bit with the weighted node; a step on which enable_loss_weight() was never called captures the graph it captured
    before the masked loss existed (its node count is pinned below), and the masked one differs from it by the loss node alone"""
    B, hw = 2, 16
    graph_class = torch.cuda.CUDAGraph
    monkeypatch.setattr(torch.cuda, "CUDAGraph", lambda *a, **k: graph_class(keep_graph=True))   # keep the captured hipGraph_t for the count
    outs, nodes = [], {}
    for mode in ("eager", "graph", "unmasked_graph"):
        _, step, added = _build("fp16", masked_oracle=False)
        g = torch.Generator().manual_seed(6)
        _load(step, *_inputs(g, B, hw, added))
        if mode != "unmasked_graph":
            step.enable_loss_weight().copy_(torch.rand(B, 1, hw, hw, generator=g))
            step.loss_weight[1] = 0
        if mode == "eager":
            for _ in range(4):
                step.step_eager()
        else:
            step.capture(warmup=2)
            step.replay(); step.replay()
            nodes[mode] = _graph_nodes(step)
            if mode == "graph":
                with pytest.raises(RuntimeError):
                    step.enable_loss_weight()
        torch.cuda.synchronize()
        if mode != "unmasked_graph":
            outs.append((step.te.lora_A.clone(), step.te.lora_B.clone(), step.te.token_table[49408:].clone(), step.state.clone()))
    for a, b in zip(*outs):
        torch.testing.assert_close(a, b, rtol=0, atol=0)
    print(f"[masked loss] tiny step graph nodes: unmasked {nodes['unmasked_graph']}, masked {nodes['graph']}")
    assert nodes["unmasked_graph"] == UNMASKED_TINY_STEP_NODES
    # at N = 2048 the unmasked loss is one launch (tb_mse_loss's one-block path), the weighted loss always two
    assert nodes["graph"] == nodes["unmasked_graph"] + 1


# node count of the tiny fp16 step's captured graph on the commit before the masked loss (measured there with _graph_nodes)
UNMASKED_TINY_STEP_NODES = 882


# ------------------------------------------------------------------------------------------------------------------ 5. the command line
def test_cli_trains_from_loss_weight_pt(tmp_path):
    """train_textboost.py on a tiny model directory with pixel_values.pt [+ loss_weight.pt], 3 steps: the usual layout, training.log names the
    masked loss, and all-ones weights leave the adapter of the run without the file (within the step test's bounds)"""
    import shutil
    from safetensors.torch import load_file
    from tests.test_gpu_generate import write_model_dir
    sys.path.insert(0, ROOT)
    import train_textboost as T
    mdir = str(tmp_path / "model")
    write_model_dir(mdir, hw=16)
    shutil.rmtree(os.path.join(mdir, "tokenizer"))      # tensor inputs: no tokenizer, synthetic prompts
    shutil.rmtree(os.path.join(mdir, "vae"))            # (a decoder-only file: the encoder is then built from seeded random weights)
    g = torch.Generator().manual_seed(0)
    pixels = torch.rand(3, 3, 128, 128, generator=g) * 2 - 1
    runs = {}
    for name in ("plain", "ones"):
        data = tmp_path / f"data_{name}"
        data.mkdir()
        torch.save(pixels, str(data / "pixel_values.pt"))
        if name == "ones":
            torch.save(torch.ones(3, 1, 16, 16), str(data / "loss_weight.pt"))
        out = str(tmp_path / f"run_{name}")
        T.main(T.parse_args(["--pretrained_model_name_or_path", mdir, "--instance_data_dir", str(data), "--output_dir", out,
                             "--train_batch_size", "2", "--resolution", "128", "--max_train_steps", "3", "--placeholder_token", "<dog>",
                             "--lora_rank", "4", "--mixed_precision", "fp16", "--seed", "1"]))
        log = open(os.path.join(out, "training.log")).read()
        assert ("masked loss: on" in log) == (name == "ones"), log[-2000:]
        assert {"text_encoder", "dog.bin", "training.log"} <= set(os.listdir(out))
        runs[name] = (load_file(os.path.join(out, "text_encoder", "adapter_model.safetensors")), torch.load(os.path.join(out, "dog.bin"))["<dog>"])
    (sd0, row0), (sd1, row1) = runs["plain"], runs["ones"]
    assert sd0.keys() == sd1.keys() and any(v.abs().max() > 0 for k, v in sd1.items() if "lora_B" in k)
    assert max((sd0[k].float() - sd1[k].float()).abs().max().item() for k in sd0) < 1.5e-4
    assert torch.isfinite(row1).all() and (row0 - row1).abs().max().item() < 2.5e-3
    # a weight file of the wrong shape is refused
    torch.save(torch.ones(3, 1, 8, 8), str(tmp_path / "data_ones" / "loss_weight.pt"))
    with pytest.raises(ValueError, match="loss_weight.pt"):
        T.main(T.parse_args(["--pretrained_model_name_or_path", mdir, "--instance_data_dir", str(tmp_path / "data_ones"), "--output_dir",
                             str(tmp_path / "run_bad"), "--train_batch_size", "2", "--resolution", "128", "--max_train_steps", "1",
                             "--mixed_precision", "fp16"]))
