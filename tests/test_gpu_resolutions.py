"""Full-size UNet parity OFF the tuned grid: latent sizes and batches whose maps are not 8 * 2^k per side and whose row counts are not multiples
of 128 / 256 -- where the shape predicates of the library (attention fast paths, the row-fused LayerNorm / feed-forward kernels, sub-pixel
convolutions, split-K GroupNorm) choose other kernels than at 64x64 latents.  Per case (SD1.5 unless stated):

  B = 1, 72x72 (576 px)  5184-token maps with a half-filled last 128-row tile: the generic attention kernels, no row-fused kernel anywhere,
                         upsampler convolutions through the folded-upsample gather, a 9x9 mid block
  B = 8, 72x72           the row-fused kernels (feed-forward, chain320, LayerNorm epilogue, LayerNorm fold) on 128-row tiles that straddle two
                         images (5184 % 128 = 64) while every attention fast path is refused: checked sample by sample against B = 1 runs
  B = 2, 80x80 (640 px)  the software-pipelined hd = 40 forward over 6400 queries, the LayerNorm epilogue at exactly 200 64-row tiles, hd = 80 on
                         the general kernels, a 10x10 mid block
  B = 4, 40x40 (320 px)  a 5x5 mid block: self-attention over 25 tokens, cross-attention with fewer queries than keys, GroupNorm on 25 pixels
  SD2.1, B = 2, 72x72    hd = 64 everywhere with the DMA-staged paths refused
  bf16 build, B = 2, 64  the --mixed_precision bf16 library at full size

and the whole optimizer step at B = 8, 72x72 (graph replay == eager, bit for bit; the step's size-independent invariants).

Tolerances are those of tests/test_gpu_fullsize.py (UNet prediction 3e-3 / 4e-3 / 4e-3, d(ehs) 5e-3 / 6e-3 / 3e-2 as rel-L2 / max-abs / worst
channel), held for EVERY sample: the oracle runs one sample at a time (samples are independent), which bounds its memory to a B = 1 graph.
The bf16 case takes 8x those bounds (tests/test_gpu_bf16.py: 8 significand bits against 11)."""
import pytest
import torch

from parity import parity

pytestmark = pytest.mark.gpu
dev = "cuda"
T = 77
PRED = dict(rel=3e-3, maxabs=4e-3, ch_dim=1, ch_rel=4e-3)
DEHS = dict(rel=5e-3, maxabs=6e-3, ch_dim=2, ch_rel=3e-2)


def _weights(geo, cfg, seed):
    """random-init weights rounded to fp16 (what unet.to(fp16) keeps) and the fp32 oracle module holding them, frozen"""
    from oracle.unet_sd import UNet2DCondition
    from textboost_amd import models
    sd = models.random_state_dict(models.unet_shapes(geo), seed, device="cpu")
    sd = {k: v.half().float() for k, v in sd.items()}
    with torch.device("meta"):
        ref = UNet2DCondition(cfg)
    ref = ref.to_empty(device="cpu")
    ref.load_state_dict(sd)
    for p in ref.parameters():
        p.requires_grad_(False)
    return sd, ref


@pytest.fixture(scope="module")
def sd15():
    from oracle.unet_sd import UNetConfig
    from textboost_amd import models
    return _weights(models.SD15_UNET, UNetConfig.sd15(), 91)


def _inputs(B, hw, D, seed, dt=torch.float16):
    """distinct timesteps per sample, non-zero dpred / ehs from a seeded generator; x and ehs rounded to the 16-bit type the kernels read"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 4, hw, hw, generator=g).to(dt).float()
    t = torch.randperm(1000, generator=g)[:B]
    ehs = torch.randn(B, T, D, generator=g).to(dt).float()
    dpred = torch.randn(B, 4, hw, hw, generator=g)
    return x, t, ehs, dpred


def _oracle(ref, x, t, ehs, dpred):
    """fp32 CPU oracle, one sample at a time: prediction and d(ehs) of <pred, dpred>"""
    preds, dehs = [], []
    for b in range(x.shape[0]):
        e = ehs[b:b + 1].clone().requires_grad_(True)
        p = ref(x[b:b + 1], t[b:b + 1], e)
        p.backward(dpred[b:b + 1])
        preds.append(p.detach())
        dehs.append(e.grad.detach())
        del p, e
    return torch.cat(preds), torch.cat(dehs)


def _hip(hip, x, t, ehs, dpred):
    B, D = x.shape[0], ehs.shape[-1]
    pred = hip.forward(x.to(hip.dtype).to(dev), t.to(dev), ehs.to(hip.dtype).reshape(B * T, D).to(dev).contiguous()).float().cpu()
    d_ehs = hip.backward(dpred.to(dev)).view(B, T, D).float().cpu()
    return pred, d_ehs


def _unet(geo, sd, B, hw):
    from textboost_amd.unet import HipUNet
    return HipUNet(geo, {k: v.to(dev) for k, v in sd.items()}, B, hw, hw, device=dev)


def _vs_oracle(name, geo, sd, ref, B, hw, seed, pred_bounds=PRED, dehs_bounds=DEHS, dt=torch.float16):
    x, t, ehs, dpred = _inputs(B, hw, geo.cross_attention_dim, seed, dt)
    hip = _unet(geo, sd, B, hw)
    pred, d_ehs = _hip(hip, x, t, ehs, dpred)
    del hip
    torch.cuda.empty_cache()
    pred_ref, dehs_ref = _oracle(ref, x, t, ehs, dpred)
    for b in range(B):   # every sample against its own bounds: a wrong image cannot hide behind the others
        parity(f"{name} pred, sample {b} (t={int(t[b])})", pred[b:b + 1], pred_ref[b:b + 1], **pred_bounds)
        parity(f"{name} d_ehs, sample {b}", d_ehs[b:b + 1], dehs_ref[b:b + 1], **dehs_bounds)


def test_sd15_b1_latent72_vs_oracle(sd15):
    from textboost_amd import models
    sd, ref = sd15
    _vs_oracle("SD1.5 B=1 @72x72", models.SD15_UNET, sd, ref, 1, 72, seed=1)


def test_sd15_b8_latent72_equals_eight_b1_runs(sd15):
    """B = 8 at 72x72 runs the row-fused kernels on 128-row tiles that straddle image boundaries; B = 1 (pinned to the oracle above) runs none
    of them.  Samples are independent, so each sample of the B = 8 pass must reproduce a B = 1 pass on that sample -- bounds of
    tests/test_gpu_fullsize.py::test_batch_16_equals_two_batches_of_8 (two fp16 computations with independent rounding)."""
    from textboost_amd import models
    sd, _ = sd15
    B, hw = 8, 72
    x, t, ehs, dpred = _inputs(B, hw, 768, seed=2)
    hip8 = _unet(models.SD15_UNET, sd, B, hw)
    pred8, dehs8 = _hip(hip8, x, t, ehs, dpred)
    del hip8
    torch.cuda.empty_cache()
    hip1 = _unet(models.SD15_UNET, sd, 1, hw)
    for b in range(B):
        sl = slice(b, b + 1)
        pred1, dehs1 = _hip(hip1, x[sl], t[sl], ehs[sl], dpred[sl])
        parity(f"B=8 vs B=1 @72x72 pred, sample {b} (t={int(t[b])})", pred8[sl], pred1, rel=2.5e-3, maxabs=4e-3, ch_dim=1, ch_rel=4e-3)
        parity(f"B=8 vs B=1 @72x72 d_ehs, sample {b}", dehs8[sl], dehs1, rel=4e-3, maxabs=6e-3)


def test_sd15_b2_latent80_vs_oracle(sd15):
    from textboost_amd import models
    sd, ref = sd15
    _vs_oracle("SD1.5 B=2 @80x80", models.SD15_UNET, sd, ref, 2, 80, seed=3)


def test_sd15_b4_latent40_vs_oracle(sd15):
    from textboost_amd import models
    sd, ref = sd15
    _vs_oracle("SD1.5 B=4 @40x40", models.SD15_UNET, sd, ref, 4, 40, seed=4)


def test_sd21_b2_latent72_vs_oracle():
    from oracle.unet_sd import UNetConfig
    from textboost_amd import models
    sd, ref = _weights(models.SD21_UNET, UNetConfig.sd21(), 92)
    _vs_oracle("SD2.1 B=2 @72x72", models.SD21_UNET, sd, ref, 2, 72, seed=5)


def test_bf16_sd15_b2_latent64_vs_oracle(sd15):
    """the bfloat16 build (--mixed_precision bf16) at full size; the oracle keeps the fp16-rounded weights, the bf16 module rounds them once
    more (part of the mode's own error, as in tests/test_gpu_bf16.py::test_bf16_unet_and_text_encoder_match_oracle)"""
    from textboost_amd import _lib as L
    from textboost_amd import models
    sd, ref = sd15
    prev = L.set_half("bf16")
    try:
        assert L.half_dtype() == torch.bfloat16
        x8 = lambda d: {k: 8 * v if k != "ch_dim" else v for k, v in d.items()}   # noqa: E731
        _vs_oracle("bf16 SD1.5 B=2 @64x64", models.SD15_UNET, sd, ref, 2, 64, seed=6, pred_bounds=x8(PRED), dehs_bounds=x8(DEHS),
                   dt=torch.bfloat16)
    finally:
        L.set_half(prev)


def test_step_at_latent72_batch8_graph_equals_eager_and_invariants():
    """the whole step (text encoder, UNet, losses, optimizer tail) at B = 8 and 72x72 latents: three graph-captured steps (one eager warm-up,
    two replays) == three eager steps bit for bit, and the size-independent invariants of
    tests/test_gpu_fullsize.py::test_metric_config_properties_at_batch_8"""
    from textboost_amd.workload import build_step
    n = 3
    outs = []
    for mode in ("eager", "graph"):
        torch.manual_seed(44)
        step, added = build_step(batch=8, latent=72)
        te = step.te
        w0 = te.token_table.clone()
        if mode == "graph":
            step.capture(warmup=1)
            for _ in range(n - 1):
                step.replay()
        else:
            for _ in range(n):
                step.step_eager()
        torch.cuda.synchronize()
        sc = step.scalars()
        assert sc["found_inf"] == 0.0 and sc["opt_steps"] == float(n) and sc["loss_scale"] == 65536.0, sc
        assert 0.5 < sc["loss_mse"] < 2.0 and sc["loss_kpl"] >= 0.0, sc
        first = te.first_added
        torch.testing.assert_close(te.token_table[:first], w0[:first] * (1 - 1e-3 * 1e-2) ** n, rtol=2e-6, atol=0)
        added_rows = te.token_table[first:]
        assert torch.isfinite(added_rows).all() and not torch.equal(added_rows, w0[first:])
        assert (added_rows.norm(dim=-1) <= step.mean_norm * (1 + 1e-5)).all()
        assert torch.isfinite(te.lora_A).all() and torch.isfinite(te.lora_B).all() and te.lora_B.abs().max() > 0
        outs.append((te.lora_A.clone(), te.lora_B.clone(), te.token_table[first:].clone(), step.state.clone()))
        if mode == "graph":   # pins: null prompts and position 0 come out as the null embedding, bit-exact
            ids = step.ids_all.clone()
            ids[0, 1:] = 49407
            h = te.forward(ids, slot=0).view(ids.shape[0], 77, -1)
            assert torch.equal(h[0], te.null_embedding) and torch.equal(h[3, 0], te.null_embedding[0])
        del step, te
        torch.cuda.empty_cache()
    for a, b in zip(*outs):
        torch.testing.assert_close(a, b, rtol=0, atol=0)
