"""GPU tests of the VQA score (textboost_amd/vqa_score.py, csrc/t5.hip): the three T5 kernels against float64, HipViT.hidden_states against the
fp32 CLIP restatement, the whole CLIP-FlanT5 model (a tiny one, and one block at FlanT5-XXL's widths) against tests/vqa_ref.py, and
eval_dreambooth.py --metric vqa end to end.

Measured on one MI355X (bf16; the bounds below are at most twice these):
    tiny model, B = 3       logits rel-L2 1.32e-2, per-sample |dscore| 2.05e-4 (scores 0.0107 / 0.0078 / 0.0025)
    one full-width block    logits rel-L2 1.91e-2, |dscore| 1.64e-6 (a score below 5e-5: at these widths the logits are the check)
    kernels                 rmsnorm fp32 2.3e-7 relative, 16-bit 0.500 ulp; gated gelu 0.501 ulp; attention O rel-L2 2.7e-4 (fp16) / 2.1e-3 (bf16)
"""
import csv
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import clip_ref as C
import vqa_ref as R
from parity import parity

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# bf16 against the fp32 restatement: bound <= 2 x the measured value (module docstring)
TINY_LOGITS_BOUND, TINY_SCORE_BOUND = 2.6e-2, 3.0e-4
WIDE_LOGITS_BOUND, WIDE_SCORE_BOUND = 3.8e-2, 3.2e-6


def _half_dtype(half):
    return torch.float16 if half == "fp16" else torch.bfloat16


def _ulp(ref64, half):
    """the spacing of the 16-bit type at |ref| (the subnormal spacing below its smallest normal)"""
    p, emin = (10, -14) if half == "fp16" else (7, -126)
    e = torch.floor(torch.log2(ref64.abs().clamp_min(2.0 ** emin)))
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - p)


# ---------------------------------------------------------------------------------------------------------------- rmsnorm
@pytest.mark.parametrize("half", ["fp16", "bf16"])
@pytest.mark.parametrize("M,C,strided", [(3, 128, False), (611, 4096, True)])
def test_rmsnorm_against_float64(M, C, strided, half):
    from textboost_amd import _lib as L, ops
    g = torch.Generator().manual_seed(M + C)
    ld = 2 * C + 8 if strided else C                       # strided rows: the leading columns of a wider buffer
    buf = torch.randn(M, ld, generator=g) * torch.logspace(-2, 1.5, M)[:, None]
    gamma = 1.0 + 0.3 * torch.randn(C, generator=g)
    x = buf.cuda()[:, :C]
    ref = buf[:, :C].double()
    ref = ref * torch.rsqrt(ref.pow(2).mean(-1, keepdim=True) + 1e-6) * gamma.double()
    with L.use_half(half):
        y32 = torch.full((M, C), float("nan"), device="cuda")
        y16 = torch.full((M, C + 8), float("nan"), device="cuda", dtype=L.half_dtype())[:, :C]
        ops.rmsnorm_fwd(x, y32, gamma.cuda(), 1e-6)
        ops.rmsnorm_fwd(x, y16, gamma.cuda(), 1e-6)
        torch.cuda.synchronize()
    e32 = ((y32.cpu().double() - ref).abs() / ref.abs().clamp_min(1e-30)).max().item()
    e16 = ((y16.cpu().double() - ref).abs() / _ulp(ref, half)).max().item()
    print(f"[rmsnorm {M}x{C} {half}] fp32 out: max rel {e32:.2e} (<= 1e-6); 16-bit out: max {e16:.3f} ulp (<= 1)")
    assert e32 <= 1e-6 and e16 <= 1.0


def test_rmsnorm_refuses_bad_arguments():
    from textboost_amd import _lib as L
    b = torch.zeros(1024, device="cuda")
    assert L.lib().tb_rmsnorm_fwd(L.ptr(b), 16, L.ptr(b), 16, 7, L.ptr(b), 4, 16, 1e-6, L.stream()) == -22     # unknown dtype
    assert L.lib().tb_rmsnorm_fwd(L.ptr(b), 8, L.ptr(b), 16, L.TB_F32, L.ptr(b), 4, 16, 1e-6, L.stream()) == -22   # ldx < C


# ---------------------------------------------------------------------------------------------------------------- gated gelu
@pytest.mark.parametrize("half", ["fp16", "bf16"])
@pytest.mark.parametrize("M,F", [(5, 256), (70, 10240)])
def test_gated_gelu_against_float64(M, F, half):
    from textboost_amd import _lib as L, ops
    g = torch.Generator().manual_seed(M)
    dt = _half_dtype(half)
    hg = ((torch.rand(M, 2 * F + 8, generator=g) * 16.0 - 8.0)).to(dt)             # inputs span [-8, 8]
    hg[0, :4] = torch.tensor([-8.0, 8.0, 0.0, -0.0]).to(dt)
    hg[0, F:F + 4] = torch.tensor([8.0, -8.0, 3.0, 5.0]).to(dt)
    h, gate = hg[:, :F].double(), hg[:, F:2 * F].double()
    ref = 0.5 * h * (1.0 + torch.tanh(np.sqrt(2.0 / np.pi) * (h + 0.044715 * h.pow(3)))) * gate
    # the float64 formula's own error: 1 + tanh u carries an absolute rounding error of 2^-53 .. 2^-52, which is all of it below u = -18
    # (h < -7) and is visible to bfloat16, whose normal range reaches 1e-38 (to fp16 it is not: its smallest subnormal is 6e-8)
    ref_err = 0.5 * (h * gate).abs() * 2.0 ** -52
    views = [(0, "vector path")] + ([(1, "scalar path: rows not 16-byte aligned")] if F == 256 else [])
    with L.use_half(half):
        for shift, name in views:
            flat = torch.zeros(M * (2 * F + 8) + 8, device="cuda", dtype=dt)
            src = flat[shift:shift + M * (2 * F + 8)].view(M, 2 * F + 8)
            src.copy_(hg)
            out = torch.full((M, F + 8), float("nan"), device="cuda", dtype=dt)[:, :F]
            ops.gated_gelu_tanh(src[:, :2 * F], out)
            torch.cuda.synchronize()
            e = (((out.cpu().double() - ref).abs() - ref_err).clamp_min(0.0) / _ulp(ref, half)).max().item()
            print(f"[gated gelu {M}x{F} {half}, {name}] max {e:.3f} ulp (<= 1)")
            assert e <= 1.0


# ---------------------------------------------------------------------------------------------------------------- attention
H_ATT = 3
ATT_CASES = {   # name: (B, Sq, Skv, causal, rel, kv_len)
    "2x2 causal+rel": (2, 2, 2, True, True, None),
    "70x70 rel": (2, 70, 70, False, True, None),                    # a partial third key tile, one query block
    "130x130 rel kv_len": (2, 130, 130, False, True, [130, 37]),    # two query blocks; batch 1 skips three of its five key tiles
    "2x70 cross kv_len": (2, 2, 70, False, False, [70, 9]),
    "130x130 causal+rel": (1, 130, 130, True, True, None),
}


def _attn_ref64(q, k, v, B, H, Sq, Skv, scale, rel, kv_len, causal):
    """float64 softmax attention on the 16-bit operands -> (O [B*Sq, H*64], LSE [B, H, Sq])"""
    split = lambda t, S: t.double().cpu().reshape(B, S, H, 64).transpose(1, 2)
    s = split(q, Sq) @ split(k, Skv).transpose(-1, -2) * scale
    i, j = torch.arange(Sq)[:, None], torch.arange(Skv)[None, :]
    if rel is not None:
        s = s + rel.double().cpu()[:, j - i + Sq - 1][None]
    if causal:
        s = s.masked_fill((j > i)[None, None], float("-inf"))
    vv = split(v, Skv)
    if kv_len is not None:
        for b, n in enumerate(kv_len):
            s[b, :, :, n:] = float("-inf")
            vv[b, :, n:] = 0.0          # the test poisons these rows: the reference must not read them either
    o = (s.softmax(-1) @ vv).transpose(1, 2).reshape(B * Sq, H * 64)
    return o, torch.logsumexp(s, dim=-1)


def _att_bounds(half):
    """the project's attention-forward bounds (tests/test_gpu_norm_attn.py: rel-L2 2e-3, max-abs 4e-3, worst channel 3e-3); bf16 = x 8"""
    f = 1.0 if half == "fp16" else 8.0
    return dict(rel=2e-3 * f, maxabs=4e-3 * f, ch_dim=1, ch_rel=3e-3 * f)


@pytest.mark.parametrize("half", ["fp16", "bf16"])
@pytest.mark.parametrize("case", list(ATT_CASES))
def test_attention_rel_against_float64(case, half):
    from textboost_amd import _lib as L, ops
    B, Sq, Skv, causal, use_rel, kv_len = ATT_CASES[case]
    H, C = H_ATT, H_ATT * 64
    dt = _half_dtype(half)
    g = torch.Generator().manual_seed(Sq * 131 + Skv)
    if Sq == Skv:   # column slices of one fused buffer, like the q | k | v GEMM's output
        qkv = (torch.randn(B * Sq, 3 * C, generator=g) * 0.4).to(dt).cuda()
        q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
    else:
        q = (torch.randn(B * Sq, C, generator=g) * 0.4).to(dt).cuda()
        kv = (torch.randn(B * Skv, 2 * C, generator=g) * 0.4).to(dt).cuda()
        k, v = kv[:, :C], kv[:, C:]
    v.mul_(2.5)
    rel = (torch.randn(H, Sq + Skv - 1, generator=g) * 1.5).cuda() if use_rel else None
    o_ref, lse_ref = _attn_ref64(q, k, v, B, H, Sq, Skv, 1.0, rel, kv_len, causal)
    lens = None
    if kv_len is not None:
        lens = torch.tensor(kv_len, dtype=torch.int32, device="cuda")
        for b, n in enumerate(kv_len):   # nothing beyond the length may reach the output
            k[b * Skv + n:(b + 1) * Skv] = float("nan")
            v[b * Skv + n:(b + 1) * Skv] = float("nan")
    with L.use_half(half):
        o = torch.full((B * Sq, C), float("nan"), device="cuda", dtype=dt)
        lse = torch.full((B, H, Sq), float("nan"), device="cuda")
        ops.attention_rel_fwd(q, k, v, o, lse, B, H, Sq, Skv, 64, rel=rel, kv_len=lens, scale=1.0, causal=causal)
        o2 = torch.full_like(o, float("nan"))
        ops.attention_rel_fwd(q, k, v, o2, None, B, H, Sq, Skv, 64, rel=rel, kv_len=lens, scale=1.0, causal=causal)   # LSE may be NULL
        torch.cuda.synchronize()
    assert torch.isfinite(o).all() and torch.isfinite(lse).all(), "outputs of masked batches must be finite"
    assert torch.equal(o, o2)
    parity(f"attention_rel {case} {half}", o, o_ref, **_att_bounds(half))
    e = (lse.cpu().double() - lse_ref).abs().max().item()
    print(f"[attention_rel {case} {half}] max |dLSE| {e:.2e}")
    assert e < 2e-3


@pytest.mark.parametrize("half", ["fp16", "bf16"])
def test_attention_rel_without_bias_matches_attention_fwd(half):
    from textboost_amd import _lib as L, ops
    B, H, S, C = 2, H_ATT, 130, H_ATT * 64
    dt = _half_dtype(half)
    g = torch.Generator().manual_seed(11)
    qkv = torch.randn(B * S, 3 * C, generator=g).to(dt).cuda()
    q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
    o_ref, lse_ref = _attn_ref64(q, k, v, B, H, S, S, 64 ** -0.5, None, None, False)
    with L.use_half(half):
        o, o_old = torch.empty(B * S, C, device="cuda", dtype=dt), torch.empty(B * S, C, device="cuda", dtype=dt)
        lse, lse_old = torch.empty(B, H, S, device="cuda"), torch.empty(B, H, S, device="cuda")
        ops.attention_rel_fwd(q, k, v, o, lse, B, H, S, S, 64, scale=64 ** -0.5)
        ops.attention_fwd(q, k, v, o_old, lse_old, B, H, S, S, 64)
        torch.cuda.synchronize()
    parity(f"attention_rel (no rel, no kv_len) {half} vs float64", o, o_ref, **_att_bounds(half))
    parity(f"tb_attention_fwd {half} vs float64", o_old, o_ref, **_att_bounds(half))
    parity(f"attention_rel vs tb_attention_fwd {half}", o, o_old, **_att_bounds(half))
    assert (lse - lse_old).abs().max().item() < 2e-3


def test_attention_rel_refuses_other_head_dims():
    from textboost_amd import _lib as L, ops
    t = torch.zeros(64, 3 * 40, device="cuda", dtype=torch.float16)
    d = ops._attn_desc(t, t, t, t, None, 1, 3, 64, 64, 40, 1.0, False)
    assert L.lib().tb_attention_rel_fwd(d, None, None, L.stream()) == -22
    t = torch.zeros(64, 3 * 64 + 4, device="cuda", dtype=torch.float16)      # a leading dimension the 16-byte loads cannot take
    d = ops._attn_desc(t, t, t, t, None, 1, 3, 64, 64, 64, 1.0, False)
    assert L.lib().tb_attention_rel_fwd(d, None, None, L.stream()) == -22


# ---------------------------------------------------------------------------------------------------------------- hidden_states
@pytest.fixture(scope="module")
def fixture(golden_dir):
    return torch.load(os.path.join(golden_dir, "clip_vit_tiny.pt"), weights_only=False)


@pytest.fixture(scope="module")
def clip_sd(fixture):
    return {k: v.float() for k, v in fixture["state_dict_fp16"].items()}


@pytest.fixture(scope="module")
def images(fixture):
    """the fixture's three images through CLIP-T's device preprocessing -> (resident RGBX [3, 224, 224], CLIP pixel_values of the same bytes)"""
    from textboost_amd import augment
    from textboost_amd.clip_score import preprocess
    dev = [preprocess(augment.to_device_image(a.numpy()), 224, clip_i=False).contiguous() for a in fixture["images"]]
    u8 = np.stack([augment.to_host_rgb(d) for d in dev])
    return torch.stack(dev), C.normalise(u8)


def _bf16_vision(fixture, clip_sd):
    from textboost_amd import _lib as L
    from textboost_amd.clip_score import HipCLIPVision, clip_model_geometry_from_config
    vg, _, _ = clip_model_geometry_from_config(fixture["config"])
    with L.use_half("bf16"):
        return HipCLIPVision(vg, clip_sd)


def test_hidden_states_match_restatement(fixture, clip_sd, images):
    from textboost_amd import _lib as L
    rgbx, pv = images
    tower = _bf16_vision(fixture, clip_sd)
    n = len(tower.layers)
    with L.use_half("bf16"), torch.no_grad():
        before = tower.encode(rgbx).clone()
        hs = tower.hidden_states(rgbx, n - 1).clone()
        after = tower.encode(rgbx).clone()
        full = tower.hidden_states(rgbx, n).clone()
        ref = C.vision_residuals(clip_sd, fixture["config"], pv)
    assert torch.equal(before, after), "encode changed after a hidden_states call"
    parity("hidden_states[-2] (bf16 tiny tower)", hs, ref[-2], rel=1.6e-2)     # the tiny towers' existing bf16 bound (test_gpu_dino_score.py)
    parity("hidden_states[-1] (bf16 tiny tower)", full, ref[-1], rel=1.6e-2)
    assert not torch.equal(hs, full)
    with pytest.raises(ValueError):
        tower.hidden_states(rgbx, n + 1)


# ---------------------------------------------------------------------------------------------------------------- the whole model, tiny
# chosen on the CPU so that the conditions of `tiny_reference` hold AND the fp32 restatement is a fair yardstick for bf16: with a bias table of
# std 2, unit-gain q / k and a 3 x head (seed 1) one sample's logits moved by 16 % when the restatement's own GEMM operands were rounded to bf16
# (device: 7.3e-2 rel-L2 over the batch); these weights keep that sensitivity at 1.2e-2, the order of the tiny towers
TINY = dict(seed=4, gain=0.7, rel_std=1.0, head_gain=2.0)
TINY_LABELS, TINY_DEC = [19, 1], [0, 19]
TINY_LENGTHS = ((9, 31), (4, 3), (17, 130))                      # text ids before / after the image rows: T = 298, 265, 405


def _tiny_ids():
    g = torch.Generator().manual_seed(TINY["seed"])
    rows = []
    for n_head, n_tail in TINY_LENGTHS:
        head, tail = (torch.randint(3, 128, (n,), generator=g).tolist() for n in (n_head, n_tail))
        rows.append(head + [1, R.IMAGE_TOKEN_INDEX] + tail + [1])
    return rows


@pytest.fixture(scope="module")
def tiny_reference(fixture, clip_sd, images):
    """the restatement's fp32 logits and scores, once, and the discrimination of these inputs: what a device model that drops the bias, ignores
    the lengths, mixes up the images or reads the wrong vision layer would score.  A random T5 that answers 1 / vocab for everything would
    pass any tolerance; these weights, ids and labels do not allow that."""
    cfg = R.tiny_t5_config()
    sd = R.random_t5_state(cfg, **TINY)
    ids = _tiny_ids()
    _, pv = images
    with torch.no_grad():
        run = lambda ab: R.vqa_logits(clip_sd, fixture["config"], sd, cfg, pv, ids, TINY_DEC, ablate=ab)
        logits = run(None)
        scores = R.answer_scores(logits, TINY_LABELS)
        moved = {ab: (R.answer_scores(run(ab), TINY_LABELS) - scores).abs().max().item() for ab in ("no_rel", "no_len", "swap_images", "last_layer")}
    pair = min(abs(scores[i] - scores[j]).item() for i, j in itertools.combinations(range(3), 2))
    print(f"[tiny reference] scores {[round(s, 4) for s in scores.tolist()]}  closest pair {pair:.4f}  moved by {moved}")
    return dict(cfg=cfg, sd=sd, ids=ids, logits=logits, scores=scores, pair=pair, moved=moved)


def test_tiny_inputs_discriminate(tiny_reference):
    """a condition on the inputs (CPU, the restatement alone): >= 10 x the score bound between every two samples and under every ablation"""
    need = 10 * TINY_SCORE_BOUND
    assert tiny_reference["pair"] >= need, (tiny_reference["pair"], need)
    for ab, d in tiny_reference["moved"].items():
        assert d >= need, (ab, d, need)


def _model(cfg, sd, vision):
    from textboost_amd import vqa_score as V
    return V.HipCLIPFlanT5(V.t5_geometry_from_config(cfg), sd.items(), vision)


def test_tiny_model_matches_restatement(fixture, clip_sd, images, tiny_reference):
    from textboost_amd import vqa_score as V
    rgbx, _ = images
    model = _model(tiny_reference["cfg"], tiny_reference["sd"], _bf16_vision(fixture, clip_sd))
    with torch.no_grad():
        logits = model.logits(rgbx, tiny_reference["ids"], TINY_DEC)
        scores = V.answer_scores(logits, TINY_LABELS).cpu()
    assert torch.isfinite(logits).all()
    rel = ((logits.cpu() - tiny_reference["logits"]).norm() / tiny_reference["logits"].norm()).item()
    ds = (scores - tiny_reference["scores"]).abs().max().item()
    print(f"[tiny CLIP-FlanT5, B=3] logits rel-L2 {rel:.3e} (<= {TINY_LOGITS_BOUND})  |dscore| {ds:.3e} (<= {TINY_SCORE_BOUND})  "
          f"scores {[round(s, 4) for s in scores.tolist()]} vs {[round(s, 4) for s in tiny_reference['scores'].tolist()]}")
    assert rel <= TINY_LOGITS_BOUND and ds <= TINY_SCORE_BOUND
    # a batch of one gives the same answer as its row of the batch of three (padding and lengths do not leak between samples)
    with torch.no_grad():
        alone = model.logits(rgbx[1:2], tiny_reference["ids"][1:2], TINY_DEC)
    parity("sample 1 alone vs in the batch", alone[0], logits[1], rel=2e-3)


# ---------------------------------------------------------------------------------------------------------------- one full-width block
def test_one_full_width_block(fixture, clip_sd, images):
    """d_model 4096, 64 heads, d_ff 10240, one encoder and one decoder layer, B = 1, T = 600: GEMM dispatch and strides at FlanT5-XXL's widths"""
    from textboost_amd import vqa_score as V
    torch.set_num_threads(min(16, torch.get_num_threads()))
    cfg = R.tiny_t5_config(d_model=4096, num_heads=64, d_ff=10240, num_layers=1, num_decoder_layers=1, vocab_size=256)
    g = torch.Generator(device="cuda").manual_seed(7)
    dev_sd = {}
    for k, shp in R.t5_shapes(cfg).items():   # R.random_t5_state's distributions at gain 1, drawn on the device (0.5 G values)
        r = torch.randn(shp, generator=g, device="cuda")
        if k.endswith("layer_norm.weight"):
            r = 1.0 + 0.1 * r
        elif k.endswith(".bias"):
            r = 0.1 * r
        elif "relative_attention_bias" in k:
            r = 2.0 * r
        elif k != "shared.weight":
            r = r * shp[1] ** -0.5 * (3.0 if k == "lm_head.weight" else 1.0)
        dev_sd[k] = r
    sd = {k: v.cpu() for k, v in dev_sd.items()}
    rgbx, pv = images
    gi = torch.Generator().manual_seed(3)
    ids = [torch.randint(3, 256, (40,), generator=gi).tolist() + [1, R.IMAGE_TOKEN_INDEX] + torch.randint(3, 256, (302,), generator=gi).tolist() + [1]]
    labels, dec = [9, 1], [0, 9]
    model = _model(cfg, dev_sd, _bf16_vision(fixture, clip_sd))
    del dev_sd
    with torch.no_grad():
        logits = model.logits(rgbx[:1], ids, dec)
        scores = V.answer_scores(logits, labels).cpu()
        ref = R.vqa_logits(clip_sd, fixture["config"], sd, cfg, pv[:1], ids, dec)
        ref_scores = R.answer_scores(ref, labels)
    assert logits.shape == (1, 2, 256) and len(ids[0]) - 1 + 256 == 600
    rel = ((logits.cpu() - ref).norm() / ref.norm()).item()
    ds = (scores - ref_scores).abs().max().item()
    print(f"[one full-width block, T=600] logits rel-L2 {rel:.3e} (<= {WIDE_LOGITS_BOUND})  |dscore| {ds:.3e} (<= {WIDE_SCORE_BOUND})  "
          f"score {scores.item():.4f} vs {ref_scores.item():.4f}")
    assert rel <= WIDE_LOGITS_BOUND and ds <= WIDE_SCORE_BOUND


# ---------------------------------------------------------------------------------------------------------------- CLI end to end
def _pad_square(rgb):
    h, w, _ = rgb.shape
    s = max(h, w)
    out = np.empty((s, s, 3), np.uint8)
    out[...] = np.array([int(c * 255) for c in C.CLIP_MEAN], np.uint8)
    out[(s - h) // 2:(s - h) // 2 + h, (s - w) // 2:(s - w) // 2 + w] = rgb
    return out


def test_cli_end_to_end(tmp_path, fixture, clip_sd):
    pytest.importorskip("transformers")
    from PIL import Image
    from safetensors.torch import save_file
    from textboost_amd import vqa_score as V
    cdir, vdir = tmp_path / "clip", tmp_path / "vqa"
    cdir.mkdir()
    with open(cdir / "config.json", "w") as f:
        json.dump(dict(fixture["config"], architectures=["CLIPModel"], model_type="clip"), f)
    save_file({k: v.contiguous() for k, v in clip_sd.items()}, str(cdir / "model.safetensors"))
    cfg = R.tiny_t5_config()
    sd = R.random_t5_state(cfg, seed=2, gain=0.5, rel_std=2.0, head_gain=3.0)   # weights whose favoured first token (85) scores 0.05 .. 0.2
    names = ["a_dog_in_the_snow", "a_red_dog"]
    texts = [C.prompt_of(n + ".png") for n in names]
    prompts = [V.T5_CHAT_TEMPLATE.format(question=V.QUESTION_TEMPLATE.format(t)) for t in texts]
    yes = R.write_tiny_tokenizer(str(vdir), prompts + [V.ANSWER_TEMPLATE], cfg["vocab_size"])["Yes"]
    for k in ("lm_head.weight", "shared.weight"):   # "Yes" takes the place of token 85
        w = sd[k].clone()
        w[[yes, 85]] = w[[85, yes]]
        sd[k] = w
    R.write_vqa_model(str(vdir), cfg, sd, prompts + [V.ANSWER_TEMPLATE])
    rng = np.random.default_rng(5)
    d = tmp_path / "bench" / "run-sd15" / "seed0" / "dog"
    d.mkdir(parents=True)
    paths = []
    for n, (h, w) in zip(names, ((256, 256), (200, 260))):   # the second one is padded to a square first
        y, x = np.mgrid[0:h, 0:w]
        a = np.clip(rng.integers(40, 200, 3) + 60 * np.sin(x / rng.uniform(5, 20))[..., None] + rng.normal(0, 10, (h, w, 3)) + y[..., None] * 0.1,
                    0, 255).astype(np.uint8)
        Image.fromarray(a).save(d / f"{n}.png")
        paths.append(str(d / f"{n}.png"))
    run = tmp_path / "runs" / "run-sd15"
    run.mkdir(parents=True)
    cmd = [sys.executable, os.path.join(ROOT, "eval_dreambooth.py"), str(run), "--outdir", str(tmp_path / "bench"), "--skip-gen", "--metric", "vqa",
           "--seeds", "0", "--clip-model", str(cdir), "--vqa-model", str(vdir), "--batch-size", "4"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "VQA score" in r.stdout and "images/s" in r.stdout
    rows = list(csv.reader(open(run / "metric_last.csv")))
    assert rows[0] == ["seed", "clip_score", "vqa_score", "clip_i", "clip_i_unseen", "dino", "dino_unseen"]
    tok = V.load_t5_tokenizer(str(vdir))
    ids, labels, dec = V.build_ids(tok, texts, cfg["decoder_start_token_id"])
    u8 = np.stack([C.pil_preprocess(_pad_square(np.asarray(Image.open(p).convert("RGB"))), 224, False) for p in sorted(paths)])
    order = [paths.index(p) for p in sorted(paths)]
    with torch.no_grad():
        want = R.answer_scores(R.vqa_logits(clip_sd, fixture["config"], sd, cfg, C.normalise(u8), [ids[i] for i in order], dec), labels)
    got = [float(v) for v in rows[1][1:]]
    print(f"[e2e vqa] csv {rows[1]}  restatement {want.tolist()} mean {want.mean().item():.5f}")
    assert want.mean().item() > 5e-3, "the inputs must give a score that shows in a %.3f column"
    assert rows[1][0] == "0" and got[0] == 0.0 and got[2:] == [0.0] * 4          # the other columns stay 0.000
    assert abs(got[1] - want.mean().item()) <= 1e-3 + 5e-4   # 1e-3 on the mean (as for the CLIP columns), plus the CSV's %.3f rounding
