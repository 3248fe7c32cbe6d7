"""Token attention maps on the GPU: the kernel (csrc/attn_maps.hip) against the float64 reference of tests/attn_maps_ref.py, the recorder inside
HipUNet.forward and HipSampler.denoise, and `inference.py --attn-map`.

Kernel bound: the fp32 CPU evaluation of the same formula (attn_maps_ref.ref_token_maps(dtype=float32)) has a maximum error against float64;
the kernel's maximum error must stay within 8x that yardstick (its summation order and v_exp_f32 differ from libm by a few ulp)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import attn_maps_ref as R

pytestmark = pytest.mark.gpu
dev = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TB_EINVAL = -22
MARGIN = 8.0


def _operands(B, H, Sq, Skv, hd, seed, dtype):
    g = torch.Generator().manual_seed(seed)
    Q = torch.randn(B * Sq, H * hd, generator=g).to(dtype)
    K = torch.randn(B * Skv, H * hd, generator=g).to(dtype)
    return Q, K


def _yardstick(Q, K, B, H, Sq, Skv, hd, scale):
    """(float64 reference, max error of the fp32 evaluation against it)"""
    ref = R.ref_token_maps(Q, K, B, H, Sq, Skv, hd, scale)
    ref32 = R.ref_token_maps(Q, K, B, H, Sq, Skv, hd, scale, dtype=torch.float32)
    return ref, (ref32.double() - ref).abs().max().item()


CASES = [(2, 8, 64, 77, 40), (2, 5, 100, 77, 64), (1, 8, 36, 77, 160), (2, 2, 64, 33, 80), (2, 2, 96, 128, 64), (1, 1, 1, 1, 8)]


@pytest.mark.parametrize("half", ["fp16", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_kernel_matches_the_float64_reference(case, half):
    from textboost_amd import _lib as L
    from textboost_amd import ops
    B, H, Sq, Skv, hd = case
    with L.use_half(half):
        Q, K = _operands(B, H, Sq, Skv, hd, 7, L.half_dtype())
        scale = hd ** -0.5
        ref, yard = _yardstick(Q, K, B, H, Sq, Skv, hd, scale)
        maps = torch.full((B, Skv, Sq), float("nan"), device=dev)
        ops.attn_token_maps(Q.to(dev), K.to(dev), maps, B, H, Sq, Skv, hd, scale=scale, w=1.0 / H)
        got = maps.cpu().double()
    err = (got - ref).abs().max().item()
    sum_err = (got.sum(dim=1) - 1.0).abs().max().item()           # w * H = 1
    ratio = err / yard if yard > 0 else (0.0 if err == 0 else float("inf"))
    print(f"[attn maps] {half} {case}: kernel max err {err:.3e}, fp32 yardstick {yard:.3e}, ratio {ratio:.2f}; sum over keys off by {sum_err:.3e} "
          f"(ratio {sum_err / yard if yard > 0 else 0.0:.2f})")
    assert torch.isfinite(got).all()
    assert err <= MARGIN * yard, (err, yard)
    assert sum_err <= MARGIN * yard, (sum_err, yard)


@pytest.mark.parametrize("half", ["fp16", "bf16"])
def test_strided_operands_batch_offset_and_canaries(half):
    """K is a column slice of a wider buffer (ldk = 3 C + 16), Q has ldq = C + 4 (rows that are not 16-byte aligned: the 2-byte load path);
    b0 = 1, nb = 1 writes image 1 alone and nothing around `maps`"""
    from textboost_amd import _lib as L
    from textboost_amd import ops
    B, H, Sq, Skv, hd = 2, 2, 100, 77, 40
    C = H * hd
    with L.use_half(half):
        dt = L.half_dtype()
        Q, K = _operands(B, H, Sq, Skv, hd, 11, dt)
        g = torch.Generator().manual_seed(12)
        qbuf = (torch.randn(B * Sq, C + 4, generator=g) * 50).to(dt)
        kbuf = (torch.randn(B * Skv, 3 * C + 16, generator=g) * 50).to(dt)
        qbuf[:, :C] = Q
        kbuf[:, C:2 * C] = K
        qd, kd = qbuf.to(dev), kbuf.to(dev)
        qv, kv = qd[:, :C], kd[:, C:2 * C]
        assert qv.stride(0) == C + 4 and kv.stride(0) == 3 * C + 16
        scale = hd ** -0.5
        ref, yard = _yardstick(Q, K, B, H, Sq, Skv, hd, scale)
        pad, n = 64, Skv * Sq
        buf = torch.full((n + 2 * pad,), -7.0, device=dev)
        maps = buf[pad:pad + n].view(1, Skv, Sq)
        ops.attn_token_maps(qv, kv, maps, B, H, Sq, Skv, hd, scale=scale, b0=1, nb=1, w=1.0 / H)
        host = buf.cpu()
    assert (host[:pad] == -7.0).all() and (host[pad + n:] == -7.0).all()
    got = host[pad:pad + n].view(Skv, Sq).double()
    err = (got - ref[1]).abs().max().item()
    print(f"[attn maps] {half} strided, b0 = 1: max err {err:.3e}, yardstick {yard:.3e}")
    assert err <= MARGIN * yard
    assert (got - ref[0]).abs().max().item() > 100 * MARGIN * yard       # it is image 1, not image 0


def test_accumulate_adds_and_overwrite_ignores_old_contents():
    from textboost_amd import ops
    B, H, Sq, Skv, hd = 2, 5, 100, 77, 64
    Q, K = _operands(B, H, Sq, Skv, hd, 13, torch.float16)
    q, k = Q.to(dev), K.to(dev)
    once = torch.full((B, Skv, Sq), float("nan"), device=dev)
    ops.attn_token_maps(q, k, once, B, H, Sq, Skv, hd, w=0.3, accumulate=False)        # overwrites the NaNs
    assert torch.isfinite(once).all()
    twice = torch.zeros(B, Skv, Sq, device=dev)
    ops.attn_token_maps(q, k, twice, B, H, Sq, Skv, hd, w=0.3, accumulate=True)
    assert torch.equal(twice, once)
    ops.attn_token_maps(q, k, twice, B, H, Sq, Skv, hd, w=0.3, accumulate=True)
    assert torch.equal(twice, 2 * once)
    again = torch.empty_like(once)
    ops.attn_token_maps(q, k, again, B, H, Sq, Skv, hd, w=0.3)
    assert torch.equal(again, once)                                                     # launch to launch, bit for bit


@pytest.mark.parametrize("half", ["fp16", "bf16"])
def test_planted_token_lights_up_the_left_half(half):
    """an 8 x 8 map, 33 keys: left-half queries are 4 k* in every head (k* = 3 e_0: logit 4 * 9 * hd^-0.5 = 9 against 0 for every other key, so
    p* = e^9 / (e^9 + 32) > 0.99); all other queries and keys are unit vectors orthogonal to k* (their logits lie within +- hd^-0.5 = 0.25, so
    on the right half p* <= 1 / (1 + 32 e^-0.25) < 0.04)"""
    from textboost_amd import _lib as L
    from textboost_amd import ops
    B, H, Sq, Skv, hd, jstar = 1, 2, 64, 33, 16, 20
    g = torch.Generator().manual_seed(17)

    def unit(n):
        v = torch.randn(n, H, hd, generator=g)
        v[..., 0] = 0
        return v / v.norm(dim=-1, keepdim=True)
    kstar = torch.zeros(hd)
    kstar[0] = 3.0
    K = unit(Skv)
    K[jstar] = kstar
    Q = unit(Sq)
    left = (torch.arange(Sq) % 8) < 4
    Q[left] = 4 * kstar
    with L.use_half(half):
        dt = L.half_dtype()
        maps = torch.empty(1, Skv, Sq, device=dev)
        ops.attn_token_maps(Q.reshape(Sq, H * hd).to(dt).to(dev), K.reshape(Skv, H * hd).to(dt).to(dev), maps, B, H, Sq, Skv, hd, w=1.0 / H)
        m = maps[0, jstar].cpu().view(8, 8)
    print(f"[attn maps] {half} planted token: left min {m[:, :4].min():.4f}, right max {m[:, 4:].max():.4f}")
    assert (m[:, :4] > 0.9).all() and (m[:, 4:] < 0.1).all()


def test_refusals_launch_nothing():
    from textboost_amd import _lib as L
    from textboost_amd import ops

    def call(H, Sq, Skv, hd, dtype=torch.float16, b0=0, nb=1, accumulate=0):
        q = torch.zeros(Sq, H * hd, device=dev, dtype=dtype)
        k = torch.zeros(Skv, H * hd, device=dev, dtype=dtype)
        maps = torch.full((1, Skv, Sq), -3.0, device=dev)
        d = L.AttnDesc()
        d.B, d.H, d.Sq, d.Skv, d.hd, d.causal, d.scale = 1, H, Sq, Skv, hd, 0, hd ** -0.5
        d.Q, d.ldq, d.K, d.ldk = L.ptr(q), q.stride(0), L.ptr(k), k.stride(0)
        rc = L.lib().tb_attn_token_maps(d, ops._dt(q), b0, nb, 1.0, accumulate, L.ptr(maps), L.stream())
        torch.cuda.synchronize()
        return rc, maps
    with L.use_half("fp16"):
        for kw in (dict(H=2, Sq=16, Skv=129, hd=16), dict(H=2, Sq=16, Skv=8, hd=44), dict(H=2, Sq=16, Skv=8, hd=168),
                   dict(H=2, Sq=16, Skv=8, hd=16, dtype=torch.float32), dict(H=2, Sq=16, Skv=8, hd=16, b0=1), dict(H=2, Sq=16, Skv=8, hd=16, nb=2),
                   dict(H=2, Sq=16, Skv=8, hd=16, accumulate=2)):
            rc, maps = call(**kw)
            assert rc == TB_EINVAL, kw
            assert (maps == -3.0).all(), kw
        rc, maps = call(H=2, Sq=16, Skv=8, hd=16)
        assert rc == 0 and torch.allclose(maps, torch.full_like(maps, 2 / 8))      # zero operands: uniform over the 8 keys, two heads, w = 1
        q32 = torch.zeros(16, 32, device=dev)
        with pytest.raises(RuntimeError, match="tb_attn_token_maps"):
            ops.attn_token_maps(q32, torch.zeros(8, 32, device=dev), torch.zeros(1, 8, 16, device=dev), 1, 2, 16, 8, 16)


# ------------------------------------------------------------------------------------------------ UNet level
def _layer_refs(hip, rows):
    """{(h_l, w_l): (sum over that resolution's layers of the float64 reference on the executor's retained q2 / kv_all, sum of the layers' fp32
    yardsticks)} for the images `rows` = (b0, b1)"""
    from textboost_amd.attn_maps import cross_attention_maps
    nl = len(hip.geo.block_out_channels)
    kv_all = hip.kv_all.cpu()
    out = {hw: [0, 0.0] for hw in cross_attention_maps(hip)}
    for name, C in hip.xattn:
        block = name[:-len(".transformer_blocks.0.attn2")]
        part = block.split(".")
        level = nl - 1 if part[0] == "mid_block" else (int(part[1]) if part[0] == "down_blocks" else nl - 1 - int(part[1]))
        hw = (hip.H >> level, hip.W >> level)
        heads = hip.geo.heads(level)
        hd = C // heads
        q2 = hip._bufs[block + ".q2"].cpu()
        k2 = kv_all[:, hip.kv_off[name]: hip.kv_off[name] + C]
        ref, yard = _yardstick(q2, k2, hip.B, heads, hw[0] * hw[1], hip.T, hd, hd ** -0.5)
        out[hw][0] = out[hw][0] + ref[rows[0]:rows[1]]
        out[hw][1] += yard
    return out


def _check_against_layers(rec, hip, rows, what):
    """accumulator == sum of the layers' references, within the sum of the layers' kernel bounds (8 x the fp32 yardstick each) plus half an ulp
    of the running fp32 sum per accumulating launch"""
    for hw, (ref, yard) in _layer_refs(hip, rows).items():
        got = rec.acc[hw].cpu().double()
        n = rec.count[hw]
        bound = MARGIN * yard + n * 2.0 ** -24 * max(1.0, got.abs().max().item())
        err = (got - ref).abs().max().item()
        print(f"[attn maps] {what} {hw[0]}x{hw[1]}: {n} layers, max err {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (hw, err, bound)


def test_unet_records_every_cross_attention_and_the_prediction_is_unchanged():
    from tests.test_gpu_model import make_unet
    from textboost_amd.attn_maps import AttnMapRecorder, cross_attention_maps
    B, hw, D = 2, 16, 64
    _, hip, _ = make_unet(B, hw, D)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, 4, hw, hw, generator=g).half().to(dev)
    t = torch.tensor([17, 801], device=dev)
    ehs = torch.randn(B * 77, D, generator=g).half().to(dev)
    assert hip.attn_maps is None
    plain = hip.forward(x, t, ehs).clone()
    rec = AttnMapRecorder(hip, rows=(0, B))
    hip.attn_maps = rec
    try:
        pred = hip.forward(x, t, ehs).clone()
    finally:
        hip.attn_maps = None
    assert torch.equal(pred, plain)
    assert rec.count == cross_attention_maps(hip) and sum(rec.count.values()) == len(hip.xattn)
    _check_against_layers(rec, hip, (0, B), "tiny UNet")
    again = hip.forward(x, t, ehs)
    assert torch.equal(again, plain) and sum(rec.count.values()) == len(hip.xattn)      # off again: nothing recorded


# ------------------------------------------------------------------------------------------------ sampler level
@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    from tests.test_gpu_generate import D_TEXT, write_model_dir, write_trained_run
    from textboost_amd import generate as G
    root = tmp_path_factory.mktemp("attn_maps")
    mdir, rdir = str(root / "model"), str(root / "runs" / "dog")
    write_model_dir(mdir, hw=16)
    write_trained_run(rdir, ["<dog>"], ["<hflip>"], seed=1)
    B = 2
    with torch.no_grad():
        pipe = G.Pipeline.from_model_dir(mdir, B, steps=3, guidance=7.5, device=dev)
    g = torch.Generator().manual_seed(3)
    cond = torch.randn(B * 77, D_TEXT, generator=g).half().float().to(dev)
    uncond = torch.randn(B * 77, D_TEXT, generator=g).half().float().to(dev)
    lat = torch.cat([G.seeded_latent(s, 16) for s in (0, 1)]).to(dev)
    return dict(root=root, mdir=mdir, rdir=rdir, pipe=pipe, B=B, cond=cond, uncond=uncond, lat=lat)


def test_sampler_latents_unchanged_and_one_step_equals_the_unet_level_maps(tiny):
    from textboost_amd import _lib as L
    from textboost_amd.attn_maps import AttnMapRecorder
    from textboost_amd.sampler import HipSampler
    pipe, B = tiny["pipe"], tiny["B"]
    with torch.no_grad():
        plain = pipe.sampler.denoise(tiny["cond"], tiny["uncond"], latents=tiny["lat"]).clone()
        rec = AttnMapRecorder(pipe.unet)
        assert (rec.b0, rec.nb) == (B, B)
        with_maps = pipe.sampler.denoise(tiny["cond"], tiny["uncond"], latents=tiny["lat"], maps=rec).clone()
        assert torch.equal(with_maps, plain) and pipe.unet.attn_maps is None
        assert all(rec.count[hw] == 3 * n for hw, n in rec.layers.items())                # every step
        res = rec.result()
        assert res.shape == (B, 77, 16, 16) and res.dtype == torch.float32
        off = (res.sum(dim=1) - 1).abs().max().item()
        print(f"[attn maps] result() sums to 1 over the tokens within {off:.2e}")
        assert off <= 1e-4
        # one step: the recorder holds exactly what the UNet-level recorder holds for rows [B, 2B) of the step's forward
        one = HipSampler(pipe.unet, pipe.vae, steps=1, guidance=7.5)
        rec1 = AttnMapRecorder(pipe.unet)
        one.denoise(tiny["cond"], tiny["uncond"], latents=tiny["lat"], maps=rec1)
        x2 = torch.cat([tiny["lat"], tiny["lat"]]).to(L.half_dtype())
        ehs = torch.cat([tiny["uncond"], tiny["cond"]]).to(L.half_dtype()).contiguous()
        rec2 = AttnMapRecorder(pipe.unet, rows=(B, 2 * B))
        pipe.unet.attn_maps = rec2
        try:
            pipe.unet.forward(x2, one.t_dev[0], ehs)
        finally:
            pipe.unet.attn_maps = None
        assert rec1.count == rec2.count == rec1.layers
        for hw in rec1.acc:
            assert torch.equal(rec1.acc[hw], rec2.acc[hw]), hw
        _check_against_layers(rec2, pipe.unet, (B, 2 * B), "sampler step")


def test_captured_denoise_replays_bit_identical_maps(tiny):
    from textboost_amd.attn_maps import AttnMapRecorder
    from textboost_amd.sampler import HipSampler
    pipe = tiny["pipe"]
    with torch.no_grad():
        two = HipSampler(pipe.unet, pipe.vae, steps=2, guidance=7.5)
        rec = AttnMapRecorder(pipe.unet)
        eager_x = two.denoise(tiny["cond"], tiny["uncond"], latents=tiny["lat"], maps=rec).clone()      # also the warm-up: every buffer exists
        eager = {hw: a.clone() for hw, a in rec.acc.items()}
        counts = dict(rec.count)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):       # every launch goes to the one capturing stream: a chain
            out = two.denoise(tiny["cond"], tiny["uncond"], latents=tiny["lat"], maps=rec)
        assert rec.count == counts
        replays = []
        for _ in range(2):
            for a in rec.acc.values():
                a.fill_(float("nan"))                    # the captured zero() must clear this
            graph.replay()
            torch.cuda.synchronize()
            replays.append(({hw: a.clone() for hw, a in rec.acc.items()}, out.clone()))
    for hw in eager:
        assert torch.equal(replays[0][0][hw], replays[1][0][hw]) and torch.equal(replays[0][0][hw], eager[hw]), hw
    assert torch.equal(replays[0][1], eager_x) and torch.equal(replays[1][1], eager_x)


# ------------------------------------------------------------------------------------------------ the CLI
def test_cli_writes_maps_and_leaves_the_images_alone(tiny):
    pytest.importorskip("transformers")
    from PIL import Image
    inf = os.path.join(ROOT, "inference.py")
    outs = {}
    for flag in (False, True):
        wd = str(tiny["root"] / ("with" if flag else "without"))
        os.makedirs(wd)
        cmd = ["timeout", "-k", "10", "600", sys.executable, inf, tiny["rdir"], "--model", tiny["mdir"], "--prompt", "photo of a <dog> dog",
               "--seeds", "0", "1", "2", "--output", "g.jpg", "--steps", "2"] + (["--attn-map"] if flag else [])
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=wd)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        outs[flag] = wd
    assert open(os.path.join(outs[True], "g.jpg"), "rb").read() == open(os.path.join(outs[False], "g.jpg"), "rb").read()
    assert not os.path.exists(os.path.join(outs[False], "g_attn.jpg"))
    sheet = Image.open(os.path.join(outs[True], "g_attn.jpg"))
    assert sheet.size == (3 * 128, 1 * 128)                              # one word (the run's placeholder in the prompt) x three seeds
    z = np.load(os.path.join(outs[True], "g_attn.npz"))
    assert z["maps"].shape == (3, 1, 16, 16) and z["maps"].dtype == np.float32
    assert list(z["words"]) == ["<dog>"] and list(z["seeds"]) == [0, 1, 2]
    assert np.isfinite(z["maps"]).all() and (z["maps"] > 0).all() and (z["maps"] < 1).all()
    assert np.abs(z["maps"][0] - z["maps"][1]).max() > 0                 # different seeds, different maps
