"""Prompt-to-prompt LocalBlend on the GPU (inference.py --blend; csrc/local_blend.hip, `HipUNet.enable_blend`, `HipSampler.denoise(blend=...)`;
DESIGN.md 23): `tb_blend_mask` against the float32 definition of tests/blend_ref.py BYTE FOR BYTE (every step of the definition is exactly
reproducible in float32: no tolerance, no excluded cells; tests/test_blend_host.py holds that definition against the literal float64
formulation), `tb_dpm_step_local_blend` against `tb_dpm_step`'s bits plus an exact select, the recorder inside the tiny UNet, the sampler on
the tiny model directory of tests/test_gpu_generate.py, and the CLI in child processes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import attn_maps_ref as AR
import blend_ref as R

pytestmark = pytest.mark.gpu
dev = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TB_EINVAL = -22
PAD = 5
STEP = (7.5, 0.8, 0.6, 0.9, 0.3, -0.1)                                  # guidance, alpha_t, sigma_t, ca, cb, cc
STEP_SHAPES = [(4, 4, 16, 16), (2, 4, 8, 8), (2, 4, 5, 7), (2, 1, 1, 1)]  # tests/test_gpu_invert.py's, with an even batch; n_per_b = 1
ATTN_MARGIN = 8.0                                                       # tests/test_gpu_attn_maps.py's bound: 8 x the fp32 yardstick


class Guarded:
    """an operand in the middle of a buffer of canaries"""

    def __init__(self, t, canary=77):
        self.n, self.canary = t.numel(), canary
        self.buf = torch.full((self.n + 2 * PAD,), canary, dtype=t.dtype)
        self.buf[PAD:PAD + self.n] = t.reshape(-1)
        self.buf = self.buf.to(dev)
        self.t = self.buf[PAD:PAD + self.n].view(t.shape)

    def intact(self):
        b = self.buf.cpu()
        return bool((b[:PAD] == self.canary).all() and (b[PAD + self.n:] == self.canary).all())


# ------------------------------------------------------------------------------------------------ tb_blend_mask
def _mask_launch(acc, words, shape, th, limit=None, with_area=True):
    from textboost_amd import ops
    n, T, hl, wl, h, w = shape
    ag, wg = Guarded(torch.from_numpy(acc), canary=3.0), Guarded(torch.from_numpy(words), canary=1)
    mg = Guarded(torch.full((n, h * w), 9, dtype=torch.uint8), canary=77)
    rg = Guarded(torch.full((n,), -5, dtype=torch.int32), canary=77) if with_area else None
    lg = None if limit is None else Guarded(torch.from_numpy(limit), canary=1)
    ops.blend_mask(ag.t, wg.t, h, w, hl, wl, th, mg.t, limit=None if lg is None else lg.t, area=None if rg is None else rg.t)
    first = (mg.t.cpu().numpy().reshape(n, h, w).copy(), None if rg is None else rg.t.cpu().numpy().copy())
    ops.blend_mask(ag.t, wg.t, h, w, hl, wl, th, mg.t, limit=None if lg is None else lg.t, area=None if rg is None else rg.t)
    again = (mg.t.cpu().numpy().reshape(n, h, w), None if rg is None else rg.t.cpu().numpy())
    assert np.array_equal(first[0], again[0]) and (rg is None or np.array_equal(first[1], again[1]))       # a relaunch is bit-identical
    assert all(g.intact() for g in (ag, wg, mg) + ((rg,) if rg is not None else ()) + ((lg,) if lg is not None else ()))
    assert torch.equal(ag.t.cpu(), torch.from_numpy(acc)) and torch.equal(wg.t.cpu(), torch.from_numpy(words))
    return first


@pytest.mark.parametrize("half", ["fp16", "bf16"])
@pytest.mark.parametrize("shape,seed", R.CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_mask_kernel_gives_the_reference_bytes(shape, seed, half):
    from textboost_amd import _lib as L
    n, T, hl, wl, h, w = shape
    acc, words = R.make_case(shape, seed)                      # a multi-position word per row, a position outside [0, T)
    rng = np.random.RandomState(seed + 1)
    limit = (rng.uniform(size=h * w) < 0.6).astype(np.uint8) * 3
    single = R.make_case(shape, seed + 50, n_pos=1, multi=False)
    one_row = words.copy()
    one_row[n:] = -1                                            # the words occur in the source prompt only
    with L.use_half(half):
        for name, a, wd, th, lim, with_area in (("plain", acc, words, R.TH, None, True), ("limit", acc, words, R.TH, limit, True),
                                                ("no area", acc, words, R.TH, limit, False), ("n_pos 1", single[0], single[1], 0.5, None, True),
                                                ("source row only", acc, one_row, R.TH, None, True), ("th 0", acc, words, 0.0, None, True),
                                                ("th 1", acc, words, 1.0, None, True), ("th 2", acc, words, 2.0, limit, True),
                                                ("empty table", acc, np.full_like(words, -1), 0.0, None, True)):
            want, want_area = R.blend_mask(a, wd, hl, wl, h, w, th, limit=lim)
            got, got_area = _mask_launch(a, wd, shape, th, limit=lim, with_area=with_area)
            assert np.array_equal(got, want), (name, int((got != want).sum()))            # bytes, no tolerance
            assert not with_area or np.array_equal(got_area, want_area), name
            if name == "th 0":
                assert (got == 255).all()
            if name in ("th 1", "th 2", "empty table"):
                assert (got == 0).all() and (got_area == 0).all()
        print(f"[blend] mask {half} {shape}: area {R.blend_mask(acc, words, hl, wl, h, w, R.TH)[1].tolist()} of {h * w}")


@pytest.mark.parametrize("half", ["fp16", "bf16"])
def test_mask_kernel_constant_map_and_refusals_touch_nothing(half):
    from textboost_amd import _lib as L
    with L.use_half(half):
        _constant_map_and_refusals(L)


def _constant_map_and_refusals(L):
    shape = (2, 20, 4, 6, 8, 12)
    n, T, hl, wl, h, w = shape
    words = np.tile(np.array([[3, 1, -1, -1]], dtype=np.int32), (2 * n, 1))
    flat = np.full((2 * n, T, hl * wl), 0.125, dtype=np.float32)
    got, area = _mask_launch(flat, words, shape, 1.0)
    assert (got == 0).all() and (area == 0).all()              # the strict compare: P > 1 * mx never holds on a constant map
    got, area = _mask_launch(flat, words, shape, 0.999)
    assert (got == 255).all() and (area == h * w).all()
    acc, _ = R.make_case(shape, 7, n_pos=4)
    lib = L.lib()
    ag, wg = Guarded(torch.from_numpy(acc), 3.0), Guarded(torch.from_numpy(words), 1)
    mg, rg, lg = Guarded(torch.full((n, h * w), 9, dtype=torch.uint8)), Guarded(torch.full((n,), -5, dtype=torch.int32)), \
        Guarded(torch.ones(h * w, dtype=torch.uint8), 1)
    good = [L.ptr(ag.t), L.ptr(wg.t), n, T, hl, wl, h, w, 4, 0.3, L.ptr(lg.t), L.ptr(mg.t), L.ptr(rg.t), L.stream()]
    bads = [(0, None), (1, None), (11, None), (2, 0), (2, -1), (3, 1), (3, 129), (4, 0), (5, 0), (4, 3), (5, 5), (6, 0), (7, 0), (6, 9), (7, 13),
            (8, 0), (8, 17), (9, float("nan")), (9, float("inf")), (9, -float("inf"))]
    for k, v in bads:
        bad = list(good)
        bad[k] = v
        assert lib.tb_blend_mask(*bad) == TB_EINVAL, (k, v)
    bad = list(good)
    bad[4], bad[5], bad[6], bad[7] = 64, 64, 64, 64            # hl * wl = 4096 > 2048
    assert lib.tb_blend_mask(*bad) == TB_EINVAL
    torch.cuda.synchronize()
    assert (mg.t == 9).all() and (rg.t == -5).all() and mg.intact() and rg.intact()       # nothing was launched
    assert lib.tb_blend_mask(*good) == 0
    torch.cuda.synchronize()
    want, want_area = R.blend_mask(acc, words, hl, wl, h, w, 0.3)
    assert np.array_equal(mg.t.cpu().numpy().reshape(n, h, w), want) and np.array_equal(rg.t.cpu().numpy(), want_area)


# ------------------------------------------------------------------------------------------------ tb_dpm_step_local_blend
def _operands(shape, hd, seed=11):
    B, C, h, w = shape
    n = C * h * w
    g = torch.Generator().manual_seed(seed)
    x, mp = torch.randn(B, n, generator=g), torch.randn(B, n, generator=g)
    e = (torch.randn(2 * B, n, generator=g) * 0.8).to(hd)
    return B, n, h * w, C, x, mp, e, g


def _want(xs, x2s, mask, B, C):
    """tb_dpm_step's results + the select: edited row b takes source row b - B/2 where its pair's mask is zero"""
    n = B // 2
    keep = mask.bool().repeat(1, C)                             # [n, C * hw]: element j belongs to cell j % hw
    x = xs.clone()
    x[n:] = torch.where(keep, xs[n:], xs[:n])
    x2 = x2s.clone()
    for half in (0, B):
        x2[half + n:half + B] = torch.where(keep, x2s[half + n:half + B], x2s[half:half + n])
    return x, x2


@pytest.mark.parametrize("shape", STEP_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("half", ["fp16", "bf16"])
def test_step_kernel_is_dpm_step_plus_the_select(half, shape):
    from textboost_amd import _lib as L
    from textboost_amd import ops
    with L.use_half(half):
        hd = L.half_dtype()
        B, n, hw, C, x0, mp0, e, g = _operands(shape, hd)
        npair = B // 2
        xs, ms, x2s = x0.to(dev), mp0.to(dev), torch.zeros(2 * B, n, device=dev, dtype=hd)
        ops.dpm_step(xs, e.to(dev), ms, x2s, n, B, *STEP)
        cells = torch.arange(hw)
        checker = torch.stack([(((cells // shape[3] + cells % shape[3]) % 2) ^ (p % 2)) * (1 + 253 * (p % 2)) for p in range(npair)]).to(torch.uint8)
        rand = (torch.rand(npair, hw, generator=g) < 0.5).to(torch.uint8)
        cases = [("all 255", torch.full((npair, hw), 255, dtype=torch.uint8)), ("zeros", torch.zeros(npair, hw, dtype=torch.uint8)),
                 ("per-pair checkerboards", checker), ("random", rand)]
        eg = Guarded(e)
        for name, mask in cases:
            xg, mg, x2g, kg = Guarded(x0), Guarded(mp0), Guarded(torch.zeros(2 * B, n, dtype=hd)), Guarded(mask, 1)
            ops.dpm_step_local_blend(xg.t, eg.t, mg.t, x2g.t, n, B, *STEP, kg.t, hw)
            wx, wx2 = _want(xs, x2s, mask.to(dev), B, C)
            assert torch.equal(mg.t, ms), (name, "m_prev is every row's own unblended data prediction, tb_dpm_step's bits")
            assert torch.equal(xg.t, wx), (name, "the select is exact per element")
            assert torch.equal(x2g.t, wx2), (name, "x2: tb_dpm_step's bits of the row kept")
            assert torch.equal(xg.t[:npair], xs[:npair]) and torch.equal(x2g.t[:npair], x2s[:npair]), (name, "the source rows are tb_dpm_step's")
            assert all(t.intact() for t in (xg, mg, x2g, eg, kg)), name
            if name == "all 255":
                assert torch.equal(xg.t, xs) and torch.equal(x2g.t, x2s)                   # tb_dpm_step itself
            if name == "zeros":
                assert torch.equal(xg.t[npair:], xs[:npair]) and torch.equal(x2g.t[npair:B], x2s[:npair]) and torch.equal(x2g.t[B + npair:], x2s[B:B + npair])
            if name == "per-pair checkerboards" and hw > 1:
                assert 0 < int((xg.t[npair:] != xs[npair:]).sum()) < npair * n
                assert npair == 1 or not torch.equal(checker[0] != 0, checker[1] != 0)          # every pair reads its own mask
        # refusals: -22, nothing launched
        lib = L.lib()
        xg, mg, x2g, kg = Guarded(x0), Guarded(mp0), Guarded(torch.zeros(2 * B, n, dtype=hd)), Guarded(checker, 1)
        good = [L.ptr(xg.t), L.ptr(eg.t), L.ptr(mg.t), L.ptr(x2g.t), n, B, *STEP, L.ptr(kg.t), hw, L.stream()]
        bads = [(0, None), (1, None), (2, None), (3, None), (12, None), (4, 0), (4, -3), (5, 0), (5, -2), (5, B + 1), (5, 65536), (5, 65537), (7, 0.0),
                (13, 0), (13, -1), (13, n + 1)]
        for k, v in bads:
            bad = list(good)
            bad[k] = v
            assert lib.tb_dpm_step_local_blend(*bad) == TB_EINVAL, (k, v)
        torch.cuda.synchronize()
        assert torch.equal(xg.t.cpu(), x0) and torch.equal(mg.t.cpu(), mp0) and (x2g.t == 0).all()
        assert lib.tb_dpm_step_local_blend(*good) == 0
        torch.cuda.synchronize()


@pytest.mark.parametrize("half", ["fp16", "bf16"])
def test_step_kernel_carries_tb_dpm_step_s_x2_also_where_that_is_not_half_of_x(half):
    """Inputs with ties of the second rounding (tests/test_gpu_invert.py's second test): 2 x 65536 elements, about eight elements where
    tb_dpm_step's folded conversion differs from half(x) in the fp16 build, none in the bf16 build.  A kept element carries its own row's x2
    bits, a blended one the source row's -- never half(x) recomputed."""
    from textboost_amd import _lib as L
    from textboost_amd import ops
    with L.use_half(half):
        hd = L.half_dtype()
        B, n, hw, C, x0, mp0, e, g = _operands((2, 4, 128, 128), hd, seed=12)
        x0, mp0, e = (t.to(dev) for t in (x0, mp0, e))
        xs, ms, x2s = x0.clone(), mp0.clone(), torch.zeros(2 * B, n, device=dev, dtype=hd)
        ops.dpm_step(xs, e, ms, x2s, n, B, *STEP)
        ties = (x2s[:B] != xs.to(hd))
        print(f"[blend] step {half}: tb_dpm_step's x2 != half(x) on {int(ties.sum())} of {B * n} elements (source row {int(ties[0].sum())})")
        assert (int(ties.sum()) > 0) == (half == "fp16")
        for mask in (torch.zeros(1, hw, dtype=torch.uint8), torch.full((1, hw), 255, dtype=torch.uint8),
                     (torch.rand(1, hw, generator=g) < 0.5).to(torch.uint8)):
            xp, mq, x2p = x0.clone(), mp0.clone(), torch.zeros(2 * B, n, device=dev, dtype=hd)
            ops.dpm_step_local_blend(xp, e, mq, x2p, n, B, *STEP, mask.to(dev), hw)
            wx, wx2 = _want(xs, x2s, mask.to(dev), B, C)
            assert torch.equal(xp, wx) and torch.equal(mq, ms) and torch.equal(x2p, wx2)


# ------------------------------------------------------------------------------------------------ UNet level
def _plan77():
    from tests.test_p2p_host import StubTokenizer
    from textboost_amd import p2p
    return p2p.plan(StubTokenizer(), "a dog on a beach", "a fluffy <dog> dog on a beach", 77, (("fluffy", 2.0),))


@pytest.mark.parametrize("n", [1, 2])
def test_unet_records_the_conditional_rows_level_2_maps_and_changes_no_bit(n):
    from tests.test_gpu_model import make_unet
    from textboost_amd.p2p import P2PControl
    B, hw, D, T = 4 * n, 16, 64, 77
    _, hip, _ = make_unet(B, hw, D)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(B, 4, hw, hw, generator=g).half().to(dev)
    t = torch.full((B,), 17, device=dev)
    ehs = torch.randn(B * T, D, generator=g).half().to(dev)
    ctl = P2PControl.for_unet(hip, _plan77())
    blocks = [name[:-len(".transformer_blocks.0.attn2")] for name, _ in hip.xattn]

    def forward():
        ctl.reset()
        ctl.cross_active = ctl.self_active = True
        hip.p2p = ctl
        try:
            pred = hip.forward(x, t, ehs).clone()
        finally:
            hip.p2p = None
        return pred, {b: (hip._bufs[b + ".o1"].clone(), hip._bufs[b + ".o2"].clone()) for b in blocks}
    assert hip.blend is None
    plain, plain_o = forward()
    bl = hip.enable_blend()
    assert hip.blend is bl and not bl.record and (bl.b0, bl.nb, bl.h, bl.w) == (2 * n, 2 * n, 4, 4) and tuple(bl.acc.shape) == (2 * n, T, 16)
    idle, _ = forward()                                            # enabled but not recording: nothing is launched
    assert torch.equal(idle, plain) and (bl.acc == 0).all()
    bl.record = True
    try:
        pred, o = forward()
    finally:
        bl.record = False
    assert torch.equal(pred, plain)                                # the prediction, o1 and o2 carry the bits of the forward without blend
    assert all(torch.equal(o[b][0], plain_o[b][0]) and torch.equal(o[b][1], plain_o[b][1]) for b in blocks)
    # the accumulator against the float64 sum over the level-2 layers, from the recorded q / k (each row's own uncontrolled softmax)
    kv_all = hip.kv_all.cpu()
    ref64 = torch.zeros(2 * n, T, 16, dtype=torch.float64)
    ref32 = torch.zeros(2 * n, T, 16, dtype=torch.float32)
    layers = [(name, C) for name, C in hip.xattn if name in bl.layers]
    assert len(layers) == bl.n >= 2
    for name, C in layers:
        block = name[:-len(".transformer_blocks.0.attn2")]
        heads = hip.geo.heads(2)
        hd = C // heads
        q2 = hip._bufs[block + ".q2"].cpu()[2 * n * 16:]
        ko = hip.kv_off[name]
        k2 = kv_all[2 * n * T:, ko:ko + C].contiguous()
        ref64 += AR.ref_token_maps(q2, k2, 2 * n, heads, 16, T, hd, hd ** -0.5) / len(layers)
        ref32 += AR.ref_token_maps(q2, k2, 2 * n, heads, 16, T, hd, hd ** -0.5, dtype=torch.float32) / len(layers)
    yard = (ref32.double() - ref64).abs().max().item()
    err = (bl.acc.cpu().double() - ref64).abs().max().item()
    print(f"[blend] tiny UNet n {n}: accumulator max err {err:.3e}, fp32 yardstick {yard:.3e}, ratio {err / yard:.2f} ({len(layers)} layers)")
    assert err <= ATTN_MARGIN * yard, (err, yard)
    # the mean over heads and layers of a softmax sums to 1 over the T tokens; each entry is <= 1 and carries a few fp32 roundings
    assert (bl.acc.cpu().double().sum(dim=1) - 1.0).abs().max().item() <= T * 2.0 ** -22
    hip.blend = None
    after, _ = forward()
    assert torch.equal(after, plain)
    # a truncated forward (Attend-and-Excite's) does not record, even with the flag set
    hip.enable_excite()
    bl.acc.zero_()
    hip.blend, bl.record = bl, True
    try:
        assert hip.forward(x, t, ehs, until="excite") is None and (bl.acc == 0).all()
    finally:
        hip.blend, bl.record = None, False


# ------------------------------------------------------------------------------------------------ sampler level
STEPS = 4


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    from safetensors.torch import load_file, save_file
    from tests.test_compose_host import write_run
    from tests.test_gpu_generate import D_TEXT, write_model_dir
    from textboost_amd import generate as G
    from textboost_amd import models
    from textboost_amd.local_blend import BlendControl
    from textboost_amd.p2p import P2PControl
    from textboost_amd.vae import VAEGeometry, vae_encoder_shapes
    root = tmp_path_factory.mktemp("blend")
    mdir, rdir = str(root / "model"), str(root / "runs" / "dog")
    write_model_dir(mdir, hw=16)
    vfile = os.path.join(mdir, "vae", "diffusion_pytorch_model.safetensors")      # the CLI encodes the photo: add the encoder half
    vgeo = VAEGeometry(block_out_channels=(64, 64, 128, 128), layers_per_block=1)
    enc_sd = {k: v.half().float() for k, v in models.random_state_dict(vae_encoder_shapes(vgeo), 15, device="cpu").items()}
    save_file({**load_file(vfile), **enc_sd}, vfile)
    write_run(rdir, ["<dog>"], ["<hflip>"], seed=1, rank=4, keep_rows="even")
    B = 4                                                             # two seeds: source rows 0, 1 and edited rows 2, 3
    with torch.no_grad():
        pipe = G.Pipeline.from_model_dir(mdir, B, steps=STEPS, guidance=7.5, device=dev)
    g = torch.Generator().manual_seed(3)
    cond = torch.randn(B * 77, D_TEXT, generator=g).half().float().to(dev)
    uncond = torch.randn(77, D_TEXT, generator=g).half().float().repeat(B, 1).to(dev)
    lat = torch.cat([G.seeded_latent(s, 16) for s in (0, 1)] * 2).to(dev)
    ctl = P2PControl.for_unet(pipe.unet, _plan77(), cross_steps=0.75, self_steps=0.5)

    def blend(start, th, **kw):
        return BlendControl(pipe.unet, [2, 5], [4, 3, 7], start=start, threshold=th, **kw)      # (positions of the two prompts' own words)
    with torch.no_grad():
        plain = pipe.sampler.denoise(cond, uncond, latents=lat).clone()                          # computed once, shared, never written
        p2p = pipe.sampler.denoise(cond, uncond, latents=lat, p2p=ctl).clone()
    return dict(root=root, mdir=mdir, rdir=rdir, pipe=pipe, B=B, cond=cond, uncond=uncond, lat=lat, ctl=ctl, blend=blend, plain=plain, p2p=p2p)


def test_sampler_blend_limits_are_the_unblended_edit_and_the_source(tiny):
    smp, ctl, lat = tiny["pipe"].sampler, tiny["ctl"], tiny["lat"]
    args = (tiny["cond"], tiny["uncond"])
    with torch.no_grad():
        never = tiny["blend"](1.0, 0.3)
        x = smp.denoise(*args, latents=lat, p2p=ctl, blend=never).clone()
        assert torch.equal(x, tiny["p2p"]) and never.final_mask is None and never.area is None      # start = 1: denoise(p2p=)'s bits
        assert tiny["pipe"].unet.blend is None and tiny["pipe"].unet.p2p is None
        every = tiny["blend"](0.0, 0.0)
        x = smp.denoise(*args, latents=lat, p2p=ctl, blend=every).clone()
        assert torch.equal(x, tiny["p2p"])                                          # th = 0 from step 0: every cell keeps the edit
        assert (every.final_mask == 255).all() and every.area.tolist() == [256, 256]
        none = tiny["blend"](0.0, 2.0)
        x = smp.denoise(*args, latents=lat, p2p=ctl, blend=none).clone()
        assert torch.equal(x[2:], x[:2]) and torch.equal(x[:2], tiny["p2p"][:2])    # th = 2: the edited rows ARE the source rows, bit for bit
        assert (none.final_mask == 0).all() and none.area.tolist() == [0, 0]
        assert not torch.equal(tiny["p2p"][2:], tiny["p2p"][:2])
        # the plain denoise afterwards carries the bits it carried before
        assert torch.equal(smp.denoise(*args, latents=lat), tiny["plain"]) and tiny["pipe"].unet.blend is None
        assert torch.equal(smp.denoise(*args, latents=lat, p2p=ctl), tiny["p2p"])


def _peak_threshold(acc, table, row):
    """a threshold between the two largest distinct values of P / mx of `row`: that row's bits are then set on the cells whose window holds
    its maximum and on no other -- a mask that is neither empty nor full, whatever the weights (on the tiny random model the attention
    is nearly flat, and the published 0.3 keeps every cell)"""
    P, mx = R.row_maps(acc.cpu().numpy(), table.cpu().numpy(), 4, 4)
    v = np.unique(P[row].astype(np.float64) / float(mx[row]))
    assert len(v) >= 2 and v[-1] == 1.0
    return float(0.5 * (v[-1] + v[-2]))


def _replay(tiny, bctl, first, th, what):
    """`denoise(p2p=, blend=bctl)` against the same forwards, `ops.dpm_step` and a select with the kept masks, bit for bit; each kept
    mask against the reference mask of the accumulator read back at that step.  -> (the final latents, how many kept masks were neither
    empty nor full)"""
    from textboost_amd import _lib as L
    from textboost_amd import ops
    from textboost_amd.p2p import steps_for
    smp, ctl, lat, B = tiny["pipe"].sampler, tiny["ctl"], tiny["lat"], tiny["B"]
    unet = tiny["pipe"].unet
    n = B // 2
    bctl.keep_masks = True
    x = smp.denoise(tiny["cond"], tiny["uncond"], latents=lat, p2p=ctl, blend=bctl).clone()
    masks = bctl.masks.clone()
    assert tuple(masks.shape) == (STEPS, n, 16, 16) and (masks[:first] == 0).all() and torch.equal(masks[-1], bctl.final_mask)
    assert torch.equal(x[:n], tiny["p2p"][:n]) and torch.isfinite(x).all()          # the source rows: the unblended run's bits
    area = bctl.area.tolist()
    print(f"[blend] sampler {what}: final areas {area} of 256, per step {[int((m != 0).sum()) for m in masks]}")
    assert area == [int((m != 0).sum()) for m in masks[-1]]
    bl = smp.blend_buffers
    ehs = torch.cat([tiny["uncond"], tiny["cond"]]).to(L.half_dtype()).contiguous()
    cross, self_ = steps_for(ctl.cross_steps, STEPS), steps_for(ctl.self_steps, STEPS)
    ctl.reset()
    smp.x.copy_(lat)
    smp.m_prev.zero_()
    smp.x2[:B].copy_(smp.x)
    smp.x2[B:].copy_(smp.x)
    bl.acc.zero_()
    npb = smp.x[0].numel()
    nontrivial = 0
    for i in range(STEPS):
        unet.blend, bl.record = bl, True
        try:
            eps2 = smp.forward_step(i, ehs, ctl, i < cross, i < self_)
        finally:
            unet.blend, bl.record = None, False
        ops.dpm_step(smp.x, eps2, smp.m_prev, smp.x2, npb, B, smp.g, *smp.sch.data_prediction_scalars(i), *smp.sch.coefficients(i))
        if i >= first:
            want, _ = R.blend_mask(bl.acc.cpu().numpy(), bctl.table.cpu().numpy(), 4, 4, 16, 16, th)
            assert np.array_equal(masks[i].cpu().numpy(), want), (what, i)           # each kept mask: the reference of that step's accumulator
            nontrivial += sum(int(0 < int((m != 0).sum()) < m.size) for m in want)
            keep = masks[i].bool()[:, None].expand(n, 4, 16, 16)
            smp.x[n:] = torch.where(keep, smp.x[n:], smp.x[:n])
            for half in (0, B):
                smp.x2[half + n:half + B] = torch.where(keep, smp.x2[half + n:half + B], smp.x2[half:half + n])
    assert torch.equal(smp.x, x), what                                               # bit for bit
    return x, nontrivial


def test_sampler_blend_equals_the_by_hand_replay_and_its_masks_the_reference(tiny):
    from textboost_amd.local_blend import BlendControl
    smp, lat = tiny["pipe"].sampler, tiny["lat"]
    unet = tiny["pipe"].unet
    n = tiny["B"] // 2
    with torch.no_grad():
        _replay(tiny, tiny["blend"](0.25, 0.3), 1, 0.3, "th 0.3, start 0.25")      # floor(0.25 * 4) = 1
        # The same with masks that are certainly partial: the words occur in the source prompt only (the source rows' maps do not depend
        # on the blend), and the threshold isolates the peak of pair 0's final source map.
        final = smp.blend_buffers.acc.clone()
        th = _peak_threshold(final, tiny["blend"](0.25, 0.3).table, 0)
        src_only = BlendControl(unet, [2, 5], [], start=0.25, threshold=th)
        x, nontrivial = _replay(tiny, src_only, 1, th, f"source words only, th {th:.6f}")
        assert nontrivial > 0 and not torch.equal(x[n], tiny["p2p"][n]) and not torch.equal(x[n], x[0])
        assert torch.equal(smp.denoise(tiny["cond"], tiny["uncond"], latents=lat), tiny["plain"]) and unet.blend is None


def test_sampler_refusals_leave_no_state(tiny):
    from textboost_amd.attn_maps import AttnMapRecorder
    from textboost_amd.local_blend import BlendControl, BlendError
    smp, ctl, lat = tiny["pipe"].sampler, tiny["ctl"], tiny["lat"]
    unet = tiny["pipe"].unet
    args = (tiny["cond"], tiny["uncond"])
    with torch.no_grad():
        smp.denoise(*args, latents=lat)
        state = [t.clone() for t in (smp.x, smp.m_prev, smp.x2)]
        ok = tiny["blend"](0.25, 0.3)
        for kw, match in ((dict(blend=ok), "blend without p2p"), (dict(blend=ok, p2p=ctl, maps=AttnMapRecorder(unet)), "does not go with maps"),
                          (dict(blend=ok, p2p=ctl, regions=object()), "does not go with regions"),
                          (dict(blend=ok, p2p=ctl, excite=object()), "does not go with excite")):
            with pytest.raises(ValueError, match=match):
                smp.denoise(*args, latents=lat, **kw)
        bad = tiny["blend"](0.25, 0.3)
        bad.start = 1.5
        with pytest.raises(BlendError, match="--blend-start 1.5"):
            smp.denoise(*args, latents=lat, p2p=ctl, blend=bad)
        for kw in (dict(start=-0.1), dict(threshold=float("nan")), dict(threshold=-1.0)):
            with pytest.raises(BlendError):
                BlendControl(unet, [1], [1], **kw)
        other = tiny["blend"](0.25, 0.3)
        other.T = 20
        with pytest.raises(ValueError, match="control is built for"):
            smp.denoise(*args, latents=lat, p2p=ctl, blend=other)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(state, (smp.x, smp.m_prev, smp.x2)))      # nothing was touched
        assert unet.blend is None and unet.p2p is None
        assert torch.equal(smp.denoise(*args, latents=lat), tiny["plain"])


def test_pinned_blend_keeps_the_photo_outside_the_masks(tiny):
    from textboost_amd import generate as G
    from textboost_amd.local_blend import BlendControl
    from textboost_amd.p2p import P2PControl
    with torch.no_grad():
        pipe = G.Pipeline.from_model_dir(tiny["mdir"], 2, steps=STEPS, guidance=7.5, device=dev)
        smp = pipe.sampler
        cond, uncond = tiny["cond"][:2 * 77].contiguous(), tiny["uncond"][:2 * 77].contiguous()
        g = torch.Generator().manual_seed(5)
        z0 = (torch.randn(1, 4, 16, 16, generator=g) * 0.9).to(dev)
        ctl = P2PControl.for_unet(pipe.unet, _plan77(), cross_steps=0.75, self_steps=0.5)
        traj = smp.invert(cond, uncond, z0).clone()
        pin = traj[:, 0]
        unblended = smp.denoise(cond, uncond, p2p=ctl, pin=pin).clone()
        first = BlendControl(pipe.unet, [2, 5], [4, 3, 7], start=0.25, threshold=0.3)
        x = smp.denoise(cond, uncond, p2p=ctl, pin=pin, blend=first).clone()
        m = first.final_mask[0].bool()
        print(f"[blend] pinned, th 0.3: final area {first.area.tolist()} of 256")
        assert torch.equal(x[0], z0[0]) and torch.equal(x[1][:, ~m], z0[0][:, ~m]) and torch.isfinite(x).all()
        # a mask that is certainly partial: the words in the source prompt only, the threshold at the peak of the photo's own final map
        # (the source row is pinned: its maps do not depend on the blend)
        th = _peak_threshold(smp.blend_buffers.acc.clone(), first.table, 0)
        bctl = BlendControl(pipe.unet, [2, 5], [], start=0.25, threshold=th)
        x = smp.denoise(cond, uncond, p2p=ctl, pin=pin, blend=bctl).clone()
        m = bctl.final_mask[0].bool()
        print(f"[blend] pinned, th {th:.6f}: final area {bctl.area.tolist()} of 256")
        assert torch.equal(x[0], z0[0])                                              # row 0 is z0, bit for bit
        assert torch.equal(x[1][:, ~m], z0[0][:, ~m]) and torch.isfinite(x).all()    # outside the blend mask the edited row is z0
        assert 0 < int(m.sum()) < 256 and not torch.equal(x[1][:, m], z0[0][:, m])
        pmask = torch.zeros(16, 16, dtype=torch.uint8)
        pmask[2:13, 3:12] = 1
        pm = pmask.bool().to(dev)
        bctl2 = BlendControl(pipe.unet, [2, 5], [], start=0.25, threshold=th)
        xm = smp.denoise(cond, uncond, p2p=ctl, pin=pin, pin_mask=pmask.to(dev), blend=bctl2).clone()
        m2 = bctl2.final_mask[0].bool()
        assert torch.equal(xm[0], z0[0]) and torch.equal(xm[1][:, ~pm], z0[0][:, ~pm])       # outside pin_mask, row 1 is z0
        assert torch.equal(m2, m & pm) and torch.equal(xm[1][:, ~m2], z0[0][:, ~m2]) and int(m2.sum()) == bctl2.area.item()
        nothing = BlendControl(pipe.unet, [2, 5], [4, 3, 7], start=0.0, threshold=2.0)
        xz = smp.denoise(cond, uncond, p2p=ctl, pin=pin, blend=nothing)
        assert torch.equal(xz[1], z0[0]) and torch.equal(xz[0], z0[0])
        with pytest.raises(ValueError, match="one pair"):
            tiny["pipe"].sampler.denoise(tiny["cond"], tiny["uncond"], p2p=tiny["ctl"], pin=pin, blend=tiny["blend"](0.25, 0.3))
        assert torch.equal(smp.denoise(cond, uncond, p2p=ctl, pin=pin), unblended) and pipe.unet.blend is None


def test_captured_blended_denoise_replays_bit_identically(tiny):
    smp, ctl, lat = tiny["pipe"].sampler, tiny["ctl"], tiny["lat"]
    args = (tiny["cond"], tiny["uncond"])
    with torch.no_grad():
        bctl = tiny["blend"](0.25, 0.3)
        eager = smp.denoise(*args, latents=lat, p2p=ctl, blend=bctl).clone()          # also the warm-up: every buffer exists
        eager_mask, eager_area = bctl.final_mask.clone(), bctl.area.clone()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):             # every launch goes to the one capturing stream: a chain
            out = smp.denoise(*args, latents=lat, p2p=ctl, blend=bctl)
        for _ in range(2):
            out.fill_(float("nan"))
            bctl.final_mask.fill_(7)
            bctl.area.fill_(-1)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, eager) and torch.equal(bctl.final_mask, eager_mask) and torch.equal(bctl.area, eager_area)


# ------------------------------------------------------------------------------------------------ the CLI
def _child(cmd, cwd):
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, os.path.join(ROOT, "inference.py")] + cmd, capture_output=True, text=True, cwd=cwd)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def test_cli_blend_writes_the_grid_the_masks_and_the_report(tiny):
    pytest.importorskip("transformers")
    from PIL import Image
    common = [tiny["rdir"], "--model", tiny["mdir"], "--prompt", "a dog on a beach", "--edit-prompt", "a fluffy <dog> dog on a beach",
              "--seeds", "0", "1", "--steps", "3", "--output", "g.png", "--blend", "dog", "<dog>"]
    wds, outs = {}, {}
    for name, extra in (("blend", []), ("blend2", []), ("th2", ["--blend-threshold", "2"])):
        wds[name] = str(tiny["root"] / name)
        os.makedirs(wds[name])
        outs[name] = _child(common + extra, wds[name])
    files = ("g.png", "g_blend.png", "g_blend.json")
    for f in files:
        assert _read(os.path.join(wds["blend"], f)) == _read(os.path.join(wds["blend2"], f)), f       # two runs: byte-identical
    grid = np.asarray(Image.open(os.path.join(wds["blend"], "g.png"))).astype(int)
    assert grid.shape == (2 * 128, 2 * 128, 3)                       # the source row on top, the edited row below, one column per seed
    sheet = np.asarray(Image.open(os.path.join(wds["blend"], "g_blend.png")))
    assert sheet.shape == (128, 2 * 128) and set(np.unique(sheet)) <= {0, 255}
    with open(os.path.join(wds["blend"], "g_blend.json")) as f:
        rep = json.load(f)
    assert rep["words"] == ["dog", "<dog>"] and rep["positions"]["<dog>"]["source"] == [] and rep["positions"]["<dog>"]["edit"]
    assert rep["positions"]["dog"]["source"] and rep["start"] == 0.2 and rep["threshold"] == 0.3 and len(rep["area"]) == 2
    assert rep["area"] == [int((sheet[:, k * 128:(k + 1) * 128] != 0).sum()) // 64 for k in range(2)]      # nearest x 8: 64 pixels per cell
    print(f"[blend] inference.py: areas {rep['area']} of {rep['cells']} cells")
    t2 = np.asarray(Image.open(os.path.join(wds["th2"], "g.png"))).astype(int)
    assert np.array_equal(t2[128:], t2[:128]) and np.array_equal(t2[:128], grid[:128])       # threshold 2: the bottom row IS the top row
    assert "warning: --blend: the final mask of seed 0 is empty" in outs["th2"]              # a printed warning, not an error
    with open(os.path.join(wds["th2"], "g_blend.json")) as f:
        assert json.load(f)["area"] == [0, 0]


def test_cli_blend_with_an_inverted_photo(tiny):
    pytest.importorskip("transformers")
    from PIL import Image
    from tests.test_gpu_edit import _photo
    root = tiny["root"]
    photo = str(root / "photo.png")
    Image.fromarray(_photo()).save(photo)
    common = [tiny["rdir"], "--model", tiny["mdir"], "--prompt", "a dog on a beach", "--edit-prompt", "a fluffy <dog> dog on a beach",
              "--invert-image", photo, "--steps", "3", "--output", "g.png", "--blend", "dog", "<dog>"]
    wds = {}
    for name, extra in (("inv", []), ("inv2", []), ("inv_th2", ["--blend-threshold", "2"])):
        wds[name] = str(root / name)
        os.makedirs(wds[name])
        _child(common + extra, wds[name])
    for f in ("g.png", "g_blend.png", "g_blend.json"):
        assert _read(os.path.join(wds["inv"], f)) == _read(os.path.join(wds["inv2"], f)), f
    img = {k: np.asarray(Image.open(os.path.join(v, "g.png"))).astype(int) for k, v in wds.items()}
    assert img["inv"].shape == (2 * 128, 128, 3) and np.array_equal(img["inv"][:128], img["inv_th2"][:128])
    assert np.array_equal(img["inv_th2"][128:], img["inv_th2"][:128])               # threshold 2: the edit is the photo's round trip
    sheet = np.asarray(Image.open(os.path.join(wds["inv"], "g_blend.png")))
    assert sheet.shape == (128, 128)
    with open(os.path.join(wds["inv"], "g_blend.json")) as f:
        rep = json.load(f)
    assert rep["seeds"] == ["inv"] and rep["area"] == [int((sheet != 0).sum()) // 64]
