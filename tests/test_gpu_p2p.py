"""Prompt-to-prompt editing on the GPU: the two-term kernel (csrc/p2p_attn.hip) against the float64 references of tests/p2p_ref.py, the
`HipUNet.p2p` hook, `HipSampler.denoise(p2p=...)` and `inference.py --edit-prompt`.

Bounds (the project's own attention bounds, none derived from this kernel's output): O rel-L2 against float64 on the rounded operands <= 2e-3
in fp16 (tests/test_gpu_norm_attn.py) and <= 1.2e-2 in bf16 (tests/test_gpu_bf16.py); tests/test_gpu_regions.py reuses both.  For independent
N(0, 1) operands the two terms do not cancel: their errors add in quadrature as their norms do, so the relative error of the sum is a term's.
In the UNet the values V1 / V2 are rounded once more to fp16 (relative 2^-11 / sqrt(3) ~ 3e-4 per element, in quadrature with the kernel's
error): still inside 2e-3."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import p2p_ref as R

pytestmark = pytest.mark.gpu
dev = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TB_EINVAL = -22
O_BOUND = {"fp16": 2e-3, "bf16": 1.2e-2}

# (B, H, Sq, Skv1, Skv2, hd)
CASES = [(2, 8, 64, 77, 77, 40), (2, 5, 100, 77, 77, 64), (1, 8, 36, 77, 77, 160), (2, 2, 64, 33, 128, 80), (1, 1, 1, 1, 1, 8)]
BIG = [(8, 8, 2100, 77, 77, 40), (8, 8, 1900, 77, 77, 80)]


def _operands(B, H, Sq, Skv1, Skv2, hd, seed, dtype):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(B * n, H * hd, generator=g).to(dtype) for n in (Sq, Skv1, Skv1, Sq, Skv2, Skv2))


def _launch(ops_, B, H, Sq, Skv1, Skv2, hd, scale=None, single=False):
    from textboost_amd import ops
    Q1, K1, V1, Q2, K2, V2 = (t.to(dev) for t in ops_)
    o = torch.full((B * Sq, H * hd), float("nan"), device=dev, dtype=Q1.dtype)
    ops.attention_dual_fwd(Q1, K1, V1, None if single else Q2, K2, V2, o, B, H, Sq, Skv1, Skv2, hd, scale=scale)
    return o.cpu()


@pytest.mark.parametrize("half", ["fp16", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_dual_kernel_matches_the_float64_reference_and_repeats(case, half):
    from textboost_amd import _lib as L
    B, H, Sq, Skv1, Skv2, hd = case
    with L.use_half(half):
        x = _operands(*case, 31, L.half_dtype())
        o = _launch(x, *case)
        o2 = _launch(x, *case)
    ref = R.ref_dual_attention(*x, B, H, Sq, Skv1, Skv2, hd, hd ** -0.5)
    err = R.rel_l2(o, ref)
    print(f"[p2p] {half} {case}: O rel-L2 {err:.3e} (bound {O_BOUND[half]:.1e})")
    assert torch.isfinite(o.float()).all() and err <= O_BOUND[half], err
    assert torch.equal(o, o2)


@pytest.mark.parametrize("half", ["fp16", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_single_term_matches_plain_attention(case, half):
    from textboost_amd import _lib as L
    from textboost_amd import ops
    B, H, Sq, Skv1, Skv2, hd = case
    with L.use_half(half):
        x = _operands(*case, 32, L.half_dtype())
        o = _launch(x, *case, single=True)
        Q, K, V = (t.to(dev) for t in x[:3])
        plain = torch.full((B * Sq, H * hd), float("nan"), device=dev, dtype=Q.dtype)
        lse = torch.empty(B, H, Sq, device=dev)
        ops.attention_fwd(Q, K, V, plain, lse, B, H, Sq, Skv1, hd)
        plain = plain.cpu()
    ref = R.ref_attention(*x[:3], B, H, Sq, Skv1, hd, hd ** -0.5)
    err, vs = R.rel_l2(o, ref), R.rel_l2(o, plain)
    print(f"[p2p] {half} {case} single term: O rel-L2 {err:.3e}, against ops.attention_fwd {vs:.3e} (bound {O_BOUND[half]:.1e})")
    assert err <= O_BOUND[half] and vs <= O_BOUND[half], (err, vs)


@pytest.mark.parametrize("half", ["fp16", "bf16"])
@pytest.mark.parametrize("case", BIG, ids=lambda c: "x".join(map(str, c)))
def test_generation_sized_launches(case, half):
    """many workgroups per (batch, head), a ragged last block (Sq % 128 != 0, Sq % 32 != 0) and the XCD remap ((bands * B) % 8 == 0)"""
    from textboost_amd import _lib as L
    B, H, Sq, Skv1, Skv2, hd = case
    assert Sq % 128 != 0 and Sq % 32 != 0 and (-(-Sq // 128) * B) % 8 == 0
    with L.use_half(half):
        x = _operands(*case, 33, L.half_dtype())
        o = _launch(x, *case)
        o2 = _launch(x, *case)
    ref = R.ref_dual_attention(*x, B, H, Sq, Skv1, Skv2, hd, hd ** -0.5)
    C = H * hd
    err = R.rel_l2(o, ref)
    # per 128-query slice (one workgroup's rows of every batch row and head): a fault in one block index must not hide in the sum.  The
    # bound is the whole output's: the error is per-element rounding everywhere, and a slice from the wrong rows is off by order 1.
    worst = max(R.rel_l2(o.view(B, Sq, C)[:, s0:s0 + 128], ref.view(B, Sq, C)[:, s0:s0 + 128]) for s0 in range(0, Sq, 128))
    print(f"[p2p] {half} {case}: O rel-L2 {err:.3e}, worst 128-query slice {worst:.3e} (bound {O_BOUND[half]:.1e})")
    assert torch.isfinite(o.float()).all() and err <= O_BOUND[half] and worst <= O_BOUND[half], (err, worst)
    assert torch.equal(o, o2)


def test_strided_row_unaligned_operands_with_canaries():
    """Q1 and Q2 are row slices of ONE buffer (as in the UNet), every leading dimension is odd and every pointer 2-byte aligned only: the
    2-byte instance.  Nothing around O is written."""
    from textboost_amd import ops
    B, H, Sq, Skv1, Skv2, hd = 2, 3, 70, 77, 50, 24
    C = H * hd
    g = torch.Generator().manual_seed(34)

    def strided(rows, ld, off):
        buf = torch.randn(rows * ld + off + 8, generator=g).half().to(dev)
        return buf, buf[off:off + rows * ld].view(rows, ld)[:, :C]
    _, q = strided(2 * B * Sq + 4, C + 3, 1)
    q1, q2 = q[4:4 + B * Sq], q[4 + B * Sq:4 + 2 * B * Sq]
    _, k1 = strided(B * Skv1, C + 1, 3)
    _, v1 = strided(B * Skv1, C + 5, 1)
    _, k2 = strided(B * Skv2, C + 7, 5)
    _, v2 = strided(B * Skv2, 2 * C + 1, 7)
    ldo, off = C + 9, 11
    obuf = torch.full((B * Sq * ldo + 2 * off,), 7.0, device=dev, dtype=torch.float16)
    o = obuf[off:off + B * Sq * ldo].view(B * Sq, ldo)[:, :C]
    assert all(t.data_ptr() % 16 != 0 and t.stride(0) % 8 != 0 for t in (q1, q2, k1, v1, k2, v2, o))
    ops.attention_dual_fwd(q1, k1, v1, q2, k2, v2, o, B, H, Sq, Skv1, Skv2, hd)
    ref = R.ref_dual_attention(*(t.cpu().contiguous() for t in (q1, k1, v1, q2, k2, v2)), B, H, Sq, Skv1, Skv2, hd, hd ** -0.5)
    err = R.rel_l2(o.cpu().contiguous(), ref)
    print(f"[p2p] strided, unaligned: O rel-L2 {err:.3e}")
    assert err <= O_BOUND["fp16"], err
    canary = torch.ones(obuf.numel(), dtype=torch.bool)
    canary[off:off + B * Sq * ldo].view(B * Sq, ldo)[:, :C] = False
    assert (obuf.cpu()[canary] == 7.0).all() and int(canary.sum()) == 2 * off + B * Sq * (ldo - C)


def test_refusals_return_minus_22_and_leave_o_untouched():
    from textboost_amd import _lib as L
    from textboost_amd import ops

    def call(two=True, Sq=16, H=2, hd=16, Skv1=8, Skv2=8, dtype=torch.float16, causal1=0, causal2=0, Sq2=None, H2=None, hd2=None, B2=1, null=None):
        C = H * hd
        q = torch.zeros(Sq, C, device=dev, dtype=dtype)
        k = torch.zeros(max(Skv1, Skv2, 1), C, device=dev, dtype=dtype)
        o = torch.full((Sq, C), 5.0, device=dev, dtype=dtype)
        d1 = ops._attn_desc(q, k, k, o, None, 1, H, Sq, Skv1, hd, hd ** -0.5, causal1)
        d2 = ops._attn_desc(q, k, k, o, None, B2, H if H2 is None else H2, Sq if Sq2 is None else Sq2, Skv2, hd if hd2 is None else hd2,
                            hd ** -0.5, causal2)
        if null == "O":
            d1.O = None
        if null == "K2":
            d2.K = None
        rc = L.lib().tb_attention_dual_fwd(d1, d2 if two else None, ops._dt(q), L.stream())
        torch.cuda.synchronize()
        return rc, o
    with L.use_half("fp16"):
        for kw in (dict(hd=12), dict(hd=168), dict(hd=4), dict(Skv1=0), dict(Skv2=0), dict(Skv1=129), dict(Skv2=129), dict(two=False, Skv1=129),
                   dict(Sq2=32), dict(H2=4), dict(H2=4, hd2=8), dict(hd2=8), dict(B2=2), dict(causal1=1), dict(causal2=1), dict(two=False, causal1=1),
                   dict(dtype=torch.float32), dict(null="O"), dict(null="K2")):
            rc, o = call(**kw)
            assert rc == TB_EINVAL, (kw, rc)
            assert (o == 5.0).all(), kw
        for kw in (dict(), dict(two=False), dict(Skv1=128, Skv2=1), dict(two=False, Skv2=129), dict(two=False, causal2=1)):      # d2 is not read
            rc, o = call(**kw)
            assert rc == 0 and (o == 0).all(), kw                   # zero operands: V = 0
        with pytest.raises(RuntimeError, match="tb_attention_dual_fwd"):
            z = torch.zeros(16, 24, device=dev, dtype=torch.float16)
            ops.attention_dual_fwd(z, z[:8], z[:8], z, z[:8], z[:8], torch.empty_like(z), 1, 2, 16, 8, 8, 12)


# ------------------------------------------------------------------------------------------------ UNet level
def _plan77(reweight=(("fluffy", 2.0),)):
    from tests.test_p2p_host import StubTokenizer
    from textboost_amd import p2p
    return p2p.plan(StubTokenizer(), "a dog on a beach", "a fluffy <dog> dog on a beach", 77, reweight)


def _level(hip, block):
    nl = len(hip.geo.block_out_channels)
    part = block.split(".")
    return nl - 1 if part[0] == "mid_block" else (int(part[1]) if part[0] == "down_blocks" else nl - 1 - int(part[1]))


def test_unet_hook_controls_the_edited_rows_only_and_leaves_no_state():
    from tests.test_gpu_model import make_unet
    from textboost_amd import ops
    from textboost_amd.p2p import P2PControl
    B, hw, D, n, T = 4, 16, 64, 1, 77
    _, hip, _ = make_unet(B, hw, D)
    _, fresh, _ = make_unet(B, hw, D)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, 4, hw, hw, generator=g).half().to(dev)
    t = torch.tensor([17, 17, 17, 17], device=dev)
    ehs = torch.randn(B * T, D, generator=g).half().to(dev)
    assert hip.p2p is None
    want = fresh.forward(x, t, ehs).clone()
    plain = hip.forward(x, t, ehs).clone()
    assert torch.equal(plain, want)                                  # p2p = None: a fresh UNet's prediction, bit for bit
    blocks = [name[:-len(".transformer_blocks.0.attn2")] for name, _ in hip.xattn]
    plain_o = {b: (hip._bufs[b + ".o1"].clone(), hip._bufs[b + ".o2"].clone()) for b in blocks}
    pl = _plan77()
    assert not (pl.a == 1).all() and pl.w.max() == 2                 # an added word and a reweight: both terms are live
    ctl = P2PControl.for_unet(hip, pl)
    assert ctl.n == n and not ctl.single
    ctl.reset()
    ctl.cross_active = ctl.self_active = True
    hip.p2p = ctl
    try:
        pred = hip.forward(x, t, ehs).clone()
    finally:
        hip.p2p = None
    assert torch.isfinite(pred).all() and torch.equal(pred[:3], plain[:3]) and not torch.equal(pred[3], plain[3])
    kv_all = hip.kv_all.cpu()
    levels = set()
    for (name, C), block in zip(hip.xattn, blocks):
        level = _level(hip, block)
        levels.add(level)
        HW = (hip.H >> level) * (hip.W >> level)
        heads = hip.geo.heads(level)
        hd = C // heads
        src, edt = slice(2 * n * HW, 3 * n * HW), slice(3 * n * HW, 4 * n * HW)
        ksrc, kedt = slice(2 * n * T, 3 * n * T), slice(3 * n * T, 4 * n * T)
        q2, o2 = hip._bufs[block + ".q2"].cpu(), hip._bufs[block + ".o2"].cpu()
        ko = hip.kv_off[name]
        k2, v2 = kv_all[:, ko:ko + C], kv_all[:, ko + C:ko + 2 * C]
        ref = R.ref_p2p_cross(q2[src], k2[ksrc], q2[edt], k2[kedt], v2[kedt], pl.M, pl.a, pl.w, n, heads, HW, T, hd, hd ** -0.5)
        err = R.rel_l2(o2[edt], ref)
        unctl = R.rel_l2(R.ref_attention(q2[edt], k2[kedt], v2[kedt], n, heads, HW, T, hd, hd ** -0.5), ref)
        assert torch.equal(o2[:3 * n * HW], plain_o[block][1][:3 * n * HW].cpu())        # the other rows: the plain forward's bits
        # self-attention: the edited rows take the source rows' maps at levels >= 2.  Below, and for every other row, o1 is what the plain
        # launch gives on this forward's own qkv (the edited rows' inputs differ from the plain forward's behind the first controlled layer)
        qkv, o1 = hip._bufs[block + ".qkv"], hip._bufs[block + ".o1"]
        again = torch.empty_like(o1)
        ops.attention_fwd(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], again, torch.empty(B * heads, HW, device=dev), B, heads, HW, HW, hd)
        assert torch.equal(o1[:3 * n * HW], plain_o[block][0][:3 * n * HW]) and torch.equal(o1[:3 * n * HW], again[:3 * n * HW])
        if level >= 2:
            c = qkv.cpu()
            sref = R.ref_attention(c[src, :C], c[src, C:2 * C], c[edt, 2 * C:], n, heads, HW, HW, hd, hd ** -0.5)
            serr = R.rel_l2(o1[edt].cpu(), sref)
            assert serr <= O_BOUND["fp16"], (block, serr)
            assert not torch.equal(o1[edt], again[edt])
        else:
            serr = 0.0
            assert torch.equal(o1[edt], again[edt])
        print(f"[p2p] tiny UNet {block} (level {level}, {heads} heads of {hd}): o2[c_edit] rel-L2 {err:.3e} (uncontrolled attention is {unctl:.2e} "
              f"away), o1[c_edit] {serr:.3e}")
        assert err <= O_BOUND["fp16"], (block, err)
        assert unctl > 10 * O_BOUND["fp16"]                          # the control is not a no-op on these operands
    assert min(levels) < 2 <= max(levels)
    assert torch.equal(hip.forward(x, t, ehs), plain)                # set and unset: no state left behind


# ------------------------------------------------------------------------------------------------ sampler level
@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    from tests.test_compose_host import write_run
    from tests.test_gpu_generate import D_TEXT, write_model_dir
    from textboost_amd import generate as G
    from textboost_amd.p2p import P2PControl
    root = tmp_path_factory.mktemp("p2p")
    mdir, da, db = str(root / "model"), str(root / "runs" / "dog"), str(root / "runs" / "style")
    write_model_dir(mdir, hw=16)
    write_run(da, ["<dog>"], ["<hflip>"], seed=1, rank=4, keep_rows="even")
    write_run(db, ["<watercolor>"], ["<hflip>"], seed=2, rank=4, keep_rows="odd")
    B = 4                                                             # two seeds: source rows 0, 1 and edited rows 2, 3
    with torch.no_grad():
        pipe = G.Pipeline.from_model_dir(mdir, B, steps=4, guidance=7.5, device=dev)
    g = torch.Generator().manual_seed(3)
    cond = torch.randn(B * 77, D_TEXT, generator=g).half().float().to(dev)
    uncond = torch.randn(77, D_TEXT, generator=g).half().float().repeat(B, 1).to(dev)
    lat = torch.cat([G.seeded_latent(s, 16) for s in (0, 1)] * 2).to(dev)
    ctl = P2PControl.for_unet(pipe.unet, _plan77(), cross_steps=0.75, self_steps=0.5)
    return dict(root=root, mdir=mdir, da=da, db=db, pipe=pipe, B=B, cond=cond, uncond=uncond, lat=lat, ctl=ctl)


def test_sampler_source_rows_keep_their_bits_and_edited_rows_change(tiny):
    from textboost_amd.p2p import P2PControl
    from textboost_amd.sampler import HipSampler
    pipe, ctl = tiny["pipe"], tiny["ctl"]
    args = (tiny["cond"], tiny["uncond"])
    with torch.no_grad():
        plain = pipe.sampler.denoise(*args, latents=tiny["lat"]).clone()
        edited = pipe.sampler.denoise(*args, latents=tiny["lat"], p2p=ctl).clone()
        assert pipe.unet.p2p is None and not ctl.cross_active and not ctl.self_active
        assert torch.isfinite(edited).all()
        assert torch.equal(edited[:2], plain[:2])                     # the source images: bit for bit those of the run without control
        assert not torch.equal(edited[2], plain[2]) and not torch.equal(edited[3], plain[3])
        assert torch.equal(pipe.sampler.denoise(*args, latents=tiny["lat"], p2p=ctl), edited)
        off = P2PControl.for_unet(pipe.unet, _plan77(), cross_steps=0.0, self_steps=0.0)
        assert torch.equal(pipe.sampler.denoise(*args, latents=tiny["lat"], p2p=off), plain)
        only_self = P2PControl.for_unet(pipe.unet, _plan77(), cross_steps=0.0, self_steps=0.5)
        s = pipe.sampler.denoise(*args, latents=tiny["lat"], p2p=only_self).clone()
        assert torch.equal(s[:2], plain[:2]) and not torch.equal(s[2:], plain[2:]) and not torch.equal(s[2:], edited[2:])
        # refusals leave nothing behind
        other = P2PControl(_plan77(), 1, 77, 16, 16, device=dev)
        with pytest.raises(ValueError, match="control is built for batch 4"):
            pipe.sampler.denoise(*args, latents=tiny["lat"], p2p=other)
        bad = P2PControl.for_unet(pipe.unet, _plan77())
        bad.cross_steps = 1.5
        with pytest.raises(ValueError, match="cross_steps 1.5"):
            pipe.sampler.denoise(*args, latents=tiny["lat"], p2p=bad)
        with pytest.raises(ValueError, match="self_steps"):
            P2PControl.for_unet(pipe.unet, _plan77(), self_steps=-0.5)
        ddpm = HipSampler(pipe.unet, pipe.vae, steps=2, guidance=7.5, scheduler="DDPMScheduler")
        with pytest.raises(NotImplementedError, match="DPM-Solver"):
            ddpm.denoise(*args, latents=tiny["lat"], p2p=ctl)
        from textboost_amd.attn_maps import AttnMapRecorder
        with pytest.raises(ValueError, match="does not go with maps"):
            pipe.sampler.denoise(*args, latents=tiny["lat"], p2p=ctl, maps=AttnMapRecorder(pipe.unet))
        with pytest.raises(ValueError, match="does not go with regions"):
            pipe.sampler.denoise(*args, latents=tiny["lat"], p2p=ctl, regions=object())
        assert pipe.unet.p2p is None
        assert torch.equal(pipe.sampler.denoise(*args, latents=tiny["lat"]), plain)


def test_captured_denoise_with_control_replays_bit_identically(tiny):
    from textboost_amd.sampler import HipSampler
    pipe, ctl = tiny["pipe"], tiny["ctl"]
    with torch.no_grad():
        two = HipSampler(pipe.unet, pipe.vae, steps=2, guidance=7.5)
        eager = two.denoise(tiny["cond"], tiny["uncond"], latents=tiny["lat"], p2p=ctl).clone()      # also the warm-up: every buffer exists
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):       # every launch goes to the one capturing stream: a chain
            out = two.denoise(tiny["cond"], tiny["uncond"], latents=tiny["lat"], p2p=ctl)
        replays = []
        for _ in range(2):
            out.fill_(float("nan"))
            graph.replay()
            torch.cuda.synchronize()
            replays.append(out.clone())
    assert torch.equal(replays[0], eager) and torch.equal(replays[1], eager)


# ------------------------------------------------------------------------------------------------ the CLI
def _child(cmd, cwd):
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, os.path.join(ROOT, "inference.py")] + cmd, capture_output=True, text=True, cwd=cwd)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def test_cli_edit_prompt_writes_the_two_row_grid_and_repeats_byte_for_byte(tiny):
    pytest.importorskip("transformers")
    from PIL import Image
    common = ["--model", tiny["mdir"], "--prompt", "a dog on a beach", "--seeds", "0", "1", "--steps", "3", "--output", "g.png"]
    edit = ["--edit-prompt", "a fluffy <dog> dog on a beach", "--reweight", "fluffy=2"]
    wds = {}
    for name, cmd in (("edit", [tiny["da"]] + common + edit), ("edit2", [tiny["da"]] + common + edit),
                      ("with", [tiny["da"], "--with", tiny["db"]] + common + ["--edit-prompt", "a <watercolor> painting of a <dog> dog on a beach"])):
        wds[name] = str(tiny["root"] / name)
        os.makedirs(wds[name])
        _child(cmd, wds[name])
    g = {k: _read(os.path.join(v, "g.png")) for k, v in wds.items()}
    assert g["edit"] == g["edit2"] and g["with"] != g["edit"]
    grid = np.asarray(Image.open(os.path.join(wds["edit"], "g.png"))).astype(int)
    assert grid.shape == (2 * 128, 2 * 128, 3)                       # the source row on top, the edited row below, one column per seed
    assert np.abs(grid[:, :128] - grid[:, 128:]).max() > 0           # the two seeds differ
    d = np.abs(grid[128:] - grid[:128])
    print(f"[p2p] inference.py: edited row vs source row, mean |delta| {d.mean():.2f} levels, max {d.max()}")
    assert d.max() > 0
    w = np.asarray(Image.open(os.path.join(wds["with"], "g.png"))).astype(int)
    assert w.shape == (2 * 128, 2 * 128, 3) and np.abs(w[128:] - w[:128]).max() > 0
