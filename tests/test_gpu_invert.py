"""Editing a photo by its prompt on the GPU (inference.py --invert-image; csrc/invert.hip, `HipSampler.invert`, `HipSampler.denoise(pin=...)`,
`Pipeline.invert_edit_images`): the two kernels against float64 / `tb_dpm_step`, the sampler on the tiny model directory of
tests/test_gpu_generate.py, and the CLI in child processes.

The bound of `tb_invert_step`.  The kernel evaluates, in fp32 on operands that are exact (x fp32, e_u / e_c halves, the scalars as the C ABI
receives them),  xn = cx x + ce (e_u + g (e_c - e_u)).  Written as a sum of products, xn = [cx x] + [ce e_u] + [ce g (e_c - e_u)].  Whatever
the order of evaluation and whichever multiply-adds the compiler contracts (a contraction only removes a rounding), the value of the first
term passes through at most 2 roundings (its product, the final sum), the second through at most 3 (the sum e_u + ., the product with ce, the
final sum) and the third through at most 5 (the difference, the product with g, the sum with e_u, the product with ce, the final sum).  Each
rounding multiplies by (1 + d), |d| <= u = 2^-24, so every term is off by a factor within (1 +- u)^5, i.e. by at most gamma_5 = 5u / (1 - 5u)
relative (Higham, Accuracy and Stability of Numerical Algorithms, Lemma 3.1), and with |e_c - e_u| <= |e_c| + |e_u|:
    |err| <= gamma_5 (|cx x| + |ce| (|e_u| + |g| (|e_c| + |e_u|))).
(Operands here are of order 1: nothing underflows.)"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import invert_ref as R

pytestmark = pytest.mark.gpu
dev = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TB_EINVAL = -22
SHAPES = [(4, 4, 16, 16), (2, 4, 8, 8), (3, 4, 5, 7), (2, 1, 1, 1)]      # 420 = a partial block with hw = 35; n_per_b = 1
PAD, CANARY = 3, 77.0                                                   # odd pads: the operands are 4-byte / 2-byte aligned only
STEP = (7.5, 0.8, 0.6, 0.9, 0.3, -0.1)                                  # guidance, alpha_t, sigma_t, ca, cb, cc


class Guarded:
    """a [rows, n] operand in the middle of a buffer of canaries"""

    def __init__(self, t):
        self.n = t.numel()
        self.buf = torch.full((self.n + 2 * PAD,), CANARY, dtype=t.dtype)
        self.buf[PAD:PAD + self.n] = t.reshape(-1)
        self.buf = self.buf.to(dev)
        self.t = self.buf[PAD:PAD + self.n].view(t.shape)

    def intact(self):
        b = self.buf.cpu().float()
        return bool((b[:PAD] == CANARY).all() and (b[PAD + self.n:] == CANARY).all())


def _operands(shape, hd, seed=11):
    B, C, h, w = shape
    n = C * h * w
    g = torch.Generator().manual_seed(seed)
    x, mp = torch.randn(B, n, generator=g), torch.randn(B, n, generator=g)
    e = (torch.randn(2 * B, n, generator=g) * 0.8).to(hd)
    pin = torch.randn(n, generator=g) * 0.9
    return B, n, h * w, C, x, mp, e, pin, g


# ------------------------------------------------------------------------------------------------ tb_invert_step
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("half", ["fp16", "bf16"])
def test_invert_step_against_float64(half, shape):
    from textboost_amd import _lib as L
    from textboost_amd import ops
    with L.use_half(half):
        hd = L.half_dtype()
        B, n, hw, C, x0, _, e, _, _ = _operands(shape, hd)
        eg = Guarded(e)
        for guidance, cx, ce in ((1.0, 1.0123, 0.0456), (3.0, 1.31, -0.27), (0.0, 0.97, 0.11)):
            want, bound = R.invert_step(x0, e, guidance, cx, ce)
            outs = []
            for rep in range(2):
                xg, x2g, tg = Guarded(x0), Guarded(torch.zeros(2 * B, n, dtype=hd)), Guarded(torch.zeros(B, n))
                ops.invert_step(xg.t, eg.t, x2g.t, tg.t, n, B, guidance, cx, ce)
                outs.append((xg.t.clone(), x2g.t.clone()))
                assert xg.intact() and x2g.intact() and tg.intact() and eg.intact()
                assert torch.equal(tg.t, xg.t)                                       # traj_out = x, bit for bit
                assert torch.equal(x2g.t[:B], xg.t.to(hd)) and torch.equal(x2g.t[B:], xg.t.to(hd))
            assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])      # a repeat launch
            err = (outs[0][0].double().cpu() - want).abs()
            print(f"[invert] step {half} {shape} g {guidance}: max err / bound {(err / bound.clamp_min(1e-300)).max().item():.3f}")
            assert (err <= bound).all()
            xn, x2n = Guarded(x0), Guarded(torch.zeros(2 * B, n, dtype=hd))          # traj_out = NULL
            ops.invert_step(xn.t, eg.t, x2n.t, None, n, B, guidance, cx, ce)
            assert torch.equal(xn.t, outs[0][0]) and torch.equal(x2n.t, outs[0][1]) and xn.intact() and x2n.intact()
        # refusals: -22, nothing launched
        lib = L.lib()
        xg, x2g, tg = Guarded(x0), Guarded(torch.zeros(2 * B, n, dtype=hd)), Guarded(torch.zeros(B, n))
        good = [L.ptr(xg.t), L.ptr(eg.t), L.ptr(x2g.t), L.ptr(tg.t), n, B, 1.0, 1.01, 0.05, L.stream()]
        for k, v in ((0, None), (1, None), (2, None), (4, 0), (4, -1), (5, 0), (5, -2), (5, 65536)):
            bad = list(good)
            bad[k] = v
            assert lib.tb_invert_step(*bad) == TB_EINVAL, (k, v)
        torch.cuda.synchronize()
        assert torch.equal(xg.t.cpu(), x0) and (x2g.t == 0).all() and (tg.t == 0).all()
        assert lib.tb_invert_step(*good) == 0
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ tb_dpm_step_pin
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("half", ["fp16", "bf16"])
def test_dpm_step_pin_is_dpm_step_plus_the_select(half, shape):
    from textboost_amd import _lib as L
    from textboost_amd import ops
    with L.use_half(half):
        hd = L.half_dtype()
        B, n, hw, C, x0, mp0, e, pin, g = _operands(shape, hd)
        # The checks "x2 is tb_dpm_step's, bit for bit" and "x2 == half(x)" can both hold only where tb_dpm_step's own x2 is the rounding of
        # its own x.  In the fp16 build its conversion is folded into the update's last fma (one rounding of the exact fma), which differs
        # from half(x) where the fp32 result lands on a tie of the second rounding (about 2^-14 of the elements: seed 11 has one among the
        # 4096 of the first shape).  That is a property of tb_dpm_step and of the inputs, not of the kernel under test, so the inputs are
        # made free of it with tb_dpm_step alone: the m_prev operand of such an element is drawn again.
        redrawn = 0
        for _ in range(8):
            xs, ms, x2s = x0.to(dev), mp0.to(dev), torch.zeros(2 * B, n, device=dev, dtype=hd)
            ops.dpm_step(xs, e.to(dev), ms, x2s, n, B, *STEP)
            tie = (x2s[:B] != xs.to(hd)).cpu()
            if not tie.any():
                break
            redrawn += int(tie.sum())
            mp0[tie] = torch.randn(int(tie.sum()), generator=g)
        assert torch.equal(x2s[:B], xs.to(hd)) and torch.equal(x2s[B:], x2s[:B]) and redrawn <= 4, redrawn
        print(f"[invert] pin {half} {shape}: {redrawn} m_prev operand(s) drawn again (tb_dpm_step's x2 != half(x) there)")
        checker = ((torch.arange(hw) // shape[3] + torch.arange(hw) % shape[3]) % 2).to(torch.uint8)      # (row + column) % 2
        cases = [("n_src 0, no mask", 0, None), ("n_src 0, all 255", 0, torch.full((hw,), 255, dtype=torch.uint8)),
                 ("n_src B", B, None), ("n_src B, checkerboard", B, checker), ("n_src B/2, checkerboard", B // 2, checker),
                 ("n_src B/2, no mask", B // 2, None), ("n_src 0, zeros", 0, torch.zeros(hw, dtype=torch.uint8))]
        eg, pg = Guarded(e), Guarded(pin)
        pinb = pin.to(dev)[None].expand(B, n)
        for name, n_src, mask in cases:
            xg, mg, x2g = Guarded(x0), Guarded(mp0), Guarded(torch.zeros(2 * B, n, dtype=hd))
            kg = None if mask is None else Guarded(mask)
            ops.dpm_step_pin(xg.t, eg.t, mg.t, x2g.t, n, B, *STEP, pg.t, n_src, None if kg is None else kg.t, hw)
            cell = torch.ones(hw, dtype=torch.bool) if mask is None else mask.bool()
            step = cell.repeat(C)[None].expand(B, n).clone()             # element j of a row belongs to cell j % hw
            step[:n_src] = False
            step = step.to(dev)
            assert torch.equal(mg.t, ms), (name, "m_prev is the row's own unpinned data prediction, tb_dpm_step's bits")
            assert torch.equal(xg.t, torch.where(step, xs, pinb)), (name, "the select is exact per element")
            assert torch.equal(x2g.t[:B], torch.where(step, x2s[:B], pinb.to(hd))) and torch.equal(x2g.t[B:], x2g.t[:B]), name
            assert torch.equal(x2g.t[:B], xg.t.to(hd)), (name, "x2 == half(x)")
            assert all(t.intact() for t in (xg, mg, x2g, eg, pg)) and (kg is None or kg.intact()), name
            if n_src == 0 and (mask is None or bool(mask.all())):
                assert torch.equal(xg.t, xs) and torch.equal(x2g.t, x2s), name          # tb_dpm_step itself
            if n_src == B and mask is None:
                assert torch.equal(xg.t, pinb), name
            if B >= 2 and n_src == B // 2 and mask is not None and hw > 1:
                assert 0 < int(step.sum()) < (B - n_src) * n and not step[:n_src].any()
        # refusals: -22, nothing launched
        lib = L.lib()
        xg, mg, x2g, kg = Guarded(x0), Guarded(mp0), Guarded(torch.zeros(2 * B, n, dtype=hd)), Guarded(checker)
        good = [L.ptr(xg.t), L.ptr(eg.t), L.ptr(mg.t), L.ptr(x2g.t), n, B, *STEP, L.ptr(pg.t), B // 2, L.ptr(kg.t), hw, L.stream()]
        bads = [(0, None), (1, None), (2, None), (3, None), (12, None), (4, 0), (4, -3), (5, 0), (5, -1), (5, 65536), (7, 0.0), (13, -1), (13, B + 1),
                (15, 0), (15, -1), (15, n + 1)]
        for k, v in bads:
            for null_mask in (False, True):
                bad = list(good)
                bad[k] = v
                if null_mask:
                    bad[14] = None
                assert lib.tb_dpm_step_pin(*bad) == TB_EINVAL, (k, v, null_mask)
        torch.cuda.synchronize()
        assert torch.equal(xg.t.cpu(), x0) and torch.equal(mg.t.cpu(), mp0) and (x2g.t == 0).all()
        assert lib.tb_dpm_step_pin(*good) == 0
        torch.cuda.synchronize()


@pytest.mark.parametrize("half", ["fp16", "bf16"])
def test_an_unpinned_element_carries_tb_dpm_step_s_x2_also_where_that_is_not_half_of_x(half):
    """What the test above has to leave out: on the elements where tb_dpm_step's folded conversion differs from half(x), an element that
    keeps the step carries tb_dpm_step's x2 (the next UNet call of an unpinned row sees what text-to-image gives it), a pinned one half(pin).
    2 x 65536 elements: about eight such elements are expected in the fp16 build, none in the bf16 build (no folded conversion there)."""
    from textboost_amd import _lib as L
    from textboost_amd import ops
    with L.use_half(half):
        hd = L.half_dtype()
        B, n, hw, C, x0, mp0, e, pin, g = _operands((2, 4, 128, 128), hd, seed=12)
        x0, mp0, e, pin = (t.to(dev) for t in (x0, mp0, e, pin))
        xs, ms, x2s = x0.clone(), mp0.clone(), torch.zeros(2 * B, n, device=dev, dtype=hd)
        ops.dpm_step(xs, e, ms, x2s, n, B, *STEP)
        ties = int((x2s[:B] != xs.to(hd)).sum())
        print(f"[invert] pin {half}: tb_dpm_step's x2 != half(x) on {ties} of {B * n} elements")
        assert (ties > 0) == (half == "fp16")
        mask = (torch.rand(hw, generator=g) < 0.5).to(torch.uint8).to(dev)
        for n_src, mk in ((0, None), (1, mask)):
            xp, mq, x2p = x0.clone(), mp0.clone(), torch.zeros(2 * B, n, device=dev, dtype=hd)
            ops.dpm_step_pin(xp, e, mq, x2p, n, B, *STEP, pin, n_src, mk, hw)
            step = (torch.ones(hw, dtype=torch.bool, device=dev) if mk is None else mk.bool()).repeat(C)[None].expand(B, n).clone()
            step[:n_src] = False
            pinb = pin[None].expand(B, n)
            assert torch.equal(xp, torch.where(step, xs, pinb)) and torch.equal(mq, ms)
            assert torch.equal(x2p[:B], torch.where(step, x2s[:B], pinb.to(hd))) and torch.equal(x2p[B:], x2p[:B])


# ------------------------------------------------------------------------------------------------ sampler level
STEPS = 4


def _plan77():
    from tests.test_p2p_host import StubTokenizer
    from textboost_amd import p2p
    return p2p.plan(StubTokenizer(), "a dog on a beach", "a fluffy <dog> dog on a beach", 77, (("fluffy", 2.0),))


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    from safetensors.torch import load_file, save_file
    from tests.test_compose_host import write_run
    from tests.test_gpu_generate import D_TEXT, write_model_dir
    from textboost_amd import generate as G
    from textboost_amd import models
    from textboost_amd.p2p import P2PControl
    from textboost_amd.vae import VAEGeometry, vae_encoder_shapes
    root = tmp_path_factory.mktemp("invert")
    mdir, rdir = str(root / "model"), str(root / "runs" / "dog")
    write_model_dir(mdir, hw=16)
    vfile = os.path.join(mdir, "vae", "diffusion_pytorch_model.safetensors")      # the CLI encodes the photo: add the encoder half
    vgeo = VAEGeometry(block_out_channels=(64, 64, 128, 128), layers_per_block=1)
    enc_sd = {k: v.half().float() for k, v in models.random_state_dict(vae_encoder_shapes(vgeo), 15, device="cpu").items()}
    save_file({**load_file(vfile), **enc_sd}, vfile)
    write_run(rdir, ["<dog>"], ["<hflip>"], seed=1, rank=4, keep_rows="even")
    B = 2
    with torch.no_grad():
        pipe = G.Pipeline.from_model_dir(mdir, B, steps=STEPS, guidance=7.5, device=dev)
    g = torch.Generator().manual_seed(3)
    cond = torch.randn(B * 77, D_TEXT, generator=g).half().float().to(dev)
    uncond = torch.randn(77, D_TEXT, generator=g).half().float().repeat(B, 1).to(dev)
    z0 = (torch.randn(1, 4, 16, 16, generator=g) * 0.9).to(dev)
    ctl = P2PControl.for_unet(pipe.unet, _plan77(), cross_steps=0.75, self_steps=0.5)
    off = P2PControl.for_unet(pipe.unet, _plan77(), cross_steps=0.0, self_steps=0.0)
    with torch.no_grad():
        traj = pipe.sampler.invert(cond, uncond, z0).clone()                        # computed once, shared, never written
    return dict(root=root, mdir=mdir, rdir=rdir, pipe=pipe, B=B, cond=cond, uncond=uncond, z0=z0, ctl=ctl, off=off, traj=traj)


def test_invert_returns_the_trajectory_of_the_float64_formula(tiny):
    from textboost_amd import _lib as L
    pipe, smp, z0, B = tiny["pipe"], tiny["pipe"].sampler, tiny["z0"], tiny["B"]
    traj = tiny["traj"]
    assert traj.shape == (STEPS + 1, B, 4, 16, 16) and traj.dtype == torch.float32 and torch.isfinite(traj).all()
    assert torch.equal(traj[STEPS], z0.expand(B, -1, -1, -1))                         # level `steps` is z0, bit for bit
    ehs = torch.cat([tiny["uncond"], tiny["cond"]]).to(L.half_dtype()).contiguous()
    with torch.no_grad():
        for guidance, tr in ((1.0, traj), (3.0, smp.invert(tiny["cond"], tiny["uncond"], z0[0], guidance=3.0).clone())):
            assert torch.equal(tr[STEPS], traj[STEPS])
            worst = 0.0
            for k in range(STEPS - 1, -1, -1):         # the level's own input through the same forward call, then the formula in float64
                x2 = torch.cat([tr[k + 1], tr[k + 1]]).to(L.half_dtype())
                e = smp.unet.forward(x2, smp.t_dev[k], ehs).double()
                cx, ce = smp.sch.inversion_scalars(k)
                want = cx * tr[k + 1].double() + ce * (e[:B] + guidance * (e[B:] - e[:B]))
                worst = max(worst, ((tr[k].double() - want).abs().max() / want.abs().max()).item())
            print(f"[invert] sampler, guidance {guidance}: worst level against the by-hand replay {worst:.2e} (bound 1e-6)")
            assert worst <= 1e-6
            if guidance == 3.0:
                assert not torch.equal(tr[0], traj[0])
        assert torch.equal(smp.invert(tiny["cond"], tiny["uncond"], z0.expand(B, -1, -1, -1).contiguous()), traj)     # [B, 4, h, w] and a repeat
    assert not torch.equal(traj[0], traj[STEPS])


def test_pinned_denoise_returns_the_photo_in_the_source_row(tiny):
    smp, traj, z0, ctl = tiny["pipe"].sampler, tiny["traj"], tiny["z0"], tiny["ctl"]
    args = (tiny["cond"], tiny["uncond"])
    pin = traj[:, 0]
    start = traj[0, :1].expand(2, -1, -1, -1).contiguous()
    with torch.no_grad():
        before = smp.denoise(*args, latents=start).clone()
        x = smp.denoise(*args, p2p=ctl, pin=pin).clone()
        assert tiny["pipe"].unet.p2p is None and not ctl.cross_active and not ctl.self_active
        assert torch.equal(x[0], z0[0])                                               # the source row ends as z0, bit for bit
        assert torch.isfinite(x[1]).all() and not torch.equal(x[1], z0[0])
        assert torch.equal(smp.denoise(*args, p2p=ctl, pin=pin), x)
        # no control active: the pin changes nothing in an unpinned row
        assert torch.equal(smp.denoise(*args, p2p=tiny["off"], pin=pin)[1], before[1])
        # a mask: the edited row's cells outside it stay on the trajectory and end as z0
        mask = torch.zeros(16, 16, dtype=torch.uint8)
        mask[4:11, 3:9] = 1
        m = mask.bool().to(dev)
        xm = smp.denoise(*args, p2p=ctl, pin=pin, pin_mask=mask.to(dev)).clone()
        assert torch.equal(xm[0], z0[0]) and torch.equal(xm[1][:, ~m], z0[0][:, ~m])
        assert torch.isfinite(xm).all() and not torch.equal(xm[1][:, m], z0[0][:, m])
        assert torch.equal(smp.denoise(*args, p2p=ctl, pin=pin, pin_mask=torch.ones(16, 16, dtype=torch.uint8))[1], x[1])
        # afterwards the plain denoise gives the bits it gave before
        assert torch.equal(smp.denoise(*args, latents=start), before) and tiny["pipe"].unet.p2p is None


def test_refusals_leave_no_state(tiny):
    from textboost_amd.sampler import HipSampler
    pipe, smp, traj, z0, ctl = tiny["pipe"], tiny["pipe"].sampler, tiny["traj"], tiny["z0"], tiny["ctl"]
    args = (tiny["cond"], tiny["uncond"])
    pin = traj[:, 0]
    start = traj[0, :1].expand(2, -1, -1, -1).contiguous()
    with torch.no_grad():
        before = smp.denoise(*args, latents=start).clone()
        state = [t.clone() for t in (smp.x, smp.m_prev, smp.x2)]
        mask = torch.ones(16, 16, dtype=torch.uint8, device=dev)
        for kw, match in ((dict(pin=pin), "pin without p2p"), (dict(pin=pin, p2p=ctl, latents=start), "pin with latents"),
                          (dict(pin_mask=mask, p2p=ctl), "pin_mask without pin"), (dict(pin=pin[:-1], p2p=ctl), "expected float32"),
                          (dict(pin=pin.double(), p2p=ctl), "expected float32"), (dict(pin=traj, p2p=ctl), "expected float32"),
                          (dict(pin=pin, p2p=ctl, pin_mask=mask.float()), "expected uint8"),
                          (dict(pin=pin, p2p=ctl, pin_mask=mask[:8]), "expected uint8")):
            with pytest.raises(ValueError, match=match):
                smp.denoise(*args, **kw)
        for bad, match in ((z0.double(), "expected an fp32 tensor"), (z0[:, :, :8], "the sampler is built for"),
                           (z0.expand(3, -1, -1, -1), "the sampler is built for")):
            with pytest.raises(ValueError, match=match):
                smp.invert(*args, bad)
        for gbad in (-1.0, float("nan")):
            with pytest.raises(ValueError, match="guidance"):
                smp.invert(*args, z0, guidance=gbad)
        ddpm = HipSampler(pipe.unet, pipe.vae, steps=2, guidance=7.5, scheduler="DDPMScheduler")
        with pytest.raises(NotImplementedError, match="DPM-Solver"):
            ddpm.invert(*args, z0)
        with pytest.raises(NotImplementedError, match="DPM-Solver"):
            ddpm.denoise(*args, p2p=ctl, pin=pin[:3])
        vsmp = HipSampler(pipe.unet, pipe.vae, steps=STEPS, guidance=7.5, scheduler_config={"prediction_type": "v_prediction"})
        with pytest.raises(NotImplementedError, match="one level off"):
            vsmp.invert(*args, z0)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(state, (smp.x, smp.m_prev, smp.x2)))      # nothing was touched
        assert pipe.unet.p2p is None and not ctl.cross_active and not ctl.self_active
        assert torch.equal(smp.denoise(*args, latents=start), before)


def test_captured_inversion_and_pinned_denoise_replay_bit_identically(tiny):
    smp, z0, ctl = tiny["pipe"].sampler, tiny["z0"], tiny["ctl"]
    args = (tiny["cond"], tiny["uncond"])

    def edit():
        traj = smp.invert(*args, z0)
        return traj, smp.denoise(*args, p2p=ctl, pin=traj[:, 0])
    with torch.no_grad():
        traj_e, x_e = edit()                       # also the warm-up: every buffer exists
        traj_e, x_e = traj_e.clone(), x_e.clone()
        assert torch.equal(traj_e, tiny["traj"])
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):       # every launch goes to the one capturing stream: a chain
            traj_g, x_g = edit()
        for _ in range(2):
            traj_g.fill_(float("nan"))
            x_g.fill_(float("nan"))
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(traj_g, traj_e) and torch.equal(x_g, x_e)


# ------------------------------------------------------------------------------------------------ the CLI
def _child(cmd, cwd):
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, os.path.join(ROOT, "inference.py")] + cmd, capture_output=True, text=True, cwd=cwd)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def test_cli_inverts_a_photo_edits_it_and_repeats_byte_for_byte(tiny):
    pytest.importorskip("transformers")
    from PIL import Image
    from tests.test_gpu_edit import _photo
    from textboost_amd import edit as E
    root = tiny["root"]
    rgb = _photo()                                                    # 200 x 150
    photo, maskf = str(root / "photo.png"), str(root / "mask.png")
    Image.fromarray(rgb).save(photo)
    m = np.zeros(rgb.shape[:2], dtype=np.uint8)
    m[40:110, 60:150] = 255
    Image.fromarray(m).save(maskf)
    common = [tiny["rdir"], "--model", tiny["mdir"], "--prompt", "a dog on a beach", "--edit-prompt", "a fluffy <dog> dog on a beach",
              "--invert-image", photo, "--steps", "3", "--seeds", "5", "6", "7", "--output", "g.png"]
    wds = {}
    for name, extra in (("mask", ["--mask", maskf]), ("mask2", ["--mask", maskf]), ("nopaste", ["--mask", maskf, "--no-paste"])):
        wds[name] = str(root / name)
        os.makedirs(wds[name])
        out = _child(common + extra, wds[name])
        assert "--seeds is not read" in out
    raw = {k: open(os.path.join(v, "g.png"), "rb").read() for k, v in wds.items()}
    img = {k: np.asarray(Image.open(os.path.join(v, "g.png"))).astype(int) for k, v in wds.items()}
    assert raw["mask"] == raw["mask2"]                                # deterministic: the encoder's mode, no seed
    for k in img:
        assert img[k].shape == (2 * 128, 128, 3), k                   # the source row on top, the edit below, one column
        assert np.array_equal(img[k][:128], img["mask"][:128]), k     # the top is the VAE round trip of the photo in every run
        assert np.abs(img[k][128:] - img[k][:128]).max() > 0, k
    prepared = np.asarray(Image.fromarray(rgb).resize((170, 128), Image.LANCZOS).crop((21, 0, 149, 128))).astype(int)
    assert E.edit_geometry(200, 150, 128) == (170, 128, 21, 0)
    pm, _ = E.prepare_mask(E.load_mask(maskf), 128)
    outside = pm == 0
    assert 0 < outside.sum() < outside.size
    assert np.array_equal(img["mask"][128:][outside], prepared[outside])          # pasted: the prepared photo's bytes outside the mask
    assert not np.array_equal(img["nopaste"][128:][outside], prepared[outside])   # --no-paste: the plain decode
    assert np.array_equal(img["mask"][128:][~outside], img["nopaste"][128:][~outside])
    assert np.abs(img["mask"][:128] - prepared).max() > 0             # the source row is a decode, never pasted
