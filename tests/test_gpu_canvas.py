"""The MultiDiffusion canvas on the GPU (inference.py --width / --height; csrc/canvas.hip, `HipSampler.denoise_canvas`,
`Pipeline.canvas_images`), in both numeric libraries, operands between canaries:

  * `tb_canvas_gather` against the reference's bytes, no tolerance;
  * `tb_canvas_step` with one window against `tb_dpm_step`'s bits (x, m_prev, and the next gather's x2), with many windows against the
    float64 reference of tests/canvas_ref.py.  The bound is 8 x the error of the reference restated in float32 on the same case (the
    yardstick convention of tests/test_gpu_attn_maps.py); it is never taken from the kernel's output;
  * `tb_tile_blend`: fp32 against float64 under the same rule, the bytes against the byte rule on the kernel's own fp32 output, one tile
    against `tb_vae_image_rgbx`;
  * the sampler on the tiny model directory of tests/test_gpu_generate.py (S = 16): a 16 x 16 canvas is `denoise` / `images` bit for bit, a
    16 x 24 canvas is replayed step by step, and the CLI in child processes."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import canvas_ref as R

pytestmark = pytest.mark.gpu
dev = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TB_EINVAL = -22
PAD = 5
S = 8
STEP = (7.5, 0.8, 0.6, 0.9, 0.3, -0.1)                 # guidance, alpha_t, sigma_t, ca, cb, cc
# (Hc, Wc, stride): one window; overlap; a clamped last window; 2-D with both axes clamped; no overlap; stride 1
SHAPES = [(8, 8, 4), (8, 20, 4), (8, 21, 4), (11, 13, 3), (8, 16, 8), (8, 10, 1)]
IMAGES = (1, 3)
BATCHES = (1, 3, 13)                                   # chunks that fit exactly and chunks that end ragged
MARGIN = 8.0


def ids(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


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


def bits(t):
    """a tensor's bytes as integers (NaN-safe, sign-of-zero-safe equality)"""
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def plan_of(shape, n, Bu):
    from textboost_amd.canvas import CanvasPlan
    Hc, Wc, s = shape
    return CanvasPlan(S, Hc, Wc, s, n, Bu)


def canvas_case(shape, n, seed):
    """x, m_prev float32 [n, 4, Hc, Wc] and per-pair (e_u, e_c) already rounded to 16 bits by the caller"""
    Hc, Wc, s = shape
    rng = np.random.RandomState(seed)
    x = rng.standard_normal((n, 4, Hc, Wc)).astype(np.float32)
    mp = rng.standard_normal((n, 4, Hc, Wc)).astype(np.float32)
    P = n * len(R.offsets(Hc, S, s)) * len(R.offsets(Wc, S, s))
    eu, ec = (rng.standard_normal((P, 4, S, S)) * 0.8).astype(np.float32), (rng.standard_normal((P, 4, S, S)) * 0.8).astype(np.float32)
    return x, mp, eu, ec


def rounded(a, half):
    """float32 array -> the values the library's 16-bit type holds, as float32"""
    return R.to_half(a, half).float().numpy()


# ------------------------------------------------------------------------------------------------ tb_canvas_gather
@pytest.mark.parametrize("half", ["fp16", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_gather_gives_the_reference_bytes(shape, half):
    from textboost_amd import _lib as L
    from textboost_amd import ops
    Hc, Wc, s = shape
    oy, ox = R.offsets(Hc, S, s), R.offsets(Wc, S, s)
    with L.use_half(half):
        for n in IMAGES:
            x = canvas_case(shape, n, 3)[0] * 3.0
            for Bu in BATCHES:
                plan = plan_of(shape, n, Bu)
                assert plan.oy == oy and plan.ox == ox
                xg = Guarded(torch.from_numpy(x), 5.0)
                hg = Guarded(R.to_half(x[::-1].copy() * 0.5, half), 5.0)                  # a 16-bit canvas with other values
                for chunk in range(plan.n_chunks):
                    x2 = Guarded(torch.full((2 * Bu, 4, S, S), 9.0, dtype=L.half_dtype()), 7.0)
                    ops.canvas_gather(xg.t, x2.t, plan, chunk)
                    want = R.gather(x, S, oy, ox, Bu, chunk, half)
                    assert torch.equal(bits(x2.t), bits(want)), (n, Bu, chunk)           # bytes, no tolerance
                    last = min((chunk + 1) * Bu, plan.pairs) - 1 - chunk * Bu
                    for r in range(last + 1, Bu):                                        # ragged rows repeat the last valid pair
                        assert torch.equal(bits(x2.t[r]), bits(x2.t[last])) and torch.equal(bits(x2.t[Bu + r]), bits(x2.t[last]))
                    assert x2.intact()
                    ops.canvas_gather(xg.t, x2.t, plan, chunk, xh=hg.t)                  # from the 16-bit canvas: a copy
                    want = R.gather(hg.t.float().cpu().numpy(), S, oy, ox, Bu, chunk, half)
                    assert torch.equal(bits(x2.t), bits(want)) and x2.intact()
                assert xg.intact() and hg.intact() and torch.equal(xg.t.cpu(), torch.from_numpy(x))


# ------------------------------------------------------------------------------------------------ tb_canvas_step
def _launch_step(plan, x, mp, eps_all, half, with_xh=True):
    from textboost_amd import _lib as L
    from textboost_amd import ops
    xg, mg = Guarded(torch.from_numpy(x), 5.0), Guarded(torch.from_numpy(mp), 5.0)
    eg = Guarded(R.to_half(eps_all, half), 5.0)
    hg = Guarded(torch.full(x.shape, 9.0, dtype=L.half_dtype()), 7.0) if with_xh else None
    before = bits(eg.t).clone()
    ops.canvas_step(xg.t, eg.t, mg.t, plan, *STEP, xh=None if hg is None else hg.t)
    torch.cuda.synchronize()
    assert xg.intact() and mg.intact() and eg.intact() and (hg is None or hg.intact())
    assert torch.equal(bits(eg.t), before)
    return xg, mg, hg


@pytest.mark.parametrize("half", ["fp16", "bf16"])
def test_step_with_one_window_has_dpm_steps_bits(half):
    from textboost_amd import _lib as L
    from textboost_amd import ops
    shape = (8, 8, 4)
    per = 4 * S * S
    with L.use_half(half):
        for n in IMAGES:
            x, mp, eu, ec = canvas_case(shape, n, 11 + n)
            eu, ec = rounded(eu, half), rounded(ec, half)
            dx, dm = torch.from_numpy(x).to(dev), torch.from_numpy(mp).to(dev)
            e2 = R.to_half(np.concatenate([eu, ec]), half).to(dev).contiguous()
            dx2 = torch.zeros(2 * n, per, dtype=L.half_dtype(), device=dev)
            ops.dpm_step(dx, e2, dm, dx2, per, n, *STEP)
            for Bu in BATCHES:
                plan = plan_of(shape, n, Bu)
                xg, mg, hg = _launch_step(plan, x, mp, R.scatter_eps((eu, ec), Bu, fill=np.nan), half)
                assert torch.equal(bits(xg.t), bits(dx.view_as(xg.t))) and torch.equal(bits(mg.t), bits(dm.view_as(mg.t))), (n, Bu)
                for chunk in range(plan.n_chunks):                                       # the following gather is dpm_step's x2
                    x2 = torch.zeros(2 * Bu, 4, S, S, dtype=L.half_dtype(), device=dev)
                    ops.canvas_gather(xg.t, x2, plan, chunk, xh=hg.t)
                    for r in range(Bu):
                        p = min(chunk * Bu + r, n - 1)
                        assert torch.equal(bits(x2[r]).reshape(-1), bits(dx2[p])) and torch.equal(bits(x2[Bu + r]).reshape(-1), bits(dx2[n + p]))
                x_only = _launch_step(plan, x, mp, R.scatter_eps((eu, ec), Bu), half, with_xh=False)[0]      # xh is optional
                assert torch.equal(bits(x_only.t), bits(xg.t))


def _step_errors(shape, n, Bu, half, x, mp, eu, ec, tag):
    """launch; -> the kernel's (x, m_prev) after asserting them against float64 within MARGIN x the float32 restatement's error"""
    Hc, Wc, s = shape
    oy, ox = R.offsets(Hc, S, s), R.offsets(Wc, S, s)
    plan = plan_of(shape, n, Bu)
    eps_all = R.scatter_eps((eu, ec), Bu)
    want = R.step(x, mp, eps_all, S, oy, ox, Bu, *STEP)
    yard = R.step(x, mp, eps_all, S, oy, ox, Bu, *STEP, dtype=np.float32)
    xg, mg, hg = _launch_step(plan, x, mp, eps_all, half)
    got = (xg.t.cpu().numpy(), mg.t.cpu().numpy())
    for name, g_, w_, y_ in (("x", got[0], want[0], yard[0]), ("m_prev", got[1], want[1], yard[1])):
        bound = MARGIN * np.abs(y_.astype(np.float64) - w_).max()
        err = np.abs(g_.astype(np.float64) - w_).max()
        print(f"[canvas] step {half} {tag} {shape} n={n} Bu={Bu} {name}: error {err:.3e}, float32 yardstick {bound / MARGIN:.3e}, "
              f"ratio {err / (bound / MARGIN):.2f} (bound {MARGIN:g})")
        assert bound > 0 and err <= bound, (name, err, bound)
    assert torch.equal(bits(hg.t), bits(R.to_half(got[0], half))) or half == "fp16"      # bf16: the plain conversion of the stored x
    assert float((hg.t.float().cpu() - torch.from_numpy(got[0])).abs().max()) <= float(np.abs(got[0]).max()) * 2.0 ** -8
    return plan, eps_all, got


@pytest.mark.parametrize("half", ["fp16", "bf16"])
@pytest.mark.parametrize("shape", SHAPES[1:], ids=ids)
def test_step_with_many_windows_against_float64(shape, half):
    from textboost_amd import _lib as L
    with L.use_half(half):
        for n in IMAGES:
            x, mp, eu, ec = canvas_case(shape, n, 21 + n)
            eu, ec = rounded(eu, half), rounded(ec, half)
            for Bu in BATCHES:
                plan, eps_all, got = _step_errors(shape, n, Bu, half, x, mp, eu, ec, "random")
                again = _launch_step(plan, x, mp, eps_all, half)                          # a relaunch is bit-identical
                assert torch.equal(bits(again[0].t), bits(torch.from_numpy(got[0]))) and torch.equal(bits(again[1].t), bits(torch.from_numpy(got[1])))
                if plan.pairs % Bu:                                                     # NaN in the unused rows of the ragged chunk changes nothing
                    poisoned = R.scatter_eps((eu, ec), Bu, fill=np.nan)
                    assert np.isnan(poisoned).any()
                    nan = _launch_step(plan, x, mp, poisoned, half)
                    assert torch.equal(bits(nan[0].t), bits(torch.from_numpy(got[0]))) and torch.equal(bits(nan[1].t), bits(torch.from_numpy(got[1])))
                    assert torch.equal(bits(nan[2].t), bits(again[2].t))


@pytest.mark.parametrize("half", ["fp16", "bf16"])
@pytest.mark.parametrize("shape", SHAPES[1:], ids=ids)
def test_equal_eps_in_every_window_is_the_plain_step(shape, half):
    """no seam from the average itself: windows that agree on eps give the step of that eps"""
    from textboost_amd import _lib as L
    Hc, Wc, s = shape
    n, Bu = 3, 3
    oy, ox = R.offsets(Hc, S, s), R.offsets(Wc, S, s)
    with L.use_half(half):
        x, mp, _, _ = canvas_case(shape, n, 31)
        rng = np.random.RandomState(32)
        Eu, Ec = rounded(rng.standard_normal(x.shape) * 0.8, half), rounded(rng.standard_normal(x.shape) * 0.8, half)
        pl = R.pairs(n, oy, ox)
        eu = np.stack([Eu[i, :, y:y + S, xx:xx + S] for i, y, xx in pl])
        ec = np.stack([Ec[i, :, y:y + S, xx:xx + S] for i, y, xx in pl])
        _, _, got = _step_errors(shape, n, Bu, half, x, mp, eu, ec, "equal eps")
        g, a_t, s_t, ca, cb, cc = STEP
        eps = Eu.astype(np.float64) + g * (Ec.astype(np.float64) - Eu)
        m0 = (x - s_t * eps) / a_t
        plain = ca * x + cb * m0 + cc * mp
        yard = R.step(x, mp, R.scatter_eps((eu, ec), Bu), S, oy, ox, Bu, *STEP, dtype=np.float32)
        for name, g_, w_, y_ in (("x", got[0], plain, yard[0]), ("m_prev", got[1], m0, yard[1])):
            bound, err = MARGIN * np.abs(y_.astype(np.float64) - w_).max(), np.abs(g_.astype(np.float64) - w_).max()
            print(f"[canvas] equal eps {half} {shape} {name} against the plain step: error {err:.3e}, yardstick {bound / MARGIN:.3e}")
            assert bound > 0 and err <= bound


# ------------------------------------------------------------------------------------------------ tb_tile_blend
def byte_rule(img):
    """torch, float32: fp32 image [n, 3, H, W] in [0, 1] -> int32 RGBX [n, H, W]"""
    b = (img * 255).round().to(torch.int32)
    return b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)


@pytest.mark.parametrize("half", ["fp16", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_tile_blend_against_float64_and_its_bytes_against_its_own_fp32(shape, half):
    from textboost_amd import _lib as L
    from textboost_amd import ops
    Hp, Wp, s = shape
    P = S
    ty, tx = R.offsets(Hp, P, s), R.offsets(Wp, P, s)
    with L.use_half(half):
        for n in IMAGES:
            plan = plan_of(shape, n, 2)
            rng = np.random.RandomState(41 + n)
            tiles = (rng.standard_normal((plan.pairs, P, P, 4)) * 0.8).astype(np.float32)
            tiles[..., 3] = np.nan                                                       # the fourth column is never read
            for ramp in sorted({1, max(1, P - s), 20}):
                want = R.image_of(R.blend(tiles[..., :3], n, P, ty, tx, Hp, Wp, ramp)[0])
                yard = R.image_of(R.blend(tiles[..., :3], n, P, ty, tx, Hp, Wp, ramp, dtype=np.float32)[0].astype(np.float32))
                tg = Guarded(torch.from_numpy(tiles.reshape(-1, 4)), 5.0)
                ig = Guarded(torch.full((n, 3, Hp, Wp), 9.0), 7.0)
                bg = Guarded(torch.full((n, Hp, Wp), -3, dtype=torch.int32), 7)
                ops.tile_blend(tg.t, plan, 1, ramp, image=ig.t, rgbx=bg.t)
                torch.cuda.synchronize()
                got = ig.t.cpu()
                bound = MARGIN * np.abs(yard.astype(np.float64) - want).max()
                err = np.abs(got.numpy().astype(np.float64) - want).max()
                print(f"[canvas] blend {half} {shape} n={n} ramp={ramp}: error {err:.3e}, float32 yardstick {bound / MARGIN:.3e}")
                assert (bound > 0 or len(ty) * len(tx) == 1) and err <= bound
                assert torch.equal(bg.t.cpu(), byte_rule(got))                            # the bytes of the kernel's own fp32, exactly
                assert tg.intact() and ig.intact() and bg.intact() and torch.equal(bits(tg.t), bits(torch.from_numpy(tiles.reshape(-1, 4))))
                only = Guarded(torch.full((n, Hp, Wp), -3, dtype=torch.int32), 7)
                ops.tile_blend(tg.t, plan, 1, ramp, rgbx=only.t)                          # either output alone
                assert torch.equal(only.t, bg.t) and only.intact()
                img_only = Guarded(torch.full((n, 3, Hp, Wp), 9.0), 7.0)
                ops.tile_blend(tg.t, plan, 1, ramp, image=img_only.t)
                assert torch.equal(bits(img_only.t), bits(got)) and img_only.intact()


@pytest.mark.parametrize("half", ["fp16", "bf16"])
def test_a_single_tile_has_the_bytes_of_vae_image_rgbx(half):
    from tests.test_gpu_generate import _edge_values
    from textboost_amd import _lib as L
    from textboost_amd import ops
    with L.use_half(half):
        v = _edge_values().flip(0)                                                        # (the outliers first: the cut drops none of them)
        v = v[:v.numel() // (3 * S * S) * (3 * S * S)].reshape(-1, S * S, 3)              # every byte boundary, half-way point and outlier
        n = v.shape[0]
        tiles = torch.zeros(n * S * S, 4)
        tiles[:, :3] = v.reshape(-1, 3)
        tiles = tiles.to(dev)
        plan = plan_of((S, S, 4), n, 2)
        rgbx, image = torch.zeros(n, S, S, dtype=torch.int32, device=dev), torch.zeros(n, 3, S, S, device=dev)
        ops.tile_blend(tiles, plan, 1, 3, image=image, rgbx=rgbx)
        want, want_img = torch.zeros(n * S * S, dtype=torch.int32, device=dev), torch.zeros(n * 3, S * S, device=dev)
        ops.vae_image_rgbx(tiles, want, n, S * S)
        ops.vae_image(tiles, want_img, n, S * S, 3)
        assert torch.equal(rgbx.reshape(-1), want) and torch.equal(bits(image).reshape(-1), bits(want_img).reshape(-1))


@pytest.mark.parametrize("half", ["fp16", "bf16"])
def test_invalid_arguments_launch_nothing(half):
    from textboost_amd import _lib as L
    with L.use_half(half):
        lib = L.lib()
        n, Hc, Wc, Bu = 2, 11, 13, 3
        oy, ox = torch.tensor([0, 3], dtype=torch.int32), torch.tensor([0, 3, 5], dtype=torch.int32)
        oyd, oxd = oy.to(dev), ox.to(dev)
        xg, mg = Guarded(torch.full((n, 4, Hc, Wc), 2.0), 5.0), Guarded(torch.full((n, 4, Hc, Wc), 3.0), 5.0)
        hg = Guarded(torch.full((n, 4, Hc, Wc), 4.0, dtype=L.half_dtype()), 5.0)
        x2 = Guarded(torch.full((2 * Bu, 4, S, S), 9.0, dtype=L.half_dtype()), 7.0)
        eg = Guarded(torch.full((4, 2 * Bu, 4, S, S), 1.0, dtype=L.half_dtype()), 7.0)

        def tables(y=oy, x=ox, yd=oyd, xd=oxd, ny=2, nx=3):
            return [L.ptr(yd), L.ptr(y), ny, L.ptr(xd), L.ptr(x), nx]
        keep = []                                                  # the host tables stay alive while their pointers are in use

        def i32(*v):
            keep.append(torch.tensor(v, dtype=torch.int32))
            return keep[-1]
        bad_tables = [tables(y=i32(1, 3)), tables(y=i32(0, 2)), tables(x=i32(0, 3, 4)), tables(x=i32(1, 3, 5)), tables(x=i32(0, 5, 5)),
                      tables(x=i32(0, 5, 3)), tables(y=None), tables(x=None), tables(yd=None), tables(xd=None), tables(ny=0), tables(nx=0),
                      tables(ny=-1), tables(nx=2)]
        # gather: x, xh, x2, n, Hc, Wc, S, tables(6), Bu, chunk
        good = [L.ptr(xg.t), L.ptr(hg.t), L.ptr(x2.t), n, Hc, Wc, S] + tables() + [Bu, 0, L.stream()]
        bads = [(0, None), (2, None), (3, 0), (3, -1), (4, 0), (4, 7), (4, 12), (5, 0), (5, 7), (5, 14), (6, 0), (6, -8), (6, 12), (13, 0), (13, -1), (13, 65536),
                (14, -1), (14, 4), (14, 1000)]
        for k, v in bads:
            bad = list(good)
            bad[k] = v
            assert lib.tb_canvas_gather(*bad) == TB_EINVAL, ("gather", k, v)
        for t in bad_tables:
            assert lib.tb_canvas_gather(*(good[:7] + t + good[13:])) == TB_EINVAL
        # step: x, eps_all, m_prev, xh, n, Hc, Wc, S, tables(6), Bu, g, alpha_t, sigma_t, ca, cb, cc
        good_s = [L.ptr(xg.t), L.ptr(eg.t), L.ptr(mg.t), L.ptr(hg.t), n, Hc, Wc, S] + tables() + [Bu] + list(STEP) + [L.stream()]
        for k, v in [(0, None), (1, None), (2, None), (4, 0), (4, -1), (4, 16384), (5, 0), (5, 7), (6, 0), (6, 7), (7, 0), (7, 12), (14, 0),
                     (14, 65536), (16, 0.0)]:
            bad = list(good_s)
            bad[k] = v
            assert lib.tb_canvas_step(*bad) == TB_EINVAL, ("step", k, v)
        for t in bad_tables:
            assert lib.tb_canvas_step(*(good_s[:8] + t + good_s[14:])) == TB_EINVAL
        # blend: tiles, ld, image, rgbx, n, Hp, Wp, P, tables(6), ramp
        tg = Guarded(torch.full((n * 6 * S * S, 4), 0.25), 5.0)
        ig, bg = Guarded(torch.full((n, 3, Hc, Wc), 9.0), 7.0), Guarded(torch.full((n, Hc, Wc), -3, dtype=torch.int32), 7)
        good_b = [L.ptr(tg.t), 4, L.ptr(ig.t), L.ptr(bg.t), n, Hc, Wc, S] + tables() + [3, L.stream()]
        for k, v in [(0, None), (1, 2), (1, 0), (4, 0), (4, -1), (5, 0), (5, 7), (6, 0), (6, 7), (7, 0), (7, 12), (14, 0), (14, -2)]:
            bad = list(good_b)
            bad[k] = v
            assert lib.tb_tile_blend(*bad) == TB_EINVAL, ("blend", k, v)
        bad = list(good_b)
        bad[2] = bad[3] = None                                                            # no output at all
        assert lib.tb_tile_blend(*bad) == TB_EINVAL
        for t in bad_tables:
            assert lib.tb_tile_blend(*(good_b[:8] + t + good_b[14:])) == TB_EINVAL
        torch.cuda.synchronize()
        for g_, v in ((xg, 2.0), (mg, 3.0), (hg, 4.0), (x2, 9.0), (eg, 1.0), (ig, 9.0), (bg, -3), (tg, 0.25)):
            assert g_.intact() and bool((g_.t == v).all())                               # nothing was launched
        assert lib.tb_canvas_gather(*good) == 0 and lib.tb_canvas_step(*good_s) == 0 and lib.tb_tile_blend(*good_b) == 0
        torch.cuda.synchronize()
        assert bool((x2.t == 4.0).all()) and not bool((xg.t == 2.0).any()) and bool(((ig.t - 0.625).abs() < 1e-6).all())
        assert all(g_.intact() for g_ in (xg, mg, hg, x2, eg, ig, bg, tg))


# ------------------------------------------------------------------------------------------------ the sampler on the tiny model directory
STEPS = 4


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    from tests.test_compose_host import write_run
    from tests.test_gpu_generate import D_TEXT, write_model_dir
    from textboost_amd import generate as G
    root = tmp_path_factory.mktemp("canvas")
    mdir, rdir = str(root / "model"), str(root / "runs" / "dog")
    write_model_dir(mdir, hw=16)
    write_run(rdir, ["<dog>"], ["<hflip>"], seed=1, rank=4, keep_rows="even")
    B = 4
    with torch.no_grad():
        pipe = G.Pipeline.from_model_dir(mdir, B, steps=STEPS, guidance=7.5, device=dev)
    g = torch.Generator().manual_seed(3)
    cond = torch.randn(77, D_TEXT, generator=g).half().float().repeat(B, 1).to(dev)      # one prompt for every row
    uncond = torch.randn(77, D_TEXT, generator=g).half().float().repeat(B, 1).to(dev)
    return dict(root=root, mdir=mdir, rdir=rdir, pipe=pipe, B=B, cond=cond, uncond=uncond)


def test_a_model_sized_canvas_is_denoise_and_images_bit_for_bit(tiny):
    from textboost_amd import generate as G
    pipe, smp = tiny["pipe"], tiny["pipe"].sampler
    lat = torch.cat([G.seeded_canvas_latent(s, 16, 16) for s in range(4)]).to(dev)
    with torch.no_grad():
        plain = smp.denoise(tiny["cond"], tiny["uncond"], latents=lat).clone()
        canvas = smp.denoise_canvas(tiny["cond"], tiny["uncond"], lat)
        assert smp.canvas_plan.nw == 1 and smp.canvas_plan.n_chunks == 1
        assert torch.equal(bits(canvas), bits(plain))
        img = pipe.images(tiny["cond"], tiny["uncond"], lat).clone()
        cimg = pipe.canvas_images(tiny["cond"], tiny["uncond"], lat)
        assert tuple(cimg.shape) == (4, 128, 128) and cimg.dtype == torch.int32 and torch.equal(cimg, img)
        assert torch.equal(bits(smp.denoise(tiny["cond"], tiny["uncond"], latents=lat)), bits(plain))      # the plain path afterwards: its bits


def test_a_wide_canvas_replays_step_by_step_and_repeats(tiny):
    """16 x 24 at stride 4: 3 windows, 2 seeds, 6 pairs in chunks of 4 + 2.  Every step is rebuilt from the trace: the reference gather (of the
    fp32 canvas before step 0, of the step's own 16-bit canvas afterwards: the UNet's input is `tb_dpm_step`'s conversion, see
    `HipSampler.denoise_canvas`), the device UNet, the float64 step; m_prev comes from the previous replayed step, in float64 for the
    reference and in float32 for the yardstick."""
    from textboost_amd import _lib as L
    from textboost_amd import generate as G
    pipe, smp = tiny["pipe"], tiny["pipe"].sampler
    Sm, Bu = 16, 4
    lat = torch.cat([G.seeded_canvas_latent(s, 16, 24) for s in (0, 1)]).to(dev)
    with torch.no_grad():
        out = smp.denoise_canvas(tiny["cond"], tiny["uncond"], lat, stride=4, keep_trace=True).clone()
        plan = smp.canvas_plan
        assert (plan.oy, plan.ox, plan.pairs, [len(c) for c in plan.chunks()]) == ([0], [0, 4, 8], 6, [4, 2])
        trace, trace_h = smp.canvas_trace.cpu().numpy(), smp.canvas_trace_h.float().cpu().numpy()
        assert tuple(trace.shape) == (STEPS + 1, 2, 4, 16, 24) and np.array_equal(trace[0], lat.cpu().numpy())
        assert torch.equal(torch.from_numpy(trace[STEPS]), out.cpu()) and np.isfinite(trace).all()
        ehs = torch.cat([tiny["uncond"], tiny["cond"]]).to(L.half_dtype()).contiguous()
        m64, m32 = np.zeros(trace[0].shape), np.zeros(trace[0].shape, dtype=np.float32)
        for i in range(STEPS):
            src = trace[0] if i == 0 else trace_h[i]
            eps_all = np.zeros((plan.n_chunks, 2 * Bu, 4, Sm, Sm), dtype=np.float32)
            for c in range(plan.n_chunks):
                smp.x2.copy_(R.gather(src, Sm, plan.oy, plan.ox, Bu, c, "fp16").to(dev))
                eps_all[c] = smp.forward_step(i, ehs).float().cpu().numpy()
            a_t, s_t = smp.sch.data_prediction_scalars(i)
            sc = (smp.g, a_t, s_t) + tuple(smp.sch.coefficients(i))
            want, m64n = R.step(trace[i], m64, eps_all, Sm, plan.oy, plan.ox, Bu, *sc)
            yard, m32n = R.step(trace[i], m32, eps_all, Sm, plan.oy, plan.ox, Bu, *sc, dtype=np.float32)
            bound = MARGIN * np.abs(yard.astype(np.float64) - want).max()
            err = np.abs(trace[i + 1].astype(np.float64) - want).max()
            print(f"[canvas] replay step {i}: error {err:.3e}, float32 yardstick {bound / MARGIN:.3e}, ratio {err / (bound / MARGIN):.2f}")
            assert bound > 0 and err <= bound, (i, err, bound)
            m64, m32 = m64n, m32n
        again = smp.denoise_canvas(tiny["cond"], tiny["uncond"], lat, stride=4)
        assert torch.equal(bits(again), bits(out)) and bool(torch.isfinite(again).all())
        rgbx = pipe.canvas_images(tiny["cond"], tiny["uncond"], lat, stride=4)
        assert tuple(rgbx.shape) == (2, 128, 192) and torch.equal(rgbx, pipe.canvas_images(tiny["cond"], tiny["uncond"], lat, stride=4))
        assert int((rgbx >> 24).abs().max()) == 0                                         # X = 0


def test_canvas_refusals(tiny):
    from textboost_amd.canvas import CanvasError
    from textboost_amd.sampler import HipSampler
    smp = tiny["pipe"].sampler
    lat = torch.zeros(1, 4, 16, 24, device=dev)
    for bad, kw, exc in ((torch.zeros(1, 4, 15, 24, device=dev), {}, CanvasError), (lat, {"stride": 0}, CanvasError),
                         (lat, {"stride": 17}, CanvasError), (lat.half(), {}, ValueError), (lat[:, :3], {}, ValueError)):
        with pytest.raises(exc):
            smp.denoise_canvas(tiny["cond"], tiny["uncond"], bad, **kw)
    anc = HipSampler(tiny["pipe"].unet, tiny["pipe"].vae, steps=STEPS, scheduler="DDPMScheduler")
    with pytest.raises(NotImplementedError, match="DPM-Solver\\+\\+ scheduler only, not on DDPMAncestral"):
        anc.denoise_canvas(tiny["cond"], tiny["uncond"], lat)


def test_captured_canvas_denoise_replays_bit_identically(tiny):
    from textboost_amd import generate as G
    smp = tiny["pipe"].sampler
    lat = torch.cat([G.seeded_canvas_latent(s, 16, 24) for s in (0, 1)]).to(dev)
    with torch.no_grad():
        eager = smp.denoise_canvas(tiny["cond"], tiny["uncond"], lat, stride=4).clone()      # also the warm-up: the plan's tables exist
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):                     # no host synchronisation inside the loop
            out = smp.denoise_canvas(tiny["cond"], tiny["uncond"], lat, stride=4)
        for _ in range(2):
            out.fill_(float("nan"))
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(bits(out), bits(eager))


# ------------------------------------------------------------------------------------------------ the CLI
def _child(cmd, cwd):
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, os.path.join(ROOT, "inference.py")] + cmd, capture_output=True, text=True, cwd=cwd)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def test_cli_writes_a_wide_grid_and_a_model_sized_canvas_is_the_plain_image(tiny):
    pytest.importorskip("transformers")
    from PIL import Image
    common = [tiny["rdir"], "--model", tiny["mdir"], "--prompt", "a <dog> dog on a beach", "--seeds", "0", "1", "--steps", "3", "--output", "g.png"]
    grids = {}
    for name, extra in (("plain", []), ("square", ["--width", "128", "--height", "128"]), ("wide", ["--width", "192", "--height", "128"])):
        wd = str(tiny["root"] / name)
        os.makedirs(wd)
        _child(common + extra, wd)
        grids[name] = np.asarray(Image.open(os.path.join(wd, "g.png")))
    assert grids["wide"].shape == (128, 2 * 192, 3)                                       # one 192 x 128 tile per seed
    assert grids["plain"].shape == (128, 2 * 128, 3) and np.array_equal(grids["square"], grids["plain"])
    assert not np.array_equal(grids["wide"][:, :128], grids["plain"][:, :128])
