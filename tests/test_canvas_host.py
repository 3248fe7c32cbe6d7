"""The MultiDiffusion canvas on the host (inference.py --width / --height; textboost_amd/canvas.py): the window geometry against
tests/canvas_ref.py and known tables, the chunking of the image-window pairs, the linearity that lets ONE solver step on the averaged noise
prediction stand for a step per window, the blend weights, and the CLI's refusals, which come before the device is consulted."""
import os
import re

import numpy as np
import pytest
import torch

import canvas_ref as R


# ------------------------------------------------------------------------------------------------ geometry
KNOWN = [((20, 8, 4), [0, 4, 8, 12]), ((21, 8, 4), [0, 4, 8, 12, 13]), ((13, 8, 3), [0, 3, 5]), ((16, 8, 8), [0, 8]), ((8, 8, 4), [0]),
         ((8, 8, 1), [0]), ((10, 8, 1), [0, 1, 2]), ((256, 64, 16), list(range(0, 193, 16)))]


@pytest.mark.parametrize("args,want", KNOWN, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else None)
def test_known_offset_tables(args, want):
    from textboost_amd.canvas import axis_offsets
    assert axis_offsets(*args) == want == R.offsets(*args)


def test_offsets_cover_every_cell_and_increase():
    from textboost_amd.canvas import axis_offsets
    for S in (1, 3, 8, 16):
        for L in range(S, 4 * S + 3):
            for s in range(1, S + 1):
                o = axis_offsets(L, S, s)
                assert o == R.offsets(L, S, s)
                assert o[0] == 0 and o[-1] == L - S and len(o) == -(-(L - S) // s) + 1
                assert all(b > a for a, b in zip(o, o[1:])) and all(b - a <= S for a, b in zip(o, o[1:]))
                covered = np.zeros(L, dtype=int)
                for k in o:
                    covered[k:k + S] += 1
                assert (covered > 0).all(), (L, S, s)
                assert L != S or o == [0]


def test_plan_windows_pairs_and_chunks():
    from textboost_amd.canvas import CanvasPlan
    p = CanvasPlan(8, 11, 13, 3, n_images=3, unet_batch=4)
    assert p.oy == [0, 3] and p.ox == [0, 3, 5] and (p.ny, p.nx, p.nw) == (2, 3, 6) and p.pairs == 18
    assert p.windows() == [(0, 0), (0, 3), (0, 5), (3, 0), (3, 3), (3, 5)]            # k = iy * nx + ix
    assert [p.pair(q) for q in (0, 5, 6, 17)] == [(0, 0), (0, 5), (1, 0), (2, 5)]      # p = img * nw + k
    ch = p.chunks()
    assert p.n_chunks == 5 and [len(c) for c in ch] == [4, 4, 4, 4, 2] and sum(ch, []) == list(range(18))      # a ragged last chunk
    assert CanvasPlan(8, 8, 20, 4, 1, 13).chunks() == [[0, 1, 2, 3]]
    assert [len(c) for c in CanvasPlan(8, 8, 20, 4, 3, 3).chunks()] == [3, 3, 3, 3]  # chunks that fit exactly
    assert [len(c) for c in CanvasPlan(8, 8, 8, 4, 3, 13).chunks()] == [3]
    sd = CanvasPlan(64, 64, 256, 16, 1, 13)
    assert sd.nw == 13 and sd.n_chunks == 1                                          # 512 x 2048 at the default stride: one UNet launch
    assert CanvasPlan(64, 64, 256, 16, 4, 13).n_chunks == 4
    oy, ox, _, _ = p.tables("cpu")
    assert oy.dtype == torch.int32 and oy.tolist() == [0, 3] and ox.tolist() == [0, 3, 5]
    assert p.tables("cpu", 8)[1].tolist() == [0, 24, 40]
    with pytest.raises(IndexError):
        p.pair(18)


def test_plan_refusals():
    from textboost_amd.canvas import CanvasError, CanvasPlan
    assert issubclass(CanvasError, ValueError)
    for args, msg in (((8, 7, 20, 4), "below the window"), ((8, 20, 7, 4), "below the window"), ((8, 8, 20, 0), "stride 0"),
                      ((8, 8, 20, 9), "stride 9"), ((8, 8, 20, -1), "stride -1"), ((8, 8 + 64, 8 + 64, 1), "4225 windows"),
                      ((8, 8, 20, 4, 0), "0 images"), ((8, 8, 20, 4, 1, 0), "UNet batch 0")):
        with pytest.raises(CanvasError, match=msg):
            CanvasPlan(*args)
    assert CanvasPlan(8, 8 + 63, 8 + 63, 1).nw == 4096


def test_seeded_canvas_latent_is_the_square_latent_at_the_models_size():
    from textboost_amd.generate import seeded_canvas_latent, seeded_latent
    for s in (0, 3, 12345):
        assert torch.equal(seeded_canvas_latent(s, 16, 16), seeded_latent(s, 16))
    x = seeded_canvas_latent(1, 16, 24)
    assert tuple(x.shape) == (1, 4, 16, 24) and x.dtype == torch.float32 and torch.equal(x, x.half().float())
    assert torch.equal(x, seeded_canvas_latent(1, 16, 24)) and not torch.equal(x, seeded_canvas_latent(2, 16, 24))


# ------------------------------------------------------------------------------------------------ linearity
def test_one_canvas_step_on_averaged_eps_equals_stepping_every_window():
    """float64, two consecutive steps (so m_prev is live): per-window solver states, averaged after the step, against the canvas's one step"""
    from textboost_amd.sampler import DPMSolverPP2M
    rng = np.random.RandomState(0)
    S, Hc, Wc, n, Bu, g = 8, 11, 13, 2, 4, 7.5
    oy, ox = R.offsets(Hc, S, 3), R.offsets(Wc, S, 3)
    pl = R.pairs(n, oy, ox)
    sch = DPMSolverPP2M()
    sch.set_timesteps(4)
    x = rng.standard_normal((n, 4, Hc, Wc))
    canvas_x, canvas_m = x.copy(), np.zeros_like(x)
    win_m = [np.zeros((4, S, S)) for _ in pl]
    cur = x.copy()
    for i in (0, 1):
        a_t, s_t = sch.data_prediction_scalars(i)
        ca, cb, cc = sch.coefficients(i)
        eu, ec = rng.standard_normal((len(pl), 4, S, S)), rng.standard_normal((len(pl), 4, S, S))
        # (a) every window steps with its own m_prev; the canvas is the average of the windows' results
        total, count = np.zeros_like(x), np.zeros_like(x)
        for p, (img, y, xx) in enumerate(pl):
            xv = cur[img, :, y:y + S, xx:xx + S]
            eps = eu[p] + g * (ec[p] - eu[p])
            m0 = (xv - s_t * eps) / a_t
            total[img, :, y:y + S, xx:xx + S] += ca * xv + cb * m0 + cc * win_m[p]
            count[img, :, y:y + S, xx:xx + S] += 1
            win_m[p] = m0
        cur = total / count
        # (b) the canvas: averaged eps, one step, m_prev on the canvas
        eps_all = np.zeros((-(-len(pl) // Bu), 2 * Bu, 4, S, S))
        for p in range(len(pl)):
            eps_all[p // Bu, p % Bu], eps_all[p // Bu, Bu + p % Bu] = eu[p], ec[p]
        canvas_x, canvas_m = R.step(canvas_x, canvas_m, eps_all, S, oy, ox, Bu, g, a_t, s_t, ca, cb, cc)
        err = R.rel_err(canvas_x, cur)
        print(f"[canvas] linearity, step {i}: relative difference {err:.2e}")
        assert err <= 1e-12
    assert cc != 0.0                                                                 # the second step used m_prev


def test_float32_restatement_is_close_to_float64():
    rng = np.random.RandomState(1)
    S, oy, ox = 8, [0], R.offsets(21, 8, 4)
    x, mp = rng.standard_normal((1, 4, 8, 21)).astype(np.float32), rng.standard_normal((1, 4, 8, 21)).astype(np.float32)
    eps = R.scatter_eps((rng.standard_normal((5, 4, 8, 8)).astype(np.float32), rng.standard_normal((5, 4, 8, 8)).astype(np.float32)), 3)
    a = R.step(x, mp, eps, S, oy, ox, 3, 7.5, 0.8, 0.6, 0.9, 0.3, -0.1)
    b = R.step(x, mp, eps, S, oy, ox, 3, 7.5, 0.8, 0.6, 0.9, 0.3, -0.1, dtype=np.float32)
    assert b[0].dtype == np.float32 and 0 < R.rel_err(b[0], a[0]) < 1e-5 and R.rel_err(b[1], a[1]) < 1e-5


# ------------------------------------------------------------------------------------------------ blend reference
def test_blend_weights_are_positive_and_feather_only_shared_edges():
    P, R_ = 8, 3
    for Lp, origins in ((8, [0]), (20, [0, 6, 12]), (13, [0, 5])):
        for O in origins:
            w = np.array([R.axis_weight(O + t, O, P, Lp, R_) for t in range(P)])
            assert (w > 0).all() and (w <= 1).all()
            assert (O != 0) or w[0] == 1.0                      # an edge of the image is not feathered
            assert (O + P != Lp) or w[-1] == 1.0
            assert (O == 0) or w[0] == pytest.approx(1 / R_)
            assert (O + P == Lp) or w[-1] == pytest.approx(1 / R_)
    w = R.weight_map(6, 0, 8, 20, 8, 3)
    assert w.shape == (8, 8) and (w > 0).all() and np.allclose(w[:, 0], w[:, 7])
    assert np.allclose(w[:, 3], [1 / 3, 2 / 3, 1, 1, 1, 1, 2 / 3, 1 / 3])


def test_blend_of_constant_tiles_is_the_constant_and_one_tile_is_the_identity():
    rng = np.random.RandomState(2)
    P, ty, tx, Hp, Wp = 8, R.offsets(11, 8, 3), R.offsets(13, 8, 3), 11, 13
    tiles = np.full((2 * len(ty) * len(tx), P, P, 3), 0.37, dtype=np.float32)
    for ramp in (1, 3, 8, 20):
        val, ws = R.blend(tiles, 2, P, ty, tx, Hp, Wp, ramp)
        assert (ws > 0).all() and np.abs(val - np.float32(0.37)).max() < 1e-15
    one = rng.standard_normal((3, P, P, 3)).astype(np.float32)
    val, ws = R.blend(one, 3, P, [0], [0], P, P, 5)
    assert (ws == 1).all() and np.array_equal(val, one.transpose(0, 3, 1, 2).astype(np.float64))
    assert np.array_equal(R.blend(one, 3, P, [0], [0], P, P, 5, dtype=np.float32)[0], one.transpose(0, 3, 1, 2))


# ------------------------------------------------------------------------------------------------ the CLI
def test_cli_refusals_come_before_the_device_is_consulted(tmp_path, monkeypatch):
    pytest.importorskip("transformers")
    import inference
    from PIL import Image
    from tests.test_compose_host import write_run
    from tests.test_gpu_generate import write_model_dir
    mdir = str(tmp_path / "model")
    write_model_dir(mdir, hw=16)                                 # S = 16 latent cells, VAE factor 8: the model's size is 128 pixels
    da = str(tmp_path / "runs" / "dog")
    write_run(da, ["<dog>"], ["<hflip>"], seed=1, rank=4, keep_rows="even")
    photo = str(tmp_path / "photo.png")
    Image.fromarray(np.zeros((32, 32, 3), dtype=np.uint8)).save(photo)

    def consulted():
        raise AssertionError("torch.cuda was consulted")
    monkeypatch.setattr(torch.cuda, "is_available", consulted)
    common = [da, "--model", mdir, "--prompt", "a <dog> dog on a beach"]
    p = inference.build_parser()
    a = p.parse_args(["run"])
    assert a.width is None and a.height is None and a.window_stride is None
    W = ["--width", "192"]
    for extra, msg in ((["--window-stride", "4"], "--window-stride needs --width PX or --height PX"),
                       (W + ["--init-image", photo], "--width / --height do not go with --init-image"),
                       (W + ["--mask", photo], "--width / --height do not go with --mask"),
                       (W + ["--invert-image", photo], "--width / --height do not go with --invert-image"),
                       (W + ["--edit-prompt", "a dog"], "--width / --height do not go with --edit-prompt"),
                       (W + ["--reweight", "dog=2"], "--width / --height do not go with --reweight"),
                       (W + ["--region", "dog=0,0,0.5,1"], "--width / --height do not go with --region"),
                       (W + ["--excite", "dog"], "--width / --height do not go with --excite"),
                       (W + ["--attn-map"], "--width / --height do not go with --attn-map"),
                       (["--height", "256", "--blend", "dog"], "--width / --height do not go with --blend"),
                       (["--width", "120"], "--width 120: a multiple of 8 (the VAE's factor) from 128 (the model's size) to 8192"),
                       (["--width", "196"], "--width 196: a multiple of 8"),
                       (["--height", "64"], "--height 64: a multiple of 8"),
                       (["--height", "8200"], "--height 8200: a multiple of 8"),
                       (W + ["--window-stride", "0"], "--window-stride: stride 0: 1 .. 16"),
                       (W + ["--window-stride", "17"], "--window-stride: stride 17: 1 .. 16"),
                       (["--width", "640", "--height", "640", "--window-stride", "1"], "4225 windows per image: at most 4096")):
        with pytest.raises(SystemExit, match=re.escape(msg)) as ei:
            inference.main(common + extra)
        assert ei.value.code not in (0, None), extra
        assert "does not go with" not in msg or ": " in str(ei.value.code).split(msg, 1)[1]      # one sentence of reason each
    # accepted arguments pass every host check and reach the device question
    for extra in (W, ["--height", "128", "--width", "128"], ["--height", "136"], W + ["--window-stride", "16"],
                  W + ["--weights", "0.5"], ["--width", "8192", "--window-stride", "16"]):
        with pytest.raises(AssertionError, match="consulted"):
            inference.main(common + extra)
    got = inference.check_canvas_flags(p.parse_args(common + ["--width", "192"]))
    assert got == {"Hc": 16, "Wc": 24, "stride": 4, "S": 16, "factor": 8}
    assert inference.check_canvas_flags(p.parse_args(common + ["--height", "192", "--window-stride", "5"]))["stride"] == 5
    assert inference.check_canvas_flags(p.parse_args(common)) is None
