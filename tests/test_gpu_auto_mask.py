"""Subject masks from cross-attention on the GPU (csrc/auto_mask.hip, textboost_amd/auto_mask.py, make_masks.py, inference.py --mask auto:WORD;
DESIGN.md 17): every entry point through the C ABI against tests/auto_mask_ref.py, in both builds of the library; the whole device chain on a
planted attention signal; `MaskMaker` and the two command lines on the tiny model directory of tests/test_gpu_generate.py.

Each stage's reference consumes the DEVICE output of the stage before it (the histogram takes the device's min / max, the mask the device's
threshold), so a one-ulp difference upstream cannot flip a bin downstream.

Bounds.  tb_map_word_upsample: per element (nb npos + 6) 2^-23 weight sum|terms| -- nb npos fp32 additions in index order, then six more
roundings (two interpolations, the weight, the accumulating add); with accumulate = 1 the previous content is one more term of that sum.
Everything behind it is exact: min / max, integer counts, Otsu's bin on inputs with a unique maximiser, mask bytes.

The issue plants an all-black auto mask with a constant photo; that does not work as stated: every UNet row adds its own noise to the
encoded photo, so the attention of a constant photo is not constant (test_mask_maker_on_the_tiny_model prints its min and max).  The
refusal of an all-black mask is therefore pinned in two halves: a constant SCORE gives threshold (1, 255) and an all-zero mask here
(test_mask_from_score_*), and inference.py ends on an all-zero prepared mask (tests/test_auto_mask_host.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import auto_mask_ref as R

pytestmark = pytest.mark.gpu
dev = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TB_EINVAL = -22
HALVES = ["fp16", "bf16"]


def f32(v):
    return float(np.float32(v))


# ------------------------------------------------------------------------------------------------ tb_map_word_upsample
UPSAMPLE_CASES = [(3, 7, 5, 5, 13, 9), (2, 77, 8, 8, 64, 64), (1, 128, 16, 16, 10, 23)]


@pytest.mark.parametrize("half", HALVES)
@pytest.mark.parametrize("case", UPSAMPLE_CASES, ids=lambda c: "x".join(map(str, c)))
def test_map_word_upsample_matches_the_float64_reference(case, half):
    from textboost_amd import _lib as L
    from textboost_amd import ops
    nb, T, h, w, H, W = case
    rng = np.random.default_rng(17)
    acc_h = rng.uniform(0.0, 1.0, size=(nb, T, h * w)).astype(np.float32)
    acc_h[:, :, ::7] *= 1e-3                                   # cells of another scale
    weight = 1.0 / (3 * nb * 2)
    with L.use_half(half):
        acc = torch.from_numpy(acc_h).to(dev)
        for npos in (1, 3, T):
            positions = sorted(rng.choice(T, size=npos, replace=False).tolist())
            ref, mag = R.word_upsample(acc_h, h, w, positions, weight, H, W)
            bound = R.upsample_bound(nb, npos, mag)
            score = torch.full((H, W), float("nan"), device=dev)
            ops.map_word_upsample(acc, h, w, positions, weight, score)
            got = score.cpu().double().numpy()
            ratio = (np.abs(got - ref) / bound).max()
            print(f"[auto mask] upsample {half} {case} npos {npos}: worst error / bound {ratio:.3f}")
            assert np.isfinite(got).all() and ratio <= 1.0
            again = torch.full((H, W), float("nan"), device=dev)
            ops.map_word_upsample(acc, h, w, positions, weight, again)
            assert torch.equal(again, score)                   # a second launch: the same bits
            prev_h = rng.normal(size=(H, W)).astype(np.float32)
            summed = torch.from_numpy(prev_h).to(dev)
            ops.map_word_upsample(acc, h, w, positions, weight, summed, accumulate=True)
            err = np.abs(summed.cpu().double().numpy() - (ref + prev_h.astype(np.float64)))
            ratio = (err / R.upsample_bound(nb, npos, mag + np.abs(prev_h.astype(np.float64)))).max()
            print(f"[auto mask] upsample {half} {case} npos {npos} accumulate: worst error / bound {ratio:.3f}")
            assert ratio <= 1.0


def test_map_word_upsample_refuses_bad_arguments_and_writes_nothing():
    import ctypes
    from textboost_amd import _lib as L
    nb, T, h, w, H, W = 2, 7, 5, 5, 13, 9
    lib = L.lib()
    acc = torch.rand(nb, T, h * w, device=dev)
    big = torch.rand(1, 129, h * w, device=dev)
    score = torch.full((H, W), 7.0, device=dev)
    pos = (ctypes.c_int32 * 3)(1, 2, 6)
    good = [L.ptr(acc), nb, T, h, w, pos, 3, 0.5, L.ptr(score), H, W, 0, L.stream()]
    bad_pos = (ctypes.c_int32 * 3)(1, 2, T)
    neg_pos = (ctypes.c_int32 * 3)(-1, 2, 3)
    for k, v in ((6, 0), (5, bad_pos), (5, neg_pos), (0, None), (5, None), (8, None), (6, T + 1), (1, 0), (3, 0), (3, 129), (4, 129), (9, 0),
                 (10, 0), (11, 2)):
        bad = list(good)
        bad[k] = v
        assert lib.tb_map_word_upsample(*bad) == TB_EINVAL, (k, v)
    over = [L.ptr(big), 1, 129, h, w, pos, 3, 0.5, L.ptr(score), H, W, 0, L.stream()]        # T > 128
    assert lib.tb_map_word_upsample(*over) == TB_EINVAL
    torch.cuda.synchronize()
    assert (score == 7.0).all()                                # a refused call launched nothing
    assert lib.tb_map_word_upsample(*good) == 0
    torch.cuda.synchronize()
    assert (score != 7.0).all()


# ------------------------------------------------------------------------------------------------ tb_score_range
@pytest.mark.parametrize("half", HALVES)
def test_score_range_is_torch_min_max(half):
    from textboost_amd import _lib as L
    from textboost_amd import ops
    g = torch.Generator().manual_seed(3)
    with L.use_half(half):
        ws = torch.zeros(ops.SCORE_RANGE_WS, device=dev)
        for n in (1, 255, 256, 257, 2 ** 20 + 3):
            base = torch.randn(n + 1, generator=g)
            boundary = 1024 if n > 1025 else n // 2            # the first element of the second workgroup's first 16-byte load
            for pmin, pmax in ((0, n - 1), (n - 1, 0), (boundary, max(boundary - 1, 0))):
                for offset in (0, 1):                          # offset 1: the buffer does not start on a 16-byte boundary
                    x = base.clone()
                    if n > 1:
                        x[offset + pmax] = 50.0
                        x[offset + pmin] = -60.0
                    xd = x.to(dev)[offset:offset + n]
                    for scratch in (ws, None):
                        mm = torch.full((2,), float("nan"), device=dev)
                        ops.score_range(xd, mm, scratch)
                        assert mm[0].item() == xd.min().item() and mm[1].item() == xd.max().item(), (n, pmin, pmax, offset, scratch is None)
        lib = L.lib()
        mm = torch.zeros(2, device=dev)
        assert lib.tb_score_range(None, 4, L.ptr(mm), None, L.stream()) == TB_EINVAL
        assert lib.tb_score_range(L.ptr(ws), 4, None, None, L.stream()) == TB_EINVAL
        assert lib.tb_score_range(L.ptr(ws), 0, L.ptr(mm), None, L.stream()) == TB_EINVAL


# ------------------------------------------------------------------------------------------------ tb_score_hist
@pytest.mark.parametrize("half", HALVES)
def test_score_hist_equals_the_fp32_restatement(half):
    from textboost_amd import _lib as L
    from textboost_amd import ops
    g = torch.Generator().manual_seed(5)
    with L.use_half(half):
        ws = torch.zeros(ops.SCORE_RANGE_WS, device=dev)
        for n in (1000, 2 ** 18 + 5):
            x = torch.randn(n, generator=g)
            xd = x.to(dev)
            mm = ops.score_range(xd, torch.zeros(2, device=dev), ws)
            lo, hi = mm.cpu().numpy()                          # the device's own range feeds the reference
            hist = torch.full((256,), 12345, dtype=torch.int32, device=dev)       # dirty on entry
            ops.score_hist(xd, mm, hist)
            got = hist.cpu().numpy().astype(np.int64)
            want = R.hist256(x.numpy(), lo, hi)
            assert got.sum() == n and np.array_equal(got, want), n
            assert got[255] >= 1 and R.hist256(x.numpy()[[int(x.argmax())]], lo, hi)[255] == 1      # the maximum lands in bin 255
            ops.score_hist(xd, mm, hist)
            assert np.array_equal(hist.cpu().numpy(), got)     # the previous counts do not matter
        c = torch.full((777,), 0.3, device=dev)
        mm = ops.score_range(c, torch.zeros(2, device=dev))
        hist = ops.score_hist(c, mm, torch.full((256,), -1, dtype=torch.int32, device=dev)).cpu()
        assert hist[0].item() == 777 and hist[1:].sum().item() == 0
        lib = L.lib()
        assert lib.tb_score_hist(L.ptr(c), 777, L.ptr(mm), None, L.stream()) == TB_EINVAL
        assert lib.tb_score_hist(L.ptr(c), 0, L.ptr(mm), L.ptr(hist.to(dev)), L.stream()) == TB_EINVAL


# ------------------------------------------------------------------------------------------------ tb_otsu_threshold
def _bimodal(seed, centres, counts, spread, floor):
    """two normal bumps on a floor of `floor` counts per bin: an empty bin beside the best k would tie with it (the criterion does not move
    across a bin without mass), and the test needs a unique maximiser"""
    rng = np.random.default_rng(seed)
    v = np.concatenate([rng.normal(c, spread, size=k) for c, k in zip(centres, counts)])
    return np.bincount(np.clip(np.rint(v), 0, 255).astype(np.int64), minlength=256) + floor


OTSU_HISTS = {"two_bumps": _bimodal(1, (60, 180), (5000, 2000), 12.0, 3), "small_peak": _bimodal(2, (30, 220), (200000, 9000), 20.0, 7)}


@pytest.mark.parametrize("half", HALVES)
def test_otsu_threshold_picks_the_reference_bin(half):
    from textboost_amd import _lib as L
    from textboost_amd import ops
    with L.use_half(half):
        for name, hist_h in OTSU_HISTS.items():
            margin = R.otsu_margin(hist_h)
            assert margin > 1e-9, (name, margin)              # a condition on the INPUT: its maximiser is unique
            thr_ref, k_ref = R.otsu(hist_h)
            assert 0 < k_ref < 255
            thr = torch.full((2,), float("nan"), device=dev)
            ops.otsu_threshold(torch.from_numpy(hist_h.astype(np.int32)).to(dev), thr)
            got = thr.cpu().numpy()
            print(f"[auto mask] otsu {half} {name}: bin {int(got[1])} (reference {k_ref}), margin to the runner-up {margin:.2e}")
            assert int(got[1]) == k_ref and got[0] == thr_ref
        one = np.zeros(256, dtype=np.int32)
        one[91] = 4242
        thr = ops.otsu_threshold(torch.from_numpy(one).to(dev), torch.zeros(2, device=dev)).cpu().numpy()
        assert thr[0] == np.float32(1.0) and thr[1] == np.float32(255.0)
        tie = np.zeros(256, dtype=np.int32)
        tie[[3, 200]] = 5, 9                                   # every k in 3 .. 199 has the same criterion: the smallest
        thr = ops.otsu_threshold(torch.from_numpy(tie).to(dev), torch.zeros(2, device=dev)).cpu().numpy()
        assert thr[1] == 3.0 and thr[0] == np.float32(4 / 256)
        assert L.lib().tb_otsu_threshold(None, L.ptr(torch.zeros(2, device=dev)), L.stream()) == TB_EINVAL


# ------------------------------------------------------------------------------------------------ tb_mask_from_score
@pytest.mark.parametrize("half", HALVES)
def test_mask_from_score_is_bit_equal_in_both_modes(half):
    from textboost_amd import _lib as L
    from textboost_amd import ops
    g = torch.Generator().manual_seed(9)
    with L.use_half(half):
        # generic data: range and threshold from the device's own stages
        x = torch.randn(5003, generator=g) * 3.0 + 1.0
        xd = x.to(dev)
        mm = ops.score_range(xd, torch.zeros(2, device=dev))
        hist = ops.score_hist(xd, mm, torch.zeros(256, dtype=torch.int32, device=dev))
        thr = ops.otsu_threshold(hist, torch.zeros(2, device=dev))
        lo, hi = mm.cpu().numpy()
        t0 = thr.cpu().numpy()[0]
        for soft in (False, True):
            got = ops.mask_from_score(xd, mm, thr, torch.full((5003,), 99, dtype=torch.uint8, device=dev), soft=soft).cpu().numpy()
            want = R.mask_from_score(x.numpy(), lo, hi, t0, soft)
            assert np.array_equal(got, want), soft
            assert got[int(x.argmin())] == 0 and got[int(x.argmax())] == 255
        # planted: lo = 0 and hi = 1, so t is the score itself; elements at lo, at hi, exactly at the threshold and one ulp below it, and
        # the ties of the soft mode: 255 t = 127.5 -> 128, 63.75 -> 64, (2k + 1) / 510 -> k or k + 1 by the parity of k where the fp32
        # product is the tie exactly
        ties = [np.float32((2 * k + 1) / 510.0) for k in range(0, 255, 7)]
        planted = np.array([0.0, 1.0, 0.5, np.nextafter(np.float32(0.5), np.float32(0)), 0.25, 0.75, 0.1, 0.9] + ties, dtype=np.float32)
        pd = torch.from_numpy(planted).to(dev)
        mm = ops.score_range(pd, torch.zeros(2, device=dev))
        assert mm.cpu().tolist() == [0.0, 1.0]
        thr = torch.tensor([0.5, 127.0], device=dev)
        hard = ops.mask_from_score(pd, mm, thr, torch.zeros(planted.size, dtype=torch.uint8, device=dev)).cpu().numpy()
        assert list(hard[:4]) == [0, 255, 255, 0] and np.array_equal(hard, R.mask_from_score(planted, 0.0, 1.0, 0.5, False))
        soft = ops.mask_from_score(pd, mm, thr, torch.zeros(planted.size, dtype=torch.uint8, device=dev), soft=True).cpu().numpy()
        assert list(soft[:6]) == [0, 255, 128, 127, 64, 191] and np.array_equal(soft, R.mask_from_score(planted, 0.0, 1.0, 0.5, True))
        exact = [(k, s) for k, s in zip(range(0, 255, 7), soft[8:]) if np.float32(255.0) * np.float32((2 * k + 1) / 510.0) == k + 0.5]
        assert exact and all(s == (k if k % 2 == 0 else k + 1) for k, s in exact)     # half to even
        # a constant score: min == max, one occupied bin, threshold (1, 255), nothing is foreground in either mode
        c = torch.full((300,), 2.5, device=dev)
        mm = ops.score_range(c, torch.zeros(2, device=dev))
        thr = ops.otsu_threshold(ops.score_hist(c, mm, torch.zeros(256, dtype=torch.int32, device=dev)), torch.zeros(2, device=dev))
        assert thr.cpu().tolist() == [1.0, 255.0]
        for soft_mode in (False, True):
            assert not ops.mask_from_score(c, mm, thr, torch.ones(300, dtype=torch.uint8, device=dev), soft=soft_mode).any()
        lib = L.lib()
        m = torch.zeros(300, dtype=torch.uint8, device=dev)
        assert lib.tb_mask_from_score(L.ptr(c), L.ptr(mm), L.ptr(thr), L.ptr(m), 300, 2, L.stream()) == TB_EINVAL
        assert lib.tb_mask_from_score(L.ptr(c), L.ptr(mm), None, L.ptr(m), 300, 0, L.stream()) == TB_EINVAL


# ------------------------------------------------------------------------------------------------ tb_mask_dilate
@pytest.mark.parametrize("half", HALVES)
@pytest.mark.parametrize("case", [(9, 7, 0), (33, 17, 1), (70, 65, 8), (40, 40, 64)], ids=lambda c: "x".join(map(str, c)))
def test_mask_dilate_is_the_clipped_square_maximum(case, half):
    from textboost_amd import _lib as L
    from textboost_amd import ops
    W, H, r = case
    rng = np.random.default_rng(W * 1000 + H)
    m = ((rng.random((H, W)) < 0.02) * rng.integers(1, 256, (H, W))).astype(np.uint8)
    m[0, 0], m[H - 1, W - 1] = 200, 100                       # the corners: the clipped squares
    assert 0 < (m != 0).sum() < H * W
    with L.use_half(half):
        md = torch.from_numpy(m).to(dev)
        out = ops.mask_dilate(md, r, out=torch.full((H, W), 77, dtype=torch.uint8, device=dev))
        assert np.array_equal(out.cpu().numpy(), R.dilate(m, r))
        assert np.array_equal(md.cpu().numpy(), m)
        if r == 0:
            assert torch.equal(out, md)
        lib = L.lib()
        assert lib.tb_mask_dilate(L.ptr(md), L.ptr(out), W, H, 65, L.stream()) == TB_EINVAL
        assert lib.tb_mask_dilate(L.ptr(md), L.ptr(out), W, H, -1, L.stream()) == TB_EINVAL
        assert lib.tb_mask_dilate(L.ptr(md), L.ptr(md), W, H, 1, L.stream()) == TB_EINVAL
        assert lib.tb_mask_dilate(L.ptr(md), None, W, H, 1, L.stream()) == TB_EINVAL


# ------------------------------------------------------------------------------------------------ the chain on a planted signal
def _chain(acc, h, w, positions, weight, H, W, soft=False, dilate=0):
    """the six entry points by hand on one accumulator -> (score, mask, minmax, thr)"""
    from textboost_amd import ops
    score = ops.map_word_upsample(acc, h, w, positions, weight, torch.empty(H, W, device=dev))
    mm = ops.score_range(score, torch.zeros(2, device=dev), torch.zeros(ops.SCORE_RANGE_WS, device=dev))
    hist = ops.score_hist(score, mm, torch.zeros(256, dtype=torch.int32, device=dev))
    thr = ops.otsu_threshold(hist, torch.zeros(2, device=dev))
    mask = ops.mask_from_score(score, mm, thr, torch.empty(H, W, dtype=torch.uint8, device=dev), soft=soft)
    if dilate:
        mask = ops.mask_dilate(mask, dilate)
    return score, mask, mm, thr


def test_chain_finds_a_planted_rectangle():
    """real attention launches, no model: token 5's key is aligned with the queries of a 6 x 7-cell rectangle of the 16 x 16 map"""
    from textboost_amd import _lib as L
    from textboost_amd import ops
    B, heads, side, T, hd = 2, 2, 16, 8, 40
    Sq, H, W = side * side, 96, 80                             # one map cell = 6 x 5 pixels
    y0, y1, x0, x1 = 4, 10, 5, 12                              # rows 4 .. 9, columns 5 .. 11
    g = torch.Generator().manual_seed(21)
    u = torch.zeros(hd)
    u[0] = 1.0
    v = torch.zeros(hd)
    v[1] = 1.0
    inside = torch.zeros(side, side, dtype=torch.bool)
    inside[y0:y1, x0:x1] = True
    q1 = torch.where(inside.view(Sq, 1), 6.0 * u, 6.0 * v)                         # [Sq, hd]: inside along u, the rest orthogonal to it
    keys = 0.05 * torch.randn(T, hd, generator=g)
    keys[:, :2] = 0.0                                                               # the other keys see neither direction
    keys[5] = 8.0 * u
    with L.use_half("fp16"):
        q = q1.repeat(B, heads).half().to(dev)                                      # [B * Sq, heads * hd]
        k = keys.repeat(B, heads).half().to(dev)                                    # [B * T, heads * hd]
        acc = torch.zeros(B, T, Sq, device=dev)
        count = 2
        for _ in range(count):
            ops.attn_token_maps(q, k, acc, B, heads, Sq, T, hd, w=1.0 / heads, accumulate=True)
        weight = 1.0 / (count * B * 1)
        score, mask, mm, thr = _chain(acc, side, side, [5], weight, H, W)
        m = mask.cpu().numpy()
        lo, hi = mm.cpu().tolist()
        print(f"[auto mask] planted rectangle: score in [{lo:.4f}, {hi:.4f}], Otsu bin {int(thr[1].item())}, foreground {100.0 * (m == 255).mean():.1f}%")
        assert set(np.unique(m)) == {0, 255}
        ch, cw = H // side, W // side
        yy, xx = np.mgrid[0:H, 0:W]
        deep_in = (yy >= (y0 + 1) * ch) & (yy < (y1 - 1) * ch) & (xx >= (x0 + 1) * cw) & (xx < (x1 - 1) * cw)
        far_out = (yy < (y0 - 1) * ch) | (yy >= (y1 + 1) * ch) | (xx < (x0 - 1) * cw) | (xx >= (x1 + 1) * cw)
        assert deep_in.sum() == 4 * ch * 5 * cw and far_out.sum() > H * W // 2
        assert (m[deep_in] == 255).all() and (m[far_out] == 0).all()
        # the word at a token that attends nowhere in particular: not the rectangle
        _, other, _, _ = _chain(acc, side, side, [2], weight, H, W)
        o = other.cpu().numpy()
        assert not ((o[deep_in] == 255).all() and (o[far_out] == 0).all())
        assert (o != m).mean() > 0.25


# ------------------------------------------------------------------------------------------------ MaskMaker on the tiny model directory
def _photo(h, w, seed=4):
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    rng = np.random.default_rng(seed)
    img = np.stack([128 + 100 * np.sin(x / 23) * np.cos(y / 31), 128 + 90 * np.cos(x / 17 + y / 29), 60 + 0.8 * x + 0.2 * y], axis=-1)
    return np.clip(img + rng.normal(0, 6, img.shape), 0, 255).astype(np.uint8)


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    """the model directory of tests/test_gpu_generate.py with seeded encoder tensors (as tests/test_gpu_edit.py adds them), one trained run, a
    pipeline for two images (a UNet of 4 rows) and the run's text encoder"""
    pytest.importorskip("transformers")
    from safetensors.torch import load_file, save_file
    from tests.test_gpu_generate import write_model_dir, write_trained_run
    from textboost_amd import generate as G
    from textboost_amd import models
    from textboost_amd.vae import VAEGeometry, vae_encoder_shapes
    d = tmp_path_factory.mktemp("auto_mask")
    mdir, rdir = str(d / "model"), str(d / "runs" / "dog")
    write_model_dir(mdir, hw=16)
    vfile = os.path.join(mdir, "vae", "diffusion_pytorch_model.safetensors")
    vgeo = VAEGeometry(block_out_channels=(64, 64, 128, 128), layers_per_block=1)
    enc_sd = {k: v.half().float() for k, v in models.random_state_dict(vae_encoder_shapes(vgeo), 15, device="cpu").items()}
    save_file({**load_file(vfile), **enc_sd}, vfile)
    write_trained_run(rdir, ["<dog>"], ["<hflip>"], seed=2)
    n = 2
    with torch.no_grad():
        pipe = G.Pipeline.from_model_dir(mdir, n, steps=3, guidance=7.5, device=dev)
        base = G.load_base_text(mdir, dev)
        run = G.read_run_dir(rdir)
        te, tok = G.load_text_encoder(mdir, run, 2 * n, dev, base=base)
        pipe.set_run(run)
    return dict(d=d, mdir=mdir, rdir=rdir, pipe=pipe, te=te, tok=tok)


def test_mask_maker_on_the_tiny_model(tiny):
    from tests.test_gpu_generate import D_TEXT
    from textboost_amd import edit as E
    from textboost_amd import generate as G
    from textboost_amd.attn_maps import cross_attention_maps, token_positions
    from textboost_amd.auto_mask import MaskMaker
    pipe, te, tok = tiny["pipe"], tiny["te"], tiny["tok"]
    rgb = _photo(100, 150)
    g = torch.Generator().manual_seed(3)
    cond = torch.randn(2 * 77, D_TEXT, generator=g).half().float().to(dev)
    uncond = torch.randn(2 * 77, D_TEXT, generator=g).half().float().to(dev)
    lat = torch.cat([G.seeded_latent(s, 16) for s in (0, 1)]).to(dev)
    with torch.no_grad():
        before = pipe.sampler.denoise(cond, uncond, latents=lat).clone()
        enc = E.EditEncoder(tiny["mdir"], pipe.size)
        text_encode = lambda ids: te.forward(ids, pins=False)      # noqa: E731
        maker = MaskMaker(pipe.unet, enc, text_encode, tok, pipe.sampler.sch.alphas_cumprod)
        assert maker.R == 4 and maker.t_dev.tolist() == [100, 300, 500, 100]
        mask, stats = maker.mask(rgb, "dog", dilate=2)
        mask, stats = mask.clone(), stats.clone()
        assert pipe.unet.attn_maps is None
        assert mask.shape == (100, 150) and mask.dtype == torch.uint8 and set(mask.unique().tolist()) <= {0, 255}
        rec = maker.recorder
        assert rec.count == cross_attention_maps(pipe.unet) and sum(rec.count.values()) == len(pipe.unet.xattn)     # one launch per layer
        # by hand on the recorder's accumulators
        from textboost_amd import ops
        positions = token_positions(tok, "a photo of a dog", "dog", 77)
        assert len(positions) == 3                              # d, o, g in the byte-level test vocabulary: a multi-piece word
        score = torch.empty(100, 150, device=dev)
        for i, (hw, acc) in enumerate(rec.acc.items()):
            ops.map_word_upsample(acc, hw[0], hw[1], positions, 1.0 / (rec.count[hw] * 4 * len(rec.acc)), score, accumulate=i > 0)
        mm = ops.score_range(score, torch.zeros(2, device=dev), torch.zeros(ops.SCORE_RANGE_WS, device=dev))
        thr = ops.otsu_threshold(ops.score_hist(score, mm, torch.zeros(256, dtype=torch.int32, device=dev)), torch.zeros(2, device=dev))
        hard = ops.mask_from_score(score, mm, thr, torch.empty(100, 150, dtype=torch.uint8, device=dev))
        assert torch.equal(ops.mask_dilate(hard, 2), mask)
        assert torch.equal(torch.cat([mm, thr]), stats)
        assert 0 < (hard == 255).sum() < hard.numel() and float(mm[0]) < float(mm[1])
        score_a = maker.score(rgb, "dog").clone()
        assert torch.equal(score_a, score)
        again, _ = maker.mask(rgb, "dog", dilate=2)
        assert torch.equal(again, mask)                         # a second call: the same bytes
        soft, _ = maker.mask(rgb, "dog", soft=True)
        assert soft.max().item() == 255 and soft.min().item() == 0 and len(soft.unique()) > 2
        other = MaskMaker(pipe.unet, enc, text_encode, tok, pipe.sampler.sch.alphas_cumprod, seed=1)
        assert not torch.equal(other.score(rgb, "dog"), score_a)           # another seed, another noise
        flat = maker.score(np.full((100, 150, 3), 128, dtype=np.uint8), "dog")
        print(f"[auto mask] a constant photo: score in [{flat.min().item():.6g}, {flat.max().item():.6g}] (each row adds its own noise)")
        with pytest.raises(ValueError, match="does not occur|has no tokens"):
            maker.score(rgb, "")
        with pytest.raises(ValueError, match="smaller than"):
            maker.score(_photo(12, 150), "dog")
        after = pipe.sampler.denoise(cond, uncond, latents=lat)
        assert torch.equal(after, before) and pipe.unet.attn_maps is None   # the shared UNet is left as it was found


# ------------------------------------------------------------------------------------------------ the command lines
def _child(cmd, cwd):
    return subprocess.run(["timeout", "-k", "10", "600", sys.executable] + cmd, capture_output=True, text=True, cwd=cwd)


def test_make_masks_cli_writes_what_the_trainer_reads(tiny):
    from PIL import Image
    from textboost_amd import data as D
    d = tiny["d"]
    photos, out, pv = d / "photos", str(d / "masks" / "dog"), str(d / "previews")
    os.makedirs(photos)
    Image.fromarray(_photo(100, 150)).save(str(photos / "one.png"))
    Image.fromarray(_photo(64, 64, seed=5)).save(str(photos / "two.jpg"))
    cmd = [os.path.join(ROOT, "make_masks.py"), str(photos), "--model", tiny["mdir"], "--word", "dog", "--output", out, "--preview-dir", pv,
           "--draws", "1", "--timesteps", "100", "300"]
    r = _child(cmd, str(d))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count("otsu bin") == 2 and "wrote 2 mask(s)" in r.stdout
    sizes = {"one": (150, 100), "two": (64, 64)}
    first = {}
    for stem, size in sizes.items():
        with Image.open(os.path.join(out, stem + ".png")) as im:
            assert im.mode == "L" and im.size == size
        with Image.open(os.path.join(pv, stem + ".jpg")) as im:
            assert im.size == size
        first[stem] = open(os.path.join(out, stem + ".png"), "rb").read()
    assert sorted(os.listdir(out)) == ["one.png", "two.png"]            # the previews are elsewhere
    images = D.instance_image_paths(str(photos))
    assert D.instance_mask_paths(images, out) == [os.path.join(out, "one.png"), os.path.join(out, "two.png")]
    assert D.concept_masks([{"instance_data_dir": str(photos), "instance_mask_dir": out}]) == [[os.path.join(out, "one.png"),
                                                                                                  os.path.join(out, "two.png")]]
    r = _child(cmd, str(d))                                             # the masks exist: refused on the host
    assert r.returncode != 0 and "pass --force" in r.stderr
    r = _child(cmd + ["--force"], str(d))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    for stem in sizes:
        assert open(os.path.join(out, stem + ".png"), "rb").read() == first[stem]


def test_inference_cli_repaints_the_auto_mask_only(tiny):
    from PIL import Image
    from textboost_amd import edit as E
    d = tiny["d"]
    wd = d / "edit"
    os.makedirs(wd)
    rgb = _photo(100, 150)
    Image.fromarray(rgb).save(str(wd / "photo.png"))
    cmd = [os.path.join(ROOT, "inference.py"), tiny["rdir"], "--model", tiny["mdir"], "--prompt", "photo of a <dog> dog", "--init-image",
           "photo.png", "--mask", "auto:dog", "--strength", "0.9", "--steps", "4", "--seeds", "0", "--output", "grid.png"]
    r = _child(cmd, str(wd))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    with Image.open(str(wd / "grid_mask.png")) as im:
        assert im.mode == "L" and im.size == (150, 100)
        mask = im.copy()
    assert set(np.unique(np.asarray(mask))) == {0, 255}
    grid = np.asarray(Image.open(str(wd / "grid.png")).convert("RGB"))
    assert grid.shape == (128, 128, 3)
    pm, _ = E.prepare_mask(mask, 128, cell=8)
    nw, nh, x1, y1 = E.edit_geometry(150, 100, 128)
    prepared = np.asarray(Image.fromarray(rgb).resize((nw, nh), Image.LANCZOS).crop((x1, y1, x1 + 128, y1 + 128)))
    keep = pm == 0
    print(f"[auto mask] inference --mask auto:dog: {100.0 * pm.mean():.1f}% of the prepared photo is repainted")
    assert pm.any() and np.array_equal(grid[keep], prepared[keep])      # outside the mask: the prepared photo's bytes
    assert (grid[~keep] != prepared[~keep]).any()
    r = _child(cmd[:-2] + ["--mask", "auto:"], str(wd))
    assert r.returncode != 0 and "needs a word" in r.stderr
