"""Prompt-to-prompt LocalBlend on the host (inference.py --blend; textboost_amd/local_blend.py): the float32 definition of the
mask (tests/blend_ref.py, what the GPU tests compare bytes with) against the literal float64 formulation, its edge cases, the host tables and
the command line's refusals.

The margin.  The literal formulation computes P / mx > th in float64; the definition computes P > fl32(th mx) on fp32 sums.  m is a sum of
n_pos fp32 terms (n_pos - 1 roundings, relative error <= (n_pos - 1) 2^-24 on non-negative terms), th mx adds one rounding: the two can
disagree only on a cell with |P / mx - th| <= n_pos 2^-24 (1 + th) -- within 8 n_pos 2^-24 with room.  The cases are seeded so that NO cell
lies inside that margin (asserted), so the two masks must be equal everywhere."""
import json
import os
import re
import types

import numpy as np
import pytest
import torch

import blend_ref as R

@pytest.mark.parametrize("shape,seed", R.CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_float32_definition_is_the_literal_float64_formulation(shape, seed):
    n, T, hl, wl, h, w = shape
    acc, words = R.make_case(shape, seed)
    rng = np.random.RandomState(seed + 1)
    limit = (rng.uniform(size=h * w) < 0.6).astype(np.uint8) * 3
    for lim in (None, limit):
        mask, area = R.blend_mask(acc, words, hl, wl, h, w, R.TH, limit=lim)
        lit, closest = R.blend_mask_literal(acc, words, hl, wl, h, w, R.TH, limit=lim)
        inside = closest <= R.margin(words.shape[1])
        print(f"[blend] {shape} seed {seed}: closest |P / mx - th| {closest:.3e} (margin {R.margin(words.shape[1]):.3e}), area {area.tolist()}")
        assert not inside, "a cell of the reference lies within rounding of the threshold: pick another seed"        # 0 cells in the margin
        assert np.array_equal(mask, lit)
        assert mask.dtype == np.uint8 and set(np.unique(mask)) <= {0, 255} and np.array_equal(area, (mask.reshape(n, -1) != 0).sum(1))
    if hl * wl >= 16:
        full, _ = R.blend_mask(acc, words, hl, wl, h, w, R.TH)
        assert 0 < int((full != 0).sum()) < full.size       # the cases are not trivial


def _flat(shape, value=0.25):
    n, T, hl, wl, h, w = shape
    return np.full((2 * n, T, hl * wl), value, dtype=np.float32), np.tile(np.array([[1, 0, -1, -1]], dtype=np.int32), (2 * n, 1))


def test_edge_cases_of_the_definition():
    shape = (1, 4, 4, 5, 8, 10)
    n, T, hl, wl, h, w = shape
    acc, words = _flat(shape)
    # a constant map: P == mx everywhere, th < 1 passes, th = 1 is the strict compare P > mx: nothing
    assert (R.blend_mask(acc, words, hl, wl, h, w, 1.0)[0] == 0).all()
    assert (R.blend_mask(acc, words, hl, wl, h, w, 0.3)[0] == 255).all()
    rng = np.random.RandomState(0)
    pos = rng.uniform(0.1, 1.0, size=acc.shape).astype(np.float32)
    m0, a0 = R.blend_mask(pos, words, hl, wl, h, w, 0.0)
    assert (m0 == 255).all() and a0.tolist() == [h * w]                      # th = 0 on positive maps: everything
    for th in (1.0, 1.5, 2.0):
        assert (R.blend_mask(pos, words, hl, wl, h, w, th)[0] == 0).all()     # th >= 1: nothing
    empty = np.full_like(words, -1)
    me, ae = R.blend_mask(pos, empty, hl, wl, h, w, 0.0)
    assert (me == 0).all() and ae.tolist() == [0]                            # an empty table: nothing, even at th = 0
    assert (R.blend_mask(np.zeros_like(pos), words, hl, wl, h, w, 0.3)[0] == 0).all()     # an all-zero map: 0 > 0 is false


def test_a_word_in_one_prompt_only_contributes_through_that_row():
    shape = (1, 4, 4, 4, 8, 8)
    n, T, hl, wl, h, w = shape
    acc = np.full((2, T, 16), 0.01, dtype=np.float32)
    acc[0, 1, 0] = 1.0        # source row: token 1 peaks in the top-left corner
    acc[1, 2, 15] = 1.0       # edited row: token 2 peaks in the bottom-right corner
    words = np.full((2, 4), -1, dtype=np.int32)
    words[0, 0] = 1
    only_src, _ = R.blend_mask(acc, words, hl, wl, h, w, 0.3)
    want = np.zeros((8, 8), dtype=np.uint8)
    want[:4, :4] = 255        # the 3 x 3 pool clipped at the corner: coarse cells (0..1, 0..1), each 2 x 2 fine cells
    assert np.array_equal(only_src[0], want)
    words[1, 0] = 2
    both, area = R.blend_mask(acc, words, hl, wl, h, w, 0.3)
    want[4:, 4:] = 255
    assert np.array_equal(both[0], want) and area.tolist() == [32]
    words[0, 0] = -1
    only_edit, _ = R.blend_mask(acc, words, hl, wl, h, w, 0.3)
    want_edit = np.zeros((8, 8), dtype=np.uint8)
    want_edit[4:, 4:] = 255
    assert np.array_equal(only_edit[0], want_edit)
    # the limit ANDs
    limit = np.zeros((8, 8), dtype=np.uint8)
    limit[:, :6] = 1
    words[0, 0] = 1
    lim, area = R.blend_mask(acc, words, hl, wl, h, w, 0.3, limit=limit)
    assert np.array_equal(lim[0], want * (limit != 0)) and area.tolist() == [16 + 8]


def test_the_pool_is_clipped_at_corners_and_edges():
    hl, wl = 5, 6
    for (py, px) in ((0, 0), (0, 3), (4, 5), (2, 0), (2, 3), (4, 2)):
        acc = np.zeros((2, 2, hl * wl), dtype=np.float32)
        acc[0, 1, py * wl + px] = 1.0
        words = np.array([[1], [-1]], dtype=np.int32)
        mask, area = R.blend_mask(acc, words, hl, wl, hl, wl, 0.5)
        want = np.zeros((hl, wl), dtype=np.uint8)
        want[max(py - 1, 0):py + 2, max(px - 1, 0):px + 2] = 255
        assert np.array_equal(mask[0], want), (py, px)
        assert area[0] == (min(py + 1, hl - 1) - max(py - 1, 0) + 1) * (min(px + 1, wl - 1) - max(px - 1, 0) + 1)


def test_host_tables_and_schedule():
    from tests.test_p2p_host import StubTokenizer
    from textboost_amd import local_blend as B
    assert B.start_step(0.2, 25) == 5 and B.start_step(0.0, 4) == 0 and B.start_step(1.0, 4) == 4 and B.start_step(0.25, 4) == 1
    assert B.start_step(0.58, 50) == 29                    # rounded first, as the other fractions of the sampler
    for bad in (-0.1, 1.01, float("nan"), float("inf")):
        with pytest.raises(B.BlendError, match="--blend-start"):
            B.start_step(bad, 10)
    assert B.check_threshold(0.0) == 0.0 and B.check_threshold(2) == 2.0
    for bad in (-0.5, float("nan"), float("inf")):
        with pytest.raises(B.BlendError, match="--blend-threshold"):
            B.check_threshold(bad)
    assert B.position_row([5, 2, 5], 77, 4) == [2, 5, -1, -1] and B.position_row([], 77, 2) == [-1, -1]
    with pytest.raises(B.BlendError, match="at most 4"):
        B.position_row(range(5), 77, 4)
    with pytest.raises(B.BlendError, match="outside"):
        B.position_row([77], 77)
    tok = StubTokenizer()
    src, edt, found = B.word_positions(tok, "a dog on a beach", "a fluffy <dog> dog on a beach", ["dog", "<dog>"], 77)
    assert found["dog"]["source"] == src and found["<dog>"]["source"] == [] and len(found["<dog>"]["edit"]) >= 1
    assert set(found["dog"]["edit"]) | set(found["<dog>"]["edit"]) == set(edt) and src and len(edt) > len(src)
    with pytest.raises(ValueError, match="'cat' does not occur"):
        B.word_positions(tok, "a dog on a beach", "a fluffy dog on a beach", ["dog", "cat"], 77)
    assert (B.START, B.THRESHOLD) == (0.2, 0.3)


def test_sampler_refusals():
    from textboost_amd.sampler import HipSampler
    unet = types.SimpleNamespace(B=8, T=77, H=16, W=16, blend=None)
    ctl = types.SimpleNamespace(n=2, T=77, h=16, w=16, start=0.2, n_pos=16)
    s = types.SimpleNamespace(unet=unet, B=4, steps=4)
    f = HipSampler._blend_start
    assert f(s, None, None, object(), object(), object(), object()) is None      # without a control nothing is refused here
    with pytest.raises(ValueError, match="blend without p2p"):
        f(s, ctl, None, None, None, None, None)
    for k, name in enumerate(("maps", "regions", "excite")):
        args = [None] * 3
        args[k] = object()
        with pytest.raises(ValueError, match=f"does not go with {name}"):
            f(s, ctl, object(), *args, None)
    for other in (dict(n=1), dict(T=20), dict(h=8)):
        with pytest.raises(ValueError, match="control is built for"):
            f(s, types.SimpleNamespace(**{**vars(ctl), **other}), object(), None, None, None, None)
    with pytest.raises(ValueError, match="one pair"):
        f(s, ctl, object(), None, None, None, object())
    with pytest.raises(ValueError, match="--blend-start"):
        f(s, types.SimpleNamespace(**{**vars(ctl), "start": 1.5}), object(), None, None, None, None)
    assert unet.blend is None and not hasattr(s, "_blend_bufs")


def test_enable_blend_refusals():
    from textboost_amd.unet import HipUNet
    with pytest.raises(NotImplementedError, match="16-bit kernels only"):
        HipUNet.enable_blend(types.SimpleNamespace(dtype=torch.float32))
    shallow = types.SimpleNamespace(dtype=torch.float16, B=4, T=77, H=16, W=16, BLEND_LEVEL=2, xattn=[("a.attn2", 64), ("b.attn2", 64)],
                                    xattn_level={"a.attn2": 0, "b.attn2": 1})
    with pytest.raises(ValueError, match="levels \\[0, 1\\] only"):
        HipUNet.enable_blend(shallow)
    with pytest.raises(ValueError, match="batch 4n"):
        HipUNet.enable_blend(types.SimpleNamespace(**{**vars(shallow), "B": 6}))


def test_cli_refusals_come_before_the_device_is_consulted(tmp_path, monkeypatch):
    pytest.importorskip("transformers")
    import inference
    from tests.test_compose_host import write_run
    from tests.test_gpu_generate import _write_tokenizer
    mdir = str(tmp_path / "model")
    _write_tokenizer(os.path.join(mdir, "tokenizer"))
    os.makedirs(os.path.join(mdir, "unet"))
    with open(os.path.join(mdir, "unet", "config.json"), "w") as f:
        json.dump({"sample_size": 16}, f)
    da = str(tmp_path / "runs" / "dog")
    write_run(da, ["<dog>"], ["<hflip>"], seed=1, rank=4, keep_rows="even")
    photo = str(tmp_path / "photo.png")
    from PIL import Image
    Image.fromarray(np.zeros((32, 32, 3), dtype=np.uint8)).save(photo)

    def consulted():
        raise AssertionError("torch.cuda was consulted")
    monkeypatch.setattr(torch.cuda, "is_available", consulted)
    common = [da, "--model", mdir, "--prompt", "a dog on a beach"]
    E = ["--edit-prompt", "a <dog> dog on a beach"]
    p = inference.build_parser()
    a = p.parse_args(["run"])
    assert a.blend is None and a.blend_start is None and a.blend_threshold is None
    a = p.parse_args(["run", "--blend", "dog", "<dog>", "--blend-start", "0.4", "--blend-threshold", "0.5"])
    assert a.blend == ["dog", "<dog>"] and (a.blend_start, a.blend_threshold) == (0.4, 0.5)
    for extra, msg in ((["--blend", "dog"], "--blend needs --edit-prompt TEXT or --reweight WORD=F"),
                       (["--blend-start", "0.5"], "--blend-start needs --blend"),
                       (["--blend-threshold", "0.5"], "--blend-threshold needs --blend"),
                       (E + ["--blend-start", "0.5"], "--blend-start needs --blend"),
                       (E + ["--blend", "dog", "--blend-start", "1.5"], "--blend-start 1.5"),
                       (E + ["--blend", "dog", "--blend-start", "-0.1"], "--blend-start -0.1"),
                       (E + ["--blend", "dog", "--blend-start", "nan"], "--blend-start nan"),
                       (E + ["--blend", "dog", "--blend-threshold", "-1"], "--blend-threshold -1.0: a finite number >= 0"),
                       (E + ["--blend", "dog", "--blend-threshold", "inf"], "--blend-threshold inf: a finite number >= 0"),
                       (E + ["--blend", "dog", "--blend-threshold", "nan"], "--blend-threshold nan: a finite number >= 0"),
                       (E + ["--blend", "dog", "--region", "dog=0,0,0.5,1"], "--edit-prompt does not go with --region"),
                       (E + ["--blend", "dog", "--attn-map"], "--edit-prompt does not go with --attn-map"),
                       (E + ["--blend", "dog", "--init-image", photo], "--edit-prompt does not go with --init-image"),
                       (E + ["--blend", "dog", "--excite", "dog"], "--excite does not go with --edit-prompt"),
                       (E + ["--blend", "dog", "bird"], "--blend: 'bird' does not occur in the first 77 tokens")):
        with pytest.raises(SystemExit, match=re.escape(msg)) as ei:
            inference.main(common + extra)
        assert ei.value.code not in (0, None), extra
    # accepted arguments pass every host check and reach the device question; a word of one prompt only is accepted
    for extra in (E + ["--blend", "dog"], E + ["--blend", "<dog>"], E + ["--blend", "dog", "<dog>", "--blend-start", "0", "--blend-threshold", "2"],
                  ["--reweight", "dog=2", "--blend", "dog"]):
        with pytest.raises(AssertionError, match="consulted"):
            inference.main(common + extra)
    args = p.parse_args(common + E + ["--blend", "dog", "<dog>", "--blend-start", "0.5"])
    run = inference.load_runs(args)
    got = inference.check_blend_args(args, run, inference.check_p2p_args(args, run), inference.check_blend_flags(args))
    assert got["words"] == ["dog", "<dog>"] and got["start"] == 0.5 and got["threshold"] == 0.3
    assert got["found"]["<dog>"]["source"] == [] and got["found"]["<dog>"]["edit"] and got["found"]["dog"]["source"] == got["source"]
    assert set(got["edit"]) == set(got["found"]["dog"]["edit"]) | set(got["found"]["<dog>"]["edit"])
    assert inference.blend_stem(p.parse_args(["run", "--output", "out/grid.jpg"])) == "out/grid_blend"
