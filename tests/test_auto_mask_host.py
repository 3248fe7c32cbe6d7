"""Subject masks from cross-attention, host side (no GPU): the reference of tests/auto_mask_ref.py against independent statements, make_masks.py's
argument handling, path mapping and refusals, inference.py's `--mask auto:WORD` arguments, and the binding of the six new entry points."""
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import auto_mask_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN_SUBJECTS = os.path.join(ROOT, "tests", "golden", "sweep_subjects_db.json")


# ------------------------------------------------------------------------------------------------ the reference checks itself
@pytest.mark.parametrize("hw,HW", [((5, 5), (13, 9)), ((8, 8), (64, 64)), ((16, 16), (10, 23)), ((3, 7), (3, 7)), ((4, 6), (1, 1))])
def test_reference_bilinear_is_f_interpolate(hw, HW):
    m = np.random.default_rng(1).normal(size=hw)
    want = F.interpolate(torch.from_numpy(m)[None, None], size=HW, mode="bilinear", align_corners=False)[0, 0].numpy()
    got = R.bilinear(m, *HW)
    assert got.shape == HW and np.abs(got - want).max() <= 1e-14 * np.abs(m).max()


def test_reference_word_upsample_sums_rows_and_positions():
    rng = np.random.default_rng(2)
    acc = rng.uniform(0, 1, size=(3, 7, 25))
    got, mag = R.word_upsample(acc, 5, 5, [2, 4], 0.25, 5, 5)                # same size: the resize is the identity
    want = np.float64(np.float32(0.25)) * (acc[:, 2] + acc[:, 4]).sum(0).reshape(5, 5)
    assert np.abs(got - want).max() < 1e-15 and np.array_equal(got, mag)     # non-negative terms: the magnitudes are the values


def test_reference_otsu_is_the_two_class_variance_split():
    rng = np.random.default_rng(3)
    for trial in range(6):
        hist = np.zeros(256, dtype=np.int64)
        bins = rng.choice(256, size=8, replace=False)
        hist[bins] = rng.integers(1, 30, size=8)
        if R.otsu_margin(hist) < 1e-9:
            continue
        thr, k = R.otsu(hist)
        assert k == R.otsu_brute_force(hist), trial
        assert thr == np.float32((k + 1) / 256.0)
    one = np.zeros(256, dtype=np.int64)
    one[17] = 40
    assert R.otsu(one) == (np.float32(1.0), 255)
    two = np.zeros(256, dtype=np.int64)
    two[[3, 200]] = 5, 9
    assert R.otsu(two)[1] == 3                    # every k in 3 .. 199 splits alike: the smallest wins


def test_reference_dilate_is_the_window_maximum():
    rng = np.random.default_rng(4)
    m = ((rng.random((11, 14)) < 0.05) * rng.integers(1, 256, (11, 14))).astype(np.uint8)
    for r in (0, 1, 3, 20):
        want = np.zeros_like(m)
        for y in range(m.shape[0]):
            for x in range(m.shape[1]):
                want[y, x] = m[max(0, y - r):y + r + 1, max(0, x - r):x + r + 1].max()
        assert np.array_equal(R.dilate(m, r), want), r
    assert np.array_equal(R.dilate(m, 0), m)


def test_reference_histogram_and_mask_edges():
    s = np.array([1.0, 1.5, 2.0, 3.0], dtype=np.float32)
    h = R.hist256(s, 1.0, 3.0)
    assert h.sum() == 4 and h[0] == 1 and h[64] == 1 and h[128] == 1 and h[255] == 1      # the maximum lands in the last bin
    assert R.hist256(np.full(9, 2.5, np.float32), 2.5, 2.5)[0] == 9
    assert list(R.mask_from_score(s, 1.0, 3.0, 0.5, soft=False)) == [0, 0, 255, 255]       # t == thr is foreground
    assert list(R.mask_from_score(s, 1.0, 3.0, 0.5, soft=True)) == [0, 64, 128, 255]       # 63.75 -> 64, 127.5 -> 128 (half to even)
    assert list(R.mask_from_score(np.float32([0.0, 0.5 / 255, 1.5 / 255, 1.0]), 0.0, 1.0, 0.5, soft=True)) == [0, 0, 2, 255]


# ------------------------------------------------------------------------------------------------ make_masks.py
def _model_dir(d, sample_size=16, encoder=True):
    from safetensors.torch import save_file
    os.makedirs(os.path.join(d, "unet"))
    os.makedirs(os.path.join(d, "vae"))
    with open(os.path.join(d, "unet", "config.json"), "w") as f:
        json.dump({"sample_size": sample_size}, f)
    sd = {"decoder.conv_in.weight": torch.zeros(1)}
    if encoder:
        sd.update({"encoder.conv_in.weight": torch.zeros(1), "quant_conv.weight": torch.zeros(1)})
    save_file(sd, os.path.join(d, "vae", "diffusion_pytorch_model.safetensors"))
    return str(d)


def _photo(path, w, h):
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(np.full((h, w, 3), 90, dtype=np.uint8)).save(path)
    return path


def _plan(argv):
    import make_masks as M
    return M.plan(M.build_parser().parse_args(argv))


@pytest.fixture()
def world(tmp_path):
    model = _model_dir(tmp_path / "model")
    data = tmp_path / "data" / "dog"
    _photo(str(data / "b.jpg"), 40, 30)
    _photo(str(data / "a.png"), 64, 64)
    (data / "notes.txt").write_text("not an image")
    return dict(model=model, data=str(data), tmp=tmp_path)


def test_first_form_maps_every_image_to_a_png_of_its_stem(world):
    out = str(world["tmp"] / "masks" / "dog")
    jobs = _plan([world["data"], "--model", world["model"], "--word", "dog", "--output", out, "--preview-dir", str(world["tmp"] / "pv")])
    assert [(os.path.basename(p), w, m, v) for p, w, m, v in jobs] == [
        ("a.png", "dog", os.path.join(out, "a.png"), str(world["tmp"] / "pv" / "a.jpg")),
        ("b.jpg", "dog", os.path.join(out, "b.png"), str(world["tmp"] / "pv" / "b.jpg"))]
    one = _plan([world["data"], "--model", world["model"], "--word", "dog", "--output", out, "-n", "1"])
    assert [os.path.basename(j[0]) for j in one] == ["a.png"] and one[0][3] is None       # the first N entries, as the trainer counts them
    import make_masks as M
    args = M.build_parser().parse_args([world["data"], "--model", world["model"], "--word", "dog", "--output", out])
    assert (args.timesteps, args.draws, args.seed, args.soft, args.dilate, args.prompt) == ([100, 300, 500], 2, 0, False, 0, "a photo of a {}")


def test_second_form_writes_where_the_sweep_reads(world):
    from textboost_amd import sweep
    with open(GOLDEN_SUBJECTS) as f:
        table = json.load(f)
    names = ["backpack", "bear_plushie"]
    root = world["tmp"] / "db"
    for n in names:
        _photo(str(root / n / "00.jpg"), 48, 32)
    out = str(world["tmp"] / "masks")
    jobs = _plan(["--data-dir", str(root), "--model", world["model"], "--output", out, "--instances", *names])     # --subjects: the default table
    words = {s["name"]: s["class_token"] for s in table}
    assert [(j[0], j[1], j[2]) for j in jobs] == [(str(root / n / "00.jpg"), words[n], os.path.join(out, n, "00.png")) for n in names]
    assert words["bear_plushie"] == "stuffed animal"                       # a two-word class token goes through as it is
    sargs = sweep.db_parser().parse_args(["--model-dir", world["model"], "--data-dir", str(root), "--mask-root", out, "--instances", *names])
    _, sjobs = sweep.build_db(sargs)
    for (name, argv), n in zip(sjobs, names):
        flags = dict(a.split("=", 1) for a in argv if a.startswith("--") and "=" in a)
        mine = [j for j in jobs if os.path.dirname(j[2]) == flags["--instance_mask_dir"]]
        assert name == n and len(mine) == 1 and os.path.dirname(mine[0][0]) == flags["--instance_data_dir"]
    with pytest.raises(SystemExit, match="no such subject"):
        _plan(["--data-dir", str(root), "--model", world["model"], "--output", out, "--instances", "nobody"])


def test_refusals_come_before_any_device(world, monkeypatch):
    import make_masks as M
    out = str(world["tmp"] / "masks")
    base = [world["data"], "--word", "dog"]
    with pytest.raises(SystemExit, match="is the data directory"):
        _plan(base + ["--model", world["model"], "--output", world["data"] + "/"])
    with pytest.raises(SystemExit, match="is not a directory"):
        _plan(base + ["--model", str(world["tmp"] / "nowhere"), "--output", out])
    with pytest.raises(SystemExit, match="is not a directory"):
        _plan(base + ["--model", "runwayml/stable-diffusion-v1-5", "--output", out])
    with pytest.raises(SystemExit, match="alias of a hub repository"):
        _plan(base + ["--model", "sd15", "--output", out])
    with pytest.raises(SystemExit, match="--model DIR"):
        _plan(base + ["--output", out])
    with pytest.raises(SystemExit, match="--word WORD is required"):
        _plan([world["data"], "--model", world["model"], "--output", out])
    with pytest.raises(SystemExit, match="--dilate 65"):
        _plan(base + ["--model", world["model"], "--output", out, "--dilate", "65"])
    with pytest.raises(SystemExit, match=r"no \{\} for the word"):
        _plan(base + ["--model", world["model"], "--output", out, "--prompt", "a photo"])
    noenc = _model_dir(world["tmp"] / "noenc", encoder=False)
    with pytest.raises(SystemExit, match=r"no encoder\.\*"):
        _plan(base + ["--model", noenc, "--output", out])
    # an existing mask
    os.makedirs(out)
    open(os.path.join(out, "b.png"), "wb").close()
    with pytest.raises(SystemExit, match="pass --force"):
        _plan(base + ["--model", world["model"], "--output", out])
    assert len(_plan(base + ["--model", world["model"], "--output", out, "--force"])) == 2
    # a photo smaller than the latent grid (16 x 16 here) in one direction
    small = world["tmp"] / "small"
    _photo(str(small / "s.png"), 40, 10)
    with pytest.raises(SystemExit, match="smaller than the 16 x 16 latent grid"):
        _plan([str(small), "--word", "dog", "--model", world["model"], "--output", str(world["tmp"] / "m2")])
    # everything in order and no GPU: the usual ending, after the checks
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(SystemExit, match="needs an MI355X"):
        M.main(base + ["--model", world["model"], "--output", str(world["tmp"] / "m3")])
    assert not os.path.exists(str(world["tmp"] / "m3"))


def test_photo_size_check_warns_above_aspect_two():
    from textboost_amd import auto_mask as A
    with pytest.warns(UserWarning, match="aspect ratio"):
        A.check_photo_size(210, 100, 16, 16)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        A.check_photo_size(200, 100, 16, 16)
    with pytest.raises(ValueError, match="smaller than"):
        A.check_photo_size(15, 100, 16, 16)


# ------------------------------------------------------------------------------------------------ inference.py --mask auto:WORD
def test_inference_auto_mask_arguments(world):
    import inference as I
    from textboost_amd import auto_mask as A
    assert A.parse_auto_mask("auto:sofa") == ("auto", "sofa")
    assert A.parse_auto_mask("masks/sofa.png") == ("file", "masks/sofa.png")
    with pytest.raises(ValueError, match="needs a word"):
        A.parse_auto_mask("auto:")
    photo = _photo(str(world["tmp"] / "photo.png"), 64, 48)

    def check(*argv):
        return I.check_edit_args(I.build_parser().parse_args(["run", "--model", world["model"], *argv]))

    edit = check("--init-image", photo, "--mask", "auto:sofa", "--dilate", "3")
    assert (edit["auto"], edit["dilate"], edit["mask"]) == ("sofa", 3, None) and edit["rgb"].shape == (48, 64, 3)
    assert check("--init-image", photo, "--mask", "auto:sofa")["dilate"] == 0
    with pytest.raises(SystemExit, match="--mask needs --init-image"):
        check("--mask", "auto:sofa")
    with pytest.raises(SystemExit, match="--dilate needs --init-image"):
        check("--dilate", "2")
    with pytest.raises(SystemExit, match="needs a word"):
        check("--init-image", photo, "--mask", "auto:")
    with pytest.raises(SystemExit, match="--dilate PX goes with --mask auto:WORD"):
        check("--init-image", photo, "--dilate", "2")
    with pytest.raises(SystemExit, match="--dilate PX goes with"):
        check("--init-image", photo, "--mask", "auto:sofa", "--dilate", "65")
    assert check("--init-image", photo)["auto"] is None
    # an all-black prepared mask ends the run instead of writing the photo back
    with pytest.raises(SystemExit, match="no white pixel"):
        I.check_auto_mask(np.zeros((8, 8), dtype=np.uint8), "sofa")
    m = np.zeros((8, 8), dtype=np.uint8)
    m[3, 4] = 1
    I.check_auto_mask(m, "sofa")
    args = I.build_parser().parse_args(["run", "--output", "out/grid.jpg"])
    assert I.auto_mask_path(args) == "out/grid_mask.png"


# ------------------------------------------------------------------------------------------------ the binding
def test_the_six_entry_points_are_declared_and_bound():
    import ctypes as C
    from textboost_amd import _abi, _lib, ops
    sigs = _abi.load()[1]
    V, I, F32, I64 = C.c_void_p, C.c_int, C.c_float, C.c_int64
    want = {"tb_map_word_upsample": [V, I, I, I, I, V, I, F32, V, I, I, I, V], "tb_score_range": [V, I64, V, V, V],
            "tb_score_hist": [V, I64, V, V, V], "tb_otsu_threshold": [V, V, V], "tb_mask_from_score": [V, V, V, V, I64, I, V],
            "tb_mask_dilate": [V, V, I, I, I, V]}
    for name, argtypes in want.items():
        assert sigs[name] == (argtypes, C.c_int), name
        assert _lib._SIGS[name] == sigs[name]
    for fn in ("map_word_upsample", "score_range", "score_hist", "otsu_threshold", "mask_from_score", "mask_dilate"):
        assert callable(getattr(ops, fn))
