"""Attend-and-Excite on the host (textboost_amd/excite.py, inference.py --excite): the float64 reference of the loss against
torch autograd, its tie rule and reflect folding, the margin condition of every case the GPU tests use, the schedule arithmetic, the word
table, the sampler's refusals and every CLI refusal.  No GPU."""
import json
import math
import os
import re
import types

import numpy as np
import pytest
import torch

import excite_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_lib_binds_the_kernels():
    from textboost_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "textboost_hip.h")).read()
    for name in ("tb_excite_loss", "tb_excite_bwd", "tb_excite_update"):
        m = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, f"include/textboost_hip.h does not declare {name}"
        assert len(m.group(1).split(",")) == len(_lib._SIGS[name][0])
    assert os.path.exists(os.path.join(ROOT, "textboost_amd", "csrc", "excite.hip"))
    assert callable(ops.excite_loss) and callable(ops.excite_bwd) and callable(ops.excite_update) and ops.EXCITE_SEL == R.SEL == 9


# ------------------------------------------------------------------------------------------------ the reference itself
@pytest.mark.parametrize("case", R.LOSS_CASES, ids=lambda c: f"{c[0]}x{c[1]}x{c[2]}")
def test_reference_gradient_equals_autograd(case):
    h, w, T, last, words = case
    A = R.loss_inputs(case)
    for b in range(R.NB):
        ref = R.excite_loss_ref(A[b], last, words, h, w, loss_scale=3.0)
        a = A[b].double().clone().requires_grad_(True)
        L = R.loss_torch(a, last, words, h, w)
        L.backward()
        assert abs(L.item() - ref["loss"]) <= 1e-15 and ref["loss"] > 0
        want = torch.zeros_like(a.grad)
        for i, s in enumerate(ref["sel"]):
            if s >= 0:
                want[:, s] = ref["dA"][i] / 3.0
        err = (a.grad - want).abs().max().item()
        print(f"[excite] {case[:4]} image {b}: loss {ref['loss']:.6f}, word {ref['word']}, sel {ref['sel']}, |autograd - reference| {err:.2e}")
        assert err <= 1e-12 * max(1.0, a.grad.abs().max().item())
        assert (a.grad[0] == 0).all() and (a.grad[last:] == 0).all()          # BOS, EOS and the padding are out
        assert abs(sum(ref["kappa"]) - 1.0) <= 1e-15


def test_tie_rule_lowest_word_lowest_position():
    h, w, T, last = 4, 5, 12, 7
    A = torch.full((T, h * w), 0.25)
    ref = R.excite_loss_ref(A, last, [[3], [1, 2], [5]], h, w)
    # a constant map: every word's G is constant; the word with the SMALLEST map is the worst -- the one-token words 0 and 2 tie, 0 wins
    assert ref["word"] == 0 and ref["pos"] == 0
    assert ref["sel"][:4] == [0, 1, w, w + 1] and ref["sel"][4:] == [-1] * 5      # the corner folds onto 2 x 2 positions
    assert abs(ref["loss"] - (1.0 - 1.0 / (last - 1))) <= 1e-15
    ref = R.excite_loss_ref(A, last, [[1, 2], [3], [5]], h, w)
    assert ref["word"] == 1 and ref["pos"] == 0


def test_reflect_folding_at_a_corner_and_an_edge():
    h, w, T, last = 3, 4, 6, 4
    k = R.taps()
    for pos, want in ((h * w - 1, [(h - 2) * w + w - 2, (h - 2) * w + w - 1, (h - 1) * w + w - 2, (h - 1) * w + w - 1]),
                      (1, [0, 1, 2, w, w + 1, w + 2])):
        A = torch.full((T, h * w), 0.01)
        A[2, pos] = 0.2                                        # token 2 peaks at `pos`
        ref = R.excite_loss_ref(A, last, [[2]], h, w)
        assert ref["pos"] == pos and [s for s in ref["sel"] if s >= 0] == want
        assert abs(sum(ref["kappa"]) - 1.0) <= 1e-15
        if len(want) == 4:       # reflect (-1 -> 1): the corner keeps the centre tap alone, the diagonal neighbour collects all four corner taps
            assert abs(ref["kappa"][-1] - float(k[1] ** 2)) <= 1e-15 and abs(ref["kappa"][0] - float(4 * k[0] ** 2)) <= 1e-15
    assert R.reflect(-1, 5) == 1 and R.reflect(5, 5) == 3 and R.reflect(2, 5) == 2


def test_saturated_word_has_zero_loss_and_no_selection():
    h, w, T, last = 4, 4, 8, 4
    A = torch.zeros(T, h * w)
    A[1] = 1.0                                                 # token 1 owns every position: softmax(100 A) is 1 - 2 e^-100 there
    ref = R.excite_loss_ref(A, last, [[1]], h, w)
    assert ref["word"] == 0 and ref["sel"] == [-1] * 9 and (ref["dA"] == 0).all()
    assert ref["loss"] <= 1e-15


# ------------------------------------------------------------------------------------------------ the inputs of the GPU tests
def test_margin_condition_of_every_gpu_case():
    """The best position is separated from the second best, and the worst word from the second worst, by >= 2 % of the value: a flipped
    arg-max on the GPU is then a real failure.  A condition on the inputs (tests/excite_ref.py picks the seeds), not a tolerance."""
    for case in R.LOSS_CASES:
        h, w, T, last, words = case
        A = R.loss_inputs(case)
        for b in range(R.NB):
            ref = R.excite_loss_ref(A[b], last, words, h, w)
            print(f"[excite] margin {case[:4]} image {b}: loss {ref['loss']:.4f}, gap_pos {ref['gap_pos']:.4f}, gap_word {ref['gap_word']:.4f}")
            assert ref["loss"] > 0.05 and ref["gap_pos"] >= R.MIN_GAP and ref["gap_word"] >= R.MIN_GAP, (case, b)


@pytest.mark.parametrize("sd2", [False, True])
def test_margin_condition_of_the_tiny_unet_case(sd2):
    ref_unet = R.tiny_oracle(sd2)
    x, t, ehs = R.unet_inputs(sd2=sd2)
    with torch.no_grad():
        A, _, names, _ = R.oracle_maps(ref_unet.double(), x.double(), t, ehs.double())
    assert len(names) == 5 and tuple(A.shape) == (2, 77, 16)
    for b in range(2):
        ref = R.excite_loss_ref(A[b], R.UNET_LAST, R.UNET_WORDS, 4, 4)
        print(f"[excite] margin tiny UNet sd2={sd2} image {b}: loss {ref['loss']:.4f}, gap_pos {ref['gap_pos']:.4f}, gap_word {ref['gap_word']:.4f}")
        assert ref["loss"] > 0.05 and ref["gap_pos"] >= R.MIN_GAP and ref["gap_word"] >= R.MIN_GAP, b


# ------------------------------------------------------------------------------------------------ schedule, table
def test_schedule_arithmetic():
    from textboost_amd import excite as X
    assert (X.guided_steps(0.5, 50), X.guided_steps(0.5, 25), X.guided_steps(0.5, 4), X.guided_steps(0.0, 9), X.guided_steps(1.0, 9)) == (25, 12, 2, 0, 9)
    assert X.guided_steps(0.58, 50) == 29
    for bad in (-0.1, 1.1, float("nan"), float("inf")):
        with pytest.raises(X.ExciteError, match="--excite-steps"):
            X.guided_steps(bad, 10)
    assert X.refine_thresholds(50) == {0: 0.05, 10: 0.5, 20: 0.8}
    assert X.refine_thresholds(25) == {0: 0.05, 5: 0.5, 10: 0.8}
    assert X.refine_thresholds(4) == {0: 0.5, 1: 0.8}          # floor(0.2 * 4) = 0: the later entry wins
    assert X.step_size(20.0, 0, 50) == 20.0
    assert X.step_size(20.0, 49, 50) == 20.0 * math.sqrt(0.5)
    assert X.step_size(20.0, 24, 50) == 20.0 * math.sqrt(1.0 - 0.5 * 24 / 49)
    assert X.step_size(3.0, 0, 1) == 3.0
    assert (X.EXCITE_STEPS, X.SCALE, X.LOSS_SCALE, X.MAX_REFINE, X.LEVEL) == (0.5, 20.0, 256.0, 20, 2)
    assert math.log2(X.LOSS_SCALE) == int(math.log2(X.LOSS_SCALE))


def test_word_table_from_a_stub_tokenizer():
    from tests.test_attn_maps_host import StubTokenizer
    from textboost_amd import excite as X
    from textboost_amd.attn_maps import token_positions
    tok = StubTokenizer()
    prompt = "a photo of a <dog> dog skateboarding"      # BOS a photo of a <dog>x3 dog skate boarding EOS
    ids = tok(prompt, truncation=True, padding="max_length", max_length=16).input_ids
    last = X.first_eos(ids, tok.eos_token_id)
    assert last == 11
    pos = [token_positions(tok, prompt, w, 16) for w in ("<dog>", "skateboarding", "a")]
    table = X.word_table(pos, last)
    assert len(table) == X.MAX_WORDS and all(len(r) == X.MAX_POSITIONS for r in table)
    assert table[0][:4] == [5, 6, 7, -1] and table[1][:3] == [9, 10, -1] and table[2][:3] == [1, 4, -1] and table[3] == [-1] * 16
    assert X.first_eos([100, 1, 2], 101) == 3                                   # no end token: a truncated prompt
    for bad, msg in (([], "1 .. 8 words"), ([[1]] * 9, "1 .. 8 words"), ([[]], "no token position"), ([[0]], "own tokens"),
                     ([[last]], "own tokens"), ([list(range(1, 18))], "at most 16")):
        with pytest.raises(X.ExciteError, match=msg):
            X.word_table(bad, 30 if len(bad) == 1 and len(bad[0]) > 16 else last)


def test_sampler_refusals():
    from textboost_amd.sampler import HipSampler
    unet = types.SimpleNamespace(B=4, T=77, H=16, W=16, excite=None)
    ctl = types.SimpleNamespace(n=2, T=77, h=16, w=16, excite_steps=0.5)
    s = types.SimpleNamespace(unet=unet, B=2, steps=4)
    f = HipSampler._excite_steps
    assert f(s, None, object(), object(), object(), object()) == 0              # without a control nothing is refused here
    for k, name in enumerate(("maps", "regions", "p2p", "pin")):
        args = [None] * 4
        args[k] = object()
        with pytest.raises(ValueError, match=f"does not go with {name}"):
            f(s, ctl, *args)
    for other in (dict(n=4), dict(T=20), dict(h=8)):
        with pytest.raises(ValueError, match="control is built for"):
            f(s, types.SimpleNamespace(**{**vars(ctl), **other}), None, None, None, None)


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
    da, db = str(tmp_path / "runs" / "dog"), str(tmp_path / "runs" / "cat")
    write_run(da, ["<dog>", "<pet>"], ["<hflip>"], seed=1, rank=4, keep_rows="even")
    write_run(db, ["<cat>", "<pet>"], [], seed=2, rank=4, keep_rows="odd")
    photo = str(tmp_path / "photo.png")
    from PIL import Image
    Image.fromarray(np.zeros((32, 32, 3), dtype=np.uint8)).save(photo)

    def consulted():
        raise AssertionError("torch.cuda was consulted")
    monkeypatch.setattr(torch.cuda, "is_available", consulted)
    prompt = "a <dog> dog and a <cat> cat on a beach"
    common = [da, "--with", db, "--model", mdir, "--prompt", prompt]
    X = ["--excite", "<dog>", "<cat>"]
    p = inference.build_parser()
    a = p.parse_args(["run"])
    assert a.excite is None and a.excite_steps is None and a.excite_scale is None and a.excite_loss_scale is None and not a.no_excite_refine
    a = p.parse_args(["run"] + X + ["--excite-steps", "0.4", "--excite-scale", "10", "--excite-loss-scale", "1024", "--no-excite-refine"])
    assert a.excite == ["<dog>", "<cat>"] and (a.excite_steps, a.excite_scale, a.excite_loss_scale, a.no_excite_refine) == (0.4, 10.0, 1024.0, True)
    for extra, msg in ((X + ["--region", "dog=0,0,0.5,1"], "--excite does not go with --region"),
                       (X + ["--edit-prompt", "a cat"], "--excite does not go with --edit-prompt"),
                       (X + ["--reweight", "dog=2"], "--excite does not go with --reweight"),
                       (X + ["--invert-image", photo], "--excite does not go with --invert-image"),
                       (X + ["--init-image", photo], "--excite does not go with --init-image"),
                       (X + ["--mask", photo], "--excite does not go with --mask"),
                       (X + ["--attn-map"], "--excite does not go with --attn-map"),
                       (["--excite-steps", "0.5"], "--excite-steps needs --excite"),
                       (["--excite-scale", "5"], "--excite-scale needs --excite"),
                       (["--excite-loss-scale", "5"], "--excite-loss-scale needs --excite"),
                       (["--no-excite-refine"], "--no-excite-refine needs --excite"),
                       (X + ["--excite-steps", "1.5"], "--excite-steps 1.5"),
                       (X + ["--excite-steps", "nan"], "--excite-steps nan"),
                       (X + ["--excite-scale", "0"], "--excite-scale 0.0: a finite number > 0"),
                       (X + ["--excite-loss-scale", "-2"], "--excite-loss-scale -2.0: a finite number > 0"),
                       (["--excite"] + ["dog"] * 9, "--excite takes at most 8 words"),
                       (["--excite", "bird"], "--excite: 'bird' does not occur in the first 77 tokens")):
        with pytest.raises(SystemExit, match=re.escape(msg)) as ei:
            inference.main(common + extra)
        assert ei.value.code not in (0, None), extra
    with pytest.raises(SystemExit, match="--excite.*<pet>.*ambiguous"):
        inference.main([da, "--with", db, "--model", mdir, "--prompt", "a dog", "--excite", "<pet>"])
    # accepted arguments pass every host check and reach the device question
    for extra in (X, X + ["--excite-steps", "0.3", "--excite-scale", "10", "--excite-loss-scale", "4096", "--no-excite-refine"], ["--excite", "dog"]):
        with pytest.raises(AssertionError, match="consulted"):
            inference.main(common + extra)
    args = p.parse_args(common + X + ["--excite-steps", "0.3"])
    got = inference.check_excite_args(args, inference.load_runs(args))
    assert got["words"] == ["<dog>", "<cat>"] and len(got["positions"]) == 2 and got["steps"] == 0.3 and got["scale"] == 20.0
    assert got["loss_scale"] == 256.0 and got["refine"] and all(1 <= j < got["last"] for pos in got["positions"] for j in pos)
    assert inference.excite_path(p.parse_args(["run", "--output", "out/grid.jpg"])) == "out/grid_excite.json"
