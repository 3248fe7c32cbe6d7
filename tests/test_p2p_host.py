"""Prompt-to-prompt editing on the host (textboost_amd/p2p.py, inference.py --edit-prompt): token plans of hand-written prompts, the algebra
P^s V1 + P^e V2 = sum_j P_out[j] v_j in float64, step counts from fractions, the sampler's refusals and every CLI refusal."""
import json
import os
import re
import types

import numpy as np
import pytest
import torch

import p2p_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 16


from tests.test_regions_host import StubTokenizer as _RegionsStub


class StubTokenizer(_RegionsStub):
    """the tiny tokenizer of tests/test_regions_host.py with the further words of these prompts"""
    table = dict(_RegionsStub.table, **{"on": [9], "beach": [10], "fluffy": [11], "watercolor": [12], "painting": [13]})


def _plan(src, dst, reweight=()):
    from textboost_amd import p2p
    return p2p.plan(StubTokenizer(), src, dst, T, reweight)


def _entries(M):
    return {(int(i), int(j)): float(M[i, j]) for i, j in np.argwhere(M != 0)}


def _tail(e_s, e_e):
    return {(min(e_s + (j - e_e), T - 1), j): 1.0 for j in range(e_e, T)}


# (source, edit, reweight) of every plan below; the algebra test walks them all
PLANS = {
    "identical": ("a photo of a dog", "a photo of a dog", ()),
    "swap": ("a photo of a dog", "a photo of a cat", ()),
    "one_to_two": ("a dog", "a skateboarding", ()),
    "one_to_three": ("a dog", "a <dog>", ()),
    "added": ("a dog", "a fluffy dog", ()),
    "dropped": ("a fluffy dog", "a dog", ()),
    "placeholder": ("a photo of a dog on a beach", "a photo of a <dog> dog on a beach", ()),
    "prefix": ("dog on a beach", "a watercolor painting of dog on a beach", ()),
    "reweight": ("a fluffy dog", "a fluffy dog", (("fluffy", 2.0),)),
    "added_and_reweight": ("a dog on a beach", "a fluffy <dog> dog on a beach", (("fluffy", 0.5), ("<dog>", 3.0))),
}


def test_header_declares_and_lib_binds_the_kernel():
    from textboost_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "textboost_hip.h")).read()
    m = re.search(r"int\s+tb_attention_dual_fwd\s*\(([^)]*)\)\s*;", hdr)
    assert m, "include/textboost_hip.h does not declare tb_attention_dual_fwd"
    assert len(m.group(1).split(",")) == len(_lib._SIGS["tb_attention_dual_fwd"][0]) == 4
    assert os.path.exists(os.path.join(ROOT, "textboost_amd", "csrc", "p2p_attn.hip"))
    assert callable(ops.attention_dual_fwd)


def test_plan_of_identical_prompts_is_the_identity():
    p = _plan(*PLANS["identical"])
    assert p.M.dtype == np.float32 and p.M.shape == (T, T) and p.a.shape == (T,) and p.w.shape == (T,)
    assert (p.M == np.eye(T, dtype=np.float32)).all() and (p.a == 1).all() and (p.w == 1).all()


def test_plan_of_an_equal_length_swap_maps_in_order():
    p = _plan(*PLANS["swap"])                      # BOS a photo of a dog EOS: dog (5) -> cat (5)
    assert (p.M == np.eye(T, dtype=np.float32)).all() and (p.a == 1).all() and (p.w == 1).all()
    from textboost_amd import p2p
    tok = StubTokenizer()
    tok.table = dict(tok.table, **{"<cat>": [60, 61, 62]})
    q = p2p.plan(tok, "a <dog> on a beach", "a <cat> on a beach", T)      # three vectors -> three vectors: 1-1 in order, not 1/3 each
    assert (q.M == np.eye(T, dtype=np.float32)).all() and (q.a == 1).all()


def test_plan_of_a_one_token_word_to_a_longer_word_spreads_the_weight():
    p = _plan(*PLANS["one_to_two"])                # BOS a dog EOS -> BOS a skate boarding EOS
    assert _entries(p.M) == {(0, 0): 1.0, (1, 1): 1.0, (2, 2): 0.5, (2, 3): 0.5, **_tail(3, 4)}
    assert (p.a == 1).all() and (p.w == 1).all()
    p = _plan(*PLANS["one_to_three"])              # dog -> the three vectors of <dog>
    third = float(np.float32(1.0 / 3.0))
    assert _entries(p.M) == {(0, 0): 1.0, (1, 1): 1.0, (2, 2): third, (2, 3): third, (2, 4): third, **_tail(3, 5)}


def test_plan_of_an_added_word_uses_the_edits_own_attention_there():
    p = _plan(*PLANS["added"])                     # BOS a dog EOS -> BOS a fluffy dog EOS
    assert _entries(p.M) == {(0, 0): 1.0, (1, 1): 1.0, (2, 3): 1.0, **_tail(3, 4)}      # dog shifted by one; the tail with the source SHORTER
    assert p.a.tolist() == [1, 1, 0] + [1] * (T - 3) and (p.M[:, 2] == 0).all()
    assert _tail(3, 4)[(3, 4)] == 1.0 and (14, 15) in _tail(3, 4) and not p.M[15].any()


def test_plan_of_a_dropped_word_leaves_its_row_empty():
    p = _plan(*PLANS["dropped"])                   # BOS a fluffy dog EOS -> BOS a dog EOS
    assert _entries(p.M) == {(0, 0): 1.0, (1, 1): 1.0, (3, 2): 1.0, **_tail(4, 3)}      # the tail with the source LONGER: clamped at T - 1
    assert not p.M[2].any() and (p.a == 1).all()
    assert p.M[15, 14] == 1 and p.M[15, 15] == 1 and p.M[4, 3] == 1


def test_plan_with_a_multi_vector_placeholder_and_a_prefix():
    p = _plan(*PLANS["placeholder"])               # BOS a photo of a [<dog> x3] dog on a beach EOS
    want = {(i, i): 1.0 for i in range(5)}
    want.update({(5, 8): 1.0, (6, 9): 1.0, (7, 10): 1.0, (8, 11): 1.0, **_tail(9, 12)})
    assert _entries(p.M) == want
    assert p.a.tolist() == [1] * 5 + [0, 0, 0] + [1] * (T - 8)
    q = _plan(*PLANS["prefix"])                    # BOS [a watercolor painting of] dog on a beach EOS: four added words in front
    assert q.a.tolist() == [1, 0, 0, 0, 0] + [1] * (T - 5)
    assert _entries(q.M) == {(0, 0): 1.0, (1, 5): 1.0, (2, 6): 1.0, (3, 7): 1.0, (4, 8): 1.0, **_tail(5, 9)}


def test_plan_reweight():
    from textboost_amd import p2p
    p = _plan(*PLANS["reweight"])
    assert p.w.tolist() == [1, 1, 2] + [1] * (T - 3) and (p.M == np.eye(T, dtype=np.float32)).all() and (p.a == 1).all()
    q = _plan(*PLANS["added_and_reweight"])        # BOS a fluffy [<dog> x3] dog on a beach EOS
    assert q.w.tolist() == [1, 1, 0.5, 3, 3, 3] + [1] * (T - 6) and q.a.tolist() == [1, 1, 0, 0, 0, 0] + [1] * (T - 6)
    with pytest.raises(p2p.P2PError, match="'cat' is not in the edit prompt"):
        _plan("a dog", "a fluffy dog", (("cat", 2.0),))
    for bad in (-0.5, 10.5):
        with pytest.raises(p2p.P2PError, match="0 .. 10"):
            _plan("a dog", "a fluffy dog", (("fluffy", bad),))
    assert p2p.parse_reweight("fluffy=2") == ("fluffy", 2.0) and p2p.parse_reweight("<dog>=0") == ("<dog>", 0.0)
    assert p2p.parse_reweight("x=y=10") == ("x=y", 10.0)
    for bad in ("fluffy", "fluffy=", "=2", "fluffy=two", "fluffy=nan", "fluffy dog=2"):
        with pytest.raises(p2p.P2PError, match="expected WORD=F"):
            p2p.parse_reweight(bad)
    for bad in ("fluffy=11", "fluffy=-1"):
        with pytest.raises(p2p.P2PError, match="0 .. 10"):
            p2p.parse_reweight(bad)
    with pytest.raises(p2p.P2PError, match="does not fit"):
        p2p.plan(StubTokenizer(), "a photo of a dog on a beach", "a photo of a <dog> dog on a beach", 12)


@pytest.mark.parametrize("name", sorted(PLANS))
def test_the_two_term_form_equals_the_defined_probability_row(name):
    from textboost_amd import p2p
    pl = _plan(*PLANS[name])
    g = torch.Generator().manual_seed(sorted(PLANS).index(name))
    Ps = torch.softmax(2.0 * torch.randn(3, 5, T, generator=g, dtype=torch.float64), dim=-1)
    Pe = torch.softmax(2.0 * torch.randn(3, 5, T, generator=g, dtype=torch.float64), dim=-1)
    V = torch.randn(T, 24, generator=g, dtype=torch.float64)
    V1, V2 = p2p.mixed_values(pl, V)
    want = R.p_out(Ps, Pe, pl.M, pl.a, pl.w) @ V
    assert (Ps @ V1 + Pe @ V2 - want).abs().max().item() <= 1e-12
    V1n, V2n = p2p.mixed_values(pl, V.numpy())
    assert np.abs(V1n - V1.numpy()).max() <= 1e-12 and np.abs(V2n - V2.numpy()).max() <= 1e-12
    if (pl.a == 1).all():
        assert (V2 == 0).all()                     # the single-term launch
    if name == "identical":
        assert torch.equal(V1, V) and (R.p_out(Ps, Pe, pl.M, pl.a, pl.w) - Ps).abs().max().item() <= 1e-15


def test_step_counts_from_fractions():
    from textboost_amd import p2p
    f = p2p.steps_for
    assert (f(0.8, 50), f(0.4, 50), f(0.8, 25), f(0.4, 25)) == (40, 20, 20, 10)
    assert (f(0.75, 4), f(0.5, 4), f(0.3, 10), f(0.29, 10), f(0.0, 7), f(1.0, 7), f(0.99, 7)) == (3, 2, 3, 2, 0, 7, 6)
    for bad in (-0.1, 1.1, float("nan"), float("inf")):
        with pytest.raises(p2p.P2PError, match="--cross-steps"):
            f(bad, 10, "--cross-steps")
    assert p2p.CROSS_STEPS == 0.8 and p2p.SELF_STEPS == 0.4 and p2p.SELF_MIN_LEVEL == 2


def test_sampler_refusals():
    from textboost_amd.sampler import DDPMAncestral, DPMSolverPP2M, HipSampler
    unet = types.SimpleNamespace(B=8, T=77, H=16, W=16)
    ctl = types.SimpleNamespace(B4=8, T=77, h=16, w=16, cross_steps=0.75, self_steps=0.5)
    s = types.SimpleNamespace(unet=unet, B=4, steps=4, sch=DPMSolverPP2M.from_config(None))
    f = HipSampler._p2p_steps
    assert f(s, None) == (0, 0) and f(s, ctl) == (3, 2)
    assert f(s, None, maps=object(), regions=object()) == (0, 0)       # without a control nothing is refused here
    with pytest.raises(ValueError, match="does not go with maps"):
        f(s, ctl, maps=object())
    with pytest.raises(ValueError, match="does not go with regions"):
        f(s, ctl, regions=object())
    with pytest.raises(ValueError, match="even batch"):
        f(types.SimpleNamespace(unet=unet, B=3, steps=4, sch=s.sch), ctl)
    for other in (dict(B4=4), dict(T=20), dict(h=8)):
        with pytest.raises(ValueError, match="control is built for"):
            f(s, types.SimpleNamespace(**{**vars(ctl), **other}))
    for other in (dict(cross_steps=1.5), dict(self_steps=-0.1)):
        with pytest.raises(ValueError, match="_steps"):
            f(s, types.SimpleNamespace(**{**vars(ctl), **other}))
    with pytest.raises(NotImplementedError, match="DPM-Solver"):
        f(types.SimpleNamespace(unet=unet, B=4, steps=4, sch=DDPMAncestral.from_config(None)), ctl)


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
    prompt, edit = "a dog on a beach", "a fluffy <dog> dog on a beach"
    common = [da, "--model", mdir, "--prompt", prompt]
    E = ["--edit-prompt", edit]
    p = inference.build_parser()
    a = p.parse_args(["run"])
    assert a.edit_prompt is None and a.cross_steps is None and a.self_steps is None and a.reweight is None
    a = p.parse_args(["run"] + E + ["--reweight", "fluffy=2", "--reweight", "dog=0.5", "--cross-steps", "0.6", "--self-steps", "0.2"])
    assert a.edit_prompt == edit and a.reweight == ["fluffy=2", "dog=0.5"] and (a.cross_steps, a.self_steps) == (0.6, 0.2)
    for extra, msg in ((E + ["--init-image", photo], "--edit-prompt does not go with --init-image"),
                       (["--reweight", "dog=2", "--init-image", photo], "--reweight does not go with --init-image"),
                       (E + ["--region", "dog=0,0,0.5,1"], "--edit-prompt does not go with --region"),
                       (E + ["--attn-map"], "--edit-prompt does not go with --attn-map"),
                       (E + ["--attn-map", "dog"], "attention that did not happen"),
                       (["--cross-steps", "0.5"], "--cross-steps needs --edit-prompt"),
                       (["--self-steps", "0.5"], "--self-steps needs --edit-prompt"),
                       (E + ["--cross-steps", "1.5"], "--cross-steps 1.5"),
                       (E + ["--cross-steps", "-0.1"], "--cross-steps -0.1"),
                       (E + ["--self-steps", "1.01"], "--self-steps 1.01"),
                       (E + ["--self-steps", "nan"], "--self-steps nan"),
                       (E + ["--reweight", "bird=2"], "--reweight bird=2: the word 'bird' is not in the edit prompt"),
                       (["--reweight", "fluffy=2"], "--reweight fluffy=2: the word 'fluffy' is not in the edit prompt"),     # the edit prompt is the prompt
                       (E + ["--reweight", "fluffy"], "--reweight 'fluffy': expected WORD=F"),
                       (E + ["--reweight", "fluffy=much"], "--reweight 'fluffy=much': expected WORD=F"),
                       (E + ["--reweight", "fluffy=11"], "--reweight 'fluffy=11': the factor must lie in 0 .. 10"),
                       (E + ["--reweight", "fluffy=-1"], "--reweight 'fluffy=-1': the factor must lie in 0 .. 10")):
        with pytest.raises(SystemExit, match=re.escape(msg)) as ei:
            inference.main(common + extra)
        assert ei.value.code not in (0, None), extra
    # a shadowed token of a composed run, under the existing rule
    composed = [da, "--with", db, "--model", mdir, "--prompt", "a dog"]
    with pytest.raises(SystemExit, match="--edit-prompt.*<pet>.*ambiguous"):
        inference.main(composed + ["--edit-prompt", "a <pet> dog"])
    with pytest.raises(SystemExit, match="--reweight.*<pet>.*ambiguous"):
        inference.main(composed + ["--edit-prompt", "a <dog> dog", "--reweight", "<pet>=2"])
    # accepted arguments pass every host check and reach the device question
    for extra in (E, E + ["--reweight", "fluffy=2", "--cross-steps", "0", "--self-steps", "1"], ["--reweight", "dog=0.5"],
                  ["--with", db] + E + ["--reweight", "<dog>=1.5"]):
        with pytest.raises(AssertionError, match="consulted"):
            inference.main(common + extra)
    args = p.parse_args(common + E + ["--reweight", "fluffy=2", "--self-steps", "0.2"])
    got = inference.check_p2p_args(args, inference.load_runs(args))
    assert got["edit_prompt"] == edit and (got["cross"], got["self"]) == (0.8, 0.2) and got["plan"].M.shape == (77, 77)
    assert got["plan"].w.max() == 2 and (got["plan"].a == 0).sum() == int((got["plan"].w == 2).sum()) + 1      # fluffy's tokens and the placeholder
    args = p.parse_args(common + ["--reweight", "dog=0.5"])
    got = inference.check_p2p_args(args, inference.load_runs(args))
    assert got["edit_prompt"] == prompt and (got["plan"].M == np.eye(77, dtype=np.float32)).all() and got["plan"].w.min() == 0.5
