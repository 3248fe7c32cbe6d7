"""Host side of the token attention maps (textboost_amd/attn_maps.py, inference.py --attn-map): no GPU."""
import os
import re
import types

import numpy as np
import pytest
import torch

import attn_maps_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_lib_binds_the_kernel():
    from textboost_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "textboost_hip.h")).read()
    m = re.search(r"int\s+tb_attn_token_maps\s*\(([^)]*)\)\s*;", hdr)
    assert m, "include/textboost_hip.h does not declare tb_attn_token_maps"
    assert len(m.group(1).split(",")) == len(_lib._SIGS["tb_attn_token_maps"][0])
    assert os.path.exists(os.path.join(ROOT, "textboost_amd", "csrc", "attn_maps.hip"))
    from textboost_amd import ops
    assert callable(ops.attn_token_maps)


# ------------------------------------------------------------------------------------------------ token_positions
class StubTokenizer:
    """whitespace words -> ids through a table; a word may map to several ids (sub-tokens, or the vectors of a placeholder)"""
    bos_token_id, eos_token_id, pad_token_id = 100, 101, 101
    table = {"a": [1], "photo": [2], "of": [3], "dog": [4], "skateboarding": [5, 6], "<dog>": [50, 51, 52], "<hflip>": [60], "cat": [7]}

    def __call__(self, text, truncation=False, padding=None, max_length=None, add_special_tokens=True):
        ids = [i for w in text.split() for i in self.table[w]]
        if add_special_tokens:
            ids = [self.bos_token_id] + ids + [self.eos_token_id]
        if truncation and max_length is not None and len(ids) > max_length:
            ids = ids[:max_length - 1] + [self.eos_token_id] if add_special_tokens else ids[:max_length]
        if padding == "max_length":
            ids = ids + [self.pad_token_id] * (max_length - len(ids))
        return types.SimpleNamespace(input_ids=ids)


def test_token_positions():
    from textboost_amd.attn_maps import token_positions
    tok = StubTokenizer()
    prompt = "a photo of a <dog> dog skateboarding"      # ids: BOS a photo of a <dog>x3 dog skate boarding EOS
    assert token_positions(tok, prompt, "photo", 16) == [2]
    assert token_positions(tok, prompt, "a", 16) == [1, 4]                       # every occurrence
    assert token_positions(tok, prompt, "skateboarding", 16) == [9, 10]          # two sub-tokens
    assert token_positions(tok, prompt, "<dog>", 16) == [5, 6, 7]                # a 3-vector placeholder
    assert token_positions(tok, prompt, "dog", 16) == [8]
    with pytest.raises(ValueError, match="cat"):
        token_positions(tok, prompt, "cat", 16)
    # truncated to 8 positions: BOS a photo of a <dog>[0] <dog>[1] EOS -- `dog` and the whole placeholder lie past T
    with pytest.raises(ValueError):
        token_positions(tok, prompt, "dog", 8)
    with pytest.raises(ValueError):
        token_positions(tok, prompt, "<dog>", 8)
    assert token_positions(tok, prompt, "of", 8) == [3]
    # BOS / EOS / padding are never returned, even for a word made of their ids
    tok2 = StubTokenizer()
    tok2.table = dict(tok.table, pad=[101], start=[100])
    for w in ("pad", "start"):
        with pytest.raises(ValueError):
            token_positions(tok2, "a photo", w, 16)


def test_word_map_sums_positions():
    from textboost_amd.attn_maps import word_map
    m = torch.arange(2 * 5 * 3 * 4, dtype=torch.float32).view(2, 5, 3, 4)
    assert torch.equal(word_map(m, [1, 3]), m[:, 1] + m[:, 3])
    assert word_map(m, [2]).shape == (2, 3, 4)


# ------------------------------------------------------------------------------------------------ AttnMapRecorder.result
def _stub_unet(B=4, hw=16, T=7):
    from textboost_amd.unet import UNetGeometry
    geo = UNetGeometry(block_out_channels=(32, 64, 64, 64), cross_attn_levels=(True, True, True, False))
    tb = "transformer_blocks.0.attn2"
    xattn = [(f"down_blocks.{i}.attentions.{j}.{tb}", 32) for i in range(3) for j in range(2)]
    xattn += [(f"mid_block.attentions.0.{tb}", 64)]
    xattn += [(f"up_blocks.{i}.attentions.{j}.{tb}", 32) for i in (1, 2, 3) for j in range(3)]
    return types.SimpleNamespace(B=B, H=hw, W=hw, T=T, dev="cpu", geo=geo, xattn=xattn)


def test_recorder_result_matches_the_reference_with_uneven_counts():
    from textboost_amd.attn_maps import AttnMapRecorder, cross_attention_maps
    unet = _stub_unet()
    assert cross_attention_maps(unet) == {(16, 16): 5, (8, 8): 5, (4, 4): 5, (2, 2): 1}
    rec = AttnMapRecorder(unet)                       # rows default to the conditional half
    assert (rec.b0, rec.nb) == (2, 2) and set(rec.acc) == {(16, 16), (8, 8), (4, 4), (2, 2)}
    assert all(a.shape == (2, 7, hw[0] * hw[1]) and a.dtype == torch.float32 for hw, a in rec.acc.items())
    with pytest.raises(RuntimeError):
        rec.result()                                  # nothing recorded yet
    g = torch.Generator().manual_seed(0)
    counts = {(16, 16): 10, (8, 8): 10, (4, 4): 7, (2, 2): 3}
    for hw, a in rec.acc.items():
        a.copy_(torch.rand(a.shape, generator=g) * counts[hw])
        rec.count[hw] = counts[hw]
    got = rec.result()
    want = R.ref_result(rec.acc, counts, 16, 16)
    assert got.shape == (2, 7, 16, 16) and got.dtype == torch.float32
    err = (got.double() - want).abs().max().item()
    print(f"[attn maps] result() vs float64 reference: max |delta| {err:.2e}")
    assert err <= 1e-6
    # the counts matter: equal counts give something else
    other = R.ref_result(rec.acc, {hw: 10 for hw in counts}, 16, 16)
    assert (other - want).abs().max().item() > 1e-3
    rec.zero()
    assert all(float(a.abs().max()) == 0 for a in rec.acc.values()) and set(rec.count.values()) == {0}
    with pytest.raises(ValueError):
        AttnMapRecorder(unet, rows=(3, 5))
    with pytest.raises(ValueError):
        AttnMapRecorder(_stub_unet(T=129))


def test_reference_maps_sum_to_one_over_the_keys():
    g = torch.Generator().manual_seed(1)
    B, H, Sq, Skv, hd = 2, 3, 10, 7, 8
    Q, K = torch.randn(B * Sq, H * hd, generator=g), torch.randn(B * Skv, H * hd, generator=g)
    m = R.ref_token_maps(Q, K, B, H, Sq, Skv, hd, hd ** -0.5)
    assert m.shape == (B, Skv, Sq) and m.dtype == torch.float64
    assert (m.sum(dim=1) - 1).abs().max().item() < 1e-12 and m.min().item() > 0
    # against the definition, written out for one (b, s, j)
    q, k = Q.double().view(B, Sq, H, hd), K.double().view(B, Skv, H, hd)
    p = torch.stack([torch.softmax((k[1, :, h] @ q[1, 4, h]) * hd ** -0.5, dim=0) for h in range(H)]).mean(0)
    assert (m[1, :, 4] - p).abs().max().item() < 1e-12


# ------------------------------------------------------------------------------------------------ overlay
def test_overlay_shape_dtype_and_constant_map():
    from textboost_amd.attn_maps import overlay
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, size=(24, 40, 3), dtype=np.uint8)
    amap = torch.rand(6, 10, generator=torch.Generator().manual_seed(2))
    out = overlay(img, amap)
    assert out.shape == img.shape and out.dtype == np.uint8
    assert np.array_equal(out, overlay(img, amap.numpy()))            # deterministic, tensors and arrays alike
    assert np.abs(out.astype(int) - img.astype(int)).max() > 0
    with np.errstate(all="raise"):
        flat = overlay(img, torch.full((6, 10), 0.25))                   # max == min: no division by zero
    assert flat.shape == img.shape and flat.dtype == np.uint8 and np.isfinite(flat.astype(float)).all()
    assert np.array_equal(flat, overlay(img, torch.zeros(6, 10)))      # a constant map is the bottom of the ramp everywhere
    # the hot spot of the map is the reddest region of the overlay of a grey image
    grey = np.full((32, 32, 3), 128, dtype=np.uint8)
    spot = torch.zeros(8, 8)
    spot[2, 5] = 1.0
    o = overlay(grey, spot).astype(int)
    y, x = np.unravel_index(np.argmax(o[..., 0] - o[..., 2]), (32, 32))
    assert 8 <= y < 12 and 20 <= x < 24
    with pytest.raises(ValueError):
        overlay(img.astype(np.float32), amap)


# ------------------------------------------------------------------------------------------------ inference.py --attn-map
def test_parser_accepts_attn_map_with_and_without_words():
    import inference
    p = inference.build_parser()
    assert p.parse_args(["run"]).attn_map is None
    assert p.parse_args(["run", "--attn-map"]).attn_map == []
    assert p.parse_args(["run", "--attn-map", "<dog>", "dog", "--steps", "3"]).attn_map == ["<dog>", "dog"]


def test_absent_word_exits_before_the_device_is_consulted(tmp_path, monkeypatch):
    pytest.importorskip("transformers")
    import inference
    from tests.test_gpu_generate import _write_tokenizer, write_trained_run
    mdir, rdir = str(tmp_path / "model"), str(tmp_path / "runs" / "dog")
    _write_tokenizer(os.path.join(mdir, "tokenizer"))
    write_trained_run(rdir, ["<dog>"], ["<hflip>"], seed=1)

    def consulted():
        raise AssertionError("torch.cuda was consulted")
    monkeypatch.setattr(torch.cuda, "is_available", consulted)
    common = [rdir, "--model", mdir, "--prompt", "photo of a <dog> dog"]
    with pytest.raises(SystemExit, match="cat"):
        inference.main(common + ["--attn-map", "<dog>", "cat"])
    with pytest.raises(SystemExit, match="occurs"):                      # no word, and no token of the run in the prompt
        inference.main([rdir, "--model", mdir, "--prompt", "photo of a dog", "--attn-map"])
    # words that occur pass the host checks and reach the device question
    with pytest.raises(AssertionError, match="consulted"):
        inference.main(common + ["--attn-map", "<dog>", "dog"])
    with pytest.raises(AssertionError, match="consulted"):
        inference.main(common + ["--attn-map"])
    words, positions = inference.attn_map_words(mdir, __import__("textboost_amd.generate", fromlist=["x"]).read_run_dir(rdir),
                                                "photo of a <dog> dog", [])
    assert words == ["<dog>"] and len(positions) == 1 and len(positions[0]) == 1
