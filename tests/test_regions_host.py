"""Regional prompts on the host (textboost_amd/regions.py, inference.py --region): the float64 reference of tests/region_attn_ref.py, spec parsing,
boxes and mask pictures on the latent grid, the any-pool to coarser levels, the device tables' contents, --region-steps and every refusal."""
import json
import os
import re
import types

import numpy as np
import pytest
import torch

import region_attn_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_lib_binds_the_kernel():
    from textboost_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "textboost_hip.h")).read()
    m = re.search(r"int\s+tb_attention_region_fwd\s*\(([^)]*)\)\s*;", hdr)
    assert m, "include/textboost_hip.h does not declare tb_attention_region_fwd"
    assert len(m.group(1).split(",")) == len(_lib._SIGS["tb_attention_region_fwd"][0]) == 5
    assert os.path.exists(os.path.join(ROOT, "textboost_amd", "csrc", "region_attn.hip"))
    assert callable(ops.attention_region_fwd)


# ------------------------------------------------------------------------------------------------ the reference
def _operands(B, H, Sq, Skv, hd, seed):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(B * n, H * hd, generator=g).half() for n in (Sq, Skv, Skv))


def test_reference_with_all_keys_unrestricted_is_plain_attention():
    B, H, Sq, Skv, hd = 2, 3, 20, 11, 8
    Q, K, V = _operands(B, H, Sq, Skv, hd, 1)
    kr = np.full((B, Skv), -1, dtype=np.int32)
    qb = np.random.default_rng(0).integers(0, 2 ** 32, Sq, dtype=np.uint64).astype(np.uint32)     # whatever the bits: no key looks at them
    O, lse, P = R.ref_region_attention(Q, K, V, B, H, Sq, Skv, hd, hd ** -0.5, kr, qb)
    O0, lse0 = R.ref_attention(Q, K, V, B, H, Sq, Skv, hd, hd ** -0.5)
    assert (O - O0).abs().max().item() <= 1e-14 and (lse - lse0).abs().max().item() <= 1e-13


def test_reference_masked_probabilities_are_exact_zeros_and_rows_sum_to_one():
    B, H, Sq, Skv, hd = 2, 2, 16, 9, 8
    Q, K, V = _operands(B, H, Sq, Skv, hd, 2)
    kr = np.full((B, Skv), -1, dtype=np.int32)
    kr[1, 2], kr[1, 5], kr[1, 7] = 0, 31, 31
    qb = np.zeros(Sq, dtype=np.uint32)
    qb[:8] |= 1
    qb[4:12] |= np.uint32(1 << 31)
    O, lse, P = R.ref_region_attention(Q, K, V, B, H, Sq, Skv, hd, hd ** -0.5, kr, qb.view(np.int32))       # as the device table stores it
    ok = R.allowed(kr, qb)
    assert ok[0].all() and not ok[1, 8:, 2].any() and ok[1, :8, 2].all() and ok[1, 4:12, 5].all() and not ok[1, :4, 7].any()
    assert (P[~ok[:, None].expand_as(P)] == 0).all()                       # exactly
    assert (P[ok[:, None].expand_as(P)] > 0).all()
    assert (P.sum(-1) - 1).abs().max().item() <= 1e-14
    # a query with every key masked: O = 0, LSE = -inf, nothing non-finite in O
    kr2 = np.zeros((1, Skv), dtype=np.int32)
    O2, lse2, P2 = R.ref_region_attention(Q[:Sq], K[:Skv], V[:Skv], 1, H, Sq, Skv, hd, 1.0, kr2, qb)
    assert (O2.view(Sq, H, hd)[8:] == 0).all() and torch.isinf(lse2[0, :, 8:]).all() and torch.isfinite(O2).all() and torch.isfinite(lse2[0, :, :8]).all()


# ------------------------------------------------------------------------------------------------ specs, boxes, masks, pooling
def test_parse_region():
    from textboost_amd import regions as G
    s = G.parse_region("<dog> dog=0,0,0.5,1")
    assert s.words == ("<dog>", "dog") and s.box == (0.0, 0.0, 0.5, 1.0) and s.mask is None
    s = G.parse_region("cat = .5, 0, 1, 1 ")
    assert s.words == ("cat",) and s.box == (0.5, 0.0, 1.0, 1.0)
    s = G.parse_region("a=b=0,0,1,0.25")              # the LAST = separates the words from the place
    assert s.words == ("a=b",) and s.box == (0.0, 0.0, 1.0, 0.25)
    s = G.parse_region("cat=@masks/right.png")
    assert s.words == ("cat",) and s.box is None and s.mask == "masks/right.png"
    for bad in ("cat", "=0,0,1,1", "cat=", "cat=0,0,1", "cat=0,0,1,1,1", "cat=0,0,x,1", "cat=0.5,0,0.5,1", "cat=0.6,0,0.5,1", "cat=0,0,1.1,1",
                "cat=-0.1,0,1,1", "cat=0,1,1,1", "cat=0,0,nan,1", "cat=@"):
        with pytest.raises(G.RegionError, match="malformed box|expected|no file name"):
            G.parse_region(bad)
    with pytest.raises(G.RegionError, match="malformed box"):
        G.parse_region("cat=0,0,2,1")


def test_box_to_cells_by_the_centre_rule():
    from textboost_amd.regions import box_cells
    c = box_cells((0.0, 0.0, 0.5, 1.0), 8, 8)                     # ends on the boundary between cells 3 and 4
    assert c[:, :4].all() and not c[:, 4:].any()
    c = box_cells((0.5, 0.0, 1.0, 1.0), 8, 8)
    assert c[:, 4:].all() and not c[:, :4].any()
    # centres of an 8-wide grid are 1/16, 3/16, ...: [0.2, 0.45) holds 5/16 = 0.3125 and 7/16 = 0.4375 only
    c = box_cells((0.2, 0.3, 0.45, 0.7), 8, 8)
    assert np.argwhere(c.any(axis=0)).ravel().tolist() == [2, 3] and np.argwhere(c.any(axis=1)).ravel().tolist() == [2, 3, 4, 5]
    # a box whose edge IS a centre: half-open, so x0 = centre is inside and x1 = centre is outside
    c = box_cells((3 / 16, 0.0, 7 / 16, 1.0), 8, 8)
    assert np.argwhere(c[0]).ravel().tolist() == [1, 2]
    # a box between two centres holds no cell
    assert not box_cells((0.07, 0.0, 0.18, 1.0), 8, 8).any()
    # two boxes that share an edge partition the grid, also on an odd grid
    a, b = box_cells((0, 0, 0.5, 1), 7, 5), box_cells((0.5, 0, 1, 1), 7, 5)
    assert not (a & b).any() and (a | b).all() and a[0].tolist() == [True, True, False, False, False]      # centre 0.5 of cell 2 goes right


def test_mask_picture_to_cells():
    from PIL import Image
    from textboost_amd.regions import mask_cells
    m = np.zeros((64, 96), dtype=np.uint8)
    m[:, 48:] = 255
    m[0:8, 0:12] = 128           # >= 128 is inside
    m[8:16, 0:12] = 127
    c = mask_cells(Image.fromarray(m), 8, 8)
    assert c[:, 4:].all() and c[0, 0] and not c[1, 0] and not c[2:, :4].any()
    rgb = Image.fromarray(np.stack([m, m, m], axis=-1))          # converted to "L"
    assert (mask_cells(rgb, 8, 8) == c).all()
    assert mask_cells(m, 4, 4).shape == (4, 4)


def test_any_pool_to_coarser_levels_and_odd_grids():
    from textboost_amd.regions import halve_any, pool_any
    from textboost_amd.edit import pool_mask_any
    c = np.zeros((16, 16), dtype=bool)
    c[5, 9] = True                        # one latent cell
    c[0:16, 0:2] = True                   # a two-cell strip
    for n in (8, 4, 2):
        p = pool_any(c, (n, n))
        f = 16 // n
        assert (p == pool_mask_any(c.astype(np.uint8), f).astype(bool)).all()       # edit's rule for the latent mask
        assert p[5 // f, 9 // f] and p[:, 0].all() and p.sum() == n + 1
    assert pool_any(c, (16, 16)) is not None and (pool_any(c, (16, 16)) == c).all()
    # odd grid: ceil division, the last row / column covers what is left
    o = np.zeros((5, 7), dtype=bool)
    o[4, 6] = True
    h1 = halve_any(o)
    assert h1.shape == (3, 4) and h1[2, 3] and h1.sum() == 1
    assert pool_any(o, (2, 2)).tolist() == [[False, False], [False, True]]
    o2 = np.zeros((5, 7), dtype=bool)
    o2[1, 2] = True
    assert pool_any(o2, (3, 4)).tolist() == [[False, True, False, False], [False] * 4, [False] * 4]
    with pytest.raises(ValueError, match="not a halving"):
        pool_any(c, (5, 5))
    with pytest.raises(ValueError, match="not a halving"):
        pool_any(c, (32, 32))


# ------------------------------------------------------------------------------------------------ the tables
class StubTokenizer:
    """whitespace words -> ids through a table; a word may map to several ids (sub-tokens, or the vectors of a placeholder)"""
    bos_token_id, eos_token_id, pad_token_id = 100, 101, 101
    table = {"a": [1], "photo": [2], "of": [3], "dog": [4], "skateboarding": [5, 6], "<dog>": [50, 51, 52], "<cat>": [60], "cat": [7], "and": [8]}

    def __call__(self, text, truncation=False, padding=None, max_length=None, add_special_tokens=True):
        ids = [i for w in text.split() for i in self.table[w]]
        if add_special_tokens:
            ids = [self.bos_token_id] + ids + [self.eos_token_id]
        if truncation and max_length is not None and len(ids) > max_length:
            ids = ids[:max_length - 1] + [self.eos_token_id] if add_special_tokens else ids[:max_length]
        if padding == "max_length":
            ids = ids + [self.pad_token_id] * (max_length - len(ids))
        return types.SimpleNamespace(input_ids=ids)


PROMPT = "a <dog> dog and a <cat> cat skateboarding"      # BOS a <dog>x3 dog and a <cat> cat skate boarding EOS pad...


def _two_regions(h=16, w=16, T=20):
    from textboost_amd import regions as G
    specs = [G.parse_region("<dog> dog=0,0,0.5,1"), G.parse_region("<cat> cat skateboarding=0.5,0,1,1")]
    return G.resolve_regions(StubTokenizer(), PROMPT, T, specs, h, w)


def test_key_region_and_query_tables():
    from textboost_amd import regions as G
    regs = _two_regions()
    assert regs[0].positions == (2, 3, 4, 5) and regs[1].positions == (8, 9, 10, 11)      # the 3-vector placeholder + dog; <cat> cat + two sub-tokens
    levels = [(16, 16), (8, 8), (4, 4), (2, 2)]
    rs = G.RegionSet(regs, batch=3, T=20, h=16, w=16, levels=levels, device="cpu")
    kr = rs.key_region
    assert kr.dtype == torch.int32 and tuple(kr.shape) == (6, 20) and kr.is_contiguous()
    assert (kr[:3] == -1).all()                                                           # the unconditional half
    want = [-1, -1, 0, 0, 0, 0, -1, -1, 1, 1, 1, 1] + [-1] * 8                            # start token, "a", "and", "a", end token, padding: global
    assert all(kr[b].tolist() == want for b in (3, 4, 5))
    assert (kr[:, 0] == -1).all() and (kr[:, 12:] == -1).all()
    for hw in levels:
        t = rs.table(hw)
        assert t.dtype == torch.int32 and t.numel() == hw[0] * hw[1]
        bits = t.view(*hw)
        assert (bits[:, :hw[1] // 2] == 1).all() and (bits[:, hw[1] // 2:] == 2).all()
    with pytest.raises(KeyError, match="no region table"):
        rs.table((3, 3))
    # 32 regions: bit 31 lands in the int32's sign and reads back unsigned
    many = [G.Region((f"w{r}",), (1 + r,), np.eye(1, 64, r, dtype=bool).reshape(8, 8)) for r in range(32)]
    rs32 = G.RegionSet(many, batch=1, T=40, h=8, w=8, levels=[(8, 8), (4, 4)], device="cpu")
    got = rs32.table((8, 8)).numpy().view(np.uint32)
    assert got[:32].tolist() == [1 << r for r in range(32)] and (got[32:] == 0).all()
    assert rs32.key_region[1, 1:33].tolist() == list(range(32)) and rs32.key_region[1, 0] == -1
    assert rs32.table((4, 4)).numpy().view(np.uint32)[0] == (1 << 0) | (1 << 1) | (1 << 8) | (1 << 9)       # any-pool: cells 0, 1, 8, 9
    # for_unet: the levels of attn_maps.cross_attention_maps, batch 2B
    from tests.test_attn_maps_host import _stub_unet
    rs = G.RegionSet.for_unet(_stub_unet(B=4, hw=16, T=20), regs)
    assert sorted(rs.tables) == [(2, 2), (4, 4), (8, 8), (16, 16)] and rs.B == 2 and rs.B2 == 4 and tuple(rs.key_region.shape) == (4, 20)
    with pytest.raises(ValueError, match="even batch"):
        G.RegionSet.for_unet(_stub_unet(B=3, hw=16, T=20), regs)
    # a grid that a level does not halve exactly (18 -> 9 -> 4): the UNet's floor shapes and the ceil pooling would disagree
    with pytest.raises(ValueError, match="does not divide"):
        G.RegionSet.for_unet(_stub_unet(B=4, hw=18, T=20), _two_regions(18, 18))


def test_preview_is_flat_colours_at_the_image_size():
    from textboost_amd import regions as G
    im = G.preview(_two_regions(), (128, 128))
    a = np.asarray(im)
    assert a.shape == (128, 128, 3)
    assert (a[:, :64] == G.COLOURS[0]).all() and (a[:, 64:] == G.COLOURS[1]).all()


def test_region_steps_arithmetic():
    from textboost_amd.regions import RegionError, steps_for
    assert steps_for(1.0, 50) == 50 and steps_for(0.5, 50) == 25 and steps_for(0.2, 50) == 10       # (0.2 * 50 = 10.000000000000002)
    assert steps_for(0.21, 50) == 11 and steps_for(0.001, 50) == 1 and steps_for(0.5, 3) == 2 and steps_for(1.0, 1) == 1
    assert steps_for(0.6, 25) == 15 and steps_for(0.3, 10) == 3
    for bad in (0.0, -0.5, 1.01, float("nan")):
        with pytest.raises(RegionError, match="region-steps"):
            steps_for(bad, 50)


# ------------------------------------------------------------------------------------------------ refusals
def test_resolve_refusals_by_name(tmp_path):
    from PIL import Image
    from textboost_amd import regions as G
    tok, P = StubTokenizer(), G.parse_region

    def resolve(*specs, h=8, w=8):
        return G.resolve_regions(tok, PROMPT, 20, [P(s) for s in specs], h, w)
    with pytest.raises(G.RegionError, match="'photo' is not in the prompt"):
        resolve("photo=0,0,1,1")
    with pytest.raises(G.RegionError, match="'dog' is claimed by two regions"):
        resolve("<dog> dog=0,0,0.5,1", "dog=0.5,0,1,1")
    with pytest.raises(G.RegionError, match="claimed by two regions"):         # "a" occurs twice; "a <dog>" overlaps it in position 1
        G.resolve_regions(StubTokenizer(), "a <dog> dog", 20, [P("a=0,0,0.5,1"), G.RegionSpec(("a <dog>",), (0.5, 0, 1, 1), None, "a <dog>=...")], 8, 8)
    with pytest.raises(G.RegionError, match="an empty region"):
        resolve("dog=0.07,0,0.18,1")
    black = str(tmp_path / "black.png")
    Image.fromarray(np.zeros((32, 32), dtype=np.uint8)).save(black)
    with pytest.raises(G.RegionError, match="an empty region"):
        resolve(f"dog=@{black}")
    with pytest.raises(G.RegionError, match="cannot be read as a picture"):
        resolve(f"dog=@{tmp_path / 'missing.png'}")
    tok33 = StubTokenizer()
    tok33.table = {f"w{i}": [200 + i] for i in range(40)}
    prompt33 = " ".join(f"w{i}" for i in range(40))
    specs = [P(f"w{i}=0,0,1,1") for i in range(33)]
    with pytest.raises(G.RegionError, match="33 regions; at most 32"):
        G.resolve_regions(tok33, prompt33, 60, specs, 8, 8)
    assert len(G.resolve_regions(tok33, prompt33, 60, specs[:32], 8, 8)) == 32
    white = str(tmp_path / "white.png")
    Image.fromarray(np.full((10, 30), 200, dtype=np.uint8)).save(white)
    assert resolve(f"dog=@{white}")[0].cells.all()


def test_sampler_refuses_region_steps_out_of_range():
    from textboost_amd.sampler import HipSampler
    unet = types.SimpleNamespace(B=4, T=20, H=16, W=16)
    s = types.SimpleNamespace(unet=unet)
    rs = types.SimpleNamespace(B2=4, T=20, h=16, w=16)
    f = HipSampler._region_steps
    assert f(s, None, None, 5) == 0 and f(s, rs, None, 5) == 5 and f(s, rs, 5, 5) == 5 and f(s, rs, 1, 5) == 1
    for bad in (0, 6, -1, 2.5):
        with pytest.raises(ValueError, match="region_steps"):
            f(s, rs, bad, 5)
    with pytest.raises(ValueError, match="region_steps without regions"):
        f(s, None, 3, 5)
    with pytest.raises(ValueError, match="regions are built for"):
        f(s, types.SimpleNamespace(B2=2, T=20, h=16, w=16), None, 5)


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

    def consulted():
        raise AssertionError("torch.cuda was consulted")
    monkeypatch.setattr(torch.cuda, "is_available", consulted)
    prompt = "a <dog> dog and a <cat> cat"
    common = [da, "--with", db, "--model", mdir, "--prompt", prompt]
    L, Rr = ["--region", "<dog> dog=0,0,0.5,1"], ["--region", "<cat> cat=0.5,0,1,1"]
    p = inference.build_parser()
    assert p.parse_args(["run"]).region is None and p.parse_args(["run"]).region_steps is None
    a = p.parse_args(["run"] + L + Rr + ["--region-steps", "0.5"])
    assert a.region == ["<dog> dog=0,0,0.5,1", "<cat> cat=0.5,0,1,1"] and a.region_steps == 0.5
    for extra, msg in ((["--region", "bird=0,0,1,1"], "'bird' is not in the prompt"),
                       (L + ["--region", "dog=0.5,0,1,1"], "claimed by two regions"),
                       (["--region", "dog=0.07,0,0.09,1"], "an empty region"),
                       (["--region", "dog=0,0,1"], "malformed box"),
                       (["--region", "dog=0.5,0,0.2,1"], "malformed box"),
                       (["--region", "dog"], "expected"),
                       (L + ["--region-steps", "0"], "region-steps"),
                       (L + ["--region-steps", "1.5"], "region-steps"),
                       (["--region-steps", "0.5"], "--region-steps needs --region"),
                       (L + ["--attn-map"], "attention that did not happen"),
                       (L + ["--attn-map", "dog"], "--region does not go with --attn-map"),
                       ([f"--region=dog=@{tmp_path / 'nothing.png'}"], "cannot be read as a picture"),
                       (["--region", "a=0,0,1,1"] * 1 + [x for i in range(32) for x in ("--region", f"w{i}=0,0,1,1")], "33 regions; at most 32")):
        with pytest.raises(SystemExit, match=re.escape(msg)):
            inference.main(common + extra)
    # a shadowed token of a composed run, under the existing rule
    with pytest.raises(SystemExit, match="<pet>.*ambiguous"):
        inference.main([da, "--with", db, "--model", mdir, "--prompt", "a <pet> dog", "--region", "<pet>=0,0,0.5,1"])
    # accepted arguments pass every host check and reach the device question
    for extra in (L + Rr, L + Rr + ["--region-steps", "0.3"], L):
        with pytest.raises(AssertionError, match="consulted"):
            inference.main(common + extra)
    args = p.parse_args(common + L + Rr + ["--region-steps", "0.3", "--steps", "10", "--output", str(tmp_path / "g.jpg")])
    got = inference.check_region_args(args, inference.load_runs(args), None)
    assert got["steps"] == 3 and [r.words for r in got["regions"]] == [("<dog>", "dog"), ("<cat>", "cat")]
    assert all(r.cells.shape == (16, 16) for r in got["regions"]) and inference.regions_path(args) == str(tmp_path / "g_regions.png")
    assert inference.check_region_args(args, inference.load_runs(args), {"strength": 0.5})["steps"] == 2     # 5 executed steps: ceil(1.5)
