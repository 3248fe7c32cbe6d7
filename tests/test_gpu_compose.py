"""Composed runs on the GPU: the composed text-encoder adapter on both adapter paths against the oracle encoder with merged weights, the UNet
cross-attention K/V fold (`Pipeline.set_unet_adapters`) against the oracle UNet with merged weights, per-run switching in `generate_instance`,
and `inference.py --with` end to end.  Tiny models: text D = 64, L = 2, T = 77; the tiny UNet at 16 x 16 latents."""
import copy
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from parity import parity

pytestmark = pytest.mark.gpu
dev = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D_TEXT = 64
PROJ = ("q_proj", "k_proj", "v_proj")
# the bound tests/test_gpu_generate.py (test_loaded_text_encoder_matches_the_oracle_encoder) and tests/test_gpu_lora_wide.py hold for ONE run's
# loaded encoder.  Composition adds no device arithmetic, so it gets no tolerance of its own.
ENC = dict(rel=5e-4, maxabs=1e-3, ch_dim=2, ch_rel=2e-3)
# one fp16 forward of this tiny UNet against the fp32 oracle: tests/test_gpu_model.py, test_unet_forward_and_dgrad_backward_match_oracle,
# `parity("tiny UNet pred", ..., rel=3e-3, maxabs=4e-3, ch_dim=1, ch_rel=4e-3)` -- the model tests/test_gpu_sampler.py and
# tests/test_gpu_generate.py sample with (their own assertions bound whole sampling loops, not one forward).
UNET = dict(rel=3e-3, maxabs=4e-3, ch_dim=1, ch_rel=4e-3)


def merged_oracle_encoder(base, ccfg, parts, rows):
    """the oracle encoder WITHOUT adapters whose q / k / v weights are W + sum_i w_i B_i A_i (merged here, fp32), with the added token rows in id
    order and the base encoder's null embedding.  parts: [(TrainedRun, weight)]"""
    from oracle.clip_text import TextBoostEncoder, add_tokens
    enc = TextBoostEncoder(ccfg, r=0)
    enc.load_state_dict(base.state_dict())
    with torch.no_grad():
        null = base.transformer(torch.tensor([[49406] + [49407] * 76]))[0]
        for i, layer in enumerate(enc.layers):
            for proj, m in zip(PROJ, (layer.q, layer.k, layer.v)):
                name = f"base_model.model.text_model.encoder.layers.{i}.self_attn.{proj}"
                for run, w in parts:
                    m.weight.add_(w * (run.lora[name + ".lora_B.weight"] @ run.lora[name + ".lora_A.weight"]))
        ids = add_tokens(enc, [0] * len(rows))
        for tid, row in zip(ids, rows):
            enc.token_embedding.weight[tid] = row
    enc.set_null_embedding(null)
    return enc.eval()


def xattn_of(oracle_unet):
    """(attn2 path, channels) of every cross-attention of the oracle UNet"""
    return [(k[:-len(".to_k.weight")], int(v.shape[0])) for k, v in oracle_unet.state_dict().items() if k.endswith("attn2.to_k.weight")]


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    from tests.test_gpu_generate import write_model_dir
    mdir = str(tmp_path_factory.mktemp("compose") / "model")
    unet, dec, base, ccfg = write_model_dir(mdir)
    return mdir, unet, base, ccfg


# ------------------------------------------------------------------------------------------------ the composed encoder
@pytest.mark.parametrize("rank_b", [4, 8])
def test_composed_encoder_matches_the_oracle_with_merged_weights(model, tmp_path, rank_b):
    """ranks 4 + 4 = 8: the VALU adapter kernels; 4 + 8 = 12: csrc/lora_wide.hip"""
    from tests.test_compose_host import write_run
    from textboost_amd import generate as G
    from textboost_amd.compose import compose_runs
    mdir, _, base, ccfg = model
    da, db = str(tmp_path / "dog"), str(tmp_path / "style")
    write_run(da, ["<dog>"], ["<hflip>"], seed=1, rank=4)
    write_run(db, ["<style>"], ["<hflip>"], seed=2, rank=rank_b)
    a, b = G.read_run_dir(da), G.read_run_dir(db)
    w = (1.0, 0.7)
    run = compose_runs([a, b], w)
    assert run.rank == 4 + rank_b and [n for n, _ in run.tokens] == ["<dog>", "<hflip>", "<style>"] and run.shadowed == [("<hflip>", db)]
    prompts = ["a <dog> dog in <style> style", "", "a <hflip> photo of a <dog> dog wearing a black top hat in <style> style", "a red <style> <dog>"]
    with torch.no_grad():
        te, tok = G.load_text_encoder(mdir, run, 4, dev)
        assert te.r == 4 + rank_b and te.wide == (rank_b == 8)
        assert tok.convert_tokens_to_ids(["<dog>", "<hflip>", "<style>"]) == [49408, 49409, 49410]
        ids = G.tokenize(tok, prompts, 77)
        assert all((ids[k] == 49408).sum() == 1 and (ids[k] == 49410).sum() == 1 for k in (0, 2, 3)) and (ids[2] == 49409).sum() == 1
        out = te.forward(ids.to(dev)).view(4, 77, D_TEXT).clone()
        ref = merged_oracle_encoder(base, ccfg, [(a, w[0]), (b, w[1])], [v for _, v in run.tokens])(ids)
        parity(f"composed encoder (ranks 4 + {rank_b}) vs oracle with merged weights", out, ref, **ENC)
        # the second run matters: the first run's adapter alone (all tokens kept) is further away than 10 x the bound
        alone, _ = G.load_text_encoder(mdir, compose_runs([a, b], (1.0, 0.0)), 4, dev)
        far = alone.forward(ids.to(dev)).view(4, 77, D_TEXT)
        gap = ((far[0] - out[0]).norm() / out[0].norm()).item()
        print(f"[compose] ranks 4 + {rank_b}: first run alone vs composed, rel-L2 {gap:.3e} (> {10 * ENC['rel']:.1e})")
        assert gap > 10 * ENC["rel"]


def test_weight_zero_is_the_first_run_alone_bit_for_bit(model, tmp_path):
    from tests.test_compose_host import write_run
    from textboost_amd import generate as G
    from textboost_amd.compose import compose_runs
    mdir = model[0]
    da, db = str(tmp_path / "dog"), str(tmp_path / "style")
    write_run(da, ["<dog>"], ["<hflip>"], seed=1, rank=4)
    write_run(db, ["<style>"], [], seed=2, rank=8)
    a, b = G.read_run_dir(da), G.read_run_dir(db)
    prompts = ["a <dog> dog in the jungle", "", "a <hflip> photo of a <dog> dog", "a red <dog> dog"]
    with torch.no_grad():
        te0, tok0 = G.load_text_encoder(mdir, a, 4, dev)
        te1, tok1 = G.load_text_encoder(mdir, compose_runs([a, b], (1.0, 0.0)), 4, dev)
        ids = G.tokenize(tok0, prompts, 77)
        assert torch.equal(ids, G.tokenize(tok1, prompts, 77)) and te1.r == 4 and te1.token_table.shape[0] == te0.token_table.shape[0] + 1
        assert torch.equal(te1.forward(ids.to(dev)), te0.forward(ids.to(dev)))


# ------------------------------------------------------------------------------------------------ the K/V fold
def test_kv_fold_matches_the_oracle_unet_with_merged_weights(model):
    from tests.test_compose_host import stub_kv_unet
    from textboost_amd import checkpoint as ckpt
    from textboost_amd import generate as G
    mdir, unet, _, _ = model
    with torch.no_grad():
        pipe = G.Pipeline.from_model_dir(mdir, 1, steps=4, device=dev)
    hip = pipe.unet
    assert sorted(hip.xattn) == sorted(xattn_of(unet)) and pipe.kv_base.dtype == torch.float32
    assert tuple(pipe.kv_base.shape) == tuple(hip.P["kv_all.w"].shape)
    sds = [ckpt.unet_lora_state_dict(stub_kv_unet(hip.xattn, D_TEXT, 4, seed=s)) for s in (11, 12)]
    w = (1.0, 0.5)
    merged = copy.deepcopy(unet)
    with torch.no_grad():
        msd = merged.state_dict()
        for p, _ in hip.xattn:
            for name in ("to_k", "to_v"):
                for sd, wi in zip(sds, w):
                    msd[f"{p}.{name}.weight"].add_(wi * (sd[f"{p}.{name}.lora_B.default.weight"] @ sd[f"{p}.{name}.lora_A.default.weight"]))
    g = torch.Generator().manual_seed(1)
    B, hw = 2, 16
    x = torch.randn(B, 4, hw, hw, generator=g).half().float()
    t = torch.tensor([17, 801])
    ehs = torch.randn(B, 77, D_TEXT, generator=g).half().float()
    args = (x.half().to(dev), t.to(dev), ehs.half().view(B * 77, D_TEXT).to(dev).contiguous())
    with torch.no_grad():
        ref_base, ref = unet(x, t, ehs), merged(x, t, ehs)
        w_before = hip.P["kv_all.w"].clone()
        before = hip.forward(*args).clone()
        parity("base UNet (before any fold)", before, ref_base, **UNET)
        pipe.set_unet_adapters([(sds[0], 4, w[0]), (sds[1], 4, w[1])])
        folded = hip.forward(*args).clone()
        parity("UNet with two sets of K/V adapters folded in, weights (1, 0.5)", folded, ref, **UNET)
        off = ((before.float().cpu() - ref).norm() / ref.norm()).item()
        print(f"[compose] K/V fold: base weights vs merged oracle rel-L2 {off:.3e} (> {10 * UNET['rel']:.1e})")
        assert off > 10 * UNET["rel"]
        # one set at weight 0 is left out: the same weights as the other set alone
        pipe.set_unet_adapters([(sds[0], 4, 1.0), (sds[1], 4, 0.0)])
        w_one = hip.P["kv_all.w"].clone()
        pipe.set_unet_adapters([(sds[0], 4, 1.0)])
        assert torch.equal(hip.P["kv_all.w"], w_one) and not torch.equal(w_one, w_before)
        pipe.set_unet_adapters([])
        assert torch.equal(hip.P["kv_all.w"], w_before)
        assert torch.equal(hip.forward(*args), before)
    with pytest.raises(ValueError, match="lora_A"):
        pipe.set_unet_adapters([(sds[0], 2, 1.0)])
    with pytest.raises(ValueError, match="no tensor"):
        pipe.set_unet_adapters([({}, 4, 1.0)])
    assert torch.equal(hip.P["kv_all.w"], w_before)


# ------------------------------------------------------------------------------------------------ per-run switching
def test_generate_instance_switches_the_unet_per_run(model, tmp_path):
    from tests.test_compose_host import stub_kv_unet, write_run
    from textboost_amd import checkpoint as ckpt
    from textboost_amd import generate as G
    mdir, unet, _, _ = model
    subjects = ["dog", "can", "cat"]
    for k, s in enumerate(subjects):
        write_run(str(tmp_path / "runs" / s), [f"<{s}>"], [], seed=20 + k, rank=4)
    ckpt.save_unet_adapters(stub_kv_unet(xattn_of(unet), D_TEXT, 4, seed=30), str(tmp_path / "runs" / "can" / "unet"), "tiny")
    runs = {s: G.read_run_dir(str(tmp_path / "runs" / s)) for s in subjects}
    assert [runs[s].unet_rank for s in subjects] == [0, 4, 0]
    # `unet` in the directory listing does not change the identifier (the files that start with the subject's name are counted)
    assert G.identifier_for("<INSTANCE> SUBJECT", "can", runs["can"].files) == "<can> can"

    def read(paths):
        return [open(p, "rb").read() for p in paths]

    with torch.no_grad():
        text = G.load_base_text(mdir, dev)
        plain = G.Pipeline.from_model_dir(mdir, 13, steps=2, device=dev)          # never sees an adapter
        want = {s: read(G.generate_instance(plain, text, dataclasses.replace(runs[s], unet_rank=0, unet_lora={}), s, [3], str(tmp_path / "plain")))
                for s in subjects}
        assert not plain.kv_folded
        pipe = G.Pipeline.from_model_dir(mdir, 13, steps=2, device=dev)
        got = {}
        for s in subjects:
            got[s] = read(G.generate_instance(pipe, text, runs[s], s, [3], str(tmp_path / "switched")))
            assert pipe.kv_folded == (s == "can")
    assert all(len(got[s]) == 25 for s in subjects)
    assert got["dog"] == want["dog"] and got["cat"] == want["cat"]
    assert sum(a != b for a, b in zip(got["can"], want["can"])) == 25


# ------------------------------------------------------------------------------------------------ inference.py --with, end to end
def test_inference_cli_composes_two_runs(model, tmp_path):
    pytest.importorskip("transformers")
    from PIL import Image
    from tests.test_compose_host import stub_kv_unet, write_run
    from textboost_amd import checkpoint as ckpt
    mdir, unet, _, _ = model
    da, db = str(tmp_path / "runs" / "dog"), str(tmp_path / "runs" / "style")
    write_run(da, ["<dog>"], ["<hflip>"], seed=1, rank=4, keep_rows="even")
    write_run(db, ["<style>"], ["<hflip>"], seed=2, rank=8, keep_rows="odd")
    ckpt.save_unet_adapters(stub_kv_unet(xattn_of(unet), D_TEXT, 4, seed=3), os.path.join(db, "unet"), "tiny")
    inf = os.path.join(ROOT, "inference.py")
    prompt = "a <dog> dog in <style> style"

    def child(cmd):
        r = subprocess.run([sys.executable, inf] + cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        return r.stdout

    grid = str(tmp_path / "grid.jpg")
    out = child([da, "--with", db, "--weights", "1", "0.8", "--model", mdir, "--prompt", prompt, "--seeds", "0", "1", "--steps", "4",
                 "--output", grid, "--attn-map"])
    assert f"run {da}: rank 4, lora_B rows even, weight 1, UNet K/V adapters none" in out
    assert f"run {db}: rank 8, lora_B rows odd, weight 0.8, UNet K/V adapters rank 4" in out
    assert "disjoint output features" in out and out.index(f"run {db}") < out.index("wrote")
    assert Image.open(grid).size == (2 * 128, 128)
    z = np.load(str(tmp_path / "grid_attn.npz"))
    assert list(z["words"]) == ["<dog>", "<style>"] and z["maps"].shape == (2, 2, 16, 16) and np.isfinite(z["maps"]).all()
    assert list(z["seeds"]) == [0, 1]
    # run A alone: the prompt's <style> is then plain text; the grid differs
    alone = str(tmp_path / "alone.jpg")
    out1 = child([da, "--model", mdir, "--prompt", prompt, "--seeds", "0", "1", "--steps", "4", "--output", alone])
    assert "lora_B rows" not in out1
    d = np.abs(np.asarray(Image.open(grid)).astype(int) - np.asarray(Image.open(alone)).astype(int))
    print(f"[compose] inference.py: composed grid vs run A alone, mean |delta| {d.mean():.2f} levels")
    assert d.max() > 0
