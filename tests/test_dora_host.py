"""Host side of --use_dora (text-encoder DoRA: a magnitude vector per adapted module beside lora_A / lora_B): the flag, the key layout and the
config JSON, the run-directory reader, the refusals, and the float64 reference itself (tests/dora_ref.py) against the formulas of DESIGN 7.4.
No GPU."""
import json
import os
import types

import pytest
import torch

import dora_ref as DR
import lora_targets_ref as LT
from test_lora_targets_host import BASE, D, LAYERS, SHAPES, stub_encoder

# checkpoint.adapter_config(4, "tiny") of the commit before --use_dora, verbatim
PARENT_CONFIG = {"alpha_pattern": {}, "auto_mapping": None, "base_model_name_or_path": "tiny", "bias": "none", "fan_in_fan_out": False,
                 "inference_mode": True, "init_lora_weights": "gaussian", "layer_replication": None, "layers_pattern": None,
                 "layers_to_transform": None, "loftq_config": {}, "lora_alpha": 4, "lora_dropout": 0.0, "megatron_config": None,
                 "megatron_core": "megatron.core", "modules_to_save": None, "peft_type": "LORA", "r": 4, "rank_pattern": {}, "revision": None,
                 "target_modules": ["q_proj", "k_proj", "v_proj"], "task_type": None, "use_dora": False, "use_rslora": False}


def dora_stub(modules, rank, seed):
    """`stub_encoder` plus what checkpoint.py reads of a DoRA encoder: use_dora, mag [L, 3D], extra[name].mag [L, N]"""
    te = stub_encoder(modules, rank, seed)
    g = torch.Generator().manual_seed(seed + 100)
    te.use_dora = True
    te.mag = torch.rand(LAYERS, 3 * D, generator=g) + 0.5
    for n, X in te.extra.items():
        X.mag = torch.rand(LAYERS, SHAPES[n][1], generator=g) + 0.5
    return te


def write_run(d, te, token):
    from textboost_amd import checkpoint as ckpt
    ckpt.save_text_encoder_adapter(te, os.path.join(d, "text_encoder"), "tiny")
    ckpt.save_token_embeddings(te, d, {token: 0}, None)
    return d


# ------------------------------------------------------------------------------------------------ the flag
def test_flag_parses_needs_a_rank_and_is_no_reference_flag():
    from textboost_amd import cli
    from textboost_amd.text_encoder import CLIPGeometry, HipTextEncoder
    assert cli.parse_args(BASE).use_dora is False
    a = cli.parse_args(BASE + ["--use_dora", "--lora_rank", "16", "--lora_target_modules", *LT.ALL])
    assert a.use_dora is True and a.lora_rank == 16 and a.lora_target_modules == list(LT.ALL)
    with pytest.raises(ValueError, match=r"--use_dora needs --lora_rank > 0"):
        cli.parse_args(BASE + ["--use_dora", "--lora_rank", "0"])
    assert not any("--use_dora" in f["flags"] for f in cli.flag_table()) and len(cli.flag_table()) == 66
    assert "--use_dora" in cli.build_parser().format_help()
    with pytest.raises(ValueError, match="use_dora"):       # the encoder's own check, before it touches a weight or the device
        HipTextEncoder(CLIPGeometry(), {}, 1, lora_rank=0, use_dora=True, device="cpu")


# ------------------------------------------------------------------------------------------------ files
def test_config_of_a_plain_run_is_the_parents_and_a_dora_run_differs_in_one_key():
    from textboost_amd import checkpoint as ckpt
    assert ckpt.adapter_config(4, "tiny") == PARENT_CONFIG
    assert json.dumps(ckpt.adapter_config(4, "tiny"), indent=2, sort_keys=True) == json.dumps(PARENT_CONFIG, indent=2, sort_keys=True)
    d = ckpt.adapter_config(4, "tiny", list(LT.ALL), use_dora=True)
    assert d["use_dora"] is True and d == dict(PARENT_CONFIG, use_dora=True, target_modules=list(LT.ALL))
    assert not ckpt.has_dora_tensors(ckpt.lora_state_dict(stub_encoder(LT.ALL, 4, seed=0)))      # a plain encoder writes no magnitude key


@pytest.mark.parametrize("modules", [LT.QKV, LT.ALL], ids=["qkv", "six"])
def test_key_layout_and_round_trip_through_the_run_directory(tmp_path, modules):
    """save -> read_run_dir -> load is the identity; the magnitude of module <m> of layer i is `...layers.{i}.<path>.lora_magnitude_vector`,
    fp32 [N], beside lora_A.weight / lora_B.weight"""
    from safetensors.torch import load_file
    from textboost_amd import checkpoint as ckpt
    from textboost_amd import generate as G
    te = dora_stub(modules, 4, seed=0)
    d = write_run(str(tmp_path / "dog"), te, "<dog>")
    cfg = json.load(open(os.path.join(d, "text_encoder", "adapter_config.json")))
    assert cfg["use_dora"] is True and cfg["target_modules"] == list(modules) and cfg["r"] == cfg["lora_alpha"] == 4
    sd = load_file(os.path.join(d, "text_encoder", "adapter_model.safetensors"))
    assert set(sd) == {LT.key(i, n, w) for i in range(LAYERS) for n in modules for w in "AB"} | {DR.mkey(i, n) for i in range(LAYERS) for n in modules}
    assert DR.mkey(1, "k_proj") == "base_model.model.text_model.encoder.layers.1.self_attn.k_proj.lora_magnitude_vector"
    if "fc1" in modules:
        assert DR.mkey(0, "fc1") == "base_model.model.text_model.encoder.layers.0.mlp.fc1.lora_magnitude_vector"
    for i in range(LAYERS):
        for p, n in enumerate(LT.QKV):
            assert sd[DR.mkey(i, n)].dtype == torch.float32 and sd[DR.mkey(i, n)].shape == (D,)
            assert torch.equal(sd[DR.mkey(i, n)], te.mag[i, D * p:D * p + D])
        for n in modules[3:]:
            assert sd[DR.mkey(i, n)].shape == (SHAPES[n][1],) and torch.equal(sd[DR.mkey(i, n)], te.extra[n].mag[i])
    run = G.read_run_dir(d)
    assert run.use_dora and run.rank == 4 and G.lora_targets_of(run.lora) == modules and set(run.lora) == set(sd)
    te2 = dora_stub(modules, 4, seed=1)
    assert not torch.equal(te2.mag, te.mag)
    ckpt.load_lora_state_dict(te2, run.lora)
    assert torch.equal(te2.lora_A, te.lora_A) and torch.equal(te2.lora_B, te.lora_B) and torch.equal(te2.mag, te.mag)
    for n in modules[3:]:
        assert torch.equal(te2.extra[n].A, te.extra[n].A) and torch.equal(te2.extra[n].B, te.extra[n].B) and torch.equal(te2.extra[n].mag, te.extra[n].mag)


def test_reference_key_mapping_round_trips():
    """tests/dora_ref.py writes and reads the same keys as checkpoint.py"""
    from oracle.clip_text import CLIPTextCfg, TextBoostEncoder
    from textboost_amd import checkpoint as ckpt
    torch.manual_seed(0)
    enc = DR.add_dora(LT.add_adapters(TextBoostEncoder(CLIPTextCfg.tiny(D), r=4), LT.EXTRA, 4, seed=1), perturb=0.1)
    sd = DR.peft_state_dict(enc)
    te = dora_stub(LT.ALL, 4, seed=2)
    ckpt.load_lora_state_dict(te, sd)
    back = ckpt.lora_state_dict(te)
    assert set(back) == set(sd) and all(torch.equal(back[k], sd[k]) for k in sd)
    other = DR.add_dora(LT.add_adapters(TextBoostEncoder(CLIPTextCfg.tiny(D), r=4), LT.EXTRA, 4, seed=3))
    DR.load_peft_state_dict(other, back)
    for k, v in DR.magnitudes(enc).items():
        assert torch.equal(DR.magnitudes(other)[k], v), k


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_by_name(tmp_path):
    from safetensors.torch import load_file, save_file
    from textboost_amd import generate as G
    from textboost_amd.compose import adapter_support, compose_runs
    d = write_run(str(tmp_path / "dora"), dora_stub(LT.ALL, 4, seed=0), "<dog>")
    plain = G.read_run_dir(write_run(str(tmp_path / "plain"), stub_encoder(LT.ALL, 4, seed=1), "<style>"))
    run = G.read_run_dir(d)
    for runs in ([run, plain], [plain, run], [run]):
        with pytest.raises(NotImplementedError, match=r"dora.* is a use_dora run"):
            compose_runs(runs)
    with pytest.raises(NotImplementedError, match="use_dora"):
        adapter_support(run)
    assert compose_runs([plain]).rank == 4
    # use_dora in the config, no magnitude tensor in the file: today's refusal
    wpath = os.path.join(d, "text_encoder", "adapter_model.safetensors")
    sd = load_file(wpath)
    save_file({k: v for k, v in sd.items() if not k.endswith(".lora_magnitude_vector")}, wpath, metadata={"format": "pt"})
    with pytest.raises(NotImplementedError, match="use_dora"):
        G.read_run_dir(d)
    # magnitudes of only some adapted modules, or magnitudes without the flag
    save_file({k: v for k, v in sd.items() if k != DR.mkey(1, "fc2") and k != DR.mkey(0, "fc2")}, wpath, metadata={"format": "pt"})
    with pytest.raises(NotImplementedError, match="use_dora"):
        G.read_run_dir(d)
    save_file(sd, wpath, metadata={"format": "pt"})
    assert G.read_run_dir(d).use_dora
    cpath = os.path.join(d, "text_encoder", "adapter_config.json")
    cfg = json.load(open(cpath))
    for change, match in (({"use_dora": False}, "use_dora"), ({"lora_alpha": 8}, "lora_alpha"), ({"use_rslora": True}, "use_rslora")):
        json.dump(dict(cfg, **change), open(cpath, "w"))
        with pytest.raises(NotImplementedError, match=match):
            G.read_run_dir(d)


# ------------------------------------------------------------------------------------------------ the reference tests what we mean
def test_reference_gradients_are_the_formulas_with_the_norm_detached():
    """one DoRA Linear in float64: autograd through tests/dora_ref.py equals  dU = dY * c,  dm = colsum(dY * u) / n,  dB = s dU^T (x A^T),
    dA = s B^T dU^T x,  dx = dU W + s (dU B) A  at 1e-12 -- and WITHOUT the detach the adapter gradients move by far more than any bound the GPU
    tests use (the magnitude gradient does not: n enters dm the same way)."""
    from oracle.clip_text import LoRALinear
    torch.manual_seed(0)
    M, K, N, r, s = 37, 48, 40, 4, 1.0
    res = {}
    for detach in (True, False):
        torch.manual_seed(1)
        m = LoRALinear(K, N, r).double()
        with torch.no_grad():
            m.weight.normal_(std=0.2)
            m.lora_B.normal_(std=0.3)
            m.bias.normal_()
        DR.make_dora(m, detach=detach)
        with torch.no_grad():
            m.lora_magnitude_vector.mul_(1 + 0.3 * torch.randn(N, dtype=torch.float64))
        x = torch.randn(M, K, dtype=torch.float64, requires_grad=True)
        dY = torch.randn(M, N, dtype=torch.float64)
        y = m(x)
        y.backward(dY)
        res[detach] = (m, x, y.detach(), dY)
    m, x, y, dY = res[True]
    with torch.no_grad():
        yf, u, n, c = DR.dora_linear_f64(x, m.weight, m.bias, m.lora_A, m.lora_B, m.lora_magnitude_vector, s)
        dU = dY * c
        want = {"y": (y, yf), "dm": (m.lora_magnitude_vector.grad, (dY * u).sum(0) / n), "dB": (m.lora_B.grad, s * dU.T @ (x @ m.lora_A.T)),
                "dA": (m.lora_A.grad, s * m.lora_B.T @ dU.T @ x), "dx": (x.grad, dU @ m.weight + s * (dU @ m.lora_B) @ m.lora_A)}
    for k, (got, ref) in want.items():
        e = ((got - ref).norm() / ref.norm()).item()
        print(f"[dora ref] {k} autograd (norm detached) vs formula: {e:.3e}")
        assert e < 1e-12, k
    m2 = res[False][0]
    for k in ("lora_A", "lora_B"):
        gap = ((getattr(m2, k).grad - getattr(m, k).grad).norm() / getattr(m, k).grad.norm()).item()
        print(f"[dora ref] {k} gradient without the detach: {gap:.3e} away")
        assert gap > 5e-2, k           # ten times the widest gradient bound of tests/test_gpu_dora.py (5e-3)
    assert torch.allclose(m2.lora_magnitude_vector.grad, m.lora_magnitude_vector.grad, rtol=1e-12, atol=0)


def test_dora_at_init_is_plain_lora_in_the_reference():
    """m = ||W||, B = 0: c = 1 and the layer is the plain LoRA layer"""
    from oracle.clip_text import LoRALinear
    torch.manual_seed(2)
    m = LoRALinear(32, 24, 4).double()
    x = torch.randn(5, 32, dtype=torch.float64)
    plain = m(x)
    DR.make_dora(m)
    assert torch.allclose(m.lora_magnitude_vector, m.weight.norm(dim=1)) and torch.allclose(m(x), plain, rtol=1e-13, atol=1e-13)
