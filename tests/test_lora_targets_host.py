"""Host side of --lora_target_modules (text-encoder LoRA on out_proj / fc1 / fc2 beside q/k/v): the flag, the adapter files, the run-directory
reader and composition.  No GPU."""
import json
import os
import types

import pytest
import torch

import lora_targets_ref as LT

D, I, LAYERS = 64, 128, 2
SHAPES = {"q_proj": (D, D), "k_proj": (D, D), "v_proj": (D, D), "out_proj": (D, D), "fc1": (D, I), "fc2": (I, D)}   # (K_in, N_out)
BASE = ["--pretrained_model_name_or_path", "x"]


def stub_encoder(modules, rank, seed):
    """the attributes of a HipTextEncoder that checkpoint.py reads, with trained-looking (non-zero B) adapters on `modules`"""
    g = torch.Generator().manual_seed(seed)
    extra = {n: types.SimpleNamespace(A=torch.randn(LAYERS, rank, SHAPES[n][0], generator=g) / rank,
                                      B=torch.randn(LAYERS, SHAPES[n][1], rank, generator=g) * 0.05) for n in LT.EXTRA if n in modules}
    return types.SimpleNamespace(geo=types.SimpleNamespace(hidden_size=D, num_layers=LAYERS), r=rank, extra=extra,
                                 lora_A=torch.randn(LAYERS, 3 * rank, D, generator=g) / rank,
                                 lora_B=torch.randn(LAYERS, 3 * D, rank, generator=g) * 0.05, token_table=torch.randn(2, D, generator=g) * 0.01)


def write_run(d, te, token):
    from textboost_amd import checkpoint as ckpt
    ckpt.save_text_encoder_adapter(te, os.path.join(d, "text_encoder"), "tiny")
    ckpt.save_token_embeddings(te, d, {token: 0}, None)
    return d


# ------------------------------------------------------------------------------------------------ the flag
def test_flag_parses_and_defaults_to_qkv():
    from textboost_amd import cli
    assert cli.parse_args(BASE).lora_target_modules == ["q_proj", "k_proj", "v_proj"]
    a = cli.parse_args(BASE + ["--lora_target_modules", "fc2", "q_proj", "k_proj", "v_proj", "out_proj", "fc1", "--lora_rank", "8"])
    assert a.lora_target_modules == list(LT.ALL) and a.lora_rank == 8        # canonical order whatever the command line's
    assert cli.parse_args(BASE + ["--lora_target_modules", "q_proj", "k_proj", "v_proj", "fc2"]).lora_target_modules == list(LT.QKV) + ["fc2"]
    with pytest.raises(SystemExit):
        cli.parse_args(BASE + ["--lora_target_modules", "q_proj", "k_proj", "v_proj", "proj_out"])


def test_a_list_without_k_proj_is_refused_by_name():
    from textboost_amd import cli
    from textboost_amd.text_encoder import check_lora_targets
    with pytest.raises(ValueError, match=r"--lora_target_modules.*k_proj missing"):
        cli.parse_args(BASE + ["--lora_target_modules", "q_proj", "v_proj", "fc1"])
    with pytest.raises(ValueError, match=r"--lora_target_modules.*k_proj missing"):      # the encoder's own check (a caller that is not the CLI)
        check_lora_targets(["q_proj", "v_proj", "fc1"])
    assert check_lora_targets(None) == () and check_lora_targets(["fc2", "v_proj", "q_proj", "k_proj", "out_proj"]) == ("out_proj", "fc2")


def test_flag_table_still_reports_the_reference_flags_only():
    from textboost_amd import cli
    golden = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "cli_flags.json")))
    table = cli.flag_table()
    assert table == golden and len(table) == 66
    assert [n for n, _ in cli.EXTENSION_FLAGS] == ["--lora_target_modules"]
    assert not any("--lora_target_modules" in f["flags"] for f in table)
    assert "--lora_target_modules" in cli.build_parser().format_help()


# ------------------------------------------------------------------------------------------------ write -> read -> load
def test_six_module_adapter_round_trips_through_the_run_directory(tmp_path):
    from safetensors.torch import load_file
    from textboost_amd import checkpoint as ckpt
    from textboost_amd import generate as G
    te = stub_encoder(LT.ALL, 4, seed=0)
    d = write_run(str(tmp_path / "dog"), te, "<dog>")
    cfg = json.load(open(os.path.join(d, "text_encoder", "adapter_config.json")))
    assert cfg["target_modules"] == list(LT.ALL) and cfg["r"] == 4 and cfg["lora_alpha"] == 4
    sd = load_file(os.path.join(d, "text_encoder", "adapter_model.safetensors"))
    assert set(sd) == {LT.key(i, n, w) for i in range(LAYERS) for n in LT.ALL for w in "AB"}
    for i in range(LAYERS):
        for n in LT.ALL:
            K, N = SHAPES[n]
            assert sd[LT.key(i, n, "A")].shape == (4, K) and sd[LT.key(i, n, "B")].shape == (N, 4), (i, n)
        for p, n in enumerate(LT.QKV):
            assert torch.equal(sd[LT.key(i, n, "A")], te.lora_A[i, 4 * p:4 * p + 4]) and torch.equal(sd[LT.key(i, n, "B")], te.lora_B[i, D * p:D * p + D])
        for n in LT.EXTRA:
            assert torch.equal(sd[LT.key(i, n, "A")], te.extra[n].A[i]) and torch.equal(sd[LT.key(i, n, "B")], te.extra[n].B[i])
    run = G.read_run_dir(d)
    assert run.rank == 4 and G.lora_targets_of(run.lora) == LT.ALL and set(run.lora) == set(sd)
    te2 = stub_encoder(LT.ALL, 4, seed=1)
    ckpt.load_lora_state_dict(te2, run.lora)
    assert torch.equal(te2.lora_A, te.lora_A) and torch.equal(te2.lora_B, te.lora_B)
    for n in LT.EXTRA:
        assert torch.equal(te2.extra[n].A, te.extra[n].A) and torch.equal(te2.extra[n].B, te.extra[n].B)
    # a subset: only the trained modules are written and listed
    sub = write_run(str(tmp_path / "sub"), stub_encoder(LT.QKV + ("fc2",), 8, seed=2), "<s>")
    assert json.load(open(os.path.join(sub, "text_encoder", "adapter_config.json")))["target_modules"] == list(LT.QKV) + ["fc2"]
    assert G.lora_targets_of(G.read_run_dir(sub).lora) == LT.QKV + ("fc2",)
    # the file and the list must agree in both directions
    p = os.path.join(sub, "text_encoder", "adapter_config.json")
    c = json.load(open(p))
    c["target_modules"] = list(LT.QKV)
    json.dump(c, open(p, "w"))
    with pytest.raises(NotImplementedError, match="target_modules"):
        G.read_run_dir(sub)


# ------------------------------------------------------------------------------------------------ composition
@pytest.fixture()
def two_runs(tmp_path):
    from textboost_amd import generate as G
    a = write_run(str(tmp_path / "dog"), stub_encoder(LT.ALL, 4, seed=3), "<dog>")
    b = write_run(str(tmp_path / "style"), stub_encoder(LT.QKV + ("fc2",), 8, seed=4), "<style>")
    return G.read_run_dir(a), G.read_run_dir(b)


def merged_delta(parts, i, n, dtype=torch.float64):
    """sum_i w_i B_i A_i of module n of layer i over the [(run, w)] that adapt it"""
    return sum(w * (run.lora[LT.key(i, n, "B")].to(dtype) @ run.lora[LT.key(i, n, "A")].to(dtype)) for run, w in parts if LT.key(i, n, "A") in run.lora)


def test_composition_per_module_is_the_weighted_sum_in_float64(two_runs):
    """six modules at rank 4 + q/k/v/fc2 at rank 8, weights (1, 0.8): every module of the composed run has rank 12 (out_proj and fc1 padded with
    zero A rows / zero B columns), B_c A_c = sum_i w_i B_i A_i at 1e-6 in float64 (the only rounding: w * B in fp32), and the oracle encoder
    carrying the composed adapter equals the oracle with the sums merged into its weights at 1e-5 -- the bounds of tests/test_compose_host.py."""
    from oracle.clip_text import CLIPTextCfg, TextBoostEncoder
    from textboost_amd import generate as G
    from textboost_amd.compose import compose_runs
    a, b = two_runs
    w = (1.0, 0.8)
    c = compose_runs([a, b], w)
    assert c.rank == 12 and G.lora_targets_of(c.lora) == LT.ALL and set(c.lora) == set(a.lora)
    worst = 0.0
    for i in range(LAYERS):
        for n in LT.ALL:
            A, B = c.lora[LT.key(i, n, "A")], c.lora[LT.key(i, n, "B")]
            K, N = SHAPES[n]
            assert A.shape == (12, K) and B.shape == (N, 12) and A.dtype == B.dtype == torch.float32 and A.is_contiguous() and B.is_contiguous()
            if n in ("out_proj", "fc1"):     # only run a adapts them: its tensors, then exact zeros
                assert torch.equal(A[:4], a.lora[LT.key(i, n, "A")]) and torch.equal(B[:, :4], a.lora[LT.key(i, n, "B")])
                assert not A[4:].any() and not B[:, 4:].any()
            got, want = B.double() @ A.double(), merged_delta([(a, w[0]), (b, w[1])], i, n)
            worst = max(worst, ((got - want).norm() / want.norm()).item())
    print(f"[lora targets] B_c A_c vs sum w_i B_i A_i in float64: worst rel-L2 {worst:.2e}")
    assert worst <= 1e-6
    torch.manual_seed(0)
    ccfg = CLIPTextCfg.tiny(D)
    base = TextBoostEncoder(ccfg, r=0)
    with torch.no_grad():
        for name, p in base.named_parameters():
            if "ln" in name or name.endswith("bias"):
                p.add_(torch.randn_like(p) * 0.1)
        base.token_embedding.weight.mul_(0.5)
        composed = LT.add_adapters(TextBoostEncoder(ccfg, r=12), LT.EXTRA, 12, seed=0)
        composed.load_state_dict(base.state_dict(), strict=False)
        LT.load_peft_state_dict(composed, c.lora)
        merged = TextBoostEncoder(ccfg, r=0)
        merged.load_state_dict(base.state_dict())
        base, composed, merged = base.double(), composed.double(), merged.double()
        for i in range(LAYERS):
            for n in LT.ALL:
                getattr(merged.layers[i], LT.ATTR[n]).weight.add_(merged_delta([(a, w[0]), (b, w[1])], i, n))
        ids = torch.randint(0, 49406, (4, 77), generator=torch.Generator().manual_seed(5))
        ids[:, 0] = 49406
        for row, n_ in enumerate((9, 23, 2, 77)):
            ids[row, n_ - 1:] = 49407
        out, ref, plain = composed(ids), merged(ids), base(ids)
    e = ((out - ref).norm() / ref.norm()).item()
    far = ((plain - ref).norm() / ref.norm()).item()
    print(f"[lora targets] oracle, composed six-module adapter vs merged weights: rel-L2 {e:.2e} (<= 1e-5); base encoder vs merged: {far:.2e}")
    assert e <= 1e-5
    assert far > 1e-3               # the adapters matter on these inputs


def test_composition_refusals_with_extra_modules(two_runs):
    from textboost_amd import generate as G
    from textboost_amd.compose import compose_runs
    a, b = two_runs
    assert G.lora_targets_of(compose_runs([b, a]).lora) == LT.ALL              # the order of the runs does not decide which modules exist
    assert G.lora_targets_of(compose_runs([a, b], [0.0, 1.0]).lora) == LT.QKV + ("fc2",)
    fewer = G.TrainedRun(path="fewer", rank=4, lora={k: v for k, v in a.lora.items() if ".layers.0.self_attn.k_proj" not in k})
    with pytest.raises(ValueError, match="different modules"):
        compose_runs([b, fewer])
    ragged = G.TrainedRun(path="ragged", rank=4, lora={k: v for k, v in a.lora.items() if ".layers.1.mlp.fc1" not in k})
    with pytest.raises(ValueError, match="different modules"):
        compose_runs([b, ragged])
