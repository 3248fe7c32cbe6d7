"""CPU tests of the DINO score (textboost_amd/dino_score.py, eval_dreambooth.py --metric dino): the fp32 restatement (tests/dino_ref.py)
against transformers' Dinov2Model, the hub's offset interpolation of the position embeddings, the two weight formats, the per-instance means
against a padded, masked restatement, N from the run path, and the CLI's host logic."""
import csv
import json
import os

import numpy as np
import pytest
import torch

import dino_ref as R


def tiny_config(image_size=224, D=128, layers=2, heads=2):
    return {"model_type": "dinov2", "hidden_size": D, "num_hidden_layers": layers, "num_attention_heads": heads, "mlp_ratio": 4,
            "hidden_act": "gelu", "layer_norm_eps": 1e-6, "image_size": image_size, "patch_size": 14, "num_channels": 3, "qkv_bias": True,
            "layerscale_value": 1.0, "use_swiglu_ffn": False}


def hf_model(cfg, seed):
    """a transformers Dinov2Model with random weights, LayerScale drawn from [1e-5, 1e-3] and [0.05, 1] (not its init value 1)"""
    transformers = pytest.importorskip("transformers")
    torch.manual_seed(seed)
    m = transformers.Dinov2Model(transformers.Dinov2Config(**cfg)).eval().float()
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith("lambda1"):
                small = torch.rand(p.shape, generator=g) < 0.5
                p.copy_(torch.where(small, 1e-5 + torch.rand(p.shape, generator=g) * 1e-3, 0.05 + torch.rand(p.shape, generator=g) * 0.95))
            elif "norm" in name:
                p.add_(0.05 * torch.randn(p.shape, generator=g))
            elif name.endswith("bias") or "token" in name or "position" in name:
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
    return m


def hub_names(sd, layers):
    """the test's own transformers -> hub name table (written out, not the module's)"""
    out = {"cls_token": sd["embeddings.cls_token"], "pos_embed": sd["embeddings.position_embeddings"],
           "patch_embed.proj.weight": sd["embeddings.patch_embeddings.projection.weight"],
           "patch_embed.proj.bias": sd["embeddings.patch_embeddings.projection.bias"],
           "norm.weight": sd["layernorm.weight"], "norm.bias": sd["layernorm.bias"], "mask_token": sd["embeddings.mask_token"]}
    for i in range(layers):
        t, b = f"encoder.layer.{i}.", f"blocks.{i}."
        a = t + "attention.attention."
        out[b + "attn.qkv.weight"] = torch.cat([sd[a + "query.weight"], sd[a + "key.weight"], sd[a + "value.weight"]])
        out[b + "attn.qkv.bias"] = torch.cat([sd[a + "query.bias"], sd[a + "key.bias"], sd[a + "value.bias"]])
        out[b + "attn.proj.weight"], out[b + "attn.proj.bias"] = sd[t + "attention.output.dense.weight"], sd[t + "attention.output.dense.bias"]
        out[b + "ls1.gamma"], out[b + "ls2.gamma"] = sd[t + "layer_scale1.lambda1"], sd[t + "layer_scale2.lambda1"]
        for n in ("norm1", "norm2", "mlp.fc1", "mlp.fc2"):
            out[b + n + ".weight"], out[b + n + ".bias"] = sd[t + n + ".weight"], sd[t + n + ".bias"]
    return out


def test_restatement_matches_transformers():
    """at the model's native grid (no interpolation) the restatement is Dinov2Model's pooler_output"""
    cfg = tiny_config()
    m = hf_model(cfg, 3)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    g = torch.Generator().manual_seed(0)
    u8 = torch.randint(0, 256, (3, 224, 224, 3), generator=g, dtype=torch.uint8).numpy()
    px = R.normalise(u8)
    with torch.no_grad():
        want = m(pixel_values=px).pooler_output
        got = R.features(hub_names(sd, cfg["num_hidden_layers"]), px, cfg["num_attention_heads"])
    err = ((got - want).norm() / want.norm()).item()
    assert err < 1e-5, err


def test_interpolation_is_the_hubs_offset_form():
    from textboost_amd.dino_score import interpolate_pos_embed
    g = torch.Generator().manual_seed(1)
    D = 32
    pe = torch.randn(1, 1 + 37 * 37, D, generator=g)
    got = interpolate_pos_embed(pe, 16, 0.1)
    grid = pe[0, 1:].reshape(1, 37, 37, D).permute(0, 3, 1, 2)
    want = torch.nn.functional.interpolate(grid, scale_factor=16.1 / 37, mode="bicubic", antialias=False)
    assert want.shape[-2:] == (16, 16)
    assert torch.equal(got[0], pe[0, 0]) and torch.equal(got[1:], want.permute(0, 2, 3, 1).reshape(256, D))
    assert torch.equal(got, R.hub_interpolate_pos_encoding(pe, 256, 224, 224, 14)[0])
    # transformers' Dinov2Embeddings: size=(16, 16) maps coordinates with the exact ratio 37 / 16 -- measurably not the hub's
    sized = torch.nn.functional.interpolate(grid, size=(16, 16), mode="bicubic", align_corners=False).permute(0, 2, 3, 1).reshape(256, D)
    diff = (got[1:] - sized).abs().max().item()
    assert diff > 0.05 * pe.abs().max().item(), diff
    assert torch.equal(interpolate_pos_embed(pe, 37), pe[0])   # the native grid is not interpolated


def test_hub_and_transformers_formats_give_the_same_features(tmp_path):
    """the module's transformers -> hub mapping equals the test's own table, and the two formats give one feature; the transformers directory
    loads through load_dino_model; the hub file loader takes ViT-L/14 shapes only"""
    from safetensors.torch import save_file
    from textboost_amd import dino_score as DS
    cfg = tiny_config(image_size=98)   # a 7 x 7 trained grid, interpolated to 16 x 16 at 224 px
    m = hf_model(cfg, 4)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    geo = DS.geometry_from_transformers_config(cfg)
    assert (geo.pos_grid, geo.grid, geo.intermediate_size, geo.eps) == (7, 16, 512, 1e-6)
    mapped = DS.hub_state_from_transformers(sd, geo)
    own = hub_names(sd, cfg["num_hidden_layers"])
    assert set(mapped) == set(own) - {"mask_token"} and all(torch.equal(mapped[k], own[k]) for k in mapped)
    d = tmp_path / "dinov2"
    d.mkdir()
    (d / "config.json").write_text(json.dumps(dict(cfg, architectures=["Dinov2Model"])))
    save_file({k: v.contiguous() for k, v in sd.items()}, str(d / "model.safetensors"))
    geo2, state = DS.load_dino_model(str(d))
    assert geo2 == geo and all(torch.equal(state[k], mapped[k]) for k in mapped)
    g = torch.Generator().manual_seed(2)
    px = R.normalise(torch.randint(0, 256, (2, 224, 224, 3), generator=g, dtype=torch.uint8).numpy())
    with torch.no_grad():
        a = R.features(state, px, cfg["num_attention_heads"])
        b = R.features(own, px, cfg["num_attention_heads"])
    assert torch.equal(a, b)
    # the hub file: ViT-L/14 only
    torch.save(own, str(tmp_path / "tiny.pth"))
    with pytest.raises(ValueError, match="ViT-L/14"):
        DS.load_dino_model(str(tmp_path / "tiny.pth"))
    with pytest.raises(NotImplementedError, match="register"):
        DS.check_hub_state(dict(own, register_tokens=torch.zeros(1, 4, 128)), geo)


def test_full_size_layouts_agree():
    """hub_state_shapes(ViT-L/14) is what transformers' dinov2-large Dinov2Model maps to (shapes only, on the meta device)"""
    transformers = pytest.importorskip("transformers")
    from textboost_amd import dino_score as DS
    cfg = tiny_config(image_size=518, D=1024, layers=24, heads=16)
    geo = DS.geometry_from_transformers_config(cfg)
    assert geo == DS.DINOV2_VITL14 and geo.num_tokens == 257
    with torch.device("meta"):
        m = transformers.Dinov2Model(transformers.Dinov2Config(**cfg))
    mapped = DS.hub_state_from_transformers(dict(m.state_dict()), geo)
    assert {k: tuple(v.shape) for k, v in mapped.items()} == DS.hub_state_shapes(geo)
    assert DS.hub_state_shapes(geo)["pos_embed"] == (1, 1370, 1024)


@pytest.mark.parametrize("key,value,match", [("use_swiglu_ffn", True, "swiglu"), ("hidden_act", "silu", "hidden_act"),
                                             ("num_register_tokens", 4, "register"), ("model_type", "dinov2_with_registers", "register"),
                                             ("qkv_bias", False, "qkv")])
def test_transformers_config_refusals(key, value, match):
    from textboost_amd.dino_score import geometry_from_transformers_config
    with pytest.raises(NotImplementedError, match=match):
        geometry_from_transformers_config(dict(tiny_config(), **{key: value}))


def test_dino_scores_match_the_padded_restatement():
    """uneven real-image counts (padding + mask), negative cosines (no clamp), instances listed unsorted"""
    from textboost_amd.dino_score import dino_scores
    g = torch.Generator().manual_seed(6)
    D = 16
    real = {"dog": torch.randn(5, D, generator=g), "can": torch.randn(3, D, generator=g), "cat": torch.randn(4, D, generator=g)}
    gen = {"can": torch.randn(3, D, generator=g), "dog": -real["dog"][:2] + 0.1 * torch.randn(2, D, generator=g),
           "cat": torch.randn(4, D, generator=g)}
    names = [k for k in sorted(gen) for _ in range(gen[k].shape[0])]
    feats = torch.cat([gen[k] for k in sorted(gen)])
    for N in (1, 2):
        want_s, want_u = R.padded_means(feats, names, real, N)
        pairs = [dino_scores(gen[k], real[k], N) for k in sorted(gen)]
        got_s, got_u = torch.cat([p[0] for p in pairs]), torch.cat([p[1] for p in pairs])
        assert torch.allclose(got_s, want_s, atol=1e-6) and torch.allclose(got_u, want_u, atol=1e-6), (N, got_s, want_s, got_u, want_u)
        assert (got_s < 0).any()   # the dog images point away from their real images: no clamp at 0
    with pytest.raises(ValueError):
        dino_scores(gen["can"], real["can"], 3)   # no unseen image
    with pytest.raises(ValueError):
        dino_scores(gen["can"], real["can"], 0)


# ------------------------------------------------------------------------------------------------------------------ CLI host logic
def test_n_from_the_run_path():
    import eval_dreambooth as E
    assert E.parse_n_seen("out/tb-sd15-n1") == 1
    assert E.parse_n_seen("out/tb-sd15-n3/") == 3
    assert E.parse_n_seen("tb-sd21-n12-extra") == 12
    for bad in ("out/tb-sd15", "out/tb_sd15_n1", "out/tb-sd15-x", "/tmp/pytest-of-u/tb-sd15-n1", "out/tb-sd15-n0"):
        with pytest.raises(SystemExit, match="dino"):
            E.parse_n_seen(bad)


def _args(tmp_path, *extra, run="tb-sd15-n1"):
    import eval_dreambooth as E
    return E.build_parser().parse_args([os.path.join("runs", run), "--outdir", str(tmp_path / "bench"), *extra])


def test_cli_refusals_dino(tmp_path):
    import eval_dreambooth as E
    with pytest.raises(SystemExit, match="--dino-model"):
        E.check_args(_args(tmp_path, "--skip-gen", "--metric", "dino"))
    E.check_args(_args(tmp_path, "--skip-gen", "--metric", "dino", "--dino-model", "x.pth"))      # no --clip-model needed
    with pytest.raises(SystemExit, match="--clip-model"):
        E.check_args(_args(tmp_path, "--skip-gen", "--metric", "clip-t", "dino", "--dino-model", "x.pth"))
    with pytest.raises(SystemExit, match="pass --metric clip-t clip-i"):
        E.check_args(_args(tmp_path, "--skip-gen", "--metric", "vqa", "dino", "--dino-model", "x.pth"))
    seed = tmp_path / "bench" / "tb-sd15-n1" / "seed0"
    for inst in ("dog", "can"):
        (seed / inst).mkdir(parents=True)
        (seed / inst / "a_dog.png").write_bytes(b"")
    db = tmp_path / "db"
    for inst, n in (("dog", 3), ("can", 1)):
        (db / inst).mkdir(parents=True)
        for k in range(n):
            (db / inst / f"{k:02d}.jpg").write_bytes(b"")
    a = _args(tmp_path, "--skip-gen", "--metric", "dino", "--seeds", "0", "--dreambooth-path", str(db), "--dino-model", "x.pth")
    with pytest.raises(SystemExit, match="instance 'can' has 1 real images"):
        E.evaluate(a, dino_evaluator=object())
    (db / "can").rename(db / "cans")
    with pytest.raises(SystemExit, match="no images for instance 'can'"):
        E.evaluate(a, dino_evaluator=object())
    (db / "cans").rename(db / "can")
    (seed.parent.parent / "tb_sd15_n1").symlink_to(seed.parent)
    a = _args(tmp_path, "--skip-gen", "--metric", "dino", "--seeds", "0", "--dreambooth-path", str(db), "--dino-model", "x.pth",
              run="tb_sd15_n1")
    with pytest.raises(SystemExit, match="cannot parse"):
        E.evaluate(a, dino_evaluator=object())


class _FakeDINO:
    """features chosen per file name: the CLI's bookkeeping under test, not the tower"""
    batch_size, tower_images = 32, 0

    class geo:
        image_size = 224

    def __init__(self, table):
        self.table, self.calls = table, []

    def encode_images(self, paths):
        self.calls.append(list(paths))
        return torch.stack([self.table[os.path.basename(p)] for p in paths])

    def images_per_second(self):
        return 0.0


def test_cli_dino_means_and_csv(tmp_path, monkeypatch):
    import eval_dreambooth as E
    g = torch.Generator().manual_seed(8)
    table, gen, real = {}, {}, {}
    for s in (0, 1):
        for inst in ("dog", "can"):
            d = tmp_path / "bench" / "tb-sd15-n2" / f"seed{s}" / inst
            d.mkdir(parents=True)
            for k in range(3):
                name = f"s{s}_a_{inst}_{k}.png"
                (d / name).write_bytes(b"")
                table[name] = torch.randn(8, generator=g)
                gen.setdefault(s, {}).setdefault(inst, []).append(name)
    for inst, n in (("dog", 5), ("can", 3), ("unused", 1)):   # an instance without generated images is not in use
        d = tmp_path / "db" / inst
        d.mkdir(parents=True)
        for k in range(n):
            name = f"{inst}_{k:02d}.{'jpg' if k % 2 else 'png'}"
            (d / name).write_bytes(b"")
            table[name] = torch.randn(8, generator=g)
            real.setdefault(inst, []).append(name)
    (tmp_path / "runs" / "tb-sd15-n2").mkdir(parents=True)
    monkeypatch.chdir(tmp_path)
    a = E.build_parser().parse_args(["runs/tb-sd15-n2", "--outdir", "bench", "--skip-gen", "--metric", "dino", "--seeds", "0", "1",
                                     "--dreambooth-path", "db", "--dino-model", "x.pth"])
    E.check_args(a)
    fake = _FakeDINO(table)
    res = E.evaluate(a, dino_evaluator=fake)
    assert sum(len(c) for c in fake.calls) == 5 + 3 + 2 * 6   # every real image once per run
    rows = list(csv.reader(open(tmp_path / "runs" / "tb-sd15-n2" / "metric_last.csv")))
    assert rows[0] == ["seed", "clip_score", "vqa_score", "clip_i", "clip_i_unseen", "dino", "dino_unseen"]
    rf = {inst: torch.stack([table[n] for n in real[inst]]) for inst in ("dog", "can")}
    for s, row in zip((0, 1), rows[1:]):
        names = [inst for inst in sorted(gen[s]) for _ in gen[s][inst]]
        feats = torch.stack([table[n] for inst in sorted(gen[s]) for n in gen[s][inst]])
        ws, wu = R.padded_means(feats, names, rf, 2)
        assert torch.allclose(res[s]["dino"], ws, atol=1e-6) and torch.allclose(res[s]["dino_unseen"], wu, atol=1e-6)
        assert row == [str(s), "0.000", "0.000", "0.000", "0.000", f"{ws.mean():.3f}", f"{wu.mean():.3f}"]
