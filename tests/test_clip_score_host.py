"""CPU tests of the CLIP-T / CLIP-I evaluation (textboost_amd/clip_score.py, eval_dreambooth.py): the fp32 restatement (tests/clip_ref.py)
against transformers' CLIPModel, Pillow's BILINEAR through the library's coefficient tables, the patch-weight fold, and the CLI's host logic
(paths, CSV, metric means, refusals)."""
import csv
import os

import numpy as np
import pytest
import torch

import clip_ref as R

PRECISION_BITS = 32 - 8 - 2   # Resample.c


def tiny_config(image_size=224, patch=14, Dv=128, Dt=64, layers=2, proj=64, vocab=514):
    return {"projection_dim": proj,
            "vision_config": {"image_size": image_size, "patch_size": patch, "hidden_size": Dv, "intermediate_size": 4 * Dv,
                              "num_hidden_layers": layers, "num_attention_heads": Dv // 64, "hidden_act": "quick_gelu", "layer_norm_eps": 1e-5},
            "text_config": {"vocab_size": vocab, "hidden_size": Dt, "intermediate_size": 4 * Dt, "num_hidden_layers": layers,
                            "num_attention_heads": max(1, Dt // 32), "max_position_embeddings": 77, "hidden_act": "quick_gelu",
                            "layer_norm_eps": 1e-5, "eos_token_id": vocab - 1, "bos_token_id": vocab - 2, "pad_token_id": vocab - 1}}


def random_clip(cfg, seed):
    from textboost_amd import models
    from textboost_amd.clip_score import clip_model_geometry_from_config
    vg, tg, _ = clip_model_geometry_from_config(cfg)
    return models.random_state_dict(models.clip_model_shapes(vg, tg), seed)


def hf_model(cfg, sd):
    transformers = pytest.importorskip("transformers")
    c = transformers.CLIPConfig(text_config=cfg["text_config"], vision_config=cfg["vision_config"], projection_dim=cfg["projection_dim"])
    m = transformers.CLIPModel(c).eval().float()
    ref = m.state_dict()
    manifest = {k for k in ref if not k.endswith("position_ids") and k != "logit_scale"}
    assert manifest == set(sd), (sorted(manifest ^ set(sd)))[:10]       # the shape spec names exactly the model's parameters
    for k in manifest:
        assert tuple(ref[k].shape) == tuple(sd[k].shape), k
    m.load_state_dict(sd, strict=False)
    return m


def _ids(cfg, B, g):
    t = cfg["text_config"]
    V, eos = t["vocab_size"], t["eos_token_id"]
    ids = torch.full((B, 77), eos, dtype=torch.int64)
    for b in range(B):
        n = 3 + 5 * b
        ids[b, 0] = t["bos_token_id"]
        ids[b, 1:n] = torch.randint(0, V - 2, (n - 1,), generator=g)
    return ids


@pytest.mark.parametrize("full", [False, True], ids=["tiny", "vit_l14_336"])
def test_restatement_matches_transformers(full):
    pytest.importorskip("transformers")
    from textboost_amd import models
    cfg = tiny_config() if not full else {
        "projection_dim": 768,
        "vision_config": {"image_size": 336, "patch_size": 14, "hidden_size": 1024, "intermediate_size": 4096, "num_hidden_layers": 24,
                          "num_attention_heads": 16, "hidden_act": "quick_gelu", "layer_norm_eps": 1e-5},
        "text_config": {"vocab_size": 49408, "hidden_size": 768, "intermediate_size": 3072, "num_hidden_layers": 12, "num_attention_heads": 12,
                        "max_position_embeddings": 77, "hidden_act": "quick_gelu", "layer_norm_eps": 1e-5, "eos_token_id": 49407,
                        "bos_token_id": 49406, "pad_token_id": 49407}}
    if full:
        from textboost_amd.clip_score import clip_model_geometry_from_config
        vg, tg, eos = clip_model_geometry_from_config(cfg)
        assert (vg, tg, eos) == (models.CLIP_VIT_L14_336, models.CLIP_VIT_L14_TEXT, 49407)
    sd = random_clip(cfg, 5)
    m = hf_model(cfg, sd)
    g = torch.Generator().manual_seed(0)
    S = cfg["vision_config"]["image_size"]
    B = 1 if full else 3
    u8 = torch.randint(0, 256, (B, S, S, 3), generator=g, dtype=torch.uint8).numpy()
    ids = _ids(cfg, B, g)
    px = R.normalise(u8)
    with torch.no_grad():
        out = m(input_ids=ids, pixel_values=px)   # CLIPOutput's embeds are L2-normalised; the projections' outputs are not
        ie_hf = m.visual_projection(m.vision_model(pixel_values=px).pooler_output)
        te_hf = m.text_projection(m.text_model(input_ids=ids).pooler_output)
        ie, te = R.image_embeds(sd, cfg, px), R.text_embeds(sd, cfg, ids)
    for name, a, b in (("image", ie, ie_hf), ("text", te, te_hf), ("image normalised", ie / ie.norm(dim=-1, keepdim=True), out.image_embeds),
                       ("text normalised", te / te.norm(dim=-1, keepdim=True), out.text_embeds)):
        err = ((a - b).norm() / b.norm()).item()
        assert err < 1e-5, (name, err)
    assert torch.allclose(R.clip_t(ie, te), (out.image_embeds * out.text_embeds).sum(-1), atol=1e-5)


# ------------------------------------------------------------------------------------------------------------------ BILINEAR
def _apply_axis(a, bounds, kk, axis):
    a = np.moveaxis(a.astype(np.int64), axis, 0)
    out = np.empty((bounds.shape[0],) + a.shape[1:], dtype=np.int64)
    for xx in range(bounds.shape[0]):
        xmin, cnt = bounds[xx]
        k = kk[xx, :cnt].astype(np.int64).reshape((cnt,) + (1,) * (a.ndim - 1))
        ss = (1 << (PRECISION_BITS - 1)) + (a[xmin:xmin + cnt] * k).sum(0)
        out[xx] = np.clip(ss >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis).astype(np.uint8)


def _resize_host(a, w, h, filt):
    from textboost_amd import ops
    H, W = a.shape[:2]
    if w != W:
        _, b, kk = ops.resample_coeffs(W, w, filt)
        a = _apply_axis(a, b.numpy(), kk.numpy(), 1)
    if h != H:
        _, b, kk = ops.resample_coeffs(H, h, filt)
        a = _apply_axis(a, b.numpy(), kk.numpy(), 0)
    return a


def test_bilinear_coefficients_reproduce_pillow():
    from PIL import Image
    from textboost_amd import _lib as L
    rng = np.random.default_rng(3)
    cases = [((37, 53), (512, 512)), ((600, 410), (512, 512)), ((512, 512), (336, 336)), ((1, 7), (5, 1)), ((9, 1), (1, 4)),
             ((100, 33), (17, 250)), ((512, 683), (512, 512)), ((3, 3), (2, 9))]
    for (h, w), (oh, ow) in cases:
        a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        want = np.asarray(Image.fromarray(a).resize((ow, oh), Image.BILINEAR))
        got = _resize_host(a, ow, oh, L.IMG_BILINEAR)
        assert np.array_equal(got, want), ((h, w), (oh, ow), int(np.abs(got.astype(int) - want).max()))
    for (h, w), (oh, ow) in cases[:3]:   # the other filters' tables are unchanged
        a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        for f, pf in ((L.IMG_BICUBIC, Image.BICUBIC), (L.IMG_LANCZOS, Image.LANCZOS)):
            assert np.array_equal(_resize_host(a, ow, oh, f), np.asarray(Image.fromarray(a).resize((ow, oh), pf)))


def test_bilinear_ksize_and_unknown_filter():
    from textboost_amd import _lib as L, ops
    assert L.lib().tb_resample_ksize(512, 336, L.IMG_BILINEAR) == 2 * int(np.ceil(512 / 336)) + 1
    assert L.lib().tb_resample_ksize(100, 200, L.IMG_BILINEAR) == 3
    assert L.lib().tb_resample_ksize(8, 4, 2) == -22   # the ABI's BILINEAR id is not Pillow's 2: ids refused before stay refused
    with pytest.raises(RuntimeError):
        ops.resample_coeffs(10, 5, 4)   # BOX is not built


# ------------------------------------------------------------------------------------------------------------------ the fold
def test_patch_weight_fold_restates_normalise_then_conv():
    """W' . bytes + bias == conv(normalise(bytes), W) in float64: the fold itself is exact algebra; only its 16-bit rounding is not."""
    from textboost_amd.clip_score import pack_patch_weight
    g = torch.Generator().manual_seed(1)
    D, p, S = 32, 14, 28
    w = torch.randn(D, 3, p, p, generator=g) * 0.05
    packed, bias = pack_patch_weight(w, dtype=torch.float64)
    assert packed.shape == (D, 800) and packed[:, 784:].abs().max() == 0
    assert packed[:, :784].reshape(D, p, p, 4)[..., 3].abs().max() == 0      # the X column
    u8 = torch.randint(0, 256, (2, S, S, 3), generator=g, dtype=torch.uint8)
    ref = torch.nn.functional.conv2d(R.normalise(u8.numpy()).double(), w.double(), stride=p).flatten(2).transpose(1, 2)
    x = torch.cat([u8, torch.randint(0, 256, (2, S, S, 1), generator=g, dtype=torch.uint8)], dim=-1).double()  # junk X byte
    patches = x.reshape(2, S // p, p, S // p, p, 4).permute(0, 1, 3, 2, 4, 5).reshape(2, (S // p) ** 2, 4 * p * p)
    got = patches @ packed[:, :784].t() + bias.double()
    assert (got - ref).abs().max().item() < 1e-5 * ref.abs().max().item()


# ------------------------------------------------------------------------------------------------------------------ CLI host logic
def _args(tmp_path, *extra):
    import eval_dreambooth as E
    return E.build_parser().parse_args([str(tmp_path / "runs" / "db-sd15-n1"), "--outdir", str(tmp_path / "bench"), *extra])


def test_cli_paths():
    import eval_dreambooth as E
    a = E.build_parser().parse_args(["out/textboost-sd15-n1/", "--outdir", "bench/", "--skip-gen"])
    assert E.image_root(a) == os.path.join("bench", "textboost-sd15-n1")
    assert E.csv_path(a) == os.path.join("out/textboost-sd15-n1", "metric_last.csv")
    a = E.build_parser().parse_args(["out/run", "--checkpoint", "500", "--output-desc", "v2", "--skip-gen"])
    assert E.image_root(a) == os.path.join("./benchmarks", "run-500_v2")
    assert E.csv_path(a) == os.path.join("out/run", "metric_ckpt500_v2.csv")
    assert a.metric == ["clip-t", "clip-i", "vqa"] and a.seeds == [0, 1, 2, 3]   # the reference's defaults
    assert a.train_dir == "./data/dreambooth_n1_train" and a.val_dir == "./data/dreambooth_n1_val"


def test_cli_refusals(tmp_path):
    import eval_dreambooth as E
    cm = ["--clip-model", str(tmp_path)]
    with pytest.raises(SystemExit, match="--skip-gen"):
        E.check_args(_args(tmp_path, "--metric", "clip-t", *cm))
    with pytest.raises(SystemExit, match="pass --metric clip-t clip-i"):
        E.check_args(_args(tmp_path, "--skip-gen", *cm))                  # the default --metric names vqa
    with pytest.raises(SystemExit, match="dino"):
        E.check_args(_args(tmp_path, "--skip-gen", "--metric", "clip-i", "dino", *cm))
    with pytest.raises(SystemExit, match="--clip-model"):
        E.check_args(_args(tmp_path, "--skip-gen", "--metric", "clip-t"))
    E.check_args(_args(tmp_path, "--skip-gen", "--metric", "clip-t", "clip-i", *cm))
    # an instance without real images
    seed = tmp_path / "bench" / "db-sd15-n1" / "seed0"
    for inst in ("dog", "can"):
        (seed / inst).mkdir(parents=True)
        (seed / inst / "a_dog.png").write_bytes(b"")
    (tmp_path / "train" / "dog").mkdir(parents=True)
    (tmp_path / "train" / "dog" / "00.jpg").write_bytes(b"")
    a = _args(tmp_path, "--skip-gen", "--metric", "clip-i", "--seeds", "0", "--train-dir", str(tmp_path / "train"),
              "--val-dir", str(tmp_path / "val"), *cm)
    with pytest.raises(SystemExit, match="instance 'can' in --train-dir"):
        E.evaluate(a, evaluator=object())
    with pytest.raises(SystemExit, match="does not exist"):
        E.evaluate(_args(tmp_path, "--skip-gen", "--metric", "clip-t", "--seeds", "7", *cm), evaluator=object())


class _FakeEvaluator:
    """embeddings chosen per file name: the CLI's bookkeeping under test, not the tower"""
    batch_size, tower_images = 32, 0

    class geo:
        image_size = 336

    def __init__(self, table):
        self.table = table

    def encode_images(self, paths, clip_i):
        return torch.stack([self.table[("i" if clip_i else "t", os.path.basename(p))] for p in paths])

    def encode_texts(self, texts):
        return torch.stack([self.table[("txt", t)] for t in texts])

    def images_per_second(self):
        return 0.0


def test_cli_metric_means_and_csv(tmp_path):
    import eval_dreambooth as E
    g = torch.Generator().manual_seed(4)
    table = {}
    gen = {}
    for s in (0, 1):
        for inst in ("dog", "can"):
            d = tmp_path / "bench" / "db-sd15-n1" / f"seed{s}" / inst
            d.mkdir(parents=True)
            for k in range(3):
                name = f"s{s}_a_{inst}_{k}.png"
                (d / name).write_bytes(b"")
                for kind in ("i", "t"):
                    table[(kind, name)] = torch.randn(8, generator=g)
                table[("txt", name[:-4].replace("_", " "))] = torch.randn(8, generator=g)
                gen.setdefault(s, {}).setdefault(inst, []).append(name)
    real = {}
    for split, n in (("train", 1), ("val", 2)):
        for inst in ("dog", "can"):
            d = tmp_path / split / inst
            d.mkdir(parents=True)
            for k in range(n):
                name = f"{split}_{inst}_{k}.jpg"
                (d / name).write_bytes(b"")
                table[("i", name)] = torch.randn(8, generator=g)
                real.setdefault(split, {}).setdefault(inst, []).append(name)
    run = tmp_path / "runs" / "db-sd15-n1"
    run.mkdir(parents=True)
    a = _args(tmp_path, "--skip-gen", "--metric", "clip-t", "clip-i", "--seeds", "0", "1", "--train-dir", str(tmp_path / "train"),
              "--val-dir", str(tmp_path / "val"), "--clip-model", str(tmp_path))
    res = E.evaluate(a, evaluator=_FakeEvaluator(table))
    rows = list(csv.reader(open(run / "metric_last.csv")))
    assert rows[0] == ["seed", "clip_score", "vqa_score", "clip_i", "clip_i_unseen", "dino", "dino_unseen"]
    for s, row in zip((0, 1), rows[1:]):
        names = [n for inst in sorted(gen[s]) for n in gen[s][inst]]
        ct = R.clip_t(torch.stack([table[("t", n)] for n in names]), torch.stack([table[("txt", R.prompt_of(n))] for n in names]))
        ge = {inst: torch.stack([table[("i", n)] for n in gen[s][inst]]) for inst in gen[s]}
        ci = R.clip_i(ge, {inst: torch.stack([table[("i", n)] for n in real["train"][inst]]) for inst in ge})
        cu = R.clip_i(ge, {inst: torch.stack([table[("i", n)] for n in real["val"][inst]]) for inst in ge})
        assert ci.numel() == 2 * 3 * 1 and cu.numel() == 2 * 3 * 2 and (ci >= 0).all()
        assert torch.allclose(res[s]["clip_score"], ct, atol=1e-6)
        assert abs(res[s]["clip_i"].mean() - ci.mean()) < 1e-6 and abs(res[s]["clip_i_unseen"].mean() - cu.mean()) < 1e-6
        assert row == [str(s), f"{ct.mean():.3f}", "0.000", f"{ci.mean():.3f}", f"{cu.mean():.3f}", "0.000", "0.000"]


def test_clip_i_clamps_negative_cosines():
    from textboost_amd.clip_score import clip_i_scores
    gen = torch.tensor([[1.0, 0.0], [0.0, 1.0], [-1.0, 0.0]])
    real = torch.tensor([[2.0, 0.0], [-3.0, 0.0]])
    s = clip_i_scores(gen, real)
    assert torch.allclose(s, torch.tensor([1.0, 0.0, 0.0, 0.0, 0.0, 1.0]))
    ref = R.clip_i({"x": gen}, {"x": real})
    assert torch.allclose(s, ref)


def test_golden_fixture_restates(golden_dir):
    """tests/golden/clip_vit_tiny.pt against the restatement and live Pillow: its digests are Pillow's bytes, its embeddings the model's."""
    PIL = pytest.importorskip("PIL")  # noqa: F841
    import hashlib
    fx = torch.load(os.path.join(golden_dir, "clip_vit_tiny.pt"), weights_only=False)
    cfg, sd = fx["config"], {k: v.float() for k, v in fx["state_dict_fp16"].items()}
    digest = lambda a: f"{a.shape[0]}x{a.shape[1]}x{a.shape[2]}:" + hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    for name in ("clip_i_224", "clip_t_224", "clip_i_336", "clip_t_336"):
        kind, size = name.rsplit("_", 1)
        pre = [R.pil_preprocess(a.numpy(), int(size), kind == "clip_i") for a in fx["images"]]
        assert [digest(p) for p in pre] == fx["preprocessed_sha256"][name], name
        if size == "224":
            with torch.no_grad():
                got = R.image_embeds(sd, cfg, R.normalise(np.stack(pre)))
            assert ((got - fx["image_embeds"][name]).norm() / fx["image_embeds"][name].norm()).item() < 1e-5, name
    with torch.no_grad():
        te = R.text_embeds(sd, cfg, fx["input_ids"])
    assert ((te - fx["text_embeds"]).norm() / fx["text_embeds"].norm()).item() < 1e-5
