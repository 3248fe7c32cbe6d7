"""GPU tests of the DINO score: tb_gemm's col_scale epilogue (LayerScale) against float64 in both builds, its refusals, the device
preprocessing against Pillow's bytes, the tower against the fp32 restatement (tiny and full-size ViT-L/14), and eval_dreambooth.py end to end."""
import csv
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dino_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gamma(n, g):
    """LayerScale-like column scales: half the columns from [1e-5, 1e-3], half from [0.05, 1]"""
    small = torch.rand(n, generator=g) < 0.5
    return torch.where(small, 1e-5 + torch.rand(n, generator=g) * 1e-3, 0.05 + torch.rand(n, generator=g) * 0.95)


# M = B * 257 token rows of the tower (B = 2 / 32); (8192, 640, 640) and (2048, 1280, 5120) take gemm8 tiles, the latter split over K;
# (514, 1024, 4096) splits K on the 4-wave kernel; (300, 1001, 256): N % 8 != 0, so the last unit of each row is partial (the masked bias /
# scale / residual loads and the scalar stores of epilogue8)
SHAPES = [(514, 1024, 1024), (514, 1024, 4096), (8224, 1024, 4096), (8192, 640, 640), (2048, 1280, 5120), (300, 1001, 256)]


def _case(M, N, K, r, c, seed):
    from textboost_amd import _lib as L
    hd = L.half_dtype()
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(M, K, generator=g).to(hd).cuda()
    W = (torch.randn(N, K, generator=g) / K ** 0.5).to(hd).cuda()
    bias = (0.5 * torch.randn(N, generator=g)).cuda()
    cs = _gamma(N, g).cuda()
    R_ = None if r is None else torch.randn(M, N, generator=g).to(torch.float32 if r == "f32" else hd).cuda()
    out = lambda: torch.full((M, N), float("nan"), device="cuda", dtype=torch.float32 if c == "f32" else hd)   # noqa: E731
    return A, W, bias, cs, R_, out


def _launch(A, W, out, bias, R_, cs):
    from textboost_amd import _lib as L, ops
    ops.gemm(A, W, out, bias=bias, R=R_, col_scale=cs)
    cfg, c8 = (ctypes.c_int * 5)(), (ctypes.c_int * 6)()
    L.lib().tb_gemm_last_config(cfg)
    return list(cfg), bool(L.lib().tb_gemm8_last(c8))


@pytest.mark.parametrize("half", ["fp16", "bf16"])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_col_scale_against_float64(M, N, K, half):
    from textboost_amd import _lib as L
    with L.use_half(half):
        hd = L.half_dtype()
        ulp = {torch.float16: 2.0 ** -10, torch.bfloat16: 2.0 ** -7}[hd]
        for i, (r, c) in enumerate([("f32", "f32"), (None, "f32"), ("f16", "f16"), (None, "f16"), ("f16", "f32")]):
            A, W, bias, cs, R_, mk = _case(M, N, K, r, c, 100 * i + M % 97)
            out = mk()
            cfg, took8 = _launch(A, W, out, bias, R_, cs)
            torch.cuda.synchronize()
            if (M, N, K) == (514, 1024, 4096):
                assert cfg[4] > 1, f"not split over K: {cfg}"
            if (M, N, K) in ((8192, 640, 640), (2048, 1280, 5120)):
                assert took8, "did not take a gemm8 tile"
            branch = A.double() @ W.double().t() + bias.double()
            Rd = R_.double() if R_ is not None else torch.zeros_like(branch)
            ref = cs.double() * branch + Rd
            rms = branch.pow(2).mean(dim=0).sqrt()
            # fp32 accumulation of K products (a branch-sized error, scaled by cs), rounding of the sum with an unscaled R, the output's rounding
            tol = cs.double() * 1e-4 * rms + 1e-6 * Rd.abs() + (ulp if c == "f16" else 1e-6) * ref.abs() + (6e-8 if c == "f16" else 0.0)
            err = (out.double() - ref).abs()
            worst = (err / tol).max().item()
            assert torch.isfinite(out).all() and worst <= 1.0, (half, (M, N, K), r, c, worst)


@pytest.mark.parametrize("half", ["fp16", "bf16"])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_col_scale_of_ones_is_bit_equal_to_none(M, N, K, half):
    from textboost_amd import _lib as L, ops
    with L.use_half(half):
        for i, (r, c) in enumerate([("f32", "f32"), ("f16", "f16"), (None, "f16")]):
            A, W, bias, cs, R_, mk = _case(M, N, K, r, c, 7 + i)
            a, b = mk(), mk()
            ops.gemm(A, W, a, bias=bias, R=R_)
            ops.gemm(A, W, b, bias=bias, R=R_, col_scale=torch.ones_like(cs))
            torch.cuda.synchronize()
            assert torch.equal(a, b), (half, (M, N, K), r, c, (a.float() - b.float()).abs().max().item())


def test_col_scale_refusals():
    """every combination outside the plain Linear epilogue returns -22 instead of ignoring the field"""
    from textboost_amd import _lib as L, ops
    hd = L.half_dtype()
    M, N, K = 128, 320, 320
    A = torch.randn(M, K, device="cuda").to(hd)
    W = torch.randn(N, K, device="cuda").to(hd)
    C = torch.zeros(M, N, device="cuda").to(hd)
    C2 = torch.zeros(M, N, device="cuda").to(hd)
    cs = torch.ones(N, device="cuda")
    stats = torch.zeros(M, 16, 2, device="cuda")
    rb = torch.zeros(1, N, device="cuda")
    split = ctypes.c_int32(1)

    def desc(**kw):
        d = L.GemmDesc()
        d.M, d.N, d.K, d.K1 = M, N, K, K
        d.A, d.lda, d.W, d.ldw, d.C, d.ldc, d.c_dtype = L.ptr(A), K, L.ptr(W), K, L.ptr(C), N, L.TB_F16
        d.a_mode, d.alpha, d.col_scale = L.A_LINEAR, 1.0, L.ptr(cs)
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    cases = {"gelu": desc(act=L.ACT_GELU), "quick_gelu": desc(act=L.ACT_QUICK_GELU), "silu": desc(act=L.ACT_SILU),
             "geglu": desc(act=L.ACT_GEGLU), "ln_fwd": desc(act=L.ACT_LN_FWD, C2=L.ptr(C2), ldc2=N),
             "gelu_c2": desc(act=L.ACT_GELU, C2=L.ptr(C2), ldc2=N), "c2": desc(C2=L.ptr(C2), ldc2=N),
             "rowbias": desc(rowbias=L.ptr(rb), rows_per_group=M, ldrb=N), "rs_out": desc(rs_out=L.ptr(stats), rs_ld=16),
             "rs_in": desc(rs_in=L.ptr(stats), rs_ld=16, rs_n=1, ln_gamma=L.ptr(cs)), "split_out": desc(split_out=ctypes.pointer(split))}
    x = torch.zeros(1, 8, 8, 64, device="cuda").to(hd)
    w9 = torch.zeros(64, 9 * 64, device="cuda").to(hd)
    c64 = torch.zeros(64, 64, device="cuda").to(hd)
    cases["conv3x3"] = desc(M=64, N=64, K=576, K1=576, A=L.ptr(x), lda=64, W=L.ptr(w9), ldw=576, C=L.ptr(c64), ldc=64, a_mode=L.A_CONV3X3,
                            B=1, Hin=8, Win=8, Cin=64, Hout=8, Wout=8, stride=1, sign=1)
    for name, d in cases.items():
        assert L.lib().tb_gemm(d, L.stream()) == -22, name
    # the fp32 mode's kernels (csrc/f32_path.hip) never take it
    A32, W32, C32 = torch.zeros(M, K, device="cuda"), torch.zeros(N, K, device="cuda"), torch.zeros(M, N, device="cuda")
    d = desc(A=L.ptr(A32), W=L.ptr(W32), C=L.ptr(C32), c_dtype=L.TB_F32)
    assert L.lib().tb_gemm_f32(d, L.stream()) == -22
    assert L.lib().tb_gemm_f32_t(d, 0, 0, L.stream()) == -22
    with pytest.raises(RuntimeError):
        ops.gemm(A32, W32, C32, col_scale=cs)
    torch.cuda.synchronize()
    assert float(C.float().abs().sum()) == 0.0   # nothing was launched


# ------------------------------------------------------------------------------------------------------------------ preprocessing
def _images(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(11)
    paths = []
    for k, (h, w, ext) in enumerate([(300, 217, "jpg"), (413, 640, "png"), (512, 512, "png"), (180, 97, "jpg"), (224, 224, "png")]):
        y, x = np.mgrid[0:h, 0:w]
        a = np.clip(rng.integers(30, 220, 3) + 70 * np.sin(x / rng.uniform(4, 19))[..., None] + rng.normal(0, 18, (h, w, 3)) +
                    0.2 * y[..., None], 0, 255).astype(np.uint8)
        p = str(tmp_path / f"{k:02d}.{ext}")
        Image.fromarray(a).save(p, **({"quality": 90} if ext == "jpg" else {}))
        paths.append(p)
    return paths


def test_preprocessing_matches_pillow(tmp_path):
    from PIL import Image
    from textboost_amd import augment
    from textboost_amd.clip_score import load_rgb
    from textboost_amd.dino_score import preprocess
    for p in _images(tmp_path):
        got = augment.to_host_rgb(preprocess(augment.to_device_image(load_rgb(p))).contiguous())
        want = R.pil_preprocess(np.asarray(Image.open(p).convert("RGB")))
        assert got.shape == (224, 224, 3) and np.array_equal(got, want), (p, int(np.abs(got.astype(int) - want).max()))


# ------------------------------------------------------------------------------------------------------------------ the tower
def _rgbx(u8):
    x = torch.as_tensor(np.asarray(u8)).to(torch.int32)
    return (x[..., 0] | (x[..., 1] << 8) | (x[..., 2] << 16)).cuda().contiguous()


def _random_hub_state(geo, seed):
    from textboost_amd import models
    from textboost_amd.dino_score import hub_state_shapes
    sd = models.random_state_dict(hub_state_shapes(geo), seed)
    g = torch.Generator().manual_seed(seed + 1)
    sd["cls_token"] = 0.02 * torch.randn(sd["cls_token"].shape, generator=g)
    sd["pos_embed"] = 0.02 * torch.randn(sd["pos_embed"].shape, generator=g)
    for k in sd:
        if k.endswith(".gamma"):
            sd[k] = _gamma(sd[k].numel(), g)
        elif k.endswith(".bias") and "norm" not in k:
            sd[k] = 0.02 * torch.randn(sd[k].shape, generator=g)
    return sd


def _tower_vs_restatement(geo, sd, B, seed):
    from textboost_amd.dino_score import HipDINOv2
    g = torch.Generator().manual_seed(seed)
    u8 = torch.randint(0, 256, (B, 224, 224, 3), generator=g, dtype=torch.uint8)
    got = HipDINOv2(geo, sd).encode(_rgbx(u8)).cpu()
    with torch.no_grad():
        ref = R.features(sd, R.normalise(u8.numpy()), geo.num_heads, geo.eps, geo.interpolate_offset)
    rel = ((got - ref).norm() / ref.norm()).item()
    gn, rn = torch.nn.functional.normalize(got, dim=1), torch.nn.functional.normalize(ref, dim=1)
    dcos = ((gn @ gn.t()) - (rn @ rn.t())).abs().max().item()
    return rel, dcos


@pytest.mark.parametrize("half", ["fp16", "bf16"])
@pytest.mark.parametrize("pos_grid", [16, 7])
def test_tiny_tower_matches_restatement(pos_grid, half):
    from textboost_amd import _lib as L
    from textboost_amd.dino_score import DINOv2Geometry
    geo = DINOv2Geometry(hidden_size=128, intermediate_size=512, num_layers=2, num_heads=2, pos_grid=pos_grid)
    with L.use_half(half):
        rel, dcos = _tower_vs_restatement(geo, _random_hub_state(geo, 21 + pos_grid), 3, 5)
    print(f"[tiny DINOv2 {half} grid {pos_grid}] rel-L2 {rel:.2e}  |dcos| {dcos:.2e}")
    assert rel <= (2e-3 if half == "fp16" else 1.6e-2) and dcos <= (1e-3 if half == "fp16" else 8e-3), (rel, dcos)


def test_full_size_vit_l14():
    from textboost_amd.dino_score import DINOV2_VITL14
    torch.set_num_threads(min(16, torch.get_num_threads()))
    rel, dcos = _tower_vs_restatement(DINOV2_VITL14, _random_hub_state(DINOV2_VITL14, 31), 2, 7)
    print(f"[DINOv2 ViT-L/14 fp16, B=2] CLS rel-L2 {rel:.2e}  pairwise |dcos| {dcos:.2e}")
    assert rel <= 2e-3 and dcos <= 1e-4, (rel, dcos)   # measured 1.64e-3 and 2.0e-5


# recorded from HipDINOv2.encode at the commit before the two towers moved onto vit.HipViT (this geometry, B = 3; the same in fp16 and bf16)
_G = "gemm_kernel<64, 64, 0, 64, 4>"
_BLOCK = ["layernorm_fwd", _G, "attn_fwd_kernel", _G, "layernorm_fwd", _G, _G]   # LN1, qkv, attention, out-proj, LN2, fc1, fc2
TINY_TOWER_LAUNCHES = ["clip_patch_embed_kernel"] + 2 * _BLOCK + ["layernorm_fwd"]


def test_tiny_tower_launch_schedule():
    """the tower's launches, in order, by kernel: patch embedding, per block LN / qkv / attention / proj / LN / fc1 / fc2, the final LayerNorm
    on the CLS rows"""
    from textboost_amd import ops
    from textboost_amd.dino_score import DINOv2Geometry, HipDINOv2
    geo = DINOv2Geometry(hidden_size=128, intermediate_size=512, num_layers=2, num_heads=2, pos_grid=16)
    tower = HipDINOv2(geo, _random_hub_state(geo, 31))
    g = torch.Generator().manual_seed(3)
    x = _rgbx(torch.randint(0, 256, (3, 224, 224, 3), generator=g, dtype=torch.uint8))
    tower.encode(x)
    ops.start_recording()
    tower.encode(x)
    names = [r[0] for r in ops.stop_recording()]
    assert names == TINY_TOWER_LAUNCHES, names


# ------------------------------------------------------------------------------------------------------------------ CLI end to end
def test_cli_end_to_end(tmp_path):
    from PIL import Image
    from safetensors.torch import save_file
    from textboost_amd.dino_score import hub_state_from_transformers, geometry_from_transformers_config
    cfg = {"model_type": "dinov2", "hidden_size": 128, "num_hidden_layers": 2, "num_attention_heads": 2, "mlp_ratio": 4, "hidden_act": "gelu",
           "layer_norm_eps": 1e-6, "image_size": 98, "patch_size": 14, "num_channels": 3, "qkv_bias": True, "use_swiglu_ffn": False}
    geo = geometry_from_transformers_config(cfg)
    hub = _random_hub_state(geo, 41)
    D = 128
    tf = {"embeddings.cls_token": hub["cls_token"], "embeddings.mask_token": torch.zeros(1, D), "embeddings.position_embeddings": hub["pos_embed"],
          "embeddings.patch_embeddings.projection.weight": hub["patch_embed.proj.weight"],
          "embeddings.patch_embeddings.projection.bias": hub["patch_embed.proj.bias"], "layernorm.weight": hub["norm.weight"],
          "layernorm.bias": hub["norm.bias"]}
    for i in range(2):
        t, b = f"encoder.layer.{i}.", f"blocks.{i}."
        for j, n in enumerate(("query", "key", "value")):
            tf[f"{t}attention.attention.{n}.weight"] = hub[b + "attn.qkv.weight"][j * D:(j + 1) * D]
            tf[f"{t}attention.attention.{n}.bias"] = hub[b + "attn.qkv.bias"][j * D:(j + 1) * D]
        tf[t + "attention.output.dense.weight"], tf[t + "attention.output.dense.bias"] = hub[b + "attn.proj.weight"], hub[b + "attn.proj.bias"]
        tf[t + "layer_scale1.lambda1"], tf[t + "layer_scale2.lambda1"] = hub[b + "ls1.gamma"], hub[b + "ls2.gamma"]
        for n in ("norm1", "norm2", "mlp.fc1", "mlp.fc2"):
            tf[t + n + ".weight"], tf[t + n + ".bias"] = hub[b + n + ".weight"], hub[b + n + ".bias"]
    mapped = hub_state_from_transformers(tf, geo)
    assert all(torch.equal(mapped[k], hub[k]) for k in hub)
    mdir = tmp_path / "dinov2"
    mdir.mkdir()
    (mdir / "config.json").write_text(json.dumps(dict(cfg, architectures=["Dinov2Model"])))
    save_file({k: v.contiguous() for k, v in tf.items()}, str(mdir / "model.safetensors"))

    rng = np.random.default_rng(9)

    def img(h, w):
        y, x = np.mgrid[0:h, 0:w]
        c = rng.integers(40, 200, 3)
        return np.clip(c + 60 * np.sin(x / rng.uniform(5, 20))[..., None] + rng.normal(0, 10, (h, w, 3)) + y[..., None] * 0.1, 0,
                       255).astype(np.uint8)
    gen = {}
    for s in (0, 1):
        for inst in ("dog", "can"):
            d = tmp_path / "bench" / "tb-sd15-n1" / f"seed{s}" / inst
            d.mkdir(parents=True)
            for k in range(3):
                p = d / f"a_{inst}_{k}.png"
                Image.fromarray(img(256 + 16 * k, 256)).save(p)
                gen.setdefault(s, {}).setdefault(inst, []).append(str(p))
    real = {}
    for inst, n in (("dog", 3), ("can", 2)):
        d = tmp_path / "db" / inst
        d.mkdir(parents=True)
        for k in range(n):
            p = d / f"{k:02d}.jpg"
            Image.fromarray(img(300 + 40 * k, 217)).save(p, quality=95)
            real.setdefault(inst, []).append(str(p))
    (tmp_path / "runs" / "tb-sd15-n1").mkdir(parents=True)
    # relative paths: the reference takes N from the third '-' field of the whole path
    cmd = [sys.executable, os.path.join(ROOT, "eval_dreambooth.py"), "runs/tb-sd15-n1", "--outdir", "bench", "--skip-gen", "--metric", "dino",
           "--seeds", "0", "1", "--dreambooth-path", "db", "--dino-model", str(mdir), "--batch-size", "4"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "DINO tower" in r.stdout and "images/s" in r.stdout
    rows = list(csv.reader(open(tmp_path / "runs" / "tb-sd15-n1" / "metric_last.csv")))
    assert rows[0] == ["seed", "clip_score", "vqa_score", "clip_i", "clip_i_unseen", "dino", "dino_unseen"]

    def feats(paths):
        u8 = np.stack([R.pil_preprocess(np.asarray(Image.open(p).convert("RGB"))) for p in paths])
        return R.features(hub, R.normalise(u8), 2)
    with torch.no_grad():
        real_f = {i: feats(real[i]) for i in ("dog", "can")}
        for s, row in zip((0, 1), rows[1:]):
            names = [i for i in sorted(gen[s]) for _ in gen[s][i]]
            ws, wu = R.padded_means(feats([p for i in sorted(gen[s]) for p in gen[s][i]]), names, real_f, 1)
            got = [float(v) for v in row[1:]]
            print(f"[e2e] seed {s}: csv {row[1:]}  restatement {ws.mean():.5f} {wu.mean():.5f}")
            assert row[0] == str(s) and got[:4] == [0.0] * 4
            for v, want in ((got[4], ws.mean().item()), (got[5], wu.mean().item())):
                assert abs(v - want) <= 1e-3 + 5e-4, (row, ws.mean(), wu.mean())   # 1e-3 on the means, plus the CSV's %.3f rounding
