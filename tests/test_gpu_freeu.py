"""FreeU on the GPU: tb_freeu against the float64 restatement of tests/freeu_ref.py under a bound derived from the
kernel's arithmetic (both builds, both backbone modes, N(0, 1) data and data offset by +8), its bit identities, repeats and refusals; the
tiny UNet with FreeU against the hooked oracle; a captured 4-step denoise; the command line.

Measured on an MI355X: worst |kernel - float64| / bound between 0.499 and 0.999 over all kernel cases; the tiny UNet's prediction is
1.1e-3 .. 1.2e-3 (rel-L2) from the hooked oracle while FreeU moves it by 7.1e-2 .. 8.6e-2."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import freeu_ref as R
from parity import parity

pytestmark = pytest.mark.gpu
dev = "cuda"
TB_EINVAL = -22
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 4096            # canary elements in front of and behind the operand
PAD = 5                 # columns between hc + sc and the row stride (odd: rows start at odd element offsets)
CANARY = 12345.0
UNET_FACTORS = (1.5, 1.6, 0.9, 0.2)      # tests/test_freeu_host.py holds the hooked oracle to its margin with these


def _bits(t):
    return t.contiguous().view(torch.int16)


def _operand(rows16, pad=PAD):
    """rows16 [M, C] on the host -> (flat device buffer full of canaries, its [M, C] view with row stride C + pad)"""
    M, C = rows16.shape
    ld = C + pad
    flat = torch.full((2 * GUARD + M * ld,), CANARY, dtype=rows16.dtype, device=dev)
    view = flat[GUARD:GUARD + M * ld].view(M, ld)[:, :C]
    view.copy_(rows16.to(dev))
    return flat, view


def _outside_untouched(flat, view, before):
    """canaries in front, behind and in the padding columns carry their bits"""
    M, C = view.shape
    ld = view.stride(0)
    a, b = _bits(flat), _bits(before)
    mid_a, mid_b = a[GUARD:GUARD + M * ld].view(M, ld), b[GUARD:GUARD + M * ld].view(M, ld)
    return torch.equal(a[:GUARD], b[:GUARD]) and torch.equal(a[GUARD + M * ld:], b[GUARD + M * ld:]) and torch.equal(mid_a[:, C:], mid_b[:, C:])


@pytest.fixture(scope="module")
def references():
    """float64 references per (shape, offset, dtype, mode), computed once"""
    cache = {}

    def get(shape, offset, dtype, mode):
        key = (shape, offset, dtype, mode)
        if key not in cache:
            B, H, W, hc, sc = shape
            dkey = (shape, offset, dtype, "rows")
            if dkey not in cache:
                cache[dkey] = R.kernel_rows(B, H, W, hc, sc, offset, seed=1 + R.SHAPES.index(shape), dtype=dtype)
            r16, r64 = cache[dkey]
            b, s = R.f32(R.B_S[0]), R.f32(R.B_S[1])
            ref = R.reference_rows(r64, B, H, W, hc, b, s, mode)
            half = "fp16" if dtype == torch.float16 else "bf16"
            cache[key] = (r16, r64, ref, R.bound_rows(r64, ref, B, H, W, hc, b, s, mode, half))
        return cache[key]
    return get


@pytest.mark.parametrize("half", ["fp16", "bf16"])
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("offset", [0.0, 8.0], ids=["n01", "plus8"])
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_matches_float64_within_the_derived_bound(shape, offset, mode, half, references):
    from textboost_amd import _lib as L
    from textboost_amd import ops
    B, H, W, hc, sc = shape
    with L.use_half(half):
        r16, r64, ref, bound = references(shape, offset, L.half_dtype(), mode)
        flat, view = _operand(r16)
        before = flat.clone()
        ops.freeu(view, B, H, W, hc, R.B_S[0], R.B_S[1], mode)
        torch.cuda.synchronize()
        got = view.double().cpu()
        err = (got - ref).abs()
        ratio = (err / bound).max().item()
        print(f"[freeu] {half} {mode} {shape} offset {offset:g}: worst |kernel - float64| {err.max().item():.3e}, worst error / bound {ratio:.3f}")
        assert torch.isfinite(got).all() and ratio <= 1.0
        assert _outside_untouched(flat, view, before)
        assert torch.equal(_bits(view[:, hc // 2:hc]), _bits(r16[:, hc // 2:hc].to(dev)))      # the untouched half of the hidden part
        one_pixel = mode == "structure" and H * W == 1                                        # a one-pixel map is constant: n = 0, nothing moves
        assert torch.equal(_bits(view[:, :hc // 2]), _bits(r16[:, :hc // 2].to(dev))) == one_pixel
        assert not torch.equal(_bits(view[:, hc:]), _bits(r16[:, hc:].to(dev)))
        flat2, view2 = _operand(r16)                                                          # a repeat: the same bits
        ops.freeu(view2, B, H, W, hc, R.B_S[0], R.B_S[1], mode)
        assert torch.equal(_bits(flat2), _bits(flat))


@pytest.mark.parametrize("half", ["fp16", "bf16"])
@pytest.mark.parametrize("mode", R.MODES)
def test_kernel_bit_identities(mode, half):
    from textboost_amd import _lib as L
    from textboost_amd import ops
    B, H, W, hc, sc = R.SHAPES[1]
    with L.use_half(half):
        r16, _ = R.kernel_rows(B, H, W, hc, sc, 8.0, seed=21, dtype=L.half_dtype())
        x = r16.to(dev)
        flat, view = _operand(r16)
        before = flat.clone()
        ops.freeu(view, B, H, W, hc, 1.0, 1.0, mode)
        assert torch.equal(_bits(flat), _bits(before))
        ops.freeu(view, B, H, W, hc, 1.0, 0.2, mode)                                            # b = 1: the hidden part keeps its bits
        assert torch.equal(_bits(view[:, :hc]), _bits(x[:, :hc])) and not torch.equal(_bits(view[:, hc:]), _bits(x[:, hc:]))
        assert _outside_untouched(flat, view, before)
        flat, view = _operand(r16)
        ops.freeu(view, B, H, W, hc, 1.5, 1.0, mode)                                            # s = 1: the skip part keeps its bits
        assert torch.equal(_bits(view[:, hc // 2:]), _bits(x[:, hc // 2:])) and not torch.equal(_bits(view[:, :hc // 2]), _bits(x[:, :hc // 2]))
        assert _outside_untouched(flat, view, before)
        # a constant channel-mean map (every pixel the same row): the structure backbone leaves it alone, the scalar one does not
        const = r16[:1].repeat(B * H * W, 1)
        flat, view = _operand(const)
        ops.freeu(view, B, H, W, hc, 1.5, 1.0, mode)
        assert torch.equal(_bits(view), _bits(const.to(dev))) == (mode == "structure")


def test_kernel_refusals_touch_nothing():
    from textboost_amd import _lib as L
    B, H, W, hc, sc = 2, 4, 4, 16, 8
    r16, _ = R.kernel_rows(B, H, W, hc, sc, 0.0, seed=5, dtype=torch.float16)
    with L.use_half("fp16"):
        flat, view = _operand(r16)
        before = flat.clone()
        ld = view.stride(0)
        ok = dict(x=L.ptr(view), ld=ld, B=B, H=H, W=W, hc=hc, sc=sc, b=1.5, s=0.2, mode=0)
        bad = [dict(x=None), dict(B=0), dict(B=-1), dict(H=0), dict(W=0), dict(W=-3), dict(hc=0), dict(hc=-2), dict(hc=15, sc=9), dict(sc=0),
               dict(sc=-8), dict(ld=hc + sc - 1), dict(ld=0), dict(b=float("nan")), dict(b=float("inf")), dict(s=float("nan")),
               dict(s=float("-inf")), dict(mode=2), dict(mode=-1),
               dict(B=65536), dict(H=257, W=1), dict(H=1, W=257), dict(H=128, W=64), dict(hc=(1 << 20) + 2, ld=1 << 22),
               dict(sc=(1 << 20) + 1, ld=1 << 22)]
        for change in bad:
            a = dict(ok, **change)
            rc = L.lib().tb_freeu(a["x"], a["ld"], a["B"], a["H"], a["W"], a["hc"], a["sc"], a["b"], a["s"], a["mode"], L.stream())
            assert rc == TB_EINVAL, (change, rc)
        torch.cuda.synchronize()
        assert torch.equal(_bits(flat), _bits(before))
        # the cap admits a 768-pixel model's stage-1 concat (24 x 24 x (1280 + 1280)) and a 64 x 64 map
        big = torch.zeros(24 * 24, 2560, dtype=torch.float16, device=dev)
        assert L.lib().tb_freeu(L.ptr(big), 2560, 1, 24, 24, 1280, 1280, 1.5, 0.2, 1, L.stream()) == 0
        assert L.lib().tb_freeu(L.ptr(big), 64, 1, 64, 64, 2, 2, 1.5, 0.2, 1, L.stream()) == 0
        torch.cuda.synchronize()
        assert not big.any()


# ------------------------------------------------------------------------------------------------------------------ the tiny UNet
def _tiny(sd2):
    from tests.test_gpu_model import make_unet
    ref, hip, cfg = make_unet(2, 16, 64, sd2=sd2)
    return ref, hip


@pytest.mark.parametrize("sd2", [False, True], ids=["sd1", "sd2"])
def test_unet_forward_with_freeu_matches_the_hooked_oracle(sd2):
    from excite_ref import unet_inputs
    B, D = 2, 64
    ref, hip = _tiny(sd2)
    x, t, ehs = unet_inputs(sd2=sd2)
    args = (x.half().to(dev), t.to(dev), ehs.half().view(B * 77, D).to(dev).contiguous())
    with torch.no_grad():
        plain_ref = ref(x, t, ehs)
        plain = hip.forward(*args).clone()
        for mode in R.MODES:
            hs = R.install_hooks(ref, *UNET_FACTORS, mode=mode)
            want = ref(x, t, ehs)
            for h in hs:
                h.remove()
            fu = hip.enable_freeu(*UNET_FACTORS, mode=mode)
            assert fu.b == (1.5, 1.6) and fu.s == (0.9, 0.2) and fu.mode == mode
            got = hip.forward(*args).clone()
            assert hip._saved["freeu"] is True
            parity(f"tiny UNet pred with FreeU ({mode}, sd2={sd2})", got, want, rel=3e-3, maxabs=4e-3, ch_dim=1, ch_rel=4e-3)
            moved = ((got.float().cpu() - plain_ref).norm() / plain_ref.norm()).item()
            print(f"[freeu] tiny UNet sd2={sd2} {mode}: FreeU moves the prediction by rel-L2 {moved:.3e}")
            assert moved >= 10 * 3e-3
            assert torch.equal(hip.forward(*args), got)                      # a repeat: the same bits
            hip.enable_freeu(1, 1, 1, 1, mode=mode)
            assert torch.equal(hip.forward(*args), plain)                    # (1, 1, 1, 1): the plain forward's bits
            hip.enable_freeu(*UNET_FACTORS, mode=mode)
            hip.disable_freeu()
            assert hip.freeu is None and torch.equal(hip.forward(*args), plain) and hip._saved["freeu"] is False


def test_freeu_forward_keeps_nothing_for_a_backward():
    from excite_ref import unet_inputs
    from tests.test_gpu_model import make_unet
    from textboost_amd.unet import HipUNet, UNetGeometry
    B, D = 2, 64
    ref, hip, cfg = make_unet(B, 16, D)
    x, t, ehs = unet_inputs()
    args = (x.half().to(dev), t.to(dev), ehs.half().view(B * 77, D).to(dev).contiguous())
    dpred = torch.randn(B, 4, 16, 16, generator=torch.Generator().manual_seed(2)).to(dev)
    hip.forward(*args)
    d0 = hip.backward(dpred).clone()
    for bad in (dict(mode="mean"), dict(b1=0.0), dict(s2=float("nan")), dict(b2=float("inf")), dict(s1=-1.0)):
        kw = dict(dict(b1=1.5, b2=1.6, s1=0.9, s2=0.2), **bad)
        with pytest.raises(ValueError):
            hip.enable_freeu(**kw)
    assert hip.freeu is None
    hip.enable_excite()
    hip.enable_freeu(*UNET_FACTORS)
    with pytest.raises(ValueError, match="FreeU"):
        hip.forward(*args, until="excite")
    hip.forward(*args)
    with pytest.raises(ValueError, match="FreeU"):
        hip.backward(dpred)
    with pytest.raises(ValueError, match="FreeU"):
        hip.backward_sample(dpred)
    with pytest.raises(ValueError, match="FreeU"):
        hip.backward_sample()
    hip.disable_freeu()
    hip.forward(*args)
    assert torch.equal(hip.backward(dpred), d0)                              # off again: the backward is what it was
    hip.forward(*args, until="excite")
    geo1 = UNetGeometry(block_out_channels=(64,), num_heads=(2,), cross_attention_dim=D, cross_attn_levels=(True,))
    geo = UNetGeometry(block_out_channels=cfg.block_out_channels, num_heads=cfg.num_heads, cross_attention_dim=D,
                       cross_attn_levels=cfg.cross_attn_levels)
    with pytest.raises(NotImplementedError, match="16-bit"):
        HipUNet(geo, ref.state_dict(), B, 16, 16, device=dev, dtype=torch.float32).enable_freeu(*UNET_FACTORS)
    one = HipUNet.__new__(HipUNet)                                            # a one-level geometry: no second up block to re-weight
    one.geo, one.dtype = geo1, torch.float16
    with pytest.raises(ValueError, match="fewer than two up blocks"):
        one.enable_freeu(*UNET_FACTORS)


# ------------------------------------------------------------------------------------------------------------------ sampler, command line
@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    from tests import test_gpu_sweep as TS
    from tests.test_compose_host import write_run
    from tests.test_gpu_generate import D_TEXT
    from textboost_amd import generate as G
    root = tmp_path_factory.mktemp("freeu")
    mdir = TS._prepare(str(root))
    da = str(root / "runs" / "dog")
    write_run(da, ["<dog>"], ["<hflip>"], seed=1, rank=4, keep_rows="even")
    B = 2
    with torch.no_grad():
        pipe = G.Pipeline.from_model_dir(mdir, B, steps=4, guidance=7.5, device=dev)
    g = torch.Generator().manual_seed(3)
    cond = torch.randn(B * 77, D_TEXT, generator=g).half().float().to(dev)
    uncond = torch.randn(77, D_TEXT, generator=g).half().float().repeat(B, 1).to(dev)
    lat = torch.cat([G.seeded_latent(s, 16) for s in (0, 1)]).to(dev)
    return dict(root=root, mdir=mdir, da=da, pipe=pipe, cond=cond, uncond=uncond, lat=lat)


@pytest.mark.parametrize("mode", R.MODES)
def test_captured_denoise_with_freeu_replays_bit_identically(tiny, mode):
    pipe = tiny["pipe"]
    args = (tiny["cond"], tiny["uncond"])
    with torch.no_grad():
        plain = pipe.sampler.denoise(*args, latents=tiny["lat"]).clone()
        pipe.unet.enable_freeu(*UNET_FACTORS, mode=mode)
        try:
            eager = pipe.sampler.denoise(*args, latents=tiny["lat"]).clone()      # also the warm-up: every buffer exists
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, capture_error_mode="thread_local"):       # every launch goes to the one capturing stream: a chain
                out = pipe.sampler.denoise(*args, latents=tiny["lat"])
            replays = []
            for _ in range(2):
                out.fill_(float("nan"))
                graph.replay()
                torch.cuda.synchronize()
                replays.append(out.clone())
        finally:
            pipe.unet.disable_freeu()
        assert torch.isfinite(eager).all() and not torch.equal(eager, plain)
        assert torch.equal(replays[0], eager) and torch.equal(replays[1], eager)
        assert torch.equal(pipe.sampler.denoise(*args, latents=tiny["lat"]), plain)     # nothing is left behind


def _cli(tiny, name, extra, ok=True):
    wd = str(tiny["root"] / "cli")
    os.makedirs(wd, exist_ok=True)
    cmd = [tiny["da"], "--model", tiny["mdir"], "--prompt", "photo of a <dog> dog", "--seeds", "0", "1", "--steps", "4", "--output", name] + extra
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, os.path.join(ROOT, "inference.py")] + cmd, capture_output=True, text=True,
                       cwd=wd)
    assert (r.returncode == 0) == ok, r.stdout[-3000:] + r.stderr[-3000:]
    return r, os.path.join(wd, name)


def test_cli_freeu_images(tiny):
    pytest.importorskip("transformers")
    from PIL import Image
    _, plain = _cli(tiny, "plain.png", [])
    r, a = _cli(tiny, "a.png", ["--freeu", "1.5", "1.6", "0.9", "0.2"])
    assert "FreeU b1 1.5 b2 1.6 s1 0.9 s2 0.2 (scalar backbone)" in r.stdout
    _, b = _cli(tiny, "b.png", ["--freeu", "1.5", "1.6", "0.9", "0.2"])
    _, one = _cli(tiny, "one.png", ["--freeu", "1", "1", "1", "1"])
    r, s = _cli(tiny, "s.png", ["--freeu", "1.5", "1.6", "0.9", "0.2", "--freeu-backbone", "structure"])
    assert "(structure backbone)" in r.stdout
    read = lambda p: open(p, "rb").read()
    assert read(a) == read(b) and read(one) == read(plain)
    assert np.asarray(Image.open(a)).shape == (128, 2 * 128, 3)
    assert read(a) != read(plain) and read(s) != read(plain) and read(s) != read(a)
    assert not np.array_equal(np.asarray(Image.open(a)), np.asarray(Image.open(plain)))


@pytest.mark.parametrize("extra, why", [
    (["--freeu", "1.5", "1.6", "0.9"], "expected zero or four values"),
    (["--freeu", "1.5", "1.6", "0", "0.2"], "S1 = 0.0: finite and > 0"),
    (["--freeu-backbone", "structure"], "--freeu-backbone needs --freeu"),
    (["--freeu", "1", "1", "1", "1", "--excite", "<dog>"], "--freeu does not go with --excite"),
    (["--freeu"], "no published factors for a UNet with cross_attention_dim"),
], ids=["count", "zero", "backbone-alone", "excite", "family"])
def test_cli_refusals_build_no_model(tiny, extra, why):
    r, out = _cli(tiny, "refused.png", extra, ok=False)
    assert why in r.stderr and not os.path.exists(out)
    assert "FreeU b1" not in r.stdout and "Traceback" not in r.stderr
