"""Regional prompts on the GPU: the kernel (csrc/region_attn.hip) against the float64 reference of tests/region_attn_ref.py, the `HipUNet.regions`
hook, `HipSampler.denoise(regions=...)`, and `inference.py --region`.

Bounds (none of them derived from this kernel's output): O rel-L2 <= 2e-3 in fp16 -- the bound of test_attention_fwd_short_key_kernel
(tests/test_gpu_norm_attn.py) -- and <= 1.2e-2 in bf16 -- the attention-forward bound of tests/test_gpu_bf16.py (P is rounded to bf16 before P V);
LSE within 2e-3 of max(|LSE|, 1), as those tests measure it.  The reference is evaluated on the rounded operands."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import region_attn_ref as R

pytestmark = pytest.mark.gpu
dev = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TB_EINVAL = -22
O_BOUND = {"fp16": 2e-3, "bf16": 1.2e-2}
LSE_BOUND = 2e-3

CASES = [(2, 8, 64, 77, 40), (2, 5, 100, 77, 64), (1, 8, 36, 77, 160), (2, 2, 64, 33, 80), (2, 2, 96, 128, 64), (1, 1, 1, 1, 8)]


def _operands(B, H, Sq, Skv, hd, seed, dtype):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(B * n, H * hd, generator=g).to(dtype) for n in (Sq, Skv, Skv))


def _tables(B, Sq, Skv, regions, seed):
    """random tables: every query is inside each region with probability 1 / 2; key 0 is unrestricted (no query loses all its keys), every other
    key is unrestricted or in one of `regions` with equal probability.  -> (key_region int32 [B, Skv], query_regions uint32 [Sq])"""
    rng = np.random.default_rng(seed)
    qb = np.zeros(Sq, dtype=np.uint32)
    for r in regions:
        qb |= (rng.random(Sq) < 0.5).astype(np.uint32) << np.uint32(r)
    kr = np.asarray([-1] + list(regions), dtype=np.int32)[rng.integers(0, len(regions) + 1, (B, Skv))]
    kr[:, 0] = -1
    return kr, qb


def _dev_tables(kr, qb):
    return torch.from_numpy(kr).to(dev), torch.from_numpy(qb.view(np.int32).copy()).to(dev)


def _lse_err(lse, ref):
    return ((lse.double() - ref).abs() / ref.abs().clamp_min(1.0)).max().item()


def _launch(Q, K, V, B, H, Sq, Skv, hd, kr, qb, scale=None):
    from textboost_amd import ops
    o = torch.full((B * Sq, H * hd), float("nan"), device=dev, dtype=Q.dtype)
    lse = torch.full((B, H, Sq), float("nan"), device=dev)
    krd, qbd = _dev_tables(kr, qb)
    ops.attention_region_fwd(Q.to(dev), K.to(dev), V.to(dev), o, lse, B, H, Sq, Skv, hd, krd, qbd, scale=scale)
    return o.cpu(), lse.cpu()


@pytest.mark.parametrize("half", ["fp16", "bf16"])
@pytest.mark.parametrize("regions", [(0, 1, 2), (30, 31)], ids=["regions0-2", "regions30-31"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_kernel_matches_the_float64_reference(case, regions, half):
    from textboost_amd import _lib as L
    B, H, Sq, Skv, hd = case
    with L.use_half(half):
        Q, K, V = _operands(B, H, Sq, Skv, hd, 7, L.half_dtype())
        kr, qb = _tables(B, Sq, Skv, regions, 8)
        scale = hd ** -0.5
        oref, lref, P = R.ref_region_attention(Q, K, V, B, H, Sq, Skv, hd, scale, kr, qb)
        o, lse = _launch(Q, K, V, B, H, Sq, Skv, hd, kr, qb, scale)
        o2, lse2 = _launch(Q, K, V, B, H, Sq, Skv, hd, kr, qb, scale)
    err, lerr = R.rel_l2(o, oref), _lse_err(lse, lref)
    masked = 1.0 - R.allowed(kr, qb).double().mean().item()
    print(f"[regions] {half} {case} regions {regions}: O rel-L2 {err:.3e} (bound {O_BOUND[half]:.1e}), LSE {lerr:.3e} (bound {LSE_BOUND:.1e}), "
          f"{100 * masked:.0f} % of the (query, key) pairs masked")
    assert torch.isfinite(o.float()).all() and torch.isfinite(lse).all()
    assert err <= O_BOUND[half], (err, O_BOUND[half])
    assert lerr <= LSE_BOUND, lerr
    assert torch.equal(o, o2) and torch.equal(lse, lse2)                      # a repeat launch, bit for bit


@pytest.mark.parametrize("half", ["fp16", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_all_keys_unrestricted_agrees_with_the_flash_forward(case, half):
    from textboost_amd import _lib as L
    from textboost_amd import ops
    B, H, Sq, Skv, hd = case
    with L.use_half(half):
        Q, K, V = _operands(B, H, Sq, Skv, hd, 9, L.half_dtype())
        kr = np.full((B, Skv), -1, dtype=np.int32)
        qb = np.zeros(Sq, dtype=np.uint32)                                    # no query in any region: nothing looks at the bits
        o, lse = _launch(Q, K, V, B, H, Sq, Skv, hd, kr, qb)
        of = torch.empty(B * Sq, H * hd, device=dev, dtype=Q.dtype)
        lf = torch.empty(B, H, Sq, device=dev)
        ops.attention_fwd(Q.to(dev), K.to(dev), V.to(dev), of, lf, B, H, Sq, Skv, hd)
        of, lf = of.cpu(), lf.cpu()
    oref, lref = R.ref_attention(Q, K, V, B, H, Sq, Skv, hd, hd ** -0.5)
    err, ferr, both = R.rel_l2(o, oref), R.rel_l2(of, oref), R.rel_l2(o, of)
    print(f"[regions] {half} {case} unrestricted: region kernel {err:.3e}, flash forward {ferr:.3e} against float64; against each other {both:.3e}")
    assert err <= O_BOUND[half] and both <= O_BOUND[half]
    assert _lse_err(lse, lref) <= LSE_BOUND and _lse_err(lse, lf.double()) <= LSE_BOUND


@pytest.mark.parametrize("half", ["fp16", "bf16"])
def test_strided_unaligned_operands_and_canaries(half):
    """K / V are column slices of one wide buffer, Q and O have leading dimensions that leave their rows off 16-byte alignment (the 2-byte
    load / store instance); the columns around O keep their contents"""
    from textboost_amd import _lib as L
    from textboost_amd import ops
    B, H, Sq, Skv, hd = 2, 2, 100, 77, 40
    C = H * hd
    with L.use_half(half):
        dt = L.half_dtype()
        Q, K, V = _operands(B, H, Sq, Skv, hd, 11, dt)
        kr, qb = _tables(B, Sq, Skv, (0, 1, 31), 12)
        qbuf = torch.full((B * Sq, C + 4), 50.0, dtype=dt)
        kvbuf = torch.full((B * Skv, 3 * C + 2), 50.0, dtype=dt)
        qbuf[:, :C], kvbuf[:, 1:C + 1], kvbuf[:, 2 * C:3 * C] = Q, K, V
        qd, kvd = qbuf.to(dev), kvbuf.to(dev)
        obuf = torch.full((B * Sq, C + 6), -7.0, device=dev, dtype=dt)
        o = obuf[:, 3:C + 3]
        lse = torch.empty(B, H, Sq, device=dev)
        krd, qbd = _dev_tables(kr, qb)
        ops.attention_region_fwd(qd[:, :C], kvd[:, 1:C + 1], kvd[:, 2 * C:3 * C], o, lse, B, H, Sq, Skv, hd, krd, qbd)
        host = obuf.cpu()
        aligned, _ = _launch(Q, K, V, B, H, Sq, Skv, hd, kr, qb)
    assert (host[:, :3] == -7.0).all() and (host[:, C + 3:] == -7.0).all()
    oref, lref, _ = R.ref_region_attention(Q, K, V, B, H, Sq, Skv, hd, hd ** -0.5, kr, qb)
    err = R.rel_l2(host[:, 3:C + 3], oref)
    print(f"[regions] {half} strided, unaligned: O rel-L2 {err:.3e}")
    assert err <= O_BOUND[half] and _lse_err(lse.cpu(), lref) <= LSE_BOUND
    assert torch.equal(host[:, 3:C + 3], aligned)                              # the two instances do the same arithmetic


@pytest.mark.parametrize("half", ["fp16", "bf16"])
def test_locality_bit_for_bit(half):
    """the K and V rows of one restricted key change: every output row whose query lies outside that key's region keeps its bits"""
    from textboost_amd import _lib as L
    B, H, Sq, Skv, hd = 2, 5, 100, 77, 64
    b, j = 1, 40
    with L.use_half(half):
        Q, K, V = _operands(B, H, Sq, Skv, hd, 13, L.half_dtype())
        kr, qb = _tables(B, Sq, Skv, (0, 1, 2), 14)
        kr[b, j] = 2
        o, lse = _launch(Q, K, V, B, H, Sq, Skv, hd, kr, qb)
        K2, V2 = K.clone(), V.clone()
        K2[b * Skv + j] = (K[b * Skv + j].float() * -1.5 + 0.25).to(K.dtype)
        V2[b * Skv + j] = (V[b * Skv + j].float() + 3.0).to(V.dtype)
        o2, lse2 = _launch(Q, K2, V2, B, H, Sq, Skv, hd, kr, qb)
    inside = torch.from_numpy(((qb >> np.uint32(2)) & 1).astype(bool))
    assert 10 < int(inside.sum()) < Sq - 10
    o, o2 = o.view(B, Sq, -1), o2.view(B, Sq, -1)
    assert torch.equal(o[0], o2[0]) and torch.equal(lse[0], lse2[0])                       # the other batch row
    assert torch.equal(o[b][~inside], o2[b][~inside]) and torch.equal(lse[b][:, ~inside], lse2[b][:, ~inside])
    changed = (o[b][inside] != o2[b][inside]).any(dim=1)
    print(f"[regions] {half} locality: {int(changed.sum())} of {int(inside.sum())} rows inside the region changed, 0 of {int((~inside).sum())} outside")
    assert changed.any()


@pytest.mark.parametrize("half", ["fp16", "bf16"])
def test_a_query_outside_every_region_with_every_key_restricted(half):
    from textboost_amd import _lib as L
    B, H, Sq, Skv, hd = 2, 5, 100, 77, 64
    b, s = 1, 70                                                   # in the third wave of the first 128-query block (one tile per wave here)
    with L.use_half(half):
        Q, K, V = _operands(B, H, Sq, Skv, hd, 15, L.half_dtype())
        kr, qb = _tables(B, Sq, Skv, (0, 1, 2), 16)
        kr[b] = np.random.default_rng(17).integers(0, 3, Skv)      # batch row 1: no unrestricted key
        qb |= 1                                                    # every other query keeps region 0's keys
        qb[s] = 0
        o, lse = _launch(Q, K, V, B, H, Sq, Skv, hd, kr, qb)
        qb_in = qb.copy()
        qb_in[s] = 1
        o_in, lse_in = _launch(Q, K, V, B, H, Sq, Skv, hd, kr, qb_in)
    oref, lref, _ = R.ref_region_attention(Q, K, V, B, H, Sq, Skv, hd, hd ** -0.5, kr, qb)
    assert not torch.isnan(o.float()).any() and not torch.isnan(lse).any()
    ov = o.view(B, Sq, -1)
    assert (ov[b, s] == 0).all() and (lse[b, :, s] == -float("inf")).all()
    assert torch.isfinite(ov[0, s].float()).all() and torch.isfinite(lse[0, :, s]).all() and (ov[0, s] != 0).any()      # batch row 0 has key 0
    keep = torch.ones(B, Sq, dtype=torch.bool)
    keep[:, s] = False                                                                      # (the query's bits are shared by the batch rows)
    assert torch.equal(ov[keep], o_in.view(B, Sq, -1)[keep])                                # the other rows: the same bits
    assert torch.equal(lse.transpose(1, 2)[keep], lse_in.transpose(1, 2)[keep])
    assert R.rel_l2(o, oref) <= O_BOUND[half]
    fin = torch.isfinite(lref)
    assert int((~fin).sum()) == H and _lse_err(lse[fin], lref[fin]) <= LSE_BOUND


# ------------------------------------------------------------------------------------------------ several query tiles per wave, remapped blocks
def _dispatch(B, H, Sq):
    """(query tiles per wave, blocks remapped over the XCDs) of tb_attention_region_fwd's launch rule, restated from csrc/region_attn.hip: a
    workgroup takes 512 / 256 queries while that leaves >= 512 workgroups, else 128; blocks are remapped when (query bands * B) % 8 == 0"""
    qt = 4
    while qt > 1 and -(-Sq // (128 * qt)) * B * H < 512:
        qt //= 2
    return qt, (-(-Sq // (128 * qt)) * B) % 8 == 0


# (B, H, Sq, Skv, hd), tiles per wave, remap: the shapes a real generation launches (SD1.x 64^2 maps at batch >= 4) walk several tiles per
# wave -- the prefetch of the next tile's Q fragments and region bits, the per-tile O / LSE rows -- and run remapped; every Sq is ragged
MULTI = [((8, 8, 1900, 77, 40), 2, True), ((16, 8, 1900, 77, 8), 4, True), ((9, 8, 2100, 33, 80), 2, False), ((8, 2, 200, 77, 8), 1, True)]


@pytest.mark.parametrize("half", ["fp16", "bf16"])
@pytest.mark.parametrize("case,qtiles,remap", MULTI, ids=lambda c: "x".join(map(str, c)) if isinstance(c, tuple) else str(c))
def test_multi_tile_and_remapped_launches_match_the_float64_reference(case, qtiles, remap, half):
    from textboost_amd import _lib as L
    B, H, Sq, Skv, hd = case
    assert _dispatch(B, H, Sq) == (qtiles, remap)
    assert Sq % (128 * qtiles) != 0 and Sq % 32 != 0                         # a ragged last block and a ragged last tile
    with L.use_half(half):
        Q, K, V = _operands(B, H, Sq, Skv, hd, 21, L.half_dtype())
        kr, qb = _tables(B, Sq, Skv, (0, 1, 31), 22)
        scale = hd ** -0.5
        oref, lref, _ = R.ref_region_attention(Q, K, V, B, H, Sq, Skv, hd, scale, kr, qb)
        o, lse = _launch(Q, K, V, B, H, Sq, Skv, hd, kr, qb, scale)
        o2, lse2 = _launch(Q, K, V, B, H, Sq, Skv, hd, kr, qb, scale)
    err, lerr = R.rel_l2(o, oref), _lse_err(lse, lref)
    # per 128-query slice of the sequence (one tile of each of a workgroup's four waves): a fault in one tile index must not hide in the sum.
    # The bound is the whole output's: the error is per-element rounding of the same operands everywhere, so a slice of >= 9000 elements has
    # the same relative error as the whole, and a slice computed from the wrong tile's bits or rows is off by order 1.
    C = H * hd
    worst = max(R.rel_l2(o.view(B, Sq, C)[:, s0:s0 + 128], oref.view(B, Sq, C)[:, s0:s0 + 128]) for s0 in range(0, Sq, 128))
    print(f"[regions] {half} {case} ({qtiles} tiles per wave, remap {int(remap)}): O rel-L2 {err:.3e}, worst 128-query slice {worst:.3e} "
          f"(bound {O_BOUND[half]:.1e}), LSE {lerr:.3e}")
    assert torch.isfinite(o.float()).all() and torch.isfinite(lse).all()
    assert err <= O_BOUND[half] and worst <= O_BOUND[half], (err, worst)
    assert lerr <= LSE_BOUND, lerr
    assert torch.equal(o, o2) and torch.equal(lse, lse2)


@pytest.mark.parametrize("half", ["fp16", "bf16"])
def test_masks_follow_the_query_in_a_later_tile_of_a_multi_tile_workgroup(half):
    """two tiles per wave: query 200 is tile 1 of wave 2 of the first workgroup (query 72 is the same lane's tile 0).  With every key of one
    batch row restricted and query 200 outside all regions, exactly that row is O = 0 / LSE = -inf; a restricted key's K / V rows change only
    the rows whose query lies inside its region"""
    from textboost_amd import _lib as L
    B, H, Sq, Skv, hd = 8, 8, 1900, 77, 40
    assert _dispatch(B, H, Sq) == (2, True)
    b, s, j = 3, 200, 40
    with L.use_half(half):
        Q, K, V = _operands(B, H, Sq, Skv, hd, 23, L.half_dtype())
        kr, qb = _tables(B, Sq, Skv, (0, 1, 2), 24)
        kr[b] = np.random.default_rng(25).integers(0, 3, Skv)      # batch row 3: no unrestricted key
        kr[b, j] = 2
        qb |= 1
        qb[s] = 0
        o, lse = _launch(Q, K, V, B, H, Sq, Skv, hd, kr, qb)
        qb_in = qb.copy()
        qb_in[s] = 1
        o_in, lse_in = _launch(Q, K, V, B, H, Sq, Skv, hd, kr, qb_in)
        K2, V2 = K.clone(), V.clone()
        K2[b * Skv + j] = (K[b * Skv + j].float() * -1.5 + 0.25).to(K.dtype)
        V2[b * Skv + j] = (V[b * Skv + j].float() + 3.0).to(V.dtype)
        o_p, lse_p = _launch(Q, K2, V2, B, H, Sq, Skv, hd, kr, qb)
    assert not torch.isnan(o.float()).any() and not torch.isnan(lse).any()
    ov, ovi, ovp = o.view(B, Sq, -1), o_in.view(B, Sq, -1), o_p.view(B, Sq, -1)
    dead = (ov == 0).all(dim=2)
    assert dead[b, s] and int(dead.sum()) == 1 and (lse[b, :, s] == -float("inf")).all() and int(torch.isinf(lse).sum()) == H
    assert (ovi[b, s] != 0).any() and torch.isfinite(lse_in).all()
    keep = torch.ones(B, Sq, dtype=torch.bool)
    keep[:, s] = False                                             # (the query's bits are shared by the batch rows)
    assert torch.equal(ov[keep], ovi[keep]) and torch.equal(lse.transpose(1, 2)[keep], lse_in.transpose(1, 2)[keep])
    inside = torch.from_numpy(((qb >> np.uint32(2)) & 1).astype(bool))
    others = torch.ones(B, dtype=torch.bool)
    others[b] = False
    assert torch.equal(ov[others], ovp[others]) and torch.equal(ov[b][~inside], ovp[b][~inside])
    assert torch.equal(lse[others], lse_p[others]) and torch.equal(lse[b][:, ~inside], lse_p[b][:, ~inside])
    changed = (ov[b][inside] != ovp[b][inside]).any(dim=1)
    tile1 = inside & ((torch.arange(Sq) % 256) >= 128)
    print(f"[regions] {half} multi-tile: {int(changed.sum())} of {int(inside.sum())} rows inside the region changed ({int(tile1.sum())} of them in "
          f"a second tile), 0 of {int((~inside).sum())} outside")
    assert changed.any() and (ov[b][tile1] != ovp[b][tile1]).any()


def test_refusals_return_minus_22_and_leave_o_untouched():
    from textboost_amd import _lib as L
    from textboost_amd import ops

    def call(H=2, Sq=16, Skv=8, hd=16, dtype=torch.float16, causal=0, kr_value=-1, null=None, ldq_short=False):
        C = H * hd
        q = torch.zeros(Sq, C, device=dev, dtype=dtype)
        k = torch.zeros(max(Skv, 1), C, device=dev, dtype=dtype)
        o = torch.full((Sq, C), 5.0, device=dev, dtype=dtype)
        lse = torch.full((1, H, Sq), 5.0, device=dev)
        kr = torch.full((1, max(Skv, 1)), -1, device=dev, dtype=torch.int32)
        kr[0, -1] = kr_value
        qb = torch.zeros(Sq, device=dev, dtype=torch.int32)
        d = ops._attn_desc(q, k, k, o, lse, 1, H, Sq, Skv, hd, hd ** -0.5, causal)
        if ldq_short:
            d.ldq = C - 8
        rc = L.lib().tb_attention_region_fwd(d, ops._dt(q), None if null == "key_region" else L.ptr(kr), None if null == "query_regions" else L.ptr(qb),
                                             L.stream())
        torch.cuda.synchronize()
        return rc, o, lse
    with L.use_half("fp16"):
        for kw in (dict(kr_value=32), dict(kr_value=33), dict(kr_value=2 ** 31 - 1), dict(null="key_region"), dict(null="query_regions"),
                   dict(dtype=torch.float32), dict(causal=1), dict(Skv=129), dict(Skv=0), dict(hd=44), dict(hd=168), dict(hd=4), dict(ldq_short=True)):
            rc, o, lse = call(**kw)
            assert rc == TB_EINVAL, (kw, rc)
            assert (o == 5.0).all() and (lse == 5.0).all(), kw
        for kw in (dict(), dict(kr_value=31), dict(kr_value=-5)):
            rc, o, lse = call(**kw)
            assert rc == 0 and (o == 0).all(), kw                   # zero operands: V = 0
        with pytest.raises(RuntimeError, match="tb_attention_region_fwd"):
            z = torch.zeros(16, 32, device=dev)
            ops.attention_region_fwd(z, z[:8], z[:8], torch.empty_like(z), None, 1, 2, 16, 8, 16, torch.full((1, 8), -1, device=dev, dtype=torch.int32),
                                     torch.zeros(16, device=dev, dtype=torch.int32))


# ------------------------------------------------------------------------------------------------ UNet level
def _halves(h, w, positions=((2, 3, 4), (6, 9))):
    """two regions: the left half and the right half of the latent grid"""
    from textboost_amd.regions import Region, box_cells
    return [Region(("left",), tuple(positions[0]), box_cells((0, 0, 0.5, 1), h, w)), Region(("right",), tuple(positions[1]), box_cells((0.5, 0, 1, 1), h, w))]


def test_unet_hook_every_cross_attention_matches_the_reference_and_leaves_no_state():
    from tests.test_gpu_model import make_unet
    from textboost_amd.attn_maps import cross_attention_maps
    from textboost_amd.regions import RegionSet
    B, hw, D = 2, 16, 64
    _, hip, _ = make_unet(B, hw, D)
    _, fresh, _ = make_unet(B, hw, D)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, 4, hw, hw, generator=g).half().to(dev)
    t = torch.tensor([17, 801], device=dev)
    ehs = torch.randn(B * 77, D, generator=g).half().to(dev)
    assert hip.regions is None
    want = fresh.forward(x, t, ehs).clone()
    plain = hip.forward(x, t, ehs).clone()
    assert torch.equal(plain, want)                                  # regions = None: a fresh UNet's prediction, bit for bit
    rset = RegionSet.for_unet(hip, _halves(hw, hw))
    assert sorted(rset.tables) == sorted(cross_attention_maps(hip)) and tuple(rset.key_region.shape) == (B, 77)
    assert (rset.key_region[0] == -1).all() and rset.key_region[1].tolist()[:10] == [-1, -1, 0, 0, 0, -1, 1, -1, -1, 1]
    hip.regions = rset
    try:
        pred = hip.forward(x, t, ehs).clone()
    finally:
        hip.regions = None
    assert torch.isfinite(pred).all() and not torch.equal(pred, plain)
    nl = len(hip.geo.block_out_channels)
    kv_all = hip.kv_all.cpu()
    kr = rset.key_region.cpu().numpy()
    for name, C in hip.xattn:
        block = name[:-len(".transformer_blocks.0.attn2")]
        part = block.split(".")
        level = nl - 1 if part[0] == "mid_block" else (int(part[1]) if part[0] == "down_blocks" else nl - 1 - int(part[1]))
        lhw = (hip.H >> level, hip.W >> level)
        heads = hip.geo.heads(level)
        hd = C // heads
        q2 = hip._bufs[block + ".q2"].cpu()
        ko = hip.kv_off[name]
        oref, lref, _ = R.ref_region_attention(q2, kv_all[:, ko:ko + C], kv_all[:, ko + C:ko + 2 * C], B, heads, lhw[0] * lhw[1], hip.T, hd, hd ** -0.5,
                                               kr, rset.table(lhw).cpu().numpy())
        err = R.rel_l2(hip._bufs[block + ".o2"].cpu(), oref)
        lerr = _lse_err(hip._bufs[block + ".lse2"].cpu().view(B, heads, -1), lref)
        print(f"[regions] tiny UNet {block} ({lhw[0]}x{lhw[1]}, {heads} heads of {hd}): o2 rel-L2 {err:.3e}, lse2 {lerr:.3e}")
        assert err <= O_BOUND["fp16"] and lerr <= LSE_BOUND, (block, err, lerr)
    again = hip.forward(x, t, ehs)
    assert torch.equal(again, plain)                                 # set and unset: no state left behind


# ------------------------------------------------------------------------------------------------ sampler level
@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    from safetensors.torch import load_file, save_file
    from tests.test_compose_host import write_run
    from tests.test_gpu_generate import D_TEXT, write_model_dir
    from textboost_amd import generate as G
    from textboost_amd import models
    from textboost_amd.regions import RegionSet
    from textboost_amd.vae import VAEGeometry, vae_encoder_shapes
    root = tmp_path_factory.mktemp("regions")
    mdir, da, db = str(root / "model"), str(root / "runs" / "dog"), str(root / "runs" / "cat")
    write_model_dir(mdir, hw=16)
    vfile = os.path.join(mdir, "vae", "diffusion_pytorch_model.safetensors")      # --init-image encodes the photo: the VAE file gets an encoder half
    vgeo = VAEGeometry(block_out_channels=(64, 64, 128, 128), layers_per_block=1)
    enc_sd = {k: v.half().float() for k, v in models.random_state_dict(vae_encoder_shapes(vgeo), 15, device="cpu").items()}
    save_file({**load_file(vfile), **enc_sd}, vfile)
    write_run(da, ["<dog>"], ["<hflip>"], seed=1, rank=4, keep_rows="even")
    write_run(db, ["<cat>"], ["<hflip>"], seed=2, rank=4, keep_rows="odd")
    B = 2
    with torch.no_grad():
        pipe = G.Pipeline.from_model_dir(mdir, B, steps=3, guidance=7.5, device=dev)
    g = torch.Generator().manual_seed(3)
    cond = torch.randn(B * 77, D_TEXT, generator=g).half().float().to(dev)
    uncond = torch.randn(B * 77, D_TEXT, generator=g).half().float().to(dev)
    lat = torch.cat([G.seeded_latent(s, 16) for s in (0, 1)]).to(dev)
    rset = RegionSet.for_unet(pipe.unet, _halves(16, 16))
    return dict(root=root, mdir=mdir, da=da, db=db, pipe=pipe, B=B, cond=cond, uncond=uncond, lat=lat, rset=rset)


def test_sampler_region_steps(tiny):
    from textboost_amd.sampler import HipSampler
    pipe, rset = tiny["pipe"], tiny["rset"]
    args = (tiny["cond"], tiny["uncond"])
    with torch.no_grad():
        plain = pipe.sampler.denoise(*args, latents=tiny["lat"]).clone()
        for bad in (0, 4):
            with pytest.raises(ValueError, match="region_steps"):
                pipe.sampler.denoise(*args, latents=tiny["lat"], regions=rset, region_steps=bad)
        with pytest.raises(ValueError, match="region_steps without regions"):
            pipe.sampler.denoise(*args, latents=tiny["lat"], region_steps=2)
        assert torch.equal(pipe.sampler.denoise(*args, latents=tiny["lat"]), plain)            # a refusal leaves nothing behind
        full = pipe.sampler.denoise(*args, latents=tiny["lat"], regions=rset).clone()
        assert pipe.unet.regions is None
        at_n = pipe.sampler.denoise(*args, latents=tiny["lat"], regions=rset, region_steps=3).clone()
        one = pipe.sampler.denoise(*args, latents=tiny["lat"], regions=rset, region_steps=1).clone()
        assert torch.equal(at_n, full)                                                         # all steps is the default
        assert torch.isfinite(full).all() and not torch.equal(full, plain) and not torch.equal(one, plain) and not torch.equal(one, full)
        assert torch.equal(pipe.sampler.denoise(*args, latents=tiny["lat"]), plain) and pipe.unet.regions is None
        # the image-editing loop counts executed steps: strength 0.67 of 3 steps runs steps 1 and 2
        z0 = torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(5)).to(dev)
        e_plain = pipe.sampler.denoise_from(*args, z0, tiny["lat"], 0.67).clone()
        e_full = pipe.sampler.denoise_from(*args, z0, tiny["lat"], 0.67, regions=rset).clone()
        e_two = pipe.sampler.denoise_from(*args, z0, tiny["lat"], 0.67, regions=rset, region_steps=2).clone()
        with pytest.raises(ValueError, match="region_steps 3"):
            pipe.sampler.denoise_from(*args, z0, tiny["lat"], 0.67, regions=rset, region_steps=3)
        assert torch.equal(e_two, e_full) and not torch.equal(e_full, e_plain) and torch.isfinite(e_full).all()
        # the ancestral scheduler
        ddpm = HipSampler(pipe.unet, pipe.vae, steps=2, guidance=7.5, scheduler="DDPMScheduler")
        noise = [torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(6 + i)).to(dev) for i in range(2)]
        d_plain = ddpm.denoise(*args, latents=tiny["lat"], step_noise=noise).clone()
        d_reg = ddpm.denoise(*args, latents=tiny["lat"], step_noise=noise, regions=rset).clone()
        assert torch.isfinite(d_reg).all() and not torch.equal(d_reg, d_plain) and pipe.unet.regions is None


def test_captured_denoise_with_regions_replays_bit_identically(tiny):
    from textboost_amd.sampler import HipSampler
    pipe, rset = tiny["pipe"], tiny["rset"]
    with torch.no_grad():
        two = HipSampler(pipe.unet, pipe.vae, steps=2, guidance=7.5)
        eager = two.denoise(tiny["cond"], tiny["uncond"], latents=tiny["lat"], regions=rset).clone()      # also the warm-up: every buffer exists
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):       # every launch goes to the one capturing stream: a chain
            out = two.denoise(tiny["cond"], tiny["uncond"], latents=tiny["lat"], regions=rset)
        replays = []
        for _ in range(2):
            out.fill_(float("nan"))
            graph.replay()
            torch.cuda.synchronize()
            replays.append(out.clone())
    assert torch.equal(replays[0], eager) and torch.equal(replays[1], eager)


# ------------------------------------------------------------------------------------------------ the CLI
PROMPT = "a <dog> dog and a <cat> cat"


def _child(cmd, cwd):
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, os.path.join(ROOT, "inference.py")] + cmd, capture_output=True, text=True, cwd=cwd)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def test_cli_regions_change_the_image_and_repeat_byte_for_byte(tiny):
    pytest.importorskip("transformers")
    from PIL import Image
    from textboost_amd import regions as G
    common = [tiny["da"], "--model", tiny["mdir"], "--prompt", PROMPT, "--seeds", "0", "1", "--steps", "2", "--output", "g.png"]
    regs = ["--region", "<dog> dog=0,0,0.5,1", "--region", "cat=0.5,0,1,1"]
    wds = {}
    for name, extra in (("plain", []), ("plain2", []), ("regions", regs), ("regions2", regs)):
        wds[name] = str(tiny["root"] / name)
        os.makedirs(wds[name])
        out = _child(common + extra, wds[name])
        assert ("_regions.png" in out) == bool(extra)
    g = {k: _read(os.path.join(v, "g.png")) for k, v in wds.items()}
    assert g["plain"] == g["plain2"] and not os.path.exists(os.path.join(wds["plain"], "g_regions.png"))
    assert g["regions"] == g["regions2"] and g["regions"] != g["plain"]
    d = np.abs(np.asarray(Image.open(os.path.join(wds["regions"], "g.png"))).astype(int) - np.asarray(Image.open(os.path.join(wds["plain"], "g.png"))).astype(int))
    print(f"[regions] inference.py: with two regions vs without, mean |delta| {d.mean():.2f} levels, max {d.max()}")
    assert Image.open(os.path.join(wds["regions"], "g.png")).size == (2 * 128, 128)
    prev = np.asarray(Image.open(os.path.join(wds["regions"], "g_regions.png")).convert("RGB"))
    assert prev.shape == (128, 128, 3) and (prev[:, :64] == G.COLOURS[0]).all() and (prev[:, 64:] == G.COLOURS[1]).all()
    assert _read(os.path.join(wds["regions"], "g_regions.png")) == _read(os.path.join(wds["regions2"], "g_regions.png"))


def test_cli_regions_with_composed_runs_and_with_an_init_image(tiny):
    pytest.importorskip("transformers")
    from PIL import Image
    from tests.test_gpu_edit import _photo
    wd = str(tiny["root"] / "more")
    os.makedirs(wd)
    photo, maskf = os.path.join(wd, "photo.png"), os.path.join(wd, "right.png")
    Image.fromarray(_photo()).save(photo)
    m = np.zeros((20, 20), dtype=np.uint8)
    m[:, 10:] = 255
    Image.fromarray(m).save(maskf)
    base = ["--model", tiny["mdir"], "--prompt", PROMPT, "--seeds", "0", "1", "--steps", "2"]
    regs = ["--region", "<dog> dog=0,0,0.5,1", "--region", f"<cat> cat=@{maskf}"]
    _child([tiny["da"], "--with", tiny["db"]] + base + ["--output", "w0.png"], wd)
    out = _child([tiny["da"], "--with", tiny["db"]] + base + ["--output", "w1.png"] + regs, wd)
    assert "w1_regions.png" in out and "128 of 256 latent cells" in out
    assert _read(os.path.join(wd, "w1.png")) != _read(os.path.join(wd, "w0.png"))
    assert Image.open(os.path.join(wd, "w1_regions.png")).size == (128, 128)
    edit = [tiny["da"]] + base + ["--init-image", photo, "--strength", "1.0"]
    _child(edit + ["--output", "e0.png"], wd)
    _child(edit + ["--output", "e1.png", "--region", "<dog> dog=0,0,0.5,1", "--region", f"cat=@{maskf}", "--region-steps", "0.5"], wd)
    assert _read(os.path.join(wd, "e1.png")) != _read(os.path.join(wd, "e0.png"))
    assert Image.open(os.path.join(wd, "e1.png")).size == (2 * 128, 128) and os.path.exists(os.path.join(wd, "e1_regions.png"))
