"""The flash-attention family (tb_attention_fwd / tb_attention_bwd: csrc/attention.hip, attention_il.hip, attention_small.hip) on PEAKED and
SHIFTED score distributions -- a sink key, a dominant key in the last tile, a dominant diagonal, logits moved by +-32 nats, and heads of very
different statistics side by side in one launch -- on every dispatch path, forward and backward (tests/attn_peaked_ref.py).

Two assertions per output (O, LSE, dQ, dK, dV; rel-L2, max-abs / max|ref|, worst head-dim channel; per head for `mixed`):
  kernel vs MODEL    the float64 operand model makes exactly the roundings the kernel is documented to make, so what remains is summation order,
                     v_exp_f32 and rare rounding flips: the bound is the project's unit-scale tolerance (attn_peaked_ref.TOL), on any data.
  kernel vs float64  max(that tolerance, 4 x model-vs-float64 on the same inputs): the yardstick of tests/test_gpu_f32_split.py.
Each output prints one `[attn-peaked]` line: kernel vs float64 | model vs float64 | kernel vs model.

PATHS names, per dispatch path, which operand carries scale * log2(e) into the score product of the forward, dQ and dK/dV kernels, where delta
comes from, and what the row sum sums -- with the source line of each.  The tables are importable without a GPU: the host test
(test_attn_peaked_host.py) evaluates the cap on the yardstick at every (Sq, Skv, hd, causal) listed here."""
import functools

import pytest
import torch

import attn_peaked_ref as R

pytestmark = pytest.mark.gpu

SEED = 21

# ---- model switches per dispatch path (file:line = where the kernel does it)
#   fwd: scaled_fwd 'q' everywhere (attention.hip:266 attn_fwd_kernel, :512 attn_xs_fwd_kernel, :652 attn_fwd_dma_kernel; attention_il.hip: same
#        arithmetic, attention_il.hip:6).  tile 64 + lazy re-base (attention.hip:358, :801, attention_il.hip:150) except the short-key kernel
#        (exact row maximum, attention.hip:522-540).  The row sum is the all-ones row of V^T -- it sums the ROUNDED P -- whenever the head dim has
#        padding (hd < 32 * ceil(hd / 32): attention.hip:2208-2213, :886-893), else it sums the fp32 P (attention.hip:388); the short-key kernel
#        always sums the fp32 P (attention.hip:539).  fold_m (the reference point kept 16-bit representable): hd = 40 (attention.hip:360, :803).
#   bwd: scaled_dq 'q' (attention.hip:1390 attn_bwd_dq_kernel, :955 attn_bwd_dq_dma_kernel, :1589 attn_xs_bwd_dq_kernel), scaled_dkv 'k'
#        (attention.hip:1675 attn_bwd_dkv_kernel, :1150 attn_bwd_dkv_dma_kernel), delta = rowsum(dO * O) (attention.hip:1394-1410, :1596);
#        the one-launch cross-attention backward scales K for all three outputs (attention.hip:1918) and takes delta = rowsum(P * dP)
#        (attention.hip:1950-1972); attention_small.hip applies the scale in fp32 after the product (attention_small.hip:111) and takes
#        delta = rowsum(dO * O) (attention_small.hip:73-80).
GENERIC_BWD = dict(scaled_dq="q", scaled_dkv="k", delta_from="o")
PATHS = {
    "fwd-generic":    dict(tile=64),
    "fwd-dma":        dict(tile=64),
    "fwd-pipelined":  dict(tile=64),
    "fwd-short-key":  dict(tile=None, rowsum_of="exact"),
    "bwd-generic":    GENERIC_BWD,
    "bwd-dma-dq":     GENERIC_BWD,
    "bwd-dma-dkv":    GENERIC_BWD,
    "bwd-pipelined":  GENERIC_BWD,
    "bwd-short-key":  GENERIC_BWD,
    "bwd-one-launch": dict(scaled_dq="k", scaled_dkv="k", delta_from="pdp"),
    "bwd-small":      dict(scaled_dq=None, scaled_dkv=None, delta_from="o"),
}


def model_cfg(path, hd, fwd_path=None):
    """the model64 switches of `path` at head dim hd.  A backward case runs the DEFAULT forward first (its O and LSE feed the kernels), so its
    forward switches are those of the forward path the shape dispatches to (fwd_path)."""
    cfg = dict(scaled_fwd="q", tile=64, rowsum_of="rounded" if hd % 32 else "exact", fold_m=hd == 40)
    if fwd_path:
        cfg.update(PATHS[fwd_path])
    cfg.update(PATHS[path])
    return cfg


# ---- (path, (B, H, Sq, Skv, hd), causal, variant bits that select the path, bits that switch it off or None, proof)
# proof 'always': the two runs must differ in some bit of O / LSE, which shows that the path ran.  The hd = 80 LDS-DMA kernel and the software-
# pipelined kernel are bit-EQUAL to the kernel behind their off-bit in O and in LSE on every input tried (same arithmetic in the same order,
# attention.hip:578, attention_il.hip:6): no bitwise proof exists for them (None; the comparison is printed), their dispatch is what
# launch_fwd states (attention.hip:2156-2194)
FWD_CASES = [
    ("fwd-generic", (1, 2, 130, 70, 128), False, 1, None, None),
    ("fwd-generic", (2, 4, 64, 64, 160), False, 1, None, None),
    ("fwd-generic", (3, 12, 77, 77, 64), True, 1, None, None),
    ("fwd-dma", (2, 3, 256, 192, 40), False, 1 | 1024, 0, "always"),               # (1024: not the software-pipelined kernel; 0: the register-staged one)
    ("fwd-dma", (2, 3, 256, 320, 80), False, 1 | 2, 1, None),                  # (2: the LDS-DMA kernel also for hd = 80)
    ("fwd-pipelined", (1, 2, 256, 192, 40), False, 1, 1 | 1024, None),
    ("fwd-pipelined", (1, 5, 512, 512, 40), False, 1, 1 | 1024, None),
    ("fwd-short-key", (2, 4, 1024, 50, 40), False, 1, 1 | 16384, "always"),
    ("fwd-short-key", (1, 5, 1152, 77, 64), False, 1, 1 | 16384, "always"),
    ("fwd-short-key", (2, 8, 1024, 77, 80), False, 1, 1 | 16384, "always"),
]
# backward: + the forward path the shape's default forward takes, + ws ('self': 2 B H S floats, 'cross': 16 * 2 * B * Skv * C, None) as
# HipUNet._transformer sizes it, + which outputs must differ bitwise between the two runs
BWD_CASES = [
    ("bwd-generic", (1, 2, 130, 70, 128), False, 1, "no-ws", "fwd-generic", "cross", ("dK", "dV")),     # query-split planes vs one pass
    ("bwd-generic", (2, 8, 200, 77, 40), False, 1, "no-ws", "fwd-generic", "cross", ("dK", "dV")),
    ("bwd-generic", (1, 8, 320, 320, 80), False, 1, None, "fwd-generic", "self", ()),
    ("bwd-dma-dq", (2, 8, 512, 512, 40), False, 1, 1 | 256, "fwd-pipelined", "self", ("dQ",)),
    ("bwd-dma-dq", (1, 5, 512, 512, 64), False, 1, 1 | 256, "fwd-generic", "self", ("dQ",)),
    ("bwd-dma-dq", (2, 8, 512, 512, 80), False, 1, 1 | 256, "fwd-generic", "self", ("dQ",)),
    ("bwd-dma-dkv", (16, 8, 512, 512, 80), False, 1, 1 | 128, "fwd-generic", "self", ("dK", "dV")),
    ("bwd-dma-dkv", (16, 8, 512, 512, 64), False, 1, 1 | 128, "fwd-generic", "self", ("dK", "dV")),
    ("bwd-dma-dkv", (16, 8, 512, 512, 40), False, 1 | 2048, 1 | 2048 | 128, "fwd-pipelined", "self", ("dK", "dV")),
    # the pipelined kernels are bit-equal to the LDS-DMA kernels they replace (same arithmetic, same order), so the run is shown against the
    # register-staged pair (128 | 256); bit-equality with 2048 is asserted on top
    ("bwd-pipelined", (16, 8, 512, 512, 40), False, 1 | 4096, 1 | 128 | 256, "fwd-pipelined", "self", ("dQ", "dK", "dV")),
    ("bwd-short-key", (2, 4, 1024, 50, 40), False, 1 | 65536, 1 | 65536 | 16384, "fwd-short-key", "cross", ("dQ",)),
    ("bwd-one-launch", (2, 8, 256, 77, 40), False, 1, 1 | 65536, "fwd-generic", "cross", ("dQ", "dK", "dV")),
    ("bwd-one-launch", (1, 5, 1152, 77, 64), False, 1 | 131072, 1 | 65536, "fwd-short-key", "cross", ("dQ", "dK", "dV")),
    ("bwd-one-launch", (2, 8, 1024, 77, 80), False, 1 | 131072, 1 | 65536, "fwd-short-key", "cross", ("dQ", "dK", "dV")),
    ("bwd-one-launch", (2, 4, 1024, 50, 40), False, 1, 1 | 65536, "fwd-short-key", "cross", ("dQ", "dK", "dV")),
    ("bwd-small", (3, 12, 77, 77, 64), True, 1, 1 | 8192, "fwd-generic", None, ("dQ", "dK", "dV")),
    ("bwd-small", (2, 4, 33, 33, 64), False, 1, 1 | 8192, "fwd-generic", None, ("dQ", "dK", "dV")),
    ("bwd-small", (2, 4, 96, 96, 64), False, 1, 1 | 8192, "fwd-generic", None, ("dQ", "dK", "dV")),
]

# nats of margin g where the default 8 breaks the cap on the yardstick (fp16 model within 2e-2 of float64 on every metric, 1e-2 on LSE:
# test_attn_peaked_host.py test_cap_on_the_yardstick, over every model configuration the shape is used with): the margin shrinks, the cap stays
MARGIN = {
    ((1, 2, 130, 70, 128), "mixed"): 6.0, ((2, 3, 256, 320, 80), "mixed"): 7.0, ((2, 4, 1024, 50, 40), "mixed"): 7.0,
    ((2, 8, 1024, 77, 80), "mixed"): 6.0, ((1, 8, 320, 320, 80), "mixed"): 7.0, ((2, 8, 512, 512, 80), "mixed"): 7.0,
    ((16, 8, 512, 512, 80), "mixed"): 7.0, ((2, 8, 256, 77, 40), "mixed"): 5.0, ((2, 8, 1024, 77, 80), "late"): 7.0,
    ((2, 4, 1024, 50, 40), "sink"): 7.0, ((2, 4, 1024, 50, 40), "late"): 7.0, ((2, 4, 33, 33, 64), "mixed"): 7.0,
}


def inputs(shape, scenario, B=None, H=None):
    """the case's inputs (the host test takes a B = 1, H <= 5 slice of the same construction)"""
    return R.make_inputs(scenario, B or shape[0], H or shape[1], *shape[2:], SEED, g=MARGIN.get((shape, scenario), 8.0))


def scenarios(shape, causal):
    if causal:
        return ("sink", "late", "shift+")
    return ("sink", "late", "shift-", "mixed") + (("diag",) if shape[2] == shape[3] else ())


def _expand(cases):
    """every case with its scenarios; `unit` (the control) once per path, on the path's first case"""
    out, seen = [], set()
    for c in cases:
        scs = scenarios(c[1], c[2])
        if c[0] not in seen:
            seen.add(c[0])
            scs = ("unit",) + scs
        out += [(c, s) for s in scs]
    return out


def _id(p):
    c, s = p
    return f"{c[0]}-{'x'.join(map(str, c[1]))}{'-causal' if c[2] else ''}-v{c[3]}-{s}"


# ------------------------------------------------------------------------------------------------ GPU helpers
def _pack(x):          # [B, H, S, hd] -> [B * S, H * hd]
    B, H, S, hd = x.shape
    return x.permute(0, 2, 1, 3).reshape(B * S, H * hd)


def _unpack(x, B, H, S, hd):
    return x.reshape(B, S, H, hd).permute(0, 2, 1, 3)


def _guarded(rows, cols, dtype=torch.float16):
    """(buffer, view): outputs live in a buffer with 8 guard columns that must come back untouched"""
    buf = torch.full((rows, cols + 8), 5.0, device="cuda", dtype=dtype)
    return buf, buf[:, :cols]


@functools.lru_cache(maxsize=2)
def _case_data(shape, causal, scenario):
    """inputs as column slices of a fused qkv / kv buffer, and the float64 reference, once per (shape, scenario)"""
    B, H, Sq, Skv, hd = shape
    C = H * hd
    q, k, v, do = [t.cuda() for t in inputs(shape, scenario)]
    if Sq == Skv:
        qkv = torch.cat([_pack(q), _pack(k), _pack(v)], 1).contiguous()
        qs, ks, vs = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
    else:
        qs = _pack(q).contiguous()
        kv = torch.cat([_pack(k), _pack(v)], 1).contiguous()
        ks, vs = kv[:, :C], kv[:, C:]
    return dict(t4=(q, k, v, do), packed=(qs, ks, vs, _pack(do).contiguous()), ref=R.ref64(q, k, v, do, causal))


@functools.lru_cache(maxsize=2)
def _model(shape, causal, scenario, cfg_items):
    return R.model64(*_case_data(shape, causal, scenario)["t4"], causal=causal, rnd=torch.float16, **dict(cfg_items))


@pytest.fixture(scope="module", autouse=True)
def _drop_cached_references():
    """the float64 references of the last shapes do not stay on the device for the rest of the session"""
    yield
    _case_data.cache_clear()
    _model.cache_clear()
    torch.cuda.empty_cache()


def _check(tag, scenario, names, got, ref, model):
    """the two assertions on each output; prints the three distances first"""
    per_head = scenario == "mixed"
    fails = []
    for n in names:
        kr, mr, km = (R.metrics(n, a, b, per_head) for a, b in ((got[n], ref[n]), (model[n], ref[n]), (got[n], model[n])))
        print(f"[attn-peaked] {tag} {scenario} {n}: kernel-vs-f64 {R.fmt(kr)} | model-vs-f64 {R.fmt(mr)} | kernel-vs-model {R.fmt(km)}")
        assert all(x == x for x in kr + km), (tag, n, "NaN")
        if not R.within(km, R.TOL[n]):
            fails.append(f"{n}: kernel vs model {R.fmt(km)} > {R.fmt(R.TOL[n])}")
        bound = tuple(max(t, 4.0 * m) for t, m in zip(R.TOL[n], mr))
        if not R.within(kr, bound):
            fails.append(f"{n}: kernel vs float64 {R.fmt(kr)} > max(tol, 4 x model) {R.fmt(bound)}")
    assert not fails, f"{tag} {scenario}: " + "; ".join(fails)


def _run_fwd(ops, data, shape, causal):
    B, H, Sq, Skv, hd = shape
    qs, ks, vs, _ = data["packed"]
    obuf, o = _guarded(B * Sq, H * hd)
    lbuf = torch.full((B * H * Sq + 8,), 5.0, device="cuda")
    lse = lbuf[:B * H * Sq].view(B, H, Sq)
    ops.attention_fwd(qs, ks, vs, o, lse, B, H, Sq, Skv, hd, causal=causal)
    assert (obuf[:, H * hd:] == 5.0).all() and (lbuf[B * H * Sq:] == 5.0).all(), "forward wrote outside its outputs"
    return o, lse


def _run_bwd(ops, data, shape, causal, o, lse, ws_kind, o_nan):
    B, H, Sq, Skv, hd = shape
    C = H * hd
    qs, ks, vs, dos = data["packed"]
    dqbuf, dq = _guarded(B * Sq, C)
    dkvbuf, dkv = _guarded(B * Skv, 2 * C)
    dbuf = torch.full((B * H * Sq + 8,), 7.0, device="cuda")
    ws = {"self": lambda: torch.empty(2 * B * H * Sq, device="cuda"), "cross": lambda: torch.empty(16 * 2 * B * Skv * C, device="cuda"),
          None: lambda: None}[ws_kind]()
    if o_nan:
        o = torch.full_like(o, float("nan"))      # the one-launch cross-attention backward must not read the attention output
    ops.attention_bwd(qs, ks, vs, o, lse, dos, dbuf[:B * H * Sq].view(B, H, Sq), dq, dkv[:, :C], dkv[:, C:], B, H, Sq, Skv, hd, causal=causal, ws=ws)
    assert (dqbuf[:, C:] == 5.0).all() and (dkvbuf[:, 2 * C:] == 5.0).all() and (dbuf[B * H * Sq:] == 7.0).all(), "backward wrote outside its outputs"
    return {"dQ": _unpack(dq, B, H, Sq, hd), "dK": _unpack(dkv[:, :C], B, H, Skv, hd), "dV": _unpack(dkv[:, C:], B, H, Skv, hd)}


# ------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("case,scenario", _expand(FWD_CASES), ids=[_id(p) for p in _expand(FWD_CASES)])
def test_attention_fwd_peaked(case, scenario):
    from textboost_amd import _lib as L, ops
    path, shape, causal, on, off, proof = case
    B, H, Sq, Skv, hd = shape
    data = _case_data(shape, causal, scenario)
    model = _model(shape, causal, scenario, tuple(sorted(model_cfg(path, hd).items(), key=str)))
    runs = []
    prev = L.lib().tb_attention_set_variant(1)
    try:
        for bits in (on,) + (() if off is None else (off,)):
            L.lib().tb_attention_set_variant(bits)
            runs.append(_run_fwd(ops, data, shape, causal))
    finally:
        L.lib().tb_attention_set_variant(prev)
    o, lse = runs[0]
    assert torch.isfinite(o).all() and torch.isfinite(lse).all()
    if off is not None:
        differ = not (torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]))
        print(f"[attn-peaked-bits] {path} {'x'.join(map(str, shape))} {scenario}: variant {on} vs {off}: O / LSE bits {'differ' if differ else 'are equal'}")
        if proof == "always":
            assert differ, f"{path}: variant {on} and its off-bit {off} gave the same bits -- the path did not run"
    _check(f"{path} {'x'.join(map(str, shape))}{' causal' if causal else ''}", scenario, ("O", "LSE"),
           {"O": _unpack(o, B, H, Sq, hd), "LSE": lse}, data["ref"], model)


@pytest.mark.parametrize("case,scenario", _expand(BWD_CASES), ids=[_id(p) for p in _expand(BWD_CASES)])
def test_attention_bwd_peaked(case, scenario):
    from textboost_amd import _lib as L, ops
    path, shape, causal, on, off, fwd_path, ws_kind, differ = case
    B, H, Sq, Skv, hd = shape
    data = _case_data(shape, causal, scenario)
    cfg = lambda p: tuple(sorted(model_cfg(p, hd, fwd_path).items(), key=str))
    model = _model(shape, causal, scenario, cfg(path))
    tag = f"{path} {'x'.join(map(str, shape))}{' causal' if causal else ''}"
    runs = {}
    prev = L.lib().tb_attention_set_variant(1)
    try:
        o, lse = _run_fwd(ops, data, shape, causal)       # the default forward: its O and LSE are what the backward gets in the model
        variants = [("on", on, ws_kind)]
        if off == "no-ws":
            variants.append(("off", on, None))            # no workspace: the dK/dV launch cannot split the queries
        elif off is not None:
            variants.append(("off", off, ws_kind))
        if path == "bwd-pipelined":
            variants.append(("dma", 1 | 2048, ws_kind))
        for name, bits, wk in variants:
            L.lib().tb_attention_set_variant(bits)
            runs[name] = _run_bwd(ops, data, shape, causal, o, lse, wk, o_nan=(path == "bwd-one-launch" and name == "on"))
    finally:
        L.lib().tb_attention_set_variant(prev)
    if differ:      # (one output may agree bitwise -- dV = P^T dO is summed in the same order by several kernels -- so the outputs are taken together)
        assert any(not torch.equal(runs["on"][n], runs["off"][n]) for n in differ), \
            f"{path}: {differ} of variant {on} and of its off run are the same bits -- the path did not run"
    if "dma" in runs:
        assert all(torch.equal(runs["on"][n], runs["dma"][n]) for n in ("dQ", "dK", "dV")), "pipelined and LDS-DMA backward kernels are bit-equal"
    _check(tag, scenario, ("dQ", "dK", "dV"), runs["on"], data["ref"], model)
    if path == "bwd-small":      # the generic pair on the same short sequence (bit 8192), against ITS model
        _check(tag + " generic pair", scenario, ("dQ", "dK", "dV"), runs["off"], data["ref"], _model(shape, causal, scenario, cfg("bwd-generic")))
