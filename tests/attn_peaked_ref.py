"""Attention on peaked and shifted score distributions: inputs, a float64 reference and a float64 OPERAND MODEL of the flash-attention family
(csrc/attention.hip, attention_il.hip, attention_small.hip).  Test-side code only.

make_inputs   Q, K, V, dO of one scenario, already rounded to the 16-bit type, so every reference sees exactly what the kernel sees.
ref64         plain float64 softmax attention, its LSE and its autograd gradients.
model64       the same computation in float64 with ONLY the roundings the kernels are documented to make (the source line of
              each one is cited at its switch below).  Kernel and model then differ by summation order, v_exp_f32 and rare rounding flips, so
              the kernel-vs-model bound is the unit-scale tolerance (TOL) on ANY data; the model-vs-float64 distance is the yardstick of what the
              documented arithmetic itself costs on such data.
metrics       rel-L2, max-abs / max|ref| and the worst head-dim channel (tests/parity.py), optionally per head.

All tensors are [B, H, S, hd]."""
import math

import torch
import torch.nn.functional as F

LOG2E = 1.4426950408889634
F64 = torch.float64

SCENARIOS = ("unit", "sink", "late", "diag", "shift+", "shift-", "mixed")
MIXED = ("sink", "late", "shift+", "shift-", "unit")      # head h of `mixed` takes MIXED[h % 5]
DEFECTS = ("norescale", "dropkey", "lsehead", "deltarow")

# the project's unit-scale tolerances (tests/test_gpu_norm_attn.py _attention_fwd_bwd): rel-L2, max-abs / max|ref|, worst channel; LSE is
# |dLSE| / max(1, |LSE|)
TOL = {"O": (2e-3, 4e-3, 3e-3), "dQ": (4e-3, 6e-3, 6e-3), "dK": (4e-3, 6e-3, 6e-3), "dV": (4e-3, 6e-3, 6e-3), "LSE": (2e-3,)}
OUTPUTS = ("O", "LSE", "dQ", "dK", "dV")


# ------------------------------------------------------------------------------------------------ inputs
def _apply(scn, q, k, u, hd, g, shift):
    """one scenario on q [B, h, Sq, hd] / k [B, h, Skv, hd] (in place on k where a single key moves); returns q, k"""
    a = math.sqrt(g * math.sqrt(hd))
    Skv = k.shape[-2]
    if scn == "unit":
        return q, k
    if scn == "sink":                       # every query prefers key 0 by ~ g nats (under the causal mask: the BOS sink)
        k = k.clone()
        k[:, :, 0:1] += a * u
        return q + a * u, k
    if scn == "late":                       # ... key Skv - 2: in the last tile (partly masked when Skv is ragged), forces the re-base there
        k = k.clone()
        k[:, :, Skv - 2:Skv - 1] += a * u
        return q + a * u, k
    if scn == "diag":
        assert q.shape[-2] == Skv, "diag: self-attention only"
        return q, 0.5 * k + q * (g / math.sqrt(hd))
    if scn in ("shift+", "shift-"):         # all logits move by ~ +- shift^2 g nats (shift = 2: 32 nats)
        s = 1.0 if scn == "shift+" else -1.0
        return q + shift * a * u, k + s * shift * a * u
    raise ValueError(scn)


def make_inputs(scenario, B, H, Sq, Skv, hd, seed, dtype=torch.float16, g=8.0, shift=2.0):
    """Q, K, V, dO of `scenario` as CPU tensors of `dtype` ([B, H, S, hd]).  u: one random unit vector per (b, h); g: nats of margin."""
    gen = torch.Generator().manual_seed(seed)
    q = torch.randn(B, H, Sq, hd, dtype=F64, generator=gen)
    k = torch.randn(B, H, Skv, hd, dtype=F64, generator=gen)
    v = torch.randn(B, H, Skv, hd, dtype=F64, generator=gen)
    do = torch.randn(B, H, Sq, hd, dtype=F64, generator=gen)
    u = torch.randn(B, H, 1, hd, dtype=F64, generator=gen)
    u = u / u.norm(dim=-1, keepdim=True)
    if scenario == "mixed":
        qs, ks = [], []
        for h in range(H):
            qh, kh = _apply(MIXED[h % 5], q[:, h:h + 1], k[:, h:h + 1], u[:, h:h + 1], hd, g, shift)
            qs.append(qh)
            ks.append(kh)
        q, k = torch.cat(qs, 1), torch.cat(ks, 1)
    else:
        q, k = _apply(scenario, q, k, u, hd, g, shift)
    return tuple(t.to(dtype) for t in (q, k, v, do))


# ------------------------------------------------------------------------------------------------ float64 reference
def _mask(Sq, Skv, causal, device):
    m = torch.zeros(Sq, Skv, dtype=F64, device=device)
    if causal:
        m = torch.full_like(m, float("-inf")).triu(1)
    return m


def _per_batch(fn, tensors, max_scores=1 << 23):
    """run fn on batch slices small enough that one score tensor stays under max_scores elements; concatenates the outputs"""
    q, k = tensors[0], tensors[1]
    B, H, Sq, Skv = q.shape[0], q.shape[1], q.shape[2], k.shape[2]
    step = max(1, min(B, max_scores // max(1, H * Sq * Skv)))
    outs = [fn(*[t[b:b + step] for t in tensors]) for b in range(0, B, step)]
    return tuple(torch.cat([o[i] for o in outs], 0) for i in range(len(outs[0])))


def ref64(q, k, v, do, causal=False, device=None):
    """O, LSE, dQ, dK, dV of plain float64 softmax attention (autograd gradients) on `device` (default: q's)"""
    device = device or q.device
    hd = q.shape[-1]

    def one(q, k, v, do):
        q, k, v = [t.clone().requires_grad_(True) for t in (q, k, v)]
        s = q @ k.transpose(-1, -2) * hd ** -0.5 + _mask(q.shape[-2], k.shape[-2], causal, device)
        o = torch.softmax(s, -1) @ v
        lse = torch.logsumexp(s, -1)
        o.backward(do)
        return o.detach(), lse.detach(), q.grad, k.grad, v.grad

    return dict(zip(OUTPUTS, _per_batch(one, [t.to(device=device, dtype=F64) for t in (q, k, v, do)])))


# ------------------------------------------------------------------------------------------------ operand model
def _rounder(rnd):
    return (lambda x: x) if rnd is None else (lambda x: x.to(rnd).to(F64))


def _scores(q, k, scaled, scale, rnd):
    """log2-domain scores.  scaled = 'q' / 'k': that operand carries scale * log2(e) and is rounded back to the 16-bit type -- fp32 multiply,
    then round (attention.hip:229 scale_frags; attention.hip:1918 for the resident key image of the one-launch cross-attention backward);
    None: the scale is applied in fp32 after the product (attention_small.hip:111)."""
    if scaled is None or rnd is None:
        return q @ k.transpose(-1, -2) * (scale * LOG2E)
    c = (torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)).to(q.device)
    sc = lambda x: (x.to(torch.float32) * c).to(rnd).to(F64)
    return (sc(q) if scaled == "q" else q) @ (sc(k) if scaled == "k" else k).transpose(-1, -2)


def _any32(x):
    """x: bool [B, H, Sq, 1] -> true for every row whose 32-row group (one wave's queries) has a true row: the re-base test is wave-uniform
    (attention.hip:358 `__any`)"""
    B, H, Sq, _ = x.shape
    pad = (-Sq) % 32
    g = F.pad(x, (0, 0, 0, pad)).view(B, H, -1, 32, 1).any(-2, keepdim=True).expand(B, H, -1, 32, 1)
    return g.reshape(B, H, Sq + pad, 1)[:, :, :Sq]


def _forward(s2, v, r, tile, fold_m, rowsum_of, defect):
    """O (normalised, unrounded), m, l from log2-domain scores.  tile = 64: attn_fwd_kernel's loop over 64-key tiles with the 2^8 lazy re-base
    (attention.hip:354-381; the LDS-DMA and software-pipelined kernels: attention.hip:801, attention_il.hip:150); tile = None: the exact row
    maximum over all keys at once (attn_xs_fwd_kernel, attention.hip:522-540).  P is rounded before P.V (attention.hip:395 pack8).
    fold_m: the reference point stays representable in the 16-bit type (attention.hip:360, the FOLDM kernels of hd = 40).
    rowsum_of: 'rounded' -- the row sum rides on the P.V product as an all-ones row of V^T, so it sums the ROUNDED P (attention.hip:406-414);
    'exact' -- it sums the fp32 P (attention.hip:388, :539)."""
    if tile is None:
        m = s2.max(-1, keepdim=True).values
        P = torch.exp2(s2 - m)
        P16 = r(P)
        return (P16 @ v), m, (P16 if rowsum_of == "rounded" else P).sum(-1, keepdim=True)
    Skv = s2.shape[-1]
    m = torch.zeros(s2.shape[:-1] + (1,), dtype=F64, device=s2.device)
    l = torch.zeros_like(m)
    o = torch.zeros(s2.shape[:-1] + (v.shape[-1],), dtype=F64, device=s2.device)
    for t0 in range(0, Skv, tile):
        st = s2[..., t0:t0 + tile]
        mx = st.max(-1, keepdim=True).values - m                 # excess of the tile's scores over the reference point
        first = t0 == 0
        if first:
            d = mx
        else:
            d = torch.where(_any32(mx > 8.0), mx.clamp_min(0.0), torch.zeros_like(mx))
        if fold_m:
            d = r(m + d) - m
        if not first:
            alpha = torch.exp2(-d)
            l = l * alpha
            if defect != "norescale":
                o = o * alpha
        m = m + d
        P = torch.exp2(st - m)
        P16 = r(P)
        o = o + P16 @ v[..., t0:t0 + tile, :]
        l = l + (P16 if rowsum_of == "rounded" else P).sum(-1, keepdim=True)
    return o, m, l


def model64(q, k, v, do, causal=False, rnd=torch.float16, scaled_fwd="q", scaled_dq="q", scaled_dkv="k", delta_from="o", rowsum_of="rounded",
            tile=64, fold_m=False, defect=None, device=None):
    """O, LSE, dQ, dK, dV as the kernels are documented to compute them, in float64 with their roundings only.  rnd: the 16-bit type, or None
    for no rounding at all (then the model IS the reference).
      scaled_fwd / scaled_dq / scaled_dkv   which operand carries scale * log2(e) in the forward, the dQ and the dK/dV score products
      delta_from   'o': rowsum(dO * O) of the ROUNDED output (attention.hip:1394-1410, attention_small.hip:80);
                   'pdp': rowsum(P * dP) over the unrounded P of the dQ-side scores (attention.hip:1950-1972), O is not read
      dS is rounded before dS.K and dS^T.Q (attention.hip:1481, :1760), P before P^T.dO (attention.hip:1759); outputs are rounded
      (attention.hip:429, :1498, :1802; the fp32 query-slice partials are summed first: attention.hip:2134).
      defect       a planted defect (DEFECTS), so that the host test can show the bounds bite"""
    assert defect is None or defect in DEFECTS
    device = device or q.device
    r = _rounder(rnd)
    hd = q.shape[-1]
    scale = hd ** -0.5

    def one(q, k, v, do):
        Sq, Skv = q.shape[-2], k.shape[-2]
        mask = _mask(Sq, Skv, causal, device)
        if defect == "dropkey":
            mask = mask.clone()
            mask[:, Skv - 1] = float("-inf")
        o, m, l = _forward(_scores(q, k, scaled_fwd, scale, rnd) + mask, v, r, tile, fold_m and rnd is not None, rowsum_of, defect)
        o16 = r(o / l)
        lse2 = m + torch.log2(l)
        lse_out = lse2 / LOG2E
        if defect == "lsehead":
            lse2 = lse2.roll(1, 1)
        dP = do @ v.transpose(-1, -2)
        Pq = torch.exp2(_scores(q, k, scaled_dq, scale, rnd) + mask - lse2)
        delta = (do * o16).sum(-1, keepdim=True) if delta_from == "o" else (Pq * dP).sum(-1, keepdim=True)
        if defect == "deltarow":
            delta = delta.roll(1, -2)
        dq = r(r(Pq * (dP - delta)) @ k * scale)
        Pk = Pq if scaled_dkv == scaled_dq else torch.exp2(_scores(q, k, scaled_dkv, scale, rnd) + mask - lse2)
        dv = r(r(Pk).transpose(-1, -2) @ do)
        dk = r(r(Pk * (dP - delta)).transpose(-1, -2) @ q * scale)
        return o16, lse_out.squeeze(-1), dq, dk, dv

    return dict(zip(OUTPUTS, _per_batch(one, [t.to(device=device, dtype=F64) for t in (q, k, v, do)])))


# ------------------------------------------------------------------------------------------------ metrics
def metrics(name, got, ref, per_head=False):
    """(rel-L2, max-abs / max|ref|, worst head-dim channel) of a [B, H, S, hd] output, or (max |d| / max(1, |ref|),) of the [B, H, S] LSE;
    per_head: the worst head of each (a head of `mixed` with small statistics must not hide behind one with large ones)"""
    a, b = got.to(F64), ref.to(F64)
    assert a.shape == b.shape, (name, a.shape, b.shape)
    if name == "LSE":
        return (((a - b).abs() / b.abs().clamp_min(1.0)).max().item(),)
    if per_head:
        ms = [metrics(name, a[:, h:h + 1], b[:, h:h + 1]) for h in range(a.shape[1])]
        return tuple(max(m[i] for m in ms) for i in range(3))
    e = a - b
    rel = (e.norm() / b.norm().clamp_min(1e-30)).item()
    mab = (e.abs().max() / b.abs().max().clamp_min(1e-30)).item()
    ch = (e.pow(2).sum((0, 1, 2)).sqrt() / b.pow(2).sum((0, 1, 2)).sqrt().clamp_min(1e-30)).max().item()
    return rel, mab, ch


def within(m, bound):
    return all(x <= b for x, b in zip(m, bound))


def fmt(m):
    return "/".join(f"{x:.1e}" for x in m)
