"""The optimizer tail on the GPU -- `tb_optimizer_tail` (two launches) and the ten separate entry points it replaces, in the order of
trainer.py's optimizer_step -- against tests/optim_ref.py, a float64 restatement of the torch semantics that tests/test_optim_ref_host.py anchors
to the real torch.optim.AdamW.  Buffers are hand built (no build_step): every parameter, moment, gradient and state buffer is a slice of one
allocation with 64 sentinel floats on both sides, checked after every step.

Bounds (u = 2^-24; derived from the fp32 arithmetic, not from what the kernels give; s = successful steps of the run so far):
  m, v        s * 4u relative (three or four fp32 roundings per step on top of fl32(beta), fl32(1 - beta)), plus the rounding of the gradient
              coefficient where it is not a power of two: 2u for grad_div = 3 (1 / (scale * 3), the product), ((T + 16) / 2 + 6) u on a clipped step
              of the LoRA group (T = ceil(n / 16384) strided adds per thread + 15 tree adds + the square, halved by the root; then * inv, + 1e-6,
              the division, * inv, the product); twice that on v.  m is a sum of SIGNED terms, so its bound is relative to the same moving
              average over |g| (optim_ref.Group.m_abs), the forward error bound of a sum; v's terms are positive.
  parameters  s * 4u |p| + c * sum |delta|, c = u/2 * beta2 / (1 - beta2) + u * beta1 / (1 - beta1) + 1e-6 (3.1e-5 at the defaults, 4.2e-6 at 0.8 / 0.99)
  decay rows  s * 2u relative
  added rows  the parameter bound, plus D u relative for the clamp factor (it is formed anew from the row on every iteration: nothing of it
              accumulates), plus what the parameter bound does to the row's norm
  added_norms D u relative plus the L2 norm of the row's parameter bound
  state       scale, tracker, step, found_inf exact; grad norm, both coefficients, both sums of squares n u relative;
              bias corrections u * k beta^k / (1 - beta^k) + 2u; the lr multiplier slot u absolute

Worst observed error / bound per quantity over all cases, MI355X (the `[optim]` lines this file prints hold them per case):
  m 0.53   v 0.72   parameters 0.52   decay rows 0.65   added rows 0.05   added_norms 0.01   grad norm / coefficients / sums of squares 0.002
  bias corrections 0.16   lr multiplier 0.25   tb_sumsq alone 0.18   tb_row_norms 0.006   tb_renorm_rows 0.03
The fused and the separate form are bit-equal in every case, so the figures hold for both.

Which terms failed, and where.  (1) While 1 - beta and the bias corrections were still formed from fl32(beta), v missed its bound on the first
step of every case that runs AdamW (an fp32 host emulation of that arithmetic: 4.4x at beta2 = 0.99, 6.7x at beta2 = 0.999 on a clipped LoRA
step; (beta2 - fl32(beta2)) / (1 - beta2) = 1.3e-5 is 54x the bare 4u): fixed in the kernels.  (2) The two terms this header adds to the plain
`s * 4u` are measured on every run without them (the `[optim-literal]` lines) and do fail with the fixed kernels, MI355X: m relative to |m|
itself is missed by up to 1.25e4x (defaults, step 4, m_added element 884; hundreds to thousands in every multi-step case, always at an
element whose terms nearly cancel); v without the clip coefficient's roundings by up to 1.27x (all-D200, step 0, v_lora element 40; 1.0 ...
1.3 on the clipped LoRA steps only, never in the unclipped groups).

Each of these one-line changes of optim.hip, built as a library of its own and run under this file on an MI355X, turns tests red:
  LoRA role takes coef_emb              23 cases (m_lora, step 0: 1.6e6 x the bound)
  added rows take d.lr                  23 cases (added rows, step 0: 1.9e5 x)
  `i <= n4` in the decay slab           25 cases (the four sentinels behind the decay buffer)
  no `b == 0` in the bias corrections   decay-only (ST_BC1 published as 1)
  `tr > growth_interval`                12 cases (the scale stays 1024 on the third step)
  table index 0 past the end            lr-table (ST_LR_MULT on step 5)
"""
import dataclasses
import math
from dataclasses import dataclass, field

import pytest
import torch

import optim_ref as R

pytestmark = pytest.mark.gpu
dev = "cuda"
U = 2.0 ** -24
SENTINEL = 1234.5
GUARD = 64
SLAB = 16384                    # floats of one decay workgroup of the fused tail (256 threads x 16 float4)


def _ops():
    from textboost_amd import ops, _lib as L
    return ops, L


def _sync():
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ guarded buffers
class Arena:
    """named fp32 buffers carved out of ONE allocation: 64 sentinel floats before the first, between any two and after the last, every buffer
    starting on a 16-byte boundary (the decay view is read as float4)"""

    def __init__(self):
        self.spans, self.n = {}, GUARD

    def add(self, name, numel):
        self.spans[name] = (self.n, numel)
        self.n += (numel + 3) // 4 * 4 + GUARD

    def finish(self):
        self.buf = torch.full((self.n,), SENTINEL, device=dev)
        assert self.buf.data_ptr() % 16 == 0
        guard = torch.ones(self.n, dtype=torch.bool)
        for a, n in self.spans.values():
            guard[a:a + n] = False
        self.guard = guard.to(dev)
        self.n_guard = int(guard.sum())
        return self

    def __getitem__(self, name):
        a, n = self.spans[name]
        return self.buf[a:a + n]

    def check(self, what):
        g = self.buf[self.guard]
        assert g.numel() == self.n_guard and bool((g == SENTINEL).all()), \
            (what, "sentinel overwritten at", torch.nonzero(self.guard & (self.buf != SENTINEL)).flatten()[:8].tolist(), self.spans)


# ------------------------------------------------------------------------------------------------------------------ cases
CUSTOM = dict(lr=1e-3, emb_lr=5e-3, wd=0.05, beta1=0.8, beta2=0.99, eps=1e-8, max_norm=1.0, mean_norm=0.75, growth_interval=3)
MAIN = ("ok", "ok", "ok", "inf_lora", "ok", "ok", "ok", "nan_emb")   # growth on the 3rd, backoff, growth on the 7th, backoff


def _defaults(**kw):
    from textboost_amd.trainer import StepHyper
    h = StepHyper()
    d = dict(lr=h.lr, emb_lr=h.emb_lr, wd=h.wd, beta1=h.beta1, beta2=h.beta2, eps=h.eps, max_norm=h.max_grad_norm, mean_norm=0.75,
             growth_interval=h.growth_interval)
    d.update(kw)
    return d


@dataclass
class Case:
    name: str
    base: str = "custom"                              # "custom" = CUSTOM, "defaults" = the project's StepHyper
    over: dict = field(default_factory=dict)          # hyperparameters that differ from the base
    zero_row: int = -1                                # this added row and its gradients are all zero
    steps: tuple = MAIN
    n_lora: int = 3 * 256 + 17
    n_added: int = 3
    D: int = 200
    n_unet: int = 1000
    n_decay: int = 2 * SLAB + 4 * 37
    scale0: float = 1024.0
    step0: int = 0
    resume: bool = False
    seed: int = 0

    def __str__(self):
        return self.name


SIX = ("ok", "ok", "inf_lora", "ok", "ok", "ok")
CASES = [Case(f"all-D{D}", D=D, seed=D) for D in (64, 200, 768, 1024)] + [
    Case("decay4", n_decay=4, steps=SIX, seed=1),
    Case("defaults", base="defaults", steps=("ok",) * 6, D=768, n_decay=SLAB + 4 * 37, scale0=65536.0, seed=2),
    Case("lr-table", base="defaults", over=dict(growth_interval=3, lr_table=[1.0, 0.7, 0.45, 0.2]), steps=("ok", "ok", "inf_lora") + ("ok",) * 5, seed=3),      # 4 entries, 7 successful steps
    Case("grad-div2", over=dict(grad_div=2.0), steps=("ok", "ok", "nan_emb", "ok", "ok", "ok"), seed=4),
    Case("grad-div3", over=dict(grad_div=3.0), steps=("ok", "ok", "nan_emb", "ok", "ok", "ok"), seed=5),
    Case("noscaler", over=dict(use_scaler=False), steps=("ok",) * 6, scale0=1.0, seed=6),
    Case("noscaler-inf", over=dict(use_scaler=False), steps=SIX, scale0=1.0, seed=7),
    Case("noscaler-nan", over=dict(use_scaler=False), steps=("ok", "ok", "nan_lora", "ok", "ok", "ok"), scale0=1.0, seed=8),
    # workgroup 0 of the fused tail publishes the state whatever its role is: an added row / a UNet block / a decay slab / (LoRA, no decay at all)
    Case("no-lora", n_lora=0, steps=("ok", "ok", "ok", "nan_emb", "ok", "ok"), seed=9),
    Case("unet-decay", n_lora=0, n_added=0, steps=("ok",) * 6, seed=10),
    Case("decay-only", n_lora=0, n_added=0, n_unet=0, steps=("ok",) * 6, seed=11),
    Case("lora-only", n_added=0, n_unet=0, n_decay=0, steps=SIX, seed=12),
] + [Case(f"resume-{base}-{k}", base=base, steps=("ok",), step0=k, resume=True, n_decay=SLAB + 4 * 37, seed=20 + k)
     for base in ("defaults", "custom") for k in (0, 1, 9, 999, 1999)]


def _hyper(case):
    assert case.base in ("custom", "defaults")
    return R.Hyper(**dict(CUSTOM if case.base == "custom" else _defaults(), **case.over))


def _f32(x):
    return x.float()


def _make(case):
    """initial fp32 buffers, the raw fp32 gradients of every step and the reference's snapshots after every step.  The reference starts from the
    same fp32 values and is fed the same fp32 gradients (as doubles): its inputs are what the device's are, exactly."""
    hp = _hyper(case)
    g = torch.Generator().manual_seed(1000 + case.seed)
    rn = lambda *s: torch.randn(*s, generator=g)     # noqa: E731
    init = {}
    if case.n_lora:
        init["lora"] = rn(case.n_lora)
    if case.n_added:
        rows = rn(case.n_added, case.D)
        rows *= (hp.mean_norm * torch.tensor([0.5, 1.0, 2.0, 0.25, 4.0][:case.n_added]) / rows.norm(dim=-1))[:, None]   # both sides of mean_norm
        if case.zero_row >= 0:
            rows[case.zero_row] = 0.0
        init["added"] = rows
    if case.n_unet:
        init["unet"] = rn(case.n_unet) * 0.1
    for n in [k for k in init]:
        init["m_" + n] = rn(*init[n].shape) * 0.01 if case.resume else torch.zeros_like(init[n])
        init["v_" + n] = torch.rand(*init[n].shape, generator=g) * 1e-4 if case.resume else torch.zeros_like(init[n])
    if case.n_decay:
        init["decay"] = rn(case.n_decay)
    names = [n for n in ("lora", "added", "unet") if n in init]
    groups = {n: R.Group(init[n].double(), init["m_" + n].double(), init["v_" + n].double()) for n in names}
    groups["decay"] = init["decay"].double() if case.n_decay else None
    state = R.TailState(scale=case.scale0, step=case.step0)
    raws, snaps = [], []
    sum_delta = {n: torch.zeros_like(groups[n].p) for n in names}
    cmax = {n: 0.0 for n in names}
    cdiv = 0.0
    s_run = 0
    for it, kind in enumerate(case.steps):
        mul = state.scale * hp.grad_div
        sigma = 0.1 if it % 2 == 0 else 0.005           # unscaled LoRA norm ~ 2.8 (clipped) / ~ 0.14 (not clipped)
        raw = {}
        if "lora" in names:
            raw["lora"] = _f32(rn(case.n_lora) * sigma * mul)
        if "added" in names:
            raw["added"] = _f32(rn(case.n_added, case.D) * 0.05 * mul)
            if case.zero_row >= 0:
                raw["added"][case.zero_row] = 0.0
        if "unet" in names:
            raw["unet"] = _f32(rn(case.n_unet) * 0.3 * mul)
        if kind == "inf_lora":
            raw["lora"][7] = float("inf")
        elif kind == "nan_lora":
            raw["lora"][7] = float("nan")
        elif kind == "nan_emb":
            raw["added"][1, case.D - 1] = float("nan")
        else:
            assert kind == "ok"
        raws.append(raw)
        scale_in = state.scale
        out = R.tail_step(state, groups, {n: raw[n].double() for n in names}, hp)
        if not state.found_inf:
            s_run += 1
            pow2 = math.frexp(mul)[0] == 0.5
            for n in names:
                sum_delta[n] += out["delta"][n].abs()
                c = 0.0 if pow2 else 2 * U
                cdiv = max(cdiv, c)
                if n == "lora" and state.coef_lora * scale_in * hp.grad_div < 1.0:
                    c += ((math.ceil(case.n_lora / 16384) + 16) / 2 + 6) * U
                cmax[n] = max(cmax[n], c)
        snap = {"state": dataclasses.replace(state), "s_run": s_run, "iters": it + 1, "kind": kind, "scale_in": scale_in,
                "added_norms": out["added_norms"], "cmax": dict(cmax), "cdiv": cdiv,
                "ss": {n: float((raw[n].double() ** 2).sum()) for n in names if n != "unet"}}
        for n in names:
            G = groups[n]
            snap[n], snap["m_" + n], snap["v_" + n], snap["mabs_" + n] = G.p.clone(), G.m.clone(), G.v.clone(), G.m_abs.clone()
            snap["sum_delta_" + n] = sum_delta[n].clone()
        if case.n_decay:
            snap["decay"] = groups["decay"].clone()
        snaps.append(snap)
    return hp, init, raws, snaps


# ------------------------------------------------------------------------------------------------------------------ the device side
BUFFERS = ("state", "lora", "m_lora", "v_lora", "added", "m_added", "v_added", "unet", "m_unet", "v_unet", "decay", "added_norms")


def _run_device(case, hp, init, raws, fused):
    ops, L = _ops()
    ne = case.n_added * case.D
    A = Arena()
    A.add("state", L.ST_COUNT)
    A.add("ws", 132)
    A.add("grad", max(case.n_lora + ne + case.n_unet, 4))
    for n in init:
        A.add(n, init[n].numel())
    if case.n_added:
        A.add("added_norms", case.n_added)
    if hp.lr_table is not None:
        A.add("lr_table", len(hp.lr_table))
    A.finish()
    for n in init:
        A[n].copy_(init[n].flatten())
    st = A["state"]
    st.zero_()
    st[L.ST_LOSS_SCALE], st[L.ST_STEP] = case.scale0, float(case.step0)
    A["ws"].zero_()
    A["grad"].zero_()
    table = None
    if hp.lr_table is not None:
        table = A["lr_table"]
        table.copy_(torch.tensor(hp.lr_table))
    grp = lambda n: (A[n], A["m_" + n], A["v_" + n])     # noqa: E731
    lora = grp("lora") if case.n_lora else None
    unet = grp("unet") if case.n_unet else None
    added = (A["added"].view(case.n_added, case.D), A["m_added"], A["v_added"]) if case.n_added else None
    decay = A["decay"] if case.n_decay else None
    norms = A["added_norms"] if case.n_added else None
    grad, nl = A["grad"], case.n_lora
    kw = dict(beta1=hp.beta1, beta2=hp.beta2, eps=hp.eps, wd=hp.wd)
    snaps = []
    for it, raw in enumerate(raws):
        flat = torch.cat([raw[n].flatten() for n in ("lora", "added", "unet") if n in raw] or [torch.zeros(4)])
        grad[:flat.numel()].copy_(flat)
        if fused:
            ops.optimizer_tail(st, grad, A["ws"], lora=lora, added=added, unet=unet, decay=decay, added_norms=norms, lr_table=table,
                               lr=hp.lr, emb_lr=hp.emb_lr, max_norm=hp.max_norm, mean_norm=hp.mean_norm, growth_factor=hp.growth_factor,
                               backoff_factor=hp.backoff_factor, growth_interval=hp.growth_interval, use_scaler=hp.use_scaler,
                               grad_div=hp.grad_div, **kw)
        else:       # trainer.py optimizer_step, the unfused branch, launch for launch
            if lora:
                ops.sumsq(grad[:nl], st[L.ST_SUMSQ_LORA:])
            if added:
                ops.sumsq(grad[nl:nl + ne], st[L.ST_SUMSQ_EMB:])
            if table is not None:
                ops.lr_from_table(st, table)
            ops.scaler_update(st, hp.max_norm, hp.beta1, hp.beta2, hp.growth_factor, hp.backoff_factor, hp.growth_interval, hp.use_scaler,
                              grad_div=hp.grad_div)
            if lora:
                ops.adamw(lora[0], grad[:nl], lora[1], lora[2], hp.lr, st, L.ST_COEF_LORA, **kw)
            if decay is not None:
                ops.weight_decay(decay, 1.0 - hp.emb_lr * hp.wd, st)
            if added:
                ops.adamw(added[0].view(-1), grad[nl:nl + ne], added[1], added[2], hp.emb_lr, st, L.ST_COEF_EMB, **kw)
                ops.renorm_rows(added[0], hp.mean_norm, norms)
            if unet:
                ops.adamw(unet[0], grad[nl + ne:nl + ne + case.n_unet], unet[1], unet[2], hp.lr, st, L.ST_COEF_EMB, **kw)
        _sync()
        A.check((case.name, "fused" if fused else "separate", it))
        snaps.append({n: A[n].clone().cpu() for n in BUFFERS if n in A.spans})
    return snaps


# ------------------------------------------------------------------------------------------------------------------ comparison
class Ratios(dict):
    literal = None      # {key: (worst error / bound, where, element)} of the bounds that are measured, not asserted

    def observe(self, key, got, ref, bound, where):
        got, ref, bound = [torch.as_tensor(x, dtype=torch.float64).flatten() for x in (got, ref, bound)]
        ok = torch.isfinite(ref) & (got != ref)
        if ok.any():
            r = torch.where(ok, (got - ref).abs() / bound, torch.zeros_like(ref))
            self.literal = self.literal or {}
            if float(r.max()) > self.literal.get(key, (0.0,))[0]:
                self.literal[key] = (float(r.max()), where, int(r.argmax()))

    def add(self, key, got, ref, bound, where):
        """worst |got - ref| / bound over the elements whose reference is finite; the non-finite ones must be non-finite in the same way"""
        got, ref, bound = [torch.as_tensor(x, dtype=torch.float64).flatten() for x in (got, ref, bound)]
        bound = bound.expand_as(ref)
        fin = torch.isfinite(ref)
        assert torch.equal(torch.isnan(got), torch.isnan(ref)) and torch.equal(got[~fin & ~torch.isnan(ref)], ref[~fin & ~torch.isnan(ref)]), \
            (where, key, "non-finite pattern differs", torch.nonzero(torch.isnan(got) != torch.isnan(ref)).flatten()[:8].tolist())
        diff = (got[fin] - ref[fin]).abs()
        r = torch.where(diff == 0, torch.zeros_like(diff), diff / bound[fin])
        worst = float(r.max()) if r.numel() else 0.0
        self[key] = max(self.get(key, 0.0), worst)
        if not worst <= 1.0:
            i = int(torch.nonzero(fin).flatten()[r.argmax()])
            raise AssertionError(f"{where} {key}: error / bound = {worst:.3g} at element {i}: got {got[i].item():.9g} ref {ref[i].item():.9g} "
                                 f"bound {bound[i].item():.3g}")


def _compare(case, hp, ref_snaps, dev_snaps, init, label):
    _, L = _ops()
    rat = Ratios()
    c_upd = 0.5 * U * hp.beta2 / (1 - hp.beta2) + U * hp.beta1 / (1 - hp.beta1) + 1e-6
    nU = max(case.n_lora, 2) * U
    names = [n for n in ("lora", "added", "unet") if n in ref_snaps[0]]
    prev = {n: init[n].flatten() for n in init}
    prev_state = None
    for it, (ref, got) in enumerate(zip(ref_snaps, dev_snaps)):
        where = f"{case.name}/{label} step {it} ({ref['kind']})"
        rs, st, s = ref["state"], got["state"].double(), ref["s_run"]
        # ---- state: exact slots
        assert st[L.ST_FOUND_INF] == float(rs.found_inf) and st[L.ST_STEP] == rs.step and st[L.ST_LOSS_SCALE] == rs.scale \
            and st[L.ST_GROWTH_TRACKER] == rs.tracker, (where, st.tolist(), rs)
        rat.add("gnorm", st[L.ST_GRAD_NORM], rs.grad_norm, nU * abs(rs.grad_norm), where)
        rat.add("coef", st[L.ST_COEF_LORA], rs.coef_lora, nU * abs(rs.coef_lora), where)
        rat.add("coef", st[L.ST_COEF_EMB], rs.coef_emb, nU * abs(rs.coef_emb), where)
        for n, slot in (("lora", L.ST_SUMSQ_LORA), ("added", L.ST_SUMSQ_EMB)):
            if n in names:
                rat.add("sumsq", st[slot], ref["ss"][n], ref[n].numel() * U * abs(ref["ss"][n]), where)
        if hp.lr_table is not None:
            rat.add("lr_mult", st[L.ST_LR_MULT], float(torch.tensor(rs.lr_mult).float()) - 1.0, U, where)
        if not rs.found_inf:
            for slot, beta, bc in ((L.ST_BC1, hp.beta1, rs.bc1), (L.ST_BC2, hp.beta2, rs.bc2)):
                assert bc == 1.0 - beta ** rs.step
                rat.add("bc", st[slot], bc, (U * rs.step * beta ** rs.step / bc + 2 * U) * bc, where)
        else:
            # ---- a skipped step leaves everything but the scaler (and the clamp of the added rows) bit for bit as it was
            assert hp.use_scaler and rs.scale == ref["scale_in"] * hp.backoff_factor and rs.tracker == 0
            same = [n for n in BUFFERS if n in got and n not in ("state", "added", "added_norms")]
            for n in same:
                assert torch.equal(got[n], prev[n]), (where, n, "changed on a skipped step")
            for slot in (L.ST_STEP, L.ST_BC1, L.ST_BC2):
                assert prev_state is None or got["state"][slot] == prev_state[slot], (where, slot)
        if not hp.use_scaler:
            assert st[L.ST_FOUND_INF] == 0 and st[L.ST_LOSS_SCALE] == case.scale0 and st[L.ST_GROWTH_TRACKER] == 0 and st[L.ST_STEP] == it + 1
        # ---- moments and parameters
        for n in names:
            cm = ref["cmax"][n]
            rat.add("m", got["m_" + n], ref["m_" + n], (s * 4 * U + cm) * ref["mabs_" + n], where + " m_" + n)
            rat.add("v", got["v_" + n], ref["v_" + n], (s * 4 * U + 2 * cm) * ref["v_" + n], where + " v_" + n)
            # measured only: the bounds without the two terms the header adds (relative to |m| itself, no clip-coefficient term)
            rat.observe("m", got["m_" + n], ref["m_" + n], (s * 4 * U + ref["cdiv"]) * ref["m_" + n].abs(), where + " m_" + n)
            rat.observe("v", got["v_" + n], ref["v_" + n], (s * 4 * U + 2 * ref["cdiv"]) * ref["v_" + n], where + " v_" + n)
            bp = s * 4 * U * ref[n].abs() + c_upd * ref["sum_delta_" + n]
            if n != "added":
                rat.add("p", got[n], ref[n], bp, where + " " + n)
                continue
            rows, D = ref[n], case.D
            bpn = torch.nan_to_num(bp, nan=0.0).norm(dim=-1, keepdim=True)
            nrm = ref["added_norms"][:, None]
            rat.add("rows", got[n], rows, bp + (D * U + bpn / nrm) * rows.abs(), where + " added")
            rat.add("norms", got["added_norms"], ref["added_norms"], D * U * ref["added_norms"] + bpn[:, 0], where)
        if "decay" in ref:
            rat.add("decay", got["decay"], ref["decay"], s * 2 * U * ref["decay"].abs(), where)
        prev, prev_state = got, got["state"]
    return rat


def _bit_equal(case, a, b):
    for it, (x, y) in enumerate(zip(a, b)):
        for n in x:
            same = torch.equal(x[n], y[n]) or (bool((torch.isnan(x[n]) == torch.isnan(y[n])).all())
                                               and torch.equal(torch.nan_to_num(x[n]), torch.nan_to_num(y[n])))
            assert same, (case.name, it, n, (x[n] - y[n]).abs().max().item(), torch.nonzero(x[n] != y[n]).flatten()[:8].tolist())


def _line(case, label, rat):
    print(f"[optim] {case.name}/{label}: " + "  ".join(f"{k} {v:.3f}" for k, v in sorted(rat.items())))
    for k, (r, where, i) in sorted((rat.literal or {}).items()):
        print(f"[optim-literal] {k} without the header's two terms: {r:.3g} at {where} element {i}")


@pytest.mark.parametrize("case", CASES, ids=str)
def test_tail_fused_and_separate_match_float64_adamw(case):
    hp, init, raws, ref = _make(case)
    kinds = [r["kind"] for r in ref]
    if case.n_lora and len(case.steps) > 1:           # the clip is active on some steps and inactive on others
        cl = [r["state"].coef_lora < r["state"].coef_emb for r in ref if math.isfinite(r["state"].coef_lora)]
        assert any(cl) and not all(cl), cl
    if hp.use_scaler:
        assert [r["state"].found_inf for r in ref] == [k != "ok" for k in kinds]
    if case.steps == MAIN:                            # growth before and after an overflow
        assert [r["state"].scale for r in ref] == [1024.0, 1024.0, 2048.0, 1024.0, 1024.0, 1024.0, 2048.0, 1024.0]
    if hp.lr_table is not None:                       # the index stays on the skipped step and holds the last entry past the end
        assert [r["state"].lr_mult for r in ref] == [1.0, 0.7, 0.45, 0.45, 0.2, 0.2, 0.2, 0.2] and ref[-1]["state"].step == 7
    fused = _run_device(case, hp, init, raws, fused=True)
    _line(case, "fused", _compare(case, hp, ref, fused, init, "fused"))
    sep = _run_device(case, hp, init, raws, fused=False)
    _line(case, "separate", _compare(case, hp, ref, sep, init, "separate"))
    _bit_equal(case, fused, sep)


def test_all_zero_added_row_becomes_nan_like_the_reference():
    """min(mean_norm, 0) / 0: the reference script (train_textboost.py:1146-1149, no guard) turns an all-zero added row into NaN, and so do
    tb_renorm_rows and the fused clamp.  Documented behaviour, not a wish: a zero row with zero gradient stays zero through AdamW."""
    ops, L = _ops()
    case = Case("zero-row", steps=("ok",), n_lora=0, n_unet=0, n_decay=0, D=200, zero_row=1)
    hp, init, raws, ref = _make(case)
    assert not init["added"][1].any() and not raws[0]["added"][1].any()
    want = ref[0]["added"]
    assert torch.isnan(want[1]).all() and torch.isfinite(want[0]).all() and torch.isfinite(want[2]).all() and ref[0]["added_norms"][1] == 0
    for fused in (True, False):
        got = _run_device(case, hp, init, raws, fused)[0]
        rows = got["added"].view(case.n_added, case.D)
        assert torch.isnan(rows[1]).all() and torch.isfinite(rows[0]).all() and torch.isfinite(rows[2]).all()
        assert got["added_norms"][1] == 0 and got["state"][L.ST_FOUND_INF] == 0


def _guarded(x):
    A = Arena()
    A.add("x", x.numel())
    A.add("out", 16)
    A.finish()
    A["x"].copy_(x.flatten())
    return A


@pytest.mark.parametrize("n", [1, 255, 257, 64 * 256 + 1])
def test_sumsq_against_float64(n):
    """every term is squared (one rounding) and then goes through at most ceil(n / 16384) strided adds, the 9 adds of the block sum and the 6
    of the final wave sum; never more than n roundings in all"""
    ops, _ = _ops()
    x = torch.randn(n, generator=torch.Generator().manual_seed(n)) * 3
    A = _guarded(x)
    ops.sumsq(A["x"], A["out"])
    _sync()
    A.check(("sumsq", n))
    ref = float((x.double() ** 2).sum())
    bound = min(n, math.ceil(n / 16384) + 16) * U * ref
    got = float(A["out"][0])
    print(f"[optim] sumsq n={n}: error / bound {abs(got - ref) / bound:.3f}")
    assert abs(got - ref) <= bound, (n, got, ref)
    assert bool((A["out"][1:] == SENTINEL).all())


@pytest.mark.parametrize("D", [64, 200, 768, 1024])
def test_row_norms_and_renorm_rows_against_float64(D):
    ops, _ = _ops()
    rows = 8
    g = torch.Generator().manual_seed(D)
    mean_norm = 0.75
    x = torch.randn(rows, D, generator=g)
    x *= (mean_norm * torch.tensor([0.25, 0.5, 0.999, 1.001, 2.0, 4.0, 1.0, 30.0]) / x.norm(dim=-1))[:, None]     # both sides of mean_norm
    ref_n = x.double().norm(dim=-1)
    A = _guarded(x)
    ops.row_norms(A["x"].view(rows, D), A["out"])
    _sync()
    A.check(("row_norms", D))
    r1 = ((A["out"][:rows].cpu().double() - ref_n).abs() / (D * U * ref_n)).max().item()
    assert r1 <= 1.0 and bool((A["out"][rows:] == SENTINEL).all()), r1
    A["out"].fill_(SENTINEL)
    ops.renorm_rows(A["x"].view(rows, D), mean_norm, A["out"])
    _sync()
    A.check(("renorm_rows", D))
    r2 = ((A["out"][:rows].cpu().double() - ref_n).abs() / (D * U * ref_n)).max().item()
    want = torch.minimum(torch.full_like(ref_n, mean_norm), ref_n)[:, None] / ref_n[:, None] * x.double()
    got = A["x"].view(rows, D).cpu().double()
    r3 = ((got - want).abs() / ((D + 2) * U * want.abs())).max().item()      # the norm, the division, the product
    print(f"[optim] rows D={D}: row_norms {r1:.3f}  renorm norms {r2:.3f}  renorm rows {r3:.3f}")
    assert r2 <= 1.0 and r3 <= 1.0 and bool((A["out"][rows:] == SENTINEL).all()), (r2, r3)
    small = ref_n < mean_norm
    assert small.any() and (~small).any()
    assert torch.equal(got[small].float(), x[small])                         # f = nrm / nrm = 1: rows under mean_norm are untouched


def test_row_norms_and_weight_decay_refuse_a_ragged_count():
    _, L = _ops()
    x = torch.zeros(6 * 64, device=dev)
    out = torch.zeros(16, device=dev)
    TB_EINVAL = -22
    assert L.lib().tb_row_norms(L.ptr(x), 6, 64, L.ptr(out), L.stream()) == TB_EINVAL
    assert L.lib().tb_weight_decay(L.ptr(x), 6, 0.5, L.ptr(out), L.stream()) == TB_EINVAL
    _sync()
    assert not x.any() and not out.any()
