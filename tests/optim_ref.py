"""The optimizer tail of one loop iteration, restated on float64 CPU tensors from the documented behaviour of the torch pieces the reference
training script calls (train_textboost.py:1108-1149): GradScaler.unscale_ / step / update, torch.nn.utils.clip_grad_norm_, torch.optim.AdamW
under a LambdaLR schedule that accelerate advances on successful steps only, and the norm clamp of the added embedding rows.

It is the reference of tests/test_gpu_optim.py and is itself anchored to the real torch.optim.AdamW by tests/test_optim_ref_host.py.
Hyperparameters stay Python doubles (nothing here is rounded to fp32), every tensor is float64, the order of operations is torch's."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Optional

import torch


@dataclass
class Hyper:
    lr: float = 5e-5
    emb_lr: float = 1e-3
    beta1: float = 0.9
    beta2: float = 0.999
    eps: float = 1e-8
    wd: float = 1e-2
    max_norm: float = 1.0
    mean_norm: float = 1.0
    growth_factor: float = 2.0
    backoff_factor: float = 0.5
    growth_interval: int = 2000
    use_scaler: bool = True
    grad_div: float = 1.0                 # the gradient buffers hold a SUM over this many ranks / micro batches
    lr_table: Optional[list] = None       # lambda(k) of the k-th successful step; None = the constant schedule


@dataclass
class TailState:
    scale: float = 65536.0
    tracker: int = 0
    step: int = 0                         # successful (not skipped) optimizer steps so far
    # what the last tail_step saw (the device publishes the same quantities in its state array)
    found_inf: bool = False
    grad_norm: float = 0.0                # norm of the unscaled LoRA gradients, before the clip
    coef_lora: float = 0.0                # what a raw LoRA gradient is multiplied by: unscale x clip
    coef_emb: float = 0.0                 # the same for the unclipped groups: unscale only
    bc1: float = 0.0
    bc2: float = 0.0
    lr_mult: float = 1.0


@dataclass
class Group:
    """one AdamW param group's flat parameter with its moments.  m_abs is not optimizer state: it is the same moving average over |g|, the
    magnitude the first moment's terms had before they cancelled, which an fp32 forward error bound of m is relative to."""
    p: torch.Tensor
    m: torch.Tensor
    v: torch.Tensor
    m_abs: torch.Tensor = field(default=None)

    def __post_init__(self):
        assert self.p.dtype == self.m.dtype == self.v.dtype == torch.float64
        if self.m_abs is None:
            self.m_abs = self.m.abs()


def lr_multiplier(hp: Hyper, k: int) -> float:
    if hp.lr_table is None:
        return 1.0
    return float(hp.lr_table[min(k, len(hp.lr_table) - 1)])


def clamp_rows(rows: torch.Tensor, mean_norm: float) -> torch.Tensor:
    """the norm clamp of the added embedding rows, in place: a row longer than mean_norm is scaled back to it, a shorter one is multiplied by
    nrm / nrm (1, or NaN for an all-zero row: there is no guard).  Returns the row norms from before the clamp."""
    nrm = torch.linalg.vector_norm(rows, dim=-1)
    rows.mul_((nrm.clamp(max=mean_norm) / nrm)[:, None])
    return nrm


def tail_step(state: TailState, groups: dict, grads: dict, hp: Hyper) -> dict:
    """One iteration.  groups: {"lora": Group | None, "added": Group | None ([k, D] rows), "unet": Group | None, "decay": float64 tensor | None};
    grads: raw (loss-scaled, summed over ranks) float64 gradients under the same keys.  Everything is updated in place.  Returns
    {"delta": {name: the Adam update subtracted from that group's parameters, zeros on a skipped step}, "added_norms": row norms before the clamp}."""
    names = [n for n in ("lora", "added", "unet") if groups.get(n) is not None]
    # 1. GradScaler.unscale_ and DDP's mean
    g = {n: grads[n].to(torch.float64) / (state.scale * hp.grad_div) for n in names}
    state.coef_emb = 1.0 / (state.scale * hp.grad_div)
    # 2. the inf check exists only under the scaler, over the text encoder's two groups
    state.found_inf = bool(hp.use_scaler and any(not torch.isfinite(g[n]).all() for n in names if n != "unet"))
    # 3. clip_grad_norm_ over the LoRA group only
    total = torch.linalg.vector_norm(g["lora"]) if "lora" in g else torch.zeros((), dtype=torch.float64)
    clip = torch.clamp(hp.max_norm / (total + 1e-6), max=1.0)
    state.grad_norm, state.coef_lora = float(total), float(clip) * state.coef_emb
    if "lora" in g:
        g["lora"] = g["lora"] * clip
    state.lr_mult = lr_multiplier(hp, state.step)
    delta = {n: torch.zeros_like(groups[n].p) for n in names}
    if not state.found_inf:
        # 4. AdamW, every group at its base lr times lambda(successful steps so far)
        state.step += 1
        state.bc1 = 1.0 - hp.beta1 ** state.step
        state.bc2 = 1.0 - hp.beta2 ** state.step
        for n in names:
            G = groups[n]
            lr = (hp.emb_lr if n == "added" else hp.lr) * state.lr_mult
            G.p.mul_(1.0 - lr * hp.wd)
            G.m.mul_(hp.beta1).add_(g[n], alpha=1.0 - hp.beta1)
            G.m_abs.mul_(hp.beta1).add_(g[n].abs(), alpha=1.0 - hp.beta1)
            G.v.mul_(hp.beta2).addcmul_(g[n], g[n], value=1.0 - hp.beta2)
            denom = (G.v.sqrt() / state.bc2 ** 0.5).add_(hp.eps)
            delta[n] = (lr / state.bc1) * (G.m / denom)
            G.p.sub_(delta[n])
        # 5. the embedding rows that never see a gradient are AdamW parameters all the same: decoupled decay at the embedding group's lr
        if groups.get("decay") is not None:
            groups["decay"].mul_(1.0 - hp.emb_lr * state.lr_mult * hp.wd)
    # 6. the norm clamp of the added rows runs on every iteration, skipped or not
    norms = None
    if groups.get("added") is not None:
        norms = clamp_rows(groups["added"].p, hp.mean_norm)
    # 7. GradScaler.update()
    if hp.use_scaler:
        if state.found_inf:
            state.scale *= hp.backoff_factor
            state.tracker = 0
        else:
            state.tracker += 1
            if state.tracker == hp.growth_interval:
                state.scale *= hp.growth_factor
                state.tracker = 0
    return {"delta": delta, "added_norms": norms}
