"""References of the cross-attention localisation loss (--attn_loss_weight): test infrastructure only.

    coef_ref(target, level)                              g = (1 - m) / max(bg, 1) - m / max(fg, 1) in float64
    attn_loss_terms(q, k, tok_w, g, H, scale)            sum_b sum_s g A of one layer, differentiable, in the dtype of q
    attn_loss_ref(q, k, tok_w, g, H, scale, coef)        (that sum, d(coef * sum)/dq, d(coef * sum)/dk) by autograd, float64 or `dtype`
    attn_loss_grad_formula(q, k, tok_w, g, H, scale, coef)   the same gradients from the closed form, float64
    AttnLossTrainState                                   masked_loss_ref.MaskedTrainState with lambda * L_attn in the step's loss
"""
import torch
import torch.nn.functional as F

import masked_loss_ref as MR
from oracle import train_step as ts


def coef_ref(target, level):
    """target [B, 1, h, w] -> g float64 [B, (h >> level) * (w >> level)]: m = 2^level x 2^level box mean, fg = sum m, bg = sum (1 - m)"""
    f = 1 << level
    B, _, h, w = target.shape
    assert h % f == 0 and w % f == 0
    m = target.double().reshape(B, h // f, f, w // f, f).mean(dim=(2, 4)).reshape(B, -1)
    fg = m.sum(dim=1, keepdim=True)
    bg = (1.0 - m).sum(dim=1, keepdim=True)
    return (1.0 - m) / bg.clamp(min=1.0) - m / fg.clamp(min=1.0)


def attn_loss_terms(q, k, tok_w, g, H, scale):
    """q [B * Sq, H * hd], k [B * Skv, H * hd], tok_w [B, Skv], g [B, Sq] -> sum_b sum_s g[b, s] (1 / H) sum_h sum_j tok_w[b, j] p_{b,h,s,j}"""
    B, Skv = tok_w.shape
    Sq = g.shape[1]
    hd = q.shape[1] // H
    qh = q.reshape(B, Sq, H, hd).permute(0, 2, 1, 3)
    kh = k.reshape(B, Skv, H, hd).permute(0, 2, 1, 3)
    p = torch.softmax(scale * (qh @ kh.transpose(-1, -2)), dim=-1)            # [B, H, Sq, Skv]
    A = (p * tok_w.to(p.dtype)[:, None, None, :]).sum(dim=-1).sum(dim=1) / H   # [B, Sq]
    return (g.to(p.dtype) * A).sum()


def attn_loss_ref(q, k, tok_w, g, H, scale, coef, dtype=torch.float64):
    """-> (sum_b sum_s g A, dq, dk), the gradients those of coef * sum; computed in `dtype` on the operands as they are (already rounded)"""
    qd = q.detach().to(dtype).requires_grad_(True)
    kd = k.detach().to(dtype).requires_grad_(True)
    total = attn_loss_terms(qd, kd, tok_w, g, H, scale)
    dq, dk = torch.autograd.grad(total * coef, [qd, kd])
    return total.detach(), dq, dk


def attn_loss_grad_formula(q, k, tok_w, g, H, scale, coef):
    """ds_j = p_j (coef g_s / H) (tok_w_j - P_J), dq_s = scale sum_j ds_j k_j, dk_j = scale sum_s ds_{s,j} q_s; float64"""
    B, Skv = tok_w.shape
    Sq = g.shape[1]
    hd = q.shape[1] // H
    qh = q.double().reshape(B, Sq, H, hd).permute(0, 2, 1, 3)
    kh = k.double().reshape(B, Skv, H, hd).permute(0, 2, 1, 3)
    p = torch.softmax(scale * (qh @ kh.transpose(-1, -2)), dim=-1)
    tw = tok_w.double()[:, None, None, :]
    PJ = (p * tw).sum(dim=-1, keepdim=True)
    ds = p * (coef * g.double()[:, None, :, None] / H) * (tw - PJ)
    dq = scale * (ds @ kh)
    dk = scale * (ds.transpose(-1, -2) @ qh)
    return dq.permute(0, 2, 1, 3).reshape(B * Sq, H * hd), dk.permute(0, 2, 1, 3).reshape(B * Skv, H * hd)


class AttnLossTrainState(MR.MaskedTrainState):
    """`MaskedTrainState.step` with lambda * L_attn added to the loss.  The supervised layers' q and k come from forward hooks on the oracle UNet's
    `attn2.to_q` / `attn2.to_k` modules; the level of a layer is read off its query count.  Covers the configuration without K/V adapters."""

    def __init__(self, *a, attn_weight, attn_levels, placeholder_ids, **kw):
        super().__init__(*a, **kw)
        assert not self.unet_lora
        self.attn_weight, self.attn_levels, self.placeholder_ids = float(attn_weight), sorted(attn_levels), list(placeholder_ids)
        self._qk = {}
        for name, mod in self.unet.named_modules():
            if name.endswith("attn2.to_q") or name.endswith("attn2.to_k"):
                mod.register_forward_hook(lambda m, i, o, name=name: self._qk.__setitem__(name, o))

    def attn_loss(self, input_ids, target, heads_of):
        """L_attn from the hooks' last forward: target [B, 1, h, w]; heads_of(level) -> head count of that level's layers"""
        B, _, h, w = target.shape
        tok_w = torch.zeros(input_ids.shape, dtype=torch.float32)
        for pid in self.placeholder_ids:
            tok_w += (input_ids == pid).float()
        total, n = 0.0, 0
        for name in sorted(n_ for n_ in self._qk if n_.endswith("to_q")):
            q = self._qk[name]
            k = self._qk[name[:-1] + "k"]
            Sq, C = q.shape[1], q.shape[2]
            level = next(l for l in range(8) if (h >> l) * (w >> l) == Sq)
            if level not in self.attn_levels:
                continue
            H = heads_of(level)
            g = coef_ref(target, level).float()
            total = total + attn_loss_terms(q.reshape(B * Sq, C).float(), k.reshape(B * k.shape[1], C).float(), tok_w, g, H, (C // H) ** -0.5)
            n += 1
        return total / (B * n), n

    def step(self, x0, noise, timesteps, input_ids, prior_input_ids, weight, attn_target, heads_of, attn_weight=None, update=True):
        """attn_weight overrides lambda for this call; update=False returns the losses and gradients without the optimizer step (a probe)"""
        lam = self.attn_weight if attn_weight is None else attn_weight
        cfg, te = self.cfg, self.te
        noisy = ts.add_noise(x0, noise, timesteps, self.acp)
        target = noise if cfg.prediction_type == "epsilon" else ts.get_velocity(x0, noise, timesteps, self.acp)
        params = [te.token_embedding.weight] + self.lora
        B, C = x0.shape[0], x0.shape[1]
        ehs = te(input_ids)
        self._qk.clear()
        pred = self.unet(noisy, timesteps, ehs)
        w = weight.float()
        W = w.sum(dim=(1, 2, 3)).clamp(min=1.0)
        loss_mse = ((w * (pred.float() - target.float()) ** 2).sum(dim=(1, 2, 3)) / (C * W)).sum() / B
        loss_attn, n_layers = self.attn_loss(input_ids, attn_target, heads_of)
        loss = loss_mse + lam * loss_attn
        kp = torch.zeros(())
        if cfg.kpl_weight > 0:
            h = te(prior_input_ids).float()
            with torch.no_grad():
                h0 = self.teacher(prior_input_ids).float()
            kp = (1 - F.cosine_similarity(h, h0, dim=-1)).mean() if cfg.kpl_type == "cos" else F.mse_loss(h, h0, reduction="mean")
            loss = loss + cfg.kpl_weight * kp
        grads = list(torch.autograd.grad(loss, params, allow_unused=True))
        grads = [torch.zeros_like(p) if g is None else g for p, g in zip(params, grads)]
        g_emb, g_lora = grads[0], grads[1:]
        g_emb[: min(self.added)] = 0
        if cfg.mixing is not None:
            for (n, p), g in zip([(n, p) for n, p in te.named_parameters() if "lora_" in n], g_lora):
                if "lora_B" in n:
                    if cfg.mixing == "object":
                        g[1::2, :] = 0
                    else:
                        g[0::2, :] = 0
        gnorm = ts.clip_grad_norm(g_lora, cfg.max_grad_norm)
        out = {"loss": loss.item(), "mse": loss_mse.item(), "attn": float(loss_attn.detach()), "attn_layers": n_layers, "kpl": float(kp.detach()),
               "lora_grad_norm": gnorm.item(), "g_emb_added": g_emb[self.added].clone(), "g_lora": [g.clone() for g in g_lora]}
        self._qk.clear()
        if not update:
            return out
        with torch.no_grad():
            ts.adamw_step([te.token_embedding.weight], [g_emb], self.opt_emb)
            ts.adamw_step(self.lora, g_lora, self.opt_lora)
            tw = te.token_embedding.weight
            rows = tw[self.added]
            vn = rows.norm(dim=-1, keepdim=True)
            scale = torch.minimum(torch.full_like(vn, self.mean_norm), vn)
            tw[self.added] = (scale / vn) * rows
        return out
