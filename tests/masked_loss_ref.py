"""References of the masked training loss (--instance_mask_dir): test infrastructure only.

    weighted_mse(pred, target, weight)                 the loss in float64 torch (differentiable)
    weighted_mse_grad(pred, target, weight, scale)     its gradient in closed form, float64
    pool_ref(mask_u8, x0, y0, h, w, cell, floor)       the mask -> latent-weights arithmetic in numpy float32, operation by operation
    MaskedTrainState                                   oracle.train_step.TrainState with the weighted loss in its step
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import train_step as ts


def weighted_mse(pred, target, weight):
    """loss = (1/B) sum_b [ sum_{c,y,x} w_b (pred - target)^2 / (C max(W_b, 1)) ],  W_b = sum_{y,x} w_b.  pred, target [B, C, h, w],
    weight [B, 1, h, w] >= 0; everything in float64."""
    p, t, w = pred.double(), target.double(), weight.double()
    B, C = p.shape[0], p.shape[1]
    W = w.sum(dim=(1, 2, 3)).clamp(min=1.0)
    per_sample = (w * (p - t) ** 2).sum(dim=(1, 2, 3)) / (C * W)
    return per_sample.sum() / B


def weighted_mse_grad(pred, target, weight, loss_scale=1.0):
    """dpred = loss_scale * 2 w (pred - target) / (B C max(W_b, 1)), float64"""
    p, t, w = pred.double(), target.double(), weight.double()
    B, C = p.shape[0], p.shape[1]
    W = w.sum(dim=(1, 2, 3), keepdim=True).clamp(min=1.0)
    return float(loss_scale) * 2.0 * w * (p - t) / (B * C * W)


def pool_ref(mask_u8, x0, y0, h, w, cell, floor):
    """mask_u8 uint8 [H, W]; the crop [y0, y0 + cell h) x [x0, x0 + cell w) -> float32 [h, w]: with S the integer byte sum of a cell,
    m = fl(fl(S) / fl(255 cell^2)), out = fl(floor + fl(fl(1 - floor) * m)), every operation rounded to float32."""
    crop = np.asarray(mask_u8)[y0:y0 + cell * h, x0:x0 + cell * w]
    assert crop.shape == (cell * h, cell * w), "the crop leaves the image"
    S = crop.astype(np.int64).reshape(h, cell, w, cell).sum(axis=(1, 3))
    m = S.astype(np.float32) / np.float32(255 * cell * cell)
    f = np.float32(floor)
    scale = np.float32(1.0) - f
    out = f + scale * m
    assert m.dtype == np.float32 and out.dtype == np.float32
    return out


class MaskedTrainState(ts.TrainState):
    """`TrainState.step` restated with the weighted loss in place of `F.mse_loss(...).mean()`; the rest of the step (KPL, the row mask, the
    clip, the three AdamW groups, the renormalisation) is the parent's, line for line.  The loss is evaluated in float32 like the parent's."""

    def step(self, x0, noise, timesteps, input_ids, prior_input_ids, weight):
        cfg, te = self.cfg, self.te
        noisy = ts.add_noise(x0, noise, timesteps, self.acp)
        target = noise if cfg.prediction_type == "epsilon" else ts.get_velocity(x0, noise, timesteps, self.acp)
        params = [te.token_embedding.weight] + self.lora + self.unet_lora
        B, C = x0.shape[0], x0.shape[1]
        ehs = te(input_ids)
        pred = self.unet(noisy, timesteps, ehs)
        w = weight.float()
        W = w.sum(dim=(1, 2, 3)).clamp(min=1.0)
        loss_mse = ((w * (pred.float() - target.float()) ** 2).sum(dim=(1, 2, 3)) / (C * W)).sum() / B
        loss = loss_mse
        kp = torch.zeros(())
        if cfg.kpl_weight > 0:
            h = te(prior_input_ids).float()
            with torch.no_grad():
                h0 = self.teacher(prior_input_ids).float()
            kp = (1 - F.cosine_similarity(h, h0, dim=-1)).mean() if cfg.kpl_type == "cos" else F.mse_loss(h, h0, reduction="mean")
            loss = loss + cfg.kpl_weight * kp
        grads = list(torch.autograd.grad(loss, params, allow_unused=True))
        grads = [torch.zeros_like(p) if g is None else g for p, g in zip(params, grads)]
        g_emb, g_lora, g_unet = grads[0], grads[1:1 + len(self.lora)], grads[1 + len(self.lora):]
        g_emb[: min(self.added)] = 0
        if cfg.mixing is not None:
            for (n, p), g in zip([(n, p) for n, p in te.named_parameters() if "lora_" in n], g_lora):
                if "lora_B" in n:
                    if cfg.mixing == "object":
                        g[1::2, :] = 0
                    else:
                        g[0::2, :] = 0
        gnorm = ts.clip_grad_norm(g_lora, cfg.max_grad_norm)
        with torch.no_grad():
            ts.adamw_step([te.token_embedding.weight], [g_emb], self.opt_emb)
            ts.adamw_step(self.lora, g_lora, self.opt_lora)
            if self.unet_lora:
                ts.adamw_step(self.unet_lora, g_unet, self.opt_unet)
            tw = te.token_embedding.weight
            rows = tw[self.added]
            vn = rows.norm(dim=-1, keepdim=True)
            scale = torch.minimum(torch.full_like(vn, self.mean_norm), vn)
            tw[self.added] = (scale / vn) * rows
        return {"loss": loss.item(), "mse": loss_mse.item(), "kpl": float(kp.detach()), "lora_grad_norm": gnorm.item(),
                "g_emb_added": g_emb[self.added].clone(), "g_lora": [g.clone() for g in g_lora], "g_unet": [g.clone() for g in g_unet]}
