"""CPU reference of image editing (textboost_amd/edit.py, `HipSampler.denoise_from`): diffusers 0.29's
`StableDiffusionImg2ImgPipeline` loop and the latent blend of `StableDiffusionInpaintPipeline` for a 4-channel UNet, in fp32 torch on top of the
oracle's scheduler.  [3P: diffusers is not installed here; restated from its published `get_timesteps`, `prepare_latents` / `add_noise` and the
`(1 - init_mask) * init_latents_proper + init_mask * latents` line of the inpaint loop, as oracle/sampler.py restates the text-to-image loop.]
Only tests import this file."""
import numpy as np
import torch

from oracle.sampler import DPMSolverPP2M


def ref_begin(steps, strength):
    """`get_timesteps`: init_timestep = min(int(steps * strength), steps); t_start = max(steps - init_timestep, 0).  None: no step runs."""
    if not 0.0 < strength <= 1.0:
        raise ValueError(f"strength {strength}")
    begin = max(steps - min(int(steps * strength), steps), 0)
    return begin if begin < steps else None


class EditDPMSolverPP2M(DPMSolverPP2M):
    """the oracle's scheduler started at step `begin` (diffusers' `set_begin_index`): no model output is stored there, so that step is first
    order like step 0; the last step stays first order"""

    def set_begin(self, begin):
        self.begin = begin
        self.step_index = begin
        self.m_prev = None

    def coefficients(self, i):
        begin = getattr(self, "begin", 0)
        if i != begin or i == 0 or i == len(self.timesteps) - 1:
            return super().coefficients(i)
        a0, st0 = self._alpha_sigma(self.sigmas[i])
        a1, st1 = self._alpha_sigma(self.sigmas[i + 1])
        h = (torch.log(a1) - torch.log(st1)) - (torch.log(a0) - torch.log(st0))
        return float(st1 / st0), float(-a1 * (torch.exp(-h) - 1.0)), 0.0

    def noise_scalars(self, i):
        a, s = self._alpha_sigma(self.sigmas[i])
        return float(a), float(s)

    def data_prediction_scalars(self, i):
        a, s = self.noise_scalars(i)
        return (a, s) if self.prediction_type == "epsilon" else (1.0 / a, s / a)


def edit_latents(unet, cond, uncond, z0, noise, strength, steps=25, guidance=7.5, mask=None, **scheduler_kwargs):
    """z0 fp32 [1, 4, h, w] (or [4, h, w]), noise fp32 [B, 4, h, w], mask bool / uint8 [h, w] (true = repaint) or None -> final latents fp32.
    x = a_begin z0 + s_begin noise; steps begin .. steps-1; after step i: x = mask ? x : a_{i+1} z0 + s_{i+1} noise (a select)."""
    sch = EditDPMSolverPP2M(**scheduler_kwargs)
    ts = sch.set_timesteps(steps).tolist()
    begin = ref_begin(steps, strength)
    assert begin is not None
    sch.set_begin(begin)
    z0 = z0.reshape(1, *noise.shape[1:]).float()
    a, s = sch.noise_scalars(begin)
    x = a * z0 + s * noise
    B = x.shape[0]
    ehs = torch.cat([uncond, cond])
    keep = None if mask is None else ~torch.as_tensor(mask).bool()[None, None].expand_as(x)
    for i in range(begin, steps):
        e = unet(torch.cat([x, x]), torch.full((2 * B,), ts[i], dtype=torch.long), ehs)
        eps = e[:B] + guidance * (e[B:] - e[:B])
        x = sch.step(eps, x)
        if keep is not None:
            ka, ks = sch.noise_scalars(i + 1)
            x = torch.where(keep, ka * z0 + ks * noise, x)
    return x


def pool_mask_any(pixel_mask, cell=8):
    """uint8 [H, W] -> uint8 [H / cell, W / cell]: 1 where any pixel of the cell is non-zero (plain loops)"""
    H, W = pixel_mask.shape
    out = np.zeros((H // cell, W // cell), dtype=np.uint8)
    for i in range(H // cell):
        for j in range(W // cell):
            out[i, j] = 1 if pixel_mask[i * cell:(i + 1) * cell, j * cell:(j + 1) * cell].any() else 0
    return out
