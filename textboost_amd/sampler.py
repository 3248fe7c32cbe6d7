"""Validation / inference sampling on MI355X -- the device work of the reference's `log_validation` (train_textboost.py:453-531) and
`inference.py:73-100`: diffusers `StableDiffusionPipeline.__call__` with `DPMSolverMultistepScheduler`, 25 steps, guidance 7.5.
SURVEY.md 8(f) row 2.

    ids (prompt, empty prompt) -> text encoder -> [classifier-free guidance: UNet on (x, x) with (uncond, cond)] x steps
    -> DPM-Solver++(2M) update -> VAE decoder -> image in [0, 1]

The UNet forward, the text encoder and the VAE decoder are the executors of this package; the per-step scalar coefficients of the solver
are host arithmetic (`DPMSolverPP2M`, float64, computed once per schedule), the update itself is one elementwise kernel (`tb_dpm_step`).
Nothing here synchronises with the host, so the whole loop can be captured in a HIP graph.

`HipSampler.denoise_from` is the same loop started mid-schedule from the latents of an encoded photo (image editing, edit.py): with a mask the
update and the per-step select of the kept cells are one launch as well (`tb_dpm_step_blend`), so editing launches what text-to-image does.

`HipSampler.invert` walks an encoded photo UP the schedule (DDIM inversion, one `tb_invert_step` per level) and returns the trajectory;
`denoise(p2p=..., pin=trajectory)` then keeps the source rows of a prompt-to-prompt edit on it (`tb_dpm_step_pin`), so the source image is
the photo and the edited rows inherit its layout (inference.py --invert-image).

`HipSampler.denoise_canvas` denoises a latent larger than the UNet's square as overlapping model-sized windows (MultiDiffusion): per step
`tb_canvas_gather` and the UNet per chunk of windows, then one `tb_canvas_step` on the whole canvas (inference.py --width / --height,
DESIGN.md 24).
"""
from __future__ import annotations

import math
from typing import List, Optional, Tuple

import torch

from . import ops
from . import _lib as L


class DPMSolverPP2M:
    """diffusers DPMSolverMultistepScheduler as `from_config(pipeline.scheduler.config)` builds it (train_textboost.py:493-495): algorithm
    "dpmsolver++", solver_order 2, solver_type "midpoint", final sigma zero (last step first order), and -- inherited from the model's own
    scheduler config (`<model>/scheduler/scheduler_config.json`; a PNDMScheduler for SD1.x / SD2.1-base, a DDIMScheduler for SD2.1-768) --
    the betas, `prediction_type` ("epsilon" | "v_prediction"), `timestep_spacing` and `steps_offset`.  PNDM / DDIM instances carry
    timestep_spacing "leading" (their class default) and SD's files say steps_offset 1, so that is the default when no file exists.
    sigma = sqrt((1 - abar) / abar); alpha_t = 1 / sqrt(sigma^2 + 1); sigma_t = sigma alpha_t; lambda = log(alpha_t / sigma_t).
    [3P: diffusers 0.29 is not installed here; the three spacings are restated from its set_timesteps.]"""

    def __init__(self, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                 prediction_type="epsilon", timestep_spacing="leading", steps_offset=1):
        if beta_schedule == "scaled_linear":
            betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
        elif beta_schedule == "linear":
            betas = torch.linspace(beta_start, beta_end, num_train_timesteps, dtype=torch.float32)
        else:
            raise NotImplementedError(f"beta_schedule {beta_schedule}")
        if prediction_type not in ("epsilon", "v_prediction"):
            raise NotImplementedError(f"prediction_type {prediction_type}")
        if timestep_spacing not in ("linspace", "leading", "trailing"):
            raise ValueError(f"timestep_spacing {timestep_spacing}")
        self.alphas_cumprod = torch.cumprod(1.0 - betas, dim=0).double()
        self.T = num_train_timesteps
        self.prediction_type, self.timestep_spacing, self.steps_offset = prediction_type, timestep_spacing, int(steps_offset)
        self.init_noise_sigma = 1.0

    @classmethod
    def from_config(cls, cfg: Optional[dict]):
        """cfg = the parsed scheduler_config.json of the model (None: SD1.x's values)."""
        cfg = cfg or {}
        return cls(num_train_timesteps=cfg.get("num_train_timesteps", 1000), beta_start=cfg.get("beta_start", 0.00085),
                   beta_end=cfg.get("beta_end", 0.012), beta_schedule=cfg.get("beta_schedule", "scaled_linear"),
                   prediction_type=cfg.get("prediction_type", "epsilon"), timestep_spacing=cfg.get("timestep_spacing", "leading"),
                   steps_offset=cfg.get("steps_offset", 1))

    def set_timesteps(self, n: int) -> List[int]:
        T = self.T  # last_timestep (lambda_min_clipped = -inf: nothing is clipped)
        if self.timestep_spacing == "linspace":
            ts = torch.linspace(0, T - 1, n + 1, dtype=torch.float64).round().flip(0)[:-1].long()
        elif self.timestep_spacing == "leading":
            ratio = T // (n + 1)
            ts = (torch.arange(0, n + 1, dtype=torch.float64) * ratio).round().flip(0)[:-1].long() + self.steps_offset
        else:  # trailing
            ts = torch.arange(T, 0, -T / n, dtype=torch.float64).round().long() - 1
        ac = self.alphas_cumprod[ts]
        self.timesteps = ts.tolist()
        self.sigmas = ((1 - ac) / ac).sqrt().tolist() + [0.0]
        return self.timesteps

    @staticmethod
    def alpha_sigma(sigma: float) -> Tuple[float, float]:
        a = 1.0 / math.sqrt(sigma * sigma + 1.0)
        return a, sigma * a

    def data_prediction_scalars(self, i: int) -> Tuple[float, float]:
        """(a, s) such that the data prediction of step i is m0 = (x - s * model_output) / a -- the form `tb_dpm_step` evaluates.
        epsilon: m0 = (x - sigma_t eps) / alpha_t;  v_prediction: m0 = alpha_t x - sigma_t v = (x - (sigma_t / alpha_t) v) / (1 / alpha_t)."""
        a_t, s_t = self.alpha_sigma(self.sigmas[i])
        return (a_t, s_t) if self.prediction_type == "epsilon" else (1.0 / a_t, s_t / a_t)

    def noise_scalars(self, i: int) -> Tuple[float, float]:
        """(alpha, sigma) of `add_noise` at the start of step i: x_i = alpha z0 + sigma noise.  i = len(timesteps) (past the last step): (1, 0)."""
        return self.alpha_sigma(self.sigmas[i])

    def inversion_scalars(self, k: int) -> Tuple[float, float]:
        """(cx, ce) of the inversion step that takes x on level k+1 to level k = steps-1 .. 0 (level j is `noise_scalars(j)`, level `steps` the
        clean latent) with the model evaluated at timesteps[k] ON THAT x -- DDIM inversion in the convention of the published
        prompt-to-prompt / null-text code:  m = (x - sigma_{k+1} eps) / alpha_{k+1};  x_k = alpha_k m + sigma_k eps = cx x + ce eps.  For a
        fixed eps this is the algebraic inverse of the solver's first-order step `coefficients(k, begin=k)` (and of the final step)."""
        if self.prediction_type != "epsilon":
            raise NotImplementedError(
                f"inversion of a {self.prediction_type} model is not built: a v output would have to be converted to a noise prediction with the "
                "scalars of the level its input is on, and in an inversion step the input is one level off the timestep the model is asked about "
                "(SD1.x and SD2.1-base are epsilon models)")
        if not 0 <= k < len(self.timesteps):
            raise IndexError(f"inversion step {k}: the schedule has steps 0 .. {len(self.timesteps) - 1}")
        a_k, s_k = self.noise_scalars(k)
        a_n, s_n = self.noise_scalars(k + 1)
        return a_k / a_n, s_k - a_k * s_n / a_n

    def coefficients(self, i: int, begin: int = 0) -> Tuple[float, float, float]:
        """x_next = ca x + cb m0 + cc m_prev  for step i  (m = data prediction).  begin: the first step that runs (image editing starts
        mid-schedule, `HipSampler.denoise_from`): it has no model-output history and is first order, as step 0 is."""
        a0, st0 = self.alpha_sigma(self.sigmas[i])
        a1, st1 = self.alpha_sigma(self.sigmas[i + 1])
        if i == len(self.timesteps) - 1:      # sigma_next = 0: exp(-h) = 0, alpha_next = 1
            return 0.0, a1, 0.0
        lam0, lam1 = math.log(a0 / st0), math.log(a1 / st1)
        h = lam1 - lam0
        e = math.expm1(-h)
        ca = st1 / st0
        if i == begin:
            return ca, -a1 * e, 0.0
        ap, stp = self.alpha_sigma(self.sigmas[i - 1])
        r0 = (lam0 - math.log(ap / stp)) / h
        return ca, -a1 * e * (1.0 + 0.5 / r0), a1 * e * (0.5 / r0)


class DDPMAncestral:
    """--validation_scheduler DDPMScheduler (train_textboost.py:341-345, :483-495): diffusers DDPMScheduler built from the model's scheduler config
    with variance_type "fixed_small" -- SD's betas, clip_sample false, timestep_spacing "leading" (timesteps arange(n) * (T // n), reversed,
    + steps_offset), the ancestral step  x_prev = c_x0 x0 + c_x x + sqrt(var) z.  In `tb_dpm_step`'s form (x = ca x + cb m0 + cc m_prev, m0 the
    data prediction) the variance noise z rides in the m_prev operand: (ca, cb, cc) = (c_x, c_x0, sqrt(var)).  [3P restated]"""

    def __init__(self, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", prediction_type="epsilon",
                 steps_offset=1):
        if beta_schedule == "scaled_linear":
            betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
        elif beta_schedule == "linear":
            betas = torch.linspace(beta_start, beta_end, num_train_timesteps, dtype=torch.float32)
        else:
            raise NotImplementedError(f"beta_schedule {beta_schedule}")
        if prediction_type not in ("epsilon", "v_prediction"):
            raise NotImplementedError(f"prediction_type {prediction_type}")
        self.alphas_cumprod = torch.cumprod(1.0 - betas, dim=0).double()
        self.T, self.prediction_type, self.steps_offset = num_train_timesteps, prediction_type, int(steps_offset)
        self.init_noise_sigma = 1.0
        self.needs_noise = True

    @classmethod
    def from_config(cls, cfg: Optional[dict]):
        cfg = cfg or {}
        if cfg.get("clip_sample", False):
            raise NotImplementedError("DDPMScheduler with clip_sample = true (SD's scheduler configs say false)")
        return cls(num_train_timesteps=cfg.get("num_train_timesteps", 1000), beta_start=cfg.get("beta_start", 0.00085),
                   beta_end=cfg.get("beta_end", 0.012), beta_schedule=cfg.get("beta_schedule", "scaled_linear"),
                   prediction_type=cfg.get("prediction_type", "epsilon"), steps_offset=cfg.get("steps_offset", 1))

    def set_timesteps(self, n: int) -> List[int]:
        self.n = n
        self.timesteps = ((torch.arange(0, n, dtype=torch.float64) * (self.T // n)).round().flip(0).long() + self.steps_offset).tolist()
        return self.timesteps

    def data_prediction_scalars(self, i: int) -> Tuple[float, float]:
        ab = float(self.alphas_cumprod[self.timesteps[i]])
        a_t, s_t = math.sqrt(ab), math.sqrt(1.0 - ab)
        return (a_t, s_t) if self.prediction_type == "epsilon" else (1.0 / a_t, s_t / a_t)

    def coefficients(self, i: int) -> Tuple[float, float, float]:
        t = self.timesteps[i]
        prev_t = t - self.T // self.n
        ab_t = float(self.alphas_cumprod[t])
        ab_p = float(self.alphas_cumprod[prev_t]) if prev_t >= 0 else 1.0
        alpha = ab_t / ab_p
        beta = 1.0 - alpha
        var = max((1.0 - ab_p) / (1.0 - ab_t) * beta, 1e-20)
        return math.sqrt(alpha) * (1.0 - ab_p) / (1.0 - ab_t), math.sqrt(ab_p) * beta / (1.0 - ab_t), (math.sqrt(var) if t > 0 else 0.0)


class HipSampler:
    """`sample(cond_ehs, uncond_ehs, latents=None) -> images [B,3,8h,8w] in [0,1]`.  `unet` must be built for batch 2B (guidance runs the
    unconditional and conditional rows in one call, as the pipeline does), `vae_decoder` for batch B."""

    def __init__(self, unet, vae_decoder, steps: int = 25, guidance: float = 7.5, scheduler_config: Optional[dict] = None,
                 scheduler: str = "DPMSolverMultistepScheduler"):
        assert unet.B == 2 * vae_decoder.B and unet.H == vae_decoder.h and unet.W == vae_decoder.w
        self.unet, self.vae, self.steps, self.g = unet, vae_decoder, steps, guidance
        self.B = vae_decoder.B
        if scheduler == "DPMSolverMultistepScheduler":
            self.sch = DPMSolverPP2M.from_config(scheduler_config)
        elif scheduler == "DDPMScheduler":  # --validation_scheduler DDPMScheduler (:341-345)
            self.sch = DDPMAncestral.from_config(scheduler_config)
        else:
            raise ValueError(f"validation scheduler {scheduler}")
        self.timesteps = self.sch.set_timesteps(steps)
        dev = unet.dev
        B, h, w = self.B, unet.H, unet.W
        self.x = torch.zeros(B, 4, h, w, device=dev)
        self.m_prev = torch.zeros(B, 4, h, w, device=dev)
        self.x2 = torch.zeros(2 * B, 4, h, w, device=dev, dtype=L.half_dtype())
        self.t_dev = [torch.full((2 * B,), t, dtype=torch.int64, device=dev) for t in self.timesteps]
        self.generator: Optional[torch.Generator] = None

    def denoise(self, cond_ehs, uncond_ehs, latents=None, step_noise=None, maps=None, regions=None, region_steps=None, p2p=None, pin=None,
                pin_mask=None, excite=None, blend=None):
        """cond / uncond: fp16 or fp32 [B*77, D] text-encoder outputs.  Returns the final latents fp32 [B,4,h,w].
        step_noise (ancestral schedulers only): one [B,4,h,w] tensor per step instead of drawing from `self.generator`.
        maps: an `attn_maps.AttnMapRecorder` of this UNet (rows [B, 2B): the conditional half); it is zeroed here and records every step.
        regions: a `regions.RegionSet` of this UNet; the first `region_steps` executed steps (default: all) run the region-masked
        cross-attention, the others the plain one.
        p2p: a `p2p.P2PControl` of this UNet (DPM-Solver++ only).  Rows [0, B/2) are then the source images and [B/2, B) the edited ones (the
        caller gives both halves the same latents); steps i < floor(cross_steps * steps) run the controlled cross-attention and steps
        i < floor(self_steps * steps) the controlled self-attention of the edited conditional rows, every other row stays plain.  Not with
        `maps` (the recorder recomputes an uncontrolled softmax) or `regions` (both take over the edited rows' cross-attention): ValueError.
        pin: fp32 [steps+1, 4, h, w], one photo's trajectory from `invert` (needs `p2p`; `latents` must be None).  All rows start from pin[0];
        step i is one `tb_dpm_step_pin` launch that puts the source rows [0, B/2) on pin[i+1], so they end as pin[steps] = z0 exactly, while
        the edited rows take the solver's step.  pin_mask: uint8 [h, w] (non-zero = repaint; needs `pin`): the edited rows' cells outside it
        stay on the trajectory as well and end as z0.  Without `pin` the method launches what it launched before.
        excite: an `excite.ExciteControl` of this UNet (Attend-and-Excite; both schedulers: it acts before the step).  Every step
        i < floor(excite_steps * steps) first runs the excite pass on the current latents -- a truncated UNet forward of the usual
        (uncond | cond) batch, `excite_loss`, `backward_sample`, `excite_update` with step scale * sqrt(1 - 0.5 i / (steps - 1)) -- and then the
        unchanged guided step.  At the steps {0, floor(0.2 steps), floor(0.4 steps)} (unless refine is off) the pass repeats, at most max_refine
        times, until every image's loss is below {0.05, 0.5, 0.8}: the one place where the host reads the [B] losses; an image already
        below gets step 0.  A non-finite gradient skips that image's update and is counted in `excite.skipped`, never raised.
        `excite.trace` holds one entry per guided step.  Not with `maps`, `regions`, `p2p` or `pin`: ValueError.  Without `excite` the method
        launches what it launched before.
        blend: a `local_blend.BlendControl` of this UNet (prompt-to-prompt LocalBlend; needs `p2p`).  Every step's forward adds
        the conditional rows' level-2 cross-attention maps to an accumulator (zeroed here).  Steps i < floor(blend.start * steps) run the step
        launch they run without it; from there on a step is `tb_blend_mask` (the accumulator, step i's forward included -> one mask per pair)
        and ONE `tb_dpm_step_local_blend`: x_edit = mask ? x_edit : x_src, x_src the source row after the same step.  With `pin` (one pair):
        `tb_blend_mask(limit = pin_mask)`, then the usual `tb_dpm_step_pin` with that mask in `pin_mask`'s place.  No host synchronisation.
        `blend.final_mask` / `blend.area` are the last step's masks on the device (None when no step blended); `blend.keep_masks` keeps every
        step's in `blend.masks`.  Not without `p2p`, not with `maps`, `regions` or `excite`: ValueError.  `unet.blend` is set during the call
        only; without `blend` the method launches what it launched before."""
        B, sch = self.B, self.sch
        bl_start = self._blend_start(blend, p2p, maps, regions, excite, pin)
        ex_steps = self._excite_steps(excite, maps, regions, p2p, pin)
        p2p_cross, p2p_self = self._p2p_steps(p2p, maps, regions)
        region_steps = self._region_steps(regions, region_steps, self.steps)
        pin, pin_mask = self._pin_args(pin, pin_mask, p2p, latents)
        if p2p is not None:
            p2p.reset()
        if maps is not None:
            maps.zero()
        bl = None
        if blend is not None:
            bl = self._blend_bufs
            bl.words.copy_(blend.table)
            bl.acc.zero_()
            blend.final_mask = blend.area = None
            blend.masks = torch.zeros((self.steps,) + tuple(bl.mask.shape), dtype=torch.uint8, device=self.x.device) if blend.keep_masks else None
        if pin is not None:
            self.x.copy_(pin[0].expand_as(self.x))
        else:
            if latents is None:
                latents = torch.randn(self.x.shape, device=self.x.device, generator=self.generator)
            self.x.copy_(latents * sch.init_noise_sigma)
        self.m_prev.zero_()
        self.x2[:B].copy_(self.x)
        self.x2[B:].copy_(self.x)
        ehs = torch.cat([uncond_ehs, cond_ehs]).to(L.half_dtype()).contiguous()
        n = self.x[0].numel()
        hw = self.x.shape[2] * self.x.shape[3]
        for i in range(self.steps):
            if i < ex_steps:
                self._excite_pass(i, ehs, excite)
            if bl is None:
                eps2 = self._unet_forward(i, ehs, maps, regions if i < region_steps else None, p2p, i < p2p_cross, i < p2p_self)
            else:   # the same forward; its level-2 cross-attention layers also record the conditional rows' maps
                self.unet.blend, bl.record = bl, True
                try:
                    eps2 = self._unet_forward(i, ehs, None, None, p2p, i < p2p_cross, i < p2p_self)
                finally:
                    self.unet.blend, bl.record = None, False
            a_t, s_t = sch.data_prediction_scalars(i)
            ca, cb, cc = sch.coefficients(i)
            blending = bl is not None and i >= bl_start
            if blending:
                ops.blend_mask(bl.acc, bl.words, self.x.shape[2], self.x.shape[3], bl.h, bl.w, blend.threshold, bl.mask, limit=pin_mask, area=bl.area)
                if blend.masks is not None:
                    blend.masks[i].copy_(bl.mask)
                blend.final_mask, blend.area = bl.mask, bl.area
            if pin is not None:
                ops.dpm_step_pin(self.x, eps2, self.m_prev, self.x2, n, B, self.g, a_t, s_t, ca, cb, cc, pin[i + 1], B // 2,
                                 bl.mask if blending else pin_mask, hw)
                continue
            if blending:
                ops.dpm_step_local_blend(self.x, eps2, self.m_prev, self.x2, n, B, self.g, a_t, s_t, ca, cb, cc, bl.mask, hw)
                continue
            if getattr(sch, "needs_noise", False):  # the variance noise of the ancestral step rides in the m_prev operand
                if step_noise is not None:
                    self.m_prev.copy_(step_noise[i])
                else:
                    self.m_prev.normal_(generator=self.generator)
            ops.dpm_step(self.x, eps2, self.m_prev, self.x2, n, B, self.g, a_t, s_t, ca, cb, cc)
        if ex_steps:
            self._excite_finish(excite)
        return self.x

    # ------------------------------------------------------------------ MultiDiffusion canvas (canvas.py)
    def denoise_canvas(self, cond_ehs, uncond_ehs, latents, stride=None, keep_trace=False):
        """Wide and tall images: latents fp32 [n, 4, Hc, Wc] (Hc, Wc >= the UNet's S) are denoised as overlapping S x S windows at `stride`
        cells (default S // 4), `canvas.CanvasPlan(S, Hc, Wc, stride, n, B)`: the image-window pairs run through the UNet B at a time, at the
        batch 2B and the size it is built for.  cond / uncond: [B*77, D] as in `denoise`; all images and windows share the one prompt.
        Per step and chunk: `tb_canvas_gather` (the chunk's crops -> x2; a ragged last chunk repeats its last pair), the UNet forward of
        `denoise`, a copy of its output into eps_all; then ONE `tb_canvas_step`, which averages the windows' guided eps where they overlap
        and takes the solver's step on the canvas, `m_prev` kept on the canvas (the update is linear, so this equals stepping every window
        and averaging the results).  From the second step on the crops are copies of the step's own 16-bit canvas, which carries
        `tb_dpm_step`'s conversion: at Hc == Wc == S the UNet sees what `denoise` shows it and the result has `denoise`'s bits.
        No host synchronisation (capturable).  keep_trace: `self.canvas_trace` fp32 [steps+1, n, 4, Hc, Wc] = the canvas before step 0 and
        after every step, `self.canvas_trace_h` the 16-bit canvases beside it (entry 0 unused: step 0 converts the fp32 canvas).
        DPM-Solver++ only.  Returns the final canvas fp32 [n, 4, Hc, Wc] (a new tensor)."""
        from .canvas import CanvasPlan
        sch, unet = self.sch, self.unet
        if not isinstance(sch, DPMSolverPP2M):
            raise NotImplementedError(f"the canvas runs on the DPM-Solver++ scheduler only, not on {type(sch).__name__}")
        if unet.H != unet.W:
            raise ValueError(f"the canvas takes square windows; the UNet is built for {unet.H} x {unet.W}")
        S = unet.H
        if not torch.is_tensor(latents) or latents.dtype != torch.float32 or latents.dim() != 4 or latents.shape[1] != 4:
            raise ValueError(f"latents {getattr(latents, 'dtype', type(latents).__name__)} {tuple(getattr(latents, 'shape', ()))}: expected "
                             "float32 [n, 4, Hc, Wc]")
        n, _, Hc, Wc = latents.shape
        key = (Hc, Wc, max(1, S // 4) if stride is None else stride, n)
        plans = self.__dict__.setdefault("_canvas_plans", {})
        if key not in plans:      # kept with their device tables: a repeated call uploads nothing (graph capture)
            plans[key] = CanvasPlan(S, Hc, Wc, key[2], n, self.B)       # (CanvasError: a ValueError)
        plan = plans[key]
        dev, half = self.x.device, L.half_dtype()
        plan.tables(dev)
        x = torch.empty(n, 4, Hc, Wc, device=dev)
        m_prev = torch.zeros_like(x)
        xh = torch.empty(n, 4, Hc, Wc, device=dev, dtype=half)
        eps_all = torch.empty((plan.n_chunks,) + tuple(self.x2.shape), device=dev, dtype=half)
        x.copy_(latents * sch.init_noise_sigma)
        self.canvas_plan = plan
        self.canvas_trace = self.canvas_trace_h = None
        if keep_trace:
            self.canvas_trace = torch.empty((self.steps + 1,) + tuple(x.shape), device=dev)
            self.canvas_trace_h = torch.zeros((self.steps + 1,) + tuple(x.shape), device=dev, dtype=half)
            self.canvas_trace[0].copy_(x)
        ehs = torch.cat([uncond_ehs, cond_ehs]).to(half).contiguous()
        for i in range(self.steps):
            for c in range(plan.n_chunks):
                ops.canvas_gather(x, self.x2, plan, c, xh=xh if i else None)
                eps_all[c].copy_(unet.forward(self.x2, self.t_dev[i], ehs))
            a_t, s_t = sch.data_prediction_scalars(i)
            ca, cb, cc = sch.coefficients(i)
            ops.canvas_step(x, eps_all, m_prev, plan, self.g, a_t, s_t, ca, cb, cc, xh=xh)
            if keep_trace:
                self.canvas_trace[i + 1].copy_(x)
                self.canvas_trace_h[i + 1].copy_(xh)
        return x

    # ------------------------------------------------------------------ prompt-to-prompt LocalBlend (local_blend.py)
    def _blend_start(self, blend, p2p, maps, regions, excite, pin):
        """the first step of `denoise` whose launch blends; every refusal, before anything is touched.  Allocates the recorder's buffers on
        first use (`HipUNet.enable_blend`); they stay with the sampler, and `unet.blend` is set only while `denoise` runs."""
        if blend is None:
            return None
        from .local_blend import start_step
        if p2p is None:
            raise ValueError("blend without p2p: LocalBlend blends the edited rows of a prompt-to-prompt pair against their source rows")
        for name, given in (("maps", maps), ("regions", regions), ("excite", excite)):
            if given is not None:
                raise ValueError(f"LocalBlend does not go with {name} (prompt-to-prompt, which it needs, does not either)")
        unet = self.unet
        if 2 * blend.n != self.B or blend.T != unet.T or (blend.h, blend.w) != (unet.H, unet.W):
            raise ValueError(f"the blend control is built for {blend.n} pairs, {blend.T} tokens and a {blend.h} x {blend.w} grid; the sampler "
                             f"runs {self.B} rows, {unet.T} tokens, {unet.H} x {unet.W}")
        if pin is not None and self.B != 2:
            raise ValueError(f"blend with pin takes one pair (the pinned step's mask is shared by the rows), not {self.B // 2}")
        start = start_step(blend.start, self.steps)
        bl = getattr(self, "_blend_bufs", None)
        if bl is None or bl.n_pos != blend.n_pos:
            prev = unet.blend
            try:
                bl = unet.enable_blend(n_pos=blend.n_pos)   # (NotImplementedError for an fp32 UNet, ValueError without level-2 cross-attention)
            finally:
                unet.blend = prev
            self._blend_bufs = bl
        if tuple(bl.words.shape) != tuple(blend.table.shape):
            raise ValueError(f"the blend control's table is {tuple(blend.table.shape)}; the sampler needs {tuple(bl.words.shape)}")
        return start

    @property
    def blend_buffers(self):
        """the recorder's buffers of the last `denoise(blend=)` (`HipUNet.enable_blend`'s namespace: acc, words, mask, area, layers, ...);
        None before the first"""
        return getattr(self, "_blend_bufs", None)

    def forward_step(self, i, ehs, p2p=None, p2p_cross=False, p2p_self=False):
        """the UNet call of step i of `denoise` on the sampler's current `x2`, as `denoise` issues it (tests replay a generation with it)"""
        return self._unet_forward(i, ehs, None, None, p2p, p2p_cross, p2p_self)

    # ------------------------------------------------------------------ Attend-and-Excite (excite.py)
    def _excite_steps(self, excite, maps, regions, p2p, pin):
        """how many steps of `denoise` run the excite pass; every refusal, before anything is touched.  Writes the control's tables into the
        UNet's (enable_excite() on first use)."""
        if excite is None:
            return 0
        from .excite import guided_steps
        for name, given in (("maps", maps), ("regions", regions), ("p2p", p2p), ("pin", pin)):
            if given is not None:
                raise ValueError(f"Attend-and-Excite does not go with {name}: the excite pass runs its own forward of the UNet and moves the "
                                 f"latents between the steps, which {name} does not account for")
        unet = self.unet
        if excite.n != self.B or excite.T != unet.T or (excite.h, excite.w) != (unet.H, unet.W):
            raise ValueError(f"the excite control is built for {excite.n} images, {excite.T} tokens and a {excite.h} x {excite.w} grid; the sampler "
                             f"runs {self.B} images, {unet.T} tokens, {unet.H} x {unet.W}")
        if unet.excite is None:
            unet.enable_excite()
        ex = unet.excite
        if (ex.b0, ex.nb) != (self.B, self.B) or tuple(ex.words.shape) != tuple(excite.table.shape):
            raise ValueError(f"the UNet's excite buffers hold rows [{ex.b0}, {ex.b0 + ex.nb}) and a {tuple(ex.words.shape)} word table; the "
                             f"sampler needs rows [{self.B}, {2 * self.B}) and {tuple(excite.table.shape)}")
        ex.words.copy_(excite.table)
        ex.last.copy_(excite.last)
        if getattr(self, "_ex_step", None) is None:
            self._ex_step = torch.zeros(self.B, device=self.x.device)
            self._ex_bad = torch.zeros(self.B, dtype=torch.int32, device=self.x.device)
        excite.trace, excite.skipped = [], 0
        self._ex_pending = []
        return guided_steps(excite.excite_steps, self.steps)

    def _excite_pass(self, i, ehs, ctl):
        """the excite pass of step i on the current latents (x, x2), in front of the guided step"""
        from .excite import refine_thresholds, step_size
        unet, B = self.unet, self.B
        ex = unet.excite
        base = step_size(ctl.scale, i, self.steps)
        thr = refine_thresholds(self.steps).get(i) if ctl.refine else None
        entry = dict(step=i, step_size=base, threshold=thr, iterations=1, loss_before=None, loss_after=None, word=None, skipped=0)
        ctl.trace.append(entry)

        def evaluate():
            unet.forward(self.x2, self.t_dev[i], ehs, until="excite")
            unet.excite_loss(ctl.loss_scale)

        def update():
            g = unet.backward_sample()[B:]
            ops.excite_update(self.x, g, self._ex_step, self.x2, self._ex_bad, ctl.loss_scale)
            self._ex_pending.append((entry, "skipped", self._ex_bad.clone()))

        evaluate()
        if thr is None:   # nothing is read back: the figures of the trace are collected behind the last step
            self._ex_pending.append((entry, "loss_before", ex.loss.clone()))
            self._ex_pending.append((entry, "word", ex.word.clone()))
            self._ex_step.fill_(base)
            update()
            return
        k = 0
        while True:
            losses = ex.loss.tolist()
            if k == 0:
                entry["loss_before"], entry["word"] = losses, ex.word.tolist()
            entry["loss_after"], entry["iterations"] = losses, k
            if k == ctl.max_refine or all(l < thr for l in losses):
                return
            self._ex_step.copy_(torch.tensor([base if l >= thr else 0.0 for l in losses], dtype=torch.float32))
            update()
            k += 1
            evaluate()

    def _excite_finish(self, ctl):
        """one read-back behind the last step: the losses, worst words and skipped updates the guided steps left on the device"""
        for entry, key, t in self._ex_pending:
            v = t.tolist()
            if key == "skipped":
                entry["skipped"] += int(sum(v))
                ctl.skipped += int(sum(v))
            else:
                entry[key] = v
        self._ex_pending = []

    def invert(self, cond_ehs, uncond_ehs, z0, guidance: float = 1.0):
        """DDIM inversion of encoded photos: z0 fp32 [B, 4, h, w], or [1, 4, h, w] / [4, h, w] shared by the B rows -> the
        trajectory fp32 [steps+1, B, 4, h, w] (a new tensor): traj[steps] = z0, traj[k] = the latents on level k (`noise_scalars(k)`), traj[0]
        the noise `denoise` starts from.  Step k = steps-1 .. 0 evaluates the UNet at timesteps[k] on the latents of level k+1 and applies
        `DPMSolverPP2M.inversion_scalars(k)` in one `tb_invert_step` launch: `steps` UNet forwards, `steps` launches, no host synchronisation
        (capturable).  cond / uncond describe the photo; guidance 1 is the conditional prediction alone, the usual choice for inversion.
        DPM-Solver++ on an epsilon model only; every refusal comes before anything is touched."""
        B, sch, steps = self.B, self.sch, self.steps
        if not isinstance(sch, DPMSolverPP2M):
            raise NotImplementedError(f"inversion runs on the DPM-Solver++ scheduler only, not on {type(sch).__name__}")
        scalars = [sch.inversion_scalars(k) for k in range(steps)]          # (v-prediction: NotImplementedError)
        g = float(guidance)
        if not (math.isfinite(g) and g >= 0.0):
            raise ValueError(f"inversion guidance {guidance}: a finite number >= 0")
        if not torch.is_tensor(z0) or z0.dtype != torch.float32:
            raise ValueError(f"z0 {getattr(z0, 'dtype', type(z0).__name__)}: expected an fp32 tensor")
        shape = tuple(self.x.shape)
        if tuple(z0.shape) not in (shape, (1,) + shape[1:], shape[1:]):
            raise ValueError(f"z0 {tuple(z0.shape)}: the sampler is built for {shape} (or one {shape[1:]} shared by the rows)")
        traj = torch.empty((steps + 1,) + shape, dtype=torch.float32, device=self.x.device)
        traj[steps].copy_(z0.to(self.x.device).reshape((-1,) + shape[1:]).expand(shape))
        self.x.copy_(traj[steps])
        self.x2[:B].copy_(self.x)
        self.x2[B:].copy_(self.x)
        ehs = torch.cat([uncond_ehs, cond_ehs]).to(L.half_dtype()).contiguous()
        n = self.x[0].numel()
        for k in range(steps - 1, -1, -1):
            eps2 = self.unet.forward(self.x2, self.t_dev[k], ehs)
            cx, ce = scalars[k]
            ops.invert_step(self.x, eps2, self.x2, traj[k], n, B, g, cx, ce)
        return traj

    def _pin_args(self, pin, pin_mask, p2p, latents):
        """`denoise(pin=..., pin_mask=...)`: every refusal, before anything is touched.  -> (pin, pin_mask) on the device, contiguous"""
        if pin is None:
            if pin_mask is not None:
                raise ValueError("pin_mask without pin: the mask says which cells of the edited rows leave the pinned trajectory")
            return None, None
        if p2p is None:
            raise ValueError("pin without p2p: the pinned rows are the source rows of a prompt-to-prompt edit")
        if latents is not None:
            raise ValueError("pin with latents: every row starts from pin[0], the noise the photo inverts to")
        want = (self.steps + 1,) + tuple(self.x.shape[1:])
        if not torch.is_tensor(pin) or pin.dtype != torch.float32 or tuple(pin.shape) != want:
            raise ValueError(f"pin {getattr(pin, 'dtype', type(pin).__name__)} {tuple(getattr(pin, 'shape', ()))}: expected float32 {want}, one "
                             "photo's trajectory (`invert(...)[:, b]`)")
        if pin_mask is not None and (not torch.is_tensor(pin_mask) or pin_mask.dtype != torch.uint8 or
                                     tuple(pin_mask.shape) != tuple(self.x.shape[2:])):
            raise ValueError(f"pin_mask {getattr(pin_mask, 'dtype', type(pin_mask).__name__)} {tuple(getattr(pin_mask, 'shape', ()))}: expected "
                             f"uint8 {tuple(self.x.shape[2:])}")
        pin = pin.to(self.x.device).contiguous()
        return pin, (None if pin_mask is None else pin_mask.to(self.x.device).contiguous())

    def denoise_from(self, cond_ehs, uncond_ehs, z0, noise, strength, mask=None, maps=None, regions=None, region_steps=None):
        """Image editing: diffusers' StableDiffusionImg2ImgPipeline and, with a mask, the latent blend of StableDiffusionInpaintPipeline for a
        4-channel UNet [3P restated: diffusers 0.29 is not installed here].  z0: the encoded image, fp32 [4, h, w] or [1, 4, h, w], shared by the B
        rows; noise: fp32 [B, 4, h, w], the noise of each row's image.  Steps begin .. steps-1 run, begin = `edit.strength_begin(steps, strength)`,
        from x = alpha_begin z0 + sigma_begin noise (also at strength 1, where diffusers' inpaint pipeline starts from pure noise); step
        `begin` is first order, as step 0 of `denoise` is.  mask: uint8 [h, w] on the device (non-zero = repaint), shared by channels and rows:
        after step i, x = mask ? x : alpha_{i+1} z0 + sigma_{i+1} noise in the step's own launch (`tb_dpm_step_blend`), so the kept cells end
        as z0 exactly.  Nothing of one call is kept for the next: the scheduler holds no step state, `begin` is an argument.
        regions / region_steps: as in `denoise`, counted in EXECUTED steps (step `begin` is the first).
        Returns the final latents fp32 [B, 4, h, w]."""
        from .edit import strength_begin
        B, sch = self.B, self.sch
        if not isinstance(sch, DPMSolverPP2M):
            raise NotImplementedError(f"image editing runs on the DPM-Solver++ scheduler only, not on {type(sch).__name__}")
        begin = strength_begin(self.steps, strength)
        region_steps = self._region_steps(regions, region_steps, self.steps - begin)
        z0 = z0.reshape(self.x.shape[1:]).to(self.x.device, torch.float32).contiguous()
        noise = noise.to(self.x.device, torch.float32).contiguous()
        if tuple(noise.shape) != tuple(self.x.shape):
            raise ValueError(f"noise {tuple(noise.shape)}: the sampler is built for {tuple(self.x.shape)}")
        if mask is not None:
            mask = mask.to(self.x.device).contiguous()
            if mask.dtype != torch.uint8 or tuple(mask.shape) != tuple(self.x.shape[2:]):
                raise ValueError(f"mask {mask.dtype} {tuple(mask.shape)}: expected uint8 {tuple(self.x.shape[2:])}")
        if maps is not None:
            maps.zero()
        a_b, s_b = sch.noise_scalars(begin)
        self.x.copy_(a_b * z0 + s_b * noise)
        self.m_prev.zero_()
        self.x2[:B].copy_(self.x)
        self.x2[B:].copy_(self.x)
        ehs = torch.cat([uncond_ehs, cond_ehs]).to(L.half_dtype()).contiguous()
        n = self.x[0].numel()
        for i in range(begin, self.steps):
            eps2 = self._unet_forward(i, ehs, maps, regions if i - begin < region_steps else None)
            a_t, s_t = sch.data_prediction_scalars(i)
            ca, cb, cc = sch.coefficients(i, begin)
            if mask is None:
                ops.dpm_step(self.x, eps2, self.m_prev, self.x2, n, B, self.g, a_t, s_t, ca, cb, cc)
            else:
                k_a, k_s = sch.noise_scalars(i + 1)
                ops.dpm_step_blend(self.x, eps2, self.m_prev, self.x2, n, B, self.g, a_t, s_t, ca, cb, cc, z0, noise, mask, k_a, k_s)
        return self.x

    def _region_steps(self, regions, region_steps, executed):
        """how many of the `executed` steps run with `regions`: all by default; ValueError outside 1 .. executed or without regions"""
        if regions is None:
            if region_steps is not None:
                raise ValueError("region_steps without regions")
            return 0
        if regions.B2 != self.unet.B or regions.T != self.unet.T or (regions.h, regions.w) != (self.unet.H, self.unet.W):
            raise ValueError(f"the regions are built for batch {regions.B2}, {regions.T} tokens and a {regions.h} x {regions.w} grid; the UNet runs "
                             f"batch {self.unet.B}, {self.unet.T} tokens, {self.unet.H} x {self.unet.W}")
        if region_steps is None:
            return executed
        if not 1 <= int(region_steps) <= executed or int(region_steps) != region_steps:
            raise ValueError(f"region_steps {region_steps}: a whole number of the {executed} executed steps, 1 .. {executed}")
        return int(region_steps)

    def _p2p_steps(self, p2p, maps=None, regions=None):
        """(steps with cross control, steps with self control) of `denoise`; every refusal, before anything is touched"""
        if p2p is None:
            return 0, 0
        from .p2p import steps_for
        if maps is not None:
            raise ValueError("prompt-to-prompt does not go with maps: the recorder recomputes its own softmax from q and k, so it would report "
                             "attention that did not happen under the control")
        if regions is not None:
            raise ValueError("prompt-to-prompt does not go with regions: the control's launch would overwrite the region-masked attention of "
                             "the edited rows")
        if not isinstance(self.sch, DPMSolverPP2M):
            raise NotImplementedError(f"prompt-to-prompt runs on the DPM-Solver++ scheduler only, not on {type(self.sch).__name__}")
        if self.B % 2:
            raise ValueError(f"prompt-to-prompt takes an even batch (source rows, then edited rows), not {self.B}")
        if p2p.B4 != self.unet.B or p2p.T != self.unet.T or (p2p.h, p2p.w) != (self.unet.H, self.unet.W):
            raise ValueError(f"the prompt-to-prompt control is built for batch {p2p.B4}, {p2p.T} tokens and a {p2p.h} x {p2p.w} grid; the UNet "
                             f"runs batch {self.unet.B}, {self.unet.T} tokens, {self.unet.H} x {self.unet.W}")
        return steps_for(p2p.cross_steps, self.steps, "cross_steps"), steps_for(p2p.self_steps, self.steps, "self_steps")

    def _unet_forward(self, i, ehs, maps, regions=None, p2p=None, p2p_cross=False, p2p_self=False):
        if p2p is not None and not (p2p_cross or p2p_self):
            p2p = None
        if maps is None and regions is None and p2p is None:
            return self.unet.forward(self.x2, self.t_dev[i], ehs)
        prev = self.unet.attn_maps, self.unet.regions, self.unet.p2p
        if maps is not None:
            self.unet.attn_maps = maps
        if regions is not None:
            self.unet.regions = regions
        if p2p is not None:
            self.unet.p2p = p2p
            p2p.cross_active, p2p.self_active = bool(p2p_cross), bool(p2p_self)
        try:
            return self.unet.forward(self.x2, self.t_dev[i], ehs)
        finally:
            self.unet.attn_maps, self.unet.regions, self.unet.p2p = prev
            if p2p is not None:
                p2p.cross_active = p2p.self_active = False

    def sample(self, cond_ehs, uncond_ehs, latents=None):
        return self.vae.decode(self.denoise(cond_ehs, uncond_ehs, latents))


def make_image_grid(images: torch.Tensor, rows: int, cols: int):
    """diffusers.utils.make_image_grid on a [rows*cols, 3, H, W] tensor in [0, 1] -> one PIL image (train_textboost.py:1224-1228)."""
    from PIL import Image
    n, c, H, W = images.shape
    assert n == rows * cols and c == 3
    arr = (images.clamp(0, 1) * 255).round().to(torch.uint8).permute(0, 2, 3, 1).cpu().numpy()
    grid = Image.new("RGB", (cols * W, rows * H))
    for i in range(n):
        grid.paste(Image.fromarray(arr[i]), box=((i % cols) * W, (i // cols) * H))
    return grid
