"""Float64 references of the inversion path (textboost_amd/sampler.py `inversion_scalars` / `HipSampler.invert`, csrc/invert.hip).
Nothing here imports the kernel library."""
import math

import numpy as np
import torch

U = 2.0 ** -24                      # unit roundoff of fp32
GAMMA5 = 5 * U / (1 - 5 * U)        # five roundings in sequence


def f32(v):
    """the float the C ABI receives for a Python float"""
    return float(np.float32(v))


def invert_step(x, eps2, g, cx, ce):
    """tb_invert_step in float64 on the operands the kernel sees: x fp32 [B, n], eps2 half [2B, n] (uncond | cond), fp32-rounded scalars.
    -> (xn, bound): xn = cx x + ce (e_u + g (e_c - e_u)) and the elementwise error bound of an fp32 evaluation (tests/test_gpu_invert.py)."""
    B = x.shape[0]
    g, cx, ce = f32(g), f32(cx), f32(ce)
    xd, eu, ec = x.double().cpu(), eps2[:B].double().cpu(), eps2[B:].double().cpu()
    xn = cx * xd + ce * (eu + g * (ec - eu))
    bound = GAMMA5 * (abs(cx) * xd.abs() + abs(ce) * (eu.abs() + abs(g) * (ec.abs() + eu.abs())))
    return xn, bound


def first_order_step(sch, k, xk, eps):
    """the solver's first-order step k from xk with a given eps, float64: `data_prediction_scalars(k)` and `coefficients(k, begin=k)`"""
    a, s = sch.data_prediction_scalars(k)
    ca, cb, cc = sch.coefficients(k, begin=k)
    assert cc == 0.0
    return ca * xk + cb * ((xk - s * eps) / a)


def invert_trajectory(sch, eps_model, z0, steps):
    """[steps + 1, ...] float64: traj[steps] = z0, traj[k] = cx traj[k+1] + ce eps_model(traj[k+1], k)   (the model is asked about timesteps[k]
    and given the latents of level k+1)"""
    traj = [None] * (steps + 1)
    traj[steps] = z0.double()
    for k in range(steps - 1, -1, -1):
        cx, ce = sch.inversion_scalars(k)
        traj[k] = cx * traj[k + 1] + ce * eps_model(traj[k + 1], k).double()
    return torch.stack(traj)


# ---- an analytic model: data ~ N(0, S0^2) per coordinate, so the ideal denoiser and the probability-flow ODE are closed form
S0 = 0.9


def gaussian_eps(x, alpha, sigma):
    """eps(x; alpha, sigma) = sigma x / (S0^2 alpha^2 + sigma^2)"""
    return sigma * x / (S0 * S0 * alpha * alpha + sigma * sigma)


def gaussian_flow(x0, alpha, sigma):
    """the exact flow from the clean x0 to the level (alpha, sigma): x0 sqrt(S0^2 alpha^2 + sigma^2) / S0"""
    return x0 * math.sqrt(S0 * S0 * alpha * alpha + sigma * sigma) / S0


def gaussian_inversion_error(sch_cls, steps, x0=(0.7, -1.3)):
    """relative error of the inverted traj[0] against the exact flow, float64; the model is evaluated with the (alpha, sigma) of the timestep
    it is asked about, level k, on the latents of level k+1 -- as a network would be"""
    sch = sch_cls.from_config(None)
    sch.set_timesteps(steps)
    z0 = torch.tensor(x0, dtype=torch.float64)
    traj = invert_trajectory(sch, lambda x, k: gaussian_eps(x, *sch.noise_scalars(k)), z0, steps)
    want = gaussian_flow(z0, *sch.noise_scalars(0))
    return ((traj[0] - want).norm() / want.norm()).item()
