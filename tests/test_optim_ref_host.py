"""tests/optim_ref.py (the float64 reference of the GPU optimizer-tail tests) against the real torch.optim.AdamW, clip_grad_norm_, LambdaLR and
GradScaler on float64 CPU parameters: three param groups with distinct learning rates, the clip on the first group only, the decay-only embedding
rows as a parameter whose gradient is zero, one skipped step, a schedule shorter than the run.  No GPU."""
import pytest
import torch

import optim_ref as R


def _torch_run(hp, init, grads_per_step, scale0):
    """the loop body of the reference script (train_textboost.py:1108-1149) on torch's own classes.  accelerate's AcceleratedScheduler is the
    `if not skipped: scheduler.step()` below."""
    P = {k: torch.nn.Parameter(v.clone()) for k, v in init.items()}
    opt = torch.optim.AdamW([{"params": [P["lora"]], "lr": hp.lr},
                             {"params": [P["decay"], P["added"]], "lr": hp.emb_lr},
                             {"params": [P["unet"]], "lr": hp.lr}],
                            betas=(hp.beta1, hp.beta2), eps=hp.eps, weight_decay=hp.wd)
    n = len(hp.lr_table)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda k: hp.lr_table[min(k, n - 1)])
    scaler = torch.amp.GradScaler("cpu", init_scale=scale0, growth_factor=hp.growth_factor, backoff_factor=hp.backoff_factor,
                                  growth_interval=hp.growth_interval)
    scaler.scale(torch.zeros(1))    # (the scale tensor is created on first use)
    out = []
    for g in grads_per_step:
        for k in ("lora", "added", "unet"):
            P[k].grad = g[k].clone()
        P["decay"].grad = torch.zeros_like(P["decay"])          # :1114-1117
        scaler.unscale_(opt)
        torch.nn.utils.clip_grad_norm_([P["lora"]], hp.max_norm)
        before = opt.state[P["lora"]]["step"].item() if opt.state[P["lora"]] else 0
        scaler.step(opt)
        scaler.update()
        skipped = (opt.state[P["lora"]]["step"].item() if opt.state[P["lora"]] else 0) == before
        if not skipped:
            sched.step()
        opt.zero_grad(set_to_none=True)
        R.clamp_rows(P["added"].data, hp.mean_norm)            # (not torch's: the one piece of the loop that is the project's own)
        snap = {k: P[k].detach().clone() for k in P}
        for k in ("lora", "added", "unet"):
            st = opt.state[P[k]]
            snap["m_" + k] = st["exp_avg"].clone() if st else torch.zeros_like(P[k])
            snap["v_" + k] = st["exp_avg_sq"].clone() if st else torch.zeros_like(P[k])
        snap["scale"], snap["tracker"], snap["skipped"] = scaler.get_scale(), int(scaler._growth_tracker.item()), skipped
        out.append(snap)
    return out


@pytest.mark.parametrize("skip_at", [0, 2])
def test_reference_tail_equals_torch_adamw(skip_at):
    torch.manual_seed(3)
    D, k = 24, 3
    hp = R.Hyper(lr=1e-3, emb_lr=5e-3, beta1=0.8, beta2=0.99, wd=0.05, max_norm=1.0, mean_norm=1.0, growth_interval=3,
                 lr_table=[1.0, 0.7, 0.45, 0.2])
    rows = torch.randn(k, D, dtype=torch.float64)
    rows *= (torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64) / rows.norm(dim=-1))[:, None]   # both sides of mean_norm
    init = {"lora": torch.randn(53, dtype=torch.float64), "added": rows, "unet": torch.randn(31, dtype=torch.float64),
            "decay": torch.randn(40, dtype=torch.float64)}
    scale0 = 1024.0
    steps, scale = [], scale0
    sc = R.TailState(scale=scale0)      # only to replay the scale the gradients of each step are multiplied by
    for it in range(6):
        sigma = 0.3 if it % 2 == 0 else 0.01            # LoRA norm ~ 2.2 (clipped) / ~ 0.07 (not clipped)
        g = {"lora": torch.randn(53, dtype=torch.float64) * sigma, "added": torch.randn(k, D, dtype=torch.float64) * 0.1,
             "unet": torch.randn(31, dtype=torch.float64)}
        g = {n: x * scale for n, x in g.items()}
        if it == skip_at:
            g["lora"][7] = float("inf")
        steps.append(g)
        scale = scale * hp.backoff_factor if it == skip_at else scale
        sc.tracker = 0 if it == skip_at else sc.tracker + 1
        if sc.tracker == hp.growth_interval:
            scale, sc.tracker = scale * hp.growth_factor, 0
    want = _torch_run(hp, init, steps, scale0)

    groups = {n: R.Group(init[n].clone(), torch.zeros_like(init[n]), torch.zeros_like(init[n])) for n in ("lora", "added", "unet")}
    groups["decay"] = init["decay"].clone()
    state = R.TailState(scale=scale0)
    clipped, moves = [], set()
    for it, (g, w) in enumerate(zip(steps, want)):
        scale_in = state.scale
        R.tail_step(state, groups, g, hp)
        moves.add(state.scale / scale_in)
        assert state.found_inf == w["skipped"] == (it == skip_at)
        assert state.scale == w["scale"] and state.tracker == w["tracker"], (it, state, w["scale"], w["tracker"])
        if not state.found_inf:
            clipped.append(state.coef_lora * scale_in < 1.0)
        for n in ("lora", "added", "unet"):
            torch.testing.assert_close(groups[n].p, w[n], rtol=1e-12, atol=0, msg=lambda m: f"step {it} {n}: {m}")
            torch.testing.assert_close(groups[n].m, w["m_" + n], rtol=1e-12, atol=0, msg=lambda m: f"step {it} m_{n}: {m}")
            torch.testing.assert_close(groups[n].v, w["v_" + n], rtol=1e-12, atol=0, msg=lambda m: f"step {it} v_{n}: {m}")
        torch.testing.assert_close(groups["decay"], w["decay"], rtol=1e-12, atol=0)
    assert state.step == 5 and any(clipped) and not all(clipped)
    assert moves == {1.0, hp.growth_factor, hp.backoff_factor}


def test_reference_tail_without_scaler_never_skips():
    """use_scaler = False (the fp32 / bf16 modes): torch's optimizer.step() is not guarded by anything, the scale and the tracker do not move, and
    a non-finite LoRA gradient poisons what torch poisons: inf -> total inf -> clip 0 -> inf * 0 = NaN in that element, 0 in every other;
    NaN -> total NaN -> every LoRA gradient NaN."""
    torch.manual_seed(4)
    hp = R.Hyper(use_scaler=False, growth_interval=2)
    for bad, all_nan in ((float("inf"), False), (float("nan"), True)):
        p0 = torch.randn(20, dtype=torch.float64)
        P = torch.nn.Parameter(p0.clone())
        opt = torch.optim.AdamW([P], lr=hp.lr, betas=(hp.beta1, hp.beta2), eps=hp.eps, weight_decay=hp.wd)
        groups = {"lora": R.Group(p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0))}
        state = R.TailState(scale=1.0)
        for it in range(3):
            g = torch.randn(20, dtype=torch.float64)
            if it == 1:
                g[5] = bad
            P.grad = g.clone()
            torch.nn.utils.clip_grad_norm_([P], hp.max_norm)
            opt.step()
            R.tail_step(state, groups, {"lora": g}, hp)
            assert not state.found_inf and state.scale == 1.0 and state.tracker == 0 and state.step == it + 1
            torch.testing.assert_close(groups["lora"].p, P.detach(), rtol=1e-12, atol=0, equal_nan=True)
        assert torch.isnan(groups["lora"].p).all() == all_nan and torch.isnan(groups["lora"].p)[5]
