"""Measures Attend-and-Excite (textboost_amd/excite.py, csrc/excite.hip) at the real shapes (SD1.5 UNet geometry, random weights,
64^2 latents, batch 13 = UNet batch 26, 50 DPM-Solver++ steps, guidance 7.5; two words, one of two token positions):

  * denoise without `excite`, `rounds` times in one process, by device events -- also what the parent commit can run;
  * one excite pass (truncated forward, loss, backward to the latents, update) beside the plain step and beside the same pass on an
    untruncated forward / backward, alternating;
  * the three new kernels per launch: `launches` launches of each captured in one graph, device events around a replay;
  * a whole guided generation without refinement (with refinement the count of passes depends on the weights), alternating with the plain one;
  * d_sample at loss_scale 1 / 256 / 4096: the relative difference to the 4096 one and the share of zero elements.

Run from a tree without textboost_amd/excite.py (the parent commit) it measures the first item alone, so that the two trees can be compared on
one box.  `--combine parent1.json this1.json parent2.json this2.json out.json` writes profiles/excite_cost.json.

    python scratch/bench_excite.py [out.json] [rounds]"""
import importlib.util
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

dev = "cuda"
BATCH, STEPS, LAUNCHES = 13, 50, 50
WORDS, LAST = [[2], [5, 6]], 9


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def captured(fn):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        fn()
    g.replay()
    torch.cuda.synchronize()
    return g.replay


def rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm()).item()


def kernel_times(unet, rounds):
    from textboost_amd import ops
    ex, B = unet.excite, unet.B
    nb, H, Sq, T, hd = ex.nb, 8, ex.h * ex.w, unet.T, 160
    q = torch.randn(B * Sq, H * hd, device=dev).half()
    k = torch.randn(B * T, H * hd, device=dev).half()
    dq = torch.zeros_like(q)
    x = torch.randn(nb, 4, unet.H, unet.W, device=dev)
    g = torch.randn(nb, 4, unet.H, unet.W, device=dev).half()
    x2 = torch.zeros(2 * nb, 4, unet.H, unet.W, device=dev).half()
    step, bad = torch.full((nb,), 1e-3, device=dev), torch.zeros(nb, dtype=torch.int32, device=dev)
    fns = {"excite_loss": lambda: ops.excite_loss(ex.acc, ex.last, ex.words, ex.h, ex.w, 256.0, ex.loss, ex.word, ex.sel, ex.dA),
           "excite_bwd": lambda: ops.excite_bwd(q, k, dq, ex.sel, ex.dA, B, H, Sq, T, hd, 1.0 / (H * ex.n), b0=ex.b0, nb=nb),
           "excite_update_two_launches": lambda: ops.excite_update(x, g, step, x2, bad, 256.0)}
    graphs = {n: captured(lambda f=f: [f() for _ in range(LAUNCHES)]) for n, f in fns.items()}
    out = {n: [] for n in fns}
    for _ in range(rounds):
        for n, gr in graphs.items():
            out[n].append(timed(gr) / LAUNCHES * 1e3)
    return {"shapes": {"excite_loss": [nb, T, ex.h, ex.w], "excite_bwd": [nb, 9, H, T, hd], "excite_update": [nb, 4 * unet.H * unet.W]},
            "us_per_launch": out, "us_per_launch_median": {n: statistics.median(v) for n, v in out.items()}}


def main():
    from textboost_amd import generate as G
    from textboost_amd import models
    from textboost_amd.vae import VAEGeometry, vae_decoder_shapes
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    have = importlib.util.find_spec("textboost_amd.excite") is not None
    res = {"device": torch.cuda.get_device_name(0), "excite_available": have, "rounds": rounds}
    usd = models.random_state_dict(models.unet_shapes(models.SD15_UNET), 1, device=dev)
    vsd = models.random_state_dict(vae_decoder_shapes(VAEGeometry()), 2, device=dev)
    with torch.no_grad():
        B = BATCH
        pipe = G.Pipeline(models.SD15_UNET, usd, VAEGeometry(), vsd, None, 64, B, steps=STEPS)
        cond, uncond = torch.randn(B * 77, 768, device=dev), torch.randn(B * 77, 768, device=dev)
        lat = torch.cat([G.seeded_latent(s, 64) for s in range(B)]).to(dev)
        off = lambda: pipe.sampler.denoise(cond, uncond, latents=lat)  # noqa: E731
        off()                                                # warm-up
        torch.cuda.synchronize()
        t_off = [timed(off) for _ in range(rounds)]
        res.update(batch=B, steps=pipe.steps, off_denoise_ms=t_off, off_ms_per_step=statistics.median(t_off) / pipe.steps)
        if have:
            from textboost_amd import ops
            from textboost_amd.excite import ExciteControl
            unet, smp = pipe.unet, pipe.sampler
            ctl = ExciteControl(unet, WORDS, LAST, refine=False)
            on = lambda: smp.denoise(cond, uncond, latents=lat, excite=ctl)  # noqa: E731
            on()
            torch.cuda.synchronize()
            t_on, t_off2 = [], []
            for _ in range(rounds):
                t_on.append(timed(on))
                t_off2.append(timed(off))
            guided = len(ctl.trace)
            res.update(on_denoise_no_refine_ms=t_on, off_denoise_ms_interleaved=t_off2, guided_steps=guided, skipped_updates=ctl.skipped,
                       loss_first_step=ctl.trace[0]["loss_before"], loss_last_guided_step=ctl.trace[-1]["loss_before"])
            # one pass on the start latents: truncated against untruncated
            ex = unet.excite
            ehs = torch.cat([uncond, cond]).half().contiguous()
            smp.x.copy_(lat)
            smp.x2[:B].copy_(smp.x)
            smp.x2[B:].copy_(smp.x)
            zero_dpred = torch.zeros(2 * B, 4, 64, 64, device=dev)
            zero_step = torch.zeros(B, device=dev)           # the update launches, but moves nothing: every round sees the same latents

            def truncated(ls=256.0):
                unet.forward(smp.x2, smp.t_dev[0], ehs, until="excite")
                unet.excite_loss(ls)
                d = unet.backward_sample()
                ops.excite_update(smp.x, d[B:], zero_step, smp.x2, smp._ex_bad, ls)
                return d

            def untruncated(ls=256.0):
                ex.record = True
                try:
                    unet.forward(smp.x2, smp.t_dev[0], ehs)
                finally:
                    ex.record = False
                unet.excite_loss(ls)
                d = unet.backward_sample(zero_dpred, excite=True)
                ops.excite_update(smp.x, d[B:], zero_step, smp.x2, smp._ex_bad, ls)
                return d

            plain = lambda: unet.forward(smp.x2, smp.t_dev[0], ehs)  # noqa: E731
            truncated(), untruncated(), plain()
            torch.cuda.synchronize()
            t_tr, t_un, t_pl = [], [], []
            for _ in range(rounds + 2):
                t_tr.append(timed(truncated))
                t_un.append(timed(untruncated))
                t_pl.append(timed(plain))
            med = statistics.median
            res.update(pass_truncated_ms=t_tr, pass_untruncated_ms=t_un, plain_unet_forward_ms=t_pl,
                       truncated_over_untruncated=med(t_tr) / med(t_un), truncated_pass_over_plain_forward=med(t_tr) / med(t_pl))
            d = {ls: truncated(ls)[B:].float().clone() / ls for ls in (1.0, 256.0, 4096.0)}
            du = untruncated(256.0)[B:].float() / 256.0
            res["loss_scale"] = {"rel_diff_256_vs_4096": rel(d[256.0], d[4096.0]), "rel_diff_1_vs_4096": rel(d[1.0], d[4096.0]),
                                 "zero_share": {str(int(ls)): (v == 0).float().mean().item() for ls, v in d.items()},
                                 "finite": {str(int(ls)): bool(torch.isfinite(v).all()) for ls, v in d.items()},
                                 "max_abs_scaled_gradient": {str(int(ls)): (v.abs().max() * ls).item() for ls, v in d.items()},
                                 "truncated_vs_untruncated_rel_diff": rel(d[256.0], du), "losses": ex.loss.tolist()}
            res["kernels"] = kernel_times(unet, rounds + 2)
    print(json.dumps(res, indent=1))
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)


def combine(paths, out):
    p1, t1, p2, t2 = [json.load(open(p)) for p in paths]
    med = lambda r, k="off_denoise_ms": statistics.median(r[k])  # noqa: E731
    within = max(max(r["off_denoise_ms"]) - min(r["off_denoise_ms"]) for r in (p1, t1, p2, t2))
    pm, tm = [med(p1), med(p2)], [med(t1), med(t2)]
    res = {"device": t1["device"],
           "setting": "SD1.5 UNet geometry, random weights, 64^2 latents, batch 13 (UNet batch 26), 50 DPM-Solver++ steps, guidance 7.5; two "
                      "words (token positions [2] and [5, 6], end token at 9), guidance on the first 25 steps, no refinement; "
                      "scratch/bench_excite.py; processes in the order parent, this, parent, this on one box",
           "not_measured": "image quality, the paper's defaults (scale 20, thresholds) and a generation WITH refinement: the number of "
                           "refinement passes depends on the weights, which are random here; other batch sizes and resolutions",
           "parent_commit": [p1, p2], "this_commit": [t1, t2],
           "summary": {"parent_off_denoise_ms_medians": pm, "this_off_denoise_ms_medians": tm,
                       "run_to_run_spread_ms": {"parent_between_processes": abs(pm[0] - pm[1]), "this_between_processes": abs(tm[0] - tm[1]),
                                                "within_process_max_minus_min": within},
                       "this_off_minus_parent_ms": statistics.mean(tm) - statistics.mean(pm),
                       "plain_step_ms": [r["off_ms_per_step"] for r in (t1, t2)],
                       "pass_truncated_ms_medians": [med(r, "pass_truncated_ms") for r in (t1, t2)],
                       "pass_untruncated_ms_medians": [med(r, "pass_untruncated_ms") for r in (t1, t2)],
                       "truncated_over_untruncated": [r["truncated_over_untruncated"] for r in (t1, t2)],
                       "on_denoise_no_refine_ms_medians": [med(r, "on_denoise_no_refine_ms") for r in (t1, t2)],
                       "off_denoise_ms_interleaved_medians": [med(r, "off_denoise_ms_interleaved") for r in (t1, t2)],
                       "kernels_us_per_launch": [r["kernels"]["us_per_launch_median"] for r in (t1, t2)],
                       "loss_scale": [r["loss_scale"] for r in (t1, t2)]}}
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res["summary"], indent=1))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--combine":
        combine(sys.argv[2:6], sys.argv[6])
    else:
        main()
