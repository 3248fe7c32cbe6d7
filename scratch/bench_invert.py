"""Measures editing a photo by its prompt (HipSampler.invert / denoise(pin=...), csrc/invert.hip) at SD1.5 geometry with random
weights, 64^2 latents, by device events:

  (a) plain text-to-image `denoise`, batch 12, 25 steps, `rounds` times -- also what the parent commit can run;
  (b) on the batch-2 pipeline (UNet batch 4: one photo, source row and edited row), at 25 and at 50 steps: `invert` of one photo, and beside it
      the prompt-to-prompt `denoise` of the same batch (three added token positions and a reweighted word, the default fractions);
  (c) the same denoise with the source row pinned to the trajectory, alternating with the unpinned one; and per launch, `tb_dpm_step_pin`
      beside `tb_dpm_step` on the [2, 4, 64, 64] latents: 50 launches of each captured in one graph, device events around a replay.

Run from a tree without `HipSampler.invert` (the parent commit) it measures (a) alone, so that the two trees can be compared on one box.
`--combine parent1.json this1.json parent2.json this2.json out.json` writes profiles/invert_cost.json.

    python scratch/bench_invert.py [out.json] [rounds]"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

dev = "cuda"
LAUNCHES = 50
BATCH = 12


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def captured(fn):
    """fn's launches as one graph -> a callable that replays it"""
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        fn()
    g.replay()
    torch.cuda.synchronize()
    return g.replay


def step_kernels(rounds):
    from textboost_amd import ops
    B, n, hw = 2, 4 * 64 * 64, 64 * 64
    x, mp, pin = torch.randn(B, n, device=dev), torch.randn(B, n, device=dev), torch.randn(n, device=dev)
    e, x2 = torch.randn(2 * B, n, device=dev).half(), torch.zeros(2 * B, n, device=dev).half()
    mask = (torch.rand(hw, device=dev) < 0.5).to(torch.uint8)
    step = (7.5, 0.8, 0.6, 0.5, 0.3, -0.1)        # a contraction (0.5 + 0.3 / 0.8 < 1): repeated launches stay finite
    runs = {"dpm_step_us": captured(lambda: [ops.dpm_step(x, e, mp, x2, n, B, *step) for _ in range(LAUNCHES)]),
            "dpm_step_pin_us": captured(lambda: [ops.dpm_step_pin(x, e, mp, x2, n, B, *step, pin, 1, None, hw) for _ in range(LAUNCHES)]),
            "dpm_step_pin_masked_us": captured(lambda: [ops.dpm_step_pin(x, e, mp, x2, n, B, *step, pin, 1, mask, hw) for _ in range(LAUNCHES)]),
            "invert_step_us": captured(lambda: [ops.invert_step(x, e, x2, mp, n, B, 1.0, 1.0, 0.0) for _ in range(LAUNCHES)])}
    t = {k: [] for k in runs}
    for _ in range(rounds):                       # alternating
        for k, fn in runs.items():
            t[k].append(timed(fn) / LAUNCHES * 1e3)
    out = {"B": B, "n_per_b": n, "launches_per_graph": LAUNCHES}
    for k, v in t.items():
        out[k] = v
        out[k + "_median"] = statistics.median(v)
    out["spread_us"] = max(max(v) - min(v) for v in t.values())
    return out


def main():
    from textboost_amd import generate as G
    from textboost_amd import models
    from textboost_amd.sampler import HipSampler
    from textboost_amd.vae import VAEGeometry, vae_decoder_shapes
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    have = hasattr(HipSampler, "invert")
    res = {"device": torch.cuda.get_device_name(0), "invert_available": have, "rounds": rounds}
    usd = models.random_state_dict(models.unet_shapes(models.SD15_UNET), 1, device=dev)
    vsd = models.random_state_dict(vae_decoder_shapes(VAEGeometry()), 2, device=dev)
    med = statistics.median
    with torch.no_grad():
        B = BATCH
        pipe = G.Pipeline(models.SD15_UNET, usd, VAEGeometry(), vsd, None, 64, B)
        cond, uncond = torch.randn(B * 77, 768, device=dev), torch.randn(B * 77, 768, device=dev)
        lat = torch.cat([G.seeded_latent(s, 64) for s in range(B)]).to(dev)
        plain = lambda: pipe.sampler.denoise(cond, uncond, latents=lat)  # noqa: E731
        pipe.images(cond, uncond, lat)                      # warm-up
        torch.cuda.synchronize()
        t = [timed(plain) for _ in range(rounds)]
        res.update(batch=B, steps=pipe.steps, plain_denoise_ms=t, plain_ms_per_step=med(t) / pipe.steps)
        del pipe
        if have:
            import numpy as np
            from textboost_amd import p2p as P
            T = 77
            M, a, w = np.zeros((T, T), dtype=np.float32), np.ones(T, dtype=np.float32), np.ones(T, dtype=np.float32)
            M[np.arange(5), np.arange(5)] = 1              # "a photo of a dog ..." -> "a photo of a <dog> dog ...": three added vectors at 5 .. 7,
            M[np.arange(5, T - 3), np.arange(8, T)] = 1    # everything behind them shifted by three
            a[5:8] = 0
            w[8] = 2.0
            pipe2 = G.Pipeline(models.SD15_UNET, usd, VAEGeometry(), vsd, None, 64, 2)
            ctl = P.P2PControl.for_unet(pipe2.unet, P.P2PPlan(M, a, w))
            c2, u2 = cond[:2 * 77], uncond[:2 * 77]
            z0 = torch.randn(1, 4, 64, 64, device=dev) * 0.9
            edits = []
            for steps in (25, 50):
                smp = HipSampler(pipe2.unet, pipe2.vae, steps=steps, guidance=7.5)
                traj = smp.invert(c2, u2, z0).clone()        # warm-up
                start = traj[0, :1].expand(2, -1, -1, -1).contiguous()
                pin = traj[:, 0].contiguous()
                inv = lambda: smp.invert(c2, u2, z0)  # noqa: E731
                unpinned = lambda: smp.denoise(c2, u2, latents=start, p2p=ctl)  # noqa: E731
                pinned = lambda: smp.denoise(c2, u2, p2p=ctl, pin=pin)  # noqa: E731
                unpinned(), pinned()
                torch.cuda.synchronize()
                ti, tu, tp = [], [], []
                for _ in range(rounds):                     # alternating
                    ti.append(timed(inv))
                    tu.append(timed(unpinned))
                    tp.append(timed(pinned))
                edits.append({"steps": steps, "unet_batch": 4, "invert_ms": ti, "p2p_denoise_ms": tu, "pinned_p2p_denoise_ms": tp,
                              "invert_ms_median": med(ti), "invert_ms_per_step": med(ti) / steps, "p2p_denoise_ms_median": med(tu),
                              "p2p_denoise_ms_per_step": med(tu) / steps, "pinned_p2p_denoise_ms_median": med(tp),
                              "pinned_minus_unpinned_ms": med(tp) - med(tu),
                              "spread_ms": max(max(v) - min(v) for v in (ti, tu, tp))})
            res.update(edits=edits, step_kernels=step_kernels(rounds))
    print(json.dumps(res, indent=1))
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)


def combine(paths, out):
    p1, t1, p2, t2 = [json.load(open(p)) for p in paths]
    med = lambda r: statistics.median(r["plain_denoise_ms"])  # noqa: E731
    within = max(max(r["plain_denoise_ms"]) - min(r["plain_denoise_ms"]) for r in (p1, t1, p2, t2))
    pm, tm = [med(p1), med(p2)], [med(t1), med(t2)]
    ekeys = ("invert_ms_median", "invert_ms_per_step", "p2p_denoise_ms_median", "p2p_denoise_ms_per_step", "pinned_p2p_denoise_ms_median",
             "pinned_minus_unpinned_ms", "spread_ms")
    edits = [{"steps": a["steps"], **{k: [a[k], b[k]] for k in ekeys}} for a, b in zip(t1["edits"], t2["edits"])]
    kkeys = [k for k in t1["step_kernels"] if k.endswith("_median")] + ["spread_us"]
    res = {"device": t1["device"],
           "setting": "SD1.5 UNet geometry, random weights, 64^2 latents, DPM-Solver++, guidance 7.5; (a) batch 12, 25 steps; (b), (c) one photo "
                      "on the batch-2 pipeline (UNet batch 4), 25 and 50 steps, control: three added token positions and one reweighted word at "
                      "the default fractions, inversion guidance 1; scratch/bench_invert.py; processes in the order parent, this, parent, this "
                      "on one box",
           "not_measured": "edit quality and the default inversion guidance of 1 (the weights are random); other batch sizes and resolutions",
           "parent_commit": [p1, p2], "this_commit": [t1, t2],
           "summary": {"parent_plain_denoise_ms_medians": pm, "this_plain_denoise_ms_medians": tm,
                       "run_to_run_spread_ms": {"parent_between_processes": abs(pm[0] - pm[1]), "this_between_processes": abs(tm[0] - tm[1]),
                                                "within_process_max_minus_min": within},
                       "this_minus_parent_ms": statistics.mean(tm) - statistics.mean(pm), "edits": edits,
                       "step_kernels_per_launch_us": {k: [t1["step_kernels"][k], t2["step_kernels"][k]] for k in kkeys}}}
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res["summary"], indent=1))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--combine":
        combine(sys.argv[2:6], sys.argv[6])
    else:
        main()
