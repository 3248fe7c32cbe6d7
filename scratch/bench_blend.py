"""Measures prompt-to-prompt LocalBlend (textboost_amd/local_blend.py, csrc/local_blend.hip) at the real shapes (SD1.5 UNet geometry, random
weights, 64^2 latents, batch 12 = six pairs = UNet batch 24, 25 DPM-Solver++ steps, guidance 7.5):

  (a) the plain denoise and denoise(p2p=) without blend, `rounds` times each, alternating, by device events -- also what the parent commit
      can run, so that the two trees can be compared on one box;
  (b) denoise(p2p=, blend=) alternating with denoise(p2p=) in the same process (the default start 0.2 and threshold 0.3; a word of two
      positions in the source prompt and of four in the edit prompt);
  (c) per launch, `LAUNCHES` launches captured in one graph, device events around a replay after a warm-up replay, alternating:
      tb_blend_mask at six pairs (16 x 16 -> 64 x 64), and tb_dpm_step_local_blend beside tb_dpm_step at batch 12.

Run from a tree without textboost_amd/local_blend.py (the parent commit) it measures (a) alone.
`--combine parent1.json this1.json parent2.json this2.json out.json` writes profiles/blend_cost.json.

    python scratch/bench_blend.py [out.json] [rounds]"""
import importlib.util
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

dev = "cuda"
LAUNCHES = 50
BATCH = 12
med = statistics.median


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


def kernel_times(rounds):
    from textboost_amd import ops
    n, T, hl, wl, h, w = BATCH // 2, 77, 16, 16, 64, 64
    B, npb = BATCH, 4 * h * w
    acc = torch.rand(2 * n, T, hl * wl, device=dev)
    words = torch.full((2 * n, 16), -1, dtype=torch.int32, device=dev)
    words[:n, :2] = torch.tensor([5, 6], dtype=torch.int32)
    words[n:, :4] = torch.tensor([5, 6, 7, 8], dtype=torch.int32)
    mask = torch.zeros(n, h * w, dtype=torch.uint8, device=dev)
    area = torch.zeros(n, dtype=torch.int32, device=dev)
    x, mp = torch.randn(B, npb, device=dev), torch.randn(B, npb, device=dev)
    e, x2 = torch.randn(2 * B, npb, device=dev).half(), torch.zeros(2 * B, npb, device=dev).half()
    step = (7.5, 0.8, 0.6, 0.9, 0.3, -0.1)
    ops.blend_mask(acc, words, h, w, hl, wl, 0.3, mask, area=area)
    g_mask = captured(lambda: [ops.blend_mask(acc, words, h, w, hl, wl, 0.3, mask, area=area) for _ in range(LAUNCHES)])
    g_step = captured(lambda: [ops.dpm_step(x, e, mp, x2, npb, B, *step) for _ in range(LAUNCHES)])
    g_blend = captured(lambda: [ops.dpm_step_local_blend(x, e, mp, x2, npb, B, *step, mask, h * w) for _ in range(LAUNCHES)])
    tm, ts, tb = [], [], []
    for _ in range(rounds):                       # alternating
        x.normal_(), mp.normal_()                 # (the step feeds back into x: keep the operands finite)
        tm.append(timed(g_mask) / LAUNCHES * 1e3)
        x.normal_(), mp.normal_()
        ts.append(timed(g_step) / LAUNCHES * 1e3)
        x.normal_(), mp.normal_()
        tb.append(timed(g_blend) / LAUNCHES * 1e3)
    return {"pairs": n, "coarse": [hl, wl], "grid": [h, w], "batch": B, "launches_per_graph": LAUNCHES, "blend_mask_us": tm, "dpm_step_us": ts,
            "dpm_step_local_blend_us": tb, "blend_mask_us_median": med(tm), "dpm_step_us_median": med(ts),
            "dpm_step_local_blend_us_median": med(tb), "spread_us": max(max(v) - min(v) for v in (tm, ts, tb))}


def main():
    import numpy as np
    from textboost_amd import generate as G
    from textboost_amd import models
    from textboost_amd import p2p as P
    from textboost_amd.vae import VAEGeometry, vae_decoder_shapes
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    have = importlib.util.find_spec("textboost_amd.local_blend") is not None
    res = {"device": torch.cuda.get_device_name(0), "blend_available": have, "rounds": rounds}
    usd = models.random_state_dict(models.unet_shapes(models.SD15_UNET), 1, device=dev)
    vsd = models.random_state_dict(vae_decoder_shapes(VAEGeometry()), 2, device=dev)
    with torch.no_grad():
        B = BATCH
        pipe = G.Pipeline(models.SD15_UNET, usd, VAEGeometry(), vsd, None, 64, B)
        cond, uncond = torch.randn(B * 77, 768, device=dev), torch.randn(B * 77, 768, device=dev)
        lat = torch.cat([G.seeded_latent(s, 64) for s in range(B // 2)] * 2).to(dev)
        T = 77
        M, a, w = np.zeros((T, T), dtype=np.float32), np.ones(T, dtype=np.float32), np.ones(T, dtype=np.float32)
        M[np.arange(5), np.arange(5)] = 1              # "a photo of a dog ..." -> "a photo of a <dog> dog ...": three added vectors at 5 .. 7,
        M[np.arange(5, T - 3), np.arange(8, T)] = 1    # everything behind them shifted by three (scratch/bench_p2p.py's plan)
        a[5:8] = 0
        ctl = P.P2PControl.for_unet(pipe.unet, P.P2PPlan(M, a, w))
        plain = lambda: pipe.sampler.denoise(cond, uncond, latents=lat)  # noqa: E731
        p2p = lambda: pipe.sampler.denoise(cond, uncond, latents=lat, p2p=ctl)  # noqa: E731
        pipe.images(cond, uncond, lat)                      # warm-up
        p2p()
        torch.cuda.synchronize()
        t_plain, t_p2p = [], []
        for _ in range(rounds):                             # alternating
            t_plain.append(timed(plain))
            t_p2p.append(timed(p2p))
        res.update(batch=B, steps=pipe.steps, plain_denoise_ms=t_plain, p2p_denoise_ms=t_p2p)
        if have:
            from textboost_amd.local_blend import BlendControl, start_step
            bl = BlendControl(pipe.unet, [5, 6], [5, 6, 7, 8])
            blend = lambda: pipe.sampler.denoise(cond, uncond, latents=lat, p2p=ctl, blend=bl)  # noqa: E731
            blend()
            torch.cuda.synchronize()
            t_blend, t_p2p2 = [], []
            for _ in range(rounds):                         # alternating with the unblended edit
                t_blend.append(timed(blend))
                t_p2p2.append(timed(p2p))
            layers = len(pipe.sampler.blend_buffers.layers)
            first = start_step(bl.start, pipe.steps)
            res.update(blend_denoise_ms=t_blend, p2p_denoise_ms_interleaved=t_p2p2, final_area=bl.area.tolist(),
                       record_launches_per_denoise=layers * pipe.steps, blended_steps=pipe.steps - first, kernels=kernel_times(rounds))
    print(json.dumps(res, indent=1))
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)


def combine(paths, out):
    p1, t1, p2, t2 = [json.load(open(p)) for p in paths]
    runs = (p1, t1, p2, t2)
    summary = {}
    for key in ("plain_denoise_ms", "p2p_denoise_ms"):
        pm, tm = [med(p1[key]), med(p2[key])], [med(t1[key]), med(t2[key])]
        summary[key] = {"parent_medians": pm, "this_medians": tm, "this_minus_parent_ms": statistics.mean(tm) - statistics.mean(pm),
                        "spread_ms": {"parent_between_processes": abs(pm[0] - pm[1]), "this_between_processes": abs(tm[0] - tm[1]),
                                      "within_process_max_minus_min": max(max(r[key]) - min(r[key]) for r in runs)}}
    summary["blend_denoise_ms_medians"] = [med(t1["blend_denoise_ms"]), med(t2["blend_denoise_ms"])]
    summary["p2p_denoise_ms_interleaved_medians"] = [med(t1["p2p_denoise_ms_interleaved"]), med(t2["p2p_denoise_ms_interleaved"])]
    summary["blend_minus_p2p_ms"] = [med(r["blend_denoise_ms"]) - med(r["p2p_denoise_ms_interleaved"]) for r in (t1, t2)]
    summary["record_launches_per_denoise"] = t1["record_launches_per_denoise"]
    summary["blended_steps"] = t1["blended_steps"]
    summary["kernels_per_launch_us"] = {k: [t1["kernels"][k], t2["kernels"][k]] for k in
                                        ("blend_mask_us_median", "dpm_step_us_median", "dpm_step_local_blend_us_median", "spread_us")}
    res = {"device": t1["device"],
           "setting": "SD1.5 UNet geometry, random weights, 64^2 latents, batch 12 (six pairs, UNet batch 24), 25 DPM-Solver++ steps, guidance "
                      "7.5; prompt-to-prompt control with three added token positions (cross 20 steps, self 10); LocalBlend with start 0.2, "
                      "threshold 0.3, two source and four edit positions; scratch/bench_blend.py; processes in the order parent, this, parent, "
                      "this on one box",
           "not_measured": "edit quality and the defaults (the weights are random); other batch sizes and resolutions",
           "parent_commit": [p1, p2], "this_commit": [t1, t2], "summary": summary}
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(summary, indent=1))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--combine":
        combine(sys.argv[2:6], sys.argv[6])
    else:
        main()
