"""Measures FreeU (textboost_amd/freeu.py, csrc/freeu.hip) at the real shapes (SD1.5 UNet geometry, random weights, 64^2
latents, batch 13 = UNet batch 26, 25 DPM-Solver++ steps, guidance 7.5; the SD1.x default factors 1.5 1.6 0.9 0.2):

  * (a) denoise with FreeU off, `rounds` times in one process, by device events -- also what the parent commit can run;
  * (b) denoise with FreeU on, scalar and structure backbone, alternating with the plain one;
  * (c) tb_freeu per launch at the six concat shapes of a forward, both modes: `launches` launches captured in one graph, device events
    around a replay.

Run from a tree without textboost_amd/freeu.py (the parent commit) it measures (a) alone, so that the two trees can be compared on one box.
`--combine parent1.json this1.json parent2.json this2.json out.json` writes profiles/freeu_cost.json.

    python scratch/bench_freeu.py [out.json] [rounds]"""
import importlib.util
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

dev = "cuda"
BATCH, STEPS, LAUNCHES = 13, 25, 50
FACTORS = (1.5, 1.6, 0.9, 0.2)
# (H, W, hc, sc, b, s) in front of up_blocks.0.resnets.0-2 and up_blocks.1.resnets.0-2 at 64^2 latents
SHAPES = [(8, 8, 1280, 1280, 1.5, 0.9)] * 3 + [(16, 16, 1280, 1280, 1.6, 0.2)] * 2 + [(16, 16, 1280, 640, 1.6, 0.2)]


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


def kernel_times(B, rounds):
    """us per tb_freeu call (scalar: one kernel launch, structure: two) at every distinct concat shape; the buffer keeps being re-weighted, which
    changes values, not the work (factors near 1 so that nothing overflows over the repeats)"""
    from textboost_amd import ops
    out = {}
    for H, W, hc, sc, _, _ in sorted(set(SHAPES)):
        for mode in ("scalar", "structure"):
            cat = torch.randn(B * H * W, hc + sc, device=dev).half()
            replay = captured(lambda: [ops.freeu(cat, B, H, W, hc, 1.001, 0.999, mode) for _ in range(LAUNCHES)])
            ts = [timed(replay) / LAUNCHES * 1e3 for _ in range(rounds)]
            out[f"{B}x{H}x{W}x({hc}+{sc}) {mode}"] = {"us_per_call": ts, "median": statistics.median(ts),
                                                     "bytes_touched": B * H * W * (hc // 2 + sc) * 2 * 2 + (B * H * W * hc * 2 if mode == "structure" else 0)}
    return out


def main():
    from textboost_amd import generate as G
    from textboost_amd import models
    from textboost_amd.vae import VAEGeometry, vae_decoder_shapes
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    have = importlib.util.find_spec("textboost_amd.freeu") is not None
    res = {"device": torch.cuda.get_device_name(0), "freeu_available": have, "rounds": rounds}
    usd = models.random_state_dict(models.unet_shapes(models.SD15_UNET), 1, device=dev)
    vsd = models.random_state_dict(vae_decoder_shapes(VAEGeometry()), 2, device=dev)
    with torch.no_grad():
        B = BATCH
        pipe = G.Pipeline(models.SD15_UNET, usd, VAEGeometry(), vsd, None, 64, B, steps=STEPS)
        cond, uncond = torch.randn(B * 77, 768, device=dev), torch.randn(B * 77, 768, device=dev)
        lat = torch.cat([G.seeded_latent(s, 64) for s in range(B)]).to(dev)
        run = lambda: pipe.sampler.denoise(cond, uncond, latents=lat)  # noqa: E731
        run()                                                # warm-up
        torch.cuda.synchronize()
        t_off = [timed(run) for _ in range(rounds)]
        res.update(batch=B, steps=pipe.steps, off_denoise_ms=t_off, off_ms_per_step=statistics.median(t_off) / pipe.steps)
        if have:
            unet = pipe.unet
            t = {"scalar": [], "structure": [], "off_interleaved": []}
            for mode in ("scalar", "structure"):             # warm-up of both modes
                unet.enable_freeu(*FACTORS, mode=mode)
                run()
            unet.disable_freeu()
            torch.cuda.synchronize()
            for _ in range(rounds):
                for mode in ("scalar", "structure"):
                    unet.enable_freeu(*FACTORS, mode=mode)
                    t[mode].append(timed(run))
                unet.disable_freeu()
                t["off_interleaved"].append(timed(run))
            res.update(on_scalar_denoise_ms=t["scalar"], on_structure_denoise_ms=t["structure"], off_denoise_ms_interleaved=t["off_interleaved"],
                       freeu_calls_per_denoise=6 * pipe.steps, factors=list(FACTORS))
            res["kernels"] = kernel_times(2 * B, rounds + 2)
    print(json.dumps(res, indent=1))
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)


def combine(paths, out):
    p1, t1, p2, t2 = [json.load(open(p)) for p in paths]
    med = lambda r, k="off_denoise_ms": statistics.median(r[k])  # noqa: E731
    pm, tm = [med(p1), med(p2)], [med(t1), med(t2)]
    per_forward = [sum(r["kernels"][f"{2 * BATCH}x{H}x{W}x({hc}+{sc}) {mode}"]["median"] for H, W, hc, sc, _, _ in SHAPES)
                   for r in (t1, t2) for mode in ("scalar",)]
    res = {"device": t1["device"],
           "setting": "SD1.5 UNet geometry, random weights, 64^2 latents, batch 13 (UNet batch 26), 25 DPM-Solver++ steps, guidance 7.5; FreeU "
                      "factors 1.5 1.6 0.9 0.2; scratch/bench_freeu.py; processes in the order parent, this, parent, this on one box",
           "not_measured": "picture quality, the default factors, which backbone mode is better (random weights); other batch sizes and resolutions",
           "parent_commit": [p1, p2], "this_commit": [t1, t2],
           "summary": {"parent_off_denoise_ms_medians": pm, "this_off_denoise_ms_medians": tm,
                       "parent_spread_between_its_two_processes_ms": abs(pm[0] - pm[1]),
                       "this_off_minus_parent_ms": statistics.mean(tm) - statistics.mean(pm),
                       "flag_off_unchanged": abs(statistics.mean(tm) - statistics.mean(pm)) <= abs(pm[0] - pm[1]),
                       "on_scalar_denoise_ms_medians": [med(r, "on_scalar_denoise_ms") for r in (t1, t2)],
                       "on_structure_denoise_ms_medians": [med(r, "on_structure_denoise_ms") for r in (t1, t2)],
                       "off_denoise_ms_interleaved_medians": [med(r, "off_denoise_ms_interleaved") for r in (t1, t2)],
                       "on_scalar_minus_off_ms_per_step": [(med(r, "on_scalar_denoise_ms") - med(r, "off_denoise_ms_interleaved")) / r["steps"]
                                                           for r in (t1, t2)],
                       "on_structure_minus_off_ms_per_step": [(med(r, "on_structure_denoise_ms") - med(r, "off_denoise_ms_interleaved")) / r["steps"]
                                                              for r in (t1, t2)],
                       "six_scalar_calls_us": per_forward,
                       "kernels_us_per_call": [{k: v["median"] for k, v in r["kernels"].items()} for r in (t1, t2)]}}
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res["summary"], indent=1))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--combine":
        combine(sys.argv[2:6], sys.argv[6])
    else:
        main()
