"""Measures regional prompts (textboost_amd/regions.py, csrc/region_attn.hip) at the real shapes (SD1.5 UNet geometry, random weights, 64^2
latents, batch 13 = UNet batch 26, 25 DPM-Solver++ steps, guidance 7.5), the setting of scratch/bench_edit.py:

  * denoise with regions off, `rounds` times in one process, by device events -- also what the parent commit can run;
  * denoise with two half-image regions (left / right, four token positions each) on all steps: eager, as inference.py runs it (every
    region launch first reads the key table back to check it: one stream synchronise), alternating with regions off;
  * the region kernel beside tb_attention_fwd at the four cross-attention shapes of that UNet (B = 26, 8 heads, 77 keys): `launches`
    launches of each captured in one graph (no host work between them), device events around a replay, after a warm-up replay.

Run from a tree without textboost_amd/regions.py (the parent commit) it measures the first item alone, so that the two trees can be compared
on one box.  `--combine parent1.json this1.json parent2.json this2.json out.json` writes profiles/region_attn_cost.json.

    python scratch/bench_regions.py [out.json] [rounds]"""
import importlib.util
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

dev = "cuda"
SHAPES = [(4096, 40), (1024, 80), (256, 160), (64, 160)]      # (queries, head dim) of the 64^2 / 32^2 / 16^2 / 8^2 maps; 8 heads, 77 keys
LAUNCHES = 50


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
    import numpy as np
    from textboost_amd import ops
    B, H, T = 26, 8, 77
    out = []
    for Sq, hd in SHAPES:
        C = H * hd
        q = torch.randn(B * Sq, C, device=dev).half()
        kv = torch.randn(B * T, 2 * C, device=dev).half()
        k, v = kv[:, :C], kv[:, C:]
        o, lse = torch.empty_like(q), torch.empty(B, H, Sq, device=dev)
        side = int(Sq ** 0.5)
        qb = np.ones((side, side), dtype=np.int32)
        qb[:, side // 2:] = 2
        kr = np.full((B, T), -1, dtype=np.int32)
        kr[B // 2:, 2:6], kr[B // 2:, 8:12] = 0, 1
        krd, qbd = torch.from_numpy(kr).to(dev), torch.from_numpy(qb.reshape(-1)).to(dev)
        flash = captured(lambda: [ops.attention_fwd(q, k, v, o, lse, B, H, Sq, T, hd) for _ in range(LAUNCHES)])
        region = captured(lambda: [ops.attention_region_fwd(q, k, v, o, lse, B, H, Sq, T, hd, krd, qbd) for _ in range(LAUNCHES)])
        tf, tr = [], []
        for _ in range(rounds):                       # alternating
            tf.append(timed(flash) / LAUNCHES * 1e3)
            tr.append(timed(region) / LAUNCHES * 1e3)
        # eager, as the UNet calls it outside a capture: host time per call, the table check (a stream synchronise) included
        import time
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(LAUNCHES):
            ops.attention_region_fwd(q, k, v, o, lse, B, H, Sq, T, hd, krd, qbd)
        torch.cuda.synchronize()
        eager = (time.perf_counter() - t0) / LAUNCHES * 1e6
        traffic = 2.0 * (2 * B * Sq * C + 2 * B * T * C)          # bytes: Q in, O out, K and V once
        out.append({"B": B, "H": H, "Sq": Sq, "Skv": T, "hd": hd, "flash_fwd_us": tf, "region_fwd_us": tr,
                    "flash_fwd_us_median": statistics.median(tf), "region_fwd_us_median": statistics.median(tr),
                    "region_minus_flash_us": statistics.median(tr) - statistics.median(tf),
                    "spread_us": max(max(tf) - min(tf), max(tr) - min(tr)),
                    "region_eager_host_us_per_call": eager,
                    "region_GBps_of_Q_O_K_V_traffic": traffic / (statistics.median(tr) * 1e-6) * 1e-9})
    return out


def main():
    from textboost_amd import generate as G
    from textboost_amd import models
    from textboost_amd.vae import VAEGeometry, vae_decoder_shapes
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    have = importlib.util.find_spec("textboost_amd.regions") is not None
    res = {"device": torch.cuda.get_device_name(0), "regions_available": have, "rounds": rounds}
    usd = models.random_state_dict(models.unet_shapes(models.SD15_UNET), 1, device=dev)
    vsd = models.random_state_dict(vae_decoder_shapes(VAEGeometry()), 2, device=dev)
    with torch.no_grad():
        B = max(len(b) for b in G.prompt_batches(list(range(25)), 16))
        pipe = G.Pipeline(models.SD15_UNET, usd, VAEGeometry(), vsd, None, 64, B)
        cond, uncond = torch.randn(B * 77, 768, device=dev), torch.randn(B * 77, 768, device=dev)
        lat = G.seeded_latent(0, 64).to(dev).repeat(B, 1, 1, 1)
        off = lambda: pipe.sampler.denoise(cond, uncond, latents=lat)  # noqa: E731
        pipe.images(cond, uncond, lat)                      # warm-up
        torch.cuda.synchronize()
        t_off = [timed(off) for _ in range(rounds)]
        res.update(batch=B, steps=pipe.steps, off_denoise_ms=t_off, off_ms_per_step=statistics.median(t_off) / pipe.steps)
        if have:
            from textboost_amd.regions import Region, RegionSet, box_cells
            regs = [Region(("left",), (2, 3, 4, 5), box_cells((0, 0, 0.5, 1), 64, 64)), Region(("right",), (8, 9, 10, 11), box_cells((0.5, 0, 1, 1), 64, 64))]
            rset = RegionSet.for_unet(pipe.unet, regs)
            on = lambda: pipe.sampler.denoise(cond, uncond, latents=lat, regions=rset)  # noqa: E731
            on()
            torch.cuda.synchronize()
            t_on, t_off2 = [], []
            for _ in range(rounds):                         # alternating with regions off
                t_on.append(timed(on))
                t_off2.append(timed(off))
            res.update(on_denoise_ms=t_on, off_denoise_ms_interleaved=t_off2, on_ms_per_step=statistics.median(t_on) / pipe.steps,
                       region_launches_per_denoise=len(pipe.unet.xattn) * pipe.steps,
                       kernels=kernel_times(rounds))
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
    kern = []
    for a, b in zip(t1["kernels"], t2["kernels"]):
        kern.append({"Sq": a["Sq"], "hd": a["hd"], "flash_fwd_us": [a["flash_fwd_us_median"], b["flash_fwd_us_median"]],
                     "region_fwd_us": [a["region_fwd_us_median"], b["region_fwd_us_median"]],
                     "region_minus_flash_us": [a["region_minus_flash_us"], b["region_minus_flash_us"]], "spread_us": [a["spread_us"], b["spread_us"]],
                     "region_eager_host_us_per_call": [a["region_eager_host_us_per_call"], b["region_eager_host_us_per_call"]]})
    res = {"device": t1["device"],
           "setting": "SD1.5 UNet geometry, random weights, 64^2 latents, batch 13 (UNet batch 26), 25 DPM-Solver++ steps, guidance 7.5; two "
                      "half-image regions (left / right, four token positions each) on all steps; scratch/bench_regions.py; processes in the "
                      "order parent, this, parent, this on one box",
           "not_measured": "image quality (the weights are random); any default for --region-steps; other batch sizes and resolutions",
           "parent_commit": [p1, p2], "this_commit": [t1, t2],
           "summary": {"parent_off_denoise_ms_medians": pm, "this_off_denoise_ms_medians": tm,
                       "run_to_run_spread_ms": {"parent_between_processes": abs(pm[0] - pm[1]), "this_between_processes": abs(tm[0] - tm[1]),
                                                "within_process_max_minus_min": within},
                       "this_off_minus_parent_ms": statistics.mean(tm) - statistics.mean(pm),
                       "on_denoise_ms_medians": [med(t1, "on_denoise_ms"), med(t2, "on_denoise_ms")],
                       "off_denoise_ms_interleaved_medians": [med(t1, "off_denoise_ms_interleaved"), med(t2, "off_denoise_ms_interleaved")],
                       "on_minus_off_ms": [med(r, "on_denoise_ms") - med(r, "off_denoise_ms_interleaved") for r in (t1, t2)],
                       "region_launches_per_denoise": t1["region_launches_per_denoise"], "kernels_per_launch": kern}}
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res["summary"], indent=1))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--combine":
        combine(sys.argv[2:6], sys.argv[6])
    else:
        main()
