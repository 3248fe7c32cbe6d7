"""Measures the MultiDiffusion canvas (textboost_amd/canvas.py, csrc/canvas.hip) at the real shapes (SD1.5 UNet geometry, random weights,
64^2 windows, UNet batch 26 = 13 image-window pairs, 25 DPM-Solver++ steps, guidance 7.5):

  (a) the plain batch-13 `denoise` and `images`, `rounds` times each, by device events -- also what the parent commit can run, so that
      the two trees can be compared on one box;
  (b) `denoise_canvas` of 512 x 2048 pixels (64 x 256 cells) at stride 16 -- 13 windows, one chunk -- with one seed and with four seeds
      (52 pairs, four chunks), alternating with the plain denoise of the same process: ms per step;
  (c) per launch, `LAUNCHES` launches captured in one graph, device events around a replay after a warm-up replay: tb_canvas_gather (one
      chunk), tb_canvas_step (one seed, four seeds) beside tb_dpm_step at batch 13, tb_tile_blend (one seed);
  (d) decoding the canvas: the tiles through the decoder plus tb_tile_blend, and `canvas_images` as a whole in images per second.

Run from a tree without textboost_amd/canvas.py (the parent commit) it measures (a) alone.
`--combine parent1.json this1.json parent2.json this2.json out.json` writes profiles/canvas_cost.json.

    python scratch/bench_canvas.py [out.json] [rounds]"""
import importlib.util
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

dev = "cuda"
LAUNCHES = 50
BATCH = 13
S, HC, WC, STRIDE = 64, 64, 256, 16
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
    from textboost_amd.canvas import CanvasPlan, blend_ramp
    step = (7.5, 0.8, 0.6, 0.9, 0.3, -0.1)
    out = {"launches_per_graph": LAUNCHES}
    graphs = {}
    state = []
    for n in (1, 4):
        plan = CanvasPlan(S, HC, WC, STRIDE, n, BATCH)
        plan.tables(dev)
        x, mp = torch.randn(n, 4, HC, WC, device=dev), torch.randn(n, 4, HC, WC, device=dev)
        xh = x.half()
        e = torch.randn(plan.n_chunks, 2 * BATCH, 4, S, S, device=dev).half()
        x2 = torch.zeros(2 * BATCH, 4, S, S, device=dev).half()
        state.append((x, mp))
        graphs[f"canvas_step_{n}_seeds_us"] = captured(lambda x=x, mp=mp, e=e, xh=xh, plan=plan: [ops.canvas_step(x, e, mp, plan, *step, xh=xh)
                                                                                                  for _ in range(LAUNCHES)])
        if n == 1:
            graphs["canvas_gather_us"] = captured(lambda x=x, x2=x2, plan=plan, xh=xh: [ops.canvas_gather(x, x2, plan, 0, xh=xh) for _ in range(LAUNCHES)])
            graphs["canvas_gather_fp32_us"] = captured(lambda x=x, x2=x2, plan=plan: [ops.canvas_gather(x, x2, plan, 0) for _ in range(LAUNCHES)])
    npb = 4 * S * S
    dx, dm = torch.randn(BATCH, npb, device=dev), torch.randn(BATCH, npb, device=dev)
    de, dx2 = torch.randn(2 * BATCH, npb, device=dev).half(), torch.zeros(2 * BATCH, npb, device=dev).half()
    state.append((dx, dm))
    graphs["dpm_step_batch13_us"] = captured(lambda: [ops.dpm_step(dx, de, dm, dx2, npb, BATCH, *step) for _ in range(LAUNCHES)])
    f, ds = 8, 48
    tp = CanvasPlan(S, HC, WC, ds, 1, BATCH)
    tp.tables(dev, f)
    tiles = torch.randn(tp.pairs * (f * S) ** 2, 4, device=dev)
    rgbx = torch.zeros(1, f * HC, f * WC, dtype=torch.int32, device=dev)
    graphs["tile_blend_us"] = captured(lambda: [ops.tile_blend(tiles, tp, f, blend_ramp(S, ds, f), rgbx=rgbx) for _ in range(LAUNCHES)])
    times = {k: [] for k in graphs}
    for _ in range(rounds):                       # alternating
        for k, g in graphs.items():
            for a, b in state:                    # (the steps feed back into x: keep the operands finite)
                a.normal_(), b.normal_()
            times[k].append(timed(g) / LAUNCHES * 1e3)
    for k, v in times.items():
        out[k] = v
        out[k + "_median"] = med(v)
    out["tiles"] = tp.pairs
    out["bytes_moved"] = {"canvas_gather": BATCH * npb * (2 + 2 * 2), "canvas_step_1_seed": 4 * HC * WC * (4 * 4 + 2) + 13 * 2 * npb * 2,
                          "tile_blend": int(tiles.numel() * 4 + rgbx.numel() * 4)}
    return out


def main():
    from textboost_amd import generate as G
    from textboost_amd import models
    from textboost_amd.vae import VAEGeometry, vae_decoder_shapes
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    have = importlib.util.find_spec("textboost_amd.canvas") is not None
    res = {"device": torch.cuda.get_device_name(0), "canvas_available": have, "rounds": rounds}
    usd = models.random_state_dict(models.unet_shapes(models.SD15_UNET), 1, device=dev)
    vsd = models.random_state_dict(vae_decoder_shapes(VAEGeometry()), 2, device=dev)
    with torch.no_grad():
        B = BATCH
        pipe = G.Pipeline(models.SD15_UNET, usd, VAEGeometry(), vsd, None, 64, B)
        cond, uncond = torch.randn(77, 768, device=dev).repeat(B, 1), torch.randn(77, 768, device=dev).repeat(B, 1)
        lat = torch.cat([G.seeded_latent(s, 64) for s in range(B)]).to(dev)
        plain = lambda: pipe.sampler.denoise(cond, uncond, latents=lat)  # noqa: E731
        images = lambda: pipe.images(cond, uncond, lat)  # noqa: E731
        images()                                            # warm-up
        torch.cuda.synchronize()
        t_plain, t_images = [], []
        for _ in range(rounds):                             # alternating
            t_plain.append(timed(plain))
            t_images.append(timed(images))
        res.update(batch=B, steps=pipe.steps, plain_denoise_ms=t_plain, plain_images_ms=t_images)
        if have:
            from textboost_amd import ops
            from textboost_amd.canvas import CanvasPlan, blend_ramp
            for n in (1, 4):
                clat = torch.cat([G.seeded_canvas_latent(s, HC, WC) for s in range(n)]).to(dev)
                canvas = lambda: pipe.sampler.denoise_canvas(cond, uncond, clat, stride=STRIDE)  # noqa: E731
                canvas()
                torch.cuda.synchronize()
                t_c, t_p = [], []
                for _ in range(rounds):                     # alternating with the plain denoise
                    t_c.append(timed(canvas))
                    t_p.append(timed(plain))
                plan = pipe.sampler.canvas_plan
                res[f"canvas_{n}_seeds"] = {"pairs": plan.pairs, "chunks": plan.n_chunks, "denoise_canvas_ms": t_c, "plain_denoise_ms_interleaved": t_p,
                                            "ms_per_step": med(t_c) / pipe.steps, "plain_ms_per_step": med(t_p) / pipe.steps,
                                            "ms_per_step_per_chunk": med(t_c) / pipe.steps / plan.n_chunks}
                x = canvas().clone()
                ds, f = 48, 8
                tp = CanvasPlan(S, HC, WC, ds, n, B)
                rgbx = torch.empty(n, f * HC, f * WC, dtype=torch.int32, device=dev)

                def decode():
                    tiles = torch.stack([x[i, :, oy:oy + S, ox:ox + S] for i in range(n) for oy, ox in tp.windows()])
                    rows, _, _ = pipe.vae.decode_tiles(tiles)
                    ops.tile_blend(rows, tp, f, blend_ramp(S, ds, f), rgbx=rgbx)
                whole = lambda: pipe.canvas_images(cond, uncond, clat, stride=STRIDE)  # noqa: E731
                decode(), whole()
                torch.cuda.synchronize()
                t_d, t_w = [timed(decode) for _ in range(rounds)], [timed(whole) for _ in range(rounds)]
                res[f"canvas_{n}_seeds"].update(tiles=tp.pairs, decoder_chunks=tp.n_chunks, decode_and_blend_ms=t_d, canvas_images_ms=t_w,
                                                images_per_s=n / (med(t_w) * 1e-3))
            res["kernels"] = kernel_times(rounds)
    print(json.dumps(res, indent=1))
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)


def combine(paths, out):
    p1, t1, p2, t2 = [json.load(open(p)) for p in paths]
    runs = (p1, t1, p2, t2)
    summary = {}
    for key in ("plain_denoise_ms", "plain_images_ms"):
        pm, tm = [med(p1[key]), med(p2[key])], [med(t1[key]), med(t2[key])]
        summary[key] = {"parent_medians": pm, "this_medians": tm, "this_minus_parent_ms": statistics.mean(tm) - statistics.mean(pm),
                        "spread_ms": {"parent_between_processes": abs(pm[0] - pm[1]), "this_between_processes": abs(tm[0] - tm[1]),
                                      "within_process_max_minus_min": max(max(r[key]) - min(r[key]) for r in runs)}}
    for n in (1, 4):
        k = f"canvas_{n}_seeds"
        summary[k] = {f: [t1[k][f], t2[k][f]] for f in ("pairs", "chunks", "ms_per_step", "plain_ms_per_step", "ms_per_step_per_chunk", "tiles",
                                                         "images_per_s")}
        summary[k]["decode_and_blend_ms_medians"] = [med(t1[k]["decode_and_blend_ms"]), med(t2[k]["decode_and_blend_ms"])]
        summary[k]["canvas_images_ms_medians"] = [med(t1[k]["canvas_images_ms"]), med(t2[k]["canvas_images_ms"])]
    summary["kernels_per_launch_us"] = {k: [t1["kernels"][k], t2["kernels"][k]] for k in t1["kernels"] if k.endswith("_median")}
    summary["kernels_bytes_moved"] = t1["kernels"]["bytes_moved"]
    res = {"device": t1["device"],
           "setting": "SD1.5 UNet and VAE geometry, random weights, 64^2 windows, UNet batch 26 (13 image-window pairs), 25 DPM-Solver++ steps, "
                      "guidance 7.5; canvas 64 x 256 cells (512 x 2048 pixels) at window stride 16 and decode stride 48; "
                      "scratch/bench_canvas.py; processes in the order parent, this, parent, this on one box",
           "not_measured": "picture quality, seams and the default strides (the weights are random); other canvas shapes and batch sizes",
           "parent_commit": [p1, p2], "this_commit": [t1, t2], "summary": summary}
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(summary, indent=1))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--combine":
        combine(sys.argv[2:6], sys.argv[6])
    else:
        main()
