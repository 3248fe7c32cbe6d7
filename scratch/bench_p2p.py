"""Measures prompt-to-prompt editing (textboost_amd/p2p.py, csrc/p2p_attn.hip) at the real shapes (SD1.5 UNet geometry, random weights, 64^2
latents, batch 12 = six seeds = UNet batch 24, 25 DPM-Solver++ steps, guidance 7.5):

  * denoise with the control off, `rounds` times in one process, by device events -- also what the parent commit can run;
  * denoise with the control on (an added three-vector placeholder and a reweighted word, so both terms of the kernel are live; the default
    fractions 0.8 / 0.4), alternating with the control off in the same process;
  * per launch, at the four cross-attention shapes of that UNet (8 heads, 77 keys) and at two batch sizes -- B = 6, what the control
    launches at UNet batch 24, and B = 26, the table of DESIGN.md 19 -- the two-term kernel beside (a) one tb_attention_fwd and (b) the
    composed path: two tb_attention_fwd launches, the second into a temporary, and an add.  `launches` launches of each captured in one graph
    (no host work between them), device events around a replay, after a warm-up replay, alternating.

Run from a tree without textboost_amd/p2p.py (the parent commit) it measures the first item alone, so that the two trees can be compared on
one box.  `--combine parent1.json this1.json parent2.json this2.json out.json` writes profiles/p2p_cost.json.

    python scratch/bench_p2p.py [out.json] [rounds]"""
import importlib.util
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

dev = "cuda"
SHAPES = [(4096, 40), (1024, 80), (256, 160), (64, 160)]      # (queries, head dim) of the 64^2 / 32^2 / 16^2 / 8^2 maps; 8 heads, 77 keys
BATCHES = (6, 26)
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


def kernel_times(rounds):
    from textboost_amd import ops
    H, T = 8, 77
    out = []
    for B in BATCHES:
        for Sq, hd in SHAPES:
            C = H * hd
            q = torch.randn(2 * B * Sq, C, device=dev).half()
            q1, q2 = q[:B * Sq], q[B * Sq:]
            kv = torch.randn(2 * B * T, 2 * C, device=dev).half()
            k1, k2 = kv[:B * T, :C], kv[B * T:, :C]
            v1, v2 = torch.randn(B * T, C, device=dev).half(), torch.randn(B * T, C, device=dev).half()
            o, tmp, lse = torch.empty_like(q1), torch.empty_like(q1), torch.empty(B, H, Sq, device=dev)

            def composed():
                for _ in range(LAUNCHES):
                    ops.attention_fwd(q1, k1, v1, o, lse, B, H, Sq, T, hd)
                    ops.attention_fwd(q2, k2, v2, tmp, lse, B, H, Sq, T, hd)
                    o.add_(tmp)
            flash = captured(lambda: [ops.attention_fwd(q1, k1, v1, o, lse, B, H, Sq, T, hd) for _ in range(LAUNCHES)])
            dual = captured(lambda: [ops.attention_dual_fwd(q1, k1, v1, q2, k2, v2, o, B, H, Sq, T, T, hd) for _ in range(LAUNCHES)])
            single = captured(lambda: [ops.attention_dual_fwd(q1, k1, v1, None, None, None, o, B, H, Sq, T, T, hd) for _ in range(LAUNCHES)])
            comp = captured(composed)
            tf, td, ts, tc = [], [], [], []
            for _ in range(rounds):                       # alternating
                tf.append(timed(flash) / LAUNCHES * 1e3)
                td.append(timed(dual) / LAUNCHES * 1e3)
                ts.append(timed(single) / LAUNCHES * 1e3)
                tc.append(timed(comp) / LAUNCHES * 1e3)
            med = statistics.median
            out.append({"B": B, "H": H, "Sq": Sq, "Skv": T, "hd": hd, "flash_fwd_us": tf, "dual_fwd_us": td, "dual_single_term_us": ts,
                        "composed_two_flash_plus_add_us": tc, "flash_fwd_us_median": med(tf), "dual_fwd_us_median": med(td),
                        "dual_single_term_us_median": med(ts), "composed_us_median": med(tc),
                        "dual_minus_composed_us": med(td) - med(tc), "dual_over_flash": med(td) / med(tf),
                        "spread_us": max(max(x) - min(x) for x in (tf, td, ts, tc))})
    return out


def main():
    from textboost_amd import generate as G
    from textboost_amd import models
    from textboost_amd.vae import VAEGeometry, vae_decoder_shapes
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    have = importlib.util.find_spec("textboost_amd.p2p") is not None
    res = {"device": torch.cuda.get_device_name(0), "p2p_available": have, "rounds": rounds}
    usd = models.random_state_dict(models.unet_shapes(models.SD15_UNET), 1, device=dev)
    vsd = models.random_state_dict(vae_decoder_shapes(VAEGeometry()), 2, device=dev)
    with torch.no_grad():
        B = BATCH
        pipe = G.Pipeline(models.SD15_UNET, usd, VAEGeometry(), vsd, None, 64, B)
        cond, uncond = torch.randn(B * 77, 768, device=dev), torch.randn(B * 77, 768, device=dev)
        lat = torch.cat([G.seeded_latent(s, 64) for s in range(B // 2)] * 2).to(dev)
        off = lambda: pipe.sampler.denoise(cond, uncond, latents=lat)  # noqa: E731
        pipe.images(cond, uncond, lat)                      # warm-up
        torch.cuda.synchronize()
        t_off = [timed(off) for _ in range(rounds)]
        res.update(batch=B, steps=pipe.steps, off_denoise_ms=t_off, off_ms_per_step=statistics.median(t_off) / pipe.steps)
        if have:
            import numpy as np
            from textboost_amd import p2p as P
            T = 77
            M, a, w = np.zeros((T, T), dtype=np.float32), np.ones(T, dtype=np.float32), np.ones(T, dtype=np.float32)
            M[np.arange(5), np.arange(5)] = 1              # "a photo of a dog ..." -> "a photo of a <dog> dog ...": three added vectors at 5 .. 7,
            M[np.arange(5, T - 3), np.arange(8, T)] = 1    # everything behind them shifted by three
            a[5:8] = 0
            w[8] = 2.0
            ctl = P.P2PControl.for_unet(pipe.unet, P.P2PPlan(M, a, w))
            on = lambda: pipe.sampler.denoise(cond, uncond, latents=lat, p2p=ctl)  # noqa: E731
            on()
            torch.cuda.synchronize()
            t_on, t_off2 = [], []
            for _ in range(rounds):                         # alternating with the control off
                t_on.append(timed(on))
                t_off2.append(timed(off))
            nself = sum(1 for p, _ in pipe.unet.xattn if pipe.unet.xattn_level[p] >= P.SELF_MIN_LEVEL)
            res.update(on_denoise_ms=t_on, off_denoise_ms_interleaved=t_off2, on_ms_per_step=statistics.median(t_on) / pipe.steps,
                       cross_steps=P.steps_for(ctl.cross_steps, pipe.steps), self_steps=P.steps_for(ctl.self_steps, pipe.steps),
                       dual_launches_per_denoise=len(pipe.unet.xattn) * P.steps_for(ctl.cross_steps, pipe.steps),
                       extra_self_launches_per_denoise=nself * P.steps_for(ctl.self_steps, pipe.steps),
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
    keys = ("flash_fwd_us_median", "dual_fwd_us_median", "dual_single_term_us_median", "composed_us_median", "dual_minus_composed_us", "spread_us")
    kern = [{"B": a["B"], "Sq": a["Sq"], "hd": a["hd"], **{k: [a[k], b[k]] for k in keys}} for a, b in zip(t1["kernels"], t2["kernels"])]
    res = {"device": t1["device"],
           "setting": "SD1.5 UNet geometry, random weights, 64^2 latents, batch 12 (six seeds, UNet batch 24), 25 DPM-Solver++ steps, guidance "
                      "7.5; control: three added token positions and one reweighted word, cross-attention control on 20 steps and "
                      "self-attention control on 10; scratch/bench_p2p.py; processes in the order parent, this, parent, this on one box",
           "not_measured": "image quality and the default fractions (the weights are random); other batch sizes and resolutions",
           "parent_commit": [p1, p2], "this_commit": [t1, t2],
           "summary": {"parent_off_denoise_ms_medians": pm, "this_off_denoise_ms_medians": tm,
                       "run_to_run_spread_ms": {"parent_between_processes": abs(pm[0] - pm[1]), "this_between_processes": abs(tm[0] - tm[1]),
                                                "within_process_max_minus_min": within},
                       "this_off_minus_parent_ms": statistics.mean(tm) - statistics.mean(pm),
                       "on_denoise_ms_medians": [med(t1, "on_denoise_ms"), med(t2, "on_denoise_ms")],
                       "off_denoise_ms_interleaved_medians": [med(t1, "off_denoise_ms_interleaved"), med(t2, "off_denoise_ms_interleaved")],
                       "on_minus_off_ms": [med(r, "on_denoise_ms") - med(r, "off_denoise_ms_interleaved") for r in (t1, t2)],
                       "dual_launches_per_denoise": t1["dual_launches_per_denoise"],
                       "extra_self_launches_per_denoise": t1["extra_self_launches_per_denoise"], "kernels_per_launch": kern}}
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res["summary"], indent=1))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--combine":
        combine(sys.argv[2:6], sys.argv[6])
    else:
        main()
