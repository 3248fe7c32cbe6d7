"""Measures what recording token attention maps (textboost_amd/attn_maps.py) costs the image-generation path at the real shapes (SD1.5 UNet / VAE
geometry, random weights, 64^2 latents, 13 prompts per batch, 25 DPM-Solver++ steps, guidance 7.5), the setting of scratch/bench_generate.py:

  * denoise with maps off and with maps on, alternating rounds in one process, by device events; images/s = batch / (denoise + decode);
  * the map kernel's own time per step: the sum of its 16 launches in one UNet forward, by per-launch events (ops.start_recording).

Run from a tree without textboost_amd/attn_maps.py (the parent commit) it measures the off case alone, so that the two trees can be compared
on one box in one session.

    python scratch/bench_attn_maps.py [out.json] [rounds]"""
import importlib.util
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from textboost_amd import generate as G  # noqa: E402
from textboost_amd import models, ops  # noqa: E402
from textboost_amd.vae import VAEGeometry, vae_decoder_shapes  # noqa: E402

dev = "cuda"


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    have_maps = importlib.util.find_spec("textboost_amd.attn_maps") is not None
    res = {"device": torch.cuda.get_device_name(0), "maps_available": have_maps, "rounds": rounds}
    usd = models.random_state_dict(models.unet_shapes(models.SD15_UNET), 1, device=dev)
    vsd = models.random_state_dict(vae_decoder_shapes(VAEGeometry()), 2, device=dev)
    with torch.no_grad():
        B = max(len(b) for b in G.prompt_batches(list(range(25)), 16))
        pipe = G.Pipeline(models.SD15_UNET, usd, VAEGeometry(), vsd, None, 64, B)
        cond, uncond = torch.randn(B * 77, 768, device=dev), torch.randn(B * 77, 768, device=dev)
        lat = G.seeded_latent(0, 64).to(dev).repeat(B, 1, 1, 1)
        rec = None
        if have_maps:
            from textboost_amd.attn_maps import AttnMapRecorder
            rec = AttnMapRecorder(pipe.unet)
        off = lambda: pipe.sampler.denoise(cond, uncond, latents=lat)  # noqa: E731
        on = lambda: pipe.sampler.denoise(cond, uncond, latents=lat, maps=rec)  # noqa: E731
        pipe.images(cond, uncond, lat)                      # warm-up
        if have_maps:
            on()
        torch.cuda.synchronize()
        t_off, t_on = [], []
        for _ in range(rounds):
            t_off.append(timed(off))
            if have_maps:
                t_on.append(timed(on))
        x = off().clone()
        dec = statistics.median([timed(lambda: pipe.vae.decode_rgbx(x)) for _ in range(3)])
        res.update(prompt_batch=B, steps=pipe.steps, decode_finish_ms=dec, denoise_off_ms=t_off,
                   off_images_per_s=B / ((statistics.median(t_off) + dec) * 1e-3))
        if have_maps:
            res.update(denoise_on_ms=t_on, on_images_per_s=B / ((statistics.median(t_on) + dec) * 1e-3),
                       result_ms=statistics.median([timed(rec.result) for _ in range(3)]))
            # the kernel's own time: per-launch events around every launch of one forward (eager; the other launches are timed too and ignored)
            x2 = torch.cat([lat, lat]).half()
            ehs = torch.cat([uncond, cond]).half().contiguous()
            per_step = []
            for _ in range(3):
                pipe.unet.attn_maps = rec
                ops.start_recording()
                pipe.unet.forward(x2, pipe.sampler.t_dev[0], ehs)
                launches = ops.stop_recording()
                pipe.unet.attn_maps = None
                torch.cuda.synchronize()
                mine = [e0.elapsed_time(e1) for name, _, _, e0, e1 in launches if name == "attn_token_maps_kernel"]
                per_step.append((len(mine), sum(mine)))
            res.update(map_kernel_launches_per_step=per_step[0][0], map_kernel_ms_per_step=statistics.median(s for _, s in per_step),
                       map_kernel_note="event pairs around single launches include the launch gap: an upper bound of the kernel time")
    print(json.dumps(res, indent=1))
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
