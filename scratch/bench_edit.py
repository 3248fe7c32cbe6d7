"""Measures image editing (textboost_amd/edit.py, `HipSampler.denoise_from`, `Pipeline.edit_images`) beside text-to-image at the real shapes
(SD1.5 UNet / VAE geometry, random weights, 64^2 latents, batch 13, 25 DPM-Solver++ steps, guidance 7.5), the setting of
scratch/bench_attn_maps.py:

  * text-to-image denoise, `rounds` times in one process, by device events;
  * editing at strength 0.6 (15 of the 25 steps) with a centred half-area mask: the VAE encode (once per photo), the denoise and its time per
    executed step, decode + paste; images/s = batch / (denoise + decode + paste).

Run from a tree without textboost_amd/edit.py (the parent commit) it measures text-to-image alone, so that the two trees can be compared on one
box in one session.  `--combine parent1.json this1.json parent2.json this2.json out.json` writes the summary (profiles/edit_throughput.json).

    python scratch/bench_edit.py [out.json] [rounds]"""
import importlib.util
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

dev = "cuda"
STRENGTH = 0.6


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    import numpy as np
    from textboost_amd import generate as G
    from textboost_amd import models, ops
    from textboost_amd.vae import VAEGeometry, vae_decoder_shapes, vae_encoder_shapes
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    have_edit = importlib.util.find_spec("textboost_amd.edit") is not None
    res = {"device": torch.cuda.get_device_name(0), "edit_available": have_edit, "rounds": rounds}
    usd = models.random_state_dict(models.unet_shapes(models.SD15_UNET), 1, device=dev)
    vsd = models.random_state_dict(vae_decoder_shapes(VAEGeometry()), 2, device=dev)
    with torch.no_grad():
        B = max(len(b) for b in G.prompt_batches(list(range(25)), 16))
        pipe = G.Pipeline(models.SD15_UNET, usd, VAEGeometry(), vsd, None, 64, B)
        cond, uncond = torch.randn(B * 77, 768, device=dev), torch.randn(B * 77, 768, device=dev)
        lat = G.seeded_latent(0, 64).to(dev).repeat(B, 1, 1, 1)
        t2i = lambda: pipe.sampler.denoise(cond, uncond, latents=lat)  # noqa: E731
        pipe.images(cond, uncond, lat)                      # warm-up
        torch.cuda.synchronize()
        t_t2i = [timed(t2i) for _ in range(rounds)]
        x = t2i().clone()
        dec = statistics.median([timed(lambda: pipe.vae.decode_rgbx(x)) for _ in range(3)])
        res.update(batch=B, steps=pipe.steps, t2i_denoise_ms=t_t2i, t2i_ms_per_step=statistics.median(t_t2i) / pipe.steps, decode_ms=dec,
                   t2i_images_per_s=B / ((statistics.median(t_t2i) + dec) * 1e-3))
        if have_edit:
            from textboost_amd import edit as E
            from textboost_amd.vae import HipVAEEncoder
            esd = models.random_state_dict(vae_encoder_shapes(VAEGeometry()), 3, device=dev)
            enc = HipVAEEncoder(VAEGeometry(), esd, 1, 512, 512, device=dev)
            pixels = torch.rand(1, 3, 512, 512, device=dev) * 2 - 1
            zero = torch.zeros(1, 4, 64, 64, device=dev)
            enc.encode(pixels, noise=zero)
            t_enc = [timed(lambda: enc.encode(pixels, noise=zero)) for _ in range(rounds)]
            z0 = enc.encode(pixels, noise=zero).clone()
            pm = np.zeros((512, 512), dtype=np.uint8)
            pm[75:437, 75:437] = 1                            # 362^2 / 512^2 = 0.4999 of the area, centred
            lm = E.pool_mask_any(pm)
            pm_d, lm_d = torch.from_numpy(pm).to(dev), torch.from_numpy(lm).to(dev)
            init = torch.randint(0, 2 ** 24, (512, 512), device=dev, dtype=torch.int32)
            begin = E.strength_begin(pipe.steps, STRENGTH)
            ran = pipe.steps - begin
            ed = lambda: pipe.sampler.denoise_from(cond, uncond, z0, lat, STRENGTH, mask=lm_d)  # noqa: E731
            ed_plain = lambda: pipe.sampler.denoise_from(cond, uncond, z0, lat, STRENGTH)  # noqa: E731
            ed()
            t_ed = [timed(ed) for _ in range(rounds)]
            t_plain = [timed(ed_plain) for _ in range(rounds)]
            xe = ed().clone()

            def finish():
                rgbx = pipe.vae.decode_rgbx(xe)
                out = torch.empty_like(rgbx)
                for b in range(B):
                    ops.img_paste(rgbx[b], init, pm_d, out=out[b])
            finish()
            t_fin = [timed(finish) for _ in range(3)]
            res.update(strength=STRENGTH, executed_steps=ran, mask_area=float(pm.mean()), latent_mask_area=float(lm.mean()), encode_ms=t_enc,
                       edit_denoise_ms=t_ed, edit_ms_per_step=statistics.median(t_ed) / ran, edit_no_mask_denoise_ms=t_plain,
                       edit_no_mask_ms_per_step=statistics.median(t_plain) / ran, decode_paste_ms=statistics.median(t_fin),
                       edit_images_per_s=B / ((statistics.median(t_ed) + statistics.median(t_fin)) * 1e-3))
    print(json.dumps(res, indent=1))
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)


def combine(paths, out):
    p1, t1, p2, t2 = [json.load(open(p)) for p in paths]
    med = lambda r: statistics.median(r["t2i_denoise_ms"])  # noqa: E731
    within = max(max(r["t2i_denoise_ms"]) - min(r["t2i_denoise_ms"]) for r in (p1, t1, p2, t2))
    pm, tm = [med(p1), med(p2)], [med(t1), med(t2)]
    res = {"device": t1["device"],
           "setting": "SD1.5 UNet / VAE geometry, random weights, 64^2 latents, batch 13 (UNet batch 26), 25 DPM-Solver++ steps, guidance 7.5; "
                      "scratch/bench_edit.py; processes in the order parent, this, parent, this on one box in one session; editing at strength "
                      "0.6 (15 executed steps) with a centred half-area mask",
           "images_per_s_definition": "batch / (median denoise ms + median decode [+ paste] ms); the encode runs once per photo and is listed apart",
           "parent_commit": [p1, p2], "this_commit": [t1, t2],
           "summary": {"parent_t2i_denoise_ms_medians": pm, "this_t2i_denoise_ms_medians": tm,
                       "run_to_run_spread_ms": {"parent_between_processes": abs(pm[0] - pm[1]), "this_between_processes": abs(tm[0] - tm[1]),
                                                "within_process_max_minus_min": within},
                       "this_minus_parent_ms": statistics.mean(tm) - statistics.mean(pm),
                       "t2i_ms_per_step": [r["t2i_ms_per_step"] for r in (t1, t2)],
                       "edit_ms_per_step": [r["edit_ms_per_step"] for r in (t1, t2)],
                       "edit_no_mask_ms_per_step": [r["edit_no_mask_ms_per_step"] for r in (t1, t2)],
                       "encode_ms": [statistics.median(r["encode_ms"]) for r in (t1, t2)],
                       "edit_denoise_ms": [statistics.median(r["edit_denoise_ms"]) for r in (t1, t2)],
                       "decode_paste_ms": [r["decode_paste_ms"] for r in (t1, t2)], "decode_ms": [r["decode_ms"] for r in (t1, t2)],
                       "images_per_s": {"t2i_parent": [r["t2i_images_per_s"] for r in (p1, p2)], "t2i_this": [r["t2i_images_per_s"] for r in (t1, t2)],
                                        "edit": [r["edit_images_per_s"] for r in (t1, t2)]}}}
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res["summary"], indent=1))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--combine":
        combine(sys.argv[2:6], sys.argv[6])
    else:
        main()
