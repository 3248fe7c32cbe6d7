"""Measures the image-generation path of textboost_amd/generate.py at the real shapes (SD1.5 UNet / VAE / CLIP-L geometry, random weights, 64^2
latents -> 512^2 images, 25 DPM-Solver++ steps, guidance 7.5):

  1. throughput of one prompt batch as built (13 prompts): denoise and decode + finish by device events, download and PNG writing by wall time;
  2. the parent's validation path (HipSampler.sample + make_image_grid) on the same box, 4 images, as DESIGN.md 8(f).2 quotes it;
  3. the finish step at B = 16, 512^2: decode_rgbx + one download against decode + make_image_grid's torch expression + download, alternating,
     median of 25 runs each;
  4. peak device memory with the UNet executor at batch 26 (2 x 13) and at batch 32 (2 x 16).

    python scratch/bench_generate.py [out.json]"""
import json
import os
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from textboost_amd import generate as G  # noqa: E402
from textboost_amd import models  # noqa: E402
from textboost_amd.sampler import HipSampler, make_image_grid  # noqa: E402
from textboost_amd.unet import HipUNet  # noqa: E402
from textboost_amd.vae import HipVAEDecoder, VAEGeometry, vae_decoder_shapes  # noqa: E402

dev = "cuda"


def events(fn, n):
    out = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out


def main():
    res = {"device": torch.cuda.get_device_name(0)}
    usd = models.random_state_dict(models.unet_shapes(models.SD15_UNET), 1, device=dev)
    vsd = models.random_state_dict(vae_decoder_shapes(VAEGeometry()), 2, device=dev)
    with torch.no_grad():
        # ---- 1. one prompt batch as built
        B = max(len(b) for b in G.prompt_batches(list(range(25)), 16))
        torch.cuda.reset_peak_memory_stats()
        pipe = G.Pipeline(models.SD15_UNET, usd, VAEGeometry(), vsd, None, 64, B)
        cond = torch.randn(B * 77, 768, device=dev)
        uncond = torch.randn(B * 77, 768, device=dev)
        lat = G.seeded_latent(0, 64).to(dev).repeat(B, 1, 1, 1)
        pipe.images(cond, uncond, lat)                      # warm-up batch
        torch.cuda.synchronize()
        res["peak_GiB_unet26_decoder13"] = torch.cuda.max_memory_allocated() / 2 ** 30
        den = events(lambda: pipe.sampler.denoise(cond, uncond, latents=lat), 3)
        x = pipe.sampler.denoise(cond, uncond, latents=lat).clone()
        dec = events(lambda: pipe.vae.decode_rgbx(x), 5)
        img = pipe.vae.decode_rgbx(x)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = img.cpu().numpy()
        t_down = time.perf_counter() - t0
        tmp = tempfile.mkdtemp()
        png = []
        with ThreadPoolExecutor(max_workers=G.MAX_PNG_THREADS) as pool:
            for rep in range(3):
                t0 = time.perf_counter()
                list(pool.map(lambda k: G._save_png(host[k], os.path.join(tmp, f"{rep}_{k}.png")), range(B)))
                png.append(time.perf_counter() - t0)
            # the loop as generate_instance runs it: PNG threads beside the next batch
            t0 = time.perf_counter()
            jobs = []
            nb = 4
            for rep in range(nb):
                h = pipe.images(cond, uncond, lat).cpu().numpy()
                jobs += [pool.submit(G._save_png, h[k], os.path.join(tmp, f"l{rep}_{k}.png")) for k in range(B)]
            for j in jobs:
                j.result()
            t_loop = time.perf_counter() - t0
        res["generate"] = {"prompt_batch": B, "steps": 25, "denoise_ms": statistics.median(den), "decode_finish_ms": statistics.median(dec),
                           "download_ms": t_down * 1e3, "png_13_images_8_threads_ms": statistics.median(png) * 1e3,
                           "random_image_png_note": "random weights give noise-like images: zlib's worst case",
                           "loop_images_per_s": nb * B / t_loop,
                           "device_only_images_per_s": B / ((statistics.median(den) + statistics.median(dec)) * 1e-3)}
        del pipe
        torch.cuda.empty_cache()
        # ---- 2. the parent's validation path, 4 images
        n = 4
        smp = HipSampler(HipUNet(models.SD15_UNET, usd, 2 * n, 64, 64, device=dev), HipVAEDecoder(VAEGeometry(), vsd, n, 64, 64, device=dev),
                         steps=25, guidance=7.5)
        c4, u4 = torch.randn(n * 77, 768, device=dev).half(), torch.randn(n * 77, 768, device=dev).half()
        make_image_grid(smp.sample(c4, u4), 1, n)
        torch.cuda.synchronize()
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            make_image_grid(smp.sample(c4, u4), 1, n)
            ts.append(time.perf_counter() - t0)
        res["validation_path_4_images"] = {"seconds": statistics.median(ts), "images_per_s": n / statistics.median(ts)}
        del smp
        torch.cuda.empty_cache()
        # ---- 3. the finish step, B = 16 at 512^2
        B16 = 16
        d16 = HipVAEDecoder(VAEGeometry(), vsd, B16, 64, 64, device=dev)
        z = torch.randn(B16, 4, 64, 64, device=dev) * 0.18215

        def new():
            return d16.decode_rgbx(z).cpu()

        def old():
            images = d16.decode(z)
            return (images.clamp(0, 1) * 255).round().to(torch.uint8).permute(0, 2, 3, 1).cpu()
        new(); old()
        t_new, t_old = [], []
        for _ in range(25):
            for fn, acc in ((new, t_new), (old, t_old)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                acc.append((time.perf_counter() - t0) * 1e3)
        rgb = d16._decode_rgb(z)[0]
        only_new = events(lambda: d16.decode_rgbx(z), 5)
        only_dec = events(lambda: d16._decode_rgb(z), 5)
        res["finish_B16_512"] = {"decode_rgbx_download_ms": statistics.median(t_new), "decode_torch_bytes_download_ms": statistics.median(t_old),
                                 "decoder_alone_ms": statistics.median(only_dec), "decoder_plus_rgbx_kernel_ms": statistics.median(only_new),
                                 "runs_each": 25, "rgb_rows": list(rgb.shape)}
        del d16
        torch.cuda.empty_cache()
        # ---- 4. peak memory of the UNet executor at batch 32
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        u32 = HipUNet(models.SD15_UNET, usd, 32, 64, 64, device=dev)
        u32.forward(torch.randn(32, 4, 64, 64, device=dev).half(), torch.full((32,), 500, dtype=torch.int64, device=dev),
                    torch.randn(32 * 77, 768, device=dev).half())
        torch.cuda.synchronize()
        res["unet_batch32"] = {"peak_GiB_over_weights_source": (torch.cuda.max_memory_allocated() - base) / 2 ** 30,
                               "total_device_GiB": torch.cuda.get_device_properties(0).total_memory / 2 ** 30}
    print(json.dumps(res, indent=1))
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
