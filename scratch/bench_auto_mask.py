"""Measures one photo through textboost_amd/auto_mask.py at the real shapes: SD1.5 UNet / VAE geometry, random weights, a 512 x 512 photo,
6 UNet rows (timesteps 100 / 300 / 500, two draws each), 77 prompt tokens, the word at one position.  Device events around each phase:

  * prepare: pack the photo, the Lanczos squash to 512 x 512, bytes -> pixel values
  * encode:  the VAE encoder (the mode)
  * unet:    tb_add_noise + one UNet forward with the recorder set (and, for comparison, the same forward without it)
  * kernels: csrc/auto_mask.hip -- one tb_map_word_upsample per cross-attention resolution, range, histogram, Otsu, mask bytes; the dilation
             (radius 8) apart
  * total:   `MaskMaker.mask` + the copy of the mask to the host, by the wall clock

A first measurement of a new path: there is nothing to compare it with and no threshold on it (profiles/auto_mask_cost.json).

    python scratch/bench_auto_mask.py [out.json] [rounds]"""
import json
import os
import statistics
import sys
import time
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

dev = "cuda"
BOS, EOS, WORD = 49406, 49407, 1929


class Tokenizer:
    """"a photo of a WORD" as CLIP would tokenise it: six tokens between the start and end tokens, the word one piece"""
    bos_token_id, eos_token_id = BOS, EOS

    def __call__(self, text, truncation=True, padding=None, max_length=77, return_tensors=None, add_special_tokens=True):
        one = lambda t: [WORD] if not add_special_tokens else ([BOS, 320, 1125, 539, 320, WORD] + [EOS] * (max_length - 6))  # noqa: E731
        ids = [one(t) for t in text] if isinstance(text, (list, tuple)) else one(text)
        return types.SimpleNamespace(input_ids=torch.tensor(ids) if return_tensors == "pt" else ids)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    from textboost_amd import _lib, augment, models, ops
    from textboost_amd.auto_mask import MaskMaker
    from textboost_amd.unet import HipUNet
    from textboost_amd.vae import HipVAEEncoder, VAEGeometry, vae_encoder_shapes
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    R, size, S, T = 6, 64, 512, 77
    _lib.set_half("fp16")
    med = statistics.median
    with torch.no_grad():
        unet = HipUNet(models.SD15_UNET, models.random_state_dict(models.unet_shapes(models.SD15_UNET), 1, device=dev), R, size, size, text_len=T)
        hip_enc = HipVAEEncoder(VAEGeometry(), models.random_state_dict(vae_encoder_shapes(VAEGeometry()), 3, device=dev), 1, S, S, device=dev)
        zero = torch.zeros(1, 4, size, size, device=dev)
        enc = types.SimpleNamespace(size=size, S=S, encode=lambda px: hip_enc.encode(px, noise=zero).clone())
        states = torch.randn(R * T, 768, device=dev)
        acp = torch.cumprod(1.0 - torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000) ** 2, dim=0)
        maker = MaskMaker(unet, enc, lambda ids: states, Tokenizer(), acp)
        rgb = np.random.default_rng(0).integers(0, 256, (S, S, 3), dtype=np.uint8)
        rgb_wide = np.random.default_rng(1).integers(0, 256, (600, 800, 3), dtype=np.uint8)
        for _ in range(2):                                   # warm-up: every buffer and resample table exists
            mask, stats = maker.mask(rgb, "word", dilate=8)
        torch.cuda.synchronize()
        ehs = states.to(_lib.half_dtype()).contiguous()
        rec = maker.recorder

        def prepare(photo=rgb):
            img = augment.resize(augment.to_device_image(photo), (S, S), augment.LANCZOS)
            ops.img_to_pixels(img, 0, 0, maker.pixels[0])

        def forward(record):
            ops.add_noise(maker.x0, maker.noise, maker.t_dev, maker.acp, maker.noisy)
            rec.zero()
            unet.attn_maps = rec if record else None
            try:
                unet.forward(maker.noisy, maker.t_dev, ehs)
            finally:
                unet.attn_maps = None

        def kernels():
            maker.mask_of(maker.fuse([5], S, S))

        hard = maker.mask_of(maker.fuse([5], S, S))[0].clone()

        def total():
            t0 = time.perf_counter()
            m, _ = maker.mask(rgb, "word")
            m.cpu()
            return (time.perf_counter() - t0) * 1e3

        res = {"device": torch.cuda.get_device_name(0), "rounds": rounds,
               "setting": "SD1.5 UNet / VAE geometry, random weights, fp16 library, 512 x 512 photo, 6 UNet rows (timesteps 100 / 300 / 500 x 2 draws), "
                          "77 tokens, the word at one position; medians of device-event times over `rounds` calls; scratch/bench_auto_mask.py",
               "resolutions": {f"{h}x{w}": n for (h, w), n in rec.layers.items()},
               "prepare_ms": med([timed(prepare) for _ in range(rounds)]),
               "prepare_800x600_ms": med([timed(lambda: prepare(rgb_wide)) for _ in range(rounds)]),
               "encode_ms": med([timed(lambda: maker.encoder.encode(maker.pixels)) for _ in range(rounds)]),
               "unet_forward_with_recorder_ms": med([timed(lambda: forward(True)) for _ in range(rounds)]),
               "unet_forward_without_recorder_ms": med([timed(lambda: forward(False)) for _ in range(rounds)])}
        forward(True)
        res["new_kernels_ms"] = med([timed(kernels) for _ in range(rounds)])
        res["dilate_radius_8_ms"] = med([timed(lambda: ops.mask_dilate(hard, 8)) for _ in range(rounds)])
        res["dilate_radius_64_ms"] = med([timed(lambda: ops.mask_dilate(hard, 64)) for _ in range(rounds)])
        res["mask_call_wall_ms"] = med([total() for _ in range(rounds)])
        res["ms_per_photo"] = res["prepare_ms"] + res["encode_ms"] + res["unet_forward_with_recorder_ms"] + res["new_kernels_ms"]
    print(json.dumps(res, indent=1))
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
