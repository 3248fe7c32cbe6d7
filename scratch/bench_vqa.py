"""Throughput of the VQA score's CLIP-FlanT5 forward at full size: FlanT5-XXL + CLIP ViT-L/14@336px with random weights drawn on the device tensor
by tensor (~22 GB in bf16), B = 32 images, prompts of the evaluation's length (about 620 encoder tokens).  Images / s from device events after
warm-up; --json PATH writes the result.  Under `rocprofv3 --kernel-trace --stats -- python scratch/bench_vqa.py --steps 1` the same run gives
the per-kernel split quoted in DESIGN.md section 12."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def random_tensors(geo, seed, device):
    """(name, tensor) one at a time: N(0, 1 / fan_in) matrices (lm_head x 3), N(0, 1) embeddings, norm weights 1 + 0.1 N, bias tables 2 N"""
    from textboost_amd.vqa_score import t5_tensor_shapes
    g = torch.Generator(device=device).manual_seed(seed)
    for k, shp in t5_tensor_shapes(geo).items():
        r = torch.randn(shp, generator=g, device=device)
        if k.endswith("layer_norm.weight"):
            r = 1.0 + 0.1 * r
        elif k.endswith(".bias"):
            r = 0.1 * r
        elif "relative_attention_bias" in k:
            r = 2.0 * r
        elif k != "shared.weight":
            r = r * shp[1] ** -0.5 * (3.0 if k == "lm_head.weight" else 1.0)
        yield k, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--text-tokens", type=int, default=44, help="text ids per prompt around the 576 image rows")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--layers", type=int, default=24, help="encoder and decoder layers (24 = FlanT5-XXL)")
    ap.add_argument("--json", type=str, default=None)
    a = ap.parse_args()
    from textboost_amd import _lib as L, models
    from textboost_amd import vqa_score as V
    from textboost_amd.clip_score import HipCLIPVision
    torch.cuda.set_device(0)
    dev = "cuda"
    vg = models.CLIP_VIT_L14_336
    with L.use_half("bf16"):
        vision = HipCLIPVision(vg, models.random_state_dict(models.clip_model_shapes(vg, models.CLIP_VIT_L14_TEXT), 9), device=dev)
    geo = V.T5Geometry(num_layers=a.layers, num_decoder_layers=a.layers)
    model = V.HipCLIPFlanT5(geo, random_tensors(geo, 1, dev), vision, device=dev)
    g = torch.Generator().manual_seed(2)
    B = a.batch
    images = torch.randint(0, 1 << 24, (B, vg.image_size, vg.image_size), generator=g, dtype=torch.int32).to(dev)
    n_head = 30
    ids = [torch.randint(3, geo.vocab_size, (n_head,), generator=g).tolist() + [1, V.IMAGE_TOKEN_INDEX]
           + torch.randint(3, geo.vocab_size, (a.text_tokens - n_head - 2 - (b % 3),), generator=g).tolist() + [1] for b in range(B)]
    labels, dec = [2163, 1], [0, 2163]
    T = max(len(r) for r in ids) - 1 + vg.num_patches
    for _ in range(a.warmup):
        s = model.scores(images, ids, labels, dec)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(a.steps):
        e0.record()
        s = model.scores(images, ids, labels, dec)
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) / 1e3)
    assert torch.isfinite(s).all(), s
    best, mean = min(times), sum(times) / len(times)
    res = {"batch": B, "encoder_tokens": T, "layers": a.layers, "steps": a.steps, "warmup": a.warmup, "seconds_per_batch_mean": mean,
           "seconds_per_batch_min": best, "images_per_second": B / mean, "weights_gb": torch.cuda.memory_allocated() / 2 ** 30,
           "device": torch.cuda.get_device_name(0)}
    print(json.dumps(res))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
