"""Writes tests/golden/clip_vit_tiny.pt: a tiny random transformers CLIPModel (image_size 224, patch 14 -> 257 tokens, head dim 64; weights
rounded to and stored as fp16, the model run on exactly those values), a few uint8 images of odd sizes, the SHA-256 of their Pillow-preprocessed
bytes (CLIP-I: BILINEAR to 512 x 512, then BICUBIC shortest edge + centre crop; CLIP-T: the same without the 512 step; the bytes themselves
would be megabytes) and transformers' outputs on them: the unnormalised image_embeds / text_embeds and the CLIP-T scores.

Run on a host with transformers and Pillow (no GPU, no network):  python tests/golden/gen_clip_golden.py"""
import hashlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import clip_ref as R  # noqa: E402

SIZES = [(67, 99), (101, 70), (61, 60)]   # (H, W)
PROMPTS = ["a dog on the beach", "a red can", "a teapot with a city in the background"]


def config():
    V = 100
    return {"projection_dim": 32,
            "vision_config": {"image_size": 224, "patch_size": 14, "hidden_size": 64, "intermediate_size": 128, "num_hidden_layers": 2,
                              "num_attention_heads": 1, "hidden_act": "quick_gelu", "layer_norm_eps": 1e-5},
            "text_config": {"vocab_size": V, "hidden_size": 64, "intermediate_size": 128, "num_hidden_layers": 1, "num_attention_heads": 2,
                            "max_position_embeddings": 77, "hidden_act": "quick_gelu", "layer_norm_eps": 1e-5, "eos_token_id": V - 1,
                            "bos_token_id": V - 2, "pad_token_id": V - 1}}


def digest(u8) -> str:
    """SHA-256 of a uint8 [H, W, 3] image's bytes (row-major), with its shape"""
    a = np.ascontiguousarray(np.asarray(u8, dtype=np.uint8))
    return f"{a.shape[0]}x{a.shape[1]}x{a.shape[2]}:" + hashlib.sha256(a.tobytes()).hexdigest()


def smooth_image(h, w, rng):
    """gradients + a little noise: realistic enough for the resamplers, small enough to keep the fixture compact"""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    base = np.stack([127 + 120 * np.sin(x / (7 + 5 * c) + y / (11 + 3 * c) + c) for c in range(3)], axis=-1)
    return np.clip(base + rng.normal(0, 12, base.shape), 0, 255).astype(np.uint8)


def main():
    import transformers
    from textboost_amd import models
    from textboost_amd.clip_score import clip_model_geometry_from_config
    cfg = config()
    vg, tg, eos = clip_model_geometry_from_config(cfg)
    sd = {k: v.half().float() for k, v in models.random_state_dict(models.clip_model_shapes(vg, tg), 21).items()}
    m = transformers.CLIPModel(transformers.CLIPConfig(text_config=cfg["text_config"], vision_config=cfg["vision_config"],
                                                       projection_dim=cfg["projection_dim"])).eval()
    m.load_state_dict(sd, strict=False)
    rng = np.random.default_rng(7)
    images = [smooth_image(h, w, rng) for h, w in SIZES]
    from PIL import Image
    pre, digests = {}, {}
    for n, (size, clip_i) in {"clip_i_224": (224, True), "clip_t_224": (224, False), "clip_i_336": (336, True),
                              "clip_t_336": (336, False)}.items():
        pre[n] = np.stack([R.pil_preprocess(a, size, clip_i) for a in images])
        digests[n] = [digest(x) for x in pre[n]]
    digests["bilinear_512"] = [digest(np.asarray(Image.fromarray(a).resize((512, 512), Image.BILINEAR))) for a in images]
    g = torch.Generator().manual_seed(3)
    ids = torch.full((len(PROMPTS), 77), eos, dtype=torch.int64)
    for b, p in enumerate(PROMPTS):   # stand-in ids (the tokenizer is not what this fixture pins): BOS, one id per word, EOS
        n = len(p.split())
        ids[b, 0] = cfg["text_config"]["bos_token_id"]
        ids[b, 1:1 + n] = torch.randint(0, cfg["text_config"]["vocab_size"] - 2, (n,), generator=g)
    with torch.no_grad():
        emb = {}
        for n in ("clip_i_224", "clip_t_224"):
            emb[n] = m.visual_projection(m.vision_model(pixel_values=R.normalise(pre[n])).pooler_output)
        text = m.text_projection(m.text_model(input_ids=ids).pooler_output)
        scores = R.clip_t(emb["clip_t_224"], text)
    out = {"config": cfg, "state_dict_fp16": {k: v.half().contiguous() for k, v in sd.items()}, "images": [torch.from_numpy(a) for a in images],
           "preprocessed_sha256": digests, "input_ids": ids, "prompts": PROMPTS,
           "image_embeds": emb, "text_embeds": text, "clip_t_scores": scores}
    path = os.path.join(HERE, "clip_vit_tiny.pt")
    torch.save(out, path)
    print(f"wrote {path} ({os.path.getsize(path) / 1e6:.2f} MB); clip-t scores {scores.tolist()}")


if __name__ == "__main__":
    main()
