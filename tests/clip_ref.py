"""fp32 torch restatement of transformers' CLIPModel towers (image_embeds / text_embeds), CLIP's preprocessing in PIL and the two metrics of the
reference's eval_dreambooth.py -- the yardstick of textboost_amd/clip_score.py.  Host code only; pinned against transformers by
tests/test_clip_score_host.py."""
import os

import numpy as np
import torch
import torch.nn.functional as F

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def quick_gelu(x):
    return x * torch.sigmoid(1.702 * x)


def _layer(sd, lp, h, heads, eps, causal):
    B, T, D = h.shape
    hd = D // heads
    ln = lambda x, n: F.layer_norm(x, (D,), sd[f"{lp}{n}.weight"], sd[f"{lp}{n}.bias"], eps)
    lin = lambda x, n: F.linear(x, sd[f"{lp}{n}.weight"], sd[f"{lp}{n}.bias"])
    x = ln(h, "layer_norm1")
    q, k, v = (lin(x, f"self_attn.{n}_proj").reshape(B, T, heads, hd).transpose(1, 2) for n in "qkv")
    s = (q @ k.transpose(-1, -2)) * hd ** -0.5
    if causal:
        s = s.masked_fill(torch.ones(T, T, dtype=torch.bool).triu(1), float("-inf"))
    o = (s.softmax(-1) @ v).transpose(1, 2).reshape(B, T, D)
    h = h + lin(o, "self_attn.out_proj")
    x = ln(h, "layer_norm2")
    return h + lin(quick_gelu(lin(x, "mlp.fc1")), "mlp.fc2")


def normalise(images_u8):
    """uint8 [B, S, S, 3] -> CLIP pixel_values fp32 [B, 3, S, S] (ToTensor + Normalize)."""
    x = torch.as_tensor(np.asarray(images_u8)).float().permute(0, 3, 1, 2) / 255.0
    m, s = torch.tensor(CLIP_MEAN)[None, :, None, None], torch.tensor(CLIP_STD)[None, :, None, None]
    return (x - m) / s


def patch_embed(sd, pixel_values, pre="vision_model."):
    """embeddings of CLIPVisionModel: [B, 1 + P, D] (class row + conv patches, position embeddings added)."""
    w = sd[pre + "embeddings.patch_embedding.weight"]
    p = w.shape[-1]
    x = F.conv2d(pixel_values, w, stride=p).flatten(2).transpose(1, 2)
    B, D = x.shape[0], x.shape[2]
    cls = sd[pre + "embeddings.class_embedding"].expand(B, 1, D)
    return torch.cat([cls, x], dim=1) + sd[pre + "embeddings.position_embedding.weight"][None]


def vision_residuals(sd, cfg, pixel_values):
    """the residual stream after pre_layrnorm and after every layer (for locating a drifting layer)."""
    v = cfg["vision_config"]
    pre = "vision_model."
    eps = v.get("layer_norm_eps", 1e-5)
    h = patch_embed(sd, pixel_values)
    D = h.shape[-1]
    h = F.layer_norm(h, (D,), sd[pre + "pre_layrnorm.weight"], sd[pre + "pre_layrnorm.bias"], eps)
    out = [h]
    for i in range(v["num_hidden_layers"]):
        h = _layer(sd, f"{pre}encoder.layers.{i}.", h, v["num_attention_heads"], eps, causal=False)
        out.append(h)
    return out


def image_embeds(sd, cfg, pixel_values):
    v = cfg["vision_config"]
    pre = "vision_model."
    h = vision_residuals(sd, cfg, pixel_values)[-1]
    D = h.shape[-1]
    pooled = F.layer_norm(h[:, 0], (D,), sd[pre + "post_layernorm.weight"], sd[pre + "post_layernorm.bias"], v.get("layer_norm_eps", 1e-5))
    return pooled @ sd["visual_projection.weight"].t()


def text_embeds(sd, cfg, input_ids):
    """pooled at the first EOS of each row (transformers with a non-legacy eos_token_id, open_clip's argmax over ids)."""
    t = cfg["text_config"]
    pre = "text_model."
    eos = t.get("eos_token_id", 49407)
    eps = t.get("layer_norm_eps", 1e-5)
    ids = torch.as_tensor(input_ids)
    B, T = ids.shape
    h = sd[pre + "embeddings.token_embedding.weight"][ids] + sd[pre + "embeddings.position_embedding.weight"][:T][None]
    for i in range(t["num_hidden_layers"]):
        h = _layer(sd, f"{pre}encoder.layers.{i}.", h, t["num_attention_heads"], eps, causal=True)
    D = h.shape[-1]
    h = F.layer_norm(h, (D,), sd[pre + "final_layer_norm.weight"], sd[pre + "final_layer_norm.bias"], eps)
    pooled = h[torch.arange(B), (ids == eos).int().argmax(dim=1)]
    return pooled @ sd["text_projection.weight"].t()


# ---------------------------------------------------------------------------------------------------- preprocessing (PIL, host)
def pil_preprocess(rgb, size, clip_i):
    """uint8 [H, W, 3] -> uint8 [size, size, 3]: (BILINEAR to 512 x 512 for CLIP-I), BICUBIC shortest edge -> size, centre crop."""
    from PIL import Image
    im = Image.fromarray(np.asarray(rgb))
    if clip_i:
        im = im.resize((512, 512), Image.BILINEAR)
    w, h = im.size
    short, long = (w, h) if w <= h else (h, w)
    new_long = int(size * long / short)
    nw, nh = (size, new_long) if w <= h else (new_long, size)
    if (nw, nh) != (w, h):
        im = im.resize((nw, nh), Image.BICUBIC)
    left, top = int(round((nw - size) / 2.0)), int(round((nh - size) / 2.0))
    return np.asarray(im.crop((left, top, left + size, top + size)))


# ---------------------------------------------------------------------------------------------------- metrics (eval_dreambooth.py)
def clip_t(img_emb, txt_emb):
    a = img_emb / img_emb.norm(dim=-1, keepdim=True)
    b = txt_emb / txt_emb.norm(dim=-1, keepdim=True)
    return (a * b).sum(-1)


def clip_i(gen_by_instance, real_by_instance):
    """eval_dreambooth.py:426-449: per instance, per real image, max(cosine_similarity(generated, real), 0); concatenated."""
    scores = []
    for inst, g in gen_by_instance.items():
        for r in real_by_instance[inst].unbind(0):
            s = torch.cosine_similarity(g, r[None], dim=1)
            scores.append(torch.maximum(s, torch.zeros_like(s)))
    return torch.cat(scores)


def prompt_of(path):
    return os.path.basename(path).replace(".png", "").replace("_", " ")
