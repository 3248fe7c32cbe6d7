"""fp32 torch restatement of the hub's DINOv2 forward (dinov2/models/vision_transformer.py `DinoVisionTransformer.forward` of
`dinov2_vitl14`: the CLS row after the final LayerNorm, position embeddings interpolated with the hub's offset), the reference's PIL
preprocessing and the DINO score's per-instance means (eval_dreambooth.py:456-543), restated -- the yardstick of textboost_amd/dino_score.py.
Host code only; pinned against transformers' Dinov2Model by tests/test_dino_score_host.py.  [3P restated: torch.hub, the dinov2 package and
torchvision are not installed here.]"""
import math

import numpy as np
import torch
import torch.nn.functional as F

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


def hub_interpolate_pos_encoding(pos_embed, npatch, w, h, patch_size, offset=0.1):
    """DinoVisionTransformer.interpolate_pos_encoding (interpolate_antialias=False, interpolate_offset=offset); w, h: the input's pixel sizes
    as the hub names them (`B, nc, w, h = x.shape`)"""
    N = pos_embed.shape[1] - 1
    if npatch == N and w == h:
        return pos_embed
    pos_embed = pos_embed.float()
    class_pos_embed, patch_pos_embed = pos_embed[:, 0], pos_embed[:, 1:]
    dim = pos_embed.shape[-1]
    w0, h0 = w // patch_size, h // patch_size
    M = int(math.sqrt(N))
    assert N == M * M
    sx, sy = float(w0 + offset) / M, float(h0 + offset) / M
    patch_pos_embed = F.interpolate(patch_pos_embed.reshape(1, M, M, dim).permute(0, 3, 1, 2), mode="bicubic", antialias=False,
                                    scale_factor=(sx, sy))
    assert (w0, h0) == patch_pos_embed.shape[-2:]
    patch_pos_embed = patch_pos_embed.permute(0, 2, 3, 1).view(1, -1, dim)
    return torch.cat((class_pos_embed.unsqueeze(0), patch_pos_embed), dim=1)


def features(sd, pixel_values, num_heads, eps=1e-6, offset=0.1):
    """`model(x)` of the hub's DinoVisionTransformer (head = Identity) on a hub-named fp32 state dict: [B, D]"""
    w = sd["patch_embed.proj.weight"]
    p = w.shape[-1]
    B, _, Wpx, Hpx = pixel_values.shape
    x = F.conv2d(pixel_values, w, sd["patch_embed.proj.bias"], stride=p).flatten(2).transpose(1, 2)
    D = x.shape[-1]
    x = torch.cat((sd["cls_token"].expand(B, -1, -1), x), dim=1)
    x = x + hub_interpolate_pos_encoding(sd["pos_embed"], x.shape[1] - 1, Wpx, Hpx, p, offset)
    T = x.shape[1]
    hd = D // num_heads
    n_blocks = len({k.split(".")[1] for k in sd if k.startswith("blocks.")})
    ln = lambda t, n: F.layer_norm(t, (D,), sd[n + ".weight"], sd[n + ".bias"], eps)
    lin = lambda t, n: F.linear(t, sd[n + ".weight"], sd[n + ".bias"])
    for i in range(n_blocks):
        b = f"blocks.{i}."
        qkv = lin(ln(x, b + "norm1"), b + "attn.qkv").reshape(B, T, 3, num_heads, hd).permute(2, 0, 3, 1, 4)
        q, k, v = qkv[0] * hd ** -0.5, qkv[1], qkv[2]
        a = (q @ k.transpose(-2, -1)).softmax(dim=-1)
        o = (a @ v).transpose(1, 2).reshape(B, T, D)
        x = x + lin(o, b + "attn.proj") * sd[b + "ls1.gamma"]
        x = x + lin(F.gelu(lin(ln(x, b + "norm2"), b + "mlp.fc1")), b + "mlp.fc2") * sd[b + "ls2.gamma"]
    return ln(x, "norm")[:, 0]


# ---------------------------------------------------------------------------------------------------- preprocessing (PIL, host)
def pil_preprocess(rgb):
    """uint8 [H, W, 3] -> uint8 [224, 224, 3]: `v2.Resize((512, 512))`, `v2.Resize((224, 224))` on a PIL image (Pillow BILINEAR twice)"""
    from PIL import Image
    im = Image.fromarray(np.asarray(rgb)).resize((512, 512), Image.BILINEAR).resize((224, 224), Image.BILINEAR)
    return np.asarray(im)


def normalise(images_u8):
    """uint8 [B, S, S, 3] -> fp32 [B, 3, S, S] (ToTensor + ImageNet Normalize)"""
    x = torch.as_tensor(np.asarray(images_u8)).float().permute(0, 3, 1, 2) / 255.0
    m, s = torch.tensor(IMAGENET_MEAN)[None, :, None, None], torch.tensor(IMAGENET_STD)[None, :, None, None]
    return (x - m) / s


# ---------------------------------------------------------------------------------------------------- the metric (eval_dreambooth.py)
def padded_means(gen_features, gen_instances, real_features, N):
    """the DINO score's semantics (eval_dreambooth.py `dino_score`) restated on features with one padded tensor: real_features = {instance:
    [n_i, D]}, gen_features [G, D] with the instance name of each row in gen_instances -> (seen [G], unseen [G]).  Every instance's real rows
    are padded with zero rows to the largest n_i; a boolean mask per (instance, column) marks the seen columns (j < N) and the unseen ones
    (N <= j < n_i); a generated image's score is the masked mean of its cosines to its instance's columns."""
    names = list(real_features)
    counts = torch.tensor([real_features[k].shape[0] for k in names])
    width, D = int(counts.max()), gen_features.shape[1]
    padded = torch.zeros(len(names), width, D)
    for r, k in enumerate(names):
        padded[r, :counts[r]] = real_features[k]
    col = torch.arange(width)[None, :]
    seen_mask = (col < N).expand(len(names), width)
    unseen_mask = (col >= N) & (col < counts[:, None])
    rows = torch.tensor([names.index(k) for k in gen_instances])
    cos = F.cosine_similarity(gen_features[:, None, :], padded[rows], dim=-1)   # [G, width], padded columns included
    out = []
    for mask in (seen_mask[rows], unseen_mask[rows]):
        w = mask.to(cos.dtype)
        out.append((cos * w).sum(dim=1) / w.sum(dim=1))
    return out[0], out[1]
