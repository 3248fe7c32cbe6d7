"""float64 references of the token attention maps (textboost_amd/attn_maps.py, csrc/attn_maps.hip) in plain torch on the CPU.  The tests round
Q and K to the build's half type first; the references compute on those rounded values."""
import torch
import torch.nn.functional as F


def _probabilities(Q, K, B, H, Sq, Skv, hd, scale, dtype):
    """softmax_j(scale q k^T): [B, H, Sq, Skv] in `dtype`; Q [B*Sq, >= H*hd], K [B*Skv, >= H*hd] (the leading H*hd columns are read)"""
    q = Q.detach().cpu()[:, :H * hd].to(dtype).view(B, Sq, H, hd).permute(0, 2, 1, 3)
    k = K.detach().cpu()[:, :H * hd].to(dtype).view(B, Skv, H, hd).permute(0, 2, 1, 3)
    return torch.softmax((q @ k.transpose(-1, -2)) * scale, dim=-1)


def ref_token_maps(Q, K, B, H, Sq, Skv, hd, scale, dtype=torch.float64):
    """the head MEAN of the softmax, [B, Skv, Sq] (one image over the queries per key).  dtype = float32 gives the fp32 evaluation of the same
    formula, whose error against float64 is the yardstick of the kernel's."""
    return _probabilities(Q, K, B, H, Sq, Skv, hd, scale, dtype).mean(dim=1).transpose(1, 2).contiguous()


def ref_result(acc, count, h, w):
    """AttnMapRecorder.result(): acc {(h_l, w_l): [nb, T, h_l * w_l]}, count {(h_l, w_l): launches} -> float64 [nb, T, h, w]"""
    out = 0
    for hw, a in acc.items():
        m = (a.detach().cpu().double() / count[hw]).view(a.shape[0], a.shape[1], hw[0], hw[1])
        if hw != (h, w):
            m = F.interpolate(m, size=(h, w), mode="bicubic", align_corners=False)
        out = out + m
    return out / len(acc)
