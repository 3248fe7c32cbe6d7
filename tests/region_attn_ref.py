"""float64 reference of the regional cross-attention forward (csrc/region_attn.hip), on the rounded operands:

    O[b, s, h] = sum_j P[b, h, s, j] V[b, j, h],   P = softmax_j(scale q_{b,h,s} . k_{b,h,j} + m[b, s, j])
    m[b, s, j] = 0 if key_region[b, j] < 0 or bit key_region[b, j] of query_regions[s] is set, -inf otherwise
    LSE[b, h, s] = log sum_j exp(scale q . k_j + m)          (natural log; -inf, with O = 0, when every key of the query is masked)

Q / O are [B * Sq, H * hd], K / V [B * Skv, H * hd] (head h in columns [h hd, (h + 1) hd)), key_region int [B, Skv], query_regions the uint32 bit
words as any integer tensor / array [Sq] (an int32 tensor holds bit 31 as its sign: it is read back unsigned)."""
import numpy as np
import torch


def allowed(key_region, query_regions):
    """bool [B, Sq, Skv]"""
    kr = torch.as_tensor(np.asarray(key_region)).long()                                  # [B, Skv]
    qb = torch.as_tensor(np.asarray(query_regions).astype(np.int64) & 0xFFFFFFFF)        # [Sq], unsigned
    bit = (qb[None, :, None] >> kr.clamp(min=0)[:, None, :]) & 1
    return (kr[:, None, :] < 0) | (bit == 1)


def ref_region_attention(Q, K, V, B, H, Sq, Skv, hd, scale, key_region, query_regions):
    """-> (O float64 [B * Sq, H * hd], LSE float64 [B, H, Sq], P float64 [B, H, Sq, Skv])"""
    q = Q.double().view(B, Sq, H, hd).permute(0, 2, 1, 3)
    k = K.double().view(B, Skv, H, hd).permute(0, 2, 1, 3)
    v = V.double().view(B, Skv, H, hd).permute(0, 2, 1, 3)
    s = scale * (q @ k.transpose(-1, -2))                                                # [B, H, Sq, Skv]
    ok = allowed(key_region, query_regions)[:, None]                                     # [B, 1, Sq, Skv]
    s = torch.where(ok, s, torch.full_like(s, -float("inf")))
    mx = s.max(dim=-1, keepdim=True).values
    mx = torch.where(torch.isinf(mx), torch.zeros_like(mx), mx)
    e = torch.exp(s - mx)                                                                # masked: exp(-inf) = 0 exactly
    den = e.sum(dim=-1, keepdim=True)
    P = torch.where(den > 0, e / den.clamp(min=1e-300), torch.zeros_like(e))
    lse = torch.where(den[..., 0] > 0, mx[..., 0] + torch.log(den[..., 0].clamp(min=1e-300)), torch.full_like(den[..., 0], -float("inf")))
    O = (P @ v).permute(0, 2, 1, 3).reshape(B * Sq, H * hd)
    return O, lse, P


def ref_attention(Q, K, V, B, H, Sq, Skv, hd, scale):
    """plain softmax attention, float64 (no mask anywhere in its arithmetic)"""
    q = Q.double().view(B, Sq, H, hd).permute(0, 2, 1, 3)
    k = K.double().view(B, Skv, H, hd).permute(0, 2, 1, 3)
    v = V.double().view(B, Skv, H, hd).permute(0, 2, 1, 3)
    s = scale * (q @ k.transpose(-1, -2))
    P = torch.softmax(s, dim=-1)
    return (P @ v).permute(0, 2, 1, 3).reshape(B * Sq, H * hd), torch.logsumexp(s, dim=-1)


def rel_l2(got, ref):
    return ((got.double() - ref.double()).norm() / ref.double().norm().clamp(min=1e-300)).item()
