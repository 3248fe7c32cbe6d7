"""float64 references of prompt-to-prompt editing (textboost_amd/p2p.py, csrc/p2p_attn.hip), on the rounded operands.

    ref_dual_attention:  O = softmax(scale Q1 K1^T) V1 + softmax(scale Q2 K2^T) V2, each softmax over its own keys
    ref_p2p_cross:       the controlled cross-attention as DEFINED, with the probability row written out:
                         P_out[j] = w_j (a_j sum_i P^s[i] M[i, j] + (1 - a_j) P^e[j]),   O = sum_j P_out[j] v^e_j
                         (it never forms V1 / V2: the kernel path's algebra is what it checks)

Q / O are [B * Sq, H * hd], K / V [B * Skv, H * hd] (head h in columns [h hd, (h + 1) hd))."""
import torch


def _heads(X, B, S, H, hd):
    return X.double().view(B, S, H, hd).permute(0, 2, 1, 3)


def probabilities(Q, K, B, H, Sq, Skv, hd, scale):
    """float64 [B, H, Sq, Skv]"""
    return torch.softmax(scale * (_heads(Q, B, Sq, H, hd) @ _heads(K, B, Skv, H, hd).transpose(-1, -2)), dim=-1)


def ref_attention(Q, K, V, B, H, Sq, Skv, hd, scale):
    """plain softmax attention -> O float64 [B * Sq, H * hd]"""
    return (probabilities(Q, K, B, H, Sq, Skv, hd, scale) @ _heads(V, B, Skv, H, hd)).permute(0, 2, 1, 3).reshape(B * Sq, H * hd)


def ref_dual_attention(Q1, K1, V1, Q2, K2, V2, B, H, Sq, Skv1, Skv2, hd, scale):
    return ref_attention(Q1, K1, V1, B, H, Sq, Skv1, hd, scale) + ref_attention(Q2, K2, V2, B, H, Sq, Skv2, hd, scale)


def p_out(Ps, Pe, M, a, w):
    """the controlled probability rows: Ps / Pe float64 [..., T], M [T, T], a / w [T] -> [..., T]"""
    M, a, w = (torch.as_tensor(x).double() for x in (M, a, w))
    return w * (a * (Ps @ M) + (1.0 - a) * Pe)


def ref_p2p_cross(Qs, Ks, Qe, Ke, Ve, M, a, w, B, H, Sq, T, hd, scale):
    """Qs / Ks: the source rows' queries and keys, Qe / Ke / Ve: the edited rows' own -> O float64 [B * Sq, H * hd]"""
    P = p_out(probabilities(Qs, Ks, B, H, Sq, T, hd, scale), probabilities(Qe, Ke, B, H, Sq, T, hd, scale), M, a, w)
    return (P @ _heads(Ve, B, T, H, hd)).permute(0, 2, 1, 3).reshape(B * Sq, H * hd)


def rel_l2(got, ref):
    return ((got.double() - ref.double()).norm() / ref.double().norm().clamp(min=1e-300)).item()
