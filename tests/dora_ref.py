"""Reference side of --use_dora (peft 0.13.2 `DoraLinearLayer`, restated): the oracle's `LoRALinear`s get a magnitude parameter
`lora_magnitude_vector` [N] and the forward

    n = || W + s B A ||_2 per output row, DETACHED (peft, DoRA paper section 4.3)      c = m / n
    y = c * (x W^T + s (x A^T) B^T) + b

in whatever dtype the module is in (float64 after `.double()`).  The parameter's name contains "lora_", so `TextBoostEncoder.lora_parameters()`
and the oracle step pick it up; the step's mixing rule selects "lora_B" and leaves it alone.  Per layer the order of the adapter parameters is
q, k, v, out, fc1, fc2 and A, B, m inside a module (registration order).  Keys: peft saves `lora_magnitude_vector.default.weight` as
`<module>.lora_magnitude_vector`."""
import types

import torch
import torch.nn.functional as F
from torch import nn

import lora_targets_ref as LT


def mkey(i, name):
    return f"base_model.model.text_model.encoder.layers.{i}.{LT.PATH[name]}.lora_magnitude_vector"


def direction_norm(m):
    """|| W + s B A ||_2 per output row of one adapted module"""
    return (m.weight + m.scaling * (m.lora_B @ m.lora_A)).norm(dim=1)


def dora_forward(self, x):
    n = direction_norm(self)
    if self.dora_detach:
        n = n.detach()
    c = self.lora_magnitude_vector / n
    u = F.linear(x, self.weight) + F.linear(F.linear(x, self.lora_A), self.lora_B) * self.scaling
    return c * u + self.bias


def make_dora(module, detach=True):
    """turn one adapted oracle `LoRALinear` into a DoRA layer, m = || W + s B A || of its current weights (peft's init: with B = 0, || W ||)"""
    assert module.r > 0
    with torch.no_grad():
        module.lora_magnitude_vector = nn.Parameter(direction_norm(module).detach().clone())
    module.dora_detach = detach
    module.forward = types.MethodType(dora_forward, module)
    return module


def add_dora(enc, detach=True, perturb=0.0, seed=0):
    """every adapted module of an oracle encoder becomes a DoRA layer; perturb > 0: m *= 1 + perturb * N(0, 1), so that c != 1 and the
    magnitude path is live"""
    g = torch.Generator().manual_seed(seed)
    for layer in enc.layers:
        for n in LT.adapted(enc):
            m = make_dora(getattr(layer, LT.ATTR[n]), detach)
            if perturb:
                with torch.no_grad():
                    m.lora_magnitude_vector.mul_(1 + perturb * torch.randn(m.lora_magnitude_vector.shape, generator=g).to(m.lora_magnitude_vector))
    return enc


def peft_state_dict(enc):
    sd = LT.peft_state_dict(enc)
    for i, layer in enumerate(enc.layers):
        for n in LT.adapted(enc):
            sd[mkey(i, n)] = getattr(layer, LT.ATTR[n]).lora_magnitude_vector.detach().clone()
    return sd


def load_peft_state_dict(enc, sd):
    LT.load_peft_state_dict(enc, {k: v for k, v in sd.items() if not k.endswith(".lora_magnitude_vector")})
    with torch.no_grad():
        for i, layer in enumerate(enc.layers):
            for n in LT.adapted(enc):
                getattr(layer, LT.ATTR[n]).lora_magnitude_vector.copy_(sd[mkey(i, n)])


def magnitudes(enc):
    """{"qkv": [L, 3D], extra module: [L, N]} of an oracle DoRA encoder, keyed like HipTextEncoder"""
    out = {"qkv": torch.stack([torch.cat([l.q.lora_magnitude_vector, l.k.lora_magnitude_vector, l.v.lora_magnitude_vector]) for l in enc.layers]).detach()}
    for n in LT.adapted(enc)[3:]:
        out[n] = torch.stack([getattr(l, LT.ATTR[n]).lora_magnitude_vector for l in enc.layers]).detach()
    return out


def copy_to_hip(enc, hip):
    """adapters and magnitudes of the oracle into a HipTextEncoder(use_dora=True) with the same modules"""
    LT.copy_to_hip(enc, hip)
    for n, m in magnitudes(enc).items():
        hip._dora_of(n).mag.copy_(m)


def oracle_grads(enc):
    """-> (gA, gB, {extra: (gA, gB)}, {"qkv" | extra: gm}) from the .grad of an oracle DoRA encoder"""
    gA, gB, gx = LT.oracle_grads(enc)
    gm = {"qkv": torch.stack([torch.cat([l.q.lora_magnitude_vector.grad, l.k.lora_magnitude_vector.grad, l.v.lora_magnitude_vector.grad])
                              for l in enc.layers])}
    for n in LT.adapted(enc)[3:]:
        gm[n] = torch.stack([getattr(l, LT.ATTR[n]).lora_magnitude_vector.grad for l in enc.layers])
    return gA, gB, gx, gm


def split_step_grads(g_lora, enc):
    """the oracle step's `g_lora` list (lora_parameters() order: A, B, m per module) -> the same four as `oracle_grads`"""
    names = LT.adapted(enc)
    per = 3 * len(names)
    L = len(enc.layers)
    at = lambda l, n, j: g_lora[per * l + 3 * names.index(n) + j]   # noqa: E731
    gA = torch.stack([torch.cat([at(l, n, 0) for n in LT.QKV]) for l in range(L)])
    gB = torch.stack([torch.cat([at(l, n, 1) for n in LT.QKV]) for l in range(L)])
    gx = {n: (torch.stack([at(l, n, 0) for l in range(L)]), torch.stack([at(l, n, 1) for l in range(L)])) for n in names[3:]}
    gm = {"qkv": torch.stack([torch.cat([at(l, n, 2) for n in LT.QKV]) for l in range(L)])}
    for n in names[3:]:
        gm[n] = torch.stack([at(l, n, 2) for l in range(L)])
    return gA, gB, gx, gm


def dora_linear_f64(x, W, b, A, Bm, m, s=1.0):
    """the definition on plain tensors, float64: -> (y, u, n, c)"""
    x, W, A, Bm, m = (t.double() for t in (x, W, A, Bm, m))
    n = (W + s * (Bm @ A)).norm(dim=1)
    c = m / n
    u = x @ W.T + s * (x @ A.T) @ Bm.T
    return c * u + (0 if b is None else b.double()), u, n, c
