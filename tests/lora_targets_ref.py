"""Reference side of --lora_target_modules: the oracle's `layer.out / fc1 / fc2` are `LoRALinear`s with r = 0; this gives them adapters and maps
all six adapted modules to and from the peft key layout.  `TextBoostEncoder.lora_parameters()` and the oracle step's mixing rule select by the
substring "lora_", so they pick the new parameters up; their order per layer is q, k, v, out, fc1, fc2 (A before B), the module order of
`CLIPLayer`."""
import torch
from torch import nn

QKV = ("q_proj", "k_proj", "v_proj")
EXTRA = ("out_proj", "fc1", "fc2")
ALL = QKV + EXTRA
ATTR = {"q_proj": "q", "k_proj": "k", "v_proj": "v", "out_proj": "out", "fc1": "fc1", "fc2": "fc2"}          # attribute of oracle CLIPLayer
PATH = {"q_proj": "self_attn.q_proj", "k_proj": "self_attn.k_proj", "v_proj": "self_attn.v_proj", "out_proj": "self_attn.out_proj",
        "fc1": "mlp.fc1", "fc2": "mlp.fc2"}                                                                      # path inside a transformers layer


def key(i, name, which):
    return f"base_model.model.text_model.encoder.layers.{i}.{PATH[name]}.lora_{which}.weight"


def add_adapters(enc, modules, r, seed, b_std=0.05):
    """give `modules` (names out of EXTRA) of every layer of an oracle encoder a rank-r adapter: A ~ N(0, 1/r^2) as peft draws it, B ~ N(0, b_std^2)
    (non-zero, so that every gradient path is live; b_std = 0: peft's B = 0), lora_alpha = r"""
    g = torch.Generator().manual_seed(seed)
    for layer in enc.layers:
        for name in modules:
            assert name in EXTRA, name
            m = getattr(layer, ATTR[name])
            dout, din = m.weight.shape
            m.r, m.scaling = r, 1.0
            m.lora_A = nn.Parameter(torch.randn(r, din, generator=g) / r)
            m.lora_B = nn.Parameter(torch.randn(dout, r, generator=g) * b_std)
    return enc


def adapted(enc):
    """names of the modules of layer 0 that carry an adapter, in ALL's order"""
    return tuple(n for n in ALL if getattr(enc.layers[0], ATTR[n]).r > 0)


def peft_state_dict(enc):
    sd = {}
    for i, layer in enumerate(enc.layers):
        for n in adapted(enc):
            m = getattr(layer, ATTR[n])
            sd[key(i, n, "A")], sd[key(i, n, "B")] = m.lora_A.detach().clone(), m.lora_B.detach().clone()
    return sd


def load_peft_state_dict(enc, sd):
    """copy a peft adapter state dict into an oracle encoder whose adapted modules (and ranks) match it exactly"""
    held = {k.split(".")[-3] for k in sd}
    assert held == set(adapted(enc)), (held, adapted(enc))
    with torch.no_grad():
        for i, layer in enumerate(enc.layers):
            for n in adapted(enc):
                m = getattr(layer, ATTR[n])
                m.lora_A.copy_(sd[key(i, n, "A")])
                m.lora_B.copy_(sd[key(i, n, "B")])


def copy_to_hip(enc, hip):
    """the oracle's adapter masters into a HipTextEncoder built with the same modules"""
    assert tuple(hip.lora_targets) == adapted(enc), (hip.lora_targets, adapted(enc))
    for i, layer in enumerate(enc.layers):
        hip.lora_A[i].copy_(torch.cat([layer.q.lora_A, layer.k.lora_A, layer.v.lora_A]).detach())
        hip.lora_B[i].copy_(torch.cat([layer.q.lora_B, layer.k.lora_B, layer.v.lora_B]).detach())
        for n, X in hip.extra.items():
            m = getattr(layer, ATTR[n])
            X.A[i].copy_(m.lora_A.detach())
            X.B[i].copy_(m.lora_B.detach())


def oracle_grads(enc):
    """-> (gA [L, 3r, D], gB [L, 3D, r], {extra module: (gA [L, r, K], gB [L, N, r])}) from the .grad of an oracle encoder"""
    gA = torch.stack([torch.cat([l.q.lora_A.grad, l.k.lora_A.grad, l.v.lora_A.grad]) for l in enc.layers])
    gB = torch.stack([torch.cat([l.q.lora_B.grad, l.k.lora_B.grad, l.v.lora_B.grad]) for l in enc.layers])
    gx = {n: (torch.stack([getattr(l, ATTR[n]).lora_A.grad for l in enc.layers]), torch.stack([getattr(l, ATTR[n]).lora_B.grad for l in enc.layers]))
          for n in adapted(enc)[3:]}
    return gA, gB, gx


def split_step_grads(g_lora, enc):
    """the oracle step's `g_lora` list (lora_parameters() order) -> the same triple as `oracle_grads`"""
    names = adapted(enc)
    per = 2 * len(names)
    L = len(enc.layers)
    at = lambda l, n, which: g_lora[per * l + 2 * names.index(n) + (0 if which == "A" else 1)]   # noqa: E731
    gA = torch.stack([torch.cat([at(l, n, "A") for n in QKV]) for l in range(L)])
    gB = torch.stack([torch.cat([at(l, n, "B") for n in QKV]) for l in range(L)])
    gx = {n: (torch.stack([at(l, n, "A") for l in range(L)]), torch.stack([at(l, n, "B") for l in range(L)])) for n in names[3:]}
    return gA, gB, gx
