"""Several trained output directories as one: a subject run and a style run (`--mixing`: DESIGN section 14) composed at generation time.

    compose_runs([run_a, run_b], weights=[1.0, 0.7]) -> TrainedRun      what `generate.load_text_encoder` / `generate_instance` take unchanged
    adapter_support(run) -> "even" | "odd" | "both" | "none"            which output rows of the run's lora_B are non-zero
    disjoint(runs)       -> bool                                        no two adapters touch the same output features (what --mixing guarantees)

Host only: no kernel library, no device.  Composition is rank concatenation.  With A_c = [A_1; A_2; ...] stacked along rows and
B_c = [w_1 B_1 | w_2 B_2 | ...] side by side, B_c A_c = sum_i w_i B_i A_i, so the result is ONE adapter of rank sum r_i with lora_alpha = r
(scaling 1) and the adapter kernels apply it as they apply any other; the only arithmetic is w_i * B_i, in fp32.  The UNet cross-attention K/V
adapters (`TrainedRun.unet_lora`) compose by the same identity.

Runs may adapt different modules beyond q/k/v (--lora_target_modules: out_proj / fc1 / fc2).  A module takes the ranks of the runs that adapt it;
the encoder runs ONE rank, so every module is padded to the common rank sum r_i with zero rows of A and zero columns of B, which add exact zeros.
"""
from __future__ import annotations

import re
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from .generate import LORA_EXTRA_TARGETS, LORA_TARGETS, MAX_LORA_RANK, TrainedRun

_KEY = re.compile(r"^(?P<module>.*\.layers\.(?P<layer>\d+)\.(?:self_attn\.(?P<proj>[a-z]+_proj)|mlp\.(?P<fc>fc[12])))\.lora_(?P<which>[AB])\.weight$")


def _proj(m) -> str:
    return m.group("proj") or m.group("fc")


def _refuse_dora(run: TrainedRun):
    if getattr(run, "use_dora", False):
        raise NotImplementedError(f"compose_runs: {run.path} is a use_dora run: DoRA renormalises every row of W + B A, so adapters do not add (or "
                                  "scale) by rank concatenation; sample it on its own, without --with / --weights")


def _modules(run: TrainedRun) -> Dict[str, Tuple[torch.Tensor, torch.Tensor]]:
    """module name (`...layers.{i}.self_attn.{q,k,v,out}_proj`, `...layers.{i}.mlp.fc{1,2}`) -> (lora_A [r, K], lora_B [N, r]); a key of any
    other form is refused"""
    _refuse_dora(run)
    halves: Dict[str, Dict[str, torch.Tensor]] = {}
    for k, v in run.lora.items():
        m = _KEY.match(k)
        if not m or _proj(m) not in LORA_TARGETS + LORA_EXTRA_TARGETS:
            raise ValueError(f"{run.path}: {k!r} is not a q_proj / k_proj / v_proj / out_proj / fc1 / fc2 adapter key")
        halves.setdefault(m.group("module"), {})[m.group("which")] = v
    out = {}
    for name, h in halves.items():
        if set(h) != {"A", "B"}:
            raise ValueError(f"{run.path}: {name} holds lora_{'A' if 'A' in h else 'B'} only")
        out[name] = (h["A"], h["B"])
    return out


def _geometry(run: TrainedRun, modules) -> Tuple[int, int]:
    """(hidden size, layer count) of a run's adapter"""
    square = [ab for n, ab in modules.items() if n.endswith("_proj")]       # (fc1 / fc2 are hidden x intermediate)
    widths = {int(a.shape[1]) for a, _ in square} | {int(b.shape[0]) for _, b in square}
    if len(widths) != 1:
        raise ValueError(f"{run.path}: the adapter tensors disagree in width: {sorted(widths)}")
    return widths.pop(), 1 + max(int(_KEY.match(n + ".lora_A.weight").group("layer")) for n in modules)


def adapter_support(run: TrainedRun) -> str:
    """which output rows of lora_B are non-zero over all modules of the run: "even" (what `--mixing --augment_ops object` leaves trainable),
    "odd" (`--mixing --augment_ops style`), "both", or "none" (no adapter, or one that never left its zero initialisation)"""
    even = odd = False
    if run.rank:
        for _, b in _modules(run).values():
            even = even or bool((b[0::2] != 0).any())
            odd = odd or bool((b[1::2] != 0).any())
    return "both" if even and odd else "even" if even else "odd" if odd else "none"


def disjoint(runs: Sequence[TrainedRun]) -> bool:
    """true when no two runs with adapters share a parity class and none is "both": their deltas change disjoint output features of every
    projection.  Reported, never enforced: overlapping adapters compose as a plain weighted sum."""
    seen = [s for s in map(adapter_support, runs) if s != "none"]
    return "both" not in seen and len(set(seen)) == len(seen)


def _concat(parts: List[Tuple[torch.Tensor, torch.Tensor, float]]) -> Tuple[torch.Tensor, torch.Tensor]:
    """[(A_i [r_i, D], B_i [N, r_i], w_i)] -> (A_c [sum r_i, D], B_c [N, sum r_i]); one part at weight 1: the tensors themselves"""
    if len(parts) == 1 and parts[0][2] == 1.0:
        return parts[0][0], parts[0][1]
    A = torch.cat([a.float() for a, _, _ in parts], dim=0).contiguous()
    B = torch.cat([b.float() if w == 1.0 else b.float() * torch.tensor(w, dtype=torch.float32) for _, b, w in parts], dim=1).contiguous()
    return A, B


def compose_runs(runs: Sequence[TrainedRun], weights: Optional[Sequence[float]] = None) -> TrainedRun:
    """-> one TrainedRun that applies sum_i weights[i] * (adapter of run i) and knows the tokens of every run.

    adapters   rank concatenation (module docstring); a run of rank 0 or weight 0 contributes tokens only (its adapter is left out, not
               zero-filled); `compose_runs([run])` returns `run`'s tensors themselves
    tokens     the union in run order; a name that several runs hold keeps the vector of the first, and every later one is recorded in
               `shadowed` as (token, path of the run whose vector was dropped)
    UNet       the cross-attention K/V adapters of all runs, composed the same way (`unet_rank` = the sum of their ranks)
    path, files   the first run's
    Refused: ValueError when the runs disagree in hidden size, layer count or adapter key set, or `weights` has another length than `runs`;
    NotImplementedError when the ranks add up to more than the adapter kernels take, or when a run is a DoRA one (use_dora): its rows are
    renormalised by || W + B A ||, which is not additive in the adapters, so rank concatenation does not define the sum."""
    runs = list(runs)
    if not runs:
        raise ValueError("compose_runs: no run given")
    for run in runs:
        _refuse_dora(run)
    weights = [1.0] * len(runs) if weights is None else [float(w) for w in weights]
    if len(weights) != len(runs):
        raise ValueError(f"compose_runs: {len(weights)} weights for {len(runs)} runs")
    # ---- text-encoder adapters
    used = [(run, _modules(run), w) for run, w in zip(runs, weights) if run.rank and w != 0.0]
    first_geo = None
    for run, mods, _ in used:
        geo = _geometry(run, mods)
        if first_geo is None:
            first_geo, first = geo, (run, mods)
            continue
        if geo[0] != first_geo[0]:
            raise ValueError(f"compose_runs: hidden size {geo[0]} of {run.path} != {first_geo[0]} of {first[0].path}")
        if geo[1] != first_geo[1]:
            raise ValueError(f"compose_runs: {geo[1]} layers in {run.path} != {first_geo[1]} in {first[0].path}")
        # q/k/v: every run, every layer.  out_proj / fc1 / fc2: a run adapts one in every layer or in none (the encoder has no per-layer choice)
        qkv = lambda ms: {n for n in ms if n.rsplit(".", 1)[1] in LORA_TARGETS}   # noqa: E731
        if qkv(mods) != qkv(first[1]):
            odd_one = sorted(qkv(mods) ^ qkv(first[1]))[0]
            raise ValueError(f"compose_runs: {run.path} and {first[0].path} adapt different modules (e.g. {odd_one})")
    for run, mods, _ in used:
        for x in LORA_EXTRA_TARGETS:
            have = [n for n in mods if n.rsplit(".", 1)[1] == x]
            if have and len(have) != first_geo[1]:
                raise ValueError(f"compose_runs: {run.path} adapts {x} in {len(have)} of {first_geo[1]} layers (different modules per layer)")
    ranks = [run.rank for run, _, _ in used]
    if sum(ranks) > MAX_LORA_RANK:
        raise NotImplementedError(f"compose_runs: ranks {' + '.join(map(str, ranks))} = {sum(ranks)}: the text-encoder adapter kernels take "
                                  f"r <= {MAX_LORA_RANK}")
    lora: Dict[str, torch.Tensor] = {}
    if used:
        names = list(used[0][1]) + sorted({n for _, mods, _ in used[1:] for n in mods} - set(used[0][1]))
        for name in names:
            parts = [(mods[name][0], mods[name][1], w) for _, mods, w in used if name in mods]
            shapes = {(int(a.shape[1]), int(b.shape[0])) for a, b, _ in parts}
            if len(shapes) != 1:
                raise ValueError(f"compose_runs: the runs disagree in the shape of {name}: {sorted(shapes)}")
            A, B = _concat(parts)
            if A.shape[0] < sum(ranks):   # a module only some runs adapt: zero A rows / zero B columns up to the rank every module runs at
                pad = sum(ranks) - A.shape[0]
                A = torch.cat([A.float(), torch.zeros(pad, A.shape[1])], dim=0).contiguous()
                B = torch.cat([B.float(), torch.zeros(B.shape[0], pad)], dim=1).contiguous()
            lora[name + ".lora_A.weight"], lora[name + ".lora_B.weight"] = A, B
    # ---- tokens
    width = first_geo[0] if first_geo else None
    tokens: List[Tuple[str, torch.Tensor]] = []
    owner: Dict[str, str] = {}
    shadowed: List[Tuple[str, str]] = []
    for run in runs:
        for name, vec in run.tokens:
            if width is None:
                width = int(vec.shape[0])
            if int(vec.shape[0]) != width:
                raise ValueError(f"compose_runs: token {name!r} of {run.path} has width {int(vec.shape[0])}; the other runs' hidden size is {width}")
            if name in owner:
                shadowed.append((name, run.path))
                continue
            owner[name] = run.path
            tokens.append((name, vec))
    # ---- UNet cross-attention K/V adapters
    u_used = [(run, w) for run, w in zip(runs, weights) if run.unet_rank and w != 0.0]
    unet_lora: Dict[str, torch.Tensor] = {}
    if u_used:
        keys = set(u_used[0][0].unet_lora)
        for run, _ in u_used[1:]:
            if set(run.unet_lora) != keys:
                raise ValueError(f"compose_runs: the UNet adapters of {run.path} and {u_used[0][0].path} adapt different modules")
        for ka in sorted(k for k in keys if ".lora_A." in k):
            kb = ka.replace(".lora_A.", ".lora_B.")
            shapes = {(run.unet_lora[ka].shape[1], run.unet_lora[kb].shape[0]) for run, _ in u_used}
            if len(shapes) != 1:
                raise ValueError(f"compose_runs: the UNet adapters disagree in the shape of {ka[:-len('.lora_A.default.weight')]}")
            unet_lora[ka], unet_lora[kb] = _concat([(run.unet_lora[ka], run.unet_lora[kb], w) for run, w in u_used])
    return TrainedRun(path=runs[0].path, rank=sum(ranks), lora=lora, tokens=tokens, files=list(runs[0].files),
                      unet_rank=sum(run.unet_rank for run, _ in u_used), unet_lora=unet_lora, shadowed=shadowed)
