"""Images from a trained output directory: the read side of the layout `checkpoint.py` writes, and the generation protocol of the reference's
eval_dreambooth.py (`load_pipeline` :175-215, `generate_from_pipeline` :218-267, `generate` :270-350) and inference.py (:47-112).

    read_run_dir(<path>/<instance>[/checkpoint-N]) -> TrainedRun      text_encoder/adapter_config.json + adapter_model.safetensors, <token>.bin,
                                                                      unet/ (the cross-attention K/V adapters of --unet_params_to_train crossattn_kv)
    load_text_encoder(model_dir, run, ...)      -> HipTextEncoder (+ tokenizer) with the adapter, the learned rows and the null-embedding pins
    Pipeline.from_model_dir(model_dir, ...)     -> UNet, VAE decoder and sampler executors, built once per run
    Pipeline.set_unet_adapters([...])           -> attn2.to_k / to_v = W + sum w_i B_i A_i (one exact-fp32 GEMM, rounded once); [] = the base weights
    Pipeline.edit_images(cond, uncond, noise, z0, strength, ...)  -> `images` from an encoded photo, optionally inside a mask (edit.py)
    Pipeline.invert_edit_images(cond, uncond, z0, p2p, ...)       -> a photo inverted to noise and edited by its prompt
    Pipeline.canvas_images(cond, uncond, latents, ...)            -> wide and tall images: a canvas of overlapping windows
    generate_instance(pipe, base, run, ...)     -> <outdir>/seed<s>/<instance>/<prompt>.png for every seed, 25 prompts each

Device work: `HipTextEncoder.forward`, `HipSampler.denoise` (guided DPM-Solver++ steps on `HipUNet.forward`), `HipVAEDecoder.decode_rgbx`
(`tb_vae_image_rgbx`: decoder output -> resident RGBX bytes).  One download per prompt batch; PNG encoding runs on host threads beside the
next batch.

Stated deviations from the reference:
  * seeding: the reference seeds a `torch.Generator` and never uses it (:236-240), so its images differ from run to run.  Here the latent of a
    seed is `torch.randn(1, 4, size, size, generator=torch.Generator().manual_seed(seed))` on the CPU in fp32, rounded to fp16 (the reference
    draws in its pipeline's fp16): the same on every machine.
  * the 25 prompts run as even batches of at most `prompt_batch` (16: 13 + 12) on ONE set of executors sized for the larger batch; the short
    batch is padded with its last prompt and the padding image is dropped.  The reference runs 16 + 9.
  * the null embedding is the training-time one (the base encoder's output for the empty prompt, or the shipped SD2.1-base tensor); the reference
    loads `assets/start_emb_<model>.pt`, a file it does not ship.
  * a run's `unet/` directory (the cross-attention K/V adapters of `--unet_params_to_train crossattn_kv`) is read and folded into the UNet before
    the run is sampled; the reference's readers never open it and sample such a run with the base UNet.
  * `--model` is a local diffusers directory; UNet, decoder and sampler are built once per run and only the text encoder is reloaded per subject.
"""
from __future__ import annotations

import json
import os
import time
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
HUB_ALIASES = ("sd14", "sd15", "sd21base", "sd21")     # eval_dreambooth.py:18-23 / inference.py:15-20: names of hub repositories
SKIPPED_BIN = ("optimizer.bin", "scheduler.bin")       # :199-206
LORA_TARGETS = ("q_proj", "k_proj", "v_proj")
LORA_EXTRA_TARGETS = ("out_proj", "fc1", "fc2")     # --lora_target_modules may add these (text_encoder.LORA_EXTRA)
DORA_KEY = ".lora_magnitude_vector"                 # <module>.lora_magnitude_vector of a --use_dora run (checkpoint.DORA_KEY)


def lora_targets_of(lora) -> Tuple[str, ...]:
    """the adapted modules of a peft adapter state dict (`...{self_attn,mlp}.<module>.lora_{A,B}.weight`), q/k/v first"""
    held = {k.split(".")[-3] for k in lora if not k.endswith(DORA_KEY)}
    return tuple(n for n in LORA_TARGETS + LORA_EXTRA_TARGETS if n in held)
UNET_LORA_TARGETS = ("attn2.to_k", "attn2.to_v")      # checkpoint.save_unet_adapters
MAX_PNG_THREADS = 8


# ------------------------------------------------------------------------------------------------ subjects, prompts, names (host only)
def load_eval_prompts() -> Tuple[Dict[str, str], List[str], List[str]]:
    """(subject -> class name, the 25 object prompts, the 25 live-subject prompts) of eval_dreambooth.py:25-112"""
    with open(os.path.join(_HERE, "eval_prompts.json")) as f:
        d = json.load(f)
    return dict(d["instances"]), list(d["object_prompts"]), list(d["live_prompts"])


def is_live(instance: str) -> bool:
    """:142-146"""
    return load_eval_prompts()[0][instance] in ("cat", "dog")


def prompt_templates(instance: str) -> List[str]:
    instances, obj, live = load_eval_prompts()
    if instance not in instances:
        raise ValueError(f"Invalid instance: {instance}")   # :228
    return live if instances[instance] in ("cat", "dog") else obj


def identifier_for(token_format: str, instance: str, files: Sequence[str]) -> str:
    """:329-337: INSTANCE -> the subject; one copy per placeholder vector (= files of the model path whose name starts with the subject's), every
    '>' of copy i becoming '_i>'; then SUBJECT -> the class name."""
    cls = load_eval_prompts()[0][instance]
    num_vectors = len([f for f in files if f.startswith(instance)])
    identifier = token_format.replace("INSTANCE", instance)
    if num_vectors > 1:
        identifier = " ".join(identifier.replace(">", f"_{i}>") for i in range(num_vectors))
    return identifier.replace("SUBJECT", cls)


def instance_prompts(instance: str, identifier: str) -> List[str]:
    return [t.format(identifier) for t in prompt_templates(instance)]


def image_filename(prompt: str, identifier: str, instance: str) -> str:
    """:263"""
    cls = load_eval_prompts()[0][instance]
    return f"{prompt.replace(identifier, cls).replace(' ', '_')}.png"


def prompt_batches(prompts: Sequence[str], prompt_batch: int) -> List[List[str]]:
    """even batches of at most `prompt_batch`, in order (25, 16 -> 13 + 12)"""
    n = len(prompts)
    k = -(-n // prompt_batch)
    base, rem = divmod(n, k)
    out, off = [], 0
    for i in range(k):
        m = base + (1 if i < rem else 0)
        out.append(list(prompts[off:off + m]))
        off += m
    return out


def model_path_of(path: str, instance: str, checkpoint: Optional[int]) -> str:
    """:318-319"""
    return os.path.join(path, instance, f"checkpoint-{checkpoint}" if checkpoint is not None else "")


def select_instances(path: str, requested: Optional[Sequence[str]]) -> List[str]:
    """--instances (in the subject table's order, :271-275), else those of the 30 subjects that exist as sub-directories of `path`"""
    table = load_eval_prompts()[0]
    if requested is not None:
        unknown = [i for i in requested if i not in table]
        if unknown:
            raise SystemExit(f"unknown --instances {unknown}: the subjects are {', '.join(table)}")
        return [i for i in table if i in requested]
    found = [i for i in table if os.path.isdir(os.path.join(path, i))]
    if not found:
        raise SystemExit(f"no trained subject under {path}: expected sub-directories named after the DreamBooth subjects ({', '.join(list(table)[:4])}, ...)")
    return found


def seeded_latent(seed: int, size: int) -> torch.Tensor:
    """the one latent of a seed: CPU, fp32 draw, rounded to fp16 (returned as fp32 [1, 4, size, size])"""
    g = torch.Generator().manual_seed(int(seed))
    return torch.randn(1, 4, size, size, generator=g, dtype=torch.float32).half().float()


def seeded_canvas_latent(seed: int, Hc: int, Wc: int) -> torch.Tensor:
    """`seeded_latent` for a canvas of Hc x Wc cells (canvas.py): the same generator, an fp32 draw of [1, 4, Hc, Wc] rounded to fp16.  At
    Hc == Wc == size it is `seeded_latent(seed, size)` bit for bit."""
    g = torch.Generator().manual_seed(int(seed))
    return torch.randn(1, 4, int(Hc), int(Wc), generator=g, dtype=torch.float32).half().float()


# ------------------------------------------------------------------------------------------------ reader of a trained output directory
MAX_LORA_RANK = 64   # ops.LORA_MAX_RANK (not imported: reading a run directory needs no kernel library)


@dataclass
class TrainedRun:
    path: str
    rank: int
    lora: Dict[str, torch.Tensor]                       # peft adapter keys (checkpoint.lora_state_dict)
    tokens: List[Tuple[str, torch.Tensor]] = field(default_factory=list)   # (name, fp32 [D]) in loading order
    files: List[str] = field(default_factory=list)      # os.listdir(path): the identifier counts the subject's files
    unet_rank: int = 0                                  # <path>/unet/: rank of the cross-attention K/V adapters (0: none)
    unet_lora: Dict[str, torch.Tensor] = field(default_factory=dict)       # in-model keys (checkpoint.unet_lora_state_dict)
    shadowed: List[Tuple[str, str]] = field(default_factory=list)          # compose.compose_runs: (token, path of the run whose vector was dropped)
    use_dora: bool = False                              # a --use_dora run: `lora` also holds <module>.lora_magnitude_vector, fp32 [N]


def read_run_dir(model_path: str, hidden_size: Optional[int] = None) -> TrainedRun:
    """`load_adapter(<path>/text_encoder)` + `load_textual_inversion` of every `*.bin` in sorted order except optimizer.bin / scheduler.bin
    (:193-206).  What the HIP encoder cannot apply is refused by name.  hidden_size: the encoder's width when the caller knows it (otherwise
    taken from the adapter's lora_A)."""
    from safetensors.torch import load_file
    te_dir = os.path.join(model_path, "text_encoder")
    if not os.path.isdir(te_dir):
        raise FileNotFoundError(f"{model_path}: no text_encoder/ directory (not a trained output directory)")
    with open(os.path.join(te_dir, "adapter_config.json")) as f:
        cfg = json.load(f)
    r = int(cfg.get("r", 0))
    use_dora = bool(cfg.get("use_dora"))
    if cfg.get("use_rslora"):
        raise NotImplementedError(f"{te_dir}: use_rslora adapters are not built (scaling alpha / sqrt(r))")
    if r and cfg.get("lora_alpha", r) != r:
        raise NotImplementedError(f"{te_dir}: lora_alpha = {cfg.get('lora_alpha')} != r = {r}: the kernels carry no separate LoRA scaling")
    if use_dora and not r:
        raise NotImplementedError(f"{te_dir}: use_dora with r = 0: there is no adapter to decompose")
    if r > MAX_LORA_RANK:
        raise NotImplementedError(f"{te_dir}: rank-{r} adapters are not built (the text-encoder adapter kernels take r <= {MAX_LORA_RANK})")
    targets = cfg.get("target_modules") or []
    targets = [targets] if isinstance(targets, str) else list(targets)
    if r and (set(targets) - set(LORA_TARGETS + LORA_EXTRA_TARGETS) or not set(LORA_TARGETS) <= set(targets)):
        raise NotImplementedError(f"{te_dir}: target_modules {sorted(targets)}: adapters are built for q_proj / k_proj / v_proj (always all three) "
                                  "and, beside them, out_proj / fc1 / fc2")
    lora = load_file(os.path.join(te_dir, "adapter_model.safetensors")) if r else {}
    if r:
        mags = {k: v for k, v in lora.items() if k.endswith(DORA_KEY)}
        if use_dora and not mags:   # (the magnitudes are what makes the adapter a DoRA one: without them only a plain LoRA could run, silently)
            raise NotImplementedError(f"{te_dir}: use_dora is set, but adapter_model.safetensors holds no lora_magnitude_vector tensors")
        if mags and not use_dora:
            raise NotImplementedError(f"{te_dir}: adapter_model.safetensors holds lora_magnitude_vector tensors, but use_dora is not set")
        held = {k.split(".")[-3] for k in lora if k not in mags}
        if use_dora and {k.split(".")[-2] for k in mags} != held:
            raise NotImplementedError(f"{te_dir}: use_dora: lora_magnitude_vector tensors of {sorted({k.split('.')[-2] for k in mags})}, "
                                      f"adapters of {sorted(held)}")
        if held != set(targets):   # (a listed module without tensors would silently run un-adapted; tensors of an unlisted one would be dropped)
            raise NotImplementedError(f"{te_dir}: target_modules {sorted(targets)}, but adapter_model.safetensors holds tensors of {sorted(held)}")
        a = [v for k, v in lora.items() if k.endswith("lora_A.weight")]
        if not a or any(t.shape[0] != r for t in a):
            raise ValueError(f"{te_dir}: adapter_model.safetensors does not hold rank-{r} lora_A tensors")
        hidden_size = hidden_size or int(next(v for k, v in lora.items() if k.endswith("q_proj.lora_A.weight")).shape[1])
    files = sorted(os.listdir(model_path))
    tokens: List[Tuple[str, torch.Tensor]] = []
    for name in files:
        if not name.endswith(".bin") or name in SKIPPED_BIN:
            continue
        d = torch.load(os.path.join(model_path, name), map_location="cpu")
        if not isinstance(d, dict) or len(d) != 1:
            raise ValueError(f"{model_path}/{name}: expected a {{token: tensor}} dictionary with one entry")
        (tok, t), = d.items()
        t = t.detach().float()
        if t.dim() == 1:
            t = t[None]
        if t.dim() != 2:
            raise ValueError(f"{model_path}/{name}: token {tok!r} has shape {tuple(t.shape)}; expected [D], [1, D] or [n, D]")
        if hidden_size is not None and t.shape[1] != hidden_size:
            raise ValueError(f"{model_path}/{name}: token {tok!r} has width {t.shape[1]}, the text encoder's hidden_size is {hidden_size}")
        names = [tok] + [f"{tok}_{i}" for i in range(1, t.shape[0])]    # diffusers load_textual_inversion: tok, tok_1, ..., tok_{n-1}
        tokens += [(n, t[i].clone()) for i, n in enumerate(names)]
    unet_rank, unet_lora = read_unet_adapters(model_path)
    return TrainedRun(path=model_path, rank=r, lora=lora, tokens=tokens, files=files, unet_rank=unet_rank, unet_lora=unet_lora, use_dora=use_dora)


def read_unet_adapters(model_path: str) -> Tuple[int, Dict[str, torch.Tensor]]:
    """<run>/unet/adapter_config.json + adapter_model.safetensors (checkpoint.save_unet_adapters) -> (rank, tensors under the in-model keys
    `<attn2 path>.to_{k,v}.lora_{A,B}.default.weight`); (0, {}) when the run holds none.  Both key layouts of
    `checkpoint.load_unet_peft_adapter_state_dict` are read; what the fold cannot apply is refused by name."""
    from safetensors.torch import load_file
    from .checkpoint import unet_adapter_in_model_keys
    u_dir = os.path.join(model_path, "unet")
    wpath = os.path.join(u_dir, "adapter_model.safetensors")
    if not os.path.exists(wpath):
        return 0, {}
    with open(os.path.join(u_dir, "adapter_config.json")) as f:
        cfg = json.load(f)
    r = int(cfg.get("r", 0))
    if cfg.get("use_dora"):
        raise NotImplementedError(f"{u_dir}: use_dora adapters are not built")
    if cfg.get("use_rslora"):
        raise NotImplementedError(f"{u_dir}: use_rslora adapters are not built (scaling alpha / sqrt(r))")
    if r <= 0:
        raise ValueError(f"{u_dir}: adapter_config.json has r = {r} beside an adapter_model.safetensors")
    if cfg.get("lora_alpha", r) != r:
        raise NotImplementedError(f"{u_dir}: lora_alpha = {cfg.get('lora_alpha')} != r = {r}: the K/V fold carries no separate LoRA scaling")
    targets = cfg.get("target_modules") or []
    targets = [targets] if isinstance(targets, str) else list(targets)
    if sorted(targets) != sorted(UNET_LORA_TARGETS):
        raise NotImplementedError(f"{u_dir}: target_modules {sorted(targets)}: only attn2.to_k / attn2.to_v adapters are built")
    try:
        sd = unet_adapter_in_model_keys(load_file(wpath))
    except KeyError as e:
        raise ValueError(f"{u_dir}: {e.args[0]}")
    for k, v in sd.items():
        if v.dim() != 2 or (v.shape[0] if ".lora_A." in k else v.shape[1]) != r:
            raise ValueError(f"{u_dir}: {k} has shape {tuple(v.shape)}: not a rank-{r} adapter tensor")
    return r, {k: v.float() for k, v in sd.items()}


# ------------------------------------------------------------------------------------------------ text encoder of one subject
@dataclass
class BaseText:
    """what every subject of a run shares: the base encoder's weights and geometry and the null embedding"""
    model_dir: str
    geo: object
    state_dict: Dict[str, torch.Tensor]
    null: torch.Tensor


def load_base_text(model_dir: str, device="cuda") -> BaseText:
    from safetensors.torch import load_file
    from . import models
    from .text_encoder import HipTextEncoder
    from .workload import BOS, EOS
    wpath = os.path.join(model_dir, "text_encoder", "model.safetensors")
    if not os.path.exists(wpath):
        raise FileNotFoundError(f"{wpath} is missing: --model must be a local diffusers model directory")
    with open(os.path.join(model_dir, "text_encoder", "config.json")) as f:
        geo = models.clip_geometry_from_config(json.load(f))
    csd = load_file(wpath)
    # the null embedding exactly as the trainer makes it: the base encoder's output for the empty prompt, or the shipped SD2.1-base tensor when it fits
    frozen = HipTextEncoder(geo, csd, 1, mode="autocast", device=device)
    null_ids = torch.full((1, geo.max_pos), EOS, dtype=torch.int64, device=device)
    null_ids[0, 0] = BOS
    null = frozen.forward(null_ids, pins=False).clone()
    del frozen
    shipped = os.path.join("assets", "null_emb_sd21base.pt")
    if os.path.exists(shipped):
        t = torch.load(shipped, map_location="cpu")
        t = t[0] if t.dim() == 3 else t
        if tuple(t.shape) == tuple(null.shape[-2:]):
            null = t.to(device, null.dtype).reshape(null.shape)
    return BaseText(model_dir=model_dir, geo=geo, state_dict=csd, null=null)


def load_text_encoder(model_dir: str, run: TrainedRun, batch: int, device="cuda", base: Optional[BaseText] = None):
    """-> (HipTextEncoder, tokenizer): the base encoder in the trainer's autocast mode with the run's adapter, its tokens registered in the tokenizer
    and written into the token table, and the null-embedding pins set (the reference's eval pipeline is a TextBoostModel, :176-182)."""
    from . import checkpoint as ckpt
    from .text_encoder import HipTextEncoder
    base = base or load_base_text(model_dir, device)
    geo = base.geo
    tdir = os.path.join(model_dir, "tokenizer")
    if not os.path.exists(os.path.join(tdir, "vocab.json")):
        raise FileNotFoundError(f"{tdir}: no vocab.json (only local tokenizer files can be loaded)")
    from transformers import CLIPTokenizer
    tokenizer = CLIPTokenizer.from_pretrained(tdir, local_files_only=True)     # (train_textboost.load_tokenizer)
    te = HipTextEncoder(geo, base.state_dict, batch, mode="autocast", lora_rank=run.rank, device=device,
                        lora_targets=lora_targets_of(run.lora) if run.rank else None, **({"use_dora": True} if run.use_dora else {}))
    if run.rank:
        ckpt.load_lora_state_dict(te, run.lora)
        te.pack_lora()
    if run.tokens:
        names = [n for n, _ in run.tokens]
        for n, v in run.tokens:
            if v.shape[0] != geo.hidden_size:
                raise ValueError(f"{run.path}: token {n!r} has width {v.shape[0]}, the text encoder's hidden_size is {geo.hidden_size}")
        if tokenizer.add_tokens(names) != len(names):
            raise ValueError(f"{run.path}: the tokenizer already contains one of {names}")
        ids = tokenizer.convert_tokens_to_ids(names)
        rows = te.add_tokens([0] * len(names))
        if list(rows) != list(ids):
            raise ValueError(f"tokenizer ids {ids} and embedding rows {rows} disagree (tokenizer vocabulary != embedding table size)")
        te.token_table[rows[0]:rows[0] + len(rows)].copy_(torch.stack([v for _, v in run.tokens]))
    te.set_null_embedding(base.null)
    return te, tokenizer


def tokenize(tokenizer, prompts: Sequence[str], max_length: int) -> torch.Tensor:
    return tokenizer(list(prompts), truncation=True, padding="max_length", max_length=max_length, return_tensors="pt").input_ids


# ------------------------------------------------------------------------------------------------ the executors of a run
class Pipeline:
    """UNet (batch 2B: guidance), VAE decoder and sampler for B images per launch, on the fp16 build of the kernel library."""

    def __init__(self, unet_geo, unet_sd, vae_geo, vae_sd, scheduler_config: Optional[dict], size: int, batch: int, steps: int = 25,
                 guidance: float = 7.5, text_len: int = 77, device="cuda"):
        from . import _lib
        from .sampler import HipSampler
        from .unet import HipUNet
        from .vae import HipVAEDecoder
        _lib.set_half("fp16")      # the reference's pipelines are fp16 (:321, inference.py:47)
        self.size, self.B, self.steps, self.guidance, self.dev = size, batch, steps, guidance, device
        self.unet = HipUNet(unet_geo, unet_sd, 2 * batch, size, size, text_len=text_len, device=device)
        self.vae = HipVAEDecoder(vae_geo, vae_sd, batch, size, size, device=device)
        self.sampler = HipSampler(self.unet, self.vae, steps=steps, guidance=guidance, scheduler_config=scheduler_config)
        # the fp32 attn2.to_k / to_v weights the UNet was built from, in the layout of `HipUNet.P["kv_all.w"]`: a fold rounds them once
        self.kv_base = torch.cat([torch.cat([unet_sd[p + ".to_k.weight"], unet_sd[p + ".to_v.weight"]], dim=0) for p, _ in self.unet.xattn],
                                 dim=0).detach().float().to(device).contiguous()
        self.kv_folded = False

    @classmethod
    def from_model_dir(cls, model_dir: str, batch: int, steps: int = 25, guidance: float = 7.5, device="cuda"):
        from safetensors.torch import load_file
        from . import models
        from .vae import vae_geometry_from_config
        for sub in ("unet", "vae", "text_encoder", "tokenizer", "scheduler"):
            if not os.path.isdir(os.path.join(model_dir, sub)):
                raise FileNotFoundError(f"{model_dir}: no {sub}/ (--model must be a local diffusers model directory)")
        with open(os.path.join(model_dir, "unet", "config.json")) as f:
            ucfg = json.load(f)
        with open(os.path.join(model_dir, "vae", "config.json")) as f:
            vcfg = json.load(f)
        with open(os.path.join(model_dir, "scheduler", "scheduler_config.json")) as f:
            scfg = json.load(f)
        with open(os.path.join(model_dir, "text_encoder", "config.json")) as f:
            text_len = json.load(f).get("max_position_embeddings", 77)
        vgeo = vae_geometry_from_config(vcfg)
        usd = load_file(os.path.join(model_dir, "unet", "diffusion_pytorch_model.safetensors"))
        vsd = load_file(os.path.join(model_dir, "vae", "diffusion_pytorch_model.safetensors"))
        return cls(models.unet_geometry_from_config(ucfg), usd, vgeo, vsd, scfg, int(ucfg.get("sample_size", 64)), batch, steps, guidance,
                   text_len=text_len, device=device)

    def set_unet_adapters(self, adapters: Sequence[Tuple[Dict[str, torch.Tensor], int, float]]):
        """adapters: (state dict under the in-model keys of `TrainedRun.unet_lora`, rank, weight) per run.  Loads attn2.to_k / to_v =
        W + sum_i w_i B_i A_i into the UNet: the products as ONE exact-fp32 GEMM `W2 A_all + W` (tb_gemm_f32_t; W2 = the block-structured
        [w_1 B_1 | w_2 B_2 | ...], w_i B_i rounded in fp32 on the host, zero outside a projection's own columns; A_all = every down projection
        stacked), rounded once to the executor's operand dtype by `load_kv_weight`.  No adapter (an empty list, weights 0): the base weights,
        exactly as the UNet was built with them."""
        from . import ops
        unet = self.unet
        adapters = [(sd, int(r), float(w)) for sd, r, w in adapters if int(r) > 0 and float(w) != 0.0]
        if not adapters:
            if self.kv_folded:
                unet.load_kv_weight(self.kv_base)
                self.kv_folded = False
            return
        Dc = self.kv_base.shape[1]
        n = len(unet.xattn)
        K = sum(n * 2 * r for _, r, _ in adapters)
        w2 = torch.zeros(unet.kv_total, K, dtype=torch.float32)
        a_all = torch.empty(K, Dc, dtype=torch.float32)
        col = 0
        for sd, r, w in adapters:
            for p, C in unet.xattn:
                ko = unet.kv_off[p]
                for j, name in enumerate(("to_k", "to_v")):
                    try:
                        A, B = sd[f"{p}.{name}.lora_A.default.weight"], sd[f"{p}.{name}.lora_B.default.weight"]
                    except KeyError as e:
                        raise ValueError(f"UNet adapters: no tensor {e.args[0]} (the adapters belong to another UNet geometry)")
                    if tuple(A.shape) != (r, Dc) or tuple(B.shape) != (C, r):
                        raise ValueError(f"UNet adapters: {p}.{name} has lora_A {tuple(A.shape)} / lora_B {tuple(B.shape)}; this UNet takes "
                                         f"{(r, Dc)} / {(C, r)}")
                    a_all[col:col + r] = A.float()
                    w2[ko + j * C:ko + (j + 1) * C, col:col + r] = B.float() * w
                    col += r
        w2, a_all = w2.to(self.dev), a_all.to(self.dev)
        merged = torch.empty_like(self.kv_base)
        with ops.f32_mode(0):      # exact products whatever mode the process trains in
            ops.gemm_f32_t(w2, a_all, merged, unet.kv_total, Dc, K, w_trans=True, R=self.kv_base)
        unet.load_kv_weight(merged)
        self.kv_folded = True

    def set_run(self, run: "TrainedRun"):
        """the UNet of one trained run: its K/V adapters folded in, or the base weights"""
        self.set_unet_adapters([(run.unet_lora, run.unet_rank, 1.0)] if run.unet_rank else [])

    def images(self, cond, uncond, latents, what: str = "", maps=None, regions=None, region_steps=None, p2p=None, excite=None,
               blend=None) -> torch.Tensor:
        """text states fp32 [B*T, D] twice, latents fp32 [B, 4, size, size] on the device -> int32 RGBX [B, 8 size, 8 size] (resident).
        Non-finite final latents raise before anything is decoded.  maps: an `attn_maps.AttnMapRecorder` of `self.unet` (the images do not
        change with it).  regions / region_steps: a `regions.RegionSet` of `self.unet` and how many steps it acts on (`HipSampler.denoise`).
        p2p: a `p2p.P2PControl` of `self.unet`: rows [0, B/2) are the source images, [B/2, B) the edited ones.
        excite: an `excite.ExciteControl` of `self.unet` (Attend-and-Excite; its trace is filled by the call).
        blend: a `local_blend.BlendControl` of `self.unet` (with `p2p`): the edited rows keep the source rows' latents outside the words'
        attention; its `final_mask` / `area` are left on the device."""
        x = self.sampler.denoise(cond, uncond, latents=latents, maps=maps, regions=regions, region_steps=region_steps, p2p=p2p, excite=excite,
                                 blend=blend)
        if not bool(torch.isfinite(x).all()):
            raise FloatingPointError(f"non-finite latents after {self.steps} steps: {what}")
        return self.vae.decode_rgbx(x)

    def canvas_images(self, cond, uncond, latents, stride=None, decode_stride=None, what: str = "") -> torch.Tensor:
        """Wide and tall images (the MultiDiffusion canvas): latents fp32 [n, 4, Hc, Wc] on the device, Hc, Wc >= size, text states
        as in `images` (one prompt for all) -> int32 RGBX [n, f Hc, f Wc] (resident; f = the VAE's factor).  `HipSampler.denoise_canvas` at
        `stride` cells (default size // 4), the finite check of `images`, then the canvas is decoded as size x size latent tiles at
        `decode_stride` cells (default 3 size / 4), B at a time, and `tb_tile_blend` feathers them over the f (size - decode_stride) pixels
        two neighbours share.  A size x size canvas is one window and one tile: the bytes of `images`."""
        from . import ops
        from .canvas import CanvasPlan, blend_ramp
        S = self.size
        f = self.vae.H // self.vae.h
        ds = max(1, (3 * S) // 4) if decode_stride is None else decode_stride
        n, _, Hc, Wc = latents.shape
        tiles_of = CanvasPlan(S, Hc, Wc, ds, n, self.B)       # (refusals before the denoising)
        x = self.sampler.denoise_canvas(cond, uncond, latents, stride=stride)
        if not bool(torch.isfinite(x).all()):
            raise FloatingPointError(f"non-finite latents after {self.steps} steps: {what}")
        tiles = torch.stack([x[img, :, oy:oy + S, ox:ox + S] for img in range(n) for oy, ox in tiles_of.windows()])
        rows, _, _ = self.vae.decode_tiles(tiles)
        rgbx = torch.empty(n, f * Hc, f * Wc, dtype=torch.int32, device=x.device)
        ops.tile_blend(rows, tiles_of, f, blend_ramp(S, ds, f), rgbx=rgbx)
        return rgbx

    def edit_images(self, cond, uncond, noise, z0, strength, latent_mask=None, pixel_mask=None, init_rgbx=None, maps=None,
                    what: str = "", regions=None, region_steps=None) -> torch.Tensor:
        """`images` from an encoded photo (textboost_amd/edit.py; `HipSampler.denoise_from`): noise fp32 [B, 4, size, size] (a seed's latent is
        its image's noise), z0 fp32 [1, 4, size, size] shared by the B images, latent_mask uint8 [size, size] or None (non-zero = repaint).
        With pixel_mask (uint8 [8 size, 8 size]) and init_rgbx (the prepared photo, int32 RGBX [8 size, 8 size]) the decoded region is pasted
        into the photo: pixels outside the mask are the photo's bytes.  -> int32 RGBX [B, 8 size, 8 size] (resident)."""
        from . import ops
        if (pixel_mask is None) != (init_rgbx is None):
            raise ValueError("the paste needs both pixel_mask and init_rgbx")
        x = self.sampler.denoise_from(cond, uncond, z0, noise, strength, mask=latent_mask, maps=maps, regions=regions, region_steps=region_steps)
        if not bool(torch.isfinite(x).all()):
            raise FloatingPointError(f"non-finite latents after {self.steps} steps: {what}")
        rgbx = self.vae.decode_rgbx(x)
        if pixel_mask is None:
            return rgbx
        out = torch.empty_like(rgbx)
        for b in range(rgbx.shape[0]):      # one launch per image
            ops.img_paste(rgbx[b], init_rgbx, pixel_mask, out=out[b])
        return out

    def invert_edit_images(self, cond, uncond, z0, p2p, invert_guidance: float = 1.0, latent_mask=None, pixel_mask=None, init_rgbx=None,
                           what: str = "", blend=None) -> torch.Tensor:
        """A photo edited by its prompt: rows [0, B/2) carry the prompt that describes the photo, rows [B/2, B) the edit
        prompt.  z0 fp32 [1, 4, size, size] (the encoded photo) is inverted under row 0's prompt (`HipSampler.invert`, guidance
        `invert_guidance`), then the prompt-to-prompt denoise runs with the source rows pinned to that trajectory (`denoise(p2p=, pin=)`):
        they end as z0 exactly, so their image is the VAE round trip of the photo.  latent_mask uint8 [size, size] or None (non-zero =
        repaint): the edited rows' other cells stay on the trajectory too.  With pixel_mask (uint8 [8 size, 8 size]) and init_rgbx (the
        prepared photo, int32 RGBX) the photo's bytes are pasted outside the mask into the EDITED rows only; the source rows stay the plain
        decode.  blend: a `local_blend.BlendControl` (one pair): from its start step on the edited row leaves the trajectory only where the
        words attend (inside latent_mask, when given).  -> int32 RGBX [B, 8 size, 8 size] (resident)."""
        from . import ops
        if (pixel_mask is None) != (init_rgbx is None):
            raise ValueError("the paste needs both pixel_mask and init_rgbx")
        if p2p is None:
            raise ValueError("invert_edit_images needs the prompt-to-prompt control of the edit")
        traj = self.sampler.invert(cond, uncond, z0, guidance=invert_guidance)
        x = self.sampler.denoise(cond, uncond, p2p=p2p, pin=traj[:, 0], pin_mask=latent_mask, blend=blend)
        if not bool(torch.isfinite(x).all()):
            raise FloatingPointError(f"non-finite latents after {self.steps} inversion and {self.steps} denoising steps: {what}")
        rgbx = self.vae.decode_rgbx(x)
        if pixel_mask is None:
            return rgbx
        out = rgbx.clone()
        for b in range(rgbx.shape[0] // 2, rgbx.shape[0]):      # one launch per edited image
            ops.img_paste(rgbx[b], init_rgbx, pixel_mask, out=out[b])
        return out


# ------------------------------------------------------------------------------------------------ the protocol
def _save_png(rgbx_host, path: str):
    """one image of the downloaded RGBX buffer (int32 [H, W], little endian: R, G, B, X bytes) -> PNG with Pillow's defaults (the reference's bare
    `image.save`)"""
    from PIL import Image
    h, w = rgbx_host.shape
    Image.fromarray(rgbx_host.view("uint8").reshape(h, w, 4)[:, :, :3]).save(path)


def generate_instance(pipe: Pipeline, base: BaseText, run: TrainedRun, instance: str, seeds: Sequence[int], outdir: str,
                      token_format: str = "<INSTANCE> SUBJECT", prompt_batch: int = 16, pool: Optional[ThreadPoolExecutor] = None,
                      timings: Optional[dict] = None) -> List[str]:
    """`generate_from_pipeline` for every seed -> the PNG paths written.  `outdir` is the run's image root (`<outdir>/<basename>[-N][_desc]`)."""
    dev = pipe.dev
    identifier = identifier_for(token_format, instance, run.files)
    prompts = instance_prompts(instance, identifier)
    batches = prompt_batches(prompts, prompt_batch)
    if max(len(b) for b in batches) > pipe.B:
        raise ValueError(f"the executors are built for {pipe.B} prompts per batch; {max(len(b) for b in batches)} needed")
    te, tokenizer = load_text_encoder(base.model_dir, run, 2 * pipe.B, dev, base=base)
    pipe.set_run(run)       # the run's UNet K/V adapters; the base weights again for a run without
    T = base.geo.max_pos
    # text states once per subject (they do not depend on the seed): the empty negative prompt and the batch's prompts in one encoder call
    states = []
    for b in batches:
        padded = b + [b[-1]] * (pipe.B - len(b))
        ids = tokenize(tokenizer, [""] * pipe.B + padded, T).to(dev)
        out = te.forward(ids).view(2, pipe.B * T, -1)
        states.append((out[1].clone(), out[0].clone()))
    own_pool = pool is None
    pool = pool or ThreadPoolExecutor(max_workers=MAX_PNG_THREADS)
    written: List[str] = []
    try:
        for seed in seeds:
            dst = os.path.join(outdir, f"seed{seed}", instance)
            os.makedirs(dst, exist_ok=True)
            lat = seeded_latent(seed, pipe.size).to(dev).repeat(pipe.B, 1, 1, 1)     # one latent for all prompts (:240, :257)
            jobs = []
            for b, (cond, uncond) in zip(batches, states):
                t0 = time.perf_counter()
                img = pipe.images(cond, uncond, lat, what=f"subject {instance}, seed {seed}, prompts {b}")
                host = img[:len(b)].cpu().numpy()          # one download per batch (synchronises)
                t1 = time.perf_counter()
                for k, p in enumerate(b):
                    path = os.path.join(dst, image_filename(p, identifier, instance))
                    jobs.append(pool.submit(_save_png, host[k], path))
                    written.append(path)
                if timings is not None:
                    timings["device_s"] = timings.get("device_s", 0.0) + (t1 - t0)
                    timings["images"] = timings.get("images", 0) + len(b)
            t0 = time.perf_counter()
            for j in jobs:      # the seed's directory is complete before it is reported
                j.result()
            if timings is not None:
                timings["png_wait_s"] = timings.get("png_wait_s", 0.0) + (time.perf_counter() - t0)
            print(f"[seed {seed}] {instance}: {len(prompts)} images -> {dst} (identifier {identifier!r})")
    finally:
        if own_pool:
            pool.shutdown(wait=True)
    return written


def generate_run(path: str, model_dir: str, instances: Sequence[str], seeds: Sequence[int], image_root: str, checkpoint: Optional[int] = None,
                 token_format: str = "<INSTANCE> SUBJECT", steps: int = 25, guidance: float = 7.5, prompt_batch: int = 16, device="cuda",
                 freeu=None) -> dict:
    """`generate` (:270-350) over the subjects: executors once, the text encoder per subject.  -> {"images", "seconds", ...}
    freeu: None or (b1, b2, s1, s2, mode) of `freeu.resolve`: every image is sampled with FreeU (`HipUNet.enable_freeu`)."""
    if not torch.cuda.is_available():
        raise SystemExit("image generation needs an MI355X: the product path has no CPU fallback")
    from . import _lib
    _lib.set_half("fp16")
    _lib.lib()
    n_batch = max(len(b) for b in prompt_batches(list(range(25)), prompt_batch))
    runs = {i: read_run_dir(model_path_of(path, i, checkpoint)) for i in instances}     # every refusal before anything reaches the device
    t0 = time.perf_counter()
    with torch.no_grad():
        pipe = Pipeline.from_model_dir(model_dir, n_batch, steps=steps, guidance=guidance, device=device)
        if freeu is not None:
            pipe.unet.enable_freeu(*freeu[:4], mode=freeu[4])
        base = load_base_text(model_dir, device)
        timings: dict = {}
        with ThreadPoolExecutor(max_workers=MAX_PNG_THREADS) as pool:
            for i in instances:
                generate_instance(pipe, base, runs[i], i, seeds, image_root, token_format=token_format, prompt_batch=prompt_batch, pool=pool,
                                  timings=timings)
    timings["seconds"] = time.perf_counter() - t0
    n = timings.get("images", 0)
    print(f"generated {n} images in {timings['seconds']:.1f} s ({n / max(timings.get('device_s', 0.0) + timings.get('png_wait_s', 0.0), 1e-9):.1f} "
          f"images/s after setup; prompt batch {n_batch}, {steps} steps)")
    return timings


def check_model_dir(model: Optional[str], prog: str, flag: str = "--model"):
    """--model: a local diffusers model directory; the reference's aliases name hub repositories"""
    if model in HUB_ALIASES:
        raise SystemExit(f"{prog}: {flag} {model} is the reference's alias of a hub repository; nothing is downloaded here: pass {flag} DIR, a "
                         "local diffusers model directory (unet/, vae/, text_encoder/, tokenizer/, scheduler/)")
    if not os.path.isdir(model):
        raise SystemExit(f"{prog}: {flag} {model} is not a directory: pass {flag} DIR, a local diffusers model directory (unet/, vae/, "
                         "text_encoder/, tokenizer/, scheduler/)")
