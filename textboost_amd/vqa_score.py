"""VQA score of generated images on a HIP CLIP-FlanT5 encoder-decoder (the reference's eval_dreambooth.py:546-565: t2v_metrics
`VQAScore(model='clip-flant5-xxl')`), forward only.

The network is LLaVA's construction on a T5: the penultimate layer of CLIP ViT-L/14@336px (vit.HipViT.hidden_states), a two-layer `mm_projector`
into T5's width, the projected patch rows spliced into the embedded question where the `<image>` marker stands, a FlanT5 encoder over that
sequence and a decoder that is teacher-forced on the answer "Yes".  The score of an (image, text) pair is P("Yes") as the geometric mean over
the answer's tokens: exp(-mean_t CE(logits[t], label[t])).

Everything marked [3P] restates t2v_metrics / LLaVA from knowledge: neither they nor the checkpoint are available where this was written, so
those conventions (prompt, chunk tokenisation, splice, score) are unverified against the real thing: DESIGN.md section 12 lists them.  The
arithmetic is checked against transformers' T5ForConditionalGeneration (tests/vqa_ref.py, tests/test_vqa_host.py).

Arithmetic is the towers' "autocast" mode in bfloat16, whatever the process runs (FlanT5's activations overflow fp16, and the reference runs
this forward under bf16 autocast [3P]): fp32 residual stream and RMS-norm statistics, bf16 GEMM and attention operands, fp32 logits.  Per
encoder block: rmsnorm -> stacked q|k|v GEMM -> attention with the relative-position bias and the key length -> o GEMM + residual -> rmsnorm ->
stacked wi_0|wi_1 GEMM -> gated tanh-GELU -> wo GEMM + residual (csrc/t5.hip holds the three kernels that are not tb_gemm).
"""
from __future__ import annotations

import glob
import json
import math
import os
from dataclasses import dataclass
from typing import Dict, Iterable, Iterator, List, Optional, Sequence, Tuple

import torch

from . import _lib as L
from . import augment, ops
from .vit import CLIP_MEAN, load_rgb

# ---- the prompt [3P, from knowledge: t2v_metrics clip_t5_model / its `t5_chat` conversation template].  A correction is an edit of these
# constants or of `build_ids`, nowhere else.
QUESTION_TEMPLATE = 'Does this figure show "{}"? Please answer yes or no.'
ANSWER_TEMPLATE = "Yes"
T5_CHAT_SYSTEM = ("A chat between a curious user and an artificial intelligence assistant. "
                  "The assistant gives helpful, detailed, and polite answers to the user's questions.")
IMAGE_MARKER = "<image>"
T5_CHAT_TEMPLATE = T5_CHAT_SYSTEM + " USER: " + IMAGE_MARKER + "\n{question} ASSISTANT:"
IMAGE_TOKEN_INDEX = -200   # LLaVA's placeholder id for the image rows


def build_ids(tokenizer, texts: Sequence[str], decoder_start_id: Optional[int] = None):
    """-> (input_ids: one id list per text holding IMAGE_TOKEN_INDEX once, labels: the answer's ids, decoder_input_ids: [start, labels[:-1]]).
    [3P] Every text chunk around the image marker is tokenised on its own as `tokenizer(chunk).input_ids` gives it: a T5 tokenizer ends each
    with EOS, so one EOS stands in front of the image rows and one ends the sequence.  The answer is the same for every sample (one label row,
    EOS included); the decoder is teacher-forced on it shifted right behind the start token (T5: the pad id)."""
    rows = []
    for text in texts:
        prompt = T5_CHAT_TEMPLATE.format(question=QUESTION_TEMPLATE.format(text))
        chunks = [list(tokenizer(c).input_ids) for c in prompt.split(IMAGE_MARKER)]
        assert len(chunks) == 2, "the template holds one image marker"
        rows.append(chunks[0] + [IMAGE_TOKEN_INDEX] + chunks[1])
    labels = list(tokenizer(ANSWER_TEMPLATE).input_ids)
    start = decoder_start_id if decoder_start_id is not None else tokenizer.pad_token_id
    if start is None:
        raise ValueError("the tokenizer has no pad_token_id to start the decoder with")
    return rows, labels, [int(start)] + labels[:-1]


# ---------------------------------------------------------------------------------------------------------------- geometry
@dataclass
class T5Geometry:
    """transformers `T5Config` fields of the language model + the vision width the projector reads"""
    vocab_size: int = 32128
    d_model: int = 4096
    d_kv: int = 64
    d_ff: int = 10240
    num_layers: int = 24
    num_decoder_layers: int = 24
    num_heads: int = 64
    num_buckets: int = 32
    max_distance: int = 128
    eps: float = 1e-6
    tie_word_embeddings: bool = False
    decoder_start_token_id: int = 0
    mm_hidden_size: int = 1024

    @property
    def inner(self) -> int:
        return self.num_heads * self.d_kv


FLAN_T5_XXL = T5Geometry()


def t5_geometry_from_config(cfg: dict) -> T5Geometry:
    """a clip-flant5 / T5 config.json -> geometry; what this path does not build is refused by field name"""
    ffp = cfg.get("feed_forward_proj", "relu")
    if ffp != "gated-gelu":
        raise NotImplementedError(f"T5 feed_forward_proj={ffp!r} is not built (only gated-gelu: FlanT5)")
    if cfg.get("d_kv", 64) != 64:
        raise NotImplementedError(f"T5 d_kv={cfg.get('d_kv')!r} is not built (tb_attention_rel_fwd takes 64 only)")
    if cfg.get("mm_projector_type", "mlp2x_gelu") not in ("mlp2x_gelu",):
        raise NotImplementedError(f"mm_projector_type={cfg.get('mm_projector_type')!r} is not built (only mlp2x_gelu)")
    if cfg.get("mm_vision_select_layer", -2) != -2:
        raise NotImplementedError(f"mm_vision_select_layer={cfg.get('mm_vision_select_layer')!r} is not built (only -2)")
    L_ = cfg.get("num_layers", 6)
    nd = cfg.get("num_decoder_layers")
    pad = cfg.get("pad_token_id", 0)
    start = cfg.get("decoder_start_token_id")
    return T5Geometry(vocab_size=cfg.get("vocab_size", 32128), d_model=cfg.get("d_model", 512), d_kv=64, d_ff=cfg.get("d_ff", 2048),
                      num_layers=L_, num_decoder_layers=L_ if nd is None else nd, num_heads=cfg.get("num_heads", 8),
                      num_buckets=cfg.get("relative_attention_num_buckets", 32), max_distance=cfg.get("relative_attention_max_distance", 128),
                      eps=cfg.get("layer_norm_epsilon", 1e-6), tie_word_embeddings=bool(cfg.get("tie_word_embeddings", True)),
                      decoder_start_token_id=int(pad if start is None else start), mm_hidden_size=cfg.get("mm_hidden_size", 1024))


def t5_tensor_shapes(geo: T5Geometry) -> Dict[str, Tuple[int, ...]]:
    """name -> shape of every tensor HipCLIPFlanT5 reads, in transformers' T5 names (random full-size models: scratch/bench_vqa.py)"""
    D, I, F, V = geo.d_model, geo.inner, geo.d_ff, geo.vocab_size
    S: Dict[str, Tuple[int, ...]] = {"shared.weight": (V, D), "encoder.final_layer_norm.weight": (D,), "decoder.final_layer_norm.weight": (D,)}
    if not geo.tie_word_embeddings:
        S["lm_head.weight"] = (V, D)
    for side, n in (("encoder", geo.num_layers), ("decoder", geo.num_decoder_layers)):
        S[f"{side}.block.0.layer.0.SelfAttention.relative_attention_bias.weight"] = (geo.num_buckets, geo.num_heads)
        atts = ["0.SelfAttention"] + (["1.EncDecAttention"] if side == "decoder" else [])
        ff = len(atts)
        for i in range(n):
            p = f"{side}.block.{i}.layer."
            for a in atts:
                for x in "qkv":
                    S[f"{p}{a}.{x}.weight"] = (I, D)
                S[f"{p}{a}.o.weight"] = (D, I)
                S[f"{p}{a[0]}.layer_norm.weight"] = (D,)
            for x, shp in (("wi_0", (F, D)), ("wi_1", (F, D)), ("wo", (D, F))):
                S[f"{p}{ff}.DenseReluDense.{x}.weight"] = shp
            S[f"{p}{ff}.layer_norm.weight"] = (D,)
    S.update({"mm_projector.0.weight": (D, geo.mm_hidden_size), "mm_projector.0.bias": (D,), "mm_projector.2.weight": (D, D),
              "mm_projector.2.bias": (D,)})
    return S


# ---------------------------------------------------------------------------------------------------------------- relative-position bias
def relative_position_bucket(rel: torch.Tensor, bidirectional: bool, num_buckets: int, max_distance: int) -> torch.Tensor:
    """T5's bucket of a relative position (key - query), restated from transformers `T5Attention._relative_position_bucket`: half of the
    buckets per sign when bidirectional; exact buckets below num_buckets / 2, logarithmic ones up to max_distance, the last one beyond"""
    buckets = torch.zeros_like(rel)
    if bidirectional:
        num_buckets //= 2
        buckets = buckets + (rel > 0).to(torch.long) * num_buckets
        rel = rel.abs()
    else:
        rel = -torch.min(rel, torch.zeros_like(rel))
    max_exact = num_buckets // 2
    large = max_exact + (torch.log(rel.float() / max_exact) / math.log(max_distance / max_exact) * (num_buckets - max_exact)).to(torch.long)
    large = torch.min(large, torch.full_like(large, num_buckets - 1))
    return buckets + torch.where(rel < max_exact, rel, large)


def relative_bias_vector(table: torch.Tensor, Sq: int, Skv: int, bidirectional: bool, num_buckets: int = 32,
                         max_distance: int = 128) -> torch.Tensor:
    """table [num_buckets, H] (block 0's `relative_attention_bias.weight`, which serves every layer) -> fp32 [H, Sq + Skv - 1] on the host: entry
    d is the bias of every (query i, key j) with j - i = d - (Sq - 1), which is how tb_attention_rel_fwd indexes it"""
    rel = torch.arange(Sq + Skv - 1, dtype=torch.long) - (Sq - 1)
    bucket = relative_position_bucket(rel, bidirectional, num_buckets, max_distance)
    return table.detach().float().cpu()[bucket].t().contiguous()


# ---------------------------------------------------------------------------------------------------------------- checkpoint
def checkpoint_tensors(model_dir: str) -> Iterator[Tuple[str, torch.Tensor]]:
    """(name, tensor) of every tensor of a local checkpoint directory, one at a time: safetensors shards are read tensor by tensor, `.bin`
    shards memory-mapped, so an 11 B parameter model never stands in host memory in fp32"""
    files = sorted(glob.glob(os.path.join(model_dir, "*.safetensors")))
    if files:
        from safetensors import safe_open
        for f in files:
            with safe_open(f, framework="pt", device="cpu") as sf:
                for k in sf.keys():
                    yield k, sf.get_tensor(k)
        return
    files = sorted(glob.glob(os.path.join(model_dir, "pytorch_model*.bin")))
    if not files:
        raise FileNotFoundError(f"{model_dir}: no *.safetensors or pytorch_model*.bin weights")
    for f in files:
        try:
            sd = torch.load(f, map_location="cpu", mmap=True, weights_only=True)
        except (RuntimeError, ValueError):   # a legacy (non-zip) file cannot be mapped
            sd = torch.load(f, map_location="cpu", weights_only=True)
        for k in list(sd):
            yield k, sd.pop(k)


def load_t5_tokenizer(model_dir: str):
    from transformers import AutoTokenizer
    return AutoTokenizer.from_pretrained(model_dir, local_files_only=True)


_ATT = {"q": 0, "k": 1, "v": 2}


class HipCLIPFlanT5:
    """geo: T5Geometry.  tensors: (name, tensor) pairs of the language model in transformers' T5 names (`shared.weight`,
    `encoder.block.N.layer.0.SelfAttention.q.weight`, ..., `lm_head.weight`) plus the projector under any prefix ending
    `mm_projector.{0,2}.{weight,bias}`; other names (a vision tower stored alongside) are ignored.  Each tensor is cast to bf16 and copied into
    its place (q | k | v, cross k | v and wi_0 | wi_1 stacked by rows) as it arrives.  vision: a HipCLIPVision built under the bf16 library
    (`load`, or the caller inside `L.use_half("bf16")`)."""

    def __init__(self, geo: T5Geometry, tensors: Iterable[Tuple[str, torch.Tensor]], vision, device="cuda", half: str = "bf16"):
        if half != "bf16":
            raise NotImplementedError(f"HipCLIPFlanT5 in {half!r} is not built: FlanT5's activations overflow fp16, only bf16 runs")
        if geo.d_kv != 64:
            raise NotImplementedError(f"T5 d_kv={geo.d_kv} is not built (tb_attention_rel_fwd takes 64 only)")
        if vision.patch_w.dtype != torch.bfloat16:
            raise ValueError("the vision tower was not built under L.use_half('bf16')")
        if vision.geo.hidden_size != geo.mm_hidden_size:
            raise ValueError(f"mm_hidden_size={geo.mm_hidden_size} but the vision tower is {vision.geo.hidden_size} wide")
        self.geo, self.vision, self.dev = geo, vision, device
        D, I, F, V = geo.d_model, geo.inner, geo.d_ff, geo.vocab_size
        bf = lambda r, c: torch.empty(r, c, device=device, dtype=torch.bfloat16)
        f32 = lambda n: torch.empty(n, device=device, dtype=torch.float32)
        self.shared = bf(V, D)
        self.lm_head = self.shared if geo.tie_word_embeddings else bf(V, D)
        self.enc = [{"ln1": f32(D), "qkv": bf(3 * I, D), "o": bf(D, I), "ln2": f32(D), "wi": bf(2 * F, D), "wo": bf(D, F)}
                    for _ in range(geo.num_layers)]
        self.dec = [{"ln1": f32(D), "qkv": bf(3 * I, D), "o": bf(D, I), "ln2": f32(D), "cq": bf(I, D), "ckv": bf(2 * I, D), "co": bf(D, I),
                     "ln3": f32(D), "wi": bf(2 * F, D), "wo": bf(D, F)} for _ in range(geo.num_decoder_layers)]
        self.enc_norm, self.dec_norm = f32(D), f32(D)
        self.proj = {"0.weight": bf(D, geo.mm_hidden_size), "0.bias": f32(D), "2.weight": bf(D, D), "2.bias": f32(D)}
        self.rel_table = {"encoder": None, "decoder": None}   # host fp32 [num_buckets, H]
        want = self._slots()
        for name, t in tensors:
            slot = self._slot_of(name)
            if slot is None or slot not in want:
                continue
            dst, rows = want.pop(slot)
            if dst is None:
                self.rel_table[rows] = t.detach().float().cpu().clone()
                continue
            if rows is not None:
                dst = dst[rows[0]:rows[1]]
            if tuple(t.shape) != tuple(dst.shape):
                raise ValueError(f"{name}: shape {tuple(t.shape)}, expected {tuple(dst.shape)}")
            dst.copy_(t.detach().to(dst.dtype))   # cast on the host, tensor by tensor: no fp32 copy of the model anywhere
        if geo.tie_word_embeddings:
            want.pop("lm_head.weight", None)
        missing = sorted(want)
        if any(m.startswith("mm_projector") for m in missing):
            raise ValueError("the checkpoint has no mm_projector.{0,2}.{weight,bias}: " + ", ".join(m for m in missing if m.startswith("mm_")))
        if missing:
            raise ValueError(f"the checkpoint lacks {len(missing)} tensors, e.g. " + ", ".join(missing[:4]))
        self._rel: Dict[Tuple[str, int, int], torch.Tensor] = {}

    # ---- where every checkpoint tensor goes: slot name -> (destination, row range or None)
    def _slots(self):
        g, I, F = self.geo, self.geo.inner, self.geo.d_ff
        s = {"shared.weight": (self.shared, None), "encoder.final_layer_norm.weight": (self.enc_norm, None),
             "decoder.final_layer_norm.weight": (self.dec_norm, None)}
        if not g.tie_word_embeddings:
            s["lm_head.weight"] = (self.lm_head, None)
        for k, t in self.proj.items():
            s["mm_projector." + k] = (t, None)
        for side, blocks in (("encoder", self.enc), ("decoder", self.dec)):
            s[f"{side}.block.0.layer.0.SelfAttention.relative_attention_bias.weight"] = (None, side)
            ff = 1 if side == "encoder" else 2
            for i, W in enumerate(blocks):
                p = f"{side}.block.{i}.layer."
                for n, j in _ATT.items():
                    s[f"{p}0.SelfAttention.{n}.weight"] = (W["qkv"], (j * I, (j + 1) * I))
                s[f"{p}0.SelfAttention.o.weight"] = (W["o"], None)
                s[f"{p}0.layer_norm.weight"] = (W["ln1"], None)
                if side == "decoder":
                    s[f"{p}1.EncDecAttention.q.weight"] = (W["cq"], None)
                    s[f"{p}1.EncDecAttention.k.weight"] = (W["ckv"], (0, I))
                    s[f"{p}1.EncDecAttention.v.weight"] = (W["ckv"], (I, 2 * I))
                    s[f"{p}1.EncDecAttention.o.weight"] = (W["co"], None)
                    s[f"{p}1.layer_norm.weight"] = (W["ln2"], None)
                s[f"{p}{ff}.DenseReluDense.wi_0.weight"] = (W["wi"], (0, F))
                s[f"{p}{ff}.DenseReluDense.wi_1.weight"] = (W["wi"], (F, 2 * F))
                s[f"{p}{ff}.DenseReluDense.wo.weight"] = (W["wo"], None)
                s[f"{p}{ff}.layer_norm.weight"] = (W["ln3" if side == "decoder" else "ln2"], None)
        return s

    @staticmethod
    def _slot_of(name: str) -> Optional[str]:
        """a checkpoint name -> its slot: the projector under any prefix, T5 names with or without a leading `model.` / `transformer.`"""
        i = name.find("mm_projector.")
        if i >= 0:
            return name[i:]
        for pre in ("model.", "transformer."):
            if name.startswith(pre):
                name = name[len(pre):]
        if name in ("encoder.embed_tokens.weight", "decoder.embed_tokens.weight"):
            return None   # copies of shared.weight
        return name

    @classmethod
    def load(cls, vqa_dir: str, clip_dir: str, device="cuda"):
        """the language model and projector from `vqa_dir` (config.json + safetensors / .bin shards), the vision tower from `clip_dir` (a local
        transformers CLIPModel directory), both under the bf16 library"""
        from .clip_score import HipCLIPVision, load_clip_model
        with open(os.path.join(vqa_dir, "config.json")) as f:
            geo = t5_geometry_from_config(json.load(f))
        vg, _, _, sd = load_clip_model(clip_dir)
        with L.use_half("bf16"):
            vision = HipCLIPVision(vg, sd, device=device)
        return cls(geo, checkpoint_tensors(vqa_dir), vision, device=device)

    # ---- forward
    def _bias(self, side: str, Sq: int, Skv: int) -> torch.Tensor:
        key = (side, Sq, Skv)
        if key not in self._rel:
            g = self.geo
            self._rel = {k: v for k, v in self._rel.items() if k[0] != side}   # one shape per side at a time
            self._rel[key] = relative_bias_vector(self.rel_table[side], Sq, Skv, side == "encoder", g.num_buckets, g.max_distance).to(self.dev)
        return self._rel[key]

    def _ff(self, W, x, h_in, h_out, hg, a):
        ops.gemm(x, W["wi"], hg)
        ops.gated_gelu_tanh(hg, a)
        ops.gemm(a, W["wo"], h_out, R=h_in)

    def image_rows(self, images: torch.Tensor) -> torch.Tensor:
        """RGBX [B, S, S] -> fp32 [B, patches, d_model]: the penultimate layer's patch rows (LLaVA's select_layer = -2, CLS dropped) through
        Linear + bias -> erf GELU -> Linear + bias.  The projector runs on every token row and the CLS row is dropped as a strided view."""
        g, v = self.geo, self.vision
        hs = v.hidden_states(images, len(v.layers) - 1)
        B, T, Dv = hs.shape
        x = torch.empty(B * T, Dv, device=self.dev, dtype=torch.bfloat16)
        ops.convert(hs.view(B * T, Dv), x)
        mid = torch.empty(B * T, g.d_model, device=self.dev, dtype=torch.bfloat16)
        ops.gemm(x, self.proj["0.weight"], mid, bias=self.proj["0.bias"], act=L.ACT_GELU)
        out = torch.empty(B * T, g.d_model, device=self.dev, dtype=torch.float32)
        ops.gemm(mid, self.proj["2.weight"], out, bias=self.proj["2.bias"])
        return out.view(B, T, g.d_model)[:, 1:]

    def splice(self, input_ids: Sequence[Sequence[int]], image_rows: torch.Tensor):
        """-> (fp32 [B, T, d_model] right-padded with zeros, int32 [B] true lengths): rows of `shared.weight` for the text ids, the image rows
        where IMAGE_TOKEN_INDEX stands"""
        B, P, D = image_rows.shape
        assert len(input_ids) == B
        lens = []
        for ids in input_ids:
            if sum(1 for t in ids if t == IMAGE_TOKEN_INDEX) != 1:
                raise ValueError("every row needs exactly one image marker")
            lens.append(len(ids) - 1 + P)
        T = max(lens)
        h = torch.zeros(B, T, D, device=self.dev, dtype=torch.float32)
        for b, ids in enumerate(input_ids):
            at = list(ids).index(IMAGE_TOKEN_INDEX)
            text = torch.tensor([t for t in ids if t != IMAGE_TOKEN_INDEX], dtype=torch.long, device=self.dev)
            emb = self.shared[text].float()
            h[b, :at] = emb[:at]
            h[b, at:at + P] = image_rows[b]
            h[b, at + P:lens[b]] = emb[at:]
        return h, torch.tensor(lens, dtype=torch.int32, device=self.dev)

    def encode(self, h: torch.Tensor, kv_len: torch.Tensor) -> torch.Tensor:
        """fp32 [B, T, d_model] + lengths -> the encoder output after its final norm, bf16 [B * T, d_model] (it feeds the cross K/V GEMMs only)"""
        g = self.geo
        B, T, D = h.shape
        M, I, F, H = B * T, g.inner, g.d_ff, g.num_heads
        z = lambda c, dt: torch.empty(M, c, device=self.dev, dtype=dt)
        h = h.reshape(M, D)
        h2, x, qkv, o = z(D, torch.float32), z(D, torch.bfloat16), z(3 * I, torch.bfloat16), z(I, torch.bfloat16)
        hg, a = z(2 * F, torch.bfloat16), z(F, torch.bfloat16)
        rel = self._bias("encoder", T, T)
        for W in self.enc:
            ops.rmsnorm_fwd(h, x, W["ln1"], g.eps)
            ops.gemm(x, W["qkv"], qkv)
            ops.attention_rel_fwd(qkv[:, :I], qkv[:, I:2 * I], qkv[:, 2 * I:], o, None, B, H, T, T, 64, rel=rel, kv_len=kv_len)
            ops.gemm(o, W["o"], h2, R=h)
            ops.rmsnorm_fwd(h2, x, W["ln2"], g.eps)
            self._ff(W, x, h2, h, hg, a)
        ops.rmsnorm_fwd(h, x, self.enc_norm, g.eps)
        return x

    def decode(self, enc_out: torch.Tensor, kv_len: torch.Tensor, decoder_input_ids: Sequence[int], B: int) -> torch.Tensor:
        """the encoder output + one teacher-forced id row shared by the batch -> fp32 logits [B, Td, vocab]"""
        g = self.geo
        Td, D, I, F, H = len(decoder_input_ids), g.d_model, g.inner, g.d_ff, g.num_heads
        M, T = B * Td, enc_out.shape[0] // B
        z = lambda r, c, dt: torch.empty(r, c, device=self.dev, dtype=dt)
        ids = torch.tensor(list(decoder_input_ids), dtype=torch.long, device=self.dev)
        h = self.shared[ids].float().repeat(B, 1).contiguous()
        h2, x, qkv, o = z(M, D, torch.float32), z(M, D, torch.bfloat16), z(M, 3 * I, torch.bfloat16), z(M, I, torch.bfloat16)
        q2, kv2 = z(M, I, torch.bfloat16), z(B * T, 2 * I, torch.bfloat16)
        hg, a = z(M, 2 * F, torch.bfloat16), z(M, F, torch.bfloat16)
        rel = self._bias("decoder", Td, Td)
        for W in self.dec:
            ops.rmsnorm_fwd(h, x, W["ln1"], g.eps)
            ops.gemm(x, W["qkv"], qkv)
            ops.attention_rel_fwd(qkv[:, :I], qkv[:, I:2 * I], qkv[:, 2 * I:], o, None, B, H, Td, Td, 64, rel=rel, causal=True)
            ops.gemm(o, W["o"], h2, R=h)
            ops.rmsnorm_fwd(h2, x, W["ln2"], g.eps)
            ops.gemm(x, W["cq"], q2)
            ops.gemm(enc_out, W["ckv"], kv2)
            ops.attention_rel_fwd(q2, kv2[:, :I], kv2[:, I:], o, None, B, H, Td, T, 64, kv_len=kv_len)
            ops.gemm(o, W["co"], h, R=h2)
            ops.rmsnorm_fwd(h, x, W["ln3"], g.eps)
            self._ff(W, x, h, h2, hg, a)
            h, h2 = h2, h
        ops.rmsnorm_fwd(h, x, self.dec_norm, g.eps)
        logits = z(M, g.vocab_size, torch.float32)
        ops.gemm(x, self.lm_head, logits, alpha=D ** -0.5 if g.tie_word_embeddings else 1.0)
        return logits.view(B, Td, g.vocab_size)

    def logits(self, images: torch.Tensor, input_ids: Sequence[Sequence[int]], decoder_input_ids: Sequence[int]) -> torch.Tensor:
        with L.use_half("bf16"):
            h, kv_len = self.splice(input_ids, self.image_rows(images))
            return self.decode(self.encode(h, kv_len), kv_len, decoder_input_ids, len(input_ids))

    def scores(self, images: torch.Tensor, input_ids: Sequence[Sequence[int]], labels: Sequence[int],
               decoder_input_ids: Sequence[int]) -> torch.Tensor:
        """-> fp32 [B]"""
        return answer_scores(self.logits(images, input_ids, decoder_input_ids), labels)


def answer_scores(logits: torch.Tensor, labels: Sequence[int]) -> torch.Tensor:
    """[3P: t2v_metrics clip_t5_model] per sample exp(-CrossEntropyLoss(mean)(logits[b], labels)): the geometric mean of the label tokens'
    probabilities"""
    lab = torch.tensor(list(labels), dtype=torch.long, device=logits.device)
    logp = torch.log_softmax(logits.float(), dim=-1)
    return logp[:, torch.arange(len(lab), device=logits.device), lab].mean(dim=1).exp()


# ---------------------------------------------------------------------------------------------------------------- images and batching
def pad_to_square(rgb, fill=CLIP_MEAN):
    """uint8 [H, W, 3] -> the image centred on a square of CLIP's mean colour (LLaVA's `expand2square`, image_aspect_ratio = 'pad' [3P]); a
    square image comes back as it is"""
    import numpy as np
    H, W, _ = rgb.shape
    if H == W:
        return rgb
    S = max(H, W)
    out = np.empty((S, S, 3), dtype=np.uint8)
    out[...] = np.array([int(c * 255) for c in fill], dtype=np.uint8)
    y, x = (S - H) // 2, (S - W) // 2
    out[y:y + H, x:x + W] = rgb
    return out


class VQAEvaluator:
    """the image / text batching of the VQA score around one HipCLIPFlanT5, and its throughput over everything it scored"""

    def __init__(self, vqa_dir: str, clip_dir: str, batch_size: int = 32, device="cuda", model=None, tokenizer=None):
        self.model = model if model is not None else HipCLIPFlanT5.load(vqa_dir, clip_dir, device=device)
        self.tokenizer = tokenizer if tokenizer is not None else load_t5_tokenizer(vqa_dir)
        self.batch_size, self.dev = batch_size, device
        self.seconds, self.images = 0.0, 0

    def score_paths(self, paths: Sequence[str], texts: Sequence[str]) -> torch.Tensor:
        from .clip_score import preprocess
        S = self.model.vision.geo.image_size
        out = torch.empty(len(paths), device=self.dev)
        for i in range(0, len(paths), self.batch_size):
            chunk = paths[i:i + self.batch_size]
            batch = torch.empty(len(chunk), S, S, dtype=torch.int32, device=self.dev)
            for j, p in enumerate(chunk):
                batch[j].copy_(preprocess(augment.to_device_image(pad_to_square(load_rgb(p))), S, clip_i=False))
            ids, labels, dec = build_ids(self.tokenizer, texts[i:i + len(chunk)], self.model.geo.decoder_start_token_id)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            out[i:i + len(chunk)] = self.model.scores(batch, ids, labels, dec)
            t1.record()
            t1.synchronize()
            self.seconds += t0.elapsed_time(t1) / 1e3
            self.images += len(chunk)
        return out

    def release(self):
        """free the model's device memory (the counters stay)"""
        self.model = None
        torch.cuda.empty_cache()

    def images_per_second(self) -> float:
        return self.images / self.seconds if self.seconds > 0 else 0.0
