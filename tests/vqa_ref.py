"""Plain-torch restatement of the whole VQA score of textboost_amd/vqa_score.py: CLIP's penultimate hidden state (tests/clip_ref.py), the
mm_projector, the splice of image rows into the embedded question, a gated-GELU T5 encoder and decoder with their relative-position bias, the
cross-entropy of the answer and its exponential.  It runs in the dtype of its weights (fp32, or float64 after `to64`).  Host code only; the T5
half is pinned against transformers' T5ForConditionalGeneration by tests/test_vqa_host.py.  The `ablate` switches break one convention each, so
that a test can show its inputs would expose the matching mistake in the device code."""
import math

import torch
import torch.nn.functional as F

import clip_ref

IMAGE_TOKEN_INDEX = -200


# ---------------------------------------------------------------------------------------------------- configs and random weights
def tiny_t5_config(**kw):
    cfg = dict(vocab_size=128, d_model=128, d_kv=64, d_ff=256, num_layers=2, num_decoder_layers=2, num_heads=2,
               relative_attention_num_buckets=32, relative_attention_max_distance=128, layer_norm_epsilon=1e-6, feed_forward_proj="gated-gelu",
               tie_word_embeddings=False, pad_token_id=0, eos_token_id=1, decoder_start_token_id=0, mm_hidden_size=64,
               mm_projector_type="mlp2x_gelu", mm_vision_select_layer=-2)
    cfg.update(kw)
    return cfg


def t5_shapes(cfg):
    D, I, Ff, V, H = cfg["d_model"], cfg["num_heads"] * cfg["d_kv"], cfg["d_ff"], cfg["vocab_size"], cfg["num_heads"]
    S = {"shared.weight": (V, D), "encoder.final_layer_norm.weight": (D,), "decoder.final_layer_norm.weight": (D,)}
    if not cfg.get("tie_word_embeddings", True):
        S["lm_head.weight"] = (V, D)
    for side, n in (("encoder", cfg["num_layers"]), ("decoder", cfg["num_decoder_layers"])):
        S[f"{side}.block.0.layer.0.SelfAttention.relative_attention_bias.weight"] = (cfg["relative_attention_num_buckets"], H)
        ff = 1 if side == "encoder" else 2
        for i in range(n):
            p = f"{side}.block.{i}.layer."
            atts = ["0.SelfAttention"] + (["1.EncDecAttention"] if side == "decoder" else [])
            for a in atts:
                for x in "qkv":
                    S[f"{p}{a}.{x}.weight"] = (I, D)
                S[f"{p}{a}.o.weight"] = (D, I)
                S[f"{p}{a.split('.')[0]}.layer_norm.weight"] = (D,)
            S[f"{p}{ff}.DenseReluDense.wi_0.weight"] = (Ff, D)
            S[f"{p}{ff}.DenseReluDense.wi_1.weight"] = (Ff, D)
            S[f"{p}{ff}.DenseReluDense.wo.weight"] = (D, Ff)
            S[f"{p}{ff}.layer_norm.weight"] = (D,)
    Dv = cfg["mm_hidden_size"]
    S.update({"model.mm_projector.0.weight": (D, Dv), "model.mm_projector.0.bias": (D,), "model.mm_projector.2.weight": (D, D),
              "model.mm_projector.2.bias": (D,)})
    return S


def random_t5_state(cfg, seed, gain=1.0, rel_std=1.0, head_gain=1.0):
    """N(0, gain^2 / fan_in) matrices (q and k: N(0, gain / fan_in), so scores of unit-RMS rows have a spread of about `gain`), norm weights
    1 + 0.1 N, embeddings N(0, 1), bias table N(0, rel_std^2), lm_head N(0, head_gain^2 / fan_in), projector biases 0.1 N"""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shp in t5_shapes(cfg).items():
        r = torch.randn(shp, generator=g)
        if k.endswith("layer_norm.weight"):
            t = 1.0 + 0.1 * r
        elif k == "shared.weight":
            t = r
        elif "relative_attention_bias" in k:
            t = rel_std * r
        elif k.endswith(".bias"):
            t = 0.1 * r
        elif k == "lm_head.weight":
            t = r * head_gain * shp[1] ** -0.5
        elif "mm_projector" in k:
            t = r * shp[1] ** -0.5
        elif k.endswith(".q.weight") or k.endswith(".k.weight"):
            t = r * (gain ** 0.5) * shp[1] ** -0.5
        else:
            t = r * gain * shp[1] ** -0.5
        sd[k] = t
    return sd


def to64(sd):
    return {k: v.double() for k, v in sd.items()}


# ---------------------------------------------------------------------------------------------------- T5
def relative_position_bucket(rel, bidirectional, num_buckets, max_distance):
    """bucket of rel = key position - query position (an int64 tensor)"""
    out = torch.zeros_like(rel)
    n = num_buckets
    if bidirectional:
        n //= 2
        out = out + (rel > 0).long() * n
        rel = rel.abs()
    else:
        rel = (-rel).clamp_min(0)
    exact = n // 2
    log_part = torch.log(rel.float() / exact) / math.log(max_distance / exact) * (n - exact)
    large = (exact + log_part.long()).clamp_max(n - 1)
    return out + torch.where(rel < exact, rel, large)


def position_bias(table, Sq, Skv, bidirectional, num_buckets, max_distance):
    """table [num_buckets, H] -> [H, Sq, Skv]"""
    rel = torch.arange(Skv)[None, :] - torch.arange(Sq)[:, None]
    return table[relative_position_bucket(rel, bidirectional, num_buckets, max_distance)].permute(2, 0, 1)


def rmsnorm(x, w, eps):
    return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * w


def gelu_new(x):
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x.pow(3))))


def _attention(sd, p, x, src, H, bias):
    """x [B, Sq, D] queries, src [B, Skv, D] keys / values, bias broadcastable to [B, H, Sq, Skv] (position bias + masks); no 1/sqrt(d) scale"""
    B, Sq, _ = x.shape
    split = lambda t: t.reshape(B, t.shape[1], H, -1).transpose(1, 2)
    q, k, v = split(x @ sd[p + "q.weight"].t()), split(src @ sd[p + "k.weight"].t()), split(src @ sd[p + "v.weight"].t())
    s = q @ k.transpose(-1, -2) + bias
    o = (s.softmax(-1) @ v).transpose(1, 2).reshape(B, Sq, -1)
    return o @ sd[p + "o.weight"].t()


def _ff(sd, p, x):
    return (gelu_new(x @ sd[p + "wi_0.weight"].t()) * (x @ sd[p + "wi_1.weight"].t())) @ sd[p + "wo.weight"].t()


def _key_mask(mask, dtype):
    """attention_mask [B, Skv] of 0 / 1 -> additive [B, 1, 1, Skv]"""
    return torch.zeros(mask.shape, dtype=dtype).masked_fill(mask == 0, float("-inf"))[:, None, None, :]


def t5_encoder(sd, cfg, embeds, mask, use_rel=True):
    H, eps = cfg["num_heads"], cfg["layer_norm_epsilon"]
    B, T, _ = embeds.shape
    bias = _key_mask(mask, embeds.dtype)
    if use_rel:
        table = sd["encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"]
        bias = bias + position_bias(table, T, T, True, cfg["relative_attention_num_buckets"], cfg["relative_attention_max_distance"])[None]
    h = embeds
    for i in range(cfg["num_layers"]):
        p = f"encoder.block.{i}.layer."
        x = rmsnorm(h, sd[p + "0.layer_norm.weight"], eps)
        h = h + _attention(sd, p + "0.SelfAttention.", x, x, H, bias)
        h = h + _ff(sd, p + "1.DenseReluDense.", rmsnorm(h, sd[p + "1.layer_norm.weight"], eps))
    return rmsnorm(h, sd["encoder.final_layer_norm.weight"], eps)


def t5_decoder(sd, cfg, enc_out, mask, decoder_input_ids, use_rel=True):
    """decoder_input_ids int64 [B, Td] -> logits [B, Td, vocab]"""
    H, eps = cfg["num_heads"], cfg["layer_norm_epsilon"]
    Td = decoder_input_ids.shape[1]
    h = sd["shared.weight"][decoder_input_ids]
    causal = torch.zeros(Td, Td, dtype=h.dtype).masked_fill(torch.ones(Td, Td, dtype=torch.bool).triu(1), float("-inf"))
    self_bias = causal[None, None]
    if use_rel:
        table = sd["decoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"]
        self_bias = self_bias + position_bias(table, Td, Td, False, cfg["relative_attention_num_buckets"],
                                              cfg["relative_attention_max_distance"])[None]
    cross_bias = _key_mask(mask, h.dtype)
    for i in range(cfg["num_decoder_layers"]):
        p = f"decoder.block.{i}.layer."
        x = rmsnorm(h, sd[p + "0.layer_norm.weight"], eps)
        h = h + _attention(sd, p + "0.SelfAttention.", x, x, H, self_bias)
        h = h + _attention(sd, p + "1.EncDecAttention.", rmsnorm(h, sd[p + "1.layer_norm.weight"], eps), enc_out, H, cross_bias)
        h = h + _ff(sd, p + "2.DenseReluDense.", rmsnorm(h, sd[p + "2.layer_norm.weight"], eps))
    h = rmsnorm(h, sd["decoder.final_layer_norm.weight"], eps)
    if cfg.get("tie_word_embeddings", True):
        return (h * cfg["d_model"] ** -0.5) @ sd["shared.weight"].t()
    return h @ sd["lm_head.weight"].t()


def t5_logits(sd, cfg, inputs_embeds, attention_mask, decoder_input_ids, use_rel=True):
    enc = t5_encoder(sd, cfg, inputs_embeds, attention_mask, use_rel)
    return t5_decoder(sd, cfg, enc, attention_mask, decoder_input_ids, use_rel)


# ---------------------------------------------------------------------------------------------------- the multimodal front
def projector(sd, hs):
    w = {k[k.index("mm_projector."):]: v for k, v in sd.items() if "mm_projector." in k}
    x = F.gelu(hs @ w["mm_projector.0.weight"].t() + w["mm_projector.0.bias"])   # erf GELU
    return x @ w["mm_projector.2.weight"].t() + w["mm_projector.2.bias"]


def splice(shared, input_ids, image_rows):
    """-> (embeds [B, T, D] right-padded with zeros, attention_mask [B, T])"""
    rows = []
    for ids, img in zip(input_ids, image_rows):
        at = list(ids).index(IMAGE_TOKEN_INDEX)
        assert list(ids).count(IMAGE_TOKEN_INDEX) == 1
        rows.append(torch.cat([shared[torch.tensor(list(ids[:at]), dtype=torch.long)], img,
                               shared[torch.tensor(list(ids[at + 1:]), dtype=torch.long)]]))
    T = max(r.shape[0] for r in rows)
    emb = torch.zeros(len(rows), T, shared.shape[1], dtype=shared.dtype)
    mask = torch.zeros(len(rows), T, dtype=torch.long)
    for b, r in enumerate(rows):
        emb[b, :r.shape[0]] = r
        mask[b, :r.shape[0]] = 1
    return emb, mask


def vqa_logits(clip_sd, clip_cfg, t5_sd, t5_cfg, pixel_values, input_ids, decoder_input_ids, ablate=None):
    """pixel_values [B, 3, S, S] (CLIP-normalised) -> logits [B, Td, vocab].  ablate: None | "no_rel" | "no_len" | "swap_images" | "last_layer" """
    hs = clip_ref.vision_residuals(clip_sd, clip_cfg, pixel_values.to(t5_sd["shared.weight"].dtype))
    img = projector(t5_sd, hs[-1 if ablate == "last_layer" else -2][:, 1:])   # select_layer = -2, CLS dropped
    if ablate == "swap_images":
        img = img[[1, 0] + list(range(2, img.shape[0]))]
    emb, mask = splice(t5_sd["shared.weight"], input_ids, img)
    if ablate == "no_len":
        mask = torch.ones_like(mask)
    dec = torch.tensor(list(decoder_input_ids), dtype=torch.long)[None].expand(len(input_ids), -1)
    return t5_logits(t5_sd, t5_cfg, emb, mask, dec, use_rel=ablate != "no_rel")


def answer_scores(logits, labels):
    """per sample exp(-CrossEntropyLoss(reduction='mean')(logits[b], labels))"""
    lab = torch.tensor(list(labels), dtype=torch.long)
    return torch.stack([(-F.cross_entropy(l, lab)).exp() for l in logits])


# ---------------------------------------------------------------------------------------------------- model / tokenizer directories for tests
def write_tiny_tokenizer(d, texts, vocab_size=128):
    """a word-level tokenizer directory that AutoTokenizer loads: <pad> 0, </s> 1, <unk> 2, then the words of `texts`; like T5's it appends
    </s> to everything it tokenises"""
    import json
    import os
    from tokenizers import Tokenizer, models, pre_tokenizers, processors
    os.makedirs(d, exist_ok=True)
    pre = pre_tokenizers.Whitespace()
    vocab = {"<pad>": 0, "</s>": 1, "<unk>": 2}
    for t in texts:
        for w, _ in pre.pre_tokenize_str(t):
            if w not in vocab and len(vocab) < vocab_size:
                vocab[w] = len(vocab)
    tok = Tokenizer(models.WordLevel(vocab, unk_token="<unk>"))
    tok.pre_tokenizer = pre
    tok.post_processor = processors.TemplateProcessing(single="$A </s>", special_tokens=[("</s>", 1)])
    tok.save(os.path.join(d, "tokenizer.json"))
    with open(os.path.join(d, "tokenizer_config.json"), "w") as f:
        json.dump({"tokenizer_class": "PreTrainedTokenizerFast", "pad_token": "<pad>", "eos_token": "</s>", "unk_token": "<unk>"}, f)
    return vocab


def write_vqa_model(d, cfg, sd, texts):
    """a clip-flant5 directory: config.json, model.safetensors (T5 names + `model.mm_projector.*`), the tiny tokenizer"""
    import json
    import os
    from safetensors.torch import save_file
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "config.json"), "w") as f:
        json.dump(dict(cfg, model_type="t5"), f)
    save_file({k: v.contiguous() for k, v in sd.items()}, os.path.join(d, "model.safetensors"))
    return write_tiny_tokenizer(d, texts, cfg["vocab_size"])
