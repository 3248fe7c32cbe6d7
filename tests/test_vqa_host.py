"""CPU tests of the VQA score's host side (textboost_amd/vqa_score.py): the plain-torch restatement tests/vqa_ref.py against transformers'
T5ForConditionalGeneration, the relative-position bias vector against T5Attention.compute_bias, the prompt-id construction on a tiny tokenizer,
where the checkpoint's tensors land, and the CLI's refusals."""
import json
import os

import pytest
import torch

import vqa_ref as R


def _hf_model(cfg, sd):
    from transformers import T5Config, T5ForConditionalGeneration
    m = T5ForConditionalGeneration(T5Config(**{k: v for k, v in cfg.items() if not k.startswith("mm_")})).eval()
    t5 = {k: v for k, v in sd.items() if "mm_projector" not in k}
    tied = cfg["tie_word_embeddings"]
    missing, unexpected = m.load_state_dict({k: v for k, v in t5.items() if k != "lm_head.weight"}, strict=False)
    assert not unexpected and all(k.endswith("embed_tokens.weight") or k == "lm_head.weight" for k in missing), (missing, unexpected)
    if not tied:   # a head of its own, whatever this transformers version ties at construction
        m.lm_head.weight = torch.nn.Parameter(sd["lm_head.weight"].clone())
    assert torch.equal(m.shared.weight, sd["shared.weight"]) and torch.equal(m.encoder.embed_tokens.weight, sd["shared.weight"])
    return m


@pytest.mark.parametrize("tied", [False, True])
def test_restatement_matches_transformers_t5(tied):
    pytest.importorskip("transformers")
    cfg = R.tiny_t5_config(tie_word_embeddings=tied)
    sd = R.random_t5_state(cfg, 3)
    m = _hf_model(cfg, sd)
    g = torch.Generator().manual_seed(1)
    B, T = 3, 140
    mask = torch.ones(B, T, dtype=torch.long)
    mask[1, 97:] = 0      # right-padded rows
    mask[2, 5:] = 0
    emb = torch.randn(B, T, cfg["d_model"], generator=g) * mask[..., None]
    dec = torch.tensor([[0, 17, 1]] * B)
    with torch.no_grad():
        want = m(inputs_embeds=emb, attention_mask=mask, decoder_input_ids=dec).logits
        got = R.t5_logits(sd, cfg, emb, mask, dec)
    err = (got - want).abs().max().item() / want.abs().max().item()
    print(f"[restatement vs transformers, tied={tied}] max |d| / max |logit| = {err:.2e}")
    assert err <= 1e-5, err


@pytest.mark.parametrize("bidirectional", [True, False])
@pytest.mark.parametrize("Sq,Skv", [(2, 2), (70, 70), (130, 130), (2, 70)])   # 130 crosses max_distance = 128
def test_relative_bias_vector_expands_to_compute_bias(Sq, Skv, bidirectional):
    pytest.importorskip("transformers")
    from transformers import T5Config
    from transformers.models.t5.modeling_t5 import T5Attention
    from textboost_amd.vqa_score import relative_bias_vector
    torch.manual_seed(Sq + Skv)
    cfg = T5Config(d_model=128, d_kv=64, num_heads=3, relative_attention_num_buckets=32, relative_attention_max_distance=128,
                   is_decoder=not bidirectional)
    att = T5Attention(cfg, has_relative_attention_bias=True)
    torch.nn.init.normal_(att.relative_attention_bias.weight)
    with torch.no_grad():
        want = att.compute_bias(Sq, Skv)[0]                                    # [H, Sq, Skv]
    vec = relative_bias_vector(att.relative_attention_bias.weight, Sq, Skv, bidirectional, 32, 128)
    assert vec.shape == (3, Sq + Skv - 1) and vec.dtype == torch.float32
    i, j = torch.arange(Sq)[:, None], torch.arange(Skv)[None, :]
    assert torch.equal(vec[:, j - i + Sq - 1], want)
    assert torch.equal(R.position_bias(att.relative_attention_bias.weight.detach(), Sq, Skv, bidirectional, 32, 128), want)


def test_prompt_ids(tmp_path):
    pytest.importorskip("transformers")
    from textboost_amd import vqa_score as V
    texts = ["a dog in the snow", "a red can"]
    prompts = [V.T5_CHAT_TEMPLATE.format(question=V.QUESTION_TEMPLATE.format(t)) for t in texts]
    assert prompts[0].count(V.IMAGE_MARKER) == 1 and "USER: <image>\n" in prompts[0] and prompts[0].endswith("no. ASSISTANT:")
    assert 'Does this figure show "a dog in the snow"? Please answer yes or no.' in prompts[0]
    R.write_tiny_tokenizer(str(tmp_path), prompts + [V.ANSWER_TEMPLATE])
    tok = V.load_t5_tokenizer(str(tmp_path))
    ids, labels, dec = V.build_ids(tok, texts)
    EOS, PAD = tok.eos_token_id, tok.pad_token_id
    assert (EOS, PAD) == (1, 0)
    for row, prompt in zip(ids, prompts):
        assert row.count(V.IMAGE_TOKEN_INDEX) == 1                      # one image marker per row
        at = row.index(V.IMAGE_TOKEN_INDEX)
        head, tail = prompt.split(V.IMAGE_MARKER)
        # the documented EOS convention: every chunk is tokenised on its own and keeps the EOS the tokenizer appends
        assert row[:at] == tok(head).input_ids and row[at - 1] == EOS
        assert row[at + 1:] == tok(tail).input_ids and row[-1] == EOS
        assert row.count(EOS) == 2 and 2 not in row                     # no <unk>: the tiny vocabulary covers the prompt
    assert len(ids[0]) != len(ids[1])
    assert labels == tok("Yes").input_ids and labels[-1] == EOS and len(labels) == 2
    assert dec == [PAD] + labels[:-1]                                   # teacher forcing: the labels shifted right behind the start token
    assert V.build_ids(tok, texts, decoder_start_id=5)[2][0] == 5


def test_answer_scores_are_exp_of_minus_mean_ce():
    from textboost_amd.vqa_score import answer_scores
    g = torch.Generator().manual_seed(0)
    logits = torch.randn(3, 2, 16, generator=g)
    p = logits.softmax(-1)
    want = (p[:, 0, 7] * p[:, 1, 1]).sqrt()
    assert torch.allclose(answer_scores(logits, [7, 1]), want, rtol=1e-6)
    assert torch.allclose(R.answer_scores(logits, [7, 1]), want, rtol=1e-6)


def test_pad_to_square():
    import numpy as np
    from textboost_amd.vqa_score import pad_to_square
    sq = np.zeros((5, 5, 3), np.uint8)
    assert pad_to_square(sq) is sq
    out = pad_to_square(np.full((2, 5, 3), 9, np.uint8))
    assert out.shape == (5, 5, 3) and (out[1:3] == 9).all() and out[0, 0].tolist() == [122, 116, 104] and out[4, 4].tolist() == [122, 116, 104]


def _tiny_vision():
    from textboost_amd import models
    from textboost_amd.clip_score import CLIPVisionGeometry, HipCLIPVision
    from textboost_amd.text_encoder import CLIPGeometry
    vg = CLIPVisionGeometry(image_size=56, patch_size=14, hidden_size=64, intermediate_size=128, num_layers=2, num_heads=1, projection_dim=32)
    tg = CLIPGeometry(vocab_size=64, hidden_size=32, intermediate_size=64, num_layers=1, num_heads=2, max_pos=8)
    return HipCLIPVision(vg, models.random_state_dict(models.clip_model_shapes(vg, tg), 3), device="cpu")


def test_checkpoint_tensors_land_in_their_slots(tmp_path):
    """streamed from a safetensors directory, on the host: stacked q | k | v, cross k | v and wi_0 | wi_1, bf16 matrices, fp32 norms, the
    projector under a prefix, and the refusals of the constructor"""
    from textboost_amd import _lib as L
    from textboost_amd import vqa_score as V
    cfg = R.tiny_t5_config()
    sd = R.random_t5_state(cfg, 5)
    R.write_vqa_model(str(tmp_path), cfg, sd, ["Yes"])
    geo = V.t5_geometry_from_config(json.load(open(tmp_path / "config.json")))
    assert (geo.d_model, geo.num_heads, geo.d_ff, geo.num_layers, geo.num_decoder_layers, geo.tie_word_embeddings) == (128, 2, 256, 2, 2, False)
    with L.use_half("bf16"):
        vision = _tiny_vision()
    m = V.HipCLIPFlanT5(geo, V.checkpoint_tensors(str(tmp_path)), vision, device="cpu")
    bf = lambda k: sd[k].to(torch.bfloat16)
    e, d = "encoder.block.1.layer.", "decoder.block.1.layer."
    assert m.enc[1]["qkv"].dtype == torch.bfloat16
    assert torch.equal(m.enc[1]["qkv"], torch.cat([bf(f"{e}0.SelfAttention.{x}.weight") for x in "qkv"]))
    assert torch.equal(m.enc[1]["wi"], torch.cat([bf(f"{e}1.DenseReluDense.wi_{x}.weight") for x in "01"]))
    assert torch.equal(m.enc[1]["ln2"], sd[f"{e}1.layer_norm.weight"]) and m.enc[1]["ln2"].dtype == torch.float32
    assert torch.equal(m.dec[1]["ckv"], torch.cat([bf(f"{d}1.EncDecAttention.{x}.weight") for x in "kv"]))
    assert torch.equal(m.dec[1]["cq"], bf(f"{d}1.EncDecAttention.q.weight")) and torch.equal(m.dec[1]["co"], bf(f"{d}1.EncDecAttention.o.weight"))
    assert torch.equal(m.dec[1]["ln2"], sd[f"{d}1.layer_norm.weight"]) and torch.equal(m.dec[1]["ln3"], sd[f"{d}2.layer_norm.weight"])
    assert torch.equal(m.dec[1]["wo"], bf(f"{d}2.DenseReluDense.wo.weight"))
    assert torch.equal(m.proj["2.weight"], bf("model.mm_projector.2.weight")) and torch.equal(m.proj["0.bias"], sd["model.mm_projector.0.bias"])
    assert torch.equal(m.lm_head, bf("lm_head.weight")) and m.lm_head is not m.shared
    assert torch.equal(m.rel_table["decoder"], sd["decoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"])
    with pytest.raises(NotImplementedError, match="fp16"):
        V.HipCLIPFlanT5(geo, sd.items(), vision, device="cpu", half="fp16")
    with pytest.raises(ValueError, match="mm_projector"):
        V.HipCLIPFlanT5(geo, [(k, v) for k, v in sd.items() if "mm_projector" not in k], vision, device="cpu")
    with pytest.raises(ValueError, match="lacks"):
        V.HipCLIPFlanT5(geo, [(k, v) for k, v in sd.items() if "block.1.layer.0.SelfAttention.k" not in k], vision, device="cpu")
    with pytest.raises(ValueError, match="use_half"):
        V.HipCLIPFlanT5(geo, sd.items(), _tiny_vision(), device="cpu")          # an fp16 vision tower
    tied = V.HipCLIPFlanT5(V.t5_geometry_from_config(R.tiny_t5_config(tie_word_embeddings=True)), sd.items(), vision, device="cpu")
    assert tied.lm_head is tied.shared


def test_config_refusals():
    from textboost_amd.vqa_score import t5_geometry_from_config
    with pytest.raises(NotImplementedError, match="feed_forward_proj"):
        t5_geometry_from_config(R.tiny_t5_config(feed_forward_proj="relu"))
    with pytest.raises(NotImplementedError, match="feed_forward_proj"):
        t5_geometry_from_config(R.tiny_t5_config(feed_forward_proj="gated-silu"))
    with pytest.raises(NotImplementedError, match="d_kv"):
        t5_geometry_from_config(R.tiny_t5_config(d_kv=32))
    with pytest.raises(NotImplementedError, match="mm_vision_select_layer"):
        t5_geometry_from_config(R.tiny_t5_config(mm_vision_select_layer=-1))


def _args(tmp_path, *extra):
    import eval_dreambooth as E
    return E.build_parser().parse_args([str(tmp_path / "runs" / "tb-sd15-n1"), "--outdir", str(tmp_path / "bench"), *extra])


def test_cli_refusals_and_acceptance(tmp_path):
    import eval_dreambooth as E
    cm, vm = ["--clip-model", str(tmp_path)], ["--vqa-model", str(tmp_path)]
    with pytest.raises(SystemExit, match="vqa is not built"):                       # the old wording without --vqa-model
        E.check_args(_args(tmp_path, "--skip-gen", "--metric", "vqa", *cm))
    with pytest.raises(SystemExit, match="pass --metric clip-t clip-i"):
        E.check_args(_args(tmp_path, "--skip-gen", *cm))                            # the default --metric names vqa
    with pytest.raises(SystemExit, match="--vqa-model"):                            # ... and now says how to build it
        E.check_args(_args(tmp_path, "--skip-gen", *cm))
    with pytest.raises(SystemExit, match="--clip-model"):
        E.check_args(_args(tmp_path, "--skip-gen", "--metric", "vqa", *vm))
    with pytest.raises(SystemExit, match="unknown --metric"):
        E.check_args(_args(tmp_path, "--skip-gen", "--metric", "vqa2", *cm, *vm))
    E.check_args(_args(tmp_path, "--skip-gen", "--metric", "vqa", *cm, *vm))
    E.check_args(_args(tmp_path, "--skip-gen", *cm, *vm))                           # the reference's default: clip-t clip-i vqa


class _FakeVQA:
    batch_size, images = 4, 0

    def __init__(self, table):
        self.table, self.released = table, 0

    def score_paths(self, paths, texts):
        assert not self.released
        self.images += len(paths)
        return torch.tensor([self.table[t] for t in texts])

    def release(self):
        self.released += 1

    def images_per_second(self):
        return 1.0


def test_cli_fills_the_vqa_column(tmp_path):
    """the CSV plumbing with a fake model: text = the file name, the mean over every seed<s>/*/*.png as %.3f, the other columns 0.000, the
    model released once, after the last seed"""
    import csv
    import eval_dreambooth as E
    table = {"a dog": 0.25, "a red dog": 0.5, "a can": 0.8125}
    for s, names in ((0, {"dog": ["a_dog", "a_red_dog"], "can": ["a_can"]}), (1, {"dog": ["a_dog"], "can": ["a_can"]})):
        for inst, ns in names.items():
            d = tmp_path / "bench" / "tb-sd15-n1" / f"seed{s}" / inst
            d.mkdir(parents=True)
            for n in ns:
                (d / f"{n}.png").write_bytes(b"")
    (tmp_path / "runs" / "tb-sd15-n1").mkdir(parents=True)
    a = _args(tmp_path, "--skip-gen", "--metric", "vqa", "--seeds", "0", "1", "--clip-model", "x", "--vqa-model", "y")
    fake = _FakeVQA(table)
    E.evaluate(a, vqa_evaluator=fake)
    rows = list(csv.reader(open(tmp_path / "runs" / "tb-sd15-n1" / "metric_last.csv")))
    assert rows[0] == ["seed", "clip_score", "vqa_score", "clip_i", "clip_i_unseen", "dino", "dino_unseen"]
    assert rows[1] == ["0", "0.000", f"{(0.25 + 0.5 + 0.8125) / 3:.3f}", "0.000", "0.000", "0.000", "0.000"]
    assert rows[2] == ["1", "0.000", f"{(0.25 + 0.8125) / 2:.3f}", "0.000", "0.000", "0.000", "0.000"]
    assert fake.released == 1 and fake.images == 5


def test_splice_matches_restatement():
    """rows of shared.weight for the text ids, the image rows where the marker stands, zero padding on the right, true lengths"""
    from textboost_amd import _lib as L
    from textboost_amd import vqa_score as V
    cfg = R.tiny_t5_config()
    sd = R.random_t5_state(cfg, 5)
    with L.use_half("bf16"):
        vision = _tiny_vision()
    m = V.HipCLIPFlanT5(V.t5_geometry_from_config(cfg), sd.items(), vision, device="cpu")
    g = torch.Generator().manual_seed(0)
    img = torch.randn(3, 16, cfg["d_model"], generator=g)
    ids = [[5, 6, 1, V.IMAGE_TOKEN_INDEX, 7, 1], [V.IMAGE_TOKEN_INDEX, 9, 9, 9, 9, 9, 1], [4, 1, V.IMAGE_TOKEN_INDEX]]
    h, lens = m.splice(ids, img)
    want, mask = R.splice(sd["shared.weight"].to(torch.bfloat16).float(), ids, img)
    assert lens.dtype == torch.int32 and lens.tolist() == mask.sum(1).tolist() == [21, 22, 18]
    assert h.dtype == torch.float32 and torch.equal(h, want)
    with pytest.raises(ValueError, match="image marker"):
        m.splice([[5, 6, 1]], img[:1])
