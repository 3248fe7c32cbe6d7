"""Host side of composing trained runs (textboost_amd/compose.py, generate.read_run_dir's unet/ reader, inference.py --with): no GPU."""
import os
import types

import pytest
import torch

D_TEXT, LAYERS = 64, 2
PROJ = ("q_proj", "k_proj", "v_proj")


def module_names(layers=LAYERS):
    return [f"base_model.model.text_model.encoder.layers.{i}.self_attn.{p}" for i in range(layers) for p in PROJ]


def write_run(d, tokens, aug, seed, rank, D=D_TEXT, layers=LAYERS, keep_rows=None):
    """what train_textboost.py leaves in <output_dir>, through checkpoint.py: a rank-`rank` adapter with non-zero B (keep_rows "even" / "odd":
    the other output rows of every lora_B zeroed, as --mixing leaves them), placeholder rows [D], augmentation rows [1, D].
    -> (lora_A [L, 3r, D], lora_B [L, 3D, r], {token: row})"""
    from textboost_amd import checkpoint as ckpt
    g = torch.Generator().manual_seed(seed)
    names = list(tokens) + list(aug)
    r = max(rank, 1)
    A = torch.randn(layers, 3 * r, D, generator=g) / r
    B = torch.randn(layers, 3 * D, r, generator=g) * 0.05
    if keep_rows is not None:
        B[:, (1 if keep_rows == "even" else 0)::2] = 0          # (D is even: the parity of a row of [3D, r] is its parity inside its projection)
    te = types.SimpleNamespace(geo=types.SimpleNamespace(hidden_size=D, num_layers=layers), r=rank, lora_A=A, lora_B=B,
                               token_table=torch.randn(len(names), D, generator=g) * 0.01)
    ckpt.save_text_encoder_adapter(te, os.path.join(d, "text_encoder"), "tiny")
    ckpt.save_token_embeddings(te, d, {t: i for i, t in enumerate(tokens)}, {t: len(tokens) + i for i, t in enumerate(aug)})
    return A, B, {t: te.token_table[i] for i, t in enumerate(names)}


def stub_kv_unet(xattn, Dc, r, seed, b_std=0.3):
    """the attributes of a HipUNet that checkpoint.save_unet_adapters reads, with trained-looking (non-zero B) K/V adapters"""
    g = torch.Generator().manual_seed(seed)
    kv_off, o = {}, 0
    for p, C in xattn:
        kv_off[p] = o
        o += 2 * C
    return types.SimpleNamespace(kv_r=r, xattn=list(xattn), kv_off=kv_off, kv_total=o,
                                 kv_lora_A=torch.randn(len(xattn), 2 * r, Dc, generator=g) / r,
                                 kv_lora_B=torch.randn(o, r, generator=g) * b_std)


def merged_delta(run_parts, name, dtype=torch.float64):
    """sum_i w_i B_i A_i of module `name` over [(run, w)] in `dtype`"""
    return sum(w * (run.lora[name + ".lora_B.weight"].to(dtype) @ run.lora[name + ".lora_A.weight"].to(dtype)) for run, w in run_parts)


@pytest.fixture()
def two_runs(tmp_path):
    from textboost_amd import generate as G
    da, db = str(tmp_path / "dog"), str(tmp_path / "style")
    write_run(da, ["<dog>"], ["<hflip>"], seed=1, rank=4)
    write_run(db, ["<style>"], ["<hflip>", "<grayscale_0>"], seed=2, rank=8)
    return G.read_run_dir(da), G.read_run_dir(db)


# ------------------------------------------------------------------------------------------------ algebra
def test_rank_concatenation_is_the_weighted_sum(two_runs):
    from textboost_amd.compose import compose_runs
    a, b = two_runs
    c = compose_runs([a, b], [1.0, 0.7])
    assert c.rank == 12 and set(c.lora) == set(a.lora) and c.path == a.path and c.files == a.files
    worst = 0.0
    for name in module_names():
        A, B = c.lora[name + ".lora_A.weight"], c.lora[name + ".lora_B.weight"]
        assert A.shape == (12, D_TEXT) and B.shape == (D_TEXT, 12) and A.dtype == B.dtype == torch.float32
        assert A.is_contiguous() and B.is_contiguous()
        got, want = B.double() @ A.double(), merged_delta([(a, 1.0), (b, 0.7)], name)
        worst = max(worst, ((got - want).norm() / want.norm()).item())
    print(f"[compose] B_c A_c vs sum w_i B_i A_i in float64: worst rel-L2 {worst:.2e}")
    assert worst <= 1e-6            # the only rounding: w * B in fp32 (2^-24 per element)


def test_one_run_zero_weight_and_rank_zero(two_runs, tmp_path):
    from textboost_amd import generate as G
    from textboost_amd.compose import compose_runs
    a, b = two_runs
    one = compose_runs([a])
    assert one.rank == a.rank and set(one.lora) == set(a.lora) and all(torch.equal(one.lora[k], a.lora[k]) for k in a.lora)
    assert [n for n, _ in one.tokens] == [n for n, _ in a.tokens] and one.shadowed == [] and one.unet_rank == 0
    # weight 0: the adapter is left out, the tokens stay
    c = compose_runs([a, b], [1.0, 0.0])
    assert c.rank == 4 and all(torch.equal(c.lora[k], a.lora[k]) for k in a.lora)
    assert [n for n, _ in c.tokens] == ["<dog>", "<hflip>", "<grayscale_0>", "<style>"]     # (a run's own order: its sorted file names)
    c = compose_runs([a, b], [0.0, 1.0])
    assert c.rank == 8 and all(torch.equal(c.lora[k], b.lora[k]) for k in b.lora)
    # --lora_rank 0: tokens only
    dz = str(tmp_path / "cat")
    write_run(dz, ["<cat>"], [], seed=3, rank=0)
    z = G.read_run_dir(dz)
    assert z.rank == 0 and z.lora == {}
    c = compose_runs([z, b])
    assert c.rank == 8 and all(torch.equal(c.lora[k], b.lora[k]) for k in b.lora)
    assert [n for n, _ in c.tokens] == ["<cat>", "<grayscale_0>", "<hflip>", "<style>"]
    c = compose_runs([z])
    assert c.rank == 0 and c.lora == {} and [n for n, _ in c.tokens] == ["<cat>"]


# ------------------------------------------------------------------------------------------------ oracle level
def test_oracle_encoder_with_the_composed_adapter_equals_the_merged_encoder(two_runs):
    """TextBoostEncoder(r = 12) carrying the composed adapter against a second oracle encoder (r = 0) whose q / k / v weights were merged
    here: the same function, summed in another order.  fp32 on the CPU, rel-L2 <= 1e-5."""
    from oracle.clip_text import CLIPTextCfg, TextBoostEncoder
    from textboost_amd.compose import compose_runs
    a, b = two_runs
    w = (1.0, 0.7)
    c = compose_runs([a, b], w)
    torch.manual_seed(0)
    ccfg = CLIPTextCfg.tiny(D_TEXT)
    base = TextBoostEncoder(ccfg, r=0)
    with torch.no_grad():
        for n, p in base.named_parameters():
            if "ln" in n or n.endswith("bias"):
                p.add_(torch.randn_like(p) * 0.1)
        base.token_embedding.weight.mul_(0.5)
        composed = TextBoostEncoder(ccfg, r=12)
        composed.load_state_dict(base.state_dict(), strict=False)
        merged = TextBoostEncoder(ccfg, r=0)
        merged.load_state_dict(base.state_dict())
        for i in range(LAYERS):
            for proj, mc, mm in zip(PROJ, (composed.layers[i].q, composed.layers[i].k, composed.layers[i].v),
                                    (merged.layers[i].q, merged.layers[i].k, merged.layers[i].v)):
                name = f"base_model.model.text_model.encoder.layers.{i}.self_attn.{proj}"
                mc.lora_A.copy_(c.lora[name + ".lora_A.weight"])
                mc.lora_B.copy_(c.lora[name + ".lora_B.weight"])
                assert mc.scaling == 1.0
                mm.weight.add_(merged_delta([(a, w[0]), (b, w[1])], name, torch.float32))
        ids = torch.randint(0, 49406, (4, 77), generator=torch.Generator().manual_seed(5))
        ids[:, 0] = 49406
        for row, n in enumerate((9, 23, 2, 77)):
            ids[row, n - 1:] = 49407
        out, ref, plain = composed(ids), merged(ids), base(ids)
    e = ((out - ref).norm() / ref.norm()).item()
    far = ((plain - ref).norm() / ref.norm()).item()
    print(f"[compose] oracle, composed adapter vs merged weights: rel-L2 {e:.2e} (<= 1e-5); base encoder vs merged: {far:.2e}")
    assert e <= 1e-5
    assert far > 1e-3               # the adapters matter on these inputs


# ------------------------------------------------------------------------------------------------ --mixing
def test_mixing_runs_are_disjoint_and_keep_their_rows_bit_for_bit(tmp_path):
    from textboost_amd import generate as G
    from textboost_amd.compose import adapter_support, compose_runs, disjoint
    da, db, dc = str(tmp_path / "dog"), str(tmp_path / "style"), str(tmp_path / "plain")
    write_run(da, ["<dog>"], [], seed=1, rank=4, keep_rows="even")
    write_run(db, ["<style>"], [], seed=2, rank=8, keep_rows="odd")
    write_run(dc, ["<can>"], [], seed=3, rank=4)
    write_run(str(tmp_path / "tok"), ["<cat>"], [], seed=4, rank=0)
    a, b, u, z = (G.read_run_dir(d) for d in (da, db, dc, str(tmp_path / "tok")))
    assert (adapter_support(a), adapter_support(b), adapter_support(u), adapter_support(z)) == ("even", "odd", "both", "none")
    assert disjoint([a, b]) and disjoint([b, a, z]) and disjoint([a])
    assert not disjoint([a, u]) and not disjoint([u]) and not disjoint([a, a])
    wa, wb = 1.0, 0.7
    c = compose_runs([a, b], [wa, wb])
    def chain(B, A):
        """B @ A in fp32 as one multiply-add chain over the rank per element, in index order: no library blocking, and a zero term adds nothing"""
        out = torch.zeros(B.shape[0], A.shape[1])
        for k in range(B.shape[1]):
            out = out + B[:, k:k + 1] * A[k:k + 1]
        return out

    for name in module_names():
        Ac, Bc = c.lora[name + ".lora_A.weight"], c.lora[name + ".lora_B.weight"]
        Ba, Bb = a.lora[name + ".lora_B.weight"] * torch.tensor(wa), b.lora[name + ".lora_B.weight"] * torch.tensor(wb)
        # row n of B_c is [w_a B_a[n] | w_b B_b[n]]: in an even row the second part is zero, in an odd row the first
        assert torch.equal(Bc[:, :4], Ba) and torch.equal(Bc[:, 4:], Bb) and not Bc[0::2, 4:].any() and not Bc[1::2, :4].any()
        delta, da_, db_ = chain(Bc, Ac), chain(Ba, a.lora[name + ".lora_A.weight"]), chain(Bb, b.lora[name + ".lora_A.weight"])
        assert torch.equal(delta[0::2], da_[0::2]) and torch.equal(delta[1::2], db_[1::2])
        assert da_[0::2].abs().max() > 0 and db_[1::2].abs().max() > 0 and not da_[1::2].any() and not db_[0::2].any()


# ------------------------------------------------------------------------------------------------ tokens
def test_token_union_order_and_shadowing(two_runs):
    from textboost_amd.compose import compose_runs
    a, b = two_runs
    c = compose_runs([a, b])
    assert [n for n, _ in c.tokens] == ["<dog>", "<hflip>", "<grayscale_0>", "<style>"]
    by_name = dict(c.tokens)
    assert torch.equal(by_name["<hflip>"], dict(a.tokens)["<hflip>"]) and not torch.equal(by_name["<hflip>"], dict(b.tokens)["<hflip>"])
    assert c.shadowed == [("<hflip>", b.path)]
    r = compose_runs([b, a])
    assert [n for n, _ in r.tokens] == ["<grayscale_0>", "<hflip>", "<style>", "<dog>"]      # a run's own order: sorted file names
    assert torch.equal(dict(r.tokens)["<hflip>"], dict(b.tokens)["<hflip>"]) and r.shadowed == [("<hflip>", a.path)]
    assert r.path == b.path and r.files == b.files


def test_trained_run_keeps_its_constructor():
    from textboost_amd.generate import TrainedRun
    t = TrainedRun(path="p", rank=0, lora={})
    assert (t.tokens, t.files, t.unet_rank, t.unet_lora, t.shadowed) == ([], [], 0, {}, [])
    t = TrainedRun(path="p", rank=0, lora={}, tokens=[("<a>", torch.zeros(4))], files=["a.bin"])
    assert t.unet_rank == 0 and t.shadowed == []


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(two_runs, tmp_path):
    from textboost_amd import generate as G
    from textboost_amd.compose import compose_runs
    a, b = two_runs
    with pytest.raises(ValueError, match="3 weights for 2 runs"):
        compose_runs([a, b], [1.0, 1.0, 1.0])
    with pytest.raises(ValueError, match="1 weights for 2 runs"):
        compose_runs([a, b], [1.0])
    write_run(str(tmp_path / "r60"), ["<x>"], [], seed=5, rank=60)
    big = G.read_run_dir(str(tmp_path / "r60"))
    with pytest.raises(NotImplementedError, match=r"8 \+ 60 = 68"):
        compose_runs([b, big])
    assert compose_runs([a, big]).rank == 64                         # the limit itself composes
    assert compose_runs([b, big], [0.0, 1.0]).rank == 60             # a weight of 0 does not count
    write_run(str(tmp_path / "wide"), ["<y>"], [], seed=6, rank=4, D=96)
    with pytest.raises(ValueError, match="hidden size"):
        compose_runs([a, G.read_run_dir(str(tmp_path / "wide"))])
    write_run(str(tmp_path / "deep"), ["<z>"], [], seed=7, rank=4, layers=3)
    with pytest.raises(ValueError, match="layers"):
        compose_runs([a, G.read_run_dir(str(tmp_path / "deep"))])
    fewer = G.TrainedRun(path="fewer", rank=4, lora={k: v for k, v in a.lora.items() if ".layers.0.self_attn.k_proj" not in k})
    with pytest.raises(ValueError, match="different modules"):
        compose_runs([a, fewer])
    write_run(str(tmp_path / "wtok"), ["<w>"], [], seed=8, rank=0, D=96)
    with pytest.raises(ValueError, match="width 96"):
        compose_runs([a, G.read_run_dir(str(tmp_path / "wtok"))])
    with pytest.raises(ValueError):
        compose_runs([])


# ------------------------------------------------------------------------------------------------ the reader of <run>/unet/
XATTN = [("down_blocks.0.attentions.0.transformer_blocks.0.attn2", 32), ("mid_block.attentions.0.transformer_blocks.0.attn2", 64),
         ("up_blocks.1.attentions.2.transformer_blocks.0.attn2", 32)]


def test_read_run_dir_reads_the_unet_adapters_back(tmp_path):
    import json
    from safetensors.torch import save_file
    from textboost_amd import checkpoint as ckpt
    from textboost_amd import generate as G
    from textboost_amd.compose import compose_runs
    d = str(tmp_path / "dog")
    write_run(d, ["<dog>"], [], seed=1, rank=4)
    assert G.read_run_dir(d).unet_rank == 0 and G.read_run_dir(d).unet_lora == {}
    unet = stub_kv_unet(XATTN, D_TEXT, 4, seed=2)
    ckpt.save_unet_adapters(unet, os.path.join(d, "unet"), "tiny")
    run = G.read_run_dir(d)
    want = ckpt.unet_lora_state_dict(unet)
    assert run.unet_rank == 4 and set(run.unet_lora) == set(want) and len(want) == 12
    assert all(torch.equal(run.unet_lora[k], want[k]) for k in want)
    assert run.rank == 4 and [n for n, _ in run.tokens] == ["<dog>"] and "unet" in run.files        # the rest as before
    # the in-model key layout of earlier files
    d2 = str(tmp_path / "cat")
    write_run(d2, ["<cat>"], [], seed=3, rank=4)
    other = stub_kv_unet(XATTN, D_TEXT, 2, seed=4)
    ckpt.save_unet_adapters(other, os.path.join(d2, "unet"), "tiny")
    save_file(ckpt.unet_lora_state_dict(other), os.path.join(d2, "unet", "adapter_model.safetensors"))
    run2 = G.read_run_dir(d2)
    assert run2.unet_rank == 2 and all(torch.equal(run2.unet_lora[k], v) for k, v in ckpt.unet_lora_state_dict(other).items())
    # composed: rank concatenation with the weights, in float64 against the weighted sum
    c = compose_runs([run, run2], [1.0, 0.5])
    assert c.unet_rank == 6 and set(c.unet_lora) == set(want)
    for ka in (k for k in want if ".lora_A." in k):
        kb = ka.replace(".lora_A.", ".lora_B.")
        got = c.unet_lora[kb].double() @ c.unet_lora[ka].double()
        ref = run.unet_lora[kb].double() @ run.unet_lora[ka].double() + 0.5 * (run2.unet_lora[kb].double() @ run2.unet_lora[ka].double())
        assert ((got - ref).norm() / ref.norm()).item() <= 1e-6
    only = compose_runs([run, run2], [1.0, 0.0])
    assert only.unet_rank == 4 and all(torch.equal(only.unet_lora[k], run.unet_lora[k]) for k in want)
    assert compose_runs([run]).unet_rank == 4
    # refusals by name
    cfg_path = os.path.join(d2, "unet", "adapter_config.json")
    cfg = json.load(open(cfg_path))
    for change, exc, match in (({"lora_alpha": 8}, NotImplementedError, "lora_alpha"), ({"target_modules": ["to_q"]}, NotImplementedError, "target_modules"),
                               ({"use_dora": True}, NotImplementedError, "use_dora"), ({"r": 3, "lora_alpha": 3}, ValueError, "rank-3")):
        with open(cfg_path, "w") as f:
            json.dump(dict(cfg, **change), f)
        with pytest.raises(exc, match=match):
            G.read_run_dir(d2)
    with open(cfg_path, "w") as f:
        json.dump(cfg, f)
    save_file({"something.else": torch.zeros(2, 2)}, os.path.join(d2, "unet", "adapter_model.safetensors"))
    with pytest.raises(ValueError, match="unrecognised UNet adapter layout"):
        G.read_run_dir(d2)


# ------------------------------------------------------------------------------------------------ inference.py --with / --weights
def test_parser_accepts_with_and_weights():
    import inference
    p = inference.build_parser()
    a = p.parse_args(["run"])
    assert a.with_runs is None and a.weights is None
    a = p.parse_args(["run", "--with", "style", "--weights", "1", "0.8", "--prompt", "x"])
    assert a.with_runs == ["style"] and a.weights == [1.0, 0.8] and a.path == "run"
    a = p.parse_args(["run", "--with", "s1", "s2/checkpoint-10", "--attn-map"])
    assert a.with_runs == ["s1", "s2/checkpoint-10"] and a.attn_map == []


def test_shadowed_token_and_wrong_weight_count_exit_before_the_device_is_consulted(tmp_path, monkeypatch, capsys):
    pytest.importorskip("transformers")
    import inference
    from tests.test_gpu_generate import _write_tokenizer
    mdir, da, db = str(tmp_path / "model"), str(tmp_path / "runs" / "dog"), str(tmp_path / "runs" / "style")
    _write_tokenizer(os.path.join(mdir, "tokenizer"))
    write_run(da, ["<dog>"], ["<hflip>"], seed=1, rank=4, keep_rows="even")
    write_run(db, ["<style>"], ["<hflip>"], seed=2, rank=8, keep_rows="odd")

    def consulted():
        raise AssertionError("torch.cuda was consulted")
    monkeypatch.setattr(torch.cuda, "is_available", consulted)
    common = [da, "--with", db, "--model", mdir]
    with pytest.raises(SystemExit) as e:
        inference.main(common + ["--prompt", "a <hflip> photo of a <dog> dog in <style> style"])
    assert "<hflip>" in str(e.value) and da in str(e.value) and db in str(e.value)
    with pytest.raises(SystemExit, match="<hflip>"):
        inference.main(common + ["--prompt", "a <dog> dog in <style> style", "--attn-map", "<hflip>"])
    with pytest.raises(SystemExit, match="3 weights for 2 runs"):
        inference.main(common + ["--prompt", "a <dog> dog", "--weights", "1", "1", "1"])
    with pytest.raises(SystemExit, match="2 weights for 1 runs"):
        inference.main([da, "--model", mdir, "--weights", "1", "1"])
    capsys.readouterr()
    # an unambiguous prompt passes the host checks and reaches the device question, after the report
    with pytest.raises(AssertionError, match="consulted"):
        inference.main(common + ["--prompt", "a <dog> dog in <style> style", "--weights", "1", "0.8", "--attn-map"])
    out = capsys.readouterr().out
    assert f"run {da}: rank 4, lora_B rows even, weight 1, UNet K/V adapters none" in out
    assert f"run {db}: rank 8, lora_B rows odd, weight 0.8, UNet K/V adapters none" in out
    assert "disjoint output features" in out
    # the placeholder tokens of all runs that occur in the prompt
    args = inference.build_parser().parse_args(common + ["--prompt", "a <dog> dog in <style> style", "--attn-map"])
    words, positions = inference.attn_map_words(mdir, inference.load_runs(args), args.prompt, [])
    assert words == ["<dog>", "<style>"] and [len(p) for p in positions] == [1, 1]
    # without --with nothing is printed and the run is the one read
    capsys.readouterr()
    one = inference.load_runs(inference.build_parser().parse_args([da, "--model", mdir]))
    assert capsys.readouterr().out == "" and one.rank == 4 and one.shadowed == []
