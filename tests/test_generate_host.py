"""CPU tests of image generation's host side (textboost_amd/generate.py, eval_dreambooth.py, inference.py): the reference's identifiers, prompts
and file names (tests/golden/eval_generate_names.json, recorded from the reference's own `generate()` by tests/golden/gen_eval_generate_names.py),
the reader of the output layout checkpoint.py writes, the CLI's refusals and subject selection, and the seeded latent."""
import json
import os
import types

import pytest
import torch

from textboost_amd import checkpoint as ckpt
from textboost_amd import generate as G


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "eval_generate_names.json")) as f:
        return json.load(f)


def _flag(argv, name, default=None):
    return argv[argv.index(name) + 1] if name in argv else default


def _seeds(argv):
    i = argv.index("--seeds") + 1
    out = []
    while i < len(argv) and not argv[i].startswith("--"):
        out.append(int(argv[i]))
        i += 1
    return out


def test_subject_table_and_live_split_follow_the_reference(golden):
    instances, obj, live = G.load_eval_prompts()
    assert instances == golden["instances"] and list(instances) == list(golden["instances"]) and len(instances) == 30
    assert len(obj) == 25 and len(live) == 25
    for name, is_live in golden["live"].items():
        assert G.is_live(name) == is_live
        assert G.prompt_templates(name) is not None and (G.prompt_templates(name) == live) == is_live
    assert sorted(k for k, v in golden["live"].items() if v) == ["cat", "cat2", "dog", "dog2", "dog3", "dog5", "dog6", "dog7", "dog8"]
    with pytest.raises(ValueError, match="Invalid instance"):
        G.prompt_templates("unicorn")


def test_identifier_prompts_and_paths_equal_the_recorded_reference_calls(golden):
    import eval_dreambooth as E
    assert len(golden["cases"]) >= 4
    for case in golden["cases"]:
        argv = case["argv"]
        args = E.build_parser().parse_args([a.replace("<tmp>", "/t") for a in argv] + ["--skip-gen"])
        assert os.path.relpath(E.image_root(args), "/t") == case["image_root"], case["name"]
        token_format = _flag(argv, "--token-format", "<INSTANCE> SUBJECT")
        checkpoint = _flag(argv, "--checkpoint")
        selected = [i for i in G.load_eval_prompts()[0] if i in case["instances"]]     # the subject table's order
        model_paths = [os.path.relpath(G.model_path_of("/t/runs/tb-sd15-n1", i, int(checkpoint) if checkpoint else None), "/t").rstrip("/")
                       for i in selected]
        assert model_paths == case["model_paths"], case["name"]
        prompts, saved = [], []
        for inst in selected:
            files = case["files"][inst] + ["text_encoder"]
            ident = G.identifier_for(token_format, inst, files)
            for seed in _seeds(argv):
                ps = G.instance_prompts(inst, ident)
                prompts += ps
                saved += [os.path.join(case["image_root"], f"seed{seed}", inst, G.image_filename(p, ident, inst)) for p in ps]
        ref_prompts = [p for call in case["calls"] for p in call["prompts"]]
        assert prompts == ref_prompts, case["name"]
        assert saved == case["saved"], case["name"]
        for call in case["calls"]:      # the protocol the executors reproduce: 25 steps, guidance 7.5, one latent for all prompts, <= 16 per call
            assert call["num_inference_steps"] == 25 and call["guidance_scale"] == 7.5 and call["latent_rows_equal"]
            assert call["latents_shape"][1:] == [4, 64, 64] and len(call["prompts"]) <= 16


def test_prompt_batches_are_even_ordered_and_bounded():
    p = [str(i) for i in range(25)]
    assert [len(b) for b in G.prompt_batches(p, 16)] == [13, 12]
    assert [len(b) for b in G.prompt_batches(p, 8)] == [7, 6, 6, 6]
    assert [len(b) for b in G.prompt_batches(p, 25)] == [25] and [len(b) for b in G.prompt_batches(p, 100)] == [25]
    for n in (1, 5, 8, 16):
        b = G.prompt_batches(p, n)
        assert [x for c in b for x in c] == p and max(len(c) for c in b) <= n


def _stub_encoder(D=16, L=2, r=4, V=20, seed=0):
    g = torch.Generator().manual_seed(seed)
    return types.SimpleNamespace(geo=types.SimpleNamespace(hidden_size=D, num_layers=L), r=r, lora_A=torch.randn(L, 3 * r, D, generator=g),
                                 lora_B=torch.randn(L, 3 * D, r, generator=g), token_table=torch.randn(V, D, generator=g))


def _write_run(d, te, added, aug):
    ckpt.save_text_encoder_adapter(te, os.path.join(d, "text_encoder"), "some/base")
    ckpt.save_token_embeddings(te, d, added, aug)


def test_read_run_dir_returns_what_checkpoint_py_wrote(tmp_path):
    te = _stub_encoder()
    d = str(tmp_path / "dog")
    _write_run(d, te, {"<dog_0>": 12, "<dog_1>": 13}, {"<hflip>": 15, "<crop>": 14})
    torch.save({"m": torch.zeros(3)}, os.path.join(d, "optimizer.bin"))
    torch.save({"last_epoch": 1.0, "x": 2.0}, os.path.join(d, "scheduler.bin"))
    torch.save({"<many>": te.token_table[3:6].clone()}, os.path.join(d, "many.bin"))     # an [n, D] tensor: tok, tok_1, tok_2
    run = G.read_run_dir(d)
    assert run.rank == 4
    want = ckpt.lora_state_dict(te)
    assert set(run.lora) == set(want) and all(torch.equal(run.lora[k], want[k]) for k in want)
    # sorted FILE order: crop.bin, dog_0.bin, dog_1.bin, hflip.bin, many.bin; [D] (placeholder) and [1, D] (augmentation) are one vector each
    assert [n for n, _ in run.tokens] == ["<crop>", "<dog_0>", "<dog_1>", "<hflip>", "<many>", "<many>_1", "<many>_2"]
    rows = [14, 12, 13, 15, 3, 4, 5]
    for (n, v), row in zip(run.tokens, rows):
        assert v.shape == (16,) and torch.equal(v, te.token_table[row]), n
    assert torch.load(os.path.join(d, "dog_0.bin"))["<dog_0>"].dim() == 1 and torch.load(os.path.join(d, "hflip.bin"))["<hflip>"].dim() == 2
    assert "optimizer.bin" in run.files and G.identifier_for("<INSTANCE> SUBJECT", "dog", run.files) == "<dog_0> dog <dog_1> dog"
    # a restored adapter is the saved one
    te2 = _stub_encoder(seed=1)
    ckpt.load_lora_state_dict(te2, run.lora)
    assert torch.equal(te2.lora_A, te.lora_A) and torch.equal(te2.lora_B, te.lora_B)


def test_read_run_dir_refuses_what_the_encoder_cannot_apply(tmp_path):
    te = _stub_encoder()

    def fresh(name, **cfg):
        d = str(tmp_path / name)
        _write_run(d, te, {"<dog>": 12}, None)
        if cfg:
            p = os.path.join(d, "text_encoder", "adapter_config.json")
            c = json.load(open(p))
            c.update(cfg)
            json.dump(c, open(p, "w"))
        return d
    G.read_run_dir(fresh("ok"))
    with pytest.raises(NotImplementedError, match="lora_alpha"):
        G.read_run_dir(fresh("alpha", lora_alpha=8))
    with pytest.raises(NotImplementedError, match="target_modules"):
        G.read_run_dir(fresh("targets", target_modules=["q_proj", "k_proj", "v_proj", "out_proj"]))
    with pytest.raises(NotImplementedError, match="target_modules"):
        G.read_run_dir(fresh("targets2", target_modules=["q_proj", "v_proj"]))
    with pytest.raises(NotImplementedError, match="use_dora"):
        G.read_run_dir(fresh("dora", use_dora=True))
    with pytest.raises(NotImplementedError, match="use_rslora"):
        G.read_run_dir(fresh("rslora", use_rslora=True))
    d = fresh("width")
    torch.save({"<wide>": torch.zeros(24)}, os.path.join(d, "wide.bin"))
    with pytest.raises(ValueError, match="width 24.*hidden_size is 16"):
        G.read_run_dir(d)
    with pytest.raises(ValueError, match="hidden_size is 32"):
        G.read_run_dir(fresh("width2"), hidden_size=32)
    os.makedirs(tmp_path / "empty")
    with pytest.raises(FileNotFoundError, match="text_encoder"):
        G.read_run_dir(str(tmp_path / "empty"))


def _eval_args(tmp_path, *extra):
    import eval_dreambooth as E
    return E.build_parser().parse_args([str(tmp_path / "runs" / "tb-sd15-n1"), "--outdir", str(tmp_path / "bench"), "--metric", "clip-t",
                                        "--clip-model", str(tmp_path), *extra])


def test_cli_refusals_and_subject_selection(tmp_path):
    import eval_dreambooth as E
    import inference as I
    with pytest.raises(SystemExit) as e:
        E.check_args(_eval_args(tmp_path))
    assert "--model DIR" in str(e.value) and "--skip-gen" in str(e.value)
    for alias in ("sd14", "sd15", "sd21base", "sd21"):
        with pytest.raises(SystemExit, match="hub repository"):
            E.check_args(_eval_args(tmp_path, "--model", alias))
    with pytest.raises(SystemExit, match="not a directory"):
        E.check_args(_eval_args(tmp_path, "--model", str(tmp_path / "nowhere")))
    E.check_args(_eval_args(tmp_path, "--model", str(tmp_path)))                 # a directory passes the argument check
    E.check_args(_eval_args(tmp_path, "--skip-gen", "--model", "sd15"))          # --skip-gen never looks at --model, as before
    with pytest.raises(SystemExit, match="vqa is not built"):
        E.check_args(_eval_args(tmp_path, "--model", str(tmp_path), "--metric", "vqa"))
    with pytest.raises(SystemExit, match="hub repository"):
        I.main([str(tmp_path), "--model", "sd21base"])
    with pytest.raises(SystemExit, match="--model DIR"):
        I.main([str(tmp_path)])
    # subjects: --instances in the table's order; else the sub-directories that are subjects; none -> exit
    run = tmp_path / "runs" / "tb-sd15-n1"
    with pytest.raises(SystemExit, match="no trained subject"):
        os.makedirs(run)
        G.select_instances(str(run), None)
    for name in ("teapot", "dog", "logs", "can"):
        os.makedirs(run / name)
    (run / "vase").write_text("a file, not a directory")
    assert G.select_instances(str(run), None) == ["can", "dog", "teapot"]
    assert G.select_instances(str(run), ["dog", "backpack"]) == ["backpack", "dog"]
    with pytest.raises(SystemExit, match="unicorn"):
        G.select_instances(str(run), ["unicorn"])
    with pytest.raises(SystemExit, match="eval_dreambooth.py: .*no trained subject"):
        E.generate(_eval_args(tmp_path / "other", "--model", str(tmp_path)))


def test_seeded_latent_is_the_cpu_expression_and_repeats():
    for seed, size in ((0, 64), (3, 96), (12345, 16)):
        a, b = G.seeded_latent(seed, size), G.seeded_latent(seed, size)
        want = torch.randn(1, 4, size, size, generator=torch.Generator().manual_seed(seed)).half().float()
        assert a.device.type == "cpu" and a.dtype == torch.float32 and a.shape == (1, 4, size, size)
        assert torch.equal(a, b) and torch.equal(a, want)
    assert not torch.equal(G.seeded_latent(0, 64), G.seeded_latent(1, 64))
