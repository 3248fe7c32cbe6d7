"""The in-process subject sweep (textboost_amd/sweep.py) on the GPU: three subjects trained on resident shared models give, bit for bit, what
`train_textboost.main` gives for each subject alone; the shared models are built once; nothing of a finished subject stays on the device; every
subject has its own log and the files the evaluation tools read.  Tiny model directory of tests.test_gpu_generate (16 x 16 latents)."""
import glob
import json
import os
import pickle
import signal
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

# initializer = "<initializer_token> <class_token>"; the tiny tokenizer has no merges, so a word of n letters is n pieces:
# s1 -> "a b": 2 vectors, s2 -> "ab b": 3 vectors, s3 -> "a dog": 4 vectors.  The trainable buffers change size from subject to subject.
SUBJECTS = [{"name": "s1", "class_token": "b", "initializer_token": "a"},
            {"name": "s2", "class_token": "b", "initializer_token": "ab"},
            {"name": "s3", "class_token": "dog", "initializer_token": "a"}]
STEPS = 10


def _prepare(root):
    """model directory (tests.test_gpu_generate.write_model_dir + the VAE's encoder half), one PNG per subject, the subjects file, edit prompts"""
    from PIL import Image
    from safetensors.torch import load_file, save_file
    from tests.test_gpu_generate import write_model_dir
    from textboost_amd import models
    from textboost_amd.vae import VAEGeometry, vae_encoder_shapes
    mdir = os.path.join(root, "model")
    write_model_dir(mdir)
    vpath = os.path.join(mdir, "vae", "diffusion_pytorch_model.safetensors")
    vsd = load_file(vpath)
    vgeo = VAEGeometry(block_out_channels=(64, 64, 128, 128), layers_per_block=1)
    vsd.update({k: v.half().float() for k, v in models.random_state_dict(vae_encoder_shapes(vgeo), 15, device="cpu").items()})
    save_file(vsd, vpath)
    with open(os.path.join(mdir, "tokenizer", "tokenizer_config.json"), "w") as f:   # as in a diffusers model directory: prompts are 77 tokens
        json.dump({"model_max_length": 77}, f)
    r = np.random.default_rng(0)
    for i, s in enumerate(SUBJECTS):
        d = os.path.join(root, "data", s["name"])
        os.makedirs(d)
        h, w = 150 + 20 * i, 170 - 10 * i
        yy, xx = np.mgrid[0:h, 0:w]
        a = np.clip(np.stack([xx * 255 // w, yy * 255 // h, (xx + yy + 40 * i) % 256], -1) + r.integers(-20, 21, (h, w, 3)), 0, 255)
        Image.fromarray(a.astype(np.uint8)).save(os.path.join(d, "00.png"))
    with open(os.path.join(root, "subjects.json"), "w") as f:
        json.dump(SUBJECTS, f)
    # the knowledge-preservation prompts come from the reference's hard-coded relative path (train_textboost.py:892)
    with open(os.path.join(root, "data", "human-written-prompts.jsonl"), "w") as f:
        f.write("\n".join(json.dumps({"input": f"make the {w} blue", "output": f"a blue {w}"}) for w in ("car", "house", "sky", "boat")) + "\n")
    return mdir


def _driver_argv(root, mdir, extra=()):
    return ["-m", "sd15", "--model-dir", mdir, "--subjects", os.path.join(root, "subjects.json"), "--data-dir", os.path.join(root, "data"),
            "--total-steps", str(STEPS), "--batch-size", "2", "--resolution", "128", "--seed", "7", *extra]


class _Counts:
    """counts the constructions of the frozen models through wrapped __init__s"""

    def __init__(self, mp):
        from textboost_amd.text_encoder import HipTextEncoder
        from textboost_amd.unet import HipUNet
        from textboost_amd.vae import HipVAEDecoder, HipVAEEncoder
        self.n = {"unet": 0, "vae_decoder": 0, "vae_encoder": 0, "frozen_text": 0, "student": 0}

        def wrap(cls, key):
            orig = cls.__init__

            def init(obj, *a, **k):
                if type(obj) is cls:
                    self.n[key(a, k)] += 1
                return orig(obj, *a, **k)
            mp.setattr(cls, "__init__", init)
        wrap(HipUNet, lambda a, k: "unet")
        wrap(HipVAEDecoder, lambda a, k: "vae_decoder")
        wrap(HipVAEEncoder, lambda a, k: "vae_encoder")
        wrap(HipTextEncoder, lambda a, k: "student" if k.get("lora_rank", 0) else "frozen_text")   # teacher + the null embedding's encoder


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """the sweep over three subjects, then every subject alone from the lines of its cmd.txt: computed once, read by every test"""
    pytest.importorskip("PIL")
    import train_textboost as T
    from textboost_amd import sweep
    root = str(tmp_path_factory.mktemp("sweep"))
    mdir = _prepare(root)
    cwd = os.getcwd()
    os.chdir(root)
    mp = pytest.MonkeyPatch()
    try:
        args = sweep.db_parser().parse_args(_driver_argv(root, mdir))
        outdir, jobs = sweep.build_db(args)
        counts = _Counts(mp)
        logs_after = {}
        results = sweep.sweep_in_process(jobs, lambda r: logs_after.setdefault(r["name"], {
            n: open(os.path.join(outdir, n, "training.log")).read() for n, _ in jobs if os.path.exists(os.path.join(outdir, n, "training.log"))}))
        sweep_counts = dict(counts.n)
        mp.undo()
        alone, alone_counts = {}, None
        for name, cmd in jobs:
            lines = open(os.path.join(outdir, name, "cmd.txt")).read().split("\n")
            assert lines == cmd
            out = os.path.join(root, "alone", name)
            argv = [f"--output_dir={out}" if t.startswith("--output_dir=") else t for t in lines[1:]]
            if alone_counts is None:
                c = _Counts(mp)
            T.main(T.parse_args(argv))
            if alone_counts is None:
                alone_counts = dict(c.n)
                mp.undo()
            alone[name] = out
    finally:
        mp.undo()
        os.chdir(cwd)
    return {"root": root, "mdir": mdir, "outdir": os.path.join(root, outdir), "jobs": jobs, "results": results, "logs_after": logs_after,
            "sweep_counts": sweep_counts, "alone_counts": alone_counts, "alone": alone}


def _files(d):
    return sorted(os.path.relpath(os.path.join(p, f), d) for p, _, fs in os.walk(d) for f in fs)


def _assert_equal(a, b, where):
    if isinstance(a, torch.Tensor):
        assert a.dtype == b.dtype and a.shape == b.shape, where
        torch.testing.assert_close(a, b, atol=0, rtol=0, equal_nan=True, msg=lambda m: f"{where}: {m}")
    elif isinstance(a, np.ndarray):
        assert np.array_equal(a, b), where
    elif isinstance(a, dict):
        assert list(a) == list(b), where
        for k in a:
            _assert_equal(a[k], b[k], f"{where}[{k!r}]")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            _assert_equal(x, y, f"{where}[{i}]")
    else:
        assert a == b, where


def _load(path):
    from safetensors.torch import load_file
    if path.endswith(".safetensors"):
        return load_file(path)
    if path.endswith((".bin", ".pt")):
        return torch.load(path, map_location="cpu", weights_only=False)
    if path.endswith(".pkl"):
        with open(path, "rb") as f:
            return pickle.load(f)
    return None


def test_state_does_not_leak_between_subjects(runs):
    """every tensor a subject of the sweep wrote equals what the subject alone writes: adapter, token files, every checkpoint (optimizer moments,
    scaler, scheduler, generator states).  Subjects 2 and 3 start on models a subject has already trained on."""
    assert [r["status"] for r in runs["results"]] == ["ok"] * 3, runs["results"]
    n_vectors = []
    for s in SUBJECTS:
        got, want = os.path.join(runs["outdir"], s["name"]), runs["alone"][s["name"]]
        skip = {"cmd.txt", "train_textboost.py"}   # written by the driver, not by the trainer
        assert [f for f in _files(got) if f not in skip] == _files(want)
        compared = 0
        for f in _files(want):
            a, b = _load(os.path.join(got, f)), _load(os.path.join(want, f))
            if a is not None:
                _assert_equal(a, b, f"{s['name']}/{f}")
                compared += 1
        assert compared >= 3 + 5 * 5, compared   # adapter + >= 2 token files; per checkpoint model, optimizer, scheduler, scaler, generators
        assert os.path.exists(os.path.join(got, "text_encoder", "adapter_model.safetensors"))
        assert len(glob.glob(os.path.join(got, "checkpoint-*"))) == 5
        n_vectors.append(len(glob.glob(os.path.join(got, f"{s['name']}*.bin"))))
    assert n_vectors == [2, 3, 4]   # the placeholder's vector count, hence the trainable buffers' sizes, differs between the subjects


def test_shared_models_are_built_once(runs):
    """three subjects construct the UNets, the VAE halves and the frozen text encoders as often as one `main` does, and one student each"""
    one, three = runs["alone_counts"], runs["sweep_counts"]
    assert one == {"unet": 2, "vae_decoder": 1, "vae_encoder": 1, "frozen_text": 2, "student": 1}
    assert three == dict(one, student=3)


def test_no_device_memory_growth_per_subject(runs):
    r = runs["results"]
    assert r[1]["device_bytes"] == r[2]["device_bytes"] > 0


def test_logs_and_files_are_per_subject(runs):
    out, names = runs["outdir"], [s["name"] for s in SUBJECTS]
    final = {n: open(os.path.join(out, n, "training.log")).read() for n in names}
    # nothing was appended to a subject's log after it had finished, and no later subject's log existed yet
    for i, n in enumerate(names):
        assert runs["logs_after"][n] == {m: final[m] for m in names[:i + 1]}
    for n in names:
        assert f"<{n}_0>" in final[n] and "Training took" in final[n] and final[n].count("mean_norm") == 1
        assert not any(f"<{m}_0>" in final[n] for m in names if m != n)
        assert os.path.exists(os.path.join(out, n, "cmd.txt"))
        assert open(os.path.join(out, n, "train_textboost.py")).read() == open(os.path.join(ROOT, "train_textboost.py")).read()
        for k in range(2, STEPS + 1, 2):
            assert os.path.getsize(os.path.join(out, n, f"validation_{k}.jpg")) > 0
    # a log of the sweep reads like the log of the subject alone: the same messages in the same order
    for n in names:
        alone = open(os.path.join(runs["alone"][n], "training.log")).read()
        msg = lambda text: [ln.split(" - ", 3)[-1] for ln in text.splitlines() if "Training took" not in ln]   # noqa: E731
        assert msg(final[n]) == msg(alone)


def test_evaluation_tools_accept_the_subject_directories(runs):
    from textboost_amd import generate
    base = generate.load_base_text(runs["mdir"], "cuda")
    for s, want in zip(SUBJECTS, (2, 3, 4)):
        run = generate.read_run_dir(os.path.join(runs["outdir"], s["name"]))
        assert run.rank == 4 and sum(n.startswith(f"<{s['name']}") for n, _ in run.tokens) == want
        te, tok = generate.load_text_encoder(runs["mdir"], run, 1, base=base)
        assert tok.convert_tokens_to_ids(f"<{s['name']}_0>") >= 49408


def test_fresh_process_writes_the_same_file_set(runs):
    """--fresh-process: one subject through a child `python run_textboost_db.py ... --fresh-process`, which starts `python train_textboost.py`"""
    root = os.path.join(runs["root"], "fresh")
    os.makedirs(root)
    argv = _driver_argv(runs["root"], runs["mdir"], ["--instances", "s2", "--fresh-process"])
    # a session of its own: on a timeout the driver AND the trainer it started are ended, nothing is left on the GPU
    p = subprocess.Popen([sys.executable, os.path.join(ROOT, "run_textboost_db.py"), *argv], cwd=root, stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, text=True, start_new_session=True)
    try:
        stdout, stderr = p.communicate(timeout=300)
    except subprocess.TimeoutExpired:
        os.killpg(p.pid, signal.SIGKILL)
        p.communicate()
        raise
    assert p.returncode == 0, stdout[-2000:] + stderr[-2000:]
    assert "1 of 1 subjects trained" in stdout
    assert _files(os.path.join(root, "output", "tb-sd15-n1", "s2")) == _files(os.path.join(runs["outdir"], "s2"))
