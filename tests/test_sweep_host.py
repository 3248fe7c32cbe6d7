"""Subject sweep drivers (run_textboost_db.py / run_textboost_sdrp.py, textboost_amd/sweep.py): the per-subject command lines against what the
reference's drivers start (tests/golden/sweep_commands.json, recorded by tests/golden/gen_sweep_commands.py), the failure policy, the launch line
for several GPUs, and the split of train_textboost.main into setup_shared / train_subject.  No GPU."""
import json
import os
import sys
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from textboost_amd import sweep  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
with open(os.path.join(GOLDEN, "sweep_commands.json")) as _f:
    CASES = {c["name"]: c for c in json.load(_f)["cases"]}
MODEL_TOKEN = "--pretrained_model_name_or_path="


def build(case, model_dir):
    parser, builder = (sweep.db_parser(), sweep.build_db) if case["driver"] == "db" else (sweep.sdrp_parser(), sweep.build_sdrp)
    args = parser.parse_args(case["flags"] + ["--model-dir", model_dir])
    return args, builder(args)


@pytest.mark.parametrize("name", sorted(CASES))
def test_argv_output_directory_and_cmd_txt_equal_the_references(name, tmp_path, monkeypatch):
    case = CASES[name]
    model_dir = str(tmp_path / "model")
    args, (outdir, jobs) = build(case, model_dir)
    assert outdir in case["directories_made"]                       # os.makedirs(outdir) of the reference
    assert len(jobs) == len(case["subjects"]) > 0
    monkeypatch.chdir(tmp_path)
    for (subject, cmd), want in zip(jobs, case["subjects"]):
        assert cmd[0] == want["cmd"][0] == "train_textboost.py"
        differ = [(a, b) for a, b in zip(cmd[1:], want["cmd"][1:]) if a != b]
        assert len(cmd) == len(want["cmd"]) and len(differ) == 1, (subject, differ)
        assert differ[0][0] == MODEL_TOKEN + model_dir and differ[0][1].startswith(MODEL_TOKEN)
        # cmd.txt: the same path, the same text but for that one line; and the copy of train_textboost.py beside it
        sweep.write_records(cmd)
        assert os.path.normpath(want["cmd_txt_path"]) == os.path.normpath(os.path.join(outdir, subject, "cmd.txt"))
        got = open(want["cmd_txt_path"]).read().split("\n")
        ref = want["cmd_txt"].split("\n")
        assert len(got) == len(ref) and [(a, b) for a, b in zip(got, ref) if a != b] == [differ[0]]
        if want["copy"] is not None:
            assert open(want["copy"][1]).read() == open(os.path.join(ROOT, "train_textboost.py")).read()
    # the launcher: the reference's process count is the number of GPUs named by -g, which it exports
    assert want["launcher"][-1] == f"--nproc-per-node={len(args.gpu.split(','))}" and case["cuda_visible_devices"] == args.gpu


def test_default_subject_tables_are_the_recorded_ones():
    db = sweep.load_subjects(sweep.SUBJECTS_DB, ("name", "class_token", "initializer_token"), None)
    assert [f"--placeholder_token=<{s['name']}>" for s in db] == [next(t for t in w["cmd"] if t.startswith("--placeholder_token="))
                                                                  for w in CASES["db_defaults"]["subjects"]]
    sd = sweep.load_subjects(sweep.SUBJECTS_SDRP, ("name", "template", "initializer_token"), None)
    assert [f"--template={s['template']}" for s in sd] == [next(t for t in w["cmd"] if t.startswith("--template="))
                                                           for w in CASES["sdrp_defaults"]["subjects"]]


def test_instances_filter_in_table_order(tmp_path):
    args = sweep.db_parser().parse_args(["--instances", "dog", "cat2", "backpack", "--model-dir", str(tmp_path)])
    _, jobs = sweep.build_db(args)
    assert [n for n, _ in jobs] == ["backpack", "cat2", "dog"]
    _, jobs = build(CASES["db_instances"], str(tmp_path))[1]
    assert [n for n, _ in jobs] == ["cat2", "dog"]


@pytest.mark.parametrize("model_dir", ["sd15", "stabilityai/stable-diffusion-2-1"])
def test_hub_id_as_model_dir_is_refused(model_dir, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    with pytest.raises(SystemExit) as e:
        sweep.main_db(["-m", "sd15", "--model-dir", model_dir])
    assert "--model-dir" in str(e.value) and "local diffusers model directory" in str(e.value)
    assert not os.path.exists(tmp_path / "output")
    with pytest.raises(SystemExit):
        sweep.main_db(["-m", "sd15"])   # --model-dir is required


def _data(tmp_path, names):
    from PIL import Image
    for n in names:
        os.makedirs(tmp_path / "data" / n)
        Image.new("RGB", (8, 8), (200, 10, 10)).save(str(tmp_path / "data" / n / "00.png"))
    return str(tmp_path / "data")


def test_multi_gpu_launch_line(tmp_path, monkeypatch):
    """-g 0,1: ONE torch.distributed.run of the sweep worker, two processes, per-GPU batch 4 in every subject's argv"""
    pytest.importorskip("PIL")
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("CUDA_VISIBLE_DEVICES", "")
    model = tmp_path / "model"
    model.mkdir()
    data = _data(tmp_path, ["dog", "cat2"])
    calls = []

    def run(cmd, env=None):
        jobs = json.load(open(cmd[-1]))
        calls.append((cmd, env, jobs))
        return types.SimpleNamespace(returncode=0)
    args = sweep.db_parser().parse_args(["-g", "0,1", "--batch-size", "8", "--instances", "dog", "cat2", "--model-dir", str(model), "--data-dir", data])
    outdir, jobs = sweep.build_db(args)
    assert sweep.run_sweep(outdir, jobs, args.gpu, False, run=run) == 0
    assert len(calls) == 1
    cmd, env, sent = calls[0]
    assert cmd[0] == sys.executable and cmd[1:3] == ["-m", "torch.distributed.run"] and "--nproc-per-node=2" in cmd
    assert cmd[cmd.index("textboost_amd.sweep") - 1] == "-m" and cmd[-2] == "--worker"
    assert [n for n, _ in sent] == ["cat2", "dog"] and all("--train_batch_size=4" in c for _, c in sent)
    assert os.environ["CUDA_VISIBLE_DEVICES"] == "0,1" and env["PYTHONPATH"].split(os.pathsep)[0] == ROOT
    assert os.path.exists(os.path.join(outdir, "dog", "cmd.txt"))
    # --fresh-process on two GPUs: the reference's form, one launch per subject
    calls.clear()

    def run1(cmd, env=None):
        calls.append(cmd)
        return types.SimpleNamespace(returncode=0)
    assert sweep.run_sweep(outdir, jobs, args.gpu, True, run=run1) == 0
    assert len(calls) == 2 and all("--nproc-per-node=2" in c and c[c.index(sweep.TRAIN_SCRIPT) + 1:] == j[1][1:] for c, j in zip(calls, jobs))


def test_subject_without_data_is_skipped_and_reported(tmp_path, monkeypatch, capsys):
    pytest.importorskip("PIL")
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("CUDA_VISIBLE_DEVICES", "")
    model = tmp_path / "model"
    model.mkdir()
    data = _data(tmp_path, ["dog"])
    os.makedirs(os.path.join(data, "cat2"))   # a directory without images
    started = []

    def run(cmd, env=None):
        started.append(cmd)
        return types.SimpleNamespace(returncode=0)
    args = sweep.db_parser().parse_args(["--instances", "backpack", "cat2", "dog", "--model-dir", str(model), "--data-dir", data, "--fresh-process"])
    outdir, jobs = sweep.build_db(args)
    assert sweep.run_sweep(outdir, jobs, args.gpu, True, run=run) == 1
    assert len(started) == 1 and f"--instance_data_dir={os.path.join(data, 'dog')}" in started[0]
    out = capsys.readouterr().out
    assert "1 of 3 subjects trained" in out and "skipped: backpack: no data directory" in out and "skipped: cat2: no images" in out
    # the in-process sweep decides the same way, before the trainer is even imported for that subject
    assert sweep.cannot_start(jobs[0][1]).startswith("no data directory") and sweep.cannot_start(jobs[2][1]) is None


@pytest.mark.parametrize("status, launched", [(1, 1), (-6, 1), (134, 1), (3, 3)])
def test_fresh_process_stops_at_the_first_child_that_did_not_fail_on_its_inputs(tmp_path, monkeypatch, capsys, status, launched):
    """--fresh-process: a child that ends with anything but 0 or the trainer's input-error status (a HIP runtime error is a RuntimeError, exit
    status 1; torch.distributed.run reports an aborted rank as 1 too) ends the sweep: no later subject is started on that device"""
    pytest.importorskip("PIL")
    import train_textboost as T
    assert sweep.INPUT_ERROR_STATUS == T.INPUT_ERROR_STATUS == 3
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("CUDA_VISIBLE_DEVICES", "")
    model = tmp_path / "model"
    model.mkdir()
    data = _data(tmp_path, ["backpack", "cat2", "dog"])
    started = []

    def run(cmd, env=None):
        started.append(cmd)
        return types.SimpleNamespace(returncode=status if len(started) == 1 else 0)
    args = sweep.db_parser().parse_args(["--instances", "backpack", "cat2", "dog", "--model-dir", str(model), "--data-dir", data, "--fresh-process"])
    outdir, jobs = sweep.build_db(args)
    assert sweep.run_sweep(outdir, jobs, args.gpu, True, run=run) == 1
    assert len(started) == launched
    out = capsys.readouterr().out
    assert f"failed: backpack: exit status {status}" in out and f"{launched - 1} of 3 subjects trained" in out
    assert ("not started: dog: the sweep ended at backpack" in out) == (launched == 1)


def test_in_process_sweep_goes_on_after_an_input_error_and_stops_at_a_runtime_error(tmp_path, monkeypatch):
    """the policy of sweep_in_process on a stand-in trainer: ValueError (an unknown initializer) -> reported, next subject; RuntimeError (what the
    HIP runtime and the kernel library raise) -> the sweep ends, nothing more is started"""
    pytest.importorskip("PIL")
    import train_textboost as T
    monkeypatch.chdir(tmp_path)
    model = tmp_path / "model"
    model.mkdir()
    data = _data(tmp_path, ["backpack", "cat2", "dog"])
    args = sweep.db_parser().parse_args(["--instances", "backpack", "cat2", "dog", "--model-dir", str(model), "--data-dir", data])
    _, jobs = sweep.build_db(args)
    seen = []

    def fake_train(error):
        def train_subject(ctx, a, final=True):
            seen.append((a.placeholder_token, final))
            if a.placeholder_token == "<cat2>":
                raise error
            return {"total": 0.0}
        return train_subject
    monkeypatch.setattr(T, "setup_shared", lambda a: seen.append("setup") or object())
    monkeypatch.setattr(T, "train_subject", fake_train(ValueError("unknown initializer")))
    res = sweep.sweep_in_process(jobs)
    assert seen == ["setup", ("<backpack>", False), ("<cat2>", False), ("<dog>", True)]
    assert [r["status"] for r in res] == ["ok", "failed", "ok"] and "unknown initializer" in res[1]["reason"] and sweep.summarize(res) == 1
    seen.clear()
    monkeypatch.setattr(T, "train_subject", fake_train(RuntimeError("HIP error: an illegal memory access was encountered")))
    with pytest.raises(RuntimeError):
        sweep.sweep_in_process(jobs)
    assert seen == ["setup", ("<backpack>", False), ("<cat2>", False)]


def test_main_is_setup_shared_then_train_subject(monkeypatch):
    import train_textboost as T
    assert callable(T.setup_shared) and callable(T.train_subject)
    calls = []
    ctx = object()
    monkeypatch.setattr(T, "setup_shared", lambda a: calls.append(("setup_shared", a)) or ctx)
    monkeypatch.setattr(T, "train_subject", lambda c, a, *rest, **kw: calls.append(("train_subject", c, a, rest, kw)))
    args = object()
    T.main(args)
    assert calls == [("setup_shared", args), ("train_subject", ctx, args, (), {})]
