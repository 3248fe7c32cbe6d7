"""Subject sweeps: `run_textboost_db.py` (DreamBooth, 30 subjects) and `run_textboost_sdrp.py` (StyleDrop, 19 styles) of the reference.

The reference's drivers start one `torchrun train_textboost.py <argv>` per subject, so every subject reads and packs the UNet twice (training and
validation sampler), the VAE and the teacher again.  Here the per-subject argv is built exactly as the reference builds it (only the
`--pretrained_model_name_or_path=` token differs: it is a local directory), and by default the subjects train IN ONE PROCESS:
`train_textboost.setup_shared` once, then `train_textboost.train_subject` per subject with `parse_args(<that subject's argv>)`.  `<outdir>/<name>/
cmd.txt` therefore holds what reproduces the subject alone.  `--fresh-process` keeps the reference's form, a child `python train_textboost.py
<argv>` per subject.  With several GPUs one `python -m torch.distributed.run` starts this module as the sweep worker on every rank.

A subject that cannot start (no data directory, no images, an initializer the tokenizer does not know) is logged and the sweep goes on, as the
reference's unchecked `subprocess.run` does; the driver then exits non-zero and names it.  Any other error, first of all one raised by the HIP
runtime or the kernel library, ends the sweep at once: nothing more is started on a device that has faulted."""
from __future__ import annotations

import argparse
import gc
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time
from typing import Callable, List, Optional, Sequence, Tuple

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_HERE)
TRAIN_SCRIPT = os.path.join(ROOT, "train_textboost.py")
GOLDEN = os.path.join(ROOT, "tests", "golden")
SUBJECTS_DB = os.path.join(GOLDEN, "sweep_subjects_db.json")
SUBJECTS_SDRP = os.path.join(GOLDEN, "sweep_subjects_sdrp.json")
RESOLUTION = {"sd14": 512, "sd15": 512, "sd21base": 512, "sd21": 768}   # image side the named model was trained at
# errors of a subject's inputs: the subject is reported and the sweep goes on.  Everything else (RuntimeError is what torch's HIP runtime and
# textboost_amd._lib raise) ends the sweep.
INPUT_ERRORS = (FileNotFoundError, ValueError, NotImplementedError)
INPUT_ERROR_STATUS = 3   # exit status of `python train_textboost.py` for one of them (train_textboost.INPUT_ERROR_STATUS)

Job = Tuple[str, List[str]]   # (subject name, ["train_textboost.py", flag, ...])

_DEVIATIONS = """
differences from the reference's driver:
  --model-dir DIR   (required) the weights come from this local diffusers model directory; -m only names the run and selects the resolution.
                    Nothing is downloaded: a hub id is refused.  It is the only token of the per-subject argv that differs from the reference's.
  --subjects FILE   the subject table, a JSON list, instead of a table in the program (default: the reference's table)
  --data-dir DIR    where the subjects' image directories are (default: the reference's path)
  --fresh-process   one child `python train_textboost.py <argv>` per subject, as the reference does; default: every subject in this process on
                    models that stay on the device
  --resolution N / --seed N   passed on to every subject when given
  --mask-root DIR   every subject gains --instance_mask_dir=DIR/<subject> (the masked loss); without it the argv is the reference's
  --attn-loss-weight W   every subject gains --attn_loss_weight=W (the localisation loss, with --mask-root; run_textboost_db.py only: the
                    StyleDrop sweep is fp32 and refuses it); without it nothing is added
  -g 0,1,...        several GPUs: one `python -m torch.distributed.run` of the sweep worker, every rank walks the same subjects
  exit status       non-zero when a subject failed; the failed subjects are listed at the end
"""


def _common_flags(p: argparse.ArgumentParser, subjects: str, data_dir: str):
    p.add_argument("--model-dir", type=str, required=True, help="local diffusers model directory (unet/, vae/, text_encoder/, tokenizer/, scheduler/)")
    p.add_argument("--subjects", type=str, default=subjects, help="JSON list of subjects (default: %(default)s)")
    p.add_argument("--data-dir", type=str, default=data_dir, help="directory of the subjects' image directories (default: %(default)s)")
    p.add_argument("--fresh-process", action="store_true", default=False, help="one child process per subject (the reference's form)")
    p.add_argument("--resolution", type=int, default=None, help="image side for every subject (default: by -m)")
    p.add_argument("--seed", type=int, default=None, help="--seed of every subject (default: train_textboost.py's own)")
    p.add_argument("--mask-root", type=str, default=None, help="directory of the subjects' mask directories: every subject trains with "
                   "--instance_mask_dir=DIR/<subject> (the masked loss; default: no masks, the reference's command line)")
    p.add_argument("--attn-loss-weight", type=float, default=None, help="--attn_loss_weight of every subject (the cross-attention localisation "
                   "loss; needs --mask-root; the StyleDrop sweep trains in fp32 and refuses the switch); default: not passed on")


def db_parser() -> argparse.ArgumentParser:
    """run_textboost_db.py:41-66 + the flags of this port"""
    p = argparse.ArgumentParser(description="Run TextBoost experiment", epilog=_DEVIATIONS, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("-g", "--gpu", type=str, default="0")
    p.add_argument("-n", "--num-samples", type=int, default=1)
    p.add_argument("-m", "--model", type=str, default="sd21base")
    p.add_argument("--instances", type=str, nargs="+", default=None)
    p.add_argument("--lora-rank", type=int, default=4)
    p.add_argument("--total-steps", type=int, default=250)
    p.add_argument("--lr", type=float, default=1e-4)
    p.add_argument("--emb-lr", type=float, default=1e-3)
    p.add_argument("--batch-size", type=int, default=8)
    p.add_argument("--train-params", type=str, default="none")
    p.add_argument("--augment", type=str, default="pda")
    p.add_argument("--augment-p", type=float, default=0.5)
    p.add_argument("--null-prob", type=float, default=0.1)
    p.add_argument("--kpl-weight", type=float, default=0.1)
    p.add_argument("--no-weighted-sample", action="store_true", default=False)
    p.add_argument("--no-inversion", action="store_true", default=False)
    p.add_argument("--mixing", action="store_true", default=False)
    p.add_argument("--desc", type=str, default=None)
    _common_flags(p, SUBJECTS_DB, "datasets/dreambooth_n1_train")
    return p


def sdrp_parser() -> argparse.ArgumentParser:
    """run_textboost_sdrp.py:35-45 + the flags of this port"""
    p = argparse.ArgumentParser(description="Run TextBoost experiment", epilog=_DEVIATIONS, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("-g", "--gpu", type=str, default="7")
    p.add_argument("-m", "--model", type=str, default="sd21")
    p.add_argument("--instances", type=str, nargs="+", default=None)
    p.add_argument("--augment", type=str, default="pda")
    p.add_argument("--lora-rank", type=int, default=4)
    p.add_argument("--null-prob", type=float, default=0.1)
    p.add_argument("--kpl-weight", type=float, default=0.1)
    p.add_argument("--no-weighted-sample", action="store_true", default=False)
    p.add_argument("--no-inversion", action="store_true", default=False)
    p.add_argument("--desc", type=str, default=None)
    _common_flags(p, SUBJECTS_SDRP, "./datasets/styledrop")
    return p


def load_subjects(path: str, keys: Sequence[str], instances: Optional[Sequence[str]]) -> List[dict]:
    """the subject table, filtered by --instances IN TABLE ORDER (run_textboost_db.py:70-76)"""
    with open(path) as f:
        table = json.load(f)
    for s in table:
        missing = [k for k in keys if k not in s]
        if missing:
            raise SystemExit(f"{path}: subject {s!r} lacks {missing}")
    return table if instances is None else [s for s in table if s["name"] in instances]


# A subject's argv as data: one format string per token, filled from the subject's fields and the driver's flags.  The token order is the
# interface (cmd.txt is compared with the reference's line by line: tests/golden/sweep_commands.json).
DB_ARGV = (
    "train_textboost.py", "--pretrained_model_name_or_path={model_dir}", "--instance_data_dir={data}", "--output_dir=./{outdir}/{name}",
    "--class_token={class_token}", "--instance_token=<0>", "--validation_steps={fifth}", "--placeholder_token=<{name}>",
    "--initializer_token={initializer_token} {class_token}", "--validation_prompts", "photo of a <0>", "a <0> in the jungle",
    "a <0> in the bucket", "painting of a <0> in the Monet style", "--resolution={resolution}", "--lora_rank={lora_rank}",
    "--learning_rate={lr}", "--emb_learning_rate={emb_lr}", "--train_batch_size={per_gpu_batch}", "--max_train_steps={total_steps}",
    "--checkpointing_steps={fifth}", "--gradient_accumulation_steps=1", "--unet_params_to_train={train_params}", "--augment={augment}",
    "--augment_p={augment_p}", "--null_prob={null_prob}", "--kpl_weight={kpl_weight}", "--template=imagenet_small", "--mixed_precision=fp16")
SDRP_ARGV = (
    "train_textboost.py", "--pretrained_model_name_or_path={model_dir}", "--instance_data_dir={data}", "--output_dir=./{outdir}/{name}",
    "--instance_token=<0>", "--validation_prompts", "A man in <0>", "A cat in <0>", "Flowers in <0>", "A dog in <0>", "--validation_steps=25",
    "--placeholder_token", "<{name}>", "--initializer_token", "{initializer_token}", "--lora_rank={lora_rank}", "--learning_rate=1e-4",
    "--emb_learning_rate=1e-3", "--train_batch_size=4", "--max_train_steps=150", "--checkpointing_steps=25", "--gradient_accumulation_steps=1",
    "--augment={augment}", "--kpl_weight={kpl_weight}", "--null_prob={null_prob}", "--template={template}", "--augment_ops=style", "--mixing")


def _fill(template: Sequence[str], switches: Sequence[Tuple[bool, str]], fields: dict) -> List[str]:
    """the template's tokens filled with `fields` (a value that itself holds braces, a StyleDrop template, is inserted as it is), then the
    switches that are on, in their order"""
    return [t.format(**fields) for t in template] + [t.format(**fields) for on, t in switches if on]


def build_db(args) -> Tuple[str, List[Job]]:
    """-> (output directory, [(subject, argv)]) of the DreamBooth sweep: fp16, the model's resolution, a fifth of the steps between validations"""
    key = args.model.lower().replace("-", "")
    if key not in RESOLUTION:
        raise SystemExit(f"-m {args.model}: one of {', '.join(RESOLUTION)} (it names the run and selects the resolution)")
    outdir = "output/tb-" + args.model + ("-all" if args.num_samples is None else f"-n{args.num_samples}") + ("" if args.desc is None else f"-{args.desc}")
    common = dict(vars(args), outdir=outdir, fifth=args.total_steps // 5, per_gpu_batch=args.batch_size // len(args.gpu.split(",")),
                  resolution=RESOLUTION[key] if args.resolution is None else args.resolution)
    switches = ((args.num_samples is not None, "--num_samples={num_samples}"), (not args.no_inversion, "--augment_inversion"),
                (args.no_weighted_sample, "--disable_weighted_sample"), (args.augment == "none", "--center_crop"), (args.mixing, "--mixing"),
                (args.seed is not None, "--seed={seed}"), (args.mask_root is not None, "--instance_mask_dir={mask_root}/{name}"),
                (args.attn_loss_weight is not None, "--attn_loss_weight={attn_loss_weight}"))
    jobs = []
    for s in load_subjects(args.subjects, ("name", "class_token", "initializer_token"), args.instances):
        jobs.append((s["name"], _fill(DB_ARGV, switches, dict(common, **s, data=os.path.join(args.data_dir, s["name"])))))
    return outdir, jobs


def build_sdrp(args) -> Tuple[str, List[Job]]:
    """-> (output directory, [(subject, argv)]) of the StyleDrop sweep: no --mixed_precision (fp32), the subject's own prompt template"""
    if args.attn_loss_weight is not None:   # (here, on the host, before any subject starts: every one of them would raise in setup_shared)
        raise SystemExit("--attn-loss-weight: the StyleDrop sweep trains without --mixed_precision (fp32), and the localisation loss has 16-bit "
                         "kernels only; use it on run_textboost_db.py")
    outdir = "output/tb_style-" + args.model + ("" if args.desc is None else f"-{args.desc}")
    common = dict(vars(args), outdir=outdir)
    switches = ((not args.no_inversion, "--augment_inversion"), (args.no_weighted_sample, "--disable_weighted_sample"),
                (args.resolution is not None, "--resolution={resolution}"), (args.seed is not None, "--seed={seed}"),
                (args.mask_root is not None, "--instance_mask_dir={mask_root}/{name}"))
    jobs = []
    for s in load_subjects(args.subjects, ("name", "template", "initializer_token"), args.instances):
        jobs.append((s["name"], _fill(SDRP_ARGV, switches, dict(common, **s, data=f"{args.data_dir}/{s['name']}"))))
    return outdir, jobs


def _flag(cmd: Sequence[str], flag: str) -> Optional[str]:
    for i, t in enumerate(cmd):
        if t.startswith(flag + "="):
            return t[len(flag) + 1:]
        if t == flag and i + 1 < len(cmd):
            return cmd[i + 1]
    return None


def write_records(cmd: Sequence[str]):
    """<output_dir>/cmd.txt and the copy of train_textboost.py (run_textboost_db.py:164-168)"""
    out = _flag(cmd, "--output_dir")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "cmd.txt"), "w") as f:
        f.write("\n".join(cmd))
    shutil.copy(TRAIN_SCRIPT, os.path.join(out, "train_textboost.py"))


def cannot_start(cmd: Sequence[str]) -> Optional[str]:
    """why a subject cannot start, found without touching the device; None when it can"""
    from . import data as tbdata
    d = _flag(cmd, "--instance_data_dir")
    if not d or not os.path.isdir(d):
        return f"no data directory {d}"
    if not tbdata.has_instance_images(d):
        return f"no images in {d}"
    return None


def _result(name, status, reason=None, **kw):
    r = {"name": name, "status": status, "reason": reason}
    r.update(kw)
    return r


def sweep_in_process(jobs: Sequence[Job], report: Callable[[dict], None] = lambda r: None) -> List[dict]:
    """Every subject in this process: the frozen models are built once (`setup_shared`) and stay on the device; a subject's trainable state,
    executors, graph and buffers are released before the next subject is built.  A `crossattn_kv` subject writes adapters into the shared UNets
    and therefore gets a context of its own."""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import torch
    import train_textboost as T
    results, ctx = [], None
    runnable = [i for i, (_, cmd) in enumerate(jobs) if cannot_start(cmd) is None]
    try:
        for i, (name, cmd) in enumerate(jobs):
            if int(os.environ.get("RANK", "0")) == 0:
                write_records(cmd)
            reason = cannot_start(cmd)
            if reason is not None:
                results.append(_result(name, "skipped", reason))
                report(results[-1])
                continue
            t0 = time.perf_counter()
            setup_s, spent, error, args = 0.0, None, None, None
            try:
                args = T.parse_args(list(cmd[1:]))
                private = args.unet_params_to_train == "crossattn_kv"
                if ctx is None or private:
                    ctx = None
                    ctx = T.setup_shared(args)
                    setup_s = time.perf_counter() - t0
                spent = T.train_subject(ctx, args, final=i == runnable[-1])
                if private:
                    ctx = None
            except INPUT_ERRORS as e:   # the subject's inputs, not the device: report it and go on
                error = f"{type(e).__name__}: {e}"
                if ctx is not None and args is not None and args.unet_params_to_train == "crossattn_kv":
                    ctx = None   # its UNets may already carry this subject's adapters
            gc.collect()   # nothing of a finished subject stays on the device
            if error is not None:
                T.release_subject_caches()   # (train_subject does this itself when it returns)
            mem = torch.cuda.memory_allocated() if torch.cuda.is_available() else 0
            seconds = round(time.perf_counter() - t0, 3)
            if error is not None:
                results.append(_result(name, "failed", error, seconds=seconds, device_bytes=mem))
            else:
                results.append(_result(name, "ok", seconds=seconds, setup_seconds=round(setup_s, 3),
                                       spent={k: round(v, 3) for k, v in spent.items()}, device_bytes=mem))
            report(results[-1])
    finally:
        ctx = None
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            dist.destroy_process_group()
    return results


def child_command(cmd: Sequence[str], num_gpu: int) -> List[str]:
    """the reference's form: one process (group) per subject"""
    if num_gpu > 1:
        return [sys.executable, "-m", "torch.distributed.run", "--rdzv-backend=c10d", "--rdzv-endpoint=localhost:0",
                f"--nproc-per-node={num_gpu}", TRAIN_SCRIPT] + list(cmd[1:])
    return [sys.executable, TRAIN_SCRIPT] + list(cmd[1:])


def worker_command(num_gpu: int, jobs_file: str) -> List[str]:
    """one launch for the whole sweep: every rank runs `python -m textboost_amd.sweep --worker JOBS`"""
    return [sys.executable, "-m", "torch.distributed.run", "--rdzv-backend=c10d", "--rdzv-endpoint=localhost:0", f"--nproc-per-node={num_gpu}",
            "-m", "textboost_amd.sweep", "--worker", jobs_file]


def _child_env() -> dict:
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + (os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else "")
    return env


def sweep_fresh_process(jobs: Sequence[Job], num_gpu: int, report: Callable[[dict], None] = lambda r: None, run=subprocess.run) -> List[dict]:
    results = []
    for k, (name, cmd) in enumerate(jobs):
        write_records(cmd)
        reason = cannot_start(cmd)
        if reason is not None:
            results.append(_result(name, "skipped", reason))
            report(results[-1])
            continue
        t0 = time.perf_counter()
        rc = run(child_command(cmd, num_gpu), env=_child_env()).returncode
        seconds = round(time.perf_counter() - t0, 3)
        results.append(_result(name, "ok", seconds=seconds) if rc == 0 else _result(name, "failed", f"exit status {rc}", seconds=seconds))
        report(results[-1])
        if rc not in (0, INPUT_ERROR_STATUS):
            # a HIP runtime or kernel library error ends a child with status 1, a device fault may abort it: whatever is not the trainer's own
            # "this subject's inputs are wrong" status ends the sweep, and nothing more is started on that device
            results += [_result(n, "not started", f"the sweep ended at {name}") for n, _ in jobs[k + 1:]]
            break
    return results


def _print_result(r: dict):
    print(json.dumps(r), flush=True)


def run_sweep(outdir: str, jobs: Sequence[Job], gpu: str, fresh_process: bool, run=subprocess.run) -> int:
    """-> the driver's exit status"""
    os.makedirs(outdir, exist_ok=True)
    num_gpu = len(gpu.split(","))
    os.environ["CUDA_VISIBLE_DEVICES"] = gpu   # run_textboost_db.py:105 (the HIP runtime honours it)
    if fresh_process:
        results = sweep_fresh_process(jobs, num_gpu, _print_result, run)
    elif num_gpu > 1:
        for _, cmd in jobs:
            write_records(cmd)
        with tempfile.TemporaryDirectory() as tmp:
            jobs_file = os.path.join(tmp, "jobs.json")
            with open(jobs_file, "w") as f:
                json.dump([[n, list(c)] for n, c in jobs], f)
            rc = run(worker_command(num_gpu, jobs_file), env=_child_env()).returncode
        return rc
    else:
        results = sweep_in_process(jobs, _print_result)
    return summarize(results)


def summarize(results: Sequence[dict]) -> int:
    bad = [r for r in results if r["status"] != "ok"]
    print(f"{len(results) - len(bad)} of {len(results)} subjects trained", flush=True)
    for r in bad:
        print(f"  {r['status']}: {r['name']}: {r['reason']}", flush=True)
    return 1 if bad else 0


def _main(parser, build, argv=None) -> int:
    from .generate import check_model_dir
    args = parser.parse_args(argv)
    check_model_dir(args.model_dir, parser.prog, flag="--model-dir")
    outdir, jobs = build(args)
    return run_sweep(outdir, jobs, args.gpu, args.fresh_process)


def main_db(argv=None) -> int:
    return _main(db_parser(), build_db, argv)


def main_sdrp(argv=None) -> int:
    return _main(sdrp_parser(), build_sdrp, argv)


def worker(jobs_file: str) -> int:
    """what every rank of a multi-GPU sweep runs; rank 0 reports"""
    with open(jobs_file) as f:
        jobs = [(n, c) for n, c in json.load(f)]
    main_rank = int(os.environ.get("RANK", "0")) == 0
    results = sweep_in_process(jobs, _print_result if main_rank else (lambda r: None))
    return summarize(results) if main_rank else int(any(r["status"] != "ok" for r in results))


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--worker":
        sys.exit(worker(sys.argv[2]))
    sys.exit("usage: python -m textboost_amd.sweep --worker JOBS.json   (started by run_textboost_db.py / run_textboost_sdrp.py)")
