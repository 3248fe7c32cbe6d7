"""Writes tests/golden/eval_generate_names.json: what the REFERENCE's `eval_dreambooth.generate()` asks of its pipeline and where it saves, for a
live and an object subject with one and two placeholder vectors, with and without --checkpoint / --output-desc / a custom --token-format.

The reference's own `generate()` and `generate_from_pipeline()` run unchanged; only `load_pipeline` is replaced by a stub whose pipeline records
the prompts of every call and returns images whose `save` records the path.  The third-party modules the reference's imports name and this host
may lack (clip, t2v_metrics, diffusers, torchvision, tqdm, and its own textboost package, which imports transformers internals) are stubbed in
`sys.modules` first.  Nothing of the reference is copied: the fixture holds prompts, file names and the arguments of each case.

    python tests/golden/gen_eval_generate_names.py <directory of the reference checkout>"""
import argparse
import importlib.util
import json
import os
import sys
import tempfile
import types

HERE = os.path.dirname(os.path.abspath(__file__))

CASES = [
    # name, instances, files of the model path beside text_encoder/, extra flags
    ("live_one_vector", ["dog"], {"dog": ["dog.bin"]}, []),
    ("object_one_vector", ["can"], {"can": ["can.bin"]}, []),
    ("live_two_vectors", ["cat2"], {"cat2": ["cat2_0.bin", "cat2_1.bin"]}, []),
    ("object_two_vectors_checkpoint_desc", ["bear_plushie"], {"bear_plushie": ["bear_plushie_0.bin", "bear_plushie_1.bin", "optimizer.bin"]},
     ["--checkpoint", "100", "--output-desc", "v2"]),
    ("token_format_textual_inversion", ["teapot"], {"teapot": ["teapot.bin"]}, ["--token-format", "<INSTANCE>"]),
    ("two_subjects_two_seeds", ["dog", "can"], {"dog": ["dog.bin"], "can": ["can.bin", "hflip.bin"]}, ["--seeds", "0", "3"]),
]


def stub_modules():
    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    class _Any:
        def __init__(self, *a, **k):
            pass

        def __getattr__(self, n):
            return _Any()

        def __call__(self, *a, **k):
            return _Any()

        @classmethod
        def from_config(cls, *a, **k):
            return cls()

        @classmethod
        def from_pretrained(cls, *a, **k):
            return cls()

    mod("clip")
    mod("t2v_metrics")
    mod("diffusers", DiffusionPipeline=_Any, DPMSolverMultistepScheduler=_Any)
    tv = mod("torchvision")
    tr = mod("torchvision.transforms")
    v2 = mod("torchvision.transforms.v2")
    tv.transforms, tr.v2 = tr, v2
    mod("tqdm", tqdm=lambda it, *a, **k: it)
    tb = mod("textboost")
    tb.text_encoder = mod("textboost.text_encoder", TextBoostModel=_Any)


class StubImage:
    def __init__(self, log):
        self.log = log

    def save(self, path):
        self.log.append(path)


class StubPipeline:
    """what generate() / generate_from_pipeline() touch of a diffusers pipeline"""

    def __init__(self, calls, saved):
        import torch
        self.calls, self.saved = calls, saved
        self.dtype = torch.float32
        self.tokenizer = "stub tokenizer"
        self.scheduler = types.SimpleNamespace(config={})

    def to(self, *a, **k):
        return self

    def __call__(self, prompt, num_inference_steps, guidance_scale, latents):
        self.calls.append({"prompts": list(prompt), "num_inference_steps": num_inference_steps, "guidance_scale": guidance_scale,
                           "latents_shape": list(latents.shape), "latent_rows_equal": bool((latents == latents[:1]).all())})
        out = types.SimpleNamespace()
        out.images = [StubImage(self.saved) for _ in prompt]
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("reference", help="directory that holds the reference's eval_dreambooth.py")
    ref_dir = ap.parse_args().reference
    stub_modules()
    spec = importlib.util.spec_from_file_location("reference_eval_dreambooth", os.path.join(ref_dir, "eval_dreambooth.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    out = {"instances": dict(ref.INSTANCES), "live": {k: bool(ref.is_live(k)) for k in ref.INSTANCES}, "cases": []}
    for name, instances, files, flags in CASES:
        with tempfile.TemporaryDirectory() as tmp:
            run = os.path.join(tmp, "runs", "tb-sd15-n1")
            for inst, names in files.items():
                mp = os.path.join(run, inst, "checkpoint-100" if "--checkpoint" in flags else "")
                os.makedirs(os.path.join(mp, "text_encoder"))
                for n in names:
                    open(os.path.join(mp, n), "wb").close()
            calls, saved, loaded = [], [], []

            def load_pipeline(model_path, pretrained_model, dtype=None):
                loaded.append(os.path.relpath(model_path, tmp))
                return StubPipeline(calls, saved)
            ref.load_pipeline = load_pipeline
            argv = [run + "/", "--outdir", os.path.join(tmp, "bench") + "/", "--instances", *instances, "--model", "sd15", *flags]
            if "--seeds" not in flags:
                argv += ["--seeds", "1"]
            sys.argv = ["eval_dreambooth.py"] + argv
            args = ref.parse_args()
            root = ref.generate(args, "cpu")
            out["cases"].append({
                "name": name, "instances": instances, "files": files,
                "argv": [a.replace(tmp, "<tmp>") for a in argv],
                "image_root": os.path.relpath(root, tmp), "model_paths": [p.rstrip("/") for p in loaded],
                "calls": calls, "saved": [os.path.relpath(p, tmp) for p in saved]})
    path = os.path.join(HERE, "eval_generate_names.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(f"wrote {path}: {len(out['cases'])} cases, {sum(len(c['saved']) for c in out['cases'])} file names")


if __name__ == "__main__":
    main()
