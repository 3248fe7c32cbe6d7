"""Writes tests/golden/sweep_commands.json, sweep_subjects_db.json and sweep_subjects_sdrp.json: the command line the REFERENCE's sweep drivers
(`run_textboost_db.py`, `run_textboost_sdrp.py`) start per subject, the text of the `cmd.txt` they write and where, for the default flags and a
few others; and the two subject tables the drivers carry.

The reference's own `main(args)` runs unchanged in a temporary working directory; `subprocess.run`, `shutil.copy` and the `cmd.txt` writes are
replaced by recorders.  Both drivers import the standard library only.  Nothing of the reference is copied: the fixtures hold command lines, file
names, texts and the names of the tables.

    python tests/golden/gen_sweep_commands.py <directory of the reference checkout>"""
import argparse
import importlib.util
import io
import json
import os
import sys
import tempfile
import types

HERE = os.path.dirname(os.path.abspath(__file__))

CASES = [
    # name, driver, flags
    ("db_defaults", "db", []),
    ("db_sd21_two_gpus", "db", ["-m", "sd21", "-g", "0,1", "--batch-size", "8", "--total-steps", "100", "--augment", "none", "--mixing",
                                "--no-inversion", "--no-weighted-sample", "--desc", "x"]),
    ("db_instances", "db", ["--instances", "dog", "cat2"]),
    ("sdrp_defaults", "sdrp", []),
    ("sdrp_no_inversion", "sdrp", ["--no-inversion"]),
]


def load(ref_dir, name):
    spec = importlib.util.spec_from_file_location("reference_" + name, os.path.join(ref_dir, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class Recorder:
    """stands in for subprocess / shutil / open inside a driver module"""

    def __init__(self):
        self.runs, self.writes, self.copies = [], [], []

    def install(self, mod):
        rec = self
        mod.subprocess = types.SimpleNamespace(run=lambda cmd, *a, **k: rec.runs.append(list(cmd)))
        mod.shutil = types.SimpleNamespace(copy=lambda src, dst: rec.copies.append([src, dst]))

        class _File(io.StringIO):
            def __init__(self, path):
                super().__init__()
                self.path = path

            def close(self):
                rec.writes.append([self.path, self.getvalue()])
                super().close()

        def _open(path, mode="r", *a, **k):
            assert "w" in mode, (path, mode)
            return _File(path)
        mod.open = _open


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("reference", help="directory that holds the reference's run_textboost_db.py and run_textboost_sdrp.py")
    ref_dir = os.path.abspath(ap.parse_args().reference)
    db, sdrp = load(ref_dir, "run_textboost_db"), load(ref_dir, "run_textboost_sdrp")
    tables = {
        "sweep_subjects_db.json": [{"name": n, "class_token": c, "initializer_token": t} for n, c, t in db.INSTANCES],
        "sweep_subjects_sdrp.json": [{"name": n, "template": c, "initializer_token": t} for n, c, t in sdrp.INSTANCES],
    }
    for fn, table in tables.items():
        with open(os.path.join(HERE, fn), "w") as f:
            json.dump(table, f, indent=1)
    out = {"cases": []}
    cwd, visible = os.getcwd(), os.environ.get("CUDA_VISIBLE_DEVICES")
    for name, driver, flags in CASES:
        mod = db if driver == "db" else sdrp
        rec = Recorder()
        rec.install(mod)
        with tempfile.TemporaryDirectory() as tmp:
            os.chdir(tmp)
            try:
                sys.argv = [f"run_textboost_{driver}.py"] + flags
                args = mod.parse_args() if driver == "db" else mod.parser.parse_args()
                mod.main(args)
                made = sorted(os.path.relpath(os.path.join(d, s), tmp) for d, subs, _ in os.walk(tmp) for s in subs)
            finally:
                os.chdir(cwd)
        assert len(rec.runs) == len(rec.writes)
        subjects = []
        for i, (cmd, (path, text)) in enumerate(zip(rec.runs, rec.writes)):
            k = cmd.index("train_textboost.py")
            subjects.append({"launcher": cmd[:k], "cmd": cmd[k:], "cmd_txt_path": path, "cmd_txt": text,
                             "copy": rec.copies[i] if rec.copies else None})
        out["cases"].append({"name": name, "driver": driver, "flags": flags, "directories_made": made,
                             "cuda_visible_devices": os.environ.get("CUDA_VISIBLE_DEVICES"), "subjects": subjects})
    if visible is None:
        os.environ.pop("CUDA_VISIBLE_DEVICES", None)
    else:
        os.environ["CUDA_VISIBLE_DEVICES"] = visible
    path = os.path.join(HERE, "sweep_commands.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(f"wrote {path}: {len(out['cases'])} cases, {sum(len(c['subjects']) for c in out['cases'])} command lines; "
          f"{len(tables['sweep_subjects_db.json'])} + {len(tables['sweep_subjects_sdrp.json'])} subjects")


if __name__ == "__main__":
    main()
