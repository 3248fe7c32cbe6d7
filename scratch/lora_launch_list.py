"""The C-ABI entry points one r = 4 training step calls, in order (every launch goes through `_lib.check(rc, name)`): run on two checkouts and
compare the files to show that a change left the default path's launches alone.

    python scratch/lora_launch_list.py OUT.json [PACKAGE_PARENT_DIR]
"""
import json
import os
import sys

root = sys.argv[2] if len(sys.argv) > 2 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
import torch  # noqa: E402

from textboost_amd import _lib  # noqa: E402
from textboost_amd.workload import build_step  # noqa: E402

assert torch.cuda.is_available()
step, _ = build_step(batch=8, lora_rank=4)
step.step_eager()
torch.cuda.synchronize()
names = []
check = _lib.check


def recording_check(rc, what):
    names.append(what)
    return check(rc, what)


_lib.check = recording_check
step.step_eager()
torch.cuda.synchronize()
_lib.check = check
with open(sys.argv[1], "w") as f:
    json.dump({"package": os.path.abspath(os.path.join(root, "textboost_amd")), "lora_rank": 4, "launches": len(names), "entry_points": names}, f)
print(len(names), "launches ->", sys.argv[1])
