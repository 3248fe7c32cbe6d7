#!/usr/bin/env python
"""StyleDrop style sweep -- drop-in for the reference's `run_textboost_sdrp.py` (see textboost_amd/sweep.py and --help).

    python run_textboost_sdrp.py -g 0 -m sd21 --model-dir <local diffusers model directory>"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from textboost_amd.sweep import main_sdrp  # noqa: E402

if __name__ == "__main__":
    sys.exit(main_sdrp())
