#!/usr/bin/env python
"""DreamBooth subject sweep -- drop-in for the reference's `run_textboost_db.py` (see textboost_amd/sweep.py and --help).

    python run_textboost_db.py -g 0 -m sd15 --model-dir <local diffusers model directory>"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from textboost_amd.sweep import main_db  # noqa: E402

if __name__ == "__main__":
    sys.exit(main_db())
