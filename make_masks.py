#!/usr/bin/env python3
"""Subject masks for the masked training loss (--instance_mask_dir / --mask-root) and for editing, from the model's own cross-attention
(textboost_amd/auto_mask.py): no mask has to be painted by hand.

    python make_masks.py data/dog --model <diffusers dir> --word dog --output masks/dog
    python make_masks.py --subjects FILE --data-dir DIR --model <diffusers dir> --output masks [-n 1] [--instances a b]
        [--prompt "a photo of a {}"] [--timesteps 100 300 500] [--draws 2] [--seed 0] [--soft] [--dilate PX] [--preview-dir DIR] [--force]

First form: every image of the directory (the first N with -n, as the trainer's --num_samples counts them) gives `<output>/<stem>.png`, Pillow
mode "L" at the image's own size (EXIF orientation applied, as the trainer decodes it), white = subject: the layout --instance_mask_dir reads.
Second form: every subject of the sweep's table (default: the DreamBooth table of run_textboost_db.py; --instances selects) with word = its
class_token, images from `<data-dir>/<name>`, masks to `<output>/<name>/<stem>.png`: `run_textboost_db.py --mask-root <output>` then works as it is.

One photo is one forward of the frozen UNet at batch len(timesteps) * draws on the base (untrained) text encoder: a class word needs no run.
--soft writes the normalised attention itself (0 .. 255) instead of Otsu's cut; --dilate PX grows the mask by a square of radius PX;
--preview-dir DIR also writes `<stem>.jpg`, the attention laid over the photo, to look at before training (second form: `DIR/<name>/`).  An
existing mask is overwritten only with --force; --output may not be the data directory.  One line per image: path, min, max, Otsu bin,
foreground share.  The default timesteps and draws are a choice from the literature's range, not measured on pretrained weights here."""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PROG = "make_masks.py"


def build_parser():
    from textboost_amd import auto_mask as A
    from textboost_amd.sweep import SUBJECTS_DB
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("data", type=str, nargs="?", default=None, help="directory of one subject's images (first form)")
    p.add_argument("--model", type=str, default=None, help="local diffusers model directory")
    p.add_argument("--word", type=str, default=None, help="first form: the class word whose attention makes the mask (dog, sofa)")
    p.add_argument("--output", type=str, default=None, help="mask directory (second form: the directory of the subjects' mask directories)")
    p.add_argument("--subjects", type=str, default=SUBJECTS_DB, help="second form: JSON list of subjects (default: %(default)s)")
    p.add_argument("--data-dir", dest="data_dir", type=str, default=None, help="second form: directory of the subjects' image directories")
    p.add_argument("--instances", type=str, nargs="+", default=None, help="second form: only these subjects")
    p.add_argument("-n", "--num-samples", dest="num_samples", type=int, default=None, help="only the first N images of a directory (default: all)")
    p.add_argument("--prompt", type=str, default=A.DEFAULT_PROMPT, help="the prompt, {} = the word (default: %(default)r)")
    p.add_argument("--timesteps", type=int, nargs="+", default=list(A.DEFAULT_TIMESTEPS), help="noise levels of the UNet rows (default: %(default)s)")
    p.add_argument("--draws", type=int, default=A.DEFAULT_DRAWS, help="noise draws per timestep (default: %(default)s)")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--soft", action="store_true", help="write the normalised attention (0 .. 255) instead of the thresholded mask")
    p.add_argument("--dilate", type=int, default=0, metavar="PX", help=f"grow the mask by a square of this radius (0 .. {A.MAX_DILATE})")
    p.add_argument("--preview-dir", dest="preview_dir", type=str, default=None, metavar="DIR", help="also write <stem>.jpg overlays here")
    p.add_argument("--force", action="store_true", help="overwrite existing masks")
    return p


def _same_dir(a: str, b: str) -> bool:
    return os.path.realpath(a) == os.path.realpath(b)


def latent_size(model_dir: str) -> int:
    cfg = os.path.join(model_dir, "unet", "config.json")
    if not os.path.exists(cfg):
        raise SystemExit(f"{PROG}: {cfg} is missing: --model must be a local diffusers model directory")
    with open(cfg) as f:
        return int(json.load(f).get("sample_size", 64))


def plan(args):
    """every refusal that needs no device -> [(image path, word, mask path, preview path or None)]"""
    from textboost_amd import auto_mask as A
    from textboost_amd import data as D
    from textboost_amd import edit as E
    from textboost_amd import generate as G
    from textboost_amd.sweep import load_subjects
    if not args.model:
        raise SystemExit(f"{PROG}: --model DIR (a local diffusers model directory: unet/, vae/, text_encoder/, tokenizer/, scheduler/) is required")
    G.check_model_dir(args.model, PROG)
    if not args.output:
        raise SystemExit(f"{PROG}: --output DIR is required")
    if args.draws < 1 or not args.timesteps:
        raise SystemExit(f"{PROG}: --draws and --timesteps need at least one draw and one timestep")
    if not 0 <= args.dilate <= A.MAX_DILATE:
        raise SystemExit(f"{PROG}: --dilate {args.dilate}: 0 .. {A.MAX_DILATE} pixels")
    try:
        args.prompt.format("x")
    except (IndexError, KeyError, ValueError):
        raise SystemExit(f"{PROG}: --prompt {args.prompt!r}: one {{}} marks the word's place")
    if "{}" not in args.prompt:
        raise SystemExit(f"{PROG}: --prompt {args.prompt!r} has no {{}} for the word")
    if args.data is not None:          # first form
        if args.data_dir is not None or args.instances is not None:
            raise SystemExit(f"{PROG}: give either one image directory with --word, or --data-dir for the subject table, not both")
        if not args.word or not args.word.strip():
            raise SystemExit(f"{PROG}: --word WORD is required with an image directory (the subject's class word)")
        groups = [(args.data, args.word, args.output, args.preview_dir)]
    else:
        if args.word is not None:
            raise SystemExit(f"{PROG}: --word goes with one image directory; the subject table carries every subject's class_token")
        if not args.data_dir:
            raise SystemExit(f"{PROG}: give an image directory and --word, or --data-dir DIR for the subject table")
        subjects = load_subjects(args.subjects, ("name", "class_token"), args.instances)
        if not subjects:
            raise SystemExit(f"{PROG}: --instances {args.instances}: no such subject in {args.subjects}")
        groups = [(os.path.join(args.data_dir, s["name"]), s["class_token"], os.path.join(args.output, s["name"]),
                   None if args.preview_dir is None else os.path.join(args.preview_dir, s["name"])) for s in subjects]
    grid = latent_size(args.model)
    try:
        E.check_vae_has_encoder(args.model)
    except (OSError, ValueError) as e:
        raise SystemExit(f"{PROG}: {e}")
    jobs, exist = [], []
    for src, word, out, preview in groups:
        if not os.path.isdir(src):
            raise SystemExit(f"{PROG}: {src} is not a directory")
        if _same_dir(src, out):
            raise SystemExit(f"{PROG}: --output {out} is the data directory: the masks would be read as training images")
        if preview is not None and (_same_dir(preview, out) or _same_dir(preview, src)):
            raise SystemExit(f"{PROG}: --preview-dir {preview} is the mask or data directory: the previews are neither masks nor training images")
        paths = D.instance_image_paths(src, args.num_samples)
        if not paths:
            raise SystemExit(f"{PROG}: {src} holds no image files")
        for p in paths:
            stem = os.path.splitext(os.path.basename(p))[0]
            W, H = D._pixel_size(p)
            try:
                A.check_photo_size(W, H, grid, grid, p)
            except ValueError as e:
                raise SystemExit(f"{PROG}: {e}")
            mask = os.path.join(out, stem + ".png")
            if os.path.exists(mask):
                exist.append(mask)
            jobs.append((p, word, mask, None if preview is None else os.path.join(preview, stem + ".jpg")))
    if exist and not args.force:
        raise SystemExit(f"{PROG}: {len(exist)} mask(s) exist already ({exist[0]}{', ...' if len(exist) > 1 else ''}): pass --force to overwrite")
    return jobs


def build_maker(args):
    """the executors of one model directory: the UNet at batch len(timesteps) * draws on the fp16 library, the base text encoder, the VAE encoder"""
    from safetensors.torch import load_file
    from textboost_amd import _lib, models
    from textboost_amd import edit as E
    from textboost_amd import generate as G
    from textboost_amd.auto_mask import MaskMaker
    from textboost_amd.sampler import DPMSolverPP2M
    from textboost_amd.unet import HipUNet
    model = args.model
    _lib.set_half("fp16")
    R = len(args.timesteps) * args.draws
    with open(os.path.join(model, "unet", "config.json")) as f:
        ucfg = json.load(f)
    scfg = None
    spath = os.path.join(model, "scheduler", "scheduler_config.json")
    if os.path.exists(spath):
        with open(spath) as f:
            scfg = json.load(f)
    size = int(ucfg.get("sample_size", 64))
    base = G.load_base_text(model)
    te, tokenizer = G.load_text_encoder(model, G.TrainedRun(path=model, rank=0, lora={}), R, base=base)
    unet = HipUNet(models.unet_geometry_from_config(ucfg), load_file(os.path.join(model, "unet", "diffusion_pytorch_model.safetensors")), R, size,
                   size, text_len=base.geo.max_pos)
    enc = E.EditEncoder(model, size)
    return MaskMaker(unet, enc, lambda ids: te.forward(ids, pins=False), tokenizer, DPMSolverPP2M.from_config(scfg).alphas_cumprod,
                     timesteps=args.timesteps, seed=args.seed)


def main(argv=None):
    args = build_parser().parse_args(argv)
    jobs = plan(args)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit(f"{PROG} needs an MI355X: the product path has no CPU fallback")
    from PIL import Image
    from textboost_amd import auto_mask as A
    from textboost_amd import data as D
    from textboost_amd.attn_maps import overlay
    with torch.no_grad():
        maker = build_maker(args)
        for path, word, out, preview in jobs:
            rgb = D.decode_rgb(path)
            try:
                score = maker.score(rgb, word, args.prompt)
            except ValueError as e:
                raise SystemExit(f"{PROG}: {path}: {e}")
            mask, stats = maker.mask_of(score, soft=args.soft, dilate=args.dilate)
            os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
            Image.fromarray(mask.cpu().numpy()).save(out)
            print(f"{path} -> {out}: {A.describe(mask, stats)}")
            if preview is not None:
                os.makedirs(os.path.dirname(preview) or ".", exist_ok=True)
                Image.fromarray(overlay(rgb, score)).save(preview)
    print(f"wrote {len(jobs)} mask(s)")


if __name__ == "__main__":
    main()
