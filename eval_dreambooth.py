#!/usr/bin/env python3
"""Image generation and CLIP-T / CLIP-I / DINO / VQA evaluation of a trained DreamBooth run: the reference's eval_dreambooth.py (`generate`
:270-350, `clip_score` :353-374, `clip_i` :377-453, `dino_score` :456-543, `vqa_score` :546-565, the CSV of `main` :568-628) with the same
flags, on the HIP executors of textboost_amd/generate.py (text encoder with the trained adapter and tokens, guided DPM-Solver++ sampling, VAE
decoder), the HIP CLIP ViT-L/14 of textboost_amd/clip_score.py, the HIP DINOv2 ViT-L/14 of textboost_amd/dino_score.py and the HIP
CLIP-FlanT5 encoder-decoder of textboost_amd/vqa_score.py.

    python eval_dreambooth.py <path> --model <diffusers model dir> --metric clip-t clip-i dino --clip-model <CLIPModel dir> \
        --dino-model <DINOv2 weights> [--instances dog can ...] [--token-format "<INSTANCE> SUBJECT"] [--prompt-batch 16]
    python eval_dreambooth.py <path> --skip-gen --metric clip-t clip-i dino --clip-model <CLIPModel dir> --dino-model <DINOv2 weights> \
        [--outdir ./benchmarks] [--seeds 0 1 2 3] [--train-dir ...] [--val-dir ...] [--dreambooth-path ./data/dreambooth] [--checkpoint N]
        [--output-desc D]
    python eval_dreambooth.py <path> --skip-gen --metric clip-t clip-i vqa --clip-model <CLIPModel dir> --vqa-model <clip-flant5 dir>

Without --skip-gen the images are generated first: for every subject (`--instances`, else those of the 30 DreamBooth subjects that exist as
sub-directories of `path`) the trained output directory `<path>/<instance>[/checkpoint-<N>]` is read back (text_encoder/ adapter, `<token>.bin`),
and 25 prompts x `--seeds` are sampled (25 steps, guidance 7.5, one latent per seed) into
`<outdir>/<basename(path)>[-<checkpoint>][_<desc>]/seed<s>/<instance>/<prompt>.png`.  --model names a LOCAL diffusers model directory (unet/,
vae/, text_encoder/, tokenizer/, scheduler/); the reference's aliases (sd15, ...) name hub repositories and are refused.  The scores are then
computed from the PNGs exactly as a --skip-gen run computes them.  --freeu [B1 B2 S1 S2] and --freeu-backbone scalar|structure sample the
images with FreeU, as inference.py does, so that its effect on a subject can be scored; they are refused with --skip-gen.

Images are read from `<outdir>/<basename(path)>[-<checkpoint>][_<desc>]/seed<s>/<instance>/*.png`; the scores go to
`<path>/metric{_ckpt<N>|_last}{_<desc>}.csv` in the reference's format.  --clip-model names a local transformers
`CLIPModel` directory (config.json, model.safetensors, vocab.json, merges.txt): it replaces the reference's download of ViT-L/14@336px.
--dino-model names the hub's `dinov2_vitl14_pretrain.pth` or a local transformers `Dinov2Model` directory: it replaces the reference's
`torch.hub.load('facebookresearch/dinov2', 'dinov2_vitl14')`.  DINO reads the real images from `<dreambooth-path>/<instance>/*.*` (sorted) and
takes N, the number of seen ones, from `path` as the reference does (`<name>-<model>-n<N>`, e.g. `out/tb-sd15-n1`): an instance's first N real
images are seen, the rest unseen.

--vqa-model names a local clip-flant5 directory (config.json, safetensors or .bin shards with the T5 and `mm_projector` weights, the T5
tokenizer files): it replaces the reference's download of t2v_metrics' `clip-flant5-xxl`; its vision tower is the one of --clip-model.  The
score of an image is P("Yes") for the question 'Does this figure show "<file name>"? Please answer yes or no.', in bfloat16 arithmetic.

Without --vqa-model the VQA score is not built: asking for it is an error, so that a 0.000 placeholder in the CSV never reads as a score."""
from __future__ import annotations

import argparse
import csv
import glob
import os
import sys
from typing import Dict, List, Optional

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

METRIC_KEYS = ("clip_score", "vqa_score", "clip_i", "clip_i_unseen", "dino", "dino_unseen")   # eval_dreambooth.py:575-586, CSV column order
BUILT_METRICS = ("clip-t", "clip-i", "dino")


def build_parser():
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("path", type=str, help="path to model")
    p.add_argument("--token-format", type=str, default="<INSTANCE> SUBJECT", help="prompt token format (image generation only)")
    p.add_argument("--outdir", type=str, default="./benchmarks")
    p.add_argument("--checkpoint", type=int, default=None)
    p.add_argument("--instances", type=str, nargs="+", default=None)
    p.add_argument("--skip-gen", action="store_true")
    p.add_argument("--metric", type=str, nargs="+", default=["clip-t", "clip-i", "vqa"])
    p.add_argument("--seeds", type=int, nargs="+", default=[0, 1, 2, 3])
    p.add_argument("--dreambooth-path", type=str, default="./data/dreambooth")
    p.add_argument("--train-dir", type=str, default="./data/dreambooth_n1_train")
    p.add_argument("--val-dir", type=str, default="./data/dreambooth_n1_val")
    p.add_argument("--model", type=str, default=None, help="local diffusers model directory (image generation only)")
    p.add_argument("--prompt-batch", type=int, default=16, help="prompts per sampling batch at most (image generation only)")
    p.add_argument("--output-desc", type=str, default=None)
    p.add_argument("--clip-model", type=str, default=None, help="local transformers CLIPModel directory (ViT-L/14@336px) with its tokenizer files")
    p.add_argument("--dino-model", type=str, default=None,
                   help="DINOv2 ViT-L/14 weights: the hub's dinov2_vitl14_pretrain.pth or a local transformers Dinov2Model directory")
    p.add_argument("--vqa-model", type=str, default=None,
                   help="local clip-flant5 directory (config.json, T5 + mm_projector weights, tokenizer files); its vision tower is --clip-model's")
    p.add_argument("--batch-size", type=int, default=32, help="images per tower launch")
    from textboost_amd import freeu as F
    F.add_arguments(p)      # (image generation only)
    return p


def check_freeu_args(parser, args):
    """--freeu / --freeu-backbone of the generation stage -> None or (b1, b2, s1, s2, mode); refused by flag name before any model is built"""
    from textboost_amd import freeu as F
    F.check_count(parser, args)
    if args.skip_gen:
        for flag, given in (("--freeu", args.freeu is not None), ("--freeu-backbone", args.freeu_backbone is not None)):
            if given:
                raise SystemExit(f"eval_dreambooth.py: {flag} shapes the images the generation stage samples; --skip-gen scores images that "
                                 "exist already")
    try:
        return F.resolve(args.freeu, args.freeu_backbone, args.model)
    except F.FreeUError as e:
        raise SystemExit(f"eval_dreambooth.py: {e}")


def check_args(args):
    """the refusals, before anything touches the device"""
    if not args.skip_gen:
        if not args.model:
            raise SystemExit("eval_dreambooth.py: generating the images needs --model DIR (a local diffusers model directory: unet/, vae/, "
                             "text_encoder/, tokenizer/, scheduler/); pass --skip-gen to score images that exist already")
        from textboost_amd.generate import check_model_dir
        check_model_dir(args.model, "eval_dreambooth.py")
        if args.prompt_batch <= 0:
            raise SystemExit("eval_dreambooth.py: --prompt-batch must be positive")
    unknown = [m for m in args.metric if m not in BUILT_METRICS + ("vqa",)]
    if unknown:
        raise SystemExit(f"eval_dreambooth.py: unknown --metric {unknown}")
    missing = [m for m in args.metric if m not in BUILT_METRICS and not (m == "vqa" and args.vqa_model)]
    if missing:
        raise SystemExit(f"eval_dreambooth.py: --metric {' '.join(missing)} is not built (only CLIP-T, CLIP-I and DINO are); "
                         "pass --metric clip-t clip-i dino, or some of them.  The VQA score is built with --vqa-model DIR (a local "
                         "clip-flant5 directory) and --clip-model DIR")
    if "vqa" in args.metric and not args.clip_model:
        raise SystemExit("eval_dreambooth.py: --metric vqa needs --clip-model DIR (a local CLIPModel directory): the VQA model's vision tower "
                         "is CLIP ViT-L/14@336px")
    if "dino" in args.metric and not args.dino_model:
        raise SystemExit("eval_dreambooth.py: --metric dino needs --dino-model PATH (the hub's dinov2_vitl14_pretrain.pth or a local "
                         "Dinov2Model directory)")
    if any(m in args.metric for m in ("clip-t", "clip-i")) and not args.clip_model:
        raise SystemExit("eval_dreambooth.py: --clip-model DIR (a local CLIPModel directory) is required for clip-t / clip-i")
    if args.batch_size <= 0:
        raise SystemExit("eval_dreambooth.py: --batch-size must be positive")


def image_root(args) -> str:
    """eval_dreambooth.py `generate()` with --skip-gen"""
    path = args.path.rstrip("/") or args.path
    outdir = args.outdir.rstrip("/") or args.outdir
    base = os.path.basename(path)
    if args.checkpoint is not None:
        base = f"{base}-{args.checkpoint}"
    root = os.path.join(outdir, base)
    if args.output_desc is not None:
        root += f"_{args.output_desc}"
    return root


def csv_path(args) -> str:
    ckpt = f"_ckpt{args.checkpoint}" if args.checkpoint is not None else "_last"
    desc = f"_{args.output_desc}" if args.output_desc is not None else ""
    return os.path.join(args.path.rstrip("/") or args.path, f"metric{ckpt}{desc}.csv")


def generated_images(seed_dir: str, instances: Optional[List[str]]) -> Dict[str, List[str]]:
    """instance -> sorted *.png of seed_dir/<instance>/ (every instance directory there, or the --instances among them)"""
    if not os.path.isdir(seed_dir):
        raise SystemExit(f"eval_dreambooth.py: {seed_dir} does not exist")
    names = sorted(d for d in os.listdir(seed_dir) if os.path.isdir(os.path.join(seed_dir, d)))
    if instances is not None:
        names = [n for n in names if n in instances]
    out = {n: sorted(glob.glob(os.path.join(seed_dir, n, "*.png"))) for n in names}
    out = {n: v for n, v in out.items() if v}
    if not out:
        raise SystemExit(f"eval_dreambooth.py: no generated images under {seed_dir}/<instance>/*.png")
    return out


def real_images(root: str, instances, flag: str) -> Dict[str, List[str]]:
    """instance -> sorted real images `root/<instance>/*.*` (eval_dreambooth.py:389-390); every instance must have some"""
    out = {}
    for inst in instances:
        files = sorted(f for f in glob.glob(os.path.join(root, inst, "*.*")) if os.path.isfile(f))
        if not files:
            raise SystemExit(f"eval_dreambooth.py: no images for instance {inst!r} in {flag} {root}")
        out[inst] = files
    return out


def parse_n_seen(path: str) -> int:
    """N, the number of seen real images per instance: eval_dreambooth.py:496 `int(args.path.split("-")[2].split("n")[-1])` on the path that
    `main` left (one trailing '/' removed), e.g. `out/tb-sd15-n1` -> 1"""
    p = path[:-1] if path.endswith("/") else path
    try:
        n = int(p.split("-")[2].split("n")[-1])
    except (IndexError, ValueError):
        raise SystemExit(f"eval_dreambooth.py: --metric dino takes N (the seen real images per instance) from the run path as the reference "
                         f"does, `<name>-<model>-n<N>` with N after the second '-' (e.g. out/tb-sd15-n1); cannot parse {path!r}") from None
    if n < 1:
        raise SystemExit(f"eval_dreambooth.py: --metric dino: N = {n} seen real images (from {path!r}); it must be at least 1")
    return n


def dreambooth_images(root: str, instances, n_seen: int) -> Dict[str, List[str]]:
    """instance -> its real images: `sorted(glob(<root>/**/*.*))` (eval_dreambooth.py:467; without recursive=True `**` matches one directory
    level) grouped by parent directory.  Every instance in use needs more than N of them: the first N are the seen ones, the rest the unseen."""
    by_instance: Dict[str, List[str]] = {}
    for f in sorted(glob.glob(os.path.join(root, "*", "*.*"))):
        if os.path.isfile(f):
            by_instance.setdefault(os.path.basename(os.path.dirname(f)), []).append(f)
    for inst in instances:
        n = len(by_instance.get(inst, []))
        if n == 0:
            raise SystemExit(f"eval_dreambooth.py: no images for instance {inst!r} in --dreambooth-path {root}")
        if n <= n_seen:
            raise SystemExit(f"eval_dreambooth.py: instance {inst!r} has {n} real images in --dreambooth-path {root}; DINO needs more than "
                             f"N = {n_seen} (the first N are seen, the rest unseen)")
    return {inst: by_instance[inst] for inst in instances}


def format_row(seed, scores: Dict[str, "object"]) -> List[str]:
    """eval_dreambooth.py:620-626: the seed, then every metric's mean as %.3f (0.000 for one that was not asked for)"""
    row = [str(seed)]
    for k in METRIC_KEYS:
        v = scores.get(k)
        row.append(f"{float(v.float().mean().item()) if v is not None else 0.0:.3f}")
    return row


def clip_i_means(gen_emb: Dict[str, "object"], real_emb: Dict[str, "object"]):
    """concatenated max(cos, 0) over instances (eval_dreambooth.py:426-449)"""
    import torch
    from textboost_amd.clip_score import clip_i_scores
    return torch.cat([clip_i_scores(gen_emb[k], real_emb[k]) for k in gen_emb])


def split_by_instance(emb, table: Dict[str, List[str]], instances) -> Dict[str, "object"]:
    """rows of `emb` in the order of [p for i in instances for p in table[i]] -> instance -> its rows"""
    out, off = {}, 0
    for i in instances:
        out[i] = emb[off:off + len(table[i])]
        off += len(table[i])
    return out


def dino_means(gen_emb: Dict[str, "object"], real_emb: Dict[str, "object"], n_seen: int):
    """(seen, unseen) per generated image, concatenated over instances (eval_dreambooth.py:512-537)"""
    import torch
    from textboost_amd.dino_score import dino_scores
    pairs = [dino_scores(gen_emb[k], real_emb[k], n_seen) for k in gen_emb]
    return torch.cat([p[0] for p in pairs]), torch.cat([p[1] for p in pairs])


def evaluate(args, evaluator=None, dino_evaluator=None, vqa_evaluator=None):
    """-> {seed: {metric: per-sample scores}}; writes the CSV."""
    from textboost_amd.clip_score import CLIPEvaluator, clip_t_scores, prompt_of
    root = image_root(args)
    per_seed = {s: generated_images(os.path.join(root, f"seed{s}"), args.instances) for s in args.seeds}
    instances = sorted({i for g in per_seed.values() for i in g})
    seen = unseen = db = None
    if "clip-i" in args.metric:
        seen = real_images(args.train_dir, instances, "--train-dir")
        unseen = real_images(args.val_dir, instances, "--val-dir")
    if "dino" in args.metric:
        n_seen = parse_n_seen(args.path)
        db = dreambooth_images(args.dreambooth_path, instances, n_seen)
    ev = dev = None
    if any(m in args.metric for m in ("clip-t", "clip-i")):
        ev = evaluator or CLIPEvaluator(args.clip_model, batch_size=args.batch_size)
    if db is not None:
        from textboost_amd.dino_score import DINOEvaluator
        dev = dino_evaluator or DINOEvaluator(args.dino_model, batch_size=args.batch_size)
    vev = None
    if "vqa" in args.metric:
        from textboost_amd.vqa_score import VQAEvaluator
        vev = vqa_evaluator or VQAEvaluator(args.vqa_model, args.clip_model, batch_size=args.batch_size)
    real_emb = {}
    if seen is not None:   # every real image once per run (the reference encodes them again for every seed)
        for name, table in (("seen", seen), ("unseen", unseen)):
            real_emb[name] = split_by_instance(ev.encode_images([p for i in instances for p in table[i]], clip_i=True), table, instances)
    dino_real = None
    if db is not None:   # every real image once per run (the reference encodes them again for every seed)
        dino_real = split_by_instance(dev.encode_images([p for i in instances for p in db[i]]), db, instances)
    results = {}
    for s in args.seeds:
        gen = per_seed[s]
        paths = [p for i in sorted(gen) for p in gen[i]]
        scores = {}
        if "clip-t" in args.metric:
            scores["clip_score"] = clip_t_scores(ev.encode_images(paths, clip_i=False), ev.encode_texts([prompt_of(p) for p in paths]))
            print(f"[seed {s}] CLIP-T: {scores['clip_score'].mean():.3f} +/- {scores['clip_score'].std():.3f} ({len(paths)} images)")
        if vev is not None:
            scores["vqa_score"] = vev.score_paths(paths, [prompt_of(p) for p in paths])
            print(f"[seed {s}] VQA score: {scores['vqa_score'].mean():.3f} +/- {scores['vqa_score'].std():.3f} ({len(paths)} images)")
            if s == args.seeds[-1]:
                vev.release()   # 22 GB of weights at full size: freed as soon as the last seed is scored
        if "clip-i" in args.metric:
            gen_emb = split_by_instance(ev.encode_images(paths, clip_i=True), gen, sorted(gen))
            scores["clip_i"] = clip_i_means(gen_emb, real_emb["seen"])
            scores["clip_i_unseen"] = clip_i_means(gen_emb, real_emb["unseen"])
            print(f"[seed {s}] CLIP-I (seen): {scores['clip_i'].mean():.3f}  CLIP-I (unseen): {scores['clip_i_unseen'].mean():.3f}")
        if dino_real is not None:
            scores["dino"], scores["dino_unseen"] = dino_means(split_by_instance(dev.encode_images(paths), gen, sorted(gen)), dino_real, n_seen)
            print(f"[seed {s}] DINO (seen): {scores['dino'].mean():.3f}  DINO (unseen): {scores['dino_unseen'].mean():.3f}")
        results[s] = scores
    out = csv_path(args)
    with open(out, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["seed"] + list(METRIC_KEYS))
        for s in args.seeds:
            w.writerow(format_row(s, results[s]))
    if ev is not None:
        print(f"image tower: {ev.tower_images} images, {ev.images_per_second():.1f} images/s ({ev.geo.image_size} px, batch {ev.batch_size})")
    if dev is not None:
        print(f"DINO tower: {dev.tower_images} images, {dev.images_per_second():.1f} images/s ({dev.geo.image_size} px, batch {dev.batch_size})")
    if vev is not None:
        print(f"VQA model: {vev.images} images, {vev.images_per_second():.1f} images/s (batch {vev.batch_size})")
    print(f"wrote {out}")
    return results


def generate(args):
    """eval_dreambooth.py `generate()` without --skip-gen: the PNGs under `image_root(args)`"""
    from textboost_amd.generate import generate_run, select_instances
    path = args.path.rstrip("/") or args.path
    try:
        instances = select_instances(path, args.instances)
    except SystemExit as e:
        raise SystemExit(f"eval_dreambooth.py: {e}") from None
    return generate_run(path, args.model, instances, args.seeds, image_root(args), checkpoint=args.checkpoint, token_format=args.token_format,
                        prompt_batch=args.prompt_batch, freeu=getattr(args, "freeu_factors", None))


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    args.freeu_factors = check_freeu_args(parser, args)
    check_args(args)
    if not args.skip_gen:
        generate(args)
    return evaluate(args)


if __name__ == "__main__":
    main()
