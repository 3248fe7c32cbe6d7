#!/usr/bin/env python3
"""Images of one prompt from a trained output directory: the reference's inference.py with its flags, on the HIP executors of
textboost_amd/generate.py.

    python inference.py <output_dir> --model <diffusers model dir> --prompt "photo of a <dog> dog" [--seeds 0 1 2 3] [--output grid.jpg]
        [--checkpoint N] [--with <output_dir> ...] [--weights W ...]
        [--init-image photo.jpg [--strength S] [--mask mask.png | --mask auto:WORD [--dilate PX]] [--no-paste]]
        [--region "WORDS=x0,y0,x1,y1" | --region "WORDS=@mask.png" ...] [--region-steps F]
        [--edit-prompt TEXT] [--reweight WORD=F ...] [--cross-steps F] [--self-steps F]
        [--invert-image photo.jpg [--invert-guidance G] [--mask mask.png [--no-paste]]]
        [--excite WORD [WORD ...] [--excite-steps F] [--excite-scale S] [--excite-loss-scale V] [--no-excite-refine]]
        [--blend WORD [WORD ...] [--blend-start F] [--blend-threshold T]]
        [--width PX] [--height PX] [--window-stride CELLS]
        [--freeu [B1 B2 S1 S2]] [--freeu-backbone scalar|structure]

`<output_dir>` is read as eval_dreambooth.py reads it (text_encoder/ adapter, every `<token>.bin`) and, beyond the reference, with the UNet
cross-attention K/V adapters of a `--unet_params_to_train crossattn_kv` run (`<output_dir>/unet/`) folded into the UNet; the text encoder is the plain CLIP text model
(no null-embedding pins: the reference's pipeline here holds a `CLIPTextModel`, inference.py:47-52), one latent PER SEED, the pipeline's default
50 steps at guidance 7.5 with DPM-Solver++.  With --output the images form one grid (1 x len(seeds)); without it each is written to
`<prompt with _ for spaces>_<seed>.jpg` in the working directory.

--with DIR [DIR ...] composes further trained output directories with `<output_dir>` (textboost_amd/compose.py): a subject run and a style
run trained with --mixing, "a <dog> dog in <watercolor> style".  Adapters add (`--weights W ...`, one per run including `<output_dir>`, default
1 each; a run at weight 0 lends its tokens only), tokens are the union; a token that several runs hold keeps the first run's vector, and a
prompt that uses such a token is refused as ambiguous.  --checkpoint N applies to `<output_dir>` only: give `.../checkpoint-N` in --with.  One
line per run (rank, which lora_B rows it uses, weight, UNet adapters) and one on whether the adapters are disjoint are printed first.

--attn-map [WORD ...] also writes where each word lands in the images (textboost_amd/attn_maps.py: the UNet's cross-attention from image
positions to prompt tokens, averaged over heads, layers and steps of the conditional half): `<output stem>_attn.jpg`, one row of overlays per
word and one column per seed, and `<output stem>_attn.npz` with `maps` fp32 [seeds, words, h, w], `words` and `seeds`; without --output one
`<prompt>_<seed>_attn.jpg` / `.npz` pair per seed.  Without a word the placeholder tokens (of all composed runs) that occur in the prompt are taken.  The images
themselves do not change.

--init-image FILE edits a photo instead of starting from noise (textboost_amd/edit.py; diffusers' img2img pipeline and, with
--mask, the latent blend of its inpaint pipeline for a 4-channel UNet): the photo gets a training image's geometry (short edge to the model's
resolution with Lanczos, centre crop), is encoded once by the VAE encoder (the distribution's mode) and noised to the level --strength S in
(0, 1] selects (default 0.8): the last int(steps * S) steps run, each seed's latent being its image's noise.  --mask FILE (the photo's size;
white = repaint) keeps everything else: after every step the unmasked latent cells are reset to the photo's at that noise level, and the
decoded region is pasted into the prepared photo, so pixels outside the mask are the photo's bytes (--no-paste writes the plain decode).  One
photo and one mask serve all --seeds; --with, --weights, --checkpoint and --attn-map work as before.  --mask auto:WORD makes the mask from the
photo instead of reading a file (textboost_amd/auto_mask.py): where WORD ("sofa", "dog") attends in the noised photo, on the
pipeline's own UNet (2 x seeds rows, all conditional) with the run's text encoder, thresholded by Otsu's method at the photo's size and grown
by --dilate PX pixels; it is also written as `<output stem>_mask.png`.  A mask without a white pixel ends the run: nothing would be edited.

--region "WORDS=x0,y0,x1,y1" (repeatable, at most 32) confines words of the prompt to a part of the picture (textboost_amd/regions.py,
DESIGN.md 19): `--prompt "a <dog> dog and a <cat> cat" --region "<dog> dog=0,0,0.5,1" --region "<cat> cat=0.5,0,1,1"` puts the dog on the left
and the cat on the right.  WORDS are one or more space-separated words of the prompt; in every cross-attention layer their tokens are then
visible only to the image positions inside the box (fractions of the image, 0 <= x0 < x1 <= 1; a latent cell is inside if its centre is),
all other tokens stay global, and the unconditional half of the guidance batch is untouched.  `WORDS=@mask.png` takes a picture of any
size instead of a box (resized to the latent grid, white = inside).  --region-steps F in (0, 1] lets the regions act on the first
ceil(F * executed steps) steps only (default: all).  `<output stem>_regions.png` shows the regions as flat colours at the image's size.
Works with --with and with --init-image / --mask; not with --attn-map (the recorder recomputes an unmasked softmax and would report
attention that did not happen).

--edit-prompt TEXT changes the prompt and keeps the picture (textboost_amd/p2p.py; Prompt-to-Prompt, Hertz et al. 2022):
`--prompt "a photo of a dog on a beach" --edit-prompt "a photo of a <dog> dog on a beach"` generates both prompts side by side from each
seed's latent; for the first --cross-steps F of the steps (default 0.8) the edited image's cross-attention reuses the source image's
probabilities for the words the prompts share (a swapped word takes the place of the word it replaces, an added word attends on its own),
and for the first --self-steps F (default 0.4) its self-attention on the coarse maps (a quarter of the latent side and smaller) reuses the
source's maps.  --reweight WORD=F (repeatable, 0 <= F <= 10) multiplies the attention to a word of the edit prompt; with only --reweight
the edit prompt is the prompt.  The output is a 2 x seeds grid, the source row on top and the edited row below (without --output the edited
images are written as `<edit prompt>_<seed>_edit.jpg`).  Both prompts go through one text-encoder call.  Works with --with; not with
--init-image (a photo has to be inverted first: --invert-image, below), --region or --attn-map (the recorder recomputes its own softmax and would report
attention that did not happen).  The default fractions are the paper's; they have not been measured on pretrained weights here.

--invert-image FILE edits a real photo by its prompt: `--invert-image photo.jpg --prompt "a photo of a dog on a beach"
--edit-prompt "a photo of a <dog> dog on a beach"` puts the trained dog into THIS photo.  --prompt describes the photo.  The photo is prepared
and encoded as for --init-image (the mode, so the run is deterministic), walked up the noise schedule under --prompt (DDIM inversion, --steps
UNet calls at guidance --invert-guidance G, default 1), and the prompt-to-prompt edit then runs from the noise it arrives at, the source row
being held on the photo's own trajectory: it ends as the photo's latents exactly.  The output is a 2 x 1 grid, the VAE round trip of the
prepared photo on top and the edit below (without --output: `<prompt>_inv.jpg` and `<edit prompt>_inv_edit.jpg`); --seeds is not read.
--mask FILE (the photo's size, white = repaint) keeps the latent cells outside it on the photo's trajectory in the edited row as well, and the
photo's bytes are pasted outside the mask (--no-paste writes the plain decode).  --reweight, --cross-steps, --self-steps, --with work as with
--edit-prompt.  Not with --init-image, --strength, --region, --attn-map, --mask auto:WORD or --dilate, and not on a v-prediction model.

--excite WORD [WORD ...] keeps every named subject in the image (textboost_amd/excite.py; Attend-and-Excite, Chefer et al.
2023): `--with out/cat --prompt "a <dog> dog and a <cat> cat" --excite "<dog>" "<cat>"`.  During the first --excite-steps F of the steps
(default 0.5) every step first nudges the latents down the gradient of a loss on the 16 x 16 cross-attention maps (the level-2 maps: a quarter
of the latent side) until every word owns at least one strongly attended patch, with the step size --excite-scale S (default 20) times
sqrt(1 - 0.5 i / (steps - 1)); at the steps 0, floor(0.2 steps) and floor(0.4 steps) the nudge repeats, at most 20 times, until each image's
loss is below 0.05 / 0.5 / 0.8 (--no-excite-refine: one nudge per step).  The 16-bit backward carries the loss times --excite-loss-scale V
(default 256).  Words resolve as for --attn-map; at most 8 words of at most 16 token positions each.  `<output stem>_excite.json` reports,
per guided step and seed, the loss before (and, at the refinement steps, after) the nudges, the worst word, the number of nudges and the
updates skipped because the gradient was not finite.  Works with --with (its main use); not with --region, --edit-prompt, --reweight,
--invert-image, --init-image, --mask or --attn-map.  The defaults are the paper's; they have not been measured on pretrained weights here.

--blend WORD [WORD ...] keeps an edit where it belongs (textboost_amd/local_blend.py; Prompt-to-Prompt's LocalBlend): with
--edit-prompt / --reweight, `--prompt "a photo of a dog on a beach" --edit-prompt "a photo of a <dog> dog on a beach" --blend dog "<dog>"`
swaps the subject and leaves the beach alone.  Every step adds the 16 x 16 cross-attention maps (level 2, as --excite) of both prompts' rows to
an accumulator; after every solver step from floor(--blend-start F * steps) on (default 0.2) the edited image's latents are set back to the
source image's, except where the 3 x 3 max-pooled map of the words exceeds --blend-threshold T (default 0.3) times its maximum, in either
prompt.  Every word is looked up in both prompts and must occur in at least one.  With --invert-image the source row is the photo, and a
--mask FILE limits the blend mask further.  `<output stem>_blend.png` shows the final masks (one tile per seed, white = edited) and
`<output stem>_blend.json` the words' token positions in each prompt and the masks' areas; an empty final mask is a printed warning.  Works
with --with.  The defaults are the published ones; they have not been measured on pretrained weights here.

--width PX / --height PX make a banner, a panorama or a portrait-format picture (textboost_amd/canvas.py; MultiDiffusion, Bar-Tal
et al. 2023): `--width 2048` on an SD1.x model writes 2048 x 512 images.  The UNet is not run at that shape: the large latent is denoised as
overlapping windows of the model's own size, --window-stride CELLS latent cells apart (default a quarter of the model's latent side: 13 windows
for 2048 pixels at SD1.x), whose noise predictions are averaged where they overlap before the ONE solver step of the whole canvas; the result is
decoded as VAE tiles that are feathered where they overlap.  Either flag alone leaves the other side at the model's size; sides are multiples
of the VAE's factor, at least the model's size and at most 8192 pixels.  All windows share --prompt.  --with, --weights and --checkpoint work as
before.  Not with --init-image, --mask, --invert-image, --edit-prompt, --reweight, --region, --excite, --attn-map or --blend: each of them
places things on the model's own grid.  The paper's stride is 8 cells; the default here is a cost choice and has not been measured on pretrained
weights.

--freeu [B1 B2 S1 S2] turns FreeU on (textboost_amd/freeu.py; Si et al. 2024): in the first two decoder stages the first half of
the backbone channels is amplified (B1, B2) and the lowest spatial frequencies of the skip features are damped (S1, S2), one in-place kernel
launch in front of each of their resnets.  Without values the constants of the FreeU authors' README apply, chosen by the UNet's
cross_attention_dim (768, SD1.x: 1.5 1.6 0.9 0.2; 1024, SD2.x: 1.4 1.6 0.9 0.2; they have not been measured here); another model needs the
four values.  --freeu-backbone structure scales by (B - 1) n + 1, n the image's min-max normalised channel mean, instead of by B.  Values are
finite and > 0; `--freeu 1 1 1 1` is the plain image.  Give the flag behind `<output_dir>`.  It goes with every forward-only path above
(an --invert-image inversion and the generation run the same FreeU model; a --mask auto:WORD mask is made by the plain model), not with
--excite, which needs the UNet's backward: FreeU works in place and keeps nothing for one.

Differences from the reference: --model is a local diffusers model directory (the reference's alias handling raises KeyError); --checkpoint N
reads `<output_dir>/checkpoint-N` (the reference parses the flag and ignores it); --outdir and --skip-gen are accepted and unused, as there; the
latent of a seed is drawn on the CPU (textboost_amd.generate.seeded_latent), the same on every machine."""
from __future__ import annotations

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


DEFAULT_STRENGTH = 0.8


def build_parser():
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("path", type=str, help="path to model")
    p.add_argument("--model", type=str, default=None, help="local diffusers model directory")
    p.add_argument("--prompt", type=str, default="photo of a <dog> dog")
    p.add_argument("--outdir", type=str, default="./benchmarks")
    p.add_argument("--checkpoint", type=int, default=None)
    p.add_argument("--skip-gen", action="store_true")
    p.add_argument("--seeds", type=int, nargs="+", default=[0, 1, 2, 3])
    p.add_argument("--output", type=str, default=None)
    p.add_argument("--steps", type=int, default=50, help="sampling steps (the pipeline's default)")
    p.add_argument("--attn-map", dest="attn_map", type=str, nargs="*", default=None, metavar="WORD",
                   help="also write token attention maps of these words of the prompt (no word: the run's placeholder tokens in the prompt)")
    p.add_argument("--with", dest="with_runs", type=str, nargs="+", default=None, metavar="DIR",
                   help="further trained output directories composed with `path` (subject x style)")
    p.add_argument("--weights", type=float, nargs="+", default=None, metavar="W",
                   help="adapter weight per run, `path` first (default: 1 each)")
    p.add_argument("--init-image", dest="init_image", type=str, default=None, metavar="FILE",
                   help="edit this photo instead of starting from noise (one photo for all --seeds)")
    p.add_argument("--strength", type=float, default=None, metavar="S",
                   help=f"with --init-image: how much of the schedule runs, in (0, 1] (default {DEFAULT_STRENGTH})")
    p.add_argument("--mask", type=str, default=None, metavar="FILE",
                   help="with --init-image: repaint only where this picture (same size as the photo) is white; auto:WORD makes the mask from "
                        "the photo: where WORD attends in it")
    p.add_argument("--dilate", type=int, default=None, metavar="PX",
                   help="with --mask auto:WORD: grow the mask by a square of this radius in the photo's pixels (default 0)")
    p.add_argument("--no-paste", dest="no_paste", action="store_true",
                   help="with --mask: write the plain decode instead of pasting the repainted region into the photo")
    p.add_argument("--region", dest="region", type=str, action="append", default=None, metavar="WORDS=BOX",
                   help="confine these words of the prompt to a box x0,y0,x1,y1 (fractions of the image) or to @mask.png; repeatable")
    p.add_argument("--region-steps", dest="region_steps", type=float, default=None, metavar="F",
                   help="with --region: the regions act on the first ceil(F * executed steps) steps, 0 < F <= 1 (default 1)")
    p.add_argument("--edit-prompt", dest="edit_prompt", type=str, default=None, metavar="TEXT",
                   help="also generate this prompt from the same noise, keeping the layout of --prompt's image (prompt-to-prompt)")
    p.add_argument("--cross-steps", dest="cross_steps", type=float, default=None, metavar="F",
                   help="with --edit-prompt / --reweight: cross-attention control on the first floor(F * steps) steps, 0 <= F <= 1 (default 0.8)")
    p.add_argument("--self-steps", dest="self_steps", type=float, default=None, metavar="F",
                   help="with --edit-prompt / --reweight: self-attention control on the first floor(F * steps) steps, 0 <= F <= 1 (default 0.4)")
    p.add_argument("--reweight", dest="reweight", type=str, action="append", default=None, metavar="WORD=F",
                   help="multiply the attention to this word of the edit prompt by F, 0 <= F <= 10; repeatable")
    p.add_argument("--invert-image", dest="invert_image", type=str, default=None, metavar="FILE",
                   help="with --edit-prompt / --reweight: edit this photo; --prompt describes it, the photo is inverted to noise first")
    p.add_argument("--invert-guidance", dest="invert_guidance", type=float, default=None, metavar="G",
                   help="with --invert-image: guidance scale of the inversion, finite and >= 0 (default 1)")
    p.add_argument("--excite", dest="excite", type=str, nargs="+", default=None, metavar="WORD",
                   help="Attend-and-Excite: nudge the latents during the first steps until each of these words of the prompt owns a strongly "
                        "attended patch (at most 8 words)")
    p.add_argument("--excite-steps", dest="excite_steps", type=float, default=None, metavar="F",
                   help="with --excite: the guidance acts on the first floor(F * steps) steps, 0 <= F <= 1 (default 0.5)")
    p.add_argument("--excite-scale", dest="excite_scale", type=float, default=None, metavar="S",
                   help="with --excite: the step size factor, > 0 (default 20)")
    p.add_argument("--excite-loss-scale", dest="excite_loss_scale", type=float, default=None, metavar="V",
                   help="with --excite: the factor the 16-bit backward carries the loss with, > 0 (default 256)")
    p.add_argument("--no-excite-refine", dest="no_excite_refine", action="store_true",
                   help="with --excite: no iterative refinement at the steps 0, floor(0.2 steps), floor(0.4 steps)")
    p.add_argument("--blend", dest="blend", type=str, nargs="+", default=None, metavar="WORD",
                   help="with --edit-prompt / --reweight (LocalBlend): the edited image keeps the source image's latents except where these words "
                        "attend (each word must occur in at least one of the two prompts)")
    p.add_argument("--blend-start", dest="blend_start", type=float, default=None, metavar="F",
                   help="with --blend: blend behind every step from floor(F * steps) on, 0 <= F <= 1 (default 0.2: the published value, not "
                        "measured on pretrained weights here)")
    p.add_argument("--blend-threshold", dest="blend_threshold", type=float, default=None, metavar="T",
                   help="with --blend: a cell is edited where the pooled attention exceeds T times its maximum, finite and >= 0 (default 0.3: "
                        "the published value, not measured on pretrained weights here)")
    p.add_argument("--width", type=int, default=None, metavar="PX",
                   help="image width in pixels: a multiple of the VAE's factor, from the model's size to 8192 (a wider picture is denoised as "
                        "overlapping windows of the model's size: MultiDiffusion)")
    p.add_argument("--height", type=int, default=None, metavar="PX", help="image height in pixels, as --width")
    p.add_argument("--window-stride", dest="window_stride", type=int, default=None, metavar="CELLS",
                   help="with --width / --height: latent cells between neighbouring windows, 1 .. the model's latent side (default a quarter "
                        "of it, 16 at SD1.x, where the paper uses 8: a cost choice, not measured on pretrained weights here)")
    from textboost_amd import freeu as F
    F.add_arguments(p)
    return p


def check_freeu_flags(args):
    """--freeu / --freeu-backbone: every refusal, on the host, by flag name, before any model is built.  -> None or (b1, b2, s1, s2, mode)"""
    from textboost_amd import freeu as F
    if args.freeu is not None and args.excite:
        raise SystemExit("inference.py: --freeu does not go with --excite: the excite pass needs the UNet's backward, and FreeU rewrites the "
                         "decoder's concat inputs in place, so nothing is kept for one")
    try:
        return F.resolve(args.freeu, args.freeu_backbone, args.model)
    except F.FreeUError as e:
        raise SystemExit(f"inference.py: {e}")


MAX_CANVAS_PX = 8192
CANVAS_UNET_BATCH = 13      # image-window pairs per UNet call: the generation batch the kernels are tuned for


def check_canvas_flags(args):
    """--width / --height / --window-stride: every refusal, on the host, before any model is built.  -> None (the model's own square) or
    {"Hc", "Wc": the canvas in latent cells, "stride", "S": the model's latent side, "factor": the VAE's}"""
    import json
    from textboost_amd.canvas import CanvasError, CanvasPlan
    if args.width is None and args.height is None:
        if args.window_stride is not None:
            raise SystemExit("inference.py: --window-stride needs --width PX or --height PX (the canvas whose windows it spaces)")
        return None
    why = {"--init-image": "a photo is prepared and encoded at the model's own size; a canvas-sized photo is not built",
           "--mask": "a mask belongs to --init-image / --invert-image, which the canvas does not go with",
           "--invert-image": "the inversion walks one model-sized latent up the schedule, not a canvas of windows",
           "--edit-prompt": "the prompt-to-prompt control pairs the rows of one UNet batch, and a canvas's windows fill that batch",
           "--reweight": "the prompt-to-prompt control pairs the rows of one UNet batch, and a canvas's windows fill that batch",
           "--region": "a region is a part of the model's own grid; mapping it onto every window of a canvas is not built",
           "--excite": "the excite pass moves the latents of one model-sized image; the windows of a canvas overlap and would be moved apart",
           "--attn-map": "the recorder accumulates maps of the model's own grid; stitching the windows' maps is not built",
           "--blend": "LocalBlend needs --edit-prompt / --reweight, which the canvas does not go with"}
    for flag, given in (("--init-image", args.init_image is not None), ("--mask", args.mask is not None),
                        ("--invert-image", args.invert_image is not None), ("--edit-prompt", args.edit_prompt is not None),
                        ("--reweight", bool(args.reweight)), ("--region", bool(args.region)), ("--excite", bool(args.excite)),
                        ("--attn-map", args.attn_map is not None), ("--blend", bool(args.blend))):
        if given:
            raise SystemExit(f"inference.py: --width / --height do not go with {flag}: {why[flag]}")
    try:
        with open(os.path.join(args.model, "unet", "config.json")) as f:
            S = int(json.load(f).get("sample_size", 64))
        with open(os.path.join(args.model, "vae", "config.json")) as f:
            factor = 1 << (len(json.load(f).get("block_out_channels", [0] * 4)) - 1)
    except OSError as e:
        raise SystemExit(f"inference.py: --width / --height: {e} (--model must be a local diffusers model directory)")
    cells = {}
    for flag, px in (("--width", args.width), ("--height", args.height)):
        px = S * factor if px is None else px
        if px % factor or not S * factor <= px <= MAX_CANVAS_PX:
            raise SystemExit(f"inference.py: {flag} {px}: a multiple of {factor} (the VAE's factor) from {S * factor} (the model's size) to "
                             f"{MAX_CANVAS_PX} pixels")
        cells[flag] = px // factor
    stride = max(1, S // 4) if args.window_stride is None else args.window_stride
    try:
        CanvasPlan(S, cells["--height"], cells["--width"], stride, len(args.seeds), CANVAS_UNET_BATCH)
    except CanvasError as e:
        raise SystemExit(f"inference.py: --window-stride: {e}")
    return {"Hc": cells["--height"], "Wc": cells["--width"], "stride": stride, "S": S, "factor": factor}


def check_blend_flags(args):
    """--blend and its companions: the refusals that need no file, by flag name.  -> is the edit blended?"""
    from textboost_amd import local_blend as B
    if not args.blend:
        for flag, given in (("--blend-start", args.blend_start is not None), ("--blend-threshold", args.blend_threshold is not None)):
            if given:
                raise SystemExit(f"inference.py: {flag} needs --blend WORD [WORD ...] (the words whose attention bounds the edit)")
        return False
    if args.edit_prompt is None and not args.reweight:
        raise SystemExit("inference.py: --blend needs --edit-prompt TEXT or --reweight WORD=F: it blends the edited image of a prompt-to-prompt "
                         "pair against its source image")
    try:
        if args.blend_start is not None:
            B.start_step(args.blend_start, args.steps)
        if args.blend_threshold is not None:
            B.check_threshold(args.blend_threshold)
    except B.BlendError as e:
        raise SystemExit(f"inference.py: {e}")
    return True


def check_blend_args(args, run, p2p, blending):
    """--blend (`blending`: what `check_blend_flags` returned): the words' token positions in both prompts, on the host, before any model is
    built.  -> None or {"words", "source", "edit",
    "found", "start", "threshold"}"""
    from textboost_amd import local_blend as B
    if not blending:
        return None
    from textboost_amd.attn_maps import run_tokenizer
    try:
        tokenizer = run_tokenizer(args.model, run)
    except OSError as e:
        raise SystemExit(f"inference.py: --blend: {e} (--model must be a local diffusers model directory)")
    T = model_text_len(args.model)
    try:
        src, edt, found = B.word_positions(tokenizer, args.prompt, p2p["edit_prompt"], args.blend, T)
        B.position_row(src, T), B.position_row(edt, T)
    except ValueError as e:      # (BlendError is one)
        raise SystemExit(f"inference.py: --blend: {e}")
    return {"words": list(args.blend), "source": src, "edit": edt, "found": found,
            "start": B.START if args.blend_start is None else args.blend_start,
            "threshold": B.THRESHOLD if args.blend_threshold is None else args.blend_threshold}


def blend_stem(args):
    return (os.path.splitext(args.output)[0] if args.output is not None else args.prompt.replace(" ", "_")) + "_blend"


def write_blend(args, bctl, seeds, cell):
    """`<stem>_blend.png`: the final masks, nearest x cell, one tile per seed; `<stem>_blend.json`: the positions and the areas (read once)"""
    import json
    import numpy as np
    from PIL import Image
    stem = blend_stem(args)
    area = None
    if bctl.final_mask is None:
        print(f"--blend: no step was blended (--blend-start {bctl.start:g} of {args.steps} steps): the edit is the plain prompt-to-prompt one")
    else:
        masks, area = bctl.final_mask.cpu().numpy(), bctl.area.cpu().tolist()
        tiles = [np.kron(m, np.ones((cell, cell), dtype=np.uint8)) for m in masks]
        Image.fromarray(np.concatenate(tiles, axis=1)).save(stem + ".png")
        for s, a in zip(seeds, area):
            if a == 0:
                print(f"warning: --blend: the final mask of seed {s} is empty: the edited image is the source image")
    with open(stem + ".json", "w") as f:
        json.dump(dict(bctl.report(area=area, seeds=None), prompt=args.prompt, edit_prompt=args.edit_prompt, seeds=[str(s) for s in seeds]), f,
                  indent=1, sort_keys=True)
    print(f"wrote {stem}.json" + (f" and {stem}.png: {area} of {bctl.h * bctl.w} latent cells edited" if area is not None else ""))


def check_excite_flags(args):
    """--excite and its companions: the refusals that need no file, by flag name.  -> is the generation guided?"""
    from textboost_amd import excite as X
    if not args.excite:
        for flag, given in (("--excite-steps", args.excite_steps is not None), ("--excite-scale", args.excite_scale is not None),
                            ("--excite-loss-scale", args.excite_loss_scale is not None), ("--no-excite-refine", args.no_excite_refine)):
            if given:
                raise SystemExit(f"inference.py: {flag} needs --excite WORD [WORD ...] (the words it keeps in the image)")
        return False
    why = {"--region": "the excite pass moves the latents by the unmasked attention, which the regions then contradict; pin the words with "
                       "--region or excite them, not both",
           "--edit-prompt": "the prompt-to-prompt rows share their latents, which the excite pass would move apart",
           "--reweight": "the prompt-to-prompt rows share their latents, which the excite pass would move apart",
           "--invert-image": "the source row is pinned to the photo's trajectory, which the excite pass would leave",
           "--init-image": "the excite pass is built for a generation from noise, not for the partial schedule of an edited photo",
           "--mask": "a mask belongs to --init-image / --invert-image, which --excite does not go with",
           "--attn-map": "the recorded maps would mix the guided steps' attention with the excite pass's own forwards; run --attn-map without "
                         "--excite"}
    for flag, given in (("--region", bool(args.region)), ("--edit-prompt", args.edit_prompt is not None), ("--reweight", bool(args.reweight)),
                        ("--invert-image", args.invert_image is not None), ("--init-image", args.init_image is not None),
                        ("--mask", args.mask is not None), ("--attn-map", args.attn_map is not None)):
        if given:
            raise SystemExit(f"inference.py: --excite does not go with {flag}: {why[flag]}")
    if len(args.excite) > X.MAX_WORDS:
        raise SystemExit(f"inference.py: --excite takes at most {X.MAX_WORDS} words, not {len(args.excite)}")
    try:
        if args.excite_steps is not None:
            X.guided_steps(args.excite_steps, args.steps)
    except X.ExciteError as e:
        raise SystemExit(f"inference.py: {e}")
    import math
    for flag, v in (("--excite-scale", args.excite_scale), ("--excite-loss-scale", args.excite_loss_scale)):
        if v is not None and not (math.isfinite(v) and v > 0.0):
            raise SystemExit(f"inference.py: {flag} {v}: a finite number > 0")
    return True


def check_excite_args(args, run):
    """--excite: the words' token positions, on the host, before any model is built.  -> None or {"words", "positions", "last", options}"""
    from textboost_amd import excite as X
    if not check_excite_flags(args):
        return None
    from textboost_amd.attn_maps import run_tokenizer, token_positions
    try:
        tokenizer = run_tokenizer(args.model, run)
    except OSError as e:
        raise SystemExit(f"inference.py: --excite: {e} (--model must be a local diffusers model directory)")
    T = model_text_len(args.model)
    positions = []
    for w in args.excite:
        try:
            positions.append(token_positions(tokenizer, args.prompt, w, T))
        except ValueError as e:
            raise SystemExit(f"inference.py: --excite: {e}")
    ids = list(tokenizer(args.prompt, truncation=True, padding="max_length", max_length=T).input_ids)
    last = X.first_eos(ids, tokenizer.eos_token_id)
    try:
        X.word_table(positions, last)
    except X.ExciteError as e:
        raise SystemExit(f"inference.py: {e}")
    return {"words": list(args.excite), "positions": positions, "last": last,
            "steps": X.EXCITE_STEPS if args.excite_steps is None else args.excite_steps,
            "scale": X.SCALE if args.excite_scale is None else args.excite_scale,
            "loss_scale": X.LOSS_SCALE if args.excite_loss_scale is None else args.excite_loss_scale,
            "refine": not args.no_excite_refine}


def excite_path(args):
    stem = os.path.splitext(args.output)[0] if args.output is not None else args.prompt.replace(" ", "_")
    return stem + "_excite.json"


def load_runs(args):
    """`path` [--checkpoint N] and every --with directory, composed (textboost_amd/compose.py); on the host.  Without --with and --weights:
    the one run as read."""
    from textboost_amd import compose as C
    from textboost_amd import generate as G
    path = args.path.rstrip("/") or args.path
    if args.checkpoint is not None:
        path = os.path.join(path, f"checkpoint-{args.checkpoint}")
    paths = [path] + [d.rstrip("/") or d for d in (args.with_runs or [])]
    if args.weights is not None and len(args.weights) != len(paths):
        raise SystemExit(f"inference.py: --weights: {len(args.weights)} weights for {len(paths)} runs (one per run, `path` first)")
    runs = [G.read_run_dir(d) for d in paths]
    if len(runs) == 1 and args.weights is None:
        return runs[0]
    weights = args.weights or [1.0] * len(runs)
    for run in runs:
        if run.use_dora:   # (refused before the per-run report below reads its adapter)
            raise SystemExit(f"inference.py: --with / --weights: {run.path} is a use_dora run, which does not compose; sample it on its own")
    for run, w in zip(runs, weights):
        print(f"run {run.path}: rank {run.rank}, lora_B rows {C.adapter_support(run)}, weight {w:g}, UNet K/V adapters "
              f"{'rank ' + str(run.unet_rank) if run.unet_rank else 'none'}")
    if len(runs) > 1:
        print("the adapters change disjoint output features of q/k/v_proj (--mixing)" if C.disjoint(runs) else
              "the adapters are not disjoint: their deltas overlap and add")
    try:
        run = C.compose_runs(runs, weights)
    except (ValueError, NotImplementedError) as e:
        raise SystemExit(f"inference.py: --with: {e}")
    first = {}
    for r in runs:
        for n, _ in r.tokens:
            first.setdefault(n, r.path)
    for tok, dropped in run.shadowed:
        for what, text in [("--prompt", args.prompt)] + [("--attn-map", w) for w in (args.attn_map or [])] + \
                [("--region", r) for r in (getattr(args, "region", None) or [])] + \
                [("--edit-prompt", t) for t in [getattr(args, "edit_prompt", None)] if t is not None] + \
                [("--reweight", r) for r in (getattr(args, "reweight", None) or [])] + \
                [("--excite", w) for w in (getattr(args, "excite", None) or [])] + \
                [("--blend", w) for w in (getattr(args, "blend", None) or [])]:
            if tok in text:
                raise SystemExit(f"inference.py: {what} {text!r} uses {tok}, which both {first[tok]} and {dropped} hold: ambiguous (the first "
                                 "run's vector would be taken); rename the token in one run or leave it out of the prompt")
    return run


def check_edit_args(args):
    """--init-image / --strength / --mask: every refusal, on the host.  -> None (text-to-image) or {"rgb": uint8 [H, W, 3], "mask": PIL "L" image
    or None, "strength": float, "auto": the word of --mask auto:WORD or None, "dilate": int}"""
    from textboost_amd import auto_mask as A
    from textboost_amd import edit as E
    if args.init_image is None:
        for flag, given in (("--mask", args.mask is not None), ("--strength", args.strength is not None), ("--dilate", args.dilate is not None)):
            if given and not (flag == "--mask" and getattr(args, "invert_image", None) is not None):      # (--invert-image takes a mask file too)
                raise SystemExit(f"inference.py: {flag} needs --init-image FILE (the photo to edit)")
        return None
    strength = DEFAULT_STRENGTH if args.strength is None else args.strength
    try:
        E.strength_begin(args.steps, strength)
    except ValueError as e:
        raise SystemExit(f"inference.py: --strength: {e}")
    try:
        rgb = E.load_rgb(args.init_image)
    except (OSError, ValueError) as e:
        raise SystemExit(f"inference.py: --init-image {args.init_image}: cannot be read as a picture ({e})")
    mask = auto = None
    if args.mask is not None:
        try:
            kind, auto = A.parse_auto_mask(args.mask)
        except ValueError as e:
            raise SystemExit(f"inference.py: --mask {args.mask}: {e}")
        auto = auto if kind == "auto" else None
    if args.dilate is not None and (auto is None or not 0 <= args.dilate <= A.MAX_DILATE):
        raise SystemExit(f"inference.py: --dilate PX goes with --mask auto:WORD, 0 .. {A.MAX_DILATE} pixels")
    if args.mask is not None and auto is None:
        try:
            mask = E.load_mask(args.mask)
        except (OSError, ValueError) as e:
            raise SystemExit(f"inference.py: --mask {args.mask}: cannot be read as a picture ({e})")
        if mask.size != (rgb.shape[1], rgb.shape[0]):
            raise SystemExit(f"inference.py: --mask {args.mask} is {mask.size[0]} x {mask.size[1]}, --init-image {args.init_image} is "
                             f"{rgb.shape[1]} x {rgb.shape[0]}: the mask must have the photo's size")
    try:
        E.check_vae_has_encoder(args.model)
    except (OSError, ValueError) as e:
        raise SystemExit(f"inference.py: --init-image: {e}")
    return {"rgb": rgb, "mask": mask, "strength": strength, "auto": auto, "dilate": args.dilate or 0}


def model_text_len(model_dir):
    import json
    cfg = os.path.join(model_dir, "text_encoder", "config.json")
    if os.path.exists(cfg):
        with open(cfg) as f:
            return json.load(f).get("max_position_embeddings", 77)
    return 77


def check_region_args(args, run, edit):
    """--region / --region-steps: every refusal, on the host, before any model is built.  -> None or {"regions": [regions.Region],
    "steps": executed steps the regions act on, or None for all}"""
    import json
    from textboost_amd import regions as R
    if not args.region:
        if args.region_steps is not None:
            raise SystemExit("inference.py: --region-steps needs --region \"WORDS=x0,y0,x1,y1\"")
        return None
    if args.attn_map is not None:
        raise SystemExit("inference.py: --region does not go with --attn-map: the recorder recomputes an unmasked softmax from q and k, so it "
                         "would report attention that did not happen under the regions; run --attn-map without --region")
    try:
        specs = [R.parse_region(r) for r in args.region]
        with open(os.path.join(args.model, "unet", "config.json")) as f:
            size = int(json.load(f).get("sample_size", 64))
        from textboost_amd.attn_maps import run_tokenizer
        regions = R.resolve_regions(run_tokenizer(args.model, run), args.prompt, model_text_len(args.model), specs, size, size)
        steps = None
        if args.region_steps is not None:
            executed = args.steps
            if edit is not None:
                from textboost_amd.edit import strength_begin
                executed = args.steps - strength_begin(args.steps, edit["strength"])
            steps = R.steps_for(args.region_steps, executed)
    except R.RegionError as e:
        raise SystemExit(f"inference.py: {e}")
    except OSError as e:
        raise SystemExit(f"inference.py: --region: {e} (--model must be a local diffusers model directory)")
    return {"regions": regions, "steps": steps}


def check_p2p_flags(args):
    """--edit-prompt / --reweight / --cross-steps / --self-steps: the refusals that need no file, by flag name.  -> is this an edit?"""
    from textboost_amd import p2p as P
    editing = args.edit_prompt is not None or bool(args.reweight)
    if not editing:
        for flag, given in (("--cross-steps", args.cross_steps is not None), ("--self-steps", args.self_steps is not None)):
            if given:
                raise SystemExit(f"inference.py: {flag} needs --edit-prompt TEXT or --reweight WORD=F (the edit it controls)")
        return False
    flag = "--edit-prompt" if args.edit_prompt is not None else "--reweight"
    if args.init_image is not None:
        raise SystemExit(f"inference.py: {flag} does not go with --init-image: editing a photo by its prompt would need the photo inverted to "
                         "noise first, which is not built; use --init-image with --mask, or generate the source from a seed")
    if args.region:
        raise SystemExit(f"inference.py: {flag} does not go with --region: both take over the cross-attention launch")
    if args.attn_map is not None:
        raise SystemExit(f"inference.py: {flag} does not go with --attn-map: the recorder recomputes its own softmax from q and k, so it would "
                         "report attention that did not happen under the control")
    try:
        for name, f in (("--cross-steps", args.cross_steps), ("--self-steps", args.self_steps)):
            if f is not None:
                P.steps_for(f, args.steps, name)
        for r in args.reweight or []:
            P.parse_reweight(r)
    except P.P2PError as e:
        raise SystemExit(f"inference.py: {e}")
    return True


def check_invert_flags(args):
    """--invert-image / --invert-guidance: the refusals that need no file, by flag name.  -> is this an inversion?"""
    import math
    if args.invert_image is None:
        if args.invert_guidance is not None:
            raise SystemExit("inference.py: --invert-guidance needs --invert-image FILE (the photo whose inversion it guides)")
        return False
    if args.edit_prompt is None and not args.reweight:
        raise SystemExit("inference.py: --invert-image needs --edit-prompt TEXT or --reweight WORD=F: the photo is inverted to be edited by its "
                         "prompt (--prompt describes the photo); to restyle a photo without a second prompt use --init-image")
    why = {"--init-image": "a photo is either inverted or noised to a strength, not both",
           "--strength": "the inversion walks the whole schedule; a strength belongs to --init-image",
           "--region": "the edit's control and the regions both take over the cross-attention launch",
           "--attn-map": "the recorder recomputes its own softmax from q and k, so it would report attention that did not happen under the control",
           "--dilate": "it grows the mask of --mask auto:WORD, which is not built for an inverted photo"}
    for flag, given in (("--init-image", args.init_image is not None), ("--strength", args.strength is not None), ("--region", bool(args.region)),
                        ("--attn-map", args.attn_map is not None), ("--dilate", args.dilate is not None)):
        if given:
            raise SystemExit(f"inference.py: --invert-image does not go with {flag}: {why[flag]}")
    if args.mask is not None and args.mask.startswith("auto:"):
        raise SystemExit(f"inference.py: --invert-image does not go with --mask {args.mask}: the mask maker noises the photo to one level and is "
                         "not built for an inverted one; paint a mask and pass --mask FILE")
    g = args.invert_guidance
    if g is not None and not (math.isfinite(g) and g >= 0.0):
        raise SystemExit(f"inference.py: --invert-guidance {g}: a finite number >= 0 (1 inverts under the prompt alone)")
    return True


def check_invert_args(args):
    """--invert-image: the refusals that read files, on the host, before any model is built.  -> None or {"rgb": uint8 [H, W, 3], "mask": PIL "L"
    image or None, "guidance": float}"""
    import json
    from textboost_amd import edit as E
    if not check_invert_flags(args):
        return None
    cfg = os.path.join(args.model, "scheduler", "scheduler_config.json")
    if os.path.exists(cfg):
        with open(cfg) as f:
            pred = json.load(f).get("prediction_type", "epsilon")
        if pred != "epsilon":
            raise SystemExit(f"inference.py: --invert-image: {cfg} says prediction_type {pred!r}; inversion is built for epsilon models only (a v "
                             "output would have to be converted with the scalars of the level its input is on, which an inversion step is one "
                             "level off); SD1.x and SD2.1-base are epsilon models")
    try:
        rgb = E.load_rgb(args.invert_image)
    except (OSError, ValueError) as e:
        raise SystemExit(f"inference.py: --invert-image {args.invert_image}: cannot be read as a picture ({e})")
    mask = None
    if args.mask is not None:
        try:
            mask = E.load_mask(args.mask)
        except (OSError, ValueError) as e:
            raise SystemExit(f"inference.py: --mask {args.mask}: cannot be read as a picture ({e})")
        if mask.size != (rgb.shape[1], rgb.shape[0]):
            raise SystemExit(f"inference.py: --mask {args.mask} is {mask.size[0]} x {mask.size[1]}, --invert-image {args.invert_image} is "
                             f"{rgb.shape[1]} x {rgb.shape[0]}: the mask must have the photo's size")
    try:
        E.check_vae_has_encoder(args.model)
    except (OSError, ValueError) as e:
        raise SystemExit(f"inference.py: --invert-image: {e}")
    return {"rgb": rgb, "mask": mask, "guidance": 1.0 if args.invert_guidance is None else args.invert_guidance}


def check_p2p_args(args, run):
    """the token plan, on the host, before any model is built.  -> None or {"plan": p2p.P2PPlan, "edit_prompt": str, "cross": F, "self": F}"""
    from textboost_amd import p2p as P
    if not check_p2p_flags(args):
        return None
    edit_prompt = args.prompt if args.edit_prompt is None else args.edit_prompt
    try:
        from textboost_amd.attn_maps import run_tokenizer
        pl = P.plan(run_tokenizer(args.model, run), args.prompt, edit_prompt, model_text_len(args.model), [P.parse_reweight(r) for r in args.reweight or []])
    except P.P2PError as e:
        raise SystemExit(f"inference.py: {e}")
    except OSError as e:
        raise SystemExit(f"inference.py: --edit-prompt: {e} (--model must be a local diffusers model directory)")
    return {"plan": pl, "edit_prompt": edit_prompt, "cross": P.CROSS_STEPS if args.cross_steps is None else args.cross_steps,
            "self": P.SELF_STEPS if args.self_steps is None else args.self_steps}


def regions_path(args):
    stem = os.path.splitext(args.output)[0] if args.output is not None else args.prompt.replace(" ", "_")
    return stem + "_regions.png"


def check_auto_mask(pixel_mask, word):
    """the prepared pixel mask of --mask auto:WORD must repaint something: an all-black one would write the photo back unedited"""
    if not pixel_mask.any():
        raise SystemExit(f"inference.py: --mask auto:{word}: the mask has no white pixel inside the prepared photo (the attention to {word!r} "
                         "is flat, or its region lies outside the centre crop): nothing would be edited; paint a mask and pass --mask FILE")


def auto_mask_path(args):
    stem = os.path.splitext(args.output)[0] if args.output is not None else args.prompt.replace(" ", "_")
    return stem + "_mask.png"


def attn_map_words(model_dir, run, prompt, requested):
    """--attn-map: (words, their token positions in the tokenised prompt), on the host.  No word: the run's placeholder tokens that occur in the
    prompt.  A word that does not occur is a SystemExit."""
    import json
    from textboost_amd.attn_maps import run_tokenizer, token_positions
    tokenizer = run_tokenizer(model_dir, run)
    T = 77
    cfg = os.path.join(model_dir, "text_encoder", "config.json")
    if os.path.exists(cfg):
        with open(cfg) as f:
            T = json.load(f).get("max_position_embeddings", 77)
    words, positions = [], []
    if requested:
        for w in requested:
            try:
                positions.append(token_positions(tokenizer, prompt, w, T))
            except ValueError as e:
                raise SystemExit(f"inference.py: --attn-map: {e}")
            words.append(w)
        return words, positions
    for w, _ in run.tokens:
        try:
            positions.append(token_positions(tokenizer, prompt, w, T))
        except ValueError:
            continue
        words.append(w)
    if not words:
        raise SystemExit(f"inference.py: --attn-map: none of the run's tokens {[n for n, _ in run.tokens]} occurs in {prompt!r}; name the words")
    return words, positions


def write_attn_maps(stem, images, word_maps, words, seeds):
    """`<stem>.jpg`: overlays, one row per word and one column per seed; `<stem>.npz`: maps fp32 [seeds, words, h, w], words, seeds"""
    import numpy as np
    from PIL import Image
    from textboost_amd.attn_maps import overlay
    W, H = images[0].size
    sheet = Image.new("RGB", (len(images) * W, len(words) * H))
    for k, im in enumerate(images):
        rgb = np.asarray(im)
        for j in range(len(words)):
            sheet.paste(Image.fromarray(overlay(rgb, word_maps[k, j])), box=(k * W, j * H))
    sheet.save(stem + ".jpg")
    np.savez(stem + ".npz", maps=np.asarray(word_maps, dtype=np.float32), words=np.array(list(words)), seeds=np.array(list(seeds), dtype=np.int64))
    print(f"wrote {stem}.jpg and {stem}.npz")


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    from textboost_amd import freeu as F
    F.check_count(parser, args)      # (argparse's own refusal: usage and exit status 2)
    from textboost_amd import generate as G
    if not args.model:
        raise SystemExit("inference.py: --model DIR (a local diffusers model directory: unet/, vae/, text_encoder/, tokenizer/, scheduler/) is required")
    G.check_model_dir(args.model, "inference.py")
    freeu = check_freeu_flags(args)
    canvas = check_canvas_flags(args)
    check_excite_flags(args)
    check_invert_flags(args)
    check_p2p_flags(args)
    blending = check_blend_flags(args)
    run = load_runs(args)
    words = positions = None
    if args.attn_map is not None:        # every refusal before anything reaches the device
        words, positions = attn_map_words(args.model, run, args.prompt, args.attn_map)
    edit = check_edit_args(args)
    region = check_region_args(args, run, edit)
    p2p = check_p2p_args(args, run)
    invert = check_invert_args(args)
    excite = check_excite_args(args, run)
    blend = check_blend_args(args, run, p2p, blending)
    seeds = args.seeds
    if invert is not None:
        seeds = ["inv"]        # one photo, one deterministic edit: the file names carry `inv` in the seed's place
        print("--invert-image: --seeds is not read (the photo's inversion is the noise; the encoder's mode makes the run deterministic)")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("inference.py needs an MI355X: the product path has no CPU fallback")
    from textboost_amd import augment
    nseeds = len(seeds)
    n = 2 * nseeds if p2p is not None else nseeds      # prompt-to-prompt: the source rows, then the edited rows
    nb = n      # rows of the executors' batch: the images, or (canvas) the image-window pairs of one UNet call
    if canvas is not None:
        from textboost_amd.canvas import CanvasPlan
        nb = min(CanvasPlan(canvas["S"], canvas["Hc"], canvas["Wc"], canvas["stride"], n, 1).pairs, CANVAS_UNET_BATCH)
    with torch.no_grad():
        pipe = G.Pipeline.from_model_dir(args.model, nb, steps=args.steps, guidance=7.5)
        base = G.load_base_text(args.model)
        te, tokenizer = G.load_text_encoder(args.model, run, 2 * nb, base=base)
        pipe.set_run(run)
        enc = None
        if edit is not None and edit["auto"] is not None:      # before the prompts are encoded: the maker runs the same text encoder
            from PIL import Image
            from textboost_amd import auto_mask as A
            from textboost_amd import edit as E
            enc = E.EditEncoder(args.model, pipe.size)
            maker = A.MaskMaker(pipe.unet, enc, lambda i: te.forward(i, pins=False), tokenizer, pipe.sampler.sch.alphas_cumprod)
            try:
                auto_mask, stats = maker.mask(edit["rgb"], edit["auto"], dilate=edit["dilate"])
            except ValueError as e:
                raise SystemExit(f"inference.py: --mask auto:{edit['auto']}: {e}")
            edit["mask"] = Image.fromarray(auto_mask.cpu().numpy())
            edit["mask"].save(auto_mask_path(args))
            print(f"wrote {auto_mask_path(args)}: {A.describe(auto_mask, stats)}")
            del maker
        if freeu is not None:      # behind the mask maker: an auto mask is the plain model's attention in the photo
            from textboost_amd.freeu import describe
            pipe.unet.enable_freeu(*freeu[:4], mode=freeu[4])
            print(describe(freeu))
        T = base.geo.max_pos
        prompts = [args.prompt] * nb if p2p is None else [args.prompt] * nseeds + [p2p["edit_prompt"]] * nseeds
        ids = G.tokenize(tokenizer, [""] * nb + prompts, T).to(pipe.dev)
        states = te.forward(ids, pins=False).view(2, nb * T, -1)
        if canvas is not None:
            latents = torch.cat([G.seeded_canvas_latent(s, canvas["Hc"], canvas["Wc"]) for s in seeds]).to(pipe.dev)
        else:
            latents = None if invert is not None else torch.cat([G.seeded_latent(s, pipe.size) for s in seeds] * (n // nseeds)).to(pipe.dev)
        recorder = None
        if words is not None:
            from textboost_amd.attn_maps import AttnMapRecorder
            recorder = AttnMapRecorder(pipe.unet)
        rset = rsteps = None
        if region is not None:
            from textboost_amd import regions as R
            rset, rsteps = R.RegionSet.for_unet(pipe.unet, region["regions"]), region["steps"]
        what = f"prompt {args.prompt!r}, " + (f"seeds {seeds}" if invert is None else f"photo {args.invert_image}")
        ctl = None
        if p2p is not None:
            from textboost_amd.p2p import P2PControl
            ctl = P2PControl.for_unet(pipe.unet, p2p["plan"], cross_steps=p2p["cross"], self_steps=p2p["self"])
            what += f", edit prompt {p2p['edit_prompt']!r}"
        bctl = None
        if blend is not None:
            from textboost_amd.local_blend import BlendControl
            bctl = BlendControl(pipe.unet, blend["source"], blend["edit"], words=blend["words"], start=blend["start"],
                                threshold=blend["threshold"], found=blend["found"])
            what += f", blend {blend['words']}"
        if canvas is not None:      # the MultiDiffusion canvas (textboost_amd/canvas.py): every refusal has happened on the host already
            rgbx = pipe.canvas_images(states[1], states[0], latents, stride=canvas["stride"],
                                      what=what + f", canvas {canvas['Wc'] * canvas['factor']} x {canvas['Hc'] * canvas['factor']}")
        elif invert is not None:      # the photo is encoded once and inverted under --prompt; the source row is pinned to that trajectory
            import numpy as np
            from textboost_amd import edit as E
            enc = E.EditEncoder(args.model, pipe.size)
            init_rgbx, pixels = E.prepare_image(invert["rgb"], enc.S)
            z0 = enc.encode(pixels)
            del enc
            latent_mask = pixel_mask = None
            if invert["mask"] is not None:
                pm, lm = E.prepare_mask(invert["mask"], init_rgbx.shape[0], cell=init_rgbx.shape[0] // pipe.size)
                latent_mask = torch.from_numpy(np.ascontiguousarray(lm)).to(pipe.dev)
                if not args.no_paste:
                    pixel_mask = torch.from_numpy(np.ascontiguousarray(pm)).to(pipe.dev)
            rgbx = pipe.invert_edit_images(states[1], states[0], z0, ctl, invert_guidance=invert["guidance"], latent_mask=latent_mask,
                                           pixel_mask=pixel_mask, init_rgbx=init_rgbx if pixel_mask is not None else None, what=what,
                                           blend=bctl)
        elif excite is not None:      # Attend-and-Excite (textboost_amd/excite.py): every refusal has happened on the host already
            import json
            from textboost_amd.excite import ExciteControl
            xctl = ExciteControl(pipe.unet, excite["positions"], excite["last"], words=excite["words"], excite_steps=excite["steps"],
                                 scale=excite["scale"], loss_scale=excite["loss_scale"], refine=excite["refine"])
            rgbx = pipe.images(states[1], states[0], latents, what=what + f", excite {excite['words']}", excite=xctl)
            with open(excite_path(args), "w") as f:
                json.dump(dict(xctl.report(), prompt=args.prompt, seeds=list(seeds)), f, indent=1)
            print(f"wrote {excite_path(args)}: {len(xctl.trace)} guided step(s), {xctl.skipped} skipped update(s)")
        elif edit is None:
            rgbx = pipe.images(states[1], states[0], latents, what=what, maps=recorder, regions=rset, region_steps=rsteps, p2p=ctl, blend=bctl)
        else:       # a seed's latent is the noise of its image; the photo is encoded once
            import numpy as np
            from textboost_amd import edit as E
            enc = enc or E.EditEncoder(args.model, pipe.size)
            init_rgbx, pixels = E.prepare_image(edit["rgb"], enc.S)
            z0 = enc.encode(pixels)
            del enc
            latent_mask = pixel_mask = None
            if edit["mask"] is not None:
                pm, lm = E.prepare_mask(edit["mask"], init_rgbx.shape[0], cell=init_rgbx.shape[0] // pipe.size)
                if edit["auto"] is not None:
                    check_auto_mask(pm, edit["auto"])
                latent_mask = torch.from_numpy(np.ascontiguousarray(lm)).to(pipe.dev)
                if not args.no_paste:
                    pixel_mask = torch.from_numpy(np.ascontiguousarray(pm)).to(pipe.dev)
            rgbx = pipe.edit_images(states[1], states[0], latents, z0, edit["strength"], latent_mask=latent_mask, pixel_mask=pixel_mask,
                                    init_rgbx=init_rgbx if pixel_mask is not None else None, maps=recorder, what=what, regions=rset,
                                    region_steps=rsteps)
        from PIL import Image
        images = [Image.fromarray(augment.to_host_rgb(rgbx[k])) for k in range(n)]
        if bctl is not None:
            write_blend(args, bctl, seeds, images[0].width // pipe.size)
        word_maps = None
        if recorder is not None:
            from textboost_amd.attn_maps import word_map
            token_maps = recorder.result()                                                  # [n, T, h, w]
            word_maps = torch.stack([word_map(token_maps, p) for p in positions], dim=1).cpu().numpy()     # [n, words, h, w]
    if region is not None:
        from textboost_amd import regions as R
        R.preview(region["regions"], images[0].size).save(regions_path(args))
        print(f"wrote {regions_path(args)}: " + "; ".join(f"{' '.join(r.words)} -> {int(r.cells.sum())} of {r.cells.size} latent cells, "
                                                           f"token positions {list(r.positions)}" for r in region["regions"]))
    if args.output is not None:
        rows = n // nseeds                                                    # 2 with --edit-prompt: the source row, then the edited row
        grid = Image.new("RGB", (nseeds * images[0].width, rows * images[0].height))     # diffusers.utils.make_image_grid(images, rows, nseeds)
        for k, im in enumerate(images):
            grid.paste(im, box=((k % nseeds) * im.width, (k // nseeds) * im.height))
        grid.save(args.output)
        print(f"wrote {args.output}")
        if word_maps is not None:
            write_attn_maps(os.path.splitext(args.output)[0] + "_attn", images, word_maps, words, seeds)
    else:
        for k, im in enumerate(images):
            seed = seeds[k % nseeds]
            out = args.prompt.replace(" ", "_") + f"_{seed}.jpg" if k < nseeds else p2p["edit_prompt"].replace(" ", "_") + f"_{seed}_edit.jpg"
            im.save(out)
            print(f"wrote {out}")
        if word_maps is not None:
            for k, seed in enumerate(seeds):
                write_attn_maps(args.prompt.replace(" ", "_") + f"_{seed}_attn", images[k:k + 1], word_maps[k:k + 1], words, [seed])


if __name__ == "__main__":
    main()
