"""Command-line interface of the TextBoost trainer -- the boundary of /root/reference/train_textboost.py:49-450.

Every flag name / type / default / action / nargs / choices of the reference's `parse_args` is reproduced (66 flags, incl.
the `default=True` store_true of --disable_weighted_sample, :406-411, and argparse prefix abbreviation, which README.md:64
relies on); tests/test_host_logic.py checks this table against tests/golden/cli_flags.json, extracted from the reference
by AST.  Post-parse validation follows :435-448."""
from __future__ import annotations

import argparse
import warnings

_T = {"str": str, "int": int, "float": float}

# (flag, kwargs) -- interface facts of the reference CLI
FLAGS = [
    ("--pretrained_model_name_or_path", dict(type="str", default=None, required=True)),
    ("--revision", dict(type="str", default=None, required=False)),
    ("--variant", dict(type="str", default=None)),
    ("--tokenizer_name", dict(type="str", default=None)),
    ("--instance_data_dir", dict(type="str", default=None)),
    ("--instance", dict(type="str")),
    ("--class_data_dir", dict(type="str", default=None, required=False)),
    ("--instance_token", dict(type="str", default=None)),
    ("--class_token", dict(type="str", nargs="+", default=None)),
    ("--with_image_prior", dict(default=False, action="store_true")),
    ("--image_ppl_weight", dict(type="float", default=1.0)),
    ("--kpl_weight", dict(type="float", default=0.1)),
    ("--kpl_type", dict(type="str", default="cos")),
    ("--num_prior_images", dict(type="int", default=200)),
    ("--output_dir", dict(type="str", default="dreambooth-model")),
    ("--seed", dict(type="int", default=42)),
    ("--resolution", dict(type="int", default=512)),
    ("--center_crop", dict(default=False, action="store_true")),
    ("--train_batch_size", dict(type="int", default=1)),
    ("--sample_batch_size", dict(type="int", default=4)),
    ("--max_train_steps", dict(type="int", default=500)),
    ("--checkpointing_steps", dict(type="int", default=100)),
    ("--checkpoints_total_limit", dict(type="int", default=None)),
    ("--resume_from_checkpoint", dict(type="str", default=None)),
    ("--gradient_accumulation_steps", dict(type="int", default=1)),
    ("--gradient_checkpointing", dict(action="store_true")),
    ("--learning_rate", dict(type="float", default=5e-5)),
    ("--emb_learning_rate", dict(type="float", default=1e-3)),
    ("--scale_lr", dict(action="store_true", default=False)),
    ("--lr_scheduler", dict(type="str", default="constant")),
    ("--lr_warmup_steps", dict(type="int", default=500)),
    ("--dataloader_num_workers", dict(type="int", default=2)),
    ("--adam_beta1", dict(type="float", default=0.9)),
    ("--adam_beta2", dict(type="float", default=0.999)),
    ("--adam_weight_decay", dict(type="float", default=1e-2)),
    ("--adam_epsilon", dict(type="float", default=1e-08)),
    ("--max_grad_norm", dict(default=1.0, type="float")),
    ("--hub_token", dict(type="str", default=None)),
    ("--logging_dir", dict(type="str", default="logs")),
    ("--allow_tf32", dict(action="store_true")),
    ("--report_to", dict(type="str", default="tensorboard")),
    ("--validation_prompts", dict(type="str", nargs="+", default=None)),
    ("--num_validation_images", dict(type="int", default=4)),
    ("--validation_steps", dict(type="int", default=100)),
    ("--mixed_precision", dict(type="str", default=None, choices=["no", "fp16", "bf16"])),
    ("--prior_generation_precision", dict(type="str", default=None, choices=["no", "fp32", "fp16", "bf16"])),
    ("--concepts_list", dict(type="str", default=None)),
    ("--no_safe_serialization", dict(action="store_true")),
    ("--skip_save_text_encoder", dict(action="store_true", required=False)),
    ("--class_labels_conditioning", dict(required=False, default=None)),
    ("--validation_scheduler", dict(type="str", default="DPMSolverMultistepScheduler",
                                    choices=["DPMSolverMultistepScheduler", "DDPMScheduler"])),
    ("--text_encoder_use_attention_mask", dict(action="store_true", required=False)),
    ("--placeholder_token", dict(type="str", default="<dog>")),
    ("--initializer_token", dict(type="str", default="dog")),
    ("--unet_params_to_train", dict(type="str", choices=["none", "crossattn_kv", "crossattn", "attn", "all"], default="none")),
    ("--augment", dict(default="none")),
    ("--augment_ops", dict(type="str", default="object")),
    ("--augment_p", dict(type="float", default=0.8)),
    ("--augment_prompt", dict(type="int", default=1)),
    ("--augment_inversion", dict(action="store_true", default=False)),
    ("--num_samples", dict(type="int", default=None)),
    ("--lora_rank", dict(type="int", default=4)),
    ("--disable_weighted_sample", dict(action="store_true", default=True)),
    ("--null_prob", dict(type="float", default=0.1)),
    ("--template", dict(type="str", default="textboost")),
    ("--mixing", dict(action="store_true", default=False)),
]


# flags the reference does not have: added by `build_parser`, NOT reported by `flag_table` (the 66-flag comparison is about the reference's CLI)
LORA_TARGET_CHOICES = ["q_proj", "k_proj", "v_proj", "out_proj", "fc1", "fc2"]
EXTENSION_FLAGS = [
    # which Linear layers of every CLIP layer carry a rank --lora_rank adapter; the wider list is the one the reference keeps as a comment beside
    # its target_modules line (train_textboost.py:706)
    ("--lora_target_modules", dict(type="str", nargs="+", default=["q_proj", "k_proj", "v_proj"], choices=LORA_TARGET_CHOICES, metavar="M")),
]
# masked training loss (also not the reference's: it has the slot -- its step's `mask` branch, :1086-1088 -- and nothing that
# fills it).  A list of its own, like the adapter's variants: EXTENSION_FLAGS stays the one-entry list tests/test_lora_targets_host.py pins
MASKED_LOSS_FLAGS = [
    ("--instance_mask_dir", dict(type="str", default=None, help=(
        "directory of subject masks: instance image <stem>.<ext> needs <stem>.<any supported image extension> there, read as Pillow 'L' and of "
        "the image's pixel size.  White is the subject (loss weight 1), black the background.  The bytes are used as they are: soft masks are "
        "allowed and there is NO threshold (unlike inference.py --mask).  --concepts_list entries may carry the key instance_mask_dir instead."))),
    ("--mask_floor", dict(type="float", default=0.0, help=(
        "loss weight F of a background pixel, 0 <= F < 1: w = F + (1 - F) * mask.  Needs --instance_mask_dir; does not apply to loss_weight.pt"))),
]
# cross-attention localisation loss (FastComposer's supervision of where the placeholder token attends): off by default
ATTN_LOSS_FLAGS = [
    ("--attn_loss_weight", dict(type="float", default=0.0, help=(
        "weight of the cross-attention localisation loss (0 = off): loss = mse + kpl_weight * kpl + W * L_attn, L_attn in [-1, 1] lowest when all "
        "the attention mass of the placeholder token lies on the subject mask.  Needs --instance_mask_dir and --mixed_precision fp16 or bf16"))),
    ("--attn_loss_levels", dict(type="int", nargs="+", default=[2], metavar="L", help=(
        "UNet levels whose cross-attention layers are supervised (0 = the latent grid; default 2: the 16 x 16 maps at 512 x 512, five layers "
        "on SD1.x)"))),
]
# the adapter's variants (also not the reference's).  --use_dora: peft's LoraConfig(use_dora=True) -- every adapted Linear also trains a magnitude
# per output row; needs --lora_rank > 0
ADAPTER_VARIANT_FLAGS = [
    ("--use_dora", dict(action="store_true", default=False)),
]


def flag_table():
    """Normalised view used by the parity test (same schema as tests/golden/cli_flags.json)."""
    out = []
    for name, kw in FLAGS:
        d = {"flags": [name]}
        d.update(kw)
        out.append(d)
    return sorted(out, key=lambda s: s["flags"][0])


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="TextBoost training on MI355X (HIP kernels behind the reference CLI).")
    for name, kw in FLAGS + EXTENSION_FLAGS + ADAPTER_VARIANT_FLAGS + MASKED_LOSS_FLAGS + ATTN_LOSS_FLAGS:
        kw = dict(kw)
        if "type" in kw:
            kw["type"] = _T[kw["type"]]
        p.add_argument(name, **kw)
    return p


def check_mask_flags(args):
    """--mask_floor is a weight in [0, 1) and means nothing without masks (a --concepts_list may name them per concept: data.concept_masks
    checks that case once the list is read)"""
    floor = float(getattr(args, "mask_floor", 0.0) or 0.0)
    if not 0.0 <= floor < 1.0:
        raise ValueError(f"--mask_floor {floor}: the background weight must satisfy 0 <= F < 1")
    if floor != 0.0 and not getattr(args, "instance_mask_dir", None) and not getattr(args, "concepts_list", None):
        raise ValueError("--mask_floor needs --instance_mask_dir: without masks there is no background to weigh")


def attn_loss_weight_of(args) -> float:
    """--attn_loss_weight as a float >= 0 (nan refused); parse_args runs it, so a bad weight never leaves the command line"""
    raw = getattr(args, "attn_loss_weight", 0.0)
    w = float(0.0 if raw is None else raw)
    if not w >= 0.0:
        raise ValueError(f"--attn_loss_weight {raw}: the weight must be >= 0")
    return w


def check_attn_loss_flags(args, cross_attn_levels=None):
    """--attn_loss_weight: >= 0; when on it needs masks (--instance_mask_dir, or the key in a --concepts_list: data.concept_masks checks that
    case once the list is read), a 16-bit mode, and levels the UNet has (`cross_attn_levels`: one bool per UNet level, when known)"""
    w = attn_loss_weight_of(args)
    if w == 0.0:
        return
    levels = list(getattr(args, "attn_loss_levels", None) or [2])
    if any(l < 0 for l in levels):
        raise ValueError(f"--attn_loss_levels {levels}: levels are counted from 0, the latent grid")
    if cross_attn_levels is not None:
        bad = [l for l in levels if l >= len(cross_attn_levels) or not cross_attn_levels[l]]
        if bad:
            have = [i for i, on in enumerate(cross_attn_levels) if on]
            raise ValueError(f"--attn_loss_levels {bad}: this UNet has cross-attention on levels {have} only")
    if not getattr(args, "instance_mask_dir", None) and not getattr(args, "concepts_list", None):
        raise ValueError("--attn_loss_weight needs --instance_mask_dir: the loss is told where the subject is by its masks")
    if getattr(args, "mixed_precision", None) in (None, "no"):
        raise NotImplementedError("--attn_loss_weight without --mixed_precision: the localisation loss has 16-bit kernels only (fp16 or bf16)")


def parse_args(input_args=None):
    args = build_parser().parse_args(input_args)
    # train_textboost.py:435-448
    if args.with_image_prior:
        if args.class_data_dir is None:
            raise ValueError("You must specify a data directory for class images.")
        if args.class_token is None:
            raise ValueError("You must specify prompt for class images.")
    else:
        if args.class_data_dir is not None:
            warnings.warn("You need not use --class_data_dir without --with_image_prior.")
        if args.class_token is not None:
            warnings.warn("You need not use --class_token without --with_image_prior.")
    if args.augment_inversion and not bool(args.augment_prompt):
        raise ValueError("You need to use --augment_prompt=1 with --augment_prompt.")
    missing = [m for m in ("q_proj", "k_proj", "v_proj") if m not in args.lora_target_modules]
    if missing:  # q/k/v are one three-adapter kernel set, and the reference always trains them
        raise ValueError(f"--lora_target_modules must contain q_proj k_proj v_proj; {' '.join(missing)} missing")
    args.lora_target_modules = [m for m in LORA_TARGET_CHOICES if m in args.lora_target_modules]   # canonical order, duplicates dropped
    check_mask_flags(args)
    attn_loss_weight_of(args)
    if args.use_dora and args.lora_rank <= 0:
        raise ValueError("--use_dora needs --lora_rank > 0: DoRA decomposes the adapted weight, and --lora_rank 0 injects no adapter")
    return args
