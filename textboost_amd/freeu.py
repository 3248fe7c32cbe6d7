"""FreeU (Si et al., CVPR 2024, "FreeU: Free Lunch in Diffusion U-Net"): the host side of `--freeu` -- the flags, the
per-family default factors and every refusal, before any model is built.  The device side is `HipUNet.enable_freeu` (csrc/freeu.hip)."""
from __future__ import annotations

import json
import math
import os
from typing import Optional, Sequence, Tuple

MODES = ("scalar", "structure")

# (b1, b2, s1, s2) per model family, keyed by the UNet's cross_attention_dim.  These are the values of the FreeU authors' README as
# recalled; nobody has measured them here (only random weights are available), so they are a starting point, not a recommendation.
DEFAULTS = {768: (1.5, 1.6, 0.9, 0.2),      # SD1.x
            1024: (1.4, 1.6, 0.9, 0.2)}     # SD2.x


class FreeUError(ValueError):
    """a --freeu flag that cannot be honoured; the message names the flag"""


def add_arguments(p):
    p.add_argument("--freeu", dest="freeu", type=float, nargs="*", default=None, metavar="F",
                   help="FreeU: amplify the backbone features (B1 B2) and damp the lowest frequencies of the skip features (S1 S2) of the first "
                        "two decoder stages; four values B1 B2 S1 S2, or none for the published constants of the model's family (SD1.x: "
                        "1.5 1.6 0.9 0.2, SD2.x: 1.4 1.6 0.9 0.2; not measured here)")
    p.add_argument("--freeu-backbone", dest="freeu_backbone", type=str, choices=MODES, default=None,
                   help="with --freeu: scalar multiplies the backbone half by B (diffusers, the default); structure by (B - 1) n + 1, n the "
                        "image's min-max normalised channel mean (the paper's revised formula)")


def check_count(parser, args):
    """argparse refuses any count of --freeu values but zero and four (usage error, exit status 2)"""
    if args.freeu is not None and len(args.freeu) not in (0, 4):
        parser.error(f"argument --freeu: expected zero or four values (B1 B2 S1 S2), got {len(args.freeu)}")


def cross_attention_dim(model_dir: str) -> int:
    with open(os.path.join(model_dir, "unet", "config.json")) as f:
        return int(json.load(f).get("cross_attention_dim", 1280))


def resolve(values: Optional[Sequence[float]], backbone: Optional[str], model_dir: Optional[str]) -> Optional[Tuple[float, float, float, float, str]]:
    """the parsed --freeu / --freeu-backbone -> None (no FreeU) or (b1, b2, s1, s2, mode).  Reads unet/config.json only when the defaults
    are asked for.  Raises FreeUError."""
    if values is None:
        if backbone is not None:
            raise FreeUError("--freeu-backbone needs --freeu [B1 B2 S1 S2] (the factors whose backbone half it shapes)")
        return None
    if backbone is not None and backbone not in MODES:
        raise FreeUError(f"--freeu-backbone {backbone}: scalar or structure")
    if len(values) == 0:
        try:
            dim = cross_attention_dim(model_dir)
        except (OSError, TypeError, ValueError) as e:
            raise FreeUError(f"--freeu: {e} (the default factors are chosen by the UNet's cross_attention_dim; --model must be a local "
                             "diffusers model directory)")
        if dim not in DEFAULTS:
            raise FreeUError(f"--freeu: no published factors for a UNet with cross_attention_dim {dim} (only {sorted(DEFAULTS)}: SD1.x, "
                             "SD2.x); pass --freeu B1 B2 S1 S2")
        values = DEFAULTS[dim]
    elif len(values) != 4:
        raise FreeUError(f"--freeu takes zero or four values (B1 B2 S1 S2), not {len(values)}")
    vals = tuple(float(v) for v in values)
    for name, v in zip(("B1", "B2", "S1", "S2"), vals):
        if not (math.isfinite(v) and v > 0):
            raise FreeUError(f"--freeu {name} = {v}: finite and > 0")
    return vals + (backbone or "scalar",)


def describe(f) -> str:
    return f"FreeU b1 {f[0]:g} b2 {f[1]:g} s1 {f[2]:g} s2 {f[3]:g} ({f[4]} backbone)"
