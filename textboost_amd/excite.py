"""Attend-and-Excite: keep every named subject in the image (inference.py --excite WORD ...; Chefer et al., SIGGRAPH 2023).

    ctl  = ExciteControl.for_prompt(pipe.unet, tokenizer, prompt, ["<dog>", "<cat>"], ids[n:])      # host: words -> token positions, `last`
    rgbx = pipe.images(cond, uncond, latents, excite=ctl)                                            # the guided generation
    ctl.trace                                                                                        # per guided step: losses, worst words, ...

During the first `excite_steps` of the sampling steps, every step first nudges the latents down the gradient of a loss on the level-2
cross-attention maps (16 x 16 at 64 x 64 latents) until every word owns at least one strongly attended patch, then runs the unchanged guided
step.  Per image, with A[j][s] the mean over the supervised layers and their heads of the conditional rows' softmax_j(scale q_s . k_j):

    pt_j[s] = softmax over the prompt's own tokens j in [1, last) of 100 A[j][s]          (start token, end token and padding are out)
    M_w[s]  = sum of pt_j[s] over the token positions of word w,   G_w = M_w smoothed by the 3 x 3 Gaussian (sigma 0.5, reflect padding)
    L       = max over the words of max(0, 1 - max_s G_w[s])                               (ties: the lowest word, the lowest position)

Device work per guided step: a truncated UNet forward (`HipUNet.forward(until="excite")`, which stops behind the last supervised layer and
records A through `ops.attn_token_maps`), `ops.excite_loss`, the backward to the latents (`HipUNet.backward_sample`, which injects the
gradient through `ops.excite_bwd` into the <= 9 query rows the loss depends on) and `ops.excite_update` (csrc/excite.hip).  The step size is
scale * sqrt(1 - 0.5 i / (N - 1)) at step i of N; at the steps {0, floor(0.2 N), floor(0.4 N)} the pass repeats, at most 20 times, until the
image's loss is below {0.05, 0.5, 0.8}: the one place where the host reads the losses.  These defaults are the paper's; they have not been
measured on pretrained weights here.  Everything in this file is host arithmetic on small tables."""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence

MAX_WORDS = 8        # csrc/excite.hip: words per image
MAX_POSITIONS = 16   # token positions per word
EXCITE_STEPS = 0.5   # the paper's: guidance during the first half of the steps
SCALE = 20.0         # the paper's step size factor
LOSS_SCALE = 256.0   # the 16-bit backward carries loss_scale * L (a power of two: dividing it out is exact); DESIGN.md 22
REFINE_AT = (0.0, 0.2, 0.4)          # iterative refinement at the steps floor(f * N) ...
REFINE_BELOW = (0.05, 0.5, 0.8)      # ... until the loss is below 1 - {0.95, 0.5, 0.2} (the paper's thresholds on the attention)
MAX_REFINE = 20
LEVEL = 2            # the supervised maps: a quarter of the latent side


class ExciteError(ValueError):
    """an --excite / --excite-steps / --excite-scale / --excite-loss-scale argument that is refused"""


def guided_steps(fraction: float, steps: int) -> int:
    """the guidance acts on the steps i < floor(fraction * steps).  ExciteError outside [0, 1]."""
    f = float(fraction)
    if not (math.isfinite(f) and 0.0 <= f <= 1.0):
        raise ExciteError(f"--excite-steps {fraction}: a fraction of the steps, 0 <= F <= 1")
    return min(int(steps), math.floor(round(f * steps, 9)))   # (rounded first: 0.58 * 50 is 28.999999999999996 in binary)


def step_size(scale: float, i: int, steps: int) -> float:
    """scale * sqrt(1 - 0.5 i / (N - 1)): the paper's linear decay of the squared factor from 1 to 0.5 over the schedule"""
    return float(scale) * math.sqrt(1.0 - 0.5 * i / max(steps - 1, 1))


def refine_thresholds(steps: int) -> Dict[int, float]:
    """{step: the loss the refinement drives every image below} -- a later entry wins when two fractions fall on one step (N < 5)"""
    return {math.floor(round(f * steps, 9)): t for f, t in zip(REFINE_AT, REFINE_BELOW)}


def first_eos(ids: Sequence[int], eos: int) -> int:
    """`last`: the position of the first end-of-text token behind the start token; len(ids) when there is none (a truncated prompt)"""
    ids = list(ids)
    for j in range(1, len(ids)):
        if ids[j] == eos:
            return j
    return len(ids)


def word_table(positions: Sequence[Sequence[int]], last: int, n_words: int = MAX_WORDS, n_pos: int = MAX_POSITIONS) -> List[List[int]]:
    """one image's rows of the device table: [n_words][n_pos] token positions, -1 padded.  ExciteError for too many words / positions, a word
    without a position and a position outside [1, last)."""
    if not 1 <= len(positions) <= n_words:
        raise ExciteError(f"--excite takes 1 .. {n_words} words, not {len(positions)}")
    table = [[-1] * n_pos for _ in range(n_words)]
    for w, pos in enumerate(positions):
        pos = sorted(set(int(p) for p in pos))
        if not pos:
            raise ExciteError(f"--excite: word {w} has no token position")
        if len(pos) > n_pos:
            raise ExciteError(f"--excite: word {w} spans {len(pos)} token positions; at most {n_pos}")
        if pos[0] < 1 or pos[-1] >= last:
            raise ExciteError(f"--excite: word {w} has the token positions {pos}; the prompt's own tokens are 1 .. {last - 1}")
        table[w][:len(pos)] = pos
    return table


class ExciteControl:
    """The words of one generation for one guidance UNet (batch 2n: unconditional rows, then conditional rows): the device tables of the
    conditional rows and the schedule.  `positions`: per image, per word, the token positions (or one list shared by all images);
    `last`: per image (or one int)."""

    def __init__(self, unet, positions, last, words: Optional[Sequence[str]] = None, excite_steps: float = EXCITE_STEPS, scale: float = SCALE,
                 loss_scale: float = LOSS_SCALE, refine: bool = True, max_refine: int = MAX_REFINE):
        import torch
        if unet.B % 2:
            raise ValueError(f"Attend-and-Excite takes a guidance UNet of batch 2n (unconditional and conditional rows), not {unet.B}")
        n = unet.B // 2
        if positions and isinstance(positions[0][0], int):
            positions = [positions] * n
        last = [int(last)] * n if isinstance(last, int) else [int(v) for v in last]
        if len(positions) != n or len(last) != n:
            raise ValueError(f"{len(positions)} position tables and {len(last)} end positions for {n} images")
        guided_steps(excite_steps, 1)
        if not (math.isfinite(scale) and scale > 0.0):
            raise ExciteError(f"--excite-scale {scale}: a finite number > 0")
        if not (math.isfinite(loss_scale) and loss_scale > 0.0):
            raise ExciteError(f"--excite-loss-scale {loss_scale}: a finite number > 0")
        if not 1 <= int(max_refine) <= 1000:
            raise ExciteError(f"max_refine {max_refine}: 1 .. 1000 passes")
        for l in last:
            if not 2 <= l <= unet.T:
                raise ExciteError(f"--excite: the prompt's end token at position {l}: there must be a token in front of it, within {unet.T}")
        self.n, self.T, self.h, self.w = n, unet.T, unet.H, unet.W
        self.words = list(words) if words is not None else [f"word {i}" for i in range(len(positions[0]))]
        self.positions = [[sorted(set(p)) for p in img] for img in positions]
        self.table_host = [word_table(img, l) for img, l in zip(positions, last)]
        self.last_host = last
        self.excite_steps, self.scale, self.loss_scale = float(excite_steps), float(scale), float(loss_scale)
        self.refine, self.max_refine = bool(refine), int(max_refine)
        self.table = torch.tensor(self.table_host, dtype=torch.int32, device=unet.dev)
        self.last = torch.tensor(last, dtype=torch.int32, device=unet.dev)
        self.trace: List[dict] = []      # one entry per guided step of the last generation (HipSampler.denoise)
        self.skipped = 0                 # updates skipped because the gradient was not finite

    @classmethod
    def for_prompt(cls, unet, tokenizer, prompt: str, words: Sequence[str], ids=None, **kw):
        """`words` of `prompt` -> positions through `attn_maps.token_positions` (ValueError for a word that does not occur); one prompt for
        all images"""
        from .attn_maps import token_positions
        T = unet.T
        positions = [token_positions(tokenizer, prompt, w, T) for w in words]
        if ids is None:
            ids = list(tokenizer(prompt, truncation=True, padding="max_length", max_length=T).input_ids)
        last = first_eos(ids, tokenizer.eos_token_id)
        return cls(unet, positions, last, words=words, **kw)

    def report(self) -> dict:
        """what inference.py writes to `<output stem>_excite.json`"""
        return {"words": self.words, "positions": self.positions[0], "excite_steps": self.excite_steps, "scale": self.scale,
                "loss_scale": self.loss_scale, "refine": self.refine, "max_refine": self.max_refine, "skipped_updates": self.skipped,
                "steps": self.trace}
