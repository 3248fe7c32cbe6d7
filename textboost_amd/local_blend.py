"""Prompt-to-prompt LocalBlend: the edit stays where the named words attend (inference.py --blend WORD ...; Hertz et al. 2022).

    ctl  = P2PControl.for_unet(pipe.unet, plan)                                              # the prompt-to-prompt control (p2p.py)
    bl   = BlendControl.for_prompts(pipe.unet, tokenizer, prompt, edit_prompt, ["<dog>"])    # host: words -> each prompt's token positions
    rgbx = pipe.images(cond, uncond, latents, p2p=ctl, blend=bl)                             # rows [0, n) source, [n, 2n) edited
    bl.final_mask, bl.area                                                                   # uint8 [n, h, w], int32 [n] on the device

The batch layout is prompt-to-prompt's (p2p.py): n pairs, sampler rows [0, n) source and [n, 2n) edited, UNet rows u_src | u_edit | c_src |
c_edit.  Every step's forward adds, for the 2n conditional rows, the head-and-layer mean of the level-2 cross-attention probabilities
(the (H >> 2) x (W >> 2) map: five layers on SD1.x) to one accumulator A fp32 [2n, T, h_l w_l] -- each row's OWN uncontrolled softmax, what
`ops.attn_token_maps` computes, from step 0 on.  After solver step i >= floor(start * steps), per pair j, with J_r the words' positions in
row r's own prompt:

    m_r[s]  = sum of A_r[p][s] over p in J_r          P_r = 3 x 3 max of m_r (stride 1, clipped windows)        mx_r = max_s P_r[s]
    bit_r   = P_r > fl32(th * mx_r)                   mask_j = nearest upsampling of (bit_src | bit_edit) to the latent grid [& limit]
    x_edit  <- mask_j ? x_edit : x_src                (x_src = the source row after the same step)

`ops.blend_mask` and `ops.dpm_step_local_blend` (csrc/local_blend.hip) do this on the device with no read-back, so a generation still
captures into one graph.  The defaults start = 0.2 and th = 0.3 are the published ones; they have not been measured on pretrained weights
here.  Everything in this file is host arithmetic on small tables."""
from __future__ import annotations

import math
import numbers
from typing import List, Optional, Sequence

MAX_POSITIONS = 16   # csrc/local_blend.hip: word positions per row
START = 0.2          # the published values (prompt-to-prompt's LocalBlend: start_blend 0.2, threshold 0.3)
THRESHOLD = 0.3
LEVEL = 2            # the recorded maps: a quarter of the latent side


class BlendError(ValueError):
    """a --blend / --blend-start / --blend-threshold argument that is refused"""


def start_step(fraction: float, steps: int) -> int:
    """the blend acts behind the steps i >= floor(fraction * steps).  BlendError outside [0, 1]."""
    f = float(fraction)
    if not (math.isfinite(f) and 0.0 <= f <= 1.0):
        raise BlendError(f"--blend-start {fraction}: a fraction of the steps, 0 <= F <= 1")
    return min(int(steps), math.floor(round(f * steps, 9)))   # (rounded first, as p2p.steps_for)


def check_threshold(th: float) -> float:
    t = float(th)
    if not (math.isfinite(t) and t >= 0.0):
        raise BlendError(f"--blend-threshold {th}: a finite number >= 0 (1 or more leaves nothing of the edit)")
    return t


def position_row(positions: Sequence[int], T: int, n_pos: int = MAX_POSITIONS) -> List[int]:
    """one row of the device table: the sorted distinct positions, -1 padded to n_pos.  BlendError for too many or one outside [0, T)."""
    pos = sorted(set(int(p) for p in positions))
    if len(pos) > n_pos:
        raise BlendError(f"--blend: the words span {len(pos)} token positions of one prompt; at most {n_pos}")
    if pos and (pos[0] < 0 or pos[-1] >= T):
        raise BlendError(f"--blend: token positions {pos} outside the prompt's {T}")
    return pos + [-1] * (n_pos - len(pos))


def word_positions(tokenizer, prompt: str, edit_prompt: str, words: Sequence[str], T: int):
    """-> (positions in `prompt`, positions in `edit_prompt`, {word: {"source": [...], "edit": [...]}}) through
    `attn_maps.token_positions`.  A word may be missing from one prompt (it then contributes through the other row only); a word in
    neither raises that function's ValueError."""
    from .attn_maps import token_positions
    src: List[int] = []
    edt: List[int] = []
    found = {}
    for word in words:
        per, err = {}, None
        for key, text, into in (("source", prompt, src), ("edit", edit_prompt, edt)):
            try:
                per[key] = token_positions(tokenizer, text, word, T)
            except ValueError as e:
                per[key], err = [], (err or e)
            into += per[key]
        if not per["source"] and not per["edit"]:
            raise err
        found[word] = per
    return sorted(set(src)), sorted(set(edt)), found


class BlendControl:
    """The words of one prompt-to-prompt generation for one guidance UNet (batch 4n): the device table of the 2n conditional rows and the
    schedule.  src_positions / edit_positions: the words' token positions in the source / the edit prompt (one list shared by the pairs,
    or one list per pair)."""

    def __init__(self, unet, src_positions, edit_positions, words: Optional[Sequence[str]] = None, start: float = START,
                 threshold: float = THRESHOLD, n_pos: int = MAX_POSITIONS, found: Optional[dict] = None):
        import torch
        if unet.B % 4:
            raise ValueError(f"LocalBlend takes a guidance UNet of batch 4n (source and edited rows, unconditional and conditional), not {unet.B}")
        n = unet.B // 4
        start_step(start, 1)
        self.threshold = check_threshold(threshold)
        self.start = float(start)

        def per_pair(p):
            p = list(p)
            if p and not isinstance(p[0], numbers.Integral):   # (numpy integers are positions too)
                if len(p) != n:
                    raise ValueError(f"{len(p)} position lists for {n} pairs")
                return [list(q) for q in p]
            return [p] * n

        rows = per_pair(src_positions) + per_pair(edit_positions)
        self.n, self.T, self.h, self.w, self.n_pos = n, unet.T, unet.H, unet.W, int(n_pos)
        self.table_host = [position_row(r, unet.T, n_pos) for r in rows]
        self.words = list(words) if words is not None else []
        self.found = found
        self.table = torch.tensor(self.table_host, dtype=torch.int32, device=unet.dev)
        self.keep_masks = False     # tests: keep every step's masks on the device -> `masks` uint8 [steps, n, h, w] (zeros before `start`)
        self.masks = None
        self.final_mask = None      # uint8 [n, h, w] on the device: the masks of the last step of the last generation (None: no step blended)
        self.area = None            # int32 [n] on the device: their set cells

    @classmethod
    def for_prompts(cls, unet, tokenizer, prompt: str, edit_prompt: str, words: Sequence[str], **kw):
        src, edt, found = word_positions(tokenizer, prompt, edit_prompt, words, unet.T)
        return cls(unet, src, edt, words=words, found=found, **kw)

    def report(self, area: Optional[Sequence[int]] = None, seeds: Optional[Sequence[int]] = None) -> dict:
        """what inference.py writes to `<output stem>_blend.json`"""
        out = {"words": self.words, "positions": self.found, "start": self.start, "threshold": self.threshold,
               "source_positions": [p for p in self.table_host[0] if p >= 0], "edit_positions": [p for p in self.table_host[self.n] if p >= 0]}
        if area is not None:
            out["area"] = [int(a) for a in area]
            out["cells"] = self.h * self.w
        if seeds is not None:
            out["seeds"] = [int(s) for s in seeds]
        return out
