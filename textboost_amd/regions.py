"""Regional prompts: confine chosen prompt tokens' cross-attention to a region of the picture (inference.py --region).

    specs = [parse_region("<dog> dog=0,0,0.5,1"), parse_region("<cat> cat=@right.png")]          # host: words + box / mask file
    regs  = resolve_regions(tokenizer, prompt, T, specs, h, w)                                      # host: token positions + latent cells, every refusal
    rset  = RegionSet.for_unet(pipe.unet, regs)                                                     # device tables, once per generation
    rgbx  = pipe.images(cond, uncond, latents, regions=rset, region_steps=steps_for(0.6, steps))

Region r (0 .. 31, in the order given) owns the token positions of its words.  Inside the UNet every cross-attention forward then runs
`ops.attention_region_fwd` (csrc/region_attn.hip): a token of region r is visible only to the image positions inside r, every other token
(the start token, the end token and its padding included) stays global, and the unconditional half of the guided batch is unrestricted.  A
latent cell is inside a box if its centre is (half-open: x0 <= centre < x1, so two boxes that share an edge share no cell); inside a mask
picture if the picture, resized NEAREST to the latent grid, is >= 128 there.  A coarser cross-attention level is the any-pool of the latent
grid: a cell is inside if any latent cell it covers is (edit.py's rule for the latent mask), with ceil division on odd sizes.  Everything
here is host arithmetic on small arrays; the masked attention itself is the kernel's."""
from __future__ import annotations

import math
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

MAX_REGIONS = 32   # csrc/region_attn.hip: one bit per region in a query's uint32


class RegionError(ValueError):
    """a --region / --region-steps argument that is refused"""


class RegionSpec(NamedTuple):
    words: Tuple[str, ...]                                  # words of the prompt, as written
    box: Optional[Tuple[float, float, float, float]]        # x0, y0, x1, y1 in fractions of the image, or None
    mask: Optional[str]                                     # path of a mask picture, or None
    text: str                                               # the argument as given (messages)


class Region(NamedTuple):
    words: Tuple[str, ...]
    positions: Tuple[int, ...]     # token positions in the prompt tokenised to T
    cells: np.ndarray              # bool [h, w] on the latent grid


def parse_region(text: str) -> RegionSpec:
    """"WORDS=x0,y0,x1,y1" or "WORDS=@mask.png" -> RegionSpec.  WORDS: one or more space-separated words.  RegionError when malformed."""
    left, eq, right = text.rpartition("=")
    words = tuple(left.split())
    if not eq or not words or not right.strip():
        raise RegionError(f"--region {text!r}: expected \"WORDS=x0,y0,x1,y1\" or \"WORDS=@mask.png\"")
    right = right.strip()
    if right.startswith("@"):
        if len(right) == 1:
            raise RegionError(f"--region {text!r}: no file name after @")
        return RegionSpec(words, None, right[1:], text)
    parts = right.split(",")
    try:
        box = tuple(float(x) for x in parts)
    except ValueError:
        box = ()
    if len(parts) != 4 or len(box) != 4 or not all(math.isfinite(x) for x in box):
        raise RegionError(f"--region {text!r}: malformed box {right!r}: four numbers x0,y0,x1,y1 in fractions of the image")
    x0, y0, x1, y1 = box
    if not (0.0 <= x0 < x1 <= 1.0 and 0.0 <= y0 < y1 <= 1.0):
        raise RegionError(f"--region {text!r}: malformed box {right!r}: 0 <= x0 < x1 <= 1 and 0 <= y0 < y1 <= 1 are required")
    return RegionSpec(words, (x0, y0, x1, y1), None, text)


def box_cells(box: Sequence[float], h: int, w: int) -> np.ndarray:
    """bool [h, w]: the latent cells whose CENTRE ((j + 1/2) / w, (i + 1/2) / h) lies in [x0, x1) x [y0, y1)"""
    x0, y0, x1, y1 = box
    cx = 2 * np.arange(w) + 1          # centres in units of 1 / (2 w): exact integers against x * 2 w
    cy = 2 * np.arange(h) + 1
    inx = (cx >= x0 * 2 * w) & (cx < x1 * 2 * w)
    iny = (cy >= y0 * 2 * h) & (cy < y1 * 2 * h)
    return iny[:, None] & inx[None, :]


def mask_cells(mask, h: int, w: int) -> np.ndarray:
    """a Pillow image of any size (or a uint8 [H, W] array) -> bool [h, w]: convert("L"), resized NEAREST to the latent grid, >= 128 = inside"""
    from PIL import Image
    im = Image.fromarray(np.asarray(mask, dtype=np.uint8)) if isinstance(mask, np.ndarray) else mask
    im = im.convert("L").resize((w, h), Image.NEAREST)
    return np.asarray(im) >= 128


def halve_any(cells: np.ndarray) -> np.ndarray:
    """bool [h, w] -> bool [ceil(h / 2), ceil(w / 2)]: a cell is inside if ANY of the (up to) 2 x 2 cells it covers is"""
    h, w = cells.shape
    p = np.zeros((h + (h & 1), w + (w & 1)), dtype=bool)
    p[:h, :w] = cells
    return p.reshape(p.shape[0] // 2, 2, p.shape[1] // 2, 2).any(axis=(1, 3))


def pool_any(cells: np.ndarray, hw: Tuple[int, int]) -> np.ndarray:
    """the latent-grid region at a coarser cross-attention resolution `hw`: halve_any until the shape is reached.  ValueError when `hw` is
    not one of the UNet's levels of this grid."""
    m = np.asarray(cells, dtype=bool)
    while m.shape != tuple(hw):
        if m.shape[0] <= hw[0] and m.shape[1] <= hw[1] or m.shape == (1, 1):
            raise ValueError(f"{hw[0]} x {hw[1]} is not a halving of the {cells.shape[0]} x {cells.shape[1]} latent grid")
        m = halve_any(m)
    return m


def steps_for(fraction: float, executed: int) -> int:
    """--region-steps F: the regions act on the first ceil(F * executed) of the executed steps.  RegionError outside 0 < F <= 1."""
    f = float(fraction)
    if not 0.0 < f <= 1.0:
        raise RegionError(f"--region-steps {fraction}: a fraction of the executed steps, 0 < F <= 1")
    return min(executed, max(1, math.ceil(round(f * executed, 9))))   # (rounded first: 0.2 * 50 is 10.000000000000002 in binary)


def resolve_regions(tokenizer, prompt: str, T: int, specs: Sequence[RegionSpec], h: int, w: int, load_mask=None) -> List[Region]:
    """token positions (attn_maps.token_positions: sub-tokens and multi-vector placeholders span several; never the start token, the end
    token or padding) and latent cells of every region, on the host.  RegionError by name for: more than 32 regions, a word that is not in
    the prompt, a word (or token position) claimed by two regions, a mask that cannot be read, an empty region."""
    from .attn_maps import token_positions
    if len(specs) > MAX_REGIONS:
        raise RegionError(f"--region: {len(specs)} regions; at most {MAX_REGIONS} (one bit each in a position's region word)")
    if load_mask is None:
        from .edit import load_mask
    out: List[Region] = []
    owner: Dict[int, str] = {}
    seen: Dict[str, str] = {}
    for spec in specs:
        pos: List[int] = []
        for word in spec.words:
            if word in seen:
                raise RegionError(f"--region {spec.text!r}: the word {word!r} is claimed by two regions ({seen[word]!r} has it already)")
            seen[word] = spec.text
            try:
                pos += token_positions(tokenizer, prompt, word, T)
            except ValueError as e:
                raise RegionError(f"--region {spec.text!r}: the word {word!r} is not in the prompt ({e})")
        pos = sorted(set(pos))
        for p in pos:
            if p in owner:
                raise RegionError(f"--region {spec.text!r}: token position {p} of the prompt is claimed by two regions ({owner[p]!r} has it already)")
            owner[p] = spec.text
        if spec.mask is not None:
            try:
                cells = mask_cells(load_mask(spec.mask), h, w)
            except (OSError, ValueError) as e:
                raise RegionError(f"--region {spec.text!r}: {spec.mask} cannot be read as a picture ({e})")
        else:
            cells = box_cells(spec.box, h, w)
        if not cells.any():
            raise RegionError(f"--region {spec.text!r}: an empty region: no cell of the {h} x {w} latent grid lies inside")
        out.append(Region(spec.words, tuple(pos), cells))
    return out


def key_region_rows(regions: Sequence[Region], T: int) -> np.ndarray:
    """int32 [T]: the region of every token position of the conditional prompt, -1 = unrestricted"""
    row = np.full(T, -1, dtype=np.int32)
    for r, reg in enumerate(regions):
        for p in reg.positions:
            if not 0 < p < T:
                raise ValueError(f"token position {p} outside 1 .. {T - 1}")
            row[p] = r
    return row


def query_region_bits(regions: Sequence[Region], hw: Tuple[int, int]) -> np.ndarray:
    """uint32 [h_l * w_l]: bit r set where the position lies inside region r at the resolution `hw`"""
    bits = np.zeros(hw[0] * hw[1], dtype=np.uint32)
    for r, reg in enumerate(regions):
        bits |= pool_any(reg.cells, hw).reshape(-1).astype(np.uint32) << np.uint32(r)
    return bits


class RegionSet:
    """The device tables of one generation: `key_region` int32 [2B, T] (rows [0, B), the unconditional half, are -1; rows [B, 2B) carry the
    prompt's regions) and one `query_regions` table (uint32 bits, stored as int32 [h_l * w_l]) per cross-attention resolution in `levels`."""

    def __init__(self, regions: Sequence[Region], batch: int, T: int, h: int, w: int, levels: Sequence[Tuple[int, int]], device="cuda"):
        import torch
        if not 1 <= len(regions) <= MAX_REGIONS:
            raise RegionError(f"{len(regions)} regions: 1 .. {MAX_REGIONS}")
        for reg in regions:
            if reg.cells.shape != (h, w):
                raise ValueError(f"a region of {reg.cells.shape} cells on a {h} x {w} latent grid")
            if not reg.cells.any():
                raise RegionError(f"the region of {' '.join(reg.words)!r} is empty")
        self.regions, self.B, self.B2, self.T, self.h, self.w = list(regions), batch, 2 * batch, T, h, w
        kr = np.full((2 * batch, T), -1, dtype=np.int32)
        kr[batch:] = key_region_rows(regions, T)
        self.key_region = torch.from_numpy(kr).to(device)
        self.tables = {tuple(hw): torch.from_numpy(query_region_bits(regions, tuple(hw)).view(np.int32).copy()).to(device) for hw in levels}

    @classmethod
    def for_unet(cls, unet, regions: Sequence[Region]):
        """for a guidance UNet (batch 2B: unconditional rows first): the levels are those of `attn_maps.cross_attention_maps`"""
        from .attn_maps import cross_attention_maps
        if unet.B % 2:
            raise ValueError(f"regional prompts take a guidance UNet (an even batch: unconditional + conditional rows), not batch {unet.B}")
        levels = list(cross_attention_maps(unet))
        for hl, wl in levels:   # the level shapes are floor shifts of the grid: they agree with the ceil halving of `pool_any` only when they divide it
            f = unet.H // hl if hl else 0
            if f < 1 or hl * f != unet.H or wl * f != unet.W:
                raise ValueError(f"the {unet.H} x {unet.W} latent grid does not divide into the {hl} x {wl} cross-attention maps: regional prompts "
                                 "need a grid that every level halves exactly")
        return cls(regions, unet.B // 2, unet.T, unet.H, unet.W, levels, device=unet.dev)

    def table(self, hw: Tuple[int, int]):
        try:
            return self.tables[tuple(hw)]
        except KeyError:
            raise KeyError(f"no region table for the {hw[0]} x {hw[1]} cross-attention maps (built for {sorted(self.tables)})")


# flat preview colours, region 0 first (the cycle repeats after 8)
COLOURS = ((230, 60, 60), (60, 120, 230), (70, 190, 90), (240, 200, 50), (170, 80, 200), (60, 200, 210), (240, 140, 50), (150, 150, 150))


def preview(regions: Sequence[Region], size: Tuple[int, int]):
    """the regions as flat colours on black at the image's size (width, height): every latent cell becomes its block of pixels (NEAREST);
    where regions overlap the later one is on top"""
    from PIL import Image
    h, w = regions[0].cells.shape
    rgb = np.zeros((h, w, 3), dtype=np.uint8)
    for r, reg in enumerate(regions):
        rgb[reg.cells] = COLOURS[r % len(COLOURS)]
    return Image.fromarray(rgb).resize(tuple(size), Image.NEAREST)
