"""Prompt-to-prompt editing: change the prompt and keep the picture (inference.py --edit-prompt / --reweight; Hertz et al. 2022).

    pl   = plan(tokenizer, prompt, edit_prompt, T, reweight=[("fluffy", 2.0)])       # host: the token plan M, a, w
    ctl  = P2PControl.for_unet(pipe.unet, pl)                                         # device tables, once per pipeline
    rgbx = pipe.images(cond, uncond, latents, p2p=ctl)                                # rows [0, n) source, [n, 2n) edited

The pipeline runs batch 2n: sampler rows [0, n) are the source images, [n, 2n) the edited ones, both halves from the same latents.  The UNet
batch is 4n in the sampler's (uncond | cond) order: u_src [0, n), u_edit [n, 2n), c_src [2n, 3n), c_edit [3n, 4n).  Control touches the
c_edit rows only, by EXTRA launches behind the unchanged all-rows ones, so every other row keeps the bits of an uncontrolled run.

Cross-attention of a c_edit row: with P^s the softmax of the matching c_src row and P^e the row's own,
    P_out[j] = w_j (a_j sum_i P^s[i] M[i, j] + (1 - a_j) P^e[j]),     O = sum_j P_out[j] v^e_j  =  P^s V1 + P^e V2,
    V1[i] = sum_j M[i, j] a_j w_j v^e_j,     V2[j] = (1 - a_j) w_j v^e_j
(`ops.attention_dual_fwd`, csrc/p2p_attn.hip; V1 / V2 are made once per generation and layer from the hoisted K/V, in fp32, rounded once).
Self-attention of a c_edit row at UNet levels >= 2: O = softmax(scale q^s k^s^T) v^e, one more `ops.attention_fwd` over row slices.

Token plan (index i = a source token position, j = an edit token position).  Both prompts are split on whitespace; a word's tokens are what
the tokenizer gives for it alone (`attn_maps.token_positions`' rule: sub-tokens and multi-vector placeholders span several positions).
The word lists are aligned by a longest common subsequence.  Tie-break: the alignment found by the standard table walked back from the ends
of both lists, which on unequal words drops the SOURCE word when that keeps the length (lcs[i-1][j] >= lcs[i][j-1]) and the edit word
otherwise -- so of several equally long alignments the one that matches words as late as possible in the source."""
from __future__ import annotations

import math
from typing import List, NamedTuple, Sequence, Tuple

import numpy as np

CROSS_STEPS, SELF_STEPS = 0.8, 0.4   # the paper's usual fractions; not measured on pretrained weights here
SELF_MIN_LEVEL = 2                   # self-attention control on maps of a quarter of the latent side and smaller (16 x 16, 8 x 8 at 512^2)
MAX_REWEIGHT = 10.0


class P2PError(ValueError):
    """an --edit-prompt / --reweight / --cross-steps / --self-steps argument that is refused"""


class P2PPlan(NamedTuple):
    M: np.ndarray    # fp32 [T, T]: M[i, j] = how much of source position i's probability goes to edit position j
    a: np.ndarray    # fp32 [T]: 1 = position j takes the source's (mapped) attention, 0 = its own
    w: np.ndarray    # fp32 [T]: the reweighting factor of position j


def parse_reweight(text: str) -> Tuple[str, float]:
    """"WORD=F" -> (WORD, F), 0 <= F <= 10.  P2PError when malformed."""
    word, eq, val = text.rpartition("=")
    word = word.strip()
    try:
        f = float(val)
    except ValueError:
        f = float("nan")
    if not eq or not word or len(word.split()) != 1 or not math.isfinite(f):
        raise P2PError(f"--reweight {text!r}: expected WORD=F (one word of the edit prompt and a factor)")
    if not 0.0 <= f <= MAX_REWEIGHT:
        raise P2PError(f"--reweight {text!r}: the factor must lie in 0 .. {MAX_REWEIGHT:g}")
    return word, f


def steps_for(fraction: float, steps: int, flag: str = "fraction") -> int:
    """control acts on the steps i < floor(fraction * steps).  P2PError outside [0, 1]."""
    f = float(fraction)
    if not (math.isfinite(f) and 0.0 <= f <= 1.0):
        raise P2PError(f"{flag} {fraction}: a fraction of the steps, 0 <= F <= 1")
    return min(int(steps), math.floor(round(f * steps, 9)))   # (rounded first: 0.8 * 50 is 40.00000000000001 in binary)


def _spans(tokenizer, prompt: str, T: int, what: str):
    """-> (words, [token positions of each word], position of the end token)"""
    ids = list(tokenizer(prompt, truncation=True, padding="max_length", max_length=T).input_ids)
    bos = getattr(tokenizer, "bos_token_id", None)
    pos = 1 if ids and ids[0] == bos else 0
    if pos != 1:
        raise P2PError(f"{what} {prompt!r}: the tokenizer sets no start token")
    words, spans = prompt.split(), []
    for word in words:
        toks = list(tokenizer(word, add_special_tokens=False).input_ids)
        if not toks:
            raise P2PError(f"{what} {prompt!r}: the word {word!r} has no tokens")
        if pos + len(toks) > T - 1 or ids[pos:pos + len(toks)] != toks:
            raise P2PError(f"{what} {prompt!r}: does not fit the {T} token positions word by word (at {word!r})")
        spans.append(list(range(pos, pos + len(toks))))
        pos += len(toks)
    return words, spans, pos


def align(src: Sequence[str], dst: Sequence[str]) -> List[Tuple[int, int]]:
    """the matched (source word index, edit word index) pairs of a longest common subsequence, ascending (the module text states the tie-break)"""
    n, m = len(src), len(dst)
    lcs = [[0] * (m + 1) for _ in range(n + 1)]
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            lcs[i][j] = lcs[i - 1][j - 1] + 1 if src[i - 1] == dst[j - 1] else max(lcs[i - 1][j], lcs[i][j - 1])
    pairs, i, j = [], n, m
    while i and j:
        if src[i - 1] == dst[j - 1]:
            pairs.append((i - 1, j - 1))
            i, j = i - 1, j - 1
        elif lcs[i - 1][j] >= lcs[i][j - 1]:
            i -= 1
        else:
            j -= 1
    return pairs[::-1]


def plan(tokenizer, prompt: str, edit_prompt: str, T: int, reweight: Sequence[Tuple[str, float]] = ()) -> P2PPlan:
    """the token plan of `prompt` -> `edit_prompt` at T token positions (module text).  reweight: (word of the edit prompt, factor) pairs.
    P2PError for a prompt that does not fit T, a reweight word that is not in the edit prompt, a factor outside 0 .. 10."""
    from .attn_maps import token_positions
    sw, ss, e_s = _spans(tokenizer, prompt, T, "--prompt")
    ew, es, e_e = _spans(tokenizer, edit_prompt, T, "--edit-prompt")
    M = np.zeros((T, T), dtype=np.float32)
    a = np.ones(T, dtype=np.float32)
    w = np.ones(T, dtype=np.float32)
    M[0, 0] = 1.0                                     # the start token
    pairs = align(sw, ew)
    pi, pj = 0, 0
    for mi, mj in pairs + [(len(sw), len(ew))]:       # the gap in front of every matched pair, then the pair; last: the gap behind the last pair
        I = [p for k in range(pi, mi) for p in ss[k]]
        J = [p for k in range(pj, mj) for p in es[k]]
        if I and J:                                   # swapped words
            if len(I) == len(J):
                for i, j in zip(I, J):
                    M[i, j] = 1.0
            else:
                for i in I:
                    for j in J:
                        M[i, j] = 1.0 / len(J)
        elif J:                                       # added words: the edit's own attention
            a[J] = 0.0
        # (dropped words: their rows of M stay zero)
        if mi < len(sw):
            for i, j in zip(ss[mi], es[mj]):          # a matched word: the same tokens
                M[i, j] = 1.0
        pi, pj = mi + 1, mj + 1
    for j in range(e_e, T):                           # the end token and the padding behind it
        M[min(e_s + (j - e_e), T - 1), j] = 1.0
    for word, f in reweight:
        if not 0.0 <= float(f) <= MAX_REWEIGHT:
            raise P2PError(f"--reweight {word}={f}: the factor must lie in 0 .. {MAX_REWEIGHT:g}")
        try:
            w[token_positions(tokenizer, edit_prompt, word, T)] = float(f)
        except ValueError as e:
            raise P2PError(f"--reweight {word}={f:g}: the word {word!r} is not in the edit prompt ({e})")
    return P2PPlan(M, a, w)


def mixed_values(pl: P2PPlan, v):
    """V1 [.., T, C] = (M diag(a w)) v and V2 = diag((1 - a) w) v for v [.., T, C] (numpy or torch, any float type; computed in v's type)"""
    import torch
    if isinstance(v, np.ndarray):
        m1 = (pl.M * (pl.a * pl.w)[None, :]).astype(v.dtype)
        return m1 @ v, ((1.0 - pl.a) * pl.w).astype(v.dtype)[:, None] * v
    m1 = torch.as_tensor(pl.M * (pl.a * pl.w)[None, :]).to(v)
    return m1 @ v, torch.as_tensor((1.0 - pl.a) * pl.w).to(v)[:, None] * v


class P2PControl:
    """The device side of one plan for one UNet: the mixing matrix, V1 / V2 per cross-attention layer (made lazily from the hoisted K/V the
    first time a layer runs after `reset()`; the buffers are kept, so a captured generation replays), and the flags of the current forward."""

    def __init__(self, pl: P2PPlan, n: int, T: int, h: int, w: int, device="cuda", cross_steps: float = CROSS_STEPS, self_steps: float = SELF_STEPS):
        import torch
        if pl.M.shape != (T, T) or pl.a.shape != (T,) or pl.w.shape != (T,):
            raise ValueError(f"a plan of {pl.M.shape[0]} token positions for a UNet of {T}")
        steps_for(cross_steps, 1, "cross_steps"), steps_for(self_steps, 1, "self_steps")
        self.plan, self.n, self.B4, self.T, self.h, self.w, self.dev = pl, n, 4 * n, T, h, w, device
        self.cross_steps, self.self_steps = float(cross_steps), float(self_steps)
        self.single = bool((pl.a == 1.0).all())       # a == 1 everywhere: V2 = 0, the single-term launch
        self.m1 = torch.from_numpy(np.ascontiguousarray(pl.M * (pl.a * pl.w)[None, :])).to(device)      # fp32 [T, T]
        self.w2 = torch.from_numpy(np.ascontiguousarray((1.0 - pl.a) * pl.w)).to(device)                # fp32 [T]
        self.cross_active = self.self_active = False
        self._v = {}
        self._fresh = set()

    @classmethod
    def for_unet(cls, unet, pl: P2PPlan, cross_steps: float = CROSS_STEPS, self_steps: float = SELF_STEPS):
        """for a guidance UNet of batch 4n (module text)"""
        if unet.B % 4:
            raise ValueError(f"prompt-to-prompt takes a guidance UNet of batch 4n (source and edited rows, unconditional and conditional), not {unet.B}")
        return cls(pl, unet.B // 4, unet.T, unet.H, unet.W, device=unet.dev, cross_steps=cross_steps, self_steps=self_steps)

    def reset(self):
        """a new generation: V1 / V2 are made again from its K/V"""
        self._fresh.clear()
        self.cross_active = self.self_active = False

    def values(self, layer: str, v2):
        """(V1, V2 or None) [n T, C] in v2's type for the layer's hoisted values v2 [4n T, C] (a column slice)"""
        import torch
        n, T, C = self.n, self.T, v2.shape[1]
        bufs = self._v.get(layer)
        if bufs is None:
            bufs = self._v[layer] = (torch.empty(n * T, C, device=v2.device, dtype=v2.dtype),
                                     None if self.single else torch.empty(n * T, C, device=v2.device, dtype=v2.dtype))
        if layer not in self._fresh:
            ve = v2[3 * n * T:4 * n * T].float().view(n, T, C)
            bufs[0].view(n, T, C).copy_(torch.matmul(self.m1, ve))
            if bufs[1] is not None:
                bufs[1].view(n, T, C).copy_(self.w2[None, :, None] * ve)
            self._fresh.add(layer)
        return bufs
