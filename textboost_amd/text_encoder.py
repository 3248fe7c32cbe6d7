"""HIP executor of the TextBoost text encoder: CLIP text transformer + rank-r LoRA on q/k/v + TextBoost pins.

Mirrors /root/reference/textboost/text_encoder.py:17-87 (`TextBoostModel`), the LoRA injection of
train_textboost.py:700-722 (peft `LoraConfig(r, lora_alpha=r, init_lora_weights="gaussian",
target_modules=["q_proj","k_proj","v_proj"])`) and the token-table growth of textboost/utils.py:117-166.

Three numeric modes, matching how the reference runs the two encoders:
  * "autocast" -- the trainable encoder under accelerate autocast (--mixed_precision fp16): fp32 master params, fp32 residual stream and
    LayerNorm/softmax statistics, fp16 Linear/attention operands (`train_textboost.py:919-926`);
  * "half"     -- the KPL teacher `original_text_encoder.to(fp16)` (:650, :939): plain fp16 module, forward only;
  * "fp32"     -- no mixed precision (the default, :298-308; weight_dtype stays float32, :930-939): every parameter, activation
    and gradient fp32, for the trainable encoder and the teacher alike (csrc/f32_path.hip).

`lora_targets` (--lora_target_modules) may add out_proj / fc1 / fc2 to q/k/v: one adapter each (P = 1) on a 64-column K-extension of its own,
masters in `extra[name].A [L, r, K_in]` / `.B [L, D_out, r]`.
`use_dora` (--use_dora) adds a magnitude per output row of every adapted Linear, `mag [L, 3D]` / `extra[name].mag [L, D_out]`: the GEMM then writes
u = x W^T + (x A^T) B^T, `tb_dora_apply` scales the student rows by m / ||W + B A|| and runs the Linear's epilogue, `tb_dora_bwd` turns dY into dU
and adds the magnitude gradient (csrc/dora.hip).

All arithmetic is in libtextboost_hip.so; this file owns parameters, buffers and the layer schedule.
Trainable state lives in three flat fp32 buffers so the optimizer / all-reduce see one tensor each:
  lora_A [L, 3r, D], lora_B [L, 3D, r]  and the token table [V + k, D] (rows >= first_added train).
"""
from __future__ import annotations

from dataclasses import dataclass
from types import SimpleNamespace
from typing import Dict, List, Optional, Sequence

import torch

from . import _lib as L
from . import ops

EOS_ID = 49407  # textboost/text_encoder.py:71


@dataclass
class CLIPGeometry:
    vocab_size: int = 49408
    hidden_size: int = 768
    intermediate_size: int = 3072
    num_layers: int = 12
    num_heads: int = 12
    max_pos: int = 77
    act: str = "quick_gelu"
    eps: float = 1e-5


LORA_QKV = ("q_proj", "k_proj", "v_proj")
LORA_EXTRA = ("out_proj", "fc1", "fc2")      # in the order their masters lie in the trainer's flat buffers
_EXTRA_W = {"out_proj": "out", "fc1": "fc1", "fc2": "fc2"}


def check_lora_targets(targets: Optional[Sequence[str]]):
    """-> the extra modules (a sub-tuple of LORA_EXTRA) of a --lora_target_modules list; q/k/v are one P = 3 kernel set and always adapted"""
    if targets is None:
        return ()
    targets = list(targets)
    bad = [t for t in targets if t not in LORA_QKV + LORA_EXTRA]
    if bad:
        raise ValueError(f"--lora_target_modules: unknown module {bad[0]!r} (choices: {' '.join(LORA_QKV + LORA_EXTRA)})")
    missing = [t for t in LORA_QKV if t not in targets]
    if missing:
        raise ValueError(f"--lora_target_modules must contain q_proj k_proj v_proj (one kernel set; the reference always trains them): "
                         f"{' '.join(missing)} missing")
    return tuple(n for n in LORA_EXTRA if n in targets)


HF_LAYER = {"ln1": "layer_norm1", "ln2": "layer_norm2", "q": "self_attn.q_proj", "k": "self_attn.k_proj", "v": "self_attn.v_proj",
            "out": "self_attn.out_proj", "fc1": "mlp.fc1", "fc2": "mlp.fc2"}


class HipTextEncoder:
    def __init__(self, geo: CLIPGeometry, state_dict: Dict[str, torch.Tensor], batch: int, mode: str = "autocast", lora_rank: int = 0,
                 lora_alpha: Optional[float] = None, n_slots: int = 1, device="cuda", seed: Optional[int] = None,
                 lora_targets: Optional[Sequence[str]] = None, use_dora: bool = False):
        """state_dict uses transformers CLIPTextModel keys (`text_model.embeddings.token_embedding.weight`, ...).
        use_dora (--use_dora): every adapted Linear also trains a magnitude per output row: `mag` [L, 3D] for q/k/v and
        `extra[name].mag` [L, D_out], initialised to the stored weights' row norms."""
        assert mode in ("autocast", "half", "fp32")
        assert geo.act in ("quick_gelu", "gelu")  # SD1.x CLIP-L / SD2.x OpenCLIP-H
        if use_dora and not lora_rank:
            raise ValueError("use_dora needs a LoRA adapter (lora_rank > 0)")
        if use_dora and mode == "half":
            raise NotImplementedError("use_dora: the adapted encoder runs in the autocast and fp32 modes")
        self.act_fwd, self.act_bwd = (L.ACT_QUICK_GELU, L.ACT_QUICK_GELU_GRAD) if geo.act == "quick_gelu" else (L.ACT_GELU, L.ACT_GELU_GRAD)
        self.geo, self.B, self.T, self.mode, self.dev = geo, batch, geo.max_pos, mode, device
        self.r = lora_rank
        self.scaling = (lora_alpha if lora_alpha is not None else lora_rank) / lora_rank if lora_rank else 0.0
        self.res_dtype = torch.float32 if mode in ("autocast", "fp32") else L.half_dtype()
        self.op_dtype = torch.float32 if mode == "fp32" else L.half_dtype()   # Linear / attention operands and activations
        self.n_slots = n_slots
        self._bufs: Dict[str, torch.Tensor] = {}
        D, Lr = geo.hidden_size, geo.num_layers
        sd = state_dict
        pre = "text_model."
        odt = self.op_dtype
        f16 = lambda t: t.detach().to(odt).to(device).contiguous()
        f32r = lambda t: t.detach().to(odt).to(torch.float32).to(device).contiguous()  # rounded like the operands (not at all in fp32 mode), fp32 storage
        tbl_dt = torch.float32 if mode in ("autocast", "fp32") else L.half_dtype()
        self.token_table = sd[pre + "embeddings.token_embedding.weight"].detach().to(tbl_dt).to(device).contiguous()
        self.pos_table = sd[pre + "embeddings.position_embedding.weight"].detach().to(tbl_dt).to(device).contiguous()
        # LayerNorm affine: fp32 params under autocast (LN runs in fp32); fp16-rounded for the half module
        lnp = (lambda t: t.detach().float().to(device).contiguous()) if mode in ("autocast", "fp32") else f32r
        self.Wl: List[Dict[str, torch.Tensor]] = []
        for i in range(Lr):
            lp = f"{pre}encoder.layers.{i}."
            W = {}
            wq = torch.cat([sd[lp + HF_LAYER[x] + ".weight"] for x in "qkv"], dim=0)
            W["qkv.w"], W["qkv.wd"] = f16(wq), f16(wq).t().contiguous()
            W["qkv.b"] = f32r(torch.cat([sd[lp + HF_LAYER[x] + ".bias"] for x in "qkv"], dim=0))
            for n in ("out", "fc1", "fc2"):
                w = sd[lp + HF_LAYER[n] + ".weight"]
                W[n + ".w"], W[n + ".wd"] = f16(w), f16(w).t().contiguous()
                W[n + ".b"] = f32r(sd[lp + HF_LAYER[n] + ".bias"])
            for n in ("ln1", "ln2"):
                W[n + ".g"], W[n + ".b"] = lnp(sd[lp + HF_LAYER[n] + ".weight"]), lnp(sd[lp + HF_LAYER[n] + ".bias"])
            self.Wl.append(W)
        self.lnf_g, self.lnf_b = lnp(sd[pre + "final_layer_norm.weight"]), lnp(sd[pre + "final_layer_norm.bias"])
        if mode == "fp32":
            for slot in (0, 1, 2):  # (an encoder may run on the trainer's side streams: one score workspace per stream slot, sized before any capture)
                with ops.workspace_slot(slot):
                    ops.reserve_attention_f32(device, 3 * batch, geo.num_heads, self.T, self.T)   # student + prior + teacher rows in one pass
        self.null_embedding = torch.zeros(self.T, D, device=device, dtype=torch.float32)
        self.use_fixed_special_embedding = False
        self.first_added = self.token_table.shape[0]
        self.n_added = 0
        self.wide = False
        self.extra: Dict[str, SimpleNamespace] = {}
        self.lora_targets = LORA_QKV + check_lora_targets(lora_targets)
        self.use_dora = bool(use_dora)
        if self.r > ops.LORA_MAX_RANK:
            raise NotImplementedError(f"text-encoder LoRA rank {self.r}: ranks up to {ops.LORA_MAX_RANK} are supported")
        if self.r:
            g = torch.Generator(device="cpu")
            if seed is not None:
                g.manual_seed(seed)
            # peft init_lora_weights="gaussian": A ~ N(0, (1/r)^2), B = 0
            self.lora_A = (torch.randn(Lr, 3 * self.r, D, generator=g) / self.r).to(device)
            self.lora_B = torch.zeros(Lr, 3 * D, self.r, device=device)
            self.grad_A = torch.zeros_like(self.lora_A)
            self.grad_B = torch.zeros_like(self.lora_B)
            # ranks <= 8: the VALU adapter kernels on a 64-column K-extension; above: the wide layout (csrc/lora_wide.hip), adapter p in columns
            # [p*rp, p*rp + r) of a [*, lw] extension, the down projection / dt as GEMMs and the weight gradients on the matrix cores
            self.wide = self.r > ops.LORA_NARROW_MAX
            self.rp, self.lw = ops.lora_wide_dims(self.r) if self.wide else (self.r, 64)
            self.w2_fwd = torch.zeros(Lr, 3 * D, self.lw, device=device, dtype=odt)
            self.w2_dgrad = torch.zeros(Lr, D, self.lw, device=device, dtype=odt)
            if self.wide:
                self.a_pad = torch.zeros(Lr, self.lw, D, device=device, dtype=odt)
                # weight of the dt GEMM; the fp32 mode multiplies by w2_fwd through a transposed view instead
                self.w2_t = None if mode == "fp32" else torch.zeros(Lr, self.lw, 3 * D, device=device, dtype=odt)
            # out_proj / fc1 / fc2 (drawn after q/k/v from the same generator: the default list draws what it always drew)
            I = geo.intermediate_size
            for name in self.lora_targets[3:]:
                Kin, Dout = {"out_proj": (D, D), "fc1": (D, I), "fc2": (I, D)}[name]
                X = SimpleNamespace(K=Kin, D=Dout, w=_EXTRA_W[name])
                X.A = (torch.randn(Lr, self.r, Kin, generator=g) / self.r).to(device)
                X.B = torch.zeros(Lr, Dout, self.r, device=device)
                X.grad_A, X.grad_B = torch.zeros_like(X.A), torch.zeros_like(X.B)
                X.rp = ops.lora_rect_dims(self.r)[0]
                X.a_pad = torch.zeros(Lr, 64, Kin, device=device, dtype=odt)
                X.w2_fwd = torch.zeros(Lr, Dout, 64, device=device, dtype=odt)
                X.w2_dgrad = torch.zeros(Lr, Kin, 64, device=device, dtype=odt)
                X.w2_t = None if mode == "fp32" else torch.zeros(Lr, 64, Dout, device=device, dtype=odt)   # weight of the dt GEMM
                self.extra[name] = X
            if self.use_dora:
                self._init_dora()

    # ------------------------------------------------------------------ DoRA (csrc/dora.hip)
    def _dora_of(self, name):
        """holder of a module's magnitude state (`mag`, `grad_mag`, `dora_n`, `dora_c`, `dora_wp`): the encoder itself for "qkv" (the P = 3 stack)"""
        return self if name == "qkv" else self.extra[name]

    def dora_modules(self):
        return ("qkv",) + tuple(self.extra) if self.use_dora else ()

    def _init_dora(self):
        """magnitudes m = ||W_j|| of the stored (operand-dtype) weights: the norm kernel with B = 0, which it is here"""
        Lr, D = self.geo.num_layers, self.geo.hidden_size
        for name in self.dora_modules():
            H = self._dora_of(name)
            N = 3 * D if name == "qkv" else H.D
            H.dora_w = [W[("qkv" if name == "qkv" else H.w) + ".w"] for W in self.Wl]
            H.dora_wp = ops.dora_weight_ptrs(H.dora_w)
            H.mag = torch.zeros(Lr, N, device=self.dev)
            H.grad_mag = torch.zeros_like(H.mag)
            H.dora_n = torch.zeros_like(H.mag)      # n = ||W + s B A|| per row and c = m / n, refreshed by pack_lora()
            H.dora_c = torch.ones_like(H.mag)
        self._dora_norms(init=True)

    def _dora_norms(self, init=False):
        D = self.geo.hidden_size
        for name in self.dora_modules():
            H = self._dora_of(name)
            A, B, Dn, K, P = (self.lora_A, self.lora_B, D, D, 3) if name == "qkv" else (H.A, H.B, H.D, H.K, 1)
            if init:
                ops.dora_norms(H.dora_wp, self.op_dtype, A, torch.zeros_like(B), None, H.mag, None, Dn, K, self.r, P, self.scaling,
                               layers=self.geo.num_layers)
            else:
                ops.dora_norms(H.dora_wp, self.op_dtype, A, B, H.mag, H.dora_n, H.dora_c, Dn, K, self.r, P, self.scaling,
                               layers=self.geo.num_layers)

    # ------------------------------------------------------------------ reference-facing surface
    def set_null_embedding(self, null):  # text_encoder.py:28-32
        self.null_embedding = null.detach().to(torch.float32).to(self.dev).contiguous()
        self.use_fixed_special_embedding = True

    def get_input_embeddings_weight(self):
        return self.token_table

    def add_tokens(self, initializer_ids):
        """textboost/utils.py:117-166 row bookkeeping: grow the table, copy initializer rows; returns new ids."""
        V, D = self.token_table.shape
        k = len(initializer_ids)
        new = torch.empty(V + k, D, device=self.dev, dtype=self.token_table.dtype)
        new[:V] = self.token_table
        for j, init in enumerate(initializer_ids):
            new[V + j] = self.token_table[init]
        self.token_table = new
        if self.n_added == 0:
            self.first_added = V
        self.n_added += k
        self.grad_added = torch.zeros(self.n_added, D, device=self.dev)
        return list(range(V, V + k))

    def __call__(self, input_ids, attention_mask=None, return_dict=False, slot=0):
        assert attention_mask is None, "text_encoder_use_attention_mask is off in the reference defaults (utils.py:14-17)"
        return (self.forward(input_ids, slot=slot), None)

    # ------------------------------------------------------------------ buffers
    def buf(self, name, rows, cols, dtype):
        """named, zero-initialised activation buffer.  A buffer that already exists with MORE rows is returned as its leading row slice:
        the forward with a frozen extra batch (`extra_ids`) sizes everything for student + extra rows, the backward walks the student rows."""
        t = self._bufs.get(name)
        if t is None or t.shape[1] != cols or t.dtype != dtype or t.shape[0] < rows:
            t = torch.zeros(rows, cols, device=self.dev, dtype=dtype)
            self._bufs[name] = t
        return t if t.shape[0] == rows else t[:rows]

    def pack_lora(self):
        """refresh the fp16 K-extension operands from the fp32 LoRA masters (once per optimizer step)."""
        if not self.r:
            return
        D = self.geo.hidden_size
        assert self.lora_A.is_contiguous() and self.lora_B.is_contiguous()
        for X in self.extra.values():   # one launch per extra module: every operand of its two-source GEMMs, of its down projection and of its dt GEMM
            ops.lora_wide_pack(X.A, X.B, X.a_pad, X.w2_fwd, X.w2_t, X.w2_dgrad, X.D, X.K, self.r, X.rp, 1, self.scaling, layers=self.geo.num_layers)
        if self.wide:
            ops.lora_wide_pack(self.lora_A, self.lora_B, self.a_pad, self.w2_fwd, self.w2_t, self.w2_dgrad, D, D, self.r, self.rp, 3, self.scaling,
                               layers=self.geo.num_layers)
        else:
            ops.lora_pack(self.lora_A, self.lora_B, self.w2_fwd, self.w2_dgrad, D, D, self.r, 3, self.scaling, layers=self.geo.num_layers)
        if self.use_dora:   # one launch per module: the row norms of W + s B A from the fp32 masters, and c = m / n
            self._dora_norms()

    # ------------------------------------------------------------------ forward
    def forward(self, input_ids, slot=0, pins=True, extra_ids=None, extra_table=None):
        """extra_ids [Be, T] (+ extra_table, the ORIGINAL fp32 token table): a frozen batch that rides along in the same launches -- its rows
        get no LoRA term (their K-extension operand rows stay zero) and are embedded from `extra_table`; used for the KPL teacher
        (train_textboost.py:1096-1100: the un-adapted encoder on the prior prompts), whose separate M = 616 pass was pure launch latency.
        Returns [(B + Be) * T, D]: student rows first.  backward() only ever walks the student rows."""
        geo, B, T = self.geo, input_ids.shape[0], self.T
        D, I, H = geo.hidden_size, geo.intermediate_size, geo.num_heads
        hd = D // H
        Bs, Ms = B, B * T                # student sequences / rows (LoRA, trainable table)
        if extra_ids is not None:
            B = B + extra_ids.shape[0]
        M = B * T
        rdt, f16, f32 = self.res_dtype, self.op_dtype, torch.float32   # (`f16` = the operand dtype: fp32 in the no-AMP mode)
        full32 = self.mode == "fp32"
        ids = input_ids.reshape(-1).contiguous()
        s = f"s{slot}."
        self._bufs[s + "ids"] = ids
        xl = self.extra
        gemm_down = self.wide or full32   # the down projection as a GEMM on a_pad; else tb_lora_down / the LayerNorm launch, on the fp32 masters
        dora = self.use_dora

        def linear(name, p, i, xin, w, out, A2, W2, bias, R=None, act=L.ACT_NONE, C2=None):
            """an adapted Linear.  DoRA: the GEMM writes u = x W^T + s (x A^T) B^T (kept per layer for the backward), then tb_dora_apply scales the
            student rows' columns by c = m / n, adds the bias and runs the Linear's own epilogue; the frozen rows behind them take no scale"""
            if not dora:
                return ops.gemm(xin, w, out, A2=A2, W2=W2, bias=bias, R=R, act=act, C2=C2)
            u = self.buf(p + "u_" + name, M, w.shape[0], f16)
            ops.gemm(xin, w, u, A2=A2, W2=W2)
            ops.dora_apply(u, self._dora_of(name).dora_c[i], bias, out, Ms, act=act, R=R, pre=C2)

        def down(name, xin, p, i):
            """t [M, 64] of an extra adapter: rows < Ms = xin @ A^T in columns [0, r); padding columns and the frozen extra rows stay zero"""
            t_ = self.buf(p + "t_" + name, M, 64, f16)
            if gemm_down:
                ops.gemm(xin[:Ms], xl[name].a_pad[i], t_[:Ms])
            else:
                ops.lora_down(xin[:Ms], xl[name].A[i], t_[:Ms])
            return t_

        h = self.buf(s + "h0", M, D, rdt)
        ops.embed_fwd(ids, self.token_table, self.pos_table, h[:Ms], T)
        if extra_ids is not None:
            eids = extra_ids.reshape(-1).contiguous()
            ops.embed_fwd(eids, extra_table, self.pos_table, h[Ms:], T)
        for i, W in enumerate(self.Wl):
            p = f"{s}l{i}."
            x1 = self.buf(p + "x1", M, D, f16)
            ls1 = self.buf(p + "ls1", M, 2, f32)
            qkv = self.buf(p + "qkv", M, 3 * D, f16)
            if self.r:
                t = self.buf(p + "t", M, self.lw, f16)  # columns >= 3r (and the frozen extra rows) stay zero (K-extension operand of the qkv GEMM)
                if self.wide:  # t[:Ms] = x1 @ a_pad^T: the padded weight's zero rows write the padding columns' zeros
                    ops.layernorm_fwd(h, x1, W["ln1.g"], W["ln1.b"], ls1, geo.eps)
                    ops.gemm(x1[:Ms], self.a_pad[i], t[:Ms])
                elif full32:  # no fused (fp16) down projection: t[:Ms, :3r] = x1 @ A^T as an exact-fp32 GEMM
                    ops.layernorm_fwd(h, x1, W["ln1.g"], W["ln1.b"], ls1, geo.eps)
                    ops.gemm(x1[:Ms], self.lora_A[i], t[:Ms, :3 * self.r])
                else:
                    ops.layernorm_fwd(h, x1, W["ln1.g"], W["ln1.b"], ls1, geo.eps, lora_A=self.lora_A[i], t=t, lora_rows=Ms)
                linear("qkv", p, i, x1, W["qkv.w"], qkv, t, self.w2_fwd[i], W["qkv.b"])
            else:
                ops.layernorm_fwd(h, x1, W["ln1.g"], W["ln1.b"], ls1, geo.eps)
                ops.gemm(x1, W["qkv.w"], qkv, bias=W["qkv.b"])
            o = self.buf(p + "o", M, D, f16)
            lse = self.buf(p + "lse", B * H, T, f32)
            ops.attention_fwd(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], o, lse, B, H, T, T, hd, causal=True)
            h2 = self.buf(p + "h2", M, D, rdt)
            if "out_proj" in xl:
                linear("out_proj", p, i, o, W["out.w"], h2, down("out_proj", o, p, i), xl["out_proj"].w2_fwd[i], W["out.b"], R=h)
            else:
                ops.gemm(o, W["out.w"], h2, bias=W["out.b"], R=h)
            # (an adapted fc1 / fc2 needs its input again in the backward, for dA = dt^T x: that layer input is then kept per layer)
            x2 = self.buf((p if "fc1" in xl else s) + "x2", M, D, f16)
            ls2 = self.buf(p + "ls2", M, 2, f32)
            a = self.buf((p if "fc2" in xl else s) + "a", M, I, f16)
            pre = self.buf(p + "pre", M, I, f16)
            if "fc1" in xl:
                if gemm_down:
                    ops.layernorm_fwd(h2, x2, W["ln2.g"], W["ln2.b"], ls2, geo.eps)
                    t1 = down("fc1", x2, p, i)
                else:   # the down projection rides in the LayerNorm launch, as q/k/v's does in LayerNorm 1
                    t1 = self.buf(p + "t_fc1", M, 64, f16)
                    ops.layernorm_fwd(h2, x2, W["ln2.g"], W["ln2.b"], ls2, geo.eps, lora_A=xl["fc1"].A[i], t=t1, lora_rows=Ms)
                linear("fc1", p, i, x2, W["fc1.w"], a, t1, xl["fc1"].w2_fwd[i], W["fc1.b"], act=self.act_fwd, C2=pre)
            else:
                ops.layernorm_fwd(h2, x2, W["ln2.g"], W["ln2.b"], ls2, geo.eps)
                ops.gemm(x2, W["fc1.w"], a, bias=W["fc1.b"], act=self.act_fwd, C2=pre)
            h3 = self.buf(p + "h3", M, D, rdt)
            if "fc2" in xl:
                linear("fc2", p, i, a, W["fc2.w"], h3, down("fc2", a, p, i), xl["fc2"].w2_fwd[i], W["fc2.b"], R=h2)
            else:
                ops.gemm(a, W["fc2.w"], h3, bias=W["fc2.b"], R=h2)
            h = h3
        out = self.buf(s + "out", M, D, rdt)
        lsf = self.buf(s + "lsf", M, 2, f32)
        ops.layernorm_fwd(h, out, self.lnf_g, self.lnf_b, lsf, geo.eps)
        if pins:
            ops.pin_fwd(out[:Ms], ids, self.null_embedding, Bs, T, self.use_fixed_special_embedding, EOS_ID)
            if M > Ms:
                ops.pin_fwd(out[Ms:], eids, self.null_embedding, B - Bs, T, self.use_fixed_special_embedding, EOS_ID)
        return out

    # ------------------------------------------------------------------ backward (autocast mode only)
    def zero_grad(self):
        if self.r:
            self.grad_A.zero_()
            self.grad_B.zero_()
            for X in self.extra.values():
                X.grad_A.zero_()
                X.grad_B.zero_()
            for name in self.dora_modules():
                self._dora_of(name).grad_mag.zero_()
        if self.n_added:
            self.grad_added.zero_()

    def backward(self, d_out, slot=0, pins=True):
        """d_out: fp32 [B*T, D] gradient of the (scaled) loss w.r.t. forward(slot)'s output. Accumulates into
        grad_A / grad_B / grad_added (and the extra modules' / DoRA magnitudes' gradient buffers).  All scratch is keyed by `slot`."""
        assert self.mode in ("autocast", "fp32")
        grad_A, grad_B, grad_added = self.grad_A if self.r else None, self.grad_B if self.r else None, self.grad_added if self.n_added else None
        xl = self.extra
        grad_x = {n: (X.grad_A, X.grad_B) for n, X in xl.items()}
        grad_m = {n: self._dora_of(n).grad_mag for n in self.dora_modules()}
        full32 = self.mode == "fp32"
        geo, T = self.geo, self.T
        D, I, H = geo.hidden_size, geo.intermediate_size, geo.num_heads
        hd = D // H
        s = f"s{slot}."
        ids = self._bufs[s + "ids"]
        M = ids.numel()
        B = M // T
        f16, f32 = self.op_dtype, torch.float32
        gs = f"g{slot}."

        def extra_bwd(name, i, dY, x):
            """dt of extra adapter `name` of layer i (the second K source of that Linear's dgrad GEMM); its dA / dB are added on the way"""
            X = xl[name]
            t_ = self._bufs[f"{s}l{i}.t_{name}"][:M]
            dt_ = self.buf(gs + "dt_" + name, M, 64, f16)
            gA, gB = grad_x[name]
            if full32:
                ops.lora_bwd(dY, x, t_, X.B[i], dt_, gA[i], gB[i], X.D, X.K, self.r, 1, self.scaling, w2_fwd=X.w2_fwd[i])
            else:
                ops.lora_rect_bwd(dY, x, t_, X.w2_t[i], dt_, gA[i], gB[i], X.D, X.K, self.r, self.scaling)
            return dt_

        def dora_bwd(name, i, dY):
            """DoRA: dU = dY * c in dY's place for everything below (adapter gradients, dgrad); the magnitude gradient is added on the way"""
            if name not in grad_m:
                return dY
            H = self._dora_of(name)
            dU = self.buf(gs + f"du{dY.shape[1]}", M, dY.shape[1], f16)
            ops.dora_bwd(dY, self._bufs[f"{s}l{i}.u_{name}"][:M], H.dora_c[i], H.dora_n[i], dU, grad_m[name][i])
            return dU

        if pins:
            ops.pin_bwd(d_out, ids, B, T, self.use_fixed_special_embedding, EOS_ID)
        h_last = self._bufs[f"{s}l{geo.num_layers - 1}.h3"][:M]
        dh = self.buf(gs + "dh_a", M, D, f32)
        # fp16 copy of the running residual gradient, written by the LayerNorm backward (fp32 mode: the fp32 gradient itself feeds the GEMMs)
        dh16 = None if full32 else self.buf(gs + "dh16", M, D, f16)
        ops.layernorm_bwd(d_out, h_last, self.lnf_g, self._bufs[s + "lsf"], dh, dx16=dh16)
        dh_other = self.buf(gs + "dh_b", M, D, f32)
        pending = None
        for i in reversed(range(geo.num_layers)):
            W = self.Wl[i]
            p = f"{s}l{i}."
            # saved activations: the leading M rows (the forward may have carried a frozen extra batch behind them)
            h_in = (self._bufs[f"{s}l{i - 1}.h3"] if i > 0 else self._bufs[s + "h0"])[:M]
            h2, pre, qkv, o = (self._bufs[p + n][:M] for n in ("h2", "pre", "qkv", "o"))
            lse = self._bufs[p + "lse"][:B * H]
            x1 = self._bufs[p + "x1"][:M]
            dpre = self.buf(gs + "dpre", M, I, f16)
            dy = dh if full32 else dh16
            if "fc2" in xl:
                dy = dora_bwd("fc2", i, dy)
                ops.gemm(dy, W["fc2.wd"], dpre, A2=extra_bwd("fc2", i, dy, self._bufs[p + "a"][:M]), W2=xl["fc2"].w2_dgrad[i], act=self.act_bwd, C2=pre)
            else:
                ops.gemm(dy, W["fc2.wd"], dpre, act=self.act_bwd, C2=pre)
            dx2 = self.buf(gs + "dx", M, D, f16)
            if "fc1" in xl:
                dpre = dora_bwd("fc1", i, dpre)
                ops.gemm(dpre, W["fc1.wd"], dx2, A2=extra_bwd("fc1", i, dpre, self._bufs[p + "x2"][:M]), W2=xl["fc1"].w2_dgrad[i])
            else:
                ops.gemm(dpre, W["fc1.wd"], dx2)
            dh2 = dh_other
            ops.layernorm_bwd(dx2, h2, W["ln2.g"], self._bufs[p + "ls2"], dh2, add=dh, dx16=dh16)
            do = self.buf(gs + "do", M, D, f16)
            dy = dh2 if full32 else dh16
            if "out_proj" in xl:
                dy = dora_bwd("out_proj", i, dy)
                ops.gemm(dy, W["out.wd"], do, A2=extra_bwd("out_proj", i, dy, o), W2=xl["out_proj"].w2_dgrad[i])
            else:
                ops.gemm(dy, W["out.wd"], do)
            dqkv = self.buf(gs + "dqkv", M, 3 * D, f16)
            delta = self.buf(gs + "delta", B * H, T, f32)
            ops.attention_bwd(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], o, lse, do, delta, dqkv[:, :D], dqkv[:, D:2 * D],
                              dqkv[:, 2 * D:], B, H, T, T, hd, causal=True)
            dx1 = self.buf(gs + "dx", M, D, f16)
            if self.r:
                dqkv = dora_bwd("qkv", i, dqkv)
                if self.wide:
                    dt = self.buf(gs + "dt", M, self.lw, f16)
                    if full32:
                        ops.lora_bwd(dqkv, x1, self._bufs[p + "t"][:M], self.lora_B[i], dt, grad_A[i], grad_B[i], D, D, self.r, 3, self.scaling,
                                     w2_fwd=self.w2_fwd[i], rp=self.rp)
                    else:
                        ops.gemm(dqkv, self.w2_t[i], dt)
                        ops.lora_wide_wgrad(dqkv, x1, self._bufs[p + "t"][:M], dt, grad_A[i], grad_B[i], D, D, self.r, self.rp, 3, self.scaling)
                elif full32:
                    dt = self.buf(gs + "dt", M, 64, f16)
                    ops.lora_bwd(dqkv, x1, self._bufs[p + "t"][:M], self.lora_B[i], dt, grad_A[i], grad_B[i], D, D, self.r, 3,
                                 self.scaling, w2_fwd=self.w2_fwd[i])
                else:
                    # chained: this layer's dA panels (dt^T x1, needed by nothing in the backward) ride in the NEXT layer's dt / dB launch,
                    # which leaves a third of the chip idle -- 11 launches fewer; two dt buffers alternate
                    dt = self.buf(gs + f"dt{i & 1}", M, 64, f16)
                    pending = ops.lora_bwd(dqkv, x1, self._bufs[p + "t"][:M], self.lora_B[i], dt, grad_A[i], grad_B[i], D, D, self.r, 3,
                                           self.scaling, pending=pending, defer_da=i > 0)
                ops.gemm(dqkv, W["qkv.wd"], dx1, A2=dt, W2=self.w2_dgrad[i])
            else:
                ops.gemm(dqkv, W["qkv.wd"], dx1)
            ops.layernorm_bwd(dx1, h_in, W["ln1.g"], self._bufs[p + "ls1"], dh, add=dh2, dx16=dh16 if (i > 0 and not full32) else None)
            # dh (buffer a) now holds the gradient w.r.t. this layer's input; dh2 (buffer b) is free again
        if self.n_added:
            ops.embed_bwd(dh, ids, grad_added, self.first_added)
        return dh
