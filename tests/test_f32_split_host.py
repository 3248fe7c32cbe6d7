"""Split mode of the fp32 contractions (--allow_tf32 -> tb_f32_set_mode(1)), host side: the derived product bound on the CPU emulation
(tests/f32_split_ref.py), the dispatch mode on the unchanged oracle (the yardsticks DESIGN 7.2 records), and the trainer's flag logic."""
import copy
import os
import sys
import types

import pytest
import torch

import f32_split_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(65, 33, 20), (64, 64, 64), (7, 5, 3)]


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_product_bound_holds_for_the_three_terms_and_catches_a_missing_one(M, N, K):
    g = torch.Generator().manual_seed(100 + K)
    A, W = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g)
    C64 = A.double() @ W.double().t()
    S = A.double().abs() @ W.double().abs().t()
    bound = R.product_bound(K, S)
    err = (R.split_matmul(A, W.t()).double() - C64).abs()
    print(f"[split {M}x{N}x{K}] emulation error / S {(err / S).max().item():.2e}  bound / S {(bound / S).max().item():.2e}")
    assert bool((err <= bound).all())
    for terms in (("hl", "hh"), ("lh", "hh")):      # lo_a hi_w dropped; hi_a lo_w dropped
        bad = ((R.split_matmul(A, W.t(), terms).double() - C64).abs() > bound).sum().item()
        print(f"  two-term {terms}: {bad} of {M * N} outside the bound")
        assert bad > M * N // 2, (terms, bad)


def test_split_of_non_finite_values_keeps_lo_zero():
    x = torch.tensor([float("inf"), float("-inf"), float("nan"), 3.4e38, 1.0 + 2.0 ** -10])
    hi, lo = R.split(x)
    assert lo[:4].eq(0).all() and hi[3].isinf() and lo[4] != 0
    assert hi[4] + lo[4] == x[4]


def test_dispatch_mode_is_live_on_the_oracle_unet():
    """the oracle's tiny UNet forward and d_ehs under the emulation and without it: the difference is the split's error on these
    quantities (nonzero: the mode is live; below 1e-3: it is sane).  Printed: the yardsticks of DESIGN 7.2."""
    B, hw, D = 2, 16, 64
    ref = R.tiny_unet(D, seed=0)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, 4, hw, hw, generator=g)
    t = torch.tensor([17, 801])
    ehs = torch.randn(B, 77, D, generator=g)
    dpred = torch.randn(B, 4, hw, hw, generator=g)
    pred, dehs = R.unet_pred_and_dehs(ref, x, t, ehs, dpred)
    mode = R.split_products()
    with mode:
        pred_s, dehs_s = R.unet_pred_and_dehs(ref, x, t, ehs, dpred)
    assert mode.calls > 50
    for name, a, b in (("UNet pred", pred_s, pred), ("UNet d_ehs", dehs_s, dehs)):
        r = R.rel_l2(a, b)
        print(f"[yardstick] {name}: rel-L2 {r:.3e}")
        assert 0.0 < r < 1e-3, (name, r)


def test_dispatch_mode_is_live_on_one_oracle_train_step():
    from oracle import train_step as ts
    B, hw, D = 2, 16, 64
    unet = R.tiny_unet(D, seed=3)
    student, teacher, added = R.tiny_encoders(D, seed=4)
    st = ts.TrainState(student, teacher, unet, added, ts.StepConfig())
    st_s = copy.deepcopy(st)
    g = torch.Generator().manual_seed(5)
    ids, pids = ts.synthetic_ids(B, added, g), ts.synthetic_ids(B, added, g, prior=True)
    x0, noise = torch.randn(B, 4, hw, hw, generator=g), torch.randn(B, 4, hw, hw, generator=g)
    t = torch.randint(0, 1000, (B,), generator=g)
    out = st.step(x0, noise, t, ids, pids)
    with R.split_products():
        out_s = st_s.step(x0, noise, t, ids, pids)
    pairs = [("hidden states", out_s["ehs"], out["ehs"]), ("pred", out_s["pred"], out["pred"]),
             ("grad added rows", out_s["g_emb_added"], out["g_emb_added"]),
             ("grad lora", torch.cat([x.flatten() for x in out_s["g_lora"]]), torch.cat([x.flatten() for x in out["g_lora"]]))]
    for name, a, b in pairs:
        r = R.rel_l2(a, b)
        print(f"[yardstick] step {name}: rel-L2 {r:.3e}")
        assert 0.0 < r < 1e-3, (name, r)
    w_s, w = st_s.te.token_embedding.weight.detach()[added], st.te.token_embedding.weight.detach()[added]
    print(f"[yardstick] step updated added rows: rel-L2 {R.rel_l2(w_s, w):.3e}")
    assert R.rel_l2(w_s, w) < 1e-3


# ------------------------------------------------------------------------------------------------ the trainer's flag logic (library stubbed)
def _trainer():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import train_textboost as T
    return T


def _args(*extra):
    T = _trainer()
    return T.parse_args(["--pretrained_model_name_or_path", "/nonexistent/sd15", *extra])


@pytest.mark.parametrize("extra,mode,word", [((), None, None), (("--allow_tf32",), 1, "mode 1"),
                                             (("--allow_tf32", "--mixed_precision", "no"), 1, "mode 1"),
                                             (("--allow_tf32", "--mixed_precision", "fp16"), None, "no effect"),
                                             (("--allow_tf32", "--mixed_precision", "bf16"), None, "no effect"),
                                             (("--mixed_precision", "fp16"), None, None)])
def test_allow_tf32_requests_the_split_mode_in_the_fp32_mode_only(extra, mode, word):
    T = _trainer()
    got, line = T.requested_f32_mode(_args(*extra))
    assert got == mode
    assert (line is None) if word is None else (word in line)


@pytest.mark.parametrize("extra,calls", [((), []), (("--allow_tf32",), [1, 0]), (("--allow_tf32", "--mixed_precision", "fp16"), [])])
def test_train_subject_sets_the_mode_around_the_subject_and_restores_it(monkeypatch, extra, calls):
    """_train_subject with the library call and the subject's body stubbed: mode 1 is set before the body runs, the previous mode is put
    back afterwards -- also when the body raises -- and without the flag (or under fp16) the library is not called at all"""
    T = _trainer()
    from textboost_amd import _lib as L
    seen, state = [], {"mode": 0}

    def fake_set(m):
        seen.append(m)
        prev, state["mode"] = state["mode"], m
        return prev

    def body(ctx, args, final, fh, val_ids):
        body.mode_inside = state["mode"]
        raise KeyError("subject failed")

    monkeypatch.setattr(L, "set_f32_mode", fake_set)
    monkeypatch.setattr(T, "_train_subject_in_mode", body)
    with pytest.raises(KeyError):
        T._train_subject(types.SimpleNamespace(is_main=False), _args(*extra), True, None, None)
    assert seen == calls and state["mode"] == 0
    assert body.mode_inside == (1 if calls else 0)


def test_lib_applies_the_mode_to_every_loaded_build_and_to_one_loaded_later(monkeypatch):
    """_lib.set_f32_mode with stub libraries: both loaded builds get the call, an invalid mode changes nothing"""
    from textboost_amd import _lib as L

    class Stub:
        def __init__(self):
            self.mode = 0

        def tb_f32_set_mode(self, m):
            prev, self.mode = self.mode, m
            return prev

    a, b = Stub(), Stub()
    monkeypatch.setattr(L, "_libs", {"fp16": a, "bf16": b})
    monkeypatch.setattr(L, "_f32_mode", 0)
    assert L.set_f32_mode(1) == 0 and (a.mode, b.mode) == (1, 1) and L.get_f32_mode() == 1
    with pytest.raises(ValueError):
        L.set_f32_mode(7)
    assert (a.mode, b.mode) == (1, 1) and L.get_f32_mode() == 1
    assert L.set_f32_mode(0) == 1 and (a.mode, b.mode) == (0, 0)
    assert {"tb_f32_set_mode", "tb_f32_get_mode"} <= set(L._SIGS)
