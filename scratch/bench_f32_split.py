"""A/B of the split mode of the fp32 contractions (tb_f32_set_mode(1), --allow_tf32) against the exact mode, on one box in one session.

  step MODE        one arm in this process: the metric configuration in fp32 mode (workload.build_step(precision="fp32"): SD1.5, B = 8, 64^2
                   latents, r = 4) captured under MODE, warm-up replays, then timed graph replays by device events -> one JSON line
  kernels          mode 0 and mode 1, alternating, on three launches of that step: the Linear (2048, 1280, 1280), the 3x3 convolution at 64^2
                   320 -> 320 (B = 8), and the 64^2 self-attention's QK^T (one (batch, head) problem of the batched launch as a plain launch:
                   4096 x 4096 x 40; and the whole batched forward, QK^T + softmax + PV, B = 8, H = 8)
  ab [OUT] [PAIRS] the driver: PAIRS (default 3) pairs of `step 0` / `step 1` in alternating FRESH processes, then `kernels`, each child under
                   its own time limit; stops at the first child that fails; writes OUT (default profiles/fp32_split_step.json)

    python scratch/bench_f32_split.py ab"""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WARMUP, REPLAYS = 3, 20


def _timed(fn, n, warm):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out


def _stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "n": len(ms)}


def step_arm(mode):
    import torch
    from textboost_amd import _lib as L
    from textboost_amd import workload
    step, _ = workload.build_step(precision="fp32")
    L.set_f32_mode(mode)
    assert L.lib().tb_f32_get_mode() == mode
    step.capture(warmup=2)
    ms = _timed(step.replay, REPLAYS, WARMUP)
    sc = step.scalars()
    res = {"arm": "step", "mode": mode, "device": torch.cuda.get_device_name(0), **_stats(ms), "loss": sc["loss"], "found_inf": sc["found_inf"]}
    print(json.dumps(res), flush=True)


def kernels():
    import torch
    from textboost_amd import ops
    dev = "cuda"
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g).to(dev)   # noqa: E731
    cases = {}
    A, W, out = r(2048, 1280), r(1280, 1280), torch.empty(2048, 1280, device=dev)
    cases["linear_2048x1280x1280"] = (lambda: ops.gemm(A, W, out), 2.0 * 2048 * 1280 * 1280)
    B, H, C = 8, 64, 320
    x, w9, y = r(B * H * H, C), r(C, 9 * C), torch.empty(B * H * H, C, device=dev)
    conv = dict(B=B, Hin=H, Win=H, Cin=C, Hout=H, Wout=H, stride=1, sign=1, upsample=0, transposed=0)
    cases["conv3x3_64x64_320_320_b8"] = (lambda: ops.gemm(x, w9, y, conv=conv), 2.0 * B * H * H * C * 9 * C)
    S, hd, Hn = 4096, 40, 8
    q1, k1, s1 = r(S, hd), r(S, hd), torch.empty(S, S, device=dev)
    cases["qk_one_head_4096x4096x40"] = (lambda: ops.gemm(q1, k1, s1, alpha=hd ** -0.5), 2.0 * S * S * hd)
    q, k, v = r(B * S, Hn * hd), r(B * S, Hn * hd), r(B * S, Hn * hd)
    o, lse = torch.empty(B * S, Hn * hd, device=dev), torch.empty(B, Hn, S, device=dev)
    cases["attention_fwd_b8_h8_4096_hd40"] = (lambda: ops.attention_fwd(q, k, v, o, lse, B, Hn, S, S, hd), 4.0 * B * Hn * S * S * hd)
    res = {"arm": "kernels", "device": torch.cuda.get_device_name(0), "cases": {}}
    for name, (fn, flop) in cases.items():
        ms = {0: [], 1: []}
        for _ in range(4):                       # alternating rounds of 5 timed launches per mode
            for mode in (0, 1):
                with ops.f32_mode(mode):
                    ms[mode] += _timed(fn, 5, 2)
        m0, m1 = statistics.median(ms[0]), statistics.median(ms[1])
        res["cases"][name] = {"mode0": _stats(ms[0]), "mode1": _stats(ms[1]), "speedup": round(m0 / m1, 3),
                              "mode0_tflops": round(flop / m0 * 1e-9, 2), "mode1_tflops": round(flop / m1 * 1e-9, 2)}
    print(json.dumps(res), flush=True)


def _child(args, limit):
    r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), *args], capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"child {args} ended with status {r.returncode}: nothing more is started")
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def ab(out, pairs):
    runs = []
    for _ in range(pairs):
        for mode in (0, 1):
            runs.append(_child(["step", str(mode)], 240))
            print(json.dumps(runs[-1]), flush=True)
    arms = {}
    for mode in (0, 1):
        med = [x["median_ms"] for x in runs if x["mode"] == mode]
        arms[f"mode{mode}"] = {"run_medians_ms": med, "median_ms": round(statistics.median(med), 3), "spread_ms": round(max(med) - min(med), 3),
                               "steps_per_s": round(1e3 / statistics.median(med), 3)}
    res = {"what": "fp32 (no-AMP) metric step, B = 8, 64^2 latents, SD1.5, r = 4, one HIP graph: exact mode (0) against the three-term bf16 "
                   f"split (1); {pairs} pairs of alternating fresh processes, {WARMUP} warm-up + {REPLAYS} timed replays each, device events",
           "device": runs[0]["device"], **arms,
           "step_speedup": round(arms["mode0"]["median_ms"] / arms["mode1"]["median_ms"], 3), "runs": runs}
    res["faster_by_more_than_the_spread"] = arms["mode0"]["median_ms"] - arms["mode1"]["median_ms"] > arms["mode0"]["spread_ms"] + arms["mode1"]["spread_ms"]
    res["kernels"] = _child(["kernels"], 240)["cases"]
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: res[k] for k in ("mode0", "mode1", "step_speedup", "faster_by_more_than_the_spread", "kernels")}))


if __name__ == "__main__":
    cmd = sys.argv[1] if len(sys.argv) > 1 else "ab"
    if cmd == "step":
        step_arm(int(sys.argv[2]))
    elif cmd == "kernels":
        kernels()
    else:
        ab(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "fp32_split_step.json"), int(sys.argv[3]) if len(sys.argv) > 3 else 3)
