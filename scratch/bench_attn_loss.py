"""Cost of the cross-attention localisation loss (--attn_loss_weight): profiles/attn_loss_step.json.

    python scratch/bench_attn_loss.py --parent <dir holding the parent commit's built textboost_amd/> [--out profiles/attn_loss_step.json]
    python scratch/bench_attn_loss.py kernels          (the new kernels alone, event-timed, at the default layers' shape)

The flagship step (SD1.5, B = 8, 512^2, r = 4, fp16, one HIP graph), alternating on one box, `--alternations` times:
  (a) the parent commit's step, (b) this tree with the flag off, (c) this tree with the masked loss and the localisation loss on at the default
  level (2: five layers, 16 x 16 maps), a random binary target, the placeholder token in every prompt.
Every measurement is one child process with its own time limit: build, capture, `--warm` replays (clocks and caches settle), then `--steps`
event-timed replays; the median of those is the process's figure.  The first child that fails ends the run."""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _events(fn, reps, warm):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def _build(tree, mask):
    sys.path.insert(0, tree)
    import torch
    import textboost_amd
    assert os.path.dirname(os.path.dirname(os.path.abspath(textboost_amd.__file__))) == os.path.abspath(tree), textboost_amd.__file__
    from textboost_amd.workload import build_step
    step, added = build_step(batch=8, latent=64, lora_rank=4)
    if mask:
        g = torch.Generator().manual_seed(7)
        w = step.enable_loss_weight()
        w.copy_(torch.rand(w.shape, generator=g))
        t = step.enable_attn_loss(0.01, [2], (added[0], added[0] + 2))   # the workload's two placeholder vectors
        t.copy_((torch.rand(t.shape, generator=g) > 0.6).float())
    return step


def worker_step(args):
    import torch
    step = _build(args.tree, args.mask)
    step.capture(warmup=2)
    ms = _events(step.replay, args.steps, args.warm)
    sc = step.scalars()
    assert sc["found_inf"] == 0.0, sc
    q = statistics.quantiles(ms, n=20)
    print("RESULT " + json.dumps({"tree": args.label, "attn_loss": bool(args.mask), "ms_per_step": statistics.median(ms), "p05_ms": q[0],
                                  "p95_ms": q[-1], "steps": args.steps, "warm": args.warm, "loss_mse": sc["loss_mse"],
                                  "loss_attn": sc.get("loss_attn"), "device": torch.cuda.get_device_name(0)}))


def worker_kernels(args):
    """the new kernels alone at the default layers' shape (B = 8, 8 heads, 256 queries, 77 keys, hd = 160) and at level 1's (1024 queries, hd = 80):
    medians of event-timed launches, back to back on one stream"""
    import torch
    sys.path.insert(0, args.tree)
    from textboost_amd import ops
    out = {}
    B, H, T = 8, 8, 77
    gen = torch.Generator().manual_seed(3)
    for name, Sq, hd, f in (("level2_256x77x160", 256, 160, 4), ("level1_1024x77x80", 1024, 80, 2)):
        C = H * hd
        q = torch.randn(B * Sq, C, generator=gen).half().cuda()
        kv = torch.randn(B * T, 2 * C, generator=gen).half().cuda()
        dq, dkv = torch.zeros_like(q), torch.zeros_like(kv)
        tok_w = torch.zeros(B, T, device="cuda")
        tok_w[:, 5:7] = 1
        target = (torch.rand(B, 1, 64, 64, generator=gen) > 0.6).float().cuda()
        g = torch.zeros(B, Sq, device="cuda")
        ws = ops.attn_loss_workspace("cuda", B, H, 5)
        ls = torch.tensor([65536.0], device="cuda")
        bwd = _events(lambda: ops.attn_loss_bwd(q, kv[:, :C], dq, dkv[:, :C], tok_w, g, B, H, Sq, T, hd, 1e-3, ls, ws, 2), args.steps, args.warm)
        coef = _events(lambda: ops.attn_loss_coef(target, g, f), args.steps, args.warm)
        out[name] = {"attn_loss_bwd_us": 1e3 * statistics.median(bwd), "attn_loss_coef_us": 1e3 * statistics.median(coef)}
    st = torch.zeros(16, device="cuda")
    fin = _events(lambda: ops.attn_loss_final(ws, 1.0 / 40, st[14:]), args.steps, args.warm)
    out["attn_loss_final_us"] = 1e3 * statistics.median(fin)
    out["note"] = "event-timed single launches include the launch gap of an eager stream (a few microseconds)"
    print("RESULT " + json.dumps(out))


def child(argv, limit):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + argv, capture_output=True, text=True, timeout=limit)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"child {argv} ended with {r.returncode}: nothing more is started")
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", nargs="?", default="driver", choices=["driver", "step", "kernels"])
    ap.add_argument("--tree", default=HERE)
    ap.add_argument("--label", default="this")
    ap.add_argument("--parent", default=None)
    ap.add_argument("--mask", type=int, default=0)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warm", type=int, default=30)
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "attn_loss_step.json"))
    args = ap.parse_args()
    if args.mode == "step":
        return worker_step(args)
    if args.mode == "kernels":
        return worker_kernels(args)
    if not args.parent:
        raise SystemExit("--parent DIR: the parent commit's tree with its library built")
    legs = (("a_parent", args.parent, "parent", 0), ("b_flag_off", HERE, "this", 0), ("c_flag_on", HERE, "this", 1))
    runs = {k: [] for k, *_ in legs}
    for _ in range(args.alternations):
        for key, tree, label, mask in legs:
            runs[key].append(child(["step", "--tree", tree, "--label", label, "--mask", str(mask), "--steps", str(args.steps), "--warm",
                                    str(args.warm)], 300))
            print(key, runs[key][-1]["ms_per_step"], flush=True)
    res = {"setting": "SD1.5 UNet + CLIP-L geometry, random weights, B = 8, 64^2 latents (512^2), fp16, KPL on, the step as one HIP graph; "
                      f"scratch/bench_attn_loss.py: {args.alternations} alternations of (parent, flag off, flag on at level 2 with masks), one process each, "
                      f"{args.warm} warm-up replays then the median of {args.steps} event-timed replays",
           "device": runs["a_parent"][0]["device"]}
    for key in runs:
        ms = [r["ms_per_step"] for r in runs[key]]
        res[key] = {"ms_per_step_runs": ms, "median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "spread_ms": max(ms) - min(ms)}
    a, b, c = res["a_parent"], res["b_flag_off"], res["c_flag_on"]
    res["b_minus_a_ms"] = b["median_ms"] - a["median_ms"]
    res["b_inside_spread_of_a"] = a["min_ms"] <= b["median_ms"] <= a["max_ms"]
    res["c_minus_b_ms"] = c["median_ms"] - b["median_ms"]
    res["kernels"] = child(["kernels", "--tree", HERE, "--steps", str(args.steps), "--warm", str(args.warm)], 300)
    k2 = res["kernels"]["level2_256x77x160"]
    res["new_kernels_isolated_ms"] = (5 * k2["attn_loss_bwd_us"] + k2["attn_loss_coef_us"] + res["kernels"]["attn_loss_final_us"]) / 1e3
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
