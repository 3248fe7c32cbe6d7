"""Cost of the masked training loss (--instance_mask_dir): profiles/masked_loss_step.json.

    python scratch/bench_masked_loss.py --parent <dir holding the parent commit's built textboost_amd/> [--out profiles/masked_loss_step.json]
    rocprofv3 --kernel-trace --stats -d <dir> -o masked -- python scratch/bench_masked_loss.py trace     (the two new kernels' own times)

The flagship step (SD1.5, B = 8, 512^2, r = 4, fp16, one HIP graph), alternating on one box, `--alternations` times:
  (a) the parent commit's step, (b) this tree with the mask off, (c) this tree with the mask on and uniform random weights.
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
    step, _ = build_step(batch=8, latent=64, lora_rank=4)
    if mask:
        w = step.enable_loss_weight()
        w.copy_(torch.rand(w.shape, generator=torch.Generator().manual_seed(7)))
    return step


def worker_step(args):
    import torch
    step = _build(args.tree, args.mask)
    step.capture(warmup=2)
    ms = _events(step.replay, args.steps, args.warm)
    sc = step.scalars()
    assert sc["found_inf"] == 0.0, sc
    q = statistics.quantiles(ms, n=20)
    print("RESULT " + json.dumps({"tree": args.label, "mask": bool(args.mask), "ms_per_step": statistics.median(ms), "p05_ms": q[0], "p95_ms": q[-1],
                                  "steps": args.steps, "warm": args.warm, "loss_mse": sc["loss_mse"], "device": torch.cuda.get_device_name(0)}))


def worker_trace(args):
    """under rocprofv3 --kernel-trace --stats: 20 replays of the masked step and 20 launches of the mask -> weights kernel (512^2 -> 64^2)"""
    import torch
    step = _build(args.tree, True)
    step.capture(warmup=2)
    for _ in range(20):
        step.replay()
    from textboost_amd import augment, ops
    mask = augment.to_device_mask(torch.randint(0, 256, (512, 512), dtype=torch.uint8).numpy())
    out = torch.empty(8, 1, 64, 64, device="cuda")
    for i in range(20):
        ops.img_to_loss_weight(mask, 0, 0, out[i % 8], cell=8, floor=0.0)
    torch.cuda.synchronize()
    print("RESULT " + json.dumps({"replays": 20, "loss_weight_launches": 20}))


def child(argv, limit):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + argv, capture_output=True, text=True, timeout=limit)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"child {argv} ended with {r.returncode}: nothing more is started")
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", nargs="?", default="driver", choices=["driver", "step", "trace"])
    ap.add_argument("--tree", default=HERE)
    ap.add_argument("--label", default="this")
    ap.add_argument("--parent", default=None)
    ap.add_argument("--mask", type=int, default=0)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warm", type=int, default=30)
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "masked_loss_step.json"))
    args = ap.parse_args()
    if args.mode == "step":
        return worker_step(args)
    if args.mode == "trace":
        return worker_trace(args)
    if not args.parent:
        raise SystemExit("--parent DIR: the parent commit's tree with its library built")
    legs = (("a_parent", args.parent, "parent", 0), ("b_mask_off", HERE, "this", 0), ("c_mask_on", HERE, "this", 1))
    runs = {k: [] for k, *_ in legs}
    for _ in range(args.alternations):
        for key, tree, label, mask in legs:
            runs[key].append(child(["step", "--tree", tree, "--label", label, "--mask", str(mask), "--steps", str(args.steps), "--warm",
                                    str(args.warm)], 300))
            print(key, runs[key][-1]["ms_per_step"], flush=True)
    res = {"setting": "SD1.5 UNet + CLIP-L geometry, random weights, B = 8, 64^2 latents (512^2), fp16, KPL on, the step as one HIP graph; "
                      f"scratch/bench_masked_loss.py: {args.alternations} alternations of (parent, mask off, mask on), one process each, "
                      f"{args.warm} warm-up replays then the median of {args.steps} event-timed replays",
           "device": runs["a_parent"][0]["device"]}
    for key in runs:
        ms = [r["ms_per_step"] for r in runs[key]]
        res[key] = {"ms_per_step_runs": ms, "median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "spread_ms": max(ms) - min(ms)}
    a, b, c = res["a_parent"], res["b_mask_off"], res["c_mask_on"]
    res["b_minus_a_ms"] = b["median_ms"] - a["median_ms"]
    res["b_inside_spread_of_a"] = a["min_ms"] <= b["median_ms"] <= a["max_ms"]
    res["c_minus_b_ms"] = c["median_ms"] - b["median_ms"]
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
