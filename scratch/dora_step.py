"""Cost of --use_dora (text-encoder DoRA, csrc/dora.hip): profiles/dora_step.json.

    python scratch/dora_step.py --parent <dir holding the parent commit's built textboost_amd/> [--out profiles/dora_step.json]

(a) DoRA off on this tree against the parent commit's tree: alternating processes (parent, this, parent, this) on one box, the flagship step
    (SD1.5, B = 8, 512^2, r = 4, fp16, one HIP graph); ms per step and the captured graph's node count of each
(b) DoRA on against off, r = 4: q/k/v and all six modules; ms per step, node count, the encoder's forward / backward spans, pack_lora's span
(c) as (b) at r = 64
(d) the three new kernels isolated at the step's shapes (student rows 1232, teacher rows 616 behind them): the row norms of all 12 layers of each
    module at r = 4 and r = 64, the forward application with each epilogue, the backward
Every measurement is one child process with its own time limit; the first child that fails ends the run."""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIX = ["q_proj", "k_proj", "v_proj", "out_proj", "fc1", "fc2"]


def _events(fn, reps, warm=3):
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


def worker_step(args):
    sys.path.insert(0, args.tree)
    import torch
    import textboost_amd
    assert os.path.dirname(os.path.dirname(os.path.abspath(textboost_amd.__file__))) == os.path.abspath(args.tree), textboost_amd.__file__
    from textboost_amd.workload import build_step

    graph_class = torch.cuda.CUDAGraph            # the step creates its own graph object: keep the captured hipGraph_t for the node count
    torch.cuda.CUDAGraph = lambda *a, **k: graph_class(keep_graph=True)
    kw = {} if args.targets == SIX[:3] else {"lora_targets": args.targets}
    if args.dora:
        kw["use_dora"] = True
    step, _ = build_step(batch=8, latent=64, lora_rank=args.rank, **kw)
    te = step.te
    step.step_eager()
    pack = _events(te.pack_lora, 20)
    fwd = _events(lambda: step._phase_student(encoder_only=True), 20)
    bwd = _events(lambda: te.backward(step.d_all, slot=0), 20)
    step.capture(warmup=2)
    nodes = None
    try:
        import ctypes
        hip_path = next(l.split()[-1] for l in open("/proc/self/maps") if "libamdhip64" in l)    # the HIP runtime this process already uses
        n = ctypes.c_size_t(0)
        rc = ctypes.CDLL(hip_path).hipGraphGetNodes(ctypes.c_void_p(step.graph[0].raw_cuda_graph()), None, ctypes.byref(n))
        assert rc == 0, rc
        nodes = int(n.value)
    except Exception as e:  # noqa: BLE001 -- the count is then reported as missing
        print("RESULT_NOTE node count failed:", repr(e))
    rounds = []
    for _ in range(args.rounds):
        ms = _events(step.replay, args.steps, warm=5)
        rounds.append(statistics.median(ms))
    sc = step.scalars()
    assert sc["found_inf"] == 0.0, sc
    print("RESULT " + json.dumps({"tree": args.label, "rank": args.rank, "targets": args.targets, "use_dora": bool(args.dora),
                                  "ms_per_step_rounds": rounds, "ms_per_step": statistics.median(rounds),
                                  "steps_per_s": 1e3 / statistics.median(rounds), "graph_nodes": nodes, "n_lora": step.n_lora,
                                  "pack_lora_ms": statistics.median(pack), "encoder_forward_ms": statistics.median(fwd),
                                  "encoder_backward_ms": statistics.median(bwd), "device": torch.cuda.get_device_name(0)}))


def worker_kernel(args):
    sys.path.insert(0, args.tree)
    import torch
    from textboost_amd import _lib as L
    from textboost_amd import ops
    dev, f16 = "cuda", torch.float16
    Ms, M, Lr = 1232, 1848, 12
    mods = {"qkv": (768, 2304, 3), "out_proj": (768, 768, 1), "fc1": (768, 3072, 1), "fc2": (3072, 768, 1)}     # (K, N, P)
    out = {"norms_all_12_layers_us": {}, "apply_us": {}, "bwd_us": {}}
    torch.manual_seed(0)
    for name, (K, N, P) in mods.items():
        W = [(torch.randn(N, K, device=dev) / K ** 0.5).half() for _ in range(Lr)]
        wp = ops.dora_weight_ptrs(W)
        m, n, c = torch.ones(Lr, N, device=dev), torch.empty(Lr, N, device=dev), torch.empty(Lr, N, device=dev)
        for r in (4, 64):
            A = torch.randn(Lr, P * r, K, device=dev) / r
            B = torch.randn(Lr, N, r, device=dev) * 0.05
            t = _events(lambda: ops.dora_norms(wp, f16, A, B, m, n, c, N // P, K, r, P, layers=Lr), 30, warm=5)
            out["norms_all_12_layers_us"][f"{name} r={r}"] = {"us": 1e3 * statistics.median(t), "weight_bytes": Lr * N * K * 2,
                                                               "fma": Lr * N * K * r}
        u = torch.randn(M, N, device=dev).half()
        bias = torch.randn(N, device=dev)
        if name in ("out_proj", "fc2"):
            R, y = torch.randn(M, N, device=dev), torch.empty(M, N, device=dev)
            fn, what = (lambda: ops.dora_apply(u, c[0], bias, y, Ms, R=R)), "bias + fp32 residual"
        elif name == "fc1":
            y, pre = torch.empty_like(u), torch.empty_like(u)
            fn, what = (lambda: ops.dora_apply(u, c[0], bias, y, Ms, act=L.ACT_QUICK_GELU, pre=pre)), "bias + quick_gelu + pre-activation"
        else:
            y = torch.empty_like(u)
            fn, what = (lambda: ops.dora_apply(u, c[0], bias, y, Ms)), "bias"
        out["apply_us"][name] = {"us": 1e3 * statistics.median(_events(fn, 50, warm=5)), "epilogue": what, "M": M, "student_rows": Ms, "N": N}
        dY, dU, dm = torch.randn(Ms, N, device=dev).half(), torch.empty(Ms, N, device=dev, dtype=f16), torch.zeros(N, device=dev)
        t = _events(lambda: ops.dora_bwd(dY, u[:Ms], c[0], n[0], dU, dm), 50, warm=5)
        out["bwd_us"][name] = {"us": 1e3 * statistics.median(t), "M": Ms, "N": N, "workgroups": (N + 63) // 64}
    out["note"] = "event-timed single launches on an otherwise idle stream, median of 30 / 50 (launch latency included); fp16 build"
    print("RESULT " + json.dumps(out))


def child(argv, limit):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + argv, capture_output=True, text=True, timeout=limit)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"child {argv} ended with {r.returncode}: nothing more is started")
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1]
    d = json.loads(line[len("RESULT "):])
    notes = [l for l in r.stdout.splitlines() if l.startswith("RESULT_NOTE ")]
    if notes:
        d["notes"] = notes
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", nargs="?", default="driver", choices=["driver", "step", "kernel"])
    ap.add_argument("--tree", default=HERE)
    ap.add_argument("--label", default="this")
    ap.add_argument("--parent", default=None)
    ap.add_argument("--rank", type=int, default=4)
    ap.add_argument("--targets", nargs="+", default=SIX[:3])
    ap.add_argument("--dora", action="store_true")
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "dora_step.json"))
    args = ap.parse_args()
    if args.mode == "step":
        return worker_step(args)
    if args.mode == "kernel":
        return worker_kernel(args)
    res = {"setting": "SD1.5 UNet + CLIP-L geometry, random weights, B = 8, 64^2 latents (512^2), fp16, KPL on, the step as one HIP graph; "
                      "scratch/dora_step.py: per process 5 rounds of 60 event-timed replays, the median of each round; processes in the "
                      "order parent, this, parent, this on one box in one session"}

    def step_run(tree, label, rank, targets, dora=False):
        return child(["step", "--tree", tree, "--label", label, "--rank", str(rank), "--targets", *targets] + (["--dora"] if dora else []), 400)

    def dump():
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)

    if args.parent:
        a = [step_run(args.parent, "parent", 4, SIX[:3]), step_run(HERE, "this", 4, SIX[:3]),
             step_run(args.parent, "parent", 4, SIX[:3]), step_run(HERE, "this", 4, SIX[:3])]
        par, this = [x["ms_per_step"] for x in a if x["tree"] == "parent"], [x["ms_per_step"] for x in a if x["tree"] == "this"]
        res["a_dora_off_vs_parent"] = {
            "runs": a, "parent_ms": par, "this_ms": this, "parent_spread_ms": abs(par[0] - par[1]),
            "difference_of_means_ms": sum(this) / 2 - sum(par) / 2,
            "graph_nodes_parent": a[0]["graph_nodes"], "graph_nodes_this": a[1]["graph_nodes"]}
        res["device"] = a[0]["device"]
        dump()
    for key, rank in (("b_rank4", 4), ("c_rank64", 64)):
        res[key] = {}
        for tname, targets in (("qkv", SIX[:3]), ("six_modules", SIX)):
            off, on = step_run(HERE, "this", rank, targets), step_run(HERE, "this", rank, targets, dora=True)
            res[key][tname] = {"dora_off": off, "dora_on": on, "extra_ms_per_step": on["ms_per_step"] - off["ms_per_step"],
                               "extra_graph_nodes": (on["graph_nodes"] - off["graph_nodes"]) if on["graph_nodes"] and off["graph_nodes"] else None}
            dump()
    res["d_isolated"] = child(["kernel", "--tree", HERE], 300)
    dump()
    print(json.dumps({k: v for k, v in res.items() if k != "setting"}, indent=1)[:8000])


if __name__ == "__main__":
    main()
