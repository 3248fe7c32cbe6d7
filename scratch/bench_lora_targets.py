"""Cost of --lora_target_modules (text-encoder LoRA on out_proj / fc1 / fc2): profiles/lora_targets_step.json.

    python scratch/bench_lora_targets.py --parent <dir holding the parent commit's built textboost_amd/> [--out profiles/lora_targets_step.json]

(a) the default module list on this tree against the parent commit's tree: alternating processes (parent, this, parent, this) on one box, the
    flagship step (SD1.5, B = 8, 512^2, r = 4, fp16, one HIP graph); ms per step and the captured graph's node count of each
(b) the same step with all six modules against the default, r = 4: ms per step, node count, the encoder's forward / backward spans
(c) as (b) at r = 16
(d) the narrow (r <= 8) dt / dB / dA launches of ONE fc1 adapter at D = 3072, K = 768, M = 1848, isolated: the form the encoder runs (dt as a GEMM
    on w2_t + tb_lora_bwd_panels) against the slab form of tb_lora_bwd (all of B staged in LDS per 16 rows)
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
    step, _ = build_step(batch=8, latent=64, lora_rank=args.rank, **kw)
    te = step.te
    # the encoder's spans, eager, on the step's own buffers (the merged student + teacher forward; the backward with the mixing mask off)
    step.step_eager()
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
    print("RESULT " + json.dumps({"tree": args.label, "rank": args.rank, "targets": args.targets, "ms_per_step_rounds": rounds,
                                  "ms_per_step": statistics.median(rounds), "graph_nodes": nodes, "n_lora": step.n_lora,
                                  "encoder_forward_ms": statistics.median(fwd), "encoder_backward_ms": statistics.median(bwd),
                                  "device": torch.cuda.get_device_name(0)}))


def worker_kernel(args):
    sys.path.insert(0, args.tree)
    import torch
    from textboost_amd import ops
    out = []
    D, K, M = 3072, 768, 1848
    for r in (4, 8):
        torch.manual_seed(r)
        x = torch.randn(M, K, device="cuda").half()
        dY = torch.randn(M, D, device="cuda").half()
        A = torch.randn(r, K, device="cuda") / r
        B = torch.randn(D, r, device="cuda") * 0.1
        rp, Rp = ops.lora_rect_dims(r)
        a_pad = torch.zeros(1, Rp, K, device="cuda", dtype=torch.float16)
        w2f = torch.zeros(1, D, Rp, device="cuda", dtype=torch.float16)
        w2t = torch.zeros(1, Rp, D, device="cuda", dtype=torch.float16)
        w2d = torch.zeros(1, K, Rp, device="cuda", dtype=torch.float16)
        ops.lora_wide_pack(A, B, a_pad, w2f, w2t, w2d, D, K, r, rp, 1)
        t = torch.zeros(M, 64, device="cuda", dtype=torch.float16)
        ops.lora_down(x, A, t)
        dt = torch.zeros(M, 64, device="cuda", dtype=torch.float16)
        dA, dB = torch.zeros_like(A), torch.zeros_like(B)
        new = _events(lambda: ops.lora_rect_bwd(dY, x, t, w2t[0], dt, dA, dB, D, K, r), 50, warm=5)
        gemm_only = _events(lambda: ops.gemm(dY, w2t[0], dt), 50, warm=5)
        old = _events(lambda: ops.lora_bwd(dY, x, t, B, dt, dA, dB, D, K, r, 1), 50, warm=5)
        out.append({"r": r, "D": D, "K": K, "M": M, "gemm_dt_plus_panels_us": 1e3 * statistics.median(new), "of_which_dt_gemm_us": 1e3 * statistics.median(gemm_only),
                    "slab_form_tb_lora_bwd_us": 1e3 * statistics.median(old), "slab_form_lds_bytes": D * (4 if r <= 4 else 8) * 4})
    print("RESULT " + json.dumps({"isolated_adapter_backward": out, "note": "event-timed back-to-back launches, median of 50; each figure covers dt, dB and dA "
                                  "of one adapter (two launches in either form)"}))


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
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "lora_targets_step.json"))
    args = ap.parse_args()
    if args.mode == "step":
        return worker_step(args)
    if args.mode == "kernel":
        return worker_kernel(args)
    res = {"setting": "SD1.5 UNet + CLIP-L geometry, random weights, B = 8, 64^2 latents (512^2), fp16, KPL on, the step as one HIP graph; "
                      "scratch/bench_lora_targets.py: per process 5 rounds of 60 event-timed replays, the median of each round; processes in the "
                      "order parent, this, parent, this on one box in one session"}

    def step_run(tree, label, rank, targets):
        return child(["step", "--tree", tree, "--label", label, "--rank", str(rank), "--targets", *targets], 400)

    if args.parent:
        a = [step_run(args.parent, "parent", 4, SIX[:3]), step_run(HERE, "this", 4, SIX[:3]),
             step_run(args.parent, "parent", 4, SIX[:3]), step_run(HERE, "this", 4, SIX[:3])]
        par, this = [x["ms_per_step"] for x in a if x["tree"] == "parent"], [x["ms_per_step"] for x in a if x["tree"] == "this"]
        res["a_default_list_vs_parent"] = {
            "runs": a, "parent_ms": par, "this_ms": this, "parent_spread_ms": abs(par[0] - par[1]),
            "difference_of_means_ms": sum(this) / 2 - sum(par) / 2,
            "graph_nodes_parent": a[0]["graph_nodes"], "graph_nodes_this": a[1]["graph_nodes"]}
        res["device"] = a[0]["device"]
    for key, rank in (("b_rank4", 4), ("c_rank16", 16)):
        d, s = step_run(HERE, "this", rank, SIX[:3]), step_run(HERE, "this", rank, SIX)
        res[key] = {"default": d, "six_modules": s, "extra_ms_per_step": s["ms_per_step"] - d["ms_per_step"],
                    "extra_graph_nodes": (s["graph_nodes"] - d["graph_nodes"]) if s["graph_nodes"] and d["graph_nodes"] else None}
    res["d_isolated"] = child(["kernel", "--tree", HERE], 200)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "setting"}, indent=1)[:6000])


if __name__ == "__main__":
    main()
