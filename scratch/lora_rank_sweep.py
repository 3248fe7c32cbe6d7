"""Text-encoder LoRA rank sweep at CLIP-L, B = 8 (profiles/lora_rank_sweep.json): ranks 4, 8 on the VALU adapter kernels, 16, 32, 64 on the wide
path (csrc/lora_wide.hip).

  encoder: forward (student rows + the 8 frozen prior rows riding along, as the trainer runs it) + backward, captured as one HIP graph;
  step:    the whole training step of workload.build_step (SD1.5, 64 x 64 latents), captured by TextBoostStep.capture.

Every figure is the median over `--rounds` rounds that visit the ranks in alternating order inside ONE process (device events around `--reps`
replays each), so drift of the shared host hits every rank alike.

    python scratch/lora_rank_sweep.py [--out profiles/lora_rank_sweep.json] [--skip-step]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
RANKS = (4, 8, 16, 32, 64)


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps   # ms per call


def alternate(fns, rounds, reps):
    """fns: {rank: callable}.  -> {rank: (median ms, min, max)}"""
    samples = {r: [] for r in fns}
    for k in range(rounds):
        order = list(fns) if k % 2 == 0 else list(reversed(list(fns)))
        for r in order:
            samples[r].append(timed(fns[r], reps))
    return {r: (statistics.median(v), min(v), max(v)) for r, v in samples.items()}


def encoder_graph(r, B, dev):
    from textboost_amd import models
    from textboost_amd.text_encoder import HipTextEncoder
    from textboost_amd.workload import synthetic_ids
    geo = models.SD15_CLIP
    csd = models.random_state_dict(models.clip_shapes(geo), 1235, device=dev)
    te = HipTextEncoder(geo, csd, B, mode="autocast", lora_rank=r, n_slots=2, device=dev, seed=0)
    table0 = te.token_table.clone()                     # the teacher rows read the original table
    added = te.add_tokens(list(range(100, 118)))
    te.lora_B.normal_(std=0.02)
    g = torch.Generator().manual_seed(r)
    ids, pids = synthetic_ids(B, added, g).to(dev), synthetic_ids(B, added, g, prior=True).to(dev)
    d_out = torch.randn(B * geo.max_pos, geo.hidden_size, device=dev)

    def run():
        te.forward(ids, slot=0, extra_ids=pids, extra_table=table0)
        te.backward(d_out.clone(), slot=0)   # (the pins zero rows of d_out in place)

    te.pack_lora()
    te.zero_grad()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run(); run()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            run()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    return graph.replay, (te, ids, pids, d_out, table0)   # the captured graph reads these buffers: the caller keeps them alive


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/lora_rank_sweep.json")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--skip-step", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a timing needs the GPU"
    dev, B = "cuda", 8
    from textboost_amd import _lib
    _lib.lib()
    res = {"device": torch.cuda.get_device_name(0), "batch": B, "clip": "CLIP-L (SD1.5)", "rounds": a.rounds, "reps_per_round": a.reps,
           "path": {str(r): ("narrow (text_small.hip)" if r <= 8 else "wide (lora_wide.hip)") for r in RANKS}}
    keep = []
    enc = {}
    for r in RANKS:
        enc[r], held = encoder_graph(r, B, dev)
        keep.append(held)
    for f in enc.values():
        timed(f, 10)
    res["encoder_fwd_bwd_ms"] = {str(r): dict(zip(("median", "min", "max"), (round(x, 4) for x in v)))
                                 for r, v in alternate(enc, a.rounds, a.reps).items()}
    print(json.dumps(res["encoder_fwd_bwd_ms"]), flush=True)
    del enc, keep
    if not a.skip_step:
        from textboost_amd.workload import build_step
        steps = {}
        for r in RANKS:
            step, _ = build_step(batch=B, lora_rank=r)
            step.capture(warmup=2)
            steps[r] = step.replay
            print(f"step r={r} captured", flush=True)
        for f in steps.values():
            timed(f, 5)
        st = alternate(steps, a.rounds, max(5, a.reps // 2))
        res["train_step_ms"] = {str(r): dict(zip(("median", "min", "max"), (round(x, 3) for x in v))) for r, v in st.items()}
        res["train_steps_per_s"] = {str(r): round(1e3 / v[0], 3) for r, v in st.items()}
        print(json.dumps(res["train_step_ms"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
