#!/usr/bin/env python3
"""Decode-shaped linear layers: the fused small-M kernel (ops.linear_small) vs the op-by-op path
(norm kernel + hipBLASLt GEMM + activation / residual kernels), and an empty-ish kernel as the
per-launch floor.  Back-to-back launches in one HIP graph per case (the generation loop's mode).

    python benchmarks/smallm_bench.py [--rows 1,8,32,64]

``--stream``: the MLP products past smallm.hip's K (4096, 2048 with SwiGLU) of the 1 B – 8 B Llama-
shaped models and GPT-2 large / XL instead — the streaming kernel (smallm_stream.hip) at its plan's
K-slices and at one slice against the op-by-op path (``NBD_SMALLM_STREAM=0``), the three arms in
one process with their rounds interleaved; medians and each arm's round-to-round spread.  Every
arm rotates through enough copies of the weight that no replay finds it in the 256 MiB last-level
cache, as a decode step that streams all of a model's layers does not.

    python benchmarks/smallm_bench.py --stream [--rows 1,8,32,64] [--out profiles/smallm_stream_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def graph_time(fn, reps=20, iters=10):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            fn()
    g.replay()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        g.replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / (iters * reps) * 1e3  # us per call


# (model, hidden, intermediate) behind the --stream shapes
STREAM_MODELS = (("SmolLM2-1.7B / Llama-3.2-1B", 2048, 8192), ("Qwen2.5-1.5B", 1536, 8960),
                 ("Llama-3.2-3B", 3072, 8192), ("Llama-3-8B / Mistral-7B", 4096, 14336))
STREAM_GPT2 = (("GPT-2 large", 1280, 5120), ("GPT-2 XL", 1600, 6400))


def stream_graphs(arms, reps):
    """one captured graph of ``reps`` calls per arm (warmed on a side stream first)."""
    graphs = {}
    for name, fn in arms.items():
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for i in range(2):
                fn(i)
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for i in range(reps):
                fn(i)
        g.replay()
        graphs[name] = g
    torch.cuda.synchronize()
    return graphs


def stream_main(a):
    import statistics

    from nbdistributed_amd import ops
    from nbdistributed_amd.ops import decode

    ops.load_library()
    torch.manual_seed(0)
    bf = dict(device="cuda", dtype=torch.bfloat16)
    reps, iters, rounds = 16, 5, 9
    shapes = []  # (class, model, K, N)
    for model, H, I in STREAM_MODELS:
        if H > 2048:
            shapes.append(("rms+gate|up+swiglu", model, H, I))
        shapes.append(("down+res", model, I, H))
    shapes += [("proj2+bias+res", model, I, H) for model, H, I in STREAM_GPT2]
    out = []
    for cls, model, K, N in shapes:
        swiglu = cls.startswith("rms")
        Nw = 2 * N if swiglu else N
        copies = max(2, -(-(512 << 20) // (Nw * K * 2)))  # > 2 x the last-level cache
        Ws = [torch.randn(Nw, K, **bf) * K ** -0.5 for _ in range(copies)]
        bias = torch.randn(N, **bf) * 0.1 if "bias" in cls else None
        gamma = torch.ones(K, **bf)
        for M in [int(r) for r in a.rows.split(",")]:
            x = torch.randn(M, K, **bf)
            res = None if swiglu else torch.randn(M, N, **bf)
            kw = dict(norm=("rms", gamma, 1e-5), act="swiglu") if swiglu else dict(bias=bias, residual=res)

            def parent(i):  # what NBD_SMALLM_STREAM=0 runs: the parent's path
                mode, decode.SMALLM_STREAM = decode.SMALLM_STREAM, "0"
                try:
                    return ops.linear_small(x, Ws[i % copies], **kw)
                finally:
                    decode.SMALLM_STREAM = mode

            arms = {"op_by_op": parent,
                    "stream_plan": lambda i: ops.linear_small(x, Ws[i % copies], stream=0, **kw),
                    "stream_s1": lambda i: ops.linear_small(x, Ws[i % copies], stream=1, **kw)}
            nk = 2 if swiglu and M <= decode.FUSE_NORM_MAX_ROWS else 0
            plan = int(torch.ops.nbd.linear_small_plan(M, N, K, nk, 2 if swiglu else 0))
            graphs = stream_graphs(arms, reps)
            times = {n: [] for n in graphs}
            ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
            for _ in range(rounds):
                for n, g in graphs.items():
                    t0, t1 = ev(), ev()
                    t0.record()
                    for _ in range(iters):
                        g.replay()
                    t1.record()
                    t1.synchronize()
                    times[n].append(t0.elapsed_time(t1) / (iters * reps) * 1e3)
            r = dict(shape_class=cls, model=model, rows=M, K=K, N=N, plan_slices=plan, weight_copies=copies)
            for n, t in times.items():
                r[n + "_us"] = dict(median=round(statistics.median(t), 2), min=round(min(t), 2), max=round(max(t), 2))
            r["weight_GBps_stream_plan"] = round(Nw * K * 2 / r["stream_plan_us"]["median"] / 1e3, 1)
            print(json.dumps(r), flush=True)
            out.append(r)
        del Ws
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(reps_per_graph=reps, replays_per_round=iters, rounds=rounds, results=out), f, indent=1)
            f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="1,8,32,64")
    ap.add_argument("--stream", action="store_true", help="the shapes past smallm.hip's K, three arms interleaved")
    ap.add_argument("--out", default=None, help="--stream: also write the results to this JSON file")
    a = ap.parse_args()
    if a.stream:
        return stream_main(a)
    from nbdistributed_amd import ops

    ops.load_library()
    torch.manual_seed(0)
    C = 768
    bf = dict(device="cuda", dtype=torch.bfloat16)
    W = {"qkv": torch.randn(3 * C, C, **bf) * 0.02, "proj": torch.randn(C, C, **bf) * 0.02,
         "fc": torch.randn(4 * C, C, **bf) * 0.02, "proj2": torch.randn(C, 4 * C, **bf) * 0.02,
         "head": torch.randn(50257, C, **bf) * 0.02}
    b = {k: torch.randn(w.shape[0], **bf) * 0.1 for k, w in W.items()}
    lnw, lnb = torch.ones(C, **bf), torch.zeros(C, **bf)
    out = []
    z = torch.zeros(1, **bf)
    floor = graph_time(lambda: z.add_(1))
    print(json.dumps({"launch_floor_us": round(floor, 2)}), flush=True)
    for M in [int(r) for r in a.rows.split(",")]:
        x = torch.randn(M, C, **bf)
        h = torch.randn(M, 4 * C, **bf)
        cases = {
            "ln+qkv+bias": (lambda: ops.linear_small(x, W["qkv"], b["qkv"], norm=("ln", lnw, lnb, 1e-5)),
                            lambda: F.linear(ops.layer_norm(x, lnw, lnb), W["qkv"], b["qkv"])),
            "proj+bias+res": (lambda: ops.linear_small(x, W["proj"], b["proj"], residual=x),
                              lambda: x + F.linear(x, W["proj"], b["proj"])),
            "ln+fc+gelu": (lambda: ops.linear_small(x, W["fc"], b["fc"], norm=("ln", lnw, lnb, 1e-5), act="gelu"),
                           lambda: F.gelu(F.linear(ops.layer_norm(x, lnw, lnb), W["fc"], b["fc"]), approximate="tanh")),
            "proj2+bias+res": (lambda: ops.linear_small(h, W["proj2"], b["proj2"], residual=x),
                               lambda: x + F.linear(h, W["proj2"], b["proj2"])),
            "ln+head": (lambda: ops.linear_small(x, W["head"], norm=("ln", lnw, lnb, 1e-5)),
                        lambda: F.linear(ops.layer_norm(x, lnw, lnb), W["head"])),
            # the kernel without its norm prologue (what a separate norm kernel would feed)
            "qkv+bias (no norm)": (lambda: ops.linear_small(x, W["qkv"], b["qkv"]),
                                   lambda: F.linear(x, W["qkv"], b["qkv"])),
            "fc+gelu (no norm)": (lambda: ops.linear_small(x, W["fc"], b["fc"], act="gelu"),
                                  lambda: F.gelu(F.linear(x, W["fc"], b["fc"]), approximate="tanh")),
            "head (no norm)": (lambda: ops.linear_small(x, W["head"]), lambda: F.linear(x, W["head"])),
        }
        for name, (fused, ref) in cases.items():
            tf, tr = graph_time(fused), graph_time(ref)
            key = name.split(" ")[0].split("+")
            wbytes = W[key[1] if key[0] == "ln" else key[0]].numel() * 2
            r = dict(rows=M, op=name, fused_us=round(tf, 2), op_by_op_us=round(tr, 2), speedup=round(tr / tf, 2),
                     weight_GBps=round(wbytes / tf / 1e3, 1))
            print(json.dumps(r), flush=True)
            out.append(r)


if __name__ == "__main__":
    main()
