#!/usr/bin/env python3
"""Generation throughput: GPT-2 small (bf16, random init) decoding with the framework's KV cache
(graph-captured and eager) vs Hugging Face ``GPT2LMHeadModel.generate`` (its KV cache, eager) on
the same weights; plus the decode-attention kernel alone (achieved HBM bandwidth over the cache).

    python benchmarks/generate_bench.py [--batches 1,8,32] [--prompt 128] [--new 256]

``--continue``: the time to the first token of a second turn, continuing from the returned cache
(``generate(turn, 1, cache=cache)``: block append, ``csrc/kernels/append.hip``) against the only
way without it, re-prefilling the whole history (``generate(history + turn, 1)``); SmolLM2-135M
and GPT-2-small shapes, rounds of the two interleaved.

    python benchmarks/generate_bench.py --continue [--models smollm2,gpt2] [--batches 1,8]
        [--hist 512,2048,4096] [--turn 1,32,128] [--rounds 7] [--out table.json]

``--kv-dtype fp8``: an fp8 (e4m3fn, no scales) KV-cache arm beside the bf16 arm, same process, same
weights, rounds interleaved: marginal ms per token at ``--prompt`` and at the longest history each
model allows, the decode kernel alone for both caches, and the fp8 cache's logits and greedy
tokens against the bf16 cache's.

    python benchmarks/generate_bench.py --kv-dtype fp8 [--models smollm2,gpt2] [--batches 1,8,32]
        [--prompt 128] [--new 256] [--rounds 7] [--out table.json]

``--shared R``: R samples per prompt over one shared prompt cache (``num_return_sequences=R``)
against the same call on ``ids.repeat_interleave(R, 0)``: same process, same weights, rounds
interleaved.  Per (model, batch, prompt): the bytes of both caches, the time to the first token
(prefill of B against B·R rows) and the marginal ms per token of graphed sampling; per model: the
decode kernel alone over (prefix, own) against the repeated cache.

    python benchmarks/generate_bench.py --shared 8 [--models smollm2,gpt2] [--batches 4]
        [--prompts 128,2048] [--new 128] [--rounds 7] [--out table.json]

``--head-dim 128``: the decode kernel at head dim 128 on a Llama-3.2-3B-shaped stack (hidden 3072, 24
heads on 8 kv heads of 128, ``--layers`` layers, random bf16 weights).  ms per ``decode_step`` with
the HIP kernel against the same call with ``ops.decode.decode_supported`` patched to False (the
PyTorch path these models ran before), bf16 and fp8 caches, at ``--batches`` x ``--hist``; and the
kernel alone against the 64 kernel at equal streamed bytes (same B, G and kv_len, Hkv = h at 128
against 2h at 64).  Both arms in one process, rounds interleaved.

    python benchmarks/generate_bench.py --head-dim 128 [--layers 4] [--batches 1,8,32]
        [--hist 128,4096] [--rounds 7] [--out table.json]

``--continue --head-dim 128``: the time to the first token of turn 2 on that stack — continuing
with the block-append kernel at head dim 128 against the same call with
``ops.decode.append_supported`` patched to False (the PyTorch path) and against the re-prefill of
history + turn — and ``ops.append_attention`` alone against head dim 64 at equal streamed bytes.

    python benchmarks/generate_bench.py --continue --head-dim 128 [--layers 4] [--batches 1,8]
        [--hist 512,2048,4096] [--turn 1,32,128] [--rounds 7] [--out table.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def timed(fn, reps=2):
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t)
    return best


def kernel_bench(rows, kv_dtype=torch.bfloat16):
    from nbdistributed_amd import ops
    from nbdistributed_amd.ops.decode import partials_numel

    out = []
    for B, H, Hkv, T in rows:
        kc = torch.randn(B, Hkv, T, 64, device="cuda").to(torch.bfloat16).to(kv_dtype)
        vc = torch.randn(B, Hkv, T, 64, device="cuda").to(torch.bfloat16).to(kv_dtype)
        qkv = torch.randn(B, (H + 2 * Hkv) * 64, device="cuda").to(torch.bfloat16)
        pos = torch.full((B,), T - 1, device="cuda", dtype=torch.int64)
        ws = torch.empty(partials_numel(B, H, T), dtype=torch.float32, device="cuda")
        f = lambda: ops.decode_attention(qkv, kc, vc, pos, H, workspace=ws)  # noqa: E731
        for _ in range(3):
            f()
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        n = 50
        s.record()
        for _ in range(n):
            f()
        e.record()
        e.synchronize()
        us = s.elapsed_time(e) / n * 1e3
        gbs = 2 * kc.numel() * kc.element_size() / us / 1e3
        r = dict(B=B, H=H, Hkv=Hkv, T=T, us=round(us, 2), cache_GBps=round(gbs, 1))
        if kv_dtype != torch.bfloat16:
            r["kv_dtype"] = str(kv_dtype).replace("torch.", "")
        print(json.dumps(r), flush=True)
        out.append(r)
    return out


def continue_bench(a):
    import statistics

    from nbdistributed_amd.generation import generate
    from nbdistributed_amd.models import GPT2, GPT2Config, SMOLLM2_135M
    from nbdistributed_amd.models.llama import LlamaConfig, LlamaForCausalLM

    hists = [int(x) for x in a.hist.split(",")]
    turns = [int(x) for x in a.turn.split(",")]
    room = max(hists) + max(turns) + 2
    res = {"what": "ms to the first token of turn 2: continue from the cache vs re-prefill of history + turn",
           "dtype": "bf16", "rounds": a.rounds, "points": []}
    for name in a.models.split(","):
        torch.manual_seed(0)
        if name == "smollm2":
            cfg = {k: v for k, v in SMOLLM2_135M.items() if k != "hidden_act"}
            m, vocab = LlamaForCausalLM(LlamaConfig(**cfg)), cfg["vocab_size"]
        else:  # GPT-2 small's shapes with a position table long enough for the histories
            m, vocab = GPT2(GPT2Config(n_positions=-(-room // 128) * 128 + 128)), 50257
        m = m.to("cuda", torch.bfloat16).eval()
        for B in [int(x) for x in a.batches.split(",")]:
            for hist in hists:
                # turn 1 leaves hist - 1 rows in the cache and one pending token: a history of hist tokens
                ids = torch.randint(1, vocab, (B, hist - 8), device="cuda")
                out1, cache = generate(m, ids, 8, t_max=-(-(hist + max(turns) + 2) // 128) * 128, graph=False,
                                       return_cache=True)
                len0, pend0 = cache.lengths.clone(), cache.pending.clone()
                for turn in turns:
                    new = torch.randint(1, vocab, (B, turn), device="cuda")
                    whole = torch.cat([out1, new], 1)

                    def cont():
                        cache.lengths, cache.pending = len0.clone(), pend0.clone()
                        return generate(m, new, 1, cache=cache, graph=False)

                    def full():
                        return generate(m, whole, 1, graph=False)

                    same = bool((cont()[:, -1] == full()[:, -1]).all())  # (also the warm-up of both)
                    tc, tf = [], []
                    for _ in range(a.rounds):  # interleaved: drift hits both arms alike
                        for fn, ts in ((cont, tc), (full, tf)):
                            torch.cuda.synchronize()
                            t = time.perf_counter()
                            fn()
                            torch.cuda.synchronize()
                            ts.append((time.perf_counter() - t) * 1e3)
                    row = dict(model=name, batch=B, history=hist, turn=turn,
                               continue_ms=round(statistics.median(tc), 3), continue_min_ms=round(min(tc), 3),
                               reprefill_ms=round(statistics.median(tf), 3), reprefill_min_ms=round(min(tf), 3),
                               first_token_same=same)
                    row["speedup"] = round(row["reprefill_ms"] / row["continue_ms"], 2)
                    print(json.dumps(row), flush=True)
                    res["points"].append(row)
                del cache
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


def _bench_model(name, room):
    """(model, vocab, position limit, (H, Hkv)): random-init bf16, GPT-2 small or SmolLM2-135M shapes."""
    from nbdistributed_amd.models import GPT2, GPT2Config, SMOLLM2_135M
    from nbdistributed_amd.models.llama import LlamaConfig, LlamaForCausalLM

    torch.manual_seed(0)
    if name == "smollm2":
        cfg = {k: v for k, v in SMOLLM2_135M.items() if k != "hidden_act"}
        m, vocab, limit, heads = LlamaForCausalLM(LlamaConfig(**cfg)), cfg["vocab_size"], min(
            room, cfg["max_position_embeddings"]), (cfg["num_attention_heads"], cfg["num_key_value_heads"])
    else:
        m, vocab, limit, heads = GPT2(GPT2Config.small()), 50257, 1024, (12, 12)
    return m.to("cuda", torch.bfloat16).eval(), vocab, limit, heads


def kv_dtype_bench(a):
    """An fp8 KV-cache arm beside the bf16 arm: same process, same weights, rounds interleaved.
    Per (model, batch, prompt): the marginal ms per token of graphed decoding (two lengths, prefill
    and capture cancel) for both caches; per model: the decode kernel alone at the longest history;
    and the quality of the fp8 cache against the bf16 one over ``--new`` teacher-forced decode steps
    (max |Δlogit|, arg-max agreement) and the free-running greedy tokens."""
    import statistics

    from nbdistributed_amd.generation import KVCache, generate

    arms = (("bf16", None), ("fp8", torch.float8_e4m3fn))
    res = {"what": "decode with an fp8 (e4m3fn, no scales) KV cache vs the bf16 cache: marginal ms per token of "
                   "graphed generate, rounds interleaved", "new_tokens": a.new, "rounds": a.rounds, "points": [],
           "decode_kernel": [], "quality": []}
    for name in a.models.split(","):
        m, vocab, limit, (H, Hkv) = _bench_model(name, a.max_positions)
        longest = limit - (32 + a.new)
        for B in [int(x) for x in a.batches.split(",")]:
            for prompt in sorted({min(a.prompt, longest), longest}):
                ids = torch.randint(1, vocab, (B, prompt), device="cuda")
                outs, ts = {}, {arm: ([], []) for arm, _ in arms}
                for arm, kd in arms:  # warm-up of both lengths; the long run's tokens for the agreement
                    generate(m, ids, 32, graph=True, kv_dtype=kd)
                    outs[arm] = generate(m, ids, 32 + a.new, graph=True, kv_dtype=kd)
                for _ in range(a.rounds):
                    for arm, kd in arms:
                        for n, sink in ((32, ts[arm][0]), (32 + a.new, ts[arm][1])):
                            torch.cuda.synchronize()
                            t = time.perf_counter()
                            generate(m, ids, n, graph=True, kv_dtype=kd)
                            torch.cuda.synchronize()
                            sink.append((time.perf_counter() - t) * 1e3)
                row = dict(model=name, batch=B, prompt=prompt, history_end=prompt + 32 + a.new)
                for arm, _ in arms:
                    per = [(lo - sh) / a.new for sh, lo in zip(*ts[arm])]
                    row[arm + "_ms_per_token"] = round(statistics.median(per), 4)
                    row[arm + "_ms_per_token_min_max"] = [round(min(per), 4), round(max(per), 4)]
                row["fp8_over_bf16"] = round(row["fp8_ms_per_token"] / row["bf16_ms_per_token"], 3)
                same = (outs["bf16"][:, prompt:] == outs["fp8"][:, prompt:]).float()
                row["greedy_tokens_equal_frac"] = round(float(same.mean()), 3)
                row["greedy_tokens_agreeing_prefix_mean"] = round(float(same.cumprod(-1).sum(-1).mean()), 1)
                print(json.dumps(row), flush=True)
                res["points"].append(row)
        # the decode kernel alone, one layer's cache at the longest history
        for B in [int(x) for x in a.batches.split(",")]:
            for dt in (torch.bfloat16, torch.float8_e4m3fn):
                r = kernel_bench([(B, H, Hkv, limit)], dt)[0]
                r["model"] = name
                res["decode_kernel"].append(r)
        # quality, teacher-forced on the bf16 arm's own greedy tokens: both caches see the same inputs
        B, prompt = 8, min(a.prompt, longest)
        ids = torch.randint(1, vocab, (B, prompt), device="cuda")
        seq = generate(m, ids, a.new + 1, graph=True)
        t_pad = m.prefill_length(prompt)
        caches = [KVCache.for_model(m, B, max(t_pad, prompt + a.new + 1), dtype=dt) for dt in (None, torch.float8_e4m3fn)]
        lens = torch.full((B,), prompt, dtype=torch.int64, device="cuda")
        padded = torch.nn.functional.pad(ids, (0, t_pad - prompt))
        for c in caches:
            m.prefill(padded, c, lens)
        dmax, lmax, agree = 0.0, 0.0, 0
        for t in range(prompt, prompt + a.new):
            pos = torch.full((B,), t, dtype=torch.int64, device="cuda")
            l16, l8 = (m.decode_step(seq[:, t], pos, c).float() for c in caches)
            dmax, lmax = max(dmax, float((l16 - l8).abs().max())), max(lmax, float(l16.abs().max()))
            agree += int((l16.argmax(-1) == l8.argmax(-1)).sum())
        q = dict(model=name, batch=B, prompt=prompt, steps=a.new, max_abs_logit_diff=round(dmax, 4),
                 max_abs_logit=round(lmax, 3), argmax_agreement=round(agree / (B * a.new), 4))
        print(json.dumps(q), flush=True)
        res["quality"].append(q)
        del m, caches
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


def shared_kernel_bench(B, R, H, Hkv, Tp, Ts, kv_dtype=torch.bfloat16, n=50, rounds=5):
    """µs of one layer's decode attention at the last position: ``decode_attention_shared`` over
    (prefix [B, Hkv, Tp, 64], own [B·R, Hkv, Ts, 64]) and ``decode_attention`` over the repeated
    cache [B·R, Hkv, Tp + Ts, 64]; rounds of the two interleaved, median and [min, max]."""
    import statistics

    from nbdistributed_amd import ops
    from nbdistributed_amd.ops.decode import partials_numel

    S, T = B * R, Tp + Ts
    mk = lambda *shape: torch.randn(*shape, device="cuda").to(torch.bfloat16).to(kv_dtype)  # noqa: E731
    pk, pv, ok, ov = mk(B, Hkv, Tp, 64), mk(B, Hkv, Tp, 64), mk(S, Hkv, Ts, 64), mk(S, Hkv, Ts, 64)
    kc, vc = mk(S, Hkv, T, 64), mk(S, Hkv, T, 64)
    qkv = torch.randn(S, (H + 2 * Hkv) * 64, device="cuda").to(torch.bfloat16)
    pos = torch.full((S,), T - 1, device="cuda", dtype=torch.int64)
    plen = torch.full((B,), Tp, device="cuda", dtype=torch.int64)
    ws = torch.empty(partials_numel(S, H, T), dtype=torch.float32, device="cuda")
    arms = {"shared": lambda: ops.decode_attention_shared(qkv, pk, pv, plen, ok, ov, pos, R, H, workspace=ws),
            "repeated": lambda: ops.decode_attention(qkv, kc, vc, pos, H, workspace=ws)}
    us = {k: [] for k in arms}
    for f in arms.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, f in arms.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(n):
                f()
            e.record()
            e.synchronize()
            us[k].append(s.elapsed_time(e) / n * 1e3)
    r = dict(B=B, R=R, H=H, Hkv=Hkv, Tp=Tp, Ts=Ts, kv_dtype=str(kv_dtype).replace("torch.", ""))
    for k in arms:
        r[k + "_us"] = round(statistics.median(us[k]), 2)
        r[k + "_us_min_max"] = [round(min(us[k]), 2), round(max(us[k]), 2)]
    r["shared_over_repeated"] = round(r["shared_us"] / r["repeated_us"], 3)
    r["bytes_addressed"] = dict(shared_distinct=2 * (pk.numel() + ok.numel()) * pk.element_size(),
                                repeated=2 * kc.numel() * kc.element_size())
    print(json.dumps(r), flush=True)
    return r


def shared_bench(a):
    """R samples per prompt over one shared prompt cache against the same call on repeated prompts.
    The yardstick is the repeated arm of the same run; its own [min, max] is the margin."""
    import statistics

    from nbdistributed_amd.generation import generate

    R = a.shared
    res = {"what": f"generate(num_return_sequences={R}) over one shared prompt cache vs the same call on "
                   f"ids.repeat_interleave({R}, 0): bf16, sampling at temperature 1, graphed decode, rounds interleaved",
           "R": R, "new_tokens": a.new, "rounds": a.rounds, "points": [], "decode_kernel": []}
    for name in a.models.split(","):
        m, vocab, limit, (H, Hkv) = _bench_model(name, a.max_positions)
        longest = limit - (32 + a.new)
        prompts = sorted({min(int(x), longest) for x in a.prompts.split(",")})
        for B in [int(x) for x in a.batches.split(",")]:
            for prompt in prompts:
                ids = torch.randint(1, vocab, (B, prompt), device="cuda")
                rep = ids.repeat_interleave(R, 0)
                arms = (("shared", lambda n, **kw: generate(m, ids, n, temperature=1.0, graph=True,
                                                            num_return_sequences=R, **kw)),
                        ("repeated", lambda n, **kw: generate(m, rep, n, temperature=1.0, graph=True, **kw)))
                row = dict(model=name, batch=B, R=R, prompt=prompt, prefill_length=m.prefill_length(prompt))
                ts = {arm: ([], [], []) for arm, _ in arms}
                for arm, fn in arms:  # warm-up of every length, and the caches
                    fn(1)
                    fn(32)
                    out, cache = fn(32 + a.new, return_cache=True)
                    row[arm + "_cache_bytes"] = cache.nbytes
                    row[arm + "_rows_out"] = out.shape[0]
                    del cache
                for _ in range(a.rounds):
                    for arm, fn in arms:
                        for n, sink in zip((1, 32, 32 + a.new), ts[arm]):
                            torch.cuda.synchronize()
                            t = time.perf_counter()
                            fn(n)
                            torch.cuda.synchronize()
                            sink.append((time.perf_counter() - t) * 1e3)
                for arm, _ in arms:
                    first, short, long_ = ts[arm]
                    per = [(lo - sh) / a.new for sh, lo in zip(short, long_)]
                    row[arm + "_first_token_ms"] = round(statistics.median(first), 3)
                    row[arm + "_first_token_ms_min_max"] = [round(min(first), 3), round(max(first), 3)]
                    row[arm + "_ms_per_token"] = round(statistics.median(per), 4)
                    row[arm + "_ms_per_token_min_max"] = [round(min(per), 4), round(max(per), 4)]
                row["cache_bytes_ratio"] = round(row["shared_cache_bytes"] / row["repeated_cache_bytes"], 4)
                row["first_token_speedup"] = round(row["repeated_first_token_ms"] / row["shared_first_token_ms"], 2)
                row["shared_over_repeated_ms_per_token"] = round(row["shared_ms_per_token"] / row["repeated_ms_per_token"], 3)
                print(json.dumps(row), flush=True)
                res["points"].append(row)
        for B in [int(x) for x in a.batches.split(",")]:
            for prompt in prompts:
                r = shared_kernel_bench(B, R, H, Hkv, m.prefill_length(prompt), 32 + a.new)
                r["model"] = name
                res["decode_kernel"].append(r)
        del m
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


def head_dim_bench(a):
    """Head dim 128 in the decode kernel: a model-level arm against the PyTorch fallback and a
    kernel-alone arm against the 64 kernel at equal streamed bytes (see the module docstring)."""
    import contextlib
    import statistics
    from unittest import mock

    from nbdistributed_amd import ops
    from nbdistributed_amd.generation import KVCache
    from nbdistributed_amd.models.llama import LlamaConfig, LlamaForCausalLM
    from nbdistributed_amd.ops.decode import partials_numel

    D = a.head_dim
    med = lambda xs: round(statistics.median(xs), 4)  # noqa: E731
    span = lambda xs: [round(min(xs), 4), round(max(xs), 4)]  # noqa: E731
    res = {"what": f"decode attention at head dim {D}: Llama-3.2-3B-shaped stack of {a.layers} layers (hidden 3072, 24 / 8 "
                   f"heads), random bf16 weights, eager decode_step; HIP kernel vs decode_supported patched to False; "
                   f"and the kernel alone vs the 64 kernel at equal streamed bytes; rounds interleaved",
           "layers": a.layers, "rounds": a.rounds, "model": [], "kernel": []}
    torch.manual_seed(0)
    cfg = LlamaConfig(vocab_size=32000, hidden_size=3072, intermediate_size=8192, num_hidden_layers=a.layers,
                      num_attention_heads=24, num_key_value_heads=8, max_position_embeddings=8192, explicit_head_dim=D)
    m = LlamaForCausalLM(cfg).to("cuda", torch.bfloat16).eval()
    hists = [int(x) for x in a.hist.split(",")]
    batches = [int(x) for x in a.batches.split(",")]
    steps = 8
    for kv in (torch.bfloat16, torch.float8_e4m3fn):
        for B in batches:
            for hist in hists:
                cache = KVCache.for_model(m, B, hist + 64, dtype=kv)  # a random history: no prefill needed
                for t in (cache.k, cache.v):
                    t.copy_(torch.randn(t.shape, device="cuda", dtype=torch.bfloat16).to(kv))
                tok = torch.randint(1, 32000, (B,), device="cuda")
                pos = torch.full((B,), hist, device="cuda", dtype=torch.int64)

                def run():
                    for i in range(steps):
                        m.decode_step(tok, pos + i, cache)

                ms = {"hip": [], "fallback": []}
                for _ in range(a.rounds + 1):  # the first round warms up
                    for arm in ("hip", "fallback"):
                        with (mock.patch.object(ops.decode, "decode_supported", lambda *x: False) if arm == "fallback"
                              else contextlib.nullcontext()):
                            torch.cuda.synchronize()
                            t0 = time.perf_counter()
                            run()
                            torch.cuda.synchronize()
                            ms[arm].append((time.perf_counter() - t0) * 1e3 / steps)
                row = dict(kv_dtype=str(kv).replace("torch.", ""), batch=B, history=hist)
                for arm in ms:
                    row[arm + "_ms_per_token"], row[arm + "_min_max"] = med(ms[arm][1:]), span(ms[arm][1:])
                row["fallback_over_hip"] = round(row["fallback_ms_per_token"] / row["hip_ms_per_token"], 2)
                print(json.dumps(row), flush=True)
                res["model"].append(row)
                del cache
                torch.cuda.empty_cache()
    del m
    torch.cuda.empty_cache()
    # the kernel alone: 128 with Hkv = h against 64 with Hkv = 2h (the same K + V bytes), same B, G, kv_len
    for kv in (torch.bfloat16, torch.float8_e4m3fn):
        for B in batches:
            for T in hists:
                for G, h in ((3, 8), (1, 8), (4, 8)):
                    fns = {}
                    for d, hk in ((D, h), (64, 2 * h)):
                        H = G * hk
                        kc = torch.randn(B, hk, T, d, device="cuda").to(torch.bfloat16).to(kv)
                        vc = torch.randn(B, hk, T, d, device="cuda").to(torch.bfloat16).to(kv)
                        qkv = torch.randn(B, (H + 2 * hk) * d, device="cuda").to(torch.bfloat16)
                        p = torch.full((B,), T - 1, device="cuda", dtype=torch.int64)
                        ws = torch.empty(partials_numel(B, H, T, d), dtype=torch.float32, device="cuda")
                        fns[d] = (lambda qkv=qkv, kc=kc, vc=vc, p=p, H=H, ws=ws: ops.decode_attention(qkv, kc, vc, p, H, workspace=ws))
                        for _ in range(3):
                            fns[d]()
                    torch.cuda.synchronize()
                    us = {d: [] for d in fns}
                    n = 50
                    for _ in range(a.rounds):
                        for d, f in fns.items():
                            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            s.record()
                            for _ in range(n):
                                f()
                            e.record()
                            e.synchronize()
                            us[d].append(s.elapsed_time(e) / n * 1e3)
                    ratios = [x / y for x, y in zip(us[D], us[64])]
                    row = dict(kv_dtype=str(kv).replace("torch.", ""), B=B, G=G, kv_len=T, Hkv_128=h, Hkv_64=2 * h,
                               bytes=2 * B * h * T * D * (1 if kv != torch.bfloat16 else 2),
                               us_128=round(statistics.median(us[D]), 2), us_64=round(statistics.median(us[64]), 2),
                               ratio_128_over_64=round(statistics.median(ratios), 3), ratio_min_max=span(ratios))
                    print(json.dumps(row), flush=True)
                    res["kernel"].append(row)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


def head_dim_continue_bench(a):
    """``--continue --head-dim 128``: the time to the first token of turn 2 on the Llama-3.2-3B-shaped
    stack of ``head_dim_bench``, three arms in one process with their rounds interleaved —
    (a) ``generate(turn, 1, cache=cache)`` with the block-append kernel, (b) the same call with
    ``ops.decode.append_supported`` patched to False (the PyTorch path head dim 128 ran before),
    (c) ``generate(history + turn, 1)``, the re-prefill — and ``ops.append_attention`` alone (both
    launches) at 128 against 64 at equal streamed bytes (Hkv = h at 128, 2h at 64; same B, G, Tn, start)."""
    import contextlib
    import statistics
    from unittest import mock

    from nbdistributed_amd import ops
    from nbdistributed_amd.generation import generate
    from nbdistributed_amd.models.llama import LlamaConfig, LlamaForCausalLM

    D = a.head_dim
    med = lambda xs: round(statistics.median(xs), 3)  # noqa: E731
    span = lambda xs: [round(min(xs), 3), round(max(xs), 3)]  # noqa: E731
    hists = [int(x) for x in a.hist.split(",")]
    turns = [int(x) for x in a.turn.split(",")]
    batches = [int(x) for x in a.batches.split(",")]
    res = {"what": f"ms to the first token of turn 2 at head dim {D}: Llama-3.2-3B-shaped stack of {a.layers} layers (hidden "
                   f"3072, 24 / 8 heads), random bf16 weights, eager; (a) continue with the block-append kernel, (b) the "
                   f"same call with append_supported patched to False, (c) re-prefill of history + turn; and "
                   f"ops.append_attention alone at {D} vs 64 at equal streamed bytes; rounds interleaved",
           "layers": a.layers, "rounds": a.rounds, "points": [], "kernel": []}
    torch.manual_seed(0)
    vocab = 32000
    cfg = LlamaConfig(vocab_size=vocab, hidden_size=3072, intermediate_size=8192, num_hidden_layers=a.layers,
                      num_attention_heads=24, num_key_value_heads=8, max_position_embeddings=8192, explicit_head_dim=D)
    m = LlamaForCausalLM(cfg).to("cuda", torch.bfloat16).eval()
    off = lambda: mock.patch.object(ops.decode, "append_supported", lambda *x: False)  # noqa: E731
    for B in batches:
        for hist in hists:
            # turn 1 leaves hist - 1 rows in the cache and one pending token: a history of hist tokens
            ids = torch.randint(1, vocab, (B, hist - 8), device="cuda")
            out1, cache = generate(m, ids, 8, t_max=-(-(hist + max(turns) + 2) // 128) * 128, graph=False, return_cache=True)
            len0, pend0 = cache.lengths.clone(), cache.pending.clone()
            assert ops.append_supported(torch.zeros(1, 1, 1, dtype=torch.bfloat16, device="cuda"), cache.k[0], 24)
            for turn in turns:
                new = torch.randint(1, vocab, (B, turn), device="cuda")
                whole = torch.cat([out1, new], 1)

                def cont(patched=False):
                    cache.lengths, cache.pending = len0.clone(), pend0.clone()
                    with off() if patched else contextlib.nullcontext():
                        return generate(m, new, 1, cache=cache, graph=False)

                arms = (("kernel", cont), ("fallback", lambda: cont(True)),
                        ("reprefill", lambda: generate(m, whole, 1, graph=False)))
                first = {name: fn()[:, -1] for name, fn in arms}  # (also the warm-up of every arm)
                ms = {name: [] for name, _ in arms}
                for _ in range(a.rounds):  # interleaved: drift hits the arms alike
                    for name, fn in arms:
                        torch.cuda.synchronize()
                        t = time.perf_counter()
                        fn()
                        torch.cuda.synchronize()
                        ms[name].append((time.perf_counter() - t) * 1e3)
                row = dict(batch=B, history=hist, turn=turn)
                for name, _ in arms:
                    row[name + "_ms"], row[name + "_min_max"] = med(ms[name]), span(ms[name])
                for name in ("fallback", "reprefill"):
                    r = [x / y for x, y in zip(ms[name], ms["kernel"])]  # per round: the arms ran back to back
                    row[name + "_over_kernel"], row[name + "_over_kernel_min_max"] = med(r), span(r)
                row["first_token_same_as_fallback"] = bool((first["kernel"] == first["fallback"]).all())
                row["first_token_same_as_reprefill"] = bool((first["kernel"] == first["reprefill"]).all())
                print(json.dumps(row), flush=True)
                res["points"].append(row)
            del cache
            torch.cuda.empty_cache()
    del m
    torch.cuda.empty_cache()
    G, h = 3, 8
    for B in batches:
        for hist in hists:
            for turn in turns:
                Tn, Tmax = turn + 1, -(-(hist + max(turns) + 2) // 128) * 128
                fns = {}
                for d, hk in ((D, h), (64, 2 * h)):
                    H = G * hk
                    kc = torch.randn(B, hk, Tmax, d, device="cuda").to(torch.bfloat16)
                    vc = torch.randn(B, hk, Tmax, d, device="cuda").to(torch.bfloat16)
                    qkv = torch.randn(B, Tn, (H + 2 * hk) * d, device="cuda").to(torch.bfloat16)
                    st = torch.full((B,), hist - 1, device="cuda", dtype=torch.int64)
                    nn = torch.full((B,), Tn, device="cuda", dtype=torch.int64)
                    rope = ops.rope_tables(Tmax, d, 10000.0, "cuda")
                    fns[d] = (lambda qkv=qkv, kc=kc, vc=vc, st=st, nn=nn, H=H, rope=rope:
                              ops.append_attention(qkv, kc, vc, st, nn, H, rope=rope, kv_len_max=hist + Tn))
                    for _ in range(3):
                        fns[d]()
                torch.cuda.synchronize()
                us = {d: [] for d in fns}
                n = 20
                for _ in range(a.rounds):
                    for d, f in fns.items():
                        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        s.record()
                        for _ in range(n):
                            f()
                        e.record()
                        e.synchronize()
                        us[d].append(s.elapsed_time(e) / n * 1e3)
                ratios = [x / y for x, y in zip(us[D], us[64])]
                row = dict(B=B, G=G, history=hist, Tn=Tn, Hkv_128=h, Hkv_64=2 * h, cache_bytes_read=2 * B * h * (hist + Tn - 1) * D * 2,
                           us_128=round(statistics.median(us[D]), 2), us_64=round(statistics.median(us[64]), 2),
                           ratio_128_over_64=round(statistics.median(ratios), 3), ratio_min_max=span(ratios))
                print(json.dumps(row), flush=True)
                res["kernel"].append(row)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--head-dim", dest="head_dim", type=int, default=0, choices=[0, 128],
                    help="the head-dim-128 decode arm, with --continue the head-dim-128 multi-turn arm (see the module "
                         "docstring): --layers, --batches, --hist, --rounds")
    ap.add_argument("--layers", type=int, default=4, help="--head-dim: layers of the Llama-3.2-3B-shaped stack")
    ap.add_argument("--shared", type=int, default=0, metavar="R",
                    help="R samples per prompt over one shared prompt cache vs repeated prompts: --models, --batches "
                         "(default 4), --prompts, --new (default 128), --rounds")
    ap.add_argument("--prompts", default="128,2048", help="--shared: prompt lengths (capped by the model's positions)")
    ap.add_argument("--kv-dtype", dest="kv_dtype", default=None, choices=["fp8"],
                    help="add an fp8 KV-cache arm beside the bf16 arm (same process, same weights): --models, "
                         "--batches, --prompt and the longest history each model allows, --new, --rounds")
    ap.add_argument("--max-positions", type=int, default=8192, help="--kv-dtype: cap on the longest history")
    ap.add_argument("--continue", dest="cont", action="store_true", help="the multi-turn arm (see the module docstring)")
    ap.add_argument("--models", default="smollm2,gpt2")
    ap.add_argument("--hist", default="512,2048,4096")
    ap.add_argument("--turn", default="1,32,128")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--prompt", type=int, default=128)
    ap.add_argument("--new", type=int, default=256)
    ap.add_argument("--no-hf", action="store_true")
    ap.add_argument("--model", default="gpt2", choices=["gpt2", "smollm2"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from nbdistributed_amd import ops
    from nbdistributed_amd.models import GPT2, GPT2Config

    ops.load_library()
    if a.head_dim and a.cont:
        if a.batches == "1,8,32":
            a.batches = "1,8"
        return head_dim_continue_bench(a)
    if a.head_dim:
        if a.hist == "512,2048,4096":
            a.hist = "128,4096"
        return head_dim_bench(a)
    if a.shared:
        if a.batches == "1,8,32":
            a.batches = "4"
        if a.new == 256:
            a.new = 128
        return shared_bench(a)
    if a.kv_dtype:
        return kv_dtype_bench(a)
    if a.cont:
        if a.batches == "1,8,32":
            a.batches = "1,8"
        return continue_bench(a)
    torch.manual_seed(0)
    hf = None
    if a.model == "smollm2":
        # SmolLM2-135M architecture (random init), built in HF and converted (models.llama.from_hf)
        from transformers import LlamaConfig as HLC, LlamaForCausalLM as HLM

        from nbdistributed_amd.models import SMOLLM2_135M
        from nbdistributed_amd.models.llama import from_hf

        cfg = dict(SMOLLM2_135M)
        cfg.pop("hidden_act", None)
        hf = HLM(HLC(**cfg)).to(torch.bfloat16)
        m = from_hf(hf).to("cuda").eval()
        hf = None if a.no_hf else hf.to("cuda").eval()
        vocab, name = cfg["vocab_size"], "SmolLM2-135M (random init)"
    else:
        m = GPT2(GPT2Config.small()).to("cuda", torch.bfloat16).eval()
        vocab, name = 50257, "gpt2-small (124M, random init)"
    if a.model == "gpt2" and not a.no_hf:
        try:
            from transformers import GPT2Config as HFC, GPT2LMHeadModel

            hf = GPT2LMHeadModel(HFC(n_embd=768, n_layer=12, n_head=12, n_positions=1024, vocab_size=50257))
            sd = {}
            for k, v in m.state_dict().items():  # nn.Linear [out, in] -> HF Conv1D [in, out]
                kk = "transformer." + k if not k.startswith("lm_head") else k
                if any(s in k for s in ("c_attn.weight", "c_proj.weight", "c_fc.weight")):
                    v = v.t()
                sd[kk] = v
            hf.load_state_dict(sd, strict=False)
            hf = hf.to("cuda", torch.bfloat16).eval()
        except Exception as e:  # pragma: no cover
            print("HF baseline unavailable:", e, flush=True)
    res = {"model": name, "dtype": "bf16", "prompt": a.prompt, "new_tokens": a.new, "runs": []}
    for B in [int(x) for x in a.batches.split(",")]:
        ids = torch.randint(1, vocab, (B, a.prompt), device="cuda")
        row = {"batch": B}
        g_out = None
        for name, kw in (("nbd_graph", dict(graph=True)), ("nbd_eager", dict(graph=False))):
            holder = {}
            t = timed(lambda: holder.__setitem__("o", m.generate(ids, a.new, **kw)))
            row[name + "_tok_per_s"] = round(B * a.new / t, 1)
            row[name + "_ms_per_token"] = round(t / a.new * 1e3, 3)
            if name == "nbd_graph":
                g_out = holder["o"]
        # steady-state decode cost: the marginal time per token between two lengths (prefill,
        # cache allocation and graph capture cancel out)
        t_short = timed(lambda: m.generate(ids, 32, graph=True))
        t_long = timed(lambda: m.generate(ids, 32 + a.new, graph=True))
        row["nbd_graph_marginal_ms_per_token"] = round((t_long - t_short) / a.new * 1e3, 3)
        row["nbd_graph_marginal_tok_per_s"] = round(B * a.new / (t_long - t_short), 1)
        if hf is not None:
            holder = {}
            t = timed(lambda: holder.__setitem__("o", hf.generate(ids, attention_mask=torch.ones_like(ids),
                                                                   max_new_tokens=a.new, min_new_tokens=a.new,
                                                                   do_sample=False, use_cache=True, pad_token_id=0)))
            row["hf_tok_per_s"] = round(B * a.new / t, 1)
            row["hf_ms_per_token"] = round(t / a.new * 1e3, 3)
            row["speedup_vs_hf"] = round(row["nbd_graph_tok_per_s"] / row["hf_tok_per_s"], 2)
            # greedy tokens agree until the first bf16 near-tie
            same = (holder["o"][:, a.prompt:] == g_out[:, a.prompt:]).float().cumprod(-1).sum(-1)
            row["tokens_agreeing_with_hf_mean"] = round(float(same.mean()), 1)
        print(json.dumps(row), flush=True)
        res["runs"].append(row)
    if a.model != "gpt2":
        if a.out:
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
        return
    res["decode_kernel"] = kernel_bench([(1, 12, 12, 1024), (8, 12, 12, 1024), (32, 12, 12, 1024), (8, 32, 8, 8192),
                                         (1, 32, 8, 32768), (64, 12, 12, 2048)])
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
