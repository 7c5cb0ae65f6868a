"""Plain-PyTorch reference of the block-append attention op (``ops.append_attention``,
csrc/kernels/append.hip), in the conventions of tests/refmath.py: an fp64 formula, an emulation
of the kernel's rounding points (``emulate=True``), deliberately wrong mutants, and structured
inputs whose cache rows past ``start`` hold poison.  Never touches ``torch.ops.nbd``.

The op: sequence b appends ``nnew[b]`` new tokens (rows of the packed projection ``qkv[b]``; rows
past it are padding) to a cache holding ``start[b]`` rows.  Token i gets position start[b] + i:
its k (rotated there) and v become that cache row, its query (rotated there) attends rows
0..start[b] + i.

Rounding points of the kernel (``emulate=True``), and nothing else: bf16 inputs; the rotated q
and k rounded to bf16 (k is *stored* as bf16 and read back); the raw score an fp32 accumulator
over four 16-dim MFMA steps; the deferred-rescale running maximum per 32-query wave and 64-key
tile; P rounded to bf16 before P·V; l summed in fp32; the output rounded to bf16.  (A wave's
padding lanes are modelled as copies of its last valid query — in the kernel they carry the
padding rows' own data, which can move a rescale decision, not the size of the rounding.)
"""
import math

import torch

import refmath as rm

APPEND_MUTANTS = ("mask_plus1", "mask_minus1", "rope_local", "write_local", "gqa_mod", "pad_row_live")
D = 64


def _attend(q, kx, vx, vis, scale, emulate):
    """softmax(q·kxᵀ·scale, keys where ``vis``)·vx for q [H, n, D], kx / vx [H, S, D], vis [n, S]."""
    bf = torch.bfloat16
    masked = ~vis
    if not emulate:
        s2 = (q @ kx.transpose(-1, -2) * (scale * rm.LOG2E)).masked_fill(masked, -math.inf)
        p = torch.exp2(s2 - s2.amax(-1, keepdim=True))
        return (p @ vx) / p.sum(-1, keepdim=True)
    H, n, _ = q.shape
    S = kx.shape[1]
    pad = (-n) % 32
    if pad:  # the wave's padding lanes: the last valid query once more
        q = torch.cat([q, q[:, -1:].expand(H, pad, D)], 1)
        masked = torch.cat([masked, masked[-1:].expand(pad, S)], 0)
    n32 = n + pad
    sraw = torch.zeros(H, n32, S, dtype=torch.float64)
    for d0 in range(0, D, 16):  # `sacc[kb] = mfma(..., qf[s], sacc[kb])`: fp32 over four k-steps
        sraw = rm._f32(sraw + q[..., d0:d0 + 16] @ kx[..., d0:d0 + 16].transpose(-1, -2))
    c2 = float(torch.tensor(scale, dtype=torch.float32) * torch.tensor(rm.LOG2E, dtype=torch.float32))
    s2 = (sraw * c2).masked_fill(masked, -math.inf)
    run = torch.full((H, n32, 1), -math.inf, dtype=torch.float64)
    mt = torch.empty_like(s2)
    l = torch.zeros_like(run)
    for t0 in range(0, S, 64):  # `if (__any(mn > m + kDeferLog2))` per wave of 32 queries and 64-key tile
        mn = torch.maximum(run, rm._f32(s2[..., t0:t0 + 64].amax(-1, keepdim=True)))
        grow = (mn > run + 4.0).reshape(H, n32 // 32, 32).any(-1, keepdim=True)
        new = torch.where(grow.expand(H, n32 // 32, 32).reshape(H, n32, 1), mn, run)
        alpha = torch.where(new > run, torch.exp2(run - new), torch.ones_like(run))
        run = new
        mt[..., t0:t0 + 64] = run
        pt = torch.exp2(rm._f32(sraw[..., t0:t0 + 64] * c2 - run).masked_fill(masked[..., t0:t0 + 64], -math.inf))
        l = rm._f32(rm._f32(l * alpha) + pt.float().sum(-1, keepdim=True).double())
    p = torch.exp2(rm._f32(sraw * c2 - mt).masked_fill(masked, -math.inf))
    wt = torch.exp2(mt - run)  # the later rescales of what a tile added to O
    out = ((rm._rd(p, bf) * wt) @ vx) / l  # P packed to bf16 for O += V^T·P (pack_half)
    return rm._rd(out, bf)[:, :n]


def append_ref(qkv, k_cache, v_cache, start, nnew, n_head, scale, rope=None, *, emulate=False, mutant=None):
    """Returns ``out`` [B, Tn, H·64] (zeros on padding rows) and the updated caches, all fp64.
    ``start`` / ``nnew``: sequences of ints (valid: start + nnew <= Tmax, 1 <= nnew <= Tn)."""
    assert mutant is None or mutant in APPEND_MUTANTS, mutant
    bf = torch.bfloat16
    B, Tn, W = qkv.shape
    Hkv, Tmax = k_cache.shape[1], k_cache.shape[2]
    H, G = n_head, n_head // Hkv
    x = qkv.double().cpu()
    kc, vc = k_cache.double().cpu().clone(), v_cache.double().cpu().clone()
    if emulate:
        x = rm._rd(x, bf)
    out = torch.zeros(B, Tn, H * D, dtype=torch.float64)
    hmap = torch.arange(H) % Hkv if mutant == "gqa_mod" else torch.arange(H) // G
    for b in range(B):
        s0, n = int(start[b]), int(nnew[b])
        assert 1 <= n <= Tn and 0 <= s0 and s0 + n <= Tmax, (s0, n)
        rows = Tn if mutant == "pad_row_live" else n  # pad_row_live: the padding rows' k / v land in the cache too
        rows = min(rows, Tmax - s0)
        i = torch.arange(rows)
        q = x[b, :rows, : H * D].reshape(rows, H, D).transpose(0, 1)
        k = x[b, :rows, H * D:(H + Hkv) * D].reshape(rows, Hkv, D).transpose(0, 1)
        v = x[b, :rows, (H + Hkv) * D:].reshape(rows, Hkv, D).transpose(0, 1)
        if rope is not None:
            cos, sin = rope[0].double().cpu(), rope[1].double().cpu()
            rpos = i if mutant == "rope_local" else s0 + i  # rope_local: rotated at i, not at start + i
            q, k = rm.rot(q, cos, sin, rpos), rm.rot(k, cos, sin, rpos)
            if emulate:  # rope8: the rotated q / k go back to bf16 (k into the cache)
                q, k = rm._rd(q, bf), rm._rd(k, bf)
        wpos = i if mutant == "write_local" else s0 + i  # write_local: row i, not start + i
        kc[b, :, wpos] = k
        vc[b, :, wpos] = v
        S = s0 + n
        j = torch.arange(S)[None, :]
        last = s0 + torch.arange(n)[:, None]
        if mutant == "mask_plus1":
            last = last + 1
            S1 = min(S + 1, Tmax)  # the last query now reads one row past the sequence
            j = torch.arange(S1)[None, :]
            S = S1
        elif mutant == "mask_minus1":
            last = (last - 1).clamp(min=0)  # (key 0 stays: an empty row is a different failure)
        vis = j <= last
        o = _attend(q[:, :n], kc[b, hmap, :S], vc[b, hmap, :S], vis, scale, emulate)  # [H, n, D]
        out[b, :n] = o.transpose(0, 1).reshape(n, H * D)
    if emulate:
        kc = torch.where(kc.isnan(), kc, rm._rd(kc, bf))
    return out, kc, vc


def per_head(out, n_head):
    """[B, Tn, H·64] -> [B, H, Tn, 64]: ``refmath.tile_rel(..., rows=32)`` then scores one wave's rows of one head."""
    B, Tn, _ = out.shape
    return out.reshape(B, Tn, n_head, D).transpose(1, 2)


def append_inputs(B, H, Hkv, Tn, Tmax, start, seed, poison="loud", gain=2.0):
    """bf16 qkv [B, Tn, (H + 2·Hkv)·64] and caches [B, Hkv, Tmax, 64], seeded on the CPU.  q, k, v
    as ``refmath.attn_inputs`` draws them (a per-head mean on k and v, scores a few nats wide, so
    single keys carry weight) — for every row of qkv, the padding rows included, and for the
    cache's history rows < start[b].  Cache rows >= start[b] hold poison:
      ``loud``  k = ±30 (scores tens of nats above or below every legitimate one), v = ±1024 — a
                wrong formula that reads one of them stays finite and moves the result by orders
                of magnitude (the CPU mutant proof);
      ``huge``  ±3e38, the largest finite bf16 magnitudes;
      ``nan``   NaN."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    q = gain * torch.randn(B, Tn, H, D, generator=g)
    kmean, vmean = 0.5 * torch.randn(B, 1, Hkv, D, generator=g), torch.randn(B, 1, Hkv, D, generator=g)
    k = gain * torch.randn(B, Tn, Hkv, D, generator=g) + kmean
    v = torch.randn(B, Tn, Hkv, D, generator=g) + vmean
    qkv = torch.cat([q.reshape(B, Tn, -1), k.reshape(B, Tn, -1), v.reshape(B, Tn, -1)], -1).bfloat16()
    kc = gain * torch.randn(B, Hkv, Tmax, D, generator=g) + kmean.transpose(1, 2)
    vc = torch.randn(B, Hkv, Tmax, D, generator=g) + vmean.transpose(1, 2)
    sign = torch.where(torch.rand(2, B, Hkv, Tmax, D, generator=g) < 0.5, -1.0, 1.0)
    kp, vp = {"loud": (30.0, 1024.0), "huge": (3.0e38, 3.0e38), "nan": (math.nan, math.nan)}[poison]
    free = torch.arange(Tmax)[None, :] >= torch.as_tensor(start)[:, None]  # [B, Tmax]
    free = free[:, None, :, None]
    kc = torch.where(free, kp * sign[0], kc)
    vc = torch.where(free, vp * sign[1], vc)
    return qkv, kc.bfloat16(), vc.bfloat16()
