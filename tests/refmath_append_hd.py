"""Head-dim-generic references of the block-append attention op (csrc/kernels/append.hip
``append_kv_kernel<D>`` / ``append_attn_kernel<D>``, D = 64 | 128), in the conventions of
tests/refmath_append.py, which fixes D = 64: an fp64 formula, an emulation of the kernel's rounding
points (``emulate=True``), deliberately wrong mutants, and structured inputs whose cache rows past
``start`` hold poison.  Never touches ``torch.ops.nbd``; everything is seeded on the CPU.  At head
dim 64 every function here returns what its fixed-width twin returns, bit for bit
(tests/test_append_hd_ref.py), so there is one reference.

The rounding points are those listed in tests/refmath_append.py; the one that follows the head dim
is the raw score, an fp32 accumulator over D/16 16-dim MFMA steps.  The softmax scale is D ** -0.5.

Mutants a 128 kernel can be where a 64 one cannot (``HD_MUTANTS``):
  ``score_half_dims``      the score over four of the eight MFMA k-steps: dims 0 .. 63 only;
  ``rope_partner_32``      the RoPE partner of dim d taken at d ^ 32 (fragment s with s ^ 2), the
                           sign from d mod 64 < 32;
  ``rope_table_stride32``  the tables read as [T, 32]: the angle of (pos, i) taken at flat index
                           32·pos + i;
  ``out_high_zero``        output dims 64 .. D-1 zero (two of the four O tiles stored);
  ``out_high_neighbour``   output dims 64 .. D-1 taken from the next head's dims 0 .. 63 (a head
                           stride of 64 in the output row);
  ``k_write_half``         k written to the cache for dims 0 .. 63 only: dims 64 .. D-1 of the new
                           rows keep what the cache held;
  ``v_high_from_k``        the upper half of a new v row taken from the upper half of the token's
                           (unrotated) k.
"""
import math

import torch

import refmath as rm
import refmath_append as ra
import refmath_decode_hd as dh

HD_MUTANTS = ("score_half_dims", "rope_partner_32", "rope_table_stride32", "out_high_zero", "out_high_neighbour",
              "k_write_half", "v_high_from_k")
APPEND_MUTANTS = ra.APPEND_MUTANTS + HD_MUTANTS


def scale_of(head_dim):
    return head_dim ** -0.5


def _attend(q, kx, vx, vis, scale, emulate, dims=None):
    """``refmath_append._attend`` at q's head dim: softmax(q·kxᵀ·scale, keys where ``vis``)·vx for
    q [H, n, D], kx / vx [H, S, D], vis [n, S].  ``dims``: the score over dims [0, dims) only."""
    bf = torch.bfloat16
    D = q.shape[-1]
    DS = D if dims is None else dims
    masked = ~vis
    if not emulate:
        s2 = (q[..., :DS] @ kx[..., :DS].transpose(-1, -2) * (scale * rm.LOG2E)).masked_fill(masked, -math.inf)
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
    for d0 in range(0, DS, 16):  # `sacc[kb] = mfma(..., qf[s], sacc[kb])`: fp32 over D/16 k-steps
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
    """``refmath_append.append_ref`` at the caches' head dim: ``out`` [B, Tn, H·D] (zeros on padding
    rows) and the updated caches, all fp64.  ``start`` / ``nnew``: sequences of ints (valid:
    start + nnew <= Tmax, 1 <= nnew <= Tn)."""
    assert mutant is None or mutant in APPEND_MUTANTS, mutant
    bf = torch.bfloat16
    B, Tn, W = qkv.shape
    Hkv, Tmax, D = k_cache.shape[1], k_cache.shape[2], k_cache.shape[3]
    H, G = n_head, n_head // Hkv
    assert W == (H + 2 * Hkv) * D, (W, H, Hkv, D)
    x = qkv.double().cpu()
    kc, vc = k_cache.double().cpu().clone(), v_cache.double().cpu().clone()
    if emulate:
        x = rm._rd(x, bf)
    out = torch.zeros(B, Tn, H * D, dtype=torch.float64)
    hmap = torch.arange(H) % Hkv if mutant == "gqa_mod" else torch.arange(H) // G
    rmut = mutant if mutant in ("rope_partner_32", "rope_table_stride32") else None
    for b in range(B):
        s0, n = int(start[b]), int(nnew[b])
        assert 1 <= n <= Tn and 0 <= s0 and s0 + n <= Tmax, (s0, n)
        rows = Tn if mutant == "pad_row_live" else n  # pad_row_live: the padding rows' k / v land in the cache too
        rows = min(rows, Tmax - s0)
        i = torch.arange(rows)
        q = x[b, :rows, : H * D].reshape(rows, H, D).transpose(0, 1)
        k = x[b, :rows, H * D:(H + Hkv) * D].reshape(rows, Hkv, D).transpose(0, 1)
        v = x[b, :rows, (H + Hkv) * D:].reshape(rows, Hkv, D).transpose(0, 1)
        if mutant == "v_high_from_k":
            v = torch.cat([v[..., :64], k[..., 64:]], -1)
        if rope is not None:
            cos, sin = rope[0].double().cpu(), rope[1].double().cpu()
            rpos = i if mutant == "rope_local" else s0 + i  # rope_local: rotated at i, not at start + i
            q, k = dh.rot(q, cos, sin, rpos, rmut), dh.rot(k, cos, sin, rpos, rmut)
            if emulate:  # rope8: the rotated q / k go back to bf16 (k into the cache)
                q, k = rm._rd(q, bf), rm._rd(k, bf)
        wpos = i if mutant == "write_local" else s0 + i  # write_local: row i, not start + i
        if mutant == "k_write_half":
            k = torch.cat([k[..., :64], kc[b, :, wpos, 64:]], -1)
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
        o = _attend(q[:, :n], kc[b, hmap, :S], vc[b, hmap, :S], vis, scale, emulate,
                    dims=64 if mutant == "score_half_dims" else None)  # [H, n, D]
        if mutant == "out_high_zero":
            o = o.clone()
            o[..., 64:] = 0
        elif mutant == "out_high_neighbour":
            o = torch.cat([o[..., :64], o.roll(-1, 0)[..., : D - 64]], -1)
        out[b, :n] = o.transpose(0, 1).reshape(n, H * D)
    if emulate:
        kc = torch.where(kc.isnan(), kc, rm._rd(kc, bf))
    return out, kc, vc


def per_head(out, n_head, head_dim=64):
    """[B, Tn, H·D] -> [B, H, Tn, D]: ``refmath.tile_rel(..., rows=32)`` then scores one wave's rows of one head."""
    B, Tn, _ = out.shape
    return out.reshape(B, Tn, n_head, head_dim).transpose(1, 2)


def append_inputs(B, H, Hkv, Tn, Tmax, start, seed, poison="loud", gain=2.0, head_dim=64):
    """``refmath_append.append_inputs`` at ``head_dim``: bf16 qkv [B, Tn, (H + 2·Hkv)·D] and caches
    [B, Hkv, Tmax, D], the same draws in the same order; cache rows >= start[b] hold ``poison``
    (``loud`` k = ±30, v = ±1024; ``huge`` ±3e38; ``nan``)."""
    D = head_dim
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


# ------------------------------------------------------------------ the cases of tests/test_gpu_append_hd.py
TMAX = 384
HEADS = ((4, 4), (9, 3), (8, 1))
TNS = (1, 5, 32, 33, 100, 130)
START = (0, 63, 200)  # an empty cache, one short of a 64-key tile edge, the middle of a tile


OWN_NATS = 6.0  # what a new token's own key gains in the score of its group's first query head


def offsets_case(H, Hkv, Tn, use_rope, poison, head_dim=128):
    """(qkv, k_cache, v_cache, start, nnew): nnew = the whole block, a single token (the rest
    padding), a block that crosses a tile edge.  The draw does not depend on ``poison``.

    On top of ``append_inputs``: every new token's k leans towards the query of its group's first
    head, k_i += c · q_i with c = OWN_NATS / (scale · |q_i|²), so that head's score of its own key —
    the diagonal, and with a single-token block the only key a mask mistake can drop — rises by
    OWN_NATS nats (the rotation keeps q_i · k_i).  The scores are ~4 nats wide, so the own key
    then carries weight beside the history's best keys without taking all of it; the other heads
    of a group see one more random direction."""
    D = head_dim
    nnew = (Tn, 1, min(Tn, 37))
    seed = 1000 * H + 10 * Tn + use_rope
    qkv, kc, vc = append_inputs(3, H, Hkv, Tn, TMAX, START, seed, poison=poison, head_dim=D)
    x = qkv.float()
    q0 = x[..., : H * D].reshape(3, Tn, H, D)[:, :, :: H // Hkv]  # [3, Tn, Hkv, D]
    lean = (OWN_NATS / scale_of(D)) * q0 / q0.square().sum(-1, keepdim=True)
    k = x[..., H * D:(H + Hkv) * D] + lean.reshape(3, Tn, Hkv * D)
    qkv = torch.cat([x[..., : H * D], k, x[..., (H + Hkv) * D:]], -1).bfloat16()
    return qkv, kc, vc, START, nnew
