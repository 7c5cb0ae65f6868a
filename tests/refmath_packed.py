"""Plain-PyTorch reference for document-masked ("packed") attention: query i of row b sees key j
iff ``kstart[b, i] <= j <= i``.

THIS IS A DELIBERATE COPY of the arithmetic of ``tests/refmath.py::_attn_chunk`` (about 100 lines)
with ``masked = (j > i) | (j < kstart[i])``: ``refmath.py`` is a yardstick that is not edited and it
has no mask hook.  ``tests/test_packed_ref.py`` ties the copy to it: with ``kstart = 0`` the two
agree bit for bit, exact and emulated, plain and RoPE.  Keep the two in step.

What differs from the original, besides the mask:
  * the emulated running maximum starts at the kernel's finite floor (attn.hip ``kSegFloor``)
    instead of -inf: a lane that has seen no key keeps the floor, its probabilities are
    exp2(-inf) = 0, and at its first key the rescale factor exp2(floor - m) is exactly 0 — the same
    bits as -inf gives, which is why the kstart = 0 comparison is exact;
  * mutants of the mask (PACKED_MUTANTS) instead of the formulas'.
"""
import math

import torch

from refmath import LN2, LOG2E, _f32, _rd, rot, rot_inv

SEG_FLOOR = float(torch.tensor(-3.0e38, dtype=torch.float32))  # attn.hip kSegFloor

PACKED_MUTANTS = ("kstart_plus1", "kstart_minus1", "qend_minus1", "bounds_ignored_offdiag")

# (T, document lengths per row): the layouts of tests/test_gpu_attn_packed.py, shared with the CPU
# proof (tests/test_packed_ref.py) that the mutants show on them
LAYOUTS = {
    "one-doc": (256, [[256]]),                             # trivial bounds, fused δ
    "128+128": (256, [[128, 128]]),                        # whole-workgroup tile skip
    "80+176": (256, [[80, 176]]),                          # boundary inside a wave; nothing visible in tile 0
    "96+160": (256, [[96, 160]]),                          # boundary on a 32- but not 64-key edge
    "six-docs": (384, [[33, 31, 64, 1, 127, 128]]),        # δ pre-pass, odd block count, a length-1 document
    "1+1+1+381": (384, [[1, 1, 1, 381]]),                  # queries whose only key is themselves
    "two-rows": (256, [[80, 176], [200, 56]]),             # per-row bounds
    "100+924": (1024, [[100, 924]]),                       # long tail tiles under a bound
}


def bounds_of_lengths(rows, T):
    """kstart, qend (int64 [B, T]) and position_ids for rows given as lists of document lengths."""
    ks = torch.zeros(len(rows), T, dtype=torch.int64)
    qe = torch.zeros(len(rows), T, dtype=torch.int64)
    pos = torch.zeros(len(rows), T, dtype=torch.int64)
    for b, lens in enumerate(rows):
        assert sum(lens) == T and min(lens) >= 1, (lens, T)
        s = 0
        for n in lens:
            ks[b, s:s + n] = s
            qe[b, s:s + n] = s + n
            pos[b, s:s + n] = torch.arange(n)
            s += n
    return ks, qe, pos


def visibility(kstart, mutant=None):
    """(masked [B, 1, T, T]: True where query i does not see key j; keep_q [B, T]: the query rows
    that contribute to dK/dV) for ``kstart`` [B, T] — the whole of what a mutant changes."""
    B, T = kstart.shape
    dev = kstart.device
    i = torch.arange(T, device=dev)[:, None]
    j = torch.arange(T, device=dev)[None, :]
    ks = kstart.long()[:, None, :, None]  # [B, 1, T(query), 1]
    if mutant == "kstart_plus1":  # a query's own first key hidden (it still sees itself)
        ks = torch.minimum(ks + 1, i[None, None])
    elif mutant == "kstart_minus1":  # the previous document's last key visible
        ks = (ks - 1).clamp_min(0)
    low = j[None, None] < ks
    if mutant == "bounds_ignored_offdiag":  # the lower bound applied only in the query's own 64-key tile
        low = low & ((j // 64) == (i // 64))[None, None]
    masked = (j > i)[None, None] | low
    keep_q = torch.ones(B, T, dtype=torch.bool, device=dev)
    if mutant == "qend_minus1":  # dK/dV only: the last query of every document dropped
        keep_q[:, -1] = False
        keep_q[:, :-1] = kstart[:, 1:] == kstart[:, :-1]
    return masked, keep_q


def _chunk(q, k, v, do, scale, kstart, rope, emulate, mutant, gsplit):
    bf = torch.bfloat16
    B, H, T, D = q.shape
    Hkv = k.shape[1]
    group = H // Hkv
    dev = q.device
    q, k, v = q.double(), k.double(), v.double()
    if emulate:
        q, k, v = _rd(q, bf), _rd(k, bf), _rd(v, bf)
    if rope is not None:
        cos, sin = rope[0].double(), rope[1].double()
        q, k = rot(q, cos, sin), rot(k, cos, sin)
        if emulate:  # attn.hip rope8: the rotated q / k go back to bf16 for the MFMAs
            q, k = _rd(q, bf), _rd(k, bf)
    hmap = torch.arange(H, device=dev) // group
    kx, vx = k[:, hmap], v[:, hmap]
    masked, keep_q = visibility(kstart.to(dev), mutant)
    c2 = scale * LOG2E
    if emulate:
        # attn.hip fwd_kernel `sacc[kb] = mfma(..., qf[s], sacc[kb])`: fp32 accumulation over four
        # 16-dim MFMA steps, scaled by the fp32 constant sc2 = (float)scale * kLog2e
        sraw = torch.zeros(B, H, T, T, dtype=torch.float64, device=dev)
        for d0 in range(0, D, 16):
            sraw = _f32(sraw + q[..., d0:d0 + 16] @ kx[..., d0:d0 + 16].transpose(-1, -2))
        c2 = float(torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32))
    else:
        sraw = q @ kx.transpose(-1, -2)
    s2 = (sraw * c2).masked_fill(masked, -math.inf)  # log2 units
    m = s2.amax(-1, keepdim=True)
    if emulate:
        # fwd_kernel's deferred rescale, as refmath._attn_chunk models it; the running maximum
        # starts at the finite floor (fwd_kernel `float m = SEG ? kSegFloor : -INFINITY`)
        run = torch.full_like(m, SEG_FLOOR)
        mt = torch.empty_like(s2)
        l = torch.zeros_like(m)
        for t0 in range(0, T, 64):
            mn = torch.maximum(run, _f32(s2[..., t0:t0 + 64].amax(-1, keepdim=True)))
            grow = (mn > run + 4.0).reshape(B, H, T // 32, 32).any(-1, keepdim=True)
            new = torch.where(grow.expand(B, H, T // 32, 32).reshape(B, H, T, 1), mn, run)
            alpha = torch.where(new > run, torch.exp2(run - new), torch.ones_like(run))
            run = new
            mt[..., t0:t0 + 64] = run
            pt = torch.exp2(_f32(sraw[..., t0:t0 + 64] * c2 - run).masked_fill(masked[..., t0:t0 + 64], -math.inf))
            l = _f32(_f32(l * alpha) + pt.float().sum(-1, keepdim=True).double())
        m = run
        p = torch.exp2(_f32(sraw * c2 - mt).masked_fill(masked, -math.inf))
        wt = torch.exp2(mt - m)
        out = ((_rd(p, bf) * wt) @ vx) / l
        out = _rd(out, bf)
        lg = _f32(m + _f32(torch.log2(l)))
        lse = _f32(lg * float(torch.tensor(LN2, dtype=torch.float32))).squeeze(-1)
    else:
        p = torch.exp2(s2 - m)
        l = p.sum(-1, keepdim=True)
        out = (p @ vx) / l
        lse = ((m + torch.log2(l)) * LN2).squeeze(-1)
    if do is None:
        return out, lse
    do = do.double()
    if emulate:
        do = _rd(do, bf)
    delta = (do * out).sum(-1, keepdim=True)  # from the stored (rounded) output
    l2 = lse.unsqueeze(-1) * LOG2E
    if emulate:
        l2 = _f32(l2)
        pn = torch.exp2(_f32(sraw * c2 - l2).masked_fill(masked, -math.inf))
    else:
        pn = torch.exp2(s2 - l2)
    dp = do @ vx.transpose(-1, -2)
    ds = pn * (dp - delta)
    if emulate:  # P and dS packed to bf16 for the dV / dK / dQ products (attn.hip header)
        pn, ds = _rd(pn, bf), _rd(ds, bf)
    dq = scale * (ds @ kx)
    keep = keep_q[:, None, :, None].to(pn.dtype)  # (all ones but for the qend_minus1 mutant)
    pk, dsk = pn * keep, ds * keep
    dv_h = pk.transpose(-1, -2) @ do
    dk_h = scale * (dsk.transpose(-1, -2) @ q)
    if rope is not None:
        dq = rot_inv(dq, cos, sin)
        dk_h = rot_inv(dk_h, cos, sin)
    if emulate and gsplit and group > 1:
        # attn_bwd_hip: with the group split over workgroups each query head's dK / dV partial is
        # stored as bf16 before the fp32 sum
        dk_h, dv_h = _rd(dk_h, bf), _rd(dv_h, bf)
    dk = torch.zeros(B, Hkv, T, D, dtype=torch.float64, device=dev).index_add_(1, hmap, dk_h)
    dv = torch.zeros(B, Hkv, T, D, dtype=torch.float64, device=dev).index_add_(1, hmap, dv_h)
    if emulate:
        dq, dk, dv = _rd(dq, bf), _rd(dk, bf), _rd(dv, bf)
    return out, lse, dq, dk, dv


def attn_ref_packed(q, k, v, do, scale, kstart, rope=None, emulate=False, mutant=None, gsplit=False, chunk=None):
    """Document-masked causal attention and its FA2 backward for q, do [B, H, T, 64], k, v
    [B, Hkv, T, 64] and ``kstart`` [B, T] (start of each query's document).  Returns out, lse (and
    dq, dk, dv unless ``do`` is None) in fp64; arguments as ``refmath.attn_ref``."""
    assert mutant is None or mutant in PACKED_MUTANTS, mutant
    B = q.shape[0]
    assert tuple(kstart.shape) == (B, q.shape[2]), kstart.shape
    chunk = chunk or B
    parts = []
    for b0 in range(0, B, chunk):
        sl = slice(b0, min(B, b0 + chunk))
        parts.append(_chunk(q[sl], k[sl], v[sl], None if do is None else do[sl], scale, kstart[sl], rope, emulate,
                            mutant, gsplit))
    return tuple(torch.cat([p[n] for p in parts], 0) for n in range(len(parts[0])))
