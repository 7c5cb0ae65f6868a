"""Inputs of the shared-prefix decode tests (``decode_attn_shared``, csrc/kernels/decode.hip
``decode_kernel<G, F8, true>``), in the conventions of tests/refmath_decode.py and
tests/refmath_kv8.py.  Never touches ``torch.ops.nbd``; everything is seeded on the CPU.

The op's definition is a change of address only: sequence s of S = B·group reads logical key j
from ``prefix[s // group, :, j]`` for j < plen[s // group] and from ``own[s, :, j - plen]``
otherwise.  So the yardstick is the unshared op on the *materialised* cache ``M[s, :, j]`` — one
private cache of Tp + Ts rows per sequence — and ``materialise`` is that definition, with the wrong
versions of it (``SHARED_MUTANTS``) a wrong kernel could compute.
"""
import torch

import refmath_decode as rd
import refmath_kv8 as r8

D = 64
F8 = r8.F8
SHARED_MUTANTS = ("prefix_row_s", "own_index_j", "boundary_plus1", "boundary_minus1")
# the valid prefix rows the GPU cases draw from: empty, the 32-group edge, the iteration edges of
# both U (64 and 128 keys), the edge of a 224-key chunk from both sides, a full prefix of 320
PLENS = (0, 1, 31, 32, 33, 127, 128, 223, 224, 225, 320)


def raw(t):
    """the bits of a bf16 or e4m3fn tensor (NaN poison compares equal as integers)."""
    return t.contiguous().view(torch.uint8 if t.dtype == F8 else torch.int16)


def per_sequence(plen, group):
    return torch.as_tensor(plen, dtype=torch.int64).repeat_interleave(group)


def materialise(pre, own, plen, group, mutant=None):
    """[S, Hkv, Tp + Ts, 64]: row j of sequence s is ``pre[s // group, :, j]`` below plen and
    ``own[s, :, j - plen]`` from there on (rows past plen + Ts - 1 exist in no cache: zero bits,
    and no position reaches them).
      ``prefix_row_s``     the prefix of prompt s (mod B), not s // group;
      ``own_index_j``      own row j (clamped), not j - plen;
      ``boundary_plus1``   key plen is still taken from the prefix;
      ``boundary_minus1``  key plen - 1 is already taken from the own rows."""
    assert mutant is None or mutant in SHARED_MUTANTS, mutant
    S, Hkv, Ts, _ = own.shape
    B, Tp = pre.shape[0], pre.shape[2]
    pl = per_sequence(plen, group)
    s = torch.arange(S)
    j = torch.arange(Tp + Ts)[None, :]
    edge = pl[:, None] + {"boundary_plus1": 1, "boundary_minus1": -1}.get(mutant, 0)
    in_pre = (j < edge) & (j < Tp)  # [S, T]
    prow = s % B if mutant == "prefix_row_s" else s // group
    oj = j.expand(S, -1) if mutant == "own_index_j" else j - pl[:, None]
    rp, ro = raw(pre), raw(own)
    b = ro[s[:, None], :, oj.clamp(0, Ts - 1)].transpose(1, 2)  # [S, Hkv, T, 64]
    b = torch.where((oj < Ts)[:, None, :, None], b, torch.zeros((), dtype=b.dtype))
    if Tp:
        a = rp[prow][:, :, j[0].clamp(max=Tp - 1)]
        b = torch.where(in_pre[:, None, :, None], a, b)
    return b.contiguous().view(own.dtype)


def shared_case(B, group, H, Hkv, Tp, Ts, plen, pos, seed, poison="nan", fp8=False):
    """One launch: ``B`` prompts of ``plen[b]`` valid prefix rows, ``group`` sequences each at
    absolute positions ``pos[s]`` in [plen, plen + Ts - 1].  Returns (qkv, pre_k, pre_v, own_k,
    own_v) — bf16, or e4m3fn caches — from one ``refmath_decode.decode_history`` draw of S private
    histories whose rows below plen are made the prompt's.  Everything the op must not read holds
    ``poison`` (``refmath_decode.POISON`` kinds, or refmath_kv8's "nan" / "max" on fp8): prefix
    rows >= plen — the whole prefix of a prompt with plen = 0 — and own rows >= pos - plen, the
    row the op is about to write included."""
    S, T = B * group, Tp + Ts
    pl = per_sequence(plen, group)
    pos_t = torch.as_tensor(pos, dtype=torch.int64)
    assert len(plen) == B and len(pos) == S
    assert bool(((pos_t >= pl) & (pos_t < pl + Ts) & (pl <= Tp)).all()), (plen, pos)
    qkv, kc, vc, sign = rd.decode_history(S, H, Hkv, T, seed)
    first = torch.arange(S) // group * group
    common = (torch.arange(T)[None, :] < pl[:, None])[:, None, :, None]
    hist = (qkv, torch.where(common, kc[first], kc), torch.where(common, vc[first], vc), sign)
    fill = r8.kv8_poison if fp8 else rd.decode_poison
    q, km, vm = fill(hist, pos, poison)
    _, k_all, v_all = fill(hist, [0] * S, poison)  # poison everywhere, with the draw's signs
    out = [q]
    for m, p in ((km, k_all), (vm, v_all)):
        m, p = raw(m), raw(p)
        pre, own = p[::group, :, :Tp].clone(), p[:, :, :Ts].clone()
        for b in range(B):
            pre[b, :, :plen[b]] = m[b * group, :, :plen[b]]
        for s in range(S):
            n = min(Ts, T - int(pl[s]))
            own[s, :, :n] = m[s, :, int(pl[s]):int(pl[s]) + n]
        out += [pre.view(km.dtype), own.view(km.dtype)]
    q, pk, ok, pv, ov = out
    return q, pk, pv, ok, ov


def spread_positions(plen, group, Ts, launch=0):
    """``group`` positions per prompt out of [plen, plen + Ts - 1]: the first own row, the last,
    and rows in between that move with ``launch``."""
    pos = []
    for b, pl in enumerate(plen):
        picks = [pl, pl + Ts - 1] + [pl + (37 * (b + 1) + 61 * r + 101 * launch) % Ts for r in range(group)]
        pos += picks[:group]
    return pos
