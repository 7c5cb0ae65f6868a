"""Plain-PyTorch reference of decode attention over an fp8 (``float8_e4m3fn``, no scales) KV cache —
csrc/kernels/decode.hip ``decode_kernel<G, true>`` — in the conventions of tests/refmath_decode.py:
fp64 formulas, an emulation of the kernel's rounding points (``emulate=True``), deliberately wrong
mutants, structured inputs.  Never touches ``torch.ops.nbd``; everything is seeded on the CPU.

Semantics (fixed): a cache row holds ``q8(r)``, r the bf16 row a bf16 cache would hold there —
clamp to ±448, round to nearest even into e4m3fn; NaN stays NaN, ±inf becomes ±448.  The rotated k
is therefore rounded twice (fp32 -> bf16 -> e4m3).  The new token attends to its own key and value
as stored.

Two objects, two rules:
  * the stored row (``stored_rows8``) is a bit pattern: the GPU test compares bytes, so a row
    mutant (``ROW_MUTANTS``) is caught when its bytes differ at all (the floor is 0);
  * the output (``decode8_ref``) takes the caches and the new rows *as stored* and is scored with
    ``refmath.tile_rel`` per head row against ``floor = tile_rel(emulated, exact)``.

Rounding points of the fp8 path beyond the stored bytes: bf16 q; the rotated q stays fp32;
`p.scale2` and `q[g][e] *= p.scale2` in fp32; `v_cvt_pk_f32_fp8` is exact; scores, p and both sums
in fp32; the output rounded to bf16.  No rounding of k or v happens inside ``decode8_ref``: that
floor is the output's bf16 rounding alone (<= 2^-9 of a head row's maximum, plus fp32 noise).
"""
import math

import torch

import refmath as rm
import refmath_decode as rd

D = 64
F8 = torch.float8_e4m3fn
F8_MAX = 448.0
NAN_BYTE, MAX_BYTE = 0x7F, 0x7E  # | 0x80 for the sign
OUT_MUTANTS = ("new_key_unquantised", "fnuz_decode", "half_row", "mask_plus1", "new_key_dropped", "stale_new_key")
ROW_MUTANTS = ("single_rounding", "no_clamp")
KV8_MUTANTS = OUT_MUTANTS + ROW_MUTANTS
KV8_POISON = ("nan", "max")  # what rows >= pos hold: the NaN byte, or ±448 (e4m3fn has no inf)


def q8(x):
    """float tensor -> e4m3fn as the cache stores it: through bf16, clamped to ±448, round to
    nearest even (torch's cast); NaN stays NaN (torch.clamp keeps it)."""
    return x.to(torch.bfloat16).clamp(-F8_MAX, F8_MAX).to(F8)


def dq8(b, fnuz=False):
    """e4m3fn bytes -> fp64, exact.  ``fnuz``: the bytes read as MI300's e4m3fnuz (exponent bias 8,
    not 7): every finite value halves."""
    x = b.to(torch.float32).double()
    return 0.5 * x if fnuz else x


def bits8(b):
    return b.contiguous().view(torch.uint8)


def canon8(b):
    """the bytes with both NaN codes (0x7f, 0xff) as 0x7f: NaN stays NaN is the rule, and torch's
    own CPU casts do not agree on a NaN's sign (a vectorised bf16 conversion sets it)."""
    u = bits8(b)
    return torch.where(u & 0x7F == 0x7F, torch.full_like(u, 0x7F), u)


def stored_rows8(qkv, pos, n_head, n_kv, rope=None, mutant=None):
    """The new token's rows: (k16, v16) the bf16 rows a bf16 cache would hold — k rotated at pos and
    rounded to bf16 — and (k8, v8) = q8 of them, [B, Hkv, 64] each.
      ``single_rounding``  the rotated k goes to e4m3 without the bf16 step;
      ``no_clamp``         the cast without the clamp: beyond ±464 torch's cast gives NaN."""
    assert mutant is None or mutant in ROW_MUTANTS, mutant
    B = qkv.shape[0]
    H, Hkv = n_head, n_kv
    x = qkv.to(torch.bfloat16).double().cpu()
    pos = torch.as_tensor(pos, dtype=torch.int64)
    k = x[:, H * D:(H + Hkv) * D].reshape(B, Hkv, D)
    v = x[:, (H + Hkv) * D:].reshape(B, Hkv, D)
    if rope is not None:
        k = rm.rot(k, rope[0].double().cpu(), rope[1].double().cpu(), pos[:, None])
    k16, v16 = k.to(torch.bfloat16), v.to(torch.bfloat16)
    if mutant == "single_rounding":
        return k16, v16, k.float().clamp(-F8_MAX, F8_MAX).to(F8), q8(v16)
    if mutant == "no_clamp":
        return k16, v16, k16.to(F8), v16.to(F8)
    return k16, v16, q8(k16), q8(v16)


def decode8_ref(q, k8, v8, knew8, vnew8, pos, n_head, scale, rope=None, *, emulate=False, mutant=None, new_bf16=None):
    """``out`` [B, H·64] fp64.  ``q`` [B, H·64] the (unrotated) query part of the projection,
    ``k8`` / ``v8`` the e4m3fn caches [B, Hkv, Tmax, 64] as they stand before the call (rows >= pos
    hold anything), ``knew8`` / ``vnew8`` [B, Hkv, 64] the new token's rows as stored, ``pos`` a
    sequence of ints.  ``new_bf16`` = (k16, v16): the bf16 rows, for ``new_key_unquantised`` only."""
    assert mutant is None or mutant in OUT_MUTANTS, mutant
    bf = torch.bfloat16
    B = q.shape[0]
    Hkv, Tmax = k8.shape[1], k8.shape[2]
    H, G = n_head, n_head // Hkv
    fnuz = mutant == "fnuz_decode"
    x = q.double().cpu()
    if emulate:
        x = rm._rd(x, bf)
    pos = torch.as_tensor(pos, dtype=torch.int64).clamp(0, Tmax - 1)
    bi = torch.arange(B)
    qh = x.reshape(B, H, D)
    if rope is not None:
        qh = rm.rot(qh, rope[0].double().cpu(), rope[1].double().cpu(), pos[:, None])
        if emulate:  # `rope_lane(q[g], ...)` leaves fp32
            qh = rm._f32(qh)
    old_k, old_v = dq8(k8, fnuz), dq8(v8, fnuz)
    if mutant == "new_key_unquantised":  # the bf16 register copy, not the stored bytes
        kn, vn = new_bf16[0].double(), new_bf16[1].double()
    else:
        kn, vn = dq8(knew8, fnuz), dq8(vnew8, fnuz)
    kc, vc = old_k.clone(), old_v.clone()
    kc[bi, :, pos] = kn
    vc[bi, :, pos] = vn
    c2 = scale * rm.LOG2E
    if emulate:  # `p.scale2 = (float)scale * kLog2e`, `q[g][e] *= p.scale2`
        c2 = float(torch.tensor(scale, dtype=torch.float32) * torch.tensor(rm.LOG2E, dtype=torch.float32))
        qh = rm._f32(qh * c2)
    else:
        qh = qh * c2
    # stale_new_key: the memory row at pos as it was before this call, not the register copy
    ak, av = (old_k, old_v) if mutant == "stale_new_key" else (kc, vc)
    j = torch.arange(Tmax)[None, :]
    last = pos[:, None]
    if mutant == "mask_plus1":
        last = (last + 1).clamp(max=Tmax - 1)
    elif mutant == "new_key_dropped":
        last = last - 1
    vis = j <= last  # [B, Tmax]
    # rows the token does not attend hold anything (the NaN byte included): zeros, and masked below
    ak = torch.where(vis[:, None, :, None], ak, torch.zeros((), dtype=torch.float64))
    av = torch.where(vis[:, None, :, None], av, torch.zeros((), dtype=torch.float64))
    if mutant == "half_row":  # a lane group covers 32 of the row's 64 bytes
        ak, av = ak.clone(), av.clone()
        ak[..., 32:] = 0
        av[..., 32:] = 0
    s2 = torch.einsum("bkgd,bktd->bkgt", qh.reshape(B, Hkv, G, D), ak)
    if emulate:
        s2 = rm._f32(s2)
    s2 = s2.masked_fill(~vis[:, None, None, :], -math.inf)
    m = s2.amax(-1, keepdim=True)
    m = torch.where(m == -math.inf, torch.zeros_like(m), m)
    p = torch.exp2(s2 - m)
    if emulate:
        p = rm._f32(p)
    l = p.sum(-1, keepdim=True)
    out = (torch.einsum("bkgt,bktd->bkgd", p, av) / l.clamp_min(1e-300)).reshape(B, H * D)
    if emulate:
        out = rm._rd(out, bf)
    return out


def kv8_poison(hist, pos, poison="max"):
    """(qkv bf16, k8, v8) of a ``refmath_decode.decode_history`` draw: the history quantised with
    ``q8`` (its largest |k| is 16.7, |v| 6.6: nothing saturates), the rows >= pos[b] — the row at
    pos included — holding the NaN byte or ±448 with the draw's signs."""
    qkv, kc, vc, sign = hist
    Tmax = kc.shape[2]
    byte = NAN_BYTE if poison == "nan" else MAX_BYTE
    free = (torch.arange(Tmax)[None, :] >= torch.as_tensor(pos)[:, None])[:, None, :, None]
    out = []
    for c, sg in ((kc, sign[0]), (vc, sign[1])):
        pb = (byte | ((sg < 0).to(torch.uint8) << 7)).to(torch.uint8)
        out.append(torch.where(free, pb, bits8(q8(c))).view(F8))
    return qkv.bfloat16(), out[0], out[1]


def group_case8(G, Tmax, poison, use_rope):
    """the every-group-size case of tests/refmath_decode.py (same draw, same positions) on an fp8
    cache: (H, Hkv, pos, (qkv, k8, v8))."""
    H, pos = G * rd.GROUP_HKV, rd.GROUP_POS[Tmax]
    seed = 1000 * G + Tmax + use_rope
    return H, rd.GROUP_HKV, pos, kv8_poison(rd.decode_history(len(pos), H, rd.GROUP_HKV, Tmax, seed), pos, poison)


def saturating_case(use_rope):
    """the group case G = 3, T = 320 whose incoming k and v also hold ±inf, NaN of both signs and
    finite values beyond ±448 (449 and 464 round to 448 anyway; 480, 1000 and 3e38 need the clamp)."""
    H, Hkv, pos, (qkv, k8, v8) = group_case8(3, 320, "nan", use_rope)
    special = torch.tensor([math.inf, -math.inf, math.nan, -math.nan, 449.0, -464.0, 480.0, -1000.0, 3e38, -3e38])
    qkv = qkv.clone()
    kv = qkv[:, H * D:]
    for b in range(qkv.shape[0]):  # a different dim per sequence and per head, k and v alike
        for h in range(2 * Hkv):
            idx = h * D + (7 * b + 13 * h + 5 * torch.arange(len(special))) % D
            kv[b, idx] = special.bfloat16()
    return H, Hkv, pos, (qkv, k8, v8)


SWEEP_POISON8 = ("max", "nan")  # launch i of a sweep takes kind i % 2


def sweep_history8(kv_len, G):
    return rd.sweep_history(kv_len, G)
