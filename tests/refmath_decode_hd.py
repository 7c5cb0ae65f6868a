"""Head-dim-generic references of decode attention (csrc/kernels/decode.hip ``decode_kernel<D, G, F8,
SHARED>``, D = 64 | 128), in the conventions of tests/refmath_decode.py and tests/refmath_kv8.py, which
fix D = 64: fp64 formulas, an emulation of the kernel's rounding points (``emulate=True``),
deliberately wrong mutants, structured inputs.  Never touches ``torch.ops.nbd``; everything is seeded
on the CPU.  The head dim is the caches' last dim.  At 64 every function here returns what its
fixed-width twin returns, bit for bit (tests/test_decode_hd_ref.py), so there is one reference.

What differs from the 64 draws: lane group 0's keys — every chunk's first key is one — are doubled
at stride 2048 / D (32 groups at 64, 16 at 128), and the softmax scale is D ** -0.5.

The rounding points are those listed in tests/refmath_decode.py and tests/refmath_kv8.py; none
depends on the head dim (the 16-lane sum adds one fp32 addition to a score).

Mutants a 128 kernel can be where a 64 one cannot (``HD_MUTANTS``):
  ``score_half_dims``      q·k summed over 8 of a group's 16 lanes: dims [0, D/2) only;
  ``rope_partner_32``      the RoPE partner taken from lane d8 ^ 4: dim d pairs with d ^ 32, the sign
                           from d mod 64 < 32;
  ``rope_table_stride32``  the tables read as [T, 32]: the angle of (pos, i) taken at flat index 32·pos + i;
  ``out_high_zero``        output dims 64 .. D-1 zero (one wave merges, lane = dim);
  ``out_high_neighbour``   output dims 64 .. D-1 taken from the next head's dims 0 .. 63 (a head
                           stride of 64 in the output row);
  ``part_l_at_64``         the chunks' log-sum-exps stored behind B·H·nchunks·64 floats, inside the
                           chunks' output rows, which they overwrite (needs more than one chunk).
"""
import math

import torch

import refmath as rm
import refmath_decode as rd
import refmath_kv8 as r8

HD_MUTANTS = ("score_half_dims", "rope_partner_32", "rope_table_stride32", "out_high_zero", "out_high_neighbour",
              "part_l_at_64")
DECODE_MUTANTS = rd.DECODE_MUTANTS + HD_MUTANTS
OUT_MUTANTS8 = r8.OUT_MUTANTS
ROW_MUTANTS8 = r8.ROW_MUTANTS
F8 = r8.F8
POISON = rd.POISON


def scale_of(head_dim):
    return head_dim ** -0.5


def rot(x, cos, sin, pos=None, mutant=None):
    """rotate-half RoPE over all D dims of x [..., T, D]: dims d and d + D/2 rotate by the angle of
    (position, d); tables [T', D/2].  ``refmath.rot`` at D = 64."""
    D = x.shape[-1]
    half = D // 2
    c, s = cos.to(x.dtype), sin.to(x.dtype)
    if mutant == "rope_table_stride32":
        p = pos if pos is not None else torch.arange(x.shape[-2])[:, None]
        idx = 32 * p[..., None] + torch.arange(half)  # flat indices of a [T, 32] reading, like c[pos]
        c, s = c.reshape(-1)[idx], s.reshape(-1)[idx]
    elif pos is not None:
        c, s = c[pos], s[pos]
    else:
        c, s = c[: x.shape[-2]], s[: x.shape[-2]]
    if mutant == "rope_partner_32":
        d = torch.arange(D)
        y = x[..., d ^ 32]
        sg = torch.where(d % 64 < 32, -1.0, 1.0).to(x.dtype)
        return x * c[..., d % half] + sg * y * s[..., d % half]
    a, b = x[..., :half], x[..., half:]
    return torch.cat([a * c - b * s, b * c + a * s], -1)


def _chunk_partials(p, av, nch, chunk):
    """per-chunk (l, o) on the common maximum: p [B, kv, G, T], av [B, kv, T, D]."""
    T, D = p.shape[-1], av.shape[-1]
    pad = nch * chunk - T
    pp = torch.nn.functional.pad(p, (0, pad)) if pad > 0 else p[..., : nch * chunk]
    vv = torch.nn.functional.pad(av, (0, 0, 0, pad)) if pad > 0 else av[:, :, : nch * chunk]
    pp = pp.reshape(*p.shape[:3], nch, chunk)
    vv = vv.reshape(vv.shape[0], vv.shape[1], nch, chunk, D)
    lc = pp.sum(-1)  # [B, kv, G, nch]
    oc = torch.einsum("bkgct,bkctd->bkgcd", pp, vv) / lc.clamp_min(1e-300)[..., None]
    return lc, oc


def decode_ref(qkv, k_cache, v_cache, pos, n_head, scale, rope=None, *, emulate=False, mutant=None, chunk=None,
               kv_len_max=None):
    """``refmath_decode.decode_ref`` at the caches' head dim: ``out`` [B, H·D] and the updated
    caches, all fp64.  ``chunk`` / ``kv_len_max``: for the chunk mutants, ``part_l_at_64`` included."""
    assert mutant is None or mutant in DECODE_MUTANTS, mutant
    bf = torch.bfloat16
    B, W = qkv.shape
    Hkv, Tmax, D = k_cache.shape[1], k_cache.shape[2], k_cache.shape[3]
    H, G = n_head, n_head // Hkv
    x = qkv.double().cpu()
    old_k, old_v = k_cache.double().cpu(), v_cache.double().cpu()
    if emulate:
        x = rm._rd(x, bf)
    pos = torch.as_tensor(pos, dtype=torch.int64).clamp(0, Tmax - 1)
    bi = torch.arange(B)
    q = x[:, : H * D].reshape(B, H, D)
    k = x[:, H * D:(H + Hkv) * D].reshape(B, Hkv, D)
    v = x[:, (H + Hkv) * D:].reshape(B, Hkv, D)
    if rope is not None:
        cos, sin = rope[0].double().cpu(), rope[1].double().cpu()
        if mutant == "rope_sign":  # rotate-half with the sign of the sine terms flipped
            sin = -sin
        rpos = ((pos - 1).clamp(min=0) if mutant == "rope_prev_pos" else pos)[:, None]
        rmut = mutant if mutant in ("rope_partner_32", "rope_table_stride32") else None
        q = rot(q, cos, sin, rpos, rmut)
        if mutant != "rope_k_unrotated":
            k = rot(k, cos, sin, rpos, rmut)
        if emulate:  # `rope_lane(q[g], ...)` leaves fp32; `knew = pack8(kf)` is bf16
            q, k = rm._f32(q), rm._rd(k, bf)
    kc, vc = old_k.clone(), old_v.clone()
    kc[bi, :, pos] = k
    vc[bi, :, pos] = v
    c2 = scale * rm.LOG2E
    if emulate:  # `p.scale2 = (float)scale * kLog2e`, `q[g][e] *= p.scale2`
        c2 = float(torch.tensor(scale, dtype=torch.float32) * torch.tensor(rm.LOG2E, dtype=torch.float32))
        q = rm._f32(q * c2)
    else:
        q = q * c2
    # stale_new_key: the memory row at pos as it was before this call, not the register copy
    ak, av = (old_k, old_v) if mutant == "stale_new_key" else (kc, vc)
    j = torch.arange(Tmax)[None, :]
    last = pos[:, None]
    if mutant == "mask_plus1":
        last = (last + 1).clamp(max=Tmax - 1)
    elif mutant == "new_key_dropped":
        last = last - 1
    vis = j <= last  # [B, Tmax]
    if mutant == "chunk_head_dropped":
        vis = vis & ~((j >= chunk) & (j % chunk == 0))
    # rows the token does not attend hold anything (NaN included): zeros, and masked below
    ak = torch.where(vis[:, None, :, None], ak, torch.zeros((), dtype=torch.float64))
    av = torch.where(vis[:, None, :, None], av, torch.zeros((), dtype=torch.float64))
    if mutant == "gqa_mod":  # query head h reads kv head h % Hkv, not h / G
        hmap = torch.arange(H) % Hkv
        ak, av, qg = ak[:, hmap], av[:, hmap], q.reshape(B, H, 1, D)
    else:
        qg = q.reshape(B, Hkv, G, D)
    if mutant == "score_half_dims":
        s2 = torch.einsum("bkgd,bktd->bkgt", qg[..., : D // 2], ak[..., : D // 2])
    else:
        s2 = torch.einsum("bkgd,bktd->bkgt", qg, ak)
    if emulate:  # `acc += q[g][e] * kf[e]`, `sum_group(acc)`: fp32
        s2 = rm._f32(s2)
    s2 = s2.masked_fill(~vis[:, None, None, :], -math.inf)
    m = s2.amax(-1, keepdim=True)
    m = torch.where(m == -math.inf, torch.zeros_like(m), m)
    p = torch.exp2(s2 - m)
    if emulate:  # `pu = exp2f(s[u][g] - ms)`: fp32, never packed to bf16
        p = rm._f32(p)
    if mutant in ("merge_unweighted", "empty_chunk_live", "part_l_at_64"):
        nch = -(-(kv_len_max or Tmax) // chunk)
        lc, oc = _chunk_partials(p, av, nch, chunk)
        live = lc > 0
        if mutant == "merge_unweighted":  # the partials averaged without exp2(l - max)
            o = (oc * live[..., None]).sum(-2) / live.sum(-1, keepdim=True).clamp_min(1)
        elif mutant == "empty_chunk_live":  # a chunk past pos (o = 0) joins the merge with weight 1
            wc = lc / lc.amax(-1, keepdim=True).clamp_min(1e-300)
            empty = (torch.arange(nch)[None, :] * chunk > pos[:, None]).sum(-1).double()[:, None, None, None]
            o = (wc[..., None] * oc).sum(-2) / (wc.sum(-1, keepdim=True) + empty)
        else:
            # part_o [B, H, nch, D] flat, then part_l [B, H, nch] written at float offset B·H·nch·64:
            # the log2-sum-exps (-inf for an empty chunk) land on output partials; the merge reads both
            po = oc.reshape(B, H, nch, D).clone()
            pl = torch.where(live, m + torch.log2(lc.clamp_min(1e-300)), torch.full_like(lc, -math.inf)).reshape(-1)
            flat = po.reshape(-1)
            n64 = B * H * nch * 64
            flat[n64:n64 + pl.numel()] = pl
            po = flat.reshape(B, Hkv, G, nch, D)
            wl = pl.reshape(B, Hkv, G, nch)
            wmax = wl.amax(-1, keepdim=True)
            wc = torch.where(wl == -math.inf, torch.zeros_like(wl), torch.exp2(wl - wmax))
            po = torch.where((wc > 0)[..., None], po, torch.zeros_like(po))  # `if (lk == -INFINITY) continue`
            o = (wc[..., None] * po).sum(-2) / wc.sum(-1, keepdim=True)
    else:
        l = p.sum(-1, keepdim=True)
        o = torch.einsum("bkgt,bktd->bkgd", p, av) / l.clamp_min(1e-300)
    o = o.reshape(B, H, D)
    if mutant == "out_high_zero":
        o = o.clone()
        o[..., 64:] = 0
    elif mutant == "out_high_neighbour":
        o = torch.cat([o[..., :64], o.roll(-1, 1)[..., : D - 64]], -1)
    out = o.reshape(B, H * D)
    if emulate:
        out = rm._rd(out, bf)
    return out, kc, vc


def decode_per_head(out, n_head):
    """[B, H·D] -> [B, H, 1, D]: ``refmath.tile_rel(..., rows=1)`` then scores one head row."""
    return out.reshape(out.shape[0], n_head, 1, -1)


def decode_history(B, H, Hkv, Tmax, seed, gain=2.0, head_dim=64):
    """``refmath_decode.decode_history`` at ``head_dim``; lane group 0's keys (stride 2048 / D) doubled."""
    D = head_dim
    g = torch.Generator(device="cpu").manual_seed(seed)
    q = gain * torch.randn(B, H, D, generator=g)
    kmean, vmean = 0.5 * torch.randn(B, Hkv, 1, D, generator=g), torch.randn(B, Hkv, 1, D, generator=g)
    k = gain * torch.randn(B, Hkv, D, generator=g) + kmean[:, :, 0]
    v = torch.randn(B, Hkv, D, generator=g) + vmean[:, :, 0]
    qkv = torch.cat([q.reshape(B, -1), k.reshape(B, -1), v.reshape(B, -1)], -1)
    kc = gain * torch.randn(B, Hkv, Tmax, D, generator=g) + kmean
    kc[:, :, ::2048 // D] *= 2.0
    vc = torch.randn(B, Hkv, Tmax, D, generator=g) + vmean
    sign = torch.where(torch.rand(2, B, Hkv, Tmax, D, generator=g) < 0.5, -1.0, 1.0)
    return qkv, kc, vc, sign


decode_poison = rd.decode_poison  # (no head dim in it)
kv8_poison = r8.kv8_poison
sweep_positions = rd.sweep_positions
decode_plan = rd.decode_plan  # chunk widths are multiples of 32 groups, hence of the 16 at head dim 128

GROUP_HKV = rd.GROUP_HKV
# head dim 128: the first rows, the 16-group edge, the 32- and 64-key iteration edges, the last row;
# for 640 (three chunks of 224) both chunk edges from both sides.  64: refmath_decode's positions
GROUP_POS = {64: rd.GROUP_POS,
             128: {320: (0, 1, 15, 16, 17, 31, 32, 63, 64, 65, 255, 319),
                   640: (0, 16, 63, 64, 223, 224, 225, 239, 447, 448, 449, 639)}}


def _group_hist(G, Tmax, use_rope, head_dim):
    H, pos = G * GROUP_HKV, GROUP_POS[head_dim][Tmax]
    seed = 1000 * G + Tmax + use_rope
    return H, pos, decode_history(len(pos), H, GROUP_HKV, Tmax, seed, head_dim=head_dim)


def group_case(G, Tmax, poison, use_rope, head_dim=128):
    """(H, Hkv, pos, (qkv, k_cache, v_cache)): ``refmath_decode.group_case`` at ``head_dim``."""
    H, pos, hist = _group_hist(G, Tmax, use_rope, head_dim)
    return H, GROUP_HKV, pos, decode_poison(hist, pos, poison)


def group_case8(G, Tmax, poison, use_rope, head_dim=128):
    """(H, Hkv, pos, (qkv, k8, v8)): ``refmath_kv8.group_case8`` at ``head_dim``."""
    H, pos, hist = _group_hist(G, Tmax, use_rope, head_dim)
    return H, GROUP_HKV, pos, kv8_poison(hist, pos, poison)


def saturating_case(use_rope, head_dim=128):
    """``refmath_kv8.saturating_case`` redrawn at ``head_dim``."""
    D = head_dim
    H, Hkv, pos, (qkv, k8, v8) = group_case8(3, 320, "nan", use_rope, D)
    special = torch.tensor([math.inf, -math.inf, math.nan, -math.nan, 449.0, -464.0, 480.0, -1000.0, 3e38, -3e38])
    qkv = qkv.clone()
    kv = qkv[:, H * D:]
    for b in range(qkv.shape[0]):  # a different dim per sequence and per head, k and v alike
        for h in range(2 * Hkv):
            idx = h * D + (7 * b + 13 * h + 5 * torch.arange(len(special))) % D
            kv[b, idx] = special.bfloat16()
    return H, Hkv, pos, (qkv, k8, v8)


SWEEP_B = rd.SWEEP_B
SWEEP_POISON = rd.SWEEP_POISON


def sweep_history(kv_len, G, head_dim=128):
    return decode_history(SWEEP_B, G, 1, kv_len, seed=50000 + 10 * kv_len + G, head_dim=head_dim)


# --------------------------------------------------------------------------------------- fp8
def stored_rows8(qkv, pos, n_head, n_kv, head_dim, rope=None, mutant=None):
    """``refmath_kv8.stored_rows8`` at ``head_dim``: (k16, v16, k8, v8), [B, Hkv, D] each."""
    assert mutant is None or mutant in ROW_MUTANTS8, mutant
    D = head_dim
    B = qkv.shape[0]
    H, Hkv = n_head, n_kv
    x = qkv.to(torch.bfloat16).double().cpu()
    pos = torch.as_tensor(pos, dtype=torch.int64)
    k = x[:, H * D:(H + Hkv) * D].reshape(B, Hkv, D)
    v = x[:, (H + Hkv) * D:].reshape(B, Hkv, D)
    if rope is not None:
        k = rot(k, rope[0].double().cpu(), rope[1].double().cpu(), pos[:, None])
    k16, v16 = k.to(torch.bfloat16), v.to(torch.bfloat16)
    if mutant == "single_rounding":
        return k16, v16, k.float().clamp(-r8.F8_MAX, r8.F8_MAX).to(F8), r8.q8(v16)
    if mutant == "no_clamp":
        return k16, v16, k16.to(F8), v16.to(F8)
    return k16, v16, r8.q8(k16), r8.q8(v16)


def decode8_ref(q, k8, v8, knew8, vnew8, pos, n_head, scale, rope=None, *, emulate=False, mutant=None, new_bf16=None):
    """``refmath_kv8.decode8_ref`` at the caches' head dim; ``mutant``: its output mutants, and of
    ``HD_MUTANTS`` those of the output (``score_half_dims``, ``out_high_zero``, ``out_high_neighbour``)."""
    assert mutant is None or mutant in OUT_MUTANTS8 + HD_MUTANTS, mutant
    bf = torch.bfloat16
    B = q.shape[0]
    Hkv, Tmax, D = k8.shape[1], k8.shape[2], k8.shape[3]
    H, G = n_head, n_head // Hkv
    fnuz = mutant == "fnuz_decode"
    x = q.double().cpu()
    if emulate:
        x = rm._rd(x, bf)
    pos = torch.as_tensor(pos, dtype=torch.int64).clamp(0, Tmax - 1)
    bi = torch.arange(B)
    qh = x.reshape(B, H, D)
    if rope is not None:
        qh = rot(qh, rope[0].double().cpu(), rope[1].double().cpu(), pos[:, None])
        if emulate:  # `rope_lane(q[g], ...)` leaves fp32
            qh = rm._f32(qh)
    old_k, old_v = r8.dq8(k8, fnuz), r8.dq8(v8, fnuz)
    if mutant == "new_key_unquantised":  # the bf16 register copy, not the stored bytes
        kn, vn = new_bf16[0].double(), new_bf16[1].double()
    else:
        kn, vn = r8.dq8(knew8, fnuz), r8.dq8(vnew8, fnuz)
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
    if mutant == "half_row":  # a lane group covers half of the row's bytes
        ak, av = ak.clone(), av.clone()
        ak[..., D // 2:] = 0
        av[..., D // 2:] = 0
    qg = qh.reshape(B, Hkv, G, D)
    if mutant == "score_half_dims":
        s2 = torch.einsum("bkgd,bktd->bkgt", qg[..., : D // 2], ak[..., : D // 2])
    else:
        s2 = torch.einsum("bkgd,bktd->bkgt", qg, ak)
    if emulate:
        s2 = rm._f32(s2)
    s2 = s2.masked_fill(~vis[:, None, None, :], -math.inf)
    m = s2.amax(-1, keepdim=True)
    m = torch.where(m == -math.inf, torch.zeros_like(m), m)
    p = torch.exp2(s2 - m)
    if emulate:
        p = rm._f32(p)
    l = p.sum(-1, keepdim=True)
    o = (torch.einsum("bkgt,bktd->bkgd", p, av) / l.clamp_min(1e-300)).reshape(B, H, D)
    if mutant == "out_high_zero":
        o = o.clone()
        o[..., 64:] = 0
    elif mutant == "out_high_neighbour":
        o = torch.cat([o[..., :64], o.roll(-1, 1)[..., : D - 64]], -1)
    out = o.reshape(B, H * D)
    if emulate:
        out = rm._rd(out, bf)
    return out
