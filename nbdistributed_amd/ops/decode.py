"""Decode attention over a KV cache (K13): one new token per sequence, cache append fused.

``csrc/kernels/decode.hip`` on GPU (bf16, head dim 64 or 128, up to 8 query heads per key/value head);
the same math in PyTorch otherwise (CPU, fp32) — also the numerics reference of the GPU tests.
The caches are bf16 or, with no scales, ``float8_e4m3fn`` (:func:`q8`: half the bytes a decode
step streams); qkv and the output stay bf16.
Shared prefix (``decode_attention_shared``): ``group`` consecutive sequences read one prompt's prefix
rows and then their own — several samples per prompt with the prompt held once.
Block append (K17, ``csrc/kernels/append.hip``): several new tokens per sequence at per-sequence
offsets — what continuing from a returned cache runs instead of a second prefill (bf16 cache,
head dim 64 or 128).
"""
from __future__ import annotations

from typing import Optional

from ._lib import _require


DECODE_HEAD_DIMS = (64, 128)  # the head dims decode.hip is instantiated for


def partials_numel(batch: int, n_head: int, t_max: int, head_dim: int = 64) -> int:
    """fp32 workspace the kernel needs for its chunk partials (worst case over key bounds ≤ ``t_max``):
    ``head_dim`` + 1 floats — the chunk's output row and its log-sum-exp — per (sequence, head, chunk)."""
    nchunks = min(64, max(1, -(-t_max // 128)))
    return batch * n_head * nchunks * (head_dim + 1)


FP8_MAX = 448.0  # the largest finite float8_e4m3fn (OCP e4m3: no inf)


def q8(x):
    """What an fp8 KV cache holds for a row ``x``: the bf16 row a bf16 cache would hold, clamped to
    ±448 (so ±inf saturates; NaN stays NaN), rounded to nearest even into ``float8_e4m3fn``.  No
    scales.  Every e4m3 value is exact in bf16 and fp32, so reading one back rounds nothing."""
    import torch

    return x.to(torch.bfloat16).clamp(-FP8_MAX, FP8_MAX).to(torch.float8_e4m3fn)


def _to_cache(x, dtype):
    import torch

    return q8(x) if dtype == torch.float8_e4m3fn else x.to(dtype)


def decode_supported(qkv, k_cache, n_head: int) -> bool:
    import torch

    Hkv = k_cache.shape[1]
    return (qkv.is_cuda and qkv.dtype == torch.bfloat16 and k_cache.dtype in (torch.bfloat16, torch.float8_e4m3fn)
            and k_cache.shape[-1] in DECODE_HEAD_DIMS and n_head % Hkv == 0 and n_head // Hkv <= 8)


def _rope_at(x, cos, sin, pos):
    """HF rotate_half RoPE of x [B, h, D] at per-row positions pos [B] (fp32 math)."""
    import torch

    half = x.shape[-1] // 2
    c, s = cos[pos][:, None, :], sin[pos][:, None, :]
    a, b = x[..., :half].float(), x[..., half:].float()
    return torch.cat([a * c - b * s, b * c + a * s], -1)


def decode_attention_reference(qkv, k_cache, v_cache, pos, n_head: int, scale: Optional[float] = None, rope=None):
    """PyTorch version of :func:`decode_attention` (writes the caches the same way).  On fp8 caches
    the new rows are stored as :func:`q8` makes them and the token attends over the caches as
    stored, its own row included — as the kernel does."""
    import torch

    B, W = qkv.shape
    Hkv, Tmax, D = k_cache.shape[1], k_cache.shape[2], k_cache.shape[3]
    H, G = n_head, n_head // Hkv
    sc = float(scale) if scale is not None else D ** -0.5
    pos = pos.long().clamp(0, Tmax - 1)
    q = qkv[:, : H * D].view(B, H, D)
    k = qkv[:, H * D:(H + Hkv) * D].view(B, Hkv, D)
    v = qkv[:, (H + Hkv) * D:].view(B, Hkv, D)
    if rope is not None:
        q = _rope_at(q, rope[0], rope[1], pos)
        k = _rope_at(k, rope[0], rope[1], pos)
    bi = torch.arange(B, device=qkv.device)
    k_cache[bi, :, pos] = _to_cache(k, k_cache.dtype)
    v_cache[bi, :, pos] = _to_cache(v, v_cache.dtype)
    mask = torch.arange(Tmax, device=qkv.device)[None, :] > pos[:, None]  # [B, Tmax]
    # rows > pos hold nothing of this sequence (possibly NaN): zeros, and masked below
    held = ~mask[:, None, :, None]
    kc = torch.where(held, k_cache.float(), torch.zeros((), device=qkv.device))
    vc = torch.where(held, v_cache.float(), torch.zeros((), device=qkv.device))
    s = torch.einsum("bkgd,bktd->bkgt", q.float().view(B, Hkv, G, D), kc) * sc
    s = s.masked_fill(mask[:, None, None, :], float("-inf"))
    p = torch.softmax(s, -1)
    o = torch.einsum("bkgt,bktd->bkgd", p, vc)
    return o.reshape(B, H * D).to(qkv.dtype)


def decode_attention(qkv, k_cache, v_cache, pos, n_head: int, scale: Optional[float] = None, rope=None,
                     kv_len_max: Optional[int] = None, workspace=None):
    """Attention of one new token per sequence over its KV cache.

    ``qkv`` [B, (H + 2·Hkv)·D] is the new tokens' packed projection, ``k_cache``/``v_cache``
    [B, Hkv, Tmax, D] the caches (rows ≥ ``pos[b]`` are free; bf16, or ``float8_e4m3fn`` holding
    :func:`q8` rows: the new rows are then stored quantised and attended as stored), ``pos`` int64 [B] the new tokens'
    positions (on the device: a decode step graph-captures).  The new k (rotated when ``rope`` =
    (cos, sin) tables) and v are written into the caches at ``pos[b]`` and the token attends to
    rows 0..pos[b].  ``kv_len_max`` bounds max(pos) + 1 (default Tmax; smaller = fewer idle
    workgroups); ``workspace`` = fp32 chunk partials [≥ :func:`partials_numel`] (held by
    ``generation.KVCache``; allocated per call if None).  Returns [B, H·D].  The HIP kernel takes
    D = 64 and 128; any other head dim runs :func:`decode_attention_reference`."""
    import torch

    D = k_cache.shape[-1]
    sc = float(scale) if scale is not None else D ** -0.5
    if decode_supported(qkv, k_cache, n_head):
        _require()
        B, Tmax = k_cache.shape[0], k_cache.shape[2]
        if workspace is None:
            workspace = torch.empty(partials_numel(B, n_head, Tmax, D), dtype=torch.float32, device=qkv.device)
        cos, sin = rope if rope is not None else (None, None)
        if qkv.stride(-1) != 1 or qkv.stride(0) % 8 or qkv.data_ptr() % 16:
            qkv = qkv.contiguous()
        return torch.ops.nbd.decode_attn(qkv, k_cache, v_cache, pos, int(n_head), sc, int(kv_len_max or Tmax),
                                         cos, sin, workspace)
    return decode_attention_reference(qkv, k_cache, v_cache, pos, n_head, sc, rope)


# ------------------------------------------------------------------ shared prefix (several samples per prompt)
def decode_shared_supported(qkv, k_prefix, k_own, n_head: int) -> bool:
    import torch

    Hkv = k_own.shape[1]
    return (qkv.is_cuda and qkv.dtype == torch.bfloat16 and k_own.dtype in (torch.bfloat16, torch.float8_e4m3fn)
            and k_prefix.dtype == k_own.dtype and k_own.shape[-1] in DECODE_HEAD_DIMS
            and k_prefix.shape[-1] == k_own.shape[-1]
            and n_head % Hkv == 0 and n_head // Hkv <= 8)


def _shared_span(plen, pos, group: int, Tp: int, Ts: int):
    """``plen`` [B] and ``pos`` [B·group] clamped as the kernel clamps them before addressing:
    0 ≤ plen ≤ Tp, then plen ≤ pos ≤ plen + Ts - 1 (the new row never lands in the prefix).
    Returns (plen per sequence [B·group], pos)."""
    import torch

    pl = plen.long().clamp(0, Tp).repeat_interleave(group)
    pos = torch.minimum(torch.maximum(pos.long(), pl), pl + (Ts - 1))
    return pl, pos


def decode_attention_shared_reference(qkv, k_prefix, v_prefix, plen, k_own, v_own, pos, group: int, n_head: int,
                                      scale: Optional[float] = None, rope=None):
    """PyTorch version of :func:`decode_attention_shared` (writes the own caches the same way, never
    the prefix).  On fp8 caches the new rows are stored as :func:`q8` makes them and the token
    attends over the caches as stored, its own row included — as the kernel does."""
    import torch

    S, W = qkv.shape
    Hkv, Ts, D = k_own.shape[1], k_own.shape[2], k_own.shape[3]
    Tp = k_prefix.shape[2]
    H, G = n_head, n_head // Hkv
    dev = qkv.device
    sc = float(scale) if scale is not None else D ** -0.5
    pl, pos = _shared_span(plen, pos, group, Tp, Ts)
    q = qkv[:, : H * D].view(S, H, D)
    k = qkv[:, H * D:(H + Hkv) * D].view(S, Hkv, D)
    v = qkv[:, (H + Hkv) * D:].view(S, Hkv, D)
    if rope is not None:
        q = _rope_at(q, rope[0], rope[1], pos)
        k = _rope_at(k, rope[0], rope[1], pos)
    si = torch.arange(S, device=dev)
    k_own[si, :, pos - pl] = _to_cache(k, k_own.dtype)
    v_own[si, :, pos - pl] = _to_cache(v, v_own.dtype)
    # logical key j of sequence s: prefix[s // group, :, j] below plen, own[s, :, j - plen] from there on
    j = torch.arange(Tp + Ts, device=dev)[None, :]  # [1, Tp + Ts]
    in_pre = j < pl[:, None]  # [S, T]
    mask = j > pos[:, None]
    held = (~mask)[:, None, :, None]
    zero = torch.zeros((), device=dev)

    def logical(pre, own):
        # rows > pos hold nothing of this sequence (possibly NaN): zeros, and masked below
        a = pre.float()[si // group][:, :, j[0].clamp(max=max(Tp - 1, 0))] if Tp else None
        b = own.float()[si[:, None], :, (j - pl[:, None]).clamp(0, Ts - 1)].transpose(1, 2)  # [S, Hkv, T, D]
        m = b if a is None else torch.where(in_pre[:, None, :, None], a, b)
        return torch.where(held, m, zero)

    kc, vc = logical(k_prefix, k_own), logical(v_prefix, v_own)
    s = torch.einsum("bkgd,bktd->bkgt", q.float().view(S, Hkv, G, D), kc) * sc
    s = s.masked_fill(mask[:, None, None, :], float("-inf"))
    p = torch.softmax(s, -1)
    o = torch.einsum("bkgt,bktd->bkgd", p, vc)
    return o.reshape(S, H * D).to(qkv.dtype)


def decode_attention_shared(qkv, k_prefix, v_prefix, plen, k_own, v_own, pos, group: int, n_head: int,
                            scale: Optional[float] = None, rope=None, kv_len_max: Optional[int] = None,
                            workspace=None):
    """Attention of one new token per sequence where ``group`` consecutive sequences share a prompt.

    ``qkv`` [S = B·group, (H + 2·Hkv)·D]; sequence s belongs to prompt s // group.  Its logical key
    j is ``k_prefix[s // group, :, j]`` ([B, Hkv, Tp, D], read only) for j < ``plen[s // group]``
    (int64 [B] on the device) and ``k_own[s, :, j - plen]`` ([S, Hkv, Ts, D]) from there on.
    ``pos`` int64 [S] are absolute positions: the new k (rotated at ``pos``) and v are written to
    own row ``pos - plen`` and the token attends logical keys 0..pos.  ``plen`` is clamped to
    [0, Tp] and ``pos`` to [plen, plen + Ts - 1] first.  ``kv_len_max`` bounds max(pos) + 1 (default
    Tp + Ts); ``workspace`` as in :func:`decode_attention`, sized for S sequences and Tp + Ts keys.
    bf16 or ``float8_e4m3fn`` caches (prefix and own alike), D = 64 or 128 on the HIP kernel (prefix and
    own alike).  Returns [S, H·D]."""
    import torch

    D = k_own.shape[-1]
    sc = float(scale) if scale is not None else D ** -0.5
    if k_prefix.dtype != k_own.dtype or v_prefix.dtype != k_own.dtype or v_own.dtype != k_own.dtype:
        raise ValueError(f"decode_attention_shared: prefix ({k_prefix.dtype}) and own ({k_own.dtype}) caches "
                         f"must have the same dtype")
    if decode_shared_supported(qkv, k_prefix, k_own, n_head):
        _require()
        S, T = k_own.shape[0], k_prefix.shape[2] + k_own.shape[2]
        if workspace is None:
            workspace = torch.empty(partials_numel(S, n_head, T, D), dtype=torch.float32, device=qkv.device)
        cos, sin = rope if rope is not None else (None, None)
        if qkv.stride(-1) != 1 or qkv.stride(0) % 8 or qkv.data_ptr() % 16:
            qkv = qkv.contiguous()
        return torch.ops.nbd.decode_attn_shared(qkv, k_prefix, v_prefix, plen, k_own, v_own, pos, int(group),
                                                int(n_head), sc, int(kv_len_max or T), cos, sin, workspace)
    return decode_attention_shared_reference(qkv, k_prefix, v_prefix, plen, k_own, v_own, pos, group, n_head, sc, rope)


# ------------------------------------------------------------------ block append (K17)
APPEND_HEAD_DIMS = (64, 128)  # the head dims append.hip is instantiated for


def append_supported(qkv, k_cache, n_head: int) -> bool:
    import torch

    Hkv = k_cache.shape[1]
    return (qkv.is_cuda and qkv.dtype == torch.bfloat16 and k_cache.dtype == torch.bfloat16
            and k_cache.shape[-1] in APPEND_HEAD_DIMS and n_head % Hkv == 0)


def _append_span(start, nnew, Tn: int, limit: int):
    """``start`` / ``nnew`` clamped as the kernel clamps them before addressing: 0 ≤ start ≤ limit-1,
    0 ≤ nnew ≤ min(Tn, limit - start)."""
    import torch

    start = start.long().clamp(0, limit - 1)
    return start, torch.minimum(nnew.long().clamp(0, Tn), limit - start)


def append_attention_reference(qkv, k_cache, v_cache, start, nnew, n_head: int, scale: Optional[float] = None,
                               rope=None, kv_len_max: Optional[int] = None):
    """PyTorch version of :func:`append_attention` (fp32 math, writes the caches the same way)."""
    import torch

    B, Tn, W = qkv.shape
    Hkv, Tmax, D = k_cache.shape[1], k_cache.shape[2], k_cache.shape[3]
    H, G = n_head, n_head // Hkv
    dev = qkv.device
    sc = float(scale) if scale is not None else D ** -0.5
    start, nnew = _append_span(start, nnew, Tn, min(Tmax, int(kv_len_max or Tmax)))
    i = torch.arange(Tn, device=dev)
    valid = i[None, :] < nnew[:, None]  # [B, Tn]
    pos = (start[:, None] + i[None, :]).clamp(max=Tmax - 1)  # (clamped only on padding rows)
    q = qkv[..., : H * D].reshape(B, Tn, H, D).float()
    k = qkv[..., H * D:(H + Hkv) * D].reshape(B, Tn, Hkv, D).float()
    v = qkv[..., (H + Hkv) * D:].reshape(B, Tn, Hkv, D)
    if rope is not None:
        half = D // 2
        c, s = rope[0][pos][:, :, None, :].float(), rope[1][pos][:, :, None, :].float()

        def rot(x):
            a, b = x[..., :half], x[..., half:]
            return torch.cat([a * c - b * s, b * c + a * s], -1)

        q, k = rot(q), rot(k)
    bi, ti = valid.nonzero(as_tuple=True)
    k_cache[bi, :, pos[bi, ti]] = k[bi, ti].to(k_cache.dtype)
    v_cache[bi, :, pos[bi, ti]] = v[bi, ti].to(v_cache.dtype)
    # rows >= start + nnew hold nothing of this sequence (possibly NaN): zeros, and masked below
    t = torch.arange(Tmax, device=dev)
    held = (t[None, :] < (start + nnew)[:, None])[:, None, :, None]  # [B, 1, Tmax, 1]
    kc = torch.where(held, k_cache.float(), torch.zeros((), device=dev))
    vc = torch.where(held, v_cache.float(), torch.zeros((), device=dev))
    s = torch.einsum("btkgd,bksd->bkgts", q.reshape(B, Tn, Hkv, G, D), kc) * sc  # [B, Hkv, G, Tn, Tmax]
    mask = t[None, None, :] > pos[:, :, None]  # [B, Tn, Tmax]
    p = torch.softmax(s.masked_fill(mask[:, None, None], float("-inf")), -1)
    o = torch.einsum("bkgts,bksd->btkgd", p, vc).reshape(B, Tn, H * D)
    return o.masked_fill(~valid[:, :, None], 0.0).to(qkv.dtype)


def append_attention(qkv, k_cache, v_cache, start, nnew, n_head: int, scale: Optional[float] = None, rope=None,
                     kv_len_max: Optional[int] = None):
    """Attention of a block of new tokens per sequence over its KV cache (multi-turn append).

    ``qkv`` [B, Tn, (H + 2·Hkv)·D] is the new tokens' packed projection (any ``Tn`` ≥ 1: the kernel
    wants no padding of it), ``k_cache``/``v_cache`` [B, Hkv, Tmax, D] the caches, ``start`` int64
    [B] (on the device) the rows already valid in each, ``nnew`` int64 [B] the real rows of ``qkv``
    (1 ≤ nnew[b] ≤ Tn; rows past it are padding).  For i < nnew[b] the new k (rotated at position
    start[b] + i when ``rope`` = (cos, sin) tables) and v are written to cache row start[b] + i and
    query i attends rows 0..start[b] + i; no later row influences it, whatever it holds, and rows
    ≥ start[b] + nnew[b] are not written.  ``kv_len_max`` is a host bound on max(start + nnew)
    (default Tmax).  Returns [B, Tn, H·D] with exact zeros on the padding rows.  GPU bf16 (qkv and
    caches), head dim 64 or 128 (the caches' last dim; ``rope`` tables [≥ Tmax, D/2]) →
    ``csrc/kernels/append.hip``; elsewhere — CPU, other dtypes, other head dims — the same math in
    PyTorch (:func:`append_attention_reference`)."""
    import torch

    D = k_cache.shape[-1]
    sc = float(scale) if scale is not None else D ** -0.5
    if append_supported(qkv, k_cache, n_head):
        _require()
        Tmax = k_cache.shape[2]
        cos, sin = rope if rope is not None else (None, None)
        if qkv.stride(-1) != 1 or qkv.stride(0) % 8 or qkv.stride(1) % 8 or qkv.data_ptr() % 16:
            qkv = qkv.contiguous()
        return torch.ops.nbd.append_attn(qkv, k_cache, v_cache, start, nnew, int(n_head), sc,
                                         int(kv_len_max or Tmax), cos, sin)
    return append_attention_reference(qkv, k_cache, v_cache, start, nnew, n_head, sc, rope, kv_len_max)


# ------------------------------------------------------------------ small-M fused linear (K14)
_NORM = {None: 0, "ln": 1, "rms": 2}
_ACT = {"none": 0, "gelu": 1, "swiglu": 2}


def _lds_bytes(M: int, K: int, norm: int, act: int) -> int:
    mt = 1 if norm else -(-M // 16)  # the kernel falls back to one m-tile per workgroup
    return (mt * 16 * (K + 8) * 2 + 4 * K if norm else 0) + 8 * (2 if act == 2 else 1) * mt * 256 * 4


def linear_small_supported(x, w, norm=None, act: str = "none") -> bool:
    import torch

    M, K = x.shape
    return (x.is_cuda and x.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and 1 <= M <= 64
            and K % 32 == 0 and K <= (2048 if act == "swiglu" else 4096) and x.stride(-1) == 1
            and _lds_bytes(M, K, _NORM[norm[0] if norm else None], _ACT[act]) <= 160 * 1024)


def _apply_norm(x, norm):
    from .norm import layer_norm, rms_norm

    return layer_norm(x, norm[1], norm[2], norm[3]) if norm[0] == "ln" else rms_norm(x, norm[1], norm[2])


def linear_small_reference(x, w, bias=None, norm=None, act: str = "none", residual=None):
    """PyTorch version of :func:`linear_small` (fp32 math, output in x's dtype)."""
    import torch
    import torch.nn.functional as F

    h = x
    if norm is not None:
        if norm[0] == "ln":
            h = F.layer_norm(x.float(), (x.shape[-1],), norm[1].float(), norm[2].float(), norm[3]).to(x.dtype)
        else:
            xf = x.float()
            h = (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + norm[2]) * norm[1].float()).to(x.dtype)
    y = h.float() @ w.float().t()
    if act == "swiglu":
        g, u = y.chunk(2, -1)
        y = F.silu(g) * u
    if bias is not None:
        y = y + bias.float()
    if act == "gelu":
        y = F.gelu(y, approximate="tanh")
    if residual is not None:
        y = y + residual.float()
    return y.to(x.dtype)


# Measured on MI355X (benchmarks/smallm_bench.py, profiles/smallm_bench_r2.txt), graph-replayed:
# the in-kernel norm prologue is recomputed by every workgroup — a win up to ~8 rows (one node
# instead of two), a loss beyond (+10 µs at 64 rows vs a 2-3 µs norm kernel); and hipBLASLt
# beats this kernel on the LM head (N ≈ 50k) from a few rows up.
FUSE_NORM_MAX_ROWS = 8
LIBRARY_MIN_N = 16384
LIBRARY_MIN_ROWS = 4


def linear_small(x, w, bias=None, norm=None, act: str = "none", residual=None):
    """``residual + act(norm(x) · Wᵀ + bias)`` for a few token rows (decode), one HIP kernel.

    ``x`` [M ≤ 64, K]; ``w`` [N, K] (``act="swiglu"``: [gate; up] = [2N, K], out = silu(g)·u);
    ``norm`` = ``("ln", γ, β, eps)`` or ``("rms", γ, eps)`` applied to x first; ``residual``
    [M, N].  GPU bf16 → ``csrc/kernels/smallm.hip``; elsewhere the same math in PyTorch."""
    import torch
    import torch.nn.functional as F

    if act == "swiglu" and bias is not None:
        raise ValueError("linear_small: no bias with SwiGLU")
    M = x.shape[0]
    if norm is not None and x.is_cuda and M > FUSE_NORM_MAX_ROWS:
        x, norm = _apply_norm(x, norm), None
    if x.is_cuda and M >= LIBRARY_MIN_ROWS and w.shape[0] >= LIBRARY_MIN_N and act == "none" and residual is None:
        return F.linear(x if norm is None else _apply_norm(x, norm), w, bias)
    if linear_small_supported(x, w, norm, act):
        _require()
        nk = _NORM[norm[0] if norm else None]
        nw = norm[1] if norm else None
        nb = norm[2] if norm and norm[0] == "ln" else None
        eps = float(norm[-1]) if norm else 0.0
        return torch.ops.nbd.linear_small(x, w, bias, nw, nb, eps, nk, _ACT[act], residual)
    # the same steps as separate ops (more rows than the kernel takes, CPU, other dtypes)
    from .llama import swiglu

    h = x if norm is None else _apply_norm(x, norm)
    y = F.linear(h, w, bias)
    if act == "gelu":
        y = F.gelu(y, approximate="tanh")
    elif act == "swiglu":
        y = swiglu(y)
    return y if residual is None else residual + y
