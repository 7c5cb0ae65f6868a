"""Plain-PyTorch references of the two kernels that run on every generated token, in the
conventions of tests/refmath.py and tests/refmath_append.py: fp64 formulas (no autograd), an
emulation of the kernels' rounding points (``emulate=True``), deliberately wrong mutants, and
structured inputs.  Never touches ``torch.ops.nbd``; everything is seeded on the CPU.

``decode_ref``        csrc/kernels/decode.hip ``decode_kernel`` / ``merge_kernel``: one new token per
                      sequence; its (rotated) k and v become cache row pos[b], its query attends
                      rows 0..pos[b].
``linear_small_ref``  csrc/kernels/smallm.hip ``linear_small_kernel``:
                      out = residual + act(norm(x)·Wᵀ + bias), epilogue order bias → GELU → SwiGLU
                      → residual.

Rounding points of decode.hip (they differ from append.hip's): bf16 inputs; the rotated k rounded
to bf16 (`knew = pack8(kf)`) while the rotated q stays fp32 (`rope_lane(q[g], ...)`); `p.scale2 =
(float)scale * kLog2e` in fp32 and `q[g][e] *= p.scale2`; scores, p and both sums in fp32 with no
bf16 P (`o[g][e] += pu * vf[e]`); the output rounded to bf16 (`f32_to_bf16(O / L)`).

Rounding points of smallm.hip: bf16 inputs; the normalised x rounded to bf16 (`prologue`'s
`store8<bf16_t>`), its statistics in fp32 over two passes (`mean[j] = wave_sum(s[j]) / K`, then
`q[j] = fmaf(d, d, q[j])`); fp32 MFMA accumulation and an fp32 epilogue; the output rounded to
bf16 (`a.out[...] = f32_to_bf16(y)`).
"""
import math

import torch

import refmath as rm

D = 64
DECODE_MUTANTS = ("mask_plus1", "new_key_dropped", "stale_new_key", "rope_prev_pos", "rope_sign", "rope_k_unrotated",
                  "gqa_mod", "chunk_head_dropped", "merge_unweighted", "empty_chunk_live")
LINEAR_MUTANTS = ("ln_no_mean", "ln_no_beta", "no_eps", "stats_row_minus8", "k_tail_dropped", "bias_first_pass_only",
                  "res_first_pass_only", "res_wrong_row", "swiglu_swapped", "swiglu_up_shift", "gelu_before_bias",
                  "row_tail_zero")
POISON = {"loud": (30.0, 1024.0), "huge": (3.0e38, 3.0e38), "nan": (math.nan, math.nan)}


# ------------------------------------------------------------------------------------ decode
def decode_plan(BHkv, kv_len):
    """(nchunks, chunk) as decode.hip ``plan()`` sizes them: no split up to 512 keys, then enough
    chunks of >= 256 keys for 512 workgroups, chunk widths a multiple of the 32 lane groups."""
    nc = 1
    if kv_len > 512:
        nc = max(1, -(-512 // BHkv))
        nc = min(nc, -(-kv_len // 256), 64)
    ch = -(-kv_len // nc)
    ch = -(-ch // 32) * 32
    return -(-kv_len // ch), ch


def decode_ref(qkv, k_cache, v_cache, pos, n_head, scale, rope=None, *, emulate=False, mutant=None, chunk=None,
               kv_len_max=None):
    """Returns ``out`` [B, H·64] and the updated caches, all fp64.  ``pos``: a sequence of ints
    (clamped into [0, Tmax - 1] as the kernel clamps).  ``chunk``: the key-chunk width of the
    flash-decoding split, for the three chunk mutants only (``kv_len_max``, default Tmax, gives
    the number of chunks)."""
    assert mutant is None or mutant in DECODE_MUTANTS, mutant
    bf = torch.bfloat16
    B, W = qkv.shape
    Hkv, Tmax = k_cache.shape[1], k_cache.shape[2]
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
        q = rm.rot(q, cos, sin, rpos)
        if mutant != "rope_k_unrotated":
            k = rm.rot(k, cos, sin, rpos)
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
    s2 = torch.einsum("bkgd,bktd->bkgt", qg, ak)
    if emulate:  # `acc += q[g][e] * kf[e]`, `sum8(acc)`: fp32
        s2 = rm._f32(s2)
    s2 = s2.masked_fill(~vis[:, None, None, :], -math.inf)
    m = s2.amax(-1, keepdim=True)
    m = torch.where(m == -math.inf, torch.zeros_like(m), m)
    p = torch.exp2(s2 - m)
    if emulate:  # `pu = exp2f(s[u][g] - ms)`: fp32, never packed to bf16
        p = rm._f32(p)
    if mutant in ("merge_unweighted", "empty_chunk_live"):
        nch = -(-(kv_len_max or Tmax) // chunk)
        pad = nch * chunk - Tmax
        pp = torch.nn.functional.pad(p, (0, pad)) if pad > 0 else p[..., : nch * chunk]
        vv = torch.nn.functional.pad(av, (0, 0, 0, pad)) if pad > 0 else av[:, :, : nch * chunk]
        pp = pp.reshape(*p.shape[:3], nch, chunk)
        vv = vv.reshape(vv.shape[0], vv.shape[1], nch, chunk, D)
        lc = pp.sum(-1)  # [B, kv, G, nch]: the chunks' l on the common maximum
        oc = torch.einsum("bkgct,bkctd->bkgcd", pp, vv) / lc.clamp_min(1e-300)[..., None]
        live = lc > 0
        if mutant == "merge_unweighted":  # the partials averaged without exp2(l - max)
            o = (oc * live[..., None]).sum(-2) / live.sum(-1, keepdim=True).clamp_min(1)
        else:  # a chunk past pos (o = 0) joins the merge with weight 1
            wc = lc / lc.amax(-1, keepdim=True).clamp_min(1e-300)
            empty = (torch.arange(nch)[None, :] * chunk > pos[:, None]).sum(-1).double()[:, None, None, None]
            o = (wc[..., None] * oc).sum(-2) / (wc.sum(-1, keepdim=True) + empty)
    else:
        l = p.sum(-1, keepdim=True)
        o = torch.einsum("bkgt,bktd->bkgd", p, av) / l.clamp_min(1e-300)
    out = o.reshape(B, H * D)
    if emulate:
        out = rm._rd(out, bf)
    return out, kc, vc


def decode_per_head(out, n_head):
    """[B, H·64] -> [B, H, 1, 64]: ``refmath.tile_rel(..., rows=1)`` then scores one head row."""
    return out.reshape(out.shape[0], n_head, 1, D)


def decode_history(B, H, Hkv, Tmax, seed, gain=2.0):
    """The draw behind ``decode_inputs``, before any poison: fp32 qkv [B, (H + 2·Hkv)·64], caches
    [B, Hkv, Tmax, 64] and the poison's signs.  q, k, v as ``refmath.attn_inputs`` /
    ``append_inputs`` draw them: a per-head mean on k and v, scores a few nats wide, so single
    keys carry weight."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    q = gain * torch.randn(B, H, D, generator=g)
    kmean, vmean = 0.5 * torch.randn(B, Hkv, 1, D, generator=g), torch.randn(B, Hkv, 1, D, generator=g)
    k = gain * torch.randn(B, Hkv, D, generator=g) + kmean[:, :, 0]
    v = torch.randn(B, Hkv, D, generator=g) + vmean[:, :, 0]
    qkv = torch.cat([q.reshape(B, -1), k.reshape(B, -1), v.reshape(B, -1)], -1)
    kc = gain * torch.randn(B, Hkv, Tmax, D, generator=g) + kmean
    kc[:, :, ::32] *= 2.0  # lane group 0's keys — every chunk's first key is one — score twice as wide
    vc = torch.randn(B, Hkv, Tmax, D, generator=g) + vmean
    sign = torch.where(torch.rand(2, B, Hkv, Tmax, D, generator=g) < 0.5, -1.0, 1.0)
    return qkv, kc, vc, sign


def decode_poison(hist, pos, poison="loud"):
    """bf16 (qkv, k_cache, v_cache) of a ``decode_history`` draw with the cache rows >= pos[b] —
    the row at pos itself included: the kernel must use its register copy of the new key —
    holding poison, as in ``refmath_append.append_inputs``:
      ``loud``  k = ±30, v = ±1024: a wrong formula that reads one stays finite and moves the
                result by orders of magnitude (the CPU mutant proof);
      ``huge``  ±3e38, the largest finite bf16 magnitudes;
      ``nan``   NaN."""
    qkv, kc, vc, sign = hist
    kp, vp = POISON[poison]
    Tmax = kc.shape[2]
    free = (torch.arange(Tmax)[None, :] >= torch.as_tensor(pos)[:, None])[:, None, :, None]
    kc, vc = torch.where(free, kp * sign[0], kc), torch.where(free, vp * sign[1], vc)
    return qkv.bfloat16(), kc.bfloat16(), vc.bfloat16()


def decode_inputs(B, H, Hkv, Tmax, pos, seed, poison="loud", gain=2.0):
    return decode_poison(decode_history(B, H, Hkv, Tmax, seed, gain), pos, poison)


def sweep_positions(kv_len, launch, B=64):
    """positions of launch ``launch`` of a sweep over every pos in [0, kv_len) with B per launch:
    strided through the whole range, so every launch has early, late and empty chunks."""
    n = -(-kv_len // B)
    return [(launch + n * b) % kv_len for b in range(B)]


# the cases of tests/test_gpu_decode_paths.py; tests/test_decode_ref.py proves the mutants on them
SCALE = 0.125
GROUP_HKV = 2
# a dozen positions per cache length: the first rows, the 32-group edge, the 64- and 128-key
# iteration edges, the last row; for 640 (three chunks of 224) both chunk edges from both sides
GROUP_POS = {320: (0, 1, 31, 32, 63, 64, 127, 128, 129, 255, 256, 319),
             640: (0, 33, 127, 128, 223, 224, 225, 351, 447, 448, 449, 639)}


def group_case(G, Tmax, poison, use_rope):
    """(H, Hkv, pos, (qkv, k_cache, v_cache)) of the every-group-size test: 12 sequences, two
    key/value heads of G query heads each."""
    H, pos = G * GROUP_HKV, GROUP_POS[Tmax]
    seed = 1000 * G + Tmax + use_rope
    return H, GROUP_HKV, pos, decode_inputs(len(pos), H, GROUP_HKV, Tmax, pos, seed, poison)


SWEEP_B = 64
SWEEP_POISON = ("nan", "loud", "huge")  # launch i of a sweep takes kind i % 3: NaN where pos is a chunk's first row


def sweep_history(kv_len, G):
    """the unpoisoned draw of the position sweep: 64 sequences, one key/value head of G query
    heads, a cache of exactly kv_len rows."""
    return decode_history(SWEEP_B, G, 1, kv_len, seed=50000 + 10 * kv_len + G)


# ------------------------------------------------------------------------------- linear_small
def linear_small_plan(M, K, N, norm, act):
    """(MT, staged, lds_bytes, grid_x) as ``linear_small_hip`` chooses them (smallm.hip
    ``lds_bytes`` and the lines after it); lds_bytes > 160 KiB means the op refuses the call."""
    def lds(mt, stage):
        xs = mt * 16 * (K + 8) * 2 if stage else 0
        return xs + (4 * K if norm else 0) + 8 * (2 if act == "swiglu" else 1) * mt * 256 * 4
    ntiles = -(-N // 16)
    mt_all = -(-M // 16)
    mt = mt_all
    if mt > 1 and (ntiles < 128 or lds(mt, True) > 160 * 1024):
        mt = 1
    stage = bool(norm) or lds(mt, True) <= 160 * 1024
    return mt, stage, lds(mt, stage), (min(ntiles, 512) if stage else ntiles)


def _gelu_tanh(x):
    return 0.5 * x * (1 + torch.tanh(0.7978845608028654 * (x + 0.044715 * x ** 3)))


def linear_small_ref(x, w, bias=None, norm=None, act="none", residual=None, *, emulate=False, mutant=None, grid=512):
    """out [M, N] fp64.  ``norm`` = ("ln", γ, β, eps) | ("rms", γ, eps) | None; ``act`` = "none" |
    "gelu" | "swiglu" (w = [gate; up]).  ``grid``: the workgroups looping over column tiles, for
    the ``*_first_pass_only`` mutants."""
    assert mutant is None or mutant in LINEAR_MUTANTS, mutant
    bf = torch.bfloat16
    f = lambda t: None if t is None else t.double().cpu()  # noqa: E731
    x, w, bias, residual = f(x), f(w), f(bias), f(residual)
    M, K = x.shape
    h = x
    if norm is not None:
        ln = norm[0] == "ln"
        ct = torch.float32 if emulate else torch.float64  # the prologue computes in fp32
        xs, gam, eps = x.to(ct), norm[1].cpu().to(ct), float(norm[-1])
        mean = xs.mean(-1, keepdim=True) if ln and mutant != "ln_no_mean" else torch.zeros_like(xs[:, :1])
        rstd = torch.rsqrt(((xs - mean) ** 2).mean(-1, keepdim=True) + (0.0 if mutant == "no_eps" else eps))
        if mutant == "stats_row_minus8":  # the wave's second row takes its first row's statistics
            idx = torch.arange(M)
            idx = torch.where(idx >= 8, idx - 8, idx)
            mean, rstd = mean[idx], rstd[idx]
        h = (xs - mean) * rstd * gam
        if ln and mutant != "ln_no_beta":
            h = h + norm[2].cpu().to(ct)
        if emulate:  # `store8<bf16_t>(... xs + r * ld + c, o)`
            h = rm._rd(h, bf)
        h = h.double()
    kk = K - 32 if mutant == "k_tail_dropped" else K
    acc = h[:, :kk] @ w[:, :kk].t()
    if emulate:  # the MFMA accumulators and the cross-wave sum are fp32
        acc = rm._f32(acc)
    swiglu = act == "swiglu"
    N = w.shape[0] // 2 if swiglu else w.shape[0]
    up = None
    if swiglu:
        if mutant == "swiglu_up_shift":  # the up rows taken at 16·⌈N/16⌉ (rows past w: zeros)
            off = -(-N // 16) * 16
            up = torch.zeros(M, N, dtype=torch.float64)
            n_in = max(0, min(N, 2 * N - off))
            up[:, :n_in] = acc[:, off:off + n_in]
        else:
            up = acc[:, N:]
        acc = acc[:, :N]
        if mutant == "swiglu_swapped":
            acc, up = up, acc
    first = (torch.arange(N) // 16 < grid)[None, :]
    y = acc
    late_bias = bias is not None and act == "gelu" and mutant == "gelu_before_bias"
    if bias is not None and not late_bias:
        y = y + (bias * first if mutant == "bias_first_pass_only" else bias)
    if act == "gelu":
        y = _gelu_tanh(y)
        if late_bias:
            y = y + bias
    if swiglu:
        y = y * torch.sigmoid(y) * up
    if residual is not None:
        r = residual.reshape(M, N)
        if mutant == "res_wrong_row":
            r = r.roll(-1, 0)
        y = y + (r * first if mutant == "res_first_pass_only" else r)
    if emulate:
        y = rm._rd(rm._f32(y), bf)
    if mutant == "row_tail_zero":
        y = y.clone()
        y[M // 16 * 16:] = 0
    return y


def tiles16(y):
    """[M, N] -> [⌈N/16⌉, M, 16] (zero columns past N): ``refmath.tile_rel(..., rows=16)`` then
    scores one 16 x 16 output tile, the kernel's MFMA tile."""
    M, N = y.shape
    y = torch.nn.functional.pad(y.double(), (0, (-N) % 16))
    return y.reshape(M, -1, 16).transpose(0, 1)


def linear_small_inputs(M, K, N, norm, act, bias, res, seed, eps=1e-5):
    """bf16 (x, w, bias, norm, residual) for ``linear_small_ref``, seeded on the CPU.
      * x, γ, β as ``refmath.norm_inputs`` draws them: row scales σ log-uniform from sqrt(eps)
        upwards, offsets of several σ (RMSNorm: small on the small rows), γ and β not near 1 and 0;
      * each 16-column tile of w has its own scale, over two decades, so a wrong tile does not
        hide below another tile's magnitude; the last 32 k positions (one MFMA step) carry as much
        weight as all the others together, so a dropped k tail shows at every K;
      * on tiles 1, 4, 7, … the bias is several times the product, on tiles 2, 5, 8, … the
        residual is; elsewhere (tile 0: the only one of a narrow output) both are a fraction of
        it, so that a wrong product does not hide below them."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    d = rm.norm_inputs(M, K, seed + 1, torch.bfloat16, eps, rms=(norm == "rms"), residual=False)
    x = d["x"]
    nrm = None
    if norm == "ln":
        # norm_inputs leaves row 0 (σ = sqrt(eps)) without an offset; a single-row call needs one
        x[0] = (x[0].float() + 3.0 * math.sqrt(eps)).bfloat16()
        nrm = ("ln", d["w"], d["b"], eps)
    elif norm == "rms":
        nrm = ("rms", d["w"], eps)
    Nw = 2 * N if act == "swiglu" else N
    nt = -(-N // 16)
    tscale = 10.0 ** (2.0 * torch.rand(nt, generator=g) - 1.0)
    cscale = tscale.repeat_interleave(16)[:N] * (1 + 0.2 * torch.rand(N, generator=g))
    cscale = torch.cat([cscale, cscale]) if act == "swiglu" else cscale
    w = torch.randn(Nw, K, generator=g) * (cscale * K ** -0.5)[:, None]
    if K > 32:
        w[:, K - 32:] *= math.sqrt(K / 32.0)
    w = w.bfloat16()
    y0 = linear_small_ref(x, w, None, nrm, act, None)  # the product's magnitude, per column
    tile = torch.arange(N) // 16
    b = rs = None
    if bias:
        mag = y0.abs().mean(0) if act != "gelu" else linear_small_ref(x, w, None, nrm, "none", None).abs().mean(0)
        sgn = torch.where(torch.rand(N, generator=g) < 0.5, -1.0, 1.0)
        b = (sgn * mag * torch.where(tile % 3 == 1, 6.0, 0.25) * (1 + 0.3 * torch.rand(N, generator=g))).bfloat16()
        y0 = linear_small_ref(x, w, b, nrm, act, None)
    if res:
        mag = y0.abs().mean(0, keepdim=True)
        rs = (torch.randn(M, N, generator=g) * mag * torch.where(tile % 3 == 2, 6.0, 0.25)[None, :]).bfloat16()
    return x, w, b, nrm, rs


# the (K, N) shapes and the six prologue / epilogue combinations of the GPU numerics test; SwiGLU
# takes K = 2048 where the others take 4096 (the kernel's register budget, SMAX); N = 16389 (1025
# column tiles) goes with the two small K only, to keep its fp64 reference cheap
LINEAR_SHAPES = tuple((K, N) for K in (32, 96, 576, 4096) for N in (8, 48, 272, 2064)) + ((32, 16389), (96, 16389))
LINEAR_COMBOS = ((None, "none", False, False), ("ln", "none", True, False), ("ln", "gelu", True, False),
                 (None, "none", True, True), ("rms", "swiglu", False, False), ("rms", "none", False, True))
LINEAR_ROWS = (1, 8, 9, 16, 17, 33, 64)


def linear_case(M, K, N, combo):
    """the inputs of one GPU numerics case (K = 4096 becomes 2048 under SwiGLU) and its seed."""
    norm, act, bias, res = combo
    if act == "swiglu" and K > 2048:
        K = 2048
    seed = 7 * M + K + 3 * N + 101 * (LINEAR_COMBOS.index(combo) if combo in LINEAR_COMBOS else len(LINEAR_COMBOS))
    return (M, K, N), linear_small_inputs(M, K, N, norm, act, bias, res, seed)
