"""Plain-PyTorch reference for the bf16 MFMA GEMMs (csrc/kernels/gemm.hip, gemm256.hip,
gemm_common.h) in the conventions of tests/refmath.py: hand-written fp64 formulas for the product
and every fused epilogue (no autograd), an emulation of the kernels' rounding points, deliberately
wrong "mutants" of the same formulas, a two-dimensional tile-wise metric, a signed-bias figure for
the rounding direction and a structured input generator.  Device-agnostic; never touches
``torch.ops.nbd``.

Why not ``max|x - ref| / max|ref|`` on ``randn``: with K = 256 the pre-activations have a standard
deviation of 16, so GELU and SiLU are the identity or zero almost everywhere; a wrong 16x16
fragment in a small-magnitude region hides below the tensor's maximum; and a bound of five bf16
roundings cannot tell truncation from round-to-nearest (tests/test_gemm_ref.py measures all three).

Conventions (tests/refmath.py)
  * ``emulate=False``: fp64 throughout, on the bf16 inputs as given.
  * ``emulate=True``: the same formulas with the kernels' rounding points and nothing else; each
    point names its line below.  ``tile256=True`` selects gemm256.hip's epilogue, which rounds the
    pre-activation / the plain product to bf16 *before* GELU / GELU' (its C tile goes through LDS
    as bf16); gemm.hip applies both to the unrounded fp32 value.
  * ``mutant=<name>``: one wrong formula (GEMM_MUTANTS) reachable by a one-line slip in the
    kernels.  ``bm`` / ``bn`` / ``kgroups`` give the tile geometry the slip lives in.
The fast ``exp2`` / ``rcp`` forms of ``sig2_of`` / ``sigm`` (gemm_common.h) are not modelled: their
error is an fp32 ulp or two, far below the one bf16 rounding that follows.
"""
import math

import torch

from refmath import _f32, _rd

EPI_NONE, EPI_GELU, EPI_DGELU, EPI_ROWSUM, EPI_SWIGLU, EPI_DSWIGLU = 0, 1, 2, 3, 4, 5
BETA = 0.7978845608028654  # sqrt(2/pi)   (gemm_common.h kBeta)
KAPPA = 0.044715           # (gemm_common.h kKappa)
BK = 64                    # K-tile depth (gemm_common.h BK); one MFMA step is 32 deep
BF = torch.bfloat16

GEMM_MUTANTS = ("trunc", "gelu_silu", "gelu_relu", "gelu_before_bias", "dgelu_first_term_only", "swiglu_relu_gate",
                "swiglu_halves_swapped", "swiglu_up_rows", "dswiglu_swapped", "bias_frag_shift", "bias_last_tile",
                "drop_kstep", "drop_last_ktile", "rowsum_kgroup", "rowsum_last_split", "slab_last", "frag_transposed")


# ------------------------------------------------------------------------------------ the metrics
def _tiles(t, rows, cols):
    """[M, N] -> [ceil(M/rows), ceil(N/cols), rows·cols], zero-padded."""
    M, N = t.shape
    pr, pc = (-M) % rows, (-N) % cols
    if pr or pc:
        t = torch.nn.functional.pad(t, (0, pc, 0, pr))
    nr, nc = (M + pr) // rows, (N + pc) // cols
    return t.reshape(nr, rows, nc, cols).permute(0, 2, 1, 3).reshape(nr, nc, rows * cols)


def _as2d(x, ref):
    x, ref = x.detach().double(), ref.detach().double()
    assert x.shape == ref.shape, (x.shape, ref.shape)
    if x.dim() == 1:  # a [M] vector counts as one column
        x, ref = x[:, None], ref[:, None]
    assert x.dim() == 2, x.shape
    return x, ref


def tile_rel2(x, ref, rows, cols):
    """``refmath.tile_rel`` over two-dimensional tiles: max over (rows x cols) tiles of
    max|x - ref| in the tile over max|ref| in the tile.  A tile whose reference is all zero scores
    0 if x is zero there too, else inf.  A [M] vector counts as one column."""
    x, ref = _as2d(x, ref)
    e = _tiles((x - ref).abs(), rows, cols).amax(-1)
    m = _tiles(ref.abs(), rows, cols).amax(-1)
    r = torch.where(m > 0, e / m.clamp_min(1e-300), torch.where(e > 0, torch.full_like(e, math.inf), e))
    return float(r.max())


def signed_bias(x, ref, rows=16, cols=16):
    """mean of sign(ref)·(x - ref)/|ref| over the elements whose |ref| is at least a quarter of
    their (rows x cols) tile's maximum: ~0 for round-to-nearest, about -2.8e-3 for a bf16 result
    truncated towards zero."""
    x, ref = _as2d(x, ref)
    M, N = ref.shape
    m = _tiles(ref.abs(), rows, cols).amax(-1)  # [nr, nc]
    tmax = m.repeat_interleave(rows, 0).repeat_interleave(cols, 1)[:M, :N]
    keep = (ref.abs() >= 0.25 * tmax) & (ref != 0)
    rel = torch.sign(ref) * (x - ref) / ref.abs().clamp_min(1e-300)
    return float(rel[keep].mean())


# --------------------------------------------------------------------------------- the activations
def _sigmoid(x):
    return 1.0 / (1.0 + torch.exp(-x))


def gelu_tanh(x):
    """0.5·x·(1 + tanh u) = x·σ(2u), u = β(x + κx³)   (gemm_common.h gelu_tanh)"""
    return x * _sigmoid(2.0 * BETA * (x + KAPPA * x * x * x))


def dgelu_tanh(x, mutant=None):
    """s + 2x·s(1−s)·β(1 + 3κx²), s = σ(2u)   (gemm_common.h dgelu_tanh)"""
    s = _sigmoid(2.0 * BETA * (x + KAPPA * x * x * x))
    if mutant == "dgelu_first_term_only":
        return s
    return s + 2.0 * x * s * (1.0 - s) * BETA * (1.0 + 3.0 * KAPPA * x * x)


def silu(x):
    return x * _sigmoid(x)


def _trunc_bf16(x):
    """x (fp64) truncated towards zero to bf16: the low 16 bits of its fp32 image dropped."""
    f = x.to(torch.float32)  # (the fp32 rounding is 2^-16 of a bf16 step)
    return (f.view(torch.int32) & -65536).view(torch.float32).to(x.dtype)


def _mats(a, b, a_km, b_kn):
    A = a.double().t() if a_km else a.double()  # [M, K]
    B = b.double() if b_kn else b.double().t()  # [K, N]
    assert A.shape[1] == B.shape[0], (A.shape, B.shape)
    return A, B


def _acc(A, B, k0, k1, emulate):
    """Σ_{k0 <= k < k1} A[:, k]·B[k, :]; emulated: an fp32 accumulator over 32-deep MFMA steps
    (gemm.hip compute `acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf[i], af[j], acc[i][j]`)."""
    if not emulate:
        return A[:, k0:k1] @ B[k0:k1]
    acc = torch.zeros(A.shape[0], B.shape[1], dtype=torch.float64, device=A.device)
    for k in range(k0, k1, 32):
        acc = _f32(acc + A[:, k:k + 32] @ B[k:k + 32])
    return acc


def _frag(M, N, bm, bn):
    """the 16x16 fragment the one-fragment mutants hit: the second fragment row of the last row
    tile, the second fragment column of the last column tile."""
    return slice(M - bm + 16, M - bm + 32), slice(N - bn + 16, N - bn + 32)


def gemm_ref(a, b, a_km, b_kn, *, bias=None, epi=EPI_NONE, aux=None, splits=1, emulate=False, mutant=None,
             tile256=False, bm=128, bn=128, kgroups=1):
    """C[M, N] = A·B for bf16 ``a`` [M, K] (or [K, M] with ``a_km``) and ``b`` [N, K] (or [K, N]
    with ``b_kn``) with the epilogues of gemm_common.h, in fp64.  Returns what the op returns:
      EPI_NONE     c = A·B + bias
      EPI_GELU     (gelu(pre), pre), pre = A·B + bias
      EPI_DGELU    c = (A·B)·gelu'(aux), aux [M, N]
      EPI_ROWSUM   (c, Σ_k A[m, k])
      EPI_SWIGLU   b = [gate; up] [2I, K]: (silu(g)·u [M, I], [g|u] [M, 2I])
      EPI_DSWIGLU  aux = [g|u] [M, 2N]: d[g|u] [M, 2N] = [dact·u·σ(g)(1 + g(1−σ(g))) | dact·silu(g)]
    ``splits``: split-K slabs (plain and row-sum products)."""
    assert mutant is None or mutant in GEMM_MUTANTS, mutant
    A, B = _mats(a, b, a_km, b_kn)
    M, K = A.shape
    N = B.shape[1]
    S = splits
    assert K % (BK * S * kgroups) == 0, (K, S, kgroups)
    assert S == 1 or (epi in (EPI_NONE, EPI_ROWSUM) and bias is None)
    rd = _trunc_bf16 if mutant == "trunc" else (lambda t: _rd(t, BF))
    out = rd if (emulate or mutant == "trunc") else (lambda t: t)  # the one rounding of a stored bf16 result
    f32 = _f32 if emulate else (lambda t: t)
    Ks = K // S

    # ---- the product: S slabs, each an fp32 accumulator; gemm.hip reduce_kernel
    # `for (int s = 1; s < splits; ++s) ... v[e] += w[e]` sums them in slab order in fp32
    slabs = [_acc(A, B, s * Ks, (s + 1) * Ks, emulate) for s in range(S)]
    if mutant == "slab_last":
        assert S > 1
        slabs = slabs[:-1]
    acc = slabs[0]
    for t in slabs[1:]:
        acc = f32(acc + t)
    fr, fc = _frag(M, N, bm, bn)
    if mutant == "drop_kstep":  # the first 32-deep step of the last K-tile, in one fragment
        acc = acc.clone()
        acc[fr, fc] -= A[fr, K - 64:K - 32] @ B[K - 64:K - 32, fc]
    if mutant == "drop_last_ktile":  # the ring's last K-tile never computed by the last row tile
        acc = acc.clone()
        acc[M - bm:] -= A[M - bm:, K - 64:] @ B[K - 64:]
    if mutant == "frag_transposed":
        acc = acc.clone()
        acc[fr, fc] = acc[fr, fc].t().clone()

    # ---- row sums (EPI_ROWSUM): gemm.hip compute `accb[j] = mfma(ones, af[j], accb[j])`, fp32 per
    # (split, K-group); the second group's are added in the epilogue (`accb[j][0] += rsb[...]`),
    # the splits' partials by reduce_kernel; one rounding (`p.aux_out[m] = f32_to_bf16(...)`)
    rs = None
    if epi == EPI_ROWSUM:
        assert a_km and b_kn and bias is None
        parts = []
        for s in range(S):
            tot = torch.zeros(M, dtype=torch.float64, device=A.device)
            for t, k0 in enumerate(range(s * Ks, (s + 1) * Ks, BK)):
                if mutant == "rowsum_kgroup":
                    assert kgroups == 2
                    if t % 2 == 1:  # K-tile of the second group: its sums stay in rsb
                        continue
                tot = f32(tot + A[:, k0:k0 + BK].sum(1))
            parts.append(tot)
        if mutant == "rowsum_last_split":
            assert S > 1
            parts = parts[:-1]
        rs = parts[0]
        for t in parts[1:]:
            rs = f32(rs + t)
        return out(acc), out(rs)

    if epi == EPI_SWIGLU:
        # gemm.hip `store8_nt(p.aux_out + m * p.N + j, g)`: [g|u] is the fp32 accumulator rounded;
        # `g[e] = g[e] * sigm(g[e]) * u[e]` takes the unrounded g and u
        assert not a_km and not b_kn and bias is None and N % 2 == 0
        I = N // 2
        g, u = acc[:, :I], acc[:, I:]
        if mutant == "swiglu_up_rows":  # Pieces split_rows from I + n0 instead of I + n0/2
            j = torch.arange(I, device=A.device)
            u = u[:, (j + (j // (bn // 2)) * (bn // 2)) % I]
        if mutant == "swiglu_relu_gate":
            act = g.clamp_min(0) * u
        elif mutant == "swiglu_halves_swapped":
            act = silu(u) * g
        else:
            act = silu(g) * u
        return out(act), out(torch.cat([g, u], 1))

    if epi == EPI_DSWIGLU:
        # gemm.hip `d[e] = d[e] * u[e] * sg * (1.f + g[e] * (1.f - sg))`: d is the unrounded fp32
        # dact, g and u the stored bf16 pre-activations; dact itself is never rounded
        assert not a_km and b_kn and bias is None and aux.shape == (M, 2 * N)
        g, u = aux.double()[:, :N], aux.double()[:, N:]
        sg = _sigmoid(g)
        dg, du = acc * u * sg * (1.0 + g * (1.0 - sg)), acc * g * sg
        if mutant == "dswiglu_swapped":
            dg, du = du, dg
        return out(torch.cat([dg, du], 1))

    pre = acc
    if bias is not None and epi in (EPI_NONE, EPI_GELU):
        bv = bias.double().expand(M, N)
        if mutant == "bias_frag_shift":  # one fragment reads its bias 4 columns over
            bv = bv.clone()
            bv[fr, fc] = bias.double()[fc.start + 4:fc.stop + 4]
        if mutant == "bias_last_tile":
            bv = bv.clone()
            bv[:, N - bn:] = 0
        if mutant == "gelu_before_bias":
            assert epi == EPI_GELU
            return out(gelu_tanh(acc) + bv), out(f32(acc + bv))
        # gemm.hip `v[e] += b[e]` / `pack2_bf16(v[0] + bv[0], ...)`: added in fp32, before the one rounding
        pre = f32(acc + bv)
    if emulate and tile256:
        # gemm256.hip `w.x = pack2(v[0] + bv[0], v[1] + bv[1])`: the C tile goes through LDS as
        # bf16, so GELU / GELU' (`load8<bf16_t>(smem + r * CST + cn * 2, v)`) see the rounded value
        pre = rd(pre)
    if epi == EPI_NONE:
        return out(pre)
    if epi == EPI_GELU:
        # gemm.hip `store8_nt(p.aux_out + off, v)` then `v[e] = gelu_tanh(v[e])`: the activation of
        # the unrounded fp32 pre-activation; the stored pre-activation is that value rounded
        act = silu(pre) if mutant == "gelu_silu" else pre.clamp_min(0) if mutant == "gelu_relu" else gelu_tanh(pre)
        return out(act), out(pre)
    if epi == EPI_DGELU:
        # gemm.hip `v[e] *= dgelu_tanh(h[e])`: the unrounded fp32 product times gelu'(bf16 aux)
        assert not a_km and b_kn and aux.shape == (M, N)
        return out(pre * dgelu_tanh(aux.double(), mutant))
    raise ValueError(f"epilogue {epi}")


def gemm_pair_ref(dy, w, x, *, epi1=EPI_NONE, aux1=None, epi2=EPI_NONE, splits=1, emulate=False, mutant=None,
                  bm=128, bn=128):
    """The grouped backward launch (gemm.hip pair_kernel) for dy [M, N], w [N, K], x [M, K]:
    dx = dy·w with EPI_NONE / EPI_DGELU / EPI_DSWIGLU, dW = dyᵀ·x with EPI_NONE / EPI_ROWSUM, the
    second split ``splits`` ways along its K (= M).  Returns dx, dw, db (None without row sums)."""
    assert epi1 in (EPI_NONE, EPI_DGELU, EPI_DSWIGLU) and epi2 in (EPI_NONE, EPI_ROWSUM)
    kw = dict(emulate=emulate, mutant=mutant, bm=bm, bn=bn)
    dx = gemm_ref(dy, w, False, True, epi=epi1, aux=aux1, **kw)
    r = gemm_ref(dy, x, True, True, epi=epi2, splits=splits, **kw)
    dw, db = r if epi2 == EPI_ROWSUM else (r, None)
    return dx, dw, db


# ------------------------------------------------------------------------------------- the inputs
_SCALES = {  # (row-block cycle of A, row-block cycle of B): neighbours (cyclically) >= 4x apart
    False: ((1.0, 1 / 8, 4.0, 1 / 32, 1 / 4), (1.0, 16.0, 1 / 4)),       # products 1/128 .. 64: 3.9 decades
    True: ((1.0, 1 / 4, 1.0, 4.0), (1.0, 1 / 4, 2.0, 1 / 2, 4.0)),       # within [1/16, 8]; half the
}                                                                        # fragments at 1/2 .. 2 x unit


def block_scales(n, cycle):
    """[n] scale per row: piecewise constant over aligned blocks of 16, cycling through ``cycle``."""
    c = torch.tensor(cycle, dtype=torch.float64)
    return c[(torch.arange(n) // 16) % len(cycle)]


def _check_scales(s):
    blk = s[::16]
    if blk.numel() > 1:
        r = blk[1:] / blk[:-1]
        assert bool((torch.maximum(r, 1 / r) >= 4).all()), "neighbouring 16-row blocks differ by >= 4x"


def gemm_inputs(M, N, K, a_km, b_kn, seed, *, act=False):
    """Structured GEMM operands, seeded on the CPU; returns a dict of bf16 ``a`` ([M, K] or [K, M]),
    ``b`` ([N, K] or [K, N]), ``bias`` [N], ``aux`` [M, N] (a GELU pre-activation) and ``aux2``
    [M, 2N] (SwiGLU [g|u] pre-activations).
      * A[m, k] = sa[m]·wk[k]·(noise + μ_m), B[k, n] = sb[n]·wk[k]·noise with sa / sb piecewise
        constant over aligned blocks of 16 output rows / columns, neighbours >= 4x apart: every
        16x16 output fragment has its own magnitude (products over > 3 decades; none zero);
      * μ_m = ±(0.25 .. 1) σ per output row: the row sums Σ_k A[m, k] do not cancel; B is zero-mean;
      * wk = 2 over the first and the last 32 k: those MFMA steps carry 4x the weight of the rest
        in the product, so a ring's first or last step missing is large;
      * ``act``: block scales within [1/16, 8] around a pre-activation standard deviation of 1.5
        in the unit-scale blocks — where GELU and SiLU bend; at least a quarter of the fragments
        have a standard deviation in [0.5, 3] (asserted);
      * bias: distinct per column, magnitude 0.5 .. 1.5 of the product's standard deviation in
        that column's block (unit row scale);
      * aux / aux2: noise with the ``act`` block scales around a standard deviation of 1.5."""
    assert M % 16 == 0 and N % 16 == 0 and K % BK == 0
    g = torch.Generator(device="cpu").manual_seed(seed)
    ca, cb = _SCALES[bool(act)]
    sa, sb = block_scales(M, ca), block_scales(N, cb)
    _check_scales(sa)
    _check_scales(sb)
    wk = torch.ones(K, dtype=torch.float64)
    wk[:32] = 2.0
    wk[K - 32:] = 2.0
    sgn = torch.where(torch.rand(M, generator=g) < 0.5, -1.0, 1.0)
    mu = (sgn * (0.25 + 0.75 * torch.rand(M, generator=g))).double()
    # unit-block standard deviation of the product: sqrt(Σ_k wk⁴ · (1 + E μ²)), E μ² = 0.4375
    sigma0 = math.sqrt(float((wk ** 4).sum()) * 1.4375)
    gain = math.sqrt(1.5 / sigma0) if act else 1.0  # on both operands
    sig = 1.5 if act else sigma0
    A = gain * sa[:, None] * wk[None, :] * (torch.randn(M, K, generator=g).double() + mu[:, None])
    B = gain * sb[None, :] * wk[:, None] * torch.randn(K, N, generator=g).double()
    a = (A.t() if a_km else A).contiguous().to(BF)
    b = (B if b_kn else B.t()).contiguous().to(BF)
    bs = torch.where(torch.rand(N, generator=g) < 0.5, -1.0, 1.0) * (0.5 + torch.rand(N, generator=g))
    bias = (sig * sb * bs.double()).to(BF)
    xa, xb = _SCALES[True]
    xs = block_scales(M, xa)[:, None]
    aux = (1.5 * xs * block_scales(N, xb)[None, :] * torch.randn(M, N, generator=g).double()).to(BF)
    aux2 = (1.5 * xs * block_scales(2 * N, xb)[None, :] * torch.randn(M, 2 * N, generator=g).double()).to(BF)
    if act:
        std = _tiles(A.float() @ B.float(), 16, 16).std(-1)
        share = float(((std >= 0.5) & (std <= 3.0)).float().mean())
        assert share >= 0.25, f"only {share:.2f} of the fragments have a pre-activation std in [0.5, 3]"
    assert bool((_tiles(a.float().t() if a_km else a.float(), 16, K).abs().amax(-1) > 0).all())
    assert bool((_tiles(b.float() if not b_kn else b.float().t(), 16, K).abs().amax(-1) > 0).all())
    return {"a": a, "b": b, "bias": bias, "aux": aux, "aux2": aux2}
