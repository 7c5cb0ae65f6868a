"""Plain-PyTorch references for the attention and norm kernels: hand-written fp64 forward and
backward formulas (no autograd), an emulation of the roundings the kernels document, deliberately
wrong "mutant" variants of the same formulas, a tile-wise error metric and structured input
generators.  Imported by name from the test modules; never touches ``torch.ops.nbd``.

Why not ``max|x - ref| / max|ref|`` on ``randn``: a late causal query's output and a late key's
gradient are ~1/T of the tensor's maximum, and with iid zero-mean ``dy`` both projection terms of
a norm's dx shrink like 1/sqrt(C) — whole missing terms hide below a global bf16 bound
(tests/test_refmath_mutants.py measures it).

Conventions
  * ``emulate=False``: fp64 throughout, on the inputs as given.
  * ``emulate=True``: the same formulas with the kernels' rounding points and nothing else —
    inputs in the storage dtype, P and dS rounded to bf16 before their products (attn.hip header),
    outputs rounded to the output dtype; each further point names its line below.
  * the residual sum of add+norm is an *output*: the norm is defined on the stored (rounded) sum
    in both modes, as tests/test_gpu_norm.py already models — only then can "y normalises the
    unrounded sum" be told from a correct kernel.
  * ``mutant=<name>``: one wrong formula (ATTN_MUTANTS / NORM_MUTANTS), used to prove that a test
    built on these references can fail.
"""
import math

import torch

LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453

ATTN_MUTANTS = ("mask_wide", "skip_diag", "delta_dropped", "delta_tail", "dkdv_tail", "gqa_mod", "rope_kmod64",
                "dq_norot", "dk_norot", "dk_noscale")
NORM_MUTANTS = ("no_mean_g", "no_proj", "half_mean_g", "half_mean_gx", "no_eps", "neighbour_stats", "no_dres",
                "dw_tail", "y_unrounded_sum")


def _rd(x, dt):
    """x rounded to the storage dtype ``dt``, back in x's own dtype."""
    return x.to(dt).to(x.dtype)


def _f32(x):
    return x.to(torch.float32).to(x.dtype)


# ------------------------------------------------------------------------------------ the metric
def tile_rel(x, ref, rows, valid=None):
    """max over (leading dims, tile of ``rows`` consecutive rows) of max|x - ref| in the tile over
    max|ref| in the tile; x, ref = [..., T, D] (a [C] vector is one row).  ``valid``: only rows
    < valid contribute error (the tiles' maxima still come from the whole reference).  A tile whose
    reference is all zero scores 0 if x is zero there too, else inf."""
    x, ref = x.detach().double(), ref.detach().double()
    assert x.shape == ref.shape, (x.shape, ref.shape)
    if x.dim() == 1:
        x, ref = x[None], ref[None]
    T, D = x.shape[-2], x.shape[-1]
    err = (x - ref).abs().reshape(-1, T, D)
    mag = ref.abs().reshape(-1, T, D)
    if valid is not None:
        err = err.clone()
        err[:, valid:] = 0
    pad = (-T) % rows
    if pad:
        z = err.new_zeros(err.shape[0], pad, D)
        err, mag = torch.cat([err, z], 1), torch.cat([mag, z], 1)
    n = (T + pad) // rows
    e = err.reshape(-1, n, rows * D).amax(-1)
    m = mag.reshape(-1, n, rows * D).amax(-1)
    r = torch.where(m > 0, e / m.clamp_min(1e-300), torch.where(e > 0, torch.full_like(e, math.inf), e))
    return float(r.max())


def max_abs(x, ref, valid=None):
    d = (x.detach().double() - ref.detach().double()).abs()
    if valid is not None:
        d = d[..., :valid]
    return float(d.max())


# ------------------------------------------------------------------------------------- attention
def rope_tables_ref(T, head_dim=64, theta=10000.0, device="cpu"):
    """cos/sin [T, head_dim/2] float32 — the arithmetic of ``ops.rope_tables`` (no scaling)."""
    inv = 1.0 / (theta ** (torch.arange(0, head_dim, 2, dtype=torch.float32, device=device) / head_dim))
    f = torch.outer(torch.arange(T, dtype=torch.float32, device=device), inv)
    return f.cos().contiguous(), f.sin().contiguous()


def rot(x, cos, sin, pos=None):
    """rotate-half RoPE over all 64 dims of x [..., T, 64]: dims d and d + 32 rotate by the angle
    of (position, d) (attn.hip rope8)."""
    c, s = cos.to(x.dtype), sin.to(x.dtype)
    if pos is not None:
        c, s = c[pos], s[pos]
    else:
        c, s = c[: x.shape[-2]], s[: x.shape[-2]]
    a, b = x[..., :32], x[..., 32:]
    return torch.cat([a * c - b * s, b * c + a * s], -1)


def rot_inv(x, cos, sin, pos=None):
    """the transpose rotation: the gradient of ``rot`` (attn.hip store_dT_rope)."""
    return rot(x, cos, -sin, pos)


def _attn_chunk(q, k, v, do, causal, scale, rope, emulate, mutant, gsplit):
    bf = torch.bfloat16
    B, H, T, D = q.shape
    Hkv = k.shape[1]
    group = H // Hkv
    dev = q.device
    q, k, v = q.double(), k.double(), v.double()
    if emulate:
        q, k, v = _rd(q, bf), _rd(k, bf), _rd(v, bf)
    kpos = None
    if rope is not None:
        cos, sin = rope[0].double(), rope[1].double()
        if mutant == "rope_kmod64":  # the key's position taken inside its 64-key tile
            kpos = torch.arange(T, device=dev) % 64
        q, k = rot(q, cos, sin), rot(k, cos, sin, kpos)
        if emulate:  # attn.hip rope8: the rotated q / k go back to bf16 for the MFMAs
            q, k = _rd(q, bf), _rd(k, bf)
    hmap = torch.arange(H, device=dev) // group
    if mutant == "gqa_mod":
        hmap = torch.arange(H, device=dev) % Hkv
    kx, vx = k[:, hmap], v[:, hmap]
    i = torch.arange(T, device=dev)[:, None]
    j = torch.arange(T, device=dev)[None, :]
    masked = torch.zeros(T, T, dtype=torch.bool, device=dev)
    if causal:
        masked = j > i
        if mutant == "mask_wide":  # key i + 1 visible to rows >= 128
            masked = torch.where(i >= 128, j > i + 1, masked)
    if mutant == "skip_diag":  # the last 64 queries never see their diagonal 64-key tile
        masked = masked | ((i >= T - 64) & (j >= T - 64))
    c2 = scale * LOG2E
    if emulate:
        # attn.hip fwd_kernel `sacc[kb] = mfma(..., qf[s], sacc[kb])`: the raw score is an fp32
        # accumulator over four 16-dim MFMA steps, scaled by the fp32 constant
        # sc2 = (float)scale * kLog2e (attn_fwd_hip)
        sraw = torch.zeros(B, H, T, T, dtype=torch.float64, device=dev)
        for d0 in range(0, D, 16):
            sraw = _f32(sraw + q[..., d0:d0 + 16] @ kx[..., d0:d0 + 16].transpose(-1, -2))
        c2 = float(torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32))
    else:
        sraw = q @ kx.transpose(-1, -2)
    s2 = (sraw * c2).masked_fill(masked, -math.inf)  # log2 units
    m = s2.amax(-1, keepdim=True)
    if emulate:
        # fwd_kernel's deferred rescale (`if (__any(mn > m + kDeferLog2))`): a wave of 32 queries
        # sweeps 64-key tiles and moves its running maxima only when one of its rows' maximum grew
        # by more than 2^4, so a tile's P is exp2(s - m_stale) when it is packed to bf16 — the row's
        # largest probability is not exactly 1 and carries a rounding like every other.  mt = the
        # per-(row, key) running maximum in effect at the key's tile; `mn = fmaxf(m, mt * sc2)` and
        # `exp2f(fmaf(sacc, sc2, nmn))` are fp32 each.
        run = torch.full_like(m, -math.inf)
        mt = torch.empty_like(s2)
        l = torch.zeros_like(m)
        for t0 in range(0, T, 64):
            mn = torch.maximum(run, _f32(s2[..., t0:t0 + 64].amax(-1, keepdim=True)))
            grow = (mn > run + 4.0).reshape(B, H, T // 32, 32).any(-1, keepdim=True)
            new = torch.where(grow.expand(B, H, T // 32, 32).reshape(B, H, T, 1), mn, run)
            alpha = torch.where(new > run, torch.exp2(run - new), torch.ones_like(run))
            run = new
            mt[..., t0:t0 + 64] = run
            # `l *= alpha; ... l += rs`: fp32, the tile's unrounded p summed in fp32
            pt = torch.exp2(_f32(sraw[..., t0:t0 + 64] * c2 - run).masked_fill(masked[..., t0:t0 + 64], -math.inf))
            l = _f32(_f32(l * alpha) + pt.float().sum(-1, keepdim=True).double())
        m = run  # (>= the row's true maximum - 4)
        p = torch.exp2(_f32(sraw * c2 - mt).masked_fill(masked, -math.inf))
        wt = torch.exp2(mt - m)  # the later rescales of what a tile added to O (fp32 products)
        out = ((_rd(p, bf) * wt) @ vx) / l  # P packed to bf16 for O += V^T·P (pack_half)
        out = _rd(out, bf)
        lg = _f32(m + _f32(torch.log2(l)))  # fwd_kernel `(m + __log2f(l)) * kLn2`
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
    if mutant == "delta_dropped":
        delta = torch.zeros_like(delta)
    elif mutant == "delta_tail":  # zero for the last 128 queries
        delta = delta.clone()
        delta[:, :, T - 128:] = 0
    l2 = lse.unsqueeze(-1) * LOG2E
    if emulate:  # dkdv_body `lv = lse * kLog2e`, `exp2f(fmaf(sacc, sc2, -Ls))`
        l2 = _f32(l2)
        pn = torch.exp2(_f32(sraw * c2 - l2).masked_fill(masked, -math.inf))
    else:
        pn = torch.exp2(s2 - l2)
    dp = do @ vx.transpose(-1, -2)
    ds = pn * (dp - delta)
    if emulate:  # P and dS packed to bf16 for the dV / dK / dQ products (attn.hip header)
        pn, ds = _rd(pn, bf), _rd(ds, bf)
    dv_h = pn.transpose(-1, -2) @ do
    dq = scale * (ds @ kx)
    dk_h = (1.0 if mutant == "dk_noscale" else scale) * (ds.transpose(-1, -2) @ q)
    if rope is not None:
        if mutant != "dq_norot":
            dq = rot_inv(dq, cos, sin)
        if mutant != "dk_norot":
            dk_h = rot_inv(dk_h, cos, sin, kpos)
    if emulate and gsplit and group > 1:
        # attn_bwd_hip `pk = at::empty({gsplit, B, Hkv, T, D}, q.options())`: with the group split
        # over workgroups each query head's dK / dV partial is stored as bf16 before the fp32 sum
        dk_h, dv_h = _rd(dk_h, bf), _rd(dv_h, bf)
    dk = torch.zeros(B, Hkv, T, D, dtype=torch.float64, device=dev).index_add_(1, hmap, dk_h)
    dv = torch.zeros(B, Hkv, T, D, dtype=torch.float64, device=dev).index_add_(1, hmap, dv_h)
    if mutant == "dkdv_tail":  # the last key block's gradients never written
        dk[:, :, T - 128:] = 0
        dv[:, :, T - 128:] = 0
    if emulate:
        dq, dk, dv = _rd(dq, bf), _rd(dk, bf), _rd(dv, bf)
    return out, lse, dq, dk, dv


def attn_ref(q, k, v, do, causal, scale, n_kv=None, rope=None, *, emulate=False, mutant=None, gsplit=False,
             chunk=None):
    """softmax(q·kᵀ·scale [+ causal mask])·v and its FA2 backward for q, do [B, H, T, 64] and
    k, v [B, n_kv, T, 64]; ``rope=(cos, sin)``: q and k rotated first, dq / dk rotated back.
    Returns out, lse (and dq, dk, dv unless ``do`` is None), fp64.  ``gsplit``: the kernel splits
    the query-head group over workgroups (emulation only).  ``chunk``: batches per pass."""
    assert mutant is None or mutant in ATTN_MUTANTS, mutant
    B = q.shape[0]
    assert n_kv is None or n_kv == k.shape[1]
    chunk = chunk or B
    parts = []
    for b0 in range(0, B, chunk):
        sl = slice(b0, min(B, b0 + chunk))
        parts.append(_attn_chunk(q[sl], k[sl], v[sl], None if do is None else do[sl], causal, scale, rope, emulate,
                                 mutant, gsplit))
    return tuple(torch.cat([p[n] for p in parts], 0) for n in range(len(parts[0])))


def attn_inputs(B, H, Hkv, T, seed, gain=2.0):
    """bf16 q [B, H, T, 64], k, v [B, Hkv, T, 64], seeded on the CPU: distinct statistics per
    (batch, head) (a per-head mean on k and v) and scores with a standard deviation of a few nats
    (``gain``² · 8 · scale), so that single keys carry weight and one key too many is visible."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    q = gain * torch.randn(B, H, T, 64, generator=g)
    k = gain * torch.randn(B, Hkv, T, 64, generator=g) + 0.5 * torch.randn(B, Hkv, 1, 64, generator=g)
    v = torch.randn(B, Hkv, T, 64, generator=g) + torch.randn(B, Hkv, 1, 64, generator=g)
    return q.bfloat16(), k.bfloat16(), v.bfloat16()


def attn_do(out_ref, seed):
    """dO = noise + 2·out, so that δ = Σ dO·O is not small beside dP."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    n = torch.randn(out_ref.shape, generator=g).to(out_ref.device)
    return (n + 2 * out_ref.float()).bfloat16()


def poisoned_inputs(B, H, Hkv, T, t0, seed, scale, rope=None, margin=25.0):
    """A causal problem and its "poisoned future" twin for the cut t0.  Returns
    ``(q, k, v), (q, kp, vp)``: in the twin, keys at positions >= t0 score at least 20 nats above
    every row's largest legitimate score (all queries share a positive component along one
    direction u of the rotated space; the poisoned keys are β·u) and values there are ±1024.
    A kernel that lets a row < t0 see a key >= t0 — or a row >= t0 with dO = 0 leak into a
    gradient — moves the result by orders of magnitude, not by a rounding."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    u = torch.nn.functional.normalize(torch.randn(64, generator=g), dim=0)
    qn = 1.5 * torch.randn(B, H, T, 64, generator=g)
    a = 3.0 + torch.randn(B, H, T, 1, generator=g).clamp(-1, 1)
    qr = qn - (qn @ u)[..., None] * u + a * u
    kr = 1.5 * torch.randn(B, Hkv, T, 64, generator=g) + 0.5 * torch.randn(B, Hkv, 1, 64, generator=g)
    v = torch.randn(B, Hkv, T, 64, generator=g) + torch.randn(B, Hkv, 1, 64, generator=g)
    if rope is not None:
        cos, sin = rope[0].cpu(), rope[1].cpu()
        unrot = lambda x: rot_inv(x.double(), cos.double(), sin.double()).float()  # noqa: E731
        rerot = lambda x: rot(x.double(), cos.double(), sin.double())  # noqa: E731
    else:
        unrot = lambda x: x  # noqa: E731
        rerot = lambda x: x.double()  # noqa: E731
    q, k, v = unrot(qr).bfloat16(), unrot(kr).bfloat16(), v.bfloat16()
    # β from the data as stored: the largest legitimate score and the smallest component along u
    qd, kd = rerot(q), rerot(k)
    group = H // Hkv
    top = float((qd @ kd.repeat_interleave(group, 1).transpose(-1, -2)).amax()) * scale
    a_min = float((qd @ u.double()).amin())
    assert a_min > 1.0, a_min
    beta = (top + margin) / (scale * a_min)
    kp_r = kr.clone()
    kp_r[:, :, t0:] = beta * u
    sign = torch.where(torch.rand(B, Hkv, T, 64, generator=g) < 0.5, -1.0, 1.0)
    vp = v.clone()
    vp[:, :, t0:] = (1024.0 * sign[:, :, t0:]).bfloat16()
    kp = k.clone()
    kp[:, :, t0:] = unrot(kp_r)[:, :, t0:].bfloat16()
    return (q, k, v), (q, kp, vp)


# ----------------------------------------------------------------------------------------- norms
def _norm_ref(rms, x, delta, w, b, dy, ds, eps, dtype, wdtype, emulate, mutant, rpb):
    assert mutant is None or mutant in NORM_MUTANTS, mutant
    dtype = dtype or x.dtype
    wdtype = wdtype or (w.dtype if w.dtype != torch.float64 else dtype)
    ct = torch.float32 if emulate else torch.float64  # the kernels compute in fp32 (norm.hip)
    x, w, dy = x.to(ct), w.to(ct), dy.to(ct)
    b = None if (rms or b is None) else b.to(ct)
    ssum = None
    s = x
    if delta is not None:
        s_exact = x + delta.to(ct)
        ssum = _rd(s_exact, dtype)  # ln_fwd_kernel `round_to<T>`: "normalise what was stored"
        s = ssum
    C = s.shape[-1]
    half = C // 2

    def stats(t):
        mean = torch.zeros_like(t[..., :1]) if rms else t.mean(-1, keepdim=True)
        var = ((t - mean) ** 2).mean(-1, keepdim=True)
        return mean, torch.rsqrt(var + (0.0 if mutant == "no_eps" else eps))

    mean, rstd = stats(s)
    if mutant == "y_unrounded_sum" and delta is not None:
        my, ry = stats(s_exact)
        y = (s_exact - my) * ry * w
    else:
        y = (s - mean) * rstd * w
    if b is not None:
        y = y + b
    if mutant == "neighbour_stats":  # the backward reads row r - 1's statistics on odd rows
        idx = torch.arange(s.shape[0], device=s.device)
        idx = idx - (idx % 2)
        mean, rstd = mean[idx], rstd[idx]
    xh = (s - mean) * rstd
    g = dy * w
    gx = g * xh
    m1 = torch.zeros_like(mean) if (rms or mutant == "no_mean_g") else (
        g[..., :half].mean(-1, keepdim=True) if mutant == "half_mean_g" else g.mean(-1, keepdim=True))
    m2 = torch.zeros_like(mean) if mutant == "no_proj" else (
        gx[..., :half].mean(-1, keepdim=True) if mutant == "half_mean_gx" else gx.mean(-1, keepdim=True))
    dx = rstd * (g - m1 - xh * m2)
    if ds is not None and mutant != "no_dres":
        dx = dx + ds.to(ct)
    n = s.shape[0]
    keep = n if mutant != "dw_tail" else (n // rpb) * rpb if n % rpb else n - rpb  # drop the last workgroup
    dw = (dy * xh)[:keep].sum(0)
    db = None if rms else dy[:keep].sum(0)
    if emulate:
        y, dx = _rd(y, dtype), _rd(dx, dtype)
        dw = _rd(dw, wdtype)
        db = None if db is None else _rd(db, wdtype)
    dd = dx if delta is not None else None
    f = lambda t: None if t is None else t.double()  # noqa: E731
    return f(y), f(ssum), f(dx), f(dd), f(dw), f(db)


def ln_ref(x, delta, w, b, dy, ds, eps, *, dtype=None, wdtype=None, emulate=False, mutant=None, rpb=4):
    """LayerNorm of x (+ delta) [rows, C] and its backward for the incoming gradients dy (of y) and
    ds (of the returned sum; None without).  Returns y, sum, dx, ddelta, dw, db in fp64 (sum /
    ddelta None without delta).  ``dtype`` / ``wdtype``: storage dtypes of the activations and of
    the weight gradients (default: the inputs').  ``rpb``: rows per backward workgroup, for the
    ``dw_tail`` mutant only."""
    return _norm_ref(False, x, delta, w, b, dy, ds, eps, dtype, wdtype, emulate, mutant, rpb)


def rms_ref(x, delta, w, b, dy, ds, eps, *, dtype=None, wdtype=None, emulate=False, mutant=None, rpb=4):
    """RMSNorm: as ``ln_ref`` without centring and without a bias (``b`` ignored, db None)."""
    return _norm_ref(True, x, delta, w, None, dy, ds, eps, dtype, wdtype, emulate, mutant, rpb)


_OFFSETS = (0.0, 2.0, -5.0, 40.0, -3.0, 0.5, -48.0, 7.0)


def norm_inputs(rows, C, seed, dtype, eps, rms=False, residual=True):
    """Structured norm inputs, seeded on the CPU; returns a dict of x, delta, w, b, dy, ds in
    ``dtype`` (delta / ds None without ``residual``).
      * row scale σ log-uniform over four decades from sqrt(eps): the smallest rows' variance is
        within 10x of eps (row 0 exactly at the bottom), so eps matters and rstd spans 1e4;
      * per-row offsets of 0 .. 48 σ (several σ: the mean matters; 40+: the rounding of the stored
        residual sum is far larger than that of y); RMSNorm keeps the small rows' offset <= 2 σ;
      * dy = noise + a_r + b_r·x̂ + c_r·ramp(column): both projection terms of dx are large, and
        the ramp gives each half of the columns its own mean (a partial reduction shows)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    u = torch.rand(rows, 1, generator=g)
    u[0] = 0.0
    if rows > 1:
        u[1] = 0.02
    sigma = math.sqrt(eps) * 10.0 ** (4.0 * u)
    off = torch.tensor([_OFFSETS[r % len(_OFFSETS)] for r in range(rows)])[:, None]
    if rms:
        off = torch.where(u < 0.15, off.clamp(-2.0, 2.0), off)
    s = sigma * (torch.randn(rows, C, generator=g) + off)
    w = 1 + 0.2 * torch.randn(C, generator=g)
    b = 0.3 * torch.randn(C, generator=g)
    if residual:
        d = 0.5 * sigma * torch.randn(rows, C, generator=g)
        x, delta = (s - d).to(dtype), d.to(dtype)
        st = (x.double() + delta.double()).to(dtype).double()
    else:
        x, delta = s.to(dtype), None
        st = x.double()
    mean = torch.zeros(rows, 1, dtype=torch.float64) if rms else st.mean(-1, keepdim=True)
    xh = (st - mean) * torch.rsqrt(((st - mean) ** 2).mean(-1, keepdim=True) + eps)
    sgn = lambda: torch.where(torch.rand(rows, 1, generator=g) < 0.5, -1.0, 1.0)  # noqa: E731
    a_r = sgn() * (1 + 2 * torch.rand(rows, 1, generator=g))
    b_r = sgn() * (1 + 2 * torch.rand(rows, 1, generator=g))
    c_r = sgn() * (1 + 2 * torch.rand(rows, 1, generator=g))
    ramp = torch.linspace(-1.0, 1.0, C)[None, :]
    dy = (0.5 * torch.randn(rows, C, generator=g) + a_r + b_r * xh.float() + c_r * ramp).to(dtype)
    ds = torch.randn(rows, C, generator=g).to(dtype) if residual else None
    return {"x": x, "delta": delta, "w": w.to(dtype), "b": b.to(dtype), "dy": dy, "ds": ds}
