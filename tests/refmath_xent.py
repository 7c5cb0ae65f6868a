"""Plain-PyTorch reference for the loss kernels of csrc/kernels/xent.hip (``xent_fwd``,
``xent_bwd``, ``xent_fused``): hand-written fp64 formulas (no autograd), an emulation of the
kernels' rounding points, deliberately wrong "mutant" variants, structured logits and the error
metric.  Conventions as in tests/refmath.py; never touches ``torch.ops.nbd``.

The metric
  * lse and loss rows: ``max|Δ|`` over the rows whose reference is finite (``row_abs``), as
    ``refmath.max_abs`` scores the attention lse.
  * the gradient, **per element**: ``max_i |dx_i − ref_i| / max(|ref_i|, tiny)`` (``elem_rel``),
    ``tiny`` = the smallest normal of the storage dtype (so fp16 subnormals, whose spacing is
    2⁻¹⁰·tiny, do not define the score).  Why not a per-row or per-tensor normaliser: the
    gradient's maximum sits at the target (≈ scale) and almost every other entry is thousands of
    times smaller, so a softmax part that is wrong by tens of percent — or zero — at most columns,
    a one-hot one column off, or a row short of one chunk all stay below a bf16 bound relative to
    the row's or the tensor's maximum.  Only an element's own magnitude shows them.

The emulation's rounding points (``emulate=True``; each names its line in xent.hip)
  1. the logits are read in the storage dtype (``Elem<T>::load`` / ``load8`` / ``unpack8``);
  2. ``t = fl32(x · kLog2e)``, kLog2e the fp32 constant (``OnlineLse::add8``: ``t[j] = v[j] * kLog2e``,
     and the ``* kLog2e`` at every ``acc.add`` call);
  3. the running sum is fp32 (``OnlineLse::s``) — emulated as the fp64 sum of ``exp2(t − max t)``
     rounded once: the order of the kernel's partial sums is not a rounding *point*;
  4. ``lse = fl32(fl32(m + fl32(log2 s)) · kLn2)`` (``const float lse = (tot.m + log2f(tot.s)) * kLn2``);
  5. ``loss = fl32(lse − x[t])`` (``l = lse - Elem<T>::load(x, t)``);
  6. ``l2 = fl32(lse · kLog2e)`` (``const float l2 = lse[row] * kLog2e``);
  7. ``e = fl32(x · kLog2e − l2)`` in ONE rounding, ``p = fl32(exp2(e))``, ``g = fl32(p · sc)`` and,
     at the target, ``g = fl32(p · sc − sc)`` (``__builtin_amdgcn_exp2f(v[j] * kLog2e - l2) * sc``,
     ``if (i == t) g -= sc``).  The build contracts products into sums (HIP's default
     ``-ffp-contract=fast``): every backward exponent of xent_bwd_kernel and xent_fused_kernel is
     one ``v_fma_f32`` in the gfx950 code, and so is the scalar columns' one-hot.  With two
     roundings the emulation would differ from a correct kernel by half an ulp of t, which at
     V = 1 — where p = 1 and the reference gradient is an exact 0 — is the whole result.  (A
     chunk's ``v[j] -= sc`` is a subtraction of its own: that differs from the fused form by
     2⁻²⁴·p·sc beside (1 − p)·sc with p ≤ 3/4, far below every bound here.);
  8. g rounded to the storage dtype (``Elem<T>::store`` / ``store8`` / ``store8_nt``).

The derived fp32 floor (``derived_floor32``).  For fp32 logits the emulation's own error is fp32
arithmetic itself, and a correct kernel need not repeat it bit for bit (it may contract
``x·kLog2e − l2`` into one FMA, sums in another order, and uses the hardware ``exp2``).  What any
fp32 evaluation of ``exp2(t − l2)·sc`` may show, relative to an element:
  * the exponent ``e = t − l2`` carries three fp32 roundings (of t, of l2, of the difference), each
    at most ``2⁻²⁴·max(|t|, |l2|)`` absolute; an absolute error δ in a base-2 exponent is a relative
    error ``δ·ln2`` of the power: ``3·max(|t|, |l2|)·2⁻²⁴·ln2``;
  * ``v_exp_f32`` is documented accurate to 1 ulp: ``2⁻²³`` relative; the product with sc adds
    ``2⁻²⁴``;
  * at the target the one-hot subtraction ``(p − 1)·sc`` amplifies p's relative error by
    ``p / (1 − p)`` — the inputs keep p ≤ 3/4 there, and the factor is taken from the reference.
The fp32 bound is ``3 × max(floor, derived floor)``; nothing in it is fitted to the kernel.

The inputs keep every finite logit within 80 nats of its row's lse (asserted): a probability
below 2⁻¹²⁶ ≈ e⁻⁸⁷ is a subnormal that the raw ``v_exp_f32`` may return as 0, which is not an
error of the kernel's formula and must not reach the score.
"""
import math

import torch

LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453
LOG2E_F = float(torch.tensor(LOG2E, dtype=torch.float32))  # kLog2e as the kernel holds it
LN2_F = float(torch.tensor(LN2, dtype=torch.float32))      # kLn2
LANES = 256                                                # kXentThreads
FUSED_INSTANCES = (8, 16, 25, 32)                          # xent_fused_kernel<T, NV>

IGNORE = -100
XENT_OUT = ("loss", "lse", "dx")
XENT_MUTANTS = ("drop_head", "drop_tail", "drop_chunk", "merge_no_rescale", "onehot_shift", "onehot_missing_scalar",
                "ignored_row_scaled", "neighbour_target", "ln_for_log2", "scale_twice", "grad_unscaled_onehot")
TARGET_CLASSES = ("sentinel", "head", "tail", "d0", "d7", "ignore", "oor")
_TARGET_CYCLE = ("sentinel", "head", "tail", "d0", "d7", "ignore", "sentinel", "tail", "oor")  # 2 of 9 without a loss
_OFFSETS = (0.0, 2.0, -5.0, 40.0, -3.0, 0.5, -48.0, 7.0)  # in units of the row's σ (refmath._OFFSETS)
_SIGMAS = (1.0, 0.01, 10.0, 0.1, 3.0, 0.03, 0.3)            # three decades; 7 and 8 are coprime


def _f32(x):
    return x.to(torch.float32).to(x.dtype)


def _rd(x, dt):
    return x.to(dt).to(x.dtype)


# ------------------------------------------------------------------------------------ the metric
def row_abs(x, ref):
    """max|x − ref| over the rows whose reference is finite (lse, loss rows)."""
    x, ref = x.detach().double(), ref.detach().double()
    assert x.shape == ref.shape, (x.shape, ref.shape)
    ok = torch.isfinite(ref)
    if not bool(ok.any()):
        return 0.0
    d = (x[ok] - ref[ok]).abs()
    return math.inf if bool(torch.isnan(d).any()) else float(d.max())


def elem_rel(dx, ref, dtype, rows=None):
    """max_i |dx_i − ref_i| / max(|ref_i|, tiny(dtype)): see the module docstring.  ``rows``: a
    bool mask [N] of the rows that count."""
    dx, ref = dx.detach().double(), ref.detach().double()
    assert dx.shape == ref.shape, (dx.shape, ref.shape)
    if rows is not None:
        dx, ref = dx[rows], ref[rows]
    r = (dx - ref).abs() / ref.abs().clamp_min(torch.finfo(dtype).tiny)
    return math.inf if bool(torch.isnan(r).any()) else float(r.max())


def derived_floor32(x, lse, target, ignore_index=IGNORE):
    """The fp32 gradient floor derived in the module docstring, from the fp64 reference's own
    exponents and target probabilities."""
    xd = x.double()
    fin = torch.isfinite(xd)
    tmax = float((xd.abs() * fin).nan_to_num(0.0).max()) * LOG2E
    tmax = max(tmax, float(lse.double().abs().max()) * LOG2E)
    V = x.shape[1]
    valid = (target != ignore_index) & (target >= 0) & (target < V)
    amp = 1.0
    if bool(valid.any()):
        p = torch.exp(xd[valid].gather(1, target[valid][:, None]).squeeze(1) - lse.double()[valid])
        p = p[p < 1.0]  # p = 1 (V = 1): the reference is an exact 0, and the emulated floor alone speaks
        if p.numel():
            amp = max(1.0, float((p / (1 - p)).max()))
    return (3.0 * tmax * 2.0 ** -24 * LN2 + 2.0 ** -23) * amp + 2.0 ** -24


# --------------------------------------------------------------------------------- the partition
def row_stride(V):
    """An odd row stride with at least 9 columns of padding between rows."""
    return V + 9 if V % 2 == 0 else V + 10


def partition(N, V, ld, phase, esize):
    """(head, nv, tail0) per row, int64 [N, 3], of a view that starts ``phase`` elements into a
    16-byte aligned buffer with row stride ``ld``: ``head`` scalar columns up to the first 16-byte
    boundary, ``nv`` chunks of 8 columns, then the scalar tail from column ``tail0`` (xent.hip
    ``head_elems``, ``nv = (V - head) / 8``)."""
    r = torch.arange(N, dtype=torch.int64)
    byte = (phase + r * ld) * esize
    head = (((16 - byte % 16) % 16) // esize).clamp_max(V)
    nv = (V - head) // 8
    return torch.stack([head, nv, head + nv * 8], 1)


def lanes(part, V):
    """The lane (0 .. 255) that accumulates each column in xent_fwd_kernel, int64 [N, V]: head
    column j on lane j, chunk k on lane k mod 256, tail column tail0 + j on lane j."""
    part = part.to(torch.int64)
    col = torch.arange(V, dtype=torch.int64, device=part.device)[None, :]
    head, tail0 = part[:, 0:1], part[:, 2:3]
    return torch.where(col < head, col, torch.where(col < tail0, ((col - head) // 8) % LANES, (col - tail0) % LANES))


# --------------------------------------------------------------------------------- the reference
def _lse(t, emulate):
    """logsumexp of base-2 scaled rows t [N, V] in log2 units: (m, s)."""
    m = t.amax(-1, keepdim=True)
    s = torch.exp2(t - m).sum(-1, keepdim=True)
    return m, (_f32(s) if emulate else s)


def xent_ref(x, target, scale, ignore_index, *, dtype, emulate=False, mutant=None, part=None):
    """Cross-entropy rows of the logits ``x`` [N, V] as stored and their gradient for
    ``scale`` = grad_out / n_valid: returns ``(loss_rows, lse, dx)`` in fp64.  Rows with
    ``target == ignore_index`` have loss 0, rows with a target outside [0, V) loss NaN; both have
    dx = 0.  ``part`` [N, 3] (``partition``) is the kernels' column layout, which the layout
    mutants need; they mirror it without importing anything."""
    assert mutant is None or mutant in XENT_MUTANTS, mutant
    N, V = x.shape
    dev = x.device
    xd = x.double()
    if emulate:
        xd = _rd(xd, dtype)
    f = _f32 if emulate else (lambda v: v)
    k2, kln = (LOG2E_F, LN2_F) if emulate else (LOG2E, LN2)
    target = target.to(dev)
    col = torch.arange(V, device=dev)[None, :]
    if part is not None:
        part = part.to(dev)
        head, nv, tail0 = part[:, 0:1], part[:, 1:2], part[:, 2:3]
    else:
        assert mutant in (None, "ignored_row_scaled", "neighbour_target", "ln_for_log2", "scale_twice",
                          "grad_unscaled_onehot"), "layout mutants need the partition"
    t = f(xd * k2)
    ts = t
    if mutant == "drop_head":
        ts = t.masked_fill(col < head, -math.inf)
    elif mutant == "drop_tail":
        ts = t.masked_fill(col >= tail0, -math.inf)
    elif mutant == "drop_chunk":  # the last chunk of the row: chunk NV·256 − 1 of a full instance
        ts = t.masked_fill((col >= tail0 - 8) & (col < tail0) & (nv > 0), -math.inf)
    if mutant == "merge_no_rescale":
        ln = lanes(part, V)
        ml = torch.full((N, LANES), -math.inf, dtype=torch.float64, device=dev).scatter_reduce(1, ln, t, "amax")
        e = torch.exp2(t - ml.gather(1, ln)).nan_to_num(0.0)  # (-inf) − (-inf): nothing added
        m, s = ml.amax(-1, keepdim=True), f(e.sum(-1, keepdim=True))
    else:
        m, s = _lse(ts, emulate)
    lg = f(m + f(torch.log2(s)))
    lse = lg if mutant == "ln_for_log2" else f(lg * kln)
    tg = target
    if mutant == "neighbour_target":
        tg = torch.roll(target, -1)
    ignored = tg == ignore_index
    valid = ~ignored & (tg >= 0) & (tg < V)
    tc = tg.clamp(0, V - 1)[:, None]
    xt = xd.gather(1, tc)
    loss = torch.where(valid[:, None], f(lse - xt), torch.full_like(lse, math.nan))
    loss = torch.where(ignored[:, None], torch.zeros_like(loss), loss)
    sc = float(torch.tensor(scale, dtype=torch.float32)) if emulate else float(scale)
    l2 = f(lse * k2)
    p = f(torch.exp2(f(xd * k2 - l2)))  # (the product of two fp32 values is exact in fp64)
    g = f(p * sc)
    if mutant == "scale_twice":
        g = f(g * sc)
    hot = col == tc
    if mutant == "onehot_shift":  # d -> d + 1 inside the target's chunk
        inchunk = (tc >= head) & (tc < tail0)
        d = (tc - head) % 8
        hot = col == torch.where(inchunk, tc - d + (d + 1) % 8, tc)
    elif mutant == "onehot_missing_scalar":
        hot = hot & (tc >= head) & (tc < tail0)
    g = torch.where(hot, f((g if mutant == "scale_twice" else p * sc) - (1.0 if mutant == "grad_unscaled_onehot" else sc)), g)
    keep = valid | ignored if mutant == "ignored_row_scaled" else valid
    dx = torch.where(keep[:, None], g, torch.zeros_like(g))
    if mutant == "ignored_row_scaled":
        dx = torch.where(ignored[:, None], f(p * sc), dx)
    if emulate:
        dx = _rd(dx, dtype)
    return loss.squeeze(1), lse.squeeze(1), dx


# ------------------------------------------------------------------------------------ the inputs
def sentinel_kinds(esize):
    """The column positions at which the kernels' indexing changes, by name."""
    per = 16 // esize
    k = [f"head{j}" for j in range(per - 1)] + ["chunk0_first", "chunk0_last"]
    for nvi in FUSED_INSTANCES:  # chunk NV·256 − 1 (lane 255, chunk index NV − 1) and the next (none past 32)
        k += [f"edge{nvi}_last"] + ([f"edge{nvi}_past"] if nvi != FUSED_INSTANCES[-1] else [])
    return k + ["last_chunk"] + [f"tail{j}" for j in range(7)] + ["last_col"]


def _kind_col(kind, head, nv, tail0, V):
    """The column of a sentinel kind in a row with this partition, or None where it does not exist."""
    if kind.startswith("head"):
        j = int(kind[4:])
        return j if j < head else None
    if kind.startswith("tail"):
        j = int(kind[4:])
        return tail0 + j if tail0 + j < V else None
    if kind == "last_col":
        return V - 1
    if nv == 0:
        return None
    if kind == "chunk0_first":
        return head
    if kind == "chunk0_last":
        return head + 7
    if kind == "last_chunk":
        return tail0 - 8 + 3
    nvi, side = kind[4:].split("_")
    k = int(nvi) * LANES - (1 if side == "last" else 0)
    return head + 8 * k + (7 if side == "last" else 0) if k < nv else None


def _next_up(v, dtype):
    """The next value of ``dtype`` above the Python float v."""
    t = torch.tensor(v, dtype=dtype)
    if dtype == torch.float32:
        return float(torch.nextafter(t, torch.tensor(math.inf)))
    b = int(t.view(torch.int16))
    b = b + 1 if v > 0 else (b - 1 if v < 0 else 1)  # sign-magnitude: towards +inf
    if v < 0 and (b & 0x7FFF) == 0:
        b = 0
    return float(torch.tensor(b, dtype=torch.int16).view(dtype))


_NOISE = {}


def _noise(N, V, seed):
    key = (N, V, seed)
    if key not in _NOISE:
        if len(_NOISE) >= 2:
            _NOISE.clear()
        g = torch.Generator(device="cpu").manual_seed(seed)
        _NOISE[key] = torch.randn(N, V, generator=g).clamp_(-2.5, 2.5)
    return _NOISE[key]


def default_rows(V, esize):
    """Rows of a case: enough for every sentinel position and target class that can exist at V."""
    return 48 if V >= 23 else 32


def xent_inputs(N, V, seed, dtype, phase, ld=None):
    """Structured logits [N, V] in ``dtype`` (contiguous; the caller copies them into its strided
    view), seeded on the CPU.  Returns a dict: ``x``, ``target`` (int64), ``ignore_index``, ``ld``
    (the row stride the partition assumes: ``row_stride(V)``, odd, unless given), ``part`` [N, 3] = (head, nv, tail0) per row for a
    view starting ``phase`` elements into a 16-byte aligned buffer, ``sentinel`` [N] columns,
    ``kinds`` / ``classes`` (the sentinel position and target class of each row, by name),
    ``band`` [N, V] bool (the -inf columns) and ``n_valid``.
      * row noise σ over three decades (0.01 .. 10), noise clamped at 2.5 σ; row offsets of up to
        48 σ (at most 60 in absolute terms); a triangular trend across columns of 3 units per 2048 columns (up for 4 x 2048
        columns, then down), so lanes, waves and chunk indices hold different running maxima and
        both branches of ``add`` / ``add8`` are taken;
      * every other row that can host it has a band of -inf columns: the last head element, the
        whole first chunk and three columns of the second;
      * one sentinel per row, raised to the smallest stored value at which it alone holds at least
        a quarter of the row's softmax mass, at a position of ``sentinel_kinds`` — rarest first, so
        that every position that exists in some row of this partition is used;
      * targets cycle through the sentinel, a head column, a tail column, lanes d = 0 and d = 7 of
        a chunk, ``ignore_index`` and an out-of-range value (V and -1 in turn); a class that does
        not exist in a row (no head, no tail, no chunk) falls back to the sentinel."""
    esize = torch.finfo(dtype).bits // 8
    ld = row_stride(V) if ld is None else ld
    part = partition(N, V, ld, phase, esize)
    sig = torch.tensor([_SIGMAS[r % len(_SIGMAS)] for r in range(N)], dtype=torch.float64)[:, None]
    off = torch.tensor([_OFFSETS[r % len(_OFFSETS)] for r in range(N)], dtype=torch.float64)[:, None]
    c = torch.arange(V, dtype=torch.float64)[None, :]
    period = 8 * 2048.0
    tri = 3.0 / 2048.0 * (period / 2 - ((c + 577.0 * torch.arange(N)[:, None]) % period - period / 2).abs())
    # offsets of up to 48 σ, held within ±60: the fp32 lse then has several rows in its top binade
    # (32 .. 64), so the floor's maximum over rows is a statistic of a handful of roundings — with
    # one row at 480 alone it is that row's coin flip, and a correct kernel whose sum differs in the
    # last bit can land on the other side of it
    x = (sig * _noise(N, V, seed).double() + (sig * off).clamp(-60.0, 60.0) + tri).to(dtype)

    # sentinel positions: rarest kind first, each to the first free row that has it
    kinds = sentinel_kinds(esize)
    P = [tuple(int(v) for v in part[r]) for r in range(N)]
    cols = {k: [_kind_col(k, *P[r], V) for r in range(N)] for k in kinds}
    order = sorted((k for k in kinds if any(v is not None for v in cols[k])),
                   key=lambda k: sum(v is not None for v in cols[k]))
    row_kind = [None] * N
    for k in order:
        r = next((r for r in range(N) if row_kind[r] is None and cols[k][r] is not None), None)
        if r is not None:
            row_kind[r] = k
    for r in range(N):
        if row_kind[r] is None:
            feas = [k for k in order if cols[k][r] is not None]
            row_kind[r] = feas[r % len(feas)]
    sent = torch.tensor([cols[row_kind[r]][r] for r in range(N)], dtype=torch.int64)

    # targets
    target = torch.empty(N, dtype=torch.int64)
    classes = []
    n_oor = 0
    for r in range(N):
        head, nv, tail0 = P[r]
        cl = _TARGET_CYCLE[r % len(_TARGET_CYCLE)]
        kc = (r // len(_TARGET_CYCLE)) % max(nv, 1)  # the chunk of a d0 / d7 target
        if cl == "head" and head > 0:
            t = r % head
        elif cl == "tail" and tail0 < V:
            t = tail0 + r % (V - tail0)
        elif cl in ("d0", "d7") and nv > 0:
            t = head + 8 * kc + (0 if cl == "d0" else 7)
        elif cl == "ignore":
            t = IGNORE
        elif cl == "oor":
            t = V if n_oor % 2 == 0 else -1
            n_oor += 1
        else:
            cl, t = "sentinel", int(sent[r])
        classes.append(cl)
        target[r] = t

    # the -inf band, where neither the sentinel nor the target falls into it
    band = torch.zeros(N, V, dtype=torch.bool)
    for r in range(0, N, 2):
        head, nv, tail0 = P[r]
        lo, hi = head - 1, head + 11
        if head > 0 and nv >= 2 and not (lo <= int(sent[r]) < hi) and not (lo <= int(target[r]) < hi):
            band[r, lo:hi] = True
    x = x.masked_fill(band, -math.inf)

    # raise the sentinels
    xd = x.double()
    for r in range(N):
        if V == 1:
            continue  # the only column holds all the mass
        s = int(sent[r])
        lo = float(torch.logsumexp(torch.cat([xd[r, :s], xd[r, s + 1:]]), 0))
        if lo == -math.inf:
            continue  # every other column is masked
        v = float(torch.tensor(lo + math.log(1.0 / 3.0), dtype=torch.float64).to(dtype))
        while 1.0 / (1.0 + math.exp(lo - v)) < 0.25:
            v = _next_up(v, dtype)
        x[r, s] = v
    lse = torch.logsumexp(x.double(), -1, keepdim=True)
    gap = (x.double() - lse)[torch.isfinite(x)]
    assert float(gap.min()) >= -80.0, float(gap.min())  # no probability near the fp32 subnormals
    n_valid = int(((target != IGNORE) & (target >= 0) & (target < V)).sum())
    return {"x": x.contiguous(), "target": target, "ignore_index": IGNORE, "ld": ld, "part": part, "sentinel": sent,
            "kinds": row_kind, "classes": classes, "band": band, "n_valid": n_valid}


def feasible_kinds(part, V, esize):
    """The sentinel kinds that exist in at least one row of this partition."""
    P = [tuple(int(v) for v in row) for row in part]
    return [k for k in sentinel_kinds(esize) if any(_kind_col(k, *p, V) is not None for p in P)]
