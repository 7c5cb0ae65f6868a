"""GPU numerics: every instantiation of the loss kernels (csrc/kernels/xent.hip: ``xent_fwd``,
``xent_bwd`` with and without its vector path, ``xent_fused`` at the edges of its four register
instances) against the fp64 reference of tests/refmath_xent.py, on structured rows: noise scales
over three decades, offsets of many σ, a trend across the columns, -inf bands, and one sentinel
column per row that alone holds a quarter of the row's mass, cycled through every position at
which the kernels' indexing changes.

The logits are a view into a larger buffer with an odd row stride, started at every element
offset of a 16-byte group, so every head length occurs in each run; the padding between the rows
must come back bit-identical.  lse and loss rows are scored by max|Δ|, the gradient per element
(``refmath_xent.elem_rel``).  The bound is never a constant fitted to the kernel: each case computes
``floor = score(emulated reference, fp64 reference)`` on its own inputs, on the device, and
asserts ``score(kernel, fp64 reference) <= 3 x floor`` (fp32 gradient: ``3 x max(floor, derived
floor)``, refmath_xent's docstring).  tests/test_xent_ref.py shows on the CPU that wrong formulas
score >= 9 x floor here.  Run with ``-s`` for every figure and the worst kernel/floor ratio per
output."""
import math

import pytest
import torch

import refmath_xent as rx
from nbdistributed_amd import ops

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
G = 2.5  # grad_out: scale = G / n_valid
WORST = {}


@pytest.fixture(scope="module")
def dev(require_gpu):
    ops.load_library()
    assert ops.native_available(), ops._load_error
    yield torch.device("cuda", 0)
    print("\nworst kernel/floor ratio per output (bound 3):")
    for n, (r, case) in sorted(WORST.items()):
        print(f"  {n:16s} {r:5.2f}  {case}")


def _phases(dtype):
    return range(16 // (torch.finfo(dtype).bits // 8))


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _buffer(dev, N, ld, dtype, seed):
    """A 16-byte aligned buffer of N rows of stride ld plus 16 elements, filled with finite noise."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    buf = (3 * torch.randn(N * ld + 16, generator=g)).to(dtype).to(dev)
    assert buf.data_ptr() % 16 == 0
    return buf


def _view(buf, N, V, ld, off):
    assert 0 <= off and off + (N - 1) * ld + V <= buf.numel()
    return torch.as_strided(buf, (N, V), (ld, 1), off)


def _outside(buf, N, V, ld, off):
    m = torch.ones(buf.numel(), dtype=torch.bool, device=buf.device)
    _view(m, N, V, ld, off).fill_(False)
    return m


def _layout(dev, d, dtype, phase):
    """The logits of ``d`` as a view ``phase`` elements into a padded buffer; the view's rows have
    the heads the partition says."""
    (N, V), ld = d["x"].shape, d["ld"]
    buf = _buffer(dev, N, ld, dtype, seed=V + phase)
    x = _view(buf, N, V, ld, phase)
    x.copy_(d["x"].to(dev))
    esize = buf.element_size()
    for r in (0, 1, N - 1):
        p = x.data_ptr() + r * ld * esize
        assert min(((16 - p % 16) % 16) // esize, V) == int(d["part"][r, 0])
    return buf, x, _outside(buf, N, V, ld, phase)


def _padding_intact(case, buf, before, outside):
    assert torch.equal(_bits(buf)[outside], _bits(before)[outside]), f"{case}: columns outside the view were written"


def _refs(dev, d, dtype, scale):
    x, tgt = d["x"].to(dev), d["target"].to(dev)
    kw = dict(dtype=dtype, part=d["part"])
    exact = rx.xent_ref(x, tgt, scale, rx.IGNORE, **kw)
    emu = rx.xent_ref(x, tgt, scale, rx.IGNORE, emulate=True, **kw)
    derived = rx.derived_floor32(x, exact[1], tgt) if dtype == torch.float32 else 0.0
    return exact, emu, derived


def _note(case, name, err, floor, bad, bound=None):
    bound = floor if bound is None else bound
    ratio = err / bound if bound > 0 else (0.0 if err == 0 else math.inf)
    print(f"  {case} {name}: kernel {err:.3e} floor {floor:.3e}" + (f" bound/3 {bound:.3e}" if bound != floor else "") +
          f" ratio {ratio:.2f}")
    if ratio > WORST.get(name, (-1.0, ""))[0]:
        WORST[name] = (ratio, case)
    if not err <= 3 * bound:
        bad.append((name, err, bound))


def _check_rows(case, key, loss, lse, refs, rows=None):
    """loss rows and lse <= 3 x floor; ``rows``: the rows that count (bool [N])."""
    exact, emu, _ = refs
    bad = []
    for name, got, i in ((f"{key} loss", loss, 0), (f"{key} lse", lse, 1)):
        assert got.dtype == torch.float32 and got.shape == exact[i].shape
        sel = slice(None) if rows is None else rows
        _note(case, name, rx.row_abs(got[sel], exact[i][sel]), rx.row_abs(emu[i][sel], exact[i][sel]), bad)
    assert not bad, (case, bad)


def _check_grad(case, key, dx, refs, dtype, rows=None):
    exact, emu, derived = refs
    assert dx.dtype == dtype and dx.shape == exact[2].shape
    bad = []
    floor = rx.elem_rel(emu[2], exact[2], dtype, rows)
    _note(case, f"{key} dx", rx.elem_rel(dx, exact[2], dtype, rows), floor, bad, max(floor, derived))
    assert not bad, (case, bad)


def _check_exact(case, d, loss, dx, dev, rows=None):
    """What holds to the bit: no gradient on ignored / out-of-range rows and on -inf columns, a zero
    loss on ignored rows, a NaN loss on out-of-range rows (and only there)."""
    tgt = d["target"].to(dev)
    V = d["x"].shape[1]
    ignored = tgt == rx.IGNORE
    oor = ~ignored & ((tgt < 0) | (tgt >= V))
    if dx is not None:
        assert bool((dx[ignored | oor] == 0).all()), f"{case}: gradient on a row without a loss"
        assert bool((dx[d["band"].to(dev)] == 0).all()), f"{case}: gradient on a -inf column"
    if loss is not None:
        assert bool((loss[ignored] == 0).all()), case
        assert bool(torch.isnan(loss[oor]).all()), f"{case}: out-of-range rows must poison the loss"
        keep = ~oor if rows is None else (~oor & rows)
        assert bool(torch.isfinite(loss[keep]).all()), f"{case}: a NaN loss beside an out-of-range row"


def _scale(d):
    return float(torch.tensor(G / d["n_valid"], dtype=torch.float32))


# ----------------------------------------------------------------------- xent_fwd and xent_bwd
@pytest.mark.parametrize("V", [1, 5, 9, 23, 2048 + 5, 4099])
@pytest.mark.parametrize("dt", DT)
def test_fwd_bwd_every_phase_and_dlogits_layout(dev, dt, V):
    """V = 1, 5, 9: all scalar (9 where the head is >= 2); 23: a head, two chunks and a tail;
    2053: chunk 256 wraps to lane 0; 4099: 512 chunks.  dlogits separate at the logits' 16-byte phase
    (xent_bwd_kernel<T, true>), separate one element further (<T, false>), and in place."""
    dtype = DT[dt]
    N = rx.default_rows(V, 0)
    for phase in _phases(dtype):
        d = rx.xent_inputs(N, V, seed=V, dtype=dtype, phase=phase)
        scale = _scale(d)
        refs = _refs(dev, d, dtype, scale)
        buf, x, outside = _layout(dev, d, dtype, phase)
        before = buf.clone()
        tgt = d["target"].to(dev)
        sc = torch.tensor([scale], device=dev)
        case = f"{dt} V={V} phase={phase}"
        loss, lse = torch.ops.nbd.xent_fwd(x, tgt, rx.IGNORE)
        assert torch.equal(_bits(buf), _bits(before)), f"{case}: the forward wrote its input"
        _check_rows(case, "fwd", loss, lse, refs)
        _check_exact(case, d, loss, None, dev)
        for mode, off in (("vec", phase), ("novec", phase + 1)):
            dbuf = _buffer(dev, N, d["ld"], dtype, seed=1000 + V)
            dbefore = dbuf.clone()
            dx = _view(dbuf, N, V, d["ld"], off)
            assert ((dx.data_ptr() - x.data_ptr()) % 16 == 0) == (mode == "vec")
            torch.ops.nbd.xent_bwd(x, tgt, lse, sc, rx.IGNORE, dx)
            _check_grad(f"{case} {mode}", f"bwd {mode}", dx, refs, dtype)
            _check_exact(f"{case} {mode}", d, None, dx, dev)
            _padding_intact(f"{case} {mode}", dbuf, dbefore, _outside(dbuf, N, V, d["ld"], off))
            assert torch.equal(_bits(buf), _bits(before)), f"{case} {mode}: the logits changed"
        torch.ops.nbd.xent_bwd(x, tgt, lse, sc, rx.IGNORE, x)
        _check_grad(f"{case} inplace", "bwd inplace", x, refs, dtype)
        _check_exact(f"{case} inplace", d, None, x, dev)
        _padding_intact(f"{case} inplace", buf, before, outside)


# ----------------------------------------------------------------------------------- xent_fused
FUSED_MAX = 256 * 8 * 32 + 14


def _fused_case(dev, dt, V, phase, ld=None):
    dtype = DT[dt]
    N = rx.default_rows(V, 0)
    d = rx.xent_inputs(N, V, seed=V, dtype=dtype, phase=phase, ld=ld)
    scale = _scale(d)
    refs = _refs(dev, d, dtype, scale)
    buf, x, outside = _layout(dev, d, dtype, phase)
    before = buf.clone()
    case = f"fused {dt} V={V} phase={phase}"
    loss, lse = torch.ops.nbd.xent_fused(x, d["target"].to(dev), rx.IGNORE, torch.tensor([scale], device=dev))
    _check_rows(case, "fused", loss, lse, refs)
    _check_grad(case, "fused", x, refs, dtype)  # the gradient is the logits buffer after the call
    _check_exact(case, d, loss, x, dev)
    _padding_intact(case, buf, before, outside)
    return d


@pytest.mark.parametrize("V", [7, 23, 16384, 16385, 32768, 32769, 51200, 51201, 65536, 65543])
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_fused_every_phase_at_the_instance_edges(dev, dt, V):
    """Both sides of each edge between the 8-, 16-, 25- and 32-chunk instances; 65543 is the
    largest vocabulary whose rows fit at every 16-byte phase (head 0: 8192 chunks and a tail of 7)."""
    for phase in _phases(DT[dt]):
        _fused_case(dev, dt, V, phase)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_fused_documented_maximum(dev, dt):
    """V = 65550 = 7 + 8·8192 + 7 fits the largest instance only where every row has a head of 7:
    a row stride that is a multiple of 8 elements, the view one element into its buffer.  At any
    other phase a row would hold 8193 chunks, one more than the instance reads — the op refuses
    (before this check existed that chunk silently stayed out of the loss and kept its logits).
    One column more never fits."""
    V = FUSED_MAX
    ld = V + 10  # 65560: a multiple of 8, so all rows share one phase
    d = _fused_case(dev, dt, V, 1, ld=ld)
    assert bool((d["part"][:, 0] == 7).all()) and bool((d["part"][:, 1] == 8192).all())
    assert {"edge32_last", "head6", "tail6", "last_col"} <= set(d["kinds"])
    sc = torch.ones(1, device=dev)
    tgt = d["target"].to(dev)
    for phase in (0, 2):
        buf = _buffer(dev, 48, ld, DT[dt], seed=1)
        with pytest.raises(RuntimeError, match="too large"):
            torch.ops.nbd.xent_fused(_view(buf, 48, V, ld, phase), tgt, rx.IGNORE, sc)
    buf = _buffer(dev, 48, rx.row_stride(V), DT[dt], seed=2)  # odd stride: some row has a head below 7
    with pytest.raises(RuntimeError, match="too large"):
        torch.ops.nbd.xent_fused(_view(buf, 48, V, rx.row_stride(V), 1), tgt, rx.IGNORE, sc)
    buf = _buffer(dev, 48, ld, DT[dt], seed=3)
    with pytest.raises(RuntimeError, match="too large"):
        torch.ops.nbd.xent_fused(_view(buf, 48, V + 1, ld, 1), tgt, rx.IGNORE, sc)


# -------------------------------------------------------------------------------- public routes
def _public_inputs(dev, dtype, V):
    """Contiguous, aligned rows (V a multiple of 8: every head 0); out-of-range targets become
    ignored ones (the public ops follow F.cross_entropy, which rejects them)."""
    N = rx.default_rows(V, 0)
    d = rx.xent_inputs(N, V, seed=V, dtype=dtype, phase=0, ld=V)
    tgt = d["target"].clone()
    tgt[(tgt != rx.IGNORE) & ((tgt < 0) | (tgt >= V))] = rx.IGNORE
    d = dict(d, target=tgt, n_valid=int((tgt != rx.IGNORE).sum()))
    assert d["n_valid"] >= 3 * N // 4 - 1
    return d


def _check_total(case, name, loss, refs, n_valid, reduction):
    """The reduced loss: every row within 3 x floor, so the mean is too (the sum: n_valid times that),
    plus a handful of fp32 roundings of the total."""
    exact, emu, _ = refs
    ref = float(exact[0].sum()) / (n_valid if reduction == "mean" else 1)
    floor = rx.row_abs(emu[0], exact[0]) * (1 if reduction == "mean" else n_valid) + 2.0 ** -22 * abs(ref)
    bad = []
    _note(case, name, abs(float(loss) - ref), floor, bad)
    assert not bad, (case, bad)


@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("reduction", ["mean", "sum"])
@pytest.mark.parametrize("dt", DT)
def test_public_cross_entropy(dev, dt, reduction, inplace):
    dtype, V = DT[dt], 2056
    d = _public_inputs(dev, dtype, V)
    scale = float(torch.tensor(G / (d["n_valid"] if reduction == "mean" else 1), dtype=torch.float32))
    refs = _refs(dev, d, dtype, scale)
    x = d["x"].to(dev).requires_grad_(True)
    y = x * 1.0 if inplace else x  # in-place backward needs a non-leaf (it overwrites the storage)
    loss = ops.cross_entropy(y, d["target"].to(dev), reduction=reduction, inplace_backward=inplace)
    (loss * G).backward()
    case = f"cross_entropy {dt} {reduction} inplace={inplace}"
    _check_total(case, "public loss", loss.detach(), refs, d["n_valid"], reduction)
    _check_grad(case, "public dx", x.grad, refs, dtype)
    _check_exact(case, d, None, x.grad, dev)


@pytest.mark.parametrize("reduction", ["mean", "sum"])
def test_public_linear_cross_entropy(dev, reduction, monkeypatch):
    """The autograd glue of the fused head around ``xent_fused``: the logits are taken as the op's
    own product left them (a spy on ``torch.mm``), the gradient from the buffer the op saved for
    its backward.  The GEMMs themselves belong to test_gpu_gemm_paths.py."""
    from nbdistributed_amd.ops import loss as L

    monkeypatch.setattr(L, "LM_HEAD_HIP", False)
    monkeypatch.setattr(L, "LM_HEAD_CHUNK", 0)
    seen = []
    real_mm = torch.mm

    def spy(*a, **k):
        out = real_mm(*a, **k)
        seen.append(out.clone())
        return out

    monkeypatch.setattr(torch, "mm", spy)
    N, V, C = 48, 2056, 64
    g = torch.Generator(device="cpu").manual_seed(11)
    h = (torch.randn(N, C, generator=g) * torch.logspace(-1.5, 0, N)[:, None]).bfloat16().to(dev).requires_grad_()
    w = torch.randn(V, C, generator=g).bfloat16().to(dev)
    tgt = torch.randint(0, V, (N,), generator=g)
    tgt[::6] = rx.IGNORE
    loss = ops.linear_cross_entropy(h, w, tgt.to(dev), reduction=reduction)
    assert len(seen) == 1 and seen[0].shape == (N, V)
    n_valid = int((tgt != rx.IGNORE).sum())
    scale = float(torch.tensor(1.0 / n_valid if reduction == "mean" else 1.0, dtype=torch.float32))
    d = {"x": seen[0], "target": tgt, "part": rx.partition(N, V, V, 0, 2), "band": torch.zeros(N, V, dtype=torch.bool)}
    refs = _refs(dev, d, torch.bfloat16, scale)
    dlogits = loss.grad_fn.saved_tensors[2]
    assert dlogits.shape == (N, V)
    case = f"linear_cross_entropy {reduction}"
    _check_total(case, "public loss", loss.detach(), refs, n_valid, reduction)
    _check_grad(case, "public dx", dlogits, refs, torch.bfloat16)
    _check_exact(case, d, None, dlogits, dev)


# ------------------------------------------------------------------------ non-finite propagation
def _poison(d, V):
    """Rows of ``d`` that are finite except for one NaN — in the head, as one lane of a chunk, as a
    whole chunk, in the tail, in an all-scalar row — or that hold a +inf; each such row gets a
    valid target on a clean column.  Returns the logits, the targets and {row: what}."""
    x, tgt, part = d["x"].clone(), d["target"].clone(), d["part"]
    N = x.shape[0]
    free = [r for r in range(N) if not bool(d["band"][r].any())]
    what = {}

    def take(ok):
        r = next(r for r in free if ok(*(int(v) for v in part[r])))
        free.remove(r)
        return r, tuple(int(v) for v in part[r])

    plan = []
    if V >= 23:
        plan = [("nan head", lambda h, nv, t0: h > 0 and nv > 0, lambda h, nv, t0: [h - 1]),
                ("nan head0", lambda h, nv, t0: h > 1 and nv > 0, lambda h, nv, t0: [0]),
                ("nan lane", lambda h, nv, t0: nv > 0, lambda h, nv, t0: [h + 8 * min(nv - 1, 256) + 2]),
                ("nan chunk", lambda h, nv, t0: nv > 1, lambda h, nv, t0: list(range(h + 8 * (nv - 1), h + 8 * nv))),
                ("nan chunk0", lambda h, nv, t0: nv > 1, lambda h, nv, t0: list(range(h, h + 8))),
                ("nan tail", lambda h, nv, t0: nv > 0 and t0 < V, lambda h, nv, t0: [V - 1]),
                ("+inf chunk", lambda h, nv, t0: nv > 0, lambda h, nv, t0: [h + 5]),
                ("+inf tail", lambda h, nv, t0: nv > 0 and t0 < V, lambda h, nv, t0: [t0])]
    else:
        plan = [("nan scalar", lambda h, nv, t0: nv == 0, lambda h, nv, t0: [V // 2]),
                ("nan scalar first", lambda h, nv, t0: nv == 0 and h > 0, lambda h, nv, t0: [0]),
                ("nan scalar last", lambda h, nv, t0: nv == 0 and t0 < V, lambda h, nv, t0: [V - 1]),
                ("+inf scalar", lambda h, nv, t0: nv == 0, lambda h, nv, t0: [1])]
    for name, ok, cols in plan:
        r, p = take(ok)
        c = cols(*p)
        x[r, c] = math.inf if name.startswith("+inf") else math.nan
        tgt[r] = next(j for j in range(V) if j not in c)
        what[r] = name
    return x, tgt, what


@pytest.mark.parametrize("V", [5, 23, 2053])
@pytest.mark.parametrize("kernel,dt", [("fwd", "bf16"), ("fwd", "f16"), ("fwd", "f32"), ("fused", "bf16"), ("fused", "f16")])
def test_non_finite_logits_reach_the_loss(dev, kernel, dt, V):
    """A NaN or +inf anywhere in a row gives that row a non-finite lse and loss, as
    ``F.cross_entropy`` does — the training loops watch the loss for divergence — and every other
    row stays finite and within its bound.  (Before OnlineLse carried a NaN into its sum whatever
    the running maximum, a NaN met by a fresh accumulator was dropped: the head lanes, a whole
    chunk, an all-scalar row, and the fused kernel's tail lanes.)"""
    dtype = DT[dt]
    N = rx.default_rows(V, 0)
    phase = 3 if dtype != torch.float32 else 1
    d = rx.xent_inputs(N, V, seed=V + 1, dtype=dtype, phase=phase)
    xp, tgt, what = _poison(d, V)
    clean = torch.ones(N, dtype=torch.bool)
    clean[list(what)] = False
    dc = dict(d, target=tgt)
    scale = _scale(d)
    refs = _refs(dev, dc, dtype, scale)  # of the clean logits: rows are independent
    buf, x, _ = _layout(dev, dict(d, x=xp), dtype, phase)
    case = f"nonfinite {kernel} {dt} V={V}"
    if kernel == "fwd":
        loss, lse = torch.ops.nbd.xent_fwd(x, tgt.to(dev), rx.IGNORE)
    else:
        loss, lse = torch.ops.nbd.xent_fused(x, tgt.to(dev), rx.IGNORE, torch.tensor([scale], device=dev))
    lost = [(r, n, float(lse[r]), float(loss[r])) for r, n in what.items()
            if math.isfinite(float(lse[r])) or math.isfinite(float(loss[r]))]
    print(f"  {case}: " + ", ".join(f"{n}: lse {float(lse[r]):.4g} loss {float(loss[r]):.4g}" for r, n in what.items()))
    rows = clean.to(dev)
    _check_rows(case, f"{kernel} clean", loss, lse, refs, rows)
    _check_exact(case, dc, loss, None, dev, rows)
    if kernel == "fused":
        _check_grad(case, "fused clean", x, refs, dtype, rows)
    assert not lost, f"{case}: finite lse / loss on a row with a non-finite logit: {lost}"
