"""GPU numerics: every instantiation of the HIP LayerNorm / RMSNorm kernels (csrc/kernels/norm.hip)
against the fp64 reference of tests/refmath.py, row by row (dx scales with each row's own rstd)
on structured inputs: row scales over four decades down to variance ~ eps, offsets of many σ,
and a dy whose projections on 1 and x̂ are large and whose column halves have different means.

The bound is never a constant fitted to the kernel: each test computes
``floor = tile_rel(emulated reference, fp64 reference, rows=1)`` on its own inputs and asserts
``tile_rel(kernel, fp64 reference, rows=1) <= 3 x floor`` for y, sum, dx, ddelta, dw and db.
tests/test_refmath_mutants.py shows on the CPU that wrong formulas score >= 9 x floor here.

Row counts and ``bwd_rows_per_block`` (norm.hip): 5 and 333 rows -> 4 rows per workgroup
(ln_bwd_kernel with kRpi = 1, one row per wave; last workgroup 1 row), 4093 = 511·8 + 5 -> 8 rows
per workgroup and 8191 = 511·16 + 15 -> 16 (kRpi = 2, two rows in flight, 1 / 2 sweeps per wave;
ln_bwd16_kernel with 1 / 2 iterations per wave), each with a partial last workgroup.
C: 8 (one 8-B chunk on two lanes), 576 and 1000 (8-B kernels, NCH 3 / 4, a ragged last chunk),
768, 1536, 2048 (C = 256·k: the 16-B half-wave kernels for 2-byte types, NCH 3 / 6 / 8).
Run with ``-s`` for every figure and the worst kernel/floor ratio per output."""
import math

import pytest
import torch

import refmath as rm
from nbdistributed_amd import ops

pytestmark = pytest.mark.gpu

NAMES = ("y", "sum", "dx", "ddelta", "dw", "db")
WORST = {}
BF, HF, F32 = torch.bfloat16, torch.float16, torch.float32


@pytest.fixture(scope="module")
def dev(require_gpu):
    assert ops.native_available(), ops._load_error
    yield torch.device("cuda", 0)
    print("\nworst kernel/floor ratio per output (bound 3):")
    for n, (r, case) in WORST.items():
        print(f"  {n:6s} {r:5.2f}  {case}")


def _compare(case, got, exact, emu):
    bad = []
    for n, x, r, e in zip(NAMES, got, exact, emu):
        if r is None:
            assert x is None, n
            continue
        err, floor = rm.tile_rel(x, r, 1), rm.tile_rel(e, r, 1)
        ratio = err / floor if floor > 0 else (0.0 if err == 0 else math.inf)
        print(f"  {case} {n}: kernel {err:.3e} floor {floor:.3e} ratio {ratio:.2f}")
        if ratio > WORST.get(n, (-1.0, ""))[0]:
            WORST[n] = (ratio, case)
        if not err <= 3 * floor:
            bad.append((n, err, floor))
    assert not bad, (case, bad)


def _eps(kind):
    return 1e-6 if kind == "rms" else 1e-5


def _inputs(dev, kind, rows, C, dt, res):
    d = rm.norm_inputs(rows, C, seed=rows * 7 + C, dtype=dt, eps=_eps(kind), rms=kind == "rms", residual=res)
    return {n: (None if t is None else t.to(dev)) for n, t in d.items()}


def _run(kind, d, res):
    """through the public ops; returns y, sum, dx, ddelta, dw, db (None where the op has none)."""
    eps = _eps(kind)
    x, w = d["x"].clone().requires_grad_(), d["w"].clone().requires_grad_()
    b = d["b"].clone().requires_grad_() if kind == "ln" else None
    delta = d["delta"].clone().requires_grad_() if res else None
    if res:
        s, y = (ops.add_layer_norm(x, delta, w, b, eps) if kind == "ln" else ops.add_rms_norm(x, delta, w, eps))
        torch.autograd.backward([s, y], [d["ds"], d["dy"]])
    else:
        s = None
        y = ops.layer_norm(x, w, b, eps) if kind == "ln" else ops.rms_norm(x, w, eps)
        y.backward(d["dy"])
    torch.cuda.synchronize()
    return y, s, x.grad, (delta.grad if res else None), w.grad, (b.grad if b is not None else None)


def _refs(kind, d, dt):
    fn = rm.ln_ref if kind == "ln" else rm.rms_ref
    args = (d["x"], d["delta"], d["w"], d["b"], d["dy"], d["ds"], _eps(kind))
    return fn(*args, dtype=dt), fn(*args, dtype=dt, emulate=True)


def _check(dev, kind, rows, C, dt, res):
    d = _inputs(dev, kind, rows, C, dt, res)
    got = _run(kind, d, res)
    for t in got:
        assert t is None or t.dtype == dt
    exact, emu = _refs(kind, d, dt)
    name = {BF: "bf16", HF: "fp16", F32: "fp32"}[dt]
    _compare(f"{'add_' if res else ''}{kind} {rows}x{C} {name}", got, exact, emu)


# bf16: every C at 333 rows (kRpi 1 / one 16-B iteration); the other row counts where the
# instantiation or its sweep differs (8-B kernels: kRpi 2 at 4093 / 8191; 16-B: 1 / 2 iterations)
_BF16 = ([(333, C) for C in (8, 576, 768, 1000, 1536, 2048)] + [(5, 8), (5, 768)] +
         [(4093, 576), (4093, 768), (4093, 2048)] + [(8191, 8), (8191, 768), (8191, 1000), (8191, 1536)])


@pytest.mark.parametrize("res", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("kind", ["ln", "rms"])
@pytest.mark.parametrize("rows,C", _BF16)
def test_norm_bf16(dev, rows, C, kind, res):
    _check(dev, kind, rows, C, BF, res)


@pytest.mark.parametrize("res", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("kind", ["ln", "rms"])
@pytest.mark.parametrize("rows,C", [(333, 576), (333, 768), (4093, 576), (8191, 768)])
def test_norm_fp16(dev, rows, C, kind, res):
    _check(dev, kind, rows, C, HF, res)


@pytest.mark.parametrize("res", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("kind", ["ln", "rms"])
@pytest.mark.parametrize("rows,C", [(333, 768), (4093, 2048), (8191, 1000)])
def test_norm_fp32(dev, rows, C, kind, res):
    """fp32 rows always take the 8-B kernels (NCH 3 / 8 / 4; kRpi 1 / 2 / 2).  The emulated
    reference computes in fp32 like the kernels, so the floor here is fp32 arithmetic itself."""
    _check(dev, kind, rows, C, F32, res)


@pytest.mark.parametrize("kind", ["ln", "rms"])
def test_norm_weight_view_off_16_bytes(dev, kind):
    """γ / β as views 8 bytes into their buffers at C = 768, bf16: both directions must fall back
    from the 16-B half-wave kernels (launch_fwd16 and launch_bwd test the weight's alignment) to
    the 8-B ones, whose 8-B loads such a view satisfies — same bounds as the aligned case."""
    rows, C = 333, 768
    d = _inputs(dev, kind, rows, C, BF, True)
    for n in ("w", "b"):
        buf = torch.zeros(C + 4, device=dev, dtype=BF)
        buf[4:] = d[n]
        d[n] = buf[4:]
        assert d[n].data_ptr() % 16 == 8 and d[n].is_contiguous()
    eps = _eps(kind)
    x, delta = d["x"].clone().requires_grad_(), d["delta"].clone().requires_grad_()
    w, b = d["w"].detach().requires_grad_(), d["b"].detach().requires_grad_()
    assert w.data_ptr() % 16 == 8
    s, y = ops.add_layer_norm(x, delta, w, b, eps) if kind == "ln" else ops.add_rms_norm(x, delta, w, eps)
    torch.autograd.backward([s, y], [d["ds"], d["dy"]])
    torch.cuda.synchronize()
    exact, emu = _refs(kind, d, BF)
    _compare(f"add_{kind} {rows}x{C} bf16 weight+8B", (y, s, x.grad, delta.grad, w.grad, b.grad if kind == "ln" else None),
             exact, emu)


def test_norm_rejects_what_it_has_no_kernel_for(dev):
    """No quiet fall-back inside the extension: bf16 rows with fp32 weights (dispatch_tw has no
    mixed instantiation) and rows 8 bytes off a 16-B boundary (check_rows) are errors."""
    d = _inputs(dev, "ln", 5, 768, BF, False)
    with pytest.raises(RuntimeError, match="weight dtype"):
        torch.ops.nbd.ln_fwd(d["x"], None, d["w"].float(), d["b"].float(), 1e-5)
    with pytest.raises(RuntimeError, match="weight dtype"):
        torch.ops.nbd.rms_fwd(d["x"], None, d["w"].float(), 1e-6)
    buf = torch.zeros(5 * 768 + 4, device=dev, dtype=BF)
    off = buf[4:].view(5, 768)
    assert off.data_ptr() % 16 == 8
    with pytest.raises(RuntimeError, match="16-B aligned"):
        torch.ops.nbd.ln_fwd(off, None, d["w"], d["b"], 1e-5)


def test_embed_rms_norm_fused_producer(dev):
    """ops.embed_rms_norm (gather + RMSNorm in one pass, the residual stream's gradient added in
    the norm's backward): with distinct ids the table's gradient rows are the norm's dx."""
    rows, C, V = 333, 576, 340
    d = _inputs(dev, "rms", rows, C, BF, True)
    g = torch.Generator(device="cpu").manual_seed(2)
    ids = torch.randperm(V, generator=g)[:rows].to(dev)
    table = torch.randn(V, C, generator=g).to(dev, BF)
    table[ids] = d["x"]
    table.requires_grad_()
    w = d["w"].clone().requires_grad_()
    x0, y = ops.embed_rms_norm(ids, table, w, 1e-6)
    torch.autograd.backward([x0, y], [d["ds"], d["dy"]])
    torch.cuda.synchronize()
    assert torch.equal(x0, d["x"])
    rest = torch.ones(V, dtype=torch.bool, device=dev)
    rest[ids] = False
    assert bool((table.grad[rest] == 0).all())
    fn_args = (d["x"], None, d["w"], None, d["dy"], d["ds"], 1e-6)
    exact, emu = rm.rms_ref(*fn_args, dtype=BF), rm.rms_ref(*fn_args, dtype=BF, emulate=True)
    _compare(f"embed_rms {rows}x{C} bf16", (y, None, table.grad[ids], None, w.grad, None), exact, emu)


def test_tokpos_layer_norm_fused_producer(dev):
    """ops.tokpos_layer_norm (token + position embedding and GPT-2's first LayerNorm in one pass):
    x0 = wte[idx] + wpe[pos] is the residual sum; with distinct ids and one batch row the two
    tables' gradient rows are the norm's dx."""
    rows, C, V = 333, 768, 340
    d = _inputs(dev, "ln", rows, C, BF, True)
    g = torch.Generator(device="cpu").manual_seed(3)
    idx = torch.randperm(V, generator=g)[:rows].to(dev)
    wte = torch.randn(V, C, generator=g).to(dev, BF)
    wte[idx] = d["x"]
    wpe = d["delta"].clone().requires_grad_()
    wte.requires_grad_()
    w, b = d["w"].clone().requires_grad_(), d["b"].clone().requires_grad_()
    pos = torch.arange(rows, device=dev)
    x0, y = ops.tokpos_layer_norm(idx[None], wte, pos, wpe, V, w, b, 1e-5)
    torch.autograd.backward([x0, y], [d["ds"][None], d["dy"][None]])
    torch.cuda.synchronize()
    exact, emu = _refs("ln", d, BF)
    _compare(f"tokpos_ln {rows}x{C} bf16", (y[0], x0[0], wte.grad[idx], wpe.grad, w.grad, b.grad), exact, emu)
