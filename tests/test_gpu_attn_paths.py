"""GPU numerics: every path of the HIP flash attention (csrc/kernels/attn.hip) against the fp64
reference of tests/refmath.py, per 32-row tile (one wave's rows: the unit of every wave-uniform
branch in attn.hip) on structured inputs.

The bound is never a constant fitted to the kernel: each test computes
``floor = tile_rel(emulated reference, fp64 reference)`` on its own inputs and asserts
``tile_rel(kernel, fp64 reference) <= 3 x floor`` for out, dq, dk and dv; for lse the same with the
maximum absolute deviation.  tests/test_refmath_mutants.py shows on the CPU that wrong formulas
score >= 9 x floor on these inputs.  Paths are reached by shape (attn_bwd_hip reads its
environment overrides once per process).  Run with ``-s`` for every measured figure and, at the
end, the worst kernel/floor ratio per output (docs/FINDINGS.md keeps the last recorded table)."""
import math

import pytest
import torch

import refmath as rm
from nbdistributed_amd import ops

pytestmark = pytest.mark.gpu

SCALE = 0.125
NAMES = ("out", "lse", "dq", "dk", "dv")
WORST = {}  # output -> (worst kernel/floor ratio, case)


@pytest.fixture(scope="module")
def dev(require_gpu):
    assert ops.native_available(), ops._load_error
    yield torch.device("cuda", 0)
    print("\nworst kernel/floor ratio per output (bound 3):")
    for n, (r, case) in WORST.items():
        print(f"  {n:6s} {r:5.2f}  {case}")


def _note(name, err, floor, case):
    ratio = err / floor if floor > 0 else (0.0 if err == 0 else math.inf)
    print(f"  {case} {name}: kernel {err:.3e} floor {floor:.3e} ratio {ratio:.2f}")
    if ratio > WORST.get(name, (-1.0, ""))[0]:
        WORST[name] = (ratio, case)
    return err <= 3 * floor


def _compare(case, got, exact, emu, names=NAMES, valid=None, rows=32):
    """every output of ``got`` within 3 x the emulated reference's own error (all figures printed
    before the assertion)."""
    bad = []
    for n, x, r, e in zip(names, got, exact, emu):
        if n == "lse":
            err, floor = rm.max_abs(x, r, valid), rm.max_abs(e, r)
        else:
            err, floor = rm.tile_rel(x, r, rows, valid), rm.tile_rel(e, r, rows)
        if not _note(n, err, floor, case):
            bad.append((n, err, floor))
    assert not bad, (case, bad)


def _rope(T, dev):
    return ops.rope_tables(T, 64, 10000.0, dev)


def _kernel(q, k, v, do, causal, rope, dq=None, dk=None, dv=None):
    cos, sin = rope if rope is not None else (None, None)
    o, lse = torch.ops.nbd.attn_fwd(q, k, v, causal, SCALE, cos, sin)
    dq = torch.empty_like(q) if dq is None else dq
    dk = torch.empty_like(k) if dk is None else dk
    dv = torch.empty_like(v) if dv is None else dv
    torch.ops.nbd.attn_bwd(do, q, k, v, o, lse, causal, SCALE, dq, dk, dv, cos, sin)
    torch.cuda.synchronize()
    return o, lse, dq, dk, dv


def _gsplit(B, H, Hkv, T):
    """attn_bwd_hip: a query-head group is split over workgroups when B·Hkv·T/128 < 128."""
    return H // Hkv > 1 and B * Hkv * (T // 128) < 128


def _refs(q, k, v, do, causal, rope, gsplit, chunk=None):
    exact = rm.attn_ref(q, k, v, do, causal, SCALE, rope=rope, chunk=chunk)
    emu = rm.attn_ref(q, k, v, do, causal, SCALE, rope=rope, emulate=True, gsplit=gsplit, chunk=chunk)
    return exact, emu


def _case(dev, B, H, Hkv, T, causal, use_rope, seed, chunk=None):
    rope = _rope(T, dev) if use_rope else None
    q, k, v = (t.to(dev) for t in rm.attn_inputs(B, H, Hkv, T, seed))
    out0, _ = rm.attn_ref(q, k, v, None, causal, SCALE, rope=rope, chunk=chunk)
    do = rm.attn_do(out0, seed + 1)
    del out0
    return q, k, v, do, rope


# group 1: T = 128 one block, no order table; 256 fused δ; 384 the δ pre-pass, an odd block count
# GQA split over workgroups + gqa_reduce_kernel: B·Hkv·T/128 = 8, 12 (< 128)
# GQA unsplit: B·Hkv·T/128 = 128, 132
_MATRIX = [(2, 2, 2, 128), (2, 3, 3, 256), (1, 2, 2, 384),
           (2, 8, 2, 256), (2, 8, 2, 384),
           (64, 4, 1, 256), (22, 6, 2, 384)]


@pytest.mark.parametrize("use_rope", [False, True], ids=["plain", "rope"])
@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("B,H,Hkv,T", _MATRIX)
def test_attention_path_matrix(dev, B, H, Hkv, T, causal, use_rope):
    """{fused δ, δ pre-pass} x {group 1, GQA split, GQA unsplit} x {causal, full} x {RoPE in the
    loads, none}: all five outputs against the fp64 reference."""
    chunk = 16 if B > 16 else None
    q, k, v, do, rope = _case(dev, B, H, Hkv, T, causal, use_rope, seed=B * 1000 + H * 100 + T, chunk=chunk)
    got = _kernel(q, k, v, do, causal, rope)
    exact, emu = _refs(q, k, v, do, causal, rope, _gsplit(B, H, Hkv, T), chunk)
    _compare(f"B{B} H{H}/{Hkv} T{T} {'causal' if causal else 'full'} {'rope' if use_rope else 'plain'}", got, exact, emu)


@pytest.mark.parametrize("B,H,Hkv,T", [(1, 2, 2, 1024), (1, 4, 2, 1024)])
def test_attention_long_causal_tail_tiles(dev, B, H, Hkv, T):
    """T = 1024: the last queries' outputs and the last keys' gradients are ~1/T of the tensor's
    maximum — the tiles a global metric cannot see."""
    q, k, v, do, rope = _case(dev, B, H, Hkv, T, True, False, seed=T + H)
    got = _kernel(q, k, v, do, True, None)
    exact, emu = _refs(q, k, v, do, True, None, _gsplit(B, H, Hkv, T))
    _compare(f"B{B} H{H}/{Hkv} T{T} causal", got, exact, emu)


_CLEAN = {}


def _poison_base(dev, use_rope, gqa):
    """the unpoisoned problem and its references, shared by every cut t0 of one (rope, gqa)."""
    key = (use_rope, gqa)
    if key not in _CLEAN:
        B, H, Hkv, T = 1, (4 if gqa else 2), 2, 384
        rope = _rope(T, dev) if use_rope else None
        (q, k, v), _ = rm.poisoned_inputs(B, H, Hkv, T, 1, seed=17, scale=SCALE, rope=rope)
        q, k, v = (t.to(dev) for t in (q, k, v))
        out0, _ = rm.attn_ref(q, k, v, None, True, SCALE, rope=rope)
        do = rm.attn_do(out0, 18)
        exact, emu = _refs(q, k, v, do, True, rope, _gsplit(B, H, Hkv, T))
        _CLEAN[key] = (rope, do, exact, emu)
    return _CLEAN[key]


@pytest.mark.parametrize("gqa", [False, True], ids=["mha", "gqa"])
@pytest.mark.parametrize("use_rope", [False, True], ids=["plain", "rope"])
@pytest.mark.parametrize("t0", [1, 31, 32, 64, 127, 128, 129, 300])
def test_attention_poisoned_future(dev, t0, use_rope, gqa):
    """Causal, T = 384: keys >= t0 score 20+ nats above every legitimate score, values there are
    ±1024, dO is zero for rows >= t0.  dq, dk, dv at positions >= t0 must be exactly zero, and
    rows < t0 of out, lse, dq must stay within the unpoisoned reference's bound (not bit-equal to
    an unpoisoned kernel run: the forward's deferred-rescale decision is wave-wide and may differ);
    dk, dv of rows < t0 against the poisoned problem's own reference."""
    B, H, Hkv, T = 1, (4 if gqa else 2), 2, 384
    rope, do, clean, clean_emu = _poison_base(dev, use_rope, gqa)
    _, (q, kp, vp) = rm.poisoned_inputs(B, H, Hkv, T, t0, seed=17, scale=SCALE, rope=rope)
    q, kp, vp = (t.to(dev) for t in (q, kp, vp))
    dop = do.clone()
    dop[:, :, t0:] = 0
    out, lse, dq, dk, dv = _kernel(q, kp, vp, dop, True, rope)
    for n, t in (("dq", dq), ("dk", dk), ("dv", dv)):
        assert bool((t[:, :, t0:] == 0).all()), (n, float(t[:, :, t0:].float().abs().max()))
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(lse).all())
    case = f"poison t0={t0} {'rope' if use_rope else 'plain'} {'gqa' if gqa else 'mha'}"
    _compare(case, (out, lse, dq), clean[:3], clean_emu[:3], names=("out", "lse", "dq"), valid=t0)
    pex, pem = _refs(q, kp, vp, dop, True, rope, _gsplit(B, H, Hkv, T))
    if t0 == 1:
        # one live row and one key: P = 1 and dP = δ, so dk[0] = 0·q in exact arithmetic and a
        # rounding residue in fp32 — no non-zero reference to scale by; dv[0] = dO[0] remains
        _compare(case, (dv,), pex[4:], pem[4:], names=("dv",), valid=t0)
    else:
        _compare(case, (dk, dv), pex[3:], pem[3:], names=("dk", "dv"), valid=t0)


def test_attention_block_order_past_first_fill(dev):
    """block_order (attn.hip) builds the causal grids' permutation in two regimes: an LPT first
    fill of CUs x resident slots and a plain tail.  Residency is capped at 8 workgroups per CU (32
    waves over 4 per workgroup), so a forward grid of B·H·T/128 >= 8 x CUs blocks reaches the tail
    whatever the occupancy; a duplicated or dropped item would leave some (batch, head, block)
    stale.  T = 384, GQA, RoPE; the reference goes batch by batch."""
    H, Hkv, T = 8, 2, 384
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    B = -(-8 * cus // (H * (T // 128)))
    assert B * H * (T // 128) >= 8 * cus
    q, k, v, do, rope = _case(dev, B, H, Hkv, T, True, True, seed=99, chunk=8)
    got = _kernel(q, k, v, do, True, rope)
    exact, emu = _refs(q, k, v, do, True, rope, _gsplit(B, H, Hkv, T), chunk=8)
    _compare(f"block order B{B} H{H}/{Hkv} T{T}", got, exact, emu)


@pytest.mark.parametrize("T", [256, 384], ids=["fused-delta", "delta-prepass"])
def test_attention_strided_packed_operands(dev, T):
    """q, k, v as slices of one packed [B, T, (H + 2·Hkv)·64] projection, dO a view of [B, T, H·64]
    and dq, dk, dv slices of a packed gradient (what ops.attention_qkv hands the kernels), once per
    δ path that takes operands by view (the handed-in δ goes through the packed node below)."""
    B, H, Hkv = 2, 4, 2
    q, k, v, do, rope = _case(dev, B, H, Hkv, T, True, True, seed=T + 5)

    def pack(a, b, c):
        return torch.cat([t.transpose(1, 2).reshape(B, T, -1) for t in (a, b, c)], -1).contiguous()

    def split(p):
        a = p[:, :, : H * 64].view(B, T, H, 64).transpose(1, 2)
        b = p[:, :, H * 64:(H + Hkv) * 64].view(B, T, Hkv, 64).transpose(1, 2)
        c = p[:, :, (H + Hkv) * 64:].view(B, T, Hkv, 64).transpose(1, 2)
        return a, b, c

    qs, ks, vs = split(pack(q, k, v))
    assert not qs.is_contiguous() and torch.equal(qs, q) and torch.equal(vs, v)
    dos = do.transpose(1, 2).reshape(B, T, H * 64).contiguous().view(B, T, H, 64).transpose(1, 2)
    dqkv = torch.full((B, T, (H + 2 * Hkv) * 64), float("nan"), device=dev, dtype=torch.bfloat16)
    dqs, dks, dvs = split(dqkv)
    got = _kernel(qs, ks, vs, dos, True, rope, dqs, dks, dvs)
    assert bool(torch.isfinite(dqkv).all())  # every element of the packed gradient written
    exact, emu = _refs(q, k, v, do, True, rope, _gsplit(B, H, Hkv, T))
    _compare(f"strided T{T}", got, exact, emu)


def _proj_ref(q, k, v, w, b, dy, rope, gsplit, emulate):
    """attention -> Linear(w, b) and its backward on the formulas of refmath: y, dq|dk|dv, dW, db.
    Emulated: the attention output, y, dO (= dy·W, the attention backward's input), dW and db are
    stored as bf16 by the GEMMs."""
    bf = torch.bfloat16
    rd = (lambda t: t.to(bf).double()) if emulate else (lambda t: t)
    B, H, T, _ = q.shape
    out, _ = rm.attn_ref(q, k, v, None, True, SCALE, rope=rope, emulate=emulate)
    a = out.transpose(1, 2).reshape(B * T, H * 64)
    w, b, dy2 = w.double(), b.double(), dy.double().reshape(B * T, -1)
    y = rd(a @ w.t() + b)
    do = rd(dy2 @ w).view(B, T, H, 64).transpose(1, 2)
    dw, db = rd(dy2.t() @ a), rd(dy2.sum(0))
    _, _, dq, dk, dv = rm.attn_ref(q, k, v, do, True, SCALE, rope=rope, emulate=emulate, gsplit=gsplit)
    return y.view(B, T, -1), dq, dk, dv, dw, db


@pytest.mark.parametrize("use_rope", [False, True], ids=["plain", "rope"])
@pytest.mark.parametrize("Hkv", [4, 2], ids=["mha", "gqa"])
@pytest.mark.parametrize("T", [384, 512])
def test_attention_delta_from_out_projection(dev, T, Hkv, use_rope):
    """δ handed in by the output projection: ops.attention_qkv -> ops.gemm_linear on the native
    nodes, where the Linear's grouped backward launch computes δ in its epilogue (gemm.hip
    EPI_ADELTA) and attn_bwd_hip skips the pre-pass.  autograd.hip exposes no way to tell which
    path ran: it is chosen by T > 256 (AttnQKVFn::forward) with NBD_ATTN_DELTA_EPI unset.
    y, the packed q|k|v gradient per head and 32-row tile, dW per output row and db."""
    B, H = 2, 4
    C = H * 64
    rope = _rope(T, dev) if use_rope else None
    q, k, v = (t.to(dev) for t in rm.attn_inputs(B, H, Hkv, T, seed=T + Hkv))
    g = torch.Generator(device="cpu").manual_seed(T)
    w = (torch.randn(C, C, generator=g) * 0.05).to(dev, torch.bfloat16)
    b = (torch.randn(C, generator=g) * 0.1).to(dev, torch.bfloat16)
    gs = _gsplit(B, H, Hkv, T)
    y0 = _proj_ref(q, k, v, w, b, torch.zeros(B, T, C, device=dev), rope, gs, False)[0]
    dy = (torch.randn(B, T, C, generator=g).to(dev) + 2 * y0.float()).bfloat16()
    qkv = torch.cat([t.transpose(1, 2).reshape(B, T, -1) for t in (q, k, v)], -1).contiguous().requires_grad_()
    wp, bp = w.clone().requires_grad_(), b.clone().requires_grad_()
    y = ops.gemm_linear(ops.attention_qkv(qkv, H, causal=True, scale=SCALE, n_kv_head=Hkv, rope=rope), wp, bp)
    y.backward(dy)
    torch.cuda.synchronize()
    d = qkv.grad
    dq = d[:, :, : H * 64].view(B, T, H, 64).transpose(1, 2)
    dk = d[:, :, H * 64:(H + Hkv) * 64].view(B, T, Hkv, 64).transpose(1, 2)
    dv = d[:, :, (H + Hkv) * 64:].view(B, T, Hkv, 64).transpose(1, 2)
    exact = _proj_ref(q, k, v, w, b, dy, rope, gs, False)
    emu = _proj_ref(q, k, v, w, b, dy, rope, gs, True)
    case = f"out-proj δ T{T} H{H}/{Hkv} {'rope' if use_rope else 'plain'}"
    _compare(case, (y, dq, dk, dv), exact[:4], emu[:4], names=("y", "dq", "dk", "dv"))
    _compare(case, (wp.grad, bp.grad), exact[4:], emu[4:], names=("dW", "db"), rows=1)
