"""GPU numerics: every instantiation of the bf16 MFMA GEMMs (csrc/kernels/gemm.hip, gemm256.hip)
against the fp64 reference of tests/refmath_gemm.py, per 16x16 output fragment, on structured
inputs: a magnitude of its own per fragment, over three decades, K-steps of unequal weight,
row sums that do not cancel, and — for the activations — pre-activations where GELU and SiLU bend.

The bound is never a constant fitted to the kernel: each case computes
``floor = tile_rel2(emulated reference, fp64 reference, 16, 16)`` on its own inputs and asserts
``tile_rel2(kernel, fp64 reference, 16, 16) <= 3 x floor`` for every output.
tests/test_gemm_ref.py shows on the CPU that wrong formulas score >= 9 x floor here, and that a
truncated bf16 result shows in ``signed_bias``, which the rounding-direction cases assert.

Shapes: 3 x 5 tiles of each kernel's own size, 3 x 6 for the 96-wide one (no tile count a multiple of 8: the XCD remap's
ragged part and a short last tile group run; row-sum owners at tn == 0, SwiGLU's n0/2 and the last
tiles all exist).  K-tile counts 1, 2, 3, stages + 1 and one that wraps the ring twice and ends
mid-ring (per K-group for the kernels with two).  Run with ``-s`` for every figure and the worst
kernel/floor ratio per output."""
import math

import pytest
import torch

import refmath_gemm as rg
from nbdistributed_amd.ops import gemm as G
from refmath_gemm import EPI_DGELU, EPI_DSWIGLU, EPI_GELU, EPI_NONE, EPI_ROWSUM, EPI_SWIGLU

pytestmark = pytest.mark.gpu

LAYOUTS = {"fwd": (False, False), "dgrad": (False, True), "wgrad": (True, True)}
WORST = {}
BIAS = []

# tile code = ks*10^8 + waves*10^7 + stages*10^6 + BM*1000 + BN (ops/gemm.py matmul); every kernel
# gemm.hip launch_epi builds for all three layouts ...
ALL = ([s * 1000000 + t for t in (128128, 128064, 64128, 64064) for s in (2, 3)] +
       [200000000 + s * 1000000 + t for t in (128064, 64128, 64064) for s in (2, 3)] +
       [82128128, 83128128, 89128128])  # 8 waves; 9: the ping-pong schedule
FWD96 = [2128096, 3128096]              # ... forward layout only (any forward epilogue)
FWD192 = [82128192, 83128192]           # ... forward layout, plain / bias / GELU only
T256 = 80256256


def _geom(tile):
    ks = 2 if tile // 100000000 == 2 else 1
    stages = tile // 1000000 % 10
    return tile // 1000 % 1000, tile % 1000, ks, (3 if stages == 9 else stages)


def _mn(tile):
    """3 x 5 tiles of the kernel's own size; 3 x 6 for the 96-wide tile (ops.gemm.matmul takes
    64-granular shapes only, and 5 x 96 is not one: it would run the PyTorch path)."""
    bm, bn = _geom(tile)[:2]
    return 3 * bm, (6 if bn == 96 else 5) * bn


def _matmul(a, b, a_km=False, b_kn=False, **kw):
    """ops.gemm.matmul, on the HIP kernels for certain: a shape it would route to PyTorch is an
    error here, not a pass."""
    M, K = (a.shape[1], a.shape[0]) if a_km else a.shape
    N = b.shape[1] if b_kn else b.shape[0]
    assert kw.get("tile", 0) > 0 and kw.get("splits", 0) > 0 and G.gemm_ok(M, N, K) and a.is_cuda, (M, N, K)
    return G.matmul(a, b, a_km=a_km, b_kn=b_kn, **kw)


def _kcounts(ring):
    return (1, 2, 3, 5) if ring == 2 else (1, 2, 3, 4, 7)


@pytest.fixture(scope="module")
def dev(require_gpu):
    from nbdistributed_amd import ops

    ops.load_library()
    yield torch.device("cuda", 0)
    print("\nworst kernel/floor ratio per output (bound 3):")
    for n, (r, case) in sorted(WORST.items()):
        print(f"  {n:14s} {r:5.2f}  {case}")
    print("signed bias, kernel vs truncation (bound 0.25):")
    for case, kb, tb in BIAS:
        print(f"  {case:28s} kernel {kb:+.2e}  truncated {tb:+.2e}  ratio {abs(kb) / abs(tb):.3f}")


_INPUTS = {}


def _inputs(dev, M, N, K, layout, seed, act=False):
    key = (M, N, K, layout, seed, act)
    if key not in _INPUTS:
        if len(_INPUTS) > 8:
            _INPUTS.clear()
        a_km, b_kn = LAYOUTS[layout]
        _INPUTS[key] = {n: t.to(dev) for n, t in rg.gemm_inputs(M, N, K, a_km, b_kn, seed, act=act).items()}
    return _INPUTS[key]


def _tup(r):
    return r if isinstance(r, tuple) else (r,)


def _compare(case, names, got, exact, emu):
    """kernel <= 3 x floor for each output; the names key the worst-ratio table."""
    bad = []
    for n, x, r, e in zip(names, _tup(got), _tup(exact), _tup(emu)):
        assert x.dtype == torch.bfloat16 and x.shape == r.shape, (case, n, x.shape, r.shape)
        err, floor = rg.tile_rel2(x, r, 16, 16), rg.tile_rel2(e, r, 16, 16)
        ratio = err / floor if floor > 0 else (0.0 if err == 0 else math.inf)
        print(f"  {case} {n}: kernel {err:.3e} floor {floor:.3e} ratio {ratio:.2f}")
        if ratio > WORST.get(n, (-1.0, ""))[0]:
            WORST[n] = (ratio, case)
        if not err <= 3 * floor:
            bad.append((n, err, floor))
    assert not bad, (case, bad)


def _refs(args, chunk=None, **kw):
    """(fp64 reference, emulated reference) of one product; ``chunk``: rows per pass (A [M, K])."""
    if chunk is None:
        return rg.gemm_ref(*args, **kw), rg.gemm_ref(*args, emulate=True, **kw)
    a, b, a_km, b_kn = args
    assert not a_km
    aux = kw.pop("aux", None)
    parts = []
    for m0 in range(0, a.shape[0], chunk):
        k = dict(kw, aux=None if aux is None else aux[m0:m0 + chunk])
        ar = (a[m0:m0 + chunk], b, a_km, b_kn)
        parts.append((_tup(rg.gemm_ref(*ar, **k)), _tup(rg.gemm_ref(*ar, emulate=True, **k))))
    cat = lambda i: tuple(torch.cat([p[i][n] for p in parts], 0) for n in range(len(parts[0][i])))  # noqa: E731
    return cat(0), cat(1)


# ----------------------------------------------------------------------------------- plain products
@pytest.mark.parametrize("tile,layout", [(t, lay) for t in ALL for lay in LAYOUTS] +
                         [(t, "fwd") for t in FWD96 + FWD192])
def test_plain_product_every_kernel_and_ring_phase(dev, tile, layout):
    (M, N), (_, _, ks, ring) = _mn(tile), _geom(tile)
    a_km, b_kn = LAYOUTS[layout]
    for nk in _kcounts(ring):
        K = 64 * nk * ks
        d = _inputs(dev, M, N, K, layout, seed=tile % 1000 + nk)
        c = _matmul(d["a"], d["b"], a_km=a_km, b_kn=b_kn, tile=tile, splits=1)
        exact, emu = _refs((d["a"], d["b"], a_km, b_kn))
        _compare(f"plain {tile} {layout} K={K}", ("plain c",), c, exact, emu)


# ---------------------------------------------------------------------------------------- epilogues
@pytest.mark.parametrize("tile", ALL + FWD96 + FWD192)
def test_bias_and_gelu_epilogues(dev, tile):
    (M, N), ks = _mn(tile), _geom(tile)[2]
    K = 192 if ks == 1 else 256
    d = _inputs(dev, M, N, K, "fwd", seed=31, act=True)
    args = (d["a"], d["b"], False, False)
    c = _matmul(d["a"], d["b"], bias=d["bias"], tile=tile, splits=1)
    _compare(f"bias {tile}", ("bias c",), c, *_refs(args, bias=d["bias"]))
    got = _matmul(d["a"], d["b"], bias=d["bias"], epi=EPI_GELU, tile=tile, splits=1)
    _compare(f"gelu {tile}", ("gelu act", "gelu pre"), got, *_refs(args, bias=d["bias"], epi=EPI_GELU))


@pytest.mark.parametrize("tile", ALL)
def test_dgelu_epilogue(dev, tile):
    (M, N), ks = _mn(tile), _geom(tile)[2]
    K = 192 if ks == 1 else 256
    d = _inputs(dev, M, N, K, "dgrad", seed=32, act=True)
    c = _matmul(d["a"], d["b"], b_kn=True, epi=EPI_DGELU, aux=d["aux"], tile=tile, splits=1)
    _compare(f"dgelu {tile}", ("dgelu c",), c, *_refs((d["a"], d["b"], False, True), epi=EPI_DGELU, aux=d["aux"]))


@pytest.mark.parametrize("tile", ALL + FWD96)
def test_swiglu_epilogue(dev, tile):
    """N = 2I = 5 (6) column tiles: tile tn stages gate rows tn·BN/2.. and up rows I + tn·BN/2.."""
    (M, N), ks = _mn(tile), _geom(tile)[2]
    K = 192 if ks == 1 else 256
    d = _inputs(dev, M, N, K, "fwd", seed=33, act=True)
    act, gu = _matmul(d["a"], d["b"], epi=EPI_SWIGLU, tile=tile, splits=1)
    assert act.shape == (M, N // 2) and gu.shape == (M, N)
    _compare(f"swiglu {tile}", ("swiglu act", "swiglu gu"), (act, gu),
             *_refs((d["a"], d["b"], False, False), epi=EPI_SWIGLU))


@pytest.mark.parametrize("tile", ALL)
def test_dswiglu_epilogue(dev, tile):
    (M, N), ks = _mn(tile), _geom(tile)[2]
    K = 192 if ks == 1 else 256
    d = _inputs(dev, M, N, K, "dgrad", seed=34, act=True)
    dgu = _matmul(d["a"], d["b"], b_kn=True, epi=EPI_DSWIGLU, aux=d["aux2"], tile=tile, splits=1)
    assert dgu.shape == (M, 2 * N)
    _compare(f"dswiglu {tile}", ("dswiglu d[g|u]",), dgu,
             *_refs((d["a"], d["b"], False, True), epi=EPI_DSWIGLU, aux=d["aux2"]))


@pytest.mark.parametrize("tile", ALL)
def test_rowsum_epilogue_splits_and_k_groups(dev, tile):
    """dW = dyᵀ·x with db = Σ dy: the owners at tn == 0, the K-groups' `rsb` exchange, the splits'
    partials through reduce_kernel."""
    (M, N), ks = _mn(tile), _geom(tile)[2]
    for S in (1, 2, 8):
        K = 64 * 3 * ks * S
        d = _inputs(dev, M, N, K, "wgrad", seed=35 + S, act=True)
        got = _matmul(d["a"], d["b"], a_km=True, b_kn=True, epi=EPI_ROWSUM, splits=S, tile=tile)
        assert got[1].shape == (M,)
        _compare(f"rowsum {tile} S={S}", ("rowsum c", "rowsum sums"), got,
                 *_refs((d["a"], d["b"], True, True), epi=EPI_ROWSUM, splits=S, kgroups=ks))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("splits", [2, 4, 8])
@pytest.mark.parametrize("tile", [2128128, 3064064])
def test_split_k(dev, tile, splits, layout):
    (M, N), K = _mn(tile), 64 * splits * 3
    a_km, b_kn = LAYOUTS[layout]
    d = _inputs(dev, M, N, K, layout, seed=40 + splits)
    c = _matmul(d["a"], d["b"], a_km=a_km, b_kn=b_kn, tile=tile, splits=splits)
    _compare(f"split-K {tile} {layout} S={splits}", ("split-K c",), c,
             *_refs((d["a"], d["b"], a_km, b_kn), splits=splits))


# ------------------------------------------------------------------------------------------ gemm256
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("variant", range(7))
def test_gemm256_variants(dev, variant, layout):
    M, N = 512, 768
    a_km, b_kn = LAYOUTS[layout]
    for nk in (1, 2, 3, 5, 17):
        d = _inputs(dev, M, N, 64 * nk, layout, seed=50 + nk)
        c = _matmul(d["a"], d["b"], a_km=a_km, b_kn=b_kn, tile=T256 + (variant + 2) * 1000000, splits=1)
        _compare(f"gemm256 v{variant} {layout} K={64 * nk}", ("256 c",), c,
                 *_refs((d["a"], d["b"], a_km, b_kn), tile256=True))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("variant", [0, 6])
def test_gemm256_split_k(dev, variant, layout):
    M, N = 512, 768
    a_km, b_kn = LAYOUTS[layout]
    for S in (2, 4):
        d = _inputs(dev, M, N, 64 * 3 * S, layout, seed=60 + S)
        c = _matmul(d["a"], d["b"], a_km=a_km, b_kn=b_kn, tile=T256 + (variant + 2) * 1000000, splits=S)
        _compare(f"gemm256 v{variant} {layout} S={S}", ("256 split-K c",), c,
                 *_refs((d["a"], d["b"], a_km, b_kn), splits=S))


@pytest.mark.parametrize("variant", range(6))
def test_gemm256_epilogues(dev, variant):
    """bias, GELU and GELU' against the fp64 reference (not against the kernel's own ``pre``);
    this family rounds the pre-activation before the activation (refmath_gemm ``tile256``)."""
    M, N, K = 512, 768, 192
    tile = T256 + (variant + 2) * 1000000
    d = _inputs(dev, M, N, K, "fwd", seed=71, act=True)
    args = (d["a"], d["b"], False, False)
    c = _matmul(d["a"], d["b"], bias=d["bias"], tile=tile, splits=1)
    _compare(f"gemm256 v{variant} bias", ("256 bias c",), c, *_refs(args, bias=d["bias"], tile256=True))
    got = _matmul(d["a"], d["b"], bias=d["bias"], epi=EPI_GELU, tile=tile, splits=1)
    _compare(f"gemm256 v{variant} gelu", ("256 gelu act", "256 gelu pre"), got,
             *_refs(args, bias=d["bias"], epi=EPI_GELU, tile256=True))
    d = _inputs(dev, M, N, K, "dgrad", seed=72, act=True)
    c = _matmul(d["a"], d["b"], b_kn=True, epi=EPI_DGELU, aux=d["aux"], tile=tile, splits=1)
    _compare(f"gemm256 v{variant} dgelu", ("256 dgelu c",), c,
             *_refs((d["a"], d["b"], False, True), epi=EPI_DGELU, aux=d["aux"], tile256=True))


# ------------------------------------------------------------------------------------- column split
def _colsplit_refs(args, N0, **kw):
    """columns < N0 run on the 256x256 kernel (its epilogue's roundings), the rest on the tail."""
    exact, tail = _refs(args, chunk=2048, **dict(kw))
    if N0 == 0:
        return exact, tail
    _, head = _refs(args, chunk=2048, tile256=True, **dict(kw))
    return exact, tuple(torch.cat([h[:, :N0], t[:, N0:]], 1) for h, t in zip(head, tail))


@pytest.mark.parametrize("what", ["plain", "gelu", "dgelu"])
@pytest.mark.parametrize("N", [2304, 768])
def test_column_split(dev, N, what):
    """M = 8192: a round of 256x256 tiles is 2048 columns, so N = 2304 splits 2048 + 256 and
    N = 768 has no whole round (the tail tile runs everything)."""
    M, K = 8192, 128
    N0 = N // 2048 * 2048
    tile = G.COLSPLIT + 82128128
    layout = "dgrad" if what == "dgelu" else "fwd"
    d = _inputs(dev, M, N, K, layout, seed=80 + N, act=True)
    args = (d["a"], d["b"]) + LAYOUTS[layout]
    if what == "plain":
        got = _matmul(d["a"], d["b"], tile=tile, splits=1)
        names, kw = ("colsplit c",), {}
    elif what == "gelu":
        got = _matmul(d["a"], d["b"], bias=d["bias"], epi=EPI_GELU, tile=tile, splits=1)
        names, kw = ("colsplit act", "colsplit pre"), dict(bias=d["bias"], epi=EPI_GELU)
    else:
        got = _matmul(d["a"], d["b"], b_kn=True, epi=EPI_DGELU, aux=d["aux"], tile=tile, splits=1)
        names, kw = ("colsplit dgelu",), dict(epi=EPI_DGELU, aux=d["aux"])
    _compare(f"colsplit N={N} {what}", names, got, *_colsplit_refs(args, N0, **kw))


# ----------------------------------------------------------------------------------- grouped launch
def _pair_inputs(dev, M, N, K, seed, swiglu=False):
    """dy [M, N], w [N, K], x [M, K] (+ the pre-activations) from two structured draws.  dy is
    an operand of both products: its row-block scales serve dx = dy·w; for dW = dyᵀ·x its columns
    get block scales too (powers of two: exact) and a mean each, so db = Σ dy does not cancel."""
    d1 = _inputs(dev, M, K, N, "dgrad", seed=seed, act=True)       # a = dy [M, N], b = w as [N][K]
    d2 = _inputs(dev, N, K, M, "wgrad", seed=seed + 1, act=True)   # b = x [M][K]
    dy = d1["a"].float() * rg.block_scales(N, rg._SCALES[True][1]).to(dev).float()[None, :]
    sign = torch.where(torch.arange(N, device=dev) % 3 == 0, -1.0, 1.0)
    dy = (dy + 0.5 * sign * dy.abs().mean(0, keepdim=True)).bfloat16()
    return dy, d1["b"], d2["b"], (d1["aux2"] if swiglu else d1["aux"])


def _pair_compare(case, got, dy, w, x, **kw):
    bm = 128 if all(v % 128 == 0 for v in (*dy.shape, w.shape[1])) else 64
    exact = rg.gemm_pair_ref(dy, w, x, bm=bm, bn=bm, **kw)
    emu = rg.gemm_pair_ref(dy, w, x, bm=bm, bn=bm, emulate=True, **kw)
    keep = [i for i in range(3) if exact[i] is not None]
    assert all((got[i] is None) == (exact[i] is None) for i in range(3))
    names = ("pair dx", "pair dw", "pair db")
    _compare(case, [names[i] for i in keep], tuple(got[i] for i in keep), tuple(exact[i] for i in keep),
             tuple(emu[i] for i in keep))


@pytest.mark.parametrize("dgelu", [False, True])
@pytest.mark.parametrize("bias_grad", [False, True])
@pytest.mark.parametrize("M,N,K", [(1024, 256, 384), (1024, 320, 192)])  # 128- and 64-tile kernels
def test_backward_pair(dev, M, N, K, bias_grad, dgelu):
    dy, w, x, pre = _pair_inputs(dev, M, N, K, seed=90)
    epi1 = EPI_DGELU if dgelu else EPI_NONE
    got = G.backward_pair(dy, w, x, epi1, pre if dgelu else None, bias_grad=bias_grad)
    assert got is not None
    S = G.pair_schedule(M, N, K, 128 if K % 128 == 0 and N % 128 == 0 else 64, epi1) & 15
    _pair_compare(f"pair {M}x{N}x{K} dgelu={dgelu} db={bias_grad}", got, dy, w, x, epi1=epi1,
                  aux1=pre if dgelu else None, epi2=EPI_ROWSUM if bias_grad else EPI_NONE, splits=S)


@pytest.mark.parametrize("sched", [1 | 16, 2, 2 | 16, 4 | 16, 8, 8 | 16])
@pytest.mark.parametrize("M,N,K", [(1024, 256, 384), (1024, 320, 192)])
def test_pair_schedules(dev, M, N, K, sched):
    """Every split count / dispatch order (S | wfirst << 4) of the grouped launch, written into
    NaN-filled outputs."""
    dy, w, x, pre = _pair_inputs(dev, M, N, K, seed=92)
    nan = lambda *s: torch.full(s, float("nan"), device=dev, dtype=torch.bfloat16)  # noqa: E731
    dx, dw, db = nan(M, K), nan(N, K), nan(N)
    torch.ops.nbd.gemm_pair(dy, w, dx, EPI_DGELU, pre, dy, x, dw, EPI_ROWSUM, db, sched)
    _pair_compare(f"pair {M}x{N}x{K} sched={sched}", (dx, dw, db), dy, w, x, epi1=EPI_DGELU, aux1=pre,
                  epi2=EPI_ROWSUM, splits=sched & 15)


def test_backward_pair_dswiglu(dev):
    M, N, I = 1024, 512, 1024
    dy, w, x, pre = _pair_inputs(dev, M, N, I, seed=94, swiglu=True)
    got = G.backward_pair(dy, w, x, EPI_DSWIGLU, pre)
    assert got is not None and got[0].shape == (M, 2 * I)
    S = G.pair_schedule(M, N, I, 128, EPI_DSWIGLU) & 15
    _pair_compare("pair dswiglu", got, dy, w, x, epi1=EPI_DSWIGLU, aux1=pre, splits=S)


@pytest.mark.parametrize("dgelu", [False, True])
def test_backward_pair_ping_pong(dev, dgelu, monkeypatch):
    monkeypatch.setenv("NBD_GEMM_PAIR_PP", "1")
    M, N, K = 1024, 256, 384
    dy, w, x, pre = _pair_inputs(dev, M, N, K, seed=96)
    epi1 = EPI_DGELU if dgelu else EPI_NONE
    got = G.backward_pair(dy, w, x, epi1, pre if dgelu else None, bias_grad=True)
    S = G.pair_schedule(M, N, K, 128, epi1) & 15
    _pair_compare(f"pair ping-pong dgelu={dgelu}", got, dy, w, x, epi1=epi1, aux1=pre if dgelu else None,
                  epi2=EPI_ROWSUM, splits=S)


# ------------------------------------------------------------------------------- rounding direction
def _direction(case, got, exact, trunc):
    for n, x, r, t in zip(case[1], _tup(got), _tup(exact), _tup(trunc)):
        kb, tb = rg.signed_bias(x, r), rg.signed_bias(t, r)
        print(f"  {case[0]} {n}: signed bias kernel {kb:+.3e} truncated {tb:+.3e}")
        BIAS.append((f"{case[0]} {n}", kb, tb))
        assert tb < 0 and abs(kb) <= 0.25 * abs(tb), (case[0], n, kb, tb)


@pytest.mark.parametrize("path", ["pack2_bf16", "store8_gelu", "store8_swiglu", "reduce_kernel", "gemm256_v0",
                                  "gemm256_v6"])
def test_rounding_direction(dev, path):
    """One case per distinct store path: the kernel's mean signed relative error is within a
    quarter of the way from round-to-nearest (~1e-3 of the way) to truncation, both measured on
    the case's own inputs."""
    big = path.startswith("gemm256")
    M, N, K = (512, 768, 192) if big else (384, 640, 192)
    d = _inputs(dev, M, N, K, "fwd", seed=99, act=True)
    args = (d["a"], d["b"], False, False)
    if path == "pack2_bf16":  # the plain single-launch epilogue
        got, kw, names = _matmul(d["a"], d["b"], bias=d["bias"], tile=2128128, splits=1), dict(bias=d["bias"]), ("c",)
    elif path == "store8_gelu":  # store8 (activation) and store8_nt (pre-activation)
        got = _matmul(d["a"], d["b"], bias=d["bias"], epi=EPI_GELU, tile=2128128, splits=1)
        kw, names = dict(bias=d["bias"], epi=EPI_GELU), ("act", "pre")
    elif path == "store8_swiglu":
        got, kw, names = _matmul(d["a"], d["b"], epi=EPI_SWIGLU, tile=2128128, splits=1), dict(epi=EPI_SWIGLU), ("act", "gu")
    elif path == "reduce_kernel":
        K = 384
        d = _inputs(dev, M, N, K, "fwd", seed=98, act=True)
        args = (d["a"], d["b"], False, False)
        got, kw, names = _matmul(d["a"], d["b"], tile=2128128, splits=2), dict(splits=2), ("c",)
    else:
        v = 0 if path.endswith("v0") else 6
        got = _matmul(d["a"], d["b"], tile=T256 + (v + 2) * 1000000, splits=1)
        kw, names = dict(tile256=True), ("c",)
    exact = rg.gemm_ref(*args, **kw)
    trunc = rg.gemm_ref(*args, emulate=True, mutant="trunc", **kw)
    _direction((path, names), got, exact, trunc)
