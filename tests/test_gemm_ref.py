"""CPU proof that the tile-wise GEMM tests (test_gpu_gemm_paths.py) can fail, and that their
reference is right: tests/refmath_gemm.py against a second derivation (fp64 autograd of
``F.linear`` / ``F.gelu`` / ``F.silu``), its floors, and every deliberately wrong "mutant" of the
kernels' formulas, where

    floor = tile_rel2(emulated reference, fp64 reference, 16, 16)   (what a correct kernel may show)
    tol   = 3 x floor                                               (the GPU tests' bound)
    score = tile_rel2(emulated mutant, fp64 reference, 16, 16) >= 3 x tol

on every output the mutant is expected to move.  ``trunc`` (a bf16 result truncated instead of
rounded to nearest) moves that score by only 2x and goes by the sign of the error instead.
Run with ``-s`` to print the floors and the scores."""
import pytest
import torch
import torch.nn.functional as F

import refmath_gemm as rg
from refmath_gemm import EPI_DGELU, EPI_DSWIGLU, EPI_GELU, EPI_NONE, EPI_ROWSUM, EPI_SWIGLU

LAYOUTS = {"fwd": (False, False), "dgrad": (False, True), "wgrad": (True, True)}

# mutant -> (case, the outputs it must move by >= 3 x tol); outputs are named as the op returns them
GEMM_HITS = {
    "gelu_silu": ("gelu", ("c",)),
    "gelu_relu": ("gelu", ("c",)),
    "gelu_before_bias": ("gelu", ("c",)),
    "dgelu_first_term_only": ("dgelu", ("c",)),
    "swiglu_relu_gate": ("swiglu", ("c",)),
    "swiglu_halves_swapped": ("swiglu", ("c",)),
    "swiglu_up_rows": ("swiglu", ("c", "aux")),
    "dswiglu_swapped": ("dswiglu", ("c",)),
    "bias_frag_shift": ("bias", ("c",)),
    "bias_last_tile": ("bias", ("c",)),
    "drop_kstep": ("bias", ("c",)),
    "drop_last_ktile": ("bias", ("c",)),
    "frag_transposed": ("bias", ("c",)),
    "rowsum_kgroup": ("rowsum", ("aux",)),
    "rowsum_last_split": ("rowsum", ("aux",)),
    "slab_last": ("rowsum", ("c",)),
}
BM = BN = 64  # the tile geometry of the mutants below


def _named(r):
    return dict(zip(("c", "aux"), r)) if isinstance(r, tuple) else {"c": r}


def _scores(x, ref):
    x, ref = _named(x), _named(ref)
    return {n: rg.tile_rel2(x[n], ref[n], 16, 16) for n in ref}


_CASES = {}


def _case(name):
    """The smallest shapes at which every mutant can exist, 64x64 tiles: 2 row tiles x 3 column
    tiles (SwiGLU: 3 column tiles of 32 features), 3 K-tiles; the row-sum case 2 splits x 2
    K-groups x 1 K-tile.  act=True inputs throughout: the activations bend."""
    if name not in _CASES:
        M, N, K = 128, 192, 192
        kw = dict(bm=BM, bn=BN)
        if name in ("bias", "gelu"):
            d = rg.gemm_inputs(M, N, K, False, False, seed=11, act=True)
            args = (d["a"], d["b"], False, False)
            kw.update(bias=d["bias"], epi=EPI_GELU if name == "gelu" else EPI_NONE)
        elif name == "dgelu":
            d = rg.gemm_inputs(M, N, K, False, True, seed=12, act=True)
            args = (d["a"], d["b"], False, True)
            kw.update(epi=EPI_DGELU, aux=d["aux"])
        elif name == "swiglu":
            d = rg.gemm_inputs(M, N, K, False, False, seed=13, act=True)
            args = (d["a"], d["b"], False, False)
            kw.update(epi=EPI_SWIGLU)
        elif name == "dswiglu":
            d = rg.gemm_inputs(M, N, K, False, True, seed=14, act=True)
            args = (d["a"], d["b"], False, True)
            kw.update(epi=EPI_DSWIGLU, aux=d["aux2"])
        else:
            d = rg.gemm_inputs(M, N, 256, True, True, seed=15, act=True)
            args = (d["a"], d["b"], True, True)
            kw.update(epi=EPI_ROWSUM, splits=2, kgroups=2)
        exact = rg.gemm_ref(*args, **kw)
        emu = rg.gemm_ref(*args, emulate=True, **kw)
        _CASES[name] = (args, kw, exact, emu, _scores(emu, exact))
    return _CASES[name]


# ------------------------------------------------------- the reference against a second derivation
def _close(x, ref):
    assert x.dtype == torch.float64 and x.shape == ref.shape
    assert float((x - ref).abs().max()) <= 1e-12 * float(ref.abs().max()), float((x - ref).abs().max())


@pytest.mark.parametrize("layout", LAYOUTS)
def test_reference_plain_product_and_bias_match_linear(layout):
    a_km, b_kn = LAYOUTS[layout]
    M, N, K = 64, 96, 128
    d = rg.gemm_inputs(M, N, K, a_km, b_kn, seed=1, act=True)
    x = d["a"].double().t() if a_km else d["a"].double()
    w = d["b"].double().t() if b_kn else d["b"].double()
    _close(rg.gemm_ref(d["a"], d["b"], a_km, b_kn), F.linear(x, w))
    if layout == "fwd":
        _close(rg.gemm_ref(d["a"], d["b"], a_km, b_kn, bias=d["bias"]), F.linear(x, w, d["bias"].double()))
    for s in (2,):  # split-K changes nothing in fp64
        _close(rg.gemm_ref(d["a"], d["b"], a_km, b_kn, splits=s), F.linear(x, w))


def test_reference_gelu_and_its_backward_match_autograd():
    M, N, K = 64, 96, 128
    d = rg.gemm_inputs(M, N, K, False, False, seed=2, act=True)
    act, pre = rg.gemm_ref(d["a"], d["b"], False, False, bias=d["bias"], epi=EPI_GELU)
    want = F.linear(d["a"].double(), d["b"].double(), d["bias"].double())
    _close(pre, want)
    _close(act, F.gelu(want, approximate="tanh"))
    # GELU' on the dgrad layout: dact·gelu'(aux) is the gradient of gelu(aux) for the incoming dact
    d = rg.gemm_inputs(M, N, K, False, True, seed=3, act=True)
    h = d["aux"].double().requires_grad_()
    dact = d["a"].double() @ d["b"].double()
    F.gelu(h, approximate="tanh").backward(dact)
    _close(rg.gemm_ref(d["a"], d["b"], False, True, epi=EPI_DGELU, aux=d["aux"]), h.grad)


def test_reference_swiglu_and_its_backward_match_autograd():
    M, N, K = 64, 96, 128
    d = rg.gemm_inputs(M, 2 * N, K, False, False, seed=4, act=True)
    act, gu = rg.gemm_ref(d["a"], d["b"], False, False, epi=EPI_SWIGLU)
    want = F.linear(d["a"].double(), d["b"].double())
    _close(gu, want)
    _close(act, F.silu(want[:, :N]) * want[:, N:])
    d = rg.gemm_inputs(M, N, K, False, True, seed=5, act=True)
    pre = d["aux2"].double().requires_grad_()
    dact = d["a"].double() @ d["b"].double()
    (F.silu(pre[:, :N]) * pre[:, N:]).backward(dact)
    _close(rg.gemm_ref(d["a"], d["b"], False, True, epi=EPI_DSWIGLU, aux=d["aux2"]), pre.grad)


@pytest.mark.parametrize("splits", [1, 2])
def test_reference_rowsum_and_pair_match_linear_backward(splits):
    """The grouped backward of y = x·Wᵀ + b for an incoming dy: dx, dW and db from autograd."""
    T, O, I = 128, 64, 128  # tokens, out features, in features
    d = rg.gemm_inputs(T, O, I, False, False, seed=6, act=True)
    g = torch.Generator(device="cpu").manual_seed(7)
    dy = torch.randn(T, O, generator=g).bfloat16()
    x, w = d["a"], torch.randn(O, I, generator=g).bfloat16()
    xr, wr, br = x.double().requires_grad_(), w.double().requires_grad_(), torch.zeros(O, dtype=torch.float64,
                                                                                       requires_grad=True)
    F.linear(xr, wr, br).backward(dy.double())
    dx, dw, db = rg.gemm_pair_ref(dy, w, x, epi2=EPI_ROWSUM, splits=splits)
    _close(dx, xr.grad)
    _close(dw, wr.grad)
    _close(db, br.grad)
    c, rs = rg.gemm_ref(dy, x, True, True, epi=EPI_ROWSUM, splits=splits)
    _close(c, wr.grad)
    _close(rs, br.grad)
    assert rg.gemm_pair_ref(dy, w, x)[2] is None


# ---------------------------------------------------------------------------- floors and mutants
@pytest.mark.parametrize("name", ["bias", "gelu", "dgelu", "swiglu", "dswiglu", "rowsum"])
def test_floor_is_a_rounding(name):
    floor = _case(name)[4]
    print(f"\ngemm floor {name:8s}", {n: f"{x:.2e}" for n, x in floor.items()})
    for n, x in floor.items():
        assert 0 < x < 1e-2, (name, n, x)


def test_gemm256_floor_is_a_rounding():
    """gemm256.hip's epilogue (the pre-activation rounded before GELU / GELU'): two roundings."""
    for name in ("gelu", "dgelu"):
        args, kw, exact, _, _ = _case(name)
        floor = _scores(rg.gemm_ref(*args, emulate=True, tile256=True, **kw), exact)
        print(f"\ngemm256 floor {name:6s}", {n: f"{x:.2e}" for n, x in floor.items()})
        for n, x in floor.items():
            assert 0 < x < 1e-2, (name, n, x)


@pytest.mark.parametrize("mutant", [m for m in rg.GEMM_MUTANTS if m != "trunc"])
def test_mutant_is_caught(mutant):
    name, hits = GEMM_HITS[mutant]
    args, kw, exact, _, floor = _case(name)
    score = _scores(rg.gemm_ref(*args, emulate=True, mutant=mutant, **kw), exact)
    print(f"\ngemm {mutant:22s}", {n: f"{score[n]:.2e} ({score[n] / floor[n]:.0f}x floor)" for n in hits})
    for n in hits:
        assert score[n] >= 9 * floor[n], (mutant, n, score[n], floor[n])


def test_every_mutant_has_a_case():
    assert set(GEMM_HITS) | {"trunc"} == set(rg.GEMM_MUTANTS)


@pytest.mark.parametrize("name", ["bias", "gelu", "dgelu", "swiglu", "dswiglu", "rowsum"])
def test_truncation_shows_in_the_sign_of_the_error(name):
    """``trunc`` moves tile_rel2 by only 2x; its mean signed relative error is -2.8e-3 where
    round-to-nearest gives ~1e-6."""
    args, kw, exact, emu, floor = _case(name)
    bad = rg.gemm_ref(*args, emulate=True, mutant="trunc", **kw)
    score = _scores(bad, exact)
    for n, e in _named(exact).items():
        if n == "aux" and name == "rowsum":
            continue  # 128 values: the mean of so few roundings is not ~0
        good_b, bad_b = rg.signed_bias(_named(emu)[n], e), rg.signed_bias(_named(bad)[n], e)
        print(f"\ntrunc {name:8s} {n:3s} tile_rel2 {score[n] / floor[n]:.1f}x floor; signed bias {good_b:+.2e} -> {bad_b:+.2e}")
        assert bad_b < -1.5e-3
        assert abs(good_b) <= 0.1 * abs(bad_b), (name, n, good_b, bad_b)


# ----------------------------------------------------------------------- the finding behind this
def _glob(x, ref):
    return float((x - ref).abs().max() / ref.abs().max())


def test_global_metric_on_randn_misses_what_tiles_on_structured_inputs_see():
    """On iid randn as test_gemm_gelu_epilogue (256x384x256, bias randn) and test_swiglu_epilogue
    (256x2·384x256) draw it, a GELU epilogue computing SiLU or ReLU, a SwiGLU gate computing
    ReLU(g)·u and a truncated bf16 result all stay under those tests' global 1e-2; on
    gemm_inputs(act=True) with tile_rel2 the wrong activations score >= 9x the floor."""
    g = torch.Generator(device="cpu").manual_seed(4)
    M, N, K = 256, 384, 256
    a, b = torch.randn(M, K, generator=g).bfloat16(), torch.randn(N, K, generator=g).bfloat16()
    bias = torch.randn(N, generator=g).bfloat16()
    kw = dict(bias=bias, epi=EPI_GELU)
    exact = rg.gemm_ref(a, b, False, False, **kw)[0]
    rows = {"correct": _glob(rg.gemm_ref(a, b, False, False, emulate=True, **kw)[0], exact)}
    for m in ("gelu_silu", "gelu_relu", "trunc"):
        rows[m] = _glob(rg.gemm_ref(a, b, False, False, emulate=True, mutant=m, **kw)[0], exact)
    g = torch.Generator(device="cpu").manual_seed(21)
    x, w = torch.randn(M, K, generator=g).bfloat16(), torch.randn(2 * N, K, generator=g).bfloat16()
    sw = rg.gemm_ref(x, w, False, False, epi=EPI_SWIGLU)[0]
    rows["swiglu_relu_gate"] = _glob(rg.gemm_ref(x, w, False, False, epi=EPI_SWIGLU, emulate=True,
                                                 mutant="swiglu_relu_gate")[0], sw)
    # the bias missing in one 16x16 fragment of a K = 1216 product: caught by a hair
    g = torch.Generator(device="cpu").manual_seed(3)
    a2, b2 = torch.randn(M, 1216, generator=g).bfloat16(), torch.randn(N, 1216, generator=g).bfloat16()
    c2 = rg.gemm_ref(a2, b2, False, False, bias=bias)
    bad = rg.gemm_ref(a2, b2, False, False, bias=bias, emulate=True).clone()
    bad[16:32, 16:32] = rg.gemm_ref(a2[16:32], b2[16:32], False, False, emulate=True)
    rows["bias_missing_frag_k1216"] = _glob(bad, c2)
    print("\nglobal metric on randn (bound 1e-2):", {n: f"{v:.1e}" for n, v in rows.items()})
    for m in ("correct", "gelu_silu", "gelu_relu", "trunc", "swiglu_relu_gate"):
        assert rows[m] < 1e-2, (m, rows[m])
    # the same wrong formulas on the structured inputs, per 16x16 tile
    for name, muts in (("gelu", ("gelu_silu", "gelu_relu")), ("swiglu", ("swiglu_relu_gate",))):
        args, ckw, ex, _, floor = _case(name)
        for m in muts:
            s = _scores(rg.gemm_ref(*args, emulate=True, mutant=m, **ckw), ex)["c"]
            print(f"  {m} on gemm_inputs(act=True): tile_rel2 {s:.2e} = {s / floor['c']:.0f}x floor {floor['c']:.2e}")
            assert s >= 9 * floor["c"]
    # truncation biases every value the same way: the sign no test looked at
    tb = rg.signed_bias(rg.gemm_ref(a, b, False, False, emulate=True, mutant="trunc", **kw)[0], exact)
    nb = rg.signed_bias(rg.gemm_ref(a, b, False, False, emulate=True, **kw)[0], exact)
    print(f"  mean signed relative error on randn: truncated {tb:+.2e}, round-to-nearest {nb:+.2e}")
    assert tb < -2e-3 and abs(nb) < 1e-4


# ------------------------------------------------------------------------------------- the helpers
def test_tile_rel2_units():
    ref = torch.ones(32, 48)
    ref[:16, :16] = 100.0
    x = ref.clone()
    x[20, 40] += 0.5  # small beside the tensor's maximum, half of its own tile's
    assert abs(_glob(x, ref) - 0.005) < 1e-9
    assert rg.tile_rel2(x, ref, 16, 16) == 0.5
    assert rg.tile_rel2(x, ref, 32, 48) == 0.005  # one tile: the global metric
    x2 = ref.clone()
    x2[3, 3] += 0.5  # in the large tile: its own maximum is the tensor's
    assert rg.tile_rel2(x2, ref, 16, 16) == 0.005
    assert rg.tile_rel2(x, ref, 24, 32) == 0.5  # ragged last tiles (rows 24..31, columns 32..47)
    z = torch.zeros(16, 16)
    assert rg.tile_rel2(z, z, 16, 16) == 0.0 and rg.tile_rel2(z + 1, z, 16, 16) == float("inf")
    v, vr = torch.ones(40), torch.ones(40)
    v[33] = 1.25  # a [M] vector is one column
    assert rg.tile_rel2(v, vr, 16, 16) == 0.25 and rg.tile_rel2(v[:32], vr[:32], 16, 16) == 0.0


def test_signed_bias_units():
    ref = torch.ones(16, 32, dtype=torch.float64)
    ref[:, 16:] = -2.0
    assert rg.signed_bias(ref * (1 - 1e-3), ref) == pytest.approx(-1e-3)  # towards zero on both signs
    assert rg.signed_bias(ref + 1e-3, ref) == pytest.approx((1e-3 - 0.5e-3) / 2)  # +x on a negative: towards zero
    small = ref.clone()
    small[0, 0] = 0.1  # below a quarter of its tile's maximum: not counted
    x = small.clone()
    x[0, 0] = 0.2
    assert rg.signed_bias(x, small) == 0.0
    g = torch.Generator(device="cpu").manual_seed(0)
    r = torch.randn(64, 64, generator=g).double()
    assert abs(rg.signed_bias(r.bfloat16().double(), r)) < 1e-4
    assert rg.signed_bias(rg._trunc_bf16(r), r) == pytest.approx(-2.8e-3, abs=4e-4)


@pytest.mark.parametrize("act", [False, True])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_generator_conditions(layout, act):
    a_km, b_kn = LAYOUTS[layout]
    M, N, K = 192, 160, 256
    d = rg.gemm_inputs(M, N, K, a_km, b_kn, seed=9, act=act)
    assert d["a"].shape == ((K, M) if a_km else (M, K)) and d["b"].shape == ((K, N) if b_kn else (N, K))
    assert all(t.dtype == torch.bfloat16 and t.is_contiguous() for t in d.values())
    again = rg.gemm_inputs(M, N, K, a_km, b_kn, seed=9, act=act)
    assert all(torch.equal(d[n], again[n]) for n in d)
    c = rg.gemm_ref(d["a"], d["b"], a_km, b_kn)
    std = rg._tiles(c, 16, 16).std(-1)  # per 16x16 fragment
    assert float(std.min()) > 0
    # neighbouring fragments differ by >= 4x in scale (2x margin for the sample of 256 values)
    for r in (std[1:] / std[:-1], std[:, 1:] / std[:, :-1]):
        assert float(torch.maximum(r, 1 / r).min()) >= 2.0
    if act:
        assert float(((std >= 0.5) & (std <= 3.0)).double().mean()) >= 0.25
        assert float(std.max() / std.min()) <= 16 * 16 * 2
    else:
        assert float(std.max() / std.min()) >= 1e3  # three decades
    # the first and the last 32 k carry 4x the weight: 16x the variance of a middle step's product
    A, B = rg._mats(d["a"], d["b"], a_km, b_kn)
    edge = rg._tiles(A[:, :32] @ B[:32], 16, 16).std(-1) / rg._tiles(A[:, 64:96] @ B[64:96], 16, 16).std(-1)
    assert 2.5 < float(edge.median()) < 6.5
    # the row sums do not cancel: |Σ_k A| is of the order of K·|μ|, not sqrt(K)
    noise = A.std(1) * K ** 0.5
    assert float((A.sum(1).abs() / noise).median()) > 2.0
    # bias: distinct per column and comparable with the column block's product
    bias = d["bias"].double()
    assert bias.unique().numel() >= 0.75 * N
    unit = c / rg.block_scales(M, rg._SCALES[act][0])[:, None]  # every row at the unit row scale
    ratio = bias.abs() / unit.std(0)
    # 0.5 .. 1.5 of the design value; a column's realised deviation (64 heavy k) is within ~1.7x of it
    assert 0.25 < float(ratio.min()) and float(ratio.max()) < 2.5 and 0.8 < float(ratio.median()) < 1.25
    for n in ("aux", "aux2"):
        s = rg._tiles(d[n].double(), 16, 16).std(-1)
        assert float(((s >= 0.5) & (s <= 3.0)).double().mean()) >= 0.25


def test_generator_rejects_too_few_bending_fragments(monkeypatch):
    monkeypatch.setitem(rg._SCALES, True, ((16.0, 1 / 64), (16.0, 1 / 64, 16.0)))
    with pytest.raises(AssertionError, match="fragments"):
        rg.gemm_inputs(64, 48, 128, False, False, seed=1, act=True)
