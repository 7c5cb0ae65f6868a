"""CPU proof that the row-wise loss tests (test_gpu_xent_paths.py) can fail, and that their
reference is right: tests/refmath_xent.py against a second derivation (fp64 autograd of
``F.cross_entropy``), the conditions its inputs must meet, its floors, and every deliberately
wrong "mutant" of the kernels' formulas, where

    floor = score(emulated reference, fp64 reference)      (what a correct kernel may show)
    tol   = 3 x floor                                       (the GPU tests' bound; fp32 gradient:
                                                             3 x max(floor, derived floor))
    score(emulated mutant, fp64 reference) >= 3 x tol

on every output the mutant is declared to move; score = ``row_abs`` for loss and lse, ``elem_rel``
for the gradient.  Shapes: the smallest of each kind test_gpu_xent_paths.py uses — V = 5 (all
scalar; V = 1 has one column with p = 1 and a zero gradient, nothing for a mutant to move),
23 (head, two chunks, tail), 2053 (chunk 256 wraps to lane 0) and 16385 (past the first fused
instance).  Run with ``-s`` to print floor, tol and the scores."""
import math

import pytest
import torch
import torch.nn.functional as F

import refmath_xent as rx

DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
PHASE = {"bf16": 3, "f16": 3, "f32": 1}
G = 2.5  # grad_out
SHAPES = (5, 23, 2053, 16385)
CHUNKED = ("drop_chunk", "onehot_shift")  # need a chunk: not at V = 5

# mutant -> the outputs it must move by >= 3 x tol
XENT_HITS = {
    "drop_head": ("loss", "lse", "dx"),
    "drop_tail": ("loss", "lse", "dx"),
    "drop_chunk": ("loss", "lse", "dx"),
    "merge_no_rescale": ("loss", "lse", "dx"),
    "onehot_shift": ("dx",),
    "onehot_missing_scalar": ("dx",),
    "ignored_row_scaled": ("dx",),
    "neighbour_target": ("loss", "dx"),
    "ln_for_log2": ("loss", "lse", "dx"),
    "scale_twice": ("dx",),
    "grad_unscaled_onehot": ("dx",),
}


def _scores(got, exact, dtype):
    return {"loss": rx.row_abs(got[0], exact[0]), "lse": rx.row_abs(got[1], exact[1]),
            "dx": rx.elem_rel(got[2], exact[2], dtype)}


_CASES = {}


def _case(dt, V):
    key = (dt, V)
    if key not in _CASES:
        dtype = DT[dt]
        d = rx.xent_inputs(rx.default_rows(V, 0), V, seed=V, dtype=dtype, phase=PHASE[dt])
        scale = G / d["n_valid"]
        kw = dict(dtype=dtype, part=d["part"])
        exact = rx.xent_ref(d["x"], d["target"], scale, rx.IGNORE, **kw)
        emu = rx.xent_ref(d["x"], d["target"], scale, rx.IGNORE, emulate=True, **kw)
        floor = _scores(emu, exact, dtype)
        bound = dict(floor)
        if dtype == torch.float32:
            bound["dx"] = max(floor["dx"], rx.derived_floor32(d["x"], exact[1], d["target"]))
        _CASES[key] = (d, scale, exact, floor, bound)
    return _CASES[key]


# ------------------------------------------------------- the reference against a second derivation
@pytest.mark.parametrize("V", SHAPES)
def test_reference_matches_cross_entropy_autograd(V):
    d, scale, (loss, lse, dx), _, _ = _case("bf16", V)
    rows = (d["target"] == rx.IGNORE) | ((d["target"] >= 0) & (d["target"] < V))  # F.cross_entropy rejects the rest
    x = d["x"][rows].double().requires_grad_()
    tgt = d["target"][rows]
    want = F.cross_entropy(x, tgt, ignore_index=rx.IGNORE, reduction="none")
    (want.sum() * scale).backward()
    assert float((loss[rows] - want.detach()).abs().max()) <= 1e-12 * float(want.detach().abs().max())
    assert float((lse[rows] - torch.logsumexp(x.detach(), -1)).abs().max()) <= 1e-12 * float(lse[rows].abs().max())
    err = (dx[rows] - x.grad).abs()
    assert bool((err <= 1e-12 * x.grad.abs() + 1e-300).all()), float(err.max())  # per element, -inf columns included
    oor = ~rows
    assert bool(oor.any()) and bool(torch.isnan(loss[oor]).all()) and bool((dx[oor] == 0).all())
    assert bool(torch.isfinite(lse).all())


# ---------------------------------------------------------------------- conditions on the inputs
def _check_inputs(d, V, dtype):
    x, tgt, part, N = d["x"].double(), d["target"], d["part"], d["x"].shape[0]
    mass = torch.exp(x.gather(1, d["sentinel"][:, None]).squeeze(1) - torch.logsumexp(x, -1))
    assert float(mass.min()) >= 0.25, float(mass.min())
    if V > 1:
        assert float(mass.max()) <= 0.75, float(mass.max())  # the one-hot's cancellation stays mild
    esize = torch.finfo(dtype).bits // 8
    feas = rx.feasible_kinds(part, V, esize)
    assert set(d["kinds"]) == set(feas), sorted(set(feas) - set(d["kinds"]))
    heads = {int(h) for h in part[:, 0]}
    assert heads == {min(h, V) for h in range(16 // esize)}  # the odd stride runs through every head length
    no_loss = sum(c in ("ignore", "oor") for c in d["classes"])
    assert 0 < no_loss <= N // 4, no_loss
    want = {"sentinel", "ignore", "oor"}
    if any(int(h) > 0 for h in part[:, 0]):
        want.add("head")
    if any(int(t0) < V for t0 in part[:, 2]):
        want.add("tail")
    if any(int(nv) > 0 for nv in part[:, 1]):
        want |= {"d0", "d7"}
    assert set(d["classes"]) == want, (set(d["classes"]), want)
    oor = [int(t) for t, c in zip(tgt, d["classes"]) if c == "oor"]
    assert set(oor) == {V, -1}
    if V >= 23:
        band = d["band"]
        assert int(band.any(1).sum()) >= 3
        r = int(band.any(1).nonzero()[0])
        head = int(part[r, 0])
        assert bool(band[r, head - 1]) and bool(band[r, head:head + 8].all())  # a head column and a whole chunk
        assert bool(torch.isinf(d["x"][band]).all())


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("V", SHAPES)
def test_input_conditions(dt, V):
    d = _case(dt, V)[0]
    _check_inputs(d, V, DT[dt])
    again = rx.xent_inputs(rx.default_rows(V, 0), V, seed=V, dtype=DT[dt], phase=PHASE[dt])
    assert torch.equal(again["x"], d["x"]) and torch.equal(again["target"], d["target"])


@pytest.mark.parametrize("dt,phase", [("bf16", 0), ("f16", 5)])
def test_every_sentinel_position_exists_at_the_largest_vocabulary(dt, phase):
    """V = 65550 (2-byte types: head 7 + 8192 chunks + tail 7 in some row): every position of
    ``sentinel_kinds`` is used, the edges of all four fused instances included."""
    V = 65550
    dtype = DT[dt]
    d = rx.xent_inputs(rx.default_rows(V, 0), V, seed=7, dtype=dtype, phase=phase)
    _check_inputs(d, V, dtype)
    kinds = set(rx.sentinel_kinds(torch.finfo(dtype).bits // 8))
    assert set(d["kinds"]) == kinds, sorted(kinds - set(d["kinds"]))
    for r, k in enumerate(d["kinds"]):  # the named column is where the name says
        head, nv, tail0 = (int(v) for v in d["part"][r])
        s = int(d["sentinel"][r])
        if k.startswith("edge"):
            nvi, side = k[4:].split("_")
            chunk = (s - head) // 8
            assert chunk == int(nvi) * 256 - (1 if side == "last" else 0) and chunk % 256 == (255 if side == "last" else 0)
        elif k.startswith("head"):
            assert s < head
        elif k.startswith("tail"):
            assert tail0 <= s < V
        elif k == "last_col":
            assert s == V - 1


@pytest.mark.parametrize("V", [1, 9])
def test_small_vocabularies_build(V):
    for dt in DT:
        d = rx.xent_inputs(rx.default_rows(V, 0), V, seed=V, dtype=DT[dt], phase=1)
        _check_inputs(d, V, DT[dt])


def test_partition_is_the_kernels_arithmetic():
    part = rx.partition(9, 23, rx.row_stride(23), 3, 2)
    for r in range(9):
        byte = (3 + r * 33) * 2
        head = ((16 - byte % 16) % 16) // 2
        assert tuple(int(v) for v in part[r]) == (head, (23 - head) // 8, head + (23 - head) // 8 * 8)
    assert rx.row_stride(23) % 2 == 1 and rx.row_stride(16384) % 2 == 1
    part = rx.partition(4, 5, rx.row_stride(5), 1, 2)
    assert int(part[0, 0]) == 5 and int(part[0, 1]) == 0  # head capped at V: an all-scalar row
    ln = rx.lanes(rx.partition(1, 2100, 2109, 2, 2), 2100)[0]
    assert ln[:6].tolist() == [0, 1, 2, 3, 4, 5] and int(ln[6]) == 0 and int(ln[6 + 8 * 256]) == 0 and int(ln[6 + 8 * 255]) == 255


# ---------------------------------------------------------------------------- floors and mutants
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("V", SHAPES)
def test_floor_is_a_rounding(dt, V):
    _, _, _, floor, bound = _case(dt, V)
    print(f"\nxent floor {dt:4s} V={V:<6d}", {n: f"{x:.2e}" for n, x in floor.items()},
          "tol", {n: f"{3 * x:.2e}" for n, x in bound.items()})
    eps = torch.finfo(DT[dt]).eps  # one ulp relative to a power of two; relative to an element: eps/2 .. eps
    if dt != "f32":
        assert 0.25 * eps <= floor["dx"] <= 2 * eps, (floor["dx"], eps)  # half an ulp .. two ulps
    else:
        assert 0 < floor["dx"] < 1e-3 and bound["dx"] < 1e-3
    assert floor["lse"] < 1e-3 and floor["loss"] < 1e-3  # nats, at |lse| up to ~500: fp32 roundings


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("V", SHAPES)
@pytest.mark.parametrize("mutant", rx.XENT_MUTANTS)
def test_mutant_is_caught(mutant, V, dt):
    if V == 5 and mutant in CHUNKED:
        return  # no chunk to drop or to shift in
    d, scale, exact, floor, bound = _case(dt, V)
    got = rx.xent_ref(d["x"], d["target"], scale, rx.IGNORE, dtype=DT[dt], part=d["part"], emulate=True, mutant=mutant)
    score = _scores(got, exact, DT[dt])
    hits = XENT_HITS[mutant]
    print(f"\nxent {dt:4s} V={V:<6d} {mutant:22s}",
          {n: f"{score[n]:.2e} (tol {3 * bound[n]:.2e}, {score[n] / (3 * bound[n]):.0f}x)" for n in hits})
    for n in hits:
        assert score[n] >= 9 * bound[n], (mutant, n, score[n], bound[n])


def test_every_mutant_has_its_outputs():
    assert set(XENT_HITS) == set(rx.XENT_MUTANTS)
    assert {"drop_head", "drop_tail", "drop_chunk", "merge_no_rescale", "onehot_shift", "onehot_missing_scalar",
            "ignored_row_scaled", "neighbour_target", "ln_for_log2", "scale_twice",
            "grad_unscaled_onehot"} <= set(rx.XENT_MUTANTS)


# ----------------------------------------------------------------------- the finding behind this
def test_tensor_metric_on_randn_misses_what_elements_on_structured_rows_see():
    """On ``randn·3`` rows of 50257 columns as test_cross_entropy_matches_reference draws them, a
    dropped tail, a dropped last chunk and a softmax part that is 10 % short at every column but
    the target all stay under that test's bounds (1e-4 relative on the lse, 2e-2 of the tensor's
    maximum on the gradient); per element the last is 25 bf16 roundings off."""
    g = torch.Generator(device="cpu").manual_seed(50257)
    N, V = 8, 50257
    x = (torch.randn(N, V, generator=g) * 3).bfloat16()
    tgt = torch.randint(0, V, (N,), generator=g)
    part = rx.partition(N, V, V, 0, 2)
    kw = dict(dtype=torch.bfloat16, part=part)
    loss, lse, dx = rx.xent_ref(x, tgt, 1.0 / N, rx.IGNORE, **kw)
    for m in ("drop_tail", "drop_chunk"):
        bad = rx.xent_ref(x, tgt, 1.0 / N, rx.IGNORE, emulate=True, mutant=m, **kw)
        rel = float(((bad[1] - lse).abs() / lse.abs()).max())
        print(f"\n{m} on randn: lse off by {rel:.1e} relative")
        assert rel < 1e-4
    hot = torch.zeros_like(dx, dtype=torch.bool).scatter_(1, tgt[:, None], True)
    short = torch.where(hot, dx, 0.9 * dx)
    glob = float((short - dx).abs().max() / dx.abs().max())
    elem = rx.elem_rel(short, dx, torch.bfloat16)
    print(f"softmax part 10 % short on randn: {glob:.1e} of the tensor's maximum, per element {elem:.2f}")
    assert glob < 2e-2
    assert elem >= 0.0999


# ------------------------------------------------------------------------------------- the helpers
def test_metric_units():
    ref = torch.tensor([[1.0, 1e-6, 0.0, -2.0]], dtype=torch.float64)
    x = ref.clone()
    x[0, 1] = 1.5e-6  # small beside the row's maximum, half of itself
    assert rx.elem_rel(x, ref, torch.bfloat16) == pytest.approx(0.5)
    tiny = torch.finfo(torch.float16).tiny
    x = ref.clone()
    x[0, 2] = tiny / 4  # a zero reference: measured against the smallest normal
    assert rx.elem_rel(x, ref, torch.float16) == pytest.approx(0.25)
    x[0, 0] = math.nan
    assert rx.elem_rel(x, ref, torch.float16) == math.inf
    r = torch.tensor([1.0, math.nan, 3.0], dtype=torch.float64)
    assert rx.row_abs(torch.tensor([1.5, 7.0, 3.0]), r) == 0.5  # a NaN reference row does not count
    assert rx.row_abs(torch.tensor([math.nan, 7.0, 3.0]), r) == math.inf
    assert rx._next_up(1.0, torch.bfloat16) == 1.0 + 2.0 ** -7 and rx._next_up(-1.0, torch.float16) == -1.0 + 2.0 ** -11
