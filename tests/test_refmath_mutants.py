"""CPU proof that the tile-wise GPU tests (test_gpu_attn_paths.py, test_gpu_norm_paths.py) can
fail: on the structured inputs of tests/refmath.py every deliberately wrong "mutant" of the
attention / norm formulas scores at least 3x the tolerance those tests use, where

    floor = tile_rel(emulated reference, fp64 reference)      (what a correct kernel may show)
    tol   = 3 x floor                                          (the GPU tests' bound)
    score = tile_rel(emulated mutant, fp64 reference) >= 3 x tol

on every output the mutant is expected to move.  Run with ``-s`` to print the scores."""
import pytest
import torch

import refmath as rm

SCALE = 0.125
ATTN_OUT = ("out", "lse", "dq", "dk", "dv")
NORM_OUT = ("y", "sum", "dx", "ddelta", "dw", "db")

# mutant -> the outputs it must move by >= 3 x tol
ATTN_HITS = {
    "mask_wide": ("out", "dq", "dk", "dv"),
    "skip_diag": ("out", "dk", "dv"),
    "delta_dropped": ("dq", "dk"),
    "delta_tail": ("dq", "dk"),
    "dkdv_tail": ("dk", "dv"),
    "gqa_mod": ("out", "dq", "dk", "dv"),
    "rope_kmod64": ("out", "dq", "dk", "dv"),
    "dq_norot": ("dq",),
    "dk_norot": ("dk",),
    "dk_noscale": ("dk",),
}
NORM_HITS = {
    "no_mean_g": ("dx",),
    "no_proj": ("dx",),
    "half_mean_g": ("dx",),
    "half_mean_gx": ("dx",),
    "no_eps": ("y", "dx"),
    "neighbour_stats": ("dx", "dw"),
    "no_dres": ("dx", "ddelta"),
    "dw_tail": ("dw", "db"),
    "y_unrounded_sum": ("y",),
}
# RMSNorm has no mean(g) term, and without centring the rounding of the stored sum is no larger
# than the rounding of y itself (no cancellation): those mutants do not exist / cannot show there
RMS_SKIP = ("no_mean_g", "half_mean_g", "y_unrounded_sum")


def _attn_scores(x, ref):
    return {n: (rm.max_abs(a, b) if n == "lse" else rm.tile_rel(a, b, 32)) for n, a, b in zip(ATTN_OUT, x, ref)}


@pytest.fixture(scope="module")
def attn_case():
    """causal GQA with RoPE, B1 H4 Hkv2 T256: the smallest shape with rows >= 128, a last 128-query
    block that is not the whole sequence, keys past one 64-key tile and two key/value heads."""
    B, H, Hkv, T = 1, 4, 2, 256
    rope = rm.rope_tables_ref(T)
    q, k, v = rm.attn_inputs(B, H, Hkv, T, seed=1)
    out0, _ = rm.attn_ref(q, k, v, None, True, SCALE, rope=rope)
    do = rm.attn_do(out0, seed=2)
    exact = rm.attn_ref(q, k, v, do, True, SCALE, rope=rope)
    emu = rm.attn_ref(q, k, v, do, True, SCALE, rope=rope, emulate=True, gsplit=True)
    return (q, k, v, do, rope), exact, _attn_scores(emu, exact)


def test_attention_floor_is_a_bf16_rounding(attn_case):
    _, _, floor = attn_case
    print("\nattention floor", {n: f"{x:.2e}" for n, x in floor.items()})
    for n in ("out", "dq", "dk", "dv"):
        assert 1e-3 < floor[n] < 2.5e-2, (n, floor[n])
    assert floor["lse"] < 0.1  # nats; the rotated q / k are rounded to bf16 and scores reach tens of nats


@pytest.mark.parametrize("mutant", rm.ATTN_MUTANTS)
def test_attention_mutant_is_caught(attn_case, mutant):
    (q, k, v, do, rope), exact, floor = attn_case
    got = rm.attn_ref(q, k, v, do, True, SCALE, rope=rope, emulate=True, gsplit=True, mutant=mutant)
    score = _attn_scores(got, exact)
    print(f"\nattn {mutant:14s}", {n: f"{score[n]:.2e} ({score[n] / max(floor[n], 1e-300):.0f}x floor)"
                                   for n in ATTN_HITS[mutant]})
    for n in ATTN_HITS[mutant]:
        assert score[n] >= 9 * floor[n], (mutant, n, score[n], floor[n])


def test_attention_global_metric_misses_what_tiles_see():
    """The finding behind this module, on iid randn at causal B2 H2 T1024 as
    test_flash_forward_backward draws it: with δ zeroed for the last 128 queries, or with the last
    64 queries skipping their diagonal key tile, dk stays under that test's global 3e-2 bound while
    its worst 32-row tile is off by 20 % / 100 %."""
    g = torch.Generator(device="cpu").manual_seed(1026)
    q, k, v, do = (torch.randn(2, 2, 1024, 64, generator=g).bfloat16() for _ in range(4))
    dk = rm.attn_ref(q, k, v, do, True, SCALE)[3]
    for mutant, tile in (("delta_tail", 0.1), ("skip_diag", 0.9)):
        bad = rm.attn_ref(q, k, v, do, True, SCALE, mutant=mutant)[3]
        glob = float((bad - dk).abs().max() / dk.abs().max())
        print(f"\n{mutant} dk: global {glob:.2e}, worst tile {rm.tile_rel(bad, dk, 32):.2e}")
        assert glob < 3e-2
        assert rm.tile_rel(bad, dk, 32) > tile


@pytest.mark.parametrize("gqa", [False, True])
@pytest.mark.parametrize("use_rope", [False, True])
@pytest.mark.parametrize("t0", [1, 31, 32, 64, 127, 128, 129, 300])
def test_poisoned_future_exact_conditions(t0, use_rope, gqa):
    """fp64 reference on the poisoned twin: gradients at positions >= t0 are exactly zero, and
    rows < t0 of out, lse and dq are bit-equal to the unpoisoned run (tolerance zero: the masked
    scores are -inf, their probabilities exactly 0)."""
    B, H, Hkv, T = 1, (4 if gqa else 2), 2, 384
    rope = rm.rope_tables_ref(T) if use_rope else None
    (q, k, v), (_, kp, vp) = rm.poisoned_inputs(B, H, Hkv, T, t0, seed=t0, scale=SCALE, rope=rope)
    out0, _ = rm.attn_ref(q, k, v, None, True, SCALE, rope=rope)
    do = rm.attn_do(out0, seed=3)
    dop = do.clone()
    dop[:, :, t0:] = 0
    clean = rm.attn_ref(q, k, v, do, True, SCALE, rope=rope)
    out, lse, dq, dk, dv = rm.attn_ref(q, kp, vp, dop, True, SCALE, rope=rope)
    # the recipe's premise: every poisoned key beats every legitimate score of its row by 20 nats
    qr, kr = (rm.rot(t.double(), rope[0].double(), rope[1].double()) if use_rope else t.double() for t in (q, kp))
    s = SCALE * (qr @ kr.repeat_interleave(H // Hkv, 1).transpose(-1, -2))
    assert float(s[..., t0:].amin() - s[..., :t0].amax()) >= 20.0
    assert torch.isfinite(out).all() and torch.isfinite(lse).all()
    for n, t in (("dq", dq), ("dk", dk), ("dv", dv)):
        assert (t[:, :, t0:] == 0).all(), n
    for n, a, b in (("out", out, clean[0]), ("lse", lse.unsqueeze(-1), clean[1].unsqueeze(-1)), ("dq", dq, clean[2])):
        assert torch.equal(a[:, :, :t0], b[:, :, :t0]), n


def test_poisoned_future_shows_one_key_too_many():
    """What the poison is for: with t0 = 129 the mutant that shows key i + 1 to rows >= 128 moves
    row 128's output by the poisoned values' magnitude, not by a rounding."""
    t0, T = 129, 384
    (q, k, v), (_, kp, vp) = rm.poisoned_inputs(1, 2, 2, T, t0, seed=5, scale=SCALE)
    clean, _ = rm.attn_ref(q, k, v, None, True, SCALE)
    good, _ = rm.attn_ref(q, kp, vp, None, True, SCALE)
    bad, _ = rm.attn_ref(q, kp, vp, None, True, SCALE, mutant="mask_wide")
    assert rm.tile_rel(good, clean, 32, valid=t0) == 0.0
    assert rm.tile_rel(bad, clean, 32, valid=t0) > 100


def _norm_scores(x, ref):
    return {n: rm.tile_rel(a, b, 1) for n, a, b in zip(NORM_OUT, x, ref) if b is not None}


_NORM_CASES = {}


def _norm_case(kind):
    """13 rows x 64 columns, bf16, with the residual: 4-row workgroups with one row in the last."""
    if kind not in _NORM_CASES:
        rms = kind == "rms"
        eps = 1e-6 if rms else 1e-5
        fn = rm.rms_ref if rms else rm.ln_ref
        d = rm.norm_inputs(13, 64, seed=4, dtype=torch.bfloat16, eps=eps, rms=rms)
        args = (d["x"], d["delta"], d["w"], d["b"], d["dy"], d["ds"], eps)
        exact = fn(*args)
        _NORM_CASES[kind] = (fn, args, exact, _norm_scores(fn(*args, emulate=True), exact))
    return _NORM_CASES[kind]


@pytest.mark.parametrize("kind", ["ln", "rms"])
def test_norm_floor_is_a_rounding(kind):
    floor = _norm_case(kind)[3]
    print(f"\nnorm floor {kind}", {n: f"{x:.2e}" for n, x in floor.items()})
    for n, x in floor.items():
        assert x < 1e-2, (n, x)


@pytest.mark.parametrize("kind,mutant", [("ln", m) for m in rm.NORM_MUTANTS] +
                         [("rms", m) for m in rm.NORM_MUTANTS if m not in RMS_SKIP])
def test_norm_mutant_is_caught(kind, mutant):
    fn, args, exact, floor = _norm_case(kind)
    score = _norm_scores(fn(*args, emulate=True, mutant=mutant, rpb=4), exact)
    hits = [n for n in NORM_HITS[mutant] if n in score]
    print(f"\n{kind:3s} {mutant:16s}",
          {n: f"{score[n]:.2e} ({score[n] / max(floor[n], 1e-300):.0f}x floor)" for n in hits})
    assert hits
    for n in hits:
        assert score[n] >= 9 * floor[n] and score[n] > 0, (mutant, n, score[n], floor[n])


def test_norm_global_metric_on_randn_misses_a_whole_term():
    """The finding behind the generators: on test_layer_norm_fwd_bwd's own inputs (iid zero-mean
    dy, C = 768, bf16) a backward without mean(g·dy) stays under that test's 4e-2 bound on dx."""
    g = torch.Generator(device="cpu").manual_seed(768)
    rows, C = 333, 768
    x = (torch.randn(rows, C, generator=g) * 2 + 0.5).bfloat16()
    torch.randn(rows, C, generator=g)
    w = (1 + 0.1 * torch.randn(C, generator=g)).bfloat16()
    b = (0.1 * torch.randn(C, generator=g)).bfloat16()
    dy = torch.randn(rows, C, generator=g).bfloat16()
    dx = rm.ln_ref(x, None, w, b, dy, None, 1e-5)[2]
    bad = rm.ln_ref(x, None, w, b, dy, None, 1e-5, mutant="no_mean_g")[2]
    glob = float((bad - dx).abs().max() / dx.abs().max())
    print(f"\nno_mean_g on randn: global {glob:.2e}")
    assert glob < 4e-2


def test_tile_rel_units():
    ref = torch.zeros(1, 1, 64, 4)
    ref[0, 0, :32] = 100.0
    ref[0, 0, 32:] = 1.0
    x = ref.clone()
    x[0, 0, 40, 1] += 0.5  # small beside the tensor's maximum, half of its own tile's
    assert abs(float((x - ref).abs().max() / ref.abs().max()) - 0.005) < 1e-6
    assert rm.tile_rel(x, ref, 32) == 0.5
    assert rm.tile_rel(x, ref, 32, valid=40) == 0.0
    assert rm.tile_rel(x, ref, 40) == 0.5  # a ragged last tile (rows 40 .. 63)
    z = torch.zeros(2, 3)
    assert rm.tile_rel(z, z, 1) == 0.0 and rm.tile_rel(z + 1, z, 1) == float("inf")


def test_rope_tables_match_the_package():
    from nbdistributed_amd.ops.llama import rope_tables

    a, b = rope_tables(384, 64, 10000.0, "cpu"), rm.rope_tables_ref(384)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
