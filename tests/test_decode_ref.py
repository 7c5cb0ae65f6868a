"""CPU: the references of the per-token kernels (tests/refmath_decode.py).  The fp64 formulas
against the package's fp32 ``ops.decode_attention_reference`` / ``ops.linear_small_reference``,
and the proof that the GPU tests built on them (tests/test_gpu_decode_paths.py, bound 3 x floor
per head row / per 16 x 16 tile) can fail: on the very inputs those tests use, every wrong
"mutant" of the formulas scores >= 9 x floor on each output it must move, where floor =
tile_rel(emulated reference, fp64 reference).  ``-s`` prints the scores."""
import functools

import pytest
import torch

import refmath as rm
import refmath_decode as rd
from nbdistributed_amd import ops

SCALE = rd.SCALE

# mutant -> the outputs it must move by >= 9 x floor (k_cache only where the case rotates)
DECODE_HITS = {
    "mask_plus1": ("out",),
    "new_key_dropped": ("out",),
    "stale_new_key": ("out",),
    "rope_prev_pos": ("out", "k_cache"),
    "rope_sign": ("out", "k_cache"),
    "rope_k_unrotated": ("out", "k_cache"),
    "gqa_mod": ("out",),
    "chunk_head_dropped": ("out",),
    "merge_unweighted": ("out",),
    "empty_chunk_live": ("out",),
}
ROPE_MUTANTS = ("rope_prev_pos", "rope_sign", "rope_k_unrotated")
CHUNK_MUTANTS = ("chunk_head_dropped", "merge_unweighted", "empty_chunk_live")

# the GPU test's cases the mutants are proven on (with their loud poison); a mutant runs on every case that
# can show it (a split for the chunk mutants, RoPE for the rope mutants, two kv heads for gqa_mod)
DECODE_CASES = ("group G3 T640 rope", "group G8 T640 plain", "group G5 T320 rope", "sweep kv513 G3 launch 1",
                "sweep kv1024 G6 launch 4")


def _dscores(got, exact, H):
    return {"out": rm.tile_rel(rd.decode_per_head(got[0], H), rd.decode_per_head(exact[0], H), 1),
            "k_cache": rm.tile_rel(got[1], exact[1], 1), "v_cache": rm.tile_rel(got[2], exact[2], 1)}


@functools.lru_cache(maxsize=None)
def _decode_case(name):
    w = name.split()
    if w[0] == "group":
        G, Tmax, use_rope = int(w[1][1:]), int(w[2][1:]), w[3] == "rope"
        H, Hkv, pos, (qkv, kc, vc) = rd.group_case(G, Tmax, "loud", use_rope)
    else:
        Tmax, G, launch = int(w[1][2:]), int(w[2][1:]), int(w[4])
        assert rd.SWEEP_POISON[launch % 3] == "loud"
        H, Hkv, use_rope, pos = G, 1, True, rd.sweep_positions(Tmax, launch)
        qkv, kc, vc = rd.decode_poison(rd.sweep_history(Tmax, G), pos, "loud")
    rope = rm.rope_tables_ref(Tmax) if use_rope else None
    nch, chunk = rd.decode_plan(len(pos) * Hkv, Tmax)
    exact = rd.decode_ref(qkv, kc, vc, pos, H, SCALE, rope)
    emu = rd.decode_ref(qkv, kc, vc, pos, H, SCALE, rope, emulate=True)
    return (qkv, kc, vc, pos, H, Hkv, rope, nch, chunk), exact, _dscores(emu, exact, H)


@pytest.mark.parametrize("name", DECODE_CASES)
def test_decode_floor_is_a_bf16_rounding(name):
    (_, _, _, _, _, _, rope, _, _), _, floor = _decode_case(name)
    print(f"\ndecode floor {name}", {n: f"{x:.2e}" for n, x in floor.items()})
    # one rounding of the output to bf16: 2^-9 = 1.95e-3 of the element, up to ~3x that of the
    # head row's maximum once the rotated k's rounding has moved the scores (measured 2.7e-3 .. 5.3e-3)
    assert 1e-3 < floor["out"] < 1e-2, floor
    if rope is not None:
        assert 1e-3 < floor["k_cache"] < 4e-3, floor  # the rotated k rounded to bf16: at most 2^-8
    else:
        assert floor["k_cache"] == 0.0  # k is copied
    assert floor["v_cache"] == 0.0  # v is copied


@pytest.mark.parametrize("mutant", rd.DECODE_MUTANTS)
def test_decode_mutant_is_caught(mutant):
    ran = 0
    for name in DECODE_CASES:
        (qkv, kc, vc, pos, H, Hkv, rope, nch, chunk), exact, floor = _decode_case(name)
        if (mutant in ROPE_MUTANTS and rope is None) or (mutant in CHUNK_MUTANTS and nch == 1) or (
                mutant == "gqa_mod" and (Hkv == 1 or H == Hkv)):
            continue
        ran += 1
        got = rd.decode_ref(qkv, kc, vc, pos, H, SCALE, rope, emulate=True, mutant=mutant, chunk=chunk)
        score = _dscores(got, exact, H)
        print(f"\ndecode {mutant:18s} {name}",
              {n: f"{score[n]:.2e} (floor {floor[n]:.2e})" for n in DECODE_HITS[mutant]})
        for n in DECODE_HITS[mutant]:
            assert score[n] >= 9 * floor[n] and score[n] > 0, (mutant, name, n, score[n], floor[n])
    assert ran >= 2, (mutant, ran)


def test_decode_reference_leaves_other_rows_alone():
    (qkv, kc, vc, pos, H, Hkv, rope, _, _), exact, _ = _decode_case(DECODE_CASES[0])
    for b, p in enumerate(pos):
        for new, old in ((exact[1], kc), (exact[2], vc)):
            assert torch.equal(new[b, :, :p], old[b, :, :p].double())
            assert torch.equal(new[b, :, p + 1:], old[b, :, p + 1:].double())
        assert torch.equal(exact[2][b, :, p], qkv[b, (H + Hkv) * 64:].double().reshape(Hkv, 64))


def test_sweep_positions_cover_every_position():
    for kv in (512, 513, 1024):
        n = -(-kv // rd.SWEEP_B)
        seen = set()
        for launch in range(n):
            seen.update(rd.sweep_positions(kv, launch))
        assert seen == set(range(kv)), kv


def test_decode_plan_splits_above_512_keys():
    assert rd.decode_plan(64, 512) == (1, 512)
    assert rd.decode_plan(64, 513) == (3, 192)
    assert rd.decode_plan(64, 1024) == (4, 256)
    assert rd.decode_plan(24, 640) == (3, 224)
    assert rd.decode_plan(4, 1024) == (4, 256)


@pytest.mark.parametrize("use_rope", [False, True])
@pytest.mark.parametrize("poison", ["loud", "huge", "nan"])
def test_package_decode_reference_matches_fp64(use_rope, poison):
    """``ops.decode_attention_reference`` on fp32 inputs: the fp64 formula to fp32 accuracy, the
    caches written the same way, every other row untouched bit for bit — whatever the rows past
    ``pos`` hold."""
    Tmax, G = 320, 3
    H, Hkv, pos, (qkv, kc, vc) = rd.group_case(G, Tmax, poison, use_rope)
    qkv, kc, vc = qkv.float(), kc.float(), vc.float()
    rope = rm.rope_tables_ref(Tmax) if use_rope else None
    exact = rd.decode_ref(qkv, kc, vc, pos, H, SCALE, rope)
    k2, v2 = kc.clone(), vc.clone()
    out = ops.decode_attention_reference(qkv, k2, v2, torch.tensor(pos), H, SCALE, rope)
    assert out.dtype == qkv.dtype and out.shape == (len(pos), H * 64)
    assert torch.isfinite(out).all()
    assert rm.tile_rel(rd.decode_per_head(out, H), rd.decode_per_head(exact[0], H), 1) < 1e-5
    for b, p in enumerate(pos):
        assert rm.tile_rel(k2[b, :, p], exact[1][b, :, p], 1) < 1e-6
        assert torch.equal(v2[b, :, p].double(), exact[2][b, :, p])
        for new, old in ((k2, kc), (v2, vc)):
            assert torch.equal(new[b, :, p + 1:].view(torch.int32), old[b, :, p + 1:].view(torch.int32))
            assert torch.equal(new[b, :, :p], old[b, :, :p])
    a = ops.decode_attention(qkv, kc.clone(), vc.clone(), torch.tensor(pos), H, SCALE, rope)  # the CPU wrapper
    assert torch.equal(a, out)


# ------------------------------------------------------------------------------- linear_small
# which cases can show a mutant: (M, K, N, (norm, act, bias, res)) -> bool
APPLIES = {
    "ln_no_mean": lambda M, K, N, c: c[0] == "ln",
    "ln_no_beta": lambda M, K, N, c: c[0] == "ln",
    "no_eps": lambda M, K, N, c: c[0] is not None,
    "stats_row_minus8": lambda M, K, N, c: c[0] is not None and M > 8,
    "k_tail_dropped": lambda M, K, N, c: True,
    "bias_first_pass_only": lambda M, K, N, c: c[2] and N > 512 * 16,
    "res_first_pass_only": lambda M, K, N, c: c[3] and N > 512 * 16,
    "res_wrong_row": lambda M, K, N, c: c[3] and M > 1,
    "swiglu_swapped": lambda M, K, N, c: c[1] == "swiglu",
    "swiglu_up_shift": lambda M, K, N, c: c[1] == "swiglu" and N % 16 != 0,
    "gelu_before_bias": lambda M, K, N, c: c[1] == "gelu" and c[2],
    "row_tail_zero": lambda M, K, N, c: M % 16 != 0,
}
# the GPU test's rows the mutants are proven at (all of its shapes and combinations)
LINEAR_PROOF_ROWS = (1, 9, 33, 64)


@functools.lru_cache(maxsize=None)
def _linear_case(M, K, N, ci):
    combo = rd.LINEAR_COMBOS[ci]
    (M, K, N), (x, w, b, nrm, rs) = rd.linear_case(M, K, N, combo)
    exact = rd.linear_small_ref(x, w, b, nrm, combo[1], rs)
    emu = rd.linear_small_ref(x, w, b, nrm, combo[1], rs, emulate=True)
    return (x, w, b, nrm, rs), rd.tiles16(exact), rm.tile_rel(rd.tiles16(emu), rd.tiles16(exact), 16)


def _linear_cases():
    for M in LINEAR_PROOF_ROWS:
        for K, N in rd.LINEAR_SHAPES:
            for ci, combo in enumerate(rd.LINEAR_COMBOS):
                yield M, K, N, ci, combo


def test_linear_floor_is_a_bf16_rounding():
    lo, hi = 1.0, 0.0
    for M, K, N, ci, combo in _linear_cases():
        _, _, floor = _linear_case(M, K, N, ci)
        lo, hi = min(lo, floor), max(hi, floor)
        # the output's rounding (2^-9 of the element) plus, with a norm, K roundings of the
        # normalised x, largest relative to a tile where K = 32 terms cancel among 1025 tiles;
        # SwiGLU multiplies two such sums.  (A case of fewer than 256 outputs can have drawn only
        # small roundings.)
        assert (1e-3 if M * N >= 256 else 1e-4) < floor < (4e-2 if combo[1] == "swiglu" else 2e-2), (
            M, K, N, combo, floor)
    print(f"\nlinear_small floors {lo:.2e} .. {hi:.2e}")


@pytest.mark.parametrize("mutant", rd.LINEAR_MUTANTS)
def test_linear_mutant_is_caught(mutant):
    ran, worst = 0, (float("inf"), None)
    for M, K, N, ci, combo in _linear_cases():
        if not APPLIES[mutant](M, K, N, combo):
            continue
        (x, w, b, nrm, rs), exact, floor = _linear_case(M, K, N, ci)
        got = rd.linear_small_ref(x, w, b, nrm, combo[1], rs, emulate=True, mutant=mutant)
        score = rm.tile_rel(rd.tiles16(got), exact, 16)
        ran += 1
        worst = min(worst, (score / floor, (M, K, N, combo)))
        assert score >= 9 * floor, (mutant, M, K, N, combo, score, floor)
    print(f"\nlinear_small {mutant:22s} {ran} cases, least score/floor {worst[0]:.0f} at {worst[1]}")
    assert ran >= 4, (mutant, ran)


def test_linear_plan_reaches_the_paths():
    """the shapes of the GPU test run what no test ran: the tile loop, MT > 1 with a norm, the
    prologue's second row per wave; none of them exceeds the op's LDS."""
    assert rd.linear_small_plan(64, 576, 2064, "ln", "none")[0] == 4  # >= 128 tiles: MT = ⌈M/16⌉
    assert rd.linear_small_plan(33, 576, 2064, "rms", "swiglu")[0] == 3
    assert rd.linear_small_plan(64, 4096, 2064, "ln", "none")[0] == 1  # the x image would not fit
    assert rd.linear_small_plan(64, 576, 272, "ln", "none")[0] == 1  # < 128 tiles
    mt, staged, lds, grid = rd.linear_small_plan(9, 96, 16389, "ln", "none")
    assert staged and grid == 512 and -(-16389 // 16) == 1025  # every workgroup loops 2 or 3 times
    for M in rd.LINEAR_ROWS:
        for K, N in rd.LINEAR_SHAPES:
            for norm, act, _, _ in rd.LINEAR_COMBOS:
                k = 2048 if act == "swiglu" and K > 2048 else K
                assert rd.linear_small_plan(M, k, N, norm, act)[2] <= 160 * 1024, (M, k, N, norm, act)


@pytest.mark.parametrize("ci", range(len(rd.LINEAR_COMBOS)))
def test_package_linear_reference_matches_fp64(ci):
    """``ops.linear_small_reference`` on fp32 inputs (no bf16 rounding anywhere): the fp64 formula
    to fp32 accuracy per 16 x 16 tile.  The bound: fp32's 6e-8 times the 48 σ row offsets that
    the mean subtraction and the dot products cancel, times a few."""
    combo = rd.LINEAR_COMBOS[ci]
    for M, K, N in ((9, 96, 48), (33, 576, 272), (17, 4096, 48)):
        (M, K, N), (x, w, b, nrm, rs) = rd.linear_case(M, K, N, combo)
        f = lambda t: None if t is None else t.float()  # noqa: E731
        nf = None if nrm is None else (nrm[0],) + tuple(f(t) for t in nrm[1:-1]) + (nrm[-1],)
        y = ops.linear_small_reference(f(x), f(w), f(b), norm=nf, act=combo[1], residual=f(rs))
        exact = rd.linear_small_ref(x, w, b, nrm, combo[1], rs)
        assert y.dtype == torch.float32 and y.shape == (M, N)
        err = rm.tile_rel(rd.tiles16(y), rd.tiles16(exact), 16)
        print(f"\nlinear_small_reference {combo} M{M} K{K} N{N}: {err:.2e}")
        assert err < 2e-5, (combo, M, K, N, err)
