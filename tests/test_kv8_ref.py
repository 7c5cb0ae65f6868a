"""CPU: the reference of decode attention over an fp8 KV cache (tests/refmath_kv8.py), and the proof
that the GPU tests built on it (tests/test_gpu_kv8.py) can fail.  On the very inputs those tests
use, every output mutant scores >= 9 x floor per head row, floor = tile_rel(emulated, exact) — the
rule of tests/test_decode_ref.py — and every row mutant changes bytes of the stored row, which the
GPU test compares bit for bit (a floor of 0).  ``-s`` prints the scores.

Inputs: ``refmath_decode.decode_history`` unchanged, quantised with ``q8``.  No input had to be
changed for a mutant to reach the bound: with the caches given as stored the floor is the
output's bf16 rounding alone, and the weakest mutant, ``new_key_unquantised``, moves the rows at
the first few positions (every case has some) by the e4m3 rounding of v, up to 2^-4 of an element:
11 x floor and up."""
import functools

import pytest
import torch

import refmath as rm
import refmath_decode as rd
import refmath_kv8 as r8
from nbdistributed_amd import ops

SCALE = rd.SCALE
CASES = ("group G3 T640 rope", "group G8 T640 plain", "group G5 T320 rope", "group G1 T320 plain",
         "sweep kv513 G3 launch 0", "sweep kv512 G6 launch 2")
ROW_CASES = ("saturating rope", "saturating plain", "group G3 T640 rope")


def _head(out, H):
    return rd.decode_per_head(out, H)


@functools.lru_cache(maxsize=None)
def _case(name):
    w = name.split()
    if w[0] == "group":
        G, Tmax, use_rope = int(w[1][1:]), int(w[2][1:]), w[3] == "rope"
        H, Hkv, pos, (qkv, k8, v8) = r8.group_case8(G, Tmax, "max", use_rope)
    elif w[0] == "saturating":
        use_rope, Tmax = w[1] == "rope", 320
        H, Hkv, pos, (qkv, k8, v8) = r8.saturating_case(use_rope)
    else:
        Tmax, G, launch = int(w[1][2:]), int(w[2][1:]), int(w[4])
        assert r8.SWEEP_POISON8[launch % 2] == "max"
        H, Hkv, use_rope, pos = G, 1, True, rd.sweep_positions(Tmax, launch)
        qkv, k8, v8 = r8.kv8_poison(r8.sweep_history8(Tmax, G), pos, "max")
    rope = rm.rope_tables_ref(Tmax) if use_rope else None
    return qkv, k8, v8, pos, H, Hkv, rope


@functools.lru_cache(maxsize=None)
def _scored(name):
    qkv, k8, v8, pos, H, Hkv, rope = _case(name)
    k16, v16, kn, vn = r8.stored_rows8(qkv, pos, H, Hkv, rope)
    q = qkv[:, : H * 64]
    exact = r8.decode8_ref(q, k8, v8, kn, vn, pos, H, SCALE, rope)
    emu = r8.decode8_ref(q, k8, v8, kn, vn, pos, H, SCALE, rope, emulate=True)
    return (k16, v16, kn, vn), exact, rm.tile_rel(_head(emu, H), _head(exact, H), 1)


def test_q8_is_clamp_then_round_to_nearest_even():
    x = torch.tensor([0.0, 1.0, 1.0625, 1.1875, 17.0, 19.0, 448.0, 449.0, 464.0, 480.0, 1e4, float("inf"),
                      2.0 ** -9, 2.0 ** -10, 3 * 2.0 ** -10])
    want = torch.tensor([0.0, 1.0, 1.0, 1.25, 16.0, 20.0, 448.0, 448.0, 448.0, 448.0, 448.0, 448.0,
                         2.0 ** -9, 0.0, 2.0 ** -8])  # ties to even; 2^-9 is the smallest subnormal
    for sign in (1.0, -1.0):
        got = r8.q8(sign * x)
        assert got.dtype == torch.float8_e4m3fn
        assert torch.equal(r8.dq8(got), (sign * want).double())
        assert torch.equal(r8.bits8(ops.decode.q8(sign * x)), r8.bits8(got))  # the package's q8 is this one
    nan = r8.bits8(r8.q8(torch.tensor([float("nan"), -float("nan")])))
    assert (nan & 0x7F).tolist() == [0x7F, 0x7F]  # NaN stays NaN (its sign is torch's business: canon8)
    assert r8.bits8(r8.q8(torch.tensor([448.0, -448.0]))).tolist() == [r8.MAX_BYTE, r8.MAX_BYTE | 0x80]
    # every e4m3fn value is exact in bf16: dequantising rounds nothing
    every = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn)
    assert torch.equal(torch.nan_to_num(every.float(), nan=7.0), torch.nan_to_num(every.bfloat16().float(), nan=7.0))
    assert torch.equal(r8.dq8(every, fnuz=True)[:0x7F], 0.5 * r8.dq8(every)[:0x7F])


def test_history_does_not_saturate():
    _, kc, vc, _ = rd.decode_history(4, 6, 2, 1024, 0)
    assert kc.abs().max() < 32 and vc.abs().max() < 16  # far below 448: only the saturating case clamps


@pytest.mark.parametrize("name", CASES)
def test_kv8_floor_is_the_output_rounding(name):
    _, _, floor = _scored(name)
    print(f"\nkv8 floor {name}: {floor:.2e}")
    # one rounding of the output to bf16: 2^-9 .. 2^-8 = 3.9e-3 of the element that is the head row's
    # maximum, plus fp32 noise; no k or v rounding happens past the stored bytes (the bf16 cache's
    # floor reaches 5.3e-3 through the rotated k's rounding)
    assert 1e-3 < floor < 4e-3, floor


@pytest.mark.parametrize("mutant", r8.OUT_MUTANTS)
def test_kv8_output_mutant_is_caught(mutant):
    for name in CASES:
        qkv, k8, v8, pos, H, Hkv, rope = _case(name)
        (k16, v16, kn, vn), exact, floor = _scored(name)
        got = r8.decode8_ref(qkv[:, : H * 64], k8, v8, kn, vn, pos, H, SCALE, rope, emulate=True, mutant=mutant,
                             new_bf16=(k16, v16))
        score = rm.tile_rel(_head(got, H), _head(exact, H), 1)
        print(f"\nkv8 {mutant:20s} {name}: {score:.2e} (floor {floor:.2e}, ratio {score / floor:.0f})")
        assert score >= 9 * floor and score > 0, (mutant, name, score, floor)


@pytest.mark.parametrize("mutant", r8.ROW_MUTANTS)
def test_kv8_row_mutant_alters_the_stored_bytes(mutant):
    ran = 0
    for name in ROW_CASES:
        qkv, k8, v8, pos, H, Hkv, rope = _case(name)
        if (mutant == "single_rounding" and rope is None) or (mutant == "no_clamp" and not name.startswith("saturating")):
            continue  # an unrotated k is bf16 already; only the saturating case leaves ±448
        ran += 1
        _, _, kn, vn = r8.stored_rows8(qkv, pos, H, Hkv, rope)
        _, _, km, vm = r8.stored_rows8(qkv, pos, H, Hkv, rope, mutant=mutant)
        dk = (r8.canon8(km) != r8.canon8(kn)).float().mean().item()
        dv = (r8.canon8(vm) != r8.canon8(vn)).float().mean().item()
        print(f"\nkv8 {mutant:16s} {name}: k bytes differing {dk:.3%}, v bytes {dv:.3%}")
        assert dk > 0, (mutant, name)
        if mutant == "no_clamp":
            assert dv > 0, (mutant, name)
        else:
            assert dv == 0
    assert ran >= 2, (mutant, ran)


def test_saturating_case_stores_the_bounds_and_nan():
    qkv, k8, v8, pos, H, Hkv, rope = _case("saturating plain")
    k16, v16, kn, vn = r8.stored_rows8(qkv, pos, H, Hkv, None)
    for r16, r in ((k16, kn), (v16, vn)):
        b = r8.bits8(r)
        assert (r16.isinf().sum(), r16.isnan().sum()) == (2 * len(pos) * Hkv, 2 * len(pos) * Hkv)
        assert torch.equal(b[r16 == float("inf")], torch.full((len(pos) * Hkv,), 0x7E, dtype=torch.uint8))
        assert torch.equal(b[r16 == -float("inf")], torch.full((len(pos) * Hkv,), 0xFE, dtype=torch.uint8))
        assert torch.equal(b[r16.float() >= 449.0], torch.full((int((r16.float() >= 449.0).sum()),), 0x7E, dtype=torch.uint8))
        assert set(r8.canon8(r)[r16.isnan()].tolist()) == {0x7F}  # NaN of both signs stays NaN
        assert (b[~r16.isnan()] & 0x7F != 0x7F).all()  # and nothing else becomes NaN


@pytest.mark.parametrize("use_rope", [False, True])
@pytest.mark.parametrize("poison", r8.KV8_POISON)
def test_package_reference_on_an_fp8_cache_matches_fp64(use_rope, poison):
    """``ops.decode_attention_reference`` (the CPU path of ``generate``) on fp8 caches: rows written
    as ``q8`` of the bf16 row, every other byte untouched, the output the fp64 formula over the
    cache as stored to fp32 accuracy — whatever rows past ``pos`` hold."""
    Tmax, G = 320, 3
    H, Hkv, pos, (qkv, k8, v8) = r8.group_case8(G, Tmax, poison, use_rope)
    rope = rm.rope_tables_ref(Tmax) if use_rope else None
    k2, v2 = k8.clone(), v8.clone()
    out = ops.decode_attention_reference(qkv.float(), k2, v2, torch.tensor(pos), H, SCALE, rope)
    assert torch.isfinite(out).all() and out.shape == (len(pos), H * 64)
    bi, pt = torch.arange(len(pos)), torch.tensor(pos)
    _, _, kn, vn = r8.stored_rows8(qkv, pos, H, Hkv, rope)
    assert torch.equal(r8.canon8(v2[bi, :, pt]), r8.canon8(vn))
    # the rotation runs in fp32 there and in fp64 here: a bf16 tie may fall the other way, rarely
    assert (r8.canon8(k2[bi, :, pt]) != r8.canon8(kn)).float().mean() < (2e-3 if use_rope else 1e-9)
    for new, old in ((k2, k8), (v2, v8)):
        want = r8.bits8(old).clone()
        want[bi, :, pt] = r8.bits8(new)[bi, :, pt]
        assert torch.equal(r8.bits8(new), want)
    exact = r8.decode8_ref(qkv[:, : H * 64], k8, v8, k2[bi, :, pt], v2[bi, :, pt], pos, H, SCALE, rope)
    assert rm.tile_rel(_head(out, H), _head(exact, H), 1) < 1e-5
    a = ops.decode_attention(qkv.float(), k8.clone(), v8.clone(), torch.tensor(pos), H, SCALE, rope)  # the CPU wrapper
    assert torch.equal(a, out)
