"""CPU: the block-append attention references.  tests/refmath_append.py's fp64 formula against the
package's fp32 ``ops.append_attention_reference``, and the proof that the GPU test built on it
(tests/test_gpu_append_attn.py, bound 3 x floor per 32-row tile) can fail: on the structured,
poisoned inputs every wrong "mutant" of the formula scores >= 9 x floor on each output it must
move, where floor = tile_rel(emulated reference, fp64 reference).  ``-s`` prints the scores."""
import pytest
import torch

import refmath as rm
import refmath_append as ra
from nbdistributed_amd import ops

SCALE = 0.125
OUT = ("out", "k_cache", "v_cache")

# one short of a 64-key tile edge and the middle of a tile; a full block, a single token (its next
# row is poison), and a block that crosses a tile edge with padding behind it
B, H, HKV, TN, TMAX = 3, 4, 2, 40, 192
START, NNEW = (0, 63, 100), (40, 1, 37)

# mutant -> the outputs it must move by >= 9 x floor
HITS = {
    "mask_plus1": ("out",),
    "mask_minus1": ("out",),
    "rope_local": ("out", "k_cache"),
    "write_local": ("out", "k_cache", "v_cache"),
    "gqa_mod": ("out",),
    "pad_row_live": ("k_cache", "v_cache"),
}


def _scores(got, exact):
    out, kc, vc = got
    return {"out": rm.tile_rel(ra.per_head(out, H), ra.per_head(exact[0], H), 32),
            "k_cache": rm.tile_rel(kc, exact[1], 32), "v_cache": rm.tile_rel(vc, exact[2], 32)}


@pytest.fixture(scope="module")
def case():
    rope = rm.rope_tables_ref(TMAX)
    qkv, kc, vc = ra.append_inputs(B, H, HKV, TN, TMAX, START, seed=7, poison="loud")
    exact = ra.append_ref(qkv, kc, vc, START, NNEW, H, SCALE, rope)
    emu = ra.append_ref(qkv, kc, vc, START, NNEW, H, SCALE, rope, emulate=True)
    return (qkv, kc, vc, rope), exact, _scores(emu, exact)


def test_floor_is_a_bf16_rounding(case):
    _, _, floor = case
    print("\nappend floor", {n: f"{x:.2e}" for n, x in floor.items()})
    assert 1e-3 < floor["out"] < 2.5e-2, floor
    assert 1e-3 < floor["k_cache"] < 1e-2, floor  # the rotated k rounded to bf16
    assert floor["v_cache"] == 0.0  # v is copied


@pytest.mark.parametrize("mutant", ra.APPEND_MUTANTS)
def test_mutant_is_caught(case, mutant):
    (qkv, kc, vc, rope), exact, floor = case
    score = _scores(ra.append_ref(qkv, kc, vc, START, NNEW, H, SCALE, rope, emulate=True, mutant=mutant), exact)
    print(f"\nappend {mutant:13s}", {n: f"{score[n]:.2e} (floor {floor[n]:.2e})" for n in HITS[mutant]})
    for n in HITS[mutant]:
        assert score[n] >= 9 * floor[n] and score[n] > 0, (mutant, n, score[n], floor[n])


def test_reference_leaves_rows_past_the_block_alone(case):
    (qkv, kc, vc, rope), exact, _ = case
    for b in range(B):
        end = START[b] + NNEW[b]
        assert torch.equal(exact[1][b, :, end:], kc[b, :, end:].double())
        assert torch.equal(exact[2][b, :, end:], vc[b, :, end:].double())
        assert torch.equal(exact[1][b, :, :START[b]], kc[b, :, :START[b]].double())
        assert (exact[0][b, NNEW[b]:] == 0).all()


@pytest.mark.parametrize("use_rope", [False, True])
@pytest.mark.parametrize("poison", ["loud", "nan"])
def test_package_reference_matches_fp64(use_rope, poison):
    """``ops.append_attention_reference`` on fp32 inputs: the fp64 formula to fp32 accuracy, the
    caches written the same way, rows past the block untouched bit for bit, zeros on padding."""
    rope = rm.rope_tables_ref(TMAX) if use_rope else None
    qkv, kc, vc = (t.float() for t in ra.append_inputs(B, H, HKV, TN, TMAX, START, seed=11, poison=poison))
    exact = ra.append_ref(qkv, kc, vc, START, NNEW, H, SCALE, rope)
    k2, v2 = kc.clone(), vc.clone()
    out = ops.append_attention_reference(qkv, k2, v2, torch.tensor(START), torch.tensor(NNEW), H, SCALE, rope)
    assert out.dtype == qkv.dtype and out.shape == (B, TN, H * 64)
    assert torch.isfinite(out).all()
    assert rm.tile_rel(ra.per_head(out, H), ra.per_head(exact[0], H), 32) < 1e-5
    for b in range(B):
        s0, end = START[b], START[b] + NNEW[b]
        assert (out[b, NNEW[b]:] == 0).all()
        assert rm.tile_rel(k2[b, :, s0:end], exact[1][b, :, s0:end], 32) < 1e-6
        assert torch.equal(v2[b, :, s0:end].double(), exact[2][b, :, s0:end])
        for new, old in ((k2, kc), (v2, vc)):
            assert torch.equal(new[b, :, end:].view(torch.int32), old[b, :, end:].view(torch.int32))
            assert torch.equal(new[b, :, :s0], old[b, :, :s0])


def test_package_reference_clamps_like_the_kernel():
    """positions from start / nnew are clamped before they address anything."""
    qkv, kc, vc = (t.float() for t in ra.append_inputs(2, 2, 2, 5, 16, (0, 0), seed=3, poison="loud"))
    out = ops.append_attention_reference(qkv, kc, vc, torch.tensor([-4, 14]), torch.tensor([9, 5]), 2, SCALE)
    assert torch.isfinite(out).all()
    assert (out[1, 2:] == 0).all() and (out[1, :2] != 0).any()  # start 14 of 16: two rows fit


def test_public_wrapper_on_cpu_is_the_reference():
    qkv, kc, vc = (t.float() for t in ra.append_inputs(B, H, HKV, TN, TMAX, START, seed=5, poison="loud"))
    a = ops.append_attention(qkv, kc.clone(), vc.clone(), torch.tensor(START), torch.tensor(NNEW), H)
    b = ops.append_attention_reference(qkv, kc.clone(), vc.clone(), torch.tensor(START), torch.tensor(NNEW), H)
    assert torch.equal(a, b)
    assert not ops.append_supported(qkv, kc, H)
