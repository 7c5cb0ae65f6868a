"""GPU numerics of the block-append attention kernel (csrc/kernels/append.hip) against the fp64
reference of tests/refmath_append.py, per 32-row tile (one wave's queries of one head) on
structured inputs whose cache rows past ``start`` hold poison — huge finite values, then NaN.

The bound is test_gpu_attn_paths.py's rule, not a fitted constant: ``floor = tile_rel(emulated
reference, fp64 reference)`` on the same inputs and ``tile_rel(kernel, fp64 reference) <= 3 x
floor``.  tests/test_append_ref.py shows on the CPU that wrong formulas score >= 9 x floor.  Run
with ``-s`` for every kernel/floor ratio and, at the end, the worst one (docs/FINDINGS.md keeps
the last recorded figure)."""
import math

import pytest
import torch

import refmath as rm
import refmath_append as ra
from nbdistributed_amd import ops

pytestmark = pytest.mark.gpu

SCALE = 0.125
TMAX = 384
WORST = [0.0, ""]


@pytest.fixture(scope="module")
def dev(require_gpu):
    assert ops.native_available(), ops._load_error
    yield torch.device("cuda", 0)
    print(f"\nworst append kernel/floor ratio (bound 3): {WORST[0]:.2f}  {WORST[1]}")


def _bits(t):
    return t.contiguous().view(torch.int16)


def _note(case, err, floor):
    ratio = err / floor if floor > 0 else (0.0 if err == 0 else math.inf)
    print(f"  {case}: kernel {err:.3e} floor {floor:.3e} ratio {ratio:.2f}")
    if ratio > WORST[0]:
        WORST[0], WORST[1] = ratio, case
    return err <= 3 * floor


def _refs(qkv, kc, vc, start, nnew, H, rope):
    rope_cpu = None if rope is None else (rope[0].cpu(), rope[1].cpu())
    exact = ra.append_ref(qkv, kc, vc, start, nnew, H, SCALE, rope_cpu)
    emu = ra.append_ref(qkv, kc, vc, start, nnew, H, SCALE, rope_cpu, emulate=True)
    return exact, emu, rm.tile_rel(ra.per_head(emu[0], H), ra.per_head(exact[0], H), 32)


def _run_and_check(dev, case, qkv, kc, vc, start, nnew, H, rope, exact, emu, floor, raw=None):
    """one kernel call on device copies of (qkv, kc, vc): every figure printed, then every check.
    ``raw``: the start / nnew handed to the kernel when they differ from the clamped ones."""
    B, Tn, _ = qkv.shape
    Hkv = kc.shape[1]
    kd, vd = kc.to(dev), vc.to(dev)
    st, nn = (torch.tensor(x, dtype=torch.int64, device=dev) for x in (raw or (start, nnew)))
    out = ops.append_attention(qkv.to(dev), kd, vd, st, nn, H, scale=SCALE, rope=rope)
    torch.cuda.synchronize()
    out, kd, vd = out.cpu(), kd.cpu(), vd.cpu()
    assert out.shape == (B, Tn, H * 64) and out.dtype == torch.bfloat16
    ok = _note(case, rm.tile_rel(ra.per_head(out, H), ra.per_head(exact[0], H), 32), floor)
    assert torch.isfinite(out).all(), case
    for b in range(B):
        s0, n = start[b], nnew[b]
        assert (_bits(out[b, n:]) == 0).all(), (case, b)  # padding rows: exact zeros
        for new, old in ((kd, kc), (vd, vc)):  # nothing but rows [start, start + nnew) was written
            assert torch.equal(_bits(new[b, :, s0 + n:]), _bits(old[b, :, s0 + n:])), (case, b)
            assert torch.equal(_bits(new[b, :, :s0]), _bits(old[b, :, :s0])), (case, b)
        v_new = qkv[b, :n, (H + Hkv) * 64:].reshape(n, Hkv, 64).transpose(0, 1)
        assert torch.equal(_bits(vd[b, :, s0:s0 + n]), _bits(v_new)), (case, b)
        torch.testing.assert_close(kd[b, :, s0:s0 + n].float(), emu[1][b, :, s0:s0 + n].float(), atol=2e-2, rtol=1e-2)
    assert ok, (case, "tile_rel above 3 x floor")
    return out


@pytest.mark.parametrize("Tn", [1, 5, 32, 33, 100, 130])
@pytest.mark.parametrize("use_rope", [False, True], ids=["plain", "rope"])
@pytest.mark.parametrize("H,Hkv", [(4, 4), (9, 3), (8, 1)])
def test_append_attention_offsets_and_poison(dev, H, Hkv, use_rope, Tn):
    """start = an empty cache, one short of a 64-key tile edge, the middle of a tile; nnew = the
    whole block, a single token (the rest padding), a block that crosses a tile edge.  The rows
    past ``start`` hold huge finite values, then NaN: neither may reach an output."""
    start, nnew = (0, 63, 200), (Tn, 1, min(Tn, 37))
    rope = ops.rope_tables(TMAX, 64, 10000.0, dev) if use_rope else None
    seed = 1000 * H + 10 * Tn + use_rope
    qkv, kc, vc = ra.append_inputs(3, H, Hkv, Tn, TMAX, start, seed, poison="huge")
    exact, emu, floor = _refs(qkv, kc, vc, start, nnew, H, rope)
    case = f"H{H}/{Hkv} Tn{Tn} {'rope' if use_rope else 'plain'}"
    _run_and_check(dev, case + " huge", qkv, kc, vc, start, nnew, H, rope, exact, emu, floor)
    _, kn, vn = ra.append_inputs(3, H, Hkv, Tn, TMAX, start, seed, poison="nan")  # the same draw, NaN poison
    assert torch.equal(_bits(kn[1, :, :63]), _bits(kc[1, :, :63])) and kn[0].isnan().all()
    _run_and_check(dev, case + " nan", qkv, kn, vn, start, nnew, H, rope, exact, emu, floor)


def test_append_attention_clamps_positions(dev):
    """start / nnew outside their ranges are clamped before they address anything: the result is
    that of the clamped values (start into [0, Tmax - 1], nnew into [0, min(Tn, Tmax - start)])."""
    H, Hkv, Tn = 4, 2, 40
    raw = ((-5, 10 ** 12, TMAX - 2), (Tn + 7, 3, 50))
    start, nnew = (0, TMAX - 1, TMAX - 2), (Tn, 1, 2)
    rope = ops.rope_tables(TMAX, 64, 10000.0, dev)
    qkv, kc, vc = ra.append_inputs(3, H, Hkv, Tn, TMAX, start, 77, poison="huge")
    exact, emu, floor = _refs(qkv, kc, vc, start, nnew, H, rope)
    _run_and_check(dev, "clamped", qkv, kc, vc, start, nnew, H, rope, exact, emu, floor, raw=raw)


def test_single_token_append_and_decode_kernel_agree(dev):
    """Tn = 1 is the decode kernel's problem: both kernels, each on a copy of the same cache, stay
    within their own bounds of the same fp64 reference (decode: test_gpu_decode.py's 2e-2)."""
    H, Hkv = 9, 3
    start, nnew = (0, 63, 200), (1, 1, 1)
    rope = ops.rope_tables(TMAX, 64, 10000.0, dev)
    qkv, kc, vc = ra.append_inputs(3, H, Hkv, 1, TMAX, start, 5, poison="huge")
    exact, emu, floor = _refs(qkv, kc, vc, start, nnew, H, rope)
    out = _run_and_check(dev, "Tn1 vs decode", qkv, kc, vc, start, nnew, H, rope, exact, emu, floor)
    kd, vd = kc.to(dev), vc.to(dev)
    dec = ops.decode_attention(qkv[:, 0].to(dev), kd, vd, torch.tensor(start, device=dev), H, scale=SCALE, rope=rope)
    err = float((dec.cpu().double() - exact[0][:, 0]).abs().max())
    print(f"  decode kernel: max abs err {err:.3e} (bound 2e-2); append vs decode "
          f"{float((dec.cpu().float() - out[:, 0].float()).abs().max()):.3e}")
    assert err < 2e-2
    for b in range(3):  # and both appended the same row
        torch.testing.assert_close(kd[b, :, start[b]].cpu().float(), emu[1][b, :, start[b]].float(), atol=2e-2, rtol=1e-2)


def test_append_from_empty_cache_is_causal_prefill(dev):
    """start = 0, nnew = Tn = 128: the flash forward's problem.  ``attention_qkv`` on the same
    packed projection and the append kernel both stay within 3 x floor of the fp64 reference."""
    H, Hkv, Tn = 9, 3, 128
    start, nnew = (0, 0), (Tn, Tn)
    rope = ops.rope_tables(Tn, 64, 10000.0, dev)
    qkv, kc, vc = ra.append_inputs(2, H, Hkv, Tn, Tn, start, 9, poison="nan")
    exact, emu, floor = _refs(qkv, kc, vc, start, nnew, H, rope)
    _run_and_check(dev, "prefill append", qkv, kc, vc, start, nnew, H, rope, exact, emu, floor)
    y = ops.attention_qkv(qkv.to(dev), H, causal=True, scale=SCALE, n_kv_head=Hkv, rope=rope).cpu()
    assert _note("prefill attention_qkv", rm.tile_rel(ra.per_head(y, H), ra.per_head(exact[0], H), 32), floor)
