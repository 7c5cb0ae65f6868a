"""CPU: ``ops.decode_attention_shared_reference`` (several samples per prompt over one shared
prefix) against ``ops.decode_attention_reference`` on the materialised cache — one private cache
of Tp + Ts rows per sequence, ``M[s, :, j]`` = the prompt's prefix row below plen, the sequence's
own row j - plen from there on (tests/refmath_shared.py).  The two must be *equal*: the output,
the written row (at ``own[s, :, pos - plen]``), and every other row untouched — bf16 and fp8
caches, ragged plen including 0 and Tp, NaN in every row the op must not read.  And the proof
that this equality can fail: each wrong addressing rule of ``SHARED_MUTANTS`` changes the result."""
import pytest
import torch

import refmath as rm
import refmath_decode as rd
import refmath_shared as rs
from nbdistributed_amd import ops

SCALE = rd.SCALE
B, GROUP, HKV, G, TP, TS = 4, 3, 2, 3, 40, 24
H = G * HKV
PLEN = (0, 40, 17, 33)  # an empty prefix, a full one, two ragged
POS = (0, 5, 23,  40, 41, 63,  17, 20, 40,  33, 34, 56)  # first own row, in between, last own row


def _case(poison, fp8, seed=7):
    return rs.shared_case(B, GROUP, H, HKV, TP, TS, PLEN, POS, seed, poison, fp8)


def _run_shared(qkv, pk, pv, ok, ov, rope, plen=PLEN, pos=POS):
    ok, ov = ok.clone(), ov.clone()
    out = ops.decode_attention_shared_reference(qkv, pk, pv, torch.tensor(plen), ok, ov, torch.tensor(pos), GROUP, H,
                                                SCALE, rope)
    return out, ok, ov


def _run_materialised(qkv, pk, pv, ok, ov, rope, mutant=None, pos=POS):
    km, vm = rs.materialise(pk, ok, PLEN, GROUP, mutant), rs.materialise(pv, ov, PLEN, GROUP, mutant)
    out = ops.decode_attention_reference(qkv, km, vm, torch.tensor(pos), H, SCALE, rope)
    return out, km, vm


@pytest.mark.parametrize("use_rope", [False, True], ids=["plain", "rope"])
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_shared_reference_equals_the_materialised_cache(fp8, use_rope):
    rope = rm.rope_tables_ref(TP + TS) if use_rope else None
    rope = None if rope is None else (rope[0].float(), rope[1].float())
    for poison in ("nan", "max" if fp8 else "huge"):
        qkv, pk, pv, ok, ov = _case(poison, fp8)
        out, ok2, ov2 = _run_shared(qkv, pk.clone(), pv.clone(), ok, ov, rope)
        want, km, vm = _run_materialised(qkv, pk, pv, ok, ov, rope)
        assert out.dtype == torch.bfloat16 and out.shape == (B * GROUP, H * 64)
        assert torch.isfinite(out.float()).all()
        assert torch.equal(rs.raw(out), rs.raw(want))
        pl = rs.per_sequence(PLEN, GROUP)
        s, pos = torch.arange(B * GROUP), torch.tensor(POS)
        for new, old, mat in ((ok2, ok, km), (ov2, ov, vm)):
            # the written row sits at own[s, :, pos - plen] and is the row the unshared op wrote at pos
            assert torch.equal(rs.raw(new)[s, :, pos - pl], rs.raw(mat)[s, :, pos])
            keep = rs.raw(old).clone()
            keep[s, :, pos - pl] = rs.raw(new)[s, :, pos - pl]
            assert torch.equal(rs.raw(new), keep), "an own row other than pos - plen was written"
        # the materialised cache after the unshared call is the materialised (prefix, own) after the shared one
        assert torch.equal(rs.raw(rs.materialise(pk, ok2, PLEN, GROUP)), rs.raw(km))
        assert torch.equal(rs.raw(rs.materialise(pv, ov2, PLEN, GROUP)), rs.raw(vm))


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_shared_reference_never_writes_the_prefix_and_reads_no_other_prompt(fp8):
    """the prefix tensors are bit for bit what they were; with every *other* prompt's prefix NaN
    throughout, a prompt's sequences give what they gave."""
    qkv, pk, pv, ok, ov = _case("nan", fp8)
    pk0, pv0 = pk.clone(), pv.clone()
    out, _, _ = _run_shared(qkv, pk, pv, ok, ov, None)
    assert torch.equal(rs.raw(pk), rs.raw(pk0)) and torch.equal(rs.raw(pv), rs.raw(pv0))
    nan_k, nan_v = rs.shared_case(B, GROUP, H, HKV, TP, TS, (0,) * B, (0,) * (B * GROUP), 7, "nan", fp8)[1:3]
    for b in range(B):
        qk, qv = rs.raw(nan_k).clone(), rs.raw(nan_v).clone()
        qk[b], qv[b] = rs.raw(pk)[b], rs.raw(pv)[b]
        o2, _, _ = _run_shared(qkv, qk.view(pk.dtype), qv.view(pv.dtype), ok, ov, None)
        rows = slice(b * GROUP, (b + 1) * GROUP)
        assert torch.equal(rs.raw(o2[rows]), rs.raw(out[rows])), b


def test_shared_reference_clamps_plen_and_pos():
    """plen outside [0, Tp] and pos outside [plen, plen + Ts - 1] act as their clamped values: the
    new row never lands in the prefix, nothing is addressed out of bounds."""
    qkv, pk, pv, ok, ov = _case("nan", False)
    wild_plen = tuple(p if 0 < p < TP else (-5 if p == 0 else TP + 9) for p in PLEN)
    pl = rs.per_sequence(PLEN, GROUP).tolist()
    wild_pos = tuple(-3 if p == q else (10 ** 6 if p == q + TS - 1 else p) for p, q in zip(POS, pl))
    assert wild_plen != PLEN and wild_pos != POS
    a = _run_shared(qkv, pk, pv, ok, ov, None)
    b = _run_shared(qkv, pk, pv, ok, ov, None, plen=wild_plen, pos=wild_pos)
    for x, y in zip(a, b):
        assert torch.equal(rs.raw(x), rs.raw(y))


def test_shared_reference_refuses_mixed_cache_dtypes():
    qkv, pk, pv, ok, ov = _case("nan", False)
    with pytest.raises(ValueError, match="same dtype"):
        ops.decode_attention_shared(qkv, rs.r8.q8(pk.float()), rs.r8.q8(pv.float()), torch.tensor(PLEN), ok, ov,
                                    torch.tensor(POS), GROUP, H, SCALE)
    out = ops.decode_attention_shared(qkv, pk, pv, torch.tensor(PLEN), ok.clone(), ov.clone(), torch.tensor(POS),
                                      GROUP, H, SCALE)  # the CPU wrapper
    assert torch.equal(rs.raw(out), rs.raw(_run_shared(qkv, pk, pv, ok, ov, None)[0]))


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("mutant", rs.SHARED_MUTANTS)
def test_shared_mutant_fails_the_equality(mutant, fp8):
    """each wrong addressing rule, computed through the same unshared reference on the wrongly
    materialised cache, changes the output of every prompt it can touch: with finite poison the
    numbers differ, with NaN poison the output is NaN where a poisoned row was read."""
    for poison in (("max", "nan") if fp8 else ("loud", "nan")):
        qkv, pk, pv, ok, ov = _case(poison, fp8)
        # the op has run: the rows at pos are real, as they are when the next step reads them
        good, ok, ov = _run_shared(qkv, pk, pv, ok, ov, None)
        nxt = tuple(p + 1 if p + 1 < q + TS else p for p, q in zip(POS, rs.per_sequence(PLEN, GROUP).tolist()))
        good, _, _ = _run_shared(qkv, pk, pv, ok, ov, None, pos=nxt)
        want, _, _ = _run_materialised(qkv, pk, pv, ok, ov, None, pos=nxt)
        assert torch.equal(rs.raw(good), rs.raw(want))
        bad, _, _ = _run_materialised(qkv, pk, pv, ok, ov, None, mutant=mutant, pos=nxt)
        differs = (rs.raw(bad) != rs.raw(good)).reshape(B, GROUP, -1).any(-1)  # [prompt, sample]
        print(f"\nshared {mutant:16s} {'fp8' if fp8 else 'bf16'} {poison}: sequences changed {differs.tolist()}")
        if mutant == "prefix_row_s":  # every sequence with a prefix whose s % B is not its prompt
            hit = torch.tensor([s % B != s // GROUP and PLEN[s // GROUP] > 0 for s in range(B * GROUP)])
            assert hit.sum() >= 6 and torch.equal(differs.flatten(), hit), (mutant, poison, differs)
        elif mutant == "own_index_j":  # every prompt with a prefix reads own rows plen too far
            assert differs[1:].all() and not differs[0].any(), (mutant, poison, differs)
        elif mutant == "boundary_plus1":  # key plen from the prefix: poison, or a row past a full prefix
            assert differs[[0, 2, 3]].all(), (mutant, poison, differs)
        else:  # key plen - 1 from own row -1 (clamped to row 0): every prompt with a prefix
            assert differs[1:].all() and not differs[0].any(), (mutant, poison, differs)
