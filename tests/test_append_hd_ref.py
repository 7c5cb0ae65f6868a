"""CPU: the head-dim-generic block-append references (tests/refmath_append_hd.py) and the Python side
of head dim 128 in the block-append kernel.

  * at head dim 64 the generic reference is the fixed-width one of tests/refmath_append.py, bit for
    bit, on tests/test_append_ref.py's inputs: one reference, not two;
  * at 128 it agrees with the package's ``ops.append_attention_reference`` to fp32 accuracy per head
    row, on the inputs of tests/test_gpu_append_hd.py;
  * on those inputs (the same draws, with the finite ``loud`` poison in the free cache rows: a wrong
    formula that reads ±3e38 or NaN has no finite score to compare) every wrong "mutant" — the six
    of refmath_append and the seven a 128 kernel can be where a 64 one cannot — scores >= 9 x floor
    per 32-row tile (the rule of tests/test_append_ref.py; the GPU bound is 3 x floor);
  * ``ops.append_supported`` routes head dim 64 and 128 to the kernel, 96 and an fp8 cache away;
  * two turns on a head-dim-128 Llama on the CPU: the behaviour the GPU path must keep.
``-s`` prints the scores."""
import functools
import types

import pytest
import torch

import refmath as rm
import refmath_append as ra
import refmath_append_hd as hd
import test_append_ref as t64
from nbdistributed_amd import ops
from nbdistributed_amd.generation import generate

D = 128
SCALE = hd.scale_of(D)


# ------------------------------------------------------------------ one reference at head dim 64
def test_generic_reference_equals_the_fixed_one_at_64():
    assert hd.scale_of(64) == t64.SCALE
    args = (t64.B, t64.H, t64.HKV, t64.TN, t64.TMAX, t64.START)
    for poison in ("loud", "huge", "nan"):
        for a, b in zip(ra.append_inputs(*args, seed=7, poison=poison),
                        hd.append_inputs(*args, seed=7, poison=poison, head_dim=64)):
            assert torch.equal(a.view(torch.int16), b.view(torch.int16)), poison
    qkv, kc, vc = ra.append_inputs(*args, seed=7, poison="loud")
    for rope in (None, rm.rope_tables_ref(t64.TMAX)):
        for emulate in (False, True):
            for mutant in (None,) + ra.APPEND_MUTANTS:
                want = ra.append_ref(qkv, kc, vc, t64.START, t64.NNEW, t64.H, t64.SCALE, rope, emulate=emulate, mutant=mutant)
                got = hd.append_ref(qkv, kc, vc, t64.START, t64.NNEW, t64.H, t64.SCALE, rope, emulate=emulate, mutant=mutant)
                for a, b in zip(want, got):
                    assert torch.equal(a.view(torch.int64), b.view(torch.int64)), (rope is None, emulate, mutant)
    out = torch.randn(2, 5, 3 * 64)
    assert torch.equal(ra.per_head(out, 3), hd.per_head(out, 3, 64))


# ------------------------------------------------------------------ the GPU test's cases
CASES = tuple((H, Hkv, Tn, use_rope) for H, Hkv in hd.HEADS for Tn in hd.TNS for use_rope in (False, True))


def _scores(got, exact, H):
    out, kc, vc = got
    return {"out": rm.tile_rel(hd.per_head(out, H, D), hd.per_head(exact[0], H, D), 32),
            "k_cache": rm.tile_rel(kc, exact[1], 32), "v_cache": rm.tile_rel(vc, exact[2], 32)}


@functools.lru_cache(maxsize=None)
def _case(H, Hkv, Tn, use_rope):
    qkv, kc, vc, start, nnew = hd.offsets_case(H, Hkv, Tn, use_rope, "loud")
    rope = rm.rope_tables_ref(hd.TMAX, D) if use_rope else None
    exact = hd.append_ref(qkv, kc, vc, start, nnew, H, SCALE, rope)
    emu = hd.append_ref(qkv, kc, vc, start, nnew, H, SCALE, rope, emulate=True)
    return (qkv, kc, vc, start, nnew, rope), exact, _scores(emu, exact, H)


@pytest.mark.parametrize("poison", ["huge", "nan"])
def test_package_reference_matches_fp64_at_128(poison):
    """``ops.append_attention_reference`` on fp32 copies of the GPU test's inputs (its poisons)."""
    worst = 0.0
    for H, Hkv, Tn, use_rope in CASES:
        qkv, kc, vc, start, nnew = hd.offsets_case(H, Hkv, Tn, use_rope, poison)
        assert kc.shape == (3, Hkv, hd.TMAX, D) and qkv.shape == (3, Tn, (H + 2 * Hkv) * D)
        qkv, kc, vc = qkv.float(), kc.float(), vc.float()
        rope = rm.rope_tables_ref(hd.TMAX, D) if use_rope else None
        exact = hd.append_ref(qkv, kc, vc, start, nnew, H, SCALE, rope)
        k2, v2 = kc.clone(), vc.clone()
        out = ops.append_attention_reference(qkv, k2, v2, torch.tensor(start), torch.tensor(nnew), H, None, rope)
        assert out.shape == (3, Tn, H * D) and torch.isfinite(out).all()
        err = rm.tile_rel(hd.per_head(out, H, D), hd.per_head(exact[0], H, D), 1)  # per head row
        worst = max(worst, err)
        assert err < 1e-5, (H, Hkv, Tn, use_rope, err)
        for b in range(3):
            s0, end = start[b], start[b] + nnew[b]
            assert (out[b, nnew[b]:] == 0).all()
            assert rm.tile_rel(k2[b, :, s0:end], exact[1][b, :, s0:end], 1) < 1e-6
            assert torch.equal(v2[b, :, s0:end].double(), exact[2][b, :, s0:end])
            for new, old in ((k2, kc), (v2, vc)):
                assert torch.equal(new[b, :, end:].view(torch.int32), old[b, :, end:].view(torch.int32))
                assert torch.equal(new[b, :, :s0], old[b, :, :s0])
    print(f"\nappend 128 package reference vs fp64, {poison}: worst head row {worst:.2e}")


def test_floor_is_a_bf16_rounding_at_128():
    for c in CASES:
        (_, _, _, _, _, rope), _, floor = _case(*c)
        print(f"\nappend 128 floor H{c[0]}/{c[1]} Tn{c[2]} rope {c[3]}", {n: f"{x:.2e}" for n, x in floor.items()})
        assert 1e-3 < floor["out"] < 2.5e-2, (c, floor)  # as at 64 (tests/test_append_ref.py)
        if rope is not None:
            # the rotated k rounded to bf16: at most 2^-9 of an element, hence of the tile's largest;
            # well above fp32's 2^-24 (a single-token block rounds few elements: a smaller maximum)
            assert 2.0 ** -12 < floor["k_cache"] <= 2.0 ** -8, (c, floor)
        else:
            assert floor["k_cache"] == 0.0
        assert floor["v_cache"] == 0.0  # v is copied


# mutant -> the outputs it must move by >= 9 x floor
HITS = dict(t64.HITS, score_half_dims=("out",), rope_partner_32=("out", "k_cache"),
            rope_table_stride32=("out", "k_cache"), out_high_zero=("out",), out_high_neighbour=("out",),
            k_write_half=("out", "k_cache"), v_high_from_k=("out", "v_cache"))
ROPE_MUTANTS = ("rope_local", "rope_partner_32", "rope_table_stride32")


def _applies(mutant, H, Hkv, Tn, use_rope):
    if mutant in ROPE_MUTANTS:
        return use_rope
    if mutant == "gqa_mod":  # h % Hkv and h // G differ
        return 1 < Hkv < H
    if mutant == "pad_row_live":  # needs a padding row: sequence 1 brings one token of Tn
        return Tn > 1
    return True


@pytest.mark.parametrize("mutant", hd.APPEND_MUTANTS)
def test_mutant_is_caught_at_128(mutant):
    ran = 0
    for c in CASES:
        if not _applies(mutant, *c):
            continue
        ran += 1
        (qkv, kc, vc, start, nnew, rope), exact, floor = _case(*c)
        H = c[0]
        score = _scores(hd.append_ref(qkv, kc, vc, start, nnew, H, SCALE, rope, emulate=True, mutant=mutant), exact, H)
        print(f"\nappend 128 {mutant:20s} H{c[0]}/{c[1]} Tn{c[2]} rope {c[3]}",
              {n: f"{score[n]:.2e} (floor {floor[n]:.2e})" for n in HITS[mutant]})
        for n in HITS[mutant]:
            assert score[n] >= 9 * floor[n] and score[n] > 0, (mutant, c, n, score[n], floor[n])
    assert ran >= 6, (mutant, ran)


# ------------------------------------------------------------------ routing
def _standin(shape, dtype=torch.bfloat16):
    return types.SimpleNamespace(is_cuda=True, dtype=dtype, shape=torch.Size(shape))


def test_append_supported_takes_64_and_128():
    """stand-ins for GPU tensors: ``append_supported`` reads ``is_cuda``, ``dtype`` and ``shape`` only."""
    H, Hkv, Tn = 9, 3, 33
    for d, want in ((64, True), (128, True), (96, False)):
        qkv, kc = _standin((3, Tn, (H + 2 * Hkv) * d)), _standin((3, Hkv, hd.TMAX, d))
        assert ops.append_supported(qkv, kc, H) is want, d
        assert not ops.append_supported(qkv, _standin((3, Hkv, hd.TMAX, d), torch.float8_e4m3fn), H), d
        assert not ops.append_supported(qkv, kc, H + 1), d  # n_head % Hkv
        assert not ops.append_supported(_standin(qkv.shape, torch.float16), kc, H), d
    q = torch.zeros(3, Tn, (H + 2 * Hkv) * D, dtype=torch.bfloat16)  # not on the GPU: never supported
    assert not ops.append_supported(q, torch.zeros(3, Hkv, 8, D, dtype=torch.bfloat16), H)


# ------------------------------------------------------------------ two turns at head dim 128 (CPU)
def test_two_turns_at_128_on_the_cpu():
    from nbdistributed_amd.models.llama import LlamaConfig, LlamaForCausalLM

    torch.manual_seed(0)
    m = LlamaForCausalLM(LlamaConfig.tiny(explicit_head_dim=D)).eval()
    assert m.kv_layout()[3] == D
    with torch.no_grad():
        m.model.embed_tokens.weight.mul_(8.0)  # peaked logits: the best token is far from ties
    lens1, new1, lens2, new2 = (9, 4, 1), 5, (3, 1, 6), 4
    g = torch.Generator().manual_seed(1)
    ids1 = torch.randint(1, 512, (3, max(lens1)), generator=g)
    ids2 = torch.randint(1, 512, (3, max(lens2)), generator=g)
    out1, cache = generate(m, ids1, new1, lengths=torch.tensor(lens1), t_max=40, return_cache=True)
    assert cache.head_dim == D
    out2 = generate(m, ids2, new2, lengths=torch.tensor(lens2), cache=cache)
    hist = [out1[b, :lens1[b] + new1].tolist() + ids2[b, :lens2[b]].tolist() for b in range(3)]
    hl = torch.tensor([len(h) for h in hist])
    whole = torch.zeros(3, int(hl.max()), dtype=torch.long)
    for b, h in enumerate(hist):
        whole[b, :len(h)] = torch.tensor(h)
    ref = generate(m, whole, new2, lengths=hl)
    for b in range(3):
        n = lens2[b]
        assert out2[b, n:n + new2].tolist() == ref[b, len(hist[b]):len(hist[b]) + new2].tolist(), b
