"""CPU: the head-dim-generic decode references (tests/refmath_decode_hd.py) and the Python side of
head dim 128 in the decode kernel.

  * at head dim 64 the generic references are the fixed-width ones of tests/refmath_decode.py and
    tests/refmath_kv8.py, bit for bit: one reference, not two;
  * at 128 they agree with the package's ``decode_attention_reference`` /
    ``decode_attention_shared_reference`` to fp32 accuracy;
  * on the inputs of tests/test_gpu_decode_hd.py every wrong "mutant" — the ten of refmath_decode,
    the output mutants of refmath_kv8 and the six a 128 kernel can be where a 64 one cannot —
    scores >= 9 x floor per head row (the rule of tests/test_decode_ref.py; the GPU bound is 3 x
    floor), and the fp8 row mutants change the stored bytes;
  * the workspace: ``partials_numel(..., head_dim)`` and the caches that hold one;
  * ``generate`` on a head-dim-128 Llama on the CPU: the behaviour the GPU path must keep.
``-s`` prints the scores."""
import functools

import pytest
import torch

import refmath as rm
import refmath_decode as rd
import refmath_decode_hd as hd
import refmath_kv8 as r8
from nbdistributed_amd import ops
from nbdistributed_amd.generation import KVCache, SharedPrefixKVCache
from nbdistributed_amd.ops.decode import partials_numel

D = 128
SCALE = hd.scale_of(D)


# ------------------------------------------------------------------ one reference at head dim 64
def test_generic_references_equal_the_fixed_ones_at_64():
    assert hd.scale_of(64) == rd.SCALE
    for poison, use_rope in (("loud", True), ("nan", False)):
        H, Hkv, pos, (qkv, kc, vc) = rd.group_case(3, 640, poison, use_rope)
        H2, Hkv2, pos2, t2 = hd.group_case(3, 640, poison, use_rope, head_dim=64)
        assert (H, Hkv, pos) == (H2, Hkv2, pos2)
        for a, b in zip((qkv, kc, vc), t2):
            assert torch.equal(a.view(torch.int16), b.view(torch.int16))
        rope = rm.rope_tables_ref(640) if use_rope else None
        nch, chunk = rd.decode_plan(len(pos) * Hkv, 640)
        for emulate in (False, True):
            for mutant in (None,) + rd.DECODE_MUTANTS:
                if rope is None and mutant in ("rope_prev_pos", "rope_sign", "rope_k_unrotated"):
                    continue
                want = rd.decode_ref(qkv, kc, vc, pos, H, rd.SCALE, rope, emulate=emulate, mutant=mutant, chunk=chunk)
                got = hd.decode_ref(qkv, kc, vc, pos, H, rd.SCALE, rope, emulate=emulate, mutant=mutant, chunk=chunk)
                for a, b in zip(want, got):  # (as integers: NaN poison stays in the caches)
                    assert torch.equal(a.view(torch.int64), b.view(torch.int64)), (poison, emulate, mutant)
    for poison, use_rope in (("max", True), ("nan", False)):
        H, Hkv, pos, (qkv, k8, v8) = r8.group_case8(3, 320, poison, use_rope)
        _, _, pos2, t2 = hd.group_case8(3, 320, poison, use_rope, head_dim=64)
        assert pos == pos2
        for a, b in zip((qkv, k8, v8), t2):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
        rope = rm.rope_tables_ref(320) if use_rope else None
        for rmut in (None,) + r8.ROW_MUTANTS:
            want = r8.stored_rows8(qkv, pos, H, Hkv, rope, rmut)
            got = hd.stored_rows8(qkv, pos, H, Hkv, 64, rope, rmut)
            for a, b in zip(want, got):
                assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), rmut
        k16, v16, kn, vn = want = r8.stored_rows8(qkv, pos, H, Hkv, rope)
        for emulate in (False, True):
            for mutant in (None,) + r8.OUT_MUTANTS:
                a = r8.decode8_ref(qkv[:, : H * 64], k8, v8, kn, vn, pos, H, rd.SCALE, rope, emulate=emulate, mutant=mutant,
                                   new_bf16=(k16, v16))
                b = hd.decode8_ref(qkv[:, : H * 64], k8, v8, kn, vn, pos, H, rd.SCALE, rope, emulate=emulate, mutant=mutant,
                                   new_bf16=(k16, v16))
                assert torch.equal(a.view(torch.int64), b.view(torch.int64)), (poison, emulate, mutant)
    H, Hkv, pos, t = r8.saturating_case(True)
    H2, _, pos2, t2 = hd.saturating_case(True, head_dim=64)
    assert (H, pos) == (H2, pos2) and all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(t, t2))
    assert torch.equal(rd.sweep_history(513, 6)[1], hd.sweep_history(513, 6, head_dim=64)[1])


# ------------------------------------------------------------------ 128 against the package's references
@pytest.mark.parametrize("use_rope", [False, True])
@pytest.mark.parametrize("poison", ["loud", "nan"])
def test_package_references_match_fp64_at_128(use_rope, poison):
    Tmax, G = 320, 3
    H, Hkv, pos, (qkv, kc, vc) = hd.group_case(G, Tmax, poison, use_rope)
    assert kc.shape[-1] == D and qkv.shape[1] == (H + 2 * Hkv) * D
    qkv, kc, vc = qkv.float(), kc.float(), vc.float()
    rope = rm.rope_tables_ref(Tmax, D) if use_rope else None
    assert rope is None or rope[0].shape == (Tmax, D // 2)
    exact = hd.decode_ref(qkv, kc, vc, pos, H, SCALE, rope)
    k2, v2 = kc.clone(), vc.clone()
    out = ops.decode_attention_reference(qkv, k2, v2, torch.tensor(pos), H, None, rope)  # scale: D ** -0.5
    assert out.shape == (len(pos), H * D) and torch.isfinite(out).all()
    assert rm.tile_rel(hd.decode_per_head(out, H), hd.decode_per_head(exact[0], H), 1) < 1e-5
    for b, p in enumerate(pos):
        assert rm.tile_rel(k2[b, :, p], exact[1][b, :, p], 1) < 1e-6
        assert torch.equal(v2[b, :, p].double(), exact[2][b, :, p])
    # the shared-prefix reference on a split of the same caches: plen rows in the prefix, the rest own
    plen = [min(p, 17) for p in pos]
    Ts = Tmax
    own_k = torch.stack([torch.roll(kc[b], -plen[b], 1) for b in range(len(pos))])
    own_v = torch.stack([torch.roll(vc[b], -plen[b], 1) for b in range(len(pos))])
    out2 = ops.decode_attention_shared_reference(qkv, kc.clone(), vc.clone(), torch.tensor(plen), own_k, own_v,
                                                 torch.tensor(pos), 1, H, None, rope)
    assert rm.tile_rel(hd.decode_per_head(out2, H), hd.decode_per_head(exact[0], H), 1) < 1e-5
    for b, p in enumerate(pos):
        assert rm.tile_rel(own_k[b, :, p - plen[b]], exact[1][b, :, p], 1) < 1e-6


# ------------------------------------------------------------------ the mutants at 128
ROPE_MUTANTS = ("rope_prev_pos", "rope_sign", "rope_k_unrotated", "rope_partner_32", "rope_table_stride32")
CHUNK_MUTANTS = ("chunk_head_dropped", "merge_unweighted", "empty_chunk_live", "part_l_at_64")
HITS_K = ROPE_MUTANTS  # these move the stored k row too
CASES = ("group G3 T640 rope", "group G8 T640 plain", "group G1 T640 plain", "group G5 T320 rope",
         "sweep kv513 G3 launch 1", "sweep kv513 G6 launch 4")


def _scores(got, exact, H):
    return {"out": rm.tile_rel(hd.decode_per_head(got[0], H), hd.decode_per_head(exact[0], H), 1),
            "k_cache": rm.tile_rel(got[1], exact[1], 1)}


@functools.lru_cache(maxsize=None)
def _case(name):
    w = name.split()
    if w[0] == "group":
        G, Tmax, use_rope = int(w[1][1:]), int(w[2][1:]), w[3] == "rope"
        H, Hkv, pos, (qkv, kc, vc) = hd.group_case(G, Tmax, "loud", use_rope)
    else:
        Tmax, G, launch = int(w[1][2:]), int(w[2][1:]), int(w[4])
        assert hd.SWEEP_POISON[launch % 3] == "loud"
        H, Hkv, use_rope, pos = G, 1, True, hd.sweep_positions(Tmax, launch)
        qkv, kc, vc = hd.decode_poison(hd.sweep_history(Tmax, G), pos, "loud")
    rope = rm.rope_tables_ref(Tmax, D) if use_rope else None
    nch, chunk = hd.decode_plan(len(pos) * Hkv, Tmax)
    exact = hd.decode_ref(qkv, kc, vc, pos, H, SCALE, rope)
    emu = hd.decode_ref(qkv, kc, vc, pos, H, SCALE, rope, emulate=True)
    return (qkv, kc, vc, pos, H, Hkv, rope, nch, chunk), exact, _scores(emu, exact, H)


@pytest.mark.parametrize("name", CASES)
def test_floor_is_a_bf16_rounding_at_128(name):
    (_, _, _, _, _, _, rope, _, _), _, floor = _case(name)
    print(f"\ndecode 128 floor {name}", {n: f"{x:.2e}" for n, x in floor.items()})
    assert 1e-3 < floor["out"] < 1e-2, floor  # as at 64: one rounding of the output, the moved scores
    if rope is not None:
        assert 1e-3 < floor["k_cache"] < 4e-3, floor
    else:
        assert floor["k_cache"] == 0.0


@pytest.mark.parametrize("mutant", hd.DECODE_MUTANTS)
def test_decode_mutant_is_caught_at_128(mutant):
    ran = 0
    for name in CASES:
        (qkv, kc, vc, pos, H, Hkv, rope, nch, chunk), exact, floor = _case(name)
        if (mutant in ROPE_MUTANTS and rope is None) or (mutant in CHUNK_MUTANTS and nch == 1) or (
                mutant == "gqa_mod" and (Hkv == 1 or H == Hkv)) or (mutant == "out_high_neighbour" and H == 1):
            continue
        ran += 1
        got = hd.decode_ref(qkv, kc, vc, pos, H, SCALE, rope, emulate=True, mutant=mutant, chunk=chunk)
        score = _scores(got, exact, H)
        hits = ("out", "k_cache") if mutant in HITS_K else ("out",)
        print(f"\ndecode 128 {mutant:20s} {name}", {n: f"{score[n]:.2e} (floor {floor[n]:.2e})" for n in hits})
        for n in hits:
            assert score[n] >= 9 * floor[n] and score[n] > 0, (mutant, name, n, score[n], floor[n])
    assert ran >= 2, (mutant, ran)


@pytest.mark.parametrize("use_rope", [False, True])
def test_kv8_mutants_are_caught_at_128(use_rope):
    for G in (3, 6):
        H, Hkv, pos, (qkv, k8, v8) = hd.group_case8(G, 320, "max", use_rope)
        rope = rm.rope_tables_ref(320, D) if use_rope else None
        k16, v16, kn, vn = hd.stored_rows8(qkv, pos, H, Hkv, D, rope)
        q = qkv[:, : H * D]
        exact = hd.decode8_ref(q, k8, v8, kn, vn, pos, H, SCALE, rope)
        emu = hd.decode8_ref(q, k8, v8, kn, vn, pos, H, SCALE, rope, emulate=True)
        floor = rm.tile_rel(hd.decode_per_head(emu, H), hd.decode_per_head(exact, H), 1)
        assert 1e-3 < floor < 1e-2, floor
        for mutant in r8.OUT_MUTANTS + ("score_half_dims", "out_high_zero", "out_high_neighbour"):
            got = hd.decode8_ref(q, k8, v8, kn, vn, pos, H, SCALE, rope, emulate=True, mutant=mutant, new_bf16=(k16, v16))
            score = rm.tile_rel(hd.decode_per_head(got, H), hd.decode_per_head(exact, H), 1)
            print(f"\nkv8 128 {mutant:20s} G{G} rope {use_rope}: {score:.2e} (floor {floor:.2e})")
            assert score >= 9 * floor, (mutant, G, score, floor)
    # the row mutants change the stored bytes (the saturating inputs hold what the clamp is for)
    H, Hkv, pos, (qkv, k8, v8) = hd.saturating_case(use_rope)
    rope = rm.rope_tables_ref(320, D) if use_rope else None
    _, _, kn, vn = hd.stored_rows8(qkv, pos, H, Hkv, D, rope)
    _, _, k1, v1 = hd.stored_rows8(qkv, pos, H, Hkv, D, rope, "no_clamp")
    assert (r8.canon8(k1) != r8.canon8(kn)).any() and (r8.canon8(v1) != r8.canon8(vn)).any()
    if use_rope:
        Hq, Hk, p2, (q2, _, _) = hd.group_case8(3, 320, "max", True)
        _, _, ka, _ = hd.stored_rows8(q2, p2, Hq, Hk, D, rope)
        _, _, kb, _ = hd.stored_rows8(q2, p2, Hq, Hk, D, rope, "single_rounding")
        assert (r8.bits8(ka) != r8.bits8(kb)).any()


# ------------------------------------------------------------------ workspace
def test_partials_numel_takes_the_head_dim():
    assert partials_numel(2, 4, 1024, head_dim=128) == 2 * 4 * 8 * 129
    assert partials_numel(2, 4, 1024) == 2 * 4 * 8 * 65 == partials_numel(2, 4, 1024, 64)


def test_caches_size_their_workspace_with_the_head_dim():
    need = partials_numel(2, 4, 1024, head_dim=128)
    assert KVCache(1, 2, 4, 2, 1024, 128, device="cpu").workspace.numel() >= need
    assert SharedPrefixKVCache(1, 1, 2, 4, 2, 512, 512, 128, device="cpu").workspace.numel() >= need
    assert KVCache(1, 2, 4, 2, 1024, 64, device="cpu").workspace.numel() == 2 * 4 * 8 * 65


def test_routing_by_head_dim_on_the_cpu():
    q = torch.zeros(2, 8 * 128, dtype=torch.bfloat16)
    for d in (64, 96, 128):  # not on the GPU: never supported, whatever the head dim
        k = torch.zeros(2, 2, 8, d, dtype=torch.bfloat16)
        assert not ops.decode.decode_supported(q, k, 4) and not ops.decode.decode_shared_supported(q, k, k, 4)


# ------------------------------------------------------------------ generate at head dim 128 (CPU)
def _model():
    from nbdistributed_amd.models.llama import LlamaConfig, LlamaForCausalLM

    torch.manual_seed(0)
    m = LlamaForCausalLM(LlamaConfig.tiny(explicit_head_dim=128)).eval()
    assert m.kv_layout()[3] == 128
    with torch.no_grad():
        m.model.embed_tokens.weight.mul_(8.0)  # peaked logits: the best token is far from ties
    return m


def test_generate_at_128_on_the_cpu():
    m = _model()
    g = torch.Generator(device="cpu").manual_seed(1)
    ids = torch.randint(1, 512, (2, 12), generator=g)
    out = m.generate(ids, 6)
    assert out.shape == (2, 18) and torch.equal(out[:, :12], ids)
    with torch.no_grad():  # greedy = the arg-max of a teacher-forced forward
        logits = m(out[:, :-1]).logits
    assert torch.equal(logits[:, 11:].argmax(-1), out[:, 12:])
    assert torch.equal(m.generate(ids, 6, kv_dtype="fp8"), out)
    two = m.generate(ids, 6, num_return_sequences=2, top_k=1, temperature=1.0)
    assert torch.equal(two, out.repeat_interleave(2, 0))
