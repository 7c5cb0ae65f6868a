"""GPU: the key split of the block-append attention kernel — csrc/kernels/append.hip
``append_attn_kernel<D, true>`` + ``append_merge_kernel<D>`` — against the fp64 reference of
tests/refmath_append_hd.py, per 32-row tile, at head dims 64 and 128, on inputs whose cache rows
past ``start`` hold NaN.

The bound is tests/test_gpu_append_attn.py's rule, unchanged: ``floor = tile_rel(emulated reference,
fp64 reference)`` on the same inputs and ``tile_rel(kernel, fp64 reference) <= 3 x floor``.  Run with
``-s`` for every kernel/floor ratio and, at the end, the worst one (docs/FINDINGS.md §48 keeps the
last recorded figure)."""
import copy
import functools
import math
from unittest import mock

import pytest
import torch

import refmath as rm
import refmath_append_hd as hd
from nbdistributed_amd import ops
from nbdistributed_amd.generation import generate

pytestmark = pytest.mark.gpu

TMAX = 384  # six 64-key tiles: key_splits=6 is one tile per chunk, key_splits=2 is three
START = (0, 50, 100, 300)
WORST = [0.0, ""]


@pytest.fixture(scope="module")
def dev(require_gpu):
    assert ops.native_available(), ops._load_error
    yield torch.device("cuda", 0)
    print(f"\nworst split append kernel/floor ratio (bound 3): {WORST[0]:.2f}  {WORST[1]}")


def _bits(t):
    return t.contiguous().view(torch.int16)


def _note(case, err, floor):
    ratio = err / floor if floor > 0 else (0.0 if err == 0 else math.inf)
    print(f"  {case}: kernel {err:.3e} floor {floor:.3e} ratio {ratio:.2f}")
    if ratio > WORST[0]:
        WORST[0], WORST[1] = ratio, case
    return err <= 3 * floor


@functools.lru_cache(maxsize=None)
def _case(D, H, Hkv, Tn, use_rope, Tmax=TMAX, start=START, nnew=None, B=4):
    """inputs and both references of one shape, computed once for every ``key_splits`` that runs it"""
    nnew = nnew or (Tn, Tn, 1, min(Tn, 84))
    qkv, kc, vc = hd.append_inputs(B, H, Hkv, Tn, Tmax, start, 100 * D + Tn + H, poison="nan", head_dim=D)
    rope = ops.rope_tables(Tmax, D, 10000.0, "cuda") if use_rope else None
    rope_cpu = None if rope is None else (rope[0].cpu(), rope[1].cpu())
    exact = hd.append_ref(qkv, kc, vc, start, nnew, H, hd.scale_of(D), rope_cpu)
    emu = hd.append_ref(qkv, kc, vc, start, nnew, H, hd.scale_of(D), rope_cpu, emulate=True)
    floor = rm.tile_rel(hd.per_head(emu[0], H, D), hd.per_head(exact[0], H, D), 32)
    return qkv, kc, vc, start, nnew, rope, exact, floor


def _run_and_check(dev, name, case, H, key_splits):
    """one kernel call on device copies: the figure printed, then every check; returns the output"""
    qkv, kc, vc, start, nnew, rope, exact, floor = case
    D = kc.shape[-1]
    Hkv = kc.shape[1]
    kd, vd = kc.to(dev), vc.to(dev)
    st, nn = (torch.tensor(x, dtype=torch.int64, device=dev) for x in (start, nnew))
    out = ops.append_attention(qkv.to(dev), kd, vd, st, nn, H, scale=hd.scale_of(D), rope=rope, key_splits=key_splits)
    torch.cuda.synchronize()
    out, kd, vd = out.cpu(), kd.cpu(), vd.cpu()
    ok = _note(name, rm.tile_rel(hd.per_head(out, H, D), hd.per_head(exact[0], H, D), 32), floor)
    assert torch.isfinite(out).all(), name
    for b in range(len(start)):
        s0, n = start[b], nnew[b]
        assert (_bits(out[b, n:]) == 0).all(), (name, b)  # padding rows: exact zeros
        for new, old in ((kd, kc), (vd, vc)):  # nothing but rows [start, start + nnew) was written
            assert torch.equal(_bits(new[b, :, s0 + n:]), _bits(old[b, :, s0 + n:])), (name, b)
            assert torch.equal(_bits(new[b, :, :s0]), _bits(old[b, :, :s0])), (name, b)
        v_new = qkv[b, :n, (H + Hkv) * D:].reshape(n, Hkv, D).transpose(0, 1)
        assert torch.equal(_bits(vd[b, :, s0:s0 + n]), _bits(v_new)), (name, b)
    assert ok, (name, "tile_rel above 3 x floor")
    return out


# ================================================================================ 1. forced splits
FORCED = [(D, 9, 3, True, ks, Tn) for D in (64, 128) for ks in (2, 6) for Tn in (1, 40, 130)] + [(64, 4, 4, False, 6, 130)]


@pytest.mark.parametrize("D,H,Hkv,use_rope,key_splits,Tn", FORCED)
def test_forced_split_offsets_and_poison(dev, D, H, Hkv, use_rope, key_splits, Tn):
    """start 0: an empty history, most chunks exit early; 50 with Tn 40: the diagonal crosses the
    key-64 chunk edge inside a wave; 100 with one real row: padding beside a live row; 300 with 84
    rows: across key 320 inside a wave and up to the cache's last row."""
    case = _case(D, H, Hkv, Tn, use_rope)
    _run_and_check(dev, f"D{D} H{H}/{Hkv} Tn{Tn} splits{key_splits}", case, H, key_splits)
    assert ops.append_key_splits(4, H, Tn, TMAX, D) == 1  # 384 keys: the default call is the unsplit kernel
    one = _run_and_check(dev, f"D{D} H{H}/{Hkv} Tn{Tn} splits1", case, H, 1)
    assert torch.equal(_bits(one), _bits(_run_and_check(dev, f"D{D} H{H}/{Hkv} Tn{Tn} default", case, H, None)))


# ================================================================================ 2. the plan
def test_plan(dev):
    for D in (64, 128):
        assert all(ops.append_key_splits(1, 9, 33, kv, D) == 1 for kv in (1, 64, 511, 512))
        assert ops.append_key_splits(8, 32, 512, 4096, D) == 1  # 8 · 32 · 4 = 1024 workgroups fill the chip
    assert ops.append_key_splits(1, 9, 33, 4096, 64) > 1
    assert ops.append_key_splits(1, 24, 33, 4096, 128) > 1


@pytest.mark.parametrize("D", [64, 128])
def test_default_path_splits_a_long_history(dev, D):
    """Tmax = kv_len_max = 1024, one sequence, 4 / 2 heads, 33 new tokens at start 900: nobody asks
    for a split and the plan takes one."""
    assert ops.append_key_splits(1, 4, 33, 1024, D) > 1
    case = _case(D, 4, 2, 33, True, Tmax=1024, start=(900,), nnew=(33,), B=1)
    _run_and_check(dev, f"D{D} default at 1024 keys", case, 4, None)


# ================================================================================ 3. graph capture
def test_graph_replay_after_the_block_moved_across_a_chunk_edge(dev):
    """one captured call with six one-tile chunks; ``start`` / ``nnew`` then move in place from
    blocks inside a chunk to blocks that cross chunk edges.  The replay is the eager call on the
    same inputs, bit for bit: output and caches."""
    D, B, H, Hkv, Tn = 128, 3, 6, 2, 40
    first, second = ((10, 3, 200), (5, 40, 1)), ((40, 63, 290), (40, 2, 40))
    qkv, kc, vc = hd.append_inputs(B, H, Hkv, Tn, TMAX, second[0], 21, poison="nan", head_dim=D)
    rope = ops.rope_tables(TMAX, D, 10000.0, dev)
    qd, kd, vd = qkv.to(dev), kc.to(dev), vc.to(dev)
    st, nn = (torch.tensor(x, dtype=torch.int64, device=dev) for x in first)
    call = lambda k, v: ops.append_attention(qd, k, v, st, nn, H, scale=hd.scale_of(D), rope=rope, key_splits=6)  # noqa: E731
    call(kd, vd)  # warm-up
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call(kd, vd)
    torch.cuda.synchronize()
    kd.copy_(kc)
    vd.copy_(vc)
    st.copy_(torch.tensor(second[0], dtype=torch.int64))
    nn.copy_(torch.tensor(second[1], dtype=torch.int64))
    graph.replay()
    torch.cuda.synchronize()
    k2, v2 = kc.to(dev), vc.to(dev)
    eager = call(k2, v2)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    assert torch.equal(_bits(out.cpu()), _bits(eager.cpu()))
    assert torch.equal(_bits(kd.cpu()), _bits(k2.cpu())) and torch.equal(_bits(vd.cpu()), _bits(v2.cpu()))


# ================================================================================ 4. model level
LENS1, NEW1 = (700, 660, 620, 615), 8  # 707 held rows + 1 + 32: twelve tiles, where the plan starts to split
LENS2, NEW2 = (7, 1, 32, 20), 8
T_MAX = 768


@pytest.mark.parametrize("D", [64, 128])
def test_model_second_turn_over_a_long_history(dev, D):
    """``generate(turn, n, cache=cache)`` over ~700 held rows: the plan splits the turn's attention.
    Its first logits lie within 5 % of the largest |logit| of the full forward
    (test_gpu_generate_continue.py's bound); the tokens are the same with the graph on and off, and
    the same as with the module default set to never split."""
    from nbdistributed_amd.models.llama import LlamaConfig, LlamaForCausalLM

    torch.manual_seed(0)
    m = LlamaForCausalLM(LlamaConfig.tiny(explicit_head_dim=D)).to(dev, torch.bfloat16).eval()
    with torch.no_grad():
        m.model.embed_tokens.weight.mul_(8.0)  # test_gpu_decode.py's _peaked gain
    B = len(LENS1)
    g = torch.Generator(device="cuda").manual_seed(1)
    ids1 = torch.randint(1, 512, (B, max(LENS1)), device=dev, generator=g)
    ids2 = torch.randint(1, 512, (B, max(LENS2)), device=dev, generator=g)
    l1, l2 = torch.tensor(LENS1, device=dev), torch.tensor(LENS2, device=dev)
    assert ops.append_key_splits(B, 4, max(LENS2) + 1, max(LENS1) + NEW1 + max(LENS2) + 1, D) > 1
    outs = {}
    for arm, graph, splits in (("eager", False, 0), ("graph", True, 0), ("unsplit", True, 1)):
        with mock.patch.object(ops.decode, "APPEND_KEY_SPLITS", splits):
            out1, cache = generate(m, ids1, NEW1, lengths=l1, t_max=T_MAX, graph=graph, return_cache=True)
            if arm == "eager":  # the block's logits, on a copy of the cache state the turn starts from
                c2 = copy.copy(cache)
                c2.k, c2.v = cache.k.clone(), cache.v.clone()
                chunk = torch.cat([cache.pending.view(B, 1), ids2], 1)
                first = m.extend(chunk, c2, cache.lengths.clone(), l2 + 1).float()
            outs[arm] = (out1, generate(m, ids2, NEW2, lengths=l2, cache=cache, graph=graph))
    for arm in ("graph", "unsplit"):
        assert torch.equal(outs["eager"][0], outs[arm][0]) and torch.equal(outs["eager"][1], outs[arm][1]), arm
    out1 = outs["eager"][0]
    assert torch.isfinite(first).all()
    for b in range(B):
        hist = out1[b, :LENS1[b] + NEW1].tolist() + ids2[b, :LENS2[b]].tolist()
        with torch.no_grad():
            full = m(torch.tensor([hist], device=dev))[1][0, -1].float()
        d = (first[b] - full).abs().max().item()
        print(f"  D{D} row {b}: first-logit max|Δ| {d:.4f} of max|full| {full.abs().max().item():.3f}")
        assert d < 0.05 * full.abs().max().item()
