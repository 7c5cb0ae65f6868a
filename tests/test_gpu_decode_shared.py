"""GPU: decode attention over a shared prefix plus own rows — ``decode_attn_shared``,
csrc/kernels/decode.hip ``decode_kernel<G, F8, true>`` — and ``generate(num_return_sequences=R)``.

The shared instantiations share every line of floating-point code with the unshared ones and
differ only in the address of a key, so the first rule is *bit equality* with the unshared op
(``decode_attn``, unchanged by this path) on the materialised cache — one private cache of
Tp + Ts rows per sequence, ``refmath_shared.materialise`` — under the same ``kv_len_max``: the
output, the new row (at ``own[s, :, pos - plen]``), every other own row and every prefix byte
untouched.  Compared as integers: everything the op must not read holds poison.
tests/test_shared_prefix_ref.py shows on the CPU that each wrong addressing rule breaks this
equality.  The second rule is the project's: ``tile_rel(kernel, fp64 reference) <= 3 x floor`` per
head row on the materialised cache (``refmath_decode.decode_ref``; on fp8 the stored bytes are
dequantised exactly and the new row is taken as stored, ``refmath_kv8.decode8_ref``, as
tests/test_gpu_kv8.py does).  Run with ``-s`` for every kernel/floor ratio."""
import math

import pytest
import torch

import refmath as rm
import refmath_decode as rd
import refmath_kv8 as r8
import refmath_shared as rs
from nbdistributed_amd import ops
from nbdistributed_amd.generation import KVCache, SharedPrefixKVCache
from nbdistributed_amd.ops.decode import partials_numel

pytestmark = pytest.mark.gpu

SCALE = rd.SCALE
HKV = rd.GROUP_HKV
TP = 320
EDGES = (223, 224, 225, 447, 448, 449)  # both edges of the three 224-key chunks of 640 keys, from both sides
WORST = [0.0, ""]


@pytest.fixture(scope="module")
def dev(require_gpu):
    assert ops.native_available(), ops._load_error
    yield torch.device("cuda", 0)
    print(f"\nworst shared decode kernel/floor ratio (bound 3): {WORST[0]:.2f}  {WORST[1]}")


def _positions(plen, group, Ts, launch):
    """``group`` absolute positions per prompt in [plen, plen + Ts - 1], rotating with the launch
    through: the first own row, the last one, the chunk-edge positions in reach, rows in between."""
    pos = []
    for b, pl in enumerate(plen):
        cand = [pl, pl + Ts - 1] + [e for e in EDGES if pl <= e < pl + Ts]
        cand += [pl + (37 * b + 61 * r + 101 * launch + 13) % Ts for r in range(group)]
        pos += [cand[(launch + b + r) % len(cand)] for r in range(group)]
    return pos


def _launch_case(G, group, fp8, Ts, launch, S_target=12):
    """the ``launch``-th case of a sweep: B = ⌈12 / group⌉ prompts whose plen walk through
    ``refmath_shared.PLENS``; the poison kind changes with the launch."""
    B = -(-S_target // group)
    plen = [rs.PLENS[(launch * B + b) % len(rs.PLENS)] for b in range(B)]
    pos = _positions(plen, group, Ts, launch)
    poison = "nan" if launch % 2 == 0 else ("max" if fp8 else "loud")
    seed = 7000 + 100 * G + 10 * group + launch + (5 if fp8 else 0)
    return plen, pos, poison, rs.shared_case(B, group, G * HKV, HKV, TP, Ts, plen, pos, seed, poison, fp8)


def _check_shared(dev, case, G, group, plen, pos, tensors, rope_dev, kv_len_max=None, run=None, check_fp64=True):
    """one ``decode_attn_shared`` call on device copies of (qkv, prefix, own) against ``decode_attn``
    on the materialised cache, then against the fp64 reference.  ``run``: replaces the shared call
    (graph replay); it returns (out, pre_k, pre_v, own_k, own_v) on the device."""
    qkv, pk, pv, ok, ov = tensors
    H = G * HKV
    S, Ts = ok.shape[0], ok.shape[2]
    T = TP + Ts
    fp8 = ok.dtype == rs.F8
    pl = rs.per_sequence(plen, group)
    si, pt = torch.arange(S), torch.as_tensor(pos)
    km, vm = rs.materialise(pk, ok, plen, group), rs.materialise(pv, ov, plen, group)
    ws = torch.empty(partials_numel(S, H, T), dtype=torch.float32, device=dev)
    # the yardstick: the unshared op, same key bound
    kmd, vmd = km.to(dev), vm.to(dev)
    want = ops.decode_attention(qkv.to(dev), kmd, vmd, pt.to(dev), H, scale=SCALE, rope=rope_dev,
                                kv_len_max=kv_len_max or T, workspace=ws)
    torch.cuda.synchronize()
    want, kmd, vmd = want.cpu(), kmd.cpu(), vmd.cpu()
    if run is None:
        pkd, pvd, okd, ovd = (t.to(dev) for t in (pk, pv, ok, ov))
        out = ops.decode_attention_shared(qkv.to(dev), pkd, pvd, torch.as_tensor(plen).to(dev), okd, ovd, pt.to(dev),
                                          group, H, scale=SCALE, rope=rope_dev, kv_len_max=kv_len_max, workspace=ws)
    else:
        out, pkd, pvd, okd, ovd = run()
    torch.cuda.synchronize()
    out, pkd, pvd, okd, ovd = (t.cpu() for t in (out, pkd, pvd, okd, ovd))
    assert out.shape == (S, H * 64) and out.dtype == torch.bfloat16
    # 1. bit equality with the unshared kernel
    diff = rs.raw(out) != rs.raw(want)
    assert not diff.any(), (case, "output bits differ from decode_attn on the materialised cache",
                            sorted(set(diff.nonzero()[:, 0].tolist())))
    for what, new, old, mat, pre_new, pre_old in (("k", okd, ok, kmd, pkd, pk), ("v", ovd, ov, vmd, pvd, pv)):
        assert torch.equal(rs.raw(new)[si, :, pt - pl], rs.raw(mat)[si, :, pt]), (case, what, "new row bits differ")
        keep = rs.raw(old).clone()
        keep[si, :, pt - pl] = rs.raw(new)[si, :, pt - pl]
        assert torch.equal(rs.raw(new), keep), (case, what, "an own row other than pos - plen was written")
        assert torch.equal(rs.raw(pre_new), rs.raw(pre_old)), (case, what, "a prefix byte changed")
    assert torch.isfinite(out.float()).all(), case
    if not check_fp64:
        return
    # 2. the fp64 reference on the materialised cache: tile_rel <= 3 x floor per head row
    rope_cpu = None if rope_dev is None else (rope_dev[0].cpu(), rope_dev[1].cpu())
    if fp8:
        q = qkv[:, : H * 64]
        kn, vn = okd[si, :, pt - pl], ovd[si, :, pt - pl]
        exact = r8.decode8_ref(q, km, vm, kn, vn, pos, H, SCALE, rope_cpu)
        emu = r8.decode8_ref(q, km, vm, kn, vn, pos, H, SCALE, rope_cpu, emulate=True)
    else:
        exact = rd.decode_ref(qkv, km, vm, pos, H, SCALE, rope_cpu)[0]
        emu = rd.decode_ref(qkv, km, vm, pos, H, SCALE, rope_cpu, emulate=True)[0]
    floor = rm.tile_rel(rd.decode_per_head(emu, H), rd.decode_per_head(exact, H), 1)
    err = rm.tile_rel(rd.decode_per_head(out, H), rd.decode_per_head(exact, H), 1)
    ratio = err / floor if floor > 0 else (0.0 if err == 0 else math.inf)
    print(f"  shared decode {case}: kernel {err:.3e} floor {floor:.3e} ratio {ratio:.2f}")
    if ratio > WORST[0]:
        WORST[0], WORST[1] = ratio, case
    assert err <= 3 * floor, (case, "tile_rel above 3 x floor", err, floor)


@pytest.mark.parametrize("use_rope", [False, True], ids=["plain", "rope"])
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("group", [1, 2, 5])
@pytest.mark.parametrize("G", [1, 3, 4, 6, 8])
def test_shared_decode_equals_the_unshared_kernel(dev, G, group, fp8, use_rope):
    """Tp = Ts = 320: 640 logical keys in three chunks of 224.  Over the launches of a case every
    plen of ``PLENS`` occurs — the 32-group edge, the iteration edges of both U, a chunk edge from
    both sides, an empty and a full prefix — with a dozen (group 5: 15) positions per launch from
    pos == plen (first own row) over the chunk edges to the last own row."""
    Ts = 320
    launches = -(-len(rs.PLENS) // -(-12 // group)) + 1
    S = -(-12 // group) * group
    assert rd.decode_plan(S * HKV, TP + Ts) == (3, 224)
    rope = ops.rope_tables(TP + Ts, 64, 10000.0, dev) if use_rope else None
    seen_plen, seen_own = set(), set()
    for launch in range(launches):
        plen, pos, poison, tensors = _launch_case(G, group, fp8, Ts, launch)
        _check_shared(dev, f"G{G} group {group} {'fp8' if fp8 else 'bf16'} {'rope' if use_rope else 'plain'} "
                           f"launch {launch} {poison}", G, group, plen, pos, tensors, rope)
        seen_plen.update(plen)
        seen_own.update(p - q for p, q in zip(pos, rs.per_sequence(plen, group).tolist()))
    assert seen_plen == set(rs.PLENS)
    assert {0, Ts - 1} <= seen_own


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("G", [1, 3, 4, 6, 8])
def test_shared_decode_unsplit(dev, G, fp8):
    """Tp = 320, Ts = 192: 512 logical keys, the last bound ``plan()`` leaves in one chunk (no
    partials, no merge kernel); and a host bound of 300 keys below it."""
    Ts, group = 192, 2
    assert rd.decode_plan(12 * HKV, TP + Ts) == (1, 512)
    rope = ops.rope_tables(TP + Ts, 64, 10000.0, dev)
    for launch in range(2):
        plen, pos, poison, tensors = _launch_case(G, group, fp8, Ts, launch)
        _check_shared(dev, f"unsplit G{G} {'fp8' if fp8 else 'bf16'} launch {launch} {poison}", G, group, plen, pos,
                      tensors, rope)
    plen = [0, 1, 33, 127, 128, 224]
    pos = [0, 191, 1, 192, 33, 224, 127, 299, 128, 299, 224, 298]
    tensors = rs.shared_case(6, group, G * HKV, HKV, TP, Ts, plen, pos, 8000 + G, "nan", fp8)
    _check_shared(dev, f"bound 300 G{G} {'fp8' if fp8 else 'bf16'}", G, group, plen, pos, tensors, rope, kv_len_max=300)


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_shared_decode_graph_replay(dev, fp8):
    """one captured step (``decode_attention_shared``, then pos += 1 on the device) replayed four
    times: sequences 0 and 1 go from own row 0 to 3 and across the 224 chunk edge (into a chunk
    that was empty), sequences 2 and 3 across the 448 edge.  Every replay is checked like an eager
    call, against the caches as they then stand."""
    G, group, Ts = 3, 2, 320
    H = G * HKV
    plen, start = [222, 200], (222, 223, 446, 447)
    assert rd.decode_plan(4 * HKV, TP + Ts) == (3, 224)
    rope = ops.rope_tables(TP + Ts, 64, 10000.0, dev)
    q0, pk, pv, ok, ov = rs.shared_case(2, group, H, HKV, TP, Ts, plen, start, 99, "nan", fp8)
    pkd, pvd, okd, ovd, qd = (t.to(dev) for t in (pk, pv, ok, ov, q0))
    pld = torch.tensor(plen, dtype=torch.int64, device=dev)
    pd = torch.tensor(start, dtype=torch.int64, device=dev)
    ws = torch.empty(partials_numel(4, H, TP + Ts), dtype=torch.float32, device=dev)
    step = lambda: ops.decode_attention_shared(qd, pkd, pvd, pld, okd, ovd, pd, group, H, scale=SCALE, rope=rope,  # noqa: E731
                                               workspace=ws)
    step()  # warm-up
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
        pd.add_(1)
    torch.cuda.synchronize()
    okd.copy_(ok)  # (capture launches nothing; the warm-up wrote its rows)
    ovd.copy_(ov)
    pd.copy_(torch.tensor(start, dtype=torch.int64))
    g = torch.Generator(device="cpu").manual_seed(5)
    for i in range(4):
        pos = tuple(s + i for s in start)
        qkv = (q0.float() + 0.5 * torch.randn(q0.shape, generator=g)).bfloat16()  # a new token's projection
        qd.copy_(qkv)
        before = (qkv, pk, pv, okd.cpu(), ovd.cpu())

        def run():
            graph.replay()
            return out, pkd, pvd, okd, ovd

        _check_shared(dev, f"graph {'fp8' if fp8 else 'bf16'} step {i} pos {pos}", G, group, plen, pos, before, rope, run=run)
        assert pd.cpu().tolist() == [p + 1 for p in pos]


def test_shared_decode_checks_its_operands(dev):
    """prefix and own caches of one dtype; the prefix batch is S / group; kv_len_max <= Tp + Ts."""
    B, group, H, Tp, Ts = 2, 3, 4, 64, 32
    S = B * group
    z = lambda *shape, dt=torch.bfloat16: torch.zeros(*shape, dtype=dt, device=dev)  # noqa: E731
    qkv, pos, plen = z(S, (H + 2 * HKV) * 64), z(S, dt=torch.int64), z(B, dt=torch.int64)
    ws = z(partials_numel(S, H, Tp + Ts), dt=torch.float32)
    call = lambda pk, ok, group=group, bound=Tp + Ts: torch.ops.nbd.decode_attn_shared(  # noqa: E731
        qkv, pk, pk.clone(), plen, ok, ok.clone(), pos, group, H, 0.125, bound, None, None, ws)
    p16, o16 = z(B, HKV, Tp, 64), z(S, HKV, Ts, 64)
    p8, o8 = z(B, HKV, Tp, 64, dt=rs.F8), z(S, HKV, Ts, 64, dt=rs.F8)
    with pytest.raises(RuntimeError, match="prefix and own caches must have the same dtype"):
        call(p8, o16)
    with pytest.raises(RuntimeError, match="prefix and own caches must have the same dtype"):
        call(p16, o8)
    with pytest.raises(RuntimeError, match=r"prefix caches must be \[B / group, Hkv, Tp, 64\]"):
        call(p16, o16, group=2)
    with pytest.raises(RuntimeError, match=r"kv_len_max must be in \[1, Tp \+ Ts\]"):
        call(p16, o16, bound=Tp + Ts + 1)
    assert call(p16, o16).shape == (S, H * 64) and call(p8, o8).shape == (S, H * 64)
    assert call(z(B, HKV, 0, 64), o16, bound=Ts).shape == (S, H * 64)  # no prefix rows at all
    torch.cuda.synchronize()


# ================================================================================ model level
def _peaked(model):
    # scale the embedding (tied LM head) so the best token is far from ties under bf16 rounding
    with torch.no_grad():
        emb = model.wte.weight if hasattr(model, "wte") else model.model.embed_tokens.weight
        emb.mul_(8.0)
    return model


def _gpu_model(family):
    from nbdistributed_amd.models import GPT2, GPT2Config
    from nbdistributed_amd.models.llama import LlamaConfig, LlamaForCausalLM

    torch.manual_seed(0)
    if family == "gpt2":
        m = GPT2(GPT2Config(vocab_size=512, n_positions=512, n_embd=256, n_layer=2, n_head=4))
    else:
        m = LlamaForCausalLM(LlamaConfig.tiny())  # head dim 64, 4 query heads on 2 kv heads
    return m.to("cuda", torch.bfloat16).eval()


@pytest.mark.parametrize("kv_dtype", [None, rs.F8], ids=["kv-bf16", "kv-fp8"])
@pytest.mark.parametrize("family", ["gpt2", "llama"])
def test_shared_decode_step_logits_are_bit_equal(dev, family, kv_dtype):
    """B = 2 ragged prompts prefilled once into a ``KVCache`` and once into a
    ``SharedPrefixKVCache`` with group 3; the ``KVCache`` rows copied into an unshared batch-6 cache
    of the same ``t_max``; six teacher-forced ``decode_step`` calls on both: equal logits, bit for bit."""
    m = _gpu_model(family)
    B, R, Tp, Ts = 2, 3, 128, 16
    g = torch.Generator(device="cpu").manual_seed(1)
    ids = torch.randint(1, 512, (B, Tp), generator=g).to(dev)
    lens = torch.tensor([40, 17], device=dev)
    one = KVCache.for_model(m, B, Tp + Ts, dtype=kv_dtype)
    shared = SharedPrefixKVCache.for_model(m, B, R, Tp, Ts, dtype=kv_dtype)
    la = m.prefill(ids, one, lens)
    lb = m.prefill(ids, shared, lens)
    shared.plen.copy_(lens)
    assert torch.equal(la, lb)
    for a, b in ((one.k, shared.k), (one.v, shared.v)):
        assert torch.equal(rs.raw(a[:, :, :, :Tp].cpu()), rs.raw(b.cpu()))
    six = KVCache.for_model(m, B * R, Tp + Ts, dtype=kv_dtype)
    rs.raw(six.k).copy_(rs.raw(one.k).repeat_interleave(R, 1))  # (as integers: e4m3fn has no repeat_interleave)
    rs.raw(six.v).copy_(rs.raw(one.v).repeat_interleave(R, 1))
    assert shared.t_max == six.t_max and shared.nbytes < six.nbytes
    pos = lens.repeat_interleave(R)
    for step in range(6):
        tok = torch.randint(1, 512, (B * R,), generator=g).to(dev)
        want = m.decode_step(tok, pos + step, six)
        got = m.decode_step(tok, pos + step, shared)
        torch.cuda.synchronize()
        assert got.shape == want.shape and torch.equal(rs.raw(got.cpu()), rs.raw(want.cpu())), (family, step)
    # the prefix is what the prefill left; the samples' rows are the unshared cache's rows from plen on
    for a, b in ((one.k, shared.k), (one.v, shared.v)):
        assert torch.equal(rs.raw(a[:, :, :, :Tp].cpu()), rs.raw(b.cpu()))
    for s in range(B * R):
        n = int(lens[s // R])
        assert torch.equal(rs.raw(shared.k_own[:, s, :, :6].cpu()), rs.raw(six.k[:, s, :, n:n + 6].cpu()))
        assert torch.equal(rs.raw(shared.v_own[:, s, :, :6].cpu()), rs.raw(six.v[:, s, :, n:n + 6].cpu()))


@pytest.mark.parametrize("kv_dtype", [None, "fp8"], ids=["kv-bf16", "kv-fp8"])
@pytest.mark.parametrize("family", ["gpt2", "llama"])
def test_shared_generate_top1_is_deterministic(dev, family, kv_dtype):
    """``top_k=1`` leaves one candidate, so sampling is deterministic: the four samples of a prompt
    are identical, and graph on equals graph off token for token."""
    m = _peaked(_gpu_model(family))
    ids = torch.randint(1, 512, (3, 40), device=dev)
    lens = torch.tensor([40, 33, 1], device=dev)
    kw = dict(lengths=lens, temperature=1.0, top_k=1, num_return_sequences=4, kv_dtype=kv_dtype)
    eager, cache = m.generate(ids, 24, graph=False, return_cache=True, **kw)
    graphed = m.generate(ids, 24, graph=True, **kw)
    assert isinstance(cache, SharedPrefixKVCache) and cache.k.is_cuda and cache.is_fp8 == (kv_dtype is not None)
    assert (cache.t_prefix, cache.t_own, cache.group) == (128, 24, 4)
    assert eager.shape == (12, 64) and torch.equal(eager, graphed)
    rows = eager.view(3, 4, 64)
    assert torch.equal(rows, rows[:, :1].expand(3, 4, 64))
    greedy = m.generate(ids, 24, lengths=lens, kv_dtype=kv_dtype)  # the unshared greedy path: the same tokens
    assert torch.equal(rows[:, 0], greedy)


def test_shared_generate_sampled(dev):
    """a sampled run: the shape, the prompts preserved, new tokens from lengths[b] on, eos then
    padding, and different samples within a group."""
    m = _gpu_model("llama")
    B, R, T0, NEW = 3, 4, 40, 24
    ids = torch.randint(1, 512, (B, T0), device=dev)
    lens = torch.tensor([40, 33, 1], device=dev)
    torch.manual_seed(3)
    free = m.generate(ids, NEW, lengths=lens, temperature=1.0, top_k=50, num_return_sequences=R).cpu()
    assert free.shape == (B * R, T0 + NEW)
    rows = free.view(B, R, -1)
    for b, n in enumerate(lens.tolist()):
        assert torch.equal(rows[b, :, :n], ids[b, :n].cpu().expand(R, n))
        assert ((rows[b, :, n:n + NEW] >= 0) & (rows[b, :, n:n + NEW] < 512)).all()
        assert (rows[b, :, n + NEW:] == 0).all()
        assert any(not torch.equal(rows[b, 0], rows[b, r]) for r in range(1, R)), b
    eos = int(free[0, 40])  # a token that occurs: the first new token of sequence 0, drawn before the loop
    torch.manual_seed(3)
    out = m.generate(ids, NEW, lengths=lens, temperature=1.0, top_k=50, num_return_sequences=R, eos_token_id=eos,
                     pad_token_id=7, sync_every=4).cpu()
    assert out.shape == (B * R, T0 + NEW)
    lens_s = lens.repeat_interleave(R).tolist()
    hit = 0
    for s, n in enumerate(lens_s):
        new = out[s, n:n + NEW].tolist()
        assert torch.equal(out[s, :n], ids[s // R, :n].cpu())
        if eos in new:  # eos, then eos until the loop stopped, then padding
            hit += 1
            tail = new[new.index(eos):]
            assert all(t in (eos, 7) for t in tail) and tail == sorted(tail, key=lambda t: t != eos), (s, tail)
        assert (out[s, n + NEW:] == 7).all()
    assert hit >= 1
