"""GPU: head dim 128 in the block-append attention kernel — csrc/kernels/append.hip
``append_kv_kernel<128>`` and ``append_attn_kernel<128>`` — against the fp64 reference of
tests/refmath_append_hd.py, per 32-row tile (one wave's queries of one head) on structured inputs
whose cache rows past ``start`` hold poison: huge finite values, then NaN.

The bound is tests/test_gpu_append_attn.py's rule, unchanged: ``floor = tile_rel(emulated
reference, fp64 reference)`` on the same inputs and ``tile_rel(kernel, fp64 reference) <= 3 x
floor``.  tests/test_append_hd_ref.py shows on the CPU that wrong formulas — those a 128 kernel can
be where a 64 one cannot included — score >= 9 x floor on these inputs.  Run with ``-s`` for every
kernel/floor ratio and, at the end, the worst one (docs/FINDINGS.md keeps the last recorded figure)."""
import contextlib
import copy
import math
from unittest import mock

import pytest
import torch

import refmath as rm
import refmath_append_hd as hd
from nbdistributed_amd import ops
from nbdistributed_amd.generation import KVCache, generate

pytestmark = pytest.mark.gpu

D = 128
SCALE = hd.scale_of(D)
TMAX = hd.TMAX
WORST = [0.0, ""]


@pytest.fixture(scope="module")
def dev(require_gpu):
    assert ops.native_available(), ops._load_error
    yield torch.device("cuda", 0)
    print(f"\nworst head-dim-128 append kernel/floor ratio (bound 3): {WORST[0]:.2f}  {WORST[1]}")


def _bits(t):
    return t.contiguous().view(torch.int16)


def _note(case, err, floor):
    ratio = err / floor if floor > 0 else (0.0 if err == 0 else math.inf)
    print(f"  {case}: kernel {err:.3e} floor {floor:.3e} ratio {ratio:.2f}")
    if ratio > WORST[0]:
        WORST[0], WORST[1] = ratio, case
    return err <= 3 * floor


def _rope(T, dev):
    cos, sin = ops.rope_tables(T, D, 10000.0, dev)
    assert cos.shape == (T, D // 2)
    return cos, sin


def _refs(qkv, kc, vc, start, nnew, H, rope):
    rope_cpu = None if rope is None else (rope[0].cpu(), rope[1].cpu())
    exact = hd.append_ref(qkv, kc, vc, start, nnew, H, SCALE, rope_cpu)
    emu = hd.append_ref(qkv, kc, vc, start, nnew, H, SCALE, rope_cpu, emulate=True)
    return exact, emu, rm.tile_rel(hd.per_head(emu[0], H, D), hd.per_head(exact[0], H, D), 32)


def _run_and_check(dev, case, qkv, kc, vc, start, nnew, H, rope, exact, emu, floor, raw=None):
    """one kernel call on device copies of (qkv, kc, vc): every figure printed, then every check.
    ``raw``: the start / nnew handed to the kernel when they differ from the clamped ones."""
    B, Tn, _ = qkv.shape
    Hkv = kc.shape[1]
    kd, vd = kc.to(dev), vc.to(dev)
    st, nn = (torch.tensor(x, dtype=torch.int64, device=dev) for x in (raw or (start, nnew)))
    assert ops.append_supported(qkv.to(dev), kd, H)
    out = ops.append_attention(qkv.to(dev), kd, vd, st, nn, H, scale=SCALE, rope=rope)
    torch.cuda.synchronize()
    out, kd, vd = out.cpu(), kd.cpu(), vd.cpu()
    assert out.shape == (B, Tn, H * D) and out.dtype == torch.bfloat16
    ok = _note(case, rm.tile_rel(hd.per_head(out, H, D), hd.per_head(exact[0], H, D), 32), floor)
    assert torch.isfinite(out).all(), case
    for b in range(B):
        s0, n = start[b], nnew[b]
        assert (_bits(out[b, n:]) == 0).all(), (case, b)  # padding rows: exact zeros
        for new, old in ((kd, kc), (vd, vc)):  # nothing but rows [start, start + nnew) was written
            assert torch.equal(_bits(new[b, :, s0 + n:]), _bits(old[b, :, s0 + n:])), (case, b)
            assert torch.equal(_bits(new[b, :, :s0]), _bits(old[b, :, :s0])), (case, b)
        v_new = qkv[b, :n, (H + Hkv) * D:].reshape(n, Hkv, D).transpose(0, 1)
        assert torch.equal(_bits(vd[b, :, s0:s0 + n]), _bits(v_new)), (case, b)
        torch.testing.assert_close(kd[b, :, s0:s0 + n].float(), emu[1][b, :, s0:s0 + n].float(), atol=2e-2, rtol=1e-2)
    assert ok, (case, "tile_rel above 3 x floor")
    return out


# ================================================================================ 1. offsets and poison
@pytest.mark.parametrize("Tn", hd.TNS)
@pytest.mark.parametrize("use_rope", [False, True], ids=["plain", "rope"])
@pytest.mark.parametrize("H,Hkv", hd.HEADS)
def test_append_attention_offsets_and_poison_at_128(dev, H, Hkv, use_rope, Tn):
    """start = an empty cache, one short of a 64-key tile edge, the middle of a tile; nnew = the
    whole block, a single token (the rest padding), a block that crosses a tile edge.  The rows
    past ``start`` hold huge finite values, then NaN: neither may reach an output."""
    rope = _rope(TMAX, dev) if use_rope else None
    qkv, kc, vc, start, nnew = hd.offsets_case(H, Hkv, Tn, use_rope, "huge")
    assert (start, nnew) == ((0, 63, 200), (Tn, 1, min(Tn, 37))) and kc.shape == (3, Hkv, 384, D)
    exact, emu, floor = _refs(qkv, kc, vc, start, nnew, H, rope)
    case = f"H{H}/{Hkv} Tn{Tn} {'rope' if use_rope else 'plain'}"
    _run_and_check(dev, case + " huge", qkv, kc, vc, start, nnew, H, rope, exact, emu, floor)
    q2, kn, vn, _, _ = hd.offsets_case(H, Hkv, Tn, use_rope, "nan")  # the same draw, NaN poison
    assert torch.equal(_bits(q2), _bits(qkv))
    assert torch.equal(_bits(kn[1, :, :63]), _bits(kc[1, :, :63])) and kn[0].isnan().all()
    _run_and_check(dev, case + " nan", qkv, kn, vn, start, nnew, H, rope, exact, emu, floor)


# ================================================================================ 2. clamps
def test_append_attention_clamps_positions_at_128(dev):
    """start / nnew outside their ranges are clamped before they address anything: the result is
    that of the clamped values (start into [0, Tmax - 1], nnew into [0, min(Tn, Tmax - start)])."""
    H, Hkv, Tn = 4, 2, 40
    raw = ((-5, 10 ** 12, TMAX - 2), (Tn + 7, 3, 50))
    start, nnew = (0, TMAX - 1, TMAX - 2), (Tn, 1, 2)
    rope = _rope(TMAX, dev)
    qkv, kc, vc = hd.append_inputs(3, H, Hkv, Tn, TMAX, start, 77, poison="huge", head_dim=D)
    exact, emu, floor = _refs(qkv, kc, vc, start, nnew, H, rope)
    _run_and_check(dev, "clamped", qkv, kc, vc, start, nnew, H, rope, exact, emu, floor, raw=raw)


# ================================================================================ 3. beside the decode kernel
def test_single_token_append_and_decode_kernel_agree_at_128(dev):
    """Tn = 1 is the decode kernel's problem: both kernels, each on a copy of the same cache, stay
    within their own bounds of the same fp64 reference (decode: test_gpu_decode.py's 2e-2)."""
    H, Hkv = 9, 3
    start, nnew = (0, 63, 200), (1, 1, 1)
    rope = _rope(TMAX, dev)
    qkv, kc, vc = hd.append_inputs(3, H, Hkv, 1, TMAX, start, 5, poison="huge", head_dim=D)
    exact, emu, floor = _refs(qkv, kc, vc, start, nnew, H, rope)
    out = _run_and_check(dev, "Tn1 vs decode", qkv, kc, vc, start, nnew, H, rope, exact, emu, floor)
    kd, vd = kc.to(dev), vc.to(dev)
    assert ops.decode.decode_supported(qkv[:, 0].to(dev), kd, H)
    dec = ops.decode_attention(qkv[:, 0].to(dev), kd, vd, torch.tensor(start, device=dev), H, scale=SCALE, rope=rope)
    err = float((dec.cpu().double() - exact[0][:, 0]).abs().max())
    print(f"  decode kernel: max abs err {err:.3e} (bound 2e-2); append vs decode "
          f"{float((dec.cpu().float() - out[:, 0].float()).abs().max()):.3e}")
    assert err < 2e-2
    for b in range(3):  # and both appended the same row
        torch.testing.assert_close(kd[b, :, start[b]].cpu().float(), emu[1][b, :, start[b]].float(), atol=2e-2, rtol=1e-2)


# ================================================================================ 4. from an empty cache
def test_append_from_empty_cache_is_causal_prefill_at_128(dev):
    """start = 0, nnew = Tn = 128: causal prefill (the flash forward has no 128 kernel to stand beside)."""
    H, Hkv, Tn = 9, 3, 128
    start, nnew = (0, 0), (Tn, Tn)
    rope = _rope(Tn, dev)
    qkv, kc, vc = hd.append_inputs(2, H, Hkv, Tn, Tn, start, 9, poison="nan", head_dim=D)
    exact, emu, floor = _refs(qkv, kc, vc, start, nnew, H, rope)
    _run_and_check(dev, "prefill append", qkv, kc, vc, start, nnew, H, rope, exact, emu, floor)


# ================================================================================ 5. graph capture
def test_graph_replay_after_start_and_nnew_moved_across_a_tile_edge(dev):
    """one captured ``ops.append_attention`` call; ``start`` / ``nnew`` then change in place from
    blocks inside the first 64-key tile to blocks that cross its edge (and one that ends on it).
    The replay is the eager call on the same inputs, bit for bit: output and caches."""
    B, H, Hkv, Tn = 3, 6, 2, 40
    rope = _rope(TMAX, dev)
    first, second = ((10, 3, 20), (5, 40, 1)), ((40, 63, 24), (40, 2, 40))
    qkv, kc, vc = hd.append_inputs(B, H, Hkv, Tn, TMAX, second[0], 21, poison="nan", head_dim=D)
    qd, kd, vd = qkv.to(dev), kc.to(dev), vc.to(dev)
    st, nn = (torch.tensor(x, dtype=torch.int64, device=dev) for x in first)
    ops.append_attention(qd, kd, vd, st, nn, H, scale=SCALE, rope=rope)  # warm-up
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.append_attention(qd, kd, vd, st, nn, H, scale=SCALE, rope=rope)
    torch.cuda.synchronize()
    kd.copy_(kc)
    vd.copy_(vc)
    st.copy_(torch.tensor(second[0], dtype=torch.int64))
    nn.copy_(torch.tensor(second[1], dtype=torch.int64))
    graph.replay()
    torch.cuda.synchronize()
    k2, v2 = kc.to(dev), vc.to(dev)
    eager = ops.append_attention(qd, k2, v2, st, nn, H, scale=SCALE, rope=rope)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    assert torch.equal(_bits(out.cpu()), _bits(eager.cpu()))
    assert torch.equal(_bits(kd.cpu()), _bits(k2.cpu())) and torch.equal(_bits(vd.cpu()), _bits(v2.cpu()))
    exact, emu, floor = _refs(qkv, kc, vc, second[0], second[1], H, rope)
    assert _note("graph replay", rm.tile_rel(hd.per_head(out.cpu(), H, D), hd.per_head(exact[0], H, D), 32), floor)


# ================================================================================ 6. the op, called directly
def test_direct_op_call_takes_128(dev):
    """``torch.ops.nbd.append_attn`` with [2, 2, 384, 128] caches returns [2, Tn, H·128]; last dim 96,
    k at 128 with v at 64, a qkv as wide as head dim 64 wants and [T, 32] RoPE tables are refused."""
    B, H, Hkv, Tn = 2, 4, 2, 5
    z = lambda *shape, dt=torch.bfloat16: torch.zeros(*shape, dtype=dt, device=dev)  # noqa: E731
    st, nn = z(B, dt=torch.int64), torch.full((B,), Tn, dtype=torch.int64, device=dev)
    k = z(B, Hkv, TMAX, D)
    q = z(B, Tn, (H + 2 * Hkv) * D)
    out = torch.ops.nbd.append_attn(q, k, k.clone(), st, nn, H, SCALE, TMAX, None, None)
    assert out.shape == (B, Tn, H * D) and out.dtype == torch.bfloat16
    cos, sin = _rope(TMAX, dev)
    assert torch.ops.nbd.append_attn(q, k, k.clone(), st, nn, H, SCALE, TMAX, cos, sin).shape == (B, Tn, H * D)
    k96, q96 = z(B, Hkv, TMAX, 96), z(B, Tn, (H + 2 * Hkv) * 96)
    with pytest.raises(RuntimeError, match="head dim must be 64 or 128, got 96"):
        torch.ops.nbd.append_attn(q96, k96, k96.clone(), st, nn, H, 96 ** -0.5, TMAX, None, None)
    assert not ops.append_supported(q96, k96, H)
    assert ops.append_attention(q96, k96, k96.clone(), st, nn, H).shape == (B, Tn, H * 96)  # the PyTorch path
    k64, q64 = z(B, Hkv, TMAX, 64), z(B, Tn, (H + 2 * Hkv) * 64)
    with pytest.raises(RuntimeError, match=r"must have the same shape \(head dim 128\)"):
        torch.ops.nbd.append_attn(q, k, k64, st, nn, H, SCALE, TMAX, None, None)
    with pytest.raises(RuntimeError, match=r"qkv width 512 != \(H \+ 2·Hkv\)·128 = 1024 at head dim 128"):
        torch.ops.nbd.append_attn(q64, k, k.clone(), st, nn, H, SCALE, TMAX, None, None)
    c32, s32 = ops.rope_tables(TMAX, 64, 10000.0, dev)
    assert c32.shape == (TMAX, 32)
    with pytest.raises(RuntimeError, match=r"rope tables must be contiguous float32 \[>= Tmax, 64\].*head dim 128"):
        torch.ops.nbd.append_attn(q, k, k.clone(), st, nn, H, SCALE, TMAX, c32, s32)
    assert torch.ops.nbd.append_attn(q64, k64, k64.clone(), st, nn, H, 0.125, TMAX, c32, s32).shape == (B, Tn, H * 64)
    torch.cuda.synchronize()


# ================================================================================ 7. model level
LENS1, NEW1 = (40, 33, 12, 1), 24
LENS2, NEW2 = (7, 1, 32, 20), 16
T_MAX = 160  # the first call prefills at 128 rows; 63 held + 1 + 32 + 16 after the second


def _model(dev):
    from nbdistributed_amd.models.llama import LlamaConfig, LlamaForCausalLM

    torch.manual_seed(0)
    m = LlamaForCausalLM(LlamaConfig.tiny(explicit_head_dim=D)).to(dev, torch.bfloat16).eval()
    with torch.no_grad():
        m.model.embed_tokens.weight.mul_(8.0)  # test_gpu_decode.py's _peaked gain
    return m


def test_model_two_turns_at_128(dev):
    """``generate(turn, n, cache=cache)`` on a head-dim-128 Llama: the turn runs the kernel, and gives
    what one ``generate`` over the concatenated history gives, graph on or off; the turn's first
    logits lie within 5 % of the largest |logit| of the full forward (test_gpu_generate_continue.py's
    bound).  Printed: the same logits against the call with ``append_supported`` patched to False."""
    m = _model(dev)
    assert m.kv_layout()[1:] == (4, 2, D)
    B = len(LENS1)
    g = torch.Generator(device="cuda").manual_seed(1)
    ids1 = torch.randint(1, 512, (B, max(LENS1)), device=dev, generator=g)
    ids2 = torch.randint(1, 512, (B, max(LENS2)), device=dev, generator=g)
    l1, l2 = torch.tensor(LENS1, device=dev), torch.tensor(LENS2, device=dev)
    outs = {}
    for graph in (False, True):
        out1, cache = generate(m, ids1, NEW1, lengths=l1, t_max=T_MAX, graph=graph, return_cache=True)
        if not graph:  # the block's logits, on copies of the cache state the turn starts from
            assert isinstance(cache, KVCache) and cache.k.shape[-1] == D
            assert ops.append_supported(torch.zeros(B, 8, 8 * D, dtype=torch.bfloat16, device=dev), cache.k[0], 4)
            chunk = torch.cat([cache.pending.view(B, 1), ids2], 1)
            first = {}
            for patched in (False, True):
                c2 = copy.copy(cache)
                c2.k, c2.v = cache.k.clone(), cache.v.clone()
                ctx = mock.patch.object(ops.decode, "append_supported", lambda *a: False) if patched else \
                    contextlib.nullcontext()
                with ctx:
                    first[patched] = m.extend(chunk, c2, cache.lengths.clone(), l2 + 1).float()
            torch.cuda.synchronize()
            assert torch.isfinite(first[False]).all() and torch.isfinite(first[True]).all()
            print(f"  max |logit(kernel) - logit(PyTorch path)| = {(first[False] - first[True]).abs().max().item():.4e} "
                  f"(max |logit| {first[True].abs().max().item():.3f})")
        out2 = generate(m, ids2, NEW2, lengths=l2, cache=cache, graph=graph)
        outs[graph] = (out1, out2)
    assert torch.equal(outs[False][0], outs[True][0]) and torch.equal(outs[False][1], outs[True][1])
    out1, out2 = outs[True]
    assert out2.shape == (B, max(LENS2) + NEW2)
    hist = [out1[b, :LENS1[b] + NEW1].tolist() + ids2[b, :LENS2[b]].tolist() for b in range(B)]
    hl = torch.tensor([len(h) for h in hist], device=dev)
    whole = torch.zeros(B, int(hl.max()), dtype=torch.long, device=dev)
    for b, h in enumerate(hist):
        whole[b, :len(h)] = torch.tensor(h, device=dev)
    ref = generate(m, whole, NEW2, lengths=hl, graph=True)  # the existing path: prefill of the whole history
    for b in range(B):
        n = LENS2[b]
        assert out2[b, :n].tolist() == ids2[b, :n].tolist()
        assert out2[b, n:n + NEW2].tolist() == ref[b, len(hist[b]):len(hist[b]) + NEW2].tolist(), b
        assert (out2[b, n + NEW2:] == 0).all()
        with torch.no_grad():
            full = m(torch.tensor([hist[b]], device=dev))[1][0, -1].float()
        d = (first[False][b] - full).abs().max().item()
        print(f"  row {b}: first-logit max|Δ| {d:.4f} of max|full| {full.abs().max().item():.3f}")
        assert d < 0.05 * full.abs().max().item()
