"""GPU: fp8 (``float8_e4m3fn``, no scales) KV caches in the block-append kernels — csrc/kernels/append.hip
``append_kv_kernel<D, true>`` and ``append_attn_kernel<D, SPLIT, true>`` — on the offsets of
tests/test_gpu_append_hd.py, the caches ``q8`` of the draws, rows >= start holding ±448 then NaN bytes.
Stored rows are bit patterns; the output is the bf16 kernel's, bit for bit, on the dequantised cache;
against fp64 over the cache as stored it obeys ``tile_rel(kernel, exact) <= 3 x tile_rel(emulated,
exact)`` per 32-row tile.  ``-s`` prints every ratio and the worst (docs/FINDINGS.md §49 keeps it)."""
import contextlib
import copy
import functools
import math
from unittest import mock

import pytest
import torch

import refmath as rm
import refmath_append_hd as hd
import refmath_kv8 as r8
from nbdistributed_amd import ops
from nbdistributed_amd.generation import generate

pytestmark = pytest.mark.gpu

WORST = [0.0, ""]
# (D, H, Hkv, Tn, RoPE, key_splits); nnew = (Tn, 1, min(Tn, 37)) at starts (0, 63, 200), Tmax 384
ALL = [(D, H, Hkv, Tn, r, s) for D in (64, 128) for H, Hkv in ((9, 3), (8, 1)) for Tn in (1, 33, 130)
       for r in (False, True) for s in (1, 3)]


@pytest.fixture(scope="module")
def dev(require_gpu):
    assert ops.native_available(), ops._load_error
    yield torch.device("cuda", 0)
    print(f"\nworst fp8 append kernel/floor ratio (bound 3): {WORST[0]:.2f}  {WORST[1]}")


def _note(case, err, floor):
    ratio = err / floor if floor > 0 else (0.0 if err == 0 else math.inf)
    print(f"  {case}: kernel {err:.3e} floor {floor:.3e} ratio {ratio:.2f}")
    if ratio > WORST[0]:
        WORST[0], WORST[1] = ratio, case
    return err <= 3 * floor


def _bits(t):
    return t.contiguous().view(torch.int16)


@functools.lru_cache(maxsize=None)
def _run(D, H, Hkv, Tn, use_rope, splits, poison="max", saturate=False):
    """one op call on device copies of the case's inputs, shared by the tests: (qkv, k8, v8, nnew,
    rope, out, k8 after, v8 after), all but the RoPE tables on the CPU.  ``saturate``: sequence 2's
    k | v columns scaled past ±448, ±inf in its v."""
    dev = torch.device("cuda", 0)
    nnew = (Tn, 1, min(Tn, 37))
    qkv, kc, vc = hd.append_inputs(3, H, Hkv, Tn, hd.TMAX, hd.START, 1000 * H + 10 * Tn + use_rope, head_dim=D)
    if saturate:
        qkv[2, :, H * D:] *= 256.0
        qkv[2, :, (H + Hkv) * D::7] = math.inf
        qkv[2, :, (H + Hkv) * D + 3::7] = -math.inf
    sign = torch.stack([kc.float().sign(), vc.float().sign()])  # (the loud poison carries the draw's signs)
    _, k8, v8 = r8.kv8_poison((qkv, kc, vc, sign), hd.START, poison)
    rope = ops.rope_tables(hd.TMAX, D, 10000.0, dev) if use_rope else None
    kd, vd = k8.to(dev), v8.to(dev)
    st, nn = (torch.tensor(x, dtype=torch.int64, device=dev) for x in (hd.START, nnew))
    assert ops.append_supported(qkv.to(dev), kd, H, vd)  # (not so before the fp8 kernels)
    out = ops.append_attention(qkv.to(dev), kd, vd, st, nn, H, scale=hd.scale_of(D), rope=rope, key_splits=splits)
    torch.cuda.synchronize()
    assert out.shape == (3, Tn, H * D) and out.dtype == torch.bfloat16 and kd.dtype == r8.F8
    return qkv, k8, v8, nnew, rope, out.cpu(), kd.cpu(), vd.cpu()


def _ord8(b):
    """e4m3 codes on a line: adjacent codes differ by 1, +0 and -0 coincide"""
    u = r8.canon8(b).to(torch.int16)
    return torch.where(u >= 128, 128 - u, u)


def _check_stored(c, poison, saturate=False):
    D, H, Hkv, Tn, use_rope, _ = c
    qkv, k8, v8, nnew, rope, out, kd, vd = _run(*c, poison, saturate)
    x = qkv.double().reshape(3, Tn, H + 2 * Hkv, D).transpose(1, 2)  # [B, heads, Tn, D]
    k, v = x[:, H:H + Hkv], x[:, H + Hkv:]
    if use_rope:  # rotated in fp64, then rounded once: the bf16 row up to one bf16 ulp
        pos = torch.tensor(hd.START)[:, None, None] + torch.arange(Tn)
        k = hd.dh.rot(k, rope[0].double().cpu(), rope[1].double().cpu(), pos)
    assert torch.isfinite(out).all()
    for b, (s0, n) in enumerate(zip(hd.START, nnew)):
        assert (_bits(out[b, n:]) == 0).all()  # padding rows: exact zeros
        assert torch.equal(r8.canon8(vd[b, :, s0:s0 + n]), r8.canon8(r8.q8(v[b, :, :n])))
        step = (_ord8(kd[b, :, s0:s0 + n]) - _ord8(r8.q8(k[b, :, :n]))).abs().max()
        assert step <= (1 if use_rope else 0), (b, int(step))
        for new, old in ((kd, k8), (vd, v8)):  # every byte outside [start, start + nnew) is unchanged
            assert torch.equal(r8.bits8(new[b, :, :s0]), r8.bits8(old[b, :, :s0]))
            assert torch.equal(r8.bits8(new[b, :, s0 + n:]), r8.bits8(old[b, :, s0 + n:]))


@pytest.mark.parametrize("c", ALL, ids=str)
def test_stored_rows_are_q8_of_the_bf16_rows(dev, c):
    """v rows and, without RoPE, k rows: the bytes of ``q8``; with RoPE the code of the fp64-rotated
    row or an adjacent one (one bf16 ulp of the rotation can cross one e4m3 boundary, no further)."""
    for poison in r8.KV8_POISON:
        _check_stored(c, poison)


@pytest.mark.parametrize("use_rope", [False, True])
def test_stored_rows_saturate_at_448(dev, use_rope):
    """|k|, |v| up to ~2000 and ±inf in v arrive: the stored bytes are the clamped codes, never NaN"""
    _check_stored((64, 9, 3, 33, use_rope, 1), "nan", saturate=True)
    kd, vd = _run(64, 9, 3, 33, use_rope, 1, "nan", True)[6:]
    assert (r8.canon8(vd[2, :, 200:233]) != r8.NAN_BYTE).all() and (r8.bits8(vd[2, :, 200:233]) & 0x7F == 0x7E).any()


@pytest.mark.parametrize("c", [c for c in ALL if not c[4]], ids=str)
def test_output_is_the_bf16_kernels_on_the_dequantised_cache(dev, c):
    """On bf16 caches holding the dequantised rows the op left, with a qkv whose k | v columns are
    those rows (the bf16 kernel stores again what is there), the outputs are equal as bits, split
    and unsplit.  RoPE off only: no qkv makes the bf16 kernel store the dequantised e4m3 rows under
    a rotation; the RoPE code is shared by both variants and the fp64 test below covers it."""
    D, H, Hkv, Tn, _, splits = c
    for poison in r8.KV8_POISON:
        qkv, _, _, nnew, _, out, kd, vd = _run(*c, poison)
        kb, vb, q2 = kd.bfloat16(), vd.bfloat16(), qkv.clone()
        for b, (s0, n) in enumerate(zip(hd.START, nnew)):
            q2[b, :n, H * D:(H + Hkv) * D] = kb[b, :, s0:s0 + n].transpose(0, 1).reshape(n, Hkv * D)
            q2[b, :n, (H + Hkv) * D:] = vb[b, :, s0:s0 + n].transpose(0, 1).reshape(n, Hkv * D)
        k2, v2 = kb.to(dev), vb.to(dev)
        st, nn = (torch.tensor(x, dtype=torch.int64, device=dev) for x in (hd.START, nnew))
        ref = ops.append_attention(q2.to(dev), k2, v2, st, nn, H, scale=hd.scale_of(D), key_splits=splits)
        assert torch.equal(_bits(k2.cpu()), _bits(kb)) and torch.equal(_bits(v2.cpu()), _bits(vb))
        assert torch.equal(_bits(out), _bits(ref.cpu())), (c, poison)


def _ref64(qkv, kd, vd, nnew, H, D, rope, emulate):
    """fp64 over the caches as the op left them: query i, rotated in fp64 at start + i, attends the
    dequantised rows 0 .. start + i.  ``emulate``: the kernel's rounding points (hd._attend)."""
    kc, vc = r8.dq8(kd), r8.dq8(vd)
    Hkv, Tn = kc.shape[1], qkv.shape[1]
    out = torch.zeros(3, Tn, H * D, dtype=torch.float64)
    for b, (s0, n) in enumerate(zip(hd.START, nnew)):
        q = qkv[b, :n, :H * D].double().reshape(n, H, D).transpose(0, 1)
        if rope is not None:
            q = hd.dh.rot(q, rope[0].double().cpu(), rope[1].double().cpu(), s0 + torch.arange(n))
            q = rm._rd(q, torch.bfloat16) if emulate else q
        hm = torch.arange(H) // (H // Hkv)
        vis = torch.arange(s0 + n)[None, :] <= s0 + torch.arange(n)[:, None]
        o = hd._attend(q, kc[b, hm, :s0 + n], vc[b, hm, :s0 + n], vis, hd.scale_of(D), emulate)
        out[b, :n] = o.transpose(0, 1).reshape(n, H * D)
    return out


def _tile_check(case, out, kd, vd, qkv, nnew, H, D, rope):
    exact = hd.per_head(_ref64(qkv, kd, vd, nnew, H, D, rope, False), H, D)
    floor = rm.tile_rel(hd.per_head(_ref64(qkv, kd, vd, nnew, H, D, rope, True), H, D), exact, 32)
    return exact, floor, _note(case, rm.tile_rel(hd.per_head(out, H, D), exact, 32), floor)


@pytest.mark.parametrize("c", ALL, ids=str)
def test_output_against_fp64_over_the_cache_as_stored(dev, c):
    D, H = c[0], c[1]
    qkv, _, _, nnew, rope, out, kd, vd = _run(*c, "max")
    exact, floor, ok = _tile_check(f"{c} max", out, kd, vd, qkv, nnew, H, D, rope)
    out_n, kn, vn = _run(*c, "nan")[5:]  # the same draw, NaN bytes in the free rows: the same valid rows
    for b, (s0, n) in enumerate(zip(hd.START, nnew)):
        assert torch.equal(r8.bits8(kn[b, :, :s0 + n]), r8.bits8(kd[b, :, :s0 + n]))
    assert torch.isfinite(out).all() and torch.isfinite(out_n).all()
    assert _note(f"{c} nan", rm.tile_rel(hd.per_head(out_n, H, D), exact, 32), floor) and ok


@pytest.mark.parametrize("D", (64, 128))
def test_single_token_beside_the_decode_kernel(dev, D):
    """Tn = 1 is the decode kernel's problem: on copies of one fp8 cache both store the same bytes,
    and each output keeps its own bound of the fp64 reference (decode: 2e-2, test_gpu_kv8.py's)."""
    c = (D, 9, 3, 1, True, 1)
    qkv, k8, v8, nnew, rope, out, kd, vd = _run(*c)
    k2, v2 = k8.to(dev), v8.to(dev)
    dec = ops.decode_attention(qkv[:, 0].to(dev), k2, v2, torch.tensor(hd.START, device=dev), 9,
                               scale=hd.scale_of(D), rope=rope).cpu()
    for b, s0 in enumerate(hd.START):
        assert torch.equal(r8.canon8(k2.cpu()[b, :, s0]), r8.canon8(kd[b, :, s0]))
        assert torch.equal(r8.canon8(v2.cpu()[b, :, s0]), r8.canon8(vd[b, :, s0]))
    exact, _, ok = _tile_check(f"{c} beside decode", out, kd, vd, qkv, nnew, 9, D, rope)
    err = float((dec.double() - exact.transpose(1, 2).reshape(3, 1, -1)[:, 0]).abs().max())
    print(f"  decode kernel: max abs err {err:.3e} (bound 2e-2)")
    assert err < 2e-2 and ok


LENS1, NEW1, LENS2, NEW2, T_MAX = (40, 33, 12, 1), 24, (7, 1, 32, 20), 16, 160  # test_gpu_generate_continue.py's


@pytest.mark.parametrize("D", (64, 128))
def test_generate_continues_from_an_fp8_cache(dev, D):
    """turn 1 with ``kv_dtype="fp8"``, turn 2 from its cache (ragged, eager and graphed): the extend
    step's logits and the turn's tokens against the same calls with ``append_supported`` patched to
    False (the PyTorch path on the same fp8 cache), within test_gpu_generate_continue.py's 5 % of
    the largest |logit|."""
    from nbdistributed_amd.models.llama import LlamaConfig, LlamaForCausalLM

    torch.manual_seed(0)
    m = LlamaForCausalLM(LlamaConfig.tiny(explicit_head_dim=D)).to(dev, torch.bfloat16).eval()
    with torch.no_grad():
        m.model.embed_tokens.weight.mul_(8.0)  # test_gpu_decode.py's _peaked gain
    assert m.kv_layout()[3] == D
    B = len(LENS1)
    g = torch.Generator(device="cuda").manual_seed(1)
    ids1, ids2 = (torch.randint(1, 512, (B, max(ln)), device=dev, generator=g) for ln in (LENS1, LENS2))
    l1, l2 = torch.tensor(LENS1, device=dev), torch.tensor(LENS2, device=dev)
    first, outs = {}, {}
    for graph in (False, True):
        for patched in (False, True):
            _, cache = generate(m, ids1, NEW1, lengths=l1, t_max=T_MAX, graph=graph, kv_dtype="fp8", return_cache=True)
            assert cache.is_fp8
            held = cache.lengths.clone()
            with (mock.patch.object(ops.decode, "append_supported", lambda *a: False) if patched
                  else contextlib.nullcontext()):
                if not graph:  # the block's logits, on a copy of the cache state the turn starts from
                    c2 = copy.copy(cache)
                    c2.k, c2.v = cache.k.clone(), cache.v.clone()
                    chunk = torch.cat([cache.pending.view(B, 1), ids2], 1)
                    first[patched] = m.extend(chunk, c2, held.clone(), l2 + 1).float()
                out2 = generate(m, ids2, NEW2, lengths=l2, cache=cache, graph=graph, kv_dtype="fp8" if graph else None)
            outs[graph, patched] = out2
            assert cache.is_fp8 and torch.equal(cache.lengths, held + l2 + NEW2)  # as on a bf16 cache
            assert torch.equal(cache.pending, out2[torch.arange(B), l2 + NEW2 - 1])
    d, top = (first[False] - first[True]).abs().max().item(), first[True].abs().max().item()
    print(f"  D {D}: max |logit(kernel) - logit(PyTorch path)| = {d:.4e} of max |logit| {top:.3f}")
    assert torch.isfinite(first[False]).all() and d < 0.05 * top
    assert all(torch.equal(outs[False, False], o) for o in outs.values())
    _, c16 = generate(m, ids1, NEW1, lengths=l1, t_max=T_MAX, return_cache=True)
    with pytest.raises(ValueError, match="kv_dtype"):
        generate(m, ids2, NEW2, lengths=l2, cache=c16, kv_dtype="fp8")
