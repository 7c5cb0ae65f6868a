"""GPU: the block append behind a shared prefix — csrc/kernels/append.hip ``append_kv_kernel<D, F8,
true>`` / ``append_attn_kernel<D, SPLIT, F8, true>``, op ``append_attn_shared`` — on the inputs of
tests/test_append_shared_ref.py (unwritten prefix and own rows hold NaN), against

(a) ``ops.append_attention`` on the materialised cache: output and written rows equal as bits;
(b) ``ops.append_attention_shared_reference`` in fp64 under tests/test_gpu_append_attn.py's rule,
    unchanged: ``floor = tile_rel(emulated reference, fp64 reference)`` and ``tile_rel(kernel, fp64
    reference) <= 3 x floor`` per 32-row tile.  The emulation (``refmath_append_hd._attend``) runs
    over the cache rows as the kernel left them, as tests/test_gpu_append_kv8.py does.
``-s`` prints every kernel/floor ratio."""
import pytest
import torch

import refmath as rm
import refmath_append_hd as hd
from nbdistributed_amd import ops
from test_append_shared_ref import CASES, H, HKV, TP, bits, materialise, shared_inputs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(require_gpu):
    assert ops.native_available(), ops._load_error
    return torch.device("cuda", 0)


def _emulated(qkv, kf, vf, start, nnew, D, rope):
    """the kernel's rounding points over the materialised caches as the kernel left them"""
    out = torch.zeros(qkv.shape[0], qkv.shape[1], H * D, dtype=torch.float64)
    hm = torch.arange(H) // (H // HKV)
    for s, (s0, n) in enumerate(zip(start.tolist(), nnew.tolist())):
        q = qkv[s, :n, :H * D].double().reshape(n, H, D).transpose(0, 1)
        if rope is not None:
            q = rm._rd(hd.dh.rot(q, rope[0].double(), rope[1].double(), s0 + torch.arange(n)), torch.bfloat16)
        vis = torch.arange(s0 + n)[None, :] <= s0 + torch.arange(n)[:, None]
        o = hd._attend(q, kf[s, hm, :s0 + n].double(), vf[s, hm, :s0 + n].double(), vis, hd.scale_of(D), True)
        out[s, :n] = o.transpose(0, 1).reshape(n, H * D)
    return out


@pytest.mark.parametrize("D,f8,group,plens,Tn,use_rope", CASES)
def test_shared_append_is_the_unshared_kernel_on_the_materialised_cache(dev, D, f8, group, plens, Tn, use_rope):
    """unsplit, then forced to two key chunks (``key_splits=2``, as tests/test_gpu_append_split.py forces it)"""
    qkv, kp, vp, plen, ko, vo, start, nnew = shared_inputs(D, f8, group, plens, Tn)
    rope = ops.rope_tables(TP + ko.shape[2], D, 10000.0, dev) if use_rope else None
    rope_cpu = None if rope is None else (rope[0].cpu(), rope[1].cpu())
    wide = (lambda x: x.clone()) if f8 else (lambda x: x.double())
    exact = ops.append_attention_shared_reference(qkv.double(), wide(kp), wide(vp), plen, wide(ko), wide(vo), start,
                                                  nnew, group, H, scale=hd.scale_of(D), rope=rope_cpu)
    exact = hd.per_head(exact, H, D)
    st, nn = start.to(dev), nnew.to(dev)
    for key_splits in (1, 2):
        kw = dict(scale=hd.scale_of(D), rope=rope, key_splits=key_splits)
        kpd, vpd, kod, vod = (x.to(dev) for x in (kp, vp, ko, vo))
        out = ops.append_attention_shared(qkv.to(dev), kpd, vpd, plen.to(dev), kod, vod, st, nn, group, H, **kw)
        kfd, vfd = materialise(kp, ko, plen, group).to(dev), materialise(vp, vo, plen, group).to(dev)
        want = ops.append_attention(qkv.to(dev), kfd, vfd, st, nn, H, **kw)
        torch.cuda.synchronize()
        out, want, kod, vod, kfd, vfd = (x.cpu() for x in (out, want, kod, vod, kfd, vfd))
        # (a) bit for bit the unshared kernel; the prefix read only; own rows outside the block untouched
        assert torch.isfinite(out).all() and torch.equal(bits(out), bits(want)), key_splits
        assert torch.equal(bits(kpd.cpu()), bits(kp)) and torch.equal(bits(vpd.cpu()), bits(vp))
        for s in range(2 * group):
            pl, s0, n = int(plen[s // group]), int(start[s]), int(nnew[s])
            for new, old, full in ((kod, ko, kfd), (vod, vo, vfd)):
                assert torch.equal(bits(new[s, :, s0 - pl:s0 - pl + n]), bits(full[s, :, s0:s0 + n])), s
                assert torch.equal(bits(new[s, :, :s0 - pl]), bits(old[s, :, :s0 - pl])), s
                assert torch.equal(bits(new[s, :, s0 - pl + n:]), bits(old[s, :, s0 - pl + n:])), s
        # (b) the fp64 reference, under the bound of the unshared kernel's tests
        emu = _emulated(qkv, kfd.float(), vfd.float(), start, nnew, D, rope_cpu)
        floor = rm.tile_rel(hd.per_head(emu, H, D), exact, 32)
        err = rm.tile_rel(hd.per_head(out, H, D), exact, 32)
        print(f"  splits {key_splits}: kernel {err:.3e} floor {floor:.3e} ratio {err / floor if floor else 0.0:.2f}")
        assert err <= 3 * floor, key_splits


@pytest.mark.parametrize("D", [64, 128])
def test_graph_replays_equal_the_eager_call(dev, D):
    """one captured call (two chunks, a straddling tile), then ``start`` / ``nnew`` / ``plen`` move in
    place; three replays, each the eager call on the same inputs: output and own rows, bit for bit"""
    group, Tn = 3, 130
    qkv, kp, vp, plen, ko, vo, start, nnew = shared_inputs(D, False, group, (70, 5), Tn)
    rope = ops.rope_tables(TP + ko.shape[2], D, 10000.0, dev)
    qd, kpd, vpd, pld = qkv.to(dev), kp.to(dev), vp.to(dev), torch.tensor((64, 4), device=dev)
    st, nn = (start + plen.new_tensor((64 - 70, 4 - 5)).repeat_interleave(group)).to(dev), torch.ones_like(nnew).to(dev)
    call = lambda k, v: ops.append_attention_shared(qd, kpd, vpd, pld, k, v, st, nn, group, H,  # noqa: E731
                                                    scale=hd.scale_of(D), rope=rope, key_splits=2)
    kd, vd = ko.to(dev), vo.to(dev)
    call(kd, vd)  # warm-up
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call(kd, vd)
    pld.copy_(plen)
    st.copy_(start)
    nn.copy_(nnew)
    k2, v2 = ko.to(dev), vo.to(dev)
    eager = call(k2, v2)
    for _ in range(3):
        kd.copy_(ko)
        vd.copy_(vo)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.isfinite(out).all() and torch.equal(bits(out.cpu()), bits(eager.cpu()))
        assert torch.equal(bits(kd.cpu()), bits(k2.cpu())) and torch.equal(bits(vd.cpu()), bits(v2.cpu()))
