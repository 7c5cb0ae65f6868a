"""CPU: ``ops.append_attention_shared_reference`` — the block append behind a shared prefix — is
``ops.append_attention_reference`` on the materialised cache (each sequence's prompt rows copied in
front of its own rows), to fp32 accuracy, on inputs whose unwritten prefix and own rows hold NaN.
``shared_inputs`` / ``materialise`` also serve tests/test_gpu_append_shared.py."""
import itertools
import math

import pytest
import torch

from nbdistributed_amd import ops
from nbdistributed_amd.ops.decode import _to_cache

H, HKV, TP = 4, 2, 131  # 131 prefix rows: every plen below leaves NaN rows behind it
F8 = torch.float8_e4m3fn
PLENS = ((64, 128), (70, 5), (130, 64))  # tile-aligned; a straddle in tile 1 and own rows inside tile 0; in tile 2
OWN = (1, 40, 17, 33, 8, 25)  # own rows already held, per sequence
# (D, fp8, group, plen pair, Tn, RoPE)
CASES = list(itertools.product((64, 128), (False, True), (1, 3), PLENS, (5, 130), (False, True)))


def shared_inputs(D, f8, group, plens, Tn):
    """(qkv, k_prefix, v_prefix, plen, k_own, v_own, start, nnew): two prompts, ``group`` samples of
    each; rows the sequences do not hold (prefix >= plen, own >= held) are NaN."""
    g = torch.Generator().manual_seed(1000 * D + 100 * group + Tn + plens[0])
    S, To = 2 * group, max(OWN) + Tn + 3
    dt = F8 if f8 else torch.bfloat16
    draw = lambda *shape, gain=1.0: gain * torch.randn(*shape, generator=g)  # noqa: E731
    qkv = torch.cat([draw(S, Tn, (H + HKV) * D, gain=2.0), draw(S, Tn, HKV * D)], -1).bfloat16()
    pre = [draw(2, HKV, TP, D, gain=2.0), draw(2, HKV, TP, D)]
    own = [draw(S, HKV, To, D, gain=2.0), draw(S, HKV, To, D)]
    plen, held = torch.tensor(plens), torch.tensor(OWN[:S])
    for x in pre:
        x.masked_fill_((torch.arange(TP)[None, :] >= plen[:, None])[:, None, :, None], math.nan)
    for x in own:
        x.masked_fill_((torch.arange(To)[None, :] >= held[:, None])[:, None, :, None], math.nan)
    nnew = torch.tensor((Tn, 1, max(1, Tn // 2), Tn, min(Tn, 37), 1)[:S])
    start = plen.repeat_interleave(group) + held
    return (qkv, _to_cache(pre[0], dt), _to_cache(pre[1], dt), plen, _to_cache(own[0], dt), _to_cache(own[1], dt),
            start, nnew)


def materialise(pre, own, plen, group):
    """[S, Hkv, Tp + To, D]: rows [0, plen) of the sequence's prompt, its own rows behind them, NaN after."""
    S, To = own.shape[0], own.shape[2]
    full = torch.full((S, own.shape[1], pre.shape[2] + To, own.shape[3]), math.nan).to(own.dtype)
    for s in range(S):
        pl = int(plen[s // group])
        full[s, :, :pl] = pre[s // group, :, :pl]
        full[s, :, pl:pl + To] = own[s]
    return full


def bits(t):
    return t.contiguous().view(torch.uint8)


@pytest.mark.parametrize("D,f8,group,plens,Tn,use_rope", CASES)
def test_shared_reference_is_the_reference_on_the_materialised_cache(D, f8, group, plens, Tn, use_rope):
    qkv, kp, vp, plen, ko, vo, start, nnew = shared_inputs(D, f8, group, plens, Tn)
    rope = ops.rope_tables(TP + ko.shape[2], D, 10000.0, "cpu") if use_rope else None
    kf, vf = materialise(kp, ko, plen, group), materialise(vp, vo, plen, group)
    kp0, vp0, ko0 = kp.clone(), vp.clone(), ko.clone()
    out = ops.append_attention_shared_reference(qkv.float(), kp, vp, plen, ko, vo, start, nnew, group, H, rope=rope)
    want = ops.append_attention_reference(qkv.float(), kf, vf, start, nnew, H, rope=rope)
    assert torch.isfinite(out).all()
    torch.testing.assert_close(out, want, atol=1e-5, rtol=1e-5)
    assert torch.equal(bits(kp), bits(kp0)) and torch.equal(bits(vp), bits(vp0))  # the prefix is read only
    for s in range(2 * group):
        pl, s0, n = int(plen[s // group]), int(start[s]), int(nnew[s])
        for o, f in ((ko, kf), (vo, vf)):  # the block's rows, as the unshared reference stores them
            assert torch.equal(bits(o[s, :, s0 - pl:s0 - pl + n]), bits(f[s, :, s0:s0 + n]))
        assert torch.equal(bits(ko[s, :, s0 - pl + n:]), bits(ko0[s, :, s0 - pl + n:]))
        assert torch.equal(bits(ko[s, :, :s0 - pl]), bits(ko0[s, :, :s0 - pl]))


def test_mixed_cache_dtypes_are_refused():
    qkv, kp, vp, plen, ko, vo, start, nnew = shared_inputs(64, False, 1, PLENS[1], 5)
    with pytest.raises(ValueError, match="same dtype"):
        ops.append_attention_shared(qkv, kp.to(F8), vp.to(F8), plen, ko, vo, start, nnew, 1, H)
    with pytest.raises(ValueError, match="same dtype"):
        ops.append_attention_shared(qkv, kp, vp, plen, ko, vo.to(F8), start, nnew, 1, H)
