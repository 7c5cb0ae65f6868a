"""GPU numerics of the streaming small-M linear (csrc/kernels/smallm_stream.hip), reached through
``torch.ops.nbd.linear_small(..., stream)`` so that the routing of ``ops.linear_small`` cannot divert
a case: ``stream = 0`` past smallm.hip's K (the plan's K-slices), ``stream = n`` = n slices at any K.

References, inputs and the bound are those of tests/test_gpu_decode_paths.py: ``floor =
tile_rel(emulated reference, fp64 reference)`` per 16 x 16 output tile of ``refmath_decode``'s
structured inputs, and the kernel must be finite and score <= 3 x floor.

The ring is R = 3 chunks of C = 4 k-steps (2 with SwiGLU); at one slice a wave owns K / 256 steps."""
import functools
import math

import pytest
import torch

import refmath as rm
import refmath_decode as rd

pytestmark = pytest.mark.gpu

_NORM = {None: 0, "ln": 1, "rms": 2}
_ACT = {"none": 0, "gelu": 1, "swiglu": 2}
PLAIN, LN, RMS_SW, SW = (None, "none", True, True), ("ln", "none", True, False), rd.LINEAR_COMBOS[4], (None, "swiglu", False, False)

CASES = [  # (M, K, N, combo, stream)
    # past the old limits, at the plan's slices: refused before this kernel
    (9, 4128, 272, PLAIN, 0), (8, 2080, 272, RMS_SW, 0),
    # the ring at one slice: a wave owns less than a chunk, exactly one ring, a ring + a chunk + a ragged tail
    (17, 768, 48, PLAIN, 1), (17, 3072, 48, LN, 1), (17, 4128, 272, PLAIN, 1),
    (8, 256, 48, RMS_SW, 1), (8, 1536, 272, RMS_SW, 1), (9, 2080, 272, RMS_SW, 1),
    # slices: 280 steps divide evenly neither by 8 waves nor by 3 slices; the plan (8 slices)
    (1, 8960, 272, PLAIN, 1), (1, 8960, 272, PLAIN, 2), (1, 8960, 272, PLAIN, 3), (1, 8960, 272, PLAIN, 0),
    # norms whose statistics span 3 slices
    (8, 8192, 8, RMS_SW, 3), (8, 8192, 272, ("ln", "gelu", True, False), 3), (9, 14336, 8, ("rms", "none", False, True), 3),
    # >= 128 column tiles, 4 m-tiles, the plan (4 slices)
    (64, 4128, 2064, PLAIN, 0),
    # x fragments from global memory (the image of 64 rows x 8192 does not fit) and staged next to it
    (64, 8192, 48, PLAIN, 1), (64, 8192, 48, PLAIN, 8), (64, 8192, 8, SW, 1), (64, 14336, 8, SW, 0),
] + [(17, 4128, 272, c, 2) for c in rd.LINEAR_COMBOS]  # every epilogue (SwiGLU: K = 2080)


@pytest.fixture(scope="module")
def dev(require_gpu):
    from nbdistributed_amd import ops

    assert ops.native_available(), ops._load_error
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _case(M, K, N, combo):
    """(inputs, fp64 reference tiles, floor): computed once per shape, shared by its slice counts."""
    norm, act, bias, res = combo
    inputs = rd.linear_small_inputs(M, K, N, norm, act, bias, res, seed=7 * M + K + 3 * N)
    exact = rd.tiles16(rd.linear_small_ref(*inputs[:3], inputs[3], act, inputs[4]))
    floor = rm.tile_rel(rd.tiles16(rd.linear_small_ref(*inputs[:3], inputs[3], act, inputs[4], emulate=True)), exact, 16)
    return inputs, exact, floor


def _args(dev, inputs, act, xdev=None):
    x, w, b, nrm, rs = inputs
    to = lambda t: None if t is None else t.to(dev)  # noqa: E731
    nw = to(nrm[1]) if nrm else None
    nb = to(nrm[2]) if nrm and nrm[0] == "ln" else None
    return (to(x) if xdev is None else xdev, to(w), to(b), nw, nb, float(nrm[-1]) if nrm else 0.0,
            _NORM[nrm[0] if nrm else None], _ACT[act], to(rs))


def _op(args, stream):
    # stream = 0 goes as the nine positional arguments every caller passed before the argument existed
    return torch.ops.nbd.linear_small(*args) if stream == 0 else torch.ops.nbd.linear_small(*args, stream)


def _check(dev, M, K, N, combo, stream, xdev=None):
    if combo[1] == "swiglu" and K == 4128:
        K = 2080
    inputs, exact, floor = _case(M, K, N, combo)
    y = _op(_args(dev, inputs, combo[1], xdev(inputs[0]) if xdev else None), stream).cpu()
    err = rm.tile_rel(rd.tiles16(y), exact, 16)
    print(f"  M{M} K{K} N{N} {combo} stream {stream}: kernel {err:.3e} floor {floor:.3e} ratio {err / floor:.2f}")
    assert y.shape == (M, N) and y.dtype == torch.bfloat16 and torch.isfinite(y).all()
    assert floor > 0 and err <= 3 * floor
    return y


@pytest.mark.parametrize("M,K,N,combo,stream", CASES, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_stream_tilewise(dev, M, K, N, combo, stream):
    _check(dev, M, K, N, combo, stream)


@pytest.mark.parametrize("M,K,N,combo,stream", [(17, 4128, 272, LN, 2), (64, 8192, 48, PLAIN, 1)], ids=["staged", "global"])
def test_stream_strided_x(dev, M, K, N, combo, stream):
    """x as ``big[:, :K]``; everything of ``big`` that is not x is NaN."""
    def view(x):
        big = torch.full((M, K + 64), math.nan, dtype=torch.bfloat16)
        big[:, :K] = x
        return big.to(dev)[:, :K]

    _check(dev, M, K, N, combo, stream, xdev=view)


@pytest.mark.parametrize("M,K,N,combo,stream", [(9, 8960, 272, PLAIN, 3), (8, 2080, 272, RMS_SW, 2)], ids=["plain", "rms-swiglu"])
def test_stream_is_deterministic_and_graph_capturable(dev, M, K, N, combo, stream):
    """the same call twice gives the same bits; captured in a graph and replayed after x changed in
    place, the op gives the bits of the eager call on the new x (several replays)."""
    inputs, _, _ = _case(M, K, N, combo)
    xd = inputs[0].to(dev)
    args = _args(dev, inputs, combo[1], xd)
    bits = lambda t: t.contiguous().view(torch.int16)  # noqa: E731
    run = lambda: _op(args, stream)  # noqa: E731
    y0 = run()
    assert torch.equal(bits(y0), bits(run()))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        yg = run()
    for scale in (1.0, -0.5, 2.0):
        xd.copy_((inputs[0].float() * scale).bfloat16())
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(bits(yg), bits(run())), scale
    xd.copy_(inputs[0])
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits(yg), bits(y0))


def test_stream_out_of_range_is_refused(dev):
    x = torch.zeros(2, 64, dtype=torch.bfloat16, device=dev)
    w = torch.zeros(16, 64, dtype=torch.bfloat16, device=dev)
    for n in (3, 17, -1):  # more than K / 32 = 2 slices, more than the cap of 16, negative
        with pytest.raises(RuntimeError, match="K-slices"):
            torch.ops.nbd.linear_small(x, w, None, None, None, 0.0, 0, 0, None, n)
    assert torch.ops.nbd.linear_small(x, w, None, None, None, 0.0, 0, 0, None, 2).shape == (2, 16)
