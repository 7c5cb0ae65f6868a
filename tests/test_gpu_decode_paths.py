"""GPU numerics of the kernels that run on every generated token — ``linear_small``
(csrc/kernels/smallm.hip), ``decode_attn`` and ``greedy_advance`` (csrc/kernels/decode.hip) —
against the fp64 references of tests/refmath_decode.py, on structured inputs and on every path of
the kernels: the column-tile loop with its weight prefetch and re-fetched epilogue operands
(N = 16389: 1025 tiles on 512 workgroups), the fused norm above 8 rows and with several m-tiles
per workgroup, strided x, every query-group size 1 .. 8, every position of a 512 / 513 / 1024-row
cache (unsplit, first split, four chunks), cache rows >= pos — the row at pos included — holding
±30, ±3e38 or NaN.

``linear_small`` is called through ``torch.ops.nbd.linear_small``: the routing of
``ops.linear_small`` (library GEMM for the LM head from 4 rows, stand-alone norm above 8 rows)
cannot divert a case.

The bound is test_gpu_attn_paths.py's rule, not a fitted constant: ``floor = tile_rel(emulated
reference, fp64 reference)`` on the same inputs and ``tile_rel(kernel, fp64 reference) <= 3 x
floor`` per 16 x 16 output tile (linear_small) or per head row (decode).  tests/test_decode_ref.py
shows on the CPU that wrong formulas score >= 9 x floor on these inputs.  Run with ``-s`` for
every kernel/floor ratio and, at the end, the worst ones (docs/FINDINGS.md keeps the last
recorded figures)."""
import math

import pytest
import torch

import refmath as rm
import refmath_decode as rd
from nbdistributed_amd import ops
from nbdistributed_amd.ops.decode import partials_numel

pytestmark = pytest.mark.gpu

SCALE = rd.SCALE
WORST = {"linear_small": [0.0, ""], "decode out": [0.0, ""], "decode k row": [0.0, ""]}
_NORM = {None: 0, "ln": 1, "rms": 2}
_ACT = {"none": 0, "gelu": 1, "swiglu": 2}


@pytest.fixture(scope="module")
def dev(require_gpu):
    assert ops.native_available(), ops._load_error
    yield torch.device("cuda", 0)
    for what, (ratio, case) in WORST.items():
        print(f"\nworst {what} kernel/floor ratio (bound 3): {ratio:.2f}  {case}")


def _bits(t):
    return t.contiguous().view(torch.int16)


def _note(what, case, err, floor):
    ratio = err / floor if floor > 0 else (0.0 if err == 0 else math.inf)
    print(f"  {what} {case}: kernel {err:.3e} floor {floor:.3e} ratio {ratio:.2f}")
    if ratio > WORST[what][0]:
        WORST[what][0], WORST[what][1] = ratio, case
    return err <= 3 * floor


# ================================================================================ linear_small
def _linear_op(dev, x, w, b, nrm, act, rs):
    """``torch.ops.nbd.linear_small`` on device copies; ``x`` may already be a device view."""
    to = lambda t: None if t is None else t.to(dev)  # noqa: E731
    nw = to(nrm[1]) if nrm else None
    nb = to(nrm[2]) if nrm and nrm[0] == "ln" else None
    y = torch.ops.nbd.linear_small(to(x), to(w), to(b), nw, nb, float(nrm[-1]) if nrm else 0.0,
                                   _NORM[nrm[0] if nrm else None], _ACT[act], to(rs))
    torch.cuda.synchronize()
    return y.cpu()


def _linear_check(dev, case, inputs, act, xdev=None):
    x, w, b, nrm, rs = inputs
    exact = rd.tiles16(rd.linear_small_ref(x, w, b, nrm, act, rs))
    floor = rm.tile_rel(rd.tiles16(rd.linear_small_ref(x, w, b, nrm, act, rs, emulate=True)), exact, 16)
    y = _linear_op(dev, x if xdev is None else xdev, w, b, nrm, act, rs)
    N = w.shape[0] // 2 if act == "swiglu" else w.shape[0]
    assert y.shape == (x.shape[0], N) and y.dtype == torch.bfloat16
    ok = _note("linear_small", case, rm.tile_rel(rd.tiles16(y), exact, 16), floor)
    assert torch.isfinite(y).all(), case
    assert ok, (case, "tile_rel above 3 x floor")


def _fits(M, K, N, norm, act):
    """the op's own LDS formula (smallm.hip ``lds_bytes``, mirrored by ``linear_small_plan``)."""
    return rd.linear_small_plan(M, K, N, norm, act)[2] <= 160 * 1024


@pytest.mark.parametrize("M", rd.LINEAR_ROWS)
@pytest.mark.parametrize("combo", rd.LINEAR_COMBOS, ids=lambda c: "-".join(
    [str(c[0]), c[1]] + (["bias"] if c[2] else []) + (["res"] if c[3] else [])))
def test_linear_small_tilewise(dev, combo, M):
    """every shape of ``LINEAR_SHAPES``: one k-step (seven waves own nothing), three (an uneven
    wave split), 18, and SMAX full; N below a tile, ragged, >= 128 tiles (several m-tiles per
    workgroup) and 1025 tiles (the loop, the prefetch, the re-fetched bias / residual).  With a
    norm and M > 8 the prologue's second row per wave runs; with M > 16 on 2064 columns, MT > 1."""
    norm, act, _, _ = combo
    for K, N in rd.LINEAR_SHAPES:
        (M, K, N), inputs = rd.linear_case(M, K, N, combo)
        if not _fits(M, K, N, norm, act):  # (none does: test_decode_ref.py test_linear_plan_reaches_the_paths)
            print(f"  M{M} K{K} N{N}: over the LDS, skipped")
            continue
        _linear_check(dev, f"M{M} K{K} N{N} {norm}/{act}{'/bias' if combo[2] else ''}{'/res' if combo[3] else ''}",
                      inputs, act)


@pytest.mark.parametrize("M", [3, 17])
@pytest.mark.parametrize("combo", [("ln", "none", True, True), ("rms", "gelu", True, True), (None, "gelu", True, True)],
                         ids=["ln", "rms-gelu", "gelu"])
def test_linear_small_bias_and_residual_on_looped_tiles(dev, combo, M):
    """bias + residual together on N = 16389: workgroup g also computes tiles g + 512 (and g + 1024),
    whose bias and residual the epilogue fetches again (`first == false`)."""
    for K in (96, 576):
        (M, K, N), inputs = rd.linear_case(M, K, 16389, combo)
        assert rd.linear_small_plan(M, K, N, combo[0], combo[1])[3] == 512
        _linear_check(dev, f"M{M} K{K} N{N} {combo[0]}/{combo[1]}/bias/res", inputs, combo[1])


@pytest.mark.parametrize("view", ["row-strided", "last-token"])
def test_linear_small_strided_x(dev, view):
    """x as ``big[:, :K]`` (ldx = K + 64) and as the last token of a [M, T, K] block; everything
    of the parent that is not x is NaN."""
    for M, K, N, combo in ((9, 96, 16389, ("ln", "none", True, False)), (33, 576, 2064, (None, "none", True, True)),
                           (64, 4096, 48, ("rms", "none", False, True)),
                           (17, 2048, 272, ("rms", "swiglu", False, False))):
        (M, K, N), inputs = rd.linear_case(M, K, N, combo)
        x = inputs[0]
        if view == "row-strided":
            big = torch.full((M, K + 64), math.nan, dtype=torch.bfloat16)
            big[:, :K] = x
            xdev = big.to(dev)[:, :K]
            assert xdev.stride(0) == K + 64
        else:
            big = torch.full((M, 3, K), math.nan, dtype=torch.bfloat16)
            big[:, -1] = x
            xdev = big.to(dev)[:, -1]
            assert xdev.stride(0) == 3 * K
        assert not xdev.is_contiguous() or M == 1
        _linear_check(dev, f"{view} M{M} K{K} N{N} {combo[0]}/{combo[1]}", inputs, combo[1], xdev=xdev)


@pytest.mark.parametrize("K", [32, 96, 576, 2048, 4096])
def test_linear_small_permutation_is_bit_exact(dev, K):
    """w = a K x K permutation matrix: out == x[:, perm] bit for bit — every k position is read
    exactly once, in every wave's slice and every lane group's quarter, and lands in its column."""
    g = torch.Generator(device="cpu").manual_seed(K)
    perm = torch.randperm(K, generator=g)
    w = torch.zeros(K, K, dtype=torch.bfloat16)
    w[torch.arange(K), perm] = 1.0
    wd = w.to(dev)
    for M in (1, 16, 17, 64):
        x = (torch.randn(M, K, generator=g) * 10.0 ** (4 * torch.rand(M, 1, generator=g) - 2)).bfloat16()
        y = torch.ops.nbd.linear_small(x.to(dev), wd, None, None, None, 0.0, 0, 0, None)
        torch.cuda.synchronize()
        assert torch.equal(_bits(y.cpu()), _bits(x[:, perm])), (K, M)


def test_linear_small_rejects_bias_with_swiglu(dev):
    """the kernel's epilogue order is bias -> GELU -> SwiGLU -> residual; a bias under SwiGLU is
    defined nowhere (``ops.linear_small`` refuses it too)."""
    x = torch.zeros(2, 64, dtype=torch.bfloat16, device=dev)
    w = torch.zeros(32, 64, dtype=torch.bfloat16, device=dev)
    b = torch.zeros(16, dtype=torch.bfloat16, device=dev)
    with pytest.raises(RuntimeError, match="no bias with SwiGLU"):
        torch.ops.nbd.linear_small(x, w, b, None, None, 0.0, 0, 2, None)
    assert torch.ops.nbd.linear_small(x, w, None, None, None, 0.0, 0, 2, None).shape == (2, 16)
    with pytest.raises(ValueError, match="no bias with SwiGLU"):
        ops.linear_small(x, w, b, act="swiglu")


# ============================================================================ decode_attention
def _decode_check(dev, case, qkv, kc, vc, pos, H, rope_dev, kv_len_max=None, run=None):
    """one kernel call on device copies of (qkv, kc, vc): every figure printed, then every check.
    ``run``: replaces the call (graph replay); it returns (out, k_cache, v_cache) on the device."""
    B = qkv.shape[0]
    Hkv, Tmax = kc.shape[1], kc.shape[2]
    rope_cpu = None if rope_dev is None else (rope_dev[0].cpu(), rope_dev[1].cpu())
    exact = rd.decode_ref(qkv, kc, vc, pos, H, SCALE, rope_cpu)
    emu = rd.decode_ref(qkv, kc, vc, pos, H, SCALE, rope_cpu, emulate=True)
    bi, pt = torch.arange(B), torch.as_tensor(pos)
    floor = rm.tile_rel(rd.decode_per_head(emu[0], H), rd.decode_per_head(exact[0], H), 1)
    floor_k = rm.tile_rel(emu[1][bi, :, pt], exact[1][bi, :, pt], 1)
    if run is None:
        kd, vd = kc.to(dev), vc.to(dev)
        ws = torch.empty(partials_numel(B, H, Tmax), dtype=torch.float32, device=dev)
        out = ops.decode_attention(qkv.to(dev), kd, vd, pt.to(dev), H, scale=SCALE, rope=rope_dev,
                                   kv_len_max=kv_len_max, workspace=ws)
    else:
        out, kd, vd = run()
    torch.cuda.synchronize()
    out, kd, vd = out.cpu(), kd.cpu(), vd.cpu()
    assert out.shape == (B, H * 64) and out.dtype == torch.bfloat16
    ok = _note("decode out", case, rm.tile_rel(rd.decode_per_head(out, H), rd.decode_per_head(exact[0], H), 1), floor)
    ok_k = _note("decode k row", case, rm.tile_rel(kd[bi, :, pt], exact[1][bi, :, pt], 1), floor_k)
    assert torch.isfinite(out).all(), case
    # the v row at pos is the input's, bit for bit
    assert torch.equal(_bits(vd[bi, :, pt]), _bits(qkv[:, (H + Hkv) * 64:].reshape(B, Hkv, 64))), case
    # every other cache row is what it was (as int16: NaN poison compares equal)
    for new, old in ((kd, kc), (vd, vc)):
        want = old.clone()
        want[bi, :, pt] = new[bi, :, pt]
        assert torch.equal(_bits(new), _bits(want)), (case, "a row other than pos was written")
    assert ok, (case, "tile_rel above 3 x floor")
    assert ok_k, (case, "k row above 3 x floor")
    return out, kd, vd


@pytest.mark.parametrize("use_rope", [False, True], ids=["plain", "rope"])
@pytest.mark.parametrize("G", range(1, 9))
def test_decode_attention_every_group_size(dev, G, use_rope):
    """G = H / Hkv = 1 .. 8 (G = 5 and 6 ran in no test; G > 4 takes 2 keys in flight, not 4), two
    kv heads, a dozen positions: a 320-row cache (one chunk) and a 640-row one (three chunks of
    224: both chunk edges from both sides, empty chunks), in all three poison kinds."""
    for Tmax, poisons in ((320, ("huge", "nan")), (640, ("loud", "nan"))):
        rope = ops.rope_tables(Tmax, 64, 10000.0, dev) if use_rope else None
        for poison in poisons:
            H, Hkv, pos, (qkv, kc, vc) = rd.group_case(G, Tmax, poison, use_rope)
            _decode_check(dev, f"G{G} T{Tmax} {'rope' if use_rope else 'plain'} {poison}", qkv, kc, vc, pos, H, rope)


@pytest.mark.parametrize("G", [3, 6])
@pytest.mark.parametrize("kv_len", [512, 513, 1024])
def test_decode_attention_position_sweep(dev, kv_len, G):
    """every pos in [0, kv_len) — 512 the last unsplit bound, 513 the first split one (3 chunks of
    192), 1024 four chunks of 256 — 64 positions per launch, strided through the range: empty
    chunks, chunk edges, the 32-group edge, the 128- (G <= 4) or 64-key (G > 4) iteration edges and
    both parities of the double buffer are all hit, whatever ``plan()`` chooses.  The poison kind
    changes with the launch."""
    rope = ops.rope_tables(kv_len, 64, 10000.0, dev)
    hist = rd.sweep_history(kv_len, G)
    seen = set()
    for launch in range(-(-kv_len // rd.SWEEP_B)):
        pos = rd.sweep_positions(kv_len, launch)
        poison = rd.SWEEP_POISON[launch % 3]
        qkv, kc, vc = rd.decode_poison(hist, pos, poison)
        _decode_check(dev, f"sweep kv{kv_len} G{G} launch {launch} {poison}", qkv, kc, vc, pos, G, rope,
                      kv_len_max=kv_len)
        seen.update(pos)
    assert seen == set(range(kv_len))


def test_decode_attention_host_bound_below_the_cache(dev):
    """kv_len_max < Tmax (eager generation): the chunking follows the bound, rows past it — poison
    — are neither read nor written."""
    H, Hkv, Tmax = 6, 2, 1024
    rope = ops.rope_tables(Tmax, 64, 10000.0, dev)
    for bound, pos in ((1, (0, 0, 0)), (33, (0, 31, 32)), (513, (170, 171, 512)), (700, (0, 350, 699))):
        qkv, kc, vc = rd.decode_inputs(3, H, Hkv, Tmax, pos, seed=bound, poison="nan")
        _decode_check(dev, f"bound {bound} of {Tmax}", qkv, kc, vc, pos, H, rope, kv_len_max=bound)


def test_decode_attention_graph_replay_across_a_chunk_edge(dev):
    """one captured step (decode, then pos += 1 on the device) replayed from pos = 254 / 510 to
    257 / 513: the new row moves from the last row of a 256-key chunk into the next chunk, which
    was empty.  Every replay is checked like an eager call, against the cache as it then stands."""
    B, H, Hkv, Tmax = 2, 6, 2, 1024
    assert rd.decode_plan(B * Hkv, Tmax) == (4, 256)
    start = (254, 510)
    rope = ops.rope_tables(Tmax, 64, 10000.0, dev)
    hist = rd.decode_history(B, H, Hkv, Tmax, seed=99)
    q0, kc, vc = rd.decode_poison(hist, start, "nan")
    kd, vd = kc.to(dev), vc.to(dev)
    qd = q0.to(dev)
    pd = torch.tensor(start, dtype=torch.int64, device=dev)
    ws = torch.empty(partials_numel(B, H, Tmax), dtype=torch.float32, device=dev)
    ops.decode_attention(qd, kd, vd, pd, H, scale=SCALE, rope=rope, workspace=ws)  # warm-up
    torch.cuda.synchronize()
    kd.copy_(kc)
    vd.copy_(vc)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.decode_attention(qd, kd, vd, pd, H, scale=SCALE, rope=rope, workspace=ws)
        pd.add_(1)
    torch.cuda.synchronize()
    kd.copy_(kc)  # (capture launches nothing; restored all the same)
    vd.copy_(vc)
    pd.copy_(torch.tensor(start, dtype=torch.int64))
    g = torch.Generator(device="cpu").manual_seed(5)
    for step in range(4):
        pos = tuple(s + step for s in start)
        qkv = (q0.float() + 0.5 * torch.randn(q0.shape, generator=g)).bfloat16()  # a new token's projection
        qd.copy_(qkv)
        before_k, before_v = kd.cpu(), vd.cpu()

        def run():
            graph.replay()
            return out, kd, vd

        _decode_check(dev, f"graph step {step} pos {pos}", qkv, before_k, before_v, pos, H, rope, run=run)
        assert pd.cpu().tolist() == [p + 1 for p in pos]


# ============================================================================== greedy_advance
def _greedy(dev, logits, pos, T=6, out=None, done=None, eos=-1):
    B = logits.shape[0]
    tok = torch.full((B,), -7, dtype=torch.int64, device=dev)
    pd = torch.tensor(pos, dtype=torch.int64, device=dev)
    if out is None:
        out = torch.full((B, T), -1, dtype=torch.int64, device=dev)
    torch.ops.nbd.greedy_advance(logits, tok, pd, out, done, eos)
    torch.cuda.synchronize()
    return tok.cpu(), pd.cpu(), out


def test_greedy_advance_nan_and_inf_rows(dev):
    """an all-NaN row gives token 0; an all -inf row gives its first index, like torch.argmax; a
    NaN beside finite logits never wins."""
    V = 1000
    logits = torch.randn(4, V).bfloat16()
    logits[0] = math.nan
    logits[1] = -math.inf
    logits[2, ::2] = math.nan
    logits[3, :-1] = -math.inf  # the only finite logit is the last
    tok, pos, out = _greedy(dev, logits.to(dev), [0, 1, 2, 3])
    want2 = int(torch.where(logits[2].isnan(), -math.inf, logits[2].double()).argmax())
    assert tok.tolist() == [0, 0, want2, V - 1]
    assert pos.tolist() == [1, 2, 3, 4]
    assert out.cpu().tolist() == [[-1, 0, -1, -1, -1, -1], [-1, -1, 0, -1, -1, -1], [-1, -1, -1, want2, -1, -1],
                                  [-1, -1, -1, -1, V - 1, -1]]


@pytest.mark.parametrize("V", [1, 7, 8, 9])
def test_greedy_advance_tiny_vocabularies(dev, V):
    """V below, at and just above one 16-B load: the maximum at every index in turn, on aligned
    rows (ld = 16) and unaligned ones (ld = V odd: the scalar path)."""
    for ld in {16, V}:
        base = torch.full((V, ld), -3.0, dtype=torch.bfloat16)
        base[torch.arange(V), torch.arange(V)] = 2.0  # row b peaks at b
        logits = base.to(dev)[:, :V]
        tok, pos, out = _greedy(dev, logits, [0] * V)
        assert tok.tolist() == list(range(V)), (V, ld)
        assert out[:, 1].cpu().tolist() == list(range(V)) and pos.tolist() == [1] * V


def test_greedy_advance_maximum_in_the_scalar_tail(dev):
    """an aligned row of V = 8·n + r: the maximum among the last r logits, read by the scalar tail
    after the 16-B loop; ties between the vector part and the tail go to the lower index."""
    for V in (8 * 1024 + 3, 50257, 16 + 7):
        logits = torch.randn(3, V + (-V) % 8).bfloat16().clamp(-4, 4)
        logits[0, V - 1] = 9.0
        logits[1, V - (V % 8)] = 9.0  # the first scalar element
        logits[2, 5] = logits[2, V - 1] = 9.0  # a tie: index 5 wins
        logits[:, V:] = 50.0  # the row padding past V is not a logit
        ld = logits.to(dev)[:, :V]
        assert ld.data_ptr() % 16 == 0 and ld.stride(0) % 8 == 0
        tok, _, _ = _greedy(dev, ld, [0, 0, 0])
        assert tok.tolist() == [V - 1, V - (V % 8), 5], V


def test_greedy_advance_writes_nothing_past_the_end(dev):
    """pos + 1 == T: nothing is written, anywhere in ``out`` — also when ``out`` is a row-strided
    view of a wider buffer, whose other columns stay as they were."""
    B, T, V = 4, 6, 64
    logits = torch.randn(B, V).bfloat16().to(dev)
    want = logits.float().argmax(-1).cpu()
    pos = [T - 1, T - 2, -1, 10 ** 6]  # past the end, the last slot, slot 0, far past
    tok, p2, out = _greedy(dev, logits, pos, T=T)
    ref = torch.full((B, T), -1, dtype=torch.int64)
    ref[1, T - 1] = want[1]
    ref[2, 0] = want[2]
    assert torch.equal(out.cpu(), ref) and torch.equal(tok, want) and p2.tolist() == [p + 1 for p in pos]
    big = torch.full((B, T + 5), -1, dtype=torch.int64, device=dev)
    view = big[:, 2:2 + T]
    assert view.stride(0) == T + 5
    _greedy(dev, logits, pos, out=view)
    ref_big = torch.full((B, T + 5), -1, dtype=torch.int64)
    ref_big[:, 2:2 + T] = ref
    assert torch.equal(big.cpu(), ref_big)
