"""GPU: decode attention over an fp8 (``float8_e4m3fn``, no scales) KV cache —
csrc/kernels/decode.hip ``decode_kernel<G, true>`` — and ``generate(kv_dtype="fp8")``.

Two rules, on the smallest shapes at which each path can go wrong:
  * the row the kernel stores at ``pos`` is a bit pattern: ``q8`` (torch, on the CPU) of the row the
    bf16 kernel writes for the same call, byte for byte (both NaN codes count as NaN: torch's own
    CPU casts do not agree on a NaN's sign), every other byte of both caches untouched;
  * the output against ``refmath_kv8.decode8_ref`` in fp64 on the cache as stored, the row at
    ``pos`` as the kernel stored it (the first rule proved it right): ``tile_rel(kernel, exact) <=
    3 x floor`` per head row, ``floor = tile_rel(emulated, exact)`` on the same inputs.
    tests/test_kv8_ref.py shows on the CPU that wrong formulas score >= 9 x floor, or change the
    stored bytes, on these inputs.  Run with ``-s`` for every kernel/floor ratio."""
import copy
import math

import pytest
import torch

import refmath as rm
import refmath_decode as rd
import refmath_kv8 as r8
from nbdistributed_amd import ops
from nbdistributed_amd.generation import KVCache
from nbdistributed_amd.ops.decode import partials_numel

pytestmark = pytest.mark.gpu

SCALE = rd.SCALE
F8 = torch.float8_e4m3fn
WORST = [0.0, ""]


@pytest.fixture(scope="module")
def dev(require_gpu):
    assert ops.native_available(), ops._load_error
    yield torch.device("cuda", 0)
    print(f"\nworst fp8 decode kernel/floor ratio (bound 3): {WORST[0]:.2f}  {WORST[1]}")


def _check8(dev, case, qkv, k8, v8, pos, H, rope_dev, kv_len_max=None, run=None, check_out=True):
    """one fp8 kernel call on device copies of (qkv, k8, v8), and the bf16 kernel on a bf16 copy of
    the same case for the rows it writes.  ``run``: replaces the fp8 call (graph replay); it
    returns (out, k_cache, v_cache) on the device."""
    B = qkv.shape[0]
    Hkv, Tmax = k8.shape[1], k8.shape[2]
    bi, pt = torch.arange(B), torch.as_tensor(pos)
    ws = torch.empty(partials_numel(B, H, Tmax), dtype=torch.float32, device=dev)
    k16, v16 = k8.to(torch.bfloat16).to(dev), v8.to(torch.bfloat16).to(dev)  # exact; the NaN byte is NaN
    ops.decode_attention(qkv.to(dev), k16, v16, pt.to(dev), H, scale=SCALE, rope=rope_dev, kv_len_max=kv_len_max,
                         workspace=ws)
    torch.cuda.synchronize()
    want_k, want_v = r8.q8(k16.cpu()[bi, :, pt]), r8.q8(v16.cpu()[bi, :, pt])
    if run is None:
        kd, vd = k8.to(dev), v8.to(dev)
        out = ops.decode_attention(qkv.to(dev), kd, vd, pt.to(dev), H, scale=SCALE, rope=rope_dev,
                                   kv_len_max=kv_len_max, workspace=ws)
    else:
        out, kd, vd = run()
    torch.cuda.synchronize()
    out, kd, vd = out.cpu(), kd.cpu(), vd.cpu()
    assert out.shape == (B, H * 64) and out.dtype == torch.bfloat16
    assert kd.dtype == F8 and vd.dtype == F8
    # 1. the stored rows, bit for bit; every other byte as it was
    for what, new, old, want in (("k", kd, k8, want_k), ("v", vd, v8, want_v)):
        got = new[bi, :, pt]
        diff = r8.canon8(got) != r8.canon8(want)
        assert not diff.any(), (case, what, "stored row differs from q8 of the bf16 kernel's row", int(diff.sum()),
                                r8.bits8(got)[diff][:8].tolist(), r8.bits8(want)[diff][:8].tolist())
        keep = r8.bits8(old).clone()
        keep[bi, :, pt] = r8.bits8(new)[bi, :, pt]
        assert torch.equal(r8.bits8(new), keep), (case, what, "a byte outside the row at pos was written")
    if not check_out:
        return out, kd, vd
    # 2. the output over the cache as stored
    rope_cpu = None if rope_dev is None else (rope_dev[0].cpu(), rope_dev[1].cpu())
    q = qkv[:, : H * 64]
    kn, vn = kd[bi, :, pt], vd[bi, :, pt]
    exact = r8.decode8_ref(q, k8, v8, kn, vn, pos, H, SCALE, rope_cpu)
    emu = r8.decode8_ref(q, k8, v8, kn, vn, pos, H, SCALE, rope_cpu, emulate=True)
    floor = rm.tile_rel(rd.decode_per_head(emu, H), rd.decode_per_head(exact, H), 1)
    err = rm.tile_rel(rd.decode_per_head(out, H), rd.decode_per_head(exact, H), 1)
    ratio = err / floor if floor > 0 else (0.0 if err == 0 else math.inf)
    print(f"  fp8 decode {case}: kernel {err:.3e} floor {floor:.3e} ratio {ratio:.2f}")
    if ratio > WORST[0]:
        WORST[0], WORST[1] = ratio, case
    assert torch.isfinite(out).all(), case
    assert err <= 3 * floor, (case, "tile_rel above 3 x floor", err, floor)
    return out, kd, vd


@pytest.mark.parametrize("use_rope", [False, True], ids=["plain", "rope"])
@pytest.mark.parametrize("G", range(1, 9))
def test_fp8_decode_every_group_size(dev, G, use_rope):
    """G = H / Hkv = 1 .. 8, two kv heads, the dozen positions of ``refmath_decode.GROUP_POS``: a
    320-row cache (one chunk) and a 640-row one (three chunks of 224: both chunk edges from both
    sides, empty chunks); rows >= pos hold the NaN byte, then ±448."""
    for Tmax in (320, 640):
        rope = ops.rope_tables(Tmax, 64, 10000.0, dev) if use_rope else None
        for poison in r8.KV8_POISON:
            H, Hkv, pos, (qkv, k8, v8) = r8.group_case8(G, Tmax, poison, use_rope)
            _check8(dev, f"G{G} T{Tmax} {'rope' if use_rope else 'plain'} {poison}", qkv, k8, v8, pos, H, rope)


@pytest.mark.parametrize("use_rope", [False, True], ids=["plain", "rope"])
def test_fp8_decode_stores_the_bounds_and_nan(dev, use_rope):
    """±inf, NaN of both signs and finite values beyond ±448 in the incoming k and v: the stored
    bytes are ±448 and NaN, as ``q8`` on the CPU makes them of the bf16 kernel's rows."""
    H, Hkv, pos, (qkv, k8, v8) = r8.saturating_case(use_rope)
    rope = ops.rope_tables(320, 64, 10000.0, dev) if use_rope else None
    _, kd, vd = _check8(dev, f"saturating {'rope' if use_rope else 'plain'}", qkv, k8, v8, pos, H, rope, check_out=False)
    bi, pt = torch.arange(len(pos)), torch.as_tensor(pos)
    vin = qkv[:, (H + Hkv) * 64:].reshape(len(pos), Hkv, 64)
    vb = r8.bits8(vd[bi, :, pt])
    assert (vb[vin == math.inf] == 0x7E).all() and (vb[vin == -math.inf] == 0xFE).all()
    assert (vb[vin.float() >= 449.0] == 0x7E).all() and (vb[vin.float() <= -449.0] == 0xFE).all()
    assert (vb[vin.isnan()] & 0x7F == 0x7F).all() and (vb[~vin.isnan()] & 0x7F != 0x7F).all()
    kb = r8.bits8(kd[bi, :, pt])
    assert (kb & 0x7F == 0x7F).any()
    if use_rope:  # (a rotation turns inf · 0 and inf − inf into further NaN)
        assert (kb & 0x7F == 0x7E).any()
    else:
        assert int((kb & 0x7F == 0x7E).sum()) == 8 * len(pos) * Hkv


@pytest.mark.parametrize("G", [3, 6])
@pytest.mark.parametrize("kv_len", [512, 513])
def test_fp8_decode_position_sweep(dev, kv_len, G):
    """every pos in [0, kv_len) at the last unsplit bound (512) and the first split one (513: three
    chunks of 192), 64 positions per launch as ``refmath_decode.sweep_positions`` lays them out;
    the poison kind changes with the launch."""
    rope = ops.rope_tables(kv_len, 64, 10000.0, dev)
    hist = r8.sweep_history8(kv_len, G)
    seen = set()
    for launch in range(-(-kv_len // rd.SWEEP_B)):
        pos = rd.sweep_positions(kv_len, launch)
        poison = r8.SWEEP_POISON8[launch % 2]
        qkv, k8, v8 = r8.kv8_poison(hist, pos, poison)
        _check8(dev, f"sweep kv{kv_len} G{G} launch {launch} {poison}", qkv, k8, v8, pos, G, rope, kv_len_max=kv_len)
        seen.update(pos)
    assert seen == set(range(kv_len))


def test_fp8_decode_graph_replay_across_a_chunk_edge(dev):
    """one captured step (decode, then pos += 1 on the device) replayed from pos = 254 / 510 to
    257 / 513: the new row moves from the last row of a 256-key chunk into the next chunk, which
    was empty.  Every replay is checked like an eager call, against the cache as it then stands."""
    B, H, Hkv, Tmax = 2, 6, 2, 1024
    assert rd.decode_plan(B * Hkv, Tmax) == (4, 256)
    start = (254, 510)
    rope = ops.rope_tables(Tmax, 64, 10000.0, dev)
    hist = rd.decode_history(B, H, Hkv, Tmax, seed=99)
    q0, k8, v8 = r8.kv8_poison(hist, start, "nan")
    kd, vd = k8.to(dev), v8.to(dev)
    qd = q0.to(dev)
    pd = torch.tensor(start, dtype=torch.int64, device=dev)
    ws = torch.empty(partials_numel(B, H, Tmax), dtype=torch.float32, device=dev)
    ops.decode_attention(qd, kd, vd, pd, H, scale=SCALE, rope=rope, workspace=ws)  # warm-up
    torch.cuda.synchronize()
    kd.copy_(k8)
    vd.copy_(v8)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.decode_attention(qd, kd, vd, pd, H, scale=SCALE, rope=rope, workspace=ws)
        pd.add_(1)
    torch.cuda.synchronize()
    kd.copy_(k8)  # (capture launches nothing; restored all the same)
    vd.copy_(v8)
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

        _check8(dev, f"graph step {step} pos {pos}", qkv, before_k, before_v, pos, H, rope, run=run)
        assert pd.cpu().tolist() == [p + 1 for p in pos]


@pytest.mark.parametrize("use_rope", [False, True], ids=["plain", "rope"])
def test_fp8_prefill_store_bytes(dev, use_rope):
    """``KVCache.store`` on the GPU: the bytes it writes are ``q8`` on the CPU of the rows a bf16
    cache gets from the same call — ordinary values, subnormals of e4m3, values beyond ±448, ±inf,
    NaN."""
    B, T, H, Hkv = 2, 40, 4, 2
    g = torch.Generator(device="cpu").manual_seed(11)
    qkv = 2.0 * torch.randn(B, T, (H + 2 * Hkv) * 64, generator=g)
    qkv[:, ::5] *= 2.0 ** -8  # e4m3 subnormals and values that round to zero
    kv = qkv[:, :, H * 64:]
    kv[:, 3, ::7] = 1000.0
    kv[:, 4, ::7] = -460.0
    kv[:, 5, ::9] = math.inf
    kv[:, 6, ::9] = -math.inf
    kv[:, 7, ::11] = math.nan
    qkv = qkv.bfloat16().to(dev)
    rope = ops.rope_tables(64, 64, 10000.0, dev) if use_rope else None
    c16 = KVCache(1, B, H, Hkv, 64, 64, dtype=torch.bfloat16, device=dev)
    c8 = KVCache(1, B, H, Hkv, 64, 64, dtype=F8, device=dev)
    c16.store(0, qkv.clone(), rope=rope)
    c8.store(0, qkv.clone(), rope=rope)
    torch.cuda.synchronize()
    for what, a16, a8 in (("k", c16.k, c8.k), ("v", c16.v, c8.v)):
        a16, a8 = a16.cpu(), a8.cpu()
        assert a16[..., :T, :].float().abs().nan_to_num(0.0).max() > 0
        diff = r8.canon8(r8.q8(a16)) != r8.canon8(a8)
        assert not diff.any(), (what, int(diff.sum()), r8.bits8(a8)[diff][:8].tolist(), r8.bits8(r8.q8(a16))[diff][:8].tolist())
        b = r8.bits8(a8)
        assert (b & 0x7F == 0x7E).any() and (b & 0x7F == 0x7F).any() and ((b & 0x78 == 0) & (b & 0x07 != 0)).any()
        assert (b[..., T:, :] == 0).all()


def test_fp8_decode_checks_its_caches(dev):
    """both caches fp8, contiguous, rows of 64; the bf16 path's message is what it was."""
    B, H, Hkv, T = 2, 4, 2, 64
    qkv = torch.zeros(B, (H + 2 * Hkv) * 64, dtype=torch.bfloat16, device=dev)
    pos = torch.zeros(B, dtype=torch.int64, device=dev)
    k8 = torch.zeros(B, Hkv, T, 64, dtype=F8, device=dev)
    k16 = torch.zeros(B, Hkv, T, 64, dtype=torch.bfloat16, device=dev)
    ws = torch.empty(partials_numel(B, H, T), dtype=torch.float32, device=dev)
    call = lambda k, v: torch.ops.nbd.decode_attn(qkv, k, v, pos, H, 0.125, T, None, None, ws)  # noqa: E731
    with pytest.raises(RuntimeError, match="fp8 caches must be contiguous float8_e4m3fn"):
        call(k8, k16)
    with pytest.raises(RuntimeError, match="fp8 caches must be contiguous float8_e4m3fn"):
        call(torch.zeros(B, Hkv, T, 128, dtype=F8, device=dev)[..., :64], k8.clone())
    with pytest.raises(RuntimeError, match=r"caches must be contiguous bf16 \[B, Hkv, Tmax, 64\]"):
        call(k16, k8)
    assert call(k8, k8.clone()).shape == (B, H * 64)
    torch.cuda.synchronize()


def _peaked(model):
    # scale the embedding (tied LM head) so greedy tokens are far from ties under bf16 rounding
    with torch.no_grad():
        emb = model.wte.weight if hasattr(model, "wte") else model.model.embed_tokens.weight
        emb.mul_(8.0)
    return model


@pytest.mark.parametrize("family", ["gpt2", "llama"])
def test_fp8_generate_graph_matches_eager_and_the_cpu_path(dev, family):
    """graphed and eager ``generate(kv_dtype="fp8")`` give equal tokens; the decode-step logits go
    against the same weights in fp32 on the CPU decoding with an fp8 ``KVCache`` through the PyTorch
    path (the same quantised semantics): within 5 % of the largest logit, equal arg-max — the
    comparison and bound of the bf16 end-to-end test."""
    from nbdistributed_amd.models import GPT2, GPT2Config
    from nbdistributed_amd.models.llama import LlamaConfig, LlamaForCausalLM

    torch.manual_seed(0)
    if family == "gpt2":
        m = GPT2(GPT2Config(vocab_size=512, n_positions=512, n_embd=256, n_layer=2, n_head=4))
    else:
        m = LlamaForCausalLM(LlamaConfig.tiny())
    m = _peaked(m.to("cuda", torch.bfloat16).eval())
    ids = torch.randint(1, 512, (4, 40), device="cuda")
    lens = torch.tensor([40, 33, 12, 1], device="cuda")
    eager, cache = m.generate(ids, 24, lengths=lens, graph=False, kv_dtype="fp8", return_cache=True)
    graphed = m.generate(ids, 24, lengths=lens, graph=True, kv_dtype="fp8")
    assert cache.k.dtype == F8 and cache.k.is_cuda
    assert torch.equal(eager, graphed)
    ref = copy.deepcopy(m).float().cpu()
    seq = eager[0:1, :40 + 24]
    cg = KVCache.for_model(m, 1, 128, dtype=F8)
    cc = KVCache.for_model(ref, 1, 128, dtype=F8)
    m.prefill(torch.nn.functional.pad(seq[:, :40], (0, 88)), cg, torch.tensor([40], device="cuda"))
    ref.prefill(seq[:, :40].cpu(), cc, torch.tensor([40]))
    worst = 0.0
    for t in range(40, 48):
        lg = m.decode_step(seq[:, t], torch.tensor([t], device="cuda"), cg).float().cpu()
        full = ref.decode_step(seq[:, t].cpu(), torch.tensor([t]), cc).float()
        rel = (lg[0] - full[0]).abs().max().item() / full.abs().max().item()
        worst = max(worst, rel)
        print(f"  {family} step {t}: max |dlogit| / max |logit| = {rel:.4f}")
        assert rel < 0.05, (family, t, rel)
        assert int(lg.argmax()) == int(full.argmax())
    print(f"  {family}: worst {worst:.4f} (bound 0.05)")
