"""GPU numerics of packed-sequence (document-masked) attention: ``nbd::packed_bounds``
(csrc/kernels/packed.hip), the SEG kernels of csrc/kernels/attn.hip behind ``nbd::attn_fwd_packed`` /
``attn_bwd_packed``, and a tiny Llama fed ``position_ids``.

Kernel level, as tests/test_gpu_attn_paths.py: structured inputs (``rm.attn_inputs`` / ``rm.attn_do``),
``tile_rel(kernel, fp64) <= 3 x tile_rel(emulated, fp64)`` per 32-row tile for out, dq, dk, dv and the
same factor on the maximum absolute deviation of lse — against tests/refmath_packed.py, whose mutants
tests/test_packed_ref.py shows to score >= 9 x floor on these very layouts.  Run with ``-s`` for every
measured figure."""
import math

import pytest
import torch

import refmath as rm
import refmath_packed as rp
from nbdistributed_amd import ops
from nbdistributed_amd.models.llama import LlamaConfig, LlamaForCausalLM

pytestmark = pytest.mark.gpu

SCALE = 0.125
NAMES = ("out", "lse", "dq", "dk", "dv")


@pytest.fixture(scope="module")
def dev(require_gpu):
    assert ops.native_available(), ops._load_error
    return torch.device("cuda", 0)


def _compare(case, got, exact, emu, names=NAMES, first=0):
    """every output within 3 x the emulated reference's own error; ``first``: only rows >= first
    contribute error (tile maxima and the floor still come from the whole reference).  All figures
    are printed before the assertion."""
    bad = []
    for n, x, r, e in zip(names, got, exact, emu):
        x = x.detach().double().clone()
        r = r.to(x.device)
        if first:
            x[:, :, :first] = r[:, :, :first]
        if n == "lse":
            err, floor = rm.max_abs(x, r), rm.max_abs(e, r)
        else:
            err, floor = rm.tile_rel(x, r, 32), rm.tile_rel(e, r, 32)
        ratio = err / floor if floor > 0 else (0.0 if err == 0 else math.inf)
        print(f"  {case} {n}: kernel {err:.3e} floor {floor:.3e} ratio {ratio:.2f}")
        if not err <= 3 * floor:
            bad.append((n, err, floor))
    assert not bad, (case, bad)


def _kernel(q, k, v, do, rope, bounds):
    cos, sin = rope if rope is not None else (None, None)
    o, lse = torch.ops.nbd.attn_fwd_packed(q, k, v, SCALE, cos, sin, bounds.kstart)
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    torch.ops.nbd.attn_bwd_packed(do, q, k, v, o, lse, SCALE, dq, dk, dv, cos, sin, bounds.kstart, bounds.qend)
    torch.cuda.synchronize()
    return o, lse, dq, dk, dv


def _gsplit(B, H, Hkv, T):
    """attn_bwd_hip: a query-head group is split over workgroups when B·Hkv·T/128 < 128."""
    return H // Hkv > 1 and B * Hkv * (T // 128) < 128


def _bounds(rows, T, dev):
    """bounds from the kernel under test, checked against the lengths they were built from."""
    ks, qe, pos = rp.bounds_of_lengths(rows, T)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    b = ops.packed_bounds(pos.to(dev), bad)
    assert torch.equal(b.kstart.cpu().long(), ks) and torch.equal(b.qend.cpu().long(), qe) and int(bad) == 0
    return b, ks.to(dev)


def _run_layout(dev, rows, T, H, Hkv, use_rope, seed, chunk=None):
    B = len(rows)
    rope = ops.rope_tables(T, 64, 10000.0, dev) if use_rope else None
    bounds, ks = _bounds(rows, T, dev)
    q, k, v = (t.to(dev) for t in rm.attn_inputs(B, H, Hkv, T, seed))
    do = rm.attn_do(rp.attn_ref_packed(q, k, v, None, SCALE, ks, rope=rope, chunk=chunk)[0], seed + 1)
    got = _kernel(q, k, v, do, rope, bounds)
    for n, t in zip(NAMES, got):
        assert bool(torch.isfinite(t).all()), n
    exact = rp.attn_ref_packed(q, k, v, do, SCALE, ks, rope=rope, chunk=chunk)
    emu = rp.attn_ref_packed(q, k, v, do, SCALE, ks, rope=rope, emulate=True, gsplit=_gsplit(B, H, Hkv, T),
                             chunk=chunk)
    return got, exact, emu


@pytest.mark.parametrize("use_rope", [False, True], ids=["plain", "rope"])
@pytest.mark.parametrize("H,Hkv", [(2, 2), (4, 2)], ids=["mha", "gqa-split"])
@pytest.mark.parametrize("layout", list(rp.LAYOUTS))
def test_packed_attention_layouts(dev, layout, H, Hkv, use_rope):
    """the layouts of refmath_packed.LAYOUTS (what each exercises is said there); the 4/2 cases at
    B <= 2 reach the GQA split and gqa_reduce_kernel."""
    T, rows = rp.LAYOUTS[layout]
    assert H == Hkv or _gsplit(len(rows), H, Hkv, T)
    got, exact, emu = _run_layout(dev, rows, T, H, Hkv, use_rope, seed=T + 10 * H + len(rows))
    _compare(f"{layout} H{H}/{Hkv} {'rope' if use_rope else 'plain'}", got, exact, emu)


def test_packed_attention_gqa_unsplit(dev):
    """B 64, H 4/1, T 256: B·Hkv·T/128 = 128, the group swept by one workgroup; every row 80+176."""
    B, H, Hkv, T = 64, 4, 1, 256
    assert not _gsplit(B, H, Hkv, T)
    got, exact, emu = _run_layout(dev, [[80, 176]] * B, T, H, Hkv, True, seed=64, chunk=16)
    _compare("gqa-unsplit B64 H4/1 T256 80+176", got, exact, emu)


def test_trivial_bounds_give_the_causal_kernels_bits(dev):
    """one document per row: the finite running-maximum floor rescales by exactly 0 where the
    causal kernel's -inf does, and no bound compare is taken — same bits as attn_fwd / attn_bwd."""
    B, H, Hkv, T = 2, 4, 2, 384
    rope = ops.rope_tables(T, 64, 10000.0, dev)
    bounds, _ = _bounds([[T]] * B, T, dev)
    q, k, v = (t.to(dev) for t in rm.attn_inputs(B, H, Hkv, T, 11))
    do = torch.randn(B, H, T, 64, device=dev).bfloat16()
    got = _kernel(q, k, v, do, rope, bounds)
    o, lse = torch.ops.nbd.attn_fwd(q, k, v, True, SCALE, rope[0], rope[1])
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    torch.ops.nbd.attn_bwd(do, q, k, v, o, lse, True, SCALE, dq, dk, dv, rope[0], rope[1])
    for n, a, b in zip(NAMES, got, (o, lse, dq, dk, dv)):
        assert torch.equal(a, b), n


@pytest.mark.parametrize("use_rope", [False, True], ids=["plain", "rope"])
@pytest.mark.parametrize("T,lens", [(384, [128, 256]), (256, [80, 176])], ids=["128+256", "80+176"])
def test_packed_attention_isolates_documents(dev, T, lens, use_rope):
    """The first document poisoned: its keys score 25 nats above every legitimate score (the keys of
    ``rm.poisoned_inputs`` with every position poisoned, taken for the first document only), its
    values are ±1024 and dO is zero on its rows.  dq, dk, dv on its rows must be exactly zero, and
    the second document's five outputs stay within 3 x floor of the UNPOISONED problem's reference
    (not bit-equal to an unpoisoned run: the deferred-rescale decision is wave-wide)."""
    B, H, Hkv, cut = 1, 4, 2, lens[0]
    rope = ops.rope_tables(T, 64, 10000.0, dev) if use_rope else None
    (q, k, v), (_, kp, vp) = rm.poisoned_inputs(B, H, Hkv, T, 0, seed=23, scale=SCALE, rope=rope)
    kp[:, :, cut:], vp[:, :, cut:] = k[:, :, cut:], v[:, :, cut:]
    q, k, v, kp, vp = (t.to(dev) for t in (q, k, v, kp, vp))
    bounds, ks = _bounds([lens], T, dev)
    do = rm.attn_do(rp.attn_ref_packed(q, k, v, None, SCALE, ks, rope=rope)[0], 24)
    exact = rp.attn_ref_packed(q, k, v, do, SCALE, ks, rope=rope)
    emu = rp.attn_ref_packed(q, k, v, do, SCALE, ks, rope=rope, emulate=True, gsplit=_gsplit(B, H, Hkv, T))
    dop = do.clone()
    dop[:, :, :cut] = 0
    got = _kernel(q, kp, vp, dop, rope, bounds)
    for n, t in zip(NAMES, got):
        assert bool(torch.isfinite(t).all()), n
    for n, t in zip(NAMES[2:], got[2:]):
        assert bool((t[:, :, :cut] == 0).all()), (n, float(t[:, :, :cut].float().abs().max()))
    _compare(f"isolation {lens} {'rope' if use_rope else 'plain'}", got, exact, emu, first=cut)


@pytest.mark.parametrize("B,T", [(1, 1), (5, 10), (3, 100), (2, 1000), (9, 256)])
def test_packed_bounds_kernel_matches_the_torch_path(dev, B, T):
    """rows shorter and longer than a wave's 64-position step, more rows than one workgroup's four
    waves, documents of length 1; then the same rows with one broken, which sets the flag."""
    g = torch.Generator().manual_seed(B * 1000 + T)
    start = torch.rand(B, T, generator=g) < 0.08
    start[:, 0] = True
    if T > 3:
        start[0, 1:3] = True  # documents of length 1
    idx = torch.arange(T).expand(B, T)
    pos = idx - torch.where(start, idx, -1).cummax(1).values
    for broken in (False, True):
        if broken:
            if T < 2:
                continue
            pos = pos.clone()
            pos[B - 1, T - 1] += 2
        want_bad = torch.zeros(1, dtype=torch.int32)
        want = ops.packed_bounds(pos, want_bad)
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
        got = ops.packed_bounds(pos.to(dev), bad)
        assert torch.equal(got.kstart.cpu(), want.kstart) and torch.equal(got.qend.cpu(), want.qend)
        assert int(bad) == int(want_bad) == int(broken)


# ------------------------------------------------------------------------------------ model level
def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-300))


def _tiny(dev, dtype):
    torch.manual_seed(1)
    c = LlamaConfig(vocab_size=512, hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2,
                    num_key_value_heads=1, max_position_embeddings=256)
    return LlamaForCausalLM(c).to(dev, dtype)


def _per_document(model, docs, pad_to=None):
    """the documents one at a time (``pad_to``: right-padded to a multiple of it, pad targets
    ignored): real-token logits, the token-mean loss over all documents, every parameter gradient."""
    model.zero_grad()
    logits, total, count = [], 0.0, 0
    for d in docs:
        n = d.numel()
        ids, labels = d[None], d[None]
        if pad_to:
            P = -(-n // pad_to) * pad_to
            ids = torch.cat([d, d.new_zeros(P - n)])[None]
            labels = torch.cat([d, d.new_full((P - n,), -100)])[None]
        out = model(ids, labels=labels)
        logits.append(out.logits[0, :n].detach().float())
        total = total + out.loss.float() * (n - 1)
        count += n - 1
    loss = total / count
    loss.backward()
    return torch.cat(logits), loss.detach(), {n: p.grad.detach().float().clone() for n, p in model.named_parameters()}


def test_tiny_llama_packed_row_bf16(dev):
    """80 + 176 in one row of 256, bf16, against the fp32 module path run one document at a time;
    the floor is the error of today's unpacked bf16 HIP path on the same documents (each
    right-padded to a multiple of 128) against that reference, the bound 3 x floor for the
    real-token logits, the loss and every parameter gradient (max-abs over the tensor's max-abs)."""
    g = torch.Generator().manual_seed(5)
    docs = [torch.randint(1, 512, (n,), generator=g).to(dev) for n in (80, 176)]
    ref_model = _tiny(dev, torch.float32)
    hook = ref_model.model.layers[0].register_forward_hook(lambda *a: None)  # the module path
    want = _per_document(ref_model, docs)
    hook.remove()
    model = _tiny(dev, torch.bfloat16)
    floor = _per_document(model, docs, pad_to=128)
    model.zero_grad()
    ids = torch.cat(docs)[None]
    pos = torch.cat([torch.arange(d.numel(), device=dev) for d in docs])[None]
    out = model(input_ids=ids, labels=ids, position_ids=pos)
    out.loss.backward()
    torch.cuda.synchronize()
    got = (out.logits[0].detach().float(), out.loss.detach().float(),
           {n: p.grad.detach().float() for n, p in model.named_parameters()})
    rows = [("logits", got[0], floor[0], want[0]), ("loss", got[1], floor[1], want[1])]
    rows += [(f"grad {n}", got[2][n], floor[2][n], want[2][n]) for n in want[2]]
    bad = []
    for name, x, f, w in rows:
        err, fl = _rel(x, w), _rel(f, w)
        print(f"  {name}: packed {err:.3e} floor {fl:.3e} ratio {err / fl if fl > 0 else math.inf:.2f}")
        if not err <= 3 * fl:
            bad.append((name, err, fl))
    assert not bad, bad


def test_non_consecutive_position_ids_are_reported_at_the_next_call(dev):
    model = _tiny(dev, torch.bfloat16)
    ids = torch.randint(1, 512, (1, 128), device=dev)
    good = (torch.arange(128, device=dev) % 64)[None]
    broken = good.clone()
    broken[0, 70] += 3
    with torch.no_grad():
        model(input_ids=ids, position_ids=broken)  # the lazy flag: nothing raised here
        torch.cuda.synchronize()
        with pytest.raises(ValueError, match="position_ids"):
            model(input_ids=ids, position_ids=good)
        out = model(input_ids=ids, position_ids=good)  # the flag was cleared with the report
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out.logits).all())
        with pytest.raises(ValueError):
            model(input_ids=ids, position_ids=good, attention_mask=torch.ones_like(ids))
