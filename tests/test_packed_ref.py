"""CPU side of packed-sequence (document-masked) attention:

  * tests/refmath_packed.py — a deliberate copy of refmath's attention arithmetic with the document
    mask — is tied to the yardstick (bit-equal at kstart = 0; equal to per-document calls), and its
    mutants are shown to score >= 9 x floor on the layouts tests/test_gpu_attn_packed.py runs, the
    convention of tests/test_refmath_mutants.py;
  * ``ops.packed_bounds`` (torch path), ``data.pack_sequences``, the SDPA fallback of
    ``ops.attention_qkv(bounds=)`` and a tiny fp32 ``LlamaForCausalLM`` with ``position_ids``:
    a packed row computes what its documents compute one at a time.

Run with ``-s`` to print the scores."""
import pytest
import torch

import refmath as rm
import refmath_packed as rp
from nbdistributed_amd import data, ops
from nbdistributed_amd.models.llama import LlamaConfig, LlamaForCausalLM, LlamaForSequenceClassification

SCALE = 0.125
OUT = ("out", "lse", "dq", "dk", "dv")


def _scores(x, ref):
    return {n: (rm.max_abs(a, b) if n == "lse" else rm.tile_rel(a, b, 32)) for n, a, b in zip(OUT, x, ref)}


# ------------------------------------------------------------------ the copy against the yardstick
@pytest.mark.parametrize("emulate", [False, True], ids=["exact", "emulated"])
@pytest.mark.parametrize("use_rope", [False, True], ids=["plain", "rope"])
def test_trivial_bounds_are_refmath_bit_for_bit(use_rope, emulate):
    B, H, Hkv, T = 2, 4, 2, 256
    rope = rm.rope_tables_ref(T) if use_rope else None
    q, k, v = rm.attn_inputs(B, H, Hkv, T, seed=3)
    do = rm.attn_do(rm.attn_ref(q, k, v, None, True, SCALE, rope=rope)[0], seed=4)
    want = rm.attn_ref(q, k, v, do, True, SCALE, rope=rope, emulate=emulate, gsplit=True)
    got = rp.attn_ref_packed(q, k, v, do, SCALE, torch.zeros(B, T, dtype=torch.int64), rope=rope, emulate=emulate,
                             gsplit=True)
    for n, a, b in zip(OUT, got, want):
        assert torch.equal(a, b), (n, float((a - b).abs().max()))


@pytest.mark.parametrize("use_rope", [False, True], ids=["plain", "rope"])
def test_exact_mode_is_per_document_refmath(use_rope):
    """each document alone through refmath.attn_ref, with its slice of the rotary tables (the
    packed kernels rotate by the row index)."""
    T, rows = rp.LAYOUTS["six-docs"]
    B, H, Hkv = 1, 4, 2
    ks, _, _ = rp.bounds_of_lengths(rows, T)
    rope = rm.rope_tables_ref(T) if use_rope else None
    q, k, v = rm.attn_inputs(B, H, Hkv, T, seed=5)
    do = rm.attn_do(rp.attn_ref_packed(q, k, v, None, SCALE, ks, rope=rope)[0], seed=6)
    got = rp.attn_ref_packed(q, k, v, do, SCALE, ks, rope=rope)
    s = 0
    for n in rows[0]:
        e = s + n
        sub = None if rope is None else (rope[0][s:e], rope[1][s:e])
        want = rm.attn_ref(q[:, :, s:e], k[:, :, s:e], v[:, :, s:e], do[:, :, s:e], True, SCALE, rope=sub)
        for name, a, b in zip(OUT, got, want):
            a = a[:, :, s:e]
            assert float((a - b).abs().max()) <= 1e-12 * max(float(b.abs().max()), 1e-300), (name, s, e)
        s = e


# ---------------------------------------------------------------------------- mutants show
_LAYOUT_CASE = {}


def _layout_case(name):
    """GQA 4/2 with RoPE and the group split over workgroups, as the GPU test's B <= 2 cases."""
    if name not in _LAYOUT_CASE:
        T, rows = rp.LAYOUTS[name]
        B, H, Hkv = len(rows), 4, 2
        ks, _, _ = rp.bounds_of_lengths(rows, T)
        rope = rm.rope_tables_ref(T)
        q, k, v = rm.attn_inputs(B, H, Hkv, T, seed=T + 7 * B)
        do = rm.attn_do(rp.attn_ref_packed(q, k, v, None, SCALE, ks, rope=rope)[0], seed=T + 1)
        exact = rp.attn_ref_packed(q, k, v, do, SCALE, ks, rope=rope)
        emu = rp.attn_ref_packed(q, k, v, do, SCALE, ks, rope=rope, emulate=True, gsplit=True)
        _LAYOUT_CASE[name] = ((q, k, v, do, rope, ks), exact, _scores(emu, exact))
    return _LAYOUT_CASE[name]


@pytest.mark.parametrize("layout", list(rp.LAYOUTS))
def test_emulated_floor_is_finite_and_a_bf16_rounding(layout):
    """the emulation of the finite running-maximum floor leaves no NaN, also where a wave's later
    document sees nothing in tile 0 (80+176).  A few bf16 roundings (2^-8 each) per tile: below
    5e-2, so that 9 x floor stays well under a relative error of 1 — what a missing or an extra
    document amounts to — and the GPU test's 3 x floor means something."""
    _, exact, floor = _layout_case(layout)
    print(f"\n{layout} floor", {n: f"{x:.2e}" for n, x in floor.items()})
    for n in ("out", "dq", "dk", "dv"):
        assert 0 < floor[n] < 5e-2, (n, floor[n])
    assert floor["lse"] < 0.1


@pytest.mark.parametrize("mutant", rp.PACKED_MUTANTS)
@pytest.mark.parametrize("layout", list(rp.LAYOUTS))
def test_packed_mutant_is_caught(layout, mutant):
    """>= 9 x floor on at least one output, on every layout where the mutant is a different
    formula at all.  Whether it is one is computed from the visibility it produces, not listed:
    with a single document (kstart = 0) ``kstart_minus1`` and ``bounds_ignored_offdiag`` ARE the
    correct mask, and there the emulated mutant must equal the emulated reference exactly."""
    (q, k, v, do, rope, ks), exact, floor = _layout_case(layout)
    vis, vis0 = rp.visibility(ks, mutant), rp.visibility(ks, None)
    differs = not (torch.equal(vis[0], vis0[0]) and torch.equal(vis[1], vis0[1]))
    if layout != "one-doc":
        assert differs, (layout, mutant)  # every multi-document layout tells every mutant apart
    got = rp.attn_ref_packed(q, k, v, do, SCALE, ks, rope=rope, emulate=True, gsplit=True, mutant=mutant)
    score = _scores(got, exact)
    ratio = {n: score[n] / max(floor[n], 1e-300) for n in OUT}
    print(f"\n{layout:10s} {mutant:22s}", {n: f"{ratio[n]:.0f}x" for n in OUT})
    if differs:
        assert max(ratio.values()) >= 9, (layout, mutant, ratio)
    else:
        assert all(score[n] == floor[n] for n in OUT), (layout, mutant, score, floor)


# ------------------------------------------------------------------------------ packed_bounds (CPU)
def _loop_bounds(pos):
    B, T = pos.shape
    ks = torch.zeros(B, T, dtype=torch.int32)
    qe = torch.zeros(B, T, dtype=torch.int32)
    bad = 0
    for b in range(B):
        starts = [t for t in range(T) if t == 0 or int(pos[b, t]) == 0] + [T]
        for s, e in zip(starts[:-1], starts[1:]):
            ks[b, s:e] = s
            qe[b, s:e] = e
        for t in range(1, T):
            if int(pos[b, t]) != int(pos[b, t - 1]) + 1 and int(pos[b, t]) != 0:
                bad = 1
    return ks, qe, bad


@pytest.mark.parametrize("rows,T", [([[256]], 256), ([[1, 1, 1, 61]], 64), ([[33, 31, 64, 1, 127, 128]], 384),
                                    ([[80, 176], [200, 56]], 256), ([[5, 1, 1, 3]], 10), ([[1]], 1)])
def test_packed_bounds_cpu_matches_a_plain_loop(rows, T):
    ks0, qe0, pos = rp.bounds_of_lengths(rows, T)
    bad = torch.zeros(1, dtype=torch.int32)
    b = ops.packed_bounds(pos, bad)
    assert isinstance(b, ops.PackedBounds) and b.kstart.dtype == b.qend.dtype == torch.int32
    ks, qe, flag = _loop_bounds(pos)
    assert torch.equal(b.kstart, ks) and torch.equal(b.qend, qe) and int(bad) == flag == 0
    assert torch.equal(ks.long(), ks0) and torch.equal(qe.long(), qe0)
    assert bool((b.kstart[:, 1:] >= b.kstart[:, :-1]).all()) and bool((b.qend[:, 1:] >= b.qend[:, :-1]).all())


def test_packed_bounds_cpu_flags_a_non_consecutive_row():
    pos = torch.tensor([[0, 1, 2, 0, 1, 2, 3, 4], [0, 1, 2, 3, 5, 6, 0, 1]])
    bad = torch.zeros(1, dtype=torch.int32)
    b = ops.packed_bounds(pos, bad)
    ks, qe, flag = _loop_bounds(pos)
    assert flag == 1 and int(bad) == 1
    assert torch.equal(b.kstart, ks) and torch.equal(b.qend, qe)  # documents as the zeros delimit them
    # a row that does not begin at 0 still starts a document at t == 0, and is not flagged for that
    bad.zero_()
    b = ops.packed_bounds(torch.tensor([[3, 4, 5, 0, 1]]), bad)
    assert b.kstart.tolist() == [[0, 0, 0, 3, 3]] and b.qend.tolist() == [[3, 3, 3, 5, 5]] and int(bad) == 0


# ------------------------------------------------------------------------------- pack_sequences
def test_pack_sequences_first_fit_decreasing():
    g = torch.Generator().manual_seed(0)
    lens = [5, 12, 7, 16, 1, 3, 9, 2]
    seqs = [torch.randint(1, 500, (n,), generator=g) for n in lens]
    ids, pos, labels = data.pack_sequences(seqs, 16, pad_id=0)
    assert ids.shape == pos.shape == labels.shape and ids.shape[1] == 16 and ids.dtype == torch.int64
    assert ids.shape[0] == 4  # FFD: [16] [12, 3, 1] [9, 7] [5, 2]
    found = []
    for r in range(ids.shape[0]):
        starts = [t for t in range(16) if int(pos[r, t]) == 0] + [16]
        for s, e in zip(starts[:-1], starts[1:]):
            assert pos[r, s:e].tolist() == list(range(e - s))  # restart at 0, consecutive
            if bool((labels[r, s:e] == -100).all()):  # the padded tail: one more "document"
                assert e == 16 and bool((ids[r, s:e] == 0).all())
                continue
            assert torch.equal(labels[r, s:e], ids[r, s:e])
            found.append(ids[r, s:e])
    assert len(found) == len(seqs)  # every document once, unsplit
    for s in seqs:
        assert sum(torch.equal(s, f) for f in found) >= 1
    assert sorted(f.numel() for f in found) == sorted(lens)
    assert nbd_data_is_exposed()


def nbd_data_is_exposed():
    import nbdistributed_amd as nbd

    return nbd.data.pack_sequences is data.pack_sequences


def test_pack_sequences_refuses_to_split_or_overflow():
    with pytest.raises(ValueError):
        data.pack_sequences([[1] * 17], 16, pad_id=0)
    with pytest.raises(ValueError):
        data.pack_sequences([[1] * 10, [2] * 10], 16, pad_id=0, max_rows=1)
    ids, pos, labels = data.pack_sequences([[1] * 10, [2] * 6], 16, pad_id=0, max_rows=1)
    assert ids.shape == (1, 16) and pos[0].tolist() == list(range(10)) + list(range(6))


# ----------------------------------------------------------------------- the fallback and the model
def test_attention_qkv_bounds_cpu_fallback_is_per_document():
    torch.manual_seed(0)
    B, T, H, Hkv, D = 2, 48, 4, 2, 16
    rows = [[10, 1, 37], [48]]
    _, _, pos = rp.bounds_of_lengths(rows, T)
    bounds = ops.packed_bounds(pos)
    cos, sin = ops.rope_tables(T, D, 10000.0, "cpu")
    qkv = torch.randn(B, T, (H + 2 * Hkv) * D, requires_grad=True)
    dy = torch.randn(B, T, H * D)
    y = ops.attention_qkv(qkv, H, causal=True, n_kv_head=Hkv, rope=(cos, sin), bounds=bounds)
    y.backward(dy)
    for b, lens in enumerate(rows):
        s = 0
        for n in lens:
            sub = qkv.detach()[b:b + 1, s:s + n].clone().requires_grad_()
            ys = ops.attention_qkv(sub, H, causal=True, n_kv_head=Hkv, rope=(cos, sin))  # positions from 0
            ys.backward(dy[b:b + 1, s:s + n])
            assert torch.allclose(y[b:b + 1, s:s + n], ys, rtol=1e-5, atol=1e-5), (b, s)
            assert torch.allclose(qkv.grad[b:b + 1, s:s + n], sub.grad, rtol=1e-5, atol=1e-5), (b, s)
            s += n
    with pytest.raises(ValueError):
        ops.attention_qkv(qkv, H, causal=False, n_kv_head=Hkv, bounds=bounds)


def _tiny():
    torch.manual_seed(1)
    c = LlamaConfig(vocab_size=512, hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2,
                    num_key_value_heads=1, max_position_embeddings=256)
    return LlamaForCausalLM(c).float()


def _one_at_a_time(model, docs):
    """the documents run alone: per-token logits, the token-mean loss over all of them, gradients."""
    model.zero_grad()
    logits, total, count = [], 0.0, 0
    for d in docs:
        out = model(d[None], labels=d[None])
        logits.append(out.logits[0].detach())
        if d.numel() > 1:
            total = total + out.loss * (d.numel() - 1)
            count += d.numel() - 1
    loss = total / count
    loss.backward()
    grads = {n: p.grad.clone() for n, p in model.named_parameters()}
    return logits, loss.detach(), grads


def _check_packed(model, ids, pos, labels, docs_in_order, hooked=False):
    want_logits, want_loss, want_grads = _one_at_a_time(model, docs_in_order)
    model.zero_grad()
    h = model.model.layers[0].register_forward_hook(lambda *a: None) if hooked else None
    try:
        out = model(input_ids=ids, labels=labels, position_ids=pos)
    finally:
        if h is not None:
            h.remove()
    out.loss.backward()
    assert torch.allclose(out.loss, want_loss, rtol=1e-5, atol=1e-5), (float(out.loss), float(want_loss))
    flat = out.logits.reshape(-1, out.logits.shape[-1])
    real = torch.cat(want_logits)
    assert torch.allclose(flat[: real.shape[0]], real, rtol=1e-5, atol=1e-5)
    for n, p in model.named_parameters():
        assert torch.allclose(p.grad, want_grads[n], rtol=1e-5, atol=1e-5), n


@pytest.mark.parametrize("hooked", [False, True], ids=["ops", "modules"])
def test_tiny_llama_packed_row_equals_its_documents(hooked):
    model = _tiny()
    g = torch.Generator().manual_seed(2)
    docs = [torch.randint(1, 512, (n,), generator=g) for n in (13, 9, 5)]
    ids, pos, labels = data.pack_sequences(docs, 32, pad_id=0)  # one row: 13 + 9 + 5 and a tail of 5
    assert ids.shape == (1, 32)
    _check_packed(model, ids, pos, labels, docs, hooked)


def test_tiny_llama_takes_the_flattening_collator():
    tr = pytest.importorskip("transformers")
    coll = getattr(tr, "DataCollatorWithFlattening", None)
    if coll is None:
        pytest.skip("the installed transformers has no DataCollatorWithFlattening")
    g = torch.Generator().manual_seed(3)
    docs = [torch.randint(1, 512, (n,), generator=g) for n in (7, 4, 11)]
    batch = coll()([{"input_ids": d.tolist()} for d in docs], return_tensors="pt")
    if "position_ids" not in batch:
        pytest.skip("the installed DataCollatorWithFlattening does not emit position_ids")
    assert batch["position_ids"].tolist() == [list(range(7)) + list(range(4)) + list(range(11))]
    _check_packed(_tiny(), batch["input_ids"], batch["position_ids"], batch["labels"], docs)


def test_position_ids_exclusions():
    model = _tiny()
    ids = torch.randint(1, 512, (1, 16))
    pos = torch.arange(16)[None] % 8
    with pytest.raises(ValueError):
        model(input_ids=ids, position_ids=pos, attention_mask=torch.ones_like(ids))
    with pytest.raises(ValueError):
        model.model(ids, position_ids=pos, attention_mask=torch.ones_like(ids))
    with pytest.raises(ValueError):  # not consecutive inside a document (the CPU check is immediate)
        model(input_ids=ids, position_ids=pos * 2)
    # the classes that do not take position_ids keep rejecting it
    cls = LlamaForSequenceClassification(model.config)
    with pytest.raises(TypeError):
        cls(input_ids=ids, position_ids=pos)
    assert cls(input_ids=ids, position_ids=None).logits.shape == (1, 2)
