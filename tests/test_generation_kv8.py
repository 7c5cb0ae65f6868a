"""``generate(kv_dtype="fp8")`` on the CPU (the PyTorch path, ``ops.decode_attention_reference``): an
fp8 (``float8_e4m3fn``, no scales) KV cache holds ``q8`` of the rows a bf16 cache would hold,
whether prefill or a decode step wrote them, and a decode step attends over the cache as stored."""
import pytest
import torch
import torch.nn.functional as F

import refmath_kv8 as r8
from nbdistributed_amd.generation import KVCache, generate
from nbdistributed_amd.models import GPT2, GPT2Config
from nbdistributed_amd.models.llama import LlamaConfig, LlamaForCausalLM


def _peaked(model):
    # scale the embedding (tied LM head) so greedy tokens are far from ties
    with torch.no_grad():
        emb = model.wte.weight if hasattr(model, "wte") else model.model.embed_tokens.weight
        emb.mul_(8.0)
    return model


def _model(family):
    torch.manual_seed(0)
    return _peaked((GPT2(GPT2Config.tiny()) if family == "gpt2" else LlamaForCausalLM(LlamaConfig.tiny())).eval())


def _logits(m, x):
    return m(x)[0] if isinstance(m, GPT2) else m(x)[1]


def _rt(x):
    return r8.q8(x).to(x.dtype)


def _hand_rolled(m, prompt, n, monkeypatch):
    """Greedy decoding by full forwards, no cache.  What ``generate`` computes with an fp8 cache: a
    prompt position attended the unquantised keys and values (the prefill attention is not fp8); a
    generated position attends ``q8`` of every key and value up to itself, its own included.  So
    in each layer's attention (k already rotated) the rows from the prompt's length on take k and
    v round-tripped through ``q8``."""
    sdpa = F.scaled_dot_product_attention
    L = len(prompt)

    def attn(q, k, v, **kw):
        plain, quant = sdpa(q, k, v, **kw), sdpa(q, _rt(k), _rt(v), **kw)
        rows = torch.arange(q.shape[-2])[:, None] < L
        return torch.where(rows, plain, quant)

    monkeypatch.setattr(F, "scaled_dot_product_attention", attn)
    seq = list(prompt)
    with torch.no_grad():
        for _ in range(n):
            seq.append(int(_logits(m, torch.tensor([seq]))[0, -1].argmax()))
    monkeypatch.setattr(F, "scaled_dot_product_attention", sdpa)
    return seq


@pytest.mark.parametrize("family", ["gpt2", "llama"])
def test_fp8_cache_generates_the_hand_rolled_tokens(family, monkeypatch):
    m = _model(family)
    ids = torch.randint(1, 512, (3, 10), generator=torch.Generator().manual_seed(1))
    lens = torch.tensor([10, 7, 4])
    out = m.generate(ids, 8, lengths=lens, kv_dtype="fp8")
    plain = m.generate(ids, 8, lengths=lens)
    assert out.shape == (3, 18)
    for b in range(3):
        n = int(lens[b])
        want = _hand_rolled(m, ids[b, :n].tolist(), 8, monkeypatch)
        assert out[b, :n + 8].tolist() == want, (family, b)
        assert (out[b, n + 8:] == 0).all()
    assert torch.equal(generate(m, ids, 8, lengths=lens, kv_dtype=torch.float8_e4m3fn), out)
    # the quantised cache is a different computation from the default one: the hand-rolled loop
    # above is not vacuous if the unquantised tokens differ somewhere (they need not: reported)
    print(f"\n{family}: fp8-cache tokens equal the default cache's: {torch.equal(out, plain)}")


@pytest.mark.parametrize("family", ["gpt2", "llama"])
def test_fp8_cache_properties_and_row_rule(family):
    m = _model(family)
    ids = torch.randint(1, 512, (2, 9), generator=torch.Generator().manual_seed(2))
    out, cache = m.generate(ids, 5, kv_dtype="fp8", return_cache=True)
    assert cache.k.dtype == cache.v.dtype == torch.float8_e4m3fn and cache.is_fp8
    c16 = KVCache.for_model(m, 2, cache.t_max, dtype=torch.bfloat16)
    assert 2 * cache.nbytes == c16.nbytes
    # prefilled rows: q8 of the bf16 cache's rows, bit for bit
    c8 = KVCache.for_model(m, 2, cache.t_max, dtype=torch.float8_e4m3fn)
    lens = torch.tensor([9, 9])
    m.prefill(ids, c16, lens)
    m.prefill(ids, c8, lens)
    for a16, a8 in ((c16.k, c8.k), (c16.v, c8.v)):
        assert a16[:, :, :, :9].float().abs().max() > 0
        assert torch.equal(r8.bits8(r8.q8(a16)), r8.bits8(a8))
        assert (r8.bits8(a8[:, :, :, 9:]) == 0).all()
    # and generate's own cache holds those rows at the prompt's positions
    assert torch.equal(r8.bits8(cache.k[:, :, :, :9]), r8.bits8(c8.k[:, :, :, :9]))
    assert torch.equal(r8.bits8(cache.v[:, :, :, :9]), r8.bits8(c8.v[:, :, :, :9]))
    # a decode step writes its row by the same rule: row 9 of the fp8 cache is q8 of what the same
    # step writes into a bf16 cache whose history is the fp8 cache's, dequantised
    c16.k.copy_(c8.k.to(torch.bfloat16))
    c16.v.copy_(c8.v.to(torch.bfloat16))
    tok, pos = out[:, 9], torch.full((2,), 9)
    m.decode_step(tok, pos, c8)
    m.decode_step(tok, pos, c16)
    # (layer 0: from there on the two tokens attended different copies of their own row)
    assert c16.k[0, :, :, 9].float().abs().max() > 0
    assert torch.equal(r8.bits8(r8.q8(c16.k[0, :, :, 9])), r8.bits8(c8.k[0, :, :, 9]))
    assert torch.equal(r8.bits8(r8.q8(c16.v[0, :, :, 9])), r8.bits8(c8.v[0, :, :, 9]))
    assert (r8.bits8(c8.k[1:, :, :, 9]) != 0).any()


def test_continuing_from_an_fp8_cache_is_refused():
    m = _model("llama")
    ids = torch.randint(1, 512, (2, 6), generator=torch.Generator().manual_seed(3))
    out, cache = m.generate(ids, 4, kv_dtype="fp8", return_cache=True, t_max=32)
    before = (cache.k.clone(), cache.v.clone(), cache.lengths.clone(), cache.pending.clone())
    with pytest.raises(NotImplementedError, match="fp8 cache"):
        m.generate(ids[:, :2], 3, cache=cache)
    with pytest.raises(NotImplementedError, match="fp8 cache"):
        m.generate(None, 3, cache=cache, kv_dtype="fp8")
    with pytest.raises(NotImplementedError, match="fp8 cache"):
        cache.extend(0, torch.zeros(2, 1, 1), cache.lengths, torch.ones(2, dtype=torch.int64))
    # refused before any work: nothing of the cache moved
    after = (cache.k, cache.v, cache.lengths, cache.pending)
    assert all(torch.equal(r8.bits8(a) if a.dtype == torch.float8_e4m3fn else a,
                           r8.bits8(b) if b.dtype == torch.float8_e4m3fn else b) for a, b in zip(after, before))
    # the default cache still continues
    _, c32 = m.generate(ids, 4, return_cache=True, t_max=32)
    assert m.generate(ids[:, :2], 3, cache=c32).shape == (2, 5)


@pytest.mark.parametrize("family", ["gpt2", "llama"])
def test_without_kv_dtype_everything_is_as_before(family):
    m = _model(family)
    ids = torch.randint(1, 512, (2, 7), generator=torch.Generator().manual_seed(4))
    out, cache = m.generate(ids, 5, return_cache=True)
    assert cache.k.dtype == next(m.parameters()).dtype == torch.float32 and not cache.is_fp8
    out2, cache2 = m.generate(ids, 5, return_cache=True, kv_dtype=None)
    assert torch.equal(out, out2) and torch.equal(cache.k, cache2.k) and torch.equal(cache.v, cache2.v)
    with torch.no_grad():  # the unquantised cache reproduces the cache-free forward, token for token
        seq = ids[0].tolist()
        for _ in range(5):
            seq.append(int(_logits(m, torch.tensor([seq]))[0, -1].argmax()))
    assert out[0].tolist() == seq
    with pytest.raises(ValueError, match="kv_dtype"):
        m.generate(ids, 2, kv_dtype="int8")
    with pytest.raises(ValueError, match="kv_dtype"):
        m.generate(ids, 2, kv_dtype=torch.float8_e5m2)
