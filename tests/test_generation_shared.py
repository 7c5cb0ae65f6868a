"""CPU (fp32 tiny GPT-2 and tiny Llama with GQA): ``generate(..., num_return_sequences=R)`` — R
samples of every prompt over one shared prompt cache (``generation.SharedPrefixKVCache``) — gives
the tokens of the same call on ``ids.repeat_interleave(R, 0)``, holds the prompt once, and refuses
what it cannot do."""
import pytest
import torch

from nbdistributed_amd.generation import KVCache, SharedPrefixKVCache, generate
from nbdistributed_amd.models import GPT2, GPT2Config
from nbdistributed_amd.models.llama import LlamaConfig, LlamaForCausalLM

R, NEW, T0 = 3, 9, 12
LENS = (12, 7, 1, 10)
SEEDS = (0, 1, 2)


def _model(family):
    torch.manual_seed(0)
    return (GPT2(GPT2Config.tiny()) if family == "gpt2" else LlamaForCausalLM(LlamaConfig.tiny())).eval()


def _prompts():
    g = torch.Generator().manual_seed(3)
    return torch.randint(1, 512, (len(LENS), T0), generator=g), torch.tensor(LENS)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _unshared(m, ids, lens, seed, **kw):
    return generate(m, ids.repeat_interleave(R, 0), NEW, lengths=lens.repeat_interleave(R), temperature=1.0, top_k=8,
                    generator=_gen(seed), **kw)


def _shared(m, ids, lens, seed, **kw):
    return generate(m, ids, NEW, lengths=lens, temperature=1.0, top_k=8, generator=_gen(seed), num_return_sequences=R,
                    **kw)


@pytest.mark.parametrize("kv_dtype", [None, "fp8"], ids=["kv-model", "kv-fp8"])
@pytest.mark.parametrize("family", ["gpt2", "llama"])
def test_shared_samples_are_the_repeated_prompts_samples(family, kv_dtype):
    m = _model(family)
    ids, lens = _prompts()
    for seed in SEEDS:
        want = _unshared(m, ids, lens, seed, kv_dtype=kv_dtype)
        assert torch.equal(want, _unshared(m, ids, lens, seed, kv_dtype=kv_dtype)), "the unshared call is not reproducible"
        got = _shared(m, ids, lens, seed, kv_dtype=kv_dtype)
        assert got.shape == (len(LENS) * R, T0 + NEW)
        assert torch.equal(got, want), (family, seed)
        # rows of a prompt are different samples, laid out as today: prompt, new tokens from lengths[b], pad
        rows = got.view(len(LENS), R, -1)
        assert any(not torch.equal(rows[b, 0], rows[b, r]) for b in range(len(LENS)) for r in range(1, R))
        for b, n in enumerate(LENS):
            assert torch.equal(rows[b, :, :n], ids[b, :n].expand(R, n))
            assert (rows[b, :, n + NEW:] == 0).all()


@pytest.mark.parametrize("family", ["gpt2", "llama"])
def test_shared_samples_with_eos(family):
    m = _model(family)
    ids, lens = _prompts()
    free = _shared(m, ids, lens, SEEDS[0])
    n0 = LENS[0]
    eos = int(free[0, n0 + 2])  # a token that occurs: row 0 emits it as its third new token
    want = _unshared(m, ids, lens, SEEDS[0], eos_token_id=eos, pad_token_id=5)
    got = _shared(m, ids, lens, SEEDS[0], eos_token_id=eos, pad_token_id=5)
    assert torch.equal(got, want)
    assert (got[0, n0 + 2:n0 + NEW] == eos).all()  # a finished row keeps emitting eos


@pytest.mark.parametrize("kv_dtype", [None, "fp8"], ids=["kv-model", "kv-fp8"])
def test_shared_cache_holds_the_prompt_once(kv_dtype):
    m = _model("llama")
    ids, lens = _prompts()
    out, cache = _shared(m, ids, lens, SEEDS[0], kv_dtype=kv_dtype, return_cache=True)
    _, plain = _unshared(m, ids, lens, SEEDS[0], kv_dtype=kv_dtype, return_cache=True)
    assert isinstance(cache, SharedPrefixKVCache) and isinstance(plain, KVCache)
    L, H, Hkv, D = m.kv_layout()
    B, esize = len(LENS), (1 if kv_dtype else 4)
    assert cache.is_fp8 == bool(kv_dtype)
    assert (cache.t_prefix, cache.t_own, cache.t_max) == (T0, NEW, T0 + NEW)
    assert cache.nbytes == 2 * L * Hkv * D * esize * (B * T0 + B * R * NEW)
    assert plain.nbytes == 2 * L * Hkv * D * esize * B * R * (T0 + NEW)
    assert cache.nbytes < plain.nbytes
    # lengths / pending as KVCache keeps them: per sequence, the position and value of the last token
    assert torch.equal(cache.lengths, plain.lengths) and torch.equal(cache.pending, plain.pending)
    assert torch.equal(cache.plen, lens)
    # t_max= is a floor on prefix + own rows
    _, roomy = _shared(m, ids, lens, SEEDS[0], t_max=40, return_cache=True)
    assert (roomy.t_prefix, roomy.t_own, roomy.t_max) == (T0, 40 - T0, 40)


def test_shared_refusals():
    m = _model("gpt2")
    ids, lens = _prompts()
    with pytest.raises(ValueError, match="temperature > 0"):
        generate(m, ids, NEW, lengths=lens, num_return_sequences=R)  # greedy
    with pytest.raises(ValueError, match="num_return_sequences must be >= 1"):
        generate(m, ids, NEW, lengths=lens, num_return_sequences=0)
    _, plain = generate(m, ids, NEW, lengths=lens, t_max=64, return_cache=True)
    with pytest.raises(ValueError, match="cache="):
        generate(m, None, 2, cache=plain, temperature=1.0, num_return_sequences=R)
    _, shared = _shared(m, ids, lens, SEEDS[0], t_max=64, return_cache=True)
    with pytest.raises(NotImplementedError, match="shared prefix"):
        generate(m, None, 2, cache=shared)
    with pytest.raises(NotImplementedError, match="shared-prefix"):
        shared.extend(0, None, None, None)
    # the position limit and the sliding window count max_len + max_new_tokens, as without the argument
    generate(m, ids, 116, lengths=lens, temperature=1.0, num_return_sequences=2)  # 12 + 116 = GPT-2 tiny's 128
    with pytest.raises(ValueError, match="needs 129 positions"):
        generate(m, ids, 117, lengths=lens, temperature=1.0, num_return_sequences=2)
    w = LlamaForCausalLM(LlamaConfig.tiny(sliding_window=16)).eval()
    generate(w, ids, 4, lengths=lens, temperature=1.0, num_return_sequences=2)  # 16 positions: inside the window
    with pytest.raises(NotImplementedError, match="sliding window"):
        generate(w, ids, 5, lengths=lens, temperature=1.0, num_return_sequences=2)


@pytest.mark.parametrize("family", ["gpt2", "llama"])
def test_one_return_sequence_is_the_call_without_the_argument(family):
    m = _model(family)
    ids, lens = _prompts()
    for kw in (dict(), dict(temperature=1.0, top_k=8)):
        a, ca = generate(m, ids, NEW, lengths=lens, generator=_gen(4), return_cache=True, **kw)
        b, cb = generate(m, ids, NEW, lengths=lens, generator=_gen(4), return_cache=True, num_return_sequences=1, **kw)
        assert torch.equal(a, b) and type(cb) is KVCache
        assert torch.equal(ca.k, cb.k) and torch.equal(ca.v, cb.v)
