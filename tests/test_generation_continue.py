"""Multi-turn generation on the CPU (fp32): ``generate(..., cache=cache)`` continues from the
cache an earlier call returned — only the new turn runs through the model
(``ops.append_attention``) — and must give what one ``generate`` over the concatenated history
gives, for tiny GPT-2 and tiny Llama (GQA), ragged prompts and ragged turns."""
import pytest
import torch

from nbdistributed_amd.generation import KVCache, generate
from nbdistributed_amd.models import GPT2, GPT2Config
from nbdistributed_amd.models.llama import LlamaConfig, LlamaForCausalLM

LENS1, NEW1 = (9, 4, 1), 5
LENS2, NEW2 = (3, 1, 6), 4
T_MAX = 40


def _model(which):
    torch.manual_seed(0)
    return (GPT2(GPT2Config.tiny()) if which == "gpt2" else LlamaForCausalLM(LlamaConfig.tiny())).eval()


def _logits(m, x):
    return m(x)[0] if isinstance(m, GPT2) else m(x)[1]


def _ragged(lens, seed):
    ids = torch.randint(1, 512, (len(lens), max(lens)), generator=torch.Generator().manual_seed(seed))
    return ids, torch.tensor(lens)


def _two_turns(m):
    ids1, l1 = _ragged(LENS1, 1)
    ids2, l2 = _ragged(LENS2, 2)
    out1, cache = generate(m, ids1, NEW1, lengths=l1, t_max=T_MAX, return_cache=True)
    hist = [out1[b, :LENS1[b] + NEW1].tolist() + ids2[b, :LENS2[b]].tolist() for b in range(3)]
    return ids2, l2, cache, hist


@pytest.mark.parametrize("which", ["gpt2", "llama"])
def test_two_turns_equal_one_generate_on_the_history(which):
    m = _model(which)
    ids2, l2, cache, hist = _two_turns(m)
    assert cache.lengths.tolist() == [n + NEW1 - 1 for n in LENS1]  # the last token is pending, not cached
    out2, same = generate(m, ids2, NEW2, lengths=l2, cache=cache, return_cache=True)
    assert same is cache and cache.kv_len_max is None
    assert out2.shape == (3, max(LENS2) + NEW2)
    hl = torch.tensor([len(h) for h in hist])
    whole = torch.zeros(3, int(hl.max()), dtype=torch.long)
    for b, h in enumerate(hist):
        whole[b, :len(h)] = torch.tensor(h)
    ref = generate(m, whole, NEW2, lengths=hl)  # the existing path: prefill of the whole history
    for b in range(3):
        n = LENS2[b]
        assert out2[b, :n].tolist() == ids2[b, :n].tolist()
        assert out2[b, n:n + NEW2].tolist() == ref[b, len(hist[b]):len(hist[b]) + NEW2].tolist(), b
        assert (out2[b, n + NEW2:] == 0).all()
    assert cache.lengths.tolist() == [len(h) + NEW2 - 1 for h in hist]
    assert cache.pending.tolist() == [int(out2[b, LENS2[b] + NEW2 - 1]) for b in range(3)]


@pytest.mark.parametrize("which", ["gpt2", "llama"])
def test_first_logits_of_the_turn_match_the_full_forward(which):
    m = _model(which)
    ids2, l2, cache, hist = _two_turns(m)
    chunk = torch.cat([cache.pending.view(3, 1), ids2], 1)
    with torch.no_grad():
        lg = m.extend(chunk, cache, cache.lengths.clone(), l2 + 1)
        for b in range(3):
            full = _logits(m, torch.tensor([hist[b]]))[0, -1]
            rel = float((lg[b] - full).abs().max() / full.abs().max())
            assert rel < 1e-4, (b, rel)


@pytest.mark.parametrize("which", ["gpt2", "llama"])
@pytest.mark.parametrize("empty", [None, 0])
def test_keep_generating_equals_one_longer_generate(which, empty):
    m = _model(which)
    ids1, l1 = _ragged(LENS1, 3)
    out1, cache = generate(m, ids1, NEW1, lengths=l1, t_max=T_MAX, return_cache=True)
    turn = None if empty is None else torch.zeros(3, 0, dtype=torch.long)
    more = generate(m, turn, NEW2, cache=cache)
    assert more.shape == (3, NEW2)
    ref = generate(m, ids1, NEW1 + NEW2, lengths=l1)
    for b in range(3):
        n = LENS1[b]
        assert out1[b, :n + NEW1].tolist() == ref[b, :n + NEW1].tolist()
        assert more[b].tolist() == ref[b, n + NEW1:n + NEW1 + NEW2].tolist(), b


def test_three_turns_on_one_cache():
    m = _model("llama")
    ids1, l1 = _ragged(LENS1, 4)
    out1, cache = generate(m, ids1, 2, lengths=l1, t_max=T_MAX, return_cache=True)
    seqs = [out1[b, :LENS1[b] + 2].tolist() for b in range(3)]
    for turn_seed in (5, 6):
        ids, l = _ragged(LENS2, turn_seed)
        out = generate(m, ids, 3, lengths=l, cache=cache)
        for b in range(3):
            seqs[b] += out[b, :LENS2[b] + 3].tolist()
    for b in range(3):  # every generated token is the full forward's greedy choice on what precedes it
        with torch.no_grad():
            lg = _logits(m, torch.tensor([seqs[b]]))[0]
        n = len(seqs[b])
        for t in (n - 3, n - 2, n - 1):
            assert int(lg[t - 1].argmax()) == seqs[b][t], (b, t)


def test_without_a_cache_nothing_changed():
    """``cache=None``: the parent's code path — prefill, then the decode loop — step by step here,
    against ``generate`` on a fixed seed, greedy and sampled."""
    from nbdistributed_amd.generation import sample

    for which in ("gpt2", "llama"):
        m = _model(which)
        ids, lens = _ragged(LENS1, 9)
        for kw in ({}, {"temperature": 0.8, "top_k": 20}):
            got = generate(m, ids, 6, lengths=lens, generator=torch.Generator().manual_seed(3), **kw)
            g = torch.Generator().manual_seed(3)
            samp = dict(temperature=kw.get("temperature", 0.0), top_k=kw.get("top_k"), top_p=None, generator=g)
            cache = KVCache.for_model(m, 3, max(LENS1) + 6)
            want = torch.zeros(3, max(LENS1) + 6, dtype=torch.long)
            want[:, :max(LENS1)] = ids.masked_fill(torch.arange(max(LENS1))[None] >= lens[:, None], 0)
            tok, pos = sample(m.prefill(ids, cache, lens), **samp), lens.clone()
            want.scatter_(1, pos.view(-1, 1), tok.view(-1, 1))
            for _ in range(5):
                tok = sample(m.decode_step(tok, pos, cache), **samp)
                pos = pos + 1
                want.scatter_(1, pos.view(-1, 1), tok.view(-1, 1))
            assert torch.equal(got, want), (which, kw)


# ------------------------------------------------------------------------------------ refusals
def _filled(m, t_max=T_MAX, new=NEW1):
    ids1, l1 = _ragged(LENS1, 1)
    return generate(m, ids1, new, lengths=l1, t_max=t_max, return_cache=True)[1]


def test_refuses_a_cache_nobody_filled():
    m = _model("gpt2")
    with pytest.raises(ValueError, match="lengths"):
        generate(m, torch.ones(3, 2, dtype=torch.long), 2, cache=KVCache.for_model(m, 3, T_MAX))


def test_refuses_batch_and_layout_mismatch():
    m = _model("gpt2")
    cache = _filled(m)
    with pytest.raises(ValueError, match=r"batch 3"):
        generate(m, torch.ones(2, 2, dtype=torch.long), 2, cache=cache)
    other = _model("llama")  # 4 query heads over 2 kv heads, the cache has 4 over 4
    with pytest.raises(ValueError, match=r"\(2, 4, 4, 16\).*\(2, 4, 2, 64\)"):
        generate(other, torch.ones(3, 2, dtype=torch.long), 2, cache=cache)


def test_refuses_too_little_room_and_names_t_max():
    m = _model("llama")
    cache = _filled(m, t_max=20)  # holds 9 + 5 - 1 = 13 rows
    generate(m, torch.ones(3, 2, dtype=torch.long), 2, cache=_filled(m, t_max=20))  # 13 + 1 + 2 + 2 = 18
    with pytest.raises(ValueError, match=r"needs 21 cache rows \(13 held \+ 1 pending \+ 2 new \+ 5 to generate\).*"
                                         r"t_max 20.*t_max= on the first call"):
        generate(m, torch.ones(3, 2, dtype=torch.long), 5, cache=cache)


def test_refuses_past_the_position_limit():
    torch.manual_seed(0)
    m = GPT2(GPT2Config(vocab_size=512, n_positions=24, n_embd=64, n_layer=2, n_head=4)).eval()
    ids1, l1 = _ragged(LENS1, 1)
    _, cache = generate(m, ids1, NEW1, lengths=l1, t_max=64, return_cache=True)
    generate(m, torch.ones(3, 2, dtype=torch.long), 8, cache=cache)  # 13 + 1 + 2 + 8 = 24
    with pytest.raises(ValueError, match=r"reaches 29 positions.*model limit 24"):
        generate(m, torch.ones(3, 2, dtype=torch.long), 3, cache=cache)  # 13 + 8 + 2 - 1 = 23 held now


def test_sliding_window_counts_total_positions():
    torch.manual_seed(0)
    m = LlamaForCausalLM(LlamaConfig.tiny(sliding_window=24)).eval()
    ids1, l1 = _ragged(LENS1, 1)
    _, cache = generate(m, ids1, NEW1, lengths=l1, t_max=64, return_cache=True)
    generate(m, torch.ones(3, 2, dtype=torch.long), 8, cache=cache)
    with pytest.raises(NotImplementedError, match="sliding window"):
        generate(m, torch.ones(3, 2, dtype=torch.long), 3, cache=cache)


def test_parallel_attention_classes_refuse():
    from nbdistributed_amd.parallel import context, tensor

    for cls in (tensor.TPCausalSelfAttention, tensor.TPLlamaAttention, context.CPCausalSelfAttention,
                context.CPLlamaAttention):
        with pytest.raises(NotImplementedError, match="continuing generation from a KV cache"):
            cls.extend(None)
