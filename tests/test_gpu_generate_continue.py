"""GPU multi-turn generation: ``generate(..., cache=cache)`` (block append over the returned cache,
csrc/kernels/append.hip, then the graph-captured decode loop) against one ``generate`` over the
concatenated history and against the full forward, bf16, for the three model families of
test_gpu_decode.py's generation test."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

from nbdistributed_amd import ops  # noqa: E402
from nbdistributed_amd.generation import generate  # noqa: E402

LENS1, NEW1 = (40, 33, 12, 1), 24
LENS2, NEW2 = (7, 1, 32, 20), 16
T_MAX = 160  # the first call prefills at 128 rows; 63 held + 1 + 32 + 16 after the second
GAIN = 8.0  # test_gpu_decode.py's _peaked gain


@pytest.fixture(scope="module", autouse=True)
def _gpu(require_gpu):
    ops.load_library()


def _peaked(model):
    # scale the embedding (tied LM head) so greedy tokens are far from ties under bf16 rounding
    with torch.no_grad():
        emb = model.wte.weight if hasattr(model, "wte") else model.model.embed_tokens.weight
        emb.mul_(GAIN)
    return model


def _model(family):
    from nbdistributed_amd.models import GPT2, GPT2Config
    from nbdistributed_amd.models.llama import LlamaConfig, LlamaForCausalLM

    torch.manual_seed(0)
    if family == "gpt2":
        m = GPT2(GPT2Config(vocab_size=512, n_positions=512, n_embd=256, n_layer=2, n_head=4))
    elif family == "qwen2":
        m = LlamaForCausalLM(LlamaConfig.tiny(qkv_bias=True))
        with torch.no_grad():
            for layer in m.model.layers:
                layer.self_attn.qkv_proj.bias.normal_(0, 0.5)
    else:
        m = LlamaForCausalLM(LlamaConfig.tiny())
    return _peaked(m.to("cuda", torch.bfloat16).eval())


@pytest.mark.parametrize("family", ["gpt2", "llama", "qwen2"])
def test_gpu_two_turns_match_single_shot_and_full_forward(family):
    m = _model(family)
    B = len(LENS1)
    g = torch.Generator(device="cuda").manual_seed(1)
    ids1 = torch.randint(1, 512, (B, max(LENS1)), device="cuda", generator=g)
    ids2 = torch.randint(1, 512, (B, max(LENS2)), device="cuda", generator=g)
    l1, l2 = torch.tensor(LENS1, device="cuda"), torch.tensor(LENS2, device="cuda")
    outs = {}
    for graph in (False, True):
        out1, cache = generate(m, ids1, NEW1, lengths=l1, t_max=T_MAX, graph=graph, return_cache=True)
        if not graph:  # the block's logits, on a copy of the cache state the turn starts from
            c2 = copy.copy(cache)
            c2.k, c2.v = cache.k.clone(), cache.v.clone()
            chunk = torch.cat([cache.pending.view(B, 1), ids2], 1)
            first = m.extend(chunk, c2, cache.lengths.clone(), l2 + 1).float()
        out2 = generate(m, ids2, NEW2, lengths=l2, cache=cache, graph=graph)
        outs[graph] = (out1, out2)
    assert torch.equal(outs[False][0], outs[True][0]) and torch.equal(outs[False][1], outs[True][1])
    out1, out2 = outs[True]
    assert out2.shape == (B, max(LENS2) + NEW2)
    hist = [out1[b, :LENS1[b] + NEW1].tolist() + ids2[b, :LENS2[b]].tolist() for b in range(B)]
    hl = torch.tensor([len(h) for h in hist], device="cuda")
    whole = torch.zeros(B, int(hl.max()), dtype=torch.long, device="cuda")
    for b, h in enumerate(hist):
        whole[b, :len(h)] = torch.tensor(h, device="cuda")
    ref = generate(m, whole, NEW2, lengths=hl, graph=True)  # the existing path: prefill of the whole history
    for b in range(B):
        n = LENS2[b]
        assert out2[b, :n].tolist() == ids2[b, :n].tolist()
        assert out2[b, n:n + NEW2].tolist() == ref[b, len(hist[b]):len(hist[b]) + NEW2].tolist(), (family, b)
        assert (out2[b, n + NEW2:] == 0).all()
        with torch.no_grad():
            x = torch.tensor([hist[b]], device="cuda")
            full = (m(x)[0] if family == "gpt2" else m(x)[1])[0, -1].float()
        d = (first[b] - full).abs().max().item()
        print(f"  {family} row {b}: first-logit max|Δ| {d:.4f} of max|full| {full.abs().max().item():.3f}")
        assert d < 0.05 * full.abs().max().item()
        assert int(first[b].argmax()) == int(full.argmax())
