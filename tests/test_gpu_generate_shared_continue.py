"""GPU (bf16 tiny GPT-2 and tiny Llama with GQA, bf16 and fp8 caches): a second turn from the
``SharedPrefixKVCache`` that ``generate(..., num_return_sequences=R, return_cache=True)`` returned.
Greedy, it gives exactly the tokens of the same continue from a ``KVCache`` materialised from the
shared one — both run the same MFMA body on the same values."""
import pytest
import torch

from nbdistributed_amd import ops
from nbdistributed_amd.generation import KVCache, SharedPrefixKVCache, generate
from nbdistributed_amd.models import GPT2, GPT2Config
from nbdistributed_amd.models.llama import LlamaConfig, LlamaForCausalLM

pytestmark = pytest.mark.gpu

R, NEW1, NEW2, T_MAX = 3, 8, 6, 192  # 128 padded prompt rows + 64 own rows: 7 held + 1 + 32 + 6 fit
LENS1 = (40, 33, 12, 1)
LENS2 = (7, 1, 32, 20, 0, 5, 32, 1, 16, 2, 9, 31)  # one next turn per sample, ragged


@pytest.fixture(scope="module")
def dev(require_gpu):
    assert ops.native_available(), ops._load_error
    return torch.device("cuda", 0)


def _materialised(shared: SharedPrefixKVCache) -> KVCache:
    """the B·R private caches a user would build: prompt rows copied in front of every sample's own rows"""
    c = KVCache(shared.n_layer, shared.batch, shared.n_head, shared.n_kv, shared.t_max, shared.head_dim,
                dtype=shared.k.dtype, device=shared.k.device)
    for s in range(shared.batch):
        p, pl = s // shared.group, int(shared.plen[s // shared.group])
        for full, pre, own in ((c.k, shared.k, shared.k_own), (c.v, shared.v, shared.v_own)):
            full[:, s, :, :pl] = pre[:, p, :, :pl]
            full[:, s, :, pl:pl + shared.t_own] = own[:, s]
    c.lengths, c.pending = shared.lengths.clone(), shared.pending.clone()
    return c


@pytest.mark.parametrize("kv_dtype", [None, "fp8"], ids=["kv-model", "kv-fp8"])
@pytest.mark.parametrize("family", ["gpt2", "llama"])
def test_second_turn_from_the_shared_cache(dev, family, kv_dtype):
    torch.manual_seed(0)
    m = GPT2(GPT2Config.tiny()) if family == "gpt2" else LlamaForCausalLM(LlamaConfig.tiny())
    m = m.to(dev, torch.bfloat16).eval()
    g = torch.Generator(device="cuda").manual_seed(1)
    ids1 = torch.randint(1, 512, (len(LENS1), max(LENS1)), device=dev, generator=g)
    ids2 = torch.randint(1, 512, (len(LENS2), max(LENS2)), device=dev, generator=g)
    l1, l2 = torch.tensor(LENS1, device=dev), torch.tensor(LENS2, device=dev)
    first = dict(lengths=l1, temperature=1.0, num_return_sequences=R, kv_dtype=kv_dtype, return_cache=True)
    _, shared = generate(m, ids1, NEW1, t_max=T_MAX, **first)
    assert isinstance(shared, SharedPrefixKVCache) and shared.batch == len(LENS2) and shared.t_own == T_MAX - 128
    plain = _materialised(shared)
    held, prefix = shared.lengths.clone(), (shared.k.clone(), shared.v.clone())
    got = generate(m, ids2, NEW2, lengths=l2, cache=shared)
    want = generate(m, ids2, NEW2, lengths=l2, cache=plain)
    assert got.shape == (len(LENS2), max(LENS2) + NEW2) and torch.equal(got, want)
    assert torch.equal(shared.lengths, held + l2 + NEW2) and torch.equal(shared.pending, plain.pending)
    assert torch.equal(shared.k.view(torch.uint8), prefix[0].view(torch.uint8))  # the prompts are read only
    assert torch.equal(shared.v.view(torch.uint8), prefix[1].view(torch.uint8))
    # own rows for the first call only: the turn does not fit, and the error says how to reserve them
    _, tight = generate(m, ids1, NEW1, **first)
    with pytest.raises(ValueError, match="t_max="):
        generate(m, ids2, NEW2, lengths=l2, cache=tight)
