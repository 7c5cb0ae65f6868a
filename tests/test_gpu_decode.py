"""HIP decode attention (csrc/kernels/decode.hip) vs the fp32 PyTorch reference, and GPU
generation (KV cache + graph-captured decode loop) vs the full forward pass."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from nbdistributed_amd import ops  # noqa: E402
from nbdistributed_amd.ops.decode import partials_numel  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _gpu(require_gpu):
    ops.load_library()


def _case(B, H, Hkv, Tmax, pos, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    D = 64
    kc = torch.randn(B, Hkv, Tmax, D, device="cuda", generator=g).to(torch.bfloat16)
    vc = torch.randn(B, Hkv, Tmax, D, device="cuda", generator=g).to(torch.bfloat16)
    qkv = torch.randn(B, (H + 2 * Hkv) * D, device="cuda", generator=g).to(torch.bfloat16)
    return qkv, kc, vc, torch.tensor(pos, device="cuda", dtype=torch.int64)


def _ws(B, H, Hkv, Tmax):
    return torch.empty(partials_numel(B, H, Tmax), dtype=torch.float32, device="cuda")


def _check(B, H, Hkv, Tmax, pos, rope=False, kv_len_max=None, seed=0):
    qkv, kc, vc, p = _case(B, H, Hkv, Tmax, pos, seed)
    tabs = ops.rope_tables(Tmax, 64, 10000.0, "cuda") if rope else None
    kr, vr = kc.float(), vc.float()
    ref = ops.decode_attention_reference(qkv.float(), kr, vr, p, H, rope=tabs)
    ws = _ws(B, H, Hkv, Tmax)
    out = ops.decode_attention(qkv, kc, vc, p, H, rope=tabs, kv_len_max=kv_len_max, workspace=ws)
    assert out.shape == (B, H * 64) and out.dtype == torch.bfloat16
    err = (out.float() - ref).abs().max().item()
    assert err < 2e-2, err
    bi = torch.arange(B, device="cuda")
    torch.testing.assert_close(kc[bi, :, p].float(), kr[bi, :, p].to(torch.bfloat16).float(), atol=2e-2, rtol=1e-2)
    torch.testing.assert_close(vc[bi, :, p].float(), vr[bi, :, p].to(torch.bfloat16).float(), atol=0, rtol=0)
    return out


@pytest.mark.parametrize("H,Hkv", [(12, 12), (4, 2), (9, 3), (8, 2), (16, 2), (7, 1)])
@pytest.mark.parametrize("rope", [False, True])
def test_decode_attention_group_sizes(H, Hkv, rope):
    _check(3, H, Hkv, 300, [0, 129, 299], rope=rope)


@pytest.mark.parametrize("B,Tmax", [(1, 4096), (2, 1024), (64, 256), (8, 2000)])
def test_decode_attention_chunking(B, Tmax):
    # one sequence over a long cache: up to 64 key chunks merged by the last one; wide batch: 1 chunk
    pos = [(Tmax - 1 - 37 * b) % Tmax for b in range(B)]
    _check(B, 12, 4, Tmax, pos, rope=True, seed=B)


def test_decode_attention_host_key_bound_and_replays():
    # kv_len_max below Tmax (eager generation) and repeated launches on one workspace
    B, H, Hkv, Tmax = 4, 8, 8, 1024
    for it, bound in enumerate([1, 17, 200, 1024]):
        pos = [min(bound - 1, x) for x in (0, 5, 150, 1000)]
        _check(B, H, Hkv, Tmax, pos, kv_len_max=bound, seed=10 + it)


def test_decode_attention_graph_replay():
    B, H, Hkv, Tmax = 2, 6, 2, 512
    qkv, kc, vc, p = _case(B, H, Hkv, Tmax, [10, 300])
    ws = _ws(B, H, Hkv, Tmax)
    ops.decode_attention(qkv, kc, vc, p, H, workspace=ws)  # warm-up
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = ops.decode_attention(qkv, kc, vc, p, H, workspace=ws)
    for step in range(3):
        p.add_(1)
        kref, vref = kc.float(), vc.float()
        ref = ops.decode_attention_reference(qkv.float(), kref, vref, p, H)
        g.replay()
        assert (out.float() - ref).abs().max().item() < 2e-2


def _peaked(model):
    # scale the embedding (tied LM head) so greedy tokens are far from ties under bf16 rounding
    with torch.no_grad():
        emb = model.wte.weight if hasattr(model, "wte") else model.model.embed_tokens.weight
        emb.mul_(8.0)
    return model


@pytest.mark.parametrize("family", ["gpt2", "llama", "qwen2"])
def test_gpu_generate_graph_matches_eager_and_full_forward(family):
    from nbdistributed_amd.models import GPT2, GPT2Config
    from nbdistributed_amd.models.llama import LlamaConfig, LlamaForCausalLM

    torch.manual_seed(0)
    if family == "gpt2":
        m = GPT2(GPT2Config(vocab_size=512, n_positions=512, n_embd=256, n_layer=2, n_head=4))
    elif family == "qwen2":  # biased q|k|v through the prefill GEMM and the decode kernel's bias epilogue
        m = LlamaForCausalLM(LlamaConfig.tiny(qkv_bias=True))
        with torch.no_grad():
            for layer in m.model.layers:
                layer.self_attn.qkv_proj.bias.normal_(0, 0.5)
    else:
        m = LlamaForCausalLM(LlamaConfig.tiny())
    m = _peaked(m.to("cuda", torch.bfloat16).eval())
    ids = torch.randint(1, 512, (4, 40), device="cuda")
    lens = torch.tensor([40, 33, 12, 1], device="cuda")
    eager = m.generate(ids, 24, lengths=lens, graph=False)
    graphed = m.generate(ids, 24, lengths=lens, graph=True)
    assert torch.equal(eager, graphed)
    # decode-step logits vs the full forward over the generated prefix (fp32 tolerance on bf16)
    from nbdistributed_amd.generation import KVCache

    b = 0
    seq = eager[b:b + 1, :40 + 24]
    cache = KVCache.for_model(m, 1, 128)
    m.prefill(torch.nn.functional.pad(seq[:, :40], (0, 88)), cache, torch.tensor([40], device="cuda"))
    for t in range(40, 48):
        lg = m.decode_step(seq[:, t], torch.tensor([t], device="cuda"), cache).float()
        with torch.no_grad():
            full = (m(seq[:, :t + 1])[0] if family == "gpt2" else m(seq[:, :t + 1])[1])[0, -1].float()
        assert (lg[0] - full).abs().max().item() < 0.05 * full.abs().max().item()
        assert int(lg.argmax()) == int(full.argmax())


# ---------------------------------------------------------------- small-M fused linear (smallm.hip)
def _lin_case(M, K, N, norm, act, bias, res, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda *s, sc=1.0: (torch.randn(*s, device="cuda", generator=g) * sc).to(torch.bfloat16)  # noqa: E731
    x = r(M, K)
    w = r(2 * N if act == "swiglu" else N, K, sc=K ** -0.5)
    nrm = None
    if norm == "ln":
        nrm = ("ln", r(K, sc=0.5) + 1, r(K, sc=0.1), 1e-5)
    elif norm == "rms":
        nrm = ("rms", r(K, sc=0.5) + 1, 1e-6)
    b = r(N, sc=0.5) if bias else None
    rs = r(M, N) if res else None
    return x, w, b, nrm, rs


@pytest.mark.parametrize("M", [1, 5, 16, 17, 40, 64])
@pytest.mark.parametrize("norm,act,bias,res", [(None, "none", False, False), ("ln", "none", True, False),
                                               ("ln", "gelu", True, False), (None, "none", True, True),
                                               ("rms", "swiglu", False, False), ("rms", "none", False, True)])
def test_linear_small_matches_reference(M, norm, act, bias, res):
    for K, N in ((768, 2304), (576, 1536), (64, 48), (2048, 272)):
        x, w, b, nrm, rs = _lin_case(M, K, N, norm, act, bias, res, seed=M + K)
        # (a few M = 64 norm-prologue shapes exceed the kernel's LDS and take the op-by-op path)
        y = ops.linear_small(x, w, b, norm=nrm, act=act, residual=rs)
        ref = ops.linear_small_reference(x, w, b, norm=nrm, act=act, residual=rs).float()
        assert y.shape == (M, N)
        err = ((y.float() - ref).abs().max() / ref.abs().max().clamp_min(1e-3)).item()
        assert err < 2e-2, (K, N, err)


def test_linear_small_ragged_vocab_head():
    # LM-head shape: odd N (ragged last column tile), LayerNorm.  At M = 8 (>= LIBRARY_MIN_ROWS, N >=
    # LIBRARY_MIN_N) ``ops.linear_small`` runs the stand-alone norm kernel and the library GEMM, not
    # smallm.hip; at M = 3 it reaches the kernel: fused LayerNorm prologue, grid capped at 512
    # workgroups looping over 3142 tiles (tests/test_gpu_decode_paths.py checks that loop per tile)
    for M in (8, 3):
        x, w, _, nrm, _ = _lin_case(M, 768, 50257, "ln", "none", False, False, seed=3)
        y = ops.linear_small(x, w, norm=nrm)
        ref = ops.linear_small_reference(x, w, norm=nrm).float()
        assert ((y.float() - ref).abs().max() / ref.abs().max()).item() < 2e-2, M


@pytest.mark.parametrize("V,offset", [(50257, 0), (512, 0), (1001, 3)])
@pytest.mark.parametrize("with_eos", [False, True])
def test_greedy_advance_matches_torch(V, offset, with_eos):
    B, T = 5, 12
    g = torch.Generator(device="cuda").manual_seed(V)
    base = torch.randn(B, V + offset, device="cuda", generator=g).to(torch.bfloat16)
    logits = base[:, offset:]  # offset 3: rows not 16-B aligned (scalar path)
    logits[1, 7] = logits[1, 9] = 50.0  # tie: the first index wins, like torch.argmax
    tok = torch.zeros(B, dtype=torch.int64, device="cuda")
    pos = torch.tensor([0, 3, 5, 10, 11], device="cuda")
    out = torch.zeros(B, T, dtype=torch.int64, device="cuda")
    eos = int(logits[2].float().argmax()) if with_eos else -1
    done = torch.tensor([False, False, False, True, False], device="cuda") if with_eos else None
    want = logits.float().argmax(-1)
    want_done = None
    if with_eos:
        want = torch.where(done, torch.full_like(want, eos), want)
        want_done = done | (want == eos)
    want_pos = pos + 1
    want_out = out.clone()
    for b in range(B):
        if want_pos[b] < T:
            want_out[b, want_pos[b]] = want[b]
    torch.ops.nbd.greedy_advance(logits, tok, pos, out, done, eos)
    assert torch.equal(tok, want) and torch.equal(pos, want_pos) and torch.equal(out, want_out)
    assert int(tok[1]) == 7
    if with_eos:
        assert torch.equal(done, want_done)


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["gpt2", "llama"])
def test_gpu_graphed_sampling_two_new_tokens(family):
    """Graph capture warms up on the real buffers: with max_new_tokens=2 (one decode step) the
    warm-up must not advance past ``out`` (sampling path: temperature > 0)."""
    from nbdistributed_amd.models import GPT2, GPT2Config
    from nbdistributed_amd.models.llama import LlamaConfig, LlamaForCausalLM

    torch.manual_seed(0)
    m = (GPT2(GPT2Config(vocab_size=512, n_positions=256, n_embd=128, n_layer=2, n_head=2)) if family == "gpt2"
         else LlamaForCausalLM(LlamaConfig.tiny()))
    m = m.to("cuda", torch.bfloat16).eval()
    ids = torch.randint(1, 512, (3, 20), device="cuda")
    for n in (2, 3):
        out = m.generate(ids, n, temperature=0.8, top_k=20, graph=True)
        torch.cuda.synchronize()
        assert out.shape == (3, 20 + n) and torch.equal(out[:, :20], ids)
        assert bool(((out[:, 20:] >= 0) & (out[:, 20:] < 512)).all())
