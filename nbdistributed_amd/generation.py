"""Autoregressive generation with a KV cache for the framework's causal LMs (GPT-2, Llama).

The reference's notebooks train; after training, a user of an interactive notebook wants to
*sample* from the model in the next cell.  ``generate`` does that MI355X-first:

* **prefill** — one pass over the (right-padded) prompts through the model's training kernels
  (HIP flash attention, fused GEMMs), storing each layer's k (rotated) and v into a
  ``KVCache`` laid out [layer, batch, kv-head, position, head dim] so a decode step streams one
  contiguous run of rows per head;
* **decode** — one token per sequence per step: GEMMs on hipBLASLt (M = batch rows), and one HIP
  kernel per layer for RoPE + cache append + split-key attention with its merge
  (``ops.decode_attention``, ``csrc/kernels/decode.hip``: head dim 64 or 128, bf16 or fp8 cache);
* the positions live on the device, so the whole decode step — sampling included (Gumbel-max on
  the device RNG) — is captured once into a HIP graph and replayed per token: no host launch
  cost and no host sync per token (sequences that reach ``eos_token_id`` keep emitting it; the
  host checks for all-finished every ``sync_every`` tokens);
* **continue** — ``generate(..., return_cache=True)`` hands back the cache with each sequence's
  valid rows (``lengths``) and its last emitted token (``pending``: sampled, not yet in the
  cache); ``generate(turn, n, cache=cache)`` runs only ``[pending, turn…]`` through the stack,
  with ``ops.append_attention`` (``csrc/kernels/append.hip``) attending the block over the cache
  at per-sequence offsets and appending it, then enters the same decode loop — no second prefill
  of the history;
* **several samples per prompt** — ``generate(..., num_return_sequences=R)`` prefills the B
  prompts once into a ``SharedPrefixKVCache`` (each prompt held once, R short tails of own rows)
  and decodes B·R sequences with ``ops.decode_attention_shared``: the same decode kernel, a key's
  address taken from the prompt's prefix or the sample's own rows.

Models opt in by providing ``kv_layout()``, ``prefill(ids, cache, lengths)``,
``decode_step(tok, pos, cache)`` and ``extend(ids, cache, start, nnew)``; see ``models/gpt2.py``
and ``models/llama.py``.
"""
from __future__ import annotations

import math
from typing import Optional

import torch


def _kv_dtype(kv_dtype):
    """``generate``'s ``kv_dtype``: None (the model's dtype), "fp8" or ``torch.float8_e4m3fn``."""
    if kv_dtype is None or kv_dtype == torch.float8_e4m3fn:
        return kv_dtype
    if isinstance(kv_dtype, str) and kv_dtype.lower() == "fp8":
        return torch.float8_e4m3fn
    raise ValueError(f"generate: kv_dtype must be None, 'fp8' or torch.float8_e4m3fn, got {kv_dtype!r}")


class KVCache:
    """k / v caches [n_layer, B, Hkv, t_max, D] plus the decode kernel's workspace (D + 1 floats per
    sequence, head and key chunk).  ``attend`` (decode) and ``extend`` (continue) run their HIP kernels at D = 64
    and 128; the prefill attention has its kernel at 64 only and runs the PyTorch math at 128.

    ``dtype=torch.float8_e4m3fn``: rows are stored as ``ops.decode.q8`` makes them (clamped to
    ±448, round to nearest even, no scales) by ``store`` and by ``attend`` alike: half the bytes
    held and half the bytes a decode step streams.  ``extend`` (continue) takes no fp8 cache."""

    def __init__(self, n_layer: int, batch: int, n_head: int, n_kv: int, t_max: int, head_dim: int,
                 dtype=torch.bfloat16, device="cuda"):
        self.n_layer, self.batch, self.n_head, self.n_kv, self.t_max, self.head_dim = (
            n_layer, batch, n_head, n_kv, t_max, head_dim)
        shape = (n_layer, batch, n_kv, t_max, head_dim)
        self.k = torch.zeros(shape, dtype=dtype, device=device)
        self.v = torch.zeros(shape, dtype=dtype, device=device)
        from .ops.decode import partials_numel

        self.workspace = torch.empty(partials_numel(batch, n_head, t_max, head_dim), dtype=torch.float32, device=device)
        self.kv_len_max: Optional[int] = None  # host bound on max(pos) + 1 (None = t_max)
        # set by every ``generate`` call (None on a fresh cache), both int64 [B] on the device:
        self.lengths: Optional[torch.Tensor] = None  # valid rows per sequence
        self.pending: Optional[torch.Tensor] = None  # the last emitted token, not yet in the cache

    @classmethod
    def for_model(cls, model, batch: int, t_max: int, device=None, dtype=None) -> "KVCache":
        L, H, Hkv, D = model.kv_layout()
        p = next(model.parameters())
        return cls(L, batch, H, Hkv, t_max, D, dtype=dtype or p.dtype, device=device or p.device)

    @property
    def nbytes(self) -> int:
        return 2 * self.k.numel() * self.k.element_size()

    @property
    def is_fp8(self) -> bool:
        return self.k.dtype == torch.float8_e4m3fn

    def store(self, layer: int, qkv: torch.Tensor, rope=None) -> None:
        """Prefill: copy k (rotated by ``rope`` = (cos, sin)) and v of a packed [B, T, W]
        projection into positions [0, T) of ``layer``."""
        from . import ops

        B, T, _ = qkv.shape
        H, Hkv, D = self.n_head, self.n_kv, self.head_dim
        if T > self.t_max:
            raise ValueError(f"KVCache.store: {T} positions > t_max {self.t_max}")
        k = qkv[:, :, H * D:(H + Hkv) * D]
        if rope is not None:
            k = ops.rope_(k.contiguous(), rope[0], rope[1], Hkv, D)
        v = qkv[:, :, (H + Hkv) * D:]
        if self.is_fp8:  # once per prompt: a clamp and a cast (the decode kernel quantises its own row)
            from .ops.decode import q8

            k, v = q8(k), q8(v)
        self.k[layer, :, :, :T] = k.reshape(B, T, Hkv, D).transpose(1, 2)
        self.v[layer, :, :, :T] = v.reshape(B, T, Hkv, D).transpose(1, 2)

    def attend(self, layer: int, qkv: torch.Tensor, pos: torch.Tensor, rope=None, scale=None) -> torch.Tensor:
        """Decode: append the new tokens of ``qkv`` [B, W] at ``pos`` and attend (``ops.decode_attention``)."""
        from . import ops

        return ops.decode_attention(qkv, self.k[layer], self.v[layer], pos, self.n_head, scale=scale, rope=rope,
                                    kv_len_max=self.kv_len_max, workspace=self.workspace)

    def extend(self, layer: int, qkv: torch.Tensor, start: torch.Tensor, nnew: torch.Tensor, rope=None,
               scale=None) -> torch.Tensor:
        """Continue: append the ``nnew[b]`` real rows of ``qkv`` [B, Tn, W] at ``start[b]`` and attend
        each over the cache up to itself (``ops.append_attention``)."""
        from . import ops

        if self.is_fp8:
            raise NotImplementedError("KVCache.extend: continuing from an fp8 cache is not implemented "
                                      "(the block-append kernel reads bf16 caches only)")
        return ops.append_attention(qkv, self.k[layer], self.v[layer], start, nnew, self.n_head, scale=scale,
                                    rope=rope, kv_len_max=self.kv_len_max)


class SharedPrefixKVCache:
    """The cache of ``generate(..., num_return_sequences=R)``: ``prompts`` prompts held once, in
    prefix tensors ``k`` / ``v`` [n_layer, prompts, Hkv, t_prefix, D], and ``group`` = R samples of
    each with their own rows ``k_own`` / ``v_own`` [n_layer, prompts·group, Hkv, t_own, D].
    Sequence s (a sample) belongs to prompt s // group; its position j is prefix row j below
    ``plen[s // group]`` (the prompt's length, int64 [prompts] on the device) and own row
    j - plen from there on.  The surface the models use is ``KVCache``'s: ``t_max`` (the absolute
    capacity t_prefix + t_own: RoPE tables are sized from it), ``store`` (prefill, into the prefix)
    and ``attend`` (decode, ``ops.decode_attention_shared``).  It cannot be continued."""

    def __init__(self, n_layer: int, prompts: int, group: int, n_head: int, n_kv: int, t_prefix: int, t_own: int,
                 head_dim: int, dtype=torch.bfloat16, device="cuda"):
        if group < 1 or t_own < 1:
            raise ValueError(f"SharedPrefixKVCache: need group >= 1 and t_own >= 1, got {group}, {t_own}")
        self.n_layer, self.prompts, self.group, self.n_head, self.n_kv, self.head_dim = (
            n_layer, prompts, group, n_head, n_kv, head_dim)
        self.batch = prompts * group  # sequences, as the decode loop counts them
        self.t_prefix, self.t_own, self.t_max = t_prefix, t_own, t_prefix + t_own
        self.k = torch.zeros((n_layer, prompts, n_kv, t_prefix, head_dim), dtype=dtype, device=device)
        self.v = torch.zeros_like(self.k)
        self.k_own = torch.zeros((n_layer, self.batch, n_kv, t_own, head_dim), dtype=dtype, device=device)
        self.v_own = torch.zeros_like(self.k_own)
        self.plen = torch.zeros(prompts, dtype=torch.int64, device=device)  # valid prefix rows per prompt
        from .ops.decode import partials_numel

        self.workspace = torch.empty(partials_numel(self.batch, n_head, self.t_max, head_dim), dtype=torch.float32,
                                     device=device)
        self.kv_len_max: Optional[int] = None  # host bound on max(pos) + 1 (None = t_max)
        self.lengths: Optional[torch.Tensor] = None  # int64 [prompts·group]: valid positions per sequence
        self.pending: Optional[torch.Tensor] = None  # the last emitted token of each, not yet in the cache

    @classmethod
    def for_model(cls, model, prompts: int, group: int, t_prefix: int, t_own: int, device=None,
                  dtype=None) -> "SharedPrefixKVCache":
        L, H, Hkv, D = model.kv_layout()
        p = next(model.parameters())
        return cls(L, prompts, group, H, Hkv, t_prefix, t_own, D, dtype=dtype or p.dtype, device=device or p.device)

    @property
    def nbytes(self) -> int:
        return 2 * (self.k.numel() + self.k_own.numel()) * self.k.element_size()

    @property
    def is_fp8(self) -> bool:
        return self.k.dtype == torch.float8_e4m3fn

    def store(self, layer: int, qkv: torch.Tensor, rope=None) -> None:
        """Prefill: k (rotated by ``rope``) and v of the prompts' packed [prompts, T, W] projection
        into prefix rows [0, T) of ``layer`` (``KVCache.store``'s rule, fp8 included)."""
        if qkv.shape[0] != self.prompts or qkv.shape[1] > self.t_prefix:
            raise ValueError(f"SharedPrefixKVCache.store: a [{qkv.shape[0]}, {qkv.shape[1]}, ...] projection does "
                             f"not fit {self.prompts} prefixes of {self.t_prefix} rows")
        KVCache.store(self, layer, qkv, rope)

    def attend(self, layer: int, qkv: torch.Tensor, pos: torch.Tensor, rope=None, scale=None) -> torch.Tensor:
        """Decode: append the new tokens of ``qkv`` [prompts·group, W] at absolute positions ``pos``
        to their own rows and attend over prefix + own (``ops.decode_attention_shared``)."""
        from . import ops

        return ops.decode_attention_shared(qkv, self.k[layer], self.v[layer], self.plen, self.k_own[layer],
                                           self.v_own[layer], pos, self.group, self.n_head, scale=scale, rope=rope,
                                           kv_len_max=self.kv_len_max, workspace=self.workspace)

    def extend(self, *args, **kwargs):
        raise NotImplementedError("SharedPrefixKVCache.extend: continuing from a shared-prefix cache is not "
                                  "implemented (the block-append kernel reads one cache per sequence)")


def sample(logits: torch.Tensor, temperature: float = 0.0, top_k: Optional[int] = None,
           top_p: Optional[float] = None, generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """Next tokens [B] from logits [B, V]: greedy at ``temperature`` 0, else a softmax sample
    (restricted to the ``top_k`` best and/or the ``top_p`` nucleus) by the Gumbel-max trick —
    device-only ops, so it captures into a graph."""
    if temperature <= 0.0:
        return logits.argmax(-1)
    x = logits.float() / temperature
    idx = None
    if top_k is not None and 0 < top_k < x.shape[-1]:
        x, idx = torch.topk(x, top_k, dim=-1)
    if top_p is not None and 0.0 < top_p < 1.0:
        xs, order = torch.sort(x, dim=-1, descending=True)
        cum = torch.softmax(xs, -1).cumsum(-1)
        drop = (cum - torch.softmax(xs, -1)) >= top_p  # keep the smallest prefix reaching top_p
        xs = xs.masked_fill(drop, float("-inf"))
        x = torch.empty_like(x).scatter_(-1, order, xs)
    u = torch.rand(x.shape, device=x.device, generator=generator).clamp_(1e-20, 1.0)
    choice = (x - torch.log(-torch.log(u))).argmax(-1)
    return choice if idx is None else idx.gather(-1, choice[:, None]).squeeze(-1)


class _DecodeLoop:
    """One decode step (model step + sampling + bookkeeping) on static buffers; eager or graphed."""

    def __init__(self, model, cache, tok, pos, out, done, eos: Optional[int], sampling: dict):
        self.model, self.cache = model, cache
        self.tok, self.pos, self.out, self.done, self.eos = tok, pos, out, done, eos
        self.sampling = sampling
        self.graph = None

    def step(self):
        logits = self.model.decode_step(self.tok, self.pos, self.cache)
        if (self.sampling["temperature"] <= 0.0 and logits.is_cuda and logits.dtype == torch.bfloat16
                and logits.stride(-1) == 1 and self.out.dtype == torch.int64):
            # greedy: arg-max, eos bookkeeping, position and output update in one HIP kernel
            from .ops._lib import _require

            _require()
            torch.ops.nbd.greedy_advance(logits, self.tok, self.pos, self.out,
                                         self.done if self.eos is not None else None,
                                         -1 if self.eos is None else int(self.eos))
            return
        nxt = sample(logits, **self.sampling)
        if self.eos is not None:
            nxt = torch.where(self.done, torch.full_like(nxt, self.eos), nxt)
            self.done |= nxt == self.eos
        self.tok.copy_(nxt)
        self.pos += 1
        self.out.scatter_(1, self.pos.view(-1, 1), nxt.view(-1, 1))

    def capture(self, warmup: int = 2):
        """Warm up ``warmup`` real steps on a side stream, restore the state, capture one step.
        The caller bounds ``warmup`` by the number of decode steps it will run, so the warm-up's
        position advances stay inside ``out`` and the cache (every step scatters at pos + 1)."""
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        saved = [t.clone() for t in (self.tok, self.pos, self.out, self.done)]
        with torch.cuda.stream(side):
            for _ in range(warmup):
                self.step()
        torch.cuda.current_stream().wait_stream(side)
        for t, s in zip((self.tok, self.pos, self.out, self.done), saved):
            t.copy_(s)
        self.graph = torch.cuda.CUDAGraph()
        # thread_local: tensor-parallel decode steps hold RCCL all-reduces, and ProcessGroupNCCL's
        # watchdog thread keeps querying its events during capture
        from .graphs import _capture

        _capture(self.graph, self.step)  # (a failed capture leaves the stream and RNG usable)
        # capture does not execute: the state is still the pre-capture one

    def __call__(self):
        if self.graph is not None:
            self.graph.replay()
        else:
            self.step()


def _run_decode(loop: _DecodeLoop, n: int, graph: bool, key_bound: int, eos_token_id, sync_every: int) -> None:
    """``n`` decode steps of ``loop`` (graph-captured first when ``graph``); ``key_bound`` = host
    bound on max(pos) + 1 at the first step.  Leaves ``cache.lengths`` / ``cache.pending`` set."""
    cache = loop.cache
    if graph and n > 0:
        loop.capture(warmup=min(2, n))
    try:
        for i in range(n):
            if not graph:
                cache.kv_len_max = key_bound + i  # known on the host: fewer idle workgroups
            loop()
            if eos_token_id is not None and (i + 1) % sync_every == 0 and bool(loop.done.all()):
                break
    finally:
        cache.kv_len_max = None  # the bound only held inside this call (a returned cache is reused later)
    # what a later ``generate(..., cache=cache)`` continues from: rows [0, pos) are in the cache,
    # ``tok`` (at position pos) is not — also after an early all-eos break
    cache.lengths, cache.pending = loop.pos.clone(), loop.tok.clone()


def _continue(model, input_ids, max_new_tokens: int, cache: KVCache, lengths, sampling: dict, eos_token_id,
              pad_token_id: int, graph, sync_every: int):
    """``generate`` from a returned cache: the block ``[cache.pending, turn…]`` per sequence goes
    through ``model.extend`` at ``start = cache.lengths``, then the decode loop takes over."""
    if cache.is_fp8:
        # the block-append kernel reads bf16 caches only: refuse before any work
        raise NotImplementedError("generate: continuing from an fp8 cache (kv_dtype='fp8') is not implemented; "
                                  "generate the first turn with the default kv_dtype to continue from its cache")
    if max_new_tokens <= 0:
        raise ValueError(f"generate: continuing from a cache needs max_new_tokens >= 1, got {max_new_tokens}")
    if cache.lengths is None or cache.pending is None:
        raise ValueError("generate: this cache has no lengths (a fresh KVCache): only a cache returned by "
                         "generate(..., return_cache=True) can be continued")
    device = cache.k.device
    B = cache.batch
    if input_ids is None:
        input_ids = torch.zeros((B, 0), dtype=torch.int64, device=device)
    input_ids = input_ids.to(device)
    if input_ids.dim() != 2 or input_ids.shape[0] != B:
        raise ValueError(f"generate: input_ids {tuple(input_ids.shape)} do not match the cache's batch {B}")
    layout = tuple(model.kv_layout())
    have = (cache.n_layer, cache.n_head, cache.n_kv, cache.head_dim)
    if layout != have:
        raise ValueError(f"generate: the cache's layout (layers, heads, kv heads, head dim) {have} is not the "
                         f"model's {layout}")
    Tn = input_ids.shape[1]
    lens = (torch.full((B,), Tn, dtype=torch.int64, device=device) if lengths is None
            else lengths.to(device=device, dtype=torch.int64))
    hist = int(cache.lengths.max())  # the one host sync, before any decoding
    total = hist + 1 + Tn + max_new_tokens  # positions in use after this call (the pending token is one)
    if total > cache.t_max:
        raise ValueError(f"generate: continuing needs {total} cache rows ({hist} held + 1 pending + {Tn} new + "
                         f"{max_new_tokens} to generate), the cache has t_max {cache.t_max}: reserve room with "
                         f"t_max= on the first call")
    limit = model.max_positions()
    if limit is not None and total > limit:
        raise ValueError(f"generate: continuing reaches {total} positions ({hist} held + 1 pending + {Tn} new + "
                         f"{max_new_tokens} to generate), model limit {limit}")
    window = getattr(getattr(model, "config", None), "sliding_window", None)
    if window is not None and total > window:
        raise NotImplementedError(f"generate: {total} positions exceed the model's sliding window ({window}); "
                                  f"sliding-window decoding is not implemented")
    start = cache.lengths.clone()
    nnew = lens + 1
    ar = torch.arange(Tn, device=device)
    turn = input_ids.masked_fill(ar[None, :] >= lens[:, None], pad_token_id)
    chunk = torch.cat([cache.pending.view(B, 1).to(turn.dtype), turn], 1)
    if device.type == "cuda":
        # B·(Tn + 1) rows onto the GEMM kernels' 64-row grid once, here (padding columns, nnew
        # unchanged), instead of a pad and a slice around every GEMM of every layer
        g = 64 // math.gcd(B, 64)
        extra = (-chunk.shape[1]) % g
        if extra:
            chunk = torch.cat([chunk, chunk.new_full((B, extra), pad_token_id)], 1)
    cache.kv_len_max = hist + 1 + Tn  # host bound on max(start + nnew)
    try:
        logits = model.extend(chunk, cache, start, nnew)
    finally:
        cache.kv_len_max = None
    tok = sample(logits, **sampling)
    pos = start + nnew  # position of `tok`
    # the decode loop writes a token at column pos of its output: run it on absolute positions, then
    # read each row back relative to its turn (column j = position start + 1 + j)
    out_abs = torch.full((B, total), pad_token_id, dtype=turn.dtype, device=device)
    out_abs.scatter_(1, pos.view(-1, 1), tok.view(-1, 1))
    done = (tok == eos_token_id) if eos_token_id is not None else torch.zeros(B, dtype=torch.bool, device=device)
    if graph is None:
        graph = device.type == "cuda" and sampling["generator"] is None
    loop = _DecodeLoop(model, cache, tok, pos, out_abs, done, eos_token_id, sampling)
    _run_decode(loop, max_new_tokens - 1, graph, hist + 1 + Tn + 1, eos_token_id, sync_every)
    rel = torch.arange(Tn + max_new_tokens, device=device)
    out = out_abs.gather(1, (start.view(-1, 1) + 1 + rel[None, :]).clamp_(max=total - 1))
    out[:, :Tn] = torch.where(ar[None, :] < lens[:, None], turn, out[:, :Tn])
    return out


def _generate_shared(model, input_ids, max_new_tokens: int, R: int, lengths, sampling: dict, eos_token_id,
                     pad_token_id: int, graph, t_max, sync_every: int, kv_dtype):
    """``generate`` with ``num_return_sequences`` = R > 1: one prefill of the B prompts into the prefix
    of a ``SharedPrefixKVCache``, then the decode loop over B·R sequences.  Returns (out, cache)."""
    device = input_ids.device
    B, T0 = input_ids.shape
    if max_new_tokens <= 0:
        return input_ids.repeat_interleave(R, 0), None
    lens = (torch.full((B,), T0, dtype=torch.int64, device=device) if lengths is None
            else lengths.to(device=device, dtype=torch.int64))
    max_len = int(lens.max())  # one host sync, before any decoding
    if int(lens.min()) < 1:
        raise ValueError("generate: every prompt needs at least one token")
    t_pad = model.prefill_length(T0)
    need = max(t_pad, max_len + max_new_tokens)
    t_max = t_max or need
    limit = model.max_positions()
    if t_max < need or (limit is not None and need > limit):
        raise ValueError(f"generate: needs {need} positions (t_max {t_max}, model limit {limit})")
    window = getattr(getattr(model, "config", None), "sliding_window", None)
    if window is not None and max_len + max_new_tokens > window:
        raise NotImplementedError(f"generate: {max_len + max_new_tokens} positions exceed the model's "
                                  f"sliding window ({window}); sliding-window decoding is not implemented")
    # the prefix holds the prefill's rows, a sample's own rows its new tokens; t_max= is a floor on the sum
    cache = SharedPrefixKVCache.for_model(model, B, R, t_pad, max(max_new_tokens, t_max - t_pad), device=device,
                                          dtype=kv_dtype)
    ids = input_ids
    if t_pad > T0:
        ids = torch.cat([ids, torch.full((B, t_pad - T0), pad_token_id, dtype=ids.dtype, device=device)], 1)
    logits = model.prefill(ids, cache, lens)
    cache.plen.copy_(lens)
    # the draws have the shape [B·R, V] of the same call on repeated prompts: the same tokens for a seed
    tok = sample(logits.repeat_interleave(R, 0), **sampling)
    out = torch.full((B, T0 + max_new_tokens), pad_token_id, dtype=input_ids.dtype, device=device)
    out[:, :T0] = input_ids
    ar = torch.arange(T0, device=device)
    out[:, :T0].masked_fill_(ar[None, :] >= lens[:, None], pad_token_id)
    out = out.repeat_interleave(R, 0)
    pos = lens.repeat_interleave(R)  # position of `tok`
    out.scatter_(1, pos.view(-1, 1), tok.view(-1, 1))
    done = ((tok == eos_token_id) if eos_token_id is not None
            else torch.zeros(B * R, dtype=torch.bool, device=device))
    if graph is None:
        graph = device.type == "cuda" and sampling["generator"] is None
    loop = _DecodeLoop(model, cache, tok, pos, out, done, eos_token_id, sampling)
    _run_decode(loop, max_new_tokens - 1, graph, max_len + 1, eos_token_id, sync_every)
    return out, cache


@torch.no_grad()
def generate(model, input_ids: Optional[torch.Tensor], max_new_tokens: int, *,
             lengths: Optional[torch.Tensor] = None, cache: Optional[KVCache] = None,
             temperature: float = 0.0, top_k: Optional[int] = None, top_p: Optional[float] = None,
             eos_token_id: Optional[int] = None, pad_token_id: int = 0, graph: Optional[bool] = None,
             t_max: Optional[int] = None, sync_every: int = 32, generator: Optional[torch.Generator] = None,
             return_cache: bool = False, kv_dtype=None, num_return_sequences: int = 1):
    """Continue each prompt of ``input_ids`` [B, T0] (right-padded; ``lengths`` [B] = prompt
    lengths, default T0) by ``max_new_tokens`` tokens.  Returns [B, T0 + max_new_tokens]: row b
    holds its prompt, then its new tokens from position lengths[b] on, then ``pad_token_id``.

    ``temperature`` 0 = greedy; ``top_k`` / ``top_p`` restrict sampling.  ``graph`` (default: on
    for a GPU model without an explicit ``generator``) captures the decode step into a HIP graph.

    ``return_cache=True`` returns ``(out, cache)``; ``cache=`` that object continues the same
    sequences: ``input_ids`` [B, Tn] then holds the next turn only (right-padded, ``lengths`` its
    token counts; ``None`` or Tn = 0: keep generating), only the new tokens run through the model
    (``ops.append_attention`` over the cache), and the result [B, Tn + max_new_tokens] is laid out
    as above relative to this turn.  The cache must have room: reserve it with ``t_max=`` on the
    first call (history + 1 + Tn + max_new_tokens rows).  ``ValueError`` for a cache that no
    ``generate`` call filled, a batch or layout mismatch, too little room, or the model's position
    limit; one host sync (``cache.lengths.max()``).

    ``kv_dtype`` = ``"fp8"`` (or ``torch.float8_e4m3fn``) keeps the KV cache in OCP e4m3 without
    scales — each row clamped to ±448 and rounded to nearest even from the bf16 row the default
    cache would hold, by prefill and decode alike — for half the cache bytes held and streamed per
    token; ``None`` (default) keeps the model's dtype.  A cache of fp8 rows cannot be continued
    (``cache=`` raises ``NotImplementedError``).

    ``num_return_sequences`` = R > 1 draws R samples of every prompt (``temperature`` > 0): the B
    prompts are prefilled once into a ``SharedPrefixKVCache`` that holds each prompt once and R
    short tails, and the decode loop runs at batch B·R with ``ops.decode_attention_shared``.  The
    result is [B·R, T0 + max_new_tokens], row b·R + r laid out as above; the tokens are those of
    the same call on ``input_ids.repeat_interleave(R, 0)`` with the same ``generator``.  The
    returned cache is the shared one, and cannot be continued (``cache=`` raises
    ``NotImplementedError``); R > 1 together with ``cache=`` or greedy decoding is a ``ValueError``.
    """
    kv_dtype = _kv_dtype(kv_dtype)
    R = int(num_return_sequences)
    if R < 1:
        raise ValueError(f"generate: num_return_sequences must be >= 1, got {num_return_sequences}")
    if cache is not None and R > 1:
        raise ValueError("generate: num_return_sequences > 1 starts from prompts, not from cache=")
    if isinstance(cache, SharedPrefixKVCache):
        raise NotImplementedError("generate: continuing from a shared prefix cache (num_return_sequences > 1) is "
                                  "not implemented")
    if R > 1:
        if temperature <= 0.0:
            raise ValueError("generate: num_return_sequences > 1 needs temperature > 0 (greedy samples of one "
                             "prompt are copies of each other)")
        sampling = dict(temperature=temperature, top_k=top_k, top_p=top_p, generator=generator)
        out, shared = _generate_shared(model, input_ids, max_new_tokens, R, lengths, sampling, eos_token_id,
                                       pad_token_id, graph, t_max, sync_every, kv_dtype)
        return (out, shared) if return_cache else out
    if cache is not None:
        sampling = dict(temperature=temperature, top_k=top_k, top_p=top_p, generator=generator)
        out = _continue(model, input_ids, max_new_tokens, cache, lengths, sampling, eos_token_id, pad_token_id,
                        graph, sync_every)
        return (out, cache) if return_cache else out
    device = input_ids.device
    B, T0 = input_ids.shape
    if max_new_tokens <= 0:
        return input_ids.clone()
    lens = (torch.full((B,), T0, dtype=torch.int64, device=device) if lengths is None
            else lengths.to(device=device, dtype=torch.int64))
    max_len = int(lens.max())  # one host sync, before any decoding
    if int(lens.min()) < 1:
        raise ValueError("generate: every prompt needs at least one token")
    t_pad = model.prefill_length(T0)
    need = max(t_pad, max_len + max_new_tokens)
    t_max = t_max or need
    limit = model.max_positions()
    if t_max < need or (limit is not None and need > limit):
        raise ValueError(f"generate: needs {need} positions (t_max {t_max}, model limit {limit})")
    window = getattr(getattr(model, "config", None), "sliding_window", None)
    if window is not None and max_len + max_new_tokens > window:
        # the decode kernel attends over every cached position: past the window its logits would
        # silently differ from a sliding-window model's (the training forward refuses T > window too)
        raise NotImplementedError(f"generate: {max_len + max_new_tokens} positions exceed the model's "
                                  f"sliding window ({window}); sliding-window decoding is not implemented")
    cache = KVCache.for_model(model, B, t_max, device=device, dtype=kv_dtype)
    ids = input_ids
    if t_pad > T0:
        ids = torch.cat([ids, torch.full((B, t_pad - T0), pad_token_id, dtype=ids.dtype, device=device)], 1)
    sampling = dict(temperature=temperature, top_k=top_k, top_p=top_p, generator=generator)
    logits = model.prefill(ids, cache, lens)
    tok = sample(logits, **sampling)
    out = torch.full((B, T0 + max_new_tokens), pad_token_id, dtype=input_ids.dtype, device=device)
    out[:, :T0] = input_ids
    ar = torch.arange(T0, device=device)
    out[:, :T0].masked_fill_(ar[None, :] >= lens[:, None], pad_token_id)
    pos = lens.clone()  # position of `tok`
    out.scatter_(1, pos.view(-1, 1), tok.view(-1, 1))
    done = (tok == eos_token_id) if eos_token_id is not None else torch.zeros(B, dtype=torch.bool, device=device)
    if graph is None:
        graph = device.type == "cuda" and generator is None
    loop = _DecodeLoop(model, cache, tok, pos, out, done, eos_token_id, sampling)
    _run_decode(loop, max_new_tokens - 1, graph, max_len + 1, eos_token_id, sync_every)
    return (out, cache) if return_cache else out


__all__ = ["KVCache", "SharedPrefixKVCache", "generate", "sample"]
