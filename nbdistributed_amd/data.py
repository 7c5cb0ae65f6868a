"""Batch building for variable-length text: several documents packed into one row.

A padded batch spends attention (T² per row) and every GEMM on pad tokens.  Packing puts whole
documents back to back into rows of a fixed length and tells the model where each starts through
``position_ids`` that restart at 0 — what ``transformers.DataCollatorWithFlattening`` emits, and
what ``LlamaForCausalLM.forward(..., position_ids=)`` turns into document-masked flash attention
(``ops.packed_bounds``): the attention cost is Σ lenᵢ² instead of T².
"""
from __future__ import annotations

from typing import Optional, Sequence


def pack_sequences(seqs: Sequence, T: int, pad_id: int, max_rows: Optional[int] = None):
    """Pack token sequences into rows of length ``T``: ``(input_ids, position_ids, labels)``,
    each int64 [R, T].

    First-fit-decreasing: documents in order of decreasing length (ties in input order), each into
    the first row that still has room.  A document is never split; one longer than ``T`` raises
    ``ValueError``, and so does needing more than ``max_rows`` rows.  ``position_ids`` count from 0
    inside each document.  A row's tail is padded with ``pad_id`` as one more "document" (positions
    from 0) whose labels are -100; elsewhere ``labels`` equal ``input_ids`` — the model ignores the
    target at every document's first token itself."""
    import torch

    docs = [torch.as_tensor(s, dtype=torch.int64).reshape(-1) for s in seqs]
    for i, d in enumerate(docs):
        if d.numel() > T:
            raise ValueError(f"pack_sequences: document {i} has {d.numel()} tokens, more than a row ({T}); "
                             "documents are never split")
    order = sorted((i for i, d in enumerate(docs) if d.numel() > 0), key=lambda i: -docs[i].numel())
    rows, room = [], []
    for i in order:
        n = docs[i].numel()
        for r in range(len(rows)):
            if room[r] >= n:
                break
        else:
            if max_rows is not None and len(rows) >= max_rows:
                raise ValueError(f"pack_sequences: the documents need more than max_rows={max_rows} rows of {T}")
            rows.append([])
            room.append(T)
            r = len(rows) - 1
        rows[r].append(i)
        room[r] -= n
    R = len(rows)
    input_ids = torch.full((R, T), int(pad_id), dtype=torch.int64)
    position_ids = torch.zeros((R, T), dtype=torch.int64)
    labels = torch.full((R, T), -100, dtype=torch.int64)
    for r, members in enumerate(rows):
        t = 0
        for i in members:
            n = docs[i].numel()
            input_ids[r, t:t + n] = docs[i]
            labels[r, t:t + n] = docs[i]
            position_ids[r, t:t + n] = torch.arange(n)
            t += n
        if t < T:
            position_ids[r, t:] = torch.arange(T - t)
    return input_ids, position_ids, labels


__all__ = ["pack_sequences"]
