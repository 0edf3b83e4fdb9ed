"""Protein-level pooling of n-gram node embeddings on the GPU: the tail of the reference's GCN pipeline
(``protgram_directgcn_trainer.py:387-398``, "Step 3: Pooling N-gram Embeddings to Protein Level").

For every protein the embeddings of the n-grams it contains are pooled into one vector:

* ``mode="distinct"`` (the trainer's call, ``EmbeddingProcessor.pool_ngram_embeddings_for_protein_fast``,
  ``src/utils/models_utils.py:209-262``): every n-gram of the protein counts once; fp32 sum from +0.0 in ascending
  node id order, divided by the number of distinct ids;
* ``mode="windows"`` (``pool_ngram_embeddings_for_protein``, ``:197-207``): every window with its multiplicity, fp32
  sum from +0.0 in window order, divided by the number of valid windows.

Pooling reads the raw sequences of ``parse_sequences`` (no ' ' padding); a window with a character outside the
level's alphabet, or whose n-gram is not a node, is skipped; a protein without a valid window gets no vector. Both
modes match the reference bit for bit.

``pg_ngram_window_ids`` turns the sequences into one node id per window, ``pg_pool_rows_f32`` pools the table rows
per protein (csrc/pg_ngram.hip, csrc/pg_pool.hip). There is no CPU path.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Iterable, Optional, Sequence, Tuple

import numpy as np
import torch

from ._lib import check, load_library
from .ngram import NgramTransitions

DENSE_TABLE_MAX = 1 << 24  # key -> id table entries (64 MiB of int32) up to which window_ids reads a table


def _vp(t: Optional[torch.Tensor]):
    return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _need_cuda(dev: torch.device, what: str):
    if dev.type != "cuda":
        raise RuntimeError(f"{what} runs on the MI355X only: no CPU fallback")


def distinct_max_nodes() -> int:
    """The largest node count the in-kernel bitmap path of ``mode="distinct"`` takes."""
    return int(load_library().pg_pool_distinct_max_nodes())


def alphabet_lut(alphabet: str) -> np.ndarray:
    """int32 [256]: the code of each byte under `alphabet` (code = index), -1 for a byte outside it (ngram.encode's
    table maps those to 0, which is right for the producer, whose alphabet is every byte present)."""
    lut = np.full(256, -1, dtype=np.int32)
    for i, ch in enumerate(alphabet):
        if ord(ch) > 255:
            raise ValueError("the alphabet must be single-byte (latin-1) text")
        lut[ord(ch)] = i
    return lut


def _encode_raw(sequences: Sequence[str]) -> Tuple[np.ndarray, np.ndarray]:
    try:
        raw = [s.encode("latin-1") for s in sequences]
    except UnicodeEncodeError as e:
        raise ValueError("sequences must be single-byte (latin-1) text: windows are taken over characters") from e
    lens = np.fromiter((len(b) for b in raw), dtype=np.int64, count=len(raw))
    offsets = np.zeros(len(raw) + 1, dtype=np.int64)
    np.cumsum(lens, out=offsets[1:])
    return np.frombuffer(b"".join(raw), dtype=np.uint8), offsets


def window_ids(sequences: Sequence[str], t: NgramTransitions, device=None,
               dense_table: Optional[bool] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(ids int32 [T], offsets int64 [P + 1]) on the GPU, T = total characters: ids[offsets[s] + i] is the node id
    of the window sequences[s][i : i + n] (models_utils.py:202, :238-239), -1 where the window leaves the sequence,
    holds a character outside t.alphabet or is no node of the level. `dense_table`: look the key up in a dense
    key -> id table (default: when K^n <= 2^24 entries) instead of a binary search in the node keys."""
    dev = torch.device(device) if device is not None else t.node_keys.device
    _need_cuda(dev, "window_ids")
    sequences = list(sequences)
    K, n, N = max(len(t.alphabet), 1), int(t.n), int(t.num_nodes)
    buf, offsets = _encode_raw(sequences)
    off = torch.from_numpy(offsets).to(dev)
    T = int(buf.size)
    ids = torch.empty(T, dtype=torch.int32, device=dev)
    if T == 0:
        return ids, off
    size = K ** n
    if dense_table is None:
        dense_table = size <= DENSE_TABLE_MAX
    elif dense_table and size > (1 << 31):
        raise ValueError(f"a dense table of {K}^{n} entries is too large")
    keys = t.node_keys.to(dev).contiguous()
    table = None
    if dense_table:
        table = torch.full((size,), -1, dtype=torch.int32, device=dev)
        table[keys] = torch.arange(N, dtype=torch.int32, device=dev)
    b = torch.from_numpy(buf.copy()).to(dev)
    lut = torch.from_numpy(alphabet_lut(t.alphabet)).to(dev)
    check(load_library().pg_ngram_window_ids(len(sequences), _vp(off), _vp(b), _vp(lut), n, K, _vp(keys), N,
                                             _vp(table), _vp(ids), _stream(dev)), "pg_ngram_window_ids")
    return ids, off


def _check_table(emb: torch.Tensor, N: Optional[int] = None):
    if not torch.is_tensor(emb) or emb.dim() != 2:
        raise ValueError("emb must be a [num_nodes, F] tensor")
    _need_cuda(emb.device, "protein pooling")
    if emb.dtype != torch.float32:
        raise ValueError("emb must be float32 (the model's embedding output)")
    if N is not None and emb.size(0) != N:
        raise ValueError(f"emb has {emb.size(0)} rows, the level has {N} nodes")
    if emb.size(1) < 1:
        raise ValueError("emb must have at least one column")
    if emb.size(1) > 1 and emb.stride(1) != 1 or (emb.size(0) > 1 and emb.stride(0) < emb.size(1)):
        emb = emb.contiguous()
    return emb


def pool_rows(emb: torch.Tensor, rowptr: torch.Tensor, ids: torch.Tensor, distinct: bool = False,
              order: Optional[torch.Tensor] = None, sort_lists: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
    """pg_pool_rows_f32: (means fp32 [P, F], counts int32 [P]) of the lists ids[rowptr[r] : rowptr[r + 1]] (int32;
    negative entries are skipped) over the rows of emb [N, F]. distinct=False: every entry, in list order;
    distinct=True: every id once, in ascending order (N <= distinct_max_nodes()). `order`: the sequence in which the
    lists are started, default longest first (sort_lists=False: as given); results do not depend on it."""
    emb = _check_table(emb)
    dev = emb.device
    if rowptr.device != dev or ids.device != dev:
        raise ValueError("rowptr and ids must be on emb's device")
    if rowptr.dtype != torch.int64 or ids.dtype != torch.int32 or rowptr.dim() != 1 or ids.dim() != 1:
        raise ValueError("rowptr must be int64 [P + 1] and ids int32 [T]")
    if rowptr.numel() < 1:
        raise ValueError("rowptr must have P + 1 >= 1 entries")
    rowptr, ids = rowptr.contiguous(), ids.contiguous()
    P, N, F = rowptr.numel() - 1, emb.size(0), emb.size(1)
    out = torch.empty(P, F, dtype=torch.float32, device=dev)
    counts = torch.empty(P, dtype=torch.int32, device=dev)
    if P == 0:
        return out, counts
    lens = rowptr[1:] - rowptr[:-1]
    if int(rowptr[0]) < 0 or int(rowptr[-1]) > ids.numel() or bool((lens < 0).any()):
        raise ValueError("rowptr must be non-decreasing within [0, len(ids)]")
    if ids.numel() and int(ids.max()) >= N:
        raise ValueError(f"ids must be < N = {N} (negative: skipped)")
    if distinct and N > distinct_max_nodes():
        raise ValueError(f"distinct=True takes N <= {distinct_max_nodes()} nodes; sort the lists instead")
    if order is None and sort_lists:
        order = torch.argsort(lens, descending=True, stable=True)
    if order is not None:
        if order.device != dev or order.dtype != torch.int64 or order.shape != (P,):
            raise ValueError("order must be int64 [P] on emb's device")
        order = order.contiguous()
        if not bool((torch.sort(order).values == torch.arange(P, device=dev)).all()):
            raise ValueError("order must be a permutation of 0..P-1")
    lde = emb.stride(0) if emb.size(0) > 1 else F
    # an empty ids tensor has no address: every list is empty then and any non-null pointer stands in for it
    check(load_library().pg_pool_rows_f32(_vp(emb), lde, N, F, _vp(rowptr), _vp(ids) or _vp(rowptr), _vp(order), P,
                                          1 if distinct else 0, _vp(out), F, _vp(counts), 0, _stream(dev)),
          "pg_pool_rows_f32")
    return out, counts


def _sorted_distinct_lists(rowptr: torch.Tensor, ids: torch.Tensor, N: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """The lists with duplicates removed and ids ascending, by one global sort (the path for N above the bitmap cap)."""
    P = rowptr.numel() - 1
    dev = ids.device
    lens = rowptr[1:] - rowptr[:-1]
    which = torch.repeat_interleave(torch.arange(P, device=dev), lens)
    seg = ids[int(rowptr[0]):int(rowptr[-1])] if P else ids[:0]
    ok = seg >= 0
    u = torch.unique(which[ok] * max(N, 1) + seg[ok].to(torch.int64))  # sorted: by list, then by id
    new_ptr = torch.zeros(P + 1, dtype=torch.int64, device=dev)
    if P:
        torch.cumsum(torch.bincount(u // max(N, 1), minlength=P), 0, out=new_ptr[1:])
    return new_ptr, (u % max(N, 1)).to(torch.int32)


def pool_proteins(sequences: Sequence[str], t: NgramTransitions, emb: torch.Tensor, mode: str = "distinct",
                  distinct_path: str = "auto") -> Tuple[torch.Tensor, torch.Tensor]:
    """(pooled fp32 [P, F], counts int32 [P]) on emb's device: row p is the pooled vector of sequences[p] over the
    node embeddings emb [t.num_nodes, F] (module docstring; counts[p] = 0 and a zero row: the reference returns no
    vector for that protein). distinct_path: "bitmap" (in-kernel, N <= distinct_max_nodes()), "sort" (torch.unique
    of (protein, id), then the windows kernel) or "auto" (bitmap where it applies); identical bits either way."""
    if mode not in ("distinct", "windows"):
        raise ValueError("mode must be 'distinct' or 'windows'")
    if distinct_path not in ("auto", "bitmap", "sort"):
        raise ValueError("distinct_path must be 'auto', 'bitmap' or 'sort'")
    emb = _check_table(emb, int(t.num_nodes))
    ids, off = window_ids(sequences, t, device=emb.device)
    if mode == "windows":
        return pool_rows(emb, off, ids, distinct=False)
    N = int(t.num_nodes)
    if distinct_path == "auto":
        distinct_path = "bitmap" if N <= distinct_max_nodes() else "sort"
    if distinct_path == "bitmap":
        return pool_rows(emb, off, ids, distinct=True)
    ptr, uids = _sorted_distinct_lists(off, ids, N)
    return pool_rows(emb, ptr, uids, distinct=False)


def pooled_dict(protein_ids: Iterable[str], pooled, counts, id_map: Optional[Dict[str, str]] = None
                ) -> Dict[str, np.ndarray]:
    """The reference's result: {protein id: vector} without the proteins that have no valid window (count 0); a later
    duplicate id overwrites an earlier one; keys mapped with id_map.get(k, k) (protgram_directgcn_trainer.py:399-400)."""
    vec = pooled.detach().cpu().numpy() if torch.is_tensor(pooled) else np.asarray(pooled)
    cnt = counts.detach().cpu().numpy() if torch.is_tensor(counts) else np.asarray(counts)
    protein_ids = list(protein_ids)
    if len(protein_ids) != vec.shape[0] or cnt.shape[0] != vec.shape[0]:
        raise ValueError("protein_ids, pooled and counts must have one entry per protein")
    out: Dict[str, np.ndarray] = {}
    for i, pid in enumerate(protein_ids):
        if cnt[i] > 0:
            out[pid] = vec[i].copy()
    if id_map:
        out = {id_map.get(k, k): v for k, v in out.items()}
    return out


def protein_embeddings(model, data, t: NgramTransitions, proteins: Iterable[Tuple[str, str]], mode: str = "distinct",
                       id_map: Optional[Dict[str, str]] = None) -> Dict[str, np.ndarray]:
    """The tail of ProtGramDirectGCNTrainer.run() for one level: the model's eval-mode embeddings of `data`
    (extract_gcn_node_embeddings, models_utils.py:264-275) pooled per protein without leaving the device, as the
    reference's dict. `proteins`: (id, sequence) pairs, e.g. ngram.read_fasta(path). The model's training flag is
    restored."""
    proteins = list(proteins)
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            _, emb = model(data)
    finally:
        model.train(was_training)
    pooled, counts = pool_proteins([s for _, s in proteins], t, emb, mode=mode)
    return pooled_dict([p for p, _ in proteins], pooled, counts, id_map)
