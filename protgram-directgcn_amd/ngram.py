"""Upstream n-gram graph producer on the GPU.

The reference builds each level's transition graph with Dask string processing
(``src/pipeline/data_builder.py``):

* sequences come from ``DataLoader.parse_sequences`` (``src/utils/data_utils.py:182-212``: '>' headers,
  id = header.split('|')[1] or the first word, sequence lines stripped and upper-cased);
* only the FIRST sequence gets a leading space and EVERY sequence a trailing space
  (``_preprocess_sequence_tuple_for_bag``, :29-35);
* nodes are the distinct length-n windows, ids = ranks in sorted string order (:38-42, :171-175);
* transitions are consecutive windows inside one sequence (:45-54), aggregated to counts (:277-281).

Here the windows become base-K integer keys with an order-preserving character code, computed by the HIP
kernel ``pg_ngram_keys`` (one block per sequence); node ids and transition counts come from two GPU sorts
(``torch.unique``). The result is the raw transition table that ``graph.build_propagation_csr`` (or the
reference's ``DirectedNgramGraph``) consumes.
"""
from __future__ import annotations

import ctypes
import math
import os
import random
from dataclasses import dataclass
from typing import Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch

from ._lib import check, load_library


def read_fasta(path: str) -> Iterator[Tuple[str, str]]:
    """(protein_id, sequence) pairs with the parsing rules of DataLoader.parse_sequences
    (data_utils.py:182-212)."""
    pid: Optional[str] = None
    parts: List[str] = []
    with open(os.path.normpath(path), "r", encoding="utf-8", errors="ignore") as f:
        for line in f:
            line = line.strip()
            if not line:
                continue
            if line.startswith(">"):
                if pid and parts:
                    yield pid, "".join(parts)
                header = line[1:]
                fields = header.split("|")
                pid = fields[1] if len(fields) > 1 and fields[1] else header.split()[0]
                parts = []
            elif pid is not None:
                parts.append(line.upper())
    if pid and parts:
        yield pid, "".join(parts)


def preprocess(sequences: Sequence[str], pad: bool = True) -> List[str]:
    """data_builder.py:29-35 + :98-103: a leading space on the first sequence only, a trailing space on every
    sequence (pad=False: the sequences as given)."""
    if not pad:
        return list(sequences)
    return [(" " if i == 0 else "") + s + " " for i, s in enumerate(sequences)]


@dataclass
class NgramTransitions:
    n: int
    num_nodes: int
    src: torch.Tensor      # int64 [E] (sorted by (src, dst))
    dst: torch.Tensor      # int64 [E]
    cnt: torch.Tensor      # float32 [E] transition counts (the reference's edge weights)
    node_keys: torch.Tensor  # int64 [N] sorted window keys (node id = position)
    alphabet: str          # characters in code order (code = index)

    def node_strings(self) -> List[str]:
        """Decode the node keys to the n-gram strings (the reference's idx_to_node map, data_builder.py:264)."""
        return decode_keys(self.node_keys.cpu().numpy(), self.alphabet, self.n)


def decode_keys(keys: np.ndarray, alphabet: str, n: int) -> List[str]:
    K = len(alphabet)
    k = keys.astype(np.int64).copy()
    digits = np.empty((k.size, n), dtype=np.int64)
    for j in range(n - 1, -1, -1):
        digits[:, j] = k % K
        k //= K
    table = np.array(list(alphabet))
    return ["".join(row) for row in table[digits]] if k.size else []


def encode(sequences: Sequence[str]):
    """Concatenated bytes, int64 offsets, the order-preserving code table and the alphabet."""
    try:
        raw = [s.encode("latin-1") for s in sequences]
    except UnicodeEncodeError as e:
        raise ValueError("sequences must be single-byte (latin-1) text: windows are taken over characters") from e
    lens = np.fromiter((len(b) for b in raw), dtype=np.int64, count=len(raw))
    offsets = np.zeros(len(raw) + 1, dtype=np.int64)
    np.cumsum(lens, out=offsets[1:])
    buf = np.frombuffer(b"".join(raw), dtype=np.uint8)
    present = np.flatnonzero(np.bincount(buf, minlength=256)) if buf.size else np.zeros(0, dtype=np.int64)
    lut = np.full(256, 0, dtype=np.int32)
    lut[present] = np.arange(present.size, dtype=np.int32)  # byte order == code point order for latin-1
    alphabet = "".join(chr(b) for b in present)
    return buf, offsets, lut, alphabet


def ngram_transitions(sequences: Sequence[str], n: int, device="cuda", pad: bool = True) -> NgramTransitions:
    """Nodes and weighted transitions of the level-n graph (data_builder.py run(), phases 1-2)."""
    if n < 1:
        raise ValueError("n must be >= 1")
    seqs = preprocess(sequences, pad)
    buf, offsets, lut, alphabet = encode(seqs)
    K = max(len(alphabet), 1)
    if n * math.log2(K) >= 62.5:
        raise ValueError(f"{K}^{n} windows do not fit a 64-bit key")
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("the n-gram producer runs on the MI355X only (no CPU path)")
    T = int(buf.size)
    e = torch.zeros(0, dtype=torch.int64, device=dev)
    if T == 0:
        return NgramTransitions(n, 0, e, e, e.float(), e, alphabet)
    b = torch.from_numpy(buf.copy()).to(dev)
    off = torch.from_numpy(offsets).to(dev)
    lt = torch.from_numpy(lut).to(dev)
    keys = torch.empty(T, dtype=torch.int64, device=dev)
    nxt = torch.empty(T, dtype=torch.int64, device=dev)
    lib = load_library()
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    check(lib.pg_ngram_keys(len(seqs), ctypes.c_void_p(off.data_ptr()), ctypes.c_void_p(b.data_ptr()),
                            ctypes.c_void_p(lt.data_ptr()), n, K, ctypes.c_void_p(keys.data_ptr()),
                            ctypes.c_void_p(nxt.data_ptr()), stream), "pg_ngram_keys")
    node_keys = torch.unique(keys[keys >= 0])  # sorted: node id = rank of the window in string order
    N = int(node_keys.numel())
    m = nxt >= 0
    si = torch.searchsorted(node_keys, keys[m])
    di = torch.searchsorted(node_keys, nxt[m])
    pairs, cnt = torch.unique(si * max(N, 1) + di, return_counts=True)
    return NgramTransitions(n, N, pairs // max(N, 1), pairs % max(N, 1), cnt.to(torch.float32), node_keys, alphabet)


# ------------------------------------------------------------------------------------------------------------
# The builder's on-disk level files, next-node labels and (n-1)-gram feature pooling
# ------------------------------------------------------------------------------------------------------------

def _keys_of(strings: Sequence[str], alphabet: str, n: int) -> np.ndarray:
    """Base-K keys of equal-length strings under `alphabet`'s code (index = code)."""
    if len(strings) == 0:
        return np.zeros(0, dtype=np.int64)
    lut = np.full(256, -1, dtype=np.int64)
    for i, ch in enumerate(alphabet):
        lut[ord(ch)] = i
    try:
        raw = np.frombuffer("".join(strings).encode("latin-1"), dtype=np.uint8)
    except UnicodeEncodeError as e:
        raise ValueError("n-gram strings must be single-byte (latin-1) text") from e
    if raw.size != n * len(strings):
        raise ValueError(f"every n-gram must have length {n}")
    codes = lut[raw].reshape(len(strings), n)
    if (codes < 0).any():
        raise ValueError("n-gram strings use characters outside the alphabet")
    K = len(alphabet)
    keys = np.zeros(len(strings), dtype=np.int64)
    for j in range(n):
        keys = keys * K + codes[:, j]
    return keys


def transitions_from_table(n: int, src, dst, cnt, node_strings: Sequence[str], alphabet: Optional[str] = None,
                           device=None) -> NgramTransitions:
    """An NgramTransitions from a plain table: node ids must be the ranks of `node_strings` in sorted string order
    (the reference's ids, data_builder.py:171-175); `alphabet` defaults to the characters present, in code-point
    order (pass the other level's alphabet to pool across levels)."""
    node_strings = list(node_strings)
    if alphabet is None:
        alphabet = "".join(sorted(set("".join(node_strings))))
    if len(alphabet) and n * math.log2(max(len(alphabet), 2)) >= 62.5:
        raise ValueError(f"{len(alphabet)}^{n} windows do not fit a 64-bit key")
    keys = _keys_of(node_strings, alphabet, n)
    if keys.size > 1 and not (np.diff(keys) > 0).all():
        raise ValueError("node ids are not the ranks of the n-grams in sorted string order")
    dev = torch.device(device) if device is not None else torch.device("cpu")
    as64 = lambda a: torch.as_tensor(np.asarray(a, dtype=np.int64)).to(dev)  # noqa: E731
    return NgramTransitions(n, len(node_strings), as64(src), as64(dst),
                            torch.as_tensor(np.asarray(cnt, dtype=np.float32)).to(dev), as64(keys), alphabet)


def level_paths(directory: str, n: int) -> Tuple[str, str]:
    """(ngram_map_n{n}.parquet, aggregated_edges_n{n}.parquet) -- the builder's files for level n
    (data_builder.py:145, :281)."""
    return (os.path.join(directory, f"ngram_map_n{n}.parquet"), os.path.join(directory, f"aggregated_edges_n{n}.parquet"))


def write_level(t: NgramTransitions, directory: str) -> Tuple[str, str]:
    """Write a level in the builder's schema: the n-gram map {id: int64, ngram: string} sorted by id
    (data_builder.py:170-177) and the aggregated edges {source, target, weight: int64}
    (groupby(['source', 'target']).size(), :268-286)."""
    import pyarrow as pa
    import pyarrow.parquet as pq
    os.makedirs(directory, exist_ok=True)
    mpath, epath = level_paths(directory, t.n)
    pq.write_table(pa.table({"id": pa.array(np.arange(t.num_nodes, dtype=np.int64)),
                             "ngram": pa.array(t.node_strings(), type=pa.string())}), mpath)
    pq.write_table(pa.table({"source": pa.array(t.src.cpu().numpy().astype(np.int64)),
                             "target": pa.array(t.dst.cpu().numpy().astype(np.int64)),
                             "weight": pa.array(t.cnt.cpu().numpy().astype(np.int64))}), epath)
    return mpath, epath


def read_level(directory: str, n: int, device=None, alphabet: Optional[str] = None) -> NgramTransitions:
    """Read a level written by the reference's builder (or write_level): nodes from the n-gram map, weighted
    edges from the aggregated-edge file read as DirectedNgramGraph does (graph_utils.py:106-117: source/target
    int64, weight float32); edges are returned sorted by (source, target)."""
    import pyarrow.parquet as pq
    mpath, epath = level_paths(directory, n)
    nodes = pq.read_table(mpath, columns=["id", "ngram"]).to_pandas()
    nodes = nodes.sort_values("id")
    ids = nodes["id"].to_numpy(dtype=np.int64)
    if not np.array_equal(ids, np.arange(ids.size)):
        raise ValueError(f"{mpath}: ids are not 0..N-1")
    strings = nodes["ngram"].astype(str).tolist()
    if os.path.exists(epath):
        e = pq.read_table(epath, columns=["source", "target", "weight"]).to_pandas()
        src = e["source"].to_numpy(dtype=np.int64)
        dst = e["target"].to_numpy(dtype=np.int64)
        w = e["weight"].to_numpy(dtype=np.float32)
        order = np.lexsort((dst, src))
        src, dst, w = src[order], dst[order], w[order]
    else:  # the builder removes the file when a level has no edges (data_builder.py:291-294)
        src = dst = np.zeros(0, dtype=np.int64)
        w = np.zeros(0, dtype=np.float32)
    N = len(strings)
    if src.size and (src.min() < 0 or dst.min() < 0 or src.max() >= N or dst.max() >= N):
        raise ValueError(f"{epath}: edge endpoints outside 0..{N - 1}")
    return transitions_from_table(n, src, dst, w, strings, alphabet, device)


def read_edge_parts(paths: Sequence[str]) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The builder's raw transition parts ('source target' per line, data_builder.py:263-266) aggregated like
    groupby(['source', 'target']).size(): (source, target, count), sorted by (source, target). Malformed lines
    are skipped (on_bad_lines='skip')."""
    pairs = []
    for path in paths:
        with open(path, "r", encoding="utf-8", errors="ignore") as f:
            for line in f:
                parts = line.split()
                if len(parts) != 2:
                    continue
                try:
                    pairs.append((int(parts[0]), int(parts[1])))
                except ValueError:
                    continue
    if not pairs:
        z = np.zeros(0, dtype=np.int64)
        return z, z, z
    a = np.asarray(pairs, dtype=np.int64)
    uniq, counts = np.unique(a, axis=0, return_counts=True)  # lexicographic = sorted by (source, target)
    return uniq[:, 0], uniq[:, 1], counts.astype(np.int64)


def next_node_labels(t: NgramTransitions, tie_break: str = "first",
                     generator: Optional[torch.Generator] = None) -> Tuple[torch.Tensor, int]:
    """The trainer's next_node task labels (protgram_directgcn_trainer.py:222-236) for all nodes at once: the
    successor with the largest transition count, the node itself when it has none; num_classes = N. The
    reference breaks ties with random.choice; tie_break='first' takes the smallest successor id, 'random' a
    uniformly random one (torch `generator` on the transitions' device)."""
    N = t.num_nodes
    dev = t.src.device
    labels = torch.arange(N, dtype=torch.int64, device=dev)
    if N == 0 or t.src.numel() == 0:
        return labels, max(N, 1) if N == 0 else N
    w = t.cnt.to(torch.float32)
    rowmax = torch.full((N,), float("-inf"), device=dev).scatter_reduce(0, t.src, w, "amax")
    cand = w == rowmax[t.src]
    cs, cd = t.src[cand], t.dst[cand]
    if tie_break == "first":
        pick = torch.full((N,), N, dtype=torch.int64, device=dev).scatter_reduce(0, cs, cd, "amin")
    elif tie_break == "random":
        r = torch.rand(cs.numel(), generator=generator, device=dev)
        best = torch.full((N,), -1.0, device=dev).scatter_reduce(0, cs, r, "amax")
        win = r == best[cs]
        pick = torch.full((N,), N, dtype=torch.int64, device=dev).scatter_reduce(0, cs[win], cd[win], "amin")
    else:
        raise ValueError("tie_break must be 'first' or 'random'")
    has = pick < N
    labels[has] = pick[has]
    return labels, N


def pool_features(cur: NgramTransitions, prev: NgramTransitions, emb_prev: torch.Tensor) -> torch.Tensor:
    """Initial level-n features from the level-(n-1) embeddings (protgram_directgcn_trainer.py:317-330): the mean
    of the prefix (ngram[:-1]) and suffix (ngram[1:]) rows that exist at level n-1 -- both: (a + b) / 2 in fp32 as
    np.mean does, one: that row, none: zeros. Both levels must share one alphabet code."""
    if cur.n != prev.n + 1:
        raise ValueError("prev must be level n-1")
    if cur.alphabet != prev.alphabet:
        raise ValueError("the two levels use different alphabet codes (build them from the same sequences, or pass "
                         "one alphabet to transitions_from_table / read_level)")
    if emb_prev.size(0) != prev.num_nodes:
        raise ValueError("emb_prev must have one row per level-(n-1) node")
    dev = emb_prev.device
    K = max(len(cur.alphabet), 1)
    keys = cur.node_keys.to(dev)
    pk = prev.node_keys.to(dev)
    prefix = keys // K
    suffix = keys % (K ** (cur.n - 1))
    F = emb_prev.size(1)
    x = torch.zeros(cur.num_nodes, F, dtype=emb_prev.dtype, device=dev)
    if cur.num_nodes == 0 or pk.numel() == 0:
        return x

    def lookup(q):
        i = torch.searchsorted(pk, q).clamp_(max=pk.numel() - 1)
        return i, pk[i] == q

    pi, pok = lookup(prefix)
    si, sok = lookup(suffix)
    both = pok & sok
    x[both] = (emb_prev[pi[both]] + emb_prev[si[both]]) / 2
    only_p = pok & ~sok
    x[only_p] = emb_prev[pi[only_p]]
    only_s = sok & ~pok
    x[only_s] = emb_prev[si[only_s]]
    return x


# ------------------------------------------------------------------------------------------------------------
# closest_aa task labels (protgram_directgcn_trainer.py:239-269) as a k-hop reach of letter bitmasks
# (csrc/pg_labels.hip)
# ------------------------------------------------------------------------------------------------------------

AMINO_ACIDS = "ACDEFGHIKLMNPQRSTVWY"  # the trainer's AMINO_ACID_ALPHABET order: bit / index b is letter b


def _vp(t: torch.Tensor):
    return ctypes.c_void_p(t.data_ptr()) if t.numel() else None


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _check_letters(letters: str) -> str:
    letters = "".join(letters)
    if len(letters) < 1 or len(letters) > 32:
        raise ValueError("letters must hold 1 to 32 characters (one bit of a 32-bit mask each)")
    if len(set(letters)) != len(letters):
        raise ValueError("letters must not repeat a character")
    return letters


def _level_device(t: NgramTransitions, what: str) -> torch.device:
    dev = t.src.device
    if dev.type != "cuda" or t.dst.device != dev:
        raise RuntimeError(f"{what} runs on the MI355X only: the level's tensors must be on the GPU (no CPU fallback)")
    return dev


def letter_masks(t: NgramTransitions, letters: str = AMINO_ACIDS) -> torch.Tensor:
    """uint32 [N] on t.src's device: bit b of entry i is set when node i's n-gram contains letters[b]. Characters of
    t.alphabet outside `letters` (' ', X, U, ...) set no bit."""
    letters = _check_letters(letters)
    dev = _level_device(t, "letter_masks")
    N, n, K = int(t.num_nodes), int(t.n), max(len(t.alphabet), 1)
    masks = torch.empty(N, dtype=torch.uint32, device=dev)
    if N == 0:
        return masks
    if n < 1 or n * math.log2(K) >= 62.5:
        raise ValueError(f"{K}^{n} windows do not fit a 64-bit key")
    keys = t.node_keys.to(dev).contiguous()
    if keys.dtype != torch.int64 or keys.shape != (N,):
        raise ValueError("node_keys must be int64 [num_nodes]")
    if int(keys.min()) < 0 or int(keys.max()) >= K ** n:
        raise IndexError(f"node_keys outside [0, {K}^{n})")
    bit = {ch: b for b, ch in enumerate(letters)}
    code_bit = torch.tensor([bit.get(ch, -1) for ch in t.alphabet] or [-1], dtype=torch.int32).to(dev)
    check(load_library().pg_ngram_letter_masks(N, _vp(keys), n, K, _vp(code_bit), _vp(masks), _stream(dev)),
          "pg_ngram_letter_masks")
    return masks


def _out_csr(t: NgramTransitions, dev: torch.device) -> Tuple[torch.Tensor, torch.Tensor]:
    """(rowptr int64 [N + 1], col int64 [E]) of the out-edges; t.src is sorted (the dataclass's contract), so the
    row pointer is the running sum of its counts, as graph._rowptr builds it. Every endpoint is checked here: the hop
    kernel gathers reach[col[e]] unguarded."""
    N = int(t.num_nodes)
    src, dst = t.src.contiguous(), t.dst.contiguous()
    if src.dtype != torch.int64 or dst.dtype != torch.int64 or src.dim() != 1 or src.shape != dst.shape:
        raise ValueError("src and dst must be int64 [E]")
    if src.numel():
        if int(dst.min()) < 0 or int(dst.max()) >= N:
            raise IndexError(f"dst outside [0, {N})")
        if int(src.min()) < 0 or int(src.max()) >= N:
            raise IndexError(f"src outside [0, {N})")
        if src.numel() > 1 and bool((src[1:] < src[:-1]).any()):
            raise ValueError("src must be sorted (NgramTransitions keeps its edges ordered by (src, dst))")
    rowptr = torch.zeros(N + 1, dtype=torch.int64, device=dev)
    if src.numel():
        torch.cumsum(torch.bincount(src, minlength=N), 0, out=rowptr[1:])
    return rowptr, dst


def _check_hops(k_hops) -> int:
    k = int(k_hops)
    if k != k_hops or k < 0 or k > 255:
        raise ValueError("k_hops must be an integer in [0, 255]")
    return k


def _own_bits(masks: torch.Tensor, n_bits: int) -> torch.Tensor:
    """bool [N, n_bits]: the bits of the uint32 masks."""
    shifts = torch.arange(n_bits, dtype=torch.int32, device=masks.device)
    return ((masks.view(torch.int32).unsqueeze(1) >> shifts) & 1).bool()


def _hops(rowptr, col, masks, k, n_bits, dist=None, target=None, labels=None):
    """Hops 1..k of pg_reach_hop_u32 with two reach buffers that swap roles."""
    lib = load_library()
    dev = masks.device
    N = masks.numel()
    cur, nxt = masks, torch.empty_like(masks)
    if k > 1:
        cur = masks.clone()  # the caller's masks stay as they are
    for h in range(1, k + 1):
        # an empty col has no address: every row is empty then and any non-null pointer stands in for it
        check(lib.pg_reach_hop_u32(N, _vp(rowptr), _vp(col) or _vp(rowptr), _vp(cur), _vp(nxt), h, n_bits,
                                   _vp(dist) if dist is not None else None, n_bits,
                                   _vp(target) if target is not None else None,
                                   _vp(labels) if labels is not None else None, _stream(dev)), "pg_reach_hop_u32")
        cur, nxt = nxt, cur


def letter_distances(t: NgramTransitions, k_hops: int, letters: str = AMINO_ACIDS) -> torch.Tensor:
    """uint8 [N, len(letters)]: entry (v, b) = min(k_hops, length of the shortest out-path from node v to a node whose
    n-gram contains letters[b]), 0 when v's own n-gram contains it. k_hops launches of the hop kernel."""
    letters = _check_letters(letters)
    k = _check_hops(k_hops)
    dev = _level_device(t, "letter_distances")
    N, L = int(t.num_nodes), len(letters)
    if N == 0:
        return torch.empty(0, L, dtype=torch.uint8, device=dev)
    rowptr, col = _out_csr(t, dev)
    masks = letter_masks(t, letters)
    dist = torch.full((N, L), k, dtype=torch.uint8, device=dev)
    dist[_own_bits(masks, L)] = 0
    _hops(rowptr, col, masks, k, L, dist=dist)
    return dist


def draw_targets(num_nodes: int, letters: str = AMINO_ACIDS, rng=None) -> List[int]:
    """One target letter index per node, drawn as the trainer draws them (protgram_directgcn_trainer.py:247):
    rng.choice(list(letters)) once per node in node order, on the host; `rng` defaults to the `random` module, so
    random.seed(s) before the call gives the reference's sequence."""
    rng = random if rng is None else rng
    index = {ch: b for b, ch in enumerate(letters)}
    pool = list(letters)
    return [index[rng.choice(pool)] for _ in range(num_nodes)]


def _target_indices(targets, N: int, letters: str, rng) -> torch.Tensor:
    """uint8 [N] on the host: the drawn or given target letter index per node."""
    index = {ch: b for b, ch in enumerate(letters)}
    if targets is None:
        idx = draw_targets(N, letters, rng)
    elif isinstance(targets, str):
        try:
            idx = [index[ch] for ch in targets]
        except KeyError as e:
            raise ValueError(f"target letter {e.args[0]!r} is not one of the letters") from None
    elif torch.is_tensor(targets):
        idx = targets.detach().cpu().to(torch.int64).reshape(-1)
    else:
        idx = [int(x) for x in targets]
    idx = torch.as_tensor(idx, dtype=torch.int64).reshape(-1)
    if idx.numel() != N:
        raise ValueError(f"targets must have one entry per node ({N}), got {idx.numel()}")
    if N and (int(idx.min()) < 0 or int(idx.max()) >= len(letters)):
        raise ValueError(f"target indices must lie in [0, {len(letters)})")
    return idx.to(torch.uint8)


def closest_aa_labels(t: NgramTransitions, k_hops: int = 3, targets=None, rng=None,
                      letters: str = AMINO_ACIDS) -> Tuple[torch.Tensor, int]:
    """The trainer's closest_aa task labels (protgram_directgcn_trainer.py:239-269) for all nodes at once: per node a
    target letter, label = the number of hops along out-edges to the nearest node whose n-gram contains it (0: the
    node itself), k_hops when none is within k_hops; num_classes = k_hops + 1. targets=None draws
    rng.choice(list(letters)) per node in node order on the host (`rng`: the `random` module by default), the
    reference's own draw sequence: after random.seed(s) the labels are the reference's. Otherwise `targets` holds one
    letter index per node (sequence or tensor) or is a str of N letters."""
    letters = _check_letters(letters)
    k = _check_hops(k_hops)
    dev = _level_device(t, "closest_aa_labels")
    N = int(t.num_nodes)
    if N == 0:
        return torch.empty(0, dtype=torch.int64, device=dev), k + 1
    tgt = _target_indices(targets, N, letters, rng)
    rowptr, col = _out_csr(t, dev)
    masks = letter_masks(t, letters)
    tgt = tgt.to(dev)
    own = (masks.view(torch.int32) >> tgt.to(torch.int32)) & 1
    labels = torch.where(own.bool(), 0, k).to(torch.int64)
    _hops(rowptr, col, masks, k, len(letters), target=tgt, labels=labels)
    return labels, k + 1


def community_labels(t: NgramTransitions, **kw) -> Tuple[torch.Tensor, int]:
    """The trainer's community task labels (protgram_directgcn_trainer.py:200-220) for all nodes at once: Louvain
    communities of the level's undirected graph (community.combined_graph), found on the GPU by community.louvain
    (`kw`: its classes, max_sweeps, max_levels, min_gain). No nodes: (empty, 1); no entries: (zeros, 1), as the
    reference returns; otherwise communities 0..C-1 in ascending order of their smallest member (the reference's
    numbers come from python-louvain's RNG), an isolated node a community of its own, num_classes = C."""
    from . import community
    g = community.combined_graph(t)
    dev = g.k.device
    if g.n == 0:
        return torch.empty(0, dtype=torch.int64, device=dev), 1
    if g.two_m == 0:
        return torch.zeros(g.n, dtype=torch.int64, device=dev), 1
    labels = community.louvain(g, **kw)
    return labels, int(labels.max()) + 1


def task_labels(t: NgramTransitions, task: str, method: Optional[str] = None, **kw) -> Tuple[torch.Tensor, int]:
    """(labels, num_classes) of one of the trainer's self-supervised tasks (GCN_TASK_TYPES_PER_LEVEL,
    protgram_directgcn_trainer.py:333-341). 'community' needs method='louvain': its labels are this package's
    deterministic Louvain partition, not python-louvain's seeded one."""
    if task != "community" and method is not None:
        raise ValueError(f"method applies to task 'community' only, not to '{task}'")
    if task == "next_node":
        return next_node_labels(t, **kw)
    if task == "closest_aa":
        return closest_aa_labels(t, **kw)
    if task == "community":
        if method == "louvain":
            return community_labels(t, **kw)
        raise ValueError("task 'community' takes its labels from a Louvain partition, which differs from "
                         "python-louvain's seeded one: pass method='louvain' for community_labels (DESIGN §11) or "
                         "supply the labels")
    raise ValueError(f"Unsupported GCN_TASK_TYPE '{task}' for n={t.n}.")
