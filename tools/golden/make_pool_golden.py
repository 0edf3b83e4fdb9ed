#!/usr/bin/env python3
"""Golden vectors for protein-level pooling, from the REFERENCE's own functions (build container only).

Imports, unchanged, ``src/utils/models_utils.py`` and calls ``EmbeddingProcessor.pool_ngram_embeddings_for_protein_fast``
(:209-262, the trainer's Step 3) and ``EmbeddingProcessor.pool_ngram_embeddings_for_protein`` (:197-207). The module's
imports that are absent here and unused by those two functions are stubbed in ``sys.modules``: PyG and ``h5py`` through
``pyg_boundary.install()``, ``sklearn`` and ``tqdm`` when missing.

Writes ``tests/golden/pool_proteins.npz``: ~40 seeded (id, sequence) pairs (lengths 0, 1, n-1, n, n+1 and up to 400, a
homopolymer, sequences with X / U, one with a lower-case letter, one duplicated id) and, per level n = 2, 3: the
level's sorted node strings (the windows of the first 28 sequences padded as the builder pads them), an [N, 20] fp32
table with -0.0 entries, and the outputs of both reference functions (returned ids and vectors). The divisors are
restated here in two lines (the reference does not return them). No reference source or bytecode is written.

Usage:  python tools/golden/make_pool_golden.py
"""
import io
import os
import sys
import types
from contextlib import redirect_stdout

sys.dont_write_bytecode = True
REF = "/root/reference"
if not os.path.isdir(os.path.join(REF, "src")):
    sys.exit("make_pool_golden.py: /root/reference is absent; fixtures can only be generated in the build container")

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(REPO, "tests", "golden")

sys.path.insert(0, HERE)
import pyg_boundary  # noqa: E402

pyg_boundary.install()


def _stub(name, **attrs):
    m = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


try:
    import sklearn.decomposition  # noqa: F401
    import sklearn.preprocessing  # noqa: F401
except ImportError:
    sk = _stub("sklearn")
    sk.decomposition = _stub("sklearn.decomposition", PCA=object)
    sk.preprocessing = _stub("sklearn.preprocessing", StandardScaler=object)
try:
    import tqdm.auto  # noqa: F401
except ImportError:
    tq = _stub("tqdm")
    tq.auto = _stub("tqdm.auto", tqdm=lambda it, **kw: it)
sys.path.insert(0, REF)

import numpy as np  # noqa: E402

from src.utils.models_utils import EmbeddingProcessor  # noqa: E402

ALPHABET = "ACDEFGHIKLMNPQRSTVWY"
F = 20
N_NODE_SEQS = 28  # the level's nodes come from these; later sequences bring windows that are no nodes


def proteins(seed=11):
    rng = np.random.default_rng(seed)
    lens = [0, 1, 2, 3, 4, 2, 3, 5, 7, 8, 9, 17, 33, 40, 63, 64, 65, 90, 120, 150, 200, 257, 300, 400, 31, 12, 6, 50,
            # not among the node sequences:
            3, 2, 25, 60, 110, 400, 5, 4, 30, 45, 16, 80]
    out = []
    for i, L in enumerate(lens):
        seq = "".join(rng.choice(list(ALPHABET), size=L))
        if i == 10:
            seq = "K" * 9                      # a homopolymer
        if i in (12, 20):                      # X inside the level's alphabet
            seq = seq[:5] + "X" + seq[6:]
        if i == 30:
            seq = seq[:7] + "U" + seq[8:]      # U occurs in no node sequence
        if i == 31:
            seq = seq[:20] + "k" + seq[21:]    # a lower-case letter (parse_sequences upper-cases; raw input may not be)
        if i == 34:
            seq = "UUUUU"                      # no window is a node
        if i == 36:
            seq = seq[:10] + "XU" + seq[12:]
        out.append((f"P{i:03d}", seq))
    out[33] = ("P007", out[33][1])             # a duplicated id: the later protein overwrites the earlier one
    return out


def level_nodes(prots, n):
    """Distinct windows of the node sequences, padded as data_builder.py:29-35 pads them, sorted; id = rank."""
    grams = set()
    for i, (_, s) in enumerate(prots[:N_NODE_SEQS]):
        s = (" " if i == 0 else "") + s + " "
        grams.update(s[k:k + n] for k in range(len(s) - n + 1))
    return sorted(grams)


def main():
    prots = proteins()
    fx = {"ids": np.array([p for p, _ in prots]), "seqs": np.array([s for _, s in prots])}
    rng = np.random.default_rng(5)
    for n in (2, 3):
        nodes = level_nodes(prots, n)
        ngram_map = {g: i for i, g in enumerate(nodes)}
        emb = rng.standard_normal((len(nodes), F)).astype(np.float32)
        emb[rng.random(emb.shape) < 0.03] = -0.0
        emb[ngram_map[prots[n][1]]] = -0.0   # the length-n protein's only window: a row of -0.0
        with redirect_stdout(io.StringIO()):
            fast = EmbeddingProcessor.pool_ngram_embeddings_for_protein_fast(prots, n, ngram_map, emb)
        slow_ids, slow_vecs = [], []
        for i, pd in enumerate(prots):
            pid, v = EmbeddingProcessor.pool_ngram_embeddings_for_protein(pd, n, ngram_map, emb)
            if v is not None:
                slow_ids.append(i)
                slow_vecs.append(v)
        # the divisors, restated: distinct ids / valid windows per protein (position in `prots`)
        win = [[ngram_map[s[k:k + n]] for k in range(len(s) - n + 1) if s[k:k + n] in ngram_map] for _, s in prots]
        fx[f"n{n}_nodes"] = np.array(nodes)
        fx[f"n{n}_emb"] = emb
        fx[f"n{n}_fast_ids"] = np.array(list(fast.keys()))
        fx[f"n{n}_fast_vecs"] = np.stack(list(fast.values())).astype(np.float32)
        fx[f"n{n}_windows_idx"] = np.array(slow_ids, np.int64)  # positions in `ids` (ids repeat)
        fx[f"n{n}_windows_vecs"] = np.stack(slow_vecs)
        fx[f"n{n}_distinct_counts"] = np.array([len(set(w)) for w in win], np.int32)
        fx[f"n{n}_windows_counts"] = np.array([len(w) for w in win], np.int32)
        assert all(v.dtype == np.float32 for v in slow_vecs) and fx[f"n{n}_fast_vecs"].dtype == np.float32
        print(f"  n={n}: {len(nodes)} nodes, fast {len(fast)} proteins, windows {len(slow_ids)} proteins")
    out = os.path.join(OUT, "pool_proteins.npz")
    np.savez_compressed(out, **fx)
    print(f"  wrote {os.path.relpath(out, REPO)} ({os.path.getsize(out) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
