#!/usr/bin/env python3
"""Golden vectors for the closest_aa task labels, from the REFERENCE's own trainer method (build container only).

Imports, unchanged, ``src/pipeline/protgram_directgcn_trainer.py`` and calls
``ProtGramDirectGCNTrainer._generate_closest_amino_acid_labels`` (:239-269) on a ``SimpleNamespace`` graph with the
three attributes the method reads: ``number_of_nodes``, ``A_out_w`` (a coalesced sparse COO matrix of the transition
counts) and ``node_sequences``. The module-level imports that are absent here and unused by that method are stubbed in
``sys.modules``: PyG and ``h5py`` through ``pyg_boundary.install()`` plus ``torch_geometric.utils.subgraph`` /
``to_networkx``; ``config``, ``Bio``, ``requests``, ``sklearn``, ``tqdm`` and ``pandas`` when missing.

Writes ``tests/golden/closest_aa.npz``. Per case: the node strings, src / dst / counts, the seed, the target letter
indices the method drew (re-drawn here after re-seeding: ``random.choice(AMINO_ACID_ALPHABET)`` once per node) and the
labels for k = 0, 1, 2, 3. Cases:

* ``p1_n1``, ``p1_n2``, ``p1_n3``: levels 1-3 of ``tests/golden/p1_fasta.npz`` (seeds 1234 + n);
* ``dense_n2``, ``dense_n3``: levels of a few hundred short sequences made here over 8 standard letters plus X. A, C,
  D, E and X mix freely and A is followed by every character (rows that end in A reach an out-degree equal to the
  number of characters); T, V, W and Y run as a chain T -> V -> W -> Y, so that distances 2 and 3 arise through
  branching paths.

Every case with n >= 2 has all of the classes 0..3 at k = 3 (asserted). Data only: no reference source or bytecode is
written (``sys.dont_write_bytecode``).

Usage:  python tools/golden/make_closest_aa_golden.py
"""
import importlib
import io
import os
import random
import sys
import types
import zipfile
from contextlib import redirect_stdout

sys.dont_write_bytecode = True
REF = "/root/reference"
if not os.path.isdir(os.path.join(REF, "src")):
    sys.exit("make_closest_aa_golden.py: /root/reference is absent; fixtures can only be generated in the build "
             "container")

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(REPO, "tests", "golden")

sys.path.insert(0, HERE)
import pyg_boundary  # noqa: E402

pyg_boundary.install()
sys.modules["torch_geometric.utils"].subgraph = None      # names the trainer imports; the label method uses neither
sys.modules["torch_geometric.utils"].to_networkx = None


def _stub(name, **attrs):
    m = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


def _absent(name):
    try:
        importlib.import_module(name)
        return False
    except ImportError:
        return True


class _Config:  # the trainer's configuration class; the label method reads DEBUG_VERBOSE of an instance only
    pass


_stub("config", Config=_Config)
if _absent("Bio"):
    _stub("Bio").SeqIO = _stub("Bio.SeqIO")
if _absent("requests"):
    _stub("requests")
if _absent("pandas"):
    _stub("pandas")
if _absent("sklearn.decomposition"):
    sk = _stub("sklearn")
    sk.decomposition = _stub("sklearn.decomposition", PCA=object)
    sk.preprocessing = _stub("sklearn.preprocessing", StandardScaler=object)
if _absent("tqdm.auto"):
    tq = _stub("tqdm", tqdm=lambda it, **kw: it)
    tq.auto = _stub("tqdm.auto", tqdm=lambda it, **kw: it)
sys.path.insert(0, REF)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from src.pipeline import protgram_directgcn_trainer as ref_trainer  # noqa: E402

LETTERS = "".join(ref_trainer.AMINO_ACID_ALPHABET)
KS = (0, 1, 2, 3)


def dense_sequences(seed=3, count=300):
    """Short sequences over A C D E T V W Y and X. A, C, D, E and X follow one another freely (A most often); T, V, W
    and Y run as the chain T -> V -> W -> Y, which a free letter enters at T now and then and which leaves into a free
    letter after Y. A alone is also followed, rarely, by V, W and Y: rows that end in A have every character as a
    successor, while a node inside the chain is three hops from most letters."""
    rng = np.random.default_rng(seed)
    free, weight = list("ACDEX"), np.array([0.4, 0.15, 0.15, 0.15, 0.15])
    chain = {"T": "V", "V": "W", "W": "Y"}
    out = []
    for _ in range(count):
        L = int(rng.integers(4, 15))
        s = [free[int(rng.choice(len(free), p=weight))]]
        while len(s) < L:
            last = s[-1]
            r = rng.random()
            if last in chain:
                s.append(chain[last])
            elif last != "Y" and r < 0.06:
                s.append("T")
            elif last == "A" and r < 0.21:
                s.append("VWY"[int((r - 0.06) / 0.05)])
            else:
                s.append(free[int(rng.choice(len(free), p=weight))])
        out.append("".join(s))
    return out


def level(seqs, n):
    """The builder's level (data_builder.py:29-54, :171-175, :267-271) restated: a leading space on the first
    sequence, a trailing one on every sequence; nodes = sorted distinct windows; counted consecutive windows."""
    pre = [(" " if i == 0 else "") + s + " " for i, s in enumerate(seqs)]
    grams = sorted({s[k:k + n] for s in pre for k in range(len(s) - n + 1)})
    ids = {g: i for i, g in enumerate(grams)}
    counts = {}
    for s in pre:
        for k in range(len(s) - n):
            key = (ids[s[k:k + n]], ids[s[k + 1:k + 1 + n]])
            counts[key] = counts.get(key, 0) + 1
    keys = sorted(counts)
    return (grams, np.array([k[0] for k in keys], np.int64), np.array([k[1] for k in keys], np.int64),
            np.array([counts[k] for k in keys], np.int64))


def reference_labels(strings, src, dst, w, k, seed):
    N = len(strings)
    A = torch.sparse_coo_tensor(torch.from_numpy(np.stack([src, dst])), torch.from_numpy(w.astype(np.float32)),
                                (N, N)).coalesce()
    graph = types.SimpleNamespace(number_of_nodes=N, A_out_w=A, node_sequences=list(strings))
    me = types.SimpleNamespace(config=types.SimpleNamespace(DEBUG_VERBOSE=False))
    random.seed(seed)
    with redirect_stdout(io.StringIO()):
        labels, classes = ref_trainer.ProtGramDirectGCNTrainer._generate_closest_amino_acid_labels(me, graph, k)
    assert classes == k + 1 and labels.dtype == torch.int64 and labels.shape == (N,)
    return labels.numpy()


def main():
    with np.load(os.path.join(OUT, "p1_fasta.npz"), allow_pickle=False) as z:
        p1 = {k: z[k] for k in z.files}
    cases = []
    for n in (1, 2, 3):
        cases.append((f"p1_n{n}", n, [str(s) for s in p1[f"n{n}_ngrams"]], p1[f"n{n}_src"], p1[f"n{n}_dst"],
                      p1[f"n{n}_w"], 1234 + n))
    seqs = dense_sequences()
    for n in (2, 3):
        cases.append((f"dense_n{n}", n, *level(seqs, n), 4321 + n))
    fx = {"cases": np.array([c[0] for c in cases]), "letters": np.array(LETTERS),
          "dense_seqs": np.array(seqs)}
    for name, n, strings, src, dst, w, seed in cases:
        random.seed(seed)
        targets = np.array([LETTERS.index(random.choice(ref_trainer.AMINO_ACID_ALPHABET)) for _ in strings], np.uint8)
        fx[f"{name}:n"], fx[f"{name}:seed"] = np.int64(n), np.int64(seed)
        fx[f"{name}:strings"] = np.array(strings)
        fx[f"{name}:src"], fx[f"{name}:dst"], fx[f"{name}:w"] = src, dst, w
        fx[f"{name}:targets"] = targets
        for k in KS:
            fx[f"{name}:labels_k{k}"] = reference_labels(strings, src, dst, w, k, seed)
        hist = np.bincount(fx[f"{name}:labels_k3"], minlength=4)
        deg = np.bincount(src, minlength=len(strings)).max() if src.size else 0
        chars = len(set("".join(strings)))
        print(f"  {name}: {len(strings)} nodes, {src.size} edges, {chars} characters, max out-degree {deg}, "
              f"k=3 histogram {hist.tolist()}")
        if n >= 2:
            assert (hist > 0).all(), f"{name}: a class of 0..3 is empty at k = 3; choose another seed"
        if name.startswith("dense"):
            assert deg == chars, f"{name}: no row reaches out-degree {chars}"
    out = os.path.join(OUT, "closest_aa.npz")
    # an .npz is a zip of .npy members; written here with a fixed member date so that a rerun gives the same bytes
    with zipfile.ZipFile(out, "w", zipfile.ZIP_DEFLATED) as zf:
        for key, val in fx.items():
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with zf.open(info, "w") as f:
                np.lib.format.write_array(f, np.asanyarray(val), allow_pickle=False)
    print(f"  wrote {os.path.relpath(out, REPO)} ({os.path.getsize(out) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
