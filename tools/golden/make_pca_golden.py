#!/usr/bin/env python3
"""Golden vectors for the PCA step, from the REFERENCE's own function (build container only).

Imports, unchanged, ``src/utils/models_utils.py`` and calls ``EmbeddingProcessor.apply_pca`` (:88-136, the trainer's
Step 5) with scikit-learn as installed. The module's imports that are absent here and unused by that function are
stubbed in ``sys.modules``: PyG and ``h5py`` through ``pyg_boundary.install()``, ``tqdm`` when missing.

Writes ``tests/golden/pca_proteins.npz`` (cases A, B, D, E), ``pca_proteins_f.npz`` (F), ``pca_proteins_c.npz`` (C: the
input and the oracle's small arrays) and ``pca_proteins_c_ref.npz`` (C: the recorded results; the oracle's float64 output
for every second row, ``C_out_rows``): four files because C alone holds 1.8 MB and a committed file stays below 1 MiB.
Cases X = (Z diag(rho^j)) Q diag(u) + off v from
``numpy.random.default_rng(seed)`` (Z standard normal [P, F], Q a random orthogonal matrix, u uniform on [0.5, 2], v
Gaussian), rounded to float32:

    case seed    P    F  target  rho   off
    A       1  643   64      64  0.9     1   the production dims
    B       2  257   20       7  0.8   100   F not a multiple of 4, a large offset
    C       3 1301  128      64  0.95    3   several row chunks
    D       4  211   12      64  0.7     0   column 5 set to the constant 3.25 (k = 12)
    E       5    5    8      64  0.7     1   n < F (k = 5)
    F          A's rows as a pooled table with a counts vector that zeroes about every seventh row, a protein id list
               with two duplicated ids and an id_map: the dict the pooling step would hand to apply_pca

Per case: the inputs, the reference's result with output_dtype float32 and float16, the scikit-learn solver it took,
and the float64 oracle's (tests/pca_ref.py) output, eigenvalues, components, mean and scale. The generator asserts the
conditions the tests' bounds rest on and fails rather than write a fixture outside them: neighbouring kept eigenvalues
at least 1e-7 lambda_0 apart (E exempt: its kept null direction has eigenvalue 0), the largest and second-largest
|entry| of every component at least 1e-4 apart (relative), at least 7 components with gaps of 1e-2 lambda_0 to both
neighbours in A-D. No reference source or bytecode is written.

Usage:  python tools/golden/make_pca_golden.py
"""
import io
import os
import sys
import types
from contextlib import redirect_stdout

sys.dont_write_bytecode = True
REF = "/root/reference"
if not os.path.isdir(os.path.join(REF, "src")):
    sys.exit("make_pca_golden.py: /root/reference is absent; fixtures can only be generated in the build container")

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


import sklearn.decomposition  # noqa: E402,F401  (the reference's own dependency: required here)
import sklearn.preprocessing  # noqa: E402,F401

try:
    import tqdm.auto  # noqa: F401
except ImportError:
    tq = _stub("tqdm")
    tq.auto = _stub("tqdm.auto", tqdm=lambda it, **kw: it)
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np  # noqa: E402

from pca_ref import dict_rows, pca_oracle, well_separated  # noqa: E402
from src.utils import models_utils  # noqa: E402
from src.utils.models_utils import EmbeddingProcessor  # noqa: E402

CASES = {  # name: (seed, P, F, target, rho, off)
    "A": (1, 643, 64, 64, 0.9, 1.0),
    "B": (2, 257, 20, 7, 0.8, 100.0),
    "C": (3, 1301, 128, 64, 0.95, 3.0),
    "D": (4, 211, 12, 64, 0.7, 0.0),
    "E": (5, 5, 8, 64, 0.7, 1.0),
}
GAP_MIN, SIGN_MARGIN_MIN, WELL_MIN = 1e-7, 1e-4, 7


def make_x(seed, P, F, rho, off):
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((P, F))
    q, _ = np.linalg.qr(rng.standard_normal((F, F)))
    u = rng.uniform(0.5, 2.0, size=F)
    v = rng.standard_normal(F)
    return (((z * rho ** np.arange(F)) @ q) * u + off * v).astype(np.float32)


class _Recorder(models_utils.PCA):
    """The reference's PCA class, remembering the last fitted instance (to read the solver it took)."""
    last = None

    def fit_transform(self, X, y=None):
        out = super().fit_transform(X, y)
        _Recorder.last = self
        return out


def reference(vectors, target, dtype):
    """EmbeddingProcessor.apply_pca on {id: vector}; returns (keys, matrix, solver, explained_variance_)."""
    models_utils.PCA = _Recorder
    try:
        with redirect_stdout(io.StringIO()):
            res = EmbeddingProcessor.apply_pca(vectors, target, 42, output_dtype=dtype)
    finally:
        models_utils.PCA = _Recorder.__mro__[1]
    pca = _Recorder.last
    return list(res), np.stack(list(res.values())), pca._fit_svd_solver, np.asarray(pca.explained_variance_, np.float64)


def check_conditions(name, o, k):
    w = o["all_eigenvalues"]
    gaps = (w[:-1] - w[1:])[:k]  # every kept eigenvalue against its lower neighbour (and so its upper one)
    comps = np.sort(np.abs(o["components"]), axis=1)
    margin = ((comps[:, -1] - comps[:, -2]) / comps[:, -1]).min()
    well = well_separated(w, k)
    print(f"  {name}: k={k} min gap {gaps.min() / w[0]:.2e} lambda_0, sign margin {margin:.2e}, "
          f"{well.size} well-separated components")
    if name != "E":
        assert gaps.min() >= GAP_MIN * w[0], f"case {name}: eigenvalue gap {gaps.min() / w[0]:.2e} lambda_0"
        assert well.size >= WELL_MIN, f"case {name}: only {well.size} well-separated components"
    assert margin >= SIGN_MARGIN_MIN, f"case {name}: sign margin {margin:.2e}"
    return well


def record(fx, name, x, keys, target):
    """One case on the rows x (in dict order under `keys`)."""
    vectors = {kk: row for kk, row in zip(keys, x)}
    k32, r32, solver, ev = reference(vectors, target, np.float32)
    k16, r16, _, _ = reference(vectors, target, np.float16)
    assert k32 == list(keys) and k16 == list(keys) and r32.dtype == np.float32 and r16.dtype == np.float16
    o = pca_oracle(x, target)
    k = o["components"].shape[0]
    assert r32.shape == (x.shape[0], k)
    well = check_conditions(name, o, k)
    err = np.abs(r32[:, well] - o["out"][:, well]).max(axis=0) / np.abs(o["out"][:, well]).max(axis=0)
    ev_err = np.abs(ev - o["eigenvalues"]).max() / o["eigenvalues"][0]
    print(f"     solver {solver}; reference fp32 vs oracle on those: {err.max():.2e} of the column's largest |value|; "
          f"explained_variance_ {ev_err:.2e} lambda_0")
    fx[f"{name}_target"] = np.array([target], np.int64)
    fx[f"{name}_ref32"] = r32
    fx[f"{name}_ref16"] = r16
    fx[f"{name}_ref_explained_variance"] = ev
    fx[f"{name}_solver"] = np.array(solver)
    out_rows = np.arange(0, x.shape[0], 2 if name == "C" else 1)
    fx[f"{name}_out_rows"] = out_rows
    fx[f"{name}_out"] = o["out"][out_rows]
    fx[f"{name}_eigenvalues"] = o["eigenvalues"]
    fx[f"{name}_all_eigenvalues"] = o["all_eigenvalues"]
    fx[f"{name}_components"] = o["components"]
    fx[f"{name}_mean"] = o["mean"]
    fx[f"{name}_scale"] = o["scale"]


def main():
    fx = {}
    for name, (seed, P, F, target, rho, off) in CASES.items():
        x = make_x(seed, P, F, rho, off)
        if name == "D":
            x[:, 5] = np.float32(3.25)
        fx[f"{name}_x"] = x
        record(fx, name, x, [f"P{i:04d}" for i in range(P)], target)
    # F: A's rows as the pooling step's output
    x = fx["A_x"]
    P = x.shape[0]
    counts = np.random.default_rng(6).integers(1, 40, size=P).astype(np.int32)
    counts[3::7] = 0
    ids = [f"P{i:04d}" for i in range(P)]
    ids[200] = ids[18]    # a later duplicate with a vector: replaces the value, keeps the place of position 18
    ids[400] = ids[45]    # 45 = 3 + 7 * 6 has no vector: the later one is the key's only entry
    assert counts[18] > 0 and counts[200] > 0 and counts[45] == 0 and counts[400] > 0
    id_map = {ids[5]: "Q00005", ids[300]: ids[8], "unused": "never"}  # the second maps onto an existing key
    assert counts[5] > 0 and counts[300] > 0 and counts[8] > 0
    keys, rows = dict_rows(ids, counts, id_map)
    assert len(keys) == int((counts > 0).sum()) - 2 and keys.index(ids[8]) < keys.index(ids[9])
    fx["F_counts"] = counts
    fx["F_ids"] = np.array(ids)
    fx["F_id_map_from"] = np.array(list(id_map.keys()))
    fx["F_id_map_to"] = np.array(list(id_map.values()))
    fx["F_keys"] = np.array(keys)
    fx["F_rows"] = rows
    record(fx, "F", x[rows], keys, 64)
    big = ("C_ref32", "C_ref16", "C_out", "C_out_rows")
    files = {"pca_proteins": {k: v for k, v in fx.items() if k[0] in "ABDE"},
             "pca_proteins_f": {k: v for k, v in fx.items() if k[0] == "F"},
             "pca_proteins_c": {k: v for k, v in fx.items() if k[0] == "C" and k not in big},
             "pca_proteins_c_ref": {k: fx[k] for k in big}}
    assert sum(len(f) for f in files.values()) == len(fx)
    for stem, arrays in files.items():
        out = os.path.join(OUT, f"{stem}.npz")
        np.savez_compressed(out, **arrays)
        size = os.path.getsize(out)
        print(f"  wrote {os.path.relpath(out, REPO)} ({size / 1024:.0f} KiB)")
        assert size < (1 << 20), f"{stem}.npz: a committed file must stay below 1 MiB"


if __name__ == "__main__":
    main()
