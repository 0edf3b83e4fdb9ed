"""Float64 NumPy restatement of the reference's PCA step (EmbeddingProcessor.apply_pca, src/utils/models_utils.py:88-136:
StandardScaler().fit_transform, then PCA(n_components=k).fit_transform), written for the tests: the oracle. It runs the
reference's steps in float64 on the fp32 inputs, with two passes over the data and no moment trick, so it shares no
code path with the product. tests/test_pca_host.py pins it to the reference's recorded outputs
(tests/golden/pca_proteins.npz, tools/golden/make_pca_golden.py)."""
import functools

import numpy as np

EPS = np.finfo(np.float64).eps
CASES = ["A", "B", "C", "D", "E"]


@functools.lru_cache(maxsize=None)
def fixture():
    """The committed cases (four files: a committed file stays below 1 MiB); F_x is A_x[F_rows]. Read-only."""
    from golden_util import load
    fx = {}
    for stem in ("pca_proteins", "pca_proteins_f", "pca_proteins_c", "pca_proteins_c_ref"):
        fx.update(load(stem))
    fx["F_x"] = fx["A_x"][fx["F_rows"]]
    for v in fx.values():
        v.setflags(write=False)
    return fx


@functools.lru_cache(maxsize=None)
def oracle(name):
    """The oracle on a committed case, computed once per session and shared (read-only)."""
    fx = fixture()
    o = pca_oracle(fx[f"{name}_x"], int(fx[f"{name}_target"][0]))
    for v in o.values():
        v.setflags(write=False)
    return o


def kept(eigenvalues):
    """The components that are compared value by value: eigenvalue > 1e-8 lambda_0 (a kept null direction, as in case
    E, is arbitrary; its outputs are only required to be <= 1e-5 in magnitude)."""
    w = np.asarray(eigenvalues)
    return np.flatnonzero(w > 1e-8 * w[0])


def pca_oracle(x, target_dim, fit_rows=None):
    """x: [n, F] (fp32 values). Returns a dict of float64 arrays: out [n, k], eigenvalues [k] (explained_variance_),
    all_eigenvalues [F], components [k, F], mean [F], scale [F], and the folded affine map center [F], W [k, F] with
    out = (x - center) @ W.T up to the second centring (|mean of the scaled data| ~ 1e-17).
    fit_rows: fit on x[fit_rows] only (the transform of the other rows uses that fit)."""
    x = np.asarray(x, dtype=np.float64)
    fit = x if fit_rows is None else x[fit_rows]
    n, F = fit.shape
    k = min(int(target_dim), F, n)
    # StandardScaler: column mean and population variance; scikit-learn's _is_constant_feature
    # (sklearn/preprocessing/_data.py) gives a column within the two-pass variance's error bound the scale 1
    mean = fit.mean(axis=0)
    var = ((fit - mean) ** 2).mean(axis=0)
    constant = var <= n * EPS * var + (n * mean * EPS) ** 2
    scale = np.sqrt(var)
    scale[constant] = 1.0
    z = (fit - mean) / scale
    # PCA, covariance_eigh: eigen-decomposition of the sample covariance (divisor n - 1), descending
    zmean = z.mean(axis=0)
    zc = z - zmean
    cov = zc.T @ zc / (n - 1)
    w, v = np.linalg.eigh(cov)
    w, v = w[::-1].copy(), v[:, ::-1]
    w[w < 0.0] = 0.0
    comps = v.T[:k].copy()
    # svd_flip(u_based_decision=False): the largest-magnitude entry of every component is positive
    big = np.argmax(np.abs(comps), axis=1)
    comps *= np.sign(comps[np.arange(k), big])[:, None]
    out = ((x - mean) / scale - zmean) @ comps.T
    return {"out": out, "eigenvalues": w[:k], "all_eigenvalues": w, "components": comps, "mean": mean, "scale": scale,
            "center": mean, "W": comps / scale}


def well_separated(all_eigenvalues, k, rel=1e-2):
    """Indices c < k whose eigenvalue is at least rel * lambda_0 away from both neighbours' (of all F eigenvalues)."""
    w = np.asarray(all_eigenvalues, dtype=np.float64)
    gap = np.full(w.size, np.inf)
    d = w[:-1] - w[1:]
    gap[:-1] = np.minimum(gap[:-1], d)
    gap[1:] = np.minimum(gap[1:], d)
    return np.flatnonzero(gap[:k] >= rel * w[0])


def dict_rows(protein_ids, counts, id_map=None):
    """(keys, rows): what the reference's dict holds after the pooling step (protgram_directgcn_trainer.py:399-400) --
    proteins with a vector, a later duplicate id replacing the value but keeping the position, then the same once more
    for the ids mapped with id_map.get(k, k) -- as the row of `pooled` behind every key, in dict order."""
    d = {}
    for i, pid in enumerate(protein_ids):
        if counts[i] > 0:
            d[pid] = i
    if id_map:
        d = {id_map.get(k, k): v for k, v in d.items()}
    return list(d), np.array(list(d.values()), dtype=np.int64)
