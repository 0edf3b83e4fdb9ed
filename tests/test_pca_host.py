"""PCA reduction, host side (no GPU): the float64 oracle (pca_ref.py) against the reference's recorded outputs
(tests/golden/pca_proteins*.npz, tools/golden/make_pca_golden.py), the dict semantics of reduce.pca_dict's row
selection, the host part of the fit (reduce.model_from_moments) on moments formed in NumPy, and the error paths that are
decided before any HIP call."""
import numpy as np
import pytest
import torch

from golden_util import load
from pca_ref import CASES, dict_rows, fixture, oracle, well_separated
from pca_ref import kept as kept_components



def kept(name):
    """Components compared in full: all of them, in E those with eigenvalue > 1e-8 lambda_0."""
    w = fixture()[f"{name}_eigenvalues"]
    return kept_components(w) if name == "E" else np.arange(w.size)


@pytest.mark.parametrize("name", CASES + ["F"])
def test_oracle_reproduces_its_recorded_arrays(name):
    fx, o = fixture(), oracle(name)
    x = fx[f"{name}_x"]
    assert x.dtype == np.float32
    k = min(int(fx[f"{name}_target"][0]), x.shape[1], x.shape[0])
    assert o["components"].shape == (k, x.shape[1])
    c = kept(name)
    for key in ("mean", "scale", "all_eigenvalues", "eigenvalues"):
        print(name, key, np.abs(o[key] - fx[f"{name}_{key}"]).max())
        assert np.abs(o[key] - fx[f"{name}_{key}"]).max() <= 1e-12 * max(1.0, np.abs(fx[f"{name}_{key}"]).max()), key
    # An eigenvector moves by (rounding of the covariance) / gap. With gaps of 1e-2 lambda_0 that is ~1e-14, and those
    # components and their outputs are held to 1e-12. The others (gaps down to 1e-7 lambda_0) move by up to ~1e-9 when
    # the BLAS merely adds the covariance in another order (another thread count), so they are held to the float64
    # perturbation bound the GPU test uses for components, 1e-6.
    assert np.abs(o["components"][c] - fx[f"{name}_components"][c]).max() <= 1e-6
    well = np.intersect1d(well_separated(fx[f"{name}_all_eigenvalues"], k), c)
    rows = fx[f"{name}_out_rows"]
    print(name, "components", np.abs(o["components"][well] - fx[f"{name}_components"][well]).max(),
          "out", np.abs(o["out"][rows][:, well] - fx[f"{name}_out"][:, well]).max())
    assert np.abs(o["components"][well] - fx[f"{name}_components"][well]).max() <= 1e-12
    scale_out = np.abs(fx[f"{name}_out"]).max()
    assert np.abs(o["out"][rows][:, well] - fx[f"{name}_out"][:, well]).max() <= 1e-12 * scale_out
    if name == "E":
        rest = np.setdiff1d(np.arange(k), c)
        assert rest.size == 1 and np.abs(o["out"][:, rest]).max() <= 1e-5
    if name == "D":
        # the constant column: scale 1, and it is the last component (eigenvalue 0, no output) and in no other
        assert o["scale"][5] == 1.0 and o["mean"][5] == 3.25 and o["eigenvalues"][-1] <= 1e-12
        assert np.abs(o["components"][:-1, 5]).max() < 1e-12 and abs(o["components"][-1, 5] - 1.0) < 1e-12
        assert np.abs(o["out"][:, -1]).max() <= 1e-12


@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_reference_against_the_oracle(name):
    fx = fixture()
    assert str(fx[f"{name}_solver"]) == "covariance_eigh"
    x = fx[f"{name}_x"]
    k = fx[f"{name}_eigenvalues"].size
    well = well_separated(fx[f"{name}_all_eigenvalues"], k)
    assert well.size >= 7
    o = oracle(name)
    ref = fx[f"{name}_ref32"].astype(np.float64)
    assert ref.shape == (x.shape[0], k)
    err = np.abs(ref[:, well] - o["out"][:, well]).max(axis=0)
    bound = 1e-5 * np.abs(o["out"][:, well]).max(axis=0)
    print(name, "reference fp32 - oracle, relative to the column's largest |value|:", (err / bound * 1e-5).max())
    assert (err <= bound).all()
    lam0 = o["eigenvalues"][0]
    ev = np.abs(fx[f"{name}_ref_explained_variance"] - o["eigenvalues"]).max()
    print(name, "explained_variance_ - oracle:", ev / lam0, "lambda_0")
    assert ev <= 1e-6 * lam0
    # the reference's float16 result is its float32 result rounded once
    assert np.array_equal(fx[f"{name}_ref16"], fx[f"{name}_ref32"].astype(np.float16))


def test_case_e_takes_the_full_solver_and_agrees_on_the_kept_components():
    fx, o = fixture(), oracle("E")
    assert str(fx["E_solver"]) == "full" and fx["E_ref32"].shape == (5, 5)
    c = kept("E")
    assert c.tolist() == [0, 1, 2, 3]
    ref = fx["E_ref32"].astype(np.float64)
    assert (np.abs(ref[:, c] - o["out"][:, c]).max(axis=0) <= 1e-5 * np.abs(o["out"][:, c]).max(axis=0)).all()
    assert np.abs(ref[:, 4]).max() <= 1e-5


def test_dict_semantics_agree_with_pooled_dict(pkg):
    fx = fixture()
    ids = [str(s) for s in fx["F_ids"]]
    counts = fx["F_counts"]
    id_map = {str(a): str(b) for a, b in zip(fx["F_id_map_from"], fx["F_id_map_to"])}
    pooled = fx["A_x"]
    keys, rows = pkg.reduce.dict_rows(ids, counts, id_map)
    want = pkg.pool.pooled_dict(ids, pooled, counts, id_map)
    assert keys == list(want) == [str(s) for s in fx["F_keys"]]
    assert np.array_equal(rows, fx["F_rows"])
    for key, r in zip(keys, rows):
        assert np.array_equal(want[key], pooled[r])
    # the restatement the generator used
    k2, r2 = dict_rows(ids, counts, id_map)
    assert k2 == keys and np.array_equal(r2, rows)
    # what the fixture is meant to hold: rows without a vector, a later duplicate that wins and keeps its place, a
    # duplicate whose earlier entry had no vector, a mapped key and a key mapped onto an existing one
    assert (counts == 0).sum() > 80 and len(keys) == (counts > 0).sum() - 2
    assert ids[200] == ids[18] and rows[keys.index(ids[18])] == 200 and keys.index(ids[18]) < keys.index(ids[19])
    assert ids[400] == ids[45] and counts[45] == 0 and rows[keys.index(ids[45])] == 400
    assert "Q00005" in keys and ids[5] not in keys and rows[keys.index(ids[8])] == 300
    assert keys.index(ids[8]) < keys.index(ids[9])
    # torch counts, no id_map, all empty
    k3, r3 = pkg.reduce.dict_rows(["a", "b", "a"], torch.tensor([1, 0, 2], dtype=torch.int32))
    assert k3 == ["a"] and r3.tolist() == [2]
    assert pkg.reduce.dict_rows(["a"], np.array([0]))[0] == []
    with pytest.raises(ValueError):
        pkg.reduce.dict_rows(["a", "b"], np.array([1]))


def _moments(x, shift, rows=None):
    x = np.asarray(x, np.float64)
    if rows is not None:
        x = x[rows]
    d = x - shift
    return np.concatenate([(d.T @ d).reshape(-1), d.sum(axis=0), [x.shape[0]]])


@pytest.mark.parametrize("name", CASES)
def test_host_fit_from_numpy_moments(pkg, name):
    """reduce.model_from_moments (the host half of fit_pca) on moments formed here in float64: the same model as the
    oracle's two-pass computation, with the bounds the GPU test sets for the device moments."""
    fx, o = fixture(), oracle(name)
    x = fx[f"{name}_x"]
    shift = x[0].astype(np.float64)
    m = pkg.reduce.model_from_moments(_moments(x, shift), shift, int(fx[f"{name}_target"][0]))
    c = kept(name)
    assert m.n_samples_ == x.shape[0] and m.components_.shape == o["components"].shape
    assert (np.abs(m.mean_ - o["mean"]) <= 1e-12 * (1 + np.abs(o["mean"]))).all()
    assert (np.abs(m.scale_ - o["scale"]) <= 1e-12 * (1 + np.abs(o["scale"]))).all()
    assert np.abs(m.explained_variance_ - o["eigenvalues"]).max() <= 1e-10 * o["eigenvalues"][0]
    assert np.abs(m.components_[c] - o["components"][c]).max() <= 1e-6
    assert abs(m.explained_variance_ratio_.sum() - o["eigenvalues"].sum() / o["all_eigenvalues"].sum()) < 1e-12
    assert m.center is None and m.W is None and m.n_components_ == o["components"].shape[0]


def test_error_paths(pkg):
    red = pkg.reduce
    x = fixture()["D_x"]
    shift = x[0].astype(np.float64)
    # fewer than two rows, no valid row
    with pytest.raises(ValueError, match="at least two"):
        red.model_from_moments(_moments(x, shift, rows=[0]), shift, 4)
    with pytest.raises(ValueError, match="no valid row"):
        red.model_from_moments(np.zeros(12 * 12 + 12 + 1), shift, 4)
    with pytest.raises(ValueError):
        red.model_from_moments(np.zeros(7), shift, 4)
    assert red.model_from_moments(_moments(x, shift, rows=[0, 1]), shift, 64).n_components_ == 2
    # a non-fp32 tensor, not 2-D, not a tensor, F > 512, target_dim < 1: ValueError before the device is looked at
    for bad in (torch.zeros(4, 3, dtype=torch.float64), torch.zeros(4, 3, dtype=torch.float16), torch.zeros(5),
                np.zeros((4, 3), np.float32), torch.zeros(4, 513), torch.zeros(4, 0)):
        with pytest.raises(ValueError):
            red.fit_pca(bad)
        with pytest.raises(ValueError):
            red.apply_pca(bad)
    for bad_k in (0, -3, 1.5):
        with pytest.raises(ValueError, match="target_dim"):
            red.fit_pca(torch.zeros(4, 3), target_dim=bad_k)
        with pytest.raises(ValueError, match="target_dim"):
            red.model_from_moments(_moments(x, shift), shift, bad_k)
    with pytest.raises(ValueError, match="counts"):
        red.fit_pca(torch.zeros(4, 3), counts=torch.ones(3, dtype=torch.int32))
    with pytest.raises(ValueError, match="counts"):
        red.fit_pca(torch.zeros(4, 3), counts=torch.ones(4, dtype=torch.int64))
    # a CPU tensor: there is no CPU path
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        red.fit_pca(torch.zeros(4, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        red.apply_pca(torch.zeros(4, 3), torch.ones(4, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        red.pca_dict(["a", "b", "c", "d"], torch.zeros(4, 3), torch.ones(4, dtype=torch.int32))
    model = red.model_from_moments(_moments(x, shift), shift, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        red.transform(model, torch.zeros(4, 12))
    with pytest.raises(ValueError, match="out_dtype"):
        red.transform(model, torch.zeros(4, 12), out_dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        red.pca_dict(["a"], torch.zeros(4, 3), torch.ones(4, dtype=torch.int32))


def test_pca_abi_argument_errors_without_gpu(pkg):
    lib = pkg.load_library()
    buf = np.zeros(64, dtype=np.int64).ctypes.data  # a non-null host address: never dereferenced by the checks
    ws = lib.pg_pca_moments_workspace
    assert ws(1301, 128) > 0 and ws(0, 64) >= 1 and ws(10, 0) == -1 and ws(10, 513) == -1 and ws(-1, 64) == -1
    # the chunking: P = 1301 gives at least three chunks with a ragged last one (256 rows each: 6 chunks, 21 rows last)
    per_chunk = ws(1, 128)
    assert ws(1301, 128) == 6 * per_chunk and ws(1280, 128) == 5 * per_chunk and ws(256, 128) == per_chunk

    def mom(X=buf, ldx=8, P=4, F=8, counts=None, shift=None, out=buf, work=buf, wd=1 << 30):
        return lib.pg_pca_moments_f64(X, ldx, P, F, counts, shift, out, work, wd, None)

    assert mom(P=-1) == -1 and b"negative" in lib.pg_last_error()
    assert mom(F=0) == -1 and mom(F=513, ldx=513) == -1 and b"F=" in lib.pg_last_error()
    assert mom(ldx=7) == -1 and b"ldx" in lib.pg_last_error()
    for kw in (dict(X=None), dict(out=None), dict(work=None)):
        assert mom(**kw) == -1 and b"null" in lib.pg_last_error(), kw
    assert mom(wd=10) == -1 and b"workspace" in lib.pg_last_error()

    def proj(X=buf, ldx=8, P=4, F=8, counts=None, center=buf, W=buf, k=4, out=buf, ldo=4, dt=0):
        return lib.pg_pca_project(X, ldx, P, F, counts, center, W, k, out, ldo, dt, None)

    assert proj(P=-1) == -1 and proj(F=513, ldx=513) == -1 and proj(k=0) == -1 and proj(k=9, ldo=9) == -1
    assert proj(ldx=7) == -1 and proj(ldo=3) == -1 and b"ldo" in lib.pg_last_error()
    assert proj(dt=2) == -1 and b"out_dtype" in lib.pg_last_error()
    for kw in (dict(X=None), dict(center=None), dict(W=None), dict(out=None)):
        assert proj(**kw) == -1 and b"null" in lib.pg_last_error(), kw
    assert proj(P=0, X=None, center=None, W=None, out=None) == 0  # nothing to do
