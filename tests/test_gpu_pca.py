"""PCA reduction on the GPU (reduce.py, pg_pca_moments_f64, pg_pca_project) against the float64 oracle (pca_ref.py),
which tests/test_pca_host.py pins to the reference's recorded outputs (tests/golden/pca_proteins*.npz).

Bounds (none is fitted to what the kernels give):
* fit: mean and scale to 1e-12 (1 + |value|), eigenvalues to 1e-10 lambda_0, components to 1e-6 (float64 eigenvector
  perturbation 2^-53 n lambda_0 / gap with the fixture's gaps >= 1e-7 lambda_0);
* fp32 projection, per element: (F + 4) 2^-24 sum_f (|x_f - c_f| + |c_f|) |W_cf|, evaluated in float64 from the oracle's
  folded center and W: the a-priori bound of an fp32 dot product of length F with fp32-rounded operands;
* fp16 projection: that bound plus half an fp16 ulp of the bounded value, 2^-11 (|oracle| + bound) + 2^-25.
A kept component with eigenvalue <= 1e-8 lambda_0 (case E's null direction; the rank-deficient shapes made here) is
arbitrary: its outputs are only required to be <= 1e-5 in magnitude.
"""
import functools

import numpy as np
import pytest
import torch

from golden_util import load
from pca_ref import CASES, fixture, kept, oracle, pca_oracle, well_separated

pytestmark = pytest.mark.gpu


def bound32(x, o):
    x = np.asarray(x, np.float64)
    c, W = o["center"], o["W"]
    return (x.shape[1] + 4) * 2.0 ** -24 * ((np.abs(x - c) + np.abs(c)) @ np.abs(W).T)


def bound16(x, o, rows=slice(None)):
    b = bound32(x, o)
    return b + 2.0 ** -11 * (np.abs(o["out"][rows]) + b) + 2.0 ** -25


def check_out(got, x, o, what, half=False, rows=slice(None), null_rule=True):
    """got [n, k] against the oracle's rows `rows` (of its out) for the inputs x (those same rows)."""
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    assert got.dtype == (np.float16 if half else np.float32), (what, got.dtype)
    got = got.astype(np.float64)
    want = o["out"][rows]
    assert got.shape == want.shape, (what, got.shape, want.shape)
    # null_rule: leave out the components with eigenvalue <= 1e-8 lambda_0 (False: the fixture's cases but E)
    c = kept(o["eigenvalues"]) if null_rule else np.arange(want.shape[1])
    rest = np.setdiff1d(np.arange(want.shape[1]), c)
    bound = bound16(x, o, rows) if half else bound32(x, o)
    err = np.abs(got - want)
    print(f"{what}: max |got - oracle| / bound = {(err[:, c] / bound[:, c]).max():.3f} over {c.size} components"
          + (f"; |value| on the {rest.size} null ones <= {np.abs(got[:, rest]).max():.2e}" if rest.size else ""))
    assert (err[:, c] <= bound[:, c]).all(), what
    if rest.size:
        assert np.abs(got[:, rest]).max() <= 1e-5, what


def dev(a, cuda):
    return torch.from_numpy(np.array(a)).to(cuda)  # a writable copy: the fixture arrays are read-only


def make_x(seed, P, F, rho, off):
    """The fixture's recipe (tools/golden/make_pca_golden.py) for shapes the fixture does not hold."""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((P, F))
    q, _ = np.linalg.qr(rng.standard_normal((F, F)))
    return (((z * rho ** np.arange(F)) @ q) * rng.uniform(0.5, 2.0, size=F) + off * rng.standard_normal(F)
            ).astype(np.float32)


# shapes at which the kernels take another path than on the fixture:
#   F = 18: no multiple of 4, so per-element loads with a contiguous table; k = 18 leaves the 16-byte stores
#   F = 160, k = 160: more than 128 components: two panels of W (96 + 64), six accumulator tiles per wave
#   F = 512, n = 40: the widest table: 36 super-tile pairs in the moments, W panels of 32 components in more than 64 KiB
#   of LDS, k = 40 in two panels
EXTRA = {"odd18": (11, 301, 18, 18, 0.8, 2.0), "wide160": (12, 400, 160, 160, 0.97, 1.0),
         "max512": (13, 40, 512, 64, 0.99, 1.0)}


@functools.lru_cache(maxsize=None)
def extra(name):
    seed, P, F, target, rho, off = EXTRA[name]
    x = make_x(seed, P, F, rho, off)
    x.setflags(write=False)
    return x, target, pca_oracle(x, target)


@pytest.mark.parametrize("name", CASES)
def test_moments_and_fit(pkg, cuda, name):
    fx, o = fixture(), oracle(name)
    x = fx[f"{name}_x"]
    m = pkg.reduce.fit_pca(dev(x, cuda), target_dim=int(fx[f"{name}_target"][0]))
    lam0 = o["eigenvalues"][0]
    w = fx[f"{name}_eigenvalues"]
    c = kept(w) if name == "E" else np.arange(w.size)
    print(f"{name}: mean {np.abs(m.mean_ - o['mean']).max():.2e} scale {np.abs(m.scale_ - o['scale']).max():.2e} "
          f"eigenvalues {np.abs(m.explained_variance_ - o['eigenvalues']).max() / lam0:.2e} lambda_0 "
          f"components {np.abs(m.components_[c] - o['components'][c]).max():.2e}")
    assert m.n_samples_ == x.shape[0] and m.components_.shape == o["components"].shape
    assert (np.abs(m.mean_ - o["mean"]) <= 1e-12 * (1 + np.abs(o["mean"]))).all()
    assert (np.abs(m.scale_ - o["scale"]) <= 1e-12 * (1 + np.abs(o["scale"]))).all()
    assert np.abs(m.explained_variance_ - o["eigenvalues"]).max() <= 1e-10 * lam0
    assert np.abs(m.components_[c] - o["components"][c]).max() <= 1e-6  # the sign rule included
    big = np.argmax(np.abs(m.components_), axis=1)
    assert (m.components_[np.arange(big.size), big] > 0).all()
    ratio = o["eigenvalues"] / o["all_eigenvalues"].sum()
    assert np.abs(m.explained_variance_ratio_ - ratio).max() <= 1e-10
    assert m.center.dtype == torch.float32 and m.center.device == cuda and m.W.shape == o["components"].shape
    assert np.array_equal(m.center.cpu().numpy(), m.mean_.astype(np.float32))
    assert np.array_equal(m.W.cpu().numpy(), (m.components_ / m.scale_).astype(np.float32))
    # the raw moments against a float64 NumPy product with the same shift
    d = x.astype(np.float64) - x[0].astype(np.float64)
    F = x.shape[1]
    S = m.moments_[:F * F].reshape(F, F)
    assert np.array_equal(S, S.T) and m.moments_[-1] == x.shape[0]
    # two float64 sums of n terms in different orders: each within n 2^-53 sum |terms| of the exact value
    u2n = 2 * x.shape[0] * 2.0 ** -53
    assert (np.abs(S - d.T @ d) <= u2n * (np.abs(d).T @ np.abs(d))).all()
    assert (np.abs(m.moments_[F * F:F * F + F] - d.sum(axis=0)) <= u2n * np.abs(d).sum(axis=0)).all()
    if name == "D":
        assert m.scale_[5] == 1.0 and m.mean_[5] == 3.25 and not S[5].any()  # the constant column


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
def test_projection(pkg, cuda, name, half):
    fx, o = fixture(), oracle(name)
    x = fx[f"{name}_x"]
    out, m = pkg.reduce.apply_pca(dev(x, cuda), target_dim=int(fx[f"{name}_target"][0]),
                                  out_dtype=torch.float16 if half else torch.float32)
    assert out.device == cuda and out.is_contiguous()
    check_out(out, x, o, f"{name} {'fp16' if half else 'fp32'}", half=half, null_rule=name == "E")


@pytest.mark.parametrize("name", list(EXTRA))
def test_other_kernel_paths(pkg, cuda, name):
    x, target, o = extra(name)
    xd = dev(x, cuda)
    for half in (False, True):
        out, m = pkg.reduce.apply_pca(xd, target_dim=target, out_dtype=torch.float16 if half else torch.float32)
        check_out(out, x, o, f"{name} {'fp16' if half else 'fp32'}", half=half)
    lam0 = o["eigenvalues"][0]
    assert (np.abs(m.mean_ - o["mean"]) <= 1e-12 * (1 + np.abs(o["mean"]))).all()
    assert (np.abs(m.scale_ - o["scale"]) <= 1e-12 * (1 + np.abs(o["scale"]))).all()
    assert np.abs(m.explained_variance_ - o["eigenvalues"]).max() <= 1e-10 * lam0
    if name == "max512":  # a row mask across the widest table, and zeros written across two panels
        cnt = np.ones(x.shape[0], np.int32)
        cnt[[0, 7, 39]] = 0
        keep = np.flatnonzero(cnt)
        o2 = pca_oracle(x[keep], target)
        out, _ = pkg.reduce.apply_pca(xd, dev(cnt, cuda), target_dim=target, out_dtype=torch.float32)
        check_out(out[dev(keep, cuda)], x[keep], o2, "max512 masked")
        assert not out.cpu().numpy()[cnt == 0].view(np.uint32).any()


def test_masking_and_layout_case_f(pkg, cuda):
    fx, o = fixture(), oracle("F")
    red = pkg.reduce
    pooled_h, counts_h, rows = fx["A_x"], fx["F_counts"], fx["F_rows"]
    ids = [str(s) for s in fx["F_ids"]]
    id_map = {str(a): str(b) for a, b in zip(fx["F_id_map_from"], fx["F_id_map_to"])}
    pooled, counts = dev(pooled_h, cuda), dev(counts_h, cuda)
    xf = fx["F_x"]
    # the dict's rows as a mask over the uncompacted table, against the compacted input
    mask_h = np.zeros(pooled_h.shape[0], np.int32)
    mask_h[rows] = 1
    mask = dev(mask_h, cuda)
    rows_d = dev(rows, cuda)
    for half in (False, True):
        dt = torch.float16 if half else torch.float32
        masked, mm = red.apply_pca(pooled, mask, out_dtype=dt)
        compact, mc = red.apply_pca(dev(xf, cuda), out_dtype=dt)
        assert mm.n_samples_ == mc.n_samples_ == rows.size
        check_out(masked[rows_d], xf, o, f"F masked {dt}", half=half, null_rule=False)
        check_out(compact, xf, o, f"F compacted {dt}", half=half, null_rule=False)
        skipped = masked.cpu().numpy()[mask_h == 0]
        assert skipped.shape[0] == pooled_h.shape[0] - rows.size
        assert not skipped.view(np.uint16 if half else np.uint32).any(), "skipped rows are +0.0"
    # the model does not depend on where the rows stand
    assert np.abs(mm.mean_ - mc.mean_).max() <= 1e-12 and np.abs(mm.explained_variance_ - mc.explained_variance_).max() \
        <= 1e-10 * mc.explained_variance_[0]
    # the reference's Step 5 on (ids, pooled, counts): its recorded key order, float16 vectors
    d = red.pca_dict(ids, pooled, counts, target_dim=64, id_map=id_map, random_seed=42)
    assert list(d) == [str(s) for s in fx["F_keys"]]
    got = np.stack(list(d.values()))
    check_out(got, xf, o, "F pca_dict fp16", half=True, null_rule=False)
    # against the reference's own float16 vectors, by the triangle inequality, on the well-separated components: the
    # bound above, the host test's 1e-5 of the column's largest |value| between the reference's float32 result and the
    # oracle, and the reference's own rounding of that result to float16
    ref16, ref32 = fx["F_ref16"].astype(np.float64), np.abs(fx["F_ref32"].astype(np.float64))
    well = well_separated(fx["F_all_eigenvalues"], 64)
    assert well.size >= 7
    tri = bound16(xf, o) + 1e-5 * np.abs(o["out"]).max(axis=0) + 2.0 ** -11 * ref32
    dist = np.abs(got.astype(np.float64) - ref16)
    print(f"F pca_dict: max |got - reference fp16| = {dist.max():.3e} over all components (the reference took "
          f"scikit-learn's solver {fx['F_solver']}); on the {well.size} well-separated ones "
          f"{(dist / tri)[:, well].max():.3f} of the triangle bound")
    assert (dist[:, well] <= tri[:, well]).all()
    d32 = red.pca_dict(ids, pooled, counts, id_map=id_map, output_dtype=np.float32)
    check_out(np.stack(list(d32.values())), xf, o, "F pca_dict fp32", null_rule=False)
    # a view with row stride F + 3: the per-element loads
    wide = torch.zeros(pooled_h.shape[0], 64 + 3, device=cuda)
    view = wide[:, :64]
    view.copy_(pooled)
    assert view.stride(0) == 67 and not view.is_contiguous()
    for half in (False, True):
        out, _ = red.apply_pca(view, mask, out_dtype=torch.float16 if half else torch.float32)
        check_out(out[rows_d], xf, o, f"F stride 67 half={half}", half=half, null_rule=False)


def test_case_b_odd_row_stride(pkg, cuda):
    fx, o = fixture(), oracle("B")
    x = fx["B_x"]
    wide = torch.full((x.shape[0], 23), float("nan"), device=cuda)  # the padding is never read
    view = wide[:, :20]
    view.copy_(dev(x, cuda))
    assert view.stride(0) == 23
    for half in (False, True):
        out, m = pkg.reduce.apply_pca(view, target_dim=7, out_dtype=torch.float16 if half else torch.float32)
        assert out.shape == (x.shape[0], 7)
        check_out(out, x, o, f"B stride 23 half={half}", half=half, null_rule=False)
    assert (np.abs(m.mean_ - o["mean"]) <= 1e-12 * (1 + np.abs(o["mean"]))).all()
    assert np.abs(m.components_ - o["components"]).max() <= 1e-6


def test_transform_with_a_fitted_model(pkg, cuda):
    x = fixture()["A_x"]
    o = pca_oracle(x, 64, fit_rows=slice(0, 400))
    m = pkg.reduce.fit_pca(dev(x[:400], cuda), target_dim=64)
    assert m.n_samples_ == 400
    rest = slice(400, 643)
    for half in (False, True):
        out = pkg.reduce.transform(m, dev(x[400:], cuda), out_dtype=torch.float16 if half else torch.float32)
        assert out.shape == (243, 64)
        check_out(out, x[400:], o, f"transform half={half}", half=half, rows=rest, null_rule=False)
    with pytest.raises(ValueError):
        pkg.reduce.transform(m, torch.zeros(4, 20, device=cuda))


def test_reproducible_bits(pkg, cuda):
    x = dev(fixture()["C_x"], cuda)
    a, b = pkg.reduce.fit_pca(x), pkg.reduce.fit_pca(x)
    assert np.array_equal(a.moments_.view(np.uint64), b.moments_.view(np.uint64))
    assert torch.equal(a.W.view(torch.int32), b.W.view(torch.int32))
    oa, _ = pkg.reduce.apply_pca(x)
    ob, _ = pkg.reduce.apply_pca(x)
    assert oa.dtype == torch.float16 and torch.equal(oa.view(torch.int16), ob.view(torch.int16))
    cnt = torch.ones(x.size(0), dtype=torch.int32, device=cuda)
    cnt[5::9] = 0
    ma, mb = pkg.reduce.fit_pca(x, cnt), pkg.reduce.fit_pca(x, cnt)
    assert np.array_equal(ma.moments_.view(np.uint64), mb.moments_.view(np.uint64))
    assert ma.n_samples_ == int(cnt.sum())


def test_fewer_than_two_valid_rows(pkg, cuda):
    x = dev(fixture()["D_x"], cuda)
    cnt = torch.zeros(x.size(0), dtype=torch.int32, device=cuda)
    with pytest.raises(ValueError, match="no valid row"):
        pkg.reduce.fit_pca(x, cnt)
    cnt[17] = 3
    with pytest.raises(ValueError, match="at least two"):
        pkg.reduce.apply_pca(x, cnt)
    with pytest.raises(ValueError, match="at least two"):
        pkg.reduce.fit_pca(x[:1])
    cnt[200] = 1
    assert pkg.reduce.fit_pca(x, cnt).n_components_ == 2


def test_end_of_the_pipeline(pkg, cuda):
    """pool.pool_proteins on the committed pooling fixture, then reduce.apply_pca on its (pooled, counts): the table
    stays on the device in between."""
    fx = load("pool_proteins")
    seqs = [str(s) for s in fx["seqs"]]
    n = 2
    t = pkg.ngram.transitions_from_table(n, [], [], [], [str(s) for s in fx[f"n{n}_nodes"]], device=cuda)
    pooled, counts = pkg.pool.pool_proteins(seqs, t, dev(fx[f"n{n}_emb"], cuda))
    assert pooled.device == cuda and counts.device == cuda
    reduced, m = pkg.reduce.apply_pca(pooled, counts, target_dim=64)
    assert reduced.device == cuda and reduced.dtype == torch.float16
    have = counts.cpu().numpy() > 0
    assert have.sum() >= 2 and (~have).sum() >= 1
    x = pooled.cpu().numpy()[have]
    o = pca_oracle(x, 64)
    assert m.n_samples_ == have.sum() and reduced.shape == (len(seqs), min(64, x.shape[1], x.shape[0]))
    check_out(reduced.cpu().numpy()[have], x, o, "pooled fixture fp16", half=True)
    assert not reduced.cpu().numpy()[~have].view(np.uint16).any()
    d = pkg.reduce.pca_dict([str(s) for s in fx["ids"]], pooled, counts)
    want = pkg.pool.pooled_dict([str(s) for s in fx["ids"]], pooled, counts)
    assert list(d) == list(want) and all(v.dtype == np.float16 and v.shape == (reduced.shape[1],) for v in d.values())
