"""PCA reduction of the pooled protein table on the GPU: the reference's Step 5
(``protgram_directgcn_trainer.py:411-421``; ``EmbeddingProcessor.apply_pca``, ``src/utils/models_utils.py:88-136``), on
by default there (``config.py:107-108``: 64 dimensions) and the representation every downstream consumer reads.

The reference stacks the proteins that have a vector as float32 [n, F], sets k = min(target_dim, F, n), runs
``StandardScaler().fit_transform`` (column mean and population variance; a column that scikit-learn's
``_is_constant_feature`` calls constant keeps scale 1), then ``PCA(n_components=k).fit_transform`` -- for n >= 10 F the
``covariance_eigh`` solver: eigen-decomposition of the sample covariance (divisor n - 1), descending eigenvalues, every
component's largest-magnitude entry made positive (``svd_flip``, v-based), projection of the centred data -- and casts
to float16. That is exact PCA of the correlation matrix, and this module computes the same thing:

* ``pg_pca_moments_f64`` streams the table once and accumulates sum (x - s)(x - s)^T, sum (x - s) and n in float64
  (s: the first valid row, so that a common offset does not cancel);
* the F x F statistics come to the host (the only synchronisation of ``fit_pca``), where mean, scale, the correlation
  form of the covariance, ``numpy.linalg.eigh``, the order and the signs are derived in float64;
* standardisation, centring and signs are folded into ``center`` [F] and ``W`` [k, F] (fp32, on the device), and
  ``pg_pca_project`` streams the table a second time: out = (x - center) W^T, fp32 accumulation, one rounding to fp16.

The reference's float32 rounding order is not reproduced (it rounds the scaled matrix to float32 and forms the
covariance from that); the result agrees with it to float32 accuracy on components whose eigenvalues are separated.
Two deviations: ``random_seed`` is accepted and ignored (the exact solvers do not use it), and fewer than two valid
rows raise ``ValueError`` (the reference returns zeros for n = 1 through a 0/0 that scikit-learn swallows).
scikit-learn's ``randomized`` solver (n < 10 F with k < 0.8 min(n, F)) is not reproduced: always the exact decomposition.
There is no CPU path.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Dict, Iterable, List, Optional, Tuple

import numpy as np
import torch

from ._lib import check, load_library
from .pool import _need_cuda, _stream, _vp

MAX_FEATURES = 512  # pg_pca_moments_f64 / pg_pca_project take 1 <= F <= 512
_EPS = float(np.finfo(np.float64).eps)


@dataclass
class PCAModel:
    """A fitted reduction. The float64 attributes carry scikit-learn's names: ``mean_`` / ``scale_`` are the
    StandardScaler's, the others PCA's (of the scaled data). ``center`` [F] and ``W`` [k, F] are the folded fp32 device
    tensors ``transform`` uses; ``moments_`` is the raw float64 buffer of ``pg_pca_moments_f64`` (F*F + F + 1)."""
    mean_: np.ndarray
    scale_: np.ndarray
    components_: np.ndarray
    explained_variance_: np.ndarray
    explained_variance_ratio_: np.ndarray
    n_samples_: int
    center: Optional[torch.Tensor] = None
    W: Optional[torch.Tensor] = None
    moments_: Optional[np.ndarray] = None

    @property
    def n_components_(self) -> int:
        return int(self.components_.shape[0])

    @property
    def n_features_(self) -> int:
        return int(self.components_.shape[1])


def _check_target(target_dim) -> int:
    if int(target_dim) != target_dim or int(target_dim) < 1:
        raise ValueError(f"target_dim must be an integer >= 1 (got {target_dim!r})")
    return int(target_dim)


def _check_pooled(pooled, counts) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """As pool._check_table: fp32, 2-D, on the GPU; a view with unit column stride and row stride >= F is taken as
    it is. counts: int32 [P] on the same device."""
    if not torch.is_tensor(pooled) or pooled.dim() != 2:
        raise ValueError("pooled must be a [P, F] tensor")
    if pooled.dtype != torch.float32:
        raise ValueError("pooled must be float32 (pool_proteins' output)")
    P, F = pooled.shape
    if F < 1 or F > MAX_FEATURES:
        raise ValueError(f"pooled must have 1 <= F <= {MAX_FEATURES} columns (F = {F})")
    if counts is not None:
        if not torch.is_tensor(counts) or counts.dim() != 1 or counts.numel() != P:
            raise ValueError("counts must be a [P] tensor, one entry per row of pooled")
        if counts.dtype != torch.int32:
            raise ValueError("counts must be int32 (pool_proteins' output)")
    _need_cuda(pooled.device, "PCA reduction")
    if counts is not None and counts.device != pooled.device:
        raise ValueError("counts must be on pooled's device")
    if (F > 1 and pooled.stride(1) != 1) or (P > 1 and pooled.stride(0) < F):
        pooled = pooled.contiguous()
    return pooled, (counts.contiguous() if counts is not None else None)


def _ldx(t: torch.Tensor) -> int:
    return t.stride(0) if t.size(0) > 1 else t.size(1)


def model_from_moments(moments: np.ndarray, shift: np.ndarray, target_dim: int) -> PCAModel:
    """The host part of the fit, float64 NumPy: `moments` is pg_pca_moments_f64's buffer (S = sum (x - s)(x - s)^T
    row-major, then sum (x - s), then n) for the shift s. Raises ValueError for fewer than two rows."""
    target_dim = _check_target(target_dim)
    shift = np.asarray(shift, dtype=np.float64)
    F = shift.size
    moments = np.asarray(moments, dtype=np.float64)
    if moments.size != F * F + F + 1:
        raise ValueError("moments must hold F*F + F + 1 values")
    n = int(round(moments[-1]))
    if n < 1:
        raise ValueError("PCA needs at least two proteins with a vector: no valid row")
    if n < 2:
        raise ValueError("PCA needs at least two proteins with a vector (n = 1)")
    k = min(target_dim, F, n)
    d = moments[F * F:F * F + F] / n
    mean = shift + d
    # sum (x - mean)(x - mean)^T = S - n d d^T; made exactly symmetric
    css = moments[:F * F].reshape(F, F) - n * np.outer(d, d)
    css = 0.5 * (css + css.T)
    var = np.maximum(np.diag(css), 0.0) / n
    # StandardScaler's scale: sqrt(var), 1 for a column that is constant within the error bound of the variance
    # computation (_is_constant_feature, scikit-learn 1.7 sklearn/preprocessing/_data.py:85-100, applied through
    # _handle_zeros_in_scale in StandardScaler.partial_fit)
    constant = var <= n * _EPS * var + (n * mean * _EPS) ** 2
    scale = np.sqrt(var)
    scale[constant] = 1.0
    # covariance of the scaled data, divisor n - 1 (PCA._fit_full, covariance_eigh branch, sklearn/decomposition/_pca.py)
    cov = css / np.outer(scale, scale) / (n - 1)
    w, v = np.linalg.eigh(cov)
    w, v = w[::-1].copy(), v[:, ::-1]
    w[w < 0.0] = 0.0
    comps = np.ascontiguousarray(v.T[:k])
    # svd_flip(u_based_decision=False): the largest-magnitude entry of each component is positive
    big = np.argmax(np.abs(comps), axis=1)
    sign = np.sign(comps[np.arange(k), big])
    sign[sign == 0] = 1.0
    comps *= sign[:, None]
    total = w.sum()
    return PCAModel(mean_=mean, scale_=scale, components_=comps, explained_variance_=w[:k].copy(),
                    explained_variance_ratio_=w[:k] / total if total > 0 else np.zeros(k), n_samples_=n,
                    moments_=moments.copy())


def fit_pca(pooled: torch.Tensor, counts: Optional[torch.Tensor] = None, target_dim: int = 64) -> PCAModel:
    """Fit on the rows of pooled [P, F] (fp32, on the GPU) with counts[r] > 0 (counts None: all rows); the pair is
    what pool.pool_proteins returns. k = min(target_dim, F, n). One host synchronisation (the F*F + F + 1 moments
    and the shift row come back in one copy)."""
    target_dim = _check_target(target_dim)
    pooled, counts = _check_pooled(pooled, counts)
    dev = pooled.device
    P, F = pooled.shape
    if P < 1:
        raise ValueError("PCA needs at least two proteins with a vector: no valid row")
    lib = load_library()
    # the shift: the first valid row (row 0 when there is none; the host raises then)
    first = torch.argmax((counts > 0).to(torch.int8)) if counts is not None else torch.zeros((), dtype=torch.int64,
                                                                                               device=dev)
    shift = pooled.index_select(0, first.reshape(1)).reshape(F).contiguous()
    need = int(lib.pg_pca_moments_workspace(P, F))
    if need < 0:
        raise ValueError(f"pg_pca_moments_workspace does not take P = {P}, F = {F}")
    work = torch.empty(need, dtype=torch.float64, device=dev)
    buf = torch.empty(F * F + F + 1 + F, dtype=torch.float64, device=dev)
    check(lib.pg_pca_moments_f64(_vp(pooled), _ldx(pooled), P, F, _vp(counts), _vp(shift), _vp(buf), _vp(work), need,
                                 _stream(dev)), "pg_pca_moments_f64")
    buf[F * F + F + 1:] = shift
    host = buf.cpu().numpy()
    model = model_from_moments(host[:F * F + F + 1], host[F * F + F + 1:], target_dim)
    model.center = torch.from_numpy(model.mean_.astype(np.float32)).to(dev)
    model.W = torch.from_numpy((model.components_ / model.scale_).astype(np.float32)).to(dev).contiguous()
    return model


def transform(model: PCAModel, pooled: torch.Tensor, counts: Optional[torch.Tensor] = None,
              out_dtype: torch.dtype = torch.float16) -> torch.Tensor:
    """[P, k] on the device: (pooled - center) W^T for the rows with counts[r] > 0, zeros for the others. The model may
    come from another protein set with the same F."""
    if out_dtype not in (torch.float16, torch.float32):
        raise ValueError("out_dtype must be torch.float16 or torch.float32")
    pooled, counts = _check_pooled(pooled, counts)
    dev = pooled.device
    P, F = pooled.shape
    if model.center is None or model.W is None:
        raise ValueError("the model has no device tensors (fit it with fit_pca)")
    if model.n_features_ != F:
        raise ValueError(f"the model was fitted on F = {model.n_features_} columns, pooled has {F}")
    if model.center.device != dev:
        raise ValueError("the model is on another device than pooled")
    k = model.n_components_
    out = torch.empty(P, k, dtype=out_dtype, device=dev)
    if P:
        check(load_library().pg_pca_project(_vp(pooled), _ldx(pooled), P, F, _vp(counts), _vp(model.center),
                                            _vp(model.W), k, _vp(out), k, 0 if out_dtype == torch.float16 else 1,
                                            _stream(dev)), "pg_pca_project")
    return out


def apply_pca(pooled: torch.Tensor, counts: Optional[torch.Tensor] = None, target_dim: int = 64,
              out_dtype: torch.dtype = torch.float16) -> Tuple[torch.Tensor, PCAModel]:
    """fit_pca, then transform of the same rows: (reduced [P, k] on the device, model)."""
    model = fit_pca(pooled, counts, target_dim)
    return transform(model, pooled, counts, out_dtype), model


def dict_rows(protein_ids: Iterable[str], counts, id_map: Optional[Dict[str, str]] = None
              ) -> Tuple[List[str], np.ndarray]:
    """(keys, rows) of the reference's dict after the pooling step (pool.pooled_dict): per surviving key, in dict
    order, the row of the pooled table whose vector it holds. Proteins with count 0 are absent; a later duplicate id
    replaces an earlier one's row but keeps its position, before and after the keys are mapped with id_map.get(k, k)."""
    cnt = counts.detach().cpu().numpy() if torch.is_tensor(counts) else np.asarray(counts)
    protein_ids = list(protein_ids)
    if cnt.ndim != 1 or cnt.shape[0] != len(protein_ids):
        raise ValueError("protein_ids and counts must have one entry per protein")
    rows: Dict[str, int] = {}
    for i, pid in enumerate(protein_ids):
        if cnt[i] > 0:
            rows[pid] = i
    if id_map:
        rows = {id_map.get(k, k): v for k, v in rows.items()}
    return list(rows), np.fromiter(rows.values(), dtype=np.int64, count=len(rows))


def pca_dict(protein_ids: Iterable[str], pooled: torch.Tensor, counts: torch.Tensor, target_dim: int = 64,
             id_map: Optional[Dict[str, str]] = None, random_seed=None, output_dtype=np.float16
             ) -> Dict[str, np.ndarray]:
    """The reference's Step 5 on the result of pool.pool_proteins: what
    EmbeddingProcessor.apply_pca(pool.pooled_dict(protein_ids, pooled, counts, id_map), target_dim, random_seed,
    output_dtype) returns, {id: reduced vector} in dict order. The rows the dict would hold are passed to the kernels
    as a mask; the table is not compacted. random_seed is ignored (module docstring)."""
    del random_seed
    protein_ids = list(protein_ids)
    if not torch.is_tensor(pooled) or pooled.dim() != 2 or len(protein_ids) != pooled.size(0):
        raise ValueError("protein_ids and pooled must have one entry per protein")
    keys, rows = dict_rows(protein_ids, counts, id_map)
    mask = np.zeros(len(protein_ids), dtype=np.int32)
    mask[rows] = 1
    np_dtype = np.dtype(output_dtype)
    dev_dtype = torch.float16 if np_dtype == np.float16 else torch.float32
    reduced, _ = apply_pca(pooled, torch.from_numpy(mask).to(pooled.device), target_dim, dev_dtype)
    host = reduced.cpu().numpy()
    return {key: host[r].astype(np_dtype, copy=True) for key, r in zip(keys, rows)}
