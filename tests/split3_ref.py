"""Host model of the split-bf16 dense kernels (csrc/pg_split3.h) and the bounds their accuracy tests assert.

The fp32 dense path splits every fp32 operand exactly into three bf16 values, v = v0 + v1 + v2, and sums the six
products a_i w_j with i + j <= 2 in fp32, one MFMA k-step at a time. This module restates that scheme on the CPU
(`split3`, `gemm_split`), together with the eight one-line slips that would turn it into a ~16-bit kernel (`MUTANTS`),
and derives for every test case (`CASES`) the bound that tests/test_gpu_split_accuracy.py asserts on the GPU
(`bounds`). tests/test_split3_host.py checks, without a GPU, that this bound separates the correct scheme from every
mutant by at least 2x on either side.

The error metric is componentwise: e = |got - ref64| / den, where ref64 is the layer's formula in float64 and den the
same formula with every operand and every product replaced by its absolute value (for a bare GEMM: |A| |W|^T). A row
that holds magnitudes many powers of two apart is then judged against what was actually summed. rms(e) and max(e)
are reported and bounded separately.

The bound of a case is the geometric mean of (b) the host model's metric with the correct six products and (c) the
smallest metric over the eight mutants, both measured on the case's own operands: it comes from the scheme and the
operands, never from the code under test, and holds no hand-picked constant.
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

# the six products of a split pair (a_i, w_j), in pg_split3.h's order (small terms first)
SIX = [(2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0)]

MUTANTS = {f"no a{i} w{j}": [t for t in SIX if t != (i, j)] for (i, j) in SIX}
MUTANTS["a1 w0 for a0 w1"] = [(1, 0) if t == (0, 1) else t for t in SIX]
# a two-way split (v0, v1 alone) with its three products: the three-way split's first two pieces are the two-way's
MUTANTS["two-way split"] = [(1, 0), (0, 1), (0, 0)]
# the second-order terms: the slips the suite's earlier |d| <= 2e-5 + 2e-5 |ref| cannot see
SECOND_ORDER = ["no a2 w0", "no a1 w1", "no a0 w2"]

KSTEP_FWD = 32   # v_mfma_f32_16x16x32_bf16 (dense_x3p_kernel, dense_x3_kernel)
KSTEP_BWD = 16   # v_mfma_f32_32x32x16_bf16 (dgrad_x3_kernel, dgrad_span_kernel, wgrad_x3_kernel)
WX_K = 16        # rows per wgrad_x3_kernel step (pg_dense_bwd.hip)


def _bf(x: torch.Tensor) -> torch.Tensor:
    return x.to(torch.bfloat16).to(torch.float32)  # round-to-nearest-even


def split3(x: torch.Tensor):
    """The exact three-way bf16 split of an fp32 tensor (pgx3::split8 / split4): three fp32 tensors that hold bf16
    values, x0 + x1 + x2 == x bit for bit."""
    assert x.dtype == torch.float32
    x0 = _bf(x)
    r = x - x0
    x1 = _bf(r)
    r2 = r - x1
    x2 = _bf(r2)
    assert torch.equal(x2, r2), "the third piece is not a bf16"
    assert torch.equal(x0.double() + x1.double() + x2.double(), x.double()), "split3 is not exact"
    assert torch.equal((x0 + x1) + x2, x)
    return x0, x1, x2


def _splits(x):
    return x if isinstance(x, tuple) else split3(x.contiguous())


def gemm_split(A, W, terms, kstep: int) -> torch.Tensor:
    """sum over (i, j) in `terms` of A_i W_j^T as the split-bf16 kernels accumulate it: A [M, K] and W [N, K] (fp32,
    or their split3 tuples); every kstep-deep slice of every term is summed exactly (float64 holds the 16-bit
    products' sums) and then added into the fp32 accumulator, slice after slice, the terms of a slice in list order."""
    As, Ws = _splits(A), _splits(W)
    Ad = [a.double() for a in As]
    Wd = [w.double().t().contiguous() for w in Ws]
    M, K = As[0].shape
    acc = torch.zeros(M, Ws[0].shape[0], dtype=torch.float32)
    for k0 in range(0, K, kstep):
        for (i, j) in terms:
            acc = (acc.double() + Ad[i][:, k0:k0 + kstep] @ Wd[j][k0:k0 + kstep]).float()
    return acc


def metric(got: torch.Tensor, ref64: torch.Tensor, den: torch.Tensor, mask: Optional[torch.Tensor] = None):
    """(rms, max) of e = |got - ref64| / den over every element (den == 0: the element must be exact), or over the
    elements of `mask` (the fused dropout's kept elements; the dropped ones are checked to be exactly 0 instead)."""
    d = (got.double() - ref64).abs()
    e = torch.where(den > 0, d / den.clamp_min(1e-300), torch.where(d == 0, 0.0, math.inf).double())
    if mask is not None:
        e = e[mask]
    return float(e.pow(2).mean().sqrt()), float(e.max())


def _f(x64: torch.Tensor) -> torch.Tensor:
    return x64.float()  # one fp32 rounding of a float64 value


def _fma(a, b, c):  # fl(a b + c): the product of two fp32 values is exact in float64
    return _f(a.double() * b.double() + c.double())


# ---------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    kind: str            # "fwd" | "dgrad" | "wgrad" | "span"
    M: int
    F_in: int
    F_out: int
    proj: bool = False   # projected residual (W_res): a fourth K segment
    vec: bool = True     # vector gates (+ constant and identity residual in the forward); False: scalar gates, neither
    pre: bool = False    # forward: the operand is the pre-gated s_q Z_q (PG_FLAG_DENSE_PREGATED)
    wide: bool = False   # operand columns / weight rows scaled by 2^[-12, 12]
    drop: float = 0.0    # forward: fused dropout p
    e_res: bool = False  # span: E includes dpre
    seed: int = 0

    @property
    def id(self) -> str:
        s = f"{self.kind}-M{self.M}-{self.F_in}x{self.F_out}"
        for flag, name in ((self.proj, "proj"), (not self.vec, "scalar"), (self.pre, "pregated"), (self.wide, "wide"),
                           (self.drop > 0, "drop"), (self.e_res, "eres")):
            if flag:
                s += "-" + name
        return s


FWD_X3P = [Case("fwd", M, 128, 128, vec=vec, pre=pre, seed=11 + M + 2 * vec + pre)
           for M in (17, 257) for vec in (True, False) for pre in (False, True)]
# 257 tiles: with at most 256 compute units one workgroup runs two tiles through the software pipeline
FWD_X3P.append(Case("fwd", 4099, 128, 128, seed=23))
FWD_DROP = Case("fwd", 257, 128, 128, drop=0.3, seed=29)
FWD_X3 = [Case("fwd", M, 64, 128, proj=True, pre=pre, seed=31 + M + pre) for M in (33, 257) for pre in (False, True)]
FWD_WIDE = Case("fwd", 257, 128, 128, vec=False, wide=True, seed=41)
DGRAD = [Case("dgrad", 257, 128, 128, seed=51), Case("dgrad", 257, 64, 128, proj=True, seed=52),
         Case("dgrad", 300, 32, 32, seed=53), Case("dgrad", 257, 128, 128, wide=True, seed=54)]
WGRAD = [Case("wgrad", 257, 128, 128, seed=61), Case("wgrad", 4099, 128, 128, seed=62)]
SPAN = [Case("span", 257, 128, 128, e_res=False, seed=71), Case("span", 257, 128, 128, e_res=True, seed=72)]
CASES = FWD_X3P + [FWD_DROP] + FWD_X3 + [FWD_WIDE] + DGRAD + WGRAD + SPAN

DROP_SEED = 0x0123_4567_89AB_CDEF

_W_KEYS = ("W_main_in", "W_main_out", "W_undirected", "W_shared")
_B_KEYS = ("b_main_in", "b_dir_shared_in", "b_main_out", "b_dir_shared_out", "b_undirected", "b_undirected_shared")
_C_KEYS = ("C_in", "C_out", "C_directed", "C_undirected", "C_all")


@functools.lru_cache(maxsize=None)
def operands(case: Case) -> dict:
    """The case's fp32 operands on the CPU, from its seed (the GPU test uploads exactly these). Never modified."""
    g = torch.Generator().manual_seed(case.seed)
    M, Fi, Fo = case.M, case.F_in, case.F_out
    o = {"Z": torch.randn(M, 3 * Fi, generator=g)}
    prm = {k: torch.randn(Fo, Fi, generator=g) * 0.1 for k in _W_KEYS}
    for k in _B_KEYS:
        prm[k] = torch.randn(Fo, generator=g) * 0.1
    for k in _C_KEYS:
        prm[k] = torch.rand((M, 1) if case.vec else (1,), generator=g) + 0.5
    o["W_res"] = torch.randn(Fo, Fi, generator=g) * 0.1 if case.proj else None
    o["b_res"] = torch.randn(Fo, generator=g) * 0.1 if case.proj else None
    o["res_x"] = torch.randn(M, Fi, generator=g) if (case.proj or (case.vec and Fi == Fo)) else None
    o["constant"] = torch.randn(M, Fo, generator=g) if case.vec else None
    o["dY"] = torch.randn(M, Fo, generator=g)
    o["wdiag"] = torch.rand(M, 3, generator=g) + 0.5
    if case.wide:
        # powers of two: every split stays exact and every product keeps its significand; only the exponents spread
        r = torch.exp2(torch.randint(-12, 13, (Fi,), generator=g).float())   # column k of every Z segment
        q = torch.exp2(torch.randint(-12, 13, (Fo,), generator=g).float())   # row j of every W (and its biases)
        if case.kind == "fwd":
            o["Z"] = o["Z"] * r.repeat(3)
            for k in _W_KEYS:
                prm[k] = prm[k] * q[:, None]
            for k in _B_KEYS:
                prm[k] = prm[k] * q
        else:
            o["dY"] = o["dY"] * q
    if case.kind == "fwd" and case.wide:
        assert o["constant"] is None and o["res_x"] is None  # nothing unscaled is added to the scaled columns
    o["prm"] = prm
    s = gates32(prm, M)
    if case.pre:  # what pg_spmm3_gated_f32 stores: fl(s_q Z_q)
        o["Z"] = torch.cat([o["Z"][:, k * Fi:(k + 1) * Fi] * s[k] for k in range(3)], 1)
    return o


def gates32(prm: dict, M: int):
    """s_in, s_out, s_und [M, 1] as every kernel rounds them: fl(fl(c_all c_dir) c_in), ..., fl(c_all c_und)."""
    c = {k: prm[k].expand(M, 1) if prm[k].numel() == 1 else prm[k] for k in _C_KEYS}
    cad = c["C_all"] * c["C_directed"]
    return [cad * c["C_in"], cad * c["C_out"], c["C_all"] * c["C_undirected"]]


def gates64(prm: dict, M: int):
    c = {k: (prm[k].expand(M, 1) if prm[k].numel() == 1 else prm[k]).double() for k in _C_KEYS}
    return [c["C_all"] * c["C_directed"] * c["C_in"], c["C_all"] * c["C_directed"] * c["C_out"],
            c["C_all"] * c["C_undirected"]]


def drop_scale(p: float) -> float:
    """pg::drop_params' scale: the ABI carries p as a float."""
    return float(np.float32(1.0 / (1.0 - float(np.float32(p)))))


def drop_keep(case: Case) -> Optional[torch.Tensor]:
    """The fused dropout's kept elements [M, F_out] (the kernel's counter-based draw, restated on the host by
    test_gpu_parity._layer_drop_keep); None without dropout."""
    if case.drop <= 0:
        return None
    from test_gpu_parity import _layer_drop_keep
    return _layer_drop_keep(DROP_SEED, case.M, case.F_out, case.drop)


def plan_of_x3w(M: int, F_in: int, F_out: int):
    """(splits, rows_per_split) of wgrad_x3_kernel (plan_of, pg_dense_bwd.hip; no projected residual)."""
    tiles = (F_out // 128) * ((3 * F_in) // 384)
    steps = max((M + WX_K - 1) // WX_K, 1)
    splits = min(max((256 + tiles - 1) // tiles, 1), steps)
    rows = ((steps + splits - 1) // splits) * WX_K
    return max((M + rows - 1) // rows, 1), rows


def reduce_splits(parts):
    """reduce_splits_kernel's fixed order in fp32: eight groups, each two alternating chains over every 8th split,
    then the groups in order."""
    n = len(parts)
    zero = torch.zeros_like(parts[0])
    groups = []
    for grp in range(8):
        s0, s1, k = zero, zero, grp
        while k + 8 < n:
            s0 = s0 + parts[k]
            s1 = s1 + parts[k + 8]
            k += 16
        if k < n:
            s0 = s0 + parts[k]
        groups.append(s0 + s1)
    t = groups[0]
    for g in groups[1:]:
        t = t + g
    return t


# ---------------------------------------------------------------------------------------------------------
# the formulas: float64 reference + normaliser, torch fp32, and the host model of the kernels
# ---------------------------------------------------------------------------------------------------------
def _packed(case: Case, o: dict, dtype):
    """[W_in + W_s | W_out + W_s | W_und + W_s (| W_res)] [F_out, K] and the three bias sums, summed in `dtype`."""
    p = {k: v.to(dtype) for k, v in o["prm"].items()}
    Ws = [p["W_main_in"] + p["W_shared"], p["W_main_out"] + p["W_shared"], p["W_undirected"] + p["W_shared"]]
    if case.proj:
        Ws.append(o["W_res"].to(dtype))
    bs = [p["b_main_in"] + p["b_dir_shared_in"], p["b_main_out"] + p["b_dir_shared_out"],
          p["b_undirected"] + p["b_undirected_shared"]]
    return torch.cat(Ws, 1), bs


@functools.lru_cache(maxsize=None)
def reference(case: Case) -> dict:
    """{output: (ref64, den)}: the float64 formula on the fp32 operands, and the same formula over absolute values."""
    o = operands(case)
    M, Fi = case.M, case.F_in
    W, b = _packed(case, o, torch.float64)
    s = gates64(o["prm"], M)
    Z = o["Z"].double()
    if case.kind == "fwd":
        if case.pre:  # the kernel's operand is the gated one: nothing scales it again
            A = [Z[:, k * Fi:(k + 1) * Fi] for k in range(3)]
            sc = [torch.ones(M, 1, dtype=torch.float64)] * 3
        else:
            A = [Z[:, k * Fi:(k + 1) * Fi] for k in range(3)]
            sc = s
        y = sum(sc[k] * (A[k] @ W[:, k * Fi:(k + 1) * Fi].t()) + s[k] * b[k] for k in range(3))
        den = sum(sc[k].abs() * (A[k].abs() @ W[:, k * Fi:(k + 1) * Fi].abs().t()) + (s[k] * b[k]).abs()
                  for k in range(3))
        if case.proj:
            x = o["res_x"].double()
            y = y + x @ W[:, 3 * Fi:].t() + o["b_res"].double()
            den = den + x.abs() @ W[:, 3 * Fi:].abs().t() + o["b_res"].double().abs()
        elif o["res_x"] is not None:
            y, den = y + o["res_x"].double(), den + o["res_x"].double().abs()
        if o["constant"] is not None:
            y, den = y + o["constant"].double(), den + o["constant"].double().abs()
        return {"Y": (y, den)}
    dY = o["dY"].double()
    if case.kind in ("dgrad", "span"):
        G, Ga = dY @ W, dY.abs() @ W.abs()
        sq = torch.cat([s[k].expand(M, Fi) for k in range(3)], 1)
        out = {"dZ": (sq * G[:, :3 * Fi], sq.abs() * Ga[:, :3 * Fi])}
        if case.proj:
            out["dres"] = (G[:, 3 * Fi:], Ga[:, 3 * Fi:])
        if case.kind == "span":
            wd = o["wdiag"].double()
            dz, dza = out["dZ"]
            E = sum(wd[:, k:k + 1] * dz[:, k * Fi:(k + 1) * Fi] for k in range(3))
            Ea = sum(wd[:, k:k + 1].abs() * dza[:, k * Fi:(k + 1) * Fi] for k in range(3))
            if case.e_res:
                E, Ea = E + dY, Ea + dY.abs()
            out["E"] = (E, Ea)
        return out
    assert case.kind == "wgrad" and not case.proj
    sZ = torch.cat([s[k] * Z[:, k * Fi:(k + 1) * Fi] for k in range(3)], 1)
    S = torch.cat(s + [torch.ones(M, 1, dtype=torch.float64)], 1)  # [M, 4]: the fourth bias sum is unscaled
    return {"dB": (dY.t() @ sZ, dY.abs().t() @ sZ.abs()), "dbsum": (S.t() @ dY, S.abs().t() @ dY.abs())}


@functools.lru_cache(maxsize=None)
def fp32_reference(case: Case) -> dict:
    """The same formulas in torch fp32 on the CPU: what 'fp32 accuracy' means for the case."""
    o = operands(case)
    M, Fi = case.M, case.F_in
    W, b = _packed(case, o, torch.float32)
    s = gates32(o["prm"], M)
    Z = o["Z"]
    if case.kind == "fwd":
        sc = [torch.ones(M, 1)] * 3 if case.pre else s
        y = sum(sc[k] * (Z[:, k * Fi:(k + 1) * Fi] @ W[:, k * Fi:(k + 1) * Fi].t()) + s[k] * b[k] for k in range(3))
        if case.proj:
            y = y + o["res_x"] @ W[:, 3 * Fi:].t() + o["b_res"]
        elif o["res_x"] is not None:
            y = y + o["res_x"]
        if o["constant"] is not None:
            y = y + o["constant"]
        return {"Y": y}
    dY = o["dY"]
    if case.kind in ("dgrad", "span"):
        G = dY @ W
        out = {"dZ": torch.cat([s[k] * G[:, k * Fi:(k + 1) * Fi] for k in range(3)], 1)}
        if case.proj:
            out["dres"] = G[:, 3 * Fi:]
        if case.kind == "span":
            E = sum(o["wdiag"][:, k:k + 1] * out["dZ"][:, k * Fi:(k + 1) * Fi] for k in range(3))
            out["E"] = E + dY if case.e_res else E
        return out
    sZ = torch.cat([s[k] * Z[:, k * Fi:(k + 1) * Fi] for k in range(3)], 1)
    S = torch.cat(s + [torch.ones(M, 1)], 1)
    return {"dB": dY.t() @ sZ, "dbsum": S.t() @ dY}


@functools.lru_cache(maxsize=None)
def _split_operands(case: Case):
    """The two operands the kernels split, as they round them, split once for all nine schemes."""
    o = operands(case)
    M, Fi = case.M, case.F_in
    W, _ = _packed(case, o, torch.float32)       # fl(W_q + W_shared): pack_kernel / dense_x3p_kernel's rawW path
    s = gates32(o["prm"], M)
    if case.kind == "fwd":
        A = o["Z"] if case.pre else torch.cat([o["Z"][:, k * Fi:(k + 1) * Fi] * s[k] for k in range(3)], 1)
        if case.proj:
            A = torch.cat([A, o["res_x"]], 1)
        return split3(A.contiguous()), split3(W.contiguous())
    if case.kind in ("dgrad", "span"):           # G = dpre W: contraction over F_out
        return split3(o["dY"].contiguous()), split3(W.t().contiguous())
    sZ = torch.cat([o["Z"][:, k * Fi:(k + 1) * Fi] * s[k] for k in range(3)], 1)  # fl(s_q Z_q)
    return split3(o["dY"].t().contiguous()), split3(sZ.t().contiguous())           # contraction over the rows


def host_model(case: Case, terms=None) -> dict:
    """The kernels' arithmetic on the host with the product list `terms` (default SIX): every rounding the kernels
    make outside the MFMAs in fp32, the MFMAs as gemm_split. Computed once per (case, terms); never modified."""
    return _host_model(case, tuple(SIX if terms is None else terms))


@functools.lru_cache(maxsize=None)
def _host_model(case: Case, terms: tuple) -> dict:
    o = operands(case)
    M, Fi = case.M, case.F_in
    A3, W3 = _split_operands(case)
    s = gates32(o["prm"], M)
    if case.kind == "fwd":
        acc = gemm_split(A3, W3, terms, KSTEP_FWD)
        _, b = _packed(case, o, torch.float32)
        gb = _fma(s[2], b[2], _fma(s[1], b[1], s[0] * b[0]))  # epi_sum (pg_dense.hip)
        y = acc + gb
        y = y + (o["b_res"] if case.proj else 0.0)
        y = y + (o["constant"] if o["constant"] is not None else 0.0)
        y = y + (o["res_x"] if (o["res_x"] is not None and not case.proj) else 0.0)
        if case.drop > 0:  # kept elements are scaled by fl(1 / (1 - p)); the test divides by the same number
            y = y * drop_scale(case.drop)
        return {"Y": y}
    if case.kind in ("dgrad", "span"):
        G = gemm_split(A3, W3, terms, KSTEP_BWD)
        out = {"dZ": torch.cat([s[k] * G[:, k * Fi:(k + 1) * Fi] for k in range(3)], 1)}
        if case.proj:
            out["dres"] = G[:, 3 * Fi:]
        if case.kind == "span":
            wd = o["wdiag"]
            e = torch.zeros(M, Fi)
            for k in range(3):
                e = _fma(wd[:, k:k + 1].expand(M, Fi), out["dZ"][:, k * Fi:(k + 1) * Fi], e)
            out["E"] = e + o["dY"] if case.e_res else e
        return out
    splits, rows = plan_of_x3w(M, Fi, case.F_out)
    parts = [gemm_split(tuple(a[:, r0:r0 + rows] for a in A3), tuple(w[:, r0:r0 + rows] for w in W3), terms, WX_K)
             for r0 in range(0, M, rows)]
    assert len(parts) == splits
    return {"dB": reduce_splits(parts)}


def dbsum_bound(case: Case):
    """(rms, max) bound of wgrad's bias sums, which are plain fp32 sums of n = M rounded products s_q dpre (no split
    products, so no mutant applies). With u = 2^-24 every partial sum is at most den in magnitude, so each of the at
    most n roundings (one per product, n - 1 per element's additions in any order) errs by at most u den: max(e) <=
    n u to first order, and sqrt(n) u for the rms of n independent roundings."""
    u = 2.0 ** -24
    return math.sqrt(case.M) * u, case.M * u


@functools.lru_cache(maxsize=None)
def bounds(case: Case) -> dict:
    """{output: {"fp32": (rms, max), "model": (rms, max), "mutants": {name: (rms, max)}, "mutant_min": (rms, max),
    "bound": (rms, max)}} for every output the split products reach. bound = sqrt(model * mutant_min), for rms and
    max separately."""
    ref = reference(case)
    f32 = fp32_reference(case)
    scale = 1.0 / drop_scale(case.drop) if case.drop > 0 else 1.0  # undo the kept elements' 1 / (1 - p)
    keep = drop_keep(case)
    model = host_model(case)
    mut = {name: host_model(case, terms) for name, terms in MUTANTS.items()}
    out = {}
    for k, (r64, den) in ref.items():
        if k == "dbsum":
            continue
        b = metric(model[k].double() * scale, r64, den, keep)
        m = {name: metric(v[k].double() * scale, r64, den, keep) for name, v in mut.items()}
        c = (min(v[0] for v in m.values()), min(v[1] for v in m.values()))
        out[k] = {"fp32": metric(f32[k], r64, den, keep), "model": b, "mutants": m, "mutant_min": c,
                  "bound": (math.sqrt(b[0] * c[0]), math.sqrt(b[1] * c[1]))}
    return out


def _old_tolerance(case: Case, name: str, got: torch.Tensor):
    """|d| / tol per element under the suite's earlier tolerance for the output: |d| <= 2e-5 + 2e-5 |ref| for the
    forward, assert_grad_close's 1e-4 |ref| + 2e-5 max|ref| for the gradients (tests/test_gpu_parity.py). `got` with
    the fused dropout's scale undone; kept elements only."""
    r = reference(case)[name][0].float()
    d = (got.float() - r).abs()
    tol = 2e-5 + 2e-5 * r.abs() if case.kind == "fwd" else 1e-4 * r.abs() + 2e-5 * float(r.abs().max()) + 1e-7
    q = d / tol
    keep = drop_keep(case)
    return q if keep is None else q[keep]


def old_tolerance_headroom(case: Case, name: str, got: torch.Tensor) -> float:
    """max |d| / tol under the earlier tolerance: <= 1 passes it."""
    return float(_old_tolerance(case, name, got).max())


def old_tolerance_pass_fraction(case: Case, name: str, got: torch.Tensor) -> float:
    return float((_old_tolerance(case, name, got) <= 1).double().mean())
