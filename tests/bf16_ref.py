"""Host model of the bf16 dense kernels (csrc/pg_bf16.hip, csrc/pg_dense_bwd.hip) and the bounds their accuracy tests
assert.

bf16 mode's contract (pg_bf16.hip:3-5): storage is bf16, every sum is fp32 and rounded once to bf16 when stored. This
module restates on the CPU every rounding the kernels make -- the forward dense_bf16_kernel, the input gradients
dgrad_bf16_kernel / dgrad_bf16r_kernel, the gate-gradient pass, the weight gradients wgrad_bf16_kernel /
wgrad_bfs_kernel and the split reduction -- each cited to its source line (`forward_model`, `dgrad_model`,
`dgate_model`, `dB_model`, `dbsum_model`), together with the float64 formula on the same rounded operands and its
normaliser `den`, the same formula over absolute values (`reference`), and the sixteen one-line slips that would break
the contract while staying far inside the suite's earlier tolerances (`MUTANTS`). tests/test_bf16_host.py checks
without a GPU that the criteria below pass the model and fail every slip; tests/test_gpu_bf16_accuracy.py asserts them
on the kernels.

Two criteria, neither holding a constant taken from the kernels' output:

* bf16 outputs (Y, dZ, dres): faithful rounding. Every element obeys
      |got - ref64| <= ulp_bf16(ref64) / 2 + (K_c + 8) 2^-24 den,
  K_c the contraction length (K forward, F_out for dgrad). The first term is the one rounding to nearest of the stored
  value. The second is the first-order worst case of the fp32 arithmetic before it, with u = 2^-24: K_c exact bf16
  products summed in any order round K_c - 1 times, each by at most u times a partial sum of magnitude <= den; the
  epilogue adds at most 9 more (forward: the three gate-bias products, jointly <= u sum |s_q b_q|; their two
  additions; acc + gate-bias, + b_res, + constant, + res_x; the slope; the dropout scale. dgrad: the gate scale). It
  is a priori: it holds however the MFMA orders a k-step and whether or not the compiler contracts the epilogue's
  multiply-adds. With the fused dropout the kept elements are judged with 1 / (1 - p) undone (the stored value is
  fl(y ds), so the rounding term is ulp_bf16(ref64 ds) / (2 ds)); the dropped ones must be exactly 0.
* fp32 outputs (dB, dgate): the componentwise metric e = |got - ref64| / den of tests/split3_ref.py, rms and max
  bounded separately by the geometric mean of (b) the larger of the host model's and the plain torch-fp32 formula's
  metric -- so the model need not mirror a kernel's split plan or a compiler's contractions bit for bit -- and (c) the
  smallest metric among the mutants of that output, all three on the case's own operands.
* dbsum (plain fp32 sums of M products of rounded operands): split3_ref.dbsum_bound. dpre: bit-equal to the model.

'dpre not rounded' is listed for dB only, not for dZ: there the float64 reference itself is built on the rounded dpre
(the operand the contract names), and dZ's own rounding (2^-9 relative) is as large as the change the slip makes to half
of the products, so faithful rounding separates it only weakly; the bit-equality of the stored dpre is its check.
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass, replace
from typing import Optional

import torch

import split3_ref as sr
from split3_ref import dbsum_bound, drop_keep, drop_scale, gates32, metric, reduce_splits  # noqa: F401

# The leaky_relu slope of these tests. Not the layers' 0.01: with it the negative half of dpre = fl(dY slope) weighs a
# hundredth in every sum, and the two 'dpre not rounded' slips sit within 4x of the fp32 formulas' own error; at 0.3
# (not a power of two: fl(dY slope) needs its rounding) they sit 150x above it. The kernels take the slope as an argument.
SLOPE = 0.3
TABLE_ROWS = 300     # the gate / constant table of the row-map case
KSTEP = 16           # v_mfma_f32_32x32x16_bf16: one fp32 rounding per 16-deep step (split3_ref.gemm_split's convention)
KTILE = 64           # BKB, the kernels' LDS k-tile (pg_bf16.hip:179, pg_dense_bwd.hip:1369)
U = 2.0 ** -24

_W_KEYS, _B_KEYS, _C_KEYS = sr._W_KEYS, sr._B_KEYS, sr._C_KEYS


def _bf(x: torch.Tensor) -> torch.Tensor:
    return x.to(torch.bfloat16).to(torch.float32)  # pgbf::f2bf: round to nearest even


def _f32(v: float) -> torch.Tensor:
    return torch.tensor(v, dtype=torch.float32)


# ---------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    kind: str             # "fwd" | "bwd"
    M: int
    F_in: int
    F_out: int
    proj: bool = False    # projected residual (W_res): a fourth K segment
    vec: bool = True      # vector gates (forward: + constant, + identity residual where F_in == F_out)
    rows: bool = False    # forward: a row map into a TABLE_ROWS-row gate / constant table
    wide: bool = False    # operand columns / weight rows scaled by 2^[-12, 12]
    drop: float = 0.0     # the fused dropout's p (backward: read off Y's zeros)
    variant: str = ""     # "dgrad_tiled" | "wgrad_tiled": the kernel flag; the operands are the plain case's
    seed: int = 0

    @property
    def id(self) -> str:
        s = f"{self.kind}-M{self.M}-{self.F_in}x{self.F_out}"
        for flag, name in ((self.proj, "proj"), (not self.vec, "scalar"), (self.rows, "rows"), (self.wide, "wide"),
                           (self.drop > 0, "drop"), (bool(self.variant), self.variant)):
            if flag:
                s += "-" + name
        return s

    @property
    def K(self) -> int:
        return (4 if self.proj else 3) * self.F_in


FWD = [
    Case("fwd", 129, 128, 128, seed=101),                           # one 128-row tile and a row
    Case("fwd", 129, 128, 128, vec=False, seed=102),
    Case("fwd", 129, 128, 128, rows=True, seed=103),
    Case("fwd", 257, 64, 128, proj=True, seed=104),                 # fourth K segment
    Case("fwd", 129, 16, 40, proj=True, seed=105),                  # N tail, K = 64: a single k-tile
    Case("fwd", 4099, 256, 256, seed=106),                          # config 5's widths, two column tiles
    Case("fwd", 257, 128, 128, drop=0.3, seed=107),
    Case("fwd", 257, 128, 128, vec=False, wide=True, seed=108),     # nothing unscaled is added
]
_B0 = Case("bwd", 257, 128, 128, seed=201)
BWD = [
    _B0,                                                            # dgrad_bf16r, wgrad_bfs
    Case("bwd", 257, 256, 256, seed=202),                           # dgrad_bf16r, four k-tiles, six n-tiles
    Case("bwd", 257, 64, 128, proj=True, seed=203),                 # dgrad_bf16r with dres; wgrad_bf16
    Case("bwd", 65, 128, 64, seed=204),                             # dgrad_bf16r, one k-tile
    Case("bwd", 257, 128, 128, drop=0.3, seed=205),
    Case("bwd", 257, 128, 128, wide=True, seed=206),
    Case("bwd", 129, 16, 40, proj=True, seed=207),                  # dgrad_bf16, wgrad_bf16: partial tiles everywhere
    Case("bwd", 129, 64, 512, seed=208),                            # dgrad_bf16: F_out above the resident kernel's 256
    replace(_B0, variant="dgrad_tiled"),                            # dgrad_bf16 on the resident kernel's shape
    Case("bwd", 4099, 128, 128, seed=209),                          # wgrad_bfs: 129 splits, the last with three rows
    Case("bwd", 1025, 256, 256, seed=210),                          # wgrad_bfs: four output tiles
    replace(_B0, variant="wgrad_tiled"),                            # wgrad_bf16 on the staged kernel's shape
    Case("bwd", 257, 128, 128, proj=True, seed=211),                # wgrad_bfs + wgrad_bf16 for W_res's columns
]
CASES = FWD + BWD
DROP_SEED = sr.DROP_SEED


def operands(case: Case) -> dict:
    """The case's operands on the CPU, from its seed (the GPU test uploads exactly these). Never modified."""
    return _operands(replace(case, variant=""))


@functools.lru_cache(maxsize=None)
def _operands(case: Case) -> dict:
    g = torch.Generator().manual_seed(case.seed)
    M, Fi, Fo = case.M, case.F_in, case.F_out
    T = TABLE_ROWS if case.rows else M
    o = {"Z": _bf(torch.randn(M, 3 * Fi, generator=g))}
    prm = {k: torch.randn(Fo, Fi, generator=g) * 0.1 for k in _W_KEYS}
    for k in _B_KEYS:
        prm[k] = torch.randn(Fo, generator=g) * 0.1
    for k in _C_KEYS:
        prm[k] = torch.rand((T, 1) if case.vec else (1,), generator=g) + 0.5
    o["W_res"] = torch.randn(Fo, Fi, generator=g) * 0.1 if case.proj else None
    o["b_res"] = torch.randn(Fo, generator=g) * 0.1 if case.proj else None
    has_res = case.proj or (case.kind == "fwd" and case.vec and Fi == Fo)
    o["res_x"] = _bf(torch.randn(M, Fi, generator=g)) if has_res else None
    o["constant"] = torch.randn(T, Fo, generator=g) if (case.kind == "fwd" and case.vec) else None
    o["rows"] = torch.randint(0, T, (M,), generator=g) if case.rows else None
    o["dY"] = _bf(torch.randn(M, Fo, generator=g))
    Y = _bf(torch.randn(M, Fo, generator=g))  # backward: the stored output whose signs (and zeros) drive act'
    if case.wide:  # powers of two: every bf16 stays a bf16 and keeps its significand; only the exponents spread
        r = torch.exp2(torch.randint(-12, 13, (Fi,), generator=g).float())
        q = torch.exp2(torch.randint(-12, 13, (Fo,), generator=g).float())
        if case.kind == "fwd":
            assert o["constant"] is None and o["res_x"] is None  # nothing unscaled is added to the scaled columns
            o["Z"] = o["Z"] * r.repeat(3)
            for k in _W_KEYS:
                prm[k] = prm[k] * q[:, None]
            for k in _B_KEYS:
                prm[k] = prm[k] * q
        else:
            o["dY"] = o["dY"] * q
    if case.kind == "bwd":
        keep = drop_keep(case)
        o["Y"] = Y if keep is None else torch.where(keep, Y, torch.zeros(()))
    o["prm"] = prm
    return o


@dataclass(frozen=True)
class _Prep:
    s: tuple               # s_in, s_out, s_und [M, 1] fp32, as every kernel rounds them (gates32)
    c: dict                # the five gates per row [M, 1]
    B: torch.Tensor        # [F_out, K] bf16 values: the packed contraction operand
    B32: torch.Tensor      # the same before its rounding (pack_kernel's fp32 sums)
    bsum: torch.Tensor     # [4, F_out] fp32 bias sums
    dpre32: Optional[torch.Tensor]  # backward: act_grad before its rounding
    dpre: Optional[torch.Tensor]    # bf16(dpre32)


def act_grad(d, y, slope: float, ds: float):
    """pg::act_grad (pg_common.h:68-72) in its operation order: fl(fl(d ds) slope)."""
    sl = _f32(slope)
    if ds == 0.0:
        return torch.where(y > 0, d, d * sl)
    e = d * _f32(ds)
    return torch.where(y > 0, e, torch.where(y < 0, e * sl, torch.zeros(())))


def prepared(case: Case) -> _Prep:
    return _prepared(replace(case, variant=""))


@functools.lru_cache(maxsize=None)
def _prepared(case: Case) -> _Prep:
    o = operands(case)
    prm, M = o["prm"], case.M
    idx = o["rows"]
    c = {k: (prm[k][idx] if idx is not None else prm[k]) for k in _C_KEYS}
    s = tuple(gates32(c, M))  # pg_bf16.hip:241-244, row_gate_prologue (pg_dense_bwd.hip:142-145)
    c = {k: (v.expand(M, 1) if v.numel() == 1 else v) for k, v in c.items()}
    Ws = [prm["W_main_in"] + prm["W_shared"], prm["W_main_out"] + prm["W_shared"],
          prm["W_undirected"] + prm["W_shared"]]                     # pack_kernel (pg_dense.hip:1184-1187), fp32
    if case.proj:
        Ws.append(o["W_res"])
    B32 = torch.cat(Ws, 1)
    bsum = torch.stack([prm["b_main_in"] + prm["b_dir_shared_in"], prm["b_main_out"] + prm["b_dir_shared_out"],
                        prm["b_undirected"] + prm["b_undirected_shared"],
                        o["b_res"] if case.proj else torch.zeros(case.F_out)])  # pg_dense.hip:1192-1195
    dpre32 = dpre = None
    if case.kind == "bwd":
        ds = drop_scale(case.drop) if case.drop > 0 else 0.0
        dpre32 = act_grad(o["dY"], o["Y"], SLOPE, ds)
        dpre = _bf(dpre32)                                           # a_piece_bf16: pack8 (pg_dense_bwd.hip:1401)
    return _Prep(s, c, _bf(B32), B32, bsum, dpre32, dpre)           # pg_f32_to_bf16 (pg_bf16.hip:402)


def gemm16(A: torch.Tensor, Bt: torch.Tensor, tile_bf16: bool = False) -> torch.Tensor:
    """A [M, K] Bt [K, N] with fp32 accumulation in 16-deep steps, one rounding per step (the 16 products and their
    sum are exact in float64 for bf16 operands). tile_bf16: the mutant that rounds the accumulator to bf16 after every
    64-deep k-tile."""
    Ad, Bd = A.double(), Bt.double()
    K = A.shape[1]
    acc = torch.zeros(A.shape[0], Bt.shape[1], dtype=torch.float32)
    for k0 in range(0, K, KSTEP):
        acc = (acc.double() + Ad[:, k0:k0 + KSTEP] @ Bd[k0:k0 + KSTEP]).float()
        if tile_bf16 and ((k0 + KSTEP) % KTILE == 0 or k0 + KSTEP >= K):
            acc = _bf(acc)
    return acc


def _segs(x: torch.Tensor, Fi: int):
    return [x[:, k * Fi:(k + 1) * Fi] for k in range(3)]


MUTANTS = {
    "Y": ["bf16 accumulator", "bf16 pre-activation", "bf16 accumulator per k-tile", "fp32 A"],
    "dZ": ["s bf16(G)", "bf16(s) G", "bf16 accumulator per k-tile", "fp32 W"],
    "dres": ["bf16 accumulator per k-tile", "fp32 W"],   # s == 1 there: the first two are no slips of dres
    "dB": ["bf16 partials", "bf16(s) Z", "s Z not rounded", "dpre not rounded"],
    "dgate": ["gate dot from bf16(G)", "gate dot from dZ / s", "unrounded dpre in the bias dot", "round-5 slip"],
}


def mutants_of(case: Case, name: str):
    m = MUTANTS[name]
    if name == "dres" and case.F_out <= KTILE:  # one k-tile: bf16(bf16(G)) is bf16(G)
        m = [x for x in m if x != "bf16 accumulator per k-tile"]
    return m


# ---------------------------------------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------------------------------------
def _fwd_extras(case: Case):
    o = operands(case)
    z = torch.zeros(())
    br = prepared(case).bsum[3] if case.proj else z
    cc = z
    if o["constant"] is not None:
        cc = o["constant"] if o["rows"] is None else o["constant"][o["rows"]]   # pg_bf16.hip:381, Crow
    rr = o["res_x"] if (o["res_x"] is not None and not case.proj) else z
    return br, cc, rr


def forward_model(case: Case, mut: Optional[str] = None) -> torch.Tensor:
    """dense_bf16_kernel: Y as bf16 values. `mut`: one of MUTANTS["Y"], each one changed line."""
    return _forward_model(case, mut)


@functools.lru_cache(maxsize=None)
def _forward_model(case: Case, mut) -> torch.Tensor:
    o, P = operands(case), prepared(case)
    Fi = case.F_in
    sZ = torch.cat([s * z for s, z in zip(P.s, _segs(o["Z"], Fi))], 1)          # pg_bf16.hip:300, fp32
    A = sZ if mut == "fp32 A" else _bf(sZ)                                        # :301 pack8
    if case.proj:
        A = torch.cat([A, o["res_x"]], 1)                                        # :295 the fourth segment is unscaled
    acc = gemm16(A, P.B.t(), tile_bf16=mut == "bf16 accumulator per k-tile")     # :339
    if mut == "bf16 accumulator":
        acc = _bf(acc)
    s, b = P.s, P.bsum
    br, cc, rr = _fwd_extras(case)
    y = acc + ((s[0] * b[0] + s[1] * b[1]) + s[2] * b[2])                         # :390, left to right
    y = ((y + br) + cc) + rr
    if mut == "bf16 pre-activation":
        y = _bf(y)
    y = torch.where(y > 0, y, y * _f32(SLOPE))                                    # :391
    if case.drop > 0:
        y = torch.where(drop_keep(case), y * _f32(drop_scale(case.drop)), torch.zeros(()))   # :393
    return _bf(y)                                                                 # :396 pack2


# ---------------------------------------------------------------------------------------------------------
# backward
# ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _G(case: Case, mut=None) -> torch.Tensor:
    """G = dpre B [M, K] in fp32 (dgrad_bf16_kernel: pg_dense_bwd.hip:1556; dgrad_bf16r_kernel: :1796)."""
    P = prepared(case)
    return gemm16(P.dpre, P.B32 if mut == "fp32 W" else P.B, tile_bf16=mut == "bf16 accumulator per k-tile")


def dgrad_model(case: Case, mut: Optional[str] = None) -> dict:
    return _dgrad_model(replace(case, variant=""), mut)


@functools.lru_cache(maxsize=None)
def _dgrad_model(case: Case, mut) -> dict:
    P, Fi = prepared(case), case.F_in
    G = _G(case, mut if mut in ("fp32 W", "bf16 accumulator per k-tile") else None)
    if mut == "s bf16(G)":
        dz = [_bf(s * _bf(g)) for s, g in zip(P.s, _segs(G, Fi))]
    elif mut == "bf16(s) G":
        dz = [_bf(_bf(s) * g) for s, g in zip(P.s, _segs(G, Fi))]
    else:
        dz = [_bf(s * g) for s, g in zip(P.s, _segs(G, Fi))]                     # :1597 / :1751 pack4(sc * gv)
    out = {"dZ": torch.cat(dz, 1)}
    if case.proj:
        out["dres"] = _bf(G[:, 3 * Fi:])                                          # :1599 / :1753 pack4(gv)
    return out


def _bias_dots(case: Case, d: torch.Tensor):
    """<dpre[m], bsum_q>: a thread owns 8 columns of a 64-column k-tile and adds its 8-product sums over the k-tiles
    in order (pg_dense_bwd.hip:1411-1415); the 8 threads of a row are summed by a butterfly (bias_dot_reduce)."""
    P, Fo = prepared(case), case.F_out
    npc = (Fo + 7) // 8
    out = []
    for q in range(3):
        pieces = (d.double() * P.bsum[q].double()).view(case.M, npc, 8).sum(-1).float()
        pad = (-npc) % 8
        if pad:
            pieces = torch.cat([pieces, torch.zeros(case.M, pad)], 1)
        lanes = torch.zeros(case.M, 8)
        for t in range(pieces.shape[1] // 8):
            lanes = lanes + pieces[:, 8 * t:8 * t + 8]
        for sh in (1, 2, 4):
            lanes = lanes + lanes[:, [i ^ sh for i in range(8)]]
        out.append(lanes[:, 0])
    return out


def _gate_dots(case: Case, G: torch.Tensor, bias, slip: bool = False):
    """ds_q[m]: per 128-column n-tile, the row's dot4 products <G, Z> of 4 columns each (pg_dense_bwd.hip:1588 /
    :1740) added in column order to the segment's partial, which starts from the bias dot in the lead tile
    (row_dsp_store, :257-272); then the n-tiles in order (gate_grad_kernel, :832-836)."""
    o, Fi, M = operands(case), case.F_in, case.M
    p4 = (G[:, :3 * Fi].double() * o["Z"].double()).view(M, 3 * Fi // 4, 4).sum(-1).float()
    d = [torch.zeros(M) for _ in range(3)]
    for t in range((case.K + 127) // 128):
        ds = [bias[q].clone() if t == 0 else torch.zeros(M) for q in range(3)]
        for c in range(32):
            col = 128 * t + 4 * c
            if col < 3 * Fi:
                ds[col // Fi] = ds[col // Fi] + p4[:, col // 4]
        if slip and t == 0:  # the round-5 fault: the lead tile's segment-0 partial of rows 48-63 of each 64
            hit = (torch.arange(M) % 64) >= 48
            ds[0] = torch.where(hit, ds[0] * _f32(1.008), ds[0])
        d = [a + b for a, b in zip(d, ds)]
    return d


def _gate_grad(c: dict, d, dtype=torch.float32):
    """The five products of gate_grad_kernel (pg_dense_bwd.hip:839-844) -> [5, M]."""
    ci, co, cd, cu, ca = [c[k].to(dtype).view(-1) for k in ("C_in", "C_out", "C_directed", "C_undirected", "C_all")]
    d0, d1, d2 = [x.to(dtype) for x in d]
    cad = ca * cd
    t = d0 * ci + d1 * co
    return torch.stack([d0 * cad, d1 * cad, ca * t, d2 * ca, cd * t + d2 * cu])


def dgate_model(case: Case, mut: Optional[str] = None) -> torch.Tensor:
    return _dgate_model(replace(case, variant=""), mut)


@functools.lru_cache(maxsize=None)
def _dgate_model(case: Case, mut) -> torch.Tensor:
    P, Fi = prepared(case), case.F_in
    G = _G(case)                                   # the fp32 accumulator parked in T (:1564 / :1727)
    if mut == "gate dot from bf16(G)":
        G = _bf(G)
    elif mut == "gate dot from dZ / s":
        dz = _segs(_dgrad_model(case, None)["dZ"], Fi)
        G = torch.cat([z / s for z, s in zip(dz, P.s)], 1)
    bias = _bias_dots(case, P.dpre32 if mut == "unrounded dpre in the bias dot" else P.dpre)   # :1405 the rounded dr
    return _gate_grad(P.c, _gate_dots(case, G, bias, slip=mut == "round-5 slip"))


def wgrad_staged(case: Case) -> bool:
    """wgrad_bfs_kernel takes the gated segments (pg_directgcn_dense_bwd_bf16, pg_dense_bwd.hip:2612-2617; the
    alignment conditions hold for every tensor of these tests and the 32-bit offsets fit)."""
    return case.F_in % 128 == 0 and case.F_out % 128 == 0 and case.variant != "wgrad_tiled"


def wgrad_plan(case: Case):
    """(splits, rows_per_split): plan_of with the staged kernels' 16-row steps (pg_dense_bwd.hip:2292-2297) or
    split_rows with the tiled kernels' 32-row chunks (:1999-2010)."""
    M, Fi, Fo, K = case.M, case.F_in, case.F_out, case.K
    if wgrad_staged(case):
        tiles = (Fo // 128) * (min(K, 3 * Fi) // 384)
        steps = max((M + 15) // 16, 1)
        splits = min(max((256 + tiles - 1) // tiles, 1), steps)
        rows = ((steps + splits - 1) // splits) * 16
    else:
        tiles = ((Fo + 127) // 128) * ((K + 127) // 128)
        chunks = (M + 31) // 32
        splits = max(min((512 + tiles - 1) // tiles, chunks), 1)
        rows = max(((chunks + splits - 1) // splits) * 32, 32)
    return max((M + rows - 1) // rows, 1), rows


def _gated_Z(case: Case, s, rounded: bool = True):
    """The weight gradient's B operand: bf16(fl(s_q Z_q)) (wgrad_bf16_kernel: pg_dense_bwd.hip:1910; wgrad_bfs_kernel:
    :2080-2087), and res_x unscaled."""
    o = operands(case)
    sZ = torch.cat([sq * z for sq, z in zip(s, _segs(o["Z"], case.F_in))], 1)
    if rounded:
        sZ = _bf(sZ)
    return torch.cat([sZ, o["res_x"]], 1) if case.proj else sZ


def dB_model(case: Case, mut: Optional[str] = None) -> torch.Tensor:
    return _dB_model(case, mut)


@functools.lru_cache(maxsize=None)
def _dB_model(case: Case, mut) -> torch.Tensor:
    P = prepared(case)
    _, rows = wgrad_plan(case)
    A = P.dpre32 if mut == "dpre not rounded" else P.dpre           # the stored bf16 dpre (wgrad_params, :2394)
    s = [_bf(x) for x in P.s] if mut == "bf16(s) Z" else P.s          # `gates` [M, 4] fp32 (:146)
    Bop = _gated_Z(case, s, rounded=mut != "s Z not rounded")
    parts = [gemm16(A[r0:r0 + rows].t(), Bop[r0:r0 + rows]) for r0 in range(0, case.M, rows)]   # fp32 partials
    if mut == "bf16 partials":
        parts = [_bf(p) for p in parts]
    return reduce_splits(parts)                                      # reduce_splits_kernel (:1329)


@functools.lru_cache(maxsize=None)
def dbsum_model(case: Case) -> torch.Tensor:
    """[4, F_out]: sum over the rows of fl(s_q dpre), q = 3 unscaled, row after row within a split in fp32
    (pg_dense_bwd.hip:1926 / :2107), then reduce_splits."""
    P, M = prepared(case), case.M
    n, rows = wgrad_plan(case)
    S = torch.cat(list(P.s) + [torch.ones(M, 1)], 1)                 # [M, 4]
    pad = n * rows - M
    Sp = torch.cat([S, torch.zeros(pad, 4)]).view(n, rows, 4)
    Dp = torch.cat([P.dpre, torch.zeros(pad, case.F_out)]).view(n, rows, case.F_out)
    acc = torch.zeros(n, 4, case.F_out)
    for r in range(rows):
        acc = acc + Sp[:, r, :, None] * Dp[:, r, None, :]
    return reduce_splits([acc[i] for i in range(n)])


# ---------------------------------------------------------------------------------------------------------
# float64 reference on the same rounded operands, its normaliser, and the plain torch-fp32 formula
# ---------------------------------------------------------------------------------------------------------
def reference(case: Case) -> dict:
    """{output: (ref64, den)}. Forward: Y without the dropout's scale. den of a leaky_relu output carries the slope on
    the negative elements; dgate's carries absolute values through the five gate formulas (c_directed and c_all
    cancel)."""
    return _reference(replace(case, variant=""))


@functools.lru_cache(maxsize=None)
def _reference(case: Case) -> dict:
    o, P = operands(case), prepared(case)
    Fi, M = case.F_in, case.M
    s = [x.double() for x in P.s]
    B = P.B.double()
    if case.kind == "fwd":
        A = torch.cat([_bf(sq * z) for sq, z in zip(P.s, _segs(o["Z"], Fi))], 1).double()
        if case.proj:
            A = torch.cat([A, o["res_x"].double()], 1)
        br, cc, rr = [x.double() for x in _fwd_extras(case)]
        gb = sum(s[q] * P.bsum[q].double() for q in range(3))
        gba = sum((s[q] * P.bsum[q].double()).abs() for q in range(3))
        pre = A @ B.t() + gb + br + cc + rr
        den = A.abs() @ B.abs().t() + gba + br.abs() + cc.abs() + rr.abs()
        sl = float(_f32(SLOPE))
        return {"Y": (torch.where(pre > 0, pre, pre * sl), torch.where(pre < 0, den * sl, den))}
    d = P.dpre.double()
    G, Ga = d @ B, d.abs() @ B.abs()
    sq = torch.cat([x.expand(M, Fi) for x in s], 1)
    out = {"dZ": (sq * G[:, :3 * Fi], sq.abs() * Ga[:, :3 * Fi])}
    if case.proj:
        out["dres"] = (G[:, 3 * Fi:], Ga[:, 3 * Fi:])
    Z = o["Z"].double()
    bs = P.bsum.double()
    ds = [(g * z).sum(1) + d @ bs[q] for q, (g, z) in enumerate(zip(_segs(G, Fi), _segs(Z, Fi)))]
    dsa = [(g * z.abs()).sum(1) + d.abs() @ bs[q].abs() for q, (g, z) in enumerate(zip(_segs(Ga, Fi), _segs(Z, Fi)))]
    out["dgate"] = (_gate_grad(P.c, ds, torch.float64),
                    _gate_grad({k: v.abs() for k, v in P.c.items()}, dsa, torch.float64))
    Bop = _gated_Z(case, P.s).double()
    out["dB"] = (d.t() @ Bop, d.abs().t() @ Bop.abs())
    S = torch.cat(s + [torch.ones(M, 1, dtype=torch.float64)], 1)
    out["dbsum"] = (S.t() @ d, S.abs().t() @ d.abs())
    return out


@functools.lru_cache(maxsize=None)
def _fp32_reference(case: Case) -> dict:
    """dB and dgate by the plain torch fp32 formulas on the rounded operands: what 'fp32 sums' means for the case."""
    o, P = operands(case), prepared(case)
    Fi = case.F_in
    G = P.dpre @ P.B
    ds = [(g * z).sum(1) + P.dpre @ P.bsum[q] for q, (g, z) in enumerate(zip(_segs(G, Fi), _segs(o["Z"], Fi)))]
    return {"dgate": _gate_grad(P.c, ds), "dB": P.dpre.t() @ _gated_Z(case, P.s)}


# ---------------------------------------------------------------------------------------------------------
# criteria and bounds
# ---------------------------------------------------------------------------------------------------------
def ulp_bf16(x: torch.Tensor) -> torch.Tensor:
    """The spacing of bf16 (8 significant bits) at |x| (float64); 0 at 0."""
    _, e = torch.frexp(x.abs())  # |x| = m 2^e, m in [0.5, 1)
    return torch.where(x != 0, torch.ldexp(torch.ones_like(x), e - 8), torch.zeros_like(x))


def faithful(case: Case, name: str, got: torch.Tensor):
    """(violations, elements, worst |d| / limit) of the faithful-rounding criterion over every element of a bf16
    output. Forward with the fused dropout: the dropped elements must be exactly 0 (each one that is not counts as a
    violation, worst = inf) and the kept ones are judged with the scale undone."""
    r64, den = reference(case)[name]
    Kc = case.K if name == "Y" else case.F_out
    got = got.double()
    assert got.shape == r64.shape, (name, got.shape, r64.shape)
    ds = drop_scale(case.drop) if (name == "Y" and case.drop > 0) else 1.0
    d = (got / ds - r64).abs()
    lim = ulp_bf16(r64 * ds) / (2 * ds) + (Kc + 8) * U * den
    q = torch.where(lim > 0, d / lim.clamp_min(1e-300), torch.where(d == 0, 0.0, math.inf).double())
    if ds != 1.0:
        keep = drop_keep(case)
        q = torch.where(keep, q, torch.where(got == 0, 0.0, math.inf).double())
    return int((q > 1).sum()), q.numel(), float(q.max())


def model_outputs(case: Case, name: str, mut: Optional[str] = None) -> torch.Tensor:
    if name == "Y":
        return forward_model(case, mut)
    if name in ("dZ", "dres"):
        return dgrad_model(case, mut)[name]
    if name == "dgate":
        return dgate_model(case, mut)
    if name == "dbsum":
        return dbsum_model(case)
    return dB_model(case, mut)


def outputs_of(case: Case):
    if case.kind == "fwd":
        return ["Y"]
    return ["dZ"] + (["dres"] if case.proj else []) + ["dgate", "dB", "dbsum"]


@functools.lru_cache(maxsize=None)
def bounds(case: Case) -> dict:
    """Per output. bf16 outputs: {"model": (violations, n, worst), "mutants": {name: (violations, n, worst)}}.
    fp32 outputs: {"fp32", "model", "mutants": {name: (rms, max)}, "mutant_min", "bound"}, bound = sqrt(max(model,
    fp32) mutant_min) for rms and max separately. dbsum: {"model", "bound"} with split3_ref.dbsum_bound."""
    ref = reference(case)
    out = {}
    for name in outputs_of(case):
        if name in ("Y", "dZ", "dres"):
            out[name] = {"model": faithful(case, name, model_outputs(case, name)),
                         "mutants": {m: faithful(case, name, model_outputs(case, name, m))
                                     for m in mutants_of(case, name)}}
            continue
        r64, den = ref[name]
        model = metric(model_outputs(case, name), r64, den)
        if name == "dbsum":
            out[name] = {"model": model, "bound": dbsum_bound(case)}
            continue
        f32 = metric(_fp32_reference(replace(case, variant=""))[name], r64, den)
        mut = {m: metric(model_outputs(case, name, m), r64, den) for m in mutants_of(case, name)}
        b = (max(model[0], f32[0]), max(model[1], f32[1]))
        c = (min(v[0] for v in mut.values()), min(v[1] for v in mut.values()))
        out[name] = {"fp32": f32, "model": model, "mutants": mut, "mutant_min": c,
                     "bound": (math.sqrt(b[0] * c[0]), math.sqrt(b[1] * c[1]))}
    return out


def earlier_tolerance_used(case: Case, name: str, got: torch.Tensor) -> float:
    """max |d| / tol under the suite's earlier tolerance of the output (tests/test_gpu_parity.py): the forward's
    2^-8 |y| + 1e-5 max|y|, the backward's 2e-2 max|ref| + 2e-2 |ref| + 1e-6. <= 1 passes it."""
    r = reference(case)[name][0]
    got = got.double()
    if name == "Y" and case.drop > 0:
        keep = drop_keep(case)
        got = torch.where(keep, got / drop_scale(case.drop), r)
    d = (got - r).abs()
    mx = float(r.abs().max())
    tol = 2.0 ** -8 * r.abs() + 1e-5 * mx if case.kind == "fwd" else 2e-2 * mx + 2e-2 * r.abs() + 1e-6
    return float((d / tol).max())
