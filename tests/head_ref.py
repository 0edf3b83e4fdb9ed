"""Host model of the head-training kernels (csrc/pg_head_train.hip) and the bounds their accuracy tests assert.

head_train_kernel (fp32 h, F = 128, H = 64, 64-row tiles) and head_train5_kernel (bf16 h, F = 256, H = 128, 16-row
tiles) run the prediction head's forward, loss and backward for any class count 1 <= C <= 32:
    z = h W1^T + b1,  a = dropout(relu(z)),  x = a W2^T + b2,  loss = lw sum_m -log_softmax(x[m])[y[m]],
    dl = s lw (softmax(x) - onehot(y)),  dW2 = dl^T a,  db2 = sum dl,  da = (dl W2) (a > 0) / (1 - p),
    dW1 = da^T h,  db1 = sum da,  dh = da W1.
This module holds the cases of tests/test_gpu_head_accuracy.py (`CASES`: every class count that changes a path, the row
tails, a workgroup's second tile, constant labels, logits of +-120, dead and saturated hidden units, dropout with the
mask restated on the host, GradScaler's first scale), for each case the float64 reference with its normaliser
(`reference`), the plain torch-fp32 formula (`fp32_formula`), the kernels' arithmetic restated in fp32 on the CPU with
every step cited to its source line (`model`), and the one-line slips of that arithmetic (`MUTANTS`).
tests/test_head_host.py checks without a GPU that the criteria below pass the model and fail every slip.

Normaliser. den of an output is its formula over absolute values, carried down the chain so that each intermediate's
first-order sensitivity is in it: den_z = |h| |W1|^T + |b1|, den_a = den_z on the kept units times 1 / (1 - p),
den_x = den_a |W2|^T + |b2|, den_lp[c] = |lp_c| + (1 - p_c) den_x[c] + sum_{c' != c} p_c' den_x[c'] (d lp_c = sum_c'
(1[c = c'] - p_c') d x_c': a class that holds all of the mass does not feel its own logit), den_dl = s lw ((p + onehot)
+ p den_lp) (d p_c = p_c d lp_c), den_da = den_dl |W2| on the kept units times 1 / (1 - p), and then
loss: lw sum_m den_lp[m, y_m]; dW2: den_dl^T den_a; db2: sum den_dl; dW1: den_da^T |h|; db1: sum den_da; dh: den_da |W1|.
With it logits of +-120 (where one fp32 rounding of x is 2^-24 120 absolute, so 2^-17 relative to p) are judged
against what was summed, like every other case; where the softmax is one-hot den_dl falls back to s lw (p + onehot).

Criteria, none holding a constant taken from the kernels' output:

* fp32 outputs (both kernels' loss, dW1, db1, dW2, db2; the fp32 kernel's dh): e = |got - ref64| / den
  (split3_ref.metric), rms and max bounded separately, per case and output, by the geometric mean of (b) the larger of
  the host model's and the plain torch-fp32 formula's metric and (c) the smallest metric among the slips that move the
  output. (b) is never taken below one ulp of the stored fp32 values, ulp_fp32(ref64) / den (`ulp_floor`): a value that
  went through two or more rounded fp32 operations (the loss: the partials' sum, times lw, the reduce kernel's sums)
  is not determined to better than an ulp of itself, and for the loss -- one number per case, so the model's distance
  from float64 is one draw, 0.05 ulp in some cases -- the model's figure alone would ask for less than fp32 can hold. A slip moves an output of a case when its metric there is nonzero and at least MOVES = 4 times (b), in rms
  and in max: below that a slip cannot be told from the arithmetic's own rounding on these operands (at C = 32
  'padded classes counted' changes nothing, without dropout the dropout slips change nothing, a label below 24 hardly
  sees the fourth class slot), and the bound then sits at least 2x above (b) and 2x below (c). Every output of every
  case has such a slip (test_head_host.py).
* dh of the bf16 kernel (stored in bf16): every element obeys |got - ref64| <= ulp_bf16(ref64) / 2 + t,
  t = (C_SPLIT 2^-16 + N_SUM 2^-24) den. A two-term split leaves |v - hi - lo| <= 2^-16 |v| (bf16 keeps 8 bits: |v - hi|
  <= 2^-8 |v|, and lo rounds that remainder to 2^-8 of itself), and the lo lo product a contraction drops is at most
  2^-16 of the product. Counted in units of 2^-16 den along the chain: z: 1 (W1's remainder; h is exact and both
  products are issued); a: the same 1; x: 3 of its own (a's remainder, W2's remainder, the dropped lo lo) + a's 1 = 4;
  lp and dl: 4 (den_lp and den_dl carry the propagation); da: 3 of its own + dl's 4 = 7; dh: 3 of its own + da's 7 =
  C_SPLIT = 10. The fp32 part is the first-order worst case with one rounding per product added, in any order:
  N_SUM = 2 F + 3 H + 3 * 32 + 3 H + 16 products of z, x, da and dh, and 16 for the biases, the softmax's exp, log and
  sums, the scale and the masks. dW1 of the bf16 kernel needs no such count: it is an fp32 output under the metric.
* ReLU's kink, as test_gpu_parity.test_head_train_bf16_vs_float64 treats it: a pre-activation within the kernel's own
  error of 0 -- |z64| <= band, band = 2^-14 den_z (bf16 kernel), (F + 2) 2^-24 den_z (fp32 kernel) -- may fall on the
  other side and switch that unit's whole term, so dh, dW1 and db1 get the switched term's magnitude as slack (|dl W2|
  times the dropout's mask on those elements, through |W1|, |h| and the column sum), from the reference alone; it is
  subtracted from |got - ref64| before either criterion. At most KINK_CAP = 0.2 % of a case's M H pre-activations may
  lie in the band (asserted per case on the CPU).
* Underflow. A float64 term below fp32's 2^-126 (exp(-240) in the +-120 case: the reference's p there is 1e-52, fp32's
  is 0) is lost absolutely, not relatively: each term of a sum may lose up to 2^-126 times its other factor. With at
  most 2^15 rows and factors below 2^10 that is under UNDERFLOW = 2^-100, which is subtracted from every |got - ref64|;
  no output of any case carries a magnitude near it.
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass, replace
from typing import Optional

import numpy as np
import torch

from split3_ref import drop_scale, metric  # noqa: F401

TC = 32                     # classes, padded (pg_head_train.hip:41)
GRID_MAX = 256              # grid_of (:378-381)
U = 2.0 ** -24
C_SPLIT = 10
MOVES = 4.0
KINK_CAP = 2e-3
UNDERFLOW = 2.0 ** -100
HARD = 120.0
DIMS = {"f32": (128, 64, 64), "bf16": (256, 128, 16)}   # F, H, rows per tile (h3, :53; h5, :411)
N_SUM = 2 * 256 + 3 * 128 + 3 * TC + 3 * 128 + 16
OUTPUTS = ("loss", "dh", "dW1", "db1", "dW2", "db2")


def _bf(x: torch.Tensor) -> torch.Tensor:
    return x.to(torch.bfloat16).to(torch.float32)  # (__bf16)v: round to nearest even


def _trunc_bf(x: torch.Tensor) -> torch.Tensor:
    return (x.contiguous().view(torch.int32) & -65536).view(torch.float32)


def _cut10(x: torch.Tensor) -> torch.Tensor:
    return (x.contiguous().view(torch.int32) & -8192).view(torch.float32)  # a 10-bit mantissa


def _f32(v: float) -> torch.Tensor:
    return torch.tensor(v, dtype=torch.float32)


def _drop_keep(seed: int, M: int, H: int, p: float):
    """The kernels' dropout draw restated on the host (pg_head_train.hip, drop_hash :86-94): keep (m, j) when the mixed
    index's top 24 of 32 bits are >= ceil(p 2^24), p as the float the ABI carries (prepare, :726). `seed`: the int64
    the kernel reads, taken as its 64 bits."""
    m = np.arange(M, dtype=np.uint64)[:, None]
    j = np.arange(H, dtype=np.uint64)[None, :]
    with np.errstate(over="ignore"):
        x = np.uint64(seed & 0xFFFF_FFFF_FFFF_FFFF) ^ (np.uint64(0x9E3779B97F4A7C15) * (m * np.uint64(H) + j + np.uint64(1)))
        x ^= x >> np.uint64(33)
        x *= np.uint64(0xff51afd7ed558ccd)
        x ^= x >> np.uint64(33)
        x *= np.uint64(0xc4ceb9fe1a85ec53)
        x ^= x >> np.uint64(33)
    u = (x & np.uint64(0xffffffff)) >> np.uint64(8)
    thr = min(16777215, int(np.ceil(float(np.float32(p)) * 16777216.0)))
    return torch.from_numpy(u >= np.uint64(thr))


# ---------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    kind: str                 # "f32": head_train_kernel | "bf16": head_train5_kernel
    M: int
    C: int
    labels: str = "uniform"   # "uniform" | "last" (every row C - 1) | "first" (every row 0)
    hard: bool = False        # b2[C - 1] += 120, b2[3] -= 120, a third of the rows labelled with each
    units: bool = False       # hidden units DEAD with b1 = -10, LIVE with b1 = +10
    drop: float = 0.0
    negseed: bool = False     # the dropout seed's top bit set
    scale: float = 0.0        # the loss gradient's scale (0: no scale tensor)
    weight: float = 1.0
    seed: int = 0

    @property
    def id(self) -> str:
        s = f"{self.kind}-C{self.C}-M{self.M}"
        for flag, name in ((self.labels != "uniform", self.labels), (self.hard, "hard"), (self.units, "units"),
                           (self.drop > 0, f"drop{self.drop}"), (self.negseed, "negseed"), (self.scale > 0, "scaled")):
            if flag:
                s += "-" + name
        return s

    @property
    def F(self) -> int:
        return DIMS[self.kind][0]

    @property
    def H(self) -> int:
        return DIMS[self.kind][1]

    @property
    def TR(self) -> int:
        return DIMS[self.kind][2]

    @property
    def ntiles(self) -> int:
        return (self.M + self.TR - 1) // self.TR

    @property
    def grid(self) -> int:
        return max(1, min(self.ntiles, GRID_MAX))

    @property
    def drop_seed(self) -> int:
        return (-0x6DCB_A987_6543_2110 if self.negseed else 0x1234_5678_9ABC_DEF0) + self.seed


def _cases(kind: str, one: int, two: int, big: int, s0: int):
    """`one`, `two`: a tile and a row, two tiles and a row; `big`: 257 tiles and a row, so that workgroup 0 walks a
    second tile (the grid is min(tiles, 256)) and workgroup 0's second tile holds one row."""
    TR = one - 1
    c = [
        Case(kind, one, 1),                                        # one class: every gradient is exactly 0
        Case(kind, two, 2, labels="last"),
        Case(kind, one, 7, drop=0.5),                              # one class slot, not full
        Case(kind, two, 8),                                        # one class slot exactly
        Case(kind, one, 9, labels="first"),
        Case(kind, two, 16),                                       # the bf16 kernel's class tile 0 exactly
        Case(kind, one, 17, units=True),                           # one live class in the second class tile
        Case(kind, two, 20, scale=65536.0, weight=0.75),           # GradScaler's first scale
        Case(kind, one, 24),                                       # three class slots exactly
        Case(kind, two, 25, hard=True),                            # the fourth slot holds the +120 class alone
        Case(kind, one, 31, drop=0.9, negseed=True),
        Case(kind, two, 32, labels="last"),                        # no padded class
        Case(kind, 1, 31), Case(kind, TR - 1, 31), Case(kind, TR, 31),   # the row tails of a single tile
        Case(kind, big, 25),
    ]
    return [replace(x, seed=s0 + i) for i, x in enumerate(c)]


F32 = _cases("f32", 65, 129, 16449, 300)
BF16 = _cases("bf16", 17, 33, 4113, 400)
CASES = F32 + BF16
DEAD, LIVE = (1, 17, 62), (0, 16, 63)      # hidden units of a `units` case (both kernels: H >= 64)


def operands(case: Case) -> dict:
    """The case's operands on the CPU, from its seed (the GPU test uploads exactly these). Never modified."""
    return _operands(case)


@functools.lru_cache(maxsize=None)
def _operands(case: Case) -> dict:
    g = torch.Generator().manual_seed(case.seed)
    M, C, F, H = case.M, case.C, case.F, case.H
    h = torch.randn(M, F, generator=g)
    if case.kind == "bf16":
        h = _bf(h)
    W1, b1 = torch.randn(H, F, generator=g) * 0.1, torch.randn(H, generator=g) * 0.1
    W2, b2 = torch.randn(C, H, generator=g) * 0.2, torch.randn(C, generator=g) * 0.1
    y = torch.randint(0, C, (M,), generator=g)
    if case.labels != "uniform":
        y = torch.full((M,), C - 1 if case.labels == "last" else 0, dtype=torch.int64)
    if case.units:
        b1[list(DEAD)] = -10.0
        b1[list(LIVE)] = 10.0
    if case.hard:
        assert C > 24
        b2[C - 1] += HARD
        b2[3] -= HARD
        y[0::3] = C - 1
        y[1::3] = 3
    return {"h": h, "W1": W1, "b1": b1, "W2": W2, "b2": b2, "y": y}


def lw_of(case: Case) -> float:
    """loss_weight as ops._head_train passes it: weight / M rounded to the ABI's float."""
    return float(np.float32(case.weight / max(case.M, 1)))


def scale_of(case: Case) -> float:
    return case.scale if case.scale > 0 else 1.0


@functools.lru_cache(maxsize=None)
def keep_of(case: Case, rows: int) -> Optional[torch.Tensor]:
    return _drop_keep(case.drop_seed, rows, case.H, case.drop) if case.drop > 0 else None


# ---------------------------------------------------------------------------------------------------------
# float64 reference with its normaliser and the kink slack; the plain torch-fp32 formula
# ---------------------------------------------------------------------------------------------------------
def _formula(case: Case, dtype):
    o = operands(case)
    h, W1, b1, W2, b2 = (o[k].to(dtype) for k in ("h", "W1", "b1", "W2", "b2"))
    M, C = case.M, case.C
    z = h @ W1.t() + b1
    k = torch.ones((), dtype=dtype)
    if case.drop > 0:
        k = keep_of(case, M).to(dtype) * (drop_scale(case.drop) if dtype == torch.float32 else 1.0 / (1.0 - case.drop))
    a = torch.relu(z) * k
    lp = torch.log_softmax(a @ W2.t() + b2, dim=1)
    onehot = torch.nn.functional.one_hot(o["y"], C).to(dtype)
    lw = case.weight / M
    loss = -(lp * onehot).sum() * lw
    dl = (lp.exp() - onehot) * (scale_of(case) * lw)
    gz = (dl @ W2) * k                      # d / dz of an active unit
    da = gz * (z > 0).to(dtype)
    out = {"loss": loss, "dh": da @ W1, "dW1": da.t() @ h, "db1": da.sum(0), "dW2": dl.t() @ a, "db2": dl.sum(0)}
    return out, dict(z=z, k=k, lp=lp, onehot=onehot, gz=gz, h=h, W1=W1, b1=b1, W2=W2, b2=b2, lw=lw)


@functools.lru_cache(maxsize=None)
def reference(case: Case) -> dict:
    """{output: (ref64, den, slack)} and "kink": the fraction of the M H pre-activations inside the band."""
    out, v = _formula(case, torch.float64)
    h, W1, W2 = v["h"].abs(), v["W1"].abs(), v["W2"].abs()
    den_z = h @ W1.t() + v["b1"].abs()
    den_a = den_z * (v["z"] > 0) * v["k"]
    den_x = den_a @ W2.t() + v["b2"].abs()
    p = v["lp"].exp()
    den_lp = v["lp"].abs() + (1 - p) * den_x + ((p * den_x).sum(1, keepdim=True) - p * den_x).clamp_min(0.0)
    den_dl = ((p + v["onehot"]) + p * den_lp) * (scale_of(case) * v["lw"])
    den_da = (den_dl @ W2) * (v["z"] > 0) * v["k"]
    den = {"loss": (den_lp * v["onehot"]).sum() * v["lw"], "dh": den_da @ W1, "dW1": den_da.t() @ h,
           "db1": den_da.sum(0), "dW2": den_dl.t() @ den_a, "db2": den_dl.sum(0)}
    band = (2.0 ** -14 if case.kind == "bf16" else (case.F + 2) * U) * den_z
    amb = v["z"].abs() <= band
    g = (v["gz"] * amb).abs()
    slack = {"dh": g @ W1, "dW1": g.t() @ h, "db1": g.sum(0)}
    r = {k: (out[k], den[k], slack.get(k)) for k in OUTPUTS}
    r["kink"] = float(amb.double().mean())
    r["z"] = v["z"]
    return r


@functools.lru_cache(maxsize=None)
def fp32_formula(case: Case) -> dict:
    return _formula(case, torch.float32)[0]


# ---------------------------------------------------------------------------------------------------------
# the kernels' arithmetic
# ---------------------------------------------------------------------------------------------------------
COMMON = ["no maximum subtraction", "padded classes counted", "fourth class slot dropped", "tail rows' dl not zeroed",
          "backward mask before the dropout", "1/(1-p) forward only", "loss times the scale", "lw missing from dl",
          "db2 placed as if C = 32"]
MUTANTS = {
    "f32": COMMON + ["two-term bf16 split products", "10-bit mantissa operands"],
    "bf16": COMMON + ["W1 lo dropped", "a lo dropped", "W2 lo dropped", "dl lo dropped", "da lo dropped",
                      "lo by truncation", "dh rounded twice"],
}


def _gemm(pairs, kstep: int) -> torch.Tensor:
    """sum over the pairs (A [M, K], Bt [K, N]) as an MFMA chain accumulates it: every kstep-deep slice of every pair,
    in list order, summed (float64 holds it) and added into the fp32 accumulator."""
    A0, B0 = pairs[0]
    acc = torch.zeros(A0.shape[0], B0.shape[1], dtype=torch.float32)
    for k0 in range(0, A0.shape[1], kstep):
        for A, Bt in pairs:
            acc = (acc.double() + A[:, k0:k0 + kstep].double() @ Bt[k0:k0 + kstep].double()).float()
    return acc


def _wacc(acc, pairs, kstep: int):
    """acc [n, P, Q] += A^T B per tile: pairs of (A [n, TR, P], B [n, TR, Q]), kstep rows per MFMA."""
    TR = pairs[0][0].shape[1]
    for k0 in range(0, TR, kstep):
        for A, B in pairs:
            acc = (acc.double() + A[:, k0:k0 + kstep].transpose(1, 2).double() @ B[:, k0:k0 + kstep].double()).float()
    return acc


def _per_workgroup(case: Case, shape, step):
    """Workgroup b walks tiles b, b + grid, .. and keeps its accumulator (:163-165, :512-514): [grid, *shape]."""
    acc = torch.zeros(case.grid, *shape, dtype=torch.float32)
    for t0 in range(0, case.ntiles, case.grid):
        n = min(case.grid, case.ntiles - t0)
        acc[:n] = step(acc[:n], slice(t0, t0 + n))
    return acc


def _reduce8(parts: torch.Tensor) -> torch.Tensor:
    """head_train_reduce_kernel (:357-375): eight groups, each over every 8th partial in order, then the groups."""
    n = parts.shape[0]
    pad = (-n) % 8
    if pad:
        parts = torch.cat([parts, torch.zeros(pad, *parts.shape[1:])])
    p = parts.view(-1, 8, *parts.shape[1:])
    s = torch.zeros_like(p[0])
    for i in range(p.shape[0]):
        s = s + p[i]
    t = s[0]
    for g in range(1, 8):
        t = t + s[g]
    return t


def _butterfly(v: torch.Tensor, offs) -> torch.Tensor:
    idx = torch.arange(v.shape[1])
    for o in offs:
        v = v + v[:, idx ^ o]
    return v[:, :1]


def model(case: Case, mut: Optional[str] = None) -> dict:
    """{output: fp32 tensor} (the bf16 kernel's dh: bf16 values) of the kernel's arithmetic, or of its slip `mut`."""
    assert mut is None or mut in MUTANTS[case.kind], mut
    return _model(case, mut)


@functools.lru_cache(maxsize=None)
def _model(case: Case, mut) -> dict:
    o = operands(case)
    bf = case.kind == "bf16"
    M, C, F, H, TR, nt = case.M, case.C, case.F, case.H, case.TR, case.ntiles
    Mp = nt * TR
    pad = Mp - M
    h = torch.cat([o["h"], torch.zeros(pad, F)])                        # rows past M load as 0 (:139, :510)
    y = torch.cat([o["y"], torch.full((pad,), -1, dtype=torch.int64)])  # :219, :575
    ok = (torch.arange(Mp) < M)[:, None]
    W1, b1, b2 = o["W1"], o["b1"], torch.cat([o["b2"], torch.zeros(TC - C)])   # :208, :498
    W2 = torch.cat([o["W2"], torch.zeros(TC - C, H)])                   # rows >= C zero (:131, :486, :493)
    ik = _f32(drop_scale(case.drop)) if case.drop > 0 else _f32(1.0)    # prepare (:727)
    keep = keep_of(case, Mp) if case.drop > 0 else torch.ones(Mp, H, dtype=torch.bool)
    g = _f32(scale_of(case)) * _f32(lw_of(case))                        # gscale * p.lw (:240, :590)
    if mut == "lw missing from dl":
        g = _f32(scale_of(case))
    trunc = mut == "lo by truncation"

    def split2(v):                                                      # :423-427
        hi = _bf(v)
        return hi, (_trunc_bf(v - hi) if trunc else _bf(v - hi))

    def lo0(pair, name):                                                # the slip that never issues a lo plane
        return (pair[0], torch.zeros_like(pair[1])) if mut == name else pair

    def prod(A, Bt):
        """The fp32 kernel's products: fp32 operands on v_mfma_f32_16x16x4_f32 (:81-83)."""
        if mut == "two-term bf16 split products":
            (Ah, Al), (Bh, Bl) = split2(A), split2(Bt)
            return [(Al, Bh), (Ah, Bl), (Ah, Bh)]
        if mut == "10-bit mantissa operands":
            return [(_cut10(A), _cut10(Bt))]
        return [(A, Bt)]

    # A: z = h W1^T + b1, a = dropout(relu(z))
    if bf:
        W1h, W1l = lo0(split2(W1), "W1 lo dropped")                     # :465-476
        z = _gemm([(h, W1l.t()), (h, W1h.t())], 32) + b1                # :531-532, :538
    else:
        z = _gemm(prod(h, W1.t()), 4) + b1                              # :179-184, :192
    act = z > 0
    a = torch.where(act & keep, z * ik if case.drop > 0 else z, torch.zeros(()))   # :192-193, :539-542
    bwd = act if mut == "backward mask before the dropout" else (a > 0)  # :283 (a > 0); :541 (keep)
    ikb = _f32(1.0) if mut == "1/(1-p) forward only" else ik

    # B: x = a W2^T + b2
    if bf:
        ah, al = lo0(split2(a), "a lo dropped")                         # :544-546
        W2h, W2l = lo0(split2(W2), "W2 lo dropped")                     # :486, :493
        x = _gemm([(al, W2h.t()), (ah, W2l.t()), (ah, W2h.t())], 32) + b2   # :559-561, :566
    else:
        x = _gemm(prod(a, W2.t()), 4) + b2                              # :206, :210

    # C: log-softmax, loss, dl
    cls = torch.arange(TC)[None, :]
    live = cls < C                                                      # :229, :578
    if mut == "fourth class slot dropped" and not bf:
        live = cls < min(C, 24)                                         # u < 3 of the four slots (:227)
    xm = torch.where(live, x, _f32(-math.inf))
    mx = xm.max(1, keepdim=True).values                                 # :230-233, :579-581 (exact in any order)
    if mut == "no maximum subtraction":
        mx = torch.zeros_like(mx)
    e = torch.where(live, torch.exp(xm - mx), torch.zeros(()))          # :236, :582
    if mut == "padded classes counted":
        e = torch.where(cls < C, e, torch.exp(x - mx))                  # a padded logit is 0 + 0
    if bf:
        se = _butterfly(e, (16, 8, 4, 2, 1))                            # :584
    else:
        v = e.view(Mp, 4, 8)                                            # class part + 8 u: u in order (:236)
        se = _butterfly(((v[:, 0] + v[:, 1]) + v[:, 2]) + v[:, 3], (1, 2, 4))   # :238
    lp = (xm - mx) - torch.log(se)                                      # :239, :246, :585, :588
    onehot = (cls == y[:, None])
    okc = live if mut == "tail rows' dl not zeroed" else (ok & live)    # :245, :587
    dl = torch.where(okc, (torch.exp(lp) - onehot.float()) * g, torch.zeros(()))   # :248, :590
    nll = torch.where(ok & live & onehot, -lp, torch.zeros(())).sum(1)  # :247, :589: one class per row
    lossp = _per_workgroup(case, (), lambda acc, t: acc + nll.view(nt, TR)[t].sum(1))
    loss = _reduce8(lossp * _f32(lw_of(case)))                          # block_loss (:97-110), then the reduce
    if mut == "loss times the scale":
        loss = loss * _f32(scale_of(case))

    # D: dW2 += dl^T a, da = (dl W2) mask / (1 - p), db2
    def T(v):                                                           # [Mp, Q] -> [tiles, TR, Q]
        return v.view(nt, TR, v.shape[1])
    if bf:
        dlh, dll = lo0(split2(dl), "dl lo dropped")                     # :594-597
        dW2p = _per_workgroup(case, (TC, H), lambda acc, t: _wacc(
            acc, [(T(dll)[t], T(ah)[t]), (T(dlh)[t], T(al)[t]), (T(dlh)[t], T(ah)[t])], 16))   # :609-611
        W2bh, W2bl = W2h, W2l
        if mut == "fourth class slot dropped":                          # w2b's classes 8 g + e, g = 3 (:493)
            W2bh, W2bl = W2h * (cls.t() < 24), W2l * (cls.t() < 24)
        da = _gemm([(dll, W2bh), (dlh, W2bl), (dlh, W2bh)], 32)   # :619-621
        da = da * torch.where(bwd, ikb, torch.zeros(()))                # dsc (:541, :625)
        db2p = _per_workgroup(case, (TR, TC), lambda acc, t: acc + T(dl)[t])   # db2p (:592)
        db2w = torch.zeros(case.grid, TC)
        for r in range(TR):
            db2w = db2w + db2p[:, r]                                    # :704-707
    else:
        pr2 = [(T(A), T(B)) for A, B in prod(dl, a)]
        dW2p = _per_workgroup(case, (TC, H), lambda acc, t: _wacc(acc, [(A[t], B[t]) for A, B in pr2], 4))   # :261
        da = _gemm(prod(dl, W2), 4)                                     # :270-275
        da = torch.where(bwd, da * ikb, torch.zeros(()))                # :283
        db2w = _per_workgroup(case, (TC,), lambda acc, t: acc + _rows_in_order(T(dl)[t]))   # :286-290

    # E, F: dh = da W1, dW1 += da^T h, db1
    if bf:
        dah, dal = lo0(split2(da), "da lo dropped")                     # :627-630
        if mut == "dh rounded twice":
            dh = _bf(_bf(_gemm([(dah, W1h)], 32)) + _gemm([(dal, W1h), (dah, W1l)], 32))
        else:
            dh = _bf(_gemm([(dal, W1h), (dah, W1l), (dah, W1h)], 32))   # :648-650, :658
        dW1p = _per_workgroup(case, (H, F), lambda acc, t: _wacc(acc, [(T(dal)[t], T(h)[t]), (T(dah)[t], T(h)[t])], 16))  # :668-669

        def db1_step(acc, t):                                           # db1p: rows 4 g + r, r in order (:626)
            d = T(da)[t].view(-1, 4, 4, H)
            for r in range(4):
                acc = acc + d[:, :, r]
            return acc
        db1p = _per_workgroup(case, (4, H), db1_step)
        db1w = ((db1p[:, 0] + db1p[:, 1]) + db1p[:, 2]) + db1p[:, 3]    # :696-699
    else:
        dh = _gemm(prod(da, W1), 4)                                     # :301-307
        pr1 = [(T(A), T(B)) for A, B in prod(da, h)]
        dW1p = _per_workgroup(case, (H, F), lambda acc, t: _wacc(acc, [(A[t], B[t]) for A, B in pr1], 4))   # :322
        db1w = _per_workgroup(case, (H,), lambda acc, t: acc + _rows_in_order(T(da)[t]))     # :327-331

    # the reduce kernel: dW2 rows < C, db2 behind them (:371-374)
    out = {"loss": loss, "dh": dh[:M], "dW1": _reduce8(dW1p), "db1": _reduce8(db1w), "dW2": _reduce8(dW2p)[:C]}
    db2 = _reduce8(db2w)[:C]
    if mut == "db2 placed as if C = 32":
        flat = torch.zeros(TC * H + TC)                                 # the dW2 | db2 end of `grads`, C H + C long
        flat[TC * H:TC * H + C] = db2
        db2 = flat[C * H:C * H + C].clone()
    out["db2"] = db2
    return out


def _rows_in_order(x: torch.Tensor) -> torch.Tensor:
    """Column sums of [n, TR, Q], row after row."""
    s = torch.zeros(x.shape[0], x.shape[2])
    for r in range(x.shape[1]):
        s = s + x[:, r]
    return s


# ---------------------------------------------------------------------------------------------------------
# criteria and bounds
# ---------------------------------------------------------------------------------------------------------
def ulp_bf16(x: torch.Tensor) -> torch.Tensor:
    """The spacing of bf16 (8 significant bits) at |x| (float64); 0 at 0."""
    _, e = torch.frexp(x.abs())
    return torch.where(x != 0, torch.ldexp(torch.ones_like(x), e - 8), torch.zeros_like(x))


def fp32_outputs(case: Case):
    return [k for k in OUTPUTS if not (case.kind == "bf16" and k == "dh")]


def _excess(case: Case, name: str, got: torch.Tensor):
    """|got - ref64| less the kink slack, and den."""
    r64, den, slack = reference(case)[name]
    got = got.double()
    assert got.shape == r64.shape, (name, got.shape, r64.shape)
    d = ((got - r64).abs() - UNDERFLOW).clamp_min(0.0)
    if slack is not None:
        d = (d - slack).clamp_min(0.0)
    return torch.where(torch.isfinite(d), d, torch.full_like(d, math.inf)), den


def measure(case: Case, name: str, got: torch.Tensor):
    """(rms, max) of e = (|got - ref64| - slack)+ / den over every element; a non-finite element counts as inf."""
    d, den = _excess(case, name, got)
    return metric(d, torch.zeros_like(d), den)


def faithful(case: Case, got: torch.Tensor):
    """The bf16 kernel's dh: (elements outside the limit, elements, worst excess / limit)."""
    r64 = reference(case)["dh"][0]
    d, den = _excess(case, "dh", got)
    lim = ulp_bf16(r64) / 2 + (C_SPLIT * 2.0 ** -16 + N_SUM * U) * den
    q = torch.where(lim > 0, d / lim.clamp_min(1e-300), torch.where(d == 0, 0.0, math.inf).double())
    return int((q > 1).sum()), q.numel(), float(q.max())


def ulp_floor(case: Case, name: str):
    """(rms, max) of ulp_fp32(ref64) / den: one ulp of each stored value (see the module's docstring)."""
    r64, den, _ = reference(case)[name]
    _, e = torch.frexp(r64.abs())
    ulp = torch.where(r64 != 0, torch.ldexp(torch.ones_like(r64), e - 24), torch.zeros_like(r64))
    return metric(ulp, torch.zeros_like(ulp), den)


@functools.lru_cache(maxsize=None)
def bounds(case: Case) -> dict:
    """fp32 outputs: {"model", "fp32", "floor", "mutants": {slip: (rms, max)}, "moving": [slips], "mutant_min",
    "bound"}, bound = sqrt(max(model, fp32, floor) mutant_min) for rms and max separately. The bf16 kernel's dh: {"model": (outside, n,
    worst), "mutants": {slip: (outside, n, worst)}}."""
    out = {}
    mod = model(case)
    muts = {m: model(case, m) for m in MUTANTS[case.kind]}
    f32 = fp32_formula(case)
    for name in OUTPUTS:
        if name not in fp32_outputs(case):
            out[name] = {"model": faithful(case, mod[name]), "mutants": {m: faithful(case, v[name]) for m, v in muts.items()}}
            continue
        mm, ff, fl = measure(case, name, mod[name]), measure(case, name, f32[name]), ulp_floor(case, name)
        b = (max(mm[0], ff[0], fl[0]), max(mm[1], ff[1], fl[1]))
        mt = {m: measure(case, name, v[name]) for m, v in muts.items()}
        moving = [m for m, e in mt.items() if all(e[x] > 0 and e[x] >= MOVES * b[x] for x in (0, 1))]
        c = tuple(min((mt[m][x] for m in moving), default=math.nan) for x in (0, 1))
        bound = tuple(0.0 if b[x] == 0 else (math.inf if math.isinf(c[x]) else math.sqrt(b[x] * c[x])) for x in (0, 1))
        out[name] = {"model": mm, "fp32": ff, "floor": fl, "mutants": mt, "moving": moving, "mutant_min": c, "bound": bound}
    return out
