"""The test of the split-bf16 accuracy tests (no GPU): for every case of tests/test_gpu_split_accuracy.py, the host
model of the scheme (tests/split3_ref.py) shows that the bound the GPU test asserts passes a correct six-product
kernel and fails each of the eight one-line slips, with at least 2x of room on either side -- so no mutated kernel
ever has to run on a GPU to know that the GPU test would catch it.

It also records why that test exists: a kernel that drops any second-order term (a2 w0, a1 w1, a0 w2), 16x less
accurate than claimed, stays within the suite's earlier tolerances on at least 99.9 % of the elements.
"""
import functools

import pytest
import torch

import split3_ref as sr

CASE_IDS = [c.id for c in sr.CASES]


def test_split3_is_exact():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(1 << 16, generator=g) * torch.exp2(torch.randint(-40, 40, (1 << 16,), generator=g).float())
    edge = torch.tensor([0.0, -0.0, 1.0, -1.0, 1.0 + 2.0 ** -23, 2.0 - 2.0 ** -23, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -9,
                         1.0 + 2.0 ** -9 + 2.0 ** -23, 255.5, 3.0e38, 1.0e-30])
    for v in (x, edge):
        x0, x1, x2 = sr.split3(v)  # asserts x0 + x1 + x2 == v bit for bit
        for p in (x0, x1, x2):
            assert torch.equal(p, p.to(torch.bfloat16).float())
        assert bool(((x1.abs() <= x0.abs() * 2.0 ** -8) | (x1 == 0)).all())
        assert bool(((x2.abs() <= x0.abs() * 2.0 ** -16) | (x2 == 0)).all())


def test_mutants_are_the_eight_slips():
    assert len(sr.SIX) == 6 and sorted(sr.SIX) == sorted((i, j) for i in range(3) for j in range(3) if i + j <= 2)
    assert len(sr.MUTANTS) == 8
    assert sum(len(t) == 5 for t in sr.MUTANTS.values()) == 6
    assert sr.MUTANTS["a1 w0 for a0 w1"].count((1, 0)) == 2 and (0, 1) not in sr.MUTANTS["a1 w0 for a0 w1"]
    assert sorted(sr.MUTANTS["two-way split"]) == [(0, 0), (0, 1), (1, 0)]


def test_gemm_split_all_nine_products_is_the_exact_product():
    """With all nine products the emulation has no truncation left: it differs from float64 by its fp32 sums alone."""
    g = torch.Generator().manual_seed(2)
    A, W = torch.randn(8, 32, generator=g), torch.randn(4, 32, generator=g)
    nine = [(i, j) for i in range(3) for j in range(3)]
    got = sr.gemm_split(A, W, nine, 32)
    one = (A.double() @ W.double().t())
    # nine roundings of a partial sum <= |A||W|^T each
    assert bool(((got.double() - one).abs() <= 9 * 2.0 ** -24 * (A.double().abs() @ W.double().abs().t())).all())


def test_wgrad_plan_row_splits():
    assert sr.plan_of_x3w(257, 128, 128) == (17, 16)     # 17 splits of one 16-row step, the last with one row
    assert sr.plan_of_x3w(4099, 128, 128) == (129, 32)   # 129 splits of two steps, the last with three rows


@pytest.mark.parametrize("case", sr.CASES, ids=CASE_IDS)
def test_bound_separates_scheme_from_mutants(case):
    o = sr.operands(case)
    for t in [o["Z"], o["dY"]] + [o["prm"][k] for k in sr._W_KEYS]:
        sr.split3(t.contiguous())  # exact on the case's own operands
    b = sr.bounds(case)
    assert set(b) == {"fwd": {"Y"}, "dgrad": {"dZ", "dres"} if case.proj else {"dZ"}, "wgrad": {"dB"},
                      "span": {"dZ", "E"}}[case.kind]
    for name, v in b.items():
        a, m, c, bd = v["fp32"], v["model"], v["mutant_min"], v["bound"]
        what = f"{case.id} {name}: fp32 {a}, model {m}, smallest mutant {c}, bound {bd}"
        # fp32-class: within 2x of the torch fp32 formula in rms (0.3 - 0.9x here). Its max is the largest of a few
        # thousand samples of a matmul whose summation order depends on the host's BLAS and thread count: printed by
        # the GPU test, not a yardstick.
        assert 0 < m[0] <= 2 * a[0], "the six-product scheme is not fp32-class: " + what
        for x in (0, 1):  # rms, max
            assert 2 * m[x] <= bd[x] <= c[x] / 2, "the bound does not separate by 2x on both sides: " + what
        for mut, e in v["mutants"].items():
            assert e[0] >= 4 * m[0] and e[1] >= 3 * m[1], f"mutant '{mut}' {e} too close to the scheme: " + what


@functools.lru_cache(maxsize=None)
def _bare_gemm_pass_fractions(M, K, N):
    """The bare product at one shape: randn A [M, K], 0.1 randn W [N, K], without the second-order terms."""
    g = torch.Generator().manual_seed(1000 + M)
    A, W = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) * 0.1
    A3, W3 = sr.split3(A), sr.split3(W)
    ref = (A.double() @ W.double().t()).float()
    out = {}
    for mut in sr.SECOND_ORDER:
        d = (sr.gemm_split(A3, W3, sr.MUTANTS[mut], sr.KSTEP_FWD) - ref).abs()
        out[mut] = float((d <= 2e-5 + 2e-5 * ref.abs()).double().mean())
    return out


@pytest.mark.parametrize("case", sr.CASES, ids=CASE_IDS)
def test_earlier_tolerance_passes_the_second_order_mutants(case):
    """Why the normalised bound exists: a kernel without a2 w0, a1 w1 or a0 w2 -- 16x less accurate than claimed --
    stays within the suite's earlier tolerances on >= 99.9 % of the elements. Forward, |d| <= 2e-5 + 2e-5 |ref|: on
    the bare product of randn activations and 0.1 randn weights at the case's shape. Gradients, assert_grad_close's
    1e-4 |ref| + 2e-5 max|ref|: on the case's own operands.

    On the forward cases' own operands (two summed 0.1 randn weights and gates up to 3.4 make the outputs about 1.6x
    larger) 0.12 - 0.18 % of the elements leave the earlier tolerance, 5.5 % in the wide-range case: there the earlier
    test sits at its very edge instead of 16x away, so only the floor below is asserted for them."""
    if case.kind == "fwd":
        K = (4 if case.proj else 3) * case.F_in
        for mut, frac in _bare_gemm_pass_fractions(case.M, K, case.F_out).items():
            assert frac >= 0.999, (case.id, "bare product", mut, frac)
    scale = 1.0 / sr.drop_scale(case.drop) if case.drop > 0 else 1.0
    for mut in sr.SECOND_ORDER:
        out = sr.host_model(case, sr.MUTANTS[mut])
        for name in sr.bounds(case):
            frac = sr.old_tolerance_pass_fraction(case, name, out[name].double() * scale)
            floor = 0.999 if case.kind != "fwd" else 0.9 if case.wide else 0.995
            assert frac >= floor, (case.id, name, mut, frac)
