"""The test of the head-training accuracy tests (no GPU): for every case of tests/test_gpu_head_accuracy.py the host
model of head_train_kernel / head_train5_kernel (tests/head_ref.py) meets the criteria the GPU test asserts, and each
one-line slip of that arithmetic fails them on at least one case with room: a normalised metric (rms and max) at least
2x above the bound of an fp32 output, or at least 1 % of the elements of the bf16 kernel's dh outside a limit that
admits none. ('dh rounded twice' can be caught in no other way: a second rounding at most doubles the worst error of
one, so no bound sits 2x above the one and 2x below the other; the +-120 case, whose softmax is one-hot and so adds
nothing to the limit's a priori term, is where the limit is tight enough to see it.) So no mutated kernel has to run
on a GPU to know that the GPU test would catch it.

Also per case: the ReLU-kink cap, den > 0 wherever the reference is nonzero, the exact zeros of dead hidden units and
of the +-120 case's saturated rows, and that 'no maximum subtraction' is non-finite there while the model is not.
"""
import math

import pytest
import torch

import head_ref as hr

CASE_IDS = [c.id for c in hr.CASES]
SLIPS = [(k, m) for k in ("f32", "bf16") for m in hr.MUTANTS[k]]


def test_tables():
    assert {k: len(v) for k, v in hr.MUTANTS.items()} == {"f32": 11, "bf16": 16}
    assert len({c.id for c in hr.CASES}) == len(hr.CASES) == 32
    for cases, TR in ((hr.F32, 64), (hr.BF16, 16)):
        assert {c.C for c in cases} == {1, 2, 7, 8, 9, 16, 17, 20, 24, 25, 31, 32}
        assert {c.M for c in cases if c.C != 31 or c.drop} == {TR + 1, 2 * TR + 1, 257 * TR + 1}
        assert {c.M for c in cases if c.C == 31 and not c.drop} == {1, TR - 1, TR}
        big = [c for c in cases if c.M == 257 * TR + 1]
        assert [(c.C, c.ntiles, c.grid) for c in big] == [(25, 258, 256)]   # workgroups 0, 1 walk a second tile
        assert {c.labels for c in cases} == {"uniform", "last", "first"}
        assert sorted(c.drop for c in cases if c.drop) == [0.5, 0.9]
        assert [c.drop_seed < 0 for c in cases if c.drop] == [False, True]
        assert [(c.scale, c.weight) for c in cases if c.scale] == [(65536.0, 0.75)]
        assert sum(c.hard for c in cases) == 1 and sum(c.units for c in cases) == 1


def test_drop_keep_threshold_is_the_abi_floats():
    """prepare() computes ceil(p 2^24) from the float the ABI carries: 0.9f 2^24 is the integer 15099494, the double
    0.9 2^24 is 15099494.4 (ceil: one more). The host draw takes the former."""
    k = hr._drop_keep(7, 4096, 64, 0.9)
    assert 0.08 < float(k.double().mean()) < 0.12
    assert int(math.ceil(float(torch.tensor(0.9, dtype=torch.float32)) * 2 ** 24)) == 15099494
    assert torch.equal(hr._drop_keep(-1, 8, 64, 0.5), hr._drop_keep(2 ** 64 - 1, 8, 64, 0.5))   # an int64's 64 bits


def test_split_pieces():
    g = torch.Generator().manual_seed(5)
    v = torch.randn(1 << 14, generator=g) * torch.exp2(torch.randint(-20, 20, (1 << 14,), generator=g).float())
    hi = hr._bf(v)
    lo = hr._bf(v - hi)
    assert bool(((v.double() - hi.double() - lo.double()).abs() <= 2.0 ** -16 * v.double().abs()).all())
    assert bool((hr._trunc_bf(v).abs() <= v.abs()).all()) and torch.equal(hr._trunc_bf(hi), hi)
    assert torch.equal(hr._cut10(hi), hi) and bool(((hr._cut10(v) - v).abs() <= 2.0 ** -10 * v.abs()).all())


@pytest.mark.parametrize("case", hr.CASES, ids=CASE_IDS)
def test_criteria_pass_the_model(case):
    o = hr.operands(case)
    if case.kind == "bf16":
        assert torch.equal(o["h"], hr._bf(o["h"]))                       # exactly bf16-valued
    assert int(o["y"].min()) >= 0 and int(o["y"].max()) < case.C
    ref = hr.reference(case)
    assert ref["kink"] <= hr.KINK_CAP, f"{case.id}: {ref['kink']:.5f} of the pre-activations in the kink band"
    for name in hr.OUTPUTS:
        r64, den, _ = ref[name]
        assert bool(torch.isfinite(r64).all()) and bool((den[r64 != 0] > 0).all()), name
    b = hr.bounds(case)
    mod = hr.model(case)
    for name, v in b.items():
        what = f"{case.id} {name}: " + str({k: x for k, x in v.items() if k != "mutants"})
        if name not in hr.fp32_outputs(case):
            assert v["model"][0] == 0 and v["model"][2] <= 1, "the model's dh is outside its limit: " + what
            continue
        assert v["moving"], "no slip moves the output: " + what
        for x in (0, 1):  # rms, max
            assert math.isfinite(v["bound"][x]) and math.isfinite(v["mutant_min"][x]) or v["bound"][x] == 0, what
            base = max(v["model"][x], v["fp32"][x], v["floor"][x])
            assert base <= v["bound"][x] and (v["bound"][x] == 0 or 2 * base <= v["bound"][x]), "no 2x below the bound: " + what
    if case.units:
        z = ref["z"]
        assert bool((z[:, list(hr.DEAD)] < 0).all()) and bool((z[:, list(hr.LIVE)] > 0).all())
        assert not bool(mod["dW1"][list(hr.DEAD)].any()) and not bool(mod["db1"][list(hr.DEAD)].any())
        assert bool(mod["dW1"][list(hr.LIVE)].any(1).all())
    if case.hard:
        assert float(torch.log_softmax(ref["z"].clamp_min(0) @ o["W2"].double().t() + o["b2"].double(), 1).min()) < -200
        assert all(bool(torch.isfinite(mod[n]).all()) for n in hr.OUTPUTS)
        bad = hr.model(case, "no maximum subtraction")
        assert not all(bool(torch.isfinite(bad[n]).all()) for n in hr.OUTPUTS)
        rows = o["y"] == case.C - 1                                        # softmax == onehot(y): dl rounds to 0
        assert int(rows.sum()) >= case.M // 3 and not bool(mod["dh"][rows].any())
        assert bool(mod["dh"][~rows].any(1).all())


def slip_hits(kind: str, mut: str):
    """[(case id, output, slip / bound or share outside)] where the slip fails the criteria with room."""
    hits = []
    for case in (hr.F32 if kind == "f32" else hr.BF16):
        for name, v in hr.bounds(case).items():
            e = v["mutants"][mut]
            if name not in hr.fp32_outputs(case):
                if e[0] >= 0.01 * e[1]:
                    hits.append((case.id, name, f"{100.0 * e[0] / e[1]:.1f} % outside"))
            elif mut in v["moving"] and all(e[x] >= 2 * v["bound"][x] for x in (0, 1)):
                r = [math.inf if v["bound"][x] == 0 else e[x] / v["bound"][x] for x in (0, 1)]
                hits.append((case.id, name, f"{min(r):.3g}x"))
    return hits


@pytest.mark.parametrize("kind,mut", SLIPS, ids=[f"{k}-{m}" for k, m in SLIPS])
def test_every_slip_fails(kind, mut):
    hits = slip_hits(kind, mut)
    print(f"\nHEAD_SLIP {kind:4s} '{mut}': fails {len(hits)} case outputs, e.g. " +
          ", ".join(f"{c} {n} ({r})" for c, n, r in hits[:3]))
    assert hits, f"{kind} '{mut}' passes the criteria of every case"
