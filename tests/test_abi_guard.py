"""The guarded buffers of abi_guard.py on CPU tensors: a one-element write into each guard region is detected and
located, writes inside the view pass, for every supported dtype."""
import pytest
import torch

import abi_guard as ag

LAYOUTS = [(5, 7, 7, 0), (5, 7, 15, 0), (5, 7, 10, 0), (5, 7, 15, 1), (1, 4, 12, 3)]  # rows, cols, ld, shift


def _poke(g, off):
    """Change one element of the allocation (to a number, so that it differs from the NaN sentinel as bits)."""
    g.buf[off] = 1


@pytest.mark.parametrize("dtype", ag.DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("rows,cols,ld,shift", LAYOUTS)
def test_matrix_guards(dtype, rows, cols, ld, shift):
    g = ag.Guarded(rows, cols, dtype, "cpu", ld=ld, shift=shift)
    assert g.view.shape == (rows, cols) and g.view.stride() == (ld, 1)
    es = g.view.element_size()
    assert (g.ptr() - shift * es) % 64 == 0  # the first row starts aligned: `shift` alone misaligns the view
    assert g.ptr() == g.buf.data_ptr() + (g.front + shift) * es
    g.check()
    g.assert_untouched()
    with pytest.raises(ag.GuardError, match="NaN / unwritten" if dtype != torch.int32 else "unwritten"):
        g.assert_written()

    g.view.fill_(3)  # every element of the view, and nothing else
    g.check()
    g.assert_written()
    with pytest.raises(ag.GuardError, match="must not launch"):
        g.assert_untouched()

    base = g.front + shift
    cases = [(base - shift - 1, "front rows", -1, (ld - shift - 1) % ld),           # last element before row 0
             (0, "front rows", None, None),                                        # first element of the allocation
             (base + rows * ld - shift, "back rows", None, None),                  # row `rows`, first element
             (g.buf.numel() - 1, "back rows", None, None)]
    if ld > cols + shift or (ld > cols and rows > 1):
        cases.append((base + cols, "pad columns", 0, cols))                        # right after row 0
    if ld - shift > cols:
        cases.append((base + (rows - 1) * ld + cols, "pad columns", rows - 1, cols))
    if shift:
        cases.append((g.front, "head of the first row", -1, ld - shift))
        cases.append((base - 1, "head of the first row", -1, ld - 1))
    for off, region, r, c in cases:
        h = ag.Guarded(rows, cols, dtype, "cpu", ld=ld, shift=shift, name="Y")
        h.view.fill_(3)
        _poke(h, off)
        with pytest.raises(ag.GuardError) as e:
            h.check()
        msg = str(e.value)
        assert msg.startswith("Y: 1 guard element") and f"in the {region} at" in msg, (off, msg)
        if r is not None:
            assert f"(row {r}, column {c})" in msg, (off, msg)
        with pytest.raises(ag.GuardError):
            h.assert_written()


@pytest.mark.parametrize("dtype", ag.DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_partial_tile_row_and_wide_store_are_named(dtype):
    """The two stores the guards exist for: row M of a partial tile, and a 4-element store past the last column."""
    g = ag.Guarded(17, 12, dtype, "cpu", ld=20)
    g.view.fill_(1)
    g.buf.as_strided((1, 12), (20, 1), g.front + 17 * 20).fill_(1)  # row 17
    with pytest.raises(ag.GuardError, match=r"12 guard element\(s\) overwritten, first in the back rows at "
                                            r"\(row 17, column 0\)"):
        g.check()
    g = ag.Guarded(17, 10, dtype, "cpu", ld=18)
    g.view.fill_(1)
    g.buf[g.front + 3 * 18 + 8:g.front + 3 * 18 + 12] = 1  # columns 8..11 of row 3: two of them are pad
    with pytest.raises(ag.GuardError, match=r"2 guard element\(s\) overwritten, first in the pad columns at "
                                            r"\(row 3, column 10\)"):
        g.check()


@pytest.mark.parametrize("dtype", ag.DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_input_guards_are_nan(dtype):
    if dtype == torch.int32:
        t = torch.arange(12, dtype=dtype).reshape(3, 4)
    else:
        t = torch.arange(12, dtype=torch.float32).reshape(3, 4).to(dtype)
    g = ag.Guarded.of(t, ld=9, shift=1)
    assert torch.equal(g.view, t)
    g.check()
    g.assert_written()
    outside = g.buf[g._guard]
    assert outside.numel() == g.buf.numel() - 12
    if dtype != torch.int32:
        assert bool(torch.isnan(outside).all())  # a pad folded into a sum poisons it
        assert not bool(torch.isnan(g.view).any())
    # ... with a payload that is not the output sentinel's: an input's guard value (which arithmetic hands on) stored
    # into an output's guard is seen, where the output's own pattern would pass as untouched
    assert ag.INPUT_NAN[dtype] != ag.SENTINEL[dtype][1]
    idt = ag.SENTINEL[dtype][0]
    assert bool((outside.view(idt) == ag.INPUT_NAN[dtype]).all())
    out = ag.Guarded(3, 4, dtype, "cpu", ld=9, shift=1, name="Y")
    out.view.fill_(1)
    out.buf[out.front + 3 * 9 + 1] = g.buf[0]  # row 3, column 0: one row past the view
    with pytest.raises(ag.GuardError, match=r"Y: 1 guard element\(s\) overwritten, first in the back rows at "
                                            r"\(row 3, column 0\)"):
        out.check()
    g.buf[0] = out.buf[0]  # and the other way round
    with pytest.raises(ag.GuardError, match="front rows"):
        g.check()


@pytest.mark.parametrize("dtype", ag.DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_flat_guards(dtype):
    sizes = [1, 3, 16383, 16384, 16385]
    f = ag.GuardedFlat(sizes, dtype, "cpu", gap=8)
    es = f.view.element_size()
    for i, s in enumerate(sizes):
        assert f.views[i].numel() == s and f.ptr(i) % 16 == 0
        if i:
            assert f.starts[i] - (f.starts[i - 1] + sizes[i - 1]) >= 8 * min(1, es)  # a gap between neighbours
    f.check()
    f.assert_untouched()
    for v in f.views:
        v.fill_(2)
    f.check()
    with pytest.raises(ag.GuardError, match="must not launch"):
        f.assert_untouched()
    for i, s in enumerate(sizes):
        for off, what in ((f.starts[i] + s, f"tail of tensor {i} ({s} elements), 1 element"),
                          (f.starts[i] - 1, f"front of tensor {i} ({s} elements), 1 element")):
            h = ag.GuardedFlat(sizes, dtype, "cpu", gap=8, name="sq_partial")
            for v in h.views:
                v.fill_(2)
            h.buf[off] = 1
            with pytest.raises(ag.GuardError) as e:
                h.check()
            assert str(e.value).startswith("sq_partial: 1 guard element") and what in str(e.value), str(e.value)
    h = ag.GuardedFlat(5, dtype, "cpu")
    assert h.view.numel() == 5
    h.buf[-1] = 1
    with pytest.raises(ag.GuardError, match="tail of tensor 0"):
        h.check()


def test_rejects_bad_layouts():
    with pytest.raises(ValueError):
        ag.Guarded(4, 8, torch.float32, "cpu", ld=7)
    with pytest.raises(ValueError):
        ag.Guarded(4, 8, torch.float32, "cpu", ld=8, shift=1)
    with pytest.raises(TypeError):
        ag.Guarded(4, 8, torch.int64, "cpu")
