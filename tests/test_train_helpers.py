"""CPU-side tests (no GPU) of the helpers the trainers share: layer.Bf16InputCache, train.Adam.l2_fold,
ops.deferring_const_grads and the leaf check of ops._defer_const."""
import pytest
import torch


def test_bf16_input_cache():
    from protgram_directgcn_amd.layer import Bf16InputCache
    cache = Bf16InputCache()
    assert cache.buffer is None
    x = torch.arange(32, dtype=torch.float32).view(8, 4)
    xb = cache(x)
    assert xb.dtype == torch.bfloat16 and cache.buffer is xb and torch.equal(xb.float(), x)
    xb[0, 0] = -1.0  # a mark a second conversion would overwrite
    assert cache(x) is xb and float(xb[0, 0]) == -1.0  # same tensor, same version: not converted again
    other = torch.full((8, 4), 3.0)
    ptr = xb.data_ptr()
    x.copy_(other)  # an in-place write bumps the version: converted again, into the same buffer
    assert cache(x) is xb and xb.data_ptr() == ptr and torch.equal(xb.float(), other)
    x.data.fill_(7.0)  # the documented limit: a write through .data bumps no version and is not seen
    assert cache(x) is xb and torch.equal(xb.float(), other)  # the stale values
    assert cache(other) is xb and xb.data_ptr() == ptr  # another tensor of the same shape and device: in place
    small = torch.ones(2, 4)
    xs = cache(small)  # another shape: a new buffer replaces the old one
    assert xs is not xb and cache.buffer is xs and xs.shape == small.shape


def test_model_bf16_input_delegates_to_its_cache(pkg):
    m = pkg.ProtGramDirectGCN([4, 4], 8, 3, 2, 0, 0, 0.0, True)
    x = torch.randn(8, 4)
    assert m.bf16_input(x) is m._xb.buffer and m.bf16_input(x) is m.bf16_input(x)


def test_adam_l2_fold_sets_and_restores():
    from protgram_directgcn_amd import train
    opt = train.Adam([torch.nn.Parameter(torch.zeros(3))], lr=1e-3)
    assert opt._l2_extra == 0.0 and opt._want_sqsum is False
    assert opt._last_sqsum is None and opt._last_sqsum_groups is None
    opt._last_sqsum, opt._last_sqsum_groups = "stale", ["stale"]
    with opt.l2_fold(2e-3, want_sqsum="groups"):
        assert opt._l2_extra == 2e-3 and opt._want_sqsum == "groups"
        assert opt._last_sqsum is None and opt._last_sqsum_groups is None  # the outputs are cleared on entry
    assert opt._l2_extra == 0.0 and opt._want_sqsum is False
    with pytest.raises(KeyError):
        with opt.l2_fold(1.0, want_sqsum=True):
            assert opt._l2_extra == 1.0 and opt._want_sqsum is True
            raise KeyError("inside the block")
    assert opt._l2_extra == 0.0 and opt._want_sqsum is False


def test_deferring_const_grads_restores_and_nests():
    from protgram_directgcn_amd import ops
    assert ops._DEFER_CONST_GRAD is False and not ops._DEFERRED_GRADS
    with pytest.raises(KeyError):
        with ops.deferring_const_grads(True):
            assert ops._DEFER_CONST_GRAD is True
            ops._DEFERRED_GRADS[1234] = torch.zeros(1)
            raise KeyError("inside the block")
    assert ops._DEFER_CONST_GRAD is False and not ops._DEFERRED_GRADS
    with ops.deferring_const_grads(True):
        with ops.deferring_const_grads(False):
            assert ops._DEFER_CONST_GRAD is False
            ops._DEFERRED_GRADS[1234] = torch.zeros(1)
        assert ops._DEFER_CONST_GRAD is True and not ops._DEFERRED_GRADS  # the inner exit restores the outer value
    assert ops._DEFER_CONST_GRAD is False


def test_defer_const_takes_only_leaves_that_require_grad():
    """a non-leaf constant's bf16 gradient would be filed under an address train.Adam never looks
    up, and the real parameter would go unstepped."""
    from protgram_directgcn_amd import ops
    M, F = 6, 4
    leaf = torch.nn.Parameter(torch.randn(M, F))
    frozen = torch.nn.Parameter(torch.randn(M, F), requires_grad=False)
    assert not ops._defer_const(leaf, True, M, None)  # the deferral is off outside a step
    with ops.deferring_const_grads(True):
        assert ops._defer_const(leaf, True, M, None)
        assert not ops._defer_const(leaf * 1.0, True, M, None)
        assert not ops._defer_const(frozen, True, M, None)
        assert not ops._defer_const(leaf, False, M, None) and not ops._defer_const(leaf, True, M + 1, None)
