"""The operand gate of ndcn_amd/ops.py driven with host tensors: `_layout` is the part that asks nothing of the device (dtype, exact
shape or element count, strides; inputs are made contiguous, outputs never copied), `_on_device` the rest.  What a GPU test must not
do - a shorter tensor, a host tensor, a tensor of the wrong kind - is refused here, where nothing is launched."""
import pytest
import torch

from ndcn_amd import _lib, ops
from ndcn_amd.ops import _layout, _on_device, _operand


def refused(what, *needles):
    class ctx:
        def __enter__(self):
            self.r = pytest.raises(_lib.NdcnHipError)
            self.e = self.r.__enter__()
            return self.e

        def __exit__(self, *exc):
            out = self.r.__exit__(*exc)
            assert self.e.value.code == _lib.EINVAL
            text = str(self.e.value)
            assert 'operand %s' % what in text, text
            for n in needles:
                assert n in text, text
            return out
    return ctx()


def test_a_conforming_operand_is_returned_as_it_is():
    t = torch.arange(12, dtype=torch.float32).view(3, 4)
    for kw in ({}, {'shape': (3, 4)}, {'numel': 12}, {'shape': (3, 4), 'numel': 12, 'out': True}, {'out': True}):
        assert _layout(t, 'y0', **kw) is t
    i = torch.arange(5, dtype=torch.int32)
    assert _layout(i, 'idx', dtype=torch.int32, numel=5) is i
    acc = torch.zeros(7, dtype=torch.float64)
    assert _layout(acc, 'acc', dtype=torch.float64, numel=7, out=True) is acc


@pytest.mark.parametrize('dtype', [torch.float64, torch.float16, torch.int32, torch.int64])
def test_dtype_alone(dtype):
    with refused('y0', 'torch.float32', str(dtype)):
        _layout(torch.zeros(3, 4, dtype=dtype), 'y0')
    with refused('idx', 'torch.int32'):
        _layout(torch.zeros(3, dtype=torch.int64), 'idx', dtype=torch.int32)
    with refused('idx', 'torch.int32'):
        _layout(torch.zeros(3, dtype=torch.float32), 'idx', dtype=torch.int32)


def test_shape_alone():
    t = torch.zeros(3, 4)
    for bad in ((4, 3), (12,), (3, 5), (2, 4), (3, 4, 1)):
        with refused('out_K', 'shape %s' % (bad,), '(3, 4)'):
            _layout(t, 'out_K', shape=bad)
    assert _layout(t, 'out_K', shape=torch.Size((3, 4))) is t


def test_element_count_alone():
    t = torch.zeros(3, 4)
    for bad in (11, 13, 0):
        with refused('y0', '%d elements' % bad):
            _layout(t, 'y0', numel=bad)
    assert _layout(t.view(12), 'y0', numel=12).shape == (12,)           # any shape of that count


def test_an_input_that_needs_it_comes_back_contiguous_with_equal_values():
    big = torch.arange(48, dtype=torch.float32).view(6, 8)
    for view in (big[:, ::2], big.t(), big[::2], big[1:5, 2:6]):
        assert not view.is_contiguous()
        got = _layout(view, 'X', shape=view.shape)
        assert got.is_contiguous() and got.data_ptr() != view.data_ptr() and torch.equal(got, view)
    row_slice = big[2:4]                                                 # contiguous views are not copied
    assert _layout(row_slice, 'X') is row_slice


def test_an_output_is_never_copied():
    big = torch.zeros(6, 8)
    for view in (big[:, ::2], big.t(), big[::2]):
        with refused('out', 'contiguous output', 'strides'):
            _layout(view, 'out', out=True)
    mid = big.view(-1)[8:32].view(3, 8)
    assert _layout(mid, 'out', shape=(3, 8), out=True) is mid


def test_expectations_in_combination_report_the_first_that_fails():
    big = torch.zeros(6, 8, dtype=torch.float64)
    with refused('out', 'torch.float32'):                                # dtype before shape before strides
        _layout(big[:, ::2], 'out', shape=(3, 4), out=True)
    with refused('out', 'shape (3, 4)'):
        _layout(big.float()[:, ::2], 'out', shape=(3, 4), out=True)
    with refused('out', 'contiguous output'):
        _layout(big.float()[:, ::2], 'out', shape=(6, 4), numel=24, out=True)
    with refused('out', '25 elements'):
        _layout(big.float()[:, ::2], 'out', shape=(6, 4), numel=25, out=True)


def test_not_a_tensor_and_indexed_names():
    with refused('y0', 'a tensor', 'NoneType'):
        _layout(None, 'y0')
    with refused('ks[2]', 'torch.float32'):
        _layout(torch.zeros(2, dtype=torch.float64), ('ks', 2))
    with refused('ks[2]', 'a tensor', 'list'):
        _on_device([1.0], ('ks', 2))


def test_the_device_part_refuses_host_tensors_whatever_else_holds():
    t = torch.zeros(3, 4)
    for fn in (lambda: _on_device(t, 'kprev[1]'), lambda: _operand(t, ('kprev', 1), shape=(3, 4)),
               lambda: _operand(t, ('kprev', 1), device=torch.device('cuda', 0))):
        with pytest.raises(_lib.NdcnHipError) as e:
            fn()
        assert e.value.code == _lib.EINVAL and 'kprev[1]' in str(e.value) and 'cpu' in str(e.value) and 'no CPU fallback' in str(e.value)


def test_every_wrapper_refuses_a_host_primary_before_anything_else():
    """no wrapper reaches the library with a host tensor (none is loaded here: a call that got past the gate would fail differently)"""
    t = torch.ones(4, 4)
    hip = ops.hip
    calls = [lambda: hip.combine(t, [t], [1.0]), lambda: hip.copy(t), lambda: hip.scale(t, 2.0), lambda: hip.linear(t, t),
             lambda: hip.relu_bwd(t, t), lambda: hip.dropout_apply(t, (0.5, 1, 0)), lambda: hip.lincomb([t], [1.0]),
             lambda: hip.rhs(None, t, t, None, no_graph=True), lambda: hip.rhs_rk(None, t, t, None, 'combine', t, [], [1.0], no_graph=True),
             lambda: hip.ab_step(t, [t], [1.0], 0.1), lambda: hip.interp_eval((t, t, t, t), t, [1.0] * 5),
             lambda: hip.row_l1_normalize(t), lambda: hip.tick_emit(t, 0.1, [0.05]), lambda: hip.fixed_stage(0, t, t, dt=0.1)]
    for call in calls:
        with pytest.raises(_lib.NdcnHipError) as e:
            call()
        assert e.value.code == _lib.EINVAL and 'cpu' in str(e.value)
