"""Every tensor operand of every HipOps method against the operand gate of ndcn_amd/ops.py: one table row per method.

The C calls carry no tensor sizes, so a wrapper that forgets a check hands a kernel a pointer it reads or writes as a dense float32
array of the launch's extent.  Three things are tested for each row (a builder of valid operands at a tiny shape: a weighted ring
operator of 70 rows at widths 8 and 20, 130 rows at width 256 where a method only exists there, T = 3 for the TemporalGCN calls):

  refusals     each operand replaced by a bad one must raise NdcnHipError, and every ndcn_debug_last_*_path word must read the same
               before and after: nothing was launched.
  equivalents  an input that legitimately arrives as a non-contiguous view (the gate copies it) or as a 1-D panel gives, bit for bit,
               the result of its contiguous clone; spmm / linear / rhs / combine also stay inside their float64 bounds.
  outputs      a caller's output that is a contiguous slice in the middle of a NaN-filled buffer: exactly the slice is written (it equals
               the fresh result, the guard elements on both sides are still NaN) and the returned tensor IS that slice.

THE MEMORY-SAFETY RULE.  A missing check must show up here as a failed assertion, never as a fault on a shared card.  Every bad operand
is therefore safe even for a wrapper that wrongly accepted it - only these kinds exist:
  * a float64 (int64 for index tensors) tensor of the SAME shape: more bytes than the launch touches;
  * a tensor of the right dtype with MORE rows or columns than needed;
  * a non-contiguous view ([:, ::2] or [::2]) of a LARGER allocation whose dense extent from its data_ptr() stays inside it.
Never a shorter tensor, a host tensor, another device or a null: tests/test_ops_operands_host.py covers those expectations where
nothing can be launched.  Operands from which a launch derives its sizes get the dtype kind alone (a larger one would make the kernel
read the OTHER operands past their ends).  `_bad` asserts the rule on untyped_storage().nbytes() for every tensor it hands out."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from ndcn_amd import _lib, graphs, hip
from ndcn_amd.csr import CsrOperator
from ndcn_amd.ops import HipOps

from _fma_chain import chain, dot_bound, spmm_bound, sum_bound

pytestmark = pytest.mark.gpu

GUARD = 8           # guard elements on each side of an output slice (a multiple of 4: the slice keeps the 16-byte lanes)
PATHS = ('ndcn_debug_last_rhs_path', 'ndcn_debug_last_small_route', 'ndcn_debug_last_linear_path', 'ndcn_debug_last_rk_bwd_path',
         'ndcn_debug_last_spmm_path', 'ndcn_debug_last_rk_path', 'ndcn_debug_last_rhs_vjp_path', 'ndcn_last_readout_path')
NO_TENSORS = {'set_rhs_mid', 'set_rhs_mid_drop', 'set_rhs_abl', 'set_solver_mid', 'set_rhs_mid_bwd', 'set_rhs_abl_bwd', 'set_tgcn_fused',
              'set_adams_fused', 'set_adams_readout', 'rhs_abl_bwd_on', 'tgcn_fused_on', 'adams_fused_on', 'adams_readout_on',
              'solver_mid_mode', 'rhs_adj_supported', 'tgcn_chunk', 'adams_readout_route', 'new_error_record', 'solver_mid_takes',
              'adams_fusable'}       # adams_fusable reads its panels' attributes and answers: no pointer of theirs is passed on


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda', 0)


def ring(n):
    """weighted ring: row i holds (i - 1, i, i + 1) mod n, in stored column order"""
    rng = np.random.default_rng(n)
    i = np.arange(n)
    rows = np.repeat(i, 3)
    cols = np.stack([(i - 1) % n, i, (i + 1) % n], 1).reshape(-1)
    m = sp.csr_matrix((rng.uniform(-1, 1, 3 * n).astype(np.float32), (rows, cols)), shape=(n, n))
    m.sort_indices()
    return m


class Ctx:
    """valid operands of one row: deterministic, fresh tensors at every build (in-place operands are consumed by a call)"""
    _ops = {}

    def __init__(self, dev, H):
        grid = H == 'grid'              # width 256 on the 24 x 24 lattice: the operator whose plan has the x_mask / s_out / xadd launches
        self.dev, self.H = dev, 256 if grid else H
        self.n = 576 if grid else 130 if H == 256 else 70
        key = (self.n, str(dev))
        if key not in Ctx._ops:
            m = graphs.normalized_laplacian(graphs.grid_8_neighbor(24)).tocsr() if grid else ring(self.n)
            Ctx._ops[key] = (m, CsrOperator.from_scipy(m, dev))
        self.ring, self.A = Ctx._ops[key]
        self.g = torch.Generator().manual_seed(1000 + self.H)

    def t(self, *shape):
        return (torch.rand(*shape, generator=self.g) * 2 - 1).to(self.dev)

    def P(self):
        return self.t(self.n, self.H)

    def Ps(self, k):
        return [self.P() for _ in range(k)]


class Call:
    def __init__(self, fn, ops, sizes=(), outs=None, inout=None, dtypes=None):
        self.fn = fn                    # fn(o): o maps operand names to tensors / lists; an output that is not supplied is absent
        self.ops = ops
        self.sizes = set(sizes)         # operands the launch derives its sizes from: the dtype kind alone
        self.outs = outs or {}          # pure outputs: name -> (shape, where the tensor comes back in the result)
        self.inout = inout or {}        # operands written in place (or kept as views: never copied): name -> where, or None
        self.dtypes = dtypes or {}


def names(ops):
    for k, v in ops.items():
        if isinstance(v, (list, tuple)):
            for j in sorted({0, len(v) - 1}):
                yield '%s.%d' % (k, j)
        elif v is not None:
            yield k


def get(ops, name):
    k, _, j = name.partition('.')
    return ops[k][int(j)] if j else ops[k]


def put(ops, name, value):
    ops = dict(ops)
    k, _, j = name.partition('.')
    if j:
        ops[k] = list(ops[k])
        ops[k][int(j)] = value
    else:
        ops[k] = value
    return ops


def pick(result, where):
    for j in where:
        result = result[j]
    return result


def flat(result):
    if isinstance(result, torch.Tensor) or not isinstance(result, (list, tuple)):
        return [result]
    return [x for r in result for x in flat(r)]


def same(a, b):
    a, b = flat(a), flat(b)
    assert len(a) == len(b)
    for x, y in zip(a, b):
        if isinstance(x, torch.Tensor):
            assert isinstance(y, torch.Tensor) and x.shape == y.shape and torch.equal(x, y)
        else:
            assert x == y


def strided(t, fill=True):
    """a non-contiguous view of t's shape and values inside a larger allocation"""
    if t.dim() >= 2:
        big = torch.zeros(t.shape[:-1] + (2 * t.shape[-1],), dtype=t.dtype, device=t.device)
        v = big[..., ::2]
    else:
        big = torch.zeros(2 * t.numel(), dtype=t.dtype, device=t.device)
        v = big[::2].view(t.shape) if t.dim() == 1 else big[::2][0]
    if fill:
        v.copy_(t)
    return v


def _bad(valid, kind):
    """one of the three memory-safe kinds of bad operand (module docstring), or None where the kind does not apply"""
    wide = {torch.float32: torch.float64, torch.int32: torch.int64, torch.float64: torch.complex128}[valid.dtype]
    if kind == 'dtype':
        bad = torch.zeros(valid.shape, dtype=wide, device=valid.device)
    elif kind == 'rows':
        if valid.dim() == 0:
            return None
        bad = torch.zeros((valid.shape[0] + 1,) + tuple(valid.shape[1:]), dtype=valid.dtype, device=valid.device)
    elif kind == 'cols':
        if valid.dim() < 2:
            return None
        bad = torch.zeros(tuple(valid.shape[:-1]) + (valid.shape[-1] + 1,), dtype=valid.dtype, device=valid.device)
    else:
        bad = strided(valid, fill=False)
        if bad.is_contiguous():
            return None
    touched = valid.numel() * valid.element_size()                       # what the launch reads or writes through this pointer
    left = bad.untyped_storage().nbytes() - bad.storage_offset() * bad.element_size()
    assert left >= touched and bad.device == valid.device, 'the memory-safety rule of this module'
    return bad


def paths():
    lib = _lib.load()
    return tuple(int(getattr(lib, p)()) for p in PATHS)


def scramble(dev):
    """launches unlike any row's, so that a launch a refusal failed to stop would move a path word"""
    x = torch.ones(5, device=dev)
    hip.scale(x, 2.0)
    hip.linear(torch.ones(3, 5, device=dev), torch.ones(2, 5, device=dev))
    hip.spmm(Ctx(dev, 8).A, torch.ones(70, 3, device=dev))
    hip.dot_diff(x, x)


# ---------------------------------------------------------------------------------------------------------------- the table
CS7 = [0.2, -0.1, 0.3, 0.05, -0.25, 0.15, 0.1]
XP = [0.5, 0.25, 0.125, 0.0625, 0.03125]
DROP = (0.3, 7, 2)
ROWS = {}


def row(name, widths=(8, 20)):
    def deco(f):
        ROWS[name] = (f, widths)
        return f
    return deco


def lin_ops(c):
    return {'W': c.t(c.H, c.H), 'b': c.t(c.H)}


@row('spmm')
def _(c):
    return Call(lambda o: hip.spmm(c.A, o['X'], out=o.get('out')), {'X': c.P()}, sizes={'X'}, outs={'out': ((c.n, c.H), ())})


@row('spmm:halo')
def _(c):
    """the ring's columns 60.. address the halo panel"""
    return Call(lambda o: hip.spmm(c.A, o['X'], X_halo=o['X_halo']), {'X': c.t(60, c.H), 'X_halo': c.t(10, c.H)}, sizes={'X'})


@row('adjoint_rhs')
def _(c):
    return Call(lambda o: hip.adjoint_rhs(c.A, o['y'], o['a'], o['W'], o['b']), {'y': c.P(), 'a': c.P(), **lin_ops(c)}, sizes={'y'})


@row('gcn')
def _(c):
    return Call(lambda o: hip.gcn(c.A, o['X'], o['W'], o['b']), {'X': c.P(), 'W': c.t(12, c.H), 'b': c.t(12)}, sizes={'X', 'W'})


@row('linear')
def _(c):
    return Call(lambda o: hip.linear(o['S'], o['W'], o['b']), {'S': c.P(), 'W': c.t(12, c.H), 'b': c.t(12)}, sizes={'S', 'W'})


@row('linear_bwd')
def _(c):
    return Call(lambda o: hip.linear_bwd(o['g'], o['W'], o['S'], o['Y']),
                {'g': c.t(c.n, 12), 'W': c.t(12, c.H), 'S': c.P(), 'Y': c.t(c.n, 12)}, sizes={'g', 'W'})


@row('relu_bwd')
def _(c):
    return Call(lambda o: hip.relu_bwd(o['g'], o['y']), {'g': c.P(), 'y': c.P()}, sizes={'g'})


@row('copy')
def _(c):
    return Call(lambda o: hip.copy(o['x'], out=o.get('out')), {'x': c.P()}, sizes={'x'}, outs={'out': ((c.n, c.H), ())})


@row('scale')
def _(c):
    return Call(lambda o: hip.scale(o['x'], 0.75), {'x': c.P()}, sizes={'x'})


@row('rhs')
def _(c):
    return Call(lambda o: hip.rhs(c.A, o['X'], o['W'], o['b'], out=o.get('out')), {'X': c.P(), **lin_ops(c)}, sizes={'X'},
                outs={'out': ((c.n, c.H), ())})


@row('rhs:halo')
def _(c):
    """the ring's columns 60.. address the halo panel"""
    return Call(lambda o: hip.rhs(c.A, o['X'], o['W'], o['b'], X_halo=o['X_halo']),
                {'X': c.t(60, c.H), 'X_halo': c.t(10, c.H), **lin_ops(c)}, sizes={'X'})


@row('rhs:no_control')
def _(c):
    return Call(lambda o: hip.rhs(c.A, o['X'], None, None, no_control=True, out=o.get('out')), {'X': c.P()}, sizes={'X'},
                outs={'out': ((c.n, c.H), ())})


@row('rhs:no_graph')
def _(c):
    return Call(lambda o: hip.rhs(None, o['X'], o['W'], o['b'], no_graph=True, out=o.get('out')), {'X': c.P(), **lin_ops(c)}, sizes={'X'},
                outs={'out': ((c.n, c.H), ())})


@row('rhs:dropout')
def _(c):
    return Call(lambda o: hip.rhs(c.A, o['X'], o['W'], o['b'], out=o.get('out'), dropout=DROP), {'X': c.P(), **lin_ops(c)}, sizes={'X'},
                outs={'out': ((c.n, c.H), ())})


@row('dropout_apply')
def _(c):
    return Call(lambda o: hip.dropout_apply(o['K'], DROP), {'K': c.P()}, sizes={'K'}, inout={'K': ()})


@row('dropout_combine')
def _(c):
    return Call(lambda o: hip.dropout_combine(o['K'], DROP, o['kprev'], [0.1, 0.2, 0.3], y0=o['y0'], out=o.get('out')),
                {'K': c.P(), 'kprev': c.Ps(2), 'y0': c.P()}, sizes={'K'}, outs={'out': ((c.n, c.H), (1,))},
                inout={'K': (0,), 'kprev.0': None, 'kprev.1': None})


def rhs_rk_row(mode, **kw):
    def build(c):
        nk = 2
        cs = [0.25] if mode == 'rk4' else [0.1, 0.2, 0.3]
        outs = {'out_K': ((c.n, c.H), (0,))}
        extra = dict(kw)
        halo, A = extra.pop('halo', False), None if kw.get('no_graph') else c.A
        ops = {'X': c.t(60, c.H) if halo else c.P(), 'y0': c.P(), 'kprev': c.Ps(nk)}
        if halo:
            ops['X_halo'] = c.t(10, c.H)                 # the ring's columns 60..
        if not kw.get('no_control'):
            ops.update(lin_ops(c))
        if mode != 'error':
            outs['out_y'] = ((c.n, c.H), (1,))
        else:
            ops['y1'] = c.P()
            extra.update(rtol=1e-2, atol=1e-3)
        if 'aux_cs' in kw:
            outs['out_aux'] = ((c.n, c.H), (2,))
        return Call(lambda o: hip.rhs_rk(A, o['X'], o.get('W'), o.get('b'), mode, o['y0'], o['kprev'], cs, y1=o.get('y1'),
                                         X_halo=o.get('X_halo'), out_K=o.get('out_K'), out_y=o.get('out_y'), out_aux=o.get('out_aux'),
                                         **extra), ops, sizes={'X'}, outs=outs)
    return build


row('rhs_rk:combine')(rhs_rk_row('combine', aux_cs=[0.3, 0.2, 0.1]))
row('rhs_rk:rk4')(rhs_rk_row('rk4'))
row('rhs_rk:error')(rhs_rk_row('error'))
row('rhs_rk:dropout')(rhs_rk_row('combine', dropout=DROP))
row('rhs_rk:wide', widths=(256,))(rhs_rk_row('combine'))
row('rhs_rk:halo')(rhs_rk_row('combine', halo=True))
row('rhs_rk:halo_error')(rhs_rk_row('error', halo=True))
row('rhs_rk:no_control')(rhs_rk_row('combine', no_control=True))
row('rhs_rk:no_graph')(rhs_rk_row('rk4', no_graph=True))


def rhs_rk_adj_row(which):
    """x_mask or s_out (ndcn_rhs_rk_adj_f32 takes one of the two) on the lattice, whose plan has that launch; S = A X comes back in
    s_out with the bits of spmm"""
    def build(c):
        assert hip.rhs_adj_supported(c.A, c.H, 'combine', 1)

        def fn(o):
            if which == 'x_mask':
                return hip.rhs_rk(c.A, o['X'], o['W'], o['b'], 'combine', o['y0'], o['kprev'], [0.1, 0.2], x_mask=o['x_mask'])
            S = o['s_out'] if 's_out' in o else torch.empty(c.n, c.H, device=c.dev)
            K, y = hip.rhs_rk(c.A, o['X'], o['W'], o['b'], 'combine', o['y0'], o['kprev'], [0.1, 0.2], s_out=S)
            assert torch.equal(S, hip.spmm(c.A, o['X']))
            return K, y, S
        ops = {'X': c.P(), **lin_ops(c), 'y0': c.P(), 'kprev': c.Ps(1)}
        if which == 'x_mask':
            ops['x_mask'] = c.P()
        return Call(fn, ops, sizes={'X'}, outs={'s_out': ((c.n, c.H), (2,))} if which == 's_out' else {})
    return build


row('rhs_rk:x_mask', widths=('grid',))(rhs_rk_adj_row('x_mask'))
row('rhs_rk:s_out', widths=('grid',))(rhs_rk_adj_row('s_out'))


@row('rhs_vjp')
def _(c):
    return Call(lambda o: hip.rhs_vjp(c.A, o['X'], o['W'], o['K'], o['g'], S=o['S'], gW=o['gW'], gb=o['gb'], acc_scale=0.5),
                {'X': c.P(), 'W': c.t(c.H, c.H), 'K': c.P(), 'g': c.P(), 'S': c.P(), 'gW': c.t(c.H, c.H), 'gb': c.t(c.H)}, sizes={'X'},
                inout={'gW': (1,), 'gb': (2,)})


@row('rhs_vjp:no_control')
def _(c):
    return Call(lambda o: hip.rhs_vjp(c.A, o['X'], None, o['K'], o['g'], S=o['S'], no_control=True),
                {'X': c.P(), 'K': c.P(), 'g': c.P(), 'S': c.P()}, sizes={'X'})


@row('rhs_vjp:no_graph')
def _(c):
    return Call(lambda o: hip.rhs_vjp(None, o['X'], o['W'], o['K'], o['g'], gW=o['gW'], gb=o['gb'], no_graph=True),
                {'X': c.P(), 'W': c.t(c.H, c.H), 'K': c.P(), 'g': c.P(), 'gW': c.t(c.H, c.H), 'gb': c.t(c.H)}, sizes={'X'},
                inout={'gW': (1,), 'gb': (2,)})


@row('rhs_rk_xadd', widths=('grid',))
def _(c):
    assert hip.rhs_rk_xadd(c.A, c.P(), c.P(), 0.5, c.t(c.H, c.H), c.t(c.H), c.P(), c.P(), [0.1, 0.2]) is not None
    return Call(lambda o: hip.rhs_rk_xadd(c.A, o['X'], o['xadd'], 0.5, o['W'], o['b'], o['y0'], o['k_prev'], [0.1, 0.2]),
                {'X': c.P(), 'xadd': c.P(), **lin_ops(c), 'y0': c.P(), 'k_prev': c.P()}, sizes={'X'})


@row('gather_rows')
def _(c):
    idx = torch.tensor([3, 0, 69, 17, 17], dtype=torch.int32, device=c.dev)
    return Call(lambda o: hip.gather_rows(o['X'], o['idx']), {'X': c.P(), 'idx': idx}, sizes={'X', 'idx'})


@row('combine')
def _(c):
    return Call(lambda o: hip.combine(o['y0'], o['ks'], [0.1, -0.2, 0.3]), {'y0': c.P(), 'ks': c.Ps(3)}, sizes={'y0'})


@row('lincomb')
def _(c):
    return Call(lambda o: hip.lincomb(o['ks'], [0.1, -0.2, 0.3], y0=o['y0']), {'ks': c.Ps(3), 'y0': c.P()}, sizes={'ks.0'})


@row('readout_bwd')
def _(c):
    C = 3
    return Call(lambda o: (hip.readout_bwd(o['gd'], o['Wd'], y=o['y'], base=o['base'], addends=o['addends'], acc=o['acc']), o['acc']),
                {'gd': c.t(c.n, C), 'Wd': c.t(C, c.H), 'y': c.P(), 'base': c.P(), 'addends': c.Ps(2),
                 'acc': torch.zeros(C * c.H + C, dtype=torch.float64, device=c.dev)}, sizes={'gd', 'Wd'}, inout={'acc': (1,)})


@row('error')
def _(c):
    return Call(lambda o: hip.error(o['y0'], o['y1'], o['ks'], [0.1, -0.2], 1e-2, 1e-3), {'y0': c.P(), 'y1': c.P(), 'ks': c.Ps(2)},
                sizes={'y0'})


@row('scaled_sumsq')
def _(c):
    return Call(lambda o: hip.scaled_sumsq(o['a'], o['b'], o['y'], 1e-2, 1e-3), {'a': c.P(), 'b': c.P(), 'y': c.P()}, sizes={'a'})


BETAS = [None, 0.9, 1.1]


@row('adams_predict')
def _(c):
    return Call(lambda o: hip.adams_predict(o['y'], o['phis'], BETAS, [0.1, 0.05], 3), {'y': c.P(), 'phis': c.Ps(3)}, sizes={'y'})


@row('adams_correct')
def _(c):
    return Call(lambda o: hip.adams_correct(o['nf'], o['phis'], BETAS, 3, o['p_next'], o['y0'], 0.07, [0.1, None, 0.2, 0.3], 1e-2, 1e-3),
                {'nf': c.P(), 'phis': c.Ps(3), 'p_next': c.P(), 'y0': c.P()}, sizes={'y0'})


@row('adams_update')
def _(c):
    return Call(lambda o: hip.adams_update(o['nf2'], o['phis'], BETAS, 3, 4), {'nf2': c.P(), 'phis': c.Ps(3)}, sizes={'nf2'})


@row('combine_bwd')
def _(c):
    return Call(lambda o: hip.combine_bwd(o['g'], o['ks'], [0.1, -0.2], [True, True], accs=o['accs'], acc_y0=o['acc_y0']),
                {'g': c.P(), 'ks': c.Ps(2), 'accs': c.Ps(2), 'acc_y0': c.P()}, sizes={'g'})


@row('pull')
def _(c):
    return Call(lambda o: hip.pull(o['ps'], [0.1, -0.2], base=o['base'], mask=o['mask'], ua=o['ua'], ub=o['ub'], out=o.get('out')),
                {'ps': c.Ps(2), 'base': c.P(), 'mask': c.P(), 'ua': c.P(), 'ub': c.P()}, sizes={'ps.0'}, outs={'out': ((c.n, c.H), (0,))})


@row('dot_diff')
def _(c):
    return Call(lambda o: hip.dot_diff(o['g'], o['a'], o['b']), {'g': c.P(), 'a': c.P(), 'b': c.P()}, sizes={'g'})


@row('error_bwd')
def _(c):
    return Call(lambda o: hip.error_bwd(o['y0'], o['y1'], o['ks'], [0.1, -0.2], 1e-2, 1e-3, 0.5, True, True, [True, True], accs=o['accs'],
                                        acc_y0=o['acc_y0'], acc_y1=o['acc_y1']),
                {'y0': c.P(), 'y1': c.P(), 'ks': c.Ps(2), 'accs': c.Ps(2), 'acc_y0': c.P(), 'acc_y1': c.P()}, sizes={'y0'})


@row('rms_bwd')
def _(c):
    return Call(lambda o: hip.rms_bwd(o['a'], o['b'], o['y'], 1e-2, 1e-3, 0.5, True, True, True), {'a': c.P(), 'b': c.P(), 'y': c.P()},
                sizes={'a'})


@row('interp_bwd')
def _(c):
    return Call(lambda o: hip.interp_bwd(o['g'], o['y0'], o['y1'], o['ks'], 0.1, 0.4, True, True, [True] * 7, accs=o['accs'],
                                         acc_y0=o['acc_y0'], acc_y1=o['acc_y1']),
                {'g': c.P(), 'y0': c.P(), 'y1': c.P(), 'ks': c.Ps(7), 'accs': c.Ps(7), 'acc_y0': c.P(), 'acc_y1': c.P()}, sizes={'g'})


@row('interp_direct_multi')
def _(c):
    return Call(lambda o: hip.interp_direct_multi(o['y0'], o['y1'], o['ks'], CS7, 0.1, [XP, XP[::-1]]),
                {'y0': c.P(), 'y1': c.P(), 'ks': c.Ps(7)}, sizes={'y0'})


@row('interp_bwd_multi')
def _(c):
    return Call(lambda o: hip.interp_bwd_multi(o['gs'], o['y0'], o['y1'], o['ks'], 0.1, [0.3, 0.6], True, True, [True] * 7,
                                               accs=o['accs'], acc_y0=o['acc_y0'], acc_y1=o['acc_y1']),
                {'gs': c.Ps(2), 'y0': c.P(), 'y1': c.P(), 'ks': c.Ps(7), 'accs': c.Ps(7), 'acc_y0': c.P(), 'acc_y1': c.P()}, sizes={'y0'})


@row('interp_fit')
def _(c):
    return Call(lambda o: hip.interp_fit(o['y0'], o['y1'], o['ks'], CS7, 0.1), {'y0': c.P(), 'y1': c.P(), 'ks': c.Ps(7)}, sizes={'y0'})


@row('interp_direct')
def _(c):
    return Call(lambda o: hip.interp_direct(o['y0'], o['y1'], o['ks'], CS7, 0.1, XP, out=o.get('out')),
                {'y0': c.P(), 'y1': c.P(), 'ks': c.Ps(7)}, sizes={'y0'}, outs={'out': ((c.n, c.H), ())})


@row('interp_eval')
def _(c):
    return Call(lambda o: hip.interp_eval(o['fit'], o['e'], XP, out=o.get('out')), {'fit': c.Ps(4), 'e': c.P()}, sizes={'e'},
                outs={'out': ((c.n, c.H), ())})


@row('fixed_stage')
def _(c):
    return Call(lambda o: hip.fixed_stage(5, o['y'], o['k1'], o['k2'], o['k3'], o['k4'], dt=0.1, out=o.get('out')),
                {'y': c.P(), 'k1': c.P(), 'k2': c.P(), 'k3': c.P(), 'k4': c.P()}, sizes={'y'}, outs={'out': ((c.n, c.H), ())})


@row('ab_step')
def _(c):
    return Call(lambda o: hip.ab_step(o['y'], o['fs'], [0.5, -0.3, 0.1], 0.1, out=o.get('out')), {'y': c.P(), 'fs': c.Ps(3)}, sizes={'y'},
                outs={'out': ((c.n, c.H), ())})


@row('ab_step_readout', widths=(20,))
def _(c):
    return Call(lambda o: hip.ab_step_readout(o['y'], o['fs'], [0.5, -0.3, 0.1], 0.1, o['weight'], o['bias'], out=o.get('out')),
                {'y': c.P(), 'fs': c.Ps(3), 'weight': c.t(3, c.H), 'bias': c.t(3)}, sizes={'y', 'weight'}, outs={'out': ((c.n, c.H), (0,))})


@row('abm_predict')
def _(c):
    return Call(lambda o: hip.abm_predict(o['y'], o['fs'], [0.5, -0.3, 0.1], [0.4, 0.2, -0.1], 0.1), {'y': c.P(), 'fs': c.Ps(3)},
                sizes={'y'})


@row('abm_correct')
def _(c):
    return Call(lambda o: hip.abm_correct(o['f'], o['delta'], o['y'], o['dy'], 0.3, 1e-2, 1e-3),
                {'f': c.P(), 'delta': c.P(), 'y': c.P(), 'dy': c.P()}, sizes={'y'}, inout={'dy': (0,)})


@row('ab_adjoint')
def _(c):
    return Call(lambda o: hip.ab_adjoint(o['gs'], [0.5, -0.3], base=o['base'], out=o.get('out')), {'gs': c.Ps(2), 'base': c.P()},
                sizes={'gs.0'}, outs={'out': ((c.n, c.H), ())})


@row('abm_adjoint')
def _(c):
    return Call(lambda o: hip.abm_adjoint(o['ps'], [0.5, -0.3], o['ds'], [0.2, 0.1], base=o['base'], out=o.get('out')),
                {'ps': c.Ps(2), 'ds': c.Ps(2), 'base': c.P()}, sizes={'ps.0'}, outs={'out': ((c.n, c.H), ())})


@row('tick_emit')
def _(c):
    return Call(lambda o: hip.tick_emit(o['y'], 0.1, [0.03, 0.07], outs=o['outs']), {'y': c.P(), 'outs': c.Ps(2)}, sizes={'y'},
                inout={'outs.0': (0,), 'outs.1': (1,)})


@row('row_l1_normalize')
def _(c):
    return Call(lambda o: hip.row_l1_normalize(o['X'], out=o.get('out')), {'X': c.P()}, sizes={'X'}, outs={'out': ((c.n, c.H), ())})


@row('row_l1_normalize_bwd')
def _(c):
    return Call(lambda o: hip.row_l1_normalize_bwd(o['g'], o['X']), {'g': c.P(), 'X': c.P()}, sizes={'X'})


@row('gene_rhs', widths=(8,))
def _(c):
    return Call(lambda o: hip.gene_rhs(c.A, o['x']), {'x': c.t(c.n, 1).abs()}, sizes={'x'})


@row('mutual_rhs', widths=(8,))
def _(c):
    return Call(lambda o: hip.mutual_rhs(c.A, o['x']), {'x': c.t(c.n, 1).abs()}, sizes={'x'})


@row('dyn_rk', widths=(8,))
def _(c):
    return Call(lambda o: hip.dyn_rk('heat', (0.7,), c.A, o['x'], 'error', o['y0'], o['kprev'], [0.1, -0.2, 0.3], 1e-2, 1e-3, y1=o['y1']),
                {'x': c.t(c.n, 1), 'y0': c.t(c.n, 1), 'kprev': [c.t(c.n, 1), c.t(c.n, 1)], 'y1': c.t(c.n, 1)}, sizes={'x'})


@row('dyn_rk:combine', widths=(8,))
def _(c):
    cd = torch.tensor([0.1, -0.2, 0.3], device=c.dev)
    return Call(lambda o: hip.dyn_rk('gene', (1.0, 1.0, 2.0), c.A, o['x'], 'combine', o['y0'], o['kprev'], c_dev=o['c_dev']),
                {'x': c.t(c.n, 1).abs(), 'y0': c.t(c.n, 1), 'kprev': [c.t(c.n, 1), c.t(c.n, 1)], 'c_dev': cd}, sizes={'x', 'c_dev'})


T, HG, HR = 3, 4, 5


def tgcn_proj_ops(c, M=3 * HR):
    return {'S': c.t(c.n, T), 'r': c.t(c.n), 'w': c.t(HG), 'b': c.t(HG), 'W_ih': c.t(M, c.n * HG)}


@row('tgcn_proj', widths=(8,))
def _(c):
    return Call(lambda o: hip.tgcn_proj(o['S'], o['r'], o['w'], o['b'], o['W_ih'], o['b_ih']), {**tgcn_proj_ops(c), 'b_ih': c.t(3 * HR)},
                sizes={'S', 'w', 'W_ih'})


@row('tgcn_proj_bwd', widths=(8,))
def _(c):
    return Call(lambda o: hip.tgcn_proj_bwd(o['S'], o['r'], o['w'], o['b'], o['W_ih'], o['GGI']), {**tgcn_proj_ops(c), 'GGI': c.t(T, 3 * HR)},
                sizes={'S', 'w', 'W_ih'})


@row('tgcn_cell', widths=(8,))
def _(c):
    return Call(lambda o: hip.tgcn_cell('lstm', o['GI'], o['W_hh'], o['b_hh'], h0=o['h0'], c0=o['c0']),
                {'GI': c.t(T, 4 * HR), 'W_hh': c.t(4 * HR, HR), 'b_hh': c.t(4 * HR), 'h0': c.t(HR), 'c0': c.t(HR)}, sizes={'GI'})


@row('tgcn_cell_bwd', widths=(8,))
def _(c):
    return Call(lambda o: hip.tgcn_cell_bwd('lstm', o['gH'], o['gates'], o['c_rec'], o['H'], o['W_hh'], h0=o['h0'], c0=o['c0']),
                {'gH': c.t(T, HR), 'gates': c.t(T, 4 * HR), 'c_rec': c.t(T, HR), 'H': c.t(T, HR), 'W_hh': c.t(4 * HR, HR), 'h0': c.t(HR),
                 'c0': c.t(HR)}, sizes={'H'})


CASES = [(name, H) for name, (_, widths) in ROWS.items() for H in widths]


def build(name, H, dev):
    return ROWS[name][0](Ctx(dev, H))


# ---------------------------------------------------------------------------------------------------------------- the three properties
@pytest.mark.parametrize('name,H', CASES)
def test_refusals(dev, name, H):
    call = build(name, H, dev)
    call.fn(dict(call.ops))                              # the valid operands are valid
    scramble(dev)
    tried = 0
    for op in list(names(call.ops)) + list(call.outs):
        is_out = op in call.outs or op in call.inout
        valid = torch.empty(call.outs[op][0], device=dev) if op in call.outs else get(call.ops, op)
        kinds = ['dtype'] + ([] if op in call.sizes else ['rows', 'cols']) + (['strided'] if is_out else [])
        for kind in kinds:
            bad = _bad(valid, kind)
            if bad is None:
                continue
            before = paths()
            torch.cuda.synchronize()
            fresh = build(name, H, dev)
            try:
                fresh.fn(put(fresh.ops, op, bad))
            except _lib.NdcnHipError as e:
                assert e.code == _lib.EINVAL, (op, kind, str(e))
            else:
                raise AssertionError('%s accepted a bad operand %s (%s)' % (name, op, kind))
            assert paths() == before, '%s: a %s operand %s was refused after a launch' % (name, kind, op)
            tried += 1
    assert tried >= len(list(names(call.ops)))


@pytest.mark.parametrize('name,H', CASES)
def test_equivalents(dev, name, H):
    call = build(name, H, dev)
    want = call.fn(dict(call.ops))
    for op in names(call.ops):
        valid = get(call.ops, op)
        if op in call.inout or valid.numel() < 2:
            continue
        fresh = build(name, H, dev)
        view = strided(get(fresh.ops, op))
        assert not view.is_contiguous() and torch.equal(view, valid)
        same(fresh.fn(put(fresh.ops, op, view)), want)
        if valid.dim() == 2 and valid.shape[0] == valid.shape[1]:          # a transposed view of a square operand
            fresh = build(name, H, dev)
            tv = get(fresh.ops, op).t().contiguous().t()
            assert not tv.is_contiguous()
            same(fresh.fn(put(fresh.ops, op, tv)), want)


@pytest.mark.parametrize('name,H', CASES)
def test_outputs(dev, name, H):
    call = build(name, H, dev)
    want = call.fn(dict(call.ops))
    targets = [(op, spec[0], spec[1]) for op, spec in call.outs.items()]
    targets += [(op, get(call.ops, op).shape, where) for op, where in call.inout.items() if where is not None]
    for op, shape, where in targets:
        fresh = build(name, H, dev)
        dtype = get(fresh.ops, op).dtype if op in call.inout else torch.float32
        count = int(np.prod(shape))
        buf = torch.full((count + 2 * GUARD,), float('nan'), dtype=dtype, device=dev)
        out = buf[GUARD:GUARD + count].view(shape)
        if op in call.inout:
            out.copy_(get(fresh.ops, op))
        got = fresh.fn(put(fresh.ops, op, out))
        torch.cuda.synchronize()
        assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + count:]).all()), '%s wrote past its output %s' % (name, op)
        if where is not None:
            assert pick(got, where) is out, '%s did not return its output %s' % (name, op)
            assert torch.equal(out, pick(want, where)) and not bool(torch.isnan(out).any())
        else:
            assert not bool(torch.isnan(out).any())
        same(got, want)


# ---------------------------------------------------------------------------------------------------------------- float64 bounds
def within(got, ref, bound, what):
    err = np.abs(got.double().cpu().numpy() - ref)
    assert bool((err <= bound).all()), '%s: worst error / bound = %.3g' % (what, float((err / np.maximum(bound, 1e-300)).max()))


@pytest.mark.parametrize('H', [8, 20])
def test_equivalent_forms_stay_inside_the_float64_bounds(dev, H):
    """spmm (1-D panel and strided view), linear (leading dimensions and strided view), rhs and combine on non-contiguous inputs: bit for
    bit the contiguous call (above) AND inside the float64 bounds stated in tests/_fma_chain.py - spmm: the fma chain bit for bit and
    spmm_bound; linear: dot_bound; combine: sum_bound; rhs: the Linear's dot_bound on its own magnitudes plus what spmm_bound allows
    its input S to be off, carried through |W| (the ReLU moves no value by more than its argument moved), 1.01 for the second order."""
    c = Ctx(dev, H)
    m = c.ring
    X = c.P()
    Xv = strided(X)
    x64 = X.double().cpu().numpy()
    got = hip.spmm(c.A, Xv)
    assert np.array_equal(got.cpu().numpy(), chain(m.indptr, m.indices, m.data, X.cpu().numpy()))
    S64 = m.astype(np.float64) @ x64
    mag = abs(m).astype(np.float64) @ np.abs(x64)
    within(got, S64, spmm_bound(m.indptr, mag), 'spmm')
    x1 = strided(X[:, 0].contiguous())                                    # a 1-D panel, not contiguous
    got1 = hip.spmm(c.A, x1)
    assert got1.shape == (c.n,) and torch.equal(got1, hip.spmm(c.A, X[:, :1].contiguous()).view(-1))
    assert np.array_equal(got1.cpu().numpy(), chain(m.indptr, m.indices, m.data, X[:, 0].cpu().numpy()).reshape(-1))
    W, b = c.t(12, H), c.t(12)
    S3 = strided(c.t(2, 35, H))                                           # leading dimensions (2, 35) = 70 rows
    Y = hip.linear(S3, W.t().contiguous().t(), b)
    assert Y.shape == (2, 35, 12) and torch.equal(Y, hip.linear(S3.contiguous().view(70, H), W, b).view(2, 35, 12))
    s64, w64 = S3.double().cpu().numpy().reshape(70, H), W.double().cpu().numpy()
    within(Y.view(70, 12), s64 @ w64.T + b.double().cpu().numpy(), dot_bound(H, np.abs(s64) @ np.abs(w64).T + np.abs(b.double().cpu().numpy())),
           'linear')
    Wh, bh = c.t(H, H), c.t(H)
    K = hip.rhs(c.A, Xv, Wh.t().contiguous().t(), bh)
    wh64 = Wh.double().cpu().numpy()
    ref = np.maximum(S64 @ wh64.T + bh.double().cpu().numpy(), 0)
    kmag = mag @ np.abs(wh64).T + np.abs(bh.double().cpu().numpy())
    within(K, ref, 1.01 * (dot_bound(H, kmag) + spmm_bound(m.indptr, mag) @ np.abs(wh64).T), 'rhs')
    ks, cs = [strided(k) for k in c.Ps(3)], [0.1, -0.2, 0.3]
    y0 = strided(c.P())
    out = hip.combine(y0, ks, cs)
    terms = [np.float64(np.float32(cc)) * k.double().cpu().numpy() for cc, k in zip(cs, ks)]
    cref = y0.double().cpu().numpy() + sum(terms)
    within(out, cref, sum_bound(len(ks), np.abs(y0.double().cpu().numpy()) + sum(np.abs(t) for t in terms)), 'combine')


# ---------------------------------------------------------------------------------------------------------------- rhs_rk(record=)
def test_rhs_rk_refuses_an_error_record_that_is_not_one(dev):
    """the caller's ErrorRecord receives 16 bytes: a record whose device buffer has another dtype or count is refused before the launch
    (the bad ones hold 16 bytes or more: the module's memory-safety rule), a proper one receives what the per-device record would"""
    c = Ctx(dev, 8)
    ops = {'X': c.P(), **lin_ops(c), 'y0': c.P(), 'kprev': c.Ps(2)}
    call = lambda rec: hip.rhs_rk(c.A, ops['X'], ops['W'], ops['b'], 'error', ops['y0'], ops['kprev'], [0.1, 0.2, 0.3], 1e-2, 1e-3, record=rec)
    K, want = call(None)
    rec = hip.new_error_record(dev)
    K2, got = call(rec)
    assert torch.equal(K, K2) and got == want and tuple(rec.out.tolist()) == want
    scramble(dev)
    for bad in (torch.zeros(3, dtype=torch.float64, device=dev), torch.zeros(4, dtype=torch.float32, device=dev)):
        assert bad.untyped_storage().nbytes() >= 16
        rec = hip.new_error_record(dev)
        rec.out = bad
        before = paths()
        with pytest.raises(_lib.NdcnHipError, match='record'):
            call(rec)
        assert paths() == before


# ---------------------------------------------------------------------------------------------------------------- completeness
def test_the_table_covers_every_method_with_tensor_operands():
    public = {n for n, v in vars(HipOps).items() if isinstance(v, staticmethod) and not n.startswith('_')}
    tabled = {name.split(':')[0] for name in ROWS}
    assert tabled <= public and NO_TENSORS <= public
    assert not (tabled & NO_TENSORS)
    missing = public - tabled - NO_TENSORS
    assert not missing, 'HipOps methods neither in the table nor listed as taking no tensors: %s' % sorted(missing)
