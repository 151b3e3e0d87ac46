#!/usr/bin/env python3
"""Generate the golden parity fixtures under tests/golden/ by RUNNING the reference.

Dev-only tool.  It contains no reference code: it puts /root/reference on sys.path,
imports the reference's own modules (neural_dynamics, torchdiffeq, utils_in_learn_dynamics,
propagation) and the module-level set-up of its three dynamics scripts, feeds them seeded
inputs, and stores (inputs, expected outputs) as small .npz files.  Only those data files
travel to the GPU box; the reference's Python never does.  When /root/reference is absent
(GPU box) it exits cleanly without touching anything.

Fixture families:
  G1 rhs_*.npz        ODEFunc.forward                       neural_dynamics.py:20-39
  G2 fixed_*.npz      odeint euler / midpoint / rk4         torchdiffeq/_impl/{solvers,fixed_grid,rk_common}.py
  G3 dopri5_*.npz     odeint dopri5 + per-attempt step log  torchdiffeq/_impl/{dopri5,interp,misc}.py
  G4 ndcn_*.npz       NDCN end to end (state_dict + output) neural_dynamics.py:122-160
  G5 truth_*.npz      heat / gene / mutualistic truth       {heat,gene,mutualistic}_dynamics.py:186-232
  G6 operators_*.npz  dense operator builders, zipf alpha   utils_in_learn_dynamics.py:80-157, propagation.py:91-103
  G7 dgnn_*.npz       ODEBlock2(no_control, terminal)       dgnn.py:173-182 on the Planetoid topologies
  G10 resgcn_*.npz    RowNorm / ResBlock / GCN / resGCN     ode_gcn.py:9-60, models.py:8-47, dgnn.py:129-140
  G11 layout_*.npz    generate_node_mapping degree/community utils_in_learn_dynamics.py:212-230 (+ the P A P^T of :233-247)
  G12 gconv_dense.npz GraphConvolution (dense A, flattened)  neural_dynamics.py:163-176
  G13 adams_*.npz     odeint adams + per-attempt step log    torchdiffeq/_impl/adams.py:62-170
  G14 substep_*.npz   fixed grid, options={'step_size': h}   torchdiffeq/_impl/solvers.py:55-68,79-108
  G15 bashforth_*.npz odeint explicit_adams + nfe            torchdiffeq/_impl/fixed_adams.py:151-211
  G16 moulton_*.npz   odeint fixed_adams + iterations, flags  torchdiffeq/_impl/fixed_adams.py:151-205
  G17 tgcn_*.npz      TemporalGCN lstm / gru / rnn + gradients neural_dynamics.py:179-238
"""
import os
import sys
import io
import pickle
import runpy
import contextlib

REF = '/root/reference'
if not os.path.isdir(REF):
    print('gen_golden: %s not present - nothing to do' % REF)
    sys.exit(0)

import numpy as np
import scipy.sparse as sp
import torch

sys.path.insert(0, REF)
os.environ.setdefault('MPLBACKEND', 'Agg')
import neural_dynamics as ref_nd            # noqa: E402  (the reference)
import torchdiffeq as ref_ode               # noqa: E402  (the reference's vendored copy)
import torchdiffeq._impl.dopri5 as ref_dopri5   # noqa: E402
import utils_in_learn_dynamics as ref_u     # noqa: E402
import propagation as ref_prop              # noqa: E402

assert ref_ode.__file__.startswith(REF), ref_ode.__file__

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests', 'golden')
os.makedirs(OUT, exist_ok=True)
torch.set_num_threads(1)      # deterministic summation order inside ATen


def save(name, **arrays):
    conv = {}
    for k, v in arrays.items():
        if isinstance(v, torch.Tensor):
            v = v.detach().cpu().numpy()
        conv[k] = np.asarray(v)
    path = os.path.join(OUT, name + '.npz')
    np.savez_compressed(path, **conv)
    print('wrote %-34s %8.1f KB' % (name + '.npz', os.path.getsize(path) / 1024))


def csr_of(dense):
    m = sp.csr_matrix(np.asarray(dense, dtype=np.float32))
    m.sort_indices()
    return dict(indptr=m.indptr.astype(np.int32), indices=m.indices.astype(np.int32),
                data=m.data.astype(np.float32), shape=np.array(m.shape, dtype=np.int64))


def grid_operator(S, kind='norm_lap'):
    A = ref_u.grid_8_neighbor_graph(S)
    if kind == 'norm_lap':
        OM = torch.FloatTensor(ref_u.normalized_laplacian(A.numpy()))
    elif kind == 'norm_adj':
        OM = torch.FloatTensor(ref_u.normalized_adj(A.numpy()))
    elif kind == 'kipf':
        OM = torch.FloatTensor(ref_u.zipf_smoothing(A.numpy()))
    elif kind == 'lap':
        OM = torch.diag(A.sum(1)) - A
    return A, OM


def x0_blocks(S):
    # the reference's initial image, heat_dynamics.py:178-182
    x0 = torch.zeros(S, S)
    x0[int(0.05 * S):int(0.25 * S), int(0.05 * S):int(0.25 * S)] = 25
    x0[int(0.45 * S):int(0.75 * S), int(0.45 * S):int(0.75 * S)] = 20
    x0[int(0.05 * S):int(0.25 * S), int(0.35 * S):int(0.65 * S)] = 17
    return x0.view(-1, 1).float()


# ----------------------------------------------------------------------------- G1
def gen_rhs():
    _, OM = grid_operator(20)
    OMs = ref_u.torch_sensor_to_torch_sparse_tensor(OM)
    for H in (1, 20, 256):
        for flag in ('default', 'no_control', 'no_graph'):
            for layout in ('dense', 'coo'):
                if H == 256 and layout == 'dense':
                    continue            # keep the fixture set small
                torch.manual_seed(100 + H)
                f = ref_nd.ODEFunc(H, OM if layout == 'dense' else OMs, dropout=0.0,
                                   no_graph=(flag == 'no_graph'), no_control=(flag == 'no_control'))
                x = torch.randn(400, H)
                with torch.no_grad():
                    out = f(torch.tensor(0.0), x)
                save('rhs_grid400_H%d_%s_%s' % (H, flag, layout), x=x, W=f.wt.weight, b=f.wt.bias,
                     out=out, **csr_of(OM))


# ----------------------------------------------------------------------------- G2
def make_func(H, OM, seed, **kw):
    torch.manual_seed(seed)
    f = ref_nd.ODEFunc(H, OM, dropout=0.0, **kw)
    x = torch.rand(OM.shape[0], H)
    return f, x


def gen_fixed():
    _, OM = grid_operator(20)
    OMs = ref_u.torch_sensor_to_torch_sparse_tensor(OM)
    t_eq = torch.linspace(0., 5., 21)
    rng = np.random.RandomState(7)
    t_ir = torch.linspace(0., 5., 200)[np.sort(rng.permutation(200)[:14])].clone()
    t_ir[0] = 0
    for method in ('euler', 'midpoint', 'rk4'):
        for tname, t in (('equal', t_eq), ('irregular', t_ir)):
            f, x = make_func(20, OMs, 11)
            with torch.no_grad():
                y = ref_ode.odeint(f, x, t, method=method)
            save('fixed_%s_%s' % (method, tname), x0=x, t=t, W=f.wt.weight, b=f.wt.bias, traj=y, **csr_of(OM))
    # decreasing time vector (misc.py:184-187) on rk4
    f, x = make_func(20, OMs, 11)
    t = torch.linspace(1., 0., 6)
    with torch.no_grad():
        y = ref_ode.odeint(f, x, t, method='rk4')
    save('fixed_rk4_decreasing', x0=x, t=t, W=f.wt.weight, b=f.wt.bias, traj=y, **csr_of(OM))


# ----------------------------------------------------------------------------- G3
class StepLog:
    """Records every attempted dopri5 step by wrapping (not editing) the reference's methods."""

    def __init__(self):
        self.rows = []
        self.nfe = 0
        self._ratio = None

    @contextlib.contextmanager
    def attach(self):
        orig_step = ref_dopri5.Dopri5Solver._adaptive_dopri5_step
        orig_ratio = ref_dopri5._compute_error_ratio
        log = self

        def ratio_wrap(*a, **k):
            r = orig_ratio(*a, **k)
            log._ratio = float(r[0])
            return r

        def step_wrap(solver, rk_state):
            t0, dt = float(rk_state.t1), float(rk_state.dt)
            new = orig_step(solver, rk_state)
            accepted = float(new.t1) != t0
            log.rows.append((t0, dt, 1.0 if accepted else 0.0, log._ratio, float(new.dt)))
            return new

        ref_dopri5.Dopri5Solver._adaptive_dopri5_step = step_wrap
        ref_dopri5._compute_error_ratio = ratio_wrap
        try:
            yield self
        finally:
            ref_dopri5.Dopri5Solver._adaptive_dopri5_step = orig_step
            ref_dopri5._compute_error_ratio = orig_ratio


class CountingFunc(torch.nn.Module):
    def __init__(self, f):
        super().__init__()
        self.f = f
        self.nfe = 0

    def forward(self, t, x):
        self.nfe += 1
        return self.f(t, x)


def gen_dopri5():
    _, OM = grid_operator(20)
    OMs = ref_u.torch_sensor_to_torch_sparse_tensor(OM)
    cases = [('loose', .01, .001, torch.linspace(0., 5., 21)),
             ('dgnn', .1, .1, torch.linspace(0., 1.2, 16)),
             ('tight', 1e-7, 1e-9, torch.linspace(0., 2., 6)),
             ('twotick', .01, .001, torch.tensor([0., 5.]))]
    for name, rtol, atol, t in cases:
        f, x = make_func(20, OMs, 23)
        cf = CountingFunc(f)
        log = StepLog()
        with torch.no_grad(), log.attach():
            y = ref_ode.odeint(cf, x, t, rtol=rtol, atol=atol, method='dopri5')
        save('dopri5_%s' % name, x0=x, t=t, W=f.wt.weight, b=f.wt.bias, traj=y, rtol=rtol, atol=atol,
             steplog=np.array(log.rows, dtype=np.float64), nfe=cf.nfe, **csr_of(OM))
    # non-default controller options (dopri5.py:60,72-74): small ifactor / large dfactor / tighter safety, tolerances
    # that produce rejected steps
    f, x = make_func(20, OMs, 37)
    cf = CountingFunc(f)
    log = StepLog()
    t = torch.linspace(0., 4., 9)
    opts = dict(safety=0.99, ifactor=20.0, dfactor=0.5)
    with torch.no_grad(), log.attach():
        y = ref_ode.odeint(cf, x, t, rtol=1e-3, atol=1e-4, method='dopri5', options=dict(opts))
    # the controller itself on (dt, ratio) pairs that hit every branch (misc.py:160-170), with the solver's own
    # conversion of the option values (dopri5.py:72-74)
    import torchdiffeq._impl.misc as ref_misc
    cv = lambda v: ref_misc._convert_to_tensor(v, dtype=torch.float64)
    ctl_in = [(0.25, 0.0), (0.25, 1e-9), (0.25, 0.3), (0.25, 0.999), (0.25, 1.0), (0.25, 1.7), (0.25, 40.0), (0.25, 1e9)]
    ctl_out = [float(ref_misc._optimal_step_size(torch.tensor(dt, dtype=torch.float64), [torch.tensor(r, dtype=torch.float32)],
                                                 safety=cv(opts['safety']), ifactor=cv(opts['ifactor']), dfactor=cv(opts['dfactor'])))
               for dt, r in ctl_in]
    save('dopri5_options', x0=x, t=t, W=f.wt.weight, b=f.wt.bias, traj=y, rtol=1e-3, atol=1e-4,
         steplog=np.array(log.rows, dtype=np.float64), nfe=cf.nfe, ctl_in=np.array(ctl_in), ctl_out=np.array(ctl_out),
         **{'opt_' + k: v for k, v in opts.items()}, **csr_of(OM))
    # no_control (pure SpMM+ReLU RHS) and a decreasing time vector
    f, x = make_func(20, OMs, 29, no_control=True)
    cf = CountingFunc(f)
    log = StepLog()
    t = torch.linspace(0., 3., 7)
    with torch.no_grad(), log.attach():
        y = ref_ode.odeint(cf, x, t, rtol=.01, atol=.001, method='dopri5')
    save('dopri5_no_control', x0=x, t=t, W=f.wt.weight, b=f.wt.bias, traj=y, rtol=.01, atol=.001,
         steplog=np.array(log.rows, dtype=np.float64), nfe=cf.nfe, **csr_of(OM))
    f, x = make_func(20, OMs, 31)
    cf = CountingFunc(f)
    log = StepLog()
    t = torch.linspace(2., 0., 5)
    with torch.no_grad(), log.attach():
        y = ref_ode.odeint(cf, x, t, rtol=.01, atol=.001, method='dopri5')
    save('dopri5_decreasing', x0=x, t=t, W=f.wt.weight, b=f.wt.bias, traj=y, rtol=.01, atol=.001,
         steplog=np.array(log.rows, dtype=np.float64), nfe=cf.nfe, **csr_of(OM))


# ----------------------------------------------------------------------------- G4
def gen_ndcn():
    _, OM = grid_operator(20)
    x0 = x0_blocks(20)
    t = torch.linspace(0., 5., 21)
    variants = {
        'ndcn': dict(hidden_size=20, no_embed=False, no_graph=False, no_control=False),
        'no_embed': dict(hidden_size=1, no_embed=True, no_graph=False, no_control=False),
        'no_control': dict(hidden_size=20, no_embed=False, no_graph=False, no_control=True),
        'no_graph': dict(hidden_size=20, no_embed=False, no_graph=True, no_control=False),
    }
    for name, kw in variants.items():
        for method in ('euler', 'dopri5'):
            torch.manual_seed(0)
            m = ref_nd.NDCN(input_size=1, A=OM, num_classes=1, dropout=0.0, rtol=.01, atol=.001, method=method, **kw)
            with torch.no_grad():
                y = m(t, x0)
            sd = {'sd__' + k.replace('.', '__'): v for k, v in m.state_dict().items()}
            save('ndcn_%s_%s' % (name, method), x0=x0, t=t, out=y, **sd, **csr_of(OM))


# ----------------------------------------------------------------------------- G5
def run_script_setup(script, argv):
    """Execute a reference driver's module-level set-up (graph, operator, truth solve, model build).
    Its training loop sits under `if __name__ == '__main__'` and is not entered."""
    old_argv, old_cwd = sys.argv, os.getcwd()
    sys.argv = [script] + argv
    os.chdir(REF)
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            g = runpy.run_path(os.path.join(REF, script), run_name='ref_setup')
    finally:
        sys.argv, _ = old_argv, os.chdir(old_cwd)
    return g


def gen_truth():
    for script, tag in (('heat_dynamics.py', 'heat'), ('gene_dynamics.py', 'gene'), ('mutualistic_dynamics.py', 'mutual')):
        for sparse in (False, True):
            argv = ['--network', 'grid', '--sampled_time', 'equal', '--baseline', 'ndcn', '--gpu', '-1',
                    '--time_tick', '21'] + (['--sparse'] if sparse else [])
            g = run_script_setup(script, argv)
            A = g['A'].to_dense() if g['A'].is_sparse else g['A']
            L = g['L'].to_dense() if g['L'].is_sparse else g['L']
            OM = g['OM'].to_dense() if g['OM'].is_sparse else g['OM']
            a, l, om = csr_of(A), csr_of(L), csr_of(OM)
            save('truth_%s_%s' % (tag, 'coo' if sparse else 'dense'), x0=g['x0'], t=g['t'], traj=g['solution_numerical'],
                 A_indptr=a['indptr'], A_indices=a['indices'], A_data=a['data'],
                 L_indptr=l['indptr'], L_indices=l['indices'], L_data=l['data'],
                 OM_indptr=om['indptr'], OM_indices=om['indices'], OM_data=om['data'], n=np.int64(A.shape[0]))


# ----------------------------------------------------------------------------- G6
def load_planetoid_adj(name):
    """Adjacency of a Planetoid pickle, symmetrised as utils.py:183-196 does (utils.load_data itself
    no longer runs under scipy 1.15)."""
    with open(os.path.join(REF, 'data', name, 'ind.%s.graph' % name), 'rb') as fh:
        graph = pickle.load(fh, encoding='latin1')
    rows, cols = [], []
    for r in graph:
        for c in graph.get(r):
            rows.append(r)
            cols.append(c)
    n = max(max(rows), max(cols)) + 1
    adj = sp.csr_matrix((np.ones(len(rows)), (rows, cols)), shape=(n, n))
    adj = adj + adj.T
    adj[adj > 1] = 1
    return adj.tocsr()


def gen_operators():
    A, _ = grid_operator(20)
    a = csr_of(A)
    arrs = dict(A_indptr=a['indptr'], A_indices=a['indices'], A_data=a['data'], n=np.int64(400))
    for kind in ('norm_lap', 'norm_adj', 'kipf', 'lap'):
        _, OM = grid_operator(20, kind)
        c = csr_of(OM)
        arrs.update({kind + '_indptr': c['indptr'], kind + '_indices': c['indices'], kind + '_data': c['data']})
    arrs['x0'] = x0_blocks(20)
    save('operators_grid400', **arrs)
    # non-square canvas: n=10 nodes asked, ceil(sqrt) = 4 (heat_dynamics.py:81)
    A5, _ = grid_operator(5)
    c = csr_of(A5)
    save('operators_grid25', A_indptr=c['indptr'], A_indices=c['indices'], A_data=c['data'], n=np.int64(25))
    for name in ('cora', 'pubmed'):
        adj = load_planetoid_adj(name)
        adj.sort_indices()
        arrs = dict(adj_indptr=adj.indptr.astype(np.int32), adj_indices=adj.indices.astype(np.int32),
                    n=np.int64(adj.shape[0]))
        for alpha in (0.0, 0.5):
            with contextlib.redirect_stdout(io.StringIO()):
                op = ref_prop.Propagation(adj).zipf_smoothing_alpha(alpha)
            op = sp.csr_matrix(op).astype(np.float32)
            op.sort_indices()
            tag = 'alpha%02d' % int(alpha * 10)
            arrs.update({tag + '_indptr': op.indptr.astype(np.int32), tag + '_indices': op.indices.astype(np.int32),
                         tag + '_data': op.data.astype(np.float32)})
        save('operators_%s' % name, **arrs)


# ----------------------------------------------------------------------------- G7
def gen_dgnn():
    sys.path.insert(0, REF)
    import utils as ref_utils
    for name, H in (('cora', 64), ('pubmed', 16)):
        adj = load_planetoid_adj(name)
        with contextlib.redirect_stdout(io.StringIO()):
            op = ref_prop.Propagation(adj).zipf_smoothing_alpha(0.0)
        A = ref_utils.sparse_csr_matrix_to_torch_sparse_tensor(sp.csr_matrix(op))
        torch.manual_seed(5)
        x = torch.tanh(torch.randn(adj.shape[0], H))          # what Linear+Tanh would hand the block
        t = torch.linspace(0, 1.2, 16)
        f = ref_nd.ODEFunc(H, A, dropout=0.0, no_control=True)
        cf = CountingFunc(f)
        blk = ref_nd.ODEBlock2(cf, t, rtol=.1, atol=.1, method='dopri5', terminal=True)
        log = StepLog()
        with torch.no_grad(), log.attach():
            y = blk(x)
        save('dgnn_%s_H%d' % (name, H), x=x, t=t, out=y, steplog=np.array(log.rows, dtype=np.float64), nfe=cf.nfe)


# ----------------------------------------------------------------------------- G8
def gen_dataset():
    """Cora as utils.load_data (utils.py:91-230) assembles it - that function itself no longer runs under scipy 1.15
    (SURVEY 8c), so its steps are replayed here on the reference's own data files: features = vstack(allx, tx) with
    the test rows re-ordered, row-normalised (propagation.py:30-37); labels likewise; the reference's index split."""
    name = 'cora'
    objs = []
    for part in ('x', 'y', 'tx', 'ty', 'allx', 'ally'):
        with open(os.path.join(REF, 'data', name, 'ind.%s.%s' % (name, part)), 'rb') as fh:
            objs.append(pickle.load(fh, encoding='latin1'))
    x, y, tx, ty, allx, ally = objs
    test_idx_reorder = np.loadtxt(os.path.join(REF, 'data', name, 'ind.%s.test.index' % name), dtype=np.int64)
    test_idx_range = np.sort(test_idx_reorder)
    features = sp.vstack((allx, tx)).tolil()
    features[test_idx_reorder, :] = features[test_idx_range, :]
    labels = np.vstack((ally, ty))
    labels[test_idx_reorder, :] = labels[test_idx_range, :]
    with contextlib.redirect_stdout(io.StringIO()):
        fn = sp.csr_matrix(ref_prop.Propagation(sp.csr_matrix(features)).row_normalization()).astype(np.float32)
    fn.sort_indices()
    save('dataset_cora', feat_indptr=fn.indptr.astype(np.int32), feat_indices=fn.indices.astype(np.int16),
         feat_data=fn.data.astype(np.float32), feat_shape=np.array(fn.shape, dtype=np.int64),
         labels=labels.argmax(1).astype(np.int16), idx_train=np.arange(len(y), dtype=np.int32),
         idx_val=np.arange(len(y), len(y) + 500, dtype=np.int32), idx_test=test_idx_range.astype(np.int32))


def gen_planetoid_raw():
    """Cora's raw Planetoid parts as plain arrays (x / tx / allx as CSR, y / ty / ally dense, graph as keys + neighbour lists in
    their order, the test index): tests/test_graphs.py writes them back as the ind.cora.* files planetoid.load_data reads."""
    name = 'cora'
    arrays = {}
    for part in ('x', 'y', 'tx', 'ty', 'allx', 'ally', 'graph'):
        with open(os.path.join(REF, 'data', name, 'ind.%s.%s' % (name, part)), 'rb') as fh:
            o = pickle.load(fh, encoding='latin1')
        if part == 'graph':
            keys = list(o.keys())
            arrays.update(graph_keys=np.array(keys, dtype=np.int32),
                          graph_counts=np.array([len(o[k]) for k in keys], dtype=np.int32),
                          graph_neighbours=np.array([c for k in keys for c in o[k]], dtype=np.int32))
        elif sp.issparse(o):
            assert o.format == 'csr'
            arrays.update({part + '_indptr': o.indptr.astype(np.int32), part + '_indices': o.indices.astype(np.int16),
                           part + '_data': o.data, part + '_shape': np.array(o.shape, dtype=np.int64)})
        else:
            assert np.array_equal(o.astype(np.int8), o)
            arrays[part] = o.astype(np.int8)
    arrays['test_index'] = np.loadtxt(os.path.join(REF, 'data', name, 'ind.%s.test.index' % name), dtype=np.int64).astype(np.int32)
    save('planetoid_cora_raw', **arrays)


# ----------------------------------------------------------------------------- G9
def gen_adjoint():
    """Gradients of the reference's odeint_adjoint (torchdiffeq/_impl/adjoint.py:105-133) on a small case."""
    _, OM = grid_operator(12)
    OMs = ref_u.torch_sensor_to_torch_sparse_tensor(OM)
    for method, rtol, atol in (('dopri5', 1e-5, 1e-7), ('rk4', 0.0, 0.0)):
        torch.manual_seed(41)
        f = ref_nd.ODEFunc(8, OMs, dropout=0.0)
        x0 = torch.rand(144, 8, requires_grad=True)
        t = torch.linspace(0., 1., 5 if method == 'dopri5' else 21)
        target = torch.rand(len(t), 144, 8)
        kw = dict(method=method) if method == 'rk4' else dict(method=method, rtol=rtol, atol=atol)
        y = ref_ode.odeint_adjoint(f, x0, t, **kw)
        loss = torch.nn.functional.l1_loss(y, target)
        loss.backward()
        save('adjoint_%s' % method, x0=x0.detach(), t=t, target=target, W=f.wt.weight.detach(), b=f.wt.bias.detach(),
             traj=y.detach(), loss=loss.detach(), g_x0=x0.grad, g_W=f.wt.weight.grad, g_b=f.wt.bias.grad,
             rtol=rtol, atol=atol, **csr_of(OM))


# ----------------------------------------------------------------------------- G10
def gen_resgcn():
    import utils as ref_utils
    import ode_gcn as ref_og
    import models as ref_models
    adj = load_planetoid_adj('cora')
    with contextlib.redirect_stdout(io.StringIO()):
        op = sp.csr_matrix(ref_prop.Propagation(adj).zipf_smoothing_alpha(0.0))
    A = ref_utils.sparse_csr_matrix_to_torch_sparse_tensor(op)
    op.sort_indices()
    csr = dict(indptr=op.indptr.astype(np.int32), indices=op.indices.astype(np.int32), data=op.data.astype(np.float32),
               shape=np.array(op.shape, dtype=np.int64))
    n, H = adj.shape[0], 32
    torch.manual_seed(11)
    x = torch.randn(n, H)
    x[17] = 0                                                  # an all-zero row: 0 / max(0, eps)
    with torch.no_grad():
        save('resgcn_rownorm', x=x, out=ref_og.RowNorm()(x.clone()))
        for tag, kw in (('plain', {}), ('norm', dict(normalize=True)), ('tv', dict(time_varying=True)),
                        ('euler', dict(Euler=True)), ('norm_tv', dict(normalize=True, time_varying=True))):
            torch.manual_seed(3)
            blk = ref_og.ResBlock(H, A, **kw).eval()
            extra = {}
            if kw.get('time_varying'):
                extra.update(W=blk.linear.weight, b=blk.linear.bias)
            if kw.get('Euler'):
                extra.update(time_step=blk.time_step)
            save('resgcn_block_%s' % tag, out=blk(x.clone()), **extra, **csr)     # input: x of resgcn_rownorm.npz
        feat = torch.rand(n, 32)
        torch.manual_seed(4)
        gcn = ref_models.GCN(32, 16, 7, dropout=0.5, num_middle_layers=1).eval()
        save('resgcn_gcn', x=feat, out=gcn(feat, A), **{'sd_' + k: v for k, v in gcn.state_dict().items()}, **csr)
        for tag, norm, euler in (('model', False, False), ('model_norm_euler', True, True)):
            torch.manual_seed(5)
            layers = [torch.nn.Linear(32, H), torch.nn.ReLU(inplace=True)]
            layers += [ref_og.ResBlock(H, A, dropout=0.5, normalize=norm, Euler=euler) for _ in range(2)]
            layers += [torch.nn.Linear(H, 7)]
            model = torch.nn.Sequential(*layers).eval()
            save('resgcn_%s' % tag, x=feat, out=model(feat), **{'sd_' + k: v for k, v in model.state_dict().items()}, **csr)


def gen_layout():
    """G11: the reference's node mapping on its own graph generators (heat_dynamics.py:87-109 at n = 400).
    networkx_reorder_nodes itself calls nx.to_scipy_sparse_matrix, removed in networkx 3: the mapping
    function is what still runs; the re-labelled adjacency new_A[map[i], map[j]] = A[i, j] is formed here with the
    two calls' modern equivalents."""
    import networkx as nx
    n, seed = 400, 0
    n1, n2, n3 = int(n / 3), int(n / 3), int(n / 4)
    graphs = {
        'random': nx.erdos_renyi_graph(n, 0.1, seed=seed),
        'power_law': nx.barabasi_albert_graph(n, 5, seed=seed),
        'small_world': nx.newman_watts_strogatz_graph(400, 5, 0.5, seed=seed),
        'community': nx.random_partition_graph([n1, n2, n3, n - n1 - n2 - n3], .25, .01, seed=seed),
    }
    for name, G0 in graphs.items():
        # canonical node order (labels ascending): nx.random_partition_graph inserts its nodes out of label order, and
        # the reference's mapping breaks degree ties by insertion order - an adjacency matrix carries no such order
        G = nx.Graph()
        G.add_nodes_from(sorted(G0.nodes))
        G.add_edges_from(sorted((min(u, v), max(u, v)) for u, v in G0.edges))
        A = sp.csr_matrix(nx.to_scipy_sparse_array(G, nodelist=range(n), format='csr'))
        A.sort_indices()
        out = dict(indptr=A.indptr.astype(np.int32), indices=A.indices.astype(np.int32))
        for layout in ('degree', 'community'):
            m = ref_u.generate_node_mapping(G, layout)
            new = np.array([m[i] for i in range(n)], dtype=np.int32)
            C = A.tocoo()
            newA = sp.coo_matrix((C.data, (new[C.row], new[C.col])), shape=C.shape).tocsr()
            newA.sort_indices()
            out['map_' + layout] = new
            out['new_indptr_' + layout] = newA.indptr.astype(np.int32)
            out['new_indices_' + layout] = newA.indices.astype(np.int32)
        save('layout_%s' % name, **out)


def gen_gconv():
    """G12: the dense-A GraphConvolution that dgnn.py's star import exposes (neural_dynamics.py:163-176)."""
    _, A = grid_operator(12, 'norm_lap')
    torch.manual_seed(21)
    gc = ref_nd.GraphConvolution(7, 5, bias=True)
    gc_nb = ref_nd.GraphConvolution(7, 5, bias=False)
    x = torch.randn(A.shape[0], 7)
    with torch.no_grad():
        save('gconv_dense', A=A, x=x, W=gc.fc.weight, b=gc.fc.bias, out=gc(x, A), W_nb=gc_nb.fc.weight, out_nb=gc_nb(x, A))


def gen_adams():
    """G13: the variable-coefficient Adams-Bashforth-Moulton solver (adams.py) on the NDCN ODEFunc, with one row per
    attempted step {t_n, attempted next_t, order, accepted, next next_t} recorded by wrapping (not editing) the
    reference's step method: loose / tight tolerances (orders 1-5, rejected steps), a dense tick grid (next_t clipped
    to every tick), max_order 2, the no_control right-hand side."""
    import torchdiffeq._impl.adams as ref_adams
    _, OM = grid_operator(20)
    OMs = ref_u.torch_sensor_to_torch_sparse_tensor(OM)
    cases = [('loose', .01, .001, torch.linspace(0., 5., 6), {}, {}),
             ('tight', 1e-5, 1e-7, torch.linspace(0., 2., 5), {}, {}),
             ('ticks', 1e-3, 1e-4, torch.linspace(0., 5., 30), {}, {}),
             ('order2', 1e-4, 1e-6, torch.linspace(0., 1., 4), {'max_order': 2, 'safety': 0.8}, {}),
             ('no_control', .01, .001, torch.linspace(0., 3., 7), {}, {'no_control': True})]
    orig = ref_adams.VariableCoefficientAdamsBashforth._adaptive_adams_step
    for name, rtol, atol, t, opts, fkw in cases:
        f, x = make_func(20, OMs, 41, **fkw)
        cf = CountingFunc(f)
        rows = []

        def wrapped(self, st, final_t):
            t_n, nt, order = float(st.prev_t[0]), min(float(st.next_t), float(final_t)), int(st.order)
            out = orig(self, st, final_t)
            rows.append((t_n, nt, order, 1.0 if float(out.prev_t[0]) != t_n else 0.0, float(out.next_t)))
            return out
        ref_adams.VariableCoefficientAdamsBashforth._adaptive_adams_step = wrapped
        try:
            with torch.no_grad():
                y = ref_ode.odeint(cf, x, t, rtol=rtol, atol=atol, method='adams', options=dict(opts) if opts else None)
        finally:
            ref_adams.VariableCoefficientAdamsBashforth._adaptive_adams_step = orig
        save('adams_%s' % name, x0=x, t=t, W=f.wt.weight, b=f.wt.bias, traj=y, rtol=rtol, atol=atol,
             steplog=np.array(rows, dtype=np.float64), nfe=cf.nfe, no_control=int(bool(fkw)),
             **{'opt_' + k: v for k, v in opts.items()}, **csr_of(OM))


# ----------------------------------------------------------------------------- G14
def ref_step_grid(t, h):
    """(the reference's own grid for the float32 time vector t and step size h, did its assertion of solvers.py:83 hold)"""
    import torchdiffeq._impl.fixed_grid as ref_fg
    g = ref_fg.Euler(None, (torch.zeros(1),), step_size=h).grid_constructor(None, None, t)
    return g, bool(g[0] == t[0] and g[-1] == t[-1])


def gen_substep():
    """FixedGridODESolver with options={'step_size': h}: trajectories at the caller's ticks, the rows of the reference's own solve on
    the explicit grid they are equal to (the tick placement of solvers.py:92-97), and a table of grids.  (Names start with
    substep_, not fixed_: the fixed_*.npz globs of the existing tests must not pick these up without the option.)"""
    _, OM = grid_operator(20)
    OMs = ref_u.torch_sensor_to_torch_sparse_tensor(OM)
    cases = {
        'multiples': (torch.linspace(0., 2., 9), 0.125),                          # every tick is a grid point
        'irregular': (torch.tensor([0., .13, .5, .55, .57, 1.0]), 0.1),          # several ticks in one step, steps without a tick
        'clamped': (torch.tensor([0., .3, .65, 1.03]), 0.25),                    # the last step is cut short by the clamp
    }

    def one(name, method, t, h, fkw=None):
        f, x = make_func(20, OMs, 11, **(fkw or {}))
        tt = -t if bool((t[1:] < t[:-1]).all()) else t
        grid, ok = ref_step_grid(tt, h)
        assert ok
        with torch.no_grad():
            y = ref_ode.odeint(f, x, t, method=method, options={'step_size': h})
            fine = ref_ode.odeint(f, x, grid if tt is t else -grid, method=method)
        rows = []
        for j in range(len(t)):
            hit = [r for r in range(len(grid)) if torch.equal(fine[r], y[j])]
            assert hit, (name, j)
            rows.append(min(r for r in hit if not rows or r >= rows[-1]))
        save(name, x0=x, t=t, h=np.float64(h), W=f.wt.weight, b=f.wt.bias, traj=y, grid=grid, rows=np.array(rows, dtype=np.int64),
             no_control=int(bool(fkw)), **csr_of(OM))

    for method in ('euler', 'midpoint', 'rk4'):
        for cname, (t, h) in cases.items():
            one('substep_%s_%s' % (method, cname), method, t, h)
    one('substep_rk4_decreasing', 'rk4', torch.tensor([1., .6, .35, 0.]), 0.1)
    one('substep_euler_nocontrol', 'euler', cases['irregular'][0], 0.1, dict(no_control=True))

    # odeint_adjoint with the option: forward and every backward interval solve on their own step_size grids (adjoint.py)
    _, OM12 = grid_operator(12)
    OM12s = ref_u.torch_sensor_to_torch_sparse_tensor(OM12)
    torch.manual_seed(41)
    f = ref_nd.ODEFunc(8, OM12s, dropout=0.0)
    x0 = torch.rand(144, 8, requires_grad=True)
    t = torch.linspace(0., 1., 5)
    target = torch.rand(len(t), 144, 8)
    y = ref_ode.odeint_adjoint(f, x0, t, method='rk4', options={'step_size': 0.1})
    loss = torch.nn.functional.l1_loss(y, target)
    loss.backward()
    save('substep_adjoint_rk4', x0=x0.detach(), t=t, h=np.float64(0.1), target=target, W=f.wt.weight.detach(), b=f.wt.bias.detach(),
         traj=y.detach(), loss=loss.detach(), g_x0=x0.grad, g_W=f.wt.weight.grad, g_b=f.wt.bias.grad, **csr_of(OM12))

    # the grid table: (t0, t1, h) -> length, last three points, did the assertion of solvers.py:83 fire.  A scan of 200 000 random
    # float32 triples (t0 in [0, 2), +-2, +-100, +-1000 - the negated times of a decreasing t included; half of them with
    # t1 - t0 a whole multiple of h; h a float32 value or an arbitrary Python float) looks for one where it fires; the table keeps
    # every such triple and 400 of the others.
    rng = np.random.RandomState(2024)
    f32 = np.float32
    keep, fired = [], []
    n_scan = int(os.environ.get('NDCN_GEN_SUBSTEP_SCAN', '200000'))
    for i in range(n_scan):
        mode = i % 4
        scale = (2, 100, 2, 1000)[mode]
        t0 = f32(rng.uniform(0, 2)) if mode == 0 else f32(rng.uniform(-scale, scale))
        h = f32(10 ** rng.uniform(-2.5, 0))
        t1 = f32(t0 + f32(rng.randint(1, 60)) * h) if i % 2 else f32(t0 + f32(rng.uniform(0.01, 20)) * h)
        if not t1 > t0:
            continue
        hh = float(h) if i % 3 else float(10 ** rng.uniform(-2.5, 0))
        g, ok = ref_step_grid(torch.tensor([t0, t1]), hh)
        row = [float(t0), float(t1), hh, float(len(g)), float(not ok)] + [float(v) for v in ([np.nan] * 3 + g.tolist())[-3:]]
        if not ok:
            fired.append(row)
        elif i % (n_scan // 400) == 0:
            keep.append(row)
    print('substep grid scan: %d triples, the assertion fired for %d' % (n_scan, len(fired)))
    save('substep_grids', table=np.array(fired + keep, dtype=np.float64), n_scanned=n_scan, n_fired=len(fired))


# ----------------------------------------------------------------------------- G15
def gen_bashforth():
    """method='explicit_adams' (AdamsBashforth, fixed_adams.py:151-211) over the NDCN ODEFunc on the 6 x 6 lattice at H = 8, with the
    evaluation count.  (Names start with bashforth_: the fixed_*.npz and adams_*.npz globs of the existing tests must not pick these
    up.)  High-order Adams-Bashforth has a tiny stability region - an unstable trajectory amplifies last-bit differences and proves
    nothing - so every case asserts that the reference's own trajectory stays finite and within 10 x max |x0|."""
    _, OM = grid_operator(6)
    OMs = ref_u.torch_sensor_to_torch_sparse_tensor(OM)
    h = 1.0 / 128
    cases = {
        'default': (torch.linspace(0., 16 * 0.01, 17), {}, {}),                   # 16 steps: the order reaches 11, the history wraps
        'order4': (torch.linspace(0., 16 * 0.01, 17), {'max_order': 4}, {}),
        # 14 grid steps of 1 / 128: a tick inside a step, a coincident one, two inside one step, steps without a tick, the clamp-free end
        'stepsize': (torch.tensor([0., 1.5 * h, 4 * h, 4.3 * h, 4.6 * h, 9 * h, 14 * h]), {'step_size': h}, {}),
        'no_control': (torch.linspace(0., 16 * 0.01, 17), {}, {'no_control': True}),
        'warmup': (torch.tensor([0., 0.01, 0.02]), {}, {}),                       # two steps: RK4 only
    }
    for name, (t, opts, fkw) in cases.items():
        f, x = make_func(8, OMs, 53, **fkw)
        cf = CountingFunc(f)
        with torch.no_grad():
            y = ref_ode.odeint(cf, x, t, method='explicit_adams', options=dict(opts) if opts else None)
        n_steps = len(t) - 1
        if 'step_size' in opts:
            grid, ok = ref_step_grid(t, opts['step_size'])
            assert ok
            n_steps = len(grid) - 1
            assert n_steps >= 14
        assert bool(torch.isfinite(y).all()) and float(y.abs().max()) <= 10 * float(x.abs().max()), name
        assert cf.nfe == n_steps + 6, (name, cf.nfe, n_steps)
        save('bashforth_%s' % name, x0=x, t=t, W=f.wt.weight, b=f.wt.bias, traj=y, nfe=cf.nfe, n_steps=n_steps,
             no_control=int(bool(fkw)), **{'opt_' + k: v for k, v in opts.items()}, **csr_of(OM))


# ----------------------------------------------------------------------------- G16
def gen_moulton():
    """method='fixed_adams' (AdamsBashforthMoulton, fixed_adams.py:151-205) over the NDCN ODEFunc on the 6 x 6 lattice at H = 8, with the
    evaluation count and, per grid step, the corrector iterations run (0: an RK4 warm-up step) and whether the step converged.  (Names
    start with moulton_: no glob of the existing tests - fixed_*, adams_*, bashforth_* - picks them up.)  The per-step record comes from
    the reference's own convergence test, wrapped while the solve runs.  Every recorded decision must have a margin, so that a last-bit
    difference between this CPU and a GPU cannot flip it: a converged iteration has max(err / tol) <= 0.5, a failed one an element with
    err >= 2 tol (or tol == 0); the step sizes and tolerances below were chosen until the reference alone satisfies that."""
    import torchdiffeq._impl.fixed_adams as ref_fa
    _, OM = grid_operator(6)
    OMs = ref_u.torch_sensor_to_torch_sparse_tensor(OM)
    h = 1.0 / 128
    lin = lambda n, dt: torch.linspace(0., n * dt, n + 1)
    cases = {
        # the drivers' tolerances (dynamics.py: rtol 0.01, atol 0.001): every step converges at the first iteration
        'default': (lin(18, 0.01), 1e-2, 1e-3, {}),
        'iterate': (lin(16, MOULTON_ITERATE[0]), MOULTON_ITERATE[1], MOULTON_ITERATE[2], {}),     # two or more iterations on some steps
        'never': (lin(16, 0.01), 0.0, 0.0, {}),                                   # err < 0 is false: max_iters iterations, history stays at 3
        'one_iter': (lin(16, MOULTON_ONE[0]), MOULTON_ONE[1], MOULTON_ONE[2], {'max_iters': 1}),
        'order4': (lin(16, 0.01), 1e-2, 1e-3, {'max_order': 4}),
        'stepsize': (torch.tensor([0., 1.5 * h, 4 * h, 4.3 * h, 4.6 * h, 9 * h, 14 * h]), 1e-2, 1e-3, {'step_size': h}),
        'warmup': (torch.tensor([0., 0.01, 0.02]), 1e-2, 1e-3, {}),
    }
    for name, (t, rtol, atol, opts) in cases.items():
        f, x = make_func(8, OMs, 53)
        cf = CountingFunc(f)
        calls, steps = [], []
        orig_conv, orig_step = ref_fa._has_converged, ref_fa.AdamsBashforthMoulton.step_func

        def conv(y0, y1, rt, at):
            out = orig_conv(y0, y1, rt, at)
            tol = at + rt * torch.max(torch.abs(y0[0]), torch.abs(y1[0]))
            err = torch.abs(y0[0] - y1[0])
            if bool(out):
                assert float((err / tol).max()) <= 0.5, (name, len(steps), float((err / tol).max()))
            else:
                assert bool((tol == 0).all()) or bool((err >= 2 * tol).any()), (name, len(steps))
            calls.append(bool(out))
            return out

        def step(self, func, tt, dt, y):
            n0 = len(calls)
            dy = orig_step(self, func, tt, dt, y)
            steps.append((len(calls) - n0, all(calls[n0:][-1:])))
            return dy

        ref_fa._has_converged, ref_fa.AdamsBashforthMoulton.step_func = conv, step
        err_text = io.StringIO()
        try:
            with torch.no_grad(), contextlib.redirect_stderr(err_text):
                y = ref_ode.odeint(cf, x, t, rtol=rtol, atol=atol, method='fixed_adams', options=dict(opts) if opts else None)
        finally:
            ref_fa._has_converged, ref_fa.AdamsBashforthMoulton.step_func = orig_conv, orig_step
        n_steps = len(t) - 1
        if 'step_size' in opts:
            grid, ok = ref_step_grid(t, opts['step_size'])
            assert ok
            n_steps = len(grid) - 1
            assert n_steps >= 14
        iters = np.array([s[0] for s in steps], dtype=np.int32)
        flags = np.array([int(s[1]) for s in steps], dtype=np.int32)
        assert len(steps) == n_steps
        assert bool(torch.isfinite(y).all()) and float(y.abs().max()) <= 10 * float(x.abs().max()), name
        assert cf.nfe == n_steps + 6 + int(iters.sum()), (name, cf.nfe, n_steps, iters)
        n_warn = err_text.getvalue().count('Functional iteration did not converge')
        assert n_warn == int((flags == 0).sum())
        print('moulton_%-9s iterations %s  warnings %d' % (name, iters.tolist(), n_warn))
        if name in ('default', 'order4', 'stepsize'):
            assert iters[2:].tolist() == [1] * (n_steps - 2) and flags.all()
        if name == 'iterate':
            assert iters.max() >= 2 and flags.all()
        if name == 'never':
            assert iters[2:].tolist() == [4] * (n_steps - 2) and not flags[2:].any()
        if name == 'one_iter':
            assert iters.max() == 1 and not flags.all() and flags[2:].any()
        save('moulton_%s' % name, x0=x, t=t, W=f.wt.weight, b=f.wt.bias, traj=y, nfe=cf.nfe, n_steps=n_steps, no_control=0,
             rtol=np.float64(rtol), atol=np.float64(atol), iters=iters, converged=flags, n_warnings=n_warn,
             **{'opt_' + k: v for k, v in opts.items()}, **csr_of(OM))


# (dt, rtol, atol) of moulton_iterate and of moulton_one_iter: found by scanning the reference for decisions with a margin (gen_moulton)
MOULTON_ITERATE = (0.015, 1.2e-4, 2.1e-5)
MOULTON_ONE = (0.02, 3e-4, 3e-6)


# ----------------------------------------------------------------------------- G17
def gen_tgcn():
    """TemporalGCN (neural_dynamics.py:179-238) of the reference on the CPU: 6 x 6 lattice, Kipf operator, Hg = 5, Hr = 10, 8 input
    ticks, dropout 0, for each cell type one run with future = 0 (with the gradients of l1_loss against a written target) and one with
    future = 3.  The weights are written out (sines of the element index), not seeded draws.  Per case the float32 run and the same
    module in double agree within 1e-5 of each tensor's maximum - the bound the tests hold the kernels to is one the reference itself
    meets - and no element of Z = A (x w^T + b) is within 1e-4 of the relu's kink."""
    import torch.nn.functional as F
    _, OM = grid_operator(6, 'kipf')
    N, Hg, Hr, T = 36, 5, 10, 8
    i = torch.arange(N, dtype=torch.float64)[:, None]
    tau = torch.arange(T, dtype=torch.float64)[None, :]
    X = (1.0 + 0.5 * torch.sin(0.7 * i + 0.3 * tau) + 0.05 * tau).float()
    target = (1.1 + 0.4 * torch.cos(0.5 * i - 0.2 * tau)).float()

    def written(shape, scale, phase):
        n = int(np.prod(shape))
        return (scale * torch.sin(phase + 0.37 * torch.arange(n, dtype=torch.float64) ** 1.1)).reshape(shape).float()

    for rnn_type in ('lstm', 'gru', 'rnn'):
        def make(dtype):
            m = ref_nd.TemporalGCN(1, Hg, N, Hr, OM.to(dtype), dropout=0.0, rnn_type=rnn_type)
            with torch.no_grad():
                m.gc.fc.weight.copy_(torch.tensor([[0.9], [-0.7], [0.5], [-0.3], [0.8]]))
                m.gc.fc.bias.copy_(torch.tensor([0.2, 0.35, -0.4, 0.25, -0.3]))
                m.rnn.weight_ih.copy_(written(m.rnn.weight_ih.shape, 0.15, 0.1))
                m.rnn.weight_hh.copy_(written(m.rnn.weight_hh.shape, 0.4, 0.7))
                m.rnn.bias_ih.copy_(written(m.rnn.bias_ih.shape, 0.2, 1.3))
                m.rnn.bias_hh.copy_(written(m.rnn.bias_hh.shape, 0.2, 2.1))
                m.linear.weight.copy_(written(m.linear.weight.shape, 0.5, 0.4))
                m.linear.bias.copy_(written(m.linear.bias.shape, 0.3, 1.9) + 1.0)
            return m.to(dtype)

        def run(dtype):
            m = make(dtype)
            # the reference's forward builds its initial state in float32 whatever the module's dtype: run the double module with the
            # default dtype switched, as its own comment at :205-208 describes
            old = torch.get_default_dtype()
            torch.set_default_dtype(dtype)
            try:
                out0 = m(X.to(dtype))
                loss = F.l1_loss(out0, target.to(dtype))
                grads = torch.autograd.grad(loss, list(m.parameters()))
                with torch.no_grad():
                    out3 = m(X.to(dtype), future=3)
            finally:
                torch.set_default_dtype(old)
            return m, out0.detach(), out3, dict(zip([k for k, _ in m.named_parameters()], grads))

        m32, out0, out3, g32 = run(torch.float32)
        m64, out0d, out3d, g64 = run(torch.float64)
        close = lambda a, b: float((a.double() - b).abs().max()) <= 1e-5 * float(b.abs().max())
        assert tuple(out0.shape) == (N, T) and tuple(out3.shape) == (N, T + 3)
        assert close(out0, out0d) and close(out3, out3d), rnn_type
        for k in g32:
            assert close(g32[k], g64[k]), (rnn_type, k)
        # Z of every tick, the three fed-back ones included
        Zmin = np.inf
        for col in torch.cat([X.double(), out3d[:, T - 1:-1]], 1).t():
            Z = OM.double() @ (col[:, None] @ m64.gc.fc.weight.t() + m64.gc.fc.bias)
            Zmin = min(Zmin, float(Z.abs().min()))
        assert Zmin >= 1e-4, (rnn_type, Zmin)
        print('tgcn_%-5s min |Z| %.3e' % (rnn_type, Zmin))
        save('tgcn_%s' % rnn_type, A=OM, X=X, target=target, out_future0=out0, out_future3=out3,
             **{k: v for k, v in m32.state_dict().items()}, **{'grad.' + k: v for k, v in g32.items()})


if __name__ == '__main__':
    which = sys.argv[1:] or ['layout', 'gconv', 'rhs', 'fixed', 'dopri5', 'ndcn', 'truth', 'operators', 'dgnn', 'dataset', 'planetoid_raw', 'adjoint', 'resgcn', 'adams', 'substep', 'bashforth', 'moulton', 'tgcn']
    for w in which:
        globals()['gen_' + w]()
