"""The one-launch fixed-grid solve (csrc/solve_small.hip: solve_small_kernel) restated in numpy, float32 bit for bit, as the file's
header documents it - an independent statement of the arithmetic, not another kernel of the library:

  gather   S = A T: one correctly rounded fma per stored entry, in stored order, from +0 (_fma_chain.chain; an empty row is +0);
           no_graph: S = T itself
  linear   k = fma32(S[h], W[o][h], k) over h ascending from +0, then k + b[o] as a rounding of its own (b None: + 0.0f), then
           relu_nan (v < 0 ? 0 : v: a NaN passes, -0 stays); no_control: relu_nan(S)
  stages   the operator order of _oracle_ops.OracleOps.fixed_stage (ops 0..5), every product and sum rounded separately (the kernel is
           compiled under `fp contract(off)`); RK4's last stage as the kernel forms it: ((k1 + 3 k2) + 3 k3) + k4, times dt / 8
  ticks    the default grid: every step end is a tick.  options={'step_size': h}: the steps of core.fixed_plan's grid; a tick that
           coincides with its step's end is the state itself, a tick strictly inside a step is y + ((y - y) / dt) * dt

TEST INFRASTRUCTURE: tests/test_small_solve_host.py pins it on the CPU against the reference's fixtures and the float64 oracle; the GPU
tests compare the kernels with it bit for bit."""
import numpy as np

from _fma_chain import chain, fma32

f32 = np.float32


def relu_nan(v):
    return np.where(v < 0, f32(0.0), v).astype(f32)


def rhs(op, T, W, b, no_graph=False, no_control=False):
    """K = relu_nan(W (A T) + b) for the state panel T (n, H); op = (indptr, indices, data) of a CSR with sorted or unsorted rows -
    the stored order is the summation order"""
    T = np.asarray(T, f32)
    S = T if no_graph else chain(op[0], op[1], op[2], T)
    if no_control:
        return relu_nan(S)
    W = np.asarray(W, f32)
    H = T.shape[1]
    k = np.zeros_like(S)
    for h in range(H):
        k = fma32(S[:, h:h + 1], W[:, h][None, :], k)
    with np.errstate(invalid='ignore', over='ignore'):
        k = (k + (f32(0.0) if b is None else np.asarray(b, f32)[None, :])).astype(f32)
    return relu_nan(k)


def step(f, y, dt, method):
    """one step of size dt (float32) from y; f: panel -> K"""
    dt = f32(dt)
    with np.errstate(invalid='ignore', over='ignore'):
        if method == 'euler':
            return y + dt * f(y)                                               # op 0
        if method == 'midpoint':
            ym = y + f(y) * dt / f32(2)                                        # op 1
            return y + dt * f(ym)                                              # op 0 from y
        assert method == 'rk4'
        k1 = f(y)
        k2 = f(y + dt * k1 / f32(3))                                           # op 2
        k3 = f(y + dt * (k1 / f32(-3) + k2))                                   # op 3
        k4 = f(y + dt * (k1 - k2 + k3))                                        # op 4
        s = k1 + f32(3) * k2 + f32(3) * k3                                     # the kernel keeps this prefix in k1's registers
        return y + (s + k4) * (dt / f32(8))                                    # op 5


def solve(op, W, b, y0, t, method, no_graph=False, no_control=False, step_size=None):
    """(len(t), n, H) float32: the solution at the ticks t (any float dtype; rounded to float32 as solvers.py:81 does)"""
    y = np.ascontiguousarray(y0, dtype=f32)
    t32 = np.ascontiguousarray(t, dtype=f32)
    f = lambda T: rhs(op, T, W, b, no_graph, no_control)
    out = np.empty((len(t32),) + y.shape, f32)
    out[0] = y
    if step_size is None:
        dts = t32[1:] - t32[:-1]
        for i, dt in enumerate(dts):
            y = step(f, y, dt, method)
            assert y.dtype == f32
            out[i + 1] = y
        return out
    from ndcn_amd.torchdiffeq._impl import core
    plan = core.fixed_plan(t32, step_size)
    assert plan.n_emitted == len(t32)
    for i, dt in enumerate(plan.dts):
        y = step(f, y, dt, method)
        for j, same, _ in plan.emits[i]:
            if same:
                out[j] = y
            else:
                with np.errstate(invalid='ignore', over='ignore'):
                    out[j] = y + ((y - y) / f32(dt)) * f32(dt)
    return out


# ---- operators the tests feed the solve (valid operators a driver could produce: sorted indices, at least one stored entry) -------------

def _csr(m):
    import scipy.sparse as sp
    m = sp.csr_matrix(m).astype(f32)
    m.eliminate_zeros()
    m.sort_indices()
    return m


def driver_operator(network, n=400, mean_degree=None):
    """the drivers' --network choice (at their README size by default) with the default operator (heat_dynamics.py:83-110,150-161)"""
    from ndcn_amd import graphs
    return _csr(graphs.make_operator(graphs.make_graph(network, n, seed=0, mean_degree=mean_degree), 'norm_lap'))


def band(n, longest, kind='symmetric', seed=0):
    """A banded n x n operator whose longest row has exactly `longest` entries: the diagonals 0, +-1 .. +-k clipped at the borders (rows
    of k + 1 .. 2 k + 1 entries) and, for an even `longest`, one more entry per row at distance n / 2.  kind: 'symmetric' (A = A^T in
    pattern and values), 'values' (the same pattern, A[j, i] = A[i, j] / 2 below the diagonal), 'upper' (the diagonal and the entries
    above it only)."""
    import scipy.sparse as sp
    k, extra = (longest - 1) // 2, (longest - 1) % 2
    assert (n % 2 == 0 or not extra) and n // 2 > 2 * k + 1
    r = [np.arange(n - d) for d in range(1, k + 1)] + ([np.arange(n // 2)] if extra else [])
    c = [np.arange(n - d) + d for d in range(1, k + 1)] + ([np.arange(n // 2) + n // 2] if extra else [])
    r, c = np.concatenate(r) if r else np.zeros(0, np.int64), np.concatenate(c) if c else np.zeros(0, np.int64)
    v = (np.random.default_rng(seed).uniform(-1.0, 1.0, r.size) * (2.0 / longest)).astype(f32)
    v[v == 0] = f32(0.25)
    up = sp.coo_matrix((v, (r, c)), shape=(n, n)).tocsr()
    eye = sp.identity(n, dtype=f32, format='csr')
    lower = {'symmetric': up.T, 'values': (up * f32(0.5)).T, 'upper': None}[kind]
    m = _csr(eye + up if lower is None else eye + up + lower)
    assert int(np.diff(m.indptr).max()) == (longest if lower is not None else k + 1 + extra)
    return m


def ring(n):
    """the normalised Laplacian of a ring: 3 entries per row (n = 2: 2, n = 1: the single entry 1)"""
    import scipy.sparse as sp
    m = sp.lil_matrix((n, n), dtype=f32)
    for i in range(n):
        nb = sorted({(i - 1) % n, (i + 1) % n} - {i})
        m[i, i] = 1.0
        for j in nb:
            m[i, j] = -1.0 / len(nb) if n > 2 else -0.5
    return _csr(m)


def without_nodes(m, nodes):
    """the operator with the rows and columns of `nodes` removed entirely (rows of 0 entries; the size stays)"""
    keep = np.ones(m.shape[0], bool)
    keep[list(nodes)] = False
    import scipy.sparse as sp
    d = sp.diags(keep.astype(f32))
    return _csr(d @ m @ d)


def same_bits(a, b):
    """bit equality of two float32 arrays with every NaN equal to every NaN (the position of a NaN is the statement; its payload is not:
    the fma of the device and numpy's may pick different ones)"""
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.int32)[~na], b.view(np.int32)[~nb]))
