"""The one-launch right-hand side for hidden widths 16..128 at any size (csrc/rhs_mid.hip, NDCN_PATH_MID, ndcn_set_rhs_mid) against the
composed path of csrc/rhs.hip - row SpMM into S, MFMA Linear, stand-alone stage kernel - BIT FOR BIT: K, y_next and y_aux are compared as
int32 (torch.equal on the raw words: +0 / -0 and NaN positions and payloads count), the error record as fp64 words.  Every case launches
through the C ABI (ndcn_rhs_f32 / ndcn_rhs_rk_f32) in mode 2 and asserts ndcn_debug_last_rhs_path() == NDCN_PATH_MID exactly.

The composed side.  Above 2^18 elements it is the same call in mode 0, path 0 asserted.  At or below 2^18 elements mode 0 is NOT composed:
rhs_small.hip takes the launch (path NDCN_PATH_SMALL), and that kernel's stage sums start from the new stage's product, not from +0 (header
of tests/test_gpu_rhs_rk_routes.py: from_zero), and its error record is summed inside the launch - other bits for an all-zero sum and for
the record.  There the composed side is what rhs.hip's fallback itself issues, call by call through the C ABI: ndcn_spmm_f32 (alpha 1, no
activation) -> ndcn_linear_f32 (bias, ReLU) -> ndcn_rk_combine_f32 / ndcn_fixed_stage_f32 (op 2 + stage) / ndcn_rk_error_f32.  Every width
also has a case above 2^18 elements where both forms of the composed side are compared with each other and with the launch.

Inputs (the recipe of tests/test_gpu_rhs_rk_routes.py): X = rand - 0.3 (the ReLU cuts), y0 and the stages randn rows scaled by 2^j,
j in [-8, 8], W and b uniform in +-1/16, coefficients (0.11, 0, 0.23, 0.05, -0.31 | -0.19) - a zero, negative ones, the new stage's
negative: -0 products - and the special set {+-0, +-1e-40, 1e-20, -1.5e-19, +-3e38, +-Inf, NaN} planted in y0 and in every earlier stage
in turn.

Shapes, from the kernel's constants: the tile is 64 rows (kMidTile): n in {1, 63, 64, 65, 129}.  The grid is
min(tiles, 256 * min(4, 160 KiB / ((P + 64) (P + 1) 4 bytes))) with P = ceil32(H): 256 workgroups at H = 100 and 128 (P = 128: 99 072
bytes of LDS), so n = 16 449 rows = 258 tiles gives two workgroups a second tile and a last tile of one row.  Row lengths cycle through
0..70: empty rows, rows beyond the gather's unroll of 4 and each of its tails 0..3; one case has a hub row of 2 000 entries.  Widths
16, 20, 32 (P = 32, 8 lanes per row; 20: a ragged MFMA tile), 64 (16 lanes), 100 and 128 (32 lanes; 100: ragged)."""
import contextlib

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import _rk_epilogue as E
from _fma_chain import chain, fma32

pytestmark = pytest.mark.gpu
F = np.float32
CS = [F(c) for c in (0.11, 0.0, 0.23, 0.05, -0.31, -0.19)]          # [5]: the new stage's
AUX = [F(c) for c in (0.013, -0.02, 0.0, 0.007, -0.011, 0.017)]
SPECIALS = (0.0, -0.0, 1e-40, -1e-40, 1e-20, -1.5e-19, 3e38, -3e38, float('inf'), -float('inf'), float('nan'))
DT = F(0.37)
RTOL, ATOL = F(1e-2), F(1e-3)
SMALL_MAX = 1 << 18
WIDTHS = (16, 20, 32, 64, 100, 128)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    from ndcn_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


def _L():
    from ndcn_amd import _lib
    return _lib


def rhs_path():
    return int(_L().load().ndcn_debug_last_rhs_path())


def rk_path():
    return int(_L().load().ndcn_debug_last_rk_path())


@contextlib.contextmanager
def mid(mode):
    from ndcn_amd import hip
    prev = hip.set_rhs_mid(mode)
    try:
        yield
    finally:
        hip.set_rhs_mid(prev)


def bits(t):
    return t.contiguous().view(torch.int32)


def same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not torch.equal(bits(got), bits(want)):
        bad = (bits(got) != bits(want)).nonzero()
        i = tuple(int(v) for v in bad[0])
        raise AssertionError('%s: %d of %d words differ; first at %s: got %r (%#010x) want %r (%#010x)' % (
            what, bad.shape[0], got.numel(), i, float(got[i]), int(bits(got)[i]) & 0xffffffff, float(want[i]), int(bits(want)[i]) & 0xffffffff))


def same_record(got, want, what):
    g, w = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.array_equal(g.view(np.uint64), w.view(np.uint64)), (what, got, want)


def rows_scaled(n, H, gen, dev, k=8):
    x = torch.randn(n, H, generator=gen, device=dev)
    return x * torch.exp2(torch.randint(-k, k + 1, (n, 1), generator=gen, device=dev).float())


def plant(t, shift):
    """a copy of t with the special set threaded through it: every third row holds SPECIALS[(r / 3 + shift) % 11] in column (7 r + shift) % H"""
    t = t.clone()
    n, H = t.shape
    r = torch.arange(0, n, 3, device=t.device)
    vals = torch.tensor(SPECIALS, dtype=torch.float32, device=t.device)
    t[r, (7 * r + shift) % H] = vals[(r // 3 + shift) % len(SPECIALS)]
    return t


def matrix(n, nc, seed, hub=None):
    """n x nc, row r with (r + seed) % 71 entries (0..70) at distinct columns; hub: that row gets 2 000 entries instead"""
    assert nc % 13 and nc >= 71
    deg = (np.arange(n) + seed) % 71
    if hub is not None:
        assert nc >= 2000
        deg[hub] = 2000
    rows = np.repeat(np.arange(n), deg)
    j = np.arange(rows.size) - np.repeat(np.cumsum(deg) - deg, deg)
    cols = (rows * 7 + j * 13) % nc                          # 13 and nc coprime: distinct within a row
    val = (np.random.RandomState(seed).randn(rows.size) / 4).astype(np.float32)
    m = sp.csr_matrix((val, (rows, cols)), shape=(n, nc))
    m.sort_indices()
    assert m.nnz == rows.size
    return m


def op(m, dev):
    from ndcn_amd import CsrOperator
    A = CsrOperator.from_arrays(m.indptr, m.indices, m.data, m.shape, dev)
    A._plans_tried = True
    return A


class Case:
    def __init__(self, n, H, dev, seed=1, hub=None, nc=None):
        nc = nc or max(n, 256) + (1 if max(n, 256) % 13 == 0 else 0)
        self.n, self.H, self.dev = n, H, dev
        self.m = matrix(n, nc, seed, hub)
        self.A = op(self.m, dev)
        g = torch.Generator(device=dev).manual_seed(seed)
        self.X = torch.rand(nc, H, generator=g, device=dev) - 0.3
        self.y0 = rows_scaled(n, H, g, dev)
        self.ks = [rows_scaled(n, H, g, dev) for _ in range(5)]
        self.W = (torch.rand(H, H, generator=g, device=dev) - 0.5) / 8
        self.b = (torch.rand(H, generator=g, device=dev) - 0.5) / 8
        self.small = n * H <= SMALL_MAX
        self.name = 'n=%d H=%d' % (n, H)

    # ---- the composed side, call by call (what rhs.hip's fallback issues)
    def composed_K(self):
        from ndcn_amd import hip
        return hip.linear(hip.spmm(self.A, self.X), self.W, self.b, relu=True)

    def composed(self, mode, y0, ks, cs, K, aux_cs=None):
        from ndcn_amd import hip
        if mode == 'combine':
            out = [hip.combine(y0, ks + [K], cs)]
            if aux_cs is not None:
                out.append(hip.lincomb(ks + [K], aux_cs))
            return out
        if mode == 'rk4':
            kk = ks + [K]
            return [hip.fixed_stage(2 + len(ks), y0, kk[0], *kk[1:], dt=float(cs[0]))]
        return [hip.error(y0, self.X[:self.n].contiguous(), ks + [K], cs, RTOL, ATOL)]

    def launch(self, mode, y0, ks, cs, aux_cs=None, **kw):
        from ndcn_amd import hip
        if mode == 'plain':
            out = (hip.rhs(self.A, self.X, self.W, self.b, **kw),)
        else:
            out = hip.rhs_rk(self.A, self.X, self.W, self.b, mode, y0, ks, cs, rtol=RTOL, atol=ATOL, aux_cs=aux_cs, **kw)
        torch.cuda.synchronize()
        return out

    def reference(self, mode, y0, ks, cs, aux_cs=None):
        """[K, outputs...] of the composed path; above 2^18 elements from the launch in mode 0 (path 0) AND call by call, compared"""
        K = self.composed_K()
        parts = [K] + (self.composed(mode, y0, ks, cs, K, aux_cs) if mode != 'plain' else [])
        if not self.small:
            with mid(0):
                out = self.launch(mode, y0, ks, cs, aux_cs)
                assert rhs_path() == 0, '%s %s in mode 0: path %#x' % (self.name, mode, rhs_path())
            for i, (a, b) in enumerate(zip(out, parts)):
                if mode == 'error' and i == 1:
                    same_record(a, b, '%s %s: record, mode 0 against the composed calls' % (self.name, mode))
                else:
                    same(a, b, '%s %s: output %d, mode 0 against the composed calls' % (self.name, mode, i))
        return parts

    def check(self, mode, y0, ks, cs, aux_cs=None, what=''):
        L = _L()
        want = self.reference(mode, y0, ks, cs, aux_cs)
        with mid(2):
            got = self.launch(mode, y0, ks, cs, aux_cs)
            assert rhs_path() == L.PATH_MID, '%s %s %s: path %#x, want PATH_MID' % (self.name, mode, what, rhs_path())
            if mode == 'error':
                assert rk_path() & L.RKF_KERNEL_MASK == L.RKF_ERROR, hex(rk_path())
        assert len(got) == len(want)
        for i, (a, b) in enumerate(zip(got, want)):
            label = '%s %s %s: %s' % (self.name, mode, what, ('K', 'y_next', 'y_aux')[i] if mode != 'error' or i == 0 else 'record')
            if mode == 'error' and i == 1:
                same_record(a, b, label)
            else:
                same(a, b, label)
        return got

    def targets(self, npv):
        yield 'plain inputs', self.y0, self.ks[:npv]
        yield 'specials in y0', plant(self.y0, 1), self.ks[:npv]
        for j in range(npv):
            yield 'specials in stage %d' % j, self.y0, self.ks[:j] + [plant(self.ks[j], 2 + j)] + self.ks[j + 1:npv]

    def all_modes(self, specials=True):
        self.check('plain', None, [], [])
        for npv, aux in ((0, False), (2, False), (5, False), (4, True)):
            cs, c2 = CS[:npv] + [CS[5]], (AUX[:npv] + [AUX[5]]) if aux else None
            for label, y0, ks in self.targets(npv):
                if specials or label == 'plain inputs':
                    self.check('combine', y0, ks, cs, c2, 'np=%d aux=%s %s' % (npv, aux, label))
        for st in range(4):
            for label, y0, ks in self.targets(st):
                if specials or label == 'plain inputs':
                    self.check('rk4', y0, ks, [DT], None, 'stage %d %s' % (st, label))
        for npv in (0, 5):
            for label, y0, ks in self.targets(npv):
                if specials or label == 'plain inputs':
                    self.check('error', y0, ks, CS[:npv] + [CS[5]], None, 'np=%d %s' % (npv, label))


@pytest.mark.parametrize('H', WIDTHS)
def test_tile_edges(dev, H):
    """n around the 64-row tile, rows of 0..70 entries, every mode, the special set in y0 and every earlier stage"""
    for n in (1, 63, 64, 65, 129):
        Case(n, H, dev, seed=n).all_modes()


@pytest.mark.parametrize('H', WIDTHS)
def test_beyond_the_narrow_kernel(dev, H):
    """n H > 2^18: mode 0 is the composed path itself (path 0); a ragged last tile"""
    n = SMALL_MAX // H + 66
    c = Case(n, H, dev, seed=3)
    assert not c.small
    c.all_modes(specials=False)
    c.check('combine', plant(c.y0, 1), [plant(k, 2 + j) for j, k in enumerate(c.ks)], CS, AUX, 'specials everywhere')


@pytest.mark.parametrize('H', (100, 128))
def test_more_tiles_than_workgroups(dev, H):
    """16 449 rows = 258 tiles on 256 workgroups (P = 128: one workgroup per CU): two workgroups run a second tile, the last tile is one row"""
    c = Case(16449, H, dev, seed=5)
    c.all_modes(specials=False)
    c.check('rk4', plant(c.y0, 1), [plant(k, 2 + j) for j, k in enumerate(c.ks[:3])], [DT], None, 'specials everywhere')


@pytest.mark.parametrize('H', (20, 128))
def test_hub_row(dev, H):
    """one row of 2 000 entries among rows of 0..70"""
    c = Case(129, H, dev, seed=7, hub=70, nc=2049)
    assert int(np.diff(c.m.indptr).max()) == 2000
    c.check('plain', None, [], [])
    c.check('combine', plant(c.y0, 1), c.ks, CS, AUX, 'np=5 aux')
    c.check('rk4', c.y0, c.ks[:3], [DT], None, 'stage 3')
    c.check('error', c.y0, c.ks, CS, None, 'np=5')


def linear_chain(S, W, b):
    """relu_nan(fma chain over h from +0, then + b): linear_f32 (tests/test_gpu_linear_routes.py: the fp32 MFMA is such a chain)"""
    acc = np.zeros((S.shape[0], W.shape[0]), np.float32)
    for h in range(S.shape[1]):
        acc = fma32(S[:, h:h + 1], W[:, h][None, :], acc)
    with np.errstate(all='ignore'):
        k = acc + b[None, :]
        return np.where(k < 0, F(0), k).astype(np.float32)


def host_same(got, want, what):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    bad = (got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want))
    assert not bad.any(), '%s: %d of %d elements differ from the host oracle; first at %s' % (what, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]))


def test_against_the_host_oracle(dev):
    """no device kernel on the expected side: S by tests/_fma_chain.py, K = relu_nan(chain over h from +0, + b), the stage algebra by
    tests/_rk_epilogue.py in its from_zero form (any NaN matches any NaN)"""
    c = Case(129, 20, dev, seed=11)
    L = _L()
    S = chain(c.m.indptr, c.m.indices, c.m.data, c.X.cpu().numpy())
    Kh = linear_chain(S, c.W.cpu().numpy(), c.b.cpu().numpy())
    y0 = plant(c.y0, 1)
    ks = [plant(k, 2 + j) for j, k in enumerate(c.ks)]
    with mid(2):
        K, = c.launch('plain', None, [], [])
        assert rhs_path() == L.PATH_MID
        host_same(K.cpu().numpy(), Kh, 'K')
        K2, yn, ya = c.launch('combine', y0, ks, CS, AUX)
        assert rhs_path() == L.PATH_MID
        same(K2, K, 'K of the COMBINE launch against the plain launch')
        kk = [k.cpu().numpy() for k in ks] + [Kh]
        host_same(yn.cpu().numpy(), E.combine(y0.cpu().numpy(), kk, CS, from_zero=True), 'y_next')
        host_same(ya.cpu().numpy(), E.aux(kk, AUX, from_zero=True), 'y_aux')
        for st in range(4):
            K3, y4 = c.launch('rk4', y0, ks[:st], [DT])
            assert rhs_path() == L.PATH_MID
            same(K3, K, 'K of the RK4 launch against the plain launch')
            host_same(y4.cpu().numpy(), E.rk4_stage(st, y0.cpu().numpy(), [k.cpu().numpy() for k in ks[:st]] + [Kh], DT), 'rk4 stage %d' % st)


def test_declined_launches(dev):
    """a halo panel and dropout in mode 2: the launch runs as in mode 0 - no PATH_MID, the same bits - at a narrow-kernel size and beyond"""
    L = _L()
    for n in (129, SMALL_MAX // 64 + 66):
        c = Case(n, 64, dev, seed=13)
        n_own = c.X.shape[0] - 40
        X, Xh = c.X[:n_own].contiguous(), c.X[n_own:].contiguous()
        from ndcn_amd import hip
        runs = {}
        for mode in (0, 2):
            with mid(mode):
                out = []
                out.append((hip.rhs(c.A, X, c.W, c.b, X_halo=Xh),))
                p1 = rhs_path()
                out.append(hip.rhs_rk(c.A, X, c.W, c.b, 'combine', c.y0, c.ks[:2], CS[:2] + [CS[5]], X_halo=Xh, aux_cs=AUX[:2] + [AUX[5]]))
                p2 = rhs_path()
                out.append(hip.rhs_rk(c.A, X, c.W, c.b, 'rk4', c.y0, c.ks[:1], [DT], X_halo=Xh))
                p3 = rhs_path()
                out.append((hip.rhs(c.A, c.X, c.W, c.b, dropout=(0.3, 17, 5)),))
                p4 = rhs_path()
                out.append(hip.rhs_rk(c.A, c.X, c.W, c.b, 'combine', c.y0, c.ks, CS, dropout=(0.3, 17, 6)))
                p5 = rhs_path()
                out.append(hip.rhs_rk(c.A, c.X, c.W, c.b, 'combine', c.y0, c.ks[:4], CS[:4] + [CS[5]], aux_cs=AUX[:4] + [AUX[5]], dropout=(0.3, 17, 7)))
                p6 = rhs_path()
                torch.cuda.synchronize()
                paths = (p1, p2, p3, p4, p5, p6)
                assert not any(p & L.PATH_MID for p in paths), (n, mode, [hex(p) for p in paths])
                runs[mode] = (out, paths)
        assert runs[0][1][1:] == runs[2][1][1:], (runs[0][1], runs[2][1])     # ([0]: a plain narrow launch records no path of its own)
        for i, (a, b) in enumerate(zip(runs[0][0], runs[2][0])):
            for j, (u, v) in enumerate(zip(a, b)):
                same(v, u, 'n=%d declined launch %d output %d' % (n, i, j))
        with mid(2):                                           # the same operator without halo and dropout does take the route
            hip.rhs(c.A, c.X, c.W, c.b)
            assert rhs_path() == L.PATH_MID
