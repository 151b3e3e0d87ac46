"""Dropout inside the one-launch right-hand side for hidden widths 16..128 (csrc/rhs_mid.hip, DROP; ndcn_set_rhs_mid_drop): every launch
goes through the public calls (ndcn_rhs_drop_f32 / ndcn_rhs_rk_drop_f32) with ndcn_set_rhs_mid(2) and ndcn_set_rhs_mid_drop(1) and
asserts ndcn_debug_last_rhs_path() == NDCN_PATH_MID | NDCN_PATH_DROP_EPI exactly.  K', y_next and y_aux are compared as int32 words
(+0 / -0, NaN positions and payloads count), the error record as fp64 words.

  the mask   K' of the plain dropout launch = float32(K * m) word for word, K the p = 0 launch of the same route (tests/test_gpu_rhs_mid.py
             proves that one equal to the composed path) and m from tests/_philox.py - no device code on the mask's side
  composed   the sequence rhs.hip falls back to, call by call through the C ABI: ndcn_spmm_f32 -> ndcn_linear_f32 (bias, ReLU) ->
             ndcn_dropout_combine_f32 (COMBINE without y_aux) or ndcn_dropout_apply_f32 + ndcn_rk_combine_f32 (twice with y_aux) /
             ndcn_fixed_stage_f32 / ndcn_rk_error_f32
  two tiles  16 449 rows = 258 tiles on 256 workgroups at H = 100 and 128, against the same call with the dropout switch off - above 2^18
             elements that call is the composed form itself (path 0 asserted)
  declines   a halo panel stays NDCN_EINVAL; a misaligned y_next runs composed; ndcn_set_rhs_mid(0) makes the dropout switch inert

Inputs: the recipe of tests/test_gpu_rhs_mid.py (helpers copied): X = rand - 0.3, y0 and the stages randn rows scaled by 2^j, W and b
uniform in +-1/16, coefficients with a zero and negative ones, the special set planted in y0 and every earlier stage in turn."""
import contextlib

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import _philox

pytestmark = pytest.mark.gpu
F = np.float32
CS = [F(c) for c in (0.11, 0.0, 0.23, 0.05, -0.31, -0.19)]          # [5]: the new stage's
AUX = [F(c) for c in (0.013, -0.02, 0.0, 0.007, -0.011, 0.017)]
SPECIALS = (0.0, -0.0, 1e-40, -1e-40, 1e-20, -1.5e-19, 3e38, -3e38, float('inf'), -float('inf'), float('nan'))
DT = F(0.37)
RTOL, ATOL = F(1e-2), F(1e-3)
SMALL_MAX = 1 << 18
WIDTHS = (16, 20, 32, 64, 100, 128)
PS = (0.5, 0.3, 0.999, 1e-6)
SEED = 1234567
BIG_SEED, BIG_EVAL = 2 ** 40 + 17, 2 ** 33 + 5                        # the high words of key and counter


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


def want_path():
    return _L().PATH_MID | _L().PATH_DROP_EPI


@contextlib.contextmanager
def switches(mode, drop):
    from ndcn_amd import hip
    prev, prev_drop = hip.set_rhs_mid(mode), hip.set_rhs_mid_drop(drop)
    try:
        yield
    finally:
        hip.set_rhs_mid(prev)
        hip.set_rhs_mid_drop(prev_drop)


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


def matrix(n, nc, seed):
    """n x nc, row r with (r + seed) % 71 entries (0..70) at distinct columns"""
    assert nc % 13 and nc >= 71
    deg = (np.arange(n) + seed) % 71
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
    def __init__(self, n, H, dev, seed=1):
        nc = max(n, 256) + (1 if max(n, 256) % 13 == 0 else 0)
        self.n, self.H, self.dev = n, H, dev
        self.m = matrix(n, nc, seed)
        self.A = op(self.m, dev)
        g = torch.Generator(device=dev).manual_seed(seed)
        self.X = torch.rand(nc, H, generator=g, device=dev) - 0.3
        self.y0 = rows_scaled(n, H, g, dev)
        self.ks = [rows_scaled(n, H, g, dev) for _ in range(5)]
        self.W = (torch.rand(H, H, generator=g, device=dev) - 0.5) / 8
        self.b = (torch.rand(H, generator=g, device=dev) - 0.5) / 8
        self.name = 'n=%d H=%d' % (n, H)
        self._K = None

    def composed_K(self):
        """the unmasked K of the composed calls, formed once (the callers clone it: the dropout passes work in place)"""
        from ndcn_amd import hip
        if self._K is None:
            self._K = hip.linear(hip.spmm(self.A, self.X), self.W, self.b, relu=True)
        return self._K

    def composed(self, mode, y0, ks, cs, drop, aux_cs=None):
        """[K', outputs...] of the sequence rhs.hip falls back to"""
        from ndcn_amd import hip
        K = self.composed_K().clone()
        if mode == 'plain':
            return [hip.dropout_apply(K, drop)]
        if mode == 'combine' and aux_cs is None:
            K, y = hip.dropout_combine(K, drop, ks, cs, y0=y0)
            return [K, y]
        hip.dropout_apply(K, drop)
        if mode == 'combine':
            return [K, hip.combine(y0, ks + [K], cs), hip.lincomb(ks + [K], aux_cs)]
        if mode == 'rk4':
            kk = ks + [K]
            return [K, hip.fixed_stage(2 + len(ks), y0, kk[0], *kk[1:], dt=float(cs[0]))]
        return [K, hip.error(y0, self.X[:self.n].contiguous(), ks + [K], cs, RTOL, ATOL)]

    def launch(self, mode, y0, ks, cs, drop, aux_cs=None, X=None, **kw):
        from ndcn_amd import hip
        X = self.X if X is None else X
        if mode == 'plain':
            out = (hip.rhs(self.A, X, self.W, self.b, dropout=drop, **kw),)
        else:
            out = hip.rhs_rk(self.A, X, self.W, self.b, mode, y0, ks, cs, rtol=RTOL, atol=ATOL, aux_cs=aux_cs, dropout=drop, **kw)
        torch.cuda.synchronize()
        return out

    def check(self, mode, y0, ks, cs, drop, aux_cs=None, what=''):
        want = self.composed(mode, y0, ks, cs, drop, aux_cs)
        with switches(2, 1):
            got = self.launch(mode, y0, ks, cs, drop, aux_cs)
            assert rhs_path() == want_path(), '%s %s %s: path %#x, want PATH_MID | PATH_DROP_EPI' % (self.name, mode, what, rhs_path())
        assert len(got) == len(want)
        for i, (a, b) in enumerate(zip(got, want)):
            label = '%s %s %s: %s' % (self.name, mode, what, ("K'", 'y_next', 'y_aux')[i] if mode != 'error' or i == 0 else 'record')
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

    def all_modes(self, p):
        ev = 0
        self.check('plain', None, [], [], (p, SEED, ev))
        for npv, aux in ((0, False), (1, False), (2, False), (3, False), (4, False), (5, False), (0, True), (4, True), (5, True)):
            cs, c2 = CS[:npv] + [CS[5]], (AUX[:npv] + [AUX[5]]) if aux else None
            for label, y0, ks in self.targets(npv):
                ev += 1
                self.check('combine', y0, ks, cs, (p, SEED, ev), c2, 'np=%d aux=%s %s' % (npv, aux, label))
        for st in range(4):
            for label, y0, ks in self.targets(st):
                ev += 1
                self.check('rk4', y0, ks, [DT], (p, SEED, ev), None, 'stage %d %s' % (st, label))
        for npv in (0, 5):
            for label, y0, ks in self.targets(npv):
                ev += 1
                self.check('error', y0, ks, CS[:npv] + [CS[5]], (p, SEED, ev), None, 'np=%d %s' % (npv, label))


def host_product(K, m):
    """float32(K * m) on the host, one rounded product per element"""
    with np.errstate(all='ignore'):
        return (K.astype(np.float32) * m.astype(np.float32)).astype(np.float32)


def host_same(got, want, what):
    """word for word; a NaN matches a NaN (the host and the device may disagree on the payload of Inf * 0)"""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    bad = (got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want))
    assert not bad.any(), '%s: %d of %d words differ from float32(K * m); first at %s' % (what, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]))


def plain_pair(c, drop, X=None):
    """(K of the p = 0 launch, K' of the dropout launch) on the one-launch route, as host arrays"""
    with switches(2, 1):
        K, = c.launch('plain', None, [], [], None, X=X)
        assert rhs_path() == _L().PATH_MID
        Kd, = c.launch('plain', None, [], [], drop, X=X)
        assert rhs_path() == want_path(), '%s p=%r: path %#x' % (c.name, drop[0], rhs_path())
    return K.cpu().numpy(), Kd.cpu().numpy()


@pytest.mark.parametrize('H', WIDTHS)
def test_mask_against_the_host(dev, H):
    """K' = float32(K * m) with m from the numpy Philox: n around the 64-row tile, four probabilities, a different evaluation per launch"""
    ev = 0
    for n in (1, 63, 64, 65, 129):
        c = Case(n, H, dev, seed=n)
        for p in PS:
            ev += 1
            K, Kd = plain_pair(c, (p, SEED + H, ev))
            m = _philox.mask(p, SEED + H, ev, n, H)
            assert not np.isnan(K).any()
            assert np.array_equal(Kd.view(np.uint32), host_product(K, m).view(np.uint32)), '%s p=%r' % (c.name, p)
            if n == 129 and p in (0.5, 0.3):                    # the mask is neither empty nor full, and is not the ReLU's pattern
                live = K > 0
                assert 0 < int((m[live] == 0).sum()) < int(live.sum())
                assert np.array_equal(Kd[live] != 0, m[live] != 0)


def test_mask_high_words_of_seed_and_evaluation(dev):
    c = Case(129, 20, dev, seed=21)
    K, Kd = plain_pair(c, (0.5, BIG_SEED, BIG_EVAL))
    m = _philox.mask(0.5, BIG_SEED, BIG_EVAL, c.n, c.H)
    assert np.array_equal(Kd.view(np.uint32), host_product(K, m).view(np.uint32))
    low = _philox.mask(0.5, BIG_SEED & 0xffffffff, BIG_EVAL & 0xffffffff, c.n, c.H)
    assert not np.array_equal(m, low)                           # the high words do enter the mask


def test_mask_on_non_finite_K(dev):
    """specials planted in X: K holds Inf and NaN, and a dropped Inf or NaN is NaN (x * 0), never 0"""
    c = Case(129, 64, dev, seed=23)
    X = plant(c.X, 3)
    deg = np.diff(c.m.indptr)
    for r in np.flatnonzero(deg == 1):                          # rows of one entry: their S row gets exactly one Inf -> K = +Inf or 0
        col = int(c.m.indices[c.m.indptr[r]])
        X[col] = 0.25
        X[col, 1] = float('inf')
    drop = (0.5, SEED, 9)
    K, Kd = plain_pair(c, drop, X=X)
    m = _philox.mask(*drop, c.n, c.H)
    assert np.isinf(K).any() and np.isnan(K).any()
    host_same(Kd, host_product(K, m), c.name)
    dropped = m == 0
    assert int((np.isinf(K) & dropped).sum()) > 0 and int((np.isnan(K) & dropped).sum()) > 0
    assert np.isnan(Kd[~np.isfinite(K) & dropped]).all()
    assert (Kd[np.isfinite(K) & dropped] == 0).all()
    # and the composed pass agrees on every word, payloads included
    from ndcn_amd import hip
    Kc = hip.dropout_apply(hip.linear(hip.spmm(c.A, X), c.W, c.b, relu=True), drop)
    same(torch.from_numpy(Kd).to(dev), Kc, "%s K' against ndcn_dropout_apply_f32" % c.name)


@pytest.mark.parametrize('H', WIDTHS)
def test_against_the_composed_calls(dev, H):
    """129 rows = two tiles and a last tile of one row: plain, COMBINE with 0..5 earlier stages (with and without y_aux), RK4 stages
    0..3, ERROR with 0 and 5; the special set in y0 and in each earlier stage in turn"""
    Case(129, H, dev, seed=31).all_modes(0.5 if H != 20 else 0.3)


@pytest.mark.parametrize('H', (100, 128))
def test_more_tiles_than_workgroups(dev, H):
    """16 449 rows = 258 tiles on 256 workgroups (P = 128: one workgroup per CU): two workgroups run a second tile, the last tile is one
    row.  COMBINE with 5 earlier stages against the same call with the dropout switch off: the composed form (no path bit)"""
    L = _L()
    c = Case(16449, H, dev, seed=5)
    assert c.n * H > SMALL_MAX
    drop = (0.5, SEED, 77)
    y0, ks = plant(c.y0, 1), [plant(k, 2 + j) for j, k in enumerate(c.ks)]
    with switches(2, 0):
        want = c.launch('combine', y0, ks, CS, drop)
        assert rhs_path() & (L.PATH_MID | L.PATH_DROP_EPI) == 0, hex(rhs_path())
    with switches(2, 1):
        got = c.launch('combine', y0, ks, CS, drop)
        assert rhs_path() == want_path(), hex(rhs_path())
    for name, a, b in zip(("K'", 'y_next'), got, want):
        same(a, b, '%s COMBINE 5: %s' % (c.name, name))
    with switches(2, 1):                                       # every tile carries the mask of its own rows
        K, = c.launch('plain', None, [], [], None)
    want_K = host_product(K.cpu().numpy(), _philox.mask(*drop, c.n, H))
    assert np.array_equal(got[0].cpu().numpy().view(np.uint32), want_K.view(np.uint32))
    assert (want_K[-1] != 0).any() and (want_K[64:128] != 0).any() and (want_K[192:256] != 0).any()     # tiles 1 and 3: the second ones


def test_declines_with_the_switch_on(dev):
    L = _L()
    from ndcn_amd import hip
    drop = (0.3, 17, 5)
    for n in (129, SMALL_MAX // 64 + 66):
        c = Case(n, 64, dev, seed=13)
        # a halo panel with dropout: refused as before
        n_own = c.X.shape[0] - 40
        X, Xh = c.X[:n_own].contiguous(), c.X[n_own:].contiguous()
        with switches(2, 1):
            with pytest.raises(L.NdcnHipError) as e:
                hip.rhs(c.A, X, c.W, c.b, X_halo=Xh, dropout=drop)
            assert e.value.code == L.EINVAL and 'halo' in str(e.value)
            with pytest.raises(L.NdcnHipError) as e:
                hip.rhs_rk(c.A, X, c.W, c.b, 'combine', c.y0, c.ks[:2], CS[:2] + [CS[5]], X_halo=Xh, dropout=drop)
            assert e.value.code == L.EINVAL
        # a misaligned y_next: the launch runs as without the switch, the same bits
        runs = {}
        for on in (0, 1):
            buf = torch.zeros(n * 64 + 4, device=dev)
            view = buf[1:1 + n * 64].view(n, 64)
            assert view.data_ptr() % 16 == 4
            with switches(2, on):
                K, y = c.launch('combine', c.y0, c.ks, CS, drop, out_y=view)
                runs[on] = (K, y.clone(), rhs_path())
        assert runs[1][2] == runs[0][2] and not runs[1][2] & L.PATH_MID, [hex(r[2]) for r in runs.values()]
        same(runs[1][0], runs[0][0], "n=%d misaligned y_next: K'" % n)
        same(runs[1][1], runs[0][1], 'n=%d misaligned y_next: y_next' % n)
        with switches(2, 1):                                   # ... and agrees with the aligned launch, which does take the route
            K, y = c.launch('combine', c.y0, c.ks, CS, drop)
            assert rhs_path() == want_path()
        same(runs[1][0], K, "n=%d misaligned against aligned: K'" % n)
        same(runs[1][1], y, 'n=%d misaligned against aligned: y_next' % n)
        # ndcn_set_rhs_mid(0): the dropout switch alone changes nothing
        runs = {}
        for on in (0, 1):
            with switches(0, on):
                out = [c.launch('plain', None, [], [], drop)]
                paths = [rhs_path()]
                out.append(c.launch('combine', c.y0, c.ks, CS, drop))
                paths.append(rhs_path())
                out.append(c.launch('combine', c.y0, c.ks[:4], CS[:4] + [CS[5]], drop, AUX[:4] + [AUX[5]]))
                paths.append(rhs_path())
                out.append(c.launch('rk4', c.y0, c.ks[:2], [DT], drop))
                paths.append(rhs_path())
                assert not any(p & L.PATH_MID for p in paths), [hex(p) for p in paths]
                runs[on] = (out, paths)
        assert runs[0][1] == runs[1][1]
        for i, (a, b) in enumerate(zip(runs[0][0], runs[1][0])):
            for j, (u, v) in enumerate(zip(a, b)):
                same(v, u, 'n=%d mode 0, launch %d output %d' % (n, i, j))
