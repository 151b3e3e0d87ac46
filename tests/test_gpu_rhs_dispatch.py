"""Which launch csrc/rhs.hip picks for one evaluation (pick(): the table on its enum class Rhs), with and without a dropout mask: every
cell calls the C ABI twice through hip.rhs / hip.rhs_rk - dropout=None, then dropout=(0.5, seed, evaluation) - and asserts

  the report   ndcn_debug_last_rhs_path() after each call, exact value, against the literals of EXPECT / EXPECT_MISALIGNED / EXPECT_FLAGS.
               They were recorded by running observe() on the commit before the two dispatches (p = 0 and dropout) became one; every
               call starts from a report of 0 (clear_path), so a plain p = 0 call - which owns only the MID bit of the report - reads
               0 on the narrow-panel and composed routes
  the outputs  K, y_next, y_aux as int32 words and the error record as fp64 words against the composed form, call by call through the
               C ABI: the unmasked K (ndcn_spmm_f32 -> ndcn_linear_f32 below H = 256; the plain p = 0 launch at H = 256 and under
               no_control, where the suite establishes no other form), ndcn_dropout_apply_f32, then ndcn_rk_combine_f32 (twice with
               y_aux) / ndcn_fixed_stage_f32 / ndcn_rk_error_f32.  One exception, as recorded: an ERROR launch whose report names a
               kernel that sums the record in its own epilogue (OWN_RECORD: the narrow-panel, H = 256 and graph-only kernels, in
               fp64) does not give ndcn_rk_error_f32's float32 sum word for word - K still does; the sum is held to the bound of
               same_record.  rhs_mid.hip's route is not among them: its ERROR launch is the plain launch plus ndcn_rk_error_f32
  the pair     where the masked call reports MID, the p = 0 call under the same switches reports MID; where it reports SMALL, the p = 0
               call reports SMALL - or MID, with ndcn_set_rhs_mid_drop off.  (A plain p = 0 call never reports SMALL: 0 stands for it.)

Shapes: the smallest at which the routes differ - (45, 20) the narrow-panel kernel's; (13108, 20) and (4097, 64) the first row counts
past its 2^18-element bound (rhs_small_wanted); (30, 256) the H = 256 kernels'; (12, 33) a width rhs_mid.hip does not take (H % 4).
Switches: ndcn_set_rhs_mid 0 / 1 / 2 x ndcn_set_rhs_mid_drop 0 / 1, restored behind every cell.

Not here: RkOpt::s_out under a mask.  rhs.hip answers it with NDCN_EINVAL, but no entry point of the C ABI takes both (ndcn_rhs_rk_adj_f32
has no descriptor, ndcn_rhs_rk_drop_f32 no s_out), so no call can reach that line.

Inputs: the recipe of tests/test_gpu_rhs_mid_drop.py (helpers copied)."""
import contextlib

import numpy as np
import pytest
import scipy.sparse as sp
import torch

pytestmark = pytest.mark.gpu
F = np.float32
CS = [F(c) for c in (0.11, 0.0, 0.23, 0.05, -0.31, -0.19)]          # [5]: the new stage's
AUX = [F(c) for c in (0.013, -0.02, 0.0, 0.007, -0.011, 0.017)]
DT = F(0.37)
RTOL, ATOL = F(1e-2), F(1e-3)
SEED = 7654321
FUSED2, WIDE, SMALL, DROP, MID = 1, 64, 128, 1024, 4096             # NDCN_PATH_*
OWN_RECORD = 1 | 2 | 32 | 64 | 128 | 256                            # launches whose ERROR epilogue sums the record itself (FUSED2, FUSED3, REC, WIDE, SMALL, EXACT32)
SHAPES = {'narrow': (45, 20), 'past20': (13108, 20), 'past64': (4097, 64), 'h256': (30, 256), 'h33': (12, 33)}
MODES = ('plain', 'combine0', 'combine5', 'aux', 'error', 'rk4_0', 'rk4_3')
SWITCHES = [(m, d) for m in (0, 1, 2) for d in (0, 1)]



def every(p0, pd):
    return ((p0, pd),) * len(MODES)


# (shape, set_rhs_mid, set_rhs_mid_drop) -> per mode of MODES, (report of the p = 0 call, report of the masked call)
NARROW = ((0, SMALL | DROP),) + ((SMALL, SMALL | DROP),) * 6          # (the plain p = 0 call reports only the MID bit)
EXPECT = {
    ('narrow', 0, 0): NARROW, ('narrow', 0, 1): NARROW, ('narrow', 1, 0): NARROW, ('narrow', 1, 1): NARROW,
    ('narrow', 2, 0): every(MID, SMALL | DROP), ('narrow', 2, 1): every(MID, MID | DROP),
    ('past20', 0, 0): every(0, 0), ('past20', 0, 1): every(0, 0),
    ('past20', 1, 0): every(MID, 0), ('past20', 1, 1): every(MID, MID | DROP),
    ('past20', 2, 0): every(MID, 0), ('past20', 2, 1): every(MID, MID | DROP),
    ('past64', 0, 0): every(0, 0), ('past64', 0, 1): every(0, 0),
    ('past64', 1, 0): every(MID, 0), ('past64', 1, 1): every(MID, MID | DROP),
    ('past64', 2, 0): every(MID, 0), ('past64', 2, 1): every(MID, MID | DROP),
    # 12 x 33 is a shape of the narrow-panel kernel; rhs_mid.hip never takes the width
    ('h33', 0, 0): NARROW, ('h33', 0, 1): NARROW, ('h33', 1, 0): NARROW, ('h33', 1, 1): NARROW, ('h33', 2, 0): NARROW, ('h33', 2, 1): NARROW,
    # H = 256: the stage algebra in the launch for p = 0; under a mask the plain launch, which reports itself, and the passes behind it
    ('h256', 0, 0): every(FUSED2, FUSED2), ('h256', 2, 1): every(FUSED2, FUSED2),
}

# (shape, the one misaligned panel) at set_rhs_mid(2), set_rhs_mid_drop(1) -> (p = 0, masked) for combine5, aux and rk4_3 ('out_aux': aux only).
# Past the narrow-panel kernel's bound K still comes from rhs_mid.hip's plain launch, with the stage kernel behind it - except a masked
# COMBINE without y_aux, which composes all of it (ndcn_dropout_combine_f32 behind the SpMM and the Linear) and reports 0
EXPECT_MISALIGNED = {
    ('narrow', 'y0'): ((SMALL, SMALL | DROP),) * 3, ('narrow', 'out_y'): ((SMALL, SMALL | DROP),) * 3,
    ('narrow', 'out_aux'): ((SMALL, SMALL | DROP),), ('narrow', 'kprev0'): ((SMALL, SMALL | DROP),) * 3,
    ('past20', 'y0'): ((MID, 0), (MID, MID | DROP), (MID, MID | DROP)), ('past20', 'out_y'): ((MID, 0), (MID, MID | DROP), (MID, MID | DROP)),
    ('past20', 'out_aux'): ((MID, MID | DROP),), ('past20', 'kprev0'): ((MID, 0), (MID, MID | DROP), (MID, MID | DROP)),
    ('past64', 'y0'): ((MID, 0), (MID, MID | DROP), (MID, MID | DROP)), ('past64', 'out_y'): ((MID, 0), (MID, MID | DROP), (MID, MID | DROP)),
    ('past64', 'out_aux'): ((MID, MID | DROP),), ('past64', 'kprev0'): ((MID, 0), (MID, MID | DROP), (MID, MID | DROP)),
    ('past64', 'out_K'): ((0, 0),) * 3, ('past64', 'X'): ((0, 0),) * 3,
}

# (shape, no_control) at the default switches and at (2, 1) -> (p = 0, masked) for plain, combine5, error and rk4_3
EXPECT_FLAGS = {
    'narrow': ((0, 0),) * 8,
    'h256': ((0, 0), (WIDE, 0), (WIDE, 0), (WIDE, 0)) * 2,
}


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


def clear_path(dev):
    """relu(A X) with a stage sum on two nodes composes (no epilogue route at H = 4) and reports 0"""
    from ndcn_amd import CsrOperator, hip
    A = CsrOperator.from_arrays([0, 1, 2], [0, 1], [1.0, 1.0], (2, 2), dev)
    X = torch.ones(2, 4, device=dev)
    hip.rhs_rk(A, X, None, None, 'combine', X, [], [0.5], no_control=True)
    assert rhs_path() == 0


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
        raise AssertionError('%s: %d of %d words differ; first at %s: got %r want %r' % (what, bad.shape[0], got.numel(), i, float(got[i]),
                                                                                       float(want[i])))


def same_record(got, want, what, own, n_terms):
    """own: the launch's epilogue summed the record itself, in fp64 - against ndcn_rk_error_f32's float32 sum of the same n_terms
    non-negative squares the sum agrees to the worst case of a sequential float32 sum, (n_terms + 8) 2^-24 relative (8: the roundings
    inside one term); the count of non-finite rows is exact either way"""
    g, w = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if not own:
        assert np.array_equal(g.view(np.uint64), w.view(np.uint64)), (what, got, want)
        return
    print('%s: record %r against %r, relative %.2e' % (what, got, want, abs(g[0] - w[0]) / w[0]), flush=True)
    assert g[1] == w[1] and abs(g[0] - w[0]) <= (n_terms + 8) * 2.0 ** -24 * w[0], (what, got, want)


def rows_scaled(n, H, gen, dev, k=8):
    x = torch.randn(n, H, generator=gen, device=dev)
    return x * torch.exp2(torch.randint(-k, k + 1, (n, 1), generator=gen, device=dev).float())


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
    return m


def shifted(t):
    """a copy of t in a view that starts one float behind a 16-byte boundary"""
    buf = torch.zeros(t.numel() + 4, device=t.device)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


class Case:
    def __init__(self, shape, dev):
        from ndcn_amd import CsrOperator
        n, H = SHAPES[shape]
        nc = max(n, 256)
        self.shape, self.n, self.H, self.dev = shape, n, H, dev
        m = matrix(n, nc, 1 + n % 7)
        self.A = CsrOperator.from_arrays(m.indptr, m.indices, m.data, m.shape, dev)
        self.A._plans_tried = True
        g = torch.Generator(device=dev).manual_seed(n)
        self.X = torch.rand(nc, H, generator=g, device=dev) - 0.3
        self.y0 = rows_scaled(n, H, g, dev)
        self.ks = [rows_scaled(n, H, g, dev) for _ in range(5)]
        self.W = (torch.rand(H, H, generator=g, device=dev) - 0.5) / 8
        self.b = (torch.rand(H, generator=g, device=dev) - 0.5) / 8
        self.ev = 0
        self._K = {}

    def base_K(self, no_control):
        """the unmasked K of the composed form, formed once per flag set (the callers clone it)"""
        from ndcn_amd import hip
        if no_control not in self._K:
            with switches(0, 0):
                if self.H == 256 or no_control:
                    self._K[no_control] = hip.rhs(self.A, self.X, self.W, self.b, no_control=no_control)
                else:
                    self._K[no_control] = hip.linear(hip.spmm(self.A, self.X), self.W, self.b, relu=True)
        return self._K[no_control]

    def stage_args(self, mode):
        """(mode of hip.rhs_rk, earlier stages, coefficients, aux coefficients)"""
        if mode == 'plain':
            return 'plain', [], [], None
        if mode in ('combine0', 'combine5'):
            npv = int(mode[-1])
            return 'combine', self.ks[:npv], CS[:npv] + [CS[5]], None
        if mode == 'aux':
            return 'combine', self.ks[:4], CS[:4] + [CS[5]], AUX[:4] + [AUX[5]]
        if mode == 'error':
            return 'error', self.ks, CS, None
        return 'rk4', self.ks[:int(mode[-1])], [DT], None

    def composed(self, rk, y0, ks, cs, aux, drop, no_control):
        from ndcn_amd import hip
        K = self.base_K(no_control).clone()
        if drop is not None:
            hip.dropout_apply(K, drop)
        if rk == 'plain':
            return [K]
        if rk == 'combine':
            return [K, hip.combine(y0, ks + [K], cs)] + ([hip.lincomb(ks + [K], aux)] if aux is not None else [])
        if rk == 'rk4':
            kk = ks + [K]
            return [K, hip.fixed_stage(2 + len(ks), y0, kk[0], *kk[1:], dt=float(cs[0]))]
        return [K, hip.error(y0, self.X[:self.n].contiguous(), ks + [K], cs, RTOL, ATOL)]

    def cell(self, mode, what, misaligned=None, no_control=False):
        """both calls of one cell under the switches in force: (report of the p = 0 call, report of the masked call)"""
        from ndcn_amd import hip
        rk, ks, cs, aux = self.stage_args(mode)
        y0, X, kw = self.y0, self.X, {}
        if misaligned == 'y0':
            y0 = shifted(y0)
        elif misaligned == 'kprev0':
            ks = [shifted(ks[0])] + ks[1:]
        elif misaligned == 'X':
            X = shifted(X)
        reports = []
        for masked in (False, True):
            self.ev += 1
            drop = (0.5, SEED, self.ev) if masked else None
            if misaligned in ('out_y', 'out_aux', 'out_K'):
                kw = {misaligned: shifted(torch.zeros(self.n, self.H, device=self.dev))}
            clear_path(self.dev)
            if rk == 'plain':
                got = [hip.rhs(self.A, X, self.W, self.b, no_control=no_control, dropout=drop, out=kw.get('out_K'))]
            else:
                got = hip.rhs_rk(self.A, X, self.W, self.b, rk, y0, ks, cs, rtol=RTOL, atol=ATOL, aux_cs=aux, no_control=no_control,
                                 dropout=drop, **kw)
            torch.cuda.synchronize()
            reports.append(rhs_path())
            want = self.composed(rk, self.y0, self.stage_args(mode)[1], cs, aux, drop, no_control)
            assert len(got) == len(want)
            for i, (a, b) in enumerate(zip(got, want)):
                label = '%s %s %s: output %d' % (what, mode, 'masked' if masked else 'p = 0', i)
                if rk == 'error' and i == 1:
                    same_record(a, b, label, bool(reports[-1] & OWN_RECORD), self.n * self.H)
                else:
                    same(a, b, label)
        return tuple(reports)


_cases = {}


def case(shape, dev):
    if shape not in _cases:
        _cases[shape] = Case(shape, dev)
    return _cases[shape]


def paired(mode, p0, pd, drop_switch, what):
    """what the p = 0 and the masked dispatch promise each other"""
    if pd & MID:
        assert p0 & MID, '%s: the masked call reports MID, the p = 0 call %#x' % (what, p0)
    if pd & SMALL:
        ok = p0 == 0 if mode == 'plain' else bool(p0 & SMALL)
        assert ok or (p0 & MID and not drop_switch), '%s: the masked call reports SMALL, the p = 0 call %#x' % (what, p0)


def observe_switches(shape, mid, drop, dev):
    c = case(shape, dev)
    out = []
    with switches(mid, drop):
        for mode in MODES:
            what = '%s mid=%d drop=%d' % (shape, mid, drop)
            r = c.cell(mode, what)
            paired(mode, r[0], r[1], drop, '%s %s' % (what, mode))
            out.append(r)
    return tuple(out)


def observe_misaligned(shape, which, dev):
    c = case(shape, dev)
    out = []
    with switches(2, 1):
        for mode in (('aux',) if which == 'out_aux' else ('combine5', 'aux', 'rk4_3')):
            what = '%s misaligned %s' % (shape, which)
            r = c.cell(mode, what, misaligned=which)
            paired(mode, r[0], r[1], 1, '%s %s' % (what, mode))
            out.append(r)
    return tuple(out)


def observe_flags(shape, dev):
    c = case(shape, dev)
    out = []
    for mid, drop in ((0, 0), (2, 1)):
        with switches(mid, drop):
            for mode in ('plain', 'combine5', 'error', 'rk4_3'):
                what = '%s no_control mid=%d drop=%d' % (shape, mid, drop)
                r = c.cell(mode, what, no_control=True)
                paired(mode, r[0], r[1], drop, '%s %s' % (what, mode))
                out.append(r)
    return tuple(out)


SWITCH_CELLS = [(s, m, d) for s in ('narrow', 'past20', 'past64', 'h33') for m, d in SWITCHES] + [('h256', 0, 0), ('h256', 2, 1)]
MISALIGNED_CELLS = [(s, w) for s in ('narrow', 'past20', 'past64') for w in ('y0', 'out_y', 'out_aux', 'kprev0')] + [('past64', 'out_K'),
                                                                                                                    ('past64', 'X')]


@pytest.mark.parametrize('shape,mid,drop', SWITCH_CELLS)
def test_every_mode_under_the_switches(dev, shape, mid, drop):
    got = observe_switches(shape, mid, drop, dev)
    print(shape, mid, drop, got, flush=True)
    assert got == EXPECT[(shape, mid, drop)]


@pytest.mark.parametrize('shape,which', MISALIGNED_CELLS)
def test_one_misaligned_panel(dev, shape, which):
    """ndcn_set_rhs_mid(2), ndcn_set_rhs_mid_drop(1): a misaligned stage panel hands the launch to the narrow-panel kernel where that takes the
    shape; a misaligned X or K keeps rhs_mid.hip out altogether"""
    got = observe_misaligned(shape, which, dev)
    print(shape, which, got, flush=True)
    assert got == EXPECT_MISALIGNED[(shape, which)]


@pytest.mark.parametrize('shape', ('narrow', 'h256'))
def test_no_control(dev, shape):
    """relu(A X): no route of the two switches, and under a mask no route with an epilogue at all"""
    got = observe_flags(shape, dev)
    print(shape, got, flush=True)
    assert got == EXPECT_FLAGS[shape]
    assert all(pd == 0 for _, pd in got)


def test_argument_errors_under_a_mask(dev):
    """NDCN_EINVAL before anything is launched: a halo panel, no NDCN_F_RELU, more than five earlier stages (that one for p = 0 too)"""
    from ndcn_amd import hip
    L = _L()
    c = case('narrow', dev)
    drop = (0.5, SEED, 3)
    n_own = c.X.shape[0] - 40
    X, Xh = c.X[:n_own].contiguous(), c.X[n_own:].contiguous()
    calls = {
        'halo plain': (lambda: hip.rhs(c.A, X, c.W, c.b, X_halo=Xh, dropout=drop), 'halo'),
        'halo combine': (lambda: hip.rhs_rk(c.A, X, c.W, c.b, 'combine', c.y0, c.ks[:2], CS[:2] + [CS[5]], X_halo=Xh, dropout=drop), 'halo'),
        'relu plain': (lambda: hip.rhs(c.A, c.X, c.W, c.b, relu=False, dropout=drop), 'NDCN_F_RELU'),
        'relu rk4': (lambda: hip.rhs_rk(c.A, c.X, c.W, c.b, 'rk4', c.y0, c.ks[:1], [DT], relu=False, dropout=drop), 'NDCN_F_RELU'),
        'n_prev masked': (lambda: hip.rhs_rk(c.A, c.X, c.W, c.b, 'combine', c.y0, c.ks + [c.ks[0]], CS + [CS[0]], dropout=drop), 'n_prev'),
        'n_prev p = 0': (lambda: hip.rhs_rk(c.A, c.X, c.W, c.b, 'combine', c.y0, c.ks + [c.ks[0]], CS + [CS[0]]), 'n_prev'),
    }
    for mid, on in ((0, 0), (2, 1)):
        with switches(mid, on):
            for name, (call, word) in calls.items():
                with pytest.raises(L.NdcnHipError) as e:
                    call()
                assert e.value.code == L.EINVAL and word in str(e.value), (name, mid, on, str(e.value))
