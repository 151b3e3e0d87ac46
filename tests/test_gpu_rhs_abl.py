"""The one-launch right-hand side of the two ablations (csrc/rhs_abl.hip, NDCN_PATH_ABL, ndcn_set_rhs_abl) - no_control K = relu(A X),
no_graph K = relu(X W^T + b), hidden widths 16..128 at any number of rows - against a HOST oracle and against the composed path of
csrc/rhs.hip (the same call with the switch off: SpMM or MFMA Linear, mask pass, stand-alone stage kernel), bit for bit.

Oracles (no expected value comes from a device kernel or a torch reduction)
  K, no_control   relu_nan of tests/_fma_chain.py chain: one fma per stored entry in stored order from +0
  K, no_graph     relu_nan(fma chain over k ascending from +0, then + b)
  y_next, y_aux, RK4 outputs   tests/_rk_epilogue.py in its from_zero form applied to the K the DEVICE returned
  error record    the rules of tests/test_gpu_rhs_rk_routes.py for the stand-alone kernel: the non-finite count exactly; the sum bit-equal
                  to the ATen-order cascade up to 2^18 elements, inside the any-tree fp64 bound above; NaN / +Inf where a term is
  dropout         K' = K * m with m of tests/_philox.py, one fp32 product
Any NaN matches any NaN against the host; against the switch-off call the raw words are compared.

Shapes.  The tile is 64 rows: n in {1, 63, 64, 65, 130}; 4161 rows are 66 tiles - the no_graph launch at P = 128 holds one workgroup per
compute unit, and on a device with fewer than 66 of them some workgroups run two tiles; the last tile is one row.  H in {16, 20, 36, 64,
96, 100, 128}: P = ceil32(H) = 32 / 64 / 96 / 128 (8, 16, 32 and 32 lanes per gathered row), H no multiple of 32 in four of them.
Operators of no_control: the first n rows of the eight-neighbour lattice of side ceil(sqrt(n)) (8 x 8 .. 65 x 65), and a random CSR whose
rows cycle through 0..9 entries (empty rows, the gather's rounds of four and each of its tails) with one row of 200.  The oracle of the
4161-row cases reads the first and last 65 rows and 64 seeded ones; the switch-off comparison reads every row.

Inputs (the recipe of tests/test_gpu_rhs_rk_routes.py): X = rand - 0.3, y0 and the stages randn rows scaled by 2^j, W and b uniform in
+-1/16, coefficients (0.11, 0, 0.23, 0.05, -0.31 | -0.19) - a zero, negative ones, the new stage's negative - and the special set
{+-0, +-1e-40, 1e-20, -1.5e-19, +-3e38, +-Inf, NaN} planted in y0 and in every earlier stage; for no_graph X carries NaN, +-Inf and -0 in
a few rows too (no_control keeps X finite: one NaN would spread over its neighbours' rows all the same, and does in the oracle)."""
import contextlib
import math

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import _philox
import _rk_epilogue as E
import test_gpu_rhs_rk_routes as R
from _fma_chain import chain

pytestmark = pytest.mark.gpu
F = np.float32
CS, AUX, TOLS = R.CS, R.AUX, R.TOLS
DT = F(0.37)
WIDTHS = (16, 20, 36, 64, 96, 100, 128)
SIZES = (1, 63, 64, 65, 130)
MANY = 4161
FORMS = ('no_control', 'no_graph')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    from ndcn_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


def _L():
    from ndcn_amd import _lib
    return _lib


@contextlib.contextmanager
def abl(on):
    from ndcn_amd import hip
    prev = hip.set_rhs_abl(on)
    try:
        yield
    finally:
        hip.set_rhs_abl(prev)


def bits(t):
    return t.contiguous().view(torch.int32)


def same_words(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not torch.equal(bits(got), bits(want)):
        bad = (bits(got) != bits(want)).nonzero()
        i = tuple(int(v) for v in bad[0])
        raise AssertionError('%s: %d of %d words differ from the switch-off call; first at %s: got %r want %r' % (
            what, bad.shape[0], got.numel(), i, float(got[i]), float(want[i])))


def lattice_rows(n):
    side = max(2, int(math.ceil(math.sqrt(n))))
    return sp.csr_matrix(R.lattice(side)[:n])


def ragged_rows(n, seed):
    """rows of r % 10 entries - 0: empty, 1..3 and 5..7: the tails, 4, 8, 9: the rounds of four - and one row of 200"""
    deg = np.arange(n) % 10
    deg[n // 2] = 200
    return R.rand_rows(n, max(n, 256), seed=seed, lengths=deg)


class Case:
    def __init__(self, form, m, n, H, dev, seed, rows=None):
        self.form, self.m, self.n, self.H, self.dev = form, m, n, H, dev
        self.kw = {form: True}
        self.name = '%s n=%d H=%d' % (form, n, H)
        g = torch.Generator(device=dev).manual_seed(seed)
        nc = n if m is None else m.shape[1]
        self.A = None if m is None else R.op(m, dev)
        self.X = torch.rand(nc, H, generator=g, device=dev) - 0.3
        if m is None and n >= 3:                               # no_graph: non-finite inputs and -0 in three rows
            for r, c, v in ((0, 1, float('nan')), (n // 2, H - 1, float('inf')), (n // 2, 0, -0.0), (n - 1, 5, -float('inf')), (n - 1, 7, -0.0)):
                self.X[r, c] = v
        self.y0 = R.plant(R.rows_scaled(n, H, g, dev), 1)
        self.y0_plain = R.rows_scaled(n, H, g, dev)
        self.ks = [R.plant(R.rows_scaled(n, H, g, dev), 2 + j) for j in range(5)]
        self.ks_plain = [R.rows_scaled(n, H, g, dev) for _ in range(5)]
        self.W = self.b = None
        if m is None:
            self.W = (torch.rand(H, H, generator=g, device=dev) - 0.5) / 8
            self.b = (torch.rand(H, generator=g, device=dev) - 0.5) / 8
        self.rows = None if rows is None else np.asarray(rows, np.int64)
        self.rows_t = None if rows is None else torch.as_tensor(self.rows, device=dev)

    def h(self, t):
        return (t if self.rows_t is None else t[self.rows_t]).cpu().numpy()

    def oracle_K(self, relu=True):
        X = self.X.cpu().numpy()
        if self.m is not None:
            return chain(self.m.indptr, self.m.indices, self.m.data, X, relu=relu, rows=self.rows)
        assert relu
        return R.linear_chain(X if self.rows is None else X[self.rows], self.W.cpu().numpy(), self.b.cpu().numpy())

    def launch(self, mode, y0=None, ks=(), cs=(), **kw):
        from ndcn_amd import hip
        kw = dict(self.kw, **kw)
        if mode == 'plain':
            out = (hip.rhs(self.A, self.X, self.W, self.b, **kw),)
        else:
            out = hip.rhs_rk(self.A, self.X, self.W, self.b, mode, y0, list(ks), list(cs), **kw)
        torch.cuda.synchronize()
        return out, R.rhs_path(), R.rk_path()

    def both(self, mode, what, want=None, **args):
        """the call with the switch off and on: the raw words agree, the route bit is there with the switch on alone; returns the
        switched-on outputs"""
        L = _L()
        want = L.PATH_ABL if want is None else want
        with abl(0):
            off, p_off, _ = self.launch(mode, **args)
        with abl(1):
            on, p_on, rk = self.launch(mode, **args)
        label = '%s %s %s' % (self.name, mode, what)
        assert p_off & L.PATH_ABL == 0, '%s: switch off, path %#x' % (label, p_off)
        # (a declined plain p = 0 call owns the ABL bit alone: the others are the thread's last epilogue launch's, rhs.hip)
        seen = p_on & (L.PATH_ABL | L.PATH_DROP_EPI) if want else p_on & L.PATH_ABL
        assert seen == want, '%s: switch on, path %#x, want %#x' % (label, p_on, want)
        assert len(on) == len(off)
        for i, (a, b) in enumerate(zip(on, off)):
            if mode == 'error' and i == 1:
                assert np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64)), (label, a, b)
            else:
                same_words(a, b, '%s: %s' % (label, ('K', 'y_next', 'y_aux')[i]))
        if mode == 'error' and want:                           # the record is the stand-alone kernel's behind the plain launch
            assert rk & L.RKF_KERNEL_MASK == L.RKF_ERROR, hex(rk)
        return on

    def record(self, rec, y0, ks, cs, rtol, atol, what):
        zz, bad = E.error_terms(y0.cpu().numpy(), self.X[:self.n].cpu().numpy(), [k.cpu().numpy() for k in ks] + [self.K.cpu().numpy()],
                                cs, rtol, atol, from_zero=True)
        assert rec[1] == float(bad), '%s %s: non-finite count %r, want %d' % (self.name, what, rec[1], bad)
        if zz.size <= (1 << 18):
            R.check_sum_aten(rec[0], zz, '%s %s' % (self.name, what))
        else:
            R.check_sum(rec[0], zz, '%s %s' % (self.name, what))

    def all_modes(self):
        self.K, = self.both('plain', '')
        Kh = self.h(self.K)
        R.same_bits(Kh, self.oracle_K(), self.name + ': K against the host chain')
        y0, ks = self.y0, self.ks
        for npv in range(6):
            cs, c2 = CS[:npv] + [CS[5]], AUX[:npv] + [AUX[5]]
            kk = [self.h(k) for k in ks[:npv]] + [Kh]
            for aux in (False, True):
                what = 'np=%d aux=%s' % (npv, aux)
                out = self.both('combine', what, y0=y0, ks=ks[:npv], cs=cs, aux_cs=c2 if aux else None)
                same_words(out[0], self.K, '%s combine %s: K against the plain launch' % (self.name, what))
                R.same_bits(self.h(out[1]), E.combine(self.h(y0), kk, cs, True), '%s combine %s: y_next' % (self.name, what))
                if aux:
                    R.same_bits(self.h(out[2]), E.aux(kk, c2, True), '%s combine %s: y_aux' % (self.name, what))
        for st in range(4):
            K, yn = self.both('rk4', 'stage %d' % st, y0=y0, ks=ks[:st], cs=[DT])
            same_words(K, self.K, '%s rk4 stage %d: K against the plain launch' % (self.name, st))
            R.same_bits(self.h(yn), E.rk4_stage(st, self.h(y0), [self.h(k) for k in ks[:st]] + [Kh], DT), '%s rk4 stage %d' % (self.name, st))
        for npv in (1, 5):
            cs = CS[:npv] + [CS[5]]
            for label, yy, kk, (rtol, atol) in (('plain inputs', self.y0_plain, self.ks_plain, TOLS[0]), ('specials', y0, ks, TOLS[0]),
                                                ('plain inputs, atol 0', self.y0_plain, self.ks_plain, TOLS[1])):
                what = 'np=%d %s' % (npv, label)
                K, rec = self.both('error', what, y0=yy, ks=kk[:npv], cs=cs, rtol=rtol, atol=atol)
                same_words(K, self.K, '%s error %s: K against the plain launch' % (self.name, what))
                self.record(rec, yy, kk[:npv], cs, rtol, atol, 'error ' + what)


def make(form, n, H, dev, operator='lattice', seed=None, rows=None):
    seed = n + H if seed is None else seed
    if form == 'no_graph':
        return Case(form, None, n, H, dev, seed, rows)
    return Case(form, lattice_rows(n) if operator == 'lattice' else ragged_rows(n, seed), n, H, dev, seed, rows)


def some_rows(n):
    return np.unique(np.r_[np.arange(65), np.arange(n - 65, n), np.random.RandomState(n).randint(0, n, 64)])


# --------------------------------------------------------------------------------------------------------------------- every mode
@pytest.mark.parametrize('H', WIDTHS)
def test_no_control_on_lattices(dev, H):
    for n in SIZES:
        make('no_control', n, H, dev).all_modes()


@pytest.mark.parametrize('H', WIDTHS)
def test_no_control_on_ragged_rows(dev, H):
    for n in SIZES:
        c = make('no_control', n, H, dev, operator='ragged')
        assert int(np.diff(c.m.indptr).max()) == min(200, c.m.shape[1]) and (n < 10 or int(np.diff(c.m.indptr).min()) == 0)
        c.all_modes()


@pytest.mark.parametrize('H', WIDTHS)
def test_no_graph(dev, H):
    for n in SIZES:
        make('no_graph', n, H, dev).all_modes()


@pytest.mark.parametrize('H', WIDTHS)
@pytest.mark.parametrize('form', FORMS)
def test_more_tiles_than_one_per_workgroup(dev, form, H):
    """4161 rows = 66 tiles, the last of one row"""
    assert (MANY + 63) // 64 == 66 and MANY % 64 == 1
    make(form, MANY, H, dev, operator='ragged' if H in (20, 128) else 'lattice', rows=some_rows(MANY)).all_modes()


def test_without_the_relu(dev):
    """NDCN_F_RELU clear: K = S, negative sums and -0 kept (no_control; the oracle is the bare chain)"""
    c = make('no_control', 130, 36, dev, operator='ragged')
    K, = c.both('plain', 'no relu', relu=False)
    Kh = c.oracle_K(relu=False)
    assert (Kh < 0).any()
    R.same_bits(K.cpu().numpy(), Kh, 'K = S')
    out = c.both('combine', 'no relu np=2', y0=c.y0, ks=c.ks[:2], cs=CS[:2] + [CS[5]], relu=False)
    same_words(out[0], K, 'K of the COMBINE launch')
    R.same_bits(out[1].cpu().numpy(), E.combine(c.y0.cpu().numpy(), [k.cpu().numpy() for k in c.ks[:2]] + [Kh], CS[:2] + [CS[5]], True), 'y_next')


# --------------------------------------------------------------------------------------------------------------------- dropout
DROPS = ((0.5, 1234567, 3), (0.3, (1 << 40) + 17, (1 << 33) + 5))


@pytest.mark.parametrize('n,H', [(65, 20), (130, 100), (MANY, 16), (MANY, 128)])
@pytest.mark.parametrize('form', FORMS)
def test_dropout(dev, form, n, H):
    """the factor rides in the launch (NDCN_PATH_ABL | NDCN_PATH_DROP_EPI): K' = K * m with the host mask; y_next / y_aux by the
    host epilogue on the K' the device returned; everything bit-equal to the composed calls (mask pass or dropout_combine_f32)"""
    L = _L()
    epi = L.PATH_ABL | L.PATH_DROP_EPI
    c = make(form, n, H, dev, operator='ragged')
    K0, = c.both('plain', 'p=0')
    for p, seed, ev in DROPS:
        d = (p, seed, ev)
        Kd, = c.both('plain', 'p=%g' % p, want=epi, dropout=d)
        m = _philox.mask(p, seed, ev, n, H)
        assert 0.8 * (1 - p) < float((m != 0).mean()) < 1.2 * (1 - p) or n * H < 4096
        with np.errstate(all='ignore'):
            R.same_bits(Kd.cpu().numpy(), K0.cpu().numpy() * m, '%s p=%g: K against K * mask' % (c.name, p))
        Kh = Kd.cpu().numpy()
        for npv, aux in ((0, False), (5, False), (5, True), (2, True)):
            cs, c2 = CS[:npv] + [CS[5]], AUX[:npv] + [AUX[5]]
            out = c.both('combine', 'p=%g np=%d aux=%s' % (p, npv, aux), want=epi, y0=c.y0, ks=c.ks[:npv], cs=cs, aux_cs=c2 if aux else None,
                         dropout=d)
            same_words(out[0], Kd, '%s p=%g combine %d: K against the plain dropout launch' % (c.name, p, npv))
            kk = [k.cpu().numpy() for k in c.ks[:npv]] + [Kh]
            R.same_bits(out[1].cpu().numpy(), E.combine(c.y0.cpu().numpy(), kk, cs, True), '%s p=%g combine %d: y_next' % (c.name, p, npv))
            if aux:
                R.same_bits(out[2].cpu().numpy(), E.aux(kk, c2, True), '%s p=%g combine %d: y_aux' % (c.name, p, npv))
        for st in (0, 3):
            K, yn = c.both('rk4', 'p=%g stage %d' % (p, st), want=epi, y0=c.y0, ks=c.ks[:st], cs=[DT], dropout=d)
            same_words(K, Kd, '%s p=%g rk4 %d: K' % (c.name, p, st))
            R.same_bits(yn.cpu().numpy(), E.rk4_stage(st, c.y0.cpu().numpy(), [k.cpu().numpy() for k in c.ks[:st]] + [Kh], DT),
                        '%s p=%g rk4 stage %d' % (c.name, p, st))
        c.K = Kd
        K, rec = c.both('error', 'p=%g np=5' % p, want=epi, y0=c.y0_plain, ks=c.ks_plain, cs=CS, rtol=TOLS[0][0], atol=TOLS[0][1], dropout=d)
        same_words(K, Kd, '%s p=%g error: K' % (c.name, p))
        c.record(rec, c.y0_plain, c.ks_plain, CS, TOLS[0][0], TOLS[0][1], 'p=%g error 5' % p)


# --------------------------------------------------------------------------------------------------------------------- declines
def declined(c, **kw):
    """plain, COMBINE 2 with y_aux, RK4 1 and ERROR 1 with the switch on: no NDCN_PATH_ABL, the switch-off words"""
    c.both('plain', 'declined', want=0, **kw)
    c.both('combine', 'declined', want=0, y0=c.y0, ks=c.ks[:2], cs=CS[:2] + [CS[5]], aux_cs=AUX[:2] + [AUX[5]], **kw)
    c.both('rk4', 'declined', want=0, y0=c.y0, ks=c.ks[:1], cs=[DT], **kw)
    c.both('error', 'declined', want=0, y0=c.y0_plain, ks=c.ks_plain[:1], cs=[CS[0], CS[5]], rtol=TOLS[0][0], atol=TOLS[0][1], **kw)


@pytest.mark.parametrize('H', [18, 12, 132, 256])
@pytest.mark.parametrize('form', FORMS)
def test_declined_widths(dev, form, H):
    declined(make(form, 130, H, dev))


def test_declined_halo_panel(dev):
    c = make('no_control', 130, 64, dev, operator='ragged')
    n_own = c.X.shape[0] - 40
    Xall = c.X
    c.X = Xall[:n_own].contiguous()
    declined(c, X_halo=Xall[n_own:].contiguous())
    c.X = Xall                                                 # the same operator without the halo panel does take the route
    c.both('plain', 'no halo')


@pytest.mark.parametrize('form', FORMS)
def test_declined_misaligned_input(dev, form):
    """X offset by one float"""
    c = make(form, 130, 64, dev)
    buf = torch.empty(c.X.numel() + 4, device=dev)
    Xo = buf[1:1 + c.X.numel()].view_as(c.X)
    Xo.copy_(c.X)
    assert Xo.data_ptr() % 16 == 4 and Xo.is_contiguous()
    aligned = c.X
    with abl(1):
        want = c.launch('plain')[0][0]
    c.X = Xo
    declined(c)
    with abl(1):
        same_words(c.launch('plain')[0][0], want, 'misaligned X against the aligned launch')
    c.X = aligned
    c.both('plain', 'aligned again')


@pytest.mark.parametrize('form', FORMS)
def test_misaligned_stage_panel_takes_the_plain_launch_and_the_stage_kernel(dev, form):
    """y0, or one earlier stage, offset by one float: NDCN_PATH_ABL still (the K launch), the stage algebra by the stand-alone kernel -
    the same bits; under dropout COMBINE without y_aux goes to dropout_combine_f32 behind the composed launch instead (no ABL bit)"""
    L = _L()
    c = make(form, 130, 20, dev, operator='ragged')
    c.K, = c.both('plain', '')
    Kh = c.K.cpu().numpy()

    def shifted(t):
        buf = torch.empty(t.numel() + 4, device=dev)
        v = buf[1:1 + t.numel()].view_as(t)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4
        return v
    cs, c2 = CS[:2] + [CS[5]], AUX[:2] + [AUX[5]]
    for what, y0, ks in (('y0', shifted(c.y0), c.ks[:2]), ('stage 1', c.y0, [c.ks[0], shifted(c.ks[1])])):
        kk = [k.cpu().numpy() for k in ks] + [Kh]
        out = c.both('combine', 'misaligned ' + what, y0=y0, ks=ks, cs=cs, aux_cs=c2)
        assert R.rk_path() & L.RKF_KERNEL_MASK == L.RKF_COMBINE, hex(R.rk_path())
        same_words(out[0], c.K, 'K')
        R.same_bits(out[1].cpu().numpy(), E.combine(y0.cpu().numpy(), kk, cs, True), 'misaligned %s: y_next' % what)
        R.same_bits(out[2].cpu().numpy(), E.aux(kk, c2, True), 'misaligned %s: y_aux' % what)
        K, yn = c.both('rk4', 'misaligned ' + what, y0=y0, ks=ks, cs=[DT])
        R.same_bits(yn.cpu().numpy(), E.rk4_stage(2, y0.cpu().numpy(), kk, DT), 'misaligned %s: rk4 stage 2' % what)
        d = (0.5, 99, 1)
        c.both('combine', 'dropout, misaligned %s, no y_aux' % what, want=0, y0=y0, ks=ks, cs=cs, dropout=d)
        c.both('combine', 'dropout, misaligned %s, y_aux' % what, want=L.PATH_ABL | L.PATH_DROP_EPI, y0=y0, ks=ks, cs=cs, aux_cs=c2, dropout=d)


def test_switch(dev):
    from ndcn_amd import hip
    first = hip.set_rhs_abl(1)
    try:
        assert first == 0
        assert hip.set_rhs_abl(0) == 1 and hip.set_rhs_abl(1) == 0
        assert hip.set_rhs_abl(-1) == 1 and hip.set_rhs_abl(first) == 0
    finally:
        hip.set_rhs_abl(first)
    c = make('no_graph', 65, 16, dev)
    c.both('plain', 'after the switch test')
