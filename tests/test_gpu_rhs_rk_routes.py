"""Every with-control launch of ndcn_rhs_rk_f32 - K = relu(W (A X) + b) plus the Runge-Kutta algebra in the epilogue - against a HOST
oracle: rhs_fused3.hip, rhs_fused2.hip and its fp32 build rhs_fused2_exact.hip, the first-generation rhs_fused.hip, rhs_small.hip and
the composed fallback of rhs.hip.  No expected value below comes from a device kernel or from a torch reduction; every case asserts
its route through ndcn_debug_last_rhs_path (exact value) and, where the stage algebra runs stand-alone, ndcn_debug_last_rk_path.

Oracles
  S = A X        tests/_fma_chain.py chain / chain_hub (bit for bit where the launch writes it: s_out)
  K, split       |K - relu64(S32 W^T + b)| <= 2e-6 (sum_k |S32_k W_ok| + |b_o|) per element, S32 = the chain: the GUARANTEE of
                 csrc/split16.h (FUSED3, FUSED2, the sweep's dense stage).  Worst observed ratio to that bound on an MI355X:
                 FUSED3 0.091, FUSED2 0.106, SWEEP 0.102, x_add / x_mask / s_out launches 0.117 (printed by every case)
  K, EXACT32     (256 + 2) 2^-24 (sum |S32 w| + |b|): the fp32 MFMA bound of tests/test_gpu_linear_routes.py; worst observed 0.019 of
                 it; the first-generation kernel (fp32 MFMA too): 0.015
  K, SMALL and the narrow composed path: bit for bit relu_nan(fma chain over h from +0, then + b) of the chain's S
  y_next, y_aux, RK4 outputs: bit for bit tests/_rk_epilogue.py applied to the K the DEVICE returned (+0 / -0 told apart, NaNs at
                 the same positions); the K of a COMBINE / ERROR / RK4 launch is bit-equal to the plain launch's
  error record   d_out[1] = the count of non-finite y1 exactly; d_out[0] against the sum of _rk_epilogue.error_terms:
                 fp64 reduction inside a launch (and the stand-alone parallel kernel): |got - ref| <= 1.01 n 2^-53 ref, the bound of
                 ANY summation tree over n non-negative terms (+ the reference's own rounding); the stand-alone ATen-order kernel
                 (panels <= 2^18 elements): bit-equal to tests/_aten_order.py cascade_sum.  A NaN term makes the sum NaN, a +Inf
                 term +Inf; +-Inf in y1 leaves z = 0 there (tol = +Inf).
The composed fallback's stage sum starts from +0 (rk.hip wsum1) where the fused epilogues start from the new stage's product: the
two differ in the sign of an all-zero sum only (-0 products: a ReLU-cut K times a negative coefficient), so y_next = -0 + -0 = -0
in the fused launches and +0 in the composed ones; _rk_epilogue's from_zero states the second form.  No composed COMBINE / RK4 exists
at H = 256; the narrow one (n H > 2^18) is held to from_zero.

Inputs: X = rand - 0.3 (the ReLU cuts); y0 and the stages randn rows scaled by 2^j, j in [-8, 8]; W uniform in +-1/16; coefficients
(0.11, 0, 0.23, 0.05, -0.31 | -0.19): one zero, negative ones (the new stage's included: -0 products).  The special set {+0, -0, +-1e-40,
1e-20, -1.5e-19, +-3e38, +-Inf, NaN} is planted into y0, into every earlier stage in turn and into an explicit y1, one value per
third row; X stays finite.  ERROR runs (rtol, atol) = (1e-2, 1e-3) and (1e-2, 0) - the second also with elements where y0 = y1 = 0:
tol = 0 there, the term is +Inf (sum != 0) or NaN (0 / 0), and so is the sum.

Shapes (from the kernels' constants): FUSED3 groups are 16 rows (kF3R: 4 x 4 patches on the lattice walk order), the grid min(256, 8 ceil(groups / 8)) workgroups: side 41 =
11 x 11 = 121 groups (ragged ones along two edges, fewer groups than workgroups), side 72 = 324 groups (a workgroup serves two); halo: own rows
[0, 1200); six rows with 12 far-away entries each leave their groups unstaged.  Non-temporal stores: every halo launch, every x_add
launch, and panels above 128 MiB = 131 072 rows (side 363).  FUSED2 tiles are 64 rows (kTile2), the grid min(256, 8 ceil(tiles / 8)):
n in {1, 63, 64, 65, 129}, 16449 rows = 258 tiles, rows of 0..70 entries (rounds of 16 and every 8/4/2/1 tail).  SMALL: n H <= 2^18.
The stand-alone error kernel sums in ATen order up to 2^18 elements (1024 rows at H = 256: side 32), in parallel fp64 above.

Template instantiations reachable through the C ABI and the case that reaches them
  rhs_fused3_kernel<HALO, MODE, NP, XOP, NT, SOUT, NOK>  (launch_f3 / NDCN_F3 / NDCN_F3_ADJ)
    <false, PLAIN|COMBINE 0..5|RK4 0..3|ERROR 1,5, 0, NT=false>   test_fused3[41], [72], [hot]; SWEEP: test_sweep (identity operator)
    <true,  the same 13,            0, NT=true>                   test_fused3[halo]
    <false, the same 13,            0, NT=true>                   test_fused3_beyond_128_mib (PLAIN, COMBINE 5, RK4 3, ERROR 5)
    <false, COMBINE 1, XOP=1, NT=true>                            test_xadd (also with wide-range weights: PATH_RANGE)
    <false, COMBINE 1..4 | ERROR 5, XOP=2, NT=false>              test_adjoint_halves[mask]
    <false, COMBINE 1..4 | ERROR 5, 0, NT=false, SOUT>            test_adjoint_halves[s_out]
  rhs_fused2_kernel<HALO, MODE, NP>  (NDCN_F2)   <false | true, PLAIN|COMBINE 0..5|RK4 0..3|ERROR 1,5>
                                                                  test_fused2[...], [halo], [lengths], [hub], [tiles]
  rhs_fused2_exact_kernel<HALO, MODE, NP>        the same set     test_exact32[no_plan], [halo]; a lattice operator takes the same
                                                                  kernel (the guard leaves FUSED3): test_exact32[lattice]
  rhs_small_kernel<NH 1|2, HALO, MODE>           every mode       test_small[H, n], [halo]
  composed (rhs_f32 + rk_error_f32): ERROR with 0, 2, 3, 4 earlier stages at H = 256
                                                                  test_fused3 / test_fused2 (every stage count 0..5), ATen order:
                                                                  test_composed_error_in_aten_order; narrow: test_small_threshold
  rhs_fused_kernel (first generation)            plain            test_first_generation_kernel_in_a_child_process
Reachable only from the device solver (RkOpt fields the C ABI does not carry), covered elsewhere:
  NOK (no_k) and the dense-output kernels rhs_fused3_dense_kernel (c_mid)   tests/test_gpu_dense_fused.py
  <false, ERROR, 1, XOP=1> (ERROR with x_add: the initial step's second evaluation)   tests/test_gpu_odeint.py (solver against oracle)
  c_dev (coefficients in device memory, rhs_small under hipGraph replay)    tests/test_gpu_small_solve.py
  the adjoint halves above 128 MiB (NT=true with XOP=2 / SOUT)              tests/test_gpu_kernels.py (side 400, against device kernels)
Refusals: ndcn_rhs_rk_xadd_f32 carries neither a halo panel nor a stage count, so "x_add with a halo panel / another stage count"
cannot be expressed through it (the launcher's checks serve the solver); what CAN be asked and must return NDCN_EINVAL: x_add, x_mask,
s_out without the lattice plan; x_mask and s_out together; x_mask / s_out with a mode outside COMBINE 1..4 / ERROR 5.
The mask rule (rhs_fused3.hip xadd_rows): the input is 0 where mask <= 0 and X elsewhere - X passes where mask > 0 (a subnormal
included) or the mask is NaN: torch's threshold_backward, as test_adjoint_half_mask_is_threshold_backward states."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import _aten_order as ao
import _rk_epilogue as E
from _fma_chain import chain, chain_hub, fma32

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
F = np.float32
CS = [F(c) for c in (0.11, 0.0, 0.23, 0.05, -0.31, -0.19)]          # [5]: the new stage's
AUX = [F(c) for c in (0.013, -0.02, 0.0, 0.007, -0.011, 0.017)]
SPECIALS = (0.0, -0.0, 1e-40, -1e-40, 1e-20, -1.5e-19, 3e38, -3e38, float('inf'), -float('inf'), float('nan'))
TOLS = ((F(1e-2), F(1e-3)), (F(1e-2), F(0.0)))
WORST = {}


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


def same_bits(got, want, what):
    """float32 arrays equal bit for bit, except that any NaN matches any NaN"""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = (got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want))
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError('%s: %d of %d elements differ; first at %s: got %r (0x%08x) want %r (0x%08x)' % (
            what, int(bad.sum()), bad.size, i, float(got[i]), int(got.view(np.uint32)[i]), float(want[i]), int(want.view(np.uint32)[i])))


def ref_sum(zz):
    """the sum of non-negative fp64 terms in extended precision (any-tree error n 2^-64 of the sum) or, without one, math.fsum"""
    if np.finfo(np.longdouble).nmant >= 63:
        return float(np.sum(zz.ravel(), dtype=np.longdouble))
    return math.fsum(zz.ravel().tolist())


def check_sum(got, terms, what, extra_adds=0):
    """d_out[0] of an fp64 reduction: NaN / +Inf exactly where a term is; else the any-tree bound over all terms (+ accumulating adds)"""
    zz = np.concatenate([t.ravel() for t in terms]) if isinstance(terms, (list, tuple)) else terms.ravel()
    if np.isnan(zz).any():
        assert math.isnan(got), (what, got)
        return
    if np.isinf(zz).any():
        assert got == float('inf'), (what, got)
        return
    ref, n = ref_sum(zz), zz.size + extra_adds
    bound = ((1.01 * n + 1) * 2.0 ** -53 + n * 2.0 ** -64) * ref
    assert abs(got - ref) <= bound, '%s: error sum %r, reference %r, |diff| %.3g, bound %.3g' % (what, got, ref, abs(got - ref), bound)


def check_sum_aten(got, zz, what):
    """d_out[0] of the stand-alone ATen-order kernel: the float32 cascade sum, widened"""
    want = float(ao.cascade_sum(zz.astype(np.float32)))
    assert (math.isnan(got) and math.isnan(want)) or got == want, (what, got, want)


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


def linear_chain(S, W, b):
    """relu_nan(fma chain over h from +0, then + b): rhs_small.hip and linear_f32 (test_linear_is_an_exact_fp32_fma_chain)"""
    acc = np.zeros((S.shape[0], W.shape[0]), np.float32)
    for h in range(S.shape[1]):
        acc = fma32(S[:, h:h + 1], W[:, h][None, :], acc)
    with np.errstate(all='ignore'):
        k = acc + (b[None, :] if b is not None else F(0))
        return np.where(k < 0, F(0), k).astype(np.float32)


class Case:
    """one operator + inputs; K oracle by `kind`: 'split' (2e-6 bound), 'fp32' ((256 + 2) 2^-24 bound), 'chain' (bits)"""

    def __init__(self, name, m, A, dev, want_path, kind='split', H=256, n_own=None, hub_thr=None, seed=1, W=None, b=None, rows=None,
                 relu=True, route=None):
        self.name, self.m, self.A, self.dev, self.want, self.kind, self.H = name, sp.csr_matrix(m), A, dev, want_path, kind, H
        self.hub_thr, self.relu, self.route = hub_thr, relu, route or name.split(' ')[0]
        n, nc = m.shape
        self.n = n
        g = torch.Generator(device=dev).manual_seed(seed)
        Xall = torch.rand(nc, H, generator=g, device=dev) - 0.3
        self.Xall = Xall
        self.X, self.Xh = (Xall, None) if n_own is None else (Xall[:n_own].contiguous(), Xall[n_own:].contiguous())
        self.y0 = rows_scaled(n, H, g, dev)
        self.ks = [rows_scaled(n, H, g, dev) for _ in range(5)]
        self.W = ((torch.rand(H, H, generator=g, device=dev) - 0.5) / 8) if W is None else W.to(dev)
        self.b = ((torch.rand(H, generator=g, device=dev) - 0.5) / 8) if b is None else (b.to(dev) if b is not False else None)
        self.rows = None if rows is None else np.asarray(rows, np.int64)
        self.rows_t = None if rows is None else torch.as_tensor(self.rows, device=dev)

    def h(self, t):
        """a device panel's rows under test, on the host"""
        return (t if self.rows_t is None else t[self.rows_t]).cpu().numpy()

    def S32(self, Xall=None):
        X = (self.Xall if Xall is None else Xall).cpu().numpy()
        m = self.m
        if self.hub_thr is not None:
            S = chain_hub(m.indptr, m.indices, m.data, X, self.hub_thr)
            return S if self.rows is None else S[self.rows]
        if self.rows is None:
            return chain(m.indptr, m.indices, m.data, X)
        sub = sp.csr_matrix(m[self.rows])
        cols, inv = np.unique(sub.indices, return_inverse=True)
        return chain(sub.indptr, inv, sub.data, X[cols])

    def check_K(self, K, S=None, what=''):
        S = self.S32() if S is None else S
        Kh = self.h(K)
        W = self.W.cpu().numpy()
        b = self.b.cpu().numpy() if self.b is not None else None
        if self.kind == 'chain':
            want = linear_chain(S, W, b)
            if not self.relu:
                raise NotImplementedError
            same_bits(Kh, want, '%s %s: K against the fma chains' % (self.name, what))
            return
        Wd = W.astype(np.float64)
        ref = S.astype(np.float64) @ Wd.T
        mag = np.abs(S.astype(np.float64)) @ np.abs(Wd).T
        if b is not None:
            ref, mag = ref + b.astype(np.float64), mag + np.abs(b.astype(np.float64))
        if self.relu:
            ref = np.maximum(ref, 0.0)
        unit = 2e-6 if self.kind == 'split' else (256 + 2) * 2.0 ** -24
        err = np.abs(Kh.astype(np.float64) - ref)
        ratio = float((err / np.maximum(unit * mag, 1e-300)).max()) if err.size else 0.0
        WORST[self.route] = max(WORST.get(self.route, 0.0), ratio)
        print('%s %s: worst |K - fp64| / bound = %.4f (route %s so far %.4f)' % (self.name, what, ratio, self.route, WORST[self.route]))
        over = ~(err <= unit * mag)
        assert not over.any(), '%s %s: %d elements of K outside the bound, worst ratio %.3f' % (self.name, what, int(over.sum()), ratio)

    # ---------------------------------------------------------------------------------------------------------------- launches
    def launch(self, mode, kprev, cs, y0=None, **kw):
        from ndcn_amd import hip
        out = hip.rhs_rk(self.A, self.X, self.W, self.b, mode, self.y0 if y0 is None else y0, kprev, cs, X_halo=self.Xh, relu=self.relu, **kw)
        torch.cuda.synchronize()
        return out

    def plain(self):
        from ndcn_amd import hip
        K = hip.rhs(self.A, self.X, self.W, self.b, X_halo=self.Xh, relu=self.relu)
        torch.cuda.synchronize()
        if not self.want & _L().PATH_SMALL:                     # (rhs_f32 hands narrow panels to rhs_small.hip without recording a path)
            assert rhs_path() == self.want, '%s plain: path %#x, want %#x' % (self.name, rhs_path(), self.want)
        self.check_K(K, what='plain')
        self.K0 = K
        self.Kh = self.h(K)
        return K

    def fused(self, mode, npv):
        """does (mode, npv) run inside the launch (rhs_fused2_variant / rhs_fused3_variant; rhs_small: every one)"""
        if self.want & _L().PATH_SMALL:
            return True
        return mode != 'error' or npv in (1, 5)

    def targets(self, npv):
        """(label, y0, stages): the plain inputs, then the special set in y0 and in every earlier stage in turn"""
        yield 'plain inputs', self.y0, self.ks[:npv]
        yield 'specials in y0', plant(self.y0, 1), self.ks[:npv]
        for j in range(npv):
            yield 'specials in stage %d' % j, self.y0, self.ks[:j] + [plant(self.ks[j], 2 + j)] + self.ks[j + 1:npv]

    def same_K(self, K, what):
        assert rhs_path() == self.want, '%s %s: path %#x, want %#x' % (self.name, what, rhs_path(), self.want)
        assert torch.equal(K.view(torch.int32), self.K0.view(torch.int32)), '%s %s: K differs from the plain launch' % (self.name, what)

    def combine(self, stage_counts=range(6), specials=True, from_zero=False):
        for npv in stage_counts:
            cs, c2 = CS[:npv] + [CS[5]], AUX[:npv] + [AUX[5]]
            for label, y0, ks in self.targets(npv):
                if label != 'plain inputs' and not specials:
                    continue
                for with_aux in ((False, True) if label == 'plain inputs' else (True,)):
                    what = 'combine %d aux=%s %s' % (npv, with_aux, label)
                    out = self.launch('combine', ks, cs, y0=y0, aux_cs=c2 if with_aux else None)
                    self.same_K(out[0], what)
                    kk = [self.h(k) for k in ks] + [self.Kh]
                    same_bits(self.h(out[1]), E.combine(self.h(y0), kk, cs, from_zero), '%s %s: y_next' % (self.name, what))
                    if with_aux:
                        same_bits(self.h(out[2]), E.aux(kk, c2, from_zero), '%s %s: y_aux' % (self.name, what))

    def rk4(self, stages=range(4), specials=True):
        dt = F(0.37)
        for st in stages:
            for label, y0, ks in self.targets(st):
                if label != 'plain inputs' and not specials:
                    continue
                what = 'rk4 stage %d %s' % (st, label)
                K, yn = self.launch('rk4', ks, [dt], y0=y0)
                self.same_K(K, what)
                same_bits(self.h(yn), E.rk4_stage(st, self.h(y0), [self.h(k) for k in ks] + [self.Kh], dt), '%s %s' % (self.name, what))

    def check_record(self, rec, y0, y1, ks, cs, rtol, atol, what, inside):
        """inside: the record was formed in the launch (fp64); else by rk_error_f32 - ATen order up to 2^18 elements, parallel fp64 above"""
        L = _L()
        s1, b1 = rec
        kk = [k.cpu().numpy() for k in ks] + [self.K0.cpu().numpy()]
        zz, bad = E.error_terms(y0.cpu().numpy(), y1.cpu().numpy(), kk, cs, rtol, atol, from_zero=not inside)
        assert b1 == float(bad), '%s %s: non-finite count %r, want %d' % (self.name, what, b1, bad)
        if inside:
            check_sum(s1, zz, '%s %s' % (self.name, what))
        elif zz.size <= (1 << 18):
            assert rk_path() & 0xffffffff == L.RKF_ERROR | L.RKF_ATEN and rk_path() >> 32 == 1, hex(rk_path())
            check_sum_aten(s1, zz, '%s %s' % (self.name, what))
        else:
            assert rk_path() & 0xffffffff == L.RKF_ERROR | L.RKF_VEC | L.RKF_PAR64 and rk_path() >> 32 >= 1, hex(rk_path())
            check_sum(s1, zz, '%s %s' % (self.name, what))
        return bad

    def error(self, stage_counts=range(6), specials=True):
        assert self.rows is None
        y1x = self.X[:self.n]                                   # the default y1: the evaluation's input, by row of the launch
        for npv in stage_counts:
            cs = CS[:npv] + [CS[5]]
            inside = self.fused('error', npv)
            for rtol, atol in TOLS:
                what = 'error %d rtol %g atol %g' % (npv, rtol, atol)
                K, rec = self.launch('error', self.ks[:npv], cs, rtol=rtol, atol=atol)
                self.same_K(K, what)
                assert self.check_record(rec, self.y0, y1x, self.ks[:npv], cs, rtol, atol, what, inside) == 0
            if not specials:
                continue
            rtol, atol = TOLS[0]
            for label, y0, ks in list(self.targets(npv))[1:]:
                K, rec = self.launch('error', ks, cs, y0=y0, rtol=rtol, atol=atol)
                self.same_K(K, 'error %d %s' % (npv, label))
                self.check_record(rec, y0, y1x, ks, cs, rtol, atol, 'error %d %s' % (npv, label), inside)
            # y1 given explicitly: finite specials and +-Inf (counted; z = 0 there: the sum stays finite or +Inf), then a NaN too
            y1 = plant(y1x, 9)
            n_inf = int(torch.isinf(y1).sum())
            assert n_inf > 0 and int(torch.isnan(y1).sum()) > 0
            y1_inf = torch.where(torch.isnan(y1), torch.zeros_like(y1), y1)
            for label, yy, count in (('y1 with +-Inf', y1_inf, n_inf), ('y1 with +-Inf and NaN', y1, n_inf + int(torch.isnan(y1).sum()))):
                K, rec = self.launch('error', self.ks[:npv], cs, rtol=rtol, atol=atol, y1=yy)
                self.same_K(K, 'error %d %s' % (npv, label))
                assert self.check_record(rec, self.y0, yy, self.ks[:npv], cs, rtol, atol, 'error %d %s' % (npv, label), inside) == count
                assert math.isnan(rec[0]) == ('NaN' in label)
            # atol = 0 where y0 = y1 = 0: tol = 0, the term is +Inf or NaN (error_terms states which)
            y0z, y1z = self.y0.clone(), y1x.clone()
            y0z[0, 0] = y1z[0, 0] = 0.0
            y0z[self.n - 1, self.H - 1], y1z[self.n - 1, self.H - 1] = -0.0, 0.0
            K, rec = self.launch('error', self.ks[:npv], cs, y0=y0z, rtol=TOLS[1][0], atol=TOLS[1][1], y1=y1z)
            self.check_record(rec, y0z, y1z, self.ks[:npv], cs, TOLS[1][0], TOLS[1][1], 'error %d zero tolerance' % npv, inside)
            assert not math.isfinite(rec[0])

    def all_modes(self, specials=True):
        self.plain()
        self.combine(specials=specials)
        self.rk4(specials=specials)
        self.error(specials=specials)

    def some_modes(self):
        """one instantiation per mode, plain inputs and the specials in y0 / the last stage"""
        self.plain()
        self.combine((2, 5), specials=False)
        self.combine((1,), specials=True)
        self.rk4((1, 3), specials=False)
        self.error((1, 5, 3), specials=False)


# ------------------------------------------------------------------------------------------------------------------- operators
def lattice(side):
    from ndcn_amd import graphs
    m = graphs.normalized_laplacian(graphs.grid_8_neighbor(side)).tocsr().astype(np.float32)
    m.sort_indices()
    return m


def op(m, dev, plans=False):
    from ndcn_amd import CsrOperator
    m = sp.csr_matrix(m)
    m.sort_indices()
    A = CsrOperator.from_arrays(m.indptr, m.indices, m.data, m.shape, dev)
    if not plans:
        A._plans_tried = True
    return A


def rec_op(m, dev, hint=None, order_from=None):
    """the (16, 40, 2) record plan of rhs_fused3.hip on the lattice walk order"""
    A = op(m, dev)
    if hint is not None:
        A.lattice_hint = hint
    src = A if order_from is None else order_from
    A.group_order = torch.as_tensor(src.detect_stencil_order(), dtype=torch.int32).to(dev)
    A.build_rec_plan(16, 40, 2)
    assert A.view().rec_groups > 0
    return A


def rand_rows(n_rows, n_cols, seed, avg=6, lengths=None):
    rng = np.random.RandomState(seed)
    deg = rng.poisson(avg, size=n_rows) if lengths is None else np.resize(np.asarray(lengths), n_rows)
    deg = np.minimum(deg, n_cols)
    rows = np.repeat(np.arange(n_rows), deg)
    cols = np.concatenate([rng.choice(n_cols, size=d, replace=False) for d in deg]) if rows.size else np.zeros(0, np.int64)
    m = sp.csr_matrix(((rng.randn(rows.size) / 4).astype(np.float32), (rows, cols)), shape=(n_rows, n_cols))
    m.sort_indices()
    return m


def wide_range_weights(seed=0):
    """four elements of output row 17 sit 2^-24 below the row's largest (kS16GuardCount = 4, in-row range beyond 2^19): the range
    guard sends the launch to the fp32 matrix cores"""
    g = torch.Generator().manual_seed(seed)
    W = (torch.rand(256, 256, generator=g) - 0.5) / 8
    W[17, 33] = 1.0
    W[17, 40:44] = torch.tensor([1.0, -1.5, 1.25, 1.75]) * 2.0 ** -24
    return W.contiguous()


@pytest.fixture
def range_guard_default():
    """the guard as shipped (on), whatever an earlier test left; restored, and the packed images dropped, afterwards"""
    from ndcn_amd.ops import invalidate_packed_weights
    prev = _L().load().ndcn_set_range_guard(1)
    invalidate_packed_weights()
    yield
    _L().load().ndcn_set_range_guard(prev)
    invalidate_packed_weights()


# ------------------------------------------------------------------------------------------------------------------- FUSED3
@pytest.mark.parametrize('which', ['41', 'halo', 'hot', '72'])
def test_fused3(dev, which):
    L = _L()
    if which == '41':
        m = lattice(41)
        c = Case('FUSED3 side 41', m, rec_op(m, dev), dev, L.PATH_FUSED3)
        assert c.A.rec['groups'] == 121 and 41 % 4
        c.all_modes()
    elif which == 'halo':
        m = sp.csr_matrix(lattice(41)[:1200])
        c = Case('FUSED3 halo', m, rec_op(m, dev, hint=(0, 1200)), dev, L.PATH_FUSED3 | L.PATH_HALO, n_own=1200, seed=2)
        c.all_modes()
    elif which == 'hot':
        n = 41 * 41
        base = lattice(41)
        rs = np.random.RandomState(41)
        hot = np.repeat(rs.choice(n, 6, replace=False), 12)
        m = (base + sp.csr_matrix((rs.rand(72).astype(np.float32), (hot, rs.randint(0, n, 72))), shape=(n, n))).tocsr()
        m.sort_indices()
        A = rec_op(m, dev, order_from=op(base, dev))
        assert 0.5 < A.rec['staged'] < 1.0
        Case('FUSED3 hot rows', m, A, dev, L.PATH_FUSED3, seed=3).some_modes()
    else:
        m = lattice(72)
        c = Case('FUSED3 side 72', m, rec_op(m, dev), dev, L.PATH_FUSED3, seed=4)
        assert c.A.rec['groups'] > 256
        c.some_modes()


def test_fused3_beyond_128_mib(dev):
    """side 363: 131 769 rows, panels of 128.7 MiB - the NT = true instantiations without a halo panel, each mode once; K, y_next and
    y_aux on the first and last 48 rows (three groups at either end) plus 2048 seeded rows, the error record over every element"""
    L = _L()
    side = 363
    n = side * side
    assert n * 1024 > (128 << 20)
    m = lattice(side)
    rows = np.unique(np.r_[np.arange(48), np.arange(n - 48, n), np.random.RandomState(0).randint(0, n, 2048)])
    A = op(m, dev, plans=True)
    A.ensure_plans(256)
    assert A.rec is not None and (A.rec['rows'], A.rec['cap'], A.rec['kib']) == (16, 40, 2)
    c = Case('FUSED3 side 363', m, A, dev, L.PATH_FUSED3, seed=5, rows=rows)
    c.plain()
    c.combine((5,), specials=False)
    c.rk4((3,), specials=False)
    c.rows = c.rows_t = None
    cs = CS
    rtol, atol = TOLS[0]
    y1 = c.X.clone()
    y1[0, 0], y1[n - 1, 255], y1[n // 2, 7] = float('inf'), -float('inf'), float('inf')
    K, rec = c.launch('error', c.ks, cs, rtol=rtol, atol=atol, y1=y1)
    c.same_K(K, 'error 5')
    assert c.check_record(rec, c.y0, y1, c.ks, cs, rtol, atol, 'error 5', True) == 3 and math.isfinite(rec[0])


# ------------------------------------------------------------------------------------------------------------------- FUSED2
@pytest.mark.parametrize('n', [1, 63, 64, 65, 129])
def test_fused2_small_sizes(dev, n):
    m = rand_rows(n, n, seed=n, avg=min(6, n))
    Case('FUSED2 n=%d' % n, m, op(m, dev), dev, _L().PATH_FUSED2, seed=n).all_modes(specials=(n == 65))


@pytest.mark.parametrize('which', ['halo', 'lengths', 'hub', 'tiles'])
def test_fused2(dev, which):
    L = _L()
    if which == 'halo':
        m = rand_rows(700, 1000, seed=7)
        Case('FUSED2 halo', m, op(m, dev), dev, L.PATH_FUSED2 | L.PATH_HALO, n_own=700, seed=7).all_modes()
    elif which == 'lengths':
        n = 71 * 13 + 5
        m = rand_rows(n, n, seed=8, lengths=np.arange(71))
        Case('FUSED2 row lengths 0..70', m, op(m, dev), dev, L.PATH_FUSED2, seed=8).all_modes()
    elif which == 'hub':
        from ndcn_amd import graphs
        m = graphs.normalized_laplacian(graphs.make_graph('power_law', 2000, seed=0)).tocsr().astype(np.float32)
        m.sort_indices()
        A = op(m, dev, plans=True)
        os.environ['NDCN_HUB_THRESHOLD'] = '32'
        try:
            A.ensure_plans(256)
        finally:
            del os.environ['NDCN_HUB_THRESHOLD']
        assert A.hub is not None and A.hub['n'] > 0 and A.hub['threshold'] == 32 and A.sweep is None
        Case('FUSED2 hub', m, A, dev, L.PATH_FUSED2 | L.PATH_HUB, hub_thr=32, seed=9).some_modes()
    else:
        n = 64 * 257 + 1                                        # 258 tiles on a grid of 256 workgroups
        m = rand_rows(n, n, seed=10, avg=5)
        Case('FUSED2 258 tiles', m, op(m, dev), dev, L.PATH_FUSED2, seed=10).some_modes()


def _split_error(c, blocks, make_op, inside=True):
    """ERROR over row blocks of one state into one record (accum on every launch but the first): the any-tree bound over all terms
    plus the accumulating adds"""
    from ndcn_amd import hip
    rec = hip.new_error_record(c.dev)
    rtol, atol = TOLS[0]
    terms, bad, r = [], 0, None
    y1 = plant(c.X[:c.n], 4)
    y1 = torch.where(torch.isnan(y1), torch.zeros_like(y1), y1)
    for i, (lo, hi) in enumerate(blocks):
        A = make_op(sp.csr_matrix(c.m[lo:hi]))
        ks = [k[lo:hi].contiguous() for k in c.ks]
        K, r = hip.rhs_rk(A, c.X, c.W, c.b, 'error', c.y0[lo:hi].contiguous(), ks, CS, rtol=rtol, atol=atol, y1=y1[lo:hi].contiguous(),
                          accum=i > 0, record=rec, fetch=i == len(blocks) - 1)
        torch.cuda.synchronize()
        assert rhs_path() == c.want, hex(rhs_path())
        assert torch.equal(K.view(torch.int32), c.K0[lo:hi].view(torch.int32))
        zz, b = E.error_terms(c.y0[lo:hi].cpu().numpy(), y1[lo:hi].cpu().numpy(), [k.cpu().numpy() for k in ks] + [K.cpu().numpy()], CS, rtol, atol)
        terms.append(zz)
        bad += b
    assert r[1] == float(bad) and bad == int(torch.isinf(y1).sum()) > 0
    check_sum(r[0], terms, c.name + ' split error', extra_adds=len(blocks) - 1)


def test_error_split_over_three_row_blocks(dev):
    L = _L()
    m = rand_rows(1500, 1500, seed=11)
    c = Case('FUSED2 split', m, op(m, dev), dev, L.PATH_FUSED2, seed=11)
    c.plain()
    _split_error(c, ((0, 400), (400, 1101), (1101, 1500)), lambda part: op(part, dev))
    m = rand_rows(600, 600, seed=12)
    c = Case('SMALL split', m, op(m, dev), dev, L.PATH_SMALL, kind='chain', H=64, seed=12)
    c.plain()
    _split_error(c, ((0, 100), (100, 333), (333, 600)), lambda part: op(part, dev))
    # FUSED3: row blocks of the lattice under the record plan on consecutive rows (no walk order: most groups are gathered directly)
    m = lattice(41)
    c = Case('FUSED3 split', m, rec_op(m, dev), dev, L.PATH_FUSED3, seed=13)
    c.plain()

    def block_op(part):
        A = op(part, dev)
        A.build_rec_plan(16, 40, 2)
        return A
    _split_error(c, ((0, 512), (512, 1200), (1200, 1681)), block_op)


def test_composed_error_in_aten_order(dev):
    """ERROR with 0, 2, 3, 4 earlier stages at H = 256 on 1024 rows (2^18 elements): the plain fused launch + rk_error_aten_kernel,
    bit-equal to the cascade sum; FUSED3 (side 32) and FUSED2"""
    L = _L()
    m = lattice(32)
    c = Case('FUSED3 side 32', m, rec_op(m, dev), dev, L.PATH_FUSED3, seed=14)
    c.plain()
    c.error((0, 2, 3, 4), specials=True)
    m = rand_rows(1024, 1024, seed=15)
    c = Case('FUSED2 n=1024', m, op(m, dev), dev, L.PATH_FUSED2, seed=15)
    c.plain()
    c.error((0, 2, 3, 4), specials=False)


# ------------------------------------------------------------------------------------------------------------------- SWEEP
def test_sweep(dev):
    from ndcn_amd import graphs
    L = _L()
    if torch.cuda.get_device_properties(dev).multi_processor_count != 256:
        pytest.skip('the column sweep needs the whole chip (device_is_whole_chip): its workgroups must be co-resident')
    m = graphs.normalized_laplacian(graphs.make_graph('random', 9000, seed=1)).tocsr().astype(np.float32)
    m.sort_indices()
    A = op(m, dev, plans=True)
    A.ensure_plans(256)
    assert A.sweep is not None
    Case('SWEEP', m, A, dev, L.PATH_FUSED3 | L.PATH_SWEEP, seed=16).some_modes()


# ------------------------------------------------------------------------------------------------------------------- EXACT32
@pytest.mark.parametrize('which', ['no_plan', 'halo', 'lattice'])
def test_exact32(dev, which, range_guard_default):
    L = _L()
    W = wide_range_weights()
    if which == 'no_plan':
        m = rand_rows(700, 700, seed=17)
        c = Case('EXACT32 no plan', m, op(m, dev), dev, L.PATH_EXACT32, kind='fp32', W=W, seed=17)
        c.all_modes(specials=False)
        c.combine((3,), specials=True)
    elif which == 'halo':
        m = rand_rows(300, 500, seed=18)
        Case('EXACT32 halo', m, op(m, dev), dev, L.PATH_EXACT32 | L.PATH_HALO, kind='fp32', W=W, n_own=300, seed=18).some_modes()
    else:
        m = lattice(41)
        Case('EXACT32 lattice', m, rec_op(m, dev), dev, L.PATH_EXACT32, kind='fp32', W=W, seed=19).some_modes()


# ------------------------------------------------------------------------------------------------------------------- SMALL
@pytest.mark.parametrize('n', [1, 300])
@pytest.mark.parametrize('H', [1, 20, 64, 65, 128])
def test_small(dev, H, n):
    m = rand_rows(n, n, seed=H + n, avg=min(6, n), lengths=None if n == 1 else np.r_[np.arange(12), 70, 0, 3])
    Case('SMALL H=%d n=%d' % (H, n), m, op(m, dev), dev, _L().PATH_SMALL, kind='chain', H=H, seed=H).all_modes(specials=(n == 300 and H in (20, 65)))


def test_small_halo(dev):
    m = rand_rows(200, 320, seed=21)
    Case('SMALL halo', m, op(m, dev), dev, _L().PATH_SMALL, kind='chain', H=65, n_own=200, seed=21).all_modes(specials=False)


def test_small_threshold(dev):
    """n H = 2^18 stays on rhs_small.hip; n H = 2^18 + 128 takes the composed path (row SpMM, MFMA Linear, stand-alone stage kernels:
    the same K bits; the stage sums from +0; the error record in parallel fp64)"""
    L = _L()
    H = 128
    m = rand_rows(2048, 2048, seed=22, avg=4)
    c = Case('SMALL n H = 2^18', m, op(m, dev), dev, L.PATH_SMALL, kind='chain', H=H, seed=22)
    c.plain()
    c.combine((2,), specials=False)
    c.error((5,), specials=False)
    m = rand_rows(2049, 2049, seed=23, avg=4)
    c = Case('composed n H > 2^18', m, op(m, dev), dev, 0, kind='chain', H=H, seed=23)
    from ndcn_amd import hip
    c.K0 = hip.rhs(c.A, c.X, c.W, c.b)
    c.Kh = c.K0.cpu().numpy()
    c.check_K(c.K0, what='plain')
    c.fused = lambda mode, npv: False
    c.combine((0, 2, 5), specials=True, from_zero=True)
    assert rk_path() & 0xffffffff == L.RKF_COMBINE | L.RKF_VEC, hex(rk_path())
    c.error((0, 5), specials=True)
    dt = F(0.37)
    K, yn = c.launch('rk4', c.ks[:2], [dt])
    assert rhs_path() == 0 and rk_path() & 0xff == L.RKF_FIXED_STAGE
    same_bits(yn.cpu().numpy(), E.rk4_stage(2, c.y0.cpu().numpy(), [k.cpu().numpy() for k in c.ks[:2]] + [c.Kh], dt), 'composed rk4')


# ------------------------------------------------------------------------------------------------------------------- FUSED3 options
def test_xadd(dev, range_guard_default):
    """ndcn_rhs_rk_xadd_f32: the input is fl(X + fl(c Xadd)) in numpy float32; K and y_next by the oracles above; with wide-range
    weights the launch stays on the split product and sets PATH_RANGE (operands inside the guarantee here: the bound still holds)"""
    from ndcn_amd import hip
    L = _L()
    m = lattice(41)
    c = Case('FUSED3 x_add', m, rec_op(m, dev), dev, L.PATH_FUSED3, seed=24, route='FUSED3 options')
    g = torch.Generator(device=dev).manual_seed(25)
    xadd = rows_scaled(c.n, 256, g, dev, k=2)
    xc = F(0.0371)
    cs = [CS[0], CS[5]]
    with np.errstate(all='ignore'):
        Xin = torch.from_numpy(c.X.cpu().numpy() + xadd.cpu().numpy() * xc)
    S = c.S32(Xin)
    for label, y0, k1 in (('plain inputs', c.y0, c.ks[0]), ('specials in y0', plant(c.y0, 1), c.ks[0]), ('specials in the stage', c.y0, plant(c.ks[0], 2))):
        got = hip.rhs_rk_xadd(c.A, c.X, xadd, xc, c.W, c.b, y0, k1, cs)
        torch.cuda.synchronize()
        assert got is not None and rhs_path() == L.PATH_FUSED3
        c.check_K(got[0], S, 'x_add ' + label)
        same_bits(got[1].cpu().numpy(), E.combine(y0.cpu().numpy(), [k1.cpu().numpy(), got[0].cpu().numpy()], cs), 'x_add y_next ' + label)
    # wide-range weights whose small elements meet ordinary S: no fp32 form of this launch, the split product and PATH_RANGE
    c.W = wide_range_weights().to(dev)
    got = hip.rhs_rk_xadd(c.A, c.X, xadd, xc, c.W, c.b, c.y0, c.ks[0], cs)
    torch.cuda.synchronize()
    assert rhs_path() == L.PATH_FUSED3 | L.PATH_RANGE, hex(rhs_path())
    c.check_K(got[0], S, 'x_add wide-range weights')
    same_bits(got[1].cpu().numpy(), E.combine(c.y0.cpu().numpy(), [c.ks[0].cpu().numpy(), got[0].cpu().numpy()], cs), 'x_add y_next PATH_RANGE')
    K, _ = c.launch('combine', c.ks[:1], cs)                    # the same weights without the option: the fp32 route
    assert rhs_path() == L.PATH_EXACT32


@pytest.mark.parametrize('half', ['mask', 's_out'])
def test_adjoint_halves(dev, half):
    """ndcn_rhs_rk_adj_f32, COMBINE 1..4 and ERROR 5.  mask: the input is X where mask > 0 or the mask is NaN, +0 elsewhere (the
    transposed half: no ReLU, no bias); s_out: S = A X leaves the launch too, bit for bit the chain"""
    L = _L()
    m = lattice(41)
    A = rec_op(m, dev)
    if half == 'mask':
        g = torch.Generator(device=dev).manual_seed(26)
        M = torch.rand(m.shape[0], 256, generator=g, device=dev) - 0.4
        r = torch.arange(m.shape[0], device=dev)
        M[r, (7 * r) % 256] = torch.tensor((0.0, -0.0, 1e-40, -1e-40, 1e-37, float('nan')), device=dev)[r % 6]
        c = Case('FUSED3 x_mask', m, A, dev, L.PATH_FUSED3, seed=27, b=False, relu=False, route='FUSED3 options')
        Mh = M.cpu().numpy()
        Xin = torch.from_numpy(np.where((Mh > 0) | np.isnan(Mh), c.X.cpu().numpy(), F(0)).astype(np.float32))
        kw = dict(x_mask=M)
    else:
        c = Case('FUSED3 s_out', m, A, dev, L.PATH_FUSED3, seed=28, route='FUSED3 options')
        Xin, kw = c.X, {}
    S = c.S32(Xin)
    rtol, atol = TOLS[0]
    K0 = None
    for mode, npv in (('combine', 1), ('combine', 2), ('combine', 3), ('combine', 4), ('error', 5)):
        from ndcn_amd import hip
        assert hip.rhs_adj_supported(c.A, 256, mode, npv)
        cs = CS[:npv] + [CS[5]]
        y0 = plant(c.y0, npv)
        ks = c.ks[:npv - 1] + [plant(c.ks[npv - 1], npv + 1)]
        if half == 's_out':
            kw = dict(s_out=torch.full_like(c.X, float('nan')))
        y1 = c.X if mode == 'error' else None
        out = c.launch(mode, ks, cs, y0=y0, rtol=rtol, atol=atol, y1=y1, **kw)
        what = '%s %s %d' % (half, mode, npv)
        assert rhs_path() == L.PATH_FUSED3, what
        c.check_K(out[0], S, what)
        if K0 is not None:
            assert torch.equal(out[0].view(torch.int32), K0.view(torch.int32)), what
        K0 = c.K0 = out[0]
        if half == 's_out':
            same_bits(kw['s_out'].cpu().numpy(), S, what + ': S')
        if mode == 'combine':
            same_bits(out[1].cpu().numpy(), E.combine(y0.cpu().numpy(), [k.cpu().numpy() for k in ks] + [K0.cpu().numpy()], cs), what + ': y_next')
        else:
            c.check_record(out[1], y0, c.X, ks, cs, rtol, atol, what, True)


def test_refusals(dev):
    """what the launchers refuse returns NDCN_EINVAL and launches nothing"""
    from ndcn_amd import hip
    from ndcn_amd.ops import ptr, stream_ptr
    L = _L()
    lib = L.load()
    m = lattice(24)
    n = m.shape[0]
    A3, A2 = rec_op(m, dev), op(m, dev)
    c = Case('refusals', m, A3, dev, L.PATH_FUSED3, seed=29)
    K, yn, S, M = (torch.empty_like(c.X) for _ in range(4))
    M.fill_(1.0)
    red, ws = torch.zeros(2, dtype=torch.float64, device=dev), torch.empty(int(lib.ndcn_reduce_ws_bytes()), dtype=torch.uint8, device=dev)
    work = torch.empty(int(lib.ndcn_rhs_work_bytes(n, 256, L.F_RELU)), dtype=torch.uint8, device=dev)

    def adj(A, mask, s_out, rk, npv):
        arr_k = (ctypes.c_void_p * 5)(*[k.data_ptr() for k in c.ks])
        arr_c = (ctypes.c_float * 6)(*[float(v) for v in CS])
        with torch.cuda.device(dev):
            return int(lib.ndcn_rhs_rk_adj_f32(A.view_ref(), ptr(c.X), ptr(mask), ptr(s_out), ptr(c.W), ptr(c.b), ptr(K), ptr(work), 256, L.F_RELU,
                                               rk, ptr(c.y0), arr_k, arr_c, npv, ptr(yn), None, 1e-2, 1e-3, ptr(red), ptr(ws), stream_ptr()))

    def xadd(A):
        arr_c = (ctypes.c_float * 2)(0.1, 0.2)
        with torch.cuda.device(dev):
            return int(lib.ndcn_rhs_rk_xadd_f32(A.view_ref(), ptr(c.X), ptr(M), 0.5, ptr(c.W), ptr(c.b), ptr(K), ptr(work), 256, L.F_RELU,
                                                ptr(c.y0), ptr(c.ks[0]), arr_c, ptr(yn), stream_ptr()))

    assert adj(A3, M, None, L.RK_COMBINE, 2) == 0 and adj(A3, None, S, L.RK_ERROR, 5) == 0 and xadd(A3) == 0
    assert adj(A3, M, S, L.RK_COMBINE, 2) == L.EINVAL                   # mask and s_out together
    assert adj(A3, None, None, L.RK_COMBINE, 2) == L.EINVAL             # neither
    for rk, npv in ((L.RK_COMBINE, 0), (L.RK_COMBINE, 5), (L.RK_ERROR, 1), (L.RK_RK4, 1)):
        assert adj(A3, M, None, rk, npv) == L.EINVAL and adj(A3, None, S, rk, npv) == L.EINVAL
        assert not lib.ndcn_rhs_adj_supported(A3.view_ref(), 256, L.F_RELU, rk, npv)
    assert adj(A2, M, None, L.RK_COMBINE, 2) == L.EINVAL and adj(A2, None, S, L.RK_COMBINE, 2) == L.EINVAL     # without the plan
    assert xadd(A2) == L.EINVAL and hip.rhs_rk_xadd(A2, c.X, M, 0.5, c.W, c.b, c.y0, c.ks[0], CS[:2]) is None
    assert not lib.ndcn_rhs_xadd_supported(A3.view_ref(), 256, L.F_RELU, L.RK_COMBINE, 2)
    assert not lib.ndcn_rhs_xadd_supported(A2.view_ref(), 256, L.F_RELU, L.RK_COMBINE, 1)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------- first generation
def child_main():
    """NDCN_RHS_FUSED2=0: rhs_fused.hip serves the plain launch (fp32 MFMA: the (256 + 2) 2^-24 bound), the stage algebra runs
    stand-alone - COMBINE 2 from +0, ERROR 5 in ATen order (1024 rows) - and ndcn_debug_last_rhs_path reads 0"""
    dev = torch.device('cuda:0')
    m = lattice(32)
    c = Case('first generation', m, op(m, dev, plans=True), dev, 0, kind='fp32', seed=30)
    from ndcn_amd import hip
    c.K0 = hip.rhs(c.A, c.X, c.W, c.b)
    c.Kh = c.K0.cpu().numpy()
    c.check_K(c.K0, what='plain')
    c.fused = lambda mode, npv: False
    c.combine((2,), specials=True, from_zero=True)
    c.error((5,), specials=True)
    print('first generation ok, worst ratio %.4f' % WORST['first'])


def test_first_generation_kernel_in_a_child_process(dev):
    code = 'import sys; sys.path[:0] = [%r, %r]; import test_gpu_rhs_rk_routes as t; t.child_main()' % (ROOT, HERE)
    env = dict(os.environ, NDCN_RHS_FUSED2='0')
    r = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout[-1500:])
    assert r.returncode == 0 and 'first generation ok' in r.stdout, r.stderr[-3000:]
