"""tests/_rownorm.py (the float64 restatement the device kernels of csrc/rownorm.hip are tested against) pinned from two sides: to
double-precision torch autograd through F.normalize(x, 1, 1) and the infinity fill, special rows included, and to the reference's
recorded float32 output (tests/golden/resgcn_rownorm.npz) and the float32 CPU oracle, which must lie inside its forward bound."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _rownorm
from conftest import load_golden
from oracle import ndcn_oracle as orc

RTOL = 1e-13
SHAPES = [(1, 1), (3, 2), (5, 3), (12, 4), (13, 5), (24, 32), (9, 63), (14, 65), (12, 260), (12, 1023), (13, 1024), (12, 2050)]


def torch_double(X, G):
    x = torch.from_numpy(X.astype(np.float64)).requires_grad_()
    y = F.normalize(x, 1, 1, eps=_rownorm.EPS)
    y = y.masked_fill(torch.isinf(y), 0.0)
    y.backward(torch.from_numpy(G.astype(np.float64)))
    return y.detach().numpy(), x.grad.numpy()


def same_nans(got, want):
    return np.array_equal(np.isnan(got), np.isnan(want))


@pytest.mark.parametrize('n_rows,H', SHAPES)
def test_restatement_is_double_precision_autograd(n_rows, H):
    for seed in range(12):                                   # the special rows rotate with the seed: small panels see each of them
        X, index = _rownorm.panel(n_rows, H, seed)
        G = np.random.RandomState(100 + seed).normal(0, 1, X.shape).astype(np.float32)
        y, gx = torch_double(X, G)
        mine, mine_gx = _rownorm.forward(X), _rownorm.vjp(G, X)
        assert same_nans(mine, y) and same_nans(mine_gx, gx), (seed, index)
        ok = ~np.isnan(y)
        assert (np.abs(mine - y)[ok] <= RTOL * np.abs(y)[ok]).all(), seed
        # relative to the magnitudes that enter the element, |g_j| / den + sum |g_i x_i| / den^2: the two terms may cancel
        Xd, Gd = X.astype(np.float64), G.astype(np.float64)
        with np.errstate(invalid='ignore', over='ignore'):
            den = np.maximum(np.abs(Xd).sum(1, keepdims=True), _rownorm.EPS)
            scale = np.abs(Gd) / den + np.abs(Gd * Xd).sum(1, keepdims=True) / (den * den)
        ok = ~np.isnan(gx)
        assert (np.abs(mine_gx - gx)[ok] <= RTOL * scale[ok]).all(), seed


def test_special_rows_are_what_they_claim():
    X, index = _rownorm.panel(16, 8, 0)
    assert set(index) == set(_rownorm.SPECIAL)
    s = np.abs(X.astype(np.float64)).sum(1)
    r = lambda name: index[name][0]
    assert s[r('zeros')] == 0 and s[r('signed_zeros')] == 0 and np.signbit(X[r('signed_zeros')]).any()
    assert 0.5e-13 < s[r('clamped')] < 2e-13 and 0.5e-11 < s[r('not_clamped')] < 2e-11
    assert 0 < np.abs(X[r('denormal')]).max() < np.finfo(np.float32).tiny and np.count_nonzero(X[r('one_hot')]) == 1
    assert (X[r('negative')] < 0).all() and np.count_nonzero(X[r('one_zero')] == 0) == 1 and X[index['one_zero']] == 0
    assert 8e14 < s[r('huge')] <= 1e15
    assert np.isnan(X[index['nan']]) and X[index['pos_inf']] == np.inf and X[index['neg_inf']] == -np.inf
    finite = np.isfinite(X).all(1)
    assert finite.sum() == 13 and s[finite].max() <= 1e15
    y, gx = _rownorm.forward(X), _rownorm.vjp(np.ones_like(X), X)
    for name in ('zeros', 'signed_zeros', 'clamped', 'denormal'):                  # clamped: x / eps forward, g / eps in reverse
        assert np.array_equal(y[r(name)], X[r(name)].astype(np.float64) / _rownorm.EPS) and (gx[r(name)] == 1.0 / _rownorm.EPS).all()
    assert np.isnan(y[r('nan')]).all() and np.isnan(gx[r('nan')]).all()
    for name in ('pos_inf', 'neg_inf'):
        row = y[r(name)]
        assert np.isnan(row[index[name][1]]) and not np.delete(row, index[name][1]).any() and np.isnan(gx[r(name)]).all()
    rz, jz = index['one_zero']
    assert gx[rz, jz] == 1.0 / s[rz]                                               # sign(0) = 0: no second term


def test_reference_output_lies_inside_the_forward_bound():
    d = load_golden('resgcn_rownorm')
    want, bound = _rownorm.forward(d['x']), _rownorm.forward_bound(d['x'])
    for got in (d['out'], orc.row_normalization(torch.from_numpy(d['x']).clone()).numpy()):
        assert got.dtype == np.float32 and (np.abs(got.astype(np.float64) - want) <= bound).all()
    for n_rows, H in SHAPES:
        X, _ = _rownorm.panel(n_rows, H, 3)
        got = orc.row_normalization(torch.from_numpy(X).clone()).numpy().astype(np.float64)
        want, bound = _rownorm.forward(X), _rownorm.forward_bound(X)
        ok = ~np.isnan(want)
        assert same_nans(got, want) and (np.abs(got - want)[ok] <= bound[ok]).all(), (n_rows, H)
