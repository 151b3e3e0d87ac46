"""Host side of the three-pass step of method 'adams' (csrc/adams_vc.hip): the calls are declared, bound and exported; the switch is
documented; and the numpy restatement the GPU tests compare the kernels with (tests/_adams_vc.py) equals, bit for bit, what
core.Adams.step's own sequence of scale / combine / error calls computes when it is driven with numpy float32 ops."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import _adams_vc as vc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ('ndcn_adams_predict_f32', 'ndcn_adams_correct_f32', 'ndcn_adams_update_f32')
f32 = np.float32


def test_calls_are_declared_bound_and_exported():
    from ndcn_amd import _lib
    text = open(os.path.join(ROOT, 'include', 'ndcn_hip.h')).read()
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r' T (ndcn_\w+)', out))
    for name in CALLS + ('ndcn_adams_correct_ws_bytes', 'ndcn_aten_norm_max'):
        m = re.search(r'NDCN_API\s+\w+\s+%s\s*\(([^)]*)\)' % name, text)
        assert m, '%s is not declared in include/ndcn_hip.h' % name
        args = [a for a in m.group(1).split(',') if a.strip() and a.strip() != 'void']
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == len(args), name
        assert name in exported, name
    lib = _lib.load()
    assert int(lib.ndcn_adams_correct_ws_bytes()) > 0


def test_abi_number_is_unchanged():
    from ndcn_amd import _lib
    text = open(os.path.join(ROOT, 'include', 'ndcn_hip.h')).read()
    assert int(re.search(r'#define\s+NDCN_ABI_VERSION\s+(\d+)', text).group(1)) == 29
    assert _lib.ABI_VERSION == 29 and _lib.load().ndcn_abi_version() == 29


def test_switch_is_documented_and_settable():
    from ndcn_amd import hip
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    section = doc.split('## Run-time switches', 1)[1].split('\n## ', 1)[0]
    assert re.search(r'^\| `NDCN_ADAMS_FUSED` \|', section, re.M)
    prev = hip.set_adams_fused(0)
    try:
        assert hip.adams_fused_on() == 0 and hip.set_adams_fused(1) == 0 and hip.adams_fused_on() == 1
    finally:
        hip.set_adams_fused(-1)
    assert hip.adams_fused_on() == prev


class NumpyOps:
    """core.Adams's panel ops over numpy float32 - separate roundings, left-to-right sums from +0 - recording every call"""

    def __init__(self):
        self.calls = []

    def scale(self, x, w):
        with np.errstate(all='ignore'):
            out = f32(w) * x.numpy()
        self.calls.append(('scale', out))
        return torch.from_numpy(out)

    def combine(self, y0, ks, cs):
        with np.errstate(all='ignore'):
            acc = f32(0) + f32(cs[0]) * ks[0].numpy()
            for k, c in zip(ks[1:], cs[1:]):
                acc = acc + f32(c) * k.numpy()
            out = y0.numpy() + acc
        self.calls.append(('combine', out))
        return torch.from_numpy(out)

    def error(self, y0, y1, ks, cs, rtol, atol):
        assert len(ks) == 1
        with np.errstate(all='ignore'):
            r2 = vc.ratio_sq(f32(0) + f32(cs[0]) * ks[0].numpy(), y0.numpy(), y1.numpy(), rtol, atol)
        self.calls.append(('error', r2))
        return float(r2.sum(dtype=np.float64)), 0.0


def panel(rng, n):
    x = rng.standard_normal(n).astype(f32)
    x[rng.integers(0, n, 3)] = f32(0.0)             # exact zeros of both signs: a - b is a + (0 + (-1) b), which is not a - b at -0 - (+0)
    x[rng.integers(0, n, 3)] = f32(-0.0)
    return x


@pytest.mark.parametrize('trunc', [False, True], ids=['max12', 'max_is_order'])
@pytest.mark.parametrize('order', [1, 2, 3, 4, 12])
def test_restatement_equals_the_step_driven_with_numpy_ops(order, trunc):
    from ndcn_amd.torchdiffeq._impl import core
    rng = np.random.default_rng(100 * order + trunc)
    n, max_order = 37, (order if trunc else 12)
    ops = NumpyOps()
    y0 = panel(rng, n)
    phis = [panel(rng, n) for _ in range(order)]
    nfs = [panel(rng, n), panel(rng, n)]               # f(p_next), f(y_next)
    evals = []

    def func(t, y):
        evals.append(y[0].numpy().copy())
        return (torch.from_numpy(nfs[len(evals) - 1]),)

    s = core.Adams(ops, func, (torch.from_numpy(y0),), 1e3, 1e3, max_order=max_order)         # tolerances that accept the step
    s.prev_t = [np.float64(1.0 - 0.07 * j - 0.003 * j * j) for j in range(order + 2)]        # uneven history, newest first
    s.prev_f = [None] * (order + 2)
    s.phi = [(torch.from_numpy(p),) for p in phis]
    s.order = order
    s.next_t = np.float64(1.05)
    assert s.fused is False
    assert s.step(np.float64(2.0)) is True
    # the coefficients, as step forms them
    dt32 = f32(np.float64(1.05) - np.float64(1.0))
    g64, betas64 = core.adams_g_and_beta([np.float64(1.0 - 0.07 * j - 0.003 * j * j) for j in range(order + 2)], np.float64(1.05), order)
    g = g64.astype(f32)
    betas = [None] + [f32(b) for b in betas64[1:]]
    m = max(1, order - 1)
    cs = [f32(dt32 * g[j]) for j in range(m)]
    select = order >= 3
    coefs = [f32(dt32 * f32(g[order] - g[order - 1])),
             f32(dt32 * f32(g[order - 1] - g[order - 2])) if select else None,
             f32(dt32 * f32(g[order - 2] - g[order - 3])) if select else None,
             f32(dt32 * f32(core.GAMMA_STAR[order])) if select and order < max_order else None]
    combines = [c[1] for c in ops.calls if c[0] == 'combine']
    errors = [c[1] for c in ops.calls if c[0] == 'error']
    assert sum(c[0] == 'scale' for c in ops.calls) == order - 1 and len(combines) == 2 * order + 2
    same = lambda a, b: a.tobytes() == b.tobytes()
    # predictor
    p_next = vc.predict(y0, phis, betas, cs, order)
    assert same(p_next, combines[0]) and same(p_next, evals[0])
    # corrector and sums: combines[1 .. order] are the chain, combines[order + 1] is y_next
    y_next, r2 = vc.correct(nfs[0], phis, betas, order, p_next, y0, f32(dt32 * g[order - 1]), coefs, 1e3, 1e3)
    assert same(y_next, combines[order + 1]) and same(y_next, evals[1])
    # the step asks for sum 0 always, sums 1 and 2 when it selects an order, sum 3 only where neither lower order wins
    got = [r for r in r2 if r is not None]
    assert len(got) == 1 + (2 if select else 0) + (1 if coefs[3] is not None else 0)
    assert len(errors) in ((len(got), len(got) - 1) if coefs[3] is not None else (len(got),))
    for a, b in zip(got, errors):
        assert same(a, b)
    # new phi: the step keeps iphi[:max_order]
    n_out = min(order + 1, max_order)
    new = vc.update(nfs[1], phis, betas, order, n_out)
    assert len(s.phi) == n_out
    for a, b in zip(new, s.phi):
        assert same(a, b[0].numpy())
    assert same(new[-1], combines[order + 1 + n_out - 1]) if n_out > 1 else True
