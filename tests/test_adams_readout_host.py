"""explicit_adams / fixed_adams inference with the decoder inside the solve: what can be said without a GPU - the three calls in the
header and the binding (ABI 29 unchanged), the routing predicate as a pure function against a table, and the order-of-operations oracle
of one step + decode (tests/_adams_readout.py: the existing restatements _adams_bashforth and _readout_chain composed) pinned against
float64 and against the orders it must NOT be."""
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _adams_bashforth as ab                                        # noqa: E402
import _adams_readout as aro                                         # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_CALLS = ('ndcn_ab_step_readout_f32', 'ndcn_solve_explicit_adams_readout_f32', 'ndcn_solve_fixed_adams_readout_f32')


def header():
    return open(os.path.join(ROOT, 'include', 'ndcn_hip.h')).read()


def test_header_and_binding_declare_the_three_calls():
    from ndcn_amd import _lib
    text = header()
    assert re.search(r'#define NDCN_ABI_VERSION 29\b', text) and _lib.ABI_VERSION == 29
    for name in NEW_CALLS:
        assert re.search(r'NDCN_API int %s\(' % name, text), name
        assert name in _lib.SIGNATURES, name
    # the argument lists: the un-decoded solve's with Wd, bd, C in front of `out`
    plain = _lib.SIGNATURES['ndcn_solve_explicit_adams_f32'][1]
    dec = _lib.SIGNATURES['ndcn_solve_explicit_adams_readout_f32'][1]
    assert len(dec) == len(plain) + 3 and dec[:13] == plain[:13] and dec[16:] == plain[13:]
    plain = _lib.SIGNATURES['ndcn_solve_fixed_adams_f32'][1]
    dec = _lib.SIGNATURES['ndcn_solve_fixed_adams_readout_f32'][1]
    assert len(dec) == len(plain) + 3 and dec[:16] == plain[:16] and dec[19:] == plain[16:]
    step = _lib.SIGNATURES['ndcn_ab_step_readout_f32'][1]
    assert len(step) == 14
    m = re.search(r'#define\s+NDCN_READOUT_ADAMS\s+\(1 << 4\)', text)
    assert m and _lib.READOUT_ADAMS == 16
    assert _lib.READOUT_ADAMS & (_lib.READOUT_FUSED | _lib.READOUT_STAGED | _lib.READOUT_FIXED | _lib.READOUT_NARROW) == 0


def test_library_exports_the_three_calls():
    import subprocess
    from ndcn_amd import _lib
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(NEW_CALLS) <= set(re.findall(r' T (ndcn_\w+)', out))


# (H, C, weight_ok, needs_grad, enabled) -> does the solve take the decoder?
ROUTE_TABLE = [
    ((20, 1, True, False, True), True), ((16, 15, True, False, True), True), ((60, 1, True, False, True), True),
    ((64, 1, True, False, True), True), ((68, 4, True, False, True), True), ((512, 15, True, False, True), True),
    ((12, 1, True, False, True), False), ((18, 1, True, False, True), False), ((22, 1, True, False, True), False),
    ((62, 1, True, False, True), False), ((63, 1, True, False, True), False), ((513, 1, True, False, True), False),
    ((24, 16, True, False, True), False), ((24, 0, True, False, True), False), ((256, 16, True, False, True), False),
    ((20, 1, False, False, True), False),                  # not a float32 device (C, H) tensor
    ((20, 1, True, True, False), False), ((20, 1, True, True, True), False),      # a gradient asked of the decoder
    ((20, 1, True, False, False), False), ((256, 1, True, False, False), False),  # NDCN_ADAMS_READOUT=0
]


def test_routing_predicate_against_the_table():
    from ndcn_amd import hip
    for args, want in ROUTE_TABLE:
        assert hip.adams_readout_route(*args) is want, args
    # every width: exactly the two sets of ndcn_ab_step_readout_f32
    for H in range(1, 600):
        want = (64 <= H <= 512) or (16 <= H <= 60 and H % 4 == 0)
        assert hip.adams_readout_route(H, 1) is want, H


def test_the_switch_reads_the_environment_and_the_override(monkeypatch):
    from ndcn_amd import hip
    monkeypatch.delenv('NDCN_ADAMS_READOUT', raising=False)
    assert hip.set_adams_readout(-1) in (0, 1) and hip.adams_readout_on() == 1     # on by default
    monkeypatch.setenv('NDCN_ADAMS_READOUT', '0')
    assert hip.adams_readout_on() == 0
    assert hip.set_adams_readout(1) == 0 and hip.adams_readout_on() == 1           # the override wins; the previous mode is returned
    assert hip.set_adams_readout(-1) == 1 and hip.adams_readout_on() == 0
    monkeypatch.delenv('NDCN_ADAMS_READOUT')
    assert hip.adams_readout_on() == 1


def _case(H, rows=9, C=3, n=5, seed=0):
    g = np.random.default_rng(seed + H)
    y = (g.random((rows, H)) - .5).astype(np.float32)
    fs = [(g.random((rows, H)) - .5).astype(np.float32) for _ in range(n)]
    Wd = ((g.random((C, H)) - .5) * 2 / np.sqrt(H)).astype(np.float32)
    bd = (g.random(C) - .5).astype(np.float32)
    return y, fs, ab.weights(n), np.float32(.1), Wd, bd


def test_oracle_of_one_step_and_decode():
    """H = 20 (one in-order chain) and H = 68 (64 lane chains of <= 2 elements, butterfly): the composed oracle stays within the fp32
    bound of the float64 value - (H + 1) u of the sum of magnitudes covers every order - and is NOT the other route's order, so a
    kernel on the wrong layout is caught; an inside tick turns -0 into +0 and Inf into NaN before the decoder, the state keeps both."""
    for H in (20, 68):
        y, fs, a, dt, Wd, bd = _case(H)
        state, dec = aro.step_readout(y, fs, a, dt, Wd, bd)
        assert np.array_equal(state.view(np.int32), ab.ab_step(y, fs, a, dt).view(np.int32))
        exact = state.astype(np.float64) @ Wd.astype(np.float64).T + bd.astype(np.float64)
        mag = np.abs(state).astype(np.float64) @ np.abs(Wd).astype(np.float64).T + np.abs(bd).astype(np.float64)
        assert np.all(np.abs(dec.astype(np.float64) - exact) <= (H + 1) * 2.0 ** -24 * mag)
        other = (aro.decode_rowdot if H < 64 else aro.decode_small)(state, Wd, bd)
        assert not np.array_equal(other.view(np.int32), dec.view(np.int32))
        # emit_off: the value of the expression does not depend on the offset; finite values other than -0 pass unchanged
        _, dec_in = aro.step_readout(y, fs, a, dt, Wd, bd, emit_off=.03)
        assert np.array_equal(dec_in.view(np.int32), dec.view(np.int32))
    y, fs, a, dt, Wd, bd = _case(20)
    y[0], y[1] = 0., 0.
    for f in fs:
        f[0], f[1] = 0., 0.
    y[0, 0] = -0.
    fs[0][0, 0] = -1.4e-45                       # a0 * f0 = -2.8e-45, times dt: underflows to -0.0
    y[1, 19] = np.inf
    state, dec = aro.step_readout(y, fs, a, dt, Wd, bd)
    _, dec_in = aro.step_readout(y, fs, a, dt, Wd, bd, emit_off=.03)
    assert state[0, 0] == 0 and np.signbit(state[0, 0]) and state[1, 19] == np.inf
    assert np.all(np.isinf(dec[1])) and np.all(np.isnan(dec_in[1]))
    assert np.array_equal(dec_in[0].view(np.int32), dec[0].view(np.int32))           # (+0 and -0 decode alike from an accumulator at +0)
    assert np.array_equal(aro.emit(state, dt, .03)[0].view(np.int32), np.zeros(20, np.int32))
