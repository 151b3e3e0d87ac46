"""ndcn_ab_step_readout_f32's order of operations restated in numpy by composing the existing restatements: the step is
tests/_adams_bashforth.ab_step, the tick of a sub-stepped grid the reference's y1 + ((y1 - y1) / dt) * off, and the decoder's fma
chains are tests/_readout_chain.tick_gradient - a sequential fp32 fma chain from +0 over the rows of its second argument - on the
element order of the decoder's two routes:
  H < 64    one chain over k = 0 .. H - 1 per (row, output), then the bias (ndcn_linear_f32's small route);
  H >= 64   lane l of 64 chains the elements l, l + 64, .. (a lane without an element contributes fma(0, w, acc) = acc), the 64
            partial sums are folded by the xor butterfly 32, 16, .. 1 - every sum rounded to fp32 -, lane 0 adds the bias.
Independent of the package."""
import numpy as np

import _adams_bashforth as ab
import _readout_chain as rc

f32 = np.float32


def emit(y, dt, off):
    with np.errstate(all='ignore'):
        y = np.asarray(y, f32)
        return (y + (((y - y).astype(f32) / f32(dt)).astype(f32) * f32(off)).astype(f32)).astype(f32)


def decode_small(s, Wd, bd=None):
    out = rc.tick_gradient(s, np.asarray(Wd, f32).T)             # acc[n, o] = chain over k of s[n, k] * Wd[o, k]
    with np.errstate(all='ignore'):
        return out if bd is None else (out + np.asarray(bd, f32)[None, :]).astype(f32)


def decode_rowdot(s, Wd, bd=None):
    s, Wd = np.asarray(s, f32), np.asarray(Wd, f32)
    n, H = s.shape
    nv = (H + 63) // 64
    sp = np.zeros((n, nv * 64), f32)
    sp[:, :H] = s
    lanes = np.arange(64)
    out = np.empty((n, Wd.shape[0]), f32)
    for o in range(Wd.shape[0]):
        wp = np.full(nv * 64, Wd[o, H - 1], f32)
        wp[:H] = Wd[o]
        # per lane: the chain over v - tick_gradient over the lane's own elements, all 64 lanes side by side
        acc = np.stack([rc.tick_gradient(sp[:, l::64], wp[l::64][:, None])[:, 0] for l in lanes], axis=1)
        with np.errstate(all='ignore'):
            for off in (32, 16, 8, 4, 2, 1):
                acc = (acc + acc[:, lanes ^ off]).astype(f32)
        out[:, o] = acc[:, 0]
    with np.errstate(all='ignore'):
        return out if bd is None else (out + np.asarray(bd, f32)[None, :]).astype(f32)


def step_readout(y, fs, a, dt, Wd, bd=None, emit_off=0.0):
    """(new state, decoded) of one launch"""
    y1 = ab.ab_step(y, fs, a, dt)
    s = emit(y1, dt, emit_off) if emit_off != 0 else y1
    H = y1.shape[1]
    return y1, (decode_small if H < 64 else decode_rowdot)(s, Wd, bd)
