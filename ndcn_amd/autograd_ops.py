"""Differentiable wrappers of the HIP ops: backward of the path.

The reference trains by plain autograd THROUGH every solver op (heat_dynamics.py:333; no adjoint).  Here
each forward is the same HIP kernel the inference path uses; the backward of the two heavy ops runs on
HIP kernels too (g_X = A^T g through the SpMM on the transposed CSR, g_S = g W through the MFMA Linear);
the weight gradient g^T S as a split-row fp32-MFMA kernel with the ReLU mask and the bias gradient fused in
(csrc/linear_bwd.hip)), and the per-term scalings of the Runge-Kutta algebra are one streaming HIP kernel each.

dopri5: the reference differentiates through its step-size controller too; that chain lives in
ndcn_amd/torchdiffeq/_impl/autograd_path.py.  The wrappers below serve the right-hand side and the fixed-grid
solvers, whose step sizes are data-independent.
"""
import numpy as np
import torch

from . import _lib
from . import dropout as _dropout
from .csr import as_csr
from .ops import hip


class _Spmm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, X, A):
        ctx.A = A
        return hip.spmm(A, X.detach())

    @staticmethod
    def backward(ctx, g):
        return hip.spmm(ctx.A.transpose(), g.contiguous()), None


class _Linear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, S, W, b):
        ctx.save_for_backward(S, W)
        ctx.has_b = b is not None
        return hip.linear(S.detach(), W.detach(), None if b is None else b.detach())

    @staticmethod
    def backward(ctx, g):
        S, W = ctx.saved_tensors
        return hip.linear_bwd(g.contiguous(), W.detach(), S=S.detach(), need_gS=ctx.needs_input_grad[0],
                              need_gW=ctx.needs_input_grad[1], need_gb=ctx.has_b and ctx.needs_input_grad[2])


class _Rhs(torch.autograd.Function):
    """relu(dropout(W (A X) + b)) with the fused forward; S = A X is recomputed in the backward instead of stored.  With an active
    dropout the saved output is the masked K' = relu(z) * m, and that is all the backward needs (rhs_vjp)."""

    @staticmethod
    def forward(ctx, X, W, b, A, no_graph, no_control, dropout=None):
        # (W itself, not a detached alias: the packed-weight cache of ops.rhs is keyed on the tensor object and its version
        # counter - every evaluation of a solve then reuses the packed image instead of rebuilding it: two launches per RHS)
        Y = hip.rhs(A, X.detach(), W, None if b is None else b.detach(), no_graph=no_graph, no_control=no_control, dropout=dropout)
        ctx.A, ctx.no_graph, ctx.no_control, ctx.has_b = A, no_graph, no_control, b is not None
        ctx.scale = 1.0 if dropout is None else _dropout.scale(dropout[0])
        ctx.save_for_backward(X, W, Y)
        return Y

    @staticmethod
    def backward(ctx, g):
        X, W, Y = ctx.saved_tensors
        gX, gW, gb = rhs_vjp(ctx.A, ctx.no_graph, ctx.no_control, X, W, Y, g.contiguous(), ctx.needs_input_grad[0],
                             ctx.needs_input_grad[1], ctx.has_b and ctx.needs_input_grad[2], scale=ctx.scale)
        return gX, gW, gb, None, None, None, None


def rhs_vjp(A, no_graph, no_control, X, W, Y, g, need_x, need_w, need_b, S=None, scale=1.0):
    """(g_X, g_W, g_b) of Y = relu(W (A X) + b) for the upstream gradient g - the closed form every differentiable wrapper of the
    right-hand side shares: ReLU mask fused into the operand loads of the two GEMMs, g_W = gZ^T S split over row chunks (S = A X
    recomputed instead of stored, unless the caller kept the one the forward launch wrote), g_b with it, g_X = A^T g_S through the
    SpMM on the transposed CSR.
    scale: Y is the dropout-masked K' = relu(z) * m with m in {0, s}, scale = s.  [K' > 0] = [z > 0 and kept], so the gradient is
    gZ = s * g * [K' > 0]: the same kernels masked by the stored K', and the scalar folded into the alpha of the transposed SpMM
    and into the two small parameter gradients - no mask is re-created, no panel pass is added while the graph is on."""
    if (need_w and not no_graph and not no_control and
            _lib.load().ndcn_rhs_mid_bwd_supported(X.shape[0], X.shape[1], _lib.F_RELU, -1)):
        # the switch is on for this shape (csrc/rhs_mid_bwd.hip): the whole reverse as one call, the same bits in three launches
        return hip.rhs_vjp(A, X.detach(), W, Y, g, S=S, need_x=need_x, need_b=need_b, acc_scale=scale)
    if (no_graph != no_control and (need_x if no_control else need_w) and hip.rhs_abl_bwd_on() and
            _lib.load().ndcn_rhs_abl_bwd_supported(X.shape[0], X.shape[1], _lib.F_RELU | (_lib.F_NO_GRAPH if no_graph else _lib.F_NO_CONTROL))):
        # an ablation under its own switch (csrc/rhs_abl_bwd.hip): the whole reverse as one call, the same bits in one or two launches
        return hip.rhs_vjp(A, X.detach(), W, Y, g, need_x=need_x, need_b=need_b, acc_scale=scale, no_graph=no_graph, no_control=no_control)
    gW = gb = None
    if not no_control:
        if not need_w:
            S = None
        elif S is None:
            S = X.detach() if no_graph else hip.spmm(A, X.detach())
        # (W itself, not a detached alias: linear_bwd keeps the packed planes of W^T per weight tensor object and version)
        gS, gW, gb = hip.linear_bwd(g, W, S=S, Y=Y, need_gS=need_x, need_gW=need_w, need_gb=need_b)
        if scale != 1.0:
            gW = gW.mul_(scale) if gW is not None else None
            gb = gb.mul_(scale) if gb is not None else None
    else:
        gS = hip.relu_bwd(g, Y) if need_x else None
    gX = None
    if need_x:
        if no_graph:
            gX = gS if scale == 1.0 else hip.scale(gS, scale)
        else:
            gX = hip.spmm(A.transpose(), gS.contiguous(), alpha=scale)
    return gX, gW, gb


def spmm(A, x):
    return _Spmm.apply(x, as_csr(A))


def linear(x, W, b):
    return _Linear.apply(x, W, b)


def rhs(A, x, W, b, no_graph, no_control, dropout=None):
    """dropout: None or (p, seed, evaluation) - see ops.HipOps.rhs"""
    return _Rhs.apply(x, W, b, None if no_graph else as_csr(A), no_graph, no_control, dropout)


class _TgcnSequence(torch.autograd.Function):
    """The teacher-forced part of TemporalGCN up to the hidden states, as one node over the input projection of all ticks and the
    recurrence (csrc/tgcn.hip): H (T, Hr) from S = A X, r = A 1 and the six parameters.  S and r are saved by reference, with the
    gate record and the hidden states; the backward is the reverse of the recurrence, then of the projection - W_ih is read once
    and its gradient written once.  The decoder stays a node of its own."""

    @staticmethod
    def forward(ctx, w, b, W_ih, W_hh, b_ih, b_hh, S, r, rnn_type):
        GI = hip.tgcn_proj(S, r, w.detach(), b.detach(), W_ih.detach(), b_ih.detach())
        H, gates, c_rec, _, _ = hip.tgcn_cell(rnn_type, GI, W_hh.detach(), b_hh.detach())
        ctx.rnn_type, ctx.S, ctx.r, ctx.gates, ctx.c_rec = rnn_type, S, r, gates, c_rec
        ctx.save_for_backward(w, b, W_ih, W_hh, H)
        return H

    @staticmethod
    def backward(ctx, gH):
        w, b, W_ih, W_hh, H = ctx.saved_tensors
        GGI, g_Whh, g_bhh, _, _ = hip.tgcn_cell_bwd(ctx.rnn_type, gH.contiguous(), ctx.gates, ctx.c_rec, H.detach(), W_hh.detach())
        g_Wih, g_w, g_b, g_bih = hip.tgcn_proj_bwd(ctx.S, ctx.r, w.detach(), b.detach(), W_ih.detach(), GGI)
        return g_w.view_as(w), g_b, g_Wih, g_Whh, g_bih, g_bhh, None, None, None


def tgcn_sequence(S, r, w, b, W_ih, W_hh, b_ih, b_hh, rnn_type):
    return _TgcnSequence.apply(w, b, W_ih, W_hh, b_ih, b_hh, S, r, rnn_type)


# ---------------------------------------------------------------------------------------------------
# Runge-Kutta algebra: linear maps whose VJP is a per-input scalar times the incoming gradient
# ---------------------------------------------------------------------------------------------------

class _LinMap(torch.autograd.Function):
    """forward = a HIP kernel given as closure; out = sum_i w_i * in_i with host-side scalar weights w."""

    @staticmethod
    def forward(ctx, fwd, weights, *inputs):
        ctx.weights = weights
        return fwd(*[t.detach() for t in inputs])

    @staticmethod
    def backward(ctx, g):
        grads = []
        for need, w in zip(ctx.needs_input_grad[2:], ctx.weights):
            grads.append(hip.scale(g, w) if (need and w != 0) else (torch.zeros_like(g) if need else None))
        return (None, None) + tuple(grads)


class _TickEmit(torch.autograd.Function):
    """forward = ndcn_tick_emit_f32 (one pass, all ticks of the step); backward = the sum of the ticks' gradients (identity VJP each)"""

    @staticmethod
    def forward(ctx, y, dt, tms):
        return tuple(hip.tick_emit(y.detach(), dt, tms))

    @staticmethod
    def backward(ctx, *gs):
        gs = [g.contiguous() for g in gs]
        g = gs[0] if len(gs) == 1 else hip.lincomb(gs, [1.0] * len(gs))
        return g, None, None


# fixed_stage op -> weights of (y, k1, k2, k3, k4) as functions of dt (the formulas in include/ndcn_hip.h)
_STAGE_W = {
    0: lambda dt: (1, dt),
    1: lambda dt: (1, dt / 2),
    2: lambda dt: (1, dt / 3),
    3: lambda dt: (1, -dt / 3, dt),
    4: lambda dt: (1, dt, -dt, dt),
    5: lambda dt: (1, dt / 8, 3 * dt / 8, 3 * dt / 8, dt / 8),
}


class AutogradOps:
    """Same interface as ndcn_amd.ops.HipOps; every panel op is differentiable."""

    name = 'hip+autograd'

    @staticmethod
    def combine(y0, ks, cs):
        w = (1.0,) + tuple(float(c) for c in cs)
        return _LinMap.apply(lambda y, *k: hip.combine(y, list(k), cs), w, y0, *ks)

    @staticmethod
    def scale(x, w):
        return _LinMap.apply(lambda xx: hip.scale(xx, w), (float(w),), x)

    @staticmethod
    def fixed_stage(op, y, k1, k2=None, k3=None, k4=None, dt=0.0, out=None):
        w = _STAGE_W[op](float(dt))
        ins = [t for t in (y, k1, k2, k3, k4) if t is not None][:len(w)]
        return _LinMap.apply(lambda yy, *k: hip.fixed_stage(op, yy, *k, dt=dt), w, *ins)

    @staticmethod
    def ab_step(y, fs, coeffs, dt, out=None):
        w = (1.0,) + tuple(float(dt) * float(a) for a in coeffs)
        return _LinMap.apply(lambda yy, *f: hip.ab_step(yy, list(f), coeffs, dt), w, y, *fs)

    @staticmethod
    def abm_predict(y, fs, a, m, dt):
        # the three panels of ndcn_abm_predict_f32 as linear maps of (y, f_0, ..): the bits of the kernel (one pass each under a
        # gradient: every output is its own node)
        n = len(fs)
        pick = lambda q: (lambda yy, *f: hip.abm_predict(yy, list(f), a, m, dt)[q])
        wa = tuple(float(dt) * float(c) for c in a)
        wm = tuple(float(dt) * float(c) for c in m)
        dy = _LinMap.apply(pick(0), (0.0,) + wa, y, *fs)
        delta = _LinMap.apply(pick(1), (0.0,) + wm, y, *fs)
        u = _LinMap.apply(pick(2), (1.0,) + wa, y, *fs)
        return dy, delta, u

    @staticmethod
    def abm_correct(f, delta, y, dy, c0, rtol, atol):
        # the count comes from the kernel on detached tensors (on a copy of dy: the graph keeps the old one); the values are composed
        # from the differentiable maps - c0 * f + delta and y + dy', the kernel's own roundings - so the iteration count is a constant
        # of the graph
        _, _, failed = hip.abm_correct(f.detach(), delta.detach(), y.detach(), dy.detach().clone(), c0, rtol, atol)
        new = _LinMap.apply(lambda dl, ff: hip.combine(dl, [ff], [c0]), (1.0, float(c0)), delta, f)
        u = _LinMap.apply(lambda yy, dd: hip.combine(yy, [dd], [np.float32(1)]), (1.0, 1.0), y, new)
        return new, u, failed

    @staticmethod
    def tick_emit(y, dt, tms, outs=None):
        # y + ((y - y) / dt) * tm: the derivative with respect to y is 1 wherever the state is finite (the slope term is a constant
        # zero there), so every tick hands its gradient to the state that ended the step, unchanged
        return list(_TickEmit.apply(y, dt, tuple(tms)))

    @staticmethod
    def error(y0, y1, ks, cs, rtol, atol):
        return hip.error(y0.detach(), y1.detach(), [k.detach() for k in ks], cs, rtol, atol)

    @staticmethod
    def scaled_sumsq(a, b, y, rtol, atol):
        return hip.scaled_sumsq(a.detach(), None if b is None else b.detach(), y.detach(), rtol, atol)

    @staticmethod
    def interp_fit(y0, y1, ks, cmid, dt):
        with torch.no_grad():
            abcd = hip.interp_fit(y0.detach(), y1.detach(), [k.detach() for k in ks], cmid, dt)
        return {'abcd': abcd, 'y0': y0, 'y1': y1, 'ks': list(ks), 'cmid': [float(c) for c in cmid], 'dt': float(dt)}

    @staticmethod
    def interp_eval(fit, e, xpow, out=None):
        x4, x3, x2, x1, _ = [float(v) for v in xpow]
        dt = fit['dt']
        w_f0 = dt * (-2 * x4 + 5 * x3 - 4 * x2 + x1)
        w_f1 = dt * (2 * x4 - 3 * x3 + x2)
        w_y0 = -8 * x4 + 18 * x3 - 11 * x2 + 1
        w_y1 = -8 * x4 + 14 * x3 - 5 * x2
        w_ym = 16 * x4 - 32 * x3 + 16 * x2
        wk = [w_ym * c for c in fit['cmid']]
        wk[0] += w_f0
        wk[-1] += w_f1
        weights = (w_y0 + w_ym, w_y1) + tuple(wk)
        abcd = fit['abcd']
        return _LinMap.apply(lambda y0, y1, *k: hip.interp_eval(abcd, y0, xpow), weights, fit['y0'], fit['y1'], *fit['ks'])

    # row-local pieces used by sharded / custom funcs
    spmm = staticmethod(lambda A, X, X_halo=None, alpha=1.0, relu=False, out=None: spmm(A, X))
    linear = staticmethod(lambda S, W, b=None, relu=False: linear(S, W, b))


autograd_ops = AutogradOps()
