"""Training through a fixed-grid solve (euler / midpoint / rk4 / explicit_adams) over ODEFunc: the routes of `odeint` under a gradient and their
autograd nodes, one per route, each differentiated the way the reference's drivers train - plain backpropagation through every step
(heat_dynamics.py:313-334).

  _SmallEulerSolve   a state that fits one compute unit: the whole solve and its reverse sweep, one launch each (csrc/solve_small.hip);
  _NativeFixedGrid   any size: the loops inside the library, two calls per solve (csrc/tape.hip: ndcn_fixed_grid_train_f32 /
                     ndcn_fixed_grid_backward[_readout]_f32);
  _FixedGridSolve    the same launches issued from Python, one step per tick: the A/B partner of the native loops
                     (NDCN_FIXED_GRID_NATIVE=0) and the form that carries an active dropout;
  _SubstepSolve      options={'step_size': h}: a grid finer than the ticks, checkpointed per tick interval;
  _ExplicitAdamsSolve  method='explicit_adams' (NDCN_ADAMS_TRAIN=1): the library's loop forward with a record of every evaluation, the
                     reverse sweep of a multistep method in closed form (csrc/adams.hip, csrc/adams_bwd.hip);
  _FixedAdamsSolve   method='fixed_adams' (the same switch): that loop with the Adams-Moulton corrector, a record of every corrector
                     evaluation too, the reverse of a predictor-corrector step in closed form.

Which solves the two Adams nodes take is decided in one place, with the solve without a gradient: _adams_admission, plus the nodes'
own declines in _adams_with_grad.

The last five take the decoder of odeint's `readout` as an optional input (Wd, bd; None without one).  With it the node's output is
the decoded solution (T, N, C) - hip.linear of the trajectory, the bits of the two-step form - the hidden trajectory is saved for the
reverse sweep only, and that sweep takes the (T, N, C) gradient as it is: the (T, N, H) gradient of the trajectory is never written.
Where a tick's gradient comes from is one object in the two Python sweeps (_PlainTicks, _ReadoutTicks: the Python mirror of TickGrad
in csrc/tape.hip) and the `decoder` argument of _fixed_grid_reverse in the native one.

Why _FixedGridSolve and _SubstepSolve stay two nodes.  A tick-per-step grid is a step_size plan whose every step reports one coincident
tick, and the forward launches of the two are indeed the same; the reverse sweeps are not.  The per-tick sweep adds the entering tick
gradient INSIDE the step's closing combination: combine_kernel and readout_bwd_kernel form a + ((((0 + gu_0) + gu_1) + ...) + g_i),
the sum started from +0 and the base added last ("The decoder inside the fixed-grid reverse sweep").  The step_size sweep
closes the step first and adds the tick gradients in a pass of their own: (a + sum gu) + sum g.  Those are different roundings, and
the second form costs one more launch per step, so one merged sweep would change either the bits of one path or the launch count of
the other.  They share the step launches, the closed-form sweep of one step and the tick-gradient objects, nothing more.

Nothing here imports odeint.py at module level (it routes into this module)."""
import ctypes
import sys

import torch
from torch.autograd.function import once_differentiable

from ... import _lib
from ... import dropout as _dropout
from ..._lib import check, ptr, stream_ptr
from ...ops import hip
from . import core
from .tape import Tape

EVALS = {'euler': 1, 'midpoint': 2, 'rk4': 4}             # right-hand-side evaluations per step


# ---- the repeated lines, once each ---------------------------------------------------------------------------------------------

def _view(csr, n_rows, **kw):
    """the library's view of the operator, or of the empty stand-in where there is none (no_graph: only n_rows is read)"""
    return csr.view_ref(**kw) if csr is not None else ctypes.byref(_lib.empty_csr(n_rows))


def _detached(*tensors):
    """what the library reads of each: detached and contiguous (None stays None)"""
    return tuple(None if x is None else x.detach().contiguous() for x in tensors)


def _finish(scratch, rc):
    """the tail of a library call that allocated through `scratch` (a Tape): the blocks go back (stream-ordered), what the allocator
    callback caught is raised in preference to the return code it caused"""
    err = scratch.error
    scratch.close()
    if rc < 0:
        if err is not None:
            raise err
        check(rc)


def _small_operator(odefunc, y0):
    """(csr or None, ctypes view ref, flags) of an ODEFunc for the library's whole-solve entry points, or None when the operator
    does not live with the state."""
    from ...csr import as_csr
    flags = _lib.operator_flags(odefunc)
    if odefunc.no_graph:
        return None, ctypes.byref(_lib.empty_csr(y0.shape[0])), flags
    csr = as_csr(odefunc.A)
    if csr.device != y0.device or csr.shape[0] != y0.shape[0]:
        return None
    return csr, csr.view_ref(), flags


def _drop_at(drop, method, step):
    """the (p, seed, evaluation) of the first evaluation of grid step `step`"""
    return None if drop is None else (drop[0], drop[1], drop[2] + step * EVALS[method])


# ---------------------------------------------------------------------------------------------------
# a state that fits one compute unit: the whole solve and its reverse sweep, one launch each
# ---------------------------------------------------------------------------------------------------

class _SmallEulerSolve(torch.autograd.Function):
    """FixedGridODESolver.integrate with Euler (and, round 5, midpoint / RK4 3-8) steps (solvers.py:79-99, fixed_grid.py:7-29,
    rk_common.py:72-78) over ODEFunc with ndcn_solve_small_f32 / ndcn_solve_small_bwd_f32 (csrc/solve_small.hip): the forward's
    trajectory IS the saved state."""

    @staticmethod
    def forward(ctx, y0, W, b, csr, flags, dts, method='euler'):
        lib = _lib.load()
        n_ticks = len(dts)
        H = y0.shape[1]
        ctx.method = _lib.METHODS[method]
        out = torch.empty((n_ticks + 1,) + tuple(y0.shape), dtype=torch.float32, device=y0.device)
        out[0].copy_(y0)
        arr = (ctypes.c_float * n_ticks)(*dts)
        if flags & _lib.F_NO_CONTROL:
            W = b = None
        Wd, bd = _detached(W, b)
        view = _view(csr, y0.shape[0], need_symmetric=True)
        # Euler on the README shapes: the forward launch keeps S_i = A y_i and K_i of every step for the reverse sweep (two panels per
        # tick instead of a gather and a Linear per tick in backward: ndcn_solve_small_keep_*)
        keep = None
        if ctx.method == _lib.M_EULER and csr is not None and Wd is not None and lib.ndcn_solve_small_keep_supported(view, H, flags):
            keep = torch.empty((n_ticks, 2) + tuple(y0.shape), dtype=torch.float32, device=y0.device)
        with torch.cuda.device(y0.device):
            if keep is not None:
                check(lib.ndcn_solve_small_keep_f32(view, ptr(Wd), ptr(bd), H, flags, ptr(out[0]), arr, n_ticks, ptr(out[1:]), ptr(keep),
                                                    stream_ptr()))
            else:
                check(lib.ndcn_solve_small_f32(view, ptr(Wd), ptr(bd), H, flags, ctx.method, ptr(out[0]), arr, n_ticks, ptr(out[1:]),
                                               stream_ptr()))
        ctx.csr, ctx.flags, ctx.dts, ctx.keep = csr, flags, arr, keep
        # (W and b through save_for_backward: an in-place parameter change between forward and backward raises, as it does for
        # every other autograd node, instead of differentiating the wrong weights)
        ctx.save_for_backward(out, W, b)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        out, W, b = ctx.saved_tensors
        lib = _lib.load()
        Wd, bd = _detached(W, b)
        H = out.shape[2]
        g = g.contiguous()
        g_y0 = torch.empty_like(out[0])
        g_W = torch.empty((H, H), dtype=torch.float32, device=out.device) if Wd is not None else None
        g_b = torch.empty((H,), dtype=torch.float32, device=out.device) if Wd is not None else None
        csr = ctx.csr
        view = _view(csr, out.shape[1], need_symmetric=True)
        view_t = csr.transpose().view_ref() if csr is not None else view
        with torch.cuda.device(out.device):
            if ctx.keep is not None:
                check(lib.ndcn_solve_small_bwd_keep_f32(view, view_t, ptr(Wd), ptr(bd), H, ctx.flags, ptr(out), ptr(g), ctx.dts, len(ctx.dts),
                                                        ptr(ctx.keep), ptr(g_y0), ptr(g_W), ptr(g_b), stream_ptr()))
                ctx.keep = None
            else:
                check(lib.ndcn_solve_small_bwd_f32(view, view_t, ptr(Wd), ptr(bd), H, ctx.flags, ctx.method, ptr(out), ptr(g), ctx.dts,
                                                   len(ctx.dts), ptr(g_y0), ptr(g_W), ptr(g_b), stream_ptr()))
        return g_y0, g_W, (g_b if bd is not None else None), None, None, None, None


# ---------------------------------------------------------------------------------------------------
# any size, from Python: fused launches forward, closed-form sweep backward
# ---------------------------------------------------------------------------------------------------

def _step(csr, y, W, b, no_graph, no_control, method, dt, out_y, keep=None, drop=None):
    """one step by fused launches; keep (a list) receives [(stage input, K), ...] for the reverse sweep; drop: the dropout triple
    of the step's first evaluation (the following ones count on from it)"""
    kw = dict(no_graph=no_graph, no_control=no_control)
    ev = lambda j: {} if drop is None else {'dropout': (drop[0], drop[1], drop[2] + j)}
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))
    if method == 'euler':
        K, _ = hip.rhs_rk(csr, y, W, b, 'combine', y, [], [dt], out_y=out_y, **kw, **ev(0))              # y + dt k1
        stages = [(y, K)]
    elif method == 'midpoint':
        K1, ym = hip.rhs_rk(csr, y, W, b, 'combine', y, [], [f32(dt / 2.0)], **kw, **ev(0))             # y + k1 dt / 2 (an exact halving)
        K2, _ = hip.rhs_rk(csr, ym, W, b, 'combine', y, [], [dt], out_y=out_y, **kw, **ev(1))           # y + dt k2
        stages = [(y, K1), (ym, K2)]
    else:
        stages, x, ks = [], y, []
        for i in range(4):
            K, nxt = hip.rhs_rk(csr, x, W, b, 'rk4', y, ks, [dt], out_y=out_y if i == 3 else None, **kw, **ev(i))
            stages.append((x, K))
            ks = ks + [K]
            x = nxt
    if keep is not None:
        keep.extend(stages)


def _vjp(csr, u, K, g, W, b, no_graph, no_control, alpha):
    """alpha * J(u)^T g for K = relu(W (A u) + b): (g_u, g_W, g_b) with g_W / g_b UNSCALED (the caller scales the small ones)"""
    gW = gb = None
    if no_control:
        gS = hip.relu_bwd(g, K)
    else:
        S = u if no_graph else hip.spmm(csr, u)
        gS, gW, gb = hip.linear_bwd(g, W, S=S, Y=K)
    gu = hip.scale(gS, alpha) if no_graph else hip.spmm(csr.transpose(), gS, alpha=alpha)
    return gu, gW, gb


def _sweep_totals(out, csr, W, b, no_graph, no_control, drop):
    """(gW_tot, gb_tot, vj, acc): the zeroed parameter gradients of a reverse sweep (None under no_control) and the two closures of
    _sweep_step that fill them.  With dropout K is the masked K' = relu(z) * m, m in {0, s}: J^T g = s * (the p = 0 closed form masked
    by K'), so s multiplies the alpha of the transposed SpMM and the scale of the parameter gradients"""
    H = out.shape[2]
    gW_tot = torch.zeros((H, H), dtype=torch.float32, device=out.device) if not no_control else None
    gb_tot = torch.zeros((H,), dtype=torch.float32, device=out.device) if not no_control else None
    s = 1.0 if drop is None else _dropout.scale(drop[0])
    vj = lambda u, K, gk, alpha: _vjp(csr, u, K, gk, W, b, no_graph, no_control, alpha * s)
    if (no_graph != no_control and hip.rhs_abl_bwd_on() and _lib.load().ndcn_rhs_abl_bwd_supported(
            out.shape[1], H, _lib.F_RELU | (_lib.F_NO_GRAPH if no_graph else _lib.F_NO_CONTROL))):
        # an ablation under hip.set_rhs_abl_bwd (csrc/rhs_abl_bwd.hip): the evaluation's reverse as ONE call, which also accumulates
        # g_W / g_b with the scale acc() would apply - _sweep_step hands acc the alpha it handed vj - so acc receives None
        vj = lambda u, K, gk, alpha: (hip.rhs_vjp(csr, u, W, K, gk, acc_scale=alpha * s, gW=gW_tot, gb=gb_tot, no_graph=no_graph,
                                                  no_control=no_control)[0], None, None)

    def acc(gW, gb, scale):
        if gW is not None:
            gW_tot.add_(gW, alpha=scale * s)
            gb_tot.add_(gb, alpha=scale * s)
    return gW_tot, gb_tot, vj, acc


def _sweep_step(method, dt, st, a, vj, acc, close, gk1_extra=None):
    """the adjoint before one step from the adjoint `a` after it: st = the step's [(stage input, K), ...], vj / acc as _sweep_totals
    makes them; close(a, [gu, ...]) is the step's last pass, a + the sum of the stages' gu (+ whatever enters at the state the step
    starts from: the per-tick sweep adds that tick's gradient in the same pass).  gk1_extra (rk4 only): one more addend of the gradient
    of k1, last in its sum - the RK4 warm-up step of explicit_adams, whose k1 is also a history term of later steps"""
    if method == 'euler':                                   # y1 = y + dt k1
        (u1, K1), = st
        gu1, gW, gb = vj(u1, K1, a, dt)
        acc(gW, gb, dt)
        return close(a, [gu1])
    if method == 'midpoint':                                # ym = y + (dt / 2) k1 ; y1 = y + dt k2
        (u1, K1), (u2, K2) = st
        gu2, gW, gb = vj(u2, K2, a, dt)                     # dL/d ym
        acc(gW, gb, dt)
        gu1, gW, gb = vj(u1, K1, gu2, dt / 2.0)
        acc(gW, gb, dt / 2.0)
        return close(a, [gu2, gu1])
    (u1, K1), (u2, K2), (u3, K3), (u4, K4) = st             # the 3/8 rule, rk_common.py:72-78
    c8 = dt / 8.0
    gu4, gW, gb = vj(u4, K4, a, c8)                         # J4^T (c8 a)
    acc(gW, gb, c8)
    gk3 = hip.lincomb([a, gu4], [3.0 * c8, dt])
    gu3, gW, gb = vj(u3, K3, gk3, 1.0)
    acc(gW, gb, 1.0)
    gk2 = hip.lincomb([a, gu4, gu3], [3.0 * c8, -dt, dt])
    gu2, gW, gb = vj(u2, K2, gk2, 1.0)
    acc(gW, gb, 1.0)
    more = ([gk1_extra], [1.0]) if gk1_extra is not None else ([], [])
    gk1 = hip.lincomb([a, gu4, gu3, gu2] + more[0], [c8, dt, -dt / 3.0, dt / 3.0] + more[1])
    gu1, gW, gb = vj(u1, K1, gk1, 1.0)
    acc(gW, gb, 1.0)
    return close(a, [gu4, gu3, gu2, gu1])


def _sum_onto(a, panels):
    """a + the panels, left to right from +0, in one pass"""
    return hip.lincomb(panels, [1.0] * len(panels), y0=a)


class _PlainTicks:
    """Where the reverse sweeps take the gradient of tick j from - without a decoder: the panel g[j] of the trajectory's gradient."""

    def __init__(self, g):
        self.g = g

    def seed(self, j):
        """the adjoint at the last tick"""
        return self.g[j]

    def close(self, a, gus, j):
        """the closing combination of the step that starts at tick j, the tick's gradient inside the same pass"""
        return _sum_onto(a, gus + [self.g[j]])

    def enter(self, a, ticks):
        """the step_size sweep: the adjoint `a` (None: nothing yet) plus the gradients of the ticks reported at this state"""
        gs = [self.g[j] for j in ticks]
        if a is None:
            a, gs = gs[0], gs[1:]
        for q in range(0, len(gs), 8):
            a = _sum_onto(a, gs[q:q + 8])
        return a

    def decoder_grads(self):
        return None, None


class _ReadoutTicks:
    """With the decoder inside the node: g is the gradient of the DECODED ticks (T, N, C), and tick j's g[j] . Wd is formed inside the
    pass that adds it (hip.readout_bwd), which also accumulates the decoder's own gradients from the stored state out[j] in fp64 (when
    either is wanted) - rounded to float32 once, after the last tick."""

    def __init__(self, g, out, Wd, needs_W, needs_b):
        C, H = Wd.shape
        self.g, self.out, self.Wd, self.needs = g, out, Wd, (needs_W, needs_b)
        self.acc = torch.zeros(C * H + C, dtype=torch.float64, device=Wd.device) if (needs_W or needs_b) else None

    def seed(self, j):
        return hip.readout_bwd(self.g[j], self.Wd, y=self.out[j], acc=self.acc)

    def close(self, a, gus, j):
        return hip.readout_bwd(self.g[j], self.Wd, y=self.out[j], base=a, addends=gus, acc=self.acc)

    def enter(self, a, ticks):
        """one call per tick (an interval's last step may report several)"""
        for j in ticks:
            a = hip.readout_bwd(self.g[j], self.Wd, y=self.out[j], base=a, acc=self.acc)
        return a

    def decoder_grads(self):
        if self.acc is None:
            return None, None
        C, H = self.Wd.shape
        f = self.acc.to(torch.float32)
        return (f[:C * H].view(C, H) if self.needs[0] else None), (f[C * H:] if self.needs[1] else None)


def _ticks(ctx, g, out, Wd):
    """the tick-gradient source of a node's backward: Wd (input 3, bd input 4) is None without a decoder"""
    if Wd is None:
        return _PlainTicks(g.contiguous())
    return _ReadoutTicks(g.contiguous(), out, Wd, ctx.needs_input_grad[3], ctx.needs_input_grad[4])


class _FixedGridSolve(torch.autograd.Function):
    """FixedGridODESolver.integrate (solvers.py:79-99) over ODEFunc at ANY size on the kernels of the inference path:
      forward   the launches of the device-resident solver - the stage algebra of every step rides in the epilogues of its
                right-hand-side launches (ndcn_rhs_rk_f32: Euler / midpoint 1 launch per evaluation, RK4 4 per step); only the
                trajectory is kept;
      backward  per step, in reverse: the stages are re-formed from the stored state by the same launches (checkpointing: the
                reference's autograd keeps every stage of every step), then the step's vector-Jacobian products in closed
                form - SpMM, the masked Linear backward (g_S, g_W, g_b in one call), SpMM with A^T with the step size folded
                into its alpha - and the stage recurrences as one linear-combination launch each.
    No autograd graph per operation: the torch `add` / `mul` launches between the kernels are gone (they were 17 % of the
    kernel time of a 100k-node Euler training step).
    Active dropout (drop = (p, seed, first evaluation number of the solve)): evaluation e of the solve - EVALS[method] per step, in the
    solver's order - runs with the mask of (seed, first + e) in its launch; the reverse pass re-forms the stages with the same
    numbers, so the K it masks the backward kernels with are the forward's, and the scalar s = 1 / (1 - p) rides in the alphas."""

    @staticmethod
    def forward(ctx, y0, W, b, Wd, bd, csr, flags, method, dts, drop=None):
        n_ticks = len(dts)
        out = torch.empty((n_ticks + 1,) + tuple(y0.shape), dtype=torch.float32, device=y0.device)
        out[0].copy_(y0)
        no_graph, no_control = bool(flags & _lib.F_NO_GRAPH), bool(flags & _lib.F_NO_CONTROL)
        ctx.meta = (csr, no_graph, no_control, method, dts, drop)
        for i, dt in enumerate(dts):
            _step(csr, out[i], W, b, no_graph, no_control, method, dt, out[i + 1], drop=_drop_at(drop, method, i))
        ctx.save_for_backward(out, W, b, Wd)
        return out if Wd is None else hip.linear(out, Wd, bd)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        out, W, b, Wd = ctx.saved_tensors
        csr, no_graph, no_control, method, dts, drop = ctx.meta
        ticks = _ticks(ctx, g, out, Wd)
        a = ticks.seed(len(dts))
        gW_tot, gb_tot, vj, acc = _sweep_totals(out, csr, W, b, no_graph, no_control, drop)
        for i in range(len(dts) - 1, -1, -1):
            st = []
            _step(csr, out[i], W, b, no_graph, no_control, method, dts[i], torch.empty_like(out[0]), keep=st, drop=_drop_at(drop, method, i))
            a = _sweep_step(method, dts[i], st, a, vj, acc, lambda a, gus, i=i: ticks.close(a, gus, i))
        return (a, gW_tot, (gb_tot if b is not None else None)) + ticks.decoder_grads() + (None,) * 5


class _SubstepSolve(torch.autograd.Function):
    """_FixedGridSolve on a grid finer than the ticks (options={'step_size': h}; core.FixedPlan) WITHOUT a record per grid step:
      forward   the same fused launches, step after step; kept are the ticks and the state each tick interval starts from - the
                tick panel itself where the interval's last tick coincides with the end of its step, else one panel;
      backward  one tick interval at a time, last first: the interval is run again from its start by the same launches, this time
                keeping the stages of its steps, then swept backwards in closed form (_sweep_step).  The gradient of a tick enters
                at the end of the step that reported it (the VJP of ops.tick_emit is the identity).
    Memory: ticks + interval starts + ONE interval's stages, whatever the number of grid steps."""

    @staticmethod
    def _segments(plan):
        """[(first step, last step)]: runs of grid steps that end with a step reporting ticks"""
        segs, lo = [], 0
        for i, em in enumerate(plan.emits):
            if em:
                segs.append((lo, i))
                lo = i + 1
        return segs

    @staticmethod
    def _run(csr, y, W, b, no_graph, no_control, method, plan, lo, hi, last_out, keep=None, drop=None):
        """steps lo .. hi from the state y; the last one writes to `last_out`; keep (a list) receives each step's stages; drop: the
        solve's dropout triple - grid step i evaluates with the numbers it had in the forward pass, whenever it is run"""
        pp = [None, None]
        for i in range(lo, hi + 1):
            if i == hi:
                dst = last_out
            else:
                q = (i - lo) & 1
                if pp[q] is None or keep is not None:         # (kept stages hold on to the panels they read)
                    pp[q] = torch.empty_like(last_out)
                dst = pp[q]
            st = None if keep is None else []
            _step(csr, y, W, b, no_graph, no_control, method, float(plan.dts[i]), dst, keep=st, drop=_drop_at(drop, method, i))
            if keep is not None:
                keep.append(st)
            y = dst
        return y

    @staticmethod
    def forward(ctx, y0, W, b, Wd, bd, csr, flags, method, plan, drop=None):
        n_ticks = len(plan.t)
        out = torch.empty((n_ticks,) + tuple(y0.shape), dtype=torch.float32, device=y0.device)
        out[0].copy_(y0)
        no_graph, no_control = bool(flags & _lib.F_NO_GRAPH), bool(flags & _lib.F_NO_CONTROL)
        segs = _SubstepSolve._segments(plan)
        starts, own = [], []                 # per segment: where its first state lives - ('out', tick) or ('own', index into `own`)
        y, where = out[0], ('out', 0)
        for lo, hi in segs:
            starts.append(where)
            em = plan.emits[hi]
            j_last, same_last, _ = em[-1]
            if same_last:
                y1, where = out[j_last], ('out', j_last)
            else:
                y1 = torch.empty_like(out[0])
                own.append(y1)
                where = ('own', len(own) - 1)
            y = _SubstepSolve._run(csr, y, W, b, no_graph, no_control, method, plan, lo, hi, y1, drop=drop)
            loose = [e for e in em if not e[1]]
            for q in range(0, len(loose), core.MAX_EMIT):
                part = loose[q:q + core.MAX_EMIT]
                hip.tick_emit(y, plan.dts[hi], [e[2] for e in part], outs=[out[e[0]] for e in part])
        if own and where[0] == 'own':
            own.pop()                        # nothing starts from the state after the last step
        ctx.meta = (csr, no_graph, no_control, method, plan, segs, starts, drop)
        ctx.save_for_backward(out, W, b, Wd, *own)
        return out if Wd is None else hip.linear(out, Wd, bd)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        out, W, b, Wd, *own = ctx.saved_tensors
        csr, no_graph, no_control, method, plan, segs, starts, drop = ctx.meta
        ticks = _ticks(ctx, g, out, Wd)
        gW_tot, gb_tot, vj, acc = _sweep_totals(out, csr, W, b, no_graph, no_control, drop)
        a = None
        for (lo, hi), (kind, idx) in zip(reversed(segs), reversed(starts)):           # the tick intervals, last first
            a = ticks.enter(a, [e[0] for e in plan.emits[hi]])                        # the ticks this interval's last step reported
            y = out[idx] if kind == 'out' else own[idx]
            keep = []
            _SubstepSolve._run(csr, y, W, b, no_graph, no_control, method, plan, lo, hi, torch.empty_like(out[0]), keep=keep, drop=drop)
            for i in range(hi, lo - 1, -1):
                a = _sweep_step(method, float(plan.dts[i]), keep.pop(), a, vj, acc, _sum_onto)
        if a is None:
            a = torch.zeros_like(out[0])
        a = ticks.enter(a, [0])                                                       # the first tick is y0 itself
        return (a, gW_tot, (gb_tot if b is not None else None)) + ticks.decoder_grads() + (None,) * 5


# ---------------------------------------------------------------------------------------------------
# explicit_adams: the library's forward loop with a record, the reverse sweep of a multistep method - first what it shares with
# fixed_adams below and with the solve without a gradient (odeint._adams_solve): admission, report, record, the sweeps' tick handling
# ---------------------------------------------------------------------------------------------------

def plan_arrays(plan):
    """(dts, n_steps, tick steps, coincident flags, tick offsets, n_emit): a core.FixedPlan as the C arrays of the explicit_adams entry
    points (ndcn_solve_explicit_adams_f32, ndcn_explicit_adams_train_f32) - the ticks after the first"""
    import numpy as np
    n_ticks, n_steps = len(plan.t), len(plan.dts)
    n_emit = n_ticks - 1
    dts = (ctypes.c_float * max(n_steps, 1))(*plan.dts.tolist())
    steps = (ctypes.c_int64 * max(n_emit, 1))(*plan.tick_step[1:].tolist())
    same = (ctypes.c_int * max(n_emit, 1))(*[int(v) for v in plan.tick_coincident[1:]])
    offs = (ctypes.c_float * max(n_emit, 1))(*[float(np.float32(plan.t[j] - plan.grid[plan.tick_step[j]])) for j in range(1, n_ticks)])
    return dts, n_steps, steps, same, offs, n_emit


def _adams_admission(odefunc, y0, t, plan, max_order, corrector=None):
    """May the explicit_adams / fixed_adams solve of a plain ODEFunc run inside the library?  -> (csr, flags, plan, contiguous y0) - the
    default plan where `plan` is None - or None.  The one statement of the decline reasons, for the solve without a gradient
    (odeint._adams_solve) and the training nodes (_adams_with_grad) alike:
      * no_graph or no_control (the entry points have no such form);
      * max_order < 2 (the reference itself fails on it);
      * an operator that does not live with the state (_small_operator);
      * with corrector = (rtol, atol, max_iters, step_log), fixed_adams: a max_iters that is not an int >= 1, tolerances that are not
        plain numbers (the generic branch fails on them as the reference does).
    Every decline comes before the check of `t`: a declined solve gets the generic path's own exception."""
    if odefunc.no_graph or odefunc.no_control or max_order < 2:
        return None
    if corrector is not None:
        rtol, atol, max_iters = corrector[:3]
        if type(max_iters) is not int or max_iters < 1 or not all(isinstance(v, (int, float)) for v in (rtol, atol)):
            return None
    op = _small_operator(odefunc, y0)
    if op is None:
        return None
    csr, _, flags = op
    core.assert_increasing(t)
    if plan is None:
        plan = core.fixed_plan(core.host_grid(t).to(y0.dtype).numpy())         # solvers.py:81: the grid is t in the state dtype
    return csr, flags, plan, _lib.require_device(y0, 'state y0').contiguous()


def _report_corrector(step_log, iters, conv):
    """what a fixed_adams solve inside the library tells its caller: the reference's warning line once per step that did not converge,
    and in step_log one (corrector iterations, converged) pair per grid step - (0, True) for a warm-up step - and ('nfe', evaluations)"""
    for c in conv:
        if not c:
            print(core.NOT_CONVERGED, file=sys.stderr)            # fixed_adams.py:198
    if step_log is not None:
        warm = sum(1 for i in iters if i == 0)
        step_log.extend((int(i), bool(c)) for i, c in zip(iters, conv))
        step_log.append(('nfe', len(iters) + 3 * warm + sum(iters)))


def _adams_record(y0c, plan):
    """(out, rec_f, rec_y) of a training solve: the ticks (y0 first), f_i = F(y_i) of every grid step and the state after it"""
    shape = tuple(y0c.shape)
    new = lambda n: torch.empty((n,) + shape, dtype=torch.float32, device=y0c.device)
    out = new(len(plan.t))
    out[0].copy_(y0c)
    # the default grid: step i reports tick i + 1 and nothing else, the state after it - no state is stored twice
    return out, new(len(plan.dts)), (out[1:] if plan.default else new(len(plan.dts)))


def _adams_sweep_open(ctx, g, out, W, b, Wd, csr, plan):
    """(ticks, the totals of _sweep_totals, the adjoint at the last tick - None on a step_size plan, whose ticks enter step by step)"""
    ticks = _ticks(ctx, g, out, Wd)
    totals = _sweep_totals(out, csr, W, b, False, False, None)
    return ticks, totals, (ticks.seed(len(plan.dts)) if plan.default else None)


def _adams_sweep_enter(ticks, plan, out, a, i):
    """(the adjoint of the state after grid step i, the step's closing pass): on a step_size plan the ticks the step reported enter at the
    state it ends in and the step closes without one; on the default grid the tick the step starts from rides in its closing pass"""
    if plan.default:
        return a, lambda a, gus: ticks.close(a, gus, i)
    if plan.emits[i]:
        a = ticks.enter(a, [e[0] for e in plan.emits[i]])
    return (torch.zeros_like(out[0]) if a is None else a), _sum_onto


def _adams_sweep_close(ticks, plan, a, gW_tot, gb_tot, b, n_rest):
    """the gradients a node returns: of y0, W, b, the decoder's two, None for the n_rest other inputs"""
    if not plan.default:
        a = ticks.enter(a, [0])                                   # the first tick is y0 itself
    return (a, gW_tot, (gb_tot if b is not None else None)) + ticks.decoder_grads() + (None,) * n_rest


def _warmup_reverse(csr, Wc, bc, y, f, dt, a, vj, acc, close, gf):
    """the adjoint before an RK4 warm-up step: its stages re-formed from the stored y and f = F(y) by the forward loop's own calls
    (fixed_stage ops 2..4, the plain right-hand side: its bits), then _sweep_step's closed form with gf - the gradient f gathers as a
    history term of later steps - one more addend of the gradient of k1"""
    u2 = hip.fixed_stage(2, y, f, dt=dt)
    K2 = hip.rhs(csr, u2, Wc, bc)
    u3 = hip.fixed_stage(3, y, f, K2, dt=dt)
    K3 = hip.rhs(csr, u3, Wc, bc)
    u4 = hip.fixed_stage(4, y, f, K2, K3, dt=dt)
    K4 = hip.rhs(csr, u4, Wc, bc)
    return _sweep_step('rk4', dt, [(y, f), (u2, K2), (u3, K3), (u4, K4)], a, vj, acc, close, gk1_extra=gf)


class _ExplicitAdamsSolve(torch.autograd.Function):
    """FixedGridODESolver.integrate with the AdamsBashforth step (fixed_adams.py:151-211) over ODEFunc, one node per solve:
      forward   ndcn_explicit_adams_train_f32: the loop of the un-differentiated solve, which keeps f_i = F(y_i) of every grid step and
                the state after it in a record (2 panels per step; the per-operation graph keeps y_i, A y_i, the pre-activation and
                f_i).  On the default grid the states ARE the ticks: the record of the states is the solution itself;
      backward  from the last step to the first.  lam_j is the full adjoint of the state y_j.  The evaluation f_i is a term of the
                Adams-Bashforth steps i .. i + max_order - 2, so its gradient gathers from their adjoints in one pass,
                gf_i = sum c * lam_j (core.ab_adjoint_terms; hip.ab_adjoint), and one reverse evaluation gives gu = J(y_i)^T gf_i
                (hip.rhs_vjp, which follows NDCN_RHS_MID_BWD and accumulates the parameter gradients).  An Adams-Bashforth step closes
                with lam_i = lam_{i+1} + gu; an RK4 warm-up step re-forms its stages from the stored y_i and f_i by the forward loop's
                own calls (fixed_stage ops 2..4, the plain right-hand side: its bits) and runs _sweep_step's closed form, gf_i one
                more addend of the gradient of k1.  Kept meanwhile: the max_order - 1 newest adjoints.
    Tick gradients: on the default grid inside the step's closing pass (the `close` form of _FixedGridSolve), on a step_size plan at the
    end of the step that reported the tick, in a pass of their own (the `enter` form of _SubstepSolve; the VJP of tick_emit is the
    identity).  With a decoder the output is hip.linear of the ticks and the sweep takes the (T, N, C) gradient as it is."""

    @staticmethod
    def forward(ctx, y0, W, b, Wd, bd, csr, flags, plan, max_order):
        lib = _lib.load()
        y0c, Wc, bc = _detached(y0, W, b)
        dts, n_steps, steps, same, offs, n_emit = plan_arrays(plan)
        shape, H = tuple(y0c.shape), y0c.shape[1]
        out, rec_f, rec_y = _adams_record(y0c, plan)
        nbytes = int(lib.ndcn_explicit_adams_train_workspace_bytes(shape[0], H))
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=y0c.device)
        with torch.cuda.device(y0c.device):
            check(lib.ndcn_explicit_adams_train_f32(_view(csr, shape[0]), ptr(Wc), ptr(bc), H, flags, ptr(out[0]), dts, n_steps, steps, same,
                                                    offs, n_emit, max_order, ptr(out[1:]), ptr(rec_f), ptr(rec_y), ptr(workspace), nbytes,
                                                    stream_ptr()))
        ctx.meta = (csr, plan, max_order)
        ctx.save_for_backward(out, rec_f, W, b, Wd, *(() if plan.default else (rec_y,)))
        return out if Wd is None else hip.linear(out, Wd.detach(), None if bd is None else bd.detach())

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        out, rec_f, W, b, Wd, *own = ctx.saved_tensors
        csr, plan, max_order = ctx.meta
        rec_y = own[0] if own else out[1:]
        Wc, bc = _detached(W, b)
        dts = plan.dts
        ticks, (gW_tot, gb_tot, vj, acc), a = _adams_sweep_open(ctx, g, out, W, b, Wd, csr, plan)
        lam = {}                                                  # the adjoints that evaluations still to come gather from
        for i in range(len(dts) - 1, -1, -1):
            a, close = _adams_sweep_enter(ticks, plan, out, a, i)
            lam[i + 1] = a
            lam.pop(i + max_order, None)
            terms = core.ab_adjoint_terms(i, dts, max_order)
            gf = hip.ab_adjoint([lam[j] for j, _ in terms], [c for _, c in terms]) if terms else None
            y, f, dt = (out[0] if i == 0 else rec_y[i - 1]), rec_f[i], float(dts[i])
            if min(i + 1, max_order - 1) >= core.AB_MIN_ORDER - 1:
                gu, _, _ = hip.rhs_vjp(csr, y, Wc, f, gf, need_b=bc is not None, gW=gW_tot, gb=gb_tot)
                a = close(a, [gu])
            else:
                a = _warmup_reverse(csr, Wc, bc, y, f, dt, a, vj, acc, close, gf)
        return _adams_sweep_close(ticks, plan, a, gW_tot, gb_tot, b, 4)


def adams_train_enabled():
    """NDCN_ADAMS_TRAIN=1: explicit_adams under a gradient runs on _ExplicitAdamsSolve, fixed_adams on _FixedAdamsSolve (default: the
    per-operation graph)"""
    return _lib.env_str('NDCN_ADAMS_TRAIN', '0') == '1'


def _adams_with_grad(odefunc, y0, t, plan, max_order, readout, corrector=None):
    """explicit_adams (corrector None: _ExplicitAdamsSolve) or fixed_adams (corrector = (rtol, atol, max_iters, step_log):
    _FixedAdamsSolve) over a plain ODEFunc under a gradient on its node, or None where the node has no form: what _adams_admission
    declines, and the nodes' own - the switch off, a `t` that requires grad, fewer than two ticks, an empty state.
    readout = (Wd, bd) (checked by _readout_for_grad): the decoded solution, the decoder inside the node."""
    if not adams_train_enabled() or t.requires_grad or t.numel() < 2:
        return None
    admitted = _adams_admission(odefunc, y0, t, plan, max_order, corrector)
    if admitted is None or admitted[3].numel() == 0:
        return None
    csr, flags, plan, y0 = admitted
    csr.ensure_plans(y0.shape[1])
    csr.transpose().ensure_plans(y0.shape[1])                    # (the reverse sweep's; the solve without a gradient builds none)
    Wd, bd = readout if readout is not None else (None, None)
    args = (y0, odefunc.wt.weight, odefunc.wt.bias, Wd, bd, csr, flags, plan, max_order)
    return _ExplicitAdamsSolve.apply(*args) if corrector is None else _FixedAdamsSolve.apply(*args, *corrector)


def _explicit_adams_with_grad(odefunc, y0, t, plan, max_order, readout=None):
    return _adams_with_grad(odefunc, y0, t, plan, max_order, readout)


def _fixed_adams_with_grad(odefunc, y0, t, plan, max_order, rtol, atol, max_iters, step_log=None, readout=None):
    return _adams_with_grad(odefunc, y0, t, plan, max_order, readout, (rtol, atol, max_iters, step_log))


# ---------------------------------------------------------------------------------------------------
# fixed_adams: the predictor-corrector loop with a record, its reverse sweep in closed form
# ---------------------------------------------------------------------------------------------------

def _first_cap(n_steps):
    """corrector evaluations the first attempt of a fixed_adams training solve has room for: one per grid step, what the drivers'
    tolerances give (the second attempt: n_steps * max_iters, which always suffices)"""
    return n_steps


def _fixed_adams_attempt(view, Wc, bc, flags, out, arrays, max_order, rtol, atol, max_iters, rec_f, rec_y, cap):
    """one call of ndcn_fixed_adams_train_f32 with room for `cap` corrector evaluations -> (return code, iterations, converged flags, first
    slots, rec_u, rec_c)"""
    lib = _lib.load()
    dts, n_steps, steps, same, offs, n_emit = arrays
    shape, H = tuple(out.shape[1:]), out.shape[2]
    rec_u = torch.empty((max(cap, 1),) + shape, dtype=torch.float32, device=out.device)
    rec_c = torch.empty((max(cap, 1),) + shape, dtype=torch.float32, device=out.device)
    nbytes = int(lib.ndcn_fixed_adams_train_workspace_bytes(shape[0], H))
    workspace = torch.empty(nbytes, dtype=torch.uint8, device=out.device)
    iters, conv, slots = (ctypes.c_int * n_steps)(), (ctypes.c_int * n_steps)(), (ctypes.c_int64 * n_steps)()
    with torch.cuda.device(out.device):
        rc = lib.ndcn_fixed_adams_train_f32(view, ptr(Wc), ptr(bc), H, flags, ptr(out[0]), dts, n_steps, steps, same, offs, n_emit, max_order,
                                            float(rtol), float(atol), int(max_iters), ptr(out[1:]), iters, conv, ptr(rec_f), ptr(rec_y),
                                            ptr(rec_u), ptr(rec_c), cap, slots, ptr(workspace), nbytes, stream_ptr())
    return rc, list(iters), [bool(c) for c in conv], list(slots), rec_u, rec_c


class _FixedAdamsSolve(torch.autograd.Function):
    """FixedGridODESolver.integrate with the AdamsBashforthMoulton step (fixed_adams.py:151-205) over ODEFunc, one node per solve:
      forward   ndcn_fixed_adams_train_f32: the loop, read-backs and bits of the un-differentiated solve, which keeps f_i = F(y_i) and the
                state after every grid step (as _ExplicitAdamsSolve) and, per corrector evaluation, the iterate it read and its result
                (u_{r-1}, F_r) in slots handed out in order.  Room for one evaluation per step first; where a step iterates more and the
                room runs out the library says so (NDCN_ECAPACITY) and the solve runs once more with room for max_iters per step.  The
                iteration counts and converged flags are constants of the graph, as on the per-operation path;
      backward  from the last step to the first, lam_{i+1} the full adjoint of y_{i+1}.  A step that held n >= 3 evaluations ran
                u_0 = y_i + dy_0, u_r = y_i + c0 F_r + delta (F_r = F(u_{r-1}), r = 1..R), y_{i+1} = u_R.  So G_R = lam_{i+1},
                G_{r-1} = J(u_{r-1})^T (c0 G_r) - one hip.scale (the factor c0 by a pass of its own: every G is then a panel the
                existing closing forms take with unit weights) and one hip.rhs_vjp at the stored pair, which accumulates gW / gb -,
                P_i = G_0 the adjoint of dy_0, D_i = sum_{r>=1} G_r that of delta (R = 1: lam_{i+1} itself, no pass).  f_i is a term of
                dy_0 and of delta of every later step that holds it: gf_i = sum cP P_i' + cD D_i' in one pass (core.abm_adjoint_terms,
                hip.abm_adjoint), gu = J(y_i)^T gf_i, and lam_i = D_i + (P_i + gu [+ the tick]).  RK4 warm-up steps as in
                _ExplicitAdamsSolve, gf_i one more addend of the gradient of k1.  Kept meanwhile: the max_order - 1 newest P and D.
    Ticks and the decoder as in _ExplicitAdamsSolve."""

    @staticmethod
    def forward(ctx, y0, W, b, Wd, bd, csr, flags, plan, max_order, rtol, atol, max_iters, step_log):
        y0c, Wc, bc = _detached(y0, W, b)
        arrays = plan_arrays(plan)
        n_steps = arrays[1]
        out, rec_f, rec_y = _adams_record(y0c, plan)
        view = _view(csr, y0c.shape[0])
        full = n_steps * max_iters
        cap = min(_first_cap(n_steps), full)
        res = _fixed_adams_attempt(view, Wc, bc, flags, out, arrays, max_order, rtol, atol, max_iters, rec_f, rec_y, cap)
        if res[0] == _lib.ECAPACITY and cap < full:
            del res                                               # (the first attempt's slots go back before the larger ones are taken)
            res = _fixed_adams_attempt(view, Wc, bc, flags, out, arrays, max_order, rtol, atol, max_iters, rec_f, rec_y, full)
        rc, iters, conv, slots, rec_u, rec_c = res
        check(rc)
        _report_corrector(step_log, iters, conv)
        ctx.meta = (csr, plan, max_order, iters, conv, slots)
        ctx.save_for_backward(out, rec_f, rec_u, rec_c, W, b, Wd, *(() if plan.default else (rec_y,)))
        return out if Wd is None else hip.linear(out, Wd.detach(), None if bd is None else bd.detach())

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        out, rec_f, rec_u, rec_c, W, b, Wd, *own = ctx.saved_tensors
        csr, plan, max_order, iters, conv, slots = ctx.meta
        rec_y = own[0] if own else out[1:]
        Wc, bc = _detached(W, b)
        dts = plan.dts
        n_steps = len(dts)
        lengths = core.abm_history_lengths(n_steps, max_order, conv)
        ticks, (gW_tot, gb_tot, vj, acc), a = _adams_sweep_open(ctx, g, out, W, b, Wd, csr, plan)
        rvjp = lambda u, K, gk: hip.rhs_vjp(csr, u, Wc, K, gk, need_b=bc is not None, gW=gW_tot, gb=gb_tot)[0]
        Ps, Ds = {}, {}                                           # the adjoints that evaluations still to come gather from
        for i in range(n_steps - 1, -1, -1):
            a, close = _adams_sweep_enter(ticks, plan, out, a, i)
            y, f, dt = (out[0] if i == 0 else rec_y[i - 1]), rec_f[i], float(dts[i])
            pc_step = lengths[i] >= core.AB_MIN_ORDER - 1
            if pc_step:
                c0 = float(core.abm_lead(dts[i], lengths[i]))
                G, later = a, []
                for s in range(slots[i] + iters[i] - 1, slots[i] - 1, -1):
                    if G is not a:
                        later.append(G)
                    G = rvjp(rec_u[s], rec_c[s], hip.scale(G, c0))
                Ps[i], Ds[i] = G, (a if not later else _sum_onto(a, later))
                Ps.pop(i + max_order - 1, None)
                Ds.pop(i + max_order - 1, None)
            terms = core.abm_adjoint_terms(i, dts, max_order, conv)
            gf = hip.abm_adjoint([Ps[s] for s, _, _ in terms], [c for _, c, _ in terms], [Ds[s] for s, _, _ in terms],
                                 [c for _, _, c in terms]) if terms else None
            if pc_step:
                a = close(Ds[i], [Ps[i], rvjp(y, f, gf)])
            else:
                a = _warmup_reverse(csr, Wc, bc, y, f, dt, a, vj, acc, close, gf)
        return _adams_sweep_close(ticks, plan, a, gW_tot, gb_tot, b, 8)


# ---------------------------------------------------------------------------------------------------
# any size, the loops inside the library
# ---------------------------------------------------------------------------------------------------

def _fixed_grid_train(y0c, Wc, bc, csr, flags, method, dts):
    """ndcn_fixed_grid_train_f32 -> (trajectory (n_ticks + 1, N, H), the step sizes as the C array)"""
    lib = _lib.load()
    n_ticks = len(dts)
    out = torch.empty((n_ticks + 1,) + tuple(y0c.shape), dtype=torch.float32, device=y0c.device)
    scratch = Tape(y0c.device)
    arr = (ctypes.c_float * n_ticks)(*dts)
    with torch.cuda.device(y0c.device):
        rc = lib.ndcn_fixed_grid_train_f32(_view(csr, y0c.shape[0]), ptr(Wc), ptr(bc), y0c.shape[1], flags, _lib.METHODS[method], ptr(y0c),
                                           arr, n_ticks, ptr(out), ctypes.cast(scratch.cb, ctypes.c_void_p), None, stream_ptr())
    _finish(scratch, rc)
    return out, arr


def _fixed_grid_reverse(out, Wc, bc, csr, flags, method, arr, n_ticks, g, decoder=None):
    """The reverse sweep in the library -> (g_y0, g_W, g_b, g_Wd, g_bd).  g: the gradient of the trajectory (n_ticks + 1, N, H), or
    with decoder = (Wd (C, H), want g_Wd, want g_bd) the gradient of the DECODED ticks (n_ticks + 1, N, C): the sweep then forms every
    tick's g[i] . Wd where it adds it (ndcn_fixed_grid_backward_readout_f32) and returns the decoder's gradients too."""
    lib = _lib.load()
    g = g.contiguous()
    no_control = bool(flags & _lib.F_NO_CONTROL)
    gy = torch.empty_like(out[0])
    gW = torch.empty_like(Wc) if (Wc is not None and not no_control) else None
    gb = torch.empty_like(bc) if (bc is not None and not no_control) else None
    scratch = Tape(g.device)
    view = _view(csr, out.shape[1])
    view_t = csr.transpose().view_ref() if csr is not None else None
    alloc = ctypes.cast(scratch.cb, ctypes.c_void_p)
    gWd = gbd = None
    with torch.cuda.device(g.device):
        if decoder is None:
            rc = lib.ndcn_fixed_grid_backward_f32(view, view_t, ptr(Wc), ptr(bc), out.shape[2], flags, _lib.METHODS[method], ptr(out), ptr(g), arr,
                                                  n_ticks, ptr(gy), ptr(gW), ptr(gb), alloc, None, stream_ptr())
        else:
            Wd, want_W, want_b = decoder
            if want_W or want_b:
                gWd = torch.empty_like(Wd)
                gbd = torch.empty((Wd.shape[0],), dtype=torch.float32, device=g.device) if want_b else None
            rc = lib.ndcn_fixed_grid_backward_readout_f32(view, view_t, ptr(Wc), ptr(bc), out.shape[2], flags, _lib.METHODS[method], ptr(out),
                                                          ptr(g), ptr(Wd), Wd.shape[0], arr, n_ticks, ptr(gy), ptr(gW), ptr(gb), ptr(gWd),
                                                          ptr(gbd), alloc, None, stream_ptr())
    _finish(scratch, rc)
    return gy, gW, gb, gWd, gbd


class _NativeFixedGrid(torch.autograd.Function):
    """Euler / midpoint / RK4 over ODEFunc with the loops of _FixedGridSolve inside the library (ndcn_fixed_grid_train_f32 /
    ndcn_fixed_grid_backward_f32, with a decoder ndcn_fixed_grid_backward_readout_f32): the same launches, two calls instead of ~10
    per step."""

    @staticmethod
    def forward(ctx, y0, W, b, Wd, bd, csr, flags, method, dts):
        y0c, Wc, bc = _detached(y0, W, b)
        out, arr = _fixed_grid_train(y0c, Wc, bc, csr, flags, method, dts)
        ctx.keep = (Wc, bc, csr, flags, method, arr, len(dts))
        # Without a decoder `out` is this node's own output: saved through autograd (no out -> grad_fn -> ctx -> out cycle that only the
        # cyclic collector would break - a (T, N, H) trajectory - and an in-place edit of the returned trajectory before backward
        # raises).  With one the hidden trajectory is no output of the node: nothing differentiates through it, and it is released
        # with the graph.
        ctx.save_for_backward(out, W, b, Wd)
        return out if Wd is None else hip.linear(out, Wd.detach(), None if bd is None else bd.detach())

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        out, _, _, Wd = ctx.saved_tensors
        Wc, bc, csr, flags, method, arr, n_ticks = ctx.keep
        needs = ctx.needs_input_grad
        decoder = None if Wd is None else (Wd.detach().contiguous(), needs[3], needs[4])
        grads = _fixed_grid_reverse(out, Wc, bc, csr, flags, method, arr, n_ticks, g, decoder=decoder)
        return tuple(x if want else None for x, want in zip(grads, needs)) + (None,) * 4


def fixed_grid(y0, W, b, Wd, bd, csr, flags, method, dts):
    """-> the solution from _NativeFixedGrid, or None when the native loops are switched off (NDCN_FIXED_GRID_NATIVE=0)"""
    if not _lib.env_on('NDCN_FIXED_GRID_NATIVE') or _lib.env_str('NDCN_VJP', 'hip') == 'torch':
        return None
    if csr is not None:
        csr.ensure_plans(y0.shape[1])
        csr.transpose().ensure_plans(y0.shape[1])
    return _NativeFixedGrid.apply(y0, W, b, Wd, bd, csr, flags, method, dts)


# ---------------------------------------------------------------------------------------------------
# routing (odeint under a gradient calls these, in this order)
# ---------------------------------------------------------------------------------------------------

def _small_solve_with_grad(odefunc, y0, t, method='euler', plan=None):
    """The one-launch training path when the library supports the shape (H <= 31, the state and three work panels in one
    CU's LDS: the reference's README commands), else None - the caller falls back to the fused-launch nodes."""
    if t.requires_grad or not _lib.env_on('NDCN_SOLVE_SMALL_GRAD') or t.numel() < 2:
        return None
    op = _small_operator(odefunc, y0)
    if op is None:
        return None
    csr, view, flags = op
    if not _lib.load().ndcn_solve_small_supported(view, odefunc.hidden_size, flags, _lib.METHODS[method], 1):
        return None
    if method != 'euler' and not _lib.env_on('NDCN_SOLVE_SMALL_RK_GRAD'):
        return None
    core.assert_increasing(t)
    y0 = _lib.require_device(y0, 'state y0').contiguous()
    W, b = odefunc.wt.weight, odefunc.wt.bias
    if plan is not None:
        # the step_size option: the one-launch pair on the explicit grid into a scratch trajectory (kilobytes per step at sizes that
        # fit one compute unit), the ticks gathered from it - coincident ticks are its rows, the others pass through tick_emit
        from ...autograd_ops import autograd_ops
        fine = _SmallEulerSolve.apply(y0, W, b, csr, flags, plan.dts.tolist(), method)
        ticks = [fine[0]]
        for i, em in enumerate(plan.emits):
            loose = [e for e in em if not e[1]]
            made = {}
            for q in range(0, len(loose), core.MAX_EMIT):
                part = loose[q:q + core.MAX_EMIT]
                for e, o in zip(part, autograd_ops.tick_emit(fine[i + 1], plan.dts[i], [e[2] for e in part])):
                    made[e[0]] = o
            ticks.extend(fine[i + 1] if same else made[j] for j, same, _ in em)
        return torch.stack(ticks)
    tt = core.host_grid(t).to(y0.dtype)                    # solvers.py:81: the grid in the state dtype
    dts = (tt[1:] - tt[:-1]).tolist()
    return _SmallEulerSolve.apply(y0, W, b, csr, flags, dts, method)


def _readout_for_grad(readout, y0):
    """(Wd, bd) when the fixed-grid training nodes can hold this decoder (hip.readout_bwd: float32 on the state's device, (C, H) with
    1 <= C <= 15), else None - odeint then decodes the hidden solution in a step of its own"""
    if readout is None:
        return None
    Wd, bd = readout
    ok = torch.is_tensor(Wd) and Wd.dim() == 2 and Wd.dtype == torch.float32 and Wd.device == y0.device and Wd.shape[1] == y0.shape[1] and \
        1 <= Wd.shape[0] <= hip.READOUT_BWD_MAX_C
    if ok and bd is not None:
        ok = torch.is_tensor(bd) and bd.dtype == torch.float32 and bd.device == y0.device and tuple(bd.shape) == (Wd.shape[0],)
    return (Wd, bd) if ok else None


def _fixed_grid_with_grad(odefunc, y0, t, method, plan=None, readout=None):
    """The fused-launch training path of a fixed-grid solve over ODEFunc when the one-launch kernels do not take it (any size).
    readout = (Wd, bd) (checked by _readout_for_grad): the DECODED solution, the decoder's Linear inside the solve's autograd node."""
    if t.requires_grad or not _lib.env_on('NDCN_FIXED_GRID_GRAD') or t.numel() < 2:
        return None
    op = _small_operator(odefunc, y0)
    if op is None:
        return None
    csr, _, flags = op
    core.assert_increasing(t)
    drop = None
    n_steps = len(plan.dts) if plan is not None else t.numel() - 1
    if _dropout.is_active(odefunc):
        # the solve's seed and a block of evaluation numbers, one per evaluation in the solver's order - the numbers the per-operation
        # path hands out one by one (ODEFunc.forward), so both paths apply the same masks
        stream = _dropout.current() or _dropout.Stream()
        drop = (float(odefunc.dropout), stream.seed, stream.take(n_steps * EVALS[method]))
    y0 = _lib.require_device(y0, 'state y0').contiguous()
    W, b = odefunc.wt.weight, odefunc.wt.bias
    Wd, bd = readout if readout is not None else (None, None)
    if plan is not None:                                      # the step_size option: checkpointed per tick interval
        return _SubstepSolve.apply(y0, W, b, Wd, bd, csr, flags, method, plan, drop)
    tt = core.host_grid(t).to(y0.dtype)
    dts = (tt[1:] - tt[:-1]).tolist()
    if drop is None:                                          # (the C++ tape has no dropout form)
        sol = fixed_grid(y0, W, b, Wd, bd, csr, flags, method, dts)
        if sol is not None:
            return sol
    return _FixedGridSolve.apply(y0, W, b, Wd, bd, csr, flags, method, dts, drop)
