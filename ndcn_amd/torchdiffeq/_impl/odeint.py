"""`odeint(func, y0, t, rtol, atol, method, options)` - drop-in for the reference's vendored
torchdiffeq entry point (torchdiffeq/_impl/odeint.py:20-76), computed by HIP kernels.

Two execution paths, both on the GPU:
  * device-resident: `func` is this package's ODEFunc acting on one N x H fp32 panel - or one of the drivers' ground-truth
    dynamics (ndcn_amd.truth) on an N x 1 state - -> the whole solve
    runs inside libndcn_hip.so (`ndcn_solver_*`): state, stages and dense-output coefficients never
    leave HBM and the host sees one 16-byte record per adaptive step;
  * generic: any callable / tuple state -> the reference's solver control flow (core.py) with one fused
    HIP kernel per bookkeeping chain and `func` called back in Python.
Host tensors are refused: there is no CPU fallback.
"""
import collections
import ctypes
import os
import weakref

import torch

from ... import _lib
from ... import dropout as _dropout
from ...ops import hip, new_solve_epoch
from ...truth import TRUTH_CLASSES
from . import core

SOLVERS = {m: m for m in core.METHODS}      # the in-scope subset of odeint.py:8-17
GRAPH_MAX_ELEMS = 1 << 23                   # below ~8M state elements (Pubmed x 256) a step is launch-bound


def _autonomous(func):
    return bool(getattr(func, 'ndcn_autonomous', False))


def _needs_grad(func, y0, probe=None):
    """(needs_grad, probe output or None).  True when the solve must be differentiable: the state or the parameters of
    an nn.Module `func` require grad - or `func` is a plain callable (lambda, bound method, closure over parameters)
    whose output carries autograd history: the reference differentiates through any callable, so that case is detected
    by evaluating `probe()` = func(t0, y0).  That evaluation is the solver's own first one (f0 of dopri5.py:78, k1 of
    the first fixed-grid step): its output is handed back so that the solve REUSES it instead of evaluating twice
    (user-side evaluation counters and RNG-consuming functions see exactly the reference's sequence of calls)."""
    if not torch.is_grad_enabled():
        return False, None
    if any(y.requires_grad for y in y0):
        return True, None
    if isinstance(func, torch.nn.Module):
        return any(p.requires_grad for p in func.parameters()), None
    if probe is not None:
        out = probe()
        return any(torch.is_tensor(o) and o.requires_grad for o in out), out
    return False, None


def _reuse_first_evaluation(func, y0, out):
    """func, except that its FIRST call - which every solver path makes at (t[0], y0) - returns `out`, the value the
    differentiability probe already computed there."""
    pending = [out]

    def wrapped(t, y):
        o = pending[0]
        if o is not None:
            pending[0] = None
            if len(y) == len(y0) and all(a is b for a, b in zip(y, y0)):
                return o
        return func(t, y)
    return wrapped


def odeint(func, y0, t, rtol=1e-7, atol=1e-9, method=None, options=None, step_log=None, readout=None):
    """Integrate dy/dt = func(t, y), y(t[0]) = y0; returns y at every t (first dim), y0 first.  (The body is `_odeint`; this frame
    fetches the time grid to the host once for everything below that asks about it: core.grid_scope - and opens the solve's dropout
    stream: one seed, evaluations numbered from 0, ndcn_amd/dropout.py.)

    readout=(weight (C, H), bias (C,) or None): return `linear(odeint(...), weight, bias)`, shape (len(t), N, C), instead of the
    hidden states (neural_dynamics.py:148-160: NDCN decodes every tick).  Where nothing needs a gradient and the solve is
    device-resident, the library decodes each tick as the solver produces it (ndcn_solver_advance_many_readout: H = 16, 20, .. 60
    or 64 <= H <= 512, C <= 15) and the (len(t), N, H) trajectory is never stored; under a gradient, euler / midpoint / rk4 over ODEFunc on the fused-launch training
    path hold the decoder inside the solve's autograd node: the trajectory is stored once (the reverse sweep needs it) but the
    (len(t), N, H) gradient of it, which the Linear's own backward would write, is not - the sweep forms each tick's g . W where it
    adds it (ndcn_readout_bwd_f32); everywhere else the ordinary solve runs and the Linear is applied to its result - the
    values are the same bits either way, only the memory differs.  A tuple state raises ValueError."""
    with core.grid_scope(t), _dropout.solve_scope():
        if readout is None:
            return _odeint(func, y0, t, rtol, atol, method, options, step_log)[0]
        if not torch.is_tensor(y0):
            raise ValueError('`readout` decodes a tensor state; got a tuple')
        W, b = readout
        _lib.load().ndcn_clear_readout_path()
        sol, decoded = _odeint(func, y0, t, rtol, atol, method, options, step_log, readout=(W, b))
        return sol if decoded else _decode(sol, W, b)


def _decode(sol, W, b):
    """linear(sol, W, b) over the last dimension: the differentiable wrapper where a gradient is asked for"""
    if torch.is_grad_enabled() and any(x is not None and x.requires_grad for x in (sol, W, b)):
        from ...autograd_ops import linear
        return linear(sol, W, b)
    return hip.linear(sol, W, b)


def _odeint(func, y0, t, rtol=1e-7, atol=1e-9, method=None, options=None, step_log=None, readout=None):
    """Integrate dy/dt = func(t, y), y(t[0]) = y0; returns y at every t (first dim), y0 first.

    Same signature, defaults, return layout and exceptions as the reference (odeint.py:20-76):
    TypeError for non-float y0 / t, ValueError for `options` without `method`, KeyError for an unknown
    method, AssertionError for a non-monotone t.  Deviations: dopri5 / adams / explicit_adams / euler / midpoint / rk4 are
    provided (tsit5 / fixed_adams raise NotImplementedError); the state must be float32 on a ROCm device;
    `step_log` (a list) optionally receives the dopri5 per-attempt log.  Returns (solution, decoded): decoded is True when
    `readout` was applied inside the solve (the device-resident inference path; the fixed-grid training nodes), else the solution
    is the hidden one.

    Fixed-grid methods take options={'step_size': h} as the reference's FixedGridODESolver does (solvers.py:39-108): the solver
    integrates on its own float32 grid t[0], t[0] + h, ... (last point clamped to t[-1]; AssertionError where rounding leaves it
    short) and every tick gets the state at the END of the first grid step that reaches it - the reference overwrites y0 with y1
    before it "interpolates", so nothing is interpolated; a tick strictly inside a step additionally has -0.0 turned into +0.0 and
    Inf into NaN.  Any `grid_constructor` raises the reference's ValueError; other names only warn.  One deviation: `step_size`
    with a `t` that requires grad raises NotImplementedError (the grid's dependence on t[0] / t[-1] is not differentiated).

    explicit_adams is the reference's AdamsBashforth (fixed_adams.py:151-211) on the same grids: two RK4 (3/8 rule) steps, then ONE
    evaluation per step combined with up to ten earlier ones (options={'max_order': m}, default 12: orders 3 .. m - 1; m = 2 or 3
    never leaves RK4; m < 2 fails as in the reference).  Without a gradient a plain ODEFunc runs the whole solve inside the library
    (ndcn_solve_explicit_adams_f32: nothing is read back); any other callable, a tuple state or a gradient steps through core.py.
    """
    user_func = func
    t_user = t
    tensor_input, func, y0, t = core.check_inputs(func, y0, t)
    new_solve_epoch()                            # weights written through `.data` since the last solve are packed afresh

    if options is None:
        options = {}
    elif method is None:
        raise ValueError('cannot supply `options` without specifying `method`')
    if method is None:
        method = 'dopri5'
    if method in core.UNSUPPORTED:
        raise NotImplementedError('method %r of the reference is outside the accelerated path '
                                  '(dopri5, adams, explicit_adams, euler, midpoint, rk4 are provided)' % method)
    method = SOLVERS[method]                     # KeyError for an unknown name, as the reference's dict lookup

    plan = None
    if method in core.GRID_METHODS:
        options = core.fixed_options(method, options)       # solvers.py:39-53: warns about unknown names, ValueError for a grid_constructor
        step_size = options.get('step_size')                # (what is left: the step size, explicit_adams' max_order)
        if step_size is not None:
            if t_user.requires_grad:
                raise NotImplementedError('step_size with a time vector that requires grad: the dependence of the grid on t[0] / t[-1] '
                                          'is not differentiated')
            core.assert_increasing(t)
            plan = core.fixed_plan(core.host_grid(t).to(y0[0].dtype).numpy(), step_size)
    for y in y0:
        _lib.require_device(y, 'state y0')
    needs_grad, f0 = _needs_grad(user_func, y0, probe=lambda: func(t[0].to(y0[0].dtype), y0))
    if f0 is not None:
        func = _reuse_first_evaluation(func, y0, f0)
    if needs_grad and method in ('euler', 'midpoint', 'rk4') and \
            _device_resident_ok(user_func, tensor_input, y0, t_user, method, options, allow_dropout=True):
        # (an active dropout: the one-launch pair declines; the fused launches carry the mask and re-create it in the reverse sweep)
        sol = None
        if not _dropout.is_active(user_func):
            sol = _small_solve_with_grad(user_func, y0[0], t, method, plan)                  # one launch forward, one backward
        if sol is None:
            # any size: fused launches forward, closed-form sweep backward - with `readout` the decoder inside the same node
            dec = _readout_for_grad(readout, y0[0])
            sol = _fixed_grid_with_grad(user_func, y0[0], t, method, plan, readout=dec)
            if sol is not None:
                return sol, dec is not None
        if sol is not None:
            return sol, False
    if needs_grad:
        from .autograd_path import odeint_with_grad
        plain, taped = _dopri5_tape_route(user_func, tensor_input, y0, t_user, method, options)
        if taped:
            # one autograd node per solve: the native tape (csrc/tape.hip) runs the launches below and their reverse pass itself
            from . import tape
            return tape.solve(user_func, y0[0], t, rtol, atol, options, step_log), False
        sol = odeint_with_grad(func, y0, t, rtol, atol, method, options, autonomous=_autonomous(user_func),
                               step_log=step_log, odefunc=user_func if plain else None, plan=plan)
    elif method == 'explicit_adams':
        out = None
        if _device_resident_ok(user_func, tensor_input, y0, t_user, method, options):
            out = _explicit_adams_solve(user_func, y0[0], t, plan, options['max_order'])
        if out is not None:
            return out, False
        sol = core.integrate_fixed(hip, func, y0, t, method, autonomous=_autonomous(user_func), plan=plan, max_order=options['max_order'])
    elif _device_resident_ok(user_func, tensor_input, y0, t_user, method, options, allow_truth=True):
        return _device_resident(user_func, y0[0], t, rtol, atol, method, options, step_log, plan, readout)
    elif method == 'dopri5':
        sol = core.integrate_dopri5(hip, func, y0, t, rtol, atol, autonomous=_autonomous(user_func),
                                    step_log=step_log, **options)
    elif method == 'adams':
        sol = core.integrate_adams(hip, func, y0, t, rtol, atol, autonomous=_autonomous(user_func),
                                   step_log=step_log, **options)
    else:
        sol = core.integrate_fixed(hip, func, y0, t, method, autonomous=_autonomous(user_func), plan=plan)
    out = tuple(torch.stack([s[i] for s in sol]) for i in range(len(y0)))
    return (out[0] if tensor_input else out), False


# ---------------------------------------------------------------------------------------------------
# training on a state that fits one compute unit: the whole Euler solve and its reverse sweep, one launch each
# ---------------------------------------------------------------------------------------------------

class _SmallEulerSolve(torch.autograd.Function):
    """FixedGridODESolver.integrate with Euler (and, round 5, midpoint / RK4 3-8) steps (solvers.py:79-99, fixed_grid.py:7-29,
    rk_common.py:72-78) over ODEFunc, differentiated the
    way the reference's drivers train - plain backpropagation through every step (heat_dynamics.py:313-334) - with
    ndcn_solve_small_f32 / ndcn_solve_small_bwd_f32 (csrc/solve_small.hip): the forward's trajectory IS the saved state."""

    @staticmethod
    def forward(ctx, y0, W, b, csr, flags, dts, method='euler'):
        lib = _lib.load()
        n_ticks = len(dts)
        H = y0.shape[1]
        ctx.method = _lib.METHODS[method]
        out = torch.empty((n_ticks + 1,) + tuple(y0.shape), dtype=torch.float32, device=y0.device)
        out[0].copy_(y0)
        arr = (ctypes.c_float * n_ticks)(*dts)
        no_control = bool(flags & _lib.F_NO_CONTROL)
        Wd = None if no_control else W.detach().contiguous()
        bd = None if (no_control or b is None) else b.detach().contiguous()
        view = csr.view_ref(need_symmetric=True) if csr is not None else ctypes.byref(_lib.empty_csr(y0.shape[0]))
        # Euler on the README shapes: the forward launch keeps S_i = A y_i and K_i of every step for the reverse sweep (two panels per
        # tick instead of a gather and a Linear per tick in backward: ndcn_solve_small_keep_*)
        keep = None
        if ctx.method == _lib.M_EULER and csr is not None and Wd is not None and lib.ndcn_solve_small_keep_supported(view, H, flags):
            keep = torch.empty((n_ticks, 2) + tuple(y0.shape), dtype=torch.float32, device=y0.device)
        with torch.cuda.device(y0.device):
            if keep is not None:
                _lib.check(lib.ndcn_solve_small_keep_f32(view, _lib.ptr(Wd), _lib.ptr(bd), H, flags, _lib.ptr(out[0]), arr, n_ticks,
                                                         _lib.ptr(out[1:]), _lib.ptr(keep), _lib.stream_ptr()))
            else:
                _lib.check(lib.ndcn_solve_small_f32(view, _lib.ptr(Wd), _lib.ptr(bd), H, flags, ctx.method, _lib.ptr(out[0]), arr,
                                                    n_ticks, _lib.ptr(out[1:]), _lib.stream_ptr()))
        ctx.csr, ctx.flags, ctx.dts, ctx.keep = csr, flags, arr, keep
        ctx.has_W, ctx.has_b = Wd is not None, bd is not None
        # (W and b through save_for_backward: an in-place parameter change between forward and backward raises, as it does for
        # every other autograd node, instead of differentiating the wrong weights)
        ctx.save_for_backward(out, *([W] if Wd is not None else []), *([b] if bd is not None else []))
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        out, *wb = ctx.saved_tensors
        lib = _lib.load()
        Wd = wb[0].detach().contiguous() if ctx.has_W else None
        bd = wb[1 if ctx.has_W else 0].detach().contiguous() if ctx.has_b else None
        H = out.shape[2]
        g = g.contiguous()
        g_y0 = torch.empty_like(out[0])
        g_W = torch.empty((H, H), dtype=torch.float32, device=out.device) if Wd is not None else None
        g_b = torch.empty((H,), dtype=torch.float32, device=out.device) if Wd is not None else None
        csr = ctx.csr
        view = csr.view_ref(need_symmetric=True) if csr is not None else ctypes.byref(_lib.empty_csr(out.shape[1]))
        view_t = csr.transpose().view_ref() if csr is not None else view
        with torch.cuda.device(out.device):
            if ctx.keep is not None:
                _lib.check(lib.ndcn_solve_small_bwd_keep_f32(view, view_t, _lib.ptr(Wd), _lib.ptr(bd), H, ctx.flags, _lib.ptr(out), _lib.ptr(g),
                                                             ctx.dts, len(ctx.dts), _lib.ptr(ctx.keep), _lib.ptr(g_y0), _lib.ptr(g_W),
                                                             _lib.ptr(g_b), _lib.stream_ptr()))
                ctx.keep = None
            else:
                _lib.check(lib.ndcn_solve_small_bwd_f32(view, view_t, _lib.ptr(Wd), _lib.ptr(bd), H, ctx.flags, ctx.method, _lib.ptr(out),
                                                        _lib.ptr(g), ctx.dts, len(ctx.dts), _lib.ptr(g_y0), _lib.ptr(g_W), _lib.ptr(g_b),
                                                        _lib.stream_ptr()))
        return g_y0, g_W, (g_b if bd is not None else None), None, None, None, None


class _FixedGridSolve(torch.autograd.Function):
    """FixedGridODESolver.integrate (solvers.py:79-99) over ODEFunc at ANY size, differentiated the way the drivers train (plain
    backpropagation through every step, heat_dynamics.py:313-334), on the kernels of the inference path:
      forward   the launches of the device-resident solver - the stage algebra of every step rides in the epilogues of its
                right-hand-side launches (ndcn_rhs_rk_f32: Euler / midpoint 1 launch per evaluation, RK4 4 per step); only the
                trajectory - the output - is kept;
      backward  per step, in reverse: the stages are re-formed from the stored state by the same launches (checkpointing: the
                reference's autograd keeps every stage of every step), then the step's vector-Jacobian products in closed
                form - SpMM, the masked Linear backward (g_S, g_W, g_b in one call), SpMM with A^T with the step size folded
                into its alpha - and the stage recurrences as one linear-combination launch each.
    No autograd graph per operation: the torch `add` / `mul` launches between the kernels are gone (they were 17 % of the
    kernel time of a 100k-node Euler training step).
    Active dropout (drop = (p, seed, first evaluation number of the solve)): evaluation e of the solve - EVALS[method] per step, in the
    solver's order - runs with the mask of (seed, first + e) in its launch; the reverse pass re-forms the stages with the same
    numbers, so the K it masks the backward kernels with are the forward's, and the scalar s = 1 / (1 - p) rides in the alphas."""

    EVALS = {'euler': 1, 'midpoint': 2, 'rk4': 4}

    @staticmethod
    def _drop_at(drop, method, step):
        """the (p, seed, evaluation) of the first evaluation of grid step `step`"""
        return None if drop is None else (drop[0], drop[1], drop[2] + step * _FixedGridSolve.EVALS[method])

    @staticmethod
    def _solve(ctx, y0, W, b, csr, flags, method, dts, drop):
        """the forward launches -> the trajectory; ctx.meta set"""
        n_ticks = len(dts)
        out = torch.empty((n_ticks + 1,) + tuple(y0.shape), dtype=torch.float32, device=y0.device)
        out[0].copy_(y0)
        no_graph, no_control = bool(flags & _lib.F_NO_GRAPH), bool(flags & _lib.F_NO_CONTROL)
        ctx.meta = (csr, no_graph, no_control, method, dts, drop)
        for i, dt in enumerate(dts):
            _FixedGridSolve._step(csr, out[i], W, b, no_graph, no_control, method, dt, out[i + 1],
                                  drop=_FixedGridSolve._drop_at(drop, method, i))
        return out

    @staticmethod
    def forward(ctx, y0, W, b, csr, flags, method, dts, drop=None):
        out = _FixedGridSolve._solve(ctx, y0, W, b, csr, flags, method, dts, drop)
        ctx.save_for_backward(out, W, b)
        return out

    @staticmethod
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

    @staticmethod
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

    @staticmethod
    def _sweep_step(method, dt, st, a, vj, acc, extra):
        """the adjoint before one step from the adjoint `a` after it: st = the step's [(stage input, K), ...], vj / acc as in backward;
        extra: gradients that enter at the state the step starts from, added in the same pass - a list of panels, or a callable
        extra(a, [gu, ...]) that makes the pass itself (the readout form: the entering gradient is formed inside hip.readout_bwd)"""
        if callable(extra):
            close = lambda gus: extra(a, gus)
        else:
            close = lambda gus: hip.lincomb(gus + extra, [1.0] * (len(gus) + len(extra)), y0=a)
        if method == 'euler':                                   # y1 = y + dt k1
            (u1, K1), = st
            gu1, gW, gb = vj(u1, K1, a, dt)
            acc(gW, gb, dt)
            return close([gu1])
        if method == 'midpoint':                                # ym = y + (dt / 2) k1 ; y1 = y + dt k2
            (u1, K1), (u2, K2) = st
            gu2, gW, gb = vj(u2, K2, a, dt)                     # dL/d ym
            acc(gW, gb, dt)
            gu1, gW, gb = vj(u1, K1, gu2, dt / 2.0)
            acc(gW, gb, dt / 2.0)
            return close([gu2, gu1])
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
        gk1 = hip.lincomb([a, gu4, gu3, gu2], [c8, dt, -dt / 3.0, dt / 3.0])
        gu1, gW, gb = vj(u1, K1, gk1, 1.0)
        acc(gW, gb, 1.0)
        return close([gu4, gu3, gu2, gu1])

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        out, W, b = ctx.saved_tensors
        csr, no_graph, no_control, method, dts, drop = ctx.meta
        g = g.contiguous()
        n_ticks = len(dts)
        H = out.shape[2]
        a = g[n_ticks]
        gW_tot = torch.zeros((H, H), dtype=torch.float32, device=out.device) if not no_control else None
        gb_tot = torch.zeros((H,), dtype=torch.float32, device=out.device) if not no_control else None
        vj, acc = _FixedGridSolve._vj_acc(csr, W, b, no_graph, no_control, drop, gW_tot, gb_tot)
        for i in range(n_ticks - 1, -1, -1):
            st = []
            scratch = torch.empty_like(out[0])
            _FixedGridSolve._step(csr, out[i], W, b, no_graph, no_control, method, dts[i], scratch, keep=st,
                                  drop=_FixedGridSolve._drop_at(drop, method, i))
            a = _FixedGridSolve._sweep_step(method, dts[i], st, a, vj, acc, [g[i]])
        return a, gW_tot, (gb_tot if b is not None else None), None, None, None, None, None

    @staticmethod
    def _vj_acc(csr, W, b, no_graph, no_control, drop, gW_tot, gb_tot):
        """the two closures of _sweep_step.  With dropout K is the masked K' = relu(z) * m, m in {0, s}: J^T g = s * (the p = 0 closed
        form masked by K'), so s multiplies the alpha of the transposed SpMM and the scale of the parameter gradients"""
        s = 1.0 if drop is None else _dropout.scale(drop[0])
        vj = lambda u, K, gk, alpha: _FixedGridSolve._vjp(csr, u, K, gk, W, b, no_graph, no_control, alpha * s)

        def acc(gW, gb, scale):
            if gW is not None:
                gW_tot.add_(gW, alpha=scale * s)
                gb_tot.add_(gb, alpha=scale * s)
        return vj, acc


def _decoder_acc(Wd, needs_W, needs_b):
    """the fp64 accumulator of the decoder's gradients over a reverse sweep (hip.readout_bwd), or None when neither is wanted"""
    if not (needs_W or needs_b):
        return None
    C, H = Wd.shape
    return torch.zeros(C * H + C, dtype=torch.float64, device=Wd.device)


def _decoder_grads(acc, Wd, needs_W, needs_b):
    """(g_Wd, g_bd): the accumulator rounded to float32 once, after the last tick"""
    if acc is None:
        return None, None
    C, H = Wd.shape
    f = acc.to(torch.float32)
    return (f[:C * H].view(C, H) if needs_W else None), (f[C * H:] if needs_b else None)


class _FixedGridSolveReadout(torch.autograd.Function):
    """_FixedGridSolve with the decoder Linear(Wd, bd) of every tick inside the node (odeint's `readout` under a gradient): the output
    is the decoded solution (T, N, C), hip.linear of the trajectory; the reverse sweep takes the (T, N, C) gradient and forms tick i's
    g[i] . Wd inside the pass that adds it (hip.readout_bwd in _sweep_step's last combination) - the (T, N, H) gradient of the
    trajectory is never written - and accumulates the decoder's own gradients from the stored states on the way."""

    @staticmethod
    def forward(ctx, y0, W, b, Wd, bd, csr, flags, method, dts, drop=None):
        out = _FixedGridSolve._solve(ctx, y0, W, b, csr, flags, method, dts, drop)
        ctx.save_for_backward(out, W, b, Wd)
        return hip.linear(out, Wd, bd)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        out, W, b, Wd = ctx.saved_tensors
        csr, no_graph, no_control, method, dts, drop = ctx.meta
        g = g.contiguous()
        n_ticks = len(dts)
        H = out.shape[2]
        needs = ctx.needs_input_grad
        dacc = _decoder_acc(Wd, needs[3], needs[4])
        a = hip.readout_bwd(g[n_ticks], Wd, y=out[n_ticks], acc=dacc)
        gW_tot = torch.zeros((H, H), dtype=torch.float32, device=out.device) if not no_control else None
        gb_tot = torch.zeros((H,), dtype=torch.float32, device=out.device) if not no_control else None
        vj, acc = _FixedGridSolve._vj_acc(csr, W, b, no_graph, no_control, drop, gW_tot, gb_tot)
        for i in range(n_ticks - 1, -1, -1):
            st = []
            scratch = torch.empty_like(out[0])
            _FixedGridSolve._step(csr, out[i], W, b, no_graph, no_control, method, dts[i], scratch, keep=st,
                                  drop=_FixedGridSolve._drop_at(drop, method, i))
            a = _FixedGridSolve._sweep_step(method, dts[i], st, a, vj, acc,
                                            lambda base, gus, i=i: hip.readout_bwd(g[i], Wd, y=out[i], base=base, addends=gus, acc=dacc))
        gWd, gbd = _decoder_grads(dacc, Wd, needs[3], needs[4])
        return a, gW_tot, (gb_tot if b is not None else None), gWd, gbd, None, None, None, None, None


class _SubstepSolve(torch.autograd.Function):
    """_FixedGridSolve on a grid finer than the ticks (options={'step_size': h}; core.FixedPlan) WITHOUT a record per grid step:
      forward   the same fused launches, step after step; kept are the ticks (the output) and the state each tick interval starts
                from - the output panel itself where the interval's last tick coincides with the end of its step, else one panel;
      backward  one tick interval at a time, last first: the interval is run again from its start by the same launches, this time
                keeping the stages of its steps, then swept backwards in closed form (_FixedGridSolve._sweep_step).  The gradient
                of a tick enters at the end of the step that reported it (the VJP of ops.tick_emit is the identity).
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
            _FixedGridSolve._step(csr, y, W, b, no_graph, no_control, method, float(plan.dts[i]), dst, keep=st,
                                  drop=_FixedGridSolve._drop_at(drop, method, i))
            if keep is not None:
                keep.append(st)
            y = dst
        return y

    @staticmethod
    def _solve(ctx, y0, W, b, csr, flags, method, plan, drop):
        """the forward launches -> (the ticks, the interval starts that are no tick); ctx.meta set"""
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
        return out, own

    @staticmethod
    def forward(ctx, y0, W, b, csr, flags, method, plan, drop=None):
        out, own = _SubstepSolve._solve(ctx, y0, W, b, csr, flags, method, plan, drop)
        ctx.save_for_backward(out, W, b, *own)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        out, W, b, *own = ctx.saved_tensors
        g = g.contiguous()

        def enter(a, ticks):
            """the adjoint `a` (None: nothing yet) plus the gradients of the ticks reported at this state"""
            gs = [g[j] for j in ticks]
            if a is None:
                a, gs = gs[0], gs[1:]
            for q in range(0, len(gs), 8):
                a = hip.lincomb(gs[q:q + 8], [1.0] * len(gs[q:q + 8]), y0=a)
            return a
        return _SubstepSolve._reverse(ctx, out, W, b, own, enter) + (None, None, None, None, None)

    @staticmethod
    def _reverse(ctx, out, W, b, own, enter):
        """(g_y0, g_W, g_b): the tick intervals last first; enter(a, ticks) adds the gradients of the listed ticks to the adjoint"""
        csr, no_graph, no_control, method, plan, segs, starts, drop = ctx.meta
        H = out.shape[2]
        gW_tot = torch.zeros((H, H), dtype=torch.float32, device=out.device) if not no_control else None
        gb_tot = torch.zeros((H,), dtype=torch.float32, device=out.device) if not no_control else None
        vj, acc = _FixedGridSolve._vj_acc(csr, W, b, no_graph, no_control, drop, gW_tot, gb_tot)
        a = None
        for (lo, hi), (kind, idx) in zip(reversed(segs), reversed(starts)):
            a = enter(a, [e[0] for e in plan.emits[hi]])                 # the ticks this interval's last step reported
            y = out[idx] if kind == 'out' else own[idx]
            keep = []
            _SubstepSolve._run(csr, y, W, b, no_graph, no_control, method, plan, lo, hi, torch.empty_like(out[0]), keep=keep, drop=drop)
            for i in range(hi, lo - 1, -1):
                a = _FixedGridSolve._sweep_step(method, float(plan.dts[i]), keep.pop(), a, vj, acc, [])
        if a is None:
            a = torch.zeros_like(out[0])
        a = enter(a, [0])                                               # the first tick is y0 itself
        return a, gW_tot, (gb_tot if b is not None else None)


class _SubstepSolveReadout(torch.autograd.Function):
    """_SubstepSolve with the decoder of every tick inside the node, as _FixedGridSolveReadout: a tick's gradient enters the adjoint
    at the end of the step that reported it, one hip.readout_bwd call per tick (an interval's last step may report several)."""

    @staticmethod
    def forward(ctx, y0, W, b, Wd, bd, csr, flags, method, plan, drop=None):
        out, own = _SubstepSolve._solve(ctx, y0, W, b, csr, flags, method, plan, drop)
        ctx.save_for_backward(out, W, b, Wd, *own)
        return hip.linear(out, Wd, bd)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        out, W, b, Wd, *own = ctx.saved_tensors
        g = g.contiguous()
        needs = ctx.needs_input_grad
        dacc = _decoder_acc(Wd, needs[3], needs[4])

        def enter(a, ticks):
            for j in ticks:
                a = hip.readout_bwd(g[j], Wd, y=out[j], base=a, acc=dacc)
            return a
        ga, gW, gb = _SubstepSolve._reverse(ctx, out, W, b, own, enter)
        gWd, gbd = _decoder_grads(dacc, Wd, needs[3], needs[4])
        return ga, gW, gb, gWd, gbd, None, None, None, None, None


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
        drop = (float(odefunc.dropout), stream.seed, stream.take(n_steps * _FixedGridSolve.EVALS[method]))
    y0 = _lib.require_device(y0, 'state y0').contiguous()
    W, b = odefunc.wt.weight, odefunc.wt.bias
    if plan is not None:                                      # the step_size option: checkpointed per tick interval
        if readout is not None:
            return _SubstepSolveReadout.apply(y0, W, b, readout[0], readout[1], csr, flags, method, plan, drop)
        return _SubstepSolve.apply(y0, W, b, csr, flags, method, plan, drop)
    tt = core.host_grid(t).to(y0.dtype)
    dts = (tt[1:] - tt[:-1]).tolist()
    if drop is None:                                          # (the C++ tape has no dropout form)
        from . import tape
        sol = tape.fixed_grid(y0, W, b, csr, flags, method, dts, readout=readout)
        if sol is not None:
            return sol
    if readout is not None:
        return _FixedGridSolveReadout.apply(y0, W, b, readout[0], readout[1], csr, flags, method, dts, drop)
    return _FixedGridSolve.apply(y0, W, b, csr, flags, method, dts, drop)


def _small_solve_with_grad(odefunc, y0, t, method='euler', plan=None):
    """The one-launch training path when the library supports the shape (H <= 31, the state and three work panels in one
    CU's LDS: the reference's README commands), else None - the caller falls back to the per-step autograd path."""
    from ...csr import as_csr
    if t.requires_grad or not _lib.env_on('NDCN_SOLVE_SMALL_GRAD') or t.numel() < 2:
        return None
    lib = _lib.load()
    H = odefunc.hidden_size
    flags = _lib.F_RELU | (_lib.F_NO_GRAPH if odefunc.no_graph else 0) | (_lib.F_NO_CONTROL if odefunc.no_control else 0)
    csr = None
    if not odefunc.no_graph:
        csr = as_csr(odefunc.A)
        if csr.device != y0.device or csr.shape[0] != y0.shape[0]:
            return None
    view = csr.view_ref() if csr is not None else ctypes.byref(_lib.empty_csr(y0.shape[0]))
    if not lib.ndcn_solve_small_supported(view, H, flags, _lib.METHODS[method], 1):
        return None
    if method != 'euler' and not _lib.env_on('NDCN_SOLVE_SMALL_RK_GRAD'):
        return None
    core.assert_increasing(t)
    if plan is not None:
        # the step_size option: the one-launch pair on the explicit grid into a scratch trajectory (kilobytes per step at sizes that
        # fit one compute unit), the ticks gathered from it - coincident ticks are its rows, the others pass through tick_emit
        from ...autograd_ops import autograd_ops
        fine = _SmallEulerSolve.apply(_lib.require_device(y0, 'state y0').contiguous(), odefunc.wt.weight, odefunc.wt.bias, csr, flags,
                                      plan.dts.tolist(), method)
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
    return _SmallEulerSolve.apply(_lib.require_device(y0, 'state y0').contiguous(), odefunc.wt.weight, odefunc.wt.bias, csr, flags, dts, method)


# ---------------------------------------------------------------------------------------------------
# device-resident path
# ---------------------------------------------------------------------------------------------------

def _dopri5_tape_route(user_func, tensor_input, y0, t_user, method, options):
    """(plain, taped) of a solve that needs a gradient.  plain: dopri5 over a plain ODEFunc whose evaluations are deterministic - the
    per-operation graph may fuse its stage algebra into them; taped: the solve runs on the native tape (csrc/tape.hip) - a plain one
    where the tape applies, and with NDCN_TAPE_DROPOUT=1 also one with an ACTIVE dropout (training mode, 0 < p < 1: the tape's launches
    carry the mask, ndcn_tape_dopri5_drop_f32; the fused per-operation nodes do not, so `plain` stays False there)."""
    if method != 'dopri5':
        return False, False
    from . import tape
    plain = _device_resident_ok(user_func, tensor_input, y0, t_user, method, options) and _small_operator(user_func, y0[0]) is not None
    ok = plain or (tape.dropout_enabled() and _device_resident_ok(user_func, tensor_input, y0, t_user, method, options, allow_dropout=True)
                   and _small_operator(user_func, y0[0]) is not None)
    return plain, bool(ok and tape.applicable(user_func, y0[0], t_user))


def _device_resident_ok(user_func, tensor_input, y0, t, method, options, allow_dropout=False, allow_truth=False):
    """allow_dropout: the caller (the fixed-grid training path; the dopri5 tape under NDCN_TAPE_DROPOUT=1) takes an ACTIVE dropout,
    0 < p < 1 in training mode, too.
    allow_truth: the caller (the solve without a gradient) takes the ground-truth dynamics of ndcn_amd.truth, too - exactly those
    classes, on a float32 (N, 1) state that lives with the operator."""
    from ...neural_dynamics import ODEFunc
    if not tensor_input:
        return False
    y = y0[0]
    if allow_truth and type(user_func) in TRUTH_CLASSES:
        from ...csr import as_csr
        op = user_func.ndcn_dynamics()[0]
        if torch.is_grad_enabled() and torch.is_tensor(op) and op.requires_grad:     # (a gradient is asked of the operator)
            return False
        csr = as_csr(op)
        if y.dtype != torch.float32 or y.dim() != 2 or y.shape[1] != 1 or csr.device != y.device or \
                tuple(csr.shape) != (y.shape[0], y.shape[0]):
            return False
    elif type(user_func) is not ODEFunc:
        return False
    elif y.dim() != 2 or y.shape[1] != user_func.hidden_size:
        return False
    elif user_func.training and user_func.dropout > 0 and not (allow_dropout and _dropout.is_active(user_func)):
        return False
    if method in core.GRID_METHODS:
        if set(options) - {'step_size', 'max_order'}:         # (odeint hands over what core.fixed_options left)
            return False
    elif set(options) - set(core.DOPRI5_OPTIONS) or (method != 'dopri5' and options):
        return False
    if options.get('first_step') is not None:                  # dopri5.py:82: then 0.01 is used; host logic handles it
        return False
    th = core.host_grid(t)
    if bool((th[1:] < th[:-1]).any()):          # decreasing grids go through the generic sign flip
        return False
    return method != 'adams'                    # adams steps through the host logic (core.Adams) over the panel kernels


class DeviceSolver:
    """RAII wrapper of ndcn_solver_* for one (ODEFunc, method) pair - or one of the ground-truth dynamics of ndcn_amd.truth in
    ODEFunc's place (an N x 1 state: the descriptor's `dyn` field) -; the workspace is a torch allocation."""

    def __init__(self, odefunc, n_rows, method, rtol=1e-7, atol=1e-9, max_num_steps=2 ** 31 - 1, use_graph=False,
                 safety=core.SAFETY, ifactor=core.IFACTOR, dfactor=core.DFACTOR, shard=None):
        """shard: a ndcn_amd.sharding.DeviceShard - this rank's part of a node-range sharded graph; the operator is then
        the shard's (own rows, [own | halo] columns) and `odefunc.A` is ignored."""
        from ...csr import as_csr
        self.lib = _lib.load()
        if type(odefunc) in TRUTH_CLASSES:
            self._init_truth(odefunc, n_rows, method, rtol, atol, max_num_steps, use_graph, safety, ifactor, dfactor, shard)
            return
        H = odefunc.hidden_size
        flags = _lib.F_RELU | (_lib.F_NO_GRAPH if odefunc.no_graph else 0) | (_lib.F_NO_CONTROL if odefunc.no_control else 0)
        dev = odefunc.wt.weight.device
        self.csr = None
        if shard is not None:
            csr = shard.operator(H)
            assert csr.shape[0] == n_rows
            view = csr.view()
            self._keep = (csr, shard)
        elif odefunc.no_graph:
            view = _lib.empty_csr(n_rows)
            self._keep = ()
        else:
            csr = as_csr(odefunc.A)
            if csr.device != dev:
                raise _lib.NdcnHipError(_lib.EINVAL, 'operator on %s, weights on %s' % (csr.device, dev))
            assert csr.shape[0] == n_rows, 'operator has %d rows, state has %d' % (csr.shape[0], n_rows)
            csr.ensure_plans(H)
            view = csr.view()
            self._keep = (csr,)
            self.csr = csr
        W = odefunc.wt.weight.detach().contiguous()
        b = odefunc.wt.bias.detach().contiguous() if odefunc.wt.bias is not None else None
        _lib.require_device(W, 'weight')
        self._keep += (W, b)
        self.desc = _lib.SolverDesc(_lib.METHODS[method], H, flags, 1 if use_graph else 0, view,
                                    W.data_ptr(), b.data_ptr() if b is not None else None,
                                    float(rtol), float(atol), int(max_num_steps), float(safety), float(ifactor),
                                    float(dfactor), shard.view_ptr(H) if shard is not None else None)
        self._create(dev, (n_rows, H))

    def _init_truth(self, module, n_rows, method, rtol, atol, max_num_steps, use_graph, safety, ifactor, dfactor, shard):
        """the descriptor of a truth solve: H = 1, no weights, the module's operator, kind and scalars in `dyn`"""
        from ...csr import as_csr
        assert shard is None, 'the truth dynamics have no sharded form'
        op, kind, params = module.ndcn_dynamics()
        csr = as_csr(op)
        assert csr.shape[0] == n_rows, 'operator has %d rows, state has %d' % (csr.shape[0], n_rows)
        self.csr = csr
        self._dyn = _lib.dynamics(kind, params)
        self._keep = (csr, self._dyn)
        self.desc = _lib.SolverDesc(_lib.METHODS[method], 1, 0, 1 if use_graph else 0, csr.view(), None, None, float(rtol), float(atol),
                                    int(max_num_steps), float(safety), float(ifactor), float(dfactor), None, ctypes.pointer(self._dyn))
        self._create(csr.device, (n_rows, 1))

    def _create(self, dev, shape):
        self.device = dev
        self.shape = shape
        nbytes = int(self.lib.ndcn_solver_workspace_bytes(ctypes.byref(self.desc)))
        self.workspace = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self.handle = ctypes.c_void_p()
        self._pid = os.getpid()
        with torch.cuda.device(dev):
            _lib.check(self.lib.ndcn_solver_create(ctypes.byref(self.desc), _lib.ptr(self.workspace), nbytes,
                                                   ctypes.byref(self.handle)))

    def begin(self, y0, t0, borrow=False):
        """borrow=True (ndcn_solver_begin_borrowed): dopri5 reads y0 in place instead of copying it - the caller leaves
        the tensor alone until the solve is over and never passes an `out` that overlaps it (this object keeps it alive)."""
        y0 = _lib.require_device(y0, 'state y0').contiguous()
        assert tuple(y0.shape) == self.shape
        self._y0 = y0 if borrow else None
        entry = self.lib.ndcn_solver_begin_borrowed if borrow else self.lib.ndcn_solver_begin
        with torch.cuda.device(self.device):
            _lib.check(entry(self.handle, _lib.ptr(y0), float(t0), _lib.stream_ptr()))

    def advance(self, next_t, out=None, step_budget=0):
        """Returns True when next_t was reached (and `out` written), False when the step budget ran out."""
        with torch.cuda.device(self.device):
            rc = _lib.check(self.lib.ndcn_solver_advance(self.handle, float(next_t), _lib.ptr(out), int(step_budget),
                                                         _lib.stream_ptr()))
        return rc == 0

    def advance_many(self, ticks, out):
        """All `ticks` in one library call; out: (len(ticks), n_rows, H) contiguous."""
        assert out.is_contiguous() and tuple(out.shape) == (len(ticks),) + self.shape
        arr = (ctypes.c_double * len(ticks))(*[float(v) for v in ticks])
        with torch.cuda.device(self.device):
            _lib.check(self.lib.ndcn_solver_advance_many(self.handle, arr, len(ticks), _lib.ptr(out), _lib.stream_ptr()))

    def advance_many_readout(self, ticks, weight, bias, out, scratch):
        """advance_many with Linear(weight (C, H), bias (C,) or None) applied to every tick inside the library: out is
        (len(ticks), n_rows, C) and no hidden tick panel is stored; scratch: room for two n_rows x H panels.  Returns False where the
        library declines (NDCN_EINVAL: a sharded solver, H neither in 64..512 nor one of 16, 20, .. 60, C outside 1..15, a state that
        the one-launch solve takes)
        - nothing has been advanced then.  With no ticks (out and scratch may be None, before begin too) it only asks that question."""
        C = weight.shape[0]
        assert weight.is_contiguous() and weight.shape[1] == self.shape[1] and (bias is None or bias.is_contiguous())
        if len(ticks):
            assert out.is_contiguous() and tuple(out.shape) == (len(ticks), self.shape[0], C)
            assert scratch.is_contiguous() and scratch.numel() >= 2 * self.shape[0] * self.shape[1]
        arr = (ctypes.c_double * max(len(ticks), 1))(*[float(v) for v in ticks])
        with torch.cuda.device(self.device):
            rc = self.lib.ndcn_solver_advance_many_readout(self.handle, arr, len(ticks), _lib.ptr(weight), _lib.ptr(bias), C,
                                                           _lib.ptr(out), _lib.ptr(scratch), _lib.stream_ptr())
        if rc == _lib.EINVAL:
            return False
        _lib.check(rc)
        return True

    def advance_grid(self, plan, out):
        """A sub-stepped fixed grid (core.FixedPlan) in one library call: every step of plan.grid with the state inside the solver,
        out: (len(plan.t) - 1, n_rows, H) contiguous - the ticks after the first."""
        n_emit = len(plan.t) - 1
        assert out.is_contiguous() and tuple(out.shape) == (n_emit,) + self.shape
        grid = (ctypes.c_float * len(plan.grid))(*plan.grid.tolist())
        steps = (ctypes.c_int64 * n_emit)(*plan.tick_step[1:].tolist())
        times = (ctypes.c_float * n_emit)(*plan.t[1:].tolist())
        with torch.cuda.device(self.device):
            _lib.check(self.lib.ndcn_solver_advance_grid(self.handle, grid, len(plan.grid), steps, times, n_emit, _lib.ptr(out),
                                                         _lib.stream_ptr()))

    def stats(self):
        buf = (ctypes.c_double * 6)()
        _lib.check(self.lib.ndcn_solver_stats(self.handle, buf))
        keys = ('steps', 'accepted', 'nfe', 't1', 'dt_next', 'last_ratio')
        return dict(zip(keys, list(buf)))

    def steplog(self):
        n = int(self.lib.ndcn_solver_steplog(self.handle, None, 0))
        buf = (ctypes.c_double * (5 * max(n, 1)))()
        self.lib.ndcn_solver_steplog(self.handle, buf, n)
        return [tuple(buf[5 * i:5 * i + 5]) for i in range(n)]

    def close(self):
        if self.handle and self._pid == os.getpid():          # (never from a fork()ed copy of this object)
            self.lib.ndcn_solver_destroy(self.handle)
        self.handle = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _small_operator(odefunc, y0):
    """(csr or None, ctypes view ref, flags) of an ODEFunc for the ndcn_solve_small_* entry points, or None when the operator
    does not live with the state."""
    from ...csr import as_csr
    flags = _lib.F_RELU | (_lib.F_NO_GRAPH if odefunc.no_graph else 0) | (_lib.F_NO_CONTROL if odefunc.no_control else 0)
    if odefunc.no_graph:
        return None, ctypes.byref(_lib.empty_csr(y0.shape[0])), flags
    csr = as_csr(odefunc.A)
    if csr.device != y0.device or csr.shape[0] != y0.shape[0]:
        return None
    return csr, csr.view_ref(), flags


def _explicit_adams_solve(odefunc, y0, t, plan, max_order):
    """The whole explicit_adams solve of a plain ODEFunc inside the library (ndcn_solve_explicit_adams_f32: RK4 warm-up, then one
    right-hand side and one ndcn_ab_step_f32 per grid step, ticks through ndcn_tick_emit_f32), enqueued on the current stream without
    a read-back.  None where the entry point has no form: no_graph / no_control, an operator that does not live with the state, a
    max_order the reference itself fails on."""
    import numpy as np
    if odefunc.no_graph or odefunc.no_control or max_order < 2:
        return None
    op = _small_operator(odefunc, y0)
    if op is None:
        return None
    csr, view, flags = op
    core.assert_increasing(t)
    if plan is None:
        plan = core.fixed_plan(core.host_grid(t).to(y0.dtype).numpy())         # solvers.py:81: the grid is t in the state dtype
    lib = _lib.load()
    H = odefunc.hidden_size
    n_ticks = len(plan.t)
    out = torch.empty((n_ticks,) + tuple(y0.shape), dtype=torch.float32, device=y0.device)
    out[0].copy_(y0)
    n_steps, n_emit = len(plan.dts), n_ticks - 1
    if n_steps == 0 or y0.numel() == 0:
        return out
    csr.ensure_plans(H)
    view = csr.view_ref()
    W = _lib.require_device(odefunc.wt.weight.detach().contiguous(), 'weight')
    b = None if odefunc.wt.bias is None else odefunc.wt.bias.detach().contiguous()
    dts = (ctypes.c_float * n_steps)(*plan.dts.tolist())
    steps = (ctypes.c_int64 * max(n_emit, 1))(*plan.tick_step[1:].tolist())
    same = (ctypes.c_int * max(n_emit, 1))(*[int(v) for v in plan.tick_coincident[1:]])
    offs = (ctypes.c_float * max(n_emit, 1))(*[float(np.float32(plan.t[j] - plan.grid[plan.tick_step[j]])) for j in range(1, n_ticks)])
    nbytes = int(lib.ndcn_explicit_adams_workspace_bytes(y0.shape[0], H, max_order))
    workspace = torch.empty(nbytes, dtype=torch.uint8, device=y0.device)
    with torch.cuda.device(y0.device):
        _lib.check(lib.ndcn_solve_explicit_adams_f32(view, _lib.ptr(W), _lib.ptr(b), H, flags, _lib.ptr(out[0]), dts, n_steps, steps, same,
                                                     offs, n_emit, max_order, _lib.ptr(out[1:]) if n_emit else None, _lib.ptr(workspace),
                                                     nbytes, _lib.stream_ptr()))
    # (the workspace goes back to torch's stream-ordered allocator: a later allocation on this stream is ordered behind the solve)
    return out


def _small_solve(odefunc, y0, tt, method, plan=None):
    """ndcn_solve_small_f32 without a solver object (no workspace, no host synchronisation): the inference counterpart of
    _SmallEulerSolve.  tt: the time grid as Python floats ALREADY rounded to the state dtype (solvers.py:81).  plan (the step_size
    option): ndcn_solve_small_grid_f32 - the steps of plan.grid, still one launch per 128 steps, only the ticks written."""
    import numpy as np
    if type(odefunc) in TRUTH_CLASSES:                        # (the one-launch solve is ODEFunc's)
        return None
    op = _small_operator(odefunc, y0)
    if op is None:
        return None
    csr, view, flags = op
    lib = _lib.load()
    H = odefunc.hidden_size
    if not lib.ndcn_solve_small_supported(view, H, flags, _lib.METHODS[method], 0):
        return None
    g = np.asarray(tt, dtype=np.float32)
    dts = (g[1:] - g[:-1]).tolist()
    out = torch.empty((len(tt),) + tuple(y0.shape), dtype=torch.float32, device=y0.device)
    out[0].copy_(y0)
    no_control = bool(flags & _lib.F_NO_CONTROL)
    W = None if no_control else _lib.require_device(odefunc.wt.weight.detach().contiguous(), 'weight')
    b = None if (no_control or odefunc.wt.bias is None) else odefunc.wt.bias.detach().contiguous()
    if plan is not None:
        n_steps, n_emit = len(plan.dts), len(tt) - 1
        arr = (ctypes.c_float * n_steps)(*plan.dts.tolist())
        steps = (ctypes.c_int64 * n_emit)(*plan.tick_step[1:].tolist())
        same = (ctypes.c_int * n_emit)(*[int(v) for v in plan.tick_coincident[1:]])
        y_end = torch.empty_like(out[0]) if n_steps > 128 else None
        with torch.cuda.device(y0.device):
            _lib.check(lib.ndcn_solve_small_grid_f32(view, _lib.ptr(W), _lib.ptr(b), H, flags, _lib.METHODS[method], _lib.ptr(out[0]), arr,
                                                     n_steps, steps, same, n_emit, _lib.ptr(out[1:]), _lib.ptr(y_end), _lib.stream_ptr()))
        return out
    arr = (ctypes.c_float * len(dts))(*dts)
    with torch.cuda.device(y0.device):
        _lib.check(lib.ndcn_solve_small_f32(view, _lib.ptr(W), _lib.ptr(b), H, flags, _lib.METHODS[method], _lib.ptr(out[0]), arr,
                                            len(dts), _lib.ptr(out[1:]), _lib.stream_ptr()))
    return out


# Reference-sized solves (the README commands: 400 x 20) spend a third of their time CREATING the solver - workspace, streams,
# events and above all the capture + instantiation of the per-step hipGraph (~0.5 ms of a 1.7 ms dopri5 solve, rocprofv3 kernel
# trace) - and every odeint call of a training loop's evaluation pass builds the same one again.  Solvers of launch-bound sizes are
# therefore kept (a handful, least recently used out) and re-begun: ndcn_solver_begin resets the state, the captured graph reads the
# weights, the operator and the workspace through pointers that the key pins.
_SOLVERS = collections.OrderedDict()
_SOLVER_CACHE_MAX_ELEMS = 1 << 20
_SOLVER_CACHE_SIZE = 4


def _cached_solver(odefunc, y0, method, rtol, atol, opt, use_graph):
    """(solver, key or None): a kept solver re-used when everything its captured graph points at is unchanged."""
    def make():
        return DeviceSolver(odefunc, y0.shape[0], method, rtol, atol, opt.get('max_num_steps', 2 ** 31 - 1), use_graph=use_graph,
                            safety=opt.get('safety', core.SAFETY), ifactor=opt.get('ifactor', core.IFACTOR),
                            dfactor=opt.get('dfactor', core.DFACTOR))
    if not use_graph or y0.numel() > _SOLVER_CACHE_MAX_ELEMS:
        return make(), None
    from ...csr import as_csr
    solve = (tuple(y0.shape), method, float(rtol), float(atol), tuple(sorted((k, v) for k, v in opt.items() if v is not None)),
             y0.device.index, torch.cuda.current_stream(y0.device).cuda_stream)
    truth = type(odefunc) in TRUTH_CLASSES
    if truth:
        # everything the descriptor is built from: the class, its scalars and the operator the module's attribute converts to NOW
        # (a module is made per solve - drivers/dynamics.py - so the kept solver belongs to the operator, not to the module)
        op, _, params = odefunc.ndcn_dynamics()
        owner = current = as_csr(op)
        key = (type(odefunc), params, id(owner)) + solve
    else:
        W, b = odefunc.wt.weight, odefunc.wt.bias
        owner = odefunc
        key = (id(odefunc), W.data_ptr(), None if b is None else b.data_ptr(), id(getattr(odefunc, 'A', None))) + solve + \
            (bool(odefunc.no_graph), bool(odefunc.no_control))
    hit = _SOLVERS.get(key)
    if hit is not None and (truth or not odefunc.no_graph):
        # id(A) names an object, not its contents: an in-place write to A re-converts (csr.as_csr keys on A._version), and a new
        # tensor may re-use a freed one's id - the kept solver's captured graph would go on reading the OLD operator arrays that
        # its _keep holds alive.  The CsrOperator the solver was built on must be the one the operator converts to now.
        if not truth:
            current = as_csr(odefunc.A)
        if getattr(hit[1], 'csr', None) is not current:
            del _SOLVERS[key]
            if not getattr(hit[1], '_in_use', False):
                hit[1].close()
            hit = None
    if hit is not None and hit[0]() is owner and not getattr(hit[1], '_in_use', False) and hit[1].handle:
        _SOLVERS.move_to_end(key)
        hit[1]._in_use = True
        return hit[1], key
    solver = make()
    solver._in_use = True
    if hit is None:
        _SOLVERS[key] = (weakref.ref(owner), solver)
        while len(_SOLVERS) > _SOLVER_CACHE_SIZE:
            _, (_, old) = _SOLVERS.popitem(last=False)
            if not getattr(old, '_in_use', False):
                old.close()
        return solver, key
    return solver, None                                      # the kept one is busy (another thread): a solver of its own


def _device_resident_readout(solver, y0, tt, Wd, bd):
    """The decoded solution (len(tt), N, C) through ndcn_solver_advance_many_readout, or None where the library declines.  The hidden
    state lives in the solver's workspace and in two scratch panels that are freed on return."""
    C = Wd.shape[0]
    if not solver.advance_many_readout([], Wd, bd, None, None):   # asked before begin: a declined solve pays nothing twice
        return None
    out = torch.empty((len(tt), y0.shape[0], C), dtype=torch.float32, device=y0.device)
    scratch = torch.empty((2,) + tuple(y0.shape), dtype=torch.float32, device=y0.device)
    y0 = y0.contiguous()
    solver.begin(y0, tt[0], borrow=True)                     # dopri5 reads the caller's y0 in place; nothing here writes it
    try:
        if not solver.advance_many_readout(tt[1:], Wd, bd, out[1:], scratch):
            return None
    except _lib.NdcnHipError as e:
        if e.code in (_lib.ENONFINITE, _lib.EUNDERFLOW, _lib.EMAXSTEPS, _lib.ESTATE):
            raise AssertionError(str(e)) from None             # the reference raises AssertionError here
        raise
    out[0].copy_(hip.linear(y0, Wd, bd))
    torch.cuda.current_stream().synchronize()                # the scratch is released here, the workspace by the caller
    return out


def _device_resident(odefunc, y0, t, rtol, atol, method, options, step_log, plan=None, readout=None):
    """(solution, decoded).  readout (weight, bias): with no gradient asked of them and no step_size plan the library decodes every
    tick inside the solve - decoded is True and the solution is (len(t), N, C); where it declines, the hidden solution is returned."""
    core.assert_increasing(t)
    tt = core.host_grid(t).to(torch.float64).tolist()
    if method != 'dopri5':
        # solvers.py:81: the fixed grid is t in the state dtype
        tt = core.host_grid(t).to(y0.dtype).to(torch.float64).tolist()
    if method != 'dopri5' and len(tt) > 1:
        out = _small_solve(odefunc, y0, tt, method, plan)       # a state that fits one compute unit: the whole grid in ONE launch
        if out is not None:
            return out, False
    fuse = False
    if readout is not None and plan is None and len(tt) > 1 and type(odefunc) not in TRUTH_CLASSES:
        Wd, bd = readout
        fuse = not (torch.is_grad_enabled() and (Wd.requires_grad or (bd is not None and bd.requires_grad))) and \
            Wd.dim() == 2 and Wd.shape[1] == y0.shape[1] and Wd.is_cuda and Wd.dtype == torch.float32
    # launch-bound sizes replay ONE captured hipGraph per step - a fixed-grid step, or one attempted dopri5 step - with the
    # step size in device memory (the library declines where a path has no replayable form)
    use_graph = y0.numel() <= GRAPH_MAX_ELEMS
    opt = core.dopri5_options(options, 1) if method == 'dopri5' else dict(options)      # (fixed grid: nothing, or the step size)
    solver, cache_key = _cached_solver(odefunc, y0, method, rtol, atol, opt, use_graph)
    try:
        if fuse:
            out = _device_resident_readout(solver, y0, tt, Wd.detach().contiguous(), None if bd is None else bd.detach().contiguous())
            if out is not None:
                if step_log is not None:
                    step_log.extend(solver.steplog())
                    step_log.append(('nfe', int(solver.stats()['nfe'])))
                return out, True
        out = torch.empty((len(tt),) + tuple(y0.shape), dtype=torch.float32, device=y0.device)
        out[0].copy_(y0)
        solver.begin(out[0], tt[0], borrow=True)           # the solution's first panel IS the initial state: read in place
        try:
            if len(tt) > 1 and plan is not None:
                solver.advance_grid(plan, out[1:])                 # the step_size option: every grid step inside the solver
            elif len(tt) > 1:
                solver.advance_many(tt[1:], out[1:])               # one library call for the whole time vector
        except _lib.NdcnHipError as e:
            if e.code in (_lib.ENONFINITE, _lib.EUNDERFLOW, _lib.EMAXSTEPS, _lib.ESTATE):
                raise AssertionError(str(e)) from None         # the reference raises AssertionError here
            raise
        if step_log is not None:
            step_log.extend(solver.steplog())
            step_log.append(('nfe', int(solver.stats()['nfe'])))
        torch.cuda.current_stream().synchronize()    # the workspace is released (or handed to the next solve) below
        return out, False
    finally:
        if cache_key is None:
            solver.close()
        else:
            solver._in_use = False
