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
from . import core, fixed_train
from .fixed_train import _small_operator

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
    or 64 <= H <= 512, C <= 15) and the (len(t), N, H) trajectory is never stored - dopri5, euler, midpoint and rk4 on the grid of `t`,
    and explicit_adams / fixed_adams on any of their grids, `step_size` included (ndcn_solve_explicit_adams_readout_f32 /
    ndcn_solve_fixed_adams_readout_f32: an Adams-Bashforth step that reports ticks decodes them in its own launch, RK4 warm-up steps
    and the corrector's steps decode the state they leave in the workspace; NDCN_ADAMS_READOUT=0 / hip.set_adams_readout(0) restores
    decode-after for these two methods); under a gradient, euler / midpoint / rk4 over ODEFunc on the fused-launch training
    path hold the decoder inside the solve's autograd node: the trajectory is stored once (the reverse sweep needs it) but the
    (len(t), N, H) gradient of it, which the Linear's own backward would write, is not - the sweep forms each tick's g . W where it
    adds it (ndcn_readout_bwd_f32); everywhere else the ordinary solve runs and the Linear is applied to its result - the
    values are the same bits either way, only the memory differs.  A tuple state raises ValueError.

    Without a gradient the device-resident solver evaluates f by one launch kind per solve (DeviceSolver.rhs_kind()).  Under
    hip.set_solver_mid / NDCN_SOLVER_MID (off by default) hidden widths 16..128 on more than 2^18 state elements, and the no_graph /
    no_control ablations below H = 256, take the one-launch kernels of csrc/rhs_mid.hip / rhs_abl.hip - dopri5, euler and rk4; solution,
    decoded ticks, step_log and nfe are bit for bit those of the switched-off solve."""
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
    method, AssertionError for a non-monotone t.  Deviations: dopri5 / adams / explicit_adams / fixed_adams / euler / midpoint / rk4 are
    provided (tsit5 raises NotImplementedError); the state must be float32 on a ROCm device;
    `step_log` (a list) optionally receives the dopri5 per-attempt log - for fixed_adams one (corrector iterations, converged) pair per
    grid step and ('nfe', evaluations).  Returns (solution, decoded): decoded is True when
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
    never leaves RK4; m < 2 fails as in the reference).  A plain ODEFunc that fixed_train._adams_admission admits (the decline reasons
    are stated there, once, for both methods) runs the whole solve inside the library: without a gradient _adams_solve
    (ndcn_solve_explicit_adams_f32: nothing is read back), under one and with NDCN_ADAMS_TRAIN=1 one autograd node per solve
    (fixed_train._ExplicitAdamsSolve, `readout` inside it as for rk4).  Everything else steps through core.py.

    fixed_adams is the reference's AdamsBashforthMoulton (fixed_adams.py:151-205): the same history, warm-up and predictor, then the
    Adams-Moulton corrector over the history and the evaluation at the step's end, iterated up to options={'max_iters': n} (default 4)
    times until EVERY element of the increment satisfies |dy_old - dy_new| < atol + rtol * max(|dy_old|, |dy_new|) - `rtol` and `atol`
    are this function's arguments (naming them in `options` is the reference's TypeError).  A step that does not converge writes the
    reference's warning line to stderr and drops the oldest evaluation of its history.  options={'implicit': False} is explicit_adams,
    bit for bit.  The routes are explicit_adams' own: inside the library ndcn_solve_fixed_adams_f32 (one 8-byte read-back per corrector
    iteration, the host decides whether to iterate again) and fixed_train._FixedAdamsSolve; everything else steps through core.py over
    ndcn_abm_predict_f32 / ndcn_abm_correct_f32 - under a gradient the iteration counts are constants of the graph.  A host state is
    refused here, where unsupported methods are, with an exception that is both NdcnHipError and NotImplementedError.
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
                                  '(dopri5, adams, explicit_adams, fixed_adams, euler, midpoint, rk4 are provided)' % method)
    if method == 'fixed_adams':
        for y in y0:
            _lib.require_device(y, 'state y0', error=_lib.NdcnHostStateError)
    method = SOLVERS[method]                     # KeyError for an unknown name, as the reference's dict lookup

    plan = None
    max_iters = core.ABM_MAX_ITERS
    if method in core.GRID_METHODS:
        options = core.fixed_options(method, options)       # solvers.py:39-53: warns about unknown names, ValueError for a grid_constructor
        if method == 'fixed_adams':
            max_iters = options.pop('max_iters')
            if not options.pop('implicit'):                 # fixed_adams.py:185: the corrector is skipped - AdamsBashforth's step
                method = 'explicit_adams'
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
            sol = fixed_train._small_solve_with_grad(user_func, y0[0], t, method, plan)                  # one launch forward, one backward
        if sol is None:
            # any size: fused launches forward, closed-form sweep backward - with `readout` the decoder inside the same node
            dec = fixed_train._readout_for_grad(readout, y0[0])
            sol = fixed_train._fixed_grid_with_grad(user_func, y0[0], t, method, plan, readout=dec)
            if sol is not None:
                return sol, dec is not None
        if sol is not None:
            return sol, False
    if needs_grad and method in ('explicit_adams', 'fixed_adams') and fixed_train.adams_train_enabled() and \
            _device_resident_ok(user_func, tensor_input, y0, t_user, method, options):
        # NDCN_ADAMS_TRAIN=1: one autograd node per solve - the library's loop forward (fixed_adams: the predictor-corrector loop, with a
        # record), its reverse sweep in closed form backward; what the node declines stays on the per-operation graph below
        dec = fixed_train._readout_for_grad(readout, y0[0])
        if method == 'explicit_adams':
            sol = fixed_train._explicit_adams_with_grad(user_func, y0[0], t, plan, options['max_order'], readout=dec)
        else:
            sol = fixed_train._fixed_adams_with_grad(user_func, y0[0], t, plan, options['max_order'], rtol, atol, max_iters, step_log, readout=dec)
        if sol is not None:
            return sol, dec is not None
    if needs_grad:
        from .autograd_path import odeint_with_grad
        plain, taped = _dopri5_tape_route(user_func, tensor_input, y0, t_user, method, options)
        if taped:
            # one autograd node per solve: the native tape (csrc/tape.hip) runs the launches below and their reverse pass itself
            from . import tape
            return tape.solve(user_func, y0[0], t, rtol, atol, options, step_log), False
        sol = odeint_with_grad(func, y0, t, rtol, atol, method, options, autonomous=_autonomous(user_func),
                               step_log=step_log, odefunc=user_func if plain else None, plan=plan, max_iters=max_iters)
    elif method == 'fixed_adams':
        out = None
        if _device_resident_ok(user_func, tensor_input, y0, t_user, method, options):
            out = _fixed_adams_solve(user_func, y0[0], t, plan, options['max_order'], rtol, atol, max_iters, step_log, readout)
        if out is not None:
            return out                                      # (solution, decoded)
        sol = core.integrate_fixed(hip, func, y0, t, method, autonomous=_autonomous(user_func), plan=plan, max_order=options['max_order'],
                                   max_iters=max_iters, rtol=rtol, atol=atol, step_log=step_log)
    elif method == 'explicit_adams':
        out = None
        if _device_resident_ok(user_func, tensor_input, y0, t_user, method, options):
            out = _explicit_adams_solve(user_func, y0[0], t, plan, options['max_order'], readout)
        if out is not None:
            return out                                      # (solution, decoded)
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
    ODEFunc's place (an N x 1 state: the descriptor's `dyn` field) -; the workspace is a torch allocation.  The library picks one launch
    kind per solver at creation (rhs_kind()); under hip.set_solver_mid hidden widths 16..128 beyond the narrow-panel sizes, and the
    no_graph / no_control ablations, take the one-launch kernels ('mid' / 'abl') with the same bits in every result."""

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
        flags = _lib.operator_flags(odefunc)
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

    def rhs_kind(self):
        """The launch kind this solver evaluates f with, chosen when it was created (ndcn_solver_rhs_kind): one of
        _lib.SOLVER_RHS_KINDS - 'mid' / 'abl', the one-launch kernels for hidden widths 16..128, only under hip.set_solver_mid."""
        return _lib.SOLVER_RHS_KINDS[_lib.check(self.lib.ndcn_solver_rhs_kind(self.handle))]

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


def _adams_decoder(readout, y0):
    """(Wd, bd) for the decoder inside the library's explicit_adams / fixed_adams solve (ndcn_solve_*_adams_readout_f32), or None: no
    readout, a gradient asked of it, a weight that is not a float32 device (C, H) tensor, a shape outside hip.adams_readout_route, or
    the switch off (NDCN_ADAMS_READOUT=0 / hip.set_adams_readout(0)) - the solve then stores the hidden ticks and odeint decodes them."""
    if readout is None:
        return None
    Wd, bd = readout
    if not torch.is_tensor(Wd) or Wd.dim() != 2 or (bd is not None and not torch.is_tensor(bd)):
        return None
    needs_grad = torch.is_grad_enabled() and (Wd.requires_grad or (bd is not None and bd.requires_grad))
    weight_ok = Wd.shape[1] == y0.shape[1] and Wd.device == y0.device and Wd.is_cuda and Wd.dtype == torch.float32 and \
        (bd is None or (bd.shape == (Wd.shape[0],) and bd.device == Wd.device and bd.dtype == torch.float32))
    if not hip.adams_readout_route(y0.shape[1], Wd.shape[0], weight_ok, needs_grad, hip.adams_readout_on()):
        return None
    return Wd.detach().contiguous(), None if bd is None else bd.detach().contiguous()


def _adams_solve(odefunc, y0, t, plan, max_order, readout, corrector=None):
    """(solution, decoded): the whole explicit_adams solve of a plain ODEFunc inside the library (ndcn_solve_explicit_adams_f32: RK4
    warm-up, then one right-hand side and one ndcn_ab_step_f32 per grid step, ticks through ndcn_tick_emit_f32), enqueued on the current
    stream without a read-back - or, with corrector = (rtol, atol, max_iters, step_log), the fixed_adams solve (ndcn_solve_fixed_adams_f32:
    the same launches, then per step one ndcn_abm_predict_f32 and up to max_iters x (right-hand side + ndcn_abm_correct_f32 + an 8-byte
    read-back)), reported through fixed_train._report_corrector.  With a `readout` that _adams_decoder admits, the *_readout_f32 form of
    either: the solution is (len(t), N, C), each tick decoded by the launch that forms it (fixed_adams: the accepted iterate of every
    reporting step; iteration counts, warning lines and step_log are those of the un-decoded solve), and no hidden tick is stored.
    None where the entry points have no form: fixed_train._adams_admission."""
    admitted = fixed_train._adams_admission(odefunc, y0, t, plan, max_order, corrector)
    if admitted is None:
        return None
    csr, flags, plan, y0 = admitted
    lib = _lib.load()
    H = odefunc.hidden_size
    dec = _adams_decoder(readout, y0)
    first = y0 if dec is None else hip.linear(y0, dec[0], dec[1])
    out = torch.empty((len(plan.t),) + tuple(first.shape), dtype=torch.float32, device=y0.device)
    out[0].copy_(first)
    dts, n_steps, steps, same, offs, n_emit = fixed_train.plan_arrays(plan)           # (named: the arrays outlive the call)
    if n_steps == 0 or y0.numel() == 0:
        if corrector is not None and corrector[3] is not None:
            corrector[3].extend([(0, True)] * n_steps + [('nfe', 0)])
        return out, dec is not None
    csr.ensure_plans(H)
    view = csr.view_ref()                                    # (after ensure_plans: the view is the handle's as of plan-building time)
    W = _lib.require_device(odefunc.wt.weight.detach().contiguous(), 'weight')
    b = None if odefunc.wt.bias is None else odefunc.wt.bias.detach().contiguous()
    size = lib.ndcn_explicit_adams_workspace_bytes if corrector is None else lib.ndcn_fixed_adams_workspace_bytes
    nbytes = int(size(y0.shape[0], H, max_order))
    workspace = torch.empty(nbytes, dtype=torch.uint8, device=y0.device)
    # the decoded form reads y0 itself, the hidden one the solution's first panel
    head = (view, _lib.ptr(W), _lib.ptr(b), H, flags, _lib.ptr(y0 if dec is not None else out[0]), dts, n_steps, steps, same, offs, n_emit,
            max_order)
    decoder = () if dec is None else (_lib.ptr(dec[0]), _lib.ptr(dec[1]), dec[0].shape[0])
    ticks = _lib.ptr(out[1:]) if n_emit else None
    with torch.cuda.device(y0.device):
        tail = (_lib.ptr(workspace), nbytes, _lib.stream_ptr())
        if corrector is None:
            if dec is None:
                _lib.check(lib.ndcn_solve_explicit_adams_f32(*head, ticks, *tail))
            else:
                _lib.check(lib.ndcn_solve_explicit_adams_readout_f32(*head, *decoder, ticks, *tail))
        else:
            rtol, atol, max_iters, step_log = corrector
            tol = (float(rtol), float(atol), max_iters)
            iters, conv = (ctypes.c_int * n_steps)(), (ctypes.c_int * n_steps)()
            if dec is None:
                _lib.check(lib.ndcn_solve_fixed_adams_f32(*head, *tol, ticks, iters, conv, *tail))
            else:
                _lib.check(lib.ndcn_solve_fixed_adams_readout_f32(*head, *tol, *decoder, ticks, iters, conv, *tail))
            fixed_train._report_corrector(step_log, iters, conv)
    # (the workspace goes back to torch's stream-ordered allocator: a later allocation on this stream is ordered behind the solve)
    return out, dec is not None


def _explicit_adams_solve(odefunc, y0, t, plan, max_order, readout=None):
    return _adams_solve(odefunc, y0, t, plan, max_order, readout)


def _fixed_adams_solve(odefunc, y0, t, plan, max_order, rtol, atol, max_iters, step_log=None, readout=None):
    return _adams_solve(odefunc, y0, t, plan, max_order, readout, (rtol, atol, max_iters, step_log))


def _small_solve(odefunc, y0, tt, method, plan=None):
    """ndcn_solve_small_f32 without a solver object (no workspace, no host synchronisation): the inference counterpart of
    fixed_train._SmallEulerSolve.  tt: the time grid as Python floats ALREADY rounded to the state dtype (solvers.py:81).  plan (the step_size
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
             y0.device.index, torch.cuda.current_stream(y0.device).cuda_stream,
             hip.solver_mid_mode())                            # (a solver keeps the launch kind, and the captured graph, it was created under)
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
