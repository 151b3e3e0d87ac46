"""Backpropagation through a dopri5 solve of a plain ODEFunc as two library calls (csrc/tape.hip).

The reference trains by autograd through odeint (heat_dynamics.py:313-334, dgnn.py:192-222): here `ndcn_tape_dopri5_f32` runs the
solve with the per-operation path's own launches and keeps every attempted step; `ndcn_tape_backward_f32` is its reverse pass - the
VJP kernels of the panel operations plus the hand-written adjoint of the step-size controller's scalar chain (which the reference
differentiates: dt, the initial step, the interpolation abscissa are tensors with history).  One autograd node per solve instead of
~130 (`autograd_path.integrate_dopri5_grad`, which stays the path of tuple states, plain callables, `t` with gradient and the A/B:
NDCN_GRAD_TAPE=0).

The forward record grows with the number of attempted steps (12 to 18 panels each).  NDCN_TAPE_BUDGET_MB bounds it: attempts past
the budget keep two panels each and the reverse pass re-forms the rest by the forward pass's launches (`ndcn_tape_dopri5_budget_f32`:
the same gradients bit for bit, six more evaluations per such attempt); unset, a solve whose record does not fit the device runs once
more with budget 0.  `last_record` says what the last solve kept.

An active dropout (training mode, 0 < p < 1) takes the tape under NDCN_TAPE_DROPOUT=1 (`ndcn_tape_dopri5_drop_f32`): the solve's
stream (ndcn_amd/dropout.py) gives the seed and the number of the first evaluation, the library numbers the evaluations as the
per-operation path makes them - the same masks, trajectory and step log bit for bit - and reports how many it consumed."""
import ctypes
import warnings

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from ... import _lib
from ... import dropout as _dropout
from ..._lib import check, ptr, stream_ptr

ALLOC_FN = ctypes.CFUNCTYPE(ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64)


# what the last tape solve recorded (ndcn_tape_record) and whether it was the second run after the record did not fit
last_record = {'full_panels': 0, 'thin_kept_panels': 0, 'ring_panels': 0, 'thin_attempts': 0, 'retried': False}
_retry_warned = False


def enabled():
    return _lib.env_on('NDCN_GRAD_TAPE') and _lib.env_str('NDCN_VJP', 'hip') != 'torch'


def dropout_enabled():
    """NDCN_TAPE_DROPOUT=1: a solve with an active dropout takes the tape too (default: the per-operation graph)"""
    return _lib.env_str('NDCN_TAPE_DROPOUT', '0') == '1'


class Tape:
    """Owner of one ndcn_tape and of the device memory it asked for (torch's caching allocator, on the solve's stream)."""

    def __init__(self, device):
        self.device = device
        self.blocks = []
        self.error = None
        self.handle = ctypes.c_void_p()
        self.cb = ALLOC_FN(self._alloc_cb)          # (kept: the library calls it until the reverse pass has run)

    def _alloc(self, ctx, nbytes):
        blk = torch.empty(int(nbytes), dtype=torch.uint8, device=self.device)
        self.blocks.append(blk)
        return blk.data_ptr()

    def _alloc_cb(self, ctx, nbytes):
        try:
            return self._alloc(ctx, nbytes)
        except Exception as e:                      # an exception cannot cross the C frames: the call fails with "no memory", then re-raised
            self.error = e
            return None

    def close(self):
        if self.handle:
            _lib.load().ndcn_tape_destroy(self.handle)
            self.handle = ctypes.c_void_p()
        self.blocks = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _TapeDopri5(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y0, W, b, op, ticks, rtol, atol, opts, step_log, budget, drop=None):
        """drop: None or (p, seed, number of the solve's first evaluation, the dropout stream to advance by what the solve consumed)"""
        csr, csr_t, flags, H = op
        lib = _lib.load()
        y0c = y0.detach().contiguous()
        Wc = W.detach().contiguous() if W is not None else None
        bc = b.detach().contiguous() if b is not None else None
        n_t = len(ticks)
        out = torch.empty((n_t,) + tuple(y0c.shape), dtype=torch.float32, device=y0c.device)
        tk = (ctypes.c_double * n_t)(*ticks)
        op_arr = (ctypes.c_double * 6)(*opts)
        view = csr.view_ref() if csr is not None else ctypes.byref(_lib.empty_csr(y0c.shape[0]))
        view_t = csr_t.view_ref() if csr_t is not None else None
        desc = _lib.dropout_desc(None if drop is None else drop[:3])       # (a retry runs with the SAME seed and first number)
        retried = False
        while True:
            tape = Tape(y0c.device)
            with torch.cuda.device(y0c.device):
                rc = lib.ndcn_tape_dopri5_drop_f32(view, view_t, ptr(Wc), ptr(bc), H, flags, ptr(y0c), tk, n_t, float(rtol), float(atol),
                                                   op_arr, ptr(out), ctypes.cast(tape.cb, ctypes.c_void_p), None,
                                                   ctypes.byref(tape.handle), stream_ptr(), budget, desc)
            if rc < 0 and budget < 0 and not retried and isinstance(tape.error, torch.cuda.OutOfMemoryError):
                # the unlimited record did not fit: its blocks go back to the allocator and the solve runs once more with every attempt
                # thin (a failure of that run is raised as it is)
                tape.close()
                del tape
                _warn_retry()
                retried, budget = True, 0
                continue
            break
        if tape.handle:
            rec = (ctypes.c_int64 * 4)()
            lib.ndcn_tape_record(tape.handle, rec)
            last_record.update(full_panels=int(rec[0]), thin_kept_panels=int(rec[1]), ring_panels=int(rec[2]), thin_attempts=int(rec[3]),
                               retried=retried)
        if drop is not None and tape.handle:
            drop[3].take(max(int(lib.ndcn_tape_evaluations(tape.handle)), 0))
        if step_log is not None and tape.handle:
            n = int(lib.ndcn_tape_steplog(tape.handle, None, 0))
            rows = (ctypes.c_double * (5 * max(n, 1)))()
            lib.ndcn_tape_steplog(tape.handle, rows, n)
            step_log.extend(tuple(rows[5 * i + j] for j in range(5)) for i in range(n))
            step_log.append(('nfe', int(lib.ndcn_tape_nfe(tape.handle))))
        if rc < 0:
            text = lib.ndcn_last_error().decode('utf-8', 'replace')
            err = tape.error
            tape.close()
            if err is not None:
                raise err
            if rc in (_lib.EMAXSTEPS, _lib.EUNDERFLOW, _lib.ENONFINITE):
                raise AssertionError(text)          # the reference's assertions (dopri5.py:89,100-102)
            raise _lib.NdcnHipError(rc, text)
        ctx.tape, ctx.keep = tape, (y0c, Wc, bc, csr, csr_t)
        ctx.has = (W is not None, b is not None)
        # (the library reads y0 / W / b again in the reverse pass: saved through autograd, so that an in-place change between forward
        # and backward raises instead of giving a gradient at other parameters - round-4 advisor on the fixed-grid Functions)
        # The forward record's device blocks ride along as saved tensors: autograd releases them with the graph - after the first
        # backward unless retain_graph - and a reverse pass over a released graph raises autograd's own "second time" error; with
        # retain_graph the record stays and the pass runs again (round-5 advisor: the reference's graph is re-runnable)
        blocks, tape.blocks = tape.blocks, []
        ctx.save_for_backward(y0, W, b, *blocks)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        tape = ctx.tape
        record = ctx.saved_tensors                  # version check of y0 / W / b; raises once the graph (and with it the record) is released
        if tape is None or not tape.handle:
            raise RuntimeError('the dopri5 tape of this solve has been destroyed')
        y0c, Wc, bc, csr, csr_t = ctx.keep
        g = g.contiguous()
        gy = torch.empty_like(y0c)
        gW = torch.empty_like(Wc) if Wc is not None else None
        gb = torch.empty_like(bc) if bc is not None else None
        lib = _lib.load()
        try:
            with torch.cuda.device(g.device):
                rc = lib.ndcn_tape_backward_f32(tape.handle, ptr(g), ptr(gy), ptr(gW), ptr(gb), stream_ptr())
            if rc < 0:
                if tape.error is not None:
                    raise tape.error
                check(rc)
        finally:
            tape.blocks = []                        # this pass's scratch (kernels still queued read it: the caching allocator reuses blocks stream-ordered)
            del record
        needs = ctx.needs_input_grad
        return (gy if needs[0] else None, gW if (needs[1] and ctx.has[0]) else None, gb if (needs[2] and ctx.has[1]) else None,
                None, None, None, None, None, None, None, None)


def _warn_retry():
    global _retry_warned
    if not _retry_warned:
        _retry_warned = True
        warnings.warn('the dopri5 training tape did not fit the device memory: solving again with every attempted step re-formed in the '
                      'reverse pass (set NDCN_TAPE_BUDGET_MB to bound the record from the start; 0 keeps two panels per accepted step)',
                      RuntimeWarning, stacklevel=2)


def applicable(odefunc, y0, t_user):
    if not enabled() or (torch.is_tensor(t_user) and t_user.requires_grad):
        return False
    if y0.dim() != 2 or y0.dtype != torch.float32:
        return False
    if not odefunc.no_graph:
        from ...csr import as_csr
        A = as_csr(odefunc.A)
        if A.shape[0] != A.shape[1] or A.shape[0] != y0.shape[0] or A.device != y0.device:
            return False
    return True


def solve(odefunc, y0, t, rtol, atol, options, step_log):
    """-> trajectory (T, N, H) with one autograd node, or None where the tape does not apply"""
    from . import core
    from ...csr import as_csr
    opt = core.dopri5_options(options, 1)
    rt, at = core.per_state_tolerance(rtol, 1)[0], core.per_state_tolerance(atol, 1)[0]
    flags = _lib.F_RELU | (_lib.F_NO_GRAPH if odefunc.no_graph else 0) | (_lib.F_NO_CONTROL if odefunc.no_control else 0)
    csr = csr_t = None
    if not odefunc.no_graph:
        csr = as_csr(odefunc.A)
        csr.ensure_plans(odefunc.hidden_size)
        csr_t = csr.transpose()
        csr_t.ensure_plans(odefunc.hidden_size)
    W = b = None
    if not odefunc.no_control:
        W, b = odefunc.wt.weight, odefunc.wt.bias
    ticks = core.host_grid(t).to(torch.float64).tolist()
    from .autograd_path import _keep_s_enabled
    keep_s = (not odefunc.no_graph) and (not odefunc.no_control) and _keep_s_enabled(y0)      # (the library keeps S where a kernel writes it)
    opts = (0.0 if opt['first_step'] is None else 1.0, opt['safety'], opt['ifactor'], opt['dfactor'], float(min(opt['max_num_steps'], 2 ** 53)),
            1.0 if keep_s else 0.0)
    budget_mb = _lib.env_int('NDCN_TAPE_BUDGET_MB', -1)
    budget = budget_mb * (1 << 20) if budget_mb >= 0 else -1         # bytes of forward record kept in full; < 0: no bound
    drop = None
    if _dropout.is_active(odefunc):
        stream = _dropout.current() or _dropout.Stream()
        drop = (float(odefunc.dropout), stream.seed, stream.evaluations, stream)
    return _TapeDopri5.apply(y0, W, b, (csr, csr_t, flags, odefunc.hidden_size), ticks, rt, at, opts, step_log, budget, drop)


# ---- fixed grids ---------------------------------------------------------------------------------------------------------------

def _fixed_grid_train(y0c, Wc, bc, csr, flags, method, dts):
    """ndcn_fixed_grid_train_f32 -> (trajectory (n_ticks + 1, N, H), the step sizes as the C array)"""
    lib = _lib.load()
    n_ticks = len(dts)
    out = torch.empty((n_ticks + 1,) + tuple(y0c.shape), dtype=torch.float32, device=y0c.device)
    scratch = Tape(y0c.device)
    arr = (ctypes.c_float * n_ticks)(*dts)
    view = csr.view_ref() if csr is not None else ctypes.byref(_lib.empty_csr(y0c.shape[0]))
    H = y0c.shape[1]
    with torch.cuda.device(y0c.device):
        rc = lib.ndcn_fixed_grid_train_f32(view, ptr(Wc), ptr(bc), H, flags, _lib.METHODS[method], ptr(y0c), arr, n_ticks, ptr(out),
                                           ctypes.cast(scratch.cb, ctypes.c_void_p), None, stream_ptr())
    err = scratch.error
    scratch.close()
    if rc < 0:
        if err is not None:
            raise err
        check(rc)
    return out, arr


def _fixed_grid_reverse(out, Wc, bc, csr, flags, method, arr, n_ticks, g, decoder=None):
    """The reverse sweep in the library -> (g_y0, g_W, g_b[, g_Wd, g_bd]).  g: the gradient of the trajectory (n_ticks + 1, N, H), or
    with decoder = (Wd (C, H), want g_Wd, want g_bd) the gradient of the DECODED ticks (n_ticks + 1, N, C): the sweep then forms every
    tick's g[i] . Wd where it adds it (ndcn_fixed_grid_backward_readout_f32) and returns the decoder's gradients too."""
    lib = _lib.load()
    g = g.contiguous()
    no_control = bool(flags & _lib.F_NO_CONTROL)
    gy = torch.empty_like(out[0])
    gW = torch.empty_like(Wc) if (Wc is not None and not no_control) else None
    gb = torch.empty_like(bc) if (bc is not None and not no_control) else None
    scratch = Tape(g.device)
    view = csr.view_ref() if csr is not None else ctypes.byref(_lib.empty_csr(out.shape[1]))
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
    err = scratch.error
    scratch.close()
    if rc < 0:
        if err is not None:
            raise err
        check(rc)
    return gy, gW, gb, gWd, gbd


class _NativeFixedGrid(torch.autograd.Function):
    """Euler / midpoint / RK4 over ODEFunc with the loops of `_impl/odeint.py::_FixedGridSolve` inside the library
    (ndcn_fixed_grid_train_f32 / ndcn_fixed_grid_backward_f32): the same launches, two calls instead of ~10 per step."""

    @staticmethod
    def forward(ctx, y0, W, b, csr, flags, method, dts):
        y0c = y0.detach().contiguous()
        Wc = W.detach().contiguous() if W is not None else None
        bc = b.detach().contiguous() if b is not None else None
        out, arr = _fixed_grid_train(y0c, Wc, bc, csr, flags, method, dts)
        ctx.keep = (Wc, bc, csr, flags, method, arr, len(dts))
        ctx.has = (W is not None, b is not None)
        # `out` is this node's own output: saved through autograd (no out -> grad_fn -> ctx -> out cycle that only the cyclic collector
        # would break - a (T, N, H) trajectory - and an in-place edit of the returned trajectory before backward raises)
        ctx.save_for_backward(out, W, b)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        out = ctx.saved_tensors[0]
        Wc, bc, csr, flags, method, arr, n_ticks = ctx.keep
        gy, gW, gb, _, _ = _fixed_grid_reverse(out, Wc, bc, csr, flags, method, arr, n_ticks, g)
        needs = ctx.needs_input_grad
        return (gy if needs[0] else None, gW if needs[1] else None, gb if needs[2] else None, None, None, None, None)


class _NativeFixedGridReadout(torch.autograd.Function):
    """_NativeFixedGrid with the decoder Linear(Wd, bd) of every tick inside the node (odeint's `readout` under a gradient): the
    differentiable output is the decoded solution (T, N, C) - hip.linear of the trajectory, the bits of the two-step form -, the hidden
    trajectory is kept for the reverse sweep only, and that sweep takes the (T, N, C) gradient as it is
    (ndcn_fixed_grid_backward_readout_f32): the (T, N, H) tensor g . Wd of the Linear's own backward is never written."""

    @staticmethod
    def forward(ctx, y0, W, b, Wd, bd, csr, flags, method, dts):
        from ...ops import hip
        y0c = y0.detach().contiguous()
        Wc = W.detach().contiguous() if W is not None else None
        bc = b.detach().contiguous() if b is not None else None
        out, arr = _fixed_grid_train(y0c, Wc, bc, csr, flags, method, dts)
        dec = hip.linear(out, Wd.detach(), None if bd is None else bd.detach())
        ctx.keep = (Wc, bc, csr, flags, method, arr, len(dts))
        # (the hidden trajectory is no output of the node: nothing differentiates through it, and it is released with the graph)
        ctx.save_for_backward(out, W, b, Wd)
        return dec

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        out, _, _, Wd = ctx.saved_tensors
        Wc, bc, csr, flags, method, arr, n_ticks = ctx.keep
        needs = ctx.needs_input_grad
        gy, gW, gb, gWd, gbd = _fixed_grid_reverse(out, Wc, bc, csr, flags, method, arr, n_ticks, g,
                                                   decoder=(Wd.detach().contiguous(), needs[3], needs[4]))
        return (gy if needs[0] else None, gW if needs[1] else None, gb if needs[2] else None, gWd if needs[3] else None,
                gbd if needs[4] else None, None, None, None, None)


def fixed_grid(y0, W, b, csr, flags, method, dts, readout=None):
    """-> trajectory (T, N, H), or None when the native loops are switched off (NDCN_FIXED_GRID_NATIVE=0); readout = (Wd, bd): the
    decoded solution (T, N, C) from the node that holds the decoder"""
    if not _lib.env_on('NDCN_FIXED_GRID_NATIVE') or _lib.env_str('NDCN_VJP', 'hip') == 'torch':
        return None
    if csr is not None:
        csr.ensure_plans(y0.shape[1])
        csr.transpose().ensure_plans(y0.shape[1])
    if readout is not None:
        return _NativeFixedGridReadout.apply(y0, W, b, readout[0], readout[1], csr, flags, method, dts)
    return _NativeFixedGrid.apply(y0, W, b, csr, flags, method, dts)
