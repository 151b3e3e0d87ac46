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
    flags = _lib.operator_flags(odefunc)
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
