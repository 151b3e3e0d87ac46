"""torch-tensor front end of the C-ABI kernels (include/ndcn_hip.h).

PyTorch supplies device memory and the current HIP stream; every computation below is a call into
libndcn_hip.so.  Host tensors are refused (`_lib.require_device`) - there is no CPU path in the product.

`HipOps` is the one shipped implementation of the small "panel ops" interface the integrator's host
logic is written against (ndcn_amd/torchdiffeq/_impl/core.py).  Tests drive that same host logic with
an oracle-backed double to check the control flow without a GPU; product code never does.
"""
import ctypes
import threading
import weakref

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, require_device, stream_ptr
from .csr import CsrOperator, as_csr

_F = ctypes.c_float
_P = ctypes.c_void_p


def _panel(t, what='panel'):
    require_device(t, what)
    return t if t.is_contiguous() else t.contiguous()


# The C calls carry pointers and a few sizes, never a tensor's own shape, strides or dtype: whatever reaches `ptr()` is read and written
# as a dense float32 (or int32) array of the extent the launch derives from its FIRST operand.  Every tensor operand of every wrapper
# below therefore passes `_operand` (or `_panel`, its form without expectations) before its data_ptr() is taken.
def _name(what):
    return what if isinstance(what, str) else '%s[%d]' % what


def _refuse(what, expected, t):
    given = '%s of shape %s, strides %s on %s' % (t.dtype, tuple(t.shape), tuple(t.stride()), t.device) if isinstance(t, torch.Tensor) \
        else type(t).__name__
    raise _lib.NdcnHipError(_lib.EINVAL, 'operand %s: expected %s, got %s' % (_name(what), expected, given))


def _layout(t, what, dtype=torch.float32, shape=None, numel=None, out=False):
    """The part of the operand gate that asks nothing of the device (the CPU suite drives it with host tensors): dtype, exact shape or
    exact element count, strides.  An input that is not contiguous comes back as its contiguous copy; an OUTPUT (out=True: the caller
    reads the result from this very tensor) must be contiguous already and is returned as it is.  Attribute reads only."""
    if not isinstance(t, torch.Tensor):
        _refuse(what, 'a tensor', t)
    if t.dtype != dtype:
        _refuse(what, 'dtype %s' % dtype, t)
    if shape is not None and tuple(t.shape) != tuple(shape):
        _refuse(what, 'shape %s' % (tuple(shape),), t)
    if numel is not None and t.numel() != numel:
        _refuse(what, '%d elements' % numel, t)
    if t.is_contiguous():
        return t
    if out:
        _refuse(what, 'a contiguous output', t)
    return t.contiguous()


def _on_device(t, what, device=None):
    """The device part of the gate: a ROCm tensor, on the launch's device where one is named."""
    if not isinstance(t, torch.Tensor):
        _refuse(what, 'a tensor', t)
    if not t.is_cuda:
        raise _lib.NdcnHipError(_lib.EINVAL, 'operand %s lives on %s; ndcn_amd computes on a ROCm device only (no CPU fallback). '
                                             'Move it with .to("cuda").' % (_name(what), t.device))
    if device is not None and t.device != device:
        _refuse(what, 'a tensor on %s, the device of the launch' % device, t)
    return t


def _operand(t, what, device=None, dtype=torch.float32, shape=None, numel=None, out=False):
    """The one gate between a caller's tensor and a kernel: `_on_device`, then `_layout`.  Returns the tensor to take data_ptr() of."""
    return _layout(_on_device(t, what, device), what, dtype, shape, numel, out)


def _like(t, what, ref, out=False, shape=False):
    """a nullable operand on ref's device with ref's element count (shape=True: ref's shape)"""
    if t is None:
        return None
    if shape:
        return _operand(t, what, ref.device, shape=ref.shape, out=out)
    return _operand(t, what, ref.device, numel=ref.numel(), out=out)


def _likes(ts, what, ref):
    return [_like(t, (what, j), ref) for j, t in enumerate(ts)]


def _terms(ks, cs):
    n = len(ks)
    arr_k = (_P * n)(*[k.data_ptr() for k in ks])
    arr_c = (_F * n)(*[float(c) for c in cs])
    return arr_k, arr_c, n


# The reductions below share per-device scratch (partials, the result record, its pinned host mirror).  Under autograd
# they are reached from TWO threads at once - the engine runs the backward of nodes whose gradient lives on the GPU on its
# device thread and the nodes of the solver's CPU scalar chain (error ratio, norms) on the calling thread - so launch +
# read-back of one reduction is one critical section.
_REDUCE_LOCK = threading.RLock()
_ADAMS_FUSED_OVERRIDE = None        # HipOps.set_adams_fused; None: the environment's NDCN_ADAMS_FUSED
_ADAMS_READOUT_OVERRIDE = None      # HipOps.set_adams_readout; None: the environment's NDCN_ADAMS_READOUT
_TGCN_FUSED_OVERRIDE = None         # HipOps.set_tgcn_fused; None: the environment's NDCN_TGCN_FUSED


class _Reducer:
    """Per-device scratch for the two-pass reductions + a pinned host mirror for the 16-byte record."""
    _by_device = {}

    @classmethod
    def get(cls, device):
        r = cls._by_device.get(device)
        if r is None:
            r = cls()
            lib = _lib.load()
            r.ws = torch.empty(int(lib.ndcn_reduce_ws_bytes()), dtype=torch.uint8, device=device)
            r.out = torch.zeros(2, dtype=torch.float64, device=device)
            r.host = torch.zeros(2, dtype=torch.float64).pin_memory()
            cls._by_device[device] = r
        return r

    def fetch(self):
        self.host.copy_(self.out, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        return float(self.host[0]), float(self.host[1])


class ErrorRecord:
    """A caller-owned {sum of squared error ratios, non-finite count} record: two doubles on the device + a pinned host
    mirror.  An error evaluation that is split into several launches (row blocks of a shard: NDCN_F_ACCUM) accumulates
    into ITS OWN record - the per-device one of _Reducer is shared with every other reduction of the process, and the
    lock is released between the launches of a split."""

    def __init__(self, device):
        self.out = torch.zeros(2, dtype=torch.float64, device=device)
        self.host = torch.zeros(2, dtype=torch.float64).pin_memory()

    fetch = _Reducer.fetch


class _PackedWeights:
    """The fused H = 256 kernels read W in a packed, split form that ndcn_rhs_f32 / ndcn_rhs_rk_f32 build in their
    scratch at every call (two small launches in front of the big one).  A solver calls them thousands of times with
    the same weights: the scratch is kept per weight TENSOR OBJECT (weak reference: a new tensor that happens to reuse the
    address or the id of a dead one never hits), version counter (in-place updates - optimizers, load_state_dict - move
    it), stream and EPOCH; later calls pass NDCN_F_PACKED.

    Epoch (round 5): `W.data.add_()`, `W.data.copy_()`, `dist.broadcast(W.data)` and raw-pointer writes bypass the version
    counter - hand-written SGD / EMA / clipping code does exactly that between two solves.  Every `odeint` / `odeint_adjoint`
    call therefore starts a new epoch (`new_epoch`): the first use of a weight inside it re-packs (two small launches, ~10 us
    per solve), the thousands that follow hit.  What is left to the caller: such a write BETWEEN two direct `hip.rhs` calls
    outside any solve (or in the middle of one - which no autograd graph survives either): call
    `ndcn_amd.ops.invalidate_packed_weights()` after it."""
    _cache = {}
    _epoch = 0

    @classmethod
    def invalidate(cls):
        cls._cache.clear()

    @classmethod
    def new_epoch(cls):
        cls._epoch += 1

    @classmethod
    def get(cls, W, nbytes, tag='fwd'):
        # a whole-tensor alias (the training path hands W on from evaluation to evaluation as `W.view_as(W)`: a new tensor object each
        # time) is the tensor it views: same storage, same version counter
        base = W._base
        if base is not None and base.data_ptr() == W.data_ptr() and base.shape == W.shape and base.is_contiguous():
            W = base
        key = (id(W), torch.cuda.current_stream(W.device).cuda_stream, nbytes, tag)
        hit = cls._cache.get(key)
        if hit is not None and hit[0]() is W and hit[1] == W._version and hit[2] == W.data_ptr():
            if hit[4] == cls._epoch:
                return hit[3], _lib.F_PACKED
            cls._cache[key] = hit[:4] + (cls._epoch,)             # same buffer, packed again by this call (stream-ordered)
            return hit[3], 0
        if len(cls._cache) >= 8:
            dead = [k for k, v in cls._cache.items() if v[0]() is None]
            for k in dead or [next(iter(cls._cache))]:
                cls._cache.pop(k)
        work = torch.empty(nbytes, dtype=torch.uint8, device=W.device)
        cls._cache[key] = (weakref.ref(W), W._version, W.data_ptr(), work, cls._epoch)
        return work, 0


class _BwdDots:
    """Per-device scratch of the solver VJP kernels: partial sums + the 8-double result + its pinned host mirror."""
    _by_device = {}

    @classmethod
    def get(cls, device):
        r = cls._by_device.get(device)
        if r is None:
            r = cls()
            r.ws = torch.empty(int(_lib.load().ndcn_rk_bwd_ws_bytes()), dtype=torch.uint8, device=device)
            r.out = torch.zeros(8, dtype=torch.float64, device=device)
            r.host = torch.zeros(8, dtype=torch.float64).pin_memory()
            cls._by_device[device] = r
        return r

    def fetch(self):
        self.host.copy_(self.out, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        return self.host.tolist()

    # ---- deferred read-back ------------------------------------------------------------------------------------------
    # A training step's backward makes ~35 of these reductions, and `fetch` stops the host at each of them until the GPU has
    # drained - with nothing queued behind: 6.7 ms of idle GPU per step on the 100k-node case (rocprofv3 kernel trace, 17 %).
    # `lazy` instead returns 0-d float32 HOST tensors (views of a pinned ring) that an asynchronous copy fills, plus an event;
    # whoever reads them first calls `await_lazy` (autograd_path._Await, the only consumer): by then the panel launches of the
    # whole solver step are queued behind the copy.  Same bits as `fetch`: the fp64 sums, times `scale` in fp64, rounded to fp32.
    RING = 1 << 15
    _ring_lock = threading.Lock()
    _ring = None
    _ring_pos = 0
    _pending = {}

    def lazy(self, n, scale=1.0):
        cls = _BwdDots
        src = self.out[:n]
        m = int(n)
        with cls._ring_lock:                # (ring position and pending table: written by the device's autograd worker, read by the caller's thread)
            if cls._ring is None:
                cls._ring = torch.zeros(cls.RING, dtype=torch.float32).pin_memory()
            if cls._ring_pos + m > cls.RING:
                cls._ring_pos = 0
            lo = cls._ring_pos
            cls._ring_pos += m
        dst = cls._ring[lo:lo + m]
        vals = (src * scale) if scale != 1.0 else src
        dst.copy_(vals.to(torch.float32), non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        outs = [dst[i] for i in range(m)]
        rec = (ev, [o.data_ptr() for o in outs])
        with cls._ring_lock:
            for p in rec[1]:
                cls._pending[p] = rec      # (a slot the ring hands out again replaces the stale record of its previous use)
        return outs

    @classmethod
    def await_lazy(cls, t):
        if t is not None and cls._pending:
            with cls._ring_lock:
                rec = cls._pending.get(t.data_ptr())
            if rec is not None:
                rec[0].synchronize()
                with cls._ring_lock:
                    for p in rec[1]:       # one copy filled all the slots of this read-back: none of them needs the event again
                        if cls._pending.get(p) is rec:
                            del cls._pending[p]
        return t


def _grad_ptrs(like, needs):
    outs = [torch.empty_like(like) if n else None for n in needs]
    return outs, (_P * len(needs))(*[None if o is None else o.data_ptr() for o in outs])


def _acc_ptrs(accs, n, ref):
    """(the gated tensors, the nullable array of their pointers) of the gradients the terms have ALREADY received (accumulating VJPs,
    include/ndcn_hip.h).  The caller holds the first until its launch is queued: the gate's contiguous copy of a strided gradient has no
    other owner, and its memory would go back to the caching allocator - and out again, to the outputs allocated next."""
    if accs is None or all(a is None for a in accs):
        return None, None
    assert len(accs) == n
    accs = [_like(a, ('accs', j), ref) for j, a in enumerate(accs)]
    return accs, (_P * n)(*[None if a is None else a.data_ptr() for a in accs])


class HipOps:
    """Panel operations on fp32 CUDA tensors, each ONE kernel launch through the C-ABI."""

    name = 'hip'

    # ---------------------------------------------------------------- graph convolution pieces
    @staticmethod
    def spmm(A, X, X_halo=None, alpha=1.0, relu=False, out=None):
        """alpha * (A X) [relu].  Replaces torch.sparse.mm / torch.mm(A, x) (neural_dynamics.py:29,31)."""
        A = as_csr(A)
        X = _panel(X, 'X')
        squeeze = X.dim() == 1
        X2 = X.view(-1, 1) if squeeze else X
        assert X2.dim() == 2
        H = X2.shape[1]
        n_own = X2.shape[0]
        if X_halo is not None:
            X_halo = _operand(X_halo, 'X_halo', X2.device)
            if X_halo.dim() != 2 or X_halo.shape[1] != H:
                _refuse('X_halo', 'a panel of %d columns' % H, X_halo)
        HipOps._rhs_operator(A, X2, X_halo)
        A.ensure_plans(H)
        if out is None:
            Y = torch.empty((A.shape[0], H), dtype=torch.float32, device=X2.device)
        elif squeeze and out.dim() == 1:
            Y = _operand(out, 'out', X2.device, numel=A.shape[0], out=True)
        else:
            Y = _operand(out, 'out', X2.device, shape=(A.shape[0], H), out=True)
        with torch.cuda.device(X2.device):
            check(_lib.load().ndcn_spmm_f32(A.view_ref(), ptr(X2), ptr(X_halo), n_own, ptr(Y), H, float(alpha),
                                            _lib.F_RELU if relu else 0, stream_ptr()))
        return Y.view(-1) if squeeze else Y

    @staticmethod
    def adjoint_rhs(A, y, a, W, b, no_graph=False, no_control=False):
        """ndcn_adjoint_rhs_f32: (K, vjp_y, vjp_W, vjp_b) = (ODEFunc(y), -A^T((a.[K>0]) W), -(a.[K>0])^T (A y), -sum_rows a.[K>0]) -
        the right-hand side of odeint_adjoint's augmented system (adjoint.py:34-59) without a torch graph; vjp_W / vjp_b are
        None under no_control."""
        y = _panel(y, 'y')
        if y.dim() != 2:
            _refuse('y', 'a 2-D panel', y)
        a = _like(a, 'a', y, shape=True)
        H = y.shape[1]
        flags = _lib.F_RELU | (_lib.F_NO_GRAPH if no_graph else 0) | (_lib.F_NO_CONTROL if no_control else 0)
        lib = _lib.load()
        if no_graph:
            view = view_t = ctypes.byref(_lib.empty_csr(y.shape[0]))
        else:
            A = as_csr(A)
            if tuple(A.shape) != (y.shape[0], y.shape[0]) or A.device != y.device:
                raise _lib.NdcnHipError(_lib.EINVAL, 'operator %s on %s, panel of %d rows on %s' % (tuple(A.shape), A.device, y.shape[0], y.device))
            A.ensure_plans(H)
            At = A.transpose()
            At.ensure_plans(H)
            view, view_t = A.view_ref(), At.view_ref()
        K, vjp_y = torch.empty_like(y), torch.empty_like(y)
        vW = vb = None
        if not no_control:
            W = _operand(W, 'W', y.device, shape=(H, H))
            b = _operand(b, 'b', y.device, numel=H) if b is not None else None
            vW = torch.empty((H, H), dtype=torch.float32, device=y.device)
            vb = torch.empty((H,), dtype=torch.float32, device=y.device)
        work = torch.empty(int(lib.ndcn_adjoint_rhs_work_bytes(y.shape[0], H, flags)) + 256, dtype=torch.uint8, device=y.device)
        off = (-work.data_ptr()) % 256
        with torch.cuda.device(y.device):
            check(lib.ndcn_adjoint_rhs_f32(view, view_t, ptr(y), ptr(a), ptr(None if no_control else W), ptr(None if no_control else b),
                                           ptr(K), ptr(vjp_y), ptr(vW), ptr(vb), ctypes.c_void_p(work.data_ptr() + off), H, flags,
                                           stream_ptr()))
        return K, vjp_y, vW, vb

    @staticmethod
    def gcn(A, X, W, b=None, relu=False):
        """A (X W^T + b) [relu]: GraphConvolution.forward of the reference (models.py:14-18) in one library call."""
        A = as_csr(A)
        X = _panel(X, 'X')
        W = _operand(W, 'W', X.device)
        if W.dim() != 2:
            _refuse('W', 'a 2-D weight', W)
        Ho, Hi = W.shape
        if b is not None:
            b = _operand(b, 'b', X.device, numel=Ho)
        assert X.dim() == 2 and X.shape == (A.shape[1], Hi)
        if A.device != X.device:
            raise _lib.NdcnHipError(_lib.EINVAL, 'operator on %s, panel on %s' % (A.device, X.device))
        A.ensure_plans(Ho)
        lib = _lib.load()
        Y = torch.empty((A.shape[0], Ho), dtype=torch.float32, device=X.device)
        work = torch.empty(int(lib.ndcn_gcn_work_bytes(A.shape[1], Ho)), dtype=torch.uint8, device=X.device)
        with torch.cuda.device(X.device):
            check(lib.ndcn_gcn_f32(A.view_ref(), ptr(X), ptr(W), ptr(b), ptr(Y), ptr(work), Hi, Ho,
                                   _lib.F_RELU if relu else 0, stream_ptr()))
        return Y

    @staticmethod
    def linear(S, W, b=None, relu=False):
        """S W^T + b [relu] over the last dimension (nn.Linear semantics; neural_dynamics.py:33,143-148)."""
        S = _panel(S, 'S')
        if S.dim() < 1:
            _refuse('S', 'a panel of at least one dimension', S)
        W = _operand(W, 'W', S.device)
        if W.dim() != 2:
            _refuse('W', 'a 2-D weight (Ho, Hi)', W)
        if S.shape[-1] != W.shape[1]:
            _refuse('S', 'a last dimension of %d, the columns of W' % W.shape[1], S)
        lead = S.shape[:-1]
        Hi, Ho = S.shape[-1], W.shape[0]
        if b is not None:
            b = _operand(b, 'b', S.device, numel=Ho)
        S2 = S.reshape(-1, Hi)
        Y = torch.empty((S2.shape[0], Ho), dtype=torch.float32, device=S.device)
        with torch.cuda.device(S.device):
            check(_lib.load().ndcn_linear_f32(ptr(S2), ptr(W), ptr(b), ptr(Y), S2.shape[0], Hi, Ho,
                                              _lib.F_RELU if relu else 0, stream_ptr()))
        return Y.view(*lead, Ho)

    @staticmethod
    def linear_bwd(g, W, S=None, Y=None, need_gS=True, need_gW=True, need_gb=True):
        """Backward of act(S W^T + b): returns (gS, gW, gb) (None where not requested).  Y: the ReLU output (mask
        gZ = g where Y > 0) or None.  One GEMM launch for gS, one split-row launch + fixed-order sum for gW / gb."""
        g = _panel(g, 'g')
        if g.dim() < 1:
            _refuse('g', 'a panel of at least one dimension', g)
        W = _operand(W, 'W', g.device)
        if W.dim() != 2:
            _refuse('W', 'a 2-D weight (Ho, Hi)', W)
        if g.shape[-1] != W.shape[0]:
            _refuse('g', 'a last dimension of %d, the rows of W' % W.shape[0], g)
        Ho, Hi = W.shape
        lead = g.shape[:-1]
        g2 = g.reshape(-1, Ho)
        n = g2.shape[0]
        S2 = _operand(S, 'S', g.device, shape=tuple(lead) + (Hi,)).reshape(-1, Hi) if S is not None else None
        Y2 = _operand(Y, 'Y', g.device, shape=g.shape).reshape(-1, Ho) if Y is not None else None
        need_gW = need_gW and S2 is not None
        lib = _lib.load()
        gS = torch.empty((n, Hi), dtype=torch.float32, device=g.device) if need_gS else None
        gW = torch.empty((Ho, Hi), dtype=torch.float32, device=g.device) if need_gW else None
        gb = torch.empty((Ho,), dtype=torch.float32, device=g.device) if need_gb else None
        work, flags = None, 0
        if need_gW or need_gb or (need_gS and Hi == 256 and Ho == 256):      # (H = 256: gS packs the planes of W^T there)
            nbytes = int(lib.ndcn_linear_bwd_work_bytes(n, Hi, Ho))
            if need_gS and Hi == 256 and Ho == 256:
                # the scratch is kept per weight tensor (object, version, stream): the planes of W^T packed by the first VJP of a
                # backward pass serve the dozens that follow (the head of the buffer is per-call scratch, stream-ordered)
                work, flags = _PackedWeights.get(W, nbytes, tag='bwd')
            else:
                work = torch.empty(nbytes, dtype=torch.uint8, device=g.device)
        with torch.cuda.device(g.device):
            check(lib.ndcn_linear_bwd_f32(ptr(g2), ptr(Y2), ptr(S2 if S2 is not None else g2), ptr(W), ptr(gS), ptr(gW), ptr(gb),
                                          ptr(work), n, Hi, Ho, flags, stream_ptr()))
        return (gS.view(*lead, Hi) if gS is not None else None), gW, gb

    @staticmethod
    def relu_bwd(g, y):
        """0 where y <= 0 else g (VJP of relu from its output; threshold_backward: a NaN y passes g)."""
        g = _panel(g, 'g')
        y = _like(y, 'y', g)
        out = torch.empty_like(g)
        with torch.cuda.device(g.device):
            check(_lib.load().ndcn_relu_bwd_f32(ptr(out), ptr(g), ptr(y), g.numel(), stream_ptr()))
        return out

    @staticmethod
    def copy(x, out=None):
        """out = x as the library's streaming pass (ndcn_copy_f32)."""
        x = _panel(x, 'x')
        out = torch.empty_like(x) if out is None else _like(out, 'out', x, out=True)
        with torch.cuda.device(x.device):
            check(_lib.load().ndcn_copy_f32(ptr(out), ptr(x), x.numel(), stream_ptr()))
        return out

    @staticmethod
    def scale(x, w):
        """w * x as one streaming kernel."""
        x = _panel(x, 'x')
        out = torch.empty_like(x)
        with torch.cuda.device(x.device):
            check(_lib.load().ndcn_scale_f32(ptr(out), ptr(x), float(w), x.numel(), stream_ptr()))
        return out

    @staticmethod
    def _rhs_input(X, X_halo):
        """the gate of a right-hand side's input panels: (X, X_halo, H)"""
        X = _panel(X, 'X')
        if X.dim() != 2:
            _refuse('X', 'a 2-D panel', X)
        if X_halo is not None:
            X_halo = _operand(X_halo, 'X_halo', X.device)
            if X_halo.dim() != 2 or X_halo.shape[1] != X.shape[1]:
                _refuse('X_halo', 'a panel of %d columns' % X.shape[1], X_halo)
        return X, X_halo, X.shape[1]

    @staticmethod
    def _rhs_operator(A, X, X_halo):
        """the operator of a right-hand side against the rows its panels supply (what spmm asserts)"""
        A = as_csr(A)
        if A.device != X.device:
            raise _lib.NdcnHipError(_lib.EINVAL, 'operator on %s, panel on %s' % (A.device, X.device))
        rows = X.shape[0] + (0 if X_halo is None else X_halo.shape[0])
        if A.shape[1] != rows:
            raise _lib.NdcnHipError(_lib.EINVAL, 'operator has %d columns, panels supply %d rows' % (A.shape[1], rows))
        return A

    @staticmethod
    def rhs(A, X, W, b, no_graph=False, no_control=False, X_halo=None, out=None, relu=True, dropout=None):
        """The whole ODEFunc.forward: relu(dropout(W (A X) + b))   (neural_dynamics.py:20-39).
        relu=False: the same launch without the activation - the transposed half of the adjoint right-hand side,
        (A^T gZ) W with the operator / weight pair (A^T, W^T) and no bias (_impl/adjoint_fused.py).
        dropout: None (p = 0, eval mode) or (p, seed, evaluation) with 0 < p < 1 - the result times the mask of csrc/dropout.h,
        a function of those three numbers and the element index alone (ndcn_rhs_drop_f32)."""
        X, X_halo, H = HipOps._rhs_input(X, X_halo)
        flags = (_lib.F_RELU if relu else 0) | (_lib.F_NO_GRAPH if no_graph else 0) | (_lib.F_NO_CONTROL if no_control else 0)
        lib = _lib.load()
        if no_graph:
            view = _lib.empty_csr(X.shape[0])
            view_ref = ctypes.byref(view)
            n_rows = X.shape[0]
        else:
            A = HipOps._rhs_operator(A, X, X_halo)
            A.ensure_plans(H)
            view_ref = A.view_ref()
            n_rows = A.shape[0]
        if not no_control:
            W = _operand(W, 'W', X.device, shape=(H, H))
            b = _operand(b, 'b', X.device, numel=H) if b is not None else None
        Y = _operand(out, 'out', X.device, shape=(n_rows, H), out=True) if out is not None \
            else torch.empty((n_rows, H), dtype=torch.float32, device=X.device)
        work = None
        wbytes = int(lib.ndcn_rhs_work_bytes(n_rows, H, flags))
        if wbytes:
            if H == 256 and not no_control and not no_graph and not torch.is_grad_enabled():
                work, packed = _PackedWeights.get(W, wbytes)
                flags |= packed
            else:
                work = torch.empty(wbytes, dtype=torch.uint8, device=X.device)
        with torch.cuda.device(X.device):
            if dropout is not None:
                check(lib.ndcn_rhs_drop_f32(view_ref, ptr(X), ptr(X_halo), X.shape[0], ptr(None if no_control else W),
                                            ptr(None if no_control else b), ptr(Y), ptr(work), H, flags, stream_ptr(),
                                            _lib.dropout_desc(dropout)))
                return Y
            check(lib.ndcn_rhs_f32(view_ref, ptr(X), ptr(X_halo), X.shape[0], ptr(None if no_control else W),
                                   ptr(None if no_control else b), ptr(Y), ptr(work), H, flags, stream_ptr()))
        return Y

    @staticmethod
    def dropout_apply(K, dropout):
        """K *= mask in place (ndcn_dropout_apply_f32): dropout = (p, seed, evaluation), element index = position in K's memory.
        K: a contiguous float32 device tensor or view (a misaligned one takes the scalar kernel).  Returns K."""
        K = _operand(K, 'K', out=True)
        with torch.cuda.device(K.device):
            check(_lib.load().ndcn_dropout_apply_f32(ptr(K), K.numel(), _lib.dropout_desc(dropout), stream_ptr()))
        return K

    @staticmethod
    def dropout_combine(K, dropout, kprev, cs, y0=None, out=None):
        """K *= mask in place and, in the same pass, out = y0 + sum_j cs[j] kprev[j] + cs[-1] K (ndcn_dropout_combine_f32): the bits of
        dropout_apply(K, dropout) followed by combine(y0, kprev + [K], cs).  y0 None: the sum alone.  Contiguous float32 device
        tensors or views (misaligned ones take the scalar lanes); out must not overlap K.  Returns (K, out)."""
        K = _operand(K, 'K', out=True)
        assert len(cs) == len(kprev) + 1
        # (the terms may be views INTO a record the caller keeps: never copied, like an output)
        kprev = [_like(k, ('kprev', j), K, out=True) for j, k in enumerate(kprev)]
        y0 = _like(y0, 'y0', K)
        out = torch.empty_like(K) if out is None else _like(out, 'out', K, out=True)
        n = len(kprev)
        arr_k = (_P * max(n, 1))(*[k.data_ptr() for k in kprev])
        arr_c = (_F * (n + 1))(*[float(c) for c in cs])
        with torch.cuda.device(K.device):
            check(_lib.load().ndcn_dropout_combine_f32(ptr(K), K.numel(), _lib.dropout_desc(dropout), ptr(out), ptr(y0), arr_k, arr_c, n,
                                                       stream_ptr()))
        return K, out

    @staticmethod
    def rhs_rk(A, X, W, b, mode, y0, kprev, cs, rtol=0.0, atol=0.0, no_graph=False, no_control=False, X_halo=None,
               out_K=None, out_y=None, y1=None, accum=False, fetch=True, aux_cs=None, out_aux=None, record=None, relu=True,
               x_mask=None, s_out=None, dropout=None):
        """K = ODEFunc(X) plus, in the same pass, the stage algebra consuming K (ndcn_rhs_rk_f32).
        record (mode 'error'): an ErrorRecord of the caller's that receives / accumulates the result instead of the
        per-device one (split evaluations: new_error_record()).
        mode 'combine': returns (K, y0 + sum cs[m] kprev[m] + cs[-1] K); mode 'error': returns
        (K, (sum of squared error ratios, non-finite count of X)) - the dopri5 error record with X = y1;
        mode 'rk4': stage len(kprev) of the 3/8-rule step, cs = [dt]: returns (K, next stage input / step result).
        mode 'error' only - y1: the rows of the state whose error record is formed (default X: the single-launch case);
        accum: add the record to the one already in the device buffer (an evaluation split into several launches);
        fetch=False: leave the record on the device (returns (K, None); the last launch of the split fetches).
        mode 'combine' only - aux_cs: coefficients of a second linear combination of the same stages (no y0), formed in
        the same pass: returns (K, y_next, sum aux_cs[m] kprev[m] + aux_cs[-1] K) - dopri5's partial error sum E.
        x_mask / s_out (ndcn_rhs_rk_adj_f32, where rhs_adj_supported says so): the input is X (.) [x_mask > 0] formed on the staged
        rows / S = A X is written into s_out too - the two halves of odeint_adjoint's right-hand side (_impl/adjoint_fused.py).
        dropout: None or (p, seed, evaluation) as in rhs(): K, as returned and as consumed by the stage algebra, is the masked one
        (ndcn_rhs_rk_drop_f32; not with x_mask / s_out / a halo panel)."""
        X, X_halo, H = HipOps._rhs_input(X, X_halo)
        dev = X.device
        flags = (_lib.F_RELU if relu else 0) | (_lib.F_NO_GRAPH if no_graph else 0) | (_lib.F_NO_CONTROL if no_control else 0)
        lib = _lib.load()
        if no_graph:
            view_ref = ctypes.byref(_lib.empty_csr(X.shape[0]))
            n_rows = X.shape[0]
        else:
            A = HipOps._rhs_operator(A, X, X_halo)
            A.ensure_plans(H)
            view_ref = A.view_ref()
            n_rows = A.shape[0]
        panel = (n_rows, H)
        if not no_control:
            W = _operand(W, 'W', dev, shape=(H, H))
            b = _operand(b, 'b', dev, numel=H) if b is not None else None
        else:
            W = b = None                                        # (not read: no pointer of theirs is handed on)
        y0 = _operand(y0, 'y0', dev, shape=panel)
        kprev = [_operand(k, ('kprev', j), dev, shape=panel) for j, k in enumerate(kprev)]
        assert len(cs) == (1 if mode == 'rk4' else len(kprev) + 1)
        if y1 is not None:
            assert mode == 'error'
            y1 = _operand(y1, 'y1', dev, shape=panel)
        if accum:
            flags |= _lib.F_ACCUM
        K = _operand(out_K, 'out_K', dev, shape=panel, out=True) if out_K is not None \
            else torch.empty(panel, dtype=torch.float32, device=dev)
        wbytes = int(lib.ndcn_rhs_work_bytes(n_rows, H, flags))
        work = None
        if wbytes:
            if H == 256 and not no_control and not no_graph and not torch.is_grad_enabled():
                work, packed = _PackedWeights.get(W, wbytes)
                flags |= packed
            else:
                work = torch.empty(wbytes, dtype=torch.uint8, device=X.device)
        arr_k = (_P * max(len(kprev), 1))(*[k.data_ptr() for k in kprev])
        arr_c = (_F * len(cs))(*[float(c) for c in cs])
        y_aux = arr_c2 = None
        if aux_cs is not None:
            assert mode == 'combine' and len(aux_cs) == len(kprev) + 1
            arr_c2 = (_F * len(aux_cs))(*[float(c) for c in aux_cs])
            y_aux = _operand(out_aux, 'out_aux', dev, shape=panel, out=True) if out_aux is not None else torch.empty_like(K)
        rk = {'combine': _lib.RK_COMBINE, 'error': _lib.RK_ERROR, 'rk4': _lib.RK_RK4}[mode]
        y_next = None
        if mode in ('combine', 'rk4'):
            y_next = _operand(out_y, 'out_y', dev, shape=panel, out=True) if out_y is not None else torch.empty_like(K)
        red = _Reducer.get(X.device)
        if record is not None and (record.out.device != dev or record.out.dtype != torch.float64 or record.out.numel() != 2):
            _refuse('record', 'an ErrorRecord of the launch\'s device', record.out)
        if x_mask is not None or s_out is not None:
            assert X_halo is None and aux_cs is None and not accum and dropout is None
            x_mask = _like(x_mask, 'x_mask', X, shape=True)
            s_out = _operand(s_out, 's_out', dev, shape=panel, out=True) if s_out is not None else None
            with _REDUCE_LOCK, torch.cuda.device(X.device):
                check(lib.ndcn_rhs_rk_adj_f32(view_ref, ptr(X), ptr(x_mask), ptr(s_out), ptr(W), ptr(b), ptr(K), ptr(work), H, flags, rk,
                                              ptr(y0), arr_k, arr_c, len(kprev), ptr(y_next), ptr(y1), float(rtol), float(atol),
                                              ptr((record or red).out), ptr(red.ws), stream_ptr()))
                if mode == 'combine':
                    return K, y_next
                return K, ((record or red).fetch() if fetch else None)
        with _REDUCE_LOCK, torch.cuda.device(X.device):
            args = (view_ref, ptr(X), ptr(X_halo), X.shape[0], ptr(None if no_control else W),
                    ptr(None if no_control else b), ptr(K), ptr(work), H, flags, rk, ptr(y0), arr_k,
                    arr_c, len(kprev), ptr(y_next), ptr(y1), ptr(y_aux), arr_c2, float(rtol), float(atol),
                    ptr((record or red).out), ptr(red.ws), stream_ptr())
            if dropout is not None:
                check(lib.ndcn_rhs_rk_drop_f32(*args, _lib.dropout_desc(dropout)))
            else:
                check(lib.ndcn_rhs_rk_f32(*args))
            if aux_cs is not None:
                return K, y_next, y_aux
            if mode in ('combine', 'rk4'):
                return K, y_next
            return K, ((record or red).fetch() if fetch else None)

    @staticmethod
    def rhs_adj_supported(A, H, mode, n_prev, no_control=False):
        """can rhs_rk honour x_mask / s_out for this operator and launch?"""
        A = as_csr(A)
        A.ensure_plans(H)
        flags = _lib.F_NO_CONTROL if no_control else 0
        rk = {'combine': _lib.RK_COMBINE, 'error': _lib.RK_ERROR}.get(mode, 0)
        return bool(_lib.load().ndcn_rhs_adj_supported(A.view_ref(), H, flags, rk, n_prev))

    @staticmethod
    def set_rhs_mid(mode):
        """The one-launch right-hand side for hidden widths 16..128 at any size (ndcn_set_rhs_mid, csrc/rhs_mid.hip): 0 off, 1 on
        wherever the narrow-panel kernel does not take the shape, 2 on for every supported shape; < 0: the environment's
        (NDCN_RHS_MID).  Process-wide; returns the previous mode."""
        return int(_lib.load().ndcn_set_rhs_mid(int(mode)))

    @staticmethod
    def set_rhs_mid_drop(on):
        """Dropout inside the one-launch right-hand side for hidden widths 16..128 (ndcn_set_rhs_mid_drop, csrc/rhs_mid.hip): 0 off -
        launches with a dropout descriptor run as without set_rhs_mid -, 1 on wherever the set_rhs_mid mode takes the shape; < 0: the
        environment's (NDCN_RHS_MID_DROP).  Process-wide; returns the previous value."""
        return int(_lib.load().ndcn_set_rhs_mid_drop(int(on)))

    @staticmethod
    def set_rhs_abl(on):
        """The one-launch right-hand side of the no_control / no_graph ablations for hidden widths 16..128 at any size (ndcn_set_rhs_abl,
        csrc/rhs_abl.hip): 0 off, 1 on - rhs / rhs_rk with exactly one of the two flags form K, the dropout factor and the stage algebra
        in one launch, the composed launches' bits; < 0: the environment's (NDCN_RHS_ABL).  Process-wide; returns the previous value."""
        return int(_lib.load().ndcn_set_rhs_abl(int(on)))

    @staticmethod
    def set_solver_mid(mode):
        """The one-launch kernels of set_rhs_mid / set_rhs_abl inside the device-resident solver (ndcn_set_solver_mid; odeint without a
        gradient, DeviceSolver): 0 off, 1 on except the widths that measured slower per solver step (H > 96), 2 on for every supported shape; < 0: the environment's (NDCN_SOLVER_MID).  Read when a solver is created;
        the results are the switched-off solve's bit for bit.  Process-wide; returns the previous mode."""
        return int(_lib.load().ndcn_set_solver_mid(int(mode)))

    @staticmethod
    def solver_mid_mode():
        """the mode set_solver_mid would return, read without changing it (odeint keys its kept solvers by it)"""
        return int(_lib.load().ndcn_solver_mid_mode())

    @staticmethod
    def solver_mid_takes(n_rows, H, no_graph=False, no_control=False, mode=2):
        """ndcn_solver_mid_takes: the sizes' part of the solver's decision for the kinds 'mid' / 'abl' under `mode` (no device needed)"""
        flags = _lib.F_RELU | (_lib.F_NO_GRAPH if no_graph else 0) | (_lib.F_NO_CONTROL if no_control else 0)
        return bool(_lib.load().ndcn_solver_mid_takes(int(n_rows), int(H), flags, int(mode)))

    @staticmethod
    def set_rhs_mid_bwd(mode):
        """The one-launch reverse of the right-hand side for hidden widths 16..128 at any size (ndcn_set_rhs_mid_bwd,
        csrc/rhs_mid_bwd.hip): 0 off, 1 on for the widths that measured not slower than the composed launches, 2 on for every
        supported shape; < 0: the environment's (NDCN_RHS_MID_BWD).  Process-wide; returns the previous mode."""
        return int(_lib.load().ndcn_set_rhs_mid_bwd(int(mode)))

    @staticmethod
    def set_rhs_abl_bwd(on):
        """The one-launch reverse of the no_control / no_graph ablations for hidden widths 16..128 at any size (ndcn_set_rhs_abl_bwd,
        csrc/rhs_abl_bwd.hip): 0 off, 1 on - rhs_vjp and the native tapes run the reverse of an evaluation with exactly one of the two
        flags as one launch (no_control) or one launch plus the chunk sum (no_graph), the composed launches' bits; < 0: the environment's
        (NDCN_RHS_ABL_BWD).  Process-wide; returns the previous value."""
        return int(_lib.load().ndcn_set_rhs_abl_bwd(int(on)))

    @staticmethod
    def rhs_abl_bwd_on():
        """the value set_rhs_abl_bwd would return, read without changing it (autograd_ops.rhs_vjp decides its route by it)"""
        return int(_lib.load().ndcn_rhs_abl_bwd_on())

    # ---------------------------------------------------------------- TemporalGCN: the hoisted input projection and the recurrence (csrc/tgcn.hip)
    @staticmethod
    def set_tgcn_fused(mode):
        """The fused form of neural_dynamics.TemporalGCN (one projection of all ticks, one launch for the recurrence): 0 off - every
        forward takes the composed per-tick loop -, 1 on wherever the module's conditions hold; < 0: the environment's
        (NDCN_TGCN_FUSED, default 1).  Process-wide; returns the previous mode."""
        global _TGCN_FUSED_OVERRIDE
        prev = HipOps.tgcn_fused_on()
        _TGCN_FUSED_OVERRIDE = None if int(mode) < 0 else (1 if int(mode) else 0)
        return prev

    @staticmethod
    def tgcn_fused_on():
        if _TGCN_FUSED_OVERRIDE is not None:
            return _TGCN_FUSED_OVERRIDE
        return 1 if _lib.env_int('NDCN_TGCN_FUSED', 1) > 0 else 0

    @staticmethod
    def tgcn_chunk(reverse=False):
        """ticks per pass over W_ih in tgcn_proj (reverse: per staging step of tgcn_proj_bwd)"""
        return int(_lib.load().ndcn_tgcn_chunk(1 if reverse else 0))

    @staticmethod
    def tgcn_proj(S, r, w, b, W_ih, b_ih):
        """GI (T, M) = b_ih + sum_{i,j} W_ih[:, i Hg + j] relu(S[i, :] w_j + r_i b_j) for all T ticks (ndcn_tgcn_proj_f32).  S (N, T) = A X,
        r (N,) = A 1, w / b (Hg,): the graph convolution's Linear(1, Hg), W_ih (M, N Hg), b_ih (M,)."""
        S = _panel(S, 'S')
        if S.dim() != 2:
            _refuse('S', 'a 2-D panel (N, T)', S)
        N, T = S.shape
        dev = S.device
        w = _operand(w, 'w', dev).reshape(-1)
        Hg = w.numel()
        r, b = _operand(r, 'r', dev, numel=N), _operand(b, 'b', dev, numel=Hg).reshape(-1)
        W_ih = _operand(W_ih, 'W_ih', dev)
        if W_ih.dim() != 2 or W_ih.shape[1] != N * Hg:
            _refuse('W_ih', 'a weight of shape (M, %d)' % (N * Hg), W_ih)
        M = W_ih.shape[0]
        b_ih = _operand(b_ih, 'b_ih', dev, numel=M)
        lib = _lib.load()
        GI = torch.empty((T, M), dtype=torch.float32, device=S.device)
        ws = torch.empty(max(int(lib.ndcn_tgcn_proj_ws_bytes(N, T, M)), 4), dtype=torch.uint8, device=S.device)
        with torch.cuda.device(S.device):
            check(lib.ndcn_tgcn_proj_f32(ptr(S), ptr(r), ptr(w), ptr(b), ptr(W_ih), ptr(b_ih), ptr(GI), ptr(ws), N, T, Hg, M, stream_ptr()))
        return GI

    @staticmethod
    def tgcn_proj_bwd(S, r, w, b, W_ih, GGI):
        """(g_Wih, g_w, g_b, g_bih) of tgcn_proj for GGI = dL/dGI (T, M) (ndcn_tgcn_proj_bwd_f32): g_Wih is written once, W_ih read once."""
        S = _panel(S, 'S')
        if S.dim() != 2:
            _refuse('S', 'a 2-D panel (N, T)', S)
        N, T = S.shape
        dev = S.device
        w = _operand(w, 'w', dev).reshape(-1)
        Hg = w.numel()
        r, b = _operand(r, 'r', dev, numel=N), _operand(b, 'b', dev, numel=Hg).reshape(-1)
        W_ih = _operand(W_ih, 'W_ih', dev)
        if W_ih.dim() != 2 or W_ih.shape[1] != N * Hg:
            _refuse('W_ih', 'a weight of shape (M, %d)' % (N * Hg), W_ih)
        M = W_ih.shape[0]
        GGI = _operand(GGI, 'GGI', dev, shape=(T, M))
        lib = _lib.load()
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=S.device)
        g_Wih, g_w, g_b, g_bih = new(M, N * Hg), new(Hg), new(Hg), new(M)
        ws = torch.empty(max(int(lib.ndcn_tgcn_proj_bwd_ws_bytes(N)), 4), dtype=torch.uint8, device=S.device)
        with torch.cuda.device(S.device):
            check(lib.ndcn_tgcn_proj_bwd_f32(ptr(S), ptr(r), ptr(w), ptr(b), ptr(W_ih), ptr(GGI), ptr(g_Wih), ptr(g_w), ptr(g_b),
                                             ptr(g_bih), ptr(ws), N, T, Hg, M, stream_ptr()))
        return g_Wih, g_w, g_b, g_bih

    @staticmethod
    def tgcn_cell(rnn_type, GI, W_hh, b_hh, h0=None, c0=None):
        """The recurrence of an LSTMCell / GRUCell / RNNCell ('lstm' / 'gru' / 'rnn') over the T rows of GI in one launch
        (ndcn_tgcn_cell_f32): (H (T, Hr), gates (T, 4 Hr), c_rec (T, Hr) or None, hT, cT or None); h0 / c0 None: zeros."""
        kind = _lib.TGCN_TYPES[rnn_type]
        GI = _panel(GI, 'GI')
        if GI.dim() != 2 or GI.shape[1] % _lib.TGCN_GATES[kind]:
            _refuse('GI', 'a 2-D panel (T, %d Hr)' % _lib.TGCN_GATES[kind], GI)
        T, M = GI.shape
        dev = GI.device
        Hr = M // _lib.TGCN_GATES[kind]
        W_hh, b_hh = _operand(W_hh, 'W_hh', dev, shape=(M, Hr)), _operand(b_hh, 'b_hh', dev, numel=M)
        h0 = _operand(h0, 'h0', dev, numel=Hr).reshape(-1) if h0 is not None else None
        c0 = _operand(c0, 'c0', dev, numel=Hr).reshape(-1) if c0 is not None else None
        lstm = kind == _lib.TGCN_LSTM
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=GI.device)
        H, gates, hT = new(T, Hr), new(T, 4 * Hr), new(Hr)
        c_rec, cT = (new(T, Hr), new(Hr)) if lstm else (None, None)
        with torch.cuda.device(GI.device):
            check(_lib.load().ndcn_tgcn_cell_f32(kind, ptr(GI), ptr(W_hh), ptr(b_hh), ptr(h0), ptr(c0), ptr(H), ptr(gates), ptr(c_rec),
                                                 ptr(hT), ptr(cT), T, Hr, stream_ptr()))
        return H, gates, c_rec, hT, cT

    @staticmethod
    def tgcn_cell_bwd(rnn_type, gH, gates, c_rec, H, W_hh, h0=None, c0=None):
        """The reverse of tgcn_cell for gH = dL/dH (T, Hr) (ndcn_tgcn_cell_bwd_f32): (GGI (T, M), g_Whh, g_bhh, g_h0, g_c0 or None)."""
        kind = _lib.TGCN_TYPES[rnn_type]
        H = _panel(H, 'H')
        if H.dim() != 2:
            _refuse('H', 'a 2-D panel (T, Hr)', H)
        T, Hr = H.shape
        dev = H.device
        M = _lib.TGCN_GATES[kind] * Hr
        lstm = kind == _lib.TGCN_LSTM
        gH, gates = _operand(gH, 'gH', dev, shape=(T, Hr)), _operand(gates, 'gates', dev, shape=(T, 4 * Hr))
        W_hh = _operand(W_hh, 'W_hh', dev, shape=(M, Hr))
        c_rec = _operand(c_rec, 'c_rec', dev, shape=(T, Hr)) if lstm else None
        h0 = _operand(h0, 'h0', dev, numel=Hr).reshape(-1) if h0 is not None else None
        c0 = _operand(c0, 'c0', dev, numel=Hr).reshape(-1) if c0 is not None else None
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=gH.device)
        GGI, g_Whh, g_bhh, g_h0 = new(T, M), new(M, Hr), new(M), new(Hr)
        g_c0 = new(Hr) if lstm else None
        with torch.cuda.device(gH.device):
            check(_lib.load().ndcn_tgcn_cell_bwd_f32(kind, ptr(gH), ptr(gates), ptr(c_rec), ptr(H), ptr(h0), ptr(c0), ptr(W_hh), ptr(GGI),
                                                     ptr(g_Whh), ptr(g_bhh), ptr(g_h0), ptr(g_c0), T, Hr, stream_ptr()))
        return GGI, g_Whh, g_bhh, g_h0, g_c0

    @staticmethod
    def rhs_vjp(A, X, W, K, g, S=None, need_x=True, need_b=True, relu=True, premasked=False, acc_scale=1.0, gW=None, gb=None,
                no_graph=False, no_control=False, return_gs=False):
        """The reverse of one evaluation K = relu(W (A X) + b) (ndcn_rhs_vjp_f32): (gX, gW, gb) for the upstream gradient g, None
        where not requested.  S: A X as the forward wrote it (re-formed when None).  gW / gb given: the call ACCUMULATES
        acc_scale * (this evaluation's) into them and returns them; otherwise they are new tensors.  return_gs: a fourth result, the
        panel gS = gZ W as it stands in the call's scratch (need_x only).  Under set_rhs_abl_bwd a no_graph / no_control call that
        the one-launch reverse takes leaves no gS panel in the scratch: return_gs promises nothing there."""
        X, _, H = HipOps._rhs_input(X, None)
        n = X.shape[0]
        dev = X.device
        g, K, S = _like(g, 'g', X, shape=True), _like(K, 'K', X, shape=True), _like(S, 'S', X, shape=True)
        lib = _lib.load()
        flags = (_lib.F_RELU if relu else 0) | (_lib.F_NO_GRAPH if no_graph else 0) | (_lib.F_NO_CONTROL if no_control else 0)
        if no_graph:
            view = view_t = ctypes.byref(_lib.empty_csr(n))
        else:
            A = HipOps._rhs_operator(A, X, None)
            if A.shape[0] != n:
                raise _lib.NdcnHipError(_lib.EINVAL, 'the reverse takes a square operator, got %s' % (tuple(A.shape),))
            A.ensure_plans(H)
            At = A.transpose()
            At.ensure_plans(H)
            view, view_t = A.view_ref(), At.view_ref()
        accumulate = gW is not None
        if no_control:
            gW = gb = W = None                                  # (W is not read: no pointer of it is handed on)
        else:
            W = _operand(W, 'W', dev, shape=(H, H))
            if gW is None:
                gW = torch.empty((H, H), dtype=torch.float32, device=X.device)
                gb = torch.empty((H,), dtype=torch.float32, device=X.device) if need_b else None
            else:
                gW = _operand(gW, 'gW', dev, shape=(H, H), out=True)
                gb = _operand(gb, 'gb', dev, numel=H, out=True) if need_b and gb is not None else None
        gX = torch.empty_like(X) if need_x else None
        work = torch.empty(int(lib.ndcn_rhs_vjp_work_bytes(n, H, flags)), dtype=torch.uint8, device=X.device)
        with torch.cuda.device(X.device):
            check(lib.ndcn_rhs_vjp_f32(view, view_t, ptr(X), ptr(K), ptr(g), ptr(W), ptr(S), ptr(gX), ptr(gW), ptr(gb), ptr(work), H, flags,
                                       1 if premasked else 0, float(acc_scale), 1 if accumulate else 0, stream_ptr()))
        if not return_gs:
            return gX, gW, gb
        off = int(lib.ndcn_rhs_vjp_work_bytes(n, H, _lib.F_NO_CONTROL)) // 2
        gS = work[off:off + n * H * 4].view(torch.float32).view(n, H) if need_x else None
        return gX, gW, gb, gS

    @staticmethod
    def new_error_record(device):
        return ErrorRecord(device)

    @staticmethod
    def rhs_rk_xadd(A, X, xadd, xadd_c, W, b, y0, k_prev, cs):
        """The evaluation that opens a dopri5 step (ndcn_rhs_rk_xadd_f32): K = ODEFunc(X + xadd_c * xadd) and
        y_next = y0 + (cs[0] * k_prev + cs[1] * K) in one pass, the input formed on the rows the kernel stages - the bits of
        combine(X, [xadd], [xadd_c]) followed by rhs_rk(..., 'combine', y0, [k_prev], cs).  Returns (K, y_next), or None where
        the operator has no such kernel (ndcn_rhs_xadd_supported)."""
        X, _, H = HipOps._rhs_input(X, None)
        xadd, y0, k_prev = _like(xadd, 'xadd', X, shape=True), _like(y0, 'y0', X, shape=True), _like(k_prev, 'k_prev', X, shape=True)
        W = _operand(W, 'W', X.device, shape=(H, H))
        b = _operand(b, 'b', X.device, numel=H) if b is not None else None
        A = HipOps._rhs_operator(A, X, None)
        if A.shape[0] != X.shape[0]:
            raise _lib.NdcnHipError(_lib.EINVAL, 'the step-opening launch takes a square operator, got %s' % (tuple(A.shape),))
        A.ensure_plans(H)
        lib = _lib.load()
        flags = _lib.F_RELU
        if not int(lib.ndcn_rhs_xadd_supported(A.view_ref(), H, flags, _lib.RK_COMBINE, 1)):
            return None
        assert len(cs) == 2
        K, y_next = torch.empty_like(X), torch.empty_like(X)
        work = torch.empty(int(lib.ndcn_rhs_work_bytes(A.shape[0], H, flags)), dtype=torch.uint8, device=X.device)
        arr_c = (_F * 2)(float(cs[0]), float(cs[1]))
        with torch.cuda.device(X.device):
            check(lib.ndcn_rhs_rk_xadd_f32(A.view_ref(), ptr(X), ptr(xadd), float(xadd_c), ptr(W), ptr(b), ptr(K), ptr(work), H, flags,
                                           ptr(y0), ptr(k_prev), arr_c, ptr(y_next), stream_ptr()))
        return K, y_next

    @staticmethod
    def gather_rows(X, idx):
        X = _panel(X, 'X')
        if X.dim() != 2:
            _refuse('X', 'a 2-D panel', X)
        idx = _operand(idx, 'idx', X.device, dtype=torch.int32)
        out = torch.empty((idx.numel(), X.shape[1]), dtype=torch.float32, device=X.device)
        with torch.cuda.device(X.device):
            check(_lib.load().ndcn_gather_rows_f32(ptr(X), ptr(idx), idx.numel(), X.shape[1], ptr(out), stream_ptr()))
        return out

    # ---------------------------------------------------------------- Runge-Kutta bookkeeping
    @staticmethod
    def combine(y0, ks, cs):
        """y0 + sum_j cs[j] * ks[j]  (cs already dt*beta in fp32; misc.py:22-25 order and rounding)."""
        y0 = _panel(y0, 'y0')
        ks = _likes(ks, 'ks', y0)
        out = torch.empty_like(y0)
        arr_k, arr_c, n = _terms(ks, cs)
        with torch.cuda.device(y0.device):
            check(_lib.load().ndcn_rk_combine_f32(ptr(out), ptr(y0), arr_k, arr_c, n, y0.numel(), stream_ptr()))
        return out

    @staticmethod
    def lincomb(ks, cs, y0=None):
        """[y0 +] sum_j cs[j] * ks[j] in one pass (ndcn_rk_combine_f32 with or without the unit-coefficient term)."""
        k0 = _panel(ks[0], ('ks', 0))
        ks = [k0] + [_like(k, ('ks', j + 1), k0) for j, k in enumerate(ks[1:])]
        y0 = _like(y0, 'y0', k0)
        out = torch.empty_like(ks[0])
        arr_k, arr_c, n = _terms(ks, cs)
        with torch.cuda.device(out.device):
            check(_lib.load().ndcn_rk_combine_f32(ptr(out), ptr(y0), arr_k, arr_c, n, out.numel(),
                                                  stream_ptr()))
        return out

    READOUT_BWD_MAX_C = 15

    @staticmethod
    def readout_bwd(gd, Wd, y=None, base=None, addends=(), acc=None):
        """One tick of the decoder's backward inside a fixed-grid reverse sweep (ndcn_readout_bwd_f32): with gi = gd (N, C) . Wd (C, H)
        as the fp32 fma chain over c, returns base + (sum of the addends, left to right from +0, + gi) - lincomb(addends + [gi], ones,
        y0=base) without gi ever stored - or gi itself without base and addends.  acc (C * H + C float64, zeroed by the caller): += the
        decoder's gradients gd^T y and the column sums of gd for this tick, in a fixed order."""
        gd = _panel(gd, 'gd')
        if gd.dim() != 2:
            _refuse('gd', 'a 2-D panel (N, C)', gd)
        N, C = gd.shape
        dev = gd.device
        Wd = _operand(Wd, 'Wd', dev)
        if Wd.dim() != 2 or Wd.shape[0] != C:
            _refuse('Wd', 'a decoder weight of shape (%d, H)' % C, Wd)
        H = Wd.shape[1]
        assert len(addends) <= 5
        adds = [_operand(k, ('addends', j), dev, shape=(N, H)) for j, k in enumerate(addends)]
        base = _operand(base, 'base', dev, shape=(N, H)) if base is not None else None
        out = torch.empty((N, H), dtype=torch.float32, device=gd.device)
        lib = _lib.load()
        ws = None
        if acc is not None:
            y = _operand(y, 'y', dev, shape=(N, H))
            acc = _operand(acc, 'acc', dev, dtype=torch.float64, numel=C * H + C, out=True)
            ws = torch.empty(max(int(lib.ndcn_readout_bwd_ws_bytes(N, H, C)), 8), dtype=torch.uint8, device=gd.device)
        arr = (_P * max(len(adds), 1))(*[k.data_ptr() for k in adds])
        with torch.cuda.device(gd.device):
            check(lib.ndcn_readout_bwd_f32(ptr(out), ptr(base), arr, len(adds), ptr(gd), ptr(Wd), ptr(y) if acc is not None else None, N, H, C,
                                           ptr(acc), ptr(ws), stream_ptr()))
        return out

    @staticmethod
    def error(y0, y1, ks, cs, rtol, atol):
        """(sum of squared error ratios, non-finite count of y1) as host floats; one 16-byte read-back."""
        y0 = _panel(y0, 'y0')
        y1, ks = _like(y1, 'y1', y0), _likes(ks, 'ks', y0)
        red = _Reducer.get(y0.device)
        arr_k, arr_c, n = _terms(ks, cs)
        with _REDUCE_LOCK, torch.cuda.device(y0.device):
            check(_lib.load().ndcn_rk_error_f32(ptr(y0), ptr(y1), arr_k, arr_c, n, float(rtol), float(atol), y0.numel(),
                                                ptr(red.out), ptr(red.ws), stream_ptr()))
            return red.fetch()

    @staticmethod
    def scaled_sumsq(a, b, y, rtol, atol):
        """sum(((a - b) / (atol + |y| rtol))^2) and the non-finite count of a  (misc.py:121-138)."""
        a = _panel(a, 'a')
        y, b = _like(y, 'y', a), _like(b, 'b', a)
        red = _Reducer.get(a.device)
        with _REDUCE_LOCK, torch.cuda.device(a.device):
            check(_lib.load().ndcn_scaled_sumsq_f32(ptr(a), ptr(b), ptr(y), float(rtol), float(atol), a.numel(),
                                                    ptr(red.out), ptr(red.ws), stream_ptr()))
            return red.fetch()

    # ---------------------------------------------------------------- method 'adams': a step's algebra in three passes (csrc/adams_vc.hip)
    @staticmethod
    def set_adams_fused(mode):
        """The three-pass form of core.Adams.step for panels above the ATen-order bound: 0 off - every step runs the scale / combine /
        error calls -, 1 on; < 0: the environment's (NDCN_ADAMS_FUSED, default 1).  The results are the same bits either way.
        Process-wide; returns the previous mode."""
        global _ADAMS_FUSED_OVERRIDE
        prev = HipOps.adams_fused_on()
        _ADAMS_FUSED_OVERRIDE = None if int(mode) < 0 else (1 if int(mode) else 0)
        return prev

    @staticmethod
    def adams_fused_on():
        if _ADAMS_FUSED_OVERRIDE is not None:
            return _ADAMS_FUSED_OVERRIDE
        return 1 if _lib.env_int('NDCN_ADAMS_FUSED', 1) > 0 else 0

    # ---------------------------------------------------------------- explicit_adams / fixed_adams inference: the decoder inside the solve
    @staticmethod
    def set_adams_readout(mode):
        """odeint(..., method='explicit_adams' | 'fixed_adams', readout=...) without a gradient decodes each tick inside the library's
        solve (ndcn_solve_*_adams_readout_f32, csrc/adams.hip): 0 off - the solve stores the hidden trajectory and the Linear runs over
        it afterwards -, 1 on; < 0: the environment's (NDCN_ADAMS_READOUT, default 1).  The results are the same bits either way.
        Process-wide; returns the previous mode."""
        global _ADAMS_READOUT_OVERRIDE
        prev = HipOps.adams_readout_on()
        _ADAMS_READOUT_OVERRIDE = None if int(mode) < 0 else (1 if int(mode) else 0)
        return prev

    @staticmethod
    def adams_readout_on():
        if _ADAMS_READOUT_OVERRIDE is not None:
            return _ADAMS_READOUT_OVERRIDE
        return 1 if _lib.env_int('NDCN_ADAMS_READOUT', 1) > 0 else 0

    @staticmethod
    def adams_readout_route(H, C, weight_ok=True, needs_grad=False, enabled=True):
        """Does a device-resident explicit_adams / fixed_adams solve at hidden width H take the decoder (C, H) inside the library?  The
        admissible shapes of ndcn_ab_step_readout_f32 - H = 16, 20, .. 60 (the decoder's small route) or 64 <= H <= 512 (its row-dot
        route), 1 <= C <= 15 -, a float32 device weight of that shape (weight_ok), no gradient asked of the decoder, the switch on."""
        wide = 64 <= H <= 512
        narrow = 16 <= H <= 60 and H % 4 == 0
        return bool(enabled and weight_ok and not needs_grad and (wide or narrow) and 1 <= C <= 15)

    @staticmethod
    def adams_fusable(*panels):
        """May core.Adams.step take the three-pass form for these panels of one state tensor?  Contiguous float32 device panels of more
        elements than the ATen-order bound (at or below it ndcn_rk_error_f32 sums in ATen's float32 order, which the fused sums do not
        reproduce), 16-byte aligned (so that both forms take the same element path)."""
        if not HipOps.adams_fused_on():
            return False
        n = panels[0].numel()
        if n <= int(_lib.load().ndcn_aten_norm_max()):
            return False
        return all(p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() and p.numel() == n and p.data_ptr() % 16 == 0
                   for p in panels)

    @staticmethod
    def _adams_phi(phis, betas, order, ref):
        phis = _likes(phis[:order], 'phis', ref)
        assert len(phis) == order and len(betas) >= order
        arr_p = (_P * order)(*[p.data_ptr() for p in phis])
        arr_b = (_F * order)(*[0.0 if (j == 0 or betas[j] is None) else float(betas[j]) for j in range(order)])
        return phis, arr_p, arr_b

    @staticmethod
    def adams_predict(y, phis, betas, cs, order):
        """p_next = y + sum_j cs[j] e_j over the first max(1, order - 1) explicit phi e_0 = phis[0], e_j = betas[j] * phis[j] - the bits of
        scale x (order - 2) + combine, the explicit phi never stored (ndcn_adams_predict_f32)."""
        y = _panel(y, 'y')
        phis, arr_p, arr_b = HipOps._adams_phi(phis, betas, order, y)
        m = max(1, order - 1)
        assert len(cs) == m
        arr_c = (_F * m)(*[float(c) for c in cs])
        out = torch.empty_like(y)
        with torch.cuda.device(y.device):
            check(_lib.load().ndcn_adams_predict_f32(ptr(out), ptr(y), arr_p, arr_b, arr_c, order, y.numel(), stream_ptr()))
        return out

    @staticmethod
    def adams_correct(nf, phis, betas, order, p_next, y0, c_corr, coefs, rtol, atol):
        """(y_next, sums): y_next = p_next + c_corr * ip_{order-1} with the predictor's implicit phi chain ip_0 = nf, ip_j = ip_{j-1} - e_{j-1}
        held in registers, and for every coefs[q] that is not None the sum of squared error ratios of coefs[q] * {ip_order, ip_{order-1},
        ip_{order-2}, ip_order}[q] against (y0, y_next) as a host float - what `error` returns above the ATen-order bound -, None for the
        others; one 32-byte read-back (ndcn_adams_correct_f32)."""
        y0 = _panel(y0, 'y0')
        nf, p_next = _like(nf, 'nf', y0), _like(p_next, 'p_next', y0)
        phis, arr_p, arr_b = HipOps._adams_phi(phis, betas, order, y0)
        assert len(coefs) == 4
        mask = sum(1 << q for q in range(4) if coefs[q] is not None)
        arr_c = (_F * 4)(*[0.0 if c is None else float(c) for c in coefs])
        red = _Reducer.get(y0.device)
        lib = _lib.load()
        out = torch.empty_like(p_next)
        with _REDUCE_LOCK, torch.cuda.device(y0.device):
            if getattr(red, 'ws4', None) is None:
                red.ws4 = torch.empty(int(lib.ndcn_adams_correct_ws_bytes()), dtype=torch.uint8, device=y0.device)
                red.out4 = torch.zeros(4, dtype=torch.float64, device=y0.device)
                red.host4 = torch.zeros(4, dtype=torch.float64).pin_memory()
            check(lib.ndcn_adams_correct_f32(ptr(out), ptr(nf), arr_p, arr_b, order, ptr(p_next), ptr(y0), float(c_corr), arr_c, mask,
                                             float(rtol), float(atol), y0.numel(), ptr(red.out4), ptr(red.ws4), red.ws4.numel(), stream_ptr()))
            red.host4.copy_(red.out4, non_blocking=True)
            torch.cuda.current_stream().synchronize()
            sums = [float(red.host4[q]) if coefs[q] is not None else None for q in range(4)]
        return out, sums

    @staticmethod
    def adams_update(nf2, phis, betas, order, n_out):
        """The implicit phi of an accepted step: [nf2, nf2 - e_0, (nf2 - e_0) - e_1, ...], n_out panels, the first nf2 itself; one pass,
        out of place (ndcn_adams_update_f32)."""
        nf2 = _panel(nf2, 'nf2')
        assert 1 <= n_out <= order + 1
        phis, arr_p, arr_b = HipOps._adams_phi(phis, betas, order, nf2)
        outs = [nf2] + [torch.empty_like(nf2) for _ in range(n_out - 1)]
        arr_o = (_P * n_out)(*[o.data_ptr() for o in outs])
        with torch.cuda.device(nf2.device):
            check(_lib.load().ndcn_adams_update_f32(arr_o, ptr(nf2), arr_p, arr_b, order, n_out, nf2.numel(), stream_ptr()))
        return outs

    # ---------------------------------------------------------------- VJPs of the dopri5 panel operations
    @staticmethod
    def combine_bwd(g, ks, cs, need_k, need_dots=True, accs=None, acc_y0=None, lazy=False):
        """VJP of combine: ([c_j g or None], [<g, k_j>] as host floats or None).  accs / acc_y0: gradients the terms / y0 have
        already received - the outputs become acc_j + c_j g (and a third result acc_y0 + g is returned when acc_y0 is given).
        lazy: the inner products as deferred 0-d float32 host tensors (_BwdDots.lazy) instead of floats."""
        g = _panel(g, 'g')
        ks = _likes(ks, 'ks', g)
        assert len(need_k) == len(ks)
        arr_k, arr_c, n = _terms(ks, cs)
        gk, arr_g = _grad_ptrs(g, need_k)
        accs, arr_a = _acc_ptrs(accs, n, g)
        gy0 = torch.empty_like(g) if acc_y0 is not None else None
        acc_y0 = _like(acc_y0, 'acc_y0', g)
        d = _BwdDots.get(g.device)
        with _REDUCE_LOCK, torch.cuda.device(g.device):
            check(_lib.load().ndcn_rk_combine_bwd_f32(ptr(g), arr_k, arr_c, n, arr_g, arr_a, ptr(gy0),
                                                      ptr(acc_y0), ptr(d.out), ptr(d.ws),
                                                      g.numel(), stream_ptr()))
            dots = (d.lazy(n) if lazy else d.fetch()[:n]) if need_dots else None
        return (gk, dots) if acc_y0 is None else (gk, dots, gy0)

    @staticmethod
    def pull(ps, cs, base=None, mask=None, ua=None, ub=None, out=None):
        """The tape's pull: (out, <p_0, ua - ub> as a host float or None).  out = base + ((c_0 p_0 + c_1 p_1) + ...) with combine's
        order and rounding, zeroed where mask <= 0 (threshold_backward: a NaN mask passes); ua / ub / base / mask nullable."""
        p0 = _panel(ps[0], ('ps', 0))
        ps = [p0] + [_like(p, ('ps', j + 1), p0) for j, p in enumerate(ps[1:])]
        base, mask, ua, ub = _like(base, 'base', p0), _like(mask, 'mask', p0), _like(ua, 'ua', p0), _like(ub, 'ub', p0)
        arr_p, arr_c, n = _terms(ps, cs)
        out = torch.empty_like(p0) if out is None else _like(out, 'out', p0, out=True)
        d = _BwdDots.get(ps[0].device)
        with _REDUCE_LOCK, torch.cuda.device(ps[0].device):
            check(_lib.load().ndcn_rk_pull_f32(ptr(out), ptr(base), arr_p, arr_c, n, ptr(mask), ptr(ua), ptr(ub), ptr(d.out), ptr(d.ws),
                                               ps[0].numel(), stream_ptr()))
            return out, (d.fetch()[0] if ua is not None else None)

    @staticmethod
    def dot_diff(g, a, b=None, scale=1.0, lazy=False):
        """scale * <g, a - b> (fp64 sum, fixed order): a float, or with lazy a deferred 0-d float32 host tensor (_BwdDots.lazy)"""
        g = _panel(g, 'g')
        a, b = _like(a, 'a', g), _like(b, 'b', g)
        d = _BwdDots.get(g.device)
        with _REDUCE_LOCK, torch.cuda.device(g.device):
            check(_lib.load().ndcn_rk_dot_diff_f32(ptr(g), ptr(a), ptr(b), ptr(d.out), ptr(d.ws), g.numel(), stream_ptr()))
            return d.lazy(1, scale)[0] if lazy else d.fetch()[0] * scale

    @staticmethod
    def error_bwd(y0, y1, ks, cs, rtol, atol, g_r, need_y0, need_y1, need_k, need_dots=True, accs=None, acc_y0=None, acc_y1=None, lazy=False):
        """VJP of the error ratio mean(((sum c_j k_j) / tol)^2) for upstream gradient g_r:
        (gy0, gy1, [gk_j], [d ratio / d c_j] (NOT yet multiplied by g_r) as host floats); accs / acc_y0 / acc_y1 as combine_bwd."""
        y0 = _panel(y0, 'y0')
        y1, ks = _like(y1, 'y1', y0), _likes(ks, 'ks', y0)
        acc_y0, acc_y1 = _like(acc_y0, 'acc_y0', y0), _like(acc_y1, 'acc_y1', y0)
        assert len(need_k) == len(ks)
        arr_k, arr_c, n = _terms(ks, cs)
        gk, arr_g = _grad_ptrs(y0, need_k)
        accs, arr_a = _acc_ptrs(accs, n, y0)
        gy0 = torch.empty_like(y0) if need_y0 else None
        gy1 = torch.empty_like(y0) if need_y1 else None
        d = _BwdDots.get(y0.device)
        with _REDUCE_LOCK, torch.cuda.device(y0.device):
            check(_lib.load().ndcn_rk_error_bwd_f32(ptr(y0), ptr(y1), arr_k, arr_c, n, float(rtol), float(atol), float(g_r),
                                                    1.0 / y0.numel(), ptr(gy0), ptr(gy1), arr_g,
                                                    ptr(acc_y0), ptr(acc_y1), arr_a, ptr(d.out), ptr(d.ws),
                                                    y0.numel(), stream_ptr()))
            if lazy:                          # deferred, already multiplied by g_r (the eager form leaves that to the caller)
                return gy0, gy1, gk, (d.lazy(n, float(g_r)) if need_dots else None)
            return gy0, gy1, gk, (d.fetch()[:n] if need_dots else None)

    @staticmethod
    def rms_bwd(a, b, y, rtol, atol, coef, need_a, need_b, need_y):
        """VJP of ||(a - b) / (atol + |y| rtol)|| / sqrt(N); coef = g / (||.|| sqrt(N))."""
        a = _panel(a, 'a')
        y, b = _like(y, 'y', a), _like(b, 'b', a)
        ga = torch.empty_like(a) if need_a else None
        gb = torch.empty_like(a) if (need_b and b is not None) else None
        gy = torch.empty_like(a) if need_y else None
        with torch.cuda.device(a.device):
            check(_lib.load().ndcn_rk_rms_bwd_f32(ptr(a), ptr(b), ptr(y), float(rtol), float(atol), float(coef), ptr(ga),
                                                  ptr(gb), ptr(gy), a.numel(), stream_ptr()))
        return ga, gb, gy

    @staticmethod
    def interp_bwd(g, y0, y1, ks, dt, x, need_y0, need_y1, need_k, need_dots=True, accs=None, acc_y0=None, acc_y1=None):
        """VJP of the dopri5 dense output at abscissa x: (gy0, gy1, [gk_j], <g, do/dx>, <g, do/ddt>); accs / acc_y0 / acc_y1 as
        combine_bwd."""
        g = _panel(g, 'g')
        y0, y1, ks = _like(y0, 'y0', g), _like(y1, 'y1', g), _likes(ks, 'ks', g)
        acc_y0, acc_y1 = _like(acc_y0, 'acc_y0', g), _like(acc_y1, 'acc_y1', g)
        assert len(ks) == 7 and len(need_k) == 7
        arr_k = (_P * 7)(*[k.data_ptr() for k in ks])
        gk, arr_g = _grad_ptrs(g, need_k)
        accs, arr_a = _acc_ptrs(accs, 7, g)
        gy0 = torch.empty_like(g) if need_y0 else None
        gy1 = torch.empty_like(g) if need_y1 else None
        d = _BwdDots.get(g.device)
        with _REDUCE_LOCK, torch.cuda.device(g.device):
            check(_lib.load().ndcn_dopri5_interp_bwd_f32(ptr(g), ptr(y0), ptr(y1), arr_k, float(dt), float(x), ptr(gy0),
                                                         ptr(gy1), arr_g, ptr(acc_y0), ptr(acc_y1), arr_a, ptr(d.out),
                                                         ptr(d.ws), g.numel(), stream_ptr()))
            dots = d.fetch() if need_dots else (0.0, 0.0)
        return gy0, gy1, gk, dots[0], dots[1]

    @staticmethod
    def interp_direct_multi(y0, y1, ks, cmid, dt, xpows):
        """len(xpows) <= 7 ticks of one step in one pass: [dense output at each tick] - per tick the arithmetic of interp_direct."""
        y0 = _panel(y0, 'y0')
        y1, ks = _like(y1, 'y1', y0), _likes(ks, 'ks', y0)
        nt = len(xpows)
        assert len(ks) == 7 and 1 <= nt <= 7
        outs = [torch.empty_like(y0) for _ in range(nt)]
        arr_k, arr_c, _ = _terms(ks, cmid)
        xp = (_F * (5 * nt))(*[float(v) for row in xpows for v in row])
        arr_o = (_P * nt)(*[o.data_ptr() for o in outs])
        with torch.cuda.device(y0.device):
            check(_lib.load().ndcn_dopri5_interp_direct_multi_f32(ptr(y0), ptr(y1), arr_k, arr_c, float(dt), xp, arr_o, nt, y0.numel(),
                                                                  stream_ptr()))
        return outs

    @staticmethod
    def interp_bwd_multi(gs, y0, y1, ks, dt, xs, need_y0, need_y1, need_k, accs=None, acc_y0=None, acc_y1=None, lazy=False):
        """VJP of len(gs) <= 7 dense outputs of ONE step: (gy0, gy1, [gk_j], [<g_t, do/dx_t>], sum_t <g_t, do/ddt>)."""
        y0 = _panel(y0, 'y0')
        y1, ks, gs = _like(y1, 'y1', y0), _likes(ks, 'ks', y0), _likes(gs, 'gs', y0)
        acc_y0, acc_y1 = _like(acc_y0, 'acc_y0', y0), _like(acc_y1, 'acc_y1', y0)
        nt = len(gs)
        assert len(ks) == 7 and 1 <= nt <= 7 and len(xs) == nt and len(need_k) == 7
        arr_k = (_P * 7)(*[k.data_ptr() for k in ks])
        arr_gs = (_P * nt)(*[g.data_ptr() for g in gs])
        arr_x = (_F * nt)(*[float(v) for v in xs])
        gk, arr_g = _grad_ptrs(y0, need_k)
        accs, arr_a = _acc_ptrs(accs, 7, y0)
        gy0 = torch.empty_like(y0) if need_y0 else None
        gy1 = torch.empty_like(y0) if need_y1 else None
        d = _BwdDots.get(y0.device)
        with _REDUCE_LOCK, torch.cuda.device(y0.device):
            check(_lib.load().ndcn_dopri5_interp_bwd_multi_f32(arr_gs, nt, ptr(y0), ptr(y1), arr_k, float(dt), arr_x, ptr(gy0), ptr(gy1), arr_g,
                                                               ptr(acc_y0), ptr(acc_y1), arr_a, ptr(d.out),
                                                               ptr(d.ws), y0.numel(), stream_ptr()))
            if lazy:
                dots = d.lazy(8)
                return gy0, gy1, gk, dots[:nt], dots[7]
            dots = d.fetch()
        return gy0, gy1, gk, list(dots[:nt]), dots[7]

    @staticmethod
    def interp_fit(y0, y1, ks, cmid, dt):
        y0 = _panel(y0, 'y0')
        y1, ks = _like(y1, 'y1', y0), _likes(ks, 'ks', y0)
        assert len(ks) == 7
        a, b, c, d = (torch.empty_like(y0) for _ in range(4))
        arr_k, arr_c, _ = _terms(ks, cmid)
        with torch.cuda.device(y0.device):
            check(_lib.load().ndcn_dopri5_interp_fit_f32(ptr(y0), ptr(y1), arr_k, arr_c, float(dt), ptr(a), ptr(b), ptr(c),
                                                         ptr(d), y0.numel(), stream_ptr()))
        return a, b, c, d

    @staticmethod
    def interp_direct(y0, y1, ks, cmid, dt, xpow, out=None):
        """interp_fit + interp_eval in one pass, coefficients not stored (same arithmetic, bit-identical)."""
        y0 = _panel(y0, 'y0')
        y1, ks = _like(y1, 'y1', y0), _likes(ks, 'ks', y0)
        assert len(ks) == 7
        out = torch.empty_like(y0) if out is None else _like(out, 'out', y0, out=True)
        arr_k, arr_c, _ = _terms(ks, cmid)
        xp = (_F * 5)(*[float(v) for v in xpow])
        with torch.cuda.device(y0.device):
            check(_lib.load().ndcn_dopri5_interp_direct_f32(ptr(y0), ptr(y1), arr_k, arr_c, float(dt), xp, ptr(out),
                                                            y0.numel(), stream_ptr()))
        return out

    @staticmethod
    def interp_eval(fit, e, xpow, out=None):
        """`fit` = the (a, b, c, d) panels interp_fit returned; e = y at the start of the fitted step."""
        e = _panel(e, 'e')
        a, b, c, d = _likes(fit, 'fit', e)
        out = torch.empty_like(e) if out is None else _like(out, 'out', e, out=True)
        xp = (_F * 5)(*[float(v) for v in xpow])
        with torch.cuda.device(e.device):
            check(_lib.load().ndcn_interp_eval_f32(ptr(a), ptr(b), ptr(c), ptr(d), ptr(e), xp, ptr(out), e.numel(),
                                                   stream_ptr()))
        return out

    @staticmethod
    def fixed_stage(op, y, k1, k2=None, k3=None, k4=None, dt=0.0, out=None):
        y = _panel(y, 'y')
        ks = [_like(k, ('k', j + 1), y) for j, k in enumerate((k1, k2, k3, k4))]
        out = torch.empty_like(y) if out is None else _like(out, 'out', y, out=True)
        with torch.cuda.device(y.device):
            check(_lib.load().ndcn_fixed_stage_f32(int(op), ptr(out), ptr(y), ptr(ks[0]), ptr(ks[1]), ptr(ks[2]),
                                                   ptr(ks[3]), float(dt), y.numel(), stream_ptr()))
        return out

    @staticmethod
    def ab_step(y, fs, coeffs, dt, out=None):
        """One Adams-Bashforth step (fixed_adams.py:180-182 + solvers.py:92): y + dt * (((0 + a_0 f_0) + a_1 f_1) + ...), every product
        and sum rounded on its own - ndcn_ab_step_f32; fs: the 3..11 newest evaluations, newest first; coeffs: their float32 weights.
        out may be y."""
        y = _panel(y, 'y')
        fs = _likes(fs, 'fs', y)
        out = torch.empty_like(y) if out is None else _like(out, 'out', y, out=True)
        arr_f, arr_a, n = _terms(fs, coeffs)
        with torch.cuda.device(y.device):
            check(_lib.load().ndcn_ab_step_f32(ptr(out), ptr(y), arr_f, arr_a, n, float(dt), y.numel(), stream_ptr()))
        return out

    @staticmethod
    def ab_step_readout(y, fs, coeffs, dt, weight, bias=None, emit_off=0.0, out=None):
        """(new state, decoded): ab_step on an (N, H) panel that also writes linear(s, weight, bias), shape (N, C), in the same launch
        (ndcn_ab_step_readout_f32) - s the new state, or with emit_off != 0 the tick s + ((s - s) / dt) * emit_off of a sub-stepped
        grid; the bits of hip.linear on that panel.  H = 16, 20, .. 60 or 64 <= H <= 512, C <= 15; out may be y."""
        y = _panel(y, 'y')
        fs = _likes(fs, 'fs', y)
        assert y.dim() == 2 and weight.dim() == 2 and weight.shape[1] == y.shape[1]
        weight = _operand(weight, 'weight', y.device)
        bias = None if bias is None else _operand(bias, 'bias', y.device, numel=weight.shape[0])
        out = torch.empty_like(y) if out is None else _like(out, 'out', y, out=True)
        dec = torch.empty((y.shape[0], weight.shape[0]), dtype=torch.float32, device=y.device)
        arr_f, arr_a, n = _terms(fs, coeffs)
        with torch.cuda.device(y.device):
            check(_lib.load().ndcn_ab_step_readout_f32(ptr(out), ptr(y), arr_f, arr_a, n, float(dt), y.shape[0], y.shape[1], ptr(weight),
                                                       ptr(bias), weight.shape[0], ptr(dec), float(emit_off), stream_ptr()))
        return out, dec

    @staticmethod
    def abm_predict(y, fs, a, m, dt):
        """(dy, delta, u) of a fixed_adams step that holds len(fs) = 3..11 evaluations (fixed_adams.py:180-188): dy = dt * sum a_i f_i,
        delta = dt * sum m_i f_i, u = y + dy - one pass over the history, every product and sum rounded on its own
        (ndcn_abm_predict_f32).  a: the Adams-Bashforth weights, m: the Adams-Moulton weights of the history (core.am_weights)."""
        y = _panel(y, 'y')
        fs = _likes(fs, 'fs', y)
        assert len(a) == len(fs) == len(m)
        dy, delta, u = torch.empty_like(y), torch.empty_like(y), torch.empty_like(y)
        arr_f, arr_a, n = _terms(fs, a)
        arr_m = (_F * n)(*[float(c) for c in m])
        with torch.cuda.device(y.device):
            check(_lib.load().ndcn_abm_predict_f32(ptr(dy), ptr(delta), ptr(u), ptr(y), arr_f, arr_a, arr_m, n, float(dt), y.numel(),
                                                   stream_ptr()))
        return dy, delta, u

    @staticmethod
    def abm_correct(f, delta, y, dy, c0, rtol, atol):
        """One corrector iteration (fixed_adams.py:192-194): (dy, u, failed) with dy <- c0 * f + delta IN PLACE, u = y + dy a new panel and
        `failed` the number of elements for which |dy_old - dy_new| < atol + rtol * max(|dy_old|, |dy_new|) does not hold, as a host int -
        counted in integers on the device, one 8-byte read-back (ndcn_abm_correct_f32)."""
        y = _panel(y, 'y')
        f, delta = _like(f, 'f', y), _like(delta, 'delta', y)
        dy = _like(dy, 'dy', y, out=True)
        u = torch.empty_like(y)
        red = _Reducer.get(y.device)
        with _REDUCE_LOCK, torch.cuda.device(y.device):
            if getattr(red, 'count', None) is None:
                red.count = torch.zeros(1, dtype=torch.int64, device=y.device)
                red.count_host = torch.zeros(1, dtype=torch.int64).pin_memory()
            check(_lib.load().ndcn_abm_correct_f32(ptr(dy), ptr(u), ptr(f), ptr(delta), ptr(y), float(c0), float(rtol), float(atol),
                                                   y.numel(), ptr(red.count), stream_ptr()))
            red.count_host.copy_(red.count, non_blocking=True)
            torch.cuda.current_stream().synchronize()
            failed = int(red.count_host[0])
        return dy, u, failed

    @staticmethod
    def ab_adjoint(gs, cs, base=None, out=None):
        """The gradient of one evaluation of an explicit_adams solve, gathered from the adjoints of the Adams-Bashforth steps that used
        it (ndcn_ab_adjoint_f32): [base +] (((0 + c_0 g_0) + c_1 g_1) + ...), every product and sum rounded on its own, the base added
        last.  gs: 1..11 panels, cs: their float32 coefficients (core.ab_adjoint_terms).  out may be base, never one of gs."""
        g0 = _panel(gs[0], ('gs', 0))
        gs = [g0] + [_like(g, ('gs', j + 1), g0) for j, g in enumerate(gs[1:])]
        base = _like(base, 'base', g0)
        out = torch.empty_like(g0) if out is None else _like(out, 'out', g0, out=True)
        arr_g, arr_c, n = _terms(gs, cs)
        with torch.cuda.device(out.device):
            check(_lib.load().ndcn_ab_adjoint_f32(ptr(out), ptr(base), arr_g, arr_c, n, out.numel(), stream_ptr()))
        return out

    @staticmethod
    def abm_adjoint(ps, cps, ds, cds, base=None, out=None):
        """The gradient of one evaluation of a fixed_adams solve, gathered from the adjoints of the predictor-corrector steps that held
        it (ndcn_abm_adjoint_f32): [base +] ((((0 + cp_0 P_0) + cd_0 D_0) + cp_1 P_1) + cd_1 D_1 ...), every product and sum rounded on
        its own, the base added last.  ps / ds: 1..11 panels each (P_q may be D_q), cps / cds: their float32 coefficients
        (core.abm_adjoint_terms).  out may be base, never a term."""
        p0 = _panel(ps[0], ('ps', 0))
        ps, ds = [p0] + [_like(g, ('ps', j + 1), p0) for j, g in enumerate(ps[1:])], _likes(ds, 'ds', p0)
        assert len(ps) == len(ds) == len(cps) == len(cds)
        base = _like(base, 'base', p0)
        out = torch.empty_like(p0) if out is None else _like(out, 'out', p0, out=True)
        arr_p, arr_cp, n = _terms(ps, cps)
        arr_d, arr_cd, _ = _terms(ds, cds)
        with torch.cuda.device(out.device):
            check(_lib.load().ndcn_abm_adjoint_f32(ptr(out), ptr(base), arr_p, arr_cp, arr_d, arr_cd, n, out.numel(), stream_ptr()))
        return out

    @staticmethod
    def tick_emit(y, dt, tms, outs=None):
        """The ticks a sub-stepped fixed-grid step reports that are NOT an end of the step (solvers.py:92-108, y0 already overwritten
        with y1): [y + ((y - y) / dt) * tm for tm in tms] - one pass over y per 8 ticks (ndcn_tick_emit_f32)."""
        y = _panel(y, 'y')
        nt = len(tms)
        if outs is None:
            outs = [torch.empty_like(y) for _ in range(nt)]
        assert len(outs) == nt
        for j, o in enumerate(outs):
            _like(o, ('outs', j), y, out=True)
        if nt == 0:
            return outs
        arr_t = (_F * nt)(*[float(v) for v in tms])
        arr_s = (ctypes.c_int * nt)(*([0] * nt))
        arr_o = (_P * nt)(*[o.data_ptr() for o in outs])
        with torch.cuda.device(y.device):
            check(_lib.load().ndcn_tick_emit_f32(ptr(y), float(dt), arr_t, arr_s, arr_o, nt, y.numel(), stream_ptr()))
        return outs

    # ---------------------------------------------------------------- truth dynamics (N x 1 state)
    @staticmethod
    def row_l1_normalize(X, out=None):
        """F.normalize(X, p=1, dim=1) with infinities zeroed (ode_gcn.py:9-26)."""
        X = _panel(X, 'X')
        if X.dim() != 2:
            _refuse('X', 'a 2-D panel', X)
        out = torch.empty_like(X) if out is None else _like(out, 'out', X, out=True, shape=True)
        with torch.cuda.device(X.device):
            check(_lib.load().ndcn_row_l1_normalize_f32(ptr(X), ptr(out), X.shape[0], X.shape[1], stream_ptr()))
        return out

    @staticmethod
    def row_l1_normalize_bwd(g, X):
        """VJP of row_l1_normalize at X for the upstream gradient g."""
        X = _panel(X, 'X')
        if X.dim() != 2:
            _refuse('X', 'a 2-D panel', X)
        g = _like(g, 'g', X, shape=True)
        out = torch.empty_like(X)
        with torch.cuda.device(X.device):
            check(_lib.load().ndcn_row_l1_normalize_bwd_f32(ptr(g), ptr(X), ptr(out), X.shape[0], X.shape[1], stream_ptr()))
        return out

    @staticmethod
    def _state(A, x):
        """the N x 1 state of a truth-dynamics launch on the square operator A"""
        x = _panel(x, 'x')
        if not (x.numel() == A.shape[0] == A.shape[1]) or A.device != x.device:
            raise _lib.NdcnHipError(_lib.EINVAL, 'operator %s on %s, state of %d elements on %s' % (tuple(A.shape), A.device, x.numel(), x.device))
        return x

    @staticmethod
    def gene_rhs(A, x, b=1.0, f=1.0, h=2.0):
        A = as_csr(A)
        x = HipOps._state(A, x)
        out = torch.empty_like(x)
        with torch.cuda.device(x.device):
            check(_lib.load().ndcn_gene_rhs_f32(A.view_ref(), ptr(x), ptr(out), float(b), float(f), float(h), stream_ptr()))
        return out

    @staticmethod
    def mutual_rhs(A, x, b=0.1, k=5., c=1., d=5., e=0.9, h=0.1):
        A = as_csr(A)
        x = HipOps._state(A, x)
        out = torch.empty_like(x)
        with torch.cuda.device(x.device):
            check(_lib.load().ndcn_mutual_rhs_f32(A.view_ref(), ptr(x), ptr(out), float(b), float(k), float(c), float(d),
                                                  float(e), float(h), stream_ptr()))
        return out

    @staticmethod
    def dyn_rk(kind, params, A, x, mode='plain', y0=None, kprev=(), cs=(), rtol=0.0, atol=0.0, y1=None, aux_cs=None, c_dev=None):
        """One of the truth dynamics on an N x 1 state plus, in the same launch, the stage algebra consuming K (ndcn_dyn_rk_f32):
        rhs_rk's contract.  kind: 'heat' (params (k,); A = L), 'gene' (b, f, h) or 'mutual' (b, k, c, d, e, h).
        mode 'plain': returns K; 'combine': (K, y0 + sum cs[m] kprev[m] + cs[-1] K), with aux_cs also the second combination
        (K, y_next, y_aux); 'rk4': stage len(kprev) of the 3/8-rule step, cs = [dt]: (K, next stage input / step result);
        'error': (K, (sum of squared error ratios, non-finite count of y1)), y1 defaulting to x.
        c_dev: a float32 device tensor holding the coefficients in place of cs (what a replayed step reads)."""
        A = as_csr(A)
        x = HipOps._state(A, x)
        dyn = _lib.dynamics({'heat': _lib.DYN_HEAT, 'gene': _lib.DYN_GENE, 'mutual': _lib.DYN_MUTUAL}.get(kind, kind), params)
        rk = {'plain': _lib.RK_NONE, 'combine': _lib.RK_COMBINE, 'error': _lib.RK_ERROR, 'rk4': _lib.RK_RK4}[mode]
        kprev = _likes(kprev, 'kprev', x)
        y0, y1 = _like(y0, 'y0', x), _like(y1, 'y1', x)
        K = torch.empty_like(x)
        y_next = torch.empty_like(x) if mode in ('combine', 'rk4') else None
        arr_k = (_P * max(len(kprev), 1))(*[k.data_ptr() for k in kprev])
        arr_c = (_F * len(cs))(*[float(c) for c in cs]) if len(cs) else None
        y_aux = arr_c2 = None
        if aux_cs is not None:
            arr_c2 = (_F * len(aux_cs))(*[float(c) for c in aux_cs])
            y_aux = torch.empty_like(x)
        if c_dev is not None:
            c_dev = _operand(c_dev, 'c_dev', x.device)          # (how many coefficients the replayed step reads is the C side's knowledge)
        red = _Reducer.get(x.device)
        with _REDUCE_LOCK, torch.cuda.device(x.device):
            check(_lib.load().ndcn_dyn_rk_f32(ctypes.byref(dyn), A.view_ref(), ptr(x), ptr(K), rk, ptr(y0), arr_k, arr_c, len(kprev),
                                              ptr(y_next), ptr(y1), ptr(y_aux), arr_c2, float(rtol), float(atol), ptr(red.out),
                                              ptr(red.ws), ptr(c_dev), stream_ptr()))
            if mode == 'error':
                return K, red.fetch()
        if mode == 'plain':
            return K
        return (K, y_next, y_aux) if aux_cs is not None else (K, y_next)


hip = HipOps()


def new_solve_epoch():
    """Called at the top of every odeint / odeint_adjoint: packed weight images of earlier solves are re-validated by re-packing
    (see _PackedWeights)."""
    _PackedWeights.new_epoch()


def invalidate_packed_weights():
    """Drop the cached packed images of ODEFunc weights (see _PackedWeights): call after writing weights in a way that
    does not move the tensor's version counter (`.data` writes, collectives on `.data`, raw-pointer writes)."""
    _PackedWeights.invalidate()


def device_info():
    out = (ctypes.c_int64 * 6)()
    check(_lib.load().ndcn_device_info(out))
    keys = ('compute_units', 'xcds', 'wave_size', 'clock_khz', 'hbm_mib', 'l2_kib')
    return dict(zip(keys, [int(v) for v in out]))


__all__ = ['HipOps', 'hip', 'device_info', 'CsrOperator', 'as_csr', 'invalidate_packed_weights']
