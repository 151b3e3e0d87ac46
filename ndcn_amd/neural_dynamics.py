"""Drop-in for the classes of the reference's neural_dynamics.py: ODEFunc, ODEBlock, ODEBlock2, NDCN,
GraphConvolution, TemporalGCN - same constructor signatures, attribute names and state_dict keys
(SURVEY.md 8b), computed by the HIP kernels of libndcn_hip.so.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from . import dropout as _dropout
from . import torchdiffeq as ode
from .ops import hip


def _needs_grad(*tensors_and_modules):
    if not torch.is_grad_enabled():
        return False
    for obj in tensors_and_modules:
        if isinstance(obj, nn.Module):
            if any(p.requires_grad for p in obj.parameters()):
                return True
        elif torch.is_tensor(obj) and obj.requires_grad:
            return True
    return False


def _has_hooks(module):
    return bool(module._forward_hooks or module._forward_pre_hooks or module._backward_hooks or module._backward_pre_hooks)


class ODEFunc(nn.Module):
    """dX/dt = relu(dropout(W (A X) + b))   -- reference neural_dynamics.py:8-39."""

    ndcn_autonomous = True        # forward ignores t (neural_dynamics.py:20-26)

    def __init__(self, hidden_size, A, dropout=0.0, no_graph=False, no_control=False):
        super(ODEFunc, self).__init__()
        self.hidden_size = hidden_size
        self.dropout = dropout
        self.dropout_layer = nn.Dropout(dropout)
        self.A = A  # N_node * N_node: dense tensor, torch sparse tensor or ndcn_amd.CsrOperator
        self.wt = nn.Linear(hidden_size, hidden_size)
        self.no_graph = no_graph
        self.no_control = no_control

    def forward(self, t, x):
        if _dropout.is_active(self):
            # stochastic RHS, 0 < p < 1: the factor is 0 or 1 / (1 - p) > 0, so relu(dropout(z)) = relu(z) * m - one fused launch (and
            # one autograd node) with the counter-based mask of csrc/dropout.h; ndcn_amd/dropout.py numbers the evaluations
            triple = _dropout.next_evaluation(self.dropout)
            if _needs_grad(x, self.wt):
                from .autograd_ops import rhs
                return rhs(self.A, x, self.wt.weight, self.wt.bias, self.no_graph, self.no_control, dropout=triple)
            return hip.rhs(self.A, x, self.wt.weight, self.wt.bias, no_graph=self.no_graph, no_control=self.no_control, dropout=triple)
        if self.dropout > 0 and self.training:
            # p >= 1: un-fused sequence, dropout between Linear and relu as neural_dynamics.py:34
            from .autograd_ops import spmm, linear
            if not self.no_graph:
                x = spmm(self.A, x)
            if not self.no_control:
                x = linear(x, self.wt.weight, self.wt.bias)
            x = self.dropout_layer(x)
            return torch.relu(x)
        if _needs_grad(x, self.wt):
            from .autograd_ops import rhs
            return rhs(self.A, x, self.wt.weight, self.wt.bias, self.no_graph, self.no_control)
        return hip.rhs(self.A, x, self.wt.weight, self.wt.bias, no_graph=self.no_graph, no_control=self.no_control)


class _OdeBlock(nn.Module):
    """What the reference's two block classes share (neural_dynamics.py:42-119): a right-hand side module held as
    `.odefunc` (the state_dict prefix `odefunc.`), the solver settings as plain attributes, and one solve per forward -
    `odeint_adjoint` when `adjoint` is set, the whole trajectory or its last tick."""

    def _configure(self, odefunc, rtol, atol, method, adjoint, terminal):
        self.odefunc = odefunc
        self.rtol, self.atol, self.method = rtol, atol, method
        self.adjoint, self.terminal = adjoint, terminal

    def _solve(self, x, vt, readout=None):
        """readout=(weight, bias): the decoder applied to every tick inside the solve (odeint's keyword; non-adjoint blocks)"""
        if readout is not None:
            assert not self.adjoint, 'readout: odeint_adjoint has no such keyword'
            out = ode.odeint(self.odefunc, x, vt.type_as(x), rtol=self.rtol, atol=self.atol, method=self.method, readout=readout)
            return out[-1] if self.terminal else out
        solve = ode.odeint_adjoint if self.adjoint else ode.odeint
        out = solve(self.odefunc, x, vt.type_as(x), rtol=self.rtol, atol=self.atol, method=self.method)
        return out[-1] if self.terminal else out


class ODEBlock(_OdeBlock):
    """forward(vt, x): the time vector arrives with every call (neural_dynamics.py:42-79; NDCN's block)."""

    def __init__(self, odefunc, rtol=.01, atol=.001, method='dopri5', adjoint=False, terminal=False):
        super().__init__()
        self._configure(odefunc, rtol, atol, method, adjoint, terminal)

    def forward(self, vt, x):
        return self._solve(x, vt)


class ODEBlock2(_OdeBlock):
    """forward(x): the time vector is fixed at construction as `.integration_time_vector` - a plain attribute, not a
    buffer, so `.to(device)` leaves it where the caller put it (neural_dynamics.py:82-119; dgnn.py's Sequential)."""

    def __init__(self, odefunc, vt, rtol=.01, atol=.001, method='dopri5', adjoint=False, terminal=False):
        super().__init__()
        self._configure(odefunc, rtol, atol, method, adjoint, terminal)
        self.integration_time_vector = vt

    def forward(self, x):
        return self._solve(x, self.integration_time_vector)


class _HipLinear(nn.Linear):
    """nn.Linear whose forward is the MFMA kernel (same parameters / state_dict keys)."""

    def forward(self, x):
        if _needs_grad(x, self):
            from .autograd_ops import linear
            return linear(x, self.weight, self.bias)
        return hip.linear(x, self.weight, self.bias)


class NDCN(nn.Module):
    """encoder -> graph ODE -> decoder   -- reference neural_dynamics.py:122-160.  Submodule names (and with them the
    state_dict keys input_layer.{0,2}.*, neural_dynamic_layer.odefunc.wt.*, output_layer.*) and the constructor's
    arguments, kept as attributes, are the contract; the three Linears run on the MFMA kernel."""

    def __init__(self, input_size, hidden_size, A, num_classes, dropout=0.0,
                 no_embed=False, no_graph=False, no_control=False,
                 rtol=.01, atol=.001, method='dopri5'):
        super().__init__()
        for name, value in (('input_size', input_size), ('hidden_size', hidden_size), ('A', A), ('num_classes', num_classes),
                            ('dropout', dropout), ('no_embed', no_embed), ('no_graph', no_graph), ('no_control', no_control),
                            ('rtol', rtol), ('atol', atol), ('method', method)):
            setattr(self, name, value)
        self.dropout_layer = nn.Dropout(dropout)
        # construction order = parameter order = the order nn.Linear draws its initial weights in (seeded parity)
        self.input_layer = nn.Sequential(_HipLinear(input_size, hidden_size), nn.Tanh(), _HipLinear(hidden_size, hidden_size))
        func = ODEFunc(hidden_size, A, dropout=dropout, no_graph=no_graph, no_control=no_control)
        self.neural_dynamic_layer = ODEBlock(func, rtol=rtol, atol=atol, method=method)
        self.output_layer = _HipLinear(hidden_size, num_classes)

    def forward(self, vt, x):
        h = x if self.no_embed else self.input_layer(x)
        block, dec = self.neural_dynamic_layer, self.output_layer
        # the decoder rides inside the solve (odeint's `readout`: the same bits as the two steps below): in inference the (T, N, H)
        # trajectory is never stored, in training its (T, N, H) gradient is not (the fixed-grid reverse sweep takes the decoded
        # ticks' gradient; odeint decodes in a step of its own wherever the solve does not take the decoder).  Anything that could
        # observe the hidden trajectory keeps the two-step form: a replaced or hooked decoder, hooks on the block, an adjoint block.
        if type(dec) is _HipLinear and type(block) is ODEBlock and not block.adjoint and \
                not _has_hooks(dec) and not _has_hooks(block):
            return block._solve(h, vt, readout=(dec.weight, dec.bias))
        return dec(block(vt, h))


class GraphConvolution(nn.Module):
    """A (x W^T + b) flattened to 1 x (N*out)   -- reference neural_dynamics.py:163-176 (dense-A variant
    that dgnn.py's star-import exposes)."""

    def __init__(self, input_size, output_size, bias=True):
        super(GraphConvolution, self).__init__()
        self.fc = _HipLinear(input_size, output_size, bias=bias)

    def forward(self, input, propagation_adj):
        support = self.fc(input)
        if _needs_grad(support):
            from .autograd_ops import spmm
            output = spmm(propagation_adj, support)
        else:
            output = hip.spmm(propagation_adj, support)
        return output.view(1, -1)


class TemporalGCN(nn.Module):
    """The LSTM-GNN / GRU-GNN / RNN-GNN baselines   -- reference neural_dynamics.py:179-238: per tick a GraphConvolution on an N x 1
    column, flattened to 1 x (N Hg), an LSTMCell / GRUCell / RNNCell and a Linear(Hr, N) decoder; `future` further ticks feed the
    last output back.  forward(input (N, T), future=0) -> (N, T + future).  The cell is a parameter holder in the fused form.

    Composed form: the reference's loop over the existing pieces - any shapes, any dropout, gradients by autograd.
    Fused form (csrc/tgcn.hip), taken when every condition of `_fusable` holds and NDCN_TGCN_FUSED / hip.set_tgcn_fused is on: the
    input projections of all teacher-forced ticks as ONE product that streams the (G Hr) x (N Hg) input weight once (not once per
    tick), the recurrence in one launch, the decoder as one Linear on the (T, Hr) hidden states; under a gradient one autograd node
    (autograd_ops.tgcn_sequence) plus the decoder's.  The future ticks, inference only, run one tick at a time from the same calls.
    `last_route` ('fused' / 'composed') and `route_counts` say what the last forward took."""

    def __init__(self, input_size_gnn, hidden_size_gnn, input_n_graph, hidden_size_rnn, A, dropout=0.5, rnn_type='lstm'):
        super(TemporalGCN, self).__init__()
        self.input_size_gnn = input_size_gnn
        self.hidden_size_gnn = hidden_size_gnn
        self.input_size_rnn = input_n_graph * hidden_size_gnn
        self.hidden_size_rnn = hidden_size_rnn
        self.output_size = input_n_graph
        self.dropout = dropout
        self.dropout_layer = nn.Dropout(dropout)
        self.A = A
        # construction order = parameter order = the order of the seeded initial draws (neural_dynamics.py:191-201)
        self.gc = GraphConvolution(input_size_gnn, hidden_size_gnn)
        self.rnn_type = rnn_type
        if rnn_type == 'lstm':
            self.rnn = nn.LSTMCell(self.input_size_rnn, hidden_size_rnn)
        elif rnn_type == 'gru':
            self.rnn = nn.GRUCell(self.input_size_rnn, hidden_size_rnn)
        elif rnn_type == 'rnn':
            self.rnn = nn.RNNCell(self.input_size_rnn, hidden_size_rnn)
        self.linear = _HipLinear(hidden_size_rnn, input_n_graph)
        self.last_route = None
        self.route_counts = {'fused': 0, 'composed': 0}

    def _fusable(self, input, future):
        if not hip.tgcn_fused_on() or self.rnn_type not in _lib.TGCN_TYPES:
            return False
        gates = _lib.TGCN_GATES[_lib.TGCN_TYPES[self.rnn_type]]
        if self.input_size_gnn != 1 or not 1 <= self.hidden_size_gnn <= 8 or gates * self.hidden_size_rnn > 64:
            return False
        if input.dim() != 2 or input.shape[1] < 1 or not input.is_cuda or input.dtype != torch.float32 or input.requires_grad:
            return False
        if any(p.dtype != torch.float32 or p.device != input.device for p in self.parameters()):
            return False
        if self.dropout > 0 and self.training:
            return False
        if type(self.gc) is not GraphConvolution or type(self.linear) is not _HipLinear or getattr(self.rnn, 'nonlinearity', 'tanh') != 'tanh':
            return False
        if any(_has_hooks(m) for m in (self.gc, self.gc.fc, self.rnn, self.linear, self.dropout_layer)):
            return False
        return future == 0 or not _needs_grad(self)

    def forward(self, input, future=0):
        route = 'fused' if self._fusable(input, future) else 'composed'
        self.last_route = route
        self.route_counts[route] += 1
        return self._forward_fused(input, future) if route == 'fused' else self._forward_composed(input, future)

    def _forward_composed(self, input, future):
        outputs = []
        h_t = torch.zeros(1, self.hidden_size_rnn, device=input.device)
        c_t = torch.zeros(1, self.hidden_size_rnn, device=input.device) if self.rnn_type == 'lstm' else None
        output = None

        def tick(input_t, h_t, c_t):
            input_t = self.dropout_layer(input_t)
            input_t = F.relu(self.gc(input_t, self.A))
            if self.rnn_type == 'lstm':
                h_t, c_t = self.rnn(input_t, (h_t, c_t))
            else:
                h_t = self.rnn(input_t, h_t)
            return self.linear(h_t).t(), h_t, c_t

        for input_t in input.chunk(input.size(1), dim=1):
            output, h_t, c_t = tick(input_t, h_t, c_t)
            outputs += [output]
        for _ in range(future):
            output, h_t, c_t = tick(output, h_t, c_t)
            outputs += [output]
        return torch.stack(outputs, 1).squeeze(2)

    def _row_sums(self, A):
        """r = A 1, once per operator: kept on the operator's converted form (csr.as_csr caches that on the tensor it came from, keyed
        on its version counter - a changed operator gets a new converted form and with it a new r)."""
        r = getattr(A, '_tgcn_row_sums', None)
        if r is None:
            r = hip.spmm(A, torch.ones(A.shape[1], dtype=torch.float32, device=A.device))
            A._tgcn_row_sums = r
        return r

    def _forward_fused(self, input, future):
        from .csr import as_csr
        A = as_csr(self.A)
        gc, rnn = self.gc.fc, self.rnn
        r = self._row_sums(A)
        S = hip.spmm(A, input.detach().contiguous())                  # (N, T): A X for all ticks in one call
        if _needs_grad(self):
            from .autograd_ops import tgcn_sequence
            H = tgcn_sequence(S, r, gc.weight, gc.bias, rnn.weight_ih, rnn.weight_hh, rnn.bias_ih, rnn.bias_hh, self.rnn_type)
            return self.linear(H).t()
        w, b = gc.weight.detach(), gc.bias.detach()
        W_ih, W_hh, b_ih, b_hh = (p.detach() for p in (rnn.weight_ih, rnn.weight_hh, rnn.bias_ih, rnn.bias_hh))
        GI = hip.tgcn_proj(S, r, w, b, W_ih, b_ih)
        H, _, _, h_t, c_t = hip.tgcn_cell(self.rnn_type, GI, W_hh, b_hh)
        Wd, bd = self.linear.weight.detach(), self.linear.bias.detach()
        out = hip.linear(H, Wd, bd).t()
        if future == 0:
            return out
        # the rollout, one tick at a time from the same calls: the input weight is read once per future tick
        cols = [out]
        x = out[:, -1].contiguous()
        for _ in range(future):
            GI = hip.tgcn_proj(hip.spmm(A, x).view(-1, 1), r, w, b, W_ih, b_ih)
            H, _, _, h_t, c_t = hip.tgcn_cell(self.rnn_type, GI, W_hh, b_hh, h0=h_t, c0=c_t)
            x = hip.linear(H, Wd, bd).view(-1)
            cols.append(x.view(-1, 1))
        return torch.cat(cols, 1)
