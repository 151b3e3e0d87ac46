"""TemporalGCN restated in float64 from its formulas (not from any implementation's code): the yardstick of tests/test_tgcn_host.py
and tests/test_gpu_tgcn.py.  Arrays in, numpy float64 out; gradients by float64 autograd over the same formulas.

    Z[i, j, tau] = S[i, tau] w[j] + r[i] b[j]                      S = A X (N x T, ticks in columns), r = A 1
    GI[tau, g]   = b_ih[g] + sum_{i,j} W_ih[g, i Hg + j] relu(Z[i, j, tau])
    lstm   (i, f, g, o) = (sig, sig, tanh, sig)(GI + W_hh h + b_hh);  c' = f c + i g;  h' = o tanh(c')
    gru    r = sig(GI_r + (W_hh h + b_hh)_r), z likewise, n = tanh(GI_n + r (W_hh h + b_hh)_n);  h' = (1 - z) n + z h
    rnn    h' = tanh(GI + W_hh h + b_hh)
    out[:, tau] = W_d h_tau + b_d;  a future tick feeds the last output column back as X.
"""
import numpy as np
import torch

GATES = {'rnn': 1, 'gru': 3, 'lstm': 4}
PARAMS = ('gc.fc.weight', 'gc.fc.bias', 'rnn.weight_ih', 'rnn.weight_hh', 'rnn.bias_ih', 'rnn.bias_hh', 'linear.weight', 'linear.bias')


def param_count(N, Hg, Hr, rnn_type):
    G = GATES[rnn_type]
    return 2 * Hg + G * Hr * (N * Hg + Hr + 2) + N * (Hr + 1)


def _t(x, grad=False):
    t = torch.tensor(np.asarray(x, dtype=np.float64), dtype=torch.float64)
    return t.requires_grad_() if grad else t


def _np(t):
    return None if t is None else t.detach().numpy().copy()


def _proj(S, r, w, b, W_ih, b_ih):
    w, b = w.reshape(-1), b.reshape(-1)
    Z = S[:, None, :] * w[None, :, None] + (r[:, None] * b[None, :])[:, :, None]       # (N, Hg, T)
    V = torch.relu(Z).reshape(-1, S.shape[1])                                          # row i Hg + j
    return (W_ih @ V).t() + b_ih[None, :], Z


def _step(rnn_type, gi, h, c, W_hh, b_hh):
    Hr = h.shape[0]
    gh = W_hh @ h + b_hh
    if rnn_type == 'lstm':
        a = gi + gh
        i, f, g, o = torch.sigmoid(a[:Hr]), torch.sigmoid(a[Hr:2 * Hr]), torch.tanh(a[2 * Hr:3 * Hr]), torch.sigmoid(a[3 * Hr:])
        c = f * c + i * g
        return o * torch.tanh(c), c
    if rnn_type == 'gru':
        r = torch.sigmoid(gi[:Hr] + gh[:Hr])
        z = torch.sigmoid(gi[Hr:2 * Hr] + gh[Hr:2 * Hr])
        n = torch.tanh(gi[2 * Hr:] + r * gh[2 * Hr:])
        return (1 - z) * n + z * h, c
    return torch.tanh(gi + gh), c


def _cell(rnn_type, GI, W_hh, b_hh, h, c):
    hs = []
    for tau in range(GI.shape[0]):
        h, c = _step(rnn_type, GI[tau], h, c, W_hh, b_hh)
        hs.append(h)
    return torch.stack(hs), h, c


def proj(S, r, w, b, W_ih, b_ih):
    return _np(_proj(*[_t(x) for x in (S, r, w, b, W_ih, b_ih)])[0])


def proj_min_abs_z(S, r, w, b):
    Z = _proj(_t(S), _t(r), _t(w), _t(b), torch.zeros(1, np.asarray(S).shape[0] * np.asarray(w).size, dtype=torch.float64),
              torch.zeros(1, dtype=torch.float64))[1]
    return float(Z.abs().min())


def proj_bwd(S, r, w, b, W_ih, GGI):
    """(g_Wih, g_w, g_b, g_bih) of sum(GI * GGI)"""
    S, r, GGI = _t(S), _t(r), _t(GGI)
    w, b, W_ih = _t(w, True), _t(b, True), _t(W_ih, True)
    b_ih = torch.zeros(W_ih.shape[0], dtype=torch.float64, requires_grad=True)
    GI, _ = _proj(S, r, w, b, W_ih, b_ih)
    g = torch.autograd.grad((GI * GGI).sum(), (W_ih, w, b, b_ih))
    return tuple(_np(x) for x in g)


def cell(rnn_type, GI, W_hh, b_hh, h0=None, c0=None):
    """(H (T, Hr), hT, cT)"""
    GI, W_hh, b_hh = _t(GI), _t(W_hh), _t(b_hh)
    Hr = W_hh.shape[1]
    h = _t(h0).reshape(-1) if h0 is not None else torch.zeros(Hr, dtype=torch.float64)
    c = _t(c0).reshape(-1) if c0 is not None else torch.zeros(Hr, dtype=torch.float64)
    H, h, c = _cell(rnn_type, GI, W_hh, b_hh, h, c)
    return _np(H), _np(h), _np(c)


def cell_bwd(rnn_type, GI, W_hh, b_hh, gH, h0=None, c0=None):
    """(GGI, g_Whh, g_bhh, g_h0, g_c0) of sum(H * gH)"""
    GI, W_hh, b_hh = _t(GI, True), _t(W_hh, True), _t(b_hh, True)
    Hr = W_hh.shape[1]
    h = _t(np.zeros(Hr) if h0 is None else np.asarray(h0).reshape(-1), True)
    c = _t(np.zeros(Hr) if c0 is None else np.asarray(c0).reshape(-1), True)
    H, _, _ = _cell(rnn_type, GI, W_hh, b_hh, h, c)
    g = torch.autograd.grad((H * _t(gH)).sum(), (GI, W_hh, b_hh, h, c), allow_unused=True)
    return tuple(_np(x) if x is not None else np.zeros(Hr) for x in g)


def _model(rnn_type, A, X, P, future):
    r = A.sum(1)
    Hr = P['rnn.weight_hh'].shape[1]
    h = torch.zeros(Hr, dtype=torch.float64)
    c = torch.zeros(Hr, dtype=torch.float64)
    cols = []
    x = None
    for tau in range(X.shape[1] + future):
        x = X[:, tau] if tau < X.shape[1] else x
        GI, _ = _proj((A @ x)[:, None], r, P['gc.fc.weight'], P['gc.fc.bias'], P['rnn.weight_ih'], P['rnn.bias_ih'])
        h, c = _step(rnn_type, GI[0], h, c, P['rnn.weight_hh'], P['rnn.bias_hh'])
        x = P['linear.weight'] @ h + P['linear.bias']
        cols.append(x)
    return torch.stack(cols, 1)


def forward(rnn_type, A, X, params, future=0):
    """out (N, T + future); params: a mapping with the state_dict names"""
    P = {k: _t(params[k]) for k in PARAMS}
    return _np(_model(rnn_type, _t(A), _t(X), P, future))


def loss_and_grads(rnn_type, A, X, params, target):
    """(mean |out - target|, {name: gradient}) for future = 0"""
    P = {k: _t(params[k], True) for k in PARAMS}
    out = _model(rnn_type, _t(A), _t(X), P, 0)
    loss = (out - _t(target)).abs().mean()
    grads = torch.autograd.grad(loss, [P[k] for k in PARAMS])
    return float(loss.detach()), {k: _np(g) for k, g in zip(PARAMS, grads)}
