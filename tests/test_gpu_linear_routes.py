"""Every dispatch route of the dense Linear (linear.hip: ndcn_linear_f32; linear_bwd.hip: ndcn_linear_bwd_f32) against an fp64 product of
the same fp32 inputs, at the shapes and row counts where a route changes or a kernel's loop ends, each route asserted through
ndcn_debug_last_linear_path.

Bounds are per element, in terms of the element's own sum of magnitudes sum_k |a_k b_k| (u = 2^-24):
  fp32 MFMA / fma-chain routes           (K + 2) u sum |a b|  (+ |b| for the bias)
  gS, two fp16 pieces (split16.h)        2e-6 sum_o |gZ_o| |W_oi|                   (split16.h: GUARANTEE)
  gW, three bf16 pieces                  1.01 (2^-23 + u (6 rows_per_chunk + chunks)) sum_r |gZ_ro| |S_ri|   (linear_bwd.hip: BOUND)
  gW, fp32 routes                        1.01 u (rows_per_chunk + chunks) sum_r |gZ_ro| |S_ri|
  gb                                     1.01 u (rows_per_chunk + chunks + 1) sum_r |gZ_ro|
The ReLU mask is torch's threshold_backward: g is zeroed where Y <= 0 and passed elsewhere, a NaN Y included.
Switches read once per process (NDCN_GS_ROWS, NDCN_GS_SPLIT, NDCN_GW_SPLIT) run in fresh child processes."""
import hashlib
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return torch.device('cuda:0')


def _lib():
    from ndcn_amd import _lib
    return _lib


def _path():
    return _lib().load().ndcn_debug_last_linear_path()


def _chunks(n, small=False):
    """linear_bwd.hip wgrad_chunks + the launcher's rounding: (rows per chunk, chunks used, rows of the last chunk)"""
    c = (n + 15) // 16 if n <= 4096 else (n + 63) // 64
    c = max(1, min(c, 4096 if small else 256))
    rpc = -(-(-(-n // c)) // 8) * 8
    used = -(-n // rpc)
    return rpc, used, n - (used - 1) * rpc


# ------------------------------------------------------------------------------------------------------------------------ inputs
def _rows_scaled(n, H, gen, dev, k=12, zero_every=13):
    """randn rows, each multiplied by 2^j (j uniform in [-k, k]); every zero_every-th row all zero"""
    x = torch.randn(n, H, generator=gen, device=dev)
    j = torch.randint(-k, k + 1, (n, 1), generator=gen, device=dev).float()
    x = x * torch.exp2(j)
    if zero_every:
        x[::zero_every] = 0.0
    return x


SPECIALS = (0.0, -0.0, 1e-40, 1e-37, float('nan'))      # +0, -0, subnormal, tiny positive, NaN


def _relu_out(n, Ho, gen, dev, specials=SPECIALS):
    """a ReLU output with the special values threaded through it: row r holds specials[r % 5] in column (7 r) % Ho"""
    Y = torch.relu(torch.randn(n, Ho, generator=gen, device=dev))
    r = torch.arange(n, device=dev)
    vals = torch.tensor(specials, dtype=torch.float32, device=dev)
    Y[r, (7 * r) % Ho] = vals[r % len(specials)]
    return Y


def _bwd_inputs(n, Hi, Ho, seed, dev, specials=SPECIALS):
    gen = torch.Generator(device=dev).manual_seed(seed)
    g = _rows_scaled(n, Ho, gen, dev, zero_every=11)
    g[torch.rand(n, Ho, generator=gen, device=dev) < 0.1] = 0.0         # exact zeros of g
    S = _rows_scaled(n, Hi, gen, dev, zero_every=17)
    W = torch.randn(Ho, Hi, generator=gen, device=dev) / 16
    Y = _relu_out(n, Ho, gen, dev, specials)
    return g, S, W, Y


def _gz(g, Y):
    """threshold_backward(g, Y, 0): 0 where Y <= 0, g elsewhere (NaN passes) - on the CPU, where a subnormal compares as itself"""
    if Y is None:
        return g.double()
    m = (Y.cpu() <= 0).to(g.device)
    return torch.where(m, torch.zeros_like(g), g).double()


# ------------------------------------------------------------------------------------------------------------------------ checks
def _within(got, ref, bound, what):
    err = (got.double() - ref).abs()
    bad = ~(err <= bound)
    if bool(bad.any()):
        i = int(torch.nonzero(bad.flatten())[0])
        pytest.fail('%s: %d elements out of bound; first flat %d: got %r ref %r bound %r' % (
            what, int(bad.sum()), i, float(got.flatten()[i]), float(ref.flatten()[i]), float(bound.flatten()[i])))


def _check_bwd(g, S, W, Y, gS, gW, gb, route):
    """each output against fp64 and its route's bound"""
    n, Ho = g.shape
    Hi = W.shape[1]
    gz = _gz(g, Y)
    Wd = W.double()
    if gS is not None:
        ref, mag = gz @ Wd, gz.abs() @ Wd.abs()
        if route & (_lib().LIN_GS_RES | _lib().LIN_GS_RES_MASK | _lib().LIN_GS_SPLIT32 | _lib().LIN_GS_SPLIT64):
            _within(gS, ref, 2e-6 * mag, 'gS split')
        else:
            _within(gS, ref, (Ho + 2) * U * mag, 'gS fp32')
    rpc, used, _ = _chunks(n, Hi < 16 or Ho < 16)
    rows = min(rpc, n)
    if gW is not None:
        Sd = S.double()
        ref, mag = gz.t() @ Sd, gz.abs().t() @ Sd.abs()
        if route & _lib().LIN_GW_SPLIT:
            _within(gW, ref, 1.01 * (2.0 ** -23 + U * (6 * rows + used)) * mag, 'gW split')
        else:
            _within(gW, ref, 1.01 * U * (rows + used) * mag, 'gW fp32')
    if gb is not None:
        _within(gb, gz.sum(0), 1.01 * U * (rows + used + 1) * gz.abs().sum(0), 'gb')


def _bwd(g, W, S, Y, need=(True, True, True)):
    from ndcn_amd import hip
    out = hip.linear_bwd(g, W, S=S, Y=Y, need_gS=need[0], need_gW=need[1], need_gb=need[2])
    return out, _path()


def _expect_bwd(route, Hi, Ho, n, masked, need, aligned=True, gs_split=True, gw_split=True):
    L = _lib()
    want = 0
    small = Hi < 16 or Ho < 16
    if need[0]:
        if small:
            want |= L.LIN_GS_SMALL
        elif Hi == 256 and Ho == 256 and aligned and gs_split:
            want |= (L.LIN_GS_RES_MASK if masked else L.LIN_GS_RES) if n * 1024 < 2 ** 32 else L.LIN_GS_SPLIT64
        else:
            want |= L.LIN_GS_FP32
    if need[1] or need[2]:
        want |= L.LIN_GW_SMALL if small else (L.LIN_GW_SPLIT if Hi == 256 and Ho == 256 and gw_split else L.LIN_GW_FP32)
        if need[1] and need[2]:
            want |= L.LIN_GW_SUM2
    assert route == want, (hex(route), hex(want))


# ------------------------------------------------------------------------------------------------------------------------ forward
def _check_fwd(S, W, b, relu, dev):
    from ndcn_amd import hip
    Y = hip.linear(S, W, b, relu=relu)
    route = _path()
    Sd, Wd = S.double(), W.double()
    ref = Sd @ Wd.t() + (b.double() if b is not None else 0.0)
    mag = Sd.abs() @ Wd.abs().t() + (b.double().abs() if b is not None else 0.0)
    if relu:
        ref = torch.relu(ref)
    _within(Y, ref, (S.shape[1] + 2) * U * mag, 'forward')
    assert torch.equal(Y, hip.linear(S, W, b, relu=relu)) and _path() == route
    return route


def _fwd_inputs(n, Hi, Ho, seed, dev):
    gen = torch.Generator(device=dev).manual_seed(seed)
    S = _rows_scaled(n, Hi, gen, dev, k=8, zero_every=9)
    W = torch.randn(Ho, Hi, generator=gen, device=dev) / Hi ** 0.5
    b = torch.randn(Ho, generator=gen, device=dev)
    return S, W, b


@pytest.mark.parametrize('Hi', [64, 65, 100, 128, 192, 256, 257, 320, 448, 512])
@pytest.mark.parametrize('Ho', [1, 2, 7, 15])
def test_forward_rowdot(dev, Hi, Ho):
    """linear_rowdot_kernel<NV> for NV = 1..8, Hi off a multiple of 64 (masked lanes)"""
    S, W, b = _fwd_inputs(1237, Hi, Ho, Hi * 31 + Ho, dev)
    for relu in (False, True):
        assert _check_fwd(S, W, b if relu else None, relu, dev) == _lib().LIN_ROWDOT


@pytest.mark.parametrize('Hi,Ho', [(1, 20), (7, 256), (15, 16), (20, 1), (40, 15), (63, 3), (513, 2), (600, 15), (1, 1)])
def test_forward_small(dev, Hi, Ho):
    S, W, b = _fwd_inputs(901, Hi, Ho, Hi * 7 + Ho, dev)
    for relu in (False, True):
        assert _check_fwd(S, W, b, relu, dev) == _lib().LIN_SMALL


@pytest.mark.parametrize('Ho', [16, 64, 65, 128, 129, 256, 257, 300])
@pytest.mark.parametrize('Hi', [16, 37, 256])
def test_forward_mfma(dev, Hi, Ho):
    """fp32 MFMA tile kernel: BN = 64 / 128 / 256, grid.y > 1 past 256 output features, float4 staging or (Hi % 4 != 0) scalar"""
    L = _lib()
    S, W, b = _fwd_inputs(333, Hi, Ho, Hi + 1000 * Ho, dev)
    bn = L.LIN_MFMA256 if Ho > 128 else L.LIN_MFMA128 if Ho > 64 else L.LIN_MFMA64
    for relu in (False, True):
        assert _check_fwd(S, W, b, relu, dev) == bn | (L.LIN_VEC if Hi % 4 == 0 else 0)


@pytest.mark.parametrize('Hi,Ho', [(256, 256), (64, 100), (128, 300)])
def test_forward_mfma_misaligned_views(dev, Hi, Ho):
    """Hi % 4 == 0 but S and W one float off 16-byte alignment: the scalar staging path, same bound"""
    L = _lib()
    S0, W0, b = _fwd_inputs(129, Hi, Ho, Hi + Ho, dev)
    S = torch.empty(S0.numel() + 1, device=dev)[1:].view(S0.shape)
    W = torch.empty(W0.numel() + 1, device=dev)[1:].view(W0.shape)
    S.copy_(S0)
    W.copy_(W0)
    assert S.data_ptr() % 16 == 4 and W.data_ptr() % 16 == 4
    bn = L.LIN_MFMA256 if Ho > 128 else L.LIN_MFMA128 if Ho > 64 else L.LIN_MFMA64
    for relu in (False, True):
        assert _check_fwd(S, W, b, relu, dev) == bn
    from ndcn_amd import hip
    assert torch.equal(hip.linear(S, W, b), hip.linear(S0, W0, b))       # fp32 MFMA chain either way: same bits


# ------------------------------------------------------------------------------------------------------------------------ backward
TILE_EDGES = sorted({32 * t - d for t in (255, 256, 257, 511, 512, 513, 767, 769) for d in (0, 5)})
SMALL_N = [1, 7, 31, 32, 33, 63, 64, 65]
CHUNK_EDGES = [4095, 4096, 4097, 16383, 16384, 16385]
N_256 = SMALL_N + TILE_EDGES + CHUNK_EDGES


def test_size_lists_reach_the_edges():
    """the row counts above end the res kernel's rounds exactly / with one tile over, and reach a last wgrad chunk of < 16 rows"""
    assert any(_chunks(n)[2] < 16 for n in N_256 if n > 4096) and any(_chunks(n)[2] < 16 for n in SMALL_N if n > 16)
    tiles = {(n + 31) // 32 for n in N_256}
    assert {255, 256, 257, 511, 512, 513, 767, 769} <= tiles


@pytest.mark.parametrize('masked', [True, False])
@pytest.mark.parametrize('n', N_256)
def test_backward_256_sizes(dev, n, masked):
    """H = 256: resident-weight gS (both mask forms) and the bf16-piece gW / gb, against fp64 per element; repeat calls bit-identical"""
    g, S, W, Y = _bwd_inputs(n, 256, 256, n * 2 + masked, dev)
    Y = Y if masked else None
    (gS, gW, gb), route = _bwd(g, W, S, Y)
    _expect_bwd(route, 256, 256, n, masked, (True, True, True))
    _check_bwd(g, S, W, Y, gS, gW, gb, route)
    (gS2, gW2, gb2), route2 = _bwd(g, W, S, Y)
    assert route2 == route and torch.equal(gS, gS2) and torch.equal(gW, gW2) and torch.equal(gb, gb2)


@pytest.mark.parametrize('need', [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)])
@pytest.mark.parametrize('Hi,Ho,n', [(256, 256, 4097), (300, 40, 1001), (20, 1, 777)])
def test_backward_output_subsets(dev, Hi, Ho, n, need):
    """every subset of (gS, gW, gb): each output equals, bit for bit, the one of the call that forms all three (chunk_sum / chunk_sum2)"""
    need = tuple(bool(v) for v in need)
    g, S, W, Y = _bwd_inputs(n, Hi, Ho, n + Hi, dev)
    full, _ = _bwd(g, W, S, Y)
    part, route = _bwd(g, W, S, Y, need)
    _expect_bwd(route, Hi, Ho, n, True, need)
    for want, a, b in zip(need, part, full):
        assert (a is None) != want and (a is None or torch.equal(a, b))


@pytest.mark.parametrize('Hi,Ho', [(300, 40), (40, 300), (513, 257), (257, 513), (256, 255), (64, 16), (16, 64),
                                   (1, 20), (20, 1), (256, 7), (7, 256)])
@pytest.mark.parametrize('n', [1, 33, 4097])
def test_backward_generic_shapes(dev, Hi, Ho, n):
    """fp32 gS (linear_gs_kernel<BN>, grid.y > 1 for Hi > 256) and gW (linear_wgrad_kernel<NI>, grid.y / grid.z > 1 past 256), and the
    narrow-shape kernels"""
    for masked in (True, False):
        g, S, W, Y = _bwd_inputs(n, Hi, Ho, n * 3 + Hi + masked, dev)
        Y = Y if masked else None
        (gS, gW, gb), route = _bwd(g, W, S, Y)
        _expect_bwd(route, Hi, Ho, n, masked, (True, True, True))
        _check_bwd(g, S, W, Y, gS, gW, gb, route)
        (gS2, gW2, gb2), _ = _bwd(g, W, S, Y)
        assert torch.equal(gS, gS2) and torch.equal(gW, gW2) and torch.equal(gb, gb2)


@pytest.mark.parametrize('n', [33, 4097])
def test_backward_256_misaligned_panels(dev, n):
    """H = 256 with panels one float off 16-byte alignment: gS leaves the split product for the fp32 MFMA GEMM and meets its bound"""
    g0, S0, W, Y0 = _bwd_inputs(n, 256, 256, n + 5, dev)
    flat = lambda x: torch.empty(x.numel() + 1, device=dev)[1:].view(x.shape).copy_(x)
    g, S, Y = flat(g0), flat(S0), flat(Y0)
    (gS, gW, gb), route = _bwd(g, W, S, Y)
    _expect_bwd(route, 256, 256, n, True, (True, True, True), aligned=False)
    _check_bwd(g, S, W, Y, gS, gW, gb, route)
    (_, gW0, gb0), _ = _bwd(g0, W, S0, Y0)
    assert torch.equal(gW, gW0) and torch.equal(gb, gb0)


@pytest.mark.parametrize('Hi,Ho', [(256, 256), (300, 40), (20, 1)])
def test_relu_mask_is_threshold_backward(dev, Hi, Ho):
    """Y = +0, -0 stop the gradient; a subnormal, a tiny positive value and NaN pass it (torch's threshold_backward) - on every mask
    site: gS, gW, gb and ndcn_relu_bwd_f32; the reference's own autograd agrees"""
    from ndcn_amd import hip
    n = 65
    gen = torch.Generator(device=dev).manual_seed(Hi)
    g = torch.randn(n, Ho, generator=gen, device=dev)
    S = torch.randn(n, Hi, generator=gen, device=dev)
    W = torch.randn(Ho, Hi, generator=gen, device=dev) / 16
    Y = torch.empty(n, Ho, device=dev)
    Y.view(-1).copy_(torch.tensor(SPECIALS * (n * Ho // 5 + 1), device=dev)[:n * Ho])
    z = torch.tensor(SPECIALS, requires_grad=True)
    torch.relu(z).backward(torch.ones(5))                   # reference semantics on the CPU: grad 0 at +0 and -0, 1 elsewhere
    assert z.grad.tolist() == [0.0, 0.0, 1.0, 1.0, 1.0]
    (gS, gW, gb), route = _bwd(g, W, S, Y)
    _check_bwd(g, S, W, Y, gS, gW, gb, route)
    gz = _gz(g, Y).float()
    assert int((gz != 0).sum()) > n * Ho // 2
    assert torch.equal(hip.relu_bwd(g, Y), gz)
    (rS, rW, rb), _ = _bwd(gz.contiguous(), W, S, None)
    assert torch.equal(gW, rW) and torch.equal(gb, rb)
    if Hi == 256:
        assert torch.equal(gS, rS)                          # the res kernel's two mask forms: same pieces, same bits


# ------------------------------------------------------------------------------------------------------------------------ child processes
def _digest(t):
    return None if t is None else hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()


def _run_cases(cases, dev, check):
    """[{'n', 'masked', 'seed'}] at H = 256 -> [{'route', 'gS', 'gW', 'gb'}] (sha256 of the bits); check: each against fp64 too"""
    out = []
    for c in cases:
        g, S, W, Y = _bwd_inputs(c['n'], 256, 256, c['seed'], dev)
        Y = Y if c['masked'] else None
        (gS, gW, gb), route = _bwd(g, W, S, Y)
        if check:
            _check_bwd(g, S, W, Y, gS, gW, gb, route)
        out.append({'route': route, 'gS': _digest(gS), 'gW': _digest(gW), 'gb': _digest(gb)})
        del g, S, W, Y, gS, gW, gb
    return out


def child_main(spec):
    sys.path.insert(0, os.path.dirname(HERE))
    torch.cuda.set_device(0)
    print('RESULT ' + json.dumps(_run_cases(spec['cases'], torch.device('cuda:0'), spec['check'])), flush=True)


def _in_child(env, cases, check):
    code = 'import sys, json; sys.path.insert(0, %r); import test_gpu_linear_routes as T; T.child_main(json.loads(sys.argv[1]))' % HERE
    e = dict(os.environ)
    for k in ('NDCN_GS_ROWS', 'NDCN_GS_SPLIT', 'NDCN_GW_SPLIT'):
        e.pop(k, None)
    e.update(env)
    p = subprocess.run([sys.executable, '-c', code, json.dumps({'cases': cases, 'check': check})], env=e, capture_output=True, text=True,
                       timeout=600, cwd=os.path.dirname(HERE))
    assert p.returncode == 0, (env, p.returncode, p.stdout[-3000:], p.stderr[-3000:])
    line = [l for l in p.stdout.splitlines() if l.startswith('RESULT ')][-1]
    return json.loads(line[len('RESULT '):])


ROUTE_N = SMALL_N + TILE_EDGES


def _route_cases():
    return [{'n': n, 'masked': m, 'seed': 7 * n + m} for n in ROUTE_N for m in (True, False)]


def test_gs_tile_kernels_equal_the_resident_kernel(dev):
    """NDCN_GS_ROWS=32 / 64 (linear_gs_256_split_kernel<1> / <2>, fresh processes) give the resident-weight kernel's bits at every size
    edge, both mask forms"""
    L = _lib()
    cases = _route_cases()
    base = _run_cases(cases, dev, check=False)
    for rows, bit in (('32', L.LIN_GS_SPLIT32), ('64', L.LIN_GS_SPLIT64)):
        got = _in_child({'NDCN_GS_ROWS': rows}, cases, check=False)
        for c, a, b in zip(cases, got, base):
            assert a['route'] & ~(L.LIN_GW_SPLIT | L.LIN_GW_SUM2) == bit, (rows, c, hex(a['route']))
            assert a['gS'] == b['gS'] and a['gW'] == b['gW'] and a['gb'] == b['gb'], (rows, c)


@pytest.mark.parametrize('env', [{'NDCN_GS_SPLIT': '0'}, {'NDCN_GW_SPLIT': '0'}])
def test_fp32_fallbacks_of_the_256_backward_meet_their_bound(dev, env):
    """NDCN_GS_SPLIT=0: gS by the fp32 MFMA GEMM; NDCN_GW_SPLIT=0: gW / gb by linear_wgrad_kernel<8> - each held to its own bound"""
    L = _lib()
    cases = [{'n': n, 'masked': m, 'seed': 5 * n + m} for n in (1, 33, 8192, 8187, 16385) for m in (True, False)]
    got = _in_child(env, cases, check=True)
    gs = L.LIN_GS_FP32 if 'NDCN_GS_SPLIT' in env else None
    for c, r in zip(cases, got):
        want_gs = gs if gs else (L.LIN_GS_RES_MASK if c['masked'] else L.LIN_GS_RES)
        want_gw = L.LIN_GW_SPLIT if gs else L.LIN_GW_FP32
        assert r['route'] == want_gs | want_gw | L.LIN_GW_SUM2, (env, c, hex(r['route']))


# ------------------------------------------------------------------------------------------------------------------------ past 2^31 / 2^32 bytes
BIG_N = [2 ** 21 + 33, 4194274, 4194303, 2 ** 22 + 17]


def _sample_rows(n):
    rows = set(range(32)) | set(range(2 ** 21 - 40, 2 ** 21 + 40)) | set(range(n - 70, n))
    return torch.tensor(sorted(r for r in rows if r < n))


def test_backward_256_beyond_2_and_4_gib(dev):
    """The res kernel with byte offsets past 2^31 (n = 2^21 + 33) and at its last sizes with a partial tail tile (n = 4194274, 4194303:
    offsets up to 2^32 - 1), the 64-row tile kernel and the wgrad kernel on panels over 4 GiB (n = 2^22 + 17).  gS on sampled rows
    against fp64 (the first tile, around 2^21, the tail), its rows 0..31 bit for bit against a 32-row call (a tail tile whose offsets
    wrapped would land there); gW / gb whole against an fp64 reduction in row chunks.  Then the tile kernel (NDCN_GS_ROWS=64, fresh
    process) on the same inputs at the tail sizes: same bits."""
    L = _lib()
    N = max(BIG_N)
    free, _ = torch.cuda.mem_get_info()
    assert free > 24 * 2 ** 30, 'needs ~24 GiB of device memory, %.1f GiB free' % (free / 2 ** 30)
    gen = torch.Generator(device=dev).manual_seed(2024)
    g = torch.randn(N, 256, generator=gen, device=dev)
    S = torch.randn(N, 256, generator=gen, device=dev)
    Y = _relu_out(N, 256, gen, dev, specials=(0.0, -0.0, 2.0 ** -120, float('nan')))
    W = torch.randn(256, 256, generator=gen, device=dev) / 16
    Wd = W.double()
    digests = {}
    for n in BIG_N:
        gn, Sn, Yn = g[:n], S[:n], Y[:n]
        for masked in (True, False):
            Ym = Yn if masked else None
            need = (True, masked, masked)
            (gS, gW, gb), route = _bwd(gn, W, Sn, Ym, need)
            _expect_bwd(route, 256, 256, n, masked, need)
            rows = _sample_rows(n).to(dev)
            gz = _gz(gn[rows], Ym[rows] if masked else None)
            _within(gS[rows], gz @ Wd, 2e-6 * (gz.abs() @ Wd.abs()), 'gS n=%d masked=%d' % (n, masked))
            (head, _, _), _ = _bwd(gn[:32].contiguous(), W, None, Ym[:32].contiguous() if masked else None, (True, False, False))
            assert torch.equal(gS[:32], head), (n, masked)
            if n in (4194274, 4194303):
                digests[(n, masked)] = _digest(gS)
            if masked:
                (gS2, gW2, gb2), _ = _bwd(gn, W, Sn, Ym, need)
                assert torch.equal(gS, gS2) and torch.equal(gW, gW2) and torch.equal(gb, gb2), n
                del gS2
                ref_w = torch.zeros(256, 256, dtype=torch.float64, device=dev)
                mag_w = torch.zeros_like(ref_w)
                ref_b = torch.zeros(256, dtype=torch.float64, device=dev)
                mag_b = torch.zeros_like(ref_b)
                for r0 in range(0, n, 1 << 19):
                    z = torch.where(Yn[r0:r0 + (1 << 19)] <= 0, 0.0, gn[r0:r0 + (1 << 19)]).double()
                    s = Sn[r0:r0 + (1 << 19)].double()
                    ref_w += z.t() @ s
                    mag_w += z.abs().t() @ s.abs()
                    ref_b += z.sum(0)
                    mag_b += z.abs().sum(0)
                    del z, s
                rpc, used, _ = _chunks(n)
                _within(gW, ref_w, 1.01 * (2.0 ** -23 + U * (6 * rpc + used)) * mag_w, 'gW n=%d' % n)
                _within(gb, ref_b, 1.01 * U * (rpc + used + 1) * mag_b, 'gb n=%d' % n)
            del gS
    del g, S, Y
    torch.cuda.empty_cache()
    # the same panels in a fresh process through the tile kernel: regenerate them with the same generator state
    code = ('import sys, json; sys.path.insert(0, %r); import test_gpu_linear_routes as T; '
            'print("RESULT " + json.dumps(T.big_tail_digests()), flush=True)' % HERE)
    e = dict(os.environ, NDCN_GS_ROWS='64')
    p = subprocess.run([sys.executable, '-c', code], env=e, capture_output=True, text=True, timeout=600, cwd=os.path.dirname(HERE))
    assert p.returncode == 0, (p.returncode, p.stdout[-3000:], p.stderr[-3000:])
    got = json.loads([l for l in p.stdout.splitlines() if l.startswith('RESULT ')][-1][len('RESULT '):])
    for (n, masked), d in digests.items():
        assert got['%d_%d' % (n, masked)] == [d, L.LIN_GS_SPLIT64], (n, masked)


def big_tail_digests():
    """(child of test_backward_256_beyond_2_and_4_gib) gS at the res kernel's tail sizes, through whatever route this process takes"""
    dev = torch.device('cuda:0')
    N = max(BIG_N)
    gen = torch.Generator(device=dev).manual_seed(2024)
    g = torch.randn(N, 256, generator=gen, device=dev)
    torch.randn(N, 256, generator=gen, device=dev)                      # S: same generator state as the parent, not needed here
    Y = _relu_out(N, 256, gen, dev, specials=(0.0, -0.0, 2.0 ** -120, float('nan')))
    W = torch.randn(256, 256, generator=gen, device=dev) / 16
    out = {}
    for n in (4194274, 4194303):
        for masked in (True, False):
            (gS, _, _), route = _bwd(g[:n], W, None, Y[:n] if masked else None, (True, False, False))
            out['%d_%d' % (n, masked)] = [_digest(gS), route]
            del gS
    return out
