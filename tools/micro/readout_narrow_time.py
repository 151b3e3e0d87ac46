"""Timing aid: the fused dense-output readout at the narrow widths (csrc/rk.hip readout_narrow_kernel, 16 <= H <= 60) against the
pair of launches it replaces, in ONE process, the two alternating round by round.

launch  a dopri5 solve on the 316 x 316 lattice (99 856 rows, C = 1) whose 8 ticks all fall inside ONE accepted step: through
        ndcn_solver_advance_many_readout that step's ticks are one launch of the fused kernel; through ndcn_solver_advance_many they
        are one interp_direct_multi launch that writes 8 hidden panels, which one ndcn_linear_f32 call then decodes.  The times are
        the library's own HIP-event brackets around exactly those launches (ndcn_prof_*: kinds interp_eval and linear).
solve   NDCN(1, 20) inference, dopri5, the same lattice, 100 ticks over [0, 5]: NDCN.forward (the decoder inside the solve) against
        the two-step form output_layer(neural_dynamic_layer(...)) - what NDCN.forward ran at this width before the narrow kernel
        existed; wall time by HIP events and torch's peak allocation beyond what was allocated before the call.

Prints one JSON line per measurement (median, min and max over the rounds) and, with --out FILE, writes them there too.

    python tools/micro/readout_narrow_time.py [--rounds 9] [--out profiles/NAME.jsonl] [--quick]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch

from ndcn_amd import _lib, graphs, hip
from ndcn_amd.neural_dynamics import NDCN, ODEFunc
from ndcn_amd.torchdiffeq._impl.odeint import DeviceSolver

FUSED, NARROW = _lib.READOUT_FUSED, _lib.READOUT_NARROW


def prof(fn):
    """{kind: (launches, ms)} of the library launches fn() makes"""
    lib = _lib.load()
    nk = lib.ndcn_prof_kinds()
    buf = (_lib.ctypes.c_double * (4 * nk))()
    lib.ndcn_prof_enable(1)
    lib.ndcn_prof_read(buf, nk)
    fn()
    torch.cuda.synchronize()
    lib.ndcn_prof_enable(0)
    lib.ndcn_prof_read(buf, nk)
    return {k: (int(buf[4 * i]), buf[4 * i + 1]) for i, k in enumerate(_lib.PROF_KINDS) if buf[4 * i]}


def emit(row, sink):
    line = json.dumps(row)
    print(line, flush=True)
    if sink:
        sink.write(line + '\n')
        sink.flush()


def med(v):
    return {'median': round(statistics.median(v), 5), 'min': round(min(v), 5), 'max': round(max(v), 5)}


def launch_case(A, n, H, dev, rounds, sink, graph):
    torch.manual_seed(0)
    f = ODEFunc(H, A).to(dev).eval()
    x0 = torch.rand(n, H, generator=torch.Generator().manual_seed(1)).to(dev)
    g = torch.Generator().manual_seed(5)
    Wd = ((torch.rand(1, H, generator=g) - .5) * (2. / H ** .5)).to(dev)
    bd = (torch.rand(1, generator=g) - .5).to(dev)
    s = DeviceSolver(f, n, 'dopri5', rtol=.01, atol=.001)
    try:
        hidden = torch.empty((8, n, H), device=dev)
        out = torch.empty((8, n, 1), device=dev)
        scratch = torch.empty((2, n, H), device=dev)
        s.begin(x0, 0.)
        s.advance_many([5.], hidden[:1])
        steps = [r for r in s.steplog() if len(r) == 5 and r[2]]
        t0, dt = steps[min(2, len(steps) - 1)][:2]                         # an accepted step past the start-up
        ticks = [t0 + dt * (i + 1) / 9. for i in range(8)]

        def fused():
            s.begin(x0, 0.)
            assert s.advance_many_readout(ticks, Wd, bd, out, scratch)

        def staged():
            s.begin(x0, 0.)
            s.advance_many(ticks, hidden)

        res = {'fused': [], 'direct_multi': [], 'linear': []}
        for r in range(rounds + 2):                                        # two warm-up rounds
            p = prof(fused)
            bits = int(_lib.load().ndcn_last_readout_path())
            assert p['interp_eval'][0] == 1 and bits == FUSED | NARROW, (p, bits)
            q = prof(staged)
            assert q['interp_eval'][0] == 1, q
            lin = prof(lambda: hip.linear(hidden, Wd, bd))
            assert lin['linear'][0] == 1 and len(lin) == 1, lin
            if r >= 2:
                res['fused'].append(p['interp_eval'][1])
                res['direct_multi'].append(q['interp_eval'][1])
                res['linear'].append(lin['linear'][1])
        assert torch.equal(out, hip.linear(hidden, Wd, bd))
    finally:
        s.close()
    pair = [a + b for a, b in zip(res['direct_multi'], res['linear'])]
    emit({'what': 'launch', 'graph': graph, 'n': n, 'H': H, 'C': 1, 'ticks': 8, 'rounds': rounds,
          'fused_ms': med(res['fused']), 'direct_multi_ms': med(res['direct_multi']), 'linear_ms': med(res['linear']),
          'pair_ms': med(pair), 'fused_over_pair': round(statistics.median(res['fused']) / statistics.median(pair), 4)}, sink)


def solve_case(A, n, H, T, dev, rounds, sink, graph):
    torch.manual_seed(0)
    m = NDCN(input_size=1, hidden_size=H, A=A, num_classes=1, rtol=.01, atol=.001, method='dopri5').to(dev).eval()
    x = torch.rand(n, 1, generator=torch.Generator().manual_seed(1)).to(dev)
    vt = torch.linspace(0., 5., T).to(dev)
    forms = {'decoder_in_solve': lambda: m(vt, x),
             'two_step': lambda: m.output_layer(m.neural_dynamic_layer(vt, m.input_layer(x)))}
    res = {k: {'ms': [], 'peak_mb': []} for k in forms}
    bits = {}
    with torch.no_grad():
        for r in range(rounds + 2):
            for name, fn in forms.items():
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats(dev)
                base = torch.cuda.memory_allocated(dev)
                _lib.load().ndcn_clear_readout_path()
                a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                y = fn()
                e.record()
                torch.cuda.synchronize()
                bits[name] = int(_lib.load().ndcn_last_readout_path())
                if r >= 2:
                    res[name]['ms'].append(a.elapsed_time(e))
                    res[name]['peak_mb'].append((torch.cuda.max_memory_allocated(dev) - base) / 2 ** 20)
                del y
    panel_mb = n * H * 4 / 2 ** 20
    for name in forms:
        emit({'what': 'solve', 'form': name, 'graph': graph, 'n': n, 'H': H, 'ticks': T, 'rounds': rounds, 'readout_path': bits[name],
              'panel_mb': round(panel_mb, 3), 'ms': med(res[name]['ms']), 'peak_mb': med(res[name]['peak_mb']),
              'peak_panels': round(statistics.median(res[name]['peak_mb']) / panel_mb, 2)}, sink)


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--rounds', type=int, default=9)
    p.add_argument('--out', default=None)
    p.add_argument('--quick', action='store_true', help='a 64 x 64 lattice and one width: a rehearsal of every code path')
    a = p.parse_args()
    assert torch.cuda.is_available(), 'a timing needs the device'
    dev = torch.device('cuda:0')
    if a.out and os.path.dirname(a.out):
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
    sink = open(a.out, 'w') if a.out else None
    side = 64 if a.quick else 316
    graph = 'lattice %d x %d' % (side, side)
    A = graphs.to_device(graphs.normalized_laplacian(graphs.grid_8_neighbor(side)), dev)
    for H in ((20,) if a.quick else (16, 20, 32, 60)):
        launch_case(A, side * side, H, dev, a.rounds, sink, graph)
    solve_case(A, side * side, 20, 100, dev, a.rounds, sink, graph)
    if sink:
        sink.close()


if __name__ == '__main__':
    main()
