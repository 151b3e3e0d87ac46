"""ISA audit of the kernels the fixed-grid `step_size` option adds to rk.hip - tick_emit_kernel and the emitting final stages
(fixed_stage_emit_kernel, ops 0 and 5) - for gfx950: no spill, no scratch; the vector forms move 16 bytes per access, the ticks
are written with non-temporal stores, and the reference's expression keeps a correctly rounded division (v_div_fixup, not a bare
reciprocal) followed by a product and a sum of their own (the bit-for-bit check is on the GPU: test_gpu_substep.py).  Cross-compiles
on the CPU."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')


@pytest.fixture(scope='module')
def asm(tmp_path_factory):
    path = str(tmp_path_factory.mktemp('isa') / 'rk.s')
    subprocess.run([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-S', '--cuda-device-only', '-o', path,
                    os.path.join(ROOT, 'ndcn_amd', 'csrc', 'rk.hip')], check=True, stderr=subprocess.DEVNULL)
    return open(path).read()


def body_of(text, symbol):
    m = re.search(r'^%s:[^\n]*\n(.*?)^\s*s_endpgm' % re.escape(symbol), text, re.S | re.M)
    assert m, symbol
    return m.group(1)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not installed')
def test_emit_kernels_have_no_spill_and_no_scratch(asm):
    blocks = re.findall(r'\.name:\s+(\S*(?:tick_emit_kernel|fixed_stage_emit_kernel)\S*)(.*?)(?=\n\s+- \.|\n\s*\.end_amdgpu_metadata)', asm, re.S)
    names = sorted(set(n for n, _ in blocks))
    # tick_emit <VEC> x 2, fixed_stage_emit <OP 0 / 5> x <VEC> x 2
    assert len(names) == 6, names
    for name, meta in blocks:
        fields = dict(re.findall(r'\.(vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size|vgpr_count):\s+(\d+)', meta))
        assert fields.get('vgpr_spill_count') == '0' and fields.get('sgpr_spill_count') == '0', (name, fields)
        assert fields.get('private_segment_fixed_size') == '0', (name, fields)
        assert int(fields.get('vgpr_count', '999')) <= 128, (name, fields)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not installed')
def test_emit_kernels_stream_and_keep_the_roundings(asm):
    symbols = re.findall(r'^(_ZN4ndcn\d+(?:tick_emit_kernel|fixed_stage_emit_kernel)\w+):', asm, re.M)
    assert len(set(symbols)) == 6, symbols
    for sym in set(symbols):
        body = body_of(asm, sym)
        assert 'v_div_fixup_f32' in body and 'v_mul_f32' in body and 'v_add_f32' in body, sym      # (y - y) / dt, * tm, y + .
        assert 'scratch_' not in body and 'buffer_store' not in body, sym
        stores = re.findall(r'global_store_dword(x4)?\b[^\n]*', body)
        assert stores, sym
        vec = 'Lb1E' in sym
        if vec:
            assert 'global_load_dwordx4' in body and any(s == 'x4' for s in stores), sym
        nt_stores = [l for l in re.findall(r'global_store_dword\w*[^\n]*', body) if ' nt' in l]
        assert len(nt_stores) >= 1, sym                                           # the tick panels: written once, never read here
