"""ISA audit of rhs_fused3.hip's dopri5 dense-output variants (rhs_fused3_dense_kernel: <COMBINE, 4> without the store of K, with
and without the midpoint sum M in its place), the same rules as the inference-path
kernels in test_isa_audit.py: no instruction touches a panel register while its request is in flight, no spill, no scratch.
Cross-compiles on the CPU."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not installed')
def test_fused3_dense_variants_never_touch_panels_in_flight(tmp_path):
    asm = str(tmp_path / 'rhs_fused3.s')
    subprocess.run([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-S', '--cuda-device-only', '-o', asm,
                    os.path.join(ROOT, 'ndcn_amd', 'csrc', 'rhs_fused3.hip')], check=True, stderr=subprocess.DEVNULL)
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'audit_async_regs.py'), asm, 'rhs_fused3_dense_kernel'],
                         capture_output=True, text=True)
    assert out.returncode == 0 and 'TOTAL problems 0' in out.stdout, out.stdout[-2000:]
    # {M in K's panel, no K} x {non-temporal, plain stores}: only the variants the solver launches
    assert out.stdout.count('asm loads') == 4, out.stdout
    text = open(asm).read()
    # per-kernel metadata of the dense variants: no spill, no private segment (scratch), at most 128 registers
    blocks = re.findall(r'\.name:\s+(\S*rhs_fused3_dense_kernel\S*)(.*?)(?=\n\s+- \.|\n\s*\.end_amdgpu_metadata)', text, re.S)
    names = set(n for n, _ in blocks)
    assert len(names) == 4, names
    for name, meta in blocks:
        fields = dict(re.findall(r'\.(vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size|vgpr_count):\s+(\d+)', meta))
        assert fields.get('vgpr_spill_count') == '0' and fields.get('sgpr_spill_count') == '0', (name, fields)
        assert fields.get('private_segment_fixed_size') == '0', (name, fields)
        assert int(fields.get('vgpr_count', '999')) <= 128, (name, fields)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not installed')
def test_fused3_dense_variants_request_what_the_combine4_kernel_requests(tmp_path):
    """The producer pipeline's run-time waits count every vector-memory operation a wave issues (rhs_fused3.hip: issued()).  The dense
    variants must not change what is counted beyond their stores: the same panel loads and LDS-DMA requests as the <COMBINE, 4>
    kernel of the inference path, the same number of stores with M in K's place, fewer without K."""
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_isa_audit import text_of
    asm = str(tmp_path / 'rhs_fused3.s')
    subprocess.run([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-S', '--cuda-device-only', '-o', asm,
                    os.path.join(ROOT, 'ndcn_amd', 'csrc', 'rhs_fused3.hip')], check=True, stderr=subprocess.DEVNULL)

    def mem(symbol):
        lines = list(text_of(asm, symbol))
        assert lines, symbol
        return (sum('global_load_dwordx4' in l for l in lines), sum('global_load_lds' in l for l in lines),
                sum('global_store' in l for l in lines))
    for nt in ('0', '1'):
        base = mem('_ZN4ndcn17rhs_fused3_kernelILb0ELi1ELi4ELi0ELb%sELb0ELb0EEEvNS_6F3ArgsENS_5F3EpiE' % nt)
        mid = mem('_ZN4ndcn23rhs_fused3_dense_kernelILi1ELi4ELb%sELb1ELi1EEEvNS_6F3ArgsENS_5F3EpiE' % nt)
        nok = mem('_ZN4ndcn23rhs_fused3_dense_kernelILi1ELi4ELb%sELb1ELi0EEEvNS_6F3ArgsENS_5F3EpiE' % nt)
        assert mid == base, (nt, mid, base)
        assert nok[:2] == base[:2] and nok[2] < base[2], (nt, nok, base)
