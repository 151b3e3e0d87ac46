"""ISA audit of the narrow-width fused readout for gfx950 (cross-compiles on the CPU): every instantiation of readout_narrow_kernel
(rk.hip: 1 to 4 quads per thread, aligned and unaligned panels), compiled with build()'s flags, spills no register, uses no private
segment - at four quads a thread holds 80 fit coefficients and state values - and makes no call."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not installed')


@pytest.fixture(scope='module')
def asm(tmp_path_factory):
    import __graft_entry__ as entry
    path = str(tmp_path_factory.mktemp('isa') / 'rk.s')
    flags = [f for f in entry.HIPCC_FLAGS if f != '-fPIC']
    subprocess.run([HIPCC] + flags + ['-S', '--cuda-device-only', '-o', path, os.path.join(ROOT, 'ndcn_amd', 'csrc', 'rk.hip')],
                   check=True, stderr=subprocess.DEVNULL)
    return open(path).read()


def metadata(text, pattern):
    blocks = re.findall(r'\.name:\s+(\S*(?:%s)\S*)(.*?)(?=\n\s+- \.|\n\s*\.end_amdgpu_metadata)' % pattern, text, re.S)
    return {n: dict(re.findall(r'\.(vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size|vgpr_count):\s+(\d+)', meta))
            for n, meta in blocks}


def body_of(text, symbol):
    m = re.search(r'^%s:[^\n]*\n(.*?)^\s*s_endpgm' % re.escape(symbol), text, re.S | re.M)
    assert m, symbol
    return m.group(1)


def test_every_instantiation_exists_without_spill_private_segment_or_call(asm):
    meta = metadata(asm, 'readout_narrow_kernel')
    got = sorted(tuple(int(v) for v in re.search(r'readout_narrow_kernelILi(\d)ELb([01])E', n).groups()) for n in meta)
    assert got == [(nq, vec) for nq in (1, 2, 3, 4) for vec in (0, 1)], sorted(meta)
    for name, fields in meta.items():
        print(name, fields)
        assert fields.get('vgpr_spill_count') == '0' and fields.get('sgpr_spill_count') == '0', (name, fields)
        assert fields.get('private_segment_fixed_size') == '0', (name, fields)
        assert 's_swappc' not in body_of(asm, name), name
