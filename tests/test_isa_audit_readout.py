"""ISA audit of the fused dense-output readout for gfx950 (cross-compiles on the CPU): every NV instantiation of
interp_readout_kernel (rk.hip), compiled with build()'s flags, uses no private segment and spills no register - at NV = 8 a lane
holds 40 fit coefficients plus 8 evaluated elements - and the only fused multiply-adds in its body are the decoder's own chain
(NV per tick, 8 unrolled ticks): rk.hip switches FP contraction off, and a contracted fit1 / poly1 would round differently from
interp_direct_multi_kernel, whose tick panels the readout is defined by."""
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


def nv_of(symbol):
    m = re.search(r'interp_readout_kernelILi(\d)E', symbol)
    assert m, symbol
    return int(m.group(1))


def test_every_nv_instantiation_exists_without_spill_or_private_segment(asm):
    meta = metadata(asm, 'interp_readout_kernel')
    assert sorted(nv_of(n) for n in meta) == list(range(1, 9)), sorted(meta)
    for name, fields in meta.items():
        assert fields.get('vgpr_spill_count') == '0' and fields.get('sgpr_spill_count') == '0', (name, fields)
        assert fields.get('private_segment_fixed_size') == '0', (name, fields)
        assert int(fields.get('vgpr_count', '999')) <= 128, (name, fields)          # 4 waves per SIMD stay resident
        assert 's_swappc' not in body_of(asm, name), name


def test_only_the_decoder_chain_is_fused(asm):
    for name in metadata(asm, 'interp_readout_kernel'):
        n_fma = len(re.findall(r'^\s*v_(?:fma|fmac|pk_fma)_f32', body_of(asm, name), re.M))
        assert 0 < n_fma <= 8 * nv_of(name), (name, n_fma)
