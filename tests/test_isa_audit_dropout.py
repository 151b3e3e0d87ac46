"""ISA audit of the dropout kernels for gfx950 (cross-compiles on the CPU): dropout_apply_kernel (dropout.hip) and the dropout
instantiations of the narrow-panel launch (rhs_small.hip: rhs_small_kernel<.., DropArgs>) have no spill and no scratch; the vector form of
dropout_apply moves 16 bytes per access and keeps the Philox rounds as v_mul_hi_u32 (not 64-bit library calls); and the p = 0
instantiations of rhs_small_kernel carry no trace of the generator - the feature costs them nothing.

The last check was planned as "the p = 0 instantiations contain no v_mul_hi_u32".  They always did: the weight staging loop splits
i into (i / H, i % H) and the compiler divides by the run-time H with high products (14 of them, before and after this change).  The
instruction therefore cannot tell the generator's presence; its four constants can - no Philox round exists without the two
multipliers, no key schedule without the two Weyl increments - so the check is that none of them occurs in a p = 0 body, and that
every one occurs in each dropout body.  (That the p = 0 bodies are the ones they were is not something this file can see; the
p = 0 instantiations take no extra argument and no extra template value, and DESIGN section 2 says how they were compared.)"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
PHILOX_CONSTANTS = ('0xd2511f53', '0xcd9e8d57', '0x9e3779b9', '0xbb67ae85')       # the two multipliers, the two Weyl increments
pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not installed')


def compile_asm(tmp, name):
    path = str(tmp / (name + '.s'))
    subprocess.run([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-S', '--cuda-device-only', '-o', path,
                    os.path.join(ROOT, 'ndcn_amd', 'csrc', name + '.hip')], check=True, stderr=subprocess.DEVNULL)
    return open(path).read()


@pytest.fixture(scope='module')
def asm_apply(tmp_path_factory):
    return compile_asm(tmp_path_factory.mktemp('isa'), 'dropout')


@pytest.fixture(scope='module')
def asm_small(tmp_path_factory):
    return compile_asm(tmp_path_factory.mktemp('isa'), 'rhs_small')


def body_of(text, symbol):
    m = re.search(r'^%s:[^\n]*\n(.*?)^\s*s_endpgm' % re.escape(symbol), text, re.S | re.M)
    assert m, symbol
    return m.group(1)


def metadata(text, pattern):
    blocks = re.findall(r'\.name:\s+(\S*(?:%s)\S*)(.*?)(?=\n\s+- \.|\n\s*\.end_amdgpu_metadata)' % pattern, text, re.S)
    return {n: dict(re.findall(r'\.(vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size|vgpr_count):\s+(\d+)', meta))
            for n, meta in blocks}


def is_drop(symbol):
    """rhs_small_kernel<NH, HALO, MODE, DROP...>: the dropout instantiations carry DropArgs in the template pack"""
    return 'DropArgs' in symbol.split('EvNS')[0]


def assert_no_spill(fields, name):
    assert fields.get('vgpr_spill_count') == '0' and fields.get('sgpr_spill_count') == '0', (name, fields)
    assert fields.get('private_segment_fixed_size') == '0', (name, fields)
    assert int(fields.get('vgpr_count', '999')) <= 128, (name, fields)


def test_dropout_apply_kernels(asm_apply):
    meta = metadata(asm_apply, 'dropout_apply_kernel')
    assert len(meta) == 2, sorted(meta)                                            # <VEC> x 2
    assert sorted('Lb1E' in name for name in meta) == [False, True], sorted(meta)  # exactly one is the vector form
    for name, fields in meta.items():
        assert_no_spill(fields, name)
        body = body_of(asm_apply, name)
        assert 'scratch_' not in body and 'buffer_store' not in body and 's_swappc' not in body, name
        assert 'v_mul_hi_u32' in body, name                                        # the rounds stayed 32 x 32 -> high word
        if 'Lb1E' in name:                                                         # the vector form: 16 bytes per access
            assert 'global_load_dwordx4' in body and 'global_store_dwordx4' in body, name
            # one Philox call per four elements: 2 high products per round, 10 rounds, in the main loop; the scalar tail has its own
            assert body.count('v_mul_hi_u32') >= 20, name


def test_dropout_instantiations_of_the_narrow_panel_launch(asm_small):
    meta = {n: f for n, f in metadata(asm_small, 'rhs_small_kernel').items() if is_drop(n)}
    assert len(meta) == 8, sorted(meta)                                            # <NH 1 / 2> x <plain, COMBINE, ERROR, RK4>
    for name, fields in meta.items():
        assert_no_spill(fields, name)
        body = body_of(asm_small, name)
        assert 'scratch_' not in body and 's_swappc' not in body, name
        assert 'v_mul_hi_u32' in body, name
        for const in PHILOX_CONSTANTS:
            assert const in body.lower(), (name, const)


def test_p0_instantiations_carry_no_generator(asm_small):
    meta = {n: f for n, f in metadata(asm_small, 'rhs_small_kernel').items() if not is_drop(n)}
    assert len(meta) == 16, sorted(meta)                                           # <NH> x <HALO> x <MODE>
    for name, fields in meta.items():
        assert_no_spill(fields, name)
        body = body_of(asm_small, name)
        for const in PHILOX_CONSTANTS:
            assert const not in body.lower(), (name, const)
