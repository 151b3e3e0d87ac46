"""ISA audit of the H = 256 backward kernels of the dense Linear (linear_bwd.hip): the resident-weight gS kernel computes its buffer
offsets in unsigned arithmetic (rows past 2^21 put them above 2^31); that must not cost registers, scratch or spills.  Ceilings are
the register counts before the change.  Cross-compiles on the CPU."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')

# kernel (mangled-name fragment) -> VGPR ceiling
CEILINGS = {
    'linear_gs_256_res_kernelILb1E': 228,
    'linear_gs_256_res_kernelILb0E': 198,
    'linear_gs_256_split_kernelILi1E': 124,
    'linear_gs_256_split_kernelILi2E': 172,
    'linear_wgrad_256_split_kernel': 247,
}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not installed')
def test_linear_bwd_256_kernels_no_scratch_no_spill_no_more_registers(tmp_path):
    asm = str(tmp_path / 'linear_bwd.s')
    subprocess.run([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-S', '--cuda-device-only', '-o', asm,
                    os.path.join(ROOT, 'ndcn_amd', 'csrc', 'linear_bwd.hip')], check=True, stderr=subprocess.DEVNULL)
    text = open(asm).read()
    blocks = re.findall(r'\.name:\s+(\S*linear\S*)(.*?)(?=\n\s+- \.|\n\s*\.end_amdgpu_metadata)', text, re.S)
    seen = set()
    for name, meta in blocks:
        key = next((k for k in CEILINGS if k in name), None)
        if key is None:
            continue
        seen.add(key)
        fields = dict(re.findall(r'\.(vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size|vgpr_count):\s+(\d+)', meta))
        assert fields.get('vgpr_spill_count') == '0' and fields.get('sgpr_spill_count') == '0', (name, fields)
        assert fields.get('private_segment_fixed_size') == '0', (name, fields)
        assert int(fields.get('vgpr_count', '999')) <= CEILINGS[key], (name, fields)
    assert seen == set(CEILINGS), seen
    # no scratch instructions anywhere in the resident-weight kernel's body
    for mangled in re.findall(r'^(_ZN4ndcn24linear_gs_256_res_kernel\S*):', text, re.M):
        body = text[text.index(mangled + ':'):text.index('.Lfunc_end', text.index(mangled + ':'))]
        assert 'scratch_' not in body, mangled
