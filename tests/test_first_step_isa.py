"""The first-step instantiations (ABI v37) as the compiler reports them (``-Rpass-analysis=kernel-resource-usage``, the library's own flags; needs
hipcc, no GPU): no scratch in any of them, and the two-ring blend on the zero state -- a translation unit of its own, outside the count of
tests/test_isa.py -- keeps the <= 256 registers that let two workgroups share a compute unit."""
import os
import re
import subprocess

import pytest

from tests.test_isa import CSRC, HIPCC, _library_flags


def _resource_usage(source, tmp_path):
    """{kernel name: {field: int}} of every kernel ``source`` compiles to."""
    out = subprocess.run([HIPCC, *_library_flags(source), '-Rpass-analysis=kernel-resource-usage', '-c', '--cuda-device-only', '-o',
                          str(tmp_path / 'unit.o'), os.path.join(CSRC, source)], stderr=subprocess.PIPE, text=True, check=True).stderr
    usage, name = {}, None
    for line in out.split('\n'):
        m = re.search(r'remark:\s+Function Name: (\S+)', line)
        if m:
            name = m.group(1)
            usage[name] = {}
            continue
        m = re.search(r'remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)', line)
        if m and name:
            usage[name][m.group(1).strip()] = int(m.group(2))
    return usage


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not present')
def test_two_ring_blend_on_the_zero_state_keeps_two_workgroups_per_cu_without_scratch(tmp_path):
    usage = _resource_usage('stc_spmm_ring2_first.hip', tmp_path)
    assert len(usage) == 1, sorted(usage)                       # the R2_BLEND0 form of ring2_sum_kernel and nothing else
    (name, u), = usage.items()
    assert 'ring2_sum_kernelILi3ELb0ELi1ELi0E' in name, name
    assert u['VGPRs'] <= 256 and u['ScratchSize'] == 0 and u['Occupancy'] >= 2, (name, u)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not present')
@pytest.mark.parametrize('source,pattern,n_forms', [('stc_cell_bwd_x3.hip', r'cell_bwd_x3_kernelINS_5Fmt\w\dELi\d+ELi\dELi\dELi0ELi1EE', 6),
                                                    ('stc_node_x3.hip', r'node_fwd_x3_kernelI.*NS_5Fmt\w\dELi1EE', 4)])
def test_first_step_cell_kernels_use_no_scratch(tmp_path, source, pattern, n_forms):
    """cell_bwd_x3_kernel<F, L, PL, ACCX, 0, FIRST = 1> (both formats x wide, wide accumulating, narrow) and node_fwd_x3_kernel<..., F, FIRST = 1>
    (both formats x wide, narrow)."""
    usage = {k: u for k, u in _resource_usage(source, tmp_path).items() if re.search(pattern, k)}
    assert len(usage) == n_forms, sorted(usage)
    for name, u in usage.items():
        assert u['ScratchSize'] == 0, (name, u)
