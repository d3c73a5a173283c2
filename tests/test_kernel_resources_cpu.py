"""Static resource check of every gfx950 kernel (no GPU needed: hipcc cross-compiles): nothing may touch scratch.

A spilled register or a lambda that the compiler did not inline (its captured loop state then lives in scratch memory)
costs 10-20 % on the affinity kernels without failing a single numerical test -- the round-2 measurements of that are
in profiles/r02e_affinity_shapes.txt (items 2 and 11) -- so the compiler's own resource report is asserted here, with
the flags of csrc/Makefile."""
import os

import pytest

import abi_util
from abi_util import HIPCC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'tracking-anything-with-deva_amd', 'csrc')
SOURCES = sorted(f for f in os.listdir(CSRC) if f.endswith('.hip'))
# once-per-frame kernels whose per-thread tables are indexed dynamically (the antialias filter taps of the input head)
SCRATCH_BY_DESIGN = ('input_head_kernel',)
# kernel-name fragment -> waves per SIMD the launch geometry is sized for (2 workgroups of 4 waves per CU, ...)
MIN_OCCUPANCY = {
    'affinity_topk_wg_kernelILi352ELi2ELi4E': 2,
    'affinity_topk_wg_kernelILi704ELi1ELi8E': 2,
    'affinity_topk_kernelILi100ELi2EE': 2,
    'conv_igemm_kernelILi128ELi128E': 4,
    'affinity_pf_pass_kernelILi0ELi2E': 2,
    'affinity_pf_pass_kernelILi1ELi2E': 2,
    'affinity_pf_pass_kernelILi0ELi1E': 2,
    'affinity_pf_pass_kernelILi1ELi1E': 2,
}
# the source that carries each of them: a kernel that moves or is renamed must take its entry along
HOME = {'affinity_topk': 'affinity.hip', 'affinity_pf_pass': 'affinity_prefilter.hip', 'conv_igemm': 'conv_igemm.hip'}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not found')
@pytest.mark.parametrize('src', SOURCES)
def test_no_kernel_spills_or_uses_scratch(src):
    # (empty for host-only sources such as runtime.hip)
    kernels = abi_util.kernel_resources(os.path.join(CSRC, src), ['-mllvm', '-amdgpu-mfma-vgpr-form=1'] if src.startswith('affinity') else ())
    for name, r in kernels.items():
        if any(k in name for k in SCRATCH_BY_DESIGN):
            continue
        assert r.get('ScratchSize', 0) == 0, (name, r)
        assert r.get('VGPRs Spill', 0) == 0, (name, r)  # (SGPR spills go to VGPR lanes, not to memory)
        assert r.get('LDS Size', 0) <= 160 * 1024, (name, r)
        for frag, occ in MIN_OCCUPANCY.items():
            if frag in name:
                assert r['Occupancy'] >= occ, (name, r)
    for prefix, home in HOME.items():  # (affinity.hip: the three list-kernel shapes the automatic choice uses)
        if src == home:
            for frag in MIN_OCCUPANCY:
                assert not frag.startswith(prefix) or any(frag in n for n in kernels), frag


def test_every_sized_kernel_has_a_home():
    assert all(any(frag.startswith(p) for p in HOME) for frag in MIN_OCCUPANCY) and set(HOME.values()) <= set(SOURCES)
