"""Static resource check of the gfx950 kernels of the scoring library (csrc/metrics/*.hip, which the listing of
tests/test_kernel_resources_cpu.py does not reach), with its assertions and the flags of csrc/Makefile: nothing may
touch scratch, no VGPR may spill, LDS stays within 160 KB.  No GPU needed: hipcc cross-compiles."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'tracking-anything-with-deva_amd', 'csrc', 'metrics')
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
SOURCES = sorted(f for f in os.listdir(CSRC) if f.endswith('.hip'))


def resource_report(src, tmp_path):
    flags = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-I' + os.path.join(ROOT, 'include'),
             '-Rpass-analysis=kernel-resource-usage']
    out = subprocess.run([HIPCC] + flags + ['-c', os.path.join(CSRC, src), '-o', str(tmp_path / (src + '.o'))],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    kernels, cur = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r'remark: (?:Function Name: (\S+)|\s*([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+))', line)
        if not m:
            continue
        if m.group(1):
            cur = kernels.setdefault(m.group(1), {})
        elif cur is not None:
            cur[m.group(2).strip()] = int(m.group(3))
    return kernels


def test_the_listing_is_not_empty():
    assert 'panoptic_counts.hip' in SOURCES


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not found')
@pytest.mark.parametrize('src', SOURCES)
def test_no_kernel_spills_or_uses_scratch(src, tmp_path):
    kernels = resource_report(src, tmp_path)
    if src == 'panoptic_counts.hip':   # 2 ground-truth encodings x 4 predicted x (LDS, global)
        assert sum('panoptic_counts_kernel' in name for name in kernels) == 16
    for name, r in kernels.items():
        assert r.get('ScratchSize', 0) == 0, (name, r)
        assert r.get('VGPRs Spill', 0) == 0, (name, r)  # (SGPR spills go to VGPR lanes, not to memory)
        assert r.get('LDS Size', 0) <= 160 * 1024, (name, r)
        assert r['Occupancy'] >= 4, (name, r)            # the launch is sized for 8 workgroups of 4 waves per CU
