"""The HIP-free side of the joint count -- every argument check of deva_metrics_panoptic_counts and the launch decision
behind deva_metrics_panoptic_plan (csrc/metrics/panoptic_plan.cpp) -- under the host sanitizers, as a stand-alone
program: tests/panoptic_plan_sanitize_main.cpp walks them over the product of their boundary values with made-up
addresses (nothing is dereferenced).  Nothing is loaded into Python and no GPU is involved."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'tracking-anything-with-deva_amd', 'csrc', 'metrics')
CLANG = os.environ.get('DEVA_HOST_CXX', '/opt/rocm/llvm/bin/clang++')


def test_panoptic_plan_and_checks_under_host_sanitizers(tmp_path):
    exe = tmp_path / 'panoptic_plan_sanitize'
    subprocess.run([CLANG, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    '-I', os.path.join(ROOT, 'include'), '-I', CSRC, os.path.join(CSRC, 'panoptic_plan.cpp'),
                    os.path.join(ROOT, 'tests', 'panoptic_plan_sanitize_main.cpp'), '-o', str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout, run.stderr[-4000:])
    assert run.returncode == 0, run.stderr[-4000:]
    checks, refused, failures = (int(v) for v in re.findall(r'\d+', run.stdout))
    assert checks > 100000 and 0 < refused < checks and failures == 0
