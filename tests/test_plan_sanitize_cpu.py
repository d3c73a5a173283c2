"""The HIP-free host code of every feature -- argument checks, scratch layouts, launch decisions, the convolution planner
and the weight packers -- under the host sanitizers, each as a stand-alone program: tests/<main> walks its sources over
the product of their boundary values with made-up addresses (nothing is dereferenced; the convolution one also packs one
tiny layer per packer and layout into buffers of exactly the size asked for) and prints how many calls it made, how many
were refused and how many answered wrongly.  Nothing is loaded into Python and no GPU is involved."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'tracking-anything-with-deva_amd', 'csrc')
CLANG = os.environ.get('DEVA_HOST_CXX', '/opt/rocm/llvm/bin/clang++')

# id -> (sources under csrc/, main under tests/, include directories under csrc/)
PROGRAMS = {
    'conv': (['conv_plan.cpp', 'conv_pack.cpp'], 'conv_plan_sanitize_main.cpp', ['']),
    'detection': (['detection_plan.cpp'], 'detection_plan_sanitize_main.cpp', ['']),
    'proposal': (['proposal_plan.cpp'], 'proposal_plan_sanitize_main.cpp', ['']),
    'prompt': (['prompt_plan.cpp'], 'prompt_plan_sanitize_main.cpp', ['']),
    'box_prompt': (['box_prompt_plan.cpp', 'proposal_plan.cpp'], 'box_prompt_plan_sanitize_main.cpp', ['']),   # (the NMS's scratch)
    'panoptic': (['metrics/panoptic_plan.cpp'], 'panoptic_plan_sanitize_main.cpp', ['metrics']),
    'vos': (['vos_metrics/boundary_plan.cpp'], 'vos_plan_sanitize_main.cpp', ['vos_metrics']),
}


@pytest.mark.parametrize('name', list(PROGRAMS))
def test_host_code_under_host_sanitizers(name, tmp_path):
    sources, main, dirs = PROGRAMS[name]
    exe = tmp_path / (name + '_sanitize')
    includes = [arg for d in dirs for arg in ('-I', os.path.join(CSRC, d))]
    subprocess.run([CLANG, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    '-I', os.path.join(ROOT, 'include')] + includes + [os.path.join(CSRC, s) for s in sources] +
                   [os.path.join(ROOT, 'tests', main), '-o', str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout, run.stderr[-4000:])
    assert run.returncode == 0, run.stderr[-4000:]
    checks, refused, failures = (int(v) for v in re.findall(r'\d+', run.stdout))
    assert checks > 100000 and 0 < refused < checks and failures == 0
