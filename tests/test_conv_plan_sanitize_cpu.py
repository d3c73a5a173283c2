"""The HIP-free convolution code -- the dispatch planner (csrc/conv_plan.cpp) and the weight packers (csrc/conv_pack.cpp) --
under the host sanitizers, as a stand-alone program: tests/conv_plan_sanitize_main.cpp walks the planner over the product
of its boundary values (made-up addresses: the planner dereferences none) and packs one tiny layer per packer and layout
into buffers of exactly the size asked for.  Nothing is loaded into Python and no GPU is involved."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'tracking-anything-with-deva_amd', 'csrc')
CLANG = os.environ.get('DEVA_HOST_CXX', '/opt/rocm/llvm/bin/clang++')


def test_conv_planner_and_packers_under_host_sanitizers(tmp_path):
    exe = tmp_path / 'conv_plan_sanitize'
    subprocess.run([CLANG, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    '-I', os.path.join(ROOT, 'include'), '-I', CSRC,
                    os.path.join(CSRC, 'conv_plan.cpp'), os.path.join(CSRC, 'conv_pack.cpp'),
                    os.path.join(ROOT, 'tests', 'conv_plan_sanitize_main.cpp'), '-o', str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout, run.stderr[-4000:])
    assert run.returncode == 0, run.stderr[-4000:]
    plans, refused, failures = (int(v) for v in re.findall(r'\d+', run.stdout))
    assert plans > 100000 and 0 < refused < plans and failures == 0
