"""What the ABI tests of every feature ask of a library: that it is built, what its header declares, what it exports,
and that a feature's entry points are exported, declared and bound; and what the static-resource tests ask of the
compiler about a source file's kernels."""
import ctypes
import os
import re
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'


def built(module):
    """a binding module (`deva.hip`, `deva.hip.metrics`, `deva.hip.vos_metrics`) whose library exists -> the module"""
    if not os.path.exists(module.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return module


def declared(header):
    text = open(header).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    text = re.sub(r'//[^\n]*', '', text)
    return sorted(set(re.findall(r'\b(deva_[a-z0-9_]+)\s*\(', text)))


def exported(lib_path):
    """-> (the deva_* functions, sorted; every symbol the library defines)"""
    out = subprocess.run(['nm', '-D', '--defined-only', lib_path], capture_output=True, text=True, check=True).stdout
    return sorted(set(re.findall(r'\bT (deva_[a-z0-9_]+)$', out, flags=re.M))), set(re.findall(r'\b[TDBW] (\S+)$', out, flags=re.M))


def kernel_resources(source, extra_flags=()):
    """a .hip file compiled for gfx950 with the common flags of csrc/Makefile (and `extra_flags`, for a file that has
    flags of its own there) -> {kernel name: {field: int}} from the compiler's resource remarks: 'VGPRs', 'SGPRs',
    'ScratchSize', 'VGPRs Spill', 'SGPRs Spill', 'LDS Size', 'Occupancy', ...; empty for a source without kernels"""
    flags = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-I' + os.path.join(ROOT, 'include'),
             '-Rpass-analysis=kernel-resource-usage']
    with tempfile.TemporaryDirectory() as tmp:
        out = subprocess.run([HIPCC] + flags + list(extra_flags) + ['-c', source, '-o', os.path.join(tmp, 'kernels.o')],
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


def inference_entry_points(names, returns=r'int(?:64_t)?'):
    """every name is exported by libdeva_hip.so, declared in deva_hip.h and bound; the version has not moved -> the header"""
    from deva import hip
    handle = ctypes.CDLL(built(hip).LIB_PATH)
    header = open(os.path.join(ROOT, 'include', 'deva_hip.h')).read()
    for name in names:
        assert hasattr(handle, name), f'{name} not exported'
        assert re.search(r'\b' + returns + ' ' + name + r'\s*\(', header), f'{name} not declared'
        assert name in hip.SIGNATURES
    assert hip.ABI_VERSION == 11 and hip.lib().deva_hip_version() == 11  # additive: the version does not move
    assert re.search(r'#define DEVA_HIP_ABI_VERSION 11\b', header)
    return header
