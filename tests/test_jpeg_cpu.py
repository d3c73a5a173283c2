"""The JPEG coder without a GPU: libdeva_jpeg.so on its ABI, the plan by hand, the refusals before any launch, the plan's
host code under the host sanitizers, the kernels' static resources, the numpy statement of rules J1-J10
(tests/jpeg_case.py) against libjpeg's tables (through PIL), by hand and through `PIL.Image.open` against PIL's own files,
the crafted image that reaches the corners of the code space, and `FrameResultSaver(jpeg='device')` on the CPU contracts
(tests/emu_jpeg.py) against `jpeg='host'`."""
import ctypes
import functools
import io
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch
from PIL import Image

import abi_util
import emu_frame_result as EF
import emu_jpeg as EJPEG
import emu_ops
import emu_png as EPNG
import jpeg_case as JC
import result_case as RC

torch.set_grad_enabled(False)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'deva_jpeg.h')
CSRC = os.path.join(ROOT, 'tracking-anything-with-deva_amd', 'csrc')
JPEG_SRC = os.path.join(CSRC, 'jpeg')
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
CLANG = os.environ.get('DEVA_HOST_CXX', '/opt/rocm/llvm/bin/clang++')
WANT = ['deva_jpeg_last_error', 'deva_jpeg_limits', 'deva_jpeg_place', 'deva_jpeg_plan', 'deva_jpeg_quant', 'deva_jpeg_scan', 'deva_jpeg_version']
SUBS = ('4:2:0', '4:4:4')


def _built():
    from deva.hip import jpeg
    return abi_util.built(jpeg)


# ------------------------------------------------------------------------------------------ layout and ABI
def test_exports_header_and_binding_are_one_list():
    jpeg = _built()
    exported, _ = abi_util.exported(jpeg.LIB_PATH)
    assert exported == abi_util.declared(HEADER) == sorted(jpeg.SIGNATURES) == WANT
    header = open(HEADER).read()
    assert re.search(r'#define DEVA_JPEG_ABI_VERSION 1\b', header)
    assert jpeg.ABI_VERSION == 1 and jpeg.lib().deva_jpeg_version() == 1
    for name, value in (('MAX_SIDE', jpeg.MAX_SIDE), ('MAX_RESTART', jpeg.MAX_RESTART), ('420', 420), ('444', 444)):
        assert re.search(rf'#define DEVA_JPEG_{name} {value}\b', header), name
    assert re.search(r'#define DEVA_JPEG_MAX_BYTES \(1 << 29\)', header) and jpeg.MAX_BYTES == 1 << 29
    assert jpeg.SUBSAMPLINGS == {'4:2:0': 420, '4:4:4': 444}
    for rule in ('J1', 'J2', 'J3', 'J4', 'J5', 'J6', 'J7', 'J8', 'J9', 'J10'):
        assert re.search(rf'^ \* {rule}\. ', header, flags=re.M), rule
    limits = jpeg.limits()
    assert limits[:5] == (jpeg.MAX_SIDE, jpeg.MAX_BYTES, jpeg.MAX_RESTART, 20 + 63 * 26, 256) and limits.lds_bytes <= 65536
    assert (limits.block, limits.block_bits, limits.max_side, limits.max_bytes) == (JC.BLOCK, JC.BLOCK_BITS, JC.MAX_SIDE, JC.MAX_BYTES)
    assert os.path.basename(os.path.dirname(jpeg.LIB_PATH)) == 'jpeg_lib'
    assert {'jpeg_encode.hip', 'jpeg_plan.cpp', 'jpeg_plan.h'} <= set(os.listdir(JPEG_SRC))


def test_no_symbol_is_shared_and_the_other_libraries_have_not_moved():
    from deva import hip
    from deva.hip import lowres, mask_runs, metrics, pair_metrics, png, regions, rle, rle_overlap, rle_text, vos_metrics
    jpeg = _built()
    exported, mine = abi_util.exported(jpeg.LIB_PATH)
    assert all(name.startswith('deva_jpeg_') for name in exported)
    others = (hip, metrics, vos_metrics, pair_metrics, regions, rle, mask_runs, rle_overlap, rle_text, lowres, png)
    for other in others:
        theirs_exported, theirs = abi_util.exported(abi_util.built(other).LIB_PATH)
        assert not any(n.startswith('deva_jpeg') for n in theirs_exported)
        shared = {s for s in mine & theirs if 'deva' in s}
        assert not shared, (other.LIB_PATH, shared)
    for name in sorted(os.listdir(os.path.join(ROOT, 'include'))):
        if name != 'deva_jpeg.h':
            assert 'deva_jpeg' not in open(os.path.join(ROOT, 'include', name)).read(), name
    abi_util.inference_entry_points([])       # libdeva_hip.so stays at its ABI version
    assert len(hip.SIGNATURES) == 80
    assert [m.ABI_VERSION for m in others[1:]] == [1] * 10
    assert os.path.basename(os.path.dirname(png.LIB_PATH)) == 'png_lib'


def test_struct_mirrors_have_the_c_layout(tmp_path):
    jpeg = _built()
    assert [f[0] for f in jpeg.Plan._fields_] == list(jpeg.PlanInfo._fields)
    assert [f[0] for f in jpeg.Limits._fields_] == list(jpeg.LimitInfo._fields)
    mirrors = (('deva_jpeg_plan', jpeg.Plan), ('deva_jpeg_limits', jpeg.Limits))
    lines = []
    for tag, mirror in mirrors:
        lines.append(f'printf("%zu\\n", sizeof(struct {tag}));\n')
        lines += [f'printf("%zu\\n", offsetof(struct {tag}, {f[0]}));\n' for f in mirror._fields_]
    src = tmp_path / 'probe.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "deva_jpeg.h"\nint main(void){\n' + ''.join(lines) + 'return 0;}\n')
    exe = tmp_path / 'probe'
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    vals = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = []
    for _, mirror in mirrors:
        want += [ctypes.sizeof(mirror)] + [getattr(mirror, f[0]).offset for f in mirror._fields_]
    assert vals == want


# ------------------------------------------------------------------------------------------ the plan by hand
def test_plan_by_hand():
    jpeg = _built()
    # one pixel at 4:2:0: one MCU of 6 blocks, one interval.  6 * 1658 = 9948 bits -> 1244 bytes, stuffed 2488, the marker 2:
    # 2490 -> a slot of 2496 + 16.  Scratch: two tables of 8 -> 256 each, 768 bytes of coefficients, a slot of 2512 -> 2560.
    assert jpeg.plan(1, 1) == jpeg.PlanInfo(16, 1, 1, 6, 1, 1, 6, 256, 768, 2512, 256 + 256 + 768 + 2560, 2488)
    # at 4:4:4: 3 blocks, 4974 bits -> 622 bytes -> 1246 with the marker -> 1248 + 16; 384 bytes of coefficients take 512
    assert jpeg.plan(1, 1, '4:4:4') == jpeg.PlanInfo(8, 1, 1, 3, 1, 1, 3, 256, 384, 1264, 256 + 256 + 512 + 1280, 1244)
    # 17 x 33 at 4:2:0: 3 x 2 MCUs, an interval an MCU row of 3: 18 blocks -> 29844 bits -> 3731 bytes (rounded up) -> 7464
    p = jpeg.plan(17, 33)
    assert p[:8] == (16, 3, 2, 6, 3, 2, 36, 256) and p.coef_bytes == 36 * 128
    assert p.slot_bytes == 7472 + 16 and p.worst_case == 2 * 7464 - 2 and p.scratch_bytes == 256 + 256 + 4608 + 15104
    # at 4:4:4: 5 x 3 MCUs of 3 blocks, 15 blocks an interval -> 24870 bits -> 3109 bytes -> 6220; with restart=4: 4 intervals, the last of 3 MCUs
    p = jpeg.plan(17, 33, '4:4:4')
    assert p[:8] == (8, 5, 3, 3, 5, 3, 45, 256) and p.worst_case == 3 * 6220 - 2 and p.slot_bytes == 6224 + 16
    p = jpeg.plan(17, 33, '4:4:4', 4)
    assert (p.restart, p.intervals) == (4, 4) and p.worst_case == 3 * (2 * 2487 + 2) + (2 * 1866 + 2) - 2
    # 1080p at 4:2:0: 120 x 68 MCUs, 68 intervals of 720 blocks: 1193760 bits = 149220 bytes -> 298442 -> a slot of 298448 + 16
    p = jpeg.plan(1080, 1920)
    assert p[:8] == (16, 120, 68, 6, 120, 68, 48960, 256) and p.coef_bytes == 6266880
    assert p.slot_bytes == 298464 and p.worst_case == 68 * 298442 - 2
    assert p.scratch_bytes == 2 * 768 + 6266880 + 68 * 298464 + (-(68 * 298464) % 256)
    # at 4:4:4: 240 x 135 MCUs, 135 intervals of 720 blocks
    p = jpeg.plan(1080, 1920, '4:4:4')
    assert p[:8] == (8, 240, 135, 3, 240, 135, 97200, 256) and p.worst_case == 135 * 298442 - 2
    # the whole picture in one interval
    p = jpeg.plan(1080, 1920, restart=8160)
    assert p.intervals == 1 and p.worst_case == 2 * (48960 * 1658 // 8) + 2 - 2
    for shape in ((1, 1), (17, 33), (9, 1023), (480, 854), (1080, 1920), (2160, 3840), (16384, 10922), (7, 342)):
        for sub in SUBS:
            for restart in (0, 1, 3, 65535):
                assert jpeg.plan(*shape, sub, restart)._asdict() == JC.plan(*shape, sub, restart), (shape, sub, restart)


def test_quant_tables_of_the_library_are_the_statements():
    jpeg = _built()
    for q in range(1, 101):
        lum, chrom = JC.quant_tables(q)
        assert jpeg.quant_tables(q) == (lum.tobytes(), chrom.tobytes()), q


# ------------------------------------------------------------------------------------------ refusals before any launch
A = 1 << 40   # made-up device addresses: validation fails before anything is dereferenced or launched


def test_library_refusals_before_any_launch():
    jpeg = _built()
    L = jpeg.lib()
    err = L.deva_jpeg_last_error
    plan = jpeg.Plan()
    good = dict(plane=A + 3, h=65, w=129, q=75, sub=420, restart=0, scratch=A + (1 << 24), nbytes=1 << 30, out=A + (1 << 26) + 1, cap=4096,
                info=A + (1 << 27), stream=None)
    scan = lambda **o: L.deva_jpeg_scan(*[dict(good, **o)[k] for k in ('plane', 'h', 'w', 'q', 'sub', 'restart', 'scratch', 'nbytes', 'out', 'cap',
                                                                           'info', 'stream')])
    place = lambda **o: L.deva_jpeg_place(*[dict(good, **o)[k] for k in ('h', 'w', 'sub', 'restart', 'scratch', 'nbytes', 'out', 'cap', 'info', 'stream')])
    for over, text in ((dict(h=0), b'bad height x width'), (dict(w=16385), b'bad height x width'), (dict(sub=422), b'subsampling: 420'),
                       (dict(sub=0), b'subsampling: 420'), (dict(restart=-1), b'restart: 0'), (dict(restart=65536), b'restart: 0'),
                       (dict(h=16384, w=16384), b'bytes, a call takes'), (dict(scratch=None), b'scratch: null'),
                       (dict(scratch=A + 8), b'not 16-byte aligned'), (dict(nbytes=100), b'deva_jpeg_plan asks for'), (dict(out=None), b'out: null'),
                       (dict(cap=-1), b'capacity'), (dict(info=None), b'info: null'), (dict(info=A + (1 << 27) + 4), b'info: null or misaligned'),
                       (dict(out=A + (1 << 24) + 100), b'out overlaps scratch'), (dict(info=A + (1 << 24) + 512), b'info overlaps scratch')):
        assert scan(**over) == 2 and text in err(), over
        assert place(**over) == 2 and text in err(), over
    for q in (0, -5, 101):
        assert scan(q=q) == 2 and b'quality: 1 to 100' in err()
    assert scan(plane=None) == 2 and b'plane: null' in err()
    assert scan(plane=A + (1 << 24) + 4096) == 2 and b'plane overlaps scratch' in err()
    assert scan(plane=A + (1 << 26)) == 2 and b'plane overlaps out' in err()
    assert L.deva_jpeg_plan(0, 5, 420, 0, ctypes.byref(plan)) == 2 and b'bad height x width' in err()
    assert L.deva_jpeg_plan(5, 5, 420, 0, None) == 2 and b'null plan' in err()
    assert L.deva_jpeg_limits(None) == 2 and b'null limits' in err()
    assert L.deva_jpeg_quant(75, None) == 2 and b'null tables' in err()


def test_wrapper_refusals_happen_before_any_launch(monkeypatch):
    jpeg = _built()
    for name in ('_launch_scan', '_launch_place'):
        monkeypatch.setattr(jpeg, name, lambda *a: pytest.fail('a launch was reached'))
    plane = torch.zeros(4, 6, 3, dtype=torch.uint8)
    for call in (jpeg.encode, jpeg.scan):
        with pytest.raises(jpeg.DevaHipError, match='plane must be torch.uint8'):
            call(plane.float())
        for bad in (torch.zeros(4, 6, 4, dtype=torch.uint8), torch.zeros(4, 6, dtype=torch.uint8), torch.zeros(6, dtype=torch.uint8)):
            with pytest.raises(jpeg.DevaHipError, match=r'\[H,W,3\] expected'):
                call(bad)
        with pytest.raises(jpeg.DevaHipError, match='plane must be contiguous'):
            call(torch.zeros(6, 4, 3, dtype=torch.uint8).transpose(0, 1))
        with pytest.raises(jpeg.DevaHipError, match='bad height x width'):
            call(torch.zeros(0, 6, 3, dtype=torch.uint8))
        with pytest.raises(jpeg.DevaHipError, match='bad height x width'):
            call(torch.zeros(1, jpeg.MAX_SIDE + 1, 3, dtype=torch.uint8))
        with pytest.raises(jpeg.DevaHipError, match='uint8 tensor'):
            call(np.zeros((4, 6, 3), dtype=np.uint8))
        with pytest.raises(jpeg.DevaHipError, match='capacity must not be negative'):
            call(plane, capacity=-1)
        for quality in (0, 101, -1):
            with pytest.raises(jpeg.DevaHipError, match='quality: 1 to 100'):
                call(plane, quality=quality)
        for sub in ('4:2:2', 420, None, '420'):
            with pytest.raises(jpeg.DevaHipError, match='subsampling'):
                call(plane, subsampling=sub)
        for restart in (-1, 65536):
            with pytest.raises(jpeg.DevaHipError, match='restart: 0'):
                call(plane, restart=restart)
        with pytest.raises(jpeg.DevaHipError, match='are integers'):
            call(plane, quality='high')
    with pytest.raises(jpeg.DevaHipError, match='subsampling'):
        jpeg.plan(4, 4, '4:1:1')
    with pytest.raises(jpeg.DevaHipError, match='quality: 1 to 100'):
        jpeg.file_bytes(b'', 4, 4, quality=0)


def test_host_tensors_are_refused_before_the_library_is_called(monkeypatch):
    """no CPU path: the launcher refuses a host plane itself; the library's entry point is never reached"""
    jpeg = _built()
    handle = jpeg.lib()
    from types import SimpleNamespace
    reached = lambda *a: pytest.fail('a launcher of the library was reached')
    proxy = SimpleNamespace(deva_jpeg_plan=handle.deva_jpeg_plan, deva_jpeg_last_error=handle.deva_jpeg_last_error, deva_jpeg_quant=handle.deva_jpeg_quant,
                            deva_jpeg_scan=reached, deva_jpeg_place=reached)
    monkeypatch.setattr(jpeg, 'lib', lambda: proxy)          # (the plan is host code: sizes alone)
    for call in (jpeg.encode, jpeg.scan):
        for capacity in (None, 100):
            with pytest.raises(jpeg.DevaHipError, match='plane must live on the HIP device'):
                call(torch.zeros(4, 6, 3, dtype=torch.uint8), capacity=capacity)


# ------------------------------------------------------------------------------------------ the sanitizers
def test_plan_code_under_host_sanitizers(tmp_path):
    """csrc/jpeg/jpeg_plan.cpp in a stand-alone program with its own main (tests/jpeg_plan_sanitize_main.cpp); nothing is
    loaded into Python and no GPU is involved"""
    exe = tmp_path / 'jpeg_sanitize'
    subprocess.run([CLANG, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    '-I', os.path.join(ROOT, 'include'), '-I', JPEG_SRC, os.path.join(JPEG_SRC, 'jpeg_plan.cpp'),
                    os.path.join(ROOT, 'tests', 'jpeg_plan_sanitize_main.cpp'), '-o', str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout, run.stderr[-4000:])
    assert run.returncode == 0, run.stderr[-4000:]
    checks, refused, failures = (int(v) for v in re.findall(r'\d+', run.stdout))
    assert checks > 10000 and 0 < refused < checks and failures == 0


# ------------------------------------------------------------------------------------------ static resources
def test_the_plan_is_host_code():
    assert sorted(f for f in os.listdir(JPEG_SRC) if f.endswith('.hip')) == ['jpeg_encode.hip']
    assert sorted(f for f in os.listdir(JPEG_SRC) if f.endswith('.cpp')) == ['jpeg_plan.cpp']
    for name in ('jpeg_plan.cpp', 'jpeg_plan.h'):
        text = open(os.path.join(JPEG_SRC, name)).read()
        assert 'hip/' not in text and '__global__' not in text, name


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not found')
def test_no_kernel_spills_or_uses_scratch():
    """the compiler's own resource report, with the flags of csrc/Makefile: five kernels (the transform in both
    subsamplings), no scratch memory, no spilled register of either kind, and the LDS that deva_jpeg_limits reports"""
    kernels = abi_util.kernel_resources(os.path.join(JPEG_SRC, 'jpeg_encode.hip'))
    assert len(kernels) == 5
    for k in ('transform_kernelILb1', 'transform_kernelILb0', 'interval_kernel', 'offsets_kernel', 'place_kernel'):
        assert sum(k in name for name in kernels) == 1, k
    lds = _built().limits().lds_bytes
    for name, r in kernels.items():
        print(name, r)
        assert r['ScratchSize'] == 0 and r['VGPRs Spill'] == 0 and r['SGPRs Spill'] == 0, (name, r)
        assert r['LDS Size'] <= lds, (name, r)
        assert r['Occupancy'] >= (2 if 'interval_kernel' in name else 8), (name, r)    # (the bit buffer of 256 worst-case blocks: 2 workgroups a CU)


# ------------------------------------------------------------------------------------------ the statement against libjpeg
def _pil_file(image, quality, subsampling, restart):
    """PIL's own file; its `restart_marker_blocks` counts MCUs, and an MCU row when the statement's 0 means one"""
    every = restart if restart else JC.geometry(*image.shape[:2], subsampling, 0)[1]
    buf = io.BytesIO()
    Image.fromarray(image).save(buf, format='JPEG', quality=quality, subsampling=subsampling, restart_marker_blocks=every)
    return buf.getvalue()


def test_statement_dqt_equals_libjpegs_for_every_quality():
    jpeg = _built()
    image = JC.overlay(16, 16, 0)
    for quality in range(1, 101):
        pil = JC.segments(_pil_file(image, quality, '4:2:0', 0))
        lum, chrom = JC.quant_tables(quality)
        assert b''.join(pil[0xDB]) == b'\x00' + lum.tobytes() + b'\x01' + chrom.tobytes(), quality
        mine = JC.segments(jpeg.file_bytes(b'\x00', 16, 16, quality=quality))
        assert [m for m in mine[0xDB]] == [b'\x00' + lum.tobytes(), b'\x01' + chrom.tobytes()], quality


def test_statement_dht_equals_libjpegs_and_the_bindings():
    jpeg = _built()
    pil = JC.segments(_pil_file(JC.overlay(16, 16, 0), 75, '4:2:0', 0))
    tables = {}
    data = b''.join(pil[0xC4])
    while data:                                              # (libjpeg may put several tables into one DHT)
        n = sum(data[1:17])
        tables[data[0]] = data[1:17 + n]
        data = data[17 + n:]
    want = {0x00: JC.DC_LUMINANCE, 0x10: JC.AC_LUMINANCE, 0x01: JC.DC_CHROMINANCE, 0x11: JC.AC_CHROMINANCE}
    assert tables == {k: bytes(counts) + bytes(symbols) for k, (counts, symbols) in want.items()}
    for file in (JC.file_bytes(b'\x00', 16, 16), jpeg.file_bytes(b'\x00', 16, 16)):
        assert {m[0]: m[1:] for m in JC.segments(file)[0xC4]} == tables


def test_the_bindings_file_is_the_statements():
    jpeg = _built()
    for (h, w), quality, sub, restart in (((1, 1), 75, '4:2:0', 0), ((17, 33), 1, '4:4:4', 3), ((120, 214), 100, '4:2:0', 1), ((16, 4000), 50, '4:4:4', 0)):
        data = bytes(range(200))
        assert jpeg.file_bytes(data, h, w, quality=quality, subsampling=sub, restart=restart) == JC.file_bytes(data, h, w, quality, sub, restart)


# ------------------------------------------------------------------------------------------ the statement by hand
def _bytes_of(bits):
    bits += '1' * (-len(bits) % 8)
    return bytes(int(bits[i:i + 8], 2) for i in range(0, len(bits), 8))


def test_statement_by_hand_for_one_pixel():
    """a 1 x 1 pixel of (255, 255, 255): Y = 255, Cb = Cr = 128, padded to one MCU of flat blocks.  A flat block of
    value v has t[r][0] = (8 * 2896 * (v - 128) + 1024) >> 11 and u[0][0] = 8 * 2896 * t; Y: t = 1436, u = 33269248,
    / 2^15 = 1015.3 -> with Q = 8 (quality 75) (u + (8 << 14)) / (8 << 15) = 127.4 -> 127; chroma 0.
    At 4:2:0: Y0 has the DC difference 127 (category 7: code 11110, bits 1111111) and EOB (1010); Y1 .. Y3 have
    difference 0 (00) and EOB; Cb, Cr have 0 (00) and EOB (00).  At 4:4:4 one Y block and the two chroma blocks."""
    white = np.full((1, 1, 3), 255, dtype=np.uint8)
    coef, comp, _ = JC.coefficients(white, 75, '4:2:0')
    assert coef[:, 0].tolist() == [127, 127, 127, 127, 0, 0] and not coef[:, 1:].any() and comp.tolist() == [0, 0, 0, 0, 1, 2]
    bits = '11110' + '1111111' + '1010' + ('00' + '1010') * 3 + ('00' + '00') * 2
    data, info = JC.scan(white, 75, '4:2:0')
    assert data == _bytes_of(bits) and info == [len(data), 6, 0, 1]
    data, info = JC.scan(white, 75, '4:4:4')
    assert data == _bytes_of('11110' + '1111111' + '1010' + '0000' * 2) and info == [len(data), 3, 0, 1]
    # black at quality 100 (Q = 1): t = (8 * 2896 * -128 + 1024) >> 11 = -1448, u = -33547264 -> -(33547264 + 16384) / 32768 = -1024:
    # category 11 (111111110), the extra bits of -1024 are -1024 + 2047 = 1023 = 01111111111
    data, _ = JC.scan(np.zeros((1, 1, 3), dtype=np.uint8), 100, '4:4:4')
    assert data == _bytes_of('111111110' + '01111111111' + '1010' + '0000' * 2).replace(b'\xff', b'\xff\x00')


def test_statement_by_hand_for_one_flat_block_per_interval():
    """8 x 24 at 4:4:4, restart 1: three MCUs of one flat gray each (64, 64, 200), each its own interval, so every DC is
    coded against 0 and a marker FF D0, FF D1 stands between them.  gray v: Y = v, chroma 128.  v = 64: t = (23168 * -64
    + 1024) >> 11 = -724, u = -16773632, Q = 8: -((16773632 + 131072) / 262144) = -64: category 7 (11110), extra bits
    -64 + 127 = 63 = 0111111.  v = 200: t = 814 (1668096 + 1024 >> 11 = 815.0 -> 815), u from the statement's own matrix."""
    image = np.zeros((8, 24, 3), dtype=np.uint8)
    image[:, :16] = 64
    image[:, 16:] = 200
    t = (8 * 2896 * 72 + 1024) >> 11
    level = (8 * 2896 * t + (8 << 14)) // (8 << 15)
    assert (t, level) == (815, 72)
    low = _bytes_of('11110' + '0111111' + '1010' + '0000' * 2)
    high = _bytes_of('11110' + format(72, '07b') + '1010' + '0000' * 2)
    data, info = JC.scan(image, 75, '4:4:4', restart=1)
    assert data == low + b'\xff\xd0' + low + b'\xff\xd1' + high and info == [len(data), 9, 0, 3]
    # in one interval the second block's difference is 0 and the third's 72 + 64 = 136: category 8 (111110), 10001000
    data, info = JC.scan(image, 75, '4:4:4', restart=0)
    one = '11110' + '0111111' + '1010' + '0000' * 2 + '00' + '1010' + '0000' * 2 + '111110' + '10001000' + '1010' + '0000' * 2
    assert data == _bytes_of(one) and info == [len(data), 9, 0, 1]


# ------------------------------------------------------------------------------------------ the statement's files through PIL
SHAPES = [(1, 1), (8, 8)] + [(h, w) for h in (15, 16, 17) for w in (31, 32, 33)] + [(120, 214), (240, 427)]


@functools.lru_cache(maxsize=None)
def _image(shape):
    return JC.overlay(*shape, seed=shape[0] * 1000 + shape[1])


@pytest.mark.parametrize('subsampling', SUBS)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_statement_files_open_in_pil_and_match_pils_own(shape, subsampling):
    """every file opens at the right size and mode; at 120 x 214 and above it is at most 1.10 x PIL's file of the same
    image, quality, subsampling and restart interval, and its PSNR against the source is at most 0.2 dB below PIL's
    (about twice what the numpy prototype measured: sizes -0.5 % .. +5.3 %, PSNR -0.07 .. +0.01 dB; decoded pixels differ
    from PIL's by up to about 20 levels, so pixel equality is not a test)"""
    image = _image(shape)
    for restart in (0, 1, 3):
        for quality in (1, 50, 75, 95, 100):
            file = JC.encode(image, quality, subsampling, restart)
            opened = Image.open(io.BytesIO(file))
            assert opened.size == (shape[1], shape[0]) and opened.mode == 'RGB'
            mine = np.array(opened)                                # (decodes the whole scan: a bad marker or code raises)
            theirs_file = _pil_file(image, quality, subsampling, restart)
            theirs = np.array(Image.open(io.BytesIO(theirs_file)))
            ratio, a, b = len(file) / len(theirs_file), JC.psnr(mine, image), JC.psnr(theirs, image)
            if shape[0] >= 120:
                print(f'{shape} {subsampling} restart={restart} q={quality}: {len(file)} vs {len(theirs_file)} bytes ({ratio:.3f}), {a:.3f} vs {b:.3f} dB')
                assert ratio <= 1.10, (restart, quality, ratio)
                assert a >= b - 0.2, (restart, quality, a, b)
            else:
                assert a >= b - 3.0 or a > 30, (restart, quality, a, b)     # (a few pixels: only that the picture is the picture)


# ------------------------------------------------------------------------------------------ coverage of the code space
def test_the_crafted_image_reaches_the_corners_of_the_code():
    """conditions on the input of the GPU tests: asserted, so that no test passes by leaving them out"""
    image = JC.crafted()
    assert image.shape == (160, 96, 3)
    for subsampling in SUBS:
        data, info, symbols = JC.scan(image, 100, subsampling, 0, detail=True)
        assert int(symbols['dc'].max()) == 11                          # black next to white at Q = 1
        assert int((symbols['ac'] & 15).max()) >= 10                   # the checkerboard's highest frequency
        assert symbols['zrl'] > 0                                      # the one-level checkerboard: only high frequencies survive
        assert symbols['eob'] < symbols['blocks']                      # coefficient 63 is non-zero somewhere
        assert symbols['stuffed'] > 0 and data.count(b'\xff\x00') >= symbols['stuffed']
        assert info[3] > 8 and b'\xff\xd7' in data and data.count(b'\xff\xd0') >= 2     # the restart counter wraps
        assert len(data) <= JC.plan(160, 96, subsampling, 0)['worst_case']
        opened = np.array(Image.open(io.BytesIO(JC.file_bytes(data, 160, 96, 100, subsampling, 0))))
        assert JC.psnr(opened, image) > 35


# ------------------------------------------------------------------------------------------ the saver
@pytest.fixture()
def emu(monkeypatch):
    emu_ops.install(monkeypatch)
    EF.install(monkeypatch)
    EPNG.install(monkeypatch)
    EJPEG.install(monkeypatch)


def _run(root, **modes):
    from deva.inference.frame_results import FrameResultSaver
    from deva.inference.object_info import ObjectInfo
    from deva.inference.object_manager import ObjectManager
    return RC.run_saver(functools.partial(FrameResultSaver, **modes), ObjectManager, ObjectInfo, 'demo', root)[0]


def _files(root):
    return sorted(os.path.relpath(os.path.join(b, f), root) for b, _, fs in os.walk(root) for f in fs)


@pytest.mark.parametrize('png', ['host', 'device'])
def test_device_jpeg_saver_writes_what_the_statement_gives(png, emu, tmp_path, monkeypatch):
    from deva.inference import frame_results
    blends, launch = [], frame_results.launch_frame

    def spy(*a, **k):
        pending = launch(*a, **k)
        blends.append((tuple(k['host']), pending.products.blend.cpu().numpy().copy()))
        return pending
    monkeypatch.setattr(frame_results, 'launch_frame', spy)
    host = _run(str(tmp_path / 'host'), png=png, jpeg='host')
    asked_host = [h for h, _ in blends]
    blends.clear()
    device = _run(str(tmp_path / 'device'), png=png, jpeg='device')
    assert _files(tmp_path / 'host') == _files(tmp_path / 'device') and sum(f.endswith('.jpg') for f in _files(tmp_path / 'device')) == RC.FRAMES
    assert asked_host == [(('color', 'blend') if png == 'host' else ('blend',))] * RC.FRAMES
    assert [h for h, _ in blends] == [(('color',) if png == 'host' else ())] * RC.FRAMES      # the overlay stayed on the device
    for t, (_, blend) in enumerate(blends):
        rel = os.path.join('Visualizations', 'clip', f'{t:05d}.jpg')
        data = open(tmp_path / 'device' / rel, 'rb').read()
        assert data == JC.encode(blend, 75, '4:2:0', 0)
        mine, theirs = np.array(Image.open(io.BytesIO(data))), np.array(Image.open(tmp_path / 'host' / rel))
        assert mine.shape == theirs.shape == blend.shape and JC.psnr(mine, blend) >= JC.psnr(theirs, blend) - 0.2
        rel = os.path.join('Annotations', 'clip', f'{t:05d}.png')
        assert np.array_equal(np.array(Image.open(tmp_path / 'device' / rel)), np.array(Image.open(tmp_path / 'host' / rel)))
    assert host.video_json == device.video_json
    assert device.jpeg_largest > 0 and device.jpeg_capacity == 2 * device.jpeg_largest < device.JPEG_FIRST_CAPACITY
    assert host.jpeg_largest == 0 and host.jpeg_capacity == host.JPEG_FIRST_CAPACITY


def test_the_savers_capacity_adapts_and_an_overflow_is_copied_again(emu, tmp_path, monkeypatch):
    from deva.inference import frame_results
    monkeypatch.setattr(frame_results.FrameResultSaver, 'JPEG_FIRST_CAPACITY', 40)       # below any frame of the clip
    seen = []
    finish = frame_results.jpeg_coder.PendingJpeg.finish

    def spy(self):
        data = finish(self)
        seen.append((self.capacity, self.total, self.overflowed))
        return data
    monkeypatch.setattr(frame_results.jpeg_coder.PendingJpeg, 'finish', spy)
    small = _run(str(tmp_path / 'small'), jpeg='device')
    monkeypatch.setattr(frame_results.FrameResultSaver, 'JPEG_FIRST_CAPACITY', 1 << 20)
    _run(str(tmp_path / 'large'), jpeg='device')
    first, second = seen[:RC.FRAMES], seen[RC.FRAMES:]
    assert first[0][0] == 40 and first[0][2] and all(total > 40 for _, total, _ in first) and len(first) == len(second) == RC.FRAMES
    # (the worker runs behind `save_mask`: a frame is launched with the capacity that the frames finished by then have left)
    prefixes = [2 * max(total for _, total, _ in first[:k]) for k in range(1, RC.FRAMES)]
    assert all(cap in [40] + prefixes[:k + 1] for k, (cap, _, _) in enumerate(first[1:]))
    assert all(over == (total > cap) for cap, total, over in seen)
    assert small.jpeg_capacity == 2 * small.jpeg_largest == 2 * max(total for _, total, _ in first)
    assert not any(over for _, _, over in second)
    for t in range(RC.FRAMES):
        rel = os.path.join('Visualizations', 'clip', f'{t:05d}.jpg')
        assert open(tmp_path / 'small' / rel, 'rb').read() == open(tmp_path / 'large' / rel, 'rb').read()


def test_host_jpeg_makes_exactly_todays_calls(emu, tmp_path, monkeypatch):
    """`jpeg='host'`, and no `jpeg` at all: the coder is never called, `launch_frame` is asked for the same host planes as
    before, `_save_image` gets the same images at the same paths, and the files are PIL's own bytes"""
    from deva.inference import frame_results
    monkeypatch.setattr(frame_results.jpeg_coder, 'encode', lambda *a, **k: pytest.fail('the device coder was called'))
    asked, saved = [], []
    launch, save_image = frame_results.launch_frame, frame_results.FrameResultSaver._save_image

    def spy(*a, **k):
        asked.append((tuple(k['planes']), tuple(k['host'])))
        return launch(*a, **k)

    def save_spy(self, image, where):
        saved.append((os.path.relpath(where, self.output_root), image.mode, np.array(image).copy()))
        return save_image(self, image, where)
    monkeypatch.setattr(frame_results, 'launch_frame', spy)
    monkeypatch.setattr(frame_results.FrameResultSaver, '_save_image', save_spy)
    monkeypatch.setattr(frame_results.FrameResultSaver, '_save_bytes', lambda *a: pytest.fail('bytes were written'))
    calls = {}
    for mode in (None, 'host'):
        asked.clear(), saved.clear()
        _run(str(tmp_path / str(mode)), **({} if mode is None else {'jpeg': mode}))
        assert asked == [(('color', 'blend'), ('color', 'blend'))] * RC.FRAMES
        assert [s[0] for s in saved] == [os.path.join(d, 'clip', f'{t:05d}.{e}') for t in range(RC.FRAMES)
                                         for d, e in (('Annotations', 'png'), ('Visualizations', 'jpg'))]
        calls[mode] = list(saved)
    for a, b in zip(calls[None], calls['host']):
        assert a[:2] == b[:2] and np.array_equal(a[2], b[2])
    for t in range(RC.FRAMES):
        rel = os.path.join('Visualizations', 'clip', f'{t:05d}.jpg')
        data = open(tmp_path / 'None' / rel, 'rb').read()
        assert data == open(tmp_path / 'host' / rel, 'rb').read()
        buf = io.BytesIO()
        Image.fromarray(calls['host'][2 * t + 1][2]).save(buf, format='JPEG')
        assert buf.getvalue() == data                          # PIL's own bytes of the overlay, default settings
    with pytest.raises(ValueError, match="jpeg: 'host' or 'device'"):
        from deva.inference.object_manager import ObjectManager
        frame_results.FrameResultSaver(str(tmp_path), 'clip', dataset='demo', object_manager=ObjectManager(), jpeg='gpu')


def test_other_datasets_ignore_the_option(emu, tmp_path):
    """no overlay, no JPEG: `jpeg='device'` changes nothing for a dataset without `blend`"""
    from deva.inference.frame_results import FrameResultSaver
    from deva.inference.object_info import ObjectInfo
    from deva.inference.object_manager import ObjectManager
    for mode in ('host', 'device'):
        RC.run_saver(functools.partial(FrameResultSaver, jpeg=mode), ObjectManager, ObjectInfo, 'unsup_davis17', str(tmp_path / mode))
    assert _files(tmp_path / 'host') == _files(tmp_path / 'device') and not any(f.endswith('.jpg') for f in _files(tmp_path / 'host'))
    for rel in _files(tmp_path / 'host'):
        assert open(tmp_path / 'host' / rel, 'rb').read() == open(tmp_path / 'device' / rel, 'rb').read()
