"""The PNG coder without a GPU: libdeva_png.so on its ABI, the plan by hand, the refusals before any launch, the plan's host
code under the host sanitizers, the kernels' static resources, the numpy statement of rules Z1-Z8 (tests/png_case.py)
against independent decoders (zlib, PIL) and by hand, and `FrameResultSaver(png='device')` on the CPU contracts
(tests/emu_png.py) against `png='host'` on the clip of tests/golden/result_saver.*."""
import ctypes
import functools
import io
import json
import os
import re
import shutil
import subprocess
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

import abi_util
import emu_frame_result as EF
import emu_ops
import emu_png as EPNG
import png_case as PC
import result_case as RC

torch.set_grad_enabled(False)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'deva_png.h')
CSRC = os.path.join(ROOT, 'tracking-anything-with-deva_amd', 'csrc')
PNG_SRC = os.path.join(CSRC, 'png')
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
CLANG = os.environ.get('DEVA_HOST_CXX', '/opt/rocm/llvm/bin/clang++')
WANT = ['deva_png_deflate', 'deva_png_last_error', 'deva_png_limits', 'deva_png_place', 'deva_png_plan', 'deva_png_version']


def _built():
    from deva.hip import png
    return abi_util.built(png)


# ------------------------------------------------------------------------------------------ layout and ABI
def test_exports_header_and_binding_are_one_list():
    png = _built()
    exported, _ = abi_util.exported(png.LIB_PATH)
    assert exported == abi_util.declared(HEADER) == sorted(png.SIGNATURES) == WANT
    header = open(HEADER).read()
    assert re.search(r'#define DEVA_PNG_ABI_VERSION 1\b', header)
    assert png.ABI_VERSION == 1 and png.lib().deva_png_version() == 1
    for name, value in (('MAX_SIDE', png.MAX_SIDE), ('ROWS_PER_SEGMENT', png.ROWS_PER_SEGMENT), ('STEP', png.STEP)):
        assert re.search(rf'#define DEVA_PNG_{name} {value}\b', header), name
    assert re.search(r'#define DEVA_PNG_MAX_BYTES \(1 << 29\)', header) and png.MAX_BYTES == 1 << 29
    for rule in ('Z1', 'Z2', 'Z3', 'Z4', 'Z5', 'Z6', 'Z7', 'Z8'):
        assert re.search(rf'^ \* {rule}\. ', header, flags=re.M), rule
    limits = png.limits()
    assert limits[:5] == (png.MAX_SIDE, png.MAX_BYTES, png.ROWS_PER_SEGMENT, png.STEP, 256) and limits.lds_bytes <= 8192
    assert png.ROWS_PER_SEGMENT == PC.R and png.STEP == PC.STEP
    assert os.path.basename(os.path.dirname(png.LIB_PATH)) == 'png_lib'
    assert {'png_encode.hip', 'png_plan.cpp', 'png_plan.h'} <= set(os.listdir(PNG_SRC))


def test_no_symbol_is_shared_and_the_other_libraries_have_not_moved():
    from deva import hip
    from deva.hip import lowres, mask_runs, metrics, pair_metrics, regions, rle, rle_overlap, rle_text, vos_metrics
    png = _built()
    exported, mine = abi_util.exported(png.LIB_PATH)
    assert all(name.startswith('deva_png_') for name in exported)
    others = (hip, metrics, vos_metrics, pair_metrics, regions, rle, mask_runs, rle_overlap, rle_text, lowres)
    for other in others:
        theirs_exported, theirs = abi_util.exported(abi_util.built(other).LIB_PATH)
        assert not any(n.startswith('deva_png') for n in theirs_exported)
        shared = {s for s in mine & theirs if 'deva' in s}
        assert not shared, (other.LIB_PATH, shared)
    for name in sorted(os.listdir(os.path.join(ROOT, 'include'))):
        if name != 'deva_png.h':
            assert 'deva_png' not in open(os.path.join(ROOT, 'include', name)).read(), name
    abi_util.inference_entry_points([])       # libdeva_hip.so stays at its ABI version
    assert len(hip.SIGNATURES) == 80
    assert [m.ABI_VERSION for m in others[1:]] == [1] * 9
    assert os.path.basename(os.path.dirname(lowres.LIB_PATH)) == 'lowres_lib' and os.path.basename(os.path.dirname(rle_text.LIB_PATH)) == 'rle_text_lib'


def test_struct_mirrors_have_the_c_layout(tmp_path):
    png = _built()
    assert [f[0] for f in png.Plan._fields_ if f[0] != 'reserved'] == list(png.PlanInfo._fields)
    assert [f[0] for f in png.Limits._fields_] == list(png.LimitInfo._fields)
    mirrors = (('deva_png_plan', png.Plan), ('deva_png_limits', png.Limits))
    lines = []
    for tag, mirror in mirrors:
        lines.append(f'printf("%zu\\n", sizeof(struct {tag}));\n')
        lines += [f'printf("%zu\\n", offsetof(struct {tag}, {f[0]}));\n' for f in mirror._fields_]
    src = tmp_path / 'probe.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "deva_png.h"\nint main(void){\n' + ''.join(lines) + 'return 0;}\n')
    exe = tmp_path / 'probe'
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    vals = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = []
    for _, mirror in mirrors:
        want += [ctypes.sizeof(mirror)] + [getattr(mirror, f[0]).offset for f in mirror._fields_]
    assert vals == want


# ------------------------------------------------------------------------------------------ the plan by hand
def test_plan_by_hand():
    png = _built()
    # 1080p gray: 135 segments of 8 rows of 1921 bytes.  A segment at 9 bits a byte: 3 + 9 * 15368 + 7 + 3 = 138325 bits ->
    # 17291 bytes + 4 = 17295 -> a slot of 17296.  Scratch: three tables of 8 * 135 = 1080 -> 1280 bytes, the slots
    # 135 * 17296 = 2334960 -> 2334976 (9121 * 256).  Worst case: 2 + 135 * 17295 + 6.
    assert png.plan(1080, 1920, 1) == png.PlanInfo(8, 135, 1920, 2, 256, 17296, 3 * 1280 + 2334976, 2 + 135 * 17295 + 6)
    # 480 x 854 RGB: 60 segments, rows of 2563 bytes in 3 steps
    p = png.plan(480, 854, 3)
    assert (p.rows_per_segment, p.segments, p.row_bytes, p.steps_per_row) == (8, 60, 2562, 3)
    # one pixel: one segment of one row of 2 bytes: 3 + 18 + 7 + 3 = 31 bits -> 4 + 4 bytes; the slot is sized for 8 rows
    p = png.plan(1, 1, 1)
    assert (p.segments, p.worst_case, p.slot_bytes) == (1, 2 + 8 + 6, 32)
    # a short last segment: 17 rows = 8 + 8 + 1
    p = png.plan(17, 5, 1)
    assert p.segments == 3 and p.worst_case == 2 + 2 * ((3 + 9 * 48 + 10 + 7) // 8 + 4) + ((3 + 9 * 6 + 10 + 7) // 8 + 4) + 6
    for shape in ((1, 1, 1), (9, 1023, 1), (9, 1024, 1), (2160, 3840, 3), (16384, 16384, 1), (7, 342, 3)):
        assert png.plan(*shape)._asdict() == PC.plan(*shape), shape
    assert png.plan(2160, 3840, 3).steps_per_row == 12


# ------------------------------------------------------------------------------------------ refusals before any launch
A = 1 << 40   # made-up device addresses: validation fails before anything is dereferenced or launched


def test_library_refusals_before_any_launch():
    png = _built()
    L = png.lib()
    err = L.deva_png_last_error
    plan = png.Plan()
    good = dict(plane=A + 3, h=65, w=129, bpp=3, scratch=A + (1 << 24), nbytes=1 << 30, out=A + (1 << 26) + 1, cap=4096, info=A + (1 << 27),
                stream=None)
    deflate = lambda **o: L.deva_png_deflate(*[dict(good, **o)[k] for k in ('plane', 'h', 'w', 'bpp', 'scratch', 'nbytes', 'out', 'cap', 'info', 'stream')])
    place = lambda **o: L.deva_png_place(*[dict(good, **o)[k] for k in ('h', 'w', 'bpp', 'scratch', 'nbytes', 'out', 'cap', 'info', 'stream')])
    for over, text in ((dict(h=0), b'bad height x width'), (dict(w=16385), b'bad height x width'), (dict(bpp=2), b'bpp: 1'), (dict(bpp=4), b'bpp: 1'),
                       (dict(h=16384, w=16384), b'bytes, a call takes'), (dict(scratch=None), b'scratch: null'),
                       (dict(scratch=A + 8), b'not 16-byte aligned'), (dict(nbytes=100), b'deva_png_plan asks for'), (dict(out=None), b'out: null'),
                       (dict(cap=-1), b'capacity'), (dict(info=None), b'info: null'), (dict(info=A + (1 << 27) + 4), b'info: null or misaligned'),
                       (dict(out=A + (1 << 24) + 100), b'out overlaps scratch'), (dict(info=A + (1 << 24) + 512), b'info overlaps scratch')):
        assert deflate(**over) == 2 and text in err(), over
        assert place(**over) == 2 and text in err(), over
    assert deflate(plane=None) == 2 and b'plane: null' in err()
    assert deflate(plane=A + (1 << 24) + 4096) == 2 and b'plane overlaps scratch' in err()
    assert deflate(plane=A + (1 << 26)) == 2 and b'plane overlaps out' in err()
    assert L.deva_png_plan(0, 5, 1, ctypes.byref(plan)) == 2 and b'bad height x width' in err()
    assert L.deva_png_plan(5, 5, 1, None) == 2 and b'null plan' in err()
    assert L.deva_png_limits(None) == 2 and b'null limits' in err()


def test_wrapper_refusals_happen_before_any_launch(monkeypatch):
    png = _built()
    for name in ('_launch_deflate', '_launch_place'):
        monkeypatch.setattr(png, name, lambda *a: pytest.fail('a launch was reached'))
    plane = torch.zeros(4, 6, dtype=torch.uint8)
    for call in (png.encode, png.deflate):
        with pytest.raises(png.DevaHipError, match='plane must be torch.uint8'):
            call(plane.float())
        with pytest.raises(png.DevaHipError, match=r'\[H,W\] or \[H,W,3\] expected'):
            call(torch.zeros(4, 6, 4, dtype=torch.uint8))
        with pytest.raises(png.DevaHipError, match=r'\[H,W\] or \[H,W,3\] expected'):
            call(torch.zeros(6, dtype=torch.uint8))
        with pytest.raises(png.DevaHipError, match='plane must be contiguous'):
            call(torch.zeros(6, 4, dtype=torch.uint8).t())
        with pytest.raises(png.DevaHipError, match='bad height x width'):
            call(torch.zeros(0, 6, dtype=torch.uint8))
        with pytest.raises(png.DevaHipError, match='uint8 tensor'):
            call(np.zeros((4, 6), dtype=np.uint8))
        with pytest.raises(png.DevaHipError, match='capacity must not be negative'):
            call(plane, capacity=-1)
    for palette, text in ((bytes(769), '768 bytes at most'), (bytes(771), '768 bytes at most'), (bytes(10), 'RGB triples'), (b'', 'RGB triples'),
                          ([0, 1], 'RGB triples'), (object(), 'palette')):
        with pytest.raises(png.DevaHipError, match=text):
            png.encode(plane, palette=palette)
    with pytest.raises(png.DevaHipError, match=r'a palette belongs to an \[H,W\] plane'):
        png.encode(torch.zeros(4, 6, 3, dtype=torch.uint8), palette=bytes(768))
    with pytest.raises(png.DevaHipError, match='bpp: 1'):
        png.plan(4, 4, 2)


def test_host_tensors_are_refused_before_the_library_is_called(monkeypatch):
    """no CPU path: the launcher refuses a host plane itself; the library's entry point is never reached"""
    png = _built()
    handle = png.lib()
    from types import SimpleNamespace
    reached = lambda *a: pytest.fail('a launcher of the library was reached')
    proxy = SimpleNamespace(deva_png_plan=handle.deva_png_plan, deva_png_last_error=handle.deva_png_last_error, deva_png_deflate=reached,
                            deva_png_place=reached)
    monkeypatch.setattr(png, 'lib', lambda: proxy)          # (the plan is host code: sizes alone)
    for call in (png.encode, png.deflate):
        for capacity in (None, 100):
            with pytest.raises(png.DevaHipError, match='plane must live on the HIP device'):
                call(torch.zeros(4, 6, dtype=torch.uint8), capacity=capacity)


# ------------------------------------------------------------------------------------------ the sanitizers
def test_plan_code_under_host_sanitizers(tmp_path):
    """csrc/png/png_plan.cpp in a stand-alone program with its own main (tests/png_plan_sanitize_main.cpp); nothing is
    loaded into Python and no GPU is involved"""
    exe = tmp_path / 'png_sanitize'
    subprocess.run([CLANG, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    '-I', os.path.join(ROOT, 'include'), '-I', PNG_SRC, os.path.join(PNG_SRC, 'png_plan.cpp'),
                    os.path.join(ROOT, 'tests', 'png_plan_sanitize_main.cpp'), '-o', str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout, run.stderr[-4000:])
    assert run.returncode == 0, run.stderr[-4000:]
    checks, refused, failures = (int(v) for v in re.findall(r'\d+', run.stdout))
    assert checks > 10000 and 0 < refused < checks and failures == 0


# ------------------------------------------------------------------------------------------ static resources
def test_the_plan_is_host_code():
    assert sorted(f for f in os.listdir(PNG_SRC) if f.endswith('.hip')) == ['png_encode.hip']
    assert sorted(f for f in os.listdir(PNG_SRC) if f.endswith('.cpp')) == ['png_plan.cpp']
    for name in ('png_plan.cpp', 'png_plan.h'):
        text = open(os.path.join(PNG_SRC, name)).read()
        assert 'hip/' not in text and '__global__' not in text, name


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not found')
def test_no_kernel_spills_or_uses_scratch():
    """the compiler's own resource report, with the flags of csrc/Makefile: three kernels, no scratch memory, no spilled
    register of either kind, and the LDS that deva_png_limits reports"""
    kernels = abi_util.kernel_resources(os.path.join(PNG_SRC, 'png_encode.hip'))
    assert len(kernels) == 3 and all(any(k in name for name in kernels) for k in ('segment_kernel', 'offsets_kernel', 'place_kernel'))
    lds = _built().limits().lds_bytes
    for name, r in kernels.items():
        print(name, r)
        assert r['ScratchSize'] == 0 and r['VGPRs Spill'] == 0 and r['SGPRs Spill'] == 0, (name, r)
        assert r['LDS Size'] <= lds, (name, r)
        assert r['Occupancy'] >= 4, (name, r)


# ------------------------------------------------------------------------------------------ the statement
def test_statement_by_hand_for_one_pixel():
    """a 1 x 1 plane of 0: the row string 02 00.  Bits, first to last: 0 10 (BFINAL, BTYPE = 01 LSB first), literal 2 =
    0011 0010, literal 0 = 0011 0000, end-of-block 0000000, the stored block's 000 -> 29 bits:
        0100 0110 | 0100 0110 | 0000 0000 | 0000 0...  LSB first per byte = 62 62 00 00, then 00 00 FF FF.
    Adler-32 of 02 00: a = 1 + 2 = 3, b = 3 + 3 = 6."""
    data, info = PC.stream(np.zeros((1, 1), dtype=np.uint8))
    assert data.hex() == '7801' + '62620000' + '0000ffff' + '0300' + '00060003'
    assert info == [16, 0x00060003, 0, 1]


def test_statement_by_hand_for_two_rows_of_five():
    """rows 0 1 2 3 4 and 5 6 7 8 9: row strings 02 00 01 02 03 04 and 02 05 05 05 05 05 (`Up`): the second row is the
    literal 2, the literal 5 and one match of length 4 at distance 1 (symbol 258: 0000010, then 00000).  Hand-packed bit
    string, in stream order: header 010; literals 0x32 0x30 0x31 0x32 0x33 0x34; 0x32 0x35; 0000010 00000; 0000000; 000"""
    plane = np.arange(10, dtype=np.uint8).reshape(2, 5)
    bits = '010' + ''.join(format(0x30 + b, '08b') for b in (2, 0, 1, 2, 3, 4, 2, 5)) + '0000010' + '00000' + '0000000' + '000'
    bits += '0' * (-len(bits) % 8)
    body = bytes(int(bits[i:i + 8][::-1], 2) for i in range(0, len(bits), 8))
    strings = bytes([2, 0, 1, 2, 3, 4, 2, 5, 5, 5, 5, 5])
    a = b = 0
    a = 1
    for v in strings:
        a = (a + v) % 65521
        b = (b + a) % 65521
    data, info = PC.stream(plane)
    assert data == b'\x78\x01' + body + b'\x00\x00\xff\xff' + b'\x03\x00' + bytes([b >> 8, b & 255, a >> 8, a & 255])
    assert info == [len(data), b << 16 | a, 0, 1] and zlib.decompress(data) == strings


CASES = [(1, 1), (1, 9), (2, 5), (7, 37), (8, 37), (9, 37), (17, 37), (3, 1023), (3, 1024), (3, 341, 3), (3, 342, 3), (64, 300)]


@pytest.mark.parametrize('shape', CASES)
def test_statement_against_zlib_and_pil(shape):
    rng = np.random.default_rng(sum(shape))
    few = np.array([0, 0, 0, 2, 143, 144, 255], dtype=np.uint8)
    bpp = 3 if len(shape) == 3 else 1
    for plane in (rng.integers(0, 256, shape).astype(np.uint8), few[rng.integers(0, len(few), shape)], np.zeros(shape, dtype=np.uint8),
                  np.full(shape, 2, dtype=np.uint8)):
        strings = PC.row_strings(plane).tobytes()
        data, info = PC.stream(plane)
        assert zlib.decompress(data) == strings                      # (zlib verifies the Adler-32 itself)
        assert info == [len(data), zlib.adler32(strings), 0, -(-shape[0] // PC.R)] and len(data) == PC.stream_size(plane)
        assert len(data) <= PC.plan(shape[0], shape[1], bpp)['worst_case']
        from deva.hip import png
        image = Image.open(io.BytesIO(png.file_bytes(data, shape[0], shape[1], bpp)))
        assert image.mode == ('RGB' if bpp == 3 else 'L') and np.array_equal(np.array(image), plane)
        if bpp == 1:
            palette = bytes(rng.integers(0, 256, 3 * 200).astype(np.uint8))
            image = Image.open(io.BytesIO(png.file_bytes(data, shape[0], shape[1], 1, palette)))
            assert image.mode == 'P' and np.array_equal(np.array(image), plane) and bytes(image.getpalette()[:600]) == palette


def test_statement_runs_and_tokens():
    """Z3 on one row: a run of 2 is two literals, of 3 three, of 4 a literal and a match of 3, of 259 a literal and a full
    match, of 260 one literal more, of 262 a match of 3 after the full one; the filter byte joins a leading 2"""
    row = np.concatenate([[2, 2], [7] * 2, [9] * 3, [7] * 4, [1] * 259, [0] * 260, [200] * 262]).astype(np.uint8)
    plane = row[None, :]
    values, lengths, _ = PC.runs(PC.row_strings(plane))
    assert values.tolist() == [2, 7, 9, 7, 1, 0, 200] and lengths.tolist() == [3, 2, 3, 4, 259, 260, 262]
    _, bits = PC.tokens(values, lengths)
    assert bits.tolist() == [8] * 3 + [8] * 2 + [8] * 3 + [8, 12] + [8, 13] + [8, 13, 8] + [9, 13, 12]
    assert PC.run_bit_counts(values, lengths).tolist() == [24, 16, 24, 20, 21, 29, 34]
    assert [int(PC.MATCH_BITS[m]) for m in (3, 10, 11, 18, 19, 114, 115, 130, 131, 257, 258)] == [12, 12, 13, 13, 14, 16, 17, 17, 18, 18, 13]


def test_blob_maps_are_what_the_gpu_tests_expect():
    plane = PC.blobs(135, 240, objects=14, seed=1080)
    assert plane.dtype == np.uint8 and plane.shape == (135, 240) and len(np.unique(plane)) >= 10
    rgb = PC.blobs(135, 240, objects=14, seed=1080, rgb=True)
    assert rgb.shape == (135, 240, 3) and len(np.unique(rgb.reshape(-1, 3), axis=0)) == len(np.unique(plane))
    assert zlib.decompress(PC.stream(rgb)[0]) == PC.row_strings(rgb).tobytes()


# ------------------------------------------------------------------------------------------ the saver
@pytest.fixture()
def emu(monkeypatch):
    emu_ops.install(monkeypatch)
    EF.install(monkeypatch)
    EPNG.install(monkeypatch)


SAVER_CASES = dict(RC.DATASETS, burst=RC.BURST, ref_davis=(False, [(1, None, None), (2, None, None), (3, None, None)], False))


def _run(dataset, root, mode, hooks, monkeypatch=None):
    from deva.inference.frame_results import FrameResultSaver
    from deva.inference.object_info import ObjectInfo
    from deva.inference.object_manager import ObjectManager

    def hook(name, result, annotation):
        hooks.append((name, sorted(result.host), result.index.clone(), result.channel_ids.copy(), json.dumps(annotation, sort_keys=True),
                      [dict(s) for s in result.segments]))
    make = functools.partial(FrameResultSaver, frame_hook=hook, **({} if mode is None else {'png': mode}))
    return RC.run_saver(make, ObjectManager, ObjectInfo, dataset, root, SAVER_CASES[dataset])


@pytest.mark.parametrize('dataset', sorted(SAVER_CASES))
def test_device_png_saver_equals_the_host_png_saver(dataset, emu, tmp_path):
    hooks = {'host': [], 'device': []}
    savers = {mode: _run(dataset, str(tmp_path / mode), mode, hooks[mode])[0] for mode in ('host', 'device')}
    files = lambda mode: sorted(os.path.relpath(os.path.join(b, f), tmp_path / mode) for b, _, fs in os.walk(tmp_path / mode) for f in fs)
    assert files('host') == files('device') and sum(f.endswith('.png') for f in files('host')) == RC.FRAMES
    long_id = SAVER_CASES[dataset][0]
    for rel in files('host'):
        a, b = Image.open(tmp_path / 'host' / rel), Image.open(tmp_path / 'device' / rel)
        assert a.mode == b.mode and a.size == b.size, rel
        if rel.endswith('.png'):
            assert a.mode == ('RGB' if long_id else 'P') and np.array_equal(np.array(a), np.array(b)), rel
            assert len(np.unique(np.array(b))) > 2
            if not long_id:
                assert a.getpalette() == b.getpalette() and bytes(b.getpalette()) == RC.palette()
        else:
            assert np.array_equal(np.array(a), np.array(b)), rel      # (the same PIL wrote both JPEGs from the same overlay)
    assert getattr(savers['host'], 'video_json', None) == getattr(savers['device'], 'video_json', None)
    assert len(hooks['host']) == len(hooks['device']) == RC.FRAMES
    for (name_a, host_a, index_a, ids_a, ann_a, seg_a), (name_b, host_b, index_b, ids_b, ann_b, seg_b) in zip(hooks['host'], hooks['device']):
        assert name_a == name_b and ann_a == ann_b and seg_a == seg_b and torch.equal(index_a, index_b) and np.array_equal(ids_a, ids_b)
        assert [k for k in host_a if k == 'blend'] == host_b and len(host_a) == len(host_b) + 1    # the PNG's plane stayed on the device
    device = savers['device']
    assert device.png_largest > 0 and device.png_capacity == 2 * device.png_largest < device.PNG_FIRST_CAPACITY


def test_the_savers_capacity_adapts_and_an_overflow_is_copied_again(emu, tmp_path, monkeypatch):
    from deva.inference import frame_results
    monkeypatch.setattr(frame_results.FrameResultSaver, 'PNG_FIRST_CAPACITY', 40)       # below any stream of the clip
    seen = []
    finish = frame_results.png_coder.PendingPng.finish

    def spy(self):
        data = finish(self)
        seen.append((self.capacity, self.total, self.overflowed))
        return data
    monkeypatch.setattr(frame_results.png_coder.PendingPng, 'finish', spy)
    _run('unsup_davis17', str(tmp_path / 'device'), 'device', [])
    _run('unsup_davis17', str(tmp_path / 'host'), 'host', [])
    assert seen[0][0] == 40 and seen[0][2] and all(total > 40 for _, total, _ in seen) and len(seen) == RC.FRAMES
    assert any(not over for _, _, over in seen[1:])                                      # twice the largest seen is enough later on
    for t in range(RC.FRAMES):
        rel = os.path.join('clip', f'{t:05d}.png')
        assert np.array_equal(np.array(Image.open(tmp_path / 'device' / rel)), np.array(Image.open(tmp_path / 'host' / rel)))


def test_host_png_makes_exactly_todays_calls(emu, tmp_path, monkeypatch):
    """`png='host'`, and no `png` at all: the coder is never called, `launch_frame` is asked for the same host planes as
    before, and the files are PIL's own bytes"""
    from deva.inference import frame_results
    monkeypatch.setattr(frame_results.png_coder, 'encode', lambda *a, **k: pytest.fail('the device coder was called'))
    asked = []
    launch = frame_results.launch_frame

    def spy(*a, **k):
        asked.append((tuple(k['planes']), tuple(k['host'])))
        return launch(*a, **k)
    monkeypatch.setattr(frame_results, 'launch_frame', spy)
    for mode in (None, 'host'):
        asked.clear()
        _run('demo', str(tmp_path / str(mode)), mode, [])
        assert asked == [(('color', 'blend'), ('color', 'blend'))] * RC.FRAMES
    for t in range(RC.FRAMES):
        rel = os.path.join('Annotations', 'clip', f'{t:05d}.png')
        data = open(tmp_path / 'None' / rel, 'rb').read()
        assert data == open(tmp_path / 'host' / rel, 'rb').read()
        buf = io.BytesIO()
        Image.open(io.BytesIO(data)).save(buf, format='PNG')
        assert buf.getvalue() == data
    with pytest.raises(ValueError, match="png: 'host' or 'device'"):
        from deva.inference.object_manager import ObjectManager
        frame_results.FrameResultSaver(str(tmp_path), 'clip', dataset='demo', object_manager=ObjectManager(), png='gpu')
