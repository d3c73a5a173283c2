"""The run-length text codec without a GPU: libdeva_rle_text.so on its ABI, the refusals of C8 before any launch, the plan and
deva_text_max_chars by hand, the plan's host code under the host sanitizers, the kernels' static resources, the per-value
statement (tests/rle_text_case.py) against the host codec (`coco_strings`, `parse_many`) and the per-value `coco_string` of
tests/emu_frame_result.py, and the public functions with `text='device'` / `parse='device'` on the CPU contract
(tests/emu_rle_text.py) against the host path: results and the text of every error."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import abi_util
import emu_frame_result as EF
import emu_overlap as EO
import emu_rle_text as ET
import emu_runs as ER
import rle_case as LC
import runs_case as RC
import rle_text_case as TC

torch.set_grad_enabled(False)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'deva_rle_text.h')
CSRC = os.path.join(ROOT, 'tracking-anything-with-deva_amd', 'csrc')
TEXT_SRC = os.path.join(CSRC, 'rle_text')
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
CLANG = os.environ.get('DEVA_HOST_CXX', '/opt/rocm/llvm/bin/clang++')
WANT = ['deva_text_encode_count', 'deva_text_encode_write', 'deva_text_last_error', 'deva_text_limits', 'deva_text_max_chars', 'deva_text_parse',
        'deva_text_parse_scratch', 'deva_text_plan', 'deva_text_version']


def _built():
    from deva.hip import rle_text
    return abi_util.built(rle_text)


def _install(monkeypatch):
    ET.install(monkeypatch)
    ER.install(monkeypatch)
    EO.install(monkeypatch)


# ------------------------------------------------------------------------------------------ ABI
def test_exports_header_and_binding_are_one_list():
    rt = _built()
    exported, _ = abi_util.exported(rt.LIB_PATH)
    assert exported == abi_util.declared(HEADER) == sorted(rt.SIGNATURES) == WANT
    header = open(HEADER).read()
    assert re.search(r'#define DEVA_TEXT_ABI_VERSION 1\b', header)
    assert rt.ABI_VERSION == 1 and rt.lib().deva_text_version() == 1
    for name, value in (('MAX_MASKS', rt.MAX_MASKS), ('MAX_WORDS', rt.MAX_WORDS), ('MAX_CHARS', rt.MAX_CHARS), ('SCAN_CHUNK', rt.SCAN_CHUNK),
                        ('MASK_CHUNK', rt.MASK_CHUNK), ('FLAG_CHAR', rt.FLAG_CHAR), ('FLAG_OPEN', rt.FLAG_OPEN), ('FLAG_LONG', rt.FLAG_LONG),
                        ('FLAG_COUNT', rt.FLAG_COUNT), ('FLAG_SUM', rt.FLAG_SUM)):
        assert re.search(rf'#define DEVA_TEXT_{name} {value}\b', header), name
    for rule in ('C1', 'C2', 'C3', 'C4', 'C5', 'C6', 'C7', 'C8'):
        assert re.search(rf'^ \*   {rule}  ', header, flags=re.M), rule
    assert rt.text_limits() == rt.LimitInfo(rt.MAX_MASKS, rt.MAX_WORDS, rt.MAX_CHARS, 256, rt.SCAN_CHUNK, rt.MASK_CHUNK)
    from deva.hip import rle
    assert (rt.MAX_MASKS, rt.MAX_WORDS, rt.MAX_CHARS) == (rle.MAX_MASKS, rle.MAX_WORDS, rle.MAX_CHARS)      # C8: the limits of deva_rle.h
    assert (TC.SCAN_CHUNK, TC.MASK_CHUNK, TC.MAX_CHARS) == (rt.SCAN_CHUNK, rt.MASK_CHUNK, rt.MAX_CHARS)
    assert (TC.FLAG_CHAR, TC.FLAG_OPEN, TC.FLAG_LONG, TC.FLAG_COUNT, TC.FLAG_SUM) == tuple(rt.FLAGS)


def test_no_symbol_is_shared_and_the_other_libraries_have_not_moved():
    from deva import hip
    from deva.hip import mask_runs, metrics, pair_metrics, regions, rle, rle_overlap, vos_metrics
    rt = _built()
    exported, mine = abi_util.exported(rt.LIB_PATH)
    assert all(name.startswith('deva_text_') for name in exported)
    others = (hip, metrics, vos_metrics, pair_metrics, regions, rle, mask_runs, rle_overlap)
    for other in others:
        theirs_exported, theirs = abi_util.exported(abi_util.built(other).LIB_PATH)
        assert not any(n.startswith('deva_text') for n in theirs_exported)
        shared = {s for s in mine & theirs if 'deva' in s}
        assert not shared, (other.LIB_PATH, shared)
    for name in sorted(os.listdir(os.path.join(ROOT, 'include'))):
        if name != 'deva_rle_text.h':
            assert 'deva_text' not in open(os.path.join(ROOT, 'include', name)).read(), name
    abi_util.inference_entry_points([])       # libdeva_hip.so stays at its ABI version
    assert [m.ABI_VERSION for m in others[1:]] == [1] * 7
    assert (len(rle.SIGNATURES), len(mask_runs.SIGNATURES), len(rle_overlap.SIGNATURES)) == (6, 7, 7)


def test_struct_mirrors_have_the_c_layout(tmp_path):
    rt = _built()
    assert [f[0] for f in rt.Plan._fields_] == list(rt.PlanInfo._fields) and [f[0] for f in rt.Limits._fields_] == list(rt.LimitInfo._fields)
    lines = []
    for tag, mirror in (('deva_text_plan', rt.Plan), ('deva_text_limits', rt.Limits)):
        lines.append(f'printf("%zu\\n", sizeof(struct {tag}));\n')
        lines += [f'printf("%zu\\n", offsetof(struct {tag}, {f[0]}));\n' for f in mirror._fields_]
    src = tmp_path / 'probe.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "deva_rle_text.h"\nint main(void){\n' + ''.join(lines) + 'return 0;}\n')
    exe = tmp_path / 'probe'
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    vals = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = []
    for mirror in (rt.Plan, rt.Limits):
        want += [ctypes.sizeof(mirror)] + [getattr(mirror, f[0]).offset for f in mirror._fields_]
    assert vals == want


def test_plan_and_max_chars_by_hand():
    rt = _built()
    assert rt.text_plan(64, (1080, 1920), 800000) == rt.PlanInfo(64, 1, 1, 4, 5, 0, 2 * 64 + 1 + 800000, 512)
    assert rt.text_plan(257, (480, 854)) == rt.PlanInfo(257, 1, 2, 4, 4, 0, 515, 2056)
    assert rt.text_plan(0, (5, 5)) == rt.PlanInfo(0, 0, 0, 4, 2, 0, 1, 0)
    assert rt.text_plan(1, (1, 2**31 - 1)).value_chars == 7
    assert rt.text_plan(1, (4, 4), rt.MAX_WORDS - 3).min_words == rt.MAX_WORDS
    # 5 k bits hold -2^(5k-1) .. 2^(5k-1) - 1, and a difference of two counts within [0, total] lies within [-total, total]
    assert [rt.max_chars(t) for t in (1, 15, 16, 17, 511, 512, 513, 16384, 16385, 480 * 854, 2**19, 2**19 + 1, 1080 * 1920, 2**24 + 1, 2**29 + 1,
                                      2**31 - 1)] == [1, 1, 2, 2, 2, 3, 3, 4, 4, 4, 5, 5, 5, 6, 7, 7]
    for total in (1, 15, 16, 17, 512, 513, 1080 * 1920, 2**31 - 1):
        assert rt.max_chars(total) == TC.max_chars(total)
    assert rt.max_chars(0) == rt.max_chars(2**31) == -1
    assert rt.parse_scratch(3) == 24 and rt.parse_scratch(0) == 0 and rt.parse_scratch(65537) == rt.parse_scratch(-1) == -1
    for bad in ((0, 5), (5, -1), (46341, 46341)):
        with pytest.raises(rt.DevaHipError, match='bad height x width'):
            rt.text_plan(1, bad)
    with pytest.raises(rt.DevaHipError, match='n: 0 to 65536 masks'):
        rt.text_plan(65537, (4, 4))
    with pytest.raises(rt.DevaHipError, match=r'chars_len: 0 to 2\^31 - 1 characters'):
        rt.text_plan(1, (4, 4), 2**31)
    with pytest.raises(rt.DevaHipError, match='need 67108865 words, a call takes 67108864'):
        rt.text_plan(1, (4, 4), rt.MAX_WORDS - 2)
    assert rt.text_chunks([5, 5, 5, 5], 3, 100) == [(0, 3), (3, 4)] and rt.text_chunks([5, 5, 5, 5], 65536, 15) == [(0, 2), (2, 4)]
    assert rt.text_chunks([5, 20], 4, 22) is None and rt.text_chunks([], 4, 22) == [] and rt.text_chunks([19], 4, 22) == [(0, 1)]


# ------------------------------------------------------------------------------------------ C8: refusals before any launch
A = 1 << 40   # made-up device addresses: validation fails before anything is dereferenced or launched
N_IN, BASE, BOUNDS, TEXT_LEN, TEXT_BASE, TEXT_TOTAL, CHARS, TEXT_FIRST, SCRATCH, RUNS, INFO = (A + (k << 24) for k in range(11))
H, W = 7, 5


def _count(L, n_in=N_IN, base=BASE, bounds=BOUNDS, bounds_len=20, n=2, h=H, w=W, text_len=TEXT_LEN, text_base=TEXT_BASE, text_total=TEXT_TOTAL,
           first=None):
    return L.deva_text_encode_count(n_in, base, bounds, bounds_len, n, h, w, text_len, text_base, text_total, first, None)


def _write(L, n_in=N_IN, base=BASE, bounds=BOUNDS, bounds_len=20, n=2, h=H, w=W, text_base=TEXT_BASE, chars=CHARS + 1, capacity=50):
    return L.deva_text_encode_write(n_in, base, bounds, bounds_len, n, h, w, text_base, chars, capacity, None)


def _parse(L, chars=CHARS + 3, chars_len=30, text_first=TEXT_FIRST, n=2, h=H, w=W, scratch=SCRATCH, nbytes=16, runs=RUNS, words_cap=35, info=INFO):
    return L.deva_text_parse(chars, chars_len, text_first, n, h, w, scratch, nbytes, runs, words_cap, info, None)


def test_library_refusals_before_any_launch():
    rt = _built()
    L = rt.lib()
    err = L.deva_text_last_error
    for kw, text in ((dict(n=-1), b'n: 0 to 65536 masks'), (dict(n=65537), b'n: 0 to 65536 masks'), (dict(h=0), b'bad height x width 0 x 5'),
                     (dict(h=46341, w=46341), b'bad height x width'), (dict(bounds_len=-1), b'bounds_len: 0 to 2^60'),
                     (dict(n_in=None), b'n_in: null or misaligned'), (dict(n_in=N_IN + 2), b'n_in: null or misaligned'),
                     (dict(base=None), b'base: null or misaligned'), (dict(base=BASE + 4), b'base: null or misaligned'),
                     (dict(bounds=None), b'bounds: null or misaligned'), (dict(bounds=BOUNDS + 2), b'bounds: null or misaligned'),
                     (dict(text_len=None), b'text_len: null or misaligned'), (dict(text_base=TEXT_BASE + 4), b'text_base: null or misaligned'),
                     (dict(text_total=None), b'text_total: null or misaligned'), (dict(first=TEXT_TOTAL), b'first: it must not be `text_total` itself'),
                     (dict(first=BASE + 4), b'first: misaligned'), (dict(text_len=N_IN + 4), b'text_len overlaps n_in'),
                     (dict(text_base=BASE + 8), b'text_base overlaps base'), (dict(text_total=BOUNDS + 72), b'text_total overlaps bounds'),
                     (dict(text_total=TEXT_BASE + 8), b'overlaps'), (dict(first=TEXT_BASE), b'text_base overlaps first')):
        assert _count(L, **kw) == 2 and text in err() and b'deva_text_encode_count' in err(), (kw, err())
    assert _count(L, n=0, n_in=None, base=None, bounds=None, bounds_len=0, text_len=None, text_base=None, text_total=None) == 0   # no masks: no work
    for kw, text in ((dict(capacity=-1), b'capacity: 0 to 2^60'), (dict(chars=None), b'chars: null'), (dict(text_base=None), b'text_base: null'),
                     (dict(n_in=N_IN + 1), b'n_in: null or misaligned'), (dict(w=0), b'bad height x width'), (dict(n=65537), b'n: 0 to'),
                     (dict(chars=BOUNDS + 79), b'chars overlaps bounds'), (dict(chars=TEXT_BASE + 15), b'chars overlaps text_base'),
                     (dict(chars=N_IN - 49), b'chars overlaps n_in'), (dict(chars=BASE + 1), b'chars overlaps base')):
        assert _write(L, **kw) == 2 and text in err() and b'deva_text_encode_write' in err(), (kw, err())
    assert _write(L, n=0, n_in=None, base=None, bounds=None, bounds_len=0, text_base=None, chars=None, capacity=0) == 0
    for kw, text in ((dict(words_cap=34), b'words_cap: 34 given, 2 masks and 30 characters need 35'), (dict(words_cap=rt.MAX_WORDS + 1), b'words_cap'),
                     (dict(chars_len=2**31), b'chars_len: 0 to 2^31 - 1'), (dict(chars_len=-1), b'chars_len: 0 to'),
                     (dict(chars_len=rt.MAX_WORDS, words_cap=rt.MAX_WORDS), b'words, a call takes 67108864'), (dict(n=65537), b'n: 0 to 65536'),
                     (dict(chars=None), b'chars: null'), (dict(text_first=None), b'text_first: null or misaligned'),
                     (dict(text_first=TEXT_FIRST + 4), b'text_first: null or misaligned'), (dict(scratch=None), b'scratch: null or not 4-byte aligned'),
                     (dict(scratch=SCRATCH + 1), b'scratch: null or not 4-byte aligned'),
                     (dict(nbytes=15), b'scratch_bytes: 15 given, deva_text_parse_scratch asks for 16'), (dict(runs=None), b'runs: null or misaligned'),
                     (dict(runs=RUNS + 2), b'runs: null or misaligned'), (dict(info=None), b'info: null or misaligned'),
                     (dict(info=INFO + 4), b'info: null or misaligned'), (dict(h=-1), b'bad height x width'),
                     (dict(runs=CHARS + 32), b'runs overlaps chars'), (dict(runs=TEXT_FIRST + 20), b'runs overlaps text_first'),
                     (dict(info=RUNS + 136), b'overlaps'), (dict(scratch=RUNS + 136), b'overlaps')):
        assert _parse(L, **kw) == 2 and text in err() and b'deva_text_parse' in err(), (kw, err())
    assert L.deva_text_limits(None) == 2 and b'null limits' in err()
    assert L.deva_text_plan(1, 4, 4, 0, None) == 2 and b'null plan' in err()


def test_wrapper_refusals_happen_before_any_launch(monkeypatch):
    from deva.hip import rle
    rt = _built()
    for name in ('_launch_encode_count', '_launch_encode_write', '_launch_parse'):
        monkeypatch.setattr(rt, name, lambda *a: pytest.fail('a launch was reached'))
    n, base, bounds = torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.int64), torch.zeros(4, dtype=torch.int32)
    with pytest.raises(rt.DevaHipError, match='`n` must be a contiguous torch.int32 vector'):
        rt.encode_text(n.long(), base, bounds, (4, 5))
    with pytest.raises(rt.DevaHipError, match='`base` must be a contiguous torch.int64 vector'):
        rt.encode_text(n, base.int(), bounds, (4, 5))
    with pytest.raises(rt.DevaHipError, match='`bounds` must be a contiguous torch.int32 vector'):
        rt.encode_text(n, base, bounds.view(2, 2), (4, 5))
    with pytest.raises(rt.DevaHipError, match='`base` has 1 entries for 2 masks'):
        rt.encode_text(n, base[:1], bounds, (4, 5))
    with pytest.raises(rt.DevaHipError, match='bad height x width 46341 x 46341'):
        rt.encode_text(n, base, bounds, (46341, 46341))
    with pytest.raises(rt.DevaHipError, match='limit of 1 to 65536 masks'):
        rt.encode_text(n, base, bounds, (4, 5), max_masks=0)
    with pytest.raises(rt.DevaHipError, match='capacity must not be negative'):
        rt.encode_text(n, base, bounds, (4, 5), capacity=-1)
    assert rt.encode_text(n[:0], base[:0], bounds, (4, 5)) == []
    with pytest.raises(rt.DevaHipError, match='a list of bytes expected'):
        rt.parse_text(['04'], (2, 2))
    with pytest.raises(rt.DevaHipError, match='a list of bytes expected'):
        rt.parse_text(b'04', (2, 2))
    with pytest.raises(rt.DevaHipError, match='bad height x width 0 x 2'):
        rt.parse_text([b'04'], (0, 2))
    with pytest.raises(rt.DevaHipError, match='limits of 1 to 65536 masks and 4 to 67108864 words'):
        rt.parse_text([b'04'], (2, 2), max_words=3)
    with pytest.raises(rt.DevaHipError, match='one text alone is above the limit'):
        rt.parse_text([b'04'], (2, 2), max_words=4)
    planes = torch.zeros(2, 4, 5, dtype=torch.uint8)
    from deva.hip import mask_runs
    with pytest.raises(rt.DevaHipError, match=r"text must be one of \('host', 'device'\)"):
        mask_runs.encode(planes, text='gpu')
    with pytest.raises(rt.DevaHipError, match=r"text must be one of \('host', 'device'\)"):
        mask_runs.encode_labels(torch.zeros(4, 5, dtype=torch.int64), [1], text=None)
    for call in (lambda: rle.decode(['04'], source_size=(2, 2), parse='gpu'), lambda: rle.records(['04'], (2, 2), parse='gpu'),
                 lambda: rle.intersections(['04'], ['04'], source_size=(2, 2), parse='gpu'), lambda: rle.iou(['04'], ['04'], source_size=(2, 2), parse=1)):
        with pytest.raises(rt.DevaHipError, match=r"parse must be one of \('host', 'device'\)"):
            call()


def test_host_tensors_are_refused_there_is_no_cpu_path():
    rt = _built()
    n, base, bounds = torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.int64), torch.zeros(4, dtype=torch.int32)
    with pytest.raises(rt.DevaHipError, match='n must live on the HIP device'):
        rt.encode_text(n, base, bounds, (4, 5))
    with pytest.raises(rt.DevaHipError, match='chars must live on the HIP device'):
        rt.parse_text([b'04'], (2, 2), device='cpu')


# ------------------------------------------------------------------------------------------ the sanitizers
def test_plan_code_under_host_sanitizers(tmp_path):
    """csrc/rle_text/rle_text_plan.cpp in a stand-alone program with its own main (tests/rle_text_plan_sanitize_main.cpp);
    nothing is loaded into Python and no GPU is involved"""
    exe = tmp_path / 'rle_text_sanitize'
    subprocess.run([CLANG, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    '-I', os.path.join(ROOT, 'include'), '-I', TEXT_SRC, os.path.join(TEXT_SRC, 'rle_text_plan.cpp'),
                    os.path.join(ROOT, 'tests', 'rle_text_plan_sanitize_main.cpp'), '-o', str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout, run.stderr[-4000:])
    assert run.returncode == 0, run.stderr[-4000:]
    checks, refused, failures = (int(v) for v in re.findall(r'\d+', run.stdout))
    assert checks > 30000 and 0 < refused < checks and failures == 0


# ------------------------------------------------------------------------------------------ static resources
SOURCES = sorted(f for f in os.listdir(TEXT_SRC) if f.endswith('.hip')) if os.path.isdir(TEXT_SRC) else []
KERNELS = {'text_len_kernel': 32, 'text_base_kernel': 32, 'text_write_kernel': 32, 'values_kernel': 20, 'first_kernel': 40, 'starts_kernel': 112}


def test_the_listing_is_not_empty():
    assert SOURCES == ['rle_text.hip']
    assert sorted(f for f in os.listdir(TEXT_SRC) if f.endswith('.cpp')) == ['rle_text_plan.cpp']
    for name in ('rle_text_plan.cpp', 'rle_text_plan.h'):
        text = open(os.path.join(TEXT_SRC, name)).read()
        assert 'hip/' not in text and '__global__' not in text, name        # the plan is host code
    make = open(os.path.join(CSRC, 'Makefile')).read()
    assert 'TEXT_OUT := ../deva/hip/rle_text_lib/libdeva_rle_text.so' in make and '$(eval $(call LIBRARY,TEXT_OUT,rle_text/))' in make
    assert re.search(r'^clean:\n\trm -f .*\$\(TEXT_OUT\)', make, flags=re.M) and re.search(r'^all: .*\$\(TEXT_OUT\)', make, flags=re.M)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not found')
@pytest.mark.parametrize('src', SOURCES)
def test_no_kernel_spills_or_uses_scratch(src):
    kernels = abi_util.kernel_resources(os.path.join(TEXT_SRC, src))
    assert len(kernels) == len(KERNELS)
    for name, r in kernels.items():
        lds = [v for k, v in KERNELS.items() if k in name]
        assert len(lds) == 1, name
        assert r.get('ScratchSize', 0) == 0, (name, r)
        assert r.get('VGPRs Spill', 0) == 0 and r.get('SGPRs Spill', 0) == 0, (name, r)
        assert r.get('LDS Size', 0) == lds[0], (name, r)
        assert r['Occupancy'] >= 4, (name, r)                                # (a workgroup is 4 waves, one per SIMD)


# ------------------------------------------------------------------------------------------ the statement against the host codec
def _all_masks():
    """(counts of every mask, H * W) per group of generated cases"""
    groups = [(TC.edge_masks(), TC.TOP), (TC.few_counts(TC.TOP), TC.TOP), (TC.few_counts(5), 5), (TC.chunk_edge_masks(70000), 70000)]
    for h, w in ((64, 64), (65, 63)):
        groups.append((TC.blob_counts(h, w), h * w))
    return groups


def test_c1_by_hand():
    assert TC.value_chars(0) == b'0' and TC.value_chars(15) == b'?' and TC.value_chars(16) == b'`0' and TC.value_chars(-1) == b'O'
    assert TC.value_chars(-16) == b'@' and TC.value_chars(-17) == b'_O' and TC.value_chars(2**31 - 1) == b'oooooo1'
    assert TC.value_chars(3, 3) == b'SP0' and TC.value_chars(-1, 2) == b'oO' and TC.read_text(b'SP0oO') == ([3, -1], 0)
    assert TC.text_of([4]) == b'4' and TC.text_of([0, 4]) == b'04' and TC.text_of([1, 2, 3, 2, 3]) == b'12300'      # C2: differences from place 3
    assert TC.text_of([5, 6, 7, 1, 9]) == TC.value_chars(5) + TC.value_chars(6) + TC.value_chars(7) + TC.value_chars(-5) + TC.value_chars(2)
    words, flags = TC.run_words([b'04', b'4', b'121'], 4)
    assert flags == 0 and words.tolist() == [0, 3, 5, 9, 0, 0, 4, 0, 4, 0, 1, 3, 4]


def test_the_statement_equals_the_host_codec():
    """tests/rle_text_case.py against `frame_results.coco_strings`, `rle.parse_many` / `parse_checked` / `run_array` and the
    per-value `coco_string` of tests/emu_frame_result.py, on the generated cases"""
    from deva.hip import rle
    from deva.inference.frame_results import coco_strings
    for masks, total in _all_masks():
        texts = [TC.text_of(c) for c in masks]
        flat = np.array([v for c in masks for v in c], dtype=np.int64)
        assert [t.decode() for t in texts] == coco_strings(flat, np.array([len(c) for c in masks]))
        for c, t in zip(masks[:40], texts):
            assert t.decode() == EF.coco_string(c) and EF.coco_parse(t.decode()) == list(c)
            assert TC.read_text(t, total) == (list(c), 0)
        counts, per_mask, _ = rle.parse_many(texts)
        assert counts.tolist() == flat.tolist() and per_mask.tolist() == [len(c) for c in masks]
        n, base, bounds = TC.to_bounds(masks, first=3)
        assert TC.counts_of_bounds(n, base, bounds, total) == [list(c) for c in masks]
        want = TC.encode_statement(n, base, bounds, total, first=11)
        assert want['texts'] == texts and want['text_base'][0] == 11 and want['text_total'] == 11 + sum(len(t) for t in texts)
        assert max(len(TC.value_chars(v)) for c in masks for v in TC._values(c)) <= TC.max_chars(total)
        parsed = rle.parse_checked(texts, (1, total))
        words, flags = TC.run_words(texts, total)
        assert flags == 0 and np.array_equal(words, rle.run_array(parsed, 0, len(texts)))


def test_the_statement_reads_what_the_host_parser_reads():
    from deva.hip import rle
    text, total = TC.every_character_text()
    texts = [text] + TC.padded_texts(total) + [TC.text_of(c) for c in TC.zero_count_masks(total)] + TC.parity_chunk_texts(total)
    texts += TC.straddling_texts(total)
    parsed = rle.parse_checked(texts, (1, total))
    words, flags = TC.run_words(texts, total)
    assert flags == 0 and np.array_equal(words, rle.run_array(parsed, 0, len(texts)))
    assert len({len(t) for t in TC.padded_texts(total)}) == TC.MAX_CHARS and all(TC.read_text(t)[0] == TC.read_text(TC.padded_texts(total)[0])[0]
                                                                     for t in TC.padded_texts(total))
    for t in TC.straddling_texts(total):
        wide = len(t) - TC.MAX_CHARS                              # where the 12-character value begins
        assert wide < TC.SCAN_CHUNK < wide + TC.MAX_CHARS
    assert sorted(TC.SCAN_CHUNK - (len(t) - TC.MAX_CHARS) for t in TC.straddling_texts(total)) == list(range(1, TC.MAX_CHARS))
    # C7: every flag case is an error of the host parser, and a case without a flag is none
    for name, (bad, flag) in TC.flag_cases(total).items():
        assert TC.read_text(bad, total)[1] == flag, name
        with pytest.raises(rle.DevaHipError):
            rle.parse_checked([bad], (1, total))


# ------------------------------------------------------------------------------------------ the public functions on the CPU contract
def test_encode_text_equals_the_statement_and_coco_strings(monkeypatch):
    from deva.inference.frame_results import coco_strings
    rt = _built()
    _install(monkeypatch)
    for masks, total in _all_masks():
        n, base, bounds = (torch.from_numpy(a) for a in TC.to_bounds(masks))
        want = [TC.text_of(c) for c in masks]
        assert rt.encode_text(n, base, bounds, (1, total)) == want
        assert rt.encode_text(n, base, bounds, (1, total), max_masks=7) == want        # chunks fill one `chars`
        flat = np.array([v for c in masks for v in c], dtype=np.int64)
        assert [t.decode() for t in want] == coco_strings(flat, np.array([len(c) for c in masks]))
        exact = sum(len(t) for t in want)
        assert rt.encode_text(n, base, bounds, (1, total), capacity=exact) == want
        with pytest.raises(rt.DevaHipError, match=f'the texts have {exact} characters, the capacity is {exact - 1}'):
            rt.encode_text(n, base, bounds, (1, total), capacity=exact - 1)
        assert exact <= rt.max_chars(total) * (bounds.numel() + len(masks))           # the default capacity always holds


def test_encode_with_text_on_the_device_equals_the_host_path(monkeypatch):
    from deva.hip import mask_runs
    _built()
    _install(monkeypatch)
    for h, w in ((2, 2), (33, 67), (65, 63)):
        names, planes = RC.row_planes(h, w)
        stack = torch.from_numpy(planes.copy())
        for kw in (dict(), dict(form='bytes'), dict(stats=True), dict(max_masks=2), dict(form='counts')):
            assert mask_runs.encode(stack, text='device', **kw) == mask_runs.encode(stack, **kw), (h, w, kw)
        assert mask_runs.encode(stack != 0, text='device') == mask_runs.encode(stack)
        logits = RC.float_stack(h, w, 0.0)[1]
        assert mask_runs.encode(torch.from_numpy(logits), threshold=0.0, text='device') == mask_runs.encode(torch.from_numpy(logits), threshold=0.0)
        total = int(RC.statement(planes)['total'])
        assert mask_runs.encode(stack, capacity=total, text='device').finish() == mask_runs.encode(stack)
        messages = []
        for text in mask_runs.TEXT:
            with pytest.raises(mask_runs.DevaHipError) as e:
                mask_runs.encode(stack, capacity=max(total - 1, 0), text=text).finish()
            messages.append(str(e.value))
        assert messages[0] == messages[1] and 'run boundaries, the capacity is' in messages[0]


def _both(call):
    """the result or the error text of `call(parse=...)` on both paths"""
    from deva.hip import rle
    out = []
    for parse in rle.PARSE:
        try:
            out.append(('ok', call(parse)))
        except rle.DevaHipError as e:
            out.append(('error', str(e)))
    return out


def _same(a, b):
    if isinstance(a, torch.Tensor):
        return torch.equal(a, b)
    if isinstance(a, np.ndarray):
        return np.array_equal(a, b)
    if isinstance(a, tuple):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b


def test_parse_on_the_device_equals_the_host_path_results_and_errors(monkeypatch):
    from deva.hip import rle
    _built()
    _install(monkeypatch)
    h, w = 65, 63
    names, all_counts = LC.row(h, w)
    good = [{'size': [h, w], 'counts': TC.text_of(c).decode()} for c in all_counts]
    mixed = good[:3] + [{'size': [h, w], 'counts': list(all_counts[3])}] + good[4:]
    bare = [TC.text_of(c) for c in all_counts]
    calls = {
        'decode': lambda masks, **kw: lambda parse: rle.decode(masks, device='cpu', parse=parse, **kw),
        'decode-resized': lambda masks, **kw: lambda parse: rle.decode(masks, (40, 50), dtype=torch.float32, device='cpu', parse=parse, **kw),
        'records': lambda masks, **kw: lambda parse: tuple(rle.records(masks, kw.get('source_size'), parse=parse, device='cpu')),
        'intersections': lambda masks, **kw: lambda parse: rle.intersections(masks, masks[:4], device='cpu', parse=parse, **kw),
        'iou': lambda masks, **kw: lambda parse: rle.iou(masks, masks[2:5], [0, 1, 0], device='cpu', parse=parse, **kw),
    }
    seen_device = []
    real_parse = ET._launch_parse
    monkeypatch.setattr(rle.rle_text, '_launch_parse', lambda *a: (seen_device.append(1), real_parse(*a))[1])
    for name, make in calls.items():
        for masks, kw in ((good, {}), (bare, dict(source_size=(h, w))), (mixed, {})):
            before = len(seen_device)
            host, device = _both(make(masks, **kw))
            assert host[0] == device[0] == 'ok' and _same(host[1], device[1]), (name, host, device)
            assert (len(seen_device) > before) == (masks is not mixed), name            # a list of counts: the host path whole
    host, device = _both(lambda parse: rle.decode(good, device='cpu', parse=parse, max_masks=2, max_words=2000))
    assert _same(host[1], device[1])
    # every error: the device flags it, the host parser words it
    total = h * w
    flagged = {name: good[:2] + [{'size': [h, w], 'counts': text}] + good[2:] for name, (text, _) in TC.flag_cases(total).items()}
    flagged['two kinds'] = good[:1] + [dict(good[1], counts=TC.flag_cases(total)['short-sum'][0])] + [dict(good[2], counts=b'\xff')]
    flagged['two kinds, the other way'] = good[:1] + [dict(good[1], counts=TC.flag_cases(total)['open'][0])] + [dict(good[2], counts='4')]
    flagged['negative before a sum'] = [dict(good[0], counts='4'), dict(good[1], counts=TC.flag_cases(total)['negative'][0])]
    flagged['another size'] = good[:2] + [dict(good[2], size=[w, h])]
    flagged['no size'] = bare
    flagged['not a dict'] = good[:1] + [{'counts': '04'}]
    flagged['unicode'] = good[:1] + [dict(good[1], counts='0€')]
    texts = set()
    for name, masks in flagged.items():
        for call in ('decode', 'records', 'intersections'):
            host, device = _both(calls[call](masks))
            assert host[0] == device[0] == 'error' and host[1] == device[1], (name, call, host, device)
            texts.add(host[1].split(':')[-1][:25])
    assert len(texts) >= 9, texts                                                          # the cases do reach different messages


def test_a_flag_the_host_parser_does_not_see_is_reported(monkeypatch):
    from deva.hip import rle
    rt = _built()
    _install(monkeypatch)

    def lying(chars, chars_len, text_first, n, h, w, scratch, runs, words_cap, info):
        info[0], info[1] = rt.FLAG_SUM, 1
    monkeypatch.setattr(rt, '_launch_parse', lying)
    with pytest.raises(rle.DevaHipError, match=r'decode: the device parser flags the texts \(0x10: counts that do not sum to H \* W\) and the host'):
        rle.decode([{'size': [2, 2], 'counts': '04'}], device='cpu', parse='device')
    with pytest.raises(rt.DevaHipError, match='parse_text: counts that do not sum'):
        rt.parse_text([b'04'], (2, 2), device='cpu')
