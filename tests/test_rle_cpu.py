"""The run-length library without a GPU: libdeva_rle.so on its ABI, rule D2 and the argument errors before any launch, the
text parser against the loop form of tests/emu_frame_result.py, the records by hand, the plan's host code and the kernel's
arithmetic under the host sanitizers, the kernels' static resources, the index rule D3 against `F.interpolate` on the CPU,
the numpy statement (tests/rle_case.py) against the per-pixel decoder, and the coverage of the case table the GPU test
runs on."""
import ctypes
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import abi_util
import emu_frame_result as EF
import rle_case as LC

torch.set_grad_enabled(False)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'deva_rle.h')
CSRC = os.path.join(ROOT, 'tracking-anything-with-deva_amd', 'csrc')
RLE_SRC = os.path.join(CSRC, 'rle')
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
CLANG = os.environ.get('DEVA_HOST_CXX', '/opt/rocm/llvm/bin/clang++')
WANT = ['deva_rle_check', 'deva_rle_decode', 'deva_rle_last_error', 'deva_rle_limits', 'deva_rle_plan', 'deva_rle_version']


def _built():
    from deva.hip import rle
    return abi_util.built(rle)


# ------------------------------------------------------------------------------------------ ABI
def test_exports_header_and_binding_are_one_list():
    rl = _built()
    exported, _ = abi_util.exported(rl.LIB_PATH)
    assert exported == abi_util.declared(HEADER) == sorted(rl.SIGNATURES) == WANT
    header = open(HEADER).read()
    assert re.search(r'#define DEVA_RLE_ABI_VERSION 1\b', header)
    assert rl.ABI_VERSION == 1 and rl.lib().deva_rle_version() == 1
    for name, value in (('TILE', rl.TILE), ('MAX_MASKS', rl.MAX_MASKS), ('MAX_WORDS', rl.MAX_WORDS), ('U8', rl.DTYPES[torch.uint8]),
                        ('F32', rl.DTYPES[torch.float32])):
        assert re.search(rf'#define DEVA_RLE_{name} {value}\b', header), name
    for rule in ('D1', 'D2', 'D3', 'D4', 'D5', 'D6'):
        assert re.search(rf'^ \*   {rule}  ', header, flags=re.M), rule
    assert rl.rle_limits() == rl.LimitInfo(rl.MAX_MASKS, rl.MAX_WORDS, rl.TILE, 256)


def test_no_symbol_is_shared_and_the_inference_library_has_not_moved():
    from deva import hip
    from deva.hip import metrics, pair_metrics, regions, vos_metrics
    rl = _built()
    exported, mine = abi_util.exported(rl.LIB_PATH)
    assert all(name.startswith('deva_rle_') for name in exported)
    for other in (hip.LIB_PATH, metrics.LIB_PATH, vos_metrics.LIB_PATH, pair_metrics.LIB_PATH, regions.LIB_PATH):
        theirs_exported, theirs = abi_util.exported(other)
        assert not any(n.startswith('deva_rle') for n in theirs_exported)
        shared = {s for s in mine & theirs if 'deva' in s}
        assert not shared, (other, shared)
    for name in ('deva_hip.h', 'deva_metrics.h', 'deva_vos_metrics.h', 'deva_pair_metrics.h', 'deva_regions.h'):
        assert 'deva_rle' not in open(os.path.join(ROOT, 'include', name)).read(), name
    abi_util.inference_entry_points([])       # libdeva_hip.so stays at its ABI version


def test_struct_mirrors_have_the_c_layout(tmp_path):
    rl = _built()
    assert [f[0] for f in rl.Plan._fields_] == list(rl.PlanInfo._fields) and [f[0] for f in rl.Limits._fields_] == list(rl.LimitInfo._fields)
    lines = []
    for tag, mirror in (('deva_rle_plan', rl.Plan), ('deva_rle_limits', rl.Limits)):
        lines.append(f'printf("%zu\\n", sizeof(struct {tag}));\n')
        lines += [f'printf("%zu\\n", offsetof(struct {tag}, {f[0]}));\n' for f in mirror._fields_]
    src = tmp_path / 'probe.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "deva_rle.h"\nint main(void){\n' + ''.join(lines) + 'return 0;}\n')
    exe = tmp_path / 'probe'
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    vals = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = []
    for mirror in (rl.Plan, rl.Limits):
        want += [ctypes.sizeof(mirror)] + [getattr(mirror, f[0]).offset for f in mirror._fields_]
    assert vals == want


def test_plan_is_host_side():
    rl = _built()
    assert rl.rle_plan(3, (480, 854)) == rl.PlanInfo(14, 8, 3 * 14 * 8, 64 * 80, 1.0, 1.0, 3 * 480 * 854)
    p = rl.rle_plan(64, (1080, 1920), (480, 854), torch.float32)
    assert (p.tiles_x, p.tiles_y, p.grid, p.out_bytes) == (14, 8, 64 * 14 * 8, 4 * 64 * 480 * 854)
    assert p.scale_y == np.float32(1080) / np.float32(480) and p.scale_x == np.float32(1920) / np.float32(854)
    assert rl.rle_plan(1, (1, 1)) == rl.PlanInfo(1, 1, 1, 5120, 1.0, 1.0, 1)
    assert rl.rle_plan(0, (5, 5)).grid == 0
    assert rl.rle_plan(65536, (2160, 3840)).grid == 65536          # capped: the rest is a grid-stride loop
    for bad in ((0, 5), (5, -1), (46341, 46341)):                   # the last: 2^31 pixels and more
        with pytest.raises(rl.DevaHipError, match='bad source size'):
            rl.rle_plan(1, bad)
        with pytest.raises(rl.DevaHipError, match='bad output size'):
            rl.rle_plan(1, (4, 4), bad)
    assert rl.rle_plan(1, (46340, 46341)).tiles_x == 725            # 2^31 - 47 045 pixels: the largest plane there is
    with pytest.raises(rl.DevaHipError, match='0 to 65536 masks'):
        rl.rle_plan(65537, (4, 4))
    with pytest.raises(rl.DevaHipError, match='dtype must be'):
        rl.rle_plan(1, (4, 4), dtype=torch.int32)


# ------------------------------------------------------------------------------------------ D2: refusals before any launch
H, W = 7, 5
GOOD = [3, 4, 5, 20, 3]


def _bad_masks():
    """(what, masks, the text of the refusal): each breaks mask 1 of three"""
    ok = {'size': [H, W], 'counts': EF.coco_string(GOOD)}
    text = EF.coco_string(GOOD)
    return [('a negative count', [ok, {'size': [H, W], 'counts': [3, 4, -1, 26, 3]}, ok], r'mask 1: a count is negative \(-1\)'),
            ('a negative count in a text', [ok, {'size': [H, W], 'counts': EF.coco_string([3, 4, -1, 26, 3])}, ok], r'mask 1: a count is negative'),
            ('a sum one short', [ok, {'size': [H, W], 'counts': [3, 4, 5, 20, 2]}, ok], r'mask 1: the counts sum to 34, H \* W is 35'),
            ('a sum one long', [ok, {'size': [H, W], 'counts': EF.coco_string([3, 4, 5, 20, 4])}, ok], r'mask 1: the counts sum to 36, H \* W is 35'),
            ('no counts', [ok, {'size': [H, W], 'counts': ''}, ok], r'mask 1: the counts sum to 0'),
            ('mixed sizes', [ok, {'size': [W, H], 'counts': GOOD}, ok], r'mask 1: size 5 x 7, the call\'s is 7 x 5 \(one source size per call\)'),
            ('a bad character', [ok, {'size': [H, W], 'counts': text[:2] + 'p' + text[2:]}, ok], r"mask 1: character b'p' is outside '0'\.\.'o'"),
            ('a bad character below', [ok, {'size': [H, W], 'counts': text[:2] + '/' + text[2:]}, ok], r"mask 1: character b'/' is outside"),
            ('a character that is no byte', [ok, {'size': [H, W], 'counts': text + '☃'}, ok], r"mask 1: a character is outside '0'\.\.'o'"),
            ('a truncated text', [ok, {'size': [H, W], 'counts': EF.coco_string([3, 4, 5, 2000, 3])[:-2]}, ok], r'mask 1: the text ends inside a value'),
            ('a value too long', [ok, {'size': [H, W], 'counts': 'o' * 12 + '0'}, ok], r'mask 1: a value of more than 12 characters'),
            ('a dict without a size', [ok, {'counts': GOOD}, ok], r"mask 1: a dict must hold 'size'"),
            ('fractions', [ok, {'size': [H, W], 'counts': [3.5, 31.5]}, ok], r'mask 1: counts must be')]


def test_d2_refusals_happen_before_any_launch(monkeypatch):
    rl = _built()
    monkeypatch.setattr(rl, 'lib', lambda: pytest.fail('the library was reached'))      # (parsing and D2 come first)
    out = torch.full((3, H, W), 7, dtype=torch.uint8)
    for what, masks, text in _bad_masks():
        with pytest.raises(rl.DevaHipError, match=text):
            rl.decode(masks, out=out)
        with pytest.raises(rl.DevaHipError, match=text):
            rl.records(masks)
    assert (out == 7).all()
    with pytest.raises(rl.DevaHipError, match='no mask carries its size'):
        rl.decode([GOOD, EF.coco_string(GOOD)])
    with pytest.raises(rl.DevaHipError, match='a list of masks expected'):
        rl.decode({'size': [H, W], 'counts': GOOD})
    for bad in ((0, 35), (46341, 46341)):
        with pytest.raises(rl.DevaHipError, match='bad source size'):
            rl.decode([[0]], source_size=bad)
    with pytest.raises(rl.DevaHipError, match='dtype must be'):
        rl.decode([GOOD], source_size=(H, W), dtype=torch.int64)


def test_wrapper_errors_before_any_launch():
    rl = _built()
    ok = [{'size': [H, W], 'counts': GOOD}] * 3
    with pytest.raises(rl.DevaHipError, match='bad output size 0 x 4'):
        rl.decode(ok, (0, 4))
    with pytest.raises(rl.DevaHipError, match=r'`out` must be torch.uint8 \[3, 7, 5\]'):
        rl.decode(ok, out=torch.zeros(3, 7, 5))
    with pytest.raises(rl.DevaHipError, match=r'`out` must be torch.float32 \[3, 4, 6\]'):
        rl.decode(ok, (4, 6), dtype=torch.float32, out=torch.zeros(3, 7, 5))
    with pytest.raises(rl.DevaHipError, match='HIP device'):
        rl.decode(ok, out=torch.zeros(3, 7, 5, dtype=torch.uint8))
    with pytest.raises(rl.DevaHipError, match='HIP device'):
        rl.decode(ok, device='cpu')
    for kw in (dict(max_masks=0), dict(max_words=3), dict(max_masks=rl.MAX_MASKS + 1), dict(max_words=rl.MAX_WORDS + 1)):
        with pytest.raises(rl.DevaHipError, match='limits of 1 to 65536 masks and 4 to 67108864 words'):
            rl.decode(ok, **kw)
    with pytest.raises(rl.DevaHipError, match=r'mask 0: 5 runs are above the limit of one call \(7 words\)'):
        rl.decode(ok, max_words=7)


A = 1 << 40   # made-up device addresses: validation fails before anything is dereferenced or launched
RUNS, OUT = A, A + (1 << 34)


def _decode(L, words, n=2, h=H, w=W, oh=H, ow=W, dtype=0, host=True, runs=RUNS, out=OUT, count=None):
    words = np.ascontiguousarray(words, dtype=np.int32)
    return L.deva_rle_decode(words.ctypes.data if host else None, runs, words.size if count is None else count, n, h, w, oh, ow, dtype,
                             out, None)


def test_library_refusals_before_any_launch():
    rl = _built()
    L = rl.lib()
    err = L.deva_rle_last_error
    good = rl.run_array(rl.parse_checked([GOOD, [0, 35]], (H, W)), 0, 2)
    assert good.tolist() == [0, 6, 9, 0, 3, 7, 12, 32, 35, 0, 0, 35]
    assert L.deva_rle_check(good.ctypes.data, good.size, 2, H, W) == 0

    def broken(at, value):
        bad = good.copy()
        bad[at] = value
        return bad
    for words, text in ((broken(5, 2), b'mask 0: count 1 is negative (-1)'), (broken(8, 34), b'mask 0: the counts sum to 34, H * W is 35'),
                        (broken(11, 36), b'mask 1: the counts sum to 36, H * W is 35'), (broken(3, 1), b'mask 0: the first start must be 0'),
                        (broken(1, 9), b'mask 1: no counts'), (broken(1, 13), b'mask 0: its starts end at word 13 of 9'),
                        (broken(2, 8), b'the run array holds 9 starts, the masks take 8'), (broken(0, 1), b'first[0] must be 0')):
        assert _decode(L, words) == 2 and text in err() and b'deva_rle_decode' in err(), (words, err())
        assert L.deva_rle_check(words.ctypes.data, words.size, 2, H, W) == 2 and text in err()
    assert _decode(L, good, count=good.size - 1) == 2 and b'mask 1: its starts end at word 9 of 8' in err()
    assert _decode(L, good, count=rl.MAX_WORDS + 1) == 2 and b'a run array of 3 to 67108864 words' in err()
    assert _decode(L, good, host=False) == 2 and b'null run array' in err()
    assert _decode(L, good, runs=None) == 2 and b'null or misaligned run array on the device' in err()
    assert _decode(L, good, runs=RUNS + 2) == 2 and b'null or misaligned run array on the device' in err()
    assert _decode(L, good, out=None) == 2 and b'null or misaligned out' in err()
    assert _decode(L, good, out=OUT + 2, dtype=1) == 2 and b'null or misaligned out' in err()
    assert _decode(L, good, out=RUNS + 4 * good.size - 1) == 2 and b'out overlaps the run array' in err()
    assert _decode(L, good, runs=OUT + (2 * H * W - 1 & ~3)) == 2 and b'out overlaps the run array' in err()
    for kw, text in ((dict(h=0), b'bad source size'), (dict(oh=0), b'bad output size'), (dict(oh=46341, ow=46341), b'bad output size'),
                     (dict(n=-1), b'0 to 65536 masks'), (dict(n=65537), b'0 to 65536 masks'), (dict(dtype=2), b'dtype must be'),
                     (dict(h=W, w=H + 1), b'mask 0: the counts sum to 35, H * W is 40')):
        assert _decode(L, good, **kw) == 2 and text in err(), kw
    assert _decode(L, good, n=0, host=False, runs=None, out=None, count=0) == 0       # no masks is no work, whatever the pointers
    assert L.deva_rle_limits(None) == 2 and b'null limits' in err()
    assert L.deva_rle_plan(1, 4, 4, 4, 4, 0, None) == 2 and b'null plan' in err()


def test_chunks_stay_within_the_limits_and_cover_every_mask():
    rl = _built()
    rng = np.random.default_rng(3)
    for _ in range(50):
        per = rng.integers(1, 30, int(rng.integers(1, 40)))
        max_masks, max_words = int(rng.integers(1, 9)), int(rng.integers(33, 120))
        parts = rl.chunks(per, max_masks, max_words)
        assert [lo for lo, _ in parts] == [0] + [hi for _, hi in parts[:-1]] and parts[-1][1] == per.size
        for lo, hi in parts:
            words = 2 * (hi - lo) + 1 + int(per[lo:hi].sum())
            assert 1 <= hi - lo <= max_masks and words <= max_words
            if hi < per.size and hi - lo < max_masks:         # greedy: the next mask did not fit
                assert words + int(per[hi]) + 2 > max_words
    assert rl.chunks(np.zeros(0, dtype=np.int64), 4, 100) == []
    # the run array of a chunk is the library's: D2 holds on it, and the words are what `chunks` counted
    names, all_counts = LC.row(33, 67)
    parsed = rl.parse_checked(LC.as_rles(all_counts, 33, 67))
    for lo, hi in rl.chunks(parsed.per_mask, 3, 1 << 20):
        words = rl.run_array(parsed, lo, hi)
        assert words.size == 2 * (hi - lo) + 1 + int(parsed.per_mask[lo:hi].sum())
        assert rl.lib().deva_rle_check(words.ctypes.data, words.size, hi - lo, 33, 67) == 0
        for k in range(lo, hi):
            starts = words[hi - lo + 1 + words[k - lo]:hi - lo + 1 + words[k - lo + 1]]
            assert np.diff(starts).tolist() == list(all_counts[k])


# ------------------------------------------------------------------------------------------ the text
def test_parse_counts_equals_the_loop_form():
    from deva.inference.frame_results import coco_strings
    rl = _built()
    for text, want in (('52203', [5, 2, 2, 2, 5]), ('04', [0, 4]), ('?', [15]), ('', [])):         # the strings of test_frame_result_cpu.py
        assert rl.parse_counts(text).tolist() == EF.coco_parse(text) == want
        assert rl.parse_counts(text.encode()).tolist() == want and rl.parse_counts(text).dtype == np.int64
    for counts in ([2**21, 2**21 - 1, 2**21 + 1, 5, 2**30, 1], [0, 2**31 - 2, 1], [2**25, 3, 2**25, 3, 2**25 - 1, 2, 2**21], [7, 2**40, 1, 0, 2**21]):
        text = EF.coco_string(counts)
        assert rl.parse_counts(text).tolist() == EF.coco_parse(text) == counts
    rng = np.random.default_rng(11)
    sweep = []
    for k in range(300):
        top = (4, 40, 3000, 2**22, 2**31)[k % 5]
        counts = rng.integers(0, top, int(rng.integers(1, 60)))
        counts[rng.random(counts.size) < 0.15] = 0
        sweep.append(counts)
        text = EF.coco_string(counts.tolist())
        assert rl.parse_counts(text).tolist() == EF.coco_parse(text) == counts.tolist()
        assert rl.parse_counts({'size': [1, int(counts.sum()) or 1], 'counts': text}).tolist() == counts.tolist()
    # the product's own encoder, all masks of a call at once, and back in one vectorised pass
    texts = coco_strings(np.concatenate(sweep), [c.size for c in sweep])
    flat, per_mask, sizes = rl.parse_many(texts)
    assert flat.tolist() == np.concatenate(sweep).tolist() and per_mask.tolist() == [c.size for c in sweep] and sizes == [None] * 300
    mixed = [texts[0], sweep[1].tolist(), texts[2].encode(), torch.from_numpy(sweep[3]), {'size': [3, 4], 'counts': texts[4]}, sweep[5]]
    flat, per_mask, sizes = rl.parse_many(mixed)
    assert flat.tolist() == np.concatenate(sweep[:6]).tolist() and sizes == [None] * 4 + [(3, 4), None]
    source = open(rl.__file__).read()
    body = source[source.index('def _decode_texts'):source.index('def _text')]
    loops = [line.split('#')[0].strip() for line in re.findall(r'^\s+for .*$', body, flags=re.M)]
    assert 'while' not in body and loops == ['for place in range(1, int(width.max())):', 'for parity in (0, 1):']   # none over runs or characters


# ------------------------------------------------------------------------------------------ D5
def test_records_by_hand_on_the_2x2_row():
    rl = _built()
    names, all_counts = LC.row(2, 2)
    assert names == ['empty', 'full', 'corners', 'checkerboard', 'column-stripes', 'row-stripes', 'blobs-1', 'blobs-2', 'zero-counts']
    rec = rl.records(LC.as_rles(all_counts, 2, 2))
    by_hand = {'empty': ([4], 0, [-1, -1, -1, -1]), 'full': ([0, 4], 4, [0, 0, 1, 1]), 'corners': ([0, 4], 4, [0, 0, 1, 1]),
               'checkerboard': ([1, 1, 1, 1], 2, [0, 1, 1, 1]),                  # positions 1 and 3: (y, x) = (1, 0) and (1, 1)
               'column-stripes': ([2, 2], 2, [1, 0, 1, 1]), 'row-stripes': ([1, 1, 1, 1], 2, [0, 1, 1, 1]),
               'zero-counts': ([0, 2, 0, 0, 2, 0], 2, [0, 0, 0, 1])}
    for name, (counts, area, box) in by_hand.items():
        k = names.index(name)
        assert list(all_counts[k]) == counts, name
        assert (int(rec.runs[k]), int(rec.area[k]), rec.bbox[k].tolist()) == (len(counts), area, box), name
    # every row against the statement, which reads the decoded planes
    for h, w in LC.GEOMETRIES[:-1]:
        names, all_counts = LC.row(h, w)
        rec = rl.records(LC.as_rles(all_counts, h, w))
        runs, area, bbox = LC.records(all_counts, h, w)
        assert np.array_equal(rec.runs, runs) and np.array_equal(rec.area, area) and np.array_equal(rec.bbox, bbox), (h, w)
    assert rl.records([], (3, 3)).bbox.shape == (0, 4)


# ------------------------------------------------------------------------------------------ the sanitizers
def test_plan_and_walk_code_under_host_sanitizers(tmp_path):
    """csrc/rle/rle_plan.cpp and the kernel's arithmetic (csrc/rle/rle_walk.h) in a stand-alone program with its own main
    (tests/rle_plan_sanitize_main.cpp); nothing is loaded into Python and no GPU is involved"""
    exe = tmp_path / 'rle_sanitize'
    subprocess.run([CLANG, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    '-I', os.path.join(ROOT, 'include'), '-I', RLE_SRC, os.path.join(RLE_SRC, 'rle_plan.cpp'),
                    os.path.join(ROOT, 'tests', 'rle_plan_sanitize_main.cpp'), '-o', str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout, run.stderr[-4000:])
    assert run.returncode == 0, run.stderr[-4000:]
    checks, refused, failures = (int(v) for v in re.findall(r'\d+', run.stdout))
    assert checks > 50000 and 0 < refused < checks and failures == 0


# ------------------------------------------------------------------------------------------ static resources
SOURCES = sorted(f for f in os.listdir(RLE_SRC) if f.endswith('.hip')) if os.path.isdir(RLE_SRC) else []


def test_the_listing_is_not_empty():
    assert SOURCES == ['rle_decode.hip']
    assert sorted(f for f in os.listdir(RLE_SRC) if f.endswith('.cpp')) == ['rle_plan.cpp']
    for name in ('rle_plan.cpp', 'rle_plan.h', 'rle_walk.h'):
        text = open(os.path.join(RLE_SRC, name)).read()
        assert 'hip/' not in text and '__global__' not in text, name        # the plan and the walk are host code too


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not found')
@pytest.mark.parametrize('src', SOURCES)
def test_no_kernel_spills_or_uses_scratch(src):
    kernels = abi_util.kernel_resources(os.path.join(RLE_SRC, src))
    assert len(kernels) == 2 and all('rle_decode_kernel' in name for name in kernels)          # uint8 and float
    for name, r in kernels.items():
        assert r.get('ScratchSize', 0) == 0, (name, r)
        assert r.get('VGPRs Spill', 0) == 0 and r.get('SGPRs Spill', 0) == 0, (name, r)
        assert r.get('LDS Size', 0) == 64 * 80, (name, r)
        assert r['Occupancy'] >= 8, (name, r)


# ------------------------------------------------------------------------------------------ D3
PAIRS = LC.RESIZES + (((33, 67), (33, 67)), ((1080, 1920), (480, 854)), ((720, 1280), (480, 854)), ((7, 5), (70, 131)), ((1, 9), (3, 2)))


def test_the_index_rule_is_interpolate_nearest():
    """D3 against `F.interpolate(mode='nearest')` on the CPU, for the size pairs of the GPU test and the bench: on a plane
    whose value is its position both ways, and on byte and float planes alike"""
    rl = _built()
    for (h, w), (oh, ow) in PAIRS:
        position = torch.arange(h * w, dtype=torch.float32).view(1, 1, h, w)
        want = F.interpolate(position, size=(oh, ow), mode='nearest')[0, 0].long()
        sy, sx = LC.nearest_index(oh, h), LC.nearest_index(ow, w)
        assert np.array_equal((sy[:, None] * w + sx[None, :]), want.numpy()), ((h, w), (oh, ow))
        plan = rl.rle_plan(1, (h, w), (oh, ow))       # the scales the kernel is handed are the statement's
        assert plan.scale_y == np.float32(h) / np.float32(oh) and plan.scale_x == np.float32(w) / np.float32(ow)
        stack = np.stack([LC.blobs(h, w, 5), LC.blobs(h, w, 6)])
        for dtype in (torch.uint8, torch.float32):
            want = F.interpolate(torch.from_numpy(stack).to(dtype)[None], size=(oh, ow), mode='nearest')[0]
            assert np.array_equal(LC.nearest(stack, oh, ow), want.numpy().astype(np.uint8))
    assert np.array_equal(LC.nearest_index(66, 33), np.arange(66) >> 1)


# ------------------------------------------------------------------------------------------ the statement and the table
def test_the_statement_equals_the_per_pixel_decoder():
    for h, w in LC.GEOMETRIES[:-1]:
        names, all_counts = LC.row(h, w)
        for name, counts in zip(names, all_counts):
            slow = EF.coco_decode({'size': [h, w], 'counts': EF.coco_string(counts)})
            assert np.array_equal(LC.plane(counts, h, w), slow.astype(np.uint8)), (h, w, name)
            assert LC.plane(LC.counts_of(slow), h, w).tolist() == slow.astype(np.uint8).tolist()
    # D1 by hand: runs that share a start leave the pixel to the last of them
    assert LC.plane([0, 0, 0, 2, 0, 0, 1, 1], 2, 2).T.reshape(-1).tolist() == [1, 1, 0, 1]
    assert LC.plane([0, 4], 2, 2).all() and not LC.plane([4, 0], 2, 2).any() and not LC.plane([4], 2, 2).any()
    assert LC.plane([1, 2, 3], 2, 3).tolist() == [[0, 1, 0], [1, 0, 0]]


def test_every_geometry_row_holds_every_outcome_it_claims():
    for h, w in LC.GEOMETRIES:
        names, all_counts = LC.row(h, w)
        assert len(set(names)) == len(names)
        assert LC.check_row(h, w) >= LC.claims(h, w), (h, w, LC.claims(h, w) - LC.check_row(h, w))
        by_name = dict(zip(names, all_counts))
        assert list(by_name['full']) == [0, h * w] and list(by_name['empty']) == [h * w]
        assert list(by_name['checkerboard']) == [1] * (h * w) and list(by_name['column-stripes']) == [h] * w
        zeros = list(by_name['zero-counts'])
        assert zeros[0] == 0 and zeros[2:4] == [0, 0] and zeros[-1] == 0
        assert LC.outcomes(zeros, h, w) >= {'zero-first', 'zero-twice-inside', 'zero-last'}
        if min(h, w) >= 33:      # the seeded blobs: two different masks, runs that begin and end anywhere
            one, two = by_name['blobs-1'], by_name['blobs-2']
            assert list(one) != list(two) and min(len(one), len(two)) > 2 * w and not LC.outcomes(one, h, w) and not LC.outcomes(two, h, w)
        if h >= 2 and w >= 4:
            assert 'crosses-columns' in LC.outcomes(by_name['mid-column-run'], h, w)
            assert 'crosses-columns' not in LC.outcomes(by_name['column-stripes'], h, w)
    assert LC.claims(33, 67) == set(LC.OUTCOMES) and 'crosses-columns' not in LC.claims(1, 9) | LC.claims(9, 1) | LC.claims(2, 2)
    assert len(LC.row(480, 854)[1][3]) == 480 * 854             # the most runs a plane can have


# ------------------------------------------------------------------------------------------ host bookkeeping
def test_coco_results_groups_by_image(tmp_path):
    from deva.inference.detections import CocoResults
    seg = {'size': [H, W], 'counts': EF.coco_string(GOOD)}
    entries = [dict(image_id=i, category_id=c, score=s, segmentation=seg) for i, c, s in ((7, 1, 0.9), (3, 2, 0.8), (7, 5, 0.7), (3, 2, 0.6), (9, 4, 0.5))]
    path = tmp_path / 'results.json'
    path.write_text(json.dumps(entries))
    for source in (entries, str(path), path):
        res = CocoResults(source)
        assert len(res) == 3 and res.image_ids() == [7, 3, 9] and 7 in res and 8 not in res
        assert [a['score'] for a in res.annotations(7)] == [0.9, 0.7] and res.annotations(8) == []
        assert [(i, len(a)) for i, a in res] == [(7, 2), (3, 2), (9, 1)]
    with pytest.raises(ValueError, match='entry 1 must hold'):
        CocoResults([entries[0], {'image_id': 3}])
