"""libdeva_rle_text.so on the device against the per-value statement of tests/rle_text_case.py and against the host codec
(`frame_results.coco_strings`, `rle.parse_checked` / `run_array`): exact equality, bytes and words.  The encoder takes
`n` / `base` / `bounds` / H * W directly, so large counts need no large plane; the parser takes bytes.  Every case is the
smallest at which its path can still go wrong: both sides of every width edge, masks of 1 to 5 counts, count and character
totals around the steps of the per-mask walk, mask numbers around the steps of the cross-mask scan, capacities around the
exact one, values across the boundary between two steps, one input per flag; sentinel margins around every output.

With DEVA_TEST_DRYRUN=1 the same code runs on the CPU contract of tests/emu_rle_text.py."""
import os

import numpy as np
import pytest
import torch

import emu_overlap as EO
import emu_rle_text as ET
import emu_runs as ER
import gpu_util
import rle_case as LC
import runs_case as RC
import rle_text_case as TC
from deva.hip import mask_runs, rle, rle_text
from deva.inference.frame_results import coco_strings

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DRYRUN = os.environ.get('DEVA_TEST_DRYRUN') == '1'
MARGIN = 64
CHAR_SENTINEL, WORD_SENTINEL = 0xA5, -7777777


@pytest.fixture(autouse=True)
def _emulated_when_dry(monkeypatch):
    if DRYRUN:
        ET.install(monkeypatch)
        ER.install(monkeypatch)
        EO.install(monkeypatch)


def _dev(a):
    return (torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a).to(gpu_util.dev())


# ------------------------------------------------------------------------------------------ the encoder, call by call
def _raw_encode(masks, total, capacity=None, first=None):
    """deva_text_encode_count and _write on `masks` (lists of counts) -> (text_len, text_base, text_total, chars with its
    margin, the statement); `chars` is `capacity` characters (default: exact) and MARGIN sentinels behind them"""
    n, base, bounds = TC.to_bounds(masks)
    want = TC.encode_statement(n, base, bounds, total, 0 if first is None else first)
    capacity = want['text_total'] if capacity is None else capacity
    n_d, base_d, bounds_d = _dev(n), _dev(base), _dev(bounds)
    text_len = _dev(torch.full((len(masks),), -1, dtype=torch.int32))
    text_base = _dev(torch.full((len(masks),), -1, dtype=torch.int64))
    text_total = _dev(torch.full((1,), -1, dtype=torch.int64))
    first_d = None if first is None else _dev(torch.tensor([first], dtype=torch.int64))
    chars = _dev(torch.full((capacity + MARGIN,), CHAR_SENTINEL, dtype=torch.uint8))
    rle_text._launch_encode_count(n_d, base_d, bounds_d, bounds_d.numel(), 1, total, text_len, text_base, text_total, first_d)
    rle_text._launch_encode_write(n_d, base_d, bounds_d, bounds_d.numel(), 1, total, text_base, chars, capacity)
    return text_len.cpu().numpy(), text_base.cpu().numpy(), int(text_total.cpu()), chars.cpu().numpy(), want


def _check_encoded(masks, total, capacity=None, first=None):
    text_len, text_base, text_total, chars, want = _raw_encode(masks, total, capacity, first)
    assert np.array_equal(text_len, want['text_len']) and np.array_equal(text_base, want['text_base']) and text_total == want['text_total']
    start = 0 if first is None else first
    capacity = want['text_total'] if capacity is None else capacity
    full = np.concatenate([np.full(start, CHAR_SENTINEL, dtype=np.uint8), want['chars']])
    fits = min(capacity, full.size)
    assert np.array_equal(chars[start:fits], full[start:fits])                          # byte for byte up to the capacity
    assert (chars[:min(start, capacity)] == CHAR_SENTINEL).all() and (chars[fits:] == CHAR_SENTINEL).all()   # and nothing anywhere else
    return want


def test_values_on_both_sides_of_every_width_edge():
    masks = TC.edge_masks()
    widths = {len(TC.value_chars(v)) for c in masks for v in TC._values(c)}
    assert widths == {1, 2, 3, 4, 5, 6, 7}
    want = _check_encoded(masks, TC.TOP)
    flat = np.array([v for c in masks for v in c], dtype=np.int64)
    assert [t.decode() for t in want['texts']] == coco_strings(flat, np.array([len(c) for c in masks]))
    single = _check_encoded([[TC.TOP]], TC.TOP)                                          # H * W = 2^31 - 1 in one count
    assert single['texts'] == [b'oooooo1'] and rle_text.max_chars(TC.TOP) == 7


@pytest.mark.parametrize('total', [5, 4099, TC.TOP])
def test_masks_of_one_to_five_counts(total):
    masks = TC.few_counts(total)
    assert [len(c) for c in masks] == [1, 2, 3, 3, 4, 4, 5, 5] and masks[0] == [total] and masks[1][0] == 0
    _check_encoded(masks, total)
    _check_encoded(masks, total, first=9)


def test_count_totals_around_the_steps_of_the_walk():
    total = 70000
    masks = TC.chunk_edge_masks(total)
    assert [len(c) for c in masks] == [TC.SCAN_CHUNK - 1, TC.SCAN_CHUNK, TC.SCAN_CHUNK + 1, 2 * TC.SCAN_CHUNK + 1]
    _check_encoded(masks, total)
    _check_encoded(masks[::-1] + TC.few_counts(total), total, first=3)


@pytest.mark.parametrize('n', [1, TC.MASK_CHUNK - 1, TC.MASK_CHUNK, TC.MASK_CHUNK + 1])
def test_mask_numbers_around_the_steps_of_the_cross_mask_scan(n):
    total = 977
    masks = [TC.long_mask(2 + k % 9, total, k) for k in range(n)]
    _check_encoded(masks, total)


def test_capacities_around_the_exact_one():
    total = TC.TOP
    masks = TC.few_counts(total) + TC.chunk_edge_masks(total)[:2] + TC.edge_masks(total)[:6]
    exact = TC.encode_statement(*TC.to_bounds(masks), total)['text_total']
    for capacity in (0, 1, exact // 2, exact - 1, exact, exact + 5):
        _check_encoded(masks, total, capacity)
    _check_encoded(masks, total, exact + 2, first=7)            # the last five characters do not fit behind a `first` of 7


def test_a_boundary_outside_bounds_is_not_read():
    """C3: a `bounds` shorter than `n` and `base` say (a capacity that was too small): the slots outside count as H * W"""
    total = 500
    n, base, bounds = TC.to_bounds([[100, 50, 350], [10, 20, 30, 440]])
    n_d, base_d, bounds_d = _dev(n), _dev(base), _dev(bounds[:3].copy())           # mask 1 keeps its first boundary alone
    text_len, text_base, text_total = (_dev(torch.zeros(m, dtype=d)) for m, d in ((2, torch.int32), (2, torch.int64), (1, torch.int64)))
    want = [TC.text_of([100, 50, 350]), TC.text_of([10, 490, 0, 0])]                # the boundaries that are not there read H * W
    chars = _dev(torch.full((sum(len(t) for t in want) + MARGIN,), CHAR_SENTINEL, dtype=torch.uint8))
    rle_text._launch_encode_count(n_d, base_d, bounds_d, 3, 1, total, text_len, text_base, text_total, None)
    rle_text._launch_encode_write(n_d, base_d, bounds_d, 3, 1, total, text_base, chars, chars.numel() - MARGIN)
    assert text_len.cpu().tolist() == [len(t) for t in want] and int(text_total.cpu()) == sum(len(t) for t in want)
    assert bytes(chars.cpu().numpy().tobytes()) == b''.join(want) + bytes([CHAR_SENTINEL]) * MARGIN


def test_encode_text_equals_the_statement_and_coco_strings():
    for masks, total in ((TC.edge_masks(), TC.TOP), (TC.chunk_edge_masks(70000) + TC.few_counts(70000), 70000), (TC.blob_counts(65, 63), 65 * 63)):
        n, base, bounds = (_dev(a) for a in TC.to_bounds(masks))
        want = [TC.text_of(c) for c in masks]
        assert rle_text.encode_text(n, base, bounds, (1, total)) == want
        assert rle_text.encode_text(n, base, bounds, (1, total), max_masks=5) == want
        flat = np.array([v for c in masks for v in c], dtype=np.int64)
        assert [t.decode() for t in want] == coco_strings(flat, np.array([len(c) for c in masks]))


# ------------------------------------------------------------------------------------------ the parser, call by call
def _raw_parse(texts, total, spare_words=0):
    """deva_text_parse on `texts` -> (flags, words used, the run buffer with its margins, words_cap); MARGIN sentinels stand
    before and behind the `words_cap` words, and around `info`"""
    n = len(texts)
    body = b''.join(texts)
    first = np.concatenate([[0], np.cumsum([len(t) for t in texts])]).astype(np.int64)
    words_cap = 2 * n + 1 + len(body) + spare_words
    chars = _dev(torch.frombuffer(bytearray(body), dtype=torch.uint8) if body else torch.zeros(0, dtype=torch.uint8))
    runs = _dev(torch.full((words_cap + 2 * MARGIN,), WORD_SENTINEL, dtype=torch.int32))
    info = _dev(torch.full((2 + 2 * MARGIN,), WORD_SENTINEL, dtype=torch.int64))
    scratch = _dev(torch.zeros(max(2 * n, 1), dtype=torch.int32))
    rle_text._launch_parse(chars, len(body), _dev(first), n, 1, total, scratch, runs[MARGIN:MARGIN + words_cap], words_cap, info[MARGIN:MARGIN + 2])
    info, runs = info.cpu().numpy(), runs.cpu().numpy()
    assert (info[:MARGIN] == WORD_SENTINEL).all() and (info[MARGIN + 2:] == WORD_SENTINEL).all()
    assert (runs[:MARGIN] == WORD_SENTINEL).all() and (runs[MARGIN + words_cap:] == WORD_SENTINEL).all()   # C7: never outside
    return int(info[MARGIN]), int(info[MARGIN + 1]), runs[MARGIN:MARGIN + words_cap], words_cap


def _check_parsed(texts, total):
    flags, used, runs, _ = _raw_parse(texts, total)
    words, want_flags = TC.run_words(texts, total)
    assert want_flags == 0 and flags == 0 and used == words.size
    assert np.array_equal(runs[:used], words) and (runs[used:] == WORD_SENTINEL).all()
    parsed = rle.parse_checked(texts, (1, total))
    assert np.array_equal(words, rle.run_array(parsed, 0, len(texts)))                 # word for word the host path's
    return words


def test_every_character_and_every_width():
    text, total = TC.every_character_text()
    assert set(text) == set(range(48, 112))
    _check_parsed([text], total)
    padded = TC.padded_texts(total)
    assert len(padded) == 1 + TC.MAX_CHARS and len({len(t) for t in padded}) == TC.MAX_CHARS
    words = _check_parsed(padded, total)
    assert len({tuple(words[len(padded) + 1:][8 * k:8 * k + 8].tolist()) for k in range(len(padded))}) == 1    # one mask of 7 counts, 13 codings
    wide = [TC.text_of(c, [TC.MAX_CHARS] * len(c)) for c in TC.edge_masks()[:12]]      # every value at the full 12 characters
    _check_parsed(wide, TC.TOP)
    _check_parsed([TC.text_of(c) for c in TC.edge_masks()], TC.TOP)                    # canonical widths 1 .. 7, both signs


@pytest.mark.parametrize('total', [5, TC.TOP])
def test_texts_of_one_to_five_values_and_zero_counts(total):
    _check_parsed([TC.text_of(c) for c in TC.few_counts(total)], total)
    _check_parsed([TC.text_of(c) for c in TC.zero_count_masks(total)], total)


def test_no_mask_at_all():
    flags, used, runs, _ = _raw_parse([], 12)
    assert (flags, used, runs.tolist()) == (0, 1, [0])


def test_value_totals_around_the_steps_of_the_walk_in_both_parities():
    total = 70000
    texts = TC.parity_chunk_texts(total)
    assert {len(TC.read_text(t)[0]) & 1 for t in texts} == {0, 1} and min(len(t) for t in texts) > TC.SCAN_CHUNK
    _check_parsed(texts, total)
    ones = [TC.text_of(TC.filled([1] * (m - 1), total)) for m in (TC.SCAN_CHUNK - 1, TC.SCAN_CHUNK, TC.SCAN_CHUNK + 1, 2 * TC.SCAN_CHUNK + 1)]
    assert [len(t) for t in ones] == [TC.SCAN_CHUNK - 2 + 4, TC.SCAN_CHUNK - 1 + 4, TC.SCAN_CHUNK + 4, 2 * TC.SCAN_CHUNK + 4]   # one character a value but the last
    _check_parsed(ones, total)


def test_a_wide_value_across_every_boundary_between_two_steps():
    total = 70000
    texts = TC.straddling_texts(total)
    assert len(texts) == TC.MAX_CHARS - 1
    _check_parsed(texts, total)
    _check_parsed([TC.text_of([total])] + texts[::-1], total)                           # the same texts at other byte addresses


@pytest.mark.parametrize('n', [1, TC.MASK_CHUNK - 1, TC.MASK_CHUNK, TC.MASK_CHUNK + 1])
def test_parse_mask_numbers_around_the_steps_of_the_cross_mask_scan(n):
    total = 977
    _check_parsed([TC.text_of(TC.long_mask(2 + k % 9, total, k)) for k in range(n)], total)


@pytest.mark.parametrize('name', sorted(TC.flag_cases(100)))
def test_one_input_per_flag_and_nothing_outside_the_buffers(name):
    total = 4200
    good = [TC.text_of(c) for c in TC.few_counts(total)]
    bad, flag = TC.flag_cases(total)[name]
    assert TC.read_text(bad, total)[1] == flag
    for texts in ([bad], good[:3] + [bad] + good[3:], [bad] * 3):
        flags, used, _, words_cap = _raw_parse(texts, total)                           # (the margins are checked in there)
        if flag & (TC.FLAG_CHAR | TC.FLAG_OPEN | TC.FLAG_LONG):
            assert flags & flag == flag                    # what a broken text decodes to may break the counts as well
        else:
            assert flags == flag
        assert 0 < used <= words_cap


def test_any_bytes_at_all_stay_inside_the_buffers():
    rng = np.random.default_rng(11)
    for lo, hi in ((0, 256), (48, 112), (48, 88)):         # any byte, any character, mostly characters that end a value
        texts = [bytes(rng.integers(lo, hi, size=int(m)).astype(np.uint8)) for m in rng.integers(0, 3 * TC.SCAN_CHUNK, size=9)]
        flags, used, _, words_cap = _raw_parse(texts, 4200)
        assert flags != 0 and 0 < used <= words_cap


# ------------------------------------------------------------------------------------------ the public functions
def _message(call):
    with pytest.raises(rle.DevaHipError) as e:
        call()
    return str(e.value)


def test_the_exception_text_is_the_host_paths():
    h, w = 60, 70
    total, dev = h * w, gpu_util.dev()
    good = [{'size': [h, w], 'counts': TC.text_of(c).decode()} for c in TC.few_counts(total)]
    cases = TC.flag_cases(total)
    inputs = {name: good[:2] + [{'size': [h, w], 'counts': text}] + good[2:] for name, (text, _) in cases.items()}
    # two errors of different kinds in different masks: which message wins
    inputs['sum before char'] = [good[0], dict(good[1], counts=cases['short-sum'][0]), dict(good[2], counts=cases['char-low'][0])]
    inputs['open before long'] = [dict(good[0], counts=cases['open'][0]), good[1], dict(good[2], counts=cases['long'][0])]
    inputs['sum before negative'] = [dict(good[0], counts=cases['short-sum'][0]), dict(good[1], counts=cases['negative'][0])]
    inputs['empty before above'] = [dict(good[0], counts=cases['empty-text'][0]), dict(good[1], counts=cases['above'][0])]
    seen = set()
    for name, masks in inputs.items():
        host = _message(lambda: rle.decode(masks, device=dev))
        assert _message(lambda: rle.decode(masks, device=dev, parse='device')) == host, name
        assert _message(lambda: rle.records(masks, parse='device', device=dev)) == _message(lambda: rle.records(masks)), name
        assert (_message(lambda: rle.intersections(good, masks, device=dev, parse='device')) ==
                _message(lambda: rle.intersections(good, masks, device=dev))), name
        seen.add(host.split(': ', 2)[-1][:20])
    assert len(seen) >= 7, seen


@pytest.mark.parametrize('size', [(64, 64), (65, 63), (480, 854)])
def test_round_trip_on_blobs(size):
    h, w = size
    planes = np.stack([LC.blobs(h, w, seed) for seed in (1, 2, 3)] + [np.zeros((h, w), np.uint8), np.ones((h, w), np.uint8)])
    counted = mask_runs.count(_dev(planes))
    total = int(RC.statement(planes)['total'])
    bounds = mask_runs.write(counted, _dev(torch.zeros(total, dtype=torch.int32)))
    texts = rle_text.encode_text(counted.n, counted.base, bounds, size)
    want = [TC.text_of(LC.counts_of(p)) for p in planes]
    assert texts == want
    chunks = rle_text.parse_text(texts, size, device=gpu_util.dev())
    parsed = rle.parse_checked(texts, size)
    assert [(c.lo, c.hi) for c in chunks] == [(0, len(planes))]
    words = rle.run_array(parsed, 0, len(planes))
    assert chunks[0].words == words.size and np.array_equal(chunks[0].host, words) and np.array_equal(chunks[0].device[:words.size].cpu().numpy(), words)
    several = rle_text.parse_text(texts, size, device=gpu_util.dev(), max_masks=2)
    assert [(c.lo, c.hi) for c in several] == [(0, 2), (2, 4), (4, 5)]
    assert all(np.array_equal(c.host, rle.run_array(parsed, c.lo, c.hi)) for c in several)


@pytest.mark.parametrize('size', [(33, 67), (65, 129)])
def test_encode_with_text_on_the_device_equals_the_host_path(size):
    h, w = size
    names, planes = RC.row_planes(h, w)
    stack = _dev(planes)
    want = mask_runs.encode(stack)
    assert want == RC.records(planes) and mask_runs.encode(stack, text='device') == want
    assert mask_runs.encode(stack != 0, text='device', form='bytes', stats=True) == mask_runs.encode(stack != 0, form='bytes', stats=True)
    assert mask_runs.encode(stack, text='device', max_masks=2) == want
    assert mask_runs.encode(stack, text='device', form='counts') == mask_runs.encode(stack, form='counts')
    for threshold in RC.THRESHOLDS:
        logits = _dev(RC.float_stack(h, w, threshold)[1])
        assert mask_runs.encode(logits, threshold=threshold, text='device') == want
    total = int(RC.statement(planes)['total'])
    assert mask_runs.encode(stack, capacity=total, text='device').finish() == want      # the pending form
    assert mask_runs.encode(stack, capacity=total + 50, text='device', stats=True).finish() == mask_runs.encode(stack, stats=True)
    host = _message(lambda: mask_runs.encode(stack, capacity=total - 1).finish())
    assert _message(lambda: mask_runs.encode(stack, capacity=total - 1, text='device').finish()) == host


def test_encode_labels_with_text_on_the_device(monkeypatch):
    if DRYRUN:
        import emu_frame_result
        emu_frame_result.install(monkeypatch)
    labels, ids = RC.disjoint(33, 67)
    want = mask_runs.encode_labels(_dev(labels), ids)
    assert mask_runs.encode_labels(_dev(labels), ids, text='device') == want
    assert mask_runs.encode_labels(_dev(labels), ids[::-1], text='device', form='bytes') == mask_runs.encode_labels(_dev(labels), ids[::-1], form='bytes')


def test_parse_on_the_device_equals_the_host_path():
    h, w = 65, 63
    dev = gpu_util.dev()
    names, all_counts = LC.row(h, w)
    good = [{'size': [h, w], 'counts': TC.text_of(c).decode()} for c in all_counts]
    bare = [TC.text_of(c) for c in all_counts]
    mixed = good[:3] + [{'size': [h, w], 'counts': list(all_counts[3])}] + good[4:]
    want = rle.decode(good, device=dev)
    assert np.array_equal(want.cpu().numpy(), LC.decoded(all_counts, h, w))
    for masks, kw in ((good, {}), (bare, dict(source_size=(h, w))), (mixed, {}), (good, dict(max_masks=2)), (good, dict(max_words=4200))):
        assert torch.equal(rle.decode(masks, device=dev, parse='device', **kw), want)
    resized = rle.decode(good, (40, 50), dtype=torch.float32, device=dev)
    assert torch.equal(rle.decode(good, (40, 50), dtype=torch.float32, device=dev, parse='device'), resized)
    out = _dev(torch.full((len(good), h, w), 7, dtype=torch.uint8))
    assert rle.decode(good, out=out, parse='device') is out and torch.equal(out, want)
    for masks in (good, mixed):
        host, device = rle.records(masks), rle.records(masks, parse='device', device=dev)
        assert all(np.array_equal(a, b) for a, b in zip(host, device))
        host, device = rle.intersections(masks, good[2:7], device=dev), rle.intersections(masks, good[2:7], device=dev, parse='device')
        assert all(torch.equal(a, b) for a, b in zip(host, device))
    several = rle.intersections(good, bare[1:6], source_size=(h, w), device=dev, parse='device', max_masks=4)
    assert all(torch.equal(a, b) for a, b in zip(several, rle.intersections(good, good[1:6], device=dev)))
    crowd = [0, 1, 0, 0, 1]
    assert np.array_equal(rle.iou(good, good[2:7], crowd, device=dev, parse='device'), rle.iou(good, good[2:7], crowd, device=dev))
    empty = rle.intersections(good, [], device=dev, parse='device')
    assert all(torch.equal(a, b) for a, b in zip(empty, rle.intersections(good, [], device=dev)))
