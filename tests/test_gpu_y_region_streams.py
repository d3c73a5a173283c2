"""Does every launch of `label_components` and `remove_small_regions` go to the caller's stream?  The probe of
tests/stream_probe.py as tests/test_gpu_w_pair_streams.py uses it: the call runs on a side stream that is still blocked
behind a delay kernel while its inputs hold decoys (other valid planes), and must be bit-identical to the default-stream
run.  All three launches of a labelling and all twelve of a clean-up pass are behind the one stream argument; a launch on
the null stream would read the decoys or run before the stage it depends on."""
import os

import numpy as np
import pytest
import torch

import emu_regions as ER
import region_case as RC
import stream_probe as SP
from deva.hip import regions
from gpu_util import dev

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DRYRUN = os.environ.get('DEVA_TEST_DRYRUN') == '1'
H, W = 33, 67       # two tile rows, three tile columns: the border stage has work


@pytest.fixture(autouse=True)
def _emulated_when_dry(monkeypatch):
    if DRYRUN:
        ER.install(monkeypatch)


def _inputs():
    names, planes, min_area = RC.row(H, W)
    real = np.array(planes)
    decoy = np.ascontiguousarray(real[::-1, :, ::-1])       # other planes, mirrored: valid, and different everywhere that matters
    return real, decoy, min_area


@pytest.mark.parametrize('of_zeros', [False, True])
def test_label_components_on_a_blocked_side_stream(of_zeros):
    real, decoy, _ = _inputs()
    want = SP.probe(lambda i, mark: regions.label_components(i['planes'], of_zeros=of_zeros), dict(planes=torch.from_numpy(real)),
                    dict(planes=torch.from_numpy(decoy)), f'label_components (of_zeros={of_zeros})')
    # the default-stream run the probe compared with is the statement's
    assert [path for path, _ in want] == ['out']
    assert np.array_equal(want[0][1].numpy(), RC.expected(H, W)[3 if of_zeros else 2])


@pytest.mark.parametrize('passes', [1, 3])
def test_remove_small_regions_on_a_blocked_side_stream(passes):
    real, decoy, min_area = _inputs()
    one = regions.region_scratch_bytes(H, W)
    together = -(-len(real) // passes)
    assert regions.region_plan(H, W, len(real), together * one).passes == passes
    scratch = torch.empty(together * one, dtype=torch.uint8, device=dev())

    def run(i, mark):
        return regions.remove_small_regions(i['planes'].clone(), min_area, scratch=scratch)    # (the call works in place)
    want = SP.probe(run, dict(planes=torch.from_numpy(real)), dict(planes=torch.from_numpy(decoy)), f'remove_small_regions ({passes} passes)')
    assert [path for path, _ in want] == ['out[0]', 'out[1]']
    want_planes, want_records = RC.expected(H, W)[:2]
    assert np.array_equal(want[0][1].numpy(), want_planes) and np.array_equal(want[1][1].numpy(), want_records)
