"""The reference's text-prompted frame loop, UNCHANGED, on top of this package, against `TextPromptedProcessor` on the
same clip: deva/ext/with_text_processor.py `process_frame_with_text` and deva/ext/grounding_dino.py `segment_with_text`
are executed as they are (tests/run_reference_text_loop.py puts the overlay in front of the reference checkout, stands
in for cv2 / torchvision / groundingdino / segment_anything / supervision and wraps the fakes of tests/text_case.py).
Needs the reference checkout, so it runs in the build container (HIP ops emulated on the CPU) and is skipped elsewhere.

Compared exactly: every index mask and segment list handed to `incorporate_detection` (which is never given
`incremental`), and every saved probability, bit for bit."""
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get('DEVA_REFERENCE_ROOT', '/root/reference')
LAUNCH = os.path.join(ROOT, 'tests', 'run_reference_text_loop.py')

pytestmark = pytest.mark.skipif(not os.path.isfile(os.path.join(REF, 'deva', 'ext', 'with_text_processor.py')),
                                reason='needs the reference checkout (build container only)')


@pytest.fixture(scope='module')
def checkpoint(tmp_path_factory, recipe_state_dict):
    path = str(tmp_path_factory.mktemp('ckpt') / 'recipe.pth')
    torch.save(recipe_state_dict[0], path)
    return path


@pytest.mark.parametrize('setting', ['online', 'semionline'])
def test_the_reference_loop_and_the_processor_agree(setting, checkpoint):
    res = subprocess.run([sys.executable, LAUNCH, setting, checkpoint], cwd=REF, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         text=True, timeout=900)
    print(res.stdout[-6000:])
    assert res.returncode == 0, res.stdout[-6000:]
    frames, channels, failures = (int(v) for v in re.findall(r'(\d+) frames compared, (\d+) channels at most, (\d+) failures',
                                                             res.stdout)[0])
    assert frames == 13 and channels >= 3 and failures == 0
