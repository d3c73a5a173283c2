"""Detection merging and semi-online voting in frame-owner mode (`shard_queries(owner=0)`, `shard_bank(owner=0)`) on
the HIP library over a 1-rank RCCL group: the collective paths of a detection frame (query broadcast, sharded read,
object-table broadcast, memory-row broadcast; the vote's broadcast) must reproduce the unsharded run BIT FOR BIT --
outputs, object tables, bank sizes, usage counters and long-term keys.  The 2- and 3-rank splits run on CPU / gloo in
tests/test_owner_detections_gloo.py; the scenarios are tests/owner_mode.py's."""
import socket

import pytest
import torch

import owner_mode
from gpu_util import dev, net_config

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


@pytest.fixture(scope='module')
def network(recipe_state_dict):
    from deva.model.network import DEVA
    sd, _ = recipe_state_dict
    net = DEVA(net_config())
    net.load_weights(sd)
    return net.to(dev()).eval()


@pytest.fixture(scope='module')
def one_rank_group():
    import torch.distributed as dist
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    # "nccl" is RCCL on ROCm; gloo only for the CPU dry run of this file (DEVA_TEST_DRYRUN=1)
    dist.init_process_group('nccl' if dev().type == 'cuda' else 'gloo', init_method=f'tcp://127.0.0.1:{port}', rank=0,
                            world_size=1)
    yield
    dist.destroy_process_group()


_plain = {}


def _unsharded(name, network, golden_dir):
    if name not in _plain:
        _plain[name] = owner_mode.run(name, network, None, golden_dir, device=dev())
    return _plain[name]


def _equal(a, b) -> bool:
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_equal(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(_equal(x, y) for x, y in zip(a, b))
    return a == b


@pytest.mark.parametrize('name,mode', [('detection', 'owner'), ('detection', 'owner_bank'), ('consistent', 'owner'),
                                       ('consistent', 'owner_bank'), ('semionline', 'owner')])
def test_owner_mode_detections_are_bit_identical(network, golden_dir, one_rank_group, name, mode):
    plain, plain_cores, plain_extra = _unsharded(name, network, golden_dir)
    outs, cores, extra = owner_mode.run(name, network, mode, golden_dir, device=dev())
    assert len(outs) == len(plain) > 0 and len(cores) == len(plain_cores)
    assert all(_equal(a, b) for a, b in zip(plain, outs)), [float((a - b).abs().max()) for a, b in zip(plain, outs)
                                                            if a.shape == b.shape]
    for a, b in zip(plain_cores, cores):
        assert owner_mode.table(b.object_manager) == owner_mode.table(a.object_manager)
        assert _equal(owner_mode.bank(b.memory), owner_mode.bank(a.memory))
        assert b.memory.comm_bytes > 0
    assert _equal(extra, plain_extra)  # semionline: the saved index masks and the objects alive at the end
    print(f'{name} / {mode}: {len(outs)} calls, final table {owner_mode.table(cores[-1].object_manager)["ids"]}, '
          f'{cores[-1].memory.comm_bytes} B counted')
