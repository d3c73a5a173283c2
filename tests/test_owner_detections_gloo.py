"""Detection merging and semi-online voting of ONE clip on several ranks in frame-owner mode: `shard_queries(owner=0)`
(replicated bank) and `shard_bank(owner=0)` (token-sharded read, value rows sharded), 2 and 3 CPU processes over gloo
with the HIP ops replaced by their PyTorch emulation (tests/owner_mode.py).  Every rank calls `incorporate_detection` /
`vote_in_temporary_buffer` / `step` like the unsharded run; rank 0 alone merges, votes and decodes.

Against the unsharded run of the same scenario: rank 0's outputs agree within `TOL` (BLAS column blocking, as in
tests/test_sharded_read_gloo.py), the other ranks return None; every rank ends with the object table of the unsharded
run (ids, tmp order, votes, missed-detection counters, reserved ids), its bank sizes, bucket membership and usage
counters; with `owner_bank` every value row lives on exactly one rank."""
import os
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

TOL = 2e-5  # tests/test_sharded_read_gloo.py: the emulated ops' BLAS blocking depends on how many columns a call has

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


class _Patch:
    @staticmethod
    def setattr(obj, name, value):
        setattr(obj, name, value)


def _worker(rank, world, port, mode, out):
    try:
        _run(rank, world, port, mode, out)
    except Exception:  # report instead of leaving the parent waiting on the queue
        import traceback
        out.put((rank, 'error', traceback.format_exc()))


def _values_owned_once(mem) -> bool:
    """value-sharded storage: every token's value row lives on exactly one rank (collective: all ranks call it with the
    same buckets)"""
    ok = True
    for store in (mem.work_mem, mem.long_mem) if mem.use_long_term else (mem.work_mem,):
        for b in store.buckets:
            n = store.size(b)
            lrow = store.row_map(b)[:n]
            ok = ok and int((lrow >= 0).sum()) == store.local_size(b)
            owned = (lrow >= 0).to(torch.float32)
            dist.all_reduce(owned)
            ok = ok and bool((owned == 1).all())
    return ok


def _run(rank, world, port, mode, out):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    for p in (ROOT, os.path.join(ROOT, 'tracking-anything-with-deva_amd'), os.path.join(ROOT, 'tests')):
        sys.path.insert(0, p)
    torch.set_grad_enabled(False)
    torch.set_num_threads(max(1, min(4, (os.cpu_count() or 2) // world)))
    import json
    import warnings
    import emu_ops
    import owner_mode
    from workload import synth, weights
    emu_ops.install(_Patch)
    from deva.model.network import DEVA
    golden_dir = os.path.join(ROOT, 'tests', 'golden')
    with open(os.path.join(golden_dir, 'state_dict_spec.json')) as f:
        spec = json.load(f)
    sd = weights.make_state_dict([(k, tuple(s), getattr(torch, d)) for k, s, d in spec['tensors']], seed=0)
    net = DEVA(synth.base_config())
    net.load_weights(sd)
    dist.init_process_group(backend='gloo', rank=rank, world_size=world)
    warnings.simplefilter('ignore')  # the edge cases record their own warnings
    results = {}
    for name in owner_mode.RUNS:
        plain, plain_cores, plain_extra = owner_mode.run(name, net, None, golden_dir)
        outs, cores, extra = owner_mode.run(name, net, mode, golden_dir)
        r = dict(calls=len(outs), plain_calls=len(plain), cores=len(cores) == len(plain_cores))
        if rank == 0:
            r['d_out'] = max((a - b).abs().max().item() if a.shape == b.shape else float('inf')
                             for a, b in zip(plain, outs))
        else:
            r['none'] = all(p is None for p in outs)
        r['tables'] = [owner_mode.table(c.object_manager) for c in cores]
        r['tables_equal'] = r['tables'] == [owner_mode.table(c.object_manager) for c in plain_cores]
        r['d_bank'] = max(owner_mode.bank_difference(owner_mode.bank(a.memory), owner_mode.bank(b.memory))
                          for a, b in zip(plain_cores, cores))
        r['sizes'] = [{k: v for k, v in owner_mode.bank(c.memory).items() if not torch.is_tensor(v)} for c in cores]
        r['comm'] = all(c.memory.comm_bytes > 0 for c in cores if c.memory.engaged or c.object_manager.num_obj)
        if mode == 'owner_bank':
            r['values_owned_once'] = all(_values_owned_once(c.memory) for c in cores)
        if name == 'edge':
            r['edge_host'] = all(torch.equal(plain_extra[k], extra[k]) for k in owner_mode.EDGE_HOST_KEYS)
        if name == 'semionline':
            r['alive'] = extra['alive'] == plain_extra['alive']
        results[name] = r
    out.put((rank, 'ok', results))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize('world,mode', [(2, 'owner'), (3, 'owner'), (2, 'owner_bank'), (3, 'owner_bank')])
def test_owner_mode_detections_reproduce_the_unsharded_run(world, mode):
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, mode, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = {}
    for _ in range(world):
        rank, status, payload = q.get(timeout=900)
        if status == 'error':
            for p in procs:
                p.terminate()
            pytest.fail(f'rank {rank} failed:\n{payload}')
        res[rank] = payload
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    import owner_mode
    for name in owner_mode.RUNS:
        print(f'{name}: {res[0][name]["calls"]} calls, owner outputs within {res[0][name]["d_out"]:.2e}, bank within '
              f'{max(res[r][name]["d_bank"] for r in res):.2e}; final table {res[0][name]["tables"][-1]["ids"]}, '
              f'sizes {res[0][name]["sizes"][-1]}')
        for rank in range(world):
            r = res[rank][name]
            where = f'{name}, rank {rank}'
            assert r['calls'] == r['plain_calls'] > 0 and r['cores'], where
            if rank == 0:
                assert r['d_out'] <= TOL, f'{where}: outputs differ from the unsharded run by {r["d_out"]:.3e}'
            else:
                assert r['none'], f'{where}: a non-owner rank returned probabilities'
            assert r['tables_equal'], f'{where}: object table differs from the unsharded run: {r["tables"]}'
            assert r['d_bank'] <= TOL, f'{where}: bank (sizes / buckets / usage / long-term keys) differs: {r["d_bank"]}'
            assert r['comm'], where
            if mode == 'owner_bank':
                assert r['values_owned_once'], f'{where}: a value row is stored on none or several ranks'
            if name == 'edge':
                assert r['edge_host'], f'{where}: warnings / object counts / engaged flag differ'
            if name == 'semionline':
                assert r['alive'], where
        # every rank holds the same table and the same bank
        assert all(res[rank][name]['tables'] == res[0][name]['tables'] for rank in range(world)), name
        assert all(res[rank][name]['sizes'] == res[0][name]['sizes'] for rank in range(world)), name
