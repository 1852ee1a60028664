"""CPU, world_size 2 over gloo (as tests/test_dist_gloo.py): the exchange that ends a validation pass on more than one rank
(vln_hamt_amd/validate.py::gather_totals) -- every rank hands in its own totals and every rank gets their rank-ordered sum, which is
what the reference's ``sum(all_gather(x))`` gives."""
import os
import socket
import sys

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

TOTALS = [([3.25, 1e-3, 0.0, 7.0], [5, 9, 0, 0, 64]), ([0.125, 1e3, 2.0, 0.0], [2, 11, 0, 1, 36])]       # injected, per rank


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out_dir):
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(2)
    from vln_hamt_amd.parallel import barrier, init_distributed
    from vln_hamt_amd.validate import combine_totals, gather_totals
    assert gather_totals(*TOTALS[rank]) == (TOTALS[rank][0], TOTALS[rank][1])          # no process group yet: this rank's totals
    r, _, w = init_distributed(backend="gloo")
    assert (r, w) == (rank, world) and dist.get_backend() == "gloo"
    sums, counts = gather_totals(*TOTALS[rank])
    assert (sums, counts) == combine_totals(TOTALS), (rank, sums, counts)
    assert sums == [0.0 + a + b for a, b in zip(TOTALS[0][0], TOTALS[1][0])] and counts == [7, 20, 0, 1, 100]
    assert all(type(c) is int for c in counts) and all(type(s) is float for s in sums)
    barrier()
    open(os.path.join(out_dir, f"ok{rank}"), "w").write("ok")
    dist.destroy_process_group()


def test_validation_totals_world2(tmp_path):
    world = 2
    port = _free_port()
    mp.spawn(_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    assert all(os.path.exists(os.path.join(str(tmp_path), f"ok{r}")) for r in range(world))
