"""sharding.exchange_bytes on CPU: two gloo ranks hand each other byte strings of unequal length,
one of them empty -- what carries snapshot blobs between ranks.  The process pattern is
test_distributed's."""
import os
import pickle
import socket

import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _payload(src, dst, rnd):
    """What rank src sends to rank dst in round rnd: lengths 0, 1, 5000, 70001, ... by pair."""
    n = [[3, 70001], [0, 5000]][src][dst] if rnd == 0 else [[0, 0], [1, 0]][src][dst]
    return bytes((7 * src + 3 * dst + i) % 251 for i in range(n))


def _worker(rank, world, port, out_dir):
    import sys
    sys.path[:0] = [ROOT]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from mhpc_minimal_env_amd import sharding
    got = [sharding.exchange_bytes([_payload(rank, r, rnd) for r in range(world)]) for rnd in (0, 1)]
    try:
        sharding.exchange_bytes([b""])
        got.append("accepted a list of the wrong length")
    except ValueError:
        pass
    with open(os.path.join(out_dir, f"rank{rank}.pkl"), "wb") as f:
        pickle.dump(got, f)
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_exchange(tmp_path):
    world = 2
    mp.start_processes(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True,
                       start_method="spawn")
    for rank in range(world):
        with open(tmp_path / f"rank{rank}.pkl", "rb") as f:
            got = pickle.load(f)
        assert len(got) == 2, got[-1]
        for rnd in (0, 1):
            assert got[rnd] == [_payload(src, rank, rnd) for src in range(world)], (rank, rnd)
