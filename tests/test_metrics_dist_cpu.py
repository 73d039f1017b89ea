"""Sharded scoring on CPU (gloo, 2 ranks): the all-reduced calibration record
of an uneven split of m1 equals the single-process record word for word."""
import os
import socket
import sys
import tempfile

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "calibration-normalizing-flows_amd")
SPLIT = 1537  # rank 0: rows [0, 1537), rank 1: the other 2,608


def _setup_path():
    for p in (ROOT, PKG, HERE):
        if p not in sys.path:
            sys.path.insert(0, p)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, out):
    _setup_path()
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import _metrics_ref as R
    from cnf_hip.dist import sharded_calibration_record
    f = R.load("m1")
    rows = slice(0, SPLIT) if rank == 0 else slice(SPLIT, None)
    rec = sharded_calibration_record(torch.from_numpy(f["probs"][rows]),
                                     torch.from_numpy(f["y"][rows]), 15)
    torch.save(rec, out % rank)
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_record_equals_single_process():
    _setup_path()
    import _metrics_ref as R
    from cnf_hip.metrics import calibration_record
    out = os.path.join(tempfile.mkdtemp(), "rec%d.pt")
    mp.spawn(_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    f = R.load("m1")
    single = calibration_record(torch.from_numpy(f["probs"]), torch.from_numpy(f["y"]), 15)
    R.check_record_counts(single.numpy(), R.score(f["probs"], f["y"], 15), 15)
    for rank in range(2):
        assert torch.equal(torch.load(out % rank, weights_only=True), single), rank
