"""N > 1 on REAL GPUs (missing 2): self-activating -- every test here is skipped on a box with one GPU and runs the
moment two are visible.  One process, er_comm_create_local (ncclCommInitAll) on DISTINCT devices, one host thread per rank: the frame-split merge over RCCL
(grouped ncclSend / ncclRecv of band records to the unit owners, the owners' rank-ordered sums; and round 5's ncclReduce / ncclAllReduce protocol), the
drop-in programs with --gpus N against their single-GPU files, and bench.py through the driver's torch.distributed.run command line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers
from elasticreconstruction_amd import _ffi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def n_devices():
    try:
        return int(_ffi.lib().er_device_count())
    except Exception:
        return 0


needs2 = pytest.mark.skipif(n_devices() < 2, reason="needs two or more GPUs (found %d)" % n_devices())


@needs2
@pytest.mark.parametrize("root", [-2, 0, -1], ids=["owner--2", "owner-0", "owner--1"])
def test_frame_split_merge_over_rccl_two_gpus(gpu, root):
    """er_tsdf_allreduce over RCCL between TWO devices against the single-volume result: raw units bit-identical, summed units 1e-5 with exact weights and
    the rank-ordered float32 sum bit for bit, stats equal to the key-set arithmetic; run twice: the summed units must be bit-reproducible (the owner
    merge's summation order is a function of the key sets)."""
    from elasticreconstruction_amd import parallel
    out = helpers.check_frame_split_merge(lambda: parallel.LocalComms([0, 1]), [0, 1], root, repeat=2)
    out["bit_reproducible"] = True
    print("RCCL merge, 2 GPUs:", out)


@needs2
@pytest.mark.parametrize("root", [-2, 0])
def test_frame_split_merge_over_rccl_all_gpus(gpu, root):
    """The owner merge with one rank per visible GPU (up to 8)."""
    from elasticreconstruction_amd import parallel
    devs = list(range(min(n_devices(), 8)))
    out = helpers.check_frame_split_merge(lambda: parallel.LocalComms(devs), devs, root, per=50)
    print("RCCL merge, %d GPUs:" % len(devs), out)


@needs2
def test_integrate_program_two_gpus_equals_single_gpu(gpu, tmp_path):
    """bin/Integrate --gpus 2 --shard frame (frame blocks + the merge over RCCL, world.pcd assembled from the owners' extractions) and --shard unit
    (bit-exact, no collective) against the single-GPU program's world.pcd."""
    import test_host_programs_gpu as hp
    hp.integrate_multi_gpu_case(str(tmp_path), ["--gpus", "2"], same_device=False)


@needs2
def test_build_correspondence_program_two_gpus_equals_single_gpu(gpu, tmp_path):
    """bin/BuildCorrespondence --gpus 2 (pairs p -> GPU p mod 2, no collective): the same reg_output.log / .info / corres_*.txt as with one GPU."""
    import test_host_programs_gpu as hp
    hp.build_correspondence_multi_gpu_case(str(tmp_path), 2)


@needs2
def test_bench_two_ranks_over_rccl(gpu, tmp_path):
    """bench.py as the driver launches it for N = 2 (torch.distributed.run, one rank per GPU, er_comm_create with the id carried by torch.distributed):
    ONE compact JSON line, n_gpus 2, rccl_ranks 2, weak scaling, the merge inside the timed region."""
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    full = str(tmp_path / "bench_full.json")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(ROOT, "bench.py"), "--gpus", "2", "--full", "--steps", "4", "--warmup", "1", "--min-seconds", "0.3", "--icp-pairs", "0", "--full-json", full]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    last = [l for l in r.stdout.splitlines() if l.strip()][-1]
    assert len(last) < 4096
    c = json.loads(last)
    assert c["n_gpus"] == 2 and c["config"]["rccl_ranks"] == 2 and c["scaling"] == "weak" and c["value"] > 0
    with open(full) as fh:
        out = json.load(fh)
    ms = out["config"]["merge_stats"]
    assert ms["impl"] == "owner" and ms["multi_toucher_units"] > 0 and ms["bytes_reduced"] == 0
    print("bench.py --gpus 2:", last)
