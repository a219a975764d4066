"""swps_erase on a routed table across two ranks (tests/dist_erase_check.py: two gloo ranks on one
GPU against one unrouted table, overlapping erase lists, an n = 0 round, one rank finishing early)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_routed_erase_two_ranks_host_transport(lib, gpu):
    from conftest import free_port
    env = dict(os.environ, OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes", "1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()),
           os.path.join(ROOT, "tests", "dist_erase_check.py")]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
    print(r.stdout[-6000:])
    print("\n".join(ln for ln in r.stderr.splitlines() if "rank0" in ln or "Error" in ln)[-6000:])
    assert r.returncode == 0 and "ERASE ROUTE OK" in r.stdout
