"""The drop-in Cluster's SWPS_MAX_CAPACITY (include/swiftmpi_compat.h): with it the shard starts at
SWPS_CAPACITY rows and grows under the ceiling as the app's first pull inserts its keys; without
it the capacity is fixed, as before.  The LR main of tests/cpp/compat_apps.cpp on
tests/golden/lr_data.txt, started with a 16-row shard."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

LR_CONF = """[ worker ]
minibatch: 200
[ server ]
initial_learning_rate: 0.05
"""


@pytest.fixture(scope="module")
def compat_bin(lib, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cpp") / "compat_apps")
    libdir = os.path.join(ROOT, "swiftmpi_amd", "lib")
    cmd = ["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "compat_apps.cpp"), "-L" + libdir, "-lswps", "-L/opt/rocm/lib",
           "-Wl,-rpath," + libdir, "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def test_cluster_max_capacity_env(compat_bin, lib, gpu, tmp_path):
    conf = tmp_path / "demo.conf"
    conf.write_text(LR_CONF)
    data = os.path.join(GOLDEN, "lr_data.txt")
    out = str(tmp_path / "err.txt")
    cmd = [compat_bin, "lr", "-config", str(conf), "-data", data, "-niters", "2", "-output", out]
    base = {k: v for k, v in os.environ.items() if k not in ("SWPS_CAPACITY", "SWPS_MAX_CAPACITY")}
    for extra in ({}, {"SWPS_MAX_CAPACITY": "0"}):  # unset or 0: the fixed 16 rows overflow
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=120, env=dict(base, SWPS_CAPACITY="16", **extra))
        assert r.returncode == 3 and "error -1" in r.stderr and "capacity" in r.stderr, r.stdout + r.stderr
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120,
                       env=dict(base, SWPS_CAPACITY="16", SWPS_MAX_CAPACITY="100000"))
    assert r.returncode == 0 and "lr ok" in r.stdout, r.stdout + r.stderr
    t = lib.Table("lr", capacity=4096, dtype="f32", learning_rate=0.05)
    m = lib.LR(t, minibatch=200)
    m.load_text(data)
    m.init()
    assert np.array_equal(np.loadtxt(out), m.train(2))
    m.close()
    t.close()
