"""bench.py's command line: a plain run is lean (window + the whole solve), ``--full`` adds the start sets
and the CPU baseline, ``--dump-outputs DIR`` writes what the timed window's last step left on the device.

* CPU: ``dump_outputs`` on a stand-in handle: fp64 ``.npy`` files, the same seeded sample of trajectories
  in every array and from call to call, all files together under 64 MB even for a batch far over it.
* ``bench.py --help`` lists the options.
"""
import pathlib
import subprocess
import sys

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import bench  # noqa: E402


class _FakeHandle:
    """tog_get stand-in: B trajectories of the headline's shape with recognisable rows."""

    def __init__(self, abi, B, N=101, n=13, m=4):
        self.abi, self.B, self.N, self.n, self.m = abi, B, N, n, m

    def get(self, field):
        abi, B = self.abi, self.B
        row = np.arange(B, dtype=np.float64)
        if field == abi.FIELD_X:
            return np.broadcast_to(row[:, None, None], (B, self.N, self.n))
        if field == abi.FIELD_U:
            return np.broadcast_to(-row[:, None, None], (B, self.N - 1, self.m))
        assert field == abi.FIELD_STATS
        return np.repeat(row[:, None], abi.NSTATS, axis=1) + np.arange(abi.NSTATS)


NAMES = {"X", "U", "cost", "c_max", "iterations", "flags", "traj_index"}


@pytest.mark.parametrize("B", [5, 20000])
def test_dump_outputs_sample(tog, tmp_path, B):
    abi = tog.abi
    info = bench.dump_outputs(str(tmp_path / "a"), _FakeHandle(abi, B), abi)
    bench.dump_outputs(str(tmp_path / "b"), _FakeHandle(abi, B), abi)
    files = sorted((tmp_path / "a").iterdir())
    assert {f.stem for f in files} == NAMES and all(f.suffix == ".npy" for f in files)
    assert sum(f.stat().st_size for f in files) <= 64 * 10 ** 6
    a = {f.stem: np.load(f) for f in files}
    assert all(v.dtype == np.float64 for v in a.values())
    idx = a["traj_index"]
    keep = len(idx)
    assert keep == info["trajectories"] and info["of"] == B
    assert keep == B if B == 5 else 1000 < keep < B  # the sample is a real share of a large batch
    assert np.all(np.diff(idx) > 0) and 0 <= idx[0] and idx[-1] < B
    # every array holds the same trajectories: the stand-in's rows carry their trajectory number
    assert a["X"].shape == (keep, 101, 13) and np.array_equal(a["X"][:, 7, 3], idx)
    assert a["U"].shape == (keep, 100, 4) and np.array_equal(a["U"][:, 7, 3], -idx)
    assert np.array_equal(a["cost"], idx + abi.STAT_J) and np.array_equal(a["c_max"], idx + abi.STAT_C_MAX)
    assert np.array_equal(a["iterations"], idx + abi.STAT_TOTAL_STEPS)
    assert np.array_equal(a["flags"], idx + abi.STAT_FLAGS)
    for f in files:  # the same arguments give the same files
        assert np.array_equal(a[f.stem], np.load(tmp_path / "b" / f.name))


def test_bench_options():
    out = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--help"], capture_output=True, text=True)
    assert out.returncode == 0
    for opt in ("--full", "--dump-outputs", "--gpus", "--steps", "--warmup"):
        assert opt in out.stdout
