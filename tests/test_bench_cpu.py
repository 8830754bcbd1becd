"""bench.py's launch logic (no GPU needed): `--gpus N` must end up with N ranks or refuse to run; its options and what
--dump-outputs writes."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_single_gpu_needs_no_spawn():
    assert bench.resolve_world(1, {}) == (1, False)
    assert bench.resolve_world(1, {"WORLD_SIZE": "1"}) == (1, False)


def test_multi_gpu_without_launcher_spawns_ranks():
    assert bench.resolve_world(8, {}) == (8, True)
    assert bench.resolve_world(2, {"PATH": "/usr/bin"}) == (2, True)


def test_multi_gpu_under_launcher_runs_in_place():
    assert bench.resolve_world(4, {"WORLD_SIZE": "4", "RANK": "3"}) == (4, False)


@pytest.mark.parametrize("gpus,ws", [(8, "1"), (1, "2"), (4, "8")])
def test_world_size_mismatch_refuses(gpus, ws):
    with pytest.raises(SystemExit) as e:
        bench.resolve_world(gpus, {"WORLD_SIZE": ws})
    assert "refusing" in str(e.value)


def test_spawn_command_is_the_drivers_launch_line():
    seen = {}

    def fake_run(cmd, env):
        seen["cmd"], seen["env"] = cmd, env
        return 7

    rc = bench.spawn_ranks(4, ["--gpus", "4", "--steps", "2"], environ={"PATH": "/usr/bin"}, run=fake_run)
    assert rc == 7
    cmd = seen["cmd"]
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nnodes=1" in cmd and cmd[cmd.index("--nproc-per-node") + 1] == "4"
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    port = int(cmd[cmd.index("--master-port") + 1])
    assert 1024 < port < 65536
    assert cmd[-5:] == [os.path.join(ROOT, "bench.py"), "--gpus", "4", "--steps", "2"]
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"       # dmabuf IPC: RCCL across processes needs it


def test_config3_is_one_million_in_total():
    assert bench.N_TOTAL_SHARDED == 1_000_000 and bench.N_PER_GPU == 100_000


def test_plain_run_is_the_default_and_steps_are_checked():
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.steps == 7 and a.warmup == 2 and a.full is False and a.dump_outputs is None
    a = bench.parse_args(["--full", "--dump-outputs", "out"])
    assert a.full is True and a.dump_outputs == "out"
    with pytest.raises(SystemExit):
        bench.parse_args(["--steps", "0"])


class _FakeEngine:
    """The handle calls dump_outputs makes, on host arrays."""

    def __init__(self, n, d, k):
        rs = np.random.RandomState(3)
        self.n, self.R, self.k = n, d + 5, k
        self.P = np.asfortranarray(rs.standard_normal((n, d + 5)))
        self.w, self.W = rs.random_sample((n, k)), rs.random_sample((n, k))

    def download_cloud(self):
        return self.P.copy(order="F")

    def stages_held(self):
        return self.k

    def stage_records(self, n_stages):
        s = np.linspace(0.0, 1.0, n_stages)
        return dict(schedule=s, ess=s * 2, c_hist=s * 3, accept_hist=s * 4, resampled=(np.arange(n_stages) % 2).astype(np.int32))

    def history(self, n_stages):
        return self.w[:, :n_stages], self.W[:, :n_stages]


@pytest.mark.parametrize("n", [500, 300000])
def test_dump_outputs_writes_float_arrays_within_the_budget(tmp_path, n):
    eng = _FakeEngine(n, 10, 40)
    res = dict(n_stages=40, resamples=3, logmdd=-25.5)
    bench.dump_outputs(eng, res, str(tmp_path / "a"), history=True)
    got = {f[:-4]: np.load(str(tmp_path / "a" / f)) for f in os.listdir(str(tmp_path / "a"))}
    assert all(a.dtype == np.float64 for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64e6
    assert float(got["logmdd"]) == -25.5 and float(got["n_stages"]) == 40 and float(got["resamples"]) == 3
    assert got["tempering_schedule"].shape == (40,) and got["resampled"][1] == 1.0
    if n <= bench.DUMP_HISTORY_ROWS:
        np.testing.assert_array_equal(got["cloud"], eng.P)
        np.testing.assert_array_equal(got["incremental_weights"], eng.w)
        assert "cloud_rows" not in got and "history_rows" not in got
    else:                                                            # a seeded sample of rows, the same in every run
        rows, hrows = got["cloud_rows"].astype(np.int64), got["history_rows"].astype(np.int64)
        assert rows.size * eng.R * 8 <= bench.DUMP_CLOUD_BYTES < n * eng.R * 8 and hrows.size == bench.DUMP_HISTORY_ROWS
        np.testing.assert_array_equal(got["cloud"], eng.P[rows])
        np.testing.assert_array_equal(got["normalized_weights"], eng.W[hrows])
        bench.dump_outputs(eng, res, str(tmp_path / "b"), history=True)
        np.testing.assert_array_equal(np.load(str(tmp_path / "b" / "cloud_rows.npy")), got["cloud_rows"])
    bench.dump_outputs(eng, res, str(tmp_path / "c"), history=False)
    assert not os.path.exists(str(tmp_path / "c" / "incremental_weights.npy"))


def test_julia_probe_reports_unavailable_or_a_version():
    """the bench line says by itself whether the reference's runtime is on the box (cpu_baseline.reference_julia)."""
    import shutil

    got = bench.probe_julia()
    if shutil.which("julia") is None:
        assert got == "unavailable"
    else:
        assert "julia" in got.lower()
