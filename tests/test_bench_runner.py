"""CPU: bench.py's step runners against a stand-in mapper that follows include/loam_core.h's queue
rules (solve_async enqueues a frame, wait finishes the oldest, pose / total_iterations report
the newest finished frame).  The pipelined runner (the default for the timed steps) must count
every frame once and record stream 0's pose after every frame, in order, as the blocking runner
does; one host thread per handle."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class QueueMapper:
    def __init__(self, offset=0):
        self.given = None
        self.queue = []
        self.done = None
        self.offset = offset
        self.calls = []

    def input_device_batch_args(self, plan):
        self.given = plan[0]

    def solve_async(self):
        assert self.given is not None
        assert len(self.queue) < 2
        self.queue.append(self.given)
        self.given = None
        self.calls.append("async")

    def wait(self):
        self.done = self.queue.pop(0)
        self.calls.append("wait")

    def solve(self):
        self.solve_async()
        self.wait()

    def total_iterations(self):
        return 10 + self.done

    def pose(self, s):
        return (self.offset + self.done, s)


def test_pipelined_runner_counts_every_frame_once_in_order():
    import bench
    plan = [(k,) for k in range(12)]
    m = QueueMapper()
    poses = []
    it = bench.run_steps_pipelined(m, plan, 3, 6, poses)
    assert it == sum(10 + k for k in range(3, 9))
    assert poses == [(k, 0) for k in range(3, 9)]
    # each frame enqueued before the one in flight is waited for
    assert m.calls[:3] == ["async", "async", "wait"]
    assert m.calls.count("async") == m.calls.count("wait") == 6
    b = QueueMapper()
    bposes = []
    assert bench.run_steps(b, plan, 3, 6, bposes) == it
    assert bposes == poses


def test_plain_run_is_the_default(monkeypatch):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    a = bench.parse()
    assert not a.full and a.dump_outputs is None and a.steps == 3
    # a plain run takes no leg beside the headline
    bench.select_legs(a)
    assert a.no_cpu and a.no_exact_leg and a.no_single_stream and a.no_depth and a.shard_streams == 0
    # older command lines that switch legs off still parse and stay plain
    monkeypatch.setattr(sys, "argv", ["bench.py", "--no-cpu", "--shard-streams", "0"])
    a = bench.select_legs(bench.parse())
    assert a.no_exact_leg and a.no_single_stream and a.no_depth and a.shard_streams == 0
    # the sharded leg asked for without --full: refused, not dropped
    monkeypatch.setattr(sys, "argv", ["bench.py", "--shard-streams", "8"])
    with pytest.raises(SystemExit, match="--full"):
        bench.select_legs(bench.parse())
    # --full: every leg, less the ones switched off
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.select_legs(bench.parse())
    assert a.full and a.dump_outputs == "d" and a.shard_streams == 32
    assert not (a.no_cpu or a.no_exact_leg or a.no_single_stream or a.no_depth)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--no-cpu", "--no-single-stream", "--no-depth",
                                      "--shard-streams", "0"])
    a = bench.select_legs(bench.parse())
    assert a.no_cpu and a.no_single_stream and a.no_depth and not a.no_exact_leg and a.shard_streams == 0
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--shard-streams", "8"])
    assert bench.select_legs(bench.parse()).shard_streams == 8


class OutputMapper:
    """stand-in with the calls last_step_outputs makes; stream b of handle h answers from the
    global stream number g = h * n_streams + b"""

    def __init__(self, h, n_streams):
        self.h, self.n_streams = h, n_streams

    def g(self, b):
        return self.h * self.n_streams + b

    def stats_all(self):
        from loam_amd import _core
        out = []
        for b in range(self.n_streams):
            st = _core.MapStats()
            st.corner_num[0], st.corner_num[1] = 100 + self.g(b), 200 + self.g(b)
            st.surf_num[0], st.surf_num[1] = 300 + self.g(b), 400 + self.g(b)
            st.lm[0].iterations, st.lm[1].iterations = 4, self.g(b) % 5
            st.lm[0].final_cost, st.lm[1].final_cost = 0.5 * self.g(b), 0.25 * self.g(b)
            out.append(st)
        return out

    def pose(self, b):
        import numpy as np
        return np.full(4, float(self.g(b))), np.full(3, 10.0 + self.g(b))

    def get_state(self, b):
        import numpy as np
        return np.zeros(3, np.int32), np.full(4, -float(self.g(b))), np.full(3, -10.0 - self.g(b))

    def map_cloud(self, b):
        import numpy as np
        return np.full((3 + self.g(b), 4), float(self.g(b)), dtype=np.float32)


def test_last_step_outputs_names_order_and_map_streams():
    import numpy as np

    import bench
    sys.path.insert(0, os.path.join(ROOT, "vloam-noted_amd"))
    ms = [OutputMapper(0, 6), OutputMapper(1, 6)]
    out = bench.last_step_outputs(ms, 7)
    g = np.arange(12.0)
    per_stream = {"pose_q": (12, 4), "pose_t": (12, 3), "q_wmap_wodom": (12, 4), "t_wmap_wodom": (12, 3),
                  "corner_num": (12, 2), "surf_num": (12, 2), "lm_iterations": (12, 2), "lm_final_cost": (12, 2)}
    for name, shape in per_stream.items():
        assert out[name].shape == shape and out[name].dtype == np.float64, name
    # every stream of handle 0, then every stream of handle 1
    assert np.array_equal(out["pose_q"][:, 0], g) and np.array_equal(out["pose_t"][:, 0], 10 + g)
    assert np.array_equal(out["q_wmap_wodom"][:, 0], -g) and np.array_equal(out["t_wmap_wodom"][:, 0], -10 - g)
    assert np.array_equal(out["corner_num"], np.stack([100 + g, 200 + g], 1))
    assert np.array_equal(out["surf_num"], np.stack([300 + g, 400 + g], 1))
    assert np.array_equal(out["lm_iterations"], np.stack([np.full(12, 4.0), g % 5], 1))
    assert np.array_equal(out["lm_final_cost"], np.stack([0.5 * g, 0.25 * g], 1))
    # the map clouds: DUMP_MAP_STREAMS distinct streams, named by their global number, chosen by the
    # seed alone
    clouds = sorted(set(out) - set(per_stream))
    assert len(clouds) == bench.DUMP_MAP_STREAMS
    for name in clouds:
        assert name.startswith("map_cloud_stream")
        s = int(name[len("map_cloud_stream"):])
        assert 0 <= s < 12 and out[name].dtype == np.float32 and out[name].shape == (3 + s, 4)
        assert np.all(out[name] == s)
    assert sorted(set(bench.last_step_outputs(ms, 7)) - set(per_stream)) == clouds
    # fewer streams than DUMP_MAP_STREAMS: all of them
    few = bench.last_step_outputs([OutputMapper(0, 2)], 7)
    assert sorted(set(few) - set(per_stream)) == ["map_cloud_stream0", "map_cloud_stream1"]


def test_dump_outputs_types_and_size_limit(tmp_path, monkeypatch):
    import numpy as np

    import bench
    rng = np.random.default_rng(0)
    outs = {"pose_q": rng.normal(size=(5, 4)), "counts": np.arange(10, dtype=np.int32).reshape(5, 2),
            "cloud": rng.normal(size=(1000, 4)).astype(np.float32)}
    bench.dump_outputs(str(tmp_path / "a"), outs, 7)
    got = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in outs}
    assert got["pose_q"].dtype == np.float64 and np.array_equal(got["pose_q"], outs["pose_q"])
    assert got["counts"].dtype == np.float64 and np.array_equal(got["counts"], outs["counts"])
    assert got["cloud"].dtype == np.float32 and np.array_equal(got["cloud"], outs["cloud"])
    # over the limit: the same seeded rows every time, in order, and the files fit
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 3 * 4096 + 8000)
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), outs, 7)
    b, c = (np.load(tmp_path / d / "cloud.npy") for d in ("b", "c"))
    assert np.array_equal(b, c) and 0 < len(b) < 1000
    rows = [int(np.flatnonzero((outs["cloud"] == r).all(axis=1))[0]) for r in b]
    assert rows == sorted(rows)
    assert sum(os.path.getsize(tmp_path / "b" / f) for f in os.listdir(tmp_path / "b")) <= 3 * 4096 + 8000
    assert np.array_equal(np.load(tmp_path / "b" / "pose_q.npy"), outs["pose_q"])


def test_run_handles_pipelined_threads():
    import bench
    plans = [[(k,) for k in range(8)] for _ in range(2)]
    ms = [QueueMapper(0), QueueMapper(100)]
    poses = []
    it = bench.run_handles(ms, plans, 2, 5, poses, pipelined=True)
    assert it == 2 * sum(10 + k for k in range(2, 7))
    assert poses == [(k, 0) for k in range(2, 7)]  # handle 0's stream 0 only
