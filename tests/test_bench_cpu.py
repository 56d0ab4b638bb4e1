"""bench.py's launcher contract (CPU): `--gpus N` without a torchrun
environment launches N ranks itself; a torchrun environment whose WORLD_SIZE
differs from --gpus is refused before any GPU work."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, **env_over):
    env = {k: v for k, v in os.environ.items()
           if not k.startswith("FRECSYS_") and k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(env_over)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env,
                          capture_output=True, text=True, timeout=120)


def _plan(r):
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_gpus_n_launches_n_ranks():
    r = _run(["--gpus", "4", "--steps", "3", "--print-launch"])
    cmd = _plan(r)["launch"]
    assert cmd[1:3] == ["-m", "torch.distributed.run"]
    assert "--nproc-per-node=4" in cmd and "--nnodes=1" in cmd
    assert "--master-addr=127.0.0.1" in cmd
    assert cmd[cmd.index(os.path.join(ROOT, "bench.py")) + 1:] == ["--gpus", "4", "--steps", "3",
                                                                   "--print-launch"]


def test_torchrun_env_is_used_as_is():
    r = _run(["--gpus", "2", "--print-launch"], WORLD_SIZE="2", RANK="1", LOCAL_RANK="1")
    assert _plan(r)["launch"] is None  # no second launch


def test_world_size_mismatch_refused():
    r = _run(["--gpus", "1"], WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    assert r.returncode != 0
    assert "--gpus 1 but WORLD_SIZE=2" in r.stderr
    r = _run(["--gpus", "8"], WORLD_SIZE="4", RANK="0", LOCAL_RANK="0")
    assert r.returncode != 0 and "WORLD_SIZE=4" in r.stderr


def test_frecsys_env_refused():
    r = _run(["--gpus", "1"], FRECSYS_DUAL="0")
    assert r.returncode != 0 and "refusing" in r.stderr


def test_default_extras_every_config_at_every_n():
    """BASELINE configs[3] and [4] are defined on 8 GPUs: the N = 8 run with
    --full measures configs 3, 4 and 5 beside the headline."""
    import bench
    for n in (1, 2, 4, 8):
        assert bench.default_extras(n).split(",") == ["safer2_ml20m_d256", "ials_msd_d512",
                                                      "safer2_2m500k_d1024"]
    assert bench.WORKLOADS["safer2_2m500k_d1024"]["max_extra_steps"] == 2
    for n in (1, 8):
        plan = _plan(_run(["--gpus", str(n), "--full", "--print-launch"]))
        assert plan["n_gpus"] == n and plan["workload"] == "ials_ml20m_d256" and plan["full"]
        assert plan["extras"] == ["safer2_ml20m_d256", "ials_msd_d512", "safer2_2m500k_d1024"]
        assert plan["cpu_baseline"] == (n == 1)  # the CPU baseline stays at N = 1
        assert (plan["launch"] is None) == (n == 1)
        if n == 8:
            assert "--nproc-per-node=8" in plan["launch"]
    # every default extra is a BASELINE config the bench knows
    assert all(w in bench.WORKLOADS for w in bench.DEFAULT_EXTRAS)


def test_plain_run_measures_the_headline_only():
    """Without --full a run times the headline and nothing else: no extra
    workloads, no CPU baseline, whatever --cpu-seconds says; --extras without
    --full is refused, not dropped silently."""
    for n in (1, 8):
        plan = _plan(_run(["--gpus", str(n), "--steps", "3", "--warmup", "1", "--cpu-seconds", "10",
                           "--print-launch"]))
        assert plan["workload"] == "ials_ml20m_d256" and plan["full"] is False
        assert plan["extras"] == [] and plan["cpu_baseline"] is False
    assert _plan(_run(["--extras=", "--print-launch"]))["extras"] == []
    r = _run(["--extras", "ials_msd_d512", "--print-launch"])
    assert r.returncode != 0 and "--full" in r.stderr
    plan = _plan(_run(["--full", "--extras", "ials_msd_d512", "--cpu-seconds", "0",
                       "--print-launch"]))
    assert plan["extras"] == ["ials_msd_d512"] and plan["cpu_baseline"] is False


def test_dump_sample_is_fixed_and_bounded():
    """--dump-outputs: a table above DUMP_SIDE_BYTES is written as the same
    ascending sample of rows on every call, a smaller one whole; two tables
    stay under 64 MB."""
    import numpy as np
    import bench

    class Ctx:
        def __init__(self):
            self.t = {0: np.arange(50000 * 256, dtype=np.float32).reshape(50000, 256),
                      1: np.arange(300 * 256, dtype=np.float32).reshape(300, 256)}

        def get_embeddings(self, side):
            return self.t[side]

    class FH:
        SIDE_USER, SIDE_ITEM = 0, 1

    assert 2 * bench.DUMP_SIDE_BYTES <= 64 * 10 ** 6
    old, bench.fh = bench.fh, FH
    try:
        import tempfile
        with tempfile.TemporaryDirectory() as a, tempfile.TemporaryDirectory() as b:
            sa = bench.dump_outputs(Ctx(), os.path.join(a, "sub"))
            bench.dump_outputs(Ctx(), b)
            ua = np.load(os.path.join(a, "sub", "user_emb.npy"))
            ub = np.load(os.path.join(b, "user_emb.npy"))
            va = np.load(os.path.join(a, "sub", "item_emb.npy"))
    finally:
        bench.fh = old
    assert ua.dtype == np.float32 and va.dtype == np.float32
    assert np.array_equal(ua, ub) and np.array_equal(va, Ctx().t[1])
    rows = bench.DUMP_SIDE_BYTES // (256 * 4)
    assert ua.shape == (rows, 256) and ua.nbytes <= bench.DUMP_SIDE_BYTES
    first = ua[:, 0] / 256  # the row index of each sampled row
    assert np.all(np.diff(first) > 0) and np.array_equal(ua, Ctx().t[0][first.astype(np.int64)])
    assert sa == {"user_emb": {"rows": rows, "of": 50000, "dim": 256},
                  "item_emb": {"rows": 300, "of": 300, "dim": 256}}
