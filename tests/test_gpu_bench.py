"""bench.py end to end (small --scale): the single-GPU line the driver records, and the N > 1 path
(two ranks sharing cuda:0 over gloo — RCCL needs one device per rank; the protocol is the same:
the staleness-budget cadence with the two-tier reconciliation, and r3's job cadence with the
sharded snapshot refresh + all-gather)."""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]


def _line(res):
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, res.stdout[-1000:]
    return json.loads(lines[0])


def test_bench_single_gpu_line():
    res = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--full", "--scale", "0.05", "--steps", "6",
                          "--warmup", "2", "--cpu-seconds", "1", "--steady-timed-epochs", "3"],
                         capture_output=True, text=True, timeout=900)
    j = _line(res)
    assert j["n_gpus"] == 1 and j["unit"] == "triples/s" and j["value"] > 1e6 and j["dtype"] == "f32"
    assert j["vs_baseline"] is None and j["higher_is_better"] is True and j["data"] == "synthetic"
    r = j["roofline"]
    assert r["bound"] == "hbm" and r["peak"] == 8000.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
    assert r["traffic_measured_in_this_run"] is False
    assert j["roofline_atomic"]["line_atomics_per_triple"] >= 8.0
    assert j["cpu_baseline"]["cores"] >= 1 and j["cpu_baseline"]["value"] > 0
    sched = j["config"]["refresh_schedule"]
    assert sched["lag"] == 1.0 and sched["side_stream_cus"] >= 32  # the schedule the gates hold (32 CUs since the binned sort)
    sus = j["sustained"]  # whole epochs from random init, every plan in place
    st = j["steady_state"]  # whole epochs timed after 30 epochs of the same job: the trained state, the headline
    spe = j["config"]["steps_per_epoch"]
    assert st["epochs_trained_before"] >= 30 and st["steps"] == st["epochs"] * spe and st["value"] > 1e6
    assert st["first_epoch"]["epoch"] == st["epochs_trained_before"] + 1 and st["first_epoch"]["value"] > 1e6
    trained = (st["epochs_trained_before"] + st["epochs"]) * spe - ((6 + 2 + 1) // spe + 1 + sus["epochs"]) * spe
    tr = j["trained_region"]  # the headline's steps run after the steady epochs: its untimed lead-in and its K steps
    assert j["config"]["triples_counted_by_kernel"] == (6 + sus["steps"] + trained + tr["untimed_steps_before"] + 6) * \
        j["config"]["triples_per_step_per_gpu"]
    assert sus["epochs"] >= 3 and sus["value"] > 1e6 and 0 < r["read_only_frac"] < r["frac"]
    # the headline is the TRAINED state: the K = --steps steps of the job after --trained-epochs epochs, by wall clock,
    # `steps` the steps behind it; the early state, the driver's K-step region from random init and the trained
    # state's whole epochs (epochs 31.. as before) ride along under --full
    assert st["epochs_trained_before"] == 30
    assert j["value_source"].startswith("trained state") and j["steps"] == tr["steps"] == 6 and j["warmup"] == 2
    assert tr["epochs_trained_before"] >= 80 and tr["first_step"] == tr["epochs_trained_before"] * spe + 1
    assert tr["first_step"] >= (st["epochs_trained_before"] + st["epochs"]) * spe
    assert abs(j["value"] - 6 * j["config"]["triples_per_step_per_gpu"] / (6 * j["ms_per_step"] * 1e-3)) < 1e-6 * j["value"]
    assert tr["plans_added"] == 6 / spe - 6 // spe and tr["ms_per_step_measured"] <= j["ms_per_step"]
    assert j["early_state"]["value"] == sus["value"] and 0 < j["early_state"]["roofline_frac"] < 1
    assert r["kernel_ms_avg"] == st["kernel_ms_avg"] and st["ms_per_step"] > 0
    assert j["timed_region"]["steps"] == 6 and j["timed_region"]["value_measured"] > 1e6
    lds = j["config"]["hot_lds"]  # lr 0.001: inside the staleness budget -> asked for; a 5 % shard's launches may not fill the chip
    assert lds["rows_asked"] > 0 and lds["rows_in_lds_last_launch"] >= 0
    assert j["config"]["parity"]["tolerance_north_star"] == 0.002
    port = j["cpu_baseline_c_port"]  # the C restatement with OpenMP over triples
    assert port["kind"] == "port" and port["cores"] >= 1 and port["value"] > 0 and "OpenMP" in port["sample"]
    assert "optim.sgd.SGD" in j["cpu_baseline"]["sample"] or "SGD" in j["cpu_baseline"]["sample"]


def test_bench_workload_brings_its_own_hyperparameters():
    """--workload yelp = BASELINE configs[4]: Adam(0.1, 0.999), reg .0025/.0025/.00025, and a CPU baseline
    with the SAME optimizer (the committed cfg5 line carried an SGD baseline)."""
    res = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--full", "--workload", "yelp", "--scale", "0.1",
                          "--steps", "4", "--warmup", "2", "--cpu-seconds", "1", "--sustained-epochs", "1",
                          "--steady-epochs", "0"],
                         capture_output=True, text=True, timeout=900)
    j = _line(res)
    w = j["config"]["workload"]
    assert "Adam lr=0.001 betas=(0.1, 0.999)" in w and "(0.0025, 0.0025, 0.00025)" in w and "d=128" in w
    assert "Adam" in j["cpu_baseline"]["sample"] and j["roofline"]["kernel"].startswith("k_vstream")


@pytest.mark.parametrize("cadence", ["auto", "job"])
def test_bench_forced_distributed_one_rank_through_rccl(cadence):
    """WORLD_SIZE = 1 under torch.distributed.run with backend nccl drives the exact
    N > 1 code path of bench.py through RCCL — process group on the device, two-tier ItemSync with both
    all-reduces on the side stream (auto: fused bpr_sync_cut; job: the sharded refresh's all-gather), the
    cold message as reduce-scatter + all-gather behind the size switch — before a node ever sees it."""
    env = dict(os.environ)
    env.pop("BPR_DIST_BACKEND", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1",
           "--master-addr", "127.0.0.1", "--master-port", "29673", str(ROOT / "bench.py"), "--full", "--gpus", "1",
           "--force-dist", "--scale", "0.05", "--steps", "6", "--warmup", "2", "--no-cpu-baseline",
           "--cadence", cadence, "--sustained-epochs", "1", "--steady-epochs", "0", "--split-cold-mb", "1"]
    j = _line(subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900))
    assert j["rccl_ranks_seen"] == 1 and j["dist_backend"] == "nccl" and j["forced_distributed"] is True
    assert j["item_sync"]["all_reduces"] >= 6 and j["item_sync"]["all_reduce_ms_avg"] > 0
    if cadence == "job":
        assert j["config"]["refresh_schedule"]["sharded_over_ranks"] is True
    else:
        assert j["item_sync"]["hot"]["all_reduces"] >= 6 and j["config"]["refresh_schedule"]["lag"] == 1.0
    tr = j["trained_region"]
    steps = 6 + j["sustained"]["steps"] + tr["untimed_steps_before"] + tr["steps"]
    assert j["config"]["triples_counted_by_kernel"] == steps * j["config"]["triples_per_step_per_gpu"]


@pytest.mark.parametrize("cadence", ["auto", "job"])
def test_bench_two_ranks_over_gloo(cadence):
    env = dict(os.environ, BPR_DIST_BACKEND="gloo")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", "29671", str(ROOT / "bench.py"), "--full", "--gpus", "2",
           "--scale", "0.05", "--steps", "6", "--warmup", "2", "--no-cpu-baseline", "--cadence", cadence,
           "--sustained-epochs", "1", "--steady-epochs", "0"]
    j = _line(subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900))
    assert j["n_gpus"] == 2 and j["scaling"] == "weak" and j["value"] > 1e6
    assert j["config"]["cadence"].startswith(cadence)
    assert j["item_sync"]["all_reduces"] >= 6
    if cadence == "job":
        assert j["config"]["refresh_schedule"]["sharded_over_ranks"] is True
    else:  # lr 0.001: a full period per rank, hot tier exchanged after every launch
        assert "1 chunk(s)" in j["config"]["cadence"] and j["item_sync"]["hot"]["all_reduces"] >= 6
        assert j["config"]["refresh_schedule"]["lag"] == 1.0
    tr = j["trained_region"]
    steps = 6 + j["sustained"]["steps"] + tr["untimed_steps_before"] + tr["steps"]
    assert j["config"]["triples_counted_by_kernel"] == steps * j["config"]["triples_per_step_per_gpu"]


def test_bench_plain_line_is_lean_and_dumps_outputs(tmp_path):
    """A plain run: set up, the job on to the trained state (--trained-epochs, the last --warmup steps just before),
    exactly --steps timed steps, the line — none of --full's legs; --dump-outputs writes what the step function
    computed from the seeded inputs (the tables after steps 0 and 1, step 1 on the timed schedule) as float .npy files
    within 64 MB, and a second run with the same arguments writes them again within the spread measured below."""
    out = tmp_path / "outputs"
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--scale", "0.05", "--steps", "5", "--warmup", "3",
           "--trained-epochs", "4", "--dump-outputs", str(out)]
    j = _line(subprocess.run(cmd, capture_output=True, text=True, timeout=600))
    assert j["n_gpus"] == 1 and j["unit"] == "triples/s" and j["value"] > 1e6 and j["dtype"] == "f32"
    assert j["higher_is_better"] is True and j["steps"] == 5 and j["warmup"] == 3 and j["ms_per_step"] > 0
    spe, tps = j["config"]["steps_per_epoch"], j["config"]["triples_per_step_per_gpu"]
    tr = j["trained_region"]
    assert tr["epochs_trained_before"] == 4 and tr["first_step"] == tr["untimed_steps_before"]
    assert tr["first_step"] == tr["epochs_trained_before"] * spe + 1 and tr["plans_inside"] == 5 // spe
    assert tr["plans_added"] == 5 / spe - 5 // spe and tr["plan_ms"] > 0
    assert abs(j["value"] - 5 * tps / (5 * j["ms_per_step"] * 1e-3)) < 1e-6 * j["value"]
    assert j["config"]["triples_counted_by_kernel"] == (tr["first_step"] + 5) * tps
    assert not {"timed_region", "early_state", "sustained", "steady_state", "roofline", "roofline_atomic",
                "cpu_baseline", "cpu_baseline_c_port", "item_sync"} & set(j)
    assert "plan_epoch" not in j["config"]
    import numpy as np

    arrays = {p.stem: np.load(p) for p in out.iterdir()}
    assert sorted(arrays) == j["outputs_dumped"]["arrays"] == ["item_emb", "scalars", "user_emb_sample"]
    assert j["outputs_dumped"]["after_step"] == 1
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    assert arrays["item_emb"].shape[1] == 128 and np.isfinite(arrays["item_emb"]).all()
    assert np.isfinite(arrays["user_emb_sample"]).all() and arrays["user_emb_sample"].shape[1] == 128
    assert arrays["scalars"][3] == 2 * tps and 0 < arrays["scalars"][0] / arrays["scalars"][3] < 5
    again = tmp_path / "again"
    _line(subprocess.run(cmd[:-1] + [str(again)], capture_output=True, text=True, timeout=600))
    # the kernel applies a launch's triples concurrently: a user row two workgroups share can be read before or after
    # the other adds to it, and a few triples of the launch then draw another negative — about one SGD update on a few
    # rows, 1e-5 .. 7e-5 of the table measured; the counters agree to float rounding
    for name, a in arrays.items():
        b = np.load(again / f"{name}.npy")
        tol = 1e-6 if name == "scalars" else 5e-4
        assert a.shape == b.shape and np.linalg.norm(a - b) <= tol * np.linalg.norm(a), name
