"""CPU: `python bench.py --gpus 2` spawns its own two ranks (rfdnet_amd/sharding.launch_local_ranks),
shards scenes with sharding.scene_ids_for_rank, counts a failing scene instead of dying, gathers the
statistics over gloo and prints ONE JSON line with n_gpus = 2.  RFD_BENCH_STUB=1 swaps the HIP scene for
a CPU stand-in -- this exercises the launcher and the accounting, not the kernels."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(argv, **env):
    e = dict(os.environ, RFD_BENCH_STUB="1", **env)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        if k not in env:
            e.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + argv, env=e, capture_output=True,
                       text=True, timeout=300)
    return p


def test_self_launch_two_ranks_and_failure_accounting():
    p = run_bench(["--gpus", "2", "--steps", "3", "--warmup", "1", "--in-flight", "2"],
                  RFD_BENCH_STUB_FAIL="9")
    assert p.returncode == 0, p.stderr
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout                     # rank 0 only, one line
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 3 and out["warmup"] == 1
    c = out["config"]
    assert c["scenes_per_step"] == 4                     # 2 ranks x 2 in flight
    assert c["scenes_failed"] == 1 and c["scenes_done"] == 3 * 4 - 1      # scene 9 is in the timed region
    assert "scene(s) [9] failed" in p.stderr
    assert out["scaling"] == "weak" and out["unit"] == "scenes/s" and out["value"] > 0
    assert "cpu_baseline" not in out                     # rank-0-at-N=1 only


def test_single_process_default():
    p = run_bench(["--steps", "2", "--warmup", "0", "--no-cpu-baseline"])
    assert p.returncode == 0, p.stderr
    out = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][0])
    # two steps of the default four scenes in flight
    assert out["n_gpus"] == 1 and out["config"]["scenes_failed"] == 0 and out["config"]["scenes_done"] == 8
    assert out["config"]["scenes_in_flight_per_gpu"] == 4


def test_world_size_mismatch_fails_loudly():
    p = run_bench(["--gpus", "4"], WORLD_SIZE="2", RANK="0", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1",
                  MASTER_PORT="29999")
    assert p.returncode != 0 and "WORLD_SIZE=2" in p.stderr


def test_every_scene_is_run_exactly_once_across_ranks_and_workers():
    from rfdnet_amd import sharding
    world, S, NB, steps, warm = 4, 3, 2, 5, 2
    per_step = S * NB * world
    seen = []
    for rank in range(world):
        lo, hi = warm * per_step, (warm + steps) * per_step
        mine = [i for i in sharding.scene_ids_for_rank(hi, rank, world) if i >= lo]
        assert all(i % world == rank for i in mine)
        for w in range(S):
            for ids in sharding.scene_ids_for_worker(mine, w, S, NB):
                assert len(ids) == NB
                seen += ids
    assert sorted(seen) == list(range(warm * per_step, (warm + steps) * per_step))


def test_failing_rank_takes_the_job_down(tmp_path):
    from rfdnet_amd import sharding
    script = tmp_path / "r.py"
    script.write_text("import os, sys, time\n"
                      "if os.environ['RANK'] == '1': sys.exit(3)\n"
                      "time.sleep(60)\n")
    rc = sharding.launch_local_ranks(str(script), [], 2)
    assert rc == 3


def test_eight_ranks_over_gloo_dry_run(tmp_path):
    """configs[3] / [4] shape without the node: 8 ranks (stub scenes, gloo), one scene in flight per rank;
    every rank's scenes are its residue class, the job's throughput is paced by the slowest rank, the per-scene
    statistics file of every rank is written."""
    stats = str(tmp_path / "scenes.json")
    p = run_bench(["--gpus", "8", "--steps", "5", "--warmup", "1", "--in-flight", "1", "--stats-out", stats],
                  RFD_BENCH_STUB_SLOW_RANK="5")
    assert p.returncode == 0, p.stderr
    out = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][0])
    assert out["n_gpus"] == 8 and out["config"]["scenes_per_step"] == 8 and out["config"]["scenes_done"] == 40
    # rank 5 sleeps 10x longer per scene: 5 scenes x 20 ms is the floor of the job's time
    assert out["ms_per_step"] >= 19.0, out["ms_per_step"]
    for r in range(8):
        d = json.load(open(stats if r == 0 else "%s.rank%d" % (stats, r)))
        ids = sorted(i for s in d["scenes"] for i in s["scenes"])
        assert ids == list(range(8 + r, 48, 8)), (r, ids)            # warm-up step = scenes 0..7


def test_scene_to_rank_map_of_the_scannet_test_split():
    """datasets/splits/fullscan/scannetv2_test.json holds 311 scans; scene i -> rank i mod 8."""
    from rfdnet_amd import sharding
    n, world = 311, 8
    parts = [sharding.scene_ids_for_rank(n, r, world) for r in range(world)]
    assert sorted(i for p in parts for i in p) == list(range(n))
    assert [len(p) for p in parts] == [39, 39, 39, 39, 39, 39, 39, 38]
    assert all(i % world == r for r, p in enumerate(parts) for i in p)


def test_job_throughput_is_paced_by_the_slowest_rank():
    import numpy as np
    from rfdnet_amd import sharding
    F = sharding.STAT_FIELDS
    g = np.zeros((8, len(F)))
    g[:, F.index("steps")] = 39
    g[:, F.index("elapsed_s")] = [2.0, 2.1, 1.9, 2.0, 2.0, 3.0, 2.0, 2.0]
    v, t = sharding.job_throughput(g)
    assert t == 3.0 and abs(v - 8 * 39 / 3.0) < 1e-12


def test_numa_cpu_list_from_a_fake_topology(tmp_path):
    """launch_local_ranks pins rank r to the CPUs of GPU r's NUMA node (KFD topology -> PCI -> node cpulist)."""
    from rfdnet_amd import sharding
    root = tmp_path
    for i, props in enumerate(("simd_count 0\n", "simd_count 1024\nlocation_id 1280\ndomain 0\n",
                               "simd_count 1024\nlocation_id 34304\ndomain 0\n")):
        d = root / "class" / "kfd" / "kfd" / "topology" / "nodes" / str(i)
        d.mkdir(parents=True)
        (d / "properties").write_text(props)
    for bdf, node in (("0000:05:00.0", "0"), ("0000:86:00.0", "1")):
        d = root / "bus" / "pci" / "devices" / bdf
        d.mkdir(parents=True)
        (d / "numa_node").write_text(node + "\n")
    for node, cl in (("node0", "0-3,16-19"), ("node1", "4-7")):
        d = root / "devices" / "system" / "node" / node
        d.mkdir(parents=True)
        (d / "cpulist").write_text(cl + "\n")
    assert sharding.numa_cpus_for_gpu(0, str(root)) == [0, 1, 2, 3, 16, 17, 18, 19]
    assert sharding.numa_cpus_for_gpu(1, str(root)) == [4, 5, 6, 7]
    assert sharding.numa_cpus_for_gpu(2, str(root)) is None            # no such GPU: leave the affinity alone


def test_pinning_respects_the_allowed_cpuset_and_device_remapping(tmp_path, monkeypatch):
    """the NUMA cpulist is intersected with the launcher's own allowed set (a cpuset-confined
    container: sched_setaffinity would fail with EINVAL), skipped when the intersection is empty, translated through
    HIP_ / ROCR_VISIBLE_DEVICES and skipped when those cannot be translated; the preexec hook never raises."""
    import os
    from rfdnet_amd import sharding
    root = tmp_path / "sys"
    nodes = root / "class" / "kfd" / "kfd" / "topology" / "nodes"
    for i, (simd, loc) in enumerate([(0, 0), (256, 0x0500), (256, 0x2500)]):
        d = nodes / str(i)
        d.mkdir(parents=True)
        (d / "properties").write_text("simd_count %d\nlocation_id %d\ndomain 0\n" % (simd, loc))
    for bdf, node in (("0000:05:00.0", "0"), ("0000:25:00.0", "1")):
        d = root / "bus" / "pci" / "devices" / bdf
        d.mkdir(parents=True)
        (d / "numa_node").write_text(node + "\n")
    for n, cl in ((0, "0-3"), (1, "4-7")):
        d = root / "devices" / "system" / "node" / ("node%d" % n)
        d.mkdir(parents=True)
        (d / "cpulist").write_text(cl + "\n")
    sr = str(root)
    monkeypatch.setattr(os, "sched_getaffinity", lambda pid: {2, 3, 4, 5})
    assert sharding.pin_cpus_for_rank(0, {}, sr) == [2, 3]                       # node 0 = 0-3, allowed 2-5
    assert sharding.pin_cpus_for_rank(1, {}, sr) == [4, 5]
    monkeypatch.setattr(os, "sched_getaffinity", lambda pid: {8, 9})
    assert sharding.pin_cpus_for_rank(0, {}, sr) is None                         # empty intersection: leave it alone
    monkeypatch.setattr(os, "sched_getaffinity", lambda pid: set(range(16)))
    assert sharding.pin_cpus_for_rank(0, {"HIP_VISIBLE_DEVICES": "1,0"}, sr) == [4, 5, 6, 7]    # device 0 = physical GPU 1
    assert sharding.pin_cpus_for_rank(0, {"ROCR_VISIBLE_DEVICES": "1"}, sr) == [4, 5, 6, 7]
    assert sharding.pin_cpus_for_rank(0, {"ROCR_VISIBLE_DEVICES": "1,0", "HIP_VISIBLE_DEVICES": "1"}, sr) == [0, 1, 2, 3]
    assert sharding.pin_cpus_for_rank(0, {"CUDA_VISIBLE_DEVICES": "1", "HIP_VISIBLE_DEVICES": "0"}, sr) == [0, 1, 2, 3]
    assert sharding.pin_cpus_for_rank(0, {"ROCR_VISIBLE_DEVICES": "GPU-deadbeef"}, sr) is None  # UUIDs: skip pinning
    assert sharding.pin_cpus_for_rank(3, {"HIP_VISIBLE_DEVICES": "0"}, sr) is None               # out of range
    assert sharding.visible_device_index(2, {}) == 2

    def boom(pid, cpus):
        raise OSError(22, "Invalid argument")
    monkeypatch.setattr(os, "sched_setaffinity", boom)
    sharding._pin([0, 1])                                                       # swallowed


def test_a_rank_that_cannot_be_spawned_takes_the_started_ranks_with_it(tmp_path, monkeypatch):
    """no orphan: if Popen fails for rank 1, rank 0 (already running) is terminated before the error propagates"""
    import subprocess
    import sys
    import pytest
    from rfdnet_amd import sharding
    script = tmp_path / "sleeper.py"
    script.write_text("import time\ntime.sleep(60)\n")
    started = []
    real = subprocess.Popen

    def popen(*a, **k):
        if started:
            raise OSError("cannot spawn")
        p = real(*a, **k)
        started.append(p)
        return p
    monkeypatch.setattr(sharding.subprocess, "Popen", popen)
    with pytest.raises(OSError):
        sharding.launch_local_ranks(str(script), [], 2, env={"RFD_PIN_NUMA": "0"})
    assert started and started[0].poll() is not None


def test_numa_lookup_skips_kfd_nodes_it_may_not_read(tmp_path):
    """Inside a container only the job's own GPUs are readable under /sys/class/kfd: the other nodes' `properties`
    raise EPERM (seen on the MI355X boxes: nodes 8, 9) or are empty.  The lookup must skip them instead of giving up
    (round 3's version returned None there, so no rank was ever pinned on those boxes)."""
    from rfdnet_amd import sharding
    root = tmp_path / "sys"
    nodes = root / "class" / "kfd" / "kfd" / "topology" / "nodes"
    for i in range(4):
        (nodes / str(i)).mkdir(parents=True)
    (nodes / "0" / "properties").write_text("simd_count 0\nlocation_id 0\ndomain 0\n")      # the CPU node
    (nodes / "1" / "properties").write_text("")                                                 # hidden GPU: empty
    (nodes / "2" / "properties").write_text("simd_count 1024\nlocation_id 61696\ndomain 0\n") # ours: 0000:f1:00.0
    # node 3: no properties file at all (open() raises, like EPERM)
    d = root / "bus" / "pci" / "devices" / "0000:f1:00.0"
    d.mkdir(parents=True)
    (d / "numa_node").write_text("1\n")
    n1 = root / "devices" / "system" / "node" / "node1"
    n1.mkdir(parents=True)
    (n1 / "cpulist").write_text("64-127,192-255\n")
    cpus = sharding.numa_cpus_for_gpu(0, str(root))
    assert cpus is not None and cpus[0] == 64 and cpus[-1] == 255 and len(cpus) == 128


def test_preflight_over_eight_gloo_ranks(tmp_path):
    """`bench.py --preflight --gpus 8` -- every rank checks its devices, joins ONE all-gather over
    the job's backend and reports its affinity / hardware-queue settings; rank 0 prints one JSON line, exit code 0."""
    import time
    t0 = time.time()
    p = run_bench(["--preflight", "--gpus", "8"], GPU_MAX_HW_QUEUES="16")
    assert p.returncode == 0, p.stderr
    assert time.time() - t0 < 60
    out = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][0])
    assert out["preflight"] == "ok" and out["n_gpus"] == 8
    assert [int(r["rank"]) for r in out["ranks"]] == list(range(8))
    assert all(int(r["hw_queues"]) == 16 and int(r["visible_devices"]) == 8 for r in out["ranks"])


def test_preflight_fails_on_every_rank_with_one_actionable_line_when_there_are_fewer_devices_than_ranks():
    """8 ranks, 4 visible devices: no rank may sit in the rendezvous -- each one sees the mismatch by itself, prints the
    line that says what to do and exits non-zero, well inside 60 s."""
    import time
    t0 = time.time()
    p = run_bench(["--preflight", "--gpus", "8"], RFD_PREFLIGHT_FAKE_DEVICES="4")
    assert p.returncode != 0
    assert time.time() - t0 < 60
    lines = [l for l in p.stderr.splitlines() if l.startswith("preflight FAILED")]
    assert lines and all("8 ranks on this node but 4 visible GPU(s)" in l and "--nproc-per-node 4" in l for l in lines)
    assert not [l for l in p.stdout.splitlines() if l.startswith("{")]


def test_preflight_watchdog_ends_a_rank_whose_peers_never_arrive():
    """a rank alone in a world of 2 (its peer was never started): the rendezvous cannot complete; the rank must not
    hang -- one actionable line, non-zero exit, inside the deadline"""
    import time
    from rfdnet_amd import sharding
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from rfdnet_amd import sharding\n"
            "sharding.preflight(0, 0, 2, stub=True, deadline_s=6.0)\n" % ROOT)
    env = dict(os.environ, RANK="0", LOCAL_RANK="0", WORLD_SIZE="2", LOCAL_WORLD_SIZE="2", MASTER_ADDR="127.0.0.1",
               MASTER_PORT=str(sharding.free_port()))
    t0 = time.time()
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and time.time() - t0 < 40
    assert "preflight FAILED [rank 0]" in p.stderr


def test_scenes_flag_sweeps_the_311_scan_split_over_eight_ranks(tmp_path):
    """`bench.py --config mise128 --scenes 311 --gpus 8` = BASELINE configs[4] in one command: scene j of the sweep ->
    rank j mod 8 (39 x 7 + 38), every scene exactly once, steps derived from the scene count."""
    stats = str(tmp_path / "sweep.json")
    p = run_bench(["--config", "mise128", "--scenes", "311", "--gpus", "8", "--warmup", "1", "--in-flight", "4",
                   "--stats-out", stats])
    assert p.returncode == 0, p.stderr
    out = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][0])
    assert out["n_gpus"] == 8 and out["config"]["scenes_done"] == 311 and out["config"]["sweep_scenes"] == 311
    assert out["steps"] == 10                               # ceil(311 / (8 ranks x 4 in flight))
    first = 1 * 8 * 4                                       # the warm-up step's scenes come first
    seen = []
    for r in range(8):
        d = json.load(open(stats if r == 0 else "%s.rank%d" % (stats, r)))
        ids = sorted(i for s in d["scenes"] for i in s["scenes"])
        assert ids == [first + j for j in range(r, 311, 8)], r
        seen += ids
    assert sorted(seen) == list(range(first, first + 311))


def test_dump_outputs_of_the_last_step_and_the_lean_default(tmp_path):
    """`--dump-outputs DIR` writes what the last timed step returned, rank 0 as <name>.npy and rank r as rank<r>_<name>.npy,
    as float arrays; the same command writes the same files.  Without --full nothing is measured after the timed region."""
    import numpy as np
    for d in ("a", "b"):
        p = run_bench(["--gpus", "2", "--steps", "2", "--warmup", "1", "--in-flight", "2", "--dump-outputs", str(tmp_path / d)])
        assert p.returncode == 0, p.stderr
        out = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][0])
        assert out["steps"] == 2 and out["ms_per_step"] > 0 and "single_scene" not in out and "cpu_baseline" not in out
    # scenes 0-3 warm up, 4-7 and 8-11 are the two timed steps: the last one's scenes, split over 2 ranks x 2 workers
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["rank1_scene11_stub.npy", "rank1_scene9_stub.npy", "scene10_stub.npy", "scene8_stub.npy"]
    for n in names:
        a = np.load(tmp_path / "a" / n)
        assert a.dtype == np.float64 and np.array_equal(a, np.load(tmp_path / "b" / n))


def test_dump_outputs_samples_what_does_not_fit(tmp_path):
    """64 MB in all: an array larger than its share is written as a seeded sample of its rows plus the row indices"""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    big = torch.arange(3 * 10 ** 7, dtype=torch.int32).reshape(-1, 3)
    logits = torch.linspace(-1, 1, 2 * 10 ** 7)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), [("faces", big), ("logits", logits), ("ends", [0, 5, 9])])
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["ends.npy", "faces.npy", "faces_rows.npy", "logits.npy", "logits_rows.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in names) <= 64 * 10 ** 6
    for name, full in (("faces", big.numpy()), ("logits", logits.numpy())):
        rows = np.load(tmp_path / "a" / (name + "_rows.npy"))
        got = np.load(tmp_path / "a" / (name + ".npy"))
        assert rows.dtype == np.float64 and np.all(np.diff(rows) > 0) and len(rows) > 10 ** 5
        assert got.dtype == (np.float64 if name == "faces" else np.float32)
        assert np.array_equal(got, full[rows.astype(np.int64)])
        assert np.array_equal(rows, np.load(tmp_path / "b" / (name + "_rows.npy")))
    assert np.array_equal(np.load(tmp_path / "a" / "ends.npy"), [0.0, 5.0, 9.0])
