"""world_size-2 gloo test of the N>1 bookkeeping bench.py uses (no GPU needed)."""
import os
import socket

import torch.multiprocessing as mp


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    os.environ.update(WORLD_SIZE=str(world), RANK=str(rank), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                    "patchwork-plusplus_amd", "python"))
    import pwpp_dist
    w, r, lr = pwpp_dist.init("gloo")
    assert (w, r, lr) == (world, rank, rank)
    shard = pwpp_dist.shard_sources(6, 8, rank)
    pwpp_dist.barrier()
    elapsed, frames = pwpp_dist.aggregate(1.0 + rank, len(shard) * 3)
    per_rank = pwpp_dist.gather_values(100.0 * (rank + 1))  # every rank's own rate, in rank order
    info = pwpp_dist.describe("gloo")  # the "dist" record of the N > 1 bench line
    assert info["world_size"] == world and info["backend"] == "gloo" and [d["rank"] for d in info["devices"]] == list(range(world))
    q.put((rank, shard, elapsed, frames, per_rank))
    pwpp_dist.finalize()


def test_two_rank_aggregation():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    out = sorted(q.get(timeout=120) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert out[0][1] == [0, 1, 2, 3, 4, 5, 0, 1] and out[1][1] == [1, 2, 3, 4, 5, 0, 1, 2]
    for _, _, elapsed, frames, per_rank in out:
        assert elapsed == 2.0      # MAX over ranks
        assert frames == 48        # SUM over ranks: whole-job frames
        assert per_rank == [100.0, 200.0]  # bench.py's "per_gpu" list


def test_single_process_passthrough():
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                    "patchwork-plusplus_amd", "python"))
    import pwpp_dist
    assert pwpp_dist.aggregate(0.5, 7) == (0.5, 7)
    assert pwpp_dist.gather_values(3.5) == [3.5]
    assert pwpp_dist.shard_sources(6, 4, 5) == [5, 0, 1, 2]


def test_bench_spawns_its_own_ranks_when_started_bare():
    """`python bench.py --gpus 2` as a plain process (the way the driver starts --gpus 1): bench.py must become the launcher.
    Without a GPU every rank stops at "needs a GPU" -- what is checked here is that TWO ranks were started and said so."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["PWPP_BENCH_ECHO_RANK"] = "1"
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "1"], env=env, cwd=root,
                         capture_output=True, text=True, timeout=600)
    seen = sorted(l for l in out.stderr.splitlines() if l.startswith("bench rank "))
    assert seen == ["bench rank 0 of 2 (self-spawned)", "bench rank 1 of 2 (self-spawned)"], out.stderr[-2000:]
    import torch
    if not torch.cuda.is_available():
        assert out.returncode != 0 and "needs a GPU" in out.stderr


def test_bench_memory_estimate_is_checked_before_any_collective():
    """bench.py --gpus N compares the rank's free HBM with an estimate of what the workload takes BEFORE RCCL is initialised (VERDICT r05
    item 8): the estimate is a plain function of the arguments -- sane for the headline (tens of GB on one GPU with the extra legs, under
    20 GB per rank at N = 8), growing with the frames, and the check sits in front of pwpp_dist.init in main()."""
    import importlib.util
    import types
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_for_test", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    a = types.SimpleNamespace(workload="kitti", in_flight=2, frames=1024, gpus=1, full=True, skip_extras=False, dense_frames=1024,
                              distinct_frames=1024)
    one = bench.estimate_memory_gb(a)
    a.full = False  # a plain run holds the headline's buffers and handles only
    assert 10.0 < bench.estimate_memory_gb(a) < 30.0
    a.full = True
    a.gpus = 8
    eight = bench.estimate_memory_gb(a)
    assert 60.0 < one < 288.0 and 10.0 < eight < 30.0
    a.frames = 4096
    assert bench.estimate_memory_gb(a) > 3.0 * eight
    src = open(os.path.join(root, "bench.py")).read()
    assert src.index("estimate_memory_gb(args)") < src.index("pwpp_dist.init(backend, dev)")
