"""What the oriented vehicle footprint (pwpp_footprint_grid) costs on one MI355X (profiles/footprint_cost.txt), and the A/B of the option
"footprint_path": "1" the yardstick, a lane per pose and then a lane per trajectory; "2" a wave per trajectory, the window's cells dealt to
the lanes.  What "0" means (pwpp_footprint_path_of, pwpp_footprint.hip) follows from the last lines of the output, which also check it.

  * the workload of tools/route_cost.py: `frames` replayed KITTI frames in device memory, their terrain cost bytes at radius 1 on 256 x 256
    cells of 0.5 m, the obstacle distances of pwpp_distance_obstacles and the unlimited field of pwpp_reach_grid from the sensor's cell;
    every image is a device array.
  * a shared fan (n_sets = 1) of 64 arcs x 32 poses from the sensor's cell: curvatures -0.2 .. 0.2 per metre, 0.5 m a step, the poses by
    pwpp_footprint_pose.  Two footprints on a rear axle: 9 x 4 cells (front 108, rear 36, half_width 32 ticks: 4.5 m x 2 m) and 36 x 16
    cells (432, 144, 128).  clearance2 = 1 with dist2.
  * every case with and without dist2, reach and pose rows; path 1, path 1 again (the A/A twin, whose distance from the first is the floor
    no difference can be read below), path 2 and path 0, the library's choice between them.
  * pwpp_plan_grid (16 starts, look 64, reach kept on the device) followed by pwpp_footprint_grid on its cost and reach in one enqueued
    sequence, against pwpp_plan_grid alone: the footprints' cost on top of the plan.
  * the host alternative the stage replaces: cost, dist2 and reach copied to the host (9 bytes a cell) and the one text run there in C++:
    tools/footprint_check.cpp built with -O2, its dump mode (the serial deal, one thread), which reports the time of the fold alone.
  Every figure is the median over `steps` rounds; a round runs each variant once, in turn (interleaved), every other round in reversed
  order.  One measurement = `reps` calls enqueued back to back and one synchronise, timed with the host clock and divided by `reps`.
  The condition on path 0: slower than path 1 in no case beyond the floor (|path 1 - its twin|) and the spread of the rounds.

    python tools/footprint_cost.py [--frames 1024] [--steps 5] [--warmup 1] [--reps 4]
"""
import argparse
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("tests", "patchwork-plusplus_amd/python", "tools", ""):
    sys.path.insert(0, os.path.join(ROOT, p))
import numpy as np  # noqa: E402
import torch  # noqa: E402  (before libpwpp_hip: see tests/conftest.py)

import bench  # noqa: E402
import pwpp_hip  # noqa: E402
from point_records_cost import device_batch  # noqa: E402

N, CELL = 256, 0.5
LIMITS = (0.2, 0.3, 0.05)
BASE, LETHAL, UNKNOWN = 10, 100, 50
BAND = (0.3, 2.5)
ARCS, STEPS, STEP_M, CURVATURE = 64, 32, 0.5, 0.2
FOOTPRINTS = (("9 x 4 cells", (108, 36, 32)), ("36 x 16 cells", (432, 144, 128)))


def fan(grid):
    """(1, ARCS, STEPS, 4) poses: arcs of constant curvature from the sensor's cell, heading +x at the start."""
    q = np.zeros((1, ARCS, STEPS, 4), np.int32)
    cx = grid.x0 + (N // 2 + 0.5) * CELL
    for j in range(ARCS):
        k = CURVATURE * (2.0 * j / (ARCS - 1) - 1.0)
        for i in range(STEPS):
            s = (i + 1) * STEP_M
            x, y = (np.sin(k * s) / k, (1.0 - np.cos(k * s)) / k) if abs(k) > 1e-9 else (s, 0.0)
            q[0, j, i] = pwpp_hip.footprint_pose(grid, cx + x, cx + y, k * s)
    return q


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "footprint_cost.txt"))
    a = ap.parse_args()
    lines = []

    def out(s=""):
        print(s, flush=True)
        lines.append(s)

    src, kind = bench.load_source_frames("kitti")
    F = a.frames
    big, ptrs, ns, _ = device_batch(src, F, "row4")
    cells = F * N * N
    d_cost = torch.empty(cells, dtype=torch.int8, device="cuda")
    d_dist2, d_reach = torch.empty(cells, dtype=torch.int32, device="cuda"), torch.empty(cells, dtype=torch.int32, device="cuda")
    d_prow, d_trow = torch.empty(F * ARCS * STEPS * 8, dtype=torch.int32, device="cuda"), torch.empty(F * ARCS * 8, dtype=torch.int32, device="cuda")
    d_routes, d_wps = torch.empty(F * 16 * 8, dtype=torch.int32, device="cuda"), torch.empty(F * 16 * 64, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    x0 = -0.5 * N * CELL
    grid = pwpp_hip.GroundGrid(x0, x0, CELL, N, N, 0, 0)
    tp = pwpp_hip.TerrainParams(1, 3, LIMITS[0], LIMITS[1], LIMITS[2], 0)
    rp = lambda with_d2=False: pwpp_hip.ReachParams(BASE, LETHAL, UNKNOWN, 1 if with_d2 else 0, 0, 0)
    qp = pwpp_hip.RouteParams(0, 64, 64, 0)
    poses = fan(grid)
    src_cell = (N // 2, N // 2)
    starts = np.array([(N // 2 + int(round(24 * np.cos(k * np.pi / 8))), N // 2 + int(round(24 * np.sin(k * np.pi / 8)))) for k in range(16)], np.int32)

    def timed(enqueue, sync, reps):
        t0 = time.perf_counter()
        for _ in range(reps):
            enqueue()
        sync()
        return (time.perf_counter() - t0) * 1e6 / reps

    h = pwpp_hip.Handle()
    h.submit_batch(ptrs, ns, 4, pwpp_hip.LAYOUT_ROW_MAJOR, pwpp_hip.MEM_DEVICE, pwpp_hip.MODE_FRESH)
    h.synchronize()
    h.terrain_ground_device(x0, x0, CELL, N, N, tp, 0, 0, 0, 0, d_cost.data_ptr(), 0, 0, F)
    h.distance_obstacles_device(x0, x0, CELL, N, N, BAND[0], BAND[1], 1, 0, d_dist2.data_ptr(), 0, 0, 0, 0, F)
    h.reach_grid_device(N, N, F, d_cost.data_ptr(), src_cell, rp(), d_reach.data_ptr())
    h.synchronize()

    def foot(ext, with_d2, with_reach, with_rows, path):
        fp = pwpp_hip.FootprintParams(ext[0], ext[1], ext[2], 0, (0, 0))

        def enqueue():
            h.footprint_grid_device(N, N, F, d_cost.data_ptr(), rp(with_d2), fp, poses, pose_rows_ptr=d_prow.data_ptr() if with_rows else 0, traj_rows_ptr=d_trow.data_ptr(),
                                    dist2_ptr=d_dist2.data_ptr() if with_d2 else 0, reach_ptr=d_reach.data_ptr() if with_reach else 0)

        def go():
            h.set_option("footprint_path", path)
            return timed(enqueue, h.synchronize, a.reps)
        return go, enqueue

    def plan(ext, path):
        """pwpp_plan_grid alone (ext None) or followed by the footprints on its cost and reach, one enqueued sequence"""
        follow = foot(ext, False, True, False, path)[1] if ext else (lambda: None)

        def go():
            h.set_option("footprint_path", path)
            return timed(lambda: (h.plan_grid_device(N, N, F, d_cost.data_ptr(), src_cell, rp(), starts, qp, d_routes.data_ptr(), 0, d_wps.data_ptr(), reach_ptr=d_reach.data_ptr()),
                                  follow()), h.synchronize, 2)
        return go

    out("python tools/footprint_cost.py --frames %d --steps %d --warmup %d --reps %d" % (F, a.steps, a.warmup, a.reps))
    out("footprint_cost: %s, %d frames of %d x %d cells of %g m, %s" % (kind, F, N, N, CELL, torch.cuda.get_device_name(0)))
    out("terrain cost at radius 1, min_known 3, limits %s; reach: base %d, lethal %d, unknown %d, clearance2 1 with dist2; a shared fan of %d arcs x %d poses, %g m a step, "
        "curvature up to %g per metre" % (LIMITS, BASE, LETHAL, UNKNOWN, ARCS, STEPS, STEP_M, CURVATURE))
    for name, ext in FOOTPRINTS:
        for with_d2 in (False, True):
            h.set_option("footprint_path", 1)
            foot(ext, with_d2, True, True, 1)[1]()
            h.synchronize()
            rows = d_prow.cpu().numpy().view(pwpp_hip.FOOT_POSE_DTYPE)
            trow = d_trow.cpu().numpy().view(pwpp_hip.FOOT_TRAJ_DTYPE)
            out("  %-13s %s dist2: %d poses, %d free, %d hit; %.1f cells covered a pose, %.1f outside; %d trajectories, %d with a hit, %.1f free steps a trajectory"
                % (name, "with" if with_d2 else "without", rows.size, int((rows["status"] == 0).sum()), int((rows["status"] == 1).sum()), float(rows["covered"].mean()),
                   float(rows["outside"].mean()), trow.size, int((trow["first_hit"] >= 0).sum()), float(trow["free_steps"].mean())))
    out("us per call: host clock over %d calls (2 for the sequences with pwpp_plan_grid) enqueued back to back + one synchronise; median of %d interleaved rounds "
        "(every other one reversed) after %d warm-up rounds" % (a.reps, a.steps, a.warmup))
    out()

    variants, cases = [], []
    for name, ext in FOOTPRINTS:
        for with_d2 in (False, True):
            for with_reach in (False, True):
                for with_rows in (False, True):
                    what = "%s, %s dist2, %s reach, %s pose rows" % (name, "with" if with_d2 else "no", "with" if with_reach else "no", "with" if with_rows else "no")
                    cases.append(what)
                    for label, path in (("path 1", 1), ("path 1 twin", 1), ("path 2", 2), ("path 0", 0)):
                        variants.append(("pwpp_footprint_grid %s, %s" % (what, label), foot(ext, with_d2, with_reach, with_rows, path)[0]))
    extra = len(variants)
    variants.append(("pwpp_plan_grid 16 starts, look 64, reach to the caller", plan(None, 1)))
    for name, ext in FOOTPRINTS:
        for path in (1, 2):
            variants.append(("pwpp_plan_grid + pwpp_footprint_grid %s on its reach, footprint_path %d" % (name, path), plan(ext, path)))
    t = [[] for _ in variants]
    for rnd in range(a.warmup + a.steps):
        order = range(len(variants)) if rnd % 2 == 0 else range(len(variants) - 1, -1, -1)
        for k in order:
            v = variants[k][1]()
            if rnd >= a.warmup:
                t[k].append(v)
        print("round %d of %d done" % (rnd + 1, a.warmup + a.steps), file=sys.stderr, flush=True)
    h.set_option("footprint_path", 0)
    med = [float(np.median(x)) for x in t]
    for (name, _), x, m in zip(variants, t, med):
        out("  %-100s %11.1f us   [%11.1f .. %11.1f]" % (name, m, min(x), max(x)))
    out()

    # the host alternative: the images through host memory, the fold in C++ on the host
    th = []
    for _ in range(3):
        t0 = time.perf_counter()
        cost_host, dist2_host, reach_host = d_cost.cpu().numpy(), d_dist2.cpu().numpy(), d_reach.cpu().numpy()
        th.append((time.perf_counter() - t0) * 1e6)
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "footprint_check")
        subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "patchwork-plusplus_amd", "csrc"), os.path.join(ROOT, "tools", "footprint_check.cpp"),
                        "-o", exe], check=True)
        files = {}
        for name, arr in (("cost", cost_host), ("dist2", dist2_host), ("reach", reach_host), ("poses", poses)):
            files[name] = os.path.join(tmp, name)
            arr.tofile(files[name])
        for name, ext in FOOTPRINTS:
            r = subprocess.run([exe, "dump", files["cost"], str(N), str(N), str(F), str(BASE), str(LETHAL), str(UNKNOWN), "1", files["dist2"], files["reach"], str(ext[0]), str(ext[1]),
                                str(ext[2]), "0", files["poses"], "1", str(ARCS), str(STEPS), "1", "0", os.path.join(tmp, "out")], check=True, capture_output=True, text=True)
            fold_us = float(r.stdout.split("folded in ")[1].split(" us")[0])
            out("the host alternative, %s: cost, dist2 and reach brought to the host (%.0f MB) %.1f us (of 3 copies: %.1f .. %.1f) + the fold of %d poses in C++ on the host (one "
                "thread) %.1f us = %.1f us" % (name, cells * 9 / 1e6, float(np.median(th)), min(th), max(th), F * ARCS * STEPS, fold_us, float(np.median(th)) + fold_us))
    out()

    slower = faster = slower0 = 0
    total = [0.0, 0.0, 0.0]
    for ci, what in enumerate(cases):
        k1, kt, k2, k0 = 4 * ci, 4 * ci + 1, 4 * ci + 2, 4 * ci + 3
        floor = abs(med[k1] - med[kt])
        spread = max(max(t[k]) - min(t[k]) for k in (k1, k2, k0))
        out("pwpp_footprint_grid %s: path 1 %.1f us, its twin %.1f us, path 2 %.1f us, path 0 %.1f us: path 1 - path 2 = %.1f us, path 1 - path 0 = %.1f us against a floor of %.1f us "
            "and a spread of %.1f us" % (what, med[k1], med[kt], med[k2], med[k0], med[k1] - med[k2], med[k1] - med[k0], floor, spread))
        faster += med[k1] - med[k2] > max(floor, spread)
        slower += med[k2] - med[k1] > max(floor, spread)
        slower0 += med[k0] - med[k1] > max(floor, spread)
        total[0] += med[k1]
        total[1] += med[k2]
        total[2] += med[k0]
    alone = med[extra]
    for i, (name, _) in enumerate(FOOTPRINTS):
        p1, p2 = med[extra + 1 + 2 * i], med[extra + 2 + 2 * i]
        out("pwpp_plan_grid + pwpp_footprint_grid %s: %.1f us (footprint_path 1), %.1f us (footprint_path 2) against pwpp_plan_grid alone %.1f us: the footprints on top %.1f / %.1f us"
            % (name, p1, p2, alone, p1 - alone, p2 - alone))
    out()
    out("path 2 beats path 1 by more than floor and spread in %d of %d cases and loses by more in %d; over the cases path 1 sums to %.1f us, path 2 to %.1f us and path 0 to "
        "%.1f us; path 0 is slower than path 1 by more than floor and spread in %d cases: %s"
        % (faster, len(cases), slower, total[0], total[1], total[2], slower0, "the choice stands" if slower0 == 0 else "path 0 should be path 1"))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    del big


if __name__ == "__main__":
    main()
