"""What the routes on the reach field (pwpp_route_grid, pwpp_plan_grid) cost on one MI355X (profiles/route_cost.txt), and the A/B of the
option "route_path": "1" the yardstick, a lane per route, wholly serial; "2" a wave per route, the route's last cells in LDS, the
shortcut candidates dealt to the lanes.  What "0" means (kRouteDefaultWaves, pwpp_route.hip) follows from the last lines of the output.

  * the workload of tools/reach_cost.py: `frames` replayed KITTI frames in device memory, their terrain cost bytes at radius 1 on
    256 x 256 cells of 0.5 m and on 64 x 64 cells of 2 m, the source at the sensor's cell, the unlimited field of pwpp_reach_grid and its
    from image; every image is a device array.
  * pwpp_route_grid alone on that from: 1 and 16 starts per frame (on a circle of 12 m round the sensor, the same for every frame), look
    16 and 64, line_cost 0 (the terrain's byte is rarely 0: nearly every line fails, every search tests all its candidates) and 100 (every
    passable cell may be crossed: the far candidates are clear and the search ends early), 64 waypoints and no cell list; path 1, path 1 again (the A/A twin: the same variant under another name, whose distance
    from the first is the floor no difference can be read below) and path 2.
  * what a call achieves against its ceiling.  A route is a dependent chain: one L2 or HBM access per hop, about 200 or 900 cycles by
    the microarchitecture tables.  A call cannot end before its longest route has taken its hops, so `us per call / hops of the longest
    route` is the time per dependent hop the call achieved: compare with 0.08 us (L2) and 0.38 us (HBM) at 2.4 GHz.  The HBM roofline
    says nothing here: the bytes are few.
  * pwpp_plan_grid (16 starts, look 64) without the field's images against pwpp_reach_grid with from on the same handle, box and
    inputs, unlimited and with max_reach at 20 m of free ground: the routes' cost on top of the field.  The reach kernels are the
    parent commit's, unchanged.
  * the host alternative the stage replaces: pwpp_reach_grid in PWPP_MEM_HOST, reach and from brought to the host (8 bytes a cell), plus
    the walk in C++ on the host: tools/route_check.cpp built with -O2, its dump mode on that from (16 starts, look 64, the serial deal,
    one thread), which reports the time of the walks alone.
  Every figure is the median over `steps` rounds; a round runs each variant once, in turn (interleaved), every other round in reversed
  order.  One measurement = `reps` calls enqueued back to back and one synchronise, timed with the host clock and divided by `reps`.
  The floor of a case: |path 1 - its twin|.  No case is the flagship of this stage, so path 0 is the path with the smaller sum of
  medians over the cases; the wins and losses beyond the floor are printed beside it.

    python tools/route_cost.py [--frames 1024] [--steps 5] [--warmup 1] [--reps 8]
"""
import argparse
import math
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

SHAPES = ((256, 0.5), (64, 2.0))  # (cells a side, metres a cell)
LIMITS = (0.2, 0.3, 0.05)
BASE, LETHAL, UNKNOWN = 10, 100, 50
RADIUS_M, START_M = 20.0, 12.0
MAX_WAYPOINTS = 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "route_cost.txt"))
    a = ap.parse_args()
    lines = []

    def out(s=""):
        print(s, flush=True)
        lines.append(s)

    src, kind = bench.load_source_frames("kitti")
    F = a.frames
    big, ptrs, ns, _ = device_batch(src, F, "row4")
    d_cost = {n: torch.empty(F * n * n, dtype=torch.int8, device="cuda") for n, _ in SHAPES}
    d_from = {n: torch.empty(F * n * n, dtype=torch.int32, device="cuda") for n, _ in SHAPES}
    d_reach = torch.empty(F * 256 * 256, dtype=torch.int32, device="cuda")
    d_rows = torch.empty(F * 16 * 8, dtype=torch.int32, device="cuda")
    d_wps = torch.empty(F * 16 * MAX_WAYPOINTS, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    tp = pwpp_hip.TerrainParams(1, 3, LIMITS[0], LIMITS[1], LIMITS[2], 0)
    rp = lambda max_reach=0: pwpp_hip.ReachParams(BASE, LETHAL, UNKNOWN, 0, max_reach, 0)
    qp = lambda look, line_cost=0: pwpp_hip.RouteParams(0, MAX_WAYPOINTS, look, line_cost)
    limit = {n: int(10 * BASE * RADIUS_M / cell) for n, cell in SHAPES}

    def starts(n, cell, count):
        return np.array([(n // 2 + int(round(START_M / cell * math.cos(k * math.pi / 8))), n // 2 + int(round(START_M / cell * math.sin(k * math.pi / 8)))) for k in range(count)],
                        np.int32)

    def timed(enqueue, sync, reps):
        t0 = time.perf_counter()
        for _ in range(reps):
            enqueue()
        sync()
        return (time.perf_counter() - t0) * 1e6 / reps

    h = pwpp_hip.Handle()
    h.submit_batch(ptrs, ns, 4, pwpp_hip.LAYOUT_ROW_MAJOR, pwpp_hip.MEM_DEVICE, pwpp_hip.MODE_FRESH)
    h.synchronize()
    for n, cell in SHAPES:  # the cost bytes and the unlimited field's from, once
        x0 = -0.5 * n * cell
        h.terrain_ground_device(x0, x0, cell, n, n, tp, 0, 0, 0, 0, d_cost[n].data_ptr(), 0, 0, F)
        h.reach_grid_device(n, n, F, d_cost[n].data_ptr(), (n // 2, n // 2), rp(), d_reach.data_ptr(), d_from[n].data_ptr())
    h.synchronize()

    def route(n, cell, count, look, path, line_cost=0):
        st = starts(n, cell, count)

        def go():
            h.set_option("route_path", path)
            return timed(lambda: h.route_grid_device(n, n, F, d_cost[n].data_ptr(), (n // 2, n // 2), rp(), d_from[n].data_ptr(), st, qp(look, line_cost), d_rows.data_ptr(), 0,
                                                     d_wps.data_ptr()), h.synchronize, a.reps)
        return go

    def plan(n, cell, max_reach, path):
        st = starts(n, cell, 16)

        def go():
            h.set_option("route_path", path)
            return timed(lambda: h.plan_grid_device(n, n, F, d_cost[n].data_ptr(), (n // 2, n // 2), rp(max_reach), st, qp(64), d_rows.data_ptr(), 0, d_wps.data_ptr()),
                         h.synchronize, 2)
        return go

    def reach(n, max_reach):
        return lambda: timed(lambda: h.reach_grid_device(n, n, F, d_cost[n].data_ptr(), (n // 2, n // 2), rp(max_reach), d_reach.data_ptr(), d_from[n].data_ptr()),
                             h.synchronize, 2)

    out("python tools/route_cost.py --frames %d --steps %d --warmup %d --reps %d" % (F, a.steps, a.warmup, a.reps))
    out("route_cost: %s, %d frames, %s" % (kind, F, torch.cuda.get_device_name(0)))
    out("terrain cost at radius 1, min_known 3, limits %s; reach: base %d, lethal %d, unknown %d, unlimited; the source is the sensor's cell; starts on a circle of %g m; "
        "%d waypoints stored, no cell list" % (LIMITS, BASE, LETHAL, UNKNOWN, START_M, MAX_WAYPOINTS))
    longest = {}
    for n, cell in SHAPES:
        for count in (1, 16):
            for look, line_cost in ((16, 0), (64, 0), (16, 100), (64, 100)):
                route(n, cell, count, look, 1, line_cost)()
                rows = d_rows[:F * count * 8].cpu().numpy().reshape(-1, 8)
                ok = rows[:, 0] == pwpp_hip.ROUTE_OK
                longest[(n, count)] = int(rows[ok, 1].max()) - 1 if ok.any() else 0
                out("  %3d x %3d, %2d starts, look %2d, line_cost %3d: %5d routes, %5d arrive, %5d have none, %d broken; %d hops in all, the longest route %d; %.1f waypoints a route that arrives"
                    % (n, n, count, look, line_cost, len(rows), int(ok.sum()), int((rows[:, 0] == pwpp_hip.ROUTE_NONE).sum()), int((rows[:, 0] == pwpp_hip.ROUTE_BROKEN).sum()),
                       int((rows[ok, 1] - 1).sum()), longest[(n, count)], float(rows[ok, 7].mean()) if ok.any() else 0.0))
    out("us per call: host clock over %d calls (2 for pwpp_plan_grid and pwpp_reach_grid) enqueued back to back + one synchronise; median of %d interleaved rounds "
        "(every other one reversed) after %d warm-up rounds" % (a.reps, a.steps, a.warmup))
    out()

    variants, cases = [], []
    for n, cell in SHAPES:
        for count in (1, 16):
            for look, line_cost in ((16, 0), (64, 0), (16, 100), (64, 100)):
                cases.append((n, count, look, line_cost))
                for label, path in (("path 1", 1), ("path 1 twin", 1), ("path 2", 2)):
                    variants.append(("pwpp_route_grid %d x %d, %2d starts, look %2d, line_cost %3d, %s" % (n, n, count, look, line_cost, label),
                                     route(n, cell, count, look, path, line_cost)))
    extra = len(variants)
    n0, cell0 = SHAPES[0]
    for what, max_reach in (("unlimited", 0), ("max_reach %d (%g m)" % (limit[n0], RADIUS_M), limit[n0])):
        variants.append(("pwpp_reach_grid %d x %d with from, %s" % (n0, n0, what), reach(n0, max_reach)))
        for path in (1, 2):
            variants.append(("pwpp_plan_grid %d x %d, 16 starts, look 64, %s, route_path %d" % (n0, n0, what, path), plan(n0, cell0, max_reach, path)))
    t = [[] for _ in variants]
    for rnd in range(a.warmup + a.steps):
        order = range(len(variants)) if rnd % 2 == 0 else range(len(variants) - 1, -1, -1)
        for k in order:
            v = variants[k][1]()
            if rnd >= a.warmup:
                t[k].append(v)
        print("round %d of %d done" % (rnd + 1, a.warmup + a.steps), file=sys.stderr, flush=True)
    h.reach_grid_device(n0, n0, F, d_cost[n0].data_ptr(), (n0 // 2, n0 // 2), rp(), d_reach.data_ptr(), d_from[n0].data_ptr())  # (the unlimited from again)
    h.synchronize()
    med = [float(np.median(x)) for x in t]
    for (name, _), x, m in zip(variants, t, med):
        out("  %-78s %11.1f us   [%11.1f .. %11.1f]" % (name, m, min(x), max(x)))
    out()

    # the host alternative: the field through host memory
    cost_host = d_cost[n0].cpu().numpy().reshape(F, n0, n0)
    th = []
    for _ in range(3):
        t0 = time.perf_counter()
        h.reach_grid(cost_host, (n0 // 2, n0 // 2), rp())
        th.append((time.perf_counter() - t0) * 1e6)
    frm_host = d_from[n0].cpu().numpy()
    with tempfile.TemporaryDirectory() as tmp:  # the walk in C++ on the host: the one text, the serial deal, -O2, one thread
        exe = os.path.join(tmp, "route_check")
        subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "patchwork-plusplus_amd", "csrc"), os.path.join(ROOT, "tools", "route_check.cpp"),
                        "-o", exe], check=True)
        files = {}
        for name, arr in (("cost", cost_host), ("from", frm_host), ("src", np.array([[n0 // 2, n0 // 2]], np.int32)), ("starts", starts(n0, cell0, 16))):
            files[name] = os.path.join(tmp, name)
            arr.tofile(files[name])
        r = subprocess.run([exe, "dump", files["cost"], str(n0), str(n0), str(F), str(BASE), str(LETHAL), str(UNKNOWN), "0", "-", files["src"], "1", files["from"],
                            files["starts"], "1", "16", "0", str(MAX_WAYPOINTS), "64", "0", "1", os.path.join(tmp, "out")], check=True, capture_output=True, text=True)
        walk_us = float(r.stdout.split("walked in ")[1].split(" us")[0])
    out("the host alternative: pwpp_reach_grid %d x %d in PWPP_MEM_HOST with reach and from brought to the host (%.0f MB) %.1f us (of 3 calls: %.1f .. %.1f) + the walk of %d "
        "routes in C++ on the host (look 64, line_cost 0, one thread) %.1f us = %.1f us"
        % (n0, n0, F * n0 * n0 * 8 / 1e6, float(np.median(th)), min(th), max(th), F * 16, walk_us, float(np.median(th)) + walk_us))
    out()

    faster = slower = 0
    total = [0.0, 0.0]
    for ci, (n, count, look, line_cost) in enumerate(cases):
        k1, kt, k2 = 3 * ci, 3 * ci + 1, 3 * ci + 2
        floor = abs(med[k1] - med[kt])
        best = min(med[k1], med[k2])
        hops = max(longest[(n, count)], 1)
        out("pwpp_route_grid %3d x %3d, %2d starts, look %2d, line_cost %3d: path 1 %.1f us, its twin %.1f us, path 2 %.1f us: path 1 - path 2 = %.1f us against a floor of %.1f us; "
            "the longest route has %d hops: %.3f us per dependent hop on the faster path (L2 about 0.08, HBM about 0.38)"
            % (n, n, count, look, line_cost, med[k1], med[kt], med[k2], med[k1] - med[k2], floor, hops, best / hops))
        faster += med[k1] - med[k2] > floor
        total[0] += med[k1]
        total[1] += med[k2]
        slower += med[k2] - med[k1] > floor
    for i, what in enumerate(("unlimited", "max_reach")):
        r, p1, p2 = med[extra + 3 * i], med[extra + 3 * i + 1], med[extra + 3 * i + 2]
        out("pwpp_plan_grid %d x %d, 16 starts, %s: %.1f us (route_path 1), %.1f us (route_path 2) against pwpp_reach_grid with from %.1f us: the routes on top %.1f / %.1f us"
            % (n0, n0, what, p1, p2, r, p1 - r, p2 - r))
    out()
    out("path 2 beats path 1 by more than the floor in %d of %d cases and loses by more than the floor in %d; over the cases path 1 sums to %.1f us and path 2 to %.1f us: "
        "path 0 should be path %d" % (faster, len(cases), slower, total[0], total[1], 2 if total[1] < total[0] else 1))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    del big


if __name__ == "__main__":
    main()
