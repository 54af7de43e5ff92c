"""What the elevation fusion (pwpp_fuse_height_grid, pwpp_fuse_ground) costs on one MI355X (profiles/elevation_fusion_cost.txt), and
the A/B of the option "elevation_path": "1" the yardstick, the quotients u, v by double divisions and the share a capped mean
forgets by an integer division, as the contract writes them; "2" the product with the exact reciprocal of a cell size that is a
power of two (0.5 m here) and the multiply-shift by n_max.  What "0" means (kElevationDefaultFast, pwpp_elevation.hip) follows from
the last lines of the output.

  * `frames` replayed KITTI frames in device memory, their elevation images on 256 x 256 cells of 0.5 m, into maps of 256 x 256
    cells of 0.5 m with n_max 16, a yawing, translating pose and a height offset per frame, for
      (a) `frames` maps, frame i into map i          (b) one map, all frames in sequence          (c) 16 maps, frame i into map i % 16
    sums, counts and means are device arrays.
  * pwpp_fuse_height_grid alone on the device images a pwpp_rasterize_ground call left: path 1, path 1 again (the A/A twin: the
    same variant under another name, whose distance from the first is the floor no difference can be read below) and path 2.
  * pwpp_fuse_ground on both paths, the per-frame images kept in the handle's buffer, and pwpp_rasterize_ground alone on the same
    handle and grid in the same rounds: the fusion's own cost is the difference.
  * For scale, pwpp_fuse_grid -- the occupancy fusion -- on the same maps and poses, on the bytes a visibility call left.
  Beside each time of pwpp_fuse_height_grid: the algorithmic bytes -- 6 in + 6 out + 4 of the mean per map cell, 4 nx ny per frame
  read once -- and the share of the HBM peak (8.0 TB/s) they amount to in that time.
  Every figure is the median over `steps` rounds; a round runs each variant once, in turn (interleaved), every other round in
  reversed order, so that a drift of the clocks and the neighbour a variant runs after hit every variant alike.  One measurement =
  `reps` calls enqueued back to back and one synchronise, timed with the host clock and divided by `reps`.  The whole set is run
  `runs` times in this process (fresh handles each time).  The floor of a case: the larger of |path 1 - its twin| and the spread of
  the three variants' medians between runs.  Path 0 becomes path 2 only where path 2 beats path 1 by more than the floor in EVERY
  case.

    python tools/elevation_fusion_cost.py [--frames 1024] [--steps 7] [--warmup 2] [--reps 4] [--runs 3]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("tests", "patchwork-plusplus_amd/python", "tools", ""):
    sys.path.insert(0, os.path.join(ROOT, p))
import numpy as np  # noqa: E402
import torch  # noqa: E402  (before libpwpp_hip: see tests/conftest.py)

import bench  # noqa: E402
import pwpp_hip  # noqa: E402
from point_records_cost import device_batch  # noqa: E402

NX = NY = 256
CELL = 0.5
N_MAX = 16
BAND = (0.2, 2.5)
MAX_RANGE = 40
HBM_PEAK = 8.0e12  # bytes/s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "elevation_fusion_cost.txt"))
    a = ap.parse_args()
    lines = []

    def out(s=""):
        print(s, flush=True)
        lines.append(s)

    src, kind = bench.load_source_frames("kitti")
    F = a.frames
    big, ptrs, ns, _ = device_batch(src, F, "row4")
    x0 = y0 = -0.5 * NX * CELL
    per = NX * NY
    hmap = pwpp_hip.HeightMap(x0, y0, CELL, NX, NY, N_MAX, 0)
    fmap = pwpp_hip.FusionMap(x0, y0, CELL, NX, NY, 40, 20, -200, 350, 60, -40)
    # the vehicle drives a circle of 8 m radius, 5 rad over 1024 frames, and climbs 1 mm a frame: yaw, translation and offset change with every frame
    yaw = 0.005 * np.arange(F)
    poses = np.stack([np.cos(yaw), -np.sin(yaw), 8.0 * np.sin(yaw), np.sin(yaw), np.cos(yaw), 8.0 * (1.0 - np.cos(yaw))], axis=1)
    tz = 0.001 * np.arange(F)
    cases = [("(a) %d maps, frame i into map i" % F, F, None), ("(b) one map, %d frames in sequence" % F, 1, None),
             ("(c) 16 maps, frame i into map i % 16", 16, np.arange(F, dtype=np.int32) % 16)]
    d_h = torch.empty(F * per, dtype=torch.float32, device="cuda")
    d_sin, d_nin = torch.zeros(F * per, dtype=torch.int32, device="cuda"), torch.zeros(F * per, dtype=torch.int16, device="cuda")
    d_sout, d_nout = torch.empty(F * per, dtype=torch.int32, device="cuda"), torch.empty(F * per, dtype=torch.int16, device="cuda")
    d_mean = torch.empty(F * per, dtype=torch.float32, device="cuda")
    d_first, d_count = (torch.empty(F * per, dtype=torch.int32, device="cuda") for _ in range(2))
    d_occ, d_byte = (torch.empty(F * per, dtype=torch.int8, device="cuda") for _ in range(2))
    d_lin, d_lout = torch.zeros(F * per, dtype=torch.int16, device="cuda"), torch.empty(F * per, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    algo_bytes = [16 * per * n_maps + 4 * per * F for _, n_maps, _ in cases]

    def timed(enqueue, sync):
        t0 = time.perf_counter()
        for _ in range(a.reps):
            enqueue()
        sync()
        return (time.perf_counter() - t0) * 1e6 / a.reps

    names, medians, head = None, [], False
    for run in range(a.runs):
        h = pwpp_hip.Handle()
        h.submit_batch(ptrs, ns, 4, pwpp_hip.LAYOUT_ROW_MAJOR, pwpp_hip.MEM_DEVICE, pwpp_hip.MODE_FRESH)
        h.synchronize()
        batch_us = h.time_us()

        def raster():
            return timed(lambda: h.rasterize_ground_device(x0, y0, CELL, NX, NY, d_h.data_ptr(), 0, 0, F), h.synchronize)

        def height_grid(n_maps, mof, path):
            def go():
                h.set_option("elevation_path", path)
                return timed(lambda: h.fuse_height_grid_device((x0, y0, CELL), NX, NY, F, d_h.data_ptr(), poses, hmap, n_maps, d_sin.data_ptr(), d_nin.data_ptr(),
                                                               d_sout.data_ptr(), d_nout.data_ptr(), d_mean.data_ptr(), tz, mof), h.synchronize)
            return go

        def ground(n_maps, mof, path):
            def go():
                h.set_option("elevation_path", path)
                return timed(lambda: h.fuse_ground_device(x0, y0, CELL, NX, NY, poses, hmap, n_maps, d_sin.data_ptr(), d_nin.data_ptr(), d_sout.data_ptr(),
                                                          d_nout.data_ptr(), d_mean.data_ptr(), 0, tz, 0, F, mof), h.synchronize)
            return go

        def occupancy(n_maps, mof):
            return lambda: timed(lambda: h.fuse_grid_device((x0, y0, CELL), NX, NY, F, d_occ.data_ptr(), poses, fmap, n_maps, d_lin.data_ptr(), d_lout.data_ptr(),
                                                            d_byte.data_ptr(), mof), h.synchronize)

        raster()  # (d_h holds the frames' elevation images from here on: what pwpp_fuse_height_grid reads)
        h.visibility_obstacles_device(x0, y0, CELL, NX, NY, BAND[0], BAND[1], (0.0, 0.0), 1, MAX_RANGE, d_first.data_ptr(), d_occ.data_ptr(), d_count.data_ptr(), 0, F)
        h.synchronize()
        variants = []
        for name, n_maps, mof in cases:
            for label, path in (("path 1", 1), ("path 1 twin", 1), ("path 2", 2)):
                variants.append(("pwpp_fuse_height_grid %s, %s" % (name, label), height_grid(n_maps, mof, path)))
        for name, n_maps, mof in cases:
            for path in (1, 2):
                variants.append(("pwpp_fuse_ground      %s, path %d" % (name, path), ground(n_maps, mof, path)))
        for name, n_maps, mof in cases:
            variants.append(("pwpp_fuse_grid (occupancy) %s" % name, occupancy(n_maps, mof)))
        variants.append(("pwpp_rasterize_ground (height) alone", raster))
        t = [[] for _ in variants]
        for r in range(a.warmup + a.steps):
            order = range(len(variants)) if r % 2 == 0 else range(len(variants) - 1, -1, -1)
            for k in order:
                v = variants[k][1]()
                if r >= a.warmup:
                    t[k].append(v)
        if not head:
            head = True
            out("elevation_fusion_cost: %s, %d frames, elevation images of %d x %d cells of %.1f m, %s" % (kind, F, NX, NY, CELL, torch.cuda.get_device_name(0)))
            out("maps of %d x %d cells of %.1f m, n_max %d; pose i: yaw 0.005 i rad on a circle of 8 m, offset 0.001 i m" % (NX, NY, CELL, N_MAX))
            out("  the frames: %.1f %% of the cells have a height" % (100.0 * int(torch.isfinite(d_h).sum().item()) / (F * per)))
            for (name, n_maps, mof), go in zip(cases, [height_grid(c[1], c[2], 1) for c in cases]):
                go()
                n = d_nout[:n_maps * per]
                out("  the maps of %s: %.1f %% of the cells observed, %.1f %% at n_max" % (name, 100.0 * int((n > 0).sum().item()) / n.numel(),
                                                                                         100.0 * int((n == N_MAX).sum().item()) / n.numel()))
            out("us per call: host clock over %d calls enqueued back to back + one synchronise; median of %d interleaved rounds (every other one reversed)"
                % (a.reps, a.steps))
            out("after %d warm-up rounds; %d runs of the whole set, each with a fresh handle and batch" % (a.warmup, a.runs))
            out()
        names = [v[0] for v in variants]
        medians.append([float(np.median(x)) for x in t] + [batch_us])
        out("run %d (min .. max of the rounds in brackets):" % run)
        for name, x in zip(names, t):
            out("  %-72s %10.1f us   [%10.1f .. %10.1f]" % (name, float(np.median(x)), min(x), max(x)))
        out("  %-72s %10.1f us" % ("the batch's own pwpp_get_time_us", batch_us))
        del h
    m = np.array(medians)
    out()
    out("over the %d runs: median of the runs' medians, and their spread (max - min) between runs" % a.runs)
    for k, name in enumerate(names + ["the batch's own pwpp_get_time_us"]):
        out("  %-72s %10.1f us   spread %8.1f us" % (name, float(np.median(m[:, k])), float(m[:, k].max() - m[:, k].min())))
    out()
    med = lambda k: float(np.median(m[:, k]))
    spread = lambda k: float(m[:, k].max() - m[:, k].min())
    ras = med(len(names) - 1)
    wins = []
    for ci, (name, n_maps, mof) in enumerate(cases):
        k1, kt, k2 = 3 * ci, 3 * ci + 1, 3 * ci + 2
        floor = max(abs(med(k1) - med(kt)), spread(k1), spread(kt), spread(k2))
        rate = algo_bytes[ci] / (med(k1) * 1e-6)
        out("pwpp_fuse_height_grid %s: path 1 %.1f us, its twin %.1f us, path 2 %.1f us: path 1 - path 2 = %.1f us against a floor of %.1f us; "
            "algorithmic bytes %.1f MB = %.3f TB/s = %.2f %% of the HBM peak of %.1f TB/s on path 1; pwpp_fuse_grid on the same maps %.1f us"
            % (name, med(k1), med(kt), med(k2), med(k1) - med(k2), floor, algo_bytes[ci] / 1e6, rate / 1e12, 100.0 * rate / HBM_PEAK, HBM_PEAK / 1e12,
               med(15 + ci)))
        g1, g2 = 9 + 2 * ci, 10 + 2 * ci
        out("pwpp_fuse_ground      %s: path 1 %.1f us, path 2 %.1f us; pwpp_rasterize_ground alone %.1f us (spread %.1f): the fusion on top of it %.1f us"
            % (name, med(g1), med(g2), ras, spread(len(names) - 1), med(g1) - ras))
        wins.append(med(k1) - med(k2) > floor)
    out()
    out("path 2 beats path 1 by more than the floor in: " + (", ".join(c[0][:3] for c, w in zip(cases, wins) if w) or "no case"))
    out("kElevationDefaultFast (what \"elevation_path\" = 0 means) should be: %s" % ("true" if all(wins) else "false"))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    del big


if __name__ == "__main__":
    main()
