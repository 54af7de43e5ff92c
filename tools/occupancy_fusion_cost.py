"""What the occupancy fusion (pwpp_fuse_obstacles, pwpp_fuse_grid) costs on one MI355X (profiles/occupancy_fusion_cost.txt), and the
A/B of the option "fusion_path": "1" the yardstick, every sample's cell by two double divisions as the contract writes them;
"0" the default, the product with the exact reciprocal of a cell size that is a power of two (0.5 m here).

  * pwpp_fuse_obstacles of `frames` replayed KITTI frames in device memory on 256 x 256 cells of 0.5 m, band [0.2, 2.5] m,
    min_count 1, origin {0, 0}, max_range 40, into maps of 256 x 256 cells of 0.5 m, a yawing, translating pose per frame, for
      (a) `frames` maps, frame i into map i          (b) one map, all frames in sequence          (c) 16 maps, frame i into map i % 16
    on both paths; map_in, map_out and the byte are device arrays, the per-frame bytes stay in the handle's buffer.
  * The yardstick: pwpp_visibility_obstacles alone on the same handle and grid, in the same rounds -- the fusion's own cost is the
    difference -- and pwpp_fuse_grid alone on the device images a visibility call left.
  Beside each time of pwpp_fuse_grid: the algorithmic bytes -- 2 in + 2 out + 1 byte out per map cell, nx * ny bytes per frame read
  once -- and the share of the HBM peak (8.0 TB/s, the specified peak of MI355X_MICROARCH; 6.3 TB/s is what a copy reaches) they
  amount to in that time.
  Every figure is the median over `steps` rounds; a round runs each variant once, in turn (interleaved), so that a drift of the
  clocks hits every variant alike.  One measurement = `reps` calls enqueued back to back and one synchronise, timed with the host
  clock and divided by `reps`.  The whole set is run `runs` times in this process (fresh handles each time): the spread BETWEEN
  runs is what a difference between the two paths has to exceed to be a difference.  The condition the tool states at the end:
  path 0 beats path 1 by more than that spread in case (a), which it was built for, and loses by more than it in no case.

    python tools/occupancy_fusion_cost.py [--frames 1024] [--steps 7] [--warmup 2] [--reps 4] [--runs 3]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "occupancy_fusion_cost.txt"))
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
    fmap = pwpp_hip.FusionMap(x0, y0, CELL, NX, NY, 40, 20, -200, 350, 60, -40)
    # the vehicle drives a circle of 8 m radius, 5 rad over 1024 frames: yaw and translation change with every frame
    yaw = 0.005 * np.arange(F)
    poses = np.stack([np.cos(yaw), -np.sin(yaw), 8.0 * np.sin(yaw), np.sin(yaw), np.cos(yaw), 8.0 * (1.0 - np.cos(yaw))], axis=1)
    cases = [("(a) %d maps, frame i into map i" % F, F, None), ("(b) one map, %d frames in sequence" % F, 1, None),
             ("(c) 16 maps, frame i into map i % 16", 16, np.arange(F, dtype=np.int32) % 16)]
    d_first, d_count = (torch.empty(F * per, dtype=torch.int32, device="cuda") for _ in range(2))
    d_occ = torch.empty(F * per, dtype=torch.int8, device="cuda")
    d_in = torch.zeros(F * per, dtype=torch.int16, device="cuda")
    d_out = torch.empty(F * per, dtype=torch.int16, device="cuda")
    d_byte = torch.empty(F * per, dtype=torch.int8, device="cuda")
    torch.cuda.synchronize()
    algo_bytes = [5 * per * n_maps + per * F for _, n_maps, _ in cases]

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

        def visibility():
            return timed(lambda: h.visibility_obstacles_device(x0, y0, CELL, NX, NY, BAND[0], BAND[1], (0.0, 0.0), 1, MAX_RANGE, d_first.data_ptr(),
                                                               d_occ.data_ptr(), d_count.data_ptr(), 0, F), h.synchronize)

        def obstacles(n_maps, mof, path):
            def go():
                h.set_option("fusion_path", path)
                return timed(lambda: h.fuse_obstacles_device(x0, y0, CELL, NX, NY, BAND[0], BAND[1], poses, fmap, n_maps, d_in.data_ptr(), d_out.data_ptr(),
                                                             d_byte.data_ptr(), 0, (0.0, 0.0), 1, MAX_RANGE, 0, F, mof), h.synchronize)
            return go

        def grid(n_maps, mof, path):
            def go():
                h.set_option("fusion_path", path)
                return timed(lambda: h.fuse_grid_device((x0, y0, CELL), NX, NY, F, d_occ.data_ptr(), poses, fmap, n_maps, d_in.data_ptr(), d_out.data_ptr(),
                                                        d_byte.data_ptr(), mof), h.synchronize)
            return go

        visibility()  # (d_occ holds the frames' bytes from here on: what pwpp_fuse_grid reads)
        variants = []
        for name, n_maps, mof in cases:
            for path in (0, 1):
                variants.append(("pwpp_fuse_obstacles %s, path %d" % (name, path), obstacles(n_maps, mof, path)))
        for name, n_maps, mof in cases:
            for path in (0, 1):
                variants.append(("pwpp_fuse_grid      %s, path %d" % (name, path), grid(n_maps, mof, path)))
        variants.append(("pwpp_visibility_obstacles (first, occupancy, count) alone", visibility))
        t = [[] for _ in variants]
        for r in range(a.warmup + a.steps):
            for k, (_, go) in enumerate(variants):
                v = go()
                if r >= a.warmup:
                    t[k].append(v)
        if not head:
            head = True
            out("occupancy_fusion_cost: %s, %d frames, %d x %d cells of %.1f m, band [%.1f, %.1f] m, min_count 1, origin {0, 0}, max_range %d, %s"
                % (kind, F, NX, NY, CELL, BAND[0], BAND[1], MAX_RANGE, torch.cuda.get_device_name(0)))
            out("maps of %d x %d cells of %.1f m, hit 40, miss 20, clamps [-200, 350], thresholds 60 / -40; pose i: yaw 0.005 i rad on a circle of 8 m" % (NX, NY, CELL))
            n = F * per
            share = [100.0 * int((d_occ == v).sum().item()) / n for v in (pwpp_hip.OCC_OCCUPIED, pwpp_hip.OCC_FREE, pwpp_hip.OCC_UNKNOWN)]
            out("  the frames: %.1f %% of the cells occupied, %.1f %% free, %.1f %% unknown" % tuple(share))
            for (name, n_maps, mof), go in zip(cases, [grid(c[1], c[2], 1) for c in cases]):
                go()
                b = d_byte[:n_maps * per]
                share = [100.0 * int((b == v).sum().item()) / b.numel() for v in (pwpp_hip.OCC_OCCUPIED, pwpp_hip.OCC_FREE, pwpp_hip.OCC_UNKNOWN)]
                out("  the maps of %s: %.1f %% occupied, %.1f %% free, %.1f %% unknown" % ((name,) + tuple(share)))
            out("us per call: host clock over %d calls enqueued back to back + one synchronise; median of %d interleaved rounds after %d warm-up rounds;"
                % (a.reps, a.steps, a.warmup))
            out("%d runs of the whole set, each with a fresh handle and batch" % a.runs)
            out()
        names = [v[0] for v in variants]
        medians.append([float(np.median(x)) for x in t] + [batch_us])
        out("run %d (min .. max of the rounds in brackets):" % run)
        for name, x in zip(names, t):
            out("  %-68s %10.1f us   [%10.1f .. %10.1f]" % (name, float(np.median(x)), min(x), max(x)))
        out("  %-68s %10.1f us" % ("the batch's own pwpp_get_time_us", batch_us))
        del h
    m = np.array(medians)
    out()
    out("over the %d runs: median of the runs' medians, and their spread (max - min) between runs" % a.runs)
    for k, name in enumerate(names + ["the batch's own pwpp_get_time_us"]):
        out("  %-68s %10.1f us   spread %8.1f us" % (name, float(np.median(m[:, k])), float(m[:, k].max() - m[:, k].min())))
    out()
    vis = float(np.median(m[:, 12]))
    vis_spread = float(m[:, 12].max() - m[:, 12].min())
    wins, loses = [], []
    for ci, (name, n_maps, mof) in enumerate(cases):
        for what, k0 in (("pwpp_fuse_obstacles", 2 * ci), ("pwpp_fuse_grid", 6 + 2 * ci)):
            p0, p1 = float(np.median(m[:, k0])), float(np.median(m[:, k0 + 1]))
            spread = max(float(m[:, k0].max() - m[:, k0].min()), float(m[:, k0 + 1].max() - m[:, k0 + 1].min()))
            line = "%s %s: path 0 %.1f us, path 1 %.1f us: path 1 - path 0 = %.1f us against a spread between runs of %.1f us" % (what, name, p0, p1, p1 - p0, spread)
            if what == "pwpp_fuse_obstacles":
                line += "; the fusion alone (path 1 - visibility %.1f us, spread %.1f) %.1f us" % (vis, vis_spread, p1 - vis)
            else:
                rate = algo_bytes[ci] / (p1 * 1e-6)
                line += "; algorithmic bytes %.1f MB = %.3f TB/s = %.2f %% of the HBM peak of %.1f TB/s" % (algo_bytes[ci] / 1e6, rate / 1e12, 100.0 * rate / HBM_PEAK,
                                                                                                          HBM_PEAK / 1e12)
            out(line)
            if p1 - p0 > spread:
                wins.append("%s %s" % (what, name[:3]))
            if p0 - p1 > spread:
                loses.append("%s %s" % (what, name[:3]))
    out()
    out("path 0 beats path 1 by more than the spread between runs in: " + ("; ".join(wins) if wins else "no case"))
    out("path 0 is not slower than path 1 by more than the spread between runs in any case" if not loses else
        "PATH 0 IS SLOWER THAN PATH 1 in: " + "; ".join(loses))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    del big


if __name__ == "__main__":
    main()
