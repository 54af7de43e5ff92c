"""What the obstacle grid (pwpp_rasterize_obstacles) costs on one MI355X (profiles/obstacle_grid_cost.txt).

  * The raster of `frames` replayed KITTI frames in device memory, all three images (count, top, unref), band [0.2, 2.5] m, on
    256 x 256 cells of 0.5 m and on 64 x 64 cells of 2 m (the same area, sixteen times the points per cell: more contention on the
    atomics).
  * The yardsticks of each grid: a hipMemsetAsync of the same output bytes, pwpp_rasterize_ground (height + patch) on the same
    grid, and the batch's own pwpp_get_time_us.
  Every figure is the median over `steps` rounds; a round runs each variant once, in turn (interleaved).  One measurement = `reps`
  calls enqueued back to back and one synchronise, timed with the host clock and divided by `reps`: the handle's stream is its
  own, so no HIP event of this tool can bracket work on it.  The ratios are reported, nothing is gated on them.

    python tools/obstacle_grid_cost.py [--frames 1024] [--steps 9] [--warmup 2] [--reps 8]
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
from ground_query_cost import hip_runtime  # noqa: E402
from point_records_cost import device_batch  # noqa: E402

GRIDS = [(256, 256, 0.5), (64, 64, 2.0)]  # nx, ny, cell: both 128 m x 128 m around the sensor
BAND = (0.2, 2.5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "obstacle_grid_cost.txt"))
    a = ap.parse_args()
    lines = []

    def out(s=""):
        print(s, flush=True)
        lines.append(s)

    hip = hip_runtime()
    src, kind = bench.load_source_frames("kitti")
    F = a.frames
    big, ptrs, ns, _ = device_batch(src, F, "row4")
    h = pwpp_hip.Handle()
    h.submit_batch(ptrs, ns, 4, pwpp_hip.LAYOUT_ROW_MAJOR, pwpp_hip.MEM_DEVICE, pwpp_hip.MODE_FRESH)
    h.synchronize()
    batch_us = h.time_us()
    nonground = sum(h.counts(f)[1] for f in range(F))
    cells_max = F * max(nx * ny for nx, ny, _ in GRIDS)
    d = [torch.empty(cells_max, dtype=torch.int32, device="cuda") for _ in range(3)]
    torch.cuda.synchronize()

    def timed(enqueue, sync):
        t0 = time.perf_counter()
        for _ in range(a.reps):
            enqueue()
        sync()
        return (time.perf_counter() - t0) * 1e6 / a.reps

    variants = []
    for nx, ny, cell in GRIDS:
        x0, y0, cells = -0.5 * nx * cell, -0.5 * ny * cell, F * nx * ny
        tag = "%d x %d cells of %.1f m" % (nx, ny, cell)
        variants.append(("obstacles (count, top, unref), " + tag, lambda x0=x0, y0=y0, cell=cell, nx=nx, ny=ny: timed(
            lambda: h.rasterize_obstacles_device(x0, y0, cell, nx, ny, BAND[0], BAND[1], d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), 0, F),
            h.synchronize)))
        variants.append(("obstacles (count only), " + tag, lambda x0=x0, y0=y0, cell=cell, nx=nx, ny=ny: timed(
            lambda: h.rasterize_obstacles_device(x0, y0, cell, nx, ny, BAND[0], BAND[1], d[0].data_ptr(), 0, 0, 0, F), h.synchronize)))
        variants.append(("pwpp_rasterize_ground (height + patch), " + tag, lambda x0=x0, y0=y0, cell=cell, nx=nx, ny=ny: timed(
            lambda: h.rasterize_ground_device(x0, y0, cell, nx, ny, d[0].data_ptr(), d[1].data_ptr(), 0, F), h.synchronize)))
        variants.append(("hipMemsetAsync of three images, " + tag, lambda cells=cells: timed(
            lambda: [hip.hipMemsetAsync(t.data_ptr(), 0, 4 * cells, None) for t in d], hip.hipDeviceSynchronize)))
    t = [[] for _ in variants]
    for r in range(a.warmup + a.steps):
        for k, (_, run) in enumerate(variants):
            v = run()
            if r >= a.warmup:
                t[k].append(v)
    med = [float(np.median(x)) for x in t]
    out("obstacle_grid_cost: %s, %d frames, %d non-ground points (%.0f per frame), %s" % (kind, F, nonground, nonground / F, torch.cuda.get_device_name(0)))
    out("us per call: host clock over %d calls enqueued back to back + one synchronise; median / min .. max of %d interleaved rounds after %d warm-up rounds"
        % (a.reps, a.steps, a.warmup))
    out("band [%.1f, %.1f] m; plain global atomics (no combining variant was built); the batch's own pwpp_get_time_us: %.1f us" % (BAND[0], BAND[1], batch_us))
    out()
    for (name, _), m, x in zip(variants, med, t):
        out("  %-66s %10.1f us   %10.1f .. %10.1f" % (name, m, min(x), max(x)))
    out()
    out("ratios (reported, not gated):")
    for g, (nx, ny, cell) in enumerate(GRIDS):
        k = 4 * g
        out("  %3d x %3d: three images %.2f x the memset of their bytes, %.2f x the ground raster, %.1f %% of the batch; %.2f ns per non-ground point"
            % (nx, ny, med[k] / med[k + 3], med[k] / med[k + 2], 100.0 * med[k] / batch_us, 1e3 * med[k] / nonground))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    del big


if __name__ == "__main__":
    main()
