"""What the obstacle clusters (pwpp_label_obstacles) cost on one MI355X (profiles/obstacle_clusters_cost.txt), and the A/B of the
option "clusters_path": "0" tiles of 64 x 16 cells in LDS and then their borders, "1" one global union-find without LDS.

  * pwpp_label_obstacles of `frames` replayed KITTI frames in device memory (label, count, top, table of 64 rows per frame,
    n_clusters), 256 x 256 cells of 0.5 m, band [0.2, 2.5] m, min_count 1, at both paths and both connectivities; and once more
    with the per-point cluster ids.
  * The yardsticks: pwpp_rasterize_obstacles (count, top) alone, a hipMemsetAsync of the label bytes, and the batch's own
    pwpp_get_time_us.
  Every figure is the median over `steps` rounds; a round runs each variant once, in turn (interleaved), so that a drift of the
  clocks hits every variant alike.  One measurement = `reps` calls enqueued back to back and one synchronise, timed with the host
  clock and divided by `reps`: the handle's stream is its own, so no HIP event of this tool can bracket work on it.  The whole
  set is run `runs` times in this process (fresh handles each time): the spread BETWEEN runs is what a difference between the two
  paths has to exceed to be a difference.

    python tools/obstacle_clusters_cost.py [--frames 1024] [--steps 7] [--warmup 2] [--reps 4] [--runs 3]
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

NX, NY, CELL = 256, 256, 0.5
BAND = (0.2, 2.5)
ROWS = 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "obstacle_clusters_cost.txt"))
    a = ap.parse_args()
    lines = []

    def out(s=""):
        print(s, flush=True)
        lines.append(s)

    hip = hip_runtime()
    src, kind = bench.load_source_frames("kitti")
    F = a.frames
    big, ptrs, ns, _ = device_batch(src, F, "row4")
    cells, x0, y0 = F * NX * NY, -0.5 * NX * CELL, -0.5 * NY * CELL
    d_label, d_count, d_top = (torch.empty(cells, dtype=torch.int32, device="cuda") for _ in range(3))
    d_table = torch.empty(F * ROWS * 12, dtype=torch.int32, device="cuda")
    d_n = torch.empty(F, dtype=torch.int32, device="cuda")
    d_pc = torch.empty(int(sum(ns)), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def timed(enqueue, sync):
        t0 = time.perf_counter()
        for _ in range(a.reps):
            enqueue()
        sync()
        return (time.perf_counter() - t0) * 1e6 / a.reps

    names, medians, head = None, [], None
    for run in range(a.runs):
        h = pwpp_hip.Handle()
        h.submit_batch(ptrs, ns, 4, pwpp_hip.LAYOUT_ROW_MAJOR, pwpp_hip.MEM_DEVICE, pwpp_hip.MODE_FRESH)
        h.synchronize()
        batch_us = h.time_us()

        def label(path, conn, ids=False):
            def go():
                h.set_option("clusters_path", path)
                return timed(lambda: h.label_obstacles_device(x0, y0, CELL, NX, NY, BAND[0], BAND[1], 1, conn, d_label.data_ptr(), d_count.data_ptr(),
                                                              d_top.data_ptr(), d_table.data_ptr(), d_n.data_ptr(), ROWS, d_pc.data_ptr() if ids else 0, 0, F),
                             h.synchronize)
            return go

        variants = [("label_obstacles, tiles (path 0), connectivity %d" % c, label(0, c)) for c in (4, 8)]
        variants += [("label_obstacles, global (path 1), connectivity %d" % c, label(1, c)) for c in (4, 8)]
        variants.append(("label_obstacles, tiles, connectivity 8, + point_cluster", label(0, 8, True)))
        variants.append(("pwpp_rasterize_obstacles (count, top) alone", lambda: timed(
            lambda: h.rasterize_obstacles_device(x0, y0, CELL, NX, NY, BAND[0], BAND[1], d_count.data_ptr(), d_top.data_ptr(), 0, 0, F), h.synchronize)))
        variants.append(("hipMemsetAsync of the label bytes", lambda: timed(
            lambda: hip.hipMemsetAsync(d_label.data_ptr(), 0, 4 * cells, None), hip.hipDeviceSynchronize)))
        t = [[] for _ in variants]
        for r in range(a.warmup + a.steps):
            for k, (_, go) in enumerate(variants):
                v = go()
                if r >= a.warmup:
                    t[k].append(v)
        if head is None:
            h.set_option("clusters_path", 0)
            h.label_obstacles_device(x0, y0, CELL, NX, NY, BAND[0], BAND[1], 1, 8, d_label.data_ptr(), d_count.data_ptr(), d_top.data_ptr(), 0, d_n.data_ptr(), 0,
                                     0, 0, F)
            h.synchronize()
            n = d_n.cpu().numpy()
            occupied = int((d_count > 0).sum().item())
            head = "%s, %d frames, %d x %d cells of %.1f m, band [%.1f, %.1f] m: %d occupied cells (%.1f %%), %.0f clusters per frame (connectivity 8, max %d), %s" % (
                kind, F, NX, NY, CELL, BAND[0], BAND[1], occupied, 100.0 * occupied / cells, n.mean(), n.max(), torch.cuda.get_device_name(0))
            out("obstacle_clusters_cost: " + head)
            out("us per call: host clock over %d calls enqueued back to back + one synchronise; median of %d interleaved rounds after %d warm-up rounds;"
                % (a.reps, a.steps, a.warmup))
            out("%d runs of the whole set, each with a fresh handle and batch" % a.runs)
            out()
        names = [v[0] for v in variants]
        medians.append([float(np.median(x)) for x in t] + [batch_us])
        out("run %d (min .. max of the rounds in brackets):" % run)
        for name, x in zip(names, t):
            out("  %-58s %10.1f us   [%10.1f .. %10.1f]" % (name, float(np.median(x)), min(x), max(x)))
        out("  %-58s %10.1f us" % ("the batch's own pwpp_get_time_us", batch_us))
        del h
    m = np.array(medians)
    out()
    out("over the %d runs: median of the runs' medians, and their spread (max - min) between runs" % a.runs)
    for k, name in enumerate(names + ["the batch's own pwpp_get_time_us"]):
        out("  %-58s %10.1f us   spread %8.1f us" % (name, float(np.median(m[:, k])), float(m[:, k].max() - m[:, k].min())))
    out()
    raster, memset, batch = (float(np.median(m[:, k])) for k in (5, 6, 7))
    for c, (k0, k1) in ((4, (0, 2)), (8, (1, 3))):
        tiles, glob = float(np.median(m[:, k0])), float(np.median(m[:, k1]))
        spread = max(float(m[:, k0].max() - m[:, k0].min()), float(m[:, k1].max() - m[:, k1].min()))
        out("connectivity %d: tiles %.1f us, global %.1f us: global - tiles = %.1f us against a spread between runs of %.1f us; labelling alone (tiles - raster) "
            "%.1f us = %.2f x the memset of the label bytes, %.1f %% of the batch" % (c, tiles, glob, glob - tiles, spread, tiles - raster, (tiles - raster) / memset,
                                                                                       100.0 * (tiles - raster) / batch))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    del big


if __name__ == "__main__":
    main()
