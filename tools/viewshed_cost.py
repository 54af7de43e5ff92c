"""What the viewshed (pwpp_viewshed_grid, pwpp_viewshed_obstacles) costs on one MI355X (profiles/viewshed_cost.txt), and the A/B of
the option "viewshed_path": "1" every test of a cell reads count and every rise reads block in global memory, "2" the occupancy in
the visibility's bit image, its rows in LDS where they fit, a rise fetched only where a bit is set.

  * The images: pwpp_rasterize_obstacles (count, top), pwpp_rasterize_ground and pwpp_rasterize_ground_returns of `frames` replayed
    KITTI frames, band [0.2, 2.5] m, on two grids -- 256 x 256 cells of 0.5 m and 64 x 64 cells of 2 m -- quantised on the host
    with the restatement's quantiser, in device memory.  The sensor is the origin of the model's frame: eye = units(0).
  * pwpp_viewshed_grid on them, paths 1 and 2, with and without the shadow image, unlimited and at max_range 40 cells (20 m on the
    fine grid), against pwpp_visibility_grid on the SAME count images in the same run (its default path).
  * The chained pwpp_viewshed_obstacles (default path, with shadow, min_seen 1) against pwpp_visibility_obstacles.
  * A/A twins: path 2 with shadow, unlimited, is measured twice per round under two names; their difference is what the method
    cannot resolve.  The floor: an empty call (pwpp_synchronize alone).
  Every figure is the median over `steps` rounds; a round runs each variant once, in turn (interleaved), so that a drift of the
  clocks hits every variant alike.  One measurement = `reps` calls enqueued back to back and one synchronise, timed with the host
  clock and divided by `reps`.  The whole set is run `runs` times in this process (fresh handles each time): the spread BETWEEN
  runs, and the A/A difference, are what a difference between two paths has to exceed to be a difference.
  It also reports the share of cells FREE under each operator on those frames.

    python tools/viewshed_cost.py [--frames 1024] [--steps 7] [--warmup 2] [--reps 4] [--runs 3]
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
import viewshed_ref as vr  # noqa: E402
from point_records_cost import device_batch  # noqa: E402

GRIDS = [(256, 256, 0.5), (64, 64, 2.0)]  # (nx, ny, cell)
RADII = (0, 40)
BAND = (0.2, 2.5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "viewshed_cost.txt"))
    a = ap.parse_args()
    lines = []

    def out(s=""):
        print(s, flush=True)
        lines.append(s)

    src, kind = bench.load_source_frames("kitti")
    F = a.frames
    big, ptrs, ns, _ = device_batch(src, F, "row4")
    cells = F * max(nx * ny for nx, ny, _ in GRIDS)
    d_first, d_shadow, d_count = (torch.empty(cells, dtype=torch.int32, device="cuda") for _ in range(3))
    d_occ = torch.empty(cells, dtype=torch.int8, device="cuda")
    torch.cuda.synchronize()
    eye = vr.units(0.0)

    def timed(enqueue, sync):
        t0 = time.perf_counter()
        for _ in range(a.reps):
            enqueue()
        sync()
        return (time.perf_counter() - t0) * 1e6 / a.reps

    names, medians, head, images = None, [], False, {}
    for run in range(a.runs):
        h = pwpp_hip.Handle()
        h.submit_batch(ptrs, ns, 4, pwpp_hip.LAYOUT_ROW_MAJOR, pwpp_hip.MEM_DEVICE, pwpp_hip.MODE_FRESH)
        h.synchronize()
        batch_us = h.time_us()
        for g in GRIDS if run == 0 else ():  # the four images of a grid, once, in device memory
            nx, ny, cell = g
            x0, y0 = -0.5 * nx * cell, -0.5 * ny * cell
            count, top = h.rasterize_obstacles(x0, y0, cell, nx, ny, *BAND, frames=F)
            ground = h.rasterize_ground(x0, y0, cell, nx, ny, frames=F).astype(np.float64)
            seen = h.rasterize_ground_returns(x0, y0, cell, nx, ny, frames=F)
            images[g] = [torch.from_numpy(np.ascontiguousarray(x).reshape(-1)).cuda() for x in
                         (count, vr.units_image(ground + top.astype(np.float64)), vr.units_image(ground), seen)]
        torch.cuda.synchronize()

        def viewshed(grid, max_range, path, shadow):
            nx, ny, cell = grid
            c, b, t, s = (x.data_ptr() for x in images[grid])

            def go():
                h.set_option("viewshed_path", path)
                return timed(lambda: h.viewshed_grid_device(nx, ny, F, c, (nx // 2, ny // 2, eye), 1, max_range, d_first.data_ptr(), d_shadow.data_ptr() if shadow else 0,
                                                            d_occ.data_ptr(), b, t, s, 1), h.synchronize)
            return go

        def visibility(grid, max_range):
            nx, ny, cell = grid
            c = images[grid][0].data_ptr()
            return lambda: timed(lambda: h.visibility_grid_device(nx, ny, F, c, (nx // 2, ny // 2), 1, max_range, d_first.data_ptr(), d_occ.data_ptr()), h.synchronize)

        def chained(grid, max_range, which):
            nx, ny, cell = grid
            x0, y0 = -0.5 * nx * cell, -0.5 * ny * cell

            def go():
                h.set_option("viewshed_path", 0)
                if which == "viewshed":
                    return timed(lambda: h.viewshed_obstacles_device(x0, y0, cell, nx, ny, BAND[0], BAND[1], (0.0, 0.0, 0.0), 1, 1, max_range, d_first.data_ptr(),
                                                                     d_shadow.data_ptr(), d_occ.data_ptr(), d_count.data_ptr(), 0, F), h.synchronize)
                return timed(lambda: h.visibility_obstacles_device(x0, y0, cell, nx, ny, BAND[0], BAND[1], (0.0, 0.0), 1, max_range, d_first.data_ptr(),
                                                                   d_occ.data_ptr(), d_count.data_ptr(), 0, F), h.synchronize)
            return go

        variants = []
        for g in GRIDS:
            tag = "%d x %d of %.1f m" % g
            for r in RADII:
                for path in (1, 2):
                    for shadow in (True, False):
                        variants.append(("%s, max_range %2d, viewshed path %d, %s" % (tag, r, path, "shadow" if shadow else "no shadow"), viewshed(g, r, path, shadow)))
                variants.append(("%s, max_range %2d, pwpp_visibility_grid" % (tag, r), visibility(g, r)))
                variants.append(("%s, max_range %2d, pwpp_viewshed_obstacles" % (tag, r), chained(g, r, "viewshed")))
                variants.append(("%s, max_range %2d, pwpp_visibility_obstacles" % (tag, r), chained(g, r, "visibility")))
            variants.append(("%s, max_range  0, viewshed path 2, shadow (A/A twin)" % tag, viewshed(g, 0, 2, True)))
        variants.append(("floor: pwpp_synchronize alone", lambda: timed(lambda: None, h.synchronize)))
        t = [[] for _ in variants]
        for r in range(a.warmup + a.steps):
            for k, (_, go) in enumerate(variants):
                v = go()
                if r >= a.warmup:
                    t[k].append(v)
        if not head:
            head = True
            out("viewshed_cost: %s, %d frames, band [%.1f, %.1f] m, min_count 1, min_seen 1, origin {0, 0, 0}, %s" % (kind, F, BAND[0], BAND[1], torch.cuda.get_device_name(0)))
            for g in GRIDS:
                nx, ny, cell = g
                n = F * nx * ny
                c, b, tg, s = (x.data_ptr() for x in images[g])
                share = {}
                h.visibility_grid_device(nx, ny, F, c, (nx // 2, ny // 2), 1, 0, d_first.data_ptr(), d_occ.data_ptr())
                h.synchronize()
                share["pwpp_visibility_grid"] = [100.0 * int((d_occ[:n] == v).sum().item()) / n for v in (pwpp_hip.OCC_OCCUPIED, pwpp_hip.OCC_FREE, pwpp_hip.OCC_UNKNOWN)]
                for name, sp in (("pwpp_viewshed_grid without seen", 0), ("pwpp_viewshed_grid with seen", s)):
                    h.viewshed_grid_device(nx, ny, F, c, (nx // 2, ny // 2, eye), 1, 0, d_first.data_ptr(), 0, d_occ.data_ptr(), b, tg, sp, 1)
                    h.synchronize()
                    share[name] = [100.0 * int((d_occ[:n] == v).sum().item()) / n for v in (pwpp_hip.OCC_OCCUPIED, pwpp_hip.OCC_FREE, pwpp_hip.OCC_UNKNOWN)]
                for name, sh in share.items():
                    out("  %d x %d cells of %.1f m, %-32s %5.1f %% of the cells occupied, %5.1f %% free, %5.1f %% unknown" % (nx, ny, cell, name + ":", sh[0], sh[1], sh[2]))
            out("us per call: host clock over %d calls enqueued back to back + one synchronise; median of %d interleaved rounds after %d warm-up rounds;"
                % (a.reps, a.steps, a.warmup))
            out("%d runs of the whole set, each with a fresh handle and batch" % a.runs)
            out()
        names = [v[0] for v in variants]
        medians.append([float(np.median(x)) for x in t] + [batch_us])
        out("run %d (min .. max of the rounds in brackets):" % run)
        for name, x in zip(names, t):
            out("  %-66s %10.1f us   [%10.1f .. %10.1f]" % (name, float(np.median(x)), min(x), max(x)))
        out("  %-66s %10.1f us" % ("the batch's own pwpp_get_time_us", batch_us))
        del h
    m = np.array(medians)
    out()
    out("over the %d runs: median of the runs' medians, and their spread (max - min) between runs" % a.runs)
    for k, name in enumerate(names + ["the batch's own pwpp_get_time_us"]):
        out("  %-66s %10.1f us   spread %8.1f us" % (name, float(np.median(m[:, k])), float(m[:, k].max() - m[:, k].min())))
    out()
    med = {name: float(np.median(m[:, k])) for k, name in enumerate(names)}
    spr = {name: float(m[:, k].max() - m[:, k].min()) for k, name in enumerate(names)}
    wins = []
    for g in GRIDS:
        tag = "%d x %d of %.1f m" % g
        twin = abs(med["%s, max_range  0, viewshed path 2, shadow" % tag] - med["%s, max_range  0, viewshed path 2, shadow (A/A twin)" % tag])
        out("%s: the A/A twins differ by %.1f us" % (tag, twin))
        for r in RADII:
            vis = med["%s, max_range %2d, pwpp_visibility_grid" % (tag, r)]
            for shadow in ("shadow", "no shadow"):
                n1, n2 = ("%s, max_range %2d, viewshed path %d, %s" % (tag, r, p, shadow) for p in (1, 2))
                noise = max(spr[n1], spr[n2], twin)
                out("%s, max_range %2d, %-9s: path 1 %.1f us = %.2f x pwpp_visibility_grid, path 2 %.1f us = %.2f x; path 1 - path 2 = %.1f us against %.1f us of spread and A/A"
                    % (tag, r, shadow, med[n1], med[n1] / vis, med[n2], med[n2] / vis, med[n1] - med[n2], noise))
                wins.append(0 if abs(med[n1] - med[n2]) <= noise else (2 if med[n2] < med[n1] else 1))
            cv, c2 = med["%s, max_range %2d, pwpp_viewshed_obstacles" % (tag, r)], med["%s, max_range %2d, pwpp_visibility_obstacles" % (tag, r)]
            out("%s, max_range %2d: pwpp_viewshed_obstacles %.1f us = %.2f x pwpp_visibility_obstacles (%.1f us)" % (tag, r, cv, cv / c2, c2))
    out()
    out("path 2 is faster beyond the noise in %d of %d configurations, path 1 in %d, neither in %d" % (wins.count(2), len(wins), wins.count(1), wins.count(0)))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    del big


if __name__ == "__main__":
    main()
