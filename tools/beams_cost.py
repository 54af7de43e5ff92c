"""What the per-beam free space (pwpp_rasterize_beams, pwpp_beam_grid, pwpp_beam_ground) costs on one MI355X
(profiles/beams_cost.txt), and the A/B of the option "beams_path": "1" a lane per endpoint cell with atomics on the global images
after a fill, "2" a workgroup per tile of 64 x 64 cells with the tile's passes and low in LDS.

  * The images: pwpp_rasterize_beams (which = 1, the ground lists) of `frames` replayed KITTI frames written straight into device
    memory, pwpp_rasterize_ground quantised on the host with the restatement's quantiser, and the bytes pwpp_viewshed_obstacles
    gives for the same frames (band [0.2, 2.5] m, min_seen 1) as the base bytes, on two grids -- 256 x 256 cells of 0.5 m and 64 x 64
    cells of 2 m.  The sensor is the origin of the model's frame: eye = units(0).
  * pwpp_rasterize_beams alone; pwpp_beam_grid on the images, paths 1 and 2, unlimited and within 20 m (40 and 10 cells), min_pass 2,
    clearance 0.3 m; the chained pwpp_beam_ground (default path); next to them pwpp_viewshed_obstacles on the same frames.
  * Path 2 once more on hits images that are all zero: no endpoint is queued or walked, what remains is every tile's scan of the
    frame's endpoint images and the write-out -- the part of path 2 a compacted endpoint list would remove.
  * A/A twins: path 2, unlimited, is measured twice per round under two names; their difference is what the method cannot resolve.
    The floor: an empty call (pwpp_synchronize alone).
  Every figure is the median over `steps` rounds; a round runs each variant once, in turn (interleaved), so that a drift of the
  clocks hits every variant alike.  One measurement = `reps` calls enqueued back to back and one synchronise, timed with the host
  clock and divided by the number of calls -- `reps` on the fine grid, 16 x `reps` on the coarse one, where a call takes well under
  0.1 ms and a window of four would time the clock.  The whole set is run `runs` times in this process (fresh handles each time): the spread BETWEEN
  runs, and the A/A difference, are what a difference between two paths has to exceed to be a difference.
  It also reports the endpoint cells and the cells that a beam crossed per frame, and on the six KITTI frames themselves the share of cells FREE after the
  viewshed and after the beams on top of it (which = 1, min_pass 1 and 2, clearance 0.3 m).

    python tools/beams_cost.py [--frames 1024] [--steps 7] [--warmup 2] [--reps 4] [--runs 3]
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

import beams_ref as br  # noqa: E402
import bench  # noqa: E402
import pwpp_hip  # noqa: E402
from point_records_cost import device_batch  # noqa: E402

GRIDS = [(256, 256, 0.5), (64, 64, 2.0)]  # (nx, ny, cell)
WITHIN = 20.0                             # metres: the limited calls
BAND = (0.2, 2.5)
MIN_PASS, CLEARANCE = 2, 0.3


def radii(cell):
    return (0, int(round(WITHIN / cell)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "beams_cost.txt"))
    a = ap.parse_args()
    lines = []

    def out(s=""):
        print(s, flush=True)
        lines.append(s)

    src, kind = bench.load_source_frames("kitti")
    F = a.frames
    big, ptrs, ns, _ = device_batch(src, F, "row4")
    cells = F * max(nx * ny for nx, ny, _ in GRIDS)
    d_passes, d_low, d_hits, d_zmin, d_first, d_shadow, d_count = (torch.empty(cells, dtype=torch.int32, device="cuda") for _ in range(7))
    d_occ = torch.empty(cells, dtype=torch.int8, device="cuda")
    d_zero = torch.zeros(cells, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    eye, clear_units = br.units(0.0), br.units(CLEARANCE)

    def timed(enqueue, sync, reps=None):
        reps = reps or a.reps
        t0 = time.perf_counter()
        for _ in range(reps):
            enqueue()
        sync()
        return (time.perf_counter() - t0) * 1e6 / reps

    def reps_of(grid):  # calls of one measurement: 16 times as many on the coarse grid, where a call takes well under 0.1 ms
        return a.reps * (16 if grid[0] * grid[1] <= 64 * 64 else 1)

    def corner(g):
        nx, ny, cell = g
        return -0.5 * nx * cell, -0.5 * ny * cell

    names, medians, head, images = None, [], False, {}
    for run in range(a.runs):
        h = pwpp_hip.Handle()
        h.submit_batch(ptrs, ns, 4, pwpp_hip.LAYOUT_ROW_MAJOR, pwpp_hip.MEM_DEVICE, pwpp_hip.MODE_FRESH)
        h.synchronize()
        batch_us = h.time_us()
        for g in GRIDS if run == 0 else ():  # hits, zmin, target and the viewshed's bytes of a grid, once, in device memory
            nx, ny, cell = g
            x0, y0 = corner(g)
            n = F * nx * ny
            hits, zmin = (torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(2))
            base = torch.empty(n, dtype=torch.int8, device="cuda")
            h.rasterize_beams_device(x0, y0, cell, nx, ny, hits.data_ptr(), zmin.data_ptr(), 1, 0, F)
            h.viewshed_obstacles_device(x0, y0, cell, nx, ny, BAND[0], BAND[1], (0.0, 0.0, 0.0), 1, 1, 0, d_first.data_ptr(), 0, base.data_ptr(), 0, 0, F)
            h.synchronize()
            ground = h.rasterize_ground(x0, y0, cell, nx, ny, frames=F).astype(np.float64)
            images[g] = [hits, zmin, torch.from_numpy(np.ascontiguousarray(br.units_image(ground)).reshape(-1)).cuda(), base]
        torch.cuda.synchronize()

        def beams(grid, max_range, path, empty=False):
            nx, ny, cell = grid
            hi, zm, tg, ba = (x.data_ptr() for x in images[grid])
            if empty:  # no endpoint anywhere: what is left of path 2 is the tiles' scans of the endpoint images and the write-out
                hi = d_zero.data_ptr()

            def go():
                h.set_option("beams_path", path)
                return timed(lambda: h.beam_grid_device(nx, ny, F, hi, zm, (nx // 2, ny // 2, eye), max_range, MIN_PASS, clear_units, d_passes.data_ptr(),
                                                        d_low.data_ptr(), d_occ.data_ptr(), tg, ba), h.synchronize, reps_of(grid))
            return go

        def raster(grid):
            nx, ny, cell = grid
            x0, y0 = corner(grid)
            return lambda: timed(lambda: h.rasterize_beams_device(x0, y0, cell, nx, ny, d_hits.data_ptr(), d_zmin.data_ptr(), 1, 0, F), h.synchronize, reps_of(grid))

        def chained(grid, max_range, which):
            nx, ny, cell = grid
            x0, y0 = corner(grid)
            ba = images[grid][3].data_ptr()

            def go():
                h.set_option("beams_path", 0)
                if which == "beams":
                    return timed(lambda: h.beam_ground_device(x0, y0, cell, nx, ny, (0.0, 0.0, 0.0), 1, max_range, MIN_PASS, CLEARANCE, d_passes.data_ptr(),
                                                              d_low.data_ptr(), d_occ.data_ptr(), ba, 0, 0, 0, F), h.synchronize, reps_of(grid))
                return timed(lambda: h.viewshed_obstacles_device(x0, y0, cell, nx, ny, BAND[0], BAND[1], (0.0, 0.0, 0.0), 1, 1, max_range, d_first.data_ptr(),
                                                                 d_shadow.data_ptr(), d_occ.data_ptr(), d_count.data_ptr(), 0, F), h.synchronize, reps_of(grid))
            return go

        variants = []
        for g in GRIDS:
            tag = "%d x %d of %.1f m" % g
            variants.append(("%s, pwpp_rasterize_beams" % tag, raster(g)))
            for r in radii(g[2]):
                for path in (1, 2):
                    variants.append(("%s, max_range %2d, beams path %d" % (tag, r, path), beams(g, r, path)))
                variants.append(("%s, max_range %2d, pwpp_beam_ground" % (tag, r), chained(g, r, "beams")))
                variants.append(("%s, max_range %2d, pwpp_viewshed_obstacles" % (tag, r), chained(g, r, "viewshed")))
            variants.append(("%s, max_range  0, beams path 2 (A/A twin)" % tag, beams(g, 0, 2)))
            variants.append(("%s, max_range  0, beams path 2, no endpoints" % tag, beams(g, 0, 2, True)))
        variants.append(("floor: pwpp_synchronize alone", lambda: timed(lambda: None, h.synchronize)))
        t = [[] for _ in variants]
        for r in range(a.warmup + a.steps):
            for k, (_, go) in enumerate(variants):
                v = go()
                if r >= a.warmup:
                    t[k].append(v)
        if not head:
            head = True
            out("beams_cost: %s, %d frames, which = 1 (ground lists), min_pass %d, clearance %.1f m, origin {0, 0, 0}, base bytes: pwpp_viewshed_obstacles (band [%.1f, %.1f] m, "
                "min_seen 1), %s" % (kind, F, MIN_PASS, CLEARANCE, BAND[0], BAND[1], torch.cuda.get_device_name(0)))
            for g in GRIDS:
                nx, ny, cell = g
                n = F * nx * ny
                hi, zm, tg, ba = images[g]
                ends = int(((hi >= 1) & (zm != br.NO_HEIGHT)).sum().item())
                h.set_option("beams_path", 0)
                h.beam_grid_device(nx, ny, F, hi.data_ptr(), zm.data_ptr(), (nx // 2, ny // 2, eye), 0, MIN_PASS, clear_units, d_passes.data_ptr(), d_low.data_ptr(),
                                   d_occ.data_ptr(), tg.data_ptr(), ba.data_ptr())
                h.synchronize()
                crossed = int((d_passes[:n] != 0).sum().item())
                out("  %d x %d cells of %.1f m: %.0f points in the ground lists' cells, %.0f endpoint cells and %.0f cells that a beam crossed per frame"
                    % (nx, ny, cell, float(hi.sum(dtype=torch.int64).item()) / F, ends / F, crossed / F))
            out("us per call: host clock over %d calls (64 x 64: %d) enqueued back to back + one synchronise; median of %d interleaved rounds after %d warm-up rounds;"
                % (a.reps, 16 * a.reps, a.steps, a.warmup))
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
        twin = abs(med["%s, max_range  0, beams path 2" % tag] - med["%s, max_range  0, beams path 2 (A/A twin)" % tag])
        out("%s: the A/A twins differ by %.1f us" % (tag, twin))
        for r in radii(g[2]):
            n1, n2 = ("%s, max_range %2d, beams path %d" % (tag, r, p) for p in (1, 2))
            noise = max(spr[n1], spr[n2], twin)
            view = med["%s, max_range %2d, pwpp_viewshed_obstacles" % (tag, r)]
            out("%s, max_range %2d: path 1 %.1f us, path 2 %.1f us; path 1 - path 2 = %.1f us against %.1f us of spread and A/A" % (tag, r, med[n1], med[n2], med[n1] - med[n2], noise))
            chain = med["%s, max_range %2d, pwpp_beam_ground" % (tag, r)]
            out("%s, max_range %2d: pwpp_beam_ground %.1f us = %.2f x pwpp_viewshed_obstacles (%.1f us)" % (tag, r, chain, chain / view, view))
            wins.append(0 if abs(med[n1] - med[n2]) <= noise else (2 if med[n2] < med[n1] else 1))
        bare, full = med["%s, max_range  0, beams path 2, no endpoints" % tag], med["%s, max_range  0, beams path 2" % tag]
        out("%s, max_range  0: path 2 on images without an endpoint (the tiles' scans and the write-out alone) %.1f us = %.0f %% of its %.1f us on the frames' endpoints"
            % (tag, bare, 100.0 * bare / full, full))
    out()
    out("path 2 is faster beyond the noise in %d of %d configurations, path 1 in %d, neither in %d" % (wins.count(2), len(wins), wins.count(1), wins.count(0)))
    out()

    # the six KITTI frames themselves: what the beams add to the viewshed's free space
    six = [np.ascontiguousarray(f, np.float32) for f in src[:6]]
    h = pwpp_hip.Handle()
    h.estimate_ground_batch(six, mode=pwpp_hip.MODE_FRESH)
    out("the %d source frames: share of the cells FREE after pwpp_viewshed_obstacles (band [%.1f, %.1f] m, min_seen 1) and after pwpp_beam_ground on top of its bytes"
        % (len(six), BAND[0], BAND[1]))
    for g in GRIDS:
        nx, ny, cell = g
        x0, y0 = corner(g)
        base = h.viewshed_obstacles(x0, y0, cell, nx, ny, BAND[0], BAND[1], min_seen=1, want_shadow=False)[2]
        share = lambda occ: 100.0 * float((occ == pwpp_hip.OCC_FREE).sum()) / occ.size
        row = "  %d x %d cells of %.1f m: viewshed %5.1f %%" % (nx, ny, cell, share(base))
        for min_pass in (1, 2):
            occ = h.beam_ground(x0, y0, cell, nx, ny, which=1, occupancy_in=base, min_pass=min_pass, clearance=CLEARANCE)[2]
            assert (occ[base != pwpp_hip.OCC_UNKNOWN] == base[base != pwpp_hip.OCC_UNKNOWN]).all()
            row += ", + beams (which = 1, min_pass %d, clearance %.1f m) %5.1f %%" % (min_pass, CLEARANCE, share(occ))
        out(row + "; occupied %5.1f %%" % (100.0 * float((base == pwpp_hip.OCC_OCCUPIED).sum()) / base.size))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    del big


if __name__ == "__main__":
    main()
