"""What the obstacle hulls (pwpp_hull_obstacles) cost on one MI355X (profiles/obstacle_hulls_cost.txt), and the A/B behind the option
"hulls_path": "1" a lane per row, serial gift wrapping and rectangle (the yardstick), "2" a wave per row ("0" is what
pwpp_hull_path_of in csrc/pwpp_hull.h makes of this file).

  * pwpp_hull_obstacles of `frames` replayed KITTI frames in device memory, on the label image pwpp_label_obstacles wrote for the same
    grid (band [0.2, 2.5] m, min_count 1, connectivity 8), tables of 256 rows per frame, lists of 32 vertices, at every path, on two
    grids: 256 x 256 cells of 0.5 m (many small clusters) and 64 x 64 cells of 2 m (few large ones).
  * A/A first: path 0 measured twice in every round, as two variants.  Their difference is the floor under which no difference
    between paths is one; path 0 may not be slower than the better of paths 1 and 2 by more than that floor.
  * Beside it pwpp_box_obstacles on the same labels and rows, and the batch's own pwpp_get_time_us.
  * The passes: the two point passes and the offsets are common to the paths, so path 2 - path 1 is the difference of the row
    kernels alone; --once runs every path once per grid for a kernel trace (rocprofv3 --kernel-trace --stats -- python
    tools/obstacle_hulls_cost.py --once), whose per-kernel figures are copied under the table by hand.
  The protocol is that of tools/obstacle_boxes_cost.py: every figure is the median over `steps` rounds, a round runs each variant
  once, in turn; one measurement = `reps` calls enqueued back to back and one synchronise, host clock, divided by `reps`; the whole
  set is run `runs` times with fresh handles.

    python tools/obstacle_hulls_cost.py [--frames 1024] [--steps 7] [--warmup 2] [--reps 4] [--runs 3] [--once]
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

GRIDS = ((256, 256, 0.5), (64, 64, 2.0))
BAND = (0.2, 2.5)
ROWS, HULLS, VERTICES = 64, 256, 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--once", action="store_true", help="every path once per grid and nothing written: for a kernel trace")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "obstacle_hulls_cost.txt"))
    a = ap.parse_args()
    lines = []

    def out(s=""):
        print(s, flush=True)
        lines.append(s)

    src, kind = bench.load_source_frames("kitti")
    F = a.frames
    big, ptrs, ns, _ = device_batch(src, F, "row4")
    d_table = torch.empty(F * ROWS * 12, dtype=torch.int32, device="cuda")
    d_n = torch.empty(F, dtype=torch.int32, device="cuda")
    d_hulls = torch.empty(F * HULLS * 16, dtype=torch.int32, device="cuda")
    d_lists = torch.empty(F * HULLS * VERTICES * 2, dtype=torch.int32, device="cuda")
    d_boxes = torch.empty(F * HULLS * 16, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def timed(enqueue, sync):
        t0 = time.perf_counter()
        for _ in range(a.reps):
            enqueue()
        sync()
        return (time.perf_counter() - t0) * 1e6 / a.reps

    out("obstacle_hulls_cost: %s, %d frames, band [%.1f, %.1f] m, connectivity 8, %d rows per frame, lists of %d vertices, %s"
        % (kind, F, BAND[0], BAND[1], HULLS, VERTICES, torch.cuda.get_device_name(0)))
    out("us per call: host clock over %d calls enqueued back to back + one synchronise; median of %d interleaved rounds after %d warm-up rounds;"
        % (a.reps, a.steps, a.warmup))
    out("%d runs of the whole set per grid, each with a fresh handle and batch" % a.runs)
    verdicts = []
    for NX, NY, CELL in GRIDS:
        x0, y0 = -0.5 * NX * CELL, -0.5 * NY * CELL
        d_label = torch.empty(F * NX * NY, dtype=torch.int32, device="cuda")
        names, medians, head = None, [], False
        for run in range(1 if a.once else a.runs):
            h = pwpp_hip.Handle()
            h.submit_batch(ptrs, ns, 4, pwpp_hip.LAYOUT_ROW_MAJOR, pwpp_hip.MEM_DEVICE, pwpp_hip.MODE_FRESH)
            h.synchronize()
            batch_us = h.time_us()
            h.label_obstacles_device(x0, y0, CELL, NX, NY, BAND[0], BAND[1], 1, 8, d_label.data_ptr(), 0, 0, d_table.data_ptr(), d_n.data_ptr(), ROWS, 0, 0, F)
            h.synchronize()

            def call(path):
                h.set_option("hulls_path", path)
                h.hull_obstacles_device(x0, y0, CELL, NX, NY, BAND[0], BAND[1], d_label.data_ptr(), d_hulls.data_ptr(), HULLS, d_lists.data_ptr(), VERTICES, 0, F)

            def hulls(path):
                return lambda: timed(lambda: call(path), h.synchronize)

            def boxes():
                return timed(lambda: h.box_obstacles_device(x0, y0, CELL, NX, NY, BAND[0], BAND[1], d_label.data_ptr(), d_boxes.data_ptr(), HULLS, 0, F), h.synchronize)

            if not head:
                got = []
                for path in (1, 2, 0):
                    call(path)
                    h.synchronize()
                    got.append(d_hulls.cpu().numpy().tobytes())
                r = np.frombuffer(got[0], pwpp_hip.OBSTACLE_HULL_DTYPE).reshape(F, HULLS)
                n, live = d_n.cpu().numpy(), r["points"] > 0
                out()
                out("%d x %d cells of %.1f m: %.0f clusters per frame (max %d), %.0f counted points per frame in %.0f rows; vertices per row: mean %.1f, max %d; "
                    "%d rows truncated at %d" % (NX, NY, CELL, n.mean(), n.max(), r["points"].sum() / F, live.sum() / F, r["n_vertices"][live].mean(),
                                                 r["n_vertices"].max(), (r["n_vertices"] > VERTICES).sum(), VERTICES))
                out("the three paths give %s bytes" % ("IDENTICAL" if got[0] == got[1] == got[2] else "DIFFERENT"))
                head = True
            if a.once:
                continue
            variants = [("hull_obstacles, path 0 (A)", hulls(0)), ("hull_obstacles, path 0 again (A)", hulls(0)),
                        ("hull_obstacles, a lane per row (path 1)", hulls(1)), ("hull_obstacles, a wave per row (path 2)", hulls(2)),
                        ("box_obstacles, same labels and rows", boxes)]
            t = [[] for _ in variants]
            for rnd in range(a.warmup + a.steps):
                for k, (_, go) in enumerate(variants):
                    v = go()
                    if rnd >= a.warmup:
                        t[k].append(v)
            names = [v[0] for v in variants]
            medians.append([float(np.median(x)) for x in t] + [batch_us])
            out("run %d (min .. max of the rounds in brackets):" % run)
            for name, x in zip(names, t):
                out("  %-44s %10.1f us   [%10.1f .. %10.1f]" % (name, float(np.median(x)), min(x), max(x)))
            out("  %-44s %10.1f us" % ("the batch's own pwpp_get_time_us", batch_us))
            h.set_option("hulls_path", 0)
            del h
        del d_label
        if a.once:
            continue
        m = np.array(medians)
        out("over the %d runs: median of the runs' medians, and their spread (max - min) between runs" % a.runs)
        for k, name in enumerate(names + ["the batch's own pwpp_get_time_us"]):
            out("  %-44s %10.1f us   spread %8.1f us" % (name, float(np.median(m[:, k])), float(m[:, k].max() - m[:, k].min())))
        a0, a1, lane, wave, box, batch = (float(np.median(m[:, k])) for k in range(6))
        floor = max(abs(a0 - a1), max(float(m[:, k].max() - m[:, k].min()) for k in (0, 1)))
        better = min(lane, wave)
        ok = min(a0, a1) <= better + floor
        verdicts.append(ok)
        out("A/A floor %.1f us (|A - A| of the medians, or the spread of A between runs, whichever is larger); path 1 %.1f us, path 2 %.1f us: the row kernels "
            "differ by %.1f us; path 0 %.1f us is %s the better of the two plus the floor (%.1f us)" % (floor, lane, wave, lane - wave, min(a0, a1),
                                                                                                       "WITHIN" if ok else "BEYOND", better + floor))
        out("against box_obstacles (%.1f us): path 0 %.2f x; against the batch's own estimate (%.1f us): %.2f x" % (box, min(a0, a1) / box, batch, min(a0, a1) / batch))
    if a.once:
        return
    out()
    out("path 0 within the floor of the better path on every grid: %s" % ("yes" if all(verdicts) else "NO"))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    del big


if __name__ == "__main__":
    main()
