"""What the obstacle boxes (pwpp_box_obstacles) cost on one MI355X (profiles/obstacle_boxes_cost.txt), and the A/B behind the
option "boxes_path": "1" every counted lane issues its atomics on its row, "2" the lanes of a wave that name the same row are
summed first ("0" is whichever of the two this file shows faster).

  * pwpp_box_obstacles of `frames` replayed KITTI frames in device memory, on the label image pwpp_label_obstacles wrote for the
    same grid (256 x 256 cells of 0.5 m, band [0.2, 2.5] m, min_count 1, connectivity 8), a table of 256 rows per frame, at
    both paths.
  * The yardsticks: pwpp_label_obstacles with point_cluster on the same batch -- the same two passes over every non-ground list
    (raster, per-point ids) plus the labelling -- pwpp_label_obstacles without the ids, and the batch's own pwpp_get_time_us.
  The protocol is that of tools/obstacle_clusters_cost.py: every figure is the median over `steps` rounds, a round runs each
  variant once, in turn; one measurement = `reps` calls enqueued back to back and one synchronise, host clock, divided by
  `reps`; the whole set is run `runs` times with fresh handles: the spread BETWEEN runs is what a difference between the two
  paths has to exceed to be a difference.

    python tools/obstacle_boxes_cost.py [--frames 1024] [--steps 7] [--warmup 2] [--reps 4] [--runs 3]
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

NX, NY, CELL = 256, 256, 0.5
BAND = (0.2, 2.5)
ROWS, BOXES = 64, 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "obstacle_boxes_cost.txt"))
    a = ap.parse_args()
    lines = []

    def out(s=""):
        print(s, flush=True)
        lines.append(s)

    src, kind = bench.load_source_frames("kitti")
    F = a.frames
    big, ptrs, ns, _ = device_batch(src, F, "row4")
    cells, x0, y0 = F * NX * NY, -0.5 * NX * CELL, -0.5 * NY * CELL
    d_label, d_scratch = (torch.empty(cells, dtype=torch.int32, device="cuda") for _ in range(2))
    d_table = torch.empty(F * ROWS * 12, dtype=torch.int32, device="cuda")
    d_n = torch.empty(F, dtype=torch.int32, device="cuda")
    d_pc = torch.empty(int(sum(ns)), dtype=torch.int32, device="cuda")
    d_boxes = torch.empty(F * BOXES * 16, dtype=torch.int32, device="cuda")
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

        def labels(into, ids):
            return lambda: h.label_obstacles_device(x0, y0, CELL, NX, NY, BAND[0], BAND[1], 1, 8, into.data_ptr(), 0, 0, d_table.data_ptr(), d_n.data_ptr(),
                                                    ROWS, d_pc.data_ptr() if ids else 0, 0, F)

        labels(d_label, False)()  # the label image every box call reads
        h.synchronize()

        def boxes(path):
            def go():
                h.set_option("boxes_path", path)
                return timed(lambda: h.box_obstacles_device(x0, y0, CELL, NX, NY, BAND[0], BAND[1], d_label.data_ptr(), d_boxes.data_ptr(), BOXES, 0, F),
                             h.synchronize)
            return go

        variants = [("box_obstacles, every lane its atomics (path 1)", boxes(1)),
                    ("box_obstacles, equal rows of a wave combined (path 2)", boxes(2)),
                    ("label_obstacles, connectivity 8, + point_cluster", lambda: timed(labels(d_scratch, True), h.synchronize)),
                    ("label_obstacles, connectivity 8", lambda: timed(labels(d_scratch, False), h.synchronize))]
        t = [[] for _ in variants]
        for r in range(a.warmup + a.steps):
            for k, (_, go) in enumerate(variants):
                v = go()
                if r >= a.warmup:
                    t[k].append(v)
        if head is None:
            got = []
            for path in (1, 2):
                h.set_option("boxes_path", path)
                h.box_obstacles_device(x0, y0, CELL, NX, NY, BAND[0], BAND[1], d_label.data_ptr(), d_boxes.data_ptr(), BOXES, 0, F)
                h.synchronize()
                got.append(d_boxes.cpu().numpy().tobytes())
            b = np.frombuffer(got[0], pwpp_hip.OBSTACLE_BOX_DTYPE).reshape(F, BOXES)
            n = d_n.cpu().numpy()
            head = "%s, %d frames, %d x %d cells of %.1f m, band [%.1f, %.1f] m, connectivity 8: %.0f clusters per frame (max %d), %d rows per frame, " \
                   "%.0f counted points per frame in %.0f boxes, %s" % (kind, F, NX, NY, CELL, BAND[0], BAND[1], n.mean(), n.max(), BOXES,
                                                                         b["points"].sum() / F, (b["points"] > 0).sum() / F, torch.cuda.get_device_name(0))
            out("obstacle_boxes_cost: " + head)
            out("the two paths give %s bytes" % ("IDENTICAL" if got[0] == got[1] else "DIFFERENT"))
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
        h.set_option("boxes_path", 0)
        del h
    m = np.array(medians)
    out()
    out("over the %d runs: median of the runs' medians, and their spread (max - min) between runs" % a.runs)
    for k, name in enumerate(names + ["the batch's own pwpp_get_time_us"]):
        out("  %-58s %10.1f us   spread %8.1f us" % (name, float(np.median(m[:, k])), float(m[:, k].max() - m[:, k].min())))
    out()
    plain, comb, ids, noids, batch = (float(np.median(m[:, k])) for k in range(5))
    spread = max(float(m[:, k].max() - m[:, k].min()) for k in (0, 1))
    out("plain %.1f us, combined %.1f us: plain - combined = %.1f us against a spread between runs of %.1f us" % (plain, comb, plain - comb, spread))
    out("against label_obstacles + point_cluster (%.1f us): plain %.2f x, combined %.2f x; the per-point pass of the ids alone is %.1f us; "
        "against the batch's own estimate (%.1f us): plain %.2f x, combined %.2f x" % (ids, plain / ids, comb / ids, ids - noids, batch, plain / batch, comb / batch))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    del big


if __name__ == "__main__":
    main()
