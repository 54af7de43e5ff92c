"""What the cluster association (pwpp_associate_grid, pwpp_track_obstacles) costs on one MI355X (profiles/tracks_cost.txt).  There is
one path through the kernels (csrc/pwpp_tracks.hip: the pair tables in global memory), so the twin below measures the noise floor
and no option is decided here.

  * `frames` replayed KITTI frames in device memory; their label images (pwpp_label_obstacles, heights 0.3 .. 2.5 m, 8-connected,
    `--max-clusters` rows) on 256 x 256 cells of 0.5 m and on 64 x 64 cells of 2 m.  The previous image of frame f is the label
    image of frame f - 1 of the replay (of the last frame for f = 0), the pose the identity; the replay cycles the sample scans, so
    a frame and its predecessor are two different scans of one drive.
  * pwpp_associate_grid alone on those images with ids, at gate 0 and at gate 2, each twice (the A/A twin: the same variant under
    another name, whose distance from the first is the floor no difference can be read below).
  * pwpp_track_obstacles (256 x 256, gate 0) and pwpp_label_obstacles alone on the same handle and grid in the same rounds: the
    association's cost on top of the labelling is the difference.
  Every figure is the median over `steps` rounds; a round runs each variant once, in turn (interleaved), every other round in
  reversed order.  One measurement = `reps` calls enqueued back to back and one synchronise, timed with the host clock and divided
  by `reps` -- 16 times as many calls for the 64 x 64 shape.  The output begins with the command line it was made with.  The whole
  set is run `runs` times in this process (fresh handles each time).

    python tools/tracks_cost.py [--frames 1024] [--steps 5] [--warmup 1] [--reps 2] [--runs 2] [--max-clusters 256]
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

SHAPES = ((256, 0.5), (64, 2.0))  # (cells a side, metres a cell)
BAND = (0.3, 2.5)
GATES = (0, 2)
SMALL_REPS = 16  # times --reps for the shapes below 256 cells a side
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--max-clusters", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tracks_cost.txt"))
    a = ap.parse_args()
    lines = []

    def out(s=""):
        print(s, flush=True)
        lines.append(s)

    src, kind = bench.load_source_frames("kitti")
    F, R = a.frames, a.max_clusters
    P = 4 * R  # max_pairs
    big, ptrs, ns, _ = device_batch(src, F, "row4")
    i32 = lambda n, fill=0: torch.full((n,), fill, dtype=torch.int32, device="cuda")
    d_label = {n: i32(F * n * n) for n, _ in SHAPES}
    d_prev = {n: i32(F * n * n) for n, _ in SHAPES}
    d_table = torch.zeros(F * R * 48, dtype=torch.uint8, device="cuda")
    d_n = i32(F)
    d_cl, d_pl = i32(F * R * 4), i32(F * R * 4)
    d_pairs, d_id_prev, d_next, d_id_curr, d_next_out = i32(F), i32(F * R, 1), i32(F, 1000), i32(F * R), i32(F)
    torch.cuda.synchronize()

    def timed(enqueue, sync, reps=None):
        reps = reps or a.reps
        t0 = time.perf_counter()
        for _ in range(reps):
            enqueue()
        sync()
        return (time.perf_counter() - t0) * 1e6 / reps

    reps_of = lambda n: a.reps * (SMALL_REPS if n < 256 else 1)

    names, medians, head = None, [], False
    for run in range(a.runs):
        h = pwpp_hip.Handle()
        h.submit_batch(ptrs, ns, 4, pwpp_hip.LAYOUT_ROW_MAJOR, pwpp_hip.MEM_DEVICE, pwpp_hip.MODE_FRESH)
        h.synchronize()
        batch_us = h.time_us()

        def label(n, cell):
            x0 = -0.5 * n * cell
            return timed(lambda: h.label_obstacles_device(x0, x0, cell, n, n, BAND[0], BAND[1], 1, 8, d_label[n].data_ptr(), 0, 0, d_table.data_ptr(), d_n.data_ptr(),
                                                          R, 0, 0, F), h.synchronize, reps_of(n))

        def associate(n, cell, gate):
            x0 = -0.5 * n * cell
            g = (x0, x0, cell, n, n)
            return lambda: timed(lambda: h.associate_grid_device(g, g, F, d_label[n].data_ptr(), d_prev[n].data_ptr(), IDENTITY, gate, 1, R, P, d_cl.data_ptr(),
                                                                 d_pl.data_ptr(), d_pairs.data_ptr(), d_id_prev.data_ptr(), d_next.data_ptr(), d_id_curr.data_ptr(),
                                                                 d_next_out.data_ptr()), h.synchronize, reps_of(n))

        def track(n, cell, gate):
            x0 = -0.5 * n * cell
            return lambda: timed(lambda: h.track_obstacles_device(x0, x0, cell, n, n, BAND[0], BAND[1], 1, 8, d_label[n].data_ptr(), d_prev[n].data_ptr(), IDENTITY, gate,
                                                                  1, R, P, d_cl.data_ptr(), d_pl.data_ptr(), d_pairs.data_ptr(), d_id_prev.data_ptr(), d_next.data_ptr(),
                                                                  d_id_curr.data_ptr(), d_next_out.data_ptr(), 0, 0, d_table.data_ptr(), d_n.data_ptr(), 0, 0, F),
                                 h.synchronize, reps_of(n))

        for n, cell in SHAPES:
            label(n, cell)  # (d_label[n] holds the frames' label images from here on; the previous image of a frame is its predecessor's)
            d_prev[n].copy_(torch.roll(d_label[n].view(F, n * n), 1, 0).reshape(-1))
        torch.cuda.synchronize()
        variants, cases = [], []
        for n, cell in SHAPES:
            for gate in GATES:
                cases.append((n, gate))
                for tag in ("", " twin"):
                    variants.append(("pwpp_associate_grid %d x %d, gate %d%s" % (n, n, gate, tag), associate(n, cell, gate)))
        n0, cell0 = SHAPES[0]
        variants.append(("pwpp_track_obstacles %d x %d, gate 0" % (n0, n0), track(n0, cell0, 0)))
        variants.append(("pwpp_label_obstacles %d x %d alone" % (n0, n0), lambda: label(n0, cell0)))
        t = [[] for _ in variants]
        for rnd in range(a.warmup + a.steps):
            order = range(len(variants)) if rnd % 2 == 0 else range(len(variants) - 1, -1, -1)
            for k in order:
                v = variants[k][1]()
                if rnd >= a.warmup:
                    t[k].append(v)
            print("run %d, round %d of %d done" % (run, rnd + 1, a.warmup + a.steps), file=sys.stderr, flush=True)
        if not head:
            head = True
            out("python tools/tracks_cost.py --frames %d --steps %d --warmup %d --reps %d --runs %d --max-clusters %d" % (F, a.steps, a.warmup, a.reps, a.runs, R))
            out("tracks_cost: %s, %d frames, %s" % (kind, F, torch.cuda.get_device_name(0)))
            out("labels: heights %g .. %g m, min_count 1, 8-connected, max_rows %d, max_pairs %d; previous image = the predecessor's labels, identity pose, ids on" % (BAND + (R, P)))
            for n, cell in SHAPES:
                for gate in GATES:
                    associate(n, cell, gate)()
                    torch.cuda.synchronize()
                    lab = d_label[n]
                    named = int(((lab >= 0) & (lab < R)).sum().item())
                    cl = d_cl.view(F, R, 4)
                    rows_of = (cl[:, :, 2] > 0).sum(1)  # the rows of a frame that exist
                    out("  %d x %d cells of %.1f m, gate %d: %.2f %% of the cells carry a row, %.1f existing rows a frame (most %d), %.1f pairs a frame (most %d), "
                        "%d frames overflowed, %.1f %% of the existing rows continue an id"
                        % (n, n, cell, gate, 100.0 * named / lab.numel(), float(rows_of.float().mean().item()), int(rows_of.max().item()), float(d_pairs.float().mean().item()),
                           int(d_pairs.max().item()), int((d_pairs > P).sum().item()),
                           100.0 * int(((cl[:, :, 2] > 0) & (d_id_curr.view(F, R) == 1)).sum().item()) / max(1, int((cl[:, :, 2] > 0).sum().item()))))
            out("us per call: host clock over %d calls (%d for the shapes below 256 cells a side) enqueued back to back + one synchronise; median of %d "
                "interleaved rounds (every other one reversed)" % (a.reps, a.reps * SMALL_REPS, a.steps))
            out("after %d warm-up rounds; %d runs of the whole set, each with a fresh handle and batch" % (a.warmup, a.runs))
            out()
        names = [v[0] for v in variants]
        medians.append([float(np.median(x)) for x in t] + [batch_us])
        out("run %d (min .. max of the rounds in brackets):" % run)
        for name, x in zip(names, t):
            out("  %-56s %12.1f us   [%12.1f .. %12.1f]" % (name, float(np.median(x)), min(x), max(x)))
        out("  %-56s %12.1f us" % ("the batch's own pwpp_get_time_us", batch_us))
        del h
    m = np.array(medians)
    out()
    out("over the %d runs: median of the runs' medians, and their spread (max - min) between runs" % a.runs)
    for k, name in enumerate(names + ["the batch's own pwpp_get_time_us"]):
        out("  %-56s %12.1f us   spread %10.1f us" % (name, float(np.median(m[:, k])), float(m[:, k].max() - m[:, k].min())))
    out()
    med = lambda k: float(np.median(m[:, k]))
    spread = lambda k: float(m[:, k].max() - m[:, k].min())
    for ci, (n, gate) in enumerate(cases):
        k1, kt = 2 * ci, 2 * ci + 1
        floor = max(abs(med(k1) - med(kt)), spread(k1), spread(kt))
        out("pwpp_associate_grid %d x %d, gate %d: %.1f us, its twin %.1f us, floor %.1f us; %.3f us a frame; %.1f GB/s of the two label images"
            % (n, n, gate, med(k1), med(kt), floor, med(k1) / F, 2 * 4 * F * n * n / med(k1) / 1e3))
    base = 2 * len(cases)
    lab = med(base + 1)
    out("pwpp_track_obstacles %d x %d, gate 0: %.1f us; pwpp_label_obstacles alone %.1f us (spread %.1f): the association on top of it %.1f us"
        % (n0, n0, med(base), lab, spread(base + 1), med(base) - lab))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    del big


if __name__ == "__main__":
    main()
