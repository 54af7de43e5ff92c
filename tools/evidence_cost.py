"""What the map evidence (pwpp_evidence_grid, pwpp_evidence_obstacles) costs on one MI355X, and which path of its count kernel the
option "evidence_path" = 0 should mean (profiles/evidence_cost.txt): path 1, the sums go to the rows with global atomics, against
path 2, a workgroup sums a run of cells in LDS first (csrc/pwpp_evidence.hip).

  * `frames` replayed KITTI frames in device memory; their label images (pwpp_label_obstacles, heights 0.3 .. 2.5 m, 8-connected,
    `--max-clusters` rows) on 256 x 256 cells of 0.5 m and on 64 x 64 cells of 2 m; one map per shape on the same grid, fused from
    the same replay under the identity pose (pwpp_fuse_obstacles), whose per-frame bytes are the occupancy the mask works on.
  * pwpp_evidence_grid alone on those images under the identity pose, at gate 0 and at gate 2, on path 1 and on path 2, the rows
    alone and with the class image and the masked bytes, each twice (the A/A twin: the same variant under another name, whose
    distance from the first is the floor no difference can be read below).
  * pwpp_evidence_obstacles (256 x 256, gate 0, rows alone) and pwpp_label_obstacles alone on the same handle and grid in the same
    rounds: the evidence's cost on top of the labelling is the difference.
  Every figure is the median over `steps` rounds; a round runs each variant once, in turn (interleaved), every other round in
  reversed order.  One measurement = `reps` calls enqueued back to back and one synchronise, timed with the host clock and divided
  by `reps` -- 16 times as many calls for the 64 x 64 shape.  The output begins with the command line it was made with.  The whole
  set is run `runs` times in this process (fresh handles each time).  A path wins a shape where it is faster by more than the
  floor: the larger of the A/A distances and the spreads between runs of the two variants compared.

    python tools/evidence_cost.py [--frames 1024] [--steps 5] [--warmup 1] [--reps 2] [--runs 2] [--max-clusters 256]
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
PATHS = (1, 2)
SMALL_REPS = 16  # times --reps for the shapes below 256 cells a side
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
RULE = (0, 3, 192, 192)  # (the gate is set per variant)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--max-clusters", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "evidence_cost.txt"))
    a = ap.parse_args()
    lines = []

    def out(s=""):
        print(s, flush=True)
        lines.append(s)

    src, kind = bench.load_source_frames("kitti")
    F, R = a.frames, a.max_clusters
    big, ptrs, ns, _ = device_batch(src, F, "row4")
    i32 = lambda n, fill=0: torch.full((n,), fill, dtype=torch.int32, device="cuda")
    i8 = lambda n: torch.zeros(n, dtype=torch.int8, device="cuda")
    d_label = {n: i32(F * n * n) for n, _ in SHAPES}
    d_occ = {n: i8(F * n * n) for n, _ in SHAPES}
    d_map = {n: torch.zeros(n * n, dtype=torch.int16, device="cuda") for n, _ in SHAPES}
    d_class, d_masked = i8(F * 256 * 256), i8(F * 256 * 256)
    d_table = torch.zeros(F * R * 48, dtype=torch.uint8, device="cuda")
    d_n = i32(F)
    d_rows = torch.zeros(F * R * 4, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    fmap = lambda n, cell: pwpp_hip.FusionMap(-0.5 * n * cell, -0.5 * n * cell, cell, n, n, 40, 20, -350, 350, 100, -60)

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

        def evidence(n, cell, gate, path, images):
            x0 = -0.5 * n * cell
            rule = (gate,) + RULE[1:]

            def one():
                h.set_option("evidence_path", path)
                return timed(lambda: h.evidence_grid_device((x0, x0, cell), n, n, F, d_label[n].data_ptr(), IDENTITY, fmap(n, cell), 1, d_map[n].data_ptr(), rule, R,
                                                            d_rows.data_ptr(), d_class.data_ptr() if images else 0, d_occ[n].data_ptr() if images else 0,
                                                            d_masked.data_ptr() if images else 0), h.synchronize, reps_of(n))
            return one

        def chain(n, cell, gate):
            x0 = -0.5 * n * cell

            def one():
                h.set_option("evidence_path", 0)
                return timed(lambda: h.evidence_obstacles_device(x0, x0, cell, n, n, BAND[0], BAND[1], 1, 8, d_label[n].data_ptr(), IDENTITY, fmap(n, cell), 1,
                                                                 d_map[n].data_ptr(), (gate,) + RULE[1:], R, d_rows.data_ptr(), clusters_ptr=d_table.data_ptr(),
                                                                 n_clusters_ptr=d_n.data_ptr(), frames=F), h.synchronize, reps_of(n))
            return one

        for n, cell in SHAPES:
            x0 = -0.5 * n * cell
            label(n, cell)  # (d_label[n] holds the frames' label images from here on)
            d_map[n].zero_()
            h.fuse_obstacles_device(x0, x0, cell, n, n, BAND[0], BAND[1], IDENTITY, fmap(n, cell), 1, 0, d_map[n].data_ptr(), 0, d_occ[n].data_ptr(), frames=F)
            h.synchronize()
        torch.cuda.synchronize()
        variants, cases = [], []
        for n, cell in SHAPES:
            for gate in GATES:
                for images in (False, True):
                    cases.append((n, gate, images))
                    for path in PATHS:
                        for tag in ("", " twin"):
                            variants.append(("evidence_grid %d x %d, gate %d, %s, path %d%s" % (n, n, gate, "rows + images" if images else "rows", path, tag),
                                             evidence(n, cell, gate, path, images)))
        n0, cell0 = SHAPES[0]
        variants.append(("pwpp_evidence_obstacles %d x %d, gate 0, rows" % (n0, n0), chain(n0, cell0, 0)))
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
            out("python tools/evidence_cost.py --frames %d --steps %d --warmup %d --reps %d --runs %d --max-clusters %d" % (F, a.steps, a.warmup, a.reps, a.runs, R))
            out("evidence_cost: %s, %d frames, %s" % (kind, F, torch.cuda.get_device_name(0)))
            out("labels: heights %g .. %g m, min_count 1, 8-connected, max_rows %d; one map per shape fused from the same frames (hit 40, miss 20, occupied_at 100, "
                "free_at -60), identity pose; rule: min_cells %d, shares %d / %d" % (BAND + (R,) + RULE[1:]))
            for n, cell in SHAPES:
                for gate in GATES:
                    evidence(n, cell, gate, 1, False)()
                    torch.cuda.synchronize()
                    lab = d_label[n]
                    named = int(((lab >= 0) & (lab < R)).sum().item())
                    rows = d_rows.view(torch.int32).view(F, R, 8)  # sum (2 words), cells, landed, occupied, free, unknown, verdict
                    exist = rows[:, :, 2] > 0
                    verdicts = [int(((rows[:, :, 7] == v) & exist).sum().item()) for v in (0, 1, 2)]
                    out("  %d x %d cells of %.1f m, gate %d: %.2f %% of the cells carry a row, %.1f existing rows a frame (most %d), %.1f %% of their cells landed; "
                        "verdicts of the existing rows: %.1f %% undecided, %.1f %% static, %.1f %% moving"
                        % (n, n, cell, gate, 100.0 * named / lab.numel(), float(exist.sum(1).float().mean().item()), int(exist.sum(1).max().item()),
                           100.0 * int(rows[:, :, 3].sum().item()) / max(1, int(rows[:, :, 2].sum().item())), *[100.0 * v / max(1, int(exist.sum().item())) for v in verdicts]))
            out("us per call: host clock over %d calls (%d for the shapes below 256 cells a side) enqueued back to back + one synchronise; median of %d "
                "interleaved rounds (every other one reversed)" % (a.reps, a.reps * SMALL_REPS, a.steps))
            out("after %d warm-up rounds; %d runs of the whole set, each with a fresh handle and batch" % (a.warmup, a.runs))
            out()
        names = [v[0] for v in variants]
        medians.append([float(np.median(x)) for x in t] + [batch_us])
        out("run %d (min .. max of the rounds in brackets):" % run)
        for name, x in zip(names, t):
            out("  %-64s %12.1f us   [%12.1f .. %12.1f]" % (name, float(np.median(x)), min(x), max(x)))
        out("  %-64s %12.1f us" % ("the batch's own pwpp_get_time_us", batch_us))
        del h
    m = np.array(medians)
    out()
    out("over the %d runs: median of the runs' medians, and their spread (max - min) between runs" % a.runs)
    for k, name in enumerate(names + ["the batch's own pwpp_get_time_us"]):
        out("  %-64s %12.1f us   spread %10.1f us" % (name, float(np.median(m[:, k])), float(m[:, k].max() - m[:, k].min())))
    out()
    med = lambda k: float(np.median(m[:, k]))
    spread = lambda k: float(m[:, k].max() - m[:, k].min())
    wins = {1: 0, 2: 0}
    for ci, (n, gate, images) in enumerate(cases):
        k1, k1t, k2, k2t = 4 * ci, 4 * ci + 1, 4 * ci + 2, 4 * ci + 3
        floor = max(abs(med(k1) - med(k1t)), abs(med(k2) - med(k2t)), spread(k1), spread(k1t), spread(k2), spread(k2t))
        diff = med(k2) - med(k1)
        verdict = "no difference beyond the floor" if abs(diff) <= floor else ("path 2 wins" if diff < 0 else "path 1 wins")
        if n == SHAPES[0][0] and abs(diff) > floor:
            wins[2 if diff < 0 else 1] += 1
        out("%d x %d, gate %d, %s: path 1 %.1f us (twin %.1f), path 2 %.1f us (twin %.1f), floor %.1f us: %s; %.3f us a frame on path 1"
            % (n, n, gate, "rows + images" if images else "rows", med(k1), med(k1t), med(k2), med(k2t), floor, verdict, med(k1) / F))
    n_big = sum(1 for c in cases if c[0] == SHAPES[0][0])
    if wins[2] == n_big:
        out("path 2 wins every %d x %d case beyond the floor: kEvidDefaultLds = true" % (SHAPES[0][0], SHAPES[0][0]))
    elif wins[2] == 0:
        out("path 2 wins no %d x %d case beyond the floor: kEvidDefaultLds = false, path 0 is path 1 and path 2 stays the option" % (SHAPES[0][0], SHAPES[0][0]))
    else:
        out("path 2 wins %d of the %d cases of %d x %d beyond the floor and path 1 %d: no path wins the shape; kEvidDefaultLds = false"
            % (wins[2], n_big, SHAPES[0][0], SHAPES[0][0], wins[1]))
    base = 4 * len(cases)
    lab = med(base + 1)
    out("pwpp_evidence_obstacles %d x %d, gate 0: %.1f us; pwpp_label_obstacles alone %.1f us (spread %.1f): the evidence on top of it %.1f us"
        % (n0, n0, med(base), lab, spread(base + 1), med(base) - lab))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    del big


if __name__ == "__main__":
    main()
