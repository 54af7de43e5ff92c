"""What the per-point patch rows and plane distances cost on one MI355X (profiles/point_planes_cost.txt).

Three settings -- default, point planes, point planes + labels -- on
  * 1024 replayed KITTI frames from device memory, overlap schedule (bench.py's configs[2] shape),
  * the same batch on the single-stream schedule,
  * one fresh KITTI frame from host memory (the latency path).
GPU time of a call = pwpp_get_time_us (first kernel -> lists and point planes written): median of `steps` calls after `warmup`,
settings interleaved round by round so that clock drift hits all of them alike.  The spread (min .. max, and the half
interquartile range) of the default's calls is printed next to the medians: a difference below it is noise.  Then one profiled
call per setting on the single-stream schedule: the k_emit slot, which holds the new kernels (k_pp_prep, k_pp_patch); its
growth over the default is their time, set against the bytes they must move (8 B per point filled, 16 B read and 8 B written per
point of a patch) and the copy roof of profiles/r06_copy_bw.txt (~5 TB/s).

    python tools/point_planes_cost.py [--steps 20] [--warmup 5]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("tests", "patchwork-plusplus_amd/python", ""):
    sys.path.insert(0, os.path.join(ROOT, p))
import numpy as np  # noqa: E402
import torch  # noqa: E402  (before libpwpp_hip: see tests/conftest.py)

import bench  # noqa: E402
import pwpp_hip  # noqa: E402

SETTINGS = [("default", False, False), ("point planes", True, False), ("planes + labels", True, True)]
COPY_ROOF_TBS = 4.94  # float4 -> float4 copy, grid 2048 (profiles/r06_copy_bw.txt)


def make(overlap):
    hs = []
    for _, planes, labels in SETTINGS:
        h = pwpp_hip.Handle()
        h.set_point_planes(planes)
        h.set_labels(labels)
        h.set_overlap(overlap)
        hs.append(h)
    return hs


def measure(hs, run, steps, warmup):
    t = [[] for _ in hs]
    for r in range(warmup + steps):
        for k, h in enumerate(hs):
            run(h)
            h.synchronize()
            if r >= warmup:
                t[k].append(h.time_us())
    return [np.asarray(x) for x in t]


def emit_slot(h, run):
    h.set_overlap(False)
    h.set_profiling(True)
    h.reset_kernel_profile()
    run(h)
    h.synchronize()
    prof = h.kernel_profile()
    h.set_profiling(False)
    total = sum(v[0] for v in prof.values())
    return prof["k_emit"][0] * 1e3, total * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "point_planes_cost.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    src, kind = bench.load_source_frames("kitti")
    F = a.frames
    ns = [src[i % len(src)].shape[0] for i in range(F)]
    offs = np.concatenate([[0], np.cumsum(ns)]).astype(np.int64)
    big = torch.empty((int(offs[-1]), 4), dtype=torch.float32, device=dev)
    sd = [torch.from_numpy(x).to(dev) for x in src]
    for i in range(F):
        big[offs[i]:offs[i + 1]].copy_(sd[i % len(src)])
    torch.cuda.synchronize()
    ptrs = [big.data_ptr() + int(offs[i]) * 16 for i in range(F)]
    lines = []

    def out(s=""):
        print(s)
        lines.append(s)

    out("point_planes_cost: %s, %d frames of %d points on average, %s" % (kind, F, int(offs[-1]) // F, torch.cuda.get_device_name(0)))
    out("GPU time per call (pwpp_get_time_us), median of %d after %d warm-up calls; + = over the default" % (a.steps, a.warmup))
    rows = []
    for name, overlap in (("1024-frame batch, overlap schedule", True), ("1024-frame batch, single-stream schedule", False)):
        hs = make(overlap)
        batches = [h.make_device_batch(ptrs, ns) for h in hs]
        run = lambda h, m={id(x): b for x, b in zip(hs, batches)}: h.launch_device_batch(m[id(h)], cols=4, mode=pwpp_hip.MODE_FRESH)
        rows.append((name, measure(hs, run, a.steps, a.warmup), hs, run, F))
    hs = make(True)
    one = src[0]
    run1 = lambda h: h.estimate_ground_batch([one], mode=pwpp_hip.MODE_FRESH)
    rows.append(("single fresh frame (%d points, host memory)" % one.shape[0], measure(hs, run1, 5 * a.steps, a.warmup), hs, run1, 1))
    for name, t, hs, run, frames in rows:
        out("\n%s" % name)
        base = float(np.median(t[0]))
        q1, q3 = np.percentile(t[0], [25, 75])
        for k, ((sname, _, _), v) in enumerate(zip(SETTINGS, t)):
            med = float(np.median(v))
            extra = "  spread of the default's %d calls: %.1f .. %.1f us, half IQR %.1f us" % (len(v), v.min(), v.max(), (q3 - q1) / 2) if k == 0 \
                else "  %+8.1f us  %+6.1f %%" % (med - base, 100.0 * (med - base) / base)
            out("  %-16s %10.1f us%s" % (sname, med, extra))
        # what the new kernels move: every slot of the launch filled (8 B), every point of a patch read (16 B) and written (8 B)
        pats, _ = hs[1].all_point_patches()
        n_all, n_in = len(pats), int((pats >= 0).sum())
        nbytes = 8 * n_all + 24 * n_in
        out("  k_emit slot of one profiled call (single-stream schedule; it also holds the new kernels, and the label kernels):")
        slots = []
        for (sname, _, _), h in zip(SETTINGS, hs):
            e, tot = emit_slot(h, run)
            slots.append(e)
            out("    %-16s k_emit %8.1f us of %8.1f us profiled" % (sname, e, tot))
        dt = slots[1] - slots[0]
        out("  new kernels (k_emit slot, point planes - default): %.1f us for %.1f MB (%d points, %d in patches): %s"
            % (dt, nbytes / 1e6, n_all, n_in, "%.2f TB/s = %.0f %% of the %.2f TB/s copy roof" % (nbytes / dt / 1e6, 100 * nbytes / dt / 1e6 / COPY_ROOF_TBS, COPY_ROOF_TBS)
               if dt > 0 else "below the resolution of one profiled call"))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
