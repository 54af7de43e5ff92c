"""What per-point labels and the cloud-order lists cost on one MI355X (profiles/labels_cost.txt).

Four settings -- default (scatter order), labels only, cloud order, reference order -- on
  * 1024 replayed KITTI frames from device memory, overlap schedule (bench.py's configs[2] shape),
  * the same batch on the single-stream schedule,
  * one fresh KITTI frame from host memory (the latency path).
GPU time of a call = pwpp_get_time_us (first kernel -> lists written; labels included): median of `steps` calls after
`warmup`, settings interleaved round by round so that clock drift hits all four alike.  Then one profiled call per
setting on the single-stream schedule: the k_emit slot, which holds the label kernels.

    python tools/labels_cost.py [--steps 20] [--warmup 5]
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

SETTINGS = [("default", False, pwpp_hip.ORDER_SCATTER), ("labels", True, pwpp_hip.ORDER_SCATTER),
            ("cloud order", False, pwpp_hip.ORDER_CLOUD), ("reference order", False, pwpp_hip.ORDER_REFERENCE)]


def make(overlap):
    hs = []
    for _, labels, order in SETTINGS:
        h = pwpp_hip.Handle()
        h.set_labels(labels)
        h.set_order(order)
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
    return [float(np.median(x)) for x in t]


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
    print("labels_cost: %s, %d frames of %d points on average, %s" % (kind, F, int(offs[-1]) // F, torch.cuda.get_device_name(0)))
    print("GPU time per call (pwpp_get_time_us), median of %d after %d warm-up calls; + = over the default" % (a.steps, a.warmup))
    rows = []
    for name, overlap in (("1024-frame batch, overlap schedule", True), ("1024-frame batch, single-stream schedule", False)):
        hs = make(overlap)
        batches = [h.make_device_batch(ptrs, ns) for h in hs]
        run = lambda h, m={id(x): b for x, b in zip(hs, batches)}: h.launch_device_batch(m[id(h)], cols=4, mode=pwpp_hip.MODE_FRESH)
        rows.append((name, measure(hs, run, a.steps, a.warmup), "us", hs, run))
    hs = make(True)
    one = src[0]
    run1 = lambda h: h.estimate_ground_batch([one], mode=pwpp_hip.MODE_FRESH)
    rows.append(("single fresh frame (%d points, host memory)" % one.shape[0], measure(hs, run1, 5 * a.steps, a.warmup), "us", hs, run1))
    for name, t, unit, hs, run in rows:
        print("\n%s" % name)
        base = t[0]
        for k, ((sname, _, _), v) in enumerate(zip(SETTINGS, t)):
            extra = "" if k == 0 else "  %+8.1f us  %+6.1f %%" % (v - base, 100.0 * (v - base) / base)
            print("  %-16s %10.1f %s%s" % (sname, v, unit, extra))
        print("  k_emit slot of one profiled call (single-stream schedule; with labels on it also holds the label kernels):")
        for (sname, _, _), h in zip(SETTINGS, hs):
            e, tot = emit_slot(h, run)
            print("    %-16s k_emit %8.1f us of %8.1f us profiled" % (sname, e, tot))


if __name__ == "__main__":
    main()
