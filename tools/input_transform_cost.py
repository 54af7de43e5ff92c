"""What the input transform (pwpp_set_input_transforms) costs on one MI355X (profiles/input_transform_cost.txt).

For a 1024-frame KITTI batch in device memory (bench.py's flagship shape) and for one fresh frame from host memory:
  (a) transforms off;
  (b) transforms on (one tilt for every frame): the kernels transform where they read the input;
  (c) transforms off, preceded by a separate pass that writes a transformed copy of the batch -- one torch.addmm over the
      (n, 4) batch (x' = r . p + t per row, 16 B read and 16 B written per point), timed with events around it.  The yardstick that
      justifies fusing.
The three are interleaved round by round; GPU time of a call = pwpp_get_time_us, (c) adds the copy's event time.  Medians, the
spread of the calls and the half inter-quartile range are written out.

    python tools/input_transform_cost.py [--steps 20] [--warmup 5] [--frames 1024]
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
import input_transform_ref as xf  # noqa: E402
import pwpp_hip  # noqa: E402

TILT = xf.rigid(np.radians(3.0), np.radians(-5.0), np.radians(20.0), t=(0.2, -0.1, 0.15))


def copy_pass(src, dst, M, t):
    """dst = src @ M + t over the whole (n, 4) batch in ONE launch: M = [[R^T, 0], [0, 1]], t = (t0, t1, t2, 0) -- the separate
    transformed copy a caller writes today (the intensity times one plus zero is itself)."""
    torch.addmm(t, src, M, out=dst)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "input_transform_cost.txt"))
    a = ap.parse_args()
    lines = []

    def out(s=""):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda", 0)
    src, kind = bench.load_source_frames("kitti")
    sensor = [xf.transform_cloud(xf.inverse(TILT), c) for c in src]  # un-levelled: TILT levels them again
    m4 = np.eye(4, dtype=np.float32)
    m4[:3, :3] = TILT[:, :3].T
    Rt = torch.from_numpy(m4).to(dev)
    tt = torch.from_numpy(np.append(TILT[:, 3], np.float32(0)).astype(np.float32)).to(dev)
    out("input_transform_cost: %s, %s" % (kind, torch.cuda.get_device_name(0)))
    out("GPU time per call (pwpp_get_time_us; (c) adds the event time of its copy pass), interleaved round by round")

    def report(title, t, steps):
        out("\n%s" % title)
        base = float(np.median(t[0]))
        for label, v in zip(("(a) transforms off", "(b) transforms on", "(c) off + separate transformed copy"), t):
            v = np.asarray(v)
            q1, q3 = np.percentile(v, [25, 75])
            out("  %-38s %9.1f us  %+8.1f us  spread of its %d calls %.1f .. %.1f us, half IQR %.1f us"
                % (label, np.median(v), np.median(v) - base, steps, v.min(), v.max(), (q3 - q1) / 2))
        out("  (b) - (a) = %+.1f us     (c) - (a) = %+.1f us" % (np.median(t[1]) - base, np.median(t[2]) - base))

    def measure(run_a, run_b, run_c, steps):
        t = [[], [], []]
        for r in range(a.warmup + steps):
            for k, run in enumerate((run_a, run_b, run_c)):
                v = run()
                if r >= a.warmup:
                    t[k].append(v)
        return t

    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    # ---- the batch: device memory, the overlap schedule
    ns = [sensor[i % len(sensor)].shape[0] for i in range(a.frames)]
    offs = np.concatenate([[0], np.cumsum(ns)]).astype(np.int64)
    big = torch.empty((int(offs[-1]), 4), dtype=torch.float32, device=dev)
    for i in range(a.frames):
        big[offs[i]:offs[i + 1]].copy_(torch.from_numpy(sensor[i % len(sensor)]))
    levelled = torch.empty_like(big)
    copy_pass(big, levelled, Rt, tt)
    torch.cuda.synchronize()
    ha, hb, hc = pwpp_hip.Handle(), pwpp_hip.Handle(), pwpp_hip.Handle()
    hb.set_input_transforms(TILT)
    raw = hb.make_device_batch([big.data_ptr() + int(o) * 16 for o in offs[:-1]], ns)
    lev = ha.make_device_batch([levelled.data_ptr() + int(o) * 16 for o in offs[:-1]], ns)

    def call(h, batch):
        h.launch_device_batch(batch)
        h.synchronize()
        return h.time_us()

    def with_copy():
        ev0.record()
        copy_pass(big, levelled, Rt, tt)
        ev1.record()
        torch.cuda.synchronize()
        return ev0.elapsed_time(ev1) * 1000.0 + call(hc, lev)

    t = measure(lambda: call(ha, lev), lambda: call(hb, raw), with_copy, a.steps)
    report("%d-frame batch (%d points, device memory, row-major 4 columns)" % (a.frames, int(offs[-1])), t, a.steps)
    for h in (ha, hb, hc):
        h.close()
    del big, levelled
    torch.cuda.empty_cache()

    # ---- one fresh frame from host memory (the latency path)
    one = sensor[0]
    one_dev = torch.from_numpy(one).to(dev)
    one_lev = torch.empty_like(one_dev)
    copy_pass(one_dev, one_lev, Rt, tt)
    torch.cuda.synchronize()
    lev_host = one_lev.cpu().numpy()
    ha, hb, hc = pwpp_hip.Handle(), pwpp_hip.Handle(), pwpp_hip.Handle()
    hb.set_input_transforms(TILT)

    def one_call(h, c):
        h.estimate_ground_batch([c], mode=pwpp_hip.MODE_FRESH)
        return h.time_us()

    def one_with_copy():
        ev0.record()
        copy_pass(one_dev, one_lev, Rt, tt)
        ev1.record()
        torch.cuda.synchronize()
        return ev0.elapsed_time(ev1) * 1000.0 + one_call(hc, lev_host)

    t = measure(lambda: one_call(ha, lev_host), lambda: one_call(hb, one), one_with_copy, 5 * a.steps)
    report("single fresh frame (%d points, host memory)" % one.shape[0], t, 5 * a.steps)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
