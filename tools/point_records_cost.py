"""What the point records (pwpp_set_point_records) cost on one MI355X (profiles/point_records_cost.txt).

  * Records off / on, interleaved round by round on the same build: one fresh KITTI frame from host memory (the latency path)
    and 1024 replayed KITTI frames from device memory (bench.py's configs[2] shape), as 16-byte matrix rows (row4) and as a
    32-byte fields layout.  GPU time of a call = pwpp_get_time_us, median of `steps` calls after `warmup`.
  * The gather paths against each other at 32 and 48 bytes per record: the kernel's choice (16-byte pieces), the dword stream
    (option records_path = 2) and a plain one-lane-per-row copy (records_path = 1), same batch, interleaved.
  * What the records add is set against the bytes they must move -- 4 (index) + 2 x record_bytes per listed point -- and the
    copy roof profiles/point_planes_cost.txt used.
  * --parent-lib PATH: the off figures of this build against a build of the parent commit, each in fresh child processes that
    alternate (parent, this, parent, this); the parent's own range over its runs is the yardstick.

    python tools/point_records_cost.py [--steps 20] [--warmup 5] [--parent-lib /path/to/parent/libpwpp_hip.so]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("tests", "patchwork-plusplus_amd/python", ""):
    sys.path.insert(0, os.path.join(ROOT, p))
import numpy as np  # noqa: E402
import torch  # noqa: E402  (before libpwpp_hip: see tests/conftest.py)

import bench  # noqa: E402
import pwpp_hip  # noqa: E402

COPY_ROOF_TBS = 4.94  # float4 -> float4 copy, grid 2048 (profiles/r06_copy_bw.txt)
# name: (point_step, (off_x, off_y, off_z, off_intensity)); None = an (n, 4) row-major matrix
LAYOUTS = {"row4": None, "fields32": (32, (4, 12, 20, 0)), "fields48": (48, (8, 0, 16, 4))}


def device_batch(src, frames, layout):
    """`frames` replayed source frames back to back in one device tensor: (tensor, addresses, point counts, record bytes)."""
    dev = torch.device("cuda", 0)
    spec = LAYOUTS[layout]
    step = 16 if spec is None else spec[0]
    enc = []
    for x in src:
        if spec is None:
            enc.append(torch.from_numpy(np.ascontiguousarray(x)).view(torch.uint8).reshape(-1, 16).to(dev))
        else:
            blob = np.random.default_rng(1).integers(0, 256, (x.shape[0], step), dtype=np.uint8)
            for k, o in enumerate(spec[1]):
                blob[:, o:o + 4] = np.ascontiguousarray(x[:, k]).view(np.uint8).reshape(-1, 4)
            enc.append(torch.from_numpy(blob).to(dev))
    ns = [src[i % len(src)].shape[0] for i in range(frames)]
    offs = np.concatenate([[0], np.cumsum(ns)]).astype(np.int64)
    big = torch.empty((int(offs[-1]), step), dtype=torch.uint8, device=dev)
    for i in range(frames):
        big[offs[i]:offs[i + 1]].copy_(enc[i % len(src)])
    torch.cuda.synchronize()
    return big, [big.data_ptr() + int(offs[i]) * step for i in range(frames)], ns, step


def runner(layout, ptrs, ns):
    spec = LAYOUTS[layout]
    if spec is None:
        return lambda h: h.submit_batch(ptrs, ns, 4, pwpp_hip.LAYOUT_ROW_MAJOR, pwpp_hip.MEM_DEVICE, pwpp_hip.MODE_FRESH)
    return lambda h: h.estimate_ground_fields_batch(ptrs, ns, spec[0], *spec[1], mem=pwpp_hip.MEM_DEVICE, mode=pwpp_hip.MODE_FRESH)


def measure(hs, run, steps, warmup):
    t = [[] for _ in hs]
    for r in range(warmup + steps):
        for k, h in enumerate(hs):
            run(h)
            h.synchronize()
            if r >= warmup:
                t[k].append(h.time_us())
    return [np.asarray(x) for x in t]


def handles(settings):
    hs = []
    for on, path in settings:
        h = pwpp_hip.Handle()
        if on:
            h.set_point_records(True)
            h.set_option("records_path", path)
        hs.append(h)
    return hs


def child_off(a):
    """The default setting only (this runs against whichever library PWPP_LIB_PATH names): one JSON line."""
    src, _ = bench.load_source_frames("kitti")
    h1, hb = pwpp_hip.Handle(), pwpp_hip.Handle()
    one = src[0]
    t1 = measure([h1], lambda h: h.estimate_ground_batch([one], mode=pwpp_hip.MODE_FRESH), 5 * a.steps, a.warmup)[0]
    big, ptrs, ns, _ = device_batch(src, a.frames, "row4")
    tb = measure([hb], runner("row4", ptrs, ns), a.steps, a.warmup)[0]
    print("CHILD " + json.dumps({"single": t1.tolist(), "batch": tb.tolist()}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--child-off", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "point_records_cost.txt"))
    a = ap.parse_args()
    if a.child_off:
        return child_off(a)
    lines = []

    def out(s=""):
        print(s, flush=True)
        lines.append(s)

    # ---- the off path against the parent commit: fresh child processes, alternating, before this process opens the GPU
    if a.parent_lib:
        runs = {"parent": [], "this": []}
        for who in ("parent", "this", "parent", "this"):
            env = dict(os.environ)
            if who == "parent":
                env["PWPP_LIB_PATH"] = os.path.abspath(a.parent_lib)
            else:
                env.pop("PWPP_LIB_PATH", None)
            cp = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-off", "--steps", str(a.steps), "--warmup", str(a.warmup),
                                 "--frames", str(a.frames)], env=env, capture_output=True, text=True, timeout=400, check=True)
            runs[who].append(json.loads([l for l in cp.stdout.splitlines() if l.startswith("CHILD ")][0][6:]))
    src, kind = bench.load_source_frames("kitti")
    out("point_records_cost: %s, %d frames, %s" % (kind, a.frames, torch.cuda.get_device_name(0)))
    out("GPU time per call (pwpp_get_time_us), median of %d (single frame: %d) after %d warm-up calls" % (a.steps, 5 * a.steps, a.warmup))
    if a.parent_lib:
        out("\nrecords off: this build against a build of the parent commit (two fresh processes each, alternating)")
        for key, label in (("single", "single fresh frame, host memory"), ("batch", "%d-frame batch, device memory, row4" % a.frames)):
            pm = [float(np.median(r[key])) for r in runs["parent"]]
            tm = [float(np.median(r[key])) for r in runs["this"]]
            pall = np.concatenate([np.asarray(r[key]) for r in runs["parent"]])
            lo, hi = float(pall.min()), float(pall.max())
            inside = all(lo <= m <= hi for m in tm)
            out("  %-44s parent medians %s us, its calls %.1f .. %.1f us; this build %s us: %s"
                % (label, " / ".join("%.1f" % m for m in pm), lo, hi, " / ".join("%.1f" % m for m in tm),
                   "inside the parent's range" if inside else "OUTSIDE the parent's range"))

    def report(name, t, labels, listed, rb):
        out("\n%s" % name)
        base = float(np.median(t[0]))
        q1, q3 = np.percentile(t[0], [25, 75])
        nbytes = (4 + 2 * rb) * listed
        for k, (label, v) in enumerate(zip(labels, t)):
            med = float(np.median(v))
            if k == 0:
                out("  %-34s %10.1f us  spread of its %d calls: %.1f .. %.1f us, half IQR %.1f us" % (label, med, len(v), v.min(), v.max(), (q3 - q1) / 2))
            else:
                d = med - base
                rate = "%.2f TB/s = %.0f %% of the %.2f TB/s copy roof" % (nbytes / d / 1e6, 100 * nbytes / d / 1e6 / COPY_ROOF_TBS, COPY_ROOF_TBS) if d > 0 else "below the resolution"
                out("  %-34s %10.1f us  %+8.1f us  %+6.1f %%   %.1f MB for %d listed points: %s" % (label, med, d, 100 * d / base, nbytes / 1e6, listed, rate))

    def listed_points(h):
        c = h.all_counts()
        return int(c[:, 0].sum() + c[:, 1].sum())

    # ---- single frame, host memory
    one = src[0]
    hs = handles([(False, 0), (True, 0)])
    t = measure(hs, lambda h: h.estimate_ground_batch([one], mode=pwpp_hip.MODE_FRESH), 5 * a.steps, a.warmup)
    report("single fresh frame (%d points, host memory), row4: 16-byte records" % one.shape[0], t, ["records off", "records on"], listed_points(hs[1]), 16)
    blob = np.random.default_rng(1).integers(0, 256, (one.shape[0], 32), dtype=np.uint8)
    for k, o in enumerate(LAYOUTS["fields32"][1]):
        blob[:, o:o + 4] = np.ascontiguousarray(one[:, k]).view(np.uint8).reshape(-1, 4)
    flat = blob.ravel()
    hs = handles([(False, 0), (True, 0)])
    t = measure(hs, lambda h: h.estimate_ground_fields_batch([flat], [one.shape[0]], 32, *LAYOUTS["fields32"][1], mem=pwpp_hip.MEM_HOST,
                                                             mode=pwpp_hip.MODE_FRESH), 5 * a.steps, a.warmup)
    report("single fresh frame, fields layout: 32-byte records", t, ["records off", "records on"], listed_points(hs[1]), 32)
    for h in hs:
        h.close()
    # ---- the batch: off / on, and the paths against each other
    for layout, settings, labels in (
            ("row4", [(False, 0), (True, 0), (True, 1)], ["records off", "records on (16 B per lane)", "records on, plain lane per row"]),
            ("fields32", [(False, 0), (True, 0), (True, 2), (True, 1)],
             ["records off", "records on (16-byte pieces)", "records on, dword stream", "records on, plain lane per row"]),
            ("fields48", [(False, 0), (True, 0), (True, 2), (True, 1)],
             ["records off", "records on (16-byte pieces)", "records on, dword stream", "records on, plain lane per row"])):
        big, ptrs, ns, rb = device_batch(src, a.frames, layout)
        hs = handles(settings)
        t = measure(hs, runner(layout, ptrs, ns), a.steps, a.warmup)
        report("%d-frame batch (device memory, overlap schedule), %s: %d-byte records" % (a.frames, layout, rb), t, labels, listed_points(hs[1]), rb)
        for h in hs:
            h.close()
        del big
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
