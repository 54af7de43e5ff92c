"""What the ground queries (pwpp_query_ground, pwpp_rasterize_ground) cost on one MI355X (profiles/ground_query_cost.txt).

  * The raster of `frames` replayed KITTI frames at 256 x 256 cells of 0.5 m, height image alone and with the patch image, with
    the fast bin path and with exact binning only (option debug_flags = 16), device memory.
  * A query list of `frames` x 1024 positions (uniform in [-90, 90]^2, frame ids in order), device memory.
  * The yardstick of each: a hipMemsetAsync of the same output bytes.
  Every figure is the median over `steps` rounds; a round runs each variant once, in turn (interleaved).  One measurement = `reps`
  calls enqueued back to back and one synchronise, timed with the host clock and divided by `reps`: the handle's stream is its
  own, so no HIP event of this tool can bracket work on it.  The ratios are reported, nothing is gated on them.

    python tools/ground_query_cost.py [--frames 1024] [--steps 9] [--warmup 2] [--reps 8]
"""
import argparse
import ctypes
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


def hip_runtime():
    """The HIP runtime this process already uses, for the memset yardstick."""
    with open("/proc/self/maps") as f:
        paths = sorted({ln.split()[-1] for ln in f if "libamdhip64.so" in ln})
    lib = ctypes.CDLL(paths[0])
    lib.hipMemsetAsync.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
    lib.hipDeviceSynchronize.argtypes = []
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ground_query_cost.txt"))
    a = ap.parse_args()
    lines = []

    def out(s=""):
        print(s, flush=True)
        lines.append(s)

    hip = hip_runtime()
    src, kind = bench.load_source_frames("kitti")
    F, NX, NY, CELL, M = a.frames, 256, 256, 0.5, 1024
    big, ptrs, ns, _ = device_batch(src, F, "row4")
    h = pwpp_hip.Handle()
    h.submit_batch(ptrs, ns, 4, pwpp_hip.LAYOUT_ROW_MAJOR, pwpp_hip.MEM_DEVICE, pwpp_hip.MODE_FRESH)
    h.synchronize()
    cells = F * NY * NX
    d_h = torch.empty(cells, dtype=torch.float32, device="cuda")
    d_p = torch.empty(cells, dtype=torch.int32, device="cuda")
    rng = np.random.default_rng(3)
    xyz = rng.uniform(-90.0, 90.0, (F * M, 3)).astype(np.float32)
    d_xyz = torch.from_numpy(xyz).to("cuda")
    d_fr = torch.from_numpy(np.repeat(np.arange(F, dtype=np.int32), M)).to("cuda")
    d_out = torch.empty(4 * F * M, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    x0 = y0 = -0.5 * NX * CELL

    def timed(enqueue, sync):
        t0 = time.perf_counter()
        for _ in range(a.reps):
            enqueue()
        sync()
        return (time.perf_counter() - t0) * 1e6 / a.reps

    def raster(flags, with_patch):
        def run():
            h.set_option("debug_flags", flags)
            return timed(lambda: h.rasterize_ground_device(x0, y0, CELL, NX, NY, d_h.data_ptr(), d_p.data_ptr() if with_patch else 0, 0, F),
                         h.synchronize)
        return run

    def memset(ptr, nbytes):
        return lambda: timed(lambda: hip.hipMemsetAsync(ptr, 0, nbytes, None), hip.hipDeviceSynchronize)

    variants = [
        ("raster, height only, fast bins", raster(0, False)),
        ("raster, height only, exact bins (debug_flags 16)", raster(16, False)),
        ("hipMemsetAsync of the height image", memset(d_h.data_ptr(), 4 * cells)),
        ("raster, height + patch, fast bins", raster(0, True)),
        ("raster, height + patch, exact bins (debug_flags 16)", raster(16, True)),
        ("hipMemsetAsync of both images", lambda: timed(lambda: (hip.hipMemsetAsync(d_h.data_ptr(), 0, 4 * cells, None),
                                                                    hip.hipMemsetAsync(d_p.data_ptr(), 0, 4 * cells, None)), hip.hipDeviceSynchronize)),
        ("query list", lambda: (h.set_option("debug_flags", 0),
                                timed(lambda: h.query_ground_device(d_xyz.data_ptr(), d_fr.data_ptr(), F * M, d_out.data_ptr()), h.synchronize))[1]),
        ("hipMemsetAsync of the samples", memset(d_out.data_ptr(), 16 * F * M)),
    ]
    t = [[] for _ in variants]
    for r in range(a.warmup + a.steps):
        for k, (_, run) in enumerate(variants):
            v = run()
            if r >= a.warmup:
                t[k].append(v)
    h.set_option("debug_flags", 0)
    med = [float(np.median(x)) for x in t]
    out("ground_query_cost: %s, %d frames, %s" % (kind, F, torch.cuda.get_device_name(0)))
    out("us per call: host clock over %d calls enqueued back to back + one synchronise; median / min .. max of %d interleaved rounds after %d warm-up rounds"
        % (a.reps, a.steps, a.warmup))
    out("raster: %d frames x %d x %d cells of %.1f m = %.1f MB per image; query list: %d frames x %d positions = %.1f MB of samples"
        % (F, NY, NX, CELL, 4 * cells / 1e6, F, M, 16 * F * M / 1e6))
    out()
    for (name, _), m, x in zip(variants, med, t):
        out("  %-52s %10.1f us   %10.1f .. %10.1f" % (name, m, min(x), max(x)))
    out()
    out("ratios to the memset of the same output bytes (reported, not gated):")
    out("  raster, height only, fast bins   %.2f x" % (med[0] / med[2]))
    out("  raster, height + patch, fast bins %.2f x" % (med[3] / med[5]))
    out("  query list                        %.2f x" % (med[6] / med[7]))
    out()
    for label, fast, exact in (("height only", 0, 1), ("height + patch", 3, 4)):
        lo, hi = min(t[exact]), max(t[exact])
        clear = max(t[fast]) < lo
        out("fast against exact bins, %s: %.1f against %.1f us (%.2f x); the exact path's rounds span %.1f .. %.1f us, the fast path's %.1f .. %.1f us: %s"
            % (label, med[fast], med[exact], med[exact] / med[fast], lo, hi, min(t[fast]), max(t[fast]),
               "the fast path is clearly outside the exact path's range" if clear else "NOT clearly outside the exact path's range"))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    del big


if __name__ == "__main__":
    main()
