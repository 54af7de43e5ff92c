#!/usr/bin/env python3
"""The cases of tests/test_gpu_fit_limits.py as a table (CPU only): per frame its size, the grid, how far the quantised
coordinates reach into the contract's range (max |Q| / 2^35, or / 2^26 on the narrow grid) and the most points one lane adds
up under the dealing rule of pwpp_fit.hip (one stored part / both parts half full).  A frame beyond its plan's entry goes to
k_fit_stream, whose lanes sum in 128 bits.

    python tools/fit_limits_table.py > profiles/fit_limits_cases.txt
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "patchwork-plusplus_amd", "python"))

import fit_limits_ref as fl  # noqa: E402
import oracle_lib as ol  # noqa: E402
import test_gpu_fit_limits as t  # noqa: E402


def row(test, plan, geometry, wide, az, zl, n):
    lib = ol.restatement()
    est = ol.Estimator(lib, fl.configure(lib.default_params(), geometry), arith=ol.ARITH_FXP if wide else ol.ARITH_FXP21)
    shift, _, ox, oy = est.fxp_geometry()
    b = fl.GEOMETRIES[geometry]["bin"]
    pts = fl.cloud(geometry, az, zl, n)
    a = fl.Anchor(pts, shift, wide, (ox[b], oy[b]), fl.z_origin(pts))
    lanes = "128-bit lane sums"
    entry = plan.split(",")[0] if plan else "S64:65535"  # (the launcher's plan for these twelve frames)
    if entry != "S8:0" and n <= fl.effective_edge(entry):
        mode, g, _, upper = fl.plan_entry(entry)
        if mode == "H" and n <= upper:
            mode = "S"  # one wave per patch below the entry's bound
        lanes = "%d / %d" % (fl.max_lane_points(mode, g, (n, 0)), fl.max_lane_points(mode, g, (n // 2, n - n // 2)))
    print("%-22s %-13s %s %-6s %-5s %8d  %-6s  %.4f %.4f %.4f  %3d  %s"
          % (test, plan or "(launcher)", geometry, az, zl, n, "wide" if wide else "narrow", a.reach[0], a.reach[1], a.reach[2], a.numerator_bits, lanes))


def main():
    print("# test / plan / geometry, azimuth, zlow / points / grid / reach x y z / bits of the largest covariance numerator / "
          "most points per lane (one part / two halves)")
    for wide in (True, False):
        for plans, name in ((t.W16_PLANS, "sixteen_lane_rows"), (t.S_PLANS, "streaming_rows"), (t.W64_PLANS, "big_bins_per_wave")):
            for plan in plans:
                geometry, frames = t.edge_pair(t.ROTATION[plans.index(plan)], fl.effective_edge(plan))
                for az, zl, n in frames:
                    row(name, plan, geometry, wide, az, zl, n)
        for plan in t.BIG_PLANS:
            geometry, frames = t.big_frames(plan)
            for az, zl, n in frames:
                row("four_waves_per_patch", plan, geometry, wide, az, zl, n)
        if not wide:
            for plan in t.S_PLANS:
                geometry, frames = t.edge_pair(t.ROTATION[(t.S_PLANS.index(plan) + 1) % 4], 2047)
                for az, zl, n in frames + [(frames[0][0], "clamp", 2049)]:
                    row("row_sum_switch", plan, geometry, wide, az, zl, n)
        for az, zl, n in t.mixed_frames(wide):
            row("launchers_own_plan", "", "A", wide, az, zl, n)
    row("workgroup_kernel_alone", "S8:0", "A", True, "x-", "reach", fl.MAX_POINTS)


if __name__ == "__main__":
    main()
