#!/usr/bin/env python3
"""The cases of tests/test_gpu_one_pass_arena.py as a table (CPU only, no library): per planned frame the case, its position in the
test batch, the limit it stands at and on which side, its points, the parts whose counts differ from the sizing frame's (count /
capacity under the table the test batch meets), overgrown parts, spilled records and arena run against their three limits, the outcome
the restatement of tests/one_pass_arena_ref.py predicts, and what the batch adds to arena_stats / redo_stats / one_pass_stats.

    python tools/one_pass_arena_table.py > profiles/one_pass_arena_cases.txt
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "patchwork-plusplus_amd", "python"))

import one_pass_arena_ref as ar  # noqa: E402
import oracle_lib as ol  # noqa: E402


def main():
    p = ol.restatement().default_params()  # (the parameter block alone is read: CZM, RNR rule, sensor height)
    print("# case / frame / limit / side / points / parts that differ from the sizing frame: count/capacity / overgrown parts, spilled records, "
          "arena run: value/limit / predicted outcome | what the batch adds to the statistics")
    for case in ar.CASES:
        b = case.built(p)
        print("# %-22s %2d frames, one_pass_scale %g, debug_flags %d: sizing frame of %d points; slots per frame %d -> %d, arena %d -> %d (records %d)"
              % (case.name, case.frames, case.scale, case.debug, case.base.n(), b.sizing_table.slots_per_frame, b.test_table.slots_per_frame,
                 b.sizing_table.arena_slots, b.test_table.arena_slots, b.test_table.arena_spill))
    for row in ar.rows_of_table(p):
        print(row)


if __name__ == "__main__":
    main()
