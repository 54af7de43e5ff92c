#!/usr/bin/env python3
"""The cases of tests/test_gpu_list_order.py as a table (CPU only): per case the part under test as the oracle reports it -- list,
length, categories, distinct heights (-0 taken as +0) -- the fullest bucket of the distribution sort, the path K7 takes by the
restated rule of tests/list_order_ref.py (sort_path), and for lists above one tile the tiles and merge passes.

    python tools/list_order_table.py > profiles/list_order_cases.txt
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "patchwork-plusplus_amd", "python"))

import list_order_ref as lo  # noqa: E402
import oracle_lib as ol  # noqa: E402


def main():
    lib = ol.restatement()
    print("# case / list / part length / categories (cloud: a part in cloud order) / distinct heights / fullest bucket / path "
          "(network: keys it sorts) / tiles / merge passes")
    for case in lo.CASES:
        p = lo.configured(lib.default_params(), case.variant)
        pts, chosen = case.cloud(p)
        d = lo.describe(case, pts, chosen, ol.Estimator(lib, p, arith=ol.ARITH_FXP).run(pts))
        cats = "cloud" if d["cloud_order"] else ",".join(str(c) for c in d["categories"])
        path = d["path"] + (" (%d)" % d["network"] if d["network"] else "")
        print("%-26s %-9s %6d  %-6s %6d  %-4s %-27s %2d %2d"
              % (d["case"], d["list"], d["length"], cats, d["heights"], "-" if d["fullest"] is None else d["fullest"], path, d["tiles"], d["passes"]))


if __name__ == "__main__":
    main()
