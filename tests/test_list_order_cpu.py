"""list_order_ref.py on the CPU: every built cloud has the part it aims for, the cases together reach every regime of K7
(k_order_sublists) by the restated path rule, and `expected_lists` takes no freedom but the order among equal heights."""
import numpy as np
import pytest

import list_order_ref as lo
import oracle_lib as ol
import pwpp_synth
from conftest import load_kitti


@pytest.fixture(scope="module")
def oracle(oracle_built):
    return oracle_built.restatement()


def run_case(oracle, case):
    p = lo.configured(oracle.default_params(), case.variant)
    pts, chosen = case.cloud(p)
    return pts, chosen, ol.Estimator(oracle, p, arith=ol.ARITH_FXP).run(pts)


@pytest.fixture(scope="module")
def rows(oracle):
    out = {}
    for case in lo.CASES:
        pts, chosen, res = run_case(oracle, case)
        out[case.name] = lo.describe(case, pts, chosen, res)
    return out


@pytest.mark.parametrize("case", lo.CASES, ids=repr)
def test_case_has_the_part_it_aims_for(oracle, case):
    pts, chosen, res = run_case(oracle, case)
    assert len(chosen) == case.length
    which, ordinal, at = lo.part_under_test(res, chosen)  # (asserts: the part is the chosen points and nothing else)
    assert (which, len(at)) == (case.which, case.length)
    assert len(res.ground_idx) + len(res.nonground_idx) == len(pts)
    g, n = lo.expected_lists(pts, res)
    assert np.array_equal(np.sort(g), np.sort(res.ground_idx)) and np.array_equal(np.sort(n), np.sort(res.nonground_idx))


def test_cases_reach_every_regime(rows):
    r = list(rows.values())
    paths = {d["path"] for d in r}
    for want in ("wave", "bucket", "network:categories", "network:non-finite", "network:one height", "network:scale", "network:skew",
                 "network:above 4032", "tiles"):
        assert want in paths, want
    assert {512, 1024, 2048, 4096} <= {d["network"] for d in r}
    assert {0, 1, 2, 3, 4} <= {d["passes"] for d in r}
    by_length = lambda which, cloud: {d["length"] for d in r if d["list"] == which and d["cloud_order"] == cloud}
    for n in (256, 257, 4032, 4033, 4096, 4097):  # each edge as a ground part and as a non-ground part of category 255
        assert n in by_length("ground", False) and n in by_length("nonground", False), n
    for n in (1, 2, 63, 64, 65, 128, 129, 255, 256, 257, 512, 513, 4031, 4032, 4033, 4095, 4096, 4097, 8192, 8193, 12289, 16385):
        assert n in by_length("ground", False) | by_length("nonground", False), n
    assert {9, 256, 257, 4096, 4097, 8193, 20000} <= by_length("nonground", True)
    # the named decline cases take the path they are there for
    for name, path in (("one-height-300", "network:one height"), ("ties-16x32", "bucket"), ("ties-16x32-and-one-of-33", "network:skew"),
                       ("two-categories-1100", "network:categories"), ("one-ulp-apart-600", "bucket"), ("range-overflows-2100", "network:scale"),
                       ("plus-infinity-4000", "network:non-finite"), ("zeros-column-200", "wave"), ("zeros-column-700", "bucket"),
                       ("zeros-column-1000", "network:skew"), ("zeros-column-5000", "tiles")):
        assert rows[name]["path"] == path, (name, rows[name])
    assert rows["ties-16x32"]["fullest"] == 32 and rows["ties-16x32-and-one-of-33"]["fullest"] == 33
    assert rows["two-categories-1100"]["categories"] == [1, 255]
    # 8193 and 12289: a last run of one key; 4097: one pass, the result lies in the second scratch array
    assert rows["spread-ground-8193"]["passes"] == 2 and rows["spread-column-12289"]["passes"] == 2 and rows["spread-ground-4097"]["passes"] == 1


def test_signed_zero_cases_interleave_both_zeros(oracle):
    for case in lo.CASES:
        if not case.name.startswith("zeros-"):
            continue
        pts, chosen, _ = run_case(oracle, case)
        z = pts[chosen, 2]
        zero = np.nonzero(z == 0.0)[0]
        sign = np.signbit(z[zero])
        assert len(zero) >= 24 and sign[0::2].sum() == 0 and sign[1::2].all()  # +0, -0, +0 ... in cloud index
        assert (z != 0.0).sum() > len(zero)


def differs_only_inside_ties(z, mine, theirs, part, cat):
    d = np.nonzero(mine != theirs)[0]
    if not len(d):
        return True
    # a run = consecutive positions of one (part, category) with equal z; every differing position lies in a run longer than one
    key_same = (part[1:] == part[:-1]) & (cat[1:] == cat[:-1]) & (z[theirs][1:] == z[theirs][:-1])
    start = np.concatenate([[0], np.cumsum(~key_same)])
    size = np.bincount(start)
    return bool((size[start[d]] > 1).all()) and np.array_equal(z[mine], z[theirs])


def test_expected_lists_on_scans(oracle):
    syn = pwpp_synth.add_edge_cases(pwpp_synth.make_cloud(7, beams=48, azimuth_steps=1500), 7)
    for pts in [load_kitti(k) for k in range(6)] + [syn]:
        res = ol.Estimator(oracle, arith=ol.ARITH_FXP).run(pts)
        g, n = lo.expected_lists(pts, res)  # (its own checks: same indices per (part, category), same z sequence)
        z = pts[:, 2]
        assert differs_only_inside_ties(z, g, res.ground_idx, res.ground_part, res.ground_cat)
        cloud = res.nonground_part_cloud[res.nonground_part]
        keep = ~cloud
        assert differs_only_inside_ties(z, n[keep], res.nonground_idx[keep], res.nonground_part[keep], res.nonground_cat[keep])
        for p in np.nonzero(res.nonground_part_cloud)[0]:  # the oracle builds these in cloud order itself
            at = res.nonground_part == p
            assert np.array_equal(n[at], res.nonground_idx[at]) and (np.diff(n[at]) > 0).all()
        assert len(res.ground_part_cloud) and not res.ground_part_cloud.any()
        # the parts are the patch records' lists, in order
        sizes = np.bincount(res.nonground_part)
        assert sizes.sum() == len(n) and (sizes > 0).all()


def test_hand_made_part():
    """Ten entries of one non-ground part: a round-1 group, a round-2 entry, and the rest with a tie and a +-0 pair."""
    class R:
        pass
    #               idx: 0     1     2     3     4     5     6     7     8     9
    z = np.array([0.5, -0.0, 2.0, 0.0, 2.0, -1.0, 7.0, 0.25, 0.5, -3.0], np.float32)
    r = R()
    r.ground_idx, r.ground_part, r.ground_cat, r.ground_part_cloud = np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.uint8), np.zeros(0, bool)
    # as an unstable sort may leave it: every group ascending in z, the equal heights (0.0 / -0.0, 0.5 / 0.5) in either order
    r.nonground_idx = np.array([7, 6, 4, 9, 5, 3, 1, 8, 0, 2], np.int32)
    r.nonground_part = np.zeros(10, np.int32)
    r.nonground_cat = np.array([1, 1, 2, 255, 255, 255, 255, 255, 255, 255], np.uint8)
    r.nonground_part_cloud = np.array([False])
    pts = np.zeros((10, 4), np.float32)
    pts[:, 2] = z
    g, n = lo.expected_lists(pts, r)
    assert len(g) == 0
    # round 1: 0.25, 7.0; round 2: 2.0 (index 4); rest: -3.0, -1.0, then -0.0 and 0.0 tie -> 1, 3; 0.5 twice -> 0, 8; 2.0 -> 2
    assert n.tolist() == [7, 6, 4, 9, 5, 1, 3, 0, 8, 2]
    # a part in cloud order ignores the heights
    r.nonground_idx = np.array([7, 2, 4], np.int32)
    r.nonground_part, r.nonground_cat, r.nonground_part_cloud = np.zeros(3, np.int32), np.zeros(3, np.uint8), np.array([True])
    assert lo.expected_lists(pts, r)[1].tolist() == [2, 4, 7]
    # an input that is not the z sequence of a sorted part is refused
    r.nonground_idx = np.array([2, 0], np.int32)
    r.nonground_part, r.nonground_cat, r.nonground_part_cloud = np.zeros(2, np.int32), np.full(2, 255, np.uint8), np.array([False])
    with pytest.raises(AssertionError):
        lo.expected_lists(pts, r)


def test_sort_path_rules():
    spread = lo.spread
    c = np.full(5000, 255, np.uint8)
    assert lo.sort_path(c[:256], spread(256)) == "wave" and lo.sort_path(c[:257], spread(257)) == "bucket"
    assert lo.sort_path(c[:4032], spread(4032)) == "bucket" and lo.sort_path(c[:4033], spread(4033)) == "network:above 4032"
    assert lo.sort_path(c[:300], np.where(np.arange(300) % 2 == 0, np.float32(0.0), np.float32(-0.0))) == "network:one height"
    assert lo.sort_path(c[:300], spread(300), cloud_order=True) == "network:one height"
    assert lo.sort_path(c[:300], np.concatenate([spread(299), [np.float32(-np.inf)]])) == "network:non-finite"
    assert lo.sort_path(np.concatenate([c[:299], [1]]), spread(300)) == "network:categories"
    assert lo.sort_path(c[:300], np.concatenate([spread(298), np.float32([3e38, -3e38])])) == "network:scale"
    assert lo.network_size(257) == 512 and lo.network_size(512) == 512 and lo.network_size(513) == 1024 and lo.network_size(4096) == 4096
    assert [lo.tiles_and_passes(n) for n in (4096, 4097, 8192, 8193, 16384, 16385, 32769)] == [(1, 0), (2, 1), (2, 1), (3, 2), (4, 2), (5, 3), (9, 4)]


def test_case_table_is_current():
    """profiles/list_order_cases.txt is what tools/list_order_table.py prints for these cases."""
    import contextlib
    import importlib.util
    import io
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("list_order_table", os.path.join(root, "tools", "list_order_table.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    printed = io.StringIO()
    with contextlib.redirect_stdout(printed):
        tool.main()
    with open(os.path.join(root, "profiles", "list_order_cases.txt")) as f:
        assert f.read() == printed.getvalue()
