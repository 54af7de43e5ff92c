"""PWPP_ORDER_REFERENCE entry for entry (K7: k_order_worklist, k_order_sublists): on clouds built so that a part of chosen
length and chosen heights reaches every size regime and every fall-back of the sort (list_order_ref.py, the account in
profiles/list_order_cases.txt), both index lists equal what the contract demands -- the oracle's lists with every part in
(category, z with -0 taken as +0, cloud index) order, parts in cloud order by index alone.  No tolerance: ties are checked."""
import numpy as np
import pytest

import list_order_ref as lo
import oracle_lib as ol
import pwpp_hip
from test_gpu_parity import apply_variant, to_oracle_params

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def oracle(oracle_built):
    return oracle_built.restatement()


class Built:
    def __init__(self, oracle, case, permuted=False):
        self.case = case
        self.params = apply_variant(pwpp_hip.default_params(), case.variant)
        pts, _ = case.cloud(self.params)
        if permuted:  # the same rows in another order: ties follow the new indices
            self.perm = np.random.default_rng(len(pts)).permutation(len(pts))
            pts = np.ascontiguousarray(pts[self.perm])
        self.pts = pts
        self.ref = ol.Estimator(oracle, to_oracle_params(self.params), arith=ol.ARITH_FXP).run(pts)
        self.ground, self.nonground = lo.expected_lists(pts, self.ref)


GROUPS = []  # the cases that share a parameter block share a handle and a batch
for _c in lo.CASES:
    if _c.variant not in GROUPS:
        GROUPS.append(_c.variant)


@pytest.fixture(scope="module")
def built(oracle):
    return {c.name: Built(oracle, c) for c in lo.CASES}


@pytest.fixture(scope="module")
def handles():
    out = []
    for variant in GROUPS:
        h = pwpp_hip.Handle(apply_variant(pwpp_hip.default_params(), variant))
        h.set_output_order(True)
        out.append(h)
    return out


def lists_of(h, i):
    return h.ground_indices(i).copy(), h.nonground_indices(i).copy()


def first_difference(z, mine, want):
    d = np.nonzero(mine != want)[0]
    k = int(d[0])
    return "%d of %d entries differ, first at %d: index %d (z %r) where %d (z %r) belongs" % (
        len(d), len(want), k, mine[k], float(z[mine[k]]), want[k], float(z[want[k]]))


def assert_lists(h, i, b):
    g, n = lists_of(h, i)
    assert len(g) == len(b.ground) and len(n) == len(b.nonground), (b.case.name, len(g), len(n))
    assert np.array_equal(g, b.ground), "%s, ground list: %s" % (b.case.name, first_difference(b.pts[:, 2], g, b.ground))
    assert np.array_equal(n, b.nonground), "%s, non-ground list: %s" % (b.case.name, first_difference(b.pts[:, 2], n, b.nonground))
    # getGround() / getNonground() rows follow the lists
    assert h.ground(i).tobytes() == b.pts[g, :3].tobytes() and h.nonground(i).tobytes() == b.pts[n, :3].tobytes()
    return g, n


@pytest.mark.parametrize("case", lo.CASES, ids=repr)
def test_one_frame_alone(built, handles, case):
    """a call with that frame alone: the latency plan, two-pass binning"""
    b = built[case.name]
    h = handles[GROUPS.index(case.variant)]
    h.estimate_ground_batch([b.pts], mode=pwpp_hip.MODE_FRESH)
    first = assert_lists(h, 0, b)
    h.estimate_ground_batch([b.pts], mode=pwpp_hip.MODE_FRESH)
    again = lists_of(h, 0)
    assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes()


@pytest.mark.parametrize("group", range(len(GROUPS)), ids=lambda g: ",".join("%s=%s" % kv for kv in GROUPS[g].items()) or "default")
def test_all_cases_in_one_batch_launched_twice(built, group):
    """one batch of all the cases of a parameter block (one-pass binning); the second launch knows the long bins"""
    cases = [c for c in lo.CASES if c.variant == GROUPS[group]]
    h = pwpp_hip.Handle(apply_variant(pwpp_hip.default_params(), GROUPS[group]))
    h.set_output_order(True)
    frames = [built[c.name].pts for c in cases]
    seen = []
    for launch in range(2):
        h.estimate_ground_batch(frames, mode=pwpp_hip.MODE_FRESH)
        seen.append([assert_lists(h, i, built[c.name]) for i, c in enumerate(cases)])
    for (g0, n0), (g1, n1) in zip(*seen):
        assert g0.tobytes() == g1.tobytes() and n0.tobytes() == n1.tobytes()
    # the default order again: the same sets
    h.set_output_order(False)
    h.estimate_ground_batch(frames, mode=pwpp_hip.MODE_FRESH)
    for i, c in enumerate(cases):
        g, n = lists_of(h, i)
        assert np.array_equal(np.sort(g), np.sort(built[c.name].ground)) and np.array_equal(np.sort(n), np.sort(built[c.name].nonground))


@pytest.mark.parametrize("group", range(len(GROUPS)), ids=lambda g: ",".join("%s=%s" % kv for kv in GROUPS[g].items()) or "default")
def test_rows_permuted(oracle, built, group):
    """The same clouds with their rows permuted give the expected lists of the permuted clouds: the heights come in the same
    sequence, the same points are listed, and ties follow the NEW indices."""
    cases = [c for c in lo.CASES if c.variant == GROUPS[group]]
    moved = [Built(oracle, c, permuted=True) for c in cases]
    h = pwpp_hip.Handle(apply_variant(pwpp_hip.default_params(), GROUPS[group]))
    h.set_output_order(True)
    h.estimate_ground_batch([m.pts for m in moved], mode=pwpp_hip.MODE_FRESH)
    for i, (c, m) in enumerate(zip(cases, moved)):
        g, n = assert_lists(h, i, m)
        b = built[c.name]
        for mine, theirs in ((g, b.ground), (n, b.nonground)):
            assert np.array_equal(np.sort(m.perm[mine]), np.sort(theirs))  # (row j of the permuted cloud is row perm[j] of the original)
        assert np.array_equal(m.pts[g, 2], b.pts[b.ground, 2])
        z_sorted = ~b.ref.nonground_part_cloud[b.ref.nonground_part]  # (a part in cloud order lists other heights first now)
        assert np.array_equal(m.pts[n, 2][z_sorted], b.pts[b.nonground, 2][z_sorted])
