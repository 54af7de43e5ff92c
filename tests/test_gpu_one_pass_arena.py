"""The overflow arena of one-pass binning at each of its limits (k_czm_bin_scatter, k_czm_scan, build_capacity_table, finish_pending,
pwpp_member_offset): synthetic frames whose parts hold chosen numbers of points (one_pass_arena_ref.py, the account in
profiles/one_pass_arena_cases.txt) put one count at a time at its edge -- a segment at its capacity, 64 overgrown parts, the room for
spilled records, the arena's last slot -- and on both sides of it.  Per case: the restated capacity table is the handle's, the
statistics gain exactly what the restatement predicts (frames that moved parts, frames redone, batches redone), every frame is the
oracle's bit for bit, and the same batch again fits the rebuilt table.  On a subset also the index lists entry for entry in reference
and in cloud order, labels, per-point patch and distance, gathered records, the same frames as lock-step streams; one case runs as two
frame ranges, one needs k_fit_fixup for a frame with a moved part."""
import numpy as np
import pytest

import list_order_ref as lo
import one_pass_arena_ref as ar
import oracle_lib as ol
import pwpp_hip
from test_gpu_labels import check_labels
from test_gpu_parity import assert_frame_equal, to_oracle_params
from test_gpu_point_planes import check_point_planes
from test_gpu_point_records import check_records, matrix_src

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def oracle(oracle_built):
    return oracle_built.restatement()


@pytest.fixture(scope="module")
def op():
    return to_oracle_params(pwpp_hip.default_params())


_refs = {}  # id(cloud) -> (cloud, the oracle's result for it as a fresh frame): identical frames share one run


def ref_of(oracle, op, pts):
    if id(pts) not in _refs:
        _refs[id(pts)] = (pts, ol.Estimator(oracle, op, arith=ol.ARITH_FXP).run(pts))
    return _refs[id(pts)][1]


def handle_for(case):
    h = pwpp_hip.Handle()
    if case.scale != 4.0:
        h.set_option("one_pass_scale", case.scale)
    if case.debug:
        h.set_option("debug_flags", case.debug)
    if case.whole_batch:
        h.set_option("redo_whole_batch", 1)
    return h


def stats(h):
    return h.arena_stats()[0], h.redo_stats(), h.one_pass_stats()


def gained(h, before):
    a, r, o = stats(h)
    return a - before[0], (r[0] - before[1][0], r[1] - before[1][1]), (o[0] - before[2][0], o[1] - before[2][1])


def sized(case, b, mode=pwpp_hip.MODE_FRESH, h=None):
    """a handle that has seen the sizing batch: its table is the restated one, nothing moved, nothing redone"""
    h = handle_for(case) if h is None else h
    h.estimate_ground_batch(b.sizing, mode=mode)
    assert h.arena_stats()[1:] == (b.sizing_table.slots_per_frame, b.sizing_table.arena_slots), (case.name, h.arena_stats())
    assert stats(h) == (0, (case.frames, 0), (1, 0)), (case.name, stats(h))
    return h


def assert_gain(case, h, before, pr, what):
    got = gained(h, before)
    print("%s, %s: gained %s, predicted %s" % (case.name, what, got, (pr.arena, pr.redo_stats, pr.one_pass_stats)))
    assert got == (pr.arena, pr.redo_stats, pr.one_pass_stats), "%s, %s: statistics gained %s, predicted %s" % (case.name, what, got, pr)


@pytest.mark.parametrize("case", ar.CASES, ids=repr)
def test_case(oracle, op, case):
    b = case.built(op)
    h = sized(case, b)
    fixed = h.fixed_up_frames()
    before = stats(h)
    h.estimate_ground_batch(b.test, mode=pwpp_hip.MODE_FRESH)
    assert_gain(case, h, before, b.prediction, "test batch")
    assert h.arena_stats()[1:] == (b.test_table.slots_per_frame, b.test_table.arena_slots), (case.name, h.arena_stats())
    for i, pts in enumerate(b.test):
        assert_frame_equal(h, i, ref_of(oracle, op, pts), len(pts))
    if case.name == "fixup":
        assert h.fixed_up_frames() == fixed + 1  # the frame with the moved part, finished by k_fit_fixup
    else:
        assert h.fixed_up_frames() == fixed
    lists = [(h.ground_indices(i).copy(), h.nonground_indices(i).copy()) for i in sorted(b.plan)]
    # the same batch again: the rebuilt table holds every count (a one_pass_scale below 1 sizes segments below the counts it has seen:
    # there the restatement says what moves or goes back to the host this time)
    before = stats(h)
    h.estimate_ground_batch(b.test, mode=pwpp_hip.MODE_FRESH)
    assert case.scale < 1.0 or all(o.kind == "fits" for o in b.again_outcomes)
    assert_gain(case, h, before, b.again_prediction, "the same batch again")
    assert h.arena_stats()[1:] == (b.again_table.slots_per_frame, b.again_table.arena_slots), (case.name, h.arena_stats())
    for i, pts in enumerate(b.test):
        assert_frame_equal(h, i, ref_of(oracle, op, pts), len(pts))
    for (g, n), i in zip(lists, sorted(b.plan)):  # (scatter order: the same sets)
        assert np.array_equal(np.sort(g), np.sort(h.ground_indices(i))) and np.array_equal(np.sort(n), np.sort(h.nonground_indices(i)))
    h.close()


DEEP = [c for c in ar.CASES if c.name in ar.DEEP]


@pytest.mark.parametrize("order", [pwpp_hip.ORDER_REFERENCE, pwpp_hip.ORDER_CLOUD], ids=["reference-order", "cloud-order"])
@pytest.mark.parametrize("case", DEEP, ids=repr)
def test_lists_and_per_point_outputs(oracle, op, case, order):
    """both lists entry for entry, labels, per-point patch and distance and the gathered records of every planned frame"""
    b = case.built(op)
    h = handle_for(case)
    h.set_order(order)
    h.set_labels(True)
    h.set_point_planes(True)
    h.set_point_records(True)
    sized(case, b, h=h)
    before = stats(h)
    h.estimate_ground_batch(b.test, mode=pwpp_hip.MODE_FRESH)
    assert_gain(case, h, before, b.prediction, "test batch")
    for i in sorted(b.plan) + [j for j in (0, case.frames - 1) if j not in b.plan]:
        pts, ref = b.test[i], ref_of(oracle, op, b.test[i])
        assert_frame_equal(h, i, ref, len(pts))
        g, n = h.ground_indices(i).copy(), h.nonground_indices(i).copy()
        if order == pwpp_hip.ORDER_REFERENCE:
            want_g, want_n = lo.expected_lists(pts, ref)
        else:
            want_g, want_n = np.sort(ref.ground_idx), np.sort(ref.nonground_idx)
        assert np.array_equal(g, want_g), "%s frame %d: ground list differs at %s" % (case.name, i, np.flatnonzero(g != want_g)[:8])
        assert np.array_equal(n, want_n), "%s frame %d: non-ground list differs at %s" % (case.name, i, np.flatnonzero(n != want_n)[:8])
        check_labels(h, i, len(pts), ref, cloud=order == pwpp_hip.ORDER_CLOUD)
        check_point_planes(h, i, pts, ref, h.params)
        check_records(h, i, matrix_src(pts), 16)
    h.close()


@pytest.mark.parametrize("case", DEEP, ids=repr)
def test_as_streams_in_lock_step(oracle, op, case):
    """one stream per frame: two steps of the sizing frame, the test batch at the third step, the sizing frame again; state and
    histories of every stream are the oracle's, and a stream whose frame moves parts is not redone"""
    b = case.built(op)
    S = case.frames
    h = handle_for(case)
    h.set_num_streams(S)
    ests = [ol.Estimator(oracle, op, arith=ol.ARITH_FXP) for _ in range(S)]
    height = [op.sensor_height] * S
    for step in range(4):
        frames = b.test if step == 2 else b.sizing
        # a stream splits its bins and tests for RNR at its ADAPTED sensor height: the planned counts hold while that stays within the
        # 0.3 m the clouds keep from the split height (one_pass_arena_ref.place)
        assert step == 3 or max(abs(v - op.sensor_height) for v in height) < 0.25, (case.name, step, height)
        before = stats(h)
        h.estimate_ground_batch(frames, mode=pwpp_hip.MODE_STREAMS)
        if step == 0:
            assert h.arena_stats()[1:] == (b.sizing_table.slots_per_frame, b.sizing_table.arena_slots)
        pr = b.prediction if step == 2 else ar.resubmitted(S)
        assert_gain(case, h, before, pr, "step %d" % step)
        for s in range(S):
            ref = ests[s].run(frames[s])
            height[s] = ref.sensor_height
            if step >= 2 or s in (0, S - 1):
                assert_frame_equal(h, s, ref, len(frames[s]), state_index=s)
    h.close()
