"""one_pass_arena_ref.py on the CPU: the restated capacity table against two inputs worked by hand, the restated outcome rule at each
limit, and the cases -- every outcome and reason is reached, every edge has both of its neighbours, every kind of part is moved, and the
oracle finds in every bin and pseudo-bin of every planned frame exactly the points the plan puts there."""
import numpy as np
import pytest

import one_pass_arena_ref as ar
import oracle_lib as ol


@pytest.fixture(scope="module")
def oracle(oracle_built):
    return oracle_built.restatement()


@pytest.fixture(scope="module")
def params(oracle):
    return oracle.default_params()


def test_capacity_table_by_hand():
    """Four bins, the first two split: parts 0-3 are their low and high parts, 4 and 6 the other two bins (5 and 7 never used), 8 the
    RNR hits, 9 the out-of-range points."""
    observed = [100, 0, 50, 7, 1000, 0, 16, 0, 45, 0]
    # one_pass_scale 4 (the default), 17 frames: 1.0625 x + 2 sqrt(x) + 16, truncated, rounded up to 32
    #   100: 106.25 + 20 + 16 = 142 -> 160      0: 16 -> 32              50: 53.125 + 14.14 + 16 = 83 -> 96
    #     7: 7.4375 + 5.29 + 16 = 28 -> 32   1000: 1062.5 + 63.25 + 16 = 1141 -> 1152
    #    16: 17 + 8 + 16 = 41 -> 64            45: 47.8125 + 13.42 + 16 = 77 -> 96
    t = ar.capacity_table(observed, 2000, 17, 4.0, 2, 4)
    assert t.cap == [160, 32, 96, 32, 1152, 0, 64, 0, 96, 32] and not t.few
    assert t.arena_base == 1664
    assert t.arena_slots == 5472  # 1000 + 250 + 2000 / 16 + 4096 = 5471 -> 5472
    assert t.arena_spill == 2048 and t.slots_per_frame == 7136 and t.cap_max_n == 2000
    # no segment is longer than the largest frame + 16
    assert ar.capacity_table(observed, 1000, 17, 4.0, 2, 4).cap[4] == 1024  # 1016 -> 1024
    # a quarter of a large arena holds records: 8000 + 2000 + 1000 + 4096 = 15096 -> 15104
    big = ar.capacity_table([100, 0, 50, 7, 8000, 0, 16, 0, 45, 0], 16000, 17, 4.0, 2, 4)
    assert (big.arena_slots, big.arena_spill) == (15104, 3776)
    # one_pass_scale 0.25: 0.06640625 x + 16;  100: 22 -> 32   1000: 82 -> 96   the others 16-19 -> 32
    s = ar.capacity_table(observed, 2000, 17, 0.25, 2, 4)
    assert s.cap == [32, 32, 32, 32, 96, 0, 32, 0, 32, 32] and not s.few
    assert s.arena_slots == 1376 and s.arena_spill == 1376 and s.slots_per_frame == 320 + 1376  # 5471 / 4 = 1367 -> 1376, all of it for records
    assert not ar.capacity_table(observed, 2000, 3, 0.25, 2, 4).few  # a small scale: an arena whatever the batch
    # 16 frames: 3.75 x + 2048 and no arena;  100: 2423 -> 2432   1000: 5798, at most 4016 -> 4032
    f = ar.capacity_table(observed, 4000, 16, 4.0, 2, 4)
    assert f.few and f.cap == [2432, 2048, 2240, 2080, 4032, 0, 2112, 0, 2240, 2048]
    assert (f.arena_slots, f.arena_spill, f.slots_per_frame) == (0, 0, sum(f.cap))
    # debug_flags 2048: the segments of 17 frames, no arena
    d = ar.capacity_table(observed, 2000, 17, 4.0, 2, 4, ar.NO_ARENA_FLAG)
    assert d.cap == t.cap and d.arena_slots == 0 and d.slots_per_frame == 1664


def test_rebuild_rule():
    t = ar.capacity_table([100, 0, 50, 7, 1000, 0, 16, 0, 45, 0], 2000, 17, 4.0, 2, 4)
    assert ar.next_table(None, False, 100, 17, 4.0) == (True, True)
    assert ar.next_table(t, False, 2000, 17, 4.0) == (False, False) and ar.next_table(t, False, 1000, 40, 4.0) == (False, False)
    assert ar.next_table(t, False, 2001, 17, 4.0) == (True, False)   # a larger frame than the table was built for
    assert ar.next_table(t, False, 999, 17, 4.0) == (True, True)     # a much smaller sensor: observed maxima start over
    assert ar.next_table(t, True, 1500, 17, 4.0) == (True, False)    # stale: a part held more than ever before
    assert ar.next_table(t, False, 1500, 16, 4.0) == (True, False)   # few frames now
    assert ar.next_table(t, False, 1500, 16, 0.25) == (False, False)
    assert ar.passed_max_n(1001) == 1126


def test_outcome_rule_at_every_limit():
    t = ar.capacity_table([0] * 200, 4000, 17, 4.0, 0, 99)  # 198 real parts, 99 of them in use, capacity 32 each; 4 352 arena slots
    assert t.arena_slots == 4352 and t.arena_spill == 2048 and t.cap[0] == 32 and t.cap[1] == 0

    def frame(**parts):
        c = [0] * 200
        for k, v in parts.items():
            c[int(k[1:])] = v
        return c
    assert str(ar.outcome(frame(p0=32, p2=32), t)) == "fits"
    o = ar.outcome(frame(p0=33, p4=40), t)
    assert (o.kind, o.nov, o.spilled, o.run, o.moved) == ("moved", 2, 9, 32 + 64 + 64, (0, 4))
    many = lambda k: [33 if b % 2 == 0 and b // 2 < k else 0 for b in range(200)]
    assert str(ar.outcome(many(64), t)) == "moved" and ar.outcome(many(64), t).run == 64 + 64 * 64
    assert str(ar.outcome(many(65), t)) == "host: too-many-parts"
    assert str(ar.outcome(frame(p0=32 + 2048), t)) == "moved" and str(ar.outcome(frame(p0=32 + 2049), t)) == "host: spill-full"
    # three parts seen with 2 000 points: 2125 + 89.4 + 16 = 2230 -> 2240 slots each; the arena 2000 + 500 + 250 + 4096 = 6846 -> 6848
    big = ar.capacity_table([2000, 0, 2000, 0, 2000, 0] + [0] * 194, 4000, 17, 4.0, 0, 99)
    assert big.cap[:6] == [2240, 0, 2240, 0, 2240, 0] and big.arena_slots == 6848
    o = ar.outcome(frame(p0=2241, p2=2241, p4=2241), big)   # 3 records -> 32, then 3 x 2272
    assert (str(o), o.run) == ("moved", 6848)
    o = ar.outcome(frame(p0=2241, p2=2241, p4=2273), big)   # 35 records -> 64, 2272 + 2272 + 2304
    assert (str(o), o.run, o.spilled) == ("host: arena-full", 6912, 35)
    # the first reason in the kernel's order
    assert str(ar.outcome([33 if b % 2 == 0 and b < 130 else 0 for b in range(199)] + [5000], t)) == "host: too-many-parts"
    none = ar.capacity_table([0] * 200, 4000, 16, 4.0, 0, 99)
    assert str(ar.outcome(frame(p0=2049), none)) == "host: no-arena" and str(ar.outcome(frame(p0=2048), none)) == "fits"


def test_redo_policy():
    t = ar.capacity_table([0] * 200, 4000, 40, 4.0, 0, 99)
    fits, moved, host = ar.Outcome("fits"), ar.Outcome("moved"), ar.Outcome("host", "arena-full")
    pr = ar.predict([fits] * 38 + [moved] * 2, [500] * 40, t, 200)
    assert (pr.arena, pr.redo_stats, pr.one_pass_stats, pr.redo) == (2, (40, 0), (1, 0), None)
    room = t.slots_per_frame - 31 * 200 - 32  # the largest frame that can be redone inside its own slots
    pr = ar.predict([fits] * 37 + [moved] * 2 + [host], [500] * 39 + [room], t, 200)
    assert (pr.arena, pr.redo_stats, pr.one_pass_stats, pr.redo) == (2, (40, 1), (1, 1), "in-place")
    pr = ar.predict([fits] * 37 + [moved] * 2 + [host], [500] * 39 + [room + 1], t, 200)
    assert (pr.arena, pr.redo_stats, pr.one_pass_stats, pr.redo) == (0, (40, 40), (1, 1), "whole-batch")
    pr = ar.predict([fits] * 37 + [moved] * 2 + [host], [500] * 40, t, 200, redo_whole_batch=True)
    assert pr.redo == "whole-batch"
    every_other = [host if f % 2 == 0 and f < 34 else fits for f in range(300)]  # 17 runs of frames, more than an eighth of 100 frames
    assert ar.predict(every_other[:100], [500] * 100, t, 200).redo == "whole-batch"
    assert ar.predict(every_other, [500] * 300, t, 200).redo == "in-place"    # 17 of 300 frames: each run on its own


@pytest.mark.parametrize("case", ar.CASES, ids=repr)
def test_planned_counts_are_the_oracles(oracle, params, case):
    """Every planned frame: the restated part of every point gives the planned counts, the oracle's patch records report the same
    points per bin, and its RNR and out-of-range lists have the planned lengths."""
    b = case.built(params)
    seen = set()
    for i, pts in enumerate(b.test):
        if id(pts) in seen:
            continue
        seen.add(id(pts))
        planned = b.counts[i]
        assert len(pts) == b.specs[i].n() == planned.sum()
        part = ar.parts_of_points(params, pts)
        assert np.array_equal(np.bincount(part, minlength=len(planned)), planned), (case.name, i)
        res = ol.Estimator(oracle, params, arith=ol.ARITH_FXP).run(pts)
        B = ar.num_bins(params)
        per_bin = planned[0:2 * B:2] + planned[1:2 * B:2]
        assert (per_bin[per_bin > 0] >= params.num_min_pts).all()  # (a smaller bin has no record)
        rec = np.zeros(B, np.int64)
        rec[res.records["bin"]] = res.records["n_points"]
        assert len(np.unique(res.records["bin"])) == len(res.records) and np.array_equal(rec, per_bin), (case.name, i)
        for pseudo in (2 * B, 2 * B + 1):
            mine = np.nonzero(part == pseudo)[0]
            assert len(mine) == planned[pseudo]
            if len(mine):
                at = np.nonzero(res.nonground_idx == mine[0])[0]
                assert len(at) == 1
                q = res.nonground_part[at[0]]
                assert res.nonground_part_cloud[q] and np.array_equal(res.nonground_idx[res.nonground_part == q], mine), (case.name, i, pseudo)
        assert len(res.ground_idx) + len(res.nonground_idx) == len(pts)


def test_every_frame_has_the_outcome_it_is_there_for(params):
    for case in ar.CASES:
        b = case.built(params)
        assert str(ar.outcome(b.observed, b.sizing_table)) == "fits"
        for i, f in b.plan.items():
            assert str(b.outcomes[i]) == f.want, (case.name, i, f.edge, f.delta, str(b.outcomes[i]))
        for i in range(case.frames):
            if i not in b.plan:
                assert b.outcomes[i].kind == "fits"
        # the same batch again fits the rebuilt table -- unless one_pass_scale sizes the segments below the counts they have seen
        assert all(o.kind == "fits" for o in b.again_outcomes) == (case.scale >= 1.0), case.name
        assert b.again_prediction.redo_stats[0] == case.frames
        hosts = sum(o.kind == "host" for o in b.outcomes)
        assert hosts == 0 or all(o.kind != "moved" for o in b.outcomes) or b.prediction.redo == "in-place", \
            "%s: a redo of the whole batch would hide the frames that moved parts" % case.name


def test_cases_reach_every_outcome_and_both_sides_of_every_edge(params):
    frames = [(case, b, i, f) for case in ar.CASES for b in [case.built(params)] for i, f in b.plan.items()]
    got = {str(b.outcomes[i]) for _, b, i, _ in frames}
    assert got == {"fits", "moved", "host: too-many-parts", "host: spill-full", "host: arena-full", "host: no-arena"}
    assert {b.prediction.redo for _, b, _, _ in frames} == {None, "in-place", "whole-batch"}
    at = lambda edge: {f.delta: (b.outcomes[i], b.test_table) for _, b, i, f in frames if f.edge == edge}
    # segment: capacity - 1, capacity, capacity + 1 for every kind of part
    for kind, parts in ar.KINDS:
        e = at("segment:" + kind)
        assert [str(e[d][0]) for d in (-1, 0, 1)] == ["fits", "fits", "moved"], kind
        assert e[1][0].spilled == len(parts) and e[1][0].nov == len(parts)
    e = at("parts")
    assert [(e[d][0].nov, str(e[d][0])) for d in (-1, 0, 1)] == [(63, "moved"), (64, "moved"), (65, "host: too-many-parts")]
    for edge in ("spill:single", "spill:spread"):
        e = at(edge)
        assert [(e[d][0].spilled - e[d][1].arena_spill, str(e[d][0])) for d in (-1, 0, 1)] == [(-1, "moved"), (0, "moved"), (1, "host: spill-full")]
        assert all(e[d][0].run + 256 <= e[d][1].arena_slots for d in (-1, 0)) and (e[0][0].nov == 1) == (edge == "spill:single")
    e = at("arena")
    assert [(e[d][0].run - e[d][1].arena_slots, str(e[d][0])) for d in (-32, 0, 32)] == [(-32, "moved"), (0, "moved"), (32, "host: arena-full")]
    assert all(3 * e[d][0].spilled < 2 * e[d][1].arena_spill and e[d][0].nov == 3 for d in e)
    e = at("small:room")
    assert e[0][0].run == e[0][1].arena_slots and str(e[0][0]) == "moved" and str(e[1][0]) == "host: arena-full" and e[1][0].spilled == e[0][0].spilled + 1
    e = at("small:records")
    assert e[0][0].spilled == e[0][1].arena_slots == e[0][1].arena_spill < 2048 and str(e[0][0]) == "host: arena-full" and str(e[1][0]) == "host: spill-full"
    assert str(at("small:one-record")[0][0]) == "moved" and at("small:one-record")[0][0].spilled == 1
    # the same frames with and without an arena
    by = {c.name: c.built(params) for c in ar.CASES}
    for twin in ("few-16", "debug-2048"):
        for i in by[twin].plan:
            assert by[twin].test[i].tobytes() == by["arena-17"].test[i].tobytes()
            assert str(by[twin].outcomes[i]) == "host: no-arena" and str(by["arena-17"].outcomes[i]) == "moved"
    assert by["few-16"].test_table.few and not by["debug-2048"].test_table.few
    # positions, rank interleaving, fix-up
    assert {i for i in by["positions"].plan} == {0, 8, 9, 16} and by["positions"].prediction.arena == 4
    seg = by["segment-edge"]
    assert seg.outcomes[0].kind == "moved" and seg.outcomes[40].kind == "moved" and all(seg.outcomes[i].kind == "moved" for i in range(29, 41))
    assert by["ranks"].outcomes[7].moved == (63, 64) and min(by["ranks"].counts[7][63:65]) // 8 > 64  # (bits of one part reach past the pad)
    for i, f in by["ranks"].plan.items():
        if f.pair is None:
            continue
        pts, part = by["ranks"].test[i], ar.parts_of_points(params, by["ranks"].test[i])
        a, c = (ar.part_index(params, s) for s in f.pair)
        assert c == a + 1 and min(by["ranks"].counts[i][a], by["ranks"].counts[i][c]) >= 3000
        pair = np.nonzero((part == a) | (part == c))[0]
        alternating = int((np.diff(pair) == 1).sum())
        if f.layout == "one-tile":
            assert pair[0] == 1024 and alternating >= 2 * 3000  # one block from the second tile on, low and high in turn
            assert (part[1024:1024 + 6000:2] == a).all() and (part[1025:1025 + 6000:2] == c).all()
        else:
            assert pair[-1] - pair[0] > 0.9 * len(pts) and (part[pair[:6000:2]] == a).all() and (part[pair[1:6000:2]] == c).all()
    assert np.isneginf(by["fixup"].test[7][:, 2]).sum() == 1


def test_every_kind_of_part_is_moved(params):
    kinds = set()
    for case in ar.CASES:
        for o in case.built(params).outcomes:
            kinds |= {ar.part_kind(params, q) for q in o.moved}
    assert kinds == {"low", "high", "zone1", "zone2", "zone3", "rnr", "far"}
    moved = {q for case in ar.CASES for o in case.built(params).outcomes for q in o.moved}
    B = ar.num_bins(params)
    assert {0, 2 * B - 2, 2 * B, 2 * B + 1} <= moved  # part 0, the last real part, both pseudo-bins
    both = [o for case in ar.CASES for o in case.built(params).outcomes if {2 * B, 2 * B + 1} <= set(o.moved)]
    high_alone = [o for case in ar.CASES for o in case.built(params).outcomes if len(o.moved) == 1 and ar.part_kind(params, o.moved[0]) == "high"]
    assert both and high_alone
    # 64 parts out of part order for the insertion sort: spread over the range, both sides of split bins among them
    o = next(o for case in ar.CASES for o in case.built(params).outcomes if o.nov == 64 and o.kind == "moved")
    assert max(o.moved) - min(o.moved) > 1.5 * B and {ar.part_kind(params, q) for q in o.moved} >= {"low", "high", "zone1", "zone2", "zone3", "rnr"}


def test_case_table_is_current():
    """profiles/one_pass_arena_cases.txt is what tools/one_pass_arena_table.py prints for these cases."""
    import contextlib
    import importlib.util
    import io
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("one_pass_arena_table", os.path.join(root, "tools", "one_pass_arena_table.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    printed = io.StringIO()
    with contextlib.redirect_stdout(printed):
        tool.main()
    with open(os.path.join(root, "profiles", "one_pass_arena_cases.txt")) as f:
        assert f.read() == printed.getvalue()
