"""The 16-lane rows of k_fit_w64 at the ends of their parts, on a real MI355X.  A row deals a part out in chunks of eight slots per lane
and loads only the slots below the part's end (load_chunk, load_chunk_z): the registers of the other slots hold anything, and every
consumer masks them.  Synthetic frames of one to four patches put a part's end at every place of a chunk -- inside the first slot row,
at a row's last lane, one beyond it, at a chunk's last slot, one beyond it -- stored in one part and split across a low and a high
part, beside a 1023-point patch in the same sub-batch (the wave runs every row to the longest row's trip count), in a part that was
moved into the overflow arena, in the last bin of the last frame with the slots behind it full of points that would change the plane,
and in a zone-0 patch whose wall R-VPF strips.  Every frame is compared with the restatement bit for bit (assert_frame_equal, as
test_gpu_fit_limits.py does), under every plan token of the 16-lane kernel and both sum widths."""
import numpy as np
import pytest

import list_order_ref as lo
import one_pass_arena_ref as ar
import oracle_lib as ol
import pwpp_hip
from test_gpu_one_pass_arena import gained, stats
from test_gpu_parity import assert_frame_equal, to_oracle_params

pytestmark = pytest.mark.gpu

WIDTHS = [pytest.param(True, id="wide"), pytest.param(False, id="narrow")]
PLANS = ["W16:1023", "W16.16:1023", "W16.32:1023"]
MIN_PTS = 10  # the default num_min_pts: the smallest patch that is fitted at all (test_the_frames_hold_every_size)
SIZES = (MIN_PTS, 15, 16, 17, 127, 128, 129, 255, 256, 1023)
# four patches per frame: one wave, ONE sub-batch of four rows -- twice the 1023-point patch (eight chunks) beside the smallest (one slot row)
GROUPS = ((MIN_PTS, 1023, 16, 128), (15, 17, 127, 129), (255, 256, MIN_PTS, 1023))
UNSPLIT_BINS = ((1, 0, 2), (1, 1, 9), (2, 1, 5), (3, 0, 7))  # zones 1-3: one stored part, no R-VPF
SPLIT_BINS = ((0, 0, 1), (0, 0, 6), (0, 1, 3), (0, 1, 12))   # zone 0: a low and a high part, R-VPF first


@pytest.fixture(scope="module")
def oracle(oracle_built):
    return oracle_built.restatement()


@pytest.fixture(scope="module")
def op():
    return to_oracle_params(pwpp_hip.default_params())


_refs = {}  # (id(cloud), wide) -> (cloud, the restatement's result for it as a fresh frame)


def ref_of(oracle, op, pts, wide):
    key = (id(pts), wide)
    if key not in _refs:
        _refs[key] = (pts, ol.Estimator(oracle, op, arith=ol.ARITH_FXP if wide else ol.ARITH_FXP21).run(pts))
    return _refs[key][1]


def make_handle(plan, wide):
    h = pwpp_hip.Handle()
    if not wide:
        h.set_option("exact_moments", 0)
    h.set_option("fit_plan", plan)
    return h


def cloud_of(p, counts, seed):
    """A shuffled frame with exactly counts[spec] points in each part (one_pass_arena_ref.place), checked with the restated binning."""
    rng = np.random.default_rng(seed)
    pts = np.concatenate([ar.place(rng, p, spec, n) for spec, n in sorted(counts.items())], axis=0)
    pts = np.ascontiguousarray(pts[rng.permutation(len(pts))])
    got = np.bincount(ar.parts_of_points(p, pts), minlength=ar.num_parts(p))
    for spec, n in counts.items():
        assert got[ar.part_index(p, spec)] == n, (spec, n)
    assert got.sum() == sum(counts.values())
    return pts


_size_frames = {}


def size_frames(two_parts):
    """The three frames of GROUPS; two_parts: every patch in a zone-0 bin, half of it below the split height and half above."""
    if two_parts not in _size_frames:
        p = pwpp_hip.default_params()
        frames = []
        for g, sizes in enumerate(GROUPS):
            counts = {}
            for n, b in zip(sizes, SPLIT_BINS if two_parts else UNSPLIT_BINS):
                if two_parts:
                    counts[("lo",) + b], counts[("hi",) + b] = (n + 1) // 2, n // 2
                else:
                    counts[("bin",) + b] = n
            frames.append((cloud_of(p, counts, [16, g, int(two_parts)]), sizes))
        _size_frames[two_parts] = frames
    return _size_frames[two_parts]


def test_the_frames_hold_every_size():
    assert int(pwpp_hip.default_params().num_min_pts) == MIN_PTS
    assert sorted({n for g in GROUPS for n in g}) == sorted(set(SIZES))
    assert any(MIN_PTS in g and 1023 in g for g in GROUPS)


@pytest.mark.parametrize("wide", WIDTHS)
@pytest.mark.parametrize("two_parts", [False, True], ids=["one-part", "two-parts"])
@pytest.mark.parametrize("plan", PLANS)
def test_a_parts_end_at_every_place_of_a_chunk(oracle, op, plan, two_parts, wide):
    frames = size_frames(two_parts)
    h = make_handle(plan, wide)
    h.estimate_ground_batch([pts for pts, _ in frames], mode=pwpp_hip.MODE_FRESH)
    for k, (pts, sizes) in enumerate(frames):
        ref = ref_of(oracle, op, pts, wide)
        assert sorted(int(n) for n in ref.records["n_points"]) == sorted(sizes)  # (the patches are what the frame was built for)
        assert_frame_equal(h, k, ref, len(pts))
    assert h.fixed_up_frames() == 0
    h.close()


ARENA_CASE = next(c for c in ar.CASES if c.name == "segment-edge")


@pytest.mark.parametrize("wide", WIDTHS)
@pytest.mark.parametrize("plan", PLANS)
def test_parts_moved_into_the_overflow_arena(oracle, op, plan, wide):
    """test_gpu_one_pass_arena.py's segment-edge batch: every kind of part one point over its segment, hence stored in the arena, far
    from its bin's other part and with another frame's moved parts behind it."""
    case = ARENA_CASE
    b = case.built(op)
    assert b.prediction.arena > 0  # (frames whose parts the device moved)
    h = make_handle(plan, wide)
    h.estimate_ground_batch(b.sizing, mode=pwpp_hip.MODE_FRESH)
    before = stats(h)
    h.estimate_ground_batch(b.test, mode=pwpp_hip.MODE_FRESH)
    assert gained(h, before) == (b.prediction.arena, b.prediction.redo_stats, b.prediction.one_pass_stats)
    for i, pts in enumerate(b.test):
        assert_frame_equal(h, i, ref_of(oracle, op, pts, wide), len(pts))
    assert h.fixed_up_frames() == 0
    h.close()


def poisoned(p, spec, n, seed):
    """n points of the part `spec` three metres below the floor (intensity 0.5: no RNR hit): any one of them among a patch's points
    becomes its lowest-point representative and moves the plane."""
    rng = np.random.default_rng(seed)
    pts = ar.place(rng, p, spec, n)
    pts[:, 2] = -float(p.sensor_height) - 3.0 + rng.uniform(-0.03, 0.03, n)
    return pts


@pytest.mark.parametrize("wide", WIDTHS)
@pytest.mark.parametrize("n_last", [17, 129])
@pytest.mark.parametrize("plan", PLANS)
def test_the_last_bin_of_the_last_frame(oracle, op, plan, n_last, wide):
    """The patch whose chunks reach furthest: the last bin's, in the last frame.  A first call fills that bin's slots in that frame
    with 600 poisoned points; the second call leaves n_last points there, so that the slots behind them still hold the poison.
    Frame 0 is the largest frame of both calls and the same, so both meet the same capacity table."""
    p = pwpp_hip.default_params()
    first = cloud_of(p, {ar.Z1: 900, ar.Z3: 700, ar.LAST: 600}, [17, 0])
    rng = np.random.default_rng([17, 1])
    base = {ar.Z1: 80, ar.Z2: 70, ar.P0: 40}
    loud = np.concatenate([cloud_of(p, base, [17, 2]), poisoned(p, ar.LAST, 600, [17, 3])], axis=0)
    loud = np.ascontiguousarray(loud[rng.permutation(len(loud))])
    quiet = cloud_of(p, {**base, ar.LAST: n_last}, [17, 4, n_last])
    assert len(loud) < len(first) and len(quiet) < len(first)
    h = make_handle(plan, wide)
    h.estimate_ground_batch([first, loud], mode=pwpp_hip.MODE_FRESH)
    table = h.arena_stats()[1:]
    assert_frame_equal(h, 1, ref_of(oracle, op, loud, wide), len(loud))
    h.estimate_ground_batch([first, quiet], mode=pwpp_hip.MODE_FRESH)
    assert h.arena_stats()[1:] == table  # (the same segments: the poison lies where the last bin's slots are)
    ref = ref_of(oracle, op, quiet, wide)
    assert n_last in [int(n) for n in ref.records["n_points"]]
    assert_frame_equal(h, 1, ref, len(quiet))
    assert_frame_equal(h, 0, ref_of(oracle, op, first, wide), len(first))
    h.close()


WALLS = ((350, 30), (700, 259))  # (points of the wall, points of the column): 444 and 1023 points in the bin with the floor


@pytest.mark.parametrize("wide", WIDTHS)
@pytest.mark.parametrize("plan", PLANS)
def test_a_zone0_patch_from_which_rvpf_strips_a_wall(oracle, op, plan, wide):
    """list_order_ref.wall_cloud: the seed plane of R-VPF round 1 is vertical and the round removes the wall, whose heights become NaN
    marks in the z plane -- in both parts, among slots the later passes load and slots they do not."""
    p = pwpp_hip.default_params()
    clouds = [lo.wall_cloud(p, n_wall, n_column, 1600 + k)[0] for k, (n_wall, n_column) in enumerate(WALLS)]
    h = make_handle(plan, wide)
    h.estimate_ground_batch(clouds, mode=pwpp_hip.MODE_FRESH)
    for k, pts in enumerate(clouds):
        ref = ref_of(oracle, op, pts, wide)
        assert int((np.asarray(ref.nonground_cat) == 1).sum()) == WALLS[k][0]  # (round 1 removed the wall, all of it)
        assert_frame_equal(h, k, ref, len(pts))
    h.close()
