"""The oriented vehicle footprint (pwpp_footprint_grid) on a real MI355X, exactly equal -- pose rows and trajectory rows -- to the brute
force of tests/footprint_ref.py, for host and device memory (the cost bytes at odd addresses, the int32 images and the rows at their
minimum alignment, poisoned surroundings intact, inputs unwritten, a row array that was not given untouched) and for every value of the
option "footprint_path".  The shapes are the smallest that can go wrong: 1 x 1, 1 x 9 and 9 x 1 images; footprints wholly outside, over
each border and corner, p at negative ticks, PWPP_FOOT_OUTSIDE_BLOCKS on and off; windows of 1, 63, 64 and 65 cells and the largest,
181 x 181; the compass headings, multiples of (3, 4), random u; front != rear; a dist2 image with a clearance, unknown cells passable
and not, lethal 101; several blocked cells under one pose; 1, 63, 64, 65 and 4096 steps, 1 and 65 trajectories, one pose set and one
per frame; skipped poses first, in the middle, last and throughout; the first hit at step 0, at the last step and nowhere; reach given
and not, the last free pose outside the image; every choice of outputs; the chain costmap -> plan -> footprint in device memory.
References are computed once and shared."""
import functools

import numpy as np
import pytest

import footprint_ref as fr
import pwpp_hip
import reach_ref as rr

pytestmark = pytest.mark.gpu

PATHS = (0, 1, 2)
COMPASS = ((1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1))


def params_of(p):
    return pwpp_hip.ReachParams(p["base"], p["lethal"], p["unknown"], p["clearance2"], p["max_reach"], 0)


def foot_of(fp):
    return pwpp_hip.FootprintParams(fp["front"], fp["rear"], fp["half_width"], fp["flags"], (0, 0))


@pytest.fixture(scope="module")
def handle():
    return pwpp_hip.Handle()  # (no estimate call: the footprints need the handle's stream and buffer only)


def on_host(h, cost, p, fp, poses, dist2=None, reach=None, want=(True, True)):
    return h.footprint_grid(cost, params_of(p), foot_of(fp), poses, dist2=dist2, reach=reach, want_poses=want[0], want_trajectories=want[1])


def poisoned(torch, words, dtype):
    b = torch.full((words + 128,), -7, dtype=dtype, device="cuda")
    assert b.data_ptr() % 256 == 0
    return b


def on_device(h, cost, p, fp, poses, dist2=None, reach=None, want=(True, True)):
    """footprint_grid on device arrays: the cost bytes start 1 byte, every int32 array and both row arrays 4 bytes behind a 256-byte
    boundary -- their minimum; what surrounds them is poisoned and must survive, the inputs must not be written, and a row array that was
    not given stays as it was."""
    import torch
    c3 = cost.reshape((-1,) + cost.shape[-2:])
    frames, ny, nx = c3.shape
    cells = c3.size
    q = fr.as_poses(poses)
    n_traj, n_steps = q.shape[1], q.shape[2]
    n_poses, n_trajs = frames * n_traj * n_steps, frames * n_traj
    dc = poisoned(torch, cells, torch.int8)
    dd, dr = poisoned(torch, cells, torch.int32), poisoned(torch, cells, torch.int32)
    dp, dt = poisoned(torch, n_poses * 8, torch.int32), poisoned(torch, n_trajs * 8, torch.int32)
    dc[1:1 + cells] = torch.from_numpy(c3.reshape(-1).copy()).cuda()
    for given, buf in ((dist2, dd), (reach, dr)):
        if given is not None:
            buf[1:1 + cells] = torch.from_numpy(np.ascontiguousarray(given, np.int32).reshape(-1).copy()).cuda()
    torch.cuda.synchronize()
    h.footprint_grid_device(nx, ny, frames, dc.data_ptr() + 1, params_of(p), foot_of(fp), q, pose_rows_ptr=dp.data_ptr() + 4 if want[0] else 0,
                            traj_rows_ptr=dt.data_ptr() + 4 if want[1] else 0, dist2_ptr=dd.data_ptr() + 4 if dist2 is not None else 0,
                            reach_ptr=dr.data_ptr() + 4 if reach is not None else 0)
    h.synchronize()  # (complete after pwpp_synchronize: the copies below are on another stream)
    rc = dc.cpu().numpy()
    assert rc[0] == -7 and (rc[1 + cells:] == -7).all() and rc[1:1 + cells].tobytes() == c3.tobytes(), "the cost bytes were written"
    for given, buf, name in ((dist2, dd, "dist2"), (reach, dr, "reach")):
        raw = buf.cpu().numpy()
        if given is None:
            assert (raw == -7).all(), "a %s image that was not given was written" % name
        else:
            assert raw[0] == -7 and (raw[1 + cells:] == -7).all() and raw[1:1 + cells].tobytes() == np.ascontiguousarray(given, np.int32).tobytes(), name
    out = []
    for wanted, b, words, dtype, shape in ((want[0], dp, n_poses * 8, fr.POSE_ROW, (frames, n_traj, n_steps)), (want[1], dt, n_trajs * 8, fr.TRAJ_ROW, (frames, n_traj))):
        raw = b.cpu().numpy()
        if not wanted:
            assert (raw == -7).all(), "a row array that was not given was written"
            out.append(None)
            continue
        assert raw[0] == -7 and (raw[1 + words:] == -7).all(), "an element outside an array was written"
        out.append(raw[1:1 + words].copy().view(dtype).reshape(shape))
    return tuple(out)


def same(got, want, what, wanted=(True, True)):
    for name, g, w, on in zip(("pose rows", "trajectory rows"), got, want, wanted):
        if not on:
            assert g is None, "%s: %s nobody asked for" % (what, name)
            continue
        assert g.dtype == w.dtype and g.shape == w.shape, "%s: %s %r %r" % (what, name, g.shape, w.shape)
        if g.tobytes() != w.tobytes():
            bad = np.argwhere(g != w)
            assert False, "%s: %d %s differ, the first %s: %r, expected %r" % (what, len(bad), name, bad[0], g[tuple(bad[0])], w[tuple(bad[0])])


def everywhere(h, cost, p, fp, poses, want, what, dist2=None, reach=None, outputs=((True, True),)):
    """Every path, in host and in device memory, against `want`."""
    for path in PATHS:
        h.set_option("footprint_path", path)
        try:
            for o in outputs:
                same(on_host(h, cost, p, fp, poses, dist2, reach, o), want, "%s (host, path %d, outputs %s)" % (what, path, o), o)
                same(on_device(h, cost, p, fp, poses, dist2, reach, o), want, "%s (device, path %d, outputs %s)" % (what, path, o), o)
        finally:
            h.set_option("footprint_path", 0)


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def kinds(want):
    """(statuses present among the pose rows, whether trajectories with and without a hit are present)"""
    return set(np.unique(want[0]["status"]).tolist()), (want[1]["first_hit"] >= 0).any(), (want[1]["first_hit"] < 0).any()


def test_the_option_is_checked(handle):
    for v in (3, -1):
        with pytest.raises(Exception):
            handle.set_option("footprint_path", v)


# ---- the smallest images, every border and corner, p at negative ticks ------------------------------------------------------------
def sweep(nx, ny, step, margin):
    """Poses on a lattice from `margin` ticks before the image to `margin` behind it, the headings cycling through the compass, multiples of (3, 4) and (0, 0)."""
    us = list(COMPASS) + [(3, 4), (-4, 3), (300, -400), (0, 0)]
    q = [(x, y) for y in range(-margin, 16 * ny + margin + 1, step) for x in range(-margin, 16 * nx + margin + 1, step)]
    return np.array([[(x, y) + us[(i + j) % len(us)] for i, (x, y) in enumerate(q)] for j in range(3)], np.int32)


@functools.lru_cache(maxsize=None)
def small_case(nx, ny, flags):
    cost = rr.random_cost(2, ny, nx, 5 * nx + ny, lethal=0.15, unknown=0.15)
    reach = np.arange(2 * nx * ny, dtype=np.int32).reshape(2, ny, nx) * 3 + 1
    p = rr.params(base=2, unknown=30)
    fp = fr.foot_params(front=22, rear=7, half_width=9, flags=flags)
    poses = sweep(nx, ny, 13, 40)
    return frozen(cost, reach, poses) + (p, fp, fr.footprints(cost, p, fp, poses, reach=reach))


@pytest.mark.parametrize("flags", [0, fr.OUTSIDE_BLOCKS])
@pytest.mark.parametrize("shape", [(1, 1), (1, 9), (9, 1), (12, 10)], ids=lambda s: "%dx%d" % s)
def test_the_smallest_images_every_border_and_corner(handle, shape, flags):
    cost, reach, poses, p, fp, want = small_case(shape[0], shape[1], flags)
    rows = want[0]
    assert (rows["covered"] > 0).any() and ((rows["covered"] > 0) & (rows["outside"] == rows["covered"])).any(), "a footprint wholly outside"
    assert ((rows["outside"] > 0) & (rows["outside"] < rows["covered"])).any(), "a footprint over a border"
    assert (poses[..., 0] < 0).any() and (poses[..., 1] < 0).any()
    if flags:
        assert ((rows["outside"] > 0) & (rows["blocked"] == 0) & (rows["status"] == fr.HIT)).any()
    else:
        assert ((rows["outside"] > 0) & (rows["blocked"] == 0) & (rows["status"] == fr.FREE)).any()
        assert ((want[1]["last"] >= 0) & (want[1]["reach_last"] == fr.REACH_NONE)).any(), "a last free pose whose centre lies outside"
    everywhere(handle, cost, p, fp, poses, want, "%dx%d flags %d" % (shape + (flags,)), reach=reach)


# ---- windows of 1, 63, 64, 65 cells and the largest ---------------------------------------------------------------------------------
WINDOWS = {  # cells: (front, rear, half_width), (px, py, ux, uy) on a 24 x 24 image (a heading along an axis: the window is extent x width)
    0: ((0, 0, 0), (100, 100, 5, 0)),       # p on no centre: nothing is covered
    1: ((0, 0, 0), (104, 88, 0, -7)),       # p on a centre: that cell alone
    63: ((48, 48, 64), (200, 184, 1, 0)),   # 7 x 9
    64: ((56, 56, 56), (192, 192, 0, 1)),   # 8 x 8, p on a corner of four cells
    65: ((32, 32, 96), (184, 200, -2, 0)),  # 5 x 13
}


@functools.lru_cache(maxsize=None)
def window_case(cells, steps):
    cost = fr.random_images(1, 24, 24, 40 + cells)[0]
    ext, pose = WINDOWS[cells]
    fp = fr.foot_params(*ext)
    x, y, w, h = fr.window(fp, pose)
    assert w * h == cells, (w, h)
    # the same window on every step of a trajectory, shifted by whole cells; one step: path 2 deals the window to all 64 lanes, 5 steps: to 8
    poses = np.array([[(pose[0] + 16 * k, pose[1] - 16 * j, pose[2], pose[3]) for k in range(steps)] for j in range(2)], np.int32)
    p = rr.params(base=1, unknown=0)
    return frozen(cost, poses) + (p, fp, fr.footprints(cost, p, fp, poses))


@pytest.mark.parametrize("steps", [1, 5])
@pytest.mark.parametrize("cells", sorted(WINDOWS))
def test_windows_of_1_63_64_and_65_cells(handle, cells, steps):
    cost, poses, p, fp, want = window_case(cells, steps)
    assert (want[0]["covered"] == cells).all()  # (along an axis the window is the rectangle)
    everywhere(handle, cost, p, fp, poses, want, "window of %d cells" % cells)


@functools.lru_cache(maxsize=None)
def largest_case():
    cost = fr.random_images(1, 300, 300, 9, walls=12)
    dist2 = np.random.default_rng(5).integers(0, 4000, cost.shape).astype(np.int32)
    fp = fr.foot_params(1024, 1024, 1024)
    poses = np.array([[(2408, 2408, 1, 1), (2408, 2408, 3, 4), (8, 4792, 1024, -1), (2400, 2400, 0, -5), (-1000, 2408, -7, 2), (0, 0, 0, 0)]], np.int32)
    assert fr.window(fp, poses[0, 0])[2:] == (181, 181) and fr.window(fp, poses[0, 3])[2:] == (128, 128)  # (the bounding box of the square on its corner: 2048 sqrt(2) ticks)
    p = rr.params(base=3, unknown=-1, clearance2=9)
    return frozen(cost, dist2, poses) + (p, fp, fr.footprints(cost, p, fp, poses, dist2=dist2))


def test_the_largest_footprint_on_300_x_300_cells(handle):
    cost, dist2, poses, p, fp, want = largest_case()
    assert want[0]["covered"].max() > 16000 and (want[0]["outside"] > 0).any() and (want[0]["blocked"] > 1).any()
    everywhere(handle, cost, p, fp, poses, want, "largest", dist2=dist2)


# ---- random differential suites: headings, front != rear, the rules -------------------------------------------------------------------
def random_poses(rng, sets, n_traj, n_steps, nx, ny, margin, skipped=0.15):
    q = np.zeros((sets, n_traj, n_steps, 4), np.int32)
    q[..., 0] = rng.integers(-margin, 16 * nx + margin, q.shape[:3])
    q[..., 1] = rng.integers(-margin, 16 * ny + margin, q.shape[:3])
    kind = rng.integers(0, 3, q.shape[:3])
    compass = np.array(COMPASS)[rng.integers(0, 8, q.shape[:3])] * rng.integers(1, 1025, q.shape[:3])[..., None]
    three_four = np.array([(3, 4), (4, 3), (-3, 4), (4, -3), (-4, -3)])[rng.integers(0, 5, q.shape[:3])] * rng.integers(1, 205, q.shape[:3])[..., None]
    anyu = rng.integers(-1024, 1025, q.shape[:3] + (2,))
    q[..., 2:] = np.where(kind[..., None] == 0, compass, np.where(kind[..., None] == 1, three_four, anyu))
    q[rng.random(q.shape[:3]) < skipped, 2:] = 0
    return q


RULES = {
    "plain": (rr.params(base=2, unknown=-1), False),
    "unknown_passable": (rr.params(base=1, unknown=0), False),
    "no_lethal_value": (rr.params(base=7, lethal=101, unknown=100), False),
    "clearance": (rr.params(base=2, unknown=20, clearance2=8), True),
}


@functools.lru_cache(maxsize=None)
def random_case(rule, seed):
    p, with_d2 = RULES[rule]
    rng = np.random.default_rng(seed)
    frames, ny, nx = 3, 19, 23
    cost = fr.random_images(frames, ny, nx, seed)
    dist2 = rng.integers(0, 60, cost.shape).astype(np.int32) if with_d2 else None
    reach = rng.integers(0, 10 ** 6, cost.shape).astype(np.int32)
    fp = fr.foot_params(front=int(rng.integers(20, 50)), rear=int(rng.integers(0, 20)), half_width=int(rng.integers(5, 20)), flags=int(seed % 2))
    poses = random_poses(rng, frames if seed % 2 else 1, 8, 4, nx, ny, 10, skipped=0.25)
    arrays = frozen(cost, reach, poses) + (frozen(dist2)[0] if with_d2 else None,)
    return arrays + (p, fp, fr.footprints(cost, p, fp, poses, dist2=dist2, reach=reach))


@pytest.mark.parametrize("rule,seed", [("plain", 11), ("unknown_passable", 12), ("no_lethal_value", 14), ("clearance", 14), ("clearance", 15)])
def test_random_images_with_walls_and_unknown_cells(handle, rule, seed):
    cost, reach, poses, dist2, p, fp, want = random_case(rule, seed)
    statuses, with_hit, without_hit = kinds(want)
    assert statuses == {fr.FREE, fr.HIT, fr.SKIPPED} and with_hit and without_hit, "the suite misses a kind"
    assert fp["front"] != fp["rear"] and (want[0]["unknown"] > 0).any()
    several = want[0][want[0]["blocked"] > 1]
    assert several.size > 0, "several blocked cells under one pose: hit is the smallest index"
    if rule == "clearance":
        assert (want[0]["min_dist2"] < fr.BEYOND).any() and ((want[0]["blocked"] > 0) & (want[0]["min_dist2"] <= p["clearance2"])).any()
    everywhere(handle, cost, p, fp, poses, want, "random %s %d" % (rule, seed), dist2=dist2, reach=reach)


def test_hit_is_the_smallest_index_among_several_blocked_cells(handle):
    cost = np.zeros((8, 8), np.int8)
    cost[5, 2] = cost[3, 6] = cost[3, 4] = cost[6, 1] = 100
    fp, p = fr.foot_params(60, 60, 60), rr.params()
    poses = np.array([[(64, 64, 1, 1)], [(64, 64, 0, 1)], [(72, 88, 0, 1)]], np.int32)
    want = fr.footprints(cost, p, fp, poses)
    assert (want[0]["blocked"] >= 2).all() and (want[0]["hit"] == 3 * 8 + 4).all()
    everywhere(handle, cost, p, fp, poses, want, "several blocked cells")


# ---- trajectories: the steps, the skipped poses, where the first hit lies -------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def steps_case(n_steps, n_traj, slot_kind):
    """A small footprint walking to and fro over a 16 x 16 image with a few walls; slot_kind: the rule's E + W in ticks (windows of 1 to 7 x 7
    cells).  Path 2 takes min(64, n_steps rounded up to a power of two) steps a round."""
    frames = 2
    cost = fr.random_images(frames, 16, 16, 70 + n_steps % 97 + n_traj, walls=1)
    cost[:, 12:, :] = np.where(cost[:, 12:, :] >= 100, 0, cost[:, 12:, :])  # (a few rows without walls: trajectories without a hit)
    reach = (np.arange(cost.size, dtype=np.int32) * 7 % 1000).reshape(cost.shape)
    fp = fr.foot_params(front=slot_kind - slot_kind // 3, rear=slot_kind // 4, half_width=slot_kind // 3)
    k = np.arange(n_steps)
    poses = np.zeros((1, n_traj, n_steps, 4), np.int32)
    for j in range(n_traj):
        y = 200 + (j * 5) % 50 if j % 3 else 16 * (j % 11) + 8
        poses[0, j, :, 0] = 8 + (k * (3 + j % 5)) % 240
        poses[0, j, :, 1] = y
        poses[0, j, :, 2:] = COMPASS[j % 8]
        poses[0, j, (k + j) % 9 == 4, 2:] = 0  # skipped poses in between
    return frozen(cost, reach, poses) + (rr.params(base=1, unknown=5), fp, fr.footprints(cost, rr.params(base=1, unknown=5), fp, poses, reach=reach))


@pytest.mark.parametrize("n_steps,n_traj,slot_kind", [(1, 1, 3), (63, 2, 3), (64, 2, 3), (65, 65, 3), (65, 3, 12), (63, 3, 20), (65, 2, 36), (7, 65, 48), (4096, 2, 3), (4096, 1, 12)])
def test_steps_and_trajectories_at_the_edges_of_a_round(handle, n_steps, n_traj, slot_kind):
    cost, reach, poses, p, fp, want = steps_case(n_steps, n_traj, slot_kind)
    if n_steps > 1:
        assert (want[0]["status"] == fr.SKIPPED).any() and (want[0]["status"] == fr.FREE).any()
    outputs = ((True, True), (False, True)) if n_steps >= 63 else ((True, True),)  # (without pose rows path 2 ends a trajectory at its first hit)
    everywhere(handle, cost, p, fp, poses, want, "%d steps, %d trajectories, E + W %d" % (n_steps, n_traj, slot_kind), reach=reach, outputs=outputs)


@functools.lru_cache(maxsize=None)
def prefix_case():
    """20 x 8 cells, a wall in column 15; every trajectory drives along +x from cell 1, 16 ticks a step, 18 steps; a pose of step k reaches the wall from k = 12."""
    cost = np.zeros((2, 8, 20), np.int8)
    cost[0, :, 15] = 100
    cost[1, :, 15] = 100
    cost[1, 4, 15] = 0  # frame 1: a gate in the wall where the trajectories drive
    cost[:, 0, 0] = -1
    reach = np.arange(320, dtype=np.int32).reshape(2, 8, 20) + 1000
    fp = fr.foot_params(front=32, rear=8, half_width=6)
    n = 18
    base = np.array([(24 + 16 * k, 72, 1, 0) for k in range(n)], np.int32)

    def variant(skip=(), start_blocked=False, leave=False):
        q = base.copy()
        q[list(skip), 2:] = 0
        if start_blocked:
            q[0, :2] = (16 * 15 + 8, 72)
        if leave:
            q[:, 0] += 16 * 6  # drives out of the image behind the wall's column: the last poses' centres lie outside
        return q

    trajs = [variant(), variant(skip=(0, 1)), variant(skip=(5, 6, 7)), variant(skip=range(12, n)), variant(skip=range(n)), variant(start_blocked=True),
             variant(skip=range(13, n)), variant(skip=(11,)), variant(leave=True), variant(skip=(0,), leave=True)]
    poses = np.stack(trajs)[None]
    p = rr.params(base=4, unknown=-1)
    return frozen(cost, reach, poses) + (p, fp, fr.footprints(cost, p, fp, poses, reach=reach))


def test_skipped_poses_and_the_place_of_the_first_hit(handle):
    cost, reach, poses, p, fp, want = prefix_case()
    t0, t1 = want[1][0], want[1][1]
    assert t0["first_hit"].tolist()[:8] == [12, 12, 12, -1, -1, 0, 12, 12]
    assert t0["free_steps"].tolist()[:8] == [12, 10, 9, 12, 0, 0, 12, 11] and t0["last"].tolist()[:8] == [11, 11, 11, 11, -1, -1, 11, 10]
    assert t0["reach_last"][4] == fr.REACH_NONE and t0["reach_last"][0] == 1000 + 4 * 20 + 12 and t0["min_dist2"][0] == fr.BEYOND
    assert (t1["first_hit"][:5] == -1).all() and t1["free_steps"][0] == 18 and t1["last"][0] == 17   # through the gate: a hit nowhere
    assert t1["first_hit"][5] == -1 and t1["free_steps"][5] == 18                                      # (frame 1: the start stands in the gate)
    assert (t1["reach_last"][8:] == fr.REACH_NONE).all() and (t1["last"][8:] == 17).all(), "the last free pose lies outside the image"
    hit_last = poses[:, :7, :13].copy()   # 13 steps: the first hit at the last step
    want13 = fr.footprints(cost, p, fp, hit_last, reach=reach)
    assert want13[1]["first_hit"][0, 0] == 12 == hit_last.shape[2] - 1
    for outputs in (((True, True), (True, False), (False, True)),):
        everywhere(handle, cost, p, fp, poses, want, "prefixes", reach=reach, outputs=outputs)
        everywhere(handle, cost, p, fp, hit_last, want13, "a hit at the last step", reach=reach, outputs=outputs)
    no_reach = fr.footprints(cost, p, fp, poses)
    assert (no_reach[1]["reach_last"] == fr.REACH_NONE).all()
    everywhere(handle, cost, p, fp, poses, no_reach, "prefixes without reach", outputs=((True, True), (False, True)))


# ---- several frames, one pose set and one per frame ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def frames_case(per_frame):
    rng = np.random.default_rng(31 + per_frame)
    frames, ny, nx = 5, 11, 13
    cost = fr.random_images(frames, ny, nx, 90 + per_frame)
    assert len({cost[f].tobytes() for f in range(frames)}) == frames
    reach = rng.integers(0, 5000, cost.shape).astype(np.int32)
    fp = fr.foot_params(front=30, rear=10, half_width=11)
    poses = random_poses(rng, frames if per_frame else 1, 4, 6, nx, ny, 10, skipped=0.25)
    p = rr.params(base=2, unknown=10)
    return frozen(cost, reach, poses) + (p, fp, fr.footprints(cost, p, fp, poses, reach=reach))


@pytest.mark.parametrize("per_frame", [0, 1])
def test_several_frames_with_one_pose_set_and_with_one_per_frame(handle, per_frame):
    cost, reach, poses, p, fp, want = frames_case(per_frame)
    statuses, with_hit, without_hit = kinds(want)
    assert statuses == {fr.FREE, fr.HIT, fr.SKIPPED} and with_hit and without_hit
    if not per_frame:
        assert any(want[0][0].tobytes() != want[0][f].tobytes() for f in range(1, 5)), "the frames differ, so do their rows"
    everywhere(handle, cost, p, fp, poses, want, "frames, per_frame %d" % per_frame, reach=reach, outputs=((True, True), (True, False), (False, True)))


# ---- the chain in device memory: costmap -> plan -> footprint, no synchronise in between ----------------------------------------------
def test_costmap_plan_footprint_chain_in_device_memory(handle):
    import torch
    rng = np.random.default_rng(77)
    frames, ny, nx = 2, 24, 28
    occ = np.where(rng.random((frames, ny, nx)) < 0.05, 100, 0).astype(np.int8)
    occ[rng.random(occ.shape) < 0.05] = -1
    occ[:, 12, 14] = 0
    curve = pwpp_hip.costmap_curve(0.5, 0.6, 1.6, 2.0, 60)
    cm = pwpp_hip.CostmapParams(3, -1, -1, 101, (0, 0))  # occupancy and inflation, the distances its own
    p, fp = rr.params(base=2, unknown=40), fr.foot_params(front=40, rear=10, half_width=14)
    q = pwpp_hip.RouteParams(0, 0, 8, 0)
    src, starts = np.array([[14, 12]], np.int32), np.array([[1, 1], [26, 22]], np.int32)
    poses = random_poses(rng, 1, 6, 8, nx, ny, 8)
    # host memory: the same three calls
    cost_h = handle.costmap_grid(cm, occupancy=occ, curve=curve)
    plan_h = handle.plan_grid(cost_h, src, params_of(p), starts, q, want_field=True)
    reach_h = plan_h[3]
    want = fr.footprints(cost_h, p, fp, poses, reach=reach_h)
    statuses, with_hit, without_hit = kinds(want)
    assert statuses == {fr.FREE, fr.HIT, fr.SKIPPED} and with_hit and without_hit and (want[1]["reach_last"] != fr.REACH_NONE).any()
    same(on_host(handle, cost_h, p, fp, poses, reach=reach_h), want, "chain (host)")
    # device memory, enqueued back to back
    cells = occ.size
    d_occ = torch.from_numpy(occ.reshape(-1).copy()).cuda()
    d_cost = torch.full((cells,), -7, dtype=torch.int8, device="cuda")
    d_reach, d_routes = torch.full((cells,), -7, dtype=torch.int32, device="cuda"), torch.full((frames * 2 * 8,), -7, dtype=torch.int32, device="cuda")
    d_prow, d_trow = torch.full((frames * 6 * 8 * 8,), -7, dtype=torch.int32, device="cuda"), torch.full((frames * 6 * 8,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for path in PATHS:
        handle.set_option("footprint_path", path)
        try:
            handle.costmap_grid_device(nx, ny, frames, cm, d_cost.data_ptr(), occupancy_ptr=d_occ.data_ptr(), curve=curve)
            handle.plan_grid_device(nx, ny, frames, d_cost.data_ptr(), src, params_of(p), starts, q, d_routes.data_ptr(), reach_ptr=d_reach.data_ptr())
            handle.footprint_grid_device(nx, ny, frames, d_cost.data_ptr(), params_of(p), foot_of(fp), poses, pose_rows_ptr=d_prow.data_ptr(),
                                         traj_rows_ptr=d_trow.data_ptr(), reach_ptr=d_reach.data_ptr())
            handle.synchronize()
        finally:
            handle.set_option("footprint_path", 0)
        assert d_cost.cpu().numpy().tobytes() == cost_h.tobytes() and d_reach.cpu().numpy().tobytes() == reach_h.tobytes()
        got = (d_prow.cpu().numpy().view(fr.POSE_ROW).reshape(want[0].shape), d_trow.cpu().numpy().view(fr.TRAJ_ROW).reshape(want[1].shape))
        same(got, want, "chain (device, path %d)" % path)
        d_prow.fill_(-7), d_trow.fill_(-7)
        torch.cuda.synchronize()


def test_the_working_memory_is_counted_and_freed():
    h = pwpp_hip.Handle()
    before = h.workspace_bytes()
    cost, reach, poses, p, fp, want = frames_case(0)
    same(on_host(h, cost, p, fp, poses, reach=reach), want, "a fresh handle")
    grown = h.workspace_bytes()
    assert grown >= before + cost.size + 4 * reach.size + poses.size * 4 + want[0].size * 32 + want[1].size * 32
    h.trim_workspace()
    assert h.workspace_bytes() <= before
