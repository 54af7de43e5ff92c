"""The cluster tracks (pwpp_associate_grid, pwpp_track_obstacles) on a real MI355X: every comparison is exact equality of bytes with
the dictionaries of tests/tracks_ref.py, in host memory and in device memory, where every array starts 4 bytes behind a 256-byte
boundary -- its minimum alignment -- inside a poisoned buffer that must survive, and the inputs must come back unwritten.  There
is one path through the kernels, so no option to vary.  Three frames at most; references are computed once and shared."""
import ctypes
import functools

import numpy as np
import pytest

import pwpp_hip
import tracks_ref as tr
from test_gpu_obstacle_grid import _everything, small_cloud, three_frames

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -4
NAN = float("nan")
POISON = -77
SHAPES = [(1, 1), (1, 9), (9, 1), (7, 5), (63, 65), (64, 64), (65, 63), (96, 96)]  # (nx, ny) of the current grid
shape_ids = lambda s: "%dx%d" % s
NAMES = ("curr_links", "prev_links", "n_pairs", "id_curr", "next_id_out")


@pytest.fixture(scope="module")
def handle():
    return pwpp_hip.Handle()  # (no estimate call: pwpp_associate_grid needs the handle's stream and buffer only)


def g5(g):
    return (g["x0"], g["y0"], g["cell"], g["nx"], g["ny"])


def on_host(h, curr, prev, gc, gp, poses, gate, min_overlap, max_rows, max_pairs, id_prev=None, next_id=None):
    out = h.associate_grid(curr, prev, poses, g5(gc)[:3], g5(gp)[:3], gate, min_overlap, max_rows, max_pairs, id_prev=id_prev, next_id=next_id)
    return dict(zip(NAMES, out))


def placed(arr):
    """(tensor, address, elements): the int32 words of `arr` 4 bytes behind the start of a poisoned device buffer."""
    import torch
    words = np.ascontiguousarray(arr).view(np.int32).reshape(-1)
    t = torch.full((len(words) + 64,), POISON, dtype=torch.int32, device="cuda")
    assert t.data_ptr() % 256 == 0
    t[1:1 + len(words)] = torch.from_numpy(words.copy()).cuda()
    return t, t.data_ptr() + 4, len(words)


def taken(t, n, what, unwritten=None):
    raw = t.cpu().numpy()
    assert raw[0] == POISON and (raw[1 + n:] == POISON).all(), "an element outside %s was written" % what
    if unwritten is not None:
        assert raw[1:1 + n].tobytes() == np.ascontiguousarray(unwritten).tobytes(), "%s, an input, was written" % what
    return raw[1:1 + n].copy()


def on_device(h, curr, prev, gc, gp, poses, gate, min_overlap, max_rows, max_pairs, id_prev=None, next_id=None):
    import torch
    frames = curr.shape[0]
    with_ids = id_prev is not None
    dc, dp = placed(curr), placed(prev)
    links = [placed(np.full((frames, max_rows * 4), POISON, np.int32)) for _ in range(2)]
    dn = placed(np.full(frames, POISON, np.int32))
    ids_in = [placed(np.ascontiguousarray(id_prev, np.int32)), placed(np.ascontiguousarray(next_id, np.int32))] if with_ids else []
    ids_out = [placed(np.full((frames, max_rows), POISON, np.int32)), placed(np.full(frames, POISON, np.int32))] if with_ids else []
    torch.cuda.synchronize()
    id_ptrs = [ids_in[0][1], ids_in[1][1], ids_out[0][1], ids_out[1][1]] if with_ids else []
    h.associate_grid_device(g5(gc), g5(gp), frames, dc[1], dp[1], poses, gate, min_overlap, max_rows, max_pairs, links[0][1], links[1][1], dn[1], *id_ptrs)
    h.synchronize()  # (complete after pwpp_synchronize: the copies below are on another stream)
    taken(dc[0], dc[2], "curr", curr), taken(dp[0], dp[2], "prev", prev)
    out = dict(curr_links=taken(links[0][0], links[0][2], "curr_links").view(tr.LINK).reshape(frames, max_rows),
               prev_links=taken(links[1][0], links[1][2], "prev_links").view(tr.LINK).reshape(frames, max_rows), n_pairs=taken(dn[0], dn[2], "n_pairs"))
    if with_ids:
        taken(ids_in[0][0], ids_in[0][2], "id_prev", np.ascontiguousarray(id_prev, np.int32)), taken(ids_in[1][0], ids_in[1][2], "next_id", np.ascontiguousarray(next_id, np.int32))
        out.update(id_curr=taken(ids_out[0][0], ids_out[0][2], "id_curr").reshape(frames, max_rows), next_id_out=taken(ids_out[1][0], ids_out[1][2], "next_id_out"))
    return out


def same(got, want, what):
    assert set(got) == set(want), what
    for name in NAMES:
        if name not in want:
            continue
        g, w = np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name])
        assert g.dtype == w.dtype and g.shape == w.shape, "%s: %s" % (what, name)
        if g.tobytes() != w.tobytes():
            bad = np.argwhere(g != w)
            assert False, "%s: %d entries of %s differ, the first %s: %r, expected %r" % (what, len(bad), name, bad[0], g[tuple(bad[0])], w[tuple(bad[0])])


def everywhere(h, want, what, *args, **kw):
    """In host and in device memory against `want`."""
    same(on_host(h, *args, **kw), want, what + " (host)")
    same(on_device(h, *args, **kw), want, what + " (device)")


def frozen(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


def ids_for(frames, rows, seed, next_id=(100, 0x7FFFFFF0, 7)):
    rng = np.random.default_rng(seed)
    id_prev = rng.permutation(frames * rows).astype(np.int32).reshape(frames, rows) + 1000
    id_prev[rng.random((frames, rows)) < 0.2] = -1
    return id_prev, np.array(next_id[:frames], np.int32)


# ---- shapes: different sides and cell sizes for the two grids, a pose per frame ------------------------------------------------
@functools.lru_cache(maxsize=None)
def shape_case(nx, ny):
    k = SHAPES.index((nx, ny))
    gc = tr.grid(-0.25 * nx, -0.25 * ny, 0.5, nx, ny)
    nxp, nyp = nx // 2 + 2, ny // 2 + 1
    gp = tr.grid(-0.5 * nxp, -0.5 * nyp, 1.0, nxp, nyp)            # cells twice the current grid's
    rows = 8
    curr, prev = tr.blobs(3, ny, nx, 20 + k, n_blobs=8, max_rows=rows), tr.blobs(3, nyp, nxp, 60 + k, n_blobs=8, max_rows=rows)
    poses = np.array([tr.yaw(30, 0.3, -0.2), (1.0, 0.0, 1.0, 0.0, 1.0, -2.0), tr.yaw(90)], np.float64)
    id_prev, next_id = ids_for(3, rows, k)
    gate = k % 5
    want = tr.associate(curr, prev, gc, gp, poses, gate, 1 + k % 2, rows, 64, id_prev, next_id)
    frozen(curr, prev, poses, id_prev, next_id, *want.values())
    return gc, gp, curr, prev, poses, gate, 1 + k % 2, rows, id_prev, next_id, want


@pytest.mark.parametrize("shape", SHAPES, ids=shape_ids)
def test_shapes_against_the_reference(handle, shape):
    gc, gp, curr, prev, poses, gate, min_overlap, rows, id_prev, next_id, want = shape_case(*shape)
    everywhere(handle, want, shape_ids(shape), curr, prev, gc, gp, poses, gate, min_overlap, rows, 64, id_prev=id_prev, next_id=next_id)
    if shape[0] * shape[1] > 100:
        assert want["n_pairs"].min() >= 2 and want["n_pairs"].max() <= 64
    one = tr.associate(curr, prev, gc, gp, poses[:1], gate, min_overlap, rows, 64)                 # one pose for every frame, no ids, no n_pairs
    got = dict(zip(NAMES, handle.associate_grid(curr, prev, poses[0], g5(gc)[:3], g5(gp)[:3], gate, min_overlap, rows, 64, want_n_pairs=False)))
    assert got.pop("n_pairs") is None and one.pop("n_pairs") is not None
    same(got, one, shape_ids(shape) + ", one pose")


# ---- poses: each kind on its own, a previous grid whose cell is no power of two (the quotient as a division) -----------------------
POSES = {"identity": tr.IDENTITY, "shift": (1.0, 0.0, 1.5, 0.0, 1.0, -1.0), "quarter": tr.yaw(90), "yaw30": tr.yaw(30, 0.7, 0.1), "nan": (1.0, 0.0, NAN, 0.0, 1.0, 0.0),
         "inf": (float("inf"), 0.0, 0.0, 0.0, 1.0, 0.0), "far": (1.0, 0.0, 1e9, 0.0, 1.0, 0.0)}


@pytest.mark.parametrize("kind", sorted(POSES))
@pytest.mark.parametrize("cell_prev", [0.5, 0.3])
def test_each_kind_of_pose(handle, kind, cell_prev):
    nx, ny = 63, 65
    gc = tr.grid(-15.75, -16.25, 0.5, nx, ny)
    gp = tr.grid(-15.75, -16.25, cell_prev, nx if cell_prev == 0.5 else 105, ny if cell_prev == 0.5 else 108)
    curr, prev = tr.blobs(1, ny, nx, 5), tr.blobs(1, gp["ny"], gp["nx"], 5 if cell_prev == 0.5 else 6)
    id_prev, next_id = ids_for(1, 8, 3)
    want = tr.associate(curr, prev, gc, gp, [POSES[kind]], 1, 1, 8, 64, id_prev, next_id)
    everywhere(handle, want, kind, curr, prev, gc, gp, [POSES[kind]], 1, 1, 8, 64, id_prev=id_prev, next_id=next_id)
    existing = int((want["curr_links"]["cells"] > 0).sum())
    if kind in ("nan", "inf", "far"):   # no votes: no links, every existing row fresh
        assert want["n_pairs"][0] == 0 and (want["curr_links"]["links"] == 0).all() and (want["curr_links"]["other"] == -1).all()
        assert sorted(want["id_curr"][want["id_curr"] >= 0].tolist()) == list(range(100, 100 + existing)) and want["next_id_out"][0] == 100 + existing
    else:
        assert want["n_pairs"][0] >= 3
    if kind == "identity" and cell_prev == 0.5:
        for b in range(8):
            cells = int((curr == b).sum())
            assert tuple(want["curr_links"][0, b]) == ((b, cells, cells, 1) if cells else (-1, 0, 0, 0))


# ---- the gate ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gate", range(5))
def test_the_gate_at_the_border_on_ties_and_over_an_unlabelled_cell(handle, gate):
    n = 11
    g = tr.grid(0.0, 0.0, 1.0, n, n)
    prev = np.full((1, n, n), -1, np.int32)
    prev[0, 0, 0], prev[0, n - 1, n - 1], prev[0, 0, n - 1] = 0, 1, 2        # the corners: windows clipped by the border
    prev[0, 5, 5 - max(gate, 1)], prev[0, 5, 5 + max(gate, 1)] = 4, 3         # equidistant from (5, 5), itself unlabelled: the smaller index wins
    prev[0, 5 - max(gate, 1), 5] = 5                                          # as near, a smaller index still
    curr = np.full((1, n, n), -1, np.int32)
    curr[0, 0:5, 0:5], curr[0, n - 4:, n - 4:], curr[0, 1:4, n - 4:n - 1], curr[0, 5, 5] = 0, 1, 2, 3
    want = tr.associate(curr, prev, g, g, [tr.IDENTITY], gate, 1, 6, 16)
    everywhere(handle, want, "gate %d" % gate, curr, prev, g, g, [tr.IDENTITY], gate, 1, 6, 16)
    assert tuple(want["curr_links"][0, 3]) == ((-1, 0, 1, 0) if gate == 0 else (5, 1, 1, 1))
    assert want["curr_links"][0, 0]["overlap"] >= 1 and want["curr_links"][0, 1]["overlap"] >= 1 and (want["curr_links"][0, 2]["overlap"] > 0) == (gate > 0)


# ---- ties, labels outside the rows, contention ------------------------------------------------------------------------------------
def test_ties_go_to_the_smaller_label_on_both_sides(handle):
    g = tr.grid(0.0, 0.0, 1.0, 8, 4)
    prev = np.full((1, 4, 8), -1, np.int32)
    curr = np.full((1, 4, 8), -1, np.int32)
    prev[0, 0, 0:2], prev[0, 0, 2:4], curr[0, 0, 0:4] = 5, 2, 1                # two previous rows under one current row, two cells each
    curr[0, 2, 0:3], curr[0, 2, 3:6], prev[0, 2, 0:6] = 4, 3, 0                # two current rows over one previous row, three cells each
    want = tr.associate(curr, prev, g, g, [tr.IDENTITY], 0, 1, 6, 8)
    everywhere(handle, want, "ties", curr, prev, g, g, [tr.IDENTITY], 0, 1, 6, 8)
    assert tuple(want["curr_links"][0, 1]) == (2, 2, 4, 2) and tuple(want["prev_links"][0, 0]) == (3, 3, 6, 2) and want["n_pairs"][0] == 4


def test_labels_outside_the_rows_count_as_unlabelled_on_both_sides(handle):
    rows = 4
    g = tr.grid(0.0, 0.0, 1.0, 6, 2)
    values = np.array([-1, rows - 1, rows, 2 ** 31 - 1, -2 ** 31, 0], np.int32)
    curr = np.stack([values, values])[None]
    prev = np.stack([np.full(6, rows - 1, np.int32), values])[None]
    want = tr.associate(curr, prev, g, g, [tr.IDENTITY], 0, 1, rows, 8)
    everywhere(handle, want, "labels", curr, prev, g, g, [tr.IDENTITY], 0, 1, rows, 8)
    assert want["n_pairs"][0] == 3 and tuple(want["curr_links"][0, rows - 1]) == (rows - 1, 2, 2, 1) and tuple(want["prev_links"][0, rows - 1]) == (rows - 1, 2, 7, 2)
    swapped = tr.associate(prev, curr, g, g, [tr.IDENTITY], 0, 1, rows, 8)
    everywhere(handle, swapped, "labels, the sides swapped", prev, curr, g, g, [tr.IDENTITY], 0, 1, rows, 8)


def test_one_cluster_over_every_cell_is_one_pair(handle):
    n = 96
    g = tr.grid(-24.0, -24.0, 0.5, n, n)
    img = np.zeros((1, n, n), np.int32)
    want = tr.associate(img, img, g, g, [tr.IDENTITY], 0, 1, 1, 1, [[41]], [9])
    everywhere(handle, want, "one cluster", img, img.copy(), g, g, [tr.IDENTITY], 0, 1, 1, 1, id_prev=[[41]], next_id=[9])
    assert tuple(want["curr_links"][0, 0]) == (0, n * n, n * n, 1) and want["n_pairs"][0] == 1 and want["id_curr"][0, 0] == 41


# ---- the table at its limits ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def every_cell_its_own_label():
    n = 64
    img = np.arange(n * n, dtype=np.int32).reshape(1, n, n)
    g = tr.grid(0.0, 0.0, 1.0, n, n)
    pairs = int(tr.associate(img, img, g, g, [(1.0, 0.0, 1.0, 0.0, 1.0, 0.0)], 0, 1, n * n, 2 * n * n)["n_pairs"][0])
    img.setflags(write=False)
    return img, g, pairs


@pytest.mark.parametrize("room", ["exact", "one_fewer", "twice"])
def test_the_table_exactly_full_one_short_and_half_empty(handle, room):
    img, g, pairs = every_cell_its_own_label()
    rows = img.size
    assert pairs == 64 * 63                                              # shifted by one cell: the first column has no previous cell
    pose = (1.0, 0.0, 1.0, 0.0, 1.0, 0.0)
    max_pairs = {"exact": pairs, "one_fewer": pairs - 1, "twice": 2 * pairs}[room]
    id_prev, next_id = np.arange(rows, dtype=np.int32)[None] + 7, np.array([0x7FFFFFF0], np.int32)
    want = tr.associate(img, img, g, g, [pose], 0, 1, rows, max_pairs, id_prev, next_id)
    everywhere(handle, want, room, img, img.copy(), g, g, [pose], 0, 1, rows, max_pairs, id_prev=id_prev, next_id=next_id)
    if room == "one_fewer":
        assert want["n_pairs"][0] == max_pairs + 1 and (want["curr_links"]["other"] == -2).all() and (want["prev_links"]["other"] == -2).all()
        assert (want["curr_links"]["cells"] == 1).all() and (want["curr_links"]["links"] == 0).all() and (want["curr_links"]["overlap"] == 0).all()
        assert want["id_curr"][0, 16] == 0 and want["id_curr"][0, 15] == 0x7FFFFFFF      # every row fresh, across the wrap
    else:
        assert want["n_pairs"][0] == pairs and (want["curr_links"]["other"][0].reshape(64, 64)[:, 1:] == img[0, :, :-1]).all()


# ---- merge and split, the id rule ---------------------------------------------------------------------------------------------------
def test_merge_split_the_mutual_best_min_overlap_and_the_wrap(handle):
    g = tr.grid(0.0, 0.0, 1.0, 12, 6)
    prev = np.full((1, 6, 12), -1, np.int32)
    curr = np.full((1, 6, 12), -1, np.int32)
    prev[0, 0, 0:3], prev[0, 0, 3:5], curr[0, 0, 0:5] = 0, 1, 0                # a merge: rows 0 (3 cells) and 1 (2 cells) under current row 0
    prev[0, 2, 0:7], curr[0, 2, 0:3], curr[0, 2, 3:7] = 2, 1, 2                # a split: row 2 under current rows 1 (3 cells) and 2 (4 cells)
    prev[0, 4, 0:4], curr[0, 4, 0:4] = 3, 3                                    # one to one; its id is -1
    curr[0, 5, 8:12] = 4                                                       # appears
    id_prev = np.array([[10, 11, 12, -1, 99, 98]], np.int32)
    for min_overlap, next_id in ((3, 0x7FFFFFF0), (4, 0x7FFFFFF0), (5, 0x7FFFFFFE)):
        want = tr.associate(curr, prev, g, g, [tr.IDENTITY], 0, min_overlap, 6, 16, id_prev, [next_id])
        everywhere(handle, want, "min_overlap %d" % min_overlap, curr, prev, g, g, [tr.IDENTITY], 0, min_overlap, 6, 16, id_prev=id_prev, next_id=[next_id])
        assert want["curr_links"][0, 0]["links"] == 2 and want["prev_links"][0, 2]["links"] == 2 and want["n_pairs"][0] == 5
        ids = want["id_curr"][0].tolist()
        if min_overlap == 3:      # row 0 continues 0 (overlap 3), row 2 continues 2 (overlap 4); row 1 is not row 2's best; row 3's partner has no id
            assert ids == [10, 0x7FFFFFF0, 12, 0x7FFFFFF1, 0x7FFFFFF2, -1] and want["next_id_out"][0] == 0x7FFFFFF3
        if min_overlap == 4:      # one above row 0's overlap
            assert ids == [0x7FFFFFF0, 0x7FFFFFF1, 12, 0x7FFFFFF2, 0x7FFFFFF3, -1]
        if min_overlap == 5:      # everything fresh, across the wrap
            assert ids == [0x7FFFFFFE, 0x7FFFFFFF, 0, 1, 2, -1] and want["next_id_out"][0] == 3
    L, z = handle._L, np.zeros(8, np.int32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    gg = pwpp_hip.GroundGrid(0.0, 0.0, 1.0, 12, 6, 0, 0)
    cl, pl = np.zeros(6, tr.LINK), np.zeros(6, tr.LINK)
    pose = np.array(tr.IDENTITY, np.float64)
    rc = L.pwpp_associate_grid(handle._h, ctypes.byref(gg), ctypes.byref(gg), 1, pwpp_hip.MEM_HOST, vp(curr), vp(prev), vp(pose), 1, 0, 1, 6, 16, vp(cl), vp(pl), None,
                               vp(id_prev), vp(z), None, vp(z))
    assert rc == E_ARG and b"null id_curr with other id arrays given" in L.pwpp_last_error()


def test_repeated_calls_give_the_same_bytes(handle):
    gc, gp, curr, prev, poses, gate, min_overlap, rows, id_prev, next_id, want = shape_case(65, 63)
    for i in range(3):
        same(on_host(handle, curr, prev, gc, gp, poses, gate, min_overlap, rows, 64, id_prev, next_id), want, "call %d" % i)
    for i in range(2):
        same(on_device(handle, curr, prev, gc, gp, poses, gate, min_overlap, rows, 64, id_prev, next_id), want, "device call %d" % i)


def test_three_steps_feed_the_ids_back(handle):
    """A cluster that moves one cell a step keeps its id; one that appears at step 2 gets the next one."""
    n, rows = 16, 4
    g = tr.grid(0.0, 0.0, 1.0, n, n)

    def frame(step):
        img = np.full((1, n, n), -1, np.int32)
        if step >= 2:
            img[0, 1:3, 10:13] = 0                 # the newcomer takes the smaller label: labels are per frame
        img[0, 8:11, 3 + step:6 + step] = 1 if step >= 2 else 0
        return img

    prev, id_prev, next_id = np.full((1, n, n), -1, np.int32), np.full((1, rows), -1, np.int32), np.array([50], np.int32)
    seen = []
    for step in range(4):
        curr = frame(step)
        want = tr.associate(curr, prev, g, g, [tr.IDENTITY], 0, 1, rows, 8, id_prev, next_id)
        everywhere(handle, want, "step %d" % step, curr, prev, g, g, [tr.IDENTITY], 0, 1, rows, 8, id_prev=id_prev, next_id=next_id)
        seen.append(want["id_curr"][0].tolist())
        prev, id_prev, next_id = curr, want["id_curr"], want["next_id_out"]
    assert seen == [[50, -1, -1, -1], [50, -1, -1, -1], [51, 50, -1, -1], [51, 50, -1, -1]] and next_id[0] == 52


# ---- pwpp_track_obstacles -------------------------------------------------------------------------------------------------------------
GRID = (-20.0, -20.0, 0.5, 80, 80)
BAND = (0.2, 2.5)
ROWS = 64


def check_chain(h, frames, poses, what):
    label, table, n = h.label_obstacles(*GRID, *BAND, min_count=1, connectivity=8, max_clusters=ROWS, frames=frames)
    prev = np.ascontiguousarray(np.roll(label, (1, -2), (1, 2)))     # what the scene looked like a step ago, for the test's purposes
    prev[:, :, -3:] = 2 ** 31 - 1
    id_prev, next_id = ids_for(frames, ROWS, 9, next_id=(5, 0x7FFFFFFA, 70))
    got = h.track_obstacles(*GRID, *BAND, prev, poses, max_clusters=ROWS, gate=2, min_overlap=2, max_pairs=4 * ROWS, id_prev=id_prev, next_id=next_id, frames=frames)
    assert got[0].tobytes() == label.tobytes() and got[2].tobytes() == n.tobytes(), what
    for f in range(frames):
        k = min(int(n[f]), ROWS)
        assert got[1][f, :k].tobytes() == table[f, :k].tobytes(), what
    g = tr.grid(*GRID)
    want = tr.associate(label, prev, g, g, poses, 2, 2, ROWS, 4 * ROWS, id_prev, next_id)
    same(dict(zip(NAMES, got[3:])), want, what + " against the restatement")
    same(on_host(h, label, prev, g, g, poses, 2, 2, ROWS, 4 * ROWS, id_prev, next_id), want, what + ": pwpp_associate_grid on those images")
    # device memory: the label image and every array of the association at their minimum alignment
    import torch
    dl, dp = placed(np.full(label.shape, POISON, np.int32)), placed(prev)
    links = [placed(np.full((frames, ROWS * 4), POISON, np.int32)) for _ in range(2)]
    dn, di, dx = placed(np.full(frames, POISON, np.int32)), placed(id_prev), placed(next_id)
    do, dy = placed(np.full((frames, ROWS), POISON, np.int32)), placed(np.full(frames, POISON, np.int32))
    dt = torch.zeros(frames * ROWS * 48, dtype=torch.uint8, device="cuda")   # the cluster table: 8-byte aligned
    torch.cuda.synchronize()
    h.track_obstacles_device(*GRID, *BAND, 1, 8, dl[1], dp[1], poses, 2, 2, ROWS, 4 * ROWS, links[0][1], links[1][1], dn[1], di[1], dx[1], do[1], dy[1], clusters_ptr=dt.data_ptr(),
                             frames=frames)
    h.synchronize()
    for f in range(frames):
        k = min(int(n[f]), ROWS)
        assert dt.cpu().numpy()[f * ROWS * 48:(f * ROWS + k) * 48].tobytes() == table[f, :k].tobytes(), what
    assert taken(dl[0], dl[2], "label").tobytes() == label.tobytes(), what
    taken(dp[0], dp[2], "prev_label", prev), taken(di[0], di[2], "id_prev", id_prev), taken(dx[0], dx[2], "next_id", next_id)
    dev = dict(curr_links=taken(links[0][0], links[0][2], "curr_links").view(tr.LINK).reshape(frames, ROWS),
               prev_links=taken(links[1][0], links[1][2], "prev_links").view(tr.LINK).reshape(frames, ROWS), n_pairs=taken(dn[0], dn[2], "n_pairs"),
               id_curr=taken(do[0], do[2], "id_curr").reshape(frames, ROWS), next_id_out=taken(dy[0], dy[2], "next_id_out"))
    same(dev, want, what + " (device)")
    return want, n


def test_track_obstacles_is_label_obstacles_plus_associate_grid():
    h = pwpp_hip.Handle()
    L = h._L
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    g = pwpp_hip.GroundGrid(*GRID, 0, 0)
    label, prev, n = np.zeros(6400, np.int32), np.zeros(6400, np.int32), np.zeros(1, np.int32)
    table, cl, pl = np.zeros(ROWS, pwpp_hip.OBSTACLE_CLUSTER_DTYPE), np.zeros(ROWS, tr.LINK), np.zeros(ROWS, tr.LINK)
    pose = np.array(tr.IDENTITY, np.float64)

    def raw(gate=0, max_pairs=8):
        return L.pwpp_track_obstacles(h._h, ctypes.byref(g), 0.2, 2.5, 1, 8, 0, 1, pwpp_hip.MEM_HOST, vp(label), None, None, vp(table), vp(n), ROWS, None, vp(prev),
                                      vp(pose), 1, gate, 1, max_pairs, vp(cl), vp(pl), None, None, None, None, None)

    assert raw() == E_STATE and raw(gate=9) == E_STATE       # the labelling's checks, the state among them, come first
    h.set_labels(True)  # (_everything reads them)
    h.estimate_ground(small_cloud(5))
    before = _everything(h, 1)
    assert raw(gate=9) == E_ARG and b"gate 9" in L.pwpp_last_error()
    assert raw(max_pairs=0) == E_ARG and b"max_pairs 0" in L.pwpp_last_error()
    want, n_clusters = check_chain(h, 1, [tr.IDENTITY], "one frame")
    assert n_clusters[0] >= 5 and want["n_pairs"][0] >= 5 and (want["curr_links"]["links"] > 0).sum() >= 5
    assert _everything(h, 1) == before, "the association changed the results of the call it reads"


def test_track_obstacles_on_three_frames_of_a_batch():
    h = pwpp_hip.Handle()
    h.estimate_ground_batch(three_frames(), mode=pwpp_hip.MODE_FRESH)  # a 16-beam scan, an empty frame, a frame that is all unref
    poses = [tr.IDENTITY, tr.yaw(30), (1.0, 0.0, 0.5, 0.0, 1.0, 0.0)]
    want, n_clusters = check_chain(h, 3, poses, "three frames")
    assert n_clusters[0] >= 5 and n_clusters[1] == 0 and want["n_pairs"][1] == 0 and (want["id_curr"][1] == -1).all() and want["next_id_out"][1] == 0x7FFFFFFA


# ---- workspace ------------------------------------------------------------------------------------------------------------------
def test_workspace_and_that_nothing_else_moves():
    gc, gp, curr, prev, poses, gate, min_overlap, rows, id_prev, next_id, want = shape_case(96, 96)
    h = pwpp_hip.Handle()
    empty = h.workspace_bytes()
    same(on_host(h, curr, prev, gc, gp, poses, gate, min_overlap, rows, 64, id_prev, next_id), want, "before any estimate call")
    assert h.workspace_bytes() >= empty + 3 * 64 * 2 * 12 + 3 * rows * 16 + curr.nbytes + prev.nbytes, "the cluster buffer is not counted"
    h.trim_workspace()
    assert h.workspace_bytes() == empty, "pwpp_trim_workspace did not free the cluster buffer"
    # with the feature unused nothing is allocated; with it used nothing of the estimate path moves
    a, b = pwpp_hip.Handle(), pwpp_hip.Handle()
    frames = three_frames()
    for w in (a, b):
        w.set_labels(True)
        w.set_order(pwpp_hip.ORDER_CLOUD)  # (a deterministic order of the index lists: two calls are compared below)
        w.estimate_ground_batch(frames, mode=pwpp_hip.MODE_FRESH)
    untouched = a.workspace_bytes()
    assert untouched == b.workspace_bytes()
    before, t_before = _everything(b, 3), b.time_us()
    same(on_host(b, curr, prev, gc, gp, poses, gate, min_overlap, rows, 64, id_prev, next_id), want, "after an estimate call")
    assert b.workspace_bytes() >= untouched + 3 * 64 * 2 * 12 + 3 * rows * 16 + curr.nbytes + prev.nbytes   # the tables, the rows' words, the staged images
    assert a.workspace_bytes() == untouched, "a handle that never associated grew"
    assert _everything(b, 3) == before and b.time_us() == t_before, "the association changed the results of the call before it"
    for w in (a, b):
        w.estimate_ground_batch(frames, mode=pwpp_hip.MODE_FRESH)
    assert _everything(b, 3) == _everything(a, 3), "an estimate call after an association differs from one without"
    b.trim_workspace()
    a.trim_workspace()
    assert a.workspace_bytes() == b.workspace_bytes()


# ---- bindings -----------------------------------------------------------------------------------------------------------------
def test_pybind_module_keeps_the_tracks_between_calls_and_agrees_with_the_ctypes_handle():
    import pypatchworkpp
    pp = pypatchworkpp.patchworkpp(pypatchworkpp.Parameters())
    h = pwpp_hip.Handle()
    with pytest.raises(RuntimeError):
        pp.trackObstacleClusters(*GRID, *BAND)  # no frame yet
    g = tr.grid(*GRID)
    rows, gate, min_overlap = 4, 1, 1                # fewer rows than clusters: the cells of the others count as unlabelled
    prev, ids, nxt = np.full((1, 80, 80), -1, np.int32), np.full((1, rows), -1, np.int32), np.zeros(1, np.int32)
    pose = (1.0, 0.0, 0.25, 0.0, 1.0, 0.0)
    for step, seed in enumerate((5, 5, 6)):          # the same scan twice, then another
        pts = small_cloud(seed)
        pp.estimateGround(pts)
        h.estimate_ground(pts)
        label, table, cl, pl, got_ids, count, pairs = pp.trackObstacleClusters(*GRID, *BAND, pose=pose, max_clusters=rows, gate=gate, min_overlap=min_overlap)
        want = h.track_obstacles(*GRID, *BAND, prev, pose, max_clusters=rows, gate=gate, min_overlap=min_overlap, max_pairs=4 * rows, id_prev=ids, next_id=nxt)
        k = min(int(want[2][0]), rows)
        assert count == want[2][0] and count >= 5 and label.shape == (80, 80) and label.tobytes() == want[0].tobytes()
        assert table.tobytes() == want[1][0, :k].tobytes() and cl.tobytes() == want[3][0, :k].tobytes() and pl.tobytes() == want[4][0].tobytes()
        assert got_ids.tobytes() == want[6][0, :k].tobytes() and pairs == want[5][0]
        ref = tr.associate(want[0], prev, g, g, [pose], gate, min_overlap, rows, 4 * rows, ids, nxt)
        same(dict(zip(NAMES, want[3:])), ref, "step %d" % step)
        if step == 0:
            assert pairs == 0 and got_ids.tolist() == list(range(rows))
        if step == 1:                                # the same scene, moved by half a cell under gate 1: most clusters keep their ids
            assert pairs >= rows // 2 and (got_ids < rows).sum() >= rows // 2
        prev, ids, nxt = want[0], want[6], want[7]
    pp.resetObstacleTracks()
    pp.estimateGround(small_cloud(6))
    assert pp.trackObstacleClusters(*GRID, *BAND, max_clusters=rows)[4].tolist() == list(range(rows))   # afresh: no previous image, ids from 0
