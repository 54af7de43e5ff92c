"""The map evidence (pwpp_evidence_grid, pwpp_evidence_obstacles) on a real MI355X: every comparison is exact equality of bytes with
the dictionaries of tests/evidence_ref.py, in host memory and in device memory, where every array starts at its minimum alignment
-- rows 8, label 4, map 2, bytes 1 -- behind a 256-byte boundary inside a poisoned buffer that must survive, and the inputs must
come back unwritten; at the option "evidence_path" 0, 1 and 2.  Three frames at most; references are computed once and shared."""
import ctypes
import functools

import numpy as np
import pytest

import evidence_ref as er
import occupancy_fusion_ref as fr
import pwpp_hip
from test_gpu_obstacle_grid import _everything, small_cloud, three_frames

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -4
NAN = float("nan")
POISON = 0xB3
SHAPES = [(1, 1), (1, 9), (9, 1), (7, 5), (63, 65), (64, 64), (65, 63), (96, 96)]  # (nx, ny)
PATHS = (0, 1, 2)
LDS_ROWS = pwpp_hip.EVID_LDS_ROWS


@pytest.fixture(scope="module")
def handle():
    return pwpp_hip.Handle()  # (no estimate call: pwpp_evidence_grid needs the handle's stream and buffer only)


def fmap_of(m):
    return pwpp_hip.FusionMap(m["x0"], m["y0"], m["cell"], m["nx"], m["ny"], 40, 20, -350, 350, m["occupied_at"], m["free_at"])


def yaw(degrees, tx=0.0, ty=0.0):
    return fr.rigid(np.deg2rad(degrees), tx, ty)


def case(g, m, label, poses, maps, rule, max_rows, occ=None, mof=None):
    """A problem and, computed once, what the restatement gives for it: rows, the class image, the masked bytes."""
    c = dict(g=g, m=m, label=np.ascontiguousarray(label, np.int32), poses=np.asarray(poses, np.float64).reshape(-1, 6), maps=np.ascontiguousarray(maps, np.int16),
             rule=rule, max_rows=max_rows, occ=None if occ is None else np.ascontiguousarray(occ, np.int8), mof=mof)
    c["rows"], c["cls"], c["masked"] = er.evidence_grid(g, c["label"], c["occ"], c["poses"], mof, m, c["maps"], rule, max_rows)
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


def rule4(r):
    return (r["gate"], r["min_cells"], r["moving_share"], r["static_share"])


def on_host(h, c, want_class, with_occ, in_place):
    occ = c["occ"] if with_occ else None
    out = h.evidence_grid(c["label"], (c["g"]["x0"], c["g"]["y0"], c["g"]["cell"]), c["poses"], fmap_of(c["m"]), c["maps"], rule4(c["rule"]), c["max_rows"], occupancy=occ,
                          map_of_frame=c["mof"], want_class=want_class, in_place=in_place)
    out = out if isinstance(out, tuple) else (out,)
    return dict(rows=out[0], cls=out[1] if want_class else None, masked=out[-1] if with_occ else None)


def placed(arr, offset):
    """(tensor, address, bytes, offset): the bytes of `arr`, `offset` bytes behind the start of a poisoned device buffer."""
    import torch
    raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
    t = torch.full((len(raw) + 256,), POISON, dtype=torch.uint8, device="cuda")
    assert t.data_ptr() % 256 == 0
    t[offset:offset + len(raw)] = torch.from_numpy(raw.copy()).cuda()
    return t, t.data_ptr() + offset, len(raw), offset


def taken(p, what, unwritten=None):
    t, _, n, offset = p
    raw = t.cpu().numpy()
    assert (raw[:offset] == POISON).all() and (raw[offset + n:] == POISON).all(), "a byte outside %s was written" % what
    if unwritten is not None:
        assert raw[offset:offset + n].tobytes() == np.ascontiguousarray(unwritten).tobytes(), "%s, an input, was written" % what
    return raw[offset:offset + n].copy()


def on_device(h, c, want_class, with_occ, in_place):
    import torch
    frames, shape = c["label"].shape[0], c["label"].shape
    dl, dm = placed(c["label"], 4), placed(c["maps"], 2)
    dr = placed(np.full((frames, c["max_rows"] * 32), POISON, np.uint8), 8)
    dc = placed(np.full(shape, POISON, np.uint8), 1) if want_class else None
    di = placed(c["occ"], 1) if with_occ else None
    do = (di if in_place else placed(np.full(shape, POISON, np.uint8), 3)) if with_occ else None
    torch.cuda.synchronize()
    h.evidence_grid_device((c["g"]["x0"], c["g"]["y0"], c["g"]["cell"]), c["g"]["nx"], c["g"]["ny"], frames, dl[1], c["poses"], fmap_of(c["m"]), c["maps"].shape[0], dm[1],
                           rule4(c["rule"]), c["max_rows"], dr[1], dc[1] if dc else 0, di[1] if di else 0, do[1] if do else 0, map_of_frame=c["mof"])
    h.synchronize()  # (complete after pwpp_synchronize: the copies below are on another stream)
    taken(dl, "label", c["label"]), taken(dm, "map", c["maps"])
    if with_occ and not in_place:
        taken(di, "occupancy_in", c["occ"])
    return dict(rows=taken(dr, "rows").view(er.EVIDENCE).reshape(frames, c["max_rows"]), cls=taken(dc, "cell_class").view(np.int8).reshape(shape) if dc else None,
                masked=taken(do, "occupancy_out").view(np.int8).reshape(shape) if do else None)


def same(got, c, what):
    for name in ("rows", "cls", "masked"):
        if got[name] is None:
            continue
        g, w = np.ascontiguousarray(got[name]), c[name]
        assert g.dtype == w.dtype and g.shape == w.shape, "%s: %s" % (what, name)
        if g.tobytes() != w.tobytes():
            bad = np.argwhere(g != w)
            assert False, "%s: %d entries of %s differ, the first %s: %r, expected %r" % (what, len(bad), name, bad[0], g[tuple(bad[0])], w[tuple(bad[0])])


def everywhere(h, c, what, want_class=True, with_occ=None, in_place=False, paths=PATHS):
    """At every value of the option, in host and in device memory, against the restatement."""
    with_occ = c["occ"] is not None if with_occ is None else with_occ
    try:
        for path in paths:
            h.set_option("evidence_path", path)
            same(on_host(h, c, want_class, with_occ, in_place), c, "%s (host, path %d)" % (what, path))
            same(on_device(h, c, want_class, with_occ, in_place), c, "%s (device, path %d)" % (what, path))
    finally:
        h.set_option("evidence_path", 0)


def noise_labels(frames, ny, nx, seed, max_rows, share=0.6):
    """Rectangles of a few rows and noise over all rows, on a ground of -1."""
    rng = np.random.default_rng(seed)
    out = np.where(rng.random((frames, ny, nx)) < share * 0.3, rng.integers(0, max_rows, (frames, ny, nx)), -1).astype(np.int32)
    for f in range(frames):
        for r in range(min(max_rows, 6)):
            y, x = int(rng.integers(0, ny)), int(rng.integers(0, nx))
            out[f, y:y + int(rng.integers(1, 12)), x:x + int(rng.integers(1, 12))] = r
    return out


# ---- shapes: the grid's and the map's sides taken independently, different cell sizes, a pose and a map per frame ------------------
PAIRS = [(SHAPES[k], SHAPES[(3 * k + 5) % 8]) for k in range(8)] + [(SHAPES[k], SHAPES[(5 * k + 2) % 8]) for k in range(8)]
pair_ids = lambda p: "%dx%d_on_%dx%d" % (p[0] + p[1])


@functools.lru_cache(maxsize=None)
def shape_case(shape, map_shape):
    k = PAIRS.index((shape, map_shape))
    (nx, ny), (NX, NY) = shape, map_shape
    CELL = 0.25 if k % 2 else 0.3  # a power of two: the product with the reciprocal; not one: the quotient
    g = er.grid(-0.25 * nx, -0.25 * ny, 0.5, nx, ny)
    m = er.fusion_map(-0.5 * CELL * NX + 0.1, -0.5 * CELL * NY - 0.2, CELL, NX, NY, 100, -60)
    rows = 8
    rng = np.random.default_rng(40 + k)
    maps = rng.integers(-300, 300, (3, NY, NX)).astype(np.int16)
    poses = [yaw(30, 0.3, -0.2), (1.0, 0.0, 1.0, 0.0, 1.0, -2.0), yaw(90)]
    occ = fr.random_occupancy(3, ny, nx, 70 + k)
    return case(g, m, noise_labels(3, ny, nx, 20 + k, rows), poses, maps, er.rule(k % 5, 1 + k % 3, 120, 90), rows, occ=occ)


@pytest.mark.parametrize("pair", PAIRS, ids=pair_ids)
def test_shapes_against_the_reference(handle, pair):
    c = shape_case(*pair)
    everywhere(handle, c, pair_ids(pair))
    if min(pair[0]) > 60 and min(pair[1]) > 60:
        assert c["rows"]["landed"].sum() > 500


# ---- the gate: landings on the map's border and corners, the window clipped on each side ------------------------------------------
@functools.lru_cache(maxsize=None)
def gate_case(gate):
    n = 11
    g, m = er.grid(0.0, 0.0, 1.0, n, n), er.fusion_map(0.0, 0.0, 1.0, n, n, 100, -60)
    label = np.full((1, n, n), -1, np.int32)
    label[0, 0, 0], label[0, 0, n - 1], label[0, n - 1, 0], label[0, n - 1, n - 1] = 0, 1, 2, 3   # the corners
    label[0, 0, 3:8], label[0, n - 1, 3:8], label[0, 3:8, 0], label[0, 3:8, n - 1] = 4, 5, 6, 7   # the four borders
    label[0, 5, 5] = 8
    maps = np.full((1, n, n), -200, np.int16)
    maps[0, 4, 4], maps[0, 1, 1], maps[0, n - 2, n - 3], maps[0, 5, 5 + max(gate, 1)] = 150, 120, 300, -10
    return case(g, m, label, [er.IDENTITY], maps, er.rule(gate, 1, 256, 256), 9, occ=np.full((1, n, n), 100, np.int8))


@pytest.mark.parametrize("gate", range(5))
def test_the_gate_at_the_border_and_the_corners(handle, gate):
    c = gate_case(gate)
    everywhere(handle, c, "gate %d" % gate)
    assert c["rows"][0, 0]["sum"] == (-200, 120, 120, 120, 150)[gate] and c["rows"][0, 0]["verdict"] == (er.STATIC if gate >= 1 else er.MOVING)
    assert c["rows"][0, 8]["sum"] == (-200, 150, 150, 150, 300)[gate] and (c["rows"][0]["landed"] == c["rows"][0]["cells"]).all()


# ---- poses: yaw with unequal cells on both sides, both forms of the quotient, a NaN pose on one frame of three ---------------------
@functools.lru_cache(maxsize=None)
def pose_case(CELL):
    nx, ny = 63, 65
    g = er.grid(-15.75, -16.25, 0.5, nx, ny)
    m = er.fusion_map(-16.0, -15.0, CELL, 64 if CELL == 0.5 else 105, 64 if CELL == 0.5 else 99, 100, -60)
    rng = np.random.default_rng(8)
    maps = rng.integers(-300, 300, (1, m["ny"], m["nx"])).astype(np.int16)
    return {kind: case(g, m, noise_labels(3, ny, nx, 5, 8), poses, maps, er.rule(1, 2, 100, 100), 8)
            for kind, poses in (("yaw", [yaw(30, 0.7, 0.1), yaw(90), yaw(200, -1.0, 2.0)]), ("nan", [er.IDENTITY, (1.0, 0.0, NAN, 0.0, 1.0, 0.0), yaw(200)]),
                                ("one", [yaw(30)]), ("far", [(float("inf"), 0.0, 0.0, 0.0, 1.0, 0.0), (1.0, 0.0, 1e9, 0.0, 1.0, 0.0), (1.0, 0.0, 0.0, 0.0, 1.0, -3e5)]))}


@pytest.mark.parametrize("kind", ["yaw", "nan", "one", "far"])
@pytest.mark.parametrize("CELL", [0.5, 0.3])
def test_each_kind_of_pose(handle, kind, CELL):
    c = pose_case(CELL)[kind]
    everywhere(handle, c, "%s, CELL %g" % (kind, CELL), want_class=kind != "one")
    landed = c["rows"]["landed"].sum(axis=1)
    if kind == "yaw" or kind == "one":
        assert (landed > 200).all()
    if kind == "nan":
        assert landed[1] == 0 and landed[0] > 200 and landed[2] > 200 and c["rows"]["cells"][1].sum() > 200 and (c["cls"][1] == er.CELL_NONE).all()
    if kind == "far":
        assert (landed == 0).all() and (c["rows"]["verdict"][c["rows"]["cells"] > 0] == er.UNDECIDED).all()


# ---- the frames' maps: one shared, one per frame, explicit with a skipped frame ------------------------------------------------------
@functools.lru_cache(maxsize=None)
def maps_case(kind):
    g, m = er.grid(-3.5, -2.5, 0.5, 14, 10), er.fusion_map(-4.0, -3.0, 0.5, 16, 12, 100, -60)
    n_maps, mof = {"shared": (1, None), "per_frame": (3, None), "explicit": (2, [1, -1, 0]), "all_skipped": (1, [-1, -1, -1])}[kind]
    maps = np.random.default_rng(2).integers(-300, 300, (n_maps, 12, 16)).astype(np.int16)
    return case(g, m, noise_labels(3, 10, 14, 3, 5), [er.IDENTITY], maps, er.rule(1, 1, 128, 128), 5, occ=fr.random_occupancy(3, 10, 14, 4), mof=mof)


@pytest.mark.parametrize("kind", ["shared", "per_frame", "explicit", "all_skipped"])
def test_map_of_frame(handle, kind):
    c = maps_case(kind)
    everywhere(handle, c, kind)
    if kind == "explicit":
        assert c["rows"]["landed"][1].sum() == 0 and c["rows"]["cells"][1].sum() > 0 and c["masked"][1].tobytes() == c["occ"][1].tobytes()
    if kind == "per_frame":
        assert c["rows"][0].tobytes() != c["rows"][1].tobytes()


# ---- labels outside the rows; the number of rows on both sides of the LDS table ------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rows_case(max_rows):
    g, m = er.grid(0.0, 0.0, 1.0, 40, 33), er.fusion_map(0.0, 0.0, 1.0, 40, 33, 100, -60)
    rng = np.random.default_rng(max_rows)
    label = rng.integers(0, max_rows, (2, 33, 40)).astype(np.int32)        # every row has cells, neighbours differ: little to combine
    label[0, 0, :6] = [-1, max_rows, 2 ** 31 - 1, -2 ** 31, max_rows - 1, 0]
    label[1, 5:20, 5:30] = max_rows - 1                                     # ... and one row with many
    maps = rng.integers(-300, 300, (1, 33, 40)).astype(np.int16)
    return case(g, m, label, [er.IDENTITY], maps, er.rule(0, 2, 100, 100), max_rows, occ=fr.random_occupancy(2, 33, 40, 6))


@pytest.mark.parametrize("max_rows", [1, 8, 257, LDS_ROWS, LDS_ROWS + 1])
def test_the_number_of_rows_and_labels_outside_them(handle, max_rows):
    c = rows_case(max_rows)
    everywhere(handle, c, "max_rows %d" % max_rows)
    named = (c["label"] >= 0) & (c["label"] < max_rows)
    assert c["rows"]["cells"].sum() == named.sum() and not named[0, 0, :4].any() and named[0, 0, 4:6].all()
    assert (c["cls"][~named] == er.CELL_NONE).all() and c["masked"][~named].tobytes() == c["occ"][~named].tobytes()


# ---- map values at the thresholds and at the ends of int16 -----------------------------------------------------------------------------
def test_map_values_at_the_thresholds(handle):
    values = np.array([100, 99, -60, -59, -32768, 32767], np.int16)
    g, m = er.grid(0.0, 0.0, 1.0, 6, 4), er.fusion_map(0.0, 0.0, 1.0, 6, 4, 100, -60)
    label = np.tile(np.arange(6, dtype=np.int32), (1, 4, 1))                 # column x is row x
    c = case(g, m, label, [er.IDENTITY], np.tile(values, (1, 4, 1)), er.rule(0, 1, 256, 256), 6)
    everywhere(handle, c, "thresholds")
    assert c["rows"]["verdict"][0].tolist() == [er.STATIC, er.UNDECIDED, er.MOVING, er.UNDECIDED, er.MOVING, er.STATIC]
    assert c["rows"]["sum"][0].tolist() == [4 * int(v) for v in values] and c["rows"]["unknown"][0].tolist() == [0, 4, 0, 4, 0, 0]


# ---- sums beyond 2^31: one frame of 257 x 256 cells, all in one row ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def big_case(value):
    nx, ny = 257, 256
    g, m = er.grid(0.0, 0.0, 0.5, nx, ny), er.fusion_map(0.0, 0.0, 0.5, nx, ny, 100, -60)
    return case(g, m, np.zeros((1, ny, nx), np.int32), [er.IDENTITY], np.full((1, ny, nx), value, np.int16), er.rule(0, 1, 256, 256), 2)


@pytest.mark.parametrize("value", [32767, -32768])
def test_the_sum_is_accumulated_in_64_bits(handle, value):
    c = big_case(value)
    everywhere(handle, c, "all %d" % value, want_class=False, paths=(1, 2))
    assert c["rows"][0, 0]["sum"] == 257 * 256 * value and abs(int(c["rows"][0, 0]["sum"])) > 2 ** 31
    assert tuple(c["rows"][0, 0])[1:] == (65792, 65792, 65792 if value > 0 else 0, 0 if value > 0 else 65792, 0, er.STATIC if value > 0 else er.MOVING)


# ---- the two images: each on its own, both, in place, stray bytes ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def images_case():
    g, m = er.grid(-8.0, -8.0, 0.5, 33, 31), er.fusion_map(-8.0, -8.0, 0.5, 33, 31, 100, -60)
    rng = np.random.default_rng(12)
    maps = np.where(rng.random((1, 31, 33)) < 0.5, -200, 200).astype(np.int16)
    maps[0, :, :16] = -200                                                   # the rows on the left are movers
    occ = rng.integers(-128, 128, (2, 31, 33)).astype(np.int8)              # every byte there is, not only the three known ones
    label = noise_labels(2, 31, 33, 13, 8)
    label[:, 2:12, 1:9] = 7
    return case(g, m, label, [er.IDENTITY], maps, er.rule(0, 3, 200, 200), 8, occ=occ)


@pytest.mark.parametrize("want_class,with_occ,in_place", [(True, False, False), (False, True, False), (True, True, False), (True, True, True), (False, False, False)])
def test_the_class_image_and_the_masked_bytes(handle, want_class, with_occ, in_place):
    c = images_case()
    everywhere(handle, c, "class %d, mask %d, in place %d" % (want_class, with_occ, in_place), want_class, with_occ, in_place)
    assert c["rows"][0, 7]["verdict"] == er.MOVING and (c["masked"][:, 2:12, 1:9] == er.OCC_UNKNOWN).all()
    changed = c["masked"] != c["occ"]
    moving = c["rows"]["verdict"] == er.MOVING
    assert changed.any() and all(moving[f, c["label"][f, y, x]] for f, y, x in np.argwhere(changed))
    stray = ~np.isin(c["occ"], (0, 100, -1))
    assert stray.sum() > 1000 and (c["masked"][stray & ~changed] == c["occ"][stray & ~changed]).all()


# ---- pwpp_evidence_obstacles ----------------------------------------------------------------------------------------------------------
GRID = (-20.0, -20.0, 0.5, 80, 80)
BAND = (0.2, 2.5)
ROWS = 64


def chain_map():
    m = er.fusion_map(-21.0, -19.0, 0.4, 100, 104, 100, -60)
    return m, np.random.default_rng(31).integers(-300, 300, (2, 104, 100)).astype(np.int16)


def check_chain(h, frames, poses, mof, what):
    m, maps = chain_map()
    rule = er.rule(1, 2, 120, 120)
    label, table, n = h.label_obstacles(*GRID, *BAND, min_count=1, connectivity=8, max_clusters=ROWS, frames=frames)
    occ = fr.random_occupancy(frames, 80, 80, 17)
    got = h.evidence_obstacles(*GRID, *BAND, fmap_of(m), maps, rule4(rule), pose=poses, min_count=1, connectivity=8, max_clusters=ROWS, occupancy=occ, map_of_frame=mof,
                               want_class=True, frames=frames)
    assert got[0].tobytes() == label.tobytes() and got[2].tobytes() == n.tobytes(), what     # the labelling's outputs are pwpp_label_obstacles' bytes
    for f in range(frames):
        k = min(int(n[f]), ROWS)
        assert got[1][f, :k].tobytes() == table[f, :k].tobytes(), what
    c = case(er.grid(*GRID), m, label, poses, maps, rule, ROWS, occ=occ, mof=mof)
    same(dict(rows=got[3], cls=got[4], masked=got[5]), c, what + " against the restatement")
    same(on_host(h, c, True, True, False), c, what + ": pwpp_evidence_grid on that image")
    # device memory: the label image an output at its minimum alignment, like every array of the evidence
    import torch
    L = h._L
    dl, dm, di = placed(np.full(label.shape, POISON, np.uint8).repeat(4), 4), placed(maps, 2), placed(occ, 1)
    dr, dc, do = placed(np.full((frames, ROWS * 32), POISON, np.uint8), 8), placed(np.full(label.shape, POISON, np.uint8), 1), placed(np.full(label.shape, POISON, np.uint8), 3)
    dt = torch.zeros(frames * ROWS * 48, dtype=torch.uint8, device="cuda")   # the cluster table: 8-byte aligned
    dn = torch.zeros(frames, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    g = pwpp_hip.GroundGrid(*GRID, 0, 0)
    p = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1, 6))
    mo = None if mof is None else np.asarray(mof, np.int32)
    vp, dp = (lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)), ctypes.c_void_p
    fm, r = fmap_of(m), pwpp_hip.EvidenceRule(*rule4(rule))
    rc = L.pwpp_evidence_obstacles(h._h, ctypes.byref(g), BAND[0], BAND[1], 1, 8, 0, frames, pwpp_hip.MEM_DEVICE, dp(dl[1]), None, None, dp(dt.data_ptr()), dp(dn.data_ptr()), ROWS,
                                   None, dp(di[1]), vp(p), len(p), vp(mo), ctypes.byref(fm), 2, dp(dm[1]), ctypes.byref(r), dp(dr[1]), dp(dc[1]), dp(do[1]))
    assert rc == 0, L.pwpp_last_error()
    h.synchronize()
    assert taken(dl, "label").tobytes() == label.tobytes() and dn.cpu().numpy().tobytes() == n.tobytes(), what
    taken(dm, "map", maps), taken(di, "occupancy_in", occ)
    dev = dict(rows=taken(dr, "rows").view(er.EVIDENCE).reshape(frames, ROWS), cls=taken(dc, "cell_class").view(np.int8).reshape(label.shape),
               masked=taken(do, "occupancy_out").view(np.int8).reshape(label.shape))
    same(dev, c, what + " (device)")
    return c, n


def test_evidence_obstacles_is_label_obstacles_plus_evidence_grid():
    h = pwpp_hip.Handle()
    L = h._L
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    g = pwpp_hip.GroundGrid(*GRID, 0, 0)
    m, maps = chain_map()
    fm = fmap_of(m)
    label, n, table, rows = np.zeros(6400, np.int32), np.zeros(1, np.int32), np.zeros(ROWS, pwpp_hip.OBSTACLE_CLUSTER_DTYPE), np.zeros(ROWS, er.EVIDENCE)
    pose = np.array(er.IDENTITY, np.float64)

    def raw(gate=0, max_rows=ROWS):
        r = pwpp_hip.EvidenceRule(gate, 1, 128, 128)
        return L.pwpp_evidence_obstacles(h._h, ctypes.byref(g), 0.2, 2.5, 1, 8, 0, 1, pwpp_hip.MEM_HOST, vp(label), None, None, vp(table), vp(n), max_rows, None, None,
                                         vp(pose), 1, None, ctypes.byref(fm), 2, vp(maps), ctypes.byref(r), vp(rows), None, None)

    assert raw() == E_STATE and raw(gate=9) == E_STATE       # the labelling's checks, the state among them, come first
    h.set_labels(True)  # (_everything reads them)
    h.estimate_ground(small_cloud(5))
    before = _everything(h, 1)
    assert raw(gate=9) == E_ARG and b"gate 9" in L.pwpp_last_error()
    assert raw(max_rows=0) == E_ARG and b"max_rows 0" in L.pwpp_last_error()
    for path in PATHS:
        h.set_option("evidence_path", path)
        c, n_clusters = check_chain(h, 1, [yaw(5, 0.2, 0.1)], [1], "one frame, path %d" % path)
    assert n_clusters[0] >= 5 and (c["rows"]["landed"] > 0).sum() >= 5 and len(set(c["rows"]["verdict"][0].tolist())) >= 3
    assert _everything(h, 1) == before, "the evidence changed the results of the call it reads"


def test_evidence_obstacles_on_three_frames_of_a_batch():
    h = pwpp_hip.Handle()
    h.estimate_ground_batch(three_frames(), mode=pwpp_hip.MODE_FRESH)  # a 16-beam scan, an empty frame, a frame that is all unref
    c, n_clusters = check_chain(h, 3, [er.IDENTITY, yaw(30), (1.0, 0.0, 0.5, 0.0, 1.0, 0.0)], [0, 1, -1], "three frames")
    assert n_clusters[0] >= 5 and n_clusters[1] == 0 and (c["rows"]["verdict"][1] == er.NONE).all() and c["rows"]["landed"][2].sum() == 0


# ---- workspace and neutrality ------------------------------------------------------------------------------------------------------
def test_workspace_and_that_nothing_else_moves():
    c = shape_case(*PAIRS[7])
    h = pwpp_hip.Handle()
    empty = h.workspace_bytes()
    same(on_host(h, c, True, True, False), c, "before any estimate call")
    staged = c["label"].nbytes + c["maps"].nbytes + c["rows"].nbytes + 3 * c["occ"].nbytes
    assert h.workspace_bytes() >= empty + staged, "the cluster buffer is not counted"
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
    same(on_host(b, c, True, True, False), c, "after an estimate call")
    assert b.workspace_bytes() >= untouched + staged
    assert a.workspace_bytes() == untouched, "a handle that never asked for evidence grew"
    assert _everything(b, 3) == before and b.time_us() == t_before, "the evidence changed the results of the call before it"
    for w in (a, b):
        w.estimate_ground_batch(frames, mode=pwpp_hip.MODE_FRESH)
    assert _everything(b, 3) == _everything(a, 3), "an estimate call after an evidence call differs from one without"
    b.trim_workspace()
    a.trim_workspace()
    assert a.workspace_bytes() == b.workspace_bytes()


# ---- bindings -----------------------------------------------------------------------------------------------------------------
def test_pybind_module_agrees_with_the_ctypes_handle():
    import pypatchworkpp
    pp = pypatchworkpp.patchworkpp(pypatchworkpp.Parameters())
    h = pwpp_hip.Handle()
    fm = pypatchworkpp.FusedObstacleMap()
    fm.x0, fm.y0, fm.cell, fm.nx, fm.ny = -20.0, -20.0, 0.5, 80, 80
    pose = [1.0, 0.0, 0.25, 0.0, 1.0, 0.0]
    pts = small_cloud(5)
    pp.estimateGround(pts)
    h.estimate_ground(pts)
    pp.updateObstacleMap(fm, pose, *GRID, *BAND)
    log_odds, _ = pp.updateObstacleMap(fm, pose, *GRID, *BAND)               # twice: 2 * hit = 80 >= occupied_at = 60
    m = er.fusion_map(fm.x0, fm.y0, fm.cell, fm.nx, fm.ny, fm.occupied_at, fm.free_at)
    occ = fr.random_occupancy(1, 80, 80, 3)
    rows = 6                                                               # fewer rows than clusters: the cells of the others count as unlabelled
    label, table, ev, cls, masked, count = pp.getObstacleEvidence(fm, *GRID, *BAND, pose=pose, gate=1, min_cells=2, moving_share=150, static_share=150, occupancy=occ[0],
                                                                  max_clusters=rows)
    want = h.evidence_obstacles(*GRID, *BAND, fmap_of(m), log_odds, (1, 2, 150, 150), pose=pose, max_clusters=rows, occupancy=occ, want_class=True)
    assert count == want[2][0] and count > rows and label.tobytes() == want[0][0].tobytes() and table.tobytes() == want[1][0, :rows].tobytes()
    assert ev.dtype == er.EVIDENCE and ev.tobytes() == want[3][0].tobytes() and cls.tobytes() == want[4][0].tobytes() and masked.tobytes() == want[5][0].tobytes()
    c = case(er.grid(*GRID), m, want[0], [pose], log_odds[None], er.rule(1, 2, 150, 150), rows, occ=occ)
    same(dict(rows=want[3], cls=want[4], masked=want[5]), c, "the chain against the restatement")
    # a scan against the map it was just fused into, under the same pose: every labelled cell was fused as occupied, so every landed cell reads occupied
    assert (ev["landed"] >= 2).any() and (ev["verdict"][ev["landed"] >= 2] == er.STATIC).all() and (ev["occupied"] == ev["landed"]).all()
    assert pp.getObstacleEvidence(fm, *GRID, *BAND)[4] is None
