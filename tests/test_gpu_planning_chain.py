"""On a real MI355X: the labelling chain that pwpp_label_obstacles, pwpp_track_obstacles and pwpp_evidence_obstacles share -- raster,
labelling, the fill of point_cluster with -1 and the per-point scatter -- gives the same bytes from all three, in host and in device
memory, with point_cluster asked for and without; and every option that picks a kernel variant names its values in one sentence.
(pwpp_set_option enters its handle before it reads the option, so its messages need a device.)  Two frames, one estimate call."""
import ctypes

import numpy as np
import pytest

import pwpp_hip
from test_gpu_obstacle_grid import small_cloud

pytestmark = pytest.mark.gpu

E_ARG = -1
GRID = (-20.0, -20.0, 0.5, 80, 80)  # the grid of the cluster tracks' chain tests
BAND = (0.2, 2.5)
ROWS, FRAMES = 64, 2
CELLS = FRAMES * GRID[3] * GRID[4]
POISON = -77
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
NAMES = ("label", "count", "top", "clusters", "n_clusters", "point_cluster")


@pytest.fixture(scope="module")
def handle():
    h = pwpp_hip.Handle()
    h.estimate_ground_batch([small_cloud(5), small_cloud(6)], mode=pwpp_hip.MODE_FRESH)
    return h


def fusion_map():
    return pwpp_hip.FusionMap(x0=GRID[0], y0=GRID[1], cell=GRID[2], nx=GRID[3], ny=GRID[4], hit=10, miss=5, l_min=-100, l_max=100, occupied_at=20, free_at=-20)


def labelling_on_host(h, which, with_pc):
    """The six arrays of the labelling from one of the three entry points, PWPP_MEM_HOST, every array poisoned before the call."""
    L, vp = h._L, lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    g = pwpp_hip.GroundGrid(*GRID, 0, 0)
    points = int(h.frame_base()[FRAMES] - h.frame_base()[0])
    label, count, n = np.full(CELLS, POISON, np.int32), np.full(CELLS, POISON, np.int32), np.full(FRAMES, POISON, np.int32)
    top = np.full(CELLS, np.float32(POISON), np.float32)
    table = np.zeros(FRAMES * ROWS, pwpp_hip.OBSTACLE_CLUSTER_DTYPE)
    pc = np.full(points, POISON, np.int32) if with_pc else None
    first = (h._h, ctypes.byref(g), BAND[0], BAND[1], 1, 8, 0, FRAMES, pwpp_hip.MEM_HOST, vp(label), vp(count), vp(top), vp(table), vp(n), ROWS, vp(pc))
    pose = np.array(IDENTITY, np.float64)
    if which == "label":
        rc = L.pwpp_label_obstacles(*first)
    elif which == "track":
        prev = np.full(CELLS, -1, np.int32)
        links = [np.zeros(FRAMES * ROWS, pwpp_hip.CLUSTER_LINK_DTYPE) for _ in range(2)]
        rc = L.pwpp_track_obstacles(*first, vp(prev), vp(pose), 1, 0, 1, 4 * ROWS, vp(links[0]), vp(links[1]), None, None, None, None, None)
    else:
        fmap, rule = fusion_map(), pwpp_hip.EvidenceRule(0, 1, 128, 128)
        maps, rows = np.zeros(GRID[3] * GRID[4], np.int16), np.zeros(FRAMES * ROWS, pwpp_hip.CLUSTER_EVIDENCE_DTYPE)
        rc = L.pwpp_evidence_obstacles(*first, None, vp(pose), 1, None, ctypes.byref(fmap), 1, vp(maps), ctypes.byref(rule), vp(rows), None, None)
    assert rc == 0, (which, L.pwpp_last_error())
    return dict(zip(NAMES, (label, count, top, table.view(np.uint8).reshape(FRAMES, ROWS * 48), n, pc)))


def labelling_on_device(h, which, with_pc):
    """The same from device arrays, poisoned before the call."""
    import torch
    points = int(h.frame_base()[FRAMES] - h.frame_base()[0])
    i32 = lambda n_, fill=POISON: torch.full((n_,), fill, dtype=torch.int32, device="cuda")
    label, count, n, pc = i32(CELLS), i32(CELLS), i32(FRAMES), i32(points)
    top = torch.full((CELLS,), float(POISON), dtype=torch.float32, device="cuda")
    table = torch.zeros(FRAMES * ROWS * 48, dtype=torch.uint8, device="cuda")
    common = dict(count_ptr=count.data_ptr(), top_ptr=top.data_ptr(), clusters_ptr=table.data_ptr(), n_clusters_ptr=n.data_ptr(),
                  point_cluster_ptr=pc.data_ptr() if with_pc else 0, frames=FRAMES)
    torch.cuda.synchronize()
    if which == "label":
        h.label_obstacles_device(*GRID, *BAND, 1, 8, label.data_ptr(), max_clusters=ROWS, **common)
    elif which == "track":
        prev, links = i32(CELLS, -1), [torch.zeros(FRAMES * ROWS * 4, dtype=torch.int32, device="cuda") for _ in range(2)]
        torch.cuda.synchronize()
        h.track_obstacles_device(*GRID, *BAND, 1, 8, label.data_ptr(), prev.data_ptr(), [IDENTITY], 0, 1, ROWS, 4 * ROWS, links[0].data_ptr(), links[1].data_ptr(), **common)
    else:
        maps = torch.zeros(GRID[3] * GRID[4], dtype=torch.int16, device="cuda")
        rows = torch.zeros(FRAMES * ROWS * 8, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        h.evidence_obstacles_device(*GRID, *BAND, 1, 8, label.data_ptr(), [IDENTITY], fusion_map(), 1, maps.data_ptr(), (0, 1, 128, 128), ROWS, rows.data_ptr(), **common)
    h.synchronize()
    out = [t.cpu().numpy() for t in (label, count, top, table, n, pc)]
    assert with_pc or (out[5] == POISON).all(), "point_cluster was written without being asked for"
    out[3] = out[3].reshape(FRAMES, ROWS * 48)
    return dict(zip(NAMES, out[:5] + [out[5] if with_pc else None]))


@pytest.mark.parametrize("with_pc", (True, False), ids=("point_cluster", "no_point_cluster"))
@pytest.mark.parametrize("mem", ("host", "device"))
def test_the_three_labelling_entry_points_give_the_same_bytes(handle, mem, with_pc):
    run = labelling_on_host if mem == "host" else labelling_on_device
    want = run(handle, "label", with_pc)
    n = np.minimum(want["n_clusters"], ROWS)  # the rows of a frame that are written
    assert want["n_clusters"].min() >= 2, "more than one cluster per frame"
    assert (want["label"] >= 0).any() and (want["count"] > 0).any() and (want["label"] != POISON).all() and (want["count"] != POISON).all()
    if with_pc:
        pc = want["point_cluster"]
        assert (pc == -1).any() and (pc >= 0).any() and (pc != POISON).all(), "points that are not counted, points that are, and none left unwritten"
        assert len(set(pc[pc >= 0].tolist())) >= 2
    for which in ("track", "evidence"):
        got = run(handle, which, with_pc)
        for name in NAMES:
            if name == "clusters":  # (the rows behind a frame's n_clusters are not written)
                for f in range(FRAMES):
                    assert got[name][f, :int(n[f]) * 48].tobytes() == want[name][f, :int(n[f]) * 48].tobytes(), "%s, %s: frame %d of the cluster table differs" % (which, mem, f)
            elif want[name] is None:
                assert got[name] is None
            else:
                assert got[name].tobytes() == want[name].tobytes(), "%s, %s: %s differs from pwpp_label_obstacles'" % (which, mem, name)


PATH_OPTIONS = dict(records_path=2, clusters_path=1, distance_path=1, visibility_path=1, fusion_path=1, elevation_path=2, terrain_path=2, reach_path=2, route_path=2,
                    costmap_path=2, match_path=2, evidence_path=2, boxes_path=2)


def test_every_path_option_names_its_values_in_one_sentence():
    h = pwpp_hip.Handle()
    L = h._L
    assert len(PATH_OPTIONS) == 13
    for name, most in PATH_OPTIONS.items():
        expected = {1: "0 or 1 expected", 2: "0, 1 or 2 expected"}[most]
        for bad in (-1, most + 1):
            assert L.pwpp_set_option(h._h, name.encode(), str(bad).encode()) == E_ARG, (name, bad)
            assert L.pwpp_last_error().decode() == "%s=%d: %s" % (name, bad, expected), (name, bad)
        for good in (most, 0):  # (0 last: the option is left at its default)
            assert L.pwpp_set_option(h._h, name.encode(), str(good).encode()) == 0, (name, good, L.pwpp_last_error())
    assert L.pwpp_set_option(h._h, b"no_such_path", b"0") == E_ARG and L.pwpp_last_error() == b"unknown option 'no_such_path'"
