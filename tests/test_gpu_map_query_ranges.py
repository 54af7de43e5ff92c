"""The frame range of the post-call map queries: pwpp_rasterize_obstacles, pwpp_label_obstacles and pwpp_box_obstacles on frames
[1, 3) of a three-frame batch against the slices of the same calls on [0, 3), byte for byte, from host and from device memory.
All three walk the non-ground lists through one description of the range (PwppObstacleScan: frame_first, the longest list of the
range, the first per-point slot), so the batch is made to tell the ranges apart: three scans of 2400, 3200 and 6400 points, the
LAST with the longest non-ground list, on the 65 x 17 grid that cuts the cloud.  tests/test_map_queries_cpu.py shows with the
restatements that frames 1 and 2 have clusters and boxes, so that the comparison is not one of empty tables."""
import numpy as np
import pytest

import obstacle_boxes_ref as ob
import obstacle_clusters_ref as oc
import pwpp_hip
import pwpp_synth

pytestmark = pytest.mark.gpu

F32 = np.float32
GRID = (2.0, -17 * 1.7 / 3, 1.7, 65, 17)  # x0, y0, cell, nx, ny
BAND = (0.2, 2.5)
MIN_COUNT, CONN, MAX_ROWS = 1, 4, 32
FIRST, FRAMES = 1, 2


def batch():
    return [pwpp_synth.make_cloud(seed, beams=16, azimuth_steps=steps) for seed, steps in ((11, 150), (12, 200), (13, 400))]


@pytest.fixture(scope="module")
def handle():
    h = pwpp_hip.Handle()
    h.estimate_ground_batch(batch(), mode=pwpp_hip.MODE_FRESH)
    n = [h.counts(f)[1] for f in range(3)]
    assert n[2] > max(n[:2])
    return h


def from_host_memory(h, first, frames):
    kw = dict(frame_first=first, frames=frames)
    out = {}
    out["count"], out["top"], out["unref"] = h.rasterize_obstacles(*GRID, *BAND, want_top=True, want_unref=True, **kw)
    out["label"], out["table"], out["n"], out["pc"] = h.label_obstacles(*GRID, *BAND, MIN_COUNT, CONN, max_clusters=MAX_ROWS, want_point_cluster=True, **kw)
    for path in (1, 2):
        h.set_option("boxes_path", path)
        out["boxes%d" % path] = h.box_obstacles(*GRID, *BAND, out["label"], MAX_ROWS, **kw)
    h.set_option("boxes_path", 0)
    return out


def from_device_memory(h, first, frames):
    import torch
    kw = dict(frame_first=first, frames=frames)
    nx, ny = GRID[3:]
    base = h.frame_base()
    points = int(base[first + frames] - base[first])
    new = lambda words: torch.full((words,), -7, dtype=torch.int32, device="cuda")
    img = {k: new(frames * ny * nx) for k in ("count", "top", "unref", "label")}
    table, n, pc = new(frames * MAX_ROWS * 12), new(frames), new(points)
    boxes = {path: new(frames * MAX_ROWS * 16) for path in (1, 2)}
    torch.cuda.synchronize()
    h.rasterize_obstacles_device(*GRID, *BAND, img["count"].data_ptr(), img["top"].data_ptr(), img["unref"].data_ptr(), **kw)
    h.label_obstacles_device(*GRID, *BAND, MIN_COUNT, CONN, img["label"].data_ptr(), 0, 0, table.data_ptr(), n.data_ptr(), MAX_ROWS, pc.data_ptr(), **kw)
    for path in (1, 2):
        h.set_option("boxes_path", path)
        h.box_obstacles_device(*GRID, *BAND, img["label"].data_ptr(), boxes[path].data_ptr(), MAX_ROWS, **kw)
    h.set_option("boxes_path", 0)
    h.synchronize()  # (complete after pwpp_synchronize: the copies below are on another stream)
    out = {k: v.cpu().numpy().reshape(frames, ny, nx) for k, v in img.items()}
    out["top"] = out["top"].view(F32)
    out["table"] = table.cpu().numpy().view(oc.CLUSTER_DTYPE).reshape(frames, MAX_ROWS)
    out["n"], out["pc"] = n.cpu().numpy(), pc.cpu().numpy()
    for path in (1, 2):
        out["boxes%d" % path] = boxes[path].cpu().numpy().view(ob.BOX_DTYPE).reshape(frames, MAX_ROWS)
    return out


@pytest.mark.parametrize("run", [from_host_memory, from_device_memory], ids=["host", "device"])
def test_a_sub_range_gives_the_slices_of_the_whole_range(handle, run):
    h = handle
    whole, sub = run(h, 0, 3), run(h, FIRST, FRAMES)
    same = lambda a, b: np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()
    for name in ("count", "top", "unref", "label", "n", "boxes1", "boxes2"):
        assert sub[name].shape[0] == FRAMES and same(sub[name], whole[name][FIRST:]), name
    assert same(whole["boxes1"], whole["boxes2"])
    base = h.frame_base()
    assert len(sub["pc"]) == base[3] - base[FIRST] and same(sub["pc"], whole["pc"][int(base[FIRST] - base[0]):]), "point_cluster"
    for fr in range(FRAMES):  # (the rows beyond the frame's clusters are unspecified)
        k = int(sub["n"][fr])
        assert 2 <= k <= MAX_ROWS and same(sub["table"][fr, :k], whole["table"][FIRST + fr, :k]), "cluster table of frame %d" % (FIRST + fr)
        assert (sub["boxes1"]["points"][fr, :k] > 0).all() and (sub["pc"] >= 0).any()
