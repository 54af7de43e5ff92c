"""The edges of the group loop (wave_for_each_group, csrc/pwpp_wave.h; wave_combine of the tracks) on a real MI355X, through the two entry points that take a
label image directly, so that lane = cell: pwpp_evidence_grid at every value of "evidence_path" and pwpp_associate_grid.  One frame
of 8 x 8 cells is exactly one wave; 13 x 5 cells are 65: a second wave with one live lane.  Every comparison is exact equality of
bytes with the restatements the modules' own tests use (tests/evidence_ref.py, tests/tracks_ref.py), in host and in device memory.
References are computed once per case."""
import functools

import numpy as np
import pytest

import evidence_ref as er
import pwpp_hip
import test_gpu_evidence as ev
import test_gpu_tracks as tk
import tracks_ref as tr

pytestmark = pytest.mark.gpu

SHAPES = [(8, 8), (13, 5)]  # (nx, ny)
PATTERNS = ["distinct", "one_row", "alternating", "interleaved", "lane_63_alone", "lanes_0_and_63"]


def labels(pattern, n):
    """The rows of cells 0 .. n - 1 (cell i is lane i % 64 of wave i / 64), and the number of rows."""
    i = np.arange(n, dtype=np.int32)
    if pattern == "distinct":          # 64 rows in the first wave: the 64-round worst case
        return i.copy(), n
    if pattern == "one_row":           # one round
        return np.zeros(n, np.int32), 1
    if pattern == "alternating":       # rows on the even lanes, -1 on the odd ones
        return np.where(i % 2 == 0, (i // 2) % 3, -1).astype(np.int32), 3
    if pattern == "interleaved":       # two rows, lane by lane
        return (i % 2).astype(np.int32), 2
    out = np.full(n, -1, np.int32)     # a row held by lane 63 alone, or by lanes 0 and 63 only (and by the one lane of a second wave)
    out[63:] = 2
    if pattern == "lanes_0_and_63":
        out[0] = 2
    return out, 3


@pytest.fixture(scope="module")
def handle():
    return pwpp_hip.Handle()


@functools.lru_cache(maxsize=None)
def evidence_case(pattern, shape):
    nx, ny = shape
    label, rows = labels(pattern, nx * ny)
    g, m = er.grid(0.0, 0.0, 1.0, nx, ny), er.fusion_map(0.0, 0.0, 1.0, nx, ny, 100, -60)
    maps = np.random.default_rng(nx).integers(-300, 300, (1, ny, nx)).astype(np.int16)  # every class, sums of both signs
    return ev.case(g, m, label.reshape(1, ny, nx), [er.IDENTITY], maps, er.rule(0, 1, 128, 128), rows)


@functools.lru_cache(maxsize=None)
def tracks_case(pattern, shape):
    nx, ny = shape
    curr, rows = labels(pattern, nx * ny)
    prev = np.ascontiguousarray(curr[::-1])  # another partner for most lanes: the pairs' 64-bit keys differ from the rows' 32-bit ones
    g = tr.grid(0.0, 0.0, 1.0, nx, ny)
    curr, prev = curr.reshape(1, ny, nx), prev.reshape(1, ny, nx)
    want = tr.associate(curr, prev, g, g, [tr.IDENTITY], 0, 1, rows, 2 * nx * ny)
    tk.frozen(curr, prev, *want.values())
    return g, curr, prev, rows, want


@pytest.mark.parametrize("shape", SHAPES, ids=tk.shape_ids)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_evidence_of_each_pattern_at_every_path(handle, pattern, shape):
    c = evidence_case(pattern, shape)
    ev.everywhere(handle, c, "%s, %s" % (pattern, tk.shape_ids(shape)))
    named = c["label"] >= 0
    assert c["rows"]["cells"].sum() == named.sum() and (c["rows"]["landed"] == c["rows"]["cells"]).all()
    assert c["rows"]["sum"].sum() == c["maps"][named].astype(np.int64).sum()
    if pattern == "distinct":
        assert (c["rows"]["cells"] == 1).all()


@pytest.mark.parametrize("shape", SHAPES, ids=tk.shape_ids)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_tracks_of_each_pattern(handle, pattern, shape):
    g, curr, prev, rows, want = tracks_case(pattern, shape)
    tk.everywhere(handle, want, "%s, %s" % (pattern, tk.shape_ids(shape)), curr, prev, g, g, [tr.IDENTITY], 0, 1, rows, 2 * curr.size)
    assert want["curr_links"]["cells"].sum() == (curr >= 0).sum() and want["prev_links"]["cells"].sum() == (prev >= 0).sum()
    if pattern == "distinct":
        assert want["n_pairs"][0] == curr.size and (want["curr_links"]["cells"] == 1).all()
