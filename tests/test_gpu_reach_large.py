"""The cost-to-reach field where tests/test_gpu_reach.py stops: frames of more than 32 tiles, whose dirty bits (k_reach_tiles, one bit
per tile in words of 32) fill more than one word, and calls of more than 2^22 frames, which pwpp_launch_reach cuts into several launches.
Every comparison is byte for byte, reach and from.

The images are combs (rr.comb): random costs and walls across the image, each open at one end, so that the cheapest path runs the whole
image back and forth and the front passes into tiles of smaller index as often as into tiles of larger index -- a mark on a tile of the
word being walked or of an earlier word waits for the next pass, one on a later word is seen in the same pass.  tests/test_reach_cpu.py
builds them, computes the references once and shows without a GPU that each is exercised: every tile holds a reached cell, 3/4 of the
cells are reached, and the from chain of the dearest cell crosses the word boundaries; the same is asserted here before the GPU is asked.
A lost mark leaves values that are real path lengths or PWPP_REACH_NONE and sets no defect word: only an exact comparison sees it.

  a  219 x 183, 42 tiles in two words, vertical neighbours 7 indices apart; sources in the corners, in tiles 31 and 32 (the nine first
     marks fall into both words) and in the ragged last tile
  b  rows and columns of 34 tiles and a row of 66 (three words), from either end and from tiles 31 and 32
  c  max_reach on the 66 tiles: at most 4 of them are ever visited, the others keep their start
  d  two frames of 8193 x 9 cells, 257 tiles in 9 words, held to rr.certify, which decides exactly and without a Dijkstra whether a field
     is the reach field (the frame of the most tiles, 2193 in 69 words, passes too but needs minutes: see the test)
  e  2^22 + 3 frames of 2 x 1 cells against a closed form, the source alternating with the frame's parity: a frame index that ignores
     the launch's first frame reads a source of the other parity in half of the tail

Not provoked here: the defect path (a loop that meets its bound sets the defect word); it needs a defect to run."""
import numpy as np
import pytest

import pwpp_hip
import reach_ref as rr
import test_reach_cpu as C
from test_gpu_reach import PATHS, everywhere, on_device, on_host, same
from test_reach_cpu import TILE_X as TX, TILE_Y as TY

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def handle():
    return pwpp_hip.Handle()


# ---- a: two words, tiles above and below each other on either side of the boundary ---------------------------------------------
@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("k", range(len(C.COMB_SOURCES)), ids=lambda k: "source%d" % k)
def test_a_comb_of_42_tiles_in_two_words(handle, k, where):
    """(A case per memory kind: the sweeps of reach_path 1 need a sweep for every step of the path, 0.3 s a call here.)"""
    cost, src, p, want = C.comb_case(k)
    assert cost.shape == (6 * TY - 9, 7 * TX - 5)
    C.exercised(cost, src, want, crossings=4)
    for path in PATHS:
        handle.set_option("reach_path", path)
        try:
            same((on_host if where == "host" else on_device)(handle, cost, src, p), want, "comb, source %r (%s, path %d)" % (src, where, path))
        finally:
            handle.set_option("reach_path", 0)


# ---- b: strips of 34 and 66 tiles ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sorted(C.STRIPS))
def test_strips_of_tiles_from_either_end_and_from_the_word_boundary(handle, kind):
    for k, src in enumerate(C.strip_sources(kind)):
        cost, _, p, want = C.strip_case(kind, k)
        C.exercised(cost, src, want, every_boundary=k < 2)
        everywhere(handle, cost, src, p, want, "%s, source %r" % (kind, src))
    # the four sources as the frames of one call
    batch = np.stack([C.strip_image(kind)] * 4)
    srcs = np.array(C.strip_sources(kind), np.int32)
    want = tuple(np.stack([C.strip_case(kind, k)[3][i] for k in range(4)]) for i in range(2))
    everywhere(handle, batch, srcs, C.STRIP_P, want, "%s, four frames" % kind)


# ---- c: max_reach among many tiles ---------------------------------------------------------------------------------------------
def test_max_reach_among_66_tiles_leaves_the_others_at_their_start(handle):
    for cost, src, p, want in C.limited_strip_cases():
        ny, nx = cost.shape
        yy, xx = np.nonzero(want[0] != rr.NONE)
        used = np.unique(C.tile_of(xx, yy, nx))
        assert 2 <= len(used) <= 4
        everywhere(handle, cost, src, p, want, "max_reach %d" % p["max_reach"])
        never = ~np.isin(C.tile_of(*np.meshgrid(np.arange(nx), np.arange(ny)), nx), used)
        assert never.sum() > 60 * TX * ny and (want[0][never] == rr.NONE).all() and (want[1][never] == -1).all()


# ---- d: 257 tiles in 9 words ----------------------------------------------------------------------------------------------------
def test_two_frames_of_257_tiles_in_9_words(handle):
    """Two frames of 8193 x 9 cells at base 1, one uniform, one a comb from its far end; reach_path 2 in host and in device memory and
    reach_path 0 in host memory.  Held to rr.certify, which needs no Dijkstra, and only then judged through the GPU's own from chain.
    Not reach_path 1: k_reach_sweep is one workgroup a frame that sweeps all its cells once for every step of the comb's path.

    The frame of the most tiles the entry points accept, 23365 x 65 cells (2193 tiles, 69 words), passed these same checks on an
    MI355X -- path 2 in host and device memory, path 0 in host memory, the uniform frame equal to the closed form, both frames
    certified, the comb's chain through all 69 words -- but took 159 s, 53 s a call, against 0.47 s for the slowest test of
    tests/test_gpu_reach.py in the same run: one workgroup walks a path of 69302 steps through its 2193 tiles.  So this smaller frame
    stands in its place."""
    nx, ny = C.WIDE
    cost, p = C.wide_images(), C.WIDE_P
    src = np.array(C.WIDE_SOURCES, np.int32)
    assert cost.shape == (2, ny, nx) and (nx + TX - 1) // TX == 257 and ny <= TY and rr.range_ok(p["base"], nx, ny)
    handle.set_option("reach_path", 2)
    try:
        first = on_host(handle, cost, src, p)
        # frame 0, uniform: the closed form, then the field and its from as a whole
        assert first[0][0].tobytes() == C.octile(nx, ny, src[0], p["base"] + 17).tobytes(), "the uniform frame is not the octile distance"
        assert rr.certify(cost[0], src[0], p, first[0][0], first[1][0]) is None
        assert C.exercised(cost[0], src[0], (first[0][0], first[1][0]))["reached"] == nx * ny
        # frame 1, the comb: certified, then -- the field being the reach field -- judged through its own from chain
        assert rr.certify(cost[1], src[1], p, first[0][1], first[1][1]) is None
        found = C.exercised(cost[1], src[1], (first[0][1], first[1][1]), every_boundary=True)
        assert found["words"] == list(range(9))
        same(on_device(handle, cost, src, p), first, "257 tiles (device, path 2)")
        handle.set_option("reach_path", 0)
        same(on_host(handle, cost, src, p), first, "257 tiles (host, path 0)")
    finally:
        handle.set_option("reach_path", 0)


# ---- e: more than 2^22 frames in one call --------------------------------------------------------------------------------------
FRAMES = (1 << 22) + 3


def two_cells(cost, src_x, p):
    """(reach, from) of (frames, 1, 2) frames in closed form; src_x: (frames,) the source's x.  0 at the source, which names itself; the
    other cell 5 (t_source + t_other) through the source, or NONE / -1 where it is impassable; the source's term is base where its byte
    is impassable."""
    t = rr.terms_array(cost.reshape(-1, 2), None, p)
    f = np.arange(len(t))
    t_src, t_other = t[f, src_x], t[f, 1 - src_x]
    t_src = np.where(t_src == 0, p["base"], t_src)
    reach = np.zeros((len(t), 2), np.int64)
    frm = np.empty((len(t), 2), np.int64)
    reach[f, 1 - src_x] = np.where(t_other > 0, 5 * (t_src + t_other), rr.NONE)
    frm[f, src_x] = src_x
    frm[f, 1 - src_x] = np.where(t_other > 0, src_x, -1)
    return reach.astype(np.int32).reshape(cost.shape), frm.astype(np.int32).reshape(cost.shape)


@pytest.fixture(scope="module")
def many():
    """The inputs and the expected fields of the 2^22 + 3 frames, computed once, and a handle of their own whose buffers are given back."""
    rng = np.random.default_rng(5)
    cost = rng.integers(-128, 128, (FRAMES, 1, 2), dtype=np.int8)   # every byte: unknown ones (as 40), lethal ones (90 .. 127)
    p = rr.params(base=3, lethal=90, unknown=40)
    src = np.zeros((FRAMES, 2), np.int32)
    src[:, 0] = np.arange(FRAMES) % 2
    want = two_cells(cost, src[:, 0], p)
    one = two_cells(cost, np.ones(FRAMES, np.int64), p)
    for part in (slice(0, 64), slice(FRAMES - 64, FRAMES), slice((1 << 22) - 32, (1 << 22) + 32)):   # the closed form against the Dijkstra
        same(tuple(w[part] for w in want), rr.reach(cost[part], src[part], p), "the closed form, frames %r" % (part,))
        same(tuple(w[part] for w in one), rr.reach(cost[part], (1, 0), p), "the closed form, one source, frames %r" % (part,))
    flat = want[0].reshape(-1, 2)
    assert (flat == rr.NONE).sum() > FRAMES // 16 and ((flat != rr.NONE) & (flat != 0)).sum() > FRAMES // 2
    assert (src[1 << 22:, 0] == [0, 1, 0]).all() and (flat[np.arange(1 << 22, FRAMES), src[1 << 22:, 0]] == 0).all()
    # a second launch that began at frame 0 again would leave the three frames of the tail at their start: they must have something to lose
    assert ((flat[1 << 22:] != 0) & (flat[1 << 22:] != rr.NONE)).sum() >= 2 and flat[(1 << 22) + 1, 1] == 0
    for a in (cost, src) + want + one:
        a.setflags(write=False)
    h = pwpp_hip.Handle()
    empty = h.workspace_bytes()
    yield h, cost, src, p, want, one
    h.set_option("reach_path", 0)
    h.trim_workspace()
    assert h.workspace_bytes() == empty


@pytest.mark.parametrize("where,path,sources", [("host", 1, "each"), ("host", 2, "each"), ("device", 2, "each"), ("host", 2, "one")])
def test_more_frames_than_one_launch_takes(many, where, path, sources):
    h, cost, src, p, want, one = many
    h.set_option("reach_path", path)
    try:
        got = (on_host if where == "host" else on_device)(h, cost, src if sources == "each" else (1, 0), p)
    finally:
        h.set_option("reach_path", 0)
    same(got, want if sources == "each" else one, "2^22 + 3 frames (%s, path %d, %s)" % (where, path, sources))
