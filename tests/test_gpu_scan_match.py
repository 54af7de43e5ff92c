"""The correlative scan match (pwpp_match_grid, pwpp_match_obstacles) on a real MI355X, against the restatement of
tests/scan_match_ref.py -- the best rows and the whole scores array compared, no tolerance: frame images from one cell to 64 x 64
filled from none occupied to all occupied with stray bytes, frames with fewer cells than a chunk, exactly a chunk and several chunks,
maps of one cell, three maps of 70 x 67 and one of 400 x 300, map values over the whole int16 range, windows from (0, 0) to more
shifts than a workgroup has lanes and (64, 64) once, 1 to 33 candidates of every kind for all frames or a set per frame, four cell
ratios of which one divides, every form of map_of_frame, a sum beyond int32, all three values of the option "match_path" with
rectangles of the map that fit the LDS and ones that do not, host and
device memory with a misaligned map and bytes in poisoned surroundings, scores absent, pwpp_match_obstacles against its three steps,
two device calls back to back with different origins and candidates, the workspace, and that asking changes nothing else."""
import ctypes
import functools

import numpy as np
import pytest

import occupancy_fusion_ref as fr
import pwpp_hip
import scan_match_ref as mr
from test_gpu_obstacle_grid import _everything, small_cloud, three_frames

pytestmark = pytest.mark.gpu

E_STATE = -4
BAND = (0.2, 2.5)
MAP_SHAPES = [(1, 1, 1), (70, 67, 3), (400, 300, 1)]  # (NX, NY, n_maps): a single cell; several maps; more halfwords than a CU has LDS
IMAGES = [(1, 1), (5, 7), (33, 31), (64, 64)]  # (nx, ny) of the frame images
WINDOWS = [(0, 0), (1, 0), (3, 2), (8, 8)]  # (wx, wy); 17 x 17 shifts are more than the 256 of a workgroup
CANDIDATES = (1, 2, 5, 33)
CELLS = ((0.5, 0.5), (0.25, 0.5), (1.0, 0.5), (0.3, 0.5))  # (CELL, cell); 0.3 has no exact reciprocal: the division
FILLS = ((1.0, 0.0, 0.0), (0.55, 0.15, 0.3), (0.3, 0.6, 0.1), (0.0, 1.0, 0.0))  # (free, occupied, unknown): none occupied .. all occupied
CHUNK = 256  # PWPP_MATCH_CHUNK: the occupied cells a workgroup lands at a time
shape_ids = lambda s: "%dx%dx%d" % s
NAN = float("nan")


def fmap_of(mgrid):
    return pwpp_hip.FusionMap(float(mgrid[0]), float(mgrid[1]), float(mgrid[2]), int(mgrid[3]), int(mgrid[4]), *[int(p) for p in fr.PAR])


def centred(n, cell):
    return -0.5 * n * cell


def candidate_kinds(CELL, reach, seed, n):
    """identity, a whole-cell translation, a quarter turn, two random rigid poses, a frame half outside, one wholly outside, a NaN,
    a mirror; beyond nine, further random rigid poses."""
    r = fr.random_poses(2 + max(n - 9, 0), seed, 0.25 * reach)
    kinds = [fr.IDENTITY, (1.0, 0.0, 3 * CELL, 0.0, 1.0, -2 * CELL), (0.0, -1.0, 0.0, 1.0, 0.0, 0.0), r[0], r[1], fr.rigid(0.4, 0.5 * reach, 0.1),
             (1.0, 0.0, 1e7, 0.0, 1.0, 0.0), (1.0, 0.0, NAN, 0.0, 1.0, 0.0), (-1.0, 0.0, 0.3, 0.0, 1.0, -0.2)]
    return [kinds[(seed + i) % 9] for i in range(min(n, 9))] + r[2:]


def kind_of(c, mgrid, reach):
    """The kind of one candidate of candidate_kinds, told from its numbers."""
    a, b, tx, cc, d, ty = (float(v) for v in c)
    if np.isnan(c).any():
        return "nan"
    if tx == 1e7:
        return "wholly outside"
    if a * d - b * cc < 0:
        return "mirror"
    if (a, b, cc, d) == (1.0, 0.0, 0.0, 1.0):
        return "identity" if (tx, ty) == (0.0, 0.0) else "translation"
    if (a, b, cc, d) == (0.0, -1.0, 1.0, 0.0):
        return "quarter turn"
    return "half outside" if tx == 0.5 * reach else "rigid"


def random_maps(n_maps, NY, NX, seed):
    """Values over the whole int16 range, both ends among them."""
    rng = np.random.default_rng(seed)
    maps = rng.integers(-32768, 32768, (n_maps, NY, NX)).astype(np.int16)
    flat = maps.reshape(-1)
    flat[rng.integers(0, flat.size, max(1, flat.size // 8))] = 32767
    flat[rng.integers(0, flat.size, max(1, flat.size // 8))] = -32768
    return maps


@functools.lru_cache(maxsize=None)
def case(NX, NY, n_maps, nx, ny, window, k):
    """The inputs and the expected results of one combination: computed once, shared, never written.  k rotates the fills, the
    number and kinds of the candidates, the sets, the cell ratio and the form of map_of_frame, so that the combinations together
    cover all of them."""
    CELL, cell = CELLS[k % len(CELLS)]
    wx, wy = WINDOWS[window]
    n_cand = CANDIDATES[(k // 4 + k) % 4]
    frames = n_maps if (n_maps > 1 and k % 2 == 0) else 1 + k % 3 + (n_maps > 1)
    grid, mgrid = (centred(nx, cell), centred(ny, cell), cell), (centred(NX, CELL) + CELL, centred(NY, CELL), CELL, NX, NY)
    occ = np.concatenate([fr.random_occupancy(1, ny, nx, 100 * k + f, FILLS[(k + f) % len(FILLS)], stray=(k + f) % 2 == 0) for f in range(frames)])
    reach = max(NX * CELL, nx * cell)
    sets = frames if k % 3 == 0 else 1
    cand = np.array([candidate_kinds(CELL, reach, k + 5 * s, n_cand) for s in range(sets)], np.float64)
    if n_maps == 1 or frames == n_maps:
        mof = None  # one map, or lock-step
    else:  # explicit, interleaved and unsorted, with a skipped frame
        mof = [(7 * i + k) % n_maps for i in range(frames)]
        mof[(k + 1) % frames] = -1
    maps = random_maps(n_maps, NY, NX, k)
    want = mr.match(occ, grid, cand if sets > 1 else cand[0], mgrid, maps, wx, wy, mof)
    for a in (occ, maps, cand) + want:
        a.setflags(write=False)
    return occ, grid, cand, mgrid, maps, wx, wy, mof, want


@pytest.fixture(scope="module")
def handle():
    return pwpp_hip.Handle()  # (no estimate call: pwpp_match_grid needs the handle's stream and buffer only)


def on_host(h, occ, grid, cand, mgrid, maps, wx, wy, mof, want_scores=True):
    got = h.match_grid(occ, grid, cand, fmap_of(mgrid), maps, wx, wy, mof, want_scores=want_scores)
    return got if want_scores else (got, None)


def on_device(h, occ, grid, cand, mgrid, maps, wx, wy, mof, want_scores=True, off=1):
    """match_grid on device arrays; the map starts `off` halfwords, the bytes `off` bytes behind a 256-byte boundary; what surrounds
    them and the results is poisoned and must survive, the inputs must not be written."""
    import torch
    frames, ny, nx = occ.shape
    n_cand = cand.shape[-2]
    n_scores = frames * n_cand * (2 * wy + 1) * (2 * wx + 1)
    docc = torch.full((occ.size + 512,), 77, dtype=torch.int8, device="cuda")
    dmap = torch.full((maps.size + 256,), -7, dtype=torch.int16, device="cuda")
    dbest = torch.full((3 * frames + 32,), -7, dtype=torch.int64, device="cuda")
    dscores = torch.full((n_scores + 32,), -7, dtype=torch.int64, device="cuda")
    assert all(b.data_ptr() % 256 == 0 for b in (docc, dmap, dbest, dscores))
    docc[off:off + occ.size] = torch.from_numpy(occ.reshape(-1).copy()).cuda()
    dmap[off:off + maps.size] = torch.from_numpy(maps.reshape(-1).copy()).cuda()
    torch.cuda.synchronize()
    h.match_grid_device(grid, nx, ny, frames, docc.data_ptr() + off, cand, fmap_of(mgrid), maps.shape[0], dmap.data_ptr() + 2 * off, wx, wy,
                        dbest.data_ptr() + 8, dscores.data_ptr() + 8 if want_scores else 0, mof)
    h.synchronize()  # (complete after pwpp_synchronize: the copies below are on another stream)
    rocc, rmap, rbest, rscores = docc.cpu().numpy(), dmap.cpu().numpy(), dbest.cpu().numpy(), dscores.cpu().numpy()
    assert (rocc[:off] == 77).all() and (rocc[off + occ.size:] == 77).all() and np.array_equal(rocc[off:off + occ.size], occ.reshape(-1)), "the frames were written"
    assert (rmap[:off] == -7).all() and (rmap[off + maps.size:] == -7).all() and np.array_equal(rmap[off:off + maps.size], maps.reshape(-1)), "the map was written"
    assert rbest[0] == -7 and (rbest[1 + 3 * frames:] == -7).all(), "a word outside the rows was written"
    assert rscores[0] == -7 and (rscores[1 + n_scores:] == -7).all() and (want_scores or (rscores == -7).all()), "a word outside the scores was written"
    best = np.frombuffer(rbest[1:1 + 3 * frames].tobytes(), mr.BEST_DTYPE)
    return best, (rscores[1:1 + n_scores].reshape(frames, n_cand, 2 * wy + 1, 2 * wx + 1) if want_scores else None)


def both_paths(h, call):
    """call() at "match_path" 0, 1 (every read from global memory) and 2 (the map's rectangle in LDS where it fits): identical
    bytes; returns them."""
    res = []
    for path in (0, 1, 2):
        h.set_option("match_path", path)
        res.append(call())
    h.set_option("match_path", 0)
    for other in res[1:]:
        for a, b in zip(res[0], other):
            assert (a is None and b is None) or a.tobytes() == b.tobytes(), "the values of match_path differ"
    return res[0]


def check(got, want, what):
    best, scores = got
    if scores is not None:
        assert scores.dtype == np.int64 and scores.shape == want[1].shape, what
        bad = np.argwhere(scores != want[1])
        assert len(bad) == 0, "%s: %d scores differ, the first (frame, candidate, sy, sx) = %s: %d, expected %d" % (
            what, len(bad), bad[0], scores[tuple(bad[0])], want[1][tuple(bad[0])])
    assert best.dtype == mr.BEST_DTYPE and best.shape == want[0].shape, what
    assert best.tolist() == want[0].tolist(), "%s: the best rows differ: %s, expected %s" % (what, best.tolist(), want[0].tolist())


@pytest.mark.parametrize("shape", MAP_SHAPES, ids=shape_ids)
def test_map_shapes_against_the_reference(handle, shape):
    NX, NY, n_maps = shape
    k = 0
    for nx, ny in IMAGES:
        for window in range(len(WINDOWS)):
            k += 1
            occ, grid, cand, mgrid, maps, wx, wy, mof, want = case(NX, NY, n_maps, nx, ny, window, k)
            what = "map %s, frames %d of %dx%d, window %s, %s candidates, cells %s, case %d" % (
                shape_ids(shape), len(occ), nx, ny, WINDOWS[window], cand.shape, CELLS[k % len(CELLS)], k)
            args = (occ, grid, cand, mgrid, maps, wx, wy, mof)
            check(both_paths(handle, lambda: on_host(handle, *args)), want, what)
            if k % 3 == 1:
                check(both_paths(handle, lambda: on_device(handle, *args)), want, what + ", device")
            if k % 4 == 2:
                check(on_host(handle, *args, want_scores=False), want, what + ", no scores")
                check(on_device(handle, *args, want_scores=False), want, what + ", device, no scores")


def test_the_rotation_covers_every_kind_of_case():
    """What the parametrised test above relies on: together its cases hold every candidate count, both kinds of sets, every cell
    ratio, every form of map_of_frame, skipped frames, empty and full frames, and scores of both signs."""
    seen = set()
    for NX, NY, n_maps in MAP_SHAPES:
        k = 0
        for nx, ny in IMAGES:
            for window in range(len(WINDOWS)):
                k += 1
                occ, grid, cand, mgrid, maps, wx, wy, mof, want = case(NX, NY, n_maps, nx, ny, window, k)
                for c in cand.reshape(-1, 6):
                    seen.add(("kind", kind_of(c, mgrid, max(NX * mgrid[2], nx * grid[2]))))
                seen.add(("candidates", cand.shape[1]))
                seen.add(("sets", "per frame" if cand.shape[0] == len(occ) and len(occ) > 1 else "one"))
                seen.add(("cells", CELLS[k % len(CELLS)]))
                seen.add(("mof", "null" if mof is None else "explicit"))
                seen.add(("lock-step", mof is None and n_maps > 1))
                if mof is not None and -1 in mof:
                    seen.add("skipped")
                for f in range(len(occ)):
                    n = int((occ[f] == 100).sum())
                    seen.add("empty" if n == 0 else ("full" if n == nx * ny else ("chunks" if n > CHUNK else "some")))
                seen.add(("positive", bool((want[1] > 0).any())))
                seen.add(("negative", bool((want[1] < 0).any())))
    for kind in ("identity", "translation", "quarter turn", "rigid", "half outside", "wholly outside", "nan", "mirror"):
        assert ("kind", kind) in seen, kind
    for n in CANDIDATES:
        assert ("candidates", n) in seen
    for c in CELLS:
        assert ("cells", c) in seen
    for what in (("sets", "one"), ("sets", "per frame"), ("mof", "null"), ("mof", "explicit"), ("lock-step", True), "skipped", "empty", "full", "chunks", "some",
                 ("positive", True), ("negative", True)):
        assert what in seen, what


def test_a_chunk_exactly_one_more_one_less_and_several(handle):
    nx, ny, NX, NY = 64, 64, 70, 67
    grid, mgrid = (centred(nx, 0.5), centred(ny, 0.5), 0.5), (centred(NX, 0.5), centred(NY, 0.5), 0.5, NX, NY)
    rng = np.random.default_rng(5)
    counts = (CHUNK, CHUNK + 1, CHUNK - 1, 2 * CHUNK, 1000, 64 * 64)
    occ = np.full((len(counts), ny, nx), -1, np.int8)
    for f, n in enumerate(counts):
        occ[f].reshape(-1)[rng.permutation(nx * ny)[:n]] = 100
    maps = random_maps(1, NY, NX, 6)
    cand = np.array([fr.IDENTITY, fr.rigid(0.3, 1.0, -0.5)], np.float64)
    want = mr.match(occ, grid, cand, mgrid, maps, 2, 1)
    assert want[0]["cells"].tolist() == list(counts)
    for run in (on_host, on_device):
        check(both_paths(handle, lambda: run(handle, occ, grid, cand, mgrid, maps, 2, 1, None)), want, "chunks, %s" % run.__name__)


def test_the_widest_window_once(handle):
    nx, ny = 5, 7
    for NX, NY in ((70, 67), (1, 1)):
        grid, mgrid = (centred(nx, 0.5), centred(ny, 0.5), 0.5), (centred(NX, 0.5), centred(NY, 0.5), 0.5, NX, NY)
        occ = fr.random_occupancy(1, ny, nx, 3, FILLS[2])
        maps = random_maps(1, NY, NX, 4)
        cand = np.array([fr.rigid(0.2, 0.3, 0.1), fr.IDENTITY], np.float64)
        want = mr.match(occ, grid, cand, mgrid, maps, 64, 64)
        assert want[1].shape == (1, 2, 129, 129)
        check(both_paths(handle, lambda: on_host(handle, occ, grid, cand, mgrid, maps, 64, 64, None)), want, "window (64, 64), map %d x %d" % (NX, NY))
    check(on_device(handle, occ, grid, cand, mgrid, maps, 64, 64, None), want, "window (64, 64), device")


def test_a_sum_beyond_int32(handle):
    nx, ny = 384, 256
    occ = np.full((1, ny, nx), 100, np.int8)
    maps = np.full((1, ny, nx), 32767, np.int16)
    grid, mgrid = (0.0, 0.0, 0.5), (0.0, 0.0, 0.5, nx, ny)
    want = mr.match(occ, grid, [fr.IDENTITY], mgrid, maps, 1, 1)
    assert want[1][0, 0, 1, 1] == 98304 * 32767 > 2 ** 31
    for run in (on_host, on_device):
        got = both_paths(handle, lambda: run(handle, occ, grid, np.array([fr.IDENTITY]), mgrid, maps, 1, 1, None))
        check(got, want, "98304 cells of 32767, %s" % run.__name__)
        assert got[0][0].tolist() == (98304 * 32767, 0, 0, 0, 98304)
    low = np.full((1, ny, nx), -32768, np.int16)
    check(on_host(handle, occ, grid, np.array([fr.IDENTITY]), mgrid, low, 1, 1, None), mr.match(occ, grid, [fr.IDENTITY], mgrid, low, 1, 1), "98304 cells of -32768")


def test_a_rectangle_larger_than_lds_is_read_from_global_memory(handle):
    """Path 0 stages at most 65536 map cells.  Occupied cells in the corners of a 400 x 300 image on a 400 x 300 map of the same cells
    reach all 120000 of them under the identity, so that (frame, candidate) takes the fallback; the second candidate turns the frame
    about its centre, the third moves it out of the map but for one corner (a rectangle of a few cells, staged), the fourth is out of
    reach altogether (no rectangle)."""
    nx, ny = 400, 300
    grid, mgrid = (centred(nx, 0.5), centred(ny, 0.5), 0.5), (centred(nx, 0.5), centred(ny, 0.5), 0.5, nx, ny)
    rng = np.random.default_rng(8)
    occ = np.full((2, ny, nx), -1, np.int8)
    for f in range(2):
        occ[f].reshape(-1)[rng.permutation(nx * ny)[:300 + 300 * f]] = 100
        occ[f, 0, 0] = occ[f, ny - 1, nx - 1] = occ[f, 0, nx - 1] = occ[f, ny - 1, 0] = 100
    maps = random_maps(1, ny, nx, 9)
    cand = np.array([fr.IDENTITY, fr.rigid(0.5, 0.0, 0.0), (1.0, 0.0, 199.0, 0.0, 1.0, 149.0), (1.0, 0.0, 300.0, 0.0, 1.0, 0.0)], np.float64)
    want = mr.match(occ, grid, cand, mgrid, maps, 3, 2)
    assert want[1][:, 0].any() and want[1][:, 2].any() and not want[1][:, 3].any()
    for run in (on_host, on_device):
        check(both_paths(handle, lambda: run(handle, occ, grid, cand, mgrid, maps, 3, 2, None)), want, "400 x 300 in reach, %s" % run.__name__)


def test_map_of_frame_in_every_form(handle):
    NX, NY, nx, ny = 37, 29, 33, 31
    grid, mgrid = (centred(nx, 0.5), centred(ny, 0.5), 0.5), (centred(NX, 0.5), centred(NY, 0.5), 0.5, NX, NY)
    occ = fr.random_occupancy(6, ny, nx, 21)
    cand = np.array([fr.random_poses(3, 22 + f, 3.0) for f in range(6)], np.float64)
    maps = random_maps(6, NY, NX, 23)
    # NULL with one map; NULL with n_maps == frames: lock-step; explicit: interleaved, unsorted, skipped frames, a map no frame names
    for n_maps, mof in ((1, None), (6, None), (4, [3, 0, -1, 3, 1, 0]), (4, [-1] * 6)):
        want = mr.match(occ, grid, cand, mgrid, maps[:n_maps], 2, 2, mof)
        for run in (on_host, on_device):
            check(both_paths(handle, lambda: run(handle, occ, grid, cand, mgrid, maps[:n_maps], 2, 2, mof)), want, "%d maps, map_of_frame %s, %s" % (n_maps, mof, run.__name__))
    assert want[0]["candidate"].tolist() == [-1] * 6 and not want[1].any() and (want[0]["cells"] > 0).all()
    L = pwpp_hip.load()
    with pytest.raises(pwpp_hip.PwppError):
        on_host(handle, occ, grid, cand, mgrid, maps[:4], 2, 2, np.array([0, 4, 0, 0, 0, 0], np.int32))
    assert b"map_of_frame 1 names map 4" in L.pwpp_last_error()


def test_a_fused_frame_matches_at_its_own_pose(handle):
    """The chain closed: fuse on the device, match on the device, and the frame is found where it was put."""
    grid, mgrid = (-6.0, -6.0, 0.5), (-16.0, -16.0, 0.5, 64, 64)
    occ = fr.random_occupancy(1, 24, 24, 7)
    true_pose = fr.rigid(0.0, 1.5, -2.0)
    fused, _ = handle.fuse_grid(occ, grid, true_pose, fmap_of(mgrid))
    prior = fr.rigid(0.0, 2.5, -0.5)   # two cells east, three north of the truth
    cand = pwpp_hip.yaw_candidates(prior, 0.05, 3)
    best, scores = handle.match_grid(occ, grid, cand, fmap_of(mgrid), fused, 4, 4, want_scores=True)
    check((best, scores), mr.match(occ, grid, cand, mgrid, fused, 4, 4), "a fused frame")
    cells = int((occ == 100).sum())
    assert best[0].tolist() == (cells * fr.PAR[0], 0, -2, -3, cells)
    assert pwpp_hip.match_pose(cand[0], 0.5, -2, -3).tolist() == list(true_pose)


# ---- pwpp_match_obstacles ------------------------------------------------------------------------------------------------------
def test_match_obstacles_is_rasterize_plus_visibility_plus_match_grid():
    frames = three_frames()  # a 16-beam scan, an empty frame, a frame that is all unref
    grid = (-16.0, -16.0, 0.5, 64, 64)
    mgrid = (-20.0, -18.0, 0.5, 80, 72)
    fm = fmap_of(mgrid)
    xy = np.array([[0.0, 0.0], [3.3, -2.1], [-15.9, 15.9]])
    poses = [fr.rigid(0.1 * f, 0.5 * f, -0.25 * f) for f in range(3)]
    cand = np.array([pwpp_hip.yaw_candidates(fr.rigid(0.1 * f + 0.04, 0.5 * f + 1.0, -0.25 * f - 0.5), 0.02, 5) for f in range(3)])
    L = pwpp_hip.load()
    h = pwpp_hip.Handle()
    g = pwpp_hip.GroundGrid(*grid, 0, 0)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    best_buf, zero, some = np.zeros(3, mr.BEST_DTYPE), np.zeros(2, np.float64), np.zeros(mgrid[3] * mgrid[4], np.int16)
    assert L.pwpp_match_obstacles(h._h, ctypes.byref(g), BAND[0], BAND[1], 1, vp(zero), 1, 0, 0, 1, pwpp_hip.MEM_HOST, vp(cand), 1, 5, None, ctypes.byref(fm), 1,
                                  vp(some), 2, 2, vp(best_buf), None, None) == E_STATE
    h.set_labels(True)  # (_everything reads them)
    h.estimate_ground_batch(frames, mode=pwpp_hip.MODE_FRESH)
    before = _everything(h, 3)
    maps, _ = h.fuse_obstacles(*grid, *BAND, poses, fm, 3, None, xy)   # a map per frame, fused under the true poses
    for min_count, max_range in ((1, 40), (2, 0)):
        what = "min_count %d, max_range %d" % (min_count, max_range)
        _, vocc = h.visibility_obstacles(*grid, *BAND, xy, min_count, max_range)
        steps = h.match_grid(vocc, grid[:3], cand, fm, maps, 4, 3, want_scores=True)
        got = both_paths(h, lambda: h.match_obstacles(*grid, *BAND, cand, fm, maps, 4, 3, xy, min_count, max_range, want_scores=True, want_frames=True))
        assert got[2].tobytes() == vocc.tobytes(), what + ": the per-frame bytes differ from the visibility's"
        assert got[0].tobytes() == steps[0].tobytes() and got[1].tobytes() == steps[1].tobytes(), what + ": differs from the three steps"
        kept = h.match_obstacles(*grid, *BAND, cand, fm, maps, 4, 3, xy, min_count, max_range)  # the bytes kept in the handle, no scores
        assert kept.tobytes() == got[0].tobytes(), what
        check(got[:2], mr.match(vocc, grid[:3], cand, mgrid, maps, 4, 3), what)
    assert got[0]["cells"][0] >= 3 and got[0]["cells"][1:].tolist() == [0, 0] and got[0][1].tolist() == (0, 0, 0, 0, 0)
    # entry i belongs to frame frame_first + i; one map for the frames named
    sub = h.match_obstacles(*grid, *BAND, cand[1:], fm, maps[1:], 4, 3, xy[1:], 2, 0, frame_first=1, frames=2)
    assert sub.tobytes() == got[0][1:].tobytes()
    # into device memory: the map one halfword off a 256-byte boundary, the frames' bytes kept and asked for one byte off
    import torch
    n_scores = 3 * 5 * 7 * 9
    dmap = torch.full((maps.size + 256,), -7, dtype=torch.int16, device="cuda")
    dmap[1:1 + maps.size] = torch.from_numpy(maps.reshape(-1).copy()).cuda()
    dbest = torch.full((9 + 16,), -7, dtype=torch.int64, device="cuda")
    dscores = torch.full((n_scores + 16,), -7, dtype=torch.int64, device="cuda")
    docc = torch.full((3 * 64 * 64 + 512,), -7, dtype=torch.int8, device="cuda")
    torch.cuda.synchronize()
    for occ_ptr in (0, docc.data_ptr() + 1):
        h.match_obstacles_device(*grid, *BAND, cand, fm, 3, dmap.data_ptr() + 2, 4, 3, dbest.data_ptr(), dscores.data_ptr(), occ_ptr, xy, 2, 0)
        h.synchronize()
        rbest, rscores = dbest.cpu().numpy(), dscores.cpu().numpy()
        assert rbest[:9].tobytes() == got[0].tobytes() and (rbest[9:] == -7).all()
        assert rscores[:n_scores].tobytes() == got[1].tobytes() and (rscores[n_scores:] == -7).all()
    rocc = docc.cpu().numpy()
    assert rocc[1:1 + vocc.size].tobytes() == vocc.tobytes() and rocc[0] == -7 and (rocc[1 + vocc.size:] == -7).all()
    assert _everything(h, 3) == before, "the match changed the results of the call it reads"


def test_two_device_calls_back_to_back_each_match_their_own_tables():
    """The origins, the candidates and the frames' maps of a call are uploaded from the handle's own copy, and the second call
    replaces that copy while the first may still be in flight: two calls with an origin and a candidate set per frame, different
    ones, one synchronize() after both."""
    import torch
    h = pwpp_hip.Handle()
    h.estimate_ground_batch(three_frames(), mode=pwpp_hip.MODE_FRESH)
    grid = (-16.0, -16.0, 0.5, 64, 64)
    mgrid = (-20.0, -18.0, 0.5, 80, 72)
    fm = fmap_of(mgrid)
    xy = np.array([[0.0, 0.0], [3.3, -2.1], [-15.9, 15.9]])
    maps, _ = h.fuse_obstacles(*grid, *BAND, [fr.rigid(0.1 * f, 0.5 * f, -0.25 * f) for f in range(3)], fm, 3, None, xy)
    calls = [(xy, np.array([pwpp_hip.yaw_candidates(fr.rigid(0.1 * f + 0.04, 0.5 * f + 1.0, -0.25 * f - 0.5), 0.02, 5) for f in range(3)])),
             (xy[::-1].copy(), np.array([pwpp_hip.yaw_candidates(fr.rigid(0.1 * f - 0.03, 0.5 * f - 1.5, -0.25 * f + 1.0), 0.03, 5) for f in range(3)]))]
    want = [mr.match(h.visibility_obstacles(*grid, *BAND, o)[1], grid[:3], cand, mgrid, maps, 4, 3) for o, cand in calls]
    assert want[0][1].tobytes() != want[1][1].tobytes() and want[0][0]["cells"][0] >= 3
    n_scores = 3 * 5 * 7 * 9
    dmap = torch.from_numpy(maps.reshape(-1).copy()).cuda()
    out = [(torch.full((9,), -7, dtype=torch.int64, device="cuda"), torch.full((n_scores,), -7, dtype=torch.int64, device="cuda")) for _ in calls]
    torch.cuda.synchronize()
    for (o, cand), (dbest, dscores) in zip(calls, out):
        h.match_obstacles_device(*grid, *BAND, cand, fm, 3, dmap.data_ptr(), 4, 3, dbest.data_ptr(), dscores.data_ptr(), 0, o)
    h.synchronize()
    for i, (dbest, dscores) in enumerate(out):
        check((np.frombuffer(dbest.cpu().numpy().tobytes(), mr.BEST_DTYPE), dscores.cpu().numpy().reshape(want[i][1].shape)), want[i], "call %d of two" % i)


# ---- workspace ------------------------------------------------------------------------------------------------------------------
def test_workspace_and_that_nothing_else_moves():
    h = pwpp_hip.Handle()
    empty = h.workspace_bytes()
    occ, grid, cand, mgrid, maps, wx, wy, mof, want = case(70, 67, 3, 33, 31, 2, 11)
    check(on_host(h, occ, grid, cand, mgrid, maps, wx, wy, mof), want, "before any estimate call")
    grown = h.workspace_bytes()
    # the candidates and the frames' maps, the cell list, the staged frames, the maps and the scores in words
    assert grown >= empty + 4 * (12 * cand.shape[0] * cand.shape[1] + len(occ) + occ.size + occ.size // 4 + maps.size // 2 + 2 * want[1].size), "the cluster buffer is not counted"
    h.trim_workspace()
    assert h.workspace_bytes() == empty, "pwpp_trim_workspace did not free the cluster buffer"
    # with the feature unused nothing is allocated; with it used nothing of the estimate path moves
    a, b = pwpp_hip.Handle(), pwpp_hip.Handle()
    frames = three_frames()
    for w in (a, b):
        w.set_labels(True)
        w.set_order(pwpp_hip.ORDER_CLOUD)  # (a deterministic order of the index lists: two calls are compared below)
        w.estimate_ground_batch(frames, mode=pwpp_hip.MODE_FRESH)
    assert a.workspace_bytes() == b.workspace_bytes()
    before, t_before = _everything(b, 3), b.time_us()
    fm = fmap_of((-20.0, -20.0, 0.5, 80, 80))
    b.match_obstacles(-20.0, -20.0, 0.5, 80, 80, *BAND, [fr.IDENTITY], fm, np.zeros((3, 80, 80), np.int16), 2, 2)
    assert b.workspace_bytes() >= a.workspace_bytes() + 4 * (2 * 3 * 80 * 80 + 3 * 80 * 80 // 4 + 3 * 80 * 80)  # the kept count, first and byte images, the cell list
    assert _everything(b, 3) == before and b.time_us() == t_before, "the match changed the results of the call it reads"
    for w in (a, b):
        w.estimate_ground_batch(frames, mode=pwpp_hip.MODE_FRESH)
    assert _everything(b, 3) == _everything(a, 3), "an estimate call after a match differs from one without"
    b.trim_workspace()
    a.trim_workspace()
    assert a.workspace_bytes() == b.workspace_bytes()
    with pytest.raises(pwpp_hip.PwppError):
        h.set_option("match_path", 3)


def test_pybind_module_agrees_with_the_ctypes_handle():
    import pypatchworkpp
    pp = pypatchworkpp.patchworkpp(pypatchworkpp.Parameters())
    h = pwpp_hip.Handle()
    m = pypatchworkpp.FusedObstacleMap()
    m.x0, m.y0, m.cell, m.nx, m.ny = -32.0, -14.0, 0.5, 130, 56
    pose = fr.rigid(0.2, 1.0, -0.5)
    cand = pwpp_hip.yaw_candidates(fr.rigid(0.16, 2.0, -1.5), 0.02, 5)
    with pytest.raises(RuntimeError):
        pp.matchObstacleMap(m, [tuple(c) for c in cand], 4, 4, -30.0, -12.0, 0.5, 120, 48, 0.2, 2.5)  # no map yet
    pts = small_cloud(5)
    pp.estimateGround(pts)
    h.estimate_ground(pts)
    L1, _ = pp.updateObstacleMap(m, pose, -30.0, -12.0, 0.5, 120, 48, 0.2, 2.5)
    got = pp.matchObstacleMap(m, [tuple(c) for c in cand], 4, 4, -30.0, -12.0, 0.5, 120, 48, 0.2, 2.5)
    fm = fmap_of((-32.0, -14.0, 0.5, 130, 56))
    best = h.match_obstacles(-30.0, -12.0, 0.5, 120, 48, 0.2, 2.5, cand, fm, L1, 4, 4)
    assert got[:5] == (best[0]["candidate"], best[0]["sx"], best[0]["sy"], best[0]["score"], best[0]["cells"]) and got[4] >= 3
    assert list(got[5]) == pwpp_hip.match_pose(cand[got[0]], 0.5, got[1], got[2]).tolist()
