"""No-GPU checks of the correlative scan match (pwpp_match_grid, pwpp_match_obstacles, pwpp_match_pose): the exports, the feature
macro, the size of pwpp_match_best, the ctypes prototypes and the bindings' methods, every argument check that needs no device with
its message and its place in the order, pwpp_match_pose's two roundings, the C++ mirror in both flavours -- the properties of the
restatement the GPU tests compare against (tests/scan_match_ref.py): a frame fused under a whole-cell translation or a quarter turn
matches at its own pose and nowhere else, the tie order, skipped and empty frames, a candidate that is not finite, a sum beyond
int32, and the recovery of a displaced prior on a committed list of random wall scenes -- and the stand-alone program that runs the
kernels' functions on the host against a brute force of its own (tools/match_check.cpp), built with the address and undefined-
behaviour sanitizers where the toolchain has them."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import occupancy_fusion_ref as fr
import pwpp_hip
import scan_match_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "patchwork-plusplus_amd")
E_ARG = -1


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(pwpp_hip.LIB_PATH):
        subprocess.run(["make", "-C", PKG, "lib/libpwpp_hip.so"], check=True, stdout=subprocess.DEVNULL)
    return pwpp_hip.load()


def test_symbols_macro_struct_and_prototypes(lib):
    hdr = open(os.path.join(ROOT, "include", "pwpp.h")).read()
    for name in ("pwpp_match_grid", "pwpp_match_obstacles", "pwpp_match_pose"):
        assert hasattr(lib, name), name
        assert "PWPP_API int %s(" % name in hdr
    assert "#define PWPP_HAS_SCAN_MATCH 1" in hdr
    assert "#define PWPP_VERSION_MINOR 4 " in hdr
    assert '"match_path"' in hdr and "typedef struct pwpp_match_best {" in hdr
    assert ctypes.sizeof(pwpp_hip.MatchBest) == 24 and ctypes.alignment(pwpp_hip.MatchBest) == 8
    assert [f[0] for f in pwpp_hip.MatchBest._fields_] == ["score", "candidate", "sx", "sy", "cells"]
    assert pwpp_hip.MATCH_BEST_DTYPE.itemsize == 24 and pwpp_hip.MATCH_BEST_DTYPE == mr.BEST_DTYPE
    assert [pwpp_hip.MATCH_BEST_DTYPE.fields[n][1] for n in ("score", "candidate", "sx", "sy", "cells")] == [0, 8, 12, 16, 20]
    assert len(lib.pwpp_match_grid.argtypes) == 16 and len(lib.pwpp_match_obstacles.argtypes) == 23 and len(lib.pwpp_match_pose.argtypes) == 5
    assert lib.pwpp_match_obstacles.argtypes[2] is ctypes.c_float and lib.pwpp_match_obstacles.argtypes[3] is ctypes.c_float
    assert lib.pwpp_match_pose.argtypes[1] is ctypes.c_double
    for name in ("match_grid", "match_grid_device", "match_obstacles", "match_obstacles_device"):
        assert callable(getattr(pwpp_hip.Handle, name)), name
    assert callable(pwpp_hip.match_pose) and callable(pwpp_hip.yaw_candidates)
    import pypatchworkpp
    assert hasattr(pypatchworkpp.patchworkpp, "matchObstacleMap")


def fusion_map(**kw):
    f = dict(x0=-2.0, y0=-2.0, cell=1.0, nx=4, ny=4, hit=40, miss=20, l_min=-200, l_max=350, occupied_at=60, free_at=-40)
    f.update(kw)
    return pwpp_hip.FusionMap(**f)


def test_every_argument_is_named_before_the_device_is_touched_and_in_order(lib):
    occ = np.zeros(64, np.int8)
    maps = np.zeros(64, np.int16)
    best = np.zeros(8, mr.BEST_DTYPE)
    scores = np.zeros(4096, np.int64)
    cand = np.array(fr.IDENTITY * 256, np.float64)   # (the largest set a call below copies)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    at = lambda a, n: ctypes.c_void_p(a.ctypes.data + n)
    fake = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(8)))  # (never dereferenced: these checks come first)
    H, D = pwpp_hip.MEM_HOST, pwpp_hip.MEM_DEVICE
    err = lib.pwpp_last_error
    g = pwpp_hip.GroundGrid(-2.0, -2.0, 1.0, 4, 4, 0, 0)
    fm = fusion_map()

    def grid(h=fake, gr=ctypes.byref(g), frames=1, mem=2, occupancy=vp(occ), candidates=vp(cand), n_sets=1, n_candidates=1, mof=None, m=ctypes.byref(fm),
             n_maps=1, map_=vp(maps), wx=1, wy=1, best_=vp(best), scores_=vp(scores)):
        return lib.pwpp_match_grid(h, gr, frames, mem, occupancy, candidates, n_sets, n_candidates, mof, m, n_maps, map_, wx, wy, best_, scores_)

    def G(**kw):
        return ctypes.byref(pwpp_hip.GroundGrid(**dict(dict(x0=-2.0, y0=-2.0, cell=1.0, nx=4, ny=4, flags=0, pad_=0), **kw)))

    M = lambda **kw: ctypes.byref(fusion_map(**kw))
    # (the default mem is PWPP_MEM_HOST_PINNED, the last but one check: a call that gets that far has passed everything before it)
    PINNED = b"PWPP_MEM_HOST or PWPP_MEM_DEVICE"
    assert grid() == E_ARG and PINNED in err() and b"the scan match takes" in err()
    # 1 null pointers
    assert grid(h=None) == E_ARG and b"null handle" in err()
    assert grid(gr=None) == E_ARG and b"null grid" in err()
    assert grid(occupancy=None) == E_ARG and b"null occupancy" in err()
    assert grid(candidates=None) == E_ARG and b"null candidates" in err()
    assert grid(m=None) == E_ARG and b"null map description" in err()
    assert grid(map_=None) == E_ARG and b"null map" in err() and b"description" not in err()
    assert grid(best_=None) == E_ARG and b"null best" in err()
    assert grid(scores_=None) == E_ARG and PINNED in err()   # the scores may be absent
    # 2 the frame images: frames and sides < 1, sides > 32768, the cells beyond 2^31; the flags
    for kw in (dict(frames=0), dict(gr=G(nx=0)), dict(gr=G(ny=-1))):
        assert grid(**kw) == E_ARG and b"cells" in err(), kw
    for kw in (dict(nx=32769), dict(ny=32769)):
        assert grid(gr=G(**kw)) == E_ARG and b"32768 a side" in err(), kw
    assert grid(gr=G(nx=32768, ny=32768), frames=3, n_sets=3) == E_ARG and b"exceed 2^31" in err()
    assert grid(gr=G(flags=1)) == E_ARG and b"grid flags 1" in err()
    # 3 the same of the maps
    for kw in (dict(n_maps=0), dict(m=M(nx=0)), dict(m=M(ny=0))):
        assert grid(**kw) == E_ARG and b"cells" in err(), kw
    for kw in (dict(nx=32769), dict(ny=40000)):
        assert grid(m=M(**kw)) == E_ARG and b"32768 a side" in err(), kw
    assert grid(m=M(nx=32768, ny=32768), n_maps=3) == E_ARG and b"exceed 2^31" in err()
    # 4 the cell sizes
    for c in (0.0, -1.0, np.nan, np.inf):
        assert grid(gr=G(cell=c)) == E_ARG and b"finite and positive" in err(), c
        assert grid(m=M(cell=c)) == E_ARG and b"finite and positive" in err(), c
    assert grid(m=M(hit=-1, miss=99999, l_min=7, free_at=99)) == E_ARG and PINNED in err()   # only x0, y0, cell, nx, ny are read
    # 5 the candidates, 6 the sets, 7 the window
    for n in (0, -1, 257):
        assert grid(n_candidates=n) == E_ARG and b"candidates: 1 .. 256 expected" in err(), n
    assert grid(n_candidates=256, scores_=None) == E_ARG and PINNED in err()
    for n in (0, 2, -1):
        assert grid(n_sets=n) == E_ARG and b"candidate sets for 1 frames" in err(), n
    assert grid(frames=4, n_sets=3) == E_ARG and b"3 candidate sets for 4 frames" in err()
    assert grid(frames=4, n_sets=4) == E_ARG and PINNED in err()
    for kw in (dict(wx=-1), dict(wx=65), dict(wy=-1), dict(wy=65)):
        assert grid(**kw) == E_ARG and b"0 .. 64 cells expected" in err(), kw
    assert grid(wx=64, wy=64) == E_ARG and PINNED in err() and grid(wx=0, wy=0) == E_ARG and PINNED in err()
    # 8 frames x candidates, 9 the scores' element count
    one = G(nx=1, ny=1)
    assert grid(gr=one, frames=(1 << 16) + 1, n_candidates=256, scores_=None) == E_ARG and b"exceed 2^24" in err()
    assert grid(gr=one, frames=1 << 16, n_candidates=256, wx=5, wy=6, scores_=None) == E_ARG and PINNED in err()
    assert grid(gr=one, frames=1 << 16, n_candidates=256, wx=5, wy=6) == E_ARG and b"the scores exceed 2^31 elements" in err()   # 2^24 x 143
    assert grid(gr=one, frames=1 << 16, n_candidates=256, wx=5, wy=6, n_maps=1 << 16) == E_ARG and b"the scores exceed" in err()
    assert grid(gr=one, frames=1 << 16, n_candidates=256, wx=5, wy=5) == E_ARG and PINNED in err()   # 2^24 x 121 < 2^31
    assert grid(gr=one, frames=1 << 15, n_candidates=256, wx=7, wy=8) == E_ARG and PINNED in err()   # 2^23 x 255 < 2^31; x 256 would be 2^31: allowed too
    # 10 map_of_frame
    assert grid(frames=3, n_maps=2) == E_ARG and b"null map_of_frame with 2 maps for 3 frames" in err()
    for bad, where in (([0, 1, 2], b"map_of_frame 2 names map 2"), ([0, -2, 1], b"map_of_frame 1 names map -2")):
        assert grid(frames=3, n_maps=2, mof=vp(np.array(bad, np.int32))) == E_ARG and where in err(), bad
    assert grid(frames=3, n_maps=2, mof=vp(np.array([1, -1, 0], np.int32))) == E_ARG and PINNED in err()
    # 11 mem, 12 the alignment of the results in device memory (the map: 2 bytes, the bytes: 1 -- not looked at)
    assert grid(mem=7) == E_ARG and b"mem 7" in err()
    assert grid(candidates=vp(np.full(6, np.nan)), mem=2) == E_ARG and PINNED in err()   # a candidate that is not finite is no error
    assert grid(mem=D, best_=at(best, 4)) == E_ARG and b"best rows must be 8-byte aligned" in err()
    assert grid(mem=D, scores_=at(scores, 4)) == E_ARG and b"scores must be 8-byte aligned" in err()
    assert grid(mem=D, best_=at(best, 4), scores_=at(scores, 2)) == E_ARG and b"best rows" in err()
    # the order
    assert grid(occupancy=None, frames=0) == E_ARG and b"null occupancy" in err()
    assert grid(frames=0, n_maps=0) == E_ARG and b"0 frames of 4 x 4" in err()
    assert grid(gr=G(nx=32769), m=M(nx=0)) == E_ARG and b"32768 a side" in err()
    assert grid(gr=G(cell=0.0, flags=1)) == E_ARG and b"grid flags" in err()   # the frame grid's own checks come before the map's
    assert grid(n_maps=0, gr=G(cell=0.0)) == E_ARG and b"0 frames of 4 x 4" in err()   # (the maps' own "frames" are the maps)
    assert grid(m=M(cell=0.0), n_candidates=0) == E_ARG and b"finite and positive" in err()
    assert grid(n_candidates=0, n_sets=0) == E_ARG and b"candidates: 1 .. 256" in err()
    assert grid(n_sets=0, wx=99) == E_ARG and b"candidate sets" in err()
    assert grid(wx=99, gr=one, frames=(1 << 16) + 1, n_sets=(1 << 16) + 1, n_candidates=256) == E_ARG and b"0 .. 64" in err()
    assert grid(gr=one, frames=(1 << 16) + 1, n_sets=(1 << 16) + 1, n_candidates=256, wx=5, wy=6) == E_ARG and b"exceed 2^24" in err()
    assert grid(gr=one, frames=1 << 16, n_candidates=256, wx=5, wy=6, n_maps=2) == E_ARG and b"the scores exceed" in err()
    assert grid(frames=3, n_maps=2, mem=7) == E_ARG and b"null map_of_frame" in err()
    assert grid(mem=7, best_=at(best, 4)) == E_ARG and b"mem 7" in err()

    zero2 = np.zeros(2, np.float64)

    def obstacles(h=fake, gr=ctypes.byref(g), band=(0.2, 2.5), min_count=1, origin=vp(zero2), n_origins=1, max_range=0, frames=1, candidates=vp(cand),
                  n_sets=1, n_candidates=1, mof=None, m=ctypes.byref(fm), n_maps=1, map_=vp(maps), wx=1, wy=1, best_=vp(best)):
        return lib.pwpp_match_obstacles(h, gr, band[0], band[1], min_count, origin, n_origins, max_range, 0, frames, H, candidates, n_sets, n_candidates,
                                        mof, m, n_maps, map_, wx, wy, best_, None, None)

    assert obstacles(h=None) == E_ARG and b"null handle" in err()
    assert obstacles(gr=None) == E_ARG and b"null grid" in err()
    assert obstacles(origin=None) == E_ARG and b"null origin" in err()
    assert obstacles(candidates=None) == E_ARG and b"null candidates" in err()
    assert obstacles(m=None) == E_ARG and b"null map description" in err()
    assert obstacles(map_=None) == E_ARG and b"null map" in err()
    assert obstacles(best_=None) == E_ARG and b"null best" in err()
    # everything pwpp_visibility_obstacles rejects, first
    assert obstacles(band=(2.5, 0.2)) == E_ARG and b"height band" in err()
    assert obstacles(gr=G(flags=2)) == E_ARG and b"grid flags" in err()
    for kw in (dict(nx=0), dict(cell=0.0), dict(cell=np.nan), dict(x0=np.inf)):
        assert obstacles(gr=G(**kw)) == E_ARG and (b"grid of" in err() or b"finite" in err()), kw
    assert obstacles(gr=G(nx=32769)) == E_ARG and b"32768 a side" in err()
    assert obstacles(min_count=0) == E_ARG and b"min_count" in err()
    assert obstacles(max_range=32769) == E_ARG and b"max_range" in err()
    assert obstacles(n_origins=2) == E_ARG and b"2 origins for 1 frames" in err()
    assert obstacles(origin=vp(np.array((2.0, 0.0)))) == E_ARG and b"origin 0" in err() and b"outside the grid" in err()
    assert obstacles(origin=vp(np.array((np.nan, 0.0)))) == E_ARG and b"not finite" in err()
    # then the map's and the match's
    assert obstacles(frames=0, n_origins=1) == E_ARG and b"0 frames" in err()
    assert obstacles(n_maps=0) == E_ARG and b"cells" in err()
    assert obstacles(m=M(cell=-1.0)) == E_ARG and b"finite and positive" in err()
    assert obstacles(n_candidates=300) == E_ARG and b"1 .. 256" in err()
    assert obstacles(n_sets=2) == E_ARG and b"2 candidate sets for 1 frames" in err()
    assert obstacles(wy=70) == E_ARG and b"0 .. 64" in err()
    assert obstacles(mof=vp(np.array([1], np.int32))) == E_ARG and b"map_of_frame 0 names map 1" in err()
    assert obstacles(min_count=0, n_candidates=0) == E_ARG and b"min_count" in err()


def test_match_pose_rounds_one_product_and_one_sum(lib):
    rng = np.random.default_rng(3)
    for _ in range(200):
        cand = rng.uniform(-50, 50, 6)
        cell = float(rng.choice([0.3, 0.5, 0.1, 1.0 / 3.0, 0.25]))
        sx, sy = int(rng.integers(-64, 65)), int(rng.integers(-64, 65))
        got = pwpp_hip.match_pose(cand, cell, sx, sy)
        want = mr.match_pose(cand, cell, sx, sy)
        assert got.tobytes() == want.tobytes(), (cand, cell, sx, sy)
    assert pwpp_hip.match_pose((1, 0, 0.3, 0, 1, 0.7), 0.3, 7, -3)[2] == 0.3 + 7.0 * 0.3
    out = np.empty(6)
    assert lib.pwpp_match_pose(None, 0.5, 0, 0, out.ctypes.data_as(ctypes.c_void_p)) == E_ARG and b"null candidate" in lib.pwpp_last_error()
    assert lib.pwpp_match_pose(out.ctypes.data_as(ctypes.c_void_p), 0.5, 0, 0, None) == E_ARG and b"null output pose" in lib.pwpp_last_error()


def test_yaw_candidates_put_the_prior_first_then_alternate():
    prior = fr.rigid(0.3, 1.5, -2.0)
    c = pwpp_hip.yaw_candidates(prior, 0.02, 5)
    assert c.shape == (5, 6) and c[0].tolist() == list(prior)
    for i, k in enumerate((0, 1, -1, 2, -2)):
        assert np.allclose(c[i], fr.rigid(0.3 + 0.02 * k, 1.5, -2.0), rtol=0, atol=1e-14), i
    # a rotation about the FRAME's origin: the translation stays
    assert (c[:, 2] == 1.5).all() and (c[:, 5] == -2.0).all()


CPP = r"""
#include "patchwork/patchworkpp.h"
#ifndef PWPP_HAS_SCAN_MATCH
#error "include/pwpp.h does not announce the scan match"
#endif
static_assert(sizeof(pwpp_match_best) == 24 && alignof(pwpp_match_best) == 8, "pwpp_match_best");
double use(patchwork::PatchWorkpp &pw) {
    patchwork::PatchWorkpp::FusedObstacleMap map;
    map.x0 = -64.0, map.y0 = -64.0, map.cell = 0.5, map.nx = 256, map.ny = 256;
    const double candidates[12] = {1.0, 0.0, 3.0, 0.0, 1.0, -1.5, 0.0, -1.0, 3.0, 1.0, 0.0, -1.5};
    pw.updateObstacleMap(map, candidates, -40.0, -40.0, 0.5, 160, 160, 0.2f, 2.5f);
    const patchwork::PatchWorkpp::ObstacleMatch a = pw.matchObstacleMap(map, candidates, 2, 10, 10, -40.0, -40.0, 0.5, 160, 160, 0.2f, 2.5f);
    const patchwork::PatchWorkpp::ObstacleMatch b = pw.matchObstacleMap(map, candidates, 2, 4, 3, -40.0, -40.0, 0.5, 160, 160, 0.2f, 2.5f, 2, 40, 1.5, -0.5);
    pw.updateObstacleMap(map, a.pose, -40.0, -40.0, 0.5, 160, 160, 0.2f, 2.5f);
    return (double)a.score + a.candidate + a.sx + a.sy + a.cells + b.pose[2];
}
"""


@pytest.mark.parametrize("flavour", ["plain", "eigen_shim"])
def test_cpp_mirror_method_compiles(tmp_path, flavour):
    src = tmp_path / "scan_match.cpp"
    src.write_text(CPP)
    cmd = ["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(PKG, "include"), "-I", os.path.join(ROOT, "include")]
    cmd += ["-DPWPP_NO_EIGEN"] if flavour == "plain" else ["-I", os.path.join(ROOT, "oracle", "eigen_shim")]
    subprocess.run(cmd + [str(src)], check=True)


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "match.c"
    src.write_text('#include "pwpp.h"\nint f(const pwpp_fusion_map *m, pwpp_match_best *b) { return pwpp_match_grid(0, 0, 1, PWPP_MEM_HOST, 0, 0, 1, 1, 0, m, 1, 0, 1, 1, b, 0) + '
                   'pwpp_match_obstacles(0, 0, 0.f, 1.f, 1, 0, 1, 0, 0, 1, PWPP_MEM_HOST, 0, 1, 1, 0, m, 1, 0, 1, 1, b, 0, 0) + pwpp_match_pose(0, 0.5, 1, 1, 0) + '
                   '(int)sizeof(*b) + b->candidate; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)


# ---- the restatement itself ---------------------------------------------------------------------------------------------------
GRID = (-6.0, -6.0, 0.5)             # 24 x 24 frame cells
MGRID = (-16.0, -16.0, 0.5, 64, 64)
QUARTER = (0.0, -1.0, 0.0, 1.0, 0.0, 0.0)


@pytest.mark.parametrize("true_pose, other", [((1.0, 0.0, 1.5, 0.0, 1.0, -2.0), QUARTER), (QUARTER, fr.IDENTITY)])
def test_a_frame_matches_the_map_it_was_fused_into_at_its_own_pose_and_nowhere_else(true_pose, other):
    occ = fr.random_occupancy(1, 24, 24, 7)
    fused, _ = fr.fuse(occ, GRID, true_pose, MGRID)   # hit 40 where occupied, -20 where free, 0 elsewhere: lossless for these poses
    rows, s = mr.match(occ, GRID, [other, true_pose], MGRID, fused, 3, 2)
    cells = int((occ == 100).sum())
    assert cells > 50 and rows[0]["cells"] == cells
    assert s.shape == (1, 2, 5, 7) and s[0, 1, 2, 3] == cells * fr.PAR[0]
    rest = np.delete(s.reshape(-1), np.ravel_multi_index((0, 1, 2, 3), s.shape))
    assert (rest < cells * fr.PAR[0]).all()
    assert rows[0].tolist() == (cells * fr.PAR[0], 1, 0, 0, cells)


def test_the_tie_order():
    g1, m9 = (0.0, 0.0, 1.0), (-4.0, -4.0, 1.0, 9, 9)
    occ = np.full((1, 1, 1), 100, np.int8)   # one occupied cell, centre (0.5, 0.5): lands in map cell (4, 4)
    at = lambda dx, dy: (1.0, 0.0, float(dx), 0.0, 1.0, float(dy))
    # a constant map: every score is equal; the zero shift of the first candidate wins
    rows, s = mr.match(occ, g1, [at(1, 0), at(0, 0)], m9, np.full((1, 9, 9), 7, np.int16), 2, 2)
    assert (s == 7).all() and rows[0].tolist() == (7, 0, 0, 0, 1)
    # four peaks at distance 1: the smaller sy first ...
    peaks = np.zeros((1, 9, 9), np.int16)
    for jx, jy in ((5, 4), (3, 4), (4, 5), (4, 3)):
        peaks[0, jy, jx] = 5
    assert mr.match(occ, g1, [at(0, 0)], m9, peaks, 2, 2)[0][0].tolist() == (5, 0, 0, -1, 1)
    peaks[0, 3, 4] = 0   # ... then, among sy = 0 and sy = 1, sy = 0 and the smaller sx
    assert mr.match(occ, g1, [at(0, 0)], m9, peaks, 2, 2)[0][0].tolist() == (5, 0, -1, 0, 1)
    # the distance comes before the candidate: candidate 0 needs the shift (2, 0), candidate 1 the shift (0, 1)
    one = np.zeros((1, 9, 9), np.int16)
    one[0, 4, 6] = 5
    assert mr.match(occ, g1, [at(0, 0), at(2, -1)], m9, one, 2, 2)[0][0].tolist() == (5, 1, 0, 1, 1)
    # the candidate comes before sy: equal distances
    assert mr.match(occ, g1, [at(1, 0), at(2, -1)], m9, one, 2, 2)[0][0].tolist() == (5, 0, 1, 0, 1)
    # the larger score beats everything
    one[0, 2, 2] = 6
    assert mr.match(occ, g1, [at(0, 0), at(2, -1)], m9, one, 2, 2)[0][0].tolist() == (6, 0, -2, -2, 1)


def test_skipped_empty_and_not_finite():
    occ = fr.random_occupancy(3, 6, 5, 9)
    occ[1] = np.where(occ[1] == 100, 50, occ[1])   # no occupied cell; stray bytes are not occupied
    maps = np.random.default_rng(1).integers(-32768, 32768, (2, 8, 8)).astype(np.int16)
    grid, mgrid = (-1.0, -1.5, 0.5), (-2.0, -2.0, 0.5, 8, 8)
    nan = (1.0, 0.0, np.nan, 0.0, 1.0, 0.0)
    rows, s = mr.match(occ, grid, [nan, fr.IDENTITY, (1.0, 0.0, np.inf, 0.0, 1.0, 0.0)], mgrid, maps, 1, 2, map_of_frame=[1, 0, -1])
    assert (s[1] == 0).all() and rows[1].tolist() == (0, 0, 0, 0, 0)                      # empty: the zero shift of the first candidate
    assert (s[2] == 0).all() and rows[2].tolist() == (0, -1, 0, 0, int((occ[2] == 100).sum()))   # skipped: cells still counted
    assert (s[0, 0] == 0).all() and (s[0, 2] == 0).all() and s[0, 1].any()              # not finite: lands nowhere, scores 0
    assert rows[0]["candidate"] in (0, 1) and rows[0]["cells"] == (occ[0] == 100).sum()
    # a frame all of whose candidates are not finite: like an empty one
    assert mr.match(occ[:1], grid, [nan], mgrid, maps[:1], 1, 1)[0][0].tolist() == (0, 0, 0, 0, int((occ[0] == 100).sum()))


def test_a_sum_beyond_int32():
    occ = np.full((1, 256, 384), 100, np.int8)
    maps = np.full((1, 256, 384), 32767, np.int16)
    rows, s = mr.match(occ, (0.0, 0.0, 0.5), [fr.IDENTITY], (0.0, 0.0, 0.5, 384, 256), maps, 1, 1)
    assert s[0, 0, 1, 1] == 98304 * 32767 and s[0, 0, 1, 1] > 2 ** 31
    assert s[0, 0, 0, 0] == 383 * 255 * 32767 and rows[0].tolist() == (98304 * 32767, 0, 0, 0, 98304)


# ---- the recovery experiment: a displaced prior on a fused map of random walls ----------------------------------------------------
SCAN = (-12.0, -12.0, 0.5)            # 48 x 48 cells about the sensor
WORLD = (-24.0, -24.0, 0.5, 96, 96)
YAW_STEP = 0.02
# A list of inputs, not a pass rate: the seeds of range(40) on which the restatement alone returns the true candidate and shift
# with no tie at the top.  Left out: 10 and 31 (fewer than 20 occupied cells in the fifth scan), 19 and 24 (a tie at the top), and
# 6, 15, 22, 27, 37, 39, where a neighbouring yaw step scores higher -- 0.02 rad moves a wall 12 m away by half a cell.
RECOVERY_SEEDS = [0, 1, 2, 3, 4, 5, 7, 8, 9, 11, 12, 13, 14, 16, 17, 18, 20, 21, 23, 25, 26, 28, 29, 30, 32, 33, 34, 35, 36, 38]


def wall_scan(points, pose):
    """The 48 x 48 occupancy image a sensor at `pose` (theta, tx, ty) sees of the wall points: occupied where a point falls, free
    elsewhere."""
    theta, tx, ty = pose
    c, s = np.cos(theta), np.sin(theta)
    dx, dy = points[:, 0] - tx, points[:, 1] - ty
    fx, fy = c * dx + s * dy, -s * dx + c * dy   # world -> sensor: the transpose
    u, v = np.floor((fx - SCAN[0]) / SCAN[2]).astype(int), np.floor((fy - SCAN[1]) / SCAN[2]).astype(int)
    ok = (u >= 0) & (u < 48) & (v >= 0) & (v < 48)
    occ = np.zeros((48, 48), np.int8)
    occ[v[ok], u[ok]] = 100
    return occ


def recovery_trial(seed):
    rng = np.random.default_rng(1000 + seed)
    walls = []
    for _ in range(6):
        p = rng.uniform(-18, 18, 2)
        ang, length = rng.uniform(0, np.pi), rng.uniform(4, 14)
        t = np.arange(0.0, length, 0.1)
        walls.append(p + np.outer(t, (np.cos(ang), np.sin(ang))))
    points = np.concatenate(walls)
    sensors = [(rng.uniform(-0.3, 0.3), rng.integers(-6, 7) * 0.5, rng.integers(-6, 7) * 0.5) for _ in range(5)]
    scans = np.stack([wall_scan(points, p) for p in sensors])
    fused, _ = fr.fuse(scans[:4], SCAN, [fr.rigid(*p) for p in sensors[:4]], WORLD)
    k, dx, dy = int(rng.integers(-2, 3)), int(rng.integers(-3, 4)), int(rng.integers(-3, 4))
    theta, tx, ty = sensors[4]
    prior = fr.rigid(theta - k * YAW_STEP, tx + dx * 0.5, ty + dy * 0.5)
    cand = pwpp_hip.yaw_candidates(prior, YAW_STEP, 5)
    true_candidate = 0 if k == 0 else (2 * k - 1 if k > 0 else -2 * k)
    return scans[4:], cand, fused, (true_candidate, -dx, -dy)


@pytest.mark.parametrize("seed", RECOVERY_SEEDS)
def test_the_restatement_recovers_a_displaced_prior(seed):
    scan, cand, fused, truth = recovery_trial(seed)
    assert (scan == 100).sum() >= 20
    rows, s = mr.match(scan, SCAN, cand, WORLD, fused, 4, 4)
    top = np.sort(s.reshape(-1))[-2:]
    assert top[1] > top[0], "a tie at the top"
    assert (int(rows[0]["candidate"]), int(rows[0]["sx"]), int(rows[0]["sy"])) == truth


# ---- the kernels' functions on the host ----------------------------------------------------------------------------------------
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"]


def sanitizers_work(tmp_path):
    """The toolchain links the two runtimes into a program and that program starts in this environment."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++"] + SANITIZE + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        return False
    return subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode == 0


def test_match_program_builds_and_passes(tmp_path):
    exe = tmp_path / "match_check"
    flags = SANITIZE if sanitizers_work(tmp_path) else []
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off"] + flags +
                   ["-I", os.path.join(PKG, "csrc"), os.path.join(ROOT, "tools", "match_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)  # (a stand-alone child process with its own main)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 mismatches" in r.stdout
    assert int(r.stdout.split("match_check: ")[1].split(" cases")[0]) >= 3000
