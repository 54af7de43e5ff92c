"""No-GPU checks of two sentences that many pwpp_*_grid entry points share, word for word: the count of something given "1 or one per
frame" (origins, sources, start sets, candidate sets, and the poses of the fusion, the elevation fusion, the association and the map
evidence), and a cell of a list that lies outside the image (the visibility's origins, the sources of the reach, the routes and the
plan).  One loop each feeds the same bad values to every entry point and compares the WHOLE sentence.  A handle that is never
dereferenced and mem = 2 (PWPP_MEM_HOST_PINNED, which none of them takes) reach every check in front of mem without a device, as in
tests/test_tracks_cpu.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import pwpp_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "patchwork-plusplus_amd")
E_ARG = -1
NX, NY, MAX_FRAMES = 5, 4, 3


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(pwpp_hip.LIB_PATH):
        subprocess.run(["make", "-C", PKG, "lib/libpwpp_hip.so"], check=True, stdout=subprocess.DEVNULL)
    return pwpp_hip.load()


def vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


class Calls:
    """Every entry point with arguments that pass all its checks up to mem; a test overrides the count or the list it is about."""

    def __init__(self, lib):
        self.lib = lib
        self.fake = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(8)))  # (never dereferenced: these checks come first)
        cells = MAX_FRAMES * NX * NY
        self.i32 = [np.zeros(cells, np.int32) for _ in range(4)]       # count / dist2 / label, first / reach, from, prev
        self.i8 = [np.zeros(cells, np.int8) for _ in range(2)]         # cost / occupancy
        self.f32 = np.zeros(cells, np.float32)                         # height
        self.cell_list = np.zeros((MAX_FRAMES, 2), np.int32)           # origins, sources, starts: cell (0, 0)
        self.poses = np.tile(np.array([1.0, 0.0, 0.0, 0.0, 1.0, 0.0]), (MAX_FRAMES, 1))
        self.routes = np.zeros(MAX_FRAMES, pwpp_hip.ROUTE_DTYPE)
        self.map16, self.map16_out = np.zeros(NX * NY, np.int16), np.zeros(NX * NY, np.int16)
        self.sum_out = np.zeros(NX * NY, np.int32)
        self.best = np.zeros(MAX_FRAMES, pwpp_hip.MATCH_BEST_DTYPE)
        self.links = [np.zeros(MAX_FRAMES * 2, pwpp_hip.CLUSTER_LINK_DTYPE) for _ in range(2)]
        self.rows = np.zeros(MAX_FRAMES * 2, pwpp_hip.CLUSTER_EVIDENCE_DTYPE)
        self.grid = pwpp_hip.GroundGrid(x0=-2.0, y0=-2.0, cell=1.0, nx=NX, ny=NY, flags=0, pad_=0)
        self.fmap = pwpp_hip.FusionMap(x0=-2.0, y0=-2.0, cell=1.0, nx=NX, ny=NY, hit=10, miss=5, l_min=-100, l_max=100, occupied_at=20, free_at=-20)
        self.hmap = pwpp_hip.HeightMap(x0=-2.0, y0=-2.0, cell=1.0, nx=NX, ny=NY, n_max=8, pad_=0)
        self.reach = pwpp_hip.ReachParams(base=1, lethal=101, unknown=-1, clearance2=0, max_reach=0, pad_=0)
        self.route = pwpp_hip.RouteParams(max_cells=0, max_waypoints=0, look=1, line_cost=0)
        self.rule = pwpp_hip.EvidenceRule(gate=0, min_cells=1, moving_share=128, static_share=128)

    def visibility(self, frames=1, origin=None, n=1):
        return self.lib.pwpp_visibility_grid(self.fake, NX, NY, frames, 2, vp(self.i32[0]), 1, vp(self.cell_list if origin is None else origin), n, 0, vp(self.i32[1]), None)

    def reach_grid(self, frames=1, source=None, n=1):
        return self.lib.pwpp_reach_grid(self.fake, NX, NY, frames, 2, vp(self.i8[0]), None, ctypes.byref(self.reach), vp(self.cell_list if source is None else source), n,
                                        vp(self.i32[1]), None)

    def route_grid(self, frames=1, source=None, n=1, n_sets=1):
        return self.lib.pwpp_route_grid(self.fake, NX, NY, frames, 2, vp(self.i8[0]), None, ctypes.byref(self.reach), vp(self.cell_list if source is None else source), n,
                                        vp(self.i32[2]), vp(self.cell_list), n_sets, 1, ctypes.byref(self.route), vp(self.routes), None, None)

    def plan_grid(self, frames=1, source=None, n=1, n_sets=1):
        return self.lib.pwpp_plan_grid(self.fake, NX, NY, frames, 2, vp(self.i8[0]), None, ctypes.byref(self.reach), vp(self.cell_list if source is None else source), n,
                                       vp(self.cell_list), n_sets, 1, ctypes.byref(self.route), vp(self.routes), None, None, None, None)

    def match_grid(self, frames=1, n=1):
        return self.lib.pwpp_match_grid(self.fake, ctypes.byref(self.grid), frames, 2, vp(self.i8[0]), vp(self.poses), n, 1, None, ctypes.byref(self.fmap), 1, vp(self.map16),
                                        0, 0, vp(self.best), None)

    def fuse_grid(self, frames=1, n=1):
        return self.lib.pwpp_fuse_grid(self.fake, ctypes.byref(self.grid), frames, 2, vp(self.i8[0]), vp(self.poses), n, None, ctypes.byref(self.fmap), 1, None, None,
                                       vp(self.map16_out), None)

    def fuse_height_grid(self, frames=1, n=1):
        return self.lib.pwpp_fuse_height_grid(self.fake, ctypes.byref(self.grid), frames, 2, vp(self.f32), vp(self.poses), None, n, None, ctypes.byref(self.hmap), 1, None,
                                              None, None, vp(self.sum_out), vp(self.map16_out), None)

    def associate_grid(self, frames=1, n=1):
        g = ctypes.byref(self.grid)
        return self.lib.pwpp_associate_grid(self.fake, g, g, frames, 2, vp(self.i32[0]), vp(self.i32[3]), vp(self.poses), n, 0, 1, 2, 2, vp(self.links[0]), vp(self.links[1]),
                                            None, None, None, None, None)

    def evidence_grid(self, frames=1, n=1):
        return self.lib.pwpp_evidence_grid(self.fake, ctypes.byref(self.grid), frames, 2, vp(self.i32[0]), None, vp(self.poses), n, None, ctypes.byref(self.fmap), 1,
                                           vp(self.map16), ctypes.byref(self.rule), 2, vp(self.rows), None, None)


@pytest.fixture(scope="module")
def calls(lib):
    return Calls(lib)


# (entry point, the argument that carries the count, the noun of the sentence)
PER_FRAME = [("visibility", "n", "origins"), ("reach_grid", "n", "sources"), ("route_grid", "n", "sources"), ("plan_grid", "n", "sources"),
             ("route_grid", "n_sets", "start sets"), ("plan_grid", "n_sets", "start sets"), ("match_grid", "n", "candidate sets"), ("fuse_grid", "n", "poses"),
             ("fuse_height_grid", "n", "poses"), ("associate_grid", "n", "poses"), ("evidence_grid", "n", "poses")]


def test_every_call_passes_every_check_in_front_of_mem(lib, calls):
    """The arguments the loops start from are good ones: each call gets as far as mem, so a sentence below is the only thing wrong."""
    for name in sorted({c[0] for c in PER_FRAME}):
        for frames in (1, MAX_FRAMES):
            assert getattr(calls, name)(frames=frames) == E_ARG and b"mem 2: " in lib.pwpp_last_error() and b"PWPP_MEM_HOST or PWPP_MEM_DEVICE" in lib.pwpp_last_error(), name


@pytest.mark.parametrize("name,arg,noun", PER_FRAME, ids=["%s-%s" % (c[0], c[2].replace(" ", "_")) for c in PER_FRAME])
def test_one_or_one_per_frame_is_one_sentence_with_its_noun(lib, calls, name, arg, noun):
    for n, frames in ((0, 1), (2, 1), (2, 3), (-1, 1)):
        assert getattr(calls, name)(frames=frames, **{arg: n}) == E_ARG, (name, n, frames)
        assert lib.pwpp_last_error().decode() == "%d %s for %d frames: 1 or one per frame expected" % (n, noun, frames), (name, n, frames)
    for n, frames in ((1, 1), (1, 3), (3, 3)):  # the two good counts
        assert getattr(calls, name)(frames=frames, **{arg: n}) == E_ARG and b"mem 2: " in lib.pwpp_last_error(), (name, n, frames)


CELL_LISTS = [("visibility", "origin", "origin"), ("reach_grid", "source", "source"), ("route_grid", "source", "source"), ("plan_grid", "source", "source")]


@pytest.mark.parametrize("name,arg,noun", CELL_LISTS, ids=[c[0] for c in CELL_LISTS])
def test_a_cell_outside_is_one_sentence_with_its_index(lib, calls, name, arg, noun):
    for x, y in ((-1, 0), (NX, 0), (0, -1), (0, NY)):
        for n, at in ((1, 0), (MAX_FRAMES, MAX_FRAMES - 1), (MAX_FRAMES, 1)):  # one for all; one per frame, the last and a middle one
            cells = np.zeros((n, 2), np.int32)
            cells[at] = (x, y)
            assert getattr(calls, name)(frames=n, n=n, **{arg: cells}) == E_ARG, (name, x, y, n, at)
            assert lib.pwpp_last_error().decode() == "%s %d, cell (%d, %d), lies outside the %d x %d cells" % (noun, at, x, y, NX, NY), (name, x, y, n, at)
    corners = np.array([[0, 0], [NX - 1, NY - 1], [NX - 1, 0]], np.int32)  # the outermost cells inside
    assert getattr(calls, name)(frames=MAX_FRAMES, n=MAX_FRAMES, **{arg: corners}) == E_ARG and b"mem 2: " in lib.pwpp_last_error()
    first_bad = np.array([[0, NY], [-1, 0], [0, 0]], np.int32)  # the first bad cell of a list is the one named
    assert getattr(calls, name)(frames=MAX_FRAMES, n=MAX_FRAMES, **{arg: first_bad}) == E_ARG
    assert lib.pwpp_last_error().decode() == "%s 0, cell (0, %d), lies outside the %d x %d cells" % (noun, NY, NX, NY)
