"""No-GPU checks of the routes on the reach field (pwpp_route_grid, pwpp_plan_grid): the exports, the feature macro and its place, the
sizes of pwpp_route_params and pwpp_route, the ctypes prototypes and the bindings' methods, every argument check that needs no device
with its message and its place in the order, the header from C99 and the C++ mirror in both flavours; the properties of the
contract, asked of csrc/pwpp_route.h through route_check's dump mode by both deals and of the restatement (tests/route_ref.py) alike: look = 1 is the route itself, the open field has two waypoints, the
eight symmetries of the square map routes onto routes up to the tie-break of from, judged by rt.certify -- which is shown to refuse a
tied-but-wrong predecessor, a waypoint one too near and one too far; and the stand-alone program that runs the kernels' functions on
the host, dealt as both kernels deal them, against a brute force of its own (tools/route_check.cpp), built with the address and
undefined-behaviour sanitizers where the toolchain has them, whose dump mode is compared byte for byte with the restatement."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import pwpp_hip
import reach_ref as rr
import route_ref as rt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "patchwork-plusplus_amd")
E_ARG = -1


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(pwpp_hip.LIB_PATH):
        subprocess.run(["make", "-C", PKG, "lib/libpwpp_hip.so"], check=True, stdout=subprocess.DEVNULL)
    return pwpp_hip.load()


def test_symbols_macro_structs_and_prototypes(lib):
    hdr = open(os.path.join(ROOT, "include", "pwpp.h")).read()
    for name in ("pwpp_route_grid", "pwpp_plan_grid"):
        assert hasattr(lib, name), name
        assert "PWPP_API int %s(" % name in hdr
    assert "#define PWPP_HAS_ROUTES 1" in hdr and '"route_path"' in hdr
    for k, name in enumerate(("OK", "NONE", "BROKEN")):
        assert "#define PWPP_ROUTE_%s %d\n" % (name, k) in hdr and getattr(pwpp_hip, "ROUTE_" + name) == k == getattr(rt, name)
    assert "typedef struct pwpp_route_params {" in hdr and "typedef struct pwpp_route {" in hdr
    # declared after the costmap and before the input transforms
    assert hdr.index("PWPP_API int pwpp_costmap_curve(") < hdr.index("PWPP_HAS_ROUTES") < hdr.index("PWPP_API int pwpp_route_grid(")
    assert hdr.index("PWPP_API int pwpp_route_grid(") < hdr.index("PWPP_API int pwpp_plan_grid(") < hdr.index("#define PWPP_HAS_INPUT_TRANSFORM")
    assert ctypes.sizeof(pwpp_hip.RouteParams) == 16 and pwpp_hip.ROUTE_DTYPE.itemsize == 32 == rt.ROW.itemsize
    assert [f[0] for f in pwpp_hip.RouteParams._fields_] == ["max_cells", "max_waypoints", "look", "line_cost"]
    assert list(pwpp_hip.ROUTE_DTYPE.names) == ["status", "cells", "cost", "edge_steps", "corner_steps", "max_term", "min_dist2", "waypoints"] == list(rt.ROW.names)
    assert len(lib.pwpp_route_grid.argtypes) == 18 and len(lib.pwpp_plan_grid.argtypes) == 19
    for name in ("route_grid", "route_grid_device", "plan_grid", "plan_grid_device"):
        assert callable(getattr(pwpp_hip.Handle, name)), name
    import pypatchworkpp
    assert hasattr(pypatchworkpp.patchworkpp, "getRoutes") and hasattr(pypatchworkpp.patchworkpp, "planRoutes")
    q = pypatchworkpp.RouteParams()
    assert (q.max_cells, q.max_waypoints, q.look, q.line_cost) == (1024, 64, 64, 0)
    doc = pypatchworkpp.patchworkpp.getRoutes.__doc__
    assert "starts_xy:" in doc and "terrain_params:" in doc and "reach_params:" in doc and "route_params:" in doc and "ground_only: bool = False)" in doc
    doc = pypatchworkpp.patchworkpp.planRoutes.__doc__
    assert "cost:" in doc and "starts_xy:" in doc and "route_params:" in doc and doc.count("= 0.0") == 2
    src = open(os.path.join(PKG, "csrc", "pwpp_route.h")).read()
    assert "#define PWPP_ROUTE_MAX_LOOK 256\n" in src and "#define PWPP_ROUTE_MAX_STARTS 65536\n" in src
    mirror = open(os.path.join(PKG, "include", "patchwork", "patchworkpp.h")).read()
    assert "floor" not in mirror.split("Routes planRoutes(")[1].split("return r;")[0] and "pwpp_grid_cell_of(" in mirror.split("Routes planRoutes(")[1].split("return r;")[0]


def rparams(**kw):
    f = dict(base=1, lethal=100, unknown=-1, clearance2=0, max_reach=0, pad_=0)
    f.update(kw)
    return pwpp_hip.ReachParams(**f)


def qparams(**kw):
    f = dict(max_cells=4, max_waypoints=4, look=8, line_cost=0)
    f.update(kw)
    return pwpp_hip.RouteParams(**f)


def test_every_argument_is_named_before_the_device_is_touched_and_in_order(lib):
    cost = np.zeros(16, np.int8)
    dist2, reach, frm = np.zeros(16, np.int32), np.zeros(16, np.int32), np.zeros(16, np.int32)
    src, start = np.array([[1, 2]], np.int32), np.array([[0, 0], [3, 3]], np.int32)
    rows, cells, wps = np.zeros(2, rt.ROW), np.zeros(8, np.int32), np.zeros(8, np.int32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    at = lambda a, n: ctypes.c_void_p(a.ctypes.data + n)
    fake = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(8)))  # (never dereferenced: these checks come first)
    D = pwpp_hip.MEM_DEVICE
    err = lib.pwpp_last_error
    P = lambda **kw: ctypes.byref(rparams(**kw))
    Q = lambda **kw: ctypes.byref(qparams(**kw))

    def route(h=fake, nx=4, ny=4, frames=1, mem=2, cost=vp(cost), dist2=None, p=P(), source=vp(src), n_sources=1, frm=vp(frm), start=vp(start), sets=1, n=2, q=Q(),
              rows=vp(rows), cells=vp(cells), wps=vp(wps)):
        return lib.pwpp_route_grid(h, nx, ny, frames, mem, cost, dist2, p, source, n_sources, frm, start, sets, n, q, rows, cells, wps)

    def plan(h=fake, nx=4, ny=4, frames=1, mem=2, cost=vp(cost), dist2=None, p=P(), source=vp(src), n_sources=1, start=vp(start), sets=1, n=2, q=Q(),
             rows=vp(rows), cells=vp(cells), wps=vp(wps), reach=None, frm=None):
        return lib.pwpp_plan_grid(h, nx, ny, frames, mem, cost, dist2, p, source, n_sources, start, sets, n, q, rows, cells, wps, reach, frm)

    ok = b"PWPP_MEM_HOST or"  # (mem = 2, PWPP_MEM_HOST_PINNED: every check before mem has passed)
    for call in (route, plan):
        # 1 null pointers
        assert call(h=None) == E_ARG and b"null handle" in err()
        assert call(cost=None) == E_ARG and b"null cost image" in err()
        assert call(p=None) == E_ARG and b"null reach parameters" in err()
        assert call(source=None) == E_ARG and b"null source" in err()
        assert call(start=None) == E_ARG and b"null start" in err()
        assert call(q=None) == E_ARG and b"null route parameters" in err()
        assert call(rows=None) == E_ARG and b"null routes" in err()
        assert call() == E_ARG and ok in err()
        # 2 the images, 3 the reach parameters, 4 the range, 5 the sources: as pwpp_reach_grid
        assert call(frames=0) == E_ARG and b"0 frames of 4 x 4 cells" in err()
        assert call(nx=32769) == E_ARG and b"32768 a side" in err()
        assert call(p=P(base=0)) == E_ARG and b"base 0: 1 .. 255" in err()
        assert call(p=P(clearance2=-1)) == E_ARG and ok in err()  # read only with dist2
        assert call(p=P(clearance2=-1), dist2=vp(dist2)) == E_ARG and b"clearance2 -1" in err()
        assert call(p=P(pad_=3)) == E_ARG and b"pad_ 3" in err()
        assert call(nx=32768, ny=32768) == E_ARG and b"exceeds 2^31 - 2" in err()
        assert call(n_sources=2) == E_ARG and b"2 sources for 1 frames" in err()
        assert call(source=vp(np.array([[4, 0]], np.int32))) == E_ARG and b"source 0, cell (4, 0), lies outside the 4 x 4 cells" in err()
        # 6 the route parameters, each at both ends
        assert call(q=Q(max_cells=-1)) == E_ARG and b"max_cells -1" in err()
        assert call(q=Q(max_waypoints=-2)) == E_ARG and b"max_waypoints -2" in err()
        for v in (0, 257, -1):
            assert call(q=Q(look=v)) == E_ARG and b"look %d: 1 .. 256" % v in err()
        for v in (-1, 101):
            assert call(q=Q(line_cost=v)) == E_ARG and b"line_cost %d: 0 .. 100" % v in err()
        for kw in (dict(look=1, line_cost=0), dict(look=256, line_cost=100)):
            assert call(q=Q(**kw)) == E_ARG and ok in err(), kw
        # 7 the starts: sets, count, product, each
        for sets, frames in ((0, 1), (2, 1), (2, 3)):
            assert call(sets=sets, frames=frames, cost=vp(np.zeros(48, np.int8))) == E_ARG and b"%d start sets for %d frames" % (sets, frames) in err()
        for n in (0, -1, 65537):
            assert call(n=n) == E_ARG and b"%d starts: 1 .. 65536" % n in err()
        assert call(q=Q(max_cells=2 ** 30), n=2) == E_ARG and b"1 frames x 2 starts x 1073741824 list entries exceed 2^31 - 1" in err()   # 2^31, one past
        assert call(q=Q(max_cells=1, max_waypoints=2 ** 30), n=2) == E_ARG and b"exceed 2^31 - 1" in err()
        for bad in ((-1, 0), (4, 0), (0, -1), (0, 4)):
            s = np.array([[0, 0], bad], np.int32)
            assert call(start=vp(s)) == E_ARG and b"start 1 of set 0, cell (%d, %d), lies outside the 4 x 4 cells" % bad in err()
        s = np.array([[[0, 0], [1, 1]], [[2, 2], [9, 1]]], np.int32)
        big8, big32 = np.zeros(32, np.int8), np.zeros(32, np.int32)
        assert call(start=vp(s), sets=2, frames=2, cost=vp(big8), **({"frm": vp(big32)} if call is route else {})) == E_ARG and b"start 1 of set 1, cell (9, 1)" in err()
        # 8 the lists a limit asks for
        assert call(cells=None) == E_ARG and b"null cell lists with max_cells 4" in err()
        assert call(wps=None) == E_ARG and b"null waypoint lists with max_waypoints 4" in err()
        assert call(q=Q(max_cells=0, max_waypoints=0), cells=None, wps=None) == E_ARG and ok in err()
        # 9 the overlaps
        assert call(cells=vp(wps)) == E_ARG and b"cells and waypoints overlap" in err()
        assert call(cost=at(cells, 3)) == E_ARG and b"cost and cells overlap" in err()
        assert call(dist2=vp(wps)) == E_ARG and b"dist2 and waypoints overlap" in err()
        assert call(rows=vp(cells)) == E_ARG and b"routes and cells overlap" in err()
        assert call(q=Q(max_cells=0), cells=vp(wps)) == E_ARG and ok in err()  # a list without entries is not looked at
        # 10 mem, 11 the alignment in device memory
        assert call(mem=7) == E_ARG and b"mem 7" in err() and b"the routes take" in err()
        both = np.zeros(64, np.int32)
        assert call(mem=D, rows=at(both, 2)) == E_ARG and b"routes must be 4-byte aligned" in err()
        assert call(mem=D, cells=at(both, 1)) == E_ARG and b"cell lists must be 4-byte aligned" in err()
        assert call(mem=D, wps=at(both, 3)) == E_ARG and b"waypoint lists must be 4-byte aligned" in err()
        assert call(mem=D, dist2=at(both, 130)) == E_ARG and b"dist2 image must be 4-byte aligned" in err()
        # the order
        assert call(cost=None, frames=0) == E_ARG and b"null cost" in err()
        assert call(frames=0, p=P(base=0)) == E_ARG and b"0 frames" in err()
        assert call(p=P(base=0), n_sources=0) == E_ARG and b"base 0" in err()
        assert call(n_sources=0, q=Q(look=0)) == E_ARG and b"0 sources" in err()
        assert call(source=vp(np.array([[9, 9]], np.int32)), q=Q(look=0)) == E_ARG and b"source 0" in err()
        assert call(q=Q(max_cells=-1, max_waypoints=-1)) == E_ARG and b"max_cells -1" in err()
        assert call(q=Q(max_waypoints=-1, look=0)) == E_ARG and b"max_waypoints -1" in err()
        assert call(q=Q(look=0, line_cost=-1)) == E_ARG and b"look 0" in err()
        assert call(q=Q(line_cost=-1), sets=0) == E_ARG and b"line_cost -1" in err()
        assert call(sets=0, n=0) == E_ARG and b"0 start sets" in err()
        assert call(n=0, cells=None) == E_ARG and b"0 starts" in err()
        assert call(start=vp(np.array([[0, 0], [5, 5]], np.int32)), cells=None) == E_ARG and b"start 1 of set 0" in err()
        assert call(cells=None, rows=vp(cells)) == E_ARG and b"null cell lists" in err()
        assert call(cells=vp(wps), mem=7) == E_ARG and b"overlap" in err()
        assert call(mem=7, rows=at(both, 2)) == E_ARG and b"mem 7" in err()
    # what only one of the two has: the from image of pwpp_route_grid is an input, the field of pwpp_plan_grid an optional output
    assert route(frm=None) == E_ARG and b"null from image" in err()
    assert route(source=None, frm=None) == E_ARG and b"null source" in err()
    assert route(frm=None, start=None) == E_ARG and b"null from image" in err()
    assert route(frm=vp(cells)) == E_ARG and b"from and cells overlap" in err()
    assert route(mem=D, frm=at(both, 2)) == E_ARG and b"from image must be 4-byte aligned" in err()
    assert plan(reach=vp(reach), frm=vp(reach)) == E_ARG and b"reach and from overlap" in err()
    assert plan(reach=vp(cells)) == E_ARG and b"reach and cells overlap" in err()
    assert plan(reach=vp(reach), frm=vp(frm)) == E_ARG and ok in err()
    assert plan(mem=D, reach=at(both, 2)) == E_ARG and b"reach image must be 4-byte aligned" in err()
    assert plan(mem=D, frm=at(both, 1)) == E_ARG and b"from image must be 4-byte aligned" in err()


CPP = r"""
#include "patchwork/patchworkpp.h"
#ifndef PWPP_HAS_ROUTES
#error "include/pwpp.h does not announce the routes"
#endif
static_assert(sizeof(pwpp_route_params) == 16 && sizeof(pwpp_route) == 32, "the route structs");
static_assert(PWPP_ROUTE_OK == 0 && PWPP_ROUTE_NONE == 1 && PWPP_ROUTE_BROKEN == 2, "the status values");
long use(patchwork::PatchWorkpp &pw) {
    patchwork::PatchWorkpp::RouteParams q;
    patchwork::PatchWorkpp::ReachParams r;
    patchwork::PatchWorkpp::TerrainParams t;
    if (q.max_cells != 1024 || q.max_waypoints != 64 || q.look != 64 || q.line_cost != 0) return -1;
    q.look = 16, q.line_cost = 20;
    const std::vector<double> starts = {1.0, 2.0, -3.0, 4.0};
    const patchwork::PatchWorkpp::Routes a = pw.getRoutes(-40.0, -40.0, 0.5, 160, 160, starts), b = pw.getRoutes(-40.0, -40.0, 0.5, 160, 160, starts, t, r, q, 1.5, -2.0, true);
    const std::vector<int8_t> cost(160 * 160, 0);
    const patchwork::PatchWorkpp::Routes c = pw.planRoutes(cost, -40.0, -40.0, 0.5, 160, 160, starts), d = pw.planRoutes(cost, -40.0, -40.0, 0.5, 160, 160, starts, r, q, 3.0, 4.0);
    return (long)a.rows[0].cost + b.rows[1].cells + c.cells[3] + d.waypoints[1] + (long)d.waypoints_xy[2] + a.n + b.max_cells + c.max_waypoints;
}
"""


@pytest.mark.parametrize("flavour", ["plain", "eigen_shim"])
def test_cpp_mirror_methods_compile(tmp_path, flavour):
    src = tmp_path / "routes.cpp"
    src.write_text(CPP)
    cmd = ["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(PKG, "include"), "-I", os.path.join(ROOT, "include")]
    cmd += ["-DPWPP_NO_EIGEN"] if flavour == "plain" else ["-I", os.path.join(ROOT, "oracle", "eigen_shim")]
    subprocess.run(cmd + [str(src)], check=True)


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "routes.c"
    src.write_text('#include "pwpp.h"\nint f(const pwpp_reach_params *p, const pwpp_route_params *q, pwpp_route *r) {\n'
                   '    return pwpp_route_grid(0, 1, 1, 1, PWPP_MEM_HOST, 0, 0, p, 0, 1, 0, 0, 1, 1, q, r, 0, 0) +\n'
                   '           pwpp_plan_grid(0, 1, 1, 1, PWPP_MEM_HOST, 0, 0, p, 0, 1, 0, 1, 1, q, r, 0, 0, 0, 0) + (int)sizeof(*q) + (r->status == PWPP_ROUTE_BROKEN); }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)


# ---- the restatement and the one text: each property below is asked of csrc/pwpp_route.h, run by tools/route_check.cpp ---------------
def dumped(checker, tmp_path, cost, src, p, frm, starts, q, deal, dist2=None):
    """(rows, cells, waypoints) of route_check's dump mode -- the kernels' functions dealt as kernel `deal` deals them -- shaped as rt.routes."""
    c3 = np.ascontiguousarray(cost, np.int8).reshape((-1,) + np.shape(cost)[-2:])
    frames, ny, nx = c3.shape
    src = np.ascontiguousarray(np.asarray(src, np.int32).reshape(-1, 2))
    st = np.ascontiguousarray(starts, np.int32)
    sets, n = (st.shape[0], st.shape[1]) if st.ndim == 3 else (1, st.reshape(-1, 2).shape[0])
    d = tmp_path / ("dump%d" % len(list(tmp_path.iterdir())))
    d.mkdir()
    for name, a in (("cost", c3), ("src", src), ("from", np.ascontiguousarray(frm, np.int32)), ("starts", st)) + ((("dist2", np.ascontiguousarray(dist2, np.int32)),) if dist2 is not None else ()):
        a.tofile(d / name)
    args = ["dump", str(d / "cost"), str(nx), str(ny), str(frames)] + [str(p[k]) for k in ("base", "lethal", "unknown", "clearance2")]
    args += [str(d / "dist2") if dist2 is not None else "-", str(d / "src"), str(len(src)), str(d / "from"), str(d / "starts"), str(sets), str(n)]
    args += [str(q[k]) for k in ("max_cells", "max_waypoints", "look", "line_cost")] + [str(deal), str(d / "out")]
    subprocess.run([str(checker)] + args, check=True)
    return (np.fromfile(str(d / "out.rows"), rt.ROW).reshape(frames, n), np.fromfile(str(d / "out.cells"), np.int32).reshape(frames, n, q["max_cells"]),
            np.fromfile(str(d / "out.waypoints"), np.int32).reshape(frames, n, q["max_waypoints"]))


def both_deals(checker, tmp_path, cost, src, p, frm, starts, q, dist2=None):
    """The routes by both deals of the one text, equal to each other and to the restatement byte for byte."""
    want = rt.routes(cost, src, p, frm, starts, q, dist2)
    for deal in (1, 2):
        got = dumped(checker, tmp_path, cost, src, p, frm, starts, q, deal, dist2)
        for g, w in zip(got, want):
            assert g.tobytes() == w.tobytes(), "deal %d" % deal
    return got


def test_look_1_returns_the_route_itself(checker, tmp_path):
    c = rr.random_cost(1, 13, 12, 8, lethal=0.2)[0]
    p = rr.params(base=4, unknown=20)
    _, frm = rr.reach(c, (5, 6), p)
    starts = [(x, y) for y in range(0, 13, 3) for x in range(0, 12, 3)]
    rows, cells, wps = both_deals(checker, tmp_path, c, (5, 6), p, frm, starts, rt.route_params(max_cells=160, max_waypoints=160, look=1, line_cost=100))
    assert (rows["status"] == rt.OK).sum() > 8
    assert np.array_equal(cells, wps) and np.array_equal(rows["waypoints"], np.where(rows["status"] == rt.OK, rows["cells"], 0))


def test_an_open_uniform_field_has_two_waypoints_per_route_and_one_at_the_source(checker, tmp_path):
    for byte, line_cost in ((0, 0), (30, 30)):
        c = np.full((9, 14), byte, np.int8)
        p = rr.params(base=3)
        reach, frm = rr.reach(c, (4, 5), p)
        starts = [(x, y) for y in range(9) for x in range(14)]
        rows, cells, wps = both_deals(checker, tmp_path, c, (4, 5), p, frm, starts, rt.route_params(max_cells=16, max_waypoints=3, look=15, line_cost=line_cost))
        assert rows["cells"].max() <= 16 and (rows["status"] == rt.OK).all()
        at_source = np.array([s == (4, 5) for s in starts])
        assert np.array_equal(rows[0]["waypoints"], np.where(at_source, 1, 2))
        assert (wps[0, ~at_source, 1] == 5 * 14 + 4).all() and (wps[0, :, 2] == -1).all() and (wps[0, at_source, 1] == -1).all()
        assert np.array_equal(rows[0]["cost"], reach.reshape(-1))
    rows, _, _ = both_deals(checker, tmp_path, c, (4, 5), p, frm, starts, rt.route_params(max_waypoints=3, look=15, line_cost=29))  # dearer than the lines may cross
    assert np.array_equal(rows[0]["waypoints"], rows[0]["cells"])


MOVES = (lambda m: m, np.rot90, lambda m: np.rot90(m, 2), lambda m: np.rot90(m, 3), np.fliplr, np.flipud, np.transpose, lambda m: np.rot90(np.transpose(m), 2))


def test_the_eight_symmetries_of_the_square_map_routes_onto_routes(checker, tmp_path):
    """Up to the tie-break of from (the first neighbour in index order is another one in a turned image): the moved route is a route
    of the moved image with the same row and the moved waypoints, judged by certify on the moved field."""
    c = rr.random_cost(1, 12, 15, 31, lethal=0.15)[0]
    p = rr.params(base=6, unknown=25)
    q = rt.route_params(max_cells=180, max_waypoints=180, look=7, line_cost=60)
    src, starts = (7, 5), [(0, 0), (14, 11), (2, 9), (13, 1), (7, 5)]
    _, frm = rr.reach(c, src, p)
    rows, cells, wps = (a[0] for a in both_deals(checker, tmp_path, c, src, p, frm, starts, q))
    assert (rows["status"] == rt.OK).sum() >= 4 and (rows["waypoints"] < rows["cells"]).any()
    index = np.arange(c.size).reshape(c.shape)
    for move in MOVES:
        mc, mi = np.ascontiguousarray(move(c)), move(index)
        to = np.empty(c.size, np.int64)  # the moved index of every cell
        to[mi.reshape(-1)] = np.arange(c.size)
        cell = lambda i: (int(to[i]) % mc.shape[1], int(to[i]) // mc.shape[1])
        msrc = cell(src[1] * c.shape[1] + src[0])
        mreach, _ = rr.reach(mc, msrc, p)
        for k, s in enumerate(starts):
            cl, wp = rt.lists_of(rows[k], cells[k], wps[k])
            verdict = rt.certify(mc, msrc, p, mreach, cell(s[1] * c.shape[1] + s[0]), q, rows[k], [to[i] for i in cl], [to[i] for i in wp], tie_break=False)
            assert verdict is None, (move, s, verdict)


def certified_case(checker, tmp_path):
    c = np.zeros((9, 12), np.int8)
    c[2:9, 5] = 100  # a wall with a gap at the top
    c[0, 8] = 40     # and a dear cell beyond it
    p, q = rr.params(base=2), rt.route_params(max_cells=64, max_waypoints=64, look=6, line_cost=10)
    src, start = (10, 7), (1, 7)
    reach, frm = rr.reach(c, src, p)
    rows, cells, wps = (a[0] for a in both_deals(checker, tmp_path, c, src, p, frm, [start], q))
    cl, wp = rt.lists_of(rows[0], cells[0], wps[0])
    return c, src, p, reach, start, q, rows[0], cl, wp


def test_certify_accepts_the_one_text_and_refuses_a_tied_but_wrong_predecessor(checker, tmp_path):
    c, src, p, reach, start, q, row, cl, wp = certified_case(checker, tmp_path)
    assert rt.certify(c, src, p, reach, start, q, row, cl, wp) is None
    assert 2 < len(wp) < len(cl)
    # on free ground (2, 1) comes from (1, 0) across a corner or from (1, 1) across an edge at the same 24: from names the first, (1, 0)
    c = np.zeros((4, 5), np.int8)
    p, q0 = rr.params(base=1), rt.route_params(max_cells=8)
    reach, frm = rr.reach(c, (0, 0), p)
    rows, cells, _ = (a[0] for a in both_deals(checker, tmp_path, c, (0, 0), p, frm, [(2, 1)], q0))
    assert reach[1, 2] == 24 == reach[0, 1] + 14 == reach[1, 1] + 10 and cells[0, :3].tolist() == [7, 1, 0] and rows[0]["cost"] == 24
    assert rt.certify(c, (0, 0), p, reach, (2, 1), q0, rows[0], [7, 1, 0], []) is None
    tied = row_with(rows[0], edge_steps=1, corner_steps=1)
    assert (rows[0]["edge_steps"], rows[0]["corner_steps"]) == (1, 1)
    assert "the first neighbour that attains the value is 1" in rt.certify(c, (0, 0), p, reach, (2, 1), q0, tied, [7, 6, 0], [])
    assert rt.certify(c, (0, 0), p, reach, (2, 1), q0, tied, [7, 6, 0], [], tie_break=False) is None
    assert "no step onto a reach" in rt.certify(c, (0, 0), p, reach, (2, 1), q0, tied, [7, 2, 1, 0], [], tie_break=False)   # a detour is no tie


def row_with(row, **kw):
    r = np.zeros(1, rt.ROW)[0]
    for n in rt.ROW.names:
        r[n] = kw.get(n, row[n])
    return r


def test_certify_refuses_a_waypoint_one_too_near_and_one_too_far(checker, tmp_path):
    c, src, p, reach, start, q, row, cl, wp = certified_case(checker, tmp_path)
    at = {cell: i for i, cell in enumerate(cl)}
    w = [at[x] for x in wp]
    seen = set()
    for k in range(1, len(w) - 1):
        for delta, word in ((-1, "near"), (1, "far")):
            j = w[k] + delta
            if not w[k - 1] < j < w[k + 1]:
                continue
            moved = wp[:k] + [cl[j]] + wp[k + 1:]
            verdict = rt.certify(c, src, p, reach, start, q, row, cl, moved)
            assert verdict is not None, (k, word)
            assert ("although the line" in verdict) if delta < 0 else ("no legal path" in verdict or "with look" in verdict or "although the line" in verdict), verdict
            seen.add(word)
    assert seen == {"near", "far"}
    assert "do not run from the start" in rt.certify(c, src, p, reach, start, q, row, cl, wp[:-1])
    assert "cost is" in rt.certify(c, src, p, reach, start, q, row_with(row, cost=row["cost"] + 1), cl, wp)


# ---- the one text on the host ----------------------------------------------------------------------------------------------------
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"]


def sanitizers_work(tmp_path):
    """The toolchain links the two runtimes into a program and that program starts in this environment."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++"] + SANITIZE + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        return False
    return subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode == 0


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("route_check")
    exe = tmp / "route_check"
    flags = SANITIZE if sanitizers_work(tmp) else []
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off"] + flags +
                   ["-I", os.path.join(PKG, "csrc"), os.path.join(ROOT, "tools", "route_check.cpp"), "-o", str(exe)], check=True)
    return exe


def test_route_program_builds_and_passes(checker):
    r = subprocess.run([str(checker)], capture_output=True, text=True)  # (a stand-alone child process with its own main)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 mismatches" in r.stdout
    assert int(r.stdout.split("route_check: ")[1].split(" cases")[0]) >= 3000


@pytest.mark.parametrize("deal", [1, 2])
@pytest.mark.parametrize("case", ["plain", "dist2", "per_frame", "damaged"])
def test_the_restatement_and_the_one_text_agree_byte_for_byte(checker, tmp_path, case, deal):
    """The kernels' functions, dealt lane by lane and wave by wave on the host, against the restatement: what the GPU tests compare, without a GPU."""
    frames, ny, nx = 3, 23, 41
    c = rr.random_cost(frames, ny, nx, 17, lethal=0.18)
    p = rr.params(base=5, lethal=95, unknown=-1 if case == "plain" else 35, clearance2=3)
    d2 = np.random.default_rng(4).integers(0, 50, c.shape).astype(np.int32) if case == "dist2" else None
    src = np.array([[20, 11], [0, 0], [40, 22]] if case == "per_frame" else [[19, 12]], np.int32)
    rng = np.random.default_rng(9)
    sets = frames if case == "per_frame" else 1
    starts = np.stack([rng.integers(0, nx, (sets, 9)), rng.integers(0, ny, (sets, 9))], axis=-1).astype(np.int32)
    _, frm = rr.reach(c, src, p, d2)
    if case == "damaged":
        flat = frm.reshape(-1)
        hit = rng.integers(0, flat.size, 40)
        flat[hit] = rng.integers(-2, nx * ny + 2, 40)
    q = rt.route_params(max_cells=12, max_waypoints=3, look=9, line_cost=50)
    for name, a in (("cost", c), ("src", src), ("from", frm), ("starts", starts)) + ((("dist2", d2),) if d2 is not None else ()):
        a.tofile(tmp_path / name)
    args = ["dump", str(tmp_path / "cost"), str(nx), str(ny), str(frames)] + [str(p[k]) for k in ("base", "lethal", "unknown", "clearance2")]
    args += [str(tmp_path / "dist2") if d2 is not None else "-", str(tmp_path / "src"), str(len(src)), str(tmp_path / "from"), str(tmp_path / "starts"), str(sets), "9"]
    args += [str(q[k]) for k in ("max_cells", "max_waypoints", "look", "line_cost")] + [str(deal), str(tmp_path / "out")]
    subprocess.run([str(checker)] + args, check=True)
    want = rt.routes(c, src, p, frm, starts if sets > 1 else starts[0], q, d2)
    got = (np.fromfile(str(tmp_path / "out.rows"), rt.ROW), np.fromfile(str(tmp_path / "out.cells"), np.int32), np.fromfile(str(tmp_path / "out.waypoints"), np.int32))
    for g, w in zip(got, want):
        assert g.tobytes() == w.tobytes()
    assert (want[0]["status"] == rt.OK).sum() > 8 and (want[0]["cells"] > 12).any() and (want[0]["waypoints"] > 3).any() and (want[0]["cells"] < 12).any()
    if case == "damaged":
        assert (want[0]["status"] == rt.BROKEN).any()
