"""The per-beam free space without a device: the symbols and the header, pwpp_beam_height (the function the kernels call, on the host)
against the restatement of tests/beams_ref.py, the worked row of include/pwpp.h, the order of pwpp_beam_grid's argument checks, the
library's byte rule on every combination (printed by tools/beams_check.cpp from csrc/pwpp_beams.h), the two ways into the restatement
against each other (a check of the reference), and tools/beams_check.cpp itself -- the walks of both paths dealt as the kernels deal
them against a brute force of its own, under the address and undefined-behaviour sanitizers."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

import beams_ref as br
import pwpp_hip
from test_obstacle_visibility_cpu import SANITIZE, sanitizers_work

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "patchwork-plusplus_amd")
E_ARG = -1


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(pwpp_hip.LIB_PATH):
        subprocess.run(["make", "-C", PKG, "lib/libpwpp_hip.so"], check=True, stdout=subprocess.DEVNULL)
    return pwpp_hip.load()


def test_symbols_macro_constants_and_prototypes(lib):
    hdr = open(os.path.join(ROOT, "include", "pwpp.h")).read()
    for name in ("pwpp_rasterize_beams", "pwpp_beam_grid", "pwpp_beam_ground"):
        assert hasattr(lib, name), name
        assert "PWPP_API int %s(" % name in hdr
    assert hasattr(lib, "pwpp_beam_height") and "PWPP_API int32_t pwpp_beam_height(int32_t eye, int32_t z, int k, int n);" in hdr
    assert "#define PWPP_HAS_BEAMS 1" in hdr and "#define PWPP_BEAMS_GROUND 1" in hdr and "#define PWPP_BEAMS_NONGROUND 2" in hdr
    assert '"beams_path"' in hdr and "reflected-noise removal rejected" in hdr and "min_pass >= 2 is the remedy" in hdr
    assert (pwpp_hip.BEAMS_GROUND, pwpp_hip.BEAMS_NONGROUND) == (br.GROUND, br.NONGROUND) == (1, 2)
    assert len(lib.pwpp_rasterize_beams.argtypes) == 8 and len(lib.pwpp_beam_grid.argtypes) == 17 and len(lib.pwpp_beam_ground.argtypes) == 17
    assert lib.pwpp_beam_ground.argtypes[7] is ctypes.c_double
    for name in ("rasterize_beams", "rasterize_beams_device", "beam_grid", "beam_grid_device", "beam_ground", "beam_ground_device"):
        assert callable(getattr(pwpp_hip.Handle, name)), name
    import pypatchworkpp
    assert hasattr(pypatchworkpp.patchworkpp, "getBeamClearance")
    assert os.path.exists(os.path.join(PKG, "csrc", "pwpp_beams.h")) and "csrc/pwpp_beams.hip" in open(os.path.join(PKG, "Makefile")).read()
    assert "#define PWPP_BEAMS_TILE 64" in open(os.path.join(PKG, "csrc", "pwpp_beams.h")).read()  # (the sides of the GPU test's tiled shapes follow it)


RISES = (-3 * br.R, -br.R - 1, -br.R, -br.R + 1, -3000, -41, -1, 0, 1, 41, 3000, br.R - 1, br.R, br.R + 1, 3 * br.R)


def test_beam_height_against_the_restatement(lib):
    for eye in (1700, -350, 2 ** 30, -2 ** 30):
        for n in range(2, 41):
            for k in range(1, n):
                got = [pwpp_hip.beam_height(eye, min(max(eye + r, br.NO_HEIGHT + 1), br.INT32_MAX), k, n) for r in RISES]
                assert got == [br.height(eye, min(max(eye + r, br.NO_HEIGHT + 1), br.INT32_MAX), k, n) for r in RISES], (eye, k, n)
                assert got == sorted(got), "the height is not monotone in z at k %d of n %d" % (k, n)
                assert all(eye - br.R <= v <= eye + br.R for v in got)
    # the closed form in other words: exact rational ceiling
    from fractions import Fraction
    import math
    for r, k, n in ((-1700, 10, 34), (680, 17, 34), (7, 3, 5), (-7, 3, 5), (br.R, 39, 40), (-br.R, 1, 40)):
        D = 2 * k - 1 if r < 0 else 2 * k + 1
        assert pwpp_hip.beam_height(100, 100 + r, k, n) == 100 + math.ceil(Fraction(r * D, 2 * n))
    for bad in ((0, 0, 0, 5), (0, 0, 5, 5), (0, 0, 1, 1), (2 ** 30 + 1, 0, 1, 5), (0, br.NO_HEIGHT, 1, 5), (0, 0, 1, 32769)):
        with pytest.raises(pwpp_hip.PwppError, match="beam height"):
            pwpp_hip.beam_height(*bad)


def test_the_worked_row(lib):
    hits, zmin = np.zeros((1, 40), np.int32), np.full((1, 40), br.NO_HEIGHT, np.int32)
    hits[0, 34], zmin[0, 34] = 3, 0
    passes, low = br.beams_of(hits, zmin, (0, 0, 1700))
    assert (passes[0, 1:34] == 3).all() and passes[0, 0] == 0 and (passes[0, 34:] == 0).all()
    assert low[0, [1, 10, 17, 33]].tolist() == [1675, 1225, 875, 75] == [pwpp_hip.beam_height(1700, 0, k, 34) for k in (1, 10, 17, 33)]
    assert low[0, 0] == low[0, 34] == br.NO_HEIGHT
    zmin[0, 34] = 2380
    low = br.beams_of(hits, zmin, (0, 0, 1700))[1]
    assert low[0, [1, 17, 33]].tolist() == [1730, 2050, 2370] == [pwpp_hip.beam_height(1700, 2380, k, 34) for k in (1, 17, 33)]


def test_every_argument_is_named_before_the_device_is_touched_and_in_order(lib):
    hits, zmin, passes, low = (np.zeros(16, np.int32) for _ in range(4))
    occ = np.zeros(16, np.int8)
    one = np.array([1, 2, 1700], np.int32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    fake = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(8)))  # (never dereferenced: these checks come first)
    H = pwpp_hip.MEM_HOST
    err = lib.pwpp_last_error

    def grid(h=fake, nx=4, ny=4, frames=1, mem=H, hits=vp(hits), zmin=vp(zmin), target=None, base=None, origin=vp(one), n_origins=1, max_range=0, min_pass=1,
             clearance=0, passes=vp(passes), low=vp(low), occ=vp(occ)):
        return lib.pwpp_beam_grid(h, nx, ny, frames, mem, hits, zmin, target, base, origin, n_origins, max_range, min_pass, clearance, passes, low, occ)

    # 1 null pointers
    assert grid(h=None) == E_ARG and b"null handle" in err()
    for name in ("hits", "zmin", "origin", "passes", "low"):
        assert grid(**{name: None}) == E_ARG and b"null " + name.encode() in err(), name
    # 2 .. 4 the shape
    for kw in (dict(nx=0), dict(ny=0), dict(frames=0), dict(nx=-3)):
        assert grid(**kw) == E_ARG and b"cells" in err(), kw
    for kw in (dict(nx=32769), dict(ny=40000)):
        assert grid(**kw) == E_ARG and b"32768 a side" in err(), kw
    assert grid(nx=32768, ny=32768, frames=3, n_origins=3) == E_ARG and b"exceed 2^31" in err()
    # 5 .. 7 the parameters
    for m in (-1, 32769):
        assert grid(max_range=m) == E_ARG and b"max_range" in err(), m
    for m in (0, -5):
        assert grid(min_pass=m) == E_ARG and b"min_pass" in err(), m
    assert grid(clearance=-1) == E_ARG and b"clearance" in err()
    # 8 .. 10 the origins
    for n in (0, 2, -1):
        assert grid(n_origins=n) == E_ARG and b"origins for 1 frames" in err(), n
    assert grid(frames=3, n_origins=2) == E_ARG and b"2 origins for 3 frames" in err()
    for bad in ((4, 0), (0, 4), (-1, 0), (0, -1)):
        assert grid(origin=vp(np.array(bad + (0,), np.int32))) == E_ARG and b"origin 0" in err() and b"outside" in err(), bad
    three = np.array([0, 0, 0, 3, 3, 2 ** 30, 3, 3, -2 ** 30 - 1], np.int32)
    big = np.zeros(48, np.int32)
    assert grid(frames=3, n_origins=3, origin=vp(three), hits=vp(big), zmin=vp(big.copy())) == E_ARG and b"origin 2" in err() and b"eye" in err()
    # 11 .. 12 overlaps, mem
    assert grid(passes=vp(hits)) == E_ARG and b"hits and passes overlap" in err()
    assert grid(low=vp(passes)) == E_ARG and b"passes and low overlap" in err()
    assert grid(base=vp(occ), occ=vp(occ[1:])) == E_ARG and b"without being equal" in err()
    assert grid(mem=2) == E_ARG and b"PWPP_MEM_HOST or PWPP_MEM_DEVICE" in err()   # PWPP_MEM_HOST_PINNED
    # the order: each check with every later one failing too
    assert grid(hits=None, nx=0) == E_ARG and b"null hits" in err()
    assert grid(nx=32769, ny=32769, frames=4, max_range=-1) == E_ARG and b"32768 a side" in err()
    assert grid(nx=32768, ny=32768, frames=3, max_range=-1) == E_ARG and b"exceed 2^31" in err()
    assert grid(max_range=-1, min_pass=0) == E_ARG and b"max_range" in err()
    assert grid(min_pass=0, clearance=-1) == E_ARG and b"min_pass" in err()
    assert grid(clearance=-1, n_origins=2) == E_ARG and b"clearance" in err()
    assert grid(n_origins=2, origin=vp(np.array([9, 9, 0], np.int32))) == E_ARG and b"origins for" in err()
    assert grid(origin=vp(np.array([9, 9, 2 ** 30 + 1], np.int32))) == E_ARG and b"outside the 4 x 4" in err()
    assert grid(origin=vp(np.array([0, 0, 2 ** 30 + 1], np.int32)), passes=vp(hits)) == E_ARG and b"eye" in err()
    assert grid(passes=vp(hits), mem=2) == E_ARG and b"overlap" in err()
    assert grid(mem=2, passes=ctypes.c_void_p(vp(passes).value + 2)) == E_ARG and b"PWPP_MEM_HOST or" in err()

    g = pwpp_hip.GroundGrid(-2.0, -2.0, 1.0, 4, 4, 0, 0)
    zero = np.zeros(3, np.float64)

    def ground(h=fake, gr=ctypes.byref(g), which=1, origin=vp(zero), n_origins=1, max_range=0, min_pass=1, clearance=0.3, frames=1, passes=vp(passes), low=vp(low)):
        return lib.pwpp_beam_ground(h, gr, which, origin, n_origins, max_range, min_pass, clearance, 0, frames, H, None, passes, low, None, None, None)

    assert ground(h=None) == E_ARG and b"null handle" in err()
    for kw, word in ((dict(gr=None), b"grid"), (dict(origin=None), b"origin"), (dict(passes=None), b"passes"), (dict(low=None), b"low")):
        assert ground(**kw) == E_ARG and b"null " + word in err(), kw
    bad = pwpp_hip.GroundGrid(0.0, 0.0, 1.0, 4, 4, 2, 0)
    assert ground(gr=ctypes.byref(bad)) == E_ARG and b"grid flags" in err()
    for which in (0, 4, -1):
        assert ground(which=which) == E_ARG and b"which" in err()
    for c in (-0.1, np.nan, np.inf):
        assert ground(clearance=c) == E_ARG and b"clearance" in err(), c
    assert ground(max_range=32769) == E_ARG and b"max_range" in err()
    assert ground(min_pass=0) == E_ARG and b"min_pass" in err()
    assert ground(n_origins=2) == E_ARG and b"2 origins for 1 frames" in err()
    assert ground(origin=vp(np.array((2.0, 0.0, 0.0)))) == E_ARG and b"outside the grid" in err()
    assert ground(origin=vp(np.array((0.0, 0.0, np.nan)))) == E_ARG and b"not finite" in err()
    assert ground(low=vp(passes)) == E_ARG and b"overlap" in err()

    def ends(h=fake, gr=ctypes.byref(g), which=1, a=vp(hits), b=vp(zmin)):
        return lib.pwpp_rasterize_beams(h, gr, which, 0, 1, H, a, b)

    assert ends(h=None) == E_ARG and b"null handle" in err()
    assert ends(gr=None) == E_ARG and b"null grid" in err()
    assert ends(a=None) == E_ARG and b"null hits" in err() and ends(b=None) == E_ARG and b"null zmin" in err()
    for flags in (1, 2):  # PWPP_GRID_GROUND_ONLY too: the endpoints read no reference
        gg = pwpp_hip.GroundGrid(-2.0, -2.0, 1.0, 4, 4, flags, 0)
        assert ends(gr=ctypes.byref(gg)) == E_ARG and b"grid flags" in err()
    for which in (0, 4, 8, -2):
        assert ends(which=which) == E_ARG and b"which" in err()
    assert lib.pwpp_rasterize_beams(fake, ctypes.byref(g), 3, 0, 1, 2, vp(hits), vp(zmin)) == E_ARG and b"PWPP_MEM_HOST or PWPP_MEM_DEVICE" in err()


@pytest.fixture(scope="module")
def beams_check(tmp_path_factory):
    """tools/beams_check.cpp built once, with the sanitizers where the toolchain has them: a stand-alone program with its own main."""
    tmp = tmp_path_factory.mktemp("beams_check")
    exe = tmp / "beams_check"
    flags = SANITIZE if sanitizers_work(tmp) else []
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror"] + flags +
                   ["-I", os.path.join(PKG, "csrc"), os.path.join(ROOT, "tools", "beams_check.cpp"), "-o", str(exe)], check=True)
    return str(exe)


def test_the_byte_rule_on_every_combination(beams_check):
    """Base byte x passes against min_pass x target (no image, no height, at, below and above low - clearance), through the
    LIBRARY's rule: beams_check --bytes prints what pwpp_beams_low and pwpp_beams_occupancy of csrc/pwpp_beams.h give for every
    combination, as the kernels call them; every row is compared with the restatement and with the rule in plain words."""
    r = subprocess.run([beams_check, "--bytes"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [tuple(int(v) for v in line.split()) for line in r.stdout.splitlines()]
    kinds, none_under_a_wide_clearance = set(), 0
    for base, passes, raw, has_target, target, min_pass, clearance, low, byte in rows:
        want_low = br.NO_HEIGHT if passes == 0 else raw
        assert low == want_low, (base, passes, raw)
        want = br.occupancy_of(np.array([[passes]], np.uint32), np.array([[want_low]]), np.array([[target]]) if has_target else None,
                               np.array([[base]], np.int8), min_pass, clearance)[0, 0]
        edge = want_low - clearance  # low - target <= clearance  <=>  target >= edge
        kind = "null" if not has_target else ("none" if target == br.NO_HEIGHT else ("at" if target == edge else ("below" if target < edge else "above")))
        free = base == br.UNKNOWN and passes >= min_pass and kind in ("null", "at", "above")  # (above: a higher ground, a smaller gap)
        assert byte == want == (br.FREE if free else base), (base, passes, raw, has_target, target, clearance, byte)
        kinds.add((base, passes >= min_pass, kind))
        # the clause that asks for a height alone decides: low - INT32_MIN <= clearance would call the cell free
        if kind == "none" and base == br.UNKNOWN and passes >= min_pass and low - br.NO_HEIGHT <= clearance:
            none_under_a_wide_clearance += 1
            assert byte == br.UNKNOWN
    assert kinds == set(itertools.product((br.FREE, br.OCCUPIED, br.UNKNOWN, 42), (False, True), ("null", "none", "at", "below", "above")))
    assert none_under_a_wide_clearance >= 3 and {p for _, p, *_ in rows} == {0, 2, 3, 4, 2 ** 32 - 1} and {r[5] for r in rows} == {3}
    # no base bytes: all unknown (the restatement's own default; the GPU tests compare it with the library's)
    assert br.occupancy_of(np.array([[0, 3]], np.uint32), np.array([[br.NO_HEIGHT, 5]]), None, None, 3, 0).tolist() == [[br.UNKNOWN, br.FREE]]


def test_images_and_points_give_the_same_beams():
    """A test of the REFERENCE alone, not of the library: the theorem of the header on the restatement itself -- tracing every point
    from its own cell and z gives what the two images give -- so that the two oracles of tests/test_gpu_beams.py, where the chained
    call is compared with both, cannot drift apart unnoticed."""
    rng = np.random.default_rng(4)
    grid = (-8.0, -6.0, 0.5, 32, 24)
    xyz = np.stack([rng.uniform(-9, 9, 900), rng.uniform(-7, 7, 900), rng.normal(-1.0, 1.5, 900)], 1).astype(np.float32)
    xyz[::50, 2] = np.nan
    hits, zmin = br.ends_of_points(xyz, grid)
    assert hits.sum() < 900 - 18 and hits.max() >= 2
    for origin, max_range in (((16, 12, 0), 0), ((0, 0, -1500), 0), ((31, 12, 2000), 7)):
        a, b = br.beams_of(hits, zmin, origin, max_range), br.beams_of_points(xyz, grid, origin, max_range)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and (a[0] > 0).sum() > 50


def test_cpp_mirror_method_compiles_and_the_header_as_c99(tmp_path):
    src = tmp_path / "beams.cpp"
    src.write_text('#include "patchwork/patchworkpp.h"\n#ifndef PWPP_HAS_BEAMS\n#error "include/pwpp.h does not announce the beams"\n#endif\n'
                   'double use(patchwork::PatchWorkpp &pw) {\n'
                   '    patchwork::PatchWorkpp::BeamClearance v = pw.getBeamClearance(-40.0, -40.0, 0.5, 160, 160);\n'
                   '    patchwork::PatchWorkpp::BeamClearance w = pw.getBeamClearance(-40.0, -40.0, 0.5, 160, 160, 2, 0.3, 40, 1.5, -0.5, 0.1, PWPP_BEAMS_GROUND | PWPP_BEAMS_NONGROUND, true, v.occupancy);\n'
                   '    return v.passes[5] + v.low[9] + v.occupancy[7] + (double)w.passes.size() + w.nx + w.ny;\n}\n')
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-DPWPP_NO_EIGEN", "-I", os.path.join(PKG, "include"), "-I", os.path.join(ROOT, "include"),
                    str(src)], check=True)
    c = tmp_path / "beams.c"
    c.write_text('#include "pwpp.h"\nint f(void) { return pwpp_rasterize_beams(0, 0, PWPP_BEAMS_GROUND, 0, 1, PWPP_MEM_HOST, 0, 0) + '
                 'pwpp_beam_grid(0, 1, 1, 1, PWPP_MEM_HOST, 0, 0, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0) + '
                 'pwpp_beam_ground(0, 0, 1, 0, 1, 0, 1, 0.3, 0, 1, PWPP_MEM_HOST, 0, 0, 0, 0, 0, 0) + (int)pwpp_beam_height(0, 0, 1, 2) + PWPP_HAS_BEAMS; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(c)], check=True)


# ---- the kernels' functions and sequence on the host -----------------------------------------------------------------------------
def test_beams_program_builds_and_passes(beams_check):
    r = subprocess.run([beams_check], capture_output=True, text=True)  # (a stand-alone child process with its own main)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 mismatches" in r.stdout and "119209 cases" in r.stdout and " 0 theorem failures" in r.stdout
