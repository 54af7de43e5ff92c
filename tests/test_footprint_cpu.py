"""No-GPU checks of the oriented vehicle footprint (pwpp_footprint_grid): the exports, the feature macro and its place, the macros and
struct sizes, the ctypes prototypes and the bindings' methods, every argument check that needs no device with its message and its
place in the order (a pose entry named by set, trajectory and step), the header from C99 and the C++ mirror in both flavours; the
properties of the contract, asked of csrc/pwpp_footprint.h through footprint_check's dump mode by both deals and of the restatement
(tests/footprint_ref.py, brute force and windowed visit) alike: scaling u changes no byte, reversing u swaps front and rear, the eight
symmetries of the square map footprints onto footprints, cells exactly on an edge are covered and one tick less drops exactly them,
Lemma 1 and Lemma 2 (the touching in exact integers), the footprint of all zeros, negative ticks; pwpp_footprint_covers and
pwpp_footprint_pose against the restatement; and the stand-alone program that runs the kernels' functions on the host, dealt as both
kernels deal them, against a brute force of its own (tools/footprint_check.cpp), built with the address and undefined-behaviour
sanitizers where the toolchain has them."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import footprint_ref as fr
import pwpp_hip
import reach_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "patchwork-plusplus_amd")
E_ARG = -1


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(pwpp_hip.LIB_PATH):
        subprocess.run(["make", "-C", PKG, "lib/libpwpp_hip.so"], check=True, stdout=subprocess.DEVNULL)
    return pwpp_hip.load()


def test_symbols_macros_structs_and_prototypes(lib):
    hdr = open(os.path.join(ROOT, "include", "pwpp.h")).read()
    for name in ("pwpp_footprint_grid", "pwpp_footprint_covers", "pwpp_footprint_pose"):
        assert hasattr(lib, name), name
        assert "PWPP_API int %s(" % name in hdr
    assert "#define PWPP_HAS_FOOTPRINT 1" in hdr and '"footprint_path"' in hdr
    for name, value in (("SUB", 16), ("MAX_EXTENT", 1024), ("MAX_STEPS", 4096), ("FREE", 0), ("HIT", 1), ("SKIPPED", 2), ("OUTSIDE_BLOCKS", 1)):
        assert any(line.split()[:3] == ["#define", "PWPP_FOOT_" + name, str(value)] for line in hdr.splitlines()), name
    assert (pwpp_hip.FOOT_FREE, pwpp_hip.FOOT_HIT, pwpp_hip.FOOT_SKIPPED) == (0, 1, 2) == (fr.FREE, fr.HIT, fr.SKIPPED)
    assert pwpp_hip.FOOT_OUTSIDE_BLOCKS == 1 == fr.OUTSIDE_BLOCKS and pwpp_hip.FOOT_SUB == 16 == fr.SUB
    for struct in ("pwpp_footprint_params", "pwpp_footprint_pose_row", "pwpp_footprint_traj_row"):
        assert "typedef struct %s {" % struct in hdr
    # declared after the routes and before the input transforms
    assert hdr.index("PWPP_API int pwpp_plan_grid(") < hdr.index("PWPP_HAS_FOOTPRINT") < hdr.index("PWPP_API int pwpp_footprint_grid(")
    assert hdr.index("PWPP_API int pwpp_footprint_pose(") < hdr.index("#define PWPP_HAS_INPUT_TRANSFORM")
    assert ctypes.sizeof(pwpp_hip.FootprintParams) == 24 and pwpp_hip.FOOT_POSE_DTYPE.itemsize == 32 == fr.POSE_ROW.itemsize
    assert pwpp_hip.FOOT_TRAJ_DTYPE.itemsize == 32 == fr.TRAJ_ROW.itemsize
    assert [f[0] for f in pwpp_hip.FootprintParams._fields_] == ["front", "rear", "half_width", "flags", "pad_"]
    assert list(pwpp_hip.FOOT_POSE_DTYPE.names) == ["status", "covered", "outside", "blocked", "unknown", "max_term", "min_dist2", "hit"] == list(fr.POSE_ROW.names)
    assert list(pwpp_hip.FOOT_TRAJ_DTYPE.names) == ["first_hit", "free_steps", "last", "max_term", "sum_term", "unknown", "min_dist2", "reach_last"] == list(fr.TRAJ_ROW.names)
    assert len(lib.pwpp_footprint_grid.argtypes) == 16 and len(lib.pwpp_footprint_covers.argtypes) == 4 and len(lib.pwpp_footprint_pose.argtypes) == 5
    for name in ("footprint_grid", "footprint_grid_device"):
        assert callable(getattr(pwpp_hip.Handle, name)), name
    assert callable(pwpp_hip.footprint_covers) and callable(pwpp_hip.footprint_pose)
    import pypatchworkpp
    assert hasattr(pypatchworkpp.patchworkpp, "checkFootprints")
    f = pypatchworkpp.FootprintParams()
    assert (f.front, f.rear, f.half_width, f.pad, f.outside_blocks) == (3.4, 1.1, 0.9, 0, False)
    doc = pypatchworkpp.patchworkpp.checkFootprints.__doc__
    assert "cost:" in doc and "poses_xyyaw:" in doc and "footprint_params:" in doc and "reach_params:" in doc and "reach: object = None" in doc
    src = open(os.path.join(PKG, "csrc", "pwpp_footprint.h")).read()
    assert "#define PWPP_FOOT_TRAJ_MAX 65536\n" in src and "LEMMA 1" in src and "LEMMA 2" in src
    hip = open(os.path.join(PKG, "csrc", "pwpp_footprint.hip")).read()
    for kernel in ("k_foot_poses", "k_foot_trajs", "k_foot_waves"):
        assert kernel in hip and kernel in open(os.path.join(PKG, "csrc", "pwpp_dev.h")).read()
    assert "csrc/pwpp_footprint.hip" in open(os.path.join(PKG, "Makefile")).read()


def rparams(**kw):
    f = dict(base=1, lethal=100, unknown=-1, clearance2=0, max_reach=0, pad_=0)
    f.update(kw)
    return pwpp_hip.ReachParams(**f)


def fparams(pad_=(0, 0), **kw):
    f = dict(front=20, rear=4, half_width=8, flags=0)
    f.update(kw)
    return pwpp_hip.FootprintParams(f["front"], f["rear"], f["half_width"], f["flags"], pad_)


def test_every_argument_is_named_before_the_device_is_touched_and_in_order(lib):
    cost = np.zeros(16, np.int8)
    dist2, reach = np.zeros(16, np.int32), np.zeros(16, np.int32)
    poses = np.tile(np.array([8, 8, 1, 0], np.int32), (2, 3, 1))  # 2 trajectories x 3 steps
    prow, trow = np.zeros(6, fr.POSE_ROW), np.zeros(2, fr.TRAJ_ROW)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    at = lambda a, n: ctypes.c_void_p(a.ctypes.data + n)
    fake = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(8)))  # (never dereferenced: these checks come first)
    D = pwpp_hip.MEM_DEVICE
    err = lib.pwpp_last_error
    P = lambda **kw: ctypes.byref(rparams(**kw))
    F = lambda **kw: ctypes.byref(fparams(**kw))

    def call(h=fake, nx=4, ny=4, frames=1, mem=2, cost=vp(cost), dist2=None, reach=None, p=P(), fp=F(), poses=vp(poses), sets=1, n_traj=2, n_steps=3, prow=vp(prow),
             trow=vp(trow)):
        return lib.pwpp_footprint_grid(h, nx, ny, frames, mem, cost, dist2, reach, p, fp, poses, sets, n_traj, n_steps, prow, trow)

    ok = b"PWPP_MEM_HOST or"  # (mem = 2, PWPP_MEM_HOST_PINNED: every check before mem has passed)
    # 1 null pointers
    assert call(h=None) == E_ARG and b"null handle" in err()
    assert call(cost=None) == E_ARG and b"null cost image" in err()
    assert call(p=None) == E_ARG and b"null reach parameters" in err()
    assert call(fp=None) == E_ARG and b"null footprint parameters" in err()
    assert call(poses=None) == E_ARG and b"null poses" in err()
    assert call() == E_ARG and ok in err() and b"the footprints take" in err()
    # 2 the image's shape
    assert call(frames=0) == E_ARG and b"0 frames of 4 x 4 cells" in err()
    assert call(nx=32769) == E_ARG and b"32768 a side" in err()
    assert call(nx=32768, ny=32768, frames=3) == E_ARG and b"exceed 2^31" in err()
    # 3 the reach parameters as pwpp_reach_grid names them -- without the range
    assert call(p=P(base=0)) == E_ARG and b"base 0: 1 .. 255" in err()
    assert call(p=P(lethal=102)) == E_ARG and b"lethal 102" in err()
    assert call(p=P(unknown=101)) == E_ARG and b"unknown 101" in err()
    assert call(p=P(clearance2=-1)) == E_ARG and ok in err()  # read only with dist2
    assert call(p=P(clearance2=-1), dist2=vp(dist2)) == E_ARG and b"clearance2 -1" in err()
    assert call(p=P(max_reach=-1)) == E_ARG and b"max_reach -1" in err()
    assert call(p=P(pad_=3)) == E_ARG and b"pad_ 3" in err()
    wide = np.zeros(10 ** 6, np.int8)  # 14 * 355 * (10^6 - 1) exceeds 2^31 - 2: beyond the reach's range check, which is not made -- nothing is summed over the image
    assert lib.pwpp_reach_grid(fake, 1000, 1000, 1, 2, vp(wide), None, P(base=255), vp(np.zeros(2, np.int32)), 1, fake, None) == E_ARG and b"exceeds 2^31 - 2" in err()
    assert call(nx=1000, ny=1000, cost=vp(wide), p=P(base=255)) == E_ARG and ok in err()
    # 4 the footprint parameters, each at both ends
    for name in ("front", "rear", "half_width"):
        for v in (-1, 1025):
            assert call(fp=F(**{name: v})) == E_ARG and b"%s %d: 0 .. 1024 ticks" % (name.encode(), v) in err()
        for v in (0, 1024):
            assert call(fp=F(**{name: v})) == E_ARG and ok in err()
    for v in (2, 3, -1):
        assert call(fp=F(flags=v)) == E_ARG and b"footprint flags %d" % v in err()
    assert call(fp=F(flags=1)) == E_ARG and ok in err()
    assert call(fp=F(pad_=(0, 5))) == E_ARG and b"pad_ {0, 5} of the footprint parameters" in err()
    assert call(fp=F(pad_=(7, 0))) == E_ARG and b"pad_ {7, 0}" in err()
    # 5 the counts and their product
    big8 = np.zeros(48, np.int8)
    for sets, frames in ((0, 1), (2, 1), (2, 3)):
        assert call(sets=sets, frames=frames, cost=vp(big8)) == E_ARG and b"%d pose sets for %d frames" % (sets, frames) in err()
    for n in (0, -1, 65537):
        assert call(n_traj=n) == E_ARG and b"%d trajectories: 1 .. 65536" % n in err()
    for n in (0, -1, 4097):
        assert call(n_steps=n) == E_ARG and b"%d steps: 1 .. 4096" % n in err()
    many = np.zeros(64 * 64 * 5, np.int8)  # 5 frames x 65536 trajectories x 256 steps: one frame past 2^26
    assert call(nx=64, ny=64, frames=5, cost=vp(many), n_traj=65536, n_steps=256, poses=fake) == E_ARG and b"5 frames x 65536 trajectories x 256 steps exceed 2^26" in err()
    # 6 the first pose entry out of range, by set, trajectory and step
    for k, (v, what) in enumerate(((2 ** 20 + 1, b"px"), (-2 ** 20 - 1, b"py"), (1025, b"ux"), (-1025, b"uy"))):
        q = poses.copy()
        q[1, 2, k] = v
        q[1, 1, k] = q[1, 1, k]
        assert call(poses=vp(q)) == E_ARG and b"pose of set 0, trajectory 1, step 2, {" in err() and str(v).encode() in err(), what
    q = np.tile(poses, (3, 1, 1, 1))
    q[2, 0, 1, 2] = 2000
    q[2, 1, 0, 0] = -2 ** 21
    assert call(poses=vp(q), sets=3, frames=3, cost=vp(big8)) == E_ARG and b"pose of set 2, trajectory 0, step 1, {8, 8, 2000, 0}" in err()
    for q in (np.tile(np.array([2 ** 20, -2 ** 20, 1024, -1024], np.int32), (2, 3, 1)), np.zeros((2, 3, 4), np.int32)):
        assert call(poses=vp(q)) == E_ARG and ok in err()   # the range's ends; u == (0, 0) is a skipped pose, not an error
    # 7 both outputs null
    assert call(prow=None, trow=None) == E_ARG and b"null pose rows and null trajectory rows" in err()
    assert call(prow=None) == E_ARG and ok in err()
    assert call(trow=None) == E_ARG and ok in err()
    # 8 the overlaps
    both = np.zeros(128, np.int32)
    assert call(prow=vp(both), trow=at(both, 32 * 6 - 4)) == E_ARG and b"pose rows and trajectory rows overlap" in err()
    assert call(prow=vp(both), trow=at(both, 32 * 6)) == E_ARG and ok in err()
    assert call(cost=at(prow, 3)) == E_ARG and b"cost and pose rows overlap" in err()
    assert call(dist2=vp(dist2), reach=at(dist2, 60)) == E_ARG and b"dist2 and reach overlap" in err()
    assert call(reach=vp(trow)) == E_ARG and b"reach and trajectory rows overlap" in err()
    # 9 mem, 10 the alignment in device memory
    assert call(mem=7) == E_ARG and b"mem 7" in err() and b"the footprints take" in err()
    assert call(mem=D, prow=at(both, 2)) == E_ARG and b"pose rows must be 4-byte aligned" in err()
    assert call(mem=D, trow=at(both, 1)) == E_ARG and b"trajectory rows must be 4-byte aligned" in err()
    assert call(mem=D, dist2=at(both, 130)) == E_ARG and b"dist2 image must be 4-byte aligned" in err()
    assert call(mem=D, reach=at(both, 3)) == E_ARG and b"reach image must be 4-byte aligned" in err()
    # the order
    bad_pose = poses.copy()
    bad_pose[0, 0, 3] = 5000
    assert call(cost=None, frames=0) == E_ARG and b"null cost" in err()
    assert call(frames=0, p=P(base=0)) == E_ARG and b"0 frames" in err()
    assert call(p=P(base=0), fp=F(front=-1)) == E_ARG and b"base 0" in err()
    assert call(fp=F(front=-1, rear=-1)) == E_ARG and b"front -1" in err()
    assert call(fp=F(rear=-1, half_width=-1)) == E_ARG and b"rear -1" in err()
    assert call(fp=F(half_width=-1, flags=2)) == E_ARG and b"half_width -1" in err()
    assert call(fp=F(flags=2, pad_=(1, 1))) == E_ARG and b"flags 2" in err()
    assert call(fp=F(pad_=(1, 1)), sets=0) == E_ARG and b"pad_ {1, 1}" in err()
    assert call(sets=0, n_traj=0) == E_ARG and b"0 pose sets" in err()
    assert call(n_traj=0, n_steps=0) == E_ARG and b"0 trajectories" in err()
    assert call(n_steps=5000, poses=vp(bad_pose)) == E_ARG and b"5000 steps" in err()
    assert call(poses=vp(bad_pose), prow=None, trow=None) == E_ARG and b"pose of set 0, trajectory 0, step 0" in err()
    assert call(prow=None, trow=None, cost=at(prow, 3)) == E_ARG and b"null pose rows and null" in err()
    assert call(cost=at(prow, 3), mem=7) == E_ARG and b"overlap" in err()
    assert call(mem=7, prow=at(both, 2)) == E_ARG and b"mem 7" in err()


CPP = r"""
#include "patchwork/patchworkpp.h"
#ifndef PWPP_HAS_FOOTPRINT
#error "include/pwpp.h does not announce the footprints"
#endif
static_assert(sizeof(pwpp_footprint_params) == 24 && sizeof(pwpp_footprint_pose_row) == 32 && sizeof(pwpp_footprint_traj_row) == 32, "the footprint structs");
static_assert(PWPP_FOOT_FREE == 0 && PWPP_FOOT_HIT == 1 && PWPP_FOOT_SKIPPED == 2 && PWPP_FOOT_SUB == 16 && PWPP_FOOT_MAX_EXTENT == 1024 && PWPP_FOOT_MAX_STEPS == 4096, "the values");
long use(patchwork::PatchWorkpp &pw) {
    patchwork::PatchWorkpp::FootprintParams f;
    patchwork::PatchWorkpp::ReachParams r;
    if (f.front != 3.4 || f.rear != 1.1 || f.half_width != 0.9 || f.pad != 0 || f.outside_blocks) return -1;
    f.pad = 12, f.outside_blocks = true;
    const std::vector<int8_t> cost(160 * 160, 0);
    const std::vector<double> poses = {1.0, 2.0, 0.1, 1.5, 2.0, 0.2, -3.0, 4.0, 0.0, -3.0, 4.5, std::numeric_limits<double>::quiet_NaN()};
    const patchwork::PatchWorkpp::Footprints a = pw.checkFootprints(cost, -40.0, -40.0, 0.5, 160, 160, poses, 2);
    const patchwork::PatchWorkpp::Footprints b = pw.checkFootprints(cost, -40.0, -40.0, 0.5, 160, 160, poses, 2, f, r, std::vector<int32_t>(160 * 160, 7));
    return (long)a.poses[0].status + b.trajectories[1].reach_last + a.n_traj + b.n_steps;
}
"""


@pytest.mark.parametrize("flavour", ["plain", "eigen_shim"])
def test_cpp_mirror_methods_compile(tmp_path, flavour):
    src = tmp_path / "footprints.cpp"
    src.write_text(CPP)
    cmd = ["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(PKG, "include"), "-I", os.path.join(ROOT, "include")]
    cmd += ["-DPWPP_NO_EIGEN"] if flavour == "plain" else ["-I", os.path.join(ROOT, "oracle", "eigen_shim")]
    subprocess.run(cmd + [str(src)], check=True)


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "footprints.c"
    src.write_text('#include "pwpp.h"\nint f(const pwpp_reach_params *p, const pwpp_footprint_params *fp, pwpp_footprint_pose_row *a, pwpp_footprint_traj_row *b,\n'
                   '      const pwpp_ground_grid *g, int32_t pose[4]) {\n'
                   '    return pwpp_footprint_grid(0, 1, 1, 1, PWPP_MEM_HOST, 0, 0, 0, p, fp, pose, 1, 1, 1, a, b) + pwpp_footprint_covers(fp, pose, 0, 0) +\n'
                   '           pwpp_footprint_pose(g, 0.0, 0.0, 0.0, pose) + (int)sizeof(*fp) + (a->status == PWPP_FOOT_SKIPPED) + (b->first_hit < PWPP_FOOT_MAX_STEPS) +\n'
                   '           (fp->flags & PWPP_FOOT_OUTSIDE_BLOCKS) + PWPP_FOOT_SUB + PWPP_FOOT_MAX_EXTENT + PWPP_FOOT_FREE + PWPP_FOOT_HIT; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)


# ---- the stand-alone program ---------------------------------------------------------------------------------------------------------
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
    tmp = tmp_path_factory.mktemp("footprint_check")
    exe = tmp / "footprint_check"
    flags = SANITIZE if sanitizers_work(tmp) else []
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off"] + flags +
                   ["-I", os.path.join(PKG, "csrc"), os.path.join(ROOT, "tools", "footprint_check.cpp"), "-o", str(exe)], check=True)
    return exe


def test_footprint_program_builds_and_passes(checker):
    r = subprocess.run([str(checker)], capture_output=True, text=True)  # (a stand-alone child process with its own main)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 mismatches" in r.stdout
    assert int(r.stdout.split("footprint_check: ")[1].split(" cases")[0]) >= 3000


# ---- the restatement and the one text: each property below is asked of csrc/pwpp_footprint.h, run by tools/footprint_check.cpp --------
def dumped(checker, tmp_path, cost, p, fp, poses, deal, dist2=None, reach=None, want_pose=True):
    """(pose_rows, traj_rows) of footprint_check's dump mode -- the kernels' functions dealt as kernel `deal` deals them -- shaped as fr.footprints."""
    c3 = fr.as_frames(cost, np.int8)
    frames, ny, nx = c3.shape
    q = fr.as_poses(poses)
    sets, n_traj, n_steps = q.shape[:3]
    d = tmp_path / ("dump%d" % len(list(tmp_path.iterdir())))
    d.mkdir()
    files = [("cost", c3), ("poses", q)] + ([("dist2", np.ascontiguousarray(dist2, np.int32))] if dist2 is not None else []) + \
        ([("reach", np.ascontiguousarray(reach, np.int32))] if reach is not None else [])
    for name, a in files:
        a.tofile(d / name)
    args = ["dump", str(d / "cost"), str(nx), str(ny), str(frames)] + [str(p[k]) for k in ("base", "lethal", "unknown", "clearance2")]
    args += [str(d / "dist2") if dist2 is not None else "-", str(d / "reach") if reach is not None else "-"]
    args += [str(fp[k]) for k in ("front", "rear", "half_width", "flags")] + [str(d / "poses"), str(sets), str(n_traj), str(n_steps), str(deal), "1" if want_pose else "0", str(d / "out")]
    subprocess.run([str(checker)] + args, check=True, stdout=subprocess.DEVNULL)
    prow = np.fromfile(str(d / "out.pose"), fr.POSE_ROW).reshape(frames, n_traj, n_steps) if want_pose else None
    return prow, np.fromfile(str(d / "out.traj"), fr.TRAJ_ROW).reshape(frames, n_traj)


def every_way(checker, tmp_path, cost, p, fp, poses, dist2=None, reach=None, windowed=True):
    """The rows by both deals of the one text (the waves' with and without pose rows) and by both routes of the restatement: all equal, byte for byte."""
    want = fr.footprints(cost, p, fp, poses, dist2, reach, "brute")
    assert fr.certify(cost, p, fp, poses, want[0], want[1], dist2, reach) == []
    if windowed:
        other = fr.footprints(cost, p, fp, poses, dist2, reach, "windowed")
        assert other[0].tobytes() == want[0].tobytes() and other[1].tobytes() == want[1].tobytes(), "the windowed visit differs from the brute force"
    for deal, want_pose in ((1, True), (2, True), (2, False)):
        got = dumped(checker, tmp_path, cost, p, fp, poses, deal, dist2, reach, want_pose)
        assert got[0] is None or got[0].tobytes() == want[0].tobytes(), "deal %d: pose rows" % deal
        assert got[1].tobytes() == want[1].tobytes(), "deal %d (pose rows %s): trajectory rows" % (deal, want_pose)
    return want


def fan(rng, n_traj, n_steps, nx, ny, margin=20, us=None):
    q = np.zeros((n_traj, n_steps, 4), np.int32)
    q[..., 0] = rng.integers(-margin, 16 * nx + margin, (n_traj, n_steps))
    q[..., 1] = rng.integers(-margin, 16 * ny + margin, (n_traj, n_steps))
    q[..., 2:] = rng.integers(-9, 10, (n_traj, n_steps, 2)) if us is None else np.asarray(us)[rng.integers(0, len(us), (n_traj, n_steps))]
    return q


def test_certify_refuses_a_wrong_row():
    cost = fr.random_images(1, 9, 11, 2)
    p, fp = rr.params(), fr.foot_params(30, 8, 10)
    poses = fan(np.random.default_rng(1), 3, 5, 11, 9)
    prow, trow = fr.footprints(cost, p, fp, poses)
    assert fr.certify(cost, p, fp, poses, prow, trow) == []
    bad = prow.copy()
    bad[0, 1, 2]["covered"] += 1
    assert len(fr.certify(cost, p, fp, poses, bad, trow)) == 1
    bad = trow.copy()
    bad[0, 2]["sum_term"] -= 1
    assert "trajectory row" in fr.certify(cost, p, fp, poses, None, bad)[0]


def test_scaling_u_changes_no_byte(checker, tmp_path):
    rng = np.random.default_rng(3)
    cost, reach = fr.random_images(2, 12, 13, 4), rng.integers(0, 999, (2, 12, 13)).astype(np.int32)
    p, fp = rr.params(base=3, unknown=7), fr.foot_params(front=44, rear=9, half_width=17)
    base = fan(rng, 4, 6, 13, 12, us=[(1, 0), (0, -1), (3, 4), (-4, 3), (1, 1), (2, -5), (0, 0)])
    want = every_way(checker, tmp_path, cost, p, fp, base, reach=reach)
    for k in (2, 100, 204):  # (1, 0) and (1024 > 204, 0) below; (3, 4) and (300, 400); 5 * 204 = 1020 <= 1024
        scaled = base.copy()
        scaled[..., 2:] *= k
        got = every_way(checker, tmp_path, cost, p, fp, scaled, reach=reach, windowed=(k == 2))
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), k
    axis = base.copy()
    axis[..., 2:] = (1, 0)
    far = axis.copy()
    far[..., 2] = 1024
    assert every_way(checker, tmp_path, cost, p, fp, axis)[0].tobytes() == every_way(checker, tmp_path, cost, p, fp, far)[0].tobytes()


def test_reversing_u_swaps_front_and_rear(checker, tmp_path):
    rng = np.random.default_rng(5)
    cost = fr.random_images(1, 10, 14, 6)
    p = rr.params(base=2)
    poses = fan(rng, 3, 7, 14, 10)
    turned = poses.copy()
    turned[..., 2:] *= -1
    a = every_way(checker, tmp_path, cost, p, fr.foot_params(front=50, rear=6, half_width=12), poses)
    b = every_way(checker, tmp_path, cost, p, fr.foot_params(front=6, rear=50, half_width=12), turned)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert a[0].tobytes() != fr.footprints(cost, p, fr.foot_params(front=50, rear=6, half_width=12), turned)[0].tobytes()


def test_the_eight_symmetries_of_the_square_map_footprints_onto_footprints(checker, tmp_path):
    rng = np.random.default_rng(8)
    n = 11
    cost = fr.random_images(1, n, n, 9)[0]
    dist2 = rng.integers(0, 30, (n, n)).astype(np.int32)
    p, fp = rr.params(base=2, unknown=4, clearance2=3), fr.foot_params(front=37, rear=11, half_width=13)
    poses = fan(rng, 3, 6, n, n)
    want = every_way(checker, tmp_path, cost, p, fp, poses, dist2=dist2)
    T = 16 * n  # the image in ticks: a cell centre 16 i + 8 goes to T - (16 i + 8), the centre of cell n - 1 - i
    for flip_x in (False, True):
        for flip_y in (False, True):
            for swap in (False, True):
                c, d, q = cost, dist2, poses.copy()
                if flip_x:
                    c, d = c[:, ::-1], d[:, ::-1]
                    q[..., 0], q[..., 2] = T - q[..., 0], -q[..., 2]
                if flip_y:
                    c, d = c[::-1, :], d[::-1, :]
                    q[..., 1], q[..., 3] = T - q[..., 1], -q[..., 3]
                if swap:
                    c, d = c.T, d.T
                    q = q[..., [1, 0, 3, 2]]
                got = every_way(checker, tmp_path, np.ascontiguousarray(c), p, fp, np.ascontiguousarray(q), dist2=np.ascontiguousarray(d), windowed=False)
                # a reflection turns "left of u" into "right of u": the rectangle is symmetric across u, so the cells are the images of the cells
                for name in ("status", "covered", "outside", "blocked", "unknown", "max_term", "min_dist2"):
                    assert np.array_equal(got[0][name], want[0][name]), (flip_x, flip_y, swap, name)
                for name in ("first_hit", "free_steps", "last", "max_term", "sum_term", "unknown", "min_dist2"):
                    assert np.array_equal(got[1][name], want[1][name]), (flip_x, flip_y, swap, name)


def test_cells_exactly_on_an_edge_are_covered_and_one_tick_less_drops_exactly_them(checker, tmp_path):
    """u = (3, 4), |u| = 5: a = 3 dx + 4 dy and b = 3 dy - 4 dx are integers, and with extents that are multiples of 5 the edges a = 5 front,
    a = -5 rear, |b| = 5 half_width pass through lattice points."""
    n = 24
    cost = np.zeros((n, n), np.int8)
    p = rr.params()
    pose = (16 * 12 + 8, 16 * 12 + 8, 3, 4)  # p on a cell centre: d = 16 (i - 12, j - 12), a and b are multiples of 16
    full = fr.foot_params(front=80, rear=80, half_width=80)  # the edges at |a| = 400 = 16 * 25, |b| = 400
    cells = [(x, y) for y in range(n) for x in range(n)]
    a_of = lambda x, y: 3 * 16 * (x - 12) + 4 * 16 * (y - 12)
    b_of = lambda x, y: 3 * 16 * (y - 12) - 4 * 16 * (x - 12)
    inside = lambda fp: {c for c in cells if fr.covers(fp, pose, *c)}
    whole = inside(full)
    on_front = {c for c in whole if a_of(*c) == 400}
    on_rear = {c for c in whole if a_of(*c) == -400}
    on_side = {c for c in whole if abs(b_of(*c)) == 400}
    assert len(on_front) >= 3 and len(on_rear) >= 3 and len(on_side) >= 6, "cells exactly on each edge"
    for name, gone in (("front", on_front), ("rear", on_rear), ("half_width", on_side)):
        less = dict(full)
        less[name] -= 1
        assert inside(less) == whole - gone, name
        for fp, count in ((full, len(whole)), (less, len(whole - gone))):
            want = every_way(checker, tmp_path, cost, p, fp, np.array([pose], np.int32))
            assert want[0]["covered"][0, 0, 0] == count and want[0]["outside"][0, 0, 0] == 0
    F = pwpp_hip.FootprintParams(80, 80, 80, 0, (0, 0))
    assert {c for c in cells if pwpp_hip.footprint_covers(F, pose, *c)} == whole


def test_lemma_1_holds_on_random_poses():
    rng = np.random.default_rng(12)
    for _ in range(60):
        f, r, w = (int(v) for v in rng.integers(0, 1025, 3))
        fp = fr.foot_params(f, r, w)
        pose = (int(rng.integers(-2 ** 20, 2 ** 20)), int(rng.integers(-2 ** 20, 2 ** 20)), int(rng.integers(-1024, 1025)), int(rng.integers(-1024, 1025)))
        if pose[2] == 0 and pose[3] == 0:
            continue
        cx, cy = pose[0] >> 4, pose[1] >> 4
        xs, ys = np.arange(cx - 140, cx + 141), np.arange(cy - 140, cy + 141)   # beyond E + W = 2048 ticks = 128 cells on every side
        m = fr.covered_mask(fp, pose, xs, ys)
        dx, dy = np.abs(16 * xs + 8 - pose[0])[None, :], np.abs(16 * ys + 8 - pose[1])[:, None]
        bound = max(f, r) + w
        assert not (m & ((dx > bound) | (dy > bound))).any()
        x0, y0, ww, hh = fr.window(fp, pose)
        in_window = ((ys >= y0) & (ys < y0 + hh))[:, None] & ((xs >= x0) & (xs < x0 + ww))[None, :]
        assert not (m & ~in_window).any(), "a covered cell outside the window"
        assert ww <= 2 * bound // 16 + 1 and hh <= 2 * bound // 16 + 1 and ww * hh <= 257 * 257
        # the largest products of the rule, in Python integers: below 2^45
        assert max(abs(pose[2]) * 2048 + abs(pose[3]) * 2048, 1) ** 2 < 2 ** 45 and max(f, r, w) ** 2 * (pose[2] ** 2 + pose[3] ** 2) < 2 ** 45


def test_lemma_2_a_cell_the_rectangle_touches_is_covered_by_the_padded_one():
    rng = np.random.default_rng(14)
    touched = only_touched = 0
    for _ in range(150):
        f, r, w = (int(v) for v in rng.integers(0, 90, 3))
        fp, padded = fr.foot_params(f, r, w), fr.foot_params(f + 12, r + 12, w + 12)
        pose = (int(rng.integers(0, 400)), int(rng.integers(0, 400)), int(rng.integers(-20, 21)), int(rng.integers(-20, 21)))
        if pose[2] == 0 and pose[3] == 0:
            continue
        for iy in range(-10, 36):
            for ix in range(-10, 36):
                if fr.touches(fp, pose, ix, iy):
                    touched += 1
                    only_touched += not fr.covers(fp, pose, ix, iy)
                    assert fr.covers(padded, pose, ix, iy), (fp, pose, ix, iy)
                else:
                    assert not fr.covers(fp, pose, ix, iy), "a covered centre is a point of the rectangle in its cell"
    assert touched > 5000 and only_touched > 1000


def test_a_footprint_of_all_zeros_covers_the_cell_whose_centre_is_p_or_nothing(checker, tmp_path):
    cost = np.zeros((5, 6), np.int8)
    cost[2, 3] = 100
    p, fp = rr.params(), fr.foot_params(0, 0, 0)
    poses = np.array([[(16 * 3 + 8, 16 * 2 + 8, 1, 0), (16 * 3 + 8, 16 * 2 + 8, -3, 7), (16 * 3 + 7, 16 * 2 + 8, 1, 0), (16 * 3 + 8, 16 * 2 + 9, 0, 1), (8, 8, 1, 1),
                       (-8, -8, 1, 0), (16 * 6 + 8, 8, 5, 5)]], np.int32)
    want = every_way(checker, tmp_path, cost, p, fp, poses)
    assert want[0]["covered"][0, 0].tolist() == [1, 1, 0, 0, 1, 1, 1] and want[0]["hit"][0, 0].tolist() == [15, 15, -1, -1, -1, -1, -1]
    assert want[0]["outside"][0, 0].tolist() == [0, 0, 0, 0, 0, 1, 1] and want[0]["status"][0, 0].tolist() == [fr.HIT, fr.HIT, fr.FREE, fr.FREE, fr.FREE, fr.FREE, fr.FREE]
    for ix in range(-2, 8):
        for iy in range(-2, 7):
            assert fr.covers(fp, poses[0, 0], ix, iy) == ((ix, iy) == (3, 2))


def test_negative_ticks_floor(checker, tmp_path):
    """Cell -1 covers the ticks [-16, 0): a pose at tick -1 lies in cell -1, at tick -16 too, at -17 in cell -2; reach_last looks at px >> 4."""
    cost = np.zeros((3, 3), np.int8)
    reach = np.arange(9, dtype=np.int32).reshape(3, 3) + 50
    p, fp = rr.params(), fr.foot_params(front=8, rear=8, half_width=8)   # a cell-sized square: covers the centres within 8 ticks, edges included
    poses = np.array([[(-8, -8, 1, 0)], [(-1, 8, 1, 0)], [(0, 8, 1, 0)], [(-16, 8, 0, 1)], [(-17, 8, 0, 1)], [(15, 47, 1, 0)], [(16, 48, 1, 0)]], np.int32)
    want = every_way(checker, tmp_path, cost, p, fp, poses, reach=reach)
    rows, trajs = want[0][0, :, 0], want[1][0]
    assert rows["covered"].tolist() == [1, 1, 2, 2, 1, 1, 4] and rows["outside"].tolist() == [1, 1, 1, 2, 1, 0, 2]
    assert fr.covers(fp, poses[3, 0], -2, 0) and fr.covers(fp, poses[3, 0], -1, 0) and fr.covers(fp, poses[4, 0], -2, 0) and not fr.covers(fp, poses[4, 0], -1, 0)
    assert fr.covers(fp, poses[0, 0], -1, -1) and not fr.covers(fp, poses[0, 0], 0, 0) and fr.covers(fp, poses[2, 0], -1, 0) and fr.covers(fp, poses[2, 0], 0, 0)
    assert trajs["reach_last"].tolist() == [fr.REACH_NONE, fr.REACH_NONE, 50, fr.REACH_NONE, fr.REACH_NONE, 50 + 2 * 3 + 0, fr.REACH_NONE]
    assert fr.window(fp, (-8, -8, 1, 0)) == (-2, -2, 3, 3) and fr.window(fp, (-17, 8, 0, 1)) == (-2, -1, 2, 3)  # (the E + W square: centres within 16 ticks)


def test_random_cases_by_every_way(checker, tmp_path):
    """The two routes of the restatement and both deals of the one text on images with walls and unknown cells; the suite holds every kind."""
    statuses, hits = set(), set()
    for seed in range(6):
        rng = np.random.default_rng(100 + seed)
        frames, ny, nx = 2, int(rng.integers(1, 15)), int(rng.integers(1, 15))
        cost = fr.random_images(frames, ny, nx, 200 + seed)
        dist2 = rng.integers(0, 40, cost.shape).astype(np.int32) if seed % 2 else None
        reach = rng.integers(0, 9999, cost.shape).astype(np.int32) if seed % 3 else None
        p = rr.params(base=int(rng.integers(1, 256)), lethal=int(rng.integers(90, 102)), unknown=int(rng.integers(-1, 30)), clearance2=int(rng.integers(0, 10)))
        ew = (7, 23, 39, 90, 90, 300)[seed]   # the packed deal's slots of 1, 16 and 32 lanes, and one pose a round
        w = int(rng.integers(0, ew // 2 + 1))
        fp = fr.foot_params(front=ew - w, rear=int(rng.integers(0, ew - w + 1)), half_width=w, flags=seed % 2)
        poses = np.stack([fan(rng, 3, 9, nx, ny, margin=12) for _ in range(frames if seed % 2 else 1)])
        poses[rng.random(poses.shape[:3]) < 0.2, 2:] = 0
        want = every_way(checker, tmp_path, cost, p, fp, poses, dist2=dist2, reach=reach)
        statuses |= set(np.unique(want[0]["status"]).tolist())
        hits |= set((want[1]["first_hit"] >= 0).reshape(-1).tolist())
    assert statuses == {fr.FREE, fr.HIT, fr.SKIPPED} and hits == {True, False}


# ---- the host helpers ----------------------------------------------------------------------------------------------------------------
def test_footprint_covers_is_the_rule(lib):
    rng = np.random.default_rng(21)
    n = 0
    for _ in range(40):
        f, r, w = (int(v) for v in rng.integers(0, 1025, 3))
        fp, F = fr.foot_params(f, r, w), pwpp_hip.FootprintParams(f, r, w, 0, (0, 0))
        pose = [int(rng.integers(-2 ** 20, 2 ** 20 + 1)), int(rng.integers(-2 ** 20, 2 ** 20 + 1)), int(rng.integers(-1024, 1025)), int(rng.integers(-1024, 1025))]
        cx, cy = pose[0] >> 4, pose[1] >> 4
        for _ in range(60):
            ix, iy = cx + int(rng.integers(-140, 141)), cy + int(rng.integers(-140, 141))
            assert pwpp_hip.footprint_covers(F, pose, ix, iy) == fr.covers(fp, pose, ix, iy)
            n += fr.covers(fp, pose, ix, iy)
        for ix, iy in ((2 ** 31 - 1, -2 ** 31), (-2 ** 31, 2 ** 31 - 1), (0, 0)):   # any int cell: the far ones are never covered, and nothing overflows
            assert pwpp_hip.footprint_covers(F, pose, ix, iy) == fr.covers(fp, pose, ix, iy)
    assert n > 100
    F = pwpp_hip.FootprintParams(10, 10, 10, 0, (0, 0))
    assert not pwpp_hip.footprint_covers(F, (8, 8, 0, 0), 0, 0)   # u == (0, 0) covers nothing
    far = (2 ** 20, -2 ** 20, 1024, -1024)   # the corner of the range: the centre of cell (2^16, -2^16) lies 8 ticks beside p in x and in y
    assert not pwpp_hip.footprint_covers(F, far, 2 ** 16, -2 ** 16) and pwpp_hip.footprint_covers(pwpp_hip.FootprintParams(12, 12, 12, 0, (0, 0)), far, 2 ** 16, -2 ** 16)
    q4 = lambda *v: (ctypes.c_int32 * 4)(*v)
    err = lib.pwpp_last_error
    assert lib.pwpp_footprint_covers(None, q4(0, 0, 1, 0), 0, 0) == E_ARG and b"null footprint parameters" in err()
    assert lib.pwpp_footprint_covers(ctypes.byref(F), None, 0, 0) == E_ARG and b"null pose" in err()
    assert lib.pwpp_footprint_covers(ctypes.byref(pwpp_hip.FootprintParams(1025, 0, 0, 0, (0, 0))), q4(0, 0, 1, 0), 0, 0) == E_ARG and b"front 1025" in err()
    assert lib.pwpp_footprint_covers(ctypes.byref(pwpp_hip.FootprintParams(1, 0, 0, 0, (0, 1))), q4(0, 0, 1, 0), 0, 0) == E_ARG and b"pad_" in err()
    for bad in ((2 ** 20 + 1, 0, 1, 0), (0, -2 ** 20 - 1, 1, 0), (0, 0, 1025, 0), (0, 0, 0, -1025)):
        assert lib.pwpp_footprint_covers(ctypes.byref(F), q4(*bad), 0, 0) == E_ARG and b"|px|, |py| <= 2^20" in err()
        with pytest.raises(pwpp_hip.PwppError):
            pwpp_hip.footprint_covers(F, bad, 0, 0)


def test_footprint_pose_is_the_stated_convenience(lib):
    g = pwpp_hip.GroundGrid(-12.5, 3.25, 0.5, 40, 30, 0, 0)
    rng = np.random.default_rng(22)
    for _ in range(200):
        x, y, yaw = float(rng.uniform(-40, 40)), float(rng.uniform(-40, 40)), float(rng.uniform(-7, 7))
        want = [int(math.floor((x - g.x0) / g.cell * 16)), int(math.floor((y - g.y0) / g.cell * 16)), int(round(1024 * math.cos(yaw))), int(round(1024 * math.sin(yaw)))]
        got = pwpp_hip.footprint_pose(g, x, y, yaw).tolist()
        assert got[:2] == want[:2] and abs(got[2] - want[2]) <= (abs(1024 * math.cos(yaw)) % 1 == 0.5) and abs(got[3] - want[3]) <= (abs(1024 * math.sin(yaw)) % 1 == 0.5)
    assert pwpp_hip.footprint_pose(g, -12.5, 3.25, 0.0).tolist() == [0, 0, 1024, 0]
    assert pwpp_hip.footprint_pose(g, -12.5 - 0.5 / 16 / 2, 3.25 + 0.5, math.pi / 2).tolist() == [-1, 16, 0, 1024]   # a negative tick floors
    assert pwpp_hip.footprint_pose(g, 0.0, 0.0, math.pi).tolist()[2:] == [-1024, 0]
    edge = 2 ** 20 * 0.5 / 16   # 2^20 ticks from the origin: the last position accepted
    assert pwpp_hip.footprint_pose(g, g.x0 + edge, g.y0 - edge, 0.0).tolist()[:2] == [2 ** 20, -2 ** 20]
    q = (ctypes.c_int32 * 4)()
    err = lib.pwpp_last_error
    assert lib.pwpp_footprint_pose(None, 0.0, 0.0, 0.0, q) == E_ARG and b"null grid" in err()
    assert lib.pwpp_footprint_pose(ctypes.byref(g), 0.0, 0.0, 0.0, None) == E_ARG and b"null pose" in err()
    for x, y, yaw in ((math.nan, 0, 0), (0, math.inf, 0), (0, 0, math.nan), (0, 0, -math.inf)):
        assert lib.pwpp_footprint_pose(ctypes.byref(g), x, y, yaw, q) == E_ARG and b"finite values expected" in err()
    for x, y in ((g.x0 + edge + 0.5 / 16, 0.0), (0.0, g.y0 - edge - 0.5 / 16), (1e300, 0.0)):
        assert lib.pwpp_footprint_pose(ctypes.byref(g), x, y, 0.0, q) == E_ARG and b"at most 2^20 expected" in err()
        with pytest.raises(pwpp_hip.PwppError):
            pwpp_hip.footprint_pose(g, x, y, 0.0)
    bad = pwpp_hip.GroundGrid(0.0, 0.0, 0.0, 4, 4, 0, 0)
    assert lib.pwpp_footprint_pose(ctypes.byref(bad), 0.0, 0.0, 0.0, q) == E_ARG and b"cell size" in err()
