"""The per-frame input transform (pwpp_set_input_transforms) on a real MI355X.

Rule under test (include/pwpp.h): with transforms set, every result of an estimate call is what the same call returns for the
cloud whose points are T_f(p) -- bit for bit.  So every case runs two handles: one WITH transforms on the sensor-frame cloud C,
one WITHOUT on transform_points(T, C) (the library's own host function, checked against a numpy restatement by
tests/test_input_transform_cpu.py), and compares bytes: counts, both index lists in cloud order, patch records, labels, point
patches and distances, the xyz getters, state and plane state.  No tolerance anywhere.

The clouds: KITTI fixture frames un-levelled with the (approximate) inverse of a tilt, so that T levels them again and the fits
see real ground; a few input heights of FLT_MIN (not special: they do not map onto the marker), and -- under a pure translation --
a few points that map exactly onto FLT_MIN and must be skipped."""
import ctypes

import numpy as np
import pytest

import input_transform_ref as xf
import oracle_lib as ol
import pwpp_hip
from test_gpu_inputs import Placed, encode, submit
from test_gpu_parity import apply_variant, assert_frame_equal
from test_tiny_fits import ROS_LAUNCH

pytestmark = pytest.mark.gpu

F32 = np.float32
TINY = np.finfo(F32).tiny  # FLT_MIN
# five different transforms: four tilts that level their clouds again, and one pure translation whose z part is FLT_MIN
TILTS = [xf.rigid(np.radians(3.0), np.radians(-5.0), np.radians(20.0), t=(0.2, -0.1, 0.15)),
         xf.rigid(np.radians(-1.5), np.radians(2.0), np.radians(-75.0), t=(-0.4, 0.3, -0.05)),
         xf.rigid(np.radians(0.7), np.radians(8.0), 0.0, t=(0.0, 0.0, 0.3)),
         xf.rigid(np.radians(-4.0), np.radians(-0.5), np.radians(170.0), t=(1.0, -1.0, 0.0), scale=0.001)]  # a driver's millimetres
SHIFT = np.array([[1, 0, 0, 0.5], [0, 1, 0, -0.25], [0, 0, 1, TINY]], F32)
LAYOUTS = {"row4": ("matrix", 4, pwpp_hip.LAYOUT_ROW_MAJOR), "row3": ("matrix", 3, pwpp_hip.LAYOUT_ROW_MAJOR),
           "col4": ("matrix", 4, pwpp_hip.LAYOUT_COL_MAJOR), "fields32": ("fields", 32, (4, 12, 20, 0))}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8)


def pre_transformed(T, c):
    out = c.copy()
    out[:, :3] = pwpp_hip.transform_points(T, c[:, :3])
    return out


def sensor_cloud(level, T, seed):
    """A cloud in the sensor's frame that T maps (nearly) onto the levelled frame `level`, with planted FLT_MIN heights."""
    rng = np.random.default_rng(seed)
    if T is SHIFT:
        c = level.copy()
        pick = rng.choice(len(c), 12, replace=False)
        c[pick[:6], 2] = 0.0      # 0 + FLT_MIN = FLT_MIN: maps exactly onto the skip marker
        c[pick[6:], 2] = TINY     # FLT_MIN + FLT_MIN: an input marker that is NOT special
    else:
        c = xf.transform_cloud(xf.inverse(T), level)
        c[rng.choice(len(c), 6, replace=False), 2] = TINY  # lands near the ground level, a point like any other
    return np.ascontiguousarray(c, F32)


@pytest.fixture(scope="module")
def clouds(kitti):
    """(T, C, transform_points(T, C)) for five frames; frame 4 is the pure translation."""
    out = []
    for k, T in enumerate(TILTS + [SHIFT]):
        c = sensor_cloud(kitti[k], T, 40 + k)
        out.append((T, c, pre_transformed(T, c)))
    pre = out[4][2]
    assert (pre[:, 2] == TINY).sum() == 6 and (out[4][1][:, 2] == TINY).sum() == 6
    assert not (out[0][2][:, 2] == TINY).any()
    assert abs(np.median(out[0][2][:, 2]) - np.median(kitti[0][:, 2])) < 0.01  # levelled again: real ground under the fits
    return out


def make(params=None, order=pwpp_hip.ORDER_CLOUD, options=(), records=False):
    h = pwpp_hip.Handle(params)
    h.set_order(order)
    h.set_point_planes(True)
    h.set_labels(True)
    if records:
        h.set_point_records(True)
    for k, v in options:
        h.set_option(k, v)
    return h


def state_bytes(h, i):
    st = h.state(i)
    hist = [h.history(i, w, r).tobytes() for w in range(2) for r in range(4)]
    return bytes(st), h.plane_state(i).tobytes(), hist


def assert_same(a, fa, b, fb, state=None):
    """Frame fa of handle a equals frame fb of handle b, byte for byte."""
    assert a.counts(fa) == b.counts(fb)
    assert np.array_equal(a.all_counts()[fa], b.all_counts()[fb])  # RNR, out of range and dropped (skip marker) counts too
    for name in ("ground_indices", "nonground_indices", "patch_records", "labels", "point_patches", "point_distances", "ground",
                 "nonground", "centers", "normals"):
        x, y = getattr(a, name)(fa), getattr(b, name)(fb)
        assert x.shape == y.shape and np.array_equal(bits(x), bits(y)), name
    if state is not None:
        assert state_bytes(a, state[0]) == state_bytes(b, state[1])


# ---- 1. the default path ---------------------------------------------------------------------------------------------------
def test_one_frame_five_frames_broadcast_and_off_again(clouds, oracle_built):
    on, off, never = make(), make(), make()
    T, c, pre = clouds[0]
    on.set_input_transforms(T)
    on.estimate_ground_batch([c])
    off.estimate_ground_batch([pre])
    assert_same(on, 0, off, 0, state=(0, 0))
    # ... and held against the oracle's restatement run on the pre-transformed cloud
    ref = ol.Estimator(oracle_built.restatement(), arith=ol.ARITH_FXP).run(pre)
    assert_frame_equal(on, 0, ref, len(pre))
    # five frames, five transforms (count == frames), an empty frame among them
    empty = np.zeros((0, 4), F32)
    cs = [clouds[0][1], clouds[1][1], empty, clouds[3][1], clouds[4][1]]
    ps = [clouds[0][2], clouds[1][2], empty, clouds[3][2], clouds[4][2]]
    on.set_input_transforms(np.stack([t for t, _, _ in clouds]))
    on.estimate_ground_batch(cs)
    off.estimate_ground_batch(ps)
    for f in range(5):
        assert_same(on, f, off, f, state=(f, f))
    assert on.counts(2) == (0, 0, 0)
    assert on.all_counts()[4, 5] == 6 and on.all_counts()[0, 5] == 0  # six points mapped onto FLT_MIN; six input FLT_MINs did not
    # broadcast: one transform for every frame
    on.set_input_transforms(clouds[2][0].reshape(12))
    same_t = [clouds[2][1], empty, clouds[2][1][:5000]]
    on.estimate_ground_batch(same_t)
    off.estimate_ground_batch([clouds[2][2], empty, clouds[2][2][:5000]])
    for f in range(3):
        assert_same(on, f, off, f, state=(f, f))
    # off again: a handle that never had transforms
    on.set_input_transforms(None)
    on.estimate_ground_batch(same_t)
    never.estimate_ground_batch(same_t)
    for f in range(3):
        assert_same(on, f, never, f, state=(f, f))
    for h in (on, off, never):
        h.close()
    # set and turned off before any call: nothing was allocated for it (the same calls leave the same workspace)
    was_set, never = make(), make()
    was_set.set_input_transforms(T)
    was_set.set_input_transforms(None)
    for h in (was_set, never):
        h.estimate_ground_batch(same_t)
    assert was_set.workspace_bytes() == never.workspace_bytes()
    was_set.close()
    never.close()


# ---- 2. input forms ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mem", ["host", "pinned_slab", "device"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_layouts_and_memory_kinds(clouds, layout, mem, monkeypatch):
    import test_gpu_inputs
    monkeypatch.setattr(test_gpu_inputs, "LAYOUTS", dict(test_gpu_inputs.LAYOUTS, **LAYOUTS))
    kind, a, b = LAYOUTS[layout]
    cols = a if kind == "matrix" else 4
    T = clouds[1][0]
    cs = [np.ascontiguousarray(clouds[1][1][:, :cols]), np.ascontiguousarray(clouds[1][1][:30011, :cols])]
    ps = [np.ascontiguousarray(clouds[1][2][:, :cols]), np.ascontiguousarray(clouds[1][2][:30011, :cols])]
    on, off = make(), make()
    on.set_input_transforms(T)
    pc = Placed([encode(c, layout, 3 + k) for k, c in enumerate(cs)], mem)
    pp = Placed([encode(p, layout, 3 + k) for k, p in enumerate(ps)], mem)
    try:
        submit(on, pc, layout, [len(c) for c in cs], pwpp_hip.MODE_FRESH)
        submit(off, pp, layout, [len(p) for p in ps], pwpp_hip.MODE_FRESH)
        for f in range(2):
            assert_same(on, f, off, f, state=(f, f))
        pc.assert_unchanged()  # the input is read where it lies, never written
    finally:
        pc.free()
        pp.free()
        on.close()
        off.close()


def test_single_frame_fields_call(clouds):
    """pwpp_estimate_ground_fields: one PointCloud2 blob, point_step 32, shuffled offsets, the handle's stream 0 -- twice."""
    from test_gpu_parity import pointcloud2_blob
    T, c, pre = clouds[0]
    on, off = make(), make()
    on.set_input_transforms(T)
    for rnd in range(2):
        on.estimate_ground_fields(pointcloud2_blob(c, 32, (4, 12, 20, 0), 7).ravel(), len(c), 32, 4, 12, 20, 0)
        off.estimate_ground_fields(pointcloud2_blob(pre, 32, (4, 12, 20, 0), 7).ravel(), len(c), 32, 4, 12, 20, 0)
        assert_same(on, 0, off, 0, state=(0, 0))
    on.close()
    off.close()


# ---- 3. the side paths, each with its counter ----------------------------------------------------------------------------------
def run_pair(cs, ps, Ts, params=None, order=pwpp_hip.ORDER_CLOUD, options=(), warm=None):
    on, off = make(params, order, options), make(params, order, options)
    on.set_input_transforms(Ts)
    if warm is not None:
        on.estimate_ground_batch(warm[0])
        off.estimate_ground_batch(warm[1])
    on.estimate_ground_batch(cs)
    off.estimate_ground_batch(ps)
    return on, off


def test_two_pass_binning(clouds):
    cs, ps = [c for _, c, _ in clouds], [p for _, _, p in clouds]
    on, off = run_pair(cs, ps, np.stack([t for t, _, _ in clouds]), options=[("one_pass", "0")])
    assert on.one_pass_stats() == (0, 0)
    for f in range(5):
        assert_same(on, f, off, f, state=(f, f))


def test_host_redo_after_segment_overflow(clouds):
    cs, ps = [c for _, c, _ in clouds], [p for _, _, p in clouds]
    on, off = run_pair(cs, ps, np.stack([t for t, _, _ in clouds]), options=[("one_pass_scale", 0.05)])
    assert on.redo_stats()[1] > 0 and on.redo_stats() == off.redo_stats()
    for f in range(5):
        assert_same(on, f, off, f, state=(f, f))


def test_parts_moved_into_the_overflow_arena(clouds, kitti):
    """24 frames size the segments; then one frame with 40 % more points in one sector: its parts move to the arena on the device."""
    T, c, pre = clouds[0]
    rng = np.random.default_rng(11)
    a = np.arctan2(pre[:, 1], pre[:, 0])
    sel = np.where((a > 0.3) & (a < 0.6))[0]
    extra = c[rng.choice(sel, int(len(sel) * 0.4), replace=True)].copy()
    extra[:, :3] += rng.normal(0.0, 0.004, (len(extra), 3)).astype(F32)
    dense = np.ascontiguousarray(np.concatenate([c, extra]).astype(F32))
    base_c, base_p = [c] * 24, [pre] * 24
    odd_c, odd_p = list(base_c), list(base_p)
    odd_c[7], odd_p[7] = dense, pre_transformed(T, dense)
    on, off = run_pair(odd_c, odd_p, T, warm=(base_c, base_p))
    assert on.arena_stats()[0] >= 1 and on.redo_stats() == (48, 0), (on.arena_stats(), on.redo_stats())
    assert on.arena_stats()[0] == off.arena_stats()[0]
    for f in (6, 7, 8, 23):
        assert_same(on, f, off, f, state=(f, f))


def test_serial_fix_up(clouds):
    p = apply_variant(pwpp_hip.default_params(), dict(num_lpr=0))
    cs, ps = [clouds[0][1], clouds[4][1]], [clouds[0][2], clouds[4][2]]
    on, off = run_pair(cs, ps, np.stack([clouds[0][0], clouds[4][0]]), params=p)
    assert on.fixed_up_frames() > 0 and on.fixed_up_frames() == off.fixed_up_frames()
    for f in range(2):
        assert_same(on, f, off, f, state=(f, f))


def test_reference_order(clouds):
    cs, ps = [clouds[1][1], clouds[4][1]], [clouds[1][2], clouds[4][2]]
    on, off = run_pair(cs, ps, np.stack([clouds[1][0], clouds[4][0]]), order=pwpp_hip.ORDER_REFERENCE)
    for f in range(2):
        assert_same(on, f, off, f, state=(f, f))
        z = ps[f][on.ground_indices(f), 2]
        assert len(z) > 1000 and not np.array_equal(np.sort(on.ground_indices(f)), on.ground_indices(f))  # not cloud order: the keys ran


@pytest.mark.parametrize("exact", [0, 1])
def test_both_sum_widths(clouds, exact):
    cs, ps = [clouds[2][1], clouds[3][1]], [clouds[2][2], clouds[3][2]]
    on, off = run_pair(cs, ps, np.stack([clouds[2][0], clouds[3][0]]), options=[("exact_moments", exact)])
    assert on.fxp_shift() == (30 if exact else 21)
    for f in range(2):
        assert_same(on, f, off, f, state=(f, f))


def test_ros_launch_parameters(clouds):
    p = apply_variant(pwpp_hip.default_params(), ROS_LAUNCH)
    cs = [np.ascontiguousarray(clouds[k][1][:, :3]) for k in (0, 4)]  # the node's N x 3 input
    ps = [np.ascontiguousarray(clouds[k][2][:, :3]) for k in (0, 4)]
    on, off = run_pair(cs, ps, np.stack([clouds[0][0], clouds[4][0]]), params=p)
    for f in range(2):
        assert_same(on, f, off, f, state=(f, f))


# ---- 4. streams ------------------------------------------------------------------------------------------------------------------
def test_three_streams_four_steps(clouds):
    on, off = make(), make()
    for h in (on, off):
        h.set_num_streams(3)
    on.set_input_transforms(np.stack([clouds[s][0] for s in (0, 1, 4)]))
    for step in range(4):
        cs, ps = [], []
        for s in (0, 1, 4):
            n = len(clouds[s][1]) - 997 * step  # a different cloud every step
            cs.append(clouds[s][1][:n])
            ps.append(clouds[s][2][:n])
        on.estimate_ground_batch(cs, mode=pwpp_hip.MODE_STREAMS)
        off.estimate_ground_batch(ps, mode=pwpp_hip.MODE_STREAMS)
        for f in range(3):
            assert_same(on, f, off, f, state=(f, f))
    assert on.state(0).sensor_height != pwpp_hip.default_params().sensor_height  # the streams did adapt
    on.close()
    off.close()


# ---- 5. records stay in the sensor frame; queries live in the transformed one ---------------------------------------------------
def test_records_verbatim_xyz_transformed_and_queries(clouds):
    T, c, pre = clouds[0]
    for records in (True, False):  # written behind the lists / gathered when the getter runs
        h = make(records=records)
        h.set_input_transforms(T)
        h.estimate_ground_batch([c])
        rows = c.view(np.uint8).reshape(len(c), 16)
        for rec, xyz, idx in ((h.ground_records(), h.ground(), h.ground_indices()), (h.nonground_records(), h.nonground(), h.nonground_indices())):
            assert np.array_equal(rec, rows[idx])                              # the input bytes, untransformed
            assert np.array_equal(bits(xyz), bits(np.ascontiguousarray(pre[idx, :3])))  # the transformed coordinates
        assert not np.array_equal(c[:, :3], pre[:, :3])
        pp, dist = h.point_patches(), h.point_distances()
        q = h.query_ground(pwpp_hip.transform_points(T, c[:, :3]))
        m = pp >= 0  # (a point RNR removed has patch -1; its position would query into its bin's patch)
        assert m.sum() > 50000
        assert np.array_equal(q["patch"][m], pp[m]) and np.array_equal(bits(q["distance"][m]), bits(dist[m]))
        # a later change of the setting does not reach the results of the call that ran
        h.set_input_transforms(clouds[1][0])
        assert np.array_equal(bits(h.ground()), bits(np.ascontiguousarray(pre[h.ground_indices(), :3])))
        h.close()


# ---- 6. a pipe -------------------------------------------------------------------------------------------------------------------
def test_depth_two_pipe(clouds):
    import torch
    T = clouds[3][0]
    pipe = pwpp_hip.Pipe(depth=2)
    pipe.set_input_transforms(T)
    off = make()
    for i in range(2):
        v = pipe.handle(i)
        v.set_order(pwpp_hip.ORDER_CLOUD)
        v.set_point_planes(True)
    dev = torch.device("cuda", 0)
    for rnd, ks in enumerate(([3, 0], [1, 3], [3])):
        cs = [clouds[3][1][: len(clouds[3][1]) - 100 * k] for k in ks]
        ps = [pre_transformed(T, c) for c in cs]
        ts = [torch.from_numpy(c).to(dev) for c in cs]
        torch.cuda.synchronize()
        v = pipe.submit_device_batch(pipe.handle(0).make_device_batch([t.data_ptr() for t in ts], [len(c) for c in cs]))
        v.synchronize()
        off.estimate_ground_batch(ps)
        for f in range(len(cs)):
            assert_same(v, f, off, f, state=(f, f))
    pipe.close()
    off.close()


# ---- 7. errors -------------------------------------------------------------------------------------------------------------------
def test_errors(clouds):
    T, c, pre = clouds[0]
    h = make()
    h.set_input_transforms(T)
    h.estimate_ground_batch([c])
    before = (h.counts(0), h.ground_indices().copy(), h.ground().copy())
    h.set_input_transforms(np.stack([T, T, T]))
    with pytest.raises(pwpp_hip.PwppError, match="pwpp error -1"):
        h.estimate_ground_batch([c])  # three transforms, one frame
    assert h.counts(0) == before[0] and np.array_equal(h.ground_indices(), before[1]) and np.array_equal(bits(h.ground()), bits(before[2]))
    h.estimate_ground_batch([c, c[:1000], c[:10]])  # three frames: fine
    bad = T.copy()
    bad[1, 2] = np.nan
    with pytest.raises(pwpp_hip.PwppError, match="pwpp error -1"):
        h.set_input_transforms(bad)
    bad[1, 2] = np.inf
    with pytest.raises(pwpp_hip.PwppError, match="pwpp error -1"):
        h.set_input_transforms(bad)
    t12 = np.ascontiguousarray(T.reshape(12))
    assert h._L.pwpp_set_input_transforms(h._h, t12.ctypes.data_as(ctypes.c_void_p), -1) == -1
    assert h._L.pwpp_set_input_transforms(h._h, t12.ctypes.data_as(ctypes.c_void_p), 65536) == -1
    h.estimate_ground_batch([c, c[:1000], c[:10]])  # the rejected calls changed nothing: still three transforms
    assert h._L.pwpp_set_input_transforms(h._h, None, 3) == 0  # a null T turns it off whatever the count
    h.estimate_ground_batch([c])
    h.close()
