"""The records of the ground / non-ground points (pwpp_set_point_records, pwpp_get_*_records) on a real MI355X.

Every expected value is exact: the bytes of the input at the handle's own indices -- `blob.reshape(n, point_step)[idx]` for a
fields layout, the rows of the (n, cols) matrix for a matrix -- and the index sets are the oracle's.  Row sizes from 12 to 260
bytes take every path of the gather kernel (one lane per row, 16-byte pieces, the dword stream: csrc/pwpp_kernels.hip); the
frames are small except one KITTI frame per layout."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as ol
import pwpp_hip
import pwpp_synth
from test_gpu_inputs import LAYOUTS, Placed, encode, expected_array, submit
from test_gpu_labels import expected_labels, hip_copy
from test_gpu_parity import ROS_LAUNCH, apply_variant, assert_frame_equal, pointcloud2_blob, to_oracle_params

pytestmark = pytest.mark.gpu

# fields layouts beyond tests/test_gpu_inputs.LAYOUTS: 5 dwords, 18 dwords, and 65 dwords -- a record wider than a wave has lanes
WIDE = {
    "fields20": ("fields", 20, (4, 8, 16, 0)),
    "fields72": ("fields", 72, (40, 4, 60, 12)),
    "fields260": ("fields", 260, (0, 128, 256, 64)),
}
ALL = dict(LAYOUTS, **WIDE)
MEMS = ["host", "pinned_slab", "device"]


@pytest.fixture(scope="module")
def oracle(oracle_built):
    return oracle_built.restatement()


@pytest.fixture(scope="module")
def frames(kitti):
    syn = pwpp_synth.add_edge_cases(pwpp_synth.make_cloud(23, beams=16, azimuth_steps=300), 23)
    assert (syn[:, 2] == np.finfo(np.float32).tiny).any()  # the reference's skip marker: the lists are shorter than n
    return {"empty": np.zeros((0, 4), np.float32), "one": kitti[4][7:8].copy(), "ten": kitti[2][1000:1010].copy(),
            "odd": kitti[1][20000:24133].copy(),  # 4133 points: neither a multiple of 4 nor of 64
            "syn": syn, "kitti": kitti[3]}


def small_frames(count, seed=0):
    """`count` synthetic frames of varied length (a few thousand points each)."""
    out = []
    for k in range(count):
        c = pwpp_synth.make_cloud(seed + k % 7, beams=16, azimuth_steps=300)
        out.append(np.ascontiguousarray(c[(k * 37) % 301: c.shape[0] - (k * 53) % 997]))
    return out


def cols_of(layout):
    kind, a, b = ALL[layout]
    return a if kind == "matrix" else (4 if b[3] >= 0 else 3)


def record_bytes_of(layout):
    kind, a, _ = ALL[layout]
    return 4 * a if kind == "matrix" else a


def encode_any(exp, layout, salt):
    if layout in LAYOUTS:
        return encode(exp, layout, salt)
    _, step, off = ALL[layout]
    return pointcloud2_blob(exp, step, off, salt).ravel()


def submit_any(h, placed, layout, ns, mode=pwpp_hip.MODE_FRESH):
    if layout in LAYOUTS:
        return submit(h, placed, layout, ns, mode)
    _, step, off = ALL[layout]
    h.estimate_ground_fields_batch(placed.data(), ns, step, *off, mem=placed.mem_kind, mode=mode)
    if placed.mem_kind != pwpp_hip.MEM_HOST:
        h.synchronize()


def rows_of(exp, blob, layout):
    """(n, record_bytes) uint8: what a record of every point of the frame must be."""
    kind, a, _ = ALL[layout]
    if kind == "matrix":  # the matrix row, also for a column-major matrix (gathered from its planes)
        return np.ascontiguousarray(exp).view(np.uint8).reshape(len(exp), 4 * a)
    return blob.reshape(len(exp), a)


def check_records(h, frame, src, rb):
    """Both lists' rows = the input's records at the handle's own indices of the same call."""
    assert h.record_bytes == rb
    for rows, idx in ((h.ground_records(frame), h.ground_indices(frame)), (h.nonground_records(frame), h.nonground_indices(frame))):
        assert rows.dtype == np.uint8 and rows.shape == (len(idx), rb)
        assert np.array_equal(rows, src[idx]), "records differ from the input's bytes at the handle's indices"


_refs = {}


def ref_of(oracle, exp, key):
    if key not in _refs:
        _refs[key] = ol.Estimator(oracle, arith=ol.ARITH_FXP).run(exp) if len(exp) else None
    return _refs[key]


def matrix_src(c):
    return np.ascontiguousarray(c).view(np.uint8).reshape(c.shape[0], 4 * c.shape[1])


# ---- 1. widths and layouts ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("layout", list(ALL))
def test_widths_layouts_and_memory_kinds(frames, oracle, layout, mem):
    names = ["empty", "one", "ten", "odd", "syn", "kitti"]
    exps = [expected_array(frames[n], layout) if layout in LAYOUTS else np.ascontiguousarray(frames[n][:, :cols_of(layout)]) for n in names]
    blobs = [encode_any(e, layout, 11 + k) for k, e in enumerate(exps)]
    rb = record_bytes_of(layout)
    h = pwpp_hip.Handle()
    h.set_point_records(True)
    placed = Placed(blobs, mem)
    try:
        submit_any(h, placed, layout, [len(e) for e in exps])
        for k, (name, e) in enumerate(zip(names, exps)):
            ref = ref_of(oracle, e, (name, cols_of(layout)))
            if ref is None:
                assert h.counts(k) == (0, 0, 0) and h.ground_records(k).shape == (0, rb) and h.nonground_records(k).shape == (0, rb)
                continue
            assert_frame_equal(h, k, ref, len(e))
            check_records(h, k, rows_of(e, blobs[k], layout), rb)
        assert h.all_counts()[names.index("syn"), 5] > 0
        placed.assert_unchanged()
    finally:
        placed.free()
        h.close()


@pytest.mark.parametrize("layout", ["fields16", "fields48", "row3", "fields260"])
def test_device_input_that_is_only_4_byte_aligned(frames, layout):
    """A device blob at an address that is a multiple of 4 and no more: the 16-byte paths must not be taken."""
    import torch
    exp = np.ascontiguousarray(frames["odd"][:, :cols_of(layout)])
    blob = encode_any(exp, layout, 5)
    t = torch.zeros(len(blob) + 64, dtype=torch.uint8, device="cuda:0")
    t[4:4 + len(blob)] = torch.from_numpy(blob).to("cuda:0")
    torch.cuda.synchronize()
    assert (t.data_ptr() + 4) % 16 == 4
    for on in (True, False):
        h = pwpp_hip.Handle()
        h.set_point_records(on)
        kind, a, b = ALL[layout]
        if kind == "matrix":
            h.submit_batch([t.data_ptr() + 4], [len(exp)], a, b, pwpp_hip.MEM_DEVICE, pwpp_hip.MODE_FRESH)
        else:
            h.estimate_ground_fields_batch([t.data_ptr() + 4], [len(exp)], a, *b, mem=pwpp_hip.MEM_DEVICE, mode=pwpp_hip.MODE_FRESH)
        h.synchronize()
        check_records(h, 0, rows_of(exp, blob, layout), record_bytes_of(layout))
        h.close()


# ---- 2. the batch buffer -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["row3", "row4", "fields72"])
def test_batch_buffer_and_device_pointer(frames, layout):
    names = ["odd", "empty", "syn", "one", "ten", "odd"]
    exps = [np.ascontiguousarray(frames[n][:, :cols_of(layout)]) for n in names]
    blobs = [encode_any(e, layout, 3 + k) for k, e in enumerate(exps)]
    rb = record_bytes_of(layout)
    h = pwpp_hip.Handle()
    h.set_point_records(True)
    placed = Placed(blobs, "host")
    submit_any(h, placed, layout, [len(e) for e in exps])
    rec, base, counts = h.all_records()
    total = sum(len(e) for e in exps)
    assert rec.dtype == np.uint8 and rec.shape == (total, rb) and int(base[-1]) == total
    assert np.array_equal(base, h.frame_base()) and np.array_equal(counts, h.all_counts())
    ptr, drb = h.device_records()
    assert ptr != 0 and drb == rb
    if rb % 16 == 0:
        assert ptr % 16 == 0
    raw = hip_copy(ptr, total * rb).reshape(total, rb)
    for k, e in enumerate(exps):
        g, ng = h.ground_records(k), h.nonground_records(k)
        assert (len(g), len(ng)) == (counts[k, 0], counts[k, 1])
        for buf in (rec, raw):
            seg = buf[base[k]:base[k + 1]]
            assert np.array_equal(seg[:len(g)], g) and np.array_equal(seg[len(g):len(g) + len(ng)], ng)
        check_records(h, k, rows_of(e, blobs[k], layout), rb)
    out = np.zeros(total * rb + 7, np.uint8)
    rec2, _, _ = h.all_records(out)
    written = np.concatenate([np.arange(base[k], base[k] + counts[k, 0] + counts[k, 1]) for k in range(len(exps))])
    assert np.array_equal(rec2[written], rec[written]) and not out[total * rb:].any()
    placed.free()
    h.close()


# ---- 3. on demand against in-pipeline ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", list(ALL))
def test_on_demand_rows_equal_the_pipeline_rows(frames, layout):
    """Setting off: the getters gather when they are called.  Each call's rows are compared with the indices of that same call (in
    the default order the lists' order differs from call to call).  records_path 1 / 2 -- one lane per row, no 16-byte pieces -- are
    other ways to the same bytes, in the pipeline and on demand."""
    names = ["ten", "odd", "syn"]
    exps = [np.ascontiguousarray(frames[n][:, :cols_of(layout)]) for n in names]
    blobs = [encode_any(e, layout, 21 + k) for k, e in enumerate(exps)]
    rb = record_bytes_of(layout)
    for on in (False, True):
        for path in (0, 1, 2):
            h = pwpp_hip.Handle()
            h.set_point_records(on)
            h.set_option("records_path", path)
            placed = Placed(blobs, "host")
            submit_any(h, placed, layout, [len(e) for e in exps])
            for k, e in enumerate(exps):
                check_records(h, k, rows_of(e, blobs[k], layout), rb)
            if not on:
                with pytest.raises(pwpp_hip.PwppError, match="without point records"):
                    h.all_records()
            placed.free()
            h.close()
    with pytest.raises(pwpp_hip.PwppError):
        pwpp_hip.Handle().set_option("records_path", 3)


# ---- 4. every path that writes lists -----------------------------------------------------------------------------------------
def check_batch(h, clouds, refs=None, which=None):
    for i in (range(len(clouds)) if which is None else which):
        check_records(h, i, matrix_src(clouds[i]), 4 * clouds[i].shape[1])
        if refs is not None:
            assert_frame_equal(h, i, refs[i], clouds[i].shape[0])


def written_rows(h):
    rec, base, counts = h.all_records()
    return b"".join(rec[base[k]:base[k] + counts[k, 0] + counts[k, 1]].tobytes() for k in range(len(base) - 1))


def test_overlap_and_single_stream_schedules(oracle):
    clouds = small_frames(132)
    assert len({c.shape[0] for c in clouds}) > 100
    probe = (0, 1, 63, 64, 65, 66, 67, 127, 128, 131)
    refs = {i: ol.Estimator(oracle, arith=ol.ARITH_FXP).run(clouds[i]) for i in probe}
    for overlap in (True, False):
        h = pwpp_hip.Handle()
        h.set_point_records(True)
        h.set_overlap(overlap)
        h.estimate_ground_batch(clouds, mode=pwpp_hip.MODE_FRESH)
        check_batch(h, clouds)
        for i in probe:
            assert_frame_equal(h, i, refs[i], clouds[i].shape[0])
        h.close()
    # cloud order on the overlap schedule: two runs give byte-identical buffers over the written rows
    h = pwpp_hip.Handle()
    h.set_point_records(True)
    h.set_order(pwpp_hip.ORDER_CLOUD)
    h.estimate_ground_batch(clouds, mode=pwpp_hip.MODE_FRESH)
    first = written_rows(h)
    check_batch(h, clouds, which=probe)
    h.estimate_ground_batch(clouds, mode=pwpp_hip.MODE_FRESH)
    assert written_rows(h) == first
    h.close()


def test_redo_fixup_streams_orders_and_profiling(kitti, oracle):
    est = lambda p, op=None: ol.Estimator(oracle, op, arith=ol.ARITH_FXP).run(p)
    clouds = small_frames(6, seed=3)
    refs = [est(c) for c in clouds]

    def handle(params=None, **opts):
        h = pwpp_hip.Handle(params)
        h.set_point_records(True)
        for k, v in opts.items():
            h.set_option(k, v)
        return h

    # two-pass binning; a redo after a forced segment overflow (in place, and of the whole batch)
    h = handle(one_pass=0)
    h.estimate_ground_batch(clouds, mode=pwpp_hip.MODE_FRESH)
    check_batch(h, clouds, refs)
    for opts in (dict(one_pass_scale=0.02), dict(one_pass_scale=0.02, redo_whole_batch=1)):
        h = handle(**opts)
        h.estimate_ground_batch(clouds, mode=pwpp_hip.MODE_FRESH)
        assert h.redo_stats()[1] > 0, "the overflow redo did not run"
        check_batch(h, clouds, refs)
        h.close()
    # the serial fix-up of frames whose patches start from the plane fitted before them (k_fit_fixup)
    frng = np.random.default_rng(5)

    def spoil(c, k):
        c = c.copy()
        c[frng.choice(c.shape[0], k, replace=False), 2] = -np.inf
        lone = np.array([[70.0, 30.0 + i, 1e30, 0.5] for i in range(3)] + [[3.5, -1.0, 3e38, 0.5]], np.float32)
        return np.ascontiguousarray(np.concatenate([c, lone]))

    spoiled = [spoil(kitti[0], 40), clouds[1], spoil(clouds[2], 3)]
    h = handle()
    h.estimate_ground_batch(spoiled, mode=pwpp_hip.MODE_FRESH)
    assert h.fixed_up_frames() >= 1
    check_batch(h, spoiled, [est(c) for c in spoiled])
    h.close()
    # stateful streams in lock step
    h = handle()
    h.set_num_streams(3)
    ests = [ol.Estimator(oracle, arith=ol.ARITH_FXP) for _ in range(3)]
    for t in range(3):
        fr = [clouds[(s + t) % 6] for s in range(3)]
        h.estimate_ground_batch(fr, mode=pwpp_hip.MODE_STREAMS)
        check_batch(h, fr, [ests[s].run(fr[s]) for s in range(3)])
    h.close()
    # reference order, cloud order (byte-identical from run to run), profiling
    for order in (pwpp_hip.ORDER_REFERENCE, pwpp_hip.ORDER_CLOUD):
        h = handle()
        h.set_order(order)
        h.estimate_ground_batch(clouds, mode=pwpp_hip.MODE_FRESH)
        check_batch(h, clouds, refs)
        if order == pwpp_hip.ORDER_CLOUD:
            first = written_rows(h)
            for k, c in enumerate(clouds):
                assert np.array_equal(h.ground_records(k), matrix_src(c)[np.sort(refs[k].ground_idx)])
            h.estimate_ground_batch(clouds, mode=pwpp_hip.MODE_FRESH)
            assert written_rows(h) == first
        h.close()
    h = handle()
    h.set_profiling(True)
    h.estimate_ground_batch(clouds, mode=pwpp_hip.MODE_FRESH)
    check_batch(h, clouds, refs)
    prof = h.kernel_profile()
    assert pwpp_hip.NUM_KERNELS == 11 and prof["k_emit"][1] == 1 and prof["k_emit"][0] > 0
    h.close()


def test_pipe_handles_take_the_setting(oracle):
    import torch
    clouds = small_frames(5, seed=2)
    refs = [ol.Estimator(oracle, arith=ol.ARITH_FXP).run(c) for c in clouds]
    tens = [torch.from_numpy(c).to("cuda:0") for c in clouds]
    torch.cuda.synchronize()
    ptrs = (ctypes.c_void_p * 5)(*[t.data_ptr() for t in tens])
    ns = (ctypes.c_int32 * 5)(*[c.shape[0] for c in clouds])
    pipe = pwpp_hip.Pipe(depth=2)
    try:
        for i in range(2):
            pipe.handle(i).set_point_records(True)
        held = []
        for rep in range(4):
            hv = pipe.submit_device_batch((ptrs, ns, 5))
            held.append(hv)
            if rep >= 1:  # the batch before this one: its handle has not come round again
                prev = held[rep - 1]
                prev.synchronize()
                check_batch(prev, clouds, refs)
                assert prev.device_records()[1] == 16
        pipe.drain()
        check_batch(held[-1], clouds, refs)
    finally:
        pipe.close()


# ---- 5. state and errors -----------------------------------------------------------------------------------------------------
def test_state_errors_trim_and_workspace(frames):
    clouds = [frames["odd"], frames["syn"]]
    h = pwpp_hip.Handle()
    for get in (lambda: h.all_records(), lambda: h.device_records(), lambda: h.record_bytes, lambda: h.ground_records(0)):
        with pytest.raises(pwpp_hip.PwppError, match="error -4"):  # PWPP_E_STATE: no call yet
            get()
    h.estimate_ground_batch(clouds, mode=pwpp_hip.MODE_FRESH)
    for get in (lambda: h.all_records(), lambda: h.device_records()):
        with pytest.raises(pwpp_hip.PwppError, match="without point records"):
            get()
    assert h.record_bytes == 16
    check_batch(h, clouds)  # (on demand)
    h.set_point_records(True)
    h.estimate_ground_batch(clouds, mode=pwpp_hip.MODE_FRESH)
    check_batch(h, clouds)
    for bad in (-1, 2):
        for get in (h.ground_records, h.nonground_records):
            with pytest.raises(pwpp_hip.PwppError, match="out of range"):
                get(bad)
    h.trim_workspace()
    for get in (lambda: h.ground_records(0), lambda: h.all_records(), lambda: h.device_records()):
        with pytest.raises(pwpp_hip.PwppError):
            get()
    h.estimate_ground_batch(clouds, mode=pwpp_hip.MODE_FRESH)
    check_batch(h, clouds)
    assert h.all_records()[0].shape == (sum(c.shape[0] for c in clouds), 16)
    h.close()
    # nothing is allocated while the setting is off
    a, b, c = pwpp_hip.Handle(), pwpp_hip.Handle(), pwpp_hip.Handle()
    b.set_point_records(True)
    b.set_point_records(False)
    c.set_point_records(True)
    for x in (a, b, c):
        x.estimate_ground_batch(clouds, mode=pwpp_hip.MODE_FRESH)
    assert a.workspace_bytes() == b.workspace_bytes()
    assert c.workspace_bytes() >= a.workspace_bytes() + 16 * sum(len(x) for x in clouds)
    for x in (a, b):
        x.ground_records(0)  # (on demand: the getters' gather scratch, the same for both)
    assert a.workspace_bytes() == b.workspace_bytes()
    c.trim_workspace()
    assert c.workspace_bytes() < a.workspace_bytes()
    for x in (a, b, c):
        x.close()


@pytest.mark.parametrize("layout", ["row4", "fields48", "col3"])
def test_device_input_may_be_overwritten_once_the_records_are_written(frames, layout):
    exps = [np.ascontiguousarray(frames[n][:, :cols_of(layout)]) for n in ("odd", "syn")]
    blobs = [encode_any(e, layout, 9 + k) for k, e in enumerate(exps)]
    h = pwpp_hip.Handle()
    h.set_point_records(True)
    placed = Placed(blobs, "device")
    try:
        submit_any(h, placed, layout, [len(e) for e in exps])
        import torch
        for t in placed._dev:
            t.fill_(0x5A)
        torch.cuda.synchronize()
        for k, e in enumerate(exps):
            check_records(h, k, rows_of(e, blobs[k], layout), record_bytes_of(layout))
    finally:
        placed.free()
        h.close()


# ---- 6. labels, point planes and records in one call -------------------------------------------------------------------------
@pytest.mark.parametrize("order", [pwpp_hip.ORDER_SCATTER, pwpp_hip.ORDER_CLOUD])
def test_labels_point_planes_and_records_together(oracle, order):
    clouds = small_frames(4, seed=5)
    refs = [ol.Estimator(oracle, arith=ol.ARITH_FXP).run(c) for c in clouds]
    alone = pwpp_hip.Handle()  # point planes are a function of the input alone: a handle with nothing else is the yardstick
    alone.set_point_planes(True)
    alone.estimate_ground_batch(clouds, mode=pwpp_hip.MODE_FRESH)
    h = pwpp_hip.Handle()
    h.set_labels(True)
    h.set_point_planes(True)
    h.set_point_records(True)
    h.set_order(order)
    h.estimate_ground_batch(clouds, mode=pwpp_hip.MODE_FRESH)
    check_batch(h, clouds, refs)
    for k, c in enumerate(clouds):
        assert np.array_equal(h.labels(k), expected_labels(c.shape[0], refs[k].ground_idx, refs[k].nonground_idx))
        assert np.array_equal(h.point_patches(k), alone.point_patches(k))
        assert np.array_equal(h.point_distances(k).view(np.uint32), alone.point_distances(k).view(np.uint32))
    h.close()
    alone.close()


def tiny_frames():
    """Three synthetic frames: a few hundred points, an empty one and a single point."""
    c = pwpp_synth.make_cloud(31, beams=8, azimuth_steps=60)
    assert 200 < c.shape[0] < 1000
    return [np.ascontiguousarray(c), np.zeros((0, 4), np.float32), np.ascontiguousarray(c[17:18])]


def all_outputs(h):
    """Everything the last call wrote, as bytes: lists, labels, point planes and records of the whole batch."""
    idx, base, counts = h.all_indices()
    lists = b"".join(idx[base[k]:base[k] + counts[k, 0] + counts[k, 1]].tobytes() for k in range(len(base) - 1))
    return (lists, counts[:, :3].tobytes(), h.all_labels()[0].tobytes(), h.all_point_patches()[0].tobytes(),
            h.all_point_distances()[0].tobytes(), written_rows(h))


def test_trim_leaves_the_same_bytes_with_and_without_outputs():
    clouds = tiny_frames()
    points = sum(c.shape[0] for c in clouds)
    on, off = pwpp_hip.Handle(), pwpp_hip.Handle()
    on.set_labels(True)
    on.set_point_planes(True)
    on.set_point_records(True)
    for h, last_order in ((on, pwpp_hip.ORDER_CLOUD), (off, pwpp_hip.ORDER_SCATTER)):
        h.set_num_streams(3)
        h.estimate_ground_batch(clouds, mode=pwpp_hip.MODE_FRESH)
        h.estimate_ground_batch(clouds, mode=pwpp_hip.MODE_STREAMS)
        h.set_order(pwpp_hip.ORDER_REFERENCE)
        h.estimate_ground_batch(clouds, mode=pwpp_hip.MODE_FRESH)
        h.set_order(last_order)  # (cloud order implies labels; the handle without outputs runs a plain call instead)
        h.estimate_ground_batch(clouds, mode=pwpp_hip.MODE_FRESH)
    assert on.record_bytes == 16
    assert on.workspace_bytes() >= off.workspace_bytes() + (1 + 4 + 4 + on.record_bytes) * points
    before = all_outputs(on)
    on.trim_workspace()
    off.trim_workspace()
    assert on.workspace_bytes() == off.workspace_bytes()
    on.estimate_ground_batch(clouds, mode=pwpp_hip.MODE_FRESH)
    assert all_outputs(on) == before
    on.close()
    off.close()


def test_frame_getters_equal_the_batch_getters():
    clouds = tiny_frames()
    h = pwpp_hip.Handle()
    h.set_labels(True)
    h.set_point_planes(True)
    h.set_point_records(True)
    h.estimate_ground_batch(clouds, mode=pwpp_hip.MODE_FRESH)
    base = h.frame_base()
    assert list(np.diff(base)) == [c.shape[0] for c in clouds]
    labels, patches, dists = h.all_labels()[0], h.all_point_patches()[0], h.all_point_distances()[0]
    rec, rbase, counts = h.all_records()
    assert np.array_equal(rbase, base)
    for k in range(len(clouds)):
        span = slice(int(base[k]), int(base[k + 1]))
        assert np.array_equal(h.labels(k), labels[span])
        assert np.array_equal(h.point_patches(k), patches[span])
        assert np.array_equal(h.point_distances(k).view(np.uint32), dists[span].view(np.uint32))
        rows = np.concatenate([h.ground_records(k), h.nonground_records(k)])
        assert np.array_equal(rows, rec[base[k]:base[k] + counts[k, 0] + counts[k, 1]])
    # a call with an output off: its getters, per frame and for the batch, say which one is missing
    for off, text, getters in (
            (h.set_labels, "without labels", (lambda: h.labels(0), lambda: h.labels(1), h.all_labels, h.device_labels)),
            (h.set_point_planes, "without point planes", (lambda: h.point_patches(0), lambda: h.point_distances(1), h.all_point_patches,
                                                          h.all_point_distances, h.device_point_planes)),
            (h.set_point_records, "without point records", (h.all_records, h.device_records))):
        off(False)
        h.estimate_ground_batch(clouds, mode=pwpp_hip.MODE_FRESH)
        for get in getters:
            with pytest.raises(pwpp_hip.PwppError, match=text):
                get()
    h.close()


# ---- 7. class and ROS core ---------------------------------------------------------------------------------------------------
def test_pybind_ground_points_keep_the_intensity(kitti):
    import pypatchworkpp
    pts = kitti[2]
    for on in (False, True):
        pp = pypatchworkpp.patchworkpp(pypatchworkpp.Parameters())
        pp.setPointRecords(on)
        pp.estimateGround(pts)
        g, ng = pp.getGroundPoints(), pp.getNongroundPoints()
        assert g.dtype == np.float32 and g.shape == (len(pp.getGroundIndices()), 4) and ng.shape == (len(pp.getNongroundIndices()), 4)
        assert np.array_equal(g.view(np.uint32), pts[pp.getGroundIndices()].view(np.uint32))
        assert np.array_equal(ng.view(np.uint32), pts[pp.getNongroundIndices()].view(np.uint32))
        assert np.array_equal(g[:, :3], pp.getGround())


def test_ros_core_keeps_the_fields(kitti, oracle, tmp_path):
    """examples/ros_core_demo --keep-fields: ground / non-ground are the multisets of the message's own 32-byte records at the
    oracle's index sets, with the message's fields and point_step; the cloud stays x, y, z.  Without the flag: x, y, z payloads."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "patchwork-plusplus_amd", "examples", "ros_core_demo")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.join(root, "patchwork-plusplus_amd"), "examples/ros_core_demo"], check=True)
    paths = []
    for k in range(2):
        p = tmp_path / ("%06d.bin" % k)
        kitti[k].tofile(p)
        paths.append(str(p))

    def run(*flags):
        out = subprocess.run([exe, *flags] + paths, capture_output=True, text=True, check=True).stdout
        lines = [json.loads(l) for l in out.splitlines() if l.startswith("{")]
        assert len(lines) == 2, out
        return lines

    def point_sum(rows):  # the sum of the records' FNV-1a: a list as a multiset
        a = np.ascontiguousarray(rows).astype(np.uint64)
        h = np.full(a.shape[0], 1469598103934665603, np.uint64)
        with np.errstate(over="ignore"):
            for j in range(a.shape[1]):
                h = (h ^ a[:, j]) * np.uint64(1099511628211)
            return "%016x" % int(h.sum(dtype=np.uint64))

    def message(pts):  # the demo's 32-byte records: intensity, x, ring, y, z, time between bytes of 0xA5
        n = pts.shape[0]
        blob = np.full((n, 32), 0xA5, np.uint8)
        f = pts.view(np.uint8).reshape(n, 4, 4)
        blob[:, 0:4], blob[:, 4:8], blob[:, 12:16], blob[:, 20:24] = f[:, 3], f[:, 0], f[:, 1], f[:, 2]
        blob[:, 8:10] = (np.arange(n) % 64).astype(np.uint16).view(np.uint8).reshape(n, 2)
        blob[:, 24:32] = (1e-6 * np.arange(n, dtype=np.float64)).view(np.uint8).reshape(n, 8)
        return blob

    def xyz_payload(xyz):  # CreatePointCloud2Msg: point_step 16
        a = np.zeros((xyz.shape[0], 4), np.float32)
        a[:, :3] = xyz
        return a.view(np.uint8).reshape(-1, 16)

    fields = ["intensity:0:7:1", "x:4:7:1", "ring:8:4:1", "y:12:7:1", "z:20:7:1", "time:24:8:1"]
    prm = apply_variant(pwpp_hip.default_params(), ROS_LAUNCH)
    kept, plain = run("--keep-fields"), run()
    est = ol.Estimator(oracle, to_oracle_params(prm), arith=ol.ARITH_FXP)
    for k in range(2):
        c3 = np.ascontiguousarray(kitti[k][:, :3])
        ref = est.run(c3)
        g, ng = np.asarray(ref.ground_idx), np.asarray(ref.nonground_idx)
        msg = message(kitti[k])
        assert kept[k]["ground"] == [len(g), 32, point_sum(msg[g])]
        assert kept[k]["nonground"] == [len(ng), 32, point_sum(msg[ng])]
        assert kept[k]["ground_fields"] == fields and kept[k]["nonground_fields"] == fields
        assert kept[k]["cloud"] == plain[k]["cloud"] and plain[k]["cloud"][:2] == [c3.shape[0], 16]
        assert plain[k]["ground"] == [len(g), 16, point_sum(xyz_payload(c3[g]))]
        assert plain[k]["nonground"] == [len(ng), 16, point_sum(xyz_payload(c3[ng]))]
        assert "ground_fields" not in plain[k]
