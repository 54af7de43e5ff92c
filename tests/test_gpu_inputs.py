"""Every input layout and memory kind of include/pwpp.h against the oracle (oracle/pwpp_oracle.cpp, fixed-point flavour).

A frame reaches the kernels in one of eight layouts -- row-major and column-major matrices of 3 or 4 columns, PointCloud2 blobs
with the float32 fields at byte offsets of a record (packed, padded and shuffled, without intensity, 12-byte records) -- from
pageable host memory, from page-locked memory (one slab or one allocation per frame) or from the caller's device memory.  The
binning kernels, the height fetch of k_emit (reference order) and the xyz getters' gather all read the caller's layout through
load_point (csrc/pwpp_common.hpp); on the device path they read the caller's own buffer.  Each case is compared with the oracle
run on the equivalent contiguous float32 (n, 3 | 4) array: index sets, patch records, planes, state and histories bit for bit,
getGround()/getNonground() rows bitwise equal to the input rows, and the input buffers unchanged.
"""
import numpy as np
import pytest

import oracle_lib as ol
import pwpp_hip
import pwpp_synth
from test_gpu_parity import assert_frame_equal, pointcloud2_blob, reference_consensus, to_oracle_params
from test_ref_fidelity import boundary_case

pytestmark = pytest.mark.gpu

# name: ("matrix", cols, layout) or ("fields", point_step, (off_x, off_y, off_z, off_intensity))
LAYOUTS = {
    "row4": ("matrix", 4, pwpp_hip.LAYOUT_ROW_MAJOR),
    "row3": ("matrix", 3, pwpp_hip.LAYOUT_ROW_MAJOR),
    "col4": ("matrix", 4, pwpp_hip.LAYOUT_COL_MAJOR),
    "col3": ("matrix", 3, pwpp_hip.LAYOUT_COL_MAJOR),
    "fields16": ("fields", 16, (0, 4, 8, 12)),           # packed
    "fields48": ("fields", 48, (8, 0, 16, 4)),           # padded and shuffled: unused bytes between and after the fields
    "fields_noi": ("fields", 24, (16, 8, 0, -1)),        # no intensity field: RNR is skipped
    "fields12": ("fields", 12, (0, 4, 8, -1)),           # x, y, z and nothing else
}
MEMS = ["host", "pinned_slab", "pinned_scattered", "device"]
PATHS = ["fresh1", "fresh6", "fresh6_two_pass", "redo", "streams"]


def cols_of(layout):
    kind, a, b = LAYOUTS[layout]
    return a if kind == "matrix" else (4 if b[3] >= 0 else 3)


def expected_array(pts, layout):
    """The contiguous float32 (n, 3 | 4) matrix the layout encodes (3 columns when there is no intensity)."""
    return np.ascontiguousarray(pts[:, :cols_of(layout)], np.float32)


def encode(exp, layout, salt):
    """The bytes of one frame in `layout` (uint8, 1-D)."""
    kind, a, b = LAYOUTS[layout]
    if kind == "matrix":
        m = exp if b == pwpp_hip.LAYOUT_ROW_MAJOR else np.ascontiguousarray(exp.T)  # column-major = the transpose, C-order
        return np.ascontiguousarray(m, np.float32).view(np.uint8).ravel().copy()
    return pointcloud2_blob(exp, a, b, salt).ravel()


class Placed:
    """A batch of encoded frames placed in one memory kind (the host copies, pinned views or device tensors are kept alive here)."""

    def __init__(self, blobs, mem):
        self.mem, self.blobs, self._pinned, self._dev = mem, blobs, [], []
        if mem == "host":
            self.views = [b.copy() for b in blobs]
        elif mem == "pinned_slab":  # frames back to back in one page-locked slab
            slab = pwpp_hip.pinned_empty((max(sum(len(b) for b in blobs), 1),), np.uint8)
            self._pinned.append(slab)
            self.views, at = [], 0
            for b in blobs:
                slab[at:at + len(b)] = b
                self.views.append(slab[at:at + len(b)])
                at += len(b)
        elif mem == "pinned_scattered":  # one page-locked allocation per frame
            self.views = []
            for b in blobs:
                a = pwpp_hip.pinned_empty((max(len(b), 1),), np.uint8)
                a[:len(b)] = b
                self._pinned.append(a)
                self.views.append(a[:len(b)])
        else:
            import torch
            dev = torch.device("cuda", 0)
            self._dev = [torch.from_numpy(b.copy()).to(dev) for b in blobs]  # uint8 tensors on cuda:0
            torch.cuda.synchronize()
            self.views = None

    @property
    def mem_kind(self):
        return {"host": pwpp_hip.MEM_HOST, "device": pwpp_hip.MEM_DEVICE}.get(self.mem, pwpp_hip.MEM_HOST_PINNED)

    def addresses(self):
        if self.mem == "device":
            return [t.data_ptr() if t.numel() else 0 for t in self._dev]
        return [v.ctypes.data for v in self.views]

    def data(self):
        return [t.data_ptr() if t.numel() else 0 for t in self._dev] if self.mem == "device" else self.views

    def assert_unchanged(self):
        for k, b in enumerate(self.blobs):
            now = self._dev[k].cpu().numpy() if self.mem == "device" else self.views[k]
            assert np.array_equal(now, b), "input buffer of frame %d changed" % k

    def free(self):
        for a in self._pinned:
            pwpp_hip.pinned_free(a)
        self._pinned, self._dev = [], []


def submit(h, placed, layout, ns, mode):
    kind, a, b = LAYOUTS[layout]
    if kind == "matrix":
        h.submit_batch(placed.addresses(), ns, a, b, placed.mem_kind, mode)
    else:
        h.estimate_ground_fields_batch(placed.data(), ns, a, *b, mem=placed.mem_kind, mode=mode)
    if placed.mem_kind != pwpp_hip.MEM_HOST:
        h.synchronize()


def assert_rows_bitwise(h, frame, exp):
    """getGround()/getNonground(): the input rows at the returned indices, bit for bit (NaN payloads and -0.0 included)."""
    for rows, idx in ((h.ground(frame), h.ground_indices(frame)), (h.nonground(frame), h.nonground_indices(frame))):
        want = np.ascontiguousarray(exp[idx, :3])
        assert rows.shape == want.shape
        assert np.array_equal(rows.view(np.uint32), want.view(np.uint32)), "xyz rows differ from the input rows"


def to_hip_params(op):
    """pwpp_hip.Params with the fields of an oracle_lib.Params (the rest at their defaults)."""
    p = pwpp_hip.default_params()
    for name, _ in ol.Params._fields_:
        v = getattr(op, name)
        if hasattr(v, "__len__"):
            for k in range(4):
                getattr(p, name)[k] = v[k]
        else:
            setattr(p, name, v)
    return p


@pytest.fixture(scope="module")
def oracle(oracle_built):
    return oracle_built.restatement()


@pytest.fixture(scope="module")
def frames(kitti):
    syn = pwpp_synth.add_edge_cases(pwpp_synth.make_cloud(23, beams=32, azimuth_steps=900), 23)
    f = {"k%d" % k: kitti[k] for k in range(6)}
    f.update(syn=syn, empty=np.zeros((0, 4), np.float32), one=kitti[4][7:8].copy(), ten=kitti[2][1000:1010].copy())
    return f


MIXED = ["k0", "empty", "one", "syn", "ten", "k3"]   # sizes 0, 1 and 10 next to KITTI frames
STREAM_STEPS = [["k1", "syn", "k4"], ["k2", "k5", "syn"], ["k0", "k3", "k1"]]   # 3 streams x 3 steps

_fresh_refs, _stream_refs = {}, {}


def fresh_ref(oracle, frames, name, cols):
    key = (name, cols)
    if key not in _fresh_refs:
        _fresh_refs[key] = ol.Estimator(oracle, arith=ol.ARITH_FXP).run(frames[name][:, :cols]) if len(frames[name]) else None
    return _fresh_refs[key]


def stream_refs(oracle, frames, cols):
    if cols not in _stream_refs:
        ests = [ol.Estimator(oracle, arith=ol.ARITH_FXP) for _ in range(3)]
        _stream_refs[cols] = [[ests[s].run(frames[name][:, :cols]) for s, name in enumerate(step)] for step in STREAM_STEPS]
    return _stream_refs[cols]


def run_and_check(h, frames, names, layout, mem, mode, refs, salt):
    exps = [expected_array(frames[n], layout) for n in names]
    placed = Placed([encode(e, layout, salt + k) for k, e in enumerate(exps)], mem)
    try:
        submit(h, placed, layout, [len(e) for e in exps], mode)
        for k, (e, ref) in enumerate(zip(exps, refs)):
            if ref is None:
                assert h.counts(k) == (0, 0, 0)
                continue
            assert_frame_equal(h, k, ref, len(e))
            assert_rows_bitwise(h, k, e)   # (device memory: the gather reads the caller's buffer, still alive here)
        placed.assert_unchanged()
    finally:
        placed.free()


@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_layout_memory_and_path(frames, oracle, layout, mem):
    """One layout from one memory kind down every path: a fresh single frame; a fresh batch of six mixing sizes 0, 1 and 10 with
    KITTI and synthetic frames, with one-pass binning, with two-pass binning (option one_pass = 0), and with segments far too
    small (one_pass_scale = 0.02: every frame overflows and is binned again from the caller's input); three stateful streams
    over three steps."""
    cols = cols_of(layout)
    salt = 100 * list(LAYOUTS).index(layout) + 10 * MEMS.index(mem)
    for path in PATHS:
        h = pwpp_hip.Handle()
        if path == "streams":
            h.set_num_streams(3)
            for step, refs in zip(STREAM_STEPS, stream_refs(oracle, frames, cols)):
                run_and_check(h, frames, step, layout, mem, pwpp_hip.MODE_STREAMS, refs, salt)
            h.close()
            continue
        names = [["k0", "k1", "k2", "k3", "k4", "k5"][salt % 6]] if path == "fresh1" else MIXED
        if path == "fresh6_two_pass":
            h.set_option("one_pass", 0)
        if path == "redo":
            h.set_option("one_pass_scale", 0.02)
        run_and_check(h, frames, names, layout, mem, pwpp_hip.MODE_FRESH, [fresh_ref(oracle, frames, n, cols) for n in names], salt)
        one_pass, redone = h.redo_stats()
        if path == "fresh6_two_pass":
            assert h.one_pass_stats() == (0, 0), "two-pass binning expected"
        elif path == "redo":
            assert redone > 0, "the overflow redo did not run"
        else:
            assert one_pass > 0 and redone == 0, "one-pass binning expected"
        h.close()


@pytest.mark.parametrize("layout", ["col4", "col3", "fields48", "fields12"])
def test_reference_order_from_device(frames, oracle, layout):
    """set_output_order(1) on device input: k_emit fetches the heights of the points R-VPF removed from the caller's buffer, in the
    caller's layout.  The parameter set makes R-VPF strip points (checked against the oracle without R-VPF)."""
    p = pwpp_hip.default_params()
    p.uprightness_thr, p.th_dist_v = 0.9999, 0.3   # nearly every seed plane of zone 0 counts as vertical: R-VPF strips its points
    op = to_oracle_params(p)
    names = ["k0", "syn", "k3", "k5"]
    exps = [expected_array(frames[n], layout) for n in names]
    refs = [ol.Estimator(oracle, op, arith=ol.ARITH_FXP).run(e) for e in exps]
    op_off = to_oracle_params(p)
    op_off.enable_RVPF = 0
    off = ol.Estimator(oracle, op_off, arith=ol.ARITH_FXP).run(exps[0])
    assert not np.array_equal(off.records["n_nonground"], refs[0].records["n_nonground"]), "R-VPF strips nothing here"
    for batch in ([0], [0, 1, 2, 3]):   # a single frame; a batch
        h = pwpp_hip.Handle(p)
        h.set_output_order(True)
        placed = Placed([encode(exps[i], layout, 7 + i) for i in batch], "device")
        try:
            submit(h, placed, layout, [len(exps[i]) for i in batch], pwpp_hip.MODE_FRESH)
            for k, i in enumerate(batch):
                assert_frame_equal(h, k, refs[i], len(exps[i]))
                z = exps[i][:, 2]
                for mine, theirs in ((h.ground_indices(k), refs[i].ground_idx), (h.nonground_indices(k), refs[i].nonground_idx)):
                    assert np.array_equal(z[mine], z[np.asarray(theirs)], equal_nan=True), "the z sequence differs from the reference's"
                assert_rows_bitwise(h, k, exps[i])
            placed.assert_unchanged()
        finally:
            placed.free()
        h.close()


@pytest.mark.parametrize("how", ["row4_host", "fields48_device"])
@pytest.mark.parametrize("kind", ["default", "ties"])
def test_input_values_at_the_boundary(oracle, kind, how):
    """NaN / +-inf in x or y with a finite z, NaN intensities with RNR on, +-0.0 and subnormal coordinates, radii exactly at
    min_range / max_range, RNR inputs exactly at its thresholds (tests/test_ref_fidelity.boundary_case): the three reference
    builds first, on the CPU; then the HIP path against the oracle, the partition of the cloud, the xyz getters and, where the
    builds agree, their ground set."""
    op, pts = boundary_case(oracle, kind)
    n = len(pts)
    for arith in (ol.ARITH_EIGEN_F32, ol.ARITH_EXACT_F64, ol.ARITH_F32_PACKET4):  # the restatement is the reference here too
        lib = ol.reference(arith)
        if lib is not None:
            a, b = ol.Estimator(lib, op, arith=arith).run(pts), ol.Estimator(oracle, op, arith=arith).run(pts)
            assert np.array_equal(a.ground_idx, b.ground_idx) and np.array_equal(a.nonground_idx, b.nonground_idx)
    want = reference_consensus(op, pts)
    ref = ol.Estimator(oracle, op, arith=ol.ARITH_FXP).run(pts)
    h = pwpp_hip.Handle(to_hip_params(op))
    layout, mem = how.split("_")
    placed = Placed([encode(pts, layout, 3)], mem)
    try:
        submit(h, placed, layout, [n], pwpp_hip.MODE_FRESH)
        assert_frame_equal(h, 0, ref, n)
        ng, nn, _ = h.counts(0)
        assert ng + nn + h.all_counts()[0, 5] == n
        assert ng + nn == len(ref.ground_idx) + len(ref.nonground_idx)
        assert_rows_bitwise(h, 0, pts)
        if want is not None:
            assert np.array_equal(np.sort(h.ground_indices(0)), want), "ground set differs from the reference builds"
        placed.assert_unchanged()
    finally:
        placed.free()
