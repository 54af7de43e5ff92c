"""The costmap (pwpp_costmap_grid, pwpp_costmap_obstacles) on a real MI355X, exactly equal -- cost and why -- to the numpy restatement
tests/costmap_ref.py, for every value of the option "costmap_path" in host and in device memory.  In device memory every byte image
sits at its own odd offset (1, 2, 3) behind a 256-byte boundary and dist2 at +4, their minimum; what surrounds them is poisoned and
must survive, and the inputs must not be written.  Path 2 deals four cells a lane behind the cost image's first 4-byte boundary and
PWPP_COSTMAP_GROUP_CELLS cells a workgroup (read from csrc/pwpp_costmap.h): the shapes are written for that."""
import functools

import numpy as np
import pytest

import costmap_ref as cr
import pwpp_hip
import reach_ref as rr
from test_costmap_cpu import group_cells, params, tparams
from test_gpu_obstacle_grid import _everything, small_cloud, three_frames

pytestmark = pytest.mark.gpu

E_STATE = -4
PATHS = (0, 1, 2)
G = group_cells()
POISON = -7


@pytest.fixture(scope="module")
def handle():
    return pwpp_hip.Handle()  # (no estimate call: pwpp_costmap_grid needs the handle's stream and buffer only)


def frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)
    return arrays


def device_bytes(n, offset, image=None, dtype=None):
    """A poisoned device array with room for n elements `offset` elements behind its 256-byte boundary, `image` copied there."""
    import torch
    kind = torch.int32 if dtype == np.int32 else torch.int8
    buf = torch.full((n + 256,), POISON, dtype=kind, device="cuda")
    assert buf.data_ptr() % 256 == 0
    if image is not None:
        flat = np.ascontiguousarray(image).reshape(-1)
        buf[offset:offset + n] = torch.from_numpy(flat.view(np.int8).copy() if dtype != np.int32 else flat.copy()).cuda()
    return buf


def intact(buf, n, offset, image, what):
    """The image of a device array; everything around it is still poison, and (image given) the image is unchanged."""
    raw = buf.cpu().numpy()
    assert (raw[:offset] == POISON).all() and (raw[offset + n:] == POISON).all(), "%s: an element outside the image was written" % what
    body = raw[offset:offset + n]
    if image is not None:
        assert body.tobytes() == np.ascontiguousarray(image).tobytes(), "%s: an input was written" % what
    return body


def on_host(h, p, o, t, d, curve, want_why):
    got = h.costmap_grid(p, occupancy=o, terrain=t, dist2=d, curve=curve, want_why=want_why)
    return got if want_why else (got, None)


def on_device(h, p, o, t, d, curve, want_why):
    import torch
    shape = next(a.shape for a in (o, t, d) if a is not None)
    shape3 = (1,) + shape if len(shape) == 2 else shape
    n = int(np.prod(shape))
    do, dt = (device_bytes(n, k, a) if a is not None else None for k, a in ((1, o), (2, t)))
    dd = device_bytes(n, 1, d, np.int32) if d is not None else None
    dc, dw = device_bytes(n, 3), device_bytes(n, 1)
    torch.cuda.synchronize()
    h.costmap_grid_device(shape3[2], shape3[1], shape3[0], p, dc.data_ptr() + 3, do.data_ptr() + 1 if do is not None else 0,
                          dt.data_ptr() + 2 if dt is not None else 0, dd.data_ptr() + 4 if dd is not None else 0, curve, dw.data_ptr() + 1 if want_why else 0)
    h.synchronize()  # (complete after pwpp_synchronize: the copies below are on another stream)
    for buf, off, a, name in ((do, 1, o, "occupancy"), (dt, 2, t, "terrain"), (dd, 1, d, "dist2")):
        if buf is not None:
            intact(buf, n, off, a, name)
    cost = intact(dc, n, 3, None, "cost").reshape(shape)
    why = intact(dw, n, 1, None, "why")
    assert want_why or (why == POISON).all(), "a why image that was not asked for was written"
    return cost, why.view(np.uint8).reshape(shape) if want_why else None


def same(got, want, what):
    for name, g, w in zip(("cost", "why"), got, want):
        if g is None:
            continue
        assert g.dtype == w.dtype and g.shape == w.shape, "%s: %s" % (what, name)
        if g.tobytes() != w.tobytes():
            bad = np.argwhere(g != w)
            assert False, "%s: %d cells of %s differ, the first %s: %r, expected %r" % (what, len(bad), name, bad[0], g[tuple(bad[0])], w[tuple(bad[0])])


def everywhere(h, p, o, t, d, curve, want, what, whys=(True,)):
    """Every path, in host and in device memory, against `want`."""
    for path in PATHS:
        h.set_option("costmap_path", path)
        try:
            for want_why in whys:
                same(on_host(h, p, o, t, d, curve, want_why), want, "%s (host, path %d, why %s)" % (what, path, want_why))
                same(on_device(h, p, o, t, d, curve, want_why), want, "%s (device, path %d, why %s)" % (what, path, want_why))
        finally:
            h.set_option("costmap_path", 0)


def reference(p, o, t, d, curve):
    return cr.fold(p.layers, p.occupancy_unknown, p.terrain_unknown, p.unknown_below, curve, o, t, d)


def random_curve(rng, n):
    c = np.sort(rng.integers(0, 100, n))[::-1].astype(np.uint8)
    c[0] = 100
    return c


# ---- the exhaustive frame: every pair of bytes -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def exhaustive(n_curve):
    rng = np.random.default_rng(n_curve)
    byte = np.arange(256, dtype=np.uint8).view(np.int8)
    o = np.broadcast_to(byte[None, :, None], (4, 256, 256)).copy()   # the row's byte
    t = np.broadcast_to(byte[None, None, :], (4, 256, 256)).copy()   # the column's byte
    d = np.empty((4, 256, 256), np.int32)
    d[0], d[1], d[2], d[3] = 0, n_curve - 1, n_curve, rng.integers(0, 2 * n_curve + 1, (256, 256))
    curve = random_curve(rng, n_curve)
    p = params(layers=7, occupancy_unknown=(-1, 35, -1)[n_curve % 3], terrain_unknown=(20, -1, -1)[n_curve % 3], unknown_below=(100, 101, 50)[n_curve % 3])
    want = reference(p, o, t, d, curve)
    frozen(o, t, d, curve, *want)
    return p, o, t, d, curve, want


@pytest.mark.parametrize("n_curve", (1, 2, 4097))
def test_every_pair_of_bytes_at_four_distances(handle, n_curve):
    p, o, t, d, curve, want = exhaustive(n_curve)
    everywhere(handle, p, o, t, d, curve, want, "n_curve %d" % n_curve)
    assert (want[0] == -1).any() and (want[0] == 100).any() and len(np.unique(want[1])) >= 8


# ---- shapes at which the dealing of four cells a lane can go wrong ---------------------------------------------------------------
SHAPES = [(1, 1), (3, 1), (1, 5), (7, 9), (64, 1), (65, 1), (1023, 1), (1024, 1), (1025, 1), (G - 1, 1), (G, 1), (G + 1, 1)]  # (nx, ny)
shape_ids = lambda s: "%dx%d" % s if isinstance(s, tuple) else str(s)


@functools.lru_cache(maxsize=None)
def shape_case(nx, ny, frames):
    k = SHAPES.index((nx, ny))
    rng = np.random.default_rng(100 * k + frames)
    o = rng.integers(-128, 128, (frames, ny, nx)).astype(np.int8)   # the full int8 range ...
    o[rng.random(o.shape) < 0.4] = 0                                 # ... and enough of the two bytes that mean something
    o[rng.random(o.shape) < 0.2] = 100
    t = rng.integers(-128, 128, (frames, ny, nx)).astype(np.int8)
    n_curve = (1, 2, 26, 4097)[k % 4]
    d = rng.integers(0, 2 * n_curve + 1, (frames, ny, nx)).astype(np.int32)
    d.reshape(-1)[0] = cr.DIST_BEYOND
    d.reshape(-1)[-1] = -1
    curve = random_curve(rng, n_curve)
    p = params(layers=7, occupancy_unknown=(-1, 50)[k % 2], terrain_unknown=(-1, 0, 100)[k % 3], unknown_below=(1, 50, 100, 101)[(k + frames) % 4])
    want = reference(p, o, t, d, curve)
    frozen(o, t, d, curve, *want)
    return p, o, t, d, curve, want


@pytest.mark.parametrize("frames", (1, 3))
@pytest.mark.parametrize("shape", SHAPES, ids=shape_ids)
def test_shapes_against_the_reference(handle, shape, frames):
    p, o, t, d, curve, want = shape_case(shape[0], shape[1], frames)
    everywhere(handle, p, o, t, d, curve, want, "%s x %d" % (shape_ids(shape), frames), whys=(True, False))


# ---- the call size at which path 0 changes kernels ---------------------------------------------------------------------------------
def quads_from_cells():
    import os
    src = open(os.path.join(os.path.dirname(pwpp_hip.LIB_PATH), "..", "csrc", "pwpp_costmap.h")).read()
    return int(src.split("#define PWPP_COSTMAP_QUADS_FROM_CELLS ")[1].split()[0])


@pytest.mark.parametrize("below", (1, 0))
def test_path_0_on_both_sides_of_its_threshold(handle, below):
    """Path 0 is path 1 below PWPP_COSTMAP_QUADS_FROM_CELLS cells a call and path 2 from there on: one cell below it and exactly at it
    every path gives the same bytes on the device, and a sample of the cells -- both ends and 2^16 random ones -- equals the reference."""
    import torch
    cells = quads_from_cells() - below
    nx = next(k for k in range(min(cells, 32768), 0, -1) if cells % k == 0)   # (frames, 1, nx) with the longest row that divides it
    frames = cells // nx
    gen = torch.Generator(device="cuda").manual_seed(11 + below)
    curve = random_curve(np.random.default_rng(5), 26)
    o = torch.randint(-128, 128, (cells + 8,), generator=gen, device="cuda", dtype=torch.int8)
    o[torch.rand(cells + 8, generator=gen, device="cuda") < 0.5] = 0
    o[torch.rand(cells + 8, generator=gen, device="cuda") < 0.2] = 100
    t = torch.randint(-128, 128, (cells + 8,), generator=gen, device="cuda", dtype=torch.int8)
    d = torch.randint(0, 60, (cells + 8,), generator=gen, device="cuda", dtype=torch.int32)
    p = params(layers=7, occupancy_unknown=-1, terrain_unknown=40, unknown_below=100)
    out = {}
    for path in PATHS:
        cost, why = (torch.full((cells + 8,), POISON, dtype=torch.int8, device="cuda") for _ in range(2))
        torch.cuda.synchronize()
        handle.set_option("costmap_path", path)
        try:
            handle.costmap_grid_device(nx, 1, frames, p, cost.data_ptr() + 3, o.data_ptr() + 1, t.data_ptr() + 2, d.data_ptr() + 4, curve, why.data_ptr() + 1)
            handle.synchronize()
        finally:
            handle.set_option("costmap_path", 0)
        assert bool((cost[:3] == POISON).all()) and bool((cost[3 + cells:] == POISON).all()) and bool((why[:1] == POISON).all()) and bool((why[1 + cells:] == POISON).all())
        out[path] = (cost[3:3 + cells], why[1:1 + cells])
    for path in (1, 2):
        assert torch.equal(out[0][0], out[path][0]) and torch.equal(out[0][1], out[path][1]), "path 0 and path %d differ at %d cells" % (path, cells)
    pick = np.unique(np.concatenate([np.arange(4096), np.arange(cells - 4096, cells), np.random.default_rng(below).integers(0, cells, 1 << 16)]))
    idx = torch.from_numpy(pick).cuda()
    want = reference(p, o[1:1 + cells][idx].cpu().numpy(), t[2:2 + cells][idx].cpu().numpy(), d[1:1 + cells][idx].cpu().numpy(), curve)
    assert out[0][0][idx].cpu().numpy().tobytes() == want[0].tobytes() and out[0][1][idx].cpu().numpy().view(np.uint8).tobytes() == want[1].tobytes()


# ---- each layer alone and every subset ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layers", range(1, 8))
def test_every_subset_of_the_layers_reads_only_its_own_images(handle, layers):
    p0, o, t, d, curve, _ = shape_case(7, 9, 3)
    p = params(layers=layers, occupancy_unknown=p0.occupancy_unknown, terrain_unknown=p0.terrain_unknown, unknown_below=p0.unknown_below)
    want = reference(p, o, t, d, curve)
    given = (o if layers & 1 else None, t if layers & 4 else None, d if layers & 2 else None)   # an image whose layer is off is absent
    everywhere(handle, p, given[0], given[1], given[2], curve if layers & 2 else None, want, "layers %d" % layers, whys=(True, False))
    off_o, off_t = np.full(o.shape, 100, np.int8), np.full(o.shape, 100, np.int8)   # ... or present and not read
    same(on_host(handle, p, o if layers & 1 else off_o, t if layers & 4 else off_t, d, curve, True), want, "layers %d, every image given" % layers)
    bits = int(np.bitwise_or.reduce(want[1].reshape(-1)))
    assert bits & 7 & ~layers == 0 and (bits & 7) != 0


# ---- the distances the call computes itself ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def occupancy_case():
    rng = np.random.default_rng(77)
    o = rng.integers(-128, 128, (3, 33, 40)).astype(np.int8)
    o[o == 100] = 99
    o[rng.random(o.shape) < 0.05] = 100   # about 5 % occupied
    o[2, :, :20][o[2, :, :20] == 100] = 0  # a half without obstacles: distances beyond every cap
    t = rng.integers(-128, 128, o.shape).astype(np.int8)
    brute = cr.dist2_brute(o == 100)
    frozen(o, t, brute)
    return o, t, brute


@pytest.mark.parametrize("n_curve", (1, 2, 26, 4097))
def test_own_distances_equal_the_uncapped_distance_image(handle, n_curve):
    o, t, brute = occupancy_case()
    uncapped = handle.distance_grid((o == 100).astype(np.int32), want_nearest=False, want_metres=False)[0]
    assert uncapped.tobytes() == brute.tobytes()
    assert (brute > cr.cap(n_curve) ** 2).any() or n_curve == 4097
    curve = random_curve(np.random.default_rng(n_curve), n_curve)
    for layers in (2, 3, 6, 7):
        p = params(layers=layers, occupancy_unknown=-1, terrain_unknown=30, unknown_below=100)
        want = reference(p, o, t, brute, curve)
        what = "own distances, n_curve %d, layers %d" % (n_curve, layers)
        tt = t if layers & 4 else None
        everywhere(handle, p, o, tt, None, curve, want, what, whys=(True,))
        same(on_host(handle, p, o, tt, uncapped, curve, True), want, what + ": the supplied image")
        same(on_device(handle, p, o if layers & 1 else None, tt, uncapped, curve, True), want, what + ": the supplied image (device)")


def test_a_frame_without_obstacles_and_one_that_is_all_obstacle(handle):
    o = np.zeros((2, 5, 9), np.int8)
    o[1] = 100
    curve = np.array([100, 60, 30], np.uint8)
    p = params(layers=2)
    want = reference(p, o, None, cr.dist2_brute(o == 100), curve)
    assert (want[0][0] == 0).all() and (want[0][1] == 100).all()
    everywhere(handle, p, o, None, None, curve, want, "empty and full")


# ---- pwpp_costmap_obstacles: the chain ------------------------------------------------------------------------------------------------
GRID = (-16.0, -16.0, 0.5, 64, 64)
BAND = (0.2, 2.5)
ORIGINS = np.array([[0.2, 0.3], [-15.9, 15.9], [4.0, -7.5]])
CHAIN_CURVE = pwpp_hip.costmap_curve(0.5, 0.4, 2.0, 1.2, 99) if hasattr(pwpp_hip, "costmap_curve") else None


def chain_on_device(h, p, tp, first, frames, ground_only, keep):
    """costmap_obstacles into device arrays at odd offsets; keep: the layers' images stay in the handle.  Returns (cost, why, occupancy, dist2, terrain)."""
    import torch
    nx, ny = GRID[3], GRID[4]
    n = frames * nx * ny
    dc, dw, do, dt = device_bytes(n, 3), device_bytes(n, 1), device_bytes(n, 1), device_bytes(n, 2)
    dd = device_bytes(n, 1, None, np.int32)
    torch.cuda.synchronize()
    h.costmap_obstacles_device(*GRID, p, dc.data_ptr() + 3, h_min=BAND[0], h_max=BAND[1], min_count=2, origin_xy=ORIGINS[first:first + frames], max_range=40,
                               terrain_params=tp, curve=CHAIN_CURVE, why_ptr=dw.data_ptr() + 1, occupancy_ptr=0 if keep else do.data_ptr() + 1,
                               dist2_ptr=0 if keep else dd.data_ptr() + 4, terrain_ptr=0 if keep else dt.data_ptr() + 2, frame_first=first, frames=frames,
                               ground_only=ground_only)
    h.synchronize()
    shape = (frames, ny, nx)
    out = [intact(dc, n, 3, None, "cost").reshape(shape), intact(dw, n, 1, None, "why").view(np.uint8).reshape(shape)]
    for buf, off, bit in ((do, 1, 1), (dd, 1, 2), (dt, 2, 4)):
        body = intact(buf, n, off, None, "a layer's image")
        if keep or not p.layers & bit:
            assert (body == POISON).all(), "an image that was not asked for, or whose layer is off, was written"
            out.append(None)
        else:
            out.append(body.reshape(shape))
    return out


@pytest.fixture(scope="module")
def batch():
    h = pwpp_hip.Handle()
    h.set_labels(True)  # (_everything reads them)
    h.estimate_ground_batch(three_frames(), mode=pwpp_hip.MODE_FRESH)  # a 16-beam scan, an empty frame, a frame that is all unref
    return h


@functools.lru_cache(maxsize=None)
def stages(ground_only):
    """The images of the stand-alone calls for all three frames: (occupancy, dist2 uncapped, dist2 capped, terrain)."""
    h = pwpp_hip.Handle()
    h.estimate_ground_batch(three_frames(), mode=pwpp_hip.MODE_FRESH)
    occ = h.visibility_obstacles(*GRID, *BAND, origin_xy=ORIGINS, min_count=2, max_range=40, ground_only=ground_only)[1]
    far = h.distance_obstacles(*GRID, *BAND, min_count=2, ground_only=ground_only, want_nearest=False, want_metres=False)[0]
    near = h.distance_obstacles(*GRID, *BAND, min_count=2, max_dist=cr.cap(len(CHAIN_CURVE)), ground_only=ground_only, want_nearest=False, want_metres=False)[0]
    ter = h.terrain_ground(*GRID, tparams(), ground_only=ground_only)[4]
    return frozen(occ, far, near, ter)


@pytest.mark.parametrize("ground_only", (False, True))
@pytest.mark.parametrize("layers", range(1, 8))
def test_the_chain_is_the_fold_of_the_stand_alone_calls(batch, layers, ground_only):
    h = batch
    occ, far, near, ter = stages(ground_only)
    assert (occ == 100).sum() > 20 and (occ == 0).sum() > 100 and (ter >= 0).sum() > 200 and (near != far).any()
    before = _everything(h, 3)
    p = params(layers=layers, occupancy_unknown=-1, terrain_unknown=-1, unknown_below=100)
    tp = tparams() if layers & 4 else None
    for first, frames in ((0, 3), (1, 2), (0, 1)):
        rng = slice(first, first + frames)
        want = reference(p, occ[rng], ter[rng], far[rng], CHAIN_CURVE)   # (the fold of the uncapped image: the cap changes no byte of it)
        assert want[0].tobytes() == reference(p, occ[rng], ter[rng], near[rng], CHAIN_CURVE)[0].tobytes()
        for path in PATHS:
            h.set_option("costmap_path", path)
            what = "layers %d, frames [%d, %d), path %d, ground_only %s" % (layers, first, first + frames, path, ground_only)
            got = h.costmap_obstacles(*GRID, p, *BAND, min_count=2, origin_xy=ORIGINS[rng], max_range=40, terrain_params=tp, curve=CHAIN_CURVE, frame_first=first,
                                      frames=frames, ground_only=ground_only, want_why=True, want_layers=True)
            same(got[:2], want, what)
            same((h.costmap_obstacles(*GRID, p, *BAND, min_count=2, origin_xy=ORIGINS[rng], max_range=40, terrain_params=tp, curve=CHAIN_CURVE, frame_first=first,
                                      frames=frames, ground_only=ground_only)[0], None), want, what + ": everything kept")
            for keep in (True, False):
                dev = chain_on_device(h, p, tp, first, frames, ground_only, keep)
                same(dev[:2], want, what + " (device, layers %s)" % ("kept" if keep else "returned"))
                if not keep:
                    got_dev = dev[2:]
                    for g, d_ in zip(got[2:], got_dev):
                        assert (g is None) == (d_ is None) and (g is None or g.tobytes() == d_.tobytes()), what + ": host and device layers differ"
            for bit, g, w, name in ((1, got[2], occ[rng], "occupancy"), (2, got[3], near[rng], "dist2"), (4, got[4], ter[rng], "terrain")):
                assert (g is None) == (not layers & bit), what
                assert g is None or g.tobytes() == w.tobytes(), what + ": %s differs from the stand-alone call's" % name
        h.set_option("costmap_path", 0)
    assert _everything(h, 3) == before, "the costmap changed the results of the call it reads"


def test_errors_of_the_chain_with_a_real_handle():
    h = pwpp_hip.Handle()
    p = params()
    with pytest.raises(pwpp_hip.PwppError, match="pwpp error %d" % E_STATE):   # before any estimate call
        h.costmap_obstacles(*GRID, p, *BAND, origin_xy=(0.0, 0.0), terrain_params=tparams(), curve=CHAIN_CURVE, frames=1)
    h.estimate_ground(small_cloud(5))
    with pytest.raises(pwpp_hip.PwppError, match="frames"):
        h.costmap_obstacles(*GRID, p, *BAND, origin_xy=(0.0, 0.0), terrain_params=tparams(), curve=CHAIN_CURVE, frame_first=1, frames=1)
    with pytest.raises(pwpp_hip.PwppError, match="outside the grid"):
        h.costmap_obstacles(*GRID, p, *BAND, origin_xy=(16.0, 0.0), terrain_params=tparams(), curve=CHAIN_CURVE)
    with pytest.raises(pwpp_hip.PwppError, match="4-byte aligned"):
        import torch
        buf = torch.zeros(64 * 64 * 8, dtype=torch.int8, device="cuda")
        h.costmap_obstacles_device(*GRID, p, buf.data_ptr(), *BAND, origin_xy=(0.0, 0.0), terrain_params=tparams(), curve=CHAIN_CURVE, dist2_ptr=buf.data_ptr() + 8194)
    with pytest.raises(Exception):
        h.set_option("costmap_path", 3)
    with pytest.raises(Exception):
        h.set_option("costmap_path", -1)


# ---- costmap, then reach, on the device with no synchronise between -----------------------------------------------------------------
def test_costmap_then_reach_on_the_device():
    import torch
    o, t, brute = occupancy_case()
    o, t, brute = o[:1], t[:1], brute[:1]
    curve = np.array([100, 100, 90, 90, 70, 50, 50, 50, 30, 20, 10], np.uint8)
    p = params(layers=7, occupancy_unknown=0, terrain_unknown=20, unknown_below=101)
    cost = reference(p, o, t, brute, curve)[0]
    rp = rr.params(base=2, lethal=100, unknown=-1)
    src = (3, 30)
    want = rr.reach(cost, src, rp)
    assert 100 < (want[0] != rr.NONE).sum() < cost.size
    n = o.size
    h = pwpp_hip.Handle()
    do, dt, dc = device_bytes(n, 1, o), device_bytes(n, 2, t), device_bytes(n, 3)
    dr, df = device_bytes(n, 1, None, np.int32), device_bytes(n, 1, None, np.int32)
    torch.cuda.synchronize()
    for path in PATHS:
        h.set_option("costmap_path", path)
        h.costmap_grid_device(40, 33, 1, p, dc.data_ptr() + 3, do.data_ptr() + 1, dt.data_ptr() + 2, 0, curve)
        h.reach_grid_device(40, 33, 1, dc.data_ptr() + 3, src, pwpp_hip.ReachParams(rp["base"], rp["lethal"], rp["unknown"], rp["clearance2"], rp["max_reach"], 0),
                            dr.data_ptr() + 4, df.data_ptr() + 4)
        h.synchronize()
        assert intact(dc, n, 3, None, "cost").tobytes() == cost.tobytes()
        assert intact(dr, n, 1, None, "reach").tobytes() == want[0].tobytes() and intact(df, n, 1, None, "from").tobytes() == want[1].tobytes(), "path %d" % path
        dr.fill_(POISON), df.fill_(POISON), dc.fill_(POISON)
        torch.cuda.synchronize()


# ---- workspace ------------------------------------------------------------------------------------------------------------------
def test_workspace_and_that_nothing_else_moves():
    h = pwpp_hip.Handle()
    empty = h.workspace_bytes()
    o, t, brute = occupancy_case()
    curve = random_curve(np.random.default_rng(3), 26)
    p = params(layers=7, terrain_unknown=0)
    same(on_host(h, p, o, t, None, curve, True), reference(p, o, t, brute, curve), "before any estimate call")
    assert h.workspace_bytes() >= empty + o.size * (4 + 4 + 4), "the cluster buffer is not counted"   # count, the distance kernels' image, dist2
    h.trim_workspace()
    assert h.workspace_bytes() == empty, "pwpp_trim_workspace did not free the cluster buffer"
    a, b = pwpp_hip.Handle(), pwpp_hip.Handle()
    frames = three_frames()
    for w in (a, b):
        w.set_labels(True)
        w.set_order(pwpp_hip.ORDER_CLOUD)  # (a deterministic order of the index lists: two calls are compared below)
        w.estimate_ground_batch(frames, mode=pwpp_hip.MODE_FRESH)
    assert a.workspace_bytes() == b.workspace_bytes()   # with the feature unused nothing is allocated
    before, t_before = _everything(b, 3), b.time_us()
    b.costmap_obstacles(*GRID, p, *BAND, origin_xy=(0.0, 0.0), terrain_params=tparams(), curve=CHAIN_CURVE)
    assert b.workspace_bytes() > a.workspace_bytes()
    assert _everything(b, 3) == before and b.time_us() == t_before, "the costmap changed the results of the call it reads"
    for w in (a, b):
        w.estimate_ground_batch(frames, mode=pwpp_hip.MODE_FRESH)
    assert _everything(b, 3) == _everything(a, 3), "an estimate call after a costmap call differs from one without"


# ---- the C++ mirror through pybind11 -----------------------------------------------------------------------------------------------
def test_pybind_module_agrees_with_the_ctypes_handle():
    import pypatchworkpp
    pp = pypatchworkpp.patchworkpp(pypatchworkpp.Parameters())
    h = pwpp_hip.Handle()
    curve = pypatchworkpp.patchworkpp.inflationCurve(0.5, 0.4, 2.0, 1.2)
    assert curve.dtype == np.uint8 and curve.tobytes() == CHAIN_CURVE.tobytes()
    with pytest.raises(RuntimeError):
        pp.getCostmap(-30.0, -12.0, 0.5, 120, 48, 0.2, 2.5, curve)  # no frame yet
    om, em, other = pypatchworkpp.FusedObstacleMap(), pypatchworkpp.FusedElevationMap(), pypatchworkpp.FusedElevationMap()
    om.x0, om.y0, om.cell, om.nx, om.ny = -32.0, -14.0, 0.5, 130, 56
    em.x0, em.y0, em.cell, em.nx, em.ny, em.n_max = -32.0, -14.0, 0.5, 130, 56, 4
    other.x0, other.y0, other.cell, other.nx, other.ny, other.n_max = -32.0, -14.0, 0.5, 130, 55, 4
    with pytest.raises(ValueError):
        pp.fusedCostmap(om, None, curve)  # no occupancy yet
    pose = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
    for seed in (5, 5):   # maps fused from two frames: the same scan twice, so that a cell it hits reaches occupied_at
        pts = small_cloud(seed)
        pp.estimateGround(pts)
        h.estimate_ground(pts)
        _, occupancy = pp.updateObstacleMap(om, pose, -30.0, -12.0, 0.5, 120, 48, 0.2, 2.5)[:2]
        mean = pp.updateElevationMap(em, pose, 0.0, -30.0, -12.0, 0.5, 120, 48)[2]
        pp.updateElevationMap(other, pose, 0.0, -30.0, -12.0, 0.5, 120, 48)
    cp, tp = pypatchworkpp.CostmapParams(), pypatchworkpp.TerrainParams()
    assert (cp.layers, cp.occupancy_unknown, cp.terrain_unknown, cp.unknown_below) == (7, -1, -1, 101)
    got = pp.getCostmap(-30.0, -12.0, 0.5, 120, 48, 0.2, 2.5, curve)   # the defaults: every layer, unknown wins, the origin at (0, 0) m
    want = h.costmap_obstacles(-30.0, -12.0, 0.5, 120, 48, params(), 0.2, 2.5, terrain_params=pwpp_hip.TerrainParams(1, 3, np.inf, np.inf, np.inf, 0),
                               curve=curve, want_why=True)
    for g, w, dtype in zip(got, want, (np.int8, np.uint8)):
        assert g.dtype == dtype and g.shape == (48, 120) and g.tobytes() == w[0].tobytes()
    assert (got[0] == 100).any() and (got[0] == -1).any()
    cp.occupancy_unknown, cp.terrain_unknown, cp.unknown_below = 10, 25, 100
    tp.radius, tp.min_known, tp.step_max, tp.slope_max, tp.rough_max = 2, 6, 0.3, 0.4, 0.05
    got = pp.fusedCostmap(om, em, curve, cp, tp)
    terrain = h.terrain_grid(mean, 0.5, pwpp_hip.TerrainParams(2, 6, 0.3, 0.4, 0.05, 0))[4]
    occupancy = np.asarray(occupancy, np.int8)
    p = params(occupancy_unknown=10, terrain_unknown=25, unknown_below=100)
    want = h.costmap_grid(p, occupancy=occupancy, terrain=terrain, curve=curve, want_why=True)
    ref = reference(p, occupancy, terrain, cr.dist2_brute((occupancy == 100)[None])[0], curve)
    for g, w, r in zip(got, want, ref):
        assert g.shape == (56, 130) and g.tobytes() == w.tobytes() == r.tobytes()
    assert (occupancy == 100).sum() > 5 and 3 <= len(np.unique(got[0]))
    cp.layers = 3
    got = pp.fusedCostmap(om, None, curve, cp)   # without an elevation map: occupancy and inflation
    p = params(layers=3, occupancy_unknown=10, terrain_unknown=25, unknown_below=100)
    assert got[0].tobytes() == h.costmap_grid(p, occupancy=occupancy, curve=curve).tobytes()
    with pytest.raises(ValueError):
        pp.fusedCostmap(om, other, curve)   # another geometry
    with pytest.raises(RuntimeError):
        pp.fusedCostmap(om, None, curve)    # the terrain layer without an elevation map: the library names it
