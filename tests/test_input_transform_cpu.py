"""No-GPU checks of the input transform (pwpp_set_input_transforms, pwpp_transform_points): the exports and the header text, and
pwpp_transform_points -- the formula of include/pwpp.h, compiled from the function the kernels use -- bit for bit against the
numpy float32 restatement (tests/input_transform_ref.py)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import input_transform_ref as xf
import pwpp_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "patchwork-plusplus_amd")
F32 = np.float32
TINY = np.finfo(F32).tiny  # FLT_MIN, the reference's skip marker


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(pwpp_hip.LIB_PATH):
        subprocess.run(["make", "-C", PKG, "lib/libpwpp_hip.so"], check=True, stdout=subprocess.DEVNULL)
    return pwpp_hip.load()


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def random_points(seed, m):
    rng = np.random.default_rng(seed)
    p = rng.uniform(-80.0, 80.0, (m, 3))
    p[:, 2] = rng.uniform(-3.0, 6.0, m)
    p[: m // 8] *= rng.uniform(1e-6, 1e-2, (m // 8, 1))  # small magnitudes: cancellation against the translation
    return p.astype(F32)


def test_symbols_are_exported_and_declared(lib):
    hdr = open(os.path.join(ROOT, "include", "pwpp.h")).read()
    for name in ("pwpp_set_input_transforms", "pwpp_transform_points"):
        assert hasattr(lib, name), name
        assert "PWPP_API int %s(" % name in hdr, name
    assert "#define PWPP_HAS_INPUT_TRANSFORM 1" in hdr
    for phrase in ("0 * inf is NaN", "TRANSFORMED coordinates", "SENSOR's frame", "z == FLT_MIN"):
        assert phrase in hdr, phrase


@pytest.mark.parametrize("name, T", [
    ("tilt_and_translation", xf.rigid(np.radians(2.5), np.radians(-7.0), np.radians(31.0), t=(0.31, -0.07, 1.19))),
    ("millimetres", xf.rigid(0.0, 0.0, 0.0, scale=0.001)),
    ("mirror_and_shear", np.array([[1, 0.25, 0, 0], [0, -1, 0, 3], [0.125, 0, 1, -2]], F32)),
    ("identity", xf.IDENTITY),
])
def test_transform_points_equals_the_restatement_bit_for_bit(lib, name, T):
    p = random_points(len(name), 6007)  # (a few thousand points, no multiple of any vector width)
    if name == "millimetres":
        p = (p * F32(1000.0)).astype(F32)
    got = pwpp_hip.transform_points(T, p)
    want = xf.transform_points(T, p)
    assert got.dtype == F32 and got.shape == p.shape
    assert np.array_equal(bits(got), bits(want))
    assert np.array_equal(bits(pwpp_hip.transform_points(T.reshape(12), p)), bits(want))  # (12,) and (3, 4) are the same thing


def test_identity_returns_its_input_except_the_sign_of_zero(lib):
    """x' = ((1 * x + 0 * y) + 0 * z) + (+0.0).  For finite y, z the two middle terms are zeros of either sign, which leave a
    non-zero x alone; the LAST add has +0.0 on its right, and -0.0 + +0.0 is +0.0 in round-to-nearest.  So the identity
    returns every non-zero finite value unchanged, +0.0 as +0.0, and -0.0 ALWAYS as +0.0."""
    p = random_points(3, 4099)
    p[5] = [-0.0, 1.0, -1.0]
    p[6] = [0.0, -0.0, -0.0]
    p[7] = [-0.0, -0.0, -0.0]
    p[8] = [TINY, -TINY, 1e-45]          # the smallest normal and a subnormal survive
    p[9] = [3.4e38, -3.4e38, 1.0]
    got = pwpp_hip.transform_points(xf.IDENTITY, p)
    neg_zero = bits(p) == 0x80000000
    assert neg_zero.sum() == 6
    assert np.array_equal(bits(got)[~neg_zero], bits(p)[~neg_zero])
    assert (bits(got)[neg_zero] == 0).all()


def test_non_finite_rows_match_the_restatement(lib):
    """0 * inf is NaN: one infinite coordinate poisons all three outputs (none stays finite), also under the identity."""
    inf, nan = np.inf, np.nan
    p = np.array([[inf, 1, 2], [1, -inf, 2], [1, 2, inf], [nan, 1, 2], [1, nan, 2], [1, 2, nan], [inf, -inf, nan],
                  [inf, inf, inf], [3.4e38, 3.4e38, 3.4e38], [1, 2, 3]], F32)
    for T in (xf.IDENTITY, xf.rigid(0.02, -0.1, 0.5, t=(1, 2, 3)), np.array([[2, 2, 2, 0], [0, 0, 0, 1], [-2, 2, 0, 0]], F32)):
        got, want = pwpp_hip.transform_points(T, p), xf.transform_points(T, p)
        assert np.array_equal(np.isnan(got), np.isnan(want))
        ok = ~np.isnan(want)
        assert np.array_equal(bits(got)[ok], bits(want)[ok])
    got = pwpp_hip.transform_points(xf.IDENTITY, p)
    # one infinite coordinate leaves NO output of its point finite: NaN wherever its coefficient is zero (under the identity: the
    # other two outputs), +-inf or NaN elsewhere; a NaN coordinate makes NaN of all three
    assert not np.isfinite(got[:8]).any() and np.isnan(got[3:8]).all() and np.array_equal(got[9], p[9])
    assert np.array_equal(np.isnan(got[:3]), ~np.eye(3, dtype=bool)) and got[0, 0] == inf and got[1, 1] == -inf and got[2, 2] == inf
    assert np.array_equal(got[8], p[8])  # large and finite: untouched


def test_flt_min_is_only_special_where_it_is_the_result(lib):
    """The skip marker is tested on the transformed z.  Under a pure translation by t2 = FLT_MIN an input z of 0 lands exactly
    on the marker (0 * x + 0 * y + 1 * 0 is +0, and +0 + FLT_MIN is FLT_MIN), while an input z of FLT_MIN does not (2 FLT_MIN)."""
    T = xf.IDENTITY.copy()
    T[2, 3] = TINY
    p = np.array([[10, 5, 0.0], [10, 5, TINY], [10, 5, -1.7]], F32)
    got = pwpp_hip.transform_points(T, p)
    assert got[0, 2] == TINY and got[1, 2] == F32(2) * TINY and got[2, 2] == F32(-1.7)


def test_edge_arguments_and_in_place(lib):
    T = xf.rigid(0.1, 0.2, 0.3, t=(1, 2, 3))
    assert pwpp_hip.transform_points(T, np.zeros((0, 3), F32)).shape == (0, 3)
    p = random_points(9, 257)
    want = xf.transform_points(T, p)
    buf = p.copy()
    t12 = np.ascontiguousarray(T.reshape(12))
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert lib.pwpp_transform_points(vp(t12), vp(buf), len(buf), vp(buf)) == 0  # out may be xyz itself
    assert np.array_equal(bits(buf), bits(want))
    assert lib.pwpp_transform_points(None, vp(buf), 1, vp(buf)) == -1
    assert lib.pwpp_transform_points(vp(t12), None, 1, vp(buf)) == -1
    assert lib.pwpp_transform_points(vp(t12), vp(buf), -1, vp(buf)) == -1
    assert lib.pwpp_transform_points(vp(t12), None, 0, None) == 0
    assert lib.pwpp_set_input_transforms(None, vp(t12), 1) == -1  # null handle
    with pytest.raises(ValueError):
        pwpp_hip.transform_points(np.zeros((2, 12), F32), p)
    with pytest.raises(ValueError):
        pwpp_hip.transform_points(T, np.zeros((4, 4), F32))


def test_binding_shapes():
    for shape, k in (((12,), 1), ((3, 4), 1), ((5, 12), 5), ((5, 3, 4), 5), ((1, 12), 1)):
        t = pwpp_hip._transforms(np.arange(int(np.prod(shape)), dtype=np.float64).reshape(shape))
        assert t.shape == (k, 12) and t.dtype == F32 and t.flags.c_contiguous
        assert np.array_equal(t.ravel(), np.arange(12 * k, dtype=F32))
    for bad in ((4, 4), (11,), (2, 4, 3), (2, 2, 3, 4)):
        with pytest.raises(ValueError):
            pwpp_hip._transforms(np.zeros(bad))
    assert callable(pwpp_hip.Handle.set_input_transforms) and callable(pwpp_hip.Pipe.set_input_transforms)
    import pypatchworkpp
    assert hasattr(pypatchworkpp.patchworkpp, "setInputTransform")


def test_restatement_is_one_rounding_per_operation():
    """The yardstick itself, against exact rational arithmetic rounded step by step."""
    from fractions import Fraction
    T = xf.rigid(0.03, -0.12, 0.7, t=(0.5, -0.25, 1.75))
    p = random_points(1, 64)
    got = xf.transform_points(T, p)

    def fl(q):  # q rounded ONCE to the nearest float32, ties to even (never through a double: that would round twice)
        c = F32(float(q))
        near = [np.nextafter(c, F32(-np.inf)), c, np.nextafter(c, F32(np.inf))]
        return min(near, key=lambda v: (abs(Fraction(float(v)) - q), int(bits(v)[0]) & 1))

    for i in range(len(p)):
        for r in range(3):
            x, y, z = (Fraction(float(v)) for v in p[i])
            a, b, c = (fl(Fraction(float(T[r, k])) * v) for k, v in enumerate((x, y, z)))
            s = fl(Fraction(float(a)) + Fraction(float(b)))
            s = fl(Fraction(float(s)) + Fraction(float(c)))
            s = fl(Fraction(float(s)) + Fraction(float(T[r, 3])))
            assert bits(got[i, r]) == bits(s)
