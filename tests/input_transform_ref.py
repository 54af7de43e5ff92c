"""numpy float32 restatement of the input transform (include/pwpp.h, pwpp_set_input_transforms / pwpp_transform_points):

    x' = fl32(fl32(fl32(fl32(r00 * x) + fl32(r01 * y)) + fl32(r02 * z)) + t0)      y', z' alike with rows 1 and 2

One rounding per operation: every operand is a float32 array or scalar, so numpy rounds each product and each sum to float32
(no FMA, no wider intermediate).  Used by the CPU tests as the yardstick of pwpp_transform_points and by the GPU tests to build
the sensor-frame clouds."""
import numpy as np

F32 = np.float32


def as_matrix(T):
    """(3, 4) float32 from (12,) or (3, 4)."""
    return np.asarray(T, F32).reshape(3, 4)


def transform_points(T, xyz):
    """(m, 3) float32: T applied to the rows of xyz (m, 3) float32, by the formula above."""
    T = as_matrix(T)
    xyz = np.asarray(xyz, F32)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    out = np.empty_like(xyz)
    with np.errstate(invalid="ignore", over="ignore"):  # (inf and NaN rows are part of the contract: whatever IEEE gives)
        for r in range(3):
            a = T[r, 0] * x
            b = T[r, 1] * y
            c = T[r, 2] * z
            s = a + b
            s = s + c
            out[:, r] = s + T[r, 3]
    assert out.dtype == F32
    return out


def transform_cloud(T, cloud):
    """The (n, 3 | 4) cloud whose xyz went through T; the fourth column (intensity) is passed through untouched."""
    out = np.array(cloud, F32, copy=True)
    out[:, :3] = transform_points(T, out[:, :3])
    return out


def rotation(roll, pitch, yaw=0.0):
    """Rz(yaw) Ry(pitch) Rx(roll) in double (radians)."""
    cr, sr, cp, sp, cy, sy = np.cos(roll), np.sin(roll), np.cos(pitch), np.sin(pitch), np.cos(yaw), np.sin(yaw)
    rx = np.array([[1, 0, 0], [0, cr, -sr], [0, sr, cr]])
    ry = np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]])
    rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1]])
    return rz @ ry @ rx


def rigid(roll, pitch, yaw=0.0, t=(0.0, 0.0, 0.0), scale=1.0):
    """(3, 4) float32 [scale * R | t]."""
    return np.concatenate([scale * rotation(roll, pitch, yaw), np.asarray(t, np.float64).reshape(3, 1)], axis=1).astype(F32)


def inverse(T):
    """The inverse affine map of a (3, 4) T, computed in double and rounded to float32 (approximate: it builds test clouds,
    nothing compares against it)."""
    T = as_matrix(T).astype(np.float64)
    ri = np.linalg.inv(T[:, :3])
    return np.concatenate([ri, -(ri @ T[:, 3:])], axis=1).astype(F32)


IDENTITY = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], F32)
