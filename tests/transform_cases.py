"""The transforms and masks the transform tests share (tests/test_transform.py on the host, tests/test_transform_gpu.py on the GPU)."""
import numpy as np

N = 357                                # five full clusters of 64 and one of 37

# name -> keyword arguments of engine.xform
TRANSFORMS = {
    "translate": dict(translate=(0.31, -0.17, 0.23)),
    "rotate": dict(axis_angle=((1.0, 2.0, 3.0), 37.0)),                  # a generic rotation: axis (1, 2, 3) normalised, 37 degrees
    "scale_half": dict(scale=0.5),
    "scale_3": dict(scale=3.0),
    "all": dict(axis_angle=((-2.0, 1.0, 0.5), 118.0), scale=1.7, translate=(0.2, 0.1, -0.3), pivot=(0.4, -0.25, 0.15)),
    "half_turn_x": dict(rotate=(1.0, 0.0, 0.0, 0.0)),                     # 180 degrees about x: the quaternion is exact
    "identity": dict(),
}
ROTATIONS = ("rotate", "all", "half_turn_x", "identity")                  # the transforms whose rotation the SH tests go through


def make_xform(pkg, name):
    return pkg.engine.xform(**TRANSFORMS[name])


def _bits(n, idx):
    m = np.zeros(n, bool)
    m[np.asarray(idx, dtype=np.int64)] = True
    return m


def masks(pkg, n=N):
    """name -> what Engine.transform / engine.transform_eval take as `mask`: None, a boolean array over the n splats, or packed words"""
    every = pkg.engine.pack_mask(np.ones(n, bool)).copy()
    if n & 31:
        every[-1] |= np.uint32((0xffffffff << (n & 31)) & 0xffffffff)     # ... plus set bits behind n in the last word
    else:
        every = np.concatenate([every, np.array([0xffffffff], np.uint32)])
    out = {
        "null": None,
        "all": np.ones(n, bool),
        "first": _bits(n, [0]),
        "last": _bits(n, [n - 1]),
        "middle": _bits(n, [n // 2]),
        "word_edges": _bits(n, [k for k in (31, 32, 63, 64) if k < n]),
        "every_third": _bits(n, np.arange(0, n, 3)),
        "range_50_200": _bits(n, np.arange(min(50, n), min(200, n))),
        "empty": np.zeros(n, bool),
        "all_and_behind_n": every,
    }
    return out


def selected(mask, n=N):
    """the boolean array over n splats a mask of masks() selects"""
    if mask is None:
        return np.ones(n, bool)
    m = np.asarray(mask)
    if m.dtype == np.bool_:
        return m.copy()
    return np.unpackbits(np.ascontiguousarray(m, "<u4").view(np.uint8), bitorder="little")[:n].astype(bool)


def quat_matrix(q):
    """float64 rotation matrix of a quaternion (x, y, z, w) of any non-zero length"""
    x, y, z, w = np.asarray(q, np.float64) / np.linalg.norm(np.asarray(q, np.float64))
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def quat_mul(a, b):
    """a (x) b, both (x, y, z, w), float64"""
    ax, ay, az, aw = np.asarray(a, np.float64)
    bx, by, bz, bw = np.asarray(b, np.float64)
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


# Y_l(d): the polynomials gsr_shade_sh (csrc/k_preprocess.h) multiplies band l's coefficients with, its float32 constants and signs
_F = lambda v: float(np.float32(v))
SH_C1 = _F(0.4886025)
SH_C2 = [_F(v) for v in (1.0925484, -1.0925484, 0.3153916, -1.0925484, 0.5462742)]
SH_C3 = [_F(v) for v in (-0.5900436, 2.8906114, -0.4570458, 0.3731763, -0.4570458, 1.4453057, -0.5900436)]
BAND = {1: slice(0, 3), 2: slice(3, 8), 3: slice(8, 15)}                  # where band l sits among sh[0..14]


def sh_basis(l, d):
    """float64 (..., 2l + 1) for unit directions d (..., 3)"""
    d = np.asarray(d, np.float64)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
    if l == 1:
        out = [-SH_C1 * y, SH_C1 * z, -SH_C1 * x]
    elif l == 2:
        out = [SH_C2[0] * xy, SH_C2[1] * yz, SH_C2[2] * (2.0 * zz - xx - yy), SH_C2[3] * xz, SH_C2[4] * (xx - yy)]
    else:
        out = [SH_C3[0] * y * (3.0 * xx - yy), SH_C3[1] * xy * z, SH_C3[2] * y * (4.0 * zz - xx - yy),
               SH_C3[3] * z * (2.0 * zz - 3.0 * xx - 3.0 * yy), SH_C3[4] * x * (4.0 * zz - xx - yy), SH_C3[5] * z * (xx - yy),
               SH_C3[6] * x * (xx - 3.0 * yy)]
    return np.stack(out, axis=-1)


def basis_max(l):
    """max |Y_l| over the sphere, from a dense sample (a bound's factor, not a measurement of the code under test)"""
    rng = np.random.default_rng(5)
    d = rng.normal(size=(20000, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return float(np.abs(sh_basis(l, d)).max())
