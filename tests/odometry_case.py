"""The yardstick of the odometry tests, written out: the snippet rule of the reference's eval/odometry.py (dump_xyz, compute_ate and
the loop of eval_odom behind the network) in numpy, in any floating type -- float64 to stand beside the golden, np.longdouble to
measure how far the reference's own float64 result lies from the exact one.  Relative poses are formed as
[R0^-1 R1 | R0^-1 (t1 - t0)], the large global translations cancelling before anything multiplies them; 3x3 blocks are inverted by
cofactors (np.linalg has no extended precision).  Also: the trajectories the tests and the script's --synthetic mode generate, and
the unit in which the odometry tolerance is expressed."""
import numpy as np

# How far the reference's float64 `ates` / `speeds` of tests/golden/odometry.npz lie from this restatement evaluated in np.longdouble
# (x87 extended, eps 1.1e-19), worst over all cases, in units() below: measured on the CPU, profiles/eval_accumulators.txt.
REFERENCE_ERROR_UNITS = 0.787
# The tolerance of anything held against the golden: 8x that.  The device inverts in closed form and contracts to FMAs where numpy
# calls LAPACK and BLAS; each may contribute an error of the reference's own order.  The yardstick is the reference, never the kernel.
BOUND_UNITS = 8 * REFERENCE_ERROR_UNITS


def snippet_count(N, track_length):
    """S of dd_odom_snippet_count: snippets i = 0 .. N-1 have min(track_length-1, N-i) + 1 points and are kept iff that is at least
    track_length - 1."""
    if N < 1 or not 2 <= track_length <= 16:
        return -1
    return max(0, min(N, N - track_length + 3))


def pad_global(gt):
    """(N+1, 3 or 4, 4) -> (N+1, 4, 4) with last row 0 0 0 1, as the reference pads a 12-column file."""
    gt = np.asarray(gt)
    if gt.shape[1] == 3:
        last = np.zeros((gt.shape[0], 1, 4), dtype=gt.dtype)
        last[:, 0, 3] = 1
        gt = np.concatenate((gt, last), 1)
    return gt


def _inv3(m):
    c = np.empty((3, 3), dtype=m.dtype)
    for r in range(3):
        for k in range(3):
            r1, r2, k1, k2 = (r + 1) % 3, (r + 2) % 3, (k + 1) % 3, (k + 2) % 3
            c[r, k] = m[r1, k1] * m[r2, k2] - m[r1, k2] * m[r2, k1]
    det = (m[0] * c[0]).sum()
    return c.T / det


def local_pose(g0, g1):
    """inv(inv(g0) . g1) of two affine 4x4 poses."""
    i0 = _inv3(g0[:3, :3])
    rel_r, rel_t = i0 @ g1[:3, :3], i0 @ (g1[:3, 3] - g0[:3, 3])
    out = np.eye(4, dtype=g0.dtype)
    out[:3, :3] = _inv3(rel_r)
    out[:3, 3] = -(out[:3, :3] @ rel_t)
    return out


def snippets(pred, gt_global, track_length=5, dtype=np.float64):
    """(ates, speeds, extents): per kept snippet, in `dtype`; extents[i] = the largest distance of snippet i's ground-truth points from
    its first."""
    pred = np.asarray(pred).astype(dtype)
    gt = pad_global(np.asarray(gt_global)).astype(dtype)
    N = pred.shape[0]
    assert gt.shape == (N + 1, 4, 4), (pred.shape, gt.shape)
    local = [local_pose(gt[k], gt[k + 1]) for k in range(N)]
    ates, speeds, extents = [], [], []
    for i in range(max(snippet_count(N, track_length), 0)):
        steps = min(track_length - 1, N - i)
        cam_p, cam_g = np.eye(4, dtype=dtype), np.eye(4, dtype=dtype)
        pp, gp = [cam_p[:3, 3].copy()], [cam_g[:3, 3].copy()]
        for k in range(i, i + steps):
            cam_p, cam_g = cam_p @ pred[k], cam_g @ local[k]
            pp.append(cam_p[:3, 3].copy())
            gp.append(cam_g[:3, 3].copy())
        pp, gp = np.array(pp)[:, [2, 0, 1]], np.array(gp)
        pp = pp + (gp[0] - pp[0])[None]
        with np.errstate(invalid="ignore", divide="ignore"):
            scale = (gp * pp).sum() / (pp ** 2).sum()
            ates.append(np.sqrt(((pp * scale - gp) ** 2).sum()) / gp.shape[0])
        speeds.append(np.sqrt(((gp[1:] - gp[:-1]) ** 2).sum(1)).mean())
        extents.append(np.sqrt((gp ** 2).sum(1)).max())
    return np.array(ates, dtype=dtype), np.array(speeds, dtype=dtype), np.array(extents, dtype=dtype)


def units(got, want, gt_global, extents):
    """|got - want| per snippet in units of 2**-52 * (max |ground-truth coordinate| + snippet extent): the rounding of one float64
    operation on the largest numbers the evaluation touches.  NaN must meet NaN (returned as 0), anything else against NaN is inf."""
    got, want = np.asarray(got, dtype=np.longdouble), np.asarray(want, dtype=np.longdouble)
    scale = np.abs(pad_global(np.asarray(gt_global))[:, :3, 3]).max() + np.asarray(extents, dtype=np.longdouble)
    out = np.abs(got - want) / (np.longdouble(2.0) ** -52 * scale)
    both_nan = np.isnan(got) & np.isnan(want)
    out[both_nan] = 0
    out[np.isnan(out)] = np.inf
    return out.astype(np.float64)


def trajectory(n_poses, magnitude, seed, step=1.0):
    """(n_poses, 4, 4) float64 global poses: a start `magnitude` metres from the origin with an arbitrary heading, then ~`step` metres per
    frame along the camera's z axis with small random yaw / pitch changes (a car's track)."""
    rng = np.random.RandomState(seed)

    def rot(axis, angle):
        axis = axis / np.linalg.norm(axis)
        K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)

    pose = np.eye(4)
    pose[:3, :3] = rot(rng.randn(3), rng.uniform(0, np.pi))
    start = rng.randn(3)
    pose[:3, 3] = magnitude * start / np.linalg.norm(start)
    poses = [pose.copy()]
    for _ in range(n_poses - 1):
        move = np.eye(4)
        move[:3, :3] = rot(np.array([0.05 * rng.randn(), 1.0, 0.05 * rng.randn()]), 0.03 * rng.randn())
        move[:3, 3] = [0.02 * rng.randn(), 0.02 * rng.randn(), step * (1 + 0.2 * rng.randn())]
        pose = pose @ move
        poses.append(pose.copy())
    return np.stack(poses)


def pose_parameters(n, seed, scale=0.1):
    """(axisangle, translation) (n,1,3) float32 each: what a pose head would emit for n frame pairs."""
    rng = np.random.RandomState(seed)
    axisangle = (0.02 * rng.randn(n, 1, 3)).astype(np.float32)
    translation = (scale * np.array([0.1, 0.1, 1.0]) * (1 + 0.3 * rng.randn(n, 1, 3))).astype(np.float32)
    return axisangle, translation
