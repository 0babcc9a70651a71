"""An independent numpy restatement of the rollout selection: the row's frame count, the slice of
``terrain_util.slice_terrain_around_motion(localize=False)`` as two index tables, the scores of ``compute_motion_loss`` on that view
(through ``motion_terrain_ref``), the weights, the penalty, the noise, the thresholds and the stable rank.  ``test_mdm_select_cpu.py``
checks it against the reference's record (``tests/golden/mdm_select.npz``); it is the CPU-side statement of what the kernels of
``parc_mpath_select.hpp`` compute.
"""
import os

import numpy as np

import motion_terrain_ref as MR

F32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STATUS_NONFINITE, STATUS_TOO_LARGE, STATUS_EMPTY = 1, 2, 4
MAX_SLICE_DIM = 1024


class Fixture:
    """``mdm_select.npz``: the scene, the hand-made frames and the reference's record per mode (``s``: sliced, ``w``: whole terrain)."""

    def __init__(self, golden=GOLDEN):
        z = np.load(os.path.join(golden, "mdm_select.npz"))
        self.z = z
        self.hfs, self.min_points, self.dx, self.padding = z["hfs"], z["min_points"], float(z["dx"]), float(z["padding"])
        self.K = int(z["candidates"])
        self.P = self.hfs.shape[0]
        self.N = self.P * self.K
        self.frames = dict(root_pos=z["root_pos"], root_rot=z["root_rot"], joint_rot=z["joint_rot"], contacts=z["contacts"].astype(F32))
        self.F = self.frames["root_pos"].shape[1]
        self.final_frame, self.noise = z["final_frame"].astype(np.int32), z["noise"]
        self.w_contact, self.w_pen, self.penalty = float(z["w_contact"]), float(z["w_pen"]), float(z["penalty"])
        self.thresholds = dict(zip(("max_contact_loss", "max_pen_loss", "max_total_loss"), (float(v) for v in z["thresholds"])))
        self.points, self.point_body = z["points"], z["point_body"]
        self.row_path = np.repeat(np.arange(self.P), self.K)

    def rec(self, mode, key):
        return self.z[f"{mode}/{key}"]

    def sliced_hf(self, row):
        d = self.rec("s", "dims").astype(np.int64)
        off = np.concatenate([[0], np.cumsum(d[:, 0] * d[:, 1])])
        return self.rec("s", "hf")[off[row]:off[row + 1]].reshape(d[row])

    def paths(self):
        """A two-node path per terrain (the selection reads none)."""
        return [np.array([[mp[0] + 1.0, mp[1] + 1.0, 0.0], [mp[0] + 2.0, mp[1] + 1.0, 0.0]], F32) for mp in self.min_points]


def row_length(final_frame, num_frames):
    """len(frames[0:final_frame]) as Python slices it."""
    ff = int(final_frame)
    return max(num_frames + ff, 0) if ff < 0 else min(ff, num_frames)


def arange(start, end, step):
    """torch.arange of fp32 scalars: the size in double, the values start + step i in double stored as fp32."""
    n = int(np.ceil((float(end) - float(start)) / float(step)))
    return (float(start) + float(step) * np.arange(n, dtype=np.float64)).astype(F32)


def slice_tables(root_xy, min_point, dx, dims, padding):
    """(slice min point [2] fp32, ix, iy): the parent index of every slice column / row."""
    xy = np.asarray(root_xy, F32)
    mp, d = np.asarray(min_point, F32), F32(dx)
    lo = xy.min(0) - F32(padding)
    hi = xy.max(0) + F32(padding)
    grid = lambda p: (np.rint((p - mp) / d) * d + mp).astype(F32)   # noqa: E731  round_point_to_grid_point
    g0, g1 = grid(lo), grid(hi)
    tabs = []
    for a in (0, 1):
        pts = arange(g0[a], F32(g1[a] + d), d)
        tabs.append(np.clip(np.rint((pts - mp[a]) / d).astype(np.int64), 0, dims[a] - 1))
    return g0, tabs[0], tabs[1]


def view(hf, min_point, dx, root_pos, padding, slice_terrain):
    """(status, hf of the view, its min point): the materialised slice, or the terrain itself."""
    if root_pos.shape[0] < 1:
        return STATUS_EMPTY, None, None
    if not np.isfinite(root_pos).all():
        return STATUS_NONFINITE, None, None
    if not slice_terrain:
        return 0, hf, np.asarray(min_point, F32)
    g0, ix, iy = slice_tables(root_pos[:, 0:2], min_point, dx, hf.shape, padding)
    if len(ix) > MAX_SLICE_DIM or len(iy) > MAX_SLICE_DIM:
        return STATUS_TOO_LARGE, None, None
    return 0, hf[np.ix_(ix, iy)].astype(F32), g0


def select(cm, fx_frames, final_frame, hfs, min_points, dx, row_path, points, point_body, w_contact, w_pen, penalty, padding, slice_terrain, noise=None,
           max_contact_loss=np.inf, max_pen_loss=np.inf, max_total_loss=np.inf):
    """The whole selection.  Returns per-row arrays (``contact``, ``pen``, ``total``, ``valid``, ``status``, ``n``, ``min_point``, ``dims``,
    ``hf`` list) and ``order`` [N] (the rows of path 0 sorted, then path 1, ...), ``num_valid`` [P]."""
    N, Fn = fx_frames["root_pos"].shape[:2]
    nan = F32(np.nan)
    out = dict(contact=np.full(N, nan), pen=np.full(N, nan), total=np.full(N, nan), status=np.zeros(N, np.int32), n=np.zeros(N, np.int32),
               min_point=np.zeros((N, 2), F32), dims=np.zeros((N, 2), np.int32), hf=[None] * N)
    for r in range(N):
        p = int(row_path[r])
        n = row_length(final_frame[r], Fn)
        fr = {k: np.asarray(v[r, :n], F32) for k, v in fx_frames.items()}
        st, vhf, vmp = view(hfs[p], min_points[p], dx, fr["root_pos"], padding, slice_terrain)
        out["status"][r], out["n"][r] = st, n
        if st:
            continue
        out["min_point"][r], out["dims"][r], out["hf"][r] = vmp, vhf.shape, vhf
        pos, rot = MR.fk(cm, fr["root_pos"], fr["root_rot"], fr["joint_rot"])
        world = MR.world_points(pos, rot, points, point_body)
        pen, con = MR.scores(world, fr["contacts"], point_body, vhf, vmp, dx)
        c, q = F32(w_contact) * F32(con), F32(w_pen) * F32(pen)
        t = F32(c + q)
        if final_frame[r] < 0:
            t = F32(t + F32(penalty))
        if noise is not None:
            t = F32(t + F32(noise[r]))
        out["contact"][r], out["pen"][r], out["total"][r] = c, q, t
    with np.errstate(invalid="ignore"):
        out["valid"] = (out["contact"] < F32(max_contact_loss)) & (out["pen"] < F32(max_pen_loss)) & (out["total"] < F32(max_total_loss))
    order, nv = [], []
    for p in range(int(np.max(row_path)) + 1):
        rows = np.nonzero(np.asarray(row_path) == p)[0]
        order.append(rows[np.argsort(out["total"][rows], kind="stable")])   # NaN last, ties in row order
        nv.append(int(out["valid"][rows].sum()))
    out["order"], out["num_valid"] = np.concatenate(order), np.asarray(nv, np.int32)
    return out
