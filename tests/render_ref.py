"""Numpy reference ray-caster for the renderer tests (float64, independent of the HIP code).

Brute force: every top face and every wall face of a window of cells is intersected with every ray (no grid traversal), plus analytic
sphere / capsule / box intersections.  Conventions (camera, ID encoding, shadow-ray offset) are those documented in
parc_amd/csrc/parc_render.hpp and include/parc_env.h.
"""
import numpy as np

SKY, TOP, WALL = 0, 1, 2
SHADOW_BIT = 0x80
SHADOW_OFFSET = 2e-3
PRIM_TMIN = 1e-4
BOX, SPHERE, CAPSULE = 0, 1, 2


def camera_rays(eye, target, W, H, fov_y):
    """[H, W, 3] unit directions: f = target - eye, r = f x z (f x y when f is vertical), u = r x f, pixel centres."""
    f = np.asarray(target, np.float64) - np.asarray(eye, np.float64)
    f /= np.linalg.norm(f)
    r = np.cross(f, [0.0, 0.0, 1.0])
    if np.linalg.norm(r) < 1e-6:
        r = np.cross(f, [0.0, 1.0, 0.0])
    r /= np.linalg.norm(r)
    u = np.cross(r, f)
    th = np.tan(0.5 * fov_y)
    sx = ((np.arange(W) + 0.5) / W * 2.0 - 1.0) * th * W / H
    sy = (1.0 - (np.arange(H) + 0.5) / H * 2.0) * th
    d = f[None, None, :] + sx[None, :, None] * r[None, None, :] + sy[:, None, None] * u[None, None, :]
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def quat_rotate(q, v):
    q = np.asarray(q, np.float64)
    qv, w = q[:3], q[3]
    t = 2.0 * np.cross(qv, v)
    return v + w * t + np.cross(qv, t)


class Terrain:
    """Columns: cell (i, j) solid below hf[i, j] over [gx0 + i dx, gx0 + (i + 1) dx] x [...]; gx0 / gy0 = low edge of cell 0 (in the frame
    the rays are given in).  ``window`` = (i0, i1, j0, j1) half-open: the cells tested; None = all."""

    def __init__(self, hf, gx0, gy0, dx, dy, window=None):
        self.hf = np.asarray(hf, np.float64)
        self.gx0, self.gy0, self.dx, self.dy = float(gx0), float(gy0), float(dx), float(dy)
        X, Y = self.hf.shape
        self.window = window or (0, X, 0, Y)

    def window_exit(self, O, D):
        """Distance at which each ray leaves the window's xy box (inf when it never does)."""
        i0, i1, j0, j1 = self.window
        lo = np.array([self.gx0 + i0 * self.dx, self.gy0 + j0 * self.dy])
        hi = np.array([self.gx0 + i1 * self.dx, self.gy0 + j1 * self.dy])
        with np.errstate(divide="ignore", invalid="ignore"):
            ta = (lo[None] - O[:, :2]) / D[:, :2]
            tb = (hi[None] - O[:, :2]) / D[:, :2]
        t = np.where(np.isnan(ta), np.inf, np.maximum(ta, tb))
        return t.min(axis=1)

    def hit(self, O, D):
        """Nearest hit per ray: t (inf = none), id, normal (facing the ray), checker parity."""
        P = O.shape[0]
        best = np.full(P, np.inf)
        ids = np.zeros(P, np.int64)
        nrm = np.zeros((P, 3))
        par = np.zeros(P, np.int64)
        hf, dx, dy, gx0, gy0 = self.hf, self.dx, self.dy, self.gx0, self.gy0
        X, Y = hf.shape
        i0, i1, j0, j1 = self.window
        # an origin inside a column is a hit at distance 0
        ci = np.floor((O[:, 0] - gx0) / dx).astype(np.int64)
        cj = np.floor((O[:, 1] - gy0) / dy).astype(np.int64)
        ok = (ci >= 0) & (ci < X) & (cj >= 0) & (cj < Y)
        inside = np.zeros(P, bool)
        inside[ok] = O[ok, 2] < hf[ci[ok], cj[ok]]
        best[inside] = 0.0; ids[inside] = WALL; nrm[inside] = -D[inside]
        js = np.arange(j0, j1)
        ylo, yhi = gy0 + js * dy, gy0 + (js + 1) * dy
        with np.errstate(divide="ignore", invalid="ignore"):
            for i in range(i0, i1):
                xlo, xhi = gx0 + i * dx, gx0 + (i + 1) * dx
                h = hf[i, j0:j1]
                # top faces of the cells (i, j0..j1)
                t = (h[None, :] - O[:, 2:3]) / D[:, 2:3]
                x = O[:, 0:1] + t * D[:, 0:1]
                y = O[:, 1:2] + t * D[:, 1:2]
                m = (D[:, 2:3] < 0) & (t >= 0) & (x >= xlo) & (x <= xhi) & (y >= ylo[None]) & (y <= yhi[None])
                self._take(m, t, best, ids, nrm, par, TOP, np.array([0.0, 0.0, 1.0]), (i + js) & 1)
                # x faces: x = xhi between (i, j) and (i + 1, j) (or the rim), x = xlo on the rim of cell 0
                for xb, hn_side in ((xhi, i + 1),) + (((xlo, -1),) if i == 0 else ()):
                    hn = hf[hn_side, j0:j1] if 0 <= hn_side < X else np.full(j1 - j0, -np.inf)
                    t = (xb - O[:, 0:1]) / D[:, 0:1]
                    y = O[:, 1:2] + t * D[:, 1:2]
                    z = O[:, 2:3] + t * D[:, 2:3]
                    zl, zh = np.minimum(h, hn)[None], np.maximum(h, hn)[None]
                    m = (t >= 0) & (y >= ylo[None]) & (y <= yhi[None]) & (z >= zl) & (z < zh)
                    n = np.where(D[:, 0:1] > 0, -1.0, 1.0)
                    self._take(m, t, best, ids, nrm, par, WALL, None, 0, nx=n)
            # y faces: y = gy0 + j dy between (i, j - 1) and (i, j) (the rim when j = 0 or Y)
            for j in range(j0, j1 + 1):
                yb = gy0 + j * dy
                ia = np.arange(i0, i1)
                xlo, xhi = gx0 + ia * dx, gx0 + (ia + 1) * dx
                ha = hf[i0:i1, j - 1] if j - 1 >= 0 else np.full(i1 - i0, -np.inf)
                hb = hf[i0:i1, j] if j < Y else np.full(i1 - i0, -np.inf)
                t = (yb - O[:, 1:2]) / D[:, 1:2]
                x = O[:, 0:1] + t * D[:, 0:1]
                z = O[:, 2:3] + t * D[:, 2:3]
                zl, zh = np.minimum(ha, hb)[None], np.maximum(ha, hb)[None]
                m = (t >= 0) & (x >= xlo[None]) & (x <= xhi[None]) & (z >= zl) & (z < zh)
                n = np.where(D[:, 1:2] > 0, -1.0, 1.0)
                self._take(m, t, best, ids, nrm, par, WALL, None, 0, ny=n)
        return best, ids, nrm, par

    @staticmethod
    def _take(m, t, best, ids, nrm, par, kind, n, parity, nx=None, ny=None):
        tt = np.where(m, t, np.inf)
        k = tt.argmin(axis=1)
        tk = tt[np.arange(tt.shape[0]), k]
        upd = tk < best
        if not upd.any():
            return
        best[upd] = tk[upd]
        ids[upd] = kind
        if n is not None:
            nrm[upd] = n
        elif nx is not None:
            nrm[upd] = 0.0; nrm[upd, 0] = nx[upd, 0]
        else:
            nrm[upd] = 0.0; nrm[upd, 1] = ny[upd, 0]
        par[upd] = parity[k[upd]] if np.ndim(parity) else parity


def _sphere_t(O, D, c, r):
    oc = O - c
    b = (oc * D).sum(-1)
    cc = (oc * oc).sum(-1) - r * r
    disc = b * b - cc
    with np.errstate(invalid="ignore"):
        t = -b - np.sqrt(disc)
    return np.where((disc >= 0) & (t > PRIM_TMIN), t, np.inf)


def prim_hit(prim, O, D):
    """(t, normal) of one primitive dict {type, a, b, s, q} for every ray."""
    typ = prim["type"]
    a = np.asarray(prim["a"], np.float64)
    if typ == SPHERE:
        r = prim["s"][0]
        t = _sphere_t(O, D, a, r)
        x = O + np.where(np.isfinite(t), t, 0)[:, None] * D
        return t, (x - a) / r
    if typ == CAPSULE:
        b = np.asarray(prim["b"], np.float64)
        r = prim["s"][0]
        # union of the finite cylinder's side and the two end spheres: the entry point of the union is the smallest entry
        ax = b - a
        L = np.linalg.norm(ax)
        w = ax / L
        oa = O - a
        dp = D - (D @ w)[:, None] * w
        op = oa - (oa @ w)[:, None] * w
        qa = (dp * dp).sum(-1)
        qb = 2 * (dp * op).sum(-1)
        qc = (op * op).sum(-1) - r * r
        disc = qb * qb - 4 * qa * qc
        with np.errstate(invalid="ignore", divide="ignore"):
            tc = (-qb - np.sqrt(disc)) / (2 * qa)
        s = (oa @ w) + tc * (D @ w)
        tc = np.where((disc >= 0) & (qa > 1e-18) & (tc > PRIM_TMIN) & (s >= 0) & (s <= L), tc, np.inf)
        t = np.minimum(tc, np.minimum(_sphere_t(O, D, a, r), _sphere_t(O, D, b, r)))
        x = O + np.where(np.isfinite(t), t, 0)[:, None] * D
        u = np.clip(((x - a) @ w) / L, 0, 1)
        return t, (x - a - u[:, None] * ax) / r
    # box: slabs in the box frame
    q = np.asarray(prim["q"], np.float64)
    qi = np.array([-q[0], -q[1], -q[2], q[3]])
    Rm = np.stack([quat_rotate(qi, e) for e in np.eye(3)], axis=1)  # world -> box
    o = (O - a) @ Rm.T
    d = D @ Rm.T
    s = np.asarray(prim["s"], np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t1 = (-s[None] - o) / d
        t2 = (s[None] - o) / d
    lo, hi = np.minimum(t1, t2), np.maximum(t1, t2)
    par0 = d == 0
    lo = np.where(par0, np.where(np.abs(o) <= s[None], -np.inf, np.inf), lo)
    hi = np.where(par0, np.where(np.abs(o) <= s[None], np.inf, -np.inf), hi)
    tn, tf = lo.max(1), hi.min(1)
    t = np.where((tn <= tf) & (tn > PRIM_TMIN), tn, np.inf)
    axk = lo.argmax(1)
    nl = np.zeros_like(o)
    nl[np.arange(len(o)), axk] = -np.sign(d[np.arange(len(o)), axk])
    return t, nl @ Rm  # box -> world


def cast(terrain, prims, O, D):
    """Nearest hit: t, id, normal facing the ray."""
    t, ids, n, _ = terrain.hit(O, D)
    for p in prims:
        tp, np_ = prim_hit(p, O, D)
        upd = tp < t
        t[upd] = tp[upd]; ids[upd] = p["id"]; n[upd] = np_[upd]
    flip = (n * D).sum(-1) > 0
    n[flip] = -n[flip]
    return t, ids, n


def render(terrain, prims, eye, target, W, H, fov_y, sun=None):
    """(depth [H, W], id [H, W] uint8 with the shadow bit when ``sun`` is given, window-exit distance [H, W])."""
    D = camera_rays(eye, target, W, H, fov_y).reshape(-1, 3)
    O = np.broadcast_to(np.asarray(eye, np.float64), D.shape).copy()
    t, ids, n = cast(terrain, prims, O, D)
    hit = np.isfinite(t)
    out = ids.copy()
    if sun is not None and hit.any():
        sun = np.asarray(sun, np.float64) / np.linalg.norm(sun)
        Os = O[hit] + t[hit, None] * D[hit] + SHADOW_OFFSET * n[hit]
        Ds = np.broadcast_to(sun, Os.shape).copy()
        ts, _, _ = cast(terrain, prims, Os, Ds)
        out[np.nonzero(hit)[0][np.isfinite(ts)]] |= SHADOW_BIT
    return t.reshape(H, W), out.astype(np.uint8).reshape(H, W), terrain.window_exit(O, D).reshape(H, W)


def near_boundary(ids, radius=1):
    """True where some pixel within ``radius`` (Chebyshev) carries another ID."""
    H, W = ids.shape
    pad = np.pad(ids.astype(np.int32), radius, mode="edge")
    out = np.zeros((H, W), bool)
    for a in range(-radius, radius + 1):
        for b in range(-radius, radius + 1):
            out |= pad[radius + a:radius + a + H, radius + b:radius + b + W] != ids
    return out
