"""Reference ray caster (TEST INFRASTRUCTURE ONLY): pure numpy float64, vectorised over rays.

Semantics (MuJoCo's mj_ray [ext], restated in include/mgx.h and DESIGN.md "Ray casting"): a ray
is p + x v with x >= 0, v not normalised, x in units of |v|. In the geom frame lp = R'(p - pos),
lv = R'v, the result for one geom is the smallest x >= 0 over the pieces of its surface, each
accepted only inside its own extent; a ray that starts inside a closed geom hits its exit surface.
"""
import numpy as np

PLANE, HFIELD, SPHERE, CAPSULE, ELLIPSOID, CYLINDER, BOX = range(7)
MINVAL = 1e-15
CAM_FIXED, CAM_TRACK, CAM_TRACKCOM = 0, 1, 2


def _quad(a, b, c):
    """Both roots of a x^2 + 2 b x + c = 0 per ray; nan where there is none (a or the
    discriminant under MINVAL, as mju ray_quad)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        det = b * b - a * c
        ok = (a >= MINVAL) & (det >= MINVAL)
        s = np.sqrt(np.where(ok, det, 0.0))
        safe = np.where(ok, a, 1.0)
        return np.where(ok, (-b - s) / safe, np.nan), np.where(ok, (-b + s) / safe, np.nan)


def _take(best, x, ok):
    """min(best, x) where x is a valid candidate: finite, x >= 0 and accepted."""
    with np.errstate(invalid="ignore"):
        good = ok & np.isfinite(x) & (x >= 0) & (x < best)
    return np.where(good, x, best)


def ray_geom(gtype, size, pos, mat, p, v):
    """Distance of rays (p, v) [R, 3] to one geom with world pose (pos [3], mat [3, 3]); inf = no hit."""
    size = np.asarray(size, dtype=np.float64)
    mat = np.asarray(mat, dtype=np.float64).reshape(3, 3)
    lp = (np.asarray(p, dtype=np.float64) - np.asarray(pos, dtype=np.float64)) @ mat   # rows: R'(p - pos)
    lv = np.asarray(v, dtype=np.float64) @ mat
    best = np.full(lp.shape[0], np.inf)

    def at(x, k):
        return lp[:, k] + x * lv[:, k]

    with np.errstate(invalid="ignore", divide="ignore"):
        if gtype == PLANE:
            front = lv[:, 2] < -MINVAL
            x = np.where(front, -lp[:, 2] / np.where(front, lv[:, 2], 1.0), np.nan)
            ok = front
            if size[0] > 0:
                ok = ok & (np.abs(at(x, 0)) <= size[0])
            if size[1] > 0:
                ok = ok & (np.abs(at(x, 1)) <= size[1])
            best = _take(best, x, ok)
        elif gtype == SPHERE:
            for x in _quad((lv * lv).sum(1), (lv * lp).sum(1), (lp * lp).sum(1) - size[0] ** 2):
                best = _take(best, x, True)
        elif gtype in (CAPSULE, CYLINDER):
            r, h = size[0], size[1]
            # side: |z| <= h
            for x in _quad(lv[:, 0] ** 2 + lv[:, 1] ** 2, lv[:, 0] * lp[:, 0] + lv[:, 1] * lp[:, 1],
                           lp[:, 0] ** 2 + lp[:, 1] ** 2 - r * r):
                best = _take(best, x, np.abs(at(x, 2)) <= h)
            for s in (-1.0, 1.0):
                if gtype == CAPSULE:   # cap sphere at z = s h, accepted where s z >= h
                    c = lp - np.array([0.0, 0.0, s * h])
                    for x in _quad((lv * lv).sum(1), (lv * c).sum(1), (c * c).sum(1) - r * r):
                        best = _take(best, x, s * at(x, 2) >= h)
                else:                  # flat cap at z = s h, accepted inside the disc
                    par = np.abs(lv[:, 2]) > MINVAL
                    x = np.where(par, (s * h - lp[:, 2]) / np.where(par, lv[:, 2], 1.0), np.nan)
                    best = _take(best, x, par & (at(x, 0) ** 2 + at(x, 1) ** 2 <= r * r))
        elif gtype == BOX:
            for i in range(3):
                j, k = (i + 1) % 3, (i + 2) % 3
                par = np.abs(lv[:, i]) > MINVAL
                for s in (-1.0, 1.0):   # face i = s size[i], accepted inside the other two extents
                    x = np.where(par, (s * size[i] - lp[:, i]) / np.where(par, lv[:, i], 1.0), np.nan)
                    best = _take(best, x, par & (np.abs(at(x, j)) <= size[j]) & (np.abs(at(x, k)) <= size[k]))
        else:
            raise ValueError(f"geom type {gtype} is not supported by ray casting")
    return best


def default_enable(model):
    """Geoms mj_ray eliminates by default: alpha exactly 0 and no material."""
    alpha = np.asarray(model.geom_rgba).reshape(-1, 4)[:, 3]
    mat = np.array([bool(n) for n in model.geom_material], dtype=bool)
    return ~((alpha == 0) & ~mat)


def ray_scene(model, geom_xpos, geom_xmat, p, v, enable=None, bodyexclude=-1, scale=1.0):
    """Nearest hit over the enabled geoms: (dist [R], geomid [R]); a miss is (-1, -1). ``enable``
    is an optional bool / uint8 [ngeom] mask on top of the default elimination; ``scale``
    multiplies every geom size (the decided-ray filter)."""
    ng = model.ngeom
    gx = np.asarray(geom_xpos, dtype=np.float64).reshape(ng, 3)
    gm = np.asarray(geom_xmat, dtype=np.float64).reshape(ng, 3, 3)
    on = default_enable(model)
    if enable is not None:
        on = on & (np.asarray(enable).reshape(-1) != 0)
    if bodyexclude >= 0:
        on = on & (np.asarray(model.geom_bodyid) != bodyexclude)
    p = np.asarray(p, dtype=np.float64).reshape(-1, 3)
    v = np.asarray(v, dtype=np.float64).reshape(-1, 3)
    best = np.full(p.shape[0], np.inf)
    gid = np.full(p.shape[0], -1, dtype=np.int32)
    for g in range(ng):
        if not on[g]:
            continue
        x = ray_geom(int(model.geom_type[g]), np.asarray(model.geom_size[g]) * scale, gx[g], gm[g], p, v)
        closer = x < best          # strict: ties keep the lower geom id
        best = np.where(closer, x, best)
        gid = np.where(closer, g, gid).astype(np.int32)
    return np.where(gid >= 0, best, -1.0), gid


def decided(model, geom_xpos, geom_xmat, p, v, delta, **kw):
    """(dist, geomid, decided [R] bool): a ray is decided when the winning geom (a miss counting
    as -1) is the same with every geom size scaled by 1, 1 - delta and 1 + delta."""
    d, g = ray_scene(model, geom_xpos, geom_xmat, p, v, **kw)
    _, g_lo = ray_scene(model, geom_xpos, geom_xmat, p, v, scale=1.0 - delta, **kw)
    _, g_hi = ray_scene(model, geom_xpos, geom_xmat, p, v, scale=1.0 + delta, **kw)
    return d, g, (g == g_lo) & (g == g_hi)


def camera_pose(model, cam, xpos, xmat, subtree_com):
    """World position [3] and orientation [3, 3] of camera ``cam`` (mj_camlight [ext])."""
    b = int(model.cam_bodyid[cam])
    xpos = np.asarray(xpos, dtype=np.float64).reshape(-1, 3)
    xmat = np.asarray(xmat, dtype=np.float64).reshape(-1, 3, 3)
    com = np.asarray(subtree_com, dtype=np.float64).reshape(-1, 3)
    mode = int(model.cam_mode[cam])
    if mode == CAM_FIXED:
        q = np.asarray(model.cam_quat[cam], dtype=np.float64)
        w, x, y, z = q / np.linalg.norm(q)
        rel = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                        [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                        [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
        return xpos[b] + xmat[b] @ np.asarray(model.cam_pos[cam]), xmat[b] @ rel
    mat0 = np.asarray(model.cam_mat0[cam], dtype=np.float64).reshape(3, 3)
    if mode == CAM_TRACK:
        return xpos[b] + np.asarray(model.cam_pos0[cam]), mat0
    if mode == CAM_TRACKCOM:
        return com[b] + np.asarray(model.cam_poscom0[cam]), mat0
    raise ValueError(f"camera mode {mode} is not supported")


def camera_rays(pos, mat, fovy_deg, height, width):
    """Pixel rays, row-major from the top-left: p [H W, 3] (the camera position) and
    v = R_cam ((2 (c + 1/2) / W - 1) t W / H, (1 - 2 (r + 1/2) / H) t, -1), t = tan(fovy / 2)."""
    t = np.tan(np.deg2rad(fovy_deg) / 2)
    r, c = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
    vc = np.stack([(2 * (c + 0.5) / width - 1) * t * width / height, (1 - 2 * (r + 0.5) / height) * t,
                   -np.ones_like(r, dtype=np.float64)], axis=-1).reshape(-1, 3)
    v = vc @ np.asarray(mat, dtype=np.float64).reshape(3, 3).T
    return np.tile(np.asarray(pos, dtype=np.float64), (v.shape[0], 1)), v
