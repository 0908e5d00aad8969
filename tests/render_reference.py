"""Reference renderer (TEST INFRASTRUCTURE ONLY): the shading model of include/mgx.h "RGB camera
images"  restated in numpy float64, vectorised over pixels.

It builds on tests/ray_reference.py for the camera pose and the pixel rays; the ray-geom routine is
restated here because shading needs the surface PIECE whose root won (``ray_geom_piece`` gives the
same distances as ``ray_reference.ray_geom``, which tests/test_render_cpu.py checks).

``render`` also returns every discrete choice it made per pixel (hit geom and piece per layer,
checker parity, per light the shadow flag and the spot inside / outside), so that ``decided`` can
leave out the pixels where rounding may flip one.
"""
import numpy as np

from tests import ray_reference as rr

PLANE, SPHERE, CAPSULE, CYLINDER, BOX = rr.PLANE, rr.SPHERE, rr.CAPSULE, rr.CYLINDER, rr.BOX
MINVAL = rr.MINVAL
MAX_LAYERS = 4
TEX_SKYBOX = 2
BUILTIN_NONE, BUILTIN_GRADIENT, BUILTIN_CHECKER, BUILTIN_FLAT = range(4)


def _take(best, piece, x, ok, k):
    with np.errstate(invalid="ignore"):
        good = ok & np.isfinite(x) & (x >= 0) & (x < best)
    return np.where(good, x, best), np.where(good, k, piece)


def ray_geom_piece(gtype, size, pos, mat, p, v):
    """(dist [R], piece [R]) of rays against one geom; inf = no hit. Pieces: 0 = plane, sphere, the
    side of a capsule / cylinder; 1 / 2 = the -z / +z cap; box faces 2 i + (s > 0). Ties keep the
    first piece tried (side, -z, +z; -x +x -y +y -z +z)."""
    size = np.asarray(size, dtype=np.float64)
    mat = np.asarray(mat, dtype=np.float64).reshape(3, 3)
    lp = (np.asarray(p, dtype=np.float64) - np.asarray(pos, dtype=np.float64)) @ mat
    lv = np.asarray(v, dtype=np.float64) @ mat
    best = np.full(lp.shape[0], np.inf)
    piece = np.zeros(lp.shape[0], dtype=np.int64)

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
            best, piece = _take(best, piece, x, ok, 0)
        elif gtype == SPHERE:
            for x in rr._quad((lv * lv).sum(1), (lv * lp).sum(1), (lp * lp).sum(1) - size[0] ** 2):
                best, piece = _take(best, piece, x, True, 0)
        elif gtype in (CAPSULE, CYLINDER):
            r, h = size[0], size[1]
            for x in rr._quad(lv[:, 0] ** 2 + lv[:, 1] ** 2, lv[:, 0] * lp[:, 0] + lv[:, 1] * lp[:, 1],
                              lp[:, 0] ** 2 + lp[:, 1] ** 2 - r * r):
                best, piece = _take(best, piece, x, np.abs(at(x, 2)) <= h, 0)
            for s, k in ((-1.0, 1), (1.0, 2)):
                if gtype == CAPSULE:
                    c = lp - np.array([0.0, 0.0, s * h])
                    for x in rr._quad((lv * lv).sum(1), (lv * c).sum(1), (c * c).sum(1) - r * r):
                        best, piece = _take(best, piece, x, s * at(x, 2) >= h, k)
                else:
                    par = np.abs(lv[:, 2]) > MINVAL
                    x = np.where(par, (s * h - lp[:, 2]) / np.where(par, lv[:, 2], 1.0), np.nan)
                    best, piece = _take(best, piece, x, par & (at(x, 0) ** 2 + at(x, 1) ** 2 <= r * r), k)
        elif gtype == BOX:
            for i in range(3):
                j, k = (i + 1) % 3, (i + 2) % 3
                par = np.abs(lv[:, i]) > MINVAL
                for s in (-1.0, 1.0):
                    x = np.where(par, (s * size[i] - lp[:, i]) / np.where(par, lv[:, i], 1.0), np.nan)
                    best, piece = _take(best, piece, x,
                                        par & (np.abs(at(x, j)) <= size[j]) & (np.abs(at(x, k)) <= size[k]),
                                        2 * i + (s > 0))
        else:
            raise ValueError(f"geom type {gtype} is not supported by ray casting")
    return best, piece


def _normal(gtype, piece, size, hp):
    """Outward unit normal [R, 3] in the geom frame at the geom-frame hit points hp."""
    n = np.zeros_like(hp)
    if gtype == PLANE:
        n[:, 2] = 1.0
    elif gtype == SPHERE:
        n = hp.copy()
    elif gtype == CAPSULE:
        n[:, :2] = hp[:, :2]
        n[:, 2] = np.where(piece == 0, 0.0, np.where(piece == 1, hp[:, 2] + size[1], hp[:, 2] - size[1]))
    elif gtype == CYLINDER:
        side = piece == 0
        n[:, 0], n[:, 1] = np.where(side, hp[:, 0], 0.0), np.where(side, hp[:, 1], 0.0)
        n[:, 2] = np.where(side, 0.0, np.where(piece == 1, -1.0, 1.0))
    elif gtype == BOX:
        n[np.arange(len(piece)), piece // 2] = np.where(piece % 2 == 1, 1.0, -1.0)
    return n / np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-300)


class Scene:
    """One env's geometry and appearance, from a compiled model and its poses."""

    def __init__(self, model, poses, enable=None, bodyexclude=-1, scale=1.0):
        m, ng = model, model.ngeom
        self.model, self.scale = m, scale
        self.gx = np.asarray(poses["geom_xpos"], dtype=np.float64).reshape(ng, 3)
        self.gm = np.asarray(poses["geom_xmat"], dtype=np.float64).reshape(ng, 3, 3)
        on = rr.default_enable(m)
        if enable is not None:
            on = on & (np.asarray(enable).reshape(-1) != 0)
        if bodyexclude >= 0:
            on = on & (np.asarray(m.geom_bodyid) != bodyexclude)
        self.on = on
        self.rgba = np.asarray(m.geom_rgba_eff, dtype=np.float64).reshape(ng, 4)
        self.shadow_on = on & (self.rgba[:, 3] == 1.0)
        xpos = np.asarray(poses["xpos"], dtype=np.float64).reshape(-1, 3)
        xmat = np.asarray(poses["xmat"], dtype=np.float64).reshape(-1, 3, 3)
        nl = len(m.light_names)
        self.light_pos = np.array([xpos[b] + xmat[b] @ m.light_pos[l] for l, b in enumerate(m.light_bodyid)]).reshape(nl, 3)
        self.light_dir = np.array([xmat[b] @ m.light_dir[l] for l, b in enumerate(m.light_bodyid)]).reshape(nl, 3)
        # per geom: colours of the two checker cells (equal without a checker), cell edges, material scalars
        self.c0, self.c1, self.cell = np.zeros((ng, 3)), np.zeros((ng, 3)), np.zeros((ng, 2))
        self.emission, self.ks, self.shin = np.zeros(ng), np.full(ng, 0.5), np.full(ng, 64.0)
        for g in range(ng):
            t0 = t1 = np.ones(3)
            mt = int(m.geom_matid[g])
            if mt >= 0:
                self.emission[g], self.ks[g] = m.mat_emission[mt], m.mat_specular[mt]
                self.shin[g] = 128.0 * m.mat_shininess[mt]
                tx = int(m.mat_texid[mt])
                if tx >= 0 and m.tex_builtin[tx] != BUILTIN_NONE:
                    if m.tex_builtin[tx] == BUILTIN_FLAT:
                        t0 = t1 = m.tex_rgb1[tx]
                    elif m.tex_builtin[tx] == BUILTIN_CHECKER and m.geom_type[g] == PLANE:
                        t0, t1 = m.tex_rgb1[tx], m.tex_rgb2[tx]
                        for k in range(2):
                            rep, sz = m.mat_texrepeat[mt][k], m.geom_size[g][k]
                            self.cell[g, k] = sz / rep if (sz > 0 and not m.mat_texuniform[mt]) else 1.0 / (2.0 * rep)
                    else:
                        t0 = t1 = 0.5 * (m.tex_rgb1[tx] + m.tex_rgb2[tx])
            self.c0[g], self.c1[g] = self.rgba[g, :3] * t0, self.rgba[g, :3] * t1
        sky = np.flatnonzero(np.asarray(m.tex_type) == TEX_SKYBOX)
        self.sky = int(sky[0]) if sky.size else -1

    def nearest(self, p, v, skip):
        """(dist, geomid, piece) of rays p + x v, geom ``skip[r]`` left out; a miss is (inf, -1, 0)."""
        m = self.model
        best = np.full(p.shape[0], np.inf)
        gid = np.full(p.shape[0], -1, dtype=np.int64)
        piece = np.zeros(p.shape[0], dtype=np.int64)
        for g in np.flatnonzero(self.on):
            x, pc = ray_geom_piece(int(m.geom_type[g]), np.asarray(m.geom_size[g]) * self.scale, self.gx[g], self.gm[g], p, v)
            closer = (x < best) & (skip != g)          # strict: ties keep the lower geom id
            best, gid, piece = np.where(closer, x, best), np.where(closer, g, gid), np.where(closer, pc, piece)
        return best, gid, piece

    def occluded(self, p, v, limit):
        """Does the ray p + x v meet a shadow caster (enabled, alpha exactly 1) at x < limit?"""
        m = self.model
        hit = np.zeros(p.shape[0], dtype=bool)
        for g in np.flatnonzero(self.shadow_on):
            x, _ = ray_geom_piece(int(m.geom_type[g]), np.asarray(m.geom_size[g]) * self.scale, self.gx[g], self.gm[g], p, v)
            hit |= x < limit
        return hit

    def background(self, dhat):
        m = self.model
        if self.sky >= 0 and m.tex_builtin[self.sky] == BUILTIN_GRADIENT:
            f = 0.5 + 0.5 * dhat[:, 2:3]
            return m.tex_rgb2[self.sky] + (m.tex_rgb1[self.sky] - m.tex_rgb2[self.sky]) * f
        if self.sky >= 0 and m.tex_builtin[self.sky] == BUILTIN_FLAT:
            return np.tile(np.asarray(m.tex_rgb1[self.sky], dtype=np.float64), (dhat.shape[0], 1))
        return np.zeros_like(dhat)


GATE_EPS = 1e-5     # float32 shading: n.L within this of 0 may take either side of [n.L > 0]
GATE_JUMP = 1e-6    # ... which matters only where the gated specular term is larger than this


def _blinn_phong(c, n, L, dhat, diffuse, specular, ks, shin, w, delta):
    """w [c diffuse max(0, n.L) + k_s specular max(0, n.H)^shin [n.L > 0]] and whether the gate
    [n.L > 0] is safe: n.L is away from 0, or the specular term it switches is negligible."""
    ndl = (n * L).sum(1)
    H = L - dhat
    H = H / np.maximum(np.linalg.norm(H, axis=1, keepdims=True), 1e-300)
    with np.errstate(invalid="ignore"):
        sp = ks * np.maximum((n * H).sum(1), 0.0) ** shin
    lit = ndl > 0
    jump = w * sp * np.max(specular)
    safe = (np.abs(ndl) > max(delta, GATE_EPS)) | (jump <= GATE_JUMP)
    return w[:, None] * np.where(lit[:, None], c * diffuse * ndl[:, None] + sp[:, None] * specular, 0.0), safe


def _shade(sc, gid, piece, x, o, v, cam_pos, cam_mat, dhat, delta):
    """Colour [R, 3] of the hits, the choices made [R, 1 + 2 nlight] (checker parity; per light the
    shadow flag and the spot inside / outside) and whether the pixel is safe from the two choices that
    are not geometric [R]: the checker hit keeps its distance from every cell edge, and no light's
    gate [n.L > 0] switches a visible specular term at n.L = 0 (_blinn_phong)."""
    m = sc.model
    R, nl = len(gid), len(m.light_names)
    P = o + x[:, None] * v
    n, c = np.zeros((R, 3)), np.zeros((R, 3))
    parity, edge_ok = np.zeros(R, dtype=np.int64), np.ones(R, dtype=bool)
    for g in np.unique(gid):
        k = gid == g
        hp = (P[k] - sc.gx[g]) @ sc.gm[g]
        nloc = _normal(int(m.geom_type[g]), piece[k], np.asarray(m.geom_size[g]) * sc.scale, hp)
        n[k] = nloc @ sc.gm[g].T
        c[k] = sc.c0[g]
        if sc.cell[g, 0] > 0:
            q = hp[:, :2] / sc.cell[g]
            par = (np.floor(q[:, 0]) + np.floor(q[:, 1])) % 2 != 0
            c[k] = np.where(par[:, None], sc.c1[g], sc.c0[g])
            parity[k] = par
            near = np.abs(q - np.round(q)) * sc.cell[g] <= delta * np.maximum(1.0, np.abs(hp[:, :2]))
            edge_ok[k] = ~near.any(1)
    flip = (n * v).sum(1) > 0
    n[flip] = -n[flip]
    emission, ks, shin = sc.emission[gid][:, None], sc.ks[gid], sc.shin[gid]
    A = np.zeros(3)
    if m.headlight_active[0]:
        A = A + m.headlight_ambient
    for l in range(nl):
        if m.light_active[l]:
            A = A + m.light_ambient[l]
    C = c * (emission + A)
    if m.headlight_active[0]:
        headL = np.tile(cam_mat[:, 2], (R, 1))
        term, safe = _blinn_phong(c, n, headL, dhat, m.headlight_diffuse, m.headlight_specular, ks, shin, np.ones(R), delta)
        C, edge_ok = C + term, edge_ok & safe
    eps = 1e-4 * np.maximum(1.0, np.linalg.norm(P - cam_pos, axis=1))
    O = P + eps[:, None] * n
    choices = [parity]
    for l in range(nl):
        shadow, inside = np.zeros(R, dtype=np.int64), np.ones(R, dtype=np.int64)
        if m.light_active[l]:
            if m.light_directional[l]:
                L, w, limit = np.tile(-sc.light_dir[l], (R, 1)), np.ones(R), np.full(R, np.inf)
            else:
                Lv = sc.light_pos[l] - P
                limit = np.linalg.norm(Lv, axis=1)
                L = Lv / np.maximum(limit, MINVAL)[:, None]
                a = m.light_attenuation[l]
                w = 1.0 / (a[0] + a[1] * limit + a[2] * limit * limit)
                if m.light_cutoff[l] < 180.0:
                    ct = -(L * sc.light_dir[l]).sum(1)
                    ins = ct >= np.cos(np.deg2rad(m.light_cutoff[l]))
                    inside = ins.astype(np.int64)
                    w = np.where(ins, w * np.maximum(ct, 0.0) ** m.light_exponent[l], 0.0)
            if m.light_castshadow[l]:
                # cast for every pixel: where the light gives nothing anyway (outside the cone, facing
                # away) the flag changes no colour, and it must not depend on the sign of a rounded n.L
                occ = sc.occluded(O, L, limit)
                shadow = occ.astype(np.int64)
                w = np.where(occ, 0.0, w)
            term, safe = _blinn_phong(c, n, L, dhat, m.light_diffuse[l], m.light_specular[l], ks, shin, w, delta)
            C, edge_ok = C + term, edge_ok & safe
        choices += [shadow, inside]
    return C, np.stack(choices, axis=1), edge_ok


def render(model, poses, cam, height, width, enable=None, bodyexclude=-1, scale=1.0, delta=0.0):
    """One env's image from camera ``cam``: dict of rgbf [H, W, 3] float64 in [0, 1], rgb8 uint8,
    depth [H, W] (inf for a miss), seg [H, W], choices [H W, K] (every discrete choice made) and
    edge_ok [H W] (no checker hit within delta max(1, |u|) of a cell edge, no unsafe [n.L > 0] gate)."""
    sc = Scene(model, poses, enable, bodyexclude, scale)
    cam_pos, cam_mat = rr.camera_pose(model, cam, poses["xpos"], poses["xmat"], poses["subtree_com"])
    p, v = rr.camera_rays(cam_pos, cam_mat, float(model.cam_fovy[cam]), height, width)
    R, nl = p.shape[0], len(model.light_names)
    dhat = v / np.linalg.norm(v, axis=1, keepdims=True)
    out, weight = np.zeros((R, 3)), np.ones(R)
    live, o, skip = np.ones(R, dtype=bool), p.copy(), np.full(R, -1, dtype=np.int64)
    per_layer = 3 + 2 * nl
    choices = np.full((R, MAX_LAYERS * per_layer), -2, dtype=np.int64)
    edge_ok = np.ones(R, dtype=bool)
    depth = seg = None
    for layer in range(MAX_LAYERS):
        idx = np.flatnonzero(live)
        if idx.size == 0:
            break
        x, gid, piece = sc.nearest(o[idx], v[idx], skip[idx])
        if layer == 0:
            depth, seg = np.where(gid >= 0, x, np.inf), gid.copy()
        col = layer * per_layer
        choices[idx, col], choices[idx, col + 1] = gid, piece
        miss = gid < 0
        mi = idx[miss]
        out[mi] += weight[mi, None] * sc.background(dhat[mi])
        live[mi] = False
        hi = idx[~miss]
        if hi.size:
            C, ch, ok = _shade(sc, gid[~miss], piece[~miss], x[~miss], o[hi], v[hi], cam_pos, cam_mat, dhat[hi], delta)
            choices[hi, col + 2:col + per_layer] = ch
            edge_ok[hi] &= ok
            alpha = np.ones(hi.size) if layer == MAX_LAYERS - 1 else sc.rgba[gid[~miss], 3]
            out[hi] += (weight[hi] * alpha)[:, None] * C
            weight[hi] *= 1.0 - alpha
            live[hi[alpha >= 1.0]] = False
            o[hi] = o[hi] + x[~miss, None] * v[hi]
            skip[hi] = gid[~miss]
    rgbf = np.clip(out, 0.0, 1.0)
    return dict(rgbf=rgbf.reshape(height, width, 3), rgb8=quantise(rgbf).reshape(height, width, 3),
                depth=depth.reshape(height, width), seg=seg.reshape(height, width).astype(np.int32),
                choices=choices, edge_ok=edge_ok)


def quantise(rgbf):
    """rgb8 = (uint8)(rgbf 255 + 0.5)"""
    return np.floor(np.asarray(rgbf, dtype=np.float64) * 255.0 + 0.5).astype(np.uint8)


def decided(model, poses, cam, height, width, delta, **kw):
    """(image dict at scale 1, decided [H, W] bool): a pixel is decided when every discrete choice
    is the same with every geom size scaled by 1, 1 - delta and 1 + delta, no checker hit lies
    within delta max(1, |u|) of a cell edge, and no gate [n.L > 0] switches a visible specular term
    within rounding of n.L = 0 (a surface exactly tangent to a light)."""
    img = render(model, poses, cam, height, width, delta=delta, **kw)
    lo = render(model, poses, cam, height, width, scale=1.0 - delta, delta=delta, **kw)
    hi = render(model, poses, cam, height, width, scale=1.0 + delta, delta=delta, **kw)
    same = (img["choices"] == lo["choices"]).all(1) & (img["choices"] == hi["choices"]).all(1)
    return img, (same & img["edge_ok"]).reshape(height, width)
