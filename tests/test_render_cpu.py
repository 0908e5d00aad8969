"""CPU: what the MJCF compiler keeps about appearance, cabi's render structs against include/mgx.h,
and tests/render_reference.py (the numpy reference the GPU render tests compare with) pinned by
hand on the closed-form scenes of tests/render_scenes.py.
"""
import ctypes as C
import hashlib
import importlib
import json
import os
import subprocess

import numpy as np
import pytest

from mujoco_gymnasium_environments_amd import cabi, mjcf
from tests import ray_reference as rr
from tests import render_reference as ref
from tests import render_scenes as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOADERS = {"soccer": "soccer_model", "parkour": "parkour_model", "bipedal": "bipedal_model", "dancing": "dancing_model",
           "martial": "martial_model", "assembly": "assembly_model", "construction": "construction_model"}


def _model(task):
    return getattr(importlib.import_module(f"mujoco_gymnasium_environments_amd.envs.{task}"), LOADERS[task])()


# ---------------------------------------------------------------- C-ABI
def test_header_matches_ctypes(tmp_path):
    """Size and every field offset of mgx_render_desc, and the render constants, of include/mgx.h
    against cabi.py; the ABI version is unchanged (the section only adds)."""
    fields = [n for n, _ in cabi.MgxRenderDesc._fields_]
    offs = "".join(f' printf("%zu ", offsetof(mgx_render_desc, {f}));' for f in fields)
    prog = tmp_path / "render.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mgx.h"\n'
                    'int main(void){printf("%zu ", sizeof(mgx_render_desc));' + offs +
                    ' printf("%d %d %d %d %d %d %d %d %d %d\\n", MGX_RENDER_MAX_LAYERS, MGX_RENDER_MAX_LIGHT, MGX_TEX_2D,'
                    ' MGX_TEX_CUBE, MGX_TEX_SKYBOX, MGX_BUILTIN_NONE, MGX_BUILTIN_GRADIENT, MGX_BUILTIN_CHECKER,'
                    ' MGX_BUILTIN_FLAT, MGX_ABI_VERSION); return 0;}\n')
    exe = tmp_path / "render"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    vals = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = [C.sizeof(cabi.MgxRenderDesc)] + [getattr(cabi.MgxRenderDesc, f).offset for f in fields]
    assert vals == want + [cabi.MGX_RENDER_MAX_LAYERS, cabi.MGX_RENDER_MAX_LIGHT, cabi.MGX_TEX_2D, cabi.MGX_TEX_CUBE,
                           cabi.MGX_TEX_SKYBOX, cabi.MGX_BUILTIN_NONE, cabi.MGX_BUILTIN_GRADIENT,
                           cabi.MGX_BUILTIN_CHECKER, cabi.MGX_BUILTIN_FLAT, 6]
    assert cabi.MGX_ABI_VERSION == 6 and ref.MAX_LAYERS == cabi.MGX_RENDER_MAX_LAYERS
    assert mjcf.TEX_TYPES == {"2d": cabi.MGX_TEX_2D, "cube": cabi.MGX_TEX_CUBE, "skybox": cabi.MGX_TEX_SKYBOX}
    assert mjcf.TEX_BUILTIN == {"none": 0, "gradient": 1, "checker": 2, "flat": 3}
    from mujoco_gymnasium_environments_amd import native
    for name in ("mgx_render_configure", "mgx_render_scene_bytes", "mgx_render_scene", "mgx_render_camera"):
        assert name in native.EXPORTS
    assert "mgx_render.hip" in native.SOURCES
    # the packed descriptor points at what the model says
    m = _model("assembly")
    p = cabi.PackedRender(m)
    assert (p.desc.ngeom, p.desc.nmat, p.desc.ntex, p.desc.nlight) == (m.ngeom, len(m.mat_names), 1, 2)
    assert p.desc.skybox_tex == -1 and list(p.desc.headlight_ambient) == [0.3] * 3
    np.testing.assert_array_equal(p.arrays["geom_rgba"].reshape(-1, 4), m.geom_rgba_eff)


# ---------------------------------------------------------------- compiler pins (read off the XML)
def test_construction_lights():
    m = _model("construction")
    assert len(m.light_names) == 3 and list(m.light_directional) == [1, 1, 1] and list(m.light_bodyid) == [0, 0, 0]
    s = np.sqrt(1.25)
    np.testing.assert_allclose(m.light_dir, [[0, 0, -1], [1 / s, 0, -0.5 / s], [-1 / s, 0, -0.5 / s]], atol=1e-15)
    np.testing.assert_allclose(np.linalg.norm(m.light_dir, axis=1), 1.0, atol=1e-15)
    np.testing.assert_array_equal(m.light_diffuse, [[1, 1, 1], [0.8] * 3, [0.8] * 3])
    np.testing.assert_array_equal(m.light_specular, [[0.5] * 3, [0.3] * 3, [0.3] * 3])
    np.testing.assert_array_equal(m.light_cutoff, [100, 50, 50])
    assert list(m.light_exponent) == [1, 10, 10] and list(m.light_castshadow) == [1, 1, 1]
    assert list(m.light_mode) == [mjcf.CAM_FIXED] * 3 and list(m.light_active) == [1, 1, 1]
    np.testing.assert_array_equal(m.light_ambient, np.zeros((3, 3)))
    np.testing.assert_array_equal(m.light_attenuation, [[1, 0, 0]] * 3)
    np.testing.assert_array_equal(m.light_pos, [[0, 0, 30], [-20, 0, 20], [20, 0, 20]])
    # headlight defaults
    assert list(m.headlight_ambient) == [0.1] * 3 and list(m.headlight_diffuse) == [0.4] * 3
    assert list(m.headlight_specular) == [0.5] * 3 and int(m.headlight_active[0]) == 1
    # a material with rgba and shininess only; the effective rgba of a geom with that material and no own rgba
    i = m.mat_names.index("steel")
    assert list(m.mat_rgba[i]) == [0.8, 0.8, 0.9, 1] and m.mat_shininess[i] == 0.8 and m.mat_specular[i] == 0.9
    assert m.mat_emission[i] == 0 and m.mat_texid[i] == -1 and list(m.mat_texrepeat[i]) == [1, 1]
    j = m.mat_names.index("geom")
    assert m.mat_texuniform[j] == 1 and m.tex_names[m.mat_texid[j]] == "texgeom"


def test_assembly_spots_headlight_and_translucent_marker():
    m = _model("assembly")
    assert m.light_names == ["spotlight1", "spotlight2"] and list(m.light_directional) == [0, 0]
    np.testing.assert_array_equal(m.light_cutoff, [45, 45])
    s = np.sqrt(1.5)
    np.testing.assert_allclose(m.light_dir, [[-0.5 / s, -0.5 / s, -1 / s], [0.5 / s, 0.5 / s, -1 / s]], atol=1e-15)
    np.testing.assert_array_equal(m.light_exponent, [10, 10])
    assert list(m.headlight_ambient) == [0.3] * 3 and list(m.headlight_diffuse) == [0.5] * 3
    assert list(m.headlight_specular) == [0, 0, 0]
    i = m.mat_names.index("marker_yellow")
    assert list(m.mat_rgba[i]) == [1, 1, 0, 0.5]   # metallic / roughness are read and ignored
    assert m.mat_specular[i] == 0.5 and m.mat_shininess[i] == 0.5
    # the asset's main default class gives every geom rgba 0.7 0.7 0.7 1: by the effective-colour rule
    # that attribute is present on every geom, so it wins over the geom's material
    g = m.geom_names.index("base_plate")
    assert m.mat_names[m.geom_matid[g]] == "joint_black" and list(m.geom_rgba_eff[g]) == [0.7, 0.7, 0.7, 1]
    assert (m.geom_matid >= 0).sum() > 20 and all((n >= 0) == bool(s) for n, s in zip(m.geom_matid, m.geom_material))
    # martial arts: no rgba in the defaults, so a geom with a material and no own rgba shows the material's
    t = _model("martial")
    for name, mat in (("floor", "grid"), ("training_mat", "mat")):
        g = t.geom_names.index(name)
        assert t.mat_names[t.geom_matid[g]] == mat and list(t.geom_rgba_eff[g]) == [1, 1, 1, 1]
        assert list(t.geom_rgba[g]) == [0.5, 0.5, 0.5, 1]
    i = t.mat_names.index("grid")
    assert (t.mat_specular[i], t.mat_shininess[i], list(t.mat_texrepeat[i])) == (0.3, 0.3, [10, 10])
    assert list(t.headlight_specular) == [0.1] * 3 and len(t.light_names) == 0


def test_bipedal_coloured_point_lights():
    m = _model("bipedal")
    assert m.light_names == ["emergency_light1", "emergency_light2", "searchlight"]
    assert list(m.light_directional) == [0, 0, 0]
    np.testing.assert_array_equal(m.light_diffuse, [[1, 0.2, 0.2], [1, 0.5, 0], [0.8] * 3])
    np.testing.assert_array_equal(m.light_specular, [[0.5, 0.1, 0.1], [0.5, 0.2, 0], [0.3] * 3])
    np.testing.assert_array_equal(m.light_pos, [[20, 0, 5], [-10, 5, 4], [0, 0, 10]])
    np.testing.assert_array_equal(m.light_cutoff, [45] * 3)


def test_parkour_checker_floor_and_sky():
    m = _model("parkour")
    i = m.mat_names.index("MatPlane")
    t = int(m.mat_texid[i])
    assert list(m.mat_texrepeat[i]) == [60, 60] and m.tex_names[t] == "texplane"
    assert m.tex_builtin[t] == mjcf.TEX_BUILTIN["checker"] and m.tex_type[t] == mjcf.TEX_TYPES["2d"]
    assert list(m.tex_rgb1[t]) == [0, 0, 0] and list(m.tex_rgb2[t]) == [0.8] * 3
    assert m.mat_specular[i] == 1 and m.mat_shininess[i] == 1     # reflectance is read and ignored
    sky = cabi.skybox_texture(m)
    assert sky == 0 and m.tex_builtin[sky] == mjcf.TEX_BUILTIN["gradient"]
    assert list(m.tex_rgb1[sky]) == [1, 1, 1] and list(m.tex_rgb2[sky]) == [0, 0, 0]
    assert not m.tex_file.any()
    # the soccer torso carries a light: it moves with the body
    s = _model("soccer")
    assert list(s.light_bodyid) == [0, s.body_names.index("torso")] and list(s.light_dir[1]) == [0, 0, -1]


def test_effective_rgba_rule_and_file_textures():
    m = mjcf.compile_xml("""<mujoco><default><default class="blue"><geom rgba="0 0 1 1"/></default></default>
<asset><texture name="wood" type="2d" file="wood.png"/><texture name="flat" type="2d" builtin="flat" rgb1="1 0 0"/>
 <material name="red" rgba="1 0 0 0.25" emission="0.3" texture="flat" texrepeat="2 3" texuniform="true"/>
 <material name="planks" texture="wood"/></asset>
<worldbody><light name="lamp" mode="track" pos="1 2 3" dir="0 3 -4" castshadow="false" active="false" cutoff="30"/>
 <geom name="a" type="sphere" size="1" material="red"/><geom name="b" type="sphere" size="1" material="red" rgba="0 1 0 1"/>
 <geom name="c" type="sphere" size="1"/><geom name="d" type="sphere" size="1" class="blue" material="red"/>
 <geom name="e" type="sphere" size="1" material="planks"/></worldbody></mujoco>""")
    np.testing.assert_array_equal(m.geom_rgba_eff, [[1, 0, 0, 0.25], [0, 1, 0, 1], [0.5, 0.5, 0.5, 1], [0, 0, 1, 1],
                                                    [1, 1, 1, 1]])
    # geom_rgba itself stays what it was: the ray code's elimination rule reads it
    np.testing.assert_array_equal(m.geom_rgba[0], [0.5, 0.5, 0.5, 1])
    assert list(m.geom_matid) == [0, 0, -1, 0, 1]
    assert list(m.tex_file) == [1, 0] and m.mat_emission[0] == 0.3 and m.mat_texuniform[0] == 1
    assert list(m.mat_texrepeat[0]) == [2, 3] and list(m.tex_rgb2[1]) == [0.5] * 3
    assert m.light_names == ["lamp"] and m.light_mode[0] == mjcf.CAM_TRACK
    assert (m.light_castshadow[0], m.light_active[0], m.light_directional[0]) == (0, 0, 0)
    np.testing.assert_allclose(m.light_dir[0], [0, 0.6, -0.8], atol=1e-15)
    assert list(m.light_diffuse[0]) == [0.7] * 3 and list(m.light_specular[0]) == [0.3] * 3


def test_no_physics_field_changed():
    """Every field mgx_model_create reads, and geom_rgba, hashed per model before the appearance
    fields were added (tests/golden/render_pack_model_sha256.json)."""
    with open(os.path.join(ROOT, "tests", "golden", "render_pack_model_sha256.json")) as f:
        want = json.load(f)
    assert sorted(want) == sorted(LOADERS)
    for task in LOADERS:
        model = _model(task)
        p = cabi.pack_model(model)
        h = hashlib.sha256()
        for n in cabi._INT_SIZES:
            h.update(n.encode() + repr(int(getattr(p.desc, n))).encode())
        for n in cabi._REAL_SCALARS:
            h.update(n.encode() + float(getattr(p.desc, n)).hex().encode())
        h.update(bytes(bytearray(C.string_at(C.addressof(p.desc.gravity), 24))))
        for n, _ in cabi._ARRAYS:
            h.update(n.encode() + p.arrays[n].tobytes())
        h.update(model.geom_rgba.tobytes())
        assert h.hexdigest() == want[task], task


# ---------------------------------------------------------------- the reference, pinned by hand
def test_piece_routine_gives_the_ray_reference_distances():
    rng = np.random.default_rng(3)
    p = rng.uniform(-2, 2, (400, 3))
    pos, q = rng.uniform(-0.3, 0.3, 3), rng.normal(size=4)
    v = pos + rng.normal(0, 0.5, (400, 3)) - p        # aimed near the geom, some from inside it
    mat = mjcf.quat2mat(q / np.linalg.norm(q))
    for gtype, size in ((rr.PLANE, [1.0, 0, 0.1]), (rr.SPHERE, [0.7, 0, 0]), (rr.CAPSULE, [0.3, 0.6, 0]),
                        (rr.CYLINDER, [0.4, 0.5, 0]), (rr.BOX, [0.5, 0.3, 0.8])):
        x, piece = ref.ray_geom_piece(gtype, size, pos, mat, p, v)
        np.testing.assert_array_equal(x, rr.ray_geom(gtype, size, pos, mat, p, v))
        hit = np.isfinite(x)
        assert hit.sum() > 20
        hp = (p[hit] + x[hit, None] * v[hit] - pos) @ mat
        n = ref._normal(gtype, piece[hit], np.asarray(size), hp)
        np.testing.assert_allclose(np.linalg.norm(n, axis=1), 1.0, atol=1e-12)
        if gtype == rr.BOX:      # the face a hit lies on is the one its piece names
            ax, sg = piece[hit] // 2, np.where(piece[hit] % 2 == 1, 1.0, -1.0)
            np.testing.assert_allclose(hp[np.arange(hit.sum()), ax], sg * np.asarray(size)[ax], atol=1e-12)
        if gtype == rr.CYLINDER:
            cap = piece[hit] > 0
            assert cap.any() and (~cap).any()
            np.testing.assert_allclose(np.abs(hp[cap, 2]), size[1], atol=1e-12)
            np.testing.assert_allclose(np.hypot(hp[~cap, 0], hp[~cap, 1]), size[0], atol=1e-12)
        if gtype == rr.CAPSULE:
            assert set(np.unique(piece[hit])) == {0, 1, 2}
            assert (np.abs(hp[piece[hit] == 0, 2]) <= size[1] + 1e-12).all()


@pytest.mark.parametrize("name", list(rs.SCENES))
def test_reference_on_closed_form_scenes(name):
    model, pins = rs.scene(name)
    poses = rs.static_poses(model)
    images = {}
    for cam, r, c, want in pins:
        assert (want >= 0).all() and (want <= 1).all()
        if cam not in images:
            images[cam] = ref.render(model, poses, model.cam_names.index(cam), rs.H, rs.W)
        img = images[cam]
        np.testing.assert_allclose(img["rgbf"][r, c], want, atol=1e-12, err_msg=f"{name} {cam} ({r}, {c})")
        np.testing.assert_array_equal(img["rgb8"][r, c], ref.quantise(want))


def test_reference_discrete_structure():
    """What the closed forms do not show: the sky pixel is a miss (depth inf, seg -1), the shadow
    pixel's shadow flag is set, the checker parity flips across the cell edge, the plate pixel has two
    layers, and `decided` leaves out a pixel on a silhouette."""
    model, pins = rs.scene("sky")
    img = ref.render(model, rs.static_poses(model), 0, rs.H, rs.W)
    assert img["seg"][0, 0] == -1 and np.isinf(img["depth"][0, 0]) and img["seg"][4, 4] == 0
    assert img["depth"][4, 4] == 5.0
    model, pins = rs.scene("sun_ball")
    poses = rs.static_poses(model)
    img = ref.render(model, poses, model.cam_names.index("aside"), rs.H, rs.W)
    per = 3 + 2 * 1
    (_, r, c, _), (_, r2, c2, _) = pins[1], pins[2]
    assert img["choices"][r * rs.W + c, 3] == 1 and img["choices"][r2 * rs.W + c2, 3] == 0
    assert img["seg"][r, c] == model.geom_names.index("floor")
    model, pins = rs.scene("checker")
    img = ref.render(model, rs.static_poses(model), 0, rs.H, rs.W)
    assert img["choices"][3 * rs.W + 5, 2] == 0 and img["choices"][3 * rs.W + 7, 2] == 1
    model, pins = rs.scene("plate")
    img = ref.render(model, rs.static_poses(model), 0, rs.H, rs.W)
    ch = img["choices"][4 * rs.W + 4]
    assert ch[0] == model.geom_names.index("plate") and ch[1] == 5 and ch[per] == model.geom_names.index("floor")
    assert ch[2 * per] == -2
    # a ball whose silhouette passes through a pixel centre: that pixel is undecided at a coarse delta
    model, _ = rs.scene("sun_ball")
    img, ok = ref.decided(model, poses, 0, 64, 64, 2e-2)
    assert 0 < (~ok).sum() < 0.2 * ok.size
    _, ok6 = ref.decided(model, poses, 0, rs.H, rs.W, 1e-6)
    assert ok6.all()
