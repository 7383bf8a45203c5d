"""The scenes tests/test_emissive_cpu.py and tests/test_emissive.py share: each recipe builds the scene with either API (conftest's
OracleApi / ProductApi) and `LAMPS` names the triangles that are its lamps.  A lamp's colour is a float vector (make_color takes
bytes), about (30, 30, 30).  A plain helper module."""
import numpy as np

import conftest as CT

F32 = np.float32
LAMP_COLOR = (30.0, 28.0, 26.0)


def solid_f32(api, color):
    """A Solid surface whose colour is the given floats, not make_color's bytes / 255"""
    c = np.asarray(color, F32)
    return api.m.Surface(api.m.SOLID, c) if api.kind == "oracle" else api.m.SurfaceKind.Solid(c)


def _quad(api, s, pts, surface, edge):
    a, b, c, d = (np.asarray(p, F32) for p in pts)
    api.add_triangle(s, np.array([a, b, c], F32), surface, edge)
    api.add_triangle(s, np.array([a, c, d], F32), surface, edge)


# Triangles 1, 2: the wall; 3, 4: the lamp; 5, 6: the occluder between the lamp and the wall; 7, 8: the screen in front of the lamp
WALL_LAMPS = (3, 4)


def recipe_wall_lamp(lamp_color=LAMP_COLOR, lamp_edge=0.05):
    """shadowed_ref.recipe_wall (a Matte wall at z = 6 + 0.05 x + 0.03 y that covers the canonical view) with a small bright Solid quad
    lamp at z ~ 2.5 up and to the right, a Matte occluder at z ~ 4.5 between the two, and a Matte screen at z ~ 1.5 across the top of
    the view whose camera side faces away from the lamp (its candidates are culled).  The lamp has an edge band, which is Solid
    black.  (A candidate whose omega is more than 45 degrees off the normal starts behind its own surface, as the reference's bounce
    along omega would, and is lost to that surface: the lamp is far enough from the wall for a good share to be nearer than that.)"""
    def r(api):
        s = api.scene()
        m = api.matte((200, 200, 200), 0.5)
        zw = lambda x, y: 6.0 + 0.05 * x + 0.03 * y
        _quad(api, s, [[x, y, zw(x, y)] for x, y in ((-10.0, -12.0), (14.0, -12.0), (14.0, 12.0), (-10.0, 12.0))], m, 0.0)
        zl = lambda x, y: 2.5 + 0.02 * x - 0.01 * y
        _quad(api, s, [[x, y, zl(x, y)] for x, y in ((3.5, 0.5), (5.0, 0.5), (5.0, 2.0), (3.5, 2.0))], solid_f32(api, lamp_color), lamp_edge)
        zo = lambda x, y: 4.5 + 0.01 * x + 0.02 * y
        _quad(api, s, [[x, y, zo(x, y)] for x, y in ((1.0, -2.5), (4.0, -2.5), (4.0, 1.0), (1.0, 1.0))], api.matte((180, 120, 90), 0.4), 0.0)
        zs = lambda x, y: 1.5 - 0.01 * x + 0.02 * y
        _quad(api, s, [[x, y, zs(x, y)] for x, y in ((0.0, 1.2), (4.0, 1.2), (4.0, 2.0), (0.0, 2.0))], api.matte((90, 160, 200), 0.6), 0.0)
        s.populate_triangle_numbers()
        s.build_bounding_box([2.0, 0.0, 6.0], 16.0, 3, 1)
        return s
    return r


NTEAPOT = 6320  # triangles 1 .. 6320 of the canonical scene are the teapot's
TEAPOT_LAMPS = (NTEAPOT + 1, NTEAPOT + 2)


def recipe_teapot_lamp(accel="octree", lamp_color=LAMP_COLOR, half=0.75, maxdepth=10, minobjs=19):
    """conftest.recipe_canonical (main.rs:116-164) with a Solid quad lamp of 2 half x 2 half above the teapot (the image's up is
    +x) and towards the camera, so that the surfaces the camera sees have it within 45 degrees of their normals; added right behind
    the teapot's triangles so that it is in the octree (or the linear list) like everything else"""
    def r(api):
        s = api.scene()
        api.add_obj(s, CT.TEAPOT_TRI, [0.0, 0.5, 5.0], 1.0, api.transform([0.0, 0.3, 1.0], 270.0), api.matte((252, 119, 0), 0.2), 0.05)
        x = lambda y, z: 4.3 + 0.03 * y - 0.25 * (z - 2.0)
        _quad(api, s, [[x(y, z), y, z] for y, z in ((0.3 - half, 2.0 - half), (0.3 + half, 2.0 - half), (0.3 + half, 2.0 + half), (0.3 - half, 2.0 + half))],
              solid_f32(api, lamp_color), 0.0)
        side = api.matte((40, 40, 40), 0.2)
        api.add_disk(s, [4.0, 4.0, 7.0], api.unit([-0.3, -0.55, -0.5]), 2.0, 0.1, 50, api.reflective(0.0002, (230, 230, 230), 0.7), side, -1.0)
        api.add_disk(s, [4.0, -3.0, 5.0], api.unit([-0.5, 2.0, -0.5]), 1.0, 0.04, 50, api.reflective(0.002, (230, 230, 230), 0.7), side, -1.0)
        s.populate_triangle_numbers()
        if accel == "octree":
            s.build_bounding_box([0.0, 0.0, 20.1], 20.0, maxdepth, minobjs)
        else:
            s.build_trivial_bounding_box([0.0, 0.0, 0.0], 20.0)
        return s
    return r


def recipe_lamp_field(corners, radiance):
    """L Solid triangles with the given corners (L, 3, 3) and float colours (L, 3) as a linear list: every one of them a lamp"""
    def r(api):
        s = api.scene()
        for c, col in zip(np.asarray(corners, F32), np.asarray(radiance, F32)):
            api.add_triangle(s, c, solid_f32(api, col), 0.0)
        s.populate_triangle_numbers()
        s.build_trivial_bounding_box([0.0, 0.0, 0.0], 20.0)
        return s
    return r
