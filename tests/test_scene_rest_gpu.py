"""csrc/scene_rest.hip against the restatement tests/ref_scene_rest.py (SPEC.md 13.16-13.18), bit for bit: the support
heights at their edge sizes, the drop on an 8 x 8 field over three scenes of 0, 1 and 5 instances -- cubes on and beside
one another, a rotated tetrahedron, the flat table mesh, a scale, a mesh of 1 280 faces and one of 1, triangles outside,
across and all over the grid, bad vertices, indices and table rows -- on fields of 1 and of 128 x 128 cells, outputs
between guard words, the refusals, and a rest layout end to end at 48 x 64. No tolerance on anything the device computes."""
import numpy as np
import pytest
import torch

import guarded
import ref_raster
import ref_scene as rs
import ref_scene_rest as rr
from ossid_code_amd import _lib, render, scenes

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
HW = (48, 64)
CAM_K = rs.rc.cam_matrix(60.0, 60.0, 31.5, 23.5)


def _dev(a, dt):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dt))).cuda()


# ---- support heights -----------------------------------------------------------------------------------------------------------
def _support(V, dirs, null=(), V_n=None, D_n=None, fill=0xA5):
    guarded.ready()
    V, dirs = np.asarray(V, F32).reshape(-1, 3), np.asarray(dirs, F64).reshape(-1, 3)
    d_v, d_d = _dev(V, F32), _dev(dirs, F64)
    g = guarded.Guarded(8 * len(dirs), fill)
    ptr = lambda name, p: None if name in null else p
    rc = _lib.fn("ossid_mesh_support")(ptr("vertices", d_v.data_ptr()), len(V) if V_n is None else V_n, ptr("dirs", d_d.data_ptr()),
                                       len(dirs) if D_n is None else D_n, ptr("h", g.ptr), _lib.stream())
    guarded.sync()
    assert g.intact(), "the guard words around h were overwritten"
    return rc, g.view(torch.float64).cpu().numpy()


def _unit_dirs(n, seed):
    d = np.random.default_rng(seed).normal(size=(n, 3))
    return d / np.sqrt((d * d).sum(1))[:, None]


@pytest.mark.parametrize("V_n,D_n", [(1, 1), (1, 65), (1025, 1), (1025, 65), (300, 8), (257, 9)])
def test_support_heights_equal_the_restatement(hiplib, V_n, D_n):
    V = np.random.default_rng(V_n + D_n).normal(size=(V_n, 3)).astype(F32)
    dirs = _unit_dirs(D_n, 3)
    rc, h = _support(V, dirs)
    want = rr.support_heights(V, dirs)
    print("V %d D %d differing %d" % (V_n, D_n, int((h != want).sum())))
    assert rc == 0 and np.array_equal(h, want) and np.isfinite(h).all()
    assert np.array_equal(_support(V, dirs)[1], h)                            # and again, the same bits


def test_support_skips_vertices_that_are_not_finite(hiplib):
    V = np.random.default_rng(1).normal(size=(700, 3)).astype(F32)
    V[5, 0], V[300, 1], V[699, 2], V[64] = np.nan, np.inf, -np.inf, (1e30, 1e30, np.nan)
    V[6] = (50.0, 0.0, 0.0)                                                   # the finite maximum along +x
    dirs = np.concatenate([np.eye(3), -np.eye(3), _unit_dirs(20, 4)])
    rc, h = _support(V, dirs)
    assert rc == 0 and np.array_equal(h, rr.support_heights(V, dirs)) and h[0] == 50.0 and np.isfinite(h).all()
    bad = np.full((130, 3), np.nan, F32)
    bad[1::2, 1] = np.inf
    bad[::2, 0] = 1.0
    rc, h = _support(bad, dirs)
    assert rc == 0 and (h == -np.inf).all() and np.array_equal(h, rr.support_heights(bad, dirs))


def test_support_refusals_write_nothing(hiplib):
    V, dirs = np.zeros((4, 3), F32), _unit_dirs(3, 0)
    for kw in ({"null": ("vertices",)}, {"null": ("dirs",)}, {"null": ("h",)}, {"V_n": 0}, {"V_n": _lib.RASTER_MAX_VERTICES + 1},
               {"D_n": 0}, {"D_n": _lib.REST_MAX_DIRS + 1}, {"D_n": -1}):
        rc, h = _support(V, dirs, **kw)
        assert rc == guarded.EINVAL and (h.view(np.uint8) == 0xA5).all(), kw


def test_resting_through_the_atlas_is_the_table_of_the_restatements_heights(hiplib):
    V, F = rr.box(0.1, 0.2, 0.3)
    sv, sf = ref_raster.icosphere(1)
    atlas = scenes.MeshAtlas({1: render.Mesh(V, F, colors=np.full((8, 3), 200, np.uint8)),
                              4: render.Mesh((0.1 * sv).astype(F32), sf, colors=np.full((len(sv), 3), 90, np.uint8))})
    t = atlas.resting(1, level=2)
    assert atlas.resting(1, level=2) is t and atlas.resting(1, level=1) is not t        # kept per (object, level)
    dirs = render._icosphere_vertices(2)
    want = scenes.resting_table(dirs, rr.support_heights(V, dirs), scenes.surface_centroid(V, F))
    assert np.array_equal(t.h, want.h) and np.array_equal(t.rest_of, want.rest_of) and np.array_equal(t.fixed, want.fixed)
    assert np.array_equal(t.rotations, want.rotations) and len(t.fixed) == 6
    assert np.array_equal(atlas.resting(4, level=2).h, rr.support_heights(atlas.mesh_arrays(4)[0], dirs))


# ---- the drop ------------------------------------------------------------------------------------------------------------------
def _meshes():
    """The test's atlas rows -> list of (vertices f32, faces int32)."""
    sv, sf = ref_raster.icosphere(3)                                          # 1 280 faces: more than one triangle per thread
    tet = (np.array([[0.1, 0.1, 0.1], [0.1, -0.1, -0.1], [-0.1, 0.1, -0.1], [-0.1, -0.1, 0.1]], F32),
           np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], np.int32))
    square = (np.array([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]], F32), np.array([[0, 1, 2], [0, 2, 3]], np.int32))
    one = (np.array([[0, 0, -0.1], [0.2, 0, 0.1], [0, 0.2, 0.05]], F32), np.array([[0, 1, 2]], np.int32))
    # a NaN vertex, an index past the mesh and a negative one: their triangles are skipped, the fourth is placed
    broken = (np.array([[0, 0, -0.2], [0.3, 0, 0], [0, 0.3, 0.1], [np.nan, 0, 0], [0, np.inf, 0]], F32),
              np.array([[0, 1, 3], [0, 1, 5], [-1, 1, 2], [0, 1, 2], [4, 1, 2]], np.int32))
    nothing = (np.array([[0, 0, 0], [np.nan, 0, 0], [0, 1, 0]], F32), np.array([[0, 1, 2], [0, 2, 3], [7, 8, 9]], np.int32))
    return [rr.cube(0.5), tet, square, ((0.4 * sv).astype(F32), sf), one, broken, nothing]


CUBE, TET, SQUARE, SPHERE, ONE, BROKEN, NOTHING, CORRUPT = range(8)


def _pack(meshes):
    nv, nf = [len(m[0]) for m in meshes], [len(m[1]) for m in meshes]
    v0, f0 = np.concatenate([[0], np.cumsum(nv)[:-1]]), np.concatenate([[0], np.cumsum(nf)[:-1]])
    table = np.stack([v0, nv, f0, nf], 1).astype(np.int32)
    V, F = np.concatenate([m[0] for m in meshes]).astype(F32), np.concatenate([m[1] for m in meshes]).astype(np.int32)
    # one more row whose vertex count leads past the atlas: an instance of it places nothing
    table = np.concatenate([table, np.array([[len(V) - 2, 3, 0, 1]], np.int32)])
    return V, F, table


@pytest.fixture(scope="module")
def packed(hiplib):
    meshes = _meshes()
    V, F, table = _pack(meshes)
    return meshes + [(np.zeros((1, 3), F32), np.zeros((0, 3), np.int32))], (_dev(V, F32), _dev(F, np.int32), _dev(table, np.int32))


def _raw_drop(dev, mesh, first, local, G, cell, height=True, null=(), fill=0xA5, **over):
    """ossid_scene_drop itself, every output between guard words -> (status code, drop, status, height or None)."""
    guarded.ready()
    d_v, d_f, d_t = dev
    mesh, first = np.asarray(mesh, np.int32).reshape(-1), np.asarray(first, np.int32).reshape(-1)
    local = np.asarray(local, F64).reshape(-1, 3, 4)
    I, S = len(mesh), len(first) - 1
    d_m, d_s, d_l = _dev(mesh, np.int32), _dev(first, np.int32), _dev(local, F64)
    g_d, g_s = guarded.Guarded(8 * I, fill), guarded.Guarded(4 * I, fill)
    g_h = guarded.Guarded(4 * max(S, 1) * G * G, fill) if height and G >= 1 else None
    a = {"Vt": d_v.shape[0], "Ft": d_f.shape[0], "K": d_t.shape[0], "I": I, "S": S, "G": G, "cell": cell}
    a.update(over)
    ptr = lambda name, p: None if name in null else p
    rc = _lib.fn("ossid_scene_drop")(
        ptr("vertices", d_v.data_ptr()), ptr("faces", d_f.data_ptr()), ptr("meshes", d_t.data_ptr()), a["Vt"], a["Ft"], a["K"],
        ptr("instance_mesh", d_m.data_ptr() if I else None), ptr("scene_first", d_s.data_ptr()),
        ptr("local", d_l.data_ptr() if I else None), a["I"], a["S"], a["G"], float(a["cell"]), ptr("drop", g_d.ptr if I else None),
        ptr("status", g_s.ptr if I else None), None if g_h is None else g_h.ptr, _lib.stream())
    guarded.sync()
    for g in (g_d, g_s) + (() if g_h is None else (g_h,)):
        assert g.intact(), "guard words around an output of ossid_scene_drop were overwritten"
    h = None if g_h is None else g_h.view(torch.float32).cpu().numpy().reshape(max(S, 1), G, G)
    return rc, g_d.view(torch.float64).cpu().numpy(), g_s.view(torch.int32).cpu().numpy(), h


def _check(packed, mesh, first, local, G, cell):
    """The device's drop, status and height field equal the restatement's, bit for bit -> the three arrays."""
    meshes, dev = packed
    rc, d, s, h = _raw_drop(dev, mesh, first, local, G, cell)
    wd, ws, wh = rr.drop(meshes, mesh, first, local, G, cell)
    print("G %d: drop differs in %d, status in %d, height in %d cells" % (G, int((d != wd).sum()), int((s != ws).sum()),
                                                                      int((h.view(np.uint32) != wh.view(np.uint32)).sum())))
    assert rc == 0
    assert np.array_equal(d, wd) and np.array_equal(s, ws) and np.array_equal(h, wh)
    assert np.array_equal(h.view(np.uint32), wh.view(np.uint32)) and not np.signbit(h).any()      # a -0 is never stored
    return d, s, h


def _turn():
    q = np.array([0.9, 0.3, -0.2, 0.4])
    w, x, y, z = q / np.sqrt(q @ q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _tet_low(R, scale=1.0):
    V = _meshes()[TET][0].astype(F64)
    L = rr.place(0.0, 0.0, R, scale)
    return min(((L[2, 0] * v[0] + L[2, 1] * v[1]) + L[2, 2] * v[2]) + L[2, 3] for v in V)


def test_drop_cubes_on_and_beside_one_another(packed):
    """Scenes of 0, 1 and 5 instances at G = 8, cell 0.25: a unit cube takes the cells 2..6 of a row."""
    R = _turn()
    mesh = [CUBE, CUBE, CUBE, CUBE, TET, CUBE]
    local = [rr.place(), rr.place(), rr.place(), rr.place(-1.5, 0.0), rr.place(0.87, 0.87, R, 0.5), rr.place(0.25, 0.0)]
    d, s, h = _check(packed, mesh, [0, 0, 1, 6], local, 8, 0.25)
    assert d[0] == 0.5 and s[0] == 0                                          # a unit cube on the table
    assert d[1] == 0.5 and d[2] == 1.5                                        # a second cube on the same cells
    assert d[3] == 0.5 and s[3] == 2                                          # a disjoint cube (it leaves the grid on the left)
    assert d[4] == -_tet_low(R, 0.5) and s[4] == 0 and 0.02 < d[4] < 0.09         # a rotated tetrahedron on free cells
    assert d[5] == 2.5                                                        # one cell over, still above both cubes
    assert not h[0].any() and h[1, 2:7, 2:7].min() == 1.0 and h[1].sum() == 25.0
    assert h[2, 4, 4] == 3.0 and h[2, 4, 7] == 3.0 and h[2, 4, 2] == 2.0 and h[2, 4, 0] == 1.0 and h[2, 0, 4] == 0.0


def test_drop_the_table_mesh_a_scale_and_many_faces(packed):
    mesh = [SQUARE, CUBE, CUBE, CUBE, SPHERE, ONE]
    local = [rr.place(scale=0.9), rr.place(), rr.place(0.25, 0.0), rr.place(scale=2.0), rr.place(0.1, -0.1), rr.place(-0.9, -0.9)]
    d, s, h = _check(packed, mesh, [0, 0, 1, 6], local, 8, 0.25)
    assert d[0] == 0.0 and s[0] == 0 and not h[1].any()                       # the flat table mesh: drop 0, H stays 0
    assert d[1] == 0.5 and d[2] == 1.5                                        # a second cube one cell over, still overlapping
    assert d[3] == 3.0 and s[3] == 2                                          # twice the size: 2 above, 1 below its origin
    assert 4.35 < d[4] < 4.45 and s[4] == 0                                   # 1 280 faces, on top of the big cube (at 4.0)
    assert d[5] > 4.0 and s[5] == 0                                           # one face, over a corner cell of the big cube


def test_drop_triangles_outside_across_and_all_over_the_grid(packed):
    mesh = [ONE, ONE, ONE, BROKEN, NOTHING, CUBE]
    local = [rr.place(scale=40.0, x=-3.0, y=-3.0), rr.place(5.0, 0.0), rr.place(0.9, 0.0), rr.place(), rr.place(), rr.place()]
    d, s, h = _check(packed, mesh, [0, 0, 1, 6], local, 8, 0.25)
    assert d[0] == 40.0 * np.float64(F32(0.1)) and s[0] == 2 and (h[1] == h[1, 0, 0]).all() and h[1, 0, 0] >= 8.0     # one triangle over every cell
    assert d[1] == np.float64(F32(0.1)) and s[1] == 2                         # wholly outside: the table term alone
    assert s[2] == 2 and d[2] == np.float64(F32(0.1)) and h[2, 4, 7] > 0 and h[2, 3, 7] == 0  # across the right edge
    assert d[3] == np.float64(F32(0.2)) and s[3] == 0                         # the NaN vertex and the bad indices are skipped
    assert d[4] == 0.0 and s[4] == 1                                          # nothing usable: status 1 ...
    assert 0.8 <= d[5] < 0.8000001 and s[5] == 0                              # ... and the next object meets H as it was
    meshes, dev = packed
    without = rr.drop(meshes, [m for k, m in enumerate(mesh) if k != 4], [0, 0, 1, 5], [l for k, l in enumerate(local) if k != 4],
                      8, 0.25)
    assert d[5] == without[0][4] and np.array_equal(h, without[2])            # as if the unusable mesh were not there


def test_drop_does_not_follow_indices_out_of_the_arrays(packed):
    meshes, dev = packed
    mesh = [CUBE, 99, -1, CORRUPT, CUBE]
    local = [rr.place()] * 5
    d, s, h = _check(packed, mesh, [0, 0, 0, 5], local, 8, 0.25)
    assert d.tolist() == [0.5, 0.0, 0.0, 0.0, 1.5] and s.tolist() == [0, 1, 1, 1, 0]
    # scene_first entries that lead outside [0, I] or run backwards place nothing; the other scenes are untouched
    for first in ([0, 1, 9], [0, -1, 5], [3, 1, 5]):
        rc, d, s, h = _raw_drop(dev, [CUBE] * 5, first, local, 8, 0.25)
        wd, ws, wh = rr.drop(meshes, [CUBE] * 5, first, local, 8, 0.25)
        assert rc == 0 and np.array_equal(h, wh)
        placed = np.zeros(5, bool)
        for a, b in zip(first[:-1], first[1:]):
            if 0 <= a <= b <= 5:
                placed[a:b] = True
        assert np.array_equal(d[placed], wd[placed]) and np.array_equal(s[placed], ws[placed])
        assert (d[~placed].view(np.uint8) == 0xA5).all()                      # never written


@pytest.mark.parametrize("G,cell", [(1, 4.0), (3, 0.7), (128, 1.0 / 64.0), (128, 0.011), (111, 0.02)])
def test_drop_at_other_field_sizes(packed, G, cell):
    """G = 1; an odd G, whose origin is the middle of a cell; G = 128, the full 64 KiB field, and the first size above the
    default LDS limit. The large boxes here are walked by whole waves."""
    R = _turn()
    mesh = [CUBE, CUBE, SPHERE, TET, ONE, SQUARE]
    local = [rr.place(), rr.place(0.1, -0.2, R), rr.place(0.3, 0.3), rr.place(-0.8, 0.8, R, 2.0), rr.place(0.5, -0.6, R),
             rr.place(scale=0.5)]
    d, s, h = _check(packed, mesh, [0, 0, 1, 6], local, G, cell)
    assert d[0] == 0.5 and (d[1:] > 0).all()
    again = _raw_drop(packed[1], mesh, [0, 0, 1, 6], local, G, cell)
    assert np.array_equal(again[1], d) and np.array_equal(again[3], h)        # the same bits twice


def test_drop_without_a_height_output_and_without_instances(packed):
    meshes, dev = packed
    rc, d, s, h = _raw_drop(dev, [CUBE, CUBE], [0, 2], [rr.place(), rr.place()], 8, 0.25, height=False)
    assert rc == 0 and d.tolist() == [0.5, 1.5] and s.tolist() == [0, 0] and h is None
    rc, d, s, h = _raw_drop(dev, [], [0, 0, 0], np.zeros((0, 3, 4)), 8, 0.25)
    assert rc == 0 and not h.any() and h.shape == (2, 8, 8)


def test_drop_refusals_write_nothing(packed):
    meshes, dev = packed
    args = ([CUBE, CUBE], [0, 2], [rr.place(), rr.place()])
    cases = [{"G": 0}, {"G": 129}, {"cell": 0.0}, {"cell": -1.0}, {"cell": np.inf}, {"cell": np.nan}, {"S": 0},
             {"S": _lib.SCENE_MAX_SCENES + 1}, {"I": -1}, {"I": _lib.SCENE_MAX_INSTANCES + 1}, {"K": 0}, {"Vt": 0}, {"Ft": -1},
             {"Vt": (1 << 29) + 1}]
    nulls = ["vertices", "faces", "meshes", "instance_mesh", "scene_first", "local", "drop", "status"]
    for kw in cases + [{"null": (n,)} for n in nulls]:
        over = dict(kw)
        G = over.pop("G", 8)
        cell = over.pop("cell", 0.25)
        rc, d, s, h = _raw_drop(dev, *args, G, cell, **over)
        assert rc == guarded.EINVAL, kw
        assert (d.view(np.uint8) == 0xA5).all() and (s.view(np.uint8) == 0xA5).all(), kw
        assert h is None or (h.view(np.uint8) == 0xA5).all(), kw


def test_scene_drop_wrapper_is_the_entry(packed):
    V, F = rr.cube(0.5)
    atlas = scenes.MeshAtlas({1: render.Mesh(V, F, colors=np.full((8, 3), 99, np.uint8))})
    local = [rr.place(), rr.place(0.25, 0.0), rr.place(scale=0.9)]
    mesh = [0, 0, atlas.index_of[scenes.TABLE_OBJ_ID]]
    d, s, h = scenes.scene_drop(atlas, mesh, [0, 3], local, 8, 0.25, height=True)
    wd, ws, wh = rr.drop([atlas.mesh_arrays(o)[:2] for o in atlas.obj_ids], mesh, [0, 3], local, 8, 0.25)
    assert np.array_equal(d, wd) and np.array_equal(s, ws) and np.array_equal(h, wh) and d.tolist() == [0.5, 1.5, 2.0]
    assert len(scenes.scene_drop(atlas, mesh, [0, 3], local, 8, 0.25)) == 2


# ---- a rest layout, end to end -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rest_setup(hiplib):
    sv, sf = ref_raster.icosphere(1)
    rng = np.random.default_rng(3)
    col = lambda V: rng.integers(60, 256, (len(V), 3)).astype(np.uint8)
    bv, bf = rr.box(0.04, 0.07, 0.10)
    cv, cf = rr.cube(0.03)
    ev = (sv * np.array([0.05, 0.03, 0.02])).astype(F32)
    atlas = scenes.MeshAtlas({1: render.Mesh(bv, bf, colors=col(bv)), 2: render.Mesh(cv, cf, colors=col(cv)),
                              3: render.Mesh(ev, sf, colors=col(ev))})
    make = lambda: scenes.sample_layouts(atlas, 4, 3, CAM_K, HW, np.random.default_rng(21), z_range=(0.3, 0.5),
                                         placement="rest", rest_level=2, grid=64)
    return atlas, make(), make


def test_rest_layout_is_the_restatements_drop_and_composition(rest_setup):
    atlas, lay, make = rest_setup
    table = atlas.index_of[scenes.TABLE_OBJ_ID]
    assert lay.scene_first.tolist() == [0, 4, 8, 12, 16] and lay.table_mesh == table
    assert lay.table_pose.shape == (4, 4, 4) and lay.local.shape == (16, 3, 4) and lay.drop.shape == (16,)
    assert (lay.status == 0).all()                                            # the grid covers what the sampler places
    obj = lay.instance_mesh != table
    assert obj.sum() == 12 and not obj[::4].any() and (lay.drop[~obj] == 0).all()
    # the restatement reproduces the drop from the locals, on the sampler's own grid
    G, cell = lay.grid
    reach = max(max(abs(L[0, 3]), abs(L[1, 3])) + atlas.radius(atlas.obj_ids[m]) for L, m in zip(lay.local[obj], lay.instance_mesh[obj]))
    assert G == 64 and reach <= 32 * cell                                     # the field covers every object's sphere
    meshes = [atlas.mesh_arrays(o)[:2] for o in atlas.obj_ids]
    wd, ws, _h = rr.drop(meshes, lay.instance_mesh[obj], [0, 3, 6, 9, 12], lay.local[obj], 64, cell)
    assert np.array_equal(lay.drop[obj], wd) and np.array_equal(lay.status[obj], ws)
    low_first = []
    for s in range(4):
        P = lay.table_pose[s]
        assert np.allclose(P[:3, :3] @ P[:3, :3].T, np.eye(3), atol=1e-14) and 0.3 <= P[2, 3] <= 0.5 and P[0, 3] == P[1, 3] == 0
        elev = np.rad2deg(np.arcsin(-P[2, 2]))                                # the table's up against the optical axis
        assert 25.0 - 1e-9 <= elev <= 65.0 + 1e-9 and P[1, 2] < 0             # it faces the camera, image-up
        inv = np.linalg.inv(P)
        for i in range(lay.scene_first[s], lay.scene_first[s + 1]):
            assert np.array_equal(lay.transforms[i], rr.compose(P, lay.drop[i], lay.local[i]))       # the composition
            if not obj[i]:
                continue
            V = atlas.mesh_arrays(atlas.obj_ids[lay.instance_mesh[i]])[0].astype(F64)
            in_table = (inv @ lay.transforms[i] @ np.concatenate([V, np.ones((len(V), 1))], 1).T).T
            lowest = in_table[:, 2].min()
            print("scene %d instance %d lowest %.3e drop %.6f" % (s, i, lowest, lay.drop[i]))
            assert lowest >= -1e-12                                           # nothing is below the table
            if i == lay.scene_first[s] + 1:
                low_first.append(lowest)
            c = lay.transforms[i][:3, 3]                                      # the object's centre projects inside the frame
            u, v = 60.0 * c[0] / c[2] + 31.5, 60.0 * c[1] / c[2] + 23.5
            assert c[2] > 0 and 0.0 <= u <= HW[1] and 0.0 <= v <= HW[0]
            R = lay.local[i][:, :3]
            assert np.allclose(R @ R.T, np.eye(3), atol=1e-12) and np.linalg.det(R) > 0 and lay.local[i][2, 3] == 0.0
    assert len(low_first) == 4 and max(abs(v) for v in low_first) <= 1e-12    # each scene's first object is on the table


def test_rest_layout_renders_and_repeats(rest_setup):
    atlas, lay, make = rest_setup
    again = make()
    for name in ("instance_mesh", "transforms", "scene_first", "cams", "table_pose", "local", "drop", "status"):
        assert np.array_equal(getattr(lay, name), getattr(again, name)), name
    lights, material = scenes.sample_lights(lay, np.random.default_rng(2))
    batch = scenes.render_scenes(atlas, lay, HW, lights=lights, material=material, shadows=scenes.Shadows(size=(64, 64)))
    torch.cuda.synchronize()
    g = batch.gt_info.cpu().numpy()
    table = atlas.index_of[scenes.TABLE_OBJ_ID]
    print("px_count_all", g[:, 0].tolist())
    assert (g[lay.instance_mesh != table, 0] > 0).all()                       # every object is in the picture
    assert (g[lay.instance_mesh == table, 0] > HW[0] * HW[1] // 4).all()      # and so is the table under them
    assert len(list(batch.frames())) == 12
    bare = scenes.sample_layouts(atlas, 2, 5, CAM_K, HW, np.random.default_rng(4), z_range=(0.3, 0.5), placement="rest",
                                 rest_level=1, table=False)
    assert bare.scene_first.tolist() == [0, 5, 10] and table not in bare.instance_mesh and (bare.status == 0).all()
    assert (bare.drop > 0).all()
