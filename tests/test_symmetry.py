"""SPEC.md section 17 on the host: the selection of ossid_code_amd.symmetry.find_symmetries run over the numpy restatement
(tests/ref_symmetry.py, brute-force neighbours) through score=, on analytic objects whose groups are derived by hand; the
candidate set; the models_info.json form and its way through bop_eval.symmetry_transformations and SceneBatch.write_bop.

Sizes. Brute force over C candidates costs C * Mq * Nt distances, so the objects are sampled at Nt = 2048, Mq = 128 and the
candidates come from icosphere level 3 (321 axes, 7.9 degrees apart) at max_order = 4: 963 candidates. A level-3 direction
lies up to half a spacing (0.069 rad) off the true axis before the refinement and a quarter after it (0.035 rad), which a
two-fold rotation doubles at the rim (radius d / 2): 0.035 d; the 2048 targets are about 0.03 d apart, so a mapped point
finds one within about 0.02 d. The sum exceeds the default tol_rel = 0.05, which belongs to level 4 and 32768 targets (SPEC
17.6; test_symmetry_gpu.py runs it): the objects below are found at tol_rel = 0.1, and their nearest false symmetry is off
by more than that (the box's sides differ by 0.25 d and more, the lathe's ends by 0.25 d in radius). The ellipsoid's bump
sticks out 0.08 d, so it is run at tol_rel = 0.05, where none of its own near-symmetries needs to pass."""
import json
import os

import numpy as np
import pytest

import ref_icp
import ref_symmetry as rs
from ossid_code_amd import bop_eval, symmetry

NT, MQ, LEVEL, MAX_ORDER = 2048, 128, 3, 4


def _sample(gen):
    """The first of a shrinking series of spacings whose sample has at least NT points, thinned to NT."""
    s = 0.1
    for _ in range(60):
        P = gen(s)
        if len(P) >= NT:
            break
        s *= 0.93
    T = rs.thin(P, NT).astype(np.float32)
    return T, rs.thin(T, MQ), rs.diameter(T)


OBJECTS = {
    "box": (lambda s: rs.box_points(1.0, 0.6, 0.3, s), 0.1, 3, 0),
    "square_prism": (lambda s: rs.prism_points(4, 0.5, 0.4, s), 0.1, 7, 0),
    "triangular_prism": (lambda s: rs.prism_points(3, 0.5, 0.4, s), 0.1, 5, 0),
    "lathe": (lambda s: rs.lathe_points(rs.LATHE_PROFILE, s), 0.1, 0, 1),
    "cylinder": (lambda s: rs.lathe_points(rs.CYLINDER_PROFILE, s), 0.1, 1, 1),
    "ellipsoid_with_bump": (lambda s: ref_icp._surface(4 * NT, np.random.default_rng(0))[0], 0.05, 0, 0),
}
_FOUND = {}


def found(name):
    """find_symmetries of one object, computed once and shared."""
    if name not in _FOUND:
        gen, tol_rel, _nd, _nc = OBJECTS[name]
        T, Q, d = _sample(gen)
        out, info = symmetry.find_symmetries((T, Q), tol_rel=tol_rel, level=LEVEL, max_order=MAX_ORDER, score=rs.score_transforms,
                                             diameter=d, return_info=True)
        _FOUND[name] = (out, info, T, Q)
    return _FOUND[name]


def _rotation_parts(M):
    """(axis, angle in (0, pi]) of a rotation matrix' upper 3x3."""
    R = np.asarray(M, dtype=np.float64).reshape(4, 4)[:3, :3]
    ang = float(np.arccos(np.clip((np.trace(R) - 1.0) / 2.0, -1.0, 1.0)))
    w, v = np.linalg.eig(R)
    a = np.real(v[:, int(np.argmin(np.abs(w - 1.0)))])
    return a / np.linalg.norm(a), ang


@pytest.mark.parametrize("name", list(OBJECTS))
def test_the_group_is_the_one_derived_by_hand(name):
    _gen, _tol_rel, n_disc, n_cont = OBJECTS[name]
    out, info, T, Q = found(name)
    print(name, "discrete", len(out["symmetries_discrete"]), "continuous", len(out["symmetries_continuous"]), "scored",
          info["n_scored"])
    assert set(out) == {"symmetries_discrete", "symmetries_continuous"}
    assert len(out["symmetries_discrete"]) == n_disc and len(out["symmetries_continuous"]) == n_cont
    assert all(len(m) == 16 and all(isinstance(v, float) for v in m) for m in out["symmetries_discrete"])
    json.dumps(out)                                              # plain lists and floats


def test_the_elements_are_the_groups_own():
    z, tol_axis = np.array([0.0, 0.0, 1.0]), 2.0 * symmetry.grid_spacing(LEVEL)

    def parts(name):
        return [_rotation_parts(m) for m in found(name)[0]["symmetries_discrete"]]

    def about_z(a):
        return abs(a[2]) > np.cos(tol_axis)

    # the box: the three coordinate half-turns
    axes = np.abs(np.stack([a for a, _ in parts("box")]))
    assert all(abs(th - np.pi) < 1e-9 for _, th in parts("box"))
    assert sorted(int(np.argmax(a)) for a in axes) == [0, 1, 2] and (axes.max(1) > np.cos(tol_axis)).all()
    # the square prism: quarter, half and three-quarter turns about z (3/4 shows as a quarter turn about -z) and four
    # half-turns in the plane, 45 degrees apart
    sq = parts("square_prism")
    zs = sorted(round(th / (np.pi / 2)) for a, th in sq if about_z(a))
    assert zs == [1, 1, 2]
    flat = [a for a, th in sq if not about_z(a)]
    assert len(flat) == 4 and all(abs(a[2]) < np.sin(tol_axis) for a in flat)
    phis = sorted(np.degrees(np.arctan2(a[1], a[0])) % 180.0 for a in flat)
    assert np.allclose(np.diff(phis), 45.0, atol=np.degrees(tol_axis))
    # the triangular prism: thirds about z, three half-turns in the plane 60 degrees apart
    tr = parts("triangular_prism")
    assert sorted(round(th / (2 * np.pi / 3)) for a, th in tr if about_z(a)) == [1, 1]
    flat = [a for a, th in tr if not about_z(a)]
    assert len(flat) == 3 and all(abs(th - np.pi) < 1e-9 for a, th in tr if not about_z(a))
    phis = sorted(np.degrees(np.arctan2(a[1], a[0])) % 180.0 for a in flat)
    assert np.allclose(np.diff(phis), 60.0, atol=np.degrees(tol_axis))
    # the lathe and the cylinder: z, through the centroid; the cylinder's flip is a half-turn perpendicular to it
    for name in ("lathe", "cylinder"):
        out, info = found(name)[:2]
        c = out["symmetries_continuous"][0]
        assert about_z(np.asarray(c["axis"])) and np.allclose(c["offset"], info["centre"])
    (a, th), = parts("cylinder")
    assert abs(th - np.pi) < 1e-9 and abs(a[2]) < np.sin(tol_axis)


@pytest.mark.parametrize("name", list(OBJECTS))
def test_every_emitted_transform_maps_the_surface_within_tol(name):
    """... and the dict goes through bop_eval.symmetry_transformations: the identity first, every discrete element next (or
    its products with the continuous steps), each a proper rigid motion under which every query has a target within tol."""
    out, info, T, Q = found(name)
    S = bop_eval.symmetry_transformations(out, max_sym_disc_step=0.05)
    n_disc, n_cont = len(out["symmetries_discrete"]), len(out["symmetries_continuous"])
    steps = int(np.ceil(np.pi / 0.05))
    assert len(S) == (1 + n_disc) * (steps if n_cont else 1)
    assert np.allclose(S[0], np.eye(4))
    for M in S:
        assert np.allclose(M[:3, :3] @ M[:3, :3].T, np.eye(3), atol=1e-9) and np.linalg.det(M[:3, :3]) > 0.0
        assert np.array_equal(M[3], [0.0, 0.0, 0.0, 1.0])
    if n_cont > 1:
        return
    miss, worst, _sum = rs.score_transforms(T, Q, S, info["tol"])
    assert miss.max() == 0 and float(np.sqrt(worst.max())) <= info["tol"]
    # every vertex of the sample, not the queries alone (max_miss = 0 was asked of the queries)
    D = np.stack([np.asarray(m).reshape(4, 4) for m in out["symmetries_discrete"]]) if n_disc else np.zeros((0, 4, 4))
    if n_disc:
        miss, worst, _sum = rs.score_transforms(T, T, D, info["tol"])
        assert miss.max() == 0


def test_candidates_count_and_one_axis_per_pair():
    for level in (0, 1, 2, 3):
        axes = symmetry.candidate_axes(level)
        n_dirs = 10 * 4 ** level + 2
        assert axes.shape == (n_dirs // 2, 3) and np.allclose((axes * axes).sum(1), 1.0)
        both = np.concatenate([axes, -axes])
        # the kept axes and their opposites are the whole icosphere, each direction once
        from ossid_code_amd import render
        dirs = render._icosphere_vertices(level)
        d = np.abs(both[:, None, :] - dirs[None]).max(-1)
        assert (d.min(1) < 1e-9).all() and len(set(d.argmin(1).tolist())) == n_dirs
        dots = axes @ axes.T
        assert dots.min() > -1.0 + 1e-6                          # no axis is another's opposite
    centre = np.array([0.3, -0.2, 0.1])
    for level, max_order in ((0, 2), (1, 4), (2, 8)):
        T = symmetry.candidate_rotations(centre, level=level, max_order=max_order)
        assert T.shape == ((10 * 4 ** level + 2) // 2 * (max_order - 1), 4, 4)
        assert np.allclose(T[:, :3, :3] @ np.swapaxes(T[:, :3, :3], 1, 2), np.eye(3), atol=1e-12)
        assert np.allclose(np.linalg.det(T[:, :3, :3]), 1.0)     # proper rotations only
        assert np.allclose(T[:, :3, :3] @ centre + T[:, :3, 3], centre, atol=1e-12)          # about the centre
        ang = np.arccos(np.clip((np.trace(T[:, :3, :3], axis1=1, axis2=2) - 1.0) / 2.0, -1.0, 1.0))
        want = np.tile([min(2 * np.pi / k, 2 * np.pi - 2 * np.pi / k) for k in range(2, max_order + 1)], len(T) // (max_order - 1))
        assert np.allclose(ang, want, atol=1e-7)
    assert len(symmetry.candidate_rotations(centre)) == 1281 * 7


def test_bad_arguments_are_refused_before_the_device():
    P = np.zeros((4, 3), np.float32)
    T = np.eye(4)[None]
    for bad in (lambda: symmetry.score_transforms(np.zeros((0, 3)), P, T, 0.1), lambda: symmetry.score_transforms(P, np.zeros((4, 2)), T, 0.1),
                lambda: symmetry.score_transforms(np.zeros((32769, 3)), P, T, 0.1), lambda: symmetry.score_transforms(P, np.zeros((4097, 3)), T, 0.1),
                lambda: symmetry.score_transforms(P, P, np.eye(4), 0.1), lambda: symmetry.score_transforms(P, P, np.zeros((0, 4, 4)), 0.1),
                lambda: symmetry.score_transforms(P, P, T, 0.0), lambda: symmetry.score_transforms(P, P, T, float("nan")),
                lambda: symmetry.score_transforms(P, P, T, float("inf")), lambda: symmetry.score_transforms(P, P, T, 1e-30),
                lambda: symmetry.score_transforms(P, P, T, 1e30), lambda: symmetry.score_transforms(np.full((4, 3), np.nan), P, T, 0.1),
                lambda: symmetry.find_symmetries((P, P), tol_rel=0.0, diameter=1.0, score=rs.score_transforms),
                lambda: symmetry.find_symmetries((P, P), max_miss=-1, diameter=1.0, score=rs.score_transforms),
                lambda: symmetry.find_symmetries((P, P), max_order=1, diameter=1.0, score=rs.score_transforms),
                lambda: symmetry.find_symmetries((P, P), level=6, diameter=1.0, score=rs.score_transforms),
                lambda: symmetry.find_symmetries((P, P), diameter=0.0, score=rs.score_transforms)):
        with pytest.raises(ValueError):
            bad()


def test_scaled_moves_translations_and_offsets_only():
    sym = {"symmetries_discrete": [[float(v) for v in range(16)]],
           "symmetries_continuous": [{"axis": [0.0, 0.0, 1.0], "offset": [0.001, 0.002, 0.003]}]}
    mm = symmetry.scaled(sym, 1000.0)
    want = [float(v) for v in range(16)]
    for i in (3, 7, 11):
        want[i] *= 1000.0
    assert mm["symmetries_discrete"] == [want]
    assert mm["symmetries_continuous"] == [{"axis": [0.0, 0.0, 1.0], "offset": [1.0, 2.0, 3.0]}]
    assert symmetry.has_symmetry(sym) and not symmetry.has_symmetry({"symmetries_discrete": [], "symmetries_continuous": []})


def test_models_info_entry_gains_the_keys_in_millimetres_and_keeps_the_rest():
    """SceneBatch.write_bop's models_info.json: with symmetries given as a dict (metres) the entry gains the two keys in
    millimetres; the bytes of every other key are the ones written without."""
    from ossid_code_amd import scenes
    base = {"diameter": 123.5, "min_x": -1.0, "min_y": -2.0, "min_z": -3.0, "size_x": 2.0, "size_y": 4.0, "size_z": 6.0}
    T = symmetry.rotation_about([0.0, 0.0, 1.0], np.pi, [0.01, 0.02, 0.03])
    sym = {"symmetries_discrete": [[float(v) for v in T.reshape(-1)]],
           "symmetries_continuous": [{"axis": [0.0, 0.0, 1.0], "offset": [0.01, 0.02, 0.03]}]}
    entry = scenes.models_info_entry(dict(base), sym)
    assert list(entry)[:len(base)] == list(base) and all(entry[k] == base[k] for k in base)
    assert json.dumps({k: entry[k] for k in base}, indent=1) == json.dumps(base, indent=1)
    got = np.asarray(entry["symmetries_discrete"][0]).reshape(4, 4)
    assert np.array_equal(got[:3, :3], T[:3, :3]) and np.allclose(got[:3, 3], 1000.0 * T[:3, 3], rtol=1e-15)
    assert entry["symmetries_continuous"] == [{"axis": [0.0, 0.0, 1.0], "offset": [10.0, 20.0, 30.0]}]
    assert scenes.models_info_entry(dict(base), None) == base
    S = bop_eval.symmetry_transformations(entry, max_sym_disc_step=0.5)
    assert np.allclose(S[0], np.eye(4))


def test_write_bop_with_a_dict_writes_millimetres_and_leaves_the_other_bytes(hiplib, tmp_path):
    """The folder written with symmetries={obj: dict} differs from the one written without in models_info.json alone, and
    there only by the two keys of that object, in millimetres."""
    import test_scene as ts
    atlas = ts._atlas()
    batch = ts._host_batch(atlas, 1.0)
    T = symmetry.rotation_about([0.0, 1.0, 0.0], np.pi, [0.001, 0.002, 0.003])
    sym = {2: {"symmetries_discrete": [[float(v) for v in T.reshape(-1)]],
               "symmetries_continuous": [{"axis": [0.0, 1.0, 0.0], "offset": [0.001, 0.002, 0.003]}]},
           3: {"symmetries_discrete": [], "symmetries_continuous": []}}
    plain = batch.write_bop(str(tmp_path / "plain"), "synth", diameters=ts._diameters(atlas))
    with_sym = batch.write_bop(str(tmp_path / "sym"), "synth", diameters=ts._diameters(atlas), symmetries=sym)
    for sub in ("models", "models_eval"):
        a = json.load(open(os.path.join(plain, sub, "models_info.json")))
        b = json.load(open(os.path.join(with_sym, sub, "models_info.json")))
        assert list(a) == list(b) and a["1"] == b["1"] and a["3"] == b["3"]
        assert list(b["2"])[:len(a["2"])] == list(a["2"]) and {k: b["2"][k] for k in a["2"]} == a["2"]
        assert sorted(set(b["2"]) - set(a["2"])) == ["symmetries_continuous", "symmetries_discrete"]
        got = np.asarray(b["2"]["symmetries_discrete"][0]).reshape(4, 4)
        assert np.array_equal(got[:3, :3], T[:3, :3]) and np.allclose(got[:3, 3], 1000.0 * T[:3, 3], rtol=1e-15)
        assert b["2"]["symmetries_continuous"] == [{"axis": [0.0, 1.0, 0.0], "offset": [1.0, 2.0, 3.0]}]
        # the bytes: the file without the two keys is the file written without symmetries
        del b["2"]["symmetries_discrete"], b["2"]["symmetries_continuous"]
        assert json.dumps(b, indent=1) == open(os.path.join(plain, sub, "models_info.json")).read()
    import filecmp
    for root, _dirs, files in os.walk(plain):
        for f in files:
            if f != "models_info.json":
                other = os.path.join(with_sym, os.path.relpath(os.path.join(root, f), plain))
                assert filecmp.cmp(os.path.join(root, f), other, shallow=False), f


def test_stream_auto_needs_meshes():
    from ossid_code_amd.stream import OnlineStream
    with pytest.raises(ValueError, match="auto"):
        OnlineStream(None, None, None, symmetries="auto")
    with pytest.raises(ValueError, match="auto"):
        OnlineStream(None, None, None, symmetries="always", meshes={})
    assert OnlineStream(None, None, None, symmetries={1: np.eye(4)[None]})._symmetries(1).shape == (1, 4, 4)
    assert OnlineStream(None, None, None)._symmetries(1) is None and OnlineStream(None, None, None)._symmetric({"obj_id": 1}) is False


def test_merge_into_models_info_json(tmp_path):
    """tools/find_symmetries.py --write merges: other keys and other objects keep their values."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("find_symmetries_tool", os.path.join(os.path.dirname(__file__), "..", "tools",
                                                                                       "find_symmetries.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    path = tmp_path / "models_info.json"
    info = {"1": {"diameter": 100.0, "min_x": -1.0}, "2": {"diameter": 50.0, "symmetries_discrete": [[0.0] * 16]}}
    path.write_text(json.dumps(info))
    found_ = {1: {"symmetries_discrete": [[1.0] * 16], "symmetries_continuous": []},
              2: {"symmetries_discrete": [], "symmetries_continuous": [{"axis": [0.0, 0.0, 1.0], "offset": [0.0, 0.0, 0.0]}]}}
    tool.merge(str(path), found_)
    got = json.loads(path.read_text())
    assert got["1"] == {"diameter": 100.0, "min_x": -1.0, "symmetries_discrete": [[1.0] * 16]}
    assert got["2"] == {"diameter": 50.0, "symmetries_continuous": [{"axis": [0.0, 0.0, 1.0], "offset": [0.0, 0.0, 0.0]}]}


def test_grid_size_query_on_the_host(hiplib):
    """ossid_sym_grid_nbytes is a host function: 0 outside [1, OSSID_SYM_MAX_TARGETS], otherwise a header, the cell table
    and 16 bytes per target; tests/test_symmetry_gpu.py holds the kernels to exactly that many bytes between guard words."""
    q = hiplib.fn("ossid_sym_grid_nbytes")
    assert q(0) == 0 and q(-1) == 0 and q(hiplib.SYM_MAX_TARGETS + 1) == 0
    assert q(2) - q(1) == 16 and q(hiplib.SYM_MAX_TARGETS) == q(1) + 16 * (hiplib.SYM_MAX_TARGETS - 1)
    assert q(1) >= (2 * 32768 + 1) * 4 + 16 and q(37) % 512 != 0
