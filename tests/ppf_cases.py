"""Inputs of the PPF edge tests (SPEC.md section 6, csrc/ppf.hip), built once and shared by the CPU tests
(tests/test_ppf_edges.py: the premises, the float32 restatement against the float64 geometric statement) and the GPU tests
(tests/test_ppf_edges_gpu.py: the five stages through the C ABI against the restatement tests/ref_ppf.py), in the manner of
tests/featurize_cases.py. The C ABI takes every stage's inputs as raw arrays, so no case comes out of a renderer.

Every builder asserts on the restatement's output that the edge it is named after occurs, and records the figures in
case["premise"]: a case cannot pass vacuously. Values that decide a comparison are exactly representable in float32
(h = 0.25, lattice points, axis normals), and every exact edge has the neighbouring float on each side.

A case is a dict: name, the arrays and scalar arguments of the entry point it drives, `want` (the restatement's outputs)
and `premise` (figures). Per stage: sample_cases(), table_cases(), normals_cases(), vote_cases(), cluster_cases()."""
import functools
import math

import numpy as np

import ref_ppf as rp

f32 = np.float32
H25 = f32(0.25)
SNT, VNT, CHUNK, CNT = 1024, 512, 1024, 1024        # csrc/ppf.hip: points per sampling block, vote / cluster workgroup, chunk
EINVAL = -22

# stage -> the names of its cases, in no particular order (the builders are run on first use; the tests parametrise
# over these names without building anything at collection time)
NAMES = {
    "sample": ("s_points_blocks1026", "s_depth_blocks1026", "s_points_n1", "s_points_n1024", "s_points_n1025", "s_depth_n1",
               "s_depth_n1024", "s_depth_n1025", "s_count_over_max_out", "s_all_invalid", "s_one_valid_diam",
               "s_one_valid_diam0", "s_depth_rules", "s_voxel_coordinates_1e6", "s_model_bad_normals"),
    "table": ("t_ms1", "t_ms2", "t_ms1024_lattice", "t_ms1025_lattice", "t_ms4096_nd128", "t_nd1_h_above_D", "t_exact_edges",
              "t_random"),
    "normals": ("n_two_and_three_neighbours", "n_neighbour_on_r2", "n_planar_patch_axis", "n_diagonal_n_dot_p_zero",
                "n_count_0", "n_count_cap", "n_count_cap_plus_1", "n_wavy_surface", "n_collinear_and_isotropic"),
    "vote": ("v_ms2_n1", "v_ms2_n2", "v_ms1024_n512_step5", "v_ms1025_n513_step1_ok_zeros_cap", "v_ms2049_n1025_step1025",
             "v_ms2049_n1025_step1026", "v_ms2049_n1025_step205", "v_no_keyed_pair", "v_plane_one_long_range",
             "v_symmetric_lattice_ties"),
    "cluster": ("c_no_candidate", "c_count_zero", "c_one_candidate", "c_generic_nref1", "c_generic_nref2", "c_generic_nref3",
                "c_generic_nref1024", "c_generic_nref1025", "c_generic_nref4096", "c_generic_nref8192", "c_count_over_cap",
                "c_8192_equal_votes_all_seeds", "c_one_cluster", "c_joins_first_seed_across_rounds",
                "c_translation_on_threshold", "c_translation_past_threshold", "c_rotation_both_sides", "c_huge_votes_and_ties"),
}


def by_name(stage):
    return {c["name"]: c for c in STAGE_BUILDERS[stage]()}


def up(x, k=1):
    x = f32(x)
    for _ in range(k):
        x = np.nextafter(x, f32(np.inf), dtype=f32)
    return x


def down(x, k=1):
    x = f32(x)
    for _ in range(k):
        x = np.nextafter(x, f32(-np.inf), dtype=f32)
    return x


def unit_normals(M, seed):
    n = np.random.default_rng(seed).normal(size=(M, 3))
    return (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(f32)


AXES = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=f32)


def lattice(nx, ny, nz, step, origin=(0.0, 0.0, 0.0)):
    g = np.stack(np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij"), -1).reshape(-1, 3)[:, ::-1]
    return (g.astype(f32) * f32(step) + np.asarray(origin, dtype=f32)).astype(f32)


# ---- sampling -----------------------------------------------------------------------------------------------------------
def sample_want(c):
    """SPEC 6.2 on a sampling case -> idx (input indices), pts, nrm (model form) of the kept points, the true count and
    stats = (lo, hi, D, h). h = f32(rel) * (diam > 0 ? diam : D); with h = 0 (one valid point and no diameter given)
    nothing is kept."""
    nrm = None
    if c["form"] == "depth":
        with np.errstate(invalid="ignore"):
            C = rp.depth2cloud(c["depth"], c["mask"], c["K"])
        src = np.flatnonzero(c["mask"].astype(bool) & (c["depth"] > 0))
        ok = rp.scene_valid(C)
    elif c.get("normals") is not None:
        C, nrm, ok = rp.prepare_model(c["points"], c["normals"])
        src = np.arange(len(C))
    else:
        C = np.asarray(c["points"], dtype=f32)
        src, ok = np.arange(len(C)), rp.scene_valid(C)
    stats = np.zeros(8, dtype=f32)
    if ok.any():
        lo, D = rp.bounds(C, ok)
        stats[0:3], stats[3:6], stats[6] = lo, C[ok].max(0), D
    stats[7] = f32(c["rel"]) * (f32(c["diam"]) if c["diam"] > 0 else stats[6])
    idx = rp.sample(C, ok, stats[7]) if (stats[7] > 0 and ok.any()) else np.zeros(0, dtype=np.int64)
    return dict(idx=src[idx].astype(np.int32), pts=C[idx], nrm=None if nrm is None else nrm[idx], count=len(idx), stats=stats)


def _scase(name, rel=0.25, diam=1.0, max_out=None, **kw):
    c = dict(name=name, rel=float(rel), diam=float(diam), form="depth" if "depth" in kw else "points", **kw)
    c["want"] = sample_want(c)
    c["n_in"] = c["depth"].size if c["form"] == "depth" else len(c["points"])
    c["max_out"] = max(c["want"]["count"], 1) + 5 if max_out is None else max_out
    c["premise"] = dict(n_in=c["n_in"], blocks=(c["n_in"] + SNT - 1) // SNT, count=c["want"]["count"], max_out=c["max_out"])
    return c


def _lattice_cloud(N, seed, cells=5):
    """scene points on voxel faces (multiples of h from 1.0), duplicates included, a few invalid"""
    rng = np.random.default_rng(seed)
    P = rng.integers(0, cells, size=(N, 3)).astype(f32) * H25 + f32(1.0)
    if N > 8:
        P[3::41, 2] = np.nan
        P[5::53, 2] = -1.0
        P[7::67, 0] = np.inf
    return P


def _block_voxel_ids(N):
    """voxel number of input i such that blocks 1024 and 1025 (of 1026) hold first-of-voxel points"""
    i = np.arange(N)
    vid = i // 4096
    late = i >= SNT * 1024
    vid[late] = 256 + (i[late] - SNT * 1024) // 512
    vid[-1] = 258
    return vid


def _depth_as_rows(P_z, K, shape):
    return dict(depth=np.ascontiguousarray(P_z.reshape(shape), dtype=f32), mask=np.ones(shape, dtype=np.uint8), K=K)


K_S = np.array([[128.0, 0.0, 3.0], [0.0, 128.0, 2.0], [0.0, 0.0, 1.0]])
K_FAR = np.array([[2.0 ** 20, 0.0, 0.0], [0.0, 2.0 ** 20, 0.0], [0.0, 0.0, 1.0]])     # x, y << h: the voxel is the depth's


@functools.lru_cache(maxsize=None)
def sample_cases():
    out = []
    for N in (1, 1024, 1025):
        c = _scase("s_points_n%d" % N, points=_lattice_cloud(N, N))
        assert c["premise"]["blocks"] == (2 if N == 1025 else 1) and c["want"]["count"] >= 1
        out.append(c)
        rng = np.random.default_rng(100 + N)
        z = (rng.integers(0, 5, size=N).astype(f32) * H25 + f32(1.0))
        if N > 8:
            z[3::41], z[5::53], z[7::67], z[9::71] = np.nan, -1.0, np.inf, 0.0
        c = _scase("s_depth_n%d" % N, **_depth_as_rows(z, K_S, (1, N)))
        if N > 8:
            c["mask"][0, 11::73] = 0
            c = _scase(c["name"], depth=c["depth"], mask=c["mask"], K=K_S)
        assert c["want"]["count"] >= 1
        out.append(c)

    # 1026 blocks: the compaction's sum over the blocks before takes a second round in blocks 0 and 1025
    N = SNT * 1024 + 1025
    vid = _block_voxel_ids(N)
    cell = np.stack([vid % 8, (vid // 8) % 8, vid // 64], 1).astype(f32)
    jit = (np.random.default_rng(5).integers(0, 4, size=(N, 3)).astype(f32) * f32(0.0625))
    P = (cell * H25 + jit + f32(1.0)).astype(f32)
    P[0] = cell[0] * H25 + f32(1.0)                       # lo = the lattice origin
    P[12345::99991, 2] = np.nan
    c = _scase("s_points_blocks1026", points=P)
    kept = c["want"]["idx"]
    c["premise"].update(kept_in_block_1024=int(((kept // SNT) == 1024).sum()), kept_in_block_1025=int(((kept // SNT) == 1025).sum()))
    assert c["premise"]["blocks"] == 1026 and c["premise"]["kept_in_block_1024"] >= 1 and c["premise"]["kept_in_block_1025"] >= 1
    assert c["want"]["count"] == 259
    out.append(c)
    z = (f32(1.0) + vid.astype(f32) * H25).astype(f32)
    z[12345::99991] = np.nan
    c = _scase("s_depth_blocks1026", **_depth_as_rows(z, K_FAR, (1057, 993)))
    kept = c["want"]["idx"]
    c["premise"].update(kept_in_block_1024=int(((kept // SNT) == 1024).sum()), kept_in_block_1025=int(((kept // SNT) == 1025).sum()))
    assert c["premise"]["blocks"] == 1026 and c["premise"]["kept_in_block_1024"] >= 1 and c["premise"]["kept_in_block_1025"] >= 1
    out.append(c)

    P = _lattice_cloud(100, 7)
    P[:, 2] = np.where(np.arange(100) % 3 == 0, np.nan, np.where(np.arange(100) % 3 == 1, f32(0.0), f32(-2.0)))
    c = _scase("s_all_invalid", points=P)
    assert c["want"]["count"] == 0 and not c["want"]["stats"][:7].any() and c["want"]["stats"][7] == H25
    out.append(c)
    P = P.copy()
    P[37] = (1.5, 2.25, 3.0)
    c = _scase("s_one_valid_diam", points=P)
    assert c["want"]["count"] == 1 and c["want"]["idx"][0] == 37 and c["want"]["stats"][6] == 0 and c["want"]["stats"][7] == H25
    out.append(c)
    c = _scase("s_one_valid_diam0", points=P, diam=0.0)          # D = 0 -> h = 0: nothing is kept (SPEC 6.2)
    assert c["want"]["count"] == 0 and c["want"]["stats"][7] == 0 and np.array_equal(c["want"]["stats"][:3], P[37])
    out.append(c)

    c = _scase("s_count_over_max_out", points=_lattice_cloud(3000, 9, cells=6), max_out=100)
    assert c["want"]["count"] > c["max_out"]
    out.append(c)

    rng = np.random.default_rng(13)
    P = (rng.integers(0, 3, size=(400, 3)).astype(f32) * H25 + f32(1.0))
    far = rng.random(400) < 0.5
    P[far] += rng.choice([f32(250000.0), f32(249999.75)], size=(int(far.sum()), 3)).astype(f32)
    P[0] = 1.0
    c = _scase("s_voxel_coordinates_1e6", points=P)
    v = np.floor((c["want"]["pts"] - c["want"]["stats"][:3]) / H25)
    c["premise"]["max_voxel_coordinate"] = float(v.max())
    assert v.max() >= 1.0e6 and np.all((P - f32(1.0)) / H25 == np.round((P - f32(1.0)) / H25))
    out.append(c)

    # the depth form's own validity rules, every kind of bad pixel next to good ones
    rng = np.random.default_rng(17)
    depth = (rng.integers(0, 4, size=(6, 9)).astype(f32) * H25 + f32(1.0))
    mask = np.ones((6, 9), dtype=np.uint8)
    mask[0, 0], mask[2, 3], mask[5, 8] = 0, 0, 0
    depth[0, 1], depth[1, 1], depth[2, 2], depth[3, 3], depth[4, 4] = 0.0, -1.5, np.nan, np.inf, -np.inf
    mask[1, 2], depth[1, 2] = 7, 3.0                                # any non-zero byte is "inside"; a voxel of its own
    c = _scase("s_depth_rules", depth=depth, mask=mask, K=K_S)
    with np.errstate(invalid="ignore"):
        C = rp.depth2cloud(depth, mask, K_S)
    c["premise"].update(pixels=54, masked_positive=len(C), finite=int(rp.scene_valid(C).sum()))
    assert len(C) == 54 - 3 - 4 and rp.scene_valid(C).sum() == len(C) - 1 and 1 * 9 + 2 in c["want"]["idx"]
    out.append(c)

    P = lattice(6, 5, 4, 0.125, (1.0, 1.0, 1.0))
    P = np.concatenate([P, P[::3] + f32(0.03125)])
    Nn = unit_normals(len(P), 3) * f32(3.0)
    Nn[4], Nn[9], Nn[17], Nn[30], Nn[31] = 0.0, (np.nan, 0, 1), (np.inf, 0, 0), (1e30, 0, 0), (0, -0.0, 1e-30)
    P[50, 1] = np.nan
    c = _scase("s_model_bad_normals", points=P, normals=Nn, rel=0.25, diam=0.5)
    _P, _N, ok = rp.prepare_model(P, Nn)
    c["premise"]["invalid_vertices"] = int((~ok).sum())
    assert (~ok).sum() == 6 and not set(c["want"]["idx"]) & {4, 9, 17, 30, 31, 50} and c["want"]["count"] > 100
    out.append(c)
    return out


def cloud_twin(c):
    """The cloud form of a depth case: the same pixels back-projected on the host (SPEC 6.2: the kept points are equal)."""
    with np.errstate(invalid="ignore"):
        C = rp.depth2cloud(c["depth"], c["mask"], c["K"])
    pix = np.flatnonzero(c["mask"].astype(bool) & (c["depth"] > 0))
    return dict(name=c["name"] + "_cloud", form="points", points=C, rel=c["rel"], diam=c["diam"], max_out=c["max_out"],
                n_in=len(C)), pix


# ---- model table --------------------------------------------------------------------------------------------------------
def _tcase(name, P, N, h, D, **premise):
    P, N = np.ascontiguousarray(P, dtype=f32), np.ascontiguousarray(N, dtype=f32)
    c = dict(name=name, P=P, N=N, h=f32(h), D=f32(D), Ms=len(P))
    m = rp.Model.from_sampled(P, N, h, D)
    c["model"], c["nch"] = m, (len(P) + CHUNK - 1) // CHUNK
    c["words"] = m.tab["nd"] * rp.NA ** 3 * c["nch"] + 1
    c["premise"] = dict(Ms=len(P), nd=m.tab["nd"], words=c["words"], entries=len(m.entries), **premise)
    return c


def decode(key):
    """key -> (dist_bin, a1, a2, a3)"""
    key = int(key)
    return key // 3375, key // 225 % 15, key // 15 % 15, key % 15


def _pair(m, r, i):
    ok, key, bn = rp.feature(m.P[r], m.N[r], m.e1[r], m.e2[r], m.P[i], m.N[i], m.tab)
    return bool(ok), (decode(key) if ok else None), int(bn)


@functools.lru_cache(maxsize=None)
def edge_model():
    """Isolated pairs (reference 2g, partner 2g + 1) stacked along z, 4 apart with D = 1: each pair pins one edge of SPEC
    6.4, with the intended outcome written beside it. -> (P, N, expect), expect[g] = (what, field, value)."""
    tab = rp.tables(H25, f32(1.0))
    T, Sn = tab["cos_a"], tab["sec_s"]
    groups = []

    def add(what, d, nr=(0, 0, 1), ni=(0, 0, 1), **expect):
        groups.append((what, np.asarray(d, dtype=f32), np.asarray(nr, dtype=f32), np.asarray(ni, dtype=f32), expect))

    for k in (1, 2, 3):                                                     # s = S_k bit for bit, and one float each side
        kh = f32(k) * H25
        add("dist_on_S%d" % k, (kh, 0, 0), db=k, s=tab["dist2"][k - 1])
        add("dist_below_S%d" % k, (down(kh), 0, 0), db=k - 1)
        add("dist_above_S%d" % k, (up(kh), 0, 0), db=k)
    add("dist_on_D", (1.0, 0, 0), db=4, s=tab["d2max"])
    add("dist_above_D", (up(1.0), 0, 0), ok=False)
    for k in (1, 7, 8, 14):                                                 # c3 = n_r . n_i = t exactly
        for what, t, a3 in (("on", T[k - 1], k), ("above", up(T[k - 1]), k - 1), ("below", down(T[k - 1]), k)):
            ni = (f32(math.sqrt(1.0 - float(t) ** 2)), 0, t)
            add("c3_%s_T%d" % (what, k), (0.5, 0, 0), ni=ni, a3=a3, c3=t)
    for k in (1, 7, 8, 14):                                                 # (u, v) = (C_k, S'_k) / 2: C_k v - S'_k u = 0 exactly
        u, v = T[k - 1] / f32(2), Sn[k - 1] / f32(2)
        add("sector_on_%d" % k, (u, v, 0), bin=k)
        add("sector_below_%d" % k, (up(u), v, 0), bin=k - 1)              # a larger u is a smaller angle (v > 0)
        add("sector_above_%d" % k, (down(u), v, 0), bin=k)
        add("sector_lower_on_%d" % k, (-u, -v, 0), bin=15 + k)
        add("sector_lower_below_%d" % k, (-up(u), -v, 0), bin=15 + k - 1)
    tiny = f32(2.0) ** -140                                                  # a denormal: d.y survives, d.y * d.y = 0
    add("v0_u_negative", (-0.5, 0, 0), bin=15)                              # the v = 0, u < 0 rule
    add("v0_u_positive", (0.5, 0, 0), bin=0)
    add("v_tiny_positive_u_negative", (-0.5, tiny, 0), bin=14)
    add("v_tiny_negative_u_negative", (-0.5, -tiny, 0), bin=15)
    add("v_tiny_negative_u_positive", (0.5, -tiny, 0), bin=29)
    add("nz_plus_zero", (0.25, 0.5, 0.25), nr=(1, 0, 0.0), ni=(0, 1, 0))
    add("nz_minus_zero", (0.25, 0.5, 0.25), nr=(1, 0, -0.0), ni=(0, 1, 0))
    add("n_plus_z", (0.25, 0.5, 0.25), nr=(0, 0, 1), ni=(0, 0, -1))
    add("n_minus_z", (0.25, 0.5, 0.25), nr=(0, 0, -1), ni=(0, 0, 1))
    P = np.zeros((2 * len(groups), 3), dtype=f32)
    N = np.zeros_like(P)
    for g, (_w, d, nr, ni, _e) in enumerate(groups):
        P[2 * g] = (0, 0, 4.0 * g)
        P[2 * g + 1] = P[2 * g] + d
        assert np.array_equal((P[2 * g + 1] - P[2 * g]).astype(f32), d)    # the offset survives the addition exactly
        N[2 * g], N[2 * g + 1] = nr, ni
    return P, N, [(g[0], g[4]) for g in groups]


@functools.lru_cache(maxsize=None)
def table_cases():
    out = []
    one = lattice(1, 1, 1, 0.25, (1, 2, 3))
    c = _tcase("t_ms1", one, AXES[4:5], 0.25, 1.0)
    assert c["premise"]["entries"] == 0
    out.append(c)
    c = _tcase("t_ms2", lattice(2, 1, 1, 0.5), AXES[[4, 0]], 0.25, 1.0)
    assert c["premise"]["entries"] == 2
    out.append(c)
    P = lattice(16, 8, 8, 0.25)
    N = AXES[np.random.default_rng(21).integers(0, 6, size=1025)]
    c = _tcase("t_ms1024_lattice", P, N[:1024], 0.25, 1.0)
    out.append(c)
    c = _tcase("t_ms1025_lattice", np.concatenate([P, [[0.125, 0.125, 0.125]]]).astype(f32), N, 0.25, 1.0)
    m = c["model"]
    c["premise"]["entries_of_the_lone_chunk"] = int(((m.entries >> 5) >= 1024).sum())
    assert c["nch"] == 2 and c["premise"]["entries_of_the_lone_chunk"] > 0
    out.append(c)

    # Ms = 4096 and ND = 128: the scan at its largest, L = 128 * 3375 * 4. Lattice step 64 h, so few pairs have a key.
    P = lattice(16, 16, 16, 16.0)
    P[1, 0] += f32(0.25)                          # (16.25, 0, 0) .. (48, 0, 0): l = 31.75 = 127 h exactly, the last bin
    c = _tcase("t_ms4096_nd128", P, unit_normals(4096, 22), 0.25, 31.875)
    m = c["model"]
    c["premise"]["top_distance_bin"] = int(m.keys.max() // 3375)
    assert c["premise"]["nd"] == 128 and c["words"] == 128 * 3375 * 4 + 1 and c["premise"]["top_distance_bin"] == 127
    out.append(c)

    c = _tcase("t_nd1_h_above_D", lattice(3, 3, 3, 0.5), unit_normals(27, 23), 4.0, 2.0)
    assert c["premise"]["nd"] == 1 and c["words"] == 3375 + 1 and c["premise"]["entries"] == 27 * 26
    out.append(c)

    P, N, expect = edge_model()
    c = _tcase("t_exact_edges", P, N, 0.25, 1.0)
    m = c["model"]
    tab = m.tab
    for g, (what, e) in enumerate(expect):
        r, i = 2 * g, 2 * g + 1
        ok, k, bn = _pair(m, r, i)
        d = (m.P[i] - m.P[r]).astype(f32)
        s = rp._dot(d, d)
        assert ok == e.get("ok", True), what
        if "s" in e:
            assert s.tobytes() == f32(e["s"]).tobytes(), what                # on the edge bit for bit
        if "db" in e:
            assert k[0] == e["db"], (what, k)
        if "c3" in e:
            assert rp._dot(m.N[r], m.N[i]).tobytes() == f32(e["c3"]).tobytes() and k[3] == e["a3"], (what, k)
        if "bin" in e:
            assert bn == e["bin"], (what, bn)
    ok, kp, bp = _pair(m, 2 * [w for w, _ in expect].index("nz_plus_zero"), 2 * [w for w, _ in expect].index("nz_plus_zero") + 1)
    ok, km, bm = _pair(m, 2 * [w for w, _ in expect].index("nz_minus_zero"), 2 * [w for w, _ in expect].index("nz_minus_zero") + 1)
    assert kp == km and bp != bm                                             # the sign of zero picks another basis
    c["premise"].update(groups=len(expect), bin_nz_plus_zero=bp, bin_nz_minus_zero=bm)
    assert c["premise"]["entries"] == 2 * len(expect) - 2                    # every pair both ways but the one beyond D
    out.append(c)

    out.append(_tcase("t_random", *rand_model(300, 24, h=0.11, D=2.0, box=2.0)))
    return out


TABLE_EINVAL = dict(name="t_nd129_einval", Ms=8, h=f32(0.25), D=f32(32.0))      # floor(D / h) + 1 = 129 bins: refused


def rand_model(Ms, seed, h=0.25, D=1.0, box=4.0):
    """Ms distinct points on a 1/64 grid in a box, random unit normals -> (P, N, h, D)"""
    rng = np.random.default_rng(seed)
    cells = rng.choice(int(box * 64) ** 3, size=Ms, replace=False)
    n = int(box * 64)
    P = (np.stack([cells % n, cells // n % n, cells // (n * n)], 1).astype(f32) / f32(64.0)).astype(f32)
    return P, unit_normals(Ms, seed + 1), f32(h), f32(D)


# ---- the float64 leg's pairs ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def geometric_cases():
    """(name, P, N, h, D, r, i): ordered pairs whose float32 decisions the float64 geometric statement must reproduce.
    Random clouds only; the exact-edge cases are pinned bit for bit instead (their pairs sit on the edges by design)."""
    out = []
    rng = np.random.default_rng(31)
    P = rng.uniform(-1.0, 1.0, size=(600, 3)).astype(f32)
    r, i = np.nonzero(~np.eye(600, dtype=bool))
    out.append(("g_uniform_h011_D2", P, unit_normals(600, 32), f32(0.11), f32(2.0), r, i))
    P, N, h, D = rand_model(300, 24, h=0.11, D=2.0, box=2.0)                  # t_random's model
    r, i = np.nonzero(~np.eye(300, dtype=bool))
    out.append(("t_random", P, N, h, D, r, i))
    P, N, h, D = rand_model(1025, 41)                                          # a vote model
    r, i = np.nonzero(~np.eye(1025, dtype=bool))
    sel = np.random.default_rng(33).choice(len(r), size=300000, replace=False)
    out.append(("v_model_1025", P, N, h, D, r[sel], i[sel]))
    return out


# ---- scene normals ------------------------------------------------------------------------------------------------------
def _ncase(name, S, radius, count=None, cap=None, loose=False, **premise):
    S = np.ascontiguousarray(S, dtype=f32).reshape(-1, 3)
    count = len(S) if count is None else count
    cap = len(S) if cap is None else cap
    buf = np.full((cap, 3), f32(5.0), dtype=f32)
    buf[:min(len(S), cap)] = S[:cap]
    n = count if count <= cap else 0
    nrm, ok = rp.scene_normals_radius(buf[:n], f32(radius))
    if not loose and ok.any():                              # well conditioned: the eigenvalue gap of every normal computed
        premise["min_gap"] = float(min(eig_gap(buf[:n], neighbours(buf[:n], i, radius)) for i in np.flatnonzero(ok)))
        assert premise["min_gap"] >= 0.05, (name, premise["min_gap"])
    c = dict(name=name, S=buf, count=count, cap=cap, radius=f32(radius), n=n, loose=loose,
             want=dict(nrm=nrm, ok=ok), premise=dict(n=n, cap=cap, ok=int(ok.sum()), **premise))
    return c


def neighbours(S, i, radius):
    r = float(f32(radius))
    d = (S - S[i]).astype(f32)
    return np.nonzero(rp._dot(d, d) <= f32(r * r))[0]


def eig_gap(S, nb):
    Q = S[nb].astype(np.float64)
    X = Q - Q.mean(0)
    w = np.linalg.eigvalsh(X.T @ X)
    return (w[1] - w[0]) / w[2]


@functools.lru_cache(maxsize=None)
def normals_cases():
    out = []
    far = 10.0
    # exactly 2 and exactly 3 neighbours (the point itself included)
    S = np.array([[0, 0, 2], [0.25, 0, 2], [far, 0, 2], [far + 0.25, 0, 2], [far, 0.25, 2.25]], dtype=f32)
    c = _ncase("n_two_and_three_neighbours", S, 0.5)
    assert [len(neighbours(S, i, 0.5)) for i in range(5)] == [2, 2, 3, 3, 3] and list(c["want"]["ok"]) == [0, 0, 1, 1, 1]
    out.append(c)
    # a third neighbour at d^2 = f32(r r) exactly, and one float beyond it
    on = np.array([[1, 1, 2], [1.25, 1, 2], [1, 1.5, 2]], dtype=f32)
    off = on.copy()
    off[2, 1] = up(1.5)
    d = (on[2] - on[0]).astype(f32)
    assert rp._dot(d, d).tobytes() == f32(0.25).tobytes()
    c = _ncase("n_neighbour_on_r2", np.concatenate([on, off + f32([far, 0, 0])]), 0.5)
    assert list(c["want"]["ok"][[0, 3]]) == [1, 0]
    out.append(c)
    # an exactly planar patch: the covariance is diagonal with a zero, the normal an axis; n.p != 0
    S = lattice(3, 3, 1, 0.25, (1, 1, 2))
    c = _ncase("n_planar_patch_axis", S, 0.625)
    assert c["want"]["ok"].all() and np.array_equal(c["want"]["nrm"], np.tile(f32([0, 0, -1]), (9, 1)))
    out.append(c)
    # diagonal covariance with the smallest eigenvalue in the middle slot, in the plane y = 0: n.p = 0 exactly, so 6.3's
    # flip does not apply and the solver's own sign stands: the kernel starts from the identity and leaves a diagonal
    # matrix alone, so it returns +y (SPEC 6.3). numpy's eigh may return either sign: the direction is compared.
    S = lattice(3, 1, 3, 0.25, (1, 0, 2))
    S[:, 0] *= f32(2.0)
    c = _ncase("n_diagonal_n_dot_p_zero", S, 1.5, loose=True)
    c["pinned"] = np.tile(f32([0, 1, 0]), (9, 1))
    assert c["want"]["ok"].all() and np.array_equal(np.abs(c["want"]["nrm"]), c["pinned"])
    out.append(c)
    # count = 0, count = cap, count = cap + 1 (nothing is valid)
    rng = np.random.default_rng(51)
    g = lattice(7, 6, 1, 0.125, (1, 1, 2)) + (rng.integers(-8, 9, size=(42, 3)).astype(f32) / f32(512.0))
    out.append(_ncase("n_count_0", g, 0.3, count=0))
    out.append(_ncase("n_count_cap", g, 0.3, count=42, cap=42))
    out.append(_ncase("n_count_cap_plus_1", g, 0.3, count=43, cap=42))
    assert out[-1]["n"] == 0 and out[-2]["want"]["ok"].all()
    # well conditioned: a wavy surface, two blocks of the kernel, rows past count in the buffer
    u, v = np.meshgrid(np.arange(20), np.arange(16))
    u, v = u.ravel() / 8.0, v.ravel() / 8.0
    S = np.stack([u - 1.2, v - 0.9, 2.0 + 0.08 * np.sin(2.0 * u) * np.cos(1.5 * v)], 1) + rng.normal(scale=0.004, size=(320, 3))
    c = _ncase("n_wavy_surface", S, 0.3, count=320, cap=331)
    assert c["want"]["ok"].all() and c["n"] > 256
    out.append(c)
    # collinear and isotropic neighbourhoods: the eigenvector is not unique (marked here, by name)
    S = np.concatenate([lattice(1, 1, 4, 0.25, (1, 1, 2)), lattice(2, 2, 2, 0.25, (far, 1, 2))])
    c = _ncase("n_collinear_and_isotropic", S, 1.0, loose=True)
    assert c["want"]["ok"].all()
    out.append(c)
    return out


# ---- vote ---------------------------------------------------------------------------------------------------------------
ROT90 = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], dtype=f32)


def _scene_of(P, N, n, seed, first=None):
    """n scene points: model points of one corner of the box turned 90 degrees about z and shifted (exact in f32), or
    random ones when the model is smaller than n"""
    rng = np.random.default_rng(seed)
    if len(P) >= n:
        near = np.argsort(np.abs(P - P.min(0)).max(1), kind="stable")[:n]
        sel = near[rng.permutation(n)]
        if first is not None:                              # model point `first` becomes scene point 0
            sel = np.concatenate([[first], sel[sel != first]])[:n]
        return (P[sel] @ ROT90.T + f32([0.5, -0.25, 3.0])).astype(f32), (N[sel] @ ROT90.T).astype(f32)
    S = (rng.integers(0, 128, size=(n, 3)).astype(f32) / f32(64.0) + f32([0, 0, 2.0])).astype(f32)
    return S, unit_normals(n, seed + 1)


def host_table(m, nch):
    """offsets u32 [nkeys * nch + 1], entries u32 as the C ABI lays them out, from the restatement's model"""
    slot = m.keys.astype(np.int64) * nch + (m.entries >> 5).astype(np.int64) // CHUNK
    order = np.argsort(slot, kind="stable")
    off = np.zeros(m.nkeys * nch + 1, dtype=np.int64)
    np.cumsum(np.bincount(slot, minlength=m.nkeys * nch), out=off[1:])
    return off.astype(np.uint32), np.ascontiguousarray(m.entries[order], dtype=np.uint32)


def _vcase(name, model, S, Sn, Sok, ref_step, cap=None, **premise):
    P, N, h, D = model
    S, Sn = np.ascontiguousarray(S, dtype=f32), np.ascontiguousarray(Sn, dtype=f32)
    n = len(S)
    cap = n if cap is None else cap
    m = rp.Model.from_sampled(P, N, h, D)
    max_ref = (cap + ref_step - 1) // ref_step
    peaks = np.zeros((max_ref, 3), dtype=np.int32)
    poses = np.tile(np.eye(4), (max_ref, 1, 1))
    Sok = np.asarray(Sok, dtype=np.uint8)
    for j, (r, m_r, al, cnt) in enumerate(rp.vote(m, S, Sn, Sok.astype(bool), ref_step)):
        if cnt > 0:
            peaks[j], poses[j] = (m_r, al, cnt), rp.pose(m, m_r, al, S[r], Sn[r])
    pad = lambda a, v: np.concatenate([a, np.full((cap - n,) + a.shape[1:], v, dtype=a.dtype)])   # noqa: E731
    c = dict(name=name, model=m, Ms=len(P), nch=(len(P) + CHUNK - 1) // CHUNK, S=pad(S, 9.0), Sn=pad(Sn, 1.0), Sok=pad(Sok, 1),
             n=n, cap=cap, ref_step=ref_step, max_ref=max_ref, want=dict(peaks=peaks, poses=poses))
    c["premise"] = dict(Ms=len(P), n=n, cap=cap, ref_step=ref_step, slots=max_ref, candidates=int((peaks[:, 2] > 0).sum()),
                        max_votes=int(peaks[:, 2].max()), **premise)
    return c


def _ties(c, r):
    """accumulator cells of reference r that equal the maximum -> (count, chunks they lie in)"""
    m = c["model"]
    acc, ln = rp.vote_acc(m, c["S"][:c["n"]], c["Sn"][:c["n"]], c["Sok"][:c["n"]].astype(bool), r)
    cells = np.flatnonzero(acc == acc.max())
    return len(cells), sorted(set((cells // rp.NALPHA // CHUNK).tolist())), ln


@functools.lru_cache(maxsize=None)
def vote_cases():
    out = []
    m2 = (lattice(2, 1, 1, 0.5), AXES[[4, 4]], H25, f32(1.0))
    c = _vcase("v_ms2_n1", m2, [[0, 0, 2]], [[0, 0, -1]], [1], 1, cap=4)
    assert c["premise"]["candidates"] == 0
    out.append(c)
    c = _vcase("v_ms2_n2", m2, [[0, 0, 2], [0, 0.5, 2]], [[0, 0, -1], [0, 0, -1]], [1, 1], 1)
    assert c["premise"]["candidates"] == 2
    out.append(c)

    mod = rand_model(1024, 40)
    S, Sn = _scene_of(mod[0], mod[1], 512, 60)
    c = _vcase("v_ms1024_n512_step5", mod, S, Sn, np.ones(512), 5)
    assert c["premise"]["candidates"] > 50 and c["premise"]["max_votes"] >= 5
    out.append(c)

    mod = rand_model(1025, 41)
    S, Sn = _scene_of(mod[0], mod[1], 513, 61, first=1024)
    ok = np.ones(513, dtype=np.uint8)
    ok[[1, 7, 8, 100, 511, 512]] = 0                       # references dropped; partners dropped at both ends of a round
    c = _vcase("v_ms1025_n513_step1_ok_zeros_cap", mod, S, Sn, ok, 1, cap=520)
    p = c["want"]["peaks"]
    c["premise"]["peaks_in_the_lone_chunk"] = int(((p[:, 0] >= 1024) & (p[:, 2] > 0)).sum())
    assert not p[[1, 7, 8, 100, 511, 512]].any() and not p[513:].any() and c["premise"]["candidates"] > 300
    assert p[0, 0] == 1024 and p[0, 2] > 0                 # the peak of reference 0 is the chunk's only model point
    out.append(c)

    mod = rand_model(2049, 42)
    S, Sn = _scene_of(mod[0], mod[1], 1025, 62, first=2048)
    for step, cap in ((1025, 1025), (1026, 1030), (205, 1025)):
        c = _vcase("v_ms2049_n1025_step%d" % step, mod, S, Sn, np.ones(1025), step, cap=cap)
        assert c["premise"]["candidates"] == (1025 + step - 1) // step and c["want"]["peaks"][0, 0] == 2048
        out.append(c)
    assert out[-2]["max_ref"] == 2 and not out[-2]["want"]["peaks"][1].any()        # ref_step = n + 1: slot 1 is past n

    # no pair with a key: points farther than D apart, and coincident points (s = 0)
    S = lattice(4, 3, 1, 1.5, (0, 0, 2))
    S = np.concatenate([S, S[:5]])
    c = _vcase("v_no_keyed_pair", rand_model(1024, 40), S, unit_normals(len(S), 63), np.ones(len(S)), 1)
    assert c["premise"]["candidates"] == 0
    out.append(c)

    # a flat plane: one key holds every pair (ND = 1, equal normals), its range is far longer than one 512-entry round
    Pm = lattice(15, 10, 1, 0.25)
    mod = (Pm, np.tile(AXES[4], (150, 1)), f32(16.0), f32(8.0))
    S = lattice(8, 5, 1, 0.25, (-1, -1, 2))
    c = _vcase("v_plane_one_long_range", mod, S, np.tile(AXES[5], (40, 1)), np.ones(40), 7)
    cnt, chunks, ln = _ties(c, 0)
    c["premise"].update(longest_range=int(ln.max()), ties_at_max=cnt)
    assert ln.max() >= 20000 and len(np.unique(c["model"].keys)) == 1
    out.append(c)

    # a symmetric lattice: interior model points have equal neighbourhoods, so their accumulator rows tie, in both chunks
    Pm = np.concatenate([lattice(64, 32, 1, 0.25), [[20.0, 20.0, 0.0]]]).astype(f32)
    mod = (Pm, np.tile(AXES[4], (2049, 1)), H25, f32(1.0))
    S = lattice(9, 9, 1, 0.25, (-1, -1, 2))
    c = _vcase("v_symmetric_lattice_ties", mod, S, np.tile(AXES[5], (81, 1)), np.ones(81), 40)
    cnt, chunks, _ln = _ties(c, 40)
    c["premise"].update(ties_at_max=cnt, chunks_with_a_tie=chunks)
    assert cnt >= 64 and chunks == [0, 1] and c["want"]["peaks"][1, 0] < 1024      # the runner-up lies in another chunk
    out.append(c)
    return out


# ---- cluster ------------------------------------------------------------------------------------------------------------
def rot_z(c):
    """rotation about z with cos = c exactly"""
    s = math.sqrt(1.0 - c * c)
    T = np.eye(4)
    T[0, 0], T[0, 1], T[1, 0], T[1, 1] = c, -s, s, c
    return T


def at(x, y=0.0, z=0.0, R=None):
    T = np.eye(4) if R is None else R.copy()
    T[:3, 3] = (x, y, z)
    return T


def trace_cos(Ta, Tb):
    tr = 0.0
    for a in range(3):
        for b in range(3):
            tr += Ta[a, b] * Tb[a, b]
    return (tr - 1.0) / 2.0


def _ccase(name, votes, poses, num_result=100, ref_step=1, count=None, cap=None, Ms=1000, D=1.0, dist_rel=0.25, **premise):
    """votes / poses: the nref candidate rows. Rows past nref (up to max_ref) are non-zero garbage."""
    votes = np.asarray(votes, dtype=np.int64)
    nref = len(votes)
    count = (nref - 1) * ref_step + 1 if count is None else count
    count = max(count, 0) if nref else 0
    cap = min(max(count, 1) + 3 * ref_step, 8192) if cap is None else cap
    max_ref = (cap + ref_step - 1) // ref_step
    n = count if count <= cap else 0
    live = min((n + ref_step - 1) // ref_step, max_ref)
    peaks = np.full((max_ref, 3), 12345, dtype=np.int32)
    cp = np.full((max_ref, 4, 4), 3.5)
    k = min(nref, max_ref)
    peaks[:k, 0], peaks[:k, 1], peaks[:k, 2] = np.arange(k) % 1000, np.arange(k) % 30, votes[:k]
    cp[:k] = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)[:k]
    thr = float(f32(dist_rel)) * float(f32(D))
    P, Sc, ncand, nseed = rp.cluster_arrays(peaks[:live, 2], cp[:live], thr, Ms, num_result)
    c = dict(name=name, peaks=peaks, cand_poses=cp, count=count, cap=cap, ref_step=ref_step, Ms=Ms, D=f32(D), dist_rel=f32(dist_rel),
             num_result=num_result, nref=live, max_ref=max_ref,
             want=dict(poses=P, scores=Sc, info=np.array([len(P), count, ncand, nseed], dtype=np.int32)))
    c["premise"] = dict(nref=live, max_ref=max_ref, ncand=ncand, nseed=nseed, num_result=num_result, results=len(P), **premise)
    return c


def _generic_cluster(nref, seed, **kw):
    """random candidates around a few group poses: translations near each other, rotations on both sides of 12 degrees,
    votes with many ties and some zeros"""
    rng = np.random.default_rng(seed)
    G = max(1, min(40, nref // 3))
    centre = rng.integers(-8, 9, size=(G, 3)) * 0.5
    g = rng.integers(0, G, size=nref)
    poses = np.zeros((nref, 4, 4))
    for j in range(nref):
        poses[j] = at(*(centre[g[j]] + rng.integers(-3, 4, size=3) / 16.0), R=rot_z(math.cos(math.radians(rng.choice([0.0, 5.0, 11.0, 13.0, 30.0])))))
    votes = rng.integers(0, 6, size=nref) * rng.integers(1, 4, size=nref)
    return _ccase("c_generic_nref%d" % nref, votes, poses, **kw)


@functools.lru_cache(maxsize=None)
def cluster_cases():
    out = []
    I = np.eye(4)
    c = _ccase("c_no_candidate", [0, 0, 0, 0, 0], [I] * 5)
    assert c["premise"]["ncand"] == 0 and c["premise"]["results"] == 0
    out.append(c)
    c = _ccase("c_count_zero", [], np.zeros((0, 4, 4)), cap=6)
    assert c["nref"] == 0
    out.append(c)
    c = _ccase("c_one_candidate", [0, 0, 7, 0], [I, I, at(1, 2, 3), I], num_result=1)
    assert c["premise"]["ncand"] == 1 and c["premise"]["results"] == 1
    out.append(c)
    for nref, kw in ((1, {}), (2, {}), (3, {}), (1024, dict(ref_step=2)), (1025, dict(num_result=1)), (4096, dict(ref_step=2)),
                     (8192, dict(num_result=1025))):
        c = _generic_cluster(nref, 70 + nref, **kw)
        if nref >= 1024:
            assert c["premise"]["nseed"] > 128
        out.append(c)
    c = _generic_cluster(1025, 99, count=5000, cap=4999)
    c["name"] = "c_count_over_cap"
    assert c["nref"] == 0 and c["want"]["info"].tolist() == [0, 5000, 0, 0]
    out.append(c)

    # 8192 equal votes, all far apart: every candidate is a seed, both sorts run at 8192, the output is in index order
    far = lattice(32, 16, 16, 1.0).astype(np.float64)
    c = _ccase("c_8192_equal_votes_all_seeds", np.full(8192, 3), [at(*p) for p in far], num_result=8192 + 7)
    assert c["premise"]["nseed"] == 8192 and np.array_equal(c["want"]["poses"][:, :3, 3], far)
    out.append(c)
    c = _ccase("c_one_cluster", np.arange(1, 301), [at(0.01 * (j % 7), 0, 0) for j in range(300)])
    assert c["premise"]["nseed"] == 1 and c["want"]["scores"][0] == 300 * 301 / 2 / 1000
    out.append(c)

    # more than 1024 seeds; the last candidates lie within reach of an early seed and of a later one, in another round of
    # the seed loop (3 and 1030) or another wave of the same round (2 and 70): each joins the earlier seed
    ns = 1100
    line = [at(2.0 * j, 0, 0) for j in range(ns)]
    line[1030] = at(2.0 * 3 + 0.4, 0, 0)
    line[70] = at(2.0 * 2, 0.4, 0)
    votes = [10 * (5000 - j) for j in range(ns)] + [3, 2, 1]          # the third: within reach of seed 1050 alone
    c = _ccase("c_joins_first_seed_across_rounds", votes,
               line + [at(2.0 * 3 + 0.2, 0, 0), at(2.0 * 2, 0.2, 0), at(2.0 * 1050, 0.2, 0)], num_result=ns + 7)
    w = c["want"]
    assert c["premise"]["nseed"] == ns > CNT and c["num_result"] == c["premise"]["nseed"] + 7
    assert w["scores"][3] == (49970 + 3) / 1000 and w["scores"][2] == (49980 + 2) / 1000
    assert w["scores"][1030] == 39700 / 1000 and w["scores"][70] == 49300 / 1000 and w["scores"][1050] == (39500 + 1) / 1000
    out.append(c)

    # the translation test at d^2 = thr^2 exactly (D = 1, dist_rel = 0.25, dx = 0.25) and one float beyond it
    step = float(np.nextafter(0.25, 1.0))
    c = _ccase("c_translation_on_threshold", [9, 5, 4], [I, at(0.25), at(10 + step)], num_result=100)
    c2 = _ccase("c_translation_past_threshold", [9, 5, 8], [I, at(step), at(10)], num_result=100)
    assert 0.25 * 0.25 == float(f32(0.25)) ** 2 and step * step > 0.0625
    assert c["want"]["scores"].tolist() == [0.014, 0.004] and c2["want"]["scores"].tolist() == [0.009, 0.008, 0.005]
    out += [c, c2]

    # the rotation test on both sides of cos(pi / 15): the f64 cosines whose (tr - 1) / 2, summed as written, land there
    lo = hi = None
    x = rp.CLUSTER_COS
    for _ in range(8):
        if trace_cos(rot_z(x), I) >= rp.CLUSTER_COS and hi is None:
            hi = x
        x = float(np.nextafter(x, 2.0))
    x = rp.CLUSTER_COS
    for _ in range(8):
        x = float(np.nextafter(x, 0.0))
        if trace_cos(rot_z(x), I) < rp.CLUSTER_COS and lo is None:
            lo = x
    assert hi is not None and lo is not None and trace_cos(rot_z(hi), I) >= rp.CLUSTER_COS > trace_cos(rot_z(lo), I)
    c = _ccase("c_rotation_both_sides", [9, 5, 4], [I, rot_z(hi), rot_z(lo)], num_result=100, cos_in=hi, cos_out=lo,
               cos_in_minus_threshold=trace_cos(rot_z(hi), I) - rp.CLUSTER_COS, cos_out_minus_threshold=trace_cos(rot_z(lo), I) - rp.CLUSTER_COS)
    assert c["want"]["scores"].tolist() == [0.014, 0.004]
    out.append(c)

    # votes up to 2^30 with ties (order by reference index), cluster sums that tie (order by seed), sums up to 3 * 2^30
    big = 1 << 30
    votes = [big, 7, big, big, 7, big - 1, 1, big]
    poses = [at(0), at(5), at(0.1), at(9), at(5.1), at(20), at(20.1), at(0.2)]
    c = _ccase("c_huge_votes_and_ties", votes, poses, Ms=1)
    assert c["want"]["scores"].tolist() == [3.0 * big, float(big), float(big), 14.0]
    assert np.array_equal(c["want"]["poses"][:, 0, 3], [0.0, 9.0, 20.0, 5.0])       # equal sums keep the seeds' order
    out.append(c)
    return out


STAGE_BUILDERS = dict(sample=sample_cases, table=table_cases, normals=normals_cases, vote=vote_cases, cluster=cluster_cases)
