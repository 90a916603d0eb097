"""CPU side of the PPF edge tests (SPEC.md section 6): every case of tests/ppf_cases.py holds the edge it is named after,
the float32 restatement tests/ref_ppf.py takes the decisions of the float64 geometric statement, and the array forms
added for the cases equal the forms the existing GPU tests use. Prints the premise figures and the excluded shares."""
import numpy as np
import pytest

import ppf_cases as pc
import ref_ppf as rp

STAGES = (("sample", pc.sample_cases), ("table", pc.table_cases), ("normals", pc.normals_cases), ("vote", pc.vote_cases),
          ("cluster", pc.cluster_cases))

ROWS = pc.NAMES


@pytest.mark.parametrize("stage,build", STAGES, ids=[s for s, _ in STAGES])
def test_every_premise_holds(stage, build):
    """Building asserts each premise; here: every named case exists once, and its figures are printed."""
    cases = build()
    assert sorted(c["name"] for c in cases) == sorted(ROWS[stage])
    for c in cases:
        print(c["name"], c["premise"])


def test_sizes_that_take_another_path():
    """The sizes the issue names, read off the built cases."""
    by = {c["name"]: c for _s, b in STAGES for c in b()}
    assert {by[k]["n_in"] for k in ROWS["sample"] if "_n1" in k or "blocks" in k} == {1, 1024, 1025, 1024 * 1024 + 1025}
    assert {c["Ms"] for c in pc.table_cases()} >= {1, 2, 1024, 1025, 4096}
    assert {c["premise"]["nd"] for c in pc.table_cases()} >= {1, 128} and by["t_nd1_h_above_D"]["words"] - 1 == 3375
    assert int(np.floor(float(pc.TABLE_EINVAL["D"]) / float(pc.TABLE_EINVAL["h"]))) + 1 == 129
    assert {c["Ms"] for c in pc.vote_cases()} >= {2, 1024, 1025, 2049} and {c["n"] for c in pc.vote_cases()} >= {1, 2, 512, 513, 1025}
    assert {c["nref"] for c in pc.cluster_cases()} >= {0, 1, 2, 3, 1024, 1025, 4096, 8192}
    assert {c["num_result"] for c in pc.cluster_cases()} >= {1, 100, 1025, by["c_joins_first_seed_across_rounds"]["premise"]["nseed"] + 7}


@pytest.mark.parametrize("k", range(3), ids=["g_uniform_h011_D2", "t_random", "v_model_1025"])
def test_float32_restatement_takes_the_geometric_decisions(k):
    """Validity, key and rotation bin of the f32 restatement equal those of the f64 geometric statement on every pair
    farther than 1e-5 rad / 1e-6 D from a bin edge; the excluded pairs are counted and at most 1 %."""
    name, P, N, h, D, r, i = pc.geometric_cases()[k]
    tab = rp.tables(h, D)
    e1, e2 = rp.basis(N)
    ok32, key32, bin32 = rp.feature(P[r], N[r], e1[r], e2[r], P[i], N[i], tab)
    ok64, key64, bin64, safe = rp.feature_geometric(P[r], N[r], P[i], N[i], h, D)
    share = 1.0 - safe.mean()
    keyed = safe & ok64
    wrong = int((safe & (ok32 != ok64)).sum() + (keyed & ((key32 != key64) | (bin32 != bin64))).sum())
    print("%s: %d pairs, %d keyed, excluded %.4f %%, disagreeing %d" % (name, len(r), int(keyed.sum()), 100.0 * share, wrong))
    assert share <= 0.01 and keyed.sum() >= 10000                   # at most 1 % left out, and the rest is no handful
    assert wrong == 0


@pytest.fixture(scope="module")
def scene0():
    P, N = rp.object_model()
    model = rp.Model(P, N, 0.03)
    depth, K, mask, _T = rp.scene(0)
    trace = {}
    poses, scores = rp.find(model, rp.depth2cloud(depth, mask, K), trace=trace)
    return model, trace, poses, scores


def test_array_forms_equal_todays_forms(scene0):
    """Model.from_sampled, scene_normals_radius and cluster_arrays against Model, scene_normals and cluster on a scene the
    existing tests use: the yardstick did not move."""
    model, tr, poses, scores = scene0
    m2 = rp.Model.from_sampled(model.P, model.N, model.h, model.D)
    assert np.array_equal(m2.keys, model.keys) and np.array_equal(m2.entries, model.entries) and m2.nkeys == model.nkeys
    S, Sn, Sok, cands = tr["S"], tr["normals"], tr["normals_ok"], tr["cands"]
    n2, ok2 = rp.scene_normals_radius(S, rp.F32(rp.F32(rp.NORMAL_RADIUS_REL) * tr["h"]))
    assert np.array_equal(n2, Sn) and np.array_equal(ok2, Sok)
    assert rp.vote(m2, S, Sn, Sok, 5) == cands
    votes = np.array([c[3] for c in cands])
    cp = np.array([rp.pose(model, c[1], c[2], S[c[0]], Sn[c[0]]) if c[3] > 0 else np.eye(4) for c in cands])
    p2, s2, ncand, nseed = rp.cluster_arrays(votes, cp, float(rp.F32(0.1)) * float(model.D), len(model.idx), 100)
    assert np.array_equal(p2, poses) and np.array_equal(s2, scores) and ncand == int((votes > 0).sum()) and nseed >= len(poses)
