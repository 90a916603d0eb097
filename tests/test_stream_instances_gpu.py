"""OnlineStream(max_instances=K): the estimating half of targets with several instances. Random-weight nets on a synthetic
frame whose hypotheses are synth's 64 around the sphere plus a copy of them 0.3 m to the right: with max_instances=2 pick 0
and every single-instance key equal the max_instances=1 result bit for bit, selected / owner equal the restatement
(tests/ref_pose_select.py) on the scored poses, the second pick is another object in space; max_instances=1 changes
nothing; a [2,4,4] pose_gt gives the minimum of the two single-gt errors."""
import numpy as np
import pytest
import torch

import ref_pose_select as rp
from ossid_code_amd import scoring, synth

pytestmark = pytest.mark.gpu

SEP_REL = 1.5                   # x the sphere's 0.1 m diameter: wider than one cloud of hypotheses, half the 0.3 m between the two
OLD_KEYS = {"pred_pose", "pred_score", "pred_err", "confident", "dtoid_score", "dtoid_bbox", "pred_mask_visib", "sample"}


class _Args:
    dataset, no_valid_proj, no_valid_depth, inconst_ratio_th, interp = "HSVD_diff_uv_norm", True, True, 100, 0


@pytest.fixture(scope="module")
def world(hiplib):
    from ossid_code_amd import dtoid, zephyr
    from ossid_code_amd.stream import OnlineStream
    torch.manual_seed(0)
    det = dtoid.DtoidNet(dtoid.DtoidConfig()).cuda().eval()
    ds = zephyr.ScoreDataset([], "", "lmo", _Args(), mode="test")
    scorer = synth.random_pn2_state(zephyr.PointNet2SSG(ds.dim_point, _Args(), num_class=1), 0).to(0).eval()
    g = torch.Generator().manual_seed(1)
    frame = synth.make_scoring_inputs(64, 512, seed=200)
    moved = frame["pose_hypos"].copy()
    moved[:, 0, 3] += 0.3
    frame["pose_hypos"] = np.concatenate([frame["pose_hypos"], moved])
    frame.update(limg=torch.rand(3, 3, 124, 124, generator=g), lmask=(torch.rand(3, 1, 124, 124, generator=g) > 0.5).float(),
                 obj_id=1, pose_gt=frame["pose_hypos"][0].copy())

    def run(max_instances, icp, **over):
        st = OnlineStream(det, scorer, ds, confident_threshold=-1e30, icp_max_dist=0.01 if icp else None,
                          max_instances=max_instances, instance_sep_rel=SEP_REL)
        return st.process({**frame, **over}), st
    return {"frame": frame, "scorer": scorer, "ds": ds, "run": run, "cache": {}}


def _result(world, max_instances, icp):
    key = (max_instances, icp)
    if key not in world["cache"]:
        world["cache"][key] = world["run"](max_instances, icp)
    return world["cache"][key]


def _same(a, b):
    """Bit for bit, whatever the value is: tensors, arrays, floats, dicts of them, None."""
    if isinstance(a, dict):
        return isinstance(b, dict) and set(a) == set(b) and all(_same(a[k], b[k]) for k in a)
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    if isinstance(a, float):
        return isinstance(b, float) and np.float64(a).tobytes() == np.float64(b).tobytes()
    return type(a) is type(b) and a == b


@pytest.mark.parametrize("icp", [False, True])
def test_two_instances_keep_the_single_instance_result(world, icp):
    one, st1 = _result(world, 1, icp)
    two, st2 = _result(world, 2, icp)
    old = OLD_KEYS | ({"icp"} if icp else set())
    # max_instances = 1: no new key, no new timer
    assert set(one) == old and "select" not in st1.times
    assert set(two) == old | {"selected", "owner", "instances"} and st2.times["select"] > 0
    assert set(st2.times) == set(st1.times) | {"select"}
    for k in sorted(old):
        assert _same(two[k], one[k]), k
    assert len(two["instances"]) == 2
    first = two["instances"][0]
    assert set(first) == {"pred_pose", "pred_score", "pred_err", "confident", "pred_mask_visib", "sample"} | ({"icp"} if icp else set())
    for k in first:
        assert _same(first[k], one[k]), k
    # selected and owner are the restatement's on the poses and scores the scorer returned for this frame
    frame = world["frame"]
    data = {k: frame[k] for k in ("img", "depth", "cam_K", "model_points", "model_normals", "model_colors", "pose_hypos")}
    poses, scores, _errs, _uv = scoring.networkInference(world["scorer"], world["ds"], data)
    sep = SEP_REL * 0.1
    assert abs(st2._diameter(frame) - 0.1) < 1e-3                     # the sphere's, from its 512 points
    want = rp.select(poses, scores, frame["model_points"], 2, SEP_REL * st2._diameter(frame))
    assert two["selected"].dtype == two["owner"].dtype == np.int32
    assert np.array_equal(two["selected"], want[0]) and np.array_equal(two["owner"], want[2]) and want[1][0] == 2
    a, b = (int(v) for v in two["selected"])
    assert a == int(scores.argmax()) and a // 64 != b // 64           # one pick in each cloud of hypotheses
    D = rp.distances(poses, a, frame["model_points"], np.eye(4)[None])
    print("picks", a, b, "D", float(np.sqrt(D[b])), "sep", sep, "owned", np.bincount(two["owner"] + 1).tolist())
    assert D[b] > (SEP_REL * st2._diameter(frame)) ** 2
    second = two["instances"][1]
    src = second["icp"]["pose_unrefined"] if icp else second["pred_pose"]
    assert np.array_equal(src, poses[b]) and second["pred_score"] == float(np.asarray(scores).reshape(-1)[b])
    assert second["confident"] and second["sample"] is not None and second["pred_mask_visib"].dtype == torch.bool
    if icp:
        assert second["icp"]["iterations"] >= 1 and not np.array_equal(second["pred_pose"], src)


def test_frames_with_one_instance_take_the_old_path(world):
    one, _ = _result(world, 1, False)
    r, st = world["run"](2, False, inst_count=1)
    assert set(r) == OLD_KEYS and all(_same(r[k], one[k]) for k in OLD_KEYS) and st.times["select"] == 0.0


def test_error_against_several_ground_truths_is_the_minimum(world):
    frame = world["frame"]
    A, B = frame["pose_hypos"][0].copy(), frame["pose_hypos"][64].copy()
    ra, _ = _result(world, 2, False)                                  # pose_gt = A
    rb, _ = world["run"](2, False, pose_gt=B)
    rab, _ = world["run"](2, False, pose_gt=np.stack([A, B]))
    assert np.array_equal(rab["selected"], ra["selected"]) and np.array_equal(rab["selected"], rb["selected"])
    for i in range(2):
        ea, eb, eab = (r["instances"][i]["pred_err"] for r in (ra, rb, rab))
        print(i, ea, eb, eab)
        assert eab == min(ea, eb) and ea != eb
    assert rab["pred_err"] == rab["instances"][0]["pred_err"]
    # each pick is nearest its own cloud's ground truth
    assert {rab["instances"][i]["pred_err"] == ra["instances"][i]["pred_err"] for i in range(2)} == {True, False}
