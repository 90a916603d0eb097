"""Where SPEC.md section 17 plugs in, on the device: SceneBatch.write_bop(symmetries=True) on a folder with a lathe, read
back by the evaluation (a pose turned about the lathe's axis is correct under MSSD with the found symmetry and wrong
without), and OnlineStream(symmetries="auto"), whose process() hands the found transforms to the distinct-pose selection
and scores the object with ADI."""
import json
import os

import numpy as np
import pytest
import torch

import ref_pose_select as rp
import ref_symmetry as rs
from guarded import ready, sync
from ossid_code_amd import bop_eval, pipeline, render, scenes, scoring, symmetry, synth

pytestmark = pytest.mark.gpu


def _lathe_mesh(scale, segments=96):
    prof = np.asarray(rs.LATHE_PROFILE, dtype=np.float64) * scale
    th = 2.0 * np.pi * np.arange(segments) / segments
    V = np.concatenate([np.stack([r * np.cos(th), r * np.sin(th), np.full(segments, z)], 1) for r, z in prof])
    F = []
    for k in range(len(prof) - 1):
        for i in range(segments):
            a, b, c, d = k * segments + i, k * segments + (i + 1) % segments, (k + 1) * segments + i, (k + 1) * segments + (i + 1) % segments
            F += [[a, b, d], [a, d, c]]
    C = np.full((len(V), 3), 160, np.uint8)
    C[V[:, 0] > 0] = (200, 60, 60)                              # the colour breaks the symmetry; it is not looked at (17.6)
    return render.Mesh(V, np.asarray(F, dtype=np.int32), colors=C)


def test_write_bop_finds_the_lathes_axis_and_the_evaluation_uses_it(hiplib, tmp_path):
    ready()
    atlas = scenes.MeshAtlas({1: _lathe_mesh(0.1)})             # metres: 0.1 m tall
    hw = (120, 160)
    K = synth.CAM_K * np.array([[hw[1] / 640.0], [hw[0] / 480.0], [1.0]])
    layout = scenes.sample_layouts(atlas, 2, 1, K, hw, np.random.default_rng(3))
    batch = scenes.render_scenes(atlas, layout, hw)
    roots = {tag: batch.write_bop(str(tmp_path / tag), "synth", symmetries=flag) for tag, flag in (("plain", False), ("sym", True))}
    sync()
    info = {tag: json.load(open(os.path.join(root, "models_eval", "models_info.json"))) for tag, root in roots.items()}
    assert "symmetries_continuous" not in info["plain"]["1"] and "symmetries_discrete" not in info["plain"]["1"]
    entry = info["sym"]["1"]
    assert {k: entry[k] for k in info["plain"]["1"]} == info["plain"]["1"] and "symmetries_discrete" not in entry
    (cont,) = entry["symmetries_continuous"]
    axis, offset = np.asarray(cont["axis"]), np.asarray(cont["offset"])
    assert abs(axis[2]) > np.cos(2.0 * symmetry.grid_spacing(4)) and abs(np.linalg.norm(axis) - 1.0) < 1e-9
    # millimetres: on the axis (within a hundredth of the 122 mm diameter), between the ends of the 100 mm profile
    assert np.hypot(offset[0], offset[1]) < 0.01 * entry["diameter"] and -50.0 < offset[2] < 50.0 and 100.0 < entry["diameter"] < 150.0
    turn = np.eye(4)
    turn[:2, :2] = [[0.0, -1.0], [1.0, 0.0]]                    # 90 degrees about the lathe's axis
    scores = {}
    for tag, root in roots.items():
        rows = []
        for s in range(2):
            for g in json.load(open(os.path.join(root, "test", "%06d" % s, "scene_gt.json")))["0"]:
                T = np.eye(4)
                T[:3, :3], T[:3, 3] = np.asarray(g["cam_R_m2c"]).reshape(3, 3), np.asarray(g["cam_t_m2c"]) / 1000.0
                rows.append({"scene_id": s, "im_id": 0, "obj_id": g["obj_id"], "score": 1.0, "pose": T @ turn})
        csv = pipeline.save_results_bop(rows, str(tmp_path / tag), "turned", "synth")
        scores[tag] = bop_eval.evaluate(bop_eval.read_results_csv(csv), bop_eval.BopFolder(str(tmp_path / tag), "synth", "test"))
        print(tag, {k: scores[tag][k] for k in ("AR_VSD", "AR_MSSD", "AR_MSPD", "AR")})
    assert scores["sym"]["AR_MSSD"] == 1.0 and scores["plain"]["AR_MSSD"] == 0.0
    assert scores["sym"]["AR_MSPD"] > scores["plain"]["AR_MSPD"]


class _Args:
    dataset, no_valid_proj, no_valid_depth, inconst_ratio_th, interp = "HSVD_diff_uv_norm", True, True, 100, 0


def test_process_passes_the_found_symmetries_on(hiplib):
    """A box's mesh beside synth's frame: with symmetries="auto" the selection is the restatement's WITH the box's four
    transformations and the errors are ADI; without, the selection has none and the errors are ADD."""
    from ossid_code_amd import dtoid, zephyr
    from ossid_code_amd.stream import OnlineStream
    ready()
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
    a, b, c = 0.05, 0.03, 0.015
    V = [[sx * a, sy * b, sz * c] for sz in (-1, 1) for sy in (-1, 1) for sx in (-1, 1)]
    F = [[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]]
    box = render.Mesh(np.asarray(V, dtype=np.float64), np.asarray(F, dtype=np.int32), colors=np.full((8, 3), 160, np.uint8))
    out = {}
    for tag, sym in (("auto", "auto"), ("none", None)):
        st = OnlineStream(det, scorer, ds, confident_threshold=-1e30, max_instances=2, instance_sep_rel=1.5, meshes={1: box},
                          symmetries=sym)
        out[tag] = (st.process(dict(frame)), st)
    sync()
    S = out["auto"][1]._symmetries(1)
    assert S.shape == (4, 4, 4)                                 # the identity and the box's three half-turns
    data = {k: frame[k] for k in ("img", "depth", "cam_K", "model_points", "model_normals", "model_colors", "pose_hypos")}
    poses, scores, _errs, _uv = scoring.networkInference(scorer, ds, data)
    sep = 1.5 * out["auto"][1]._diameter(frame)
    for tag, syms, symmetric in (("auto", S, True), ("none", None, False)):
        r = out[tag][0]
        want = rp.select(poses, scores, frame["model_points"], 2, sep, symmetries=syms)
        assert np.array_equal(r["selected"], want[0]) and np.array_equal(r["owner"], want[2]), tag
        errs = scoring.pose_errors(frame["pose_hypos"], frame["pose_gt"], frame["model_points"], symmetric)
        assert r["pred_err"] == float(np.asarray(errs)[int(r["selected"][0])]), tag
    adi = scoring.pose_errors(frame["pose_hypos"], frame["pose_gt"], frame["model_points"], True)
    add = scoring.pose_errors(frame["pose_hypos"], frame["pose_gt"], frame["model_points"], False)
    assert not np.array_equal(np.asarray(adi), np.asarray(add))
