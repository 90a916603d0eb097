"""Drop-in wiring for the unchanged reference caller, scripts/online_learning.py.

    import ossid_code_amd.compat as compat
    compat.install()              # before `import ossid.scripts.online_learning`

install() registers this package's mirrors under the module paths the script imports from
(/root/reference/python/ossid/scripts/online_learning.py:18-41), so that

    from ossid.models.dtoid import DtoidNet
    from ossid.utils.zephyr_utils import networkInference
    from zephyr.datasets.score_dataset import ScoreDataset
    from zephyr.models.pointnet2 import PointNet2SSG
    from zephyr.options import getOptions
    from zephyr.utils import K2meta, meta2K, projectPointsUv
    from zephyr.utils.icp import icpRefinement
    from zephyr.utils.halcon_wrapper import PPFModel      (only with install(ppf=True); refining by default with
                                                          install(ppf=True, ppf_dense_refinement=True))
    from zephyr.utils.renderer import Renderer, blend      (only with install(renderer=True): render.Renderer, the
                                                          device rasteriser of SPEC.md section 7, depth only)
    from ossid.utils.detection import evalFinetuneResults  (only with install(det_eval=True): det_eval's, SPEC.md section 10)
    from zephyr.full_pipeline.model_featurization import FeatureModel          (only with install(sift=True): the keypoint-
    from zephyr.full_pipeline.scene_featurization import featurizeScene         feature hypotheses of --use_sift_hypos,
                                                                                features.py, SPEC.md section 11)

resolve to the MI355X path. Only these names are provided; everything else the script imports (Halcon PPF unless install(ppf=True), the
renderer unless install(renderer=True), datasets) stays with the reference / zephyr installation -- when a real `zephyr` or
`ossid` package is importable, just these attributes are overridden on it, nothing else is shadowed. The BOP evaluation the
run ends with is a script the reference shells out to, not an import: tools/eval_bop19.py (bop_eval.py, SPEC.md section 8)
takes its command line, see INTEGRATION.md.
"""
import importlib
import sys
import types


def _module(name, made=None):
    """The importable module `name`, or an empty stand-in registered under it (then noted in `made`)."""
    try:
        return importlib.import_module(name)
    except Exception:
        if made is not None:
            made.add(name)
        mod = types.ModuleType(name)
        mod.__path__ = []
        sys.modules[name] = mod
        parent, _, child = name.rpartition(".")
        if parent:
            setattr(_module(parent, made), child, mod)
        return mod


def install(ppf=False, ppf_dense_refinement=False, renderer=False, det_eval=False, sift=False):
    """ppf=True also maps zephyr.utils.halcon_wrapper.PPFModel to this build's device PPF (SPEC.md section 6), whose
    find_surface_model defaults to DensePoseRefinement='false'; with ppf_dense_refinement=True as well it maps
    ppf.PPFModelDense instead, whose default is Halcon's 'true' (SPEC.md 6.9), so the LM-O call (:446, no keyword) gets
    refined hypotheses and the YCB-V call (:418, 'false') does not. By default a user with Halcon keeps Halcon.
    renderer=True maps zephyr.utils.renderer.Renderer to render.Renderer (:485-493). The script's import line also names
    `blend`, which it never calls: when -- and only when -- no real zephyr.utils.renderer imports and the module had to
    be synthesised, render.blend (a plain alpha blend, a placeholder of unknown fidelity) is set so that the line
    imports. By default a user with pyrender keeps pyrender.
    det_eval=True maps ossid.utils.detection.{runMapEval, evalFinetuneResults} (:615-618) and
    ossid.utils.detection_metrics.DetectionMetric to det_eval's (SPEC.md section 10): the mAP the run ends with, without the
    external script. By default the reference's own stay.
    sift=True maps zephyr.full_pipeline.model_featurization.FeatureModel and
    zephyr.full_pipeline.scene_featurization.featurizeScene (:52-76, :427-435, --use_sift_hypos) to features.py's
    (SPEC.md section 11: this build's own keypoint features, not zephyr's SIFT). By default zephyr's own stay."""
    from . import dtoid, hostutil, pipeline, scoring, zephyr
    table = {
        "zephyr.datasets.score_dataset": {"ScoreDataset": zephyr.ScoreDataset},
        "zephyr.models.pointnet2": {"PointNet2SSG": zephyr.PointNet2SSG},
        "zephyr.options": {"getOptions": zephyr.getOptions},
        "zephyr.utils": {"projectPointsUv": zephyr.projectPointsUv, "K2meta": hostutil.K2meta,
                         "meta2K": hostutil.meta2K},
        "zephyr.utils.icp": {"icpRefinement": pipeline.icpRefinement},
        "ossid.utils.zephyr_utils": {"networkInference": scoring.networkInference,
                                     "filterHypoByMask": scoring.filterHypoByMask},
        "ossid.models.dtoid": {"DtoidNet": dtoid.DtoidNet},
    }
    if ppf:
        from . import ppf as ppf_mod
        cls = ppf_mod.PPFModelDense if ppf_dense_refinement else ppf_mod.PPFModel
        table["zephyr.utils.halcon_wrapper"] = {"PPFModel": cls}
    if renderer:
        from . import render
        table["zephyr.utils.renderer"] = {"Renderer": render.Renderer}
    if det_eval:
        from . import det_eval as det_mod
        table["ossid.utils.detection"] = {"runMapEval": det_mod.runMapEval, "evalFinetuneResults": det_mod.evalFinetuneResults}
        table["ossid.utils.detection_metrics"] = {"DetectionMetric": det_mod.DetectionMetric}
    if sift:
        from . import features
        table["zephyr.full_pipeline.model_featurization"] = {"FeatureModel": features.FeatureModel}
        table["zephyr.full_pipeline.scene_featurization"] = {"featurizeScene": features.featurizeScene}
    for modname, attrs in table.items():
        made = set()
        mod = _module(modname, made)
        for k, v in attrs.items():
            setattr(mod, k, v)
        if modname == "zephyr.utils.renderer" and modname in made:
            mod.blend = render.blend
    return sorted(table)
