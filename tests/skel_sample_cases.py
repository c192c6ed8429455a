"""Inputs shared by the skeleton-sample tests (host and GPU): those of tests/skel_cov_cases.py by name, each with the banded
matrix and pin set of tests/skel_cov_ref.py, built once per process.  Test infrastructure."""
import os

import numpy as np

import pinhole_fte_ref as pref
import skel_cov_cases as cases
import skel_sample_ref as sref

NAMES = ("golden", "slice40", "slice40pin", "slice100", "slice12", "p51", "pt16", "pt16b", "pt16pin", "pt32")
# the sub-tree inputs (cases.SUB_TREES; 12 frames): name -> (PT, first frame, camera model)
SUB_TREE_CASES = {"pt16": (16, cases.SLICE_STARTS[0], "fisheye"), "pt16b": (16, cases.SLICE_STARTS[1], "fisheye"),
                  "pt16pin": (16, cases.SLICE_STARTS[0], "pinhole"), "pt32": (32, cases.SLICE_STARTS[0], "fisheye")}
_CACHE = {}


def scene(g, camera_model="fisheye"):
    if camera_model == "pinhole":
        return g["K"], np.tile(pref.D5, (len(g["K"]), 1)), g["R"], g["t"]
    return g["K"], g["D"], g["R"], g["t"]


def fixture(golden_dir):
    g, sk = cases.load(golden_dir)
    det = np.load(os.path.join(golden_dir, "human_dlc_slice.npz"))["det"].astype(np.float64)
    return g, sk, det


def case(golden_dir, name):
    """dict(model, x, prob, sk, ab, fixed): "p51" is the 51-state skeleton (PT 64) on 24 frames, "slice12" the 12-frame slice at
    frame 60, "pt16" .. "pt32" the sub-trees of SUB_TREE_CASES, the others the inputs of the covariance tests."""
    if name in _CACHE:
        return _CACHE[name]
    g, sk0, det = fixture(golden_dir)
    if name == "p51":
        sk = cases.generic_skeleton(sk0, extra=5)
        det5, parts5 = cases.with_extra_detections(det, g["parts"], 5)
        cam, sc = "fisheye", scene(g)
        model = cases.make_model(g, sk, det5, 24, 60, parts=parts5)
    elif name in SUB_TREE_CASES:
        pt, sf, cam = SUB_TREE_CASES[name]
        sk, sc = cases.sub_skeleton(cases.generic_skeleton(sk0), cases.SUB_TREES[pt]), scene(g, cam)
        model = cases.make_model(g, sk, det, 12, sf, cam, sc)
    else:
        sk = cases.generic_skeleton(sk0)
        src, n, sf, cam = {"golden": (g["det"], int(g["n_frames"]), int(g["start_frame"]), "fisheye"),
                           "slice40": (det, 40, cases.SLICE_STARTS[0], "fisheye"),
                           "slice40pin": (det, 40, cases.SLICE_STARTS[0], "pinhole"),
                           "slice100": (det, 100, 60, "fisheye"),
                           "slice12": (det, 12, 60, "fisheye")}[name]
        sc = scene(g, cam)
        model = cases.make_model(g, sk, src, n, sf, cam, sc)
    x = cases.iterate(g, model)
    prob = cases.problem(sk, model, sc, cam)
    cases.assert_observed(prob, x[:, prob.ACT])
    ab, fixed = sref.system(prob, x[:, prob.ACT])
    _CACHE[name] = dict(model=model, x=x, prob=prob, sk=sk, scene=sc, cam=cam, ab=ab, fixed=fixed)
    return _CACHE[name]


def normal_z(c, S, seed=5):
    return np.random.default_rng(seed).standard_normal((S,) + c["fixed"].shape)
