"""Inputs shared by the observability tests (host and GPU), built once per process on top of tests/skel_cov_cases.py.  Test
infrastructure.  r_meas = 0.3 as there; the iterate is ``skel_cov_cases.iterate`` (seed 0); frames 60 .. of human_dlc_slice.npz.

  shipped40 / shipped12   the shipped human skeleton, UNMODIFIED (two psi states that move no pose)
  lost12 / lost40         ``generic_skeleton``, the weights of elbow1 and wrist1 set to 0 in every frame (six states unobserved)
  lost12pin               lost12 on the pinhole camera
  lost12p51               ``generic_skeleton(extra=5)`` (51 active states, PT = 64: the input of the covariance tests' P > 48
                          case, 12 frames), same lost limb
  two12                   lost12 with the limb detected in frames 0 and 1 only: nothing unobserved, singular all the same
  slice40                 the covariance tests' fully observed window"""
import copy
import os

import numpy as np

import skel_cov_cases as cases
import skel_sample_cases as scases
import skel_unobs_ref as uref

LIMB = ("elbow1", "wrist1")
NAMES = ("shipped40", "shipped12", "lost12", "lost40", "lost12pin", "lost12p51", "two12", "slice40")
_CACHE = {}


def lose_limb(model, keep_frames=0):
    """A copy of the model whose detections of elbow1 and wrist1 carry weight 0 from frame ``keep_frames`` on."""
    m = copy.copy(model)
    names = list(model.names)
    m.weights = model.weights.copy()
    m.weights[keep_frames:, :, [names.index(k) for k in LIMB]] = 0.0
    return m


def case(golden_dir, name):
    """dict(model, x, prob, sk, scene, cam, ref): ``ref`` is skel_unobs_ref.reference(prob, xa) (no inverse yet: ``solved``)."""
    if name in _CACHE:
        return _CACHE[name]
    g, sk0, det = scases.fixture(golden_dir)
    cam = "pinhole" if name.endswith("pin") else "fisheye"
    sc = scases.scene(g, cam)
    n = 40 if name.endswith("40") else 12
    if name.startswith("shipped"):
        sk = sk0
        model = cases.make_model(g, sk, det, n, cases.SLICE_STARTS[0], cam, sc)
    elif name == "lost12p51":
        sk = cases.generic_skeleton(sk0, extra=5)
        det5, parts5 = cases.with_extra_detections(det, g["parts"], 5)
        model = lose_limb(cases.make_model(g, sk, det5, n, cases.SLICE_STARTS[0], parts=parts5))
    else:
        sk = cases.generic_skeleton(sk0)
        model = cases.make_model(g, sk, det, n, cases.SLICE_STARTS[0], cam, sc)
        if name.startswith("lost"):
            model = lose_limb(model)
        elif name == "two12":
            model = lose_limb(model, keep_frames=2)
    x = cases.iterate(g, model)
    prob = cases.problem(sk, model, sc, cam)
    _CACHE[name] = dict(model=model, x=x, prob=prob, sk=sk, scene=sc, cam=cam, ref=uref.reference(prob, x[:, prob.ACT]))
    return _CACHE[name]


def solved(golden_dir, name):
    """``case`` with the dense inverse, the banded probes, d0 (<= 1e-8 asserted) and the pose covariance in ``ref``."""
    c = case(golden_dir, name)
    if "Sa" not in c["ref"]:
        uref.solve(c["ref"])
    return c


def full_index(c, active_positions):
    return [int(c["prob"].ACT[p]) for p in active_positions]
