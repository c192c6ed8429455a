"""Inputs shared by the rate-covariance tests of the skeleton FTE (host and GPU), built once per process on top of
tests/skel_cov_cases.py and tests/skel_sample_cases.py.  Test infrastructure.

  pt16n8 / pt32n8      the 15- and 24-state sub-trees (PT 16, PT 32) on 8 frames of human_dlc_slice.npz from frame 60
  slice40 / slice40pin the covariance tests' 40-frame window, fisheye and pinhole (PT 48)
  p51                  ``generic_skeleton(extra=5)`` (51 active states, PT 64) on 24 frames
  short1 .. short5     the PT 16 sub-tree on 1 .. 5 frames; the detections are the iterate's own poses projected with the oracle
                       camera, every slot seen by every camera at weight 1.  A clip shorter than the prior's stencil has no prior
                       at all and the detections alone must determine every state, so the three angles that move no pose
                       (``SHORT_OFF``) are switched off in the skeleton: 12 active states, still PT 16"""
import copy

import numpy as np

from oracle import camera
from oracle import skel_fte as osf

import skel_cov_cases as cases
import skel_cov_ref as cref
import skel_cov_rates_ref as rref
import skel_sample_cases as scases

PARITY = ("pt16n8", "pt32n8", "slice40", "slice40pin", "p51")
SHORT = (1, 2, 3, 4, 5)
# The seed of ``skel_cov_cases.iterate`` for the 8-frame inputs.  At seed 0 the two factorisations (c) and (c') of the PT 32
# input disagree by 2.3e-8 on cov_dx, above the 1e-8 at which the project's bar refuses an input (eight frames of prior hold
# the twist of a joint with one child only through the frame-to-frame change of its direction); at seed 3 they agree to 3e-9.
# Chosen on the references' own disagreement, on the CPU, before any GPU run.
ITERATE_SEED = {"pt16n8": 0, "pt32n8": 3}
# Every joint of the PT 16 sub-tree with one child ("chin", "forehead", "shoulder1") has a twist about the link to that child
# which moves no pose: the Fisher block of a frame has three zero eigenvalues whatever the cameras see, and a clip of fewer than
# four frames (no prior) is exactly singular.  One angle per such joint (part: axis) spans that null space; with these three off
# in ``dofs`` - the same states leave ``model.active`` and the oracle's - every N = 1 .. 5 is regular and (c) and (c') agree to
# 3e-11 or better (tests/test_skel_cov_rates_host.py checks both statements).
SHORT_OFF = {"shoulder1": 0, "chin": 2, "forehead": 2}
_CACHE = {}


def finish(sk, model, sc, cam, x=None, g=None):
    """dict(model, x, prob, sk, scene, cam, ref): ``ref`` is skel_cov_rates_ref.reference at x (oracle pin set)."""
    x = cases.iterate(g, model) if x is None else x
    prob = cases.problem(sk, model, sc, cam)
    xa = x[:, prob.ACT]
    fixed = cref.pin_set(prob, xa)
    ab = rref.banded(prob, cref.fisher_blocks(prob, xa), fixed)
    G = cref.pose_jacobian(prob, xa)
    return dict(model=model, x=x, prob=prob, sk=sk, scene=sc, cam=cam, ref=rref.reference(ab, fixed, G, model.h))


def short_skeleton(sk0, regular=True):
    """The PT 16 sub-tree; ``regular``: with the angles ``SHORT_OFF`` switched off.  (A marker's angles are all on by definition,
    so the three parts leave the marker list too; ``synthetic`` sets every slot's detections itself.)"""
    sk = cases.sub_skeleton(cases.generic_skeleton(sk0), cases.SUB_TREES[16])
    if regular:
        for part, axis in SHORT_OFF.items():
            sk["dofs"][part][axis] = 0
        sk["markers"] = [m for m in sk["markers"] if m not in SHORT_OFF]
    return sk


def synthetic(g, sk, n):
    """``sk`` on n frames with its own poses as detections (weight 1, every camera, every slot)."""
    sc = scases.scene(g)
    det = np.zeros((max(n, 1) + 60, len(sc[0]), len(g["parts"]), 3))
    model = cases.make_model(g, sk, det, n, 0, "fisheye", sc)
    x = cases.iterate(g, model)
    pos = osf.skeleton_fk_jac(sk, x)[0]                      # [n, L, 3]
    m = copy.copy(model)
    m.meas = np.stack([camera.pt3d_to_2d(pos, sc[0][c], sc[1][c], sc[2][c], sc[3][c]) for c in range(len(sc[0]))], axis=1)
    m.weights = np.ones(m.meas.shape[:3])
    assert m.meas.shape == model.meas.shape and np.isfinite(m.meas).all()
    return m, x


def case(golden_dir, name):
    if name in _CACHE:
        return _CACHE[name]
    g, sk0, det = scases.fixture(golden_dir)
    if name in ("slice40", "slice40pin"):
        c = scases.case(golden_dir, name)
        out = finish(c["sk"], c["model"], c["scene"], c["cam"], x=c["x"])
    elif name == "p51":
        sk = cases.generic_skeleton(sk0, extra=5)
        det5, parts5 = cases.with_extra_detections(det, g["parts"], 5)
        model = cases.make_model(g, sk, det5, 24, 60, parts=parts5)
        out = finish(sk, model, scases.scene(g), "fisheye", g=g)
    elif name in ("pt16n8", "pt32n8"):
        pt = int(name[2:4])
        sk = cases.sub_skeleton(cases.generic_skeleton(sk0), cases.SUB_TREES[pt])
        model = cases.make_model(g, sk, det, 8, cases.SLICE_STARTS[0], "fisheye", scases.scene(g))
        out = finish(sk, model, scases.scene(g), "fisheye", x=cases.iterate(g, model, seed=ITERATE_SEED[name]))
        assert (len(model.active) + 15) // 16 * 16 == pt
    elif name.startswith("short"):
        sk = short_skeleton(sk0)
        model, x = synthetic(g, sk, int(name[5:]))
        assert len(model.active) == 12
        out = finish(sk, model, scases.scene(g), "fisheye", x=x)
    else:
        raise KeyError(name)
    cases.assert_observed(out["prob"], out["x"][:, out["prob"].ACT])
    _CACHE[name] = out
    return out
