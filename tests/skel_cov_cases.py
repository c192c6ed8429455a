"""Inputs shared by the skeleton-covariance tests (host and GPU).  Test infrastructure.

The shipped human skeleton has two active states that move NO pose at any x (the psi angles of "chin" and "hip2": every link
they rotate has its offset along the rotation's own axis), so the Fisher matrix of the definition is singular on every clip of
it - status 5, by the definition.  The parity inputs therefore use ``generic_skeleton``: the same skeleton with every rest
position moved by a fixed +-15 cm, which leaves no link offset on a coordinate axis; that every active state is then observed
is checked on the CPU by ``assert_observed``.  The iterate is the fixture's straight line with fixed pseudo-random joint angles
(the matrix is defined at any x), clipped to the limits."""
import copy
import json
import os

import numpy as np

from oracle import skel_fte as osf

import skel_cov_ref as ref

# Detection noise of 0.3 px instead of the reference's 3: with w = 1/3 the matrix has a condition number of 3e9 (prior stiffness
# 5e7 against 0.02 in the depth direction two cameras see worst) and the two CPU references themselves disagree by 2e-8 .. 1e-7,
# above the 1e-8 at which the project's bar refuses an input; at w = 1/0.3 they agree to ~1e-10 and the test can resolve errors.
R_MEAS_TEST = 0.3
SLICE_STARTS = (60, 300)          # the two 40-frame windows of human_dlc_slice.npz used by the host and GPU tests


def load(golden_dir):
    g = np.load(os.path.join(golden_dir, "skel_fte_model.npz"))
    return g, json.loads(str(g["skeleton_json"]))


def generic_skeleton(sk, extra=0):
    """Rest positions moved by fixed offsets of up to 15 cm.  ``extra`` > 0 appends that many marker-less chain parts below
    "ankle1" (each a parent of the next: 3 more active angles apiece) - the P > 48 case."""
    sk = copy.deepcopy(sk)
    rng = np.random.default_rng(11)
    for k in sk["positions"]:
        sk["positions"][k] = [float(v + d) for v, d in zip(sk["positions"][k], rng.uniform(-0.15, 0.15, 3))]
    prev = "ankle1"
    for k in range(extra):
        part = f"extra{k}"
        sk["positions"][part] = [float(v + d) for v, d in zip(sk["positions"][prev], rng.uniform(-0.2, 0.2, 3))]
        sk["dofs"][part] = [1, 1, 1]
        sk["markers"] = list(sk["markers"]) + [part]
        sk["links"] = list(sk["links"]) + [[prev, part]]
        prev = part
    return sk


# Connected sub-trees of the skeleton (root "chin" included) whose leaves all carry detections, by the padded size PT of their
# active states (3 + 3 per part that is a parent): the solve, covariance and sampler kernels are templates on PT = 16, 32, 48, 64,
# and the full skeleton (PT 48) and ``extra=5`` (PT 64) reach only two of them.
SUB_TREES = {16: ("chin", "forehead", "neck", "shoulder1", "shoulder2", "elbow1"),                          # 15 active states
             32: ("chin", "forehead", "neck", "shoulder1", "shoulder2", "elbow1", "elbow2", "wrist1", "wrist2")}     # 24


def sub_skeleton(sk, keep):
    """``sk`` cut down to the parts ``keep``.  A part whose only children are left out or carry no detection would keep angles
    that no pixel observes: ``keep`` must be a connected sub-tree that ends in detected parts (``assert_observed`` checks it)."""
    keep = set(keep)
    return dict(links=[list(l) for l in sk["links"] if l[0] in keep and l[1] in keep],
                dofs={k: list(v) for k, v in sk["dofs"].items() if k in keep},
                positions={k: list(v) for k, v in sk["positions"].items() if k in keep},
                markers=[m for m in sk["markers"] if m in keep])


def with_extra_detections(det, parts, extra):
    """The detection table with ``extra`` more body parts "extra0" .. (copies of the first columns: the Fisher matrix reads the
    weights, not the pixel values)."""
    return np.concatenate([det, det[:, :, :extra]], axis=2), list(parts) + [f"extra{k}" for k in range(extra)]


def tables(det, parts):
    return [(list(parts), det[:, c]) for c in range(det.shape[1])]


def make_model(g, sk, det, n, sf, camera_model="fisheye", scene=None, parts=None):
    from acinoset_amd import build
    scene = (g["K"], g["D"], g["R"], g["t"]) if scene is None else scene
    model, _ = build.build_model(sk, scene=scene, dlc_tables=tables(det, g["parts"] if parts is None else parts), n_frames=n, start_frame=sf, pairing="name",
                                 initial_line=False, camera_model=camera_model, r_meas=R_MEAS_TEST)
    return model


def iterate(g, model, seed=0):
    """[N, P_full]: the fixture's straight line for the root, fixed pseudo-random angles (0.3 rad spread, 0.02 rad frame to
    frame), inside the limits."""
    n, act = model.N, np.asarray(model.active)
    x0 = g["init_x"]
    x = np.zeros((n, model.P))
    x[:, :3] = x0[0, :3][None, :] + np.arange(n)[:, None] * (x0[1, :3] - x0[0, :3])[None, :]
    rng = np.random.default_rng(seed)
    x[:, act[3:]] = 0.3 * rng.standard_normal((1, len(act) - 3)) + 0.02 * rng.standard_normal((n, len(act) - 3))
    x[:, act] = np.clip(x[:, act], model.lo[:, act], model.hi[:, act])
    return x


def problem(sk, model, scene, camera_model="fisheye", lo=None, hi=None):
    if camera_model == "pinhole":
        import pinhole_skel_ref as pskel
        return pskel.PinholeSkelFTEProblem(sk, model.meas, model.weights, *scene, model.h, lo=model.lo if lo is None else lo,
                                           hi=model.hi if hi is None else hi)
    return osf.SkelFTEProblem(sk, model.meas, model.weights, *scene, model.h, lo=model.lo if lo is None else lo,
                              hi=model.hi if hi is None else hi)


def assert_observed(prob, xa):
    HF = ref.fisher_blocks(prob, xa)
    unseen = np.nonzero(np.einsum("npp->p", HF) == 0)[0]
    assert unseen.size == 0, f"active states observed in no frame: {unseen}"
