"""Inputs shared by the redescending-loss tests of the skeleton FTE (tests/test_gpu_skel_loss.py).  Test infrastructure.

``cov_case``: the covariance parity input.  A sub-tree of tests/skel_cov_cases.py (PT 16, 12 frames) or the full generic
skeleton (PT 48, 40 frames) at ``skel_cov_cases.iterate``; the detections are the iterate's OWN projection (the reference's
projection, CPU) plus Gaussian noise of 0.15 px, and 5 % of the weighted detections are moved by 9 .. 30 px in u and in v
(either sign); weights 1 / R_MEAS_TEST where the shipped detections are weighted.  At R_MEAS_TEST = 0.3 px an inlier's scaled
residual is ~0.5 (the quadratic core, h = 1) and an outlier's is 30 .. 100 (beyond c = 20, h = 0).  The L1 twin carries the
same detections with the outliers' weights set to 0.  Built once per process."""
import copy

import numpy as np

import skel_cov_cases as cases
import skel_loss_ref as lref
import skel_reproj_ref as rref
import skel_sample_cases as scases

_CACHE = {}


def with_loss(model, loss):
    m = copy.copy(model)
    m.loss = loss
    return m


def cov_case(golden_dir, pt=16, seed=3, camera_model="fisheye", n_frames=None, x_seed=0):
    """``n_frames``: fewer frames than the 12 of the sub-tree (the iterate's seed ``x_seed`` then decides whether the two CPU
    references still agree to skel_cov_ref.bar's 1e-8: the caller asserts it)."""
    key = ("cov", pt, camera_model, n_frames, x_seed)
    if key in _CACHE:
        return _CACHE[key]
    g, sk0, det = scases.fixture(golden_dir)
    sc = scases.scene(g, camera_model)
    if pt == 48:
        sk, n = cases.generic_skeleton(sk0), 40
    else:
        sk, n = cases.sub_skeleton(cases.generic_skeleton(sk0), cases.SUB_TREES[pt]), 12
    n = n if n_frames is None else n_frames
    base = cases.make_model(g, sk, det, n, cases.SLICE_STARTS[0], camera_model, sc)
    x = cases.iterate(g, base, seed=x_seed)
    rep = rref.reprojection(sk, x, base.meas, base.weights, sc, camera_model, gate_w=1.0)
    rng = np.random.default_rng(seed)
    weighted = (rep["flags"] & 1) != 0
    meas = rep["uv"] + 0.15 * rng.standard_normal(rep["uv"].shape)
    idx = np.argwhere(weighted)
    out_idx = idx[rng.choice(len(idx), size=max(1, int(round(0.05 * len(idx)))), replace=False)]
    is_out = np.zeros_like(weighted)
    for n_, c_, l_ in out_idx:
        meas[n_, c_, l_] += rng.uniform(9.0, 30.0, 2) * rng.choice([-1.0, 1.0], 2)      # (the loss judges u and v separately)
        is_out[n_, c_, l_] = True
    robust = with_loss(base, "redescending")
    robust.meas = np.where(np.isfinite(base.meas), meas, base.meas)         # (a missing detection stays missing)
    twin = with_loss(robust, "l1")
    twin.weights = np.where(is_out, 0.0, robust.weights)
    prob = lref.problem(sk, robust, sc, camera_model)
    prob_twin = cases.problem(sk, twin, sc, camera_model)
    xa = x[:, prob.ACT]
    cases.assert_observed(prob_twin, xa)
    _CACHE[key] = dict(sk=sk, scene=sc, model=robust, twin=twin, x=x, prob=prob, prob_twin=prob_twin, is_out=is_out, weighted=weighted,
                       ref=lref.cov_reference(prob, xa))
    return _CACHE[key]
