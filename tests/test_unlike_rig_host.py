"""CPU, oracle only: what makes tests/test_gpu_unlike_rig.py worth its name.

GUARDS.  For every case of unlike_rig.CASES the reference on the rig and the reference on a mutant of it - K and D rolled by
one camera; for the skew cases also the skew dropped - differ by at least 1 000 x the tolerance of the GPU comparison, in the
GPU comparison's own measure.  A kernel that read another camera's row, or ignored alpha, computes the mutant: it cannot pass.
VALIDITY of the inputs: pixels in the image, no flagged undistortion, the pinhole undistortion converged on the points used.
PACKING: the three places that lay the intrinsics out for the device put camera c's numbers in row c and nowhere else."""
import numpy as np
import pytest

import unlike_rig as ur
from acinoset_amd import calib, sba
from acinoset_amd import synth as gsynth
from oracle import camera as ocam
from oracle import fk as ofk
from oracle import synth as osynth

FX, FY, CX, CY = osynth.K_DUMMY[0, 0], osynth.K_DUMMY[1, 1], osynth.K_DUMMY[0, 2], osynth.K_DUMMY[1, 2]


# ------------------------------------------------------------------------------------------------------------- the rig
@pytest.mark.parametrize("model", ur.MODELS)
def test_rig_is_the_stated_one(model):
    K, D, R, t = ur.unlike_rig(9, model, skew=True)
    K0, _D0, R0, t0 = osynth.make_rig(9)
    assert np.array_equal(R, R0) and np.array_equal(t, t0)                         # the geometry of make_rig
    m = np.arange(9) % 6
    lap = 1 + 0.01 * (np.arange(9) // 6)
    assert np.allclose(K[:, 0, 0], FX * np.array([0.80, 0.88, 0.95, 1.05, 1.12, 1.20])[m] * lap, rtol=1e-15)
    assert np.allclose(K[:, 1, 1], FY * np.array([1.18, 0.83, 1.07, 0.92, 1.13, 0.86])[m] * lap, rtol=1e-15)
    assert np.array_equal(K[:, 0, 2], CX + np.array([-70, 45, -20, 60, -55, 30.0])[m])
    assert np.array_equal(K[:, 1, 2], CY + np.array([40, -35, 55, -15, 25, -50.0])[m])
    assert np.allclose(K[:, 0, 1], np.array([2e-3, -3e-3, 5e-3, -1e-3, 4e-3, -5e-3])[m] * K[:, 0, 0], rtol=1e-15)
    assert np.array_equal(K[:, 1, 0], np.zeros(9)) and np.array_equal(K[:, 2], np.tile([0.0, 0, 1], (9, 1)))
    if model == "fisheye":
        for c in range(9):
            want = osynth.D_DUMMY * [0.5, 0.7, 0.9, 1.1, 1.3, 1.5][c % 6] * np.array([1, 1 + 0.1 * (c % 6), 1 - 0.1 * (c % 6),
                                                                                    1 + 0.05 * (c % 6)])
            assert np.allclose(D[c], want, rtol=1e-15)
    else:
        base = ur.PINHOLE_D8 if model == "pinhole" else ur.pref.D12
        assert D.shape == (9, base.size) and ((D / base >= 0.8 - 1e-12) & (D / base <= 1.2 + 1e-12)).all()
    for a in range(9):                                                             # no camera is a copy of another
        for b in range(a):
            assert not np.array_equal(K[a], K[b]) and (not np.array_equal(D[a], D[b]) or a % 6 == b % 6)
    assert np.array_equal(ur.unlike_rig(9, model, skew=False)[0][:, 0, 1], np.zeros(9))
    for a, b in zip(ur.unlike_rig(9, model, skew=True, source=gsynth), (K, D, R, t)):     # either twin of make_rig
        assert np.array_equal(a, b)


def test_rolled_moves_the_intrinsics_alone():
    rig = ur.unlike_rig(6, "fisheye", skew=True)
    K, D, R, t = ur.rolled(rig)
    for c in range(6):
        assert np.array_equal(K[c], rig[0][c - 1]) and np.array_equal(D[c], rig[1][c - 1])
    assert R is rig[2] and t is rig[3]
    assert len(np.unique(ur.PINHOLE_MUL, axis=0)) == 6 and ur.PINHOLE_MUL.min() >= 0.8 and ur.PINHOLE_MUL.max() <= 1.2


# ------------------------------------------------------------------------------------------------------------- guards
@pytest.mark.parametrize("name,mutant", [(n, m) for n, c in ur.CASES.items() for m in c.mutants])
def test_guard(name, mutant):
    case = ur.CASES[name]
    want, other = ur.reference_of(name), ur.reference_of(name, mutant)
    for key in case.mutants[mutant]:
        kind, tol = case.tol[key]
        ratio = ur.error(other[key], want[key], kind) / tol
        print(f"guard [{name}] {mutant} {key}: {ratio:.2e} x the tolerance")
        assert ratio >= ur.GUARD, (name, mutant, key, ratio)


def test_every_case_has_its_mutants_and_its_gpu_test():
    import test_gpu_unlike_rig as gpu
    assert set(gpu.RUNNERS) | set(gpu.OWN_TEST) == set(ur.CASES) and not set(gpu.RUNNERS) & set(gpu.OWN_TEST)
    for name, test in gpu.OWN_TEST.items():
        assert callable(getattr(gpu, test)), (name, test)
    for name, case in ur.CASES.items():
        assert "rolled" in case.mutants and set(case.mutants["rolled"]) == set(case.tol), name
        skewed = bool(np.any(ur.inputs_of(name)["rig"][0][:, 0, 1]))
        # a skew case is guarded against a dropped skew too, unless both sides ignore the skew by design (the FTE NLP)
        assert ("no_skew" in case.mutants) == (skewed and name != "d_fte_fisheye_skew"), name
    assert {c.group for c in ur.CASES.values()} == {"a", "b", "c", "d", "e", "f", "g", "h_step", "h_points", "h_cov", "h_dense"}


def test_the_fte_references_ignore_the_skew():
    """The FTE NLP projection has no skew term: the oracle on the skewed K is the oracle on the same K without it, bit for bit
    (the GPU file holds the kernel to the same identity)."""
    a, b = ur.reference_of("d_fte_fisheye_skew"), ur.reference_of("d_fte_fisheye")
    assert np.any(ur.inputs_of("d_fte_fisheye_skew")["rig"][0][:, 0, 1])
    assert a["cost"] == b["cost"] and np.array_equal(a["grad"], b["grad"]) and np.array_equal(a["hess"], b["hess"])


# ------------------------------------------------------------------------------------------------------------- validity
def _inside(px):
    return (px[..., 0] >= 0) & (px[..., 0] < osynth.IMG_W) & (px[..., 1] >= 0) & (px[..., 1] < osynth.IMG_H)


@pytest.mark.parametrize("model,skew", [("fisheye", True), ("fisheye", False), ("pinhole", False), ("pinhole12", False)])
def test_sprint_pixels_are_finite_and_in_the_image(model, skew):
    """Every sprint the cases use (16, 20, 24, 30, 60 frames).  One exception, stated: on the 8-coefficient pinhole rig camera 4
    loses the far end of the 60-frame sprint past the right edge (4 of 7 200 pixels); the generator gives those detections the
    likelihood of an invalid one, as it does on any rig, and no kernel weighs them."""
    rig = ur.unlike_rig(6, model, skew=skew)
    for n in (16, 20, 24, 30, 60):
        pos = ofk.cheetah_fk(osynth.trajectory(n, "sprint"))
        px = ur.clean_pixels(pos, rig, "fisheye" if model == "fisheye" else "pinhole")
        assert np.isfinite(px).all()
        out = ~_inside(px)
        if (model, n) == ("pinhole", 60):
            assert 0 < out.sum() <= 4 and not out[[0, 1, 2, 3, 5]].any()
            det = ur.inputs_of("d_fte_pinhole8")["seq"]["det"]
            assert (det[:, 4][out[4], 2] <= 0.4).all()
        else:
            assert not out.any(), (model, n, int(out.sum()))
    seq = ur.inputs_of("d_fte_fisheye" if model == "fisheye" else "d_fte_pinhole8")["seq"]
    assert (seq["det"][..., 2] > 0.5).mean() > 0.8                                 # most detections above the threshold


def test_fisheye_inputs_are_undistorted_without_a_flag():
    inp = ur.inputs_of("a_undistort_fisheye_skew")
    K, D = inp["rig"][:2]
    assert len(inp["X"]) == 500
    for c in range(6):
        assert not (ocam.undistort_points_fisheye(inp["px"][c], K[c], D[c]) == -1000000.0).any()
    tri = ur.inputs_of("a_triangulate_fisheye_skew")
    for (kind, a, b), px in tri["px"].items():
        assert len(px[0]) > 400                                                    # (points in front of both cameras)
        for c, p in zip((a, b), px):
            assert np.isfinite(p).all() and not (ocam.undistort_points_fisheye(p, K[c], D[c]) == -1000000.0).any()
    und = ur.reference_of("c_pairs_fisheye_skew")
    assert np.isfinite(und["tri"]).any() and np.nanmax(np.abs(und["tri"])) < 50.0   # (a flagged point triangulates to ~1e6)


def test_pinhole_projection_points_cover_the_image():
    for name in ("b_project_pinhole8", "b_project_pinhole12"):
        inp = ur.inputs_of(name)
        for c in range(6):
            px = ocam.project_points(inp["X"][c], *ur.subset(inp["rig"], c))
            assert len(px) > 450 and np.abs(px).max() < 4000.0 and not _inside(px).all()      # in the image and around it


def test_pinhole_round_trip_on_the_points_used():
    """undistort(project(X)) returns the normalised point to 1e-9: OpenCV's five fixed-point steps have converged on the points
    the pinhole triangulations see (the narrow cloud of group b, the 16-frame sprint of group c)."""
    inp = ur.inputs_of("b_triangulate_pinhole8")
    rig = inp["rig"]
    clouds = [(pair, inp["X"][pair]) for pair in ur.PAIRS]
    clouds.append((tuple(range(6)), ofk.cheetah_fk(osynth.trajectory(ur.PINHOLE_PAIR_FRAMES, "sprint")).reshape(-1, 3)))
    for cams, X in clouds:
        assert len(X) > 50
        for c in cams:
            Y = ur.cam_xyz(X, rig, c)
            back = ocam.undistort_points(ocam.project_points(X, *ur.subset(rig, c)), rig[0][c], rig[1][c])
            assert np.abs(back - Y[:, :2] / Y[:, 2:]).max() < 1e-9, (cams, c)


def test_dense_refinement_size():
    """The 20-frame sprint of h_dense_fisheye carries test_dense_extrinsic_refinement_against_the_scipy_oracle's assertions on the
    oracle alone: every camera holds observations of kept points, twice as many equations as unknowns, and scipy (60
    evaluations, consistent mask) lowers the cost from the perturbed start - so "at or below scipy's end" asks something."""
    inp = ur.inputs_of("h_dense_fisheye")
    assert inp["det"].shape == (ur.DENSE_FRAMES, 6, 20, 3)
    assert np.bincount(inp["ci"], minlength=6).min() > 100 and np.bincount(inp["pi"]).min() >= 2
    assert 2 * len(inp["pi"]) > 2 * (3 * int(inp["keep"].sum()) + 36 - 7)
    c0 = float(ur.reference_of("h_dense_fisheye")["cost_initial"])
    assert ur.dense_scipy().cost < 0.95 * c0


# ------------------------------------------------------------------------------------------------------------- packing
@pytest.mark.parametrize("n_cams", [6, 9])
def test_fisheye_records_keep_every_camera_in_its_row(n_cams):
    K, D, R, t = ur.unlike_rig(n_cams, "fisheye", skew=True)
    rec = calib.fisheye_records(K, D, R, t)
    assert rec.shape == (n_cams, 24)
    for c in range(n_cams):
        want = np.concatenate([[K[c, 0, 0], K[c, 1, 1], K[c, 0, 2], K[c, 1, 2]], D[c], R[c].ravel(), t[c].ravel(),
                               [K[c, 0, 1] / K[c, 0, 0], 0, 0, 0]])
        assert np.array_equal(rec[c], want), c
    assert len(np.unique(rec[:, :8], axis=0)) == n_cams and len(np.unique(rec[:6, 20])) == 6


@pytest.mark.parametrize("model", ["pinhole", "pinhole12"])
def test_pinhole_records_keep_every_camera_in_its_row(model):
    K, D, R, t = ur.unlike_rig(9, model, skew=True)                                # (the record has no place for the skew)
    rec = calib.pinhole_records(K, D, R, t)
    assert rec.shape == (9, 32)
    for c in range(9):
        want = np.zeros(32)
        want[:4] = K[c, 0, 0], K[c, 1, 1], K[c, 0, 2], K[c, 1, 2]
        want[4:4 + D.shape[1]] = D[c]
        want[18:27], want[27:30] = R[c].ravel(), t[c].ravel()
        assert np.array_equal(rec[c], want), c
    assert np.array_equal(rec, calib.pinhole_records(ur.without_skew((K, D, R, t))[0], D, R, t))
    assert len(np.unique(rec[:, :4 + D.shape[1]], axis=0)) == 9


@pytest.mark.parametrize("model", ["fisheye", "pinhole", "pinhole12"])
def test_sba_camera_tables_keep_every_camera_in_its_row(model):
    K, D, R, t = ur.unlike_rig(9, model)
    intr, Rt = sba._camera_tables(K, D, R, t, "fisheye" if model == "fisheye" else "pinhole", so3=False)
    assert intr.shape == (9, 16) and Rt.shape == (9, 12)
    for c in range(9):
        want = np.zeros(16)
        want[:4] = K[c, 0, 0], K[c, 1, 1], K[c, 0, 2], K[c, 1, 2]
        want[4:4 + D.shape[1]] = D[c]
        assert np.array_equal(intr[c], want), c
        assert np.array_equal(Rt[c], np.concatenate([R[c].ravel(), t[c].ravel()])), c
    assert len(np.unique(intr, axis=0)) == 9


def test_sba_refuses_the_skewed_fisheye_rig():
    """The bundle adjustment carries no alpha: the skewed rig is refused, not solved as another model."""
    K, D, R, t = ur.unlike_rig(6, "fisheye", skew=True)
    with pytest.raises(NotImplementedError, match="skew"):
        sba._camera_tables(K, D, R, t, "fisheye", so3=False)


def test_cov_problem_takes_the_rig():
    import sba_cov_ref as sref
    rig = ur.unlike_rig(8, "pinhole")
    prob = sref.make_problem(8, 11, 3, "pinhole", rig=rig)
    assert np.array_equal(prob["K"], rig[0]) and np.array_equal(prob["D"], rig[1]) and prob["model"] == "pinhole"
    assert not np.array_equal(prob["R"][6], rig[2][6])                             # (the reused cameras are moved all the same)
    base = sref.make_problem(8, 11, 3)
    same = sref.make_problem(8, 11, 3, rig=tuple(a[np.arange(8) % 6] for a in gsynth.make_rig()))
    for k in ("K", "D", "R", "t", "X", "uv", "pi", "ci"):
        assert np.array_equal(base[k], same[k]), k
