"""The host-side rules of build.solve_video / solve_model_parallel (no GPU needed): which window owns a frame and the gather
by owner against a brute-force per-frame reference written here, which window is retried from which neighbour, and the
retried window's initial point against arrays written out by hand."""
import numpy as np
import pytest

from acinoset_amd import build


def _ref_owner(starts, window, first_frame, total):
    """Per frame, the windows in order: the strictly deepest one that covers the frame."""
    owner = []
    for n in range(total):
        best, best_depth = -1, -1
        for w, st in enumerate(starts):
            r = n - (st - first_frame)
            if 0 <= r < window and min(r, window - 1 - r) > best_depth:
                best, best_depth = w, min(r, window - 1 - r)
        owner.append(best)
    return owner


@pytest.mark.parametrize("window", [4, 5, 8])
def test_owner_and_stitch_equal_the_per_frame_reference(window):
    """Every overlap, every length from one window to past three (the pulled-back last window) and two first frames; even and
    odd windows for the ties of depth.  The per-window arrays encode (window, row), so a wrong row shows; NaN (and -1 for the
    int key) would show a frame that no window filled."""
    n_cases = 0
    for overlap in range(window):
        for total in range(window, 3 * window + 2):
            for f0 in (0, 7):
                starts = build.video_windows(f0, f0 + total - 1, window, overlap)
                owner = build._window_owner(starts, window, f0, total)
                ref = _ref_owner(starts, window, f0, total)
                assert owner.shape == (total,) and owner.dtype.kind == "i"
                assert owner.tolist() == ref, (window, overlap, total, f0)
                rows = np.arange(window)
                per_window = [dict(a=100.0 * w + rows, b=100.0 * w + rows[:, None] + np.array([0.0, 0.25, 0.5])[None, :],
                                   c=(100 * w + rows).astype(np.int32)) for w in range(len(starts))]
                got = build._stitch(owner, starts, f0, per_window, ("a", "b"), fill=np.nan)
                got.update(build._stitch(owner, starts, f0, per_window, ("c",), fill=-1))
                assert sorted(got) == ["a", "b", "c"]
                for k in ("a", "b", "c"):
                    want = np.stack([per_window[ref[n]][k][n - (starts[ref[n]] - f0)] for n in range(total)])
                    assert got[k].dtype == per_window[0][k].dtype and got[k].shape == want.shape
                    assert np.array_equal(got[k], want), (k, window, overlap, total, f0)
                assert not np.isnan(got["a"]).any() and not np.isnan(got["b"]).any() and (got["c"] >= 0).all()
                n_cases += 1
    assert n_cases == window * (2 * window + 2) * 2


def test_owner_refuses_windows_that_leave_a_frame_out():
    with pytest.raises(AssertionError):
        build._window_owner([0, 6], 4, 0, 10)


@pytest.mark.parametrize("px, want", [
    ([3.0, 40.0, 5.0], [(1, 0)]),                       # a bad window between two good ones: the better donor
    ([5.0, 40.0, 3.0], [(1, 2)]),
    ([4.0, 40.0, 4.0], [(1, 0)]),                       # equal donors: the left one
    ([20.0, 40.0, 30.0], []),                           # the better neighbours are above warm_px themselves
    ([40.0, 3.0, 50.0], [(0, 1), (2, 1)]),              # the first and the last window
    ([40.0, 3.0], [(0, 1)]),
    ([3.0, 40.0], [(1, 0)]),
    ([40.0], []),
    ([float("nan"), 40.0, 3.0], [(1, 2)]),              # a NaN is no candidate and no donor
    ([3.0, float("nan"), 3.0], []),
    ([float("nan"), 40.0, float("nan")], []),
    ([3.0, 15.0, 3.0], []),                             # px == warm_px: not a candidate ...
    ([15.0, 40.0, 20.0], [(1, 0)]),                     # ... but a donor
])
def test_warm_pairs(px, want):
    assert build._warm_pairs(px, 15.0) == want


def _warm_case():
    window, act = 8, np.array([0, 1, 2, 4, 6])
    r, c = np.arange(window, dtype=np.float64)[:, None], np.arange(7, dtype=np.float64)[None, :]
    own, donor = r + c / 8, 20 + r + c / 8              # (eighths: every entry below is exact)
    lo, hi = np.full((window, 7), -100.0), np.full((window, 7), 100.0)
    lo[:, [3, 5]] = hi[:, [3, 5]] = 0.0                 # the inactive states' box is not applied
    hi[:, 4], lo[:, 6] = 25.0, 21.0
    return window, act, own, donor, lo, hi


def test_warm_x0_from_a_donor_five_frames_earlier():
    """Shared frames: the window's rows 0..2 = the donor's rows 5..7; the donor's row 7 is the nearest to the rest.  Its angle
    4 (27.5) is clipped to 25 in every row, its angle 6 (27.75) held; the inactive columns 3 and 5 are the donor's in the
    shared rows and the window's own below them."""
    window, act, own, donor, lo, hi = _warm_case()
    keep = own.copy()
    got = build._warm_x0(own, 105, donor, 100, window, act, lo, hi)
    want = np.array([[25.0, 25.125, 25.25, 25.375, 25.0, 25.625, 25.75],
                     [26.0, 26.125, 26.25, 26.375, 25.0, 26.625, 26.75],
                     [27.0, 27.125, 27.25, 27.375, 25.0, 27.625, 27.75],
                     [3.0, 3.125, 3.25, 3.375, 25.0, 3.625, 27.75],
                     [4.0, 4.125, 4.25, 4.375, 25.0, 4.625, 27.75],
                     [5.0, 5.125, 5.25, 5.375, 25.0, 5.625, 27.75],
                     [6.0, 6.125, 6.25, 6.375, 25.0, 6.625, 27.75],
                     [7.0, 7.125, 7.25, 7.375, 25.0, 7.625, 27.75]])
    assert np.array_equal(got, want)
    assert np.array_equal(own, keep) and got is not own


def test_warm_x0_from_a_donor_five_frames_later():
    """Shared frames: the window's rows 5..7 = the donor's rows 0..2; the donor's row 0 is the nearest to the rest.  Its angle
    4 (20.5) is held, its angle 6 (20.75) clipped to 21 wherever it is below."""
    window, act, own, donor, lo, hi = _warm_case()
    got = build._warm_x0(own, 100, donor, 105, window, act, lo, hi)
    want = np.array([[0.0, 0.125, 0.25, 0.375, 20.5, 0.625, 21.0],
                     [1.0, 1.125, 1.25, 1.375, 20.5, 1.625, 21.0],
                     [2.0, 2.125, 2.25, 2.375, 20.5, 2.625, 21.0],
                     [3.0, 3.125, 3.25, 3.375, 20.5, 3.625, 21.0],
                     [4.0, 4.125, 4.25, 4.375, 20.5, 4.625, 21.0],
                     [20.0, 20.125, 20.25, 20.375, 20.5, 20.625, 21.0],
                     [21.0, 21.125, 21.25, 21.375, 21.5, 21.625, 21.75],
                     [22.0, 22.125, 22.25, 22.375, 22.5, 22.625, 22.75]])
    assert np.array_equal(got, want)
