"""The extras of the three FTE solve entries (return_cov, return_rate_cov, n_samples, return_reprojection, cov_cams) asked for
all at once, on the GPU: what FTEContext._posterior composes must be, bit for bit, what each extra gives when asked for alone,
per clip what one context gives through its public methods, and per sequence what fte_solve gives on the sequence alone.

Bit equality is the bar: the kernels are deterministic, and the neighbouring tests assert the same pairwise
(test_gpu_fte_cov_rates.py: test_superset_is_bit_identical_to_covariance, test_fte_solve_return_rate_cov; test_gpu_fte_reproj.py;
test_gpu_fte_calib.py: test_solve_entries_return_the_calibration_term).  Inputs: theirs - 60 frames of "sprint" on 6 cameras and
two clips of 45 frames with seeds 20210313 + i, max_iter=60, three samples.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BASE = {"positions", "x", "dx", "ddx", "start_frame"}
SAMPLE_KEYS = ("x_samples", "positions_samples")
SINGLES = (("return_cov",), ("return_rate_cov",), ("n_samples", "sample_seed"), ("return_reprojection",), ("cov_cams",))


@pytest.fixture(scope="module")
def mods(gpu_lib):
    from acinoset_amd import calib, fte, synth
    return fte, synth, calib


@pytest.fixture(scope="module")
def extras(mods):
    """The six keywords of the all-at-once call."""
    _fte, _synth, calib = mods
    return dict(return_cov=True, return_rate_cov=True, n_samples=3, sample_seed=7, return_reprojection=True,
                cov_cams=calib.extrinsic_cov(6, 0.05, 2e-3, fixed=(0,)))


@pytest.fixture(scope="module")
def clips(mods):
    _fte, synth, _calib = mods
    return [synth.make_sequence(45, "sprint", seed=20210313 + i) for i in range(2)]


def _rig(seq):
    return seq["K"], seq["D"], seq["R"], seq["t"]


def _solve(fte, seq, **kw):
    return fte.fte_solve(seq["det"][..., :2], seq["det"][..., 2], *_rig(seq), seq["Ts"], max_iter=60, **kw)


def _host(a):
    return a.cpu().numpy() if isinstance(a, torch.Tensor) else a


def _same(a, b):
    return np.array_equal(_host(a), _host(b), equal_nan=True)      # (NaN: uv on a singular plane, res of a missing detection)


def test_all_extras_at_once_equal_each_extra_alone(mods, extras):
    fte, synth, _calib = mods
    seq = synth.make_sequence(60, "sprint")
    full, info = _solve(fte, seq, **extras)
    union = set(BASE)
    for names in SINGLES:
        one, info1 = _solve(fte, seq, **{k: extras[k] for k in names})
        assert info1["iter"] == info["iter"], names
        assert set(one) > BASE and set(one) <= set(full), names
        for k in set(one) - {"start_frame"}:
            assert isinstance(full[k], np.ndarray) and _same(one[k], full[k]), f"{k} of {names} differs from the all-at-once call"
        union |= set(one)
    assert set(full) == union | {"std_positions_total"}
    assert len(full) == len(BASE) + 3 + 4 + 2 + 7 + 4 + 1
    assert set(fte._REPROJ_KEYS.values()) <= set(full)


def test_clips_equal_one_context_asked_through_its_public_methods(mods, extras, clips):
    fte, _synth, _calib = mods
    seq = clips[0]
    out = fte.fte_solve_clips([s["det"] for s in clips], *_rig(seq), seq["Ts"], max_iter=60, return_numpy=False, **extras)
    assert len(out) == 2
    x = torch.cat([res["x"] for res, _info in out], dim=0)
    ctx = fte.FTEContext(np.concatenate([s["det"] for s in clips]), *_rig(seq), seq["Ts"], clip_len=45)
    try:
        ctx.set_x(x)
        rates, cov = ctx.covariance_rates(with_cov=True)
        draws = ctx.sample(3, seed=7)
        report = ctx.reprojection(cov_pos=cov[1])
        cal = ctx.calibration_sensitivity(extras["cov_cams"])
    finally:
        ctx.close()
    want = dict(zip(("cov_x", "cov_positions", "std_positions"), cov))
    want.update(zip(("cov_dx", "cov_ddx", "cov_velocities", "std_velocities"), rates))
    want.update(x_samples=draws["x"], positions_samples=draws["positions"])
    want.update({name: report[k] for k, name in fte._REPROJ_KEYS.items()})
    want.update(sens_cams=cal["sens"], cov_x_calib=cal["cov_x_cal"], cov_positions_calib=cal["cov_pos_cal"],
                std_positions_calib=cal["std_pos_cal"], std_positions_total=torch.sqrt(cov[2] ** 2 + cal["std_pos_cal"] ** 2))
    for b, (res, _info) in enumerate(out):
        assert set(res) == BASE | set(want)
        sl = slice(45 * b, 45 * (b + 1))
        for k, w in want.items():
            axis = 1 if k in SAMPLE_KEYS else 0
            assert isinstance(res[k], torch.Tensor) and res[k].shape[axis] == 45, k
            assert res[k].shape[1 - axis] == w.shape[1 - axis], k
            assert _same(res[k], w[:, sl] if axis else w[sl]), f"clip {b}: {k} differs from the context's own call"


def test_batch_equals_fte_solve_on_each_sequence_alone(mods, extras, clips):
    fte, _synth, _calib = mods
    seq = clips[0]
    out = fte.fte_solve_batch([s["det"] for s in clips], *_rig(seq), seq["Ts"], max_iter=60, **extras)
    shapes = dict(cov_x=(45, 25, 25), cov_positions=(45, 20, 3, 3), std_positions=(45, 20), cov_dx=(45, 25, 25),
                  cov_ddx=(45, 25, 25), cov_velocities=(45, 20, 3, 3), std_velocities=(45, 20), x_samples=(3, 45, 25),
                  positions_samples=(3, 45, 20, 3), uv=(45, 6, 20, 2), cov_uv=(45, 6, 20, 2, 2), std_uv=(45, 6, 20),
                  residuals=(45, 6, 20, 2), weights=(45, 6, 20, 2), mahal2=(45, 6, 20), flags=(45, 6, 20),
                  sens_cams=(45, 25, 36), cov_x_calib=(45, 25, 25), cov_positions_calib=(45, 20, 3, 3),
                  std_positions_calib=(45, 20), std_positions_total=(45, 20))
    for b, (res, _info) in enumerate(out):
        alone, _info1 = _solve(fte, clips[b], **extras)
        assert set(res) == set(alone) == BASE | set(shapes)
        for k, shape in shapes.items():
            assert isinstance(res[k], np.ndarray) and res[k].shape == shape, k
        for k in set(res) - {"start_frame"}:
            assert _same(res[k], alone[k]), f"sequence {b}: {k} differs from fte_solve on the sequence alone"
