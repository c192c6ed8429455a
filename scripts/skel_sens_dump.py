#!/usr/bin/env python3
"""Every array model_calibration_sensitivity and model_link_sensitivity return on the inputs of the tests, as one .npz - and the
comparison of two such files, bit for bit.  For a change that must not move a bit of the two entries: dump in a checkout of the
parent, dump in this tree, compare.

    python scripts/skel_sens_dump.py dump OUT.npz
    python scripts/skel_sens_dump.py compare A.npz B.npz        (exit status 0: no key differs)

Only public calls and the case modules under tests/ are used, so the script runs unchanged in an older checkout.  The inputs:
pt16, pt16pin, pt32, slice12, slice40, slice40pin, p51 of tests/skel_sample_cases.py (PT 16 / 32 / 48 / 64, both camera models,
12 to 40 frames), each without a Sigma and with the tests' own (fte_calib_ref.random_psd, skel_links_ref.random_psd); shipped12
and lost12 of tests/skel_unobs_cases.py with pin_unobserved; slice12 with two link groups unknown; and a batch of three clips of
slice40 whose middle clip is singular.  A None is stored as an empty array."""
import copy
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
GOLDEN = os.path.join(ROOT, "tests", "golden")
NAMES = ("pt16", "pt16pin", "pt32", "slice12", "slice40", "slice40pin", "p51")
GROUPS = {"slice40": "global", "p51": np.arange(20) % 16}          # (the others: "links"; as tests/test_gpu_skel_links.py)


def dump(path):
    import fte_calib_ref as fref
    import skel_cov_cases as cases
    import skel_links_ref as lkref
    import skel_sample_cases as scases
    import skel_unobs_cases as ucases
    from acinoset_amd import build
    out = {}

    def put(tag, dicts):
        for i, d in enumerate(dicts):
            for key, val in d.items():
                out[f"{tag}/{i}/{key}"] = np.zeros(0) if val is None else np.asarray(val)

    def both(tag, models, xs, groups, **kw):
        n_cams = int(models[0].meas.shape[1])
        K = build.link_groups(models[0].prog, groups)[1]
        for name, sig_c, sig_l in (("plain", None, None), ("sigma", fref.random_psd(n_cams), lkref.random_psd(K))):
            put(f"{tag}/{name}/calib", build.model_calibration_sensitivity(models, xs, sig_c, **kw))
            put(f"{tag}/{name}/links", build.model_link_sensitivity(models, xs, groups, sig_l, **kw))

    for name in NAMES:
        c = scases.case(GOLDEN, name)
        both(name, [c["model"]], [c["x"]], GROUPS.get(name, "links"))
    for name in ("shipped12", "lost12"):
        c = ucases.case(GOLDEN, name)
        both(name + "/pin_unobserved", [c["model"]], [c["x"]], "links", pin_unobserved=True)
    c = scases.case(GOLDEN, "slice12")
    grp, K = build.link_groups(c["model"].prog, "links")
    obs = np.ones(K, dtype=bool)
    obs[[5, 9]] = False
    fit = dict(cov_log_scales=lkref.random_psd(K, hold=1, seed=4), observed=obs, groups=grp)
    put("slice12/unknown/links", build.model_link_sensitivity([c["model"]], [c["x"]], None, fit))
    c = scases.case(GOLDEN, "slice40")
    g, _sk0, det = scases.fixture(GOLDEN)
    models = [cases.make_model(g, c["sk"], det, 40, 60 + 45 * k) for k in range(3)]
    xs = [cases.iterate(g, m, seed=k) for k, m in enumerate(models)]
    names = list(models[1].names)
    bad = copy.copy(models[1])
    bad.weights = models[1].weights.copy()
    bad.weights[:, :, [names.index("elbow1"), names.index("wrist1")]] = 0.0
    models[1] = bad
    both("batch3", models, xs, "links")
    assert [int(out[f"batch3/sigma/{kind}/{i}/status"]) for kind in ("calib", "links") for i in range(3)] == [0, 5, 0] * 2
    np.savez(path, **out)
    print(f"{path}: {len(out)} arrays")


def compare(path_a, path_b):
    a, b = np.load(path_a), np.load(path_b)
    keys = sorted(set(a.files) | set(b.files))
    differ = [k for k in keys if k not in a.files or k not in b.files or a[k].dtype != b[k].dtype or
              not np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f")]
    for k in differ:
        print("DIFFERS  " + k + ("" if k in a.files and k in b.files else "  (in one file only)"))
    print(f"{len(keys)} keys, {len(differ)} differ")
    return 1 if differ else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
