#!/usr/bin/env python3
"""Every array link_scale_system and link_scale_system_pixels return on the inputs of the GPU tests, and the numbers of the two
outer fits, as one .npz - and the comparison of two such files, bit for bit.  For a change that must not move a bit of the
link-scale family: dump in a checkout of the parent, dump in this tree, compare.

    python scripts/link_scale_dump.py dump OUT.npz
    python scripts/link_scale_dump.py compare A.npz B.npz        (exit status 0: no key differs)

Only public calls, the case modules under tests/ and the inputs the two GPU test modules define (their models, groups and CASES)
are used, so the script runs unchanged in an older checkout.  link_scale_system: link_scale_ref.NAMES x both THETAS at the
device's own pose fit, with cov and with cov=None, with and without return_sens, and pt16 with m=None.  link_scale_system_pixels:
the CASES of tests/test_gpu_link_scale_px.py x both thetas at the device's own pixel pose fit, with and without return_sens.
fit_link_scales and fit_link_scales_pixels on the scaled-truth inputs of those tests: scales, cov_log_scales, std_scales,
observed and the numbers of the history.  A None is stored as an empty array."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
FIT_KEYS = ("scales", "cov_log_scales", "std_scales", "observed")
HISTORY_KEYS = ("cost", "max_dtheta", "lam", "n_used", "accepted")


def dump(path):
    import link_scale_px_ref as xref
    import link_scale_ref as lref
    import skel_pose_fit_px_ref as ppx
    import skel_pose_fit_ref as pref
    import test_gpu_link_scale as t3
    import test_gpu_link_scale_px as tpx
    from acinoset_amd import build
    out = {}

    def put(tag, d):
        for key, val in d.items():
            out[f"{tag}/{key}"] = np.zeros(0) if val is None else np.asarray(val)

    def put_fit(tag, res):
        put(tag, {k: res[k] for k in FIT_KEYS})
        put(tag + "/history", {k: [h[k] for h in res["history"]] for k in HISTORY_KEYS})
        out[tag + "/status"] = np.asarray(res["status"])

    for name in lref.NAMES:
        for which, th in t3.THETAS.items():
            grp, K = t3.groups(name)
            scales = np.exp(0.1 * th * np.cos(1.0 + 2.0 * np.arange(K)))
            inp, prob = pref.inputs(name), lref.problem(name, scales=scales)
            mdl = build.scale_links(t3.model(name), scales, grp)
            fit = build.pose_fit(mdl, inp["points"], inp["cov"], x0=prob.x0, return_cov=False, **pref.FIT)
            for cov_tag, cov in (("cov", inp["cov"]), ("iso", None)):
                for sens in (True, False):
                    put(f"points/{name}/{which}/{cov_tag}/sens{int(sens)}",
                        build.link_scale_system(mdl, inp["points"], cov, fit, grp, prior_sigma=pref.FIT["prior_sigma"], m=prob.x0,
                                                return_sens=sens))
            if name == "pt16":
                put(f"points/{name}/{which}/default_m",
                    build.link_scale_system(mdl, inp["points"], inp["cov"], fit, grp, prior_sigma=pref.FIT["prior_sigma"]))
    for name, groups in tpx.CASES:
        for which, th in tpx.THETAS.items():
            grp, K = xref.groups_for(name, groups)
            scales = np.exp(0.1 * th * np.cos(1.0 + 2.0 * np.arange(K)))
            prob = xref.problem(name, scales=scales, groups=groups)
            mdl = build.scale_links(ppx.model_of(name), scales, grp)
            fit = build.pose_fit_pixels(mdl, x0=prob.x0, return_cov=False, **ppx.OPTS)
            for sens in (True, False):
                put(f"pixels/{name}/{groups}/{which}/sens{int(sens)}",
                    build.link_scale_system_pixels(mdl, fit, grp, prior_sigma=ppx.OPTS["prior_sigma"], m=prob.x0, return_sens=sens))
    put_fit("fit/points/pt16", t3.fitted())
    put_fit("fit/pixels/pt16-two", tpx.fitted())
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
