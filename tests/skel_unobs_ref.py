"""Reference for the observability rule of the skeleton-FTE posterior (acino_skel_fte_observability and the pin_unobserved
argument of acino_skel_fte_covariance_pinned / acino_skel_fte_sample_pinned): numpy on the CPU, on top of tests/skel_cov_ref.py.
Test infrastructure; nothing here comes from the code under test.

With H_F[n] = skel_cov_ref.fisher_blocks (the Fisher blocks, no prior) and SK_UNOBS_REL = 1e-24, per active state p of a clip:

    info[p]       = sum_n H_F[n][p][p]                         (frames in order)
    n_seen[p]     = #{ n : H_F[n][p][p] > SK_UNOBS_REL * max_q info[q] }
    unobserved[p] = info[p] <= SK_UNOBS_REL * max_q info[q]      (max info = 0: every state)

With pinning, an unobserved state joins the oracle's bound-active set in EVERY frame (skel_cov_ref.banded's rule: row and column 0,
diagonal 1, the prior's couplings dropped).  Pose slot l of frame n depends on an unobserved state if any entry of
G[n, l][:, p] is nonzero for an unobserved p (G = skel_cov_ref.pose_jacobian): std_pos = +inf, cov_pos = NaN; every other slot is
G cov_x G^T.  The bar is the project's: bar(d0) = max(64 d0, 1e-13), d0 the disagreement of the dense inverse and the banded
probes on the pinned matrix; d0 > 1e-8 is refused."""
import numpy as np

import skel_cov_ref as cref
from skel_cov_ref import bar, rel_err  # noqa: F401  (re-exported)

SK_UNOBS_REL = 1e-24
D0_REFUSED = 1e-8


def observability(HF):
    """(info [P], n_seen [P], unobserved [P] bool) of one clip from its Fisher blocks [N, P, P]."""
    d = np.einsum("npp->np", HF)
    info = np.zeros(d.shape[1])
    for row in d:                                            # frame order
        info = info + row
    thr = SK_UNOBS_REL * info.max()
    return info, (d > thr).sum(axis=0).astype(np.int32), info <= thr


def pins(prob, xa, unobserved):
    """[N, P] bool: the oracle's bound-active set, plus the unobserved states in every frame."""
    return cref.pin_set(prob, xa) | np.asarray(unobserved, dtype=bool)[None, :]


def dependent_slots(G, unobserved):
    """[N, n_pose] bool: a nonzero entry of G[n, l] in the column of an unobserved state."""
    un = np.nonzero(unobserved)[0]
    if un.size == 0:
        return np.zeros(G.shape[:2], dtype=bool)
    return (G[..., un] != 0).any(axis=(2, 3))


def reference(prob, xa, probe_frames=None, pin=True):
    """Everything a test needs on one input, once: the rule's three outputs, the pin set with them, the dense inverse (a) and the
    banded probes (b) of the pinned matrix, d0, and the pose covariance of (a) with +inf / NaN at the dependent slots.
    ``pin=False`` leaves the unobserved states out of the pin set (the matrix of the unpinned definition)."""
    xa = np.asarray(xa, dtype=np.float64)
    HF = cref.fisher_blocks(prob, xa)
    info, n_seen, un = observability(HF)
    fixed = pins(prob, xa, un if pin else np.zeros_like(un))
    ab = cref.banded(prob, HF, fixed)
    frames = np.arange(xa.shape[0]) if probe_frames is None else np.asarray(probe_frames)
    out = dict(info=info, n_seen=n_seen, unobserved=un, fixed=fixed, ab=ab, frames=frames, HF=HF)
    G = cref.pose_jacobian(prob, xa)
    out["G"], out["dependent"] = G, dependent_slots(G, un)
    return out


def solve(r):
    """Adds (a), (b), d0 and the pose covariance to ``reference``'s dict (kept apart: a singular input has no inverse)."""
    Sa = cref.dense_blocks(r["ab"], r["fixed"])
    Sb = cref.probe_blocks(r["ab"], r["fixed"], r["frames"])
    d0 = cref.rel_err(Sb, Sa[r["frames"]])
    assert d0 <= D0_REFUSED, f"the two references disagree by {d0:.2e} on this input: refused"
    cp, sp = cref.pose_cov(Sa, r["G"])
    dep = r["dependent"]
    cp = np.where(dep[:, :, None, None], np.nan, cp)
    sp = np.where(dep, np.inf, sp)
    r.update(Sa=Sa, Sb=Sb, d0=d0, cov_pos=cp, std_pos=sp)
    return r


def deleted_inverse_blocks(prob, HF, fixed_bound, unobserved):
    """The per-frame blocks of the inverse of the matrix (bound pins only) with the rows and columns of the unobserved states
    DELETED in every frame, scattered back to [N, P, P] with zeros there: what pinning them must equal."""
    N, P = fixed_bound.shape
    un = np.asarray(unobserved, dtype=bool)
    A = cref.dense(cref.banded(prob, HF, fixed_bound))
    keep = np.tile(~un, N)
    Ai = np.linalg.inv(A[np.ix_(keep, keep)])
    k = int((~un).sum())
    out = np.zeros((N, P, P))
    idx = np.nonzero(~un)[0]
    for n in range(N):
        out[n][np.ix_(idx, idx)] = Ai[n * k:(n + 1) * k, n * k:(n + 1) * k]
    fb = fixed_bound
    return np.where(fb[:, :, None] | fb[:, None, :], 0.0, out)
