"""Full Trajectory Estimation: the drop-in for the reference's Pyomo model + ``opt.solve(m)``.

Reference: src/all_optimizations.py:22-566 (``fte``).  The reference builds a Pyomo NLP
(:283-500) and hands it to IPOPT (:503-522); here the same objective, in its equivalent reduced form
(DESIGN.md), is minimised by a projected Levenberg-Marquardt that runs entirely on the GPU:
residuals / analytic Jacobians / normal-equation assembly (fte_assemble.hip), the block-tridiagonal
Gauss-Newton solve by block cyclic reduction on the fp64 matrix cores (bcr.hip) and the accept /
reject controller (fte_api.hip).  ``fte_solve`` returns the reference's ``fte.pickle`` layout
(:548-559): ``{positions [N,20,3], x [N,25], dx [N,25], ddx [N,25], start_frame}``.
"""
import ctypes as C
import math
import os

import numpy as np
import torch

from . import _lib, calib
from ._lib import N_ACTIVE, N_MARKERS, N_STATES, FteParams, FteState, check, lib, ptr, stream_ptr

MARKERS = ["l_eye", "r_eye", "nose", "neck_base", "spine", "tail_base", "tail_mid", "tail_tip",
           "l_shoulder", "l_front_knee", "l_front_ankle", "r_shoulder", "r_front_knee", "r_front_ankle",
           "l_hip", "l_back_knee", "l_back_ankle", "r_hip", "r_back_knee", "r_back_ankle"]
PHI, THETA, PSI = 3, 17, 31          # state layout [x y z | phi_0..13 | theta_0..13 | psi_0..13]  (:182-185)
# the 25 states with Q != 0 (:245-252); convert_m (:530-556) drops the other 20 in this order
ACTIVE = np.array([0, 1, 2, PHI + 0, PHI + 1, PHI + 3] + [THETA + i for i in range(14)] +
                  [PSI + 0, PSI + 1, PSI + 3, PSI + 4, PSI + 5])
Q_SIGMA = np.array([4, 7, 5,
                    13, 32, 0, 10, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
                    9, 18, 43, 53, 90, 118, 247, 186, 194, 164, 295, 243, 334, 149,
                    26, 12, 0, 34, 43, 51, 0, 0, 0, 0, 0, 0, 0, 0], dtype=np.float64)
R_MEAS = 5.0                          # measurement std-dev, px (:243)
# acino_fte_params::precision: "f64" everywhere, or BASELINE config 5's "bf16 residuals with fp32 accumulate"
PRECISIONS = {"f64": 0, "bf16": 1, "bf16_residuals": 2}
REDESC = (3.0, 10.0, 20.0)            # redescending a, b, c (:25-27)
# the camera models live in calib (CAMERAS); these names stay for the callers that import them from here
CAMERA_MODELS = calib.CAMERA_MODELS
camera_model_of = calib.camera_model_of
camera_records = calib.camera_records


def bounds45():
    """Box bounds of :403-483 (1-based Pyomo indices -> 0-based)."""
    lo = np.full(N_STATES, -np.inf)
    hi = np.full(N_STATES, np.inf)
    for p in (4, 18, 5, 19, 33, 20, 21, 7, 35):
        lo[p - 1], hi[p - 1] = -np.pi / 6, np.pi / 6
    for p in (22, 36, 23, 37):
        lo[p - 1], hi[p - 1] = -np.pi / 1.5, np.pi / 1.5
    for p in (24, 26, 28, 30):
        lo[p - 1], hi[p - 1] = -np.pi / 2, np.pi / 2
    for p in (25, 27):
        lo[p - 1], hi[p - 1] = -np.pi, 0.0
    for p in (29, 31):
        lo[p - 1], hi[p - 1] = 0.0, np.pi
    return lo, hi


def make_params(n_frames, n_cams, Ts, dlc_thresh=0.5, r_meas=R_MEAS, Q=None, redesc=REDESC, lam0=1e-3,
                ftol=1e-10, xtol=1e-10, gtol=1e-8, n_global=None, n_offset=0, pin_left=False, pin_right=False,
                lam_max=1e16, clamp_lambda=False, shared_gpu=False, clip_len=0, precision="f64", bcr_levels=0,
                trunc_tol=1e-10, own_first=0, own_count=0, chunk_nodes=0, refine_sweeps=0):
    p = FteParams()
    p.n_frames, p.n_cams = int(n_frames), int(n_cams)
    p.n_global = int(n_frames if n_global is None else n_global)
    p.n_offset = int(n_offset)
    p.pin_left, p.pin_right = int(bool(pin_left)), int(bool(pin_right))
    p.dlc_thresh, p.inv_r_meas = float(dlc_thresh), 1.0 / float(r_meas)
    p.redesc_a, p.redesc_b, p.redesc_c = (float(v) for v in redesc)
    Qs = Q_SIGMA ** 2 if Q is None else np.asarray(Q, dtype=np.float64)
    if Qs.shape != (N_STATES,):
        raise ValueError("Q must have 45 entries")
    if set(np.nonzero(Qs)[0].tolist()) != set(ACTIVE.tolist()):
        raise ValueError("the cheetah kernels are specialised to the reference's 25 active states "
                         "(Q must be non-zero exactly where all_optimizations.py:245-252 is)")
    wq = (1.0 / Qs[ACTIVE]) / float(Ts) ** 4
    lo, hi = bounds45()
    for i in range(N_ACTIVE):
        p.q_w[i] = wq[i]
        p.lo[i] = lo[ACTIVE[i]]
        p.hi[i] = hi[ACTIVE[i]]
    p.lam0, p.ftol, p.xtol, p.gtol = float(lam0), float(ftol), float(xtol), float(gtol)
    p.lam_max, p.clamp_lambda = float(lam_max), int(bool(clamp_lambda))
    p.shared_gpu = int(bool(shared_gpu))
    p.clip_len = int(clip_len)
    if precision not in PRECISIONS:
        raise ValueError(f"precision must be one of {sorted(PRECISIONS)}")
    p.precision = PRECISIONS[precision]
    p.bcr_levels, p.trunc_tol = int(bcr_levels), float(trunc_tol)
    p.own_first, p.own_count = int(own_first), int(own_count)
    p.chunk_nodes, p.refine_sweeps = int(chunk_nodes), int(refine_sweeps)
    return p


def solver_plan(params):
    """Layout the library chooses for these parameters (acino_fte_plan): nodes per run of the chunked solver (0: block
    cyclic reduction over the whole chain), runs, separators, reduction levels of the reduced chain."""
    out = (C.c_int32 * 4)()
    check(lib().acino_fte_plan(C.byref(params), out))
    return dict(m=int(out[0]), n_chunks=int(out[1]), n_sep=int(out[2]), levels=int(out[3]))


def auto_bcr_levels(params, min_distance_frames=384):
    """Smallest K >= 1 after which the nodes that remain are >= min_distance_frames apart (3 * m * 2^K frames, m = nodes
    per run of the chunked solver, 1 without it), or 0 (complete reduction) when the chain has no level beyond it."""
    plan = solver_plan(params)
    K = 1
    while 3 * max(plan["m"], 1) * 2 ** K < min_distance_frames:
        K += 1
    return K if K <= plan["levels"] - 2 else 0      # (worth it from two saved levels on)


class FTEContext:
    """Owns the device buffers of one FTE problem (one shard of a sequence on one GPU)."""

    def __init__(self, det, k_arr, d_arr, r_arr, t_arr, Ts, camera_model=None, project_func=None, **kw):
        self.camera_model = camera_model_of(camera_model, project_func, kw.get("precision", "f64"))
        _lib.require_gpu()
        dev = torch.device("cuda", torch.cuda.current_device())
        self.device = dev
        self.det = calib._to_dev(det, dev)
        if self.det.dim() != 4 or self.det.shape[2] != N_MARKERS or self.det.shape[3] != 3:
            raise ValueError("det must be [N, C, 20, 3] = (x, y, likelihood)")
        self.N, self.C = int(self.det.shape[0]), int(self.det.shape[1])
        self.Ts = float(Ts)
        self.cams = torch.as_tensor(camera_records(self.camera_model, k_arr, d_arr, r_arr, t_arr), device=dev)
        if self.cams.shape[0] != self.C:
            raise ValueError("camera count mismatch between det and the rig")
        self._kw = self._resolve_defaults(dict(kw))
        self._kw0 = dict(self._kw)                # as asked for: an escalation (status 7 -> one more level) edits self._kw
        self._escalated = False
        self._graph = False
        self._create()

    # Linear-solver defaults of a single-GPU context (no pinned separators): chunked substructuring, the separator chain
    # reduced until the remaining nodes are >= TRUNC_DISTANCE frames apart, their dropped couplings re-introduced by
    # REFINE_SWEEPS block-Jacobi sweeps - verified on the device every iteration (state["trunc_eps"] <= trunc_tol, status 7
    # "truncation" otherwise, on which solve() continues with one more level).  bcr_levels = 0 asks for the complete
    # reduction, chunk_nodes = -1 for block cyclic reduction over the whole chain (the round-1/2 solver).
    # (a sweep costs ~2.5 us since the sweeps trade their vectors as tagged words, a reduction level ~27 us: one level less and
    #  four sweeps more than rounds 4-6 had - 160 frames, 3 sweeps.  scripts/levels_probe.py: at 10 000 frames of the benchmark
    #  sequence one level + 7 sweeps leave a verified bound <= 3.2e-16 in every iteration of the solve, 6 sweeps 3.5e-14; slow
    #  gaits, whose smoothness prior couples further, are refused at this distance and escalate, as they did at 160.)
    TRUNC_DISTANCE = 80
    REFINE_SWEEPS = 7
    TRUNC_TOL = 1e-12

    @classmethod
    def _resolve_defaults(cls, kw):
        """The linear-solver defaults, resolved ONCE and kept in the keyword set every rebuild of the context starts from
        (an escalation only replaces ``bcr_levels``: refinement sweeps, tolerance and precision travel with it)."""
        pinned = bool(kw.get("pin_left")) or bool(kw.get("pin_right"))
        if "bcr_levels" not in kw and not pinned:
            kw["bcr_levels"] = "auto"
            kw.setdefault("trunc_distance", cls.TRUNC_DISTANCE)
            kw.setdefault("refine_sweeps", cls.REFINE_SWEEPS)
            kw.setdefault("trunc_tol", cls.TRUNC_TOL)
        return kw

    def _create(self):
        kw = dict(self._kw)
        auto = kw.get("bcr_levels") == "auto"
        if auto:
            kw["bcr_levels"] = 0
        dist = kw.pop("trunc_distance", 384)
        self.params = make_params(self.N, self.C, self.Ts, **kw)
        if auto:
            self.params.bcr_levels = auto_bcr_levels(self.params, dist)
        if self.params.bcr_levels == 0:
            self.params.refine_sweeps = 0
        nbytes = lib().acino_fte_workspace_bytes(C.byref(self.params))
        self.workspace = torch.empty(nbytes + 256, dtype=torch.uint8, device=self.device)
        if os.environ.get("ACINO_POISON_WORKSPACE"):      # debug: every read-before-write of the workspace becomes a NaN
            self.workspace.view(torch.float64)[: (nbytes + 256) // 8].fill_(float("nan"))
        base = self.workspace.data_ptr()
        self._ws_ptr = (base + 255) // 256 * 256
        self._h = C.c_void_p()
        create = getattr(lib(), calib.CAMERAS[self.camera_model].fte_create)
        check(create(C.byref(self._h), C.byref(self.params), ptr(self.det), ptr(self.cams), C.c_void_p(self._ws_ptr), nbytes,
                     stream_ptr()))
        if self._graph:
            check(lib().acino_fte_enable_graph(self._h, 1))

    def _escalate(self, bound=None):
        """After status 7 (the truncated solve's verified error bound exceeded trunc_tol; the refused step was never
        applied): the same problem with more reduction levels (the complete reduction once the chain is exhausted),
        restarted from the current iterate.  ``bound``: the refused step's state["trunc_eps"], see _next_levels."""
        x = self.result()[0]
        levels = self._next_levels(bound)
        self.close()
        self._rebuild_with_levels(levels)
        check(lib().acino_fte_set_x(self._h, ptr(x), stream_ptr()))
        return levels

    def _next_levels(self, bound=None):
        """One level more - or, when the refused bound says how far off the truncation was, as many as it takes: the dropped
        couplings square with every level, so a bound b (~rho^(sweeps + 1)) becomes ~b^(2^j) after j more levels; the
        smallest j that brings it a decade under the tolerance.  (A bound of 1.0 means the sweeps did not contract by 1/2:
        no size to extrapolate from.)"""
        cur, jump = int(self.params.bcr_levels), 1
        tol = float(self.params.trunc_tol)
        if bound is not None and cur > 0 and 0.0 < bound < 1.0 and 0.0 < tol < 1.0:
            need = math.log(0.1 * tol) / math.log(bound)
            if need > 1.0:
                jump = max(1, int(math.ceil(math.log2(need) - 1e-9)))
        levels = cur + jump
        if cur == 0 or levels >= solver_plan(self.params)["levels"]:
            levels = 0
        return levels

    def _rebuild_with_levels(self, levels):
        """Same problem, same refinement settings / tolerance / precision, another number of reduction levels."""
        self._kw = dict(self._kw, bcr_levels=levels, refine_sweeps=int(self.params.refine_sweeps) or
                        int(self._kw.get("refine_sweeps", 0)), trunc_tol=float(self.params.trunc_tol))
        self._kw.pop("trunc_distance", None)
        self._escalated = True
        self._create()

    def reset_solver(self):
        """Back to the solver settings the context was created with, if an escalation changed them (contexts kept by
        ``reuse_context``: what a solve does must not depend on what earlier solves in the same context ran into)."""
        if self._escalated:
            self.close()
            self._kw = dict(self._kw0)
            self._escalated = False
            self._create()

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            lib().acino_fte_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # --- single-GPU driver -----------------------------------------------------------------------
    def set_x(self, x_active):
        x = calib._to_dev(x_active, self.device)
        if tuple(x.shape) != (self.N, N_ACTIVE):
            raise ValueError(f"x0 must be [{self.N}, 25] active states")
        self._x0 = x
        check(lib().acino_fte_set_x(self._h, ptr(x), stream_ptr()))

    def set_precision(self, precision):
        """Switch the assembly arithmetic (PRECISIONS) and re-evaluate the current iterate in it; the controller keeps
        its damping (after a lambda overflow: lam0) and goes back to "running" - used to polish a mixed-precision solve
        with fp64 iterations.  (The pinhole model is fp64 only.)"""
        camera_model_of(self.camera_model, None, precision)
        check(lib().acino_fte_set_precision(self._h, PRECISIONS[precision]))
        self._kw["precision"] = precision            # (a later rebuild - escalation - keeps the switched arithmetic)
        check(lib().acino_fte_reevaluate(self._h, stream_ptr()))

    def enable_graph(self, on=True):
        """Replay the LM step as a hipGraph (takes effect on a non-default stream)."""
        self._graph = bool(on)
        check(lib().acino_fte_enable_graph(self._h, int(bool(on))))

    def graphs_active(self):
        """Bit mask: bits 0..3 the four sharded phases, bit 4 the whole single-shard step."""
        return int(lib().acino_fte_graphs_active(self._h))

    def step(self):
        check(lib().acino_fte_step(self._h, stream_ptr()))

    def solve(self, max_iter):
        """Up to max_iter LM iterations IN TOTAL.  A step the truncated linear solve could not verify (status 7) is never
        applied: the context is rebuilt with more reduction levels (_next_levels) and the solve continues from the current iterate
        (the rebuilt controller starts from lam0 again); a refusal that uses up the last iteration is returned as status 7."""
        st = FteState()
        done = 0
        while True:
            check(lib().acino_fte_solve(self._h, max(int(max_iter) - done, 0), C.byref(st), stream_ptr()))
            info = st.as_dict()
            info["iter"] += done
            info["bcr_levels"] = int(self.params.bcr_levels)
            if info["status"] != 7 or info["iter"] >= int(max_iter):
                return info
            done = info["iter"]
            self._escalate(info.get("trunc_eps"))

    def state(self):
        st = FteState()
        check(lib().acino_fte_get_state(self._h, C.byref(st), stream_ptr()))
        return st.as_dict()

    def result(self):
        dev = self.device
        x = torch.empty((self.N, N_ACTIVE), dtype=torch.float64, device=dev)
        pos = torch.empty((self.N, N_MARKERS, 3), dtype=torch.float64, device=dev)
        dx = torch.empty_like(x)
        ddx = torch.empty_like(x)
        check(lib().acino_fte_get_result(self._h, self.Ts, ptr(x), ptr(pos), ptr(dx), ptr(ddx), stream_ptr()))
        return x, pos, dx, ddx

    PROF_CLASSES = ("elim", "elim_deep", "update0", "update", "update_deep", "backsub0", "backsub", "trial", "assemble",
                    "totals", "control", "backsub_tail", "trunc_check", "chunk_sweep", "sep_combine", "chunk_backsub", "refine")
    # (names as the profiler prints them, compared exactly; the assembly's: <JAC, PREC, SPLIT, PINHOLE>)
    PROF_KERNELS = dict(elim="k_bcr_elim", elim_deep="k_sep_level", update0="k_bcr_update0", update="k_bcr_update",
                        update_deep="k_bcr_update_deep", backsub0="k_bcr_backsub0", backsub="k_bcr_backsub",
                        backsub_tail="k_bcr_backsub_tail", trial="k_trial", assemble="k_fte_assemble<true, 0, 1, false>", totals="k_totals", control="k_control",
                        trunc_check="k_bcr_trunc_check", chunk_sweep="k_chunk_sweep", sep_combine="k_sep_combine",
                        chunk_backsub="k_chunk_backsub", refine="k_sep_tail")

    def profile_begin(self):
        check(lib().acino_fte_profile_begin(self._h))

    def profile_end(self):
        """Per kernel class: summed HIP-event time (ms), launches, work units (chain nodes / frames)."""
        n = len(self.PROF_CLASSES)
        ms = (C.c_double * n)()
        cnt = (C.c_int * n)()
        units = (C.c_int64 * n)()
        check(lib().acino_fte_profile_end(self._h, ms, cnt, units, stream_ptr()))
        return {k: dict(ms=ms[i], launches=cnt[i], units=units[i]) for i, k in enumerate(self.PROF_CLASSES)}

    def cost(self, x_active):
        x = calib._to_dev(x_active, self.device)
        out = torch.zeros(1, dtype=torch.float64, device=self.device)
        check(lib().acino_fte_cost(self._h, ptr(x), ptr(out), stream_ptr()))
        return float(out.item())

    def grad_hess(self):
        g = torch.empty((self.N, N_ACTIVE), dtype=torch.float64, device=self.device)
        h = torch.empty((self.N, N_ACTIVE, N_ACTIVE), dtype=torch.float64, device=self.device)
        check(lib().acino_fte_get_grad_hess(self._h, ptr(g), ptr(h), stream_ptr()))
        return g, h

    def _workspace(self, nbytes):
        """A fresh device buffer for one call: (the tensor that owns it, its first 256-byte aligned address)."""
        ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=self.device)
        return ws, C.c_void_p((ws.data_ptr() + 255) // 256 * 256)

    def covariance(self, std_only=False):
        """Laplace covariance of the CURRENT iterate (acino_fte_covariance): the inverse of the Gauss-Newton matrix
        blockdiag(H_n) + 2 q (x) D3^T D3 with the bound-active variables pinned, no Marquardt term.  Returns
        ``(cov_x [N,25,25], cov_pos [N,20,3,3], std_pos [N,20])`` as tensors on the context's device - rad^2 / m^2 and, for
        ``std_pos`` = sqrt(trace(cov_pos)), metres; ``std_only``: ``(None, None, std_pos)``.  The solver state is not
        touched.  Whole-sequence fp64 contexts only (RuntimeError otherwise)."""
        dev = self.device
        nbytes = lib().acino_fte_covariance_workspace_bytes(C.byref(self.params))
        ws, ws_ptr = self._workspace(nbytes)
        cov_x = None if std_only else torch.empty((self.N, N_ACTIVE, N_ACTIVE), dtype=torch.float64, device=dev)
        cov_pos = None if std_only else torch.empty((self.N, N_MARKERS, 3, 3), dtype=torch.float64, device=dev)
        std_pos = torch.empty((self.N, N_MARKERS), dtype=torch.float64, device=dev)
        check(lib().acino_fte_covariance(self._h, ws_ptr, nbytes, ptr(cov_x), ptr(cov_pos), ptr(std_pos),
                                         stream_ptr()))
        return cov_x, cov_pos, std_pos

    def covariance_rates(self, std_only=False, with_cov=False):
        """Laplace covariance of what ``result()`` returns as dx / ddx, and of the marker velocities
        (acino_fte_covariance_rates; same matrix, same sweeps as ``covariance``).  Returns ``(cov_dx [N,25,25],
        cov_ddx [N,25,25], cov_vel [N,20,3,3], std_vel [N,20])`` on the context's device - (rad/s)^2, (m/s)^2, (rad/s^2)^2,
        (m/s^2)^2; ``std_vel`` = sqrt(trace(cov_vel)) in m/s; ``std_only``: ``(None, None, None, std_vel)``.  dx_n, ddx_n
        come from the frames (n-2, n-1, n) of the frame's own clip, frames 0 and 1 of a clip from its first three frames
        by the start-up rules of ``result()``; the velocity of frame 0 repeats frame 1.  ``with_cov``: the three arrays
        of ``covariance()`` from the SAME call (one run of the sweeps), returned as a second tuple."""
        dev = self.device
        nbytes = lib().acino_fte_covariance_rates_workspace_bytes(C.byref(self.params))
        ws, ws_ptr = self._workspace(nbytes)

        def new(*shape, skip=False):
            return None if skip else torch.empty((self.N,) + shape, dtype=torch.float64, device=dev)

        cov_x = new(N_ACTIVE, N_ACTIVE, skip=std_only or not with_cov)
        cov_pos = new(N_MARKERS, 3, 3, skip=std_only or not with_cov)
        std_pos = new(N_MARKERS, skip=not with_cov)
        cov_dx = new(N_ACTIVE, N_ACTIVE, skip=std_only)
        cov_ddx = new(N_ACTIVE, N_ACTIVE, skip=std_only)
        cov_vel = new(N_MARKERS, 3, 3, skip=std_only)
        std_vel = new(N_MARKERS)
        check(lib().acino_fte_covariance_rates(self._h, self.Ts, ws_ptr, nbytes, ptr(cov_x), ptr(cov_pos),
                                               ptr(std_pos), ptr(cov_dx), ptr(cov_ddx), ptr(cov_vel), ptr(std_vel),
                                               stream_ptr()))
        rates = (cov_dx, cov_ddx, cov_vel, std_vel)
        return (rates, (cov_x, cov_pos, std_pos)) if with_cov else rates

    def sample(self, n_samples, seed=0, z=None, positions=True, rates=False, clip=False):
        """Joint draws of the whole trajectory from the Laplace posterior of the CURRENT iterate (acino_fte_sample):
        ``x[s] = x_hat + L^-T z[s]`` with ``A = L L^T`` the matrix ``covariance()`` inverts (unknowns frame-major, z of
        bound-active variables counted as 0), so ``Cov(x[s]) = A^-1`` - between frames as well, which is what a stride
        length, a mean speed or a phase between two feet needs.  Returns a dict of tensors on the context's device: ``x``
        [S,N,25]; with ``positions`` the FK of every sample, ``positions`` [S,N,20,3]; with ``rates`` also ``dx``, ``ddx``
        [S,N,25] (acino_fte_derivatives per sample and clip: the start-up rules of ``result()``).  ``z=None``:
        ``torch.randn`` from a ``torch.Generator`` on the context's device seeded with ``seed`` (same seed, same device:
        same samples); a given ``z`` [S,N,25] is used as is (the map is deterministic).  ``clip=True`` clamps ``x`` to the
        box of the solve before FK and rates; default off, the Laplace posterior as documented.  The solver state is not
        touched.  Whole-sequence fp64 contexts only (RuntimeError otherwise)."""
        S = int(n_samples)
        if S < 1:
            raise ValueError("n_samples must be >= 1")
        dev = self.device
        if z is None:
            gen = torch.Generator(device=dev)
            gen.manual_seed(int(seed))
            z = torch.randn((S, self.N, N_ACTIVE), dtype=torch.float64, device=dev, generator=gen)
        else:
            z = calib._to_dev(z, dev)
            if tuple(z.shape) != (S, self.N, N_ACTIVE) or z.dtype != torch.float64:
                raise ValueError(f"z must be float64 [{S}, {self.N}, 25]")
            z = z.contiguous()
        nbytes = lib().acino_fte_sample_workspace_bytes(C.byref(self.params))
        ws, ws_ptr = self._workspace(nbytes)
        x = torch.empty((S, self.N, N_ACTIVE), dtype=torch.float64, device=dev)
        fk_now = bool(positions) and not clip
        pos = torch.empty((S, self.N, N_MARKERS, 3), dtype=torch.float64, device=dev) if positions else None
        check(lib().acino_fte_sample(self._h, S, ptr(z), ws_ptr, nbytes, ptr(x), ptr(pos if fk_now else None),
                                     stream_ptr()))
        if clip:
            lo = torch.tensor(list(self.params.lo), dtype=torch.float64, device=dev)
            hi = torch.tensor(list(self.params.hi), dtype=torch.float64, device=dev)
            x = torch.minimum(torch.maximum(x, lo), hi).contiguous()
            if positions:
                check(lib().acino_fk_active(ptr(x), S * self.N, ptr(pos), stream_ptr()))
        out = dict(x=x)
        if positions:
            out["positions"] = pos
        if rates:
            L = int(self.params.clip_len) or self.N
            dx, ddx = torch.empty_like(x), torch.empty_like(x)
            xc, dxc, ddxc = (t.view(S * (self.N // L), L, N_ACTIVE) for t in (x, dx, ddx))
            for i in range(xc.shape[0]):
                check(lib().acino_fte_derivatives(ptr(xc[i]), L, self.Ts, ptr(dxc[i]), ptr(ddxc[i]), stream_ptr()))
            out.update(dx=dx, ddx=ddx)
        return out

    def calibration_sensitivity(self, cov_cams=None):
        """Sensitivity of the CURRENT iterate to the camera extrinsics (acino_fte_calibration_sensitivity) and the error
        bars a calibration covariance adds.  ``sens`` [N,25,6C] = S = -A^-1 G: the shift of the minimiser of the solver's own
        quadratic model (``A`` the matrix ``covariance()`` inverts, bound-active rows exactly 0) per unit change of
        c = [dw_0, dt_0, ..., dw_C-1, dt_C-1] with R_c <- exp([dw]x) R_c, t_c <- t_c + dt - the order and parametrisation of
        ``sba.covariance``.  It is not a derivative of the LM end point.  ``cov_cams``: an [6C, 6C] array or tensor, or the
        dict ``sba.covariance`` / ``return_cov=True`` returns (its ``"cov_cams"`` is used); a wrong shape, a non-finite entry
        or an asymmetric matrix is a ValueError before any launch.  Returns a dict of tensors on the context's device:
        ``sens``, ``cov_x_cal`` [N,25,25] = S_n cov_cams S_n^T, ``cov_pos_cal`` [N,20,3,3] = J_l cov_x_cal J_l^T and
        ``std_pos_cal`` [N,20] = sqrt(trace) in metres - the last three None without ``cov_cams``.  For a calibration that
        came from OTHER data the total is ``cov_x + cov_x_cal``; for extrinsics refined on the same clips
        (``refine_extrinsics_from_clips``) it is not valid.  The solver state is not touched.  Whole-sequence fp64 contexts
        only (RuntimeError otherwise)."""
        dev = self.device
        sigma = _cov_cams_matrix(cov_cams, self.C)
        if sigma is not None:
            sigma = torch.as_tensor(sigma, dtype=torch.float64, device=dev).contiguous()
        nbytes = lib().acino_fte_calibration_workspace_bytes(C.byref(self.params))
        ws, ws_ptr = self._workspace(nbytes)
        W = 6 * self.C

        def new(*shape):
            return None if sigma is None else torch.empty((self.N,) + shape, dtype=torch.float64, device=dev)

        sens = torch.empty((self.N, N_ACTIVE, W), dtype=torch.float64, device=dev)
        cov_x, cov_pos, std_pos = new(N_ACTIVE, N_ACTIVE), new(N_MARKERS, 3, 3), new(N_MARKERS)
        check(lib().acino_fte_calibration_sensitivity(self._h, ptr(sigma), ws_ptr, nbytes, ptr(sens), ptr(cov_x),
                                                      ptr(cov_pos), ptr(std_pos), stream_ptr()))
        return dict(sens=sens, cov_x_cal=cov_x, cov_pos_cal=cov_pos, std_pos_cal=std_pos)

    def reprojection(self, cov=True, cov_pos=None):
        """The CURRENT iterate in image space (acino_fte_reprojection), per (frame, camera, marker): a dict of tensors on
        the context's device - ``uv`` [N,C,20,2] the predicted pixel (NaN on a camera's singular plane), ``cov_uv``
        [N,C,20,2,2] its Laplace covariance J_pi cov_pos J_pi^T in px^2, ``std_uv`` [N,C,20] = sqrt(trace(cov_uv)) in px,
        ``res`` [N,C,20,2] = uv - detection (NaN where the detection is not finite), ``weight`` [N,C,20,2] the curvature
        weight in [0, 1] the solve gave each component (0: not weighted at all), ``mahal2`` [N,C,20] the squared gating
        distance res^T (cov_uv + R^2 I)^-1 res, ``flags`` [N,C,20] uint8 (bit 0 weighted by the solve, bit 1 behind the
        camera, bit 2 singular plane).  ``cov=True`` without ``cov_pos`` [N,20,3,3] runs ``covariance()`` first (and raises
        what that raises: whole-sequence fp64 contexts only); ``cov=False``: ``cov_uv`` and ``std_uv`` are None and
        ``mahal2`` is res^T res / R^2 - valid for every context.  One launch, nothing of the solver state is touched."""
        dev = self.device
        if cov and cov_pos is None:
            cov_pos = self.covariance()[1]
        if cov:
            cov_pos = calib._to_dev(cov_pos, dev)
            if tuple(cov_pos.shape) != (self.N, N_MARKERS, 3, 3) or cov_pos.dtype != torch.float64:
                raise ValueError(f"cov_pos must be float64 [{self.N}, 20, 3, 3]")
            cov_pos = cov_pos.contiguous()
        else:
            cov_pos = None
        shape = (self.N, self.C, N_MARKERS)
        uv = torch.empty(shape + (2,), dtype=torch.float64, device=dev)
        cov_uv = torch.empty(shape + (2, 2), dtype=torch.float64, device=dev) if cov else None
        res, weight = torch.empty_like(uv), torch.empty_like(uv)
        mahal2 = torch.empty(shape, dtype=torch.float64, device=dev)
        flags = torch.empty(shape, dtype=torch.uint8, device=dev)
        check(lib().acino_fte_reprojection(self._h, ptr(cov_pos), ptr(uv), ptr(cov_uv), ptr(res), ptr(weight), ptr(mahal2),
                                           ptr(flags), stream_ptr()))
        std_uv = torch.sqrt(cov_uv[..., 0, 0] + cov_uv[..., 1, 1]) if cov else None
        return dict(uv=uv, cov_uv=cov_uv, std_uv=std_uv, res=res, weight=weight, mahal2=mahal2, flags=flags)

    def _posterior(self, return_cov=False, return_rate_cov=False, n_samples=0, sample_seed=0, return_reprojection=False,
                   cov_cams=None):
        """The extras of the solve entries at the CURRENT iterate: a dict of device tensors under the names they have in
        ``results`` (_attach_posterior joins them), the frame axis first - second for ``x_samples`` / ``positions_samples``.
        The only place for two rules: covariance and rates come from ONE call when both are asked for, and the reprojection
        takes ``cov_positions`` from that call when it is there - the sweeps never run twice."""
        cov = rates = None
        if return_rate_cov:
            out = self.covariance_rates(with_cov=bool(return_cov))
            rates, cov = out if return_cov else (out, None)
        elif return_cov:
            cov = self.covariance()
        post = {}
        if cov is not None:
            post.update(zip(("cov_x", "cov_positions", "std_positions"), cov))
        if rates is not None:
            post.update(zip(("cov_dx", "cov_ddx", "cov_velocities", "std_velocities"), rates))
        if n_samples:
            draws = self.sample(n_samples, seed=sample_seed)
            post.update(x_samples=draws["x"], positions_samples=draws["positions"])
        if return_reprojection:
            report = self.reprojection(cov_pos=post.get("cov_positions"))
            post.update({name: report[k] for k, name in _REPROJ_KEYS.items()})
        if cov_cams is not None:
            cal = self.calibration_sensitivity(cov_cams)
            post.update(sens_cams=cal["sens"], cov_x_calib=cal["cov_x_cal"], cov_positions_calib=cal["cov_pos_cal"],
                        std_positions_calib=cal["std_pos_cal"])
            if cov is not None:
                post["std_positions_total"] = torch.sqrt(cov[2] ** 2 + cal["std_pos_cal"] ** 2)
        return post


_cov_cams_matrix = calib.cov_cams_matrix       # (the one validator of a calibration covariance, shared with build.py)


_REPROJ_KEYS = dict(uv="uv", cov_uv="cov_uv", std_uv="std_uv", res="residuals", weight="weights", mahal2="mahal2", flags="flags")


def _attach_posterior(res, post, conv, sl=slice(None)):
    """Frames ``sl`` of what FTEContext._posterior returned (None or empty: nothing) into one ``results``."""
    for name, a in (post or {}).items():
        res[name] = conv(a[:, sl] if name in ("x_samples", "positions_samples") else a[sl])


def detection_report(reproj, gate=None):
    """Summary of ``FTEContext.reprojection()`` (or of the ``uv`` ... ``flags`` entries of a solve's results) per (camera,
    marker), as a dict of numpy arrays [C, 20]: ``n_weighted`` the detections the solve weighted (bit 0 of the flags),
    ``n_inlier`` those of them whose smaller component weight is >= 0.5 ("used as inliers": the redescending loss kept at
    least half of their curvature), ``rms_inlier`` the RMS residual of those in px (NaN where there is none).  With
    ``gate`` - a chi-square quantile with 2 degrees of freedom the caller picks, e.g. 9.21 for 99 % - also the finite
    detections inside / outside ``mahal2 <= gate``, split by bit 0: ``n_weighted_inside``, ``n_weighted_outside``,
    ``n_unweighted_inside`` (low-likelihood detections that agree with the trajectory all the same) and
    ``n_unweighted_outside``.  Host arithmetic on the arrays given; no kernel."""
    def host(key):
        a = reproj[key] if key in reproj else reproj[_REPROJ_KEYS[key]]      # (a solve's results say residuals / weights)
        return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)

    res, weight, flags = host("res"), host("weight"), host("flags")
    weighted = (flags & 1) != 0
    inlier = weighted & (weight.min(axis=-1) >= 0.5)
    n_in = inlier.sum(axis=0)
    sq = np.where(inlier, (np.where(inlier[..., None], res, 0.0) ** 2).sum(axis=-1), 0.0).sum(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        rms = np.where(n_in > 0, np.sqrt(sq / np.maximum(n_in, 1)), np.nan)
    out = dict(n_weighted=weighted.sum(axis=0), n_inlier=n_in, rms_inlier=rms)
    if gate is not None:
        m2 = host("mahal2")
        finite = np.isfinite(m2)
        inside = finite & (np.where(finite, m2, np.inf) <= float(gate))
        outside = finite & ~inside
        out.update(n_weighted_inside=(inside & weighted).sum(axis=0), n_weighted_outside=(outside & weighted).sum(axis=0),
                   n_unweighted_inside=(inside & ~weighted).sum(axis=0),
                   n_unweighted_outside=(outside & ~weighted).sum(axis=0))
    return out


def cheetah_fk(q):
    """pose_to_3d of :170-186: q[N,45] full state -> positions[N,20,3]."""
    _lib.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    qd = calib._to_dev(q, dev).reshape(-1, N_STATES)
    pos = torch.empty((qd.shape[0], N_MARKERS, 3), dtype=torch.float64, device=dev)
    check(lib().acino_cheetah_fk(ptr(qd), qd.shape[0], ptr(pos), stream_ptr()))
    return calib._ret(pos, q)


def nose_line_init(det, k_arr, d_arr, r_arr, t_arr, dlc_thresh, n_frames=None, start_frame=0, det_first_frame=None,
                   camera_model="fisheye"):
    """Initial guess of :262-277,333-337: adjacent-pair triangulation of the detections above the
    likelihood threshold, least-squares line (linregress) through the nose (marker 2) over frames,
    psi_0 = atan2(y_slope, x_slope), every other state 0.  Returns x0[N,45] (numpy) for the frames
    start_frame .. start_frame + N - 1.

    The reference regresses over ALL triangulated frames of the video (:268-271) and evaluates the line on the window
    (:272-276, :334-337): pass the whole video's detections with ``det_first_frame=0`` and the window through
    ``start_frame`` / ``n_frames`` for exactly that.  By default (``det_first_frame=None``) ``det`` IS the window -
    its first row is frame ``start_frame`` - and the line is fitted to the window's own frames.
    ``camera_model``: "fisheye" or "pinhole", the model of the rig (calib.triangulate_pairs_dense)."""
    tri = calib.triangulate_pairs_dense(det, dlc_thresh, k_arr, d_arr, r_arr, t_arr, return_masks=False, model=camera_model)
    nose = tri[:, 2] if isinstance(tri, np.ndarray) else tri[:, 2].cpu().numpy()
    first = start_frame if det_first_frame is None else det_first_frame
    N = (nose.shape[0] if det_first_frame is None else nose.shape[0] - (start_frame - first)) if n_frames is None else n_frames
    ok = np.isfinite(nose).all(1)
    if ok.sum() < 2:
        raise ValueError("fewer than two triangulated nose points: cannot fit the initial line")
    return nose_line_from_points(np.arange(nose.shape[0], dtype=np.float64)[ok] + first, nose[ok], N, start_frame)


def nose_line_from_points(frames, nose_xyz, n_frames, start_frame=0):
    """The regression itself (:268-277, :333-337) on a table of triangulated nose points (frame, xyz)."""
    f = np.asarray(frames, dtype=np.float64)
    A = np.stack([f, np.ones_like(f)], 1)
    coef, *_ = np.linalg.lstsq(A, np.asarray(nose_xyz, dtype=np.float64), rcond=None)
    out_frames = np.arange(start_frame, start_frame + n_frames, dtype=np.float64)
    x0 = np.zeros((n_frames, N_STATES))
    x0[:, 0:3] = out_frames[:, None] * coef[0][None, :] + coef[1][None, :]
    x0[:, PSI + 0] = np.arctan2(coef[0][1], coef[0][0])
    return x0


def triangulation_init(det, k_arr, d_arr, r_arr, t_arr, dlc_thresh, camera_model="fisheye"):
    """Per-frame initial guess for LONG sequences (an extension: the reference's straight nose line
    cannot follow a trajectory that turns): head position from the triangulated head markers, heading
    from the neck_base->nose direction, gaps filled by linear interpolation; other states 0.
    ``camera_model`` as in nose_line_init."""
    tri = calib.triangulate_pairs_dense(det, dlc_thresh, k_arr, d_arr, r_arr, t_arr, return_masks=False, model=camera_model)
    tri = tri if isinstance(tri, np.ndarray) else tri.cpu().numpy()
    N = tri.shape[0]
    seen = np.isfinite(tri[:, 0:3]).all(-1)              # eyes + nose: mean of the ones that were triangulated
    cnt = seen.sum(1)
    head = np.where(seen[..., None], tri[:, 0:3], 0.0).sum(1) / np.maximum(cnt, 1)[:, None]
    head[cnt == 0] = np.nan                              # (no np.nanmean: frames without any head marker are expected, not a warning)
    fwd = tri[:, 2] - tri[:, 3]                          # neck_base -> nose
    idx = np.arange(N)
    x0 = np.zeros((N, N_STATES))
    for j in range(3):
        ok = np.isfinite(head[:, j])
        if ok.sum() == 0:
            raise ValueError("no triangulated head marker in the whole sequence")
        x0[:, j] = np.interp(idx, idx[ok], head[ok, j])
    ok = np.isfinite(fwd).all(1)
    if ok.sum() >= 1:
        psi = np.unwrap(np.arctan2(fwd[ok, 1], fwd[ok, 0]))
        x0[:, PSI + 0] = np.interp(idx, idx[ok], psi)
    return x0


def pose_fit(points, cov=None, x0=None, prior_sigma=np.pi, sigma_iso=0.01, min_markers=1, max_iter=100, ftol=1e-10,
             xtol=1e-10, lam0=1e-3, return_cov=True):
    """Per-frame pose of the cheetah model from 3-D marker points with a covariance each (include/acinoset_hip.h:
    acino_cheetah_pose_fit): per frame the minimiser over the 25 active states, inside the box of ``bounds45()[ACTIVE]``, of

        F(x) = 1/2 sum_{l enters} (FK_l(x) - y_l)^T W_l (FK_l(x) - y_l) + 1/2 sum_{p = 3..24} (x_p - m_p)^2 / prior_sigma^2

    by one projected Levenberg-Marquardt per frame (the controller of the FTE solve) in one launch.  ``points`` [N,20,3] in
    metres and ``cov`` [N,20,3,3] are the ``points`` / ``cov`` of ``calib.triangulate_multiview_dense``, whose dict is
    accepted in place of ``points``; a marker enters when its values are finite and its covariance positive definite
    (W = cov^-1), and with ``cov=None`` every finite point enters with W = I / sigma_iso^2.  ``x0`` [N,25] is the start and,
    clipped to the box, the centre m of the ridge on the 22 angles (``prior_sigma`` rad), which defines the states no
    entering marker moves; default: the head at the mean of the entering markers among eyes and nose (of all entering markers
    without them), psi_0 along neck_base -> nose, every other state 0.  Returns a dict:

      x [N,25], x_full [N,45], positions [N,20,3], cost [N]; n_markers, status, iters uint8 [N] (status 0 stopped on
      ``ftol`` / ``xtol``, 1 ``max_iter`` reached or lam overflowed, 2 fewer than ``min_markers`` enter, 3 numeric; every
      floating-point output of a frame is NaN for 2 and 3); pinned uint8 [N,25], the bound-active states at x; and with
      ``return_cov`` cov_x [N,25,25] = A_free^-1 (rows and columns of pinned states exactly 0), cov_positions [N,20,3,3] =
      J cov_x J^T and std_positions [N,20] in metres.

    numpy in, numpy out; CUDA tensors in, CUDA tensors out with no host copy."""
    return _pose_fit(lambda prm, dev, N, ins, outs: check(lib().acino_cheetah_pose_fit(prm, *ins, N, *outs, stream_ptr())),
                     points, cov, x0, None, N_MARKERS, ACTIVE, N_STATES,
                     ("points must be [N, 20, 3]", "cov must be [N, 20, 3, 3]", "x0 must be [N, 25] (the active states)"),
                     prior_sigma, sigma_iso, min_markers, max_iter, ftol, xtol, lam0, return_cov)


def _shape(a):
    return tuple(a.shape) if hasattr(a, "shape") else np.shape(a)


def _pose_fit(launch, points, cov, x0, N, n_slots, active, n_full, texts, prior_sigma, sigma_iso, min_markers, max_iter, ftol,
              xtol, lam0, return_cov):
    """What ``pose_fit`` and ``build.pose_fit`` share: the dict in place of ``points``, the checks of the shapes - points
    [N, n_slots, 3], cov [N, n_slots, 3, 3], x0 [N, len(active)], with ``texts`` the caller's three messages; N None: the
    frames of ``points`` - and of the parameters (``_fit_checks``), the staging, the outputs (``_fit_outputs``), ``PoseFitParams``,
    the scatter of x into x_full [N, n_full] at the columns ``active``, the dict, and numpy out for numpy in (``_fit_dict``: the
    three that ``pose_fit_pixels`` uses too).  ``launch(prm, dev, N, ins, outs)``
    makes the library call: ``ins`` the pointers of points, cov, x0 and ``outs`` those of the ten outputs, both in the order
    of the C entries."""
    if isinstance(points, dict):
        if cov is not None:
            raise ValueError("cov comes with the dict of triangulate_multiview_dense: pass one or the other")
        points, cov = points["points"], points["cov"]
    L, P = n_slots, len(active)
    shape = _shape(points)
    if N is None and len(shape) == 3:
        N = shape[0]
    if shape != (N, L, 3):
        raise ValueError(texts[0])
    if cov is not None and _shape(cov) != (N, L, 3, 3):
        raise ValueError(texts[1])
    if x0 is not None and _shape(x0) != (N, P):
        raise ValueError(texts[2])
    _fit_checks((("prior_sigma", prior_sigma), ("sigma_iso", sigma_iso), ("ftol", ftol), ("xtol", xtol), ("lam0", lam0)),
                max_iter, "min_markers", min_markers, L)
    dev = calib._dev()
    pts = calib._to_dev(points, dev)
    cv = None if cov is None else calib._to_dev(cov, dev)
    xs = None if x0 is None else calib._to_dev(x0, dev)
    o = _fit_outputs(N, P, L, dev, return_cov)
    nm = torch.empty((N,), dtype=torch.uint8, device=dev)
    prm = _lib.PoseFitParams(int(max_iter), int(min_markers), float(lam0), float(ftol), float(xtol), float(prior_sigma),
                             float(sigma_iso))
    launch(prm, dev, N, [ptr(t) for t in (pts, cv, xs)],
           [ptr(t) for t in (o["x"], o["cost"], nm, o["status"], o["iters"], o["pinned"], o["cov_x"], o["positions"],
                             o["cov_positions"], o["std_positions"])])
    return _fit_dict(o, "n_markers", nm, active, n_full, isinstance(points, torch.Tensor))


def _fit_checks(positive, max_iter, count_name, count, count_max):
    """The parameter checks of the per-frame fits: ``positive`` (name, value) pairs finite and > 0, max_iter one byte, the
    least count of measurements an integer in 1..count_max."""
    for name, val in positive:
        if not (np.isfinite(val) and val > 0):
            raise ValueError(f"{name} must be finite and > 0")
    if int(max_iter) != max_iter or not 1 <= max_iter <= 255:
        raise ValueError("max_iter must be an integer in 1..255")
    if int(count) != count or not 1 <= count <= count_max:
        raise ValueError(f"{count_name} must be an integer in 1..{count_max}")


def _fit_outputs(N, P, L, dev, return_cov):
    """The output tensors every per-frame fit has, under the names of the returned dict (None for the covariances not asked
    for)."""
    f64, u8 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.uint8, device=dev)
    o = dict(x=torch.empty((N, P), **f64), cost=torch.empty((N,), **f64), positions=torch.empty((N, L, 3), **f64))
    o.update((key, torch.empty(sh, **u8)) for key, sh in (("status", (N,)), ("iters", (N,)), ("pinned", (N, P))))
    o["cov_x"] = torch.empty((N, P, P), **f64) if return_cov else None
    o["cov_positions"] = torch.empty((N, L, 3, 3), **f64) if return_cov else None
    o["std_positions"] = torch.empty((N, L), **f64) if return_cov else None
    return o


def _fit_dict(o, count_key, count, active, n_full, tensors, **more):
    """The dict of a per-frame fit from its output tensors: x scattered into x_full [N, n_full] at the columns ``active``, the
    count under its key, ``more`` after the integer outputs, the covariances when they were asked for; numpy unless
    ``tensors``."""
    x = o["x"]
    x_full = torch.zeros((x.shape[0], n_full), dtype=torch.float64, device=x.device)
    x_full[:, torch.as_tensor(np.asarray(active, dtype=np.int64), device=x.device)] = x
    out = dict(x=x, x_full=x_full, positions=o["positions"], cost=o["cost"])
    out[count_key] = count
    out.update(status=o["status"], iters=o["iters"], pinned=o["pinned"], **more)
    if o["cov_x"] is not None:
        out.update(cov_x=o["cov_x"], cov_positions=o["cov_positions"], std_positions=o["std_positions"])
    if tensors:
        return out
    return {k: v.cpu().numpy() for k, v in out.items()}


def pose_fit_pixels(det, k_arr, d_arr, r_arr, t_arr, thresh=0.5, camera_model="fisheye", x0=None, f_scale=5.0, sigma_px=5.0,
                    prior_sigma=np.pi, min_detections=2, max_iter=100, ftol=1e-10, xtol=1e-10, lam0=1e-3, return_cov=True):
    """Per-frame pose of the cheetah model from the detections themselves (include/acinoset_hip.h:
    acino_cheetah_pose_fit_px): per frame the minimiser over the 25 active states, inside the box of ``bounds45()[ACTIVE]``, of

        F(x) = 1/sigma_px^2 sum_{(c,l) valid} sum_{k in (u,v)} 1/2 f^2 log1p(r_k^2 / f^2)
             + 1/2 sum_{p = 3..24} (x_p - m_p)^2 / prior_sigma^2,        r = pi_c(FK_l(x)) - det[n, c, l, :2],  f = f_scale

    - the reprojection error of the skeleton in every camera under the per-coordinate Cauchy loss of
    ``calib.triangulate_multiview_dense`` - by the projected Levenberg-Marquardt of ``pose_fit``, one launch.  ``det``
    [N,C,20,3] (x, y, likelihood); a detection is valid when its likelihood is above ``thresh`` and its pixel finite, so a
    marker one camera sees enters and a clip of one camera has a pose.  The rig and ``camera_model`` ("fisheye" or "pinhole")
    as in ``calib.triangulate_multiview_dense``.  ``x0`` [N,25] is the start and, clipped to the box, the centre m of the ridge;
    default: ``pose_fit`` of ``calib.triangulate_multiview_dense`` of the same detections (thresh, f_scale, sigma_px), the
    frames without a fit filled by ``fill_unfitted_frames`` (ValueError when no frame has one: give ``x0`` to a clip of one
    camera).  Returns the dict of ``pose_fit`` with n_detections uint16 [N] (the valid detections; status 2: fewer than
    ``min_detections``) in place of n_markers, plus weight [N,C,20,2]: the IRLS weight 1 / (1 + r^2 / f^2) every coordinate
    ended with, exactly 0 for an invalid detection.  cov_x = A_free^-1 with A = sum w J^T J / sigma_px^2 + the ridge: the
    matrix family of ``calib.triangulate_multiview_dense`` and ``sba.covariance``, carried to the states.

    numpy in, numpy out; CUDA tensors in, CUDA tensors out with no host copy when ``x0`` is given (the default start fills its
    unfitted frames on the host, N x 25 values, as ``pose_fit_init`` does)."""
    def start(d):
        tri = calib.triangulate_multiview_dense(d, thresh, k_arr, d_arr, r_arr, t_arr, model=camera_model, f_scale=f_scale,
                                                sigma_px=sigma_px)
        fit = pose_fit(tri, return_cov=False)
        return fill_unfitted_frames(fit["x"].cpu().numpy(), fit["status"].cpu().numpy() < 2)

    def launch(prm, dev, N, Cn, ins, outs):
        check(lib().acino_cheetah_pose_fit_px(prm, ins[0], N, Cn, *ins[1:], *outs, stream_ptr()))

    texts = dict(camera_model=f"camera_model must be one of {calib.CAMERA_MODELS}", det="det must be [N, C, 20, 3]",
                 cams="det holds {} cameras: 1..{} are supported", rig="camera count mismatch",
                 x0="x0 must be [N, 25] (the active states)")
    return _pose_fit_px(launch, det, x0, start, shape=(None, None, N_MARKERS), active=ACTIVE, n_full=N_STATES,
                        camera_model=camera_model, rig=(k_arr, d_arr, r_arr, t_arr), texts=texts,
                        tensors=isinstance(det, torch.Tensor), thresh=thresh, f_scale=f_scale, sigma_px=sigma_px,
                        prior_sigma=prior_sigma, min_detections=min_detections, max_iter=max_iter, ftol=ftol, xtol=xtol, lam0=lam0,
                        return_cov=return_cov)


def _pose_fit_px(launch, det, x0, start, *, shape, active, n_full, camera_model, rig, texts, tensors, thresh, f_scale, sigma_px,
                 prior_sigma, min_detections, max_iter, ftol, xtol, lam0, return_cov, ready=None):
    """What ``pose_fit_pixels`` and ``build.pose_fit_pixels`` share, the analogue of ``_pose_fit``: the checks, in this order -
    camera model; det [N, Cn, L, 3] with ``shape`` = (N, Cn, L), N and Cn None: those of ``det``; camera count; that of ``rig`` =
    (K, D, R, t) where ``texts`` has "rig"; x0 [N, len(active)]; ``_fit_checks``; ``thresh`` - with the caller's messages
    ``texts``, the camera records, ``ready(dev)`` (a refusal of the caller's once the device is known), the staging, the outputs,
    ``PoseFitPxParams``, the dict (numpy unless ``tensors``).  ``det`` / ``sigma_px`` may be callables, the caller's defaults,
    called after the shape checks; ``start(d)`` gives the default x0.  ``launch(prm, dev, N, Cn, ins, outs)`` makes the library
    call: ``ins`` the pointers of det, records, x0, ``outs`` those of the eleven outputs, in the order of the C entries."""
    if camera_model not in calib.CAMERAS:
        raise ValueError(texts["camera_model"])
    (N, Cn, L), P = shape, len(active)
    if not callable(det):
        got = _shape(det)
        if N is None and len(got) == 4:
            N, Cn = got[:2]
        if got != (N, Cn, L, 3):
            raise ValueError(texts["det"])
    if not 1 <= Cn <= _lib.MAX_CAMS:
        raise ValueError(texts["cams"].format(Cn, _lib.MAX_CAMS))
    if "rig" in texts and len(rig[0]) != Cn:
        raise ValueError(texts["rig"])
    if x0 is not None and _shape(x0) != (N, P):
        raise ValueError(texts["x0"])
    if callable(sigma_px):
        sigma_px = sigma_px()
    _fit_checks((("prior_sigma", prior_sigma), ("f_scale", f_scale), ("sigma_px", sigma_px), ("ftol", ftol), ("xtol", xtol),
                 ("lam0", lam0)), max_iter, "min_detections", min_detections, L * Cn)
    if np.isnan(thresh):
        raise ValueError("thresh must not be NaN")
    recs = calib.camera_records(camera_model, *rig)
    dev = calib._dev()
    if ready is not None:
        ready(dev)
    d = calib._to_dev(det() if callable(det) else det, dev)
    xs = calib._to_dev(start(d) if x0 is None else x0, dev)
    cams = torch.as_tensor(recs, device=dev)
    o = _fit_outputs(N, P, L, dev, return_cov)
    nd = torch.empty((N,), dtype=torch.uint16, device=dev)
    weight = torch.empty((N, Cn, L, 2), dtype=torch.float64, device=dev)
    prm = _lib.PoseFitPxParams(calib.CAMERAS[camera_model].code, int(max_iter), int(min_detections), 0, float(lam0), float(ftol),
                               float(xtol), float(prior_sigma), float(thresh), float(f_scale), float(sigma_px))
    launch(prm, dev, N, Cn, [ptr(t) for t in (d, cams, xs)],
           [ptr(t) for t in (o["x"], o["cost"], nd, o["status"], o["iters"], o["pinned"], o["cov_x"], o["positions"],
                             o["cov_positions"], o["std_positions"], weight)])
    return _fit_dict(o, "n_detections", nd, active, n_full, tensors, weight=weight)


PSI_COLUMNS = [int(np.nonzero(ACTIVE == PSI + k)[0][0]) for k in (0, 1, 3, 4, 5)]     # the psi states among the active ones


def fill_unfitted_frames(x, fitted, psi_columns=None):
    """The rule of ``pose_fit_init`` for the frames without a fit: x [N,25] with the rows where ``fitted`` is False filled by
    np.interp over the frames that have one (held flat at the ends), the five psi columns unwrapped over the fitted frames
    first.  ValueError when no frame has a fit.  ``psi_columns``: the columns to unwrap for another state layout
    (``build.pose_fit_start``: x [N, n_active] of a skeleton); default: the cheetah's PSI_COLUMNS."""
    psi_columns = PSI_COLUMNS if psi_columns is None else psi_columns
    x = np.array(x, dtype=np.float64, copy=True)
    fitted = np.asarray(fitted, dtype=bool)
    if not fitted.any():
        raise ValueError("no frame has a pose fit: no marker was triangulated in the whole sequence")
    idx = np.arange(len(x))
    for p in range(x.shape[1]):
        col = np.unwrap(x[fitted, p]) if p in psi_columns else x[fitted, p]
        x[:, p] = np.interp(idx, idx[fitted], col)
    return x


def pose_fit_init(det, k_arr, d_arr, r_arr, t_arr, dlc_thresh, camera_model="fisheye", **fit_kw):
    """Per-frame initial guess from a pose fit of every frame: ``calib.triangulate_multiview_dense`` of the detections, then
    ``pose_fit`` of its points with their covariances (``fit_kw`` goes to ``pose_fit``); the frames without a fit (status >= 2)
    are filled by ``fill_unfitted_frames``.  All 25 active states start near the markers, not only the head and psi_0 - the
    redescending loss of the FTE gives a detection further than c = 20 from its prediction neither gradient nor curvature.
    Returns x0[N,45] (numpy).  ``camera_model`` as in nose_line_init."""
    tri = calib.triangulate_multiview_dense(det, dlc_thresh, k_arr, d_arr, r_arr, t_arr, model=camera_model)
    fit = pose_fit(tri, return_cov=False, **fit_kw)
    host = (lambda a: a.cpu().numpy()) if isinstance(fit["x"], torch.Tensor) else (lambda a: a)
    xa = fill_unfitted_frames(host(fit["x"]), host(fit["status"]) < 2)
    x0 = np.zeros((xa.shape[0], N_STATES))
    x0[:, ACTIVE] = np.clip(xa, *(b[ACTIVE] for b in bounds45()))
    return x0


# Contexts kept alive between solves (fte_solve(..., reuse_context=True)): a second sequence of the same shape on the same rig
# finds its workspace, its uploaded constants and its captured hipGraph in place - what is left outside the LM loop is the
# copy of the detections, the initial evaluation and the outputs.  One context per key; clear_context_cache() frees them.
_CTX_CACHE = {}


def clear_context_cache():
    for ctx in _CTX_CACHE.values():
        ctx.close()
    _CTX_CACHE.clear()


def _context_for(det, k_arr, d_arr, r_arr, t_arr, Ts, reuse, kw, camera_model="fisheye"):
    if not reuse:
        return FTEContext(det, k_arr, d_arr, r_arr, t_arr, Ts, camera_model=camera_model, **kw), False
    import hashlib
    cams = camera_records(camera_model, k_arr, d_arr, r_arr, t_arr)
    key = (tuple(det.shape), str(det.device), float(Ts), camera_model, hashlib.sha256(cams.tobytes()).hexdigest(),
           tuple(sorted((k, repr(v)) for k, v in kw.items())))
    ctx = _CTX_CACHE.get(key)
    if ctx is None or not ctx._h.value:
        for old in list(_CTX_CACHE.values()):            # (one workspace at a time: a 10 000-frame context holds ~1 GB)
            old.close()
        _CTX_CACHE.clear()
        ctx = FTEContext(det.clone(), k_arr, d_arr, r_arr, t_arr, Ts, camera_model=camera_model, **kw)
        ctx.enable_graph(True)
        _CTX_CACHE[key] = ctx
    else:
        ctx.reset_solver()                                # (a no-op unless an earlier solve escalated the reduction levels)
        ctx.det.copy_(det)                                # (the library reads the detections through this tensor's pointer)
    return ctx, True


def triangulation_init_active(det, k_arr, d_arr, r_arr, t_arr, dlc_thresh, raise_now=True, camera_model="fisheye"):
    """``triangulation_init`` for a detections tensor that lives on the GPU: the same initial guess, formed on the device and
    returned as the 25 active states [N, 25].  Two launches (pairwise triangulation, ``acino_fte_triangulation_init``: head
    mean, unwrapped heading, interpolation over the frames that lack them) and no host round trip - the numpy form copied
    the 4.8 MB triangulation of a 10 000-frame sequence to the host (3 ms of a 15 ms solve), a torch form of the same
    arithmetic took ~60 small launches and three synchronisations (2 ms).  ``raise_now=False`` returns ``(xa, flag)`` with the
    "no head marker in the whole sequence" flag left on the device for the caller to test later.  ``camera_model`` as in
    nose_line_init."""
    tri = calib.triangulate_pairs_dense(det, dlc_thresh, k_arr, d_arr, r_arr, t_arr, return_masks=False, model=camera_model)
    n = int(tri.shape[0])
    xa = torch.empty((n, N_ACTIVE), dtype=torch.float64, device=tri.device)
    nbytes = int(lib().acino_fte_triangulation_init_scratch_bytes(n))
    scratch = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=tri.device)
    flag = torch.zeros(1, dtype=torch.int32, device=tri.device)
    psi_col = int(np.nonzero(ACTIVE == PSI + 0)[0][0])
    check(lib().acino_fte_triangulation_init(ptr(tri), n, int(tri.shape[1]), ptr(xa), N_ACTIVE, psi_col, ptr(scratch),
                                                scratch.numel() * 8, ptr(flag), stream_ptr()))
    if not raise_now:
        return xa, flag
    if int(flag.item()):
        raise ValueError("no triangulated head marker in the whole sequence")
    return xa


def _initial_x0(det, x0, init, rig, dlc_thresh, start_frame, camera_model, shape_error):
    """The initial state [N, 45] of one sequence (numpy): ``x0`` as given, or else the ``init`` guess from ``det`` with the
    rig's camera model; checked for its shape (``shape_error``) and for zeros in the states with Q == 0."""
    if x0 is None:
        if init == "nose_line":
            x0 = nose_line_init(det, *rig, dlc_thresh, start_frame=start_frame, camera_model=camera_model)
        elif init == "triangulation":
            x0 = triangulation_init(det, *rig, dlc_thresh, camera_model=camera_model)
        elif init == "pose_fit":
            x0 = pose_fit_init(det, *rig, dlc_thresh, camera_model=camera_model)
        else:
            raise ValueError("init must be 'nose_line', 'triangulation' or 'pose_fit'")
    x0 = np.asarray(x0.cpu().numpy() if isinstance(x0, torch.Tensor) else x0, dtype=np.float64)
    if x0.shape != (det.shape[0], N_STATES):
        raise ValueError(shape_error)
    if np.any(x0[:, np.setdiff1d(np.arange(N_STATES), ACTIVE)] != 0):
        raise ValueError("states with Q == 0 must start (and stay) at 0 (all_optimizations.py:543)")
    return x0


def fte_solve(meas, likelihood, k_arr, d_arr, r_arr, t_arr, Ts, x0=None, dlc_thresh=0.5, start_frame=0,
              max_iter=100, init="nose_line", return_numpy=True, reuse_context=False, camera_model=None, project_func=None,
              return_cov=False, return_rate_cov=False, n_samples=0, sample_seed=0, return_reprojection=False, cov_cams=None,
              **kw):
    """The FTE solve call.

    meas[N,C,20,2] pixel detections, likelihood[N,C,20], cameras as in the scene file (k_arr[C,3,3],
    d_arr[C,4(,1)], r_arr[C,3,3], t_arr[C,3(,1)]), Ts = 1/fps.  x0[N,45] optional initial state
    (default: the reference's nose-line initialisation).  Returns (results, info) where results has the
    reference's fte.pickle layout and info the solver status (iterations, final cost, |g|_inf, ...).
    ``reuse_context``: keep the context (workspace, constants, captured graph) for the next call with the same shapes, rig
    and options (see _CTX_CACHE above).  ``camera_model`` "fisheye" (default) or "pinhole" - then d_arr[C] holds OpenCV
    distortion vectors of 4, 5, 8 or 12 entries -, or the reference's ``project_func`` seam (camera_model_of); the initial
    guess and the solve both use that model.  ``return_cov``: results gain ``cov_x`` [N,25,25], ``cov_positions`` [N,20,3,3]
    and ``std_positions`` [N,20] (FTEContext.covariance at the returned x, from the context that produced it).
    ``return_rate_cov``: results gain ``cov_dx`` / ``cov_ddx`` [N,25,25], ``cov_velocities`` [N,20,3,3] and
    ``std_velocities`` [N,20] (FTEContext.covariance_rates: the error bars of dx, ddx and of the markers' velocities);
    with ``return_cov`` as well both sets come from one call.  ``n_samples`` > 0: results gain ``x_samples`` [S,N,25] and
    ``positions_samples`` [S,N,20,3], joint draws of the whole trajectory from the same posterior (FTEContext.sample with
    ``seed=sample_seed``; sample axis first).  ``return_reprojection``: results gain the solve in image space -
    ``uv`` [N,C,20,2], ``cov_uv`` [N,C,20,2,2], ``std_uv`` [N,C,20], ``residuals`` and ``weights`` [N,C,20,2], ``mahal2``
    and ``flags`` [N,C,20] (FTEContext.reprojection; ``detection_report`` summarises them); with ``return_cov`` as well the
    covariance sweeps run once.  ``cov_cams`` (an [6C,6C] covariance of the extrinsics, or the dict of ``sba.covariance``;
    ``calib.extrinsic_cov`` builds a diagonal one): results gain ``sens_cams`` [N,25,6C], ``cov_x_calib`` [N,25,25],
    ``cov_positions_calib`` [N,20,3,3] and ``std_positions_calib`` [N,20] (FTEContext.calibration_sensitivity: what the
    uncertainty of the calibration adds), and with ``return_cov`` as well ``std_positions_total`` =
    sqrt(std_positions^2 + std_positions_calib^2) - valid when the calibration came from other data than these clips."""
    _cov_cams_matrix(cov_cams, len(k_arr))       # (a malformed matrix fails before the solve, not after)
    extras = (return_cov, return_rate_cov, n_samples, sample_seed, return_reprojection, cov_cams)     # FTEContext._posterior
    model = camera_model_of(camera_model, project_func, kw.get("precision", "f64"))
    meas_t = meas if isinstance(meas, torch.Tensor) else torch.as_tensor(np.asarray(meas, dtype=np.float64))
    lik_t = likelihood if isinstance(likelihood, torch.Tensor) else torch.as_tensor(np.asarray(likelihood, dtype=np.float64))
    det = torch.cat([meas_t.to(torch.float64), lik_t.to(torch.float64).unsqueeze(-1).to(meas_t.device)], dim=-1)
    _lib.require_gpu()
    det = det.to(torch.device("cuda", torch.cuda.current_device()))
    init_flag = None
    if x0 is None and init == "triangulation":
        xa0, init_flag = triangulation_init_active(det, k_arr, d_arr, r_arr, t_arr, dlc_thresh, raise_now=False,
                                                   camera_model=model)   # (stays on the device)
    else:
        xa0 = _initial_x0(det, x0, init, (k_arr, d_arr, r_arr, t_arr), dlc_thresh, start_frame, model,
                          "x0 must be [N, 45]")[:, ACTIVE]
    ctx, cached = _context_for(det, k_arr, d_arr, r_arr, t_arr, Ts, reuse_context, dict(kw, dlc_thresh=dlc_thresh), model)
    kw.pop("trunc_distance", None)
    try:
        ctx.set_x(xa0)
        info = ctx.solve(max_iter)
        x, pos, dx, ddx = ctx.result()
        post = ctx._posterior(*extras) if info["status"] != 5 else None
    except Exception:
        # (the initial guess's flag is read after the solve - no synchronisation in front of it -, but whatever a solve from an
        #  all-zero start ran into must not hide the real cause)
        if init_flag is not None and int(init_flag.item()):
            raise ValueError("no triangulated head marker in the whole sequence") from None
        raise
    finally:
        if not cached:
            ctx.close()
    if init_flag is not None and int(init_flag.item()):
        raise ValueError("no triangulated head marker in the whole sequence")
    if info["status"] == 5:
        raise RuntimeError("FTE: block factorisation hit a non-positive pivot")
    conv = (lambda a: a.cpu().numpy()) if return_numpy else (lambda a: a)
    results = dict(positions=conv(pos), x=conv(x), dx=conv(dx), ddx=conv(ddx), start_frame=start_frame)
    _attach_posterior(results, post, conv)
    return results, info


def _derivatives(x_clip, Ts):
    dx, ddx = torch.empty_like(x_clip), torch.empty_like(x_clip)
    check(lib().acino_fte_derivatives(ptr(x_clip), x_clip.shape[0], float(Ts), ptr(dx), ptr(ddx), stream_ptr()))
    return dx, ddx


def fte_solve_clips(dets, k_arr, d_arr, r_arr, t_arr, Ts, x0s=None, dlc_thresh=0.5, start_frames=None, max_iter=100,
                    init="nose_line", return_numpy=True, camera_model=None, project_func=None, return_cov=False,
                    return_rate_cov=False, n_samples=0, sample_seed=0, return_reprojection=False, cov_cams=None, **kw):
    """Equal-length clips of one rig solved as ONE problem (BASELINE config 5's batched FTE at full width): the clips
    are laid end to end on the frame axis, the smoothness prior is cut at the clip boundaries (``clip_len``), and the
    block-cyclic reduction runs over the whole chain - every launch is as wide as all clips together, so the narrow
    levels that dominate a single short clip almost vanish.  One Levenberg-Marquardt controller acts on the SUM of the
    clips' costs (the problem is block diagonal: each clip converges to its own optimum, but damping and accept/reject
    are shared, so iterates differ from per-clip solves until convergence).  Returns a list of (results, info).
    ``camera_model`` / ``project_func`` / ``return_cov`` / ``return_rate_cov`` as in fte_solve (the covariance per clip: the
    clips are independent, so it is the one a solve of the clip alone would give at the same x).  ``n_samples`` / ``sample_seed``
    as in fte_solve: every clip gets its slice of the frame axis of one call's samples.  ``return_reprojection`` as in
    fte_solve, sliced per clip in the same way.  ``cov_cams`` as in fte_solve (one call; the calibration term of a clip does
    not depend on the other clips)."""
    _cov_cams_matrix(cov_cams, len(k_arr))
    extras = (return_cov, return_rate_cov, n_samples, sample_seed, return_reprojection, cov_cams)     # FTEContext._posterior
    model = camera_model_of(camera_model, project_func, kw.get("precision", "f64"))
    B = len(dets)
    if B == 0:
        return []
    dets_t = [d if isinstance(d, torch.Tensor) else torch.as_tensor(np.asarray(d, dtype=np.float64)) for d in dets]
    S = int(dets_t[0].shape[0])
    if any(int(d.shape[0]) != S for d in dets_t):
        raise ValueError("fte_solve_clips needs clips of equal length (use fte_solve_batch otherwise)")
    start_frames = list(start_frames) if start_frames is not None else [0] * B
    x0_all = np.zeros((B * S, N_STATES))
    for b, det in enumerate(dets_t):
        x0_all[b * S:(b + 1) * S] = _initial_x0(det, None if x0s is None else x0s[b], init, (k_arr, d_arr, r_arr, t_arr),
                                                dlc_thresh, start_frames[b], model, f"x0 of clip {b} must be [{S}, 45]")
    dev = torch.device("cuda", torch.cuda.current_device())
    det_all = torch.cat([d.to(device=dev, dtype=torch.float64) for d in dets_t], dim=0)
    polish = kw.pop("polish_f64", False)
    ctx = FTEContext(det_all, k_arr, d_arr, r_arr, t_arr, Ts, dlc_thresh=dlc_thresh, clip_len=S, camera_model=model, **kw)
    try:
        ctx.set_x(x0_all[:, ACTIVE])
        info = ctx.solve(max_iter)
        if polish and kw.get("precision", "f64") != "f64" and info["status"] in (0, 1, 2, 3, 4):
            # mixed-precision solve finished - by a stopping test or because no damping gives descent any more against
            # the fp64-summed cost (lambda overflow: the natural end of an inexact gradient) - : a few fp64 iterations
            # from its end point (same controller; damping kept, or back to lam0 after an overflow)
            n_mixed = info["iter"]
            ctx.set_precision("f64")
            info = ctx.solve(max(max_iter - n_mixed, 5))      # (a mixed solve that ran out of iterations is polished too)
            info["iter_mixed"] = n_mixed
        x, pos, _dx, _ddx = ctx.result()
        if info["status"] == 5:
            raise RuntimeError("FTE: block factorisation hit a non-positive pivot")
        post = ctx._posterior(*extras)
        conv = (lambda a: a.cpu().numpy()) if return_numpy else (lambda a: a)
        out = []
        for b in range(B):
            xb = x[b * S:(b + 1) * S].contiguous()
            dxb, ddxb = _derivatives(xb, Ts)                     # per clip: no differences across a clip boundary
            res = dict(positions=conv(pos[b * S:(b + 1) * S]), x=conv(xb), dx=conv(dxb), ddx=conv(ddxb),
                       start_frame=start_frames[b])
            _attach_posterior(res, post, conv, slice(b * S, (b + 1) * S))
            out.append((res, dict(info, clips=B, cost_is_sum_over_clips=True)))
        return out
    finally:
        ctx.close()


def fte_solve_batch(dets, k_arr, d_arr, r_arr, t_arr, Ts, x0s=None, dlc_thresh=0.5, start_frames=None, max_iter=100,
                    init="nose_line", n_streams=8, peek_every=8, return_numpy=True, camera_model=None, project_func=None,
                    return_cov=False, return_rate_cov=False, n_samples=0, sample_seed=0, return_reprojection=False,
                    cov_cams=None, **kw):
    """Several independent sequences (BASELINE config 5's "batched FTE": one rig, many clips) solved concurrently
    on ONE GPU.  Every sequence gets its own context and runs on one of ``n_streams`` HIP streams; a Levenberg-
    Marquardt step never synchronises with the host (the accept/reject controller is a device kernel and the step is
    one hipGraph launch), so the streams interleave and the narrow levels of one sequence's block-cyclic reduction
    overlap with the wide levels of another's (HIP multiplexes the streams onto 4 hardware queues by default; 8 streams
    keep all of them busy whatever the stream-to-queue assignment).  ``dets``: list of det[N_b, C, 20, 3] (lengths may differ).
    Returns a list of (results, info) exactly as ``fte_solve`` would for each sequence alone.  The reference solves
    clips one after another (src/all_optimizations.py:22, one ``fte()`` call per data directory).  ``camera_model`` /
    ``project_func`` / ``return_cov`` / ``return_rate_cov`` / ``n_samples`` / ``sample_seed`` / ``return_reprojection`` / ``cov_cams`` as in fte_solve."""
    _cov_cams_matrix(cov_cams, len(k_arr))
    extras = (return_cov, return_rate_cov, n_samples, sample_seed, return_reprojection, cov_cams)     # FTEContext._posterior
    model = camera_model_of(camera_model, project_func, kw.get("precision", "f64"))
    _lib.require_gpu()
    B = len(dets)
    if B == 0:
        return []
    start_frames = list(start_frames) if start_frames is not None else [0] * B
    streams = [torch.cuda.Stream() for _ in range(max(1, min(int(n_streams), B)))]
    ctxs = []
    try:
        for b, det in enumerate(dets):
            det = det if isinstance(det, torch.Tensor) else torch.as_tensor(np.asarray(det, dtype=np.float64))
            x0 = _initial_x0(det, None if x0s is None else x0s[b], init, (k_arr, d_arr, r_arr, t_arr), dlc_thresh,
                             start_frames[b], model, f"x0 of sequence {b} must be [N, 45]")
            s = streams[b % len(streams)]
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                ctx = FTEContext(det, k_arr, d_arr, r_arr, t_arr, Ts, dlc_thresh=dlc_thresh, shared_gpu=True, camera_model=model,
                                 **kw)
                ctxs.append(ctx)
                ctx.enable_graph(True)
                ctx.set_x(x0[:, ACTIVE])
        infos = [None] * B
        running = list(range(B))
        done_iter = 0
        while running and done_iter < max_iter:
            chunk = min(int(peek_every), max_iter - done_iter)
            for _ in range(chunk):
                for b in running:
                    with torch.cuda.stream(streams[b % len(streams)]):
                        ctxs[b].step()
            done_iter += chunk
            still = []
            for b in running:
                with torch.cuda.stream(streams[b % len(streams)]):
                    infos[b] = ctxs[b].state()
                if infos[b]["status"] == 0:
                    still.append(b)
            running = still
        out = []
        conv = (lambda a: a.cpu().numpy()) if return_numpy else (lambda a: a)
        for b in range(B):
            with torch.cuda.stream(streams[b % len(streams)]):
                if infos[b] is None:
                    infos[b] = ctxs[b].state()
                if infos[b]["status"] == 5:
                    raise RuntimeError(f"FTE: block factorisation hit a non-positive pivot (sequence {b})")
                x, pos, dx, ddx = ctxs[b].result()
                res = dict(positions=conv(pos), x=conv(x), dx=conv(dx), ddx=conv(ddx), start_frame=start_frames[b])
                _attach_posterior(res, ctxs[b]._posterior(*extras), conv)
                out.append((res, infos[b]))
        for s in streams:
            torch.cuda.current_stream().wait_stream(s)
        return out
    finally:
        for ctx in ctxs:
            ctx.close()
