// The link-scale fit as one path with two measurements (skel_link_scale.hip: 3-D points; skel_link_scale_px.hip: the detections
// of every camera).  Here, once: the most groups a call may name, the arguments and the LDS regions both kernels have, the op
// mask of every group, the per-frame load of x, m and pinned, the K scale directions as the columns P .. P + K - 1 of S.Jw
// (lsc_scale_jacobian<RAW>), the store of the Gram product that splits a result row into A, B and the mirrored C, the forward
// substitution of several right-hand sides on the register-resident factor, the elimination of a frame's pose from the joint
// (pose, log-scale) system once A, B, C, g and c are in LDS, the per-frame stores - and the host side of both C entries: the
// group checks, the fill of the shared arguments, the dispatch over PT with the summing launch behind it.
//
// A kernel keeps what its measurement defines: its regions of the LDS, the cost, how the rows of [Jw Js] come about, the Gram
// product (one pass, or carried across the cameras) and the order in which g and c are summed.  k_link_scale_total is defined in
// skel_link_scale.hip; lsc_launch_total is its host launcher (no device code is linked across files).
#pragma once
#include "pose_fit_skel.hpp"

namespace acino {

constexpr int LSC_MAXK = 16;

// what a frame leaves behind: S, r, F, used and the status (zeros and NaN in sens for a frame that did not enter)
struct LscOut {
  double *S, *r, *F, *sens;
  uint8_t *used, *frame_status;
};

// the arguments both kernels have: the link program, the pose fit's x, ridge centre, active set and status, the outputs
struct LscArgs {
  const SkelDev* dev;
  const double *x, *m;
  const uint8_t *pinned, *status;
  int64_t n_frames;
  LscOut out;
  double kappa;
  int K;
  int8_t grp[ACINO_SKEL_MAX_OPS];  // per op: its group, -1: fixed
};

// offsets into the dynamic LDS, in units of 8 bytes: spf_layout with Jw widened by the K columns of Js, around the
// measurement's own regions (``middle``) and B (K columns of PT; Y takes its place), C and c; behind it the op mask of every
// group and, for the 3-D measurement, ent
struct LscLayout {
  SpfLayout s;
  int B, C, c, gm, ent, total;
};
template <class Middle>
__host__ __device__ inline LscLayout lsc_layout_around(int P, int PT, int n_pose, int n_ops, int K, bool with_ent, Middle&& middle) {
  LscLayout L;
  SpfTake take;
  L.s = spf_layout(P, PT, n_pose, n_ops, take, [&](SpfTake& t) {
    middle(t);
    L.B = t(LSC_MAXK * PT);
    L.C = t(LSC_MAXK * LSC_MAXK);
    L.c = t(LSC_MAXK);
  }, P + K);
  L.gm = take(LSC_MAXK);
  L.ent = with_ent ? take((n_pose + 1) / 2) : 0;
  L.total = take.o;
  return L;
}

// B, C, c and the group masks of a carved workgroup
struct LscLds {
  double *Bm, *Cm, *cv;
  unsigned long long* gm;
};
__device__ __forceinline__ LscLds lsc_carve(double* base, const LscLayout& lay) {
  return LscLds{base + lay.B, base + lay.C, base + lay.c, reinterpret_cast<unsigned long long*>(base + lay.gm)};
}

// once per workgroup: per group the ops that carry its scale
__device__ __forceinline__ void lsc_group_masks(unsigned long long* gm, const int8_t* grp, int n_ops, int lane) {
  if (lane < LSC_MAXK) {
    unsigned long long om = 0;
    for (int k = 0; k < n_ops; ++k)
      if (grp[k] == lane) om |= 1ull << k;
    gm[lane] = om;
  }
}

// frame n's x and m into S, its active set as the return value (the same in every lane); the caller's barrier follows
__device__ __forceinline__ unsigned long long lsc_load_frame(const Spf& S, const LscArgs& a, int64_t n, int lane) {
  const int P = S.P;
  bool pin = false;
  if (lane < P) {
    S.x[lane] = a.x[n * P + lane];
    S.m[lane] = lane >= 3 ? a.m[n * P + lane] : 0.0;
    pin = a.pinned[n * P + lane] != 0;
  }
  return __ballot(pin);
}

// the scale directions as the columns P .. P + K - 1 of S.Jw: the sum of M_k off_k over the ops of group g on the slot's path,
// whitened by U where S.ent[l] says the slot enters - RAW: as it is, where any0 | any1 (the slots some camera detects) has the
// slot's bit; exact zeros elsewhere and where no op of the group lies on the path
template <bool RAW>
__device__ __forceinline__ void lsc_scale_jacobian(const Spf& S, const unsigned long long* gm, int K, unsigned long long any0,
                                                   unsigned long long any1, int lane) {
  lane = spf_here(lane);
  const int T = K * S.n_pose;
  for (int t = lane; t < T; t += 64) {
    const int g = t / S.n_pose, l = t - g * S.n_pose;
    double w0 = 0.0, w1 = 0.0, w2 = 0.0;
    unsigned long long mk = gm[g] & S.pm[l];
    const bool in = RAW ? ((l < 64 ? any0 : any1) >> (l & 63)) & 1ull : S.ent[l] != 0;
    if (mk && in) {
      double j0 = 0.0, j1 = 0.0, j2 = 0.0;
      while (mk) {
        const int k = __ffsll((long long)mk) - 1;
        mk &= mk - 1;
        const double* dv = S.opv + k * 12;
        j0 += dv[0];
        j1 += dv[1];
        j2 += dv[2];
      }
      if (RAW) {
        w0 = j0, w1 = j1, w2 = j2;
      } else {
        const double* U = S.U + 6 * l;
        w0 = U[0] * j0;
        w1 = U[1] * j0 + U[2] * j1;
        w2 = U[3] * j0 + U[4] * j1 + U[5] * j2;
      }
    }
    double* o = S.Jw + (S.P + g) * S.ldj + 3 * l;
    o[0] = w0;
    o[1] = w1;
    o[2] = w2;
  }
  __syncthreads();
}

// the store of the Gram product of the P + K columns: result rows below P are A's (into S.M, lower triangle), rows
// P .. P + K - 1 hold B in the columns below P and C's lower triangle beyond (mirrored: symmetric bit for bit)
template <int PT>
__device__ __forceinline__ auto lsc_gram_store(const Spf& S, int K, const LscLds& W) {
  return [M = S.M, Bm = W.Bm, Cm = W.Cm, P = S.P, K](int row, int col, double v) {
    if (row < P) {
      M[row * (PT + 1) + col] = v;
    } else if (row < P + K) {
      const int g = row - P;
      if (col < P) {
        Bm[g * PT + col] = v;
      } else {
        Cm[g * LSC_MAXK + col - P] = v;
        Cm[(col - P) * LSC_MAXK + g] = v;
      }
    }
  };
}

// v <- L^-1 v for NC right-hand sides at once, lane p holding entry p of each: the forward half of pf_solve
template <int N, int NC>
__device__ __forceinline__ void lsc_forward(const double (&r)[N], double dinv, double (&v)[NC], int lane) {
#pragma unroll
  for (int k = 0; k < N; ++k)
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const double zk = pf_readlane(v[c] * dinv, k);
      v[c] = lane == k ? zk : (lane > k ? v[c] - r[k] * zk : v[c]);
    }
}

// The elimination in three steps on the register-resident factor (r, dinv; row i in lane i).  A in S.M (lower triangle), B in Bm
// (K columns of PT), C in Cm (LSC_MAXK x LSC_MAXK, mirrored), g in S.g, c in cv, F the frame's cost.
// lsc_factor: A_FF = L L^T with lam = 0 (pinned rows the identity's).  False (the same in every lane) when there is no factor or
// F or x is not finite.
template <int PT>
__device__ __forceinline__ bool lsc_factor(SkelCore<PT>& core, unsigned long long fixmask, double F, double (&r)[PT], double& dinv,
                                           int lane) {
  bool ok = core.factor(fixmask, 0.0, lane, r, dinv) && m_finite(F);
  if (lane < core.S.P) ok = ok && m_finite(core.S.x[lane]);
  return __all(ok);
}

// lsc_sens: sens = -A_FF^-1 B_F into ``sens`` [P][K] (pinned rows exactly 0).  Before lsc_reduce: it reads B, whose place Y takes
template <int PT>
__device__ __forceinline__ void lsc_sens(const SkelCore<PT>& core, unsigned long long fixmask, int K, const double* Bm,
                                         const double (&r)[PT], double dinv, double* sens, int lane) {
  const int P = core.S.P;
  const bool free_p = lane < P && !((fixmask >> lane) & 1);
#pragma unroll 1
  for (int g = 0; g < K; ++g) {
    const double b = free_p ? Bm[g * PT + lane] : 0.0;
    const double d = core.solve(r, dinv, -b, lane);
    if (lane < P) sens[lane * K + g] = free_p ? d : 0.0;
  }
}

// lsc_reduce: Y = L^-1 B_F in B's place and v = L^-1 g_F in g's, four columns at a time, then S = C - Y^T Y (lower triangle,
// mirrored: symmetric bit for bit) in Cm and r = c - Y^T v in cv, one entry per lane, summed over the states in state order.
// False (the same in every lane) when a value is not finite.
template <int PT>
__device__ __forceinline__ bool lsc_reduce(const Spf& S, unsigned long long fixmask, int K, double* Bm, double* Cm, double* cv,
                                           const double (&r)[PT], double dinv, int lane) {
  const int P = S.P;
  const bool free_p = lane < P && !((fixmask >> lane) & 1);
#pragma unroll 1
  for (int c0 = 0; c0 <= K; c0 += 4) {
    double v[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int g = c0 + c;
      v[c] = !free_p || g > K ? 0.0 : (g == K ? S.g[lane] : Bm[g * PT + lane]);
    }
    lsc_forward<PT, 4>(r, dinv, v, spf_here(lane));
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int g = c0 + c;
      if (lane < P && g <= K) (g == K ? S.g : Bm + g * PT)[lane] = v[c];
    }
  }
  __syncthreads();
  bool fin = true;
  for (int t = lane; t < K * (K + 1) / 2 + K; t += 64) {
    int i = 0, j = 0;
    const double* right = S.g;
    const bool tri = t < K * (K + 1) / 2;
    if (tri) {
      while ((i + 1) * (i + 2) / 2 <= t) ++i;
      j = t - i * (i + 1) / 2;
      right = Bm + j * PT;
    } else {
      i = t - K * (K + 1) / 2;
    }
    const double* left = Bm + i * PT;
    double sum = 0.0;
    for (int p = 0; p < P; ++p) sum += left[p] * right[p];
    if (tri) {                                    // (entry (i, j) is read by this lane alone, (j, i) above the diagonal by none)
      const double v = Cm[i * LSC_MAXK + j] - sum;
      fin = fin && m_finite(v);
      Cm[i * LSC_MAXK + j] = v;
      Cm[j * LSC_MAXK + i] = v;
    } else {
      const double v = cv[i] - sum;
      fin = fin && m_finite(v);
      cv[i] = v;
    }
  }
  const bool ok = __all(fin);
  __syncthreads();
  return ok;
}

// the three in turn: S_n, r_n and, when ``sens`` is not NULL, sens_n of a frame; false when the frame does not enter
template <int PT>
__device__ __forceinline__ bool lsc_eliminate(const Spf& S, const SkelDev& D, unsigned long long fixmask, double F, int K, double* Bm,
                                              double* Cm, double* cv, double* sens, int lane) {
  SkelCore<PT> core{S, D, lane};
  double r[PT], dinv;
  if (!lsc_factor<PT>(core, fixmask, F, r, dinv, lane)) return false;
  if (sens) lsc_sens<PT>(core, fixmask, K, Bm, r, dinv, sens, lane);
  return lsc_reduce<PT>(S, fixmask, K, Bm, Cm, cv, r, dinv, lane);
}

__device__ __forceinline__ void lsc_store(const LscOut& o, int64_t n, int P, int K, bool live, int st_in, double F, const double* Cm,
                                          const double* cv, int lane) {
  for (int t = lane; t < K * K; t += 64) o.S[n * K * K + t] = live ? Cm[(t / K) * LSC_MAXK + t % K] : 0.0;
  if (lane < K) o.r[n * K + lane] = live ? cv[lane] : 0.0;
  if (!live && o.sens)
    for (int t = lane; t < P * K; t += 64) o.sens[n * P * K + t] = __builtin_nan("");
  if (lane == 0) {
    o.F[n] = live ? F : 0.0;
    o.used[n] = live ? 1 : 0;
    o.frame_status[n] = (uint8_t)(live || st_in >= 2 ? st_in : PF_NUMERIC);
  }
}

// [S | r | F | used] of the frames added up in frame order into d_total[K K + K + 2] (k_link_scale_total, skel_link_scale.hip)
int lsc_launch_total(const double* d_S, const double* d_r, const double* d_F, const uint8_t* d_used, int64_t n_frames, int K,
                     double* d_total, hipStream_t s);

// ---- the host side of both entries, in the order of their checks: the entry's own parameters with lsc_check_groups behind
//      them (inside spf_program's check_fit), its LDS check, its n_frames == 0 return and null-buffer check, spf_upload into
//      a.dev, lsc_fill_args, lsc_finish
inline int lsc_check_groups(const acino_skel_fte_params* p, const int32_t* h_group, int n_groups) {
  ACINO_REQUIRE(h_group != nullptr, "null buffer (h_group)");
  for (int k = 0; k < p->n_ops; ++k)
    ACINO_REQUIRE(h_group[k] >= -1 && h_group[k] < n_groups, "h_group: every op's group must be -1 (fixed) or 0..n_groups-1");
  return ACINO_OK;
}

// everything of the block but ``dev`` (spf_upload's)
inline void lsc_fill_args(LscArgs& a, const SkelDev& h, const int32_t* h_group, int n_groups, double prior_sigma, const double* d_x,
                          const double* d_m, const uint8_t* d_pinned, const uint8_t* d_status, int64_t n_frames, double* d_S,
                          double* d_r, double* d_F, uint8_t* d_used, uint8_t* d_frame_status, double* d_sens) {
  a.x = d_x, a.m = d_m, a.pinned = d_pinned, a.status = d_status, a.n_frames = n_frames;
  a.out.S = d_S, a.out.r = d_r, a.out.F = d_F, a.out.sens = d_sens, a.out.used = d_used, a.out.frame_status = d_frame_status;
  a.kappa = 1.0 / (prior_sigma * prior_sigma), a.K = n_groups;
  for (int k = 0; k < ACINO_SKEL_MAX_OPS; ++k) a.grp[k] = (int8_t)(k < h.n_ops ? h_group[k] : -1);
}

// launch(pt) starts the entry's kernel for PT = pt.value; the frames are added up behind it when d_total is given
template <class Launch>
inline int lsc_finish(int PT, const LscArgs& a, double* d_total, hipStream_t s, Launch&& launch) {
  if (int rc = skel_dispatch_pt(PT, launch)) return rc;
  if (d_total) return lsc_launch_total(a.out.S, a.out.r, a.out.F, a.out.used, a.n_frames, a.K, d_total, s);
  return ACINO_OK;
}

}  // namespace acino
