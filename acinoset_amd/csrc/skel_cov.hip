// Error bars for the generic-skeleton FTE (gfx950, fp64): per-frame covariance of the active states and of every pose slot,
// evaluated at a given iterate x (normally the solution of skel_fte.hip).  With the unknowns frame-major,
//     A = blockdiag_n( sum_{c,l,d} w_ncl^2 J_ncld^T J_ncld )  +  2 q D3^T D3 ,      q = model_weight / h^4
// J_ncld = d(pi_c(pose_l(x_n))_d)/dx_n from the solve's own assembly statements (skel_assemble.hpp: same link program,
// same camera functions, same dropped rows: w = 0, non-finite measurements, |z_cam| < 1e-9), D3 the third-difference operator
// of a clip with band_coef's coefficients.  This is the FISHER information of the model the objective states plus the prior:
// sum |w r| is the negative log-likelihood of Laplace noise of scale 1 / w, whose information for location is w^2, and A^-1
// is the asymptotic covariance of the L1 estimate.  The IRLS curvature w^2 / max(|e|, l1_eps) that the solver factors is
// deliberately NOT used: it depends on l1_eps, inflates the information of a well-fitted detection by up to 1 / l1_eps, and
// is a device of the optimiser, not a property of the model.  Every detection above the caller's likelihood threshold counts
// fully - outliers are not discounted: the bars are those of the stated model.  No Marquardt term.
// Bound-active variables are pinned exactly as the solver pins them - skel_fixed(x, g, hd, lo, hi) with the solver's own
// gradient g (L1 + smoothness) and IRLS diagonal hd at x: row and column zeroed, diagonal 1 - and their rows and columns are
// exactly 0 in every output.
// Under the redescending loss (acino_skel_fte_params::loss; k_skel_assemble<true, ., true, double>) the blocks are
// sum w^2 h(e) J^T J: the Gauss-Newton curvature of the stated objective at x, fte_cov.hip's definition.  The loss is e^2 / 2 in
// its core (Gaussian noise of scale 1 / w, h = 1) and constant beyond c (h = 0): a detection the solve has rejected adds no
// information, and the matrix depends on the residuals.  Kept rows, pins, factorisation and outputs are the same; the
// observability pass stays on w^2 (a row is observed whatever its h).
//   k_skel_assemble<.., double>    one workgroup per frame: the assembly kernel with FISHER: H_F, g, hd, link operators
//   k_skel_cov_build               k_skel_build at lam = 0 with H_F for H: band blocks, pin mask, the original diagonal
//   k_skel_selinv<PT>              ONE workgroup per clip.  Forward: the banded block Cholesky of k_skel_solve (panel in LDS,
//                                  diagonal tiles by the register pivot chain, window update in memory), factored panels to
//                                  memory - skel_band_factor<PT> of skel_factor.hpp, shared with skel_sample.hip.  Backward, right to left, the Takahashi recursion: with W = L_nn^-1 and
//                                  Z_j = L_n+j,n W (j = 1..3), and the known blocks S_n+i,n+j of the inverse,
//                                      S_n+i,n = - sum_j S_n+i,n+j Z_j   (i = 1..3),     S_nn = W^T W - sum_j Z_j^T S_n+j,n
//                                  and S_nn symmetrised at every frame (without that the recursion amplifies the rounding-level
//                                  antisymmetric part of the diagonal blocks by an order of magnitude per frame).
//                                  Every block needed lies inside the factor's band: the result is exact.  All products are
//                                  fp64 MFMA 16 x 16 tile products.  W and Z_j replace the panel IN PLACE in LDS (133 KB at
//                                  PT = 64, so nothing else fits at that size); the S blocks replace the factor's blocks in
//                                  memory (band[n][j] = S_n+j,n) and the 3 x 3 window of a frame is read from there as MFMA
//                                  operands - at every PT, one code path: the window is 6 blocks of at most 32 KB written
//                                  by this workgroup one to three frames earlier (L2 hits).
//   k_skel_cov_out, k_skel_cov_pose  one workgroup per frame, streaming: cov_x from S_nn; G_l (3 x P) from the link operators,
//                                  G_l cov_x G_l^T and sqrt(trace)
//   k_skel_observability           (only when the caller asks: acino_skel_fte_observability, or pin_unobserved / d_unobserved of
//                                  the _pinned entries)  one workgroup of one wave per clip, lane p = state p: info[p] = the
//                                  sum over the clip's frames, in frame order, of the diagonal entry (p, p) of the Fisher block;
//                                  the maximum over the states in LDS; a second walk over the same diagonals counts the frames
//                                  above SK_UNOBS_REL * max.  No atomics.  A small reduction, latency-bound (N dependent adds
//                                  per lane on strided loads).  The assembly body adds the prior's diagonal 2 q b0 to H in the
//                                  same statement as the Fisher sum, and (s + c) - c does not give s back, so the diagonals
//                                  this kernel reads come from a run of the Fisher assembly on a second SkelDev with q = 0:
//                                  there H IS the Fisher block, bit for bit (s + 2 * 0 * b0).  That run's H, g, hd, opv are
//                                  overwritten by the real assembly that follows on the same stream.
//                                  An unobserved state - info[p] <= SK_UNOBS_REL * max_q info[q]: no frame of the clip moves any
//                                  weighted pixel with it - can be pinned in every frame of the clip (k_skel_cov_build's mask):
//                                  row and column 0, diagonal 1, the prior's couplings dropped, exactly a bound pin.  A pose slot
//                                  whose G_l has a nonzero entry in the column of an unobserved state is undetermined under the
//                                  stated model: std_pos = +inf, cov_pos = NaN (k_skel_cov_pose).
// A pivot p of the factorisation that is not above SK_PIV_REL * A_pp - non-positive, or positive only by the rounding of the
// cancellation A_pp - sum L^2 - marks the clip singular (a state observed in no frame of the clip: the prior alone leaves its
// quadratic drift free): status 5, outputs NaN.  One clip is latency-bound by construction, as the solve; the call is meant
// for batches (a video is 78 windows).
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <limits>
#include <vector>

#include "skel_assemble.hpp"
#include "skel_factor.hpp"

namespace acino {

// ---- Fisher assembly: the solve's assembly kernel with the trailing opv_out argument, k_skel_assemble<true, PINHOLE, ROBUST, double>
//      of skel_assemble.hpp, current iterate only (the clip words are all zero: status 0, buffer 0).  Under the redescending loss
//      the block that goes to H is the Gauss-Newton curvature sum w^2 h(e) J^T J of the stated objective (fte_cov.hip's
//      definition; unlike the L1 Fisher block it depends on the residuals), g / hd / cost the robust solver's own.

// ---- the host half of a SkelDev (everything before the camera records, 2.9 KB) by value in the kernel-argument segment:
//      an asynchronous copy would read the caller's stack after an early return, or after the return of an entry that does not
//      synchronise (acino_skel_fte_observability).  skel_upload (skel_host.hpp) is its only launch site, for every entry.
struct SkelDevHead {
  unsigned long long w[offsetof(SkelDev, cams) / 8];
};
static_assert(offsetof(SkelDev, cams) % 8 == 0 && sizeof(SkelDevHead) == offsetof(SkelDev, cams) && sizeof(SkelDevHead) <= 3584,
              "SkelDev's host half as a kernel argument");
// (the loss record sits behind the camera records, so that every offset before it stayed: it travels as a second argument)
struct SkelDevTail {
  unsigned long long w[(sizeof(SkelDev) - offsetof(SkelDev, loss)) / 8];
};
static_assert(offsetof(SkelDev, loss) % 8 == 0 && sizeof(SkelDevTail) == sizeof(SkelDev) - offsetof(SkelDev, loss),
              "SkelDev's loss record as a kernel argument");
__global__ void __launch_bounds__(256) k_skel_dev_store(SkelDevHead a, SkelDevTail t, SkelDev* __restrict__ out) {
  unsigned long long* o = reinterpret_cast<unsigned long long*>(out);
  for (int e = threadIdx.x; e < (int)(sizeof(SkelDevHead) / 8); e += 256) o[e] = a.w[e];
  for (int e = threadIdx.x; e < (int)(sizeof(SkelDevTail) / 8); e += 256) o[offsetof(SkelDev, loss) / 8 + e] = t.w[e];
}

// ---- which states does the clip observe?  One wave per clip, lane p = active state p.  H: the Fisher blocks [NT][P][P] of an
//      assembly with q = 0 (only their diagonals are read).  info / n_seen / unobs_a / unobs_b: [n_clips][P], any may be NULL
__global__ void __launch_bounds__(64)
k_skel_observability(const SkelDev* __restrict__ dev, const double* __restrict__ H, double* __restrict__ info,
                     int32_t* __restrict__ n_seen, unsigned char* __restrict__ unobs_a, unsigned char* __restrict__ unobs_b) {
  const SkelDev& D = *dev;
  const int b = blockIdx.x, p = threadIdx.x, P = D.n_act, N = D.n_frames;
  __shared__ double mx[64];
  const size_t step = (size_t)P * P;
  const double* Hd = H + (size_t)b * N * step + (size_t)(p < P ? p : 0) * (P + 1);      // entry (p, p) of the clip's first frame
  double s = 0.0;
  if (p < P)
    for (int n = 0; n < N; ++n) s += Hd[(size_t)n * step];
  mx[p] = p < P ? s : 0.0;
  __syncthreads();
  for (int off = 32; off > 0; off >>= 1) {
    if (p < off) mx[p] = fmax(mx[p], mx[p + off]);
    __syncthreads();
  }
  const double thr = SK_UNOBS_REL * mx[0];
  if (p >= P) return;
  int seen = 0;
  for (int n = 0; n < N; ++n) seen += Hd[(size_t)n * step] > thr ? 1 : 0;
  const size_t o = (size_t)b * P + p;
  const unsigned char u = s <= thr ? 1 : 0;
  if (info) info[o] = s;
  if (n_seen) n_seen[o] = seen;
  if (unobs_a) unobs_a[o] = u;
  if (unobs_b) unobs_b[o] = u;
}

// ---- the banded system at lam = 0 (k_skel_build's statements): band[n][j] = block (n + j, n), [PT][PT] row-major;
//      fxm[n][PT] the pin mask; diag0[n][PT] the diagonal of A as built (the pivot test's yardstick).  unobs: NULL, or the
//      clips' masks [n_clips][P] of k_skel_observability: such a state is pinned in every frame of its clip
__global__ void __launch_bounds__(256)
k_skel_cov_build(const SkelDev* __restrict__ dev, const double* __restrict__ x, const double* __restrict__ g,
                 const double* __restrict__ H, const double* __restrict__ hd, const double* __restrict__ lo,
                 const double* __restrict__ hi, double* __restrict__ band, unsigned char* __restrict__ fxm,
                 double* __restrict__ diag0, const unsigned char* __restrict__ unobs) {
  const SkelDev& D = *dev;
  const int tid = threadIdx.x, n = blockIdx.x, P = D.n_act, PT = D.PT, N = D.n_frames, nl = n % N;
  __shared__ unsigned char fx[4][SK_MAXP];
  for (int e = tid; e < 4 * P; e += 256) {
    const int j = e / P, p = e % P;
    bool f = false;
    if (nl + j < N) {
      const size_t q = (size_t)(n + j) * P + p;
      f = skel_fixed(x[q], g[q], hd[q], lo[q], hi[q]);
    }
    if (unobs && unobs[(size_t)(n / N) * P + p]) f = true;
    fx[j][p] = f ? 1 : 0;
  }
  __syncthreads();
  double* B = band + (size_t)n * 4 * PT * PT;
  for (int e = tid; e < PT * PT; e += 256) {
    const int p = e / PT, pc = e % PT;
    double v = 0.0;
    if (p < P && pc < P) {
      if (fx[0][p] || fx[0][pc]) v = p == pc ? 1.0 : 0.0;
      else v = H[((size_t)n * P + p) * P + pc];
    } else if (p == pc) v = 1.0;
    B[e] = v;
    if (p == pc) diag0[(size_t)n * PT + p] = v;
#pragma unroll
    for (int j = 1; j < 4; ++j) {
      double c = 0.0;
      if (p == pc && p < P && nl + j < N && !fx[0][p] && !fx[j][p]) c = 2.0 * D.q * band_coef(nl, j, N);
      B[(size_t)j * PT * PT + e] = c;
    }
  }
  if (tid < PT) fxm[(size_t)n * PT + tid] = tid < P ? fx[0][tid] : 0;
}

// ---- selected inverse, one workgroup per clip (sk_tile_mac, SKC_T and the forward pass: skel_factor.hpp) -------------------
template <int PT>
__global__ void __launch_bounds__(SKC_T)
k_skel_selinv(const SkelDev* __restrict__ dev, SkelClip* __restrict__ clip, double* __restrict__ band_all,
              const double* __restrict__ diag0_all) {
  constexpr int LDP = PT + 1, NTP = PT / 16, NT2 = NTP * NTP, BB = PT * PT;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  SkelClip& cs = clip[blockIdx.x];
  int* const numeric_err = &cs.pivot_err;
  const int N = dev->n_frames;
  const size_t fr0 = (size_t)blockIdx.x * N;                 // the clip's first frame
  double* const band = band_all + fr0 * 4 * BB;
  const double* const diag0 = diag0_all + fr0 * PT;
  double* Pn = reinterpret_cast<double*>(smem_raw);          // [4 PT][LDP]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, lk = lane >> 4;
  auto load_panel = [&](int n) { skel_load_panel<PT>(Pn, band, n, N); };
  // ---------------- forward: the factorisation of k_skel_solve (no right-hand side) ----------------
  skel_band_factor<PT>(N, band, diag0, numeric_err, Pn);
  {
    __shared__ int failed;
    if (tid == 0) {
      failed = __hip_atomic_load(numeric_err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
      if (failed) cs.status = 5;
    }
    __syncthreads();
    if (failed) return;
  }
  // ---------------- backward: the Takahashi recursion ----------------
  // block S_a,b of the inverse (a, b frames of the window, already computed): entry (r, k)
  auto s_block = [&](int a, int b) -> const double* { return band + ((size_t)std::min(a, b) * 4 + (a > b ? a - b : b - a)) * BB; };
  for (int n = N - 1; n >= 0; --n) {
    load_panel(n);
    __syncthreads();
    // ---- W = L_nn^-1 in place of the frame's own block: diagonal tiles hold U_kk = L_kk^-T, transpose them; then row by row
    //      W(r, c) = - W(r, r) sum_{c <= k < r} L(r, k) W(k, c): a row's tiles into registers, then over the row's L tiles
    if (wave < NTP) {
      double* T = Pn + (wave * 16) * LDP + wave * 16;
      double v[4];
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) v[rr] = T[(lk + 4 * rr) * LDP + li];
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) T[li * LDP + lk + 4 * rr] = v[rr];
    }
    __syncthreads();
#pragma unroll 1
    for (int r = 1; r < NTP; ++r) {
      d4 w = {0, 0, 0, 0};
      const int c = wave;                                    // tile (r, c), c < r, on wave c
      if (c < r) {
        const double* Lr = Pn + (r * 16 + li) * LDP;
        d4 t = {0, 0, 0, 0};
        t = sk_tile_mac(t, c * 16, r * 16, lk, [&](int k) { return Lr[k]; }, [&](int k) { return Pn[k * LDP + c * 16 + li]; });
        const double* Wrr = Pn + (r * 16 + li) * LDP + r * 16;
#pragma unroll
        for (int s = 0; s < 4; ++s) w = mfma(-Wrr[4 * s + lk], t[s], w);      // (t's accumulator layout IS the B operand's)
      }
      __syncthreads();
      if (c < r) {
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) Pn[(r * 16 + lk + 4 * rr) * LDP + c * 16 + li] = w[rr];
      }
      __syncthreads();
    }
    // ---- Z_j = L_n+j,n W in place of L_n+j,n: tile (rt, ct) = sum_{k >= ct} L(rt, k) W(k, ct); all tiles into registers first
    {
      constexpr int ZT = 3 * NT2, PER = (ZT + SKC_W - 1) / SKC_W;
      d4 z[PER];
#pragma unroll
      for (int q = 0; q < PER; ++q) {
        const int t = wave + SKC_W * q;
        z[q] = d4{0, 0, 0, 0};
        if (t < ZT) {
          const int rt = t / NTP, ct = t % NTP;              // rt over the 3 NTP row tiles below the diagonal block
          const double* Lr = Pn + (PT + rt * 16 + li) * LDP;
          z[q] = sk_tile_mac(z[q], ct * 16, PT, lk, [&](int k) { return Lr[k]; }, [&](int k) { return Pn[k * LDP + ct * 16 + li]; });
        }
      }
      __syncthreads();
#pragma unroll
      for (int q = 0; q < PER; ++q) {
        const int t = wave + SKC_W * q;
        if (t < ZT) {
          const int rt = t / NTP, ct = t % NTP;
#pragma unroll
          for (int rr = 0; rr < 4; ++rr) Pn[(PT + rt * 16 + lk + 4 * rr) * LDP + ct * 16 + li] = z[q][rr];
        }
      }
      __syncthreads();
    }
    // ---- S_n+i,n = - sum_j S_n+i,n+j Z_j (i = 1..3) -> band[n][i]; S_n+i,n+j for j > i is the transpose of S_n+j,n+i
    for (int t = wave; t < 3 * NT2; t += SKC_W) {
      const int i = 1 + t / NT2, rt = (t % NT2) / NTP, ct = t % NTP;
      if (n + i >= N) continue;
      d4 a = {0, 0, 0, 0};
      for (int j = 1; j < 4; ++j) {
        if (n + j >= N) break;
        const double* Sb = s_block(n + i, n + j);
        const double* Zj = Pn + (size_t)(j * PT) * LDP + ct * 16 + li;
        if (i >= j) {
          const double* Sr = Sb + (size_t)(rt * 16 + li) * PT;
          a = sk_tile_mac(a, 0, PT, lk, [&](int k) { return -Sr[k]; }, [&](int k) { return Zj[k * LDP]; });
        } else {
          const double* Sc = Sb + rt * 16 + li;
          a = sk_tile_mac(a, 0, PT, lk, [&](int k) { return -Sc[(size_t)k * PT]; }, [&](int k) { return Zj[k * LDP]; });
        }
      }
      double* Cg = band + ((size_t)n * 4 + i) * BB;
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) Cg[(rt * 16 + lk + 4 * rr) * PT + ct * 16 + li] = a[rr];
    }
    __syncthreads();                                         // the new column is read back below (same workgroup)
    // ---- S_nn = W^T W - sum_j Z_j^T S_n+j,n -> band[n][0]
    for (int t = wave; t < NT2; t += SKC_W) {
      const int rt = t / NTP, ct = t % NTP;
      d4 a = {0, 0, 0, 0};
      a = sk_tile_mac(a, std::max(rt, ct) * 16, PT, lk, [&](int k) { return Pn[k * LDP + rt * 16 + li]; },
                      [&](int k) { return Pn[k * LDP + ct * 16 + li]; });
      for (int j = 1; j < 4; ++j) {
        if (n + j >= N) break;
        const double* Zj = Pn + (size_t)(j * PT) * LDP + rt * 16 + li;
        const double* Sj = band + ((size_t)n * 4 + j) * BB + ct * 16 + li;
        a = sk_tile_mac(a, 0, PT, lk, [&](int k) { return -Zj[k * LDP]; }, [&](int k) { return Sj[(size_t)k * PT]; });
      }
      double* Cg = band + (size_t)n * 4 * BB;
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) Cg[(rt * 16 + lk + 4 * rr) * PT + ct * 16 + li] = a[rr];
    }
    __syncthreads();
    // ---- S_nn <- (S_nn + S_nn^T) / 2.  Not cosmetic: the rounding-level antisymmetric part of a diagonal block is the one error
    //      mode the recursion amplifies (about 10 x per frame on the shipped detections, |Z_1|, |Z_2| ~ 3: the third-difference
    //      prior extrapolates); projected out at every frame, the blocks stay at the accuracy of the factor.
    {
      double* Cg = band + (size_t)n * 4 * BB;
      for (int e = tid; e < BB; e += SKC_T) {
        const int p = e / PT, pc = e % PT;
        if (p > pc) {
          const double v = 0.5 * (Cg[p * PT + pc] + Cg[pc * PT + p]);
          Cg[p * PT + pc] = v;
          Cg[pc * PT + p] = v;
        }
      }
    }
    __syncthreads();
  }
}

// ---- outputs -------------------------------------------------------------------------------------------------------
// cov_x[n][P][P] from S_nn (its lower triangle, mirrored); pinned rows / columns 0; NaN for a singular clip
__global__ void __launch_bounds__(256)
k_skel_cov_out(const SkelDev* __restrict__ dev, const SkelClip* __restrict__ clip, const double* __restrict__ band,
               const unsigned char* __restrict__ fxm, double* __restrict__ cov_x) {
  const SkelDev& D = *dev;
  const int n = blockIdx.x, P = D.n_act, PT = D.PT;
  const bool bad = clip[n / D.n_frames].status != 0;
  const double* S = band + (size_t)n * 4 * PT * PT;
  const unsigned char* fx = fxm + (size_t)n * PT;
  for (int e = threadIdx.x; e < P * P; e += 256) {
    const int p = e / P, pc = e % P;
    double v = (fx[p] || fx[pc]) ? 0.0 : S[(size_t)max(p, pc) * PT + min(p, pc)];
    if (bad) v = __builtin_nan("");
    cov_x[(size_t)n * P * P + e] = v;
  }
}

// cov_pos[n][l] = G_l cov_x G_l^T, std_pos[n][l] = sqrt(trace): G_l = [I | d(M off)/d(angle) of the ops on slot l's path].
// unobs: NULL, or the clips' masks [n_clips][P]: a slot with a nonzero entry of G_l in the column of an unobserved state gets
// std_pos = +inf and cov_pos = NaN (the state is held at x by the pin, but nothing in the clip says where it is)
__global__ void __launch_bounds__(256)
k_skel_cov_pose(const SkelDev* __restrict__ dev, const SkelClip* __restrict__ clip, const double* __restrict__ band,
                const unsigned char* __restrict__ fxm, const double* __restrict__ opv_all, double* __restrict__ cov_pos,
                double* __restrict__ std_pos, const unsigned char* __restrict__ unobs) {
  const SkelDev& D = *dev;
  const int n = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int P = D.n_act, PT = D.PT, NPOSE = D.n_pose, NOPS = D.n_ops;
  if (clip[n / D.n_frames].status != 0) {
    const double nan = __builtin_nan("");
    for (int e = tid; e < NPOSE * 9; e += 256)
      if (cov_pos) cov_pos[(size_t)n * NPOSE * 9 + e] = nan;
    for (int e = tid; e < NPOSE; e += 256)
      if (std_pos) std_pos[(size_t)n * NPOSE + e] = nan;
    return;
  }
  __shared__ double Cm[SK_MAXP][SK_MAXP + 1];
  __shared__ double opv[ACINO_SKEL_MAX_OPS * 12];
  __shared__ double G[4][3][SK_MAXP], T[4][3][SK_MAXP], out9[4][9];
  const double* S = band + (size_t)n * 4 * PT * PT;
  const unsigned char* fx = fxm + (size_t)n * PT;
  for (int e = tid; e < P * P; e += 256) {
    const int p = e / P, pc = e % P;
    Cm[p][pc] = (fx[p] || fx[pc]) ? 0.0 : S[(size_t)max(p, pc) * PT + min(p, pc)];
  }
  for (int e = tid; e < NOPS * 12; e += 256) opv[e] = opv_all[(size_t)n * NOPS * 12 + e];
  __syncthreads();
  for (int l0 = 0; l0 < NPOSE; l0 += 4) {
    const int l = l0 + wave;
    const bool on = l < NPOSE;
    bool dep = false;
    if (on && lane < P) {
      double gc[3];
      skel_pose_jac_col(D, opv, l, lane, gc);
      G[wave][0][lane] = gc[0];
      G[wave][1][lane] = gc[1];
      G[wave][2][lane] = gc[2];
      if (unobs) dep = unobs[(size_t)(n / D.n_frames) * P + lane] && (gc[0] != 0.0 || gc[1] != 0.0 || gc[2] != 0.0);
    }
    const bool undet = __any(dep ? 1 : 0) != 0;              // (wave-wide: a wave is one pose slot)
    __syncthreads();
    if (on && lane < P) {
      double t0 = 0.0, t1 = 0.0, t2 = 0.0;
      for (int q = 0; q < P; ++q) {
        const double c = Cm[q][lane];
        t0 += G[wave][0][q] * c;
        t1 += G[wave][1][q] * c;
        t2 += G[wave][2][q] * c;
      }
      T[wave][0][lane] = t0;
      T[wave][1][lane] = t1;
      T[wave][2][lane] = t2;
    }
    __syncthreads();
    if (on && lane < 9) {
      const int i = lane / 3, j = lane % 3;
      double s = 0.0;
      for (int q = 0; q < P; ++q) s += T[wave][i][q] * G[wave][j][q];
      out9[wave][lane] = s;
      if (cov_pos) cov_pos[((size_t)n * NPOSE + l) * 9 + lane] = undet ? __builtin_nan("") : s;
    }
    __syncthreads();
    if (on && lane == 0 && std_pos)
      std_pos[(size_t)n * NPOSE + l] = undet ? __builtin_inf() : sqrt(fmax(out9[wave][0] + out9[wave][4] + out9[wave][8], 0.0));
    __syncthreads();
  }
}

SkelCovLayout skel_cov_layout(size_t NT, int n_clips, int P, int PT, int n_ops, bool observe) {
  SkelCovLayout L;
  SkelTake take;
  L.dev = take(sizeof(SkelDev));
  L.clip = take(sizeof(SkelClip) * (size_t)n_clips);
  L.H = take(sizeof(double) * NT * P * P);
  L.g = take(sizeof(double) * NT * P);
  L.hd = take(sizeof(double) * NT * P);
  L.cost = take(sizeof(double) * NT);
  L.opv = take(sizeof(double) * NT * (size_t)std::max(n_ops, 1) * 12);
  L.band = take(sizeof(double) * NT * 4 * PT * PT);
  L.diag0 = take(sizeof(double) * NT * PT);
  L.fxm = take(NT * PT);
  L.dev0 = L.unobs = 0;
  if (observe) {
    L.dev0 = take(sizeof(SkelDev));
    L.unobs = take((size_t)n_clips * P);
  }
  L.total = take.off;
  return L;
}

int skel_upload(const SkelDev& h, const double* d_cams, int camera_model, SkelDev* d_dev, SkelClip* d_clip, int n_clips,
                hipStream_t s) {
  SkelDevHead head;
  memcpy(&head, &h, sizeof(head));
  SkelDevTail tail;
  memcpy(&tail, &h.loss, sizeof(tail));
  hipLaunchKernelGGL(k_skel_dev_store, dim3(1), dim3(256), 0, s, head, tail, d_dev);
  ACINO_LAUNCH_CHECK();
  const bool pinhole = camera_model == 1;
  if (d_cams)                                    // (NULL: an entry that reads the link program alone - acino_skel_pose_fit)
    ACINO_HIP_CHECK(hipMemcpyAsync(reinterpret_cast<char*>(d_dev) + (pinhole ? offsetof(SkelDev, pins) : offsetof(SkelDev, cams)),
                                 d_cams, sizeof(double) * (pinhole ? ACINO_PINHOLE_STRIDE : ACINO_CAM_STRIDE) * h.n_cams,
                                 hipMemcpyDeviceToDevice, s));
  ACINO_HIP_CHECK(hipMemsetAsync(d_clip, 0, sizeof(SkelClip) * (size_t)n_clips, s));
  return ACINO_OK;
}

int skel_read_status(const SkelClip* d_clip, int n_clips, hipStream_t s, bool per_clip_output, const char* numeric_text,
                     std::vector<SkelClip>& hc) {
  hc.resize(n_clips);
  ACINO_HIP_CHECK(hipMemcpyAsync(hc.data(), d_clip, sizeof(SkelClip) * (size_t)n_clips, hipMemcpyDeviceToHost, s));
  ACINO_HIP_CHECK(hipStreamSynchronize(s));
  bool numeric = false;
  for (const SkelClip& c : hc) numeric = numeric || c.status == 5;
  if (numeric && (n_clips == 1 || !per_clip_output)) {
    set_error("%s", numeric_text);
    return ACINO_ERR_NUMERIC;
  }
  return ACINO_OK;
}

int skel_cov_read_status(const SkelClip* d_clip, int n_clips, hipStream_t s, int32_t* h_status) {
  std::vector<SkelClip> hc;
  const int rc = skel_read_status(
      d_clip, n_clips, s, h_status != nullptr,
      "pivot not above zero in the banded factorisation of the Fisher information (a state observed in no frame of the clip)", hc);
  if (h_status && (rc == ACINO_OK || rc == ACINO_ERR_NUMERIC))
    for (int b = 0; b < n_clips; ++b) h_status[b] = hc[b].status;
  return rc;
}

// h to d_dev, then the Fisher assembly at d_x on stream s: H = the Fisher blocks (+ the prior's diagonal 2 q b0), g, hd, cost
// and the link operators opv of every frame into the workspace.  What the observability pass (q = 0, a SkelDev of its own) and
// the band's build start with.
static int skel_cov_assemble_at(const SkelDev& h, int n_clips, int camera_model, const double* d_meas, const double* d_w,
                                const double* d_cams, const double* d_x, void* d_ws, const SkelCovLayout& lay, SkelDev* d_dev,
                                hipStream_t s) {
  const size_t NT = (size_t)h.n_frames * n_clips;
  const size_t lds_asm = skel_assemble_lds(h.n_rows, h.n_act) + sizeof(double) * h.n_rows;      // + the Fisher weights
  ACINO_REQUIRE(lds_asm <= 160 * 1024, "residual rows x active states do not fit the assembly's LDS");
  using AssembleKernel = SkelFisherKernel;
  const AssembleKernel assembly[2][2] = {                                  // [loss][camera model] of <JAC, PINHOLE, ROBUST, double>
      {k_skel_assemble<true, false, false, double>, k_skel_assemble<true, true, false, double>},
      {k_skel_assemble<true, false, true, double>, k_skel_assemble<true, true, true, double>}};
  static PerDeviceOnce attr;
  if (attr.first())
    for (const auto& loss : assembly)
      for (AssembleKernel k : loss)
        ACINO_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  char* base = (char*)d_ws;
  auto D = [&](size_t off) { return reinterpret_cast<double*>(base + off); };
  SkelClip* d_clip = reinterpret_cast<SkelClip*>(base + lay.clip);
  int rc;
  if ((rc = skel_upload(h, d_cams, camera_model, d_dev, d_clip, n_clips, s))) return rc;
  const AssembleKernel* by_model = assembly[h.loss_kind == ACINO_SKEL_LOSS_REDESCENDING];
  hipLaunchKernelGGL(skel_camera_kernel(camera_model, by_model[0], by_model[1]), dim3((unsigned)NT),
                     dim3(256), lds_asm, s, d_dev, d_clip, 0, d_x, d_x, d_meas, d_w, D(lay.H), D(lay.H), D(lay.g), D(lay.g), D(lay.hd),
                     D(lay.hd), D(lay.cost), D(lay.cost), D(lay.opv));
  ACINO_LAUNCH_CHECK();
  return ACINO_OK;
}

// The Fisher assembly with the prior switched off and the reduction over it: h (already compiled by skel_program) goes to the
// SkelDev at dev0_off with q = 0, so that H IS the Fisher block, and k_skel_observability reduces the diagonals.
static int skel_cov_launch_observe(int n_clips, int camera_model, const SkelDev& h, const double* d_meas, const double* d_w,
                                   const double* d_cams, const double* d_x, void* d_ws, const SkelCovLayout& lay, size_t dev0_off,
                                   hipStream_t s, double* d_info, int32_t* d_n_seen, unsigned char* d_unobs_a,
                                   unsigned char* d_unobs_b) {
  SkelDev* d_dev0 = reinterpret_cast<SkelDev*>((char*)d_ws + dev0_off);
  SkelDev h0 = h;
  h0.q = 0.0;                                                 // H_pp = sum w^2 J^2 + 2 * 0 * b0: the Fisher diagonal itself
  h0.loss_kind = ACINO_SKEL_LOSS_L1;                          // a row is observed by the kept-row rule, whatever its h: w^2, not w^2 h
  int rc;
  if ((rc = skel_cov_assemble_at(h0, n_clips, camera_model, d_meas, d_w, d_cams, d_x, d_ws, lay, d_dev0, s))) return rc;
  hipLaunchKernelGGL(k_skel_observability, dim3((unsigned)n_clips), dim3(64), 0, s, d_dev0,
                     reinterpret_cast<const double*>((char*)d_ws + lay.H), d_info, d_n_seen, d_unobs_a, d_unobs_b);
  ACINO_LAUNCH_CHECK();
  return ACINO_OK;
}

int skel_cov_launch_build(const acino_skel_fte_params* p, int n_clips, int camera_model, const acino_skel_op* h_ops,
                          const int32_t* h_active, const double* d_meas, const double* d_w, const double* d_cams,
                          const double* d_lo, const double* d_hi, const double* d_x, void* d_ws, const SkelCovLayout& lay,
                          hipStream_t s, bool observe, bool pin, uint8_t* d_unobserved) {
  const size_t NT = (size_t)p->n_frames * n_clips;
  SkelDev h;
  int rc;
  if ((rc = skel_program(p, h_ops, h_active, h))) return rc;
  char* base = (char*)d_ws;
  auto D = [&](size_t off) { return reinterpret_cast<double*>(base + off); };
  SkelDev* d_dev = reinterpret_cast<SkelDev*>(base + lay.dev);
  unsigned char* d_fxm = reinterpret_cast<unsigned char*>(base + lay.fxm);
  unsigned char* d_unobs = observe ? reinterpret_cast<unsigned char*>(base + lay.unobs) : nullptr;
  if (observe && (rc = skel_cov_launch_observe(n_clips, camera_model, h, d_meas, d_w, d_cams, d_x, d_ws, lay, lay.dev0, s, nullptr,
                                               nullptr, d_unobs, d_unobserved)))
    return rc;
  if ((rc = skel_cov_assemble_at(h, n_clips, camera_model, d_meas, d_w, d_cams, d_x, d_ws, lay, d_dev, s))) return rc;
  hipLaunchKernelGGL(k_skel_cov_build, dim3((unsigned)NT), dim3(256), 0, s, d_dev, d_x, D(lay.g), D(lay.H), D(lay.hd), d_lo, d_hi,
                     D(lay.band), d_fxm, D(lay.diag0), (const unsigned char*)(pin ? d_unobs : nullptr));
  ACINO_LAUNCH_CHECK();
  return ACINO_OK;
}

}  // namespace acino

using namespace acino;

static bool skc_limits(const acino_skel_fte_params* p, int n_clips) {
  return p && p->n_frames >= 1 && p->n_active >= 3 && p->n_active <= SK_MAXP && n_clips >= 1 && p->n_ops >= 0 &&
         p->n_ops <= ACINO_SKEL_MAX_OPS;
}

// The body of the covariance entries: one factorisation and recursion, then the output kernels the caller asked for.  rates:
// NULL (the entries without rates: the launches are what they were), or the four rate outputs of k_skel_cov_rates.
struct SkelRateOut {
  double *cov_dx, *cov_ddx, *cov_vel, *std_vel;
};
static int skc_covariance(const acino_skel_fte_params* p, int n_clips, int camera_model, const acino_skel_op* h_ops,
                          const int32_t* h_active, const double* d_meas, const double* d_w, const double* d_cams,
                          const double* d_lo, const double* d_hi, const double* d_x, double* d_cov_x, double* d_cov_pos,
                          double* d_std_pos, const SkelRateOut* rates, int32_t* h_status, void* d_ws, size_t ws_bytes, void* stream,
                          int pin_unobserved, uint8_t* d_unobserved) {
  int rc = skel_check_batch(p, n_clips, true, camera_model, h_ops && h_active && d_meas && d_w && d_cams && d_lo && d_hi && d_x && d_ws);
  if (rc) return rc;
  ACINO_REQUIRE(pin_unobserved == 0 || pin_unobserved == 1, "pin_unobserved: 0 or 1");
  if (rates)
    ACINO_REQUIRE(d_cov_x || d_cov_pos || d_std_pos || rates->cov_dx || rates->cov_ddx || rates->cov_vel || rates->std_vel,
                  "at least one of d_cov_x, d_cov_pos, d_std_pos, d_cov_dx, d_cov_ddx, d_cov_vel, d_std_vel");
  else
    ACINO_REQUIRE(d_cov_x || d_cov_pos || d_std_pos, "at least one of d_cov_x, d_cov_pos, d_std_pos");
  const int N = p->n_frames, B = n_clips, P = p->n_active, PT = (P + 15) / 16 * 16;
  const size_t NT = (size_t)N * B;                           // frames of all clips
  const bool pin = pin_unobserved == 1, observe = pin || d_unobserved != nullptr;
  const SkelCovLayout lay = skel_cov_layout(NT, B, P, PT, p->n_ops, observe);
  if ((rc = skel_check_workspace(d_ws, ws_bytes, lay.total,
                                 rates ? "acino_skel_fte_covariance_rates_workspace_bytes"
                                 : observe ? "acino_skel_fte_covariance_pinned_workspace_bytes" : "acino_skel_fte_covariance_workspace_bytes",
                                 ACINO_ERR_WORKSPACE)))
    return rc;
  hipStream_t s = (hipStream_t)stream;
  if ((rc = skel_cov_launch_build(p, B, camera_model, h_ops, h_active, d_meas, d_w, d_cams, d_lo, d_hi, d_x, d_ws, lay, s, observe, pin,
                                  d_unobserved)))
    return rc;
  char* base = (char*)d_ws;
  auto D = [&](size_t off) { return reinterpret_cast<double*>(base + off); };
  SkelDev* d_dev = reinterpret_cast<SkelDev*>(base + lay.dev);
  SkelClip* d_clip = reinterpret_cast<SkelClip*>(base + lay.clip);
  unsigned char* d_fxm = reinterpret_cast<unsigned char*>(base + lay.fxm);
  const unsigned char* d_unobs = pin ? reinterpret_cast<const unsigned char*>(base + lay.unobs) : nullptr;
  rc = skel_dispatch_pt(PT, [&](auto pt) -> int {
    constexpr int T = decltype(pt)::value;
    static PerDeviceOnce attr;
    if (attr.first())
      ACINO_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_skel_selinv<T>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                          160 * 1024 - 1024));
    hipLaunchKernelGGL(k_skel_selinv<T>, dim3(B), dim3(SKC_T), skel_factor_lds(T), s, d_dev, d_clip, D(lay.band), D(lay.diag0));
    ACINO_LAUNCH_CHECK();
    return ACINO_OK;
  });
  if (rc) return rc;
  if (d_cov_x) {
    hipLaunchKernelGGL(k_skel_cov_out, dim3((unsigned)NT), dim3(256), 0, s, d_dev, d_clip, D(lay.band), d_fxm, d_cov_x);
    ACINO_LAUNCH_CHECK();
  }
  if (d_cov_pos || d_std_pos) {
    hipLaunchKernelGGL(k_skel_cov_pose, dim3((unsigned)NT), dim3(256), 0, s, d_dev, d_clip, D(lay.band), d_fxm, D(lay.opv), d_cov_pos,
                       d_std_pos, d_unobs);
    ACINO_LAUNCH_CHECK();
  }
  if (rates && (rates->cov_dx || rates->cov_ddx || rates->cov_vel || rates->std_vel) &&
      (rc = skel_cov_launch_rates(NT, P, d_dev, d_clip, D(lay.band), d_fxm, D(lay.opv), d_unobs, p->h, rates->cov_dx, rates->cov_ddx,
                                  rates->cov_vel, rates->std_vel, s)))
    return rc;
  return skel_cov_read_status(d_clip, B, s, h_status);
}


extern "C" {

size_t acino_skel_fte_covariance_workspace_bytes(const acino_skel_fte_params* p, int n_clips) {
  if (!skc_limits(p, n_clips)) return 0;
  const int PT = (p->n_active + 15) / 16 * 16;
  return skel_cov_layout((size_t)p->n_frames * n_clips, n_clips, p->n_active, PT, p->n_ops).total;
}

size_t acino_skel_fte_covariance_pinned_workspace_bytes(const acino_skel_fte_params* p, int n_clips, int pin_unobserved) {
  if (!skc_limits(p, n_clips) || (pin_unobserved != 0 && pin_unobserved != 1)) return 0;
  const int PT = (p->n_active + 15) / 16 * 16;
  return skel_cov_layout((size_t)p->n_frames * n_clips, n_clips, p->n_active, PT, p->n_ops, true).total;
}

// the assembly's arrays only: dev0, clip, H, g, hd, cost, opv (the leading part of the covariance's layout, no band)
static size_t skc_observe_bytes(const acino_skel_fte_params* p, int n_clips, size_t* dev0_off) {
  const int PT = (p->n_active + 15) / 16 * 16;
  const SkelCovLayout lay = skel_cov_layout((size_t)p->n_frames * n_clips, n_clips, p->n_active, PT, p->n_ops);
  if (dev0_off) *dev0_off = lay.band;                        // (in place of the band, which this call does not build)
  return lay.band + skel_align256(sizeof(SkelDev));
}

size_t acino_skel_fte_observability_workspace_bytes(const acino_skel_fte_params* p, int n_clips) {
  if (!skc_limits(p, n_clips)) return 0;
  return skc_observe_bytes(p, n_clips, nullptr);
}

int acino_skel_fte_observability(const acino_skel_fte_params* p, int n_clips, int camera_model, const acino_skel_op* h_ops,
                                 const int32_t* h_active, const double* d_meas, const double* d_w, const double* d_cams,
                                 const double* d_lo, const double* d_hi, const double* d_x, double* d_info, int32_t* d_n_seen,
                                 uint8_t* d_unobserved, void* d_ws, size_t ws_bytes, void* stream) {
  int rc = skel_check_batch(p, n_clips, true, camera_model, h_ops && h_active && d_meas && d_w && d_cams && d_lo && d_hi && d_x && d_ws);
  if (rc) return rc;
  ACINO_REQUIRE(d_info || d_n_seen || d_unobserved, "at least one of d_info, d_n_seen, d_unobserved");
  const size_t NT = (size_t)p->n_frames * n_clips;
  size_t dev0_off = 0;
  const size_t need = skc_observe_bytes(p, n_clips, &dev0_off);
  if ((rc = skel_check_workspace(d_ws, ws_bytes, need, "acino_skel_fte_observability_workspace_bytes", ACINO_ERR_WORKSPACE))) return rc;
  SkelDev h;
  if ((rc = skel_program(p, h_ops, h_active, h))) return rc;
  const int PT = (p->n_active + 15) / 16 * 16;
  const SkelCovLayout lay = skel_cov_layout(NT, n_clips, p->n_active, PT, p->n_ops);
  return skel_cov_launch_observe(n_clips, camera_model, h, d_meas, d_w, d_cams, d_x, d_ws, lay, dev0_off, (hipStream_t)stream, d_info,
                                 d_n_seen, d_unobserved, nullptr);
}

int acino_skel_fte_covariance_pinned(const acino_skel_fte_params* p, int n_clips, int camera_model, const acino_skel_op* h_ops,
                                     const int32_t* h_active, const double* d_meas, const double* d_w, const double* d_cams,
                                     const double* d_lo, const double* d_hi, const double* d_x, double* d_cov_x,
                                     double* d_cov_pos, double* d_std_pos, int32_t* h_status, void* d_ws, size_t ws_bytes,
                                     void* stream, int pin_unobserved, uint8_t* d_unobserved) {
  return skc_covariance(p, n_clips, camera_model, h_ops, h_active, d_meas, d_w, d_cams, d_lo, d_hi, d_x, d_cov_x, d_cov_pos, d_std_pos,
                        nullptr, h_status, d_ws, ws_bytes, stream, pin_unobserved, d_unobserved);
}

size_t acino_skel_fte_covariance_rates_workspace_bytes(const acino_skel_fte_params* p, int n_clips, int pin_unobserved) {
  return acino_skel_fte_covariance_pinned_workspace_bytes(p, n_clips, pin_unobserved);      // (the rates are streamed from the band)
}

int acino_skel_fte_covariance_rates(const acino_skel_fte_params* p, int n_clips, int camera_model, const acino_skel_op* h_ops,
                                    const int32_t* h_active, const double* d_meas, const double* d_w, const double* d_cams,
                                    const double* d_lo, const double* d_hi, const double* d_x, double* d_cov_x, double* d_cov_pos,
                                    double* d_std_pos, double* d_cov_dx, double* d_cov_ddx, double* d_cov_vel, double* d_std_vel,
                                    int32_t* h_status, void* d_ws, size_t ws_bytes, void* stream, int pin_unobserved,
                                    uint8_t* d_unobserved) {
  const SkelRateOut rates = {d_cov_dx, d_cov_ddx, d_cov_vel, d_std_vel};
  return skc_covariance(p, n_clips, camera_model, h_ops, h_active, d_meas, d_w, d_cams, d_lo, d_hi, d_x, d_cov_x, d_cov_pos, d_std_pos,
                        &rates, h_status, d_ws, ws_bytes, stream, pin_unobserved, d_unobserved);
}

int acino_skel_fte_covariance(const acino_skel_fte_params* p, int n_clips, int camera_model, const acino_skel_op* h_ops,
                              const int32_t* h_active, const double* d_meas, const double* d_w, const double* d_cams,
                              const double* d_lo, const double* d_hi, const double* d_x, double* d_cov_x, double* d_cov_pos,
                              double* d_std_pos, int32_t* h_status, void* d_ws, size_t ws_bytes, void* stream) {
  return acino_skel_fte_covariance_pinned(p, n_clips, camera_model, h_ops, h_active, d_meas, d_w, d_cams, d_lo, d_hi, d_x, d_cov_x,
                                          d_cov_pos, d_std_pos, h_status, d_ws, ws_bytes, stream, 0, nullptr);
}

}  // extern "C"
