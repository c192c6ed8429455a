// Body of the EKF forward kernels k_ekf_forward (fisheye) and k_ekf_forward_pinhole (ekf.hip): the statements of the
// kernel function itself, included inside each kernel's braces with ACINO_EKF_PINHOLE 0 or 1.  The two differ only in the
// camera records held in LDS (Cam, 24 doubles, or Pin, 32) and the projection of the 26 forward-difference variants.  An
// include rather than a shared __device__ function keeps the fisheye kernel's code exactly as it was.
  extern __shared__ __attribute__((aligned(16))) double sm[];
  double* P = sm;                       // [75][76]
  double* Hq = P + PR * PLD;            // [240][27]   later: V [80][28] and Ptop [28][81]
  double* hv = Hq + EROWS * HLD;        // [240] h(x)
  double* rs = hv + EROWS;              // [240] residual
  double* ri = rs + EROWS;              // [240] 1 / R
  double* sd = ri + EROWS;              // [240] diag S
  double* xs = sd + EROWS;              // [80]
  double* gv = xs + 80;                 // [32]
  double* tv = gv + 32;                 // [32]
  double* scr = tv + 32;                // FK frames, then the 25 x 27 work matrices
#if ACINO_EKF_PINHOLE
  Pin* cm = reinterpret_cast<Pin*>(scr + 2800 + 2 * 32 * WLD);
#else
  Cam* cm = reinterpret_cast<Cam*>(scr + 2800 + 2 * 32 * WLD);
#endif
  unsigned* dep = reinterpret_cast<unsigned*>(cm + EKF_MAXC);          // [20]
  int* n_pairs = reinterpret_cast<int*>(dep + NL);
  unsigned short* pairs = reinterpret_cast<unsigned short*>(n_pairs + 4);    // [<= 20 + 25 * 20]
  FkLite* fr = reinterpret_cast<FkLite*>(scr);
  double* Mm = scr;                     // M (25 x 26: column 25 = g)
  double* N1 = Mm + EP * SLD;           // Lc^T [M | g]
  double* Bm = N1 + EP * SLD;           // B -> Lb, then Z = Lb^-1 N1
  double* Am = Bm + EP * SLD;           // A
  double* Lc = scr + 2800;              // chol(Pq) [32][33]; beyond the FK frames (26 x 107 doubles): built early
  double* Ub = Lc + 32 * WLD;           // [32][33] inverse factors: scratch of chol(Pq), then U = Lb^-T
  double* V = Hq;                       // [75][27]
  double* Pt = Hq + PR * VLD;           // [28][81]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
  const int seq = blockIdx.x, N = K.n_frames, C = K.n_cams, rows = C * 2 * NL;
  const double* det = det_all + (size_t)seq * N * C * NL * 3;
  double* x_pred = x_pred_all + (size_t)seq * N * ES;
  double* x_est = x_est_all + (size_t)seq * N * ES;
  double* P_est = P_est_all + (size_t)seq * N * ES * ES;
  const double sT = K.sT, a1 = sT, a2 = sT * sT / 2;

#if ACINO_EKF_PINHOLE
  for (int e = tid; e < C * ACINO_PINHOLE_STRIDE; e += 256) reinterpret_cast<double*>(cm)[e] = cams[e];
#else
  for (int e = tid; e < C * ACINO_CAM_STRIDE; e += 256) reinterpret_cast<double*>(cm)[e] = cams[e];
#endif
  for (int e = tid; e < PR * PLD; e += 256) P[e] = 0.0;
  if (tid < ES) xs[tid] = states0_all[(size_t)seq * ES + tid];
  __syncthreads();
  if (tid < ES) {   // P0 (:713-730)
    const int blk = tid / EP, p = tid % EP;
    double v;
    if (blk == 0) v = p < 3 ? 9.0 : (M_PI / 4) * (M_PI / 4);
    else if (blk == 1) v = p < 3 ? 25.0 : 9.0;
    else v = (p >= 3 + 10) ? 25.0 : 9.0;
    P[tid * PLD + tid] = v;
  }
  int n_out = 0;
  bool bad = false;
  int bad_code = 0;
  __syncthreads();

  // sines / cosines and head positions of the 26 pose variants of ``pose`` (threads tid < nthr, stride nthr)
  auto fill_frames = [&](const double* pose, int nthr) {
    for (int task = tid; task < NVAR * 22; task += nthr) {
      const int v = task / 22, a = task % 22;               // active angle a + 3
      int p = 0;
#pragma unroll
      for (int q = 3; q < EP; ++q) p = (c_ekf2act[q] == a + 3) ? q : p;
      // the reference perturbs its FLOAT32 state array (:628, :640): fl32(x_p) + fl32(eps), a float32 sum, while the
      // difference quotient divides by the float64 eps (:643) - the filter's output carries that ~1e-4 column scaling
      const double ang = (v - 1 == p) ? (double)((float)pose[p] + (float)K.eps) : pose[p];
      double s, c;
      sincos(ang, &s, &c);
      fr[v].sc[a][0] = s;
      fr[v].sc[a][1] = c;
    }
    for (int task = tid; task < NVAR * 3; task += nthr) {
      const int v = task / 3, c = task % 3;
      fr[v].pos[20][c] = (v - 1 == c) ? (double)((float)pose[c] + (float)K.eps) : pose[c];
    }
  };
  // Which marker moves with which parameter is a property of the kinematic chain: probe it once at a generic pose
  // (a marker whose position is bit-identical in the perturbed frame gives a forward difference of exactly 0 at every
  // pose - those projections are skipped and the Jacobian entry is written as 0).  pairs[] = the base variant's 20
  // markers followed by the dependent (variant, marker) pairs; dep[l] = bit mask over the parameters.
  {
    if (tid < EP) hv[tid] = 0.3 + 0.17 * tid;
    __syncthreads();
    fill_frames(hv, 256);
    __syncthreads();
    if (tid < NVAR * 3) fk_columns(fr[tid / 3], tid % 3);
    __syncthreads();
    unsigned char* flag = reinterpret_cast<unsigned char*>(Hq);
    for (int e = tid; e < EP * NL; e += 256) {
      const int v = 1 + e / NL, l = e % NL;
      flag[e] = fr[v].pos[l][0] != fr[0].pos[l][0] || fr[v].pos[l][1] != fr[0].pos[l][1] || fr[v].pos[l][2] != fr[0].pos[l][2];
    }
    __syncthreads();
    if (tid < NL) {
      unsigned m = 0;
      for (int p = 0; p < EP; ++p) m |= flag[p * NL + tid] ? (1u << p) : 0u;
      dep[tid] = m;
      pairs[tid] = (unsigned short)tid;
    }
    if (tid == 0) {
      int n = NL;
      for (int e = 0; e < EP * NL; ++e)
        if (flag[e]) pairs[n++] = (unsigned short)(((1 + e / NL) << 5) | (e % NL));
      *n_pairs = n;
    }
    __syncthreads();
  }
  const int np = *n_pairs;

  for (int f = 0; f < N; ++f) {
    // ---- predict (:622-628; the reference rounds the predicted state to float32) ----
    if (tid < EP) {
      const double acc = xs[2 * EP + tid];
      const double vel = __dadd_rn(xs[EP + tid], __dmul_rn(sT, acc));
      const double pos = __dadd_rn(__dadd_rn(xs[tid], __dmul_rn(sT, vel)), __dmul_rn(__dmul_rn(0.5, __dmul_rn(sT, sT)), acc));
      xs[tid] = (double)(float)pos;
      xs[EP + tid] = (double)(float)vel;
      xs[2 * EP + tid] = (double)(float)acc;
    }
    // P <- F P F^T + Q, block-wise: F = [[I, a1 I, a2 I], [0, I, a1 I], [0, 0, I]]
    for (int e = tid; e < EP * EP; e += 256) predict_cov_entry(P, PLD, P, PLD, e / EP, e % EP, sT);
    __syncthreads();
    if (tid < ES) x_pred[(size_t)f * ES + tid] = xs[tid];

    // ---- measurement model: 26 pose variants (base + eps on each parameter) ----
    // waves 0-2 build the kinematic frames; wave 3 meanwhile factors Pq = Lc Lc^T in its registers
    if (wave < 3) {
      fill_frames(xs, 192);
      for (int e = tid; e < rows * EP; e += 192) Hq[(e / EP) * HLD + e % EP] = 0.0;     // entries of markers that do not move
    } else {
      if (!wave_chol32<false>(P, PLD, Lc, Ub, lane) && !bad) { bad = true; bad_code = 2 * f + 1; }
    }
    __syncthreads();
    if (tid < NVAR * 3) fk_columns(fr[tid / 3], tid % 3);
    __syncthreads();
    for (int task = tid; task < np * C; task += 256) {
      const int pr = pairs[task / C], c = task % C, v = pr >> 5, l = pr & 31;
      double u, w;
#if ACINO_EKF_PINHOLE
      {   // cv2.projectPoints; no cut behind the camera, as the fisheye branch
        const Pin& cp = cm[c];
        const double X = fr[v].pos[l][0], Y = fr[v].pos[l][1], Z = fr[v].pos[l][2];
        const double xc = cp.R[0] * X + cp.R[1] * Y + cp.R[2] * Z + cp.t[0];
        const double yc = cp.R[3] * X + cp.R[4] * Y + cp.R[5] * Z + cp.t[1];
        const double zc = cp.R[6] * X + cp.R[7] * Y + cp.R[8] * Z + cp.t[2];
        double uv[2], Jn[2][3];
        pinhole_project<false>(cp, xc, yc, zc, uv, Jn);
        u = uv[0];
        w = uv[1];
      }
#else
      project_fisheye_pt(cm[c], fr[v].pos[l][0], fr[v].pos[l][1], fr[v].pos[l][2], u, w);
#endif
      const int row = c * 2 * NL + 2 * l;
      if (v == 0) {
        hv[row] = u;
        hv[row + 1] = w;
      } else {
        Hq[row * HLD + v - 1] = u;
        Hq[(row + 1) * HLD + v - 1] = w;
      }
    }
    __syncthreads();
    for (int task = tid; task < (np - NL) * C * 2; task += 256) {
      const int pr = pairs[NL + task / (2 * C)], c = (task >> 1) % C, row = c * 2 * NL + 2 * (pr & 31) + (task & 1);
      double* h = Hq + row * HLD + (pr >> 5) - 1;
      *h = (*h - hv[row]) / K.eps;       // (:643)
    }
    if (tid < rows) {
      const int c = tid / (2 * NL), l = (tid % (2 * NL)) / 2, d = tid & 1;
      const double* dd = det + (((size_t)f * C + c) * NL + l) * 3;
      rs[tid] = dd[d] - hv[tid];
      const double sdv = dd[2] < K.dlc_thresh ? K.max_pixel_err : 25.0;     // (:805-809: the 5**2 is squared again)
      ri[tid] = 1.0 / (sdv * sdv);
    }
    __syncthreads();
    // diag S = Hq Pq Hq^T + R = row norms of Hq Lc, + R: G^T = Lc^T Hq^T on the matrix cores, 16 measurement rows per
    // tile column (lane li = row, the 25 entries of a row spread over 2 tiles x 4 registers x 4 lane groups)
    for (int tr = wave; tr < (rows + 15) / 16; tr += 4) {     // (rows = 40 C: the last tile is half empty for odd C)
      const int row = 16 * tr + li;
      double hq[7], lc0[7], lc1[7];
#pragma unroll
      for (int s7 = 0; s7 < 7; ++s7) {
        const int kk = 4 * s7 + lk;
        hq[s7] = kk < EP ? Hq[row * HLD + kk] : 0.0;
        lc0[s7] = (kk < EP && kk >= li) ? Lc[kk * WLD + li] : 0.0;
        lc1[s7] = (kk < EP && li + 16 < EP && kk >= li + 16) ? Lc[kk * WLD + li + 16] : 0.0;
      }
      d4 g0 = {0, 0, 0, 0}, g1 = {0, 0, 0, 0};
#pragma unroll
      for (int s7 = 0; s7 < 7; ++s7) {
        g0 = __builtin_amdgcn_mfma_f64_16x16x4f64(lc0[s7], hq[s7], g0, 0, 0, 0);
        g1 = __builtin_amdgcn_mfma_f64_16x16x4f64(lc1[s7], hq[s7], g1, 0, 0, 0);
      }
      double ss = 0.0;
#pragma unroll
      for (int r = 0; r < 4; ++r) ss += g0[r] * g0[r] + g1[r] * g1[r];
      ss += __shfl_xor(ss, 16, 64);
      ss += __shfl_xor(ss, 32, 64);
      if (lk == 0 && row < rows) sd[row] = ss + 1.0 / ri[row];
    }
    __syncthreads();
    if (tid < rows / 2) {   // 3-sigma gate per pixel pair (:813-819)
      const int j = 2 * tid;
      if (fabs(rs[j]) > 3.0 * sqrt(sd[j]) || fabs(rs[j + 1]) > 3.0 * sqrt(sd[j + 1])) {
        rs[j] = 0.0;
        rs[j + 1] = 0.0;
        ++n_out;
      }
    }
    __syncthreads();
    // [M | g] = Hq^T R^-1 [Hq | r] on the matrix cores: 32 x 32 padded, one 16 x 16 tile per wave
    {
      const int ti = wave >> 1, tj = wave & 1;
      const int arow = 16 * ti + li, bcol = 16 * tj + li;
      d4 acc = {0, 0, 0, 0};
      const bool a_on = arow < EP, b_h = bcol < EP, b_r = bcol == EP;
      const double* pa = Hq + (a_on ? arow : 0);
      const double* pb = b_h ? Hq + bcol : rs;            // column of Hq, or the residual as the 26th column
      const int sb = b_h ? HLD : 1;
      for (int s = 0; s < rows / 4; s += 5) {             // rows / 4 = 10 C; the operands of five steps in flight
        double av[5], bw[5];
#pragma unroll
        for (int u = 0; u < 5; ++u) {
          const int k0 = 4 * (s + u) + lk;
          av[u] = pa[k0 * HLD];
          bw[u] = ri[k0] * pb[k0 * sb];
        }
#pragma unroll
        for (int u = 0; u < 5; ++u)
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a_on ? av[u] : 0.0, (b_h || b_r) ? bw[u] : 0.0, acc, 0, 0, 0);
      }
      // (the FK frames that share scr were last read by the projections, several barriers ago)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 16 * ti + lk + 4 * r, col = 16 * tj + li;
        if (row < EP && col <= EP) Mm[row * SLD + col] = acc[r];
      }
    }
    __syncthreads();
    // N1 = Lc^T [M | g]
    tile_gemm<7>(2, 2, wave, li, lk,
                 [&](int a_, int k) { return (a_ < EP && k < EP && k >= a_) ? Lc[k * WLD + a_] : 0.0; },
                 [&](int k, int b_) { return (k < EP && b_ <= EP) ? Mm[k * SLD + b_] : 0.0; },
                 [&](int a_, int b_, double v) { if (a_ < EP && b_ <= EP) N1[a_ * SLD + b_] = v; });
    __syncthreads();
    // B = I + N1 Lc
    tile_gemm<7>(2, 2, wave, li, lk,
                 [&](int a_, int k) { return (a_ < EP && k < EP) ? N1[a_ * SLD + k] : 0.0; },
                 [&](int k, int b_) { return (k < EP && b_ < EP && k >= b_) ? Lc[k * WLD + b_] : 0.0; },
                 [&](int a_, int b_, double v) { if (a_ < EP && b_ < EP) Bm[a_ * SLD + b_] = v + (a_ == b_ ? 1.0 : 0.0); });
    __syncthreads();
    // B = Lb Lb^T with U = Lb^-T alongside, in one wave's registers
    // (waves 1-3 meanwhile copy the top rows of P for the covariance update: the Jacobian storage they go to is free)
    if (wave == 0) {
      if (!wave_chol32<true>(Bm, SLD, Lc, Ub, lane) && !bad) { bad = true; bad_code = 2 * f + 2; }   // (Lc is done with)
    } else {
      for (int e = tid - 64; e < 28 * PLD; e += 192) Pt[e] = e < EP * PLD ? P[e] : 0.0;
    }
    __syncthreads();
    // Z = Lb^-1 [N1 | u] = U^T [N1 | u]   (into Bm: Lb itself is not needed again)
    tile_gemm<7>(2, 2, wave, li, lk,
                 [&](int a_, int k) { return (a_ < EP && k <= a_) ? Ub[k * WLD + a_] : 0.0; },
                 [&](int k, int b_) { return (k < EP && b_ <= EP) ? N1[k * SLD + b_] : 0.0; },
                 [&](int a_, int b_, double v) { if (a_ < EP && b_ <= EP) Bm[a_ * SLD + b_] = v; });
    __syncthreads();
    // A = M - Z^T Z ;  w = g - Z^T zu
    tile_gemm<7>(2, 2, wave, li, lk,
                 [&](int a_, int k) { return (a_ < EP && k < EP) ? Bm[k * SLD + a_] : 0.0; },
                 [&](int k, int b_) { return (k < EP && b_ <= EP) ? Bm[k * SLD + b_] : 0.0; },
                 [&](int a_, int b_, double v) {
                   if (a_ < EP && b_ < EP) Am[a_ * SLD + b_] = Mm[a_ * SLD + b_] - v;
                   else if (a_ < EP && b_ == EP) gv[a_] = Mm[a_ * SLD + EP] - v;
                 });
    __syncthreads();
    // state correction x += P[:, :25] w ; V = P[:, :25] A ; Ptop = P[:25, :]
    if (tid < ES) {
      double s = 0.0;
      for (int a = 0; a < EP; ++a) s += P[tid * PLD + a] * gv[a];
      xs[tid] += s;
    }
    tile_gemm<7>(5, 2, wave, li, lk,
                 [&](int r_, int k) { return k < EP ? P[r_ * PLD + k] : 0.0; },
                 [&](int k, int b_) { return (k < EP && b_ < EP) ? Am[k * SLD + b_] : 0.0; },
                 [&](int r_, int b_, double v) { if (b_ < VLD) V[r_ * VLD + b_] = v; });     // zero beyond 75 x 25
    __syncthreads();
    // P -= V Ptop on the matrix cores: 5 x 5 tiles of the 75 x 75 matrix (padded to 80), K = 25 padded to 28
    for (int q0 = 0; q0 < 7; q0 += 2) {      // two tiles' operands in flight per wave
      d4 acc[2];
      double av[2][7], bv[2][7];
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int t = wave + 4 * (q0 + q);
        if (t < 25) {
          const int ti = t / 5, tj = t % 5;
          const int rowA = 16 * ti + li, colB = 16 * tj + li;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int row = 16 * ti + lk + 4 * r;
            acc[q][r] = P[row * PLD + colB];
          }
#pragma unroll
          for (int s7 = 0; s7 < 7; ++s7) {
            const int kk = 4 * s7 + lk;
            av[q][s7] = V[rowA * VLD + kk];
            bv[q][s7] = Pt[kk * PLD + colB];
          }
        }
      }
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int t = wave + 4 * (q0 + q);
        if (t < 25) {
#pragma unroll
          for (int s7 = 0; s7 < 7; ++s7) acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(-av[q][s7], bv[q][s7], acc[q], 0, 0, 0);
          const int ti = t / 5, tj = t % 5, colB = 16 * tj + li;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int row = 16 * ti + lk + 4 * r;
            P[row * PLD + colB] = acc[q][r];
          }
        }
      }
    }
    if (tid < ES) x_est[(size_t)f * ES + tid] = xs[tid];
    __syncthreads();
    // P - V Ptop is symmetric only in exact arithmetic: where the prior collapses the two triangles come out 1e-8 apart
    // (relative to sqrt(P_ii P_jj)).  Both Cholesky factorisations, here and in the smoother, read the lower triangle
    // while the products read whole rows and columns, so the filter would go on with two different matrices.  The lower
    // triangle is the covariance: mirror it, and store that as the smoother's input.
    for (int e = tid; e < ES * ES; e += 256) {
      const int r = e / ES, c = e % ES;
      const double v = r < c ? P[c * PLD + r] : P[r * PLD + c];
      if (r < c) P[r * PLD + c] = v;       // (upper entries are only written, lower ones only read: no order needed)
      P_est[(size_t)f * ES * ES + e] = v;
    }
    __syncthreads();
  }
  // outlier count: one pair per thread per frame
  for (int off = 32; off > 0; off >>= 1) n_out += __shfl_down(n_out, off, 64);
  if (lane == 0 && n_out) atomicAdd(&outliers[seq], n_out);
  if (bad && lane == 0) atomicCAS(numeric_err, 0, bad_code);   // first failure: 2 f + 1 (P) or 2 f + 2 (B)
