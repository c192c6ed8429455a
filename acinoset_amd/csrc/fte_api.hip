// FTE solve: context, Levenberg-Marquardt controller (device-resident) and the C ABI.
// Reference: the Pyomo model + IPOPT solve of src/all_optimizations.py:283-556 in reduced form.
//
// Host layer, one place per decision: Layout / carve (plan, schedule, workspace of a parameter set), reduced_chain (the
// chain `sched` reduces), fresh_state (the LM state of create and load_x), replay (hipGraph capture / replay of the four
// sharded phases and of the single-shard step, one GraphSlot each), drop_graphs (the one invalidation: destroy,
// set_precision, debug_stamps, sep_tail_fall_back), sep_schedule (the cross-rank separator chain's schedule with its
// packed ints), sep_tail_fall_back (acino_fte_solve when k_sep_tail was refused the compute units it counted on).
#include <algorithm>
#include <map>
#include <new>

#include "bcr.hpp"
#include "chunk.hpp"
#include "fte_calib.hpp"
#include "fte_cov.hpp"
#include "fte_reproj.hpp"
#include "seplevel.hpp"

namespace acino {

struct Buffers {
  FteConst* cst;
  acino_fte_state* state;
  double* x[2];       // [(N+6)][25] with 3 halo frames each side
  double* g[2];       // [N][25]
  double* H[2];       // [N][25][25] Gauss-Newton blocks (measurement + smoothness diagonal)
  double* hd[2];      // [N][25] their diagonals, contiguous (the trial kernel would otherwise touch all of H for them)
  double* cost_part;  // [nblk]
  double* pred_part;  // [nblk_t]
  double* step_part;  // [nblk_t]
  double* gn_part;    // [n_nodes]
  double* totals;     // [8]
  int* nbehind;
  int* numeric_err;
  int* sched;         // BcrSchedule::pack()
  double* trunc_eps2; // [n_pairs + 1]
  double* refine_buf; // [3][n_isolated][80] (incomplete reduction with refinement sweeps)
  int* st_flags;      // [n_isolated + n_sep] flags of k_sep_tail (chunked solver with refinement), then the epoch counter
  int n_st_flags;
  unsigned long long* st_ll;   // k_sep_tail's hand-off slots (BcrChain::st_ll)
  size_t n_st_ll;
  double* sep_al;     // chunked solver: [n_sep][80][80] the runs' contributions AL (SepView::AL; BcrChain::AL0 when consumers add it)
};

}  // namespace acino

struct acino_fte_ctx {
  double lam0;
  acino::FteConst h;
  acino::Buffers b;
  acino::BcrChain chain;         // the chain of 3-frame nodes
  acino::BcrSchedule sched;      // reduction schedule of `chain`, or - chunked solver - of the separator chain
  acino::ChunkPlan plan;         // chunked solver (csrc/chunk.hip); inactive: block cyclic reduction over `chain`
  acino::BcrChain sepchain;      // chunked solver: the runs' separators
  acino::SepView sep;
  int n_trunc = 0;               // dropped couplings of an incomplete reduction (of whichever chain `sched` reduces)
  const double* d_det;
  int n_blk_asm, n_blk_trial;
  int n_pred;         // entries of pred_part / step_part: blocks of k_trial, or runs of the chunked back-substitution (which folds it in)
  size_t ws_bytes;
  acino::Profiler prof;
  bool graph_on = false;            // replay fixed launch sequences as hipGraphs (non-null stream, profiler off)
  // captured once per stream and buffer set (key): slots 0..3 the four phases of a SHARDED iteration (between the collectives),
  // STEP_SLOT the whole LM step of a single-shard context; slot i is bit i of acino_fte_graphs_active
  struct GraphSlot {
    hipGraphExec_t exec = nullptr;
    hipStream_t stream = nullptr;
    uintptr_t key[6] = {0, 0, 0, 0, 0, 0};
  } graph[5];
  static constexpr int STEP_SLOT = 4;
};

namespace acino {

static size_t align_up(size_t v, size_t a = 256) { return (v + a - 1) / a * a; }

static int chain_nodes(const acino_fte_params* p) { return (p->n_frames + 2) / 3 + (p->pin_left ? 1 : 0); }

struct Carver {
  char* base;
  size_t off;
  template <class T>
  T* take(size_t count) {
    T* p = reinterpret_cast<T*>(base + off);
    off = align_up(off + count * sizeof(T));
    return p;
  }
};

// (sharded ranks - pinned separators - take the chunked solver too since round 4: the pins join the separator chain)
static bool use_chunks(const acino_fte_params* p) { return p->chunk_nodes >= 0; }

static bool fused_levels_enabled() { return getenv("ACINO_NO_FUSED_LEVELS") == nullptr; }

// Host-side layout of a context: the chunk plan and the reduction schedule (of the separator chain when chunked).
struct Layout {
  ChunkPlan plan;
  BcrSchedule sched;
  void build(const acino_fte_params* p) {
    plan.build(chain_nodes(p), use_chunks(p) ? p->chunk_nodes : -1, p->pin_left != 0, p->pin_right != 0);
    // (separator chains take the fused narrow levels of seplevel.hip; ACINO_NO_FUSED_LEVELS=1: the per-phase kernels of bcr.hip)
    if (plan.active()) sched.build(plan.n_sep, p->pin_left != 0, p->pin_right != 0, p->bcr_levels, p->refine_sweeps,
                                   fused_levels_enabled());
    else sched.build(chain_nodes(p), p->pin_left != 0, p->pin_right != 0, p->bcr_levels, p->refine_sweeps);
    // the one-launch back-substitutions wait for each other's workgroups: kept off GPUs that other spin-waiting kernels may
    // share (shared_gpu: batched clips, several ranks on one device).  k_sep_tail is the separator chain's; whether the device
    // holds all of its workgroups is decided by acino_fte_create.
    sched.backsub_tail = sched.backsub_tail && !p->shared_gpu;
    sched.sep_tail = sched.sep_tail && plan.active() && !p->shared_gpu;
  }
};

static size_t carve(const acino_fte_params* p, char* base, Buffers* out, BcrChain* ch, const Layout& lay, BcrChain* sepch = nullptr) {
  Carver c{base, 0};
  const size_t N = p->n_frames, T = chain_nodes(p);
  const size_t sched_ints = lay.sched.pack().size(), n_pairs = lay.sched.pairs.size() / 2;
  const bool chunked = lay.plan.active();
  Buffers b;
  b.cst = c.take<FteConst>(1);
  b.state = c.take<acino_fte_state>(1);
  for (int k = 0; k < 2; ++k) b.x[k] = c.take<double>((N + 2 * HALO) * NP);
  for (int k = 0; k < 2; ++k) b.g[k] = c.take<double>(N * NP);
  for (int k = 0; k < 2; ++k) b.H[k] = c.take<double>(N * HPAIRS);
  for (int k = 0; k < 2; ++k) b.hd[k] = c.take<double>(N * NP);
  b.cost_part = c.take<double>(n_assemble_blocks((int)N) + 1);
  const size_t n_pred = std::max((N * NP + 255) / 256, (size_t)std::max(lay.plan.n_chunks, 0)) + 1;
  b.pred_part = c.take<double>(n_pred);
  b.step_part = c.take<double>(n_pred);
  b.gn_part = c.take<double>(T + 1);
  b.totals = c.take<double>(8);
  b.nbehind = c.take<int>(4);
  b.numeric_err = b.nbehind + 1;
  b.sched = c.take<int>(sched_ints);
  b.trunc_eps2 = c.take<double>(7 * (n_pairs + 1) + 1);   // (refinement: seven [n_isolated] arrays of sweep norms, bcr_backsub)
  b.refine_buf = nullptr;
  if (lay.sched.refine > 0) b.refine_buf = c.take<double>(3 * (size_t)lay.sched.levels.back().n_elim * BS);
  b.st_flags = nullptr;
  b.n_st_flags = 0;
  b.st_ll = nullptr;
  b.n_st_ll = 0;
  if (lay.sched.sep_tail) {
    b.n_st_flags = lay.sched.levels.back().n_elim + lay.plan.n_sep;
    b.st_flags = c.take<int>((size_t)b.n_st_flags + 2);
    b.n_st_ll = (2 * (size_t)lay.sched.levels.back().n_elim + (size_t)lay.plan.n_sep) * BS * 2;
    b.st_ll = c.take<unsigned long long>(b.n_st_ll);
  }
  BcrChain chn;
  chn.n_nodes = (int)T;
  chn.D = c.take<double>(T * BS * BS);                       // chunked: G_k of the interior nodes (lower tiles)
  chn.U = chunked ? nullptr : c.take<double>(T * BS * BS);
  chn.Cpl = chunked ? nullptr : c.take<double>(T * BS * BS);
  chn.Wl = c.take<double>(chunked ? T * BS : T * BS * BS);   // chunked: f_k = F_k x_L of the interior nodes, [80] each
  chn.Wr = chunked ? nullptr : c.take<double>(T * BS * BS);
  chn.b = c.take<double>(T * BS);
  chn.trunc_eps2 = b.trunc_eps2;
  chn.implicit_couplings = 1;
  chn.dbg = nullptr;
  chn.st = b.state;
  chn.x0 = b.x[0]; chn.x1 = b.x[1];
  chn.g0 = b.g[0]; chn.g1 = b.g[1];
  chn.H0 = b.H[0]; chn.H1 = b.H[1];
  chn.gn_part = b.gn_part;
  BcrChain sc = chn;
  b.sep_al = nullptr;
  if (chunked) {
    const size_t S = lay.plan.n_sep > 0 ? lay.plan.n_sep : 1;
    sc.n_nodes = lay.plan.n_sep;
    sc.D = c.take<double>(S * BS * BS);
    sc.U = c.take<double>(S * BS * BS);
    const bool fz = lay.sched.fused_levels;
    sc.Cpl = c.take<double>((fz ? 2 : 1) * S * BS * BS);     // fused levels: slot S + i = the coupling the elimination of i created
    sc.Wl = c.take<double>(S * BS * BS);
    sc.Wr = c.take<double>(S * BS * BS);
    sc.b = c.take<double>(S * BS);
    if (fz) {
      sc.SL = c.take<double>(S * BS * BS);
      sc.SR = c.take<double>(S * BS * BS);
      sc.Y = c.take<double>(S * BS);
    }
    b.sep_al = c.take<double>(S * BS * BS);
    sc.AL0 = lay.sched.consumers_add_al ? b.sep_al : nullptr;   // (otherwise k_sep_combine folds AL into D / b: chunk_reduce)
    sc.implicit_couplings = 0;      // dense couplings, plain (non-fused) kernels
    sc.st = nullptr;
    sc.x0 = sc.x1 = sc.g0 = sc.g1 = sc.H0 = sc.H1 = nullptr;
    sc.gn_part = nullptr;
  }
  if (out) *out = b;
  if (ch) *ch = chn;
  if (sepch) *sepch = sc;
  return c.off;
}

// ---- kernels ----------------------------------------------------------------------------------
// (the damped system D = H_gn + lam*diag(H_gn), b = -g is built inside the level-0 BCR kernels: bcr.hip build_node)
// Trial iterate x_t = clip(x + delta) and the model quantities of the step.
__global__ void __launch_bounds__(256)
k_trial(const FteConst* __restrict__ cst, const acino_fte_state* __restrict__ st, double* __restrict__ x0,
        double* __restrict__ x1, const double* __restrict__ g0, const double* __restrict__ g1,
        const double* __restrict__ hd0, const double* __restrict__ hd1, const double* __restrict__ delta_nodes,
        double* __restrict__ pred_part, double* __restrict__ step_part) {
  if (st->status != 0) return;
  const FteConst& K = *cst;
  const int cur = st->cur;
  const double* x = cur ? x1 : x0;
  double* xt = cur ? x0 : x1;
  const double* g = cur ? g1 : g0;
  const double* hd = cur ? hd1 : hd0;     // diag of the Gauss-Newton blocks, written by the assembly
  const double lam = st->lam;
  const int tid = threadIdx.x;
  const int64_t e = (int64_t)blockIdx.x * 256 + tid;
  double pred = 0.0, step = 0.0;
  if (e < (int64_t)K.n_frames * NP) {
    const int n = (int)(e / NP), p = (int)(e % NP);
    const int node = n / 3 + K.pin_left, row = (n % 3) * NP + p;
    const double xv = x[(size_t)(n + HALO) * NP + p], gv = g[e];
    const double d0 = hd[e];
    const double gtol = GRAD_ZERO_REL * d0;
    const bool fixed = (xv <= K.lo[p] && gv > gtol) || (xv >= K.hi[p] && gv < -gtol);
    // A bound-active variable is pinned in the linear system by the 2^70 diagonal boost, which leaves it a step of
    // ~1e-21 instead of the exact 0 of a deleted row.  At a bound of 0.0 (theta_7, 9, 11, 13 - where the nose-line
    // initialisation puts them) that residue is representable: x would leave the bound by 1e-21, count as free in the next
    // iteration and take a different path than the active-set rule prescribes.  Its step is 0, exactly.
    const double d = fixed ? 0.0 : delta_nodes[(size_t)node * BS + row];
    const double pg = fixed ? 0.0 : gv;
    const double xn = fmin(fmax(xv + d, K.lo[p]), K.hi[p]);
    xt[(size_t)(n + HALO) * NP + p] = xn;
    if (n >= K.own_lo && n < K.own_hi) {          // (window sharding: only owned frames enter the global sums)
      pred = 0.5 * d * (lam * fmax(d0, DIAG_FLOOR) * d - pg);
      step = fabs(xn - xv);
    }
  }
  __shared__ double rp[4], rs[4];
  for (int off = 32; off > 0; off >>= 1) {
    pred += __shfl_down(pred, off, 64);
    step = fmax(step, __shfl_down(step, off, 64));
  }
  if ((tid & 63) == 0) {
    rp[tid >> 6] = pred;
    rs[tid >> 6] = step;
  }
  __syncthreads();
  if (tid == 0) {
    pred_part[blockIdx.x] = (rp[0] + rp[1]) + (rp[2] + rp[3]);
    step_part[blockIdx.x] = fmax(fmax(rs[0], rs[1]), fmax(rs[2], rs[3]));
  }
}

// totals = {cost, pred, step_inf, gnorm_inf, n_behind, 0, 0, 0}   (fixed summation order)
struct LmTol {
  double gtol, ftol, xtol, lam_max;
  int clamp_lambda;
};
__device__ void lm_control_local(const LmTol& K, acino_fte_state& S, const double* totals, int numeric_err, int init);
__device__ void lm_control(const FteConst& K, acino_fte_state* st, const double* totals, const int* numeric_err,
                           int init);

// fused_control: -1 none (sharded: the decision needs the cross-rank sums), 0 LM step, 1 initial evaluation
__global__ void __launch_bounds__(1024)
k_totals(acino_fte_state* st, const double* cost_part, int n_cost, const double* pred_part,
         const double* step_part, int n_trial, const double* gn_part, int n_nodes, int* nbehind, double* totals,
         int with_step, const FteConst* __restrict__ cst, const int* __restrict__ numeric_err, int fused_control,
         const double* __restrict__ trunc_eps2, int n_trunc) {
  // (the status word is LOADED first and TESTED behind the loads of the partial sums: tested here, every other load of this
  //  single-workgroup kernel would wait a round trip for it)
  const int st_status = st->status;
  int* numeric_err_rw = const_cast<int*>(numeric_err);
  // the four reductions run together: strided per-thread partials, one shuffle tree per wave, the sixteen waves
  // combined in order - a fixed summation order, one barrier.  1024 threads: this single workgroup is a chain of
  // HBM round trips (one per stride), so the stride count is what it costs - 4 instead of 14 for 10 000 frames
  constexpr int NW = 16;
  __shared__ double sh[NW][10];
  // thread 0 will run the controller: its operands are requested now, beside the reductions
  acino_fte_state S;
  LmTol T{0, 0, 0, 0, 0};
  int ne = 0, nb = 0, n_ref = 0;
  double e2 = 0.0, ttol = 0.0, r_d1 = 0.0, r_d0 = 0.0, r_x = 0.0, r_f1 = 0.0, r_f2 = 0.0;
  if (threadIdx.x == 0) {
    S = *st;
    T = LmTol{cst->gtol, cst->ftol, cst->xtol, cst->lam_max, cst->clamp_lambda};
    ne = *numeric_err;
    nb = *nbehind;
    ttol = cst->trunc_tol;
    n_ref = cst->refine_sweeps;
  }
  double c = 0.0, p = 0.0, s = 0.0, g = 0.0;
  // incomplete reduction: plain truncation -> the largest dropped coupling (eps^2) of this step's solve; with refinement
  // sweeps -> max |update| of the last sweep (r_d1) and of the one before (r_d0), max |x| (r_x); strided like the sums
  if (with_step && n_trunc > 0) {
    if (cst->refine_sweeps > 0) {
      const int n_iso = n_trunc + 1;
      for (int i = threadIdx.x; i < n_iso; i += 64 * NW) {
        r_d1 = fmax(r_d1, trunc_eps2[i]);
        r_x = fmax(r_x, trunc_eps2[n_iso + i]);
        r_d0 = fmax(r_d0, trunc_eps2[2 * n_iso + i]);
        r_f1 = fmax(r_f1, trunc_eps2[4 * n_iso + i]);      // (zero where the sweep count leaves them unwritten)
        r_f2 = fmax(r_f2, trunc_eps2[5 * n_iso + i]);
      }
    } else {
      for (int i = threadIdx.x; i < n_trunc; i += 64 * NW) e2 = fmax(e2, trunc_eps2[i]);
    }
  }
  for (int i = threadIdx.x; i < n_cost; i += 64 * NW) c += cost_part[i];
  if (with_step) {
    for (int i = threadIdx.x; i < n_trial; i += 64 * NW) {
      p += pred_part[i];
      s = fmax(s, step_part[i]);
    }
    for (int i = threadIdx.x; i < n_nodes; i += 64 * NW) g = fmax(g, gn_part[i]);
  }
  if (st_status != 0) return;
  for (int off = 32; off > 0; off >>= 1) {
    c += __shfl_down(c, off, 64);
    p += __shfl_down(p, off, 64);
    s = fmax(s, __shfl_down(s, off, 64));
    g = fmax(g, __shfl_down(g, off, 64));
    e2 = fmax(e2, __shfl_down(e2, off, 64));
    r_d1 = fmax(r_d1, __shfl_down(r_d1, off, 64));
    r_d0 = fmax(r_d0, __shfl_down(r_d0, off, 64));
    r_x = fmax(r_x, __shfl_down(r_x, off, 64));
    r_f1 = fmax(r_f1, __shfl_down(r_f1, off, 64));
    r_f2 = fmax(r_f2, __shfl_down(r_f2, off, 64));
  }
  if ((threadIdx.x & 63) == 0) {
    double* w = sh[threadIdx.x >> 6];
    w[0] = c;
    w[1] = p;
    w[2] = s;
    w[3] = g;
    w[4] = e2;
    w[5] = r_d1;
    w[6] = r_d0;
    w[7] = r_x;
    w[8] = r_f1;
    w[9] = r_f2;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    c = 0.0;
    p = 0.0;
    s = 0.0;
    g = 0.0;
    for (int w = 0; w < NW; ++w) {
      c += sh[w][0];
      p += sh[w][1];
      s = fmax(s, sh[w][2]);
      g = fmax(g, sh[w][3]);
      e2 = fmax(e2, sh[w][4]);
      r_d1 = fmax(r_d1, sh[w][5]);
      r_d0 = fmax(r_d0, sh[w][6]);
      r_x = fmax(r_x, sh[w][7]);
      r_f1 = fmax(r_f1, sh[w][8]);
      r_f2 = fmax(r_f2, sh[w][9]);
    }
    double tot[8] = {c, p, s, g, (double)nb, 0.0, 0.0, 0.0};
#pragma unroll
    for (int q = 0; q < 8; ++q) totals[q] = tot[q];
    *nbehind = 0;
    if (with_step && n_trunc > 0) {
      // what the step's relative error is bounded by.  Plain truncation: eps, the measured size of the dropped couplings.
      // With r block-Jacobi sweeps over them (bcr.hip k_bcr_refine): the iteration contracts by rho <= 2 eps per sweep, so
      // the error left after the last sweep is <= rho / (1 - rho) |last update|; rho is measured as a ratio of consecutive
      // updates (one sweep only: rho = 1/2 assumed), and a rho above 1/2 refuses the step.
      double bound;
      if (n_ref > 0) {
        // The contraction is measured where it can be: an update at the rounding level (below 2^-44 of the largest component)
        // is noise, and so is a ratio it takes part in.  The first two sweeps give the clean measurement (the truncated solve
        // is off by ~rho, their updates are ~rho and ~rho^2 of the solution); the last two confirm it as long as they are above
        // the noise - with many sweeps they are not, and their ratio (noise over noise, ~1) must not refuse a converged
        // solve.  Nothing measurable at all (the first update already at rounding): rho = 1/2 assumed, as with one sweep.
        double rho = 0.5;
        const double noise = 0x1p-44 * r_x;
        const double d1 = n_ref == 2 ? r_d0 : r_f1, d2 = n_ref == 2 ? r_d1 : (n_ref == 3 ? r_d0 : r_f2);
        if (n_ref >= 2) {
          const double rho_first = d1 > noise ? d2 / d1 : 0.5;
          const double rho_last = (r_d1 > noise && r_d0 > noise) ? r_d1 / r_d0 : 0.0;
          rho = fmax(rho_first, rho_last);
        }
        bound = (rho <= 0.5 && r_x > 0.0) ? rho / (1.0 - rho) * r_d1 / r_x : (r_d1 == 0.0 ? 0.0 : 1.0);
        if (n_ref >= 2 && rho <= 0.5 && r_x > 0.0 && r_d1 > 0.0) {
          // One ratio of consecutive updates is not the contraction.  Block Jacobi on a chain alternates: the max-norm ratios
          // |u_k+1| / |u_k| of odd and of even k differ (a two-node chain with couplings a, b: the ratios are a, b, a, ... while
          // the rate is sqrt(a b)), and the error left after sweep n starts with u_n+1 = r_n u_n - the ratio of the parity of n,
          // which the first pair of sweeps measures only for odd n.  With two sweeps the bound above was 5 to 7 times below the
          // true error (10 000 and 999 frames at lam = 1e-6: tests/test_gpu_fte_step_reference.py).  What does contract
          // uniformly is a PAIR of sweeps, |u_k+2| <= sigma |u_k|:
          //     |error after sweep n| <= |u_n+1| + |u_n+2| + ... <= sigma / (1 - sigma) (|u_n-1| + |u_n|).
          // sigma from updates an even number of sweeps apart - (u_3, u_1); n >= 4: (u_n, u_2) for even n, (u_n, u_1) for odd n -
          // when both are above the noise; otherwise (and with two sweeps, which have no such pair) from the first ratio and
          // the unmeasured one taken as 1/2, the rate above which a step is refused anyway.
          const int steps = n_ref == 2 ? 0 : (n_ref == 3 ? 2 : ((n_ref & 1) ? n_ref - 1 : n_ref - 2));
          const double den = (n_ref >= 4 && !(n_ref & 1)) ? d2 : d1;
          double sigma = 0.5 * (d1 > noise ? d2 / d1 : 0.5);
          if (steps > 0 && r_d1 > noise && den > noise) sigma = pow(r_d1 / den, 2.0 / (double)steps);
          const double pair = sigma <= 0.25 ? sigma / (1.0 - sigma) * (r_d0 + r_d1) / r_x : 1.0;
          // (two sweeps: u_3 <= u_2 / 2 leads, u_4 = sigma u_2 follows)
          const double two = (0.5 * r_d1 + sigma * r_d1) / (1.0 - sigma) / r_x;
          bound = fmax(bound, n_ref == 2 ? two : pair);
        }
        S.trunc_eps = bound;
      } else {
        S.trunc_eps = sqrt(e2);
        bound = S.trunc_eps;
      }
      if (!(bound <= ttol)) ne |= 4;                 // (also catches NaN)
      if (fused_control < 0) {
        // split-control path (window / separator drivers): k_control reads the DEVICE flag, so the refusal must be there
        st->trunc_eps = S.trunc_eps;
        if (ne & 4) atomicOr(numeric_err_rw, 4);
      }
    }
    // slot 5: this rank's numeric flags (bit 0 pivot, 1 tail timeout, 2 truncation).  Sharded drivers combine it over the
    // ranks (max) with the sums, so every rank's controller takes the same status in the same iteration
    totals[5] = (double)ne;
    tot[5] = (double)ne;
    if (fused_control >= 0) {
      lm_control_local(T, S, tot, ne, fused_control);
      *st = S;
    }
  }
}

// Accept / reject + Nielsen lambda update; mirrors oracle/fte.py:lm_solve step for step.
// The controller on a LOCAL copy of the state (the caller loads the state and the tolerances early and stores the state
// back once: on one thread every access to global memory is a dependent round trip).
__device__ void lm_control_local(const LmTol& K, acino_fte_state& S, const double* totals, int numeric_err, int init) {
  if (S.status != 0) return;
  if (init) {
    S.cost = totals[0];
    S.cost_trial = totals[0];
    S.n_behind = (int)totals[4];
    return;
  }
  const double F = S.cost, Ft = totals[0], pred = totals[1], step = totals[2], gnorm = totals[3];
  S.cost_trial = Ft;
  S.pred = pred;
  S.step_inf = step;
  S.gnorm_inf = gnorm;
  S.iter += 1;
  if (numeric_err) {      // bit 0: non-positive pivot, bit 1: back-substitution tail timed out, bit 2: dropped couplings too large
    S.status = (numeric_err & 1) ? 5 : ((numeric_err & 2) ? 6 : 7);
    return;
  }
  if (gnorm <= K.gtol) {   // the iterate the step started from was already stationary: keep it
    S.status = 3;
    S.last_accept = 0;
    return;
  }
  const double gain = pred > 0.0 ? (F - Ft) / pred : -1.0;
  S.gain = gain;
  if (Ft < F) {
    const double dF = F - Ft;
    S.cur ^= 1;
    S.cost = Ft;
    S.accepted += 1;
    S.last_accept = 1;
    S.n_behind = (int)totals[4];
    const double t = 2.0 * gain - 1.0;
    S.lam = S.lam * fmax(1.0 / 3.0, 1.0 - t * t * t);
    S.nu = 2.0;
    if (dF <= K.ftol * fabs(Ft)) S.status = 1;
    else if (step <= K.xtol) S.status = 2;
  } else {
    S.last_accept = 0;
    S.lam *= S.nu;
    S.nu *= 2.0;
    if (S.lam > K.lam_max) {
      if (K.clamp_lambda) {
        S.lam = K.lam_max;
        S.nu = 2.0;
      } else {
        S.status = 4;
      }
    }
  }
}

__device__ void lm_control(const FteConst& K, acino_fte_state* st, const double* totals, const int* numeric_err,
                           int init) {
  acino_fte_state S = *st;
  const LmTol T{K.gtol, K.ftol, K.xtol, K.lam_max, K.clamp_lambda};
  // the local flag and the flag that travelled with the (combined) sums: a failure on ANY rank stops every rank
  const int flag = *numeric_err | (totals[5] > 0.0 ? (int)totals[5] : 0);
  lm_control_local(T, S, totals, flag, init);
  *st = S;
}

__global__ void k_control(const FteConst* __restrict__ cst, acino_fte_state* st, const double* __restrict__ totals,
                          const int* __restrict__ numeric_err, int init) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  lm_control(*cst, st, totals, numeric_err, init);
}

// Sharded solve: every rank combines the gathered per-rank sums {cost, pred, step_inf, gnorm_inf, n_behind} in rank
// order (identical on all ranks) and takes the accept/reject decision on its own device.
__global__ void k_control_gathered(const FteConst* __restrict__ cst, acino_fte_state* st,
                                   const double* __restrict__ all_partials, int world,
                                   const int* __restrict__ numeric_err, int init) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double tot[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int g = 0; g < world; ++g) {
    const double* p = all_partials + 8 * g;
    tot[0] += p[0];
    tot[1] += p[1];
    tot[2] = fmax(tot[2], p[2]);
    tot[3] = fmax(tot[3], p[3]);
    tot[4] += p[4];
    tot[5] = (double)((int)tot[5] | (p[5] > 0.0 ? (int)p[5] : 0));
  }
  lm_control(*cst, st, tot, numeric_err, init);
}

__global__ void k_copy_x_in(const FteConst* __restrict__ cst, const acino_fte_state* __restrict__ st, int which,
                            const double* __restrict__ src, double* x0, double* x1) {
  const FteConst& K = *cst;
  double* dst = (st->cur ^ which) ? x1 : x0;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e < (int64_t)K.n_frames * NP) {
    const int p = (int)(e % NP);
    dst[e + HALO * NP] = fmin(fmax(src[e], K.lo[p]), K.hi[p]);
  }
}

__global__ void k_set_halo(const acino_fte_state* __restrict__ st, int which, double* x0, double* x1, int n_frames,
                           const double* __restrict__ hl, const double* __restrict__ hr) {
  double* xbuf = (st->cur ^ which) ? x1 : x0;
  const int t = threadIdx.x;
  if (t < HALO * NP) {
    xbuf[t] = hl ? hl[t] : 0.0;
    xbuf[(size_t)(n_frames + HALO) * NP + t] = hr ? hr[t] : 0.0;
  }
}

// dx_n = (x_n - x_{n-1})/Ts, ddx_n = (dx_n - dx_{n-1})/Ts (all_optimizations.py:369-383); the free first
// rows take the values of the optimum: ddx_0 = ddx_1 = ddx_2, dx_0 = dx_1 - Ts ddx_1.
__global__ void k_derivatives(const double* __restrict__ x, int64_t n, double ts, double* __restrict__ dx,
                              double* __restrict__ ddx) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n * NP) return;
  const int64_t f = e / NP;
  const int p = (int)(e % NP);
  auto X = [&](int64_t k) { return x[k * NP + p]; };
  auto DX = [&](int64_t k) { return (X(k) - X(k - 1)) / ts; };          // k >= 1
  auto DDX = [&](int64_t k) { return (DX(k) - DX(k - 1)) / ts; };       // k >= 2
  double v = 0.0, a = 0.0;
  if (n >= 3) {
    a = f >= 2 ? DDX(f) : DDX(2);
    v = f >= 1 ? DX(f) : DX(1) - ts * DDX(2);
  } else if (n == 2) {
    v = DX(1);
  }
  if (dx) dx[e] = v;
  if (ddx) ddx[e] = a;
}

__global__ void k_copy_x_out(const acino_fte_state* __restrict__ st, int which, const double* x0, const double* x1,
                             int64_t n, double* __restrict__ dst) {
  const double* xh = (st->cur ^ which) ? x1 : x0;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e < n * NP) dst[e] = xh[e + HALO * NP];
}

__global__ void k_export_HG(const acino_fte_state* __restrict__ st, const double* g0, const double* g1,
                            const double* H0, const double* H1, int64_t n, double* __restrict__ dg,
                            double* __restrict__ dh) {
  const double* g = st->cur ? g1 : g0;
  const double* H = st->cur ? H1 : H0;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (dg && e < n * NP) dg[e] = g[e];
  if (dh)
    for (int64_t k = e; k < n * NP * NP; k += (int64_t)gridDim.x * 256) {      // (out: the full [25][25] block)
      const int rem = (int)(k % (NP * NP));
      dh[k] = H[(k / (NP * NP)) * HPAIRS + hpair(rem / NP, rem % NP)];
    }
}

__global__ void k_export_edges(const acino_fte_state* __restrict__ st, int which, const double* x0, const double* x1,
                               int n_frames, double* __restrict__ edge) {
  const double* xh = (st->cur ^ which) ? x1 : x0;
  const int t = threadIdx.x;
  if (t < HALO * NP) {
    edge[t] = xh[HALO * NP + t];                                              // first 3 frames
    edge[HALO * NP + t] = xh[(size_t)(n_frames + HALO - 3) * NP + t];         // last 3 frames
  }
}

__global__ void __launch_bounds__(256)
k_copy_frames(const acino_fte_state* __restrict__ st, int which, int import, double* x0, double* x1, int first, int n,
              double* __restrict__ buf) {
  double* xh = ((st->cur ^ which) ? x1 : x0) + (size_t)(first + HALO) * NP;
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e < n * NP) {
    if (import) xh[e] = buf[e];
    else buf[e] = xh[e];
  }
}

__global__ void __launch_bounds__(256)
k_export_sep(BcrChain ch, int node_left, int node_right, double* __restrict__ rec_left, double* __restrict__ rec_right) {
  // rec layout: D[6400] | C[6400] | b[80]
  const size_t MB = (size_t)BS * BS;
  for (int e = threadIdx.x + blockIdx.x * 256; e < (int)MB; e += gridDim.x * 256) {
    if (rec_left) {   // this rank's pinned-left node: Schur update of separator (rank-1), plus coupling to the right separator
      rec_left[e] = ch.D[(size_t)node_left * MB + e];
    }
    if (rec_right) {
      rec_right[e] = ch.D[(size_t)node_right * MB + e];
      if (rec_left) rec_left[MB + e] = ch.Cpl[(size_t)node_left * MB + e];    // block(right sep, left sep)
    }
  }
  if (blockIdx.x == 0 && threadIdx.x < BS) {
    if (rec_left) rec_left[2 * MB + threadIdx.x] = ch.b[(size_t)node_left * BS + threadIdx.x];
    if (rec_right) rec_right[2 * MB + threadIdx.x] = ch.b[(size_t)node_right * BS + threadIdx.x];
  }
}

__global__ void k_import_sep(const double* __restrict__ rec, int n_sep, BcrChain ch) {
  const size_t MB = (size_t)BS * BS;
  const int s = blockIdx.y;
  const double* r = rec + (size_t)s * ACINO_SEP_DOUBLES;
  for (int e = threadIdx.x + blockIdx.x * 256; e < (int)MB; e += gridDim.x * 256) {
    ch.D[(size_t)s * MB + e] = r[e];
    if (s + 1 < n_sep) ch.Cpl[(size_t)s * MB + e] = r[MB + e];   // record s carries block(s+1, s)
  }
  if (blockIdx.x == 0 && threadIdx.x < BS) ch.b[(size_t)s * BS + threadIdx.x] = r[2 * MB + threadIdx.x];
}

__global__ void k_set_node_x(BcrChain ch, int node, const double* __restrict__ xsep) {
  if (threadIdx.x < BS) ch.b[(size_t)node * BS + threadIdx.x] = xsep[threadIdx.x];
}

__global__ void k_copy_vec(const double* __restrict__ src, double* __restrict__ dst, int n) {
  int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) dst[i] = src[i];
}

static int fill_const(const acino_fte_params* p, const double* h_cams, int camera_model, FteConst* c) {
  memset(c, 0, sizeof(*c));
  c->n_frames = p->n_frames;
  c->n_cams = p->n_cams;
  c->n_global = p->n_global;
  c->n_offset = p->n_offset;
  c->clip_len = p->clip_len;
  c->pin_left = p->pin_left ? 1 : 0;
  c->pin_right = p->pin_right ? 1 : 0;
  c->n_nodes = chain_nodes(p);
  c->dlc_thresh = p->dlc_thresh;
  c->inv_r = p->inv_r_meas;
  c->loss = make_loss(p->redesc_a, p->redesc_b, p->redesc_c);
  for (int i = 0; i < NP; ++i) {
    c->q_w[i] = p->q_w[i];
    c->lo[i] = p->lo[i];
    c->hi[i] = p->hi[i];
  }
  c->ftol = p->ftol;
  c->xtol = p->xtol;
  c->gtol = p->gtol;
  c->lam_max = p->lam_max > 0 ? p->lam_max : 1e16;
  c->clamp_lambda = p->clamp_lambda;
  c->precision = p->precision;
  c->trunc_tol = p->trunc_tol > 0.0 ? p->trunc_tol : 1e-10;
  c->refine_sweeps = p->refine_sweeps;
  c->own_lo = p->own_count > 0 ? p->own_first : 0;
  c->own_hi = p->own_count > 0 ? p->own_first + p->own_count : p->n_frames;
  c->camera_model = camera_model;
  if (camera_model == CAMERA_PINHOLE)
    memcpy(c->pcams, h_cams, sizeof(double) * ACINO_PINHOLE_STRIDE * p->n_cams);
  else
    memcpy(c->cams, h_cams, sizeof(double) * ACINO_CAM_STRIDE * p->n_cams);
  return ACINO_OK;
}

static int validate(const acino_fte_params* p) {
  ACINO_REQUIRE(p != nullptr, "params");
  ACINO_REQUIRE(p->n_frames >= 1, "n_frames >= 1");
  ACINO_REQUIRE(p->n_cams >= 1 && p->n_cams <= ACINO_MAX_CAMS, "n_cams in 1..16");
  ACINO_REQUIRE(p->n_global >= p->n_frames && p->n_offset >= 0 && p->n_offset + p->n_frames <= p->n_global,
                "shard range inside the sequence");
  ACINO_REQUIRE(!p->pin_left || (p->n_offset >= 3 && p->n_offset % 3 == 0), "pinned-left shard must start at a multiple of 3");
  ACINO_REQUIRE(p->clip_len >= 0, "clip_len");
  ACINO_REQUIRE(p->precision >= ACINO_PREC_F64 && p->precision <= ACINO_PREC_BF16_RES, "precision");
  ACINO_REQUIRE(p->bcr_levels >= 0 && p->trunc_tol >= 0.0, "bcr_levels, trunc_tol");
  ACINO_REQUIRE(p->chunk_nodes >= -1 && p->chunk_nodes != 1, "chunk_nodes: -1 (off), 0 (automatic) or >= 2");
  ACINO_REQUIRE(p->refine_sweeps >= 0 && p->refine_sweeps <= 64, "refine_sweeps in 0..64");
  ACINO_REQUIRE(p->own_count >= 0 && (p->own_count == 0 || (p->own_first >= 0 && p->own_first + p->own_count <= p->n_frames &&
                                                           !p->pin_left && !p->pin_right && p->clip_len == 0)),
                "own range must lie inside the window (and windows have no pinned separators / clips)");
  ACINO_REQUIRE(p->bcr_levels == 0 || (!p->pin_left && !p->pin_right),
                "incomplete reduction (bcr_levels > 0): single-GPU contexts only");
  ACINO_REQUIRE(p->clip_len == 0 || (!p->pin_left && !p->pin_right && p->n_offset == 0 && p->n_global == p->n_frames &&
                                     p->n_frames % p->clip_len == 0),
                "clips: single-GPU context whose n_frames is a multiple of clip_len");
  ACINO_REQUIRE(!p->pin_right || (p->n_frames % 3 == 0), "pinned-right shard must hold a multiple of 3 frames");
  ACINO_REQUIRE(!(p->pin_left || p->pin_right) || p->n_frames >= 6, "sharded ranks need >= 6 frames");
  ACINO_REQUIRE(p->redesc_c > p->redesc_b && p->redesc_b > p->redesc_a && p->redesc_a > 0, "redescending a<b<c");
  ACINO_REQUIRE(p->lam0 > 0, "lam0 > 0");
  return ACINO_OK;
}

}  // namespace acino

using namespace acino;

// The chain `sched` reduces: a chunked context's separator chain (the pins are its first / last node), else the 3-frame nodes
static BcrChain& reduced_chain(acino_fte_ctx* ctx) { return ctx->plan.active() ? ctx->sepchain : ctx->chain; }

// The LM state of a context that has taken no step: what create and every new start iterate (load_x) upload.
static acino_fte_state fresh_state(double lam0) {
  acino_fte_state st;
  memset(&st, 0, sizeof(st));
  st.lam = lam0;
  st.nu = 2.0;
  return st;
}

// A captured graph bakes in the assembly kernel (precision), sep_tail with its flags and the chains' stamp pointers: whoever
// changes one of them drops every capture, and the next replay() captures again.
static void drop_graphs(acino_fte_ctx* ctx) {
  for (auto& g : ctx->graph)
    if (g.exec) {
      (void)hipGraphExecDestroy(g.exec);
      g.exec = nullptr;
    }
}

static int eval_iterate(acino_fte_ctx* ctx, int which, bool need_jac, bool with_step, bool respect_status,
                        hipStream_t s, int fused_control = -1) {
  const Buffers& b = ctx->b;
  int rc;
  {
    ProfSpan sp(&ctx->prof, PC_ASSEMBLE, s, ctx->h.n_frames);
    rc = launch_assemble(b.cst, ctx->h, b.state, which, ctx->d_det, b.x, b.H, b.g, b.hd, b.cost_part, b.nbehind,
                         need_jac, respect_status, s);
  }
  if (rc) return rc;
  {
    ProfSpan sp(&ctx->prof, PC_TOTALS, s);
    hipLaunchKernelGGL(k_totals, dim3(1), dim3(1024), 0, s, b.state, b.cost_part, ctx->n_blk_asm, b.pred_part,
                       b.step_part, ctx->n_pred, b.gn_part, ctx->plan.active() ? ctx->plan.n_chunks : ctx->chain.n_nodes,   // (chunked: one entry per run)
                       b.nbehind, b.totals,
                       with_step ? 1 : 0, b.cst, b.numeric_err, fused_control, b.trunc_eps2, ctx->n_trunc);
  }
  ACINO_LAUNCH_CHECK();
  return ACINO_OK;
}

extern "C" {

size_t acino_fte_workspace_bytes(const acino_fte_params* p) {
  if (!p || p->n_frames < 1) return 0;
  Layout lay;
  lay.build(p);
  return carve(p, nullptr, nullptr, nullptr, lay) + 256;
}

}  // extern "C"

// acino_fte_create / acino_fte_create_pinhole: d_cams holds n_cams records of the model's stride (24 | 32 doubles)
static int fte_create(acino_fte_ctx** out, const acino_fte_params* p, const double* d_det, const double* d_cams,
                      int camera_model, void* d_workspace, size_t workspace_bytes, void* stream) {
  ACINO_REQUIRE(out != nullptr, "out");
  *out = nullptr;
  int rc = validate(p);
  if (rc) return rc;
  ACINO_REQUIRE(d_det && d_cams && d_workspace, "null buffer");
  if (camera_model == CAMERA_PINHOLE)
    ACINO_REQUIRE(p->precision == ACINO_PREC_F64, "the pinhole camera model is assembled in fp64 only (precision ACINO_PREC_F64)");
  ACINO_REQUIRE(((uintptr_t)d_workspace & 255) == 0, "workspace must be 256-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  acino_fte_ctx* ctx = new (std::nothrow) acino_fte_ctx();
  if (!ctx) {
    set_error("out of host memory");
    return ACINO_ERR_INVALID_ARG;
  }
  ctx->lam0 = p->lam0;
  Layout lay;
  lay.build(p);
  const size_t need = carve(p, (char*)d_workspace, &ctx->b, &ctx->chain, lay, &ctx->sepchain);
  ctx->plan = lay.plan;
  ctx->sched = std::move(lay.sched);
  if (need > workspace_bytes) {
    set_error("workspace too small: need %zu bytes, got %zu", need, workspace_bytes);
    delete ctx;
    return ACINO_ERR_WORKSPACE;
  }
  ctx->ws_bytes = need;
  ctx->d_det = d_det;
  const int stride = camera_model == CAMERA_PINHOLE ? ACINO_PINHOLE_STRIDE : ACINO_CAM_STRIDE;
  double h_cams[ACINO_MAX_CAMS * ACINO_PINHOLE_STRIDE];
  hipError_t e = hipMemcpyAsync(h_cams, d_cams, sizeof(double) * stride * p->n_cams, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) {
    set_error("reading camera records failed: %s", hipGetErrorString(e));
    delete ctx;
    return ACINO_ERR_HIP;
  }
  fill_const(p, h_cams, camera_model, &ctx->h);
  const acino_fte_state st = fresh_state(p->lam0);
  e = hipMemcpyAsync(ctx->b.cst, &ctx->h, sizeof(FteConst), hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(ctx->b.state, &st, sizeof(st), hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemsetAsync(ctx->b.nbehind, 0, 4 * sizeof(int), s);
  if (e == hipSuccess) e = hipMemsetAsync(ctx->b.x[0], 0, sizeof(double) * (p->n_frames + 2 * HALO) * NP, s);
  if (e == hipSuccess) e = hipMemsetAsync(ctx->b.x[1], 0, sizeof(double) * (p->n_frames + 2 * HALO) * NP, s);
  const std::vector<int> sched_ints = ctx->sched.pack();
  if (e == hipSuccess && !sched_ints.empty())
    e = hipMemcpyAsync(ctx->b.sched, sched_ints.data(), sizeof(int) * sched_ints.size(), hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemsetAsync(ctx->b.trunc_eps2, 0, sizeof(double) * (7 * (ctx->sched.pairs.size() / 2 + 1) + 1), s);
  if (e == hipSuccess && ctx->b.st_flags) e = hipMemsetAsync(ctx->b.st_flags, 0, sizeof(int) * ((size_t)ctx->b.n_st_flags + 2), s);
  if (e == hipSuccess && ctx->b.st_ll) e = hipMemsetAsync(ctx->b.st_ll, 0, sizeof(unsigned long long) * ctx->b.n_st_ll, s);
  // (the runs write the contribution AL of every separator that has a run on its right: a right pin has none - zero once)
  if (e == hipSuccess && ctx->plan.active() && ctx->plan.n_sep > 0)
    e = hipMemsetAsync(ctx->b.sep_al, 0, sizeof(double) * (size_t)ctx->plan.n_sep * BS * BS, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);       // (sched_ints is a local)
  if (e != hipSuccess) {
    set_error("context upload failed: %s", hipGetErrorString(e));
    delete ctx;
    return ACINO_ERR_HIP;
  }
  {
    BcrChain& red = reduced_chain(ctx);
    ctx->sched.bind(ctx->b.sched, red);
    ctx->n_trunc = red.n_pairs;
    red.refine_buf = ctx->b.refine_buf;
    red.st_flags = ctx->b.st_flags;
    red.n_st_flags = ctx->b.n_st_flags;
    red.st_ll = ctx->b.st_ll;
  }
  if (ctx->sched.sep_tail) {
    // k_sep_tail only on devices that hold all of its workgroups at once (occupancy x compute units of THIS device: a CU mask,
    // a partitioned GPU); the others take the per-level kernels
    int capacity = 0;
    rc = bcr_set_func_attributes();                // (the occupancy query needs the kernel's LDS attribute in place)
    if (!rc) rc = bcr_sep_tail_capacity(&capacity);
    if (rc) {
      delete ctx;
      return rc;
    }
    // (tests: pretend a smaller device - never a larger one, whose launch would wait for workgroups that are not resident)
    if (const char* v = getenv("ACINO_SEP_TAIL_CAPACITY")) capacity = std::min(capacity, atoi(v));
    ctx->sched.sep_tail = ctx->sched.sep_tail_blocks() <= capacity;
  }
  if (ctx->plan.active()) {
    ctx->sep = SepView{ctx->sepchain.D, ctx->sepchain.Cpl, ctx->b.sep_al, ctx->sepchain.b};
    ctx->sep.flags = ctx->sched.sep_tail ? ctx->b.st_flags : nullptr;
    ctx->sep.n_flags = ctx->sched.sep_tail ? ctx->b.n_st_flags : 0;
  }
  ctx->n_blk_asm = n_assemble_blocks(p->n_frames);
  ctx->n_blk_trial = (int)(((size_t)p->n_frames * NP + 255) / 256);
  ctx->n_pred = ctx->plan.active() ? ctx->plan.n_chunks : ctx->n_blk_trial;
  rc = bcr_set_func_attributes();
  if (!rc) rc = chunk_set_func_attributes();
  if (rc) {
    delete ctx;
    return rc;
  }
  *out = ctx;
  return ACINO_OK;
}

extern "C" {

int acino_fte_create(acino_fte_ctx** out, const acino_fte_params* p, const double* d_det, const double* d_cams24,
                     void* d_workspace, size_t workspace_bytes, void* stream) {
  return fte_create(out, p, d_det, d_cams24, CAMERA_FISHEYE, d_workspace, workspace_bytes, stream);
}

int acino_fte_create_pinhole(acino_fte_ctx** out, const acino_fte_params* p, const double* d_det, const double* d_cams32,
                             void* d_workspace, size_t workspace_bytes, void* stream) {
  return fte_create(out, p, d_det, d_cams32, CAMERA_PINHOLE, d_workspace, workspace_bytes, stream);
}

// The linear solver's layout for these parameters: out[0] = nodes per run (0: block cyclic reduction over the whole chain),
// out[1] = runs, out[2] = separators, out[3] = reduction levels of the chain that is reduced (separators or whole chain)
// when nothing is truncated.
int acino_fte_plan(const acino_fte_params* p, int32_t* out) {
  ACINO_REQUIRE(p && out, "null");
  int rc = validate(p);
  if (rc) return rc;
  acino_fte_params q = *p;
  q.bcr_levels = 0;
  q.refine_sweeps = 0;
  Layout lay;
  lay.build(&q);
  out[0] = lay.plan.m;
  out[1] = lay.plan.n_chunks;
  out[2] = lay.plan.n_sep;
  out[3] = (int32_t)lay.sched.levels.size();
  return ACINO_OK;
}

int acino_fte_destroy(acino_fte_ctx* ctx) {
  if (ctx) drop_graphs(ctx);
  delete ctx;
  return ACINO_OK;
}

int acino_fte_graphs_active(acino_fte_ctx* ctx) {
  int m = 0;
  for (int i = 0; ctx && i < 5; ++i) m |= ctx->graph[i].exec ? (1 << i) : 0;      // (phases 1, 2, 4, 8; the step 16)
  return m;
}

int acino_fte_enable_graph(acino_fte_ctx* ctx, int on) {
  ACINO_REQUIRE(ctx, "null");
  ctx->graph_on = on != 0;
  return ACINO_OK;
}

int acino_fte_load_x(acino_fte_ctx* ctx, const double* d_x0, void* stream) {
  ACINO_REQUIRE(ctx && d_x0, "null");
  hipStream_t s = (hipStream_t)stream;
  const acino_fte_state st = fresh_state(ctx->lam0);
  ACINO_HIP_CHECK(hipMemcpyAsync(ctx->b.state, &st, sizeof(st), hipMemcpyHostToDevice, s));
  ACINO_HIP_CHECK(hipStreamSynchronize(s));   // st lives on this stack frame
  ACINO_HIP_CHECK(hipMemsetAsync(ctx->b.nbehind, 0, 4 * sizeof(int), s));
  hipLaunchKernelGGL(k_copy_x_in, dim3(ctx->n_blk_trial), dim3(256), 0, s, ctx->b.cst, ctx->b.state, 0, d_x0,
                     ctx->b.x[0], ctx->b.x[1]);
  ACINO_LAUNCH_CHECK();
  return ACINO_OK;
}

int acino_fte_set_halo(acino_fte_ctx* ctx, int which, const double* d_halo_l, const double* d_halo_r, void* stream) {
  ACINO_REQUIRE(ctx, "null");
  ACINO_REQUIRE(which == 0 || which == 1, "which");
  hipLaunchKernelGGL(k_set_halo, dim3(1), dim3(128), 0, (hipStream_t)stream, ctx->b.state, which, ctx->b.x[0],
                     ctx->b.x[1], ctx->h.n_frames, d_halo_l, d_halo_r);
  ACINO_LAUNCH_CHECK();
  return ACINO_OK;
}

__global__ void k_restart_status(acino_fte_state* st, double lam0) {
  if (threadIdx.x == 0 && blockIdx.x == 0 && st->status >= 1 && st->status <= 4) {
    if (st->status == 4) st->lam = lam0;      // ended because no damping gave descent: that damping is not a start value
    st->status = 0;
    st->nu = 2.0;
  }
}

int acino_fte_set_precision(acino_fte_ctx* ctx, int precision) {
  ACINO_REQUIRE(ctx, "null");
  ACINO_REQUIRE(precision >= ACINO_PREC_F64 && precision <= ACINO_PREC_BF16_RES, "precision");
  ACINO_REQUIRE(ctx->h.camera_model != CAMERA_PINHOLE || precision == ACINO_PREC_F64,
                "the pinhole camera model is assembled in fp64 only (precision ACINO_PREC_F64)");
  ctx->h.precision = precision;            // the assembly kernel is chosen on the host; the device block does not need it
  drop_graphs(ctx);
  return ACINO_OK;
}

int acino_fte_reevaluate(acino_fte_ctx* ctx, void* stream) {
  ACINO_REQUIRE(ctx, "null");
  ACINO_REQUIRE(!ctx->h.pin_left && !ctx->h.pin_right, "single-GPU contexts");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_restart_status, dim3(1), dim3(64), 0, s, ctx->b.state, ctx->lam0);
  ACINO_LAUNCH_CHECK();
  return eval_iterate(ctx, 0, true, false, false, s, 1);      // assembly of the current iterate + cost (init-style control)
}

int acino_fte_copy_frames(acino_fte_ctx* ctx, int which, int import, int first, int n, double* d_buf, void* stream) {
  ACINO_REQUIRE(ctx && d_buf, "null");
  ACINO_REQUIRE(which == 0 || which == 1, "which");
  ACINO_REQUIRE(n >= 0 && first >= -HALO && first + n <= ctx->h.n_frames + HALO, "frame range");
  if (n == 0) return ACINO_OK;
  hipLaunchKernelGGL(k_copy_frames, dim3((unsigned)((n * NP + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     ctx->b.state, which, import ? 1 : 0, ctx->b.x[0], ctx->b.x[1], first, n, d_buf);
  ACINO_LAUNCH_CHECK();
  return ACINO_OK;
}

int acino_fte_eval(acino_fte_ctx* ctx, int which, void* stream) {
  ACINO_REQUIRE(ctx, "null");
  ACINO_REQUIRE(which == 0 || which == 1, "which");
  return eval_iterate(ctx, which, true, which == 1, which == 1, (hipStream_t)stream);
}

int acino_fte_export_partials(acino_fte_ctx* ctx, double* d_partial, void* stream) {
  ACINO_REQUIRE(ctx && d_partial, "null");
  hipLaunchKernelGGL(k_copy_vec, dim3(1), dim3(256), 0, (hipStream_t)stream, ctx->b.totals, d_partial, 8);
  ACINO_LAUNCH_CHECK();
  return ACINO_OK;
}

int acino_fte_control(acino_fte_ctx* ctx, const double* d_total, int init, void* stream) {
  ACINO_REQUIRE(ctx, "null");
  {
    ProfSpan sp(&ctx->prof, PC_CONTROL, (hipStream_t)stream);
    hipLaunchKernelGGL(k_control, dim3(1), dim3(64), 0, (hipStream_t)stream, ctx->b.cst, ctx->b.state,
                       d_total ? d_total : ctx->b.totals, ctx->b.numeric_err, init);
  }
  ACINO_LAUNCH_CHECK();
  return ACINO_OK;
}

int acino_fte_set_x(acino_fte_ctx* ctx, const double* d_x0, void* stream) {
  int rc = acino_fte_load_x(ctx, d_x0, stream);
  if (rc) return rc;
  return eval_iterate(ctx, 0, true, false, false, (hipStream_t)stream, 1);
}

int acino_fte_reduce_local(acino_fte_ctx* ctx, void* stream) {
  ACINO_REQUIRE(ctx, "null");
  hipStream_t s = (hipStream_t)stream;
  const Buffers& b = ctx->b;
  // the damped system is built inside the level-0 kernels (no separate set-up launch)
  if (ctx->plan.active())
    return chunk_reduce(ctx->chain, ctx->plan, ctx->sep, ctx->sepchain, ctx->sched, b.cst, b.numeric_err, &b.state->status, s,
                        &ctx->prof);
  return bcr_reduce(ctx->chain, ctx->sched, b.cst, b.numeric_err, &b.state->status, s, &ctx->prof);
}

int acino_fte_export_separators(acino_fte_ctx* ctx, double* d_sep, int rank, int world, void* stream) {
  ACINO_REQUIRE(ctx && d_sep, "null");
  ACINO_REQUIRE(world >= 2 && rank >= 0 && rank < world, "rank/world");
  ACINO_REQUIRE((ctx->h.pin_left != 0) == (rank > 0) && (ctx->h.pin_right != 0) == (rank + 1 < world),
                "pins must match the rank position");
  double* rec_left = ctx->h.pin_left ? d_sep + (size_t)(rank - 1) * ACINO_SEP_DOUBLES : nullptr;
  double* rec_right = ctx->h.pin_right ? d_sep + (size_t)rank * ACINO_SEP_DOUBLES : nullptr;
  const BcrChain& pc = reduced_chain(ctx);
  hipLaunchKernelGGL(k_export_sep, dim3(8), dim3(256), 0, (hipStream_t)stream, pc, 0, pc.n_nodes - 1, rec_left, rec_right);
  ACINO_LAUNCH_CHECK();
  return ACINO_OK;
}

namespace acino {
struct SepSchedule {        // of a chain of n_sep cross-rank separators: built and packed once per thread and n_sep
  BcrSchedule sch;
  std::vector<int> ints;    // sch.pack()
};
static const SepSchedule& sep_schedule(int n_sep) {
  static thread_local std::map<int, SepSchedule> cache;   // schedules are immutable once built
  auto it = cache.find(n_sep);
  if (it == cache.end()) {
    SepSchedule ss;
    // (GENERAL 80 x 80 blocks: the fused narrow levels of seplevel.hip need the identity padding of FTE nodes - their right-hand
    //  side rides in the padding column - so this chain keeps the per-phase kernels, and the per-level back-substitution)
    ss.sch.build(n_sep, false, false);
    ss.sch.backsub_tail = false;
    ss.ints = ss.sch.pack();
    it = cache.emplace(n_sep, std::move(ss)).first;
  }
  return it->second;
}
}  // namespace acino

size_t acino_sep_scratch_bytes(int n_sep) {
  if (n_sep < 1) return 0;
  const size_t ints = sep_schedule(n_sep).ints.size();
  return 6 * align_up((size_t)n_sep * BS * BS * sizeof(double)) + align_up(ints * sizeof(int)) + 1024;   // D U Cpl Wl Wr, b
}

namespace acino {
static BcrChain sep_chain(void* d_scratch, int n_sep, const SepSchedule& ss) {
  Carver c{(char*)d_scratch, 0};
  BcrChain ch;
  ch.n_nodes = n_sep;
  ch.D = c.take<double>((size_t)n_sep * BS * BS);
  ch.U = c.take<double>((size_t)n_sep * BS * BS);
  ch.Cpl = c.take<double>((size_t)n_sep * BS * BS);
  ch.Wl = c.take<double>((size_t)n_sep * BS * BS);
  ch.Wr = c.take<double>((size_t)n_sep * BS * BS);
  ch.b = c.take<double>((size_t)n_sep * BS);
  ss.sch.bind(c.take<int>(ss.ints.size()), ch);
  ch.implicit_couplings = 0;
  ch.dbg = nullptr;
  ch.st = nullptr;
  ch.x0 = ch.x1 = ch.g0 = ch.g1 = ch.H0 = ch.H1 = nullptr;
  ch.gn_part = nullptr;
  return ch;
}
// The (static) schedule is written into the caller's scratch by a kernel that carries it as an argument: no
// host-to-device copy, so the write is stream-ordered, capturable and never synchronises (chains of <= 128 separators;
// longer ones fall back to a copy and are not graph-captured).
struct SchedArg {
  static constexpr size_t cap = 960;
  int n;
  int v[cap];
};
__global__ void k_write_schedule(SchedArg a, int* __restrict__ dst) {
  for (int i = threadIdx.x; i < a.n; i += blockDim.x) dst[i] = a.v[i];
}
static bool sep_schedule_fits_arg(const SepSchedule& ss) { return ss.ints.size() <= SchedArg::cap; }
static int sep_upload_schedule(const BcrChain& ch, const SepSchedule& ss, hipStream_t s) {
  int* d_sched = const_cast<int*>(ch.d_elim);
  const std::vector<int>& v = ss.ints;
  if (sep_schedule_fits_arg(ss)) {
    SchedArg a;
    a.n = (int)v.size();
    std::copy(v.begin(), v.end(), a.v);
    hipLaunchKernelGGL(k_write_schedule, dim3(1), dim3(256), 0, s, a, d_sched);
    ACINO_LAUNCH_CHECK();
    return ACINO_OK;
  }
  ACINO_HIP_CHECK(hipMemcpyAsync(d_sched, v.data(), sizeof(int) * v.size(), hipMemcpyHostToDevice, s));
  ACINO_HIP_CHECK(hipStreamSynchronize(s));       // (the copy has left the thread's cache on return; chains this long are not graph-captured)
  return ACINO_OK;
}
static int sep_launch(const BcrChain& ch, const SepSchedule& ss, const double* d_sep, int n_sep, double* d_sep_x,
                      hipStream_t s) {
  const BcrSchedule& sch = ss.sch;
  if (int rc = sep_upload_schedule(ch, ss, s)) return rc;
  hipLaunchKernelGGL(k_import_sep, dim3(8, n_sep), dim3(256), 0, s, d_sep, n_sep, ch);
  ACINO_LAUNCH_CHECK();
  int rc = bcr_reduce(ch, sch, nullptr, nullptr, nullptr, s);
  if (rc) return rc;
  rc = bcr_backsub(ch, sch, nullptr, nullptr, s);
  if (rc) return rc;
  hipLaunchKernelGGL(k_copy_vec, dim3((n_sep * BS + 255) / 256), dim3(256), 0, s, ch.b, d_sep_x, n_sep * BS);
  ACINO_LAUNCH_CHECK();
  return ACINO_OK;
}
}  // namespace acino

int acino_solve_separators(const double* d_sep, int n_sep, double* d_sep_x, void* d_scratch, size_t scratch_bytes,
                           void* stream) {
  ACINO_REQUIRE(d_sep && d_sep_x && d_scratch, "null");
  ACINO_REQUIRE(n_sep >= 1 && n_sep <= 1024, "n_sep");
  ACINO_REQUIRE(scratch_bytes >= acino_sep_scratch_bytes(n_sep), "separator scratch too small");
  ACINO_REQUIRE(((uintptr_t)d_scratch & 255) == 0, "scratch must be 256-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const SepSchedule& ss = sep_schedule(n_sep);
  const BcrChain ch = sep_chain(d_scratch, n_sep, ss);
  if (int rc = bcr_set_func_attributes()) return rc;
  return sep_launch(ch, ss, d_sep, n_sep, d_sep_x, s);
}

int acino_fte_backsub_local(acino_fte_ctx* ctx, const double* d_sep_x, int rank, int world, void* stream) {
  ACINO_REQUIRE(ctx, "null");
  hipStream_t s = (hipStream_t)stream;
  const BcrChain& pc = reduced_chain(ctx);
  if (ctx->h.pin_left) {
    ACINO_REQUIRE(d_sep_x && rank >= 1, "separator solution");
    hipLaunchKernelGGL(k_set_node_x, dim3(1), dim3(128), 0, s, pc, 0, d_sep_x + (size_t)(rank - 1) * BS);
    ACINO_LAUNCH_CHECK();
  }
  if (ctx->h.pin_right) {
    ACINO_REQUIRE(d_sep_x && rank + 1 < world, "separator solution");
    hipLaunchKernelGGL(k_set_node_x, dim3(1), dim3(128), 0, s, pc, pc.n_nodes - 1, d_sep_x + (size_t)rank * BS);
    ACINO_LAUNCH_CHECK();
  }
  if (ctx->plan.active())
    return chunk_backsub(ctx->chain, ctx->plan, ctx->sep, ctx->sepchain, ctx->sched, ctx->b.cst, ctx->b.numeric_err,
                         &ctx->b.state->status, s, &ctx->prof,
                         TrialOut{ctx->b.hd[0], ctx->b.hd[1], ctx->b.pred_part, ctx->b.step_part});
  return bcr_backsub(ctx->chain, ctx->sched, ctx->b.cst, &ctx->b.state->status, s, &ctx->prof, ctx->b.numeric_err);
}

int acino_fte_trial(acino_fte_ctx* ctx, void* stream) {
  ACINO_REQUIRE(ctx, "null");
  if (ctx->plan.active()) return ACINO_OK;      // chunked solver: the back-substitution has formed the trial iterate already
  const Buffers& b = ctx->b;
  {
    ProfSpan sp(&ctx->prof, PC_TRIAL, (hipStream_t)stream, ctx->h.n_frames);
    hipLaunchKernelGGL(k_trial, dim3(ctx->n_blk_trial), dim3(256), 0, (hipStream_t)stream, b.cst, b.state, b.x[0],
                       b.x[1], b.g[0], b.g[1], b.hd[0], b.hd[1], ctx->chain.b, b.pred_part, b.step_part);
  }
  ACINO_LAUNCH_CHECK();
  return ACINO_OK;
}

int acino_fte_export_edges(acino_fte_ctx* ctx, int which, double* d_edge, void* stream) {
  ACINO_REQUIRE(ctx && d_edge, "null");
  ACINO_REQUIRE(ctx->h.n_frames >= 3, "need >= 3 frames");
  hipLaunchKernelGGL(k_export_edges, dim3(1), dim3(128), 0, (hipStream_t)stream, ctx->b.state, which, ctx->b.x[0],
                     ctx->b.x[1], ctx->h.n_frames, d_edge);
  ACINO_LAUNCH_CHECK();
  return ACINO_OK;
}

// ---- captured launch sequences: the four phases of a sharded iteration and the LM step -----------
// Each is a fixed launch sequence (buffer selection and the accept / reject decision live on the device) on the context's
// and on caller-owned buffers - the key; with graphs enabled it is captured once per stream and key and replayed: a rank
// issues 4 graph launches + 3 collectives per iteration instead of ~50 kernel launches, a single-shard step one instead of ~40.
// A capture that fails (another thread of the process touching the runtime, an unsupported call - nothing captured has
// executed): a phase runs eagerly, now and from now on; the step fails the call.  A body that fails in a capture returns its
// own code (a phase: from its eager run); the partial graph is destroyed either way.
enum CaptureFailure { RUN_EAGERLY, FAIL_THE_CALL };

extern "C++" {
template <class F>
static int replay(acino_fte_ctx* ctx, int slot, const uintptr_t (&key)[6], hipStream_t s, CaptureFailure on_failure, F&& body) {
  if (!(ctx->graph_on && !ctx->prof.on && s != nullptr)) return body();
  acino_fte_ctx::GraphSlot& g = ctx->graph[slot];
  if (!g.exec || g.stream != s || memcmp(g.key, key, sizeof(key)) != 0) {
    if (g.exec) (void)hipGraphExecDestroy(g.exec);
    g.exec = nullptr;
    const char* what = "hipStreamBeginCapture";
    hipError_t e = hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal);
    int rc = ACINO_OK;
    if (e == hipSuccess) {
      rc = body();
      hipGraph_t graph = nullptr;
      what = "hipStreamEndCapture";
      e = hipStreamEndCapture(s, &graph);
      if (rc == ACINO_OK && e == hipSuccess) {
        what = "hipGraphInstantiate";
        e = hipGraphInstantiate(&g.exec, graph, nullptr, nullptr, 0);
      }
      if (graph) (void)hipGraphDestroy(graph);
    }
    if (rc != ACINO_OK || e != hipSuccess) {
      g.exec = nullptr;
      if (on_failure == RUN_EAGERLY) {
        (void)hipGetLastError();
        ctx->graph_on = false;
        return body();
      }
      if (rc == ACINO_OK) set_error("%s failed: %s", what, hipGetErrorString(e));
      return rc != ACINO_OK ? rc : ACINO_ERR_HIP;
    }
    g.stream = s;
    memcpy(g.key, key, sizeof(key));
  }
  ACINO_HIP_CHECK(hipGraphLaunch(g.exec, s));
  return ACINO_OK;
}
}  // extern "C++"

int acino_fte_shard_reduce(acino_fte_ctx* ctx, double* d_sep, int rank, int world, void* stream) {
  ACINO_REQUIRE(ctx && d_sep && world >= 2, "args");
  hipStream_t s = (hipStream_t)stream;
  const uintptr_t key[6] = {(uintptr_t)d_sep, (uintptr_t)rank, (uintptr_t)world, 0, 0, 0};
  return replay(ctx, 0, key, s, RUN_EAGERLY, [&]() -> int {
    ACINO_HIP_CHECK(hipMemsetAsync(d_sep, 0, sizeof(double) * (size_t)(world - 1) * ACINO_SEP_DOUBLES, s));
    if (int rc = acino_fte_reduce_local(ctx, stream)) return rc;
    return acino_fte_export_separators(ctx, d_sep, rank, world, stream);
  });
}

int acino_fte_shard_solve(acino_fte_ctx* ctx, const double* d_sep, double* d_sep_x, void* d_scratch, size_t scratch_bytes,
                          double* d_edge_out, int rank, int world, void* stream) {
  ACINO_REQUIRE(ctx && d_sep && d_sep_x && d_scratch && d_edge_out && world >= 2, "args");
  const int n_sep = world - 1;
  ACINO_REQUIRE(scratch_bytes >= acino_sep_scratch_bytes(n_sep), "separator scratch too small");
  ACINO_REQUIRE(((uintptr_t)d_scratch & 255) == 0, "scratch must be 256-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const SepSchedule& ss = sep_schedule(n_sep);
  const BcrChain ch = sep_chain(d_scratch, n_sep, ss);
  const uintptr_t key[6] = {(uintptr_t)d_sep, (uintptr_t)d_sep_x, (uintptr_t)d_scratch, (uintptr_t)d_edge_out,
                            (uintptr_t)rank, (uintptr_t)world};
  auto body = [&]() -> int {
    if (int rc = sep_launch(ch, ss, d_sep, n_sep, d_sep_x, s)) return rc;
    if (int rc = acino_fte_backsub_local(ctx, d_sep_x, rank, world, stream)) return rc;
    if (int rc = acino_fte_trial(ctx, stream)) return rc;
    return acino_fte_export_edges(ctx, 1, d_edge_out, stream);
  };
  if (!sep_schedule_fits_arg(ss)) return body();     // (host copy inside: run eagerly)
  return replay(ctx, 1, key, s, RUN_EAGERLY, body);
}

int acino_fte_shard_eval(acino_fte_ctx* ctx, int which, const double* d_all_edges, int rank, int world,
                         double* d_partial_out, void* stream) {
  ACINO_REQUIRE(ctx && d_all_edges && d_partial_out && world >= 2 && rank >= 0 && rank < world, "args");
  ACINO_REQUIRE(which == 0 || which == 1, "which");
  hipStream_t s = (hipStream_t)stream;
  const double* hl = rank > 0 ? d_all_edges + (size_t)(rank - 1) * 6 * NP + 3 * NP : nullptr;   // left rank's last 3 frames
  const double* hr = rank + 1 < world ? d_all_edges + (size_t)(rank + 1) * 6 * NP : nullptr;     // right rank's first 3
  const uintptr_t key[6] = {(uintptr_t)d_all_edges, (uintptr_t)d_partial_out, (uintptr_t)rank, (uintptr_t)world,
                            (uintptr_t)which, 0};
  return replay(ctx, 2, key, s, RUN_EAGERLY, [&]() -> int {
    if (int rc = acino_fte_set_halo(ctx, which, hl, hr, stream)) return rc;
    if (int rc = acino_fte_eval(ctx, which, stream)) return rc;
    return acino_fte_export_partials(ctx, d_partial_out, stream);
  });
}

int acino_fte_shard_control(acino_fte_ctx* ctx, const double* d_all_partials, int world, int init, void* stream) {
  ACINO_REQUIRE(ctx && d_all_partials && world >= 1, "args");
  hipStream_t s = (hipStream_t)stream;
  const uintptr_t key[6] = {(uintptr_t)d_all_partials, (uintptr_t)world, (uintptr_t)init, 0, 0, 0};
  return replay(ctx, 3, key, s, RUN_EAGERLY, [&]() -> int {
    ProfSpan sp(&ctx->prof, PC_CONTROL, s);
    hipLaunchKernelGGL(k_control_gathered, dim3(1), dim3(64), 0, s, ctx->b.cst, ctx->b.state, d_all_partials, world,
                       ctx->b.numeric_err, init);
    ACINO_LAUNCH_CHECK();
    return ACINO_OK;
  });
}

static int step_eager(acino_fte_ctx* ctx, void* stream) {
  int rc = acino_fte_reduce_local(ctx, stream);
  if (rc) return rc;
  rc = acino_fte_backsub_local(ctx, nullptr, 0, 1, stream);
  if (rc) return rc;
  rc = acino_fte_trial(ctx, stream);
  if (rc) return rc;
  return eval_iterate(ctx, 1, true, true, true, (hipStream_t)stream, 0);   // assembly + sums + accept/reject
}

int acino_fte_step(acino_fte_ctx* ctx, void* stream) {
  ACINO_REQUIRE(ctx, "null");
  ACINO_REQUIRE(!ctx->h.pin_left && !ctx->h.pin_right, "sharded contexts are stepped by the multi-GPU driver");
  const uintptr_t key[6] = {0, 0, 0, 0, 0, 0};       // (the step touches the context's own buffers only)
  return replay(ctx, acino_fte_ctx::STEP_SLOT, key, (hipStream_t)stream, FAIL_THE_CALL,
                [&]() -> int { return step_eager(ctx, stream); });
}

int acino_fte_get_state(acino_fte_ctx* ctx, acino_fte_state* out, void* stream) {
  ACINO_REQUIRE(ctx && out, "null");
  ACINO_HIP_CHECK(hipMemcpyAsync(out, ctx->b.state, sizeof(*out), hipMemcpyDeviceToHost, (hipStream_t)stream));
  ACINO_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
  return ACINO_OK;
}

// The single-launch back-substitution of the separator chain (k_sep_tail: numeric_err bit 3) waited in vain for another
// workgroup (something else holds the compute units it counted on): the refused step changed nothing but the counters -
// fall back to the per-level kernels for the rest of this context's life and go on from the same iterate: sep_tail off,
// its flags cleared, the state (*st: as read back after the refused step) rewound by that step, the captures dropped.
// (The other bounded wait - the d_done tail of bcr.hip - has no such alternative: status 6 is returned.)
static int sep_tail_fall_back(acino_fte_ctx* ctx, acino_fte_state* st, hipStream_t s) {
  ctx->sched.sep_tail = false;
  ctx->sep.flags = nullptr;
  ctx->sep.n_flags = 0;
  drop_graphs(ctx);
  st->status = 0;
  st->iter -= 1;
  ACINO_HIP_CHECK(hipMemcpyAsync(ctx->b.state, st, sizeof(*st), hipMemcpyHostToDevice, s));
  ACINO_HIP_CHECK(hipMemsetAsync(ctx->b.numeric_err, 0, sizeof(int), s));
  ACINO_HIP_CHECK(hipMemsetAsync(ctx->b.st_flags, 0, sizeof(int) * (size_t)ctx->b.n_st_flags, s));
  ACINO_HIP_CHECK(hipStreamSynchronize(s));
  return ACINO_OK;
}

int acino_fte_solve(acino_fte_ctx* ctx, int max_iter, acino_fte_state* out, void* stream) {
  ACINO_REQUIRE(ctx, "null");
  ACINO_REQUIRE(max_iter >= 0, "max_iter");
  acino_fte_state st;
  // (a context continues where its last solve stopped: the device's iteration counter is cumulative.  What the fall-back below
  //  has left of THIS call's budget is counted from the value at entry - only read where the fall-back can happen.)
  int iter_at_entry = 0;
  if (ctx->sched.sep_tail && max_iter > 0) {
    if (int rc = acino_fte_get_state(ctx, &st, stream)) return rc;
    iter_at_entry = st.iter;
  }
  for (int it = 0; it < max_iter; ++it) {
    int rc = acino_fte_step(ctx, stream);
    if (rc) return rc;
    // the device stops by itself; the host peeks now and then to stop launching no-ops - not before a stop is plausible
    // (a synchronisation drains the launch queue: ~50 us of idle GPU each; a no-op step costs about as much)
    if (it >= 11 && ((it - 11) & 3) == 0) {
      rc = acino_fte_get_state(ctx, &st, stream);
      if (rc) return rc;
      if (st.status != 0) break;
    }
  }
  int rc = acino_fte_get_state(ctx, &st, stream);
  if (rc) return rc;
  int ne = 0;
  if (st.status == 6) {
    ACINO_HIP_CHECK(hipMemcpyAsync(&ne, ctx->b.numeric_err, sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream));
    ACINO_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
  }
  if (st.status == 6 && (ne & 8) && ctx->sched.sep_tail && max_iter > 0) {
    rc = sep_tail_fall_back(ctx, &st, (hipStream_t)stream);
    if (rc) return rc;
    const int done = st.iter - iter_at_entry;          // steps of this call that were applied before the refused one
    return acino_fte_solve(ctx, max_iter > done ? max_iter - done : 1, out, stream);
  }
  if (out) *out = st;
  if (st.status == 5) {
    set_error("non-positive pivot in the block factorisation (system not positive definite)");
    return ACINO_ERR_NUMERIC;
  }
  if (st.status == 6) {
    set_error("the fused back-substitution tail timed out waiting for lower workgroups (scheduling order not as assumed); "
              "create the context with shared_gpu = 1 to use the per-level kernels");
    return ACINO_ERR_HIP;
  }
  // (status 7 - dropped couplings of an incomplete reduction above trunc_tol - is returned in the state: the caller
  //  re-creates the context with more levels and continues from the current iterate, acinoset_amd/fte.py does)
  return ACINO_OK;
}

int acino_fte_cost(acino_fte_ctx* ctx, const double* d_x, double* d_cost, void* stream) {
  ACINO_REQUIRE(ctx && d_x && d_cost, "null");
  hipStream_t s = (hipStream_t)stream;
  // evaluated in the TRIAL buffer (clobbers it; call between LM steps)
  hipLaunchKernelGGL(k_copy_x_in, dim3(ctx->n_blk_trial), dim3(256), 0, s, ctx->b.cst, ctx->b.state, 1, d_x,
                     ctx->b.x[0], ctx->b.x[1]);
  ACINO_LAUNCH_CHECK();
  int rc = eval_iterate(ctx, 1, false, false, false, s);
  if (rc) return rc;
  hipLaunchKernelGGL(k_copy_vec, dim3(1), dim3(256), 0, s, ctx->b.totals, d_cost, 1);
  ACINO_LAUNCH_CHECK();
  return ACINO_OK;
}

int acino_fte_get_grad_hess(acino_fte_ctx* ctx, double* d_g, double* d_h, void* stream) {
  ACINO_REQUIRE(ctx, "null");
  const Buffers& b = ctx->b;
  hipLaunchKernelGGL(k_export_HG, dim3(std::max(1, ctx->n_blk_trial)), dim3(256), 0, (hipStream_t)stream, b.state,
                     b.g[0], b.g[1], b.H[0], b.H[1], (int64_t)ctx->h.n_frames, d_g, d_h);
  ACINO_LAUNCH_CHECK();
  return ACINO_OK;
}

// ---- posterior covariance (csrc/fte_cov.hip) ----
static int cov_supported(const FteConst& h, const char* who) {
  const char* why = nullptr;
  if (h.pin_left || h.pin_right || h.n_global != h.n_frames || h.n_offset != 0) why = "a sharded context (one rank's part of a sequence)";
  else if (h.own_lo != 0 || h.own_hi != h.n_frames) why = "a windowed context (own range)";
  else if (h.precision != ACINO_PREC_F64) why = "a context in a bf16 precision (switch to ACINO_PREC_F64 and re-evaluate first)";
  if (why) {
    set_error("%s: not supported for %s; it needs the whole sequence in one fp64 context", who, why);
    return ACINO_ERR_UNSUPPORTED;
  }
  return ACINO_OK;
}

// What the launchers of fte_cov.hip, fte_calib.hip and fte_reproj.hip read of a context
static PostIn post_in(const acino_fte_ctx* ctx) {
  const Buffers& b = ctx->b;
  return PostIn{b.cst, &ctx->h, b.state, ctx->d_det, b.x, b.H, b.g};
}

// The entries with a workspace, after their own ACINO_REQUIREs: the context, then the workspace - the last test before the
// first device call.  post_finish: the error word of the factorisations, the call's one synchronisation.
static int post_begin(const char* who, const acino_fte_ctx* ctx, const void* d_ws, size_t ws_bytes, size_t need) {
  if (int rc = cov_supported(ctx->h, who)) return rc;
  if (ws_bytes < need || ((uintptr_t)d_ws & 255) != 0) {
    set_error("%s: workspace too small or misaligned: need %zu bytes at a 256-byte boundary, got %zu", who, need, ws_bytes);
    return ACINO_ERR_WORKSPACE;
  }
  return ACINO_OK;
}

static int post_finish(const char* who, const void* d_ws, hipStream_t s) {
  int flag = 0;
  ACINO_HIP_CHECK(hipMemcpyAsync(&flag, d_ws, sizeof(int), hipMemcpyDeviceToHost, s));
  ACINO_HIP_CHECK(hipStreamSynchronize(s));
  if (flag) {
    set_error("%s: non-positive pivot (the Gauss-Newton matrix at this iterate is not positive definite)", who);
    return ACINO_ERR_NUMERIC;
  }
  return ACINO_OK;
}

size_t acino_fte_covariance_workspace_bytes(const acino_fte_params* p) {
  if (!p || p->n_frames < 1 || p->clip_len < 0 || (p->clip_len > 0 && p->n_frames % p->clip_len != 0)) return 0;
  return cov_workspace_bytes(p->n_frames, p->clip_len);
}

// Both covariance entries: checks, one run of the sweeps, the error word.
static int cov_run(const char* who, acino_fte_ctx* ctx, double ts, void* d_ws, size_t ws_bytes, double* d_cov_x,
                   double* d_cov_pos, double* d_std_pos, double* d_cov_dx, double* d_cov_ddx, double* d_cov_vel,
                   double* d_std_vel, void* stream) {
  if (int rc = post_begin(who, ctx, d_ws, ws_bytes, cov_workspace_bytes(ctx->h.n_frames, ctx->h.clip_len))) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (int rc = launch_fte_cov_rates(post_in(ctx), d_ws, d_cov_x, d_cov_pos, d_std_pos, d_cov_dx, d_cov_ddx, d_cov_vel, d_std_vel,
                                    ts, s))
    return rc;
  return post_finish(who, d_ws, s);
}

int acino_fte_covariance(acino_fte_ctx* ctx, void* d_ws, size_t ws_bytes, double* d_cov_x, double* d_cov_pos,
                         double* d_std_pos, void* stream) {
  ACINO_REQUIRE(ctx && d_ws, "null");
  ACINO_REQUIRE(d_cov_x || d_cov_pos || d_std_pos, "no output asked for");
  return cov_run("acino_fte_covariance", ctx, 1.0, d_ws, ws_bytes, d_cov_x, d_cov_pos, d_std_pos, nullptr, nullptr, nullptr,
                 nullptr, stream);
}

size_t acino_fte_covariance_rates_workspace_bytes(const acino_fte_params* p) {
  return acino_fte_covariance_workspace_bytes(p);        // (the rates read the sweeps' corrections: nothing more to keep)
}

int acino_fte_covariance_rates(acino_fte_ctx* ctx, double ts, void* d_ws, size_t ws_bytes, double* d_cov_x, double* d_cov_pos,
                               double* d_std_pos, double* d_cov_dx, double* d_cov_ddx, double* d_cov_vel, double* d_std_vel,
                               void* stream) {
  ACINO_REQUIRE(ctx && d_ws, "null");
  ACINO_REQUIRE(d_cov_x || d_cov_pos || d_std_pos || d_cov_dx || d_cov_ddx || d_cov_vel || d_std_vel, "no output asked for");
  ACINO_REQUIRE(ts > 0, "ts");
  return cov_run("acino_fte_covariance_rates", ctx, ts, d_ws, ws_bytes, d_cov_x, d_cov_pos, d_std_pos, d_cov_dx, d_cov_ddx,
                 d_cov_vel, d_std_vel, stream);
}

size_t acino_fte_sample_workspace_bytes(const acino_fte_params* p) {
  return acino_fte_covariance_workspace_bytes(p);        // (U_k^T takes the place of the backward sweep's corrections)
}

int acino_fte_sample(acino_fte_ctx* ctx, int64_t n_samples, const double* d_z, void* d_ws, size_t ws_bytes,
                     double* d_x_samples, double* d_pos_samples, void* stream) {
  const char* who = "acino_fte_sample";
  ACINO_REQUIRE(ctx && d_ws, "null");
  ACINO_REQUIRE(n_samples >= 1, "n_samples");
  ACINO_REQUIRE(d_z && d_x_samples, "null buffer");
  ACINO_REQUIRE((n_samples + 63) / 64 <= 65535, "n_samples (at most 65535 panels of 64)");
  ACINO_REQUIRE(d_z != d_x_samples, "d_z must not alias d_x_samples");
  if (int rc = post_begin(who, ctx, d_ws, ws_bytes, cov_workspace_bytes(ctx->h.n_frames, ctx->h.clip_len))) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (int rc = launch_fte_sample(post_in(ctx), d_ws, n_samples, d_z, d_x_samples, s)) return rc;
  if (d_pos_samples) {
    if (int rc = launch_fk_active(d_x_samples - HALO * NP, n_samples * (int64_t)ctx->h.n_frames, d_pos_samples, s)) return rc;
  }
  return post_finish(who, d_ws, s);
}

// ---- sensitivity to the camera extrinsics (csrc/fte_calib.hip) ----
size_t acino_fte_calibration_workspace_bytes(const acino_fte_params* p) {
  const size_t cov = acino_fte_covariance_workspace_bytes(p);
  if (!cov || p->n_cams < 1 || p->n_cams > ACINO_MAX_CAMS) return 0;
  return calib_workspace_bytes(p->n_frames, p->clip_len, p->n_cams);
}

int acino_fte_calibration_sensitivity(acino_fte_ctx* ctx, const double* d_cov_cams, void* d_ws, size_t ws_bytes,
                                      double* d_sens, double* d_cov_x_cal, double* d_cov_pos_cal, double* d_std_pos_cal,
                                      void* stream) {
  const char* who = "acino_fte_calibration_sensitivity";
  ACINO_REQUIRE(ctx && d_ws, "null");
  ACINO_REQUIRE(d_sens || d_cov_x_cal || d_cov_pos_cal || d_std_pos_cal, "no output asked for");
  ACINO_REQUIRE(d_cov_cams || !(d_cov_x_cal || d_cov_pos_cal || d_std_pos_cal), "a cov / std output needs d_cov_cams");
  const FteConst& h = ctx->h;
  if (int rc = post_begin(who, ctx, d_ws, ws_bytes, calib_workspace_bytes(h.n_frames, h.clip_len, h.n_cams))) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (int rc = launch_fte_calib(post_in(ctx), d_ws, d_cov_cams, d_sens, d_cov_x_cal, d_cov_pos_cal, d_std_pos_cal, s)) return rc;
  return post_finish(who, d_ws, s);
}

// ---- the iterate in image space (csrc/fte_reproj.hip): one launch, no synchronisation, no workspace ----
int acino_fte_reprojection(acino_fte_ctx* ctx, const double* d_cov_pos, double* d_uv, double* d_cov_uv, double* d_res,
                           double* d_weight, double* d_mahal2, uint8_t* d_flags, void* stream) {
  ACINO_REQUIRE(ctx, "null context");
  ACINO_REQUIRE(d_uv || d_cov_uv || d_res || d_weight || d_mahal2 || d_flags, "no output asked for");
  ACINO_REQUIRE(!d_cov_uv || d_cov_pos, "d_cov_uv needs d_cov_pos");
  return launch_fte_reproj(post_in(ctx), d_cov_pos, d_uv, d_cov_uv, d_res, d_weight, d_mahal2, d_flags, (hipStream_t)stream);
}

int acino_fte_get_result(acino_fte_ctx* ctx, double ts, double* d_x, double* d_pos, double* d_dx, double* d_ddx,
                         void* stream) {
  ACINO_REQUIRE(ctx, "null");
  hipStream_t s = (hipStream_t)stream;
  const Buffers& b = ctx->b;
  const int64_t n = ctx->h.n_frames;
  acino_fte_state st;
  int rc = acino_fte_get_state(ctx, &st, stream);
  if (rc) return rc;
  const double* xc = b.x[st.cur];
  if (d_x) {
    hipLaunchKernelGGL(k_copy_x_out, dim3(ctx->n_blk_trial), dim3(256), 0, s, b.state, 0, b.x[0], b.x[1], n, d_x);
    ACINO_LAUNCH_CHECK();
  }
  if (d_pos) {
    rc = launch_fk_active(xc, n, d_pos, s);
    if (rc) return rc;
  }
  if (d_dx || d_ddx) {
    ACINO_REQUIRE(ts > 0, "ts");
    hipLaunchKernelGGL(k_derivatives, dim3(ctx->n_blk_trial), dim3(256), 0, s, xc + HALO * NP, n, ts, d_dx, d_ddx);
    ACINO_LAUNCH_CHECK();
  }
  return ACINO_OK;
}

// Debug: phase timestamps (100 MHz wall clock) go to d_dbg[0..63] of a caller buffer of ACINO_DEBUG_STAMP_ENTRIES (72)
// entries; the selectors are d_dbg[64] = workgroup index and d_dbg[65] = reduction level (k_bcr_elim) / node of the run
// (k_chunk_sweep).  The pointer is a kernel argument: captured graphs are dropped, so that none keeps stamping into a
// buffer the caller has switched off or freed.
int acino_fte_debug_stamps(acino_fte_ctx* ctx, long long* d_dbg) {
  ACINO_REQUIRE(ctx, "null");
  ctx->chain.dbg = d_dbg;
  ctx->sepchain.dbg = d_dbg;       // (k_sep_level, k_sep_tail: selectors in their own comments)
  drop_graphs(ctx);
  return ACINO_OK;
}

// Debug / test aid: copies an internal buffer to d_out (at most n doubles).  what: 0 chain.b (step per node), 1 sep.D,
// 2 sep.b, 3 sep.Cpl, 4 sep.AL, 6 chain.D (G of the interior nodes, lower tiles), 7 chain.Wl (chunked: f_k, [80] per node).
// (5 is not assigned.)
int acino_fte_debug_read(acino_fte_ctx* ctx, int what, double* d_out, int64_t n, void* stream) {
  ACINO_REQUIRE(ctx && d_out && n >= 0, "args");
  const size_t MB = (size_t)BS * BS;
  // (S: the separators - the nodes of the reduced chain of a chunked context, which is `sepchain` then)
  const size_t T = ctx->chain.n_nodes, S = ctx->plan.active() ? (size_t)reduced_chain(ctx).n_nodes : 0;
  const double* src = nullptr;
  size_t cnt = 0;
  switch (what) {
    case 0: src = ctx->chain.b; cnt = T * BS; break;
    case 1: src = ctx->sepchain.D; cnt = S * MB; break;
    case 2: src = ctx->sepchain.b; cnt = S * BS; break;
    case 3: src = ctx->sepchain.Cpl; cnt = S * MB; break;
    case 4: src = ctx->b.sep_al; cnt = S * MB; break;
    case 6: src = ctx->chain.D; cnt = T * MB; break;
    case 7: src = ctx->chain.Wl; cnt = ctx->plan.active() ? T * BS : T * MB; break;
    default: ACINO_REQUIRE(false, "what");
  }
  if ((size_t)n < cnt) cnt = (size_t)n;
  if (cnt == 0 || !src) return ACINO_OK;
  ACINO_HIP_CHECK(hipMemcpyAsync(d_out, src, cnt * sizeof(double), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return ACINO_OK;
}

int acino_fte_profile_begin(acino_fte_ctx* ctx) {
  ACINO_REQUIRE(ctx, "null");
  ctx->prof.on = true;
  ctx->prof.used = 0;
  ctx->prof.spans.clear();
  return ACINO_OK;
}

// Stops profiling, synchronises `stream` and returns per kernel class the summed HIP-event time (ms) and
// the number of launches.  Class order: setup, elim, update, backsub, trial, assemble, totals, control.
int acino_fte_profile_end(acino_fte_ctx* ctx, double* ms_by_class, int* launches_by_class, int64_t* units_by_class,
                          void* stream) {
  ACINO_REQUIRE(ctx && ms_by_class && launches_by_class, "null");
  ctx->prof.on = false;
  ACINO_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
  for (int c = 0; c < PC_COUNT; ++c) {
    ms_by_class[c] = 0.0;
    launches_by_class[c] = 0;
    if (units_by_class) units_by_class[c] = 0;
  }
  for (const Profiler::Span& sp : ctx->prof.spans) {
    float ms = 0.f;
    ACINO_HIP_CHECK(hipEventElapsedTime(&ms, ctx->prof.pool[sp.a], ctx->prof.pool[sp.b]));
    ms_by_class[sp.cls] += ms;
    launches_by_class[sp.cls] += 1;
    if (units_by_class) units_by_class[sp.cls] += sp.units;
  }
  ctx->prof.spans.clear();
  ctx->prof.used = 0;
  return ACINO_OK;
}

int acino_fte_derivatives(const double* d_x, int64_t n_frames, double ts, double* d_dx, double* d_ddx, void* stream) {
  ACINO_REQUIRE(d_x && n_frames >= 0 && ts > 0, "args");
  if (n_frames == 0) return ACINO_OK;
  hipLaunchKernelGGL(k_derivatives, dim3((unsigned)((n_frames * NP + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, d_x, n_frames, ts, d_dx, d_ddx);
  ACINO_LAUNCH_CHECK();
  return ACINO_OK;
}

int acino_fk_active(const double* d_xa, int64_t n_frames, double* d_pos, void* stream) {
  ACINO_REQUIRE(n_frames >= 0, "n_frames");
  if (n_frames == 0) return ACINO_OK;
  ACINO_REQUIRE(d_xa && d_pos, "null buffer");
  // d_xa[N][25] without halo rows: the kernel indexes (frame + halo) * stride with halo = 0
  return launch_fk_active(d_xa - HALO * NP, n_frames, d_pos, (hipStream_t)stream);
}

}  // extern "C"
