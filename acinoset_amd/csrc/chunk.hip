// Chunked substructuring of the block-tridiagonal Gauss-Newton system (the step SURVEY.md section 7.6 describes):
// the chain of 80x80 super-blocks is cut into runs of m consecutive nodes; ONE workgroup eliminates the m - 1 interior
// nodes of a run IN ORDER with every operand resident in LDS, the last node of each run is a separator.  In sequential
// order the couplings between consecutive interior nodes stay the constant third-difference stencils E (<= 3 terms per
// entry, never stored); the only dense fill is the "spike" F_k = block(node k, left separator L):
//
//   node k (D~_k, F_k in LDS; the right-hand side b~_k rides as column 79 of F_k):
//        D~_k = L L^T,  U = L^-T             (blocked Cholesky with the inverse factor, three waves: chol80_trio below)
//        G_k = U U^T  (= D~_k^-1)             -> HBM (lower tiles) for the back-substitution
//        T_k = G_k F_k (= D~_k^-1 F_k; column 79: z_k = D~_k^-1 b~_k -> HBM)
//      left separator:   D_L -= F_k^T T_k    (row 79: its right-hand side)
//      next node:        D~_k+1 = D_k+1 - E^T G_k E    F_k+1 = -E^T T_k (+ b_k+1 in column 79)          (E = E_r(k))
//      (after the last interior node the "next node" is the right separator R: F becomes block(R, L))
//   back-substitution, right to left:  x_k = z_k - G_k (E x_k+1) - T_k x_L,  T_k x_L regenerated from G_k (k_chunk_backsub).
//
// (Until round 4 the spike went through W = U^T F, D_L -= W^T W, T = U W: 180 matrix instructions per 16-column strip and two
//  barriers of the strip waves per node; with G_k formed anyway, T = G F and F^T T cost 152 and none.)
// The separators (one per run, n_chunks - 1) are a block-tridiagonal chain with dense couplings: bcr.hip solves it.
#include "chunk.hpp"

#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include "bcr_dev.hpp"
#include "trio80.hpp"

namespace acino {

void ChunkPlan::build(int nodes_total, int chunk_nodes, bool pin_l, bool pin_r) {
  n_nodes = nodes_total;
  m = n_chunks = n_sep = 0;
  node0 = pin_l ? 1 : 0;
  pin_right = pin_r ? 1 : 0;
  const int nodes = nodes_total - node0;             // the swept part of the chain (a right pin is its last node)
  if (chunk_nodes < 0 || nodes < 1) return;
  int mm = chunk_nodes;
  if (mm == 0) {
    // automatic: one run per CU (256) - one round of workgroups, the fewest separators - for the long chains (measured on
    // config 5's 21 334-node chain: 3.45 ms per iteration with runs of 84 against 3.90 with runs of 16 in 5 rounds), runs of
    // at least 4 nodes for the short ones
    mm = (nodes + 255) / 256;
    mm = std::max(4, std::min(mm, 512));
  }
  mm = std::max(2, mm);
  m = mm;
  n_chunks = (nodes + mm - 1) / mm;
  // a right pin must not be a run of its own (a run builds its right separator from at least one interior node): the last
  // run then takes m + 1 nodes
  if (pin_r && n_chunks > 1 && nodes - (n_chunks - 1) * mm == 1) --n_chunks;
  n_sep = n_chunks - 1 + node0 + pin_right;
}

// ---- tile helpers on LDS matrices (leading dimension LD): one 16x16 output tile per call, all operands read first ----
__device__ __forceinline__ void tile_store(double* M, int ib, int jb, const d4& a, int li, int lk) {
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) M[(ib * 16 + lk + 4 * rr) * LD + jb * 16 + li] = a[rr];
}

// LDS of the sweep kernel: three 80 x 81 matrices (factor workspace | G_k | spike) + tables = 157.9 KB, one workgroup per CU.
//   cL cR | bv x 2 | red | 16 counters | kq klo khi | debug stamps
constexpr int SW_VEC = 18 * NP + 2 * BS + 8 + 8 + 3 * NP + 64;
static constexpr size_t kSweepLds = (3 * MAT + SW_VEC) * sizeof(double);

// The value of x, made opaque to the optimiser: address arithmetic derived from it cannot be hoisted out of the node loop
// (hoisted, the hundreds of per-tile LDS / HBM addresses of this kernel end up spilled to scratch and are reloaded one by
// one in front of the loads that need them).
__device__ __forceinline__ int opaque(int x) {
  asm volatile("" : "+v"(x));
  return x;
}

__device__ __forceinline__ unsigned opaque_u(unsigned x) {
  asm volatile("" : "+v"(x));
  return x;
}
// One state pair of the next-node build, packed by k_chunk_sweep once per run: p | p' << 5 | owned << 10 | diagonal << 11 |
// (p LD + p') << 12 | e << 23 (e < 325 = the pair's index in the assembly's H).
struct BuildSlot {
  int pr, pc, base, e;
  bool own, dg;
  static __device__ __forceinline__ BuildSlot unpack(unsigned w) {
    BuildSlot s;
    s.pr = w & 31;
    s.pc = (w >> 5) & 31;
    s.own = (w >> 10) & 1;
    s.dg = (w >> 11) & 1;
    s.base = (w >> 12) & 2047;
    s.e = w >> 23;
    return s;
  }
};
static_assert((NP - 1) * LD + NP - 1 < 2048 && 13 * NP <= 512 && NP <= 32, "BuildSlot's bit fields");

constexpr int SW_T = 512;
// accumulators of a run's FIRST node start from zero (a select behind the unconditional loads: a conditional load compiles to
// a branch per element with a full wait in front)
template <int NQ>
__device__ __forceinline__ void syrk_mask_n(d4 (&acc)[NQ], bool load) {
#pragma unroll
  for (int q = 0; q < NQ; ++q)
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) acc[q][rr] = load ? acc[q][rr] : 0.0;
}
// ================================================================================================================
// The sweep kernel: TWO TEAMS of waves that run their own loops over the nodes of a run and meet only through LDS counters.
//   D team (waves 0, 4 | 1, 5): the chain  U_k -> G_k = U_k U_k^T -> D~_k+1 = D_k+1 - E^T G_k E -> Cholesky -> U_k+1.
//     Per node: G_k on a fixed schedule of tiles (below), the next node built from the 325 unordered state pairs straight
//     into Xf (one pair per lane, a second one in waves 4 and 5), then chol80_trio - wave 0 the pivot chains, waves 1 and 5 the helpers - while wave 4, the pivot chain's
//     SIMD mate, which therefore carries no matrix work during the chains, streams G_k to HBM.
//   S team (waves 2, 6 | 3, 7): the spike of node k as soon as G_k is complete.  Wave 2 holds strip 1 of the spike (16 columns),
//     wave 6 strips 2 and 0, wave 3 strip 3, wave 7 strip 4.  T strips by spike_gf (the F strip in registers - the accumulator
//     layout of a 16 x 16 tile IS the B-operand layout of the four k-steps over it -, G from Xg), then the tiles of F^T T, every
//     one computed where its T strip lives (spike_node), then T -> Y and the stencil pass in place.
// Who shares a SIMD with whom decides everything here (waves w and w + 4 do): an fp64 matrix instruction holds its SIMD for 64
// cycles, and EVERY instruction of the SIMD mate - vector or matrix - waits for the slot; a wave that streams matrix
// instructions slows a latency-bound mate 2 - 5x (measured: scripts/mfma64_rate.hip, NOTES_perf.md round 5).  So the pivot
// chain shares with a wave that only moves data, the two helpers share with each other (the older one has the deadline), and
// the four strip waves share among themselves.
// Hand-offs (monotonic counters): g_open / g_done: G_k may start / its finished tiles; gfdone (a strip wave is through with
// Xg) S -> D, which then overwrites Xg with G_k+1; c_bv (next node built: its right-hand side bv[(k+1) & 1] is there) D -> S for
// the stencil pass; tdone (a wave's tiles of F^T T are finished: the strips it read may be overwritten) and fready (a wave's
// strips of F_k+1 are complete) among the S waves.  No workgroup barrier inside the node loop: the S team's tail (T -> Y,
// stencil) runs under the D team's G_k+1, the D team's build under the S team's T = G F.
// The ENDS of a run, where half the CU would stand idle, have their own role map:
//   first node (before the loop; the strip waves have no spike yet): chain wave 0, helper L wave 1, helper U WAVE 2 - each
//     helper with the matrix pipe of its own SIMD; wave 5 is helper U from the second node on (TrioSync::sat_out).
//   last node of a run with a left separator (no factorisation follows): once the right separator is built, wave 0 takes
//     strip 3 and wave 1 strip 0 with their whole pipelines (spike_node, roles 10 and 9: F from Y, T = G F, F^T T, T -> Y,
//     stencil, store of their strip of block(R, L)); wave 6 keeps strip 2 alone (role 8), wave 3 computes its tiles of G_k and
//     stores G_k in wave 4's place, waves 5 and 4 store the right separator's diagonal block.  Matrix instructions of
//     the spike per SIMD: 190 | 114 | 285 | 171 (waves 0, 4 | 1, 5 | 2, 6 | 3, 7) instead of 0 | 0 | 399 | 361.  The tiles of AL that
//     change owner (role 6's five, tile {0,0}) are handed over through memory: the old owner waits for its stores and signals
//     c_end, the new owner loads at device scope behind its poll (hand_over, AlTiles::fetch_handed_over).
// (k-step 19 - rows 76 .. 79 of F and of T - is skipped everywhere: those rows are exact zeros)
constexpr int SP_STEPS = 4 * NT - 1;
__device__ __forceinline__ void spike_gf(const double* G, const double (&bF)[NT][4], d4 (&acc)[NT], int li, int lk) {
  double a[3][NT];
  const double* gb = G + lk * LD + li;                 // A(ib, kb)[li][4 s + lk] = G[kb 16 + 4 s + lk][ib 16 + li] (symmetric)
  auto fetch = [&](int buf, int step) {
#pragma unroll
    for (int ib = 0; ib < NT; ++ib) a[buf][ib] = gb[(4 * step) * LD + ib * 16];
  };
#pragma unroll
  for (int ib = 0; ib < NT; ++ib) acc[ib] = d4{0, 0, 0, 0};
  fetch(0, 0);
  fetch(1, 1);
#pragma unroll
  for (int step = 0; step < SP_STEPS; ++step) {
    if (step + 2 < SP_STEPS) fetch((step + 2) % 3, step + 2);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int ib = 0; ib < NT; ++ib) acc[ib] = mfma(a[step % 3][ib], bF[step >> 2][step & 3], acc[ib]);
    __builtin_amdgcn_sched_barrier(0);
  }
}
template <int NQ>
__device__ __forceinline__ void spike_ftt(d4 (&acc)[NQ], const double* Yf, const d4 (&T)[NT], const int (&as)[NQ], int li, int lk) {
  constexpr int DEPTH = NQ >= 3 ? 2 : (NQ == 2 ? 3 : 6);   // operands requested ~6 matrix instructions ahead of their use
  const double* p = Yf + lk * LD + li;
  double a[DEPTH + 1][NQ];
#pragma unroll
  for (int d = 0; d < DEPTH; ++d)
#pragma unroll
    for (int q = 0; q < NQ; ++q) a[d][q] = p[(4 * d) * LD + as[q] * 16];
#pragma unroll
  for (int st = 0; st < SP_STEPS; ++st) {
    if (st + DEPTH < SP_STEPS) {
#pragma unroll
      for (int q = 0; q < NQ; ++q) a[(st + DEPTH) % (DEPTH + 1)][q] = p[(4 * (st + DEPTH)) * LD + as[q] * 16];
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int q = 0; q < NQ; ++q) acc[q] = mfma(-a[st % (DEPTH + 1)][q], T[st >> 2][st & 3], acc[q]);
    __builtin_amdgcn_sched_barrier(0);
  }
}
// NQ tiles (as[q], j) of F^T T against one T strip, accumulated in the lower tiles of AL (a < j: stored transposed).  The
// accumulators are REQUESTED by al_fetch long before they are needed (ahead of the wave's T = G F: an L2 round trip) and
// folded in by al_run.
template <int NQ>
struct AlTiles {
  d4 acc[NQ];
  int as[NQ], j;
  double* Ag;
  __device__ __forceinline__ double* at(int q, int rr, int li, int lk) const {
    return as[q] >= j ? Ag + (size_t)(as[q] * 16 + 4 * rr + lk) * BS + j * 16 + li
                      : Ag + (size_t)(j * 16 + li) * BS + as[q] * 16 + 4 * rr + lk;
  }
  __device__ __forceinline__ void fetch(int li, int lk) {
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) acc[q][rr] = *at(q, rr, li, lk);
  }
  // The tiles of a wave that takes them over from ANOTHER wave of the workgroup for the run's last node (spike_node, roles
  // 9 and 10): the previous owner has waited for its stores of node k - 1 and signalled (hand_over), and these loads are
  // issued behind the poll and at device scope - answered by the L2, which holds those stores, whatever the CU's L1 holds.
  __device__ __forceinline__ void fetch_handed_over(int li, int lk) {
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) acc[q][rr] = __hip_atomic_load(at(q, rr, li, lk), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __device__ __forceinline__ void run(bool load, const double* Yf, const d4 (&T)[NT], int li, int lk) {
    syrk_mask_n<NQ>(acc, load);
    spike_ftt<NQ>(acc, Yf, T, as, li, lk);
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) *at(q, rr, li, lk) = acc[q][rr];
  }
};
// roles of the two-team sweep by wave (waves w and w + 4 share a SIMD): the pivot-chain wave with a wave that carries no matrix work
// during the chains (0, 4), the two factor helpers together (1, 5), the four strip waves on the other two SIMDs (2, 6 | 3, 7) -
// a wave that streams fp64 matrix instructions holds its SIMD 64 cycles at a time, and every instruction of its SIMD mate,
// vector or matrix, waits for the slot: latency-bound work and matrix streams do not share a SIMD
__device__ __forceinline__ int role8(int wave) { return (0x75236410u >> (4 * wave)) & 15; }   // {0, 1, 4, 6, 3, 2, 5, 7}
// G_k = U_k U_k^T on a FIXED SCHEDULE of its 15 lower tiles (tile t costs 4 (5 - tri_i(t)) matrix instructions, 140 in all),
// level per SIMD over the three SIMDs that take part - the D team's two and the one of strip waves 3 and 7, which carries two
// strips only; waves 2 and 6 (three strips: the S team's bottleneck) take none:
//   wave 0 (role 0): t 0, 10 (24)    wave 4 (role 3): t 3, 6, 11 (24)         SIMD of the pivot chain: 48
//   wave 1 (role 1): t 1, 7 (24)     wave 5 (role 2): t 4, 8, 12 (24)         SIMD of the helpers: 48
//   wave 3 (role 6): t 2, 13 (20)    wave 7 (role 7): t 5, 9, 14 (24)         SIMD of strips 3 and 4: 44
// (a run without a left separator has only wave 7 alive in the S team: it takes wave 3's two tiles as well).  Every wave
// requests the operands of its next tile before the matrix instructions of the current one and reports all its tiles with
// one add: g_done counts finished tiles as before, 15 (k + 1) = G_k complete in Xg; g_open (U_k complete, Xg free) stays the
// start signal of the strip waves.  (Until the fixed schedule the tiles were drawn one by one through an LDS ticket: an
// atomic round trip and an exposed operand latency per draw, two uneven rounds of eight takers - 2.6 us for 1.0 us of
// matrix-pipe time.)
constexpr int ctri_i(int t) { return (t >= 1) + (t >= 3) + (t >= 6) + (t >= 10); }
template <int T>
struct GramTile {
  static constexpr int ib = ctri_i(T), jb = T - ib * (ib + 1) / 2, ns = 4 * (NT - ib);
};
template <int T>
__device__ __forceinline__ void gram_fetch(const double* X, int li, int lk, double (&a)[GramTile<T>::ns], double (&b)[GramTile<T>::ns]) {
  const double* pa = X + (GramTile<T>::ib * 16 + li) * LD + GramTile<T>::ib * 16 + lk;      // (U U^T)(ib, jb), jb <= ib: sum_{k >= 16 ib} U[ib16 + i][k] U[jb16 + j][k]
  const double* pb = X + (GramTile<T>::jb * 16 + li) * LD + GramTile<T>::ib * 16 + lk;
#pragma unroll
  for (int s = 0; s < GramTile<T>::ns; ++s) {
    a[s] = pa[4 * s];
    b[s] = pb[4 * s];
  }
}
template <int T>
__device__ __forceinline__ void gram_tile(double* Xg, int li, int lk, const double (&a)[GramTile<T>::ns], const double (&b)[GramTile<T>::ns]) {
  constexpr int ib = GramTile<T>::ib, jb = GramTile<T>::jb;
  d4 g = {0, 0, 0, 0};
#pragma unroll
  for (int s = 0; s < GramTile<T>::ns; ++s) g = mfma(a[s], b[s], g);
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    Xg[(ib * 16 + lk + 4 * rr) * LD + jb * 16 + li] = g[rr];
    if (ib != jb) Xg[(jb * 16 + li) * LD + ib * 16 + lk + 4 * rr] = g[rr];
  }
}
template <int T0, int... REST>
__device__ __forceinline__ void gram_chain(const double* Xf, double* Xg, int li, int lk, const double (&a)[GramTile<T0>::ns],
                                           const double (&b)[GramTile<T0>::ns]) {
  if constexpr (sizeof...(REST) > 0) {
    constexpr int rest[] = {REST...};
    double an[GramTile<rest[0]>::ns], bn[GramTile<rest[0]>::ns];
    gram_fetch<rest[0]>(Xf, li, lk, an, bn);
    __builtin_amdgcn_sched_barrier(0);
    gram_tile<T0>(Xg, li, lk, a, b);
    __builtin_amdgcn_sched_barrier(0);
    gram_chain<REST...>(Xf, Xg, li, lk, an, bn);
  } else {
    gram_tile<T0>(Xg, li, lk, a, b);
  }
}
template <int T0, int... REST>
__device__ __forceinline__ void gram_fixed(const double* Xf, double* Xg, int* done, int li, int lk, int lane) {
  double a[GramTile<T0>::ns], b[GramTile<T0>::ns];
  gram_fetch<T0>(Xf, li, lk, a, b);
  gram_chain<T0, REST...>(Xf, Xg, li, lk, a, b);
  asm volatile("" ::: "memory");
  if (lane == 0) __hip_atomic_fetch_add(done, 1 + (int)sizeof...(REST), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  asm volatile("" ::: "memory");
}

// The spike of one node on one strip wave (ROLE 4: wave 2, strip 1 | 5: wave 6, strips 2 and 0 | 6: wave 3, strip 3 | 7: wave 7,
// strip 4), a function per role so that each gets its own register allocation.  Tiles of F^T T: role 4 {1,1} {0,1} {1,2},
// role 5 {2,2} {0,2} | {0,0}, role 6 {3,3} {0,3} {1,3} {2,3} {3,4}, role 7 {4,4} {0,4} {1,4} {2,4}.
// The LAST node of a run with a left separator (no factorisation follows: the D team's two SIMDs would stand idle from the
// build on) deals one strip of each S SIMD to a D wave, with its whole pipeline:
//   ROLE 8: wave 6, strip 2 alone, tiles {2,2} {0,2}            ROLE 9: wave 1, strip 0, tile {0,0} (role 5's second strip)
//   ROLE 10: wave 0, strip 3 with role 6's five tiles; wave 3 computes its tiles of G_k and stores G_k at that node
// per SIMD 152 + 133 (waves 2, 6), 171 (wave 7), 190 (wave 0), 114 (wave 1) of the 760 matrix instructions, against 399 | 361.
// A moved strip's F is read from Y by a wave that did not write it (it waits for fready of node k - 1), its tiles of AL
// change owner through memory (AlTiles::fetch_handed_over; c_end below), strip 0 is now written by a wave that role 8 - a
// reader, tile {0,2} - does not share: role 8 reports its tiles on c_end.  Every strip of block(R, L) is stored by its owner.
// c_end (used at that node only): 1 + 1 when waves 3 and 6 have handed their tiles over, the third arrival = role 8's tiles.
struct SpikeArgs {
  const double* Xg;
  double* Y;
  double* Ag;
  const double* cRk;
  const double* bvn;
  double* zk;
  double *Cg, *bR;                                   // the run's last node, right separator: block(R, L) (null: no left separator) and
                                                     // its right-hand side in HBM; both null at every other node
  int *c_gfdone, *c_fready, *c_bv, *tdone;           // tdone[0 .. 2]: tile batches finished by roles 4, 6, 7
  int *g_open, *g_done;
  int* c_end;                                        // the last node's hand-overs (above)
  const double* Xf;
  int k, n_s;
  bool hasL, has_next;
  long long* stamps;
};
// G_k -> HBM by one wave, lower tiles only (G is symmetric: the back-substitution mirrors them), 30 items per lane
__device__ __forceinline__ void store_G(const double* Xg, double* Gg, int ln) {
#pragma unroll 6
  for (int q = 0; q < LOWER_ITEMS / 64; ++q) {
    const int idx = ln + 64 * q;
    int r, cc;
    lower_item(idx, r, cc);
    *reinterpret_cast<double2*>(Gg + r * BS + cc) = make_double2(Xg[r * LD + cc], Xg[r * LD + cc + 1]);
  }
}
// A wave gives tiles of AL to another wave of the workgroup: every store it has issued (its tiles of node k - 1) is complete
// before the signal - the one place where the counter protocol does wait for global memory, once per run.
__device__ __forceinline__ void hand_over(int* c_end, int ln) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  lds_signal(c_end, ln);
}
template <int ROLE>
__device__ __forceinline__ void spike_node(const SpikeArgs& A, int& tsb, int ln) {
  constexpr bool two = ROLE == 5;
  constexpr bool moved = ROLE >= 9;                    // a D wave with a strip that another wave held until this node
  constexpr int j0 = ROLE == 4 ? 1 : (ROLE == 5 || ROLE == 8 ? 2 : (ROLE == 6 || ROLE == 10 ? 3 : (ROLE == 7 ? 4 : 0)));
  constexpr int NA = ROLE == 4 ? 3 : (ROLE == 5 || ROLE == 8 ? 2 : (ROLE == 6 || ROLE == 10 ? 5 : (ROLE == 7 ? 4 : 1)));
  // stamps: a role of the last node takes the places of wave 6's (8) and of the factorisation's, which does not run then (9, 10)
  constexpr int sb = ROLE <= 7 ? 16 + 4 * (ROLE - 4) : (ROLE == 8 ? 20 : (ROLE == 9 ? 40 : 44));
  const int li = ln & 15, lk = ln >> 4;
  double* const Y = A.Y;
  auto stamp = [&](int i) { if (A.stamps && ln == 0) A.stamps[i] = (long long)wall_clock64(); };
  AlTiles<NA> al;                                      // tiles against T strip j0
  AlTiles<1> al0;                                      // role 5 only: {0, 0} against T strip 0
  al.Ag = A.Ag;
  al.j = j0;
  if (ROLE == 4) { al.as[0] = 1; al.as[1] = 0; al.as[2 % NA] = 2; }
  if (ROLE == 5 || ROLE == 8) { al.as[0] = 2; al.as[1 % NA] = 0; }
  if (ROLE == 6 || ROLE == 10) { al.as[0] = 3; al.as[1 % NA] = 0; al.as[2 % NA] = 1; al.as[3 % NA] = 2; al.as[4 % NA] = 4; }
  if (ROLE == 7) { al.as[0] = 4; al.as[1] = 0; al.as[2 % NA] = 1; al.as[3 % NA] = 2; }
  if (ROLE == 9) al.as[0] = 0;
  al0.Ag = A.Ag;
  al0.j = 0;
  al0.as[0] = 0;
  if (ROLE == 8) hand_over(A.c_end, ln);               // tile {0, 0} leaves this wave: its store of node k - 1 is complete
  if (moved) {
    lds_wait2(A.c_end, 2, A.c_fready, A.n_s * A.k);    // the tiles handed over; every strip of F_k complete (written by others)
    al.fetch_handed_over(li, lk);
  } else if (A.hasL) {
    al.fetch(li, lk);
    if (two) al0.fetch(li, lk);
  }
  // G_k: this wave's tiles of the fixed schedule once U_k is complete and Xg free (waves 3 and 7), then wait for the last one
  if (ROLE == 6 || ROLE == 7) {
    double* const Xg = const_cast<double*>(A.Xg);
    lds_wait(A.g_open, A.k + 1);
    if (ROLE == 6) gram_fixed<2, 13>(A.Xf, Xg, A.g_done, li, lk, ln);
    else if (A.hasL) gram_fixed<5, 9, 14>(A.Xf, Xg, A.g_done, li, lk, ln);
    else gram_fixed<2, 5, 9, 13, 14>(A.Xf, Xg, A.g_done, li, lk, ln);     // (wave 3 is not alive)
  }
  lds_wait(A.g_done, 15 * (A.k + 1));
  stamp(sb + 0);
  d4 T0[NT], T1[NT];
  {
    double bF[NT][4];
    const double* yb = Y + lk * LD + j0 * 16 + li;
#pragma unroll
    for (int kb = 0; kb < NT; ++kb)
#pragma unroll
      for (int s = 0; s < 4; ++s) bF[kb][s] = (4 * kb + s < SP_STEPS) ? yb[(kb * 16 + 4 * s) * LD] : 0.0;
    spike_gf(A.Xg, bF, T0, li, lk);
  }
  if (two) {
    double bF[NT][4];
    const double* yb = Y + lk * LD + li;               // strip 0
#pragma unroll
    for (int kb = 0; kb < NT; ++kb)
#pragma unroll
      for (int s = 0; s < 4; ++s) bF[kb][s] = (4 * kb + s < SP_STEPS) ? yb[(kb * 16 + 4 * s) * LD] : 0.0;
    spike_gf(A.Xg, bF, T1, li, lk);
  }
  lds_signal(A.c_gfdone, ln);                          // this wave is through with G_k
  stamp(sb + 1);
  if (A.hasL) {
    lds_wait(A.c_fready, A.n_s * A.k);                 // every strip of F_k is complete
    al.run(A.k > 0, Y, T0, li, lk);
    if (two) al0.run(A.k > 0, Y, T1, li, lk);
  }
  stamp(sb + 2);
  // nobody reads this wave's strips of F_k any more: strip 3 is read by its owner only, strip 4 also by role 6 (tile {3,4}),
  // strip 1 by roles 6 and 7, strips 0 and 2 (role 5) by everybody - and role 5 itself reads no strip but its own: nobody waits
  // for the wave with two strips, which finishes its tiles last.  At the last node role 10 stands for role 6 (tdone[1] goes on
  // counting), strip 2 is role 8's and strip 0 role 9's, which also waits for role 8's tile {0,2}: the third arrival on c_end,
  // behind the two hand-overs (a wait that has long been met).
  if (A.hasL) {
    if (ROLE == 4 || ROLE == 6 || ROLE == 7 || ROLE == 10) lds_signal(A.tdone + (ROLE == 4 ? 0 : (ROLE == 7 ? 2 : 1)), ln);
    if (ROLE == 8) {
      lds_wait(A.c_end, 2);
      lds_signal(A.c_end, ln);
    }
    if (ROLE == 7 || ROLE == 4 || ROLE == 5 || ROLE == 8 || ROLE == 9) lds_wait(A.tdone + 1, A.k + 1);
    if (ROLE == 4 || ROLE == 5 || ROLE == 8 || ROLE == 9) lds_wait(A.tdone + 2, A.k + 1);
    if (ROLE == 5 || ROLE == 8 || ROLE == 9) lds_wait(A.tdone + 0, A.k + 1);
    if (ROLE == 9) lds_wait(A.c_end, 3);
  }
  (void)tsb;
  // ---- T_k -> Y (own strips), z_k (column 79 of T) -> HBM, then F_k+1 = -E^T T_k in place, column 79 += the next node's
  //      right-hand side
#pragma unroll
  for (int ib = 0; ib < NT; ++ib) tile_store(Y, ib, j0, T0[ib], li, lk);
  if (two) {
#pragma unroll
    for (int ib = 0; ib < NT; ++ib) tile_store(Y, ib, 0, T1[ib], li, lk);
  }
  if (ROLE == 7) {
    A.zk[ln] = Y[ln * LD + (BS - 1)];
    if (ln < 16) A.zk[64 + ln] = Y[(64 + ln) * LD + (BS - 1)];
  }
  if (A.has_next) {
    lds_wait(A.c_bv, A.k + 1);                         // the next node's right-hand side is there
    const double* const cRk = A.cRk;
    const double* const bvn = A.bvn;
    const int p = ln % NP, cg = ln / NP;               // cg 0, 1 (lanes 50..63 idle)
#pragma unroll
    for (int h = 0; h < (two ? 2 : 1); ++h) {
      const int c_lo = 16 * (h ? 0 : j0);
      if (cg < 2) {
        const double e00 = cRk[(0 * 3 + 0) * NP + p], e01 = cRk[(0 * 3 + 1) * NP + p], e02 = cRk[(0 * 3 + 2) * NP + p];
        const double e11 = cRk[(1 * 3 + 1) * NP + p], e12 = cRk[(1 * 3 + 2) * NP + p], e22 = cRk[(2 * 3 + 2) * NP + p];
        const double b0 = bvn[p], b1 = bvn[NP + p], b2 = bvn[2 * NP + p];
        double fv[8][3];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const int cc = c_lo + cg + 2 * q;
          fv[q][0] = Y[p * LD + cc];
          fv[q][1] = Y[(NP + p) * LD + cc];
          fv[q][2] = Y[(2 * NP + p) * LD + cc];
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const int cc = c_lo + cg + 2 * q;
          const double f0 = fv[q][0], f1 = fv[q][1], f2 = fv[q][2];
          double o0 = -(e00 * f0 + e01 * f1 + e02 * f2), o1 = -(e11 * f1 + e12 * f2), o2 = -(e22 * f2);
          if (cc == BS - 1) {
            o0 += b0;
            o1 += b1;
            o2 += b2;
          }
          Y[p * LD + cc] = o0;
          Y[(NP + p) * LD + cc] = o1;
          Y[(2 * NP + p) * LD + cc] = o2;
        }
      }
      if (ln < 16)
        for (int r = 3 * NP; r < BS; ++r) Y[r * LD + c_lo + ln] = 0.0;     // padding rows couple to nothing
    }
  }
  lds_signal(A.c_fready, ln);
  stamp(sb + 3);
  // After the run's last node F is block(R, L) of the right separator, and this wave's strips of it are final: -> HBM by their
  // owner, now (columns >= 75 are not part of the separator's coupling: zero), the separator's right-hand side (column 79) by
  // strip 4's.  (LDS operations of one wave complete in order: the lanes read what other lanes of the wave have just written.)
  // (No wave holds two strips at that node when there is a left separator - roles 8, 9, 10 above: every strip has an owner
  //  that stores it.)
  if (A.bR) {
    if (A.Cg && !two) {
      const int cc = 16 * j0 + li;
#pragma unroll 5
      for (int r = lk; r < BS; r += 4) A.Cg[r * BS + cc] = cc < 3 * NP ? Y[r * LD + cc] : 0.0;
    }
    if (ROLE == 7) {
      A.bR[ln] = Y[ln * LD + (BS - 1)];
      if (ln < 16) A.bR[64 + ln] = Y[(64 + ln) * LD + (BS - 1)];
    }
  }
}


__global__ void __launch_bounds__(SW_T)
k_chunk_sweep(BcrChain ch, SepView sp, const FteConst* __restrict__ cst, int* numeric_err, const int* __restrict__ status,
                int m, int n_chunks, int node0, int pin_right) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  if (status && *status != 0) return;
  double* const Xf = reinterpret_cast<double*>(smem_raw);   // D~_k -> [L \ U_k] -> D~_k+1
  double* const Xg = Xf + MAT;                               // G_k
  double* const Y = Xg + MAT;                                // spike: F_k -> T_k -> F_k+1; column 79 = right-hand side
  double* const cL = Y + MAT;                          // left table of the first node; afterwards one of the two buffers of right
  double* const cR0 = cL + 9 * NP;                     // tables (tab_cur below); the first node's right table
  double* const bvb = cR0 + 9 * NP;                    // [2][80] right-hand side of the node built last, by node parity
  double* const red = bvb + 2 * BS;                    // [8]
  int* const sync = reinterpret_cast<int*>(red + 8);   // 16 counters, named below ([0] and [11 .. 15]: the factor trio's)
  int* const cB = sync + 5;                            // barrier of the four D waves
  int* const tdone = sync + 2;                         // [3]: tile batches of F^T T finished by roles 4, 6, 7 (sync[2 .. 4])
  int* const g_done = sync + 6;                        // tiles of G finished (15 per node)
  int* const g_open = sync + 10;                       // G_k may start: U_k complete, Xg free
  int* const c_end = sync + 1;                         // the last node's hand-overs between waves (spike_node)
  int* const c_gfdone = sync + 7;
  int* const c_fready = sync + 8;
  int* const c_bv = sync + 9;
  double* const kq = red + 16;                         // [25] each: copies of K.q_w, K.lo, K.hi
  double* const klo = kq + NP;
  double* const khi = klo + NP;
  long long* const lst = reinterpret_cast<long long*>(khi + NP);   // [64] debug stamps, copied out at the end of the kernel
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const FteConst& K = *cst;
  const int c = blockIdx.x;
  const int first = node0 + c * m;
  const bool hasL = c > 0 || node0 > 0, hasR = c + 1 < n_chunks || pin_right;
  const int len = c + 1 < n_chunks ? m : ch.n_nodes - first;       // (the last run: whatever is left, m + 1 at most)
  const int n_int = hasR ? len - 1 : len;
  const int sL = c - 1 + node0, sR = c + node0;                    // separator-chain indices of the run's two ends
  const size_t MB = (size_t)BS * BS;
  const int role = __builtin_amdgcn_readfirstlane(role8(wave));   // 0 chain, 1 / 2 helpers, 3 chain's mate, 4 .. 7 strip waves
  // Coupling tables, per node and exact: a node whose right table is interior (right_table_is_interior: nearly every node of a
  // long sequence) takes the constant table 2 q {-1, 6, -15}; fill_coupling_coef runs only for a node at an end of the sequence, of a
  // clip or of a window.  Two buffers, cR0 and cL (the left table of `first` until the loop starts); tab_cur is the one of the
  // node before, tab_int says which of them hold the constant table - wave-uniform, the same in all eight waves.
  const TableGeom TG = table_geom(K);
  const bool left_int = left_table_is_interior(TG, first);
  int tab_cur = 0;
  bool tab_int0 = right_table_is_interior(TG, first), tab_int1 = left_int;
  const int n_s = hasL ? 4 : 1;              // first run: only the right-hand side column (strip 4, role 7) is alive
  const bool builder = role <= 3;            // the D team
  const bool strips = role >= 4 && (hasL || role == 7);
  double gmax_run = 0.0;
  long long* const dbgp = (ch.dbg && (long long)blockIdx.x == ch.dbg[64] && ch.dbg[66] == 0) ? ch.dbg : nullptr;
  const int dbg_k = dbgp ? (int)ch.dbg[65] : -1;
  if (dbgp && lane == 0) {
    const unsigned hw = __builtin_amdgcn_s_getreg((31 << 11) | 4);
    atomicOr(reinterpret_cast<unsigned long long*>(ch.dbg + 67), (unsigned long long)((hw >> 4) & 3) << (4 * wave));
    if (wave == 0) ch.dbg[68] = hw;
  }
#define SW_STAMP(i) do { if (dbgp && k == dbg_k && lane == 0) lst[i] = (long long)wall_clock64(); } while (0)
  if (tid < 16) sync[tid] = 0;
  if (tid < 64) lst[tid] = 0;
  if (dbgp && tid == 0) dbgp[70] = (long long)wall_clock64();    // (run-level stamps: 70 start, 60 first node built, 61 factored, 62 loop done, 71 end)
  if (c == 0 && node0) {                               // the left pin owns no frames here: its block starts from zero, the
    for (int e = tid; e < BS * BS; e += SW_T) sp.D[e] = 0.0;       // run's spike contribution AL is added by the reduction
    if (tid < BS) sp.b[tid] = 0.0;
  }
  if (tid < NP) {
    kq[tid] = K.q_w[tid];
    klo[tid] = K.lo[tid];
    khi[tid] = K.hi[tid];
  }
  __syncthreads();

  TrioSync tsy;
  {  // ---- first node of the run, its spike F_0 = E_l (dense form) with the right-hand side in column 79
    NodeFetch f;
    build_fetch<SW_T>(f, ch, K, first, tid);
    if (left_int && tab_int0) {                        // both tables in one pass (cR0 follows cL), one entry per thread
      if (tid < 2 * 9 * NP) {
        const int q = tid % (9 * NP), pair = q / NP, p = q % NP, ii = pair / 3, jj = pair % 3;
        cL[tid] = ii <= jj ? 2.0 * kq[p] * (jj == ii ? -1.0 : (jj - ii == 1 ? 6.0 : -15.0)) : 0.0;
      }
    } else {                                           // a node at an end: both evaluated (an interior one comes out as the constants)
      fill_coupling_coef<SW_T>(cL, cR0, K, first, tid, kq);
    }
    for (int e = tid; e < MAT; e += SW_T) Y[e] = 0.0;
    gmax_run = build_finish<SW_T>(Xf, bvb, f, K, first, tid, kq, klo, khi);
    __syncthreads();                                   // node, bv, tables, zeros complete
    if (dbgp && tid == 0) lst[60] = (long long)wall_clock64();
    if (hasL)
      for (int e = tid; e < 9 * NP; e += SW_T) {
        const int pair = e / NP, p = e % NP, ii = pair / 3, jj = pair % 3;
        if (ii <= jj) Y[(ii * NP + p) * LD + jj * NP + p] = cL[e];
      }
    if (tid < BS) Y[tid * LD + (BS - 1)] = bvb[tid];
    __syncthreads();
    // The strip waves have nothing to do before the first node is factored, and their two SIMDs stand idle: helper U's role
    // is wave 2's for this one call, so that helper L (wave 1) has the matrix pipe of its SIMD to itself as in the separator
    // kernels.  Wave 5 takes the role from the next node on (its counters move on as if it had been there); the tiles are the
    // same instructions on the same operands whichever wave issues them.
    if (role < 2 || role == 4) chol80_trio(Xf, role == 4 ? 2 : role, lane, numeric_err, sync, tsy, (dbgp && dbg_k < 0) ? lst : nullptr);
    else if (role == 2) tsy.sat_out(true);
    __syncthreads();
    if (dbgp && tid == 0) lst[61] = (long long)wall_clock64();
  }

  // ---- who builds which of the 325 unordered state pairs {p, p'} of a node (pair e = 13 p + d is p, p' = p + d mod 25: every
  // cyclic distance d = 0 .. 12 once).  Constant over the run, so it is decomposed ONCE, here, and kept packed in one register
  // per slot (BuildSlot below).  Every D wave owns one pair per lane (slot 0), and the 69 pairs left over are a second slot of
  // ONE wave per SIMD - wave 4 (role 3) and wave 5 (role 2, the helper that starts later), never the pivot-chain wave -, so
  // that each of the two D SIMDs issues three wave-slots of the build.  The 25 diagonal pairs (d = 0: damping, bound fixing,
  // right-hand side, the three band coefficients) are lanes 0 .. 24 of wave 1 and of no other wave: one wave executes that
  // divergent block.  The off-diagonal pairs follow in the order of e: number n = 0 .. 299 is e = 13 (n / 12) + 1 + n % 12, slot 0
  // of role 0 holds n = lane, role 2 64 + lane, role 3 128 + lane, role 1 (lanes 25 ..) 192 + lane - 25; slot 1 of role 3
  // n = 231 + lane < 266, of role 2 n = 266 + lane < 300.
  unsigned slot0 = 0, slot1 = 0;
  if (builder) {
    auto pack = [](int e, bool own, bool dg) {
      const int pa = e / 13, dd = e % 13, pc = pa + dd >= NP ? pa + dd - NP : pa + dd;
      return (unsigned)pa | (unsigned)pc << 5 | (unsigned)own << 10 | (unsigned)dg << 11 | (unsigned)(pa * LD + pc) << 12 | (unsigned)e << 23;
    };
    auto offdiag = [](int n) { return 13 * (n / 12) + 1 + n % 12; };
    const bool dg0 = role == 1 && lane < NP;
    const int n0 = role == 1 ? 192 + lane - NP : (role == 0 ? 0 : (role == 2 ? 64 : 128)) + lane;
    slot0 = pack(dg0 ? 13 * lane : offdiag(n0), true, dg0);
    const bool own1 = (role == 3 && lane < 35) || (role == 2 && lane < 34);
    slot1 = pack(own1 ? offdiag((role == 3 ? 231 : 266) + lane) : 0, own1, false);
  }
  int tb = 0, tsb = 0;                       // rounds of the builders' barrier
#pragma unroll 1
  for (int k = 0; k < n_int; ++k) {
    const int node = first + k, next = node + 1;
    const bool last = k + 1 == n_int;
    const bool has_next = !last || hasR;
    const int ln = opaque(lane);
    const int li = ln & 15, lk = ln >> 4;
    // This node's right table: the buffer of the node before if both are the constant table (nothing is written), else the other
    // buffer - the strip waves may still read the previous node's in their stencil pass, and they are through with the one before
    // that (c_gfdone) when the D waves write -, written only if it does not hold the constant table already.
    bool tab_write = false, tab_interior = false;
    if (k > 0) {
      tab_interior = right_table_is_interior(TG, node);
      if (!(tab_interior && (tab_cur ? tab_int1 : tab_int0))) {
        tab_cur ^= 1;
        tab_write = !(tab_interior && (tab_cur ? tab_int1 : tab_int0));
        if (tab_cur) tab_int1 = tab_interior;
        else tab_int0 = tab_interior;
      }
    }
    double* const cRk = tab_cur ? cL : cR0;
    // The last node of a run with a left separator: waves 0 and 1 take a strip of the spike each once the right separator is
    // built (roles 10 and 9 of spike_node), wave 6 keeps strip 2 alone (role 8), wave 3 its tiles of G_k and wave 4's store of G_k.
    const bool spread = last && hasL;
    auto spike_args = [&]() {
      SpikeArgs sa;
      sa.Xg = Xg; sa.Y = Y; sa.Ag = sp.AL + (size_t)(hasL ? opaque(sL) : 0) * MB; sa.cRk = cRk; sa.bvn = bvb + ((k + 1) & 1) * BS;
      sa.zk = ch.b + (size_t)node * BS; sa.g_open = g_open; sa.g_done = g_done; sa.Xf = Xf; sa.c_gfdone = c_gfdone; sa.c_fready = c_fready; sa.c_bv = c_bv; sa.tdone = tdone;
      sa.c_end = c_end;
      sa.bR = (last && hasR) ? sp.b + (size_t)sR * BS : nullptr;
      sa.Cg = (last && hasR && hasL) ? sp.Cpl + (size_t)sL * MB : nullptr;
      sa.k = k; sa.n_s = n_s; sa.hasL = hasL; sa.has_next = has_next; sa.stamps = (dbgp && k == dbg_k) ? lst : nullptr;
      return sa;
    };
    if (builder) {
      // ============================== G_k and the next node: the four D waves ==============================
      const int bw = role;                             // 0 chain, 1, 2 helpers, 3 the chain's SIMD mate (wave 4)
      const int bt = bw * 64 + ln;                     // builder thread
      const int fb_next = 3 * (next - node0);          // (node t holds the local frames 3 (t - pin_left) ..)
      // The next node is symmetric: its 3 x 3 frame blocks are built for the 325 UNORDERED state pairs only (dealt above: slot 0 in
      // every D wave, slot 1 in waves 4 and 5) and written to both places (block (p', p) is the transpose).  The packed slots
      // are unpacked per node - a few bit-field extracts - from an opaque copy: the addresses derived from them stay out of the
      // loop's live registers.
      const BuildSlot s0 = BuildSlot::unpack(opaque_u(slot0)), s1 = BuildSlot::unpack(opaque_u(slot1));
      const bool two = bw >= 2;                        // this wave has a second slot
      double hq[2][3] = {{0, 0, 0}, {0, 0, 0}}, xq[3] = {0, 0, 0}, gq[3] = {0, 0, 0}, cvq[3] = {0, 0, 0}, lamq = 0.0;
      bool liveq[3] = {false, false, false}, ownq[3] = {false, false, false};
      if (has_next) {
        const int cur = ch.st->cur;
        const double* Hg = cur ? ch.H1 : ch.H0;
        lamq = ch.st->lam;
#pragma unroll
        for (int j = 0; j < 3; ++j)
          if (fb_next + j < K.n_frames) {
            hq[0][j] = Hg[(size_t)(fb_next + j) * HPAIRS + s0.e];                   // (pair e = 13 p + d: as stored)
            if (two && s1.own) hq[1][j] = Hg[(size_t)(fb_next + j) * HPAIRS + s1.e];
          }
        if (s0.dg) {
          const int pdg = s0.pr;
          const double* xg = cur ? ch.x1 : ch.x0;
          const double* gg = cur ? ch.g1 : ch.g0;
#pragma unroll
          for (int j = 0; j < 3; ++j)
            if (fb_next + j < K.n_frames) {
              xq[j] = xg[(size_t)(fb_next + j + HALO) * NP + pdg];
              gq[j] = gg[(size_t)(fb_next + j) * NP + pdg];
            }
#pragma unroll
          for (int pr = 0; pr < 3; ++pr) {
            const int j = pr == 2 ? 1 : 0, jp = pr == 0 ? 1 : 2;
            if (fb_next + jp < K.n_frames)
              cvq[pr] = 2.0 * kq[pdg] * band_coef_clip(K.n_offset + fb_next + j, jp - j, K.n_global, K.clip_len);
          }
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          liveq[j] = fb_next + j < K.n_frames;
          ownq[j] = fb_next + j >= K.own_lo && fb_next + j < K.own_hi;
        }
      }
      if (bw == 0) SW_STAMP(0);
      // U_k complete (the trio came out of the factorisation), wave 4 through with the store of G_k-1; then every strip wave
      // through with Xg
      lds_barrier(cB, tb, 4, ln);
      lds_wait(c_gfdone, n_s * k);
      if (bw == 0) SW_STAMP(1);
      if (bt == 0) __hip_atomic_fetch_add(g_open, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      if (tab_write) {
        if (tab_interior) right_table_interior<256>(cRk, bt, [&](int p) { return kq[p]; });
        else fill_coupling_coef<256>(nullptr, cRk, K, node, bt, kq);
      }
      if (bw == 0) gram_fixed<0, 10>(Xf, Xg, g_done, li, lk, ln);
      else if (bw == 1) gram_fixed<1, 7>(Xf, Xg, g_done, li, lk, ln);
      else if (bw == 2) gram_fixed<4, 8, 12>(Xf, Xg, g_done, li, lk, ln);
      else gram_fixed<3, 6, 11>(Xf, Xg, g_done, li, lk, ln);
      SW_STAMP(32 + wave);
      lds_barrier(cB, tb, 4, ln);                      // (the tables of this node in place)
      lds_wait(g_done, 15 * (k + 1));                  // G_k in Xg, every read of U_k (Xf) done
      if (bw == 0) SW_STAMP(2);
#pragma unroll
      for (int j = 0; j < 3; ++j) asm volatile("" : "+v"(hq[0][j]), "+v"(hq[1][j]), "+v"(xq[j]), "+v"(gq[j]));
      asm volatile("" : "+v"(lamq));
      if (has_next) {
        double* const bvn = bvb + ((k + 1) & 1) * BS;
        // S = E^T G_k E on the thread's blocks (reads Xg), the next node written straight into Xf.  Per slot every LDS read first,
        // then the arithmetic, the stores guarded (a lane of slot 1 that owns no pair reads pair (0, 0)); the second slot's
        // reads follow the first slot's stores: both slots' operands in flight together cost 31 more registers and spilled
        double ca[2][6], cb[2][6], gv[2][3][3];
        auto slot_reads = [&](const BuildSlot& sl, double (&a)[6], double (&b)[6], double (&g)[3][3]) {
          const double *ta = cRk + sl.pr, *tb_ = cRk + sl.pc;
          a[0] = ta[0 * NP]; a[1] = ta[1 * NP]; a[2] = ta[2 * NP];
          a[3] = ta[4 * NP]; a[4] = ta[5 * NP]; a[5] = ta[8 * NP];
          b[0] = tb_[0 * NP]; b[1] = tb_[1 * NP]; b[2] = tb_[2 * NP];
          b[3] = tb_[4 * NP]; b[4] = tb_[5 * NP]; b[5] = tb_[8 * NP];
          const double* gp0 = Xg + sl.base;
#pragma unroll
          for (int jj = 0; jj < 3; ++jj) {
            const double* gp = gp0 + jj * NP * LD;
            g[jj][0] = gp[0];
            g[jj][1] = gp[NP];
            g[jj][2] = gp[2 * NP];
          }
        };
        // (DIAG: the slot may hold a diagonal pair - slot 0 only)
        auto slot_finish = [&](const BuildSlot& sl, auto may_diag, const double (&a)[6], const double (&b)[6], const double (&g)[3][3],
                               const double (&h)[3]) {
          // (the order of the operations and every fused multiply-add written out, contraction off: the node is the same bits
          //  whatever the compiler would choose to fuse around this code - sums of products take their SECOND product as the
          //  plain multiplication and fuse the others onto it, first then third)
#pragma clang fp contract(off)
          constexpr bool DIAG = decltype(may_diag)::value;
          const int pr = sl.pr;
          const bool dg = DIAG && sl.dg;
          const double a00 = a[0], a01 = a[1], a02 = a[2], a11 = a[3], a12 = a[4], a22 = a[5];
          const double b00 = b[0], b01 = b[1], b02 = b[2], b11 = b[3], b12 = b[4], b22 = b[5];
          double mm[3][3], S[2][3];
#pragma unroll
          for (int jj = 0; jj < 3; ++jj) {
            const double g0 = g[jj][0], g1 = g[jj][1], g2 = g[jj][2];
            mm[jj][0] = __builtin_fma(g2, b02, __builtin_fma(g0, b00, g1 * b01));      // g0 b00 + g1 b01 + g2 b02
            mm[jj][1] = __builtin_fma(g1, b11, g2 * b12);                               // g1 b11 + g2 b12
            mm[jj][2] = g2 * b22;
          }
#pragma unroll
          for (int ii = 0; ii < 3; ++ii) {
            S[0][ii] = __builtin_fma(a02, mm[2][ii], __builtin_fma(a00, mm[0][ii], a01 * mm[1][ii]));   // a00 mm0 + a01 mm1 + a02 mm2
            S[1][ii] = __builtin_fma(a11, mm[1][ii], a12 * mm[2][ii]);                                  // a11 mm1 + a12 mm2
          }
          double v[3][3];
#pragma unroll
          for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int jp = 0; jp < 3; ++jp) v[j][jp] = (j == jp ? h[j] : 0.0);
          if (dg) {
#pragma unroll
            for (int j = 0; j < 3; ++j) {
              double d = 1.0, bb = 0.0;
              if (liveq[j]) {
                d = h[j];
                const double gtol = GRAD_ZERO_REL * d;
                const bool fixed = (xq[j] <= klo[pr] && gq[j] > gtol) || (xq[j] >= khi[pr] && gq[j] < -gtol);
                d = __builtin_fma(lamq, fmax(d, DIAG_FLOOR), d);
                if (fixed) d *= FIX_SCALE;
                bb = fixed ? 0.0 : -gq[j];
                if (ownq[j]) gmax_run = fmax(gmax_run, fabs(bb));   // (window sharding: owned frames only)
              }
              v[j][j] = d;
              bvn[j * NP + pr] = bb;
            }
            v[0][1] = v[1][0] = cvq[0];
            v[0][2] = v[2][0] = cvq[1];
            v[1][2] = v[2][1] = cvq[2];
          }
          // v - S; row 2 of S is the single product a22 mm2: fused into the subtraction in columns 0 and 2, not in column 1
          double val[3][3];
#pragma unroll
          for (int jp = 0; jp < 3; ++jp) {
            val[0][jp] = v[0][jp] - S[0][jp];
            val[1][jp] = v[1][jp] - S[1][jp];
          }
          val[2][0] = __builtin_fma(-a22, mm[2][0], v[2][0]);
          val[2][1] = v[2][1] - a22 * mm[2][1];
          val[2][2] = __builtin_fma(-a22, mm[2][2], v[2][2]);
          if (sl.own) {
            double* const xa = Xf + sl.base;                     // block (p, p'): entry (j, jp) at (j NP + p) LD + jp NP + p'
            double* const xt = Xf + sl.pc * LD + pr;             // its transpose
#pragma unroll
            for (int j = 0; j < 3; ++j)
#pragma unroll
              for (int jp = 0; jp < 3; ++jp) {
                xa[j * NP * LD + jp * NP] = val[j][jp];
                if (!dg) xt[jp * NP * LD + j * NP] = val[j][jp];
              }
          }
        };
        const BuildSlot b0 = BuildSlot::unpack(opaque_u(slot0)), b1 = BuildSlot::unpack(opaque_u(slot1));
        slot_reads(b0, ca[0], cb[0], gv[0]);
        slot_finish(b0, std::true_type{}, ca[0], cb[0], gv[0], hq[0]);
        if (two) {
          slot_reads(b1, ca[1], cb[1], gv[1]);
          slot_finish(b1, std::false_type{}, ca[1], cb[1], gv[1], hq[1]);
        }
        // (padding rows / columns 75 .. 79: the factorisation left an identity block there; the diagonal is rewritten all the same,
        //  and the padding of the right-hand side is zero in both buffers)
        if (bt < BS - 3 * NP) {
          Xf[(3 * NP + bt) * LD + 3 * NP + bt] = 1.0;
          bvn[3 * NP + bt] = 0.0;
        }
      }
      lds_barrier(cB, tb, 4, ln);                      // next node complete in Xf
      if (bt == 0) __hip_atomic_fetch_add(c_bv, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      if (bw == 0) SW_STAMP(4);
      // the node built last is the right separator: its diagonal block is final in Xf -> HBM now, while the spike is finished
      auto store_sep_diag = [&](int part, int parts) {
        double2* d2 = reinterpret_cast<double2*>(sp.D + (size_t)sR * MB);
        for (int idx = 64 * part + ln; idx < BS * BS / 2; idx += 64 * parts) {
          const int e = 2 * idx, r = e / BS, cc = e % BS;
          d2[idx] = make_double2(Xf[r * LD + cc], Xf[r * LD + cc + 1]);
        }
      };
      if (bw < 3) {
        // (no closing barrier of the trio: the four D waves meet at the top of the next iteration, before anyone reads the factor)
        if (!last) {
          chol80_trio<false>(Xf, bw, ln, numeric_err, sync, tsy, (dbgp && k == dbg_k) ? lst : nullptr);
        } else if (!spread) {
          if (hasR) store_sep_diag(bw, 3);             // by the three waves that have no factorisation to do
        } else if (bw == 2) {
          if (hasR) store_sep_diag(0, 2);              // by waves 5 and 4: waves 0 and 1 take a strip each
        } else {
          if (dbgp && k == dbg_k && ln == 0) lst[63] = (long long)wall_clock64();    // (tells the stamps' reader the role map)
          const SpikeArgs sa = spike_args();
          if (bw == 0) spike_node<10>(sa, tsb, ln);
          else spike_node<9>(sa, tsb, ln);
        }
        SW_STAMP(8 + wave);
      } else if (bw == 3) {
        // G_k -> HBM: the chain's SIMD mate.  (At a last node with the roles spread wave 3, which has no strip there, stores it:
        // this wave's SIMD mate streams matrix instructions then, and a wave that moves data beside it is 3x slower and slows it.)
        if (!spread) store_G(Xg, ch.D + node * MB, ln);
        else if (hasR) store_sep_diag(1, 2);
        SW_STAMP(8 + wave);
      }
    }
    if (strips) {
      // ============================== the spike of node k ==============================
      const SpikeArgs sa = spike_args();
      if (role == 4) spike_node<4>(sa, tsb, ln);
      else if (role == 5) {
        if (spread) spike_node<8>(sa, tsb, ln);
        else spike_node<5>(sa, tsb, ln);
      } else if (role == 6) {
        if (spread) {                                  // its strip is wave 0's at this node: the tiles of AL handed over, then G_k's
          hand_over(c_end, ln);
          lds_wait(g_open, k + 1);
          gram_fixed<2, 13>(Xf, Xg, g_done, li, lk, ln);
          lds_wait(g_done, 15 * (k + 1));
          store_G(Xg, ch.D + node * MB, ln);           // (wave 4's at every other node)
          if (dbgp && k == dbg_k && ln == 0) lst[24] = (long long)wall_clock64();
        } else {
          spike_node<6>(sa, tsb, ln);
        }
      } else {
        spike_node<7>(sa, tsb, ln);
      }
    }
  }
  __syncthreads();                                     // both teams through
  if (dbgp) {
    if (tid == 0) lst[62] = (long long)wall_clock64();
    __syncthreads();
    if (tid < 64 && lst[tid]) dbgp[tid] = lst[tid];
  }
  // (The right separator - the node built last - left for HBM inside the last iteration, each part when it was final: the
  //  diagonal block by the D waves after the build, block(R, L) and the right-hand side strip by strip after the stencil pass.  A
  //  run with a right separator has at least one interior node: ChunkPlan::build.)
#undef SW_STAMP
  publish_gmax<SW_T>(gmax_run, red, ch.gn_part, c, tid);
  if (dbgp && tid == 0) dbgp[71] = (long long)wall_clock64();
}

// Separator q: D += AL (the run on its right; lower tiles - the factorisation reads no others).  The right-hand side rode as
// column 79 of the spike, so row 79 of AL holds -(sum W^T y) = the update of b, and rows / columns >= 75 of AL are not
// part of the Schur update.  (A launch of its own: folding it into the sweep - the later of a separator's two runs adds AL -
// needs a device-scope release per workgroup, i.e. an L2 write-back on a multi-XCD part: measured +140 us on the sweep.)
__global__ void __launch_bounds__(256) k_sep_combine(SepView sp, const int* __restrict__ status) {
  if (status && *status != 0) return;
  const int q = blockIdx.x, tid = threadIdx.x;
  const size_t MB = (size_t)BS * BS;
  double* D = sp.D + q * MB;
  const double* A = sp.AL + q * MB;
  // every operand of the thread in flight before the first add (the launch is two HBM round trips, not one per element)
  constexpr int NQ = (LOWER_ITEMS + 255) / 256;
  double2 dv[NQ], av[NQ];
  const double bq = tid < 3 * NP ? sp.b[(size_t)q * BS + tid] : 0.0, aq = tid < 3 * NP ? A[(size_t)(BS - 1) * BS + tid] : 0.0;
#pragma unroll
  for (int k = 0; k < NQ; ++k) {
    const int idx = tid + 256 * k;
    if (idx < LOWER_ITEMS) {
      int r, cc;
      lower_item(idx, r, cc);
      dv[k] = *reinterpret_cast<const double2*>(D + r * BS + cc);
      av[k] = *reinterpret_cast<const double2*>(A + r * BS + cc);
    }
  }
#pragma unroll
  for (int k = 0; k < NQ; ++k) {
    const int idx = tid + 256 * k;
    if (idx < LOWER_ITEMS) {
      int r, cc;
      lower_item(idx, r, cc);
      if (r < 3 * NP) {                                // rows / columns 75 .. 79 of AL are not part of the Schur update
        const double ax = cc < 3 * NP ? av[k].x : 0.0, ay = cc + 1 < 3 * NP ? av[k].y : 0.0;
        *reinterpret_cast<double2*>(D + r * BS + cc) = make_double2(dv[k].x + ax, dv[k].y + ay);
      }
    }
  }
  if (tid < 3 * NP) sp.b[(size_t)q * BS + tid] = bq + aq;
}

// Back-substitution, one workgroup per run.  x_k = z_k - G_k (E x_k+1) - T_k x_L with T_k = D~_k^-1 F_k; T_k is not
// stored.  Its action on the left separator's solution obeys the recurrence of the spike itself,
//     f_0 = F_0 x_L = E_l x_L,    t_k = T_k x_L = G_k f_k,    f_k+1 = F_k+1 x_L = -E^T t_k,
// so the run is walked twice over the same 31 KB per node (the lower tiles of G_k):
//   forward  k = 0 .. n-2 :  t_k = G_k f_k, f_k+1 = -E^T t_k            (f_k kept: 80 doubles per node, ch.Wl)
//   backward k = n-1 .. 0 :  x_k = z_k - G_k (E x_k+1 + f_k)
// i.e. 2 n - 1 DEPENDENT 80 x 80 matrix-vector products per run ("steps"), 61 KB of HBM reads per node.  Until round 4 a step
// took 2.1 us - three barriers of eight waves around the product (partial sums through LDS, row sums, stencil by 80 threads) -
// and a prefetch distance of one step.  Now the workgroup is two teams that meet only through LDS counters:
//   * FOUR PRODUCT WAVES, one per SIMD, which touch no global memory but their stores.  Lane (p, part) - p = 8 wave + lane / 8
//     one of the 25 states, part = lane % 8 - multiplies the THREE rows (a, p), a = 0 .. 2 (the state's entry in the node's three
//     frames) by the columns part + 8 j, j = 0 .. 9: 30 multiply-adds, then a three-step butterfly over the 8 lanes of the state
//     (DPP; every lane ends with the three complete sums, bit-identical).  The stencils E couple only the three frames of ONE
//     state, so lanes part = 0 .. 2 turn the sums into the next step's vector entries (a, p) with no further exchange, store
//     x_k / f_k+1 and form the trial iterate of their row; the new vector goes to the other of two LDS buffers, the four waves
//     meet at a counter, next step.
//   * FOUR LOADER WAVES, each with one whole node in flight (its 1920 two-double items = 30 per lane, the row operands z_k and
//     the trial row's x / g / diag H, f_k of far nodes, the step's coupling table where the tables change from node to node):
//     HBM -> registers -> one of two LDS stages when the product waves are through with it -> "ready".  A loader may sit in
//     s_waitcnt vmcnt(0) for as long as HBM takes - nobody waits for IT at a barrier - and the four of them keep 120 KB per CU in
//     flight, which is what the stream needs (the compiler turns a register ring of prefetches inside ONE wave's loop into
//     vmcnt(0 .. 1) waits: measured 66 us against the 51 us of the round-4 kernel).
// The LDS image of a node: lower tiles only, leading dimension 82 (16-byte rows for ds_write_b128; the transposed reads
// G[c][r] of the upper part - stride 164 words - spread over the banks).  f_k of the eight nodes before the turning point come
// from a ring in LDS written by the row lanes themselves (they are read back sooner than a loader could fetch them).
constexpr int BK_PW = 4;                                     // product waves (waves 0 .. 3)
constexpr int BK_NL = 4;                                     // loader waves: step t is loader t % 4's
constexpr int BK_T = 64 * (BK_PW + BK_NL);
constexpr int BK_NB = 2;                                     // LDS stages
constexpr int BLD = 82;
constexpr int BK_Q = LOWER_ITEMS / 64;                       // 30 two-double items per loader lane
constexpr int BK_FL = 8;                                     // f_k of the last BK_FL nodes of the forward pass stay in LDS
static_assert(LOWER_ITEMS == 64 * NT * (NT + 1), "30 rounds of 64 items: 2 (ib + 1) per tile row");
static_assert(BK_FL >= BK_NL + BK_NB + 2, "a far f_k must have been stored (and waited for) before a loader asks for it");
// one stage: the node's tiles | z x g diagH f rows [5][80] | right table of the step's node [225] (+ 1: even size)
constexpr int BK_OPS = BS * BLD, BK_TAB = BK_OPS + 5 * BS, BK_STAGE = BK_TAB + 9 * NP + 1;
static constexpr size_t kBacksubLds =
    (BK_NB * BK_STAGE + 2 * BS + BK_FL * BS + 2 * 9 * NP + 16 + NP + 1) * sizeof(double) + 16 * sizeof(int);

typedef double d2 __attribute__((ext_vector_type(2)));
template <int CTRL>
__device__ __forceinline__ double dpp_add(double v) {      // v + (v of the lane CTRL names)
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_update_dpp(0, (int)b, CTRL, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, 0xf, 0xf, false);
  return v + __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}
// sum over the 8 lanes of a state (i <-> 7 - i, then i <-> i ^ 1, i <-> i ^ 2): every lane receives the same bits (a + b and
// b + a at every level)
__device__ __forceinline__ double lanes8_sum(double v) {
  v = dpp_add<0x141>(v);                                     // row_half_mirror
  v = dpp_add<0xB1>(v);                                      // quad_perm [1, 0, 3, 2]
  return dpp_add<0x4E>(v);                                   // quad_perm [2, 3, 0, 1]
}
__global__ void __launch_bounds__(BK_T)
k_chunk_backsub(BcrChain ch, SepView sp, const FteConst* __restrict__ cst, const int* __restrict__ status, int m,
                int n_chunks, int node0, int pin_right, TrialOut trial) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  double* const stg = reinterpret_cast<double*>(smem_raw);   // [BK_NB][BK_STAGE]
  double* const ub = stg + BK_NB * BK_STAGE;                   // [2][80] the product's vector, by step parity
  double* const fl = ub + 2 * BS;                              // [BK_FL][80] f_k of the nodes before the turning point
  double* const cL0 = fl + BK_FL * BS;                         // left table of the first node
  double* const cRl = cL0 + 9 * NP;                            // right table of the last interior node
  double* const red = cRl + 9 * NP;                            // [16]
  double* const kq = red + 16;                                 // [25] copy of K.q_w (+ 1 pad)
  int* const sync = reinterpret_cast<int*>(kq + NP + 1);       // ready, per loader | stage read | vector written
  int* const c_ready = sync;
  int* const c_rd = sync + BK_NL;
  int* const c_u = sync + BK_NL + 1;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = blockIdx.x, first = node0 + c * m;
  const bool hasL = c > 0 || node0 > 0, hasR = c + 1 < n_chunks || pin_right;
  const int len = c + 1 < n_chunks ? m : ch.n_nodes - first;
  const int n_int = hasR ? len - 1 : len;
  const int sL = c - 1 + node0, sR = c + node0;
  const size_t MB = (size_t)BS * BS;
  const int nf = hasL && n_int > 0 ? n_int - 1 : 0;         // forward steps; then n_int backward steps
  const int ns = nf + n_int;
  auto node_at = [&](int s) __attribute__((always_inline)) { return s < nf ? s : n_int - 1 - (s - nf); };   // local node of step s
  // ---- loader waves: the tiles of their first node are requested before anything else is looked at (the status word, the
  //      iterate's buffer index, the tables: three dependent round trips to memory that the first tiles now share)
  // Round q of a node's 30 rounds of 64 two-double items: eight rows of one tile row x eight items (one 128-byte line per row),
  // q -> (tile row ib, half h of its rows, 16-column chunk jc <= ib) at compile time.  The lane's part of every address is the
  // same in all rounds (row lane / 8 of the eight, item lane % 8 of the line): two registers, the rest are immediates.
  struct Rounds {
    int row0[BK_Q], col0[BK_Q];
    constexpr Rounds() : row0{}, col0{} {
      int q = 0;
      for (int ib = 0; ib < NT; ++ib)
        for (int h = 0; h < 2; ++h)
          for (int jc = 0; jc <= ib; ++jc) {
            row0[q] = 16 * ib + 8 * h;
            col0[q] = 16 * jc;
            ++q;
          }
    }
  };
  constexpr Rounds RD{};
  const int gl = (lane >> 3) * BS + 2 * (lane & 7), ll = (lane >> 3) * BLD + 2 * (lane & 7);
  d2 g[BK_Q];
  // (rows 75 .. 79 of G_k are rows of the identity - padding - and are never read as rows: the lanes that would fetch them ask
  //  for row 74 again, which costs no traffic: 10 % of the node's bytes)
  const int gl74 = ((lane >> 3) < 3 ? (lane >> 3) : 2) * BS + 2 * (lane & 7);
  auto tile_fetch = [&](int k) __attribute__((always_inline)) {
    const double* G = ch.D + (size_t)(first + k) * MB;
#pragma unroll
    for (int q = 0; q < BK_Q; ++q)
      g[q] = *reinterpret_cast<const d2*>(G + (RD.row0[q] * BS + RD.col0[q]) + (RD.row0[q] + 8 > 3 * NP ? gl74 : gl));
  };
  // Loader lw's jobs: steps lw, lw + BK_NL, ..
  const int lw = wave - BK_PW;
  if (lw >= 0 && lw < ns) tile_fetch(node_at(lw));
  if (status && *status != 0) return;
  const FteConst& K = *cst;
  const bool uni = coupling_tables_uniform(K, first, first + n_int - 1);   // (one table serves every node of the run)
  // the node whose right table step s uses: its own (forward: f_k+1 = -E_k^T t_k) or the next one's (backward: u_k-1 = .. E_k-1 x_k)
  auto table_node = [&](int s) __attribute__((always_inline)) {
    const int k = node_at(s);
    return s < nf ? k : (k > 0 ? k - 1 : 0);
  };
  const int t_cur = ch.st->cur, t_nf = K.n_frames;
  const double* t_x = t_cur ? ch.x1 : ch.x0;
  const double* t_g = t_cur ? ch.g1 : ch.g0;
  const double* t_hd = t_cur ? trial.hd1 : trial.hd0;
  double* const fst = ch.Wl + (size_t)first * BS;           // f_k of this run's nodes
  if (ch.dbg && (long long)blockIdx.x == ch.dbg[64] && ch.dbg[66] == 1 && tid == 0) ch.dbg[61] = (long long)wall_clock64();
  if (c == 0 && sp.flags) {                                 // (k_sep_tail's flags: clean for the next iteration; the int behind
    for (int e = tid; e < sp.n_flags; e += BK_T) sp.flags[e] = 0;   // them is the epoch its hand-off tags are made of)
    if (tid == 0) sp.flags[sp.n_flags] += 1;
  }
  if (tid < 16) sync[tid] = 0;
  if (tid < 2 * BS) ub[tid] = 0.0;
  if (tid < NP) kq[tid] = K.q_w[tid];
  fill_coupling_coef<BK_T>(cL0, nullptr, K, first, tid);
  fill_coupling_coef<BK_T>(nullptr, cRl, K, first + (n_int > 0 ? n_int - 1 : 0), tid);
  double t_pred = 0.0, t_step = 0.0;
  if (wave >= BK_PW) {
    // ================================ loader waves ================================
    // row operands of a backward step: [5][75] values (z, x, g, diag H, f_k-1), entry lane + 64 j; requested a job ahead, with
    // the tiles
    constexpr int NRO = (5 * 3 * NP + 63) / 64;
    double ro[NRO];
    auto ro_fetch = [&](int t) __attribute__((always_inline)) {
      if (t < nf) return;
      const int k = node_at(t), node = first + k;
      const bool far = hasL && k >= 1 && n_int - k >= BK_FL;   // f_k-1 is no longer in the LDS ring
      const int ln = opaque(lane);                          // (the address arithmetic stays inside the loop: registers)
#pragma unroll
      for (int j = 0; j < NRO; ++j) {
        const int e = ln + 64 * j < 5 * 3 * NP ? ln + 64 * j : 5 * 3 * NP - 1, o = e / (3 * NP), r = e % (3 * NP);
        int n = 3 * (node - node0) + r / NP;
        n = n < t_nf ? n : t_nf - 1;
        const size_t nr = (size_t)n * NP + r % NP;
        const double* src = o == 0 ? ch.b + (size_t)node * BS + r
                          : o == 1 ? t_x + nr + (size_t)HALO * NP
                          : o == 2 ? t_g + nr
                          : o == 3 ? t_hd + nr
                                   : fst + (size_t)(far ? k - 1 : 0) * BS + r;
        ro[j] = *src;
      }
      if (lane < BS - 3 * NP) ch.b[(size_t)node * BS + 3 * NP + lane] = 0.0;   // (padding rows of the solution)
    };
    if (lw < ns) ro_fetch(lw);
    __syncthreads();                                        // counters, kq
    for (int t = lw; t < ns; t += BK_NL) {
      const bool bwd = t >= nf;
      long long* const ldbg = (ch.dbg && (long long)blockIdx.x == ch.dbg[64] && ch.dbg[66] == 1 && lane == 0 && t >= 10 && t < 14) ? ch.dbg + 48 + 4 * (t - 10) : nullptr;
      if (ldbg) ldbg[0] = (long long)wall_clock64();
      if (t >= BK_NB) lds_wait(c_rd, BK_PW * (t - BK_NB + 1));   // the product waves are through with the stage
      if (ldbg) { __builtin_amdgcn_s_waitcnt(0x0F70); ldbg[1] = (long long)wall_clock64(); }
      double* const St = stg + (t % BK_NB) * BK_STAGE;
#pragma unroll
      for (int q = 0; q < BK_Q; ++q) *reinterpret_cast<d2*>(St + ll + (RD.row0[q] * BLD + RD.col0[q])) = g[q];
      if (bwd) {
        const int ln = opaque(lane);
#pragma unroll
        for (int j = 0; j < NRO; ++j) {
          const int e = ln + 64 * j;
          if (e < 5 * 3 * NP) St[BK_OPS + (e / (3 * NP)) * BS + e % (3 * NP)] = ro[j];
        }
      }
      // the step's table: the first node's serves every step of a uniform run (the product waves read it in steps 0 and 1);
      // elsewhere most nodes still have the interior table
      if (uni) {
        if (t < BK_NB) right_table_interior<64>(St + BK_TAB, lane, [&](int p) { return kq[p]; });
      } else if (right_table_is_interior(K, first + table_node(t))) {
        right_table_interior<64>(St + BK_TAB, lane, [&](int p) { return kq[p]; });
      } else {
        fill_coupling_coef<64>(nullptr, St + BK_TAB, K, first + table_node(t), lane, kq);
      }
      if (ldbg) { __builtin_amdgcn_s_waitcnt(0xC07F); ldbg[2] = (long long)wall_clock64(); }
      lds_signal(c_ready + lw, lane);
      if (t + BK_NL < ns) {                                 // the next job's tiles and row operands
        tile_fetch(node_at(t + BK_NL));
        ro_fetch(t + BK_NL);
      }
    }
  } else {
    // ================================ product waves ================================
    const int pg = lane >> 3, part = lane & 7;
    const int p = 8 * wave + pg, pc = p < NP ? p : NP - 1;
    const int a = part < 3 ? part : 2, ra = a * NP + pc;    // the lane's row of the triple (lanes part >= 3 shadow row 2)
    const bool rowl = p < NP && part < 3;
    const int t_own_lo = K.own_lo, t_own_hi = K.own_hi;
    const double t_lam = ch.st->lam;
    double* t_xt = const_cast<double*>(t_cur ? ch.x0 : ch.x1);   // (the other iterate buffer: the chain view holds both read-only)
    const double t_lo = K.lo[pc], t_hi = K.hi[pc];
    // trial iterate (fte_api.hip k_trial, same arithmetic): a row lane owns row (a, p) of every node of the run
    auto trial_row = [&](int node, double delta, double xv, double gv, double d0) __attribute__((always_inline)) {
      const int n = 3 * (node - node0) + a;
      if (rowl && n < t_nf) {
        const double gtol = GRAD_ZERO_REL * d0;
        const bool fixed = (xv <= t_lo && gv > gtol) || (xv >= t_hi && gv < -gtol);   // (a bound-active variable takes a step of 0)
        const double d = fixed ? 0.0 : delta, pg_ = fixed ? 0.0 : gv;
        const double xnew = fmin(fmax(xv + d, t_lo), t_hi);
        t_xt[(size_t)(n + HALO) * NP + pc] = xnew;
        if (n >= t_own_lo && n < t_own_hi) {                // (window sharding: only owned frames enter the global sums)
          t_pred += 0.5 * d * (t_lam * fmax(d0, DIAG_FLOOR) * d - pg_);
          t_step = fmax(t_step, fabs(xnew - xv));
        }
      }
    };
    // LDS offsets of the lane's 30 entries: G[(a, p)][part + 8 j] lies in a stored tile when j / 2 <= tile row of (a, p), else it
    // is read as G[part + 8 j][(a, p)]: two bases per row, the rest immediates (30 offsets kept in registers would not fit
    // beside the loaders' 120 registers of tiles: 12 waves share the CU's register file)
    constexpr int NJ = BS / 8;
    int gdir[3], gtrn[3], gtile[3];
#pragma unroll
    for (int aa = 0; aa < 3; ++aa) {
      const int r = aa * NP + pc;
      gdir[aa] = r * BLD + part;
      gtrn[aa] = part * BLD + r;
      gtile[aa] = r >> 4;
    }
    // the two separator solutions, the right separator's trial row, the first vector
    double xr[3] = {0, 0, 0}, xl[3] = {0, 0, 0};
    if (hasR) {
#pragma unroll
      for (int ii = 0; ii < 3; ++ii) xr[ii] = sp.b[(size_t)sR * BS + ii * NP + pc];
      if (tid < BS) ch.b[(size_t)(first + n_int) * BS + tid] = sp.b[(size_t)sR * BS + tid];   // the separator's solution joins the chain's vector
    }
    if (hasL) {
#pragma unroll
      for (int jj = 0; jj < 3; ++jj) xl[jj] = sp.b[(size_t)sL * BS + jj * NP + pc];
    }
    double s_xv, s_gv, s_d0;
    {
      int n = 3 * (first + n_int - node0) + a;
      n = n < t_nf ? n : t_nf - 1;
      s_xv = t_x[(size_t)(n + HALO) * NP + pc];
      s_gv = t_g[(size_t)n * NP + pc];
      s_d0 = t_hd[(size_t)n * NP + pc];
    }
    __syncthreads();                                        // tables, zeros, counters
    double wR = 0.0, f0 = 0.0;                              // (E_r x_R)[(a, p)] for the last interior node, (E_l x_L)[(a, p)]
#pragma unroll
    for (int ii = 0; ii < 3; ++ii)
      if (ii <= a) wR += cRl[(ii * 3 + a) * NP + pc] * xr[ii];
#pragma unroll
    for (int jj = 0; jj < 3; ++jj)
      if (jj >= a) f0 += cL0[(a * 3 + jj) * NP + pc] * xl[jj];
    if (rowl) {
      ub[ra] = nf > 0 ? f0 : f0 + wR;
      if (hasL) {
        fst[ra] = f0;
        fl[ra] = f0;
      }
    }
    lds_signal(c_u, lane);                                  // (the vector of step 0: c_u counts from BK_PW)
    // debug stamps (scripts/backsub_stamps.py): wave 0 of the selected workgroup, per step "stage ready" / "vector ready"
    long long* const bdbg = (ch.dbg && (long long)blockIdx.x == ch.dbg[64] && ch.dbg[66] == 1 && tid == 0) ? ch.dbg : nullptr;
    if (bdbg) bdbg[62] = (long long)wall_clock64();
    double cf[6] = {0, 0, 0, 0, 0, 0};                      // c00 c01 c02 c11 c12 c22 of the step's table for state p
    bool pend = false;                                      // a backward step's stores and trial row, done under the next step's reads
    int p_node = 0;
    double p_xa = 0.0, p_xv = 0.0, p_gv = 0.0, p_d0 = 0.0;
#pragma unroll 1
    for (int s = 0; s < ns; ++s) {
      const int b = s & 1;
      const bool fwd = s < nf;
      const int k = node_at(s), node = first + k;
      const double* const St = stg + (s % BK_NB) * BK_STAGE;
#define BK_STAMP(i) do { if (bdbg && s >= 8 && s < 16) { __builtin_amdgcn_s_waitcnt(0xC07F); bdbg[6 * (s - 8) + (i)] = (long long)wall_clock64(); } } while (0)
      // the node's stage and the vector (every product wave through with step s - 1), one poll for both
      lds_wait2(c_ready + (s % BK_NL), s / BK_NL + 1, c_u, BK_PW * (s + 1));
      BK_STAMP(0);
      BK_STAMP(1);
      double uv[NJ], gv[3][NJ];
#pragma unroll
      for (int j = 0; j < NJ; ++j) uv[j] = ub[b * BS + part + 8 * j];
#pragma unroll
      for (int aa = 0; aa < 3; ++aa) {
        const int gd = opaque(gdir[aa]), gt = opaque(gtrn[aa]);
#pragma unroll
        for (int j = 0; j < NJ; ++j) gv[aa][j] = St[(j >> 1) <= gtile[aa] ? gd + 8 * j : gt + 8 * j * BLD];
      }
      if (!uni || s < BK_NB) {
        const double* T = St + BK_TAB;
        cf[0] = T[0 * NP + pc]; cf[1] = T[1 * NP + pc]; cf[2] = T[2 * NP + pc];
        cf[3] = T[4 * NP + pc]; cf[4] = T[5 * NP + pc]; cf[5] = T[8 * NP + pc];
      }
      const double z0 = St[BK_OPS + pc], z1 = St[BK_OPS + NP + pc], z2 = St[BK_OPS + 2 * NP + pc];
      const double o_xv = St[BK_OPS + BS + ra], o_gv = St[BK_OPS + 2 * BS + ra], o_d0 = St[BK_OPS + 3 * BS + ra];
      const double o_f = St[BK_OPS + 4 * BS + ra];
      const double fnear = fl[((k > 0 ? k - 1 : 0) % BK_FL) * BS + ra];
      lds_signal(c_rd, lane);                               // (behind the reads: the LDS serves a wave's requests in order)
      // the previous step's solution row and trial row, while this step's operands are on their way from the LDS
      if (pend) {
        if (rowl) ch.b[(size_t)p_node * BS + ra] = p_xa;
        trial_row(p_node, p_xa, p_xv, p_gv, p_d0);
        pend = false;
      }
      BK_STAMP(2);
      double y[3];
#pragma unroll
      for (int aa = 0; aa < 3; ++aa) {
        double v0 = gv[aa][0] * uv[0], v1 = gv[aa][1] * uv[1];
#pragma unroll
        for (int j = 2; j < NJ; j += 2) {
          v0 = fma(gv[aa][j], uv[j], v0);
          v1 = fma(gv[aa][j + 1], uv[j + 1], v1);
        }
        y[aa] = lanes8_sum(v0 + v1);
      }
      if (bdbg && s >= 8 && s < 16) { asm volatile("" :: "v"(y[0]), "v"(y[1]), "v"(y[2])); bdbg[6 * (s - 8) + 3] = (long long)wall_clock64(); }
      if (fwd) {
        // t_k = y;  f_k+1 = -E^T t_k:  row (a, p) = -sum_{bb >= a} c[a][bb] t[(bb, p)]
        const double f0_ = -(cf[0] * y[0] + cf[1] * y[1] + cf[2] * y[2]);
        const double f1_ = -(cf[3] * y[1] + cf[4] * y[2]);
        const double f2_ = -(cf[5] * y[2]);
        const double fn = a == 0 ? f0_ : (a == 1 ? f1_ : f2_);
        if (rowl) {
          ub[(b ^ 1) * BS + ra] = s + 1 == nf ? fn + wR : fn;
          fl[((k + 1) % BK_FL) * BS + ra] = fn;
          fst[(size_t)(k + 1) * BS + ra] = fn;
        }
        // every f_k of the run stored (at L2) before a loader may ask for one: the loaders start on far f_k only after the product
        // waves have read two stages beyond the turning point
        if (s + 1 == nf) __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0)
        lds_signal(c_u, lane);
        BK_STAMP(4);
      } else {
        const double x0 = z0 - y[0], x1 = z1 - y[1], x2 = z2 - y[2];
        const double xa = a == 0 ? x0 : (a == 1 ? x1 : x2);
        // u_k-1 = f_k-1 + E_r(k-1) x_k:  row (a, p) = sum_{ii <= a} c[ii][a] x[(ii, p)]
        const double e0 = cf[0] * x0, e1 = cf[1] * x0 + cf[3] * x1, e2 = cf[2] * x0 + cf[4] * x1 + cf[5] * x2;
        const double fk = hasL ? (n_int - k < BK_FL ? fnear : o_f) : 0.0;
        if (rowl && k > 0) ub[(b ^ 1) * BS + ra] = fk + (a == 0 ? e0 : (a == 1 ? e1 : e2));
        lds_signal(c_u, lane);                              // (the next step's vector is complete: the rest is stores)
        BK_STAMP(4);
        pend = true;
        p_node = node;
        p_xa = xa;
        p_xv = o_xv;
        p_gv = o_gv;
        p_d0 = o_d0;
      }
      if (bdbg && s >= 8 && s < 16) bdbg[6 * (s - 8) + 5] = (long long)wall_clock64();
    }
#undef BK_STAMP
    if (pend) {
      if (rowl) ch.b[(size_t)p_node * BS + ra] = p_xa;
      trial_row(p_node, p_xa, p_xv, p_gv, p_d0);
    }
    if (bdbg) bdbg[63] = (long long)wall_clock64();
    if (hasR) trial_row(first + n_int, a == 0 ? xr[0] : (a == 1 ? xr[1] : xr[2]), s_xv, s_gv, s_d0);
  }
  // the run's share of the predicted reduction (sum) and of the step length (max), fixed order
  for (int off = 32; off > 0; off >>= 1) {
    t_pred += __shfl_down(t_pred, off, 64);
    t_step = fmax(t_step, __shfl_down(t_step, off, 64));
  }
  if (lane == 0 && wave < BK_PW) {
    red[2 * wave] = t_pred;
    red[2 * wave + 1] = t_step;
  }
  __syncthreads();
  if (tid == 0) {
    double sp_ = 0.0, sm = 0.0;
#pragma unroll
    for (int w = 0; w < BK_PW; ++w) {
      sp_ += red[2 * w];
      sm = fmax(sm, red[2 * w + 1]);
    }
    trial.pred_part[c] = sp_;
    trial.step_part[c] = sm;
  }
}

int chunk_set_func_attributes() {
  ACINO_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_chunk_sweep),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSweepLds));
  ACINO_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_chunk_backsub),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)kBacksubLds));
  return ACINO_OK;
}

int chunk_reduce(const BcrChain& ch, const ChunkPlan& pl, const SepView& sp, const BcrChain& sepch,
                 const BcrSchedule& sepsch, const FteConst* d_c, int* d_numeric_err, const int* d_status, hipStream_t s,
                 Profiler* prof) {
  {
    ProfSpan span(prof, PC_CHUNK_SWEEP, s, pl.n_nodes - pl.n_sep);
    hipLaunchKernelGGL(k_chunk_sweep, dim3(pl.n_chunks), dim3(SW_T), kSweepLds, s, ch, sp, d_c, d_numeric_err, d_status, pl.m,
                       pl.n_chunks, pl.node0, pl.pin_right);
  }
  ACINO_LAUNCH_CHECK();
  if (pl.n_sep == 0) return ACINO_OK;
  if (!sepsch.consumers_add_al) {    // (otherwise the kernels that consume each separator add its AL: sepch.AL0)
    {
      ProfSpan span(prof, PC_SEP_COMBINE, s, pl.n_sep);
      hipLaunchKernelGGL(k_sep_combine, dim3(pl.n_sep), dim3(256), 0, s, sp, d_status);
    }
    ACINO_LAUNCH_CHECK();
  }
  return bcr_reduce(sepch, sepsch, d_c, d_numeric_err, d_status, s, prof);
}

int chunk_backsub(const BcrChain& ch, const ChunkPlan& pl, const SepView& sp, const BcrChain& sepch,
                  const BcrSchedule& sepsch, const FteConst* d_c, int* d_numeric_err, const int* d_status, hipStream_t s,
                  Profiler* prof, const TrialOut& trial) {
  if (pl.n_sep > 0) {
    int rc = bcr_backsub(sepch, sepsch, d_c, d_status, s, prof, d_numeric_err);
    if (rc) return rc;
  }
  {
    ProfSpan span(prof, PC_CHUNK_BACKSUB, s, pl.n_nodes - pl.n_sep);
    hipLaunchKernelGGL(k_chunk_backsub, dim3(pl.n_chunks), dim3(BK_T), kBacksubLds, s, ch, sp, d_c, d_status, pl.m, pl.n_chunks, pl.node0,
                       pl.pin_right, trial);
  }
  ACINO_LAUNCH_CHECK();
  return ACINO_OK;
}

}  // namespace acino

extern "C" int acino_debug_coupling_table(int64_t n_global, int64_t n_frames, int64_t n_offset, int64_t clip_len, int pin_left,
                                          int node, int32_t* interior, double* coef) {
  using namespace acino;
  ACINO_REQUIRE(interior && coef, "outputs");
  ACINO_REQUIRE(n_global >= 1 && n_frames >= 1 && n_frames <= INT32_MAX && n_offset >= 0 && n_offset + n_frames <= n_global &&
                    clip_len >= 0 && (pin_left == 0 || pin_left == 1),
                "a window of n_frames frames at n_offset inside n_global frames");
  const TableGeom G{n_global, n_offset, clip_len, (int32_t)n_frames, pin_left};
  *interior = right_table_is_interior(G, node) ? 1 : 0;
  for (int ii = 0; ii < 3; ++ii)
    for (int jj = 0; jj < 3; ++jj) coef[3 * ii + jj] = right_table_band(G, node, ii, jj);
  return ACINO_OK;
}
