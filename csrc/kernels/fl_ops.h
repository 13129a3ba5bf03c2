#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "common.h"

// Contract of the weighted sums, FedAvg, broadcast and mixing launchers below:
//  * rows of weight 0 are never read (fl_weighted_sum, fl_stacked_weighted_sum, fl_fedavg_reduce,
//    fl_fedavg_local): a peer that did not train may hold anything, NaN included;
//  * any 4-byte-aligned pointer and any ld >= n is accepted, and the result does not depend on
//    alignment: the 16-byte vector path runs only when ld % 4 == 0 and every base pointer (out,
//    out2, stacked, src) is 16-byte aligned, the scalar path otherwise. fl_weighted_sum cannot see
//    its row pointers (they live in device memory): the caller says whether all of them are
//    16-byte aligned. The one exception is fl_neighbor_mix, which has no scalar path: it needs
//    ld % 4 == 0, ld >= 4·ceil(n/4) and a 16-byte-aligned base (myfyp_neighbor_mix_stacked
//    rejects anything else with status 2).
void fl_weighted_sum(float* out, const uint64_t* srcs, const float* w, int K, int64_t n, bool srcs_aligned16, hipStream_t s);
void fl_stacked_weighted_sum(float* out, const float* stacked, int P, int64_t n, int64_t ld, const float* w, float scale, hipStream_t s);
void fl_broadcast_rows(float* stacked, const float* src, int P, int64_t n, int64_t ld, const float* mask, hipStream_t s);
#define FEDAVG_MAX_PEERS 64
struct FedAvgWeights {
  float w[FEDAVG_MAX_PEERS];
  float wsum;
};
void fl_fedavg_reduce(float* out, float* wsum_slot, const float* stacked, int P, int64_t n, int64_t ld, const FedAvgWeights& w, hipStream_t s,
                      float* out2 = nullptr, float* wsum2 = nullptr);
void fl_fedavg_apply(float* stacked, const float* out, const float* wsum_slot, int P, int64_t n, int64_t ld, unsigned long long mask, hipStream_t s);
void fl_fedavg_delayed_land(float* stacked, float* snap, int64_t ld_snap, const float* avg, const float* wsum_slot, int P, int64_t n, int64_t ld,
                            unsigned long long mask, hipStream_t s);
void fl_fedavg_local(float* stacked, int P, int64_t n, int64_t ld, const FedAvgWeights& w, unsigned long long mask, hipStream_t s);
// Topology mixing of a stacked group in place: row p <- sum_k w[p][k] * row idx[p][k] (P <= 16 rows,
// up to P sources per row; rows with nsrc == 0 are left alone).
#define MIX_MAX_PEERS 16
#define MIX_MAX_SRC MIX_MAX_PEERS  // a row may mix every local peer (full / star topologies)
struct MixPlan {
  float w[MIX_MAX_PEERS][MIX_MAX_SRC];
  unsigned char idx[MIX_MAX_PEERS][MIX_MAX_SRC];
  unsigned char nsrc[MIX_MAX_PEERS];
};
void fl_neighbor_mix(float* stacked, int P, int64_t n, int64_t ld, const MixPlan& m, hipStream_t s);
struct RowPtrs {  // up to 16 row base pointers passed by value
  const float* p[16];
};
struct OutPtrs {  // up to 16 destination rows passed by value
  float* p[16];
};
struct RowW {
  float w[16];
};
// out rows 0..P-1 <- per-coordinate median of rows 0..K-1 (outputs may alias inputs)
void fl_coordinate_median(const OutPtrs& outs, int P, const RowPtrs& rows, int K, int64_t n, hipStream_t s);
// out rows 0..P-1 <- per-coordinate mean of the sorted values v[trim .. K-trim) of rows 0..K-1
// (0 <= 2*trim < K; outputs may alias inputs)
void fl_trimmed_mean(const OutPtrs& outs, int P, const RowPtrs& rows, int K, int trim, int64_t n, hipStream_t s);
// (Multi-)Krum. fl_krum_grid: blocks of the distance launch, a function of n and K only (work holds
// grid * K(K-1)/2 floats). fl_krum_select: pairwise squared distances of rows 0..K-1, scores over
// the min(max(1, K-f-2), K-1) nearest rows, the max(1, min(m, K)) best rows chosen; device outputs
// dist[K*K] and score[K] (double) and coef[K] = w_i / sum of the chosen w (0 for the others).
// fl_coef_mean: out rows 0..P-1 <- sum_k coef[k] * row k, coef in device memory (outputs may alias rows).
unsigned fl_krum_grid(int64_t n, int K);
void fl_krum_select(float* work, const RowPtrs& rows, const RowW& w, int K, int f, int m, int64_t n, double* dist, double* score, float* coef,
                    hipStream_t s);
void fl_coef_mean(const OutPtrs& outs, int P, const RowPtrs& rows, int K, const float* coef, int64_t n, hipStream_t s);
// Geometric median (smoothed Weiszfeld, iters steps) of rows 0..K-1: a screen pass that rejects the
// rows whose sum of squares is not a finite float, then per step the distances to the current
// point (from differences to a reference row) and coef <- w_k / max(nu, d_k), normalised. Device
// outputs coef[K] (float), dist[K] (double, the last step's distances) and obj[iters] (double,
// sum of w_k d_k per step). work holds fl_geomed_work(n, K) floats; the grid is fl_krum_grid(n, K).
// 2 (iters + 1) launches; fl_coef_mean then writes the outputs.
inline int64_t fl_geomed_work(int64_t n, int K) { return (int64_t)fl_krum_grid(n, K) * K + 16; }
void fl_geometric_median(float* work, const RowPtrs& rows, const RowW& w, int K, int iters, double nu, int64_t n, float* coef, double* dist,
                         double* obj, hipStream_t s);
// Bulyan (El Mhamdi, Guerraoui, Rouault, 2018) of rows 0..K-1 with at most f attackers (K >= 4f + 3,
// or f == 0): the distances of fl_krum_select on the same grid (work holds the same floats), theta =
// K - 2f rows picked by iterated Krum, then per coordinate the mean of the K - 4f picked values
// closest to their median into out rows 0..P-1 (outputs may alias rows; P == 0: selection only).
// Device outputs dist[K*K], score[K] (double: Krum's for the same f), pick[K] (int: the iteration a
// row was picked at, or -1) and coef[K] (float: 1/theta for a picked row, else 0). Three launches.
void fl_bulyan(float* work, const OutPtrs& outs, int P, const RowPtrs& rows, int K, int f, int64_t n, double* dist, double* score, int* pick,
               float* coef, hipStream_t s);
// The last of fl_bulyan's launches alone: coef[K] in device memory marks the K - 2f picked rows.
void fl_bulyan_mean(const OutPtrs& outs, int P, const RowPtrs& rows, int K, int f, const float* coef, int64_t n, hipStream_t s);
// Divide-and-Conquer (DnC; Shejwalkar & Houmansadr, NDSS 2021) of rows 0..K-1: per iteration t <
// iters (1..DNC_MAX_ITERS) the distances of fl_krum_select over a subsample of the coordinates, on
// the same grid (work holds iters * fl_krum_grid(n, K) * K(K-1)/2 floats); the rows of non-finite
// distances screened; the centred Gram matrix G = -1/2 J D J of the others, its top eigenpair
// (lam, u) by repeated squaring, the scores lam * u_i^2 (+inf for a screened row) and the m highest
// removed (the higher row first among equals; screened rows always go, and count towards m). A row
// is kept iff every iteration keeps it; out rows 0..P-1 <- sum_k coef[k] * row k with coef[k] =
// w_k / sum of the kept w, 0 for the others (nothing kept: every row, coef[k] = w_k / sum of w).
// Outputs may alias rows; P == 0: selection only. Coordinates go in tiles of 256 (coordinates
// 256 tau .. 256 tau + 255): with all == 0, tile tau of iteration t is taken iff
// splitmix64(key[t] ^ tau) < thr or tau == forced[t]; with all != 0 every tile is, and the slabs
// equal fl_krum_select's bit for bit. Device outputs dist[iters*K*K], score[iters*K], lam[iters]
// (double), removed[K] (int: the first iteration that removed the row, or -1) and coef[K] (float).
// Three launches: k_dnc_sqdist (gridDim.y = iters), k_dnc_select, k_coef_mean when P > 0. K == 1
// issues only the mean: no pair exists, and the caller has stored coef[0] (and the other outputs).
#define DNC_MAX_ITERS 8
struct DncTiles {
  uint64_t key[DNC_MAX_ITERS];
  uint64_t forced[DNC_MAX_ITERS];
  uint64_t thr;
  int all;
};
void fl_dnc(float* work, const OutPtrs& outs, int P, const RowPtrs& rows, const RowW& w, int K, int m, int iters, const DncTiles& tiles, int64_t n,
            double* dist, double* score, double* lam, int* removed, float* coef, hipStream_t s);
// ClippedGossip (He, Karimireddy, Jaggi, 2022) of rows 0..K-1 in place: row p moves towards each
// neighbour q (w[p][q] > 0, q != p; the diagonal is ignored) by at most a radius,
//   x_p <- x_p + sum_q w_eff[p][q] (x_q - x_p),  w_eff[p][q] = float(w[p][q] * min(1, tau_p / |x_q - x_p|)).
// mode CLIP_FIXED: tau_p = tau. mode CLIP_ADAPTIVE: the min(b, |N_p|) farthest neighbours F_p (a
// non-finite distance counts as +inf, here and in the sum below; among equals the higher row is
// farther) are set aside and tau_p^2 = sum_{N_p \ F_p} w[p][q] D_pq / sum_{F_p} w[p][q]; b == 0:
// tau_p = +inf (plain mixing), F_p == N_p: tau_p = 0. A neighbour at a non-finite distance gets
// w_eff 0, and rows of w_eff 0 never enter a sum: a NaN row reaches nobody and is itself left as it
// is; a row p whose w[p][.] is all zero is a source only and is never written. Distances as
// fl_krum_select's, on the same grid (work holds the same floats). Device outputs dist[K*K],
// tau[K] (double) and w_eff[K*K] (float). Three launches (none for K == 1); every thread loads its
// coordinates of all rows before it stores, so the update is in-place safe.
#define CLIP_FIXED 0
#define CLIP_ADAPTIVE 1
struct ClipPlan {
  float w[16][16];
  double tau;
  int mode;
  int b;
};
void fl_clipped_gossip(float* work, const OutPtrs& rows, int K, const ClipPlan& plan, int64_t n, double* dist, double* tau, float* w_eff,
                       hipStream_t s);
// Colluding attacks: one crafted row m from the K honest rows 0..K-1, stored into out rows 0..P-1
// (which are not among the rows). kind: 0 ALIE, 1 IPM, 2 min-max, 3 min-sum. m = ca·μ + cb·σ + cr·ref
// per coordinate (μ, σ: mean and population standard deviation of the honest values). ALIE and IPM
// take (ca, cb, cr) from the host: one launch, which also records z (−cb) or ε (−ca) in gamma[0].
// min-max / min-sum: four launches (Krum's distances, the statistics a_i = |μ − x_i|²,
// b_i = <μ − x_i, σ>, s = |σ|², one block that solves for γ, the write with cb = −γ read from device
// memory); device outputs gamma[1] (float) and stat[2K+3] (double: a, b, s, D, S). work holds
// fl_collude_work(n, K) floats; the grids are fl_krum_grid(n, K). ref may be null unless kind is IPM.
inline int64_t fl_collude_work(int64_t n, int K) { return (int64_t)fl_krum_grid(n, K) * (K * (K - 1) / 2 + 2 * K + 1); }
void fl_collude(float* work, const OutPtrs& outs, int P, const RowPtrs& rows, int K, int kind, float ca, float cb, float cr, const float* ref,
                int64_t n, float* gamma, double* stat, hipStream_t s);
// SCAFFOLD server step, packed buffer [Σ w_k dy_k | Σ w_k | Σ dc_k | K] (2n + 2 floats):
//   reduce: buf <- the local contributions (before the cross-rank all-reduce)
//   apply : out rows <- x_start + glr · buf[0:n] / buf[n];  c <- (c_init ? 0 : c) + buf[n+1:2n+1] / buf[2n+1]
void fl_scaffold_reduce(float* buf, const RowPtrs& dy, const RowPtrs& dc, const RowW& w, int K, int64_t n, hipStream_t s);
void fl_scaffold_apply(const OutPtrs& outs, int P, const float* x_start, const float* buf, float* c, int c_init, float glr, int64_t n, hipStream_t s);
void fl_opt_step(float* param, const float* grad, float* m, float* v, bf16* shadow, int64_t n, const OptParams& o, int step, const float* anchor,
                 const float* cg, const float* cl, hipStream_t s);
void fl_scale_add_noise(float* t, int64_t n, float scale, float sigma, uint64_t seed, hipStream_t s);
