// Federated-learning elementwise/reduction kernels (gfx950): FedAvg reductions, fused optimizers,
// coordinate median, attack injection. All memory-bound: 16-byte vector accesses, grid-stride,
// grid capped at 2048 blocks (cdna_hip_programming.md Guideline 11/13).
#include <type_traits>
#include <utility>
#include "common.h"
#include "fl_ops.h"

#define FL_BLOCK 256

static inline unsigned grid_for(int64_t n_vec) {
  int64_t g = (n_vec + FL_BLOCK - 1) / FL_BLOCK;
  if (g > 2048) g = 2048;
  if (g < 1) g = 1;
  return (unsigned)g;
}

// Vector paths. A kernel below takes its 16-byte (float4) path only when its launcher found the row
// stride a multiple of 4 floats and every base pointer 16-byte aligned (vec_ok); otherwise the
// scalar path covers every element. Both paths add the rows in the same order with the same
// arithmetic, so a result does not depend on where its buffers lie. The decision is made once per
// launch on the host.
template <typename... Ptr>
static inline bool vec_ok(int64_t ld, Ptr... ptrs) {
  uintptr_t bits = 0;
  ((bits |= reinterpret_cast<uintptr_t>(ptrs)), ...);
  return (ld % 4) == 0 && (bits & 15u) == 0;
}

// out[i] = Σ_k w[k] · src_k[i]   (src pointers in a device array; the caller, who holds them,
// says whether they are all 16-byte aligned). Rows of weight 0 are never read.
template <bool VEC>
__global__ __launch_bounds__(FL_BLOCK) void k_weighted_sum(float* __restrict__ out, const uint64_t* __restrict__ srcs, const float* __restrict__ w, int K,
                                                            int64_t n) {
  const int64_t n4 = VEC ? n / 4 : 0;
  const int64_t stride = (int64_t)gridDim.x * FL_BLOCK;
  for (int64_t i = blockIdx.x * FL_BLOCK + threadIdx.x; i < n4; i += stride) {
    float4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < K; ++k) {
      const float wk = w[k];
      if (wk == 0.f) continue;
      const float4 v = reinterpret_cast<const float4*>(srcs[k])[i];
      acc.x += wk * v.x; acc.y += wk * v.y; acc.z += wk * v.z; acc.w += wk * v.w;
    }
    reinterpret_cast<float4*>(out)[i] = acc;
  }
  for (int64_t i = n4 * 4 + blockIdx.x * FL_BLOCK + threadIdx.x; i < n; i += stride) {
    float acc = 0.f;
    for (int k = 0; k < K; ++k)
      if (w[k] != 0.f) acc += w[k] * reinterpret_cast<const float*>(srcs[k])[i];
    out[i] = acc;
  }
}

// out[i] = scale · Σ_p w[p] · stacked[p*ld + i]   (co-located peers, [P][ld] buffer). Rows of
// weight 0 are never read (peers that did not train may hold anything).
__global__ __launch_bounds__(FL_BLOCK) void k_stacked_weighted_sum(float* __restrict__ out, const float* __restrict__ stacked, int P, int64_t n, int64_t ld,
                                                                    const float* __restrict__ w, float scale, bool vec) {
  const int64_t n4 = n / 4;
  const int64_t stride = (int64_t)gridDim.x * FL_BLOCK;
  if (vec) {
    for (int64_t i = blockIdx.x * FL_BLOCK + threadIdx.x; i < n4; i += stride) {
      float4 acc = {0.f, 0.f, 0.f, 0.f};
      for (int p = 0; p < P; ++p) {
        const float wp = w[p];
        if (wp == 0.f) continue;
        const float4 v = reinterpret_cast<const float4*>(stacked + p * ld)[i];
        acc.x += wp * v.x; acc.y += wp * v.y; acc.z += wp * v.z; acc.w += wp * v.w;
      }
      acc.x *= scale; acc.y *= scale; acc.z *= scale; acc.w *= scale;
      reinterpret_cast<float4*>(out)[i] = acc;
    }
  }
  for (int64_t i = (vec ? n4 * 4 : 0) + blockIdx.x * FL_BLOCK + threadIdx.x; i < n; i += stride) {
    float acc = 0.f;
    for (int p = 0; p < P; ++p)
      if (w[p] != 0.f) acc += w[p] * stacked[p * ld + i];
    out[i] = acc * scale;
  }
}

// stacked[p*ld + i] = src[i] for rows with mask[p] != 0 (mask null = all rows)
__global__ __launch_bounds__(FL_BLOCK) void k_broadcast_rows(float* __restrict__ stacked, const float* __restrict__ src, int P, int64_t n, int64_t ld,
                                                              const float* __restrict__ mask, bool vec) {
  const int p = blockIdx.y;
  if (mask != nullptr && mask[p] == 0.f) return;
  const int64_t stride = (int64_t)gridDim.x * FL_BLOCK;
  float* dst = stacked + p * ld;
  if (vec) {
    const int64_t n4 = n / 4;
    for (int64_t i = blockIdx.x * FL_BLOCK + threadIdx.x; i < n4; i += stride)
      reinterpret_cast<float4*>(dst)[i] = reinterpret_cast<const float4*>(src)[i];
    for (int64_t i = n4 * 4 + blockIdx.x * FL_BLOCK + threadIdx.x; i < n; i += stride) dst[i] = src[i];
  } else {
    for (int64_t i = blockIdx.x * FL_BLOCK + threadIdx.x; i < n; i += stride) dst[i] = src[i];
  }
}

// FedAvg over a stacked [P][ld] group with the per-peer weights / mask passed BY VALUE (kernel
// arguments): no host→device copy, nothing for the host to wait on.
//   reduce: out[i] = Σ_p w[p] · stacked[p*ld + i] (i < n), *wsum_slot = wsum (when non-null)
//   apply:  stacked[p*ld + i] = out[i] / max(*wsum_slot, 1e-12) for rows with mask bit p set
// A bucketed all-reduce calls them per bucket (sub-ranges of out / stacked, bucket 0 carries the
// weight sum in a slot in front of the data, so bucket k's apply only waits for buckets 0 and k).
// out2 / wsum2 (nullable): a second copy of the partial sums (the failover's retained input), written
// by the same pass instead of a separate device copy behind it
__global__ __launch_bounds__(FL_BLOCK) void k_fedavg_reduce(float* __restrict__ out, float* __restrict__ wsum_slot, const float* __restrict__ stacked,
                                                             int P, int64_t n, int64_t ld, FedAvgWeights w, float* __restrict__ out2,
                                                             float* __restrict__ wsum2, bool vec) {
  const int64_t stride = (int64_t)gridDim.x * FL_BLOCK;
  const int64_t t0 = blockIdx.x * FL_BLOCK + threadIdx.x;
  if (t0 == 0 && wsum_slot != nullptr) *wsum_slot = w.wsum;
  if (t0 == 0 && wsum2 != nullptr) *wsum2 = w.wsum;
  if (vec) {
    const int64_t n4 = n / 4;
    for (int64_t i = t0; i < n4; i += stride) {
      float4 acc = {0.f, 0.f, 0.f, 0.f};
      for (int p = 0; p < P; ++p) {
        const float wp = w.w[p];
        if (wp == 0.f) continue;
        const float4 v = reinterpret_cast<const float4*>(stacked + p * ld)[i];
        acc.x += wp * v.x; acc.y += wp * v.y; acc.z += wp * v.z; acc.w += wp * v.w;
      }
      reinterpret_cast<float4*>(out)[i] = acc;
      if (out2 != nullptr) reinterpret_cast<float4*>(out2)[i] = acc;
    }
    for (int64_t i = n4 * 4 + t0; i < n; i += stride) {
      float acc = 0.f;
      for (int p = 0; p < P; ++p)
        if (w.w[p] != 0.f) acc += w.w[p] * stacked[p * ld + i];  // rows of weight 0 are never read (may be uninitialised)
      out[i] = acc;
      if (out2 != nullptr) out2[i] = acc;
    }
  } else {
    for (int64_t i = t0; i < n; i += stride) {
      float acc = 0.f;
      for (int p = 0; p < P; ++p)
        if (w.w[p] != 0.f) acc += w.w[p] * stacked[p * ld + i];  // rows of weight 0 are never read (may be uninitialised)
      out[i] = acc;
      if (out2 != nullptr) out2[i] = acc;
    }
  }
}

__global__ __launch_bounds__(FL_BLOCK) void k_fedavg_apply(float* __restrict__ stacked, const float* __restrict__ out, const float* __restrict__ wsum_slot,
                                                            int P, int64_t n, int64_t ld, unsigned long long mask, bool vec) {
  const int p = blockIdx.y;
  if (!((mask >> p) & 1ull)) return;
  const float inv = 1.f / fmaxf(*wsum_slot, 1e-12f);
  const int64_t stride = (int64_t)gridDim.x * FL_BLOCK;
  float* dst = stacked + p * ld;
  if (vec) {
    const int64_t n4 = n / 4;
    for (int64_t i = blockIdx.x * FL_BLOCK + threadIdx.x; i < n4; i += stride) {
      float4 v = reinterpret_cast<const float4*>(out)[i];
      v.x *= inv; v.y *= inv; v.z *= inv; v.w *= inv;
      reinterpret_cast<float4*>(dst)[i] = v;
    }
    for (int64_t i = n4 * 4 + blockIdx.x * FL_BLOCK + threadIdx.x; i < n; i += stride) dst[i] = out[i] * inv;
  } else {
    for (int64_t i = blockIdx.x * FL_BLOCK + threadIdx.x; i < n; i += stride) dst[i] = out[i] * inv;
  }
}

// Single-rank FedAvg (no all-reduce between reduce and apply): each thread forms the weighted mean
// of its coordinates over the rows and writes it into every masked row — one launch instead of two.
__global__ __launch_bounds__(FL_BLOCK) void k_fedavg_local(float* __restrict__ stacked, int P, int64_t n, int64_t ld, FedAvgWeights w,
                                                           unsigned long long mask, bool vec) {
  const int64_t stride = (int64_t)gridDim.x * FL_BLOCK;
  const float inv = 1.f / fmaxf(w.wsum, 1e-12f);
  if (vec) {
    const int64_t n4 = n / 4;
    for (int64_t i = blockIdx.x * FL_BLOCK + threadIdx.x; i < n4; i += stride) {
      float4 acc = {0.f, 0.f, 0.f, 0.f};
      for (int p = 0; p < P; ++p) {
        const float wp = w.w[p];
        if (wp == 0.f) continue;
        const float4 v = reinterpret_cast<const float4*>(stacked + p * ld)[i];
        acc.x += wp * v.x; acc.y += wp * v.y; acc.z += wp * v.z; acc.w += wp * v.w;
      }
      acc.x *= inv; acc.y *= inv; acc.z *= inv; acc.w *= inv;
      for (int p = 0; p < P; ++p)
        if ((mask >> p) & 1ull) reinterpret_cast<float4*>(stacked + p * ld)[i] = acc;
    }
    for (int64_t i = n4 * 4 + blockIdx.x * FL_BLOCK + threadIdx.x; i < n; i += stride) {
      float acc = 0.f;
      for (int p = 0; p < P; ++p)
        if (w.w[p] != 0.f) acc += w.w[p] * stacked[p * ld + i];  // rows of weight 0 are never read (may be uninitialised)
      for (int p = 0; p < P; ++p)
        if ((mask >> p) & 1ull) stacked[p * ld + i] = acc * inv;
    }
  } else {
    for (int64_t i = blockIdx.x * FL_BLOCK + threadIdx.x; i < n; i += stride) {
      float acc = 0.f;
      for (int p = 0; p < P; ++p)
        if (w.w[p] != 0.f) acc += w.w[p] * stacked[p * ld + i];  // rows of weight 0 are never read (may be uninitialised)
      for (int p = 0; p < P; ++p)
        if ((mask >> p) & 1ull) stacked[p * ld + i] = acc * inv;
    }
  }
}

void fl_fedavg_local(float* stacked, int P, int64_t n, int64_t ld, const FedAvgWeights& w, unsigned long long mask, hipStream_t s) {
  hipLaunchKernelGGL(k_fedavg_local, dim3(grid_for((n + 3) / 4)), dim3(FL_BLOCK), 0, s, stacked, P, n, ld, w, mask, vec_ok(ld, stacked));
}

void fl_fedavg_reduce(float* out, float* wsum_slot, const float* stacked, int P, int64_t n, int64_t ld, const FedAvgWeights& w, hipStream_t s,
                      float* out2, float* wsum2) {
  hipLaunchKernelGGL(k_fedavg_reduce, dim3(grid_for((n + 3) / 4)), dim3(FL_BLOCK), 0, s, out, wsum_slot, stacked, P, n, ld, w, out2, wsum2,
                     vec_ok(ld, out, out2, stacked));
}

void fl_fedavg_apply(float* stacked, const float* out, const float* wsum_slot, int P, int64_t n, int64_t ld, unsigned long long mask, hipStream_t s) {
  unsigned gx = grid_for((n + 3) / 4);
  if (gx > 256) gx = 256;
  hipLaunchKernelGGL(k_fedavg_apply, dim3(gx, P), dim3(FL_BLOCK), 0, s, stacked, out, wsum_slot, P, n, ld, mask, vec_ok(ld, stacked, out));
}

// Delayed averaging (opt-in): land the previous round's average as a correction and take the new
// snapshot in one pass, for every row with mask bit p set:
//   x = stacked[p][i] + avg[i] / wsum - snap[p][i];  stacked[p][i] = x;  snap[p][i] = x
// With avg == nullptr (nothing pending) it only snapshots.
__global__ __launch_bounds__(FL_BLOCK) void k_fedavg_delayed_land(float* __restrict__ stacked, float* __restrict__ snap, int64_t ld_snap,
                                                                   const float* __restrict__ avg, const float* __restrict__ wsum_slot, int P, int64_t n,
                                                                   int64_t ld, unsigned long long mask) {
  const int p = blockIdx.y;
  if (!((mask >> p) & 1ull)) return;
  const float inv = avg != nullptr ? 1.f / fmaxf(*wsum_slot, 1e-12f) : 0.f;
  float* x = stacked + p * ld;
  float* sp = snap + p * ld_snap;
  const int64_t stride = (int64_t)gridDim.x * FL_BLOCK;
  for (int64_t i = blockIdx.x * FL_BLOCK + threadIdx.x; i < n; i += stride) {
    float v = x[i];
    if (avg != nullptr) {
      v = v + (avg[i] * inv - sp[i]);
      x[i] = v;
    }
    sp[i] = v;
  }
}

void fl_fedavg_delayed_land(float* stacked, float* snap, int64_t ld_snap, const float* avg, const float* wsum_slot, int P, int64_t n, int64_t ld,
                            unsigned long long mask, hipStream_t s) {
  unsigned gx = grid_for(n);
  if (gx > 512) gx = 512;
  hipLaunchKernelGGL(k_fedavg_delayed_land, dim3(gx, P), dim3(FL_BLOCK), 0, s, stacked, snap, ld_snap, avg, wsum_slot, P, n, ld, mask);
}

// Gossip neighbour averaging of co-located peers (reference: aggregator over the neighbours'
// models, p2pfl/learning/aggregators/fedavg.py driven by gossip_weights). One thread owns a float4
// column of every row: it loads all P rows into registers, then writes each row's mixture back, so
// the in-place update never reads a row another thread has already written.
template <int P>
__global__ __launch_bounds__(FL_BLOCK) void k_neighbor_mix(float* __restrict__ stacked, int64_t n4, int64_t ld, MixPlan m) {
  const int64_t stride = (int64_t)gridDim.x * FL_BLOCK;
  for (int64_t i = blockIdx.x * FL_BLOCK + threadIdx.x; i < n4; i += stride) {
    float4 v[P];
#pragma unroll
    for (int p = 0; p < P; ++p) v[p] = reinterpret_cast<const float4*>(stacked + p * ld)[i];
#pragma unroll
    for (int p = 0; p < P; ++p) {
      const int ns = m.nsrc[p];
      if (ns == 0) continue;
      float4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int k = 0; k < MIX_MAX_SRC; ++k) {
        if (k >= ns) break;
        const float wk = m.w[p][k];
        float4 s = v[0];
        // register-array select (a dynamic index would spill v to scratch)
#pragma unroll
        for (int q = 0; q < P; ++q)
          if (q == m.idx[p][k]) s = v[q];
        acc.x += wk * s.x; acc.y += wk * s.y; acc.z += wk * s.z; acc.w += wk * s.w;
      }
      reinterpret_cast<float4*>(stacked + p * ld)[i] = acc;
    }
  }
}

void fl_neighbor_mix(float* stacked, int P, int64_t n, int64_t ld, const MixPlan& m, hipStream_t s) {
  // rows are padded to ld (a multiple of 4); mixing the padding too keeps every access a float4
  const int64_t n4 = (n + 3) / 4;
  const dim3 g(grid_for(n4)), b(FL_BLOCK);
  switch (P) {
#define MIX_CASE(K) \
  case K: hipLaunchKernelGGL(k_neighbor_mix<K>, g, b, 0, s, stacked, n4, ld, m); break;
    MIX_CASE(1) MIX_CASE(2) MIX_CASE(3) MIX_CASE(4) MIX_CASE(5) MIX_CASE(6) MIX_CASE(7) MIX_CASE(8)
    MIX_CASE(9) MIX_CASE(10) MIX_CASE(11) MIX_CASE(12) MIX_CASE(13) MIX_CASE(14) MIX_CASE(15) MIX_CASE(16)
#undef MIX_CASE
    default: break;
  }
}

// The per-coordinate sorts below order their values as
//   −inf < … < −0.0 < +0.0 < … < +inf < NaN:
// a NaN (a peer that sent one) is the largest value, as in numpy's and torch's sort, never a vote for
// its neighbour (fminf / fmaxf would drop it and duplicate the other operand). The network runs on a
// monotone integer key of the float's bits (a negative float's magnitude bits inverted; every NaN
// the quiet 0x7fc00000, above +inf) with integer min / max, and maps back: a non-NaN value comes
// out bit for bit.
__device__ __forceinline__ int sort_key(float v) {
  const int b = v != v ? 0x7fc00000 : __float_as_int(v);
  return b ^ ((b >> 31) & 0x7fffffff);
}
__device__ __forceinline__ float sort_value(int key) { return __int_as_float(key ^ ((key >> 31) & 0x7fffffff)); }

// branch-free compare-exchange network over K registers: v ascending
template <int K>
__device__ __forceinline__ void sort_keys(int (&v)[K]) {
#pragma unroll
  for (int a = 0; a < K; ++a) {
#pragma unroll
    for (int b = 0; b < K - 1 - a; ++b) {
      const int lo = min(v[b], v[b + 1]);
      v[b + 1] = max(v[b], v[b + 1]);
      v[b] = lo;
    }
  }
}

// per-coordinate median of K ≤ 16 models: the network above over K registers, the result stored
// into P destination rows (every peer that takes the aggregate). Row pointers travel as kernel
// arguments (no pointer table on the device, no H2D copy); each thread loads its coordinate from
// every row before storing, so destinations may alias sources. A NaN among the middle values makes
// the output NaN.
template <int K>
__global__ __launch_bounds__(FL_BLOCK) void k_coordinate_median(OutPtrs outs, int P, RowPtrs rows, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * FL_BLOCK;
  for (int64_t i = blockIdx.x * FL_BLOCK + threadIdx.x; i < n; i += stride) {
    int v[K];
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = sort_key(rows.p[k][i]);
    sort_keys<K>(v);
    const float med = (K & 1) ? sort_value(v[(K - 1) / 2]) : 0.5f * (sort_value(v[K / 2 - 1]) + sort_value(v[K / 2]));
    for (int p = 0; p < P; ++p) outs.p[p][i] = med;
  }
}

// per-coordinate trimmed mean of K ≤ 16 models: the median's compare-exchange network, then the
// kept values v[t .. K-t) summed in ascending order in fp32 and divided by K-2t (0 ≤ 2t < K, a
// run-time argument); a NaN among the kept values makes the output NaN. Loads every row's coordinate
// before any store: destinations may alias sources.
template <int K>
__global__ __launch_bounds__(FL_BLOCK) void k_trimmed_mean(OutPtrs outs, int P, RowPtrs rows, int t, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * FL_BLOCK;
  const float cnt = (float)(K - 2 * t);
  for (int64_t i = blockIdx.x * FL_BLOCK + threadIdx.x; i < n; i += stride) {
    int v[K];
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = sort_key(rows.p[k][i]);
    sort_keys<K>(v);
    float s = 0.f;
    // static register indices (a dynamic v[t + k] would put v in scratch)
#pragma unroll
    for (int k = 0; k < K; ++k)
      if (k >= t && k < K - t) s += sort_value(v[k]);
    const float mean = s / cnt;
    for (int p = 0; p < P; ++p) outs.p[p][i] = mean;
  }
}

// (Multi-)Krum (Blanchard et al., 2017) in three launches, no cross-block synchronisation inside a
// launch and no float atomics:
//   k_pairwise_sqdist<K>: per block the K(K-1)/2 partial sums Σ (x_i − x_j)² of its coordinates,
//                         stored into the block's slab of work[grid][K(K-1)/2]
//   k_krum_select       : one block sums the slabs in a fixed order (double), scores every row,
//                         selects, and writes dist / score / coef to device memory
//   k_coef_mean<K>      : out rows <- Σ_k coef[k] · row_k, coef read from device memory
// The distances come from differences: peers start a round from the same model, so rows differ
// by ~1e-3 of their norm and |x_i|² + |x_j|² − 2 x_i·x_j has no correct digit in fp32.

// Four consecutive coordinates 4g .. 4g+3 of a row. Rows are only guaranteed 4-byte aligned (row i
// of a packed [k, n] buffer with odd n): the float4 access is taken only when the launcher found
// every pointer 16-byte aligned. Both forms feed identical arithmetic, so a result does not depend
// on where its rows happen to lie. Coordinates past n read as 0.
template <bool VEC>
__device__ __forceinline__ float4 load4(const float* p, int64_t g, int64_t n) {
  const int64_t i = 4 * g;
  if (VEC && i + 4 <= n) return reinterpret_cast<const float4*>(p)[g];
  float4 v;
  v.x = i < n ? p[i] : 0.f;
  v.y = i + 1 < n ? p[i + 1] : 0.f;
  v.z = i + 2 < n ? p[i + 2] : 0.f;
  v.w = i + 3 < n ? p[i + 3] : 0.f;
  return v;
}

template <bool VEC>
__device__ __forceinline__ void store4(float* p, int64_t g, int64_t n, const float4& v) {
  const int64_t i = 4 * g;
  if (VEC && i + 4 <= n) {
    reinterpret_cast<float4*>(p)[g] = v;
    return;
  }
  if (i < n) p[i] = v.x;
  if (i + 1 < n) p[i + 1] = v.y;
  if (i + 2 < n) p[i + 2] = v.z;
  if (i + 3 < n) p[i + 3] = v.w;
}

#define KRUM_WAVES (FL_BLOCK / 64)

// Grid of k_pairwise_sqdist: a function of n and K only, so every rank reduces the identical
// gathered buffer in the identical order and selects the same peers, bit for bit.
// At most KRUM_MAX_GRID blocks (two per CU): K = 16 runs two waves per SIMD anyway, eight float4
// loads in flight per thread keep HBM busy at that occupancy, and k_krum_select sums every slab.
#define KRUM_MAX_GRID 512
unsigned fl_krum_grid(int64_t n, int K) {
  (void)K;
  const unsigned g = grid_for((n + 3) / 4);
  return g > KRUM_MAX_GRID ? KRUM_MAX_GRID : g;
}

// The rows' coordinates 4g .. 4g+3 by one decision for all K rows, so that the K vector loads are
// issued back to back (a branch per row, as load4<VEC> per row has, makes each load wait for the one
// before). Which of the two forms a kernel uses was tuned per kernel.
template <int K, bool VEC>
__device__ __forceinline__ void load4_rows(float4 (&v)[K], const RowPtrs& rows, int64_t g, int64_t n) {
  if (VEC && 4 * g + 4 <= n) {
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = reinterpret_cast<const float4*>(rows.p[k])[g];
  } else {
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = load4<false>(rows.p[k], g, n);
  }
}

// A block's W per-thread partial sums to its slab slab[0 .. W): wave reduction (xor butterfly: a
// fixed order), then the block's waves through LDS in wave order. Every block stores its whole slab
// (zeros included): the one-block kernels sum every slab and the workspace is never cleared. Every
// thread of the block calls it, once.
template <int W>
__device__ __forceinline__ void store_slab(float (&acc)[W], float* __restrict__ slab) {
  __shared__ float part[KRUM_WAVES][W];
#pragma unroll
  for (int q = 0; q < W; ++q) {
    float s = acc[q];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
    acc[q] = s;
  }
  const int wave = threadIdx.x / 64;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int q = 0; q < W; ++q) part[wave][q] = acc[q];
  }
  __syncthreads();
  if (threadIdx.x < W) {
    float s = part[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < KRUM_WAVES; ++w) s += part[w][threadIdx.x];
    slab[threadIdx.x] = s;
  }
}

// Group g of every row (load4<VEC> per row), then acc[q] += Σ over the four coordinates of
// (x_i − x_j)², pair q = (i, j), i < j, i ascending and then j. The one loop body of
// k_pairwise_sqdist and k_dnc_sqdist: their slabs agree bit for bit.
// Which of d·d + d·d becomes a fused multiply-add is the compiler's choice under the default
// -ffp-contract, per instantiation: that the VEC and the scalar form of a kernel round alike rests on
// it making the same choice in both. tests/test_robust_dispatch_gpu.py compares the two forms at
// every K and is what guards it.
template <int K, bool VEC>
__device__ __forceinline__ void pair_sqdist_add(const RowPtrs& rows, int64_t g, int64_t n, float (&acc)[K * (K - 1) / 2]) {
  float4 v[K];
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = load4<VEC>(rows.p[k], g, n);
  int q = 0;
#pragma unroll
  for (int i = 0; i < K; ++i) {
#pragma unroll
    for (int j = i + 1; j < K; ++j) {
      const float dx = v[i].x - v[j].x, dy = v[i].y - v[j].y, dz = v[i].z - v[j].z, dw = v[i].w - v[j].w;
      acc[q] += (dx * dx + dy * dy) + (dz * dz + dw * dw);
      ++q;
    }
  }
}

template <int K, bool VEC>
__global__ __launch_bounds__(FL_BLOCK) void k_pairwise_sqdist(float* __restrict__ work, RowPtrs rows, int64_t n) {
  constexpr int NP = K * (K - 1) / 2;
  float acc[NP];
#pragma unroll
  for (int q = 0; q < NP; ++q) acc[q] = 0.f;
  const int64_t groups = (n + 3) / 4;
  const int64_t stride = (int64_t)gridDim.x * FL_BLOCK;
  for (int64_t g = (int64_t)blockIdx.x * FL_BLOCK + threadIdx.x; g < groups; g += stride) {
    pair_sqdist_add<K, VEC>(rows, g, n, acc);
  }
  store_slab<NP>(acc, work + (int64_t)blockIdx.x * NP);
}

// The slab sum of every one-block kernel below: column t of work[G][W] for thread t < W (0 for the
// others), in double, in a fixed two-level order: the block's threads split the slabs into
// C = KRUM_SELECT_BLOCK / W chunks of consecutive slabs, each summed in slab order (eight loads in
// flight), then the chunks in chunk order. The order depends on G and W only, so every rank sums the
// identical gathered buffer to the identical bits and selects the same peers. W <= 120 (at least 8
// chunks); W == 0 sums nothing. One barrier inside; every thread of the block calls it.
#define KRUM_SELECT_BLOCK 1024
__device__ __forceinline__ double sum_slabs(const float* __restrict__ work, int G, int W, double* part) {
  const int t = threadIdx.x;
  const int C = W > 0 ? KRUM_SELECT_BLOCK / W : 0;
  if (t < C * W) {
    const int p = t % W, c = t / W;
    const int per = (G + C - 1) / C;
    const int g1 = min(G, (c + 1) * per);
    int g = c * per;
    double s = 0.0;
    for (; g + 8 <= g1; g += 8) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = work[(int64_t)(g + u) * W + p];
#pragma unroll
      for (int u = 0; u < 8; ++u) s += (double)v[u];
    }
    for (; g < g1; ++g) s += (double)work[(int64_t)g * W + p];
    part[c * W + p] = s;
  }
  __syncthreads();
  double s = 0.0;
  if (t < W)
    for (int c = 0; c < C; ++c) s += part[c * W + t];
  return s;
}

// The pair slabs of k_pairwise_sqdist summed (sum_slabs, W = K(K-1)/2) into d[i][j] = d[j][i], pair q
// being (i, j), i < j, in the order k_pairwise_sqdist enumerates them; 0 on the diagonal. Ends with a
// barrier; every thread of the block calls it.
__device__ __forceinline__ void krum_sum_slabs(const float* __restrict__ work, int G, int K, double (*d)[16], double* part) {
  const int t = threadIdx.x;
  const int NP = K * (K - 1) / 2;
  if (t < 256) (&d[0][0])[t] = 0.0;
  const double s = sum_slabs(work, G, NP, part);
  if (t < NP) {
    int i = 0, rem = t;
    while (rem >= K - 1 - i) {
      rem -= K - 1 - i;
      ++i;
    }
    const int j = i + 1 + rem;
    d[i][j] = s;
    d[j][i] = s;
  }
  __syncthreads();
}

// Row t's score: its cnt smallest distances to the rows whose bit in taken is clear, summed in
// ascending order (the lower index first among equals, a NaN as +inf).
__device__ __forceinline__ double krum_row_score(double (*d)[16], int t, int K, int cnt, unsigned taken) {
  double s = 0.0;
  for (int c = 0; c < cnt; ++c) {
    int best = -1;
    double bk = 0.0;
    for (int j = 0; j < K; ++j) {
      if ((taken >> j) & 1u) continue;
      const double key = d[t][j] != d[t][j] ? __builtin_huge_val() : d[t][j];
      if (best < 0 || key < bk) {
        best = j;
        bk = key;
      }
    }
    taken |= 1u << best;
    s += d[t][best];
  }
  return s;
}

// One block: the distances by krum_sum_slabs, then per row the
// neighbours = min(max(1, K−f−2), K−1) smallest off-diagonal distances; the
// max(1, min(m, K)) lowest scores are chosen, the lower index winning a tie; a NaN (a peer that
// sent one) orders last, as numpy's sort does. coef[i] = w_i / Σ_chosen w, 0 for the others.
__global__ __launch_bounds__(KRUM_SELECT_BLOCK) void k_krum_select(const float* __restrict__ work, int G, int K, int f, int m, RowW w,
                                                                   double* __restrict__ dist, double* __restrict__ score, float* __restrict__ coef) {
  __shared__ double d[16][16];
  __shared__ double sc[16];
  __shared__ int chosen[16];
  __shared__ double part[KRUM_SELECT_BLOCK];
  const int t = threadIdx.x;
  krum_sum_slabs(work, G, K, d, part);
  for (int q = t; q < K * K; q += KRUM_SELECT_BLOCK) dist[q] = d[q / K][q % K];
  if (t < K) {
    int cnt = K - f - 2;
    if (cnt < 1) cnt = 1;
    if (cnt > K - 1) cnt = K - 1;
    const double s = krum_row_score(d, t, K, cnt, 1u << t);
    sc[t] = s;
    score[t] = s;
  }
  __syncthreads();
  if (t < K) {
    int want = m < K ? m : K;
    if (want < 1) want = 1;
    const double mine = sc[t] != sc[t] ? __builtin_huge_val() : sc[t];
    int rank = 0;
    for (int j = 0; j < K; ++j) {
      const double other = sc[j] != sc[j] ? __builtin_huge_val() : sc[j];
      if (other < mine || (other == mine && j < t)) ++rank;
    }
    chosen[t] = rank < want ? 1 : 0;
  }
  __syncthreads();
  if (t < K) {
    double ws = 0.0;
    int cnt = 0;
    float wt = 0.f;
    for (int j = 0; j < K; ++j) {
      const float wj = w.w[j];
      if (j == t) wt = wj;
      if (chosen[j]) {
        ws += (double)wj;
        ++cnt;
      }
    }
    // all chosen weights 0 (no sample counts known): plain mean of the chosen rows
    coef[t] = !chosen[t] ? 0.f : (ws > 0.0 ? (float)((double)wt / ws) : 1.f / (float)cnt);
  }
}

// out rows 0..P-1 <- Σ_k coef[k] · row_k, k ascending, fma in fp32; rows of coefficient 0 are never
// read. Every thread loads its coordinates from all rows before it stores: outputs may alias rows.
template <int K, bool VEC>
__global__ __launch_bounds__(FL_BLOCK) void k_coef_mean(OutPtrs outs, int P, RowPtrs rows, const float* __restrict__ coef, int64_t n) {
  float c[K];
#pragma unroll
  for (int k = 0; k < K; ++k) c[k] = coef[k];
  const int64_t groups = (n + 3) / 4;
  const int64_t stride = (int64_t)gridDim.x * FL_BLOCK;
  for (int64_t g = (int64_t)blockIdx.x * FL_BLOCK + threadIdx.x; g < groups; g += stride) {
    float4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if (c[k] == 0.f) continue;
      const float4 v = load4<VEC>(rows.p[k], g, n);
      acc.x = fmaf(c[k], v.x, acc.x); acc.y = fmaf(c[k], v.y, acc.y); acc.z = fmaf(c[k], v.z, acc.z); acc.w = fmaf(c[k], v.w, acc.w);
    }
    for (int p = 0; p < P; ++p) store4<VEC>(outs.p[p], g, n, acc);
  }
}

// ClippedGossip (He, Karimireddy, Jaggi, 2022) in three launches: k_pairwise_sqdist<K> on Krum's
// grid, then
//   k_clip_plan        : one block sums the slabs as k_krum_select does; thread p forms row p's
//                        radius and the clipped weights of its neighbours in double
//   k_clipped_mix<K>   : x_p <- x_p + Σ_q w_eff[p][q] (x_q − x_p) in place
// Row p's neighbours N_p are the q != p with w[p][q] > 0. Adaptive radius: the min(b, |N_p|)
// farthest neighbours F_p are set aside (a non-finite distance counts as +inf, the higher row is
// the farther of two equals) and τ_p² = Σ_{N_p∖F_p} w_pq D_pq / Σ_{F_p} w_pq, both sums in ascending
// q; b == 0: τ_p = +inf, F_p == N_p: τ_p = 0. Scale: 0 at a non-finite distance, 1 where D_pq <= τ_p²,
// else τ_p / sqrt(D_pq); w_eff[p][q] = float(w_pq · scale), rounded once.
__global__ __launch_bounds__(KRUM_SELECT_BLOCK) void k_clip_plan(const float* __restrict__ work, int G, int K, ClipPlan plan,
                                                                 double* __restrict__ dist, double* __restrict__ tau, float* __restrict__ w_eff) {
  __shared__ double d[16][16];
  __shared__ float wsh[16][16];
  __shared__ double part[KRUM_SELECT_BLOCK];
  const int t = threadIdx.x;
  if (t < 256) wsh[t / 16][t % 16] = plan.w[t / 16][t % 16];
  krum_sum_slabs(work, G, K, d, part);  // ends with a barrier: wsh is visible too
  for (int q = t; q < K * K; q += KRUM_SELECT_BLOCK) dist[q] = d[q / K][q % K];
  if (t < K) {
    const double inf = __builtin_huge_val();
    unsigned nb = 0;
    int cnt = 0;
    for (int q = 0; q < K; ++q) {
      if (q != t && wsh[t][q] > 0.f) {
        nb |= 1u << q;
        ++cnt;
      }
    }
    double tp, tp2;
    if (plan.mode == CLIP_FIXED) {
      tp = plan.tau;
      tp2 = tp * tp;
    } else if (plan.b == 0) {
      tp = tp2 = inf;
    } else if (plan.b >= cnt) {
      tp = tp2 = 0.0;
    } else {
      double delta = 0.0, sum = 0.0;
      for (int q = 0; q < K; ++q) {
        if (!((nb >> q) & 1u)) continue;
        const double kq = __builtin_isfinite(d[t][q]) ? d[t][q] : inf;
        int rank = 0;  // neighbours farther than q
        for (int r = 0; r < K; ++r) {
          if (r == q || !((nb >> r) & 1u)) continue;
          const double kr = __builtin_isfinite(d[t][r]) ? d[t][r] : inf;
          if (kr > kq || (kr == kq && r > q)) ++rank;
        }
        if (rank < plan.b) delta += (double)wsh[t][q];
        else sum += (double)wsh[t][q] * kq;
      }
      tp2 = sum / delta;
      tp = sqrt(tp2);
    }
    tau[t] = tp;
    for (int q = 0; q < K; ++q) {
      float e = 0.f;
      const double D = d[t][q];
      if (((nb >> q) & 1u) && __builtin_isfinite(D)) {
        const double scale = D <= tp2 ? 1.0 : tp / sqrt(D);
        e = (float)((double)wsh[t][q] * scale);
      }
      w_eff[t * K + q] = e;
    }
  }
}

// One thread owns four consecutive coordinates of every row: it loads them from all K rows, then
// stores each written row p, so the in-place update never reads a value another thread has
// written. Per coordinate acc <- fma(w_eff[p][q], x_q − x_p, acc) over q ascending from 0, then
// x_p + acc, all in fp32; a q of w_eff 0 never enters the sum (a NaN row reaches nobody) and a row
// whose w_eff are all 0 is not stored. w_eff is wave-uniform: every branch on it is a scalar one,
// and every register index is static.
template <int K, bool VEC>
__global__ __launch_bounds__(FL_BLOCK) void k_clipped_mix(OutPtrs rows, const float* __restrict__ w_eff, int64_t n) {
  const int64_t groups = (n + 3) / 4;
  const int64_t stride = (int64_t)gridDim.x * FL_BLOCK;
  for (int64_t g = (int64_t)blockIdx.x * FL_BLOCK + threadIdx.x; g < groups; g += stride) {
    float4 v[K];
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = load4<VEC>(rows.p[k], g, n);
#pragma unroll
    for (int p = 0; p < K; ++p) {
      float4 acc = {0.f, 0.f, 0.f, 0.f};
      bool any = false;
      // row p's weights are fetched here, K scalars at a time: hoisted out of the loops, the K·K
      // of them would not fit the scalar registers
      const float* wl = w_eff + p * K;
      asm volatile("" : "+s"(wl));
      const __attribute__((address_space(4))) float* wp = (const __attribute__((address_space(4))) float*)wl;
#pragma unroll
      for (int q = 0; q < K; ++q) {
        if (q == p) continue;
        const float e = wp[q];
        if (e == 0.f) continue;
        any = true;
        acc.x = fmaf(e, v[q].x - v[p].x, acc.x); acc.y = fmaf(e, v[q].y - v[p].y, acc.y);
        acc.z = fmaf(e, v[q].z - v[p].z, acc.z); acc.w = fmaf(e, v[q].w - v[p].w, acc.w);
      }
      if (!any) continue;
      const float4 o = {v[p].x + acc.x, v[p].y + acc.y, v[p].z + acc.z, v[p].w + acc.w};
      store4<VEC>(rows.p[p], g, n, o);
    }
  }
}

// Bulyan (El Mhamdi, Guerraoui, Rouault, 2018) in three launches: k_pairwise_sqdist<K> on Krum's
// grid, then
//   k_bulyan_select    : one block sums the slabs as k_krum_select does and picks θ = K − 2f rows by
//                        iterated Krum; writes dist / score / pick / coef (1/θ for a picked row)
//   k_bulyan_mean<K, F>: per coordinate over the picked rows, the mean of the β = K − 4f values
//                        closest to their median
// Iteration it of the selection: every remaining row's score over its clamp(r − f − 2, 1, r − 1)
// nearest remaining rows (r rows remain), the lowest score picked, the lower index winning a tie,
// a NaN ordering as +inf. score[] is the first iteration's: Krum's score for the same f.
__global__ __launch_bounds__(KRUM_SELECT_BLOCK) void k_bulyan_select(const float* __restrict__ work, int G, int K, int f, double* __restrict__ dist,
                                                                     double* __restrict__ score, int* __restrict__ pick, float* __restrict__ coef) {
  __shared__ double d[16][16];
  __shared__ double sc[16];
  __shared__ int picked[16];
  __shared__ unsigned remaining;
  __shared__ double part[KRUM_SELECT_BLOCK];
  const int t = threadIdx.x;
  krum_sum_slabs(work, G, K, d, part);
  for (int q = t; q < K * K; q += KRUM_SELECT_BLOCK) dist[q] = d[q / K][q % K];
  const int theta = K - 2 * f;
  if (t < K) picked[t] = -1;
  if (t == 0) remaining = (1u << K) - 1u;
  __syncthreads();
  for (int it = 0; it < theta; ++it) {
    const unsigned R = remaining;
    const int r = K - it;
    int cnt = r - f - 2;
    if (cnt < 1) cnt = 1;
    if (cnt > r - 1) cnt = r - 1;  // r == 1: no distance, the remaining row is picked
    if (t < K && ((R >> t) & 1u)) {
      const double s = krum_row_score(d, t, K, cnt, ~R | (1u << t));
      sc[t] = s;
      if (it == 0) score[t] = s;
    }
    __syncthreads();
    if (t == 0) {
      int best = -1;
      double bk = 0.0;
      for (int j = 0; j < K; ++j) {
        if (!((R >> j) & 1u)) continue;
        const double key = sc[j] != sc[j] ? __builtin_huge_val() : sc[j];
        if (best < 0 || key < bk) {
          best = j;
          bk = key;
        }
      }
      picked[best] = it;
      remaining = R & ~(1u << best);
    }
    __syncthreads();
  }
  if (t < K) {
    pick[t] = picked[t];
    coef[t] = picked[t] >= 0 ? 1.f / (float)theta : 0.f;
  }
}

// Stage 2 on one coordinate: v[0 .. θ) ascending (the picked rows' values; the slots behind them
// hold +inf). m their median; among the window starts s in [0, 2F] the one that minimises
// max(m − v[s], v[s+β−1] − m), the lowest s winning a tie; the window summed in ascending order and
// divided by β, all in fp32. K and F are template parameters: every index is static.
template <int K, int F>
__device__ __forceinline__ float bulyan_window_mean(const float (&v)[K]) {
  constexpr int TH = K - 2 * F, B = K - 4 * F;
  static_assert(B >= 1, "Bulyan needs K > 4f");
  const float m = (TH & 1) ? v[(TH - 1) / 2] : 0.5f * (v[TH / 2 - 1] + v[TH / 2]);
  float best = fmaxf(m - v[0], v[B - 1] - m);
  float sum = v[0];
#pragma unroll
  for (int k = 1; k < B; ++k) sum += v[k];
#pragma unroll
  for (int s = 1; s <= 2 * F; ++s) {
    const float cost = fmaxf(m - v[s], v[s + B - 1] - m);
    float ws = v[s];
#pragma unroll
    for (int k = 1; k < B; ++k) ws += v[s + k];
    if (cost < best) {
      best = cost;
      sum = ws;
    }
  }
  return sum / (float)B;
}

// Rows of coefficient 0 are never read: their slots hold +inf, so the compare-exchange network (the
// median's) leaves the θ picked values in front. Every thread loads its four coordinates from all
// picked rows before it stores: outputs may alias rows.
template <int K, int F, bool VEC>
__global__ __launch_bounds__(FL_BLOCK) void k_bulyan_mean(OutPtrs outs, int P, RowPtrs rows, const float* __restrict__ coef, int64_t n) {
  bool on[K];
#pragma unroll
  for (int k = 0; k < K; ++k) on[k] = coef[k] != 0.f;
  const float inf = __builtin_huge_valf();
  const int64_t groups = (n + 3) / 4;
  const int64_t stride = (int64_t)gridDim.x * FL_BLOCK;
  for (int64_t g = (int64_t)blockIdx.x * FL_BLOCK + threadIdx.x; g < groups; g += stride) {
    float4 x[K];
#pragma unroll
    for (int k = 0; k < K; ++k) x[k] = {inf, inf, inf, inf};
    // one decision for all K rows (see load4_rows); on[k] is uniform over the grid
    if (VEC && 4 * g + 4 <= n) {
#pragma unroll
      for (int k = 0; k < K; ++k)
        if (on[k]) x[k] = reinterpret_cast<const float4*>(rows.p[k])[g];
    } else {
#pragma unroll
      for (int k = 0; k < K; ++k)
        if (on[k]) x[k] = load4<false>(rows.p[k], g, n);
    }
    float v[4][K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      v[0][k] = x[k].x;
      v[1][k] = x[k].y;
      v[2][k] = x[k].z;
      v[3][k] = x[k].w;
    }
    float o[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
#pragma unroll
      for (int a = 0; a < K; ++a) {
#pragma unroll
        for (int b = 0; b < K - 1 - a; ++b) {
          const float lo = fminf(v[c][b], v[c][b + 1]);
          v[c][b + 1] = fmaxf(v[c][b], v[c][b + 1]);
          v[c][b] = lo;
        }
      }
      o[c] = bulyan_window_mean<K, F>(v[c]);
    }
    const float4 res = {o[0], o[1], o[2], o[3]};
    for (int p = 0; p < P; ++p) store4<VEC>(outs.p[p], g, n, res);
  }
}

// Geometric median (RFA: Pillutla et al., 2019, smoothed Weiszfeld) in 2(T+1)+1 launches, built
// like Krum above: per-block slabs, one block that sums them in double, no float atomics, no
// cross-block synchronisation, nothing for the host to read.
//   k_gm_dist<K>  : per block the K partial sums Σ (x_k − z)² of its coordinates, z = Σ_j c_j x_j,
//                   stored into the block's slab of work[grid][K]
//   k_gm_reweight : one block sums the slabs in a fixed order (double) and, screen: rejects the
//                   rows whose Σ x² is not finite and writes the start coefficients; iterate:
//                   writes dist, obj[t] and the next coefficients β_k / Σβ, β_k = ŵ_k / max(ν, d_k)
//   k_coef_mean<K>: out rows <- Σ_k coef[k] · row_k
// x_k − z is taken as (x_k − x_r) − Σ_j c_j (x_j − x_r), r the lowest row of coefficient != 0: z
// itself is never rounded to fp32. Rows differ by ~1e-3 of their norm (see Krum), so rounding z
// would cost x_k − z its last three digits; the differences from x_r are exact or nearly so.
// With coef == nullptr every coefficient is 0 and x_r is taken as 0: the sums are |x_k|², which is
// the screen pass.
template <int K, bool VEC>
__global__ __launch_bounds__(FL_BLOCK) void k_gm_dist(float* __restrict__ work, RowPtrs rows, const float* __restrict__ coef, int64_t n) {
  float c[K], acc[K];
  int r = -1;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    c[k] = coef != nullptr ? coef[k] : 0.f;
    if (r < 0 && c[k] != 0.f) r = k;
    acc[k] = 0.f;
  }
  const int64_t groups = (n + 3) / 4;
  const int64_t stride = (int64_t)gridDim.x * FL_BLOCK;
  for (int64_t g = (int64_t)blockIdx.x * FL_BLOCK + threadIdx.x; g < groups; g += stride) {
    float4 v[K];
    load4_rows<K, VEC>(v, rows, g, n);
    // the reference row by a wave-uniform predicated copy: v[] stays in registers
    float4 xr = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < K; ++k)
      if (k == r) xr = v[k];
    float4 m = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < K; ++k) {
      v[k].x -= xr.x; v[k].y -= xr.y; v[k].z -= xr.z; v[k].w -= xr.w;
      if (c[k] == 0.f) continue;  // a rejected row may hold NaN
      m.x = fmaf(c[k], v[k].x, m.x); m.y = fmaf(c[k], v[k].y, m.y); m.z = fmaf(c[k], v[k].z, m.z); m.w = fmaf(c[k], v[k].w, m.w);
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const float dx = v[k].x - m.x, dy = v[k].y - m.y, dz = v[k].z - m.z, dw = v[k].w - m.w;
      acc[k] += (dx * dx + dy * dy) + (dz * dz + dw * dw);
    }
  }
  store_slab<K>(acc, work + (int64_t)blockIdx.x * K);
}

// One block. The slabs work[G][K] are summed by sum_slabs; thread 0 then runs the K-term arithmetic
// in double, k ascending. what[K] holds ŵ: the sample weights with
// 0 for a rejected row (all 1 where every valid weight is 0), written by the screen call and read
// by the iterations. No valid row: ŵ = 0 and coef = w / Σw (or 1/K), which every iteration keeps
// (Σβ = 0), so the output is the plain mean and shows the NaN; dist is NaN then.
#define GM_SCREEN 0
#define GM_ITERATE 1
__global__ __launch_bounds__(KRUM_SELECT_BLOCK) void k_gm_reweight(const float* __restrict__ work, int G, int K, int mode, int t, RowW w, double nu,
                                                                   float* __restrict__ what, float* __restrict__ coef, double* __restrict__ dist,
                                                                   double* __restrict__ obj) {
  __shared__ double part[KRUM_SELECT_BLOCK];
  __shared__ double sum[16], d[16], beta[16];
  const int tid = threadIdx.x;
  const double colsum = sum_slabs(work, G, K, part);
  if (tid < K) sum[tid] = colsum;
  __syncthreads();
  if (tid != 0) return;
  if (mode == GM_SCREEN) {
    // a row is valid when its Σ x² is a finite float: NaN, Inf and overflowing rows are out
    unsigned valid = 0;
    double ws = 0.0, wall = 0.0;
    int nvalid = 0;
    for (int k = 0; k < K; ++k) {
      const float s = (float)sum[k];
      wall += (double)w.w[k];
      if (s - s == 0.f) {
        valid |= 1u << k;
        ws += (double)w.w[k];
        ++nvalid;
      }
    }
    for (int k = 0; k < K; ++k) {
      const bool ok = (valid >> k) & 1u;
      if (nvalid == 0) {
        what[k] = 0.f;
        coef[k] = wall > 0.0 ? (float)((double)w.w[k] / wall) : 1.f / (float)K;
      } else {
        const float wk = !ok ? 0.f : (ws > 0.0 ? w.w[k] : 1.f);
        what[k] = wk;
        coef[k] = (float)((double)wk / (ws > 0.0 ? ws : (double)nvalid));
      }
    }
    return;
  }
  double o = 0.0, bs = 0.0;
  bool any = false;
  for (int k = 0; k < K; ++k) {
    const double wk = (double)what[k];
    d[k] = sqrt(sum[k]);
    const bool fin = d[k] - d[k] == 0.0;
    beta[k] = fin ? wk / (d[k] > nu ? d[k] : nu) : 0.0;
    if (wk != 0.0) {
      any = true;
      o += wk * d[k];
    }
    bs += beta[k];
  }
  obj[t] = o;
  for (int k = 0; k < K; ++k) dist[k] = any ? d[k] : __builtin_nan("");
  if (bs > 0.0 && bs - bs == 0.0)
    for (int k = 0; k < K; ++k) coef[k] = (float)(beta[k] / bs);
}

// Colluding omniscient attacks (ALIE: Baruch et al., 2019; IPM: Xie et al., 2019; min-max and
// min-sum: Shejwalkar & Houmansadr, 2021): one crafted row m, computed from the K honest rows and
// stored into the P attackers' rows. Built like Krum and the geometric median above: per-block
// slabs, one block that sums them in double, no float atomics, no cross-block synchronisation,
// nothing for the host to read.
//   k_pairwise_sqdist<K>   : Krum's (min-max / min-sum only: D and S come from it)
//   k_collude_stats<K>     : per block the 2K + 1 partial sums a_0..a_{K-1}, b_0..b_{K-1}, s of its
//                            coordinates, stored into the block's slab of work[grid][2K+1]
//                            (a_i = |μ − x_i|², b_i = <μ − x_i, σ>, s = |σ|²)
//   k_collude_solve        : one block sums both kinds of slabs in a fixed order (double), takes
//                            D = max d_ij or S = max_i Σ_j d_ij and solves for γ; writes gamma / stat
//   k_collude_write<K>     : out rows <- m = ca·μ + cb·σ + cr·r, cb = −γ from device memory
// ALIE and IPM take ca, cb, cr from the host and are the last launch alone.
// There is no NaN screening: a NaN in an honest row reaches σ, γ and m.
//
// One coordinate, in fp32, in exactly this order (x_0..x_{K-1} the honest values):
//   u_k = x_k − x_0                     (u_0 = 0; rows differ by ~1e-3 of their norm, see k_gm_dist)
//   δ   = (((0 + u_0) + u_1) + … + u_{K-1}) / K
//   e_k = u_k − δ                       (μ = x_0 + δ is never rounded to fp32)
//   q   = fma(e_{K-1}, e_{K-1}, … fma(e_1, e_1, fma(e_0, e_0, 0)))
//   σ   = sqrt(q / K)
// e[] holds x on entry and e on return.
template <int K>
__device__ __forceinline__ void collude_coord(float (&e)[K], float& delta, float& sigma) {
  const float x0 = e[0];
  float sum = 0.f;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    e[k] -= x0;
    sum += e[k];
  }
  delta = sum / (float)K;
  float q = 0.f;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    e[k] -= delta;
    q = fmaf(e[k], e[k], q);
  }
  sigma = sqrtf(q / (float)K);
}

// Per thread and coordinate (components x, y, z, w of a group in this order, groups in grid-stride
// order): a_k <- fma(e_k, e_k, a_k), b_k <- fma(−e_k, σ, b_k), s <- fma(σ, σ, s). Coordinates past n
// read as 0 in every row and add 0.
template <int K, bool VEC>
__global__ __launch_bounds__(FL_BLOCK) void k_collude_stats(float* __restrict__ work, RowPtrs rows, int64_t n) {
  constexpr int W = 2 * K + 1;
  float acc[W];
#pragma unroll
  for (int q = 0; q < W; ++q) acc[q] = 0.f;
  const int64_t groups = (n + 3) / 4;
  const int64_t stride = (int64_t)gridDim.x * FL_BLOCK;
  for (int64_t g = (int64_t)blockIdx.x * FL_BLOCK + threadIdx.x; g < groups; g += stride) {
    float4 v[K];
    load4_rows<K, VEC>(v, rows, g, n);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float e[K], delta, sigma;
#pragma unroll
      for (int k = 0; k < K; ++k) e[k] = c == 0 ? v[k].x : c == 1 ? v[k].y : c == 2 ? v[k].z : v[k].w;
      collude_coord<K>(e, delta, sigma);
#pragma unroll
      for (int k = 0; k < K; ++k) {
        acc[k] = fmaf(e[k], e[k], acc[k]);
        acc[K + k] = fmaf(-e[k], sigma, acc[K + k]);
      }
      acc[2 * K] = fmaf(sigma, sigma, acc[2 * K]);
    }
  }
  store_slab<W>(acc, work + (int64_t)blockIdx.x * W);
}

// One block. The pair slabs pairs[Gp][K(K-1)/2] go through krum_sum_slabs, the stats slabs
// stats[G][2K+1] through sum_slabs. Thread 0 then works in double:
//   D = max_ij d_ij, S = max_i Σ_j d_ij (j ascending)
//   min-max: the largest γ >= 0 with max_i |m − x_i|² <= D, m = μ − γσ. |m − x_i|² = a_i − 2γ b_i + γ² s,
//            so γ = min_i (b_i + sqrt(max(0, b_i² + s (D − a_i)))) / s, i ascending
//   min-sum: Σ_i |m − x_i|² = Σ a_i + γ² K s = K s (1 + γ²) <= S, so γ = sqrt(max(0, S / (K s) − 1))
// s = 0 (one honest row, or all equal) gives γ = 0: m = μ. gamma[0] = (float)γ;
// stat = [a_0..a_{K-1}, b_0..b_{K-1}, s, D, S].
#define COLLUDE_ALIE 0
#define COLLUDE_IPM 1
#define COLLUDE_MIN_MAX 2
#define COLLUDE_MIN_SUM 3
__global__ __launch_bounds__(KRUM_SELECT_BLOCK) void k_collude_solve(const float* __restrict__ pairs, int Gp, const float* __restrict__ stats, int G, int K,
                                                                     int kind, float* __restrict__ gamma, double* __restrict__ stat) {
  __shared__ double d[16][16];
  __shared__ double part[KRUM_SELECT_BLOCK];
  __shared__ double sum[33];
  const int tid = threadIdx.x;
  krum_sum_slabs(pairs, Gp, K, d, part);
  const int W = 2 * K + 1;
  const double colsum = sum_slabs(stats, G, W, part);
  if (tid < W) sum[tid] = colsum;
  __syncthreads();
  if (tid != 0) return;
  double D = 0.0, S = 0.0;
  for (int i = 0; i < K; ++i) {
    double row = 0.0;
    for (int j = 0; j < K; ++j) {
      row += d[i][j];
      if (d[i][j] > D) D = d[i][j];
    }
    if (row > S) S = row;
  }
  const double s = sum[2 * K];
  double g = 0.0;
  if (s > 0.0) {
    if (kind == COLLUDE_MIN_MAX) {
      for (int i = 0; i < K; ++i) {
        const double a = sum[i], b = sum[K + i];
        const double disc = b * b + s * (D - a);
        const double gi = (b + sqrt(disc > 0.0 ? disc : 0.0)) / s;
        if (i == 0 || gi < g) g = gi;
      }
      if (g < 0.0) g = 0.0;
    } else {
      const double r = S / ((double)K * s) - 1.0;
      g = sqrt(r > 0.0 ? r : 0.0);
    }
  }
  gamma[0] = (float)g;
  for (int q = 0; q < W; ++q) stat[q] = sum[q];
  stat[W] = D;
  stat[W + 1] = S;
}

// out rows 0..P-1 <- m. Per coordinate δ and σ as k_collude_stats computes them (collude_coord), then
//   cb' = gamma != nullptr ? −gamma[0] : cb
//   t   = fma(cb', σ, ca · δ)
//   m   = fma(ca, x_0, t);  with a reference row r: m = fma(cr, r, m)
// ALIE: (ca, cb, cr) = (1, −z, 0); IPM: (−ε, 0, 1 + ε) with r; min-max / min-sum: (1, ·, 0) and γ
// from device memory. Every thread loads its four coordinates from all rows (and r) before it
// stores. gamma_out != nullptr: thread 0 of the grid records gamma_val there (ALIE's z, IPM's ε).
template <int K, bool VEC>
__global__ __launch_bounds__(FL_BLOCK) void k_collude_write(OutPtrs outs, int P, RowPtrs rows, const float* __restrict__ ref, float ca, float cb, float cr,
                                                            const float* __restrict__ gamma, float* __restrict__ gamma_out, float gamma_val, int64_t n) {
  if (gamma != nullptr) cb = -gamma[0];
  if (gamma_out != nullptr && blockIdx.x == 0 && threadIdx.x == 0) gamma_out[0] = gamma_val;
  const int64_t groups = (n + 3) / 4;
  const int64_t stride = (int64_t)gridDim.x * FL_BLOCK;
  for (int64_t g = (int64_t)blockIdx.x * FL_BLOCK + threadIdx.x; g < groups; g += stride) {
    float4 v[K];
    float4 r4 = {0.f, 0.f, 0.f, 0.f};
    // load4_rows with the reference row inside the same decision
    if (VEC && 4 * g + 4 <= n) {
#pragma unroll
      for (int k = 0; k < K; ++k) v[k] = reinterpret_cast<const float4*>(rows.p[k])[g];
      if (ref != nullptr) r4 = reinterpret_cast<const float4*>(ref)[g];
    } else {
#pragma unroll
      for (int k = 0; k < K; ++k) v[k] = load4<false>(rows.p[k], g, n);
      if (ref != nullptr) r4 = load4<false>(ref, g, n);
    }
    float o[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float e[K], delta, sigma;
#pragma unroll
      for (int k = 0; k < K; ++k) e[k] = c == 0 ? v[k].x : c == 1 ? v[k].y : c == 2 ? v[k].z : v[k].w;
      const float x0 = e[0];
      collude_coord<K>(e, delta, sigma);
      const float t = fmaf(cb, sigma, ca * delta);
      float m = fmaf(ca, x0, t);
      if (ref != nullptr) m = fmaf(cr, c == 0 ? r4.x : c == 1 ? r4.y : c == 2 ? r4.z : r4.w, m);
      o[c] = m;
    }
    const float4 res = {o[0], o[1], o[2], o[3]};
    for (int p = 0; p < P; ++p) store4<VEC>(outs.p[p], g, n, res);
  }
}

// SCAFFOLD (Karimireddy et al.) server step in two launches around one all-reduce; float4 body,
// scalar tail. Sums run in the same k order as the host reference.
__global__ __launch_bounds__(FL_BLOCK) void k_scaffold_reduce(float* __restrict__ buf, RowPtrs dy, RowPtrs dc, RowW w, int K, int64_t n) {
  const int64_t gid = (int64_t)blockIdx.x * FL_BLOCK + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * FL_BLOCK;
  for (int64_t i = gid; i < n; i += stride) {
    float sy = 0.f, sc = 0.f;
    for (int k = 0; k < K; ++k) {
      sy = fmaf(w.w[k], dy.p[k][i], sy);
      sc += dc.p[k][i];
    }
    buf[i] = sy;
    buf[n + 1 + i] = sc;
  }
  if (gid == 0) {
    float ws = 0.f;
    for (int k = 0; k < K; ++k) ws += w.w[k];
    buf[n] = ws;
    buf[2 * n + 1] = (float)K;
  }
}

__global__ __launch_bounds__(FL_BLOCK) void k_scaffold_apply(OutPtrs outs, int P, const float* __restrict__ x_start, const float* __restrict__ buf,
                                                             float* __restrict__ c, int c_init, float glr, int64_t n) {
  const float scale = glr / fmaxf(buf[n], 1e-12f);
  const float inv_cnt = 1.f / fmaxf(buf[2 * n + 1], 1.f);
  const int64_t stride = (int64_t)gridDim.x * FL_BLOCK;
  for (int64_t i = (int64_t)blockIdx.x * FL_BLOCK + threadIdx.x; i < n; i += stride) {
    const float x = fmaf(buf[i], scale, x_start[i]);
    for (int p = 0; p < P; ++p) outs.p[p][i] = x;
    c[i] = (c_init ? 0.f : c[i]) + buf[n + 1 + i] * inv_cnt;
  }
}

// Fused Adam / SGD over a flat fp32 buffer (torch.optim semantics) + optional FedProx/SCAFFOLD terms
__global__ __launch_bounds__(FL_BLOCK) void k_opt_step(float* __restrict__ param, const float* __restrict__ grad, float* __restrict__ m,
                                                        float* __restrict__ v, bf16* __restrict__ shadow, int64_t n, OptParams o, float bc1, float bc2s,
                                                        const float* __restrict__ anchor, const float* __restrict__ cg, const float* __restrict__ cl) {
  const int64_t stride = (int64_t)gridDim.x * FL_BLOCK;
  for (int64_t i = blockIdx.x * FL_BLOCK + threadIdx.x; i < n; i += stride) {
    float w = param[i];
    float mm = m != nullptr ? m[i] : 0.f;
    float vv = v != nullptr ? v[i] : 0.f;
    opt_update(o, grad[i], w, mm, vv, bc1, bc2s, anchor, cg, cl, i);
    param[i] = w;
    if (m != nullptr) m[i] = mm;
    if (v != nullptr) v[i] = vv;
    if (shadow != nullptr) shadow[i] = (bf16)w;
  }
}

// t = scale·t + σ·N(0,1), counter-based RNG (splitmix64 + Box-Muller)
__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

__global__ __launch_bounds__(FL_BLOCK) void k_scale_add_noise(float* __restrict__ t, int64_t n, float scale, float sigma, uint64_t seed) {
  const int64_t stride = (int64_t)gridDim.x * FL_BLOCK;
  for (int64_t i = blockIdx.x * FL_BLOCK + threadIdx.x; i < n; i += stride) {
    float val = t[i] * scale;
    if (sigma != 0.f) {
      const uint64_t r = splitmix64(seed * 0x100000001B3ull + (uint64_t)i);
      const float u1 = ((r >> 40) + 1) * (1.0f / 16777217.0f);
      const float u2 = ((r & 0xFFFFFFull)) * (1.0f / 16777216.0f);
      val += sigma * sqrtf(-2.f * __logf(u1)) * __cosf(6.2831853f * u2);
    }
    t[i] = val;
  }
}

// Divide-and-Conquer (DnC; Shejwalkar & Houmansadr, NDSS 2021) in three launches:
//   k_dnc_sqdist<K>: k_pairwise_sqdist<K> over a subsample of the coordinates, one slab block of
//                    work[iters][grid][K(K-1)/2] per iteration (gridDim.y = iters)
//   k_dnc_select   : one block; per iteration the slabs summed as k_krum_select does, the rows of
//                    non-finite distances screened, the centred Gram matrix G = −½·J·D·J of the rest
//                    (J = I − 11ᵀ/K_v), its top eigenpair by repeated squaring, the scores λ·u_i² and
//                    the m highest removed; then the iterations intersected: dist / score / lam /
//                    removed / coef
//   k_coef_mean<K> : out rows <- Σ_k coef[k] · row_k
// The coordinates are subsampled in tiles of 256: the 64 float4 groups one wave loads at a time,
// so the test is wave-uniform and no cache line is half used. Tile τ of iteration t is taken iff
// splitmix64(key[t] ^ τ) < thr or τ == forced[t] (the host derives key, thr and forced from the
// seed and the round); all != 0 takes every tile and hashes nothing.

// k_pairwise_sqdist<K, VEC>'s row loads, pair_sqdist_add and store_slab: with every tile taken, block
// b of iteration t stores the slab k_pairwise_sqdist's block b stores, bit for bit. g >> 6 is the same
// in all lanes of a wave (FL_BLOCK and the grid stride are multiples of 64): it goes through
// readfirstlane, so the hash is scalar work and the skip a scalar branch. Every register index is
// static.
template <int K, bool VEC>
__global__ __launch_bounds__(FL_BLOCK) void k_dnc_sqdist(float* __restrict__ work, RowPtrs rows, DncTiles tiles, int64_t n) {
  constexpr int NP = K * (K - 1) / 2;
  float acc[NP];
#pragma unroll
  for (int q = 0; q < NP; ++q) acc[q] = 0.f;
  const int it = blockIdx.y;
  const uint64_t key = tiles.key[it], forced = tiles.forced[it];
  const int64_t groups = (n + 3) / 4;
  const int64_t stride = (int64_t)gridDim.x * FL_BLOCK;
  for (int64_t g = (int64_t)blockIdx.x * FL_BLOCK + threadIdx.x; g < groups; g += stride) {
    if (!tiles.all) {
      const int64_t tg = g >> 6;
      const uint64_t tau = ((uint64_t)(unsigned)__builtin_amdgcn_readfirstlane((int)(tg >> 32)) << 32) |
                           (uint64_t)(unsigned)__builtin_amdgcn_readfirstlane((int)(tg & 0xFFFFFFFFll));
      if (!(splitmix64(key ^ tau) < tiles.thr || tau == forced)) continue;
    }
    pair_sqdist_add<K, VEC>(rows, g, n, acc);
  }
  store_slab<NP>(acc, work + ((int64_t)it * gridDim.x + blockIdx.x) * NP);
}

// One block. Per iteration it (slabs work[it][G][K(K-1)/2], summed by krum_sum_slabs into D):
//  1 screen : row i is screened when more than half of its K−1 distances are non-finite; then, j
//             ascending, an unscreened row j with a non-finite distance to an unscreened row i < j
//             is screened too. V: the unscreened rows, K_v of them. Screened rows score +inf.
//  2 centre : r_i = (Σ_{j∈V} D_ij) / K_v and c = (Σ_{i∈V} r_i) / K_v, both sums ascending;
//             A_ij = −½ (((D_ij − r_i) − r_j) + c), G_ij = ½ (A_ij + A_ji); rows outside V hold 0.
//             K_v <= 1 or tr G <= 0: λ = 0 and every score on V is 0.
//  3 eigen  : M <- G / tr G; 20 times M <- M·M (thread (i, j) of the first 256 sums M_ik·M_kj over k
//             ascending, one fma per term) and M <- M / tr M; j* = argmax_j M_jj (the lowest on a
//             tie), u = M[:, j*] / |M[:, j*]|, λ = uᵀ(G u), s_i = λ·u_i². All in double, in LDS.
//  4 remove : the m highest scores, the higher row first among equals; screened rows always go.
// Then removed[k] = the first iteration that removed row k (−1: kept in all of them) and
// coef[k] = float(w_k / Σ_kept w) for a kept row, else 0; nothing kept (screening only): w_k / Σ w
// over all rows. Sums of weights 0: the plain mean of those rows, as k_krum_select.
#define DNC_SQUARINGS 20
__global__ __launch_bounds__(KRUM_SELECT_BLOCK) void k_dnc_select(const float* __restrict__ work, int G, int K, int m, int iters, RowW w,
                                                                  double* __restrict__ dist, double* __restrict__ score, double* __restrict__ lam,
                                                                  int* __restrict__ removed, float* __restrict__ coef) {
  __shared__ double d[16][16];
  __shared__ double gm[16][16];
  __shared__ double ma[16][16];
  __shared__ double mb[16][16];
  __shared__ double part[KRUM_SELECT_BLOCK];
  __shared__ double rmean[16], u[16], gu[16], sc[16];
  __shared__ double cen, trg;
  __shared__ unsigned screened;
  __shared__ int jstar;
  __shared__ int rem[16];
  const int t = threadIdx.x;
  const int i = (t >> 4) & 15, j = t & 15;  // the matrix entry of thread t < 256
  const int NP = K * (K - 1) / 2;
  const double inf = __builtin_huge_val();
  if (t < 16) rem[t] = -1;
  for (int it = 0; it < iters; ++it) {
    krum_sum_slabs(work + (int64_t)it * G * NP, G, K, d, part);  // ends with a barrier
    for (int q = t; q < K * K; q += KRUM_SELECT_BLOCK) dist[(int64_t)it * K * K + q] = d[q / K][q % K];
    if (t == 0) {
      unsigned s = 0;
      for (int a = 0; a < K; ++a) {
        int bad = 0;
        for (int b = 0; b < K; ++b)
          if (b != a && !__builtin_isfinite(d[a][b])) ++bad;
        if (2 * bad > K - 1) s |= 1u << a;
      }
      for (int b = 1; b < K; ++b) {
        if ((s >> b) & 1u) continue;
        for (int a = 0; a < b; ++a)
          if (!((s >> a) & 1u) && !__builtin_isfinite(d[a][b])) {
            s |= 1u << b;
            break;
          }
      }
      screened = s;
    }
    __syncthreads();
    const unsigned S = screened;
    const int kv = K - __popc(S);
    const bool vi = i < K && !((S >> i) & 1u), vj = j < K && !((S >> j) & 1u);
    if (t < 16) {
      double s = 0.0;
      if (t < K && !((S >> t) & 1u)) {
        for (int b = 0; b < K; ++b)
          if (!((S >> b) & 1u)) s += d[t][b];
        s /= (double)kv;
      }
      rmean[t] = s;
    }
    __syncthreads();
    if (t == 0) {
      double s = 0.0;
      for (int a = 0; a < K; ++a)
        if (!((S >> a) & 1u)) s += rmean[a];
      cen = kv > 0 ? s / (double)kv : 0.0;
    }
    __syncthreads();
    if (t < 256) ma[i][j] = (vi && vj) ? -0.5 * (((d[i][j] - rmean[i]) - rmean[j]) + cen) : 0.0;
    __syncthreads();
    if (t < 256) gm[i][j] = 0.5 * (ma[i][j] + ma[j][i]);
    __syncthreads();
    if (t == 0) {
      double s = 0.0;
      for (int a = 0; a < 16; ++a) s += gm[a][a];
      trg = s;
    }
    __syncthreads();
    const double tr0 = trg;
    const bool flat = kv <= 1 || !(tr0 > 0.0);  // one barrier-uniform decision: trg is shared
    if (!flat) {
      if (t < 256) ma[i][j] = gm[i][j] / tr0;
      __syncthreads();
      for (int r = 0; r < DNC_SQUARINGS; ++r) {
        if (t < 256) {
          double s = 0.0;
#pragma unroll
          for (int k = 0; k < 16; ++k) s = fma(ma[i][k], ma[k][j], s);
          mb[i][j] = s;
        }
        __syncthreads();
        if (t < 256) {
          double tr = 0.0;
#pragma unroll
          for (int k = 0; k < 16; ++k) tr += mb[k][k];
          ma[i][j] = mb[i][j] / tr;
        }
        __syncthreads();
      }
      if (t == 0) {
        int best = 0;
        for (int a = 1; a < 16; ++a)
          if (ma[a][a] > ma[best][best]) best = a;
        jstar = best;
      }
      __syncthreads();
      if (t < 16) {
        const int js = jstar;
        double nn = 0.0;
        for (int a = 0; a < 16; ++a) nn = fma(ma[a][js], ma[a][js], nn);
        u[t] = ma[t][js] / sqrt(nn);
      }
      __syncthreads();
      if (t < 16) {
        double s = 0.0;
        for (int b = 0; b < 16; ++b) s = fma(gm[t][b], u[b], s);
        gu[t] = s;
      }
      __syncthreads();
    }
    if (t < K) {
      double l = 0.0;
      if (!flat)
        for (int a = 0; a < 16; ++a) l = fma(u[a], gu[a], l);
      const double s = ((S >> t) & 1u) ? inf : (flat ? 0.0 : l * (u[t] * u[t]));
      sc[t] = s;
      score[it * K + t] = s;
      if (t == 0) lam[it] = l;
    }
    __syncthreads();
    if (t < K) {
      int rank = 0;  // rows removed before row t
      for (int b = 0; b < K; ++b)
        if (b != t && (sc[b] > sc[t] || (sc[b] == sc[t] && b > t))) ++rank;
      if ((((S >> t) & 1u) || rank < m) && rem[t] < 0) rem[t] = it;
    }
    __syncthreads();
  }
  if (t < K) {
    double ws = 0.0, wall = 0.0;
    int cnt = 0;
    float wt = 0.f;
    for (int b = 0; b < K; ++b) {
      const float wb = w.w[b];
      if (b == t) wt = wb;
      wall += (double)wb;
      if (rem[b] < 0) {
        ws += (double)wb;
        ++cnt;
      }
    }
    removed[t] = rem[t];
    float c;
    if (cnt == 0) c = wall > 0.0 ? (float)((double)wt / wall) : 1.f / (float)K;
    else if (rem[t] >= 0) c = 0.f;
    else c = ws > 0.0 ? (float)((double)wt / ws) : 1.f / (float)cnt;
    coef[t] = c;
  }
}

// ------------------------------------------------------------------------------------------------
void fl_weighted_sum(float* out, const uint64_t* srcs, const float* w, int K, int64_t n, bool srcs_aligned16, hipStream_t s) {
  const dim3 g(grid_for(n / 4 + 1)), b(FL_BLOCK);
  if (srcs_aligned16 && vec_ok(0, out)) hipLaunchKernelGGL(k_weighted_sum<true>, g, b, 0, s, out, srcs, w, K, n);
  else hipLaunchKernelGGL(k_weighted_sum<false>, g, b, 0, s, out, srcs, w, K, n);
}
void fl_stacked_weighted_sum(float* out, const float* stacked, int P, int64_t n, int64_t ld, const float* w, float scale, hipStream_t s) {
  hipLaunchKernelGGL(k_stacked_weighted_sum, dim3(grid_for(n / 4 + 1)), dim3(FL_BLOCK), 0, s, out, stacked, P, n, ld, w, scale,
                     vec_ok(ld, out, stacked));
}
void fl_broadcast_rows(float* stacked, const float* src, int P, int64_t n, int64_t ld, const float* mask, hipStream_t s) {
  unsigned gx = grid_for(n / 4 + 1);
  if (gx > 256) gx = 256;
  hipLaunchKernelGGL(k_broadcast_rows, dim3(gx, P), dim3(FL_BLOCK), 0, s, stacked, src, P, n, ld, mask, vec_ok(ld, stacked, src));
}

// The robust aggregators' kernels take the row count (and Bulyan's f) as template arguments.
// dispatch_int calls f(std::integral_constant<int, x>) for the run-time x in LO..HI and returns true;
// for an x outside the range it calls nothing, so nothing is launched, and returns false.
// dispatch_rows does so for a row count K in LO..16 and hands f the alignment flag as a second
// compile-time argument (std::bool_constant<vec>).
template <int LO, typename F, int... I>
static bool dispatch_seq(int x, F& f, std::integer_sequence<int, I...>) {
  return ((x == LO + I ? (f(std::integral_constant<int, LO + I>{}), true) : false) || ...);
}
template <int LO, int HI, typename F>
static bool dispatch_int(int x, F f) {
  return dispatch_seq<LO>(x, f, std::make_integer_sequence<int, HI - LO + 1>{});
}
template <int LO, typename F>
static bool dispatch_rows(int K, bool vec, F f) {
  return dispatch_int<LO, 16>(K, [&](auto k) {
    if (vec) f(k, std::true_type{});
    else f(k, std::false_type{});
  });
}

void fl_coordinate_median(const OutPtrs& outs, int P, const RowPtrs& rows, int K, int64_t n, hipStream_t s) {
  const dim3 g(grid_for(n)), b(FL_BLOCK);
  dispatch_int<1, 16>(K, [&](auto k) { hipLaunchKernelGGL(k_coordinate_median<k()>, g, b, 0, s, outs, P, rows, n); });
}
void fl_trimmed_mean(const OutPtrs& outs, int P, const RowPtrs& rows, int K, int trim, int64_t n, hipStream_t s) {
  const dim3 g(grid_for(n)), b(FL_BLOCK);
  dispatch_int<1, 16>(K, [&](auto k) { hipLaunchKernelGGL(k_trimmed_mean<k()>, g, b, 0, s, outs, P, rows, trim, n); });
}
static bool all_aligned16(const RowPtrs& rows, int K, const OutPtrs* outs, int P) {
  uintptr_t bits = 0;
  for (int k = 0; k < K; ++k) bits |= reinterpret_cast<uintptr_t>(rows.p[k]);
  for (int p = 0; outs != nullptr && p < P; ++p) bits |= reinterpret_cast<uintptr_t>(outs->p[p]);
  return (bits & 15u) == 0;
}
// k_pairwise_sqdist<K> on fl_krum_grid(n, K) blocks; returns the grid (0 for K == 1: no pair)
static unsigned launch_pairwise_sqdist(float* work, const RowPtrs& rows, int K, int64_t n, hipStream_t s) {
  const unsigned grid = K > 1 ? fl_krum_grid(n, K) : 0;
  const bool vec = all_aligned16(rows, K, nullptr, 0);
  const dim3 g(grid), b(FL_BLOCK);
  // from 2: K == 1 has no pair, nothing to measure
  dispatch_rows<2>(K, vec, [&](auto k, auto v) { hipLaunchKernelGGL((k_pairwise_sqdist<k(), v()>), g, b, 0, s, work, rows, n); });
  return grid;
}
void fl_krum_select(float* work, const RowPtrs& rows, const RowW& w, int K, int f, int m, int64_t n, double* dist, double* score, float* coef,
                    hipStream_t s) {
  const unsigned grid = launch_pairwise_sqdist(work, rows, K, n, s);
  hipLaunchKernelGGL(k_krum_select, dim3(1), dim3(KRUM_SELECT_BLOCK), 0, s, work, (int)grid, K, f, m, w, dist, score, coef);
}
void fl_coef_mean(const OutPtrs& outs, int P, const RowPtrs& rows, int K, const float* coef, int64_t n, hipStream_t s) {
  const bool vec = all_aligned16(rows, K, &outs, P);
  const dim3 g(grid_for((n + 3) / 4)), b(FL_BLOCK);
  dispatch_rows<1>(K, vec, [&](auto k, auto v) { hipLaunchKernelGGL((k_coef_mean<k(), v()>), g, b, 0, s, outs, P, rows, coef, n); });
}
void fl_clipped_gossip(float* work, const OutPtrs& rows, int K, const ClipPlan& plan, int64_t n, double* dist, double* tau, float* w_eff,
                       hipStream_t s) {
  if (K < 2 || K > 16) return;  // one row has no neighbour
  RowPtrs src{};
  for (int k = 0; k < K; ++k) src.p[k] = rows.p[k];
  const unsigned grid = launch_pairwise_sqdist(work, src, K, n, s);
  hipLaunchKernelGGL(k_clip_plan, dim3(1), dim3(KRUM_SELECT_BLOCK), 0, s, work, (int)grid, K, plan, dist, tau, w_eff);
  const bool vec = all_aligned16(src, K, nullptr, 0);
  const dim3 g(grid_for((n + 3) / 4)), b(FL_BLOCK);
  dispatch_rows<2>(K, vec, [&](auto k, auto v) { hipLaunchKernelGGL((k_clipped_mix<k(), v()>), g, b, 0, s, rows, w_eff, n); });
}
void fl_bulyan_mean(const OutPtrs& outs, int P, const RowPtrs& rows, int K, int f, const float* coef, int64_t n, hipStream_t s) {
  const bool vec = all_aligned16(rows, K, &outs, P);
  const dim3 g(grid_for((n + 3) / 4)), b(FL_BLOCK);
  dispatch_rows<1>(K, vec, [&](auto k, auto v) {
    constexpr int KK = decltype(k)::value;
    constexpr bool VEC = decltype(v)::value;
    dispatch_int<0, 3>(f, [&](auto ff) {
      // k_bulyan_mean<K, F> exists for the attacker bounds K admits only (K >= 4F + 3, or F == 0)
      constexpr int F = decltype(ff)::value;
      if constexpr (F == 0 || KK >= 4 * F + 3) hipLaunchKernelGGL((k_bulyan_mean<KK, F, VEC>), g, b, 0, s, outs, P, rows, coef, n);
    });
  });
}
void fl_bulyan(float* work, const OutPtrs& outs, int P, const RowPtrs& rows, int K, int f, int64_t n, double* dist, double* score, int* pick,
               float* coef, hipStream_t s) {
  const unsigned grid = launch_pairwise_sqdist(work, rows, K, n, s);
  hipLaunchKernelGGL(k_bulyan_select, dim3(1), dim3(KRUM_SELECT_BLOCK), 0, s, work, (int)grid, K, f, dist, score, pick, coef);
  if (P > 0) fl_bulyan_mean(outs, P, rows, K, f, coef, n, s);
}
void fl_dnc(float* work, const OutPtrs& outs, int P, const RowPtrs& rows, const RowW& w, int K, int m, int iters, const DncTiles& tiles, int64_t n,
            double* dist, double* score, double* lam, int* removed, float* coef, hipStream_t s) {
  if (K < 1 || K > 16 || iters < 1 || iters > DNC_MAX_ITERS) return;
  if (K > 1) {
    const unsigned grid = fl_krum_grid(n, K);
    const bool vec = all_aligned16(rows, K, nullptr, 0);
    const dim3 g(grid, iters), b(FL_BLOCK);
    dispatch_rows<2>(K, vec, [&](auto k, auto v) { hipLaunchKernelGGL((k_dnc_sqdist<k(), v()>), g, b, 0, s, work, rows, tiles, n); });
    hipLaunchKernelGGL(k_dnc_select, dim3(1), dim3(KRUM_SELECT_BLOCK), 0, s, work, (int)grid, K, m, iters, w, dist, score, lam, removed, coef);
  }
  if (P > 0) fl_coef_mean(outs, P, rows, K, coef, n, s);
}
void fl_geometric_median(float* work, const RowPtrs& rows, const RowW& w, int K, int iters, double nu, int64_t n, float* coef, double* dist,
                         double* obj, hipStream_t s) {
  const unsigned grid = fl_krum_grid(n, K);
  float* what = work + (int64_t)grid * K;
  const bool vec = all_aligned16(rows, K, nullptr, 0);
  const dim3 g(grid), b(FL_BLOCK);
  // pass -1 is the screen (coefficients 0: the sums are |x_k|^2), passes 0..iters-1 the iterations
  for (int t = -1; t < iters; ++t) {
    const float* c = t < 0 ? nullptr : coef;
    if (!dispatch_rows<1>(K, vec, [&](auto k, auto v) { hipLaunchKernelGGL((k_gm_dist<k(), v()>), g, b, 0, s, work, rows, c, n); })) return;
    hipLaunchKernelGGL(k_gm_reweight, dim3(1), dim3(KRUM_SELECT_BLOCK), 0, s, work, (int)grid, K, t < 0 ? GM_SCREEN : GM_ITERATE, t < 0 ? 0 : t, w, nu,
                       what, coef, dist, obj);
  }
}
void fl_collude(float* work, const OutPtrs& outs, int P, const RowPtrs& rows, int K, int kind, float ca, float cb, float cr, const float* ref,
                int64_t n, float* gamma, double* stat, hipStream_t s) {
  const bool solve = kind == COLLUDE_MIN_MAX || kind == COLLUDE_MIN_SUM;
  if (solve) {
    const unsigned gp = launch_pairwise_sqdist(work, rows, K, n, s);
    const unsigned grid = fl_krum_grid(n, K);
    float* stats = work + (int64_t)grid * (K * (K - 1) / 2);
    const bool vec = all_aligned16(rows, K, nullptr, 0);
    const dim3 g(grid), b(FL_BLOCK);
    if (!dispatch_rows<1>(K, vec, [&](auto k, auto v) { hipLaunchKernelGGL((k_collude_stats<k(), v()>), g, b, 0, s, stats, rows, n); })) return;
    hipLaunchKernelGGL(k_collude_solve, dim3(1), dim3(KRUM_SELECT_BLOCK), 0, s, work, (int)gp, stats, (int)grid, K, kind, gamma, stat);
  }
  const bool vec = all_aligned16(rows, K, &outs, P) && (reinterpret_cast<uintptr_t>(ref) & 15u) == 0;
  const float* gin = solve ? gamma : nullptr;
  float* gout = solve ? nullptr : gamma;
  const float gval = kind == COLLUDE_ALIE ? -cb : -ca;
  const dim3 g(grid_for((n + 3) / 4)), b(FL_BLOCK);
  dispatch_rows<1>(K, vec, [&](auto k, auto v) {
    hipLaunchKernelGGL((k_collude_write<k(), v()>), g, b, 0, s, outs, P, rows, ref, ca, cb, cr, gin, gout, gval, n);
  });
}
void fl_scaffold_reduce(float* buf, const RowPtrs& dy, const RowPtrs& dc, const RowW& w, int K, int64_t n, hipStream_t s) {
  hipLaunchKernelGGL(k_scaffold_reduce, dim3(grid_for(n)), dim3(FL_BLOCK), 0, s, buf, dy, dc, w, K, n);
}
void fl_scaffold_apply(const OutPtrs& outs, int P, const float* x_start, const float* buf, float* c, int c_init, float glr, int64_t n, hipStream_t s) {
  hipLaunchKernelGGL(k_scaffold_apply, dim3(grid_for(n)), dim3(FL_BLOCK), 0, s, outs, P, x_start, buf, c, c_init, glr, n);
}
void fl_opt_step(float* param, const float* grad, float* m, float* v, bf16* shadow, int64_t n, const OptParams& o, int step, const float* anchor,
                 const float* cg, const float* cl, hipStream_t s) {
  // in double from the float betas, rounded once: in float, 1 - powf(beta2, t) keeps only ~15 bits at small t
  const float bc1 = (float)(1.0 - pow((double)o.beta1, (double)step));
  const float bc2s = (float)sqrt(1.0 - pow((double)o.beta2, (double)step));
  hipLaunchKernelGGL(k_opt_step, dim3(grid_for(n)), dim3(FL_BLOCK), 0, s, param, grad, m, v, shadow, n, o, bc1, bc2s, anchor, cg, cl);
}
void fl_scale_add_noise(float* t, int64_t n, float scale, float sigma, uint64_t seed, hipStream_t s) {
  hipLaunchKernelGGL(k_scale_add_noise, dim3(grid_for(n)), dim3(FL_BLOCK), 0, s, t, n, scale, sigma, seed);
}

// Resolve one kernel of this translation unit on the current device: loads the unit's code object
// now (myfyp_warm_all, at engine prewarm) instead of at its first launch, which waited for the
// kernels in flight (the first FedAvg launch blocked the host until the running epoch ended)
extern "C" int myfyp_warm_fl_ops() {
  hipFuncAttributes attr;
  // the robust aggregators' launches of the headline peer count (8) resolve here too, so a first
  // Krum / trimmed-mean / geometric-median / Bulyan / DnC round pays no lookup behind a running epoch
  const void* fns[] = {reinterpret_cast<const void*>(&k_weighted_sum<true>),
                       reinterpret_cast<const void*>(&k_trimmed_mean<8>),
                       reinterpret_cast<const void*>(&k_pairwise_sqdist<8, true>),
                       reinterpret_cast<const void*>(&k_krum_select),
                       reinterpret_cast<const void*>(&k_coef_mean<8, true>),
                       reinterpret_cast<const void*>(&k_gm_dist<8, true>),
                       reinterpret_cast<const void*>(&k_gm_reweight),
                       reinterpret_cast<const void*>(&k_bulyan_select),
                       reinterpret_cast<const void*>(&k_bulyan_mean<8, 1, true>),
                       reinterpret_cast<const void*>(&k_dnc_sqdist<8, true>),
                       reinterpret_cast<const void*>(&k_dnc_select)};
  for (const void* fn : fns)
    if (hipFuncGetAttributes(&attr, fn) != hipSuccess) return 1;
  return 0;
}
