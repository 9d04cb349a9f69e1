// Minimum mapping unit for a scene's class map, on the device (kurosiwo_amd/scene.py: label_components, component_sizes, sieve;
// predict.py --mmu): connected components of a uint8 map [Hs][Ws], their sizes, and a one-pass sieve that hands every component of
// fewer than `mmu` pixels to the class most of its edge neighbours in large components have.  Integers throughout: the results do
// not depend on launch geometry or arrival order, and equal the flood fill of tests/sieve_ref.py bit for bit.
//
//   scene_label            labels[p] = the smallest linear index y * Ws + x of p's component (pixels of one class value joined by
//                          edges, or by edges and corners).  Three launches, always three, nothing read on the host, no "repeat until
//                          unchanged" flag, no grid-wide wait:
//                            1. label_tile_kernel: one workgroup per LABEL_TILE_H x LABEL_TILE_W tile runs a union-find over the
//                               tile in LDS (a union per backward neighbour of equal class), then writes every pixel's tile root
//                               as a global linear index: a forest of depth 1 whose roots are tile minima.
//                            2. label_border_kernel: one thread per pixel on the low side of a tile border unions it, in global
//                               memory, with its equal-class neighbours across the border (3 of them at 8-connectivity).
//                            3. label_flatten_kernel: labels[p] = find(p).
//                          Union-find: sieve_uf.h.  Termination, in short: parent[i] <= i always and cells are only lowered by
//                          fetch-min; find walks strictly decreasing labels (at most x steps from x); a union retries only after a
//                          fetch-min that returned a label LOWER than the root it held, which strictly lowers the larger of its two
//                          roots, so it runs at most max(a, b) rounds whatever the other threads do.  No locks, no spinning on
//                          another thread's progress.  Labels that other workgroups may be lowering in the same launch (2, 3) are
//                          read with relaxed agent-scope atomic loads and lowered with agent-scope atomics: the L2s are per XCD and
//                          the L1s per CU, a plain load may stay stale.  A stale (higher) label would still be a valid ancestor, as
//                          labels only go down; the launch boundaries publish everything else.
//   scene_component_sizes  sizes[r] = pixels whose label is r (one entry per pixel, 0 off the roots).  The background of a flood map
//                          is one component of millions of pixels, and one atomic per pixel on one address serialises, so equal
//                          labels are combined first: consecutive lanes of a wave with one label form a run (ballot of the run
//                          heads), the run heads add their length into a small per-block LDS table keyed by label (one probe; a
//                          collision goes straight to global memory), and the table's entries issue the global integer adds: one
//                          per label per 1024 pixels.  Integer adds: order does not matter.
//   scene_sieve_vote       for each pixel p of a small component (size < mmu, class not invalid) and each of its 4 edge neighbours
//                          q inside the scene: q votes for its class at votes[class(q)][label(p)] when it lies in another component
//                          that is not small and not invalid.  Always edges, whatever the connectivity of the labels.  The rows of
//                          the small roots are zeroed first by a launch of their own; no other cell of `votes` is read or written.
//                          At most 4 * mmu adds per address.
//   scene_sieve_apply      out[p] = the class with the most votes at p's root (lowest class on a tie) when p's component is small
//                          and got a vote, else classes[p]; *removed += replaced components (counted at root pixels, summed per
//                          block first).  Judged on the input map only: all replacements happen at once.
//
// A class value that is neither below K nor the invalid class has no row in the vote table: it is treated as invalid (kept, never
// votes).  Thread per pixel, consecutive threads along x: the loads of a wave are runs of consecutive words.
#include "common.h"
#include "../../include/ksmi.h"
#include "errors.h"
#include "sieve_uf.h"

namespace {

constexpr int SIEVE_MAX_K = 8;                 // SCENE_MAX_K of scene.hip
constexpr int LT_H = 16, LT_W = 64;            // the label tile (scene.LABEL_TILE); LT_W a power of two
constexpr int LT_N = LT_H * LT_W;
constexpr int LT_SHIFT = 6;
static_assert((1 << LT_SHIFT) == LT_W, "label tile width");
constexpr int SZ_PER_BLOCK = 1024;             // pixels per block of the size count
constexpr int SZ_SLOTS = 64;                   // labels a block combines in LDS

// parent cells in LDS: this workgroup alone
struct uf_lds_mem {
  int32_t* p;
  KSMI_HD int32_t load(int32_t i) const {
#if defined(__HIP_DEVICE_COMPILE__)
    return __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#else
    return p[i];
#endif
  }
  KSMI_HD int32_t fetch_min(int32_t i, int32_t v) const {
#if defined(__HIP_DEVICE_COMPILE__)
    return __hip_atomic_fetch_min(p + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#else
    return uf_plain_mem{p}.fetch_min(i, v);
#endif
  }
};

// parent cells in global memory that other workgroups lower in the same launch: agent scope, never a plain load
struct uf_global_mem {
  int32_t* p;
  KSMI_HD int32_t load(int32_t i) const {
#if defined(__HIP_DEVICE_COMPILE__)
    return __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    return p[i];
#endif
  }
  KSMI_HD int32_t fetch_min(int32_t i, int32_t v) const {
#if defined(__HIP_DEVICE_COMPILE__)
    return __hip_atomic_fetch_min(p + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    return uf_plain_mem{p}.fetch_min(i, v);
#endif
  }
};

__global__ __launch_bounds__(256) void label_tile_kernel(const unsigned char* __restrict__ cls, int Hs, int Ws, int tiles_x, int conn8,
                                                         int32_t* __restrict__ labels) {
  __shared__ int32_t lab[LT_N];
  __shared__ unsigned char c[LT_N];
  const int y0 = (int)(blockIdx.x / (unsigned)tiles_x) * LT_H, x0 = (int)(blockIdx.x % (unsigned)tiles_x) * LT_W;
  const int hh = min(LT_H, Hs - y0), ww = min(LT_W, Ws - x0);          // the part of the tile inside the scene
  for (int i = threadIdx.x; i < LT_N; i += 256) {
    const int ly = i >> LT_SHIFT, lx = i & (LT_W - 1);
    lab[i] = i;
    c[i] = (ly < hh && lx < ww) ? cls[(int64_t)(y0 + ly) * Ws + x0 + lx] : (unsigned char)0;
  }
  __syncthreads();
  const uf_lds_mem m{lab};
  for (int i = threadIdx.x; i < LT_N; i += 256) {
    const int ly = i >> LT_SHIFT, lx = i & (LT_W - 1);
    if (ly >= hh || lx >= ww) continue;
    const unsigned char cc = c[i];
    if (lx > 0 && c[i - 1] == cc) uf_union(m, i, i - 1);
    if (ly > 0) {
      if (c[i - LT_W] == cc) uf_union(m, i, i - LT_W);
      if (conn8) {
        if (lx > 0 && c[i - LT_W - 1] == cc) uf_union(m, i, i - LT_W - 1);
        if (lx + 1 < ww && c[i - LT_W + 1] == cc) uf_union(m, i, i - LT_W + 1);
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < LT_N; i += 256) {
    const int ly = i >> LT_SHIFT, lx = i & (LT_W - 1);
    if (ly >= hh || lx >= ww) continue;
    const int r = uf_find(m, i);               // row-major inside the tile orders pixels as the scene does: the tile minimum
    labels[(int64_t)(y0 + ly) * Ws + x0 + lx] = (y0 + (r >> LT_SHIFT)) * Ws + x0 + (r & (LT_W - 1));
  }
}

// items [0, n_h): pixel (y, x) of the first row of a tile row, y = (b + 1) * LT_H, against row y - 1;
// items [n_h, total): pixel (y, x) of the first column of a tile column, x = (b + 1) * LT_W, against column x - 1
__global__ __launch_bounds__(256) void label_border_kernel(const unsigned char* __restrict__ cls, int Hs, int Ws, int64_t n_h, int64_t total,
                                                           int conn8, int32_t* labels) {
  int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const uf_global_mem m{labels};
  if (idx < n_h) {
    const int y = ((int)(idx / Ws) + 1) * LT_H, x = (int)(idx % Ws);
    const int p = y * Ws + x, up = p - Ws;
    const unsigned char cc = cls[p];
    if (cls[up] == cc) uf_union(m, p, up);
    if (conn8) {
      if (x > 0 && cls[up - 1] == cc) uf_union(m, p, up - 1);
      if (x + 1 < Ws && cls[up + 1] == cc) uf_union(m, p, up + 1);
    }
  } else {
    idx -= n_h;
    const int x = ((int)(idx / Hs) + 1) * LT_W, y = (int)(idx % Hs);
    const int p = y * Ws + x, left = p - 1;
    const unsigned char cc = cls[p];
    if (cls[left] == cc) uf_union(m, p, left);
    if (conn8) {
      if (y > 0 && cls[left - Ws] == cc) uf_union(m, p, left - Ws);
      if (y + 1 < Hs && cls[left + Ws] == cc) uf_union(m, p, left + Ws);
    }
  }
}

__global__ __launch_bounds__(256) void label_flatten_kernel(int32_t* labels, int HW) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= HW) return;
  const int32_t r = uf_find(uf_global_mem{labels}, (int32_t)p);        // the roots are final in this launch; a cell is only lowered
  __hip_atomic_store(labels + p, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(256) void component_sizes_kernel(const int32_t* __restrict__ labels, int HW, int32_t* __restrict__ sizes) {
  __shared__ int32_t key[SZ_SLOTS], cnt[SZ_SLOTS];
  if (threadIdx.x < SZ_SLOTS) {
    key[threadIdx.x] = -1;
    cnt[threadIdx.x] = 0;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int64_t base = (int64_t)blockIdx.x * SZ_PER_BLOCK;
#pragma unroll
  for (int j = 0; j < SZ_PER_BLOCK / 256; ++j) {
    const int64_t p = base + j * 256 + threadIdx.x;
    int32_t l = p < HW ? labels[p] : -1;                               // every lane takes part; -1 is no label
    if ((unsigned)l >= (unsigned)HW) l = -1;                           // a value that is no pixel index is not counted
    const int32_t prev = __shfl_up(l, 1);
    const bool head = lane == 0 || prev != l;
    const unsigned long long heads = __ballot(head);
    if (head && l >= 0) {
      const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
      const int run = above ? __builtin_ctzll(above) + 1 : 64 - lane;  // lanes to the next head, or to the end of the wave
      const int s = (int)((unsigned)l * 2654435761u >> 26);            // 6 bits: SZ_SLOTS
      const int32_t was = atomicCAS(&key[s], -1, l);
      if (was == -1 || was == l) atomicAdd(&cnt[s], run);
      else atomicAdd(&sizes[l], run);
    }
  }
  __syncthreads();
  if (threadIdx.x < SZ_SLOTS && key[threadIdx.x] >= 0) atomicAdd(&sizes[key[threadIdx.x]], cnt[threadIdx.x]);
}
static_assert(SZ_SLOTS == 64, "the slot hash keeps 6 bits");

__global__ __launch_bounds__(256) void sieve_zero_kernel(const unsigned char* __restrict__ cls, const int32_t* __restrict__ labels,
                                                         const int32_t* __restrict__ sizes, int mmu, int invalid_class, int K, int64_t HW,
                                                         int32_t* __restrict__ votes) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= HW || labels[p] != p || sizes[p] >= mmu || sieve_is_invalid(cls[p], invalid_class, K)) return;
  for (int k = 0; k < K; ++k) votes[k * HW + p] = 0;
}

__global__ __launch_bounds__(256) void sieve_vote_kernel(const unsigned char* __restrict__ cls, const int32_t* __restrict__ labels,
                                                         const int32_t* __restrict__ sizes, int mmu, int invalid_class, int K, int Hs, int Ws,
                                                         int32_t* __restrict__ votes) {
  const int64_t HW = (int64_t)Hs * Ws, p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= HW) return;
  const int32_t r = labels[p];
  if (sieve_is_invalid(cls[p], invalid_class, K) || sizes[r] >= mmu) return;
  const int y = (int)(p / Ws), x = (int)(p % Ws);
  const int64_t nb[4] = {y > 0 ? p - Ws : -1, x > 0 ? p - 1 : -1, x + 1 < Ws ? p + 1 : -1, y + 1 < Hs ? p + Ws : -1};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int64_t q = nb[j];
    if (q < 0) continue;
    const int32_t rq = labels[q];
    const int cq = cls[q];
    if (rq == r || sieve_is_invalid(cq, invalid_class, K) || sizes[rq] < mmu) continue;
    atomicAdd(&votes[cq * HW + r], 1);
  }
}

__global__ __launch_bounds__(256) void sieve_apply_kernel(const unsigned char* __restrict__ cls, const int32_t* __restrict__ labels,
                                                          const int32_t* __restrict__ sizes, const int32_t* __restrict__ votes, int mmu,
                                                          int invalid_class, int K, int64_t HW, unsigned char* __restrict__ out,
                                                          int32_t* __restrict__ removed) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  int gone = 0;
  if (p < HW) {
    int c = cls[p];
    const int32_t r = labels[p];
    if (!sieve_is_invalid(c, invalid_class, K) && sizes[r] < mmu) {
      const int32_t* v = votes + r;
      const int best = sieve_vote_argmax([v, HW](int k) { return v[k * HW]; }, K);
      if (best >= 0) {
        c = best;
        gone = r == p;
      }
    }
    out[p] = (unsigned char)c;
  }
  const int n = __syncthreads_count(gone);
  if (threadIdx.x == 0 && n) atomicAdd(removed, n);
}

// blocks of `per` items, or -1 when the count does not fit a grid
int64_t blocks_of(int64_t total, int per = 256) {
  const int64_t b = (total + per - 1) / per;
  return b > 0x7fffffff ? -1 : b;
}

constexpr int64_t MAX_PIXELS = 0x7fffffff;     // labels are int32 linear indices

}  // namespace

int ksmi_scene_label(const unsigned char* classes_u8, int Hs, int Ws, int connectivity, int32_t* labels_i32, void* stream) {
  if (Hs < 1 || Ws < 1) return ksmi_fail(KSMI_E_ARG, "scene_label: a scene of Hs >= 1 by Ws >= 1 pixels");
  if (connectivity != 4 && connectivity != 8) return ksmi_fail(KSMI_E_ARG, "scene_label: connectivity is 4 or 8");
  const int64_t HW = (int64_t)Hs * Ws;
  if (HW > MAX_PIXELS) return ksmi_fail(KSMI_E_ARG, "scene_label: more than 2^31 - 1 pixels (labels are int32 linear indices)");
  if (!classes_u8 || !labels_i32) return ksmi_fail(KSMI_E_ARG, "scene_label: null pointer");
  const int tiles_x = (Ws + LT_W - 1) / LT_W, tiles_y = (Hs + LT_H - 1) / LT_H;
  const int conn8 = connectivity == 8;
  hipStream_t st = (hipStream_t)stream;
  KSMI_NOTE(label_tile_kernel);
  hipLaunchKernelGGL(label_tile_kernel, dim3((unsigned)((int64_t)tiles_x * tiles_y)), dim3(256), 0, st, classes_u8, Hs, Ws, tiles_x, conn8,
                     labels_i32);
  const int64_t n_h = (int64_t)(tiles_y - 1) * Ws, total = n_h + (int64_t)(tiles_x - 1) * Hs;
  if (total > 0) {
    KSMI_NOTE(label_border_kernel);
    hipLaunchKernelGGL(label_border_kernel, dim3((unsigned)blocks_of(total)), dim3(256), 0, st, classes_u8, Hs, Ws, n_h, total, conn8,
                       labels_i32);
  }
  KSMI_NOTE(label_flatten_kernel);
  hipLaunchKernelGGL(label_flatten_kernel, dim3((unsigned)blocks_of(HW)), dim3(256), 0, st, labels_i32, (int)HW);
  return ksmi_check_launch("scene_label");
}

int ksmi_scene_component_sizes(const int32_t* labels_i32, int64_t HW, int32_t* sizes_i32, void* stream) {
  if (HW < 0 || HW > MAX_PIXELS) return ksmi_fail(KSMI_E_ARG, "scene_component_sizes: 0 <= HW <= 2^31 - 1 pixels");
  if (HW == 0) return 0;
  if (!labels_i32 || !sizes_i32) return ksmi_fail(KSMI_E_ARG, "scene_component_sizes: null pointer");
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(sizes_i32, 0, (size_t)HW * sizeof(int32_t), st) != hipSuccess) return ksmi_check_launch("scene_component_sizes");
  KSMI_NOTE(component_sizes_kernel);
  hipLaunchKernelGGL(component_sizes_kernel, dim3((unsigned)blocks_of(HW, SZ_PER_BLOCK)), dim3(256), 0, st, labels_i32, (int)HW, sizes_i32);
  return ksmi_check_launch("scene_component_sizes");
}

int ksmi_scene_sieve_vote(const unsigned char* classes_u8, const int32_t* labels_i32, const int32_t* sizes_i32, int mmu, int invalid_class,
                          int K, int Hs, int Ws, int32_t* votes_i32, void* stream) {
  if (K < 1 || K > SIEVE_MAX_K) return ksmi_fail(KSMI_E_ARG, "scene_sieve_vote: 1 <= K <= 8 classes");
  if (Hs < 1 || Ws < 1 || invalid_class < 0 || invalid_class > 255)
    return ksmi_fail(KSMI_E_ARG, "scene_sieve_vote: a scene of Hs >= 1 by Ws >= 1 pixels, invalid_class in 0 .. 255");
  const int64_t HW = (int64_t)Hs * Ws;
  if (HW > MAX_PIXELS) return ksmi_fail(KSMI_E_ARG, "scene_sieve_vote: more than 2^31 - 1 pixels");
  if (!classes_u8 || !labels_i32 || !sizes_i32 || !votes_i32) return ksmi_fail(KSMI_E_ARG, "scene_sieve_vote: null pointer");
  hipStream_t st = (hipStream_t)stream;
  KSMI_NOTE(sieve_zero_kernel);
  hipLaunchKernelGGL(sieve_zero_kernel, dim3((unsigned)blocks_of(HW)), dim3(256), 0, st, classes_u8, labels_i32, sizes_i32, mmu, invalid_class, K,
                     HW, votes_i32);
  KSMI_NOTE(sieve_vote_kernel);
  hipLaunchKernelGGL(sieve_vote_kernel, dim3((unsigned)blocks_of(HW)), dim3(256), 0, st, classes_u8, labels_i32, sizes_i32, mmu, invalid_class, K,
                     Hs, Ws, votes_i32);
  return ksmi_check_launch("scene_sieve_vote");
}

int ksmi_scene_sieve_apply(const unsigned char* classes_u8, const int32_t* labels_i32, const int32_t* sizes_i32, const int32_t* votes_i32,
                           int mmu, int invalid_class, int K, int64_t HW, unsigned char* out_u8, int32_t* removed_i32, void* stream) {
  if (K < 1 || K > SIEVE_MAX_K) return ksmi_fail(KSMI_E_ARG, "scene_sieve_apply: 1 <= K <= 8 classes");
  if (HW < 0 || HW > MAX_PIXELS || invalid_class < 0 || invalid_class > 255)
    return ksmi_fail(KSMI_E_ARG, "scene_sieve_apply: 0 <= HW <= 2^31 - 1 pixels, invalid_class in 0 .. 255");
  if (HW == 0) return 0;
  if (!classes_u8 || !labels_i32 || !sizes_i32 || !votes_i32 || !out_u8 || !removed_i32)
    return ksmi_fail(KSMI_E_ARG, "scene_sieve_apply: null pointer");
  KSMI_NOTE(sieve_apply_kernel);
  hipLaunchKernelGGL(sieve_apply_kernel, dim3((unsigned)blocks_of(HW)), dim3(256), 0, (hipStream_t)stream, classes_u8, labels_i32, sizes_i32,
                     votes_i32, mmu, invalid_class, K, HW, out_u8, removed_i32);
  return ksmi_check_launch("scene_sieve_apply");
}
