// Percentiles per zone for a scene's rasters, on the device (kurosiwo_amd/scene.py: zonal_quantiles, zonal_sorted, component_quantiles;
// predict.py --percentiles): a segmented sort of one float32 value raster [Hs][Ws] keyed by an int32 zone raster [Hs][Ws], and a
// selection on the sorted order.  Pixels, zones, the skip rule and the rows are those of zonal.hip (the caller hands in its presence
// flags and their scan).  Everything is an integer or a bit copy: the sorted sequence of values of a row is unique (equal keys are
// equal bits), so the results depend neither on launch geometry nor on arrival order and equal tests/quantile_ref.py bit for bit.  No
// float atomic, no grid-wide wait, no lock, nothing read on the host; every loop is bounded by a size the host passed.
//
//   scene_quantile_zones    zone[row[z]] = z for the present zones: the zone ids in row order.
//   scene_quantile_keys     one 64-bit composite per pixel: (row << 32) | k(v), k(v) = bits ^ (bits >> 31 ? 0xFFFFFFFF : 0x80000000),
//                           the order-preserving map of the floats onto uint32 in which -0.0 < +0.0.  A pixel that is skipped, or
//                           whose value is NaN or +-inf, gets all ones: its every digit is the last one, and its value field is above
//                           the key of every finite value, so it sorts behind every participant whichever digits are sorted.
//   scene_quantile_sort     a stable LSD radix sort of the composites with 8-bit digits between two buffers.  A pass is three
//                           launches: quantile_hist_kernel (one workgroup per QT_TILE elements counts its digits in LDS, integer
//                           adds; a wave whose lanes agree adds once) writes hist[digit][tile]; quantile_scan_kernel (one workgroup
//                           per digit) scans a digit's counts over the tiles in place and leaves the digit's total;
//                           quantile_scatter_kernel walks its tile in rounds of 256 consecutive elements: an element's place among the
//                           equal digits of its round = the lower lanes of its wave with its digit (8 wave64 ballots) + the counts of
//                           the lower waves (LDS), the running per-digit base carries the earlier rounds: the order within a digit
//                           is kept.  The host knows N: the digits of the row field above bits(N - 1) are zero in every participant
//                           and are not sorted: 4 value passes and ceil(bits(N - 1) / 8) row passes, 4 .. 8 in all.
//   scene_quantile_select   one thread per row, which shares the row's bounds among its percentiles.  The segment of row r is [lower
//                           bound of r << 32, lower bound of (r + 1) << 32) in the sorted composites, found by two binary searches;
//                           n = its length.  For each basis point c: pos = c * (n - 1) in int64, k = pos / 10000, g = pos % 10000,
//                           lower = s[k], higher = s[k + (g > 0)], un-keyed; n == 0 gives NaN (0x7fc00000) for both.
//   scene_quantile_segments offsets[r] = the lower bound of r << 32 for r = 0 .. N, and every composite's value field un-keyed.
#include "common.h"
#include "../../include/ksmi.h"
#include "errors.h"

namespace {

constexpr int QT_ITEMS = 16;                   // rounds of a sort tile
constexpr int QT_TILE = 256 * QT_ITEMS;        // scene.QUANTILE_TILE: elements per sort tile (one workgroup)
constexpr int QT_MAX_P = 16;                   // scene.MAX_PERCENTILES
constexpr int QT_BASIS = 10000;                // basis points in 100 %
constexpr int64_t MAX_PIXELS = 0x7fffffff;
constexpr uint64_t QT_LAST = ~0ull;            // the composite of a pixel that takes no part
constexpr uint32_t QT_NAN = 0x7fc00000u;

struct QtPercentiles {
  int32_t c[QT_MAX_P];
};

__device__ __forceinline__ uint32_t key_of_bits(uint32_t b) { return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u); }
__device__ __forceinline__ uint32_t bits_of_key(uint32_t k) { return k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu); }
__device__ __forceinline__ bool is_finite_bits(uint32_t b) { return (b & 0x7f800000u) != 0x7f800000u; }

// exclusive prefix of one value per thread over a block of 256; total = the block's sum.  sh: 4 words of LDS
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t* sh, uint32_t& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint32_t x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = __shfl_up(x, o);
    if (lane >= o) x += t;
  }
  __syncthreads();                             // sh may still be read from a call before
  if (lane == 63) sh[w] = x;
  __syncthreads();
  uint32_t before = 0, all = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t s = sh[i];
    before += i < w ? s : 0u;
    all += s;
  }
  total = all;
  return before + x - v;
}

// the first index in keys[0 .. n) whose composite is not below target; n <= 2^31 - 1, so 32 halvings end the search
__device__ __forceinline__ int64_t lower_bound(const uint64_t* __restrict__ keys, int64_t n, uint64_t target) {
  int64_t lo = 0, hi = n;
  for (int it = 0; it < 32 && lo < hi; ++it) {
    const int64_t mid = (lo + hi) >> 1;
    if (keys[mid] < target) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(256) void quantile_zones_kernel(const int32_t* __restrict__ present, const int32_t* __restrict__ row, int HW, int N,
                                                             int32_t* __restrict__ zone) {
  const int64_t z = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (z >= HW || !present[z]) return;
  const int32_t r = row[z];
  if ((unsigned)r < (unsigned)N) zone[r] = (int32_t)z;                 // a row that is none addresses nothing
}

__global__ __launch_bounds__(256) void quantile_keys_kernel(const int32_t* __restrict__ zones, const unsigned char* __restrict__ where,
                                                            const float* __restrict__ values, const int32_t* __restrict__ row, int HW, int N,
                                                            uint64_t* __restrict__ keys) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= HW) return;
  uint64_t c = QT_LAST;
  const int32_t z = zones[p];
  if ((unsigned)z < (unsigned)HW && (!where || where[p])) {
    const uint32_t bits = __float_as_uint(values[p]);
    if (is_finite_bits(bits)) {
      const int32_t r = row[z];
      if ((unsigned)r < (unsigned)N) c = ((uint64_t)(uint32_t)r << 32) | key_of_bits(bits);      // a row that is none takes no part
    }
  }
  keys[p] = c;
}

// sort pass, launch 1: the digit histogram of one tile -> hist[digit][tile]
__global__ __launch_bounds__(256) void quantile_hist_kernel(const uint64_t* __restrict__ keys, uint32_t* __restrict__ hist, int64_t n, int ntiles,
                                                            int shift) {
  __shared__ uint32_t h[256];
  const int tile = blockIdx.x;
  h[threadIdx.x] = 0;
  __syncthreads();
  const int64_t base = (int64_t)tile * QT_TILE;
  for (int j = 0; j < QT_ITEMS; ++j) {
    if (base + j * 256 >= n) break;                                    // the same answer in every thread
    const int64_t i = base + j * 256 + threadIdx.x;
    const uint32_t d = i < n ? (uint32_t)(keys[i] >> shift) & 255u : 256u;
    const uint32_t d0 = __shfl(d, 0);
    if (__all(d == d0)) {                                              // a wave of one digit (the high digits of a lake): one add
      if ((threadIdx.x & 63) == 0 && d0 < 256u) atomicAdd(&h[d0], 64u);
    } else if (d < 256u) {
      atomicAdd(&h[d], 1u);                                            // integer LDS counts: order-free
    }
  }
  __syncthreads();
  hist[(int64_t)threadIdx.x * ntiles + tile] = h[threadIdx.x];
}

// sort pass, launch 2: per digit the exclusive scan of its counts over the tiles, in place; dtot[digit] = the digit's count
__global__ __launch_bounds__(256) void quantile_scan_kernel(uint32_t* __restrict__ hist, uint32_t* __restrict__ dtot, int ntiles) {
  __shared__ uint32_t sh[4];
  uint32_t* mine = hist + (int64_t)blockIdx.x * ntiles;
  uint32_t carry = 0;
  for (int base = 0; base < ntiles; base += 256) {
    const int i = base + threadIdx.x;
    const uint32_t v = i < ntiles ? mine[i] : 0u;
    uint32_t total;
    const uint32_t ex = block_excl_scan(v, sh, total);
    if (i < ntiles) mine[i] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) dtot[blockIdx.x] = carry;
}

// sort pass, launch 3: the stable scatter
__global__ __launch_bounds__(256) void quantile_scatter_kernel(const uint64_t* __restrict__ kin, uint64_t* __restrict__ kout,
                                                               const uint32_t* __restrict__ hist, const uint32_t* __restrict__ dtot, int64_t n,
                                                               int ntiles, int shift) {
  __shared__ uint32_t base[256];
  __shared__ uint32_t wc[4][256];
  __shared__ uint32_t sh[4];
  const int tile = blockIdx.x;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint32_t total;
  const uint32_t dex = block_excl_scan(dtot[threadIdx.x], sh, total);
  base[threadIdx.x] = dex + hist[(int64_t)threadIdx.x * ntiles + tile];
#pragma unroll
  for (int q = 0; q < 4; ++q) wc[q][threadIdx.x] = 0;
  __syncthreads();
  const unsigned long long lt = (1ull << lane) - 1ull;
  for (int j = 0; j < QT_ITEMS; ++j) {
    const int64_t r0 = (int64_t)tile * QT_TILE + j * 256;
    if (r0 >= n) break;                                                // the same answer in every thread
    const int64_t i = r0 + threadIdx.x;
    const bool in = i < n;
    const uint64_t key = in ? kin[i] : QT_LAST;                        // past the end: the last digit, behind every element of the tile
    const uint32_t d = (uint32_t)(key >> shift) & 255u;
    unsigned long long peers = ~0ull;
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) {
      const unsigned long long m = __ballot((d >> bit) & 1u);
      peers &= ((d >> bit) & 1u) ? m : ~m;
    }
    const uint32_t rank = (uint32_t)__popcll(peers & lt);
    if ((peers & lt) == 0ull) wc[w][d] = (uint32_t)__popcll(peers);
    __syncthreads();
    if (in) {
      uint32_t pos = base[d] + rank;
      for (int q = 0; q < w; ++q) pos += wc[q][d];
      if ((int64_t)pos < n) kout[pos] = key;                           // counts that are no histogram of kin address nothing outside
    }
    __syncthreads();
    base[threadIdx.x] += wc[0][threadIdx.x] + wc[1][threadIdx.x] + wc[2][threadIdx.x] + wc[3][threadIdx.x];
#pragma unroll
    for (int q = 0; q < 4; ++q) wc[q][threadIdx.x] = 0;
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void quantile_select_kernel(const uint64_t* __restrict__ keys, int64_t n, int N, int P, QtPercentiles pct,
                                                              int32_t* __restrict__ valid, uint32_t* __restrict__ lower,
                                                              uint32_t* __restrict__ higher) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= N) return;
  const int64_t s0 = lower_bound(keys, n, (uint64_t)r << 32), s1 = lower_bound(keys, n, ((uint64_t)r + 1ull) << 32);
  const int64_t cnt = s1 - s0;
  valid[r] = (int32_t)cnt;
  for (int j = 0; j < P; ++j) {                                        // P <= QT_MAX_P; consecutive threads, consecutive rows: the stores coalesce
    uint32_t lo = QT_NAN, hi = QT_NAN;
    if (cnt > 0) {
      const int64_t pos = (int64_t)pct.c[j] * (cnt - 1), k = pos / QT_BASIS, g = pos % QT_BASIS;   // g > 0 only where k < cnt - 1
      lo = bits_of_key((uint32_t)keys[s0 + k]);
      hi = bits_of_key((uint32_t)keys[s0 + k + (g > 0)]);
    }
    lower[(int64_t)j * N + r] = lo;
    higher[(int64_t)j * N + r] = hi;
  }
}

__global__ __launch_bounds__(256) void quantile_offsets_kernel(const uint64_t* __restrict__ keys, int64_t n, int N, int32_t* __restrict__ offsets) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r > N) return;
  offsets[r] = (int32_t)lower_bound(keys, n, (uint64_t)r << 32);
}

__global__ __launch_bounds__(256) void quantile_values_kernel(const uint64_t* __restrict__ keys, int64_t n, uint32_t* __restrict__ sorted) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) sorted[i] = bits_of_key((uint32_t)keys[i]);
}

unsigned blocks_of(int64_t total, int per = 256) { return (unsigned)((total + per - 1) / per); }

int64_t tiles_of(int64_t n) { return (n + QT_TILE - 1) / QT_TILE; }

// 4 value passes and one row pass per started byte of the largest row, N - 1
int passes_of(int64_t N) {
  int bits = 0;
  for (int64_t top = N - 1; top > 0; top >>= 1) ++bits;
  return 4 + (bits + 7) / 8;
}

// 0, or KSMI_E_ARG with a message that names the entry point
int bad_sizes(const char* entry, int64_t HW, int64_t N) {
  const char* what = HW < 0 || HW > MAX_PIXELS ? "0 <= HW <= 2^31 - 1 pixels" : N < 0 || N > HW ? "0 <= N <= HW rows" : nullptr;
  if (!what) return 0;
  char msg[96];
  snprintf(msg, sizeof(msg), "%s: %s", entry, what);
  return ksmi_fail(KSMI_E_ARG, msg);
}

}  // namespace

int ksmi_scene_quantile_passes(int64_t N) { return N < 0 || N > MAX_PIXELS ? -1 : N == 0 ? 0 : passes_of(N); }

int64_t ksmi_scene_quantile_scratch(int64_t HW) { return HW < 0 || HW > MAX_PIXELS ? -1 : HW == 0 ? 0 : 256 * tiles_of(HW) + 256; }

int ksmi_scene_quantile_zones(const int32_t* present_i32, const int32_t* row_i32, int64_t HW, int64_t N, int32_t* zone_i32, void* stream) {
  if (const int rc = bad_sizes("scene_quantile_zones", HW, N)) return rc;
  if (HW == 0 || N == 0) return 0;
  if (!present_i32 || !row_i32 || !zone_i32) return ksmi_fail(KSMI_E_ARG, "scene_quantile_zones: null pointer");
  KSMI_NOTE(quantile_zones_kernel);
  hipLaunchKernelGGL(quantile_zones_kernel, dim3(blocks_of(HW)), dim3(256), 0, (hipStream_t)stream, present_i32, row_i32, (int)HW, (int)N, zone_i32);
  return ksmi_check_launch("scene_quantile_zones");
}

int ksmi_scene_quantile_keys(const int32_t* zones_i32, const unsigned char* where_u8, const float* values_f32, const int32_t* row_i32, int64_t HW,
                             int64_t N, uint64_t* keys_u64, void* stream) {
  if (const int rc = bad_sizes("scene_quantile_keys", HW, N)) return rc;
  if (HW == 0 || N == 0) return 0;
  if (!zones_i32 || !values_f32 || !row_i32 || !keys_u64) return ksmi_fail(KSMI_E_ARG, "scene_quantile_keys: null pointer");
  KSMI_NOTE(quantile_keys_kernel);
  hipLaunchKernelGGL(quantile_keys_kernel, dim3(blocks_of(HW)), dim3(256), 0, (hipStream_t)stream, zones_i32, where_u8, values_f32, row_i32,
                     (int)HW, (int)N, keys_u64);
  return ksmi_check_launch("scene_quantile_keys");
}

int ksmi_scene_quantile_sort(uint64_t* keys_u64, uint64_t* alt_u64, int64_t HW, int64_t N, uint32_t* scratch_u32, int64_t scratch_elems,
                             void* stream) {
  if (const int rc = bad_sizes("scene_quantile_sort", HW, N)) return rc;
  if (HW == 0 || N == 0) return 0;
  if (!keys_u64 || !alt_u64 || !scratch_u32 || keys_u64 == alt_u64) return ksmi_fail(KSMI_E_ARG, "scene_quantile_sort: null pointer, or one buffer twice");
  const int64_t ntiles = tiles_of(HW);
  if (scratch_elems < 256 * ntiles + 256) return ksmi_fail(KSMI_E_ARG, "scene_quantile_sort: scratch smaller than ksmi_scene_quantile_scratch asks for");
  hipStream_t st = (hipStream_t)stream;
  uint32_t* hist = scratch_u32;
  uint32_t* dtot = scratch_u32 + 256 * ntiles;
  uint64_t* from = keys_u64;
  uint64_t* to = alt_u64;
  const int passes = passes_of(N);
  for (int pass = 0; pass < passes; ++pass) {
    const int shift = 8 * pass;
    KSMI_NOTE(quantile_hist_kernel);
    hipLaunchKernelGGL(quantile_hist_kernel, dim3((unsigned)ntiles), dim3(256), 0, st, from, hist, HW, (int)ntiles, shift);
    KSMI_NOTE(quantile_scan_kernel);
    hipLaunchKernelGGL(quantile_scan_kernel, dim3(256), dim3(256), 0, st, hist, dtot, (int)ntiles);
    KSMI_NOTE(quantile_scatter_kernel);
    hipLaunchKernelGGL(quantile_scatter_kernel, dim3((unsigned)ntiles), dim3(256), 0, st, from, to, hist, dtot, HW, (int)ntiles, shift);
    uint64_t* t = from;
    from = to;
    to = t;
  }
  return ksmi_check_launch("scene_quantile_sort");
}

int ksmi_scene_quantile_select(const uint64_t* sorted_u64, int64_t HW, int64_t N, const int32_t* percentiles_host_i32, int P, int32_t* valid_i32,
                               float* lower_f32, float* higher_f32, void* stream) {
  if (const int rc = bad_sizes("scene_quantile_select", HW, N)) return rc;
  if (P < 1 || P > QT_MAX_P) return ksmi_fail(KSMI_E_ARG, "scene_quantile_select: 1 <= P <= 16 percentiles");
  if (!percentiles_host_i32) return ksmi_fail(KSMI_E_ARG, "scene_quantile_select: null pointer");
  QtPercentiles pct = {};
  for (int j = 0; j < P; ++j) {
    if (percentiles_host_i32[j] < 0 || percentiles_host_i32[j] > QT_BASIS)
      return ksmi_fail(KSMI_E_ARG, "scene_quantile_select: a percentile is 0 .. 10000 basis points");
    pct.c[j] = percentiles_host_i32[j];
  }
  if (HW == 0 || N == 0) return 0;
  if (!sorted_u64 || !valid_i32 || !lower_f32 || !higher_f32) return ksmi_fail(KSMI_E_ARG, "scene_quantile_select: null pointer");
  KSMI_NOTE(quantile_select_kernel);
  hipLaunchKernelGGL(quantile_select_kernel, dim3(blocks_of(N)), dim3(256), 0, (hipStream_t)stream, sorted_u64, HW, (int)N, P, pct, valid_i32,
                     (uint32_t*)lower_f32, (uint32_t*)higher_f32);
  return ksmi_check_launch("scene_quantile_select");
}

int ksmi_scene_quantile_segments(const uint64_t* sorted_u64, int64_t HW, int64_t N, int32_t* offsets_i32, float* sorted_f32, void* stream) {
  if (const int rc = bad_sizes("scene_quantile_segments", HW, N)) return rc;
  if (HW == 0 || N == 0) return 0;
  if (!sorted_u64 || !offsets_i32 || !sorted_f32) return ksmi_fail(KSMI_E_ARG, "scene_quantile_segments: null pointer");
  hipStream_t st = (hipStream_t)stream;
  KSMI_NOTE(quantile_offsets_kernel);
  hipLaunchKernelGGL(quantile_offsets_kernel, dim3(blocks_of(N + 1)), dim3(256), 0, st, sorted_u64, HW, (int)N, offsets_i32);
  KSMI_NOTE(quantile_values_kernel);
  hipLaunchKernelGGL(quantile_values_kernel, dim3(blocks_of(HW)), dim3(256), 0, st, sorted_u64, HW, (uint32_t*)sorted_f32);
  return ksmi_check_launch("scene_quantile_segments");
}
