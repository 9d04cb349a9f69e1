// Zonal statistics for a scene's rasters, on the device (kurosiwo_amd/scene.py: zonal_stats, component_stats; predict.py --polygons
// attributes, --components): a reduction of up to 8 float32 value rasters [B][Hs][Ws] keyed by an int32 zone raster [Hs][Ws] -- per
// zone the pixel count, the bounding box, the sums of x and y, and per band the finite values' count, extremes and fixed-point sum.
// Everything accumulated is an integer, or a minimum / maximum under a total order: integer adds and min / max commute, so the results
// depend neither on launch geometry nor on arrival order and equal tests/zonal_ref.py bit for bit.  No float atomic, no grid-wide
// wait, no lock, nothing read on the host but N (by the caller, between scene_zonal_mark's scan and scene_zonal_tables).
//
//   scene_zonal_mark        present[z] = 1 for every zone z that a pixel which is not skipped has.  A pixel is skipped when its zone is
//                           no index 0 .. HW - 1 or `where` is zero there.  Stores to one address serialise (one store per wave on a
//                           one-zone map of 20 M pixels took 11.6 ms), so a flag is stored once per workgroup and zone at most: only the
//                           first lane of a run of equal zones goes on, a table of ZN_SLOTS keys in LDS remembers what the workgroup has
//                           marked, and a flag that is read as set is not stored again.
//   scene_zonal_tables      zone[row[z]] = z for the present zones (row = the exclusive scan of present: ascending zone id), and the
//                           neutral element in every row of the tables.
//   scene_zonal_accumulate  three launches.  The extremes are compared as keys k(v) = bits ^ (bits >> 31 ? 0xFFFFFFFF : 0x80000000),
//                           an order-preserving map of the floats onto uint32 in which -0.0 < +0.0: the first launch turns the two
//                           tables into keys in place, the last turns them back.  Between them zonal_accumulate_kernel: a workgroup
//                           takes ZN_PER_BLOCK consecutive pixels, a wave 64 of them at a time.
//                             1. Inside the wave consecutive lanes with one zone form a run; a run also ends where a row of the scene
//                                ends, so a run lies in one row and its geometry is closed form: count = its length, bbox = (x of its
//                                first lane, y, x of its last lane, y), sum_x = (x_first + x_last) * length / 2, sum_y = y * length.
//                                Per band the run's finite count is a popcount of a ballot, its key extremes and its sum of q(v) a
//                                segmented Hillis-Steele scan over the run (six shuffle steps); a wave without a finite value in the
//                                band skips the band.  The run's last lane holds the run's totals.
//                             2. That lane adds them into the workgroup's table in LDS: ZN_SLOTS slots keyed by zone, one probe at
//                                slot (zone * 2654435761 mod 2^32) >> 26; a slot held by another zone sends the run straight to the
//                                global tables.
//                             3. After a barrier every used slot issues one global atomic per statistic.
//                           The background of a flood map, millions of pixels of one zone, thus costs one global atomic per statistic
//                           per 4096 pixels, not per pixel.  Global atomics are agent scope, LDS atomics workgroup scope; no workgroup
//                           reads what another accumulates.  q(v) = (int64) rintf(clamp(v, -L, L) * 2^frac_bits), L = 2^(32 -
//                           frac_bits): |q| <= 2^32 and at most 2^31 - 1 pixels, so int64 never overflows.
#include "common.h"
#include "../../include/ksmi.h"
#include "errors.h"

namespace {

constexpr int ZN_MAX_B = 8;
constexpr int ZN_PER_BLOCK = 4096;             // pixels per workgroup of the mark and the accumulate pass
constexpr int ZN_SLOTS = 64;                   // zones a workgroup combines in LDS
constexpr int64_t MAX_PIXELS = 0x7fffffff;
constexpr uint32_t KEY_POS_INF = 0xff800000u;  // the key of +inf: above the key of every finite value
constexpr uint32_t KEY_NEG_INF = 0x007fffffu;  // the key of -inf: below them
constexpr int32_t BBOX_FAR = 0x7fffffff;

__device__ __forceinline__ uint32_t key_of_bits(uint32_t b) { return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u); }
__device__ __forceinline__ uint32_t bits_of_key(uint32_t k) { return k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu); }
__device__ __forceinline__ bool is_finite_bits(uint32_t b) { return (b & 0x7f800000u) != 0x7f800000u; }
__device__ __forceinline__ int slot_of(int32_t z) { return (int)((uint32_t)z * 2654435761u >> 26); }        // 6 bits: ZN_SLOTS
static_assert(ZN_SLOTS == 64, "the slot hash keeps 6 bits");

// the zone of pixel p, or -1 where p is skipped or past the scene
__device__ __forceinline__ int32_t zone_at(const int32_t* __restrict__ zones, const unsigned char* __restrict__ where, int64_t p, int HW) {
  if (p >= HW) return -1;
  const int32_t z = zones[p];
  if ((unsigned)z >= (unsigned)HW) return -1;
  if (where && !where[p]) return -1;
  return z;
}

template <typename T> __device__ __forceinline__ void g_add(T* a, T v) { __hip_atomic_fetch_add(a, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
template <typename T> __device__ __forceinline__ void g_min(T* a, T v) { __hip_atomic_fetch_min(a, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
template <typename T> __device__ __forceinline__ void g_max(T* a, T v) { __hip_atomic_fetch_max(a, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
template <typename T> __device__ __forceinline__ void l_add(T* a, T v) { __hip_atomic_fetch_add(a, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
template <typename T> __device__ __forceinline__ void l_min(T* a, T v) { __hip_atomic_fetch_min(a, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
template <typename T> __device__ __forceinline__ void l_max(T* a, T v) { __hip_atomic_fetch_max(a, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

__global__ __launch_bounds__(256) void zonal_mark_kernel(const int32_t* __restrict__ zones, const unsigned char* __restrict__ where, int HW,
                                                         int32_t* __restrict__ present) {
  __shared__ int32_t s_key[ZN_SLOTS];                                  // the zones this workgroup has marked already
  if (threadIdx.x < ZN_SLOTS) s_key[threadIdx.x] = -1;
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * ZN_PER_BLOCK;
  for (int j = 0; j < ZN_PER_BLOCK / 256; ++j) {
    if (base + j * 256 >= HW) break;                                   // the same answer in every thread
    const int64_t p = base + j * 256 + threadIdx.x;
    const int32_t z = zone_at(zones, where, p, HW);                    // every lane takes part in the shuffle
    const int32_t prev = __shfl_up(z, 1);
    if (z >= 0 && ((threadIdx.x & 63) == 0 || prev != z)) {            // only the first lane of a run goes on
      const int s = slot_of(z);
      const int32_t held = __hip_atomic_load(&s_key[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      const bool marked = held == z || (held == -1 && atomicCAS(&s_key[s], -1, z) == z);      // by this workgroup, before
      // stores to one address serialise, loads of it do not: a flag that is seen set is not stored again (all stores write 1)
      if (!marked && !__hip_atomic_load(present + z, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        __hip_atomic_store(present + z, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

__global__ __launch_bounds__(256) void zonal_emit_kernel(const int32_t* __restrict__ present, const int32_t* __restrict__ row, int HW, int N,
                                                         int32_t* __restrict__ zone) {
  const int64_t z = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (z >= HW || !present[z]) return;
  const int32_t r = row[z];
  if ((unsigned)r < (unsigned)N) zone[r] = (int32_t)z;                 // a row that is none addresses nothing
}

__global__ __launch_bounds__(256) void zonal_init_kernel(int N, int B, int32_t* __restrict__ count, int32_t* __restrict__ bbox,
                                                         int64_t* __restrict__ sum_x, int64_t* __restrict__ sum_y, int32_t* __restrict__ valid,
                                                         uint32_t* __restrict__ vmin, uint32_t* __restrict__ vmax, int64_t* __restrict__ vsum) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= N) return;
  count[r] = 0;
  bbox[4 * r + 0] = BBOX_FAR;
  bbox[4 * r + 1] = BBOX_FAR;
  bbox[4 * r + 2] = -1;
  bbox[4 * r + 3] = -1;
  sum_x[r] = 0;
  sum_y[r] = 0;
  for (int b = 0; b < B; ++b) {
    const int64_t i = (int64_t)b * N + r;
    valid[i] = 0;
    vmin[i] = 0x7f800000u;                     // +inf
    vmax[i] = 0xff800000u;                     // -inf
    vsum[i] = 0;
  }
}

// float bits <-> keys, in place, over the B * N cells of the two extreme tables
__global__ __launch_bounds__(256) void zonal_keys_kernel(int64_t n, int decode, uint32_t* __restrict__ vmin, uint32_t* __restrict__ vmax) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  vmin[i] = decode ? bits_of_key(vmin[i]) : key_of_bits(vmin[i]);
  vmax[i] = decode ? bits_of_key(vmax[i]) : key_of_bits(vmax[i]);
}

__global__ __launch_bounds__(256) void zonal_accumulate_kernel(const int32_t* __restrict__ zones, const unsigned char* __restrict__ where,
                                                               const float* __restrict__ values, int B, int Ws, int HW, float scale, float limit,
                                                               const int32_t* __restrict__ row, int N, int32_t* __restrict__ count,
                                                               int32_t* __restrict__ bbox, int64_t* __restrict__ sum_x, int64_t* __restrict__ sum_y,
                                                               int32_t* __restrict__ valid, uint32_t* __restrict__ kmin, uint32_t* __restrict__ kmax,
                                                               int64_t* __restrict__ vsum) {
  __shared__ int32_t s_key[ZN_SLOTS], s_cnt[ZN_SLOTS], s_x0[ZN_SLOTS], s_y0[ZN_SLOTS], s_x1[ZN_SLOTS], s_y1[ZN_SLOTS];
  __shared__ int64_t s_sx[ZN_SLOTS], s_sy[ZN_SLOTS];
  __shared__ int32_t s_valid[ZN_MAX_B][ZN_SLOTS];
  __shared__ uint32_t s_min[ZN_MAX_B][ZN_SLOTS], s_max[ZN_MAX_B][ZN_SLOTS];
  __shared__ int64_t s_sum[ZN_MAX_B][ZN_SLOTS];
  const int tid = (int)threadIdx.x;
  if (tid < ZN_SLOTS) {
    s_key[tid] = -1;
    s_cnt[tid] = 0;
    s_x0[tid] = BBOX_FAR;
    s_y0[tid] = BBOX_FAR;
    s_x1[tid] = -1;
    s_y1[tid] = -1;
    s_sx[tid] = 0;
    s_sy[tid] = 0;
  }
  for (int i = tid; i < B * ZN_SLOTS; i += 256) {
    (&s_valid[0][0])[i] = 0;
    (&s_min[0][0])[i] = KEY_POS_INF;
    (&s_max[0][0])[i] = KEY_NEG_INF;
    (&s_sum[0][0])[i] = 0;
  }
  __syncthreads();
  const int lane = tid & 63;
  const uint64_t upto = lane == 63 ? ~0ull : (2ull << lane) - 1;       // lanes 0 .. lane
  const int64_t base = (int64_t)blockIdx.x * ZN_PER_BLOCK;
  for (int j = 0; j < ZN_PER_BLOCK / 256; ++j) {
    const int64_t p = base + j * 256 + tid;
    if (base + j * 256 >= HW) break;                                   // the same answer in every thread
    const int32_t z = zone_at(zones, where, p, HW);                    // every lane of the wave goes on: -1 is no zone
    const int y = (int)((uint32_t)(p < HW ? p : 0) / (uint32_t)Ws), x = (int)((p < HW ? p : 0) - (int64_t)y * Ws);
    const int32_t prev = __shfl_up(z, 1);
    const bool head = lane == 0 || prev != z || x == 0;                // a run never wraps a row end
    const uint64_t heads = __ballot(head);
    const int first = 63 - __builtin_clzll(heads & upto);              // the head of this lane's run (bit 0 of heads is always set)
    const bool tail = lane == 63 || ((heads >> (lane + 1)) & 1ull);
    const bool emit = tail && z >= 0;                                  // this lane ends a run of a zone: it holds the run's totals
    const int len = lane - first + 1, ahead = lane - first;
    int s = 0;
    int32_t r = -1;
    bool shared = false;
    if (emit) {
      s = slot_of(z);
      const int32_t was = atomicCAS(&s_key[s], -1, z);
      shared = was == -1 || was == z;
      if (!shared) {
        r = row[z];
        if ((unsigned)r >= (unsigned)N) r = -1;                        // a row that is none addresses nothing
      }
      const int x0 = x - len + 1;
      const int64_t sx = ((int64_t)x0 + x) * len / 2, sy = (int64_t)y * len;      // (x0 + x) * len is even
      if (shared) {
        l_add(&s_cnt[s], len);
        l_min(&s_x0[s], x0);
        l_min(&s_y0[s], y);
        l_max(&s_x1[s], x);
        l_max(&s_y1[s], y);
        l_add(&s_sx[s], sx);
        l_add(&s_sy[s], sy);
      } else if (r >= 0) {
        g_add(&count[r], len);
        g_min(&bbox[4 * r + 0], x0);
        g_min(&bbox[4 * r + 1], y);
        g_max(&bbox[4 * r + 2], x);
        g_max(&bbox[4 * r + 3], y);
        g_add(&sum_x[r], sx);
        g_add(&sum_y[r], sy);
      }
    }
    for (int b = 0; b < B; ++b) {
      const uint32_t bits = z >= 0 ? __float_as_uint(values[(int64_t)b * HW + p]) : 0x7fc00000u;
      const bool fin = is_finite_bits(bits);
      const uint64_t fins = __ballot(fin);
      if (!fins) continue;                                             // the same answer in every lane of the wave
      uint32_t lo = fin ? key_of_bits(bits) : KEY_POS_INF, hi = fin ? key_of_bits(bits) : KEY_NEG_INF;
      long long q = 0;
      if (fin) {
        const float v = __uint_as_float(bits);
        q = (long long)rintf(fminf(fmaxf(v, -limit), limit) * scale);
      }
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {                               // segmented inclusive scan: lanes first .. lane
        const uint32_t lo2 = __shfl_up(lo, d), hi2 = __shfl_up(hi, d);
        const long long q2 = __shfl_up(q, d);
        if (ahead >= d) {
          lo = min(lo, lo2);
          hi = max(hi, hi2);
          q += q2;
        }
      }
      const int nv = __builtin_popcountll(fins & upto & ~((1ull << first) - 1));
      if (!emit || !nv) continue;
      if (shared) {
        l_add(&s_valid[b][s], nv);
        l_min(&s_min[b][s], lo);
        l_max(&s_max[b][s], hi);
        l_add(&s_sum[b][s], (int64_t)q);
      } else if (r >= 0) {
        const int64_t i = (int64_t)b * N + r;
        g_add(&valid[i], nv);
        g_min(&kmin[i], lo);
        g_max(&kmax[i], hi);
        g_add(&vsum[i], (int64_t)q);
      }
    }
  }
  __syncthreads();
  const int s = tid & (ZN_SLOTS - 1), part = tid >> 6;                 // four threads per slot share its statistics
  const int32_t z = s_key[s];
  if (z < 0) return;
  const int32_t r = row[z];
  if ((unsigned)r >= (unsigned)N) return;
  if (part == 0) {
    g_add(&count[r], s_cnt[s]);
    g_min(&bbox[4 * r + 0], s_x0[s]);
    g_min(&bbox[4 * r + 1], s_y0[s]);
  } else if (part == 1) {
    g_max(&bbox[4 * r + 2], s_x1[s]);
    g_max(&bbox[4 * r + 3], s_y1[s]);
  } else if (part == 2) {
    g_add(&sum_x[r], s_sx[s]);
  } else {
    g_add(&sum_y[r], s_sy[s]);
  }
  for (int b = part; b < B; b += 4) {
    if (!s_valid[b][s]) continue;
    const int64_t i = (int64_t)b * N + r;
    g_add(&valid[i], s_valid[b][s]);
    g_min(&kmin[i], s_min[b][s]);
    g_max(&kmax[i], s_max[b][s]);
    g_add(&vsum[i], s_sum[b][s]);
  }
}

unsigned blocks_of(int64_t total, int per = 256) { return (unsigned)((total + per - 1) / per); }

}  // namespace

int ksmi_scene_zonal_mark(const int32_t* zones_i32, const unsigned char* where_u8, int64_t HW, int32_t* present_i32, void* stream) {
  if (HW < 0 || HW > MAX_PIXELS) return ksmi_fail(KSMI_E_ARG, "scene_zonal_mark: 0 <= HW <= 2^31 - 1 pixels");
  if (HW == 0) return 0;
  if (!zones_i32 || !present_i32) return ksmi_fail(KSMI_E_ARG, "scene_zonal_mark: null pointer");
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(present_i32, 0, (size_t)HW * sizeof(int32_t), st) != hipSuccess) return ksmi_check_launch("scene_zonal_mark");
  KSMI_NOTE(zonal_mark_kernel);
  hipLaunchKernelGGL(zonal_mark_kernel, dim3(blocks_of(HW, ZN_PER_BLOCK)), dim3(256), 0, st, zones_i32, where_u8, (int)HW, present_i32);
  return ksmi_check_launch("scene_zonal_mark");
}

int ksmi_scene_zonal_tables(const int32_t* present_i32, const int32_t* row_i32, int64_t HW, int64_t N, int B, int32_t* zone_i32,
                            int32_t* count_i32, int32_t* bbox_i32, int64_t* sum_x_i64, int64_t* sum_y_i64, int32_t* valid_i32, float* vmin_f32,
                            float* vmax_f32, int64_t* vsum_i64, void* stream) {
  if (HW < 0 || HW > MAX_PIXELS) return ksmi_fail(KSMI_E_ARG, "scene_zonal_tables: 0 <= HW <= 2^31 - 1 pixels");
  if (N < 0 || N > HW) return ksmi_fail(KSMI_E_ARG, "scene_zonal_tables: 0 <= N <= HW rows");
  if (B < 0 || B > ZN_MAX_B) return ksmi_fail(KSMI_E_ARG, "scene_zonal_tables: 0 <= B <= 8 bands");
  if (HW == 0 || N == 0) return 0;
  if (!present_i32 || !row_i32 || !zone_i32 || !count_i32 || !bbox_i32 || !sum_x_i64 || !sum_y_i64 ||
      (B > 0 && (!valid_i32 || !vmin_f32 || !vmax_f32 || !vsum_i64)))
    return ksmi_fail(KSMI_E_ARG, "scene_zonal_tables: null pointer");
  hipStream_t st = (hipStream_t)stream;
  KSMI_NOTE(zonal_emit_kernel);
  hipLaunchKernelGGL(zonal_emit_kernel, dim3(blocks_of(HW)), dim3(256), 0, st, present_i32, row_i32, (int)HW, (int)N, zone_i32);
  KSMI_NOTE(zonal_init_kernel);
  hipLaunchKernelGGL(zonal_init_kernel, dim3(blocks_of(N)), dim3(256), 0, st, (int)N, B, count_i32, bbox_i32, sum_x_i64, sum_y_i64, valid_i32,
                     (uint32_t*)vmin_f32, (uint32_t*)vmax_f32, vsum_i64);
  return ksmi_check_launch("scene_zonal_tables");
}

int ksmi_scene_zonal_accumulate(const int32_t* zones_i32, const unsigned char* where_u8, const float* values_f32, int B, int Hs, int Ws,
                                int frac_bits, const int32_t* row_i32, int64_t N, int32_t* count_i32, int32_t* bbox_i32, int64_t* sum_x_i64,
                                int64_t* sum_y_i64, int32_t* valid_i32, float* vmin_f32, float* vmax_f32, int64_t* vsum_i64, void* stream) {
  if (Hs < 0 || Ws < 0) return ksmi_fail(KSMI_E_ARG, "scene_zonal_accumulate: a scene of Hs >= 0 by Ws >= 0 pixels");
  const int64_t HW = (int64_t)Hs * Ws;
  if (HW > MAX_PIXELS) return ksmi_fail(KSMI_E_ARG, "scene_zonal_accumulate: more than 2^31 - 1 pixels");
  if (N < 0 || N > HW) return ksmi_fail(KSMI_E_ARG, "scene_zonal_accumulate: 0 <= N <= Hs * Ws rows");
  if (B < 0 || B > ZN_MAX_B) return ksmi_fail(KSMI_E_ARG, "scene_zonal_accumulate: 0 <= B <= 8 bands");
  if (frac_bits < 0 || frac_bits > 30) return ksmi_fail(KSMI_E_ARG, "scene_zonal_accumulate: frac_bits in 0 .. 30");
  if (HW == 0 || N == 0) return 0;
  if (!zones_i32 || !row_i32 || !count_i32 || !bbox_i32 || !sum_x_i64 || !sum_y_i64 ||
      (B > 0 && (!values_f32 || !valid_i32 || !vmin_f32 || !vmax_f32 || !vsum_i64)))
    return ksmi_fail(KSMI_E_ARG, "scene_zonal_accumulate: null pointer");
  hipStream_t st = (hipStream_t)stream;
  uint32_t* kmin = (uint32_t*)vmin_f32;
  uint32_t* kmax = (uint32_t*)vmax_f32;
  const int64_t cells = (int64_t)B * N;
  if (B > 0) {
    KSMI_NOTE(zonal_keys_kernel);
    hipLaunchKernelGGL(zonal_keys_kernel, dim3(blocks_of(cells)), dim3(256), 0, st, cells, 0, kmin, kmax);
  }
  KSMI_NOTE(zonal_accumulate_kernel);
  hipLaunchKernelGGL(zonal_accumulate_kernel, dim3(blocks_of(HW, ZN_PER_BLOCK)), dim3(256), 0, st, zones_i32, where_u8, values_f32, B, Ws,
                     (int)HW, ldexpf(1.0f, frac_bits), ldexpf(1.0f, 32 - frac_bits), row_i32, (int)N, count_i32, bbox_i32, sum_x_i64, sum_y_i64,
                     valid_i32, kmin, kmax, vsum_i64);
  if (B > 0) hipLaunchKernelGGL(zonal_keys_kernel, dim3(blocks_of(cells)), dim3(256), 0, st, cells, 1, kmin, kmax);
  return ksmi_check_launch("scene_zonal_accumulate");
}
