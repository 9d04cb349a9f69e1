// Zones from a vector layer, on the device (kurosiwo_amd/scene.py: rasterize_zones; predict.py --zones): the polygons of F features,
// given as one table of edges, become the int32 zone raster [Hs][Ws] that zonal.hip and quantile.hip reduce.  Integers only: the
// result depends neither on launch geometry nor on arrival order and equals tests/zones_ref.py bit for bit.  No float arithmetic, no
// lock, no grid-wide wait; every loop is bounded by a size the host passed; the host reads one pair of integers (the number of
// crossings and the number of edges refused) between scene_zone_rows and scene_zone_crossings.
//
// Vertices are int32 in units of 1/256 pixel, x to the right and y down; the centre of pixel (x, y) is (256 x + 128, 256 y + 128).
// An edge (x0, y0, x1, y1) of feature f with y0 != y1, oriented so that y0 < y1, crosses the scanlines y with y0 <= 256 y + 128 < y1
// (half open) and 0 <= y < Hs.  With dy = y1 - y0, dx = x1 - x0, cy = 256 y + 128 its crossing column is c = clamp(ceil((x0 * dy +
// (cy - y0) * dx - 128 * dy) / (256 * dy)), 0, Ws): the first column whose centre is at or right of the crossing, in exact int64
// (every |coordinate| <= 3 * 32767 * 256, so every product stays under 2^53).  The crossing's composite is f << 32 | y << 16 | c.
// Sorted ascending, the composites 2k and 2k + 1 share f and y (closed rings cross a scanline an even number of times) and bound the
// span [c0, c1) of row y: the even-odd rule per feature.  zones[y][x] = the smallest f with a span over (y, x), -1 without one.
//
//   scene_zone_rows       one thread per edge: counts[e] = the scanlines edge e crosses inside the scene; info[0] += the counts (one
//                         int64 atomic per workgroup: integer adds commute), info[1] += the edges refused (a coordinate beyond the
//                         bound or a feature outside 0 .. F - 1), which count 0.  ksmi_scan_i32 of the counts gives the offsets.
//   scene_zone_crossings  one thread per crossing j: its edge is the last e with offsets[e] <= j (a binary search, so an edge of 32767
//                         rows does not serialise one thread), its scanline the edge's first one + j - offsets[e].  Composites past
//                         X (the caller pads the buffer up to F elements for the sort) are all ones and sort last.
//   (the sort)            ksmi_scene_quantile_sort with N = F: the feature is its row field, y << 16 | c its value field.
//   scene_zone_fill       the raster is set to all ones (-1 as int32); one wave64 per span, lanes striding over it, writes with an
//                         unsigned atomic minimum of f in global memory.  A pair that is no span of the scene addresses nothing.
#include "common.h"
#include "../../include/ksmi.h"
#include "errors.h"

namespace {

constexpr int ZR_MAX_SIDE = 32767;                           // scene.MAX_ZONE_SIDE: y and c each fit 15 bits of the composite
constexpr int ZR_MAX_COORD = 3 * ZR_MAX_SIDE * 256;          // scene.MAX_ZONE_COORD
constexpr int ZR_EDGES_PER_THREAD = 4;                       // scene_zone_rows: 1024 edges and one atomic pair per workgroup
constexpr int64_t MAX_COUNT = 0x7fffffff;
constexpr uint64_t ZR_LAST = ~0ull;

struct ZrEdge {
  int x0, y0, x1, y1;                                        // oriented: y0 < y1
  int ylo, yhi;                                              // the scanlines ylo .. yhi - 1 of the scene are crossed
};

// edge e, oriented, with its scanlines; false when it is refused (then it crosses nothing)
__device__ __forceinline__ bool edge_rows(const int32_t* __restrict__ edges, int64_t e, int Hs, ZrEdge& out) {
  const int4 v = *reinterpret_cast<const int4*>(edges + 4 * e);
  const int top = max(max(v.x, v.y), max(v.z, v.w)), bottom = min(min(v.x, v.y), min(v.z, v.w));
  const bool ok = top <= ZR_MAX_COORD && bottom >= -ZR_MAX_COORD;
  const bool up = v.y <= v.w;
  out.x0 = up ? v.x : v.z;
  out.y0 = up ? v.y : v.w;
  out.x1 = up ? v.z : v.x;
  out.y1 = up ? v.w : v.y;
  // y0 <= 256 y + 128 < y1  <=>  ceil((y0 - 128) / 256) <= y < ceil((y1 - 128) / 256); >> 8 is the floor
  const int lo = ok ? (out.y0 - 128 + 255) >> 8 : 0, hi = ok ? (out.y1 - 128 + 255) >> 8 : 0;
  out.ylo = max(lo, 0);
  out.yhi = max(min(hi, Hs), out.ylo);
  return ok;
}

__global__ __launch_bounds__(256) void zone_rows_kernel(const int32_t* __restrict__ edges, const int32_t* __restrict__ feature, int64_t E,
                                                        int64_t F, int Hs, int32_t* __restrict__ counts, int64_t* __restrict__ info) {
  __shared__ int s_sum[4], s_bad[4];
  int sum = 0, bad = 0;
  const int64_t base = (int64_t)blockIdx.x * (256 * ZR_EDGES_PER_THREAD);
#pragma unroll
  for (int j = 0; j < ZR_EDGES_PER_THREAD; ++j) {
    const int64_t e = base + j * 256 + threadIdx.x;
    if (e >= E) continue;
    ZrEdge g;
    const bool ok = edge_rows(edges, e, Hs, g) && (uint64_t)(int64_t)feature[e] < (uint64_t)F;
    const int n = ok ? g.yhi - g.ylo : 0;
    counts[e] = n;
    sum += n;                                                // at most 4 * 32767
    bad += ok ? 0 : 1;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sum += __shfl_down(sum, o);                              // lane 0 of a wave: at most 256 * 32767 < 2^31
    bad += __shfl_down(bad, o);
  }
  if ((threadIdx.x & 63) == 0) {
    s_sum[threadIdx.x >> 6] = sum;
    s_bad[threadIdx.x >> 6] = bad;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int64_t total = (int64_t)s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
    const int64_t refused = (int64_t)s_bad[0] + s_bad[1] + s_bad[2] + s_bad[3];
    if (total) __hip_atomic_fetch_add(&info[0], total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (refused) __hip_atomic_fetch_add(&info[1], refused, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// floor(a / b) for b > 0
__device__ __forceinline__ int64_t floor_div(int64_t a, int64_t b) {
  const int64_t q = a / b;
  return q - ((a % b) < 0 ? 1 : 0);
}

__global__ __launch_bounds__(256) void zone_crossings_kernel(const int32_t* __restrict__ edges, const int32_t* __restrict__ feature,
                                                             const int32_t* __restrict__ offsets, int64_t E, int64_t X, int Hs, int Ws,
                                                             uint64_t* __restrict__ keys, int64_t n_keys) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n_keys) return;
  uint64_t c = ZR_LAST;
  if (j < X) {
    int64_t lo = 0, hi = E;                                  // the last e with offsets[e] <= j: E <= 2^31 - 1, so 32 halvings end it
    for (int it = 0; it < 32 && hi - lo > 1; ++it) {
      const int64_t mid = (lo + hi) >> 1;
      if ((int64_t)offsets[mid] <= j) lo = mid;
      else hi = mid;
    }
    ZrEdge g;
    const bool ok = edge_rows(edges, lo, Hs, g);
    const int64_t y = (int64_t)g.ylo + (j - (int64_t)offsets[lo]);
    const int32_t f = feature[lo];
    if (ok && f >= 0 && y >= g.ylo && y < g.yhi) {           // offsets that are no scan of this table's counts give no crossing
      const int64_t dy = (int64_t)g.y1 - g.y0, dx = (int64_t)g.x1 - g.x0, cy = 256 * y + 128;
      const int64_t num = (int64_t)g.x0 * dy + (cy - g.y0) * dx - 128 * dy, den = 256 * dy;
      const int64_t col = min(max(floor_div(num + den - 1, den), (int64_t)0), (int64_t)Ws);
      c = ((uint64_t)(uint32_t)f << 32) | ((uint64_t)y << 16) | (uint64_t)col;
    }
  }
  keys[j] = c;
}

__global__ __launch_bounds__(256) void zone_fill_kernel(const uint64_t* __restrict__ sorted, int64_t spans, int64_t F, int Hs, int Ws,
                                                        uint32_t* __restrict__ zones) {
  const int64_t k = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);      // one wave64 per span
  if (k >= spans) return;
  const uint64_t a = sorted[2 * k], b = sorted[2 * k + 1];
  const uint32_t f = (uint32_t)(a >> 32);
  const int y = (int)((a >> 16) & 0xffffu), c0 = (int)(a & 0xffffu), c1 = (int)(b & 0xffffu);
  if ((a >> 16) != (b >> 16) || (int64_t)f >= F || y >= Hs || c1 > Ws) return;      // no span of this scene: nothing is addressed
  uint32_t* row = zones + (int64_t)y * Ws;
  const int trips = (Ws + 63) >> 6;
  int x = c0 + (int)(threadIdx.x & 63);
  for (int t = 0; t < trips && x < c1; ++t, x += 64)
    __hip_atomic_fetch_min(row + x, f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

unsigned blocks_of(int64_t total, int per = 256) { return (unsigned)((total + per - 1) / per); }

// 0, or KSMI_E_ARG with a message that names the entry point
int bad_scene(const char* entry, int64_t E, int64_t F, int Hs, int Ws) {
  const char* what = E < 0 || E > MAX_COUNT ? "0 <= E <= 2^31 - 1 edges"
                     : F < 0 || F > MAX_COUNT ? "0 <= F <= 2^31 - 1 features"
                     : Hs < 0 || Hs > ZR_MAX_SIDE || Ws < 0 || Ws > ZR_MAX_SIDE ? "a scene of 0 .. 32767 by 0 .. 32767 pixels"
                                                                                : nullptr;
  if (!what) return 0;
  char msg[96];
  snprintf(msg, sizeof(msg), "%s: %s", entry, what);
  return ksmi_fail(KSMI_E_ARG, msg);
}

}  // namespace

int ksmi_scene_zone_rows(const int32_t* edges_i32, const int32_t* edge_feature_i32, int64_t E, int64_t F, int Hs, int Ws, int32_t* counts_i32,
                         int64_t* info_i64, void* stream) {
  if (const int rc = bad_scene("scene_zone_rows", E, F, Hs, Ws)) return rc;
  if (!info_i64 || (E > 0 && (!edges_i32 || !edge_feature_i32 || !counts_i32))) return ksmi_fail(KSMI_E_ARG, "scene_zone_rows: null pointer");
  if ((uintptr_t)edges_i32 & 15) return ksmi_fail(KSMI_E_ARG, "scene_zone_rows: the edge table is 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(info_i64, 0, 2 * sizeof(int64_t), st) != hipSuccess) return ksmi_check_launch("scene_zone_rows");
  if (E == 0) return ksmi_check_launch("scene_zone_rows");
  KSMI_NOTE(zone_rows_kernel);
  hipLaunchKernelGGL(zone_rows_kernel, dim3(blocks_of(E, 256 * ZR_EDGES_PER_THREAD)), dim3(256), 0, st, edges_i32, edge_feature_i32, E, F, Hs,
                     counts_i32, info_i64);
  return ksmi_check_launch("scene_zone_rows");
}

int ksmi_scene_zone_crossings(const int32_t* edges_i32, const int32_t* edge_feature_i32, const int32_t* offsets_i32, int64_t E, int64_t X, int Hs,
                              int Ws, uint64_t* keys_u64, int64_t n_keys, void* stream) {
  if (const int rc = bad_scene("scene_zone_crossings", E, 0, Hs, Ws)) return rc;
  if (X < 0 || n_keys < X || n_keys > MAX_COUNT) return ksmi_fail(KSMI_E_ARG, "scene_zone_crossings: 0 <= X <= n_keys <= 2^31 - 1 composites");
  if (X > 0 && E == 0) return ksmi_fail(KSMI_E_ARG, "scene_zone_crossings: crossings without an edge");
  if (n_keys == 0) return 0;
  if (!keys_u64 || (X > 0 && (!edges_i32 || !edge_feature_i32 || !offsets_i32))) return ksmi_fail(KSMI_E_ARG, "scene_zone_crossings: null pointer");
  if ((uintptr_t)edges_i32 & 15) return ksmi_fail(KSMI_E_ARG, "scene_zone_crossings: the edge table is 16-byte aligned");
  KSMI_NOTE(zone_crossings_kernel);
  hipLaunchKernelGGL(zone_crossings_kernel, dim3(blocks_of(n_keys)), dim3(256), 0, (hipStream_t)stream, edges_i32, edge_feature_i32, offsets_i32,
                     E, X, Hs, Ws, keys_u64, n_keys);
  return ksmi_check_launch("scene_zone_crossings");
}

int ksmi_scene_zone_fill(const uint64_t* sorted_u64, int64_t X, int64_t F, int Hs, int Ws, int32_t* zones_i32, void* stream) {
  if (const int rc = bad_scene("scene_zone_fill", 0, F, Hs, Ws)) return rc;
  if (X < 0 || X > MAX_COUNT || (X & 1)) return ksmi_fail(KSMI_E_ARG, "scene_zone_fill: X is an even number of crossings, 0 .. 2^31 - 2");
  const int64_t HW = (int64_t)Hs * Ws;
  if (HW == 0) return 0;
  if (!zones_i32 || (X > 0 && !sorted_u64)) return ksmi_fail(KSMI_E_ARG, "scene_zone_fill: null pointer");
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(zones_i32, 0xff, (size_t)HW * sizeof(int32_t), st) != hipSuccess) return ksmi_check_launch("scene_zone_fill");
  if (X == 0 || F == 0) return ksmi_check_launch("scene_zone_fill");
  KSMI_NOTE(zone_fill_kernel);
  hipLaunchKernelGGL(zone_fill_kernel, dim3(blocks_of(X / 2, 4)), dim3(256), 0, st, sorted_u64, X / 2, F, Hs, Ws, (uint32_t*)zones_i32);
  return ksmi_check_launch("scene_zone_fill");
}
