// Flood depth for a scene's class map, on the device (kurosiwo_amd/scene.py: nearest_feature, flood_depth; predict.py --depth_out):
// the exact Euclidean nearest-feature transform of a uint8 raster [Hs][Ws], and around it the three steps of FwDET (Cohen et al.
// 2018): the DEM at the flood boundary, every flooded cell given the elevation of its nearest boundary cell, minus the DEM, clamped
// at zero.  The transform is integers throughout -- no float arithmetic, no atomics, nothing read on the host, no grid-wide wait; every
// loop is bounded by Hs or Ws -- so its results do not depend on launch geometry and equal tests/depth_ref.py bit for bit.
//
//   scene_edt_cols   near_y[y][x] = the row of the nearest feature (mask != 0) in column x, the smaller row when the one above and
//                    the one below are equally far, -1 when the column has none.  Consecutive threads along x; a column is cut into
//                    y-tiles with a carry (the nearest feature row above the tile and below it, from a table of every tile's first
//                    and last feature row in LDS), so that no dependent chain is longer than a tile: a down sweep that carries the
//                    last feature row and writes it, an up sweep that carries the next one, reads what the same thread wrote and
//                    keeps the nearer.  All global accesses of a wave are runs of consecutive cells.
//   scene_edt_rows   for pixel (y, x): the lexicographic minimum of ((x - i)^2 + (y - near_y[y][i])^2, near_y[y][i] * Ws + i) over the
//                    columns i with near_y[y][i] >= 0.  Exact: a feature of column i at minimum distance from (y, x) is a
//                    column-nearest feature of row y, and of the two column ties the smaller row has the smaller index.  One
//                    workgroup per ROW_TILE pixels of one row; the row's near_y from ROW_HALO columns left of the tile to ROW_HALO
//                    right of it is staged in LDS, a column outside that window is read from global memory (a row may be far longer
//                    than the window).  Each pixel walks outward, d = 0, 1, 2, ... over i = x - d and x + d, while d * d <= best:
//                    "<=", so a tie at a smaller index is still seen.  d never passes max(x, Ws - 1 - x).  A pixel where where_u8 is
//                    given and zero is skipped (dist2 = 2^31 - 1, nearest = -1); a workgroup whose pixels are all skipped stages
//                    nothing.  Hs, Ws <= 32767: 2 * 32766^2 = 2147221512 fits int32 below the sentinel.
//   scene_select     out[p] = p's class is in the set: the water pixels, the `where` of the transform.
//   scene_shore      shore[p] = p is water, dem[p] is finite, and some 4-edge neighbour inside the scene is valid and not water.  A
//                    scene border or an invalid neighbour makes no shore: the water's real edge is not seen there (FwDET v2).
//   scene_depth      depth and water surface elevation from the transform of the shore; the one float operation is the subtraction.
#include "common.h"
#include "../../include/ksmi.h"
#include "errors.h"

namespace {

constexpr int EDT_MAX_SIDE = 32767;
constexpr int32_t EDT_FAR = 0x7fffffff;        // dist2 where there is no feature
constexpr int COL_BLOCK = 64;                  // columns per workgroup of the column pass: threadIdx.x, one wave wide
constexpr int COL_WAVES = 16;                  // waves per workgroup: threadIdx.y, each a y-tile at a time
constexpr int COL_MIN_TILE = 64;               // rows per y-tile, more when Hs would need more than COL_MAX_TILES of them
constexpr int COL_MAX_TILES = 128;
constexpr int ROW_TILE = 256;                  // pixels per workgroup of the row pass
constexpr int ROW_HALO = 896;                  // columns staged on either side of the tile
constexpr int ROW_WIN = ROW_TILE + 2 * ROW_HALO;
constexpr int64_t MAX_PIXELS = 0x7fffffff;
constexpr uint32_t QUIET_NAN = 0x7fc00000u;

__device__ __forceinline__ bool in_set(unsigned c, uint64_t mask) { return c < 63u && ((mask >> c) & 1ull); }
__device__ __forceinline__ bool is_finite_bits(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// One workgroup owns COL_BLOCK columns from top to bottom, cut into `tiles` tiles of `tile` rows; wave j takes the tiles j, j +
// COL_WAVES, ...  First every tile's first and last feature row go to LDS (rows fit int16).  Then a tile's carry is the last feature
// row of the nearest tile above that has one and the first feature row of the nearest tile below: at most `tiles` LDS reads, and
// the sweeps of a tile are `tile` rows long whatever Hs is.  No workgroup reads what another writes.
__global__ __launch_bounds__(COL_BLOCK * COL_WAVES) void edt_cols_kernel(const unsigned char* __restrict__ mask, int Hs, int Ws, int tile,
                                                                        int tiles, int32_t* near_y) {
  __shared__ short first[COL_MAX_TILES][COL_BLOCK], last[COL_MAX_TILES][COL_BLOCK];
  const int lx = (int)threadIdx.x, x = (int)blockIdx.x * COL_BLOCK + lx;
  const bool inside = x < Ws;
  const unsigned char* m = mask + (inside ? x : 0);
  int32_t* o = near_y + (inside ? x : 0);
  for (int t = (int)threadIdx.y; t < tiles; t += COL_WAVES) {
    int f = -1, l = -1;
    if (inside) {
      const int y1 = min(Hs, (t + 1) * tile);
#pragma unroll 8
      for (int y = t * tile; y < y1; ++y)
        if (m[(int64_t)y * Ws]) {
          if (f < 0) f = y;
          l = y;
        }
    }
    first[t][lx] = (short)f;
    last[t][lx] = (short)l;
  }
  __syncthreads();
  if (!inside) return;
  for (int t = (int)threadIdx.y; t < tiles; t += COL_WAVES) {
    int prev = -1, next = -1;
    for (int k = t - 1; k >= 0 && prev < 0; --k) prev = last[k][lx];
    for (int k = t + 1; k < tiles && next < 0; ++k) next = first[k][lx];
    const int y0 = t * tile, y1 = min(Hs, y0 + tile);
#pragma unroll 8
    for (int y = y0; y < y1; ++y) {
      const int64_t p = (int64_t)y * Ws;
      if (m[p]) prev = y;
      o[p] = prev;
    }
#pragma unroll 8
    for (int y = y1 - 1; y >= y0; --y) {
      const int64_t p = (int64_t)y * Ws;
      if (m[p]) next = y;
      const int up = o[p];                     // this thread's own store of the down sweep
      if (next >= 0 && (up < 0 || next - y < y - up)) o[p] = next;    // strictly nearer: a tie keeps the smaller row
    }
  }
}

__global__ __launch_bounds__(ROW_TILE) void edt_rows_kernel(const int32_t* __restrict__ near_y, const unsigned char* __restrict__ where, int Hs,
                                                            int Ws, int32_t* __restrict__ dist2, int32_t* __restrict__ nearest) {
  __shared__ int32_t win[ROW_WIN];
  const int y = (int)blockIdx.y, x0 = (int)blockIdx.x * ROW_TILE, x = x0 + (int)threadIdx.x;
  const int64_t row = (int64_t)y * Ws;
  const bool inside = x < Ws;
  const bool active = inside && (!where || where[row + x]);
  if (!__syncthreads_or(active)) {             // the same answer in every thread: all leave or none
    if (inside) {
      dist2[row + x] = EDT_FAR;
      nearest[row + x] = -1;
    }
    return;
  }
  const int w0 = x0 - ROW_HALO;
  for (int j = threadIdx.x; j < ROW_WIN; j += ROW_TILE) {
    const int i = w0 + j;
    win[j] = (i >= 0 && i < Ws) ? near_y[row + i] : -1;
  }
  __syncthreads();
  if (!inside) return;
  int32_t best = EDT_FAR, arg = -1;
  if (active) {
    const int dmax = max(x, Ws - 1 - x);
    for (int d = 0; d <= dmax && d * d <= best; ++d) {
#pragma unroll
      for (int side = 0; side < 2; ++side) {
        if (side && d == 0) break;
        const int i = side ? x + d : x - d;
        if (i < 0 || i >= Ws) continue;
        const int j = i - w0;
        const int32_t ny = (unsigned)j < (unsigned)ROW_WIN ? win[j] : near_y[row + i];
        if ((unsigned)ny >= (unsigned)Hs) continue;                   // -1: no feature in this column; any other value is no row
        const int dy = y - ny;
        const int32_t dd = d * d + dy * dy, idx = ny * Ws + i;
        if (dd < best || (dd == best && idx < arg)) {
          best = dd;
          arg = idx;
        }
      }
    }
  }
  dist2[row + x] = best;
  nearest[row + x] = arg;
}

__global__ __launch_bounds__(256) void select_kernel(const unsigned char* __restrict__ cls, uint64_t mask, int64_t HW, unsigned char* __restrict__ out) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p < HW) out[p] = in_set(cls[p], mask) ? 1 : 0;
}

__global__ __launch_bounds__(256) void shore_kernel(const unsigned char* __restrict__ cls, const float* __restrict__ dem, uint64_t mask,
                                                    int invalid_class, int Hs, int Ws, unsigned char* __restrict__ shore) {
  const int64_t HW = (int64_t)Hs * Ws, p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= HW) return;
  unsigned char s = 0;
  if (in_set(cls[p], mask) && is_finite_bits(dem[p])) {
    const int y = (int)(p / Ws), x = (int)(p % Ws);
    const int64_t nb[4] = {y > 0 ? p - Ws : -1, x > 0 ? p - 1 : -1, x + 1 < Ws ? p + 1 : -1, y + 1 < Hs ? p + Ws : -1};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (nb[j] < 0) continue;
      const int c = cls[nb[j]];
      if (c != invalid_class && !in_set(c, mask)) s = 1;
    }
  }
  shore[p] = s;
}

__global__ __launch_bounds__(256) void depth_kernel(const unsigned char* __restrict__ cls, const float* __restrict__ dem,
                                                    const int32_t* __restrict__ nearest, uint64_t mask, int invalid_class, int64_t HW,
                                                    float* __restrict__ depth, float* __restrict__ wse) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= HW) return;
  const float nan = __uint_as_float(QUIET_NAN);
  const int c = cls[p];
  float d = nan, level = nan;
  if (in_set(c, mask)) {
    const int32_t n = nearest[p];
    if (n >= 0 && n < HW) {                    // an index that is no pixel addresses nothing
      level = dem[n];
      const float here = dem[p];
      if (is_finite_bits(here)) {
        const float diff = level - here;
        d = diff > 0.0f ? diff : 0.0f;
      }
    }
  } else if (c != invalid_class) {
    d = 0.0f;
  }
  if (c == invalid_class) d = nan;             // the first rule: not valid
  depth[p] = d;
  if (wse) wse[p] = level;
}

unsigned blocks_of(int64_t total, int per = 256) { return (unsigned)((total + per - 1) / per); }

}  // namespace

int ksmi_scene_edt_cols(const unsigned char* mask_u8, int Hs, int Ws, int32_t* near_y_i32, void* stream) {
  if (Hs < 1 || Ws < 1 || Hs > EDT_MAX_SIDE || Ws > EDT_MAX_SIDE) return ksmi_fail(KSMI_E_ARG, "scene_edt_cols: 1 <= Hs, Ws <= 32767");
  if (!mask_u8 || !near_y_i32) return ksmi_fail(KSMI_E_ARG, "scene_edt_cols: null pointer");
  const int need = (Hs + COL_MAX_TILES - 1) / COL_MAX_TILES, tile = need > COL_MIN_TILE ? need : COL_MIN_TILE;
  const int tiles = (Hs + tile - 1) / tile;    // <= COL_MAX_TILES: the table in LDS holds them all
  KSMI_NOTE(edt_cols_kernel);
  hipLaunchKernelGGL(edt_cols_kernel, dim3(blocks_of(Ws, COL_BLOCK)), dim3(COL_BLOCK, COL_WAVES), 0, (hipStream_t)stream, mask_u8, Hs, Ws, tile,
                     tiles, near_y_i32);
  return ksmi_check_launch("scene_edt_cols");
}

int ksmi_scene_edt_rows(const int32_t* near_y_i32, const unsigned char* where_u8, int Hs, int Ws, int32_t* dist2_i32, int32_t* nearest_i32,
                        void* stream) {
  if (Hs < 1 || Ws < 1 || Hs > EDT_MAX_SIDE || Ws > EDT_MAX_SIDE) return ksmi_fail(KSMI_E_ARG, "scene_edt_rows: 1 <= Hs, Ws <= 32767");
  if (!near_y_i32 || !dist2_i32 || !nearest_i32) return ksmi_fail(KSMI_E_ARG, "scene_edt_rows: null pointer");
  KSMI_NOTE(edt_rows_kernel);
  hipLaunchKernelGGL(edt_rows_kernel, dim3(blocks_of(Ws, ROW_TILE), (unsigned)Hs), dim3(ROW_TILE), 0, (hipStream_t)stream, near_y_i32, where_u8,
                     Hs, Ws, dist2_i32, nearest_i32);
  return ksmi_check_launch("scene_edt_rows");
}

int ksmi_scene_select(const unsigned char* classes_u8, int64_t select_mask, int64_t HW, unsigned char* out_u8, void* stream) {
  if (HW < 0 || HW > MAX_PIXELS) return ksmi_fail(KSMI_E_ARG, "scene_select: 0 <= HW <= 2^31 - 1 pixels");
  if (select_mask < 0) return ksmi_fail(KSMI_E_ARG, "scene_select: the mask selects classes 0 .. 62");
  if (HW == 0) return 0;
  if (!classes_u8 || !out_u8) return ksmi_fail(KSMI_E_ARG, "scene_select: null pointer");
  KSMI_NOTE(select_kernel);
  hipLaunchKernelGGL(select_kernel, dim3(blocks_of(HW)), dim3(256), 0, (hipStream_t)stream, classes_u8, (uint64_t)select_mask, HW, out_u8);
  return ksmi_check_launch("scene_select");
}

int ksmi_scene_shore(const unsigned char* classes_u8, const float* dem_f32, int64_t water_mask, int invalid_class, int Hs, int Ws,
                     unsigned char* shore_u8, void* stream) {
  if (Hs < 1 || Ws < 1 || invalid_class < 0 || invalid_class > 255)
    return ksmi_fail(KSMI_E_ARG, "scene_shore: a scene of Hs >= 1 by Ws >= 1 pixels, invalid_class in 0 .. 255");
  const int64_t HW = (int64_t)Hs * Ws;
  if (HW > MAX_PIXELS) return ksmi_fail(KSMI_E_ARG, "scene_shore: more than 2^31 - 1 pixels");
  if (water_mask < 0) return ksmi_fail(KSMI_E_ARG, "scene_shore: the mask selects classes 0 .. 62");
  if (!classes_u8 || !dem_f32 || !shore_u8) return ksmi_fail(KSMI_E_ARG, "scene_shore: null pointer");
  KSMI_NOTE(shore_kernel);
  hipLaunchKernelGGL(shore_kernel, dim3(blocks_of(HW)), dim3(256), 0, (hipStream_t)stream, classes_u8, dem_f32, (uint64_t)water_mask,
                     invalid_class, Hs, Ws, shore_u8);
  return ksmi_check_launch("scene_shore");
}

int ksmi_scene_depth(const unsigned char* classes_u8, const float* dem_f32, const int32_t* nearest_i32, int64_t water_mask, int invalid_class,
                     int64_t HW, float* depth_f32, float* wse_f32, void* stream) {
  if (HW < 0 || HW > MAX_PIXELS || invalid_class < 0 || invalid_class > 255)
    return ksmi_fail(KSMI_E_ARG, "scene_depth: 0 <= HW <= 2^31 - 1 pixels, invalid_class in 0 .. 255");
  if (water_mask < 0) return ksmi_fail(KSMI_E_ARG, "scene_depth: the mask selects classes 0 .. 62");
  if (HW == 0) return 0;
  if (!classes_u8 || !dem_f32 || !nearest_i32 || !depth_f32) return ksmi_fail(KSMI_E_ARG, "scene_depth: null pointer");
  KSMI_NOTE(depth_kernel);
  hipLaunchKernelGGL(depth_kernel, dim3(blocks_of(HW)), dim3(256), 0, (hipStream_t)stream, classes_u8, dem_f32, nearest_i32,
                     (uint64_t)water_mask, invalid_class, HW, depth_f32, wse_f32);
  return ksmi_check_launch("scene_depth");
}
