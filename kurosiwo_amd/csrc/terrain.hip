// Terrain attributes of the DEM channel on the device (dataset/Dataset.py:747-761, 1160-1171: --slope replaces the DEM by
// richdem.TerrainAttribute(rdarray(dem), attrib="slope_riserun"), then standardises it).
//
// The arithmetic is kurosiwo_amd/dataset.py:slope_riserun(dem, nodata, cell=1.0) operation for operation, in double, so that a batch
// from TileBatchLoader carries the bits the per-sample Dataset computes with numpy:
//     zc      = (double)dem[y][x]
//     a .. i  = the 3 x 3 neighbourhood widened to double; a neighbour outside ITS OWN tile, a NaN one, or one equal to `nodata`
//               (compared as doubles; nodata = NaN: no sentinel) is replaced by zc
//     dzdx    = ((c + 2f + i) - (a + 2d + g)) / 8        dzdy = ((g + 2h + i) - (a + 2b + c)) / 8
//     s       = sqrt(dzdx*dzdx + dzdy*dzdy)              -> (float)s, or (float)nodata where zc == nodata
//     standardise: (o - mean) / std in fp32, the sub-then-div torch runs on the host path
// Every product and sum is rounded on its own: numpy does not fuse dzdx*dzdx + dzdy*dzdy, and an fma there moves the last double bit
// often enough to show as rare fp32 mismatches.  Hence the file-scope contraction pragma; the square root is the correctly rounded one.
//
// Shape: one thread per cell, consecutive threads along W, nine 4-byte loads served by the same few cache lines as the neighbours'.
// No LDS, nothing to tune: 32 tiles of 224 x 224 are 12.8 MB of traffic, a latency-bound launch.
#include "common.h"
#include "../../include/ksmi.h"
#include "errors.h"

#pragma clang fp contract(off)

namespace {

struct Nbr {
  const float* __restrict__ t;          // the cell's own tile
  int H, W;
  double zc, nodata;
  bool sentinel;
  __device__ __forceinline__ double at(int y, int x) const {
    if ((unsigned)y >= (unsigned)H || (unsigned)x >= (unsigned)W) return zc;
    const double v = (double)t[(int64_t)y * W + x];
    return (v != v || (sentinel && v == nodata)) ? zc : v;
  }
};

__global__ __launch_bounds__(256) void dem_slope_kernel(const float* __restrict__ dem, float* __restrict__ out, int64_t total, int H, int W,
                                                        double nodata, float mean, float stdv, int standardise) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int64_t HW = (int64_t)H * W;
  const int64_t tile = idx / HW, r = idx - tile * HW;
  const int y = (int)(r / W), x = (int)(r - (int64_t)y * W);
  Nbr k;
  k.t = dem + tile * HW; k.H = H; k.W = W;
  k.zc = (double)dem[idx]; k.nodata = nodata; k.sentinel = nodata == nodata;
  const double a = k.at(y - 1, x - 1), b = k.at(y - 1, x), c = k.at(y - 1, x + 1);
  const double d = k.at(y, x - 1), f = k.at(y, x + 1);
  const double g = k.at(y + 1, x - 1), h = k.at(y + 1, x), i = k.at(y + 1, x + 1);
  const double dzdx = ((c + 2.0 * f + i) - (a + 2.0 * d + g)) / 8.0;
  const double dzdy = ((g + 2.0 * h + i) - (a + 2.0 * b + c)) / 8.0;
  const double s = __dsqrt_rn(dzdx * dzdx + dzdy * dzdy);
  float o = (k.sentinel && k.zc == nodata) ? (float)nodata : (float)s;
  if (standardise) o = __fdiv_rn(__fsub_rn(o, mean), stdv);
  out[idx] = o;
}

}  // namespace

int ksmi_dem_slope(const float* dem, float* out, int n, int H, int W, double nodata, float mean, float stdv, int standardise, void* stream) {
  if (n < 0 || H < 1 || W < 1) return ksmi_fail(KSMI_E_ARG, "dem_slope: n >= 0 tiles of H >= 1 by W >= 1");
  if (n == 0) return 0;
  if (!dem || !out) return ksmi_fail(KSMI_E_ARG, "dem_slope: null pointer");
  int64_t total = 0;
  if (__builtin_mul_overflow((int64_t)H * W, (int64_t)n, &total) || total > ((int64_t)0x7fffffff << 8))
    return ksmi_fail(KSMI_E_ARG, "dem_slope: more than 2^31 blocks of cells");
  if (out < dem + total && dem < out + total) return ksmi_fail(KSMI_E_ARG, "dem_slope: the stencil cannot run in place (out overlaps dem)");
  const int64_t blocks = (total + 255) / 256;
  KSMI_NOTE(dem_slope_kernel);
  hipLaunchKernelGGL(dem_slope_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, dem, out, total, H, W, nodata, mean, stdv,
                     standardise);
  return ksmi_check_launch("dem_slope");
}
