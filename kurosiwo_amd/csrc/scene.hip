// Whole-scene inference on the device: cut the windows of a product grid out of a raster that already sits in HBM, blend the model's
// logits back onto the scene and turn the blend into a class map (kurosiwo_amd/scene.py: predict_scene, predict.py).
//
// The window grid is a product grid: row origins ys[ny], column origins xs[nx], both sorted int32 device arrays, never negative;
// window i = iy * nx + ix starts at (ys[iy], xs[ix]) and is h x w.  A window overhangs the scene only at the bottom / right and
// only when the scene is smaller than the window on that axis (then that axis has the single origin 0).
//
//   scene_valid       valid[p] = (first ? 1 : valid[p]) & (no channel of the raster at p is NaN or equal to `nodata`)
//   scene_gather      out[slot][c][ly][lx] = preprocess(raster[c][ys[iy] + ly][xs[ix] + lx]); a cell outside the scene is 0.0f.
//                     preprocess is raw_tile_value of elementwise.hip (= sar_preprocess_kernel, cformer.hip) after a value equal to
//                     `nodata` became NaN: clamp[c] >= 0: NaN -> clamp, else clamp to [0, clamp]; clamp[c] < 0: NaN -> mean (the DEM
//                     channel); then (v - mean) / std, the subtraction and the division each rounded once.  mean == NULL: the raw
//                     value (nodata -> NaN) for a model that normalises inside its first convolution.
//   scene_accumulate  the blend in GATHER form: one thread owns one scene pixel and walks the windows of this launch that cover it in
//                     ascending i (rows covering y ascending, within a row the columns covering x ascending):
//                         acc[k] = acc[k] + (weight * logit_k)        wsum = wsum + weight
//                     product rounded to fp32, then the sum rounded to fp32 (file-scope contraction pragma: no fma), which is what
//                     the numpy slice loop `acc[:, sl] += weight * logits` computes.  No atomics, no LDS: the bits do not depend on
//                     the launch geometry, and across launches only on stream order.  The covering windows are found by a lower
//                     bound in ys / xs (at most ceil(h / stride) + 1 per axis are then walked), never by a scan of all n.
//   scene_finalize    m_k = acc_k / wsum (correctly rounded), class = first maximum of m (oracle/metrics_ref.argmax_lowest_index,
//                     ksmi_argmax_confusion_grouped), `invalid_class` and NaN scores where valid == 0; scores: m, or softmax(m) with
//                     the maximum subtracted first and expf.
//   scene_gather_view, scene_unview, scene_accumulate_views: test-time views (predict_scene(tta=...)): the windows gathered in one
//                     of the eight flip / transpose orientations, the model's logits turned back, and the V views of a window summed
//                     inside the pixel's window walk, so the bits still do not depend on the batch size.  Flips are index
//                     arithmetic in the one-thread-per-cell shape; a transpose stages 64 x 64 tiles through LDS so that both global
//                     sides stay runs of consecutive words.  See "test-time views" below.
//
// Shape: one thread per output cell (gather) or scene pixel (the rest), consecutive threads along x, so every load and store of a
// wave is a run of consecutive 4-byte words.  The accumulate launch covers the scene with one-row blocks of 256 pixels; a block
// outside the bounding rows of the launch's windows, and a thread outside their columns, leaves after two index loads.  These are
// elementwise, memory-bound launches: nothing to tune beyond coalescing, no knobs.
#include "common.h"
#include "../../include/ksmi.h"
#include "errors.h"

#pragma clang fp contract(off)

namespace {

constexpr int SCENE_MAX_K = 8;

__global__ __launch_bounds__(256) void scene_valid_kernel(const float* __restrict__ raster, int C, int64_t HW, float nodata,
                                                          unsigned char* __restrict__ valid, int first) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= HW) return;
  const bool sentinel = nodata == nodata;
  unsigned ok = 1;
  for (int c = 0; c < C; ++c) {
    const float v = raster[(int64_t)c * HW + p];
    if (v != v || (sentinel && v == nodata)) ok = 0;
  }
  valid[p] = (unsigned char)((first ? 1u : (unsigned)valid[p]) & ok);
}

__global__ __launch_bounds__(256) void scene_gather_kernel(const float* __restrict__ raster, int C, int Hs, int Ws, const int32_t* __restrict__ ys,
                                                           const int32_t* __restrict__ xs, int nx, int i0, int64_t total, int h, int w,
                                                           const float* __restrict__ mean, const float* __restrict__ stdv,
                                                           const float* __restrict__ clampv, float nodata, float* __restrict__ out) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int lx = (int)(idx % w);
  int64_t r = idx / w;
  const int ly = (int)(r % h);
  r /= h;
  const int c = (int)(r % C);
  const int i = i0 + (int)(r / C);
  const int y = ys[i / nx] + ly, x = xs[i % nx] + lx;
  float v = 0.0f;
  if ((unsigned)y < (unsigned)Hs && (unsigned)x < (unsigned)Ws) {
    v = raster[((int64_t)c * Hs + y) * Ws + x];
    if (nodata == nodata && v == nodata) v = __builtin_nanf("");
    if (mean != nullptr) {
      const float hi = clampv[c], m = mean[c];
      if (hi >= 0.f) v = (v != v) ? hi : fminf(fmaxf(v, 0.f), hi);
      else if (v != v) v = m;
      v = __fdiv_rn(__fsub_rn(v, m), stdv[c]);
    }
  }
  out[idx] = v;
}

// first index in [lo, hi) whose window [o[j], o[j] + len) ends after `pos` (o sorted ascending)
__device__ __forceinline__ int first_covering(const int32_t* __restrict__ o, int lo, int hi, int len, int pos) {
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (o[mid] + len > pos) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

__global__ __launch_bounds__(256) void scene_accumulate_kernel(const float* __restrict__ logits, const int32_t* __restrict__ ys,
                                                               const int32_t* __restrict__ xs, int nx, int i0, int n, int K, int h, int w,
                                                               const float* __restrict__ weight, float* __restrict__ acc,
                                                               float* __restrict__ wsum, int Hs, int Ws, int xblocks) {
  const int y = (int)(blockIdx.x / (unsigned)xblocks);
  const int x = (int)(blockIdx.x % (unsigned)xblocks) * 256 + threadIdx.x;
  const int last = i0 + n - 1;
  const int iy0 = i0 / nx, iy1 = last / nx;
  if (y < ys[iy0] || y >= ys[iy1] + h || x >= Ws) return;
  const int64_t HW = (int64_t)Hs * Ws, p = (int64_t)y * Ws + x, hw = (int64_t)h * w;
  float a[SCENE_MAX_K], s = 0.f;
  bool touched = false;
  for (int iy = first_covering(ys, iy0, iy1 + 1, h, y); iy <= iy1 && ys[iy] <= y; ++iy) {
    const int ixa = iy == iy0 ? i0 - iy0 * nx : 0, ixb = iy == iy1 ? last - iy1 * nx : nx - 1;
    const int ly = y - ys[iy];
    if (ly >= h) continue;                    // (cannot happen for sorted origins; keeps a malformed grid inside the buffers)
    for (int ix = first_covering(xs, ixa, ixb + 1, w, x); ix <= ixb && xs[ix] <= x; ++ix) {
      const int lx = x - xs[ix];
      if (lx >= w) continue;
      if (!touched) {
        touched = true;
        s = wsum[p];
#pragma unroll
        for (int k = 0; k < SCENE_MAX_K; ++k)
          if (k < K) a[k] = acc[k * HW + p];
      }
      const float wt = weight[(int64_t)ly * w + lx];
      const float* src = logits + (int64_t)(iy * nx + ix - i0) * K * hw + (int64_t)ly * w + lx;
#pragma unroll
      for (int k = 0; k < SCENE_MAX_K; ++k)
        if (k < K) a[k] = a[k] + wt * src[k * hw];
      s = s + wt;
    }
  }
  if (!touched) return;
  wsum[p] = s;
#pragma unroll
  for (int k = 0; k < SCENE_MAX_K; ++k)
    if (k < K) acc[k * HW + p] = a[k];
}

__global__ __launch_bounds__(256) void scene_finalize_kernel(const float* __restrict__ acc, const float* __restrict__ wsum,
                                                             const unsigned char* __restrict__ valid, int K, int64_t HW, int invalid_class,
                                                             unsigned char* __restrict__ cls, float* __restrict__ score, int score_mode) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= HW) return;
  if (valid != nullptr && valid[p] == 0) {
    cls[p] = (unsigned char)invalid_class;
    if (score != nullptr)
      for (int k = 0; k < K; ++k) score[k * HW + p] = __builtin_nanf("");
    return;
  }
  const float ws = wsum[p];
  float m[SCENE_MAX_K], mx = 0.f;
  int best = 0;
#pragma unroll
  for (int k = 0; k < SCENE_MAX_K; ++k)
    if (k < K) {
      m[k] = __fdiv_rn(acc[k * HW + p], ws);
      if (k == 0 || m[k] > mx) { mx = m[k]; best = k; }          // strict: the lowest index wins a tie
    }
  cls[p] = (unsigned char)best;
  if (score == nullptr) return;
  if (score_mode == 1) {
    float sum = 0.f;
#pragma unroll
    for (int k = 0; k < SCENE_MAX_K; ++k)
      if (k < K) {
        m[k] = expf(__fsub_rn(m[k], mx));
        sum = sum + m[k];
      }
#pragma unroll
    for (int k = 0; k < SCENE_MAX_K; ++k)
      if (k < K) m[k] = __fdiv_rn(m[k], sum);
  }
#pragma unroll
  for (int k = 0; k < SCENE_MAX_K; ++k)
    if (k < K) score[k * HW + p] = m[k];
}

// ---------------------------------------------------------------------------------------------------- test-time views
// A view code v in 0 .. 7 names one of the eight symmetries of a window tile T[ly][lx] (h x w): bit 2 transposes (first; h == w),
// bit 1 then flips y, bit 0 then flips x.  Cell (uy, ux) of the view U holds T[ly][lx] with
//     ay = v & 2 ? h - 1 - uy : uy     ax = v & 1 ? w - 1 - ux : ux     (ly, lx) = v & 4 ? (ax, ay) : (ay, ax)
// and the inverse view reads the same cell pairs the other way round.
constexpr int VT = 64;                         // edge of the tile the transposed views stage through LDS
constexpr int VT_LD = VT + 1;                  // its leading dimension: a column read walks the banks (65 % 32 == 1), 2 cycles a wave

// raster cell (c, y, x) as scene_gather_kernel computes it: +0.0f outside the scene, nodata -> NaN, then the preprocess arithmetic
__device__ __forceinline__ float gather_cell(const float* __restrict__ raster, int c, int Hs, int Ws, int y, int x, const float* __restrict__ mean,
                                             const float* __restrict__ stdv, const float* __restrict__ clampv, float nodata) {
  float v = 0.0f;
  if ((unsigned)y < (unsigned)Hs && (unsigned)x < (unsigned)Ws) {
    v = raster[((int64_t)c * Hs + y) * Ws + x];
    if (nodata == nodata && v == nodata) v = __builtin_nanf("");
    if (mean != nullptr) {
      const float hi = clampv[c], m = mean[c];
      if (hi >= 0.f) v = (v != v) ? hi : fminf(fmaxf(v, 0.f), hi);
      else if (v != v) v = m;
      v = __fdiv_rn(__fsub_rn(v, m), stdv[c]);
    }
  }
  return v;
}

// One 64 x 64 tile through LDS by the 256 threads of a block: tile[r][c] = src(r, c) with the lane along c, so a wave writes one LDS
// row and `src` walks its global memory along x; after the barrier dst(c, r, tile[r][c]) with the lane along r, so `dst` walks its
// global memory along x too and the wave reads one LDS column at stride 65.  src returns any value for a cell outside the plane
// without loading; dst drops it.  The value moves as bits: a NaN keeps its payload.
template <class Src, class Dst>
__device__ __forceinline__ void transpose_tile(Src src, Dst dst) {
  __shared__ float tile[VT][VT_LD];
  const int lane = threadIdx.x & (VT - 1), wave = threadIdx.x >> 6;
  for (int r = wave; r < VT; r += 4) tile[r][lane] = src(r, lane);
  __syncthreads();
  for (int c = wave; c < VT; c += 4) dst(c, lane, tile[lane][c]);
}

// views 0 .. 3: index arithmetic only; a wave that reads a row backwards touches the cache lines of the forward read
__global__ __launch_bounds__(256) void scene_gather_flip_kernel(const float* __restrict__ raster, int C, int Hs, int Ws,
                                                                const int32_t* __restrict__ ys, const int32_t* __restrict__ xs, int nx, int i0,
                                                                int64_t total, int h, int w, const float* __restrict__ mean,
                                                                const float* __restrict__ stdv, const float* __restrict__ clampv, float nodata,
                                                                int view, float* __restrict__ out) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int ux = (int)(idx % w);
  int64_t r = idx / w;
  const int uy = (int)(r % h);
  r /= h;
  const int c = (int)(r % C);
  const int i = i0 + (int)(r / C);
  const int ly = (view & 2) ? h - 1 - uy : uy, lx = (view & 1) ? w - 1 - ux : ux;
  out[idx] = gather_cell(raster, c, Hs, Ws, ys[i / nx] + ly, xs[i % nx] + lx, mean, stdv, clampv, nodata);
}

// views 4 .. 7 of s x s windows: one block per 64 x 64 tile of one (slot, channel) plane of the output; tile row r is output column
// ux0 + r, tile column c is output row uy0 + c, which lies along raster x
__global__ __launch_bounds__(256) void scene_gather_transpose_kernel(const float* __restrict__ raster, int C, int Hs, int Ws,
                                                                     const int32_t* __restrict__ ys, const int32_t* __restrict__ xs, int nx,
                                                                     int i0, int s, int tiles, const float* __restrict__ mean,
                                                                     const float* __restrict__ stdv, const float* __restrict__ clampv,
                                                                     float nodata, int view, float* __restrict__ out) {
  const int per_plane = tiles * tiles;
  const int plane = (int)(blockIdx.x / (unsigned)per_plane), t = (int)(blockIdx.x % (unsigned)per_plane);
  const int uy0 = (t / tiles) * VT, ux0 = (t % tiles) * VT;
  const int c = plane % C, i = i0 + plane / C;
  const int y0 = ys[i / nx], x0 = xs[i % nx];
  float* __restrict__ dst_plane = out + (int64_t)plane * s * s;
  transpose_tile(
      [&](int r, int col) {
        const int ux = ux0 + r, uy = uy0 + col;
        if (ux >= s || uy >= s) return 0.0f;
        const int ly = (view & 1) ? s - 1 - ux : ux, lx = (view & 2) ? s - 1 - uy : uy;
        return gather_cell(raster, c, Hs, Ws, y0 + ly, x0 + lx, mean, stdv, clampv, nodata);
      },
      [&](int row, int l, float v) {
        const int uy = uy0 + row, ux = ux0 + l;
        if (uy < s && ux < s) dst_plane[(int64_t)uy * s + ux] = v;
      });
}

// inverse of views 0 .. 3, out of place: out[p][ly][lx] = in[p][uy][ux]
__global__ __launch_bounds__(256) void scene_unview_flip_kernel(const float* __restrict__ in, float* __restrict__ out, int64_t total, int h, int w,
                                                                int view) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int lx = (int)(idx % w);
  const int64_t r = idx / w;
  const int ly = (int)(r % h);
  const int uy = (view & 2) ? h - 1 - ly : ly, ux = (view & 1) ? w - 1 - lx : lx;
  out[idx] = in[(r / h * h + uy) * w + ux];
}

// inverse of views 4 .. 7 of s x s planes: tile row r is window column lx0 + r, tile column c is window row ly0 + c, which lies
// along the x of the viewed plane
__global__ __launch_bounds__(256) void scene_unview_transpose_kernel(const float* __restrict__ in, float* __restrict__ out, int s, int tiles,
                                                                     int view) {
  const int per_plane = tiles * tiles;
  const int64_t plane = blockIdx.x / (unsigned)per_plane;
  const int t = (int)(blockIdx.x % (unsigned)per_plane);
  const int ly0 = (t / tiles) * VT, lx0 = (t % tiles) * VT;
  const float* __restrict__ src_plane = in + plane * s * s;
  float* __restrict__ dst_plane = out + plane * s * s;
  transpose_tile(
      [&](int r, int col) {
        const int lx = lx0 + r, ly = ly0 + col;
        if (lx >= s || ly >= s) return 0.0f;
        const int uy = (view & 2) ? s - 1 - lx : lx, ux = (view & 1) ? s - 1 - ly : ly;
        return src_plane[(int64_t)uy * s + ux];
      },
      [&](int row, int l, float v) {
        const int ly = ly0 + row, lx = lx0 + l;
        if (ly < s && lx < s) dst_plane[(int64_t)ly * s + lx] = v;
      });
}

// scene_accumulate_kernel with V views of every window: logits [V][n][K][h][w], already turned back to window orientation.  Per
// covering window in ascending i the views in ascending v, each one more step of the same rounded sums; V == 1 is that kernel.
__global__ __launch_bounds__(256) void scene_accumulate_views_kernel(const float* __restrict__ logits, int V, const int32_t* __restrict__ ys,
                                                                     const int32_t* __restrict__ xs, int nx, int i0, int n, int K, int h, int w,
                                                                     const float* __restrict__ weight, float* __restrict__ acc,
                                                                     float* __restrict__ wsum, int Hs, int Ws, int xblocks) {
  const int y = (int)(blockIdx.x / (unsigned)xblocks);
  const int x = (int)(blockIdx.x % (unsigned)xblocks) * 256 + threadIdx.x;
  const int last = i0 + n - 1;
  const int iy0 = i0 / nx, iy1 = last / nx;
  if (y < ys[iy0] || y >= ys[iy1] + h || x >= Ws) return;
  const int64_t HW = (int64_t)Hs * Ws, p = (int64_t)y * Ws + x, hw = (int64_t)h * w, view_stride = (int64_t)n * K * hw;
  float a[SCENE_MAX_K], s = 0.f;
  bool touched = false;
  for (int iy = first_covering(ys, iy0, iy1 + 1, h, y); iy <= iy1 && ys[iy] <= y; ++iy) {
    const int ixa = iy == iy0 ? i0 - iy0 * nx : 0, ixb = iy == iy1 ? last - iy1 * nx : nx - 1;
    const int ly = y - ys[iy];
    if (ly >= h) continue;
    for (int ix = first_covering(xs, ixa, ixb + 1, w, x); ix <= ixb && xs[ix] <= x; ++ix) {
      const int lx = x - xs[ix];
      if (lx >= w) continue;
      if (!touched) {
        touched = true;
        s = wsum[p];
#pragma unroll
        for (int k = 0; k < SCENE_MAX_K; ++k)
          if (k < K) a[k] = acc[k * HW + p];
      }
      const float wt = weight[(int64_t)ly * w + lx];
      const float* src = logits + (int64_t)(iy * nx + ix - i0) * K * hw + (int64_t)ly * w + lx;
      for (int v = 0; v < V; ++v, src += view_stride) {
#pragma unroll
        for (int k = 0; k < SCENE_MAX_K; ++k)
          if (k < K) a[k] = a[k] + wt * src[k * hw];
        s = s + wt;
      }
    }
  }
  if (!touched) return;
  wsum[p] = s;
#pragma unroll
  for (int k = 0; k < SCENE_MAX_K; ++k)
    if (k < K) acc[k * HW + p] = a[k];
}

// blocks of 256 for `total` one-thread items, or -1 when the count does not fit a grid
int64_t blocks_of(int64_t total) {
  const int64_t b = (total + 255) / 256;
  return b > 0x7fffffff ? -1 : b;
}

// blocks of one 64 x 64 tile each for `planes` planes of s x s, or -1 when the count does not fit a grid
int64_t tile_blocks_of(int64_t planes, int s) {
  const int64_t tiles = (s + VT - 1) / VT;
  int64_t b = 0;
  if (__builtin_mul_overflow(planes, tiles * tiles, &b)) return -1;
  return b > 0x7fffffff ? -1 : b;
}

// the window range of a launch: 0 = run, 1 = nothing to do (n == 0), < 0 = refused
int check_windows(const char* what, int ny, int nx, int i0, int n, int h, int w, int Hs, int Ws) {
  if (n < 0 || i0 < 0 || ny < 1 || nx < 1 || h < 1 || w < 1 || Hs < 1 || Ws < 1) return ksmi_fail(KSMI_E_ARG, what);
  if ((int64_t)i0 + n > (int64_t)ny * nx) return ksmi_fail(KSMI_E_ARG, what);
  return n == 0 ? 1 : 0;
}

}  // namespace

int ksmi_scene_valid(const float* raster, int C, int64_t HW, float nodata, unsigned char* valid, int first, void* stream) {
  if (C < 1 || HW < 0) return ksmi_fail(KSMI_E_ARG, "scene_valid: C >= 1 channels of HW >= 0 pixels");
  if (HW == 0) return 0;
  if (!raster || !valid) return ksmi_fail(KSMI_E_ARG, "scene_valid: null pointer");
  const int64_t blocks = blocks_of(HW);
  if (blocks < 0) return ksmi_fail(KSMI_E_ARG, "scene_valid: more than 2^31 blocks of pixels");
  KSMI_NOTE(scene_valid_kernel);
  hipLaunchKernelGGL(scene_valid_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, raster, C, HW, nodata, valid, first);
  return ksmi_check_launch("scene_valid");
}

int ksmi_scene_gather(const float* raster, int C, int Hs, int Ws, const int32_t* ys, int ny, const int32_t* xs, int nx, int i0, int n, int h,
                      int w, const float* mean, const float* stdv, const float* clamp, float nodata, float* out, void* stream) {
  if (C < 1) return ksmi_fail(KSMI_E_ARG, "scene_gather: C >= 1");
  const int rc = check_windows("scene_gather: windows i0 .. i0 + n - 1 of an ny x nx grid (n >= 0, i0 >= 0, h, w, Hs, Ws >= 1)", ny, nx, i0, n, h,
                               w, Hs, Ws);
  if (rc) return rc < 0 ? rc : 0;
  if (!raster || !ys || !xs || !out) return ksmi_fail(KSMI_E_ARG, "scene_gather: null pointer");
  if (mean && (!stdv || !clamp)) return ksmi_fail(KSMI_E_ARG, "scene_gather: mean, std and clamp come together (mean NULL: raw values)");
  int64_t total = 0;
  if (__builtin_mul_overflow((int64_t)h * w, (int64_t)n * C, &total) || blocks_of(total) < 0)
    return ksmi_fail(KSMI_E_ARG, "scene_gather: more than 2^31 blocks of cells");
  KSMI_NOTE(scene_gather_kernel);
  hipLaunchKernelGGL(scene_gather_kernel, dim3((unsigned)blocks_of(total)), dim3(256), 0, (hipStream_t)stream, raster, C, Hs, Ws, ys, xs, nx, i0,
                     total, h, w, mean, stdv, clamp, nodata, out);
  return ksmi_check_launch("scene_gather");
}

int ksmi_scene_accumulate(const float* logits, const int32_t* ys, int ny, const int32_t* xs, int nx, int i0, int n, int K, int h, int w,
                          const float* weight, float* acc, float* wsum, int Hs, int Ws, void* stream) {
  if (K < 1 || K > SCENE_MAX_K) return ksmi_fail(KSMI_E_ARG, "scene_accumulate: 1 <= K <= 8 classes");
  const int rc = check_windows("scene_accumulate: windows i0 .. i0 + n - 1 of an ny x nx grid (n >= 0, i0 >= 0, h, w, Hs, Ws >= 1)", ny, nx, i0,
                               n, h, w, Hs, Ws);
  if (rc) return rc < 0 ? rc : 0;
  if (!logits || !ys || !xs || !weight || !acc || !wsum) return ksmi_fail(KSMI_E_ARG, "scene_accumulate: null pointer");
  const int xblocks = (Ws + 255) / 256;
  const int64_t blocks = (int64_t)xblocks * Hs;
  if (blocks > 0x7fffffff) return ksmi_fail(KSMI_E_ARG, "scene_accumulate: more than 2^31 blocks of pixels");
  KSMI_NOTE(scene_accumulate_kernel);
  hipLaunchKernelGGL(scene_accumulate_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, logits, ys, xs, nx, i0, n, K, h, w,
                     weight, acc, wsum, Hs, Ws, xblocks);
  return ksmi_check_launch("scene_accumulate");
}

int ksmi_scene_finalize(const float* acc, const float* wsum, const unsigned char* valid, int K, int64_t HW, int invalid_class,
                        unsigned char* out_class_u8, float* out_score, int score_mode, void* stream) {
  if (K < 1 || K > SCENE_MAX_K) return ksmi_fail(KSMI_E_ARG, "scene_finalize: 1 <= K <= 8 classes");
  if (HW < 0 || invalid_class < 0 || invalid_class > 255 || (score_mode != 0 && score_mode != 1))
    return ksmi_fail(KSMI_E_ARG, "scene_finalize: HW >= 0, invalid_class in 0 .. 255, score_mode 0 (mean logits) or 1 (softmax)");
  if (HW == 0) return 0;
  if (!acc || !wsum || !out_class_u8) return ksmi_fail(KSMI_E_ARG, "scene_finalize: null pointer");
  const int64_t blocks = blocks_of(HW);
  if (blocks < 0) return ksmi_fail(KSMI_E_ARG, "scene_finalize: more than 2^31 blocks of pixels");
  KSMI_NOTE(scene_finalize_kernel);
  hipLaunchKernelGGL(scene_finalize_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, acc, wsum, valid, K, HW, invalid_class,
                     out_class_u8, out_score, score_mode);
  return ksmi_check_launch("scene_finalize");
}

int ksmi_scene_gather_view(const float* raster, int C, int Hs, int Ws, const int32_t* ys, int ny, const int32_t* xs, int nx, int i0, int n, int h,
                           int w, const float* mean, const float* stdv, const float* clamp, float nodata, int view, float* out, void* stream) {
  if (C < 1) return ksmi_fail(KSMI_E_ARG, "scene_gather_view: C >= 1");
  if (view < 0 || view > 7) return ksmi_fail(KSMI_E_ARG, "scene_gather_view: view is a code 0 .. 7 (1: flip x, 2: flip y, 4: transpose)");
  const int rc = check_windows("scene_gather_view: windows i0 .. i0 + n - 1 of an ny x nx grid (n >= 0, i0 >= 0, h, w, Hs, Ws >= 1)", ny, nx, i0, n,
                               h, w, Hs, Ws);
  if (rc < 0) return rc;
  if ((view & 4) && h != w) return ksmi_fail(KSMI_E_ARG, "scene_gather_view: a transposed view (view & 4) needs square windows, h == w");
  if (rc) return 0;
  if (!raster || !ys || !xs || !out) return ksmi_fail(KSMI_E_ARG, "scene_gather_view: null pointer");
  if (mean && (!stdv || !clamp)) return ksmi_fail(KSMI_E_ARG, "scene_gather_view: mean, std and clamp come together (mean NULL: raw values)");
  int64_t total = 0;
  if (__builtin_mul_overflow((int64_t)h * w, (int64_t)n * C, &total) || blocks_of(total) < 0)
    return ksmi_fail(KSMI_E_ARG, "scene_gather_view: more than 2^31 blocks of cells");
  if (view & 4) {
    const int64_t blocks = tile_blocks_of((int64_t)n * C, h);
    if (blocks < 0) return ksmi_fail(KSMI_E_ARG, "scene_gather_view: more than 2^31 tiles");
    KSMI_NOTE(scene_gather_transpose_kernel);
    hipLaunchKernelGGL(scene_gather_transpose_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, raster, C, Hs, Ws, ys, xs, nx, i0,
                       h, (h + VT - 1) / VT, mean, stdv, clamp, nodata, view, out);
  } else {
    KSMI_NOTE(scene_gather_flip_kernel);
    hipLaunchKernelGGL(scene_gather_flip_kernel, dim3((unsigned)blocks_of(total)), dim3(256), 0, (hipStream_t)stream, raster, C, Hs, Ws, ys, xs, nx,
                       i0, total, h, w, mean, stdv, clamp, nodata, view, out);
  }
  return ksmi_check_launch("scene_gather_view");
}

int ksmi_scene_unview(const float* in, float* out, int64_t planes, int h, int w, int view, void* stream) {
  if (view < 0 || view > 7) return ksmi_fail(KSMI_E_ARG, "scene_unview: view is a code 0 .. 7 (1: flip x, 2: flip y, 4: transpose)");
  if (planes < 0 || h < 1 || w < 1) return ksmi_fail(KSMI_E_ARG, "scene_unview: planes >= 0 planes of h x w, h, w >= 1");
  if ((view & 4) && h != w) return ksmi_fail(KSMI_E_ARG, "scene_unview: a transposed view (view & 4) needs square planes, h == w");
  if (planes == 0) return 0;
  if (!in || !out) return ksmi_fail(KSMI_E_ARG, "scene_unview: null pointer");
  if (in == out) return ksmi_fail(KSMI_E_ARG, "scene_unview: out of place, out must not be in");
  int64_t total = 0;
  if (__builtin_mul_overflow((int64_t)h * w, planes, &total) || blocks_of(total) < 0)
    return ksmi_fail(KSMI_E_ARG, "scene_unview: more than 2^31 blocks of cells");
  if (view & 4) {
    const int64_t blocks = tile_blocks_of(planes, h);
    if (blocks < 0) return ksmi_fail(KSMI_E_ARG, "scene_unview: more than 2^31 tiles");
    KSMI_NOTE(scene_unview_transpose_kernel);
    hipLaunchKernelGGL(scene_unview_transpose_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, in, out, h, (h + VT - 1) / VT, view);
  } else {
    KSMI_NOTE(scene_unview_flip_kernel);
    hipLaunchKernelGGL(scene_unview_flip_kernel, dim3((unsigned)blocks_of(total)), dim3(256), 0, (hipStream_t)stream, in, out, total, h, w, view);
  }
  return ksmi_check_launch("scene_unview");
}

int ksmi_scene_accumulate_views(const float* logits, int V, const int32_t* ys, int ny, const int32_t* xs, int nx, int i0, int n, int K, int h, int w,
                                const float* weight, float* acc, float* wsum, int Hs, int Ws, void* stream) {
  if (V < 1 || V > 8) return ksmi_fail(KSMI_E_ARG, "scene_accumulate_views: 1 <= V <= 8 views");
  if (K < 1 || K > SCENE_MAX_K) return ksmi_fail(KSMI_E_ARG, "scene_accumulate_views: 1 <= K <= 8 classes");
  const int rc = check_windows("scene_accumulate_views: windows i0 .. i0 + n - 1 of an ny x nx grid (n >= 0, i0 >= 0, h, w, Hs, Ws >= 1)", ny, nx,
                               i0, n, h, w, Hs, Ws);
  if (rc) return rc < 0 ? rc : 0;
  if (!logits || !ys || !xs || !weight || !acc || !wsum) return ksmi_fail(KSMI_E_ARG, "scene_accumulate_views: null pointer");
  const int xblocks = (Ws + 255) / 256;
  const int64_t blocks = (int64_t)xblocks * Hs;
  if (blocks > 0x7fffffff) return ksmi_fail(KSMI_E_ARG, "scene_accumulate_views: more than 2^31 blocks of pixels");
  KSMI_NOTE(scene_accumulate_views_kernel);
  hipLaunchKernelGGL(scene_accumulate_views_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, logits, V, ys, xs, nx, i0, n, K, h,
                     w, weight, acc, wsum, Hs, Ws, xblocks);
  return ksmi_check_launch("scene_accumulate_views");
}
