// Segmentation losses beyond ce / ce+dice (create_loss's `dice`, `iou`, `focal` branches), 3 classes, NCHW fp32 logits, int64 labels:
//   dice   = smp DiceLoss(mode="multiclass", ignore_index)        : batch-global soft Dice, absent classes masked
//   lovasz = smp LovaszLoss(mode="multiclass", per_image=False)   : Lovasz-softmax over the flattened batch, present classes
//   focal  = FocalLoss(alpha, gamma, reduction="mean")            : alpha[y] (1 - pt)^gamma (-log pt) / #valid
// Every reduction has a fixed order (per-block partials, fp64 finish): the results are bit-reproducible.  No float atomics, no
// allocation, no host read-back: all scratch lives in the caller's workspace (ksmi_seg_loss_workspace).
//
// Lovasz needs every valid pixel's error sorted in descending order, once per class.  The sort is a stable LSD radix sort over
// a 30-bit key (e in [0,1] has monotone fp32 bits), four passes of 8-bit digits, each pass three launches with no communication
// between workgroups inside a launch: per-tile digit histogram -> per-digit scan over the tiles -> stable scatter (ranks inside a
// tile from wave64 ballots, in element order).  A reduce-then-scan of the foreground bit over the sorted order then gives the
// Lovasz gradient g(r) in closed form, the loss partials, and g scattered back to the pixel's own position for the backward pass.
#include "common.h"
#include "../../include/ksmi.h"
#include "errors.h"

namespace {

constexpr int kSplit = 32;                    // pixel splits per image of the dice / focal partials
constexpr int kItems = 8;                     // elements per thread of a sort tile
constexpr int kTile = 256 * kItems;           // elements per sort tile (one workgroup)
constexpr uint32_t kOneBits = 0x3F800000u;    // bits of 1.0f: key = kOneBits - bits(e) sorts e descending
constexpr uint32_t kInvalidKey = 0x3FFFFFFFu; // ignored pixels: above every valid key, so they sort last (30 bits)
constexpr uint32_t kFgBit = 0x80000000u;      // payload = flat pixel index | fg << 31

typedef long long i64x2 __attribute__((ext_vector_type(2)));

// ---- pixel groups: V consecutive pixels of one image (V = 4: 16-byte loads of each class plane and of the labels) ----
template <int V>
__device__ __forceinline__ void load_px(const float* lg, const int64_t* lb, int HW, int g, float (&x)[3][V], int64_t (&t)[V]) {
  if constexpr (V == 4) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const f32x4 v = *(const f32x4*)(lg + (int64_t)c * HW + 4 * g);
      x[c][0] = v[0]; x[c][1] = v[1]; x[c][2] = v[2]; x[c][3] = v[3];
    }
    const i64x2 l0 = *(const i64x2*)(lb + 4 * g), l1 = *(const i64x2*)(lb + 4 * g + 2);
    t[0] = l0[0]; t[1] = l0[1]; t[2] = l1[0]; t[3] = l1[1];
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) x[c][0] = lg[(int64_t)c * HW + g];
    t[0] = lb[g];
  }
}

template <int V>
__device__ __forceinline__ void put_px(float* dg, int HW, int g, const float (&d)[3][V]) {
  if constexpr (V == 4) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      f32x4 v; v[0] = d[c][0]; v[1] = d[c][1]; v[2] = d[c][2]; v[3] = d[c][3];
      *(f32x4*)(dg + (int64_t)c * HW + 4 * g) = v;
    }
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) dg[(int64_t)c * HW + g] = d[c][0];
  }
}

struct Sm3 { float p[3]; float lse; };
__device__ __forceinline__ Sm3 softmax3(float a, float b, float c) {
  const float m = fmaxf(a, fmaxf(b, c));
  const float e0 = expf(a - m), e1 = expf(b - m), e2 = expf(c - m);
  const float s = e0 + e1 + e2, r = 1.f / s;
  return {{e0 * r, e1 * r, e2 * r}, m + logf(s)};
}

// softmax backward of dL/dp = h: dx_k = p_k (h_k - sum_j h_j p_j)
__device__ __forceinline__ void softmax3_bwd(const float (&p)[3], const float (&h)[3], float gs, float& d0, float& d1, float& d2) {
  const float dot = h[0] * p[0] + h[1] * p[1] + h[2] * p[2];
  d0 = p[0] * (h[0] - dot) * gs; d1 = p[1] * (h[1] - dot) * gs; d2 = p[2] * (h[2] - dot) * gs;
}

__device__ __forceinline__ int split_range(int G, int& g1) {
  const int per = (G + gridDim.x - 1) / gridDim.x;
  const int g0 = blockIdx.x * per;
  g1 = min(G, g0 + per);
  return g0;
}

// exclusive scan of one value per thread over a 256-thread block (sh: 4 words of LDS); total = the block's sum
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t* sh, uint32_t& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t y = __shfl_up(inc, o, 64);
    if (lane >= o) inc += y;
  }
  if (lane == 63) sh[w] = inc;
  __syncthreads();
  uint32_t off = 0;
  for (int i = 0; i < w; ++i) off += sh[i];
  total = sh[0] + sh[1] + sh[2] + sh[3];
  __syncthreads();
  return off + inc - v;
}

// ------------------------------------------------------------------------------------------------
// Dice: part[B][S][9] = {sum v p_c t_c, sum v p_c, sum t_c} per class; coef = {a_c, b_c}: dL/dp_c = v (a_c t_c + b_c)
// ------------------------------------------------------------------------------------------------
template <int V>
__global__ __launch_bounds__(256) void dice_fwd_kernel(const float* logits, const int64_t* labels, float* part, int HW, int ignore_index) {
  const int b = blockIdx.y;
  int g1;
  const int g0 = split_range(HW / V, g1);
  const float* lg = logits + (int64_t)b * 3 * HW;
  const int64_t* lb = labels + (int64_t)b * HW;
  float acc[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) acc[k] = 0.f;
  for (int g = g0 + threadIdx.x; g < g1; g += blockDim.x) {
    float x[3][V]; int64_t t[V];
    load_px<V>(lg, lb, HW, g, x, t);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const Sm3 q = softmax3(x[0][j], x[1][j], x[2][j]);
      const bool valid = t[j] != ignore_index;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const bool tc = valid && t[j] == c;
        acc[c] += tc ? q.p[c] : 0.f;
        acc[3 + c] += valid ? q.p[c] : 0.f;
        acc[6 + c] += tc ? 1.f : 0.f;
      }
    }
  }
  __shared__ float red[4][9];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const float s = wave_sum(acc[k]);
    if (lane == 0) red[w][k] = s;
  }
  __syncthreads();
  if (threadIdx.x < 9)
    part[((size_t)b * gridDim.x + blockIdx.x) * 9 + threadIdx.x] =
        ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// sums of R partial rows of K floats in fp64, fixed order (strided per thread, then a tree); the result is red[0][k]
template <int K>
__device__ __forceinline__ void rows_sum_f64(const float* part, int R, double (*red)[K]) {
  double a[K];
#pragma unroll
  for (int k = 0; k < K; ++k) a[k] = 0.0;
  for (int r = threadIdx.x; r < R; r += 256)
#pragma unroll
    for (int k = 0; k < K; ++k) a[k] += part[(size_t)r * K + k];
#pragma unroll
  for (int k = 0; k < K; ++k) red[threadIdx.x][k] = a[k];
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s)
#pragma unroll
      for (int k = 0; k < K; ++k) red[threadIdx.x][k] += red[threadIdx.x + s][k];
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void dice_finish_kernel(const float* part, int R, float* coef, float* out3) {
  __shared__ double red[256][9];
  rows_sum_f64<9>(part, R, red);
  if (threadIdx.x != 0) return;
  const double eps = 1e-7;
  double loss = 0.0;
  for (int c = 0; c < 3; ++c) {
    const double I = red[0][c], D = red[0][3 + c] + red[0][6 + c];
    const bool present = red[0][6 + c] > 0.0;
    const double Dm = D > eps ? D : eps;
    if (present) loss += 1.0 - 2.0 * I / Dm;
    coef[c] = present ? (float)(-2.0 / (3.0 * Dm)) : 0.f;
    coef[3 + c] = present && D >= eps ? (float)(2.0 * I / (3.0 * D * D)) : 0.f;   // clamped: D is the constant eps
  }
  out3[0] = (float)(loss / 3.0); out3[1] = 0.f; out3[2] = 0.f;
}

template <int V>
__global__ __launch_bounds__(256) void dice_bwd_kernel(const float* logits, const int64_t* labels, const float* coef, const float* gscale,
                                                       float* dlogits, int HW, int ignore_index) {
  const int b = blockIdx.y, G = HW / V;
  const float a[3] = {coef[0], coef[1], coef[2]}, bb[3] = {coef[3], coef[4], coef[5]};
  const float gs = gscale ? *gscale : 1.f;
  const float* lg = logits + (int64_t)b * 3 * HW;
  const int64_t* lb = labels + (int64_t)b * HW;
  float* dg = dlogits + (int64_t)b * 3 * HW;
  for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < G; g += gridDim.x * blockDim.x) {
    float x[3][V], d[3][V]; int64_t t[V];
    load_px<V>(lg, lb, HW, g, x, t);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const Sm3 q = softmax3(x[0][j], x[1][j], x[2][j]);
      const bool valid = t[j] != ignore_index;
      float h[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) h[c] = valid ? (t[j] == c ? a[c] : 0.f) + bb[c] : 0.f;
      softmax3_bwd(q.p, h, gs, d[0][j], d[1][j], d[2][j]);
    }
    put_px<V>(dg, HW, g, d);
  }
}

// ------------------------------------------------------------------------------------------------
// Focal: part[B][S][2] = {sum l_i, #valid}; coef[0] = 1 / #valid (0 when none)
// ------------------------------------------------------------------------------------------------
struct FocalTerm { float l, dldlp; };
__device__ __forceinline__ FocalTerm focal_term(float lp, float alpha, float gamma) {
  if (gamma == 0.f) return {-alpha * lp, -alpha};
  const float pt = expf(lp), omp = -expm1f(lp);              // 1 - pt without the cancellation near pt = 1
  const float f = powf(omp, gamma), f1 = powf(omp, gamma - 1.f);
  return {-alpha * f * lp, -alpha * (f - gamma * f1 * pt * lp)};
}

template <int V>
__global__ __launch_bounds__(256) void focal_fwd_kernel(const float* logits, const int64_t* labels, const float* cw, float gamma, float* part,
                                                        int HW, int ignore_index) {
  const int b = blockIdx.y;
  int g1;
  const int g0 = split_range(HW / V, g1);
  const float w0 = cw[0], w1 = cw[1], w2 = cw[2];
  const float* lg = logits + (int64_t)b * 3 * HW;
  const int64_t* lb = labels + (int64_t)b * HW;
  float sl = 0.f, n = 0.f;
  for (int g = g0 + threadIdx.x; g < g1; g += blockDim.x) {
    float x[3][V]; int64_t t[V];
    load_px<V>(lg, lb, HW, g, x, t);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const Sm3 q = softmax3(x[0][j], x[1][j], x[2][j]);
      const bool valid = t[j] != ignore_index;
      const int y = (int)t[j];
      const float xt = y == 0 ? x[0][j] : (y == 1 ? x[1][j] : x[2][j]);
      const float al = y == 0 ? w0 : (y == 1 ? w1 : w2);
      sl += valid ? focal_term(xt - q.lse, al, gamma).l : 0.f;
      n += valid ? 1.f : 0.f;
    }
  }
  __shared__ float red[4][2];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  sl = wave_sum(sl); n = wave_sum(n);
  if (lane == 0) { red[w][0] = sl; red[w][1] = n; }
  __syncthreads();
  if (threadIdx.x < 2)
    part[((size_t)b * gridDim.x + blockIdx.x) * 2 + threadIdx.x] =
        ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

__global__ __launch_bounds__(256) void focal_finish_kernel(const float* part, int R, float* coef, float* out3) {
  __shared__ double red[256][2];
  rows_sum_f64<2>(part, R, red);
  if (threadIdx.x != 0) return;
  const double n = red[0][1];
  coef[0] = n > 0.0 ? (float)(1.0 / n) : 0.f;
  out3[0] = n > 0.0 ? (float)(red[0][0] / n) : 0.f; out3[1] = 0.f; out3[2] = 0.f;
}

template <int V>
__global__ __launch_bounds__(256) void focal_bwd_kernel(const float* logits, const int64_t* labels, const float* cw, float gamma,
                                                        const float* coef, const float* gscale, float* dlogits, int HW, int ignore_index) {
  const int b = blockIdx.y, G = HW / V;
  const float w0 = cw[0], w1 = cw[1], w2 = cw[2];
  const float gs = (gscale ? *gscale : 1.f) * coef[0];
  const float* lg = logits + (int64_t)b * 3 * HW;
  const int64_t* lb = labels + (int64_t)b * HW;
  float* dg = dlogits + (int64_t)b * 3 * HW;
  for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < G; g += gridDim.x * blockDim.x) {
    float x[3][V], d[3][V]; int64_t t[V];
    load_px<V>(lg, lb, HW, g, x, t);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const Sm3 q = softmax3(x[0][j], x[1][j], x[2][j]);
      const bool valid = t[j] != ignore_index;
      const int y = valid ? (int)t[j] : 0;
      const float xt = y == 0 ? x[0][j] : (y == 1 ? x[1][j] : x[2][j]);
      const float al = y == 0 ? w0 : (y == 1 ? w1 : w2);
      const float k = valid ? focal_term(xt - q.lse, al, gamma).dldlp * gs : 0.f;     // d l / d log p_y
#pragma unroll
      for (int c = 0; c < 3; ++c) d[c][j] = k * ((y == c ? 1.f : 0.f) - q.p[c]);
    }
    put_px<V>(dg, HW, g, d);
  }
}

// ------------------------------------------------------------------------------------------------
// Lovasz-softmax.  keys / payloads [3][N], N = B * HW flat pixels in (b, h, w) order; the class is grid dimension y.
// ------------------------------------------------------------------------------------------------
template <int V>
__global__ __launch_bounds__(256) void lovasz_key_kernel(const float* logits, const int64_t* labels, uint32_t* keys, uint32_t* vals, int HW,
                                                         int N, int ignore_index) {
  const int b = blockIdx.y, G = HW / V;
  const float* lg = logits + (int64_t)b * 3 * HW;
  const int64_t* lb = labels + (int64_t)b * HW;
  for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < G; g += gridDim.x * blockDim.x) {
    float x[3][V]; int64_t t[V];
    load_px<V>(lg, lb, HW, g, x, t);
    uint32_t k[3][V], v[3][V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const Sm3 q = softmax3(x[0][j], x[1][j], x[2][j]);
      const bool valid = t[j] != ignore_index;
      const uint32_t idx = (uint32_t)(b * HW + V * g + j);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const bool fg = valid && t[j] == c;
        const float e = fminf(fabsf((fg ? 1.f : 0.f) - q.p[c]), 1.f);
        k[c][j] = valid ? kOneBits - __float_as_uint(e) : kInvalidKey;
        v[c][j] = idx | (fg ? kFgBit : 0u);
      }
    }
    const int64_t i0 = (int64_t)b * HW + (int64_t)V * g;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if constexpr (V == 4) {
        u32x4 kk, vv;
        kk[0] = k[c][0]; kk[1] = k[c][1]; kk[2] = k[c][2]; kk[3] = k[c][3];
        vv[0] = v[c][0]; vv[1] = v[c][1]; vv[2] = v[c][2]; vv[3] = v[c][3];
        *(u32x4*)(keys + (int64_t)c * N + i0) = kk;
        *(u32x4*)(vals + (int64_t)c * N + i0) = vv;
      } else {
        keys[(int64_t)c * N + i0] = k[c][0];
        vals[(int64_t)c * N + i0] = v[c][0];
      }
    }
  }
}

// sort pass, launch 1: digit histogram of one tile -> hist[c][digit][tile]
__global__ __launch_bounds__(256) void radix_hist_kernel(const uint32_t* keys, uint32_t* hist, int N, int ntiles, int shift) {
  __shared__ uint32_t h[256];
  const int c = blockIdx.y, tile = blockIdx.x;
  h[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t* k = keys + (int64_t)c * N;
  const int base = tile * kTile;
#pragma unroll
  for (int j = 0; j < kItems; ++j) {
    const int i = base + j * 256 + threadIdx.x;
    if (i < N) atomicAdd(&h[(k[i] >> shift) & 255u], 1u);         // integer LDS counts: order-free
  }
  __syncthreads();
  hist[((int64_t)c * 256 + threadIdx.x) * ntiles + tile] = h[threadIdx.x];
}

// sort pass, launch 2: per (class, digit) exclusive scan over the tiles, in place; dtot[c][digit] = the digit's count
__global__ __launch_bounds__(256) void radix_scan_kernel(uint32_t* hist, uint32_t* dtot, int ntiles) {
  __shared__ uint32_t sh[4];
  const int d = blockIdx.x, c = blockIdx.y;
  uint32_t* row = hist + ((int64_t)c * 256 + d) * ntiles;
  uint32_t carry = 0;
  for (int base = 0; base < ntiles; base += 256) {
    const int i = base + threadIdx.x;
    const uint32_t v = i < ntiles ? row[i] : 0u;
    uint32_t total;
    const uint32_t ex = block_excl_scan(v, sh, total);
    if (i < ntiles) row[i] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) dtot[c * 256 + d] = carry;
}

// sort pass, launch 3: stable scatter.  The tile is walked in kItems rounds of 256 consecutive elements; an element's place among the
// equal digits of its round = the lower lanes of its wave with the same digit (8 ballots) + the counts of the lower waves; the running
// per-digit base carries the earlier rounds.  Elements keep their order within a digit: the sort is stable.
__global__ __launch_bounds__(256) void radix_scatter_kernel(const uint32_t* kin, const uint32_t* vin, uint32_t* kout, uint32_t* vout,
                                                            const uint32_t* hist, const uint32_t* dtot, int N, int ntiles, int shift) {
  __shared__ uint32_t base[256];
  __shared__ uint32_t wc[4][256];
  __shared__ uint32_t sh[4];
  const int c = blockIdx.y, tile = blockIdx.x;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint32_t total;
  const uint32_t dex = block_excl_scan(dtot[c * 256 + threadIdx.x], sh, total);
  base[threadIdx.x] = dex + hist[((int64_t)c * 256 + threadIdx.x) * ntiles + tile];
#pragma unroll
  for (int q = 0; q < 4; ++q) wc[q][threadIdx.x] = 0;
  __syncthreads();
  const uint32_t* ki = kin + (int64_t)c * N;
  const uint32_t* vi = vin + (int64_t)c * N;
  uint32_t* ko = kout + (int64_t)c * N;
  uint32_t* vo = vout + (int64_t)c * N;
  const unsigned long long lt = (1ull << lane) - 1ull;
  for (int j = 0; j < kItems; ++j) {
    const int r0 = tile * kTile + j * 256;
    if (r0 >= N) break;                                           // (uniform over the block)
    const int i = r0 + threadIdx.x;
    const bool in = i < N;
    const uint32_t key = in ? ki[i] : 0xFFFFFFFFu;                // past the end: the last digit, after every real element
    const uint32_t val = in ? vi[i] : 0u;
    const uint32_t d = (key >> shift) & 255u;
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
      ko[pos] = key;
      vo[pos] = val;
    }
    __syncthreads();
    base[threadIdx.x] += wc[0][threadIdx.x] + wc[1][threadIdx.x] + wc[2][threadIdx.x] + wc[3][threadIdx.x];
#pragma unroll
    for (int q = 0; q < 4; ++q) wc[q][threadIdx.x] = 0;
    __syncthreads();
  }
}

// scan, launch 1: per sorted tile, #foreground among the valid ranks and #valid -> cnt[c][tile][2]
__global__ __launch_bounds__(256) void lovasz_count_kernel(const uint32_t* keys, const uint32_t* vals, uint32_t* cnt, int N, int ntiles) {
  __shared__ uint32_t red[4][2];
  const int c = blockIdx.y, tile = blockIdx.x;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint32_t nf = 0, nv = 0;
#pragma unroll
  for (int j = 0; j < kItems; ++j) {
    const int r = tile * kTile + j * 256 + threadIdx.x;
    const bool valid = r < N && keys[(int64_t)c * N + r] != kInvalidKey;
    const bool fg = valid && (vals[(int64_t)c * N + r] & kFgBit);
    nf += (uint32_t)__popcll(__ballot(fg));
    nv += (uint32_t)__popcll(__ballot(valid));
  }
  if (lane == 0) { red[w][0] = nf; red[w][1] = nv; }
  __syncthreads();
  if (threadIdx.x < 2)
    cnt[((int64_t)c * ntiles + tile) * 2 + threadIdx.x] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

// scan, launch 2 (one block per class): fgbase[c][tile] = #foreground before the tile; tot[c] = {gts, #valid}
__global__ __launch_bounds__(256) void lovasz_count_scan_kernel(const uint32_t* cnt, uint32_t* fgbase, uint32_t* tot, int ntiles) {
  __shared__ uint32_t sh[4];
  const int c = blockIdx.x;
  uint32_t cf = 0, cv = 0;
  for (int base = 0; base < ntiles; base += 256) {
    const int i = base + threadIdx.x;
    const uint32_t f = i < ntiles ? cnt[((int64_t)c * ntiles + i) * 2] : 0u;
    const uint32_t v = i < ntiles ? cnt[((int64_t)c * ntiles + i) * 2 + 1] : 0u;
    uint32_t tf, tv;
    const uint32_t ex = block_excl_scan(f, sh, tf);
    block_excl_scan(v, sh, tv);
    if (i < ntiles) fgbase[(int64_t)c * ntiles + i] = cf + ex;
    cf += tf; cv += tv;
  }
  if (threadIdx.x == 0) { tot[2 * c] = cf; tot[2 * c + 1] = cv; }
}

// scan, launch 3: cumulative foreground over the sorted order -> the Lovasz gradient g(r) in closed form from exact integer counts
// (I = gts - cf(r), U = gts + cb(r); g = J(r) - J(r-1) = 1/U at a foreground rank, I / (U (U - 1)) at a background rank), the loss
// partials sum_r e(r) g(r) (fp64), and g scattered to the pixel's own position: gout[c][idx]
__global__ __launch_bounds__(256) void lovasz_grad_kernel(const uint32_t* keys, const uint32_t* vals, const uint32_t* fgbase, const uint32_t* tot,
                                                          float* gout, double* part, int N, int ntiles) {
  __shared__ uint32_t sh[4];
  __shared__ double red[4];
  const int c = blockIdx.y, tile = blockIdx.x;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint32_t gts = tot[2 * c];
  const unsigned long long le = (lane == 63) ? ~0ull : ((1ull << (lane + 1)) - 1ull);
  uint32_t carry = fgbase[(int64_t)c * ntiles + tile];
  double acc = 0.0;
  for (int j = 0; j < kItems; ++j) {
    const int r0 = tile * kTile + j * 256;
    if (r0 >= N) break;                                           // (uniform over the block)
    const int r = r0 + threadIdx.x;
    const uint32_t key = r < N ? keys[(int64_t)c * N + r] : kInvalidKey;
    const uint32_t val = r < N ? vals[(int64_t)c * N + r] : 0u;
    const bool valid = key != kInvalidKey;
    const bool fg = valid && (val & kFgBit);
    const unsigned long long m = __ballot(fg);
    if (lane == 0) sh[w] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t off = 0;
    for (int q = 0; q < w; ++q) off += sh[q];
    const uint32_t round_total = sh[0] + sh[1] + sh[2] + sh[3];
    __syncthreads();
    const uint32_t cf = carry + off + (uint32_t)__popcll(m & le);
    carry += round_total;
    if (valid && gts > 0) {                                       // (valid ranks come first: every rank <= r is valid)
      const uint32_t cb = (uint32_t)r + 1u - cf;
      const double I = (double)(gts - cf), U = (double)(gts + cb);
      const double g = fg ? 1.0 / U : I / ((U - 1.0) * U);
      acc += (double)__uint_as_float(kOneBits - key) * g;
      gout[(int64_t)c * N + (val & ~kFgBit)] = (float)g;
    }
  }
  acc = wave_sum_d(acc);
  if (lane == 0) red[w] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[(int64_t)c * ntiles + tile] = ((red[0] + red[1]) + red[2]) + red[3];
}

// scan, launch 4: loss_c = sum of the partials (fp64, fixed order); n_present on the device; coef[c] = [present] / n_present
__global__ __launch_bounds__(256) void lovasz_finish_kernel(const double* part, const uint32_t* tot, float* coef, float* out3, int ntiles) {
  __shared__ double red[256];
  double lc[3];
  for (int c = 0; c < 3; ++c) {
    double a = 0.0;
    for (int i = threadIdx.x; i < ntiles; i += 256) a += part[(int64_t)c * ntiles + i];
    red[threadIdx.x] = a;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
      __syncthreads();
    }
    lc[c] = red[0];
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  int np = 0;
  double loss = 0.0;
  for (int c = 0; c < 3; ++c)
    if (tot[2 * c] > 0) { ++np; loss += lc[c]; }
  for (int c = 0; c < 3; ++c) coef[c] = (np > 0 && tot[2 * c] > 0) ? (float)(1.0 / np) : 0.f;
  out3[0] = np > 0 ? (float)(loss / np) : 0.f; out3[1] = 0.f; out3[2] = 0.f;
}

// dL/dp_c(i) = sign(p_c - fg) g_c(i) [present] / n_present (sign(0) = 0), then the softmax backward
template <int V>
__global__ __launch_bounds__(256) void lovasz_bwd_kernel(const float* logits, const int64_t* labels, const float* gin, const float* coef,
                                                         const float* gscale, float* dlogits, int HW, int N, int ignore_index) {
  const int b = blockIdx.y, G = HW / V;
  const float sc[3] = {coef[0], coef[1], coef[2]};
  const float gs = gscale ? *gscale : 1.f;
  const float* lg = logits + (int64_t)b * 3 * HW;
  const int64_t* lb = labels + (int64_t)b * HW;
  float* dg = dlogits + (int64_t)b * 3 * HW;
  for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < G; g += gridDim.x * blockDim.x) {
    float x[3][V], d[3][V], gv[3][V]; int64_t t[V];
    load_px<V>(lg, lb, HW, g, x, t);
    const int64_t i0 = (int64_t)b * HW + (int64_t)V * g;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if constexpr (V == 4) {
        const f32x4 v = *(const f32x4*)(gin + (int64_t)c * N + i0);
        gv[c][0] = v[0]; gv[c][1] = v[1]; gv[c][2] = v[2]; gv[c][3] = v[3];
      } else {
        gv[c][0] = gin[(int64_t)c * N + i0];
      }
    }
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const Sm3 q = softmax3(x[0][j], x[1][j], x[2][j]);
      const bool valid = t[j] != ignore_index;
      float h[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float diff = q.p[c] - ((valid && t[j] == c) ? 1.f : 0.f);
        const float s = diff > 0.f ? 1.f : (diff < 0.f ? -1.f : 0.f);
        h[c] = (valid && sc[c] != 0.f && s != 0.f) ? s * gv[c][j] * sc[c] : 0.f;   // (a select: an unwritten g never enters)
      }
      softmax3_bwd(q.p, h, gs, d[0][j], d[1][j], d[2][j]);
    }
    put_px<V>(dg, HW, g, d);
  }
}

// ---- workspace layouts ----
constexpr size_t kAlign = 256;
inline size_t up(size_t x) { return (x + kAlign - 1) / kAlign * kAlign; }

struct LovLayout {
  size_t kA, vA, kB, vB, hist, dtot, cnt, fgbase, tot, part, coef, bytes;
  int ntiles;
};
LovLayout lovasz_layout(int B, int HW) {
  LovLayout L;
  const size_t N = (size_t)B * HW;
  L.ntiles = (int)((N + kTile - 1) / kTile);
  const size_t arr = up(3 * N * sizeof(uint32_t));
  size_t o = 0;
  L.kA = o; o += arr; L.vA = o; o += arr; L.kB = o; o += arr; L.vB = o; o += arr;
  L.hist = o; o += up((size_t)3 * 256 * L.ntiles * sizeof(uint32_t));
  L.dtot = o; o += up(3 * 256 * sizeof(uint32_t));
  L.cnt = o; o += up((size_t)3 * L.ntiles * 2 * sizeof(uint32_t));
  L.fgbase = o; o += up((size_t)3 * L.ntiles * sizeof(uint32_t));
  L.tot = o; o += up(6 * sizeof(uint32_t));
  L.part = o; o += up((size_t)3 * L.ntiles * sizeof(double));
  L.coef = o; o += up(4 * sizeof(float));
  L.bytes = o;
  return L;
}
// dice / focal: part[B][kSplit][K] floats, then coef[8]
inline int red_k(int kind) { return kind == KSMI_LOSS_DICE ? 9 : 2; }
inline size_t red_part_bytes(int B, int kind) { return up((size_t)B * kSplit * red_k(kind) * sizeof(float)); }

bool valid_kind(int kind) { return kind == KSMI_LOSS_DICE || kind == KSMI_LOSS_LOVASZ || kind == KSMI_LOSS_FOCAL; }
bool gamma_ok(float gamma) { return gamma == 0.f || gamma >= 1.f; }
bool al16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

dim3 ew_grid(int HW, int V, int B) {
  const int G = HW / V;
  const int gx = (G + 255) / 256 > 128 ? 128 : (G + 255) / 256;
  return dim3(gx < 1 ? 1 : gx, B);
}

}  // namespace

// 4-pixel groups when every image row of every plane starts on a 16-byte boundary, single pixels otherwise
#define KSMI_VEC(OK4, EXPR4, EXPR1) \
  do {                              \
    if (OK4) { EXPR4; }             \
    else { EXPR1; }                 \
  } while (0)

extern "C" {

size_t ksmi_seg_loss_workspace(int kind, int B, int HW) {
  if (!valid_kind(kind) || B < 1 || HW < 1) return 0;
  if (kind == KSMI_LOSS_LOVASZ) return lovasz_layout(B, HW).bytes;
  return red_part_bytes(B, kind) + up(8 * sizeof(float));
}

int ksmi_seg_loss_forward(int kind, const float* logits, const int64_t* labels, const float* class_w, float gamma, float* out3,
                          void* workspace, int B, int HW, int ignore_index, void* stream) {
  if (!valid_kind(kind)) return ksmi_fail(KSMI_E_ARG, "seg_loss_forward: unknown loss kind");
  if (!logits || !labels || !out3 || !workspace || B < 1 || HW < 1) return ksmi_fail(KSMI_E_ARG, "seg_loss_forward: bad args");
  if ((int64_t)B * HW >= (1ll << 30)) return ksmi_fail(KSMI_E_UNSUPPORTED, "seg_loss_forward: more than 2^30 pixels");
  hipStream_t st = (hipStream_t)stream;
  unsigned char* ws = (unsigned char*)workspace;
  const bool v4 = HW % 4 == 0 && al16(logits) && al16(labels) && al16(workspace);
  if (kind == KSMI_LOSS_DICE || kind == KSMI_LOSS_FOCAL) {
    float* part = (float*)ws;
    float* coef = (float*)(ws + red_part_bytes(B, kind));
    if (kind == KSMI_LOSS_DICE) {
      KSMI_VEC(v4, hipLaunchKernelGGL(dice_fwd_kernel<4>, dim3(kSplit, B), dim3(256), 0, st, logits, labels, part, HW, ignore_index),
               hipLaunchKernelGGL(dice_fwd_kernel<1>, dim3(kSplit, B), dim3(256), 0, st, logits, labels, part, HW, ignore_index));
      hipLaunchKernelGGL(dice_finish_kernel, dim3(1), dim3(256), 0, st, part, B * kSplit, coef, out3);
      return ksmi_check_launch("dice_fwd");
    }
    if (!class_w) return ksmi_fail(KSMI_E_ARG, "seg_loss_forward: focal needs class weights");
    if (!gamma_ok(gamma)) return ksmi_fail(KSMI_E_ARG, "seg_loss_forward: focal gamma must be 0 or >= 1");
    KSMI_VEC(v4, hipLaunchKernelGGL(focal_fwd_kernel<4>, dim3(kSplit, B), dim3(256), 0, st, logits, labels, class_w, gamma, part, HW, ignore_index),
             hipLaunchKernelGGL(focal_fwd_kernel<1>, dim3(kSplit, B), dim3(256), 0, st, logits, labels, class_w, gamma, part, HW, ignore_index));
    hipLaunchKernelGGL(focal_finish_kernel, dim3(1), dim3(256), 0, st, part, B * kSplit, coef, out3);
    return ksmi_check_launch("focal_fwd");
  }
  const LovLayout L = lovasz_layout(B, HW);
  const int N = B * HW, nt = L.ntiles;
  uint32_t* kbuf[2] = {(uint32_t*)(ws + L.kA), (uint32_t*)(ws + L.kB)};
  uint32_t* vbuf[2] = {(uint32_t*)(ws + L.vA), (uint32_t*)(ws + L.vB)};
  uint32_t* hist = (uint32_t*)(ws + L.hist);
  uint32_t* dtot = (uint32_t*)(ws + L.dtot);
  uint32_t* cnt = (uint32_t*)(ws + L.cnt);
  uint32_t* fgbase = (uint32_t*)(ws + L.fgbase);
  uint32_t* tot = (uint32_t*)(ws + L.tot);
  double* part = (double*)(ws + L.part);
  float* coef = (float*)(ws + L.coef);
  KSMI_VEC(v4, hipLaunchKernelGGL(lovasz_key_kernel<4>, ew_grid(HW, 4, B), dim3(256), 0, st, logits, labels, kbuf[0], vbuf[0], HW, N, ignore_index),
           hipLaunchKernelGGL(lovasz_key_kernel<1>, ew_grid(HW, 1, B), dim3(256), 0, st, logits, labels, kbuf[0], vbuf[0], HW, N, ignore_index));
  int rc = ksmi_check_launch("lovasz_key");
  if (rc) return rc;
  for (int pass = 0; pass < 4; ++pass) {                          // A -> B -> A -> B -> A
    const int in = pass & 1, out = in ^ 1, shift = 8 * pass;
    hipLaunchKernelGGL(radix_hist_kernel, dim3(nt, 3), dim3(256), 0, st, kbuf[in], hist, N, nt, shift);
    hipLaunchKernelGGL(radix_scan_kernel, dim3(256, 3), dim3(256), 0, st, hist, dtot, nt);
    hipLaunchKernelGGL(radix_scatter_kernel, dim3(nt, 3), dim3(256), 0, st, kbuf[in], vbuf[in], kbuf[out], vbuf[out], hist, dtot, N, nt, shift);
    rc = ksmi_check_launch("lovasz_radix_pass");
    if (rc) return rc;
  }
  float* gout = (float*)kbuf[1];                                  // the second key array is free once the sort is done
  hipLaunchKernelGGL(lovasz_count_kernel, dim3(nt, 3), dim3(256), 0, st, kbuf[0], vbuf[0], cnt, N, nt);
  hipLaunchKernelGGL(lovasz_count_scan_kernel, dim3(3), dim3(256), 0, st, cnt, fgbase, tot, nt);
  hipLaunchKernelGGL(lovasz_grad_kernel, dim3(nt, 3), dim3(256), 0, st, kbuf[0], vbuf[0], fgbase, tot, gout, part, N, nt);
  hipLaunchKernelGGL(lovasz_finish_kernel, dim3(1), dim3(256), 0, st, part, tot, coef, out3, nt);
  return ksmi_check_launch("lovasz_fwd");
}

int ksmi_seg_loss_backward(int kind, const float* logits, const int64_t* labels, const float* class_w, float gamma, const void* workspace,
                           const float* grad_scale, float* dlogits, int B, int HW, int ignore_index, void* stream) {
  if (!valid_kind(kind)) return ksmi_fail(KSMI_E_ARG, "seg_loss_backward: unknown loss kind");
  if (!logits || !labels || !dlogits || !workspace || B < 1 || HW < 1) return ksmi_fail(KSMI_E_ARG, "seg_loss_backward: bad args");
  if ((int64_t)B * HW >= (1ll << 30)) return ksmi_fail(KSMI_E_UNSUPPORTED, "seg_loss_backward: more than 2^30 pixels");
  hipStream_t st = (hipStream_t)stream;
  const unsigned char* ws = (const unsigned char*)workspace;
  const bool v4 = HW % 4 == 0 && al16(logits) && al16(labels) && al16(dlogits) && al16(workspace);
  if (kind == KSMI_LOSS_DICE) {
    const float* coef = (const float*)(ws + red_part_bytes(B, kind));
    KSMI_VEC(v4, hipLaunchKernelGGL(dice_bwd_kernel<4>, ew_grid(HW, 4, B), dim3(256), 0, st, logits, labels, coef, grad_scale, dlogits, HW, ignore_index),
             hipLaunchKernelGGL(dice_bwd_kernel<1>, ew_grid(HW, 1, B), dim3(256), 0, st, logits, labels, coef, grad_scale, dlogits, HW, ignore_index));
    return ksmi_check_launch("dice_bwd");
  }
  if (kind == KSMI_LOSS_FOCAL) {
    if (!class_w) return ksmi_fail(KSMI_E_ARG, "seg_loss_backward: focal needs class weights");
    if (!gamma_ok(gamma)) return ksmi_fail(KSMI_E_ARG, "seg_loss_backward: focal gamma must be 0 or >= 1");
    const float* coef = (const float*)(ws + red_part_bytes(B, kind));
    KSMI_VEC(v4, hipLaunchKernelGGL(focal_bwd_kernel<4>, ew_grid(HW, 4, B), dim3(256), 0, st, logits, labels, class_w, gamma, coef, grad_scale,
                                    dlogits, HW, ignore_index),
             hipLaunchKernelGGL(focal_bwd_kernel<1>, ew_grid(HW, 1, B), dim3(256), 0, st, logits, labels, class_w, gamma, coef, grad_scale,
                                dlogits, HW, ignore_index));
    return ksmi_check_launch("focal_bwd");
  }
  const LovLayout L = lovasz_layout(B, HW);
  const float* gin = (const float*)(ws + L.kB);
  const float* coef = (const float*)(ws + L.coef);
  const int N = B * HW;
  KSMI_VEC(v4, hipLaunchKernelGGL(lovasz_bwd_kernel<4>, ew_grid(HW, 4, B), dim3(256), 0, st, logits, labels, gin, coef, grad_scale, dlogits, HW, N,
                                  ignore_index),
           hipLaunchKernelGGL(lovasz_bwd_kernel<1>, ew_grid(HW, 1, B), dim3(256), 0, st, logits, labels, gin, coef, grad_scale, dlogits, HW, N,
                              ignore_index));
  return ksmi_check_launch("lovasz_bwd");
}

}  // extern "C"
