// On-device augmentation views (dataset/Dataset.py:171-190 create_views, :864-983 SSLDataset; utilities/augmentations.py): the
// albumentations pipeline RandomResizedCrop(224, interpolation=3) -> HorizontalFlip / VerticalFlip -> MultiplicativeNoise /
// GaussNoise / CoarseDropout fused with the Dataset's clamp -> nan_to_num -> Normalize (sar_preprocess_kernel, cformer.hip) in ONE
// pass over raw fp32 tiles [B][C][224][224].  Per sample one int32 row {y0, x0, h, w, flip_h, flip_v} of a device table.
//
// Resize (formula-pinned; cv2 is in no image of this project).  albumentations 1.3.1 hands interpolation = 3 to cv2.resize as
// cv2.INTER_AREA.  A crop is never larger than the tile, so scale = w/224 <= 1 on both axes.  OpenCV's resize() runs its true
// area filter only when shrinking (scale_x >= 1 and scale_y >= 1; 224 x 224 -> 224 x 224 is a copy); otherwise INTER_AREA takes
// the two-tap linear path in "area mode" (imgproc/resize.cpp: ksize = 2, area_mode = true), whose coefficients are
//     sx = floor(dx * scale), fx = (dx + 1) - (sx + 1) * inv_scale, fx = fx <= 0 ? 0 : fx - floor(fx)        inv_scale = 224/w
// With q = dx*w, sx = q / 224, r = q % 224:  (dx+1) - (sx+1)*224/w = (q + w - (sx+1)*224) / w = (r + w - 224) / w, which is < 1
// because r < 224, so the `- floor(fx)` never fires.  In exact integers:
//     sx = q / 224;  fx = max(0, r + w - 224) / w (one fp32 division);  sx >= w-1 -> sx = w-1, fx = 0 (OpenCV's right-edge clamp)
// Rows alike with h.  Value: horizontal pass on both source rows, t = a*(1-fx) + b*fx, then vertical, all fp32, every product and
// sum rounded on its own (no contraction, so the host restatement kurosiwo_amd/augment.py:apply_cpu gives the same bits).  A zero
// coefficient selects the tap instead of multiplying (a*1 + b*0 would turn -0 into +0 and, without a clamp, drag a NaN neighbour
// in): the identity row {0, 0, 224, 224, 0, 0} is therefore bit-identical to ksmi_sar_preprocess.  An integer factor is pure
// replication.  Each tap gets the Dataset's clamp / nan_to_num BEFORE it is interpolated (the reference augments the clamped
// image, Dataset.py:164-168 then :792-805); Normalize comes last (:812-822).
// Masks (labels, valid) go through cv2.INTER_NEAREST as albumentations does: sx = min(dx*w/224, w-1), integers in and out.
// Flips act on the resized tile: out[.., x] = res[.., 223-x].
//
// The memory-bound shape: one thread = four neighbouring output pixels of one row = one 16-byte store; 256 threads per block, one
// (sample, channel) plane per blockIdx.y; the row's (sy, fy) once per thread, the columns' (sx, fx) four times; no LDS (the taps of
// neighbouring lanes fall into the same or the next cache line).
#include "common.h"
#include "../../include/ksmi.h"
#include "errors.h"

namespace {

constexpr int T = 224;                      // tile edge of the archive
constexpr int QUADS = T * (T / 4);          // 16-byte stores per plane
// sites of the counter-based stream (common.h) used by the per-pixel ops: far from the small site numbers of the model plans
constexpr uint32_t SITE_AUG = 0x41554700u;
enum { S_MULT_ON = 0, S_MULT_VAL, S_GAUSS_ON, S_GAUSS_VAR, S_GAUSS_U1, S_GAUSS_U2, S_CUT_ON, S_CUT_POS };

struct Box { int y0, x0, h, w, fh, fv; };

// the table is device data nobody validated: every row is forced inside the tile here, so no tap can leave the plane
__device__ __forceinline__ Box load_box(const int32_t* __restrict__ params, const int32_t* __restrict__ fallback, int b) {
  Box k;
  if (fallback && fallback[b] == 0) { k.y0 = 0; k.x0 = 0; k.h = T; k.w = T; k.fh = 0; k.fv = 0; return k; }
  const int32_t* p = params + (size_t)b * 6;
  k.h = min(max(p[2], 1), T); k.w = min(max(p[3], 1), T);
  k.y0 = min(max(p[0], 0), T - k.h); k.x0 = min(max(p[1], 0), T - k.w);
  k.fh = p[4] != 0; k.fv = p[5] != 0;
  return k;
}

__device__ __forceinline__ void area_coef(int d, int n, int& s, float& f) {
  const int q = d * n;
  s = q / T;
  const int num = q - s * T + n - T;
  f = num > 0 ? (float)num / (float)n : 0.f;
  if (s >= n - 1) { s = n - 1; f = 0.f; }
}
__device__ __forceinline__ float prep(float v, float clampv) {
  if (clampv >= 0.f) v = (v != v) ? clampv : fminf(fmaxf(v, 0.f), clampv);
  return v;
}
__device__ __forceinline__ float lerp_rn(float a, float b, float f) {
  return f == 0.f ? a : __fadd_rn(__fmul_rn(a, __fsub_rn(1.f, f)), __fmul_rn(b, f));
}
__device__ __forceinline__ float u01(uint32_t r) { return (float)(r >> 8) * (1.f / 16777216.f); }     // [0, 1), exact in fp32
__device__ __forceinline__ uint32_t below(uint32_t r, uint32_t n) { return (uint32_t)(((uint64_t)r * n) >> 32); }   // [0, n)

struct PixelOps {
  uint32_t mult_thr; float mult_lo, mult_hi;
  uint32_t gauss_thr; float var_lo, var_hi;
  uint32_t cut_thr; int cut_holes, cut_h, cut_w;
  int order;                                  // three 2-bit slots, first op in the low bits: 1 mult, 2 gauss, 3 dropout
};

__global__ __launch_bounds__(256) void augment_views_kernel(const float* __restrict__ x, const int32_t* __restrict__ params,
                                                            const int32_t* __restrict__ fallback, const float* __restrict__ mean,
                                                            const float* __restrict__ stdv, float* __restrict__ y, int C, float clampv,
                                                            PixelOps ops, const uint32_t* __restrict__ state) {
  const int quad = blockIdx.x * 256 + threadIdx.x;
  if (quad >= QUADS) return;
  const int plane = blockIdx.y, b = plane / C, c = plane - b * C;
  const int oy = quad / (T / 4), ox0 = (quad - oy * (T / 4)) * 4;
  const bool ident = fallback && fallback[b] == 0;
  const Box k = load_box(params, fallback, b);
  int sy; float fy;
  area_coef(k.fv ? T - 1 - oy : oy, k.h, sy, fy);
  const float* r0 = x + (size_t)plane * T * T + (size_t)(k.y0 + sy) * T + k.x0;
  const float* r1 = r0 + (sy + 1 < k.h ? T : 0);
  float v[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int ox = ox0 + j;
    int sx; float fx;
    area_coef(k.fh ? T - 1 - ox : ox, k.w, sx, fx);
    const int sb = min(sx + 1, k.w - 1);
    float top = prep(r0[sx], clampv);
    if (fx != 0.f) top = lerp_rn(top, prep(r0[sb], clampv), fx);
    if (fy != 0.f) {
      float bot = prep(r1[sx], clampv);
      if (fx != 0.f) bot = lerp_rn(bot, prep(r1[sb], clampv), fx);
      top = lerp_rn(top, bot, fy);
    }
    v[j] = top;
  }
  if (ops.order && !ident) {
    for (int slot = 0; slot < 3; ++slot) {
      const int op = (ops.order >> (2 * slot)) & 3;
      if (op == 1) {                            // MultiplicativeNoise (per_channel = elementwise = False): one factor per sample
        if (ksmi_rng_u32(ksmi_rng_key(state, SITE_AUG + S_MULT_ON), b) < ops.mult_thr) {
          const float m = __fadd_rn(ops.mult_lo, __fmul_rn(__fsub_rn(ops.mult_hi, ops.mult_lo), u01(ksmi_rng_u32(ksmi_rng_key(state, SITE_AUG + S_MULT_VAL), b))));
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] = __fmul_rn(v[j], m);
        }
      } else if (op == 2) {                     // GaussNoise (mean 0, per_channel = True): var ~ U(var_limit) per sample, N(0, var) per element
        if (ksmi_rng_u32(ksmi_rng_key(state, SITE_AUG + S_GAUSS_ON), b) < ops.gauss_thr) {
          const float var = ops.var_lo + (ops.var_hi - ops.var_lo) * u01(ksmi_rng_u32(ksmi_rng_key(state, SITE_AUG + S_GAUSS_VAR), b));
          const float sigma = sqrtf(var);
          const uint32_t k1 = ksmi_rng_key(state, SITE_AUG + S_GAUSS_U1), k2 = ksmi_rng_key(state, SITE_AUG + S_GAUSS_U2);
          const uint32_t e0 = ((uint32_t)plane * T + oy) * T + ox0;
#pragma unroll
          for (int j = 0; j < 4; ++j) {           // Box-Muller on two draws of the element
            const float u1 = ((float)(ksmi_rng_u32(k1, e0 + j) >> 8) + 1.f) * (1.f / 16777216.f);     // (0, 1]
            const float u2 = u01(ksmi_rng_u32(k2, e0 + j));
            v[j] += sigma * sqrtf(-2.f * logf(u1)) * cosf(6.28318530717958647692f * u2);
          }
        }
      } else if (op == 3) {                     // CoarseDropout (fill 0, masks untouched): the same holes in every channel
        if (ksmi_rng_u32(ksmi_rng_key(state, SITE_AUG + S_CUT_ON), b) < ops.cut_thr) {
          const uint32_t kp = ksmi_rng_key(state, SITE_AUG + S_CUT_POS);
          for (int hole = 0; hole < ops.cut_holes; ++hole) {
            const int hy = (int)below(ksmi_rng_u32(kp, (uint32_t)b * 64 + 2 * hole), T - ops.cut_h + 1);
            const int hx = (int)below(ksmi_rng_u32(kp, (uint32_t)b * 64 + 2 * hole + 1), T - ops.cut_w + 1);
            if (oy < hy || oy >= hy + ops.cut_h) continue;
#pragma unroll
            for (int j = 0; j < 4; ++j)
              if (ox0 + j >= hx && ox0 + j < hx + ops.cut_w) v[j] = 0.f;
          }
        }
      }
    }
  }
  const float m = mean[c], s = stdv[c];
  f32x4 o;
#pragma unroll
  for (int j = 0; j < 4; ++j) o[j] = (v[j] - m) / s;
  *(f32x4*)(y + (size_t)plane * T * T + (size_t)oy * T + ox0) = o;
}

// nearest-neighbour view of a mask plane [B][224][224] of E-byte elements (uint8 / fp32 / int64 labels are all moved as bits);
// y == nullptr: count only.  count[b] += number of non-zero elements of the VIEW (the reference's torch.sum(valid) > 0 test).
template <typename E>
__global__ __launch_bounds__(256) void augment_masks_kernel(const E* __restrict__ x, E* __restrict__ y, const int32_t* __restrict__ params,
                                                            const int32_t* __restrict__ fallback, int32_t* __restrict__ count) {
  const int quad = blockIdx.x * 256 + threadIdx.x;
  const int b = blockIdx.y;
  int nz = 0;
  if (quad < QUADS) {
    const int oy = quad / (T / 4), ox0 = (quad - oy * (T / 4)) * 4;
    const Box k = load_box(params, fallback, b);
    const int dy = k.fv ? T - 1 - oy : oy;
    const int sy = min(dy * k.h / T, k.h - 1);
    const E* row = x + (size_t)b * T * T + (size_t)(k.y0 + sy) * T + k.x0;
    E* out = y ? y + (size_t)b * T * T + (size_t)oy * T + ox0 : nullptr;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int dx = k.fh ? T - 1 - (ox0 + j) : ox0 + j;
      const E e = row[min(dx * k.w / T, k.w - 1)];
      nz += e != (E)0;
      if (out) out[j] = e;
    }
  }
  if (count) {                                  // (wave-uniform: count is a kernel argument) one atomic per wave
    for (int o = 32; o > 0; o >>= 1) nz += __shfl_xor(nz, o, 64);
    if ((threadIdx.x & 63) == 0 && nz) atomicAdd(count + b, nz);
  }
}

}  // namespace

int ksmi_augment_views(const float* x, const int32_t* params, const int32_t* fallback, const float* mean, const float* stdv, float* y, int B, int C,
                       int H, int W, float clamp_input, uint32_t mult_thr, float mult_lo, float mult_hi, uint32_t gauss_thr, float gauss_var_lo,
                       float gauss_var_hi, uint32_t cut_thr, int cut_holes, int cut_h, int cut_w, int op_order, const uint32_t* rng_state,
                       void* stream) {
  if (!x || !params || !mean || !stdv || !y) return ksmi_fail(KSMI_E_ARG, "augment_views: null pointer");
  if (x == y) return ksmi_fail(KSMI_E_ARG, "augment_views: the gather cannot run in place");
  if (H != T || W != T) return ksmi_fail(KSMI_E_UNSUPPORTED, "augment_views: tiles are 224 x 224");
  if (B < 0 || C <= 0 || (int64_t)B * C > 65535) return ksmi_fail(KSMI_E_ARG, "augment_views: B*C must be in [0, 65535]");
  if (op_order < 0 || op_order > 63) return ksmi_fail(KSMI_E_ARG, "augment_views: op_order");
  if (op_order && !rng_state) return ksmi_fail(KSMI_E_ARG, "augment_views: the per-pixel ops need the rng state");
  for (int s = 0; s < 3; ++s)
    if (((op_order >> (2 * s)) & 3) == 3 && (cut_holes < 0 || cut_holes > 32 || cut_h < 1 || cut_h > T || cut_w < 1 || cut_w > T))
      return ksmi_fail(KSMI_E_ARG, "augment_views: dropout holes (at most 32, inside the tile)");
  if (B == 0) return 0;
  PixelOps ops{mult_thr, mult_lo, mult_hi, gauss_thr, gauss_var_lo, gauss_var_hi, cut_thr, cut_holes, cut_h, cut_w, op_order};
  KSMI_NOTE(augment_views_kernel);
  hipLaunchKernelGGL(augment_views_kernel, dim3((QUADS + 255) / 256, B * C), dim3(256), 0, (hipStream_t)stream, x, params, fallback, mean, stdv, y, C,
                     clamp_input, ops, rng_state);
  return ksmi_check_launch("augment_views");
}

int ksmi_augment_masks(const void* x, void* y, const int32_t* params, const int32_t* fallback, int32_t* count, int B, int H, int W, int elem_bytes,
                       void* stream) {
  if (!x || !params || (!y && !count)) return ksmi_fail(KSMI_E_ARG, "augment_masks: null pointer");
  if (x == y) return ksmi_fail(KSMI_E_ARG, "augment_masks: the gather cannot run in place");
  if (H != T || W != T) return ksmi_fail(KSMI_E_UNSUPPORTED, "augment_masks: tiles are 224 x 224");
  if (B < 0 || B > 65535) return ksmi_fail(KSMI_E_ARG, "augment_masks: B must be in [0, 65535]");
  if (elem_bytes != 1 && elem_bytes != 4 && elem_bytes != 8) return ksmi_fail(KSMI_E_ARG, "augment_masks: elements of 1, 4 or 8 bytes");
  if (B == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  if (count && hipMemsetAsync(count, 0, (size_t)B * sizeof(int32_t), st) != hipSuccess) return ksmi_fail(KSMI_E_ARG, "augment_masks: memset of the counters");
  const dim3 grid((QUADS + 255) / 256, B), block(256);
  if (elem_bytes == 1)
    hipLaunchKernelGGL(augment_masks_kernel<uint8_t>, grid, block, 0, st, (const uint8_t*)x, (uint8_t*)y, params, fallback, count);
  else if (elem_bytes == 4)
    hipLaunchKernelGGL(augment_masks_kernel<uint32_t>, grid, block, 0, st, (const uint32_t*)x, (uint32_t*)y, params, fallback, count);
  else
    hipLaunchKernelGGL(augment_masks_kernel<uint64_t>, grid, block, 0, st, (const uint64_t*)x, (uint64_t*)y, params, fallback, count);
  return ksmi_check_launch("augment_masks");
}
