// The convolution entry points of include/ksmi.h.  Host only: no kernel lives here.  Which kernel runs a descriptor is decided once
// per direction -- conv_route for the forward, wgrad_route for the weight gradient -- and everything that has to agree with the launch
// (statistics rows, gate support, workspace size, fused bias gradient, the two dispatch hooks) reads the same route the launch reads.
// The kernels and their launch functions: igemm.hip (first generation, igemm1.h), igemm2.hip, igemm3.hip, igemm4.hip, wgrad3.hip and
// the token weight gradient of gemm2.hip.
#include <stdint.h>
#include "../../include/ksmi.h"
#include "errors.h"
#include "igemm1.h"
#include "igemm3.h"
#include "igemm4.h"
#include "wgrad3.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------------- forward
// A persistent kernel writes one statistics row per workgroup (gx), so a descriptor WITH statistics runs on it only when the caller
// sized the buffer for it: ROWS_AS_SET.  ROWS_OF_KERNEL answers for the kernel the descriptor gets once stats_rows is set from it.
enum RowsRule { ROWS_AS_SET, ROWS_OF_KERNEL };
struct ConvRoute { int gen; ksmi_igemm3_geom_t g3; ksmi_igemm4_geom_t g4; };      // gen: 4 igemm4, 3 igemm3, 2 igemm2, 1 first generation

ConvRoute conv_route(const ksmi_conv_desc* d, int dtype, RowsRule rule) {
  static const bool force_v1 = ksmi_knob_is_set("KSMI_IGEMM_V1");      // A/B switch for profiling
  ConvRoute r = {};
  r.gen = 1;
  if (force_v1) return r;
  auto rows_ok = [&](int gx) { return rule == ROWS_OF_KERNEL || d->stats == nullptr || d->stats_rows == gx; };
  // short K, bf16: persistent workgroups with register-resident weights (its statistics rows = workgroups, not tiles)
  if (!d->gate_src && ksmi_igemm3_geom(d, dtype, &r.g3) && rows_ok(r.g3.gx)) r.gen = 3;
  // long K, >= 64 output channels, 3x3: persistent workgroups with halo / weight rings; same statistics-row rule
  else if (ksmi_igemm4_geom(d, dtype, &r.g4) && rows_ok(r.g4.gx)) r.gen = 4;
  else if (ksmi_igemm2_eligible(d, dtype)) r.gen = 2;
  return r;
}

// the route of the launch WITH statistics (and, for `gate`, with the gate epilogue): absent pointers are filled with dummies
ConvRoute conv_route_with_stats(const ksmi_conv_desc* d, int dtype, bool gate) {
  ksmi_conv_desc c = *d;
  if (!c.stats) c.stats = (float*)(uintptr_t)16;
  if (gate && !c.gate_src) { c.gate_src = (const void*)(uintptr_t)16; c.xhat_src = c.gate_src; c.g_mean = (const float*)(uintptr_t)16; c.g_rstd = c.g_mean; }
  return conv_route(&c, dtype, ROWS_OF_KERNEL);
}

// -------------------------------------------------------------------------------------------------------------- weight gradient
enum { CORE_PATCH = 1, CORE_TOKEN1 = 2, CORE_GEMM2 = 3, CORE_WGRAD3 = 4 };
struct WgradRoute {
  int core, reducer;             // CORE_*, KSMI_RED_* (igemm1.h)
  int bias;                      // what the core does with a non-null bias_grad: 0 nothing, 1 the bias gradient, 2 one partial row per split
  bool plain, direct;            // plain row-major nn.Linear gradient; direct: one split, the core writes the gradient itself (no slabs)
  int nsplit;
  ksmi_igemm1_wgeom_t g1;        // taps / kc / npad: the slab of every core; the rest: the patch kernel
  int rps, bt;                   // token cores: rows per split, B-side tile (gemm2)
  ksmi_wgrad3_geom_t g3;
};

bool token_eligible(const ksmi_wgrad_desc* d, int dtype) {
  static const bool generic = ksmi_knob_is_set("KSMI_WGRAD_GENERIC");
  return dtype == KSMI_BF16 && d->KH == 1 && d->KW == 1 && d->stride == 1 && d->pad == 0 && d->nsrc == 1 && d->src[0].scale == nullptr &&
         d->Hin == d->Hout && d->Win == d->Wout && (d->src[0].c_len % 8) == 0 && (d->N % 8) == 0 && d->N >= 64 && d->src[0].c_len >= 64 && !generic;
}

WgradRoute wgrad_route(const ksmi_wgrad_desc* d, int dtype) {
  WgradRoute r = {};
  ksmi_igemm1_wgrad_geom(d, dtype, &r.g1);
  if (token_eligible(d, dtype)) {
    // plain row-major nn.Linear gradient: unit K stride, one tap at offset 0, contiguous k rows
    r.plain = d->gK == 1 && (!d->use_tap_off || d->tap_off[0] == 0) && d->gN >= d->src[0].c_len && d->gN < ((int64_t)1 << 31);
    if (r.plain && !d->uniform_kc)
      for (int i = 0; i < d->nchunks; ++i) r.plain = r.plain && d->k_off[i] == i * r.g1.kc;
    ksmi_gemm2_tn_geom(d->B * d->Hout * d->Wout, d->nchunks * r.g1.kc, r.g1.npad, r.plain, &r.nsplit, &r.rps, &r.bt);
    const bool gemm2 = ksmi_gemm2_tn_enabled(d->src[0].c_len, d->N, r.rps);
    r.core = gemm2 ? CORE_GEMM2 : CORE_TOKEN1;
    r.direct = gemm2 && r.plain && r.nsplit == 1;
    // KSMI_SLAB_BIAS=0: the split mode leaves the bias gradient to a channel_sum pass (the round-4 route; same-box A/B)
    static const bool slab_bias = ksmi_knob_int("KSMI_SLAB_BIAS", 1) != 0;
    if (gemm2) r.bias = r.direct ? 1 : (r.plain && slab_bias) ? 2 : 0;
    // many thin slabs (small matrices): the 8-lanes-per-element tree reducer hides the slab walk better.  The transposing reducer
    // writes the plain gradient in 128-byte runs (KSMI_TN_REDUCE_TR=0: the element-wise reducer of round 1); the first-generation
    // core never takes it
    static const int tr_on = ksmi_knob_int("KSMI_TN_REDUCE_TR", 1);
    r.reducer = r.direct ? KSMI_RED_NONE : r.nsplit > 16 ? KSMI_RED_TREE : (gemm2 && tr_on && r.plain) ? KSMI_RED_TN_TR : KSMI_RED_TN;
  } else if (ksmi_wgrad3_geom(d, dtype == KSMI_BF16 ? KSMI_BF16 : KSMI_F32, &r.g3)) {
    // 3x3 stride-1 bf16 gradients with whole 32-channel chunks: channel-owner kernel, same slab layout
    r.core = CORE_WGRAD3; r.reducer = KSMI_RED_WGRAD3; r.nsplit = r.g3.nsplit;
  } else {
    r.core = CORE_PATCH; r.reducer = KSMI_RED_TREE; r.nsplit = r.g1.nsplit;
  }
  return r;
}

int launch_reducer(const ksmi_wgrad_desc* d, const WgradRoute& r, hipStream_t st) {
  if (r.reducer == KSMI_RED_NONE) return 0;
  if (r.reducer == KSMI_RED_WGRAD3) return ksmi_wgrad3_reduce(d, &r.g3, st);
  return ksmi_igemm1_reduce(d, r.reducer, r.g1.taps, r.g1.kc, st);
}

}  // namespace

extern "C" {

int ksmi_chunk_elems(int dtype) { return dtype == KSMI_BF16 ? 32 : 16; }

int ksmi_conv_grid_m(const ksmi_conv_desc* d) {
  const int tilesX = (d->Wout + d->TW - 1) / d->TW, tilesY = (d->Hout + d->TH - 1) / d->TH;
  return d->B * tilesX * tilesY;
}

size_t ksmi_desc_size(int which) {
  static const size_t size[] = {sizeof(ksmi_conv_desc), sizeof(ksmi_wgrad_desc), sizeof(ksmi_pack_desc), sizeof(ksmi_rowsum_desc), sizeof(ksmi_tiff_info)};
  return which >= 0 && which < 5 ? size[which] : 0;
}

int ksmi_conv_gate_supported(const ksmi_conv_desc* d, int dtype) {
  return d && conv_route_with_stats(d, dtype, true).gen == 4 ? 1 : 0;
}

int ksmi_conv_stats_rows(const ksmi_conv_desc* d, int dtype) {
  if (!d) return 0;
  const ConvRoute r = conv_route_with_stats(d, dtype, false);
  return r.gen == 3 ? r.g3.gx : r.gen == 4 ? r.g4.gx : ksmi_conv_grid_m(d);
}

// info[1] = 1 when the chosen launcher has an instantiated kernel for the geometry it chose (a geometry function that accepts a
// descriptor its launcher cannot start makes the forward raise instead of falling through: ADVICE round 5)
int ksmi_conv_dispatch_info(const ksmi_conv_desc* d, int dtype, int32_t* info) {
  if (!d || !info) return ksmi_fail(KSMI_E_ARG, "conv_dispatch_info: null argument");
  for (int i = 0; i < 8; ++i) info[i] = 0;
  const ConvRoute r = conv_route(d, dtype, ROWS_AS_SET);
  info[0] = r.gen; info[1] = 1;
  if (r.gen == 3) { info[6] = r.g3.gx; info[7] = r.g3.gy; }
  if (r.gen == 4) {
    info[1] = ksmi_igemm4_launchable(d, &r.g4) ? 1 : 0;
    info[2] = r.g4.WM; info[3] = r.g4.NF; info[4] = r.g4.nwv; info[5] = r.g4.deep; info[6] = r.g4.gx; info[7] = r.g4.gy;
  }
  return 0;
}

int ksmi_conv_forward(const ksmi_conv_desc* d, int dtype, void* stream) {
  if (!d || d->nsrc < 1 || d->nsrc > KSMI_MAX_SRC || d->ndst < 1 || d->ndst > KSMI_MAX_SRC || d->nchunks < 1 ||
      (d->nchunks > KSMI_MAX_CHUNKS && !(d->uniform_kc && d->nsrc == 1)))
    return ksmi_fail(KSMI_E_ARG, "conv: bad descriptor");
  if (dtype != KSMI_BF16 && dtype != KSMI_F32) return ksmi_fail(KSMI_E_ARG, "conv: bad dtype");
  const ConvRoute r = conv_route(d, dtype, ROWS_AS_SET);
  if (r.gen == 3) return ksmi_igemm3_launch(d, &r.g3, (hipStream_t)stream);
  if (r.gen == 4) return ksmi_igemm4_launch(d, &r.g4, (hipStream_t)stream);
  // the tile kernels: one statistics row per M-tile, no gate epilogue
  if (d->gate_src) return ksmi_fail(KSMI_E_UNSUPPORTED, "conv: the gate epilogue needs the persistent long-K kernel (ksmi_conv_gate_supported)");
  if (d->stats && d->stats_rows != 0 && d->stats_rows != ksmi_conv_grid_m(d))
    return ksmi_fail(KSMI_E_ARG, "conv: stats_rows does not match the kernel this descriptor runs on (set it from ksmi_conv_stats_rows)");
  if (r.gen == 2) return ksmi_igemm2_launch(d, dtype, (hipStream_t)stream);
  if (d->alpha != 0.f || d->resid || d->relu_out || d->uniform_kc)
    return ksmi_fail(KSMI_E_UNSUPPORTED, "conv: alpha/resid/relu_out/uniform chunks need whole-chunk sources (igemm2 path)");
  return ksmi_igemm1_forward(d, dtype, (hipStream_t)stream);
}

size_t ksmi_conv_wgrad_workspace(const ksmi_wgrad_desc* d, int dtype) {
  const WgradRoute r = wgrad_route(d, dtype);
  return (size_t)r.nsplit * r.g1.taps * d->nchunks * r.g1.kc * r.g1.npad * sizeof(float);
}

// 1: ksmi_conv_wgrad(d) also writes d->bias_grad (the token-GEMM path of gemm2.hip in its one-split, direct-write mode)
// 2 (round 5): the split (slab) mode of the same path writes the PARTIAL column sums of dY, one row per split, to d->bias_grad
//    [d->nsplit][d->N] floats (overwritten, not accumulated); the caller sums the rows into the bias gradient
int ksmi_conv_wgrad_fuses_bias(const ksmi_wgrad_desc* d, int dtype) {
  static const bool off = ksmi_knob_is_set("KSMI_NO_FUSED_BIAS_GRAD");      // the caller's opt-out: it then leaves bias_grad null
  return d && !off ? wgrad_route(d, dtype).bias : 0;
}

int ksmi_conv_wgrad_dispatch_info(const ksmi_wgrad_desc* d, int dtype, int32_t* info) {
  if (!d || !info) return ksmi_fail(KSMI_E_ARG, "conv_wgrad_dispatch_info: null argument");
  for (int i = 0; i < 8; ++i) info[i] = 0;
  const WgradRoute r = wgrad_route(d, dtype);
  info[0] = r.core; info[1] = r.reducer; info[2] = r.nsplit; info[3] = r.bias;
  info[4] = r.core == CORE_GEMM2 ? r.bt : r.core == CORE_PATCH ? r.g1.nt : 0;
  return 0;
}

int ksmi_conv_wgrad(const ksmi_wgrad_desc* d, int dtype, void* stream) {
  if (!d || d->nsrc < 1 || d->nsrc > KSMI_MAX_SRC || d->nchunks < 1 || (d->nchunks > KSMI_MAX_CHUNKS && !(d->uniform_kc && d->nsrc == 1)))
    return ksmi_fail(KSMI_E_ARG, "wgrad: bad descriptor");
  if (dtype != KSMI_BF16 && dtype != KSMI_F32) return ksmi_fail(KSMI_E_ARG, "wgrad: bad dtype");
  const hipStream_t st = (hipStream_t)stream;
  const WgradRoute r = wgrad_route(d, dtype);
  if (d->TH * d->TW > 256) return ksmi_fail(KSMI_E_ARG, "wgrad: patch too large");
  if (d->nsplit != r.nsplit) return ksmi_fail(KSMI_E_ARG, "wgrad: nsplit does not match ksmi_conv_wgrad_workspace geometry");
  int rc;
  switch (r.core) {
    case CORE_WGRAD3: rc = ksmi_wgrad3_launch(d, &r.g3, st); break;
    case CORE_GEMM2:
      // bias_grad: the final gradient in direct mode; in slab mode (plain layers only) the partial column sums of dY per split
      rc = ksmi_gemm2_tn((const uint16_t*)d->src[0].ptr + d->src[0].c_off, d->src[0].C, (const uint16_t*)d->dy + d->dy_c_off, d->dyC, d->partial,
                         r.g1.npad, r.direct ? d->grad : nullptr, d->gN, d->B * d->Hout * d->Wout, d->src[0].c_len, d->N, d->nchunks * r.g1.kc,
                         r.nsplit, r.rps, r.bt, d->accumulate, r.bias ? d->bias_grad : nullptr, d->bias_accumulate, st);
      break;
    case CORE_TOKEN1: rc = ksmi_igemm1_wgrad_token(d, r.g1.kc, r.rps, st); break;
    default: rc = ksmi_igemm1_wgrad_patch(d, dtype, &r.g1, st); break;      // (its 4 GiB and kernel-size checks come first in there)
  }
  return rc ? rc : launch_reducer(d, r, st);
}

}  // extern "C"
