// igemm.hip: the first-generation kernels (tile forward, patch and token weight gradient) and the three slab reducers, behind plain
// launch functions.  Which of them runs a descriptor is decided in conv_api.hip (conv_route / wgrad_route).
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/ksmi.h"

int ksmi_igemm1_forward(const ksmi_conv_desc* d, int dtype, hipStream_t st);

// patch weight gradient: column tile, pixel splits and LDS of igemm_wgrad_kernel; taps / kc / npad describe the slab
// [nsplit][taps][nchunks * kc][npad] of every weight-gradient core
struct ksmi_igemm1_wgeom_t {
  int taps, kc, npad;
  int nt, bn, ntiles;          // 16-column fragments per workgroup (1 | 2 | 4), columns per workgroup, column tiles
  int patches, pps, nsplit;    // patches, patches per split, splits (= partial slabs)
  size_t lds;
};
void ksmi_igemm1_wgrad_geom(const ksmi_wgrad_desc* d, int dtype, ksmi_igemm1_wgeom_t* g);
// the cores write slabs only; the caller reduces them
int ksmi_igemm1_wgrad_patch(const ksmi_wgrad_desc* d, int dtype, const ksmi_igemm1_wgeom_t* g, hipStream_t st);
int ksmi_igemm1_wgrad_token(const ksmi_wgrad_desc* d, int kc, int rows_per_split, hipStream_t st);   // gemm_tn_wgrad_kernel (bf16)

// slabs -> fp32 gradient.  KSMI_RED_WGRAD3 is ksmi_wgrad3_reduce (wgrad3.h); the other three are launched by ksmi_igemm1_reduce
enum { KSMI_RED_NONE = 0, KSMI_RED_WGRAD3 = 1, KSMI_RED_TREE = 2, KSMI_RED_TN_TR = 3, KSMI_RED_TN = 4 };
int ksmi_igemm1_reduce(const ksmi_wgrad_desc* d, int reducer, int taps, int kc, hipStream_t st);
