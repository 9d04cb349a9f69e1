// Polygon output for a scene's class map, on the device (kurosiwo_amd/scene.py: scan_i32, boundary_edges, trace_rings, polygonize;
// predict.py --polygons): the boundary rings of the 4-connected components of the selected classes, as vertex lists.  Integers
// throughout: the results do not depend on launch geometry or arrival order, and equal the sequential walk of tests/polygon_ref.py
// bit for bit.  Launch boundaries are the only ordering between workgroups; scratch is the caller's; the host reads three counts
// (E edges, R rings, V vertices) to size the next buffers and nothing else.
//
// Image coordinates: x right, y down; a vertex is a pixel corner.  Side s of pixel p = y * Ws + x is walked clockwise on screen, the
// pixel on the right of the heading: 0 top (x, y) -> (x+1, y), 1 right -> (x+1, y+1), 2 bottom -> (x, y+1), 3 left -> (x, y).  A side
// is a boundary edge when p's class is selected (bit c of the mask selects class c, 0 <= c <= 62) and the pixel across it is outside
// the scene or has another label; its edge id is 4 * p + s, its compact index its rank among all boundary edges by edge id.
//
//   scan_i32            exclusive prefix sum in three passes: tile_sums_kernel (one workgroup per SCAN_TILE elements), the scan of the
//                       tile sums (the same three passes again, as deep as n needs; a single tile ends the recursion and writes the
//                       total), scan_tile_kernel (each workgroup scans its tile from its scanned tile sum).  A tile goes through LDS
//                       whole before it is written, so out may alias in.
//   scene_edge_count    counts[p] = boundary sides of p, 0 .. 4.
//   scene_edge_emit     for the j-th boundary side s of p: k = offsets[p] + j, eid[k] = 4 p + s, succ[k] = the compact index of the
//                       successor.  The edge ends at vertex v with heading s; with L the pixel ahead-left of v and R the pixel
//                       ahead-right: side s-1 of L when label(L) == label(p), else side s of R when label(R) == label(p), else side
//                       s+1 of p.  The successor's compact index is offsets[q] + its pixel's lower boundary sides, recomputed.
//   scene_ring_trace    pointer doubling over succ, double-buffered (a round reads one pair of arrays and writes the other), ceil(log2 E)
//                       rounds per phase.  Phase one carries (succ^(2^r)(k), min of k .. succ^(2^r - 1)(k)) and leaves ring_min.  Phase
//                       two cuts every cycle before its smallest edge and carries (next or -1, steps walked): d[k] = steps from k to the
//                       last edge of its ring; rank[k] = d[ring_min[k]] - d[k].  `phases` runs one of the two alone (the probe times
//                       them apart).
//   scene_ring_heads    flags[k] = ring_min[k] == k; their scan numbers the rings in ascending ring id.
//   scene_ring_table    per ring r: ring_id (the edge id of its smallest edge), label, and its length, written by the one edge whose
//                       successor is the smallest edge (rank + 1).
//   scene_ring_order    the edges in ring order: position = ring offset + rank; the edge id, the ring number and the turn flag (the
//                       successor has another side number) land there.
//   scene_ring_verts    the end vertex of every turning edge at its scanned position, start[] per ring, and area2[r] = the sum of
//                       x0 * y1 - x1 * y0 over the ring's edges in int64.  One ring can hold millions of edges and they are contiguous in
//                       ring order: a wave whose lanes share one ring reduces by shuffles, a block combines per ring in LDS, and the
//                       table's entries issue the global integer adds (component_sizes_kernel of sieve.hip, for sums).
//
// Every index that comes out of a caller's array is checked against its bound before it is used as an address: arrays that do not
// describe rings give meaningless numbers, never an access outside the buffers.
#include "common.h"
#include "../../include/ksmi.h"
#include "errors.h"

namespace {

constexpr int SCAN_TILE = 2048;                // scene.SCAN_TILE: elements one workgroup scans
constexpr int SCAN_PER = SCAN_TILE / 256;      // consecutive elements per thread
constexpr int SCAN_LDS = SCAN_TILE + SCAN_TILE / SCAN_PER;     // one pad word per thread's run: a stride of 9 words over the banks
constexpr int64_t MAX_N = 0x7fffffff;
constexpr int64_t POLY_MAX_PIXELS = (1ll << 29) - 1;           // 4 * p + 3 and E fit int32
constexpr int VT_PER_BLOCK = 1024;             // ring-order positions per block of ring_verts_kernel
constexpr int VT_SLOTS = VT_PER_BLOCK / 4 + 1; // rings a block can meet: a ring has at least 4 edges

// exclusive prefix of one value per thread over a block of 256; total = the block's sum.  wsum: 4 words of LDS
__device__ __forceinline__ int block_scan_256(int v, int* wsum, int& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(x, o);
    if (lane >= o) x += t;
  }
  __syncthreads();                             // wsum may still be read from a call before
  if (lane == 63) wsum[w] = x;
  __syncthreads();
  int before = 0, all = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int s = wsum[i];
    before += i < w ? s : 0;
    all += s;
  }
  total = all;
  return before + x - v;
}

__global__ __launch_bounds__(256) void tile_sums_kernel(const int32_t* __restrict__ in, int64_t n, int32_t* __restrict__ sums) {
  __shared__ int wsum[4];
  const int64_t base = (int64_t)blockIdx.x * SCAN_TILE;
  int v = 0;
#pragma unroll
  for (int j = 0; j < SCAN_PER; ++j) {
    const int64_t i = base + j * 256 + threadIdx.x;
    v += i < n ? in[i] : 0;
  }
  int total;
  block_scan_256(v, wsum, total);
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// out[i] = offsets[block] + the sum of the tile's elements before i (offsets NULL: 0); total (NULL, or with a grid of one): the sum
__global__ __launch_bounds__(256) void scan_tile_kernel(const int32_t* in, int32_t* out, int64_t n, const int32_t* __restrict__ offsets,
                                                        int64_t* __restrict__ total_out) {
  __shared__ int tile[SCAN_LDS];
  __shared__ int wsum[4];
  const int64_t base = (int64_t)blockIdx.x * SCAN_TILE;
#pragma unroll
  for (int j = 0; j < SCAN_PER; ++j) {
    const int l = j * 256 + threadIdx.x;
    const int64_t i = base + l;
    tile[l + l / SCAN_PER] = i < n ? in[i] : 0;
  }
  __syncthreads();
  int* mine = tile + threadIdx.x * (SCAN_PER + 1);
  int v[SCAN_PER], sum = 0;
#pragma unroll
  for (int j = 0; j < SCAN_PER; ++j) {
    v[j] = mine[j];
    sum += v[j];
  }
  int total;
  int run = block_scan_256(sum, wsum, total) + (offsets ? offsets[blockIdx.x] : 0);
#pragma unroll
  for (int j = 0; j < SCAN_PER; ++j) {
    mine[j] = run;
    run += v[j];
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < SCAN_PER; ++j) {
    const int l = j * 256 + threadIdx.x;
    const int64_t i = base + l;
    if (i < n) out[i] = tile[l + l / SCAN_PER];
  }
  if (total_out && threadIdx.x == 0) *total_out = (int64_t)total;
}

int64_t tiles_of(int64_t n) { return (n + SCAN_TILE - 1) / SCAN_TILE; }

int64_t scan_scratch(int64_t n) {
  int64_t s = 0;
  while (n > SCAN_TILE) {
    n = tiles_of(n);
    s += n;
  }
  return s;
}

void scan_launch(const int32_t* in, int32_t* out, int64_t n, int64_t* total, int32_t* scratch, hipStream_t st) {
  if (n <= SCAN_TILE) {
    KSMI_NOTE(scan_tile_kernel);
    hipLaunchKernelGGL(scan_tile_kernel, dim3(1), dim3(256), 0, st, in, out, n, (const int32_t*)nullptr, total);
    return;
  }
  const int64_t nt = tiles_of(n);              // at most 2^20
  KSMI_NOTE(tile_sums_kernel);
  hipLaunchKernelGGL(tile_sums_kernel, dim3((unsigned)nt), dim3(256), 0, st, in, n, scratch);
  scan_launch(scratch, scratch, nt, total, scratch + nt, st);
  KSMI_NOTE(scan_tile_kernel);
  hipLaunchKernelGGL(scan_tile_kernel, dim3((unsigned)nt), dim3(256), 0, st, in, out, n, (const int32_t*)scratch, (int64_t*)nullptr);
}

// ---------------------------------------------------------------------------------------------------- edges
__device__ __forceinline__ bool selected(unsigned c, uint64_t mask) { return c < 63u && ((mask >> c) & 1ull); }

// bit s: side s of pixel p = (x, y) with label m borders the outside of the scene or another label
__device__ __forceinline__ unsigned boundary_sides(const int32_t* __restrict__ lab, int Hs, int Ws, int x, int y, int p, int32_t m) {
  unsigned b = 0;
  if (y == 0 || lab[p - Ws] != m) b |= 1u;
  if (x + 1 == Ws || lab[p + 1] != m) b |= 2u;
  if (y + 1 == Hs || lab[p + Ws] != m) b |= 4u;
  if (x == 0 || lab[p - 1] != m) b |= 8u;
  return b;
}

__global__ __launch_bounds__(256) void edge_count_kernel(const unsigned char* __restrict__ cls, const int32_t* __restrict__ lab, uint64_t mask,
                                                         int Hs, int Ws, int32_t* __restrict__ counts) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)Hs * Ws) return;
  const int p = (int)i, y = p / Ws, x = p - y * Ws;
  counts[p] = selected(cls[p], mask) ? __popc(boundary_sides(lab, Hs, Ws, x, y, p, lab[p])) : 0;
}

__global__ __launch_bounds__(256) void edge_emit_kernel(const unsigned char* __restrict__ cls, const int32_t* __restrict__ lab, uint64_t mask,
                                                        int Hs, int Ws, const int32_t* __restrict__ offs, int E, int32_t* __restrict__ eid,
                                                        int32_t* __restrict__ succ) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)Hs * Ws) return;
  const int p = (int)i, y = p / Ws, x = p - y * Ws;
  if (!selected(cls[p], mask)) return;
  const int32_t m = lab[p];
  const unsigned b = boundary_sides(lab, Hs, Ws, x, y, p, m);
  int k = offs[p];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    if (!((b >> s) & 1u)) continue;
    const int fx = s == 0 ? 1 : s == 2 ? -1 : 0, fy = s == 1 ? 1 : s == 3 ? -1 : 0;      // the heading of side s
    const int rx = -fy, ry = fx;                                                        // right of it (y down): the heading of side s + 1
    const int Rx = x + fx, Ry = y + fy, Lx = Rx - rx, Ly = Ry - ry;                     // ahead-right and ahead-left of the end vertex
    int qx = x, qy = y, t = (s + 1) & 3;                                                // turn right around the own pixel
    if (Lx >= 0 && Lx < Ws && Ly >= 0 && Ly < Hs && lab[Ly * Ws + Lx] == m) {
      qx = Lx, qy = Ly, t = (s + 3) & 3;                                                // turn left onto the pixel ahead-left
    } else if (Rx >= 0 && Rx < Ws && Ry >= 0 && Ry < Hs && lab[Ry * Ws + Rx] == m) {
      qx = Rx, qy = Ry, t = s;                                                          // straight on along the pixel ahead-right
    }
    const int q = qy * Ws + qx;
    const unsigned bq = q == p ? b : boundary_sides(lab, Hs, Ws, qx, qy, q, m);
    if ((unsigned)k < (unsigned)E) {
      eid[k] = 4 * p + s;
      succ[k] = offs[q] + __popc(bq & ((1u << t) - 1u));
    }
    ++k;
  }
}

// ---------------------------------------------------------------------------------------------------- rings by pointer doubling
__device__ __forceinline__ int32_t checked_succ(const int32_t* __restrict__ succ, int k, int E) {
  const int32_t s = succ[k];
  return (unsigned)s < (unsigned)E ? s : k;                            // a value that is no edge: a ring of its own
}

__global__ __launch_bounds__(256) void trace_min_init_kernel(const int32_t* __restrict__ succ, int E, int32_t* __restrict__ nx,
                                                             int32_t* __restrict__ mn) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= E) return;
  nx[i] = checked_succ(succ, (int)i, E);
  mn[i] = (int32_t)i;
}

__global__ __launch_bounds__(256) void trace_min_round_kernel(const int32_t* __restrict__ nx, const int32_t* __restrict__ mn, int E,
                                                              int32_t* __restrict__ nx2, int32_t* __restrict__ mn2) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= E) return;
  const int32_t j = nx[i];                                             // in [0, E): the init kernel checked it
  nx2[i] = nx[j];
  mn2[i] = min(mn[i], mn[j]);
}

__global__ __launch_bounds__(256) void trace_rank_init_kernel(const int32_t* __restrict__ succ, const int32_t* __restrict__ ring_min, int E,
                                                              int32_t* __restrict__ nx, int32_t* __restrict__ d) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= E) return;
  const int32_t s = checked_succ(succ, (int)i, E);
  const bool last = s == ring_min[i];                                  // the cycle is cut before its smallest edge
  nx[i] = last ? -1 : s;
  d[i] = last ? 0 : 1;
}

__global__ __launch_bounds__(256) void trace_rank_round_kernel(const int32_t* __restrict__ nx, const int32_t* __restrict__ d, int E,
                                                               int32_t* __restrict__ nx2, int32_t* __restrict__ d2) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= E) return;
  const int32_t j = nx[i];
  nx2[i] = j < 0 ? -1 : nx[j];
  d2[i] = j < 0 ? d[i] : d[i] + d[j];
}

__global__ __launch_bounds__(256) void trace_rank_final_kernel(const int32_t* __restrict__ ring_min, const int32_t* __restrict__ d, int E,
                                                               int32_t* __restrict__ rank) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= E) return;
  const int32_t h = ring_min[i];
  rank[i] = (unsigned)h < (unsigned)E ? d[h] - d[i] : 0;
}

int rounds_of(int64_t E) {                     // ceil(log2(E)): the smallest r with 2^r >= E
  int r = 0;
  while ((1ll << r) < E) ++r;
  return r;
}

// ---------------------------------------------------------------------------------------------------- ring assembly
__global__ __launch_bounds__(256) void ring_heads_kernel(const int32_t* __restrict__ ring_min, int E, int32_t* __restrict__ flags) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= E) return;
  flags[i] = ring_min[i] == (int32_t)i ? 1 : 0;
}

// the ring number of edge k, or -1 when the arrays do not name one
__device__ __forceinline__ int ring_of_edge(const int32_t* __restrict__ ring_min, const int32_t* __restrict__ ridx, int k, int E, int R,
                                            int32_t& head) {
  head = ring_min[k];
  if ((unsigned)head >= (unsigned)E) return -1;
  const int32_t r = ridx[head];
  return (unsigned)r < (unsigned)R ? r : -1;
}

__global__ __launch_bounds__(256) void ring_table_kernel(const int32_t* __restrict__ eid, const int32_t* __restrict__ succ,
                                                         const int32_t* __restrict__ ring_min, const int32_t* __restrict__ rank,
                                                         const int32_t* __restrict__ ridx, const int32_t* __restrict__ labels, int64_t HW, int E,
                                                         int R, int32_t* __restrict__ ring_id, int32_t* __restrict__ label,
                                                         int32_t* __restrict__ len) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= E) return;
  const int k = (int)i;
  int32_t head;
  const int r = ring_of_edge(ring_min, ridx, k, E, R, head);
  if (r < 0) return;
  if (head == k) {
    const int32_t e = eid[k];
    const int64_t p = e >> 2;
    ring_id[r] = e;
    label[r] = p >= 0 && p < HW ? labels[p] : -1;
  }
  if (checked_succ(succ, k, E) == head) len[r] = rank[k] + 1;          // the one edge of the ring that closes it
}

__global__ __launch_bounds__(256) void ring_order_kernel(const int32_t* __restrict__ eid, const int32_t* __restrict__ succ,
                                                         const int32_t* __restrict__ ring_min, const int32_t* __restrict__ rank,
                                                         const int32_t* __restrict__ ridx, const int32_t* __restrict__ roff, int E, int R,
                                                         int32_t* __restrict__ oeid, int32_t* __restrict__ ring_of, int32_t* __restrict__ turn) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= E) return;
  const int k = (int)i;
  int32_t head;
  const int r = ring_of_edge(ring_min, ridx, k, E, R, head);
  if (r < 0) return;
  const int64_t pos = (int64_t)roff[r] + rank[k];
  if (pos < 0 || pos >= E) return;
  const int32_t e = eid[k];
  oeid[pos] = e;
  ring_of[pos] = r;
  turn[pos] = ((eid[checked_succ(succ, k, E)] ^ e) & 3) != 0 ? 1 : 0;
}

__global__ __launch_bounds__(256) void ring_verts_kernel(const int32_t* __restrict__ oeid, const int32_t* __restrict__ ring_of,
                                                         const int32_t* __restrict__ voff, int E, int R, int V, int Ws,
                                                         int32_t* __restrict__ verts, int32_t* __restrict__ start,
                                                         unsigned long long* __restrict__ area2) {
  __shared__ unsigned long long acc[VT_SLOTS];
  for (int s = threadIdx.x; s < VT_SLOTS; s += 256) acc[s] = 0ull;
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * VT_PER_BLOCK;             // base < E: the grid covers E
  int r0 = ring_of[base];                                              // rings are contiguous and ascending in ring order
  if ((unsigned)r0 >= (unsigned)R) r0 = 0;
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int j = 0; j < VT_PER_BLOCK / 256; ++j) {
    const int64_t pos = base + j * 256 + threadIdx.x;
    const bool live = pos < E;
    int r = -1;
    long long term = 0;
    if (live) {
      const int32_t e = oeid[pos];
      const int p = e >> 2, s = e & 3, y = p / Ws, x = p - y * Ws;
      const int x0 = x + (s == 1 || s == 2), y0 = y + (s >= 2), x1 = x + (s == 0 || s == 1), y1 = y + (s == 1 || s == 2);
      term = (long long)x0 * y1 - (long long)x1 * y0;
      const int32_t v = voff[pos], after = pos + 1 < E ? voff[pos + 1] : V;
      if (after != v && (unsigned)v < (unsigned)V) {                   // a turning edge: its end vertex is a vertex of the ring
        verts[2 * (int64_t)v] = x1;
        verts[2 * (int64_t)v + 1] = y1;
      }
      r = ring_of[pos];
      if ((unsigned)r >= (unsigned)R) r = -1;
      if (r >= 0 && (pos == 0 || ring_of[pos - 1] != r)) start[r] = v;
      if (pos == E - 1) start[R] = V;
    }
    const int r_first = __shfl(r, 0);
    if (__all(live && r == r_first)) {                                 // the whole wave on one ring: one LDS add
      if (r_first < 0) continue;                                       // wave-uniform
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) term += __shfl_down(term, o);
      if (lane == 0) {
        const int slot = r_first - r0;
        if (slot >= 0 && slot < VT_SLOTS) atomicAdd(&acc[slot], (unsigned long long)term);
        else atomicAdd(&area2[r_first], (unsigned long long)term);
      }
    } else if (r >= 0) {
      const int slot = r - r0;
      if (slot >= 0 && slot < VT_SLOTS) atomicAdd(&acc[slot], (unsigned long long)term);
      else atomicAdd(&area2[r], (unsigned long long)term);
    }
  }
  __syncthreads();
  for (int s = threadIdx.x; s < VT_SLOTS; s += 256) {
    const int64_t r = (int64_t)r0 + s;
    if (acc[s] != 0ull && r >= 0 && r < R) atomicAdd(&area2[r], acc[s]);
  }
}

// blocks of `per` items; the callers keep total <= 2^31 - 1
unsigned blocks_of(int64_t total, int per = 256) { return (unsigned)((total + per - 1) / per); }

}  // namespace

int64_t ksmi_scan_i32_scratch(int64_t n) { return n < 0 || n > MAX_N ? -1 : scan_scratch(n); }

int ksmi_scan_i32(const int32_t* in_i32, int32_t* out_i32, int64_t n, int64_t* total_i64, int32_t* scratch_i32, int64_t scratch_elems,
                  void* stream) {
  if (n < 0 || n > MAX_N) return ksmi_fail(KSMI_E_ARG, "scan_i32: 0 <= n <= 2^31 - 1 elements");
  if (n == 0) return 0;
  if (!in_i32 || !out_i32 || !total_i64) return ksmi_fail(KSMI_E_ARG, "scan_i32: null pointer");
  const int64_t need = scan_scratch(n);
  if (need > 0 && (!scratch_i32 || scratch_elems < need))
    return ksmi_fail(KSMI_E_ARG, "scan_i32: scratch smaller than ksmi_scan_i32_scratch asks for");
  scan_launch(in_i32, out_i32, n, total_i64, scratch_i32, (hipStream_t)stream);
  return ksmi_check_launch("scan_i32");
}

int ksmi_scene_edge_count(const unsigned char* classes_u8, const int32_t* labels_i32, int64_t select_mask, int Hs, int Ws, int32_t* counts_i32,
                          void* stream) {
  if (Hs < 1 || Ws < 1) return ksmi_fail(KSMI_E_ARG, "scene_edge_count: a scene of Hs >= 1 by Ws >= 1 pixels");
  const int64_t HW = (int64_t)Hs * Ws;
  if (HW > POLY_MAX_PIXELS) return ksmi_fail(KSMI_E_ARG, "scene_edge_count: more than 2^29 - 1 pixels (edge ids are int32)");
  if (select_mask < 0) return ksmi_fail(KSMI_E_ARG, "scene_edge_count: the mask selects classes 0 .. 62");
  if (!classes_u8 || !labels_i32 || !counts_i32) return ksmi_fail(KSMI_E_ARG, "scene_edge_count: null pointer");
  KSMI_NOTE(edge_count_kernel);
  hipLaunchKernelGGL(edge_count_kernel, dim3(blocks_of(HW)), dim3(256), 0, (hipStream_t)stream, classes_u8, labels_i32, (uint64_t)select_mask,
                     Hs, Ws, counts_i32);
  return ksmi_check_launch("scene_edge_count");
}

int ksmi_scene_edge_emit(const unsigned char* classes_u8, const int32_t* labels_i32, int64_t select_mask, int Hs, int Ws,
                         const int32_t* offsets_i32, int64_t E, int32_t* eid_i32, int32_t* succ_i32, void* stream) {
  if (Hs < 1 || Ws < 1) return ksmi_fail(KSMI_E_ARG, "scene_edge_emit: a scene of Hs >= 1 by Ws >= 1 pixels");
  const int64_t HW = (int64_t)Hs * Ws;
  if (HW > POLY_MAX_PIXELS) return ksmi_fail(KSMI_E_ARG, "scene_edge_emit: more than 2^29 - 1 pixels (edge ids are int32)");
  if (select_mask < 0) return ksmi_fail(KSMI_E_ARG, "scene_edge_emit: the mask selects classes 0 .. 62");
  if (E < 0 || E > 4 * HW) return ksmi_fail(KSMI_E_ARG, "scene_edge_emit: 0 <= E <= 4 * Hs * Ws edges");
  if (E == 0) return 0;
  if (!classes_u8 || !labels_i32 || !offsets_i32 || !eid_i32 || !succ_i32) return ksmi_fail(KSMI_E_ARG, "scene_edge_emit: null pointer");
  KSMI_NOTE(edge_emit_kernel);
  hipLaunchKernelGGL(edge_emit_kernel, dim3(blocks_of(HW)), dim3(256), 0, (hipStream_t)stream, classes_u8, labels_i32, (uint64_t)select_mask,
                     Hs, Ws, offsets_i32, (int)E, eid_i32, succ_i32);
  return ksmi_check_launch("scene_edge_emit");
}

int ksmi_scene_ring_trace(const int32_t* succ_i32, int64_t E, int phases, int32_t* ring_min_i32, int32_t* rank_i32, int32_t* scratch_i32,
                          int64_t scratch_elems, void* stream) {
  if (E < 0 || E > MAX_N) return ksmi_fail(KSMI_E_ARG, "scene_ring_trace: 0 <= E <= 2^31 - 1 edges");
  if (phases < 1 || phases > 3) return ksmi_fail(KSMI_E_ARG, "scene_ring_trace: phases is 1 (minima), 2 (ranks) or 3 (both)");
  if (E == 0) return 0;
  if (!succ_i32 || !ring_min_i32 || (!rank_i32 && (phases & 2)) || !scratch_i32) return ksmi_fail(KSMI_E_ARG, "scene_ring_trace: null pointer");
  if (scratch_elems < 4 * E) return ksmi_fail(KSMI_E_ARG, "scene_ring_trace: scratch smaller than 4 * E elements");
  hipStream_t st = (hipStream_t)stream;
  const int n = (int)E, rounds = rounds_of(E);
  const unsigned grid = blocks_of(E);
  int32_t* nx[2] = {scratch_i32, scratch_i32 + 2 * E};
  int32_t* val[2] = {scratch_i32 + E, scratch_i32 + 3 * E};
  // phase one: the last round (or, without a round, the init) writes the minima straight into ring_min
  if (phases & 1) {
    KSMI_NOTE(trace_min_init_kernel);
    hipLaunchKernelGGL(trace_min_init_kernel, dim3(grid), dim3(256), 0, st, succ_i32, n, nx[0], rounds ? val[0] : ring_min_i32);
    for (int r = 0; r < rounds; ++r) {
      const int a = r & 1, b = a ^ 1;
      KSMI_NOTE(trace_min_round_kernel);
      hipLaunchKernelGGL(trace_min_round_kernel, dim3(grid), dim3(256), 0, st, (const int32_t*)nx[a], (const int32_t*)val[a], n, nx[b],
                         r + 1 == rounds ? ring_min_i32 : val[b]);
    }
  }
  if (!(phases & 2)) return ksmi_check_launch("scene_ring_trace");
  KSMI_NOTE(trace_rank_init_kernel);
  hipLaunchKernelGGL(trace_rank_init_kernel, dim3(grid), dim3(256), 0, st, succ_i32, (const int32_t*)ring_min_i32, n, nx[0], val[0]);
  for (int r = 0; r < rounds; ++r) {
    const int a = r & 1, b = a ^ 1;
    KSMI_NOTE(trace_rank_round_kernel);
    hipLaunchKernelGGL(trace_rank_round_kernel, dim3(grid), dim3(256), 0, st, (const int32_t*)nx[a], (const int32_t*)val[a], n, nx[b], val[b]);
  }
  KSMI_NOTE(trace_rank_final_kernel);
  hipLaunchKernelGGL(trace_rank_final_kernel, dim3(grid), dim3(256), 0, st, (const int32_t*)ring_min_i32, (const int32_t*)val[rounds & 1], n,
                     rank_i32);
  return ksmi_check_launch("scene_ring_trace");
}

int ksmi_scene_ring_heads(const int32_t* ring_min_i32, int64_t E, int32_t* flags_i32, void* stream) {
  if (E < 0 || E > MAX_N) return ksmi_fail(KSMI_E_ARG, "scene_ring_heads: 0 <= E <= 2^31 - 1 edges");
  if (E == 0) return 0;
  if (!ring_min_i32 || !flags_i32) return ksmi_fail(KSMI_E_ARG, "scene_ring_heads: null pointer");
  KSMI_NOTE(ring_heads_kernel);
  hipLaunchKernelGGL(ring_heads_kernel, dim3(blocks_of(E)), dim3(256), 0, (hipStream_t)stream, ring_min_i32, (int)E, flags_i32);
  return ksmi_check_launch("scene_ring_heads");
}

int ksmi_scene_ring_table(const int32_t* eid_i32, const int32_t* succ_i32, const int32_t* ring_min_i32, const int32_t* rank_i32,
                          const int32_t* ring_index_i32, const int32_t* labels_i32, int64_t HW, int64_t E, int64_t R, int32_t* ring_id_i32,
                          int32_t* label_i32, int32_t* length_i32, void* stream) {
  if (E < 0 || E > MAX_N || R < 0 || R > E || HW < 0 || HW > POLY_MAX_PIXELS)
    return ksmi_fail(KSMI_E_ARG, "scene_ring_table: 0 <= R <= E <= 2^31 - 1, 0 <= HW <= 2^29 - 1");
  if (E == 0 || R == 0) return 0;
  if (!eid_i32 || !succ_i32 || !ring_min_i32 || !rank_i32 || !ring_index_i32 || !labels_i32 || !ring_id_i32 || !label_i32 || !length_i32)
    return ksmi_fail(KSMI_E_ARG, "scene_ring_table: null pointer");
  KSMI_NOTE(ring_table_kernel);
  hipLaunchKernelGGL(ring_table_kernel, dim3(blocks_of(E)), dim3(256), 0, (hipStream_t)stream, eid_i32, succ_i32, ring_min_i32, rank_i32,
                     ring_index_i32, labels_i32, HW, (int)E, (int)R, ring_id_i32, label_i32, length_i32);
  return ksmi_check_launch("scene_ring_table");
}

int ksmi_scene_ring_order(const int32_t* eid_i32, const int32_t* succ_i32, const int32_t* ring_min_i32, const int32_t* rank_i32,
                          const int32_t* ring_index_i32, const int32_t* ring_offset_i32, int64_t E, int64_t R, int32_t* ordered_eid_i32,
                          int32_t* ordered_ring_i32, int32_t* turn_i32, void* stream) {
  if (E < 0 || E > MAX_N || R < 0 || R > E) return ksmi_fail(KSMI_E_ARG, "scene_ring_order: 0 <= R <= E <= 2^31 - 1");
  if (E == 0 || R == 0) return 0;
  if (!eid_i32 || !succ_i32 || !ring_min_i32 || !rank_i32 || !ring_index_i32 || !ring_offset_i32 || !ordered_eid_i32 || !ordered_ring_i32 ||
      !turn_i32)
    return ksmi_fail(KSMI_E_ARG, "scene_ring_order: null pointer");
  KSMI_NOTE(ring_order_kernel);
  hipLaunchKernelGGL(ring_order_kernel, dim3(blocks_of(E)), dim3(256), 0, (hipStream_t)stream, eid_i32, succ_i32, ring_min_i32, rank_i32,
                     ring_index_i32, ring_offset_i32, (int)E, (int)R, ordered_eid_i32, ordered_ring_i32, turn_i32);
  return ksmi_check_launch("scene_ring_order");
}

int ksmi_scene_ring_verts(const int32_t* ordered_eid_i32, const int32_t* ordered_ring_i32, const int32_t* vertex_offset_i32, int64_t E,
                          int64_t R, int64_t V, int Ws, int32_t* verts_i32, int32_t* start_i32, int64_t* area2_i64, void* stream) {
  if (E < 0 || E > MAX_N || R < 0 || R > E || V < 0 || V > E || Ws < 1)
    return ksmi_fail(KSMI_E_ARG, "scene_ring_verts: 0 <= R <= E <= 2^31 - 1, 0 <= V <= E, Ws >= 1");
  if (E == 0 || R == 0) return 0;
  if (!ordered_eid_i32 || !ordered_ring_i32 || !vertex_offset_i32 || !start_i32 || !area2_i64 || (V > 0 && !verts_i32))
    return ksmi_fail(KSMI_E_ARG, "scene_ring_verts: null pointer");
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(area2_i64, 0, (size_t)R * sizeof(int64_t), st) != hipSuccess) return ksmi_check_launch("scene_ring_verts");
  KSMI_NOTE(ring_verts_kernel);
  hipLaunchKernelGGL(ring_verts_kernel, dim3(blocks_of(E, VT_PER_BLOCK)), dim3(256), 0, st, ordered_eid_i32, ordered_ring_i32,
                     vertex_offset_i32, (int)E, (int)R, (int)V, Ws, verts_i32, start_i32, (unsigned long long*)area2_i64);
  return ksmi_check_launch("scene_ring_verts");
}
