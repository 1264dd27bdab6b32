// Per-class detection lists of a multi-class image on the device: forward_net's flip fix and unscale (lib/test.py:52-66)
// and detect()'s per-class > thresh cut (lib/test.py:161-167) for a GROUP of finished units, as a stable compaction of the
// units' (R, C) score rows into C - 1 lists.
//
// The two-class list (tail.hip append_dets_kernel) finds a unit's survivors by bisection: its rows are sorted by the only
// foreground score, so they are a prefix.  With C > 2 the rows are sorted by the BEST foreground class
// (proposal_layer.py:180) and the survivors of one class are scattered over the unit, so each list is compacted for real:
//
//   count    one block per (unit, 256-row tile): a thread reads its row's C - 1 foreground scores once, a wave64 ballot per
//            class gives the wave's survivors, the four waves' counts meet in LDS -> tiles[class][tile]
//   scan     one block: wave w turns the tile counts of classes w, w + 4 into the tiles' first list positions (an exclusive
//            scan continued from the list's current length) and writes the new length, clamped to the capacity
//   scatter  the count grid again: the same ballots, v_mbcnt gives a survivor's rank inside its wave, the waves before it
//            come from LDS, the tile's start from the scan -> row (x1', y1', x2', y2', score) at its position
//
// Positions are prefix sums over (unit, row): the lists are in the order np.where gives on the concatenated units, and no
// atomic decides anything.  Rows at or beyond the capacity are dropped.  Plain vector stores only.
#include "class_lists.h"

namespace shf {

namespace {

constexpr int CLG = kClassListsMaxUnits;
constexpr int CL_TILE = 256;   // rows per block: four wave64

struct ClassListsGM {
  const float* boxes5;
  const float* probs;
  int R;
  float im_w, im_scale;
  int flip;
};
struct ClassListsGK {
  int n, ntiles, cap;
  float thresh;
  float* dets5;  // list c - 1 is dets5 + (c - 1) * cap * 5
  int* tiles;    // [C - 1][ntiles]: survivors per tile after count, first list position per tile after scan
  int tile_start[CLG + 1];
  ClassListsGM m[CLG];
};

__device__ __forceinline__ int find_member(const int* tile_start, int b) {
  int mi = 0;
#pragma unroll
  for (int q = 1; q < CLG; ++q) mi += (b >= tile_start[q]) ? 1 : 0;
  return mi;
}

template <int NC, bool SCATTER>
__global__ __launch_bounds__(CL_TILE) void class_lists_tile_kernel(ClassListsGK g) {
  constexpr int NF = NC - 1;
  __shared__ int wcnt[CL_TILE / 64][NF];
  const int mi = find_member(g.tile_start, blockIdx.x);
  const ClassListsGM& p = g.m[mi];
  const int r = (blockIdx.x - g.tile_start[mi]) * CL_TILE + threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool in = r < p.R;
  float pr[NF];
  unsigned long long bal[NF];
#pragma unroll
  for (int c = 0; c < NF; ++c) pr[c] = in ? p.probs[(size_t)r * NC + c + 1] : 0.f;
  // (a NaN compares false and stays out, as it does in np.where; every lane of the wave reaches the ballots)
#pragma unroll
  for (int c = 0; c < NF; ++c) bal[c] = __ballot(in && pr[c] > g.thresh);
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < NF; ++c) wcnt[wave][c] = __popcll(bal[c]);
  }
  __syncthreads();
  if (!SCATTER) {
    if (threadIdx.x < NF) {
      int s = 0;
#pragma unroll
      for (int w = 0; w < CL_TILE / 64; ++w) s += wcnt[w][threadIdx.x];
      g.tiles[(size_t)threadIdx.x * g.ntiles + blockIdx.x] = s;
    }
    return;
  }
  bool any = false;
#pragma unroll
  for (int c = 0; c < NF; ++c) any = any || (in && pr[c] > g.thresh);
  if (!any) return;
  float x1 = p.boxes5[(size_t)r * 5 + 1], y1 = p.boxes5[(size_t)r * 5 + 2], x2 = p.boxes5[(size_t)r * 5 + 3],
        y2 = p.boxes5[(size_t)r * 5 + 4];
  if (p.flip) {  // boxes[:, [1,3]] = w - boxes[:, [3,1]]
    const float nx1 = p.im_w - x2, nx2 = p.im_w - x1;
    x1 = nx1;
    x2 = nx2;
  }
  x1 = x1 / p.im_scale; y1 = y1 / p.im_scale; x2 = x2 / p.im_scale; y2 = y2 / p.im_scale;
#pragma unroll
  for (int c = 0; c < NF; ++c) {
    if (!(pr[c] > g.thresh)) continue;
    int pos = g.tiles[(size_t)c * g.ntiles + blockIdx.x];
    for (int w = 0; w < wave; ++w) pos += wcnt[w][c];
    pos += (int)__builtin_amdgcn_mbcnt_hi((unsigned)(bal[c] >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal[c], 0u));
    if (pos >= g.cap) continue;
    float* d = g.dets5 + ((size_t)c * g.cap + pos) * 5;
    d[0] = x1; d[1] = y1; d[2] = x2; d[3] = y2; d[4] = pr[c];
  }
}

// one block; wave w serves lists w, w + 4: 64 tiles per step, an inclusive shuffle scan inside the step, the running total
// carried from step to step.  len[c] is read and written by the same wave only.
__global__ __launch_bounds__(CL_TILE) void class_lists_scan_kernel(int* tiles, int ntiles, int nlists, int* len, int cap) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int c = wave; c < nlists; c += CL_TILE / 64) {
    int* t = tiles + (size_t)c * ntiles;
    int run = len[c];
    for (int b = 0; b < ntiles; b += 64) {
      const int i = b + lane;
      const int v = i < ntiles ? t[i] : 0;
      int inc = v;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
      }
      if (i < ntiles) t[i] = run + inc - v;
      run += __shfl(inc, 63, 64);
    }
    if (lane == 0) len[c] = min(run, cap);
  }
}

}  // namespace

int class_lists_tile_count(const ClassListsUnit* us, int n) {
  long long t = 0;
  for (int m = 0; m < n; ++m) t += (us[m].R + CL_TILE - 1) / CL_TILE;
  return (int)t;
}

#define SHF_CL_FOR_CLASSES(C, X) \
  switch (C) {                   \
    case 2: X(2); break;         \
    case 3: X(3); break;         \
    case 4: X(4); break;         \
    case 5: X(5); break;         \
    case 6: X(6); break;         \
    case 7: X(7); break;         \
    default: X(8); break;        \
  }

int launch_class_lists_add(const ClassListsUnit* us, int n, int C, float thresh, float* dets5, int cap, int* tiles,
                           int* len, hipStream_t s) {
  if (n < 1 || n > CLG) { set_error("class lists: 1..16 units"); return -1; }
  if (C < 2 || C > kTailMaxClasses) { set_error("class lists: 2 .. 8 classes"); return -1; }
  if (!dets5 || !tiles || !len || cap < 1) { set_error("class lists: no list buffers"); return -1; }
  ClassListsGK g;
  g.n = n; g.cap = cap; g.thresh = thresh; g.dets5 = dets5; g.tiles = tiles;
  int nt = 0;
  for (int q = 0; q <= CLG; ++q) g.tile_start[q] = 0x7fffffff;
  for (int m = 0; m < n; ++m) {
    if (us[m].R < 0 || us[m].R > kClassListsMaxRows) { set_error("class lists: a unit's row count is out of range"); return -1; }
    if (us[m].R > 0 && (!us[m].boxes5 || !us[m].probs)) { set_error("class lists: a unit without outputs"); return -1; }
    ClassListsGM& d = g.m[m];
    d.boxes5 = us[m].boxes5; d.probs = us[m].probs; d.R = us[m].R;
    d.im_w = us[m].im_w; d.im_scale = us[m].im_scale; d.flip = us[m].flip;
    g.tile_start[m] = nt;
    nt += (us[m].R + CL_TILE - 1) / CL_TILE;
  }
  for (int m = n; m < CLG; ++m) g.m[m] = ClassListsGM{nullptr, nullptr, 0, 0.f, 1.f, 0};
  g.tile_start[n] = nt;
  g.ntiles = nt;
  if (nt == 0) return 0;   // only units without score rows: the lists stay as they are
#define SHF_X(NC) hipLaunchKernelGGL((class_lists_tile_kernel<NC, false>), dim3(nt), dim3(CL_TILE), 0, s, g)
  SHF_CL_FOR_CLASSES(C, SHF_X)
#undef SHF_X
  hipLaunchKernelGGL(class_lists_scan_kernel, dim3(1), dim3(CL_TILE), 0, s, tiles, nt, C - 1, len, cap);
#define SHF_X(NC) hipLaunchKernelGGL((class_lists_tile_kernel<NC, true>), dim3(nt), dim3(CL_TILE), 0, s, g)
  SHF_CL_FOR_CLASSES(C, SHF_X)
#undef SHF_X
  SHF_HIP_OK(hipGetLastError());
  return 0;
}

}  // namespace shf
