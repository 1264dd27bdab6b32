// The pooling kernel: Caffe's Pooling layer, MAX and AVE, any rectangular window / stride / pad, global pooling, any
// channel count, on NHWC fp32 activations as ONE launch over the lanes of a pass.  (maxpool_kernel in misc.hip keeps the
// layers it always ran: MAX, square, not global, channel count and views multiples of 4.)
//
// Reference counterpart: caffe/src/caffe/layers/pooling_layer.cpp:144-215 (Forward_cpu).  Per output (ph, pw) of a channel:
//
//     hstart = ph * stride_h - pad_h                                      (the same along w)
//     MAX    hend = min(hstart + kernel_h, H), hstart = max(hstart, 0); from -FLT_MAX, `x > m ? x : m` in (y, x) order: the
//            first maximum wins
//     AVE    hend = min(hstart + kernel_h, H + pad_h); pool_size = (hend - hstart) * (wend - wstart) BEFORE the ends are
//            clipped to the image: the padding counts in the divisor, what a ceil-sized last window has beyond H + pad does
//            not; then hstart = max(hstart, 0), hend = min(hend, H); an fp32 sum from 0 in (y, x) order; ONE division by
//            (float)pool_size -- the compiler's correctly rounded one (HIP's default), no reciprocal
//
// Built with -ffp-contract=off.  Conv mode "f64": the AVE sum and the division in binary64, in the same order, rounded once.
//
// Data path.  A pixel's channels are contiguous and the layer is bandwidth bound.  An item is a channel quad (float4) where C,
// both pixel pitches and both channel offsets are multiples of 4 (VEC), else one channel.  Input and output carry their own
// pitch and offset: a member of a zero-copy Concat works on either side.
//
// Windowed form.  Grid x over (output column, item) of one output row, grid y over the output rows of every member stacked
// ((image, row) per member): 32-bit index math, two divisions per thread (its (column, item) pair; the block-uniform
// (image, row) pair).  A thread walks its window in Caffe's order, the
// loads of kPoolBatch elements issued together in front of their operations.
//
// Global pooling: the window is the whole map, the top (B, C, 1, 1).  Maps of at most kPoolGlobalT pixels take the windowed
// form (kernel = H x W, one output row per image), so the result is the windowed one bit for bit.  Larger maps take the
// tree form: one block of 256 threads owns one (image, chunk of 4 items); thread t takes item t & 3 of the chunk and pixel
// lane t >> 2 (64 of them), walks the pixels lane, lane + 64, ... with one add chain from 0 (MAX: from -FLT_MAX), and the 64
// partial results are combined by a fixed tree: an xor-butterfly over the wave's 16 pixel lanes (masks 4, 8, 16, 32: both
// lanes of a pair add the same two values, a + b == b + a bit for bit), then through LDS across the 4 waves as
// (w0 + w1) + (w2 + w3).  The order of the additions depends on (H, W) and the form alone -- never on the grid, the member
// or the lanes of the pass.  Longest chain: ceil(H W / 64) + 6 additions.  No atomics on activations, no scratch.
//
// Every output of either method is bounded by max |input|: one thread per member raises the top's activation-exponent slot
// from the bottom's (conv_common.h; atomicMax, as amax_raise_kernel does), a null slot is skipped.  Nothing here can leave
// the fp16 range that its input did not leave: no range-flag traffic.
#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include "shf_internal.h"

namespace shf {

constexpr int kPoolThreads = 256;
constexpr int kPoolGlobalT = 16;      // pixels up to which a global layer runs the windowed form
constexpr int kPoolMaxGridRows = 65535;   // gridDim.y's limit
constexpr int kPoolBatch = 8;         // window elements whose loads the windowed form issues together
constexpr int kPoolTreeItems = 4;     // items per block of the tree form ...
constexpr int kPoolTreeLanes = 64;    // ... and pixel lanes (kPoolThreads / kPoolTreeItems)

struct PoolGM {
  const float* in;                 // first channel the view reads, of pixel 0
  float* out;
  const unsigned* in_amax;         // activation-exponent slots (null: not tracked)
  unsigned* out_amax;
  int B, H, W, Ho, Wo;
  int kh, kw;                      // the window (global pooling: H x W of this member)
  int in_pitch, out_pitch;
  int row_start;                   // first grid row (blockIdx.y) of this member
  int tree;                        // 1: the global tree form (grid rows = images, grid x = chunks)
};
struct PoolGK {
  int n_members, C;
  int sh, sw, ph, pw;
  int row_base;                    // grid row of blockIdx.y == 0 (a launch covers at most 65535 rows: larger groups take several)
  int pad_;
  PoolGM mem[16];
};
static_assert(sizeof(PoolGK) <= 4096, "kernel arguments must fit the 4 KiB by-value limit");

template <bool VEC>
__device__ __forceinline__ void pool_load(const float* p, float (&o)[VEC ? 4 : 1]) {
  if constexpr (VEC) {
    const float4 v = *(const float4*)p;
    o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
  } else {
    o[0] = *p;
  }
}

template <bool VEC>
__device__ __forceinline__ void pool_store(float* p, const float (&o)[VEC ? 4 : 1]) {
  if constexpr (VEC) *(float4*)p = make_float4(o[0], o[1], o[2], o[3]);
  else *p = o[0];
}

template <bool AVE, typename Acc>
__device__ __forceinline__ Acc pool_step(Acc a, float x) {
  if constexpr (AVE) return a + (Acc)x;
  else return x > a ? x : a;    // the first maximum wins
}

template <bool AVE, typename Acc>
__device__ __forceinline__ Acc pool_join(Acc a, Acc b) {
  if constexpr (AVE) return a + b;
  else return b > a ? b : a;
}

template <bool VEC, bool F64, bool AVE>
__global__ void __launch_bounds__(kPoolThreads) pool_kernel(PoolGK g) {
  constexpr int V = VEC ? 4 : 1;
  typedef typename std::conditional<AVE && F64, double, float>::type Acc;
  const int grow = g.row_base + (int)blockIdx.y;
  int mi = 0;
#pragma unroll
  for (int q = 1; q < 16; ++q) mi += (q < g.n_members && grow >= g.mem[q].row_start) ? 1 : 0;
  const PoolGM& p = g.mem[mi];
  const int row = grow - p.row_start;
  if (blockIdx.x == 0 && row == 0 && threadIdx.x == 0 && p.out_amax && p.in_amax) atomicMax(p.out_amax, *p.in_amax);
  const unsigned items = (unsigned)g.C / V;
  const Acc first = AVE ? (Acc)0 : (Acc)-3.402823466e+38f;

  if (p.tree) {
    // ---- global pooling of a large map: block = (image `row`, chunk blockIdx.x of 4 items)
    __shared__ Acc part[kPoolThreads / 64][kPoolTreeItems][V];
    const unsigned chunks = (items + kPoolTreeItems - 1) / kPoolTreeItems;
    const bool block_live = blockIdx.x < chunks;       // (block-uniform: the barrier below is reached by all or none)
    if (!block_live) return;
    const unsigned it = blockIdx.x * kPoolTreeItems + (threadIdx.x & (kPoolTreeItems - 1));
    const int lane = (int)(threadIdx.x >> 2);          // pixel lane 0 .. 63
    const bool live = it < items;                      // (no early return: every lane takes part in the shuffles)
    const int HW = p.H * p.W;
    const float* src = p.in + (size_t)row * (size_t)HW * p.in_pitch + it * V;
    Acc acc[V];
#pragma unroll
    for (int e = 0; e < V; ++e) acc[e] = first;
    if (live) {
      int pix = lane;
      // four loads in flight, ONE chain of additions in pixel order
      for (; pix + 3 * kPoolTreeLanes < HW; pix += 4 * kPoolTreeLanes) {
        float x[4][V];
#pragma unroll
        for (int j = 0; j < 4; ++j) pool_load<VEC>(src + (size_t)(pix + j * kPoolTreeLanes) * p.in_pitch, x[j]);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int e = 0; e < V; ++e) acc[e] = pool_step<AVE, Acc>(acc[e], x[j][e]);
      }
      for (; pix < HW; pix += kPoolTreeLanes) {
        float x[V];
        pool_load<VEC>(src + (size_t)pix * p.in_pitch, x);
#pragma unroll
        for (int e = 0; e < V; ++e) acc[e] = pool_step<AVE, Acc>(acc[e], x[e]);
      }
    }
#pragma unroll
    for (int m = kPoolTreeItems; m < 64; m <<= 1)
#pragma unroll
      for (int e = 0; e < V; ++e) acc[e] = pool_join<AVE, Acc>(acc[e], __shfl_xor(acc[e], m));
    const int wave = (int)(threadIdx.x >> 6);
    if ((threadIdx.x & 63) < kPoolTreeItems)
#pragma unroll
      for (int e = 0; e < V; ++e) part[wave][threadIdx.x & 63][e] = acc[e];
    __syncthreads();
    if (threadIdx.x < kPoolTreeItems && live) {
      float o[V];
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const Acc r = pool_join<AVE, Acc>(pool_join<AVE, Acc>(part[0][threadIdx.x][e], part[1][threadIdx.x][e]),
                                          pool_join<AVE, Acc>(part[2][threadIdx.x][e], part[3][threadIdx.x][e]));
        if constexpr (AVE) o[e] = (float)(r / (Acc)HW);
        else o[e] = (float)r;
      }
      pool_store<VEC>(p.out + (size_t)row * p.out_pitch + it * V, o);
    }
    return;
  }

  // ---- windowed form: grid row = (image, output row) of the member, x over (output column, item)
  const unsigned n = blockIdx.x * kPoolThreads + threadIdx.x;
  if (n >= (unsigned)p.Wo * items) return;
  const int it = (int)(n % items), ox = (int)(n / items);
  const int b = row / p.Ho, oy = row - b * p.Ho;
  int hs = oy * g.sh - g.ph, ws = ox * g.sw - g.pw;
  int he, we, pool_size = 1;
  if constexpr (AVE) {
    he = min(hs + p.kh, p.H + g.ph);
    we = min(ws + p.kw, p.W + g.pw);
    pool_size = (he - hs) * (we - ws);
    he = min(he, p.H);
    we = min(we, p.W);
  } else {
    he = min(hs + p.kh, p.H);
    we = min(ws + p.kw, p.W);
  }
  hs = max(hs, 0);
  ws = max(ws, 0);
  Acc acc[V];
#pragma unroll
  for (int e = 0; e < V; ++e) acc[e] = first;
  const float* src = p.in + (size_t)b * (size_t)(p.H * p.W) * p.in_pitch + it * V;
  // the window in (y, x) order, kPoolBatch elements at a time: their loads are issued together (a cursor walks the window,
  // no division), then ONE chain of operations in that order -- a 2 x 2 or 3 x 3 window is one or two round trips to memory
  // instead of four or nine
  const int nw = we - ws, count = (he > hs && nw > 0) ? (he - hs) * nw : 0;
  int y = hs, x = ws;
  for (int base = 0; base < count; base += kPoolBatch) {
    float v[kPoolBatch][V];
#pragma unroll
    for (int j = 0; j < kPoolBatch; ++j) {
#pragma unroll
      for (int e = 0; e < V; ++e) v[j][e] = 0.f;
      if (base + j < count) {
        pool_load<VEC>(src + (size_t)(y * p.W + x) * p.in_pitch, v[j]);
        if (++x == we) { x = ws; ++y; }
      }
    }
#pragma unroll
    for (int j = 0; j < kPoolBatch; ++j)
      if (base + j < count) {
#pragma unroll
        for (int e = 0; e < V; ++e) acc[e] = pool_step<AVE, Acc>(acc[e], v[j][e]);
      }
  }
  float o[V];
#pragma unroll
  for (int e = 0; e < V; ++e) {
    if constexpr (AVE) o[e] = (float)(acc[e] / (Acc)pool_size);
    else o[e] = (float)acc[e];
  }
  pool_store<VEC>(p.out + ((size_t)row * p.Wo + ox) * p.out_pitch + it * V, o);
}

// SHF_POOL_GLOBAL_T (experiments; the default is the measured choice): pixels up to which global pooling runs the
// windowed form.  Read once.
int pool_global_threshold() {
  static const int t = [] {
    const char* e = getenv("SHF_POOL_GLOBAL_T");
    return e ? std::max(0, atoi(e)) : kPoolGlobalT;
  }();
  return t;
}

int launch_pool_group(const PoolArgs* as, int n, const PoolGeom& q, int f64, hipStream_t s) {
  if (n < 1 || n > 16) { set_error("pool group: 1..16 members"); return -1; }
  if (q.method != POOL_MAX && q.method != POOL_AVE) { set_error("pool: unknown method"); return -1; }
  if (!q.global && (q.kh < 1 || q.kw < 1 || q.sh < 1 || q.sw < 1 || q.ph < 0 || q.pw < 0 || q.ph >= q.kh || q.pw >= q.kw)) {
    set_error("pool: needs kernel >= 1, stride >= 1 and 0 <= pad < kernel per axis");
    return -1;
  }
  auto aligned = [](const void* p) { return (((uintptr_t)p) & 15) == 0; };
  PoolGK g;
  g.n_members = n; g.C = as[0].in.C;
  g.row_base = 0; g.pad_ = 0;
  g.sh = q.global ? 1 : q.sh; g.sw = q.global ? 1 : q.sw;
  g.ph = q.global ? 0 : q.ph; g.pw = q.global ? 0 : q.pw;
  bool vec = g.C % 4 == 0;
  for (int m = 0; m < n; ++m) {
    const View &in = as[m].in, &out = as[m].out;
    if (!in.p || !out.p || in.B < 1 || in.H < 1 || in.W < 1 || in.C < 1 || out.H < 1 || out.W < 1) { set_error("pool: empty view"); return -1; }
    if (in.C != g.C || out.C != g.C) { set_error("pool group: members differ in the channel count"); return -1; }
    if (in.B != out.B) { set_error("pool: input and output differ in the batch size"); return -1; }
    // every element read or written lies inside its buffer's pixel
    if (in.coff < 0 || out.coff < 0 || in.coff + in.C > in.cstride || out.coff + out.C > out.cstride) {
      set_error("pool: a view exceeds its buffer's pixel");
      return -1;
    }
    // (reads are clipped to the image whatever the output size: a window that starts beyond it -- a stride larger than the
    // kernel without a pad, which Caffe sizes the same way -- is empty: -FLT_MAX, or 0 / 0 as in Caffe)
    if (q.global && (out.H != 1 || out.W != 1)) { set_error("pool: a global layer's output is 1 x 1"); return -1; }
    if ((unsigned long long)in.B * in.H * in.W >= (1ull << 31) || (unsigned long long)out.W * g.C >= (1ull << 31)) {
      set_error("pool: map too large (2^31 pixels or more)");
      return -1;
    }
    vec = vec && in.cstride % 4 == 0 && in.coff % 4 == 0 && aligned(in.p) && out.cstride % 4 == 0 && out.coff % 4 == 0 && aligned(out.p);
  }
  const unsigned items = (unsigned)(vec ? g.C / 4 : g.C);
  long long rows = 0;
  unsigned gx = 1;
  for (int m = 0; m < n; ++m) {
    const View &in = as[m].in, &out = as[m].out;
    PoolGM& gm = g.mem[m];
    gm.in = in.p + in.coff;
    gm.out = out.p + out.coff;
    gm.in_amax = as[m].in_amax;
    gm.out_amax = as[m].out_amax;
    gm.B = in.B; gm.H = in.H; gm.W = in.W; gm.Ho = out.H; gm.Wo = out.W;
    gm.kh = q.global ? in.H : q.kh;
    gm.kw = q.global ? in.W : q.kw;
    gm.in_pitch = in.cstride; gm.out_pitch = out.cstride;
    gm.row_start = (int)rows;
    gm.tree = q.global && (long long)in.H * in.W > pool_global_threshold() ? 1 : 0;
    if (gm.tree) {
      rows += in.B;
      gx = std::max(gx, (items + kPoolTreeItems - 1) / kPoolTreeItems);
    } else {
      rows += (long long)in.B * out.H;
      gx = std::max(gx, ((unsigned)out.W * items + kPoolThreads - 1) / kPoolThreads);
    }
    if (rows >= (1ll << 31)) { set_error("pool: group too large (2^31 output rows or more)"); return -1; }
  }
  for (int m = n; m < 16; ++m) g.mem[m] = g.mem[0];
  const dim3 block(kPoolThreads);
  const bool ave = q.method == POOL_AVE, d = f64 != 0 && ave;   // (MAX has no arithmetic: one form in every mode)
  // the grid's y extent is 65535: a group with more rows goes out as consecutive row ranges of the same table
  for (long long base = 0; base < rows; base += kPoolMaxGridRows) {
    g.row_base = (int)base;
    const dim3 grid(gx, (unsigned)std::min<long long>(rows - base, kPoolMaxGridRows), 1);
    if (vec) {
      if (!ave) hipLaunchKernelGGL((pool_kernel<true, false, false>), grid, block, 0, s, g);
      else if (d) hipLaunchKernelGGL((pool_kernel<true, true, true>), grid, block, 0, s, g);
      else hipLaunchKernelGGL((pool_kernel<true, false, true>), grid, block, 0, s, g);
    } else {
      if (!ave) hipLaunchKernelGGL((pool_kernel<false, false, false>), grid, block, 0, s, g);
      else if (d) hipLaunchKernelGGL((pool_kernel<false, true, true>), grid, block, 0, s, g);
      else hipLaunchKernelGGL((pool_kernel<false, false, true>), grid, block, 0, s, g);
    }
  }
  SHF_HIP_OK(hipGetLastError());
  return 0;
}

}  // namespace shf
