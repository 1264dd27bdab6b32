// Detection tail for gfx950: replaces, in a handful of wave64 kernels that never leave
// the device, what the reference does with six 1x1 cuDNN convs, two concats, a 5-kernel
// softmax, a reshape, a D2H copy and the numpy ProposalLayer:
//   cls_score_d / bbox_pred_d 1x1 convs   models/test_different_dilation_template.prototxt:555-644
//   concat / softmax / reshape            :646-683, caffe/src/caffe/layers/softmax_layer.cu:85-120
//   ProposalLayer.forward (TEST phase)    lib/layers/proposal_layer.py:60-220
//   bbox_transform_inv / clip_boxes       lib/utils/bbox_transform.py:33-93
// Compiled with -ffp-contract=off: the box arithmetic keeps numpy's unfused fp32 op order.
#include <math.h>

#include <algorithm>
#include <type_traits>

#include "shf_internal.h"

namespace shf {

static inline unsigned grid_for(long long n, int block = 256) {
  long long g = (n + block - 1) / block;
  if (g > 256 * 16) g = 256 * 16;
  if (g < 1) g = 1;
  return (unsigned)g;
}

constexpr int TG = 16;  // entries per grouped launch (the units of an image's pyramid, times the net's proposal modules)
constexpr int TM = kTailMaxModules;  // proposal modules per launch: an entry's geometry is its module's, looked up by index
// The entry and module tables below go to the kernels by value.  HIP documents 4 KiB as the most a kernel's arguments may
// take; hipcc for gfx950 does not enforce it (a kernel with a 4 100-byte argument compiles), so the budget is asserted here
constexpr size_t kKernargLimit = 4096;

// which member does block `b` belong to?  blk_start[q] = first block of member q (unused entries INT_MAX)
__device__ __forceinline__ int tail_find_member(const int* blk_start, int b) {
  int mi = 0;
#pragma unroll
  for (int q = 1; q < TG; ++q) mi += (b >= blk_start[q]) ? 1 : 0;
  return mi;
}

// np.seterr(over='raise') around exp(dw) * widths (bbox_transform.py:9,52-56): does this delta overflow fp32?
__device__ __forceinline__ bool delta_overflows(float v, float anchor_extent) {
  if (!isfinite(v)) return false;
  const float e = expf(v);
  const float pw = e * anchor_extent;
  return isinf(e) || isinf(pw);
}

// ---- every kernel of the tail takes a GROUP of independent units (the 10 (level, flip) units of an image): one
//      launch per stage instead of one per unit and stage (~100 five-microsecond launches per image) --------------
struct TailResetK {
  int* counters[TG];
  unsigned* amax[TG];   // activation-exponent slots of the member lanes (null: none): consumed by this pass's convolutions,
  int n_amax[TG];       // zeroed here for the next pass
  int n;
};
__global__ void tail_reset_kernel(TailResetK p) {
  const int m = threadIdx.x >> 3, j = threadIdx.x & 7;
  if (m < p.n) {
    p.counters[m][j] = 0;
    if (p.amax[m])
      for (int i = j; i < p.n_amax[m]; i += 8) p.amax[m][i] = 0u;
  }
}

struct TailGM {  // per entry: one unit's feature maps for one module
  const float* feat[8];
  int fstride[8];
  float* logits;    // [K][A][C + 4]
  int* counters;    // [1] = overflow flag
  int K, w;
  int mod;          // index into TailGK::mod
};
struct TailLM {  // per module: the predictors and the anchor extents
  const float* Wt;  // [A][C + 4][Cf]  rows: cls0 .. cls(C-1), dx, dy, dw, dh
  const float* bt;  // [A][C + 4]
  int A, Cf;
  float aw[8], ah[8];  // base anchor widths / heights (x2-x1+1)
};
struct TailGK {
  int blk_start[TG + 1];
  TailLM mod[TM];
  TailGM m[TG];
};
static_assert(sizeof(TailGK) <= kKernargLimit, "the logits kernel's entry and module tables must fit the kernarg segment");

// ---- 1x1 cls/reg convs: wave handles two pixels, 32 lanes x float4 per pixel -------------
// F64 (conv mode "f64"): the products and the sum in binary64 (a product of two fp32 values is exact there), the bias added
// in binary64, ONE rounding to fp32
// NC: the class count (2 .. 8); a record is NC class scores and four box deltas, NC + 4 floats at 4-byte alignment
template <bool F64, int NC>
__global__ __launch_bounds__(256) void tail_logits_kernel(TailGK g) {
  constexpr int NO = NC + 4;
  typedef typename std::conditional<F64, double, float>::type acc_t;
  const int mi = tail_find_member(g.blk_start, blockIdx.x);
  const TailGM& p = g.m[mi];
  const TailLM& md = g.mod[p.mod];
  const int lb = blockIdx.x - g.blk_start[mi], lgrid = g.blk_start[mi + 1] - g.blk_start[mi];
  const int lane = threadIdx.x & 63;
  const int sub = lane >> 5, q = lane & 31;
  const long long wave = ((long long)lb * blockDim.x + threadIdx.x) >> 6;
  const long long nwaves = ((long long)lgrid * blockDim.x) >> 6;
  const long long npairs = ((long long)p.K + 1) / 2;
  for (int a = 0; a < md.A; ++a) {
    const float* f = p.feat[a];
    const int fs = p.fstride[a];
    for (long long pr = wave; pr < npairs; pr += nwaves) {
      const long long k = pr * 2 + sub;
      acc_t part[NO] = {};
      if (k < p.K) {
        for (int c0 = 0; c0 < md.Cf; c0 += 128) {
          const float4 x = *(const float4*)(f + (size_t)k * fs + c0 + q * 4);
#pragma unroll
          for (int o = 0; o < NO; ++o) {
            const float4 wv = *(const float4*)(md.Wt + ((size_t)a * NO + o) * md.Cf + c0 + q * 4);
            if constexpr (F64)
              part[o] += (double)x.x * (double)wv.x + (double)x.y * (double)wv.y + (double)x.z * (double)wv.z + (double)x.w * (double)wv.w;
            else
              part[o] += x.x * wv.x + x.y * wv.y + x.z * wv.z + x.w * wv.w;
          }
        }
      }
      // the xor butterfly 16, 8, 4, 2, 1 over the 32 lanes of a pixel -- only the first step through the LDS crossbar: after
      // step m the lanes i and i ^ m hold the same bits (a + b == b + a), so the partner of step 8 / 4 may as well be the
      // lane 8 / 4 places round the 16-lane row (DPP row_ror), and steps 2 / 1 are quad permutes: the same tree, the same bits
#pragma unroll
      for (int o = 0; o < NO; ++o) {
        if constexpr (F64) {
          double v = part[o];
#pragma unroll
          for (int m = 16; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
          part[o] = v;
        } else {
        float v = part[o];
        v += __shfl_xor(v, 16, 64);
        v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x128, 0xf, 0xf, false));   // row_ror:8
        v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x124, 0xf, 0xf, false));   // row_ror:4
        v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xf, 0xf, false));    // quad_perm [2,3,0,1]
        v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xf, 0xf, false));    // quad_perm [1,0,3,2]
        part[o] = v;
        }
      }
      if (q == 0 && k < p.K) {
        float* L = p.logits + ((size_t)k * md.A + a) * NO;
        bool of = false;
#pragma unroll
        for (int o = 0; o < NO; ++o) {
          const float v = (float)(part[o] + (acc_t)md.bt[a * NO + o]);
          L[o] = v;
          if (o >= NC + 2) of |= delta_overflows(v, o == NC + 2 ? md.aw[a] : md.ah[a]);
        }
        if (of) atomicOr(&p.counters[1], 1);
      }
    }
  }
}

// diagnostics: (1,C*A,h,w) probabilities (channel c*A + a) + (1,4A,h,w) deltas in the blobs' NCHW layout -> the tail's
// [K][A][C + 4] records, raising the same overflow flag the logits kernel raises
__global__ void tail_inject_kernel(const float* __restrict__ scores, const float* __restrict__ deltas,
                                   float* __restrict__ logits, int K, int A, int NC, TailLM g, int* counters) {
  const long long total = (long long)K * A;
  for (long long n = (long long)blockIdx.x * blockDim.x + threadIdx.x; n < total;
       n += (long long)gridDim.x * blockDim.x) {
    const int a = (int)(n % A);
    const long long k = n / A;
    float* L = logits + n * (NC + 4);
    for (int c = 0; c < NC; ++c) L[c] = scores[(size_t)(c * A + a) * K + k];
    bool of = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float v = deltas[(size_t)(a * 4 + j) * K + k];
      L[NC + j] = v;
      if (j >= 2) of |= delta_overflows(v, j == 2 ? g.aw[a] : g.ah[a]);
    }
    if (of) atomicOr(&counters[1], 1);
  }
}

struct DecodeGM {  // per member
  const float* logits;  // [K][A][C + 4]
  float* rec;           // [K*A][C + 4] the C class probabilities, x1, y1, x2, y2
  unsigned long long* keys;
  int* counters;        // 0: n candidates, 1: overflow flag ; [4..5] as u64: best key
  int K, w;
  float im_h, im_w, min_size_scaled;
  float* cls_nchw;   // optional (1,C*A,h,w), channel c*A + a
  float* bbox_nchw;  // optional (1,4A,h,w)
  int mod;           // index into DecodeGK::mod
};
struct DecodeLM {  // per module: the anchor set and the strides
  int A;
  float anchors[32];
  int sub_stride[8];
  int feat_stride;
};
struct DecodeGK {
  DecodeLM mod[TM];
  float score_thresh;
  int probs_given;   // diagnostics (shf_debug_proposal): L[0..C-1] already hold the class probabilities
  int blk_start[TG + 1];
  DecodeGM m[TG];
};
static_assert(sizeof(DecodeGK) <= kKernargLimit, "the decode kernel's entry and module tables must fit the kernarg segment");

template <int NC>
__global__ __launch_bounds__(256) void tail_decode_kernel(DecodeGK g) {
  constexpr int NO = NC + 4;
  const int mi = tail_find_member(g.blk_start, blockIdx.x);
  const DecodeGM& p = g.m[mi];
  const DecodeLM& md = g.mod[p.mod];
  const int lb = blockIdx.x - g.blk_start[mi], lgrid = g.blk_start[mi + 1] - g.blk_start[mi];
  const long long total = (long long)p.K * md.A;
  const bool clamp = p.counters[1] != 0;
  const int lane = threadIdx.x & 63;
  const long long step = (long long)lgrid * blockDim.x;
  unsigned long long best = 0;
  // every lane runs the same number of iterations so the ballots below are wave-complete
  const long long iters = (total + step - 1) / step;
  long long n = (long long)lb * blockDim.x + threadIdx.x;
  for (long long it = 0; it < iters; ++it, n += step) {
    bool cand = false;
    unsigned long long key = 0;
    if (n < total) {
      const int a = (int)(n % md.A);
      const int k = (int)(n / md.A);
      const int y = k / p.w, x = k - y * p.w;
      const float* L = p.logits + n * NO;
      // SoftmaxLayer::Forward: max, subtract, exp, sum (from class 0 upward), divide (softmax_layer.cpp:27-60)
      float lg[NC], e[NC], pr[NC];
#pragma unroll
      for (int c = 0; c < NC; ++c) lg[c] = L[c];
      float m = lg[0];
#pragma unroll
      for (int c = 1; c < NC; ++c) m = fmaxf(m, lg[c]);
#pragma unroll
      for (int c = 0; c < NC; ++c) e[c] = expf(lg[c] - m);
      float sum = e[0];
#pragma unroll
      for (int c = 1; c < NC; ++c) sum += e[c];
#pragma unroll
      for (int c = 0; c < NC; ++c) pr[c] = g.probs_given ? lg[c] : e[c] / sum;
      // the layer ranks, cuts and picks its fallback row by the best foreground class (proposal_layer.py:180-188)
      float fg = pr[1];
#pragma unroll
      for (int c = 2; c < NC; ++c) fg = fmaxf(fg, pr[c]);
      float dx = L[NC], dy = L[NC + 1], dw = L[NC + 2], dh = L[NC + 3];
      if (p.cls_nchw) {
#pragma unroll
        for (int c = 0; c < NC; ++c) p.cls_nchw[(size_t)(c * md.A + a) * p.K + k] = pr[c];
      }
      if (p.bbox_nchw) {
        p.bbox_nchw[(size_t)(a * 4 + 0) * p.K + k] = dx;
        p.bbox_nchw[(size_t)(a * 4 + 1) * p.K + k] = dy;
        p.bbox_nchw[(size_t)(a * 4 + 2) * p.K + k] = dw;
        p.bbox_nchw[(size_t)(a * 4 + 3) * p.K + k] = dh;
      }
      if (clamp) {  // bbox_transform.py:57-63
        if (dw > 50.f) dw = 5.f;
        if (dh > 50.f) dh = 5.f;
      }
      const float sx = (float)(x * md.feat_stride), sy = (float)(y * md.feat_stride);
      const float ax1 = md.anchors[a * 4 + 0] + sx, ay1 = md.anchors[a * 4 + 1] + sy;
      const float ax2 = md.anchors[a * 4 + 2] + sx, ay2 = md.anchors[a * 4 + 3] + sy;
      // bbox_transform_inv (bbox_transform.py:39-75), fp32, unfused
      const float widths = ax2 - ax1 + 1.0f, heights = ay2 - ay1 + 1.0f;
      const float ctr_x = ax1 + 0.5f * widths, ctr_y = ay1 + 0.5f * heights;
      const float pcx = dx * widths + ctr_x, pcy = dy * heights + ctr_y;
      const float pw = expf(dw) * widths, ph = expf(dh) * heights;
      float x1 = pcx - 0.5f * pw, y1 = pcy - 0.5f * ph;
      float x2 = pcx + 0.5f * pw, y2 = pcy + 0.5f * ph;
      // clip_boxes (bbox_transform.py:80-93)
      const float mw = p.im_w - 1.f, mh = p.im_h - 1.f;
      x1 = fmaxf(fminf(x1, mw), 0.f);
      y1 = fmaxf(fminf(y1, mh), 0.f);
      x2 = fmaxf(fminf(x2, mw), 0.f);
      y2 = fmaxf(fminf(y2, mh), 0.f);
      float* r = p.rec + n * NO;
#pragma unroll
      for (int c = 0; c < NC; ++c) r[c] = pr[c];
      r[NC] = x1; r[NC + 1] = y1; r[NC + 2] = x2; r[NC + 3] = y2;
      // anchor subsampling map + _filter_boxes (proposal_layer.py:160-175,231-236)
      const int ss = md.sub_stride[a];
      bool valid = (y % ss == 0) && (x % ss == 0);
      const float ws = x2 - x1 + 1.f, hs = y2 - y1 + 1.f;
      valid = valid && (ws >= p.min_size_scaled) && (hs >= p.min_size_scaled);
      if (valid) {
        key = score_key(fg, (unsigned)n);
        best = key > best ? key : best;
        cand = fg >= g.score_thresh;
      }
    }
    // wave-aggregated append of candidate keys
    const unsigned long long bal = __ballot(cand);
    if (bal) {
      int base = 0;
      const int leader = __ffsll((long long)bal) - 1;
      if (lane == leader) base = atomicAdd(&p.counters[0], __popcll(bal));
      base = __shfl(base, leader, 64);
      if (cand) p.keys[base + __popcll(bal & ((1ull << lane) - 1ull))] = key;
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const unsigned long long o = __shfl_xor(best, m, 64);
    best = o > best ? o : best;
  }
  if (lane == 0 && best) atomicMax((unsigned long long*)(p.counters + 4), best);
}

// after the sort: R = min(C, topN), or the single best valid anchor when nothing reaches the
// threshold (proposal_layer.py:182-188)
__device__ __forceinline__ int tail_rows(const int* counters, int topN, unsigned long long* best_out) {
  const int C = counters[0];
  const unsigned long long best = *(const unsigned long long*)(counters + 4);
  if (best_out) *best_out = best;
  if (C > 0) return (topN > 0 && C > topN) ? topN : C;
  return best ? 1 : 0;
}

struct GatherGM {
  const unsigned long long* keys;
  const float* rec;
  int* counters;
  float* boxes5;
  float* probs;   // (R, C) score rows
};
struct GatherGK {
  int topN;
  int blk_start[TG + 1];
  GatherGM m[TG];
};
// finalize + gather in one: every block derives R from the counters (block 0 of the member publishes it in
// counters[2] for the host / the append stage)
template <int NC>
__global__ void tail_gather_kernel(GatherGK g) {
  constexpr int NO = NC + 4;
  const int mi = tail_find_member(g.blk_start, blockIdx.x);
  const GatherGM& p = g.m[mi];
  const int lb = blockIdx.x - g.blk_start[mi], lgrid = g.blk_start[mi + 1] - g.blk_start[mi];
  unsigned long long best;
  const int R = tail_rows(p.counters, g.topN, &best);
  const bool only_best = p.counters[0] <= 0;  // nothing reached the threshold: the row is the best valid anchor
  if (lb == 0 && threadIdx.x == 0) {
    p.counters[2] = R;
    if (R == 0) {  // dummy roi, proposal_layer.py:207-208
      p.boxes5[0] = 0.f; p.boxes5[1] = 0.f; p.boxes5[2] = 0.f; p.boxes5[3] = 16.f; p.boxes5[4] = 16.f;
    }
  }
  for (int r = lb * blockDim.x + threadIdx.x; r < R; r += lgrid * blockDim.x) {
    const unsigned long long key = only_best ? best : p.keys[r];
    const unsigned n = 0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull);
    const float* q = p.rec + (size_t)n * NO;
    p.boxes5[r * 5 + 0] = 0.f;
    p.boxes5[r * 5 + 1] = q[NC];
    p.boxes5[r * 5 + 2] = q[NC + 1];
    p.boxes5[r * 5 + 3] = q[NC + 2];
    p.boxes5[r * 5 + 4] = q[NC + 3];
#pragma unroll
    for (int c = 0; c < NC; ++c) p.probs[r * NC + c] = q[c];
  }
}

// ---------------------------------------------------------------------------
// bitonic sort, descending, u64 keys, element count on the device; a GROUP of independent arrays per launch.
// Chunks of 16384 keys are sorted / merged inside one CU's LDS (128 KiB of the 160).
// ---------------------------------------------------------------------------
constexpr int SORT_CH = 16384;

__device__ __forceinline__ unsigned next_pow2(unsigned v) {
  unsigned p = 1;
  while (p < v) p <<= 1;
  return p;
}

struct SortGK {
  unsigned long long* keys[TG];
  const int* n_dev[TG];
  int blk_start[TG + 1];  // in chunks (local kernels) or in 256-thread blocks (global step)
};

// all (k,j) stages with k <= chunk: full sort of each chunk in its network direction
__global__ __launch_bounds__(1024) void bitonic_local_sort_kernel(SortGK g) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long sk[];
  const int mi = tail_find_member(g.blk_start, blockIdx.x);
  unsigned long long* keys = g.keys[mi];
  const unsigned n = (unsigned)max(*g.n_dev[mi], 0);
  const unsigned npad = next_pow2(n < 1 ? 1 : n);
  const unsigned m = npad < (unsigned)SORT_CH ? npad : (unsigned)SORT_CH;
  const unsigned start = (unsigned)(blockIdx.x - g.blk_start[mi]) * (unsigned)SORT_CH;
  if (start >= npad) return;
  for (unsigned t = threadIdx.x; t < m; t += 1024) sk[t] = (start + t < n) ? keys[start + t] : 0ull;
  __syncthreads();
  for (unsigned k = 2; k <= m; k <<= 1) {
    for (unsigned j = k >> 1; j > 0; j >>= 1) {
      for (unsigned t = threadIdx.x; t < (m >> 1); t += 1024) {
        const unsigned i = ((t / j) * 2 * j) + (t % j);
        const unsigned l = i + j;
        const bool desc = (((start + i) & k) == 0);  // overall descending order
        const unsigned long long a = sk[i], b = sk[l];
        if ((a < b) == desc) { sk[i] = b; sk[l] = a; }
      }
      __syncthreads();
    }
  }
  for (unsigned t = threadIdx.x; t < m; t += 1024) keys[start + t] = sk[t];
}

// one global compare-exchange stage (k, j) with j >= chunk
__global__ void bitonic_global_step_kernel(SortGK g, unsigned k, unsigned j) {
  const int mi = tail_find_member(g.blk_start, blockIdx.x);
  unsigned long long* keys = g.keys[mi];
  const unsigned n = (unsigned)max(*g.n_dev[mi], 0);
  const unsigned npad = next_pow2(n < 1 ? 1 : n);
  if (k > npad) return;
  const unsigned lb = blockIdx.x - g.blk_start[mi], lgrid = g.blk_start[mi + 1] - g.blk_start[mi];
  for (unsigned t = lb * blockDim.x + threadIdx.x; t < (npad >> 1); t += lgrid * blockDim.x) {
    const unsigned i = ((t / j) * 2 * j) + (t % j);
    const unsigned l = i + j;
    const bool desc = ((i & k) == 0);
    const unsigned long long a = keys[i], b = keys[l];
    if ((a < b) == desc) { keys[i] = b; keys[l] = a; }
  }
}

// remaining stages j = chunk/2 .. 1 of merge level k (> chunk), inside LDS
__global__ __launch_bounds__(1024) void bitonic_local_merge_kernel(SortGK g, unsigned k) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long sk[];
  const int mi = tail_find_member(g.blk_start, blockIdx.x);
  unsigned long long* keys = g.keys[mi];
  const unsigned n = (unsigned)max(*g.n_dev[mi], 0);
  const unsigned npad = next_pow2(n < 1 ? 1 : n);
  if (k > npad) return;
  const unsigned start = (unsigned)(blockIdx.x - g.blk_start[mi]) * (unsigned)SORT_CH;
  if (start >= npad) return;
  for (unsigned t = threadIdx.x; t < (unsigned)SORT_CH; t += 1024) sk[t] = keys[start + t];
  __syncthreads();
  const bool desc = ((start & k) == 0);
  for (unsigned j = SORT_CH >> 1; j > 0; j >>= 1) {
    for (unsigned t = threadIdx.x; t < (unsigned)(SORT_CH >> 1); t += 1024) {
      const unsigned i = ((t / j) * 2 * j) + (t % j);
      const unsigned l = i + j;
      const unsigned long long a = sk[i], b = sk[l];
      if ((a < b) == desc) { sk[i] = b; sk[l] = a; }
    }
    __syncthreads();
  }
  for (unsigned t = threadIdx.x; t < (unsigned)SORT_CH; t += 1024) keys[start + t] = sk[t];
}

static bool g_sort_attr_done = false;

// keys[m] beyond n inside [n, npad) are treated as 0 by the local sort; for npad > chunk the caller's
// buffers must hold npad entries (the tail workspace / merge context allocate pow2 capacity).
int launch_sort_desc_u64_group(unsigned long long* const* keys, const int* const* n_dev, const size_t* n_max, int n,
                               hipStream_t s) {
  if (n < 1 || n > TG) { set_error("sort group: 1..16 arrays"); return -1; }
  if (!g_sort_attr_done) {
    SHF_HIP_OK(hipFuncSetAttribute((const void*)bitonic_local_sort_kernel,
                                   hipFuncAttributeMaxDynamicSharedMemorySize, SORT_CH * 8));
    SHF_HIP_OK(hipFuncSetAttribute((const void*)bitonic_local_merge_kernel,
                                   hipFuncAttributeMaxDynamicSharedMemorySize, SORT_CH * 8));
    g_sort_attr_done = true;
  }
  SortGK loc, glo;
  size_t npad_max = 1;
  int nchunks = 0, gblocks = 0;
  for (int q = 0; q <= TG; ++q) loc.blk_start[q] = glo.blk_start[q] = 0x7fffffff;
  for (int m = 0; m < n; ++m) {
    size_t npad = 1;
    while (npad < n_max[m]) npad <<= 1;
    npad_max = std::max(npad_max, npad);
    loc.keys[m] = glo.keys[m] = keys[m];
    loc.n_dev[m] = glo.n_dev[m] = n_dev[m];
    loc.blk_start[m] = nchunks;
    glo.blk_start[m] = gblocks;
    nchunks += (int)((npad + SORT_CH - 1) / SORT_CH);
    gblocks += (int)grid_for((long long)(npad >> 1));
  }
  loc.blk_start[n] = nchunks;
  glo.blk_start[n] = gblocks;
  hipLaunchKernelGGL(bitonic_local_sort_kernel, dim3(nchunks), dim3(1024), SORT_CH * 8, s, loc);
  for (size_t k = (size_t)SORT_CH * 2; k <= npad_max; k <<= 1) {
    for (size_t j = k >> 1; j >= (size_t)SORT_CH; j >>= 1)
      hipLaunchKernelGGL(bitonic_global_step_kernel, dim3(gblocks), dim3(256), 0, s, glo, (unsigned)k, (unsigned)j);
    hipLaunchKernelGGL(bitonic_local_merge_kernel, dim3(nchunks), dim3(1024), SORT_CH * 8, s, loc, (unsigned)k);
  }
  SHF_HIP_OK(hipGetLastError());
  return 0;
}

int launch_sort_desc_u64(unsigned long long* keys, const int* n_dev, size_t n_max, hipStream_t s) {
  return launch_sort_desc_u64_group(&keys, &n_dev, &n_max, 1, s);
}

// ---------------------------------------------------------------------------
static void fill_logits_shared(const TailArgs& a, TailLM& lk) {
  lk.Wt = a.wcls[0];  // combined [A][C + 4][Cf] matrix prepared by the net (see net_graph.cpp: build_tail_weights)
  lk.bt = a.bcls[0];
  lk.A = a.A; lk.Cf = a.Cf;
  for (int i = 0; i < a.A; ++i) {
    lk.aw[i] = a.anchors[i * 4 + 2] - a.anchors[i * 4 + 0] + 1.0f;
    lk.ah[i] = a.anchors[i * 4 + 3] - a.anchors[i * 4 + 1] + 1.0f;
  }
}

// A group of units through the proposal stage.  phase 0: everything; 1: reset + logits (the kernels that read the
// head feature maps: `after_logits` is recorded behind them); 2: decode -> sort -> gather.
// the kernels are instantiated on the class count: the two-class records and arithmetic are what they were before the class
// axis existed
#define SHF_TAIL_FOR_CLASSES(C, X) \
  switch (C) {                     \
    case 2: X(2); break;           \
    case 3: X(3); break;           \
    case 4: X(4); break;           \
    case 5: X(5); break;           \
    case 6: X(6); break;           \
    case 7: X(7); break;           \
    default: X(8); break;          \
  }

int launch_tail_group(const TailArgs* as, TailWork* const* wss, float* const* out_boxes5, float* const* out_probs,
                      int n, hipStream_t s, hipEvent_t after_logits, int phase) {
  if (n < 1 || n > TG) { set_error("tail group: 1..16 units"); return -1; }
  const TailArgs& a0 = as[0];
  if (a0.C < 2 || a0.C > kTailMaxClasses) { set_error("tail: 2 .. 8 classes"); return -1; }
  // first[j]: the first entry of module j -- the launch takes the module's geometry and weights from it, and the module's
  // other entries must agree with it
  const TailArgs* first[TM] = {nullptr};
  for (int m = 0; m < n; ++m) {
    const TailArgs& a = as[m];
    if (a.module < 0 || a.module >= TM) { set_error("tail group: module index outside 0 .. 3"); return -1; }
    if (a.A < 1 || a.A > 8) { set_error("tail: at most 8 anchors per cell"); return -1; }
    const long long total = (long long)a.h * a.w * a.A;
    if ((size_t)total > wss[m]->cap_anchors) { set_error("tail: workspace too small"); return -1; }
    if (a.Cf % 128) { set_error("tail: head feature width must be a multiple of 128"); return -1; }
    if (!first[a.module]) first[a.module] = &a;
    const TailArgs& f = *first[a.module];
    if (a.A != f.A || a.C != a0.C || a.Cf != f.Cf || a.wcls[0] != f.wcls[0] || a.f64 != a0.f64) {
      set_error("tail group: members must share the proposal layer");
      return -1;
    }
  }
  if (phase != 2) {
    TailResetK rk;
    rk.n = n;
    for (int m = 0; m < n; ++m) {
      rk.counters[m] = wss[m]->counters;
      rk.amax[m] = wss[m]->amax;
      rk.n_amax[m] = wss[m]->n_amax;
    }
    hipLaunchKernelGGL(tail_reset_kernel, dim3(1), dim3(TG * 8), 0, s, rk);
    TailGK lk = {};
    for (int j = 0; j < TM; ++j)
      if (first[j]) fill_logits_shared(*first[j], lk.mod[j]);
    int blocks = 0;
    for (int q = 0; q <= TG; ++q) lk.blk_start[q] = 0x7fffffff;
    for (int m = 0; m < n; ++m) {
      const TailArgs& a = as[m];
      TailGM& g = lk.m[m];
      for (int i = 0; i < a.A; ++i) {
        const View& f = a.feat[a.heads == 1 ? 0 : i];
        g.feat[i] = f.p + f.coff;
        g.fstride[i] = f.cstride;
      }
      g.logits = wss[m]->logits;
      g.counters = wss[m]->counters;
      g.K = a.h * a.w;
      g.w = a.w;
      g.mod = a.module;
      lk.blk_start[m] = blocks;
      blocks += (int)grid_for(((long long)g.K + 1) / 2 * 64);
    }
    lk.blk_start[n] = blocks;
#define SHF_X(NC)                                                                           \
  if (a0.f64)                                                                               \
    hipLaunchKernelGGL((tail_logits_kernel<true, NC>), dim3(blocks), dim3(256), 0, s, lk);  \
  else                                                                                      \
    hipLaunchKernelGGL((tail_logits_kernel<false, NC>), dim3(blocks), dim3(256), 0, s, lk)
    SHF_TAIL_FOR_CLASSES(a0.C, SHF_X)
#undef SHF_X
    // from here on the tails only touch their own workspaces: the head feature maps may be overwritten
    if (after_logits) SHF_HIP_OK(hipEventRecord(after_logits, s));
  }
  if (phase == 1) {
    SHF_HIP_OK(hipGetLastError());
    return 0;
  }
  DecodeGK dk = {};
  for (int j = 0; j < TM; ++j) {
    if (!first[j]) continue;
    const TailArgs& f = *first[j];
    DecodeLM& md = dk.mod[j];
    md.A = f.A;
    for (int i = 0; i < f.A * 4; ++i) md.anchors[i] = f.anchors[i];
    for (int i = 0; i < f.A; ++i) md.sub_stride[i] = f.sub_stride[i] < 1 ? 1 : f.sub_stride[i];
    md.feat_stride = f.feat_stride;
  }
  dk.score_thresh = a0.score_thresh;
  dk.probs_given = a0.probs_given;
  GatherGK gk;
  gk.topN = a0.pre_nms_topN;
  unsigned long long* keys[TG];
  const int* n_dev[TG];
  size_t n_max[TG];
  int dblocks = 0, gblocks = 0;
  for (int q = 0; q <= TG; ++q) dk.blk_start[q] = gk.blk_start[q] = 0x7fffffff;
  for (int m = 0; m < n; ++m) {
    const TailArgs& a = as[m];
    const long long total = (long long)a.h * a.w * a.A;
    DecodeGM& d = dk.m[m];
    d.logits = wss[m]->logits; d.rec = wss[m]->rec; d.keys = wss[m]->keys; d.counters = wss[m]->counters;
    d.K = a.h * a.w; d.w = a.w;
    d.im_h = a.im_h; d.im_w = a.im_w;
    d.min_size_scaled = a.min_size * a.im_scale;
    d.cls_nchw = a.cls_prob_reshape_nchw;
    d.bbox_nchw = a.bbox_pred_nchw;
    d.mod = a.module;
    dk.blk_start[m] = dblocks;
    dblocks += (int)grid_for(total);
    GatherGM& q = gk.m[m];
    q.keys = wss[m]->keys; q.rec = wss[m]->rec; q.counters = wss[m]->counters;
    q.boxes5 = out_boxes5[m]; q.probs = out_probs[m];
    const long long rmax = (a.pre_nms_topN > 0 && a.pre_nms_topN < total) ? a.pre_nms_topN : total;
    gk.blk_start[m] = gblocks;
    gblocks += (int)grid_for(rmax);
    keys[m] = wss[m]->keys;
    n_dev[m] = wss[m]->counters;
    n_max[m] = (size_t)total;
  }
  dk.blk_start[n] = dblocks;
  gk.blk_start[n] = gblocks;
#define SHF_X(NC) hipLaunchKernelGGL(tail_decode_kernel<NC>, dim3(dblocks), dim3(256), 0, s, dk)
  SHF_TAIL_FOR_CLASSES(a0.C, SHF_X)
#undef SHF_X
  if (launch_sort_desc_u64_group(keys, n_dev, n_max, n, s)) return -1;
#define SHF_X(NC) hipLaunchKernelGGL(tail_gather_kernel<NC>, dim3(gblocks), dim3(256), 0, s, gk)
  SHF_TAIL_FOR_CLASSES(a0.C, SHF_X)
#undef SHF_X
  SHF_HIP_OK(hipGetLastError());
  return 0;
}

int launch_tail(const TailArgs& a, TailWork& ws, float* out_boxes5, float* out_probs, hipStream_t s,
                hipEvent_t after_logits, int phase) {
  TailWork* w = &ws;
  return launch_tail_group(&a, &w, &out_boxes5, &out_probs, 1, s, after_logits, phase);
}

int launch_tail_inject(const TailArgs& a, TailWork& ws, const float* scores_nchw, const float* deltas_nchw,
                       hipStream_t s) {
  const int K = a.h * a.w;
  const long long total = (long long)K * a.A;
  if ((size_t)total > ws.cap_anchors) { set_error("tail: workspace too small"); return -1; }
  if (a.C < 2 || a.C > kTailMaxClasses) { set_error("tail: 2 .. 8 classes"); return -1; }
  SHF_HIP_OK(hipMemsetAsync(ws.counters, 0, 8 * sizeof(int), s));
  TailLM lk = {};
  fill_logits_shared(a, lk);
  hipLaunchKernelGGL(tail_inject_kernel, dim3(grid_for(total)), dim3(256), 0, s, scores_nchw, deltas_nchw, ws.logits,
                     K, a.A, a.C, lk, ws.counters);
  SHF_HIP_OK(hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------------------
// forward_net post-processing + the >thresh cut of detect() on the device
// (lib/test.py:52-54 flip fix, :59-66 unscale, :163-167 threshold), for a GROUP of units in one launch.  Rows of a
// unit are score-descending, so its survivors are a prefix (found by bisection) and unit u lands behind the
// survivors of units 0..u-1: the image list is in the reference's concatenation order.
// dst->count: slot (pass & 1) holds the list length before this pass, slot ((pass + 1) & 1) receives the length
// after it (two slots: no block of this launch reads what another one writes).
// ---------------------------------------------------------------------------
struct AppendGM {
  const float* boxes5;
  const float* probs2;
  const int* counters;  // the unit's tail counters (rows R derived like the gather stage does)
  float im_w, im_scale;
  int flip;
  // destination list (per member in per-member-list mode, else the same for all)
  float* dets5;
  unsigned long long* keys;
  int* count;
  int cap;
};
struct AppendGK {
  int n, topN, pass, per_member;
  float thresh;
  int blk_start[TG + 1];
  AppendGM m[TG];
};

__device__ __forceinline__ int survivors(const float* probs2, int R, float thresh) {
  int lo = 0, hi = R;  // first r with !(fg > thresh)
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (probs2[mid * 2 + 1] > thresh) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__global__ void append_dets_kernel(AppendGK g) {
  const int mi = tail_find_member(g.blk_start, blockIdx.x);
  const AppendGM& p = g.m[mi];
  const int lb = blockIdx.x - g.blk_start[mi], lgrid = g.blk_start[mi + 1] - g.blk_start[mi];
  int base, ns;
  if (g.per_member) {
    base = 0;
    ns = survivors(p.probs2, tail_rows(p.counters, g.topN, nullptr), g.thresh);
    if (lb == 0 && threadIdx.x == 0) { p.count[0] = 0; p.count[1] = min(ns, p.cap); }
  } else {
    base = p.count[g.pass & 1];
    for (int v = 0; v < mi; ++v) base += survivors(g.m[v].probs2, tail_rows(g.m[v].counters, g.topN, nullptr), g.thresh);
    ns = survivors(p.probs2, tail_rows(p.counters, g.topN, nullptr), g.thresh);
    if (mi == g.n - 1 && lb == 0 && threadIdx.x == 0) p.count[(g.pass + 1) & 1] = min(base + ns, p.cap);
  }
  for (int r = lb * blockDim.x + threadIdx.x; r < ns; r += lgrid * blockDim.x) {
    const int pos = base + r;
    if (pos >= p.cap) continue;
    const float fg = p.probs2[r * 2 + 1];
    float x1 = p.boxes5[r * 5 + 1], y1 = p.boxes5[r * 5 + 2], x2 = p.boxes5[r * 5 + 3], y2 = p.boxes5[r * 5 + 4];
    if (p.flip) {  // boxes[:, [1,3]] = w - boxes[:, [3,1]]
      const float nx1 = p.im_w - x2, nx2 = p.im_w - x1;
      x1 = nx1;
      x2 = nx2;
    }
    float* d = p.dets5 + (size_t)pos * 5;
    d[0] = x1 / p.im_scale; d[1] = y1 / p.im_scale; d[2] = x2 / p.im_scale; d[3] = y2 / p.im_scale; d[4] = fg;
    p.keys[pos] = score_key(fg, (unsigned)pos);
  }
}

int launch_append_dets_group(const AppendUnit* us, int n, int topN, float thresh, int pass, int per_member,
                             hipStream_t s) {
  if (n < 1 || n > TG) { set_error("append group: 1..16 units"); return -1; }
  AppendGK g;
  g.n = n; g.topN = topN; g.pass = pass; g.per_member = per_member; g.thresh = thresh;
  int blocks = 0;
  for (int q = 0; q <= TG; ++q) g.blk_start[q] = 0x7fffffff;
  for (int m = 0; m < n; ++m) {
    AppendGM& d = g.m[m];
    d.boxes5 = us[m].boxes5; d.probs2 = us[m].probs2; d.counters = us[m].counters;
    d.im_w = us[m].im_w; d.im_scale = us[m].im_scale; d.flip = us[m].flip;
    d.dets5 = us[m].dets5; d.keys = us[m].keys; d.count = us[m].count; d.cap = us[m].cap;
    g.blk_start[m] = blocks;
    blocks += (int)grid_for(us[m].r_max < 1 ? 1 : us[m].r_max);
  }
  g.blk_start[n] = blocks;
  hipLaunchKernelGGL(append_dets_kernel, dim3(blocks), dim3(256), 0, s, g);
  SHF_HIP_OK(hipGetLastError());
  return 0;
}

}  // namespace shf
