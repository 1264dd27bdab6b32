// WIDER FACE evaluation on the device: the per-image matching and the threshold sweep of
//   image_eval / img_pr_info / dataset_pr_info    lib/wider_eval_tools/wider_eval.py:62-130
// in the parallel form of DESIGN.md 4.11 (tests/wider_eval_cases.py: parallel_counts is its numpy restatement):
//   match   the ground-truth box a detection is attributed to is the first arg-max of its IoU row (of floor(IoU + 0.5)
//           under mimic_eval_bug); it depends on the boxes alone, not on the detections before it and not on the setting.
//           One lane per detection walks the image's boxes in index order and keeps a strictly greater key, so the
//           first index wins without any cross-lane reduction; an atomic min leaves first[g], the earliest detection
//           matched to box g.
//   counts  per (image, setting): proposal[h] and flag[h] (h is the first hit of a box of the subset) from match, first
//           and the subset mask; inclusive wave scans with a carry give hits[] and the running number of proposals.
//   sweep   per (image, setting): per threshold a binary search in the score-descending detections, then two 64-bit
//           vector atomic adds into the (S, T, 2) totals.  Integer sums: exact in any order.
// All box arithmetic is fp64 in the operation order of _overlaps(); compiled with -ffp-contract=off, so every add, multiply
// and divide rounds like numpy's.
//
// AFW / Pascal Faces evaluation: one matching round of
//   VOCprRecordOptim    external/marcopede-face-eval-f2870fd85d48/VOCpr.py:118-162   (IoU: util.py:176-193)
// face_match_kernel, below (smallhardface_amd/face_eval.py: match_host is its numpy restatement).
//
// FDDB evaluation: the pixel counts of ellipse and rectangle masks, fddb_pairs_kernel / fddb_areas_kernel at the end of this
// file (smallhardface_amd/fddb_eval.py: pair_counts_host is their numpy restatement).
#include "eval.h"

namespace shf {

typedef unsigned long long u64;

static inline unsigned eval_grid_for(long long n, int block = 256) {
  long long g = (n + block - 1) / block;
  if (g > 256 * 16) g = 256 * 16;
  if (g < 1) g = 1;
  return (unsigned)g;
}

// every ground-truth box once: (x, y, w, h) -> x1, y1, x2 = w + x, y2 = h + y and its +1-pixel area, as image_counts and
// _overlaps form them; first[] starts at "no detection"
__global__ void eval_prep_kernel(const double* __restrict__ gt4, int G, double* __restrict__ gt5, int* __restrict__ first) {
  for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < G; g += gridDim.x * blockDim.x) {
    const double x1 = gt4[(size_t)g * 4 + 0], y1 = gt4[(size_t)g * 4 + 1];
    const double x2 = gt4[(size_t)g * 4 + 2] + x1, y2 = gt4[(size_t)g * 4 + 3] + y1;
    double* o = gt5 + (size_t)g * 5;
    o[0] = x1; o[1] = y1; o[2] = x2; o[3] = y2;
    o[4] = (x2 - x1 + 1) * (y2 - y1 + 1);
    first[g] = 0x7FFFFFFF;
  }
}

// one wave per tile of 64 detections of one image; lane = detection.  The box index of the loop is wave-uniform: every
// lane reads the same converted box.  match[h] = global index of the box detection h is matched to, or -1.
__global__ __launch_bounds__(64) void eval_match_kernel(const double* __restrict__ pred5, const int* __restrict__ pred_off,
                                                        const int* __restrict__ gt_off, const double* __restrict__ gt5,
                                                        const int* __restrict__ tile_img, const int* __restrict__ tile_start,
                                                        double iou_thresh, int mimic_eval_bug, int* __restrict__ match,
                                                        int* __restrict__ first) {
  const int img = tile_img[blockIdx.x];
  const int h = tile_start[blockIdx.x] + (int)threadIdx.x;
  if (h >= pred_off[img + 1]) return;
  const int g0 = gt_off[img], g1 = gt_off[img + 1];
  const double* p = pred5 + (size_t)h * 5;
  const double b0 = p[0], b1 = p[1], b2 = p[2] + b0, b3 = p[3] + b1;
  const double area_det = (b2 - b0 + 1) * (b3 - b1 + 1);
  double best = 0;
  int idx = -1;
  for (int g = g0; g < g1; ++g) {
    const double* q = gt5 + (size_t)g * 5;
    const double iw = (q[2] < b2 ? q[2] : b2) - (q[0] > b0 ? q[0] : b0) + 1;
    const double ih = (q[3] < b3 ? q[3] : b3) - (q[1] > b1 ? q[1] : b1) + 1;
    const double inter = iw * ih;
    double uni = q[4] + area_det - inter;
    if (uni == 0) uni = INFINITY;
    double o = inter / uni;
    if (iw <= 0 || ih <= 0) o = 0;
    if (mimic_eval_bug) o = floor(o + 0.5);
    if (idx < 0 || o > best) { best = o; idx = g; }   // np.argmax: the first of equal keys
  }
  const bool matched = idx >= 0 && best >= iou_thresh;
  match[h] = matched ? idx : -1;
  if (matched) atomicMin(first + idx, h);
}

__device__ __forceinline__ int wave_inclusive_scan(int v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(v, o, 64);
    if (lane >= o) v += u;
  }
  return v;
}

// one wave per (image, setting): segmented inclusive scans over the image's detections, 64 at a time with a carry
__global__ __launch_bounds__(64) void eval_counts_kernel(const int* __restrict__ pred_off, const int* __restrict__ match,
                                                         const int* __restrict__ first, const uint8_t* __restrict__ counted,
                                                         int N, int G, int* __restrict__ hits, int* __restrict__ cum_prop,
                                                         uint8_t* __restrict__ proposal) {
  const int img = blockIdx.x, s = blockIdx.y, lane = threadIdx.x;
  const int h0 = pred_off[img], h1 = pred_off[img + 1];
  const uint8_t* cnt = counted + (size_t)s * G;
  const size_t row = (size_t)s * N;
  int carry_hits = 0, carry_prop = 0;
  for (int base = h0; base < h1; base += 64) {
    const int h = base + lane;
    int flag = 0, prop = 0;
    if (h < h1) {
      const int m = match[h];
      const bool in_subset = m >= 0 && cnt[m] != 0;
      flag = in_subset && first[m] == h;
      prop = !(m >= 0 && !in_subset);
    }
    const int sf = wave_inclusive_scan(flag, lane), sp = wave_inclusive_scan(prop, lane);
    if (h < h1) {
      hits[row + h] = carry_hits + sf;
      cum_prop[row + h] = carry_prop + sp;
      if (proposal) proposal[row + h] = (uint8_t)prop;
    }
    carry_hits += __shfl(sf, 63, 64);
    carry_prop += __shfl(sp, 63, 64);
  }
}

// one block per (image, setting), a thread per threshold: cnt = number of detections with score >= thresh (the scores fall),
// then info = (cum_prop[cnt - 1], hits[cnt - 1]) when cnt > 0 (image_pr_info)
__global__ __launch_bounds__(256) void eval_sweep_kernel(const double* __restrict__ pred5, const int* __restrict__ pred_off,
                                                         const int* __restrict__ gt_off, const int* __restrict__ hits,
                                                         const int* __restrict__ cum_prop, int N,
                                                         const double* __restrict__ thresh, int T, u64* __restrict__ totals) {
  const int img = blockIdx.x, s = blockIdx.y;
  const int h0 = pred_off[img], n = pred_off[img + 1] - h0;
  if (n == 0 || gt_off[img + 1] == gt_off[img]) return;   // (evaluate_setting skips such an image)
  const double* score = pred5 + (size_t)h0 * 5 + 4;
  const size_t row = (size_t)s * N + h0;
  for (int t = threadIdx.x; t < T; t += blockDim.x) {
    const double thr = thresh[t];
    int lo = 0, hi = n;
    while (lo < hi) {
      const int mid = lo + ((hi - lo) >> 1);
      if (score[(size_t)mid * 5] >= thr) lo = mid + 1; else hi = mid;
    }
    if (lo > 0) {
      const int np = cum_prop[row + lo - 1], nh = hits[row + lo - 1];
      u64* o = totals + ((size_t)s * T + t) * 2;
      if (np) atomicAdd(o, (u64)np);
      if (nh) atomicAdd(o + 1, (u64)nh);
    }
  }
}

int launch_eval_prep(const double* gt4, int G, double* gt5, int* first, hipStream_t s) {
  if (G == 0) return 0;
  hipLaunchKernelGGL(eval_prep_kernel, dim3(eval_grid_for(G)), dim3(256), 0, s, gt4, G, gt5, first);
  SHF_HIP_OK(hipGetLastError());
  return 0;
}

int launch_eval_match(const double* pred5, const int* pred_off, const int* gt_off, const double* gt5, const int* tile_img,
                      const int* tile_start, int n_tiles, double iou_thresh, int mimic_eval_bug, int* match, int* first,
                      hipStream_t s) {
  if (n_tiles == 0) return 0;
  hipLaunchKernelGGL(eval_match_kernel, dim3((unsigned)n_tiles), dim3(64), 0, s, pred5, pred_off, gt_off, gt5, tile_img,
                     tile_start, iou_thresh, mimic_eval_bug, match, first);
  SHF_HIP_OK(hipGetLastError());
  return 0;
}

int launch_eval_counts(const int* pred_off, const int* match, const int* first, const uint8_t* counted, int n_images,
                       int n_settings, int N, int G, int* hits, int* cum_prop, uint8_t* proposal, hipStream_t s) {
  if (n_images == 0 || N == 0) return 0;
  hipLaunchKernelGGL(eval_counts_kernel, dim3((unsigned)n_images, (unsigned)n_settings), dim3(64), 0, s, pred_off, match,
                     first, counted, N, G, hits, cum_prop, proposal);
  SHF_HIP_OK(hipGetLastError());
  return 0;
}

int launch_eval_sweep(const double* pred5, const int* pred_off, const int* gt_off, const int* hits, const int* cum_prop,
                      int n_images, int n_settings, int N, const double* thresh, int T, unsigned long long* totals,
                      hipStream_t s) {
  if (n_images == 0 || N == 0) return 0;
  hipLaunchKernelGGL(eval_sweep_kernel, dim3((unsigned)n_images, (unsigned)n_settings), dim3(256), 0, s, pred5, pred_off,
                     gt_off, hits, cum_prop, N, thresh, T, totals);
  SHF_HIP_OK(hipGetLastError());
  return 0;
}

// ---- AFW / Pascal Faces: one matching round (VOCpr.py:118-162) ---------------------------------------------------------------
// One wave per image walks the image's detections in their (score-descending) order; the lanes stride over the image's boxes.
//   IoU     util.overlap (util.py:176-193) on x1-y1-x2-y2 rows: abs() extents + 1, a strict > intersection test,
//           ia / (a1 + a2 - ia), every operation in that order.
//   choice  the reference keeps a box when covr >= maxovr, starting from maxovr = 0, gt = 0: it ends on the LAST index
//           holding max(0, largest covr), or on (0, index 0) when no covr reaches 0.  A lane walks its boxes in rising index
//           order with the same >=, the butterfly keeps the larger value and among equal values the larger index.
//   verdict lane 0 alone: false positive unless maxovr > ovr; on a difficult box neither; else the box's taken flag decides
//           and is set.  taken[] is a per-call scratch segment laid out like the boxes, zero on entry; only lane 0 of the
//           image's own wave reads and writes the image's flags, in program order.
// Latency-bound by construction: the detections of an image are a serial chain, the work per link is a handful of boxes.
__global__ __launch_bounds__(64) void face_match_kernel(const double* __restrict__ det4, const int* __restrict__ det_off,
                                                        const double* __restrict__ gt4, const int* __restrict__ gt_off,
                                                        const uint8_t* __restrict__ difficult, double ovr,
                                                        uint8_t* __restrict__ taken, int* __restrict__ code,
                                                        int* __restrict__ index) {
  const int img = blockIdx.x, lane = threadIdx.x;
  const int h0 = det_off[img], h1 = det_off[img + 1];
  const int g0 = gt_off[img], ng = gt_off[img + 1] - g0;
  if (ng == 0) {   // no ground truth (an unknown image): every detection is a false positive
    for (int h = h0 + lane; h < h1; h += 64) { code[h] = kFaceFalsePositive; index[h] = -1; }
    return;
  }
  for (int h = h0; h < h1; ++h) {
    const double* p = det4 + (size_t)h * 4;   // (wave-uniform: every lane reads the same detection)
    const double dx1 = p[0], dy1 = p[1], dx2 = p[2], dy2 = p[3];
    const double a1 = (fabs(dx1 - dx2) + 1) * (fabs(dy1 - dy2) + 1);
    double best = -INFINITY;
    int bi = -1;
    for (int j = lane; j < ng; j += 64) {
      const double* q = gt4 + (size_t)(g0 + j) * 4;
      const double gx1 = q[0], gy1 = q[1], gx2 = q[2], gy2 = q[3];
      const double a2 = (fabs(gx1 - gx2) + 1) * (fabs(gy1 - gy2) + 1);
      double ia = 0;
      if (dy2 > gy1 && gy2 > dy1 && dx2 > gx1 && gx2 > dx1) {
        const double xx1 = gx1 > dx1 ? gx1 : dx1, yy1 = gy1 > dy1 ? gy1 : dy1;
        const double xx2 = gx2 < dx2 ? gx2 : dx2, yy2 = gy2 < dy2 ? gy2 : dy2;
        ia = (xx2 - xx1 + 1) * (yy2 - yy1 + 1);
      }
      const double c = ia / (a1 + a2 - ia);
      if (c >= best) { best = c; bi = j; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double ob = __shfl_xor(best, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (ob > best || (ob == best && oi > bi)) { best = ob; bi = oi; }
    }
    if (lane == 0) {
      double maxovr = 0;
      int gi = 0;
      if (bi >= 0 && best >= 0.0) { maxovr = best; gi = bi; }
      int c = kFaceFalsePositive;
      if (maxovr > ovr) {
        if (difficult[g0 + gi]) c = kFaceNeither;
        else if (!taken[g0 + gi]) { taken[g0 + gi] = 1; c = kFaceTruePositive; }
      }
      code[h] = c;
      index[h] = gi;
    }
  }
}

int launch_face_match(const double* det4, const int* det_off, const double* gt4, const int* gt_off, const uint8_t* difficult,
                      int n_images, double ovr, uint8_t* taken, int* code, int* index, hipStream_t s) {
  if (n_images == 0) return 0;
  hipLaunchKernelGGL(face_match_kernel, dim3((unsigned)n_images), dim3(64), 0, s, det4, det_off, gt4, gt_off, difficult, ovr,
                     taken, code, index);
  SHF_HIP_OK(hipGetLastError());
  return 0;
}

// ---- FDDB: pixel counts of ellipse and rectangle masks (smallhardface_amd/fddb_eval.py: pair_counts_host) -----------------------
// A pixel (ix, iy) is inside the ellipse row ra, rb, c, s, cx, cy when, with dx = ix - cx, dy = iy - cy, u = dx*c + dy*s,
// v = dy*c - dx*s,   (u*u)*(rb*rb) + (v*v)*(ra*ra) <= (ra*ra)*(rb*rb)   -- fp64 adds, multiplies and one compare in that order
// (c = cos(angle), s = sin(angle) come from the host).  The 64 lanes sweep the inclusive box x0..x1 x y0..y1 row-major, 64
// pixels a step; every lane tests its pixel, the wave adds popcount(ballot) to a wave-uniform counter.  The box is at most
// kFddbMaxScanBox pixels and every corner below kFddbMaxCoord in magnitude (checked by the caller), so w * h fits an int.
// No atomics, no LDS, no floating-point output: one wave owns one count.
__device__ __forceinline__ int fddb_sweep(const double* __restrict__ e, int x0, int y0, int x1, int y1, int lane) {
  const int w = x1 - x0 + 1, h = y1 - y0 + 1;
  if (w <= 0 || h <= 0) return 0;   // (wave-uniform: an empty pair costs its wave these few instructions)
  const int n = w * h;
  const double ra = e[0], rb = e[1], c = e[2], s = e[3], cx = e[4], cy = e[5];
  const double ra2 = ra * ra, rb2 = rb * rb, rhs = ra2 * rb2;
  // lane's pixel of the step, kept without a division per step: 64 pixels on are step_y rows down and step_x columns right
  const int step_y = 64 / w, step_x = 64 % w;
  int x = lane % w, y = lane / w, total = 0;
  for (int base = 0; base < n; base += 64) {
    bool in = false;
    if (base + lane < n) {
      const double dx = (double)(x0 + x) - cx, dy = (double)(y0 + y) - cy;
      const double u = dx * c + dy * s, v = dy * c - dx * s;
      in = (u * u) * rb2 + (v * v) * ra2 <= rhs;
    }
    total += __popcll(__ballot(in));
    x += step_x;
    y += step_y;
    if (x >= w) { x -= w; ++y; }
  }
  return total;
}

__global__ __launch_bounds__(64) void fddb_pairs_kernel(const double* __restrict__ ell6, const int* __restrict__ ell_box,
                                                        const int* __restrict__ rect4, const int* __restrict__ pair_off,
                                                        const int* __restrict__ det0, int A, int* __restrict__ inter) {
  const int p = blockIdx.x, lane = threadIdx.x;
  // the annotation owning pair p: the last a with pair_off[a] <= p (pair_off[0] = 0 <= p < pair_off[A]; an annotation
  // without detections has an empty range and is never the last)
  int lo = 0, hi = A;
  while (hi - lo > 1) {
    const int mid = lo + ((hi - lo) >> 1);
    if (pair_off[mid] <= p) lo = mid; else hi = mid;
  }
  const int a = lo, d = det0[a] + (p - pair_off[a]);
  const int* b = ell_box + (size_t)a * 4;
  const int* r = rect4 + (size_t)d * 4;
  const int x0 = b[0] > r[0] ? b[0] : r[0], y0 = b[1] > r[1] ? b[1] : r[1];
  const int x1 = b[2] < r[2] ? b[2] : r[2], y1 = b[3] < r[3] ? b[3] : r[3];
  const int total = fddb_sweep(ell6 + (size_t)a * 6, x0, y0, x1, y1, lane);
  if (lane == 0) inter[p] = total;
}

__global__ __launch_bounds__(64) void fddb_areas_kernel(const double* __restrict__ ell6, const int* __restrict__ ell_box,
                                                        int* __restrict__ area) {
  const int a = blockIdx.x, lane = threadIdx.x;
  const int* b = ell_box + (size_t)a * 4;
  const int total = fddb_sweep(ell6 + (size_t)a * 6, b[0], b[1], b[2], b[3], lane);
  if (lane == 0) area[a] = total;
}

int launch_fddb_pairs(const double* ell6, const int* ell_box, const int* rect4, const int* pair_off, const int* det0, int A,
                      int n_pairs, int* inter, hipStream_t s) {
  if (n_pairs == 0) return 0;
  hipLaunchKernelGGL(fddb_pairs_kernel, dim3((unsigned)n_pairs), dim3(64), 0, s, ell6, ell_box, rect4, pair_off, det0, A,
                     inter);
  SHF_HIP_OK(hipGetLastError());
  return 0;
}

int launch_fddb_areas(const double* ell6, const int* ell_box, int A, int* area, hipStream_t s) {
  if (A == 0) return 0;
  hipLaunchKernelGGL(fddb_areas_kernel, dim3((unsigned)A), dim3(64), 0, s, ell6, ell_box, area);
  SHF_HIP_OK(hipGetLastError());
  return 0;
}

}  // namespace shf
