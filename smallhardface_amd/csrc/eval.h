// Launchers of the evaluation kernels (eval.hip): WIDER, called by shf_wider_eval_counts, AFW / Pascal Faces, called by
// shf_face_eval_match, and FDDB, called by shf_fddb_pair_counts (net_api.cpp).
#pragma once
#include "shf_internal.h"

namespace shf {

// A lane of the match kernel walks all the ground-truth boxes of its image one after the other: the cap bounds how long one
// wave can run (WIDER's largest image has under 2 000 faces).
constexpr int kEvalMaxGtPerImage = 65536;
// gt4 (G,4) x-y-w-h -> gt5 (G,5) x1-y1-x2-y2-area; first[g] = INT_MAX
int launch_eval_prep(const double* gt4, int G, double* gt5, int* first, hipStream_t s);
// tile k covers detections tile_start[k] .. + 63 of image tile_img[k]; match[h] = matched box (global index) or -1,
// first[g] = the earliest detection matched to box g
int launch_eval_match(const double* pred5, const int* pred_off, const int* gt_off, const double* gt5, const int* tile_img,
                      const int* tile_start, int n_tiles, double iou_thresh, int mimic_eval_bug, int* match, int* first,
                      hipStream_t s);
// hits / cum_prop (S,N): inclusive scans per (setting, image); proposal (S,N) may be null
int launch_eval_counts(const int* pred_off, const int* match, const int* first, const uint8_t* counted, int n_images,
                       int n_settings, int N, int G, int* hits, int* cum_prop, uint8_t* proposal, hipStream_t s);
// totals (S,T,2) must be zero on entry
int launch_eval_sweep(const double* pred5, const int* pred_off, const int* gt_off, const int* hits, const int* cum_prop,
                      int n_images, int n_settings, int N, const double* thresh, int T, unsigned long long* totals,
                      hipStream_t s);

// the per-detection codes of shf_face_eval_match
constexpr int kFaceNeither = 0, kFaceTruePositive = 1, kFaceFalsePositive = 2;
// one wave per image: code[h], index[h] (box within the image, -1 without boxes) for the x1-y1-x2-y2 rows det4 / gt4;
// taken (G) must be zero on entry
int launch_face_match(const double* det4, const int* det_off, const double* gt4, const int* gt_off, const uint8_t* difficult,
                      int n_images, double ovr, uint8_t* taken, int* code, int* index, hipStream_t s);

// One wave sweeps an ellipse's scan box (or its part inside a rectangle) 64 pixels at a time: the cap bounds how long it can
// run.  2^20 pixels = 16 384 steps; FDDB's images are under 500 pixels a side, so any real face passes.
constexpr long long kFddbMaxScanBox = 1ll << 20;
// one 64-lane block per pair: a launch holds at most 2^32 - 1 threads, so 2^26 pairs or more cannot be one launch
constexpr long long kFddbMaxPairs = 1ll << 26;
// every integer corner stays below this in magnitude, so extents and pixel indices fit an int
constexpr int kFddbMaxCoord = 1 << 30;
// one wave per (annotation, detection) pair: pair p belongs to the annotation a with pair_off[a] <= p < pair_off[a + 1]
// (A + 1 offsets) and to detection det0[a] + p - pair_off[a]; inter[p] = pixels of rect n scan box inside the ellipse
int launch_fddb_pairs(const double* ell6, const int* ell_box, const int* rect4, const int* pair_off, const int* det0, int A,
                      int n_pairs, int* inter, hipStream_t s);
// one wave per annotation: area[a] = pixels of the scan box inside the ellipse
int launch_fddb_areas(const double* ell6, const int* ell_box, int A, int* area, hipStream_t s);

}  // namespace shf
