// Launcher of the per-class detection-list kernels (class_lists.hip), called by shf_class_lists_add and
// shf_debug_class_lists_add (net_class_lists.cpp).
#pragma once
#include "shf_internal.h"

namespace shf {

// What AppendUnit / launch_append_dets_group do for two classes, for a net with C classes, 2 .. 8
// (lib/test.py:52-66,161-167): each foreground class c gets the rows with probs[r, c] > thresh of the group's units, in
// (unit, row) order, appended behind the len[c - 1] rows list c - 1 already holds (list c - 1 is dets5 + (c - 1) * cap * 5);
// len is clamped to cap and rows beyond it are dropped.  R is host-known: the rows the unit's forward recorded; a unit with
// R = 0 contributes nothing.  `tiles`: workspace of (C - 1) * class_lists_tile_count() ints.
constexpr int kClassListsMaxUnits = 16;
constexpr int kClassListsMaxRows = 1 << 24;   // per unit: keeps every list position of a group inside an int
struct ClassListsUnit {
  const float* boxes5;
  const float* probs;   // (R, C) row-major
  int R;
  float im_w, im_scale;
  int flip;
};
int class_lists_tile_count(const ClassListsUnit* us, int n);
int launch_class_lists_add(const ClassListsUnit* us, int n, int C, float thresh, float* dets5, int cap, int* tiles,
                           int* len, hipStream_t s);

}  // namespace shf
