// tensor_kernel.h — arguments of the tensor export kernel (tensor.hip), shared with its host entry
// points (tensor.cpp: mp2vg_tensor_slots / mp2vg_tensor_planes) and the host-only side of the
// contract (runtime.cpp: tap tables, validation, sizes).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/mp2vg.h"

namespace mp2vg {

// source columns one workgroup keeps in LDS (the V rows of its two output rows, 3 channels of
// int16 each: 24 KB)
constexpr int kTensorSegCols = 2048;

// One launch exports n frames.  Planes as in ExportArgs; every table is int32 in device memory.
//   segs[4 s ..]: output columns [o_begin, o_end) of segment s, the first source column `base` any
//                 of them reads (relative to the rectangle) and the 4-pixel units that cover the
//                 columns base .. the last one read; every tap range of the segment lies inside
//                 [base, base + kTensorSegCols)
//   hfirst / hw: horizontal taps of output column o: hw[o * hmax + k], zero from the column's tap
//                 count on (the kernel runs all hmax); vfirst / vcount / vw: the rows'
//   fields[n]: MP2VG_FIELD_* of each frame, or null: every frame in mode `field`.  Read by the
//                 field-mode kernel only (launch_tensor's field_modes).
struct TensorArgs {
    const uint64_t* ftab;
    const int32_t* slots;
    const uint8_t* planes[3];
    uint32_t plane_off[3];
    int32_t stride[3];
    int32_t cw, ch;
    int32_t cy, crv, cgu, cgv, cbu, kr, kg, kb;  // as ExportArgs
    int32_t src_x, src_y;                        // top-left of the source rectangle
    int32_t out_w, out_h;
    const int32_t *segs, *hfirst, *hw, *vfirst, *vcount, *vw;
    int32_t hmax, vmax;
    float scale[3], bias[3];
    void* dst;
    // field modes, behind the arguments of the kernel without them (whose code they leave as it was)
    const int32_t* fields;
    int32_t field;
    int32_t coded_h;
    // placement, behind those (read by the placed kernel only): the picture's rectangle in the
    // out_w x out_h canvas; the tables are then those of dst_w x dst_h.  padq[c] = 64 pad[c].
    int32_t dst_x, dst_y, dst_w, dst_h;
    int32_t padq[3];
    // items, behind those (read by the items kernel only): the staged blob, which starts with the n
    // item records (kItem* below) and holds the shared tap tables behind them; every table of an
    // item is found at items + the record's offset.  The pointers and counts above that a record
    // replaces (slots, fields, src_x / src_y, the six tables, hmax, vmax) are not read.
    const int32_t* items;
    int32_t clip_len;  // planar layout [n / clip_len][3][clip_len][h][w]
};

// One item of an items launch as the kernel reads it: kItemWords int32 words.  Offsets are in words
// from the start of the blob.  kItemPlane is the planar plane index of channel 0,
// (i / clip_len) 3 clip_len + i % clip_len (channel c is clip_len planes further), so the kernel
// divides nothing.
enum {
    kItemSlot = 0, kItemField, kItemSrcX, kItemSrcY, kItemFlags, kItemNsegs, kItemHmax, kItemVmax,
    kItemSegs, kItemHfirst, kItemHw, kItemVfirst, kItemVcount, kItemVw, kItemPlane, kItemSpare,
    kItemWords
};

// cf 1..3; layout, chroma, dtype of the mp2vg_tensor_t; grid = (nsegs, row pairs of out_h, n).
// field_modes = false: every frame PROGRESSIVE, the kernel without the field row walk.
// placed = true: the placed kernel (always with the field row walk, whatever field_modes says).
hipError_t launch_tensor(int cf, int layout, int chroma, int dtype, bool field_modes, bool placed, const TensorArgs& a,
                         int nsegs, int n, hipStream_t stream);
// the items kernel (always with the field row walk, never placed); nsegs = the largest segment
// count of any item: a workgroup past its item's count returns at once
hipError_t launch_tensor_items(int cf, int layout, int chroma, int dtype, const TensorArgs& a, int nsegs, int n,
                               hipStream_t stream);

// host-only side (runtime.cpp)
// checks t against a coded size; the source rectangle in rect[4] (x, y, w, h) and the element size
int check_tensor(const mp2vg_tensor_t* t, int32_t coded_w, int32_t coded_h, int32_t rect[4], int32_t* elem);
// the same with a placement (null: none): dst[4] = the picture's rectangle in the output (the whole
// output without a placement), *placed = whether anything is left to pad
int check_tensor_placed(const mp2vg_tensor_t* t, const mp2vg_tensor_place_t* place, int32_t coded_w, int32_t coded_h,
                        int32_t rect[4], int32_t* elem, int32_t dst[4], bool* placed);
// The int32 tables of a validated tensor export, behind `lead` entries left for the caller (the
// slot list, then the field list of a launch with field modes): segs, hfirst, hw, vfirst, vcount,
// vw.  off[6] = the index of each in blob.
struct TensorTables {
    std::vector<int32_t> blob;
    size_t off[6];
    int32_t nsegs, hmax, vmax;
};
int tensor_tables(const int32_t rect[4], int32_t out_w, int32_t out_h, size_t lead, TensorTables* tt);
// a field mode's preconditions on the coded frame (include/mp2vg.h "Field modes")
int check_tensor_field(int32_t field, int32_t cf, int32_t coded_h);

// An items launch (include/mp2vg.h "Items"), validated and planned with no device.  nslots < 0:
// the slot count is not known (mp2vg_tensor_items_plan); planes: every slot must be 0.
struct ItemsPlan {
    std::vector<int32_t> blob;        // n records of kItemWords, the horizontal tables, the vertical tables
    std::vector<int32_t> htab, vtab;  // per item: its table, numbered in order of first use
    int32_t nh, nv, grid_x, elem;
};
int tensor_items_plan(const mp2vg_tensor_t* t, const mp2vg_tensor_item_t* items, int32_t n, int32_t clip_len, int32_t cf,
                      int32_t coded_w, int32_t coded_h, int32_t nslots, bool planes, ItemsPlan* plan);

}  // namespace mp2vg
