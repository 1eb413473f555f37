// tensor.hip — decoded frames to cropped, antialias-resized, normalised model-input tensors on the
// device (gfx950 / CDNA4), one launch per batch, no full-size RGB intermediate in memory.
//
// The arithmetic is the bit-exact contract of include/mp2vg.h ("tensor export"): the RGB export's
// 8-bit R'G'B' of the whole coded frame, cropped, then the triangle filter with 14-bit integer
// weights (host tables, mp2vg_tensor_weights), vertical pass first, then horizontal, then
// fmaf(Q / 64, scale, bias) and one round-to-nearest-even cast.
//
// Work split: a workgroup of 256 lanes owns two adjacent output rows of one frame (blockIdx.y,
// blockIdx.z; the last row of an odd height alone) and one segment of their columns (blockIdx.x; a
// segment is the run of output columns whose taps fit a window of kTensorSegCols = 2048 source
// columns, so a 1920-wide source is one segment).
//   vertical pass: a lane takes 4 source columns (a unit, as in export.hip: unaligned dword loads
//       clamped into the plane row, chroma taps of the RGB export) and walks the union of the two
//       rows' source rows, converting each to R'G'B' in registers once and accumulating qv P for
//       both output rows in 2 x 12 int32 (adjacent rows share half their taps when downscaling,
//       nearly all when upscaling); the rounded V values (0..16320) are parked in LDS as int16,
//       [2][3][2048]: 24 KB per workgroup whatever the ratio, one 8-byte store per row and channel.
//   horizontal pass: after one barrier, a lane takes one output element (row, pixel, channel),
//       sums its taps from LDS (every lane the axis' longest count, over zero-padded weights: a
//       uniform, unrolled loop keeps several tap loads in flight), normalises, casts and stores the
//       element (coalesced along the row; the output is small, so element stores do not matter:
//       dst needs element alignment only).
// When downscaling, a source row is still converted by about 1.5 workgroups and read that often
// (from L2 mostly), against write + read of 3 B/pixel RGB and a 12 B/pixel float intermediate on
// the unfused path.
//
// Field modes (mp2vg_tensor_slots_fields, include/mp2vg.h "Field modes"): the kernel is
// instantiated twice.  FIELDS = false is the walk above for launches whose frames are all
// PROGRESSIVE; FIELDS = true reads the mode of its frame and changes the vertical pass only: field
// chroma siting per line, and for TOP / BOTTOM a walk over the field's lines alone, with the rows
// between them made from the rounded average of two converted lines (comment at the walk).
//
// Placement (mp2vg_tensor_slots_placed, include/mp2vg.h "Placement"): a third instantiation,
// PLACED = true, always with the field row walk (a placed launch of PROGRESSIVE frames runs that walk
// in mode PROGRESSIVE), so the two above keep their code.  blockIdx.y runs over row pairs of the
// canvas; whether a canvas row is a picture row is uniform, the vertical pass accumulates for the
// picture rows of the pair only (none: skipped), and the horizontal pass writes the pad through the
// same normalise / cast as the picture (comments at both).
//
// Items (mp2vg_tensor_items, include/mp2vg.h "Items"): a fourth instantiation, ITEMS = true, always
// with the field row walk and never placed, so the three above keep their code (they read every
// argument where they read it before).  blockIdx.z is the item; its record (tensor_kernel.h: slot,
// mode, rectangle origin, where its tables lie, their nsegs / hmax / vmax, the mirror flag, its
// first output plane) is loaded once with scalar loads and stays in SGPRs.  The grid has the
// launch's largest segment count: a workgroup past its item's returns before the barrier.  The
// mirror and the clip layout change the store address only (comment at the store).
//
// Static resources (hipcc -O3, --offload-arch=gfx950, 40 variants each): 60-68 VGPRs without
// field modes, 65-72 with, 65-74 placed, 65-72 items (72-86 SGPRs, the field kernel's 66-80 plus
// the record), no scratch, 24576 B LDS per workgroup, which sets 6 waves
// per SIMD (up to 80 VGPRs keep that; measured speed, also of the one-row split this replaced:
// profiles/export/tensor.md; of the items launch: profiles/export/items.md).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mp2vg.h"
#include "export_pixels.h"
#include "tensor_kernel.h"

namespace mp2vg {

// the RGB export's matrix arithmetic on 4 pixels: luma dword yv, 8-bit chroma cb / cr -> R, G, B (0..255)
__device__ __forceinline__ void matrix4(const TensorArgs& a, uint32_t yv, const int cb[4], const int cr[4], int R[4],
                                        int G[4], int B[4]) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int yy = __mul24(a.cy, byte_of(yv, i));
        const int tr = __mul24(a.crv, cr[i]) + a.kr;
        const int tg = __mul24(a.cgu, cb[i]) + __mul24(a.cgv, cr[i]) + a.kg;
        const int tb = __mul24(a.cbu, cb[i]) + a.kb;
        R[i] = (int)clamp8((yy + tr) >> 14);
        G[i] = (int)clamp8((yy + tg) >> 14);
        B[i] = (int)clamp8((yy + tb) >> 14);
    }
}

// R, G, B (0..255) of pixels x0 .. x0 + 3: the RGB export's pixels4, unpacked
template <int CF, bool LINEAR>
__device__ __forceinline__ void rgb4(const TensorArgs& a, const Rows& r, int x0, int R[4], int G[4], int B[4]) {
    const uint32_t yv = load4(r.y, x0, a.stride[0]);
    int cb[4], cr[4];
    chroma4<CF, LINEAR>(r.cb, r.cb1, x0, a.stride[1], a.cw, cb);
    chroma4<CF, LINEAR>(r.cr, r.cr1, x0, a.stride[2], a.cw, cr);
    matrix4(a, yv, cb, cr, R, G, B);
}

// Line y of the frame for the field modes (include/mp2vg.h "Field modes"): L_{y & 1}[y] with the
// field chroma when `field_chroma`, else the progressive line.  Everything that depends on y is
// uniform over the workgroup: the chroma rows j, j1 and the vertical taps wv0, wv1 (eighths).
template <int CF, bool LINEAR>
__device__ __forceinline__ void line4(const TensorArgs& a, const uint8_t* const pl[3], int y, bool field_chroma, int x0,
                                      int R[4], int G[4], int B[4]) {
    int j = y, j1 = y, wv1 = 0;
    if (CF == 1) {
        if (field_chroma) {
            j = 2 * (y >> 2) + (y & 1);  // the chroma row of the same field
            j1 = (y & 2) ? j + 2 : j - 2;
            if (j1 < 0 || j1 > a.ch - 1) j1 = j;
            wv1 = (y & 3) == 1 || (y & 3) == 2 ? 3 : 1;
        } else {
            j = y >> 1;
            j1 = min(max(j + ((y & 1) ? 1 : -1), 0), a.ch - 1);
            wv1 = 2;  // (6 A + 2 B + 8) >> 4 = (3 A + B + 4) >> 3
        }
    }
    const uint32_t yv = load4(pl[0] + (size_t)y * a.stride[0], x0, a.stride[0]);
    int cb[4], cr[4];
    chroma4w<CF, LINEAR>(pl[1] + (size_t)j * a.stride[1], pl[1] + (size_t)j1 * a.stride[1], x0, a.stride[1], a.cw,
                         8 - wv1, wv1, cb);
    chroma4w<CF, LINEAR>(pl[2] + (size_t)j * a.stride[2], pl[2] + (size_t)j1 * a.stride[2], x0, a.stride[2], a.cw,
                         8 - wv1, wv1, cr);
    matrix4(a, yv, cb, cr, R, G, B);
}

__device__ __forceinline__ uint32_t pack4(const int v[4]) {
    return (uint32_t)v[0] | (uint32_t)v[1] << 8 | (uint32_t)v[2] << 16 | (uint32_t)v[3] << 24;
}

struct alignas(8) V4 {
    int16_t v[4];
};

// float32 to bfloat16 bits, round to nearest even (the value is never NaN: scale and bias are finite)
__device__ __forceinline__ uint16_t bf16_rne(float f) {
    uint32_t u = __float_as_uint(f);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

// FIELDS = false: every frame PROGRESSIVE (mp2vg_tensor_slots / mp2vg_tensor_planes); true: the
// frame's MP2VG_FIELD_* mode picks the row walk of the vertical pass.
// PLACED = true (with FIELDS = true only): out_w x out_h is a canvas, the tables are those of the
// picture's rectangle dst_w x dst_h in it and everything outside the rectangle is the pad colour.
// ITEMS = true (with FIELDS = true, PLACED = false only): frame f is item f of the launch; its
// slot, mode, rectangle origin, tables and mirror flag come from its record (tensor_kernel.h).
template <int CF, bool LINEAR, bool PACKED, int DTYPE, bool FIELDS, bool PLACED, bool ITEMS>
__global__ __launch_bounds__(256) void tensor_kernel(const TensorArgs a) {
    static_assert(FIELDS || !PLACED, "the placed kernel rides the field row walk");
    static_assert(!ITEMS || (FIELDS && !PLACED), "the items kernel rides the field row walk and is never placed");
    __shared__ alignas(8) int16_t lds[2][3][kTensorSegCols];
    const int tid = (int)threadIdx.x;
    const int oy = 2 * (int)blockIdx.y;         // output rows oy and, unless oy is the last, oy + 1
    const bool two = oy + 1 < a.out_h;
    const size_t f = blockIdx.z;
    // Items: the record is uniform over the workgroup, loaded once and kept scalar (readfirstlane, as
    // for the mode below), so the origin, the table pointers, hmax, vmax and the flip flag stay in
    // SGPRs.  A workgroup at or beyond its item's segment count (the grid has the launch's largest)
    // returns here, whole, so the barrier below stays uniform.
    const int32_t* rec = ITEMS ? a.items + (size_t)kItemWords * f : nullptr;
    auto item = [&](int k) { return __builtin_amdgcn_readfirstlane(rec[k]); };
    if (ITEMS && (int)blockIdx.x >= item(kItemNsegs)) return;
    const int i_src_x = ITEMS ? item(kItemSrcX) : 0, i_src_y = ITEMS ? item(kItemSrcY) : 0;
    const int i_hmax = ITEMS ? item(kItemHmax) : 0, i_vmax = ITEMS ? item(kItemVmax) : 0;
    const bool flip = ITEMS && (item(kItemFlags) & MP2VG_ITEM_HFLIP);
    const int plane0 = ITEMS ? item(kItemPlane) : 0;
    const int32_t* i_segs = ITEMS ? a.items + item(kItemSegs) : nullptr;
    const int32_t* i_hfirst = ITEMS ? a.items + item(kItemHfirst) : nullptr;
    const int32_t* i_hw = ITEMS ? a.items + item(kItemHw) : nullptr;
    const int32_t* i_vfirst = ITEMS ? a.items + item(kItemVfirst) : nullptr;
    const int32_t* i_vcount = ITEMS ? a.items + item(kItemVcount) : nullptr;
    const int32_t* i_vw = ITEMS ? a.items + item(kItemVw) : nullptr;
    // the record's value in the items kernel, else the argument, read where it is used (which keeps
    // the code of the other kernels as it was)
#define ARG(name) (ITEMS ? i_##name : a.name)
    const int32_t* seg = ARG(segs) + 4 * blockIdx.x;
    const int o_begin = seg[0], o_end = seg[1], base = seg[2], nunits = seg[3];
    const uint8_t* pl[3];
#pragma unroll
    for (int p = 0; p < 3; p++) {
        if (ITEMS)
            pl[p] = a.ftab ? (const uint8_t*)a.ftab[item(kItemSlot)] + a.plane_off[p] : a.planes[p];
        else
            pl[p] = a.slots ? (const uint8_t*)a.ftab[a.slots[f]] + a.plane_off[p] : a.planes[p];
    }

    // vertical pass over the union of the two rows' source rows (vfirst and the range ends never
    // decrease with the output row); a row outside one output row's taps has weight 0 there
    int f0, c0, f1, c1, nrows;
    const int32_t *qv0, *qv1;
    // placement (uniform over the workgroup): canvas row oy + t is a picture row (pic0 / pic1) when it
    // lies in the rectangle; its table row is then oy + t - dst_y.  A pair can be pad + picture or
    // picture + pad: the pad row has no taps (count 0, its first row the picture row's, so the
    // union is the picture row's range) and reads the weights of a row that exists.
    bool pic0 = true, pic1 = two;
    if (!PLACED) {
        f0 = ARG(vfirst)[oy], c0 = ARG(vcount)[oy];
        f1 = two ? ARG(vfirst)[oy + 1] : f0, c1 = two ? ARG(vcount)[oy + 1] : 0;
        nrows = max(f0 + c0, f1 + c1) - f0;
        qv0 = ARG(vw) + (size_t)oy * ARG(vmax);
        qv1 = qv0 + (two ? ARG(vmax) : 0);
    } else {
        const int r0 = oy - a.dst_y;
        pic0 = r0 >= 0 && r0 < a.dst_h;
        pic1 = two && r0 + 1 >= 0 && r0 + 1 < a.dst_h;
        const int ra = pic0 ? r0 : pic1 ? r0 + 1 : 0, rb = pic1 ? r0 + 1 : ra;  // rows inside the tables
        f0 = ARG(vfirst)[ra], c0 = pic0 ? ARG(vcount)[ra] : 0;
        f1 = pic1 ? ARG(vfirst)[rb] : f0, c1 = pic1 ? ARG(vcount)[rb] : 0;
        nrows = max(f0 + c0, f1 + c1) - f0;
        qv0 = ARG(vw) + (size_t)ra * ARG(vmax);
        qv1 = ARG(vw) + (size_t)rb * ARG(vmax);
    }
    // field modes (uniform over the workgroup).  WEAVE and PROGRESSIVE walk every row of the union
    // as above, with the line's own chroma siting.  TOP / BOTTOM (parity par) walk only the field's
    // lines z = z0, z0 + 2 .. z1: from the line above the first tap row when that row is an
    // interpolated one (unless it is row 0 of the frame: a = b, the average of the line with itself)
    // to the line below the last tap row (past the frame's last field line zmax it is that line
    // again: b = a).  Line z weighs in as row z, and its rounded average with the previous line,
    // formed as 8-bit values, as row z - 1; a row outside the union has weight 0.
    // (readfirstlane: the choice between the list and the argument is a vector load to the compiler;
    // as a scalar the mode keeps the walk's bounds, rows and weights in SGPRs)
    const int mode = !FIELDS ? MP2VG_FIELD_PROGRESSIVE
                : ITEMS ? item(kItemField)
                        : __builtin_amdgcn_readfirstlane(a.fields ? a.fields[f] : a.field);
    const bool single = mode == MP2VG_FIELD_TOP || mode == MP2VG_FIELD_BOTTOM;
    const int par = mode == MP2VG_FIELD_BOTTOM ? 1 : 0;
    const int Y0 = ARG(src_y) + f0, Yl = Y0 + nrows - 1;
    const int z0 = single ? max(Y0 - ((Y0 & 1) != par ? 1 : 0), par) : Y0;
    const int z1 = single ? Yl + ((Yl & 1) != par ? 1 : 0) : Yl;
    const int zmax = single ? a.coded_h - 2 + par : Yl;
    const int step = single ? 2 : 1;
    // weight of row k of the union for the two output rows: the loads are unconditional (the index
    // clamped into the row's vmax entries), so the scalar loads of one line issue together
    auto wt0 = [&](int k) {
        const int q = qv0[min(max(k, 0), ARG(vmax) - 1)];
        return k >= 0 && k < c0 ? q : 0;
    };
    auto wt1 = [&](int k) {
        const int q = qv1[min(max(k + f0 - f1, 0), ARG(vmax) - 1)];
        return k + f0 - f1 >= 0 && k + f0 - f1 < c1 ? q : 0;
    };
    // (a workgroup whose rows are both pad has no vertical pass; the barrier below stays uniform)
    for (int u = tid; u < (!PLACED || pic0 || pic1 ? nunits : 0); u += 256) {
        const int x0 = ARG(src_x) + base + 4 * u;
        int aR[2][4] = {}, aG[2][4] = {}, aB[2][4] = {};
        if (!FIELDS) {
            for (int k = 0; k < nrows; k++) {
                const int y = ARG(src_y) + f0 + k;
                Rows r;
                const int j = CF == 1 ? y >> 1 : y;
                const int j1 = CF == 1 && LINEAR ? min(max(j + ((y & 1) ? 1 : -1), 0), a.ch - 1) : j;
                r.y = pl[0] + (size_t)y * a.stride[0];
                r.cb = pl[1] + (size_t)j * a.stride[1];
                r.cr = pl[2] + (size_t)j * a.stride[2];
                r.cb1 = pl[1] + (size_t)j1 * a.stride[1];
                r.cr1 = pl[2] + (size_t)j1 * a.stride[2];
                int R[4], G[4], B[4];
                rgb4<CF, LINEAR>(a, r, x0, R, G, B);
                const int k1 = f0 + k - f1;
                const int q0 = k < c0 ? qv0[k] : 0;
                const int q1 = k1 >= 0 && k1 < c1 ? qv1[k1] : 0;
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    aR[0][i] += __mul24(q0, R[i]), aR[1][i] += __mul24(q1, R[i]);
                    aG[0][i] += __mul24(q0, G[i]), aG[1][i] += __mul24(q1, G[i]);
                    aB[0][i] += __mul24(q0, B[i]), aB[1][i] += __mul24(q1, B[i]);
                }
            }
        } else {
            uint32_t prev[3] = {0u, 0u, 0u};  // the previous field line, a dword of 4 pixels per channel
            for (int z = z0; z <= z1; z += step) {
                int R[4], G[4], B[4];
                line4<CF, LINEAR>(a, pl, min(z, zmax), mode != MP2VG_FIELD_PROGRESSIVE, x0, R, G, B);
                const int q0 = wt0(z - Y0), q1 = wt1(z - Y0);
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    aR[0][i] += __mul24(q0, R[i]), aR[1][i] += __mul24(q1, R[i]);
                    aG[0][i] += __mul24(q0, G[i]), aG[1][i] += __mul24(q1, G[i]);
                    aB[0][i] += __mul24(q0, B[i]), aB[1][i] += __mul24(q1, B[i]);
                }
                if (single) {
                    const uint32_t cur[3] = {pack4(R), pack4(G), pack4(B)};
                    if (z == z0) prev[0] = cur[0], prev[1] = cur[1], prev[2] = cur[2];
                    // v_lerp_u8: per byte (a + b + 1) >> 1
                    const uint32_t mr = __builtin_amdgcn_lerp(prev[0], cur[0], 0x01010101u);
                    const uint32_t mg = __builtin_amdgcn_lerp(prev[1], cur[1], 0x01010101u);
                    const uint32_t mb = __builtin_amdgcn_lerp(prev[2], cur[2], 0x01010101u);
                    const int m0 = wt0(z - Y0 - 1), m1 = wt1(z - Y0 - 1);
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        aR[0][i] += __mul24(m0, byte_of(mr, i)), aR[1][i] += __mul24(m1, byte_of(mr, i));
                        aG[0][i] += __mul24(m0, byte_of(mg, i)), aG[1][i] += __mul24(m1, byte_of(mg, i));
                        aB[0][i] += __mul24(m0, byte_of(mb, i)), aB[1][i] += __mul24(m1, byte_of(mb, i));
                    }
                    prev[0] = cur[0], prev[1] = cur[1], prev[2] = cur[2];
                }
            }
        }
#pragma unroll
        for (int t = 0; t < 2; t++) {
            V4 vr, vg, vb;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                vr.v[i] = (int16_t)((aR[t][i] + 128) >> 8);
                vg.v[i] = (int16_t)((aG[t][i] + 128) >> 8);
                vb.v[i] = (int16_t)((aB[t][i] + 128) >> 8);
            }
            *(V4*)&lds[t][0][4 * u] = vr;
            *(V4*)&lds[t][1][4 * u] = vg;
            *(V4*)&lds[t][2][4 * u] = vb;
        }
    }
    __syncthreads();

    // horizontal pass: one output element (row, pixel, channel) per lane
    const int nout = o_end - o_begin;
    const size_t w = (size_t)a.out_w, h = (size_t)a.out_h;
    // Placement: the canvas columns [xb, xe) of row oy + t this workgroup writes.  In a picture row
    // a segment writes its own picture columns, the first segment also the pad on their left and
    // the last one the pad on their right; a pad row is written whole by the first segment's
    // workgroup.  So every element of the canvas has exactly one writer.
    const int px0 = PLACED ? a.dst_x + o_begin : 0, px1 = PLACED ? a.dst_x + o_end : 0;
    int xb0 = 0, xb1 = 0, n0 = nout, n1 = two ? nout : 0;
    if (PLACED) {
        const bool first = blockIdx.x == 0, last = blockIdx.x + 1 == gridDim.x;
        const int xe = last ? a.out_w : px1;  // where a picture row of this workgroup ends
        xb0 = pic0 && !first ? px0 : 0;
        xb1 = pic1 && !first ? px0 : 0;
        n0 = pic0 ? xe - xb0 : first ? a.out_w : 0;
        n1 = pic1 ? xe - xb1 : first && two ? a.out_w : 0;
    }
    for (int idx = tid; idx < (PLACED ? 3 * (n0 + n1) : (two ? 6 : 3) * nout); idx += 256) {
        int t, c, o, Q;
        if (!PLACED) {
            t = idx >= 3 * nout ? 1 : 0;
            const int e = idx - 3 * nout * t;
            if (PACKED) {
                o = e / 3;
                c = e - 3 * o;
            } else {
                c = e >= 2 * nout ? 2 : e >= nout ? 1 : 0;
                o = e - c * nout;
            }
            o += o_begin;
        } else {
            t = idx >= 3 * n0 ? 1 : 0;
            const int e = idx - (t ? 3 * n0 : 0), nt = t ? n1 : n0;
            if (PACKED) {
                o = e / 3;
                c = e - 3 * o;
            } else {
                c = e >= 2 * nt ? 2 : e >= nt ? 1 : 0;
                o = e - c * nt;
            }
            o += t ? xb1 : xb0;  // the canvas column
        }
        if (!PLACED || ((t ? pic1 : pic0) && o >= px0 && o < px1)) {
            const int op = PLACED ? o - a.dst_x : o;  // the column of the tables
            // every lane runs the axis' longest tap count, so the loads of several taps are in flight:
            // the table's rows are zero from the column's tap count on, and a V index past the window is clamped (its
            // weight is zero, whatever the LDS holds there)
            const int16_t* v = &lds[t][c][0];
            const int v0 = ARG(hfirst)[op] - base;
            const int32_t* qh = ARG(hw) + (size_t)op * ARG(hmax);
            int sum = 8192;
#pragma unroll 4
            for (int k = 0; k < ARG(hmax); k++) sum += __mul24(qh[k], (int)v[min(v0 + k, kTensorSegCols - 1)]);
            Q = sum >> 14;
        } else {
            Q = c == 0 ? a.padq[0] : c == 1 ? a.padq[1] : a.padq[2];  // through the same normalise and cast below
        }
        const size_t y = (size_t)(oy + t);
        // Items: a flipped item's segment writes the mirrored run of columns (the mirror is an index
        // reversal behind both passes; every element still has exactly one writer), and the planar
        // address is the clip layout's: plane kItemPlane + c clip_len of h x w elements.
        const size_t ox = (size_t)(ITEMS && flip ? a.out_w - 1 - o : o);
        const size_t at = PACKED  ? ((f * h + y) * w + ox) * 3 + (size_t)c
                          : ITEMS ? ((size_t)(plane0 + c * a.clip_len) * h + y) * w + ox
                                  : ((f * 3 + (size_t)c) * h + y) * w + ox;
        if (DTYPE == MP2VG_TENSOR_U8) {
            ((uint8_t*)a.dst)[at] = (uint8_t)((Q + 32) >> 6);
        } else {
            const float sc = c == 0 ? a.scale[0] : c == 1 ? a.scale[1] : a.scale[2];
            const float bi = c == 0 ? a.bias[0] : c == 1 ? a.bias[1] : a.bias[2];
            const float x = __builtin_fmaf((float)Q * 0.015625f, sc, bi);  // Q / 64 is exact
            if (DTYPE == MP2VG_TENSOR_F32)
                ((float*)a.dst)[at] = x;
            else if (DTYPE == MP2VG_TENSOR_F16)
                ((_Float16*)a.dst)[at] = (_Float16)x;  // v_cvt_f16_f32: round to nearest even
            else
                ((uint16_t*)a.dst)[at] = bf16_rne(x);
        }
    }
}
#undef ARG

template <int CF, bool LINEAR, bool PACKED, bool FIELDS, bool PLACED, bool ITEMS = false>
static void launch_dtype(int dtype, const TensorArgs& a, dim3 grid, hipStream_t stream) {
    const dim3 block(256, 1, 1);
    if (dtype == MP2VG_TENSOR_U8)
        hipLaunchKernelGGL((tensor_kernel<CF, LINEAR, PACKED, MP2VG_TENSOR_U8, FIELDS, PLACED, ITEMS>), grid, block, 0, stream,
                           a);
    else if (dtype == MP2VG_TENSOR_F16)
        hipLaunchKernelGGL((tensor_kernel<CF, LINEAR, PACKED, MP2VG_TENSOR_F16, FIELDS, PLACED, ITEMS>), grid, block, 0, stream,
                           a);
    else if (dtype == MP2VG_TENSOR_BF16)
        hipLaunchKernelGGL((tensor_kernel<CF, LINEAR, PACKED, MP2VG_TENSOR_BF16, FIELDS, PLACED, ITEMS>), grid, block, 0,
                           stream, a);
    else
        hipLaunchKernelGGL((tensor_kernel<CF, LINEAR, PACKED, MP2VG_TENSOR_F32, FIELDS, PLACED, ITEMS>), grid, block, 0, stream,
                           a);
}

template <int CF, bool FIELDS, bool PLACED, bool ITEMS = false>
static void launch_cf(int layout, int chroma, int dtype, const TensorArgs& a, dim3 grid, hipStream_t stream) {
    const bool lin = chroma == MP2VG_EXPORT_CHROMA_LINEAR && CF != 3;  // 4:4:4: LINEAR is NEAREST
    if (layout == MP2VG_EXPORT_RGB_PACKED) {
        if (lin)
            launch_dtype<CF, CF != 3, true, FIELDS, PLACED, ITEMS>(dtype, a, grid, stream);
        else
            launch_dtype<CF, false, true, FIELDS, PLACED, ITEMS>(dtype, a, grid, stream);
    } else {
        if (lin)
            launch_dtype<CF, CF != 3, false, FIELDS, PLACED, ITEMS>(dtype, a, grid, stream);
        else
            launch_dtype<CF, false, false, FIELDS, PLACED, ITEMS>(dtype, a, grid, stream);
    }
}

// the three walks: without field modes, with them, and placed (which always has them)
template <int CF>
static void launch_walk(int layout, int chroma, int dtype, bool field_modes, bool placed, const TensorArgs& a, dim3 grid,
                        hipStream_t stream) {
    if (placed)
        launch_cf<CF, true, true>(layout, chroma, dtype, a, grid, stream);
    else if (field_modes)
        launch_cf<CF, true, false>(layout, chroma, dtype, a, grid, stream);
    else
        launch_cf<CF, false, false>(layout, chroma, dtype, a, grid, stream);
}

hipError_t launch_tensor(int cf, int layout, int chroma, int dtype, bool field_modes, bool placed, const TensorArgs& a,
                         int nsegs, int n, hipStream_t stream) {
    const dim3 grid((unsigned)nsegs, (unsigned)((a.out_h + 1) / 2), (unsigned)n);
    if (cf == 1)
        launch_walk<1>(layout, chroma, dtype, field_modes, placed, a, grid, stream);
    else if (cf == 2)
        launch_walk<2>(layout, chroma, dtype, field_modes, placed, a, grid, stream);
    else
        launch_walk<3>(layout, chroma, dtype, field_modes, placed, a, grid, stream);
    return hipGetLastError();
}

hipError_t launch_tensor_items(int cf, int layout, int chroma, int dtype, const TensorArgs& a, int nsegs, int n,
                               hipStream_t stream) {
    const dim3 grid((unsigned)nsegs, (unsigned)((a.out_h + 1) / 2), (unsigned)n);
    if (cf == 1)
        launch_cf<1, true, false, true>(layout, chroma, dtype, a, grid, stream);
    else if (cf == 2)
        launch_cf<2, true, false, true>(layout, chroma, dtype, a, grid, stream);
    else
        launch_cf<3, true, false, true>(layout, chroma, dtype, a, grid, stream);
    return hipGetLastError();
}

}  // namespace mp2vg
