// residual_kernel.h — the residual export (include/mp2vg.h "residual export"): the rule for one
// block, words -> QFS -> two saturating 16-bit passes -> >> 6 -> clamp, and the placement rule,
// compiled for the kernel (residual.hip) and for the host twin (residual.cpp:
// mp2vg_residual_records) alike, plus the launch arguments and the context's side (runtime.cpp).
//
// The transform is written once over a value type V with the four SSE2 operations of the
// reference's idct_sse2.hpp: the twin instantiates it with one int16 (R16), the kernel with a
// packed pair of int16 (two lines of a block per lane).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mp2vg.h"

#if defined(__HIPCC__)
#define RESIDUAL_HD __host__ __device__ inline
#else
#define RESIDUAL_HD inline
#endif

namespace mp2vg {

// scan position -> raster index (row = vertical frequency), zig-zag / alternate (ISO/IEC 13818-2
// 7.3); QFS is kept transposed, as the reference keeps it (the first pass runs over the
// horizontal frequencies): residual_qfs_index
#define MP2VG_RESIDUAL_SCAN                                                                          \
    {{0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,        \
      41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,        \
      30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63},               \
     {0,  8,  16, 24, 1,  9,  2,  10, 17, 25, 32, 40, 48, 56, 57, 49, 41, 33, 26, 18, 3,  11,        \
      4,  12, 19, 27, 34, 42, 50, 58, 35, 43, 51, 59, 20, 28, 5,  13, 6,  14, 21, 29, 36, 44,        \
      52, 60, 37, 45, 53, 61, 22, 30, 7,  15, 23, 31, 38, 46, 54, 62, 39, 47, 55, 63}}

RESIDUAL_HD int residual_qfs_index(int raster) { return ((raster & 7) << 3) | (raster >> 3); }

// the quantiser matrix of block b: W[residual_matrix(b, intra)] (blocks 4 and 5 use the luma pair)
RESIDUAL_HD int residual_matrix(int b, bool intra) { return (b < 6 ? 0 : 2) + (intra ? 0 : 1); }

// One coefficient word of a coded block: *idx = the QFS element it sets, *val = its value, *par =
// what it adds to the mismatch sum's parity (0 or 1).  W = the block's matrix in scan order, scan =
// the picture's scan table (64 raster indices).
RESIDUAL_HD void residual_word(uint32_t w, const uint8_t* W, int qs, bool intra, const uint8_t* scan, int* idx,
                               int* val, int* par) {
    const int level = (int16_t)(w & 0xffffu);
    const int i = (int)MP2VG_COEF_POS(w);
    if (w & MP2VG_COEF_DC) {  // the final QFS[0], outside the sum
        *idx = 0, *val = level, *par = 0;
        return;
    }
    const int mag = level < 0 ? -level : level;
    int v;
    if (w & MP2VG_COEF_FIRST1S) {  // unclamped, at position i itself (0 from a parser)
        v = (int16_t)((3 * (int)W[i] * qs) >> 5);
        v = level < 0 ? -v : v;
        *idx = i;
    } else {
        v = intra ? (mag * (int)W[i] * qs) >> 4 : ((2 * mag + 1) * (int)W[i] * qs) >> 5;
        v = (int16_t)(level < 0 ? -v : v);  // truncation to int16 before the clamp
        v = v > 2047 ? 2047 : (v < -2048 ? -2048 : v);
        *idx = residual_qfs_index(scan[i]);
    }
    *val = v;
    *par = v & 1;
}

// ---- the four operations on one int16 (the twin) -------------------------------------------
struct R16 {
    int16_t v;
};
RESIDUAL_HD int16_t r16_sat(int32_t x) { return (int16_t)(x > 32767 ? 32767 : (x < -32768 ? -32768 : x)); }
RESIDUAL_HD R16 r_adds(R16 a, R16 b) { return R16{r16_sat((int32_t)a.v + b.v)}; }
RESIDUAL_HD R16 r_subs(R16 a, R16 b) { return R16{r16_sat((int32_t)a.v - b.v)}; }
RESIDUAL_HD R16 r_mulhi(R16 a, int c) { return R16{(int16_t)(((int32_t)a.v * c) >> 16)}; }
RESIDUAL_HD R16 r_shl(R16 a, int n) { return R16{(int16_t)(uint16_t)((uint32_t)(uint16_t)a.v << n)}; }

#if defined(__HIPCC__)
// ---- the same on a packed pair (the kernel): saturating packed adds, wrapping packed shift, two
// 32-bit products whose high halves one byte permute joins
typedef short r_short2 __attribute__((ext_vector_type(2)));
typedef unsigned short r_ushort2 __attribute__((ext_vector_type(2)));
struct P16 {
    r_short2 v;
};
__device__ __forceinline__ P16 r_adds(P16 a, P16 b) { return P16{__builtin_elementwise_add_sat(a.v, b.v)}; }
__device__ __forceinline__ P16 r_subs(P16 a, P16 b) { return P16{__builtin_elementwise_sub_sat(a.v, b.v)}; }
__device__ __forceinline__ P16 r_mulhi(P16 a, int c) {
    const uint32_t u = __builtin_bit_cast(uint32_t, a.v);
    const int lo = (int)(int16_t)(u & 0xffffu) * c, hi = ((int)u >> 16) * c;
    return P16{__builtin_bit_cast(r_short2, __builtin_amdgcn_perm((uint32_t)hi, (uint32_t)lo, 0x07060302u))};
}
__device__ __forceinline__ P16 r_shl(P16 a, int n) {
    return P16{__builtin_bit_cast(r_short2, __builtin_bit_cast(r_ushort2, a.v) << (unsigned short)n)};
}
#endif

// One 8-point pass of the reference's 16-bit transform (idct_sse2.hpp:23-65): adds / subs
// saturate, the shift wraps, mulhi is (a * c) >> 16.
template <class V>
RESIDUAL_HD void residual_idct_1d(V s[8]) {
    const V v15 = r_adds(r_shl(r_mulhi(s[0], 27145), 1), r_shl(s[0], 1));
    const V v26 = r_adds(r_mulhi(s[1], -5037), r_shl(s[1], 2));
    const V v21 = r_adds(r_mulhi(s[2], -19954), r_shl(s[2], 2));
    const V v28 = r_adds(r_shl(r_mulhi(s[3], -22089), 1), r_shl(s[3], 2));
    const V v16 = r_adds(r_shl(r_mulhi(s[4], 27145), 1), r_shl(s[4], 1));
    const V v25 = r_adds(r_mulhi(s[5], 14567), r_shl(s[5], 1));
    const V v22 = r_adds(r_shl(r_mulhi(s[6], 17391), 1), s[6]);
    const V v27 = r_shl(r_mulhi(s[7], 25570), 1);
    const V v19 = r_subs(v25, v28);
    const V v20 = r_subs(v26, v27);
    const V v23 = r_adds(v26, v27);
    const V v24 = r_adds(v25, v28);
    const V v7 = r_adds(v23, v24);
    const V v11 = r_adds(v21, v22);
    const V v13 = r_subs(v23, v24);
    const V v17 = r_subs(v21, v22);
    const V v8 = r_adds(v15, v16);
    const V v9 = r_subs(v15, v16);
    const V v18 = r_mulhi(r_subs(v19, v20), 25079);
    const V v12 = r_subs(v18, r_adds(v19, r_mulhi(v19, 20090)));
    const V v14 = r_subs(r_subs(v20, r_mulhi(v20, 30068)), v18);
    const V v6 = r_subs(r_shl(v14, 1), v7);
    const V v5 = r_subs(r_adds(v13, r_mulhi(v13, 27145)), v6);
    const V v4 = r_adds(v5, r_shl(v12, 1));
    const V v10 = r_subs(r_adds(v17, r_mulhi(v17, 27145)), v11);
    const V v0 = r_adds(v8, v11);
    const V v1 = r_adds(v9, v10);
    const V v2 = r_subs(v9, v10);
    const V v3 = r_subs(v8, v11);
    s[0] = r_adds(v0, v7);
    s[1] = r_adds(v1, v6);
    s[2] = r_adds(v2, v5);
    s[3] = r_subs(v3, v4);
    s[4] = r_adds(v3, v4);
    s[5] = r_subs(v2, v5);
    s[6] = r_subs(v1, v6);
    s[7] = r_subs(v0, v7);
}

// the exported value of r = idct >> 6
RESIDUAL_HD int residual_lo(int dtype) { return dtype == MP2VG_RESIDUAL_I8 ? -128 : -255; }
RESIDUAL_HD int residual_hi(int dtype) { return dtype == MP2VG_RESIDUAL_I8 ? 127 : 255; }

// Placement, read from the plane's side: the 8 samples of plane pl (0 Y, 1 Cb, 2 Cr) at line y of
// the MB and 8-sample column xb are line *row of block *b (the decode's block placement,
// mb_decoder.cpp:166-196, inverted).  cf = chroma format, dctf = MP2VG_MB_DCT_FIELD.
RESIDUAL_HD void residual_source(int cf, int pl, int y, int xb, bool dctf, int* b, int* row) {
    if (pl == 0 || cf != 1) {  // 16 lines: two blocks above each other, or interleaved
        const int lower = dctf ? (y & 1) : (y >> 3);
        *row = dctf ? (y >> 1) : (y & 7);
        *b = pl == 0 ? xb + 2 * lower : 4 + (pl - 1) + 2 * lower + 4 * xb;
    } else {  // 4:2:0 chroma: one block, never interleaved
        *row = y;
        *b = 4 + (pl - 1);
    }
}

// MB size of plane pl in samples
RESIDUAL_HD int residual_mb_w(int cf, int pl) { return pl == 0 || cf == 3 ? 16 : 8; }
RESIDUAL_HD int residual_mb_h(int cf, int pl) { return pl == 0 || cf != 1 ? 16 : 8; }

// One launch exports n pictures of the resident bank: picture f is pics[order[f]].  Planes as
// mp2vg.h lays them out, elements of 2 bytes (I16) or 1 (I8); y, or cb and cr, may be null.
struct ResidualArgs {
    const mp2vg_picture_t* pics;
    const mp2vg_mb_t* mbs;
    const uint32_t* coefs;  // only words of an MB's own (coef_off, ncoef) range are loaded
    const int32_t* order;   // n device entries, each inside the bank's pictures
    int32_t mbw, mbh, cf;
    int32_t dtype, flags;
    void *y, *cb, *cr;
};
// grid = (row tiles, MB rows, n): one kernel of the (chroma format, dtype) template
hipError_t launch_residual(const ResidualArgs& a, int n, hipStream_t stream);

// the context's side (runtime.cpp), beside motion_begin / motion_enqueued and with their ordering:
// the main stream waits for the bank's `uploaded`; `consumed` is recorded before anything that
// can fail.  The bank itself is motion_source's.
int residual_begin(mp2vg_ctx* c);
int residual_enqueued(mp2vg_ctx* c);

}  // namespace mp2vg
