// export_pixels.h -- device primitives shared by the kernels that read decoded planes as R'G'B'
// (export.hip, tensor.hip): unaligned dword loads clamped into a plane row, the 8-bit clamp and the
// per-pixel chroma of the RGB export's contract (include/mp2vg.h "RGB export").
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mp2vg {

// bytes row[x .. x + 3] as a little-endian dword; positions outside [0, stride) read as garbage
// or zero (their pixels are never stored).  -3 <= x < stride.  (A second, clamp-free path for the
// interior units of a row measured slower: 1.09 against 0.82 ms for 256 planar 1080p frames.)
__device__ __forceinline__ uint32_t load4(const uint8_t* __restrict__ row, int x, int stride) {
    const int xl = min(max(x, 0), stride - 4);
    struct __attribute__((packed)) U32 {
        uint32_t v;
    };  // one global_load_dword at any byte address
    uint32_t v = ((const __attribute__((address_space(1))) U32*)(uintptr_t)(row + xl))->v;
    const int d = xl - x;
    if (d > 0) v <<= 8 * d;
    if (d < 0) v >>= -8 * d;
    return v;
}

__device__ __forceinline__ int byte_of(uint32_t v, int i) { return (int)((v >> (8 * i)) & 255u); }

// clamp to 0..255.  The empty asm keeps the value opaque to instruction selection, which otherwise
// fuses shift + clamp + byte pack of a pixel pair into v_ashr_pk_u8_i32 and then ORs bytes 2 and 3
// into that result as if its upper half were zero: on the MI355X it is not (bytes 2 and 3 came
// out wrong), so the pack is kept as med3 + shift + or.
__device__ __forceinline__ uint32_t clamp8(int v) {
    uint32_t c = (uint32_t)min(max(v, 0), 255);
    asm("" : "+v"(c));
    return c;
}

struct Rows {
    const uint8_t *y, *cb, *cr;    // luma row, chroma row j
    const uint8_t *cb1, *cr1;      // chroma row j1 (4:2:0 LINEAR)
};

// per-pixel chroma of pixels x0 .. x0 + 3 of one chroma plane, 8-bit each
template <int CF, bool LINEAR>
__device__ __forceinline__ void chroma4(const uint8_t* __restrict__ rj, const uint8_t* __restrict__ rj1, int x0,
                                        int stride, int cw, int c[4]) {
    if (CF == 3) {
        const uint32_t v = load4(rj, x0, stride);
#pragma unroll
        for (int i = 0; i < 4; i++) c[i] = byte_of(v, i);
        return;
    }
    const int c0 = x0 >> 1;  // first sample the unit touches (co-sited with even luma)
    const bool odd = x0 & 1;
    if (!LINEAR) {
        // pixel i takes sample (i + odd) >> 1
        const uint32_t v = __builtin_amdgcn_perm(0u, load4(rj, c0, stride), odd ? 0x02010100u : 0x01010000u);
#pragma unroll
        for (int i = 0; i < 4; i++) c[i] = byte_of(v, i);
        return;
    }
    // vertical taps first (4:2:0: 3 C[j] + C[j1]; else 4 C[j]), then the horizontal pair sum:
    // (wv0 (C[j][k] + C[j][k1]) + wv1 (C[j1][k] + C[j1][k1]) + 4) >> 3, one rounding
    const uint32_t va = load4(rj, c0, stride);
    const uint32_t vb = CF == 1 ? load4(rj1, c0, stride) : 0u;
    // (scalars, not an indexed array: the compiler stages a runtime-selected array through LDS)
    const int s0 = CF == 1 ? 3 * byte_of(va, 0) + byte_of(vb, 0) : 4 * byte_of(va, 0);
    int s1 = CF == 1 ? 3 * byte_of(va, 1) + byte_of(vb, 1) : 4 * byte_of(va, 1);
    int s2 = CF == 1 ? 3 * byte_of(va, 2) + byte_of(vb, 2) : 4 * byte_of(va, 2);
    if (c0 + 1 > cw - 1) s1 = s0;  // k1 clamps to the coded chroma plane
    if (c0 + 2 > cw - 1) s2 = s1;
    // pixel i sits on sample (i + odd) >> 1 when x0 + i is even, else between it and the next
    const int a01 = s0 + s1, a12 = s1 + s2;
    c[0] = ((odd ? a01 : 2 * s0) + 4) >> 3;
    c[1] = ((odd ? 2 * s1 : a01) + 4) >> 3;
    c[2] = ((odd ? a12 : 2 * s1) + 4) >> 3;
    c[3] = ((odd ? 2 * s2 : a12) + 4) >> 3;
}

// chroma4 with the vertical taps as arguments, wv0 + wv1 = 8 (the tensor export's field modes,
// include/mp2vg.h): (wv0 (C[j][k] + C[j][k1]) + wv1 (C[j1][k] + C[j1][k1]) + 8) >> 4, one rounding.
// wv0, wv1 = 6, 2 is chroma4's 4:2:0 result and 8, 0 its 4:2:2 result, bit for bit.  NEAREST and
// 4:4:4 have no taps: chroma4.
template <int CF, bool LINEAR>
__device__ __forceinline__ void chroma4w(const uint8_t* __restrict__ rj, const uint8_t* __restrict__ rj1, int x0,
                                         int stride, int cw, int wv0, int wv1, int c[4]) {
    if (CF == 3 || !LINEAR) {
        chroma4<CF, LINEAR>(rj, rj1, x0, stride, cw, c);
        return;
    }
    const int c0 = x0 >> 1;
    const bool odd = x0 & 1;
    const uint32_t va = load4(rj, c0, stride);
    const uint32_t vb = CF == 1 ? load4(rj1, c0, stride) : 0u;
    const int s0 = CF == 1 ? __mul24(wv0, byte_of(va, 0)) + __mul24(wv1, byte_of(vb, 0)) : 8 * byte_of(va, 0);
    int s1 = CF == 1 ? __mul24(wv0, byte_of(va, 1)) + __mul24(wv1, byte_of(vb, 1)) : 8 * byte_of(va, 1);
    int s2 = CF == 1 ? __mul24(wv0, byte_of(va, 2)) + __mul24(wv1, byte_of(vb, 2)) : 8 * byte_of(va, 2);
    if (c0 + 1 > cw - 1) s1 = s0;  // k1 clamps to the coded chroma plane
    if (c0 + 2 > cw - 1) s2 = s1;
    const int a01 = s0 + s1, a12 = s1 + s2;
    c[0] = ((odd ? a01 : 2 * s0) + 8) >> 4;
    c[1] = ((odd ? 2 * s1 : a01) + 8) >> 4;
    c[2] = ((odd ? a12 : 2 * s1) + 8) >> 4;
    c[3] = ((odd ? 2 * s2 : a12) + 8) >> 4;
}

}  // namespace mp2vg
