// export.hip — decoded frames to uint8 R'G'B' tensors on the device (gfx950 / CDNA4).
//
// One launch for a whole batch: strided planar Y'CbCr (frame-pool slots, or a caller's planes) in,
// tight full-range RGB out, cropped to the exported rectangle, planar [n][3][h][w] or packed
// [n][h][w][3].  The arithmetic is the bit-exact contract of include/mp2vg.h ("RGB export"):
// 14-bit fixed-point limited-range matrices, MPEG-2 progressive chroma siting, one rounding in the
// LINEAR chroma taps.  Interlaced (field) chroma siting is out of scope.
//
// Work split: a wave is 64 consecutive units of one output row, a workgroup 4 rows, the frame is
// blockIdx.z.  A unit is the 4 pixels whose output bytes fill whole aligned dwords: output rows
// are tight (w or 3w bytes), so every row (and in the planar layout every channel) starts at its
// own byte alignment a = address & 3, and unit u of a row covers pixels x0 .. x0 + 3 with
//   planar: x0 = 4u - a               one aligned dword per channel
//   packed: x0 = 4u - (3a & 3)        twelve bytes = three aligned dwords (3 x0 + a = 0 mod 4)
// Interior units store dwords (packed: one 12-byte store); only the first and the last unit of a
// row, which hang over its ends, fall back to byte stores for the up to 3 bytes of a dword that
// are inside the row.  The source is read at the unit's own x0 with unaligned dword loads (4
// luma bytes, and the 3-4 chroma samples the unit touches), clamped into the plane row.
// In the planar layout the three channels of a row share the unit when their alignments agree
// (always when w h is a multiple of 4); else the pixels are recomputed per channel.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mp2vg.h"
#include "export_kernel.h"
#include "export_pixels.h"

namespace mp2vg {

// the dword at aligned address p holds row bytes off .. off + 3 of a row of `rowbytes` bytes
__device__ __forceinline__ void store_clipped(uint8_t* p, int off, uint32_t v, int rowbytes) {
    if (off >= 0 && off + 4 <= rowbytes) {
        *(uint32_t*)p = v;
    } else {
#pragma unroll
        for (int i = 0; i < 4; i++)
            if ((unsigned)(off + i) < (unsigned)rowbytes) p[i] = (uint8_t)(v >> (8 * i));
    }
}

// R, G, B of pixels x0 .. x0 + 3, one byte per pixel in each dword
template <int CF, bool LINEAR>
__device__ __forceinline__ void pixels4(const ExportArgs& a, const Rows& r, int x0, uint32_t rgb[3]) {
    const uint32_t yv = load4(r.y, x0, a.stride[0]);
    int cb[4], cr[4];
    chroma4<CF, LINEAR>(r.cb, r.cb1, x0, a.stride[1], a.cw, cb);
    chroma4<CF, LINEAR>(r.cr, r.cr1, x0, a.stride[2], a.cw, cr);
    uint32_t R = 0, G = 0, B = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int yy = __mul24(a.cy, byte_of(yv, i));
        const int tr = __mul24(a.crv, cr[i]) + a.kr;
        const int tg = __mul24(a.cgu, cb[i]) + __mul24(a.cgv, cr[i]) + a.kg;
        const int tb = __mul24(a.cbu, cb[i]) + a.kb;
        R |= clamp8((yy + tr) >> 14) << (8 * i);
        G |= clamp8((yy + tg) >> 14) << (8 * i);
        B |= clamp8((yy + tb) >> 14) << (8 * i);
    }
    rgb[0] = R;
    rgb[1] = G;
    rgb[2] = B;
}

template <int CF, bool PACKED, bool LINEAR>
__global__ __launch_bounds__(256) void export_kernel(const ExportArgs a) {
    const int y = (int)(blockIdx.y * 4 + threadIdx.y);
    if (y >= a.h) return;
    const int u = (int)(blockIdx.x * 64 + threadIdx.x);
    const size_t f = blockIdx.z;
    const uint8_t* pl[3];
#pragma unroll
    for (int p = 0; p < 3; p++) pl[p] = a.slots ? (const uint8_t*)a.ftab[a.slots[f]] + a.plane_off[p] : a.planes[p];
    Rows r;
    const int j = CF == 1 ? y >> 1 : y;
    const int j1 = CF == 1 && LINEAR ? min(max(j + ((y & 1) ? 1 : -1), 0), a.ch - 1) : j;
    r.y = pl[0] + (size_t)y * a.stride[0];
    r.cb = pl[1] + (size_t)j * a.stride[1];
    r.cr = pl[2] + (size_t)j * a.stride[2];
    r.cb1 = pl[1] + (size_t)j1 * a.stride[1];
    r.cr1 = pl[2] + (size_t)j1 * a.stride[2];
    const size_t w = (size_t)a.w, h = (size_t)a.h;
    uint32_t rgb[3];
    if (PACKED) {
        uint8_t* row = a.dst + (f * h + (size_t)y) * 3 * w;
        const int al = (int)((uintptr_t)row & 3);
        const int x0 = 4 * u - ((3 * al) & 3);
        if (x0 >= a.w) return;
        pixels4<CF, LINEAR>(a, r, x0, rgb);
        // R0 G0 B0 R1 | G1 B1 R2 G2 | B2 R3 G3 B3
        const uint32_t d0 = __builtin_amdgcn_perm(rgb[2], __builtin_amdgcn_perm(rgb[1], rgb[0], 0x01000400u), 0x03040100u);
        const uint32_t d1 = __builtin_amdgcn_perm(rgb[2], __builtin_amdgcn_perm(rgb[1], rgb[0], 0x06020005u), 0x03020500u);
        const uint32_t d2 = __builtin_amdgcn_perm(rgb[2], __builtin_amdgcn_perm(rgb[1], rgb[0], 0x00070300u), 0x07020106u);
        const int off = 3 * x0, rowbytes = 3 * a.w;
        uint8_t* p = row + off;  // 4-byte aligned
        if (off >= 0 && off + 12 <= rowbytes) {
            struct alignas(4) D3 {
                uint32_t a, b, c;
            };
            *(D3*)p = D3{d0, d1, d2};
        } else {
            store_clipped(p, off, d0, rowbytes);
            store_clipped(p + 4, off + 4, d1, rowbytes);
            store_clipped(p + 8, off + 8, d2, rowbytes);
        }
    } else {
        int done = -1;  // the alignment rgb[] was computed for
#pragma unroll 1
        for (int c = 0; c < 3; c++) {
            uint8_t* row = a.dst + ((f * 3 + (size_t)c) * h + (size_t)y) * w;
            const int al = (int)((uintptr_t)row & 3);
            const int x0 = 4 * u - al;
            if (x0 >= a.w) continue;
            if (al != done) {
                pixels4<CF, LINEAR>(a, r, x0, rgb);
                done = al;
            }
            store_clipped(row + x0, x0, c == 0 ? rgb[0] : c == 1 ? rgb[1] : rgb[2], a.w);
        }
    }
}

template <int CF>
static void launch_cf(int layout, int chroma, const ExportArgs& a, dim3 grid, dim3 block, hipStream_t stream) {
    const bool lin = chroma == MP2VG_EXPORT_CHROMA_LINEAR && CF != 3;  // 4:4:4: LINEAR is NEAREST
    if (layout == MP2VG_EXPORT_RGB_PACKED) {
        if (lin)
            hipLaunchKernelGGL((export_kernel<CF, true, CF != 3>), grid, block, 0, stream, a);
        else
            hipLaunchKernelGGL((export_kernel<CF, true, false>), grid, block, 0, stream, a);
    } else {
        if (lin)
            hipLaunchKernelGGL((export_kernel<CF, false, CF != 3>), grid, block, 0, stream, a);
        else
            hipLaunchKernelGGL((export_kernel<CF, false, false>), grid, block, 0, stream, a);
    }
}

hipError_t launch_export(int cf, int layout, int chroma, const ExportArgs& a, int n, hipStream_t stream) {
    const int units = (a.w + 3) / 4 + 1;  // one more: a row that starts unaligned hangs over both ends
    const dim3 grid((unsigned)((units + 63) / 64), (unsigned)((a.h + 3) / 4), (unsigned)n), block(64, 4, 1);
    if (cf == 1)
        launch_cf<1>(layout, chroma, a, grid, block, stream);
    else if (cf == 2)
        launch_cf<2>(layout, chroma, a, grid, block, stream);
    else
        launch_cf<3>(layout, chroma, a, grid, block, stream);
    return hipGetLastError();
}

}  // namespace mp2vg
