// residual.hip — kernel of the residual export (include/mp2vg.h "residual export"): the resident MB
// records and coefficient words of a bank to int16 / int8 residual planes, integer arithmetic only.
// The per-word, per-block and placement rules are residual_kernel.h's, shared with the host twin
// (residual.cpp).
//
// One workgroup (4 waves) per (picture of the order list, MB row, tile of kTileMB = 8 MBs): LDS
// holds one 8 x 8 int16 slot per block of the tile (12 KB at 4:4:4), whatever the picture's width.
//   1. records, matrices and the scan table into LDS; every slot and parity cleared.
//   2. dequant: a wave takes MBs w, w + 4 of the tile, lane = coefficient word of the MB's own
//      (coef_off, ncoef) range (4-byte loads, nothing outside the range), filed by the word's block
//      index into its slot; the mismatch sum's parity is one LDS xor per odd value.
//   3. transform: lane = two lines of a coded block (4 lanes a block): mismatch toggle, pass 1 on
//      packed pairs, transpose through the slot (two 16-byte writes), pass 2, >> 6, clamp, back
//      into the slot as the block's rows.  Blocks that are not coded are skipped and stay zero.
//   4. store: lane = one 8-sample row piece of a plane (16 bytes int16, 8 bytes int8), read from
//      the slot the placement rule names, so zeros of uncoded blocks leave by the same pass and
//      every element of the tile has one writer.
#include <hip/hip_runtime.h>

#include "residual_kernel.h"

namespace mp2vg {

static constexpr int kThreads = 256;
static constexpr int kTileMB = 8;  // MBs of a row per workgroup

__constant__ uint8_t c_residual_scan[2][64] = MP2VG_RESIDUAL_SCAN;

// intra-wave LDS hand-off: the 4 lanes of a block sit in one wave
__device__ __forceinline__ void residual_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the tile's part of plane pl: PW = the plane's width in samples
template <int CF, int DT, int NB>
__device__ __forceinline__ void store_plane(const int16_t* s_blk, const uint32_t (*s_rec)[4], int pl, void* base,
                                            uint32_t f, uint32_t mby, uint32_t mx0, int mbw, int mbh, int tid) {
    const int MW = residual_mb_w(CF, pl) / 8, MH = residual_mb_h(CF, pl);
    const int cols = kTileMB * MW;
    const size_t PW = (size_t)mbw * MW * 8, PH = (size_t)mbh * MH;
    for (int it = tid; it < cols * MH; it += kThreads) {
        const int y = it / cols, xbt = it - y * cols;
        const int m = xbt / MW, xb = xbt - m * MW;
        if (mx0 + m >= (uint32_t)mbw) continue;
        const bool dctf = (s_rec[m][0] & MP2VG_MB_DCT_FIELD) != 0;
        int b, row;
        residual_source(CF, pl, y, xb, dctf, &b, &row);
        const uint4 v = *(const uint4*)(s_blk + (m * NB + b) * 64 + row * 8);
        const size_t e = ((size_t)f * PH + (size_t)mby * MH + y) * PW + (size_t)(mx0 + m) * MW * 8 + xb * 8;
        if (DT == MP2VG_RESIDUAL_I16) {
            *(uint4*)((int16_t*)base + e) = v;
        } else {  // the low bytes of the 8 clamped values
            *(uint2*)((int8_t*)base + e) = make_uint2(__builtin_amdgcn_perm(v.y, v.x, 0x06040200u),
                                                      __builtin_amdgcn_perm(v.w, v.z, 0x06040200u));
        }
    }
}

template <int CF, int DT>
__global__ __launch_bounds__(kThreads) void residual_kernel(ResidualArgs a) {
    constexpr int NB = CF == 1 ? 6 : (CF == 2 ? 8 : 12);
    constexpr int kSlots = kTileMB * NB;
    __shared__ __attribute__((aligned(16))) int16_t s_blk[kSlots * 64];
    __shared__ uint32_t s_par[kSlots];
    __shared__ uint32_t s_rec[kTileMB][4];  // flags | effective cbp << 16, qscale, ncoef, coef_off
    __shared__ __attribute__((aligned(4))) uint8_t s_W[4][64];
    __shared__ __attribute__((aligned(4))) uint8_t s_scan[64];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int mbw = a.mbw;
    const uint32_t mx0 = blockIdx.x * kTileMB, mby = blockIdx.y, f = blockIdx.z;
    const mp2vg_picture_t* pic = a.pics + a.order[f];

    // 1. the tile's records, the picture's tables, cleared slots
    if (tid < kTileMB) {
        uint32_t flags = 0, cbp = 0, qs = 0, ncoef = 0, off = 0;
        if (mx0 + tid < (uint32_t)mbw) {
            const uint4 r = *(const uint4*)(a.mbs + (size_t)pic->mb_first + (size_t)mby * mbw + mx0 + tid);
            flags = r.y & 0xffffu, cbp = (r.y >> 16) & ((1u << NB) - 1u);
            qs = r.z & 0xffu, ncoef = r.z >> 16, off = r.w;
            if ((a.flags & MP2VG_RESIDUAL_ZERO_INTRA) && (flags & MP2VG_MB_INTRA)) cbp = 0;
            if (!a.y) cbp &= ~15u;  // blocks of planes nobody wants are not transformed
            if (!a.cb) cbp &= 15u;
            if (!cbp) ncoef = 0;
        }
        s_rec[tid][0] = flags | cbp << 16, s_rec[tid][1] = qs, s_rec[tid][2] = ncoef, s_rec[tid][3] = off;
    } else if (tid >= 64 && tid < 128) {
        ((uint32_t*)s_W)[tid - 64] = ((const uint32_t*)pic->W)[tid - 64];
    } else if (tid >= 128 && tid < 144) {
        ((uint32_t*)s_scan)[tid - 128] = ((const uint32_t*)c_residual_scan[pic->alternate_scan ? 1 : 0])[tid - 128];
    }
    for (int i = tid; i < kSlots * 8; i += kThreads) ((uint4*)s_blk)[i] = make_uint4(0u, 0u, 0u, 0u);
    if (tid < kSlots) s_par[tid] = 0;
    __syncthreads();

    // 2. dequant: lane = word
    for (int m = wave; m < kTileMB; m += kThreads / 64) {
        const uint32_t fc = s_rec[m][0], cbp = fc >> 16;
        const int qs = (int)s_rec[m][1], ncoef = (int)s_rec[m][2];
        const bool intra = (fc & MP2VG_MB_INTRA) != 0;
        const uint32_t* words = a.coefs + s_rec[m][3];
        for (int j = lane; j < ncoef; j += 64) {
            const uint32_t w = words[j];
            const int b = (int)MP2VG_COEF_BLOCK(w);
            if (b >= NB || !(cbp >> b & 1u)) continue;
            int idx, val, par;
            residual_word(w, s_W[residual_matrix(b, intra)], qs, intra, s_scan, &idx, &val, &par);
            s_blk[(m * NB + b) * 64 + idx] = (int16_t)val;
            if (par) atomicXor(&s_par[m * NB + b], 1u);
        }
    }
    __syncthreads();

    // 3. transform: lane = lines 2c, 2c + 1 of a coded block
    for (int it = tid; it < kSlots * 4; it += kThreads) {
        const int slot = it >> 2, c = it & 3;
        const int m = slot / NB, b = slot - m * NB;
        if (!(s_rec[m][0] >> (16 + b) & 1u)) continue;  // the 4 lanes of a block agree
        uint32_t* blk = (uint32_t*)(s_blk + slot * 64);
        P16 s[8];
#pragma unroll
        for (int i = 0; i < 8; i++) s[i].v = __builtin_bit_cast(r_short2, blk[i * 4 + c]);
        // mismatch control: bit 0 of QFS[63] (row 7, column 7) toggles when the sum is even
        if (c == 3) s[7].v = __builtin_bit_cast(r_short2, __builtin_bit_cast(uint32_t, s[7].v) ^ (((s_par[slot] & 1u) ^ 1u) << 16));
        residual_idct_1d(s);
        // transpose: line 2c of the transposed block = the low halves of s[0..7], line 2c + 1 the high
        uint32_t lo[4], hi[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint32_t p = __builtin_bit_cast(uint32_t, s[2 * i].v), q = __builtin_bit_cast(uint32_t, s[2 * i + 1].v);
            lo[i] = __builtin_amdgcn_perm(q, p, 0x05040100u);
            hi[i] = __builtin_amdgcn_perm(q, p, 0x07060302u);
        }
        residual_wave_sync();  // every lane of the block has read its lines
        *(uint4*)(blk + (2 * c) * 4) = make_uint4(lo[0], lo[1], lo[2], lo[3]);
        *(uint4*)(blk + (2 * c + 1) * 4) = make_uint4(hi[0], hi[1], hi[2], hi[3]);
        residual_wave_sync();
#pragma unroll
        for (int i = 0; i < 8; i++) s[i].v = __builtin_bit_cast(r_short2, blk[i * 4 + c]);
        residual_idct_1d(s);
        residual_wave_sync();
        const r_short2 vlo = (r_short2)(short)residual_lo(DT), vhi = (r_short2)(short)residual_hi(DT);
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const r_short2 r = s[i].v >> (r_short2)(short)6;
            blk[i * 4 + c] = __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_elementwise_max(r, vlo), vhi));
        }
    }
    __syncthreads();

    // 4. store
    if (a.y) store_plane<CF, DT, NB>(s_blk, s_rec, 0, a.y, f, mby, mx0, mbw, a.mbh, tid);
    if (a.cb) {
        store_plane<CF, DT, NB>(s_blk, s_rec, 1, a.cb, f, mby, mx0, mbw, a.mbh, tid);
        store_plane<CF, DT, NB>(s_blk, s_rec, 2, a.cr, f, mby, mx0, mbw, a.mbh, tid);
    }
}

template <int CF>
static void launch_cf(const ResidualArgs& a, dim3 grid, hipStream_t stream) {
    if (a.dtype == MP2VG_RESIDUAL_I8)
        hipLaunchKernelGGL((residual_kernel<CF, MP2VG_RESIDUAL_I8>), grid, dim3(kThreads), 0, stream, a);
    else
        hipLaunchKernelGGL((residual_kernel<CF, MP2VG_RESIDUAL_I16>), grid, dim3(kThreads), 0, stream, a);
}

hipError_t launch_residual(const ResidualArgs& a, int n, hipStream_t stream) {
    const dim3 grid((a.mbw + kTileMB - 1) / kTileMB, a.mbh, n);
    if (a.cf == 1) launch_cf<1>(a, grid, stream);
    else if (a.cf == 2) launch_cf<2>(a, grid, stream);
    else launch_cf<3>(a, grid, stream);
    return hipGetLastError();
}

}  // namespace mp2vg
