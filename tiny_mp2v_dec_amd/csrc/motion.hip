// motion.hip — kernels of the compressed-domain export (include/mp2vg.h "motion export"): the
// resident MB records and coefficient words of a bank to the mv / info / act tensors, integer
// arithmetic only.  The per-record and per-word rules are motion_kernel.h's, shared with the host
// twin (motion.cpp).
//
// motion_mb_kernel: a plane is a flat array over a picture's records, so a thread owns kRun = 4
// adjacent cells: 8 loads of 16 bytes, then per plane 8 bytes of 16-bit values.  A plane starts
// on a 2-byte boundary when M is odd; the run's values then straddle dword boundaries, and each
// lane stores (previous lane's last value | its first), (second | third) and leaves its last value
// to the next lane: dword stores throughout, with 2-byte stores only at a wave's first and last
// cell and at the plane's tail.
//
// motion_act_kernel: one workgroup per (picture, MB row).  The row's words are one contiguous
// range (the upload contract, runtime.cpp plan_batch), streamed 16 bytes per lane; each word's MB
// is found by a search in the row's coef_off table in LDS and checked against that MB's own
// (coef_off, ncoef) range, so a word outside it is dropped and never indexes outside the row.
// A lane folds consecutive words of one (MB, block) before it touches the LDS counters.
#include <hip/hip_runtime.h>

#include "motion_kernel.h"

namespace mp2vg {

static constexpr int kThreads = 256;
static constexpr int kRun = 4;     // cells per thread of motion_mb_kernel
static constexpr int kTile = 256;  // MBs of a row per pass of motion_act_kernel (4096 / 16)

// the run of one plane: p = address of the thread's first cell, nv = its valid cells (0..4),
// v01 / v23 = the four 16-bit values in pairs
__device__ inline void store_run(uint16_t* p, int nv, uint32_t v01, uint32_t v23, int lane, bool next_has_cells) {
    if (((uintptr_t)p & 2) == 0) {  // uniform over the launch's threads of one plane
        if (nv == 4 && ((uintptr_t)p & 7) == 0) {
            *(uint2*)p = make_uint2(v01, v23);
            return;
        }
        if (nv >= 2) *(uint32_t*)p = v01;
        else if (nv == 1) p[0] = (uint16_t)v01;
        if (nv == 4) *(uint32_t*)(p + 2) = v23;
        else if (nv == 3) p[2] = (uint16_t)v23;
        return;
    }
    // every lane takes part in the shuffle, also those past the plane's end
    const uint32_t prev23 = __shfl_up(v23, 1);
    if (nv >= 1) {
        if (lane > 0) *(uint32_t*)(p - 1) = (prev23 >> 16) | (v01 << 16);  // the cells before are a full run
        else p[0] = (uint16_t)v01;
    }
    if (nv >= 3) *(uint32_t*)(p + 1) = (v01 >> 16) | (v23 << 16);
    else if (nv == 2) p[1] = (uint16_t)(v01 >> 16);
    if (nv == 4 && !(lane < 63 && next_has_cells)) p[3] = (uint16_t)(v23 >> 16);
}

__global__ __launch_bounds__(kThreads) void motion_mb_kernel(MotionArgs a) {
    const uint32_t M = (uint32_t)a.mbw * (uint32_t)a.mbh;
    const uint32_t f = blockIdx.z;
    const uint32_t cell0 = (blockIdx.x * kThreads + threadIdx.x) * kRun;
    const int nv = cell0 < M ? (int)min((uint32_t)kRun, M - cell0) : 0;
    const int lane = threadIdx.x & 63;
    const uint32_t mb_first = a.pics[a.order[f]].mb_first;
    const uint4* rec = (const uint4*)(a.mbs + (size_t)mb_first + cell0);
    uint32_t v[12][2];  // [channel: 8 mv, 4 info][pair of cells]
#pragma unroll
    for (int c = 0; c < 12; c++) v[c][0] = v[c][1] = 0;
#pragma unroll
    for (int k = 0; k < kRun; k++) {
        uint32_t r[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (k < nv) {
            const uint4 lo = rec[2 * k], hi = rec[2 * k + 1];
            r[0] = lo.x, r[1] = lo.y, r[2] = lo.z, r[3] = lo.w;
            r[4] = hi.x, r[5] = hi.y, r[6] = hi.z, r[7] = hi.w;
        }
        int16_t mv[8];
        uint16_t info[4];
        motion_mb(r, mv, info);
#pragma unroll
        for (int c = 0; c < 8; c++) v[c][k >> 1] |= (uint32_t)(uint16_t)mv[c] << (16 * (k & 1));
#pragma unroll
        for (int c = 0; c < 4; c++) v[8 + c][k >> 1] |= (uint32_t)info[c] << (16 * (k & 1));
    }
    const bool next = cell0 + kRun < M;
    if (a.mv) {
        uint16_t* p = (uint16_t*)a.mv + (size_t)f * 8 * M + cell0;
#pragma unroll
        for (int c = 0; c < 8; c++) store_run(p + (size_t)c * M, nv, v[c][0], v[c][1], lane, next);
    }
    if (a.info) {
        uint16_t* p = a.info + (size_t)f * 4 * M + cell0;
#pragma unroll
        for (int c = 0; c < 4; c++) store_run(p + (size_t)c * M, nv, v[8 + c][0], v[8 + c][1], lane, next);
    }
}

__global__ __launch_bounds__(kThreads) void motion_act_kernel(MotionArgs a) {
    __shared__ uint32_t s_start[kTile], s_end[kTile];
    __shared__ int32_t s_acc[2 * 12 * kTile];  // [plane][block][MB of the tile]
    __shared__ uint32_t s_lo, s_hi;
    const int nb = a.nb, mbw = a.mbw, tid = threadIdx.x;
    const size_t M = (size_t)mbw * a.mbh;
    const uint32_t y = blockIdx.x, f = blockIdx.z;
    const mp2vg_mb_t* row = a.mbs + (size_t)a.pics[a.order[f]].mb_first + (size_t)y * mbw;
    int32_t* out = a.act + (size_t)f * 2 * nb * M + (size_t)y * mbw;
    for (int j0 = 0; j0 < mbw; j0 += kTile) {
        const int tw = min(kTile, mbw - j0);
        if (tid == 0) s_lo = 0xffffffffu, s_hi = 0;
        for (int i = tid; i < 2 * nb * kTile; i += kThreads) s_acc[i] = 0;
        __syncthreads();
        if (tid < tw) {
            const uint4 lo = *(const uint4*)(row + j0 + tid);
            const uint32_t ncoef = lo.z >> 16, off = lo.w;
            s_start[tid] = off;
            s_end[tid] = off + ncoef;
            if (ncoef) {  // the row's range comes from the records that have words
                atomicMin(&s_lo, off);
                atomicMax(&s_hi, off + ncoef);
            }
        }
        __syncthreads();
        const uint32_t lo = s_lo, hi = s_hi;
        // a row (or a whole picture) without words loads nothing: lo > hi
        for (uint32_t w0 = (lo < hi ? (lo & ~3u) : hi) + 4u * tid; w0 < hi; w0 += 4u * kThreads) {
            const uint4 q = *(const uint4*)(a.coefs + w0);  // up to 3 words past hi: inside the bank's pad
            const uint32_t word[4] = {q.x, q.y, q.z, q.w};
            int key = -1, cj = 0;
            int32_t cnt = 0, sum = 0;
            uint32_t cs = 1, ce = 0;  // range of MB cj (empty: the first word searches)
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint32_t w = w0 + k;
                if (w < lo || w >= hi) continue;
                if (w < cs || w >= ce) {  // the last MB of the tile whose coef_off is <= w
                    int l = 0, h = tw;
                    while (l < h) {
                        const int mid = (l + h) >> 1;
                        if (s_start[mid] <= w) l = mid + 1;
                        else h = mid;
                    }
                    cj = max(l - 1, 0);
                    cs = s_start[cj], ce = s_end[cj];
                }
                if (w < cs || w >= ce) continue;  // a word no MB of the tile owns
                int b;
                int32_t mag;
                if (!motion_word(word[k], nb, &b, &mag)) continue;
                const int k2 = b * kTile + cj;
                if (k2 != key) {
                    if (key >= 0) {
                        atomicAdd(&s_acc[key], cnt);
                        atomicAdd(&s_acc[nb * kTile + key], sum);
                    }
                    key = k2, cnt = 0, sum = 0;
                }
                cnt++;
                sum += mag;
            }
            if (key >= 0) {
                atomicAdd(&s_acc[key], cnt);
                atomicAdd(&s_acc[nb * kTile + key], sum);
            }
        }
        __syncthreads();
        for (int i = tid; i < 2 * nb * tw; i += kThreads) {
            const int pb = i / tw, jj = i - pb * tw;
            out[(size_t)pb * M + j0 + jj] = s_acc[pb * kTile + jj];
        }
        __syncthreads();
    }
}

hipError_t launch_motion(const MotionArgs& a, int n, hipStream_t stream) {
    const uint32_t M = (uint32_t)a.mbw * (uint32_t)a.mbh;
    if (a.mv || a.info) {
        const uint32_t per = kThreads * kRun;
        hipLaunchKernelGGL(motion_mb_kernel, dim3((M + per - 1) / per, 1, n), dim3(kThreads), 0, stream, a);
        if (hipError_t e = hipGetLastError()) return e;
    }
    if (a.act) {
        hipLaunchKernelGGL(motion_act_kernel, dim3(a.mbh, 1, n), dim3(kThreads), 0, stream, a);
        if (hipError_t e = hipGetLastError()) return e;
    }
    return hipSuccess;
}

}  // namespace mp2vg
