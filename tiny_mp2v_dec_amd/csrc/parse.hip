// parse.hip — the record emitter as kernels (gfx950): elementary-stream slices in HBM -> MB
// records and coefficient words in HBM, where recon.hip reads them.
//
// Mapping: one lane per slice, workgroup = one wave of 64.  The accepted subset has exactly one
// slice per macroblock row, and the host scan has already given every slice its row, so lanes
// share nothing and no atomics are needed; slices are in stream order, so a wave's lanes are
// consecutive rows of one picture and their records are neighbours in memory.  The parser is
// slice_parse.h, the very source the CPU twin (mp2vg_scan_parse_host) runs.  Lanes diverge freely
// (a VLC parse is a data-dependent state machine); a wave costs what its slowest lane costs, and
// occupancy across the device's waves hides that, not any cooperation inside the wave.
//
// Two passes, for exact memory use: the count pass parses every slice, writes its records
// (coef_off relative to the slice) and its word count, status and reference usage; a one-
// workgroup scan turns the counts into each slice's first word (the layout of mp2vg_parse_es:
// slices concatenated in stream order); the emit pass parses again and writes the words there.
//
// Tables (about 90 KB: the 12-bit first level of both coefficient tables alone is 32 KB) stay in
// global memory and are read through the vector L1 / L2: a one-wave workgroup would have to fill
// an LDS copy per wave, more traffic than the handful of table lines a slice touches.
// Every memory access is a vector load or store.
#include <hip/hip_runtime.h>

#include "parse_kernel.h"

namespace mp2vg {

static __device__ __forceinline__ bool slice_ok(const ParseArgs& a, const DevSlice& s) {
    return s.pic < a.npics && s.mb_row < (uint32_t)a.G.mbh && s.byte_off <= s.byte_end && s.byte_end <= a.span;
}

__global__ __launch_bounds__(64) void parse_count_kernel(ParseArgs a) {
    const uint32_t j = blockIdx.x * 64u + threadIdx.x;
    if (j >= a.nslices) return;
    const DevSlice s = a.slices[j];
    SpResult r;
    if (!slice_ok(a, s)) {  // (the host builds the table; a bad entry touches nothing)
        r.status = MP2VG_E_INVALID, r.reason = 0, r.ncoef = 0, r.fail_pos = 0, r.uses = 0, r.iters = 0;
        a.res[j] = r;
        return;
    }
    const SpCountOut out{a.mbs + a.mb_first[s.pic] + (size_t)s.mb_row * a.G.mbw};
    sp_parse_slice(a.T, a.G, a.hdr[s.pic], a.bs, (int64_t)s.byte_off, (int64_t)s.byte_end, (int64_t)a.span,
                   (int)s.mb_row, out, r);
    a.res[j] = r;
}

// Exclusive prefix sum of the slices' word counts in table order -> base[], with
// summary[0] = the total (64-bit), summary[1] = the first failing slice (or 2^64 - 1), and the
// per-picture OR of the slices' reference usage.  One workgroup of kScanThreads lanes, each over
// a contiguous run of slices.
constexpr int kScanThreads = 1024;
__global__ __launch_bounds__(kScanThreads) void parse_scan_kernel(ParseArgs a, const uint32_t* pic_slice,
                                                                  unsigned long long* summary) {
    __shared__ unsigned long long sum[kScanThreads];
    __shared__ uint32_t bad[kScanThreads];
    const uint32_t t = threadIdx.x, n = a.nslices;
    const uint32_t chunk = (n + kScanThreads - 1) / kScanThreads;
    const uint32_t lo = min(n, t * chunk), hi = min(n, lo + chunk);
    unsigned long long s = 0;
    uint32_t fb = 0xffffffffu;
    for (uint32_t j = lo; j < hi; j++) {
        s += a.res[j].ncoef;
        if (a.res[j].status != MP2VG_OK && fb == 0xffffffffu) fb = j;
    }
    sum[t] = s;
    bad[t] = fb;
    __syncthreads();
    for (int d = 1; d < kScanThreads; d <<= 1) {  // inclusive scan of the runs' sums, min of the failures
        const unsigned long long v = t >= (uint32_t)d ? sum[t - d] : 0;
        const uint32_t b = t >= (uint32_t)d ? bad[t - d] : 0xffffffffu;
        __syncthreads();
        sum[t] += v;
        bad[t] = min(bad[t], b);
        __syncthreads();
    }
    unsigned long long at = sum[t] - s;
    for (uint32_t j = lo; j < hi; j++) {
        a.base[j] = (uint32_t)at;
        at += a.res[j].ncoef;
    }
    if (t == kScanThreads - 1) {
        a.base[n] = (uint32_t)sum[t];
        summary[0] = sum[t];
        summary[1] = bad[t] == 0xffffffffu ? ~0ull : (unsigned long long)bad[t];
    }
    for (uint32_t p = t; p < a.npics; p += kScanThreads) {
        uint32_t u = 0;
        for (uint32_t j = pic_slice[p]; j < pic_slice[p + 1] && j < n; j++) u |= a.res[j].uses;
        a.uses[p] = u;
    }
}

__global__ __launch_bounds__(64) void parse_emit_kernel(ParseArgs a) {
    const uint32_t j = blockIdx.x * 64u + threadIdx.x;
    if (j >= a.nslices) return;
    const DevSlice s = a.slices[j];
    if (!slice_ok(a, s)) return;
    const uint32_t base = a.base[j], cap = a.res[j].ncoef;
    if ((uint64_t)base + cap > a.base[a.nslices]) return;  // (never: base is the counts' prefix sum)
    const SpEmitOut out{a.mbs + a.mb_first[s.pic] + (size_t)s.mb_row * a.G.mbw, a.coefs + base, cap, base};
    SpResult r;
    sp_parse_slice(a.T, a.G, a.hdr[s.pic], a.bs, (int64_t)s.byte_off, (int64_t)s.byte_end, (int64_t)a.span,
                   (int)s.mb_row, out, r);
}

hipError_t launch_parse_count(const ParseArgs& a, hipStream_t stream) {
    if (!a.nslices) return hipSuccess;
    hipLaunchKernelGGL(parse_count_kernel, dim3((a.nslices + 63) / 64), dim3(64), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_parse_scan(const ParseArgs& a, const uint32_t* pic_slice, unsigned long long* summary,
                             hipStream_t stream) {
    hipLaunchKernelGGL(parse_scan_kernel, dim3(1), dim3(kScanThreads), 0, stream, a, pic_slice, summary);
    return hipGetLastError();
}

hipError_t launch_parse_emit(const ParseArgs& a, hipStream_t stream) {
    if (!a.nslices) return hipSuccess;
    hipLaunchKernelGGL(parse_emit_kernel, dim3((a.nslices + 63) / 64), dim3(64), 0, stream, a);
    return hipGetLastError();
}

}  // namespace mp2vg
