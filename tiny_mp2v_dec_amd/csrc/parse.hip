// parse.hip — the record emitter as kernels (gfx950): elementary-stream slices in HBM -> MB
// records and coefficient words in HBM, where recon.hip reads them.
//
// Mapping: one lane per slice, workgroup = one wave of 64.  The host scan has already given every
// slice its row, and a slice writes the records of its own columns [x0, x1) of that row (the whole
// row without MP2VG_PARSE_SLICES, where a row has exactly one slice), so the lanes of a valid stream
// share nothing and no atomics are needed; slices are in stream order, so a wave's lanes are
// consecutive rows (or parts of rows) of one picture and their records are neighbours in memory.
// Under MP2VG_PARSE_SLICES two slices that wrongly overlap may both store to one record; the row
// kernel then refuses or replaces that row, so what the record holds does not matter.  The parser is
// slice_parse.h, the very source the CPU twin (mp2vg_scan_parse_host) runs.  Lanes diverge freely
// (a VLC parse is a data-dependent state machine); a wave costs what its slowest lane costs, and
// occupancy across the device's waves hides that, not any cooperation inside the wave.
//
// Two passes, for exact memory use: the count pass parses every slice, writes its records
// (coef_off relative to the slice) and its word count, status and reference usage; a one-
// workgroup scan turns the counts into each slice's first word (the layout of mp2vg_parse_es:
// slices concatenated in stream order); the emit pass parses again and writes the words there.
// Under MP2VG_PARSE_SLICES a row is a run of table entries: a small kernel after the count pass
// applies the cover rule to every run (sp_cover_row) and marks what breaks it.
// Under MP2VG_PARSE_CONCEAL a small kernel between the count pass and the scan replaces the rows
// of failed slices and of missing rows (sp_conceal_row, the one statement of the rule); the scan
// counts them instead of reporting them, and the emit pass writes their words without parsing.
//
// Tables (about 90 KB: the 12-bit first level of both coefficient tables alone is 32 KB) stay in
// global memory and are read through the vector L1 / L2: a one-wave workgroup would have to fill
// an LDS copy per wave, more traffic than the handful of table lines a slice touches.
// Every memory access is a vector load or store.
#include <hip/hip_runtime.h>

#include "parse_kernel.h"

namespace mp2vg {

// a table entry the kernels may follow: inside the batch and the span.  An empty entry
// (byte_off == byte_end) is a missing row, which only a scan under MP2VG_PARSE_CONCEAL adds.
static __device__ __forceinline__ bool entry_ok(const ParseArgs& a, const DevSlice& s) {
    return s.pic < a.npics && s.mb_row < (uint32_t)a.G.mbh && s.byte_off <= s.byte_end && s.byte_end <= a.span;
}
// ... and holds a slice to parse
static __device__ __forceinline__ bool slice_ok(const ParseArgs& a, const DevSlice& s) {
    return s.pic < a.npics && s.mb_row < (uint32_t)a.G.mbh && s.byte_off < s.byte_end && s.byte_end <= a.span;
}

__global__ __launch_bounds__(64) void parse_count_kernel(ParseArgs a) {
    const uint32_t j = blockIdx.x * 64u + threadIdx.x;
    if (j >= a.nslices) return;
    const DevSlice s = a.slices[j];
    SpResult r;
    if (!slice_ok(a, s)) {  // (the host builds the table; a bad entry touches nothing, nor does an empty one)
        r.status = MP2VG_E_INVALID, r.reason = 0, r.ncoef = 0, r.fail_pos = 0, r.uses = 0, r.iters = 0;
        r.x0 = 0, r.x1 = 0, r.fate = SP_FATE_PARSED, r.pad = 0, r.blame = 0;
        a.res[j] = r;
        return;
    }
    const SpCountOut out{a.mbs + a.mb_first[s.pic] + (size_t)s.mb_row * a.G.mbw};
    sp_parse_slice(a.T, a.G, a.hdr[s.pic], a.bs, (int64_t)s.byte_off, (int64_t)s.byte_end, (int64_t)a.span,
                   (int)s.mb_row, out, r);
    r.x0 = 0, r.fate = SP_FATE_PARSED, r.pad = 0, r.blame = 0;  // (the row pass's fields)
    a.res[j] = r;
}

// MP2VG_PARSE_SLICES, after the count pass and before the conceal kernel and the scan, in two
// launches.  Phase 0: every lane reads its slice's start column again (sp_slice_x0: a header and one
// code; carrying the column through the count kernel's macroblock loop cost that kernel 30 SGPR
// spills) and stores it in res[j].x0.  Phase 1: the lane of each row's first entry walks the row's
// run of entries (consecutive in the table) and applies the cover rule (sp_cover_row, the one
// statement): a cover failure goes into the blamed entry's status and reason, where the scan finds
// it as it finds a parse failure; under MP2VG_PARSE_CONCEAL the
// first entry becomes the row's carrier, which the conceal kernel fills like any failed slice, and
// the others are dropped.  Every other lane returns at once.  A kernel of its own, launched under
// the flag only, as the conceal kernel is and for its reason: the count and emit passes with the
// flag clear are to be what they were.  An empty entry (a missing row) is a run of one and is left
// to the conceal kernel; a bad entry ends a run, and res[] of a run is only ever touched by its
// first lane, so the lanes share nothing.
__global__ __launch_bounds__(64) void parse_rows_kernel(ParseArgs a, int phase) {
    const uint32_t j = blockIdx.x * 64u + threadIdx.x;
    if (j >= a.nslices) return;
    const DevSlice s = a.slices[j];
    if (!slice_ok(a, s)) return;
    if (phase == 0) {
        a.res[j].x0 = (uint16_t)sp_slice_x0(a.T, a.G, a.bs, (int64_t)s.byte_off, (int64_t)s.byte_end, (int64_t)a.span);
        return;
    }
    if (j > 0) {
        const DevSlice q = a.slices[j - 1];
        if (q.pic == s.pic && q.mb_row == s.mb_row && slice_ok(a, q)) return;  // not the row's first entry
    }
    uint32_t n = 1;
    for (; j + n < a.nslices; n++) {
        const DevSlice q = a.slices[j + n];
        if (q.pic != s.pic || q.mb_row != s.mb_row || !slice_ok(a, q)) break;
    }
    sp_cover_row(a.res + j, n, a.G.mbw, a.conceal != 0);
}

// MP2VG_PARSE_CONCEAL, between the count pass and the scan: a lane whose slice failed for a
// slice-level reason, or whose row has no slice, overwrites its whole row with the replacement
// records (sp_conceal_row) and sets ncoef and uses to the replacement row's; status, reason and
// fail_pos stay in res[j] as the record of the damage.  A kernel of its own, launched under the
// flag only: inside the count kernel the call cost the parser's loop registers (28 more SGPR
// spills inline, scratch out of line), and the count pass is to be what it was with the flag clear.
__global__ __launch_bounds__(64) void parse_conceal_kernel(ParseArgs a) {
    const uint32_t j = blockIdx.x * 64u + threadIdx.x;
    if (j >= a.nslices) return;
    const DevSlice s = a.slices[j];
    if (!entry_ok(a, s)) return;
    SpResult r = a.res[j];
    if (s.byte_off == s.byte_end)  // a missing row: the count pass left it as a bad entry
        r.status = MP2VG_E_UNSUPPORTED, r.reason = SP_R_ROW_UNCOVERED;
    if (r.status == MP2VG_OK || !sp_reason_concealed(r.reason)) return;
    const SpCountOut out{a.mbs + a.mb_first[s.pic] + (size_t)s.mb_row * a.G.mbw};
    r.ncoef = sp_conceal_row(a.G, a.hdr[s.pic], (int)s.mb_row, out, r.uses);
    a.res[j] = r;
}

// Exclusive prefix sum of the slices' word counts in table order -> base[], with
// summary[0] = the total (64-bit), summary[1] = the first failing slice that is not concealed (or
// 2^64 - 1), summary[2] = the number of concealed slices, and the per-picture OR of the slices'
// reference usage (bit 2: the picture has a concealed row).  One workgroup of kScanThreads lanes,
// each over a contiguous run of slices.
constexpr int kScanThreads = 1024;
__global__ __launch_bounds__(kScanThreads) void parse_scan_kernel(ParseArgs a, const uint32_t* pic_slice,
                                                                  unsigned long long* summary) {
    __shared__ unsigned long long sum[kScanThreads];
    __shared__ uint32_t bad[kScanThreads];
    __shared__ uint32_t dmg[kScanThreads];
    const uint32_t t = threadIdx.x, n = a.nslices;
    const uint32_t chunk = (n + kScanThreads - 1) / kScanThreads;
    const uint32_t lo = min(n, t * chunk), hi = min(n, lo + chunk);
    unsigned long long s = 0;
    uint32_t fb = 0xffffffffu, nd = 0;
    for (uint32_t j = lo; j < hi; j++) {
        s += a.res[j].ncoef;
        if (a.res[j].status == MP2VG_OK) continue;
        if (a.conceal && sp_reason_concealed(a.res[j].reason)) nd++;
        else if (fb == 0xffffffffu) fb = j;
    }
    const bool conceal = a.conceal != 0;  // (uniform: without the flag the scan does what it always did)
    sum[t] = s;
    bad[t] = fb;
    if (conceal) dmg[t] = nd;
    __syncthreads();
    for (int d = 1; d < kScanThreads; d <<= 1) {  // inclusive scan of the runs' sums, min of the failures
        const unsigned long long v = t >= (uint32_t)d ? sum[t - d] : 0;
        const uint32_t b = t >= (uint32_t)d ? bad[t - d] : 0xffffffffu;
        const uint32_t g = conceal && t >= (uint32_t)d ? dmg[t - d] : 0;
        __syncthreads();
        sum[t] += v;
        bad[t] = min(bad[t], b);
        if (conceal) dmg[t] += g;
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
        summary[2] = conceal ? dmg[t] : 0;
    }
    for (uint32_t p = t; p < a.npics; p += kScanThreads) {
        uint32_t u = 0;
        for (uint32_t j = pic_slice[p]; j < pic_slice[p + 1] && j < n; j++)
            u |= a.res[j].uses | (conceal && a.res[j].status != MP2VG_OK ? 4u : 0u);
        a.uses[p] = u;
    }
}

__global__ __launch_bounds__(64) void parse_emit_kernel(ParseArgs a) {
    const uint32_t j = blockIdx.x * 64u + threadIdx.x;
    if (j >= a.nslices) return;
    const DevSlice s = a.slices[j];
    if (!entry_ok(a, s)) return;
    if (a.res[j].fate == SP_FATE_DROPPED) return;  // MP2VG_PARSE_SLICES: its row was replaced, the carrier emits it
    const uint32_t base = a.base[j], cap = a.res[j].ncoef;
    if ((uint64_t)base + cap > a.base[a.nslices]) return;  // (never: base is the counts' prefix sum)
    const SpEmitOut out{a.mbs + a.mb_first[s.pic] + (size_t)s.mb_row * a.G.mbw, a.coefs + base, cap, base};
    if (a.res[j].reason != SP_OK) {  // a concealed row: its rebased coef_off and its DC words, no second parse
        uint32_t uses;
        (void)sp_conceal_row(a.G, a.hdr[s.pic], (int)s.mb_row, out, uses);
        return;
    }
    SpResult r;
    sp_parse_slice(a.T, a.G, a.hdr[s.pic], a.bs, (int64_t)s.byte_off, (int64_t)s.byte_end, (int64_t)a.span,
                   (int)s.mb_row, out, r);
}

hipError_t launch_parse_count(const ParseArgs& a, hipStream_t stream) {
    if (!a.nslices) return hipSuccess;
    hipLaunchKernelGGL(parse_count_kernel, dim3((a.nslices + 63) / 64), dim3(64), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_parse_rows(const ParseArgs& a, hipStream_t stream) {
    if (!a.nslices || !a.rows) return hipSuccess;
    for (int phase = 0; phase < 2; phase++)
        hipLaunchKernelGGL(parse_rows_kernel, dim3((a.nslices + 63) / 64), dim3(64), 0, stream, a, phase);
    return hipGetLastError();
}

hipError_t launch_parse_conceal(const ParseArgs& a, hipStream_t stream) {
    if (!a.nslices || !a.conceal) return hipSuccess;
    hipLaunchKernelGGL(parse_conceal_kernel, dim3((a.nslices + 63) / 64), dim3(64), 0, stream, a);
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
