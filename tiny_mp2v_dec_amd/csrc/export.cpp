// export.cpp — host entry points of the RGB export that enqueue the kernel (export.hip):
// mp2vg_export_slots and mp2vg_export_planes.  The host-only part (coefficients, matrix choice,
// sizes, validation) and the context's bookkeeping live in runtime.cpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>

#include "export_kernel.h"
#include "hipchk.h"
#include "syntax.h"

using namespace mp2vg;


// coefficients, folded constants and rectangle
static void export_args(ExportArgs* a, const mp2vg_export_t* e, int32_t w, int32_t h, void* dst) {
    int32_t k[5];
    mp2vg_export_coefficients(e->matrix, k);
    a->w = w, a->h = h;
    a->cy = k[0], a->crv = k[1], a->cgu = k[2], a->cgv = k[3], a->cbu = k[4];
    const int32_t base = 8192 - 16 * k[0];
    a->kr = base - 128 * k[1];
    a->kg = base - 128 * (k[2] + k[3]);
    a->kb = base - 128 * k[4];
    a->dst = (uint8_t*)dst;
}

static constexpr int32_t kExportMaxFrames = 65535;  // the frame index is a grid dimension

extern "C" int mp2vg_export_slots(mp2vg_ctx_t* c, const int32_t* slots, int32_t n, const mp2vg_export_t* e,
                                  void* dst, uint64_t dst_bytes) {
    if (!c || !slots || !e || !dst || n <= 0 || n > kExportMaxFrames) return MP2VG_E_INVALID;
    ExportSource s;
    export_source(c, &s);
    for (int i = 0; i < n; i++)
        if (slots[i] < 0 || slots[i] >= s.nslots) {
            set_error("export: slot out of range");
            return MP2VG_E_INVALID;
        }
    int32_t w, h;
    if (int rc = check_export(e, s.pw, s.ph, &w, &h)) return rc;
    if (dst_bytes != (uint64_t)n * 3 * (uint64_t)w * (uint64_t)h) {
        set_error("export: dst_bytes is not n * 3 * width * height");
        return MP2VG_E_INVALID;
    }
    HIPCHK(hipSetDevice(s.device));
    ExportArgs a;
    memset(&a, 0, sizeof a);
    if (int rc = export_stage_slots(c, slots, n, &a.slots)) return rc;
    a.ftab = s.ftab;
    for (int p = 0; p < 3; p++) {
        a.plane_off[p] = s.plane_off[p];
        a.stride[p] = s.stride[p];
    }
    a.cw = s.cw;
    a.ch = s.ch;
    export_args(&a, e, w, h, dst);
    // the slot list's copy is in flight: its events are recorded whether or not the launch succeeded
    const hipError_t le = launch_export(s.cf, e->layout, e->chroma, a, n, s.stream);
    const int rc = export_enqueued(c);
    HIPCHK(le);
    return rc;
}

extern "C" int mp2vg_export_planes(int32_t device, const uint8_t* const planes[3], const int32_t stride[3],
                                   int32_t cf, int32_t coded_w, int32_t coded_h, const mp2vg_export_t* e, void* dst,
                                   uint64_t dst_bytes) {
    if (!planes || !stride || !e || !dst || device < 0 || cf < 1 || cf > 3 || coded_w <= 0 || coded_h <= 0)
        return MP2VG_E_INVALID;
    if ((cf < 3 && (coded_w & 1)) || (cf == 1 && (coded_h & 1))) {
        set_error("export: odd coded size with subsampled chroma");
        return MP2VG_E_INVALID;
    }
    const int32_t cw = cf == 3 ? coded_w : coded_w >> 1, ch = cf == 1 ? coded_h >> 1 : coded_h;
    for (int p = 0; p < 3; p++)
        if (!planes[p] || ((uintptr_t)planes[p] & 3) || stride[p] < 4 || (stride[p] & 3) ||
            stride[p] < (p ? cw : coded_w)) {
            set_error("export: planes must be 4-byte aligned, strides multiples of 4 and at least the plane width");
            return MP2VG_E_INVALID;
        }
    int32_t w, h;
    if (int rc = check_export(e, coded_w, coded_h, &w, &h)) return rc;
    if (dst_bytes != 3 * (uint64_t)w * (uint64_t)h) {
        set_error("export: dst_bytes is not 3 * width * height");
        return MP2VG_E_INVALID;
    }
    HIPCHK(hipSetDevice(device));
    ExportArgs a;
    memset(&a, 0, sizeof a);
    for (int p = 0; p < 3; p++) {
        a.planes[p] = planes[p];
        a.stride[p] = stride[p];
    }
    a.cw = cw;
    a.ch = ch;
    export_args(&a, e, w, h, dst);
    HIPCHK(launch_export(cf, e->layout, e->chroma, a, 1, nullptr));
    HIPCHK(hipStreamSynchronize(nullptr));
    return MP2VG_OK;
}
