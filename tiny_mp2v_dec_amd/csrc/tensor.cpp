// tensor.cpp — host entry points of the tensor export that enqueue the kernel (tensor.hip):
// mp2vg_tensor_slots_placed and mp2vg_tensor_planes_placed, their cases without a placement
// (mp2vg_tensor_slots_fields, mp2vg_tensor_planes_field) and all PROGRESSIVE (mp2vg_tensor_slots,
// mp2vg_tensor_planes), and the items launches (mp2vg_tensor_items, mp2vg_tensor_planes_items).
// The host-only part (tap tables, validation, sizes, the plan of an items launch)
// lives in runtime.cpp; the context's side (slot table, staging ring, events) is the RGB export's.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "export_kernel.h"
#include "hipchk.h"
#include "syntax.h"
#include "tensor_kernel.h"

using namespace mp2vg;

static constexpr int32_t kTensorMaxFrames = 65535;  // the frame index is a grid dimension

// coefficients, output size, normalisation and destination: what every launch takes from t
static void tensor_common_args(TensorArgs* a, const mp2vg_tensor_t* t, void* dst) {
    int32_t k[5];
    mp2vg_export_coefficients(t->matrix, k);
    a->cy = k[0], a->crv = k[1], a->cgu = k[2], a->cgv = k[3], a->cbu = k[4];
    const int32_t base = 8192 - 16 * k[0];
    a->kr = base - 128 * k[1];
    a->kg = base - 128 * (k[2] + k[3]);
    a->kb = base - 128 * k[4];
    a->out_w = t->out_w, a->out_h = t->out_h;
    for (int c = 0; c < 3; c++) a->scale[c] = t->scale[c], a->bias[c] = t->bias[c];
    a->dst = dst;
}

// those, the rectangle and the tables at d (the device copy of tt.blob)
// and the placement: the picture's rectangle pd in the output, the pad colour in units of Q
static void tensor_args(TensorArgs* a, const mp2vg_tensor_t* t, const int32_t rect[4], const TensorTables& tt,
                        const int32_t* d, void* dst, const int32_t pd[4], const mp2vg_tensor_place_t* place) {
    tensor_common_args(a, t, dst);
    a->src_x = rect[0], a->src_y = rect[1];
    a->segs = d + tt.off[0], a->hfirst = d + tt.off[1], a->hw = d + tt.off[2];
    a->vfirst = d + tt.off[3], a->vcount = d + tt.off[4], a->vw = d + tt.off[5];
    a->hmax = tt.hmax, a->vmax = tt.vmax;
    a->dst_x = pd[0], a->dst_y = pd[1], a->dst_w = pd[2], a->dst_h = pd[3];
    for (int c = 0; c < 3; c++) a->padq[c] = place ? 64 * (int32_t)place->pad[c] : 0;
}

static int check_dst(const mp2vg_tensor_t* t, int32_t n, int32_t elem, const void* dst, uint64_t dst_bytes) {
    if (dst_bytes != (uint64_t)n * 3 * (uint64_t)t->out_w * (uint64_t)t->out_h * (uint64_t)elem) {
        set_error("tensor: dst_bytes is not n * 3 * out_w * out_h * element size");
        return MP2VG_E_INVALID;
    }
    if ((uintptr_t)dst % (uintptr_t)elem) {
        set_error("tensor: dst is not aligned to the element size");
        return MP2VG_E_INVALID;
    }
    return MP2VG_OK;
}

// the plane preconditions of the calls over device plane pointers (cf 1..3, sizes positive)
static int check_planes(const uint8_t* const planes[3], const int32_t stride[3], int32_t cf, int32_t coded_w,
                        int32_t coded_h) {
    if ((cf < 3 && (coded_w & 1)) || (cf == 1 && (coded_h & 1))) {
        set_error("tensor: odd coded size with subsampled chroma");
        return MP2VG_E_INVALID;
    }
    const int32_t cw = cf == 3 ? coded_w : coded_w >> 1;
    for (int p = 0; p < 3; p++)
        if (!planes[p] || ((uintptr_t)planes[p] & 3) || stride[p] < 4 || (stride[p] & 3) ||
            stride[p] < (p ? cw : coded_w)) {
            set_error("tensor: planes must be 4-byte aligned, strides multiples of 4 and at least the plane width");
            return MP2VG_E_INVALID;
        }
    return MP2VG_OK;
}

extern "C" int mp2vg_tensor_slots_placed(mp2vg_ctx_t* c, const int32_t* slots, const int32_t* fields, int32_t n,
                                         const mp2vg_tensor_t* t, const mp2vg_tensor_place_t* place, void* dst,
                                         uint64_t dst_bytes) {
    if (!c || !slots || !t || !dst || n <= 0 || n > kTensorMaxFrames) return MP2VG_E_INVALID;
    ExportSource s;
    export_source(c, &s);
    for (int i = 0; i < n; i++)
        if (slots[i] < 0 || slots[i] >= s.nslots) {
            set_error("tensor: slot out of range");
            return MP2VG_E_INVALID;
        }
    // a list of PROGRESSIVE only is the launch without field modes (mp2vg_tensor_slots)
    bool field_modes = false;
    for (int i = 0; fields && i < n; i++) {
        if (int rc = check_tensor_field(fields[i], s.cf, s.ph)) return rc;
        field_modes |= fields[i] != MP2VG_FIELD_PROGRESSIVE;
    }
    int32_t rect[4], elem, pd[4];
    bool placed;
    if (int rc = check_tensor_placed(t, place, s.pw, s.ph, rect, &elem, pd, &placed)) return rc;
    if (int rc = check_dst(t, n, elem, dst, dst_bytes)) return rc;
    // staged in front of the tables (those of the picture's rectangle): the slot list, then the field list
    TensorTables tt;
    if (int rc = tensor_tables(rect, pd[2], pd[3], (size_t)n * (field_modes ? 2 : 1), &tt)) return rc;
    memcpy(tt.blob.data(), slots, sizeof(int32_t) * n);
    if (field_modes) memcpy(tt.blob.data() + n, fields, sizeof(int32_t) * n);
    HIPCHK(hipSetDevice(s.device));
    TensorArgs a;
    memset(&a, 0, sizeof a);
    const int32_t* d = nullptr;
    if (int rc = export_stage_slots(c, tt.blob.data(), (int32_t)tt.blob.size(), &d)) return rc;
    a.slots = d;
    a.fields = field_modes ? d + n : nullptr;
    a.coded_h = s.ph;
    a.ftab = s.ftab;
    for (int p = 0; p < 3; p++) {
        a.plane_off[p] = s.plane_off[p];
        a.stride[p] = s.stride[p];
    }
    a.cw = s.cw;
    a.ch = s.ch;
    tensor_args(&a, t, rect, tt, d, dst, pd, place);
    // the list's copy is in flight: its events are recorded whether or not the launch succeeded
    const hipError_t le =
        launch_tensor(s.cf, t->layout, t->chroma, t->dtype, field_modes, placed, a, tt.nsegs, n, s.stream);
    const int rc = export_enqueued(c);
    HIPCHK(le);
    return rc;
}

extern "C" int mp2vg_tensor_slots_fields(mp2vg_ctx_t* c, const int32_t* slots, const int32_t* fields, int32_t n,
                                         const mp2vg_tensor_t* t, void* dst, uint64_t dst_bytes) {
    return mp2vg_tensor_slots_placed(c, slots, fields, n, t, nullptr, dst, dst_bytes);
}

extern "C" int mp2vg_tensor_slots(mp2vg_ctx_t* c, const int32_t* slots, int32_t n, const mp2vg_tensor_t* t, void* dst,
                                  uint64_t dst_bytes) {
    return mp2vg_tensor_slots_fields(c, slots, nullptr, n, t, dst, dst_bytes);
}

extern "C" int mp2vg_tensor_planes_placed(int32_t device, const uint8_t* const planes[3], const int32_t stride[3],
                                          int32_t cf, int32_t coded_w, int32_t coded_h, int32_t field,
                                          const mp2vg_tensor_t* t, const mp2vg_tensor_place_t* place, void* dst,
                                          uint64_t dst_bytes) {
    if (!planes || !stride || !t || !dst || device < 0 || cf < 1 || cf > 3 || coded_w <= 0 || coded_h <= 0)
        return MP2VG_E_INVALID;
    if (int rc = check_tensor_field(field, cf, coded_h)) return rc;
    if (int rc = check_planes(planes, stride, cf, coded_w, coded_h)) return rc;
    const int32_t cw = cf == 3 ? coded_w : coded_w >> 1, ch = cf == 1 ? coded_h >> 1 : coded_h;
    int32_t rect[4], elem, pd[4];
    bool placed;
    if (int rc = check_tensor_placed(t, place, coded_w, coded_h, rect, &elem, pd, &placed)) return rc;
    if (int rc = check_dst(t, 1, elem, dst, dst_bytes)) return rc;
    TensorTables tt;
    if (int rc = tensor_tables(rect, pd[2], pd[3], 0, &tt)) return rc;
    HIPCHK(hipSetDevice(device));
    int32_t* d = nullptr;
    const size_t bytes = tt.blob.size() * sizeof(int32_t);
    HIPCHK(hipMalloc((void**)&d, bytes));
    hipError_t e = hipMemcpy(d, tt.blob.data(), bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        TensorArgs a;
        memset(&a, 0, sizeof a);
        for (int p = 0; p < 3; p++) {
            a.planes[p] = planes[p];
            a.stride[p] = stride[p];
        }
        a.cw = cw;
        a.ch = ch;
        a.field = field;
        a.coded_h = coded_h;
        tensor_args(&a, t, rect, tt, d, dst, pd, place);
        e = launch_tensor(cf, t->layout, t->chroma, t->dtype, field != MP2VG_FIELD_PROGRESSIVE, placed, a, tt.nsegs, 1,
                          nullptr);
        if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    }
    hipFree(d);
    HIPCHK(e);
    return MP2VG_OK;
}

extern "C" int mp2vg_tensor_planes_field(int32_t device, const uint8_t* const planes[3], const int32_t stride[3],
                                         int32_t cf, int32_t coded_w, int32_t coded_h, int32_t field,
                                         const mp2vg_tensor_t* t, void* dst, uint64_t dst_bytes) {
    return mp2vg_tensor_planes_placed(device, planes, stride, cf, coded_w, coded_h, field, t, nullptr, dst, dst_bytes);
}

extern "C" int mp2vg_tensor_planes(int32_t device, const uint8_t* const planes[3], const int32_t stride[3], int32_t cf,
                                   int32_t coded_w, int32_t coded_h, const mp2vg_tensor_t* t, void* dst,
                                   uint64_t dst_bytes) {
    return mp2vg_tensor_planes_field(device, planes, stride, cf, coded_w, coded_h, MP2VG_FIELD_PROGRESSIVE, t, dst,
                                     dst_bytes);
}

// ---- items (include/mp2vg.h "Items") ----------------------------------------------------------------

extern "C" int mp2vg_tensor_items(mp2vg_ctx_t* c, const mp2vg_tensor_item_t* items, int32_t n, const mp2vg_tensor_t* t,
                                  int32_t clip_len, void* dst, uint64_t dst_bytes) {
    if (!c || !items || !t || !dst) return MP2VG_E_INVALID;
    ExportSource s;
    export_source(c, &s);
    ItemsPlan plan;
    if (int rc = tensor_items_plan(t, items, n, clip_len, s.cf, s.pw, s.ph, s.nslots, false, &plan)) return rc;
    if (int rc = check_dst(t, n, plan.elem, dst, dst_bytes)) return rc;
    HIPCHK(hipSetDevice(s.device));
    TensorArgs a;
    memset(&a, 0, sizeof a);
    const int32_t* d = nullptr;
    if (int rc = export_stage_slots(c, plan.blob.data(), (int32_t)plan.blob.size(), &d)) return rc;
    a.items = d;
    a.clip_len = clip_len;
    a.coded_h = s.ph;
    a.ftab = s.ftab;
    for (int p = 0; p < 3; p++) {
        a.plane_off[p] = s.plane_off[p];
        a.stride[p] = s.stride[p];
    }
    a.cw = s.cw;
    a.ch = s.ch;
    tensor_common_args(&a, t, dst);
    // the blob's copy is in flight: its events are recorded whether or not the launch succeeded
    const hipError_t le = launch_tensor_items(s.cf, t->layout, t->chroma, t->dtype, a, plan.grid_x, n, s.stream);
    const int rc = export_enqueued(c);
    HIPCHK(le);
    return rc;
}

extern "C" int mp2vg_tensor_planes_items(int32_t device, const uint8_t* const planes[3], const int32_t stride[3],
                                         int32_t cf, int32_t coded_w, int32_t coded_h, const mp2vg_tensor_item_t* items,
                                         int32_t n, const mp2vg_tensor_t* t, int32_t clip_len, void* dst,
                                         uint64_t dst_bytes) {
    if (!planes || !stride || !items || !t || !dst || device < 0 || cf < 1 || cf > 3 || coded_w <= 0 || coded_h <= 0)
        return MP2VG_E_INVALID;
    if (int rc = check_planes(planes, stride, cf, coded_w, coded_h)) return rc;
    ItemsPlan plan;
    if (int rc = tensor_items_plan(t, items, n, clip_len, cf, coded_w, coded_h, 1, true, &plan)) return rc;
    if (int rc = check_dst(t, n, plan.elem, dst, dst_bytes)) return rc;
    HIPCHK(hipSetDevice(device));
    int32_t* d = nullptr;
    const size_t bytes = plan.blob.size() * sizeof(int32_t);
    HIPCHK(hipMalloc((void**)&d, bytes));
    hipError_t e = hipMemcpy(d, plan.blob.data(), bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        TensorArgs a;
        memset(&a, 0, sizeof a);
        for (int p = 0; p < 3; p++) {
            a.planes[p] = planes[p];
            a.stride[p] = stride[p];
        }
        a.cw = cf == 3 ? coded_w : coded_w >> 1;
        a.ch = cf == 1 ? coded_h >> 1 : coded_h;
        a.items = d;
        a.clip_len = clip_len;
        a.coded_h = coded_h;
        tensor_common_args(&a, t, dst);
        e = launch_tensor_items(cf, t->layout, t->chroma, t->dtype, a, plan.grid_x, n, nullptr);
        if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    }
    hipFree(d);
    HIPCHK(e);
    return MP2VG_OK;
}
