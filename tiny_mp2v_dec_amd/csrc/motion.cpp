// motion.cpp — host entry points of the compressed-domain export: sizes (mp2vg_motion_bytes), the
// host twin over host records (mp2vg_motion_records, no device) and the enqueue over the resident
// bank (mp2vg_motion_batch; kernels in motion.hip, the context's side in runtime.cpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>

#include "export_kernel.h"
#include "hipchk.h"
#include "motion_kernel.h"
#include "syntax.h"

using namespace mp2vg;

static constexpr int32_t kMotionMaxPictures = 65535;  // the picture index is a grid dimension

static int motion_geometry(const mp2vg_config_t* cfg, int32_t* mbw, int32_t* mbh, int32_t* nb) {
    if (!cfg || mp2vg_frame_geometry(cfg, nullptr, nullptr, nullptr, nullptr) != MP2VG_OK) return MP2VG_E_INVALID;
    *mbw = cfg->width / 16, *mbh = cfg->height / 16;
    *nb = cfg->chroma_format == 1 ? 6 : (cfg->chroma_format == 2 ? 8 : 12);
    return MP2VG_OK;
}

static void motion_sizes(int32_t mbw, int32_t mbh, int32_t nb, int32_t n, uint64_t bytes[3]) {
    const uint64_t cells = (uint64_t)n * (uint64_t)mbw * (uint64_t)mbh;
    bytes[0] = cells * 8 * sizeof(int16_t);
    bytes[1] = cells * 4 * sizeof(uint16_t);
    bytes[2] = cells * 2 * (uint64_t)nb * sizeof(int32_t);
}

static int check_count(int32_t n) {
    if (n <= 0 || n > kMotionMaxPictures) {
        set_error("motion export: n must be 1 .. 65535");
        return MP2VG_E_INVALID;
    }
    return MP2VG_OK;
}

static int check_order(const int32_t* order, int32_t n, int32_t npics) {
    for (int32_t i = 0; i < n; i++)
        if (order[i] < 0 || order[i] >= npics) {
            set_error("motion export: order[" + std::to_string(i) + "] is outside the batch's pictures");
            return MP2VG_E_INVALID;
        }
    return MP2VG_OK;
}

extern "C" int mp2vg_motion_bytes(const mp2vg_config_t* cfg, int32_t n, uint64_t bytes[3]) {
    int32_t mbw, mbh, nb;
    if (!bytes || motion_geometry(cfg, &mbw, &mbh, &nb) != MP2VG_OK) return MP2VG_E_INVALID;
    if (int rc = check_count(n)) return rc;
    motion_sizes(mbw, mbh, nb, n, bytes);
    return MP2VG_OK;
}

extern "C" int mp2vg_motion_records(const mp2vg_config_t* cfg, const mp2vg_picture_t* pics, int32_t npics,
                                    const mp2vg_mb_t* mbs, uint64_t nmbs, const uint32_t* coefs, uint64_t ncoefs,
                                    const int32_t* order, int32_t n, int16_t* mv, uint16_t* info, int32_t* act) {
    int32_t mbw, mbh, nb;
    if (!order || !pics || npics <= 0 || motion_geometry(cfg, &mbw, &mbh, &nb) != MP2VG_OK) return MP2VG_E_INVALID;
    if (int rc = check_count(n)) return rc;
    if (!mv && !info && !act) {
        set_error("motion export: no output wanted");
        return MP2VG_E_INVALID;
    }
    // the upload's own validation, over a pool just large enough for the slots the pictures name
    int32_t nslots = 1;
    for (int32_t p = 0; p < npics; p++)
        nslots = std::max(nslots, std::max(pics[p].dst_slot, std::max(pics[p].fwd_slot, pics[p].bwd_slot)) + 1);
    if (int rc = mp2vg_batch_validate(cfg, nslots, pics, npics, mbs, nmbs, coefs, ncoefs, nullptr, nullptr, nullptr, 0))
        return rc;
    if (int rc = check_order(order, n, npics)) return rc;
    const size_t M = (size_t)mbw * mbh;
    for (int32_t f = 0; f < n; f++) {
        const mp2vg_mb_t* rec = mbs + pics[order[f]].mb_first;
        for (size_t i = 0; i < M; i++) {
            uint32_t r[8];
            memcpy(r, &rec[i], sizeof r);
            int16_t v[8];
            uint16_t q[4];
            motion_mb(r, v, q);
            if (mv)
                for (int c = 0; c < 8; c++) mv[((size_t)f * 8 + c) * M + i] = v[c];
            if (info)
                for (int c = 0; c < 4; c++) info[((size_t)f * 4 + c) * M + i] = q[c];
            if (!act) continue;
            int32_t* a = act + (size_t)f * 2 * nb * M + i;
            for (int k = 0; k < 2 * nb; k++) a[(size_t)k * M] = 0;
            for (uint32_t j = 0; j < rec[i].ncoef; j++) {
                int b;
                int32_t mag;
                if (!motion_word(coefs[rec[i].coef_off + j], nb, &b, &mag)) continue;
                a[(size_t)b * M] += 1;
                a[(size_t)(nb + b) * M] += mag;
            }
        }
    }
    return MP2VG_OK;
}

extern "C" int mp2vg_motion_batch(mp2vg_ctx_t* c, const int32_t* order, int32_t n, void* mv, void* info, void* act,
                                  const uint64_t bytes[3]) {
    if (!c || !order || !bytes) return MP2VG_E_INVALID;
    MotionSource s;
    if (int rc = motion_source(c, &s)) return rc;
    if (int rc = check_count(n)) return rc;
    if (int rc = check_order(order, n, s.npics)) return rc;
    if (!mv && !info && !act) {
        set_error("motion export: no output wanted");
        return MP2VG_E_INVALID;
    }
    uint64_t want[3];
    motion_sizes(s.mbw, s.mbh, s.nb, n, want);
    void* const dst[3] = {mv, info, act};
    for (int t = 0; t < 3; t++) {
        if (!dst[t]) continue;
        if (bytes[t] != want[t]) {
            set_error("motion export: a tensor's size differs from mp2vg_motion_bytes");
            return MP2VG_E_INVALID;
        }
        if ((uintptr_t)dst[t] & 3) {
            set_error("motion export: tensors must be 4-byte aligned");
            return MP2VG_E_INVALID;
        }
    }
    HIPCHK(hipSetDevice(s.device));
    MotionArgs a;
    memset(&a, 0, sizeof a);
    if (int rc = export_stage_slots(c, order, n, &a.order)) return rc;
    a.pics = s.d_pics;
    a.mbs = s.d_mbs;
    a.coefs = s.d_coefs;
    a.mbw = s.mbw, a.mbh = s.mbh, a.nb = s.nb;
    a.mv = (int16_t*)mv;
    a.info = (uint16_t*)info;
    a.act = (int32_t*)act;
    // the order list's copy is in flight: its events are recorded whether or not the launch succeeded
    int rc = motion_begin(c);
    const hipError_t le = rc == MP2VG_OK ? launch_motion(a, n, s.stream) : hipSuccess;
    const int rc2 = motion_enqueued(c);
    HIPCHK(le);
    return rc ? rc : rc2;
}
