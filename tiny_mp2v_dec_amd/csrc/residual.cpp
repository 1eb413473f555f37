// residual.cpp — host entry points of the residual export: sizes (mp2vg_residual_bytes), the host
// twin over host records (mp2vg_residual_records, no device) and the enqueue over the resident bank
// (mp2vg_residual_batch; kernel in residual.hip, the context's side in runtime.cpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>

#include "export_kernel.h"
#include "hipchk.h"
#include "motion_kernel.h"
#include "residual_kernel.h"
#include "syntax.h"

using namespace mp2vg;

static constexpr int32_t kResidualMaxPictures = 65535;  // the picture index is a grid dimension

static const uint8_t k_scan[2][64] = MP2VG_RESIDUAL_SCAN;

struct ResidualGeo {
    int32_t mbw, mbh, cf, nb;
};

static int residual_geometry(const mp2vg_config_t* cfg, ResidualGeo* g) {
    if (!cfg || mp2vg_frame_geometry(cfg, nullptr, nullptr, nullptr, nullptr) != MP2VG_OK) return MP2VG_E_INVALID;
    g->mbw = cfg->width / 16, g->mbh = cfg->height / 16, g->cf = cfg->chroma_format;
    g->nb = g->cf == 1 ? 6 : (g->cf == 2 ? 8 : 12);
    return MP2VG_OK;
}

static void residual_sizes(const ResidualGeo& g, int32_t n, int32_t dtype, uint64_t bytes[3]) {
    const uint64_t el = dtype == MP2VG_RESIDUAL_I8 ? 1 : 2;
    for (int pl = 0; pl < 3; pl++)
        bytes[pl] = (uint64_t)n * g.mbw * residual_mb_w(g.cf, pl) * g.mbh * residual_mb_h(g.cf, pl) * el;
}

static int check_call(int32_t n, int32_t dtype, int32_t flags) {
    if (n <= 0 || n > kResidualMaxPictures) {
        set_error("residual export: n must be 1 .. 65535");
        return MP2VG_E_INVALID;
    }
    if (dtype != MP2VG_RESIDUAL_I16 && dtype != MP2VG_RESIDUAL_I8) {
        set_error("residual export: dtype outside MP2VG_RESIDUAL_*");
        return MP2VG_E_INVALID;
    }
    if (flags & ~MP2VG_RESIDUAL_ZERO_INTRA) {
        set_error("residual export: unknown flag bit");
        return MP2VG_E_INVALID;
    }
    return MP2VG_OK;
}

static int check_outputs(const void* y, const void* cb, const void* cr, bool aligned) {
    if (!cb != !cr) {
        set_error("residual export: cb and cr are given together or not at all");
        return MP2VG_E_INVALID;
    }
    if (!y && !cb) {
        set_error("residual export: no output wanted");
        return MP2VG_E_INVALID;
    }
    for (const void* p : {y, cb, cr})
        if (aligned && ((uintptr_t)p & 15)) {
            set_error("residual export: planes must be 16-byte aligned");
            return MP2VG_E_INVALID;
        }
    return MP2VG_OK;
}

static int check_order(const int32_t* order, int32_t n, int32_t npics) {
    for (int32_t i = 0; i < n; i++)
        if (order[i] < 0 || order[i] >= npics) {
            set_error("residual export: order[" + std::to_string(i) + "] is outside the batch's pictures");
            return MP2VG_E_INVALID;
        }
    return MP2VG_OK;
}

extern "C" int mp2vg_residual_bytes(const mp2vg_config_t* cfg, int32_t n, int32_t dtype, uint64_t bytes[3]) {
    ResidualGeo g;
    if (!bytes || residual_geometry(cfg, &g) != MP2VG_OK) return MP2VG_E_INVALID;
    if (int rc = check_call(n, dtype, 0)) return rc;
    residual_sizes(g, n, dtype, bytes);
    return MP2VG_OK;
}

// the residual of every block of one MB: res[b][row * 8 + x], zeros where the block is not coded
static void residual_mb(const mp2vg_picture_t& pic, const mp2vg_mb_t& mb, const uint32_t* coefs, int nb, int dtype,
                        int flags, int16_t res[12][64]) {
    memset(res, 0, sizeof(int16_t) * 12 * 64);
    const bool intra = (mb.flags & MP2VG_MB_INTRA) != 0;
    const uint32_t cbp = (flags & MP2VG_RESIDUAL_ZERO_INTRA) && intra ? 0u : mb.cbp & ((1u << nb) - 1u);
    if (!cbp) return;
    int sum[12] = {0};
    const uint8_t* scan = k_scan[pic.alternate_scan ? 1 : 0];
    for (uint32_t j = 0; j < mb.ncoef; j++) {
        const uint32_t w = coefs[mb.coef_off + j];
        const int b = (int)MP2VG_COEF_BLOCK(w);
        if (b >= nb || !(cbp >> b & 1u)) continue;
        int idx, val, par;
        residual_word(w, pic.W[residual_matrix(b, intra)], mb.qscale, intra, scan, &idx, &val, &par);
        res[b][idx] = (int16_t)val;
        sum[b] ^= par;
    }
    const int lo = residual_lo(dtype), hi = residual_hi(dtype);
    for (int b = 0; b < nb; b++) {
        if (!(cbp >> b & 1u)) continue;
        int16_t* q = res[b];
        q[63] ^= (int16_t)((sum[b] & 1) ^ 1);
        R16 t[8][8];
        for (int i = 0; i < 8; i++)
            for (int j = 0; j < 8; j++) t[i][j].v = q[i * 8 + j];
        for (int pass = 0; pass < 2; pass++) {
            for (int j = 0; j < 8; j++) {  // the pass runs down every column
                R16 s[8];
                for (int i = 0; i < 8; i++) s[i] = t[i][j];
                residual_idct_1d(s);
                for (int i = 0; i < 8; i++) t[i][j] = s[i];
            }
            if (pass == 0)
                for (int i = 0; i < 8; i++)
                    for (int j = i + 1; j < 8; j++) std::swap(t[i][j], t[j][i]);
        }
        for (int i = 0; i < 8; i++)
            for (int j = 0; j < 8; j++) q[i * 8 + j] = (int16_t)std::min(std::max(t[i][j].v >> 6, lo), hi);
    }
}

extern "C" int mp2vg_residual_records(const mp2vg_config_t* cfg, const mp2vg_picture_t* pics, int32_t npics,
                                      const mp2vg_mb_t* mbs, uint64_t nmbs, const uint32_t* coefs, uint64_t ncoefs,
                                      const int32_t* order, int32_t n, int32_t dtype, int32_t flags, void* y, void* cb,
                                      void* cr) {
    ResidualGeo g;
    if (!order || !pics || npics <= 0 || residual_geometry(cfg, &g) != MP2VG_OK) return MP2VG_E_INVALID;
    if (int rc = check_call(n, dtype, flags)) return rc;
    if (int rc = check_outputs(y, cb, cr, false)) return rc;  // host buffers: any alignment
    // the upload's own validation, over a pool just large enough for the slots the pictures name
    int32_t nslots = 1;
    for (int32_t p = 0; p < npics; p++)
        nslots = std::max(nslots, std::max(pics[p].dst_slot, std::max(pics[p].fwd_slot, pics[p].bwd_slot)) + 1);
    if (int rc = mp2vg_batch_validate(cfg, nslots, pics, npics, mbs, nmbs, coefs, ncoefs, nullptr, nullptr, nullptr, 0))
        return rc;
    if (int rc = check_order(order, n, npics)) return rc;
    void* const dst[3] = {y, cb, cr};
    for (int32_t f = 0; f < n; f++) {
        const mp2vg_picture_t& pic = pics[order[f]];
        for (int32_t my = 0; my < g.mbh; my++)
            for (int32_t mx = 0; mx < g.mbw; mx++) {
                const mp2vg_mb_t& mb = mbs[pic.mb_first + (size_t)my * g.mbw + mx];
                int16_t res[12][64];
                residual_mb(pic, mb, coefs, g.nb, dtype, flags, res);
                const bool dctf = (mb.flags & MP2VG_MB_DCT_FIELD) != 0;
                for (int pl = 0; pl < 3; pl++) {
                    if (!dst[pl]) continue;
                    const int MW = residual_mb_w(g.cf, pl), MH = residual_mb_h(g.cf, pl);
                    const size_t PW = (size_t)g.mbw * MW, PH = (size_t)g.mbh * MH;
                    for (int yy = 0; yy < MH; yy++)
                        for (int xb = 0; xb < MW / 8; xb++) {
                            int b, row;
                            residual_source(g.cf, pl, yy, xb, dctf, &b, &row);
                            const size_t e = ((size_t)f * PH + (size_t)my * MH + yy) * PW + (size_t)mx * MW + xb * 8;
                            for (int x = 0; x < 8; x++) {
                                if (dtype == MP2VG_RESIDUAL_I8) ((int8_t*)dst[pl])[e + x] = (int8_t)res[b][row * 8 + x];
                                else ((int16_t*)dst[pl])[e + x] = res[b][row * 8 + x];
                            }
                        }
                }
            }
    }
    return MP2VG_OK;
}

extern "C" int mp2vg_residual_batch(mp2vg_ctx_t* c, const int32_t* order, int32_t n, int32_t dtype, int32_t flags,
                                    void* y, void* cb, void* cr, const uint64_t bytes[3]) {
    if (!c || !order || !bytes) return MP2VG_E_INVALID;
    MotionSource s;
    if (int rc = motion_source(c, &s)) return rc;
    if (int rc = check_call(n, dtype, flags)) return rc;
    if (int rc = check_order(order, n, s.npics)) return rc;
    if (int rc = check_outputs(y, cb, cr, true)) return rc;
    ResidualGeo g{s.mbw, s.mbh, s.nb == 6 ? 1 : (s.nb == 8 ? 2 : 3), s.nb};
    uint64_t want[3];
    residual_sizes(g, n, dtype, want);
    void* const dst[3] = {y, cb, cr};
    for (int t = 0; t < 3; t++)
        if (dst[t] && bytes[t] != want[t]) {
            set_error("residual export: a plane's size differs from mp2vg_residual_bytes");
            return MP2VG_E_INVALID;
        }
    HIPCHK(hipSetDevice(s.device));
    ResidualArgs a;
    memset(&a, 0, sizeof a);
    if (int rc = export_stage_slots(c, order, n, &a.order)) return rc;
    a.pics = s.d_pics;
    a.mbs = s.d_mbs;
    a.coefs = s.d_coefs;
    a.mbw = g.mbw, a.mbh = g.mbh, a.cf = g.cf;
    a.dtype = dtype, a.flags = flags;
    a.y = y, a.cb = cb, a.cr = cr;
    // the order list's copy is in flight: its events are recorded whether or not the launch succeeded
    int rc = residual_begin(c);
    const hipError_t le = rc == MP2VG_OK ? launch_residual(a, n, s.stream) : hipSuccess;
    const int rc2 = residual_enqueued(c);
    HIPCHK(le);
    return rc ? rc : rc2;
}
