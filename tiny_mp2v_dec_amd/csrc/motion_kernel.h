// motion_kernel.h — the compressed-domain export (include/mp2vg.h "motion export"): the rule that
// maps one MB record to its 8 vector and 4 info values and one coefficient word to its activity
// terms, compiled for the kernels (motion.hip) and for the host twin (motion.cpp:
// mp2vg_motion_records) alike, plus the launch arguments and the context's side (runtime.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mp2vg.h"

#if defined(__HIPCC__)
#define MOTION_HD __host__ __device__ inline
#else
#define MOTION_HD inline
#endif

namespace mp2vg {

// One MB record as its 8 little-endian dwords (two 16-byte loads on the device): r[1] = flags |
// cbp << 16, r[2] = qscale | reserved << 8 | ncoef << 16, r[3] = coef_off, r[4 + 2 v + s] =
// mv[v][s] as x | y << 16.  mv[4 s + 2 r + k] and info[0..3] as mp2vg.h defines them.
MOTION_HD void motion_mb(const uint32_t r[8], int16_t mv[8], uint16_t info[4]) {
    const uint32_t flags = r[1] & 0xffffu;
    info[0] = (uint16_t)(flags & 0x0F1Fu);
    info[1] = (uint16_t)(r[1] >> 16);
    info[2] = (uint16_t)(r[2] & 0xffu);
    info[3] = (uint16_t)(r[2] >> 16);
    const bool inter = !(flags & MP2VG_MB_INTRA);
    const bool field = (flags & MP2VG_MB_FIELD_MC) != 0;
    for (int s = 0; s < 2; s++) {
        // the decode's own rule: a non-intra MB with neither direction bit predicts forward
        const bool used = inter && (s ? (flags & MP2VG_MB_BWD) != 0 : (flags & MP2VG_MB_FWD) || !(flags & MP2VG_MB_BWD));
        for (int v = 0; v < 2; v++) {
            const uint32_t w = r[4 + 2 * (field ? v : 0) + s];
            int32_t x = (int16_t)(w & 0xffffu), y = (int16_t)(w >> 16);
            if (field) {
                // field half-pels to frame half-pels: destination lines v, v + 2, ... read lines of
                // parity sel, so the displacement in frame lines is y + sel - v
                const int32_t sel = (flags & MP2VG_MB_FS_BIT(v, s)) ? 1 : 0;
                y = 2 * y + 2 * (sel - v);
            }
            mv[4 * s + 2 * v + 0] = (int16_t)(used ? x : 0);
            mv[4 * s + 2 * v + 1] = (int16_t)(used ? y : 0);
        }
    }
}

// One coefficient word of an MB with nb blocks: false when its block index is not a block of the
// chroma format (the word is ignored); else *block, and *mag = what it adds to plane 1 (|level| in
// 32 bits, 0 for a DC word; a '1s' word carries level +-1).  Plane 0 counts every such word.
MOTION_HD bool motion_word(uint32_t w, int nb, int* block, int32_t* mag) {
    const int b = (int)MP2VG_COEF_BLOCK(w);
    if (b >= nb) return false;
    const int32_t level = (int16_t)(w & 0xffffu);
    *block = b;
    *mag = (w & MP2VG_COEF_DC) ? 0 : (level < 0 ? -level : level);
    return true;
}

// One launch pair exports n pictures of the resident bank: picture f is pics[order[f]], its cell i
// the record mbs[mb_first + i].  Tensors as mp2vg.h lays them out; a null pointer is not written.
struct MotionArgs {
    const mp2vg_picture_t* pics;
    const mp2vg_mb_t* mbs;
    const uint32_t* coefs;  // readable up to 3 words past the last word of the batch (kCoefPad)
    const int32_t* order;   // n device entries, each inside the bank's pictures
    int32_t mbw, mbh, nb;   // geometry: MB columns, MB rows, blocks per MB
    int16_t* mv;
    uint16_t* info;
    int32_t* act;
};
// mv / info kernel when either is wanted, activity kernel when act is: grid z = n
hipError_t launch_motion(const MotionArgs& a, int n, hipStream_t stream);

// the context's side (runtime.cpp): the resident bank, as ExportSource is the slot pool
struct MotionSource {
    int device, nb;
    int32_t mbw, mbh, npics;
    const mp2vg_picture_t* d_pics;
    const mp2vg_mb_t* d_mbs;
    const uint32_t* d_coefs;
    hipStream_t stream;  // the context's main stream
};
// MP2VG_E_STATE when no batch is resident
int motion_source(const mp2vg_ctx* c, MotionSource* s);
// before the kernels: the main stream waits for the bank's records (the copies of
// mp2vg_batch_upload, or the emit pass of mp2vg_batch_upload_es)
int motion_begin(mp2vg_ctx* c);
// after the kernels: the staging ring's events (export_enqueued) and the bank's `consumed`
// event, which the upload that next reuses the bank waits for
int motion_enqueued(mp2vg_ctx* c);

}  // namespace mp2vg
