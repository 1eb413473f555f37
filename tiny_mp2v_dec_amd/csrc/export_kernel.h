// export_kernel.h — arguments of the Y'CbCr -> R'G'B' export kernel (export.hip), shared with the
// host entry points (export.cpp: mp2vg_export_slots / mp2vg_export_planes) and the context's side
// of them (runtime.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mp2vg.h"

namespace mp2vg {

// One launch exports n frames.  Frame f reads its three planes at
//   slots != nullptr:  ftab[slots[f]] + plane_off[p]     (frame-pool slots, as digest_kernel)
//   slots == nullptr:  planes[p]                          (caller's planes; n = 1)
// and writes the tight uint8 tensor at dst: planar [n][3][h][w] or packed [n][h][w][3].
struct ExportArgs {
    const uint64_t* ftab;
    const int32_t* slots;
    const uint8_t* planes[3];
    uint32_t plane_off[3];
    int32_t stride[3];  // bytes per plane row, multiples of 4; a plane row is readable over its stride
    int32_t cw, ch;     // coded chroma plane size (the clamp of the LINEAR taps)
    int32_t w, h;       // exported rectangle, top-left anchored
    int32_t cy, crv, cgu, cgv, cbu;  // mp2vg_export_coefficients
    int32_t kr, kg, kb;  // folded constants: 8192 - 16 cy - 128 (chroma coefficients of the channel)
    uint8_t* dst;
};

// cf 1..3, layout MP2VG_EXPORT_RGB_*, chroma MP2VG_EXPORT_CHROMA_*; grid = (units, rows / 4, n)
hipError_t launch_export(int cf, int layout, int chroma, const ExportArgs& a, int n, hipStream_t stream);

// the context's side (runtime.cpp)
struct ExportSource {
    int device, cf, nslots;
    int32_t pw, ph, cw, ch;  // coded luma and chroma plane sizes
    int32_t stride[3];
    uint32_t plane_off[3];
    const uint64_t* ftab;
    hipStream_t stream;  // the context's main stream
};
void export_source(const mp2vg_ctx* c, ExportSource* s);
// device copy of a slot list, enqueued on the main stream (MP2VG status); the tensor export
// (tensor.cpp) sends its tap tables behind the slots in the same list
int export_stage_slots(mp2vg_ctx* c, const int32_t* slots, int32_t n, const int32_t** d_slots);
// after the kernel: the events the next export and the next batch decode wait on
int export_enqueued(mp2vg_ctx* c);
int check_export(const mp2vg_export_t* e, int32_t coded_w, int32_t coded_h, int32_t* w, int32_t* h);

}  // namespace mp2vg
