// parse_kernel.h — the device parse (parse.hip): one lane per slice runs slice_parse.h.  Shared
// by the kernels, their launchers' caller (parse_dev.cpp: mp2vg_batch_upload_es) and the
// context's side of it (runtime.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "slice_parse.h"

namespace mp2vg {

// a slice of the uploaded span: SpSlice with 32-bit offsets from the span's first byte
struct DevSlice {
    uint32_t pic;       // index into the batch's pictures (and headers)
    uint32_t mb_row;
    uint32_t byte_off, byte_end;
};

struct ParseArgs {
    SpTables T;              // T.w: the device copy of the tables
    SpGeom G;
    const SpPicHdr* hdr;     // per picture of the batch
    const uint32_t* mb_first;  // per picture: its first MB record
    const DevSlice* slices;
    uint32_t nslices;
    const uint8_t* bs;       // the span, 4-byte aligned, kSpanPad readable zero bytes after it
    uint32_t span;           // bytes: the reader's hard end
    mp2vg_mb_t* mbs;         // the batch's MB records
    uint32_t* coefs;         // the batch's coefficient words (emit pass)
    SpResult* res;           // per slice (count pass)
    uint32_t* base;          // per slice: first word (scan); base[nslices] = total
    uint32_t* uses;          // per picture: bit 0 forward, bit 1 backward (scan)
    uint32_t npics;
    uint32_t conceal;        // MP2VG_PARSE_CONCEAL: failed slices and missing rows become replacement rows
    uint32_t rows;           // MP2VG_PARSE_SLICES: a row has a run of entries; the row kernel applies the cover rule
};

// workgroup = one wave of 64 lanes, lane = slice
hipError_t launch_parse_count(const ParseArgs& a, hipStream_t stream);
// MP2VG_PARSE_SLICES (a.rows; otherwise nothing is launched): after the count pass, before the
// conceal kernel and the scan
hipError_t launch_parse_rows(const ParseArgs& a, hipStream_t stream);
// MP2VG_PARSE_CONCEAL (a.conceal; otherwise nothing is launched): after the count pass, before the scan
hipError_t launch_parse_conceal(const ParseArgs& a, hipStream_t stream);
// pic_slice[npics + 1]: each picture's slice range; summary[3]: total words, first failing slice
// that is not concealed, concealed slices
hipError_t launch_parse_scan(const ParseArgs& a, const uint32_t* pic_slice, unsigned long long* summary,
                             hipStream_t stream);
hipError_t launch_parse_emit(const ParseArgs& a, hipStream_t stream);

// the context's side (runtime.cpp)
struct EsBank {
    int device;
    hipStream_t stream;  // the bank's upload stream: the passes run on it, behind the copies
    mp2vg_mb_t* d_mbs;
    void** state;                // the context's slot for parse_dev.cpp's state
    void (**state_free)(void*);
};
int es_begin(mp2vg_ctx* c, const mp2vg_picture_t* pics, int32_t npics, uint64_t nmbs, EsBank* out);
int es_coefs(mp2vg_ctx* c, uint64_t ncoefs, uint32_t** d_coefs);
int es_commit(mp2vg_ctx* c, const mp2vg_picture_t* pics, int32_t npics, uint64_t nmbs, uint64_t ncoefs,
              const uint8_t* uses_of);
void* ctx_es_state(mp2vg_ctx* c);
const mp2vg_config_t* ctx_config(const mp2vg_ctx* c);

}  // namespace mp2vg
