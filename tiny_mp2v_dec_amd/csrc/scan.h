// scan.h — the host scan of an elementary stream (mp2vg_scan_es, parse.cpp): pass 1 of the parse
// on its own, plus what the slice parser of slice_parse.h needs per picture and per slice.  Shared
// by parse.cpp (the scan, the CPU twin) and parse_dev.cpp (the device upload).
#pragma once
#include <vector>

#include "slice_parse.h"

struct mp2vg_scan {
    const uint8_t* buf = nullptr;  // the caller's stream: it must outlive the scan
    uint64_t len = 0;
    mp2vg_config_t cfg{};
    mp2vg::SpGeom g{};
    std::vector<mp2vg_picture_t> pics;
    std::vector<int32_t> display, gop, shard;
    std::vector<uint32_t> flags;           // MP2VG_PIC_* per picture
    int32_t nshards = 0;
    mp2vg_stream_headers_t hdrs{};
    std::vector<mp2vg::SpPicHdr> hdr;      // per picture
    std::vector<mp2vg::SpSlice> slices;    // stream order; byte offsets into buf
    std::vector<uint32_t> pic_slice;       // picture p's slices: [pic_slice[p], pic_slice[p + 1])
};

namespace mp2vg {

// bytes kept readable (zero) after the bitstream span handed to the slice parser
constexpr uint64_t kSpanPad = 16;

// The flat decode tables (built once from Tables::get()): T.w points at the host copy, whose
// nwords words a device copy mirrors with the same offsets.
void sp_tables(const uint32_t** words, size_t* nwords, SpTables* T);

// byte span [*lo, *hi) of the slices of pictures [first, first + npics)
void scan_span(const mp2vg_scan* s, int32_t first, int32_t npics, uint64_t* lo, uint64_t* hi);

// "picture %d slice @%llu: <reason>" — the host emitter's error format
void sp_set_slice_error(int pic, uint64_t byte_off, int reason);

}  // namespace mp2vg
