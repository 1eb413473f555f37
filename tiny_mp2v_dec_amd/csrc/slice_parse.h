// slice_parse.h — one slice -> its macroblock row of records, as ONE source for the device
// kernels (parse.hip) and their CPU twin (mp2vg_scan_parse_host, parse.cpp).
//
// A restatement of parse.cpp's parse_slice (the tuned host emitter, which stays the yardstick):
// the same rules and quirks in the same order, the same bit reader with the same refill schedule
// (the host's overrun test reads the reader's byte pointer, which only refills move, so the
// schedule is part of the accept / reject behaviour), the same status for every rejection and a
// reason code whose text (sp_reason_text) is the host emitter's message.  Output goes through a
// policy: SpCountOut writes the records (coef_off relative to the slice) and counts the
// coefficient words, SpEmitOut writes the words at the slice's base and rebases coef_off.
//
// Plain C++: no std containers, no exceptions, no lambdas; tables are flat arrays (SpTables)
// built from Tables::get() on the host (sp_build_tables, parse.cpp).
//
// Safety (DESIGN.md "Device parse"): every bitstream read lies in [buf, buf + hend + 16) (the
// caller keeps 16 readable zero bytes after hend and a 4-byte aligned buf on the device), every
// record goes to row[x] with x < mbw checked first, every coefficient word to words[i] with
// i < cap checked first, and the number of loop iterations of one slice is at most
// sp_iter_bound(slice bytes, mbw), which the CPU twin asserts.
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/mp2vg.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SP_HD __host__ __device__ inline
#else
#define SP_HD inline
#endif

namespace mp2vg {

// ---- reason codes: one per slice-level rejection of the host emitter -----------------------
enum {
    SP_OK = 0,
    SP_R_ROW_OUTSIDE,       // scan
    SP_R_TWO_SLICES,        // scan
    SP_R_ROW_UNCOVERED,     // scan
    SP_R_MB_BEYOND_ROW,
    SP_R_BAD_MBA,
    SP_R_NOT_COLUMN0,
    SP_R_SKIP_IN_I,
    SP_R_SKIP_BEYOND_ROW,
    SP_R_SKIP_OUTSIDE_REF,
    SP_R_BAD_MBTYPE,
    SP_R_DUAL_PRIME,
    SP_R_RESERVED_MOTION_TYPE,
    SP_R_444_FIELD_DCT,
    SP_R_BAD_MOTION_CODE,
    SP_R_MISSING_REF,
    SP_R_MV_OUTSIDE_REF,
    SP_R_BAD_CBP,
    SP_R_INTRA_VLC0,
    SP_R_BAD_DC_SIZE,
    SP_R_BAD_COEF,
    SP_R_RUN_PAST_63,
    SP_R_OVERRUN,
    SP_R_ROW_NOT_WHOLE,
    SP_R_ROW_GAP,           // MP2VG_PARSE_SLICES: the row's slices leave columns uncovered (sp_cover_row)
    SP_R_ROW_OVERLAP,       // MP2VG_PARSE_SLICES: a slice starts before the one in front of it ended
    SP_R_COUNT
};

inline const char* sp_reason_text(int r) {
    switch (r) {
    case SP_R_ROW_OUTSIDE: return "slice row outside the picture";
    case SP_R_TWO_SLICES: return "two slices in one macroblock row";
    case SP_R_ROW_UNCOVERED: return "picture with a macroblock row not covered by any slice";
    case SP_R_MB_BEYOND_ROW: return "macroblock beyond the end of the row";
    case SP_R_BAD_MBA: return "bad macroblock_address_increment";
    case SP_R_NOT_COLUMN0: return "slice does not start at column 0";
    case SP_R_SKIP_IN_I: return "skipped macroblock in an I picture";
    case SP_R_SKIP_BEYOND_ROW: return "skip run beyond the end of the row";
    case SP_R_SKIP_OUTSIDE_REF: return "skipped MB reads outside the reference";
    case SP_R_BAD_MBTYPE: return "bad macroblock_type";
    case SP_R_DUAL_PRIME: return "dual-prime prediction";
    case SP_R_RESERVED_MOTION_TYPE: return "reserved frame_motion_type";
    case SP_R_444_FIELD_DCT: return "4:4:4 field DCT (reference misplaces blocks 10/11)";
    case SP_R_BAD_MOTION_CODE: return "bad motion_code";
    case SP_R_MISSING_REF: return "prediction from a missing reference";
    case SP_R_MV_OUTSIDE_REF: return "motion vector reads outside the reference";
    case SP_R_BAD_CBP: return "bad coded_block_pattern";
    case SP_R_INTRA_VLC0: return "intra macroblock with intra_vlc_format=0 (reference mis-parses)";
    case SP_R_BAD_DC_SIZE: return "bad dct_dc_size";
    case SP_R_BAD_COEF: return "bad DCT coefficient code";
    case SP_R_RUN_PAST_63: return "coefficient run past position 63";
    case SP_R_OVERRUN: return "slice overruns the buffer";
    case SP_R_ROW_NOT_WHOLE: return "slice does not cover the whole macroblock row";
    case SP_R_ROW_GAP: return "slices of a macroblock row leave a gap";
    case SP_R_ROW_OVERLAP: return "slices of a macroblock row overlap or are out of order";
    default: return "";
    }
}

// ---- inputs ---------------------------------------------------------------------------------
// Flat decode tables in one array of 32-bit words.  VLC entries are VlcLut's ((len << 16) |
// (index + 1), 0 = invalid), motion is Tables::motion_signed, coef1/coef2 are CoefLut's two
// levels for B.14 ([0]) and B.15 ([1]); the *_val arrays map a code's index to its value.
struct SpTables {
    const uint32_t* w;
    uint32_t mba, mbtype[4], cbp, motion, dc_luma, dc_chroma, coef1[2], coef2[2];
    uint32_t mba_val, mbtype_val[4], cbp_val, dc_luma_val, dc_chroma_val, rev6;
};

enum { SP_INTRA_TAB_REFUSED = 2 };

struct SpPicHdr {  // the per-picture device header
    uint8_t pct, f_code[2][2], intra_dc_precision, frame_pred_frame_dct, concealment_motion_vectors,
        q_scale_type, intra_vlc_format, has_fwd, has_bwd;
    uint8_t has_conceal_ref;  // I picture, MP2VG_PARSE_CONCEAL: an earlier anchor exists in decode order
    // the coefficient table of the picture's intra blocks, filled by the scan: 1 = B.15
    // (intra_vlc_format 1), 0 = B.14 (intra_vlc_format 0 under MP2VG_PARSE_STANDARD), SP_INTRA_TAB_REFUSED
    // = intra_vlc_format 0 without the flag.  The one byte the parser reads of the two settings.
    uint8_t intra_tab;
    // MP2VG_PARSE_SLICES, filled by the scan: 1 = a slice starts at the column its first
    // macroblock_address_increment names and ends where its macroblock loop ends (the rule below)
    uint8_t slices;
    uint8_t reserved[1];
};  // 16 bytes
static_assert(sizeof(SpPicHdr) == 16, "SpPicHdr is the 16-byte per-picture device header");

struct SpSlice {  // slice table entry; byte offsets into the scanned stream (or the uploaded span)
    int32_t pic, mb_row;
    uint64_t byte_off, byte_end;
};  // 24 bytes

struct SpGeom {
    int32_t cf, nblocks, mbw, mbh, vext;  // vext: slice_vertical_position_extension present
    int32_t pw[3], ph[3], mbw_c, mbh_c;
};

struct SpResult {  // per slice
    int32_t status, reason;
    uint32_t ncoef;     // coefficient words of the slice
    uint32_t fail_pos;  // reader byte position (from the slice's start code) at the rejection
    uint32_t uses;      // bit 0: a macroblock predicts forward, bit 1: backward
    uint32_t iters;     // loop iterations (bounded by sp_iter_bound)
    // the slice wrote records [x0, x1) of its row.  x1: the column after its last record (mbw of a
    // whole-row slice; the column of the rejection in a failed one)
    uint32_t x1;
    // MP2VG_PARSE_SLICES, set by the row pass (sp_slice_x0, sp_cover_row; 0 without it): the slice's
    // start column, what the emit pass does with the entry, and, of a replacement carrier, the
    // blamed entry, counted from the carrier.  The parse itself sets none of the four: keeping the
    // start column through the macroblock loop cost the count kernel 30 SGPR spills.
    uint16_t x0;
    uint8_t fate;
    uint8_t pad;
    uint32_t blame;
};  // 36 bytes

// SpResult.fate
enum {
    SP_FATE_PARSED = 0,   // the emit pass parses the slice (or, with a reason set and the flag clear, conceals its row)
    SP_FATE_CARRIER = 1,  // first entry of a replaced row: it owns the replacement row and its words
    SP_FATE_DROPPED = 2   // another entry of a replaced row: no words, and the emit pass writes nothing
};

// Upper bound on the loop iterations of one slice of `bytes` bytes.  The reader position is at
// most 8 bytes past the slice's end when a macroblock starts (the host's overrun test); one
// macroblock reads under 200 header bits and at most 12 x (20 + 64 x 24) block bits; the two
// header loops (extra slice information, macroblock escapes) stop in the 23 zero bits of the
// start code that ends the slice, or in the zeros past the buffer.  Every counted iteration
// consumes at least one bit, except a skipped macroblock (at most mbw of them).
SP_HD uint64_t sp_iter_bound(uint64_t bytes, int mbw) { return 8 * bytes + (uint64_t)mbw + 20480; }

// ---- bit reader: BitReader of syntax.h on offsets, same refill schedule -----------------------
SP_HD uint64_t sp_load8_be(const uint8_t* a) {
#if defined(__HIP_DEVICE_COMPILE__)
    // three aligned dword loads (vector loads) in place of one unaligned 8-byte load
    const uintptr_t u = (uintptr_t)a;
    const uint32_t* w = (const uint32_t*)(u & ~(uintptr_t)3);
    const uint32_t sh = (uint32_t)(u & 3) * 8;
    const uint64_t lo = (uint64_t)w[0] | ((uint64_t)w[1] << 32);
    const uint64_t hi = w[2];
    const uint64_t v = sh ? (lo >> sh) | (hi << (64 - sh)) : lo;
    return __builtin_bswap64(v);
#else
    uint64_t v;
    memcpy(&v, a, 8);
    return __builtin_bswap64(v);
#endif
}

struct SpReader {
    const uint8_t* buf;
    int64_t p, end, hend, lim;  // byte offsets from buf; lim < 0: no 8-byte load fits
    int64_t base;
    uint64_t cache;
    int bits;

    SP_HD void init(const uint8_t* b, int64_t off, int64_t e, int64_t hard_end) {
        buf = b;
        base = p = off;
        end = e;
        hend = hard_end;
        lim = hard_end - off >= 8 ? hard_end - 8 : -1;
        cache = 0;
        bits = 0;
    }
    SP_HD void refill() {
        if (p <= lim) {
            cache |= sp_load8_be(buf + p) >> bits;
            p += (63 - bits) >> 3;
            bits |= 56;
            return;
        }
        while (bits <= 56) {
            const uint64_t byte = (p < hend) ? buf[p] : 0;
            cache |= byte << (56 - bits);
            p++;
            bits += 8;
        }
    }
    SP_HD uint32_t peek(int n) {
        if (n == 0) return 0;
        refill();
        return (uint32_t)(cache >> (64 - n));
    }
    SP_HD void skip(int n) {  // n <= 32
        refill();
        cache <<= n;
        bits -= n;
    }
    SP_HD uint32_t read(int n) {
        if (n == 0) return 0;
        refill();
        const uint32_t v = (uint32_t)(cache >> (64 - n));
        cache <<= n;
        bits -= n;
        return v;
    }
    SP_HD uint32_t peek_nr(int n) const { return (uint32_t)(cache >> (64 - n)); }
    SP_HD void skip_nr(int n) {
        cache <<= n;
        bits -= n;
    }
    SP_HD bool overrun() const { return p > end + 8; }
};

// VlcLut::decode on a flat table: index or -1
SP_HD int sp_vlc(SpReader& br, const uint32_t* lut, int maxlen) {
    br.refill();
    const uint32_t e = lut[br.peek_nr(maxlen)];
    if (!e) return -1;
    br.skip_nr((int)(e >> 16));
    return (int)(e & 0xffff) - 1;
}

// CoefLut::decode_tab: 0 NORMAL (escapes included), 1 EOB, -1 invalid
SP_HD int sp_coef(const uint32_t* t1, const uint32_t* t2, SpReader& br, int& run, int& level) {
    uint32_t e = t1[br.peek_nr(12)];
    if (((e >> 23) & 3) == 3) {
        br.skip_nr(12);
        e = t2[(((e >> 5) & 0x3ffff) << 5) + br.peek_nr(5)];
    }
    const int len = (int)(e & 31);
    if (!len) return -1;
    const int kind = (int)((e >> 23) & 3);
    const uint32_t esc = 0u - (uint32_t)(kind == 2);
    const uint32_t x = (uint32_t)((br.cache << 6) >> 46);
    const uint32_t rl_norm = (e >> 5) & 0x3ffffu;
    const uint32_t rl = (rl_norm & ~esc) | (((x >> 12) | ((x & 0xfffu) << 6)) & esc);
    run = (int)(rl & 63);
    level = (int32_t)(rl << 14) >> 20;
    br.skip_nr(len);
    return kind & ~(int)(esc & 2u);
}

SP_HD int sp_qscale(int code, int q_scale_type) {
    if (!q_scale_type) return code << 1;
    if (code < 9) return code;
    if (code < 17) return (code - 4) << 1;
    if (code < 25) return (code - 10) << 2;
    return (code - 17) << 3;
}

SP_HD int16_t sp_mv_reconstruct(int f_code, int motion_code, int residual, int16_t& PMV, bool field_vert) {
    const int r_size = f_code - 1;
    const int f = 1 << r_size;
    const int high = 16 * f - 1, low = -16 * f, range = 32 * f;
    const int a = motion_code < 0 ? -motion_code : motion_code;
    const int d = (a - 1) * f + residual + 1;
    int delta = motion_code < 0 ? -d : d;
    delta = motion_code != 0 ? delta : 0;
    const int prediction = field_vert ? (PMV >> 1) : PMV;
    int mv = prediction + delta;
    if (mv < low) mv += range;
    if (mv > high) mv -= range;
    const int16_t MV = (int16_t)mv;
    PMV = field_vert ? (int16_t)(MV * 2) : MV;
    return MV;
}

SP_HD bool sp_mc_reads_inside(const SpGeom& g, int mbx, int mby, int mvx, int mvy, bool field, int fs) {
    for (int plane = 0; plane < 3; plane++) {
        int mx = mvx, my = mvy;
        if (plane > 0) {
            if (g.cf < 3) mx >>= 1;
            if (g.cf < 2) my >>= 1;
        }
        const int w = plane == 0 ? 16 : g.mbw_c;
        const int h = plane == 0 ? 16 : g.mbh_c;
        const int x0 = mbx * w + (mx >> 1);
        const int x1 = x0 + w - 1 + (mx & 1);
        int y0, y1;
        if (!field) {
            y0 = mby * h + (my >> 1);
            y1 = y0 + h - 1 + (my & 1);
        } else {
            const int hf = h >> 1;
            y0 = mby * h + fs + 2 * (my >> 1);
            y1 = y0 + 2 * (hf - 1) + 2 * (my & 1);
        }
        if (x0 < 0 || y0 < 0 || x1 > g.pw[plane] - 1 || y1 > g.ph[plane] - 1) return false;
    }
    return true;
}

// ---- output policies ------------------------------------------------------------------------
// count pass: the row's records (coef_off relative to the slice), no coefficient words
struct SpCountOut {
    mp2vg_mb_t* row;  // mbw records
    SP_HD void record(int x, const mp2vg_mb_t& m) const { row[x] = m; }
    SP_HD void word(uint32_t, uint32_t) const {}
};
// emit pass: the words at the slice's base, and the base added to the row's coef_off
struct SpEmitOut {
    mp2vg_mb_t* row;
    uint32_t* words;  // the slice's words: [base, base + cap)
    uint32_t cap;     // as counted by the count pass
    uint32_t base;
    SP_HD void record(int x, const mp2vg_mb_t& m) const { row[x].coef_off = m.coef_off + base; }
    SP_HD void word(uint32_t i, uint32_t w) const {
        if (i < cap) words[i] = w;
    }
};
// neither (the CPU twin's plain count)
struct SpNullOut {
    SP_HD void record(int, const mp2vg_mb_t&) const {}
    SP_HD void word(uint32_t, uint32_t) const {}
};

#define SP_FAIL(code, why)                       \
    do {                                         \
        res.status = (code);                     \
        res.reason = (why);                      \
        res.ncoef = nw;                          \
        res.fail_pos = (uint32_t)(br.p - br.base); \
        res.uses = uses;                         \
        res.iters = iters;                       \
        res.x1 = (uint32_t)x;                    \
        return;                                  \
    } while (0)

// One slice.  buf + [off, end) is the slice (start code first), bytes at or past hend read as 0.
// The slice's row comes from the slice table (the scan read and checked it): the header's row
// bits are skipped here.
//
// MP2VG_PARSE_SLICES (h.slices), the rule for a slice that is a part of its row: the slice's first
// macroblock_address_increment (escapes included) names its start column x0 = increment - 1.  It is
// no skip run: no records are written for it, it is legal in an I picture, and it resets nothing (the
// predictors and the quantiser scale start from the slice header as ever).  x0 >= mbw is "macroblock
// beyond the end of the row".  The slice ends at the column x1 where its macroblock loop ends;
// SP_R_NOT_COLUMN0 and SP_R_ROW_NOT_WHOLE are not produced, and whether the row's slices tile
// [0, mbw) is sp_cover_row's to say.  The slice writes records [x0, x1) only.  res.x1 is set here,
// res.x0 by the row pass (sp_slice_x0 reads the increment again).
template <class Out>
SP_HD void sp_parse_slice(const SpTables& T, const SpGeom& G, const SpPicHdr& h, const uint8_t* buf, int64_t off,
                          int64_t end, int64_t hend, int mb_row, const Out& out, SpResult& res) {
    const int pct = h.pct;
    const int cf = G.cf;
    const int nblocks = G.nblocks;
    const int mbw = G.mbw;
    uint32_t nw = 0, uses = 0, iters = 0;
    SpReader br;
    br.init(buf, off, end, hend);

    // slice header
    br.skip(24);
    (void)br.read(8);
    if (G.vext) (void)br.read(3);
    const int qcode = (int)br.read(5);
    if (br.peek(1) == 1) {
        br.skip(1 + 1 + 1 + 6);
        while (br.peek(1) == 1) {
            br.skip(9);
            iters++;
        }
    }
    br.skip(1);

    int16_t PMVs[2][2][2] = {};
    uint16_t dc_pred[3];
    const uint16_t dc_reset = (uint16_t)(1 << (h.intra_dc_precision + 7));
    dc_pred[0] = dc_pred[1] = dc_pred[2] = dc_reset;
    int qscale = sp_qscale(qcode, h.q_scale_type);
    uint32_t previous_mb_type = 0;
    int x = 0;
    const uint32_t* const w = T.w;

    do {
        iters++;
        if (x >= mbw) SP_FAIL(MP2VG_E_BITSTREAM, SP_R_MB_BEYOND_ROW);
        int inc = 0;
        while (br.peek(11) == 0x008) {
            br.skip(11);
            inc += 33;
            iters++;
        }
        const int e = sp_vlc(br, w + T.mba, 11);
        if (e < 0 || e >= 33) SP_FAIL(MP2VG_E_BITSTREAM, SP_R_BAD_MBA);
        inc += (int)w[T.mba_val + e];
        // (x is 0 at a slice's first macroblock only.)  MP2VG_PARSE_SLICES: the slice's first increment is
        // its start column, not a skip run: x moves there (at most to mbw, which the test after the skip
        // run refuses) and the increment counts as 1.  Selects, not a branch of its own.
        const bool start = x == 0 && h.slices;
        if (x == 0 && inc != 1 && !start) SP_FAIL(MP2VG_E_UNSUPPORTED, SP_R_NOT_COLUMN0);
        const uint32_t ahead = (uint32_t)(inc - 1) < (uint32_t)mbw ? (uint32_t)(inc - 1) : (uint32_t)mbw;
        x += start ? (int)ahead : 0;
        inc = start ? 1 : inc;
        if (inc > 1) {
            if (pct == 1) SP_FAIL(MP2VG_E_UNSUPPORTED, SP_R_SKIP_IN_I);
            if (pct == 2)
                for (int r = 0; r < 2; r++)
                    for (int s = 0; s < 2; s++) PMVs[r][s][0] = PMVs[r][s][1] = 0;
            for (int i = 0; i < inc - 1; i++) {
                iters++;
                if (x >= mbw) SP_FAIL(MP2VG_E_BITSTREAM, SP_R_SKIP_BEYOND_ROW);
                // emit_skipped
                mp2vg_mb_t m;
                memset(&m, 0, sizeof(m));
                m.x = (uint16_t)x;
                m.y = (uint16_t)mb_row;
                m.qscale = (uint8_t)qscale;
                m.coef_off = nw;
                const uint32_t t = previous_mb_type;
                bool fwd = (t & 0x10) != 0;
                const bool bwd = (t & 0x08) != 0;
                if (!fwd && !bwd) fwd = true;
                m.flags = (uint16_t)((fwd ? MP2VG_MB_FWD : 0) | (bwd ? MP2VG_MB_BWD : 0));
                const int vsel = (pct == 3) ? 1 : 0;
                for (int s = 0; s < 2; s++)
                    for (int c = 0; c < 2; c++) m.mv[0][s][c] = PMVs[vsel][s][c];
                bool ok = true;
                for (int s = 0; s < 2 && ok; s++) {
                    if (!((s == 0 && fwd) || (s == 1 && bwd))) continue;
                    if (!(s == 0 ? h.has_fwd : h.has_bwd)) ok = false;
                    else if (!sp_mc_reads_inside(G, x, mb_row, m.mv[0][s][0], m.mv[0][s][1], false, 0)) ok = false;
                }
                // (the host emitter writes the record before it tests it)
                out.record(x, m);
                if (!ok) SP_FAIL(MP2VG_E_UNSUPPORTED, SP_R_SKIP_OUTSIDE_REF);
                uses |= (fwd ? 1u : 0u) | (bwd ? 2u : 0u);
                x++;
            }
        }
        if (x >= mbw) SP_FAIL(MP2VG_E_BITSTREAM, SP_R_MB_BEYOND_ROW);

        // macroblock_modes
        const int te = sp_vlc(br, w + T.mbtype[pct], 6);
        if (te < 0) SP_FAIL(MP2VG_E_BITSTREAM, SP_R_BAD_MBTYPE);
        const uint32_t mbt = w[T.mbtype_val[pct] + te];
        const bool intra = (mbt & 0x02) != 0;
        const bool mfwd = (mbt & 0x10) != 0, mbwd = (mbt & 0x08) != 0, pattern = (mbt & 0x04) != 0;
        int frame_motion_type = 2;
        if ((mfwd || mbwd) && h.frame_pred_frame_dct == 0) frame_motion_type = (int)br.read(2);
        int dct_type = 0;
        if (h.frame_pred_frame_dct == 0 && (intra || pattern)) dct_type = (int)br.read(1);
        bool field_mv = false;
        int mv_count = 1;
        if (!intra && (mfwd || mbwd)) {
            if (frame_motion_type == 1) {
                field_mv = true;
                mv_count = 2;
            } else if (frame_motion_type == 3) {
                SP_FAIL(MP2VG_E_UNSUPPORTED, SP_R_DUAL_PRIME);
            } else if (frame_motion_type != 2) {
                SP_FAIL(MP2VG_E_BITSTREAM, SP_R_RESERVED_MOTION_TYPE);
            }
        }
        if (mbt & 0x20) qscale = sp_qscale((int)br.read(5), h.q_scale_type);
        if (cf == 3 && dct_type && (intra || pattern)) SP_FAIL(MP2VG_E_UNSUPPORTED, SP_R_444_FIELD_DCT);

        // motion_vectors
        int16_t MVs[2][2][2] = {};
        int fsel[2][2] = {};
        // (no concealment vectors: the scan rejects pictures that carry them)
        for (int s = 0; s < 2; s++) {
            if (!(s == 0 ? mfwd : mbwd)) continue;
            for (int r = 0; r < mv_count; r++) {
                if (mv_count == 2 || field_mv) fsel[r][s] = (int)br.read(1);
                for (int t = 0; t < 2; t++) {
                    br.refill();
                    const uint32_t me = w[T.motion + br.peek_nr(11)];
                    if (!me) SP_FAIL(MP2VG_E_BITSTREAM, SP_R_BAD_MOTION_CODE);
                    br.skip_nr((int)(me >> 16));
                    const int mc = (int)(me & 0xffffu) - 32;
                    const int fc = h.f_code[s][t];
                    const int n = mc != 0 ? fc - 1 : 0;
                    const int residual = (int)(((br.cache >> 1) >> (63 - n)) & ((1u << n) - 1u));
                    br.skip_nr(n);
                    MVs[r][s][t] = sp_mv_reconstruct(fc, mc, residual, PMVs[r][s][t], field_mv && t == 1);
                }
            }
        }

        // PMV update + MC selection
        mp2vg_mb_t m;
        memset(&m, 0, sizeof(m));
        m.x = (uint16_t)x;
        m.y = (uint16_t)mb_row;
        if (pct != 1) {
            const bool frame_based = intra || !field_mv;
            if (frame_based) {
                if (intra) {
                    for (int t = 0; t < 2; t++) PMVs[1][0][t] = PMVs[0][0][t];
                } else if (mfwd && mbwd) {
                    for (int t = 0; t < 2; t++) {
                        PMVs[1][0][t] = PMVs[0][0][t];
                        PMVs[1][1][t] = PMVs[0][1][t];
                    }
                } else if (mfwd) {
                    for (int t = 0; t < 2; t++) PMVs[1][0][t] = PMVs[0][0][t];
                } else if (mbwd) {
                    for (int t = 0; t < 2; t++) PMVs[1][1][t] = PMVs[0][1][t];
                }
            }
            const bool no_mc_p = (pct == 2 && !intra && !mfwd);
            if (intra || no_mc_p) {
                for (int r = 0; r < 2; r++)
                    for (int s = 0; s < 2; s++) {
                        PMVs[r][s][0] = PMVs[r][s][1] = 0;
                        MVs[r][s][0] = MVs[r][s][1] = 0;
                    }
                field_mv = false;
            }
            if (!intra) {
                const bool fwd = mfwd || no_mc_p, bwd = mbwd;
                m.flags = (uint16_t)((fwd ? MP2VG_MB_FWD : 0) | (bwd ? MP2VG_MB_BWD : 0) |
                                     (field_mv ? MP2VG_MB_FIELD_MC : 0));
                const int nv = field_mv ? 2 : 1;
                for (int r = 0; r < nv; r++)
                    for (int s = 0; s < 2; s++) {
                        if (!((s == 0 && fwd) || (s == 1 && bwd))) continue;
                        if (!(s == 0 ? h.has_fwd : h.has_bwd)) {
                            out.record(x, m);
                            SP_FAIL(MP2VG_E_UNSUPPORTED, SP_R_MISSING_REF);
                        }
                        m.mv[r][s][0] = MVs[r][s][0];
                        m.mv[r][s][1] = MVs[r][s][1];
                        if (field_mv && fsel[r][s]) m.flags |= (uint16_t)MP2VG_MB_FS_BIT(r, s);
                        if (!sp_mc_reads_inside(G, x, mb_row, MVs[r][s][0], MVs[r][s][1], field_mv, fsel[r][s])) {
                            out.record(x, m);
                            SP_FAIL(MP2VG_E_UNSUPPORTED, SP_R_MV_OUTSIDE_REF);
                        }
                    }
                uses |= (fwd ? 1u : 0u) | (bwd ? 2u : 0u);
            }
        }
        if (intra) m.flags |= MP2VG_MB_INTRA;

        if (inc > 1 || !intra) dc_pred[0] = dc_pred[1] = dc_pred[2] = dc_reset;

        // coded_block_pattern
        uint32_t cbp = intra ? 0xfffu : 0;
        if (pattern) {
            const int ci = sp_vlc(br, w + T.cbp, 9);
            if (ci < 0) {
                out.record(x, m);
                SP_FAIL(MP2VG_E_BITSTREAM, SP_R_BAD_CBP);
            }
            const uint32_t v = w[T.cbp_val + ci];
            uint32_t c1 = 0, c2 = 0;
            if (cf == 2) c1 = br.read(2);
            if (cf == 3) c2 = br.read(6);
            cbp |= w[T.rev6 + (v & 63)];
            if (cf == 2) cbp |= (uint32_t)(((c1 & 1) << 1) | ((c1 >> 1) & 1)) << 6;
            if (cf == 3) cbp |= w[T.rev6 + (c2 & 63)] << 6;
        }
        cbp &= (1u << nblocks) - 1;
        if (dct_type && (intra || pattern)) m.flags |= MP2VG_MB_DCT_FIELD;
        m.cbp = (uint16_t)cbp;
        m.qscale = (uint8_t)qscale;
        m.coef_off = nw;
        // (the record as the host emitter leaves it when a block fails: ncoef 0)
        // (intra_vlc_format = 0: refused, or under MP2VG_PARSE_STANDARD the block goes on in B.14 after
        // its DC, in the table's "subsequent coefficient" form, which is what coef1[0] / coef2[0] hold)
        if (intra && h.intra_tab > 1) {  // SP_INTRA_TAB_REFUSED (any value that names no table)
            out.record(x, m);
            SP_FAIL(MP2VG_E_UNSUPPORTED, SP_R_INTRA_VLC0);
        }

        // blocks
        const int tab = intra ? h.intra_tab : 0;
        const uint32_t* const lut1 = w + T.coef1[tab];
        const uint32_t* const lut2 = w + T.coef2[tab];
        const uint32_t mbx_tag = MP2VG_COEF_MBX(x);
        const uint32_t n0 = nw;
        for (uint32_t bits = cbp; bits; bits &= bits - 1) {
            iters++;
            const int b = __builtin_ctz(bits);
            int i = 0;
            const uint32_t btag = ((uint32_t)b << 22) | mbx_tag;
            if (intra) {
                const int pidx = b < 4 ? 0 : ((b & 1) ? 2 : 1);
                const int si = sp_vlc(br, w + (b < 4 ? T.dc_luma : T.dc_chroma), b < 4 ? 9 : 10);
                if (si < 0) {
                    out.record(x, m);
                    SP_FAIL(MP2VG_E_BITSTREAM, SP_R_BAD_DC_SIZE);
                }
                const int size = (int)w[(b < 4 ? T.dc_luma_val : T.dc_chroma_val) + si];
                const int d = (int)(((br.cache >> 1) >> (63 - size)) & ((1u << size) - 1u));
                br.skip_nr(size);
                const int half = (1 << size) >> 1;
                const int diff = d >= half ? d : (d + 1) - 2 * half;
                dc_pred[pidx] = (uint16_t)(dc_pred[pidx] + diff);
                const int16_t dcv = (int16_t)(dc_pred[pidx] << (3 - h.intra_dc_precision));
                out.word(nw++, MP2VG_COEF_PACK(dcv, 0, b, MP2VG_COEF_DC | MP2VG_COEF_MBX(x)));
                i = 1;
            } else {
                const uint32_t c = br.peek(2);
                const uint32_t f = c >> 1;
                if (f) out.word(nw++, MP2VG_COEF_PACK(1 - 2 * (int)(c & 1), 0, b, MP2VG_COEF_FIRST1S | MP2VG_COEF_MBX(x)));
                br.skip_nr(2 * (int)f);
                i = (int)f;
            }
            // at most 64 words per block: i grows by at least 1 per word and stops past 63
            for (;;) {
                int run, level;
                br.refill();
                iters++;
                int kind = sp_coef(lut1, lut2, br, run, level);
                if (kind != 0) {
                    if (kind < 0) {
                        out.record(x, m);
                        SP_FAIL(MP2VG_E_BITSTREAM, SP_R_BAD_COEF);
                    }
                    break;
                }
                i += run;
                if (i > 63) {
                    out.record(x, m);
                    SP_FAIL(MP2VG_E_BITSTREAM, SP_R_RUN_PAST_63);
                }
                out.word(nw++, ((uint32_t)level & 0xffffu) | ((uint32_t)i << 16) | btag);
                i++;
                iters++;
                kind = sp_coef(lut1, lut2, br, run, level);
                if (kind != 0) {
                    if (kind < 0) {
                        out.record(x, m);
                        SP_FAIL(MP2VG_E_BITSTREAM, SP_R_BAD_COEF);
                    }
                    break;
                }
                i += run;
                if (i > 63) {
                    out.record(x, m);
                    SP_FAIL(MP2VG_E_BITSTREAM, SP_R_RUN_PAST_63);
                }
                out.word(nw++, ((uint32_t)level & 0xffffu) | ((uint32_t)i << 16) | btag);
                i++;
            }
        }
        m.ncoef = (uint16_t)(nw - n0);
        out.record(x, m);
        if (br.overrun()) SP_FAIL(MP2VG_E_BITSTREAM, SP_R_OVERRUN);
        previous_mb_type = mbt;
        x++;
    } while (br.peek(23) != 0);
    if (x != mbw && !h.slices) SP_FAIL(MP2VG_E_UNSUPPORTED, SP_R_ROW_NOT_WHOLE);
    SP_FAIL(MP2VG_OK, SP_OK);
}

#undef SP_FAIL

// ---- concealment (MP2VG_PARSE_CONCEAL, include/mp2vg.h): the one statement of the rule -------
// A slice that failed for one of these reasons, or a row no slice covers, is replaced as a whole
// row.  SP_R_ROW_OUTSIDE and SP_R_TWO_SLICES stay rejections: such a slice names no row of its own.
SP_HD bool sp_reason_concealed(int reason) {
    return reason == SP_R_ROW_UNCOVERED || (reason >= SP_R_MB_BEYOND_ROW && reason <= SP_R_ROW_OVERLAP);
}

// ---- row pass (MP2VG_PARSE_SLICES) ----------------------------------------------------------------
// The start column of a slice: its header and its first macroblock_address_increment read again,
// exactly as sp_parse_slice reads them.  At most mbw; 0 where the increment's code is invalid (the
// parse has failed the slice there, and a failed slice's columns are never looked at).
SP_HD uint32_t sp_slice_x0(const SpTables& T, const SpGeom& G, const uint8_t* buf, int64_t off, int64_t end, int64_t hend) {
    SpReader br;
    br.init(buf, off, end, hend);
    br.skip(24);
    (void)br.read(8);
    if (G.vext) (void)br.read(3);
    (void)br.read(5);
    if (br.peek(1) == 1) {
        br.skip(1 + 1 + 1 + 6);
        while (br.peek(1) == 1) br.skip(9);  // (ends in the zeros of the next start code or past the buffer)
    }
    br.skip(1);
    uint32_t inc = 0;
    while (br.peek(11) == 0x008) {
        br.skip(11);
        inc += 33;
    }
    const int e = sp_vlc(br, T.w + T.mba, 11);
    if (e < 0 || e >= 33) return 0;
    inc += T.w[T.mba_val + e];
    return inc - 1 < (uint32_t)G.mbw ? inc - 1 : (uint32_t)G.mbw;
}

// ---- row cover (MP2VG_PARSE_SLICES): the one statement of the rule ----------------------------
// r[0 .. n) are the count pass's results of the slices of one macroblock row, in table order (the
// scan keeps a row's entries consecutive).  They must tile [0, mbw): the first starts at column 0,
// each next one where the one before it ended, the last ends at mbw.  The row breaks at its first
// entry, in table order, that failed its parse, starts past the expected column (SP_R_ROW_GAP) or
// before it (SP_R_ROW_OVERLAP); a row whose entries all fit but end short breaks at its last entry
// (SP_R_ROW_GAP).  That entry is blamed: a cover failure is written into its status and reason
// (MP2VG_E_UNSUPPORTED), a parse failure is there already.
// Under MP2VG_PARSE_CONCEAL a row that breaks for a concealable reason is replaced as a whole: its
// first entry becomes the carrier (the blamed entry's status, reason and fail_pos, blame = its
// distance), which the conceal step fills with sp_conceal_row as it does any failed slice; every
// other entry is dropped (status OK, no words, nothing to emit).
SP_HD void sp_cover_row(SpResult* r, uint32_t n, int mbw, bool conceal) {
    uint32_t blame = n;
    int32_t status = MP2VG_OK, reason = SP_OK;
    int expect = 0;
    for (uint32_t k = 0; k < n; k++) {
        if (r[k].status != MP2VG_OK) {
            blame = k, status = r[k].status, reason = r[k].reason;
            break;
        }
        const int x0 = (int)r[k].x0;
        if (x0 != expect) {
            blame = k, status = MP2VG_E_UNSUPPORTED, reason = x0 > expect ? SP_R_ROW_GAP : SP_R_ROW_OVERLAP;
            break;
        }
        expect = (int)r[k].x1;
    }
    if (blame == n) {
        if (expect == mbw) return;
        blame = n - 1, status = MP2VG_E_UNSUPPORTED, reason = SP_R_ROW_GAP;
    }
    if (!(conceal && sp_reason_concealed(reason))) {
        r[blame].status = status;
        r[blame].reason = reason;
        return;
    }
    const uint32_t fail_pos = r[blame].fail_pos;
    for (uint32_t k = 1; k < n; k++) {
        r[k].status = MP2VG_OK;
        r[k].reason = SP_OK;
        r[k].ncoef = 0;
        r[k].uses = 0;
        r[k].fate = SP_FATE_DROPPED;
    }
    r[0].status = status;
    r[0].reason = reason;
    r[0].fail_pos = fail_pos;
    r[0].fate = SP_FATE_CARRIER;
    r[0].blame = blame;
}

// The replacement row of picture h, through an output policy (the parser's: SpCountOut writes the
// records with coef_off relative to the row, SpEmitOut writes the words and rebases coef_off).
// Every record of the row is written, so nothing the failed parse left behind survives.  Returns
// the row's word count; `uses` as SpResult.uses.  Calls out.record(x, .) for x in [0, mbw) and
// out.word(i, .) for i below the returned count only.
template <class Out>
SP_HD uint32_t sp_conceal_row(const SpGeom& G, const SpPicHdr& h, int mb_row, const Out& out, uint32_t& uses) {
    // the reference the row is copied from: 0 forward, 1 backward, -1 none (grey)
    int dir = -1;
    if (h.pct == 2) dir = 0;
    else if (h.pct == 3) dir = h.has_fwd ? 0 : (h.has_bwd ? 1 : -1);
    else if (h.has_conceal_ref) dir = 0;
    uses = dir < 0 ? 0u : 1u << dir;
    const int16_t grey = (int16_t)((1 << (h.intra_dc_precision + 7)) << (3 - h.intra_dc_precision));
    uint32_t nw = 0;
    for (int x = 0; x < G.mbw; x++) {
        mp2vg_mb_t m;
        memset(&m, 0, sizeof(m));
        m.x = (uint16_t)x;
        m.y = (uint16_t)mb_row;
        m.qscale = 1;
        m.coef_off = nw;
        if (dir >= 0) {
            m.flags = (uint16_t)(dir == 0 ? MP2VG_MB_FWD : MP2VG_MB_BWD);
        } else {
            m.flags = MP2VG_MB_INTRA;
            m.cbp = (uint16_t)((1u << G.nblocks) - 1);
            m.ncoef = (uint16_t)G.nblocks;
            for (int b = 0; b < G.nblocks; b++)
                out.word(nw++, MP2VG_COEF_PACK(grey, 0, b, MP2VG_COEF_DC | MP2VG_COEF_MBX(x)));
        }
        out.record(x, m);
    }
    return nw;
}

}  // namespace mp2vg
