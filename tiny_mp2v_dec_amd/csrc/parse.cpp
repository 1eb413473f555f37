// parse.cpp — host record emitter: MPEG-2 elementary stream -> record stream (include/mp2vg.h).
//
// Reproduces the REFERENCE's parse semantics, quirks included, so that the
// records drive the device reconstruct to the reference's exact output:
//   start-code dispatch              decoder.cpp:278-329
//   header parsers                   mp2v_hdr.cpp:4-223, slice header mp2v_hdr.h:345-363
//   W matrices from the QME only     decoder.cpp:154-192
//   slice setup                      decoder.cpp:107-145
//   macroblock parse                 mb_decoder.cpp:341-641 (parse_modes, cbp, MVs, PMV rules,
//                                    skipped MBs, DC prediction, parse_block's VLC loop)
// Where the reference has undefined behaviour the stream is rejected (MP2VG_E_UNSUPPORTED):
// missing QME / partial loads, intra MBs with intra_vlc_format=0, field pictures, dual-prime,
// slices not starting at column 0, skipped MBs in I pictures, MC reads outside the reference
// planes, 4:4:4 with field DCT (reference writes blocks 10/11 outside the MB), concealment MVs
// (P/B pictures: the reference ignores the flag; I pictures: parse_modes leaves
// motion_vector_count 0 for intra macroblocks, mb_decoder.cpp:364-367, so parse_motion_vectors
// reads two field selects and two vectors, :512-517, where the stream holds one vector, and the
// parse derails: the reference crashed on the directed stream), scalable extensions.
// MP2VG_PARSE_STANDARD (include/mp2vg.h) lifts the first two: W comes from the matrix state of
// 13818-2 6.3.3 / 6.3.11 (MatrixState, kept by pass 1 in coding order), and an intra block of a
// picture with intra_vlc_format = 0 is read from B.14.  With the flag clear both stay as above.
// MP2VG_PARSE_SLICES lifts "slices not starting at column 0" and "one slice per row": the rule is
// stated in slice_parse.h (sp_parse_slice, sp_cover_row) and restated here (parse_slice, cover_rows).
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <thread>
#include <memory>
#include <condition_variable>
#include <mutex>
#include <vector>

#include "scan.h"
#include "syntax.h"

namespace mp2vg {

namespace {

struct PictureHdr {
    int pct = 0;
    int temporal_reference = 0;
    int f_code[2][2] = {{15, 15}, {15, 15}};
    int intra_dc_precision = 0;
    int picture_structure = 3;
    int frame_pred_frame_dct = 1;
    int concealment_motion_vectors = 0;
    int q_scale_type = 0;
    int intra_vlc_format = 0;
    int alternate_scan = 0;
    int top_field_first = 0, repeat_first_field = 0, progressive_frame = 0;
    bool have_pcext = false;
    bool have_qme = false;
    int qme_load[4] = {0, 0, 0, 0};
    uint8_t qme[4][64] = {};
    uint8_t state[4][64] = {};  // MP2VG_PARSE_STANDARD: the matrices in force after the picture's own extension
};

// The quantiser matrices in force (13818-2 6.3.3, 6.3.11), in the order the bitstream carries them
// (zigzag, as build_W expects): [0] intra, [1] non-intra, [2] chroma intra, [3] chroma non-intra.
struct MatrixState {
    uint8_t m[4][64];
    // a sequence_header: its matrices where it loads them (else NULL), the defaults where not
    void reset(const uint8_t* intra, const uint8_t* non_intra) {
        // the default intra matrix as 6.3.11 prints it, in raster order
        static const uint8_t kDefaultIntraRaster[64] = {
            8,  16, 19, 22, 26, 27, 29, 34, 16, 16, 22, 24, 27, 29, 34, 37, 19, 22, 26, 27, 29, 34,
            34, 38, 22, 22, 26, 27, 29, 34, 37, 40, 22, 26, 27, 29, 32, 35, 40, 48, 26, 27, 29, 32,
            35, 40, 48, 58, 26, 27, 29, 34, 38, 46, 56, 69, 27, 29, 35, 38, 46, 56, 69, 83};
        for (int i = 0; i < 64; i++) {
            m[0][i] = intra ? intra[i] : kDefaultIntraRaster[kScanRaster[0][i]];
            m[1][i] = non_intra ? non_intra[i] : 16;
        }
        memcpy(m[2], m[0], 64);
        memcpy(m[3], m[1], 64);
    }
    // a quant_matrix_extension, in its field order: a luma load also replaces its chroma matrix
    void load(const int loaded[4], const uint8_t q[4][64]) {
        for (int k = 0; k < 4; k++) {
            if (!loaded[k]) continue;
            memcpy(m[k], q[k], 64);
            if (k < 2) memcpy(m[k + 2], q[k], 64);
        }
    }
};

struct SliceJob {
    int pic;                  // decode index
    uint64_t byte_off;        // offset of the slice start code
    uint64_t byte_end;        // end of the slice payload (next start code)
    // MP2VG_PARSE_SLICES (parse_session_start): the row the start code names (-1: outside the
    // picture), and whether that row was seen earlier in the picture but not immediately before
    int row = -1;
    bool two = false;
};

struct PicWork {
    PictureHdr hdr;
    int fwd = -1, bwd = -1;   // decode indices of reference pictures (L0 / L1)
    int conceal_ref = -1;     // I picture: the newest anchor before it (MP2VG_PARSE_CONCEAL)
    uint64_t byte_off = 0;    // the picture start code
    int gop = -1;
    // a B picture between the first two anchors of a GOP with closed_gop = 1: it predicts only
    // backward (ISO 13818-2 6.3.8), so its forward reference is not a dependency for sharding
    bool closed_leading_b = false;
    uint8_t W[4][64] = {};
    std::vector<SliceJob> slices;
};

// allocator whose resize() leaves new elements uninitialised (the coefficient array is filled
// completely by the parallel concatenation; zeroing it first would be a serial memset)
template <class T>
struct NoInitAlloc : std::allocator<T> {
    template <class U>
    struct rebind {
        using other = NoInitAlloc<U>;
    };
    NoInitAlloc() = default;
    template <class U>
    NoInitAlloc(const NoInitAlloc<U>&) {}
    template <class U>
    void construct(U* p) {
        ::new ((void*)p) U;
    }
    template <class U, class... A>
    void construct(U* p, A&&... a) {
        ::new ((void*)p) U(std::forward<A>(a)...);
    }
};

// A slice's coefficient words: grown without zeroing and written through a raw pointer into a
// per-MB worst-case reservation (a std::vector resize per macroblock was 4 % of the parse)
struct CoefVec {
    uint32_t* d = nullptr;
    size_t n = 0, cap = 0;
    CoefVec() = default;
    CoefVec(const CoefVec&) = delete;
    CoefVec& operator=(const CoefVec&) = delete;
    CoefVec(CoefVec&& o) noexcept : d(o.d), n(o.n), cap(o.cap) { o.d = nullptr, o.n = o.cap = 0; }
    ~CoefVec() { free(d); }
    void swap(CoefVec& o) noexcept { std::swap(d, o.d), std::swap(n, o.n), std::swap(cap, o.cap); }
    uint32_t* data() { return d; }
    const uint32_t* data() const { return d; }
    size_t size() const { return n; }
    bool empty() const { return n == 0; }
    // room for at least `need` words (contents kept)
    bool reserve(size_t need) {
        if (need <= cap) return true;
        size_t c = std::max<size_t>(need, 2 * cap);
        uint32_t* nd = (uint32_t*)realloc(d, c * sizeof(uint32_t));
        if (!nd) return false;
        d = nd;
        cap = c;
        return true;
    }
};

struct SliceOut {
    CoefVec coefs;
    int mb_row = -1;
    int status = MP2VG_OK;
    std::string err;
    bool concealed = false;   // MP2VG_PARSE_CONCEAL: the row was replaced (status and err say why)
    int x0 = 0, x1 = 0;       // the records whose coef_off is relative to coefs: columns [x0, x1) of the row
};

struct Ctx {
    const uint8_t* buf;
    uint64_t len;
    Geom g;
    int width, height, mbw, mbh;
    int vertical_size_value = 0;
    bool conceal = false;     // MP2VG_PARSE_CONCEAL
    bool standard = false;    // MP2VG_PARSE_STANDARD
    bool slices = false;      // MP2VG_PARSE_SLICES
    std::vector<PicWork> pics;
    mp2vg_stream_headers_t hdrs{};
};

#define FAIL(code, msg)          \
    do {                         \
        out.status = (code);     \
        out.err = (msg);         \
        return;                  \
    } while (0)

// 6-bit reversal: coded_block_pattern bit (5 - i) names block i
static const uint8_t kRev6[64] = {
    0,  32, 16, 48, 8,  40, 24, 56, 4,  36, 20, 52, 12, 44, 28, 60, 2,  34, 18, 50, 10, 42,
    26, 58, 6,  38, 22, 54, 14, 46, 30, 62, 1,  33, 17, 49, 9,  41, 25, 57, 5,  37, 21, 53,
    13, 45, 29, 61, 3,  35, 19, 51, 11, 43, 27, 59, 7,  39, 23, 55, 15, 47, 31, 63};

// One slice -> its MB row of records (mb_decoder.cpp:521-641 for every MB of the slice).
void parse_slice(const Ctx& C, const PicWork& P, const SliceJob& job, mp2vg_mb_t* row_base_all,
                 std::atomic<uint8_t>* row_done, SliceOut& out) {
    const Tables& T = Tables::get();
    const PictureHdr& h = P.hdr;
    const int pct = h.pct;
    const int cf = C.g.cf;
    const int nblocks = C.g.nblocks;
    // the reader continues past the slice into the bytes after it, as the reference's does
    BitReader br(C.buf + job.byte_off, C.buf + job.byte_end, C.buf + C.len);
    if (!out.coefs.reserve(4096)) FAIL(MP2VG_E_NOMEM, "out of host memory");

    // slice header (mp2v_hdr.h:345-363)
    br.skip(24);
    int vpos = (int)br.read(8);
    int mb_row;
    if (C.vertical_size_value > 2800) {
        int ext = (int)br.read(3);
        mb_row = (ext << 7) + vpos - 1;
    } else {
        mb_row = vpos - 1;
    }
    int qcode = (int)br.read(5);
    if (br.peek(1) == 1) {
        br.skip(1 + 1 + 1 + 6);
        while (br.peek(1) == 1) br.skip(9);
    }
    br.skip(1);
    if (mb_row < 0 || mb_row >= C.mbh) FAIL(MP2VG_E_UNSUPPORTED, "slice row outside the picture");
    // slices of one picture run on several workers: the row is claimed atomically
    // (MP2VG_PARSE_SLICES: a row has any number of consecutive slices; parse_session_start marked the
    // rows that have one and the slices that come back to a row left earlier)
    if (C.slices ? job.two : row_done[mb_row].exchange(1, std::memory_order_relaxed))
        FAIL(MP2VG_E_UNSUPPORTED, "two slices in one macroblock row");
    out.mb_row = mb_row;

    // cache setup (decoder.cpp:125-145)
    int16_t PMVs[2][2][2] = {};
    uint16_t dc_pred[3];
    const uint16_t dc_reset = (uint16_t)(1 << (h.intra_dc_precision + 7));
    dc_pred[0] = dc_pred[1] = dc_pred[2] = dc_reset;
    int qscale = qscale_from_code(qcode, h.q_scale_type);
    uint32_t previous_mb_type = 0;
    mp2vg_mb_t* row = row_base_all + (size_t)mb_row * C.mbw;
    int x = 0;
    bool first = C.slices;  // MP2VG_PARSE_SLICES: the start column is still to come
    const int pstruct_frame = 1;  // only frame pictures are accepted
    (void)pstruct_frame;

    auto emit_skipped = [&](int xx) __attribute__((always_inline)) -> bool {
        mp2vg_mb_t& m = row[xx];
        memset(&m, 0, sizeof(m));
        m.x = (uint16_t)xx;
        m.y = (uint16_t)mb_row;
        m.qscale = (uint8_t)qscale;
        m.coef_off = (uint32_t)out.coefs.size();
        // base_motion_compensation<cf, frame, two_vect = (B), skipped=true>(cache, mb, cache.PMVs)
        // (mb_decoder.cpp:546-548, :291-339): direction from previous_mb_type; in B frame
        // pictures vector 1 overwrites vector 0, so the effective vectors are PMVs[1][*].
        uint32_t t = previous_mb_type;
        bool fwd = t & MBT_FWD, bwd = t & MBT_BWD;
        if (!fwd && !bwd) fwd = true;  // 'else' branch: forward
        m.flags = (uint16_t)((fwd ? MP2VG_MB_FWD : 0) | (bwd ? MP2VG_MB_BWD : 0));
        int vsel = (pct == 3) ? 1 : 0;
        for (int s = 0; s < 2; s++)
            for (int c = 0; c < 2; c++) m.mv[0][s][c] = PMVs[vsel][s][c];
        for (int s = 0; s < 2; s++) {
            if (!((s == 0 && fwd) || (s == 1 && bwd))) continue;
            if ((s == 0 ? P.fwd : P.bwd) < 0) return false;
            if (!mc_reads_inside(C.g, xx, mb_row, m.mv[0][s][0], m.mv[0][s][1], false, 0, 0))
                return false;
        }
        return true;
    };

    do {
        if (x >= C.mbw) FAIL(MP2VG_E_BITSTREAM, "macroblock beyond the end of the row");
        // macroblock_address_increment (mb_decoder.cpp:534-539)
        int inc = 0;
        while (br.peek(11) == 0x008) {
            br.skip(11);
            inc += 33;
        }
        int e = T.mba.decode(br);
        if (e < 0 || e >= 33) FAIL(MP2VG_E_BITSTREAM, "bad macroblock_address_increment");
        inc += kMbaCodes[e].a;
        if (first) {  // the slice's first increment is its start column, not a skip run
            if ((uint32_t)(inc - 1) >= (uint32_t)C.mbw) FAIL(MP2VG_E_BITSTREAM, "macroblock beyond the end of the row");
            x = out.x0 = out.x1 = inc - 1;
            inc = 1;
            first = false;
        } else if (x == 0 && inc != 1) {
            FAIL(MP2VG_E_UNSUPPORTED, "slice does not start at column 0");
        }
        // skipped macroblocks (mb_decoder.cpp:541-550)
        if (inc > 1) {
            if (pct == 1) FAIL(MP2VG_E_UNSUPPORTED, "skipped macroblock in an I picture");
            if (pct == 2) memset(PMVs, 0, sizeof(PMVs));
            for (int i = 0; i < inc - 1; i++) {
                if (x >= C.mbw) FAIL(MP2VG_E_BITSTREAM, "skip run beyond the end of the row");
                if (!emit_skipped(x)) FAIL(MP2VG_E_UNSUPPORTED, "skipped MB reads outside the reference");
                x++;
            }
        }
        if (x >= C.mbw) FAIL(MP2VG_E_BITSTREAM, "macroblock beyond the end of the row");

        // macroblock_modes (parse_modes, mb_decoder.cpp:341-419)
        int te = T.mbtype[pct].decode(br);
        if (te < 0) FAIL(MP2VG_E_BITSTREAM, "bad macroblock_type");
        uint32_t mbt = (pct == 1 ? kMbTypeI : pct == 2 ? kMbTypeP : kMbTypeB)[te].a;
        const bool intra = mbt & MBT_INTRA;
        const bool mfwd = mbt & MBT_FWD, mbwd = mbt & MBT_BWD, pattern = mbt & MBT_PATTERN;
        int frame_motion_type = 2;
        if ((mfwd || mbwd) && h.frame_pred_frame_dct == 0) frame_motion_type = (int)br.read(2);
        int dct_type = 0;
        if (h.frame_pred_frame_dct == 0 && (intra || pattern)) dct_type = (int)br.read(1);
        bool field_mv = false;  // mv_format == Field
        int mv_count = 1;
        if (!intra && (mfwd || mbwd)) {
            if (frame_motion_type == 1) {
                field_mv = true;
                mv_count = 2;
            } else if (frame_motion_type == 3) {
                FAIL(MP2VG_E_UNSUPPORTED, "dual-prime prediction");
            } else if (frame_motion_type != 2) {
                FAIL(MP2VG_E_BITSTREAM, "reserved frame_motion_type");
            }
        }
        if (mbt & MBT_QUANT) qscale = qscale_from_code((int)br.read(5), h.q_scale_type);
        if (cf == 3 && dct_type && (intra || pattern))
            FAIL(MP2VG_E_UNSUPPORTED, "4:4:4 field DCT (reference misplaces blocks 10/11)");

        // motion_vectors (mb_decoder.cpp:479-519, 565-574)
        int16_t MVs[2][2][2] = {};
        int fsel[2][2] = {};
        // (always inline: an out-of-line lambda takes br's address and keeps the slice's bit
        // reader in memory, a store-forwarding round trip on every read)
        // one lookup for motion_code and its sign, the residual read with a width of 0 when
        // there is none (f_code 1 or code 0): no branch on the code's value
        auto parse_mv = [&](int r, int s) __attribute__((always_inline)) -> bool {
            for (int t = 0; t < 2; t++) {
                br.refill();  // >= 56 bits: code and sign <= 11, residual <= 8
                const uint32_t e = T.motion_signed[br.peek_nr(11)];
                if (!e) return false;
                br.skip_nr((int)(e >> 16));
                const int mc = (int)(e & 0xffffu) - 32;
                const int fc = h.f_code[s][t];
                const int n = mc != 0 ? fc - 1 : 0;
                const int residual = (int)(((br.cache >> 1) >> (63 - n)) & ((1u << n) - 1u));
                br.skip_nr(n);
                MVs[r][s][t] = mv_reconstruct(fc, mc, residual, PMVs[r][s][t], field_mv && t == 1);
            }
            return true;
        };
        auto parse_mvs = [&](int s) __attribute__((always_inline)) -> bool {
            if (mv_count == 1) {
                if (field_mv) fsel[0][s] = (int)br.read(1);
                return parse_mv(0, s);
            }
            fsel[0][s] = (int)br.read(1);
            if (!parse_mv(0, s)) return false;
            fsel[1][s] = (int)br.read(1);
            return parse_mv(1, s);
        };
        // (no concealment vectors: pictures that carry them are rejected in pass 1)
        if (mfwd)
            if (!parse_mvs(0)) FAIL(MP2VG_E_BITSTREAM, "bad motion_code");
        if (mbwd)
            if (!parse_mvs(1)) FAIL(MP2VG_E_BITSTREAM, "bad motion_code");

        // PMV update + MC selection (mb_decoder.cpp:580-620)
        mp2vg_mb_t& m = row[x];
        memset(&m, 0, sizeof(m));
        m.x = (uint16_t)x;
        m.y = (uint16_t)mb_row;
        if (pct != 1) {
            bool frame_based = intra || !field_mv;  // prediction_type == Frame_based
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
            bool no_mc_p = (pct == 2 && !intra && !mfwd);
            if (intra || no_mc_p) {
                memset(PMVs, 0, sizeof(PMVs));
                memset(MVs, 0, sizeof(MVs));
                field_mv = false;
            }
            if (!intra) {
                bool fwd = mfwd || no_mc_p, bwd = mbwd;
                m.flags = (uint16_t)((fwd ? MP2VG_MB_FWD : 0) | (bwd ? MP2VG_MB_BWD : 0) |
                                     (field_mv ? MP2VG_MB_FIELD_MC : 0));
                int nv = field_mv ? 2 : 1;
                for (int r = 0; r < nv; r++)
                    for (int s = 0; s < 2; s++) {
                        if (!((s == 0 && fwd) || (s == 1 && bwd))) continue;
                        if ((s == 0 ? P.fwd : P.bwd) < 0)
                            FAIL(MP2VG_E_UNSUPPORTED, "prediction from a missing reference");
                        m.mv[r][s][0] = MVs[r][s][0];
                        m.mv[r][s][1] = MVs[r][s][1];
                        if (field_mv && fsel[r][s]) m.flags |= (uint16_t)MP2VG_MB_FS_BIT(r, s);
                        if (!mc_reads_inside(C.g, x, mb_row, MVs[r][s][0], MVs[r][s][1], field_mv,
                                             fsel[r][s], r))
                            FAIL(MP2VG_E_UNSUPPORTED, "motion vector reads outside the reference");
                    }
            }
        }
        if (intra) m.flags |= MP2VG_MB_INTRA;

        // dct_dc_pred reset (mb_decoder.cpp:623-626)
        if (inc > 1 || !intra) dc_pred[0] = dc_pred[1] = dc_pred[2] = dc_reset;

        // coded_block_pattern (mb_decoder.cpp:421-445, 628-631)
        uint32_t cbp = intra ? 0xfffu : 0;
        if (pattern) {
            int ci = T.cbp.decode(br);
            if (ci < 0) FAIL(MP2VG_E_BITSTREAM, "bad coded_block_pattern");
            uint32_t v = (uint32_t)kCbpCodes[ci].a;
            uint32_t c1 = 0, c2 = 0;
            if (cf == 2) c1 = br.read(2);
            if (cf == 3) c2 = br.read(6);
            // block i <- bit (5 - i) of the code (6.3.17.4), a 6-bit reversal (no branch per bit)
            cbp |= kRev6[v & 63];
            if (cf == 2) cbp |= (uint32_t)(((c1 & 1) << 1) | ((c1 >> 1) & 1)) << 6;
            if (cf == 3) cbp |= (uint32_t)kRev6[c2 & 63] << 6;
        }
        cbp &= (1u << nblocks) - 1;
        if (dct_type && (intra || pattern)) m.flags |= MP2VG_MB_DCT_FIELD;
        m.cbp = (uint16_t)cbp;
        m.qscale = (uint8_t)qscale;
        m.coef_off = (uint32_t)out.coefs.size();

        // blocks (decode_transform_template / decode_block_template / parse_block)
        // (MP2VG_PARSE_STANDARD: such a block goes on in B.14 after its DC, in the table's
        // "subsequent coefficient" form, which is what T.coefs[0] holds)
        if (intra && h.intra_vlc_format == 0 && !C.standard)
            FAIL(MP2VG_E_UNSUPPORTED, "intra macroblock with intra_vlc_format=0 (reference mis-parses)");
        const int tab = intra && h.intra_vlc_format ? 1 : 0;
        const CoefLut& cf_lut = T.coefs[tab];
        // room for the MB's worst case (64 words per coded block), written through a raw pointer
        const size_t n0 = out.coefs.size();
        if (!out.coefs.reserve(n0 + 64 * (size_t)__builtin_popcount(cbp))) FAIL(MP2VG_E_NOMEM, "out of host memory");
        uint32_t* w = out.coefs.data() + n0;
        const uint32_t mbx_tag = MP2VG_COEF_MBX(x);
        // the block loop decodes from a local copy of the reader (its address never escapes, so
        // the cache, bit count and pointer stay in registers) and hands it back at the end
        BitReader r = br;
        const uint32_t* const lut1 = cf_lut.l1.data();
        const uint32_t* const lut2 = cf_lut.l2.data();
        // the coded blocks only, lowest first (no data-dependent branch per block position)
        for (uint32_t bits = cbp; bits; bits &= bits - 1) {
            const int b = __builtin_ctz(bits);
            int i = 0;
            const uint32_t btag = ((uint32_t)b << 22) | mbx_tag;  // MP2VG_COEF_PACK's block field
            if (intra) {
                // parse_dct_dc_coeff (mb_decoder.cpp:46-72)
                int pidx = b < 4 ? 0 : ((b & 1) ? 2 : 1);
                int si = (b < 4 ? T.dc_luma : T.dc_chroma).decode(r);  // (refilled: >= 46 bits left)
                if (si < 0) FAIL(MP2VG_E_BITSTREAM, "bad dct_dc_size");
                const int size = (b < 4 ? kDcSizeLuma : kDcSizeChroma)[si].a;  // <= 11
                // dct_dc_differential of `size` bits (none for size 0), without a branch on size
                const int d = (int)(((r.cache >> 1) >> (63 - size)) & ((1u << size) - 1u));
                r.skip_nr(size);
                const int half = (1 << size) >> 1;
                const int diff = d >= half ? d : (d + 1) - 2 * half;
                dc_pred[pidx] = (uint16_t)(dc_pred[pidx] + diff);
                int16_t dcv = (int16_t)(dc_pred[pidx] << (3 - h.intra_dc_precision));
                *w++ = MP2VG_COEF_PACK(dcv, 0, b, MP2VG_COEF_DC | MP2VG_COEF_MBX(x));
                i = 1;
            } else {
                // non-intra first coefficient '1s' (mb_decoder.cpp:79-88), without a branch: the
                // word is stored and kept (w advanced, the two bits consumed) when the bits are '1s'
                const uint32_t c = r.peek(2);
                const uint32_t f = c >> 1;
                *w = MP2VG_COEF_PACK(1 - 2 * (int)(c & 1), 0, b, MP2VG_COEF_FIRST1S | MP2VG_COEF_MBX(x));
                w += f;
                r.skip_nr(2 * (int)f);
                i = (int)f;
            }
            // parse_block's VLC loop (mb_decoder.cpp:89-149): one refill per two codes (a refill
            // leaves >= 56 bits; a code takes at most 24, an escape)
            for (;;) {
                int run, level;
                r.refill();
                int kind = CoefLut::decode_tab(lut1, lut2, r, run, level);
                if (kind != CoefLut::NORMAL) {  // escapes come back as NORMAL (:100-104)
                    if (kind < 0) FAIL(MP2VG_E_BITSTREAM, "bad DCT coefficient code");
                    break;  // EOB
                }
                i += run;
                if (__builtin_expect(i > 63, 0)) FAIL(MP2VG_E_BITSTREAM, "coefficient run past position 63");
                *w++ = ((uint32_t)level & 0xffffu) | ((uint32_t)i << 16) | btag;
                i++;
                kind = CoefLut::decode_tab(lut1, lut2, r, run, level);
                if (kind != CoefLut::NORMAL) {
                    if (kind < 0) FAIL(MP2VG_E_BITSTREAM, "bad DCT coefficient code");
                    break;
                }
                i += run;
                if (__builtin_expect(i > 63, 0)) FAIL(MP2VG_E_BITSTREAM, "coefficient run past position 63");
                *w++ = ((uint32_t)level & 0xffffu) | ((uint32_t)i << 16) | btag;
                i++;
            }
        }
        br = r;
        out.coefs.n = (size_t)(w - out.coefs.data());
        size_t nc = out.coefs.size() - m.coef_off;
        m.ncoef = (uint16_t)nc;
        if (br.overrun()) FAIL(MP2VG_E_BITSTREAM, "slice overruns the buffer");
        previous_mb_type = mbt;
        x++;
        out.x1 = x;
    } while (br.peek(23) != 0);
    if (x != C.mbw && !C.slices) FAIL(MP2VG_E_UNSUPPORTED, "slice does not cover the whole macroblock row");
}

#undef FAIL

}  // namespace

struct ParsedImpl {
    std::vector<mp2vg_picture_t> pics;
    std::vector<mp2vg_mb_t, NoInitAlloc<mp2vg_mb_t>> mbs;  // every record is written by its slice
    std::vector<uint32_t, NoInitAlloc<uint32_t>> coefs;
    std::vector<int32_t> display;
    std::vector<int32_t> gop;
    std::vector<uint32_t> flags;  // MP2VG_PIC_* of each picture (mp2vg_parsed_picture_flags)
    std::vector<int32_t> shard;  // independent decode-order runs (mp2vg_parsed_shards)
    int32_t nshards = 0;
    mp2vg_stream_headers_t hdrs{};
    std::vector<mp2vg_damage_t> damage;  // MP2VG_PARSE_CONCEAL: the replaced rows, stream order
};

}  // namespace mp2vg

struct mp2vg_parsed : mp2vg::ParsedImpl {};

// The macroblock row a slice's start code names: slice_vertical_position, the start code's last
// byte, extended by the 3 bits after it in pictures taller than 2800 lines (bytes past the buffer
// read as 0).  May lie outside the picture.
static int slice_row_of(const uint8_t* buf, uint64_t len, uint64_t off, bool vext) {
    const int vpos = buf[off + 3];
    const int ext = vext && off + 4 < len ? buf[off + 4] >> 5 : 0;
    return (ext << 7) + vpos - 1;
}

using namespace mp2vg;

// ---- parse session: pass 1 on the caller's thread, pass 2 on worker threads ---------------
// Every slice is a task, as in the reference (decoder.cpp:316-318 queues one task per slice):
// workers claim slices in decode order, so the slices of one picture run on several workers and
// a picture is ready as soon as its last slice is; the worker that finishes it checks its row
// coverage and publishes it (status + its MB records).  mp2vg_parse_es waits for all of them;
// the drop-in decoder consumes pictures as they complete (decoder.cpp), overlapping the parse
// with the device work.
struct ParseSession {
    Ctx C;
    mp2vg_parsed* res = nullptr;  // pictures, MB records (coef_off relative to the slice), display
    std::vector<SliceJob> jobs;
    std::vector<SliceOut> outs;
    std::unique_ptr<std::atomic<uint8_t>[]> row_done;  // picture p's rows at [p * mbh, (p + 1) * mbh)
    std::unique_ptr<std::atomic<int>[]> slices_left;   // per picture
    std::vector<size_t> pic_job_begin;
    // MP2VG_PARSE_CONCEAL, per picture, written by the worker that finishes it: the replacement
    // rows of its missing rows (ascending; their words follow the slices'), and its damage entries
    std::vector<std::vector<SliceOut>> extra;
    std::vector<std::vector<mp2vg_damage_t>> damage;
    std::vector<int> status;  // per picture: 1 pending, else an MP2VG_* status
    std::vector<std::string> err;
    std::mutex mu;
    std::condition_variable cv;
    std::atomic<size_t> next_job{0};
    std::vector<std::thread> workers;
    size_t mbs_per_pic = 0;
    // Streaming (window > 0, the drop-in decoder): a worker parses picture p only once
    // p < consumed + window, into a per-picture MB record buffer that parse_session_append
    // recycles, so host memory stays O(window) for any stream length.  window == 0
    // (mp2vg_parse_es): every picture's records go to res->mbs.
    int window = 0;
    int consumed = 0;  // pictures appended (under mu)
    bool stop = false;  // the consumer is gone: waiting workers return
    std::vector<mp2vg_mb_t*> pic_mbs;  // streaming: picture -> its buffer while parsed, not appended
    std::vector<mp2vg_mb_t*> spare;    // streaming: recycled buffers

    ~ParseSession() {
        {
            std::lock_guard<std::mutex> lk(mu);
            stop = true;
        }
        cv.notify_all();
        join();
        for (mp2vg_mb_t* b : pic_mbs) delete[] b;
        for (mp2vg_mb_t* b : spare) delete[] b;
        delete res;
    }
    void join() {
        for (auto& t : workers) t.join();
        workers.clear();
    }
    mp2vg_mb_t* mbs_of(int p) { return window ? pic_mbs[p] : res->mbs.data() + mbs_per_pic * p; }
    void work() {
        for (;;) {
            const size_t j = next_job.fetch_add(1);
            if (j >= jobs.size()) return;
            const int p = jobs[j].pic;
            mp2vg_mb_t* mbs = nullptr;
            if (window) {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return stop || p < consumed + window; });
                if (stop) return;
                if (!pic_mbs[p]) {  // the picture's first slice to get here gives it a buffer
                    if (!spare.empty()) {
                        pic_mbs[p] = spare.back();
                        spare.pop_back();
                    } else {
                        pic_mbs[p] = new mp2vg_mb_t[mbs_per_pic];  // every record is written by its slice
                    }
                }
                mbs = pic_mbs[p];
            } else {
                mbs = mbs_of(p);
            }
            parse_slice(C, C.pics[p], jobs[j], mbs, &row_done[(size_t)p * C.mbh], outs[j]);
            // the last slice of the picture publishes it (acq_rel: every slice's records and
            // outputs are visible to the worker that finishes the picture)
            if (slices_left[p].fetch_sub(1, std::memory_order_acq_rel) == 1) finish_picture(p);
        }
    }
    // MP2VG_PARSE_CONCEAL: row `row` of picture p replaced by sp_conceal_row, its words in o
    bool conceal_row(int p, int row, int status_, int reason, uint64_t byte_off, SliceOut& o) {
        const PicWork& P = C.pics[p];
        SpPicHdr h{};
        h.pct = (uint8_t)P.hdr.pct;
        h.intra_dc_precision = (uint8_t)P.hdr.intra_dc_precision;
        h.has_fwd = P.fwd >= 0;
        h.has_bwd = P.bwd >= 0;
        h.has_conceal_ref = P.conceal_ref >= 0;
        SpGeom g{};
        g.mbw = C.mbw;
        g.nblocks = C.g.nblocks;
        if (!o.coefs.reserve((size_t)C.mbw * C.g.nblocks + 1)) return false;
        struct Out {
            mp2vg_mb_t* row;
            uint32_t* words;
            void record(int x, const mp2vg_mb_t& m) const { row[x] = m; }
            void word(uint32_t i, uint32_t w) const { words[i] = w; }
        };
        uint32_t uses;
        o.coefs.n = sp_conceal_row(g, h, row, Out{mbs_of(p) + (size_t)row * C.mbw, o.coefs.data()}, uses);
        o.mb_row = row;
        o.x0 = 0;
        o.x1 = C.mbw;
        o.concealed = true;
        damage[p].push_back({p, row, status_, reason, byte_off});
        return true;
    }
    static int reason_of(const std::string& text) {
        for (int r = SP_R_MB_BEYOND_ROW; r <= SP_R_ROW_OVERLAP; r++)
            if (text == sp_reason_text(r)) return r;
        return SP_OK;
    }
    // MP2VG_PARSE_SLICES: the cover rule (sp_cover_row, slice_parse.h, restated) on every row of
    // picture p.  A row's slices are consecutive jobs; they must tile [0, mbw).  The row breaks at its
    // first slice that failed, starts past the expected column (gap) or before it (overlap), or, when
    // all fit but end short, at its last slice (gap).  Without concealment the blamed slice carries
    // the failure; with it the row is replaced, its words in the place of its first slice's, the
    // other slices of the row keep none.  false: out of memory.
    bool cover_rows(int p) {
        const size_t jb = pic_job_begin[p], je = pic_job_begin[p + 1];
        for (size_t a = jb, b; a < je; a = b) {
            b = a + 1;
            if (jobs[a].row < 0 || jobs[a].two) continue;  // (names no row of its own: rejected as it is)
            while (b < je && jobs[b].row == jobs[a].row && !jobs[b].two) b++;
            size_t blame = b;
            int st = MP2VG_OK, why = SP_OK, expect = 0;
            for (size_t k = a; k < b; k++) {
                const SliceOut& o = outs[k];
                if (o.status != MP2VG_OK) {
                    blame = k, st = o.status, why = reason_of(o.err);
                    break;
                }
                if (o.x0 != expect) {
                    blame = k, st = MP2VG_E_UNSUPPORTED, why = o.x0 > expect ? SP_R_ROW_GAP : SP_R_ROW_OVERLAP;
                    break;
                }
                expect = o.x1;
            }
            if (blame == b) {
                if (expect == C.mbw) continue;
                blame = b - 1, st = MP2VG_E_UNSUPPORTED, why = SP_R_ROW_GAP;
            }
            if (!(C.conceal && why != SP_OK)) {  // (why == SP_OK: a failure that is no slice-level reason)
                if (outs[blame].status == MP2VG_OK) outs[blame].status = st, outs[blame].err = sp_reason_text(why);
                continue;
            }
            for (size_t k = a + 1; k < b; k++) {
                outs[k].status = MP2VG_OK;
                outs[k].err.clear();
                outs[k].coefs.n = 0;
                outs[k].x0 = outs[k].x1 = 0;
                outs[k].mb_row = jobs[a].row;
            }
            outs[a].status = st;
            outs[a].err = sp_reason_text(why);
            if (!conceal_row(p, jobs[a].row, st, why, jobs[blame].byte_off, outs[a])) return false;
        }
        return true;
    }
    void finish_picture(int p) {
        int st = MP2VG_OK;
        std::string msg;
        bool nomem = C.slices && !cover_rows(p);
        if (C.conceal) {  // every slice-level rejection becomes a replacement row, then the missing rows
            for (size_t j = pic_job_begin[p]; j < pic_job_begin[p + 1] && !nomem && !C.slices; j++) {
                SliceOut& o = outs[j];
                const int why = o.status != MP2VG_OK ? reason_of(o.err) : SP_OK;
                if (why != SP_OK) nomem = !conceal_row(p, o.mb_row, o.status, why, jobs[j].byte_off, o);
            }
            bool other = false;
            for (size_t j = pic_job_begin[p]; j < pic_job_begin[p + 1]; j++)
                other = other || (outs[j].status != MP2VG_OK && !outs[j].concealed);
            if (!other && !nomem) {
                int missing = 0;
                for (int r = 0; r < C.mbh; r++) missing += !row_done[(size_t)p * C.mbh + r].load(std::memory_order_relaxed);
                extra[p].resize(missing);
                for (int r = 0, k = 0; r < C.mbh && !nomem; r++)
                    if (!row_done[(size_t)p * C.mbh + r].exchange(1, std::memory_order_relaxed))
                        nomem = !conceal_row(p, r, MP2VG_E_UNSUPPORTED, SP_R_ROW_UNCOVERED, C.pics[p].byte_off, extra[p][k++]);
            }
            if (nomem) {
                st = MP2VG_E_NOMEM;
                msg = "out of host memory";
            } else if (!damage[p].empty()) {
                res->flags[p] |= MP2VG_PIC_CONCEALED;
                if (C.pics[p].hdr.pct == 1 && C.pics[p].conceal_ref >= 0) {
                    res->pics[p].picture_coding_type = 2;  // (fwd_slot holds the conceal reference already)
                    res->flags[p] |= MP2VG_PIC_RETYPED_I;
                }
            }
        }
        // (MP2VG_PARSE_SLICES: a slice that comes back to a row left earlier goes first, as in the scan,
        // which meets it before any slice is parsed; the run it was cut off from ends short of its row)
        for (int scan_level = C.slices ? 1 : 0; scan_level >= 0 && st == MP2VG_OK; scan_level--)
        for (size_t j = pic_job_begin[p]; j < pic_job_begin[p + 1] && st == MP2VG_OK; j++)  // first failing slice in stream order
            if (outs[j].status != MP2VG_OK && !outs[j].concealed && (!scan_level || jobs[j].two)) {
                char m[256];
                snprintf(m, sizeof m, "picture %d slice @%llu: %s", p, (unsigned long long)jobs[j].byte_off,
                         outs[j].err.c_str());
                st = outs[j].status;
                msg = m;
                break;
            }
        if (st == MP2VG_OK)
            for (int r = 0; r < C.mbh; r++)
                if (!row_done[(size_t)p * C.mbh + r].load(std::memory_order_relaxed)) {
                    st = MP2VG_E_UNSUPPORTED;
                    msg = "picture with a macroblock row not covered by any slice";
                    break;
                }
        {
            std::lock_guard<std::mutex> lk(mu);
            status[p] = st;
            err[p] = msg;
        }
        cv.notify_all();
    }
    int wait(int p) {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return status[p] != 1; });
        if (status[p] != MP2VG_OK) set_error(err[p]);
        return status[p];
    }
};

// sequence_header / sequence_extension / sequence_display_extension bodies (after the start code,
// and after the identifier for the extensions): mp2v_hdr.cpp:4-52
static void read_sequence_header(BitReader& br, mp2vg_sequence_header_t& sh) {
    sh.sequence_header_code = 0x1B3;
    sh.horizontal_size_value = br.read(12);
    sh.vertical_size_value = br.read(12);
    sh.aspect_ratio_information = br.read(4);
    sh.frame_rate_code = br.read(4);
    sh.bit_rate_value = br.read(18);
    br.skip(1);  // marker_bit
    sh.vbv_buffer_size_value = br.read(10);
    sh.constrained_parameters_flag = br.read(1);
    sh.load_intra_quantiser_matrix = br.read(1);
    if (sh.load_intra_quantiser_matrix)
        for (int i = 0; i < 64; i++) sh.intra_quantiser_matrix[i] = (uint8_t)br.read(8);
    sh.load_non_intra_quantiser_matrix = br.read(1);
    if (sh.load_non_intra_quantiser_matrix)
        for (int i = 0; i < 64; i++) sh.non_intra_quantiser_matrix[i] = (uint8_t)br.read(8);
}
static void read_sequence_extension(BitReader& br, mp2vg_sequence_extension_t& se) {
    se.extension_start_code_identifier = 1;
    se.profile_and_level_indication = br.read(8);
    se.progressive_sequence = br.read(1);
    se.chroma_format = br.read(2);
    se.horizontal_size_extension = br.read(2);
    se.vertical_size_extension = br.read(2);
    se.bit_rate_extension = br.read(12);
    br.skip(1);  // marker_bit
    se.vbv_buffer_size_extension = br.read(8);
    se.low_delay = br.read(1);
    se.frame_rate_extension_n = br.read(2);
    se.frame_rate_extension_d = br.read(5);
}
static void read_sequence_display_extension(BitReader& br, mp2vg_sequence_display_extension_t& de) {
    de = mp2vg_sequence_display_extension_t{};
    de.extension_start_code_identifier = 2;
    de.video_format = br.read(3);
    de.colour_description = br.read(1);
    if (de.colour_description) {
        de.colour_primaries = br.read(8);
        de.transfer_characteristics = br.read(8);
        de.matrix_coefficients = br.read(8);
    }
    de.display_horizontal_size = br.read(14);
    br.skip(1);  // marker_bit
    de.display_vertical_size = br.read(14);
}

// Pass 1: start codes and headers -> C (geometry, per-picture headers, W, references, slices) and
// res (picture records, GOP index, stream headers, shards, display order).  Shared by the parse
// session and mp2vg_scan_es.
static int scan_pass1(const uint8_t* buf, uint64_t len, const mp2vg_config_t* cfg, Ctx& C, ParsedImpl* res) {
    C.buf = buf;
    C.len = len;
    C.width = cfg->width;
    C.height = cfg->height;
    C.mbw = cfg->width / 16;
    C.mbh = cfg->height / 16;
    C.g.init(cfg->width, cfg->height, cfg->chroma_format);
    C.conceal = (cfg->reserved & MP2VG_PARSE_CONCEAL) != 0;
    C.standard = (cfg->reserved & MP2VG_PARSE_STANDARD) != 0;
    C.slices = (cfg->reserved & MP2VG_PARSE_SLICES) != 0;

    double tp = now_ms();
    // ---- pass 1: start codes and headers, serially (decoder.cpp:278-329) ----
    // start codes 00 00 01 (their 01 byte at k, 2 <= k <= len - 2), found with memchr on 8
    // segments in parallel; each segment owns the 01 bytes inside it
    std::vector<uint64_t> sc;
    {
        const int nseg = len > (1u << 20) ? 8 : 1;
        std::vector<std::vector<uint64_t>> seg(nseg);
        const uint64_t kend = len >= 2 ? len - 1 : 0;  // exclusive bound on k
        parallel_for(nseg, nseg, [&](int j) {
            uint64_t k = std::max<uint64_t>(2, kend * j / nseg);
            const uint64_t hi = kend * (j + 1) / nseg;
            while (k < hi) {
                const void* hit = memchr(buf + k, 1, hi - k);
                if (!hit) break;
                k = (uint64_t)((const uint8_t*)hit - buf);
                if (buf[k - 1] == 0 && buf[k - 2] == 0) seg[j].push_back(k - 2);
                k++;
            }
        });
        for (auto& v : seg) sc.insert(sc.end(), v.begin(), v.end());
    }
    tp = trace_phase("parse: start codes", tp);
    int seq_chroma = -1;
    int cur = -1;
    int gop = -1;
    int ref_frames[2] = {-1, -1};
    bool seq_end = false;
    bool gop_closed = false;
    int gop_anchors = 0;  // anchors decoded since the last group_of_pictures_header
    // MP2VG_PARSE_STANDARD: the quantiser matrices in force, in coding order (13818-2 6.3.11)
    MatrixState mat;
    mat.reset(nullptr, nullptr);
    for (size_t k = 0; k < sc.size() && !seq_end; k++) {
        uint64_t off = sc[k];
        uint64_t end = (k + 1 < sc.size()) ? sc[k + 1] : len;
        uint8_t code = buf[off + 3];
        BitReader br(buf + off, buf + end);
        br.skip(32);
        if (code == 0xB3) {  // sequence_header (mp2v_hdr.cpp:4-21): a later one overwrites
            mp2vg_sequence_header_t& sh = C.hdrs.sequence_header;
            read_sequence_header(br, sh);
            C.vertical_size_value = (int)sh.vertical_size_value;
            mat.reset(sh.load_intra_quantiser_matrix ? sh.intra_quantiser_matrix : nullptr,
                      sh.load_non_intra_quantiser_matrix ? sh.non_intra_quantiser_matrix : nullptr);
        } else if (code == 0xB5) {  // extension (decoder.cpp:202-242)
            int id = (int)br.read(4);
            if (id == 1) {  // sequence_extension (mp2v_hdr.cpp:23-37)
                mp2vg_sequence_extension_t& se = C.hdrs.sequence_extension;
                read_sequence_extension(br, se);
                seq_chroma = (int)se.chroma_format;
            } else if (id == 2) {  // sequence_display_extension (mp2v_hdr.cpp:39-52)
                mp2vg_sequence_display_extension_t& de = C.hdrs.sequence_display_extension;
                read_sequence_display_extension(br, de);
                C.hdrs.have_sequence_display_extension = 1;
            } else if (id == 5) {
                set_error("scalable extensions are not supported by the reference path");
                return MP2VG_E_UNSUPPORTED;
            } else if (id == 8 && cur >= 0) {  // picture_coding_extension (:105-131)
                PictureHdr& h = C.pics[cur].hdr;
                for (int s = 0; s < 2; s++)
                    for (int t = 0; t < 2; t++) h.f_code[s][t] = (int)br.read(4);
                h.intra_dc_precision = (int)br.read(2);
                h.picture_structure = (int)br.read(2);
                h.top_field_first = (int)br.read(1);
                h.frame_pred_frame_dct = (int)br.read(1);
                h.concealment_motion_vectors = (int)br.read(1);
                h.q_scale_type = (int)br.read(1);
                h.intra_vlc_format = (int)br.read(1);
                h.alternate_scan = (int)br.read(1);
                h.repeat_first_field = (int)br.read(1);
                br.skip(1);  // chroma_420_type
                h.progressive_frame = (int)br.read(1);
                h.have_pcext = true;
            } else if (id == 3 && cur >= 0) {  // quant_matrix_extension (:133-152)
                PictureHdr& h = C.pics[cur].hdr;
                h.have_qme = true;
                for (int m = 0; m < 4; m++) {
                    h.qme_load[m] = (int)br.read(1);
                    if (h.qme_load[m])
                        for (int i = 0; i < 64; i++) h.qme[m][i] = (uint8_t)br.read(8);
                }
                mat.load(h.qme_load, h.qme);
                memcpy(h.state, mat.m, sizeof h.state);
            }
        } else if (code == 0xB8) {  // group_of_pictures_header (mp2v_hdr.cpp:77-83)
            gop++;
            mp2vg_group_of_pictures_header_t& gh = C.hdrs.group_of_pictures_header;
            gh.group_start_code = 0x1B8;
            gh.time_code = br.read(25);
            gh.closed_gop = br.read(1);
            gh.broken_link = br.read(1);
            C.hdrs.have_group_of_pictures_header = 1;
            gop_closed = gh.closed_gop != 0;
            gop_anchors = 0;
        } else if (code == 0x00) {  // picture_start_code (decoder.cpp:294-305)
            PicWork pw;
            pw.byte_off = off;
            pw.hdr.temporal_reference = (int)br.read(10);
            pw.hdr.pct = (int)br.read(3);
            pw.gop = gop < 0 ? 0 : gop;
            memcpy(pw.hdr.state, mat.m, sizeof pw.hdr.state);  // (its own extension, if any, comes next)
            if (pw.hdr.pct < 1 || pw.hdr.pct > 3) {
                set_error("unsupported picture_coding_type");
                return MP2VG_E_UNSUPPORTED;
            }
            int idx = (int)C.pics.size();
            if (pw.hdr.pct == 1) pw.conceal_ref = ref_frames[1];
            if (pw.hdr.pct != 3) {
                pw.fwd = ref_frames[1];  // I/P: dependency on the newest anchor (L0)
                ref_frames[0] = ref_frames[1];
                ref_frames[1] = idx;
                gop_anchors++;
            } else {
                pw.fwd = ref_frames[0];
                pw.bwd = ref_frames[1];
                pw.closed_leading_b = gop_closed && gop_anchors == 1;
            }
            if (pw.hdr.pct == 1) pw.fwd = -1;  // I pictures never predict
            C.pics.push_back(pw);
            cur = idx;
        } else if (code >= 0x01 && code <= 0xAF) {
            if (cur < 0) {
                set_error("slice before the first picture");
                return MP2VG_E_BITSTREAM;
            }
            C.pics[cur].slices.push_back({cur, off, end});
        } else if (code == 0xB7 || code == 0xB4) {
            seq_end = true;
        }
    }
    if (seq_chroma >= 0 && seq_chroma != cfg->chroma_format) {
        set_error("stream chroma_format differs from the decoder configuration");
        return MP2VG_E_UNSUPPORTED;
    }
    // slice_vertical_position_extension is present iff vertical_size (14 bits) is above 2800 (ISO
    // 13818-2 6.2.4); the reference asks the 12-bit vertical_size_value instead (mp2v_hdr.h:347), and
    // so does parse_slice.  Where the two differ (4112 lines: value 16, extension 1) the reference
    // reads a conforming stream's slices one field off, so such a stream is outside its subset.
    {
        const int vsize = C.vertical_size_value | (int)C.hdrs.sequence_extension.vertical_size_extension << 12;
        if ((vsize > 2800) != (C.vertical_size_value > 2800)) {
            set_error("vertical_size " + std::to_string(vsize) + ": slices carry slice_vertical_position_extension, "
                      "which the reference reads only when the 12-bit vertical_size_value (" +
                      std::to_string(C.vertical_size_value) + ") is above 2800");
            return MP2VG_E_UNSUPPORTED;
        }
    }
    // ---- picture-level validation + W (decoder.cpp:154-192) ----
    for (size_t pi = 0; pi < C.pics.size(); pi++) {
        PicWork& P = C.pics[pi];
        PictureHdr& h = P.hdr;
        if (!h.have_pcext) { set_error("MPEG-1 picture (no picture_coding_extension)"); return MP2VG_E_UNSUPPORTED; }
        if (h.picture_structure != 3) { set_error("field pictures"); return MP2VG_E_UNSUPPORTED; }
        if (C.standard) {
            // blocks 4 and 5 of 4:2:2 and 4:4:4 macroblocks are dequantised with W[0] / W[1],
            // which is the standard's result only while the chroma matrices equal the luma ones
            if (C.g.cf != 1 && (memcmp(h.state[2], h.state[0], 64) || memcmp(h.state[3], h.state[1], 64))) {
                set_error("picture " + std::to_string(pi) + ": chroma quantiser matrices differ from the luma ones in " +
                          (C.g.cf == 2 ? "4:2:2" : "4:4:4") + " (blocks 4 and 5 are dequantised with the luma matrices)");
                return MP2VG_E_UNSUPPORTED;
            }
        } else if (!h.have_qme || !(h.qme_load[0] && h.qme_load[1] && h.qme_load[2] && h.qme_load[3])) {
            set_error("picture without a full quant_matrix_extension (reference decoder.cpp:185-191)");
            return MP2VG_E_UNSUPPORTED;
        }
        if (h.concealment_motion_vectors && h.pct != 1) {
            set_error("concealment motion vectors in a P/B picture");
            return MP2VG_E_UNSUPPORTED;
        }
        if (h.concealment_motion_vectors) {
            set_error("concealment motion vectors in an I picture (the reference reads two field vectors)");
            return MP2VG_E_UNSUPPORTED;
        }
        if (h.pct == 2 && P.fwd < 0) { set_error("P picture without a reference"); return MP2VG_E_UNSUPPORTED; }
        // f_code of every direction the picture may code vectors for is 1..9 (0 is forbidden and
        // the reference would read f_code - 1 = -1 residual bits, mb_decoder.cpp:500-505)
        for (int s = 0; s < 2; s++) {
            const bool used = (s == 0 && h.pct != 1) || (s == 1 && h.pct == 3);
            for (int t = 0; t < 2 && used; t++)
                if (h.f_code[s][t] < 1 || h.f_code[s][t] > 9) {
                    set_error("f_code outside 1..9 for a direction the picture codes vectors for");
                    return MP2VG_E_UNSUPPORTED;
                }
        }
        if (P.slices.empty()) { set_error("picture without slices"); return MP2VG_E_BITSTREAM; }
        build_W(C.standard ? h.state : h.qme, h.alternate_scan, P.W);
    }
    tp = trace_phase("parse: headers", tp);
    const int npics = (int)C.pics.size();
    const size_t mbs_per_pic = (size_t)C.mbw * C.mbh;
    // ---- picture records ----
    res->pics.resize(npics);
    for (int p = 0; p < npics; p++) {
        mp2vg_picture_t& d = res->pics[p];
        memset(&d, 0, sizeof d);
        const PicWork& P = C.pics[p];
        d.dst_slot = p;
        // (MP2VG_PARSE_CONCEAL: an I picture's record carries its conceal reference, which only a
        // re-typed, damaged one reads; consumers keep that anchor's slot alive through it)
        d.fwd_slot = C.conceal && P.hdr.pct == 1 ? P.conceal_ref : P.fwd;
        d.bwd_slot = P.hdr.pct == 3 ? P.bwd : -1;
        d.picture_coding_type = P.hdr.pct;
        d.mb_first = (uint32_t)(mbs_per_pic * p);
        d.mb_width = (uint16_t)C.mbw;
        d.mb_height = (uint16_t)C.mbh;
        d.alternate_scan = (uint8_t)P.hdr.alternate_scan;
        d.temporal_reference = P.hdr.temporal_reference;
        memcpy(d.W, P.W, sizeof d.W);
        res->gop.push_back(P.gop);
        res->flags.push_back((P.hdr.progressive_frame ? MP2VG_PIC_PROGRESSIVE_FRAME : 0u) |
                             (P.hdr.top_field_first ? MP2VG_PIC_TOP_FIELD_FIRST : 0u) |
                             (P.hdr.repeat_first_field ? MP2VG_PIC_REPEAT_FIRST_FIELD : 0u));
    }
    res->hdrs = C.hdrs;
    // ---- independent shards: a new one starts at p when no picture from p on predicts from a
    // picture before p (references are the two latest anchors, decoder.cpp:299-304) ----
    {
        res->shard.assign(npics, 0);
        int32_t lo = npics;  // min reference of pictures >= p
        std::vector<uint8_t> starts(npics, 0);
        for (int p = npics - 1; p >= 0; p--) {
            const PicWork& P = C.pics[p];
            if (P.fwd >= 0 && !P.closed_leading_b) lo = std::min(lo, (int32_t)P.fwd);
            if (C.conceal && P.conceal_ref >= 0) lo = std::min(lo, (int32_t)P.conceal_ref);
            if (P.hdr.pct == 3 && P.bwd >= 0) lo = std::min(lo, (int32_t)P.bwd);
            starts[p] = lo >= p;
        }
        int32_t sh = -1;
        for (int p = 0; p < npics; p++) {
            if (starts[p] || sh < 0) sh++;
            res->shard[p] = sh;
        }
        res->nshards = sh + 1;
    }
    // ---- display order: the reference's output scheduler (decoder.cpp:346-369) ----
    {
        int held = -1;
        for (int p = 0; p < npics; p++) {
            if (C.pics[p].hdr.pct == 3 || !cfg->reordering) {
                res->display.push_back(p);
            } else {
                if (held >= 0) res->display.push_back(held);
                held = p;
            }
        }
        if (held >= 0) res->display.push_back(held);
    }
    return MP2VG_OK;
}

extern "C" int mp2vg_probe_es(const uint8_t* buf, uint64_t len, mp2vg_config_t* cfg, mp2vg_stream_headers_t* headers) {
    if (!cfg || (!buf && len)) return MP2VG_E_INVALID;
    // the start code after position `from` (its first 00), or len
    auto next_code = [&](uint64_t from) {
        for (uint64_t k = from; k + 3 < len; k++)
            if (buf[k] == 0 && buf[k + 1] == 0 && buf[k + 2] == 1) return k;
        return len;
    };
    uint64_t off = next_code(0);
    while (off < len && buf[off + 3] != 0xB3) off = next_code(off + 3);
    if (off >= len) {
        set_error("no sequence_header in the stream");
        return MP2VG_E_BITSTREAM;
    }
    mp2vg_stream_headers_t H{};
    uint64_t end = next_code(off + 4);
    {
        BitReader br(buf + off, buf + end);
        br.skip(32);
        read_sequence_header(br, H.sequence_header);
    }
    off = end;
    end = off < len ? next_code(off + 4) : len;
    bool have_ext = false;
    if (off < len && buf[off + 3] == 0xB5) {
        BitReader br(buf + off, buf + end);
        br.skip(32);
        if (br.read(4) == 1) {
            read_sequence_extension(br, H.sequence_extension);
            have_ext = true;
        }
    }
    if (!have_ext) {
        set_error("MPEG-1 stream (no sequence_extension after the sequence_header)");
        return MP2VG_E_UNSUPPORTED;
    }
    // extension_and_user_data(0): a sequence_display_extension may follow, user data between
    for (off = end; off < len && (buf[off + 3] == 0xB5 || buf[off + 3] == 0xB2); off = end) {
        end = next_code(off + 4);
        if (buf[off + 3] != 0xB5) continue;
        BitReader br(buf + off, buf + end);
        br.skip(32);
        if (br.read(4) == 2) {
            read_sequence_display_extension(br, H.sequence_display_extension);
            H.have_sequence_display_extension = 1;
        }
    }
    const int h = (int)(H.sequence_header.horizontal_size_value | H.sequence_extension.horizontal_size_extension << 12);
    const int v = (int)(H.sequence_header.vertical_size_value | H.sequence_extension.vertical_size_extension << 12);
    const int cw = (h + 15) / 16 * 16;
    const int ch = H.sequence_extension.progressive_sequence ? (v + 15) / 16 * 16 : (v + 31) / 32 * 32;
    if (cw > MP2VG_MAX_DIMENSION || ch > MP2VG_MAX_DIMENSION || cw < 16 || ch < 16) {
        set_error("coded size " + std::to_string(cw) + " x " + std::to_string(ch) + " outside 16 .. " +
                  std::to_string(MP2VG_MAX_DIMENSION) + " (MP2VG_MAX_DIMENSION)");
        return MP2VG_E_UNSUPPORTED;
    }
    if (H.sequence_extension.chroma_format < 1) {
        set_error("reserved chroma_format 0");
        return MP2VG_E_UNSUPPORTED;
    }
    cfg->width = cw;
    cfg->height = ch;
    cfg->chroma_format = (int32_t)H.sequence_extension.chroma_format;
    if (headers) *headers = H;
    return MP2VG_OK;
}

int parse_session_start(const uint8_t* buf, uint64_t len, const mp2vg_config_t* cfg, int threads, int window,
                        ParseSession** out) {
    if (!buf || !cfg || !out) return MP2VG_E_INVALID;
    *out = nullptr;
    if (mp2vg_frame_geometry(cfg, nullptr, nullptr, nullptr, nullptr) != MP2VG_OK) return MP2VG_E_INVALID;
    std::unique_ptr<ParseSession> S(new ParseSession());
    Ctx& C = S->C;
    auto* res = new mp2vg_parsed();
    S->res = res;
    if (int rc = scan_pass1(buf, len, cfg, C, res)) return rc;
    const int npics = (int)C.pics.size();
    const size_t mbs_per_pic = (size_t)C.mbw * C.mbh;
    S->mbs_per_pic = mbs_per_pic;
    S->window = std::max(0, window);
    if (S->window)
        S->pic_mbs.assign(npics, nullptr);
    else
        res->mbs.resize(mbs_per_pic * npics);
    for (auto& P : C.pics)
        for (auto& j : P.slices) S->jobs.push_back(j);
    S->outs.resize(S->jobs.size());
    S->row_done.reset(new std::atomic<uint8_t>[(size_t)npics * C.mbh]);
    for (size_t i = 0; i < (size_t)npics * C.mbh; i++) S->row_done[i].store(0, std::memory_order_relaxed);
    S->slices_left.reset(new std::atomic<int>[npics]);
    for (int p = 0; p < npics; p++) S->slices_left[p].store((int)C.pics[p].slices.size(), std::memory_order_relaxed);
    S->pic_job_begin.assign(npics + 1, 0);
    {
        size_t j = 0;
        for (int p = 0; p < npics; p++) {
            S->pic_job_begin[p] = j;
            j += C.pics[p].slices.size();
        }
        S->pic_job_begin[npics] = j;
    }
    if (C.slices) {  // the scan's row rule: a row's slices are consecutive; coming back to a row is refused
        std::vector<uint8_t> seen(C.mbh);
        size_t j = 0;
        for (int p = 0; p < npics; p++) {
            std::fill(seen.begin(), seen.end(), 0);
            for (size_t k = 0; k < C.pics[p].slices.size(); k++, j++) {
                SliceJob& job = S->jobs[j];
                const int row = slice_row_of(buf, len, job.byte_off, C.vertical_size_value > 2800);
                job.row = row < 0 || row >= C.mbh ? -1 : row;
                if (job.row < 0) continue;
                job.two = seen[row] && !(k > 0 && S->jobs[j - 1].row == row && !S->jobs[j - 1].two);
                seen[row] = 1;
                S->row_done[(size_t)p * C.mbh + row].store(1, std::memory_order_relaxed);
            }
        }
    }
    S->extra.resize(npics);
    S->damage.resize(npics);
    S->status.assign(npics, 1);
    S->err.assign(npics, std::string());
    int nthreads = threads > 0 ? threads : cpu_budget();
    nthreads = std::max(1, std::min(nthreads, std::max(1, (int)S->jobs.size())));
    ParseSession* sp = S.get();
    for (int t = 0; t < nthreads; t++) sp->workers.emplace_back([sp]() { sp->work(); });
    *out = S.release();
    return MP2VG_OK;
}

int parse_session_npics(const ParseSession* s) { return (int)s->C.pics.size(); }
const mp2vg_picture_t* parse_session_pictures(const ParseSession* s) { return s->res->pics.data(); }
const int32_t* parse_session_display(const ParseSession* s) { return s->res->display.data(); }
const int32_t* parse_session_shards(const ParseSession* s) { return s->res->shard.data(); }
const mp2vg_stream_headers_t* parse_session_headers(const ParseSession* s) { return &s->res->hdrs; }
int parse_session_wait(ParseSession* s, int p) { return s->wait(p); }
// rows of picture p replaced under MP2VG_PARSE_CONCEAL (after parse_session_wait)
int parse_session_damage(const ParseSession* s, int p) { return (int)s->damage[p].size(); }
void parse_session_free(ParseSession* s) { delete s; }

// Coefficient words of picture p (after parse_session_wait).
size_t parse_session_ncoefs(const ParseSession* s, int p) {
    size_t n = 0;
    for (size_t j = s->pic_job_begin[p]; j < s->pic_job_begin[p + 1]; j++) n += s->outs[j].coefs.size();
    for (const SliceOut& o : s->extra[p]) n += o.coefs.size();
    return n;
}

// Picture p (after parse_session_wait): its MB records into mbs_out and its coefficient words
// into coefs_out, with coef_off relative to coefs_out - base (the picture's words start at word
// `base` of the caller's batch).  The picture's parse buffers are released.
void parse_session_append(ParseSession* s, int p, mp2vg_mb_t* mbs_out, uint32_t* coefs_out, uint32_t base) {
    const size_t n = s->mbs_per_pic;
    memcpy(mbs_out, s->mbs_of(p), n * sizeof(mp2vg_mb_t));
    auto put = [&](SliceOut& o) {
        if (!o.coefs.empty()) memcpy(coefs_out, o.coefs.data(), o.coefs.size() * 4);
        coefs_out += o.coefs.size();
        mp2vg_mb_t* row = mbs_out + (size_t)o.mb_row * s->C.mbw;
        for (int x = o.x0; x < o.x1; x++) row[x].coef_off += base;
        base += (uint32_t)o.coefs.size();
        CoefVec().swap(o.coefs);
    };
    for (size_t j = s->pic_job_begin[p]; j < s->pic_job_begin[p + 1]; j++) put(s->outs[j]);
    for (SliceOut& o : s->extra[p]) put(o);
    if (s->window) {
        {
            std::lock_guard<std::mutex> lk(s->mu);
            s->spare.push_back(s->pic_mbs[p]);
            s->pic_mbs[p] = nullptr;
            s->consumed++;
        }
        s->cv.notify_all();
    }
}

extern "C" int mp2vg_parse_es(const uint8_t* buf, uint64_t len, const mp2vg_config_t* cfg,
                              mp2vg_parsed_t** out) {
    if (!out) return MP2VG_E_INVALID;
    *out = nullptr;
    ParseSession* sp = nullptr;
    int rc = parse_session_start(buf, len, cfg, cfg ? cfg->num_threads : 0, 0, &sp);
    if (rc != MP2VG_OK) return rc;
    std::unique_ptr<ParseSession> S(sp);
    double tp = now_ms();
    S->join();
    const int npics = (int)S->C.pics.size();
    for (int p = 0; p < npics; p++)
        if ((rc = S->wait(p)) != MP2VG_OK) return rc;
    tp = trace_phase("parse: slices", tp);
    // ---- concatenate coefficients, fix offsets: prefix sum, then copies in parallel ----
    std::vector<SliceJob>& jobs = S->jobs;
    std::vector<SliceOut>& outs = S->outs;
    const std::vector<size_t>& pic_job_begin = S->pic_job_begin;
    const size_t mbs_per_pic = S->mbs_per_pic;
    mp2vg_parsed* res = S->res;
    const Ctx& C = S->C;
    // a picture's words: its slices' in stream order, then its concealed missing rows'
    std::vector<size_t> pic_base(npics + 1, 0);
    for (int p = 0; p < npics; p++) pic_base[p + 1] = pic_base[p] + parse_session_ncoefs(S.get(), p);
    const size_t total = pic_base[npics];
    (void)jobs;
    if (total >= (1ull << 32)) {
        set_error("batch too large");
        return MP2VG_E_INVALID;
    }
    res->coefs.resize(total);
    std::atomic<int> next_cp(0);
    auto copier = [&]() {
        for (;;) {
            const int p = next_cp.fetch_add(1);
            if (p >= npics) return;
            size_t base = pic_base[p];
            auto put = [&](SliceOut& o) {
                if (!o.coefs.empty()) memcpy(&res->coefs[base], o.coefs.data(), o.coefs.size() * 4);
                mp2vg_mb_t* row = res->mbs.data() + mbs_per_pic * p + (size_t)o.mb_row * C.mbw;
                for (int x = o.x0; x < o.x1; x++) row[x].coef_off += (uint32_t)base;
                base += o.coefs.size();
                CoefVec().swap(o.coefs);
            };
            for (size_t j = pic_job_begin[p]; j < pic_job_begin[p + 1]; j++) put(outs[j]);
            for (SliceOut& o : S->extra[p]) put(o);
        }
    };
    int nthreads = cfg->num_threads > 0 ? cfg->num_threads : cpu_budget();
    nthreads = std::max(1, std::min(nthreads, std::max(1, npics)));
    if (nthreads == 1) {
        copier();
    } else {
        std::vector<std::thread> th;
        for (int t = 0; t < nthreads; t++) th.emplace_back(copier);
        for (auto& t : th) t.join();
    }
    tp = trace_phase("parse: concatenate", tp);
    for (int p = 0; p < npics; p++) res->damage.insert(res->damage.end(), S->damage[p].begin(), S->damage[p].end());
    S->res = nullptr;
    *out = res;
    return MP2VG_OK;
}

extern "C" int mp2vg_parsed_counts(const mp2vg_parsed_t* p, int32_t* npics, uint64_t* nmbs,
                                   uint64_t* ncoefs) {
    if (!p) return MP2VG_E_INVALID;
    if (npics) *npics = (int32_t)p->pics.size();
    if (nmbs) *nmbs = p->mbs.size();
    if (ncoefs) *ncoefs = p->coefs.size();
    return MP2VG_OK;
}
extern "C" const mp2vg_picture_t* mp2vg_parsed_pictures(const mp2vg_parsed_t* p) { return p ? p->pics.data() : nullptr; }
extern "C" const mp2vg_mb_t* mp2vg_parsed_mbs(const mp2vg_parsed_t* p) { return p ? p->mbs.data() : nullptr; }
extern "C" const uint32_t* mp2vg_parsed_coefs(const mp2vg_parsed_t* p) { return p ? p->coefs.data() : nullptr; }
extern "C" int mp2vg_parsed_display_order(const mp2vg_parsed_t* p, int32_t* order, int32_t n) {
    if (!p || !order || n < (int32_t)p->display.size()) return MP2VG_E_INVALID;
    if (!p->display.empty()) memcpy(order, p->display.data(), p->display.size() * 4);
    return (int)p->display.size();
}
extern "C" int mp2vg_parsed_gop_index(const mp2vg_parsed_t* p, int32_t* gop, int32_t n) {
    if (!p || !gop || n < (int32_t)p->gop.size()) return MP2VG_E_INVALID;
    if (!p->gop.empty()) memcpy(gop, p->gop.data(), p->gop.size() * 4);
    return (int)p->gop.size();
}
extern "C" int mp2vg_parsed_picture_flags(const mp2vg_parsed_t* p, uint32_t* flags, int32_t n) {
    if (!p || !flags || n < (int32_t)p->flags.size()) return MP2VG_E_INVALID;
    if (!p->flags.empty()) memcpy(flags, p->flags.data(), p->flags.size() * 4);
    return (int)p->flags.size();
}
extern "C" int mp2vg_parsed_damage(const mp2vg_parsed_t* p, mp2vg_damage_t* out, int32_t max, int32_t* n) {
    if (!p || !n || max < 0 || (max && !out)) return MP2VG_E_INVALID;
    *n = (int32_t)p->damage.size();
    for (int32_t i = 0; i < *n && i < max; i++) out[i] = p->damage[i];
    return MP2VG_OK;
}
extern "C" const char* mp2vg_damage_reason_string(int32_t reason) { return sp_reason_text(reason); }
extern "C" int mp2vg_parsed_stream_headers(const mp2vg_parsed_t* p, mp2vg_stream_headers_t* out) {
    if (!p || !out) return MP2VG_E_INVALID;
    *out = p->hdrs;
    return MP2VG_OK;
}
extern "C" int mp2vg_parsed_shards(const mp2vg_parsed_t* p, int32_t* shard, int32_t n) {
    if (!p || !shard || n < (int32_t)p->shard.size()) return MP2VG_E_INVALID;
    if (!p->shard.empty()) memcpy(shard, p->shard.data(), p->shard.size() * 4);
    return p->nshards;
}
extern "C" void mp2vg_parsed_free(mp2vg_parsed_t* p) { delete p; }

// ---- host scan (pass 1 on its own) and the CPU twin of the device slice parser ---------------
// mp2vg_scan_es keeps what a slice parser that runs elsewhere (parse.hip, one lane per slice)
// needs: per picture the few header fields the macroblock syntax depends on, per slice its
// picture, macroblock row and byte range.  The scan reads each slice's row itself and makes the
// three row rejections of the host emitter, so every slice of the table owns its row: the
// device needs no atomics.  mp2vg_scan_parse_host runs slice_parse.h, the kernels' source, on
// the host with the kernels' buffer sizes.
namespace mp2vg {

void sp_tables(const uint32_t** words, size_t* nwords, SpTables* out) {
    struct Built {
        std::vector<uint32_t> w;
        SpTables T{};
    };
    static const Built* built = [] {
        Built* b = new Built();
        const Tables& T = Tables::get();
        auto put = [&](const std::vector<uint32_t>& v) {
            const uint32_t at = (uint32_t)b->w.size();
            b->w.insert(b->w.end(), v.begin(), v.end());
            return at;
        };
        auto vals = [&](const vlc_code* c, int n) {
            const uint32_t at = (uint32_t)b->w.size();
            for (int i = 0; i < n; i++) b->w.push_back((uint32_t)c[i].a);
            return at;
        };
        SpTables& S = b->T;
        S.mba = put(T.mba.lut);
        for (int p = 1; p <= 3; p++) S.mbtype[p] = put(T.mbtype[p].lut);
        S.mbtype[0] = S.mbtype[1];
        S.cbp = put(T.cbp.lut);
        S.motion = put(T.motion_signed);
        S.dc_luma = put(T.dc_luma.lut);
        S.dc_chroma = put(T.dc_chroma.lut);
        for (int t = 0; t < 2; t++) {
            S.coef1[t] = put(T.coefs[t].l1);
            S.coef2[t] = put(T.coefs[t].l2);
        }
        S.mba_val = vals(kMbaCodes, countof(kMbaCodes));
        S.mbtype_val[1] = vals(kMbTypeI, countof(kMbTypeI));
        S.mbtype_val[2] = vals(kMbTypeP, countof(kMbTypeP));
        S.mbtype_val[3] = vals(kMbTypeB, countof(kMbTypeB));
        S.mbtype_val[0] = S.mbtype_val[1];
        S.cbp_val = vals(kCbpCodes, countof(kCbpCodes));
        S.dc_luma_val = vals(kDcSizeLuma, countof(kDcSizeLuma));
        S.dc_chroma_val = vals(kDcSizeChroma, countof(kDcSizeChroma));
        S.rev6 = (uint32_t)b->w.size();
        for (int i = 0; i < 64; i++) b->w.push_back(kRev6[i]);
        S.w = b->w.data();
        return b;
    }();
    if (words) *words = built->w.data();
    if (nwords) *nwords = built->w.size();
    if (out) *out = built->T;
}

void scan_span(const mp2vg_scan* s, int32_t first, int32_t npics, uint64_t* lo, uint64_t* hi) {
    const uint32_t j0 = s->pic_slice[first], j1 = s->pic_slice[first + npics];
    *lo = s->slices[j0].byte_off;
    // up to the next picture's first slice (the headers between are what the host emitter's
    // reader sees after the last slice too), or the end of the stream
    *hi = (size_t)(first + npics) < s->pics.size() ? s->slices[j1].byte_off : s->len;
}

void sp_set_slice_error(int pic, uint64_t byte_off, int reason) {
    char m[256];
    snprintf(m, sizeof m, "picture %d slice @%llu: %s", pic, (unsigned long long)byte_off, sp_reason_text(reason));
    set_error(m);
}

}  // namespace mp2vg

extern "C" int mp2vg_scan_es(const uint8_t* buf, uint64_t len, const mp2vg_config_t* cfg, mp2vg_scan_t** out) {
    if (!out) return MP2VG_E_INVALID;
    *out = nullptr;
    if (!buf || !cfg) return MP2VG_E_INVALID;
    if (mp2vg_frame_geometry(cfg, nullptr, nullptr, nullptr, nullptr) != MP2VG_OK) return MP2VG_E_INVALID;
    Ctx C;
    ParsedImpl res;
    if (int rc = scan_pass1(buf, len, cfg, C, &res)) return rc;
    std::unique_ptr<mp2vg_scan> S(new mp2vg_scan());
    S->buf = buf;
    S->len = len;
    S->cfg = *cfg;
    SpGeom& g = S->g;
    g.cf = C.g.cf;
    g.nblocks = C.g.nblocks;
    g.mbw = C.mbw;
    g.mbh = C.mbh;
    g.vext = C.vertical_size_value > 2800;
    for (int i = 0; i < 3; i++) g.pw[i] = C.g.pw[i], g.ph[i] = C.g.ph[i];
    g.mbw_c = C.g.mbw_c;
    g.mbh_c = C.g.mbh_c;
    S->pics = std::move(res.pics);
    S->display = std::move(res.display);
    S->gop = std::move(res.gop);
    S->flags = std::move(res.flags);
    S->shard = std::move(res.shard);
    S->nshards = res.nshards;
    S->hdrs = res.hdrs;
    const int npics = (int)C.pics.size();
    std::vector<uint8_t> seen(C.mbh);
    for (int p = 0; p < npics; p++) {
        const PicWork& P = C.pics[p];
        const PictureHdr& h = P.hdr;
        SpPicHdr d{};
        d.pct = (uint8_t)h.pct;
        for (int s = 0; s < 2; s++)
            for (int t = 0; t < 2; t++) d.f_code[s][t] = (uint8_t)h.f_code[s][t];
        d.intra_dc_precision = (uint8_t)h.intra_dc_precision;
        d.frame_pred_frame_dct = (uint8_t)h.frame_pred_frame_dct;
        d.concealment_motion_vectors = (uint8_t)h.concealment_motion_vectors;
        d.q_scale_type = (uint8_t)h.q_scale_type;
        d.intra_vlc_format = (uint8_t)h.intra_vlc_format;
        d.has_fwd = P.fwd >= 0;
        d.has_bwd = P.bwd >= 0;
        d.has_conceal_ref = C.conceal && P.conceal_ref >= 0;
        d.intra_tab = (uint8_t)(h.intra_vlc_format ? 1 : C.standard ? 0 : SP_INTRA_TAB_REFUSED);
        d.slices = C.slices;
        S->hdr.push_back(d);
        S->pic_slice.push_back((uint32_t)S->slices.size());
        std::fill(seen.begin(), seen.end(), 0);
        for (const SliceJob& j : P.slices) {
            const int row = slice_row_of(buf, len, j.byte_off, g.vext != 0);
            if (row < 0 || row >= C.mbh) {
                sp_set_slice_error(p, j.byte_off, SP_R_ROW_OUTSIDE);
                return MP2VG_E_UNSUPPORTED;
            }
            // (MP2VG_PARSE_SLICES: the slice right after one of its row continues that row, so a row's
            // entries are consecutive in the table; coming back to a row left earlier stays refused)
            if (seen[row] && !(C.slices && S->slices.size() > S->pic_slice.back() && S->slices.back().mb_row == row)) {
                sp_set_slice_error(p, j.byte_off, SP_R_TWO_SLICES);
                return MP2VG_E_UNSUPPORTED;
            }
            seen[row] = 1;
            S->slices.push_back({p, row, j.byte_off, j.byte_end});
        }
        for (int r = 0; r < C.mbh; r++)
            if (!seen[r]) {
                if (C.conceal) {  // an empty entry at the picture's start code, after the picture's slices
                    S->slices.push_back({p, r, P.byte_off, P.byte_off});
                    continue;
                }
                set_error(sp_reason_text(SP_R_ROW_UNCOVERED));
                return MP2VG_E_UNSUPPORTED;
            }
    }
    S->pic_slice.push_back((uint32_t)S->slices.size());
    *out = S.release();
    return MP2VG_OK;
}

extern "C" int mp2vg_scan_counts(const mp2vg_scan_t* s, int32_t* npics, uint64_t* nslices) {
    if (!s) return MP2VG_E_INVALID;
    if (npics) *npics = (int32_t)s->pics.size();
    if (nslices) *nslices = s->slices.size();
    return MP2VG_OK;
}
extern "C" const mp2vg_picture_t* mp2vg_scan_pictures(const mp2vg_scan_t* s) { return s ? s->pics.data() : nullptr; }
extern "C" int mp2vg_scan_display_order(const mp2vg_scan_t* s, int32_t* order, int32_t n) {
    if (!s || !order || n < (int32_t)s->display.size()) return MP2VG_E_INVALID;
    if (!s->display.empty()) memcpy(order, s->display.data(), s->display.size() * 4);
    return (int)s->display.size();
}
extern "C" int mp2vg_scan_gop_index(const mp2vg_scan_t* s, int32_t* gop, int32_t n) {
    if (!s || !gop || n < (int32_t)s->gop.size()) return MP2VG_E_INVALID;
    if (!s->gop.empty()) memcpy(gop, s->gop.data(), s->gop.size() * 4);
    return (int)s->gop.size();
}
extern "C" int mp2vg_scan_picture_flags(const mp2vg_scan_t* s, uint32_t* flags, int32_t n) {
    if (!s || !flags || n < (int32_t)s->flags.size()) return MP2VG_E_INVALID;
    if (!s->flags.empty()) memcpy(flags, s->flags.data(), s->flags.size() * 4);
    return (int)s->flags.size();
}
extern "C" int mp2vg_scan_shards(const mp2vg_scan_t* s, int32_t* shard, int32_t n) {
    if (!s || !shard || n < (int32_t)s->shard.size()) return MP2VG_E_INVALID;
    if (!s->shard.empty()) memcpy(shard, s->shard.data(), s->shard.size() * 4);
    return s->nshards;
}
extern "C" int mp2vg_scan_stream_headers(const mp2vg_scan_t* s, mp2vg_stream_headers_t* out) {
    if (!s || !out) return MP2VG_E_INVALID;
    *out = s->hdrs;
    return MP2VG_OK;
}
extern "C" void mp2vg_scan_free(mp2vg_scan_t* s) { delete s; }

extern "C" int mp2vg_scan_parse_host(const mp2vg_scan_t* s, int32_t first, int32_t npics, mp2vg_mb_t* mbs,
                                     uint64_t nmbs, uint32_t* coefs, uint64_t ncoefs, uint64_t* nmbs_out,
                                     uint64_t* ncoefs_out) {
    if (!s || first < 0 || npics <= 0 || (uint64_t)first + (uint64_t)npics > s->pics.size()) return MP2VG_E_INVALID;
    const SpGeom& g = s->g;
    const uint64_t per_pic = (uint64_t)g.mbw * g.mbh;
    if (mbs && nmbs != per_pic * npics) {
        set_error("mp2vg_scan_parse_host: nmbs is not the range's macroblock count");
        return MP2VG_E_INVALID;
    }
    if (coefs && !mbs) return MP2VG_E_INVALID;
    SpTables T;
    sp_tables(nullptr, nullptr, &T);
    // the span the device gets, in a buffer of the device's size: the bytes, then kSpanPad zeros
    uint64_t lo, hi;
    scan_span(s, first, npics, &lo, &hi);
    const uint64_t span = hi - lo;
    uint8_t* bs = (uint8_t*)malloc(span + kSpanPad);
    if (!bs) return MP2VG_E_NOMEM;
    memcpy(bs, s->buf + lo, span);
    memset(bs + span, 0, kSpanPad);
    struct Free {
        uint8_t* p;
        ~Free() { free(p); }
    } guard{bs};
    const uint32_t j0 = s->pic_slice[first], j1 = s->pic_slice[first + npics];
    const bool conceal = (s->cfg.reserved & MP2VG_PARSE_CONCEAL) != 0;
    const bool slices = (s->cfg.reserved & MP2VG_PARSE_SLICES) != 0;
    std::vector<mp2vg_mb_t> scratch(mbs ? 0 : g.mbw);  // (the counts call conceals into a scratch row)
    std::vector<SpResult> res(j1 - j0);
    auto row_of = [&](const SpSlice& sl) { return mbs + per_pic * (sl.pic - first) + (uint64_t)sl.mb_row * g.mbw; };
    for (uint32_t j = j0; j < j1; j++) {  // count pass
        const SpSlice& sl = s->slices[j];
        const SpPicHdr& h = s->hdr[sl.pic];
        SpResult& r = res[j - j0];
        if (conceal && sl.byte_off == sl.byte_end) {  // a missing row: nothing to parse
            r = SpResult{MP2VG_E_UNSUPPORTED, SP_R_ROW_UNCOVERED, 0, 0, 0, 0};
            r.ncoef = sp_conceal_row(g, h, sl.mb_row, SpCountOut{mbs ? row_of(sl) : scratch.data()}, r.uses);
            continue;
        }
        if (mbs)
            sp_parse_slice(T, g, h, bs, (int64_t)(sl.byte_off - lo), (int64_t)(sl.byte_end - lo), (int64_t)span,
                           sl.mb_row, SpCountOut{row_of(sl)}, res[j - j0]);
        else
            sp_parse_slice(T, g, h, bs, (int64_t)(sl.byte_off - lo), (int64_t)(sl.byte_end - lo), (int64_t)span,
                           sl.mb_row, SpNullOut{}, res[j - j0]);
        if (res[j - j0].iters > sp_iter_bound(sl.byte_end - sl.byte_off, g.mbw)) {
            set_error("mp2vg_scan_parse_host: iteration bound exceeded");
            return MP2VG_E_STATE;
        }
        if (conceal && !slices && r.status != MP2VG_OK && sp_reason_concealed(r.reason))
            r.ncoef = sp_conceal_row(g, h, sl.mb_row, SpCountOut{mbs ? row_of(sl) : scratch.data()}, r.uses);
    }
    if (slices) {  // the row pass: start columns, cover rule on every row's run of entries, replacement rows
        for (uint32_t j = j0; j < j1; j++) {
            const SpSlice& sl = s->slices[j];
            if (sl.byte_off != sl.byte_end)
                res[j - j0].x0 = (uint16_t)sp_slice_x0(T, g, bs, (int64_t)(sl.byte_off - lo), (int64_t)(sl.byte_end - lo), (int64_t)span);
        }
        for (uint32_t a = j0, b; a < j1; a = b) {
            const SpSlice& sl = s->slices[a];
            for (b = a + 1; b < j1 && s->slices[b].pic == sl.pic && s->slices[b].mb_row == sl.mb_row;) b++;
            if (sl.byte_off == sl.byte_end) continue;  // a missing row, concealed above
            SpResult& r = res[a - j0];
            sp_cover_row(&r, b - a, g.mbw, conceal);
            if (conceal && r.status != MP2VG_OK && sp_reason_concealed(r.reason))
                r.ncoef = sp_conceal_row(g, s->hdr[sl.pic], sl.mb_row, SpCountOut{mbs ? row_of(sl) : scratch.data()}, r.uses);
        }
    }
    for (uint32_t j = j0; j < j1; j++)  // the first failing slice in stream order
        if (res[j - j0].status != MP2VG_OK && !(conceal && sp_reason_concealed(res[j - j0].reason))) {
            sp_set_slice_error(s->slices[j].pic, s->slices[j].byte_off, res[j - j0].reason);
            return res[j - j0].status;
        }
    std::vector<uint64_t> base(j1 - j0 + 1, 0);  // scan: exclusive prefix sum in table order
    for (uint32_t j = j0; j < j1; j++) base[j - j0 + 1] = base[j - j0] + res[j - j0].ncoef;
    const uint64_t total = base[j1 - j0];
    if (nmbs_out) *nmbs_out = per_pic * npics;
    if (ncoefs_out) *ncoefs_out = total;
    if (total >= (1ull << 32)) {
        set_error("batch too large");
        return MP2VG_E_INVALID;
    }
    if (!mbs) return MP2VG_OK;  // the counts call
    if (ncoefs != total || (total && !coefs)) {
        set_error("mp2vg_scan_parse_host: ncoefs is not the counted number of words");
        return MP2VG_E_INVALID;
    }
    for (uint32_t j = j0; j < j1; j++) {  // emit pass
        const SpSlice& sl = s->slices[j];
        SpResult r2;
        const SpEmitOut eo{row_of(sl), coefs + base[j - j0], res[j - j0].ncoef, (uint32_t)base[j - j0]};
        if (res[j - j0].fate == SP_FATE_DROPPED) continue;  // its row was replaced: the carrier emits it
        if (res[j - j0].reason != SP_OK) {  // a concealed row: its rebased coef_off and its DC words
            uint32_t uses;
            if (sp_conceal_row(g, s->hdr[sl.pic], sl.mb_row, eo, uses) != res[j - j0].ncoef) return MP2VG_E_STATE;
            continue;
        }
        sp_parse_slice(T, g, s->hdr[sl.pic], bs, (int64_t)(sl.byte_off - lo), (int64_t)(sl.byte_end - lo), (int64_t)span,
                       sl.mb_row, eo, r2);
        if (r2.status != MP2VG_OK || r2.ncoef != res[j - j0].ncoef) {
            set_error("mp2vg_scan_parse_host: the emit pass differs from the count pass");
            return MP2VG_E_STATE;
        }
    }
    return MP2VG_OK;
}
