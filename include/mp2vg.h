/*
 * mp2vg.h — C ABI of the MI355X-native MPEG-2 macroblock reconstruct path.
 *
 * Plain C, plain pointers and sizes, int status codes; no torch / HIP types in any signature.
 * The shared library is tiny_mp2v_dec_amd/_build/libmp2vg.so (hipcc, gfx950).
 *
 * What each group of entry points replaces in the reference (fxslava/tiny_mp2v_dec):
 *
 *   mp2vg_create / mp2vg_destroy / mp2vg_frame_geometry
 *       replace decoder_init's frame pool (reference src/core/decoder.cpp:381-406) and the
 *       frame_c plane layout (decoder.h:34-49, decoder.cpp:44-77): 3 planes per picture,
 *       stride = round_up(width, 64), chroma stride = round_up(stride/2, 64) (4:4:4: = stride).
 *   mp2vg_batch_upload / mp2vg_batch_decode
 *       replace the per-slice hot loop `do { m_parse_macroblock_func(&bs, cache); } while(...)`
 *       (decoder.cpp:148-150) — i.e. everything parse_macroblock_template does AFTER parsing:
 *       MC (mb_decoder.cpp:291-339 -> mc.cpp tables -> mc_sse2.hpp), dequant + mismatch control
 *       (parse_block, mb_decoder.cpp:74-155), SSE2 IDCT put/add (idct_sse2.hpp:96-120) and
 *       block placement (mb_decoder.cpp:166-196) — for a whole batch of pictures per call.
 *       The seam is the packed record stream defined below (SURVEY.md §8b "Record stream").
 *   mp2vg_parse_es
 *       the host record emitter: start-code scan + header parse + VLC/MV/DC parse
 *       (decoder.cpp:278-329, mp2v_hdr.cpp, mp2v_vlc_dec.hpp, mb_decoder.cpp:341-641) producing
 *       records instead of pixels.
 *   mp2vg_decoder_*
 *       the drop-in decoder: mp2v_decoder_c(config, renderer) + decode(buf, len) with frames
 *       delivered in display order on a render thread (decoder.h:82-131, decoder.cpp:346-379).
 *       include/mp2v_decoder.h wraps these in the reference's own C++ class names.
 */
#ifndef MP2VG_H
#define MP2VG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: coefficient words carry the MB column mod 8 in bits 26-28 and the FIRST1S / DC flags in
 *    bits 29 / 30 (1: FIRST1S bit 26, DC bit 27, MB column bits 28-30); mp2vg_frame_t.device */
#define MP2VG_ABI_VERSION 2

/* ---- status codes --------------------------------------------------------------------- */
enum {
    MP2VG_OK = 0,
    MP2VG_E_INVALID = -1,     /* bad argument / malformed record batch                    */
    MP2VG_E_UNSUPPORTED = -2, /* stream outside the reference's decodable subset */
    MP2VG_E_HIP = -3,         /* HIP runtime error (no device, launch failure, ...)        */
    MP2VG_E_NOMEM = -4,
    MP2VG_E_STATE = -5,       /* call out of order                                           */
    MP2VG_E_BITSTREAM = -6    /* bitstream syntax error                                      */
};

/* ---- record stream (the seam; 32-byte MB records + 4-byte coefficient words) -------------
 *
 * One record per macroblock of every picture, skipped MBs included (as MC-only records), in
 * raster order: picture p owns records [mb_first, mb_first + mb_width*mb_height).
 * Motion vectors are FINAL luma vectors after all PMV rules and skipped-MB quirks
 * (reference mb_decoder.cpp:447-519, 541-550, 580-604); chroma scaling stays on the device
 * (mb_decoder.cpp:198-206).
 */
enum {
    MP2VG_MB_INTRA = 1u << 0,     /* IDCT put, no MC; cbp codes every block, and every MB of an
                                     I picture is intra (both checked on upload)               */
    MP2VG_MB_FWD = 1u << 1,       /* forward prediction from fwd_slot                        */
    MP2VG_MB_BWD = 1u << 2,       /* backward prediction from bwd_slot (both bits: bidir avg) */
    MP2VG_MB_FIELD_MC = 1u << 3,  /* frame picture, field prediction: 2 vectors, 16x8 each  */
    MP2VG_MB_DCT_FIELD = 1u << 4  /* dct_type = 1 (field DCT block placement)               */
};
/* motion_vertical_field_select[r][s] lives in flags bit (8 + 2*r + s) */
#define MP2VG_MB_FS_BIT(r, s) (1u << (8 + 2 * (r) + (s)))

typedef struct mp2vg_mb {
    uint16_t x, y;        /* macroblock column / row                                          */
    uint16_t flags;       /* MP2VG_MB_* | field selects                                        */
    uint16_t cbp;         /* coded block pattern, bit b <-> block b (mb_decoder.cpp:421-445)   */
    uint8_t  qscale;      /* quantiser_scale after q_scale_type mapping (decoder.cpp:140-145)  */
    uint8_t  reserved;
    uint16_t ncoef;       /* number of coefficient words                                        */
    uint32_t coef_off;    /* index of the first coefficient word in the batch's coef array     */
    int16_t  mv[2][2][2]; /* [vector r][direction s: 0 fwd, 1 bwd][x, y], half-pel luma units;
                             field-MC vertical components in field units                       */
} mp2vg_mb_t;             /* 32 bytes */

/* Coefficient word: bits 0-15 int16 level (signed run-level level, or the final QFS[0] value
 * when MP2VG_COEF_DC), bits 16-21 scan position i (0..63), bits 22-25 block index (0..11),
 * bits 26-28: the MB's column x mod 8 (bits 22-27 are the word's (MB in its 4-MB group, block)
 * index for the kernel; mp2vg_batch_upload validates them), bit 29 FIRST1S: non-intra first
 * coefficient coded with the B.14 '1s' code — dequantised as (3*W[0]*qs)>>5 without the
 * +-2047 clamp (mb_decoder.cpp:79-88), bit 30 DC: intra DC value, excluded from the mismatch
 * parity (mb_decoder.cpp:76,160), bit 31: 0.  FIRST1S and DC words carry i = 0.
 * Words of one MB are grouped by block, blocks in bitstream order.                           */
#define MP2VG_COEF_LEVEL(w) ((int16_t)((w) & 0xffffu))
#define MP2VG_COEF_POS(w) (((w) >> 16) & 63u)
#define MP2VG_COEF_BLOCK(w) (((w) >> 22) & 15u)
#define MP2VG_COEF_FIRST1S (1u << 29)
#define MP2VG_COEF_DC (1u << 30)
#define MP2VG_COEF_MBX(x) (((uint32_t)(x) & 7u) << 26)
#define MP2VG_COEF_PACK(level, pos, block, fl) \
    ((uint32_t)(uint16_t)(int16_t)(level) | ((uint32_t)(pos) << 16) | ((uint32_t)(block) << 22) | (uint32_t)(fl))

typedef struct mp2vg_picture {
    int32_t  dst_slot;            /* frame-pool slot written                                   */
    int32_t  fwd_slot;            /* forward reference slot (L0), -1 = none                    */
    int32_t  bwd_slot;            /* backward reference slot (L1), -1 = none                   */
    int32_t  picture_coding_type; /* 1 I, 2 P, 3 B                                              */
    uint32_t mb_first;            /* first MB record of this picture                            */
    uint16_t mb_width, mb_height;
    uint8_t  alternate_scan;
    uint8_t  reserved0[3];
    int32_t  temporal_reference;
    uint8_t  W[4][64];            /* quantiser matrices in scan order: [0] intra, [1] non-intra,
                                     [2] chroma intra, [3] chroma non-intra (decoder.cpp:154-192) */
} mp2vg_picture_t;                /* 288 bytes */

/* ---- device context ------------------------------------------------------------------- */
/* The largest width and height a config may hold.  Every entry point that takes a config refuses
 * a larger one with MP2VG_E_INVALID (mp2vg_frame_geometry is the gate).  Three things meet at this
 * size: MPEG-2 codes horizontal_size and vertical_size in 12 + 2 bits, so 16383, coded as 16384,
 * is the largest picture a stream can describe; the records' int16 half-pel vectors can just span
 * it (2 * (16384 - 16) = 32736); and the kernels address a slot and its anchor tiles with 32-bit
 * offsets, the largest of which (a 4:4:4 slot's Cr tile plane, 2^30 + 2^29) stays below 2^31. */
#define MP2VG_MAX_DIMENSION 16384

typedef struct mp2vg_config {
    int32_t width, height;       /* CODED size: multiples of 16, 16 .. MP2VG_MAX_DIMENSION, as
                                    the reference's config                                    */
    int32_t chroma_format;       /* 1 = 4:2:0, 2 = 4:2:2, 3 = 4:4:4                          */
    int32_t pictures_pool_size;  /* number of device frame slots                             */
    int32_t num_threads;         /* host parse threads (0 = auto)                            */
    int32_t reordering;          /* display reorder in the drop-in decoder                   */
    int32_t device;              /* HIP device ordinal                                       */
    int32_t reserved;            /* flags: MP2VG_DECODER_* (drop-in decoder), MP2VG_CTX_*     */
} mp2vg_config_t;

/* mp2vg_config_t.reserved flag for mp2vg_decoder_create: frames are handed to the renderer in
 * HBM (mp2vg_frame_t.planes are device pointers on cfg->device, valid during the callback), with
 * no PCIe download: the opt-in device-pointer output path for callers that consume frames on the
 * GPU.  Without it, planes are host memory (the reference's frame_c contract). */
#define MP2VG_DECODER_DEVICE_FRAMES 1
/* mp2vg_config_t.reserved flag for mp2vg_create: run every picture set of a batch on one stream
 * (default: closed groups of pictures dealt to 2 streams, or MP2VG_STREAMS), so per-launch
 * device times never overlap -- per-kernel roofline measurements and their rocprof traces */
#define MP2VG_CTX_ONE_STREAM 2
/* mp2vg_config_t.reserved flag for mp2vg_decoder_create (opt-in): decode() only scans the stream
 * on the host (mp2vg_scan_es) and feeds its 16-picture chunks through mp2vg_batch_upload_es, so the
 * slices are parsed on the device and no parse workers start.  Display order, the frame pool,
 * host or device frames and the lanes of mp2vg_decoder_create_multi are unchanged. */
#define MP2VG_DECODER_DEVICE_PARSE 4
/* mp2vg_config_t.reserved flag (opt-in) for mp2vg_parse_es, mp2vg_scan_es (whose scan carries it to
 * mp2vg_scan_parse_host and mp2vg_batch_upload_es) and mp2vg_decoder_create / _create_multi: a
 * damaged slice no longer fails the call.  One definition (sp_conceal_row, csrc/slice_parse.h),
 * whole rows: a slice rejected for any slice-level reason ("macroblock beyond the end of the row"
 * .. "slice does not cover the whole macroblock row", whatever its status), or a macroblock row
 * of a picture that no slice covers, is replaced by a row of mb_width records, and the records the
 * slice wrote before its fault are discarded:
 *   P picture   flags = MP2VG_MB_FWD, vectors 0, cbp 0, ncoef 0 (a copy of the reference's row);
 *   B picture   the same from the forward reference when the picture has one, else MP2VG_MB_BWD
 *               from the backward reference;
 *   I picture   with an earlier anchor in decode order (its conceal reference): as a P picture from
 *               that anchor, and the picture record is re-typed to picture_coding_type 2 with
 *               fwd_slot = that anchor.  Under the flag every I picture's record carries its conceal
 *               reference in fwd_slot (-1: none), damaged or not, so that slot lifetimes keep the
 *               anchor alive; an undamaged I picture keeps type 1 and never reads it;
 *   no reference at all (the stream's first anchor; a B picture in front of it): intra records
 *               with every block coded by one DC word of level 1 << (intra_dc_precision + 7), the
 *               predictor's reset value (mid-grey).
 * Always qscale 1, reserved 0, coef_off the running word offset.  A concealed missing row's words
 * follow those of the picture's slices (rows ascending).  Still rejected under the flag: every
 * picture-level and stream-level fault of pass 1 (a picture without any slice among them), "slice
 * row outside the picture", "two slices in one macroblock row" (without MP2VG_PARSE_SLICES: any
 * second slice of a row; with it: a slice whose row was seen earlier in the picture but not
 * immediately before it), and MP2VG_E_INVALID slice-table entries.  With the flag every anchor but the first depends on the one before it, so the stream
 * is one shard (mp2vg_parsed_shards returns 1 whenever an I picture has a conceal reference) and a
 * multi-device decoder runs it on one lane: output never depends on the lane count.  The damage
 * is reported by mp2vg_parsed_damage / mp2vg_last_upload_damage / mp2vg_decoder_damage_count. */
#define MP2VG_PARSE_CONCEAL 8
/* mp2vg_config_t.reserved flag (opt-in), honoured exactly where MP2VG_PARSE_CONCEAL is and free to
 * combine with it and with MP2VG_DECODER_DEVICE_PARSE: streams as ordinary encoders write them.
 * Two of the reference's limits go; with the flag clear nothing changes.
 *   Quantiser matrices as 13818-2 6.3.3 and 6.3.11 define them, in place of "a full
 *   quant_matrix_extension on every picture".  The parse keeps four matrices in coding order.  At
 *   the start of a call and at every sequence_header: intra = the header's matrix when it loads
 *   one, else the default intra matrix of 6.3.11; non_intra = the header's, else 16 everywhere;
 *   chroma_intra = intra; chroma_non_intra = non_intra.  At every quant_matrix_extension, in its
 *   field order: a loaded intra also replaces chroma_intra, a loaded non_intra also replaces
 *   chroma_non_intra, then a loaded chroma matrix replaces just itself.  The state holds for the
 *   picture the extension belongs to and every later one until the next load or sequence_header;
 *   a picture's W is that state in the picture's scan order, for all three chroma formats.
 *   intra_vlc_format = 0, per picture: an intra block reads dct_dc_size and the differential as
 *   ever and then goes on in table B.14 in its "subsequent coefficient" form ('10' is end of block
 *   and may follow the DC at once, '11s' is run 0 level +-1; the '1s' code belongs to the first
 *   coefficient of non-intra blocks only).  Pictures with intra_vlc_format = 1 are untouched.
 * One limit stays: the kernels dequantise blocks 4 and 5 of 4:2:2 and 4:4:4 macroblocks with the luma
 * matrices where the standard takes the chroma ones, so a 4:2:2 or 4:4:4 picture
 * whose state has chroma_intra != intra or chroma_non_intra != non_intra is refused
 * (MP2VG_E_UNSUPPORTED, "picture N: chroma quantiser matrices differ from the luma ones ...");
 * every stream that never loads a chroma matrix of its own decodes.
 * Still refused under the flag: field pictures, dual-prime, concealment motion vectors, MPEG-1,
 * scalable extensions, and (unless MP2VG_PARSE_SLICES is set too) more than one slice per macroblock
 * row and slices that start after column 0.
 * And two pieces of arithmetic stay the reference's, not the standard's: half-pel
 * prediction in both directions is the cascaded average avg(avg, avg), and the IDCT
 * is the reference's SSE2 one. */
#define MP2VG_PARSE_STANDARD 16
/* mp2vg_config_t.reserved flag (opt-in), honoured exactly where MP2VG_PARSE_CONCEAL and
 * MP2VG_PARSE_STANDARD are and free to combine with both and with MP2VG_DECODER_DEVICE_PARSE: any
 * number of slices per macroblock row, as 13818-2 allows.  With the flag clear nothing changes.
 * One statement of the rule (csrc/slice_parse.h):
 *   start   a slice's first macroblock_address_increment (escapes included) names its start column
 *           x0 = increment - 1.  It is no skip run: no records are written for it, it is legal in
 *           an I picture, and predictors and quantiser scale start from the slice header as ever.
 *           x0 >= mb_width is "macroblock beyond the end of the row".
 *   end     the slice ends at the column x1 where its macroblock loop ends; "slice does not start at
 *           column 0" and "slice does not cover the whole macroblock row" are not produced.
 *   scan    a slice whose row is the row of the slice immediately before it in the picture continues
 *           that row; a slice whose row was seen earlier but not immediately before is still "two
 *           slices in one macroblock row" (also under MP2VG_PARSE_CONCEAL: it names no row of its own),
 *           and is reported before any other fault of its picture's slices.
 *   cover   a row's slices, in stream order, must tile [0, mb_width): the first x0 = 0, each next
 *           x0 = the previous x1, the last x1 = mb_width.  The row breaks at its first slice that
 *           failed its parse, that starts past the expected column ("slices of a macroblock row
 *           leave a gap") or before it ("slices of a macroblock row overlap or are out of order"); a
 *           row that ends short breaks at its last slice (gap).  Both are MP2VG_E_UNSUPPORTED, and
 *           the call reports the failing slice that comes first in the stream, whatever its fault:
 *           "picture N slice @offset: text".
 * Records stay one per macroblock in raster order and the coefficient words stay the slices' words
 * in stream order, which on a valid row is raster order: nothing below the parse sees the flag.
 * With MP2VG_PARSE_CONCEAL concealment stays row-granular: a row that breaks for a concealable reason
 * (the two above included) is replaced as a whole, its words in the place of its first slice's; the
 * damage is reported once per row with the blamed slice's status, reason and offset.
 * Still refused: field pictures, dual-prime, concealment motion vectors, MPEG-1, scalable
 * extensions, and what MP2VG_PARSE_STANDARD lifts unless that flag is set too. */
#define MP2VG_PARSE_SLICES 32

typedef struct mp2vg_ctx mp2vg_ctx_t;

int  mp2vg_abi_version(void);
const char* mp2vg_status_string(int status);
const char* mp2vg_last_error(void); /* thread-local detail of the last failure */

int  mp2vg_create(const mp2vg_config_t* cfg, mp2vg_ctx_t** out);
int  mp2vg_destroy(mp2vg_ctx_t* ctx);
/* plane geometry of every frame slot: width/height/stride of plane 0..2, bytes per slot */
int  mp2vg_frame_geometry(const mp2vg_config_t* cfg, int32_t width[3], int32_t height[3],
                          int32_t stride[3], uint64_t* slot_bytes);
/* grow the frame pool to nslots slots (new slots read as zero).  Slots live in blocks of 16, each
 * its own allocation, with each slot's anchor tiles (the motion-compensation taps' copy of I and
 * P pictures, 2 x slot bytes); slot addresses are not contiguous: mp2vg_slot_device_ptr */
int  mp2vg_reserve_slots(mp2vg_ctx_t* ctx, int32_t nslots);

/* Upload a record batch from host memory (staged through pinned buffers, hipMemcpyAsync on the
 * context stream).  The batch stays resident in HBM until the next upload. */
int  mp2vg_batch_upload(mp2vg_ctx_t* ctx, const mp2vg_picture_t* pics, int32_t npics,
                        const mp2vg_mb_t* mbs, uint64_t nmbs, const uint32_t* coefs,
                        uint64_t ncoefs);
/* Host-only check of a record batch against a geometry and a pool of nslots slots: exactly the
 * validation and planning mp2vg_batch_upload runs before any copy (no device needed).  Returns
 * MP2VG_OK, or MP2VG_E_INVALID with the reason in mp2vg_last_error().  Optional outputs (NULL to
 * skip): *nlaunches = kernel launches per mp2vg_batch_decode; launch_of_pic[npics] = the launch
 * (index into mp2vg_batch_times' launch list) that reconstructs each picture; launch_mode[i <
 * max_launches] = that launch's kernel (0 I, 1 P, 2 B, 3 mixed P/B picture types, 4 I without tile stores). */
int  mp2vg_batch_validate(const mp2vg_config_t* cfg, int32_t nslots, const mp2vg_picture_t* pics,
                          int32_t npics, const mp2vg_mb_t* mbs, uint64_t nmbs,
                          const uint32_t* coefs, uint64_t ncoefs, int32_t* nlaunches,
                          int32_t* launch_of_pic, int32_t* launch_mode, int32_t max_launches);
/* The whole plan of a batch, host only: what mp2vg_batch_upload would make resident for
 * mp2vg_batch_decode (the same validation and planning as mp2vg_batch_validate, on the same
 * device-less context).  Every array is the caller's, sized by its max_* field (NULL or 0: counts
 * only); every n* field returns the plan's true count, and entries past max_* are not written.
 *   slices    4 words per slice, in launch order: index of its picture in the batch, first MB
 *             record, MB records, flag bits (bit 0: stores its anchor tiles in the loop, bit 1:
 *             one-direction B picture, bit 2: that direction is backward)
 *   launches  6 words per launch, in enqueue order per set: first slice, end slice, kernel mode
 *             (mp2vg_batch_validate), dependency level, picture set (= stream), slices per
 *             workgroup (0: one)
 *   writes    2 words per picture in decode order: destination slot, 1 when the batch leaves its
 *             anchor tiles current
 *   ext_reads 2 words per slot read before the batch writes it: slot, reading set
 *   post      2 words per tile conversion that follows a launch: launch, slot
 *   foot      2 words per slot of each set's footprint: set, slot (what the next batch's sets
 *             wait for)
 * Returns MP2VG_OK, or MP2VG_E_INVALID with the reason in mp2vg_last_error(). */
typedef struct mp2vg_plan {
    uint32_t* slices;
    int32_t*  launches;
    int32_t*  writes;
    int32_t*  ext_reads;
    int32_t*  post;
    int32_t*  foot;
    int32_t   max_slices, max_launches, max_writes, max_ext_reads, max_post, max_foot;
    int32_t   nslices, nlaunches, nwrites, next_reads, npost, nfoot;
    int32_t   nsets;      /* picture sets of the batch */
    int32_t   reserved;
} mp2vg_plan_t;
int  mp2vg_batch_plan(const mp2vg_config_t* cfg, int32_t nslots, const mp2vg_picture_t* pics,
                      int32_t npics, const mp2vg_mb_t* mbs, uint64_t nmbs,
                      const uint32_t* coefs, uint64_t ncoefs, mp2vg_plan_t* plan);
/* Enqueue the reconstruct of every picture of the resident batch: pictures are grouped by
 * reference-dependency depth and each depth level is one kernel launch (one workgroup per
 * slice = MB row).  Asynchronous; per-launch device times are recorded with HIP events. */
int  mp2vg_batch_decode(mp2vg_ctx_t* ctx);
int  mp2vg_synchronize(mp2vg_ctx_t* ctx);
/* number of kernel launches of the last mp2vg_batch_decode and their device times (ms) */
int  mp2vg_last_launch_times(mp2vg_ctx_t* ctx, float* ms, int32_t max, int32_t* count);
/* device time (ms) of the whole last mp2vg_batch_decode: first launch start to last launch end */
int  mp2vg_last_batch_time(mp2vg_ctx_t* ctx, float* ms);
/* times of the batch decoded `back` decodes ago (0 = the last; the last 64 are kept), so batches
 * can be decoded back to back and timed afterwards: whole-batch span (batch_ms, may be NULL) and
 * per-launch device times (launch_ms[0..min(count, max)), may be NULL); synchronises.  A decode
 * that ran the placement calibration (below) counts as one batch: its times are those of one
 * run on the pool that was kept. */
int  mp2vg_batch_times(mp2vg_ctx_t* ctx, int32_t back, float* batch_ms, float* launch_ms, int32_t max,
                       int32_t* count);
/* device time (ms) from the start of the batch decoded `back_first` decodes ago to the end of the
 * one `back_last` decodes ago (back_first >= back_last; the last 64 are kept): the device span of
 * back-to-back batches, whose picture sets overlap across batch boundaries; synchronises */
int  mp2vg_batches_span(mp2vg_ctx_t* ctx, int32_t back_first, int32_t back_last, float* ms);
/* copy one frame slot to host planes (each plane written width x height, tightly packed if
 * dst_stride is 0); synchronous */
int  mp2vg_download_slot(mp2vg_ctx_t* ctx, int32_t slot, uint8_t* dst_planes[3],
                         const int32_t dst_stride[3]);
/* copy one frame slot's visible planes Y, U, V tightly packed (the reference sample's write_yuv
 * layout, tiny_mp2v_dec.cpp:11-17) to dst: HBM of the context's device when dst_on_device
 * (e.g. an RCCL send buffer for the rank-0 frame gather), else host memory; synchronous */
int  mp2vg_copy_slot_packed(mp2vg_ctx_t* ctx, int32_t slot, void* dst, int32_t dst_on_device);
/* raw device pointer of a slot (for in-HBM consumers such as a digest kernel or RCCL).  The
 * slot is READ-ONLY for callers: the motion-compensation taps read a reference from its anchor
 * tiles, a second copy the decode writes next to the frame (recon.hip), so bytes written through
 * this pointer are not seen by later predictions unless the caller then calls
 * mp2vg_invalidate_slot, which makes the next decode that reads the slot rebuild its tiles.
 * The pointer can change once, at the context's first mp2vg_batch_decode, when the pool's
 * placement calibration keeps a copy of the pool (mp2vg_pool_placement; contents are carried
 * over): fetch it after that decode, or turn the calibration off (MP2VG_PLACE_CANDIDATES=1).
 * Whether to calibrate is decided at that first decode alone: a context whose first batch was
 * not calibrated (pool below MP2VG_PLACE_MIN_MB, or a batch that overwrites a slot it read from
 * before it) never is, also not after mp2vg_reserve_slots has grown the pool (which adds blocks
 * and moves no slot). */
int  mp2vg_slot_device_ptr(mp2vg_ctx_t* ctx, int32_t slot, void** dptr);
/* the slot's frame was written by someone other than the decode (an RCCL receive, an external
 * producer writing through mp2vg_slot_device_ptr): its anchor tiles are stale.  The next batch
 * that predicts from the slot rebuilds them from the frame first (tile_convert).  Call it after
 * the writes have completed and before mp2vg_batch_decode of a batch that reads the slot. */
int  mp2vg_invalidate_slot(mp2vg_ctx_t* ctx, int32_t slot);
/* The pool's placement calibration (runtime.cpp calibrate_placement): at the first batch of a
 * context whose pool holds at least MP2VG_PLACE_MIN_MB (4096) MB, the batch is
 * decoded on the pool and on MP2VG_PLACE_CANDIDATES - 1 (default 2) copies of it in freshly
 * allocated blocks, and the pool with the shortest batch is kept; every candidate ends in the
 * same state, so no output changes.  The other candidates stay allocated until mp2vg_destroy
 * while an eighth of the device memory stays free (freeing them slowed the kept pool;
 * MP2VG_PLACE_HOLD=0 frees them).  MP2VG_PLACE_CANDIDATES=1 turns it off.  This returns the
 * measured batch times (ms[0..n): round 0 of each candidate, then round 1; n = 0 when it did not
 * run) and the candidate kept (0 = the pool as first allocated, -1 = none). */
int  mp2vg_pool_placement(mp2vg_ctx_t* ctx, float* ms, int32_t max, int32_t* n, int32_t* kept);
/* diagnostics: device address of the context's kernel sink block (dummy loads and stores of the
 * decode; from +3072 the per-stage cycle sums of a stamp build, tools/stamps.py).  Never written
 * by callers. */
int  mp2vg_sink_device_ptr(mp2vg_ctx_t* ctx, void** dptr);
/* diagnostics: the device's shader clock (GHz) while every SIMD issues VALU for ~1 ms (s_memtime
 * against the 100-MHz s_memrealtime); bench.py records it per box.  Synchronises the device. */
int  mp2vg_clock_probe(int32_t device, double* ghz);
/* the host threads a decoder uses when num_threads = 0: the hardware threads, capped by the
 * process's affinity mask and a cgroup v2 CPU quota (cpu.max); no device needed */
int  mp2vg_cpu_budget(void);
/* diagnostics (pool placement, tools/placement.py): per pool block (frames and tiles of 16 slots
 * each, in allocation order: frames, tiles, frames, ...) the HBM rate in GB/s of `reps` sweeps
 * that load every 16-B word and, with rw = 1, store it back unchanged.  gbps[i] for the first
 * `max` blocks; *nblocks = the pool's block count.  rw = 2: one rate (gbps[0], *nblocks = 1) for
 * 1-KB reads at random slots and offsets over the whole pool; rw = 3: the same with many slots read
 * at one offset at a time; rw = 4: per block, random 1-KB reads inside the block; rw = 5: load
 * sweeps over the two record banks (MB records, coefficient words: 4 rates, 0 where a bank is
 * not allocated); rw = 6 / 7: rw = 3 / 2 with each 1-KB run stored back unchanged.  Synchronises
 * the context; contents kept. */
int  mp2vg_pool_probe(mp2vg_ctx_t* ctx, int32_t rw, int32_t reps, double* gbps, int32_t max, int32_t* nblocks);
/* 64-bit order-independent digest of each listed slot's visible planes, computed on device:
 * sum over visible dwords d at (row, byte_x) of mix64(mix64((row << 32) | byte_x) ^ d) mod 2^64
 * (numpy twin: tiny_mp2v_dec_amd.records.planes_digest) */
int  mp2vg_slot_digests(mp2vg_ctx_t* ctx, const int32_t* slots, int32_t n, uint64_t* out);

/* ---- RGB export --------------------------------------------------------------------------
 * Decoded frames (strided planar Y'CbCr in HBM) to tight uint8 R'G'B' tensors in HBM, cropped to
 * a top-left anchored rectangle, one kernel launch per call (export.hip).  The reference stops at
 * frame_c; this is what a consumer on a card without a display does next.
 *
 * The arithmetic is bit-exact, signed 32-bit, >> an arithmetic shift, results clamped to 0..255.
 * Input is limited range (MPEG-2 always is), output full range:
 *     yt = cy (Y - 16) + 8192
 *     R = (yt + crv (Cr - 128)) >> 14
 *     G = (yt + cgu (Cb - 128) + cgv (Cr - 128)) >> 14
 *     B = (yt + cbu (Cb - 128)) >> 14
 * with the 14-bit coefficients of mp2vg_export_coefficients.  Cb and Cr at luma (x, y) are 8-bit
 * values, with MPEG-2 progressive siting (horizontally co-sited with even luma samples; 4:2:0:
 * vertically midway between two luma rows):
 *     NEAREST: C[4:2:0 ? y >> 1 : y][4:4:4 ? x : x >> 1]
 *     LINEAR:  (wv0 (C[j][k] + C[j][k1]) + wv1 (C[j1][k] + C[j1][k1]) + 4) >> 3, one rounding;
 *              4:2:0: j = y >> 1, j1 = j - 1 (y even) or j + 1 (y odd), wv0, wv1 = 3, 1; else
 *              j1 = j = y, wv0, wv1 = 4, 0;  4:2:0 / 4:2:2: k = x >> 1, k1 = k (x even) or k + 1
 *              (x odd); 4:4:4: k1 = k = x.  j1 and k1 clamp to the coded chroma plane, not to the
 *              exported rectangle: a crop filters with the real neighbouring samples.
 * The RGB export has no field mode: chroma is filtered as if the frame were progressive.  The
 * full-resolution deinterlaced (or field-sited) RGB image of an interlaced frame is an identity-size
 * U8 tensor export (out == src, Q = 64 P) with a MP2VG_FIELD_* mode, below. */
enum { MP2VG_EXPORT_RGB_PLANAR = 0 /* [n][3][h][w] */, MP2VG_EXPORT_RGB_PACKED = 1 /* [n][h][w][3] */ };
enum { MP2VG_EXPORT_CHROMA_NEAREST = 0, MP2VG_EXPORT_CHROMA_LINEAR = 1 };
typedef struct mp2vg_export {
    int32_t layout, matrix, chroma; /* MP2VG_EXPORT_RGB_*, matrix_coefficients code, MP2VG_EXPORT_CHROMA_* */
    int32_t width, height;   /* exported rectangle, top-left anchored, 1..coded; 0 = coded size */
    int32_t reserved[3];     /* must be 0 */
} mp2vg_export_t;

/* The fixed-point coefficients (cy, crv, cgu, cgv, cbu) of a matrix_coefficients code (ISO/IEC
 * 13818-2 Table 6-9): 1 BT.709, 4 FCC, 5 / 6 BT.470BG / SMPTE 170M, 7 SMPTE 240M; any other code
 * is MP2VG_E_INVALID.  Each is floor(x 2^14 + 1/2) of the exact rational, Kg = 1 - Kr - Kb:
 * cy = 255/219, crv = (255/224) 2 (1 - Kr), cbu = (255/224) 2 (1 - Kb),
 * cgu = -round((255/224) 2 (1 - Kb) Kb / Kg), cgv = -round((255/224) 2 (1 - Kr) Kr / Kg).
 * Host only; the kernel's constants come from this table. */
int  mp2vg_export_coefficients(int32_t matrix, int32_t out[5]);
/* (mp2vg_export_matrix, below the stream headers: the matrix code to export a stream with) */
/* bytes of the tensor n exported frames fill (n 3 w h), after validating the export against the
 * geometry of cfg; no device needed */
int  mp2vg_export_bytes(const mp2vg_config_t* cfg, const mp2vg_export_t* exp, int32_t n, uint64_t* bytes);
/* Export frame i from slot slots[i] (any order, repeats allowed: display order is a slot list; n
 * at most 65535) into the tight tensor at dst_device (any byte alignment; dst_bytes must equal
 * mp2vg_export_bytes), all n frames in one launch.  Asynchronous: enqueued on the context's main
 * stream behind every decode enqueued so far, complete after mp2vg_synchronize; a later
 * mp2vg_batch_decode waits for it before it overwrites a slot.  The slot list is copied before
 * the call returns.  The main stream is not ordered with streams of the caller's: other work on
 * dst must have finished before the call, and other streams read dst after mp2vg_synchronize.
 * Every argument is checked before the first HIP call. */
int  mp2vg_export_slots(mp2vg_ctx_t* ctx, const int32_t* slots, int32_t n, const mp2vg_export_t* exp,
                        void* dst_device, uint64_t dst_bytes);
/* The same kernel over one frame at arbitrary device plane pointers (a device frame inside the
 * render callback of an MP2VG_DECODER_DEVICE_FRAMES decoder, or a caller's own planes) of a
 * coded_w x coded_h frame: planes 4-byte aligned, strides multiples of 4 and at least the plane's
 * width (else MP2VG_E_INVALID), each plane readable over stride x plane height bytes.
 * Synchronous (a callback frame dies on return). */
int  mp2vg_export_planes(int32_t device, const uint8_t* const planes[3], const int32_t stride[3],
                         int32_t chroma_format, int32_t coded_w, int32_t coded_h, const mp2vg_export_t* exp,
                         void* dst_device, uint64_t dst_bytes);

/* ---- tensor export -----------------------------------------------------------------------
 * Decoded frames to cropped, antialias-resized, normalised model-input tensors in HBM, one kernel
 * launch per call (tensor.hip): Y'CbCr -> R'G'B', crop, both filter passes, normalise and cast in
 * one pass over the planes, with no full-size RGB intermediate in memory.  The result is defined
 * to the bit, by composition on top of the RGB export:
 *
 * 1. Source image.  The 8-bit R'G'B' image P of the WHOLE coded frame exactly as the RGB export
 *    above defines it (matrix, NEAREST or LINEAR chroma, chroma taps clamped to the coded chroma
 *    plane), cropped to the rectangle (src_x, src_y, src_w, src_h) in luma pixels: any integers
 *    inside the coded frame, odd origins included.  src_w = src_h = 0 (with src_x = src_y = 0)
 *    is the whole coded frame.
 * 2. Tap table of one axis (src source pixels of the rectangle, out output pixels): the triangle
 *    ("antialiased bilinear") filter with half-pixel centres, in exact rationals:
 *        r = src / out, s = max(r, 1), c(o) = (o + 1/2) r
 *        first = max(0, floor(c - s + 1/2)), end = min(src, floor(c + s + 1/2))
 *        t_j = max(0, 1 - |j + 1/2 - c| / s)                    for j in [first, end)
 *        q_j = floor(t_j / sum(t) 2^14 + 1/2), then 2^14 - sum(q) is added to the tap with the
 *        largest t_j (the lowest j on a tie)
 *    so the weights of an output are non-negative 14-bit integers that sum to exactly 16384.
 *    Taps outside the rectangle do not exist: nothing beyond the crop is read (the chroma taps of
 *    step 1 still reach the real neighbouring samples).  r <= 32 per axis (at most
 *    MP2VG_TENSOR_MAX_TAPS = 65 taps), else MP2VG_E_INVALID; out > src (upscaling) is allowed;
 *    out_w, out_h at most 16384.
 * 3. Vertical pass, then horizontal pass, per channel, signed 32-bit, >> an arithmetic shift:
 *        V[y][x] = (sum_j qv_j P[j][x] + 128) >> 8             6 fractional bits, 0..16320
 *        Q[y][x] = (sum_k qh_k V[y][k] + 8192) >> 14           units of 1/64 of an 8-bit step
 *    With out == src on both axes this is the identity, Q = 64 P.
 * 4. Output element of channel c:
 *        U8:   (Q + 32) >> 6; scale must be {1, 1, 1} and bias {0, 0, 0}
 *        F32:  fmaf(Q / 64, scale[c], bias[c]): one rounding of the exact value (Q / 64 is exact)
 *        F16 / BF16: that float32 value rounded to nearest even
 *    scale and bias must be finite.  (x / 255 - mean) / std is scale = 1 / (255 std), bias =
 *    -mean / std.
 * 5. Layout: planar [n][3][out_h][out_w] or packed [n][out_h][out_w][3] (MP2VG_EXPORT_RGB_*),
 *    tight; dst is aligned to the element size and no more.
 *
 * Field modes (mp2vg_tensor_slots_fields / mp2vg_tensor_planes_field), for frame pictures whose two
 * fields are 1/50 or 1/60 s apart (progressive_frame = 0: mp2vg_parsed_picture_flags).  A mode
 * replaces step 1 only: the rectangle, the tap tables (those of the unchanged rectangle, so the
 * output geometry is the same in every mode and a single field stays spatially aligned with the
 * frame), both passes, the normalisation and the layout are untouched.  H = the coded height;
 * L_p[y] = line y converted with the matrix arithmetic above and the FIELD CHROMA of parity
 * p = y & 1:
 *     4:2:2, 4:4:4: the progressive chroma of line y (no vertical subsampling).
 *     4:2:0: j = 2 (y >> 2) + (y & 1), the chroma row of the same field; k, k1 as in the RGB export.
 *         NEAREST: C[j][k]
 *         LINEAR:  (wv0 (C[j][k] + C[j][k1]) + wv1 (C[j1][k] + C[j1][k1]) + 8) >> 4, one rounding,
 *                  y mod 4 = 0: j1 = j - 2, wv0, wv1 = 7, 1      1: j1 = j - 2, 5, 3
 *                            2: j1 = j + 2, 5, 3                 3: j1 = j + 2, 7, 1
 *                  (the 1/4 and 3/4 line siting of interlaced 4:2:0); a j1 outside 0 .. ch - 1
 *                  becomes j, so it never leaves the field.
 *     (The progressive rule (3 A + B + 4) >> 3 equals (6 A + 2 B + 8) >> 4 exactly.)
 * MP2VG_FIELD_PROGRESSIVE: P as defined in step 1.
 * MP2VG_FIELD_WEAVE:  P[y] = L_{y & 1}[y]: both fields, each line with its own field's chroma
 *     (4:2:2 and 4:4:4: equal to PROGRESSIVE bit for bit).
 * MP2VG_FIELD_TOP (p = 0) / MP2VG_FIELD_BOTTOM (p = 1): P[y] = L_p[y] on lines of parity p; a line
 *     of the other parity is the rounded average per channel (L_p[a] + L_p[b] + 1) >> 1 of the 8-bit
 *     lines a = y - 1, b = y + 1; a < 0 becomes b and b > H - 1 becomes a (row 0 of BOTTOM is line 1,
 *     row H - 1 of TOP is line H - 2).  a and b are lines of the coded frame, not clamped to the
 *     rectangle (the rule of the chroma taps).
 * A mode other than PROGRESSIVE needs an even coded height, a multiple of 4 for 4:2:0 (every decoder
 * context has one), else MP2VG_E_INVALID.
 *
 * Placement (mp2vg_tensor_slots_placed / mp2vg_tensor_planes_placed): the resized picture fills the
 * rectangle (dst_x, dst_y, dst_w, dst_h) of the out_w x out_h output (the canvas) and every other
 * element is a pad colour: letterboxing / pillarboxing in the same launch.  Placement changes steps
 * 2, 3 and 5 only; step 1 is untouched, so every MP2VG_FIELD_* mode works with it as without.
 *     Step 2: the tap tables are those of (src_w -> dst_w) and (src_h -> dst_h).
 *     Step 3: the two passes give Q_img[dst_h][dst_w]; the canvas Q[y][x], 0 <= y < out_h and
 *             0 <= x < out_w, is Q_img[y - dst_y][x - dst_x] inside the rectangle and 64 pad[c]
 *             outside it.
 *     Step 4 runs over the whole canvas unchanged, so a pad element of channel c is pad[c] for U8,
 *             fmaf((float)pad[c], scale[c], bias[c]) for F32 (no special case) and that value
 *             rounded to nearest even for F16 / BF16.
 *     Step 5 is unchanged over the canvas, and so is mp2vg_tensor_bytes.
 * dst_x, dst_y >= 0, dst_w, dst_h >= 1, dst_x + dst_w <= out_w, dst_y + dst_h <= out_h, the reserved
 * fields 0, and the ratio rule of step 2 holds for the rectangle (src_w <= 32 dst_w, src_h <= 32
 * dst_h; out_w and out_h are then not judged by it), else MP2VG_E_INVALID.  A rectangle of four
 * zeros is the whole output: no placement, pad is never written.  One placement per launch.
 *
 * Items (mp2vg_tensor_items / mp2vg_tensor_planes_items): one launch writes n images of one common
 * out_w x out_h, dtype, layout and normalisation, each from its own source slot, field mode, source
 * rectangle and mirror flag (mp2vg_tensor_item_t): the random-resized-crop and flip of every sample
 * of a training batch, or every box of a detector cut from one frame.  Items change where step 1's
 * rectangle comes from, add a mirror between steps 3 and 4 and generalise step 5; the arithmetic of
 * every step is untouched.
 *     Steps 1 to 3: Q_i[out_h][out_w] is the image those steps give for item i's rectangle (src_x,
 *             src_y, src_w, src_h; all 0 = the whole coded frame) under its field mode: exactly what
 *             mp2vg_tensor_slots_fields defines for that rectangle and mode.  t->src_* must all be
 *             0.  The ratio rule of step 2 holds per item and per axis.
 *     Mirror: with MP2VG_ITEM_HFLIP the element at column x is Q_i[y][out_w - 1 - x]: a pure index
 *             reversal after both filter passes (not the filter over a mirrored source).
 *     Step 4 is unchanged.
 *     Step 5, packed: [n][out_h][out_w][3], unchanged; clip_len is only checked.
 *     Step 5, planar: with T = clip_len (>= 1, n a multiple of it), b = i / T and k = i % T the
 *             element is at (((b 3 + c) T + k) out_h + y) out_w + x: [n / T][3][T][out_h][out_w],
 *             the clip layout of video models.  T = 1 is [n][3][out_h][out_w].
 *     dst_bytes = n 3 out_w out_h element size, as mp2vg_tensor_bytes gives for any rectangle.
 * n is 1 .. 65535; flags holds no bit but MP2VG_ITEM_HFLIP and reserved is 0; a field mode other
 * than PROGRESSIVE has the precondition on the coded height above; else MP2VG_E_INVALID with
 * nothing written, and mp2vg_last_error names the index of the first offending item.
 * Tap tables are shared: items of one src_w use one horizontal table (whatever their origin or
 * height), items of one src_h one vertical table, so the staged bytes grow with the distinct
 * sizes of a launch, not with n (mp2vg_tensor_items_plan reports them).
 * Out of scope: motion-adaptive deinterlacing, filters other than the triangle, pad modes other
 * than a constant colour; for items: a vertical flip, a placement or pad per item (an items launch
 * has no placement), per-item output sizes and per-item normalisation. */
enum { MP2VG_TENSOR_U8 = 0, MP2VG_TENSOR_F16 = 1, MP2VG_TENSOR_BF16 = 2, MP2VG_TENSOR_F32 = 3 };
enum { MP2VG_FIELD_PROGRESSIVE = 0, MP2VG_FIELD_TOP = 1, MP2VG_FIELD_BOTTOM = 2, MP2VG_FIELD_WEAVE = 3 };
#define MP2VG_TENSOR_MAX_TAPS 65
typedef struct mp2vg_tensor {
    int32_t layout, matrix, chroma; /* as mp2vg_export_t */
    int32_t src_x, src_y, src_w, src_h; /* source rectangle, luma pixels; all 0 = the coded frame */
    int32_t out_w, out_h;    /* 1..16384, each at least 1/32 of the rectangle's side */
    int32_t dtype;           /* MP2VG_TENSOR_* */
    float   scale[3], bias[3]; /* per channel R, G, B */
    int32_t reserved[4];     /* must be 0 */
} mp2vg_tensor_t;            /* 80 bytes */

/* The tap table of one axis as the library computes it (integer arithmetic only; host only):
 * output o takes taps first[o] .. first[o] + count[o] - 1 with weights[o * max_taps + k], entries
 * from count[o] to max_taps zero.  first, count: out entries; weights: out * max_taps.
 * MP2VG_E_INVALID when src < 1, out < 1, out > 16384, src > 32 out, or an output has more than
 * max_taps taps (MP2VG_TENSOR_MAX_TAPS always suffices). */
int  mp2vg_tensor_weights(int32_t src, int32_t out, int32_t* first, int32_t* count, int32_t* weights,
                          int32_t max_taps);
/* bytes of the tensor n frames fill (n 3 out_w out_h element size), after validating t against
 * the geometry of cfg; no device needed */
int  mp2vg_tensor_bytes(const mp2vg_config_t* cfg, const mp2vg_tensor_t* t, int32_t n, uint64_t* bytes);
/* Frame i from slot slots[i] (any order, repeats allowed; n at most 65535) into the tight tensor
 * at dst_device (aligned to the element size; dst_bytes must equal mp2vg_tensor_bytes), all n
 * frames in one launch.  Ordering as mp2vg_export_slots, whose events it shares: asynchronous on
 * the context's main stream behind every decode enqueued so far, complete after
 * mp2vg_synchronize; a later mp2vg_batch_decode waits for it before it overwrites a slot.  The
 * slot list and the two tap tables are copied before the call returns.  The main stream is not
 * ordered with streams of the caller's (see mp2vg_export_slots).  Every argument is checked
 * before the first HIP call. */
int  mp2vg_tensor_slots(mp2vg_ctx_t* ctx, const int32_t* slots, int32_t n, const mp2vg_tensor_t* t,
                        void* dst_device, uint64_t dst_bytes);
/* The same kernel over one frame at arbitrary device plane pointers, with the plane
 * preconditions of mp2vg_export_planes.  Synchronous. */
int  mp2vg_tensor_planes(int32_t device, const uint8_t* const planes[3], const int32_t stride[3],
                         int32_t chroma_format, int32_t coded_w, int32_t coded_h, const mp2vg_tensor_t* t,
                         void* dst_device, uint64_t dst_bytes);
/* mp2vg_tensor_slots with a field mode per frame of the launch: frame i is slot slots[i] in mode
 * fields[i] (MP2VG_FIELD_*; fields = NULL: all PROGRESSIVE, which is mp2vg_tensor_slots bit for
 * bit).  Both fields of each picture in temporal order is one launch with every slot listed twice.
 * Ordering, staging and limits as mp2vg_tensor_slots; the field list is copied with the slot list
 * before the call returns.  A field value outside 0..3 is MP2VG_E_INVALID, nothing written; every
 * argument is checked before the first HIP call. */
int  mp2vg_tensor_slots_fields(mp2vg_ctx_t* ctx, const int32_t* slots, const int32_t* fields, int32_t n,
                               const mp2vg_tensor_t* t, void* dst_device, uint64_t dst_bytes);
/* mp2vg_tensor_planes in one field mode (field = MP2VG_FIELD_PROGRESSIVE: mp2vg_tensor_planes). */
int  mp2vg_tensor_planes_field(int32_t device, const uint8_t* const planes[3], const int32_t stride[3],
                               int32_t chroma_format, int32_t coded_w, int32_t coded_h, int32_t field,
                               const mp2vg_tensor_t* t, void* dst_device, uint64_t dst_bytes);

/* Placement (the contract is in the block above the enums). */
typedef struct mp2vg_tensor_place {
    int32_t dst_x, dst_y, dst_w, dst_h; /* the picture's rectangle inside out_w x out_h; all 0 = the whole output */
    uint8_t pad[3];                     /* 8-bit R'G'B' of every element outside it */
    uint8_t reserved0;                  /* must be 0 */
    int32_t reserved[3];                /* must be 0 */
} mp2vg_tensor_place_t;                 /* 32 bytes */
/* mp2vg_tensor_slots_fields / mp2vg_tensor_planes_field with a placement: ordering, staging and
 * limits as those.  place = NULL (or its rectangle all 0) is the call without a placement bit for
 * bit, through the same kernels.  Every argument is checked before the first HIP call. */
int  mp2vg_tensor_slots_placed(mp2vg_ctx_t* ctx, const int32_t* slots, const int32_t* fields, int32_t n,
                               const mp2vg_tensor_t* t, const mp2vg_tensor_place_t* place,
                               void* dst_device, uint64_t dst_bytes);
int  mp2vg_tensor_planes_placed(int32_t device, const uint8_t* const planes[3], const int32_t stride[3],
                                int32_t chroma_format, int32_t coded_w, int32_t coded_h, int32_t field,
                                const mp2vg_tensor_t* t, const mp2vg_tensor_place_t* place,
                                void* dst_device, uint64_t dst_bytes);

/* The rectangles of a placement from the shape the source is shown at (host only, 64-bit integer
 * arithmetic).  src = (x, y, w, h) is the source rectangle, par_n : par_d the pixel's width :
 * height (each 1 .. 2^24), so the displayed shape is A : B with A = w par_n, B = h par_d;
 * rnd(p, q) = floor((2 p + q) / (2 q)).
 *   MP2VG_FIT_STRETCH: src_out = src, dst_out = (0, 0, out_w, out_h).
 *   MP2VG_FIT_CONTAIN (letterbox / pillarbox, centred): src_out = src; if A out_h >= B out_w:
 *       dst_w = out_w, dst_h = clamp(rnd(B out_w, A), 1, out_h), else dst_h = out_h,
 *       dst_w = clamp(rnd(A out_h, B), 1, out_w); dst_x = (out_w - dst_w) >> 1, dst_y likewise.
 *   MP2VG_FIT_COVER (the centre crop that fills the output): dst_out = (0, 0, out_w, out_h); if
 *       A out_h >= B out_w: h kept, w' = clamp(rnd(h par_d out_w, par_n out_h), 1, w),
 *       x' = x + ((w - w') >> 1), else w kept, h' = clamp(rnd(w par_n out_h, par_d out_w), 1, h),
 *       y' = y + ((h - h') >> 1).
 * src_out goes into mp2vg_tensor_t.src_*, dst_out into mp2vg_tensor_place_t.dst_*.
 * MP2VG_E_INVALID for a mode outside MP2VG_FIT_*, x or y below 0, w, h, out_w or out_h outside
 * 1 .. 16384, par out of range, or a result whose ratio is above 32 on an axis (the export would
 * refuse it). */
enum { MP2VG_FIT_STRETCH = 0, MP2VG_FIT_CONTAIN = 1, MP2VG_FIT_COVER = 2 };
int  mp2vg_tensor_fit(int32_t mode, const int32_t src[4], int32_t par_n, int32_t par_d,
                      int32_t out_w, int32_t out_h, int32_t src_out[4], int32_t dst_out[4]);

/* Items (the contract is in the block above the enums). */
enum { MP2VG_ITEM_HFLIP = 1 };
typedef struct mp2vg_tensor_item {
    int32_t slot;                        /* source slot (must be 0 in the planes call) */
    int32_t field;                       /* MP2VG_FIELD_* */
    int32_t src_x, src_y, src_w, src_h;  /* luma pixels; all 0 = the whole coded frame */
    int32_t flags;                       /* MP2VG_ITEM_HFLIP or 0 */
    int32_t reserved;                    /* must be 0 */
} mp2vg_tensor_item_t;                   /* 32 bytes */
/* Image i from items[i] (slots in any order, repeats allowed), all n in one launch.  Ordering,
 * staging ring, events and limits as mp2vg_tensor_slots; the item records and the shared tap tables
 * are copied before the call returns.  Every argument is checked before the first HIP call. */
int  mp2vg_tensor_items(mp2vg_ctx_t* ctx, const mp2vg_tensor_item_t* items, int32_t n,
                        const mp2vg_tensor_t* t, int32_t clip_len, void* dst_device, uint64_t dst_bytes);
/* The same kernel over one frame at arbitrary device plane pointers (preconditions of
 * mp2vg_tensor_planes; every item's slot is 0): many rectangles of one device frame, for example
 * inside a render callback.  Synchronous, like mp2vg_tensor_planes_placed. */
int  mp2vg_tensor_planes_items(int32_t device, const uint8_t* const planes[3], const int32_t stride[3],
                               int32_t chroma_format, int32_t coded_w, int32_t coded_h,
                               const mp2vg_tensor_item_t* items, int32_t n, const mp2vg_tensor_t* t,
                               int32_t clip_len, void* dst_device, uint64_t dst_bytes);
/* Host only, no device: validates t, items, n and clip_len exactly as mp2vg_tensor_items does for a
 * context of cfg (a slot is checked to be >= 0 only: the slot count belongs to the context) and
 * reports the launch.  htab[i] / vtab[i] (n entries each, or NULL): the index of item i's
 * horizontal / vertical tap table, tables numbered in order of first use.  summary = {distinct
 * horizontal tables, distinct vertical tables, grid.x (the largest segment count of any item), int32
 * words staged (item records, then the tables)}. */
int  mp2vg_tensor_items_plan(const mp2vg_config_t* cfg, const mp2vg_tensor_t* t,
                             const mp2vg_tensor_item_t* items, int32_t n, int32_t clip_len,
                             int32_t* htab, int32_t* vtab, int32_t summary[4]);

/* ---- motion export -----------------------------------------------------------------------
 * The compressed domain as tensors: the motion field and the coded residual's activity on the
 * macroblock grid, read from the resident record batch (mp2vg_batch_upload or
 * mp2vg_batch_upload_es) and not from the frame slots, so no decode is needed (motion.hip).  All
 * arithmetic is integer and every output is defined to the bit.
 *
 * order[n] lists indices into the batch's pictures (any order, repeats allowed).  Picture p has
 * M = mb_width * mb_height cells; cell i, in raster order, is record mb_first + i.  Three optional
 * tight tensors (a NULL pointer: not wanted); B = blocks per macroblock (6, 8 or 12):
 *
 * mv: int16 [n][8][mbh][mbw].  Channel c = 4 s + 2 r + k: s the direction (0 forward, 1 backward),
 *     r the vector / destination field (0 top lines, 1 bottom lines), k = 0 for x, 1 for y.  Units
 *     are FRAME half-pel luma units: the prediction of a destination sample is read at its
 *     position plus the vector.  Direction s is used when the MB is not MP2VG_MB_INTRA and its
 *     flag bit (FWD for s = 0, BWD for s = 1) is set, or s = 0 and neither bit is set (the
 *     decode's own rule).
 *         unused direction:       the four channels of s are 0, whatever the record's mv holds
 *         used, frame MC:         both r carry mv[0][s][k]
 *         used, MP2VG_MB_FIELD_MC: x = mv[r][s][0], y = 2 mv[r][s][1] + 2 (sel - r), sel = 1 when
 *                                 MP2VG_MB_FS_BIT(r, s) is set, else 0
 *     (the record's vertical component is in field half-pels, and destination lines r, r + 2, ...
 *     read reference lines of parity sel: mv_y + sel - r frame lines).  Every value fits int16 for
 *     f_code <= 9.
 * info: uint16 [n][4][mbh][mbw]: flags & 0x0F1F (the five type bits and the four field selects),
 *     cbp, qscale, ncoef.
 * act: int32 [n][2][B][mbh][mbw], over the MB's words [coef_off, coef_off + ncoef), block b =
 *     MP2VG_COEF_BLOCK: plane 0 the number of words of block b (DC and '1s' words included); plane
 *     1 the sum of |level| (MP2VG_COEF_LEVEL, absolute value in 32 bits; a '1s' word counts 1) over
 *     the words of block b without MP2VG_COEF_DC.  A word whose block index is >= B is ignored. */
/* byte sizes of mv, info and act for n pictures (1 .. 65535) of the geometry; host only */
int  mp2vg_motion_bytes(const mp2vg_config_t* cfg, int32_t n, uint64_t bytes[3]);
/* The host twin: the same tensors from host records into host buffers, no device needed.  Rejects
 * a record batch exactly as mp2vg_batch_validate does (over a pool of as many slots as the
 * pictures name), then n and order as mp2vg_motion_batch; nothing is written on failure. */
int  mp2vg_motion_records(const mp2vg_config_t* cfg, const mp2vg_picture_t* pics, int32_t npics,
                          const mp2vg_mb_t* mbs, uint64_t nmbs, const uint32_t* coefs, uint64_t ncoefs,
                          const int32_t* order, int32_t n, int16_t* mv, uint16_t* info, int32_t* act);
/* The resident batch's tensors into device memory of the context's device: at least one of mv,
 * info, act non-NULL, each 4-byte aligned, and bytes[t] of each given tensor equal to
 * mp2vg_motion_bytes.  MP2VG_E_STATE when no batch is resident; MP2VG_E_INVALID for n <= 0,
 * n > 65535, an index outside the batch's pictures, no output, a wrong size or alignment, with the
 * reason in mp2vg_last_error() and nothing written.  Asynchronous like mp2vg_export_slots: one
 * enqueue on the context's main stream behind the batch's upload (for mp2vg_batch_upload_es,
 * behind its emit pass), complete after mp2vg_synchronize; needs no mp2vg_batch_decode and does
 * not disturb one.  The upload that next reuses the batch's bank waits for it.  The order list is
 * copied before the call returns; the main stream is not ordered with streams of the caller's
 * (see mp2vg_export_slots). */
int  mp2vg_motion_batch(mp2vg_ctx_t* ctx, const int32_t* order, int32_t n, void* mv, void* info, void* act,
                        const uint64_t bytes[3]);
/* diagnostics: device time (ms, HIP events on the main stream) of the kernels of the last
 * mp2vg_motion_batch, the order list's copy excluded; waits for them.  MP2VG_E_STATE before the
 * first one (tools/motion_bench.py). */
int  mp2vg_last_motion_time(mp2vg_ctx_t* ctx, float* ms);

/* ---- residual export ---------------------------------------------------------------------
 * The coded prediction error as sample planes: what the stream codes for each block after
 * dequantisation and the inverse transform and BEFORE it is added to the prediction, read from the
 * resident record batch like the motion export (no decode, no slots), one kernel launch per call
 * (residual.hip).  All arithmetic is integer and every output is defined to the bit.
 *
 * For picture p and macroblock m, block b (0 .. B - 1) is coded when bit b of cbp is set.  Its 64
 * coefficients QFS are what the decode makes of the MB's words [coef_off, coef_off + ncoef) whose
 * MP2VG_COEF_BLOCK is b, in any order (reference parse_block, mb_decoder.cpp:74-155): matrix
 * W[(b < 6 ? 0 : 2) + (intra ? 0 : 1)], the MB's qscale, the picture's alternate_scan; a word with
 * MP2VG_COEF_DC sets QFS[0] to its level and stays out of the mismatch sum; a FIRST1S word is
 * (3 W[i] qs) >> 5 with the level's sign, unclamped; any other word is (|level| W[i] qs) >> 4
 * (intra) or ((2 |level| + 1) W[i] qs) >> 5, signed, truncated to int16 and then clamped to
 * -2048 .. 2047; position 63 has bit 0 toggled when the sum of the words' values is even.  A coded
 * block without words is legal: all zeros with position 63 toggled to 1.  A word whose block is
 * not coded, or is >= B, is ignored.
 *     r[y][x] = idct(QFS)[y][x] >> 6
 * is the int16 value the reference adds to the prediction (inverse_dct_template, idct_sse2.hpp:
 * 96-120: both saturating 16-bit passes, then the arithmetic shift, before adds / packus).  The
 * exported value is
 *     MP2VG_RESIDUAL_I16: R = clamp(r, -255, 255)        MP2VG_RESIDUAL_I8: R = clamp(r, -128, 127)
 * The int16 clamp loses nothing reconstruction can see: clip8(p + r) == clip8(p + clamp(r, -255,
 * 255)) for every p in 0 .. 255.
 * Placement is the decode's (mb_decoder.cpp:166-196): luma blocks 0-3 and chroma blocks 4 .. B - 1
 * at their MB's position in planes of the CODED size; MP2VG_MB_DCT_FIELD interleaves the lines of
 * luma, and of chroma where the format is not 4:2:0.  Every sample of a block that is not coded is
 * 0 (skipped MBs have cbp = 0).  Intra MBs are exported like any other (clip8(R) is their decoded
 * sample); with MP2VG_RESIDUAL_ZERO_INTRA they are written as zeros.  Records that repeat a scan
 * position inside one block cannot come from a parser: the values of that block are unspecified,
 * as the decode's are, and nothing outside the outputs is touched.
 *
 * order[n] as in the motion export (1 .. 65535 entries).  Three optional tight tensors of int16 or
 * int8 elements (NULL: not wanted): y [n][H][W], cb and cr [n][ch][cw] at the chroma format's plane
 * size; cb and cr are given together or not at all, and at least one of the three is given.  Every
 * element of every given tensor is written exactly once (the zeros too); nothing is read back. */
enum { MP2VG_RESIDUAL_I16 = 0, MP2VG_RESIDUAL_I8 = 1 };
enum { MP2VG_RESIDUAL_ZERO_INTRA = 1 };
/* byte sizes of y, cb and cr for n pictures (1 .. 65535) of the geometry; host only */
int  mp2vg_residual_bytes(const mp2vg_config_t* cfg, int32_t n, int32_t dtype, uint64_t bytes[3]);
/* The host twin: the same planes from host records into host buffers, no device needed.  Rejects a
 * record batch exactly as mp2vg_motion_records does, then n, order, dtype, flags and the outputs
 * as mp2vg_residual_batch (host buffers may have any alignment); nothing is written on failure. */
int  mp2vg_residual_records(const mp2vg_config_t* cfg, const mp2vg_picture_t* pics, int32_t npics,
                            const mp2vg_mb_t* mbs, uint64_t nmbs, const uint32_t* coefs, uint64_t ncoefs,
                            const int32_t* order, int32_t n, int32_t dtype, int32_t flags, void* y, void* cb,
                            void* cr);
/* The resident batch's planes into device memory of the context's device: each given pointer
 * 16-byte aligned and bytes[t] of each given tensor equal to mp2vg_residual_bytes.  MP2VG_E_STATE
 * when no batch is resident; MP2VG_E_INVALID for a bad n, index, dtype, flag bit, size or
 * alignment, no output, or cb without cr, with the reason in mp2vg_last_error() and nothing
 * written.  Asynchronous and ordered exactly like mp2vg_motion_batch: one enqueue on the context's
 * main stream behind the batch's upload (mp2vg_batch_upload or mp2vg_batch_upload_es), complete
 * after mp2vg_synchronize; needs no mp2vg_batch_decode and does not disturb one; the upload that
 * next reuses the bank waits for it.  The order list is copied before the call returns. */
int  mp2vg_residual_batch(mp2vg_ctx_t* ctx, const int32_t* order, int32_t n, int32_t dtype, int32_t flags,
                          void* y, void* cb, void* cr, const uint64_t bytes[3]);
/* diagnostics: device time (ms, HIP events on the main stream) of the kernel of the last
 * mp2vg_residual_batch, the order list's copy excluded; waits for it.  MP2VG_E_STATE before the
 * first one (tools/residual_bench.py). */
int  mp2vg_last_residual_time(mp2vg_ctx_t* ctx, float* ms);

/* ---- stream headers ----------------------------------------------------------------------
 * The sequence-level headers the reference keeps as public members of mp2v_decoder_c
 * (decoder.h:124-130), with the reference's field names (mp2v_hdr.h:61-141) and parsed the way
 * the reference parses them (mp2v_hdr.cpp:4-83): a later header of the same kind overwrites an
 * earlier one, the matrices are the 64 bytes as transmitted, fields a header does not carry stay
 * 0, and the start-code fields hold the 32-bit start code (extension_start_code stays 0, as the
 * reference never sets it).  Scalable extensions are outside the decodable subset (rejected). */
typedef struct mp2vg_sequence_header {
    uint32_t sequence_header_code, horizontal_size_value, vertical_size_value, aspect_ratio_information,
             frame_rate_code, bit_rate_value, vbv_buffer_size_value, constrained_parameters_flag,
             load_intra_quantiser_matrix;
    uint8_t  intra_quantiser_matrix[64];
    uint32_t load_non_intra_quantiser_matrix;
    uint8_t  non_intra_quantiser_matrix[64];
} mp2vg_sequence_header_t;
typedef struct mp2vg_sequence_extension {
    uint32_t extension_start_code, extension_start_code_identifier, profile_and_level_indication,
             progressive_sequence, chroma_format, horizontal_size_extension, vertical_size_extension,
             bit_rate_extension, vbv_buffer_size_extension, low_delay, frame_rate_extension_n,
             frame_rate_extension_d;
} mp2vg_sequence_extension_t;
typedef struct mp2vg_sequence_display_extension {
    uint32_t extension_start_code_identifier, video_format, colour_description, colour_primaries,
             transfer_characteristics, matrix_coefficients, display_horizontal_size, display_vertical_size;
} mp2vg_sequence_display_extension_t;
typedef struct mp2vg_sequence_scalable_extension {
    uint32_t extension_start_code_identifier, scalable_mode, layer_id, lower_layer_prediction_horizontal_size,
             lower_layer_prediction_vertical_size, horizontal_subsampling_factor_m,
             horizontal_subsampling_factor_n, vertical_subsampling_factor_m, vertical_subsampling_factor_n,
             picture_mux_enable, mux_to_progressive_sequence, picture_mux_order, picture_mux_factor;
} mp2vg_sequence_scalable_extension_t;
typedef struct mp2vg_group_of_pictures_header {
    uint32_t group_start_code, time_code, closed_gop, broken_link;
} mp2vg_group_of_pictures_header_t;
typedef struct mp2vg_stream_headers {
    int32_t have_sequence_display_extension;  /* reference: m_sequence_display_extension != nullptr */
    int32_t have_group_of_pictures_header;    /* reference: m_group_of_pictures_header != nullptr   */
    mp2vg_sequence_header_t sequence_header;
    mp2vg_sequence_extension_t sequence_extension;
    mp2vg_sequence_display_extension_t sequence_display_extension;
    mp2vg_group_of_pictures_header_t group_of_pictures_header; /* the last one in the stream      */
} mp2vg_stream_headers_t;

/* The matrix code to export a stream with (RGB export, above): its matrix_coefficients when the
 * sequence display extension carries a colour description and the code is 1, 4, 5, 6 or 7; 1
 * (BT.709, the assumption of 13818-2 6.3.6) when the extension or the description is absent or
 * the code is 2 ("unspecified"); MP2VG_E_UNSUPPORTED for 0, 3 and codes above 7. */
int  mp2vg_export_matrix(const mp2vg_stream_headers_t* headers, int32_t* matrix);

/* The pixel aspect par_n : par_d (pixel width : pixel height, reduced) of a stream, for
 * mp2vg_tensor_fit (13818-2 6.3.3).  aspect_ratio_information 1 is 1:1.  Codes 2, 3 and 4 are the
 * display aspect ratios dw : dh = 4:3, 16:9 and 221:100 of W x H, which is display_horizontal_size x
 * display_vertical_size when the sequence display extension is present and both are non-zero, else
 * horizontal_size_value | horizontal_size_extension << 12 and the height likewise; then par =
 * (dw H) : (dh W) reduced by their gcd (720 x 576 at 16:9 is 64:45).  MP2VG_E_UNSUPPORTED for code
 * 0 and codes 5..15; MP2VG_E_INVALID for a size of 0. */
int  mp2vg_stream_pixel_aspect(const mp2vg_stream_headers_t* headers, int32_t* par_n, int32_t* par_d);

/* What a config for a stream must hold, from the stream itself (host only, no context): the first
 * sequence_header and the sequence_extension that follows it.  Writes cfg->chroma_format and the
 * CODED size: cfg->width = 16 * ceil(h / 16); cfg->height = 16 * ceil(v / 16) when
 * progressive_sequence is set, else 32 * ceil(v / 32) (13818-2 6.3.3), h and v the 14-bit sizes
 * (value | extension << 12).  The other cfg fields stay as passed.  *headers (optional) gets those
 * two headers and a sequence_display_extension that follows them; the display size, pixel aspect
 * and export matrix come from it as from any mp2vg_stream_headers_t.  MP2VG_E_BITSTREAM when no
 * sequence_header is found; MP2VG_E_UNSUPPORTED, with a message, for an MPEG-1 stream (no
 * sequence_extension behind the header) and for a coded size above MP2VG_MAX_DIMENSION; cfg is
 * written only on MP2VG_OK. */
int  mp2vg_probe_es(const uint8_t* buf, uint64_t len, mp2vg_config_t* cfg, mp2vg_stream_headers_t* headers);

/* ---- host record emitter -------------------------------------------------------------- */
typedef struct mp2vg_parsed mp2vg_parsed_t;

/* Parse a whole elementary stream into records.  Pictures are numbered in decode order and
 * slot ids are decode indices (dst_slot = i; refs point at earlier indices).  Validates the
 * reference's input contract and returns MP2VG_E_UNSUPPORTED outside it.  Part of
 * that contract: the reference reads slice_vertical_position_extension when the 12-bit
 * vertical_size_value is above 2800, so a stream whose vertical_size (14 bits) is above 2800 while
 * its low 12 bits are not (4112 lines) is refused, with a reason that names vertical_size; 16384
 * coded lines decode as vertical_size 16383.  cfg holds the coded size (MP2VG_MAX_DIMENSION). */
int  mp2vg_parse_es(const uint8_t* buf, uint64_t len, const mp2vg_config_t* cfg,
                    mp2vg_parsed_t** out);
int  mp2vg_parsed_counts(const mp2vg_parsed_t* p, int32_t* npics, uint64_t* nmbs,
                         uint64_t* ncoefs);
const mp2vg_picture_t* mp2vg_parsed_pictures(const mp2vg_parsed_t* p);
const mp2vg_mb_t*      mp2vg_parsed_mbs(const mp2vg_parsed_t* p);
const uint32_t*        mp2vg_parsed_coefs(const mp2vg_parsed_t* p);
/* display order (decode indices), as the reference's output scheduler emits them */
int  mp2vg_parsed_display_order(const mp2vg_parsed_t* p, int32_t* order, int32_t n);
/* GOP index (0-based, by group_start_code) of each picture, for GOP sharding */
int  mp2vg_parsed_gop_index(const mp2vg_parsed_t* p, int32_t* gop, int32_t n);
/* interlace flags of each picture (decode order), from its picture_coding_extension: which
 * pictures hold two fields 1/50 or 1/60 s apart (progressive_frame = 0) and which field is the
 * earlier one: what a caller needs to pick the MP2VG_FIELD_* mode of a tensor export.  Returns the
 * number of pictures. */
enum { MP2VG_PIC_PROGRESSIVE_FRAME = 1, MP2VG_PIC_TOP_FIELD_FIRST = 2, MP2VG_PIC_REPEAT_FIRST_FIELD = 4,
       /* MP2VG_PARSE_CONCEAL: the picture has a concealed row; it is an I picture whose record was
        * re-typed to picture_coding_type 2 (it predicts the concealed rows from its conceal reference) */
       MP2VG_PIC_CONCEALED = 8, MP2VG_PIC_RETYPED_I = 16 };
int  mp2vg_parsed_picture_flags(const mp2vg_parsed_t* p, uint32_t* flags, int32_t n);
/* MP2VG_PARSE_CONCEAL: one entry per replaced macroblock row, in stream order (a picture's damaged
 * slices in stream order, then its missing rows ascending).  pic is relative to the parsed stream
 * or the uploaded range; status and reason are the rejection the slice would have been
 * (mp2vg_damage_reason_string(reason) is the text after "picture P slice @O: " of that message);
 * byte_off is the slice's start code in the stream, or the picture's start code for a missing row. */
typedef struct mp2vg_damage {
    int32_t  pic, mb_row, status, reason;
    uint64_t byte_off;
} mp2vg_damage_t;
/* out[0 .. min(*n, max)) are written (out may be NULL with max 0); *n is the true count */
int  mp2vg_parsed_damage(const mp2vg_parsed_t* p, mp2vg_damage_t* out, int32_t max, int32_t* n);
const char* mp2vg_damage_reason_string(int32_t reason);
/* sequence headers of the parsed stream (see mp2vg_stream_headers_t) */
int  mp2vg_parsed_stream_headers(const mp2vg_parsed_t* p, mp2vg_stream_headers_t* out);
/* Independent shards for GOP sharding: shard[i] of each picture (decode order), numbered from 0.
 * A shard is a maximal run of pictures, in decode order, that no later picture predicts across:
 * a closed GOP (or several open GOPs chained by their leading B pictures), since a picture's
 * references are only the two latest anchors (reference decoder.cpp:299-304).  The B pictures
 * between the first two anchors of a GOP whose header has closed_gop = 1 predict backward only
 * (ISO/IEC 13818-2 6.3.8), so their picture-level forward anchor (the previous GOP's last one,
 * reference decoder.cpp:299-304) does not join the shards; the multi-device decoder refuses
 * (MP2VG_E_UNSUPPORTED) such a picture if a macroblock of it does predict forward.  Returns the
 * number of shards. */
int  mp2vg_parsed_shards(const mp2vg_parsed_t* p, int32_t* shard, int32_t n);
void mp2vg_parsed_free(mp2vg_parsed_t* p);

/* ---- host scan + device parse ------------------------------------------------------------
 * mp2vg_scan_es is pass 1 of mp2vg_parse_es on its own: start codes, headers, picture records
 * with W matrices, references, display order, GOP index, shards and stream headers, plus a slice
 * table (picture, macroblock row, byte range) and the few header fields per picture the
 * macroblock syntax depends on.  It rejects what mp2vg_parse_es rejects at picture level, and
 * itself makes the host emitter's three row rejections (slice row outside the picture, two slices
 * in one macroblock row, row not covered by any slice; MP2VG_E_UNSUPPORTED), so every slice of
 * the table owns its row.  The scan keeps a pointer to buf: the stream must outlive it.
 * mp2vg_batch_upload_es (below) sends the bitstream of a picture range to the device, where one
 * lane per slice parses it into the records mp2vg_parse_es would have produced, byte for byte. */
typedef struct mp2vg_scan mp2vg_scan_t;
int  mp2vg_scan_es(const uint8_t* buf, uint64_t len, const mp2vg_config_t* cfg, mp2vg_scan_t** out);
int  mp2vg_scan_counts(const mp2vg_scan_t* s, int32_t* npics, uint64_t* nslices);
const mp2vg_picture_t* mp2vg_scan_pictures(const mp2vg_scan_t* s);
int  mp2vg_scan_display_order(const mp2vg_scan_t* s, int32_t* order, int32_t n);
int  mp2vg_scan_gop_index(const mp2vg_scan_t* s, int32_t* gop, int32_t n);
int  mp2vg_scan_picture_flags(const mp2vg_scan_t* s, uint32_t* flags, int32_t n); /* as mp2vg_parsed_picture_flags */
int  mp2vg_scan_shards(const mp2vg_scan_t* s, int32_t* shard, int32_t n);
int  mp2vg_scan_stream_headers(const mp2vg_scan_t* s, mp2vg_stream_headers_t* out);
void mp2vg_scan_free(mp2vg_scan_t* s);
/* The CPU twin of the device parse (host only, no device needed): the kernels' own slice parser
 * (csrc/slice_parse.h), slice by slice over pictures [first, first + npics) -- count pass,
 * prefix sum, emit pass -- on a copy of the range's bitstream of exactly the device's size.
 * With mbs = coefs = NULL it only counts: *nmbs_out and *ncoefs_out (either may be NULL) are the
 * array sizes of the second call, which fills mbs[nmbs] and coefs[ncoefs] (both must equal the
 * counts) laid out as mp2vg_parse_es lays them out, picture `first` at record 0.  A rejected
 * slice returns the host emitter's status and sets its message.  MP2VG_E_STATE is an internal
 * failure (the iteration bound of a slice exceeded, or the two passes disagree). */
int  mp2vg_scan_parse_host(const mp2vg_scan_t* s, int32_t first, int32_t npics, mp2vg_mb_t* mbs, uint64_t nmbs,
                           uint32_t* coefs, uint64_t ncoefs, uint64_t* nmbs_out, uint64_t* ncoefs_out);
/* Upload pictures [first, first + npics) of a scanned stream as a record batch parsed on the
 * device (parse.hip): the range's bitstream crosses to HBM, a count pass (one lane per slice)
 * writes the MB records and counts each slice's coefficient words, a prefix sum lays the words
 * out as mp2vg_parse_es does, and an emit pass writes them.  pics = NULL uses the scan's picture
 * records with mb_first rebased to the range; otherwise pics[npics] are the range's records with
 * the caller's slots and mb_first (picture i's records at mb_first, all inside npics pictures'
 * worth of records).  Synchronous up to the count pass: a rejected slice returns the host
 * emitter's status for the first failing slice in stream order, with its message in
 * mp2vg_last_error(); no batch is then resident (mp2vg_batch_decode: MP2VG_E_STATE) and the
 * context stays usable.  The resident batch decodes, exports and times like any other. */
int  mp2vg_batch_upload_es(mp2vg_ctx_t* ctx, const mp2vg_scan_t* scan, const mp2vg_picture_t* pics,
                           int32_t first, int32_t npics);
/* sizes of the resident batch's record arrays, and a copy of them (synchronous; sizes must match) */
int  mp2vg_batch_record_counts(mp2vg_ctx_t* ctx, uint64_t* nmbs, uint64_t* ncoefs);
int  mp2vg_batch_download_records(mp2vg_ctx_t* ctx, mp2vg_mb_t* mbs, uint64_t nmbs, uint32_t* coefs,
                                  uint64_t ncoefs);
/* device times (ms, HIP events) of the last mp2vg_batch_upload_es: count pass, scan, emit pass */
int  mp2vg_last_parse_times(mp2vg_ctx_t* ctx, float ms[3]);
/* the rows the last mp2vg_batch_upload_es replaced (scan with MP2VG_PARSE_CONCEAL; empty otherwise
 * and after a clean upload); as mp2vg_parsed_damage, pic relative to the uploaded range.  Damaged I
 * pictures with a conceal reference were re-typed in the resident picture records. */
int  mp2vg_last_upload_damage(mp2vg_ctx_t* ctx, mp2vg_damage_t* out, int32_t max, int32_t* n);

/* Conformance hook: decode one Annex B code (MSB-first 64-bit window: the code, then whatever
 * follows) with the emitter's own decoders.  Tables follow the reference's VLC decoders
 * (mp2v_vlc_dec.hpp:36-267) except where the emitter reads more: MOTION consumes the sign bit
 * and returns the signed motion_code; COEF_B14/B15 consume the sign bit (or the escape's run
 * and level) and return run in *value and the signed level in *aux (EOB: *value = -1); MBA
 * returns -33 for macroblock_escape.  Returns MP2VG_E_BITSTREAM for an invalid code. */
enum {
    MP2VG_VLC_MBA = 0, MP2VG_VLC_MBTYPE_I = 1, MP2VG_VLC_MBTYPE_P = 2, MP2VG_VLC_MBTYPE_B = 3,
    MP2VG_VLC_CBP = 4, MP2VG_VLC_MOTION = 5, MP2VG_VLC_DC_LUMA = 6, MP2VG_VLC_DC_CHROMA = 7,
    MP2VG_VLC_COEF_B14 = 8, MP2VG_VLC_COEF_B15 = 9
};
int  mp2vg_vlc_decode(int32_t table, uint64_t bits, int32_t* value, int32_t* aux, int32_t* consumed);

/* ---- synthetic stream writer (the accepted subset only) --------------------- */
typedef struct mp2vg_gen_params {
    int32_t width, height, chroma_format;
    int32_t n_gops;              /* closed GOPs                                              */
    int32_t gop_n, gop_m;        /* N (pictures per GOP), M (anchor distance); M=1 -> no B  */
    uint32_t seed;
    int32_t frame_pred_frame_dct;/* 1: frame MC/DCT only; 0: field MC + field DCT allowed   */
    int32_t alternate_scan;      /* 0, 1, or -1 = random per picture                        */
    int32_t q_scale_type;        /* 0, 1, or -1 = random per picture                        */
    int32_t intra_dc_precision;  /* 0..3, or -1 = random per picture                        */
    int32_t coefs_min, coefs_max;/* AC coefficients per coded block                         */
    int32_t intra_coefs_min, intra_coefs_max;
    int32_t big_level_permille;  /* probability (per 1000) of a large escape level          */
    int32_t escape_permille;     /* probability of forcing an escape code                   */
    int32_t quant_permille;      /* probability an MB carries a new quantiser_scale         */
    int32_t f_code;              /* motion f_code (1..9)                                     */
    int32_t mix;                 /* 0: SURVEY §8d C2 mix; 1: intra only; 2: MC-heavy         */
    int32_t leading_b;           /* closed GOP starts I + (M-1) backward-only B pictures    */
    int32_t big_matrix_permille; /* probability of a quantiser-matrix entry > 128           */
    int32_t top_field_first;     /* 0, 1, or -1 = random per picture; written as 1 only in
                                    pictures with progressive_frame = 0 (frame_pred_frame_dct = 0) */
    int32_t reserved[4];
} mp2vg_gen_params_t;

void mp2vg_gen_default_params(mp2vg_gen_params_t* p);
int  mp2vg_generate_es(const mp2vg_gen_params_t* p, uint8_t** out, uint64_t* len);
void mp2vg_free(void* ptr);

/* ---- drop-in decoder (reference mp2v_decoder_c) ---------------------------------------- */
typedef struct mp2vg_frame {
    uint8_t* planes[3];       /* host copy (device pointer with MP2VG_DECODER_DEVICE_FRAMES),
                                 valid only during the callback (frame_c rule)               */
    int32_t  width[3], height[3], stride[3];
    int32_t  picture_coding_type;
    int32_t  decode_index;
    int32_t  device;          /* HIP device that decoded the frame (its planes' device with
                                 MP2VG_DECODER_DEVICE_FRAMES)                                 */
} mp2vg_frame_t;
typedef void (*mp2vg_render_fn)(void* user, const mp2vg_frame_t* frame);
typedef struct mp2vg_decoder mp2vg_decoder_t;

int  mp2vg_decoder_create(const mp2vg_config_t* cfg, mp2vg_render_fn fn, void* user,
                          mp2vg_decoder_t** out);
/* The drop-in decoder over several devices (GOP sharding): the independent shards of a stream
 * (mp2vg_parsed_shards) are merged in decode order into runs of at least one decode chunk (16
 * pictures: consecutive shards join a run until it is that long) and the runs are dealt
 * round-robin, run r -> devices[r % ndevices], each device
 * decoding its shards with its own frame pool, record banks and streams, concurrently; frames
 * reach the renderer in the stream's display order whatever device decoded them.  cfg->device is
 * ignored; a device may be listed more than once (e.g. {0, 0}: two independent lanes on one GPU).
 * The reference's picture-parallel runtime this replaces: threads.cpp:22-36, 120-186 and
 * decoder.cpp:299-304, 346-379.  ndevices = 1 is mp2vg_decoder_create on devices[0]. */
int  mp2vg_decoder_create_multi(const mp2vg_config_t* cfg, const int32_t* devices, int32_t ndevices,
                                mp2vg_render_fn fn, void* user, mp2vg_decoder_t** out);
/* decode a whole elementary stream (reference decode(): single-shot, synchronous; frames are
 * delivered in display order to fn on a dedicated render thread before this returns) */
int  mp2vg_decoder_decode(mp2vg_decoder_t* dec, const uint8_t* buf, uint64_t len);
/* sequence headers of the last decoded stream (reference public members, decoder.h:124-130) */
int  mp2vg_decoder_stream_headers(const mp2vg_decoder_t* dec, mp2vg_stream_headers_t* out);
/* frames decoded by each lane of the decoder in its last decode() (lane i = devices[i]); returns
 * the number of lanes */
int  mp2vg_decoder_lane_frames(const mp2vg_decoder_t* dec, int32_t* frames, int32_t n);
/* frame buffers the decoder's frame pools hold (host + device): 2 * 16 + 4 per lane unless a
 * renderer that holds no frame had to wait for display order (then the pool grows) */
int  mp2vg_decoder_frames_allocated(const mp2vg_decoder_t* dec);
/* lane hand-offs in the last decode() (several lanes): in_flight = times the stream moved to
 * another lane while the lane just left was still downloading its last chunk (the host did not
 * wait: both lanes' chunks in flight at once); blocks = times the host waited for another lane's
 * downloads because the frame pool could not give the next chunk its frames otherwise; landed =
 * lane changes where the lane just left had nothing in flight or its downloads were found landed
 * by the non-blocking check; changes = lane changes.  Every change is in_flight, landed or one of
 * the blocks.  Any out pointer may be NULL. */
int  mp2vg_decoder_handoff_stats(const mp2vg_decoder_t* dec, int32_t* in_flight, int32_t* blocks, int32_t* landed,
                                 int32_t* changes);
/* rows replaced in the last decode() (MP2VG_PARSE_CONCEAL; 0 without it) */
int  mp2vg_decoder_damage_count(const mp2vg_decoder_t* dec);
int  mp2vg_decoder_destroy(mp2vg_decoder_t* dec);

#ifdef __cplusplus
}
#endif
#endif /* MP2VG_H */
