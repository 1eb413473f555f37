// parse_dev.cpp — host entry points of the device parse that enqueue its kernels (parse.hip):
// mp2vg_batch_upload_es and mp2vg_last_parse_times.  The scan and the CPU twin are host-only
// (parse.cpp); the context's side (banks, planning, making the batch resident) is runtime.cpp's,
// which so still links without kernels.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "hipchk.h"
#include "parse_kernel.h"
#include "scan.h"
#include "syntax.h"

using namespace mp2vg;

namespace {

// per context, created at its first mp2vg_batch_upload_es.  One set of buffers: the call is
// synchronous (it returns after the emit pass), so nothing of the previous call is in flight.
struct EsState {
    int device = 0;
    uint32_t* d_tables = nullptr;
    SpTables T{};
    uint8_t* d_bs = nullptr;
    size_t cap_bs = 0;
    uint8_t* d_small = nullptr;  // slice table | picture headers | mb_first | pic_slice
    size_t cap_small = 0;
    SpResult* d_res = nullptr;
    uint32_t* d_base = nullptr;
    size_t cap_slices = 0;
    uint32_t* d_uses = nullptr;
    size_t cap_pics = 0;
    unsigned long long* d_summary = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    float ms[3] = {0, 0, 0};
    bool timed = false;
    // host sides of the copies (kept here so that they outlive every copy in flight)
    std::vector<uint8_t> h_small;
    std::vector<uint32_t> h_uses;
    unsigned long long h_summary[3] = {0, 0, 0};
    SpResult h_res{};
    // MP2VG_PARSE_CONCEAL: the per-slice results (read back only when the scan kernel counted
    // damage) and the rows the last upload replaced (mp2vg_last_upload_damage)
    std::vector<SpResult> h_all;
    std::vector<mp2vg_damage_t> damage;
};

void es_state_free(void* p) {
    EsState* s = (EsState*)p;
    (void)hipSetDevice(s->device);
    void* const blocks[] = {s->d_tables, s->d_bs, s->d_small, s->d_res, s->d_base, s->d_uses, s->d_summary};
    for (void* b : blocks) (void)hipFree(b);
    for (hipEvent_t e : s->ev)
        if (e) (void)hipEventDestroy(e);
    delete s;
}

template <class T>
int grow_dev(T*& p, size_t& cap, size_t n) {
    if (n <= cap) return MP2VG_OK;
    if (p) HIPCHK(hipFree(p));
    p = nullptr;
    cap = 0;
    const size_t c = n + n / 2;
    HIPCHK(hipMalloc((void**)&p, c * sizeof(T)));
    cap = c;
    return MP2VG_OK;
}

// whatever path leaves the call, no copy from the caller's stream or from the state is in flight
struct SyncOnExit {
    hipStream_t st;
    ~SyncOnExit() { (void)hipStreamSynchronize(st); }
};

int upload_es(mp2vg_ctx_t* c, const mp2vg_scan* scan, const mp2vg_picture_t* pics, int32_t first, int32_t npics) {
    const SpGeom& g = scan->g;
    const uint64_t per_pic = (uint64_t)g.mbw * g.mbh;
    const uint64_t nmbs = per_pic * (uint64_t)npics;
    if (nmbs + 64 >= (1ull << 32)) {
        set_error("batch too large");
        return MP2VG_E_INVALID;
    }
    std::vector<mp2vg_picture_t> own;
    if (!pics) {
        own.assign(scan->pics.begin() + first, scan->pics.begin() + first + npics);
        for (int32_t i = 0; i < npics; i++) own[i].mb_first = (uint32_t)(per_pic * i);
        pics = own.data();
    }
    EsBank bank;
    if (int rc = es_begin(c, pics, npics, nmbs, &bank)) return rc;
    if (!*bank.state) {
        EsState* ns = new EsState();
        ns->device = bank.device;
        *bank.state = ns;
        *bank.state_free = es_state_free;
    }
    EsState& S = *(EsState*)*bank.state;
    const hipStream_t st = bank.stream;
    SyncOnExit sync{st};
    if (!S.d_tables) {
        const uint32_t* w;
        size_t nw;
        sp_tables(&w, &nw, &S.T);
        HIPCHK(hipMalloc((void**)&S.d_tables, nw * sizeof(uint32_t)));
        HIPCHK(hipMemcpy(S.d_tables, w, nw * sizeof(uint32_t), hipMemcpyHostToDevice));
        S.T.w = S.d_tables;
        HIPCHK(hipMalloc((void**)&S.d_summary, 3 * sizeof(unsigned long long)));
        for (hipEvent_t& e : S.ev) HIPCHK(hipEventCreate(&e));
    }
    S.timed = false;
    S.damage.clear();
    const bool conceal = (scan->cfg.reserved & MP2VG_PARSE_CONCEAL) != 0;

    // the range's bitstream, with kSpanPad zero bytes after it; offsets rebased to the span
    uint64_t lo, hi;
    scan_span(scan, first, npics, &lo, &hi);
    const uint64_t span = hi - lo;
    if (span + kSpanPad >= (1ull << 32)) {
        set_error("bitstream range of 4 GB or more: split it");
        return MP2VG_E_INVALID;
    }
    if (int rc = grow_dev(S.d_bs, S.cap_bs, (size_t)(span + kSpanPad))) return rc;
    HIPCHK(hipMemcpyAsync(S.d_bs, scan->buf + lo, span, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(S.d_bs + span, 0, kSpanPad, st));

    const uint32_t j0 = scan->pic_slice[first], j1 = scan->pic_slice[first + npics];
    const uint32_t ns = j1 - j0;
    const size_t o_sl = 0, o_hdr = o_sl + sizeof(DevSlice) * ns, o_mbf = o_hdr + sizeof(SpPicHdr) * npics,
                 o_ps = o_mbf + sizeof(uint32_t) * npics, small = o_ps + sizeof(uint32_t) * (npics + 1);
    S.h_small.resize(small);
    {
        DevSlice* sl = (DevSlice*)(S.h_small.data() + o_sl);
        for (uint32_t j = j0; j < j1; j++) {
            const SpSlice& s = scan->slices[j];
            // (a missing row's empty entry sits at its picture's start code, in front of the span)
            const bool empty = s.byte_off == s.byte_end;
            sl[j - j0] = {(uint32_t)(s.pic - first), (uint32_t)s.mb_row, empty ? 0u : (uint32_t)(s.byte_off - lo),
                          empty ? 0u : (uint32_t)(s.byte_end - lo)};
        }
        memcpy(S.h_small.data() + o_hdr, scan->hdr.data() + first, sizeof(SpPicHdr) * npics);
        uint32_t* mbf = (uint32_t*)(S.h_small.data() + o_mbf);
        uint32_t* ps = (uint32_t*)(S.h_small.data() + o_ps);
        for (int32_t i = 0; i < npics; i++) mbf[i] = pics[i].mb_first;
        for (int32_t i = 0; i <= npics; i++) ps[i] = scan->pic_slice[first + i] - j0;
    }
    if (int rc = grow_dev(S.d_small, S.cap_small, small)) return rc;
    if (int rc = grow_dev(S.d_uses, S.cap_pics, (size_t)npics)) return rc;
    if (ns + 1 > S.cap_slices) {
        size_t cap_res = S.cap_slices, cap_base = S.cap_slices;
        if (int rc = grow_dev(S.d_res, cap_res, (size_t)ns + 1)) return rc;
        if (int rc = grow_dev(S.d_base, cap_base, (size_t)ns + 1)) return rc;
        S.cap_slices = cap_res;
    }
    HIPCHK(hipMemcpyAsync(S.d_small, S.h_small.data(), small, hipMemcpyHostToDevice, st));

    ParseArgs a;
    memset(&a, 0, sizeof a);
    a.T = S.T;
    a.G = g;
    a.slices = (const DevSlice*)(S.d_small + o_sl);
    a.hdr = (const SpPicHdr*)(S.d_small + o_hdr);
    a.mb_first = (const uint32_t*)(S.d_small + o_mbf);
    a.nslices = ns;
    a.bs = S.d_bs;
    a.span = (uint32_t)span;
    a.mbs = bank.d_mbs;
    a.res = S.d_res;
    a.base = S.d_base;
    a.uses = S.d_uses;
    a.npics = (uint32_t)npics;
    a.conceal = conceal;
    a.rows = (scan->cfg.reserved & MP2VG_PARSE_SLICES) != 0;
    HIPCHK(hipEventRecord(S.ev[0], st));
    HIPCHK(launch_parse_count(a, st));
    HIPCHK(launch_parse_rows(a, st));     // (MP2VG_PARSE_SLICES only; counted with the count pass too)
    HIPCHK(launch_parse_conceal(a, st));  // (counted with the count pass in mp2vg_last_parse_times)
    HIPCHK(hipEventRecord(S.ev[1], st));
    HIPCHK(launch_parse_scan(a, (const uint32_t*)(S.d_small + o_ps), S.d_summary, st));
    HIPCHK(hipEventRecord(S.ev[2], st));
    // a few bytes per picture come back: the total, the first failing slice, the usage bits
    S.h_uses.resize(npics);
    HIPCHK(hipMemcpyAsync(S.h_summary, S.d_summary, sizeof S.h_summary, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(S.h_uses.data(), S.d_uses, sizeof(uint32_t) * npics, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (S.h_summary[1] != ~0ull) {  // the first failing slice in stream order
        const uint32_t j = (uint32_t)S.h_summary[1];
        HIPCHK(hipMemcpy(&S.h_res, S.d_res + j, sizeof(SpResult), hipMemcpyDeviceToHost));
        const SpSlice& s = scan->slices[j0 + j];
        sp_set_slice_error(s.pic, s.byte_off, S.h_res.reason);
        return S.h_res.status != MP2VG_OK ? S.h_res.status : MP2VG_E_INVALID;
    }
    const uint64_t total = S.h_summary[0];
    // damage: the slices' results come back, damaged I pictures with a conceal reference are re-typed
    // in this call's copy of the picture records (the copy es_commit makes resident), and the list
    // is kept for mp2vg_last_upload_damage.  A clean upload copies nothing more.
    std::vector<mp2vg_picture_t> retyped;
    if (conceal && S.h_summary[2]) {
        S.h_all.resize(ns);
        HIPCHK(hipMemcpy(S.h_all.data(), S.d_res, sizeof(SpResult) * ns, hipMemcpyDeviceToHost));
        retyped.assign(pics, pics + npics);
        for (uint32_t j = 0; j < ns; j++) {
            const SpResult& r = S.h_all[j];
            if (r.status == MP2VG_OK) continue;
            const SpSlice& s = scan->slices[j0 + j];
            // (MP2VG_PARSE_SLICES: the row's first entry carries the damage, the blamed one names the offset)
            const uint32_t jb = j + r.blame < ns ? j + r.blame : j;
            S.damage.push_back({s.pic - first, s.mb_row, r.status, r.reason, scan->slices[j0 + jb].byte_off});
        }
        for (int32_t i = 0; i < npics; i++)  // (bit 2 of the scan kernel's per-picture word: a concealed row)
            if ((S.h_uses[i] & 4) && retyped[i].picture_coding_type == 1 && scan->hdr[first + i].has_conceal_ref)
                retyped[i].picture_coding_type = 2;
        pics = retyped.data();
    }
    uint32_t* d_coefs = nullptr;
    if (int rc = es_coefs(c, total, &d_coefs)) return rc;
    a.coefs = d_coefs;
    HIPCHK(launch_parse_emit(a, st));
    HIPCHK(hipEventRecord(S.ev[3], st));
    std::vector<uint8_t> uses_of(2 * (size_t)npics);
    for (int32_t i = 0; i < npics; i++) {
        uses_of[2 * (size_t)i] = S.h_uses[i] & 1;
        uses_of[2 * (size_t)i + 1] = (S.h_uses[i] >> 1) & 1;
    }
    if (int rc = es_commit(c, pics, npics, nmbs, total, uses_of.data())) return rc;
    for (int i = 0; i < 3; i++) HIPCHK(hipEventElapsedTime(&S.ms[i], S.ev[i], S.ev[i + 1]));
    S.timed = true;
    return MP2VG_OK;
}

}  // namespace

extern "C" int mp2vg_batch_upload_es(mp2vg_ctx_t* c, const mp2vg_scan_t* scan, const mp2vg_picture_t* pics,
                                     int32_t first, int32_t npics) {
    if (!c || !scan || first < 0 || npics <= 0 || (uint64_t)first + (uint64_t)npics > scan->pics.size())
        return MP2VG_E_INVALID;
    const mp2vg_config_t* cfg = ctx_config(c);
    if (cfg->width != scan->cfg.width || cfg->height != scan->cfg.height ||
        cfg->chroma_format != scan->cfg.chroma_format) {
        set_error("the scan's geometry differs from the context's");
        return MP2VG_E_INVALID;
    }
    return upload_es(c, scan, pics, first, npics);
}

extern "C" int mp2vg_last_upload_damage(mp2vg_ctx_t* c, mp2vg_damage_t* out, int32_t max, int32_t* n) {
    if (!c || !n || max < 0 || (max && !out)) return MP2VG_E_INVALID;
    const EsState* s = (const EsState*)ctx_es_state(c);
    *n = s ? (int32_t)s->damage.size() : 0;
    for (int32_t i = 0; i < *n && i < max; i++) out[i] = s->damage[i];
    return MP2VG_OK;
}

extern "C" int mp2vg_last_parse_times(mp2vg_ctx_t* c, float ms[3]) {
    if (!c || !ms) return MP2VG_E_INVALID;
    const EsState* s = (const EsState*)ctx_es_state(c);
    if (!s || !s->timed) {
        set_error("no device parse has run on this context");
        return MP2VG_E_STATE;
    }
    for (int i = 0; i < 3; i++) ms[i] = s->ms[i];
    return MP2VG_OK;
}
