// Stand-alone check of the residual export's host twin (residual.cpp: mp2vg_residual_records with
// the per-word, per-block and placement rules of residual_kernel.h), built with
// -fsanitize=address,undefined by tests/test_residual_cpu.py together with parse.cpp, tables.cpp
// and runtime.cpp (the upload validation; no device needed).  For each input stream: parse it,
// export every picture at int16 and int8 into heap buffers of exactly mp2vg_residual_bytes between
// guard bytes, and check what the definition implies without a second implementation: the int16
// range, int8 = clamp(int16), zeros where nothing is coded, ZERO_INTRA.  Then seeded mutations of
// the records (word block indices, positions and flag bits, ncoef, cbp, MB flags): the twin either
// refuses the batch and writes nothing, or exports it inside its buffers.
//   residual_check <stream.m2v> <width> <height> <chroma_format> [...]
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "recon_kernel.h"
#include "residual_kernel.h"
#include "syntax.h"

using namespace mp2vg;

// runtime.cpp's and residual.cpp's kernel launchers live in device code: never reached here
namespace mp2vg {
hipError_t launch_recon(int, int, const KArgs&, hipStream_t) { return hipErrorInvalidValue; }
hipError_t launch_tile_convert(const KArgs&, int, const int32_t*, int, int32_t, hipStream_t) { return hipErrorInvalidValue; }
hipError_t launch_digest(const uint64_t*, const int32_t*, int, const uint64_t*, const int32_t*, const int32_t*,
                         const int32_t*, unsigned long long*, hipStream_t) {
    return hipErrorInvalidValue;
}
hipError_t launch_clock_probe(unsigned long long*, int, int, hipStream_t) { return hipErrorInvalidValue; }
hipError_t launch_block_probe(void*, size_t, int, int, void*, hipStream_t) { return hipErrorInvalidValue; }
hipError_t launch_block_random(const void*, size_t, int, int, void*, hipStream_t) { return hipErrorInvalidValue; }
hipError_t launch_pool_scatter(const uint64_t*, int, uint32_t, uint32_t, int, int, int, void*, hipStream_t) {
    return hipErrorInvalidValue;
}
hipError_t launch_residual(const ResidualArgs&, int, hipStream_t) { return hipErrorInvalidValue; }
}  // namespace mp2vg

static long g_exports = 0, g_rejected = 0, g_mutants = 0;
static constexpr size_t kGuard = 64;
static constexpr uint8_t kFill = 0x5A;

#define REQUIRE(cond)                                                       \
    do {                                                                    \
        if (!(cond)) {                                                      \
            fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
            abort();                                                        \
        }                                                                   \
    } while (0)

struct Batch {
    mp2vg_config_t cfg;
    std::vector<mp2vg_picture_t> pics;
    std::vector<mp2vg_mb_t> mbs;
    std::vector<uint32_t> coefs;
    int nb, mbw, mbh;
};

struct Out {
    std::vector<uint8_t> buf[3];  // guard | plane | guard
    uint64_t bytes[3];
    template <class T>
    const T* plane(int k) const { return (const T*)(buf[k].data() + kGuard); }
    bool guards() const {
        for (int k = 0; k < 3; k++)
            for (size_t i = 0; i < kGuard; i++)
                if (buf[k][i] != kFill || buf[k][kGuard + bytes[k] + i] != kFill) return false;
        return true;
    }
    bool untouched() const {
        for (int k = 0; k < 3; k++)
            for (uint8_t x : buf[k])
                if (x != kFill) return false;
        return true;
    }
};

static int run(const Batch& b, const std::vector<int32_t>& order, int32_t n, int dtype, int flags, bool y, bool c,
               Out* o) {
    const int32_t sized = n >= 1 && n <= 65535 ? n : 1;
    REQUIRE(mp2vg_residual_bytes(&b.cfg, sized, dtype == MP2VG_RESIDUAL_I8 ? dtype : MP2VG_RESIDUAL_I16, o->bytes) == MP2VG_OK);
    for (int k = 0; k < 3; k++) o->buf[k].assign(o->bytes[k] + 2 * kGuard, kFill);
    return mp2vg_residual_records(&b.cfg, b.pics.data(), (int32_t)b.pics.size(), b.mbs.data(), b.mbs.size(),
                                  b.coefs.data(), b.coefs.size(), order.data(), n, dtype, flags,
                                  y ? o->buf[0].data() + kGuard : nullptr, c ? o->buf[1].data() + kGuard : nullptr,
                                  c ? o->buf[2].data() + kGuard : nullptr);
}

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) {
    g_rng ^= g_rng << 13, g_rng ^= g_rng >> 7, g_rng ^= g_rng << 17;
    return (uint32_t)((g_rng >> 20) % n);
}

static void check_stream(const char* path, int w, int h, int cf) {
    FILE* f = fopen(path, "rb");
    REQUIRE(f);
    std::vector<uint8_t> es;
    uint8_t buf[65536];
    for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) es.insert(es.end(), buf, buf + k);
    fclose(f);
    Batch b;
    memset(&b.cfg, 0, sizeof b.cfg);
    b.cfg.width = w, b.cfg.height = h, b.cfg.chroma_format = cf, b.cfg.pictures_pool_size = 8, b.cfg.num_threads = 2;
    b.cfg.reordering = 1;
    mp2vg_parsed_t* p = nullptr;
    REQUIRE(mp2vg_parse_es(es.data(), es.size(), &b.cfg, &p) == MP2VG_OK);
    int32_t npics = 0;
    uint64_t nmbs = 0, ncoefs = 0;
    mp2vg_parsed_counts(p, &npics, &nmbs, &ncoefs);
    REQUIRE(npics > 0);
    b.pics.assign(mp2vg_parsed_pictures(p), mp2vg_parsed_pictures(p) + npics);
    b.mbs.assign(mp2vg_parsed_mbs(p), mp2vg_parsed_mbs(p) + nmbs);
    b.coefs.assign(mp2vg_parsed_coefs(p), mp2vg_parsed_coefs(p) + ncoefs);
    mp2vg_parsed_free(p);
    b.nb = cf == 1 ? 6 : (cf == 2 ? 8 : 12);
    b.mbw = w / 16, b.mbh = h / 16;

    std::vector<int32_t> all(npics);
    for (int i = 0; i < npics; i++) all[i] = i;
    Out o16, o8, oz;
    REQUIRE(run(b, all, npics, MP2VG_RESIDUAL_I16, 0, true, true, &o16) == MP2VG_OK && o16.guards());
    REQUIRE(run(b, all, npics, MP2VG_RESIDUAL_I8, 0, true, true, &o8) == MP2VG_OK && o8.guards());
    REQUIRE(run(b, all, npics, MP2VG_RESIDUAL_I16, MP2VG_RESIDUAL_ZERO_INTRA, true, true, &oz) == MP2VG_OK && oz.guards());
    g_exports += 3;
    for (int k = 0; k < 3; k++) {
        REQUIRE(o16.bytes[k] == 2 * o8.bytes[k]);
        const int16_t *a = o16.plane<int16_t>(k), *z = oz.plane<int16_t>(k);
        const int8_t* c = o8.plane<int8_t>(k);
        for (size_t i = 0; i < o8.bytes[k]; i++) {
            REQUIRE(a[i] >= -255 && a[i] <= 255);
            REQUIRE(c[i] == (a[i] < -128 ? -128 : (a[i] > 127 ? 127 : a[i])));
            REQUIRE(z[i] == 0 || z[i] == a[i]);
        }
    }
    // luma of MBs with nothing coded is zero; luma of intra MBs is zero under ZERO_INTRA
    const size_t W = (size_t)w, H = (size_t)h;
    for (int i = 0; i < npics; i++)
        for (int my = 0; my < b.mbh; my++)
            for (int mx = 0; mx < b.mbw; mx++) {
                const mp2vg_mb_t& m = b.mbs[b.pics[i].mb_first + (size_t)my * b.mbw + mx];
                const bool intra = m.flags & MP2VG_MB_INTRA;
                if ((m.cbp & 15) && !intra) continue;
                const int16_t* src = (intra ? oz : o16).plane<int16_t>(0);
                for (int y = 0; y < 16; y++)
                    for (int x = 0; x < 16; x++) REQUIRE(src[((size_t)i * H + my * 16 + y) * W + mx * 16 + x] == 0);
            }
    // each output alone, a reversed order with a repeat
    Out o;
    REQUIRE(run(b, all, npics, MP2VG_RESIDUAL_I16, 0, true, false, &o) == MP2VG_OK && o.guards());
    REQUIRE(o.buf[0] == o16.buf[0] && o.buf[1] == std::vector<uint8_t>(o.buf[1].size(), kFill));
    REQUIRE(run(b, all, npics, MP2VG_RESIDUAL_I16, 0, false, true, &o) == MP2VG_OK && o.guards());
    REQUIRE(o.buf[1] == o16.buf[1] && o.buf[2] == o16.buf[2] && o.buf[0] == std::vector<uint8_t>(o.buf[0].size(), kFill));
    std::vector<int32_t> order(all.rbegin(), all.rend());
    order.push_back(order[0]);
    REQUIRE(run(b, order, (int32_t)order.size(), MP2VG_RESIDUAL_I8, 0, true, true, &o) == MP2VG_OK && o.guards());
    g_exports += 3;
    for (size_t i = 0; i < order.size(); i++)
        for (int k = 0; k < 3; k++) {
            const size_t per = o8.bytes[k] / npics;
            REQUIRE(!memcmp(o.plane<int8_t>(k) + i * per, o8.plane<int8_t>(k) + (size_t)order[i] * per, per));
        }
    // rejected arguments: nothing is written
    auto rejected = [&](const Batch& bb, const std::vector<int32_t>& od, int32_t n, int dtype, int flags, bool y, bool c) {
        REQUIRE(run(bb, od, n, dtype, flags, y, c, &o) == MP2VG_E_INVALID);
        REQUIRE(o.untouched());
        g_rejected++;
    };
    rejected(b, {0, npics}, 2, 0, 0, true, true);
    rejected(b, {-1}, 1, 0, 0, true, true);
    rejected(b, {0}, 0, 0, 0, true, true);
    rejected(b, {0}, 65536, 0, 0, true, true);
    rejected(b, {0}, 1, 0, 0, false, false);
    rejected(b, {0}, 1, 2, 0, true, true);
    rejected(b, {0}, 1, 0, 2, true, true);
    // seeded mutations: refused with nothing written, or exported inside the buffers
    for (int it = 0; it < 48; it++) {
        Batch c = b;
        const int kind = it % 6;
        for (int k = 0; k < 8; k++) {
            const size_t mi = rnd((uint32_t)c.mbs.size());
            mp2vg_mb_t& m = c.mbs[mi];
            if (kind == 0 && !c.coefs.empty()) {  // a word's block index (any of the 16 codes)
                uint32_t& wd = c.coefs[rnd((uint32_t)c.coefs.size())];
                wd = (wd & ~(15u << 22)) | (rnd(16) << 22);
            } else if (kind == 1 && !c.coefs.empty()) {  // a word's position, level and flag bits
                uint32_t& wd = c.coefs[rnd((uint32_t)c.coefs.size())];
                wd = (wd & ~((63u << 16) | 0xffffu)) | (rnd(64) << 16) | rnd(65536);
                if (rnd(4) == 0) wd ^= rnd(2) ? MP2VG_COEF_DC : MP2VG_COEF_FIRST1S;
            } else if (kind == 2) {
                m.ncoef = (uint16_t)(rnd(3) ? 0 : m.ncoef + 1);
            } else if (kind == 3) {
                m.cbp = (uint16_t)rnd(1u << 12);
            } else if (kind == 4) {
                m.flags ^= (uint16_t)(1u << rnd(12));
            } else {
                m.qscale = (uint8_t)rnd(256);
                if (m.ncoef) m.coef_off += rnd(3) - 1;
            }
        }
        const int dtype = it & 1, flags = (it >> 1) & 1;
        const int rc = run(c, all, npics, dtype, flags, true, true, &o);
        REQUIRE(rc == MP2VG_OK || rc == MP2VG_E_INVALID);
        REQUIRE(rc == MP2VG_OK ? o.guards() : o.untouched());
        (rc == MP2VG_OK ? g_mutants : g_rejected)++;
    }
}

int main(int argc, char** argv) {
    if (argc < 5 || (argc - 1) % 4) {
        fprintf(stderr, "usage: residual_check <stream.m2v> <width> <height> <chroma_format> [...]\n");
        return 2;
    }
    int streams = 0;
    for (int i = 1; i + 3 < argc; i += 4, streams++) check_stream(argv[i], atoi(argv[i + 1]), atoi(argv[i + 2]), atoi(argv[i + 3]));
    printf("{\"streams\": %d, \"exports\": %ld, \"rejected\": %ld, \"mutants\": %ld}\n", streams, g_exports, g_rejected,
           g_mutants);
    return 0;
}
