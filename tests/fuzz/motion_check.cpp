// Stand-alone check of the motion export's host twin (motion.cpp: mp2vg_motion_records with the
// per-record and per-word rules of motion_kernel.h), built with -fsanitize=address,undefined by
// tests/test_motion_cpu.py together with parse.cpp, tables.cpp and runtime.cpp (the upload
// validation; no device needed).  For each input stream: parse it, export every picture, each
// output alone and subsets in reversed and repeated order, into heap buffers of exactly
// mp2vg_motion_bytes (an access past a tensor aborts the run), and check what the definition
// implies without a second implementation: plane 0 of act sums to ncoef per cell and to the
// stream's word count, info repeats the records, an intra MB has zero vectors.  Then rejected
// calls (bad order, bad n, no output, corrupted records) must leave the destinations untouched.
//   motion_check <stream.m2v> <width> <height> <chroma_format> [...]
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "motion_kernel.h"
#include "recon_kernel.h"
#include "syntax.h"

using namespace mp2vg;

// runtime.cpp's and motion.cpp's kernel launchers live in device code: never reached here
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
hipError_t launch_motion(const MotionArgs&, int, hipStream_t) { return hipErrorInvalidValue; }
}  // namespace mp2vg

static long g_exports = 0, g_rejected = 0;

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
    int nb;
    size_t M;
};

static int run(const Batch& b, const std::vector<int32_t>& order, int32_t n, bool mv, bool info, bool act,
               std::vector<int16_t>* vm, std::vector<uint16_t>* vi, std::vector<int32_t>* va) {
    uint64_t bytes[3] = {0, 0, 0};
    const int32_t sized = n >= 1 && n <= 65535 ? n : 1;
    REQUIRE(mp2vg_motion_bytes(&b.cfg, sized, bytes) == MP2VG_OK);
    vm->assign(bytes[0] / 2, (int16_t)0x5A5A);
    vi->assign(bytes[1] / 2, (uint16_t)0x5A5A);
    va->assign(bytes[2] / 4, (int32_t)0x5A5A5A5A);
    return mp2vg_motion_records(&b.cfg, b.pics.data(), (int32_t)b.pics.size(), b.mbs.data(), b.mbs.size(),
                                b.coefs.data(), b.coefs.size(), order.data(), n, mv ? vm->data() : nullptr,
                                info ? vi->data() : nullptr, act ? va->data() : nullptr);
}

template <class T>
static bool untouched(const std::vector<T>& v, T fill) {
    for (const T& x : v)
        if (x != fill) return false;
    return true;
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
    b.M = (size_t)(w / 16) * (h / 16);

    std::vector<int16_t> vm;
    std::vector<uint16_t> vi;
    std::vector<int32_t> va;
    std::vector<int32_t> all(npics);
    for (int i = 0; i < npics; i++) all[i] = i;
    // everything, in batch order
    REQUIRE(run(b, all, npics, true, true, true, &vm, &vi, &va) == MP2VG_OK);
    g_exports++;
    uint64_t words = 0;
    for (int i = 0; i < npics; i++)
        for (size_t c = 0; c < b.M; c++) {
            const mp2vg_mb_t& m = b.mbs[b.pics[i].mb_first + c];
            const uint16_t* q = vi.data() + (size_t)i * 4 * b.M + c;
            REQUIRE(q[0] == (m.flags & 0x0F1F) && q[b.M] == m.cbp && q[2 * b.M] == m.qscale && q[3 * b.M] == m.ncoef);
            int64_t cnt = 0;
            for (int k = 0; k < b.nb; k++) {
                const int32_t n0 = va[((size_t)i * 2 * b.nb + k) * b.M + c], s1 = va[((size_t)i * 2 * b.nb + b.nb + k) * b.M + c];
                REQUIRE(n0 >= 0 && n0 <= 64 && s1 >= 0);
                REQUIRE((m.cbp >> k & 1) || n0 == 0);
                cnt += n0;
            }
            REQUIRE(cnt == m.ncoef);
            words += (uint64_t)cnt;
            if (m.flags & MP2VG_MB_INTRA)
                for (int k = 0; k < 8; k++) REQUIRE(vm[((size_t)i * 8 + k) * b.M + c] == 0);
            else if (!(m.flags & MP2VG_MB_FIELD_MC) && (m.flags & MP2VG_MB_BWD))
                REQUIRE(vm[((size_t)i * 8 + 4) * b.M + c] == m.mv[0][1][0] && vm[((size_t)i * 8 + 7) * b.M + c] == m.mv[0][1][1]);
        }
    REQUIRE(words == ncoefs);
    const std::vector<int16_t> full_mv = vm;
    const std::vector<int32_t> full_act = va;
    // each output alone: the others stay untouched
    for (int t = 0; t < 3; t++) {
        REQUIRE(run(b, all, npics, t == 0, t == 1, t == 2, &vm, &vi, &va) == MP2VG_OK);
        g_exports++;
        REQUIRE(untouched(vm, (int16_t)0x5A5A) == (t != 0) && untouched(vi, (uint16_t)0x5A5A) == (t != 1) &&
                untouched(va, (int32_t)0x5A5A5A5A) == (t != 2));
    }
    // reversed with a repeat, and a single picture
    std::vector<int32_t> order(all.rbegin(), all.rend());
    order.push_back(order[0]);
    REQUIRE(run(b, order, (int32_t)order.size(), true, true, true, &vm, &vi, &va) == MP2VG_OK);
    g_exports++;
    for (size_t i = 0; i < order.size(); i++) {
        REQUIRE(!memcmp(&vm[i * 8 * b.M], &full_mv[(size_t)order[i] * 8 * b.M], 8 * b.M * 2));
        REQUIRE(!memcmp(&va[i * 2 * b.nb * b.M], &full_act[(size_t)order[i] * 2 * b.nb * b.M], 2 * b.nb * b.M * 4));
    }
    REQUIRE(run(b, {npics - 1}, 1, true, true, true, &vm, &vi, &va) == MP2VG_OK);
    g_exports++;
    // rejections: nothing is written
    auto rejected = [&](const Batch& bb, const std::vector<int32_t>& o, int32_t n, bool any) {
        REQUIRE(run(bb, o, n, any, any, any, &vm, &vi, &va) == MP2VG_E_INVALID);
        REQUIRE(untouched(vm, (int16_t)0x5A5A) && untouched(vi, (uint16_t)0x5A5A) && untouched(va, (int32_t)0x5A5A5A5A));
        g_rejected++;
    };
    rejected(b, {0, npics}, 2, true);
    rejected(b, {-1}, 1, true);
    rejected(b, {0}, 0, true);
    rejected(b, {0}, 65536, true);
    rejected(b, {0}, 1, false);
    {
        Batch c = b;
        c.pics.back().mb_first = (uint32_t)c.mbs.size();
        rejected(c, {0}, 1, true);
    }
    for (size_t k = 0; k < b.mbs.size(); k++)
        if (b.mbs[k].ncoef) {
            Batch c = b;
            c.mbs[k].coef_off = (uint32_t)c.coefs.size();  // words past the batch
            rejected(c, {0}, 1, true);
            c = b;
            c.mbs[k].ncoef += 1;  // the row's words are no longer contiguous (or run past the batch)
            rejected(c, {0}, 1, true);
            break;
        }
}

int main(int argc, char** argv) {
    if (argc < 5 || (argc - 1) % 4) {
        fprintf(stderr, "usage: motion_check <stream.m2v> <width> <height> <chroma_format> [...]\n");
        return 2;
    }
    int streams = 0;
    for (int i = 1; i + 3 < argc; i += 4, streams++) check_stream(argv[i], atoi(argv[i + 1]), atoi(argv[i + 2]), atoi(argv[i + 3]));
    printf("{\"streams\": %d, \"exports\": %ld, \"rejected\": %ld}\n", streams, g_exports, g_rejected);
    return 0;
}
