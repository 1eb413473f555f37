// Mutation harness for concealment (MP2VG_PARSE_CONCEAL) on the CPU, built with
// -fsanitize=address,undefined by tests/test_conceal_cpu.py.  The mutants of parse_fuzz.cpp's
// mutate() go through the host emitter (mp2vg_parse_es) and through mp2vg_scan_es +
// mp2vg_scan_parse_host, the CPU twin of the kernels, both under the flag.  Every buffer is a heap
// block of exactly its size (the stream, the twin's counted records and words), so a replacement
// row written one record or one word too far aborts the run.  Under the flag both must accept or
// reject a mutant together and give the same records; an accepted batch must pass
// mp2vg_batch_validate with the emitter's picture records (re-typed I pictures included); its
// damage list must be in stream order, name rows inside the picture once each and agree with the
// pictures' MP2VG_PIC_CONCEALED flags; and a mutant the unflagged emitter accepts must come out
// of the flagged one with the same records and no damage.
//   conceal_check <iters> <seed> <stream.m2v> <width> <height> <chroma_format> [...]
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <set>
#include <utility>
#include <vector>

#include "recon_kernel.h"

// runtime.cpp (mp2vg_batch_validate lives there) names its kernel launchers, which are device
// code: never reached here
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
}  // namespace mp2vg

static std::vector<uint8_t> mutate(const std::vector<uint8_t>& in, std::mt19937_64& rng) {
    std::vector<uint8_t> s = in;
    auto pos = [&](size_t n) { return n ? (size_t)(rng() % n) : 0; };
    const int kind = (int)(rng() % 6);
    if (kind == 0) {  // bit flips
        const int n = 1 + (int)(rng() % 8);
        for (int i = 0; i < n && !s.empty(); i++) s[pos(s.size())] ^= (uint8_t)(1u << (rng() % 8));
    } else if (kind == 1) {  // random byte span
        const size_t p = pos(s.size()), n = 1 + rng() % 64;
        for (size_t i = p; i < s.size() && i < p + n; i++) s[i] = (uint8_t)rng();
    } else if (kind == 2) {  // truncation
        s.resize(pos(s.size() + 1));
    } else if (kind == 3) {  // span deletion (a lost packet)
        const size_t p = pos(s.size()), n = 1 + rng() % 256;
        s.erase(s.begin() + p, s.begin() + std::min(s.size(), p + n));
    } else if (kind == 4) {  // span duplication
        const size_t p = pos(s.size()), n = std::min<size_t>(1 + rng() % 512, s.size() - p);
        std::vector<uint8_t> span(s.begin() + p, s.begin() + p + n);
        s.insert(s.begin() + pos(s.size() + 1), span.begin(), span.end());
    } else {  // a start code (random code byte) dropped in
        const uint8_t code[4] = {0, 0, 1, (uint8_t)rng()};
        s.insert(s.begin() + pos(s.size() + 1), code, code + 4);
    }
    return s;
}

static void die(const char* what) {
    fprintf(stderr, "%s: %s\n", what, mp2vg_last_error());
    abort();
}

int main(int argc, char** argv) {
    if (argc < 7 || (argc - 3) % 4) {
        fprintf(stderr, "usage: %s iters seed stream w h cf [...]\n", argv[0]);
        return 2;
    }
    const int iters = atoi(argv[1]);
    std::mt19937_64 rng(strtoull(argv[2], nullptr, 10));
    long clean = 0, concealed = 0, rejected = 0, rows = 0, retyped = 0;
    for (int a = 3; a + 3 < argc; a += 4) {
        FILE* f = fopen(argv[a], "rb");
        if (!f) { perror(argv[a]); return 2; }
        std::vector<uint8_t> es;
        for (int ch; (ch = fgetc(f)) != EOF;) es.push_back((uint8_t)ch);
        fclose(f);
        mp2vg_config_t plain{};
        plain.width = atoi(argv[a + 1]);
        plain.height = atoi(argv[a + 2]);
        plain.chroma_format = atoi(argv[a + 3]);
        plain.num_threads = 1;
        plain.reordering = 1;
        mp2vg_config_t cfg = plain;
        cfg.reserved = MP2VG_PARSE_CONCEAL;
        const int mbh = cfg.height / 16;
        for (int i = -1; i < iters; i++) {  // -1: the stream itself
            const std::vector<uint8_t> v = i < 0 ? es : mutate(es, rng);
            uint8_t* s = (uint8_t*)malloc(v.size() ? v.size() : 1);  // exactly the stream's size
            if (!v.empty()) memcpy(s, v.data(), v.size());
            mp2vg_parsed_t *p0 = nullptr, *p = nullptr;
            const int r0 = mp2vg_parse_es(s, v.size(), &plain, &p0);
            const int r2 = mp2vg_parse_es(s, v.size(), &cfg, &p);
            // the twin under the flag, into blocks of exactly the counted sizes
            mp2vg_scan_t* sc = nullptr;
            int r1 = mp2vg_scan_es(s, v.size(), &cfg, &sc);
            mp2vg_mb_t* mbs = nullptr;
            uint32_t* coefs = nullptr;
            uint64_t nm = 0, nc = 0;
            int32_t npics = 0;
            if (r1 == MP2VG_OK) {
                mp2vg_scan_counts(sc, &npics, nullptr);
                if (npics > 0) {
                    r1 = mp2vg_scan_parse_host(sc, 0, npics, nullptr, 0, nullptr, 0, &nm, &nc);
                    if (r1 == MP2VG_E_STATE) die("twin (count)");
                    if (r1 == MP2VG_OK) {
                        mbs = (mp2vg_mb_t*)malloc(nm * sizeof(mp2vg_mb_t) + !nm);
                        coefs = (uint32_t*)malloc(nc * 4 + !nc);
                        if (mp2vg_scan_parse_host(sc, 0, npics, mbs, nm, nc ? coefs : nullptr, nc, nullptr, nullptr))
                            die("twin (emit) after a clean count");
                    }
                }
            }
            if ((r1 == MP2VG_OK) != (r2 == MP2VG_OK) || (i < 0 && r2 != MP2VG_OK) || (r0 == MP2VG_OK && r2 != MP2VG_OK)) {
                fprintf(stderr, "%s mutant %d: plain %d, flagged emitter %d, flagged twin %d (%s)\n", argv[a], i, r0, r2,
                        r1, mp2vg_last_error());
                return 1;
            }
            if (r2 == MP2VG_OK) {
                int32_t n = 0, nd = 0;
                uint64_t pm = 0, pc = 0;
                mp2vg_parsed_counts(p, &n, &pm, &pc);
                if (n != npics || pm != nm || pc != nc || (nm && memcmp(mbs, mp2vg_parsed_mbs(p), nm * sizeof(mp2vg_mb_t))) ||
                    (nc && memcmp(coefs, mp2vg_parsed_coefs(p), nc * 4))) {
                    fprintf(stderr, "%s mutant %d: the twin's records differ from the host emitter's\n", argv[a], i);
                    return 1;
                }
                if (n > 0 && mp2vg_batch_validate(&plain, n, mp2vg_parsed_pictures(p), n, mp2vg_parsed_mbs(p), pm,
                                                  mp2vg_parsed_coefs(p), pc, nullptr, nullptr, nullptr, 0) != MP2VG_OK) {
                    fprintf(stderr, "%s mutant %d: the concealed batch does not validate: %s\n", argv[a], i, mp2vg_last_error());
                    return 1;
                }
                if (mp2vg_parsed_damage(p, nullptr, 0, &nd) != MP2VG_OK) die("parsed_damage");
                mp2vg_damage_t* dmg = (mp2vg_damage_t*)malloc(nd * sizeof(mp2vg_damage_t) + !nd);  // exactly nd entries
                if (mp2vg_parsed_damage(p, dmg, nd, &nd) != MP2VG_OK) die("parsed_damage");
                std::vector<uint32_t> fl(n > 0 ? n : 1);
                mp2vg_parsed_picture_flags(p, fl.data(), n);
                std::set<std::pair<int, int>> seen;
                std::set<int> hit;
                bool ok = true;
                for (int32_t k = 0; k < nd; k++) {
                    const mp2vg_damage_t& d = dmg[k];
                    ok = ok && d.pic >= 0 && d.pic < n && d.mb_row >= 0 && d.mb_row < mbh && d.status != MP2VG_OK &&
                         mp2vg_damage_reason_string(d.reason)[0] && d.byte_off < v.size() &&
                         seen.insert({d.pic, d.mb_row}).second && (k == 0 || dmg[k - 1].pic <= d.pic);
                    hit.insert(d.pic);
                }
                for (int32_t q = 0; q < n && ok; q++) {
                    ok = ((fl[q] & MP2VG_PIC_CONCEALED) != 0) == (hit.count(q) != 0);
                    if (fl[q] & MP2VG_PIC_RETYPED_I)
                        ok = ok && (fl[q] & MP2VG_PIC_CONCEALED) && mp2vg_parsed_pictures(p)[q].picture_coding_type == 2 &&
                             mp2vg_parsed_pictures(p)[q].fwd_slot >= 0 && ++retyped;
                }
                if (!ok || (r0 == MP2VG_OK && nd)) {
                    fprintf(stderr, "%s mutant %d: bad damage list (%d entries, plain status %d)\n", argv[a], i, nd, r0);
                    return 1;
                }
                if (r0 == MP2VG_OK) {
                    uint64_t m0 = 0, c0 = 0;
                    mp2vg_parsed_counts(p0, nullptr, &m0, &c0);
                    if (m0 != pm || c0 != pc || (pm && memcmp(mp2vg_parsed_mbs(p0), mp2vg_parsed_mbs(p), pm * sizeof(mp2vg_mb_t))) ||
                        (pc && memcmp(mp2vg_parsed_coefs(p0), mp2vg_parsed_coefs(p), pc * 4))) {
                        fprintf(stderr, "%s mutant %d: the flag changed the records of an accepted stream\n", argv[a], i);
                        return 1;
                    }
                }
                free(dmg);
                rows += nd;
                if (i >= 0) (nd ? concealed : clean)++;
            } else if (i >= 0) {
                rejected++;
            }
            mp2vg_parsed_free(p0);
            mp2vg_parsed_free(p);
            mp2vg_scan_free(sc);
            free(mbs);
            free(coefs);
            free(s);
        }
    }
    printf("{\"mutants_clean\": %ld, \"mutants_concealed\": %ld, \"mutants_rejected\": %ld, \"rows_replaced\": %ld, "
           "\"pictures_retyped\": %ld}\n", clean, concealed, rejected, rows, retyped);
    return 0;
}
