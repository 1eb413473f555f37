// Mutation harness for the device slice parser's source (csrc/slice_parse.h) on the CPU, built
// with -fsanitize=address,undefined by tests/test_device_parse_sanitize.py.  The mutants of
// parse_fuzz.cpp's mutate() go through mp2vg_scan_es and mp2vg_scan_parse_host, the CPU twin of
// the kernels: the twin copies the bitstream into a heap block of exactly the device's size
// (span + 16 zero bytes), and the records and coefficient words go into heap blocks of exactly
// the counted sizes, so one byte read or written too far aborts the run.  The twin itself checks
// the iteration bound of every slice (sp_iter_bound) and that the emit pass repeats the count
// pass; either failing (MP2VG_E_STATE) aborts too.  A mutant both parsers accept must give the
// same records, and both must accept or reject it together.
//   device_parse_fuzz <iters> <seed> <stream.m2v> <width> <height> <chroma_format> [...]
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "syntax.h"

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
    } else if (kind == 3) {  // span deletion
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

// scan + twin over the whole stream, and over a random sub-range when it has several pictures;
// returns the status (MP2VG_OK: *mbs / *coefs hold the whole stream's records)
static int twin(const std::vector<uint8_t>& in, const mp2vg_config_t& cfg, std::mt19937_64& rng,
                std::vector<mp2vg_mb_t>* mbs_out, std::vector<uint32_t>* coefs_out) {
    // the stream in a heap block of exactly its size: the scan may not read past it either
    uint8_t* es = (uint8_t*)malloc(in.size() ? in.size() : 1);
    if (!in.empty()) memcpy(es, in.data(), in.size());
    mp2vg_scan_t* sc = nullptr;
    int rc = mp2vg_scan_es(es, in.size(), &cfg, &sc);
    if (rc == MP2VG_OK) {
        int32_t npics = 0;
        uint64_t nslices = 0;
        mp2vg_scan_counts(sc, &npics, &nslices);
        std::vector<int32_t> v(npics > 0 ? npics : 1);
        mp2vg_scan_display_order(sc, v.data(), npics);
        mp2vg_scan_gop_index(sc, v.data(), npics);
        mp2vg_scan_shards(sc, v.data(), npics);
        mp2vg_stream_headers_t h;
        mp2vg_scan_stream_headers(sc, &h);
        for (int pass = 0; pass < 2 && npics > 0; pass++) {
            int32_t first = 0, n = npics;
            if (pass == 1) {
                if (npics < 2) break;
                first = (int32_t)(rng() % npics);
                n = 1 + (int32_t)(rng() % (npics - first));
            }
            uint64_t nm = 0, nc = 0;
            int r = mp2vg_scan_parse_host(sc, first, n, nullptr, 0, nullptr, 0, &nm, &nc);
            if (r == MP2VG_E_STATE) die("twin (count)");
            if (r == MP2VG_OK) {
                mp2vg_mb_t* mbs = (mp2vg_mb_t*)malloc(nm * sizeof(mp2vg_mb_t) + !nm);
                uint32_t* coefs = (uint32_t*)malloc(nc * 4 + !nc);
                r = mp2vg_scan_parse_host(sc, first, n, mbs, nm, nc ? coefs : nullptr, nc, nullptr, nullptr);
                if (r != MP2VG_OK) die("twin (emit) after a clean count");
                if (pass == 0) {
                    mbs_out->assign(mbs, mbs + nm);
                    coefs_out->assign(coefs, coefs + nc);
                }
                free(mbs);
                free(coefs);
            }
            if (pass == 0) rc = r;
        }
        mp2vg_scan_free(sc);
    }
    free(es);
    return rc;
}

int main(int argc, char** argv) {
    if (argc < 7 || (argc - 3) % 4) {
        fprintf(stderr, "usage: %s iters seed stream w h cf [...]\n", argv[0]);
        return 2;
    }
    const int iters = atoi(argv[1]);
    std::mt19937_64 rng(strtoull(argv[2], nullptr, 10));
    long ok = 0, rejected = 0;
    for (int a = 3; a + 3 < argc; a += 4) {
        FILE* f = fopen(argv[a], "rb");
        if (!f) { perror(argv[a]); return 2; }
        std::vector<uint8_t> es;
        for (int ch; (ch = fgetc(f)) != EOF;) es.push_back((uint8_t)ch);
        fclose(f);
        mp2vg_config_t cfg{};
        cfg.width = atoi(argv[a + 1]);
        cfg.height = atoi(argv[a + 2]);
        cfg.chroma_format = atoi(argv[a + 3]);
        cfg.num_threads = 1;
        cfg.reordering = 1;
        for (int i = -1; i < iters; i++) {  // -1: the stream itself
            const std::vector<uint8_t> s = i < 0 ? es : mutate(es, rng);
            std::vector<mp2vg_mb_t> mbs;
            std::vector<uint32_t> coefs;
            const int r1 = twin(s, cfg, rng, &mbs, &coefs);
            mp2vg_parsed_t* p = nullptr;
            const int r2 = mp2vg_parse_es(s.data(), s.size(), &cfg, &p);
            if ((r1 == MP2VG_OK) != (r2 == MP2VG_OK) || (i < 0 && r1 != MP2VG_OK)) {
                fprintf(stderr, "%s mutant %d: twin %d, host emitter %d (%s)\n", argv[a], i, r1, r2, mp2vg_last_error());
                return 1;
            }
            if (r2 == MP2VG_OK) {
                int32_t n = 0;
                uint64_t nm = 0, nc = 0;
                mp2vg_parsed_counts(p, &n, &nm, &nc);
                if (nm != mbs.size() || nc != coefs.size() ||
                    (nm && memcmp(mbs.data(), mp2vg_parsed_mbs(p), nm * sizeof(mp2vg_mb_t))) ||
                    (nc && memcmp(coefs.data(), mp2vg_parsed_coefs(p), nc * 4))) {
                    fprintf(stderr, "%s mutant %d: the twin's records differ from the host emitter's\n", argv[a], i);
                    return 1;
                }
                mp2vg_parsed_free(p);
            }
            if (i >= 0) (r1 == MP2VG_OK ? ok : rejected)++;
        }
    }
    printf("{\"mutants_parsed\": %ld, \"mutants_rejected\": %ld}\n", ok, rejected);
    return 0;
}
