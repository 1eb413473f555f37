// Mutation harness for MP2VG_PARSE_SLICES on the CPU, built with -fsanitize=address,undefined by
// tests/test_slices_cpu.py together with parse.cpp and tables.cpp.  The multi-slice fixtures
// (tests/golden/slices/*.m2v) and seeded byte mutants of them go through the host emitter
// (mp2vg_parse_es) and through mp2vg_scan_es + mp2vg_scan_parse_host, the CPU twin of the kernels
// (which asserts sp_iter_bound for every slice: MP2VG_E_STATE aborts the run), under the flag alone
// and together with MP2VG_PARSE_CONCEAL.  Every buffer is a heap block of exactly its size (the
// stream, the twin's counted records and words), so a byte read or written too far aborts the run.
// The emitter and the twin must agree on the status, on the reason and the blamed slice (the whole
// message) and, where they accept, on every byte of the records, the words and the picture records.
// One difference of order is let through: the scan makes its row rejections (a row outside the
// picture, a slice that comes back to a row, a row no slice covers) for the whole stream before the
// twin parses a slice, so where the scan itself refuses, the emitter may blame a damaged slice of an
// earlier picture instead; both must still refuse.
//   slices_check <iters> <seed> <stream.m2v> <width> <height> <chroma_format> [...]
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "scan.h"
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

int main(int argc, char** argv) {
    if (argc < 7 || (argc - 3) % 4) {
        fprintf(stderr, "usage: %s iters seed stream w h cf [...]\n", argv[0]);
        return 2;
    }
    const int iters = atoi(argv[1]);
    std::mt19937_64 rng(strtoull(argv[2], nullptr, 10));
    long streams = 0, accepted = 0, rejected = 0, concealed = 0, scan_first = 0, cover = 0;
    for (int a = 3; a + 3 < argc; a += 4) {
        FILE* f = fopen(argv[a], "rb");
        if (!f) { perror(argv[a]); return 2; }
        std::vector<uint8_t> es;
        for (int ch; (ch = fgetc(f)) != EOF;) es.push_back((uint8_t)ch);
        fclose(f);
        streams++;
        mp2vg_config_t base{};
        base.width = atoi(argv[a + 1]);
        base.height = atoi(argv[a + 2]);
        base.chroma_format = atoi(argv[a + 3]);
        base.num_threads = 1;
        base.reordering = 1;
        for (int i = -1; i < iters; i++) {  // -1: the stream itself
            const std::vector<uint8_t> v = i < 0 ? es : mutate(es, rng);
            uint8_t* s = (uint8_t*)malloc(v.size() ? v.size() : 1);  // exactly the stream's size
            if (!v.empty()) memcpy(s, v.data(), v.size());
            for (int flags : {MP2VG_PARSE_SLICES, MP2VG_PARSE_SLICES | MP2VG_PARSE_CONCEAL}) {
                mp2vg_config_t cfg = base;
                cfg.reserved = flags;
                mp2vg_parsed_t* p = nullptr;
                const int re = mp2vg_parse_es(s, v.size(), &cfg, &p);
                const std::string me = re == MP2VG_OK ? "" : mp2vg_last_error();
                mp2vg_scan_t* sc = nullptr;
                const int rs = mp2vg_scan_es(s, v.size(), &cfg, &sc);
                int rt = rs;
                mp2vg_mb_t* mbs = nullptr;
                uint32_t* coefs = nullptr;
                uint64_t nm = 0, nc = 0;
                int32_t npics = 0;
                if (rs == MP2VG_OK) {
                    mp2vg_scan_counts(sc, &npics, nullptr);
                    if (npics > 0) {
                        rt = mp2vg_scan_parse_host(sc, 0, npics, nullptr, 0, nullptr, 0, &nm, &nc);
                        if (rt == MP2VG_E_STATE) die("twin (count)");
                        if (rt == MP2VG_OK) {
                            mbs = (mp2vg_mb_t*)malloc(nm * sizeof(mp2vg_mb_t) + !nm);
                            coefs = (uint32_t*)malloc(nc * 4 + !nc);
                            if (mp2vg_scan_parse_host(sc, 0, npics, mbs, nm, nc ? coefs : nullptr, nc, nullptr, nullptr))
                                die("twin (emit) after a clean count");
                        }
                    }
                }
                const std::string mt = rt == MP2VG_OK ? "" : mp2vg_last_error();
                // a negative fixture is refused; under CONCEAL its row is replaced, but for the slice that
                // comes back to a row, which stays refused
                const bool is_neg = strstr(argv[a], "neg_") != nullptr &&
                                    (!(flags & MP2VG_PARSE_CONCEAL) || strstr(argv[a], "neg_repeat") != nullptr);
                bool bad = (re == MP2VG_OK) != (rt == MP2VG_OK) || (i < 0 && (re == MP2VG_OK) == is_neg);
                if (mt.find(mp2vg::sp_reason_text(mp2vg::SP_R_ROW_GAP)) != std::string::npos ||
                    mt.find(mp2vg::sp_reason_text(mp2vg::SP_R_ROW_OVERLAP)) != std::string::npos)
                    cover++;
                if (!bad && re != MP2VG_OK) {
                    const bool row_reason = mt.find(mp2vg::sp_reason_text(mp2vg::SP_R_ROW_OUTSIDE)) != std::string::npos ||
                                            mt.find(mp2vg::sp_reason_text(mp2vg::SP_R_TWO_SLICES)) != std::string::npos ||
                                            mt.find(mp2vg::sp_reason_text(mp2vg::SP_R_ROW_UNCOVERED)) != std::string::npos;
                    if (rs != MP2VG_OK && row_reason && (re != rt || me != mt))
                        scan_first++;  // the scan refused first (see above): both refuse, that is all
                    else
                        bad = re != rt || me != mt;
                }
                if (bad) {
                    fprintf(stderr, "%s mutant %d flags %d: emitter %d (%s), scan %d, twin %d (%s)\n", argv[a], i, flags, re,
                            me.c_str(), rs, rt, mt.c_str());
                    return 1;
                }
                if (re == MP2VG_OK) {
                    int32_t n = 0, nd = 0;
                    uint64_t pm = 0, pc = 0;
                    mp2vg_parsed_counts(p, &n, &pm, &pc);
                    if (n != npics || pm != nm || pc != nc || (nm && memcmp(mbs, mp2vg_parsed_mbs(p), nm * sizeof(mp2vg_mb_t))) ||
                        (nc && memcmp(coefs, mp2vg_parsed_coefs(p), nc * 4))) {
                        fprintf(stderr, "%s mutant %d flags %d: the twin's records differ from the host emitter's\n", argv[a], i,
                                flags);
                        return 1;
                    }
                    // the scan's picture records are the emitter's (W among them) before any re-typing
                    std::vector<uint32_t> fl(n > 0 ? n : 1);
                    mp2vg_parsed_picture_flags(p, fl.data(), n);
                    for (int32_t q = 0; q < n; q++) {
                        mp2vg_picture_t e = mp2vg_parsed_pictures(p)[q];
                        if (fl[q] & MP2VG_PIC_RETYPED_I) e.picture_coding_type = 1;
                        if (memcmp(&e, &mp2vg_scan_pictures(sc)[q], sizeof e)) {
                            fprintf(stderr, "%s mutant %d flags %d: picture record %d differs\n", argv[a], i, flags, q);
                            return 1;
                        }
                    }
                    mp2vg_parsed_damage(p, nullptr, 0, &nd);
                    std::vector<mp2vg_damage_t> dmg(nd > 0 ? nd : 1);
                    mp2vg_parsed_damage(p, dmg.data(), nd, &nd);
                    for (int32_t q = 0; q < nd; q++)
                        cover += dmg[q].reason == mp2vg::SP_R_ROW_GAP || dmg[q].reason == mp2vg::SP_R_ROW_OVERLAP;
                    if (i >= 0) (nd ? concealed : accepted)++;
                } else if (i >= 0) {
                    rejected++;
                }
                mp2vg_parsed_free(p);
                mp2vg_scan_free(sc);
                free(mbs);
                free(coefs);
            }
            free(s);
        }
    }
    printf("{\"streams\": %ld, \"accepted\": %ld, \"rejected\": %ld, \"concealed\": %ld, \"scan_refused_first\": %ld, "
           "\"cover_failures\": %ld}\n", streams, accepted, rejected, concealed, scan_first, cover);
    return 0;
}
