// The decode / validate / range-mask steps of ongym_spectrum_map (csrc/ongym_spectrum_core.hpp) on the CPU, over the doctored
// records and `active` values of tests/spectrum_cases.txt.  tests/test_spectrum_map_host.py builds this with
// -fsanitize=address,undefined and runs it: exit status 0 means every verdict is the table's and the sanitizers saw nothing.
//
//     spectrum_core_main tests/spectrum_cases.txt
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "ongym_spectrum_core.hpp"

using namespace ongym;

struct Dims { int P, M, S, C; };

static int failures = 0;
#define EXPECT(cond, name)                                                          \
    do {                                                                            \
        if (!(cond)) { std::printf("FAIL %s: %s\n", (name).c_str(), #cond); failures++; } \
    } while (0)

// the low mask word of a route: any function of the path will do here, the kernel reads the table's
static uint32_t route_mask(int path, int P) { return path >= 0 && path < P ? ((uint32_t)path * 2654435761u) | 1u : 0u; }

// bits [lo, hi) of word w, one bit at a time
static uint64_t naive_mask(int w, long long lo, long long hi) {
    uint64_t m = 0;
    for (int j = 0; j < 64; j++) {
        const long long s = 64ll * w + j;
        if (s >= lo && s < hi) m |= 1ull << j;
    }
    return m;
}

int main(int argc, char **argv) {
    if (argc != 2) { std::printf("usage: %s CASES\n", argv[0]); return 2; }
    std::ifstream in(argv[1]);
    if (!in) { std::printf("cannot read %s\n", argv[1]); return 2; }
    std::map<std::string, Dims> dims;
    int recs = 0, acts = 0, well = 0;
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ss(line);
        std::string kind, name, codec;
        if (!(ss >> kind) || kind[0] == '#') continue;
        if (kind == "dims") {
            Dims d;
            ss >> codec >> d.P >> d.M >> d.S >> d.C;
            dims[codec] = d;
        } else if (kind == "rec") {
            long long path, slot, n, mod;
            std::string xorhex, verdict;
            ss >> name >> codec >> path >> slot >> n >> mod >> xorhex >> verdict;
            if (!ss || !dims.count(codec)) { std::printf("bad line: %s\n", line.c_str()); return 2; }
            const Dims d = dims[codec];
            const bool r32 = codec == "r32";
            const uint32_t mask = route_mask((int)path, d.P), x = (uint32_t)std::strtoul(xorhex.c_str(), nullptr, 16);
            uint32_t a, b;
            if (r32) { a = mask ^ x; b = (uint32_t)slot | ((uint32_t)n << 10) | ((uint32_t)mod << 20) | ((uint32_t)path << 23); }
            else { a = (uint32_t)path | ((uint32_t)slot << 16); b = (uint32_t)n | ((uint32_t)mod << 16); }
            const SpectrumRec r = spectrum_decode(r32, a, b);
            EXPECT(r.path == path && r.slot == slot && r.n == n && r.mod == mod, name);     // the table's fields fit the codec
            bool ok = spectrum_fields_ok(r, d.P, d.M, d.S);
            if (ok) ok = spectrum_mask_ok(r32, a, (uint64_t)route_mask(r.path, d.P) | 0xABCD00000000ull);   // only after the range check
            EXPECT(ok == (verdict == "ok"), name);
            const int W = (d.S + 63) / 64;
            for (int w = -3; w < W + 3; w++)                                             // any range, any word
                EXPECT(spectrum_word_mask(w, r.slot, r.slot + r.n + 1) == naive_mask(w, r.slot, (long long)r.slot + r.n + 1), name);
            if (ok) {
                const int lo = r.slot, hi = spectrum_claim_end(r, d.S);
                EXPECT(0 <= lo && lo < hi && hi <= d.S && (hi - 1) / 64 < W, name);
                EXPECT(hi == (r.slot + r.n < d.S ? r.slot + r.n + 1 : d.S), name);
                int cells = 0;
                for (int w = 0; w < W; w++) {
                    const uint64_t m = spectrum_word_mask(w, lo, hi);
                    EXPECT(m == naive_mask(w, lo, hi), name);
                    EXPECT((m & ~spectrum_word_mask(w, 0, d.S)) == 0, name);             // nothing at or above S
                    cells += __builtin_popcountll(m);
                }
                EXPECT(cells == hi - lo, name);
                well++;
            }
            recs++;
        } else if (kind == "act") {
            long long active, A, violation;
            ss >> name >> active >> A >> violation;
            if (!ss || !dims.count("r32")) { std::printf("bad line: %s\n", line.c_str()); return 2; }
            const int C = dims["r32"].C, got = spectrum_active((int)active, C);
            EXPECT(got == A && 0 <= got && got <= C, name);
            EXPECT((got != (int)active) == (violation != 0), name);
            acts++;
        } else {
            std::printf("bad line: %s\n", line.c_str());
            return 2;
        }
    }
    // the row masks at every pair of bounds of a short and of the longest row
    for (int S : {1, 63, 64, 65, 100, 1023})
        for (int lo = 0; lo <= S; lo += (S > 128 ? 37 : 1))
            for (int hi = lo; hi <= S; hi += (S > 128 ? 41 : 1))
                for (int w = 0; w < (S + 63) / 64; w++)
                    if (spectrum_word_mask(w, lo, hi) != naive_mask(w, lo, hi)) { std::printf("FAIL mask %d %d %d\n", w, lo, hi); failures++; }
    if (failures || !recs || !acts || !well) { std::printf("%d failures\n", failures); return 1; }
    std::printf("spectrum core ok: %d records (%d well-formed), %d active values\n", recs, well, acts);
    return 0;
}
