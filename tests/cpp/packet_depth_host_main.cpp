// Test driver (tests/test_packet_depth_cpu.py::test_untrusted_depth_packets_under_sanitizers): csrc/packet_host.cpp compiled
// with g++ -fsanitize=address,undefined together with this file.  Every file on the command line holds depth packets, each
// behind its 4-byte length: the valid ones and the mutations and truncations the test made.  Each goes through
// fovpt_packet_check_depth and fovpt_packet_decode_depth_host from a heap block of exactly its length into a heap image of
// exactly the packet's size -- the sanitizers abort the process on any access outside either --, then `rounds` seeded randomly
// damaged copies of the packets that were valid do.  Every call must return FOVPT_OK or FOVPT_E_INVALID.  One line per file.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/fovpt.h"

static std::string g_err;
void fovpt_internal_set_error(const char* text) { g_err = text ? text : ""; }     // (lives in fovpt_api.hip / loader_host.cpp in the libraries)

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint32_t rnd()
{
    g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
    return (uint32_t)(g_rng >> 16);
}

static int g_bad = 0;

// -> the return code of fovpt_packet_check_depth
static int feed(const std::vector<unsigned char>& bytes, int w, int h)
{
    unsigned char* p = (unsigned char*)malloc(bytes.size() ? bytes.size() : 1);   // exactly the packet: one byte further is an error
    if (!bytes.empty()) memcpy(p, bytes.data(), bytes.size());
    const int rc = fovpt_packet_check_depth(p, bytes.size());
    if (rc != FOVPT_OK && rc != FOVPT_E_INVALID) { printf("check returned %d\n", rc); g_bad++; }
    // the output the caller expects -- or, where the header names another small size, that one, so that such packets decode too
    if (bytes.size() >= 192) {
        int32_t hw, hh;
        memcpy(&hw, p + 16, 4); memcpy(&hh, p + 20, 4);
        if (hw >= 1 && hw <= 256 && hh >= 1 && hh <= 256) { w = hw; h = hh; }
    }
    float* out = (float*)malloc((size_t)w * h * 4);
    memset(out, 0x5a, (size_t)w * h * 4);
    const int rd = fovpt_packet_decode_depth_host(p, bytes.size(), out, w, h);
    if (rd != FOVPT_OK && rd != FOVPT_E_INVALID) { printf("decode returned %d\n", rd); g_bad++; }
    if (rd == FOVPT_OK && rc != FOVPT_OK) { printf("decoded what check refused\n"); g_bad++; }
    // the colour decoder refuses every one of them
    if (fovpt_packet_check(p, bytes.size()) == FOVPT_OK && rc == FOVPT_OK) { printf("a depth packet passed the colour check\n"); g_bad++; }
    free(out);
    free(p);
    return rc;
}

int main(int argc, char** argv)
{
    const int rounds = argc > 1 ? atoi(argv[1]) : 0;
    for (int i = 2; i < argc; i++) {
        FILE* f = fopen(argv[i], "rb");
        if (!f) { printf("%s: cannot open\n", argv[i]); return 2; }
        std::vector<std::vector<unsigned char>> valid;
        int n = 0, ok = 0;
        uint32_t len;
        while (fread(&len, 4, 1, f) == 1) {
            std::vector<unsigned char> b(len);
            if (len && fread(b.data(), 1, len, f) != len) { printf("%s: short file\n", argv[i]); return 2; }
            int w = 1, h = 1;
            if (!valid.empty()) { int32_t v[2]; memcpy(v, valid[0].data() + 16, 8); w = v[0]; h = v[1]; }
            else if (len >= 192) { int32_t v[2]; memcpy(v, b.data() + 16, 8); if (v[0] >= 1 && v[0] <= 16384 && v[1] >= 1 && v[1] <= 16384) { w = v[0]; h = v[1]; } }
            n++;
            if (feed(b, w, h) == FOVPT_OK) { ok++; valid.push_back(b); }
        }
        fclose(f);
        int fuzz_ok = 0;
        for (int r = 0; r < rounds && !valid.empty(); r++) {
            std::vector<unsigned char> b = valid[rnd() % valid.size()];
            int32_t v[2];
            memcpy(v, b.data() + 16, 8);
            const int edits = 1 + (int)(rnd() % 3);
            for (int e = 0; e < edits; e++) {
                const uint32_t kind = rnd() % 6;
                const size_t at = (kind < 4 ? rnd() % 48 : rnd() % (b.size() / 4)) * 4;      // mostly the header
                uint32_t word;
                memcpy(&word, b.data() + at, 4);
                switch (rnd() % 6) {
                case 0: word ^= 1u << (rnd() % 32); break;
                case 1: word = rnd(); break;
                case 2: word += (rnd() % 9) - 4; break;
                case 3: word = 0; break;
                case 4: word = 0xffffffffu >> (rnd() % 32); break;
                default: word = (rnd() % 17) * 4; break;
                }
                memcpy(b.data() + at, &word, 4);
            }
            if (rnd() % 8 == 0) b.resize(rnd() % (b.size() + 1));
            if (feed(b, v[0], v[1]) == FOVPT_OK) fuzz_ok++;
        }
        printf("%s packets=%d valid=%d fuzzed=%d fuzzed_valid=%d bad=%d\n", argv[i], n, ok, rounds, fuzz_ok, g_bad);
    }
    return g_bad ? 1 : 0;
}
