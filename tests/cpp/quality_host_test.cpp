// Stand-alone driver of csrc/quality_host.cpp for tests/test_quality_cpu.py: built with g++ -fsanitize=address,undefined together
// with that file.  The file named on the command line holds cases (tests/quality_cases.py, write_cases): int32 w, h, flags,
// ring_width, int64 gaze x, y, the test and the reference image (w * h uint32 each, in heap blocks of exactly that size, so that a
// read past an image is seen), the classes (w * h bytes) and the 1344 bytes of the expected record.  Every case runs with the
// classes and must give the expected bytes; it runs again without them (all UNIFORM), and with each invalid argument, which must be
// refused with the record untouched.  Prints "cases=N bad=M refused=R"; exit status 0 when M is 0.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/fovpt.h"

static const char* g_error = "";
void fovpt_internal_set_error(const char* text) { g_error = text ? "set" : ""; }      // (libfovpt's: the text of fovpt_last_error(NULL))

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int cases = 0, bad = 0, refused = 0;
    for (;;) {
        int32_t head[4];
        int64_t gaze[2];
        if (fread(head, sizeof(head), 1, f) != 1) break;
        if (fread(gaze, sizeof(gaze), 1, f) != 1) return 3;
        const int w = head[0], h = head[1];
        const size_t n = (size_t)w * (size_t)h;
        uint32_t* test = (uint32_t*)malloc(n * 4);
        uint32_t* ref = (uint32_t*)malloc(n * 4);
        uint8_t* cls = (uint8_t*)malloc(n);
        fovpt_quality_sums want, got;
        if (fread(test, 4, n, f) != n || fread(ref, 4, n, f) != n || fread(cls, 1, n, f) != n || fread(&want, sizeof(want), 1, f) != 1) return 3;
        fovpt_quality_config qc;
        memset(&qc, 0, sizeof(qc));
        qc.flags = head[2]; qc.ring_width = head[3];
        cases++;
        memset(&got, 0xa5, sizeof(got));
        if (fovpt_quality_host(test, ref, w, h, cls, gaze[0], gaze[1], &qc, &got) != FOVPT_OK || memcmp(&got, &want, sizeof(got)) != 0) {
            bad++;
            fprintf(stderr, "case %d (%d x %d, flags %d, ring_width %d): the record differs\n", cases, w, h, qc.flags, qc.ring_width);
        }
        // no classes: every pixel UNIFORM, the same totals
        fovpt_quality_sums uni;
        if (fovpt_quality_host(test, ref, w, h, nullptr, gaze[0], gaze[1], &qc, &uni) != FOVPT_OK) bad++;
        else {
            uint64_t px = 0, sq = 0, usq = 0;
            for (int k = 0; k < FOVPT_QUALITY_CLASSES; k++) {
                px += want.pixels[k];
                for (int c = 0; c < 3; c++) { sq += want.sq_err[k][c]; usq += uni.sq_err[k][c]; }
            }
            if (uni.pixels[FOVPT_QUALITY_UNIFORM] != px || px != n || usq != sq || memcmp(uni.ring_sq_err, want.ring_sq_err, sizeof(uni.ring_sq_err)) != 0) bad++;
        }
        // the scores of whatever came out: no trap, no out-of-range read
        volatile double sink = 0.0;
        const double wts[FOVPT_QUALITY_CLASSES] = {4.0, 2.0, 1.0, 1.0, 0.0};
        for (int k = -2; k <= FOVPT_QUALITY_CLASSES; k++) sink = sink + (fovpt_quality_mse(&got, k) + fovpt_quality_psnr(&got, k)) + fovpt_quality_ssim(&got, k);
        sink = sink + fovpt_quality_score(&got, wts) + fovpt_quality_score(nullptr, wts) + fovpt_quality_score(&got, nullptr);
        // refusals leave the record alone
        fovpt_quality_sums keep;
        memset(&keep, 0x5a, sizeof(keep));
        got = keep;
        fovpt_quality_config q2 = qc;
        int rc[9];
        rc[0] = fovpt_quality_host(nullptr, ref, w, h, cls, 0, 0, &qc, &got);
        rc[1] = fovpt_quality_host(test, nullptr, w, h, cls, 0, 0, &qc, &got);
        rc[2] = fovpt_quality_host(test, ref, 0, h, cls, 0, 0, &qc, &got);
        rc[3] = fovpt_quality_host(test, ref, w, -1, cls, 0, 0, &qc, &got);
        rc[4] = fovpt_quality_host(test, ref, w, h, cls, 0, 0, nullptr, &got);
        q2.flags = 4; rc[5] = fovpt_quality_host(test, ref, w, h, cls, 0, 0, &q2, &got); q2 = qc;
        q2.ring_width = 0; rc[6] = fovpt_quality_host(test, ref, w, h, cls, 0, 0, &q2, &got);
        q2.ring_width = FOVPT_QUALITY_MAX_RING_WIDTH + 1; rc[7] = fovpt_quality_host(test, ref, w, h, cls, 0, 0, &q2, &got); q2 = qc;
        q2._reserved[5] = 1; rc[8] = fovpt_quality_host(test, ref, w, h, cls, 0, 0, &q2, &got);
        for (int r : rc) { if (r == FOVPT_E_INVALID) refused++; else bad++; }
        const uint8_t was = cls[n - 1];
        cls[n - 1] = FOVPT_QUALITY_CLASSES;                                 // a class byte out of range
        if (fovpt_quality_host(test, ref, w, h, cls, 0, 0, &qc, &got) == FOVPT_E_INVALID) refused++; else bad++;
        cls[n - 1] = was;
        if (fovpt_quality_host(test, ref, w, h, cls, 0, 0, &qc, nullptr) == FOVPT_E_INVALID) refused++; else bad++;
        if (memcmp(&got, &keep, sizeof(got)) != 0) bad++;
        free(test); free(ref); free(cls);
    }
    fclose(f);
    printf("cases=%d bad=%d refused=%d error=%s\n", cases, bad, refused, g_error);
    return bad ? 1 : 0;
}
