// host_warp_harness.cpp — WARP's host twin (fmhip_host.cpp: warp_weight_table, warp_first_violator) as a stand-alone program, built
// with g++ -fsanitize=address,undefined by tests/test_host_warp.py.
//   host_warp_harness <vectors file>
// The file holds what the Python twin (tests/warp_ref.py) recorded, one record per line, floats as the hex of their fp32 bits:
//   W <M> <C> <W[0]> ... <W[C]>                                the weight table of M rows and C candidates
//   F <C> <margin> <s_pos> <N> <score 0> ... <score C-1>       the first violator of one pair
// Every record is recomputed into arrays of exactly its length — a read or write past their end is a sanitizer error — and must
// agree bit for bit.  Prints "checks ok <n>".
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "../sparkfm_amd/csrc/fmhip_host.h"

using namespace fmhip::host;

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            fprintf(stderr, "%s:%d: check failed: %s (record %ld)\n", __FILE__, __LINE__, #cond, n_read); \
            return 1;                                                                \
        }                                                                            \
    } while (0)

static bool read_f32(FILE *f, float *out, uint32_t *bits_out = nullptr) {
    uint32_t bits = 0;
    if (fscanf(f, "%" SCNx32, &bits) != 1) return false;
    memcpy(out, &bits, sizeof bits);
    if (bits_out) *bits_out = bits;
    return true;
}

static uint32_t bits_of(float x) {
    uint32_t b = 0;
    memcpy(&b, &x, sizeof b);
    return b;
}

int main(int argc, char **argv) {
    long n_read = 0, n_checked = 0;
    if (argc != 2) {
        fprintf(stderr, "usage: %s vectors\n", argv[0]);
        return 2;
    }
    FILE *f = fopen(argv[1], "r");
    CHECK(f != nullptr);
    char tag = 0;
    while (fscanf(f, " %c", &tag) == 1) {
        ++n_read;
        if (tag == 'W') {
            int64_t M = 0;
            int C = 0;
            CHECK(fscanf(f, "%" SCNd64 " %d", &M, &C) == 2);
            CHECK(M >= 2 && C >= 1 && C <= 64);
            std::unique_ptr<float[]> got(new float[(size_t)C + 1]);
            warp_weight_table(M, C, got.get());
            for (int n = 0; n <= C; ++n) {
                float want = 0.f;
                uint32_t wb = 0;
                CHECK(read_f32(f, &want, &wb));
                CHECK(bits_of(got[(size_t)n]) == wb);
            }
            CHECK(bits_of(got[0]) == 0u);
        } else {
            CHECK(tag == 'F');
            int C = 0, N = -1;
            float margin = 0.f, s_pos = 0.f;
            CHECK(fscanf(f, "%d", &C) == 1 && C >= 1 && C <= 64);
            CHECK(read_f32(f, &margin) && read_f32(f, &s_pos));
            CHECK(fscanf(f, "%d", &N) == 1 && N >= 0 && N <= C);
            std::unique_ptr<float[]> sc(new float[(size_t)C]);
            for (int c = 0; c < C; ++c) CHECK(read_f32(f, &sc[(size_t)c]));
            CHECK(warp_first_violator(sc.get(), C, s_pos, margin) == N);
            // the definition, restated: nothing before candidate N - 1 is above the threshold, candidate N - 1 is
            const float thr = s_pos - margin;
            for (int c = 0; c < (N ? N - 1 : C); ++c) CHECK(!(sc[(size_t)c] > thr));
            if (N) CHECK(sc[(size_t)N - 1] > thr);
        }
        ++n_checked;
    }
    fclose(f);
    CHECK(n_checked > 0);
    printf("checks ok %ld\n", n_checked);
    return 0;
}
